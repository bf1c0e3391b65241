// gmm_model.hpp -- host-side model objects behind the C ABI handles: a model (GMM) and a device-resident speaker set
// (SRModelSet).  The reference's text model format is model_text.hpp, the packing of mixture parameters into the layouts the
// scoring kernels stream through LDS model_pack.hpp, the fp16 / bf16 part splits fp_parts.hpp.
#pragma once

#include "common.hpp"
#include "fp_parts.hpp"
#include "model_pack.hpp"
#include "model_text.hpp"

#include <atomic>
#include <memory>
#include <string>
#include <vector>

struct SRModelSet;

// The handle type of the C ABI (`GMM *`).  Reference: class GMM, src/gmm/src/gmm.hh:130-173;
// per-Gaussian mean/sigma (sigma = STANDARD DEVIATIONS) as gmm.hh:24-46.
namespace sr {
inline uint64_t next_gmm_uid() {
    static std::atomic<uint64_t> next{1};
    return next.fetch_add(1);
}
}  // namespace sr

struct GMM {
    int nr_mixtures = 0;
    int covariance_type = 1;  // COVTYPE_DIAGONAL, gmm.hh:18-22
    int dim = 0;
    std::vector<double> weights;  // [K]
    std::vector<double> mean;     // [K*D]
    std::vector<double> sigma;    // [K*D]
    // lazily packed one-model sets, one per device (threads on different GPUs may score the same handle concurrently:
    // each holds its device's lock only); invalidated by training.  (mutable: a cache -- a UBM handed to the MAP trainer as
    // `const` lends its packed set to every speaker's first E-step, em.hip)
    mutable std::shared_ptr<SRModelSet> single[sr::MAX_DEVICES];
    // identity of the PARAMETERS for caches that hold several models (sr_score_models_f32): `uid` is unique per object for the life
    // of the process (an address can come back), `generation` moves whenever the parameters change (every writer calls drop_single)
    uint64_t uid = sr::next_gmm_uid();
    uint64_t generation = 0;
    void drop_single() {
        for (auto &s : single) s.reset();
        generation++;
    }
    bool trained() const { return dim > 0 && (int)weights.size() == nr_mixtures; }
};

// Device-resident speaker set (C ABI handle `SRModelSet *`).
struct SRModelSet {
    sr::PackedModels host;
    sr::DevBuf<float> d_params, d_center0;     // vector layout and its centre
    sr::DevBuf<sr::ChunkDesc> d_chunks;
    sr::PackedSplit bx3;             // split-bf16 layout for the bf16 matrix-core engine
    sr::DevBuf<uint16_t> d_bx3_params;
    sr::DevBuf<float> d_bx3_center;
    sr::DevBuf<sr::ChunkDesc> d_bx3_chunks;
    std::vector<char> chunks_image;  // (em.hip) the bytes d_chunks holds: a re-packed model of the same shape has the same chunk table
    bool bx3_stale = false;          // a re-packed set (em.hip: a fit recycles its sets): ensure_bx3_layout fills the standing buffers again
    sr::PackedSplit h2;              // two-part fp16 layout (three part products)
    sr::DevBuf<uint16_t> d_h2_params;
    sr::DevBuf<float> d_h2_center, d_h2_scale;
    sr::DevBuf<sr::ChunkDesc> d_h2_chunks;
    sr::PackedBx3Shared shared;      // shared-sigma layout (empty unless the set qualifies)
    sr::DevBuf<uint16_t> d_shared_params;
    sr::DevBuf<sr::SharedBlock> d_shared_blocks;
    sr::DevBuf<float> d_shared_center;
    sr::PackedH2Shared h2s;          // shared-sigma layout on two fp16 parts (empty unless the set qualifies)
    sr::DevBuf<uint16_t> d_h2s_params, d_h2s_qdesc, d_h2s_ldesc, d_h2s_ref_params;
    sr::DevBuf<sr::SharedBlock> d_h2s_blocks;
    sr::DevBuf<float> d_h2s_center, d_h2s_scale, d_h2s_ref_center, d_h2s_ref_scale;
    sr::DevBuf<sr::ChunkDesc> d_h2s_ref_chunks;
    sr::DevBuf<int> d_h2s_ref_gcb;
    // ... and its compact order (PackedH2Compact), packed and uploaded on the first pass that takes the pipelined kernel
    // (0 not looked at yet, -1 the form does not apply to this set, 1 on the device)
    int h2c_state = 0;
    int h2c_nk = 0;
    sr::DevBuf<uint16_t> d_h2c_params, d_h2c_qdesc, d_h2c_ldesc;
    sr::DevBuf<sr::SharedBlock> d_h2c_blocks;
    // Hybrid form of an ill-conditioned set (score.hpp): the mixtures whose expanded form would cancel in fp32 (tight and
    // far from the centre) as one sub-set on the direct-form vector engine, the rest as another on the matrix cores;
    // the two per-frame log-likelihoods are merged by a log-add-exp.  Empty unless the set needed it.
    // Model-group tables (chunk / block index per group) of recent scoring calls and their device copies: the number of groups
    // follows the batch's size, and a caller that alternates between sizes (the pieces of sr_multi_predict_pcm) must not re-upload
    // -- and synchronise the stream -- on every call.  A handful of entries, oldest replaced.
    struct GroupTable {
        std::vector<int> host;
        sr::DevBuf<int> dev;
    };
    std::vector<std::unique_ptr<GroupTable>> group_tables;
    size_t group_table_next = 0;
    // top-C scoring (gmm_topc.hip), 0 not looked at yet, -1 the set does not qualify, 2 it does, 1 it does and its tables
    // (packed from the vector layout on first use) stand on the device
    int topc_state = 0;
    sr::DevBuf<float> d_topc_scale;  // [K][TP] the shared s_kd, zero-padded
    sr::DevBuf<float> d_topc_m;      // [K][TP][S] every model's m_skd (a lane per model reads consecutive floats)
    sr::DevBuf<float> d_topc_c;      // [K] the shared constants
    sr::DevBuf<float> d_topc_bg;     // [K][TP][2] {s, m} of the background column `topc_bg`, gathered per call when it changes
    int topc_bg = -1, topc_tp = 0, topc_k = 0;
    sr::DevBuf<int> d_flush_models;  // per model {first record, records} of the vector layout (gmm_flush.hip; built on first use)
    std::unique_ptr<SRModelSet> hy_good, hy_bad;
    int hy_bad_mixtures = 0;         // mixtures of the set's largest model that went to the vector engine
    int device = -1;
};
