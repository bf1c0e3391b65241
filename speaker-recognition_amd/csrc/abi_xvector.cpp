// abi_xvector.cpp -- speaker embeddings from a neural network the caller brings (xvector.hip): the network's handle, its plan, and
// the forward pass over a resident feature batch or over host rows.  Every argument is checked before the device is touched; the
// network's weights go to the device with the first forward pass, so that creating one needs no device.
#include "abi_internal.hpp"

#include "xvector.hpp"
#include "xvector_plan.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace sr;

namespace {

std::vector<XvLayer> layers_from(const char *what, int n_layers, const int32_t *desc, const double *var_floor) {
    if (!desc) fail("%s: null argument (the layer descriptors)", what);
    if (n_layers < 1 || n_layers > XV_MAX_LAYERS) fail("%s: %d layers; 2 .. %d", what, n_layers, XV_MAX_LAYERS);
    std::vector<XvLayer> layers((size_t)n_layers);
    for (int l = 0; l < n_layers; l++) {
        const int32_t *d = desc + (size_t)l * XV_DESC;
        if (d[5] < 0 || d[5] > XV_MAX_OFFSETS) fail("%s: layer %d: %d offsets; 1 .. %d", what, l, d[5], XV_MAX_OFFSETS);
        layers[(size_t)l] = xv_layer_from_desc(d, var_floor ? var_floor[l] : 0.0);
    }
    return layers;
}

// the call's segment table: the caller's, checked, or one segment per utterance
std::vector<int32_t> segments_of(const char *what, const XvModelInfo &m, const std::vector<int64_t> &offsets, int n_utt, const int32_t *segs, int64_t n_seg) {
    std::vector<int32_t> table;
    if (segs) {
        table.assign(segs, segs + 3 * n_seg);
    } else {
        for (int u = 0; u < n_utt; u++) {
            const int64_t T = offsets[(size_t)u + 1] - offsets[(size_t)u];
            if (T > INT32_MAX) fail("%s: utterance %d holds %lld frames; pass a segment table of shorter windows", what, u, (long long)T);
            table.push_back(u);
            table.push_back(0);
            table.push_back((int32_t)T);
        }
    }
    std::string why;
    if (!xv_check_segments(m, offsets.data(), n_utt, table.data(), (int64_t)table.size() / 3, why)) fail("%s: %s", what, why.c_str());
    return table;
}

// what a forward pass needs from the host, every refusal made: the segment table, the plan over it, the output's size
struct Prepared {
    std::vector<int32_t> table;
    XvPlan plan;
};

Prepared prepare(const char *what, const SRXvector &net, int dim, const std::vector<int64_t> &offsets, int n_utt, const int32_t *segs, int64_t n_seg,
                 int tap, int tap_bf16, const float *out, int64_t out_cap) {
    if (dim != net.info.input_dim)
        fail("%s: the features are %d wide, the network's first layer takes %d; extract the features the network was trained on", what, dim,
             net.info.input_dim);
    if (segs && n_seg < 0) fail("%s: %lld segments", what, (long long)n_seg);
    Prepared p;
    p.table = segments_of(what, net.info, offsets, n_utt, segs, n_seg);
    const int64_t n = (int64_t)p.table.size() / 3;
    std::vector<int64_t> lengths((size_t)n);
    for (int64_t i = 0; i < n; i++) lengths[(size_t)i] = p.table[(size_t)(3 * i + 2)];
    std::string why;
    if (!plan_xvector(net.layers.data(), net.info.n_layers, lengths.data(), n, tap, tap_bf16 != 0, (int64_t)xvector_scratch_mib() << 20, p.plan, why))
        fail("%s: %s", what, why.c_str());
    if (p.plan.out_rows * p.plan.out_cols > out_cap)
        fail("%s: the result is [%lld, %d], the output holds %lld floats", what, (long long)p.plan.out_rows, p.plan.out_cols, (long long)out_cap);
    if (n > 0 && !out) fail("%s: null output", what);
    if (gpu_runtime_lost()) fail_gpu_runtime_lost(what);
    return p;
}

}  // namespace

extern "C" {

SRXvector *sr_xvector_create(int n_layers, const int32_t *desc, const double *var_floor, const float *const *W, const float *const *b,
                             const float *const *scale, const float *const *shift) {
    SR_TRY
    const std::vector<XvLayer> layers = layers_from("sr_xvector_create", n_layers, desc, var_floor);
    return xvector_create(layers.data(), n_layers, W, b, scale, shift);
    SR_CATCH(nullptr)
}

void sr_xvector_free(SRXvector *net) { delete net; }

int sr_xvector_info(SRXvector *net, int32_t *out, int n_out) {
    SR_TRY
    if (!net || !out) fail("sr_xvector_info: null argument");
    if (n_out < 12) fail("sr_xvector_info writes 12 fields");
    const XvModelInfo &m = net->info;
    const int32_t v[12] = {m.n_layers, m.pool, m.input_dim, m.embedding_dim, m.context, XV_TM, XV_TN, XV_KC, XV_GRAN, XV_LDS_BYTES, XV_WG, net->device};
    std::copy(v, v + 12, out);
    return 12;
    SR_CATCH(-1)
}

int sr_xvector_plan(int n_layers, const int32_t *desc, const double *var_floor, const int64_t *lengths, int64_t n_seg, int tap, int tap_bf16,
                    int64_t scratch_bytes, int64_t *out, int n_out, int32_t *width_pad_out, int64_t *rows_out, int64_t *chunk_begin_out,
                    int64_t *tile_count_out, int tile_layer, int64_t tile_chunk, int32_t *tiles_out, int64_t tiles_cap) {
    SR_TRY
    if (!out) fail("sr_xvector_plan: null argument");
    if (n_out < 16) fail("sr_xvector_plan writes 16 fields");
    const std::vector<XvLayer> layers = layers_from("sr_xvector_plan", n_layers, desc, var_floor);
    if (scratch_bytes <= 0) scratch_bytes = (int64_t)xvector_scratch_mib() << 20;
    XvPlan p;
    std::string why;
    if (!plan_xvector(layers.data(), n_layers, lengths, n_seg, tap, tap_bf16 != 0, scratch_bytes, p, why)) fail("sr_xvector_plan: %s", why.c_str());
    const XvModelInfo &m = p.info;
    const int64_t n_chunks = (int64_t)p.chunks.size();
    int64_t worst = 0;
    for (const XvChunk &c : p.chunks) worst = std::max(worst, c.bytes);
    const int64_t v[16] = {XV_TM, XV_TN, XV_KC, XV_GRAN, m.context, m.embedding_dim, n_chunks, XV_LDS_BYTES, m.pool, p.last, p.out_rows, p.out_cols,
                           p.buf_bytes[0], p.buf_bytes[1], worst, scratch_bytes};
    std::copy(v, v + 16, out);
    if (width_pad_out) std::copy(m.width_pad.begin(), m.width_pad.end(), width_pad_out);
    if (rows_out)
        for (int s = 0; s <= n_layers; s++)
            for (int64_t i = 0; i < n_seg; i++) rows_out[(size_t)s * (size_t)n_seg + (size_t)i] = xv_stage_rows(m, lengths[i], s);
    if (chunk_begin_out) {
        for (int64_t c = 0; c < n_chunks; c++) chunk_begin_out[c] = p.chunks[(size_t)c].seg_begin;
        chunk_begin_out[n_chunks] = n_seg;
    }
    std::vector<XvTile> tiles;
    if (tile_count_out)
        for (int l = 0; l < n_layers; l++)
            for (int64_t c = 0; c < n_chunks; c++) {
                tiles.clear();
                if (l != m.pool && l <= p.last) xv_layer_tiles(m, lengths, p.chunks[(size_t)c].seg_begin, p.chunks[(size_t)c].seg_end, l, tiles);
                tile_count_out[(size_t)l * (size_t)n_chunks + (size_t)c] = (int64_t)tiles.size();
            }
    if (tiles_out) {
        if (tile_layer < 0 || tile_layer >= n_layers || tile_layer == m.pool || tile_chunk < 0 || tile_chunk >= n_chunks)
            fail("sr_xvector_plan: no tile list for layer %d of chunk %lld", tile_layer, (long long)tile_chunk);
        xv_layer_tiles(m, lengths, p.chunks[(size_t)tile_chunk].seg_begin, p.chunks[(size_t)tile_chunk].seg_end, tile_layer, tiles);
        if ((int64_t)tiles.size() > tiles_cap) fail("sr_xvector_plan: %lld tiles, the output holds %lld", (long long)tiles.size(), (long long)tiles_cap);
        for (size_t t = 0; t < tiles.size(); t++) {
            tiles_out[3 * t] = tiles[t].seg;
            tiles_out[3 * t + 1] = tiles[t].first;
            tiles_out[3 * t + 2] = tiles[t].rows;
        }
    }
    return (int)std::min<int64_t>(n_chunks, INT32_MAX);
    SR_CATCH(-1)
}

int sr_xvector_extract_batch(SRXvector *net, SRBatch *features, const int32_t *segs, int64_t n_seg, int tap, int tap_bf16, float *out,
                             int64_t out_cap, double *times_ms_out) {
    SR_TRY
    if (!net || !features) fail("sr_xvector_extract_batch: null argument");
    if (features->kind != SRBatch::FEATURES) fail("sr_xvector_extract_batch takes a feature batch");
    const Prepared p = prepare("sr_xvector_extract_batch", *net, features->dim, features->offsets, features->n_utt, segs, n_seg, tap, tap_bf16, out, out_cap);
    xvector_forward(*net, *features, p.table.data(), p.plan, tap_bf16 != 0, out, times_ms_out);
    return 0;
    SR_CATCH(-1)
}

int sr_xvector_extract(SRXvector *net, const float *X, int64_t n_rows, int dim, const int64_t *offsets, int n_utt, const int32_t *segs,
                       int64_t n_seg, int tap, int tap_bf16, float *out, int64_t out_cap, double *times_ms_out) {
    SR_TRY
    if (!net || !offsets || (n_rows > 0 && !X)) fail("sr_xvector_extract: null argument");
    if (n_utt < 0 || n_rows < 0 || dim < 1) fail("sr_xvector_extract: %d utterances, %lld rows of %d", n_utt, (long long)n_rows, dim);
    if (offsets[0] != 0 || offsets[n_utt] != n_rows) fail("sr_xvector_extract: the offsets must run from 0 to the %lld rows", (long long)n_rows);
    for (int u = 0; u < n_utt; u++)
        if (offsets[u + 1] < offsets[u]) fail("sr_xvector_extract: the offsets must not descend (utterance %d)", u);
    if (dim == net->info.input_dim)      // (another width is refused by name below; its rows are not read)
        for (int64_t i = 0; i < n_rows * dim; i++)
            if (!std::isfinite(X[i]))
                fail("sr_xvector_extract: the features hold a non-finite value at row %lld, column %lld; clean them first", (long long)(i / dim),
                     (long long)(i % dim));
    // the segment table and the plan against the host offsets: every refusal before the batch is uploaded
    const Prepared p = prepare("sr_xvector_extract", *net, dim, std::vector<int64_t>(offsets, offsets + n_utt + 1), n_utt, segs, n_seg, tap, tap_bf16, out,
                               out_cap);
    std::unique_ptr<SRBatch> feat = feature_batch(X, n_rows, dim, offsets, n_utt);
    xvector_forward(*net, *feat, p.table.data(), p.plan, tap_bf16 != 0, out, times_ms_out);
    return 0;
    SR_CATCH(-1)
}

}  // extern "C"
