// abi_options.cpp -- sr_set_option and the readers of what the last calls did.
#include "abi_internal.hpp"

#include "bw_plan.hpp"
#include "bw_stats.hpp"
#include "calib.hpp"
#include "calib_plan.hpp"
#include "diar.hpp"
#include "diar_plan.hpp"
#include "em.hpp"
#include "featnorm.hpp"
#include "featnorm_plan.hpp"
#include "fork_proxy.hpp"
#include "gmm_full.hpp"
#include "jfa.hpp"
#include "jfa_plan.hpp"
#include "kmeans_init.hpp"
#include "map_batch.hpp"
#include "map_plan.hpp"
#include "mfcc.hpp"
#include "norm_plan.hpp"
#include "plda.hpp"
#include "plda_plan.hpp"
#include "score.hpp"
#include "score_norm.hpp"
#include "silence.hpp"
#include "silence_plan.hpp"
#include "topc.hpp"
#include "topc_plan.hpp"
#include "xvector.hpp"
#include "xvector_plan.hpp"

#include <string>

using namespace sr;

// a module's scratch bound in MiB: one range and one message for all of them
static void set_scratch_mib(const char *key, long value, int64_t default_bytes, void (*set)(long)) {
    if (value < 1 || value > (1L << 20)) fail("%s must be within 1 .. %ld (the default is %ld)", key, 1L << 20, (long)(default_bytes >> 20));
    set(value);
}

extern "C" {

int sr_set_option(const char *key, long value) {
    SR_TRY
    if (!key) fail("null key");
    const std::string k(key);
    if (k == "score_frames_per_lane") {
        if (value != 0 && value != 1 && value != 2 && value != 4) fail("frames per lane must be 0/1/2/4");
        score_options().frames_per_lane = (int)value;
    } else if (k == "score_model_groups") {
        score_options().model_groups = (int)value;
    } else if (k == "score_packed") {
        score_options().packed = (int)value;
    } else if (k == "score_engine") {
        if (value < 0 || value > 6 || value == 2)
            fail("score_engine must be 0 (auto), 1 (vector ALU), 3 (split-bf16 matrix cores), 4 (split-bf16, shared-sigma form), "
                 "5 (split-fp16 matrix cores) or 6 (split-fp16, shared-sigma form); 2 was the fp32 matrix-core engine, removed in round 5 "
                 "(never selected: 1.45-1.8x slower than split-bf16 at the same accuracy)");
        score_options().engine = (int)value;
    } else if (k == "score_h2s_shape") {
        if (value < 0 || value > 6)
            fail("score_h2s_shape must be 0 (automatic), 1 (4-wave workgroups), 2 (12-wave workgroups), 3 (12 waves, image loop pipelined inside the wave), "
                 "4 (4 waves on one tile, the block's models split between them), 5 (as 3, on the flat image where 3 takes the compact one) "
                 "or 6 (as 3, one quadratic half per block where 3 forms one per two blocks)");
        score_options().h2s_shape = (int)value;
    } else if (k == "flush_list_cap") {
        if (value < 0) fail("flush_list_cap must be >= 0");
        score_options().flush_list_cap = (int)value;
    } else if (k == "score_h2s_pack_tails") {
        if (value != 0 && value != 1) fail("score_h2s_pack_tails must be 0 or 1");
        score_options().h2s_pack_tails = (int)value;
    } else if (k == "score_h2s_force_exc") {
        score_options().h2s_force_exc = value != 0;
    } else if (k == "score_split_shape") {
        if (value != 0 && value != 1 && value != 8 && value != 12 && value != 16)
            fail("score_split_shape must be 0 (automatic), 1 (4-wave workgroups) or 8 / 12 / 16 (waves of the wide, pipelined form)");
        score_options().split_shape = (int)value;
    } else if (k == "score_mfma_ft") {
        if (value < 0 || value > 4) fail("score_mfma_ft must be 0..4");
        score_options().mfma_ft = (int)value;
    } else if (k == "flush_order") {
        if (value != 1 && value != 2)
            fail("flush_order must be 2 (partial products as the reference DSO's compiler forms them: even / odd dimensions) or "
                 "1 (the source's order, gmm.cc:192-195)");
        flush_order_option() = (int)value;
    } else if (k == "kmeans_assign_engine") {
        if (value != 0 && value != 1) fail("kmeans_assign_engine must be 0 (fast full search, exact pass for what it cannot decide) or 1 (exact pass only)");
        set_kmeans_assign_engine((int)value);
    } else if (k == "reference_side_effects") {
        if (value != 0 && value != 1) fail("reference_side_effects must be 0 or 1");
        set_reference_side_effects((int)value);
    } else if (k == "em_stats_engine") {
        if (value < 0 || value > 3)
            fail("em_stats_engine must be 0 (automatic), 1 (vector ALU), 2 (fp64 matrix cores, responsibilities on the vector ALU) or "
                 "3 (automatic, an iteration per launch: no whole-fit kernel)");
        set_em_stats_engine((int)value);
    } else if (k == "multi_merge_same_device") {
        multi_merge_option().store(value != 0);
    } else if (k == "multi_numa_bind") {
        if (value != 0 && value != 1) fail("multi_numa_bind must be 0 or 1");
        numa_bind_option().store((int)value);
    } else if (k == "debug_capture_delay_ms") {
        if (value < 0 || value > 1000) fail("debug_capture_delay_ms must be 0 .. 1000");
        stream_debug_capture_delay_ms().store((int)value);         // test hook (tests/test_gpu_pipeline.py)
    } else if (k == "debug_em_small_absent_workgroup") {
        if (value != 0 && value != 1) fail("debug_em_small_absent_workgroup must be 0 or 1");
        set_em_small_test_absent((int)value);                       // test hook (tests/test_gpu_em_small.py): a workgroup of the whole-fit kernel stays away from a barrier
    } else if (k == "debug_verify_clean_counters") {
        if (value != 0 && value != 1) fail("debug_verify_clean_counters must be 0 or 1");
        score_options().verify_clean_counters = (int)value;        // test hook (tests/test_gpu_interleave.py): checked in score_device
    } else if (k == "debug_helper_max_models") {
        if (value < 0) fail("debug_helper_max_models must be >= 0 (0: the default)");
        fork_proxy_set_max_models(value);                           // test hook (tests/test_gpu_fork.py): applies in the helper, where it is forwarded
    } else if (k == "topc_scratch_mib") {
        set_scratch_mib(key, value, TOPC_DEFAULT_SCRATCH, set_topc_scratch_mib);
    } else if (k == "bw_scratch_mib") {
        set_scratch_mib(key, value, BW_DEFAULT_SCRATCH, set_bw_scratch_mib);
    } else if (k == "bw_range_frames") {
        if (value < 0 || value > (long)BW_MAX_RANGE_FRAMES) fail("bw_range_frames must be 0 (automatic) or 1 .. %ld frames", (long)BW_MAX_RANGE_FRAMES);
        set_bw_range_frames(value);
    } else if (k == "jfa_scratch_mib") {
        set_scratch_mib(key, value, JFA_DEFAULT_SCRATCH, set_jfa_scratch_mib);
    } else if (k == "norm_scratch_mib") {
        set_scratch_mib(key, value, NORM_DEFAULT_SCRATCH, set_norm_scratch_mib);
    } else if (k == "calib_scratch_mib") {
        set_scratch_mib(key, value, CALIB_DEFAULT_SCRATCH, set_calib_scratch_mib);
    } else if (k == "diar_scratch_mib") {
        set_scratch_mib(key, value, DIAR_DEFAULT_SCRATCH, set_diar_scratch_mib);
    } else if (k == "plda_scratch_mib") {
        set_scratch_mib(key, value, PLDA_DEFAULT_SCRATCH, set_plda_scratch_mib);
    } else if (k == "xvector_scratch_mib") {
        set_scratch_mib(key, value, XV_DEFAULT_SCRATCH, set_xvector_scratch_mib);
    } else if (k == "debug_xvector_mfma_shape") {
        if (value != 0 && value != 1) fail("debug_xvector_mfma_shape must be 0 (v_mfma_f32_32x32x16_bf16, what the library runs) or 1 (v_mfma_f32_16x16x32_bf16)");
        set_xvector_mfma_shape((int)value);                         // timing hook (scripts/time_xvector.py): the shape not chosen, kept to be measured against
    } else if (k == "jfa_lds_rows") {
        std::string why;
        if (!dense_check_lds_rows(value, why)) fail("%s rows", why.c_str());
        set_jfa_lds_rows(value);
    } else if (k == "full_fit_batch_bytes") {
        if (value < 1) fail("full_fit_batch_bytes must be >= 1 (the default is %ld)", 1L << 30);
        set_full_fit_batch_bytes(value);
    } else if (k == "map_fit_batch_bytes") {
        if (value < 1) fail("map_fit_batch_bytes must be >= 1 (the default is %ld)", (long)MAP_DEFAULT_SCRATCH);
        set_map_fit_batch_bytes(value);
    } else if (k == "silence_block") {
        if (value < 0 || value > SILENCE_MAX_REL) fail("silence_block must be 0 (automatic) or 1 .. 2^30 positions per block");
        set_silence_block(value);
    } else if (k == "norm_tile") {
        if (value < 0 || value > FEATNORM_MAX_TILE || value % FEATNORM_WAVE != 0)
            fail("norm_tile must be 0 (automatic) or a multiple of 64 up to 1024 frames per workgroup");
        set_feature_norm_tile(value);
    } else if (k == "mfcc_generic") {
        mfcc_set_force_generic(value != 0);
    } else if (k == "mfcc_precision") {
        if (value != 0 && value != 2)
            fail("mfcc_precision must be 2 (float64 spectrum, ln and DCT for every frame: the reference's arithmetic, MFCC.py:59-70) or "
                 "0 (fp32 throughout: ~1.5x faster, features up to 2e-2 off on voices whose mel bands lie > 60 dB apart)");
        mfcc_set_precision((int)value);
    } else {
        fail("unknown option '%s'", key);
    }
    fork_proxy_note_option(key, value);
    return 0;
    SR_CATCH(-1)
}

const char *sr_last_score_kernel(void) { return last_score_kernel(); }
int sr_last_em_stats_engine(void) { return sr::last_em_stats_engine(); }

void sr_flush_stats(long *calls, long *pairs, long *frames) { flush_stats(calls, pairs, frames); }

void sr_kmeans_fast_stats(long *passes, long *rechecked) { kmeans_fast_stats(passes, rechecked); }

}  // extern "C"
