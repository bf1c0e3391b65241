// abi_internal.hpp -- what the files that define the extern "C" surface (abi_*.cpp, stream.cpp, multi.cpp) share: the guards of
// an entry point, and the few helpers and options that one of them defines and another uses.  Nothing throws across the C ABI.
#pragma once

#include "../../include/pygmm_hip.h"

#include "batch.hpp"
#include "common.hpp"

#include <atomic>
#include <memory>

// ---- guards: park the message, never unwind into C ----
#define SR_TRY try {                                                     \
    std::lock_guard<std::recursive_mutex> _api_lock(api_mutex());
#define SR_CATCH(ret)                          \
    }                                          \
    catch (const std::exception &e) {          \
        set_error("%s", e.what());             \
        return ret;                            \
    }                                          \
    catch (...) {                              \
        set_error("unknown C++ exception");    \
        return ret;                            \
    }
#define SR_CATCH_VOID                                          \
    }                                                          \
    catch (const std::exception &e) {                          \
        set_error("%s", e.what());                             \
        fprintf(stderr, "pygmm.so: %s\n", e.what());           \
        return;                                                \
    }                                                          \
    catch (...) {                                              \
        set_error("unknown C++ exception");                    \
        return;                                                \
    }

namespace sr {

// abi_batch.cpp: host rows -> a feature batch on the current device
std::unique_ptr<SRBatch> feature_batch(const float *X, int64_t n, int dim, const int64_t *offsets, int n_utt);

// the n_cu argument of an sr_*_plan entry point: <= 0 asks for the current device's
inline int plan_n_cu(int n_cu) {
    if (n_cu <= 0) {
        ensure_device();
        n_cu = ctx().n_cu;
    }
    return n_cu;
}

}  // namespace sr

std::atomic<int> &stream_debug_capture_delay_ms();      // stream.cpp
std::atomic<int> &multi_merge_option();                 // multi.cpp
