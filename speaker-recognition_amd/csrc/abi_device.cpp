// abi_device.cpp -- the last error, devices and NUMA placement, the profile counters and the probes.
#include "abi_internal.hpp"

using namespace sr;

extern "C" {

const char *sr_last_error(void) { return last_error().c_str(); }

int sr_gpu_runtime_lost(void) { return gpu_runtime_lost() ? 1 : 0; }

int sr_device_count(void) { return visible_devices(); }

// No api lock here: these only move the calling thread between devices.
int sr_set_device(int device) {
    try {
        set_default_device(device);
        return 0;
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

int sr_set_thread_device(int device) {
    try {
        set_thread_device(device);
        return 0;
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

int sr_get_device(void) { return current_device(); }

int sr_device_synchronize(void) {
    SR_TRY
    ensure_device();
    SR_HIP(hipDeviceSynchronize());
    return 0;
    SR_CATCH(-1)
}

int sr_device_name(char *buf, int buflen) {
    SR_TRY
    ensure_device();
    hipDeviceProp_t prop;
    SR_HIP(hipGetDeviceProperties(&prop, ctx().device));
    snprintf(buf, (size_t)buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return 0;
    SR_CATCH(-1)
}

int sr_device_numa_node(int device) {
    try {
        return device_numa_node(device);
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

int sr_bind_thread_near_device(int device) {
    try {
        return bind_thread_near_device(device);
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return -1;
    }
}

int sr_hbm_copy_gbps(size_t bytes, int iters, double *gbps_out) {
    SR_TRY
    if (!gbps_out || bytes == 0 || iters <= 0) fail("bad arguments to sr_hbm_copy_gbps");
    ensure_device();
    DevBuf<char> a(bytes), b(bytes);
    SR_HIP(hipMemsetAsync(a.p, 1, bytes, ctx().stream));
    hipEvent_t e0, e1;
    SR_HIP(hipEventCreate(&e0));
    SR_HIP(hipEventCreate(&e1));
    SR_HIP(hipMemcpyAsync(b.p, a.p, bytes, hipMemcpyDeviceToDevice, ctx().stream));   // warm
    SR_HIP(hipEventRecord(e0, ctx().stream));
    for (int i = 0; i < iters; i++)
        SR_HIP(hipMemcpyAsync(b.p, a.p, bytes, hipMemcpyDeviceToDevice, ctx().stream));
    SR_HIP(hipEventRecord(e1, ctx().stream));
    SR_HIP(hipStreamSynchronize(ctx().stream));
    float ms = 0.f;
    SR_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *gbps_out = 2.0 * (double)bytes * iters / ((double)ms * 1e-3) / 1e9;
    return 0;
    SR_CATCH(-1)
}

int sr_profile_enable(int on) {
    SR_TRY
    if (on) {
        ensure_device();
        profile_prewarm();
    }
    ctx().profiling = on != 0;
    return 0;
    SR_CATCH(-1)
}

int sr_profile_reset(void) {
    SR_TRY
    profile_reset();
    return 0;
    SR_CATCH(-1)
}

int sr_profile_get(int kind, double *total_ms, long *launches) {
    SR_TRY
    profile_get(kind, total_ms, launches);
    return 0;
    SR_CATCH(-1)
}

int sr_mfma_peak_probe(double ms_target, double *tflops, double *mhz) {
    SR_TRY
    if (!(ms_target > 0.0) || ms_target > 2000.0) fail("ms_target must be in (0, 2000]");
    mfma_peak_probe(ms_target, tflops, mhz);
    return 0;
    SR_CATCH(-1)
}

int sr_mfma_streamed_probe(double ms_target, double *tflops, double *mhz) {
    SR_TRY
    if (!(ms_target > 0.0) || ms_target > 2000.0) fail("ms_target must be in (0, 2000]");
    mfma_peak_probe(ms_target, tflops, mhz, 1);
    return 0;
    SR_CATCH(-1)
}

}  // extern "C"
