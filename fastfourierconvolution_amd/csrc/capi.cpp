// C-ABI plumbing: thread-local error text, launch checks, the launch-support helpers.
#include <hip/hip_runtime.h>

#include <mutex>
#include <set>
#include <string>
#include <utility>

#include "ffc_internal.h"

namespace ffc {

static thread_local std::string g_err;

void set_error(const std::string& msg) { g_err = msg; }

int launch_status(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string(what) + ": " + hipGetErrorString(e));
        return FFC_E_LAUNCH;
    }
    return FFC_OK;
}

int raise_dynamic_lds(const void* kernel, size_t lds_bytes, const char* what) {
    if (lds_bytes <= 64 * 1024) return FFC_OK;
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> raised;
    std::lock_guard<std::mutex> g(mu);
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && raised.count({kernel, dev})) return FFC_OK;
    if (e == hipSuccess) e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) {
        set_error(std::string(what) + ": hipFuncSetAttribute: " + hipGetErrorString(e));
        return FFC_E_LAUNCH;
    }
    raised.insert({kernel, dev});
    return FFC_OK;
}

int cu_count() {
    int cus = 0, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return 0;
    return cus;
}

}  // namespace ffc

extern "C" const char* ffc_last_error(void) { return ffc::g_err.c_str(); }

extern "C" int ffc_abi_version(void) { return 4; }   // 4: ffc_bn_fold.moments, ffc_fu_forward_ex4 (round 6)

// sizes of the ABI structs, so bindings can verify their mirror layouts
extern "C" int ffc_struct_sizes(int* out, int n) {
    if (!out || n < 6) return FFC_E_INVALID;
    out[0] = (int)sizeof(ffc_conv_seg);
    out[1] = (int)sizeof(ffc_conv_phase);
    out[2] = (int)sizeof(ffc_conv_job);
    out[3] = (int)sizeof(ffc_convp_seg);
    out[4] = (int)sizeof(ffc_convp_phase);
    out[5] = (int)sizeof(ffc_convp_job);
    if (n >= 7) out[6] = (int)sizeof(ffc_bn_fold);
    if (n >= 8) out[7] = (int)sizeof(ffc_in_tf);
    if (n >= 10) {
        out[8] = (int)sizeof(ffc_bn_rf_item);
        out[9] = (int)sizeof(ffc_bn_apply_item);
    }
    if (n >= 11) out[10] = (int)sizeof(ffc_cbn_apply_item);
    if (n >= 12) out[11] = (int)sizeof(ffc_sn_job);
    return FFC_OK;
}
