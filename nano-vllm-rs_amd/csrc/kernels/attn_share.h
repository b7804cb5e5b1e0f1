// attn_share.h — host-side switches of the work-balanced decode attention launches (attn_share_kernel in attention.hip, attn_share_fp8_kernel in
// attention_fp8.hip): one definition for both files and both 16-bit builds.
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>

namespace nvr {

// NVR_ATTN_SHARE — 0: never, 1 (default): by the rule, 2: whenever it can run (probes)
inline int share_mode() { static const int v = getenv("NVR_ATTN_SHARE") ? atoi(getenv("NVR_ATTN_SHARE")) : 1; return v; }
inline bool share_enabled() { return share_mode() != 0; }
// one workgroup per CU of the current device
inline int share_workgroups() {
    static const int v = [] { int dev = 0, n = 0; if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256; return n; }();
    return v;
}

}  // namespace nvr
