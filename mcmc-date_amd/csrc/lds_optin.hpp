// lds_optin.hpp -- the one place that allows a kernel more than 64 KiB of dynamic LDS (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>

namespace mcd {

// More than 64 KiB of dynamic LDS has to be allowed once per kernel and device (a process may hold handles on several GPUs).
// Kernel: a kernel or one instantiation of a kernel template; every instantiation keeps its own mask, one bit per device.
// bytes: the most that any launch of it asks for -- always the same value for one kernel, since only the first call per device sets it.
template <auto Kernel>
inline hipError_t allow_dynamic_lds(int bytes)
{
    static std::atomic<unsigned long long> allowed{0};
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (!((allowed.load(std::memory_order_acquire) >> dev) & 1ull)) {
        if (hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)) return e;
        allowed.fetch_or(1ull << dev, std::memory_order_release);
    }
    return hipSuccess;
}

}  // namespace mcd
