// Host-side helpers of the HIP translation units (render.hip, multi.hip, denoise.hip): not part of gpu.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

namespace nrt {

inline void check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}

// Makes `device` current for a scope and restores the caller's device afterwards: the
// library never leaves the caller's (e.g. torch's) current device changed, and every
// allocation, memset and launch goes to the device the scene lives on.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (device != prev) check(hipSetDevice(device), "hipSetDevice");
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

}  // namespace nrt
