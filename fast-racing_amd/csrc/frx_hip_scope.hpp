// What a scope owns on the device, over the HIP runtime API alone (no handle): a device buffer that frees itself, the caller's current device put back, and the one
// report of a failed device allocation.  Used by the handle (frx_handle.hpp) and by the entries that take none (frx_batch.cpp, frx_multi.cpp).  Private to
// libfrx.so; host code only.
//
// Inside an entry the DeviceGuard is declared first and the buffers after it: the buffers are then freed on the device they were allocated on, before the
// caller's device is put back.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <string>
#include <vector>

#include "frx_internal.hpp"

template <class T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t count) {
        release();
        const hipError_t e = hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) n = count; else p = nullptr;
        return e;
    }
    hipError_t reserve(size_t count) { return n >= count && p ? hipSuccess : alloc(count); }   // keep what is large enough
    hipError_t upload(const std::vector<T> &h) {
        hipError_t e = alloc(h.size());
        if (e != hipSuccess || h.empty()) return e;
        return hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    }
};

// buf.alloc(count) for `entry`: FRX_OK, or FRX_ERR_ALLOC with the entry's name and the byte count.  (A failed allocation is no error of a later launch: the
// runtime's last error is cleared.)
template <class T> static int dev_alloc(DevBuf<T> &buf, size_t count, const char *entry) {
    if (buf.alloc(count) == hipSuccess) return FRX_OK;
    (void)hipGetLastError();
    return frx::set_error(FRX_ERR_ALLOC, std::string(entry) + ": cannot allocate " + std::to_string(std::max<size_t>(count, 1) * sizeof(T)) + " bytes on the device");
}

// Entry points that take a device ordinal, or walk over the shards' devices, call hipSetDevice; the caller's current device is its own business (bench.py mixes
// torch and HIP in one process: a changed current device would send later allocations and launches to the wrong GPU) and is put back on every exit path.
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
