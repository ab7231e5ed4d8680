// Stand-in for <hip/hip_runtime.h> in tests/native/devarray_check.cpp: the three calls csrc/dev_array.hpp makes, over the
// host heap, with a count of the live allocations and a way to make the n-th hipMalloc from now fail.  No GPU, no ROCm.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <cstring>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToHost, hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };

namespace fakehip {
inline long live = 0;        // hipMalloc'd and not yet hipFree'd
inline long mallocs = 0;     // successful hipMallocs so far
inline long failAfter = 0;   // n > 0: the n-th hipMalloc from now fails (once)
}  // namespace fakehip

inline hipError_t hipMalloc(void** ptr, size_t bytes) {
    if (fakehip::failAfter > 0 && --fakehip::failAfter == 0) {
        *ptr = nullptr;
        return hipErrorOutOfMemory;
    }
    *ptr = std::malloc(bytes ? bytes : 1);
    if (!*ptr) return hipErrorOutOfMemory;
    ++fakehip::live;
    ++fakehip::mallocs;
    return hipSuccess;
}

inline hipError_t hipFree(void* ptr) {
    if (ptr) --fakehip::live;
    std::free(ptr);   // (a second free of the same array is AddressSanitizer's to report)
    return hipSuccess;
}

inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
