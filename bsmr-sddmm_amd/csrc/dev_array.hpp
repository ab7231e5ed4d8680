// The owner of every device array a handle keeps: one hipMalloc'd array, freed by its destructor, moved and never copied.
// A struct of DevArrays needs no destructor and no list of what to free; building one into a local and moving it out on
// success leaves nothing half-built behind a failed upload.  Depends on the HIP runtime alone.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

template <typename T>
class DevArray {
    T* ptr_ = nullptr;
    size_t count_ = 0;

public:
    DevArray() = default;
    DevArray(const DevArray&) = delete;
    DevArray& operator=(const DevArray&) = delete;
    DevArray(DevArray&& o) noexcept : ptr_(o.ptr_), count_(o.count_) { o.ptr_ = nullptr, o.count_ = 0; }
    DevArray& operator=(DevArray&& o) noexcept {
        if (this != &o) {
            reset();
            ptr_ = o.ptr_, count_ = o.count_;
            o.release();
        }
        return *this;
    }
    ~DevArray() { reset(); }

    void reset() {
        if (ptr_) (void)hipFree(ptr_);
        release();
    }
    // `count` elements, uninitialised; what was held is freed first.  count == 0: null, no allocation, success.
    // On failure the array is null and *err (when given) says why.
    bool alloc(size_t count, hipError_t* err = nullptr) {
        reset();
        if (count == 0) return true;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&ptr_), count * sizeof(T));
        if (e != hipSuccess) {
            ptr_ = nullptr;
            if (err) *err = e;
            return false;
        }
        count_ = count;
        return true;
    }
    // hands over / takes on an array allocated as another element type (the tile masks: built as words, read as records)
    T* release() {
        T* p = ptr_;
        ptr_ = nullptr, count_ = 0;
        return p;
    }
    void adopt(T* p, size_t count) {
        reset();
        ptr_ = p, count_ = p ? count : 0;
    }

    T* get() const { return ptr_; }
    size_t count() const { return count_; }
    size_t bytes() const { return count_ * sizeof(T); }
    operator T*() const { return ptr_; }   // kernel arguments, `if (array)` and hipMemcpy take it as the pointer it holds
};

// A host vector as a fresh device array, its size added to `bytes`.  An empty source: null, hipSuccess, no allocation.
// On failure nothing is counted; `dst` is null when the allocation failed and holds the array when the copy did.
template <typename T>
hipError_t devUpload(DevArray<T>& dst, const std::vector<T>& src, uint64_t& bytes) {
    hipError_t e = hipSuccess;
    if (!dst.alloc(src.size(), &e) || src.empty()) return e;
    e = hipMemcpy(dst.get(), src.data(), dst.bytes(), hipMemcpyHostToDevice);
    if (e == hipSuccess) bytes += dst.bytes();
    return e;
}
