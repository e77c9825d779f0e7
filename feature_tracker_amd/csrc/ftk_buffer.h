// ftk_buffer.h — the one owner of device and pinned host memory behind the C ABI (host code only; every allocation and every
// release of the library is in this file, apart from the throw-away probes of ftk_warmup).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// One block of device memory, or of pinned host memory, that grows on demand and is released with its owner.  Move-only.
class ftk_buffer {
public:
    enum Kind { kDevice, kPinned, kPinnedNonCoherent };  // hipMalloc | hipHostMallocDefault | hipHostMallocNonCoherent
    explicit ftk_buffer(Kind kind = kDevice) : kind_(kind) {}
    ftk_buffer(ftk_buffer &&o) noexcept : ptr_(o.ptr_), bytes_(o.bytes_), kind_(o.kind_) { o.ptr_ = nullptr, o.bytes_ = 0; }
    ftk_buffer &operator=(ftk_buffer &&o) noexcept {
        if (this != &o) {
            release();
            ptr_ = o.ptr_, bytes_ = o.bytes_, kind_ = o.kind_;
            o.ptr_ = nullptr, o.bytes_ = 0;
        }
        return *this;
    }
    ftk_buffer(const ftk_buffer &) = delete;
    ftk_buffer &operator=(const ftk_buffer &) = delete;
    ~ftk_buffer() { release(); }

    void *get() const { return ptr_; }
    template <class T>
    T *as() const { return static_cast<T *>(ptr_); }
    size_t bytes() const { return bytes_; }  // capacity
    explicit operator bool() const { return ptr_ != nullptr; }

    // At least `bytes` large on return.  A block that is too small is replaced (its content is NOT kept) by one of
    // `bytes + slack` rounded up to `align`, after `stream` has drained: earlier launches may still use the old block.
    // *grew tells the callers whose kernels rely on a fill pattern that there is a new, unfilled block.
    hipError_t reserve(hipStream_t stream, size_t bytes, size_t slack, size_t align, bool *grew = nullptr) {
        if (grew) {
            *grew = false;
        }
        if (bytes <= bytes_) {
            return hipSuccess;
        }
        if (ptr_) {
            const hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess) {
                return e;
            }
            release();
        }
        const size_t want = (bytes + slack + align - 1) / align * align;
        void *p = nullptr;
        const hipError_t e = kind_ == kDevice ? hipMalloc(&p, want)
                                              : hipHostMalloc(&p, want, kind_ == kPinned ? hipHostMallocDefault : hipHostMallocNonCoherent);
        if (e != hipSuccess) {
            return e;
        }
        ptr_ = p;
        bytes_ = want;
        if (grew) {
            *grew = true;
        }
        return hipSuccess;
    }

    void release() {
        if (ptr_) {
            (void)(kind_ == kDevice ? hipFree(ptr_) : hipHostFree(ptr_));
            ptr_ = nullptr;
            bytes_ = 0;
        }
    }

private:
    void *ptr_ = nullptr;
    size_t bytes_ = 0;
    Kind kind_;
};
