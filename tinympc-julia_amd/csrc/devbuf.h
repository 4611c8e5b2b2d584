// Owning buffers of the solver's GPU and pinned host memory: the one place that calls the HIP allocators.  A buffer is freed
// when its owner goes (or is assigned over); nothing is listed by hand.  Every failing call reports through set_error and
// returns -1.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>
#include <vector>

namespace tmpc {

bool hip_ok(hipError_t e, const char *what);
// hipMalloc / hipFree behind a process-wide count of live device bytes (tmpc_device_bytes_live).  Defined once, in solver.hip:
// units specialised at run time include this header and must not get a counter of their own.
int device_alloc_bytes(void **p, size_t bytes);
void device_free_bytes(void *p, size_t bytes);

// Move-only owner of `count()` elements of device memory.  Converts to the raw pointer, so kernels' argument blocks, copies and
// null tests read it as they would the pointer.  alloc and upload ALWAYS free and allocate again, also at the same size (hipFree
// synchronises the device: an allocation is never reused under a launch that may still read it); reserve keeps what suffices.
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            free();
            std::swap(p_, o.p_), std::swap(n_, o.n_);
        }
        return *this;
    }
    ~DevBuf() { free(); }

    int alloc(size_t n) {   // contents undefined; n == 0 allocates one element
        free();
        if (device_alloc_bytes((void **)&p_, bytes(n))) return -1;
        n_ = n;
        return 0;
    }
    int alloc_zero(size_t n) { return alloc(n) || zero(); }
    int reserve(size_t n) { return n_ >= n ? 0 : alloc(n); }   // contents are not preserved
    int upload(const T *h, size_t n) {                         // a blocking copy
        if (alloc(n)) return -1;
        return hip_ok(hipMemcpy(p_, h, n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy (upload)") ? 0 : -1;
    }
    int upload(const std::vector<T> &h) { return upload(h.data(), h.size()); }
    int zero() { return hip_ok(hipMemset(p_, 0, n_ * sizeof(T)), "hipMemset") ? 0 : -1; }
    void free() {
        if (p_) device_free_bytes(p_, bytes(n_));
        p_ = nullptr, n_ = 0;
    }
    size_t count() const { return n_; }
    operator T *() const { return p_; }

private:
    static size_t bytes(size_t n) { return (n ? n : 1) * sizeof(T); }
    T *p_ = nullptr;
    size_t n_ = 0;
};

// The same shape over page-locked host memory (hipHostMalloc)
template <class T>
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { free(); }

    int alloc(size_t n) {
        free();
        if (!hip_ok(hipHostMalloc((void **)&p_, (n ? n : 1) * sizeof(T), hipHostMallocDefault), "hipHostMalloc")) return -1;
        n_ = n;
        return 0;
    }
    int reserve(size_t n) { return n_ >= n ? 0 : alloc(n); }
    void free() {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr, n_ = 0;
    }
    size_t count() const { return n_; }
    operator T *() const { return p_; }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace tmpc
