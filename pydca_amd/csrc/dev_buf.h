// Ownership of device memory (included from dca_internal.h).  A block from dca_dev_malloc belongs to exactly one DevBuf: a
// local of the call that needs it or a member of the engine that keeps it.  It goes back to the pool when the DevBuf goes out
// of scope, is reset or is allocated again; dca_dev_free waits for the device, so the destructor needs no stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

// ---- capi.cpp : device allocations.  Blocks of at least 1 MiB go back to a process-wide, per-device cache
// when they are freed and later requests of a similar size are served from it (zero-filled), because
// hipMalloc / hipFree of GB-sized blocks costs tens of milliseconds per call on some hosts -- more than
// the whole mfDCA chain.  dca_dev_free waits for the device like hipFree does.
hipError_t dca_dev_malloc(void** p, size_t bytes, bool zero_recycled = true);   // false: buffers their first kernel overwrites completely
hipError_t dca_dev_free(void* p);

// count elements of T into a raw pointer: for the owners that are not a DevBuf (the context's members)
template <class T>
hipError_t dca_dev_alloc(T** p, size_t count, bool zero_recycled = true)
{
    return dca_dev_malloc(reinterpret_cast<void**>(p), count * sizeof(T), zero_recycled);
}

template <class T>
class DevBuf {
    T* p_ = nullptr;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { DevBuf(std::move(o)).swap(*this); return *this; }
    ~DevBuf() { reset(); }

    // releases what it held; zero_recycled = false: for buffers their first kernel overwrites completely
    hipError_t alloc(size_t count, bool zero_recycled = true) { reset(); return dca_dev_alloc(&p_, count, zero_recycled); }
    void reset() { dca_dev_free(p_); p_ = nullptr; }
    void swap(DevBuf& o) noexcept { std::swap(p_, o.p_); }
    T* get() const { return p_; }
    operator T*() const { return p_; }       // (templated kernels deduce their argument types: pass get() there)
    explicit operator bool() const { return p_ != nullptr; }
};
