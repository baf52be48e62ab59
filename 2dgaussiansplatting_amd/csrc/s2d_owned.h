// s2d_owned.h -- host-side owners of what the HIP runtime hands out: a device array, pinned host memory, an event.
// Each starts empty, lets go in its destructor, cannot be copied and converts to the raw handle, so launch sites read
// as with plain pointers.  Whoever lets a buffer go (release(), a second alloc(), a growing reserve(), the destructor)
// makes sure first that no stream still uses it, and that its device is current.
// Host-only and self-contained (the s2d_multi units include it in the host simulation of the tests, without s2d_device.h).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#define S2D_LOCAL __attribute__((visibility("hidden"))) // nothing of these types is exported from the library

// In a function that returns hipError_t: hand a failure on.
#define S2D_TRY(expr)                      \
    do {                                   \
        const hipError_t e_ = (expr);      \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

namespace s2d {

template <typename T>
class S2D_LOCAL DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        std::swap(p_, o.p_), std::swap(cap_, o.cap_); // (what this one held goes with `o`)
        return *this;
    }
    ~DevBuf() { release(); }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; } // elements

    // Exactly `count` elements (at least one, so that an empty scene still has buffers); the old contents go.
    hipError_t alloc(size_t count)
    {
        release();
        const size_t want = std::max<size_t>(count, 1);
        const hipError_t e = hipMalloc((void**)&p_, want * sizeof(T)); // (a null pointer when it fails)
        if (e == hipSuccess) cap_ = want;
        return e;
    }
    // Room for `count` elements in an array that only grows, by a quarter more than asked for; the old contents go.
    hipError_t reserve(size_t count) { return count <= cap_ ? hipSuccess : alloc(std::max<size_t>(count + count / 4, 256)); }
    void release()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr, cap_ = 0;
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// Pinned host memory (hipHostMalloc with the caller's flags), allocated once and kept until its owner lets it go.
template <typename T>
class S2D_LOCAL HostBuf {
public:
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    ~HostBuf() { release(); }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    hipError_t alloc(size_t count, unsigned flags) { return p_ ? hipSuccess : hipHostMalloc((void**)&p_, count * sizeof(T), flags); }
    void release()
    {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
    }

private:
    T* p_ = nullptr;
};

class S2D_LOCAL Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept
    {
        std::swap(e_, o.e_);
        return *this;
    }
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    operator hipEvent_t() const { return e_; }
    hipError_t create(unsigned flags) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }

private:
    hipEvent_t e_ = nullptr;
};

} // namespace s2d
