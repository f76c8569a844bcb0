// devbuf.h -- the owners of every device and pinned host allocation of the library.
//
// Buf<T, K> holds one allocation of kind K: pointer and size live in the same object and change together, the destructor
// frees, a failed allocation leaves the owner empty (null, 0 bytes).  Move-only.  It converts to T*, so that a kernel launch
// or `if (kb->planes)` reads as with a raw pointer.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stddef.h>
#include <stdint.h>

enum class Mem {
    Scratch,        // device memory through dftk_scratch_malloc (DFTK_MI_POISON fills it with NaNs)
    Table,          // device memory through plain hipMalloc: tables and small result buffers, never poisoned
    Pinned,         // page-locked host memory
    PinnedMapped    // page-locked host memory mapped into the device's address space
};

// The one extension point: a host-only check defines these two before including the header and gets fakes.
#ifndef DFTK_DEVBUF_ALLOC
hipError_t dftk_scratch_malloc(void** p, size_t bytes);   // api.cpp
inline hipError_t devbuf_alloc(Mem k, void** p, size_t bytes) {
    switch (k) {
        case Mem::Scratch: return dftk_scratch_malloc(p, bytes);
        case Mem::Table: return hipMalloc(p, bytes);
        case Mem::Pinned: return hipHostMalloc(p, bytes);
        default: return hipHostMalloc(p, bytes, hipHostMallocMapped);
    }
}
inline hipError_t devbuf_free(Mem k, void* p) {
    return (k == Mem::Scratch || k == Mem::Table) ? hipFree(p) : hipHostFree(p);
}
#define DFTK_DEVBUF_ALLOC devbuf_alloc
#define DFTK_DEVBUF_FREE devbuf_free
#endif

// live DEVICE allocations held by owners, process-wide (dftk_mi_device_buffers_live); pinned memory is not counted
inline std::atomic<int64_t> g_devbuf_live_count{0}, g_devbuf_live_bytes{0};

template <class T, Mem K = Mem::Scratch>
class Buf {
    T* p_ = nullptr;
    size_t bytes_ = 0;
    static void book(int64_t n, int64_t bytes) {
        if (K == Mem::Scratch || K == Mem::Table) {
            g_devbuf_live_count.fetch_add(n, std::memory_order_relaxed);
            g_devbuf_live_bytes.fetch_add(bytes, std::memory_order_relaxed);
        }
    }

public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) {
        o.p_ = nullptr;
        o.bytes_ = 0;
    }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_;
            bytes_ = o.bytes_;
            o.p_ = nullptr;
            o.bytes_ = 0;
        }
        return *this;
    }
    ~Buf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t bytes() const { return bytes_; }

    // frees; the owner is empty afterwards whatever the free returned
    hipError_t reset() {
        if (!p_) return hipSuccess;
        const hipError_t e = DFTK_DEVBUF_FREE(K, (void*)p_);
        book(-1, -(int64_t)bytes_);
        p_ = nullptr;
        bytes_ = 0;
        return e;
    }
    // exactly `bytes` (0: stays empty); whatever was held is released first and its contents are not kept
    hipError_t alloc(size_t bytes) {
        hipError_t e = reset();
        if (e != hipSuccess || bytes == 0) return e;
        void* p = nullptr;
        e = DFTK_DEVBUF_ALLOC(K, &p, bytes);
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        bytes_ = bytes;
        book(1, (int64_t)bytes);
        return hipSuccess;
    }
    // grow-only: nothing happens while `bytes` fit; otherwise alloc(bytes + slack).  The caller has made sure that no
    // kernel still uses the old buffer (each site keeps its own synchronisation).
    hipError_t reserve(size_t bytes, size_t slack = 0) { return bytes <= bytes_ ? hipSuccess : alloc(bytes + slack); }
};

template <class T> using DevBuf = Buf<T, Mem::Scratch>;
template <class T> using DevTable = Buf<T, Mem::Table>;
template <class T> using PinnedBuf = Buf<T, Mem::Pinned>;
