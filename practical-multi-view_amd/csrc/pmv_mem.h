// The one owner of device and pinned memory: every allocation of the library is a Growable (or its typed form, Buf<T>) that is a member
// of the object it belongs to - the context, a back-end workspace set, a combiner, a session, a feeder - and goes when that object goes.
// This header is the only place that calls the runtime's allocation functions.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stddef.h>
#include <stdint.h>
#include <utility>

namespace pmv {

enum MemKind : uint8_t {
    MEM_DEVICE = 0,   // hipMalloc
    MEM_PINNED,       // hipHostMalloc, default flags
    MEM_MAPPED,       // hipHostMalloc(hipHostMallocMapped | hipHostMallocCoherent) and its device pointer
};
enum MemGrow : uint8_t {
    GROW_EXACT = 0,   // to the size asked for
    GROW_SLACK,       // need * 5 / 4, rounded up to 4 KB (the batch engine's per-round scratch)
};

// bytes currently allocated through this header, process-wide: [0] device, [1] pinned (pmv_debug_mem_live). Written where a block is made
// and where it is freed, nowhere else.
inline std::atomic<long long> g_mem_live[2];

struct Growable {
    void* p = nullptr;
    size_t cap = 0;        // bytes behind p
    char* dev = nullptr;   // the address kernels use: p itself, or the device alias of a mapped pinned block (null for MEM_PINNED)
    MemKind kind;
    MemGrow grow;
    explicit Growable(MemKind k = MEM_DEVICE, MemGrow g = GROW_EXACT) : kind(k), grow(g) {}
    Growable(const Growable&) = delete;
    Growable& operator=(const Growable&) = delete;
    Growable(Growable&& o) noexcept : kind(o.kind), grow(o.grow) { take(o); }
    Growable& operator=(Growable&& o) noexcept { if (this != &o) { release(); kind = o.kind; grow = o.grow; take(o); } return *this; }
    ~Growable() { release(); }
    // no-op when the block is large enough; otherwise the old block is freed first and a new one made (its contents are NOT carried over)
    hipError_t ensure(size_t need) {
        if (need <= cap) return hipSuccess;
        if (hipError_t e = release()) return e;
        if (grow == GROW_SLACK) need = (need * 5 / 4 + 4095) & ~(size_t)4095;
        hipError_t e = kind == MEM_DEVICE ? hipMalloc(&p, need)
                     : kind == MEM_PINNED ? hipHostMalloc(&p, need, hipHostMallocDefault)
                                          : hipHostMalloc(&p, need, hipHostMallocMapped | hipHostMallocCoherent);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = need;
        g_mem_live[kind != MEM_DEVICE] += (long long)need;
        if (kind == MEM_DEVICE) dev = (char*)p;
        if (kind == MEM_MAPPED) e = hipHostGetDevicePointer((void**)&dev, p, 0);
        return e;
    }
    // a fixed buffer of a create function's allocation table: the table names the kind
    hipError_t alloc(MemKind k, size_t bytes) { kind = k; return ensure(bytes); }
    hipError_t release() {
        if (!p) return hipSuccess;
        const hipError_t e = kind == MEM_DEVICE ? hipFree(p) : hipHostFree(p);
        g_mem_live[kind != MEM_DEVICE] -= (long long)cap;
        p = nullptr; cap = 0; dev = nullptr;
        return e;
    }
private:
    void take(Growable& o) { p = o.p; cap = o.cap; dev = o.dev; o.p = nullptr; o.cap = 0; o.dev = nullptr; }
};

// A Growable that reads as the T* it holds: call sites pass it, index it and add to it as they did the raw pointer; a cast to another
// pointer type is written as before, (U*)buf. dm(): the device alias of a mapped pinned block.
template <class T> struct Buf : Growable {
    using Growable::Growable;
    T* get() const { return (T*)p; }
    T* dm() const { return (T*)dev; }
    operator T*() const { return (T*)p; }
    template <class U> explicit operator U*() const { return (U*)p; }
};

struct MemRow { Growable* buf; size_t bytes; MemKind kind; };   // one row of an allocation table
inline hipError_t mem_alloc_table(const MemRow* rows, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (hipError_t e = rows[i].buf->alloc(rows[i].kind, rows[i].bytes)) return e;
    return hipSuccess;
}

}  // namespace pmv
