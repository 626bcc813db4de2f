// A cursor that carves one block into typed tables, in step on the host side and on the device side. Plain C++ (no HIP include).
//   Carve c(host_base, device_base, capacity);   auto xy = c.take<float>(2 * n);   xy.h / xy.d / xy.off
//   Carve c;   (dry run: null bases, no limit)   ... c.bytes() is the size the same sequence of takes needs
// A take that does not fit sets `overflow` and hands out null pointers; the cursor still advances, so bytes() tells what was needed.
// The library's callers size a block by a dry run of the very function that then carves it (or check the total against the capacity first,
// as the back-end's *_prepare do), so their real runs cannot overflow and they do not look at the flag; a caller that carves a block of a
// size it did not derive that way must check `overflow` before it uses a pointer.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pmv {

template <class T> struct Carved { T* h; T* d; size_t off; };   // host pointer, device pointer, byte offset of one table

struct Carve {
    char* hb = nullptr; char* db = nullptr;
    size_t cap = SIZE_MAX, pos = 0;
    bool overflow = false;
    Carve() {}
    Carve(const void* host, const void* dev, size_t capacity) : hb((char*)host), db((char*)dev), cap(capacity) {}
    void skip_to(size_t align) { pos = (pos + align - 1) & ~(align - 1); }   // align: a power of two
    template <class T> Carved<T> take(size_t count, size_t align = alignof(T)) {
        skip_to(align);
        const size_t off = pos;
        pos += count * sizeof(T);
        if (pos > cap) { overflow = true; return {nullptr, nullptr, off}; }
        return {hb ? (T*)(hb + off) : nullptr, db ? (T*)(db + off) : nullptr, off};
    }
    size_t bytes() const { return pos; }
};

}  // namespace pmv
