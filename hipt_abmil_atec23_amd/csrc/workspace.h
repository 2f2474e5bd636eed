// Host side only: how every entry point lays out, sizes and checks the scratch buffer its caller hands it.
#pragma once
#include "common.h"  // hipt_set_error, HIPT_OK / HIPT_E_WORKSPACE

inline size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

// Every workspace is described ONCE, by the carve_*() function that hands out its parts: a forward runs it over the caller's
// buffer, the matching *_workspace_bytes entry point over no buffer at all (the default Carver) and returns `used`.
struct Carver {
    char* base;
    size_t cap, used = 0;
    Carver(void* b = nullptr, size_t c = SIZE_MAX) : base((char*)b), cap(c) {}
    void* take(size_t n) {
        void* p = base ? base + used : nullptr;
        used += al256(n);
        return p;
    }
    template <class T> T* take(size_t count) { return (T*)take(count * sizeof(T)); }
    bool ok() const { return used <= cap && (((uintptr_t)base & 255) == 0 || used == 0); }
};
template <class F> size_t dry_run(F carve) {
    Carver c;
    carve(c);
    return c.used;
}
// the ONE refusal of a short or misaligned buffer: a forward calls it before its first launch, memset or DeviceSetup
inline int check_workspace(const Carver& c, const char* who) {
    if (c.ok()) return HIPT_OK;
    hipt_set_error("%s: workspace %zu B too small / unaligned (need %zu)", who, c.cap, c.used);
    return HIPT_E_WORKSPACE;
}
