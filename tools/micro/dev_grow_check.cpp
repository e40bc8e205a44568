// dev_grow_check.cpp — stand-alone check of pe::dev_grow (csrc/resident.hpp) under the host sanitizers: first use, no-grow, grow, failed allocation
// (capacity back to 0, so the next call allocates again and never hands a null buffer on), in the typed and the byte form.  The allocator is
// stubbed; nothing of the engine is linked.  From the repository root, after `make -C neuralpde.jl_amd/csrc emu` (for build/):
//   g++ -std=c++17 -DPINN_EMU -g -fsanitize=address,undefined -Ineuralpde.jl_amd/csrc -Ineuralpde.jl_amd/csrc/build tools/micro/dev_grow_check.cpp -o /tmp/dev_grow_check && /tmp/dev_grow_check
#include "plat.hpp"
#include <cassert>
#include <cstdio>
static int g_fail = 0, g_mallocs = 0, g_frees = 0, g_syncs = 0;
static void* t_malloc(size_t n) { ++g_mallocs; if (g_fail) return nullptr; return std::malloc(n ? n : 1); }
static void t_free(void* p) { if (p) ++g_frees; std::free(p); }
static int t_sync(plat_stream) { ++g_syncs; return 0; }
#define plat_malloc t_malloc
#define plat_free t_free
#define plat_sync t_sync
#include "resident.hpp"
int main() {
    double* p = nullptr; size_t cap = 0;
    assert(pe::dev_grow(p, cap, (size_t)0, nullptr) && !p && cap == 0 && g_mallocs == 0);         // nothing asked
    assert(pe::dev_grow(p, cap, (size_t)100, nullptr) && p && cap == 100 && g_mallocs == 1 && g_syncs == 1 && g_frees == 0);
    for (int i = 0; i < 100; ++i) p[i] = i;                                                     // all 100 elements are ours
    double* q = p;
    assert(pe::dev_grow(p, cap, (size_t)100, nullptr) && p == q && g_mallocs == 1 && g_syncs == 1);        // no-grow
    assert(pe::dev_grow(p, cap, (size_t)7, nullptr) && p == q && cap == 100);
    assert(pe::dev_grow(p, cap, (size_t)1000, nullptr) && cap == 1000 && g_mallocs == 2 && g_frees == 1 && g_syncs == 2);
    p[999] = 1.0;
    g_fail = 1;
    assert(!pe::dev_grow(p, cap, (size_t)2000, nullptr) && !p && cap == 0 && g_frees == 2);     // failed: null, capacity 0 (old block freed once)
    assert(!pe::dev_grow(p, cap, (size_t)10, nullptr) && !p && cap == 0);                       // the next call allocates again, never passes a null on
    g_fail = 0;
    assert(pe::dev_grow(p, cap, (size_t)10, nullptr) && p && cap == 10);
    p[9] = 2.0;
    t_free(p);
    void* v = nullptr; size_t bytes = 0;                                                        // byte form
    assert(pe::dev_grow(v, bytes, (size_t)64, nullptr) && v && bytes == 64);
    std::memset(v, 0, 64);
    void* v0 = v;
    assert(pe::dev_grow(v, bytes, (size_t)64, nullptr) && v == v0);
    g_fail = 1;
    assert(!pe::dev_grow(v, bytes, (size_t)65, nullptr) && !v && bytes == 0);
    std::puts("dev_grow: ok");
    return 0;
}
