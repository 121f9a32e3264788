// The pieces the two connected-component families share: index_components.hip (u8 instance index maps, one id per pixel) and
// plane_components.hip (ragged bit planes, one plane per mask).  Defined once, so both label a tile by the same instructions:
//
//   lds_find / lds_union   the lock-free union-find over tile-local offsets in LDS (workgroup scope);
//   glb_find / glb_union   the same over global memory (agent scope), for the merge across tile borders;
//   cc_tile_label          a CC_TH x CC_TW tile of ids in LDS -> every pixel's tile-local root and the roots' pixel counts;
//   cc_key                 the (area, first pixel) order of "the largest component, among equals the first".
//
// A link only ever decreases (atomicMin towards the smaller root), so a trip of any loop below either finishes or sees a strictly
// smaller parent, and the root of a component is its minimum raster index -- the canonical name.  Integer atomics only.
#pragma once
#include "common.h"

constexpr int CC_TH = 32, CC_TW = 64, CC_THREADS = 256, CC_PER = 8;     // a thread owns CC_PER consecutive pixels of a tile row
constexpr int CC_TILE = CC_TH * CC_TW;
constexpr unsigned CC_NONE = 0xffffffffu;
static_assert(CC_TILE == CC_THREADS * CC_PER && CC_TW % CC_PER == 0 && CC_TILE <= 65536, "tile / thread shape");

// ---- the lock-free union-find, once over LDS (workgroup scope) and once over global memory (agent scope) ----
__device__ __forceinline__ unsigned lds_find(unsigned *par, unsigned x)
{
    for (;;) {
        const unsigned p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) return x;
        x = p;                                                           // p < x
    }
}
__device__ __forceinline__ void lds_union(unsigned *par, unsigned a, unsigned b)
{
    for (;;) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = atomicMin(&par[a], b);                      // a was a root when found: hang it under the smaller root
        if (old == a) return;
        a = old;                                                         // somebody linked a first (old < a): old and b remain to be joined
    }
}
__device__ __forceinline__ int glb_find(int *par, int x)
{
    for (;;) {
        const int p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void glb_union(int *par, int a, int b)
{
    for (;;) {
        a = glb_find(par, a);
        b = glb_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&par[a], b);
        if (old == a) return;
        a = old;
    }
}

// ids[CC_TILE]: the tile's ids in LDS, 0 = not a pixel to label (background, or outside the image / plane); written by the caller,
// with a barrier behind the writes.  -> root[j] = the tile-local root (offset ly * CC_TW + lx) of the thread's pixel i0 + j, CC_NONE
// where ids is 0; cnt[r] = the tile's pixels under root r, 0 at every other offset.  Pixels join under 4- or 8-connectivity where
// their ids are equal.  All CC_THREADS threads call this (it holds barriers, the last one behind the counts).
__device__ __forceinline__ void cc_tile_label(const uint8_t *ids, unsigned *par, unsigned *cnt, int conn8, unsigned (&root)[CC_PER])
{
    const int tid = threadIdx.x;
    const int ly = tid / (CC_TW / CC_PER), lx0 = (tid % (CC_TW / CC_PER)) * CC_PER;
    const unsigned i0 = ly * CC_TW + lx0;
    unsigned my[CC_PER], up[CC_PER + 2];                                  // up[0], up[CC_PER + 1]: the row above, one to the left / right
    for (int j = 0; j < CC_PER; ++j) my[j] = ids[i0 + j];
    const unsigned left = lx0 > 0 ? ids[i0 - 1] : 0u;
    for (int j = 0; j < CC_PER + 2; ++j) {
        const int lx = lx0 - 1 + j;
        up[j] = (ly > 0 && lx >= 0 && lx < CC_TW) ? ids[i0 - CC_TW - 1 + j] : 0u;
    }
    // a run of one id inside the thread's pixels starts out linked to its first pixel
    unsigned start = i0;
    for (int j = 0; j < CC_PER; ++j) {
        if (j == 0 || my[j] != my[j - 1]) start = i0 + j;
        par[i0 + j] = my[j] ? start : CC_NONE;
        cnt[i0 + j] = 0u;
    }
    __syncthreads();
    bool prev_up = false;
    for (int j = 0; j < CC_PER; ++j) {
        const unsigned id = my[j], i = i0 + j;
        if (!id) { prev_up = false; continue; }
        const bool cont = j > 0 && my[j - 1] == id;
        if (j == 0 && left == id) lds_union(par, i, i - 1);
        if (up[j + 1] == id) {                                           // the pixel above: its own neighbours are joined in its row
            if (!(cont && prev_up)) lds_union(par, i, i - CC_TW);
            prev_up = true;
        } else {
            prev_up = false;
            if (conn8) {
                if (up[j] == id) lds_union(par, i, i - CC_TW - 1);
                if (up[j + 2] == id) lds_union(par, i, i - CC_TW + 1);
            }
        }
    }
    __syncthreads();
    // nothing writes par[] from here on: every pixel reads its root, and a run of one root adds its length to the root's count once
    unsigned run = 0;
    for (int j = 0; j < CC_PER; ++j) {
        root[j] = my[j] ? lds_find(par, i0 + j) : CC_NONE;
        if (j > 0 && root[j] != root[j - 1]) {
            if (root[j - 1] != CC_NONE) atomicAdd(&cnt[root[j - 1]], run);
            run = 0;
        }
        ++run;
    }
    if (root[CC_PER - 1] != CC_NONE) atomicAdd(&cnt[root[CC_PER - 1]], run);
    __syncthreads();
}

// larger area first, among equal areas the lower first pixel: one 64-bit atomicMax picks "the largest component"
__device__ __forceinline__ unsigned long long cc_key(int area, int first) { return ((unsigned long long)(unsigned)area << 32) | (unsigned)~(unsigned)first; }
