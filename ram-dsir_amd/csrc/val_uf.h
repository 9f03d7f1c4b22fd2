// val_uf.h -- the union-find of the validation labelling kernels (val_post.hip: planes, val_volume.hip: volumes).  A parent is never
// larger than its child (parent[n] <= n), so the root of a component is its first node in raster order.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ int load_parent(const int* P, int n) { return __hip_atomic_load(P + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// at most n steps: parent[n] <= n
__device__ __forceinline__ int find_root(const int* P, int n) {
    for (int p = load_parent(P, n); p != n; p = load_parent(P, n)) n = p;
    return n;
}

// Links the larger root under the smaller with atomicMin.  A retry happens only when another thread has lowered parent[a] in between;
// its old value is then united with b in turn, so no link is lost, and every retry starts from a strictly smaller node.
__device__ __forceinline__ void unite(int* P, int a, int b) {
    for (;;) {
        a = find_root(P, a);
        b = find_root(P, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(P + a, b);
        if (old == a) return;
        a = old;
    }
}

}  // namespace
