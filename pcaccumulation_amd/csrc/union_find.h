// Lock-free union-find on an int parent table (cluster.hip: DBSCAN's core-core edges; accum_components.hip: the voxels of the accumulated scene cloud).
// One copy for both.  The larger root always goes under the smaller one, so parent[x] <= x holds at every moment: every walk strictly descends and
// ends, and the root of a set is its smallest member.
// In a kernel the loads and stores are relaxed agent-scope atomics and the link is an atomicCAS; in a g++ build (tests/accum_components_host_driver.cpp)
// the same functions run sequentially on plain memory.  Includes nothing of HIP.
#pragma once

#if defined(__HIPCC__)
#define PCACC_UF __device__ __forceinline__
PCACC_UF int uf_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
PCACC_UF void uf_store(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
PCACC_UF int uf_cas(int *p, int expected, int v) { return atomicCAS(p, expected, v); }          // -> the value found
#else
#define PCACC_UF static inline
PCACC_UF int uf_load(const int *p) { return *p; }
PCACC_UF void uf_store(int *p, int v) { *p = v; }
PCACC_UF int uf_cas(int *p, int expected, int v)
{
    const int old = *p;
    if (old == expected) *p = v;
    return old;
}
#endif

PCACC_UF int uf_find(int *parent, int x)
{
    int p = uf_load(&parent[x]);
    while (p != x) {
        const int gp = uf_load(&parent[p]);
        if (gp != p) uf_store(&parent[x], gp);                                   // path halving
        x = p;
        p = gp;
    }
    return x;
}

// The root of x without a store: for a pass in which every slot is written by its own lane only (no joins run beside it).
PCACC_UF int uf_root(const int *parent, int x)
{
    int p = uf_load(&parent[x]);
    while (p != x) {
        x = p;
        p = uf_load(&parent[x]);
    }
    return x;
}

// joins the sets of a and b; returns the surviving (smaller) root
PCACC_UF int uf_union(int *parent, int a, int b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        if (a < b) { const int t = a; a = b; b = t; }
        if (uf_cas(&parent[a], a, b) == a) return b;                              // larger root goes under the smaller one
    }
}

// The same join with at most `tries` attempts of the CAS: -1 when every one of them lost against another lane (nothing is joined then).
PCACC_UF int uf_union_bounded(int *parent, int a, int b, int tries)
{
    for (int t = 0; t < tries; ++t) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        if (a < b) { const int s = a; a = b; b = s; }
        if (uf_cas(&parent[a], a, b) == a) return b;
    }
    return -1;
}
