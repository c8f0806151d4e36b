// qn_union_find.cuh - the lock-free union-find of the map units (k_mc_hook of qn_mapclusters.inc over cloud indices, k_mf_merge of qn_mapfrontier.inc over
// the linear indices of frontier voxels): a forest in parent[], parent[x] == x at a root, in which the root of a tree is its smallest element.
//   find      uf_find: up the chain to the root, halving the path on the way (an atomic min of parent[x] with x's grandparent).
//   unite     uf_unite: find the two roots and link the larger under the smaller one only, by compare-and-swap(parent[hi], hi, lo); on failure go on from the
//             value the swap returned.  uf_unite_min, at the end of this file, is the frontiers' faster link with its own, weaker invariant.
// Invariant: a word changes only at a root, by a link that stores a smaller root, or falls to an ancestor, by a halving.  So parent[x] <= x at every instant
// (the caller starts from parent[x] <= x with x's tree its own component so far: x itself, or what a launch before this one has already joined), the forest
// is acyclic at every instant, and a find, which moves to a strictly smaller index every trip, ends.  A value ever read from parent[x] stays an ancestor of x
// for good, so a stale read is never wrong, only longer.  A failed swap means parent[hi] was lowered by somebody else: the pair (a, b) the union goes on
// with is smaller in a well-founded order, so every union ends, and when it ends both ends have one root.  No lane ever waits on another lane, wave or
// block: there is no lock and no flag, a lane that loses a race has made progress through the winner's store.
// Inside the launch that unites, parent[] is read by agent-scope relaxed atomic loads (uf_load) and written by agent-scope atomics only: a plain load could be
// served from another XCD's stale L2 line, and would then only walk a longer path; the atomics are what the argument needs.  The launch after it sees the
// final forest through the kernel boundary.  Components are a set property, so the roots are the same whatever the schedule.
// Tested directly: tests/union_find_model.py restates uf_find, uf_unite and uf_unite_min as step machines, one step an atomic memory operation, and
// tests/test_union_find_model.py runs every interleaving of two and three lanes on four and five nodes through them (whoever changes this file changes the
// model, and the other way round); tests/test_gpu_map_prims.py runs the device builds, through qn_kf_debug_map_prims (qn_map_selftest.hip), on paths, stars,
// combs, cliques and starting forests against a serial union-find.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

__device__ __forceinline__ uint32_t uf_load(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x as far as this lane can see; every trip moves to a strictly smaller index.  Serves both linkers: under uf_unite_min g need not stay an
// ancestor of x, only an element of x's component no larger than x (the last paragraph of this file), which is all the halving needs there
__device__ __forceinline__ uint32_t uf_find(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = uf_load(parent + x);
    if (p == x) return x;
    const uint32_t g = uf_load(parent + p);
    if (g == p) return p;
    __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // path halving
    x = g;
  }
}

// a and b into one tree: the larger root under the smaller one, never the other way
__device__ __forceinline__ void uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a); b = uf_find(parent, b);
    if (a == b) return;
    const uint32_t hi = max(a, b), lo = min(a, b);
    uint32_t seen = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    a = seen; b = lo;                                    // hi is a root no more: seen < hi is its new parent
  }
}

// The second entry point, for k_mf_merge alone: the same union with the link an atomic min, not a swap.  Measured, not argued: the frontier call takes
// 0.340 ms with this link against 0.366 and 0.407 with the swap on a 3 000 000-record map, 1.022 against 1.049 on one of 30 000 000; before the two were
// unified 0.347 to 0.352 and 1.031 to 1.041 (profiles/EXPERIMENTS.md).  The min always stores, so when hi was a root no more (seen < hi) it may have hung hi under lo, which need not be an ancestor:
// the invariant weakens to "every value ever stored at parent[x] is an element of x's component, no larger than x", which still keeps the forest acyclic and
// every find finite, and the union goes on with (seen, lo), hi's parent of then, so nothing joined is lost.  The clusters keep the swap, whose invariant is
// the one stated above.
__device__ __forceinline__ void uf_unite_min(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a); b = uf_find(parent, b);
    if (a == b) return;
    const uint32_t hi = max(a, b), lo = min(a, b);
    const uint32_t seen = __hip_atomic_fetch_min(parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seen == hi) return;
    a = seen; b = lo;
  }
}

}  // namespace
