// fs_unionfind.h -- the lock-free union-find of fs_clusters.hip and fs_tree.hip over a parent
// array in device memory.
//
// uf_unite hooks the larger root under the smaller one with a compare-and-swap on the larger
// root's own entry, so parent[x] <= x always, an entry that has left itself never returns, and
// the last root of a component is its smallest member in whatever order the unions are met.  A
// lost CAS means that another lane hooked that root first: both finds are taken again, which is
// progress of the whole, not a wait for anyone.  Path halving stores an ancestor over an
// ancestor: a stale store lengthens a path, it never leaves the component.  None of this makes
// `parent[i]` a root at any given time: a halving store of another wave may land on an entry
// after its owner has looked its root up.  A kernel that needs roots that stand takes them,
// after the unions, into an array of its own that no find ever stores to.
#pragma once
#include "fs_internal.h"

namespace {

__device__ inline uint32_t uf_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x, with path halving
__device__ inline uint32_t uf_find(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = uf_load(parent + x);
    if (p == x) return x;
    const uint32_t g = uf_load(parent + p);
    if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = g;
  }
}

// true for the one lane whose compare-and-swap joined the two components; false when they were
// one already
__device__ inline bool uf_unite(uint32_t* parent, uint32_t x, uint32_t y) {
  for (;;) {
    x = uf_find(parent, x);
    y = uf_find(parent, y);
    if (x == y) return false;
    if (x > y) {
      const uint32_t t = x;
      x = y;
      y = t;
    }
    if (atomicCAS(parent + y, y, x) == y) return true;   // y was still a root: hooked under x
  }
}

}  // namespace
