// Lock-free union-find over an int array parent[] in global memory: the connected components of mesh_components.hip (vertices joined by
// faces) and of segment.hip (foreground pixels joined by their neighbours).  Device only; include after common.h.  Everything has internal
// linkage and is __forceinline__: a kernel that uses it compiles to the instructions it had with a private copy.
//
// The forest.  Its members are the indices x with parent[x] >= 0; x is a ROOT when parent[x] == x.  A caller may start from singletons
// (parent[x] = x) or from any forest that already satisfies invariant 1, and may mark cells that are no members with -1.
//
// Precondition: every index passed to a function of this file is a member.  A cell holding -1 (a background pixel of segment.hip) is
// never passed in and, since a member's parent is a member, never reached by a walk.
//
// Invariants, from the first hook to the last:
//   1. parent[x] <= x;
//   2. a root is only ever changed by a compare-and-swap from r to a smaller root (cc_unite);
//   3. a non-root is only ever changed by an atomicMin to one of its ancestors (cc_find), and never becomes a root again.
// So every value in the array only decreases, trees only merge, and the root a component ends with is its lowest index: WHICH unions won
// their compare-and-swap depends on the race, the final root does not.  Once every hook has run the roots are final, and cc_root gives
// every member that lowest index: the label.
//
// No kernel waits for a value another workgroup is to write.  A reader of parent[] that sees an old value sees an older ancestor, which is
// still an ancestor, and the compare-and-swap decides.  One launch of hooks, one of flattening; no host loop.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ int cc_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x's tree as far as this thread can see, with path halving on the way up.
// Terminates: a non-root's parent is strictly below it, so x strictly decreases and is bounded by 0.  The atomicMin writes an ancestor
// of x over x's parent; x is not a root at that point (its parent differed from it, and a root never becomes one again), so it cannot
// undo a hook, and the value only goes down.
__device__ __forceinline__ int cc_find(int *parent, int x) {
  for (;;) {
    const int p = cc_load(&parent[x]);
    if (p == x) return x;
    const int g = cc_load(&parent[p]);
    if (g != p) atomicMin(&parent[x], g);
    x = g;
  }
}

// Puts a and b into one tree: the larger of the two roots goes under the smaller one.
// Terminates: every turn either returns or continues with a strictly smaller (hi, lo) pair.  A failed compare-and-swap means that
// parent[hi] was no longer hi - another thread had ALREADY hooked that root under a smaller one, the progress is made, nothing is
// waited for - and it returns that smaller value, from which the walk goes on.  Indices are bounded below by 0.
__device__ __forceinline__ void cc_unite(int *parent, int a, int b) {
  for (;;) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    const int hi = max(a, b), lo = min(a, b);
    const int seen = atomicCAS(&parent[hi], hi, lo);
    if (seen == hi) return;
    a = seen, b = lo;      // seen < hi
  }
}

// The root of x's tree, read only: the walk of a flatten pass, after the hooks have all run.  It needs no halving and writes nothing on
// the way; a neighbour's store of ITS label into a cell this walk passes through only shortens the walk (the label is the root).
// Terminates: parent[x] < x for a non-root.
__device__ __forceinline__ int cc_root(const int *parent, int x) {
  for (;;) {
    const int p = cc_load(&parent[x]);
    if (p == x) return x;
    x = p;
  }
}

}  // namespace
