/*
 * link_forest.h -- the union-find forest that cmpr_cluster (kernels.h score_match, link mode), cmpr_hamming_cluster and
 * cmpr_edit_cluster (allpairs.h, SINK_LINK) unite their matching pairs in: one 32-bit word per sequence,
 * parent[i] == i before the first link.  Written once, included by both.
 */
#ifndef COMPAIRR_AMD_LINK_FOREST_H
#define COMPAIRR_AMD_LINK_FOREST_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cmpr {

/* The root of x's tree in the forest: parent[r] == r.  Other workgroups, on other XCDs, link
   while this one walks: the words are read with relaxed agent-scope atomic loads (from L2), never plain ones.
   Paths are halved on the way: the only word written is that of a node that already has a parent -- so never
   the word a CAS of link_pair expects --, and it is given its grandparent, an ancestor still. */
__device__ __forceinline__ uint32_t link_root(uint32_t *parent, uint32_t x)
{
  for (;;) {
    const uint32_t p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x)
      return x;
    const uint32_t gp = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (gp != p)
      __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gp;
  }
}

/* Sequences a and b are in one cluster (cluster.cc:276-410 reaches one from the other): their trees become
   one.  Lock-free and order-free.  The ONLY write that gives a node a parent is the CAS below, on a node that
   is its own parent (a root) and towards a SMALLER number; path halving replaces a parent by an ancestor.
   Hence (1) every parent is smaller than its child: no cycles, every walk ends; (2) a root is the smallest
   number of its tree; (3) a stale read names an ancestor, from which the walk goes on to the same root; (4)
   a node that has lost its root status never regains it.  When every link of a component has been made, its
   nodes share one root, and by (2) that root is the component's minimum -- whatever the schedule, and
   however often a link is repeated (a repeated link finds equal roots and writes nothing).  At most n - 1
   CAS succeed per forest; a pair inside one tree costs loads only. */
__device__ __forceinline__ void link_pair(uint32_t *parent, uint32_t a, uint32_t b)
{
  uint32_t ra = link_root(parent, a), rb = link_root(parent, b);
  while (ra != rb) {
    const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    const uint32_t seen = atomicCAS(parent + hi, hi, lo);
    if (seen == hi)
      return;
    /* somebody else gave `hi` a parent first: on from there, and from `lo`, which may have one by now too */
    ra = link_root(parent, seen);
    rb = link_root(parent, lo);
  }
}

}  // namespace cmpr

#endif
