/*
 * cluster.hip -- single-linkage clusters of one set.  cmpr_cluster / cmpr_cluster_device: the reference's
 * --cluster (cluster.cc:200-410) without its output order, for a set in host or in device memory.
 *
 * The reference runs the per-query loop of the set against itself, keeps every (seed, hit) pair in adjacency
 * lists and sweeps them breadth-first from each unvisited seed in increasing order (cluster.cc:276-410): a
 * cluster is a connected component, its first printed member the smallest sequence number in it.  Here the
 * pair list does not exist.  The set becomes the resident reference AND the resident queries; one ordinary
 * synchronous step runs in link mode, in which score_match (kernels.h) unites the two sequences of every
 * verified pair in a union-find forest of one word per sequence (link_pair: a root is the smallest number of
 * its tree, whatever the schedule).  What follows is one lane per sequence:
 *
 *   cluster_init_kernel     parent[i] = i                            (before the step; never again)
 *   cluster_flatten_kernel  label[i] = root of i, read-only on the forest; the roots counted per
 *                           workgroup, one atomic each
 *   cluster_count_kernel    cnt[label[i]] += 1, equal labels of neighbouring lanes combined first
 *   cluster_gather_kernel   size[i] = cnt[label[i]], in place
 *
 * Device memory beyond the resident sets: the forest (4 bytes per sequence; once the labels are flat it is
 * reused for the counts unless the caller's size array takes them) and the labels where the caller gave no
 * device array for them (4 bytes per sequence).
 */
#include "context.h"

#include <new>

using namespace cmpr;

namespace {

constexpr uint32_t CLUSTER_WG = 256;

template <typename T>
struct Tmp {
  DevBuf<T> b;
  ~Tmp() { b.release(); }
};

__global__ void __launch_bounds__(CLUSTER_WG)
cluster_init_kernel(uint32_t *parent, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * CLUSTER_WG + threadIdx.x;
  if (i < n)
    parent[i] = (uint32_t)i;
}

/* The forest is final (kernel boundary): plain loads, and nothing is written to it -- a lane's walk does not
   depend on how far another lane has come.  A parent is smaller than its child (kernels.h link_pair), so the
   walk ends at the tree's smallest number.  roots: the number of i with label[i] == i. */
__global__ void __launch_bounds__(CLUSTER_WG)
cluster_flatten_kernel(const uint32_t *parent, uint32_t *label, uint64_t n, unsigned long long *roots)
{
  __shared__ uint32_t block_roots;
  if (threadIdx.x == 0)
    block_roots = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * CLUSTER_WG + threadIdx.x;
  bool is_root = false;
  if (i < n) {
    uint32_t x = (uint32_t)i;
    for (uint32_t p = parent[x]; p != x; p = parent[x])
      x = p;
    label[i] = x;
    is_root = x == (uint32_t)i;
  }
  const uint64_t m = __ballot(is_root);
  if (m && lane_id() == 0)
    atomicAdd(&block_roots, (uint32_t)__popcll(m));
  __syncthreads();
  if (threadIdx.x == 0 && block_roots)
    atomicAdd(roots, (unsigned long long)block_roots);
}

/* cnt[label] += 1 per sequence.  One giant cluster is the common case (1391 of 1500 in the recorded cases):
   all 64 lanes of a wave would add to one word.  A run of neighbouring lanes with one label adds once, by
   its first lane, the length of the run. */
__global__ void __launch_bounds__(CLUSTER_WG)
cluster_count_kernel(const uint32_t *label, uint32_t *cnt, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * CLUSTER_WG + threadIdx.x;
  const uint32_t lane = lane_id();
  const bool valid = i < n;
  const uint32_t mine = valid ? label[i] : 0u;
  const uint32_t prev = __shfl_up(mine, 1, WAVE);
  /* (the lanes at and beyond n are the last of the last wave: they end a run and start none) */
  const bool head = valid && (lane == 0 || prev != mine);
  const uint64_t heads = __ballot(head), valids = __ballot(valid);
  if (head) {
    /* the run ends before the next head, or with the last valid lane */
    const uint64_t above = lane == WAVE - 1 ? 0ull : heads >> (lane + 1);
    const uint32_t end = above ? lane + 1 + (uint32_t)__ffsll((unsigned long long)above) - 1
                               : (uint32_t)__popcll(valids);
    atomicAdd(cnt + mine, end - lane);
  }
}

/* size[i] = cnt[label[i]].  cnt and size may be ONE array: the word of a root is rewritten with its own
   value, the word of any other sequence is read by nobody (only roots are labels) and written by its own lane. */
__global__ void __launch_bounds__(CLUSTER_WG)
cluster_gather_kernel(const uint32_t *label, const uint32_t *cnt, uint32_t *size, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * CLUSTER_WG + threadIdx.x;
  if (i < n)
    size[i] = cnt[label[i]];
}

int cluster_impl(cmpr_context *c, const cmpr_set_view *s, bool on_device, uint32_t *label_out,
                 uint32_t *size_out, uint64_t *n_clusters_out)
{
  if (!c)
    return CMPR_EINVAL;
  if (n_clusters_out)
    *n_clusters_out = 0;
  if (!s)
    return fail(c, CMPR_EINVAL, "set view is NULL");
  if (c->opt.existence)
    return fail(c, CMPR_EINVAL, "cmpr_cluster: clusters are not defined with options.existence");
  if (c->work_shard_count > 1)
    return fail(c, CMPR_EUNSUPPORTED, "cmpr_cluster: the components of work shards do not add up (work_shard_count > 1)");
  /* the set as the reference and as the queries: the paths, checks and messages of the two calls */
  int rc;
  if ((rc = on_device ? cmpr_set_reference_device(c, s, 0) : cmpr_set_reference(c, s, 0)))
    return rc;
  if ((rc = on_device ? cmpr_set_queries_device(c, s) : cmpr_set_queries(c, s)))
    return rc;
  const uint64_t n = s->n;
  if (n == 0)
    return CMPR_OK;
  HIP_TRY(c, hipSetDevice(c->device));

  Tmp<uint32_t> parent, labels;
  Tmp<unsigned long long> roots;
  if ((rc = dev_alloc(c, parent.b, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, roots.b, 1))) return rc;
  uint32_t *label = on_device ? label_out : nullptr;
  if (!label) {
    if ((rc = dev_alloc(c, labels.b, (size_t)n))) return rc;
    label = labels.b.p;
  }
  const dim3 grid((uint32_t)((n + CLUSTER_WG - 1) / CLUSTER_WG)), wg(CLUSTER_WG);

  /* once, before the step: its repeats and its redo pass only add links that are already implied */
  hipLaunchKernelGGL(cluster_init_kernel, grid, wg, 0, c->stream, parent.b.p, n);
  HIP_TRY(c, hipGetLastError());
  if ((rc = cmpr_link_step(c, parent.b.p)))
    return rc;

  HIP_TRY(c, hipMemsetAsync(roots.b.p, 0, sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(cluster_flatten_kernel, grid, wg, 0, c->stream, parent.b.p, label, n, roots.b.p);
  HIP_TRY(c, hipGetLastError());
  if (size_out) {
    /* the counts go where the sizes will be (a device array of the caller) or where the forest was */
    uint32_t *cnt = on_device ? size_out : parent.b.p;
    HIP_TRY(c, hipMemsetAsync(cnt, 0, n * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(cluster_count_kernel, grid, wg, 0, c->stream, label, cnt, n);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(cluster_gather_kernel, grid, wg, 0, c->stream, label, cnt, cnt, n);
    HIP_TRY(c, hipGetLastError());
    if (!on_device)
      HIP_TRY(c, hipMemcpyAsync(size_out, cnt, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  }
  if (!on_device && label_out)
    HIP_TRY(c, hipMemcpyAsync(label_out, label, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  unsigned long long clusters = 0;
  HIP_TRY(c, hipMemcpyAsync(&clusters, roots.b.p, sizeof clusters, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n_clusters_out)
    *n_clusters_out = clusters;
  return CMPR_OK;
}

/* the header promises CMPR_ENOMEM, not an exception across the C boundary */
template <typename F>
int guarded(cmpr_context *c, F call)
{
  try {
    return call();
  } catch (const std::bad_alloc &) {
    return fail(c, CMPR_ENOMEM, "out of host memory");
  }
}

}  // namespace

extern "C" int cmpr_cluster(cmpr_context *c, const cmpr_set_view *set, uint32_t *label_out, uint32_t *size_out,
                            uint64_t *n_clusters_out)
{
  return guarded(c, [&] { return cluster_impl(c, set, false, label_out, size_out, n_clusters_out); });
}

extern "C" int cmpr_cluster_device(cmpr_context *c, const cmpr_set_view *d_set, uint32_t *d_label_out,
                                   uint32_t *d_size_out, uint64_t *n_clusters_out)
{
  return guarded(c, [&] { return cluster_impl(c, d_set, true, d_label_out, d_size_out, n_clusters_out); });
}
