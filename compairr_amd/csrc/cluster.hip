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
 *
 * cmpr_cluster_table / cmpr_cluster_table_device: the reference's -c table without the member order of its
 * sweep -- the clusters numbered by (size descending, smallest member ascending), which is the reference's
 * cluster_no - 1 (its qsort compares sizes only and the seeds arrive in increasing order, cluster.cc:53-63,
 * :422), the members of every cluster as CSR, and the summed duplicate_count per cluster.  cluster_links()
 * is the path above up to "labels and sizes flat on the device", shared by both calls; the table pass starts
 * from those two arrays and the two words the host needs, K (the roots) and the largest size:
 *
 *   roots    the i with label[i] == i in increasing i (hipcub DeviceSelect over a counting iterator: it keeps
 *            the order, so the tie-break needs no key bits); table_key_kernel: key = largest - size
 *   order    hipcub's stable LSD radix sort of (key -> root) over the K roots and the bitlen(largest - 1)
 *            bits the keys have
 *   number   table_number_kernel: number[root] = rank, in the words of the size array (read for the last time
 *            by the keys); cluster_start = the exclusive 64-bit sum of the K sorted sizes and a zero (hipcub);
 *            table_of_kernel: cluster_of[i] = number[label[i]], and label[i] = i for the next sort
 *   members  the stable sort of (cluster_of -> i) over bitlen(K - 1) bits, straight into the member array:
 *            increasing inside a cluster because the sort is stable.  One giant cluster costs a sort nothing
 *   counts   table_count_kernel over the members in table order: count[member[p]] of the reference's counts
 *            (context.h cnt2: the set is resident), the run of one cluster summed inside the wave, one 64-bit
 *            add per run and wave.  With ignore_counts the sorted sizes, widened (table_sizes_kernel)
 *
 * Device memory of the table pass beyond cmpr_cluster's 8 bytes per sequence, whose two arrays it reuses (the
 * sizes become the numbers and then the sorted keys, the labels the sequence numbers): per sequence 4 bytes
 * each for cluster_of and the members where the caller gave no device array, and the radix sort's scratch
 * (hipcub: a second pair of arrays, 8 bytes, and its histograms); per cluster 16 bytes (roots and keys,
 * before and behind their sort), 8 for cluster_start and 8 for the counts in the host variant.
 */
#include "context.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>

using namespace cmpr;

namespace {

constexpr uint32_t CLUSTER_WG = 256;

__global__ void __launch_bounds__(CLUSTER_WG)
cluster_init_kernel(uint32_t *parent, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * CLUSTER_WG + threadIdx.x;
  if (i < n)
    parent[i] = (uint32_t)i;
}

/* The forest is final (kernel boundary): plain loads, and nothing is written to it -- a lane's walk does not
   depend on how far another lane has come.  A parent is smaller than its child (link_forest.h link_pair), so the
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

}  // namespace

int cmpr_cluster_forest(cmpr_context *c, uint64_t n, ClusterLinks &L)
{
  int rc;
  if ((rc = dev_alloc(c, L.parent.b, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, L.roots.b, 1))) return rc;
  hipLaunchKernelGGL(cluster_init_kernel, dim3(blocks_for(n, CLUSTER_WG)), dim3(CLUSTER_WG), 0, c->stream,
                     L.parent.b.p, n);
  HIP_TRY(c, hipGetLastError());
  return CMPR_OK;
}

int cmpr_cluster_flatten(cmpr_context *c, uint64_t n, bool want_size, ClusterLinks &L)
{
  int rc;
  if ((rc = L.label.temp(c, (size_t)n))) return rc;
  uint32_t *const parent = L.parent.b.p, *const label = L.label.p;
  const dim3 grid(blocks_for(n, CLUSTER_WG)), wg(CLUSTER_WG);
  HIP_TRY(c, hipMemsetAsync(L.roots.b.p, 0, sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(cluster_flatten_kernel, grid, wg, 0, c->stream, parent, label, n, L.roots.b.p);
  HIP_TRY(c, hipGetLastError());
  if (want_size) {
    /* the counts go where the sizes will be (a device array of the caller) or where the forest was */
    L.size.lend(parent);
    uint32_t *const cnt = L.size.p;
    HIP_TRY(c, hipMemsetAsync(cnt, 0, n * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(cluster_count_kernel, grid, wg, 0, c->stream, label, cnt, n);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(cluster_gather_kernel, grid, wg, 0, c->stream, label, cnt, cnt, n);
    HIP_TRY(c, hipGetLastError());
  }
  L.n = n;
  return CMPR_OK;
}

int cmpr_cluster_results(cmpr_context *c, ClusterLinks &L, uint64_t *n_clusters_out)
{
  const uint64_t n = L.n;
  if (n == 0)
    return CMPR_OK;
  int rc;
  if ((rc = L.size.copy_out(c, (size_t)n))) return rc;
  if ((rc = L.label.copy_out(c, (size_t)n))) return rc;
  unsigned long long clusters = 0;
  HIP_TRY(c, hipMemcpyAsync(&clusters, L.roots.b.p, sizeof clusters, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n_clusters_out)
    *n_clusters_out = clusters;
  return CMPR_OK;
}

namespace {

/* What cmpr_cluster and cmpr_cluster_table share: the refusals, the set as both sets, the link step, the
   flat labels and (want_size) the sizes, all queued on the context's stream and NOT waited for.  n == 0 leaves
   L.n == 0 and nothing queued. */
int cluster_links(cmpr_context *c, const cmpr_set_view *s, bool on_device, bool want_size, uint64_t *n_clusters_out,
                  ClusterLinks &L)
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

  /* parent[i] = i once, before the step: its repeats and its redo pass only add links that are already implied */
  if ((rc = cmpr_cluster_forest(c, n, L))) return rc;
  if ((rc = cmpr_link_step(c, L.parent.b.p)))
    return rc;
  return cmpr_cluster_flatten(c, n, want_size, L);
}

int cluster_impl(cmpr_context *c, const cmpr_set_view *s, bool on_device, uint32_t *label_out,
                 uint32_t *size_out, uint64_t *n_clusters_out)
{
  ClusterLinks L(label_out, size_out, on_device);
  int rc;
  if ((rc = cluster_links(c, s, on_device, L.size.wanted(), n_clusters_out, L)))
    return rc;
  return cmpr_cluster_results(c, L, n_clusters_out);
}

/* ---- the table pass ---- */

struct IsRoot {
  const uint32_t *label;
  __host__ __device__ bool operator()(uint32_t i) const { return label[i] == i; }
};

/* the size of cluster k from its sorted key; a zero behind the last, so that the sum's last word is n */
struct SizeAt {
  const uint32_t *key_sorted;
  uint64_t K;
  uint32_t largest;
  __host__ __device__ unsigned long long operator()(uint64_t k) const { return k < K ? largest - key_sorted[k] : 0u; }
};

__global__ void __launch_bounds__(CLUSTER_WG)
table_key_kernel(const uint32_t *root, const uint32_t *size, uint32_t largest, uint32_t *key, uint64_t K)
{
  const uint64_t k = (uint64_t)blockIdx.x * CLUSTER_WG + threadIdx.x;
  if (k < K)
    key[k] = largest - size[root[k]];
}

__global__ void __launch_bounds__(CLUSTER_WG)
table_number_kernel(const uint32_t *root_sorted, uint32_t *number, uint64_t K)
{
  const uint64_t r = (uint64_t)blockIdx.x * CLUSTER_WG + threadIdx.x;
  if (r < K)
    number[root_sorted[r]] = (uint32_t)r;
}

/* label[i] is read and then overwritten by its own lane only: the labels become the values of the next sort */
__global__ void __launch_bounds__(CLUSTER_WG)
table_of_kernel(uint32_t *label, const uint32_t *number, uint32_t *cluster_of, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * CLUSTER_WG + threadIdx.x;
  if (i < n) {
    cluster_of[i] = number[label[i]];
    label[i] = (uint32_t)i;
  }
}

__global__ void __launch_bounds__(CLUSTER_WG)
table_sizes_kernel(const uint32_t *key_sorted, uint32_t largest, unsigned long long *count, uint64_t K)
{
  const uint64_t k = (uint64_t)blockIdx.x * CLUSTER_WG + threadIdx.x;
  if (k < K)
    count[k] = largest - key_sorted[k];
}

/* count[cluster] += cnt[member] over the members in table order.  The members of a cluster are neighbours now:
   a run of lanes with one cluster is summed inside the wave (every lane takes what lies `off` lanes above it
   while that is still inside its run; after six rounds the run's first lane holds the run's sum) and added
   once.  Integer sums: the order of the adds does not show. */
__global__ void __launch_bounds__(CLUSTER_WG)
table_count_kernel(const uint32_t *cluster_at, const uint32_t *member, const uint64_t *cnt,
                   unsigned long long *count, uint64_t n)
{
  const uint64_t p = (uint64_t)blockIdx.x * CLUSTER_WG + threadIdx.x;
  const uint32_t lane = lane_id();
  const bool valid = p < n;
  const uint32_t mine = valid ? cluster_at[p] : 0u;
  unsigned long long v = valid ? cnt[member[p]] : 0ull;
  const uint32_t prev = __shfl_up(mine, 1, WAVE);
  const bool head = valid && (lane == 0 || prev != mine);
  const uint64_t heads = __ballot(head), valids = __ballot(valid);
  /* the lane's run ends before the next head, or with the last valid lane */
  const uint64_t above = lane == WAVE - 1 ? 0ull : heads >> (lane + 1);
  const uint32_t end = above ? lane + 1 + (uint32_t)__ffsll((unsigned long long)above) - 1
                             : (uint32_t)__popcll(valids);
  for (uint32_t off = 1; off < WAVE; off <<= 1) {
    const unsigned long long other = __shfl_down(v, off, WAVE);
    if (lane + off < end)
      v += other;
  }
  if (head)
    atomicAdd(count + mine, v);
}

int bit_length(uint64_t x)
{
  return x ? 64 - __builtin_clzll(x) : 0;
}

}  // namespace

int cmpr_cluster_table_pass(cmpr_context *c, ClusterLinks &L, const uint64_t *d_cnt, ClusterTableOut &T,
                            uint64_t *n_clusters_out, std::chrono::steady_clock::time_point t0, double *flat_ms)
{
  int rc;
  const uint64_t n = L.n;
  if (n == 0) {
    if (T.cluster_start.wanted()) {
      HIP_TRY(c, hipSetDevice(c->device));
      if ((rc = T.cluster_start.zero(c, 1))) return rc;
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return CMPR_OK;
  }
  uint32_t *const label = L.label.p, *const size = L.size.p;

  /* ---- the two words the host needs: the number of roots, the largest size ---- */
  Tmp<uint32_t> largest_word;
  Tmp<char> scratch;
  size_t scratch_bytes = 0;
  if ((rc = dev_alloc(c, largest_word.b, 1))) return rc;
  HIP_TRY(c, hipcub::DeviceReduce::Max(nullptr, scratch_bytes, (const uint32_t *)size, largest_word.b.p, n, c->stream));
  if ((rc = dev_alloc(c, scratch.b, scratch_bytes))) return rc;
  HIP_TRY(c, hipcub::DeviceReduce::Max(scratch.b.p, scratch_bytes, (const uint32_t *)size, largest_word.b.p, n, c->stream));
  unsigned long long clusters = 0;
  uint32_t largest = 0;
  HIP_TRY(c, hipMemcpyAsync(&clusters, L.roots.b.p, sizeof clusters, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&largest, largest_word.b.p, sizeof largest, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *flat_ms = ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  const uint64_t K = clusters;
  if (K == 0 || K > n || largest == 0 || largest > n)
    return fail(c, CMPR_EDEVICE, "cmpr_cluster_table: the labels and sizes do not describe a partition");
  if (n_clusters_out)
    *n_clusters_out = K;

  /* what has to be made for what was asked for */
  const bool sum_counts = T.count.wanted() && !c->opt.ignore_counts;
  const bool want_members = T.member.wanted() || sum_counts;
  const bool want_of = T.cluster_of.wanted() || want_members;
  if (!want_of && !T.cluster_start.wanted() && !T.count.wanted())
    return CMPR_OK;
  if (sum_counts && !d_cnt)
    return fail(c, CMPR_ESTATE, "cmpr_cluster_table: the resident set has no counts");

  Tmp<uint32_t> root, key, root_sorted, key_sorted;
  Tmp<unsigned long long> selected;      /* DeviceSelect's count, never read: K is the flatten kernel's */
  if ((rc = dev_alloc(c, root.b, (size_t)K))) return rc;
  if ((rc = dev_alloc(c, key.b, (size_t)K))) return rc;
  if ((rc = dev_alloc(c, root_sorted.b, (size_t)K))) return rc;
  if ((rc = dev_alloc(c, key_sorted.b, (size_t)K))) return rc;
  if ((rc = dev_alloc(c, selected.b, 1))) return rc;
  /* (cluster_of and member are made for the arrays that need them, whether or not the caller asked) */
  if (want_of && (rc = T.cluster_of.temp(c, (size_t)n))) return rc;
  if (want_members && (rc = T.member.temp(c, (size_t)n))) return rc;
  if (T.cluster_start.wanted() && (rc = T.cluster_start.temp(c, (size_t)(K + 1)))) return rc;
  if (T.count.wanted() && (rc = T.count.temp(c, (size_t)K))) return rc;
  uint32_t *const cluster_of = T.cluster_of.p, *const member = T.member.p;
  unsigned long long *const cluster_start = (unsigned long long *)T.cluster_start.p;
  unsigned long long *const count = (unsigned long long *)T.count.p;

  /* one scratch buffer for the four hipcub calls, which run one after the other */
  const int size_bits = std::max(1, bit_length(largest - 1)), number_bits = std::max(1, bit_length(K - 1));
  const hipcub::CountingInputIterator<uint32_t> numbers(0);
  const hipcub::TransformInputIterator<unsigned long long, SizeAt, hipcub::CountingInputIterator<uint64_t>>
      sorted_sizes(hipcub::CountingInputIterator<uint64_t>(0), SizeAt{key_sorted.b.p, K, largest});
  size_t select_bytes = 0, order_bytes = 0, scan_bytes = 0, member_bytes = 0;
  HIP_TRY(c, hipcub::DeviceSelect::If(nullptr, select_bytes, numbers, root.b.p, selected.b.p, (int64_t)n,
                                      IsRoot{label}, c->stream));
  HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, order_bytes, (const uint32_t *)key.b.p, key_sorted.b.p,
                                                (const uint32_t *)root.b.p, root_sorted.b.p, (size_t)K, 0, size_bits,
                                                c->stream));
  if (cluster_start)
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, sorted_sizes, cluster_start, (size_t)(K + 1),
                                                c->stream));
  if (want_members)
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, member_bytes, (const uint32_t *)cluster_of, size,
                                                  (const uint32_t *)label, member, (size_t)n, 0, number_bits,
                                                  c->stream));
  scratch_bytes = std::max(std::max(select_bytes, order_bytes), std::max(scan_bytes, member_bytes));
  if ((rc = dev_alloc(c, scratch.b, scratch_bytes))) return rc;

  /* ---- roots and keys; the cluster order ---- */
  HIP_TRY(c, hipcub::DeviceSelect::If(scratch.b.p, select_bytes, numbers, root.b.p, selected.b.p, (int64_t)n,
                                      IsRoot{label}, c->stream));
  hipLaunchKernelGGL(table_key_kernel, dim3(blocks_for(K, CLUSTER_WG)), dim3(CLUSTER_WG), 0, c->stream,
                     root.b.p, size, largest, key.b.p, K);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(scratch.b.p, order_bytes, (const uint32_t *)key.b.p, key_sorted.b.p,
                                                (const uint32_t *)root.b.p, root_sorted.b.p, (size_t)K, 0, size_bits,
                                                c->stream));

  /* ---- numbering ---- */
  if (cluster_start)
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(scratch.b.p, scan_bytes, sorted_sizes, cluster_start, (size_t)(K + 1),
                                                c->stream));
  if (want_of) {
    uint32_t *const number = size;               /* (the keys have read the sizes: their words are free) */
    hipLaunchKernelGGL(table_number_kernel, dim3(blocks_for(K, CLUSTER_WG)), dim3(CLUSTER_WG), 0, c->stream,
                       root_sorted.b.p, number, K);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(table_of_kernel, dim3(blocks_for(n, CLUSTER_WG)), dim3(CLUSTER_WG), 0, c->stream,
                       label, number, cluster_of, n);
    HIP_TRY(c, hipGetLastError());
  }

  /* ---- members: (cluster_of -> i), stable; the sorted keys (the cluster at every place) take the numbers' words ---- */
  if (want_members)
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(scratch.b.p, member_bytes, (const uint32_t *)cluster_of, size,
                                                  (const uint32_t *)label, member, (size_t)n, 0, number_bits,
                                                  c->stream));

  /* ---- counts ---- */
  if (sum_counts) {
    HIP_TRY(c, hipMemsetAsync(count, 0, (size_t)K * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(table_count_kernel, dim3(blocks_for(n, CLUSTER_WG)), dim3(CLUSTER_WG), 0, c->stream,
                       size, member, d_cnt, count, n);
    HIP_TRY(c, hipGetLastError());
  } else if (count) {
    hipLaunchKernelGGL(table_sizes_kernel, dim3(blocks_for(K, CLUSTER_WG)), dim3(CLUSTER_WG), 0, c->stream,
                       key_sorted.b.p, largest, count, K);
    HIP_TRY(c, hipGetLastError());
  }

  if ((rc = T.cluster_of.copy_out(c, (size_t)n))) return rc;
  if ((rc = T.cluster_start.copy_out(c, (size_t)(K + 1)))) return rc;
  if ((rc = T.member.copy_out(c, (size_t)n))) return rc;
  if ((rc = T.count.copy_out(c, (size_t)K))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->cl_ms[1] = ms_since(t0);
  return CMPR_OK;
}

namespace {

int table_impl(cmpr_context *c, const cmpr_set_view *s, bool on_device, uint32_t *cluster_of_out,
               uint64_t *cluster_start_out, uint32_t *member_out, uint64_t *count_out, uint64_t *n_clusters_out)
{
  const auto t0 = std::chrono::steady_clock::now();
  if (c)
    c->cl_ms[0] = c->cl_ms[1] = 0;
  ClusterLinks L(nullptr, nullptr, on_device);
  ClusterTableOut T(cluster_of_out, cluster_start_out, member_out, count_out, on_device);
  int rc;
  if ((rc = cluster_links(c, s, on_device, true, n_clusters_out, L)))
    return rc;
  /* the set is resident: its counts are the reference's (context.h cnt2) */
  return cmpr_cluster_table_pass(c, L, c->cnt2.p, T, n_clusters_out, t0, &c->cl_ms[0]);
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

extern "C" int cmpr_cluster_table(cmpr_context *c, const cmpr_set_view *set, uint32_t *cluster_of_out,
                                  uint64_t *cluster_start_out, uint32_t *member_out, uint64_t *count_out,
                                  uint64_t *n_clusters_out)
{
  return guarded(c, [&] {
    return table_impl(c, set, false, cluster_of_out, cluster_start_out, member_out, count_out, n_clusters_out);
  });
}

extern "C" int cmpr_cluster_table_device(cmpr_context *c, const cmpr_set_view *d_set, uint32_t *d_cluster_of_out,
                                         uint64_t *d_cluster_start_out, uint32_t *d_member_out, uint64_t *d_count_out,
                                         uint64_t *n_clusters_out)
{
  return guarded(c, [&] {
    return table_impl(c, d_set, true, d_cluster_of_out, d_cluster_start_out, d_member_out, d_count_out, n_clusters_out);
  });
}
