/*
 * neighbors.hip -- who matched whom, as CSR.  cmpr_neighbors / cmpr_neighbors_device: the pairs the reference
 * appends to its list in find_variant_matches (overlap.cc:232-245), per query and in increasing order of the
 * hit: row_start[n1 + 1] and the hits of row i in [row_start[i], row_start[i + 1]).  Exact, the same bits from
 * run to run and under every tunable, and without a capacity the caller has to guess.
 *
 * The resident sets are stepped over twice; the edges never exist anywhere but in their rows:
 *
 *   count   one synchronous step in neighbour mode (kernels.h score_match): degree[query] += 1 per match
 *   scan    row_start = exclusive 64-bit sum of the n1 + 1 degree words (the last one is zero, so
 *           row_start[n1] is the edge count), hipcub; nb_census_kernel counts the rows beyond a wave and
 *           beyond LDS.  The edge count and the census reach the host together: the call's one wait between
 *           the two steps, after which it knows whether `capacity` suffices and what the ordering will need
 *   fill    the step again: slot = row_start[q] + (atomicSub(degree + q, 1) - 1), hit[slot] = the hit.  The
 *           degree words are the cursors; every word is zero afterwards
 *   order   each row sorted in place (below)
 *
 * run_step_and_wait repeats a step whose no-redo shortcut overflowed.  What the first attempt counted or
 * placed must not survive: the hook in front of EVERY attempt zeroes the degrees (count) or sets them to the
 * row lengths again (fill, nb_cursor_kernel).
 *
 * Ordering the rows.  Which hit takes which place of its row depends on the schedule; the set of hits of a
 * row does not, and a row never holds a sequence twice, so sorting the rows makes the result unique.  Four
 * paths by row length n, the thresholds being what each path holds:
 *
 *   n <= 1              nothing.  Real data: most rows.
 *   n <= LANE_MAX = 8   one lane per row, the row in eight registers, a 19-comparator network
 *                       (nb_sort_short_kernel).  Eight is where real data ends (20 000 CDR3 against themselves,
 *                       d = 1 -i: longest row 9), a network of 16 costs 60 comparators for every lane of a
 *                       wave that has one such row, and neighbouring lanes read neighbouring rows.
 *   n <= WAVE = 64      one element per lane, a bitonic sort with 21 shuffle steps; the wave takes the rows
 *                       of its 64 lanes that need it one after the other (same kernel).  No LDS, no workgroup.
 *   n <= LDS_MAX = 8192 one workgroup of 256 lanes per row, bitonic in 32 KiB of LDS over the next power of
 *                       two (nb_sort_lds_kernel).  32 KiB of the CU's 160 leaves room for four such workgroups
 *                       per CU (with 40 960 words one would fit); at 8192 words a single-workgroup bitonic
 *                       sort is 91 passes of 32 elements per lane, and beyond that the device-wide radix
 *                       sort, which has the whole GPU for one row, is the better tool.  These rows are listed
 *                       by the short-row kernel (big_rows: the census sized the list exactly), so rows of 0 and
 *                       1 cost a lane, not a workgroup.
 *   longer              no limit: the rows' (start, length) are listed too, come to the host (16 bytes per
 *                       such row) and each goes through hipcub::DeviceRadixSort into a scratch buffer the
 *                       size of the longest of them and back.  A handful of rows in skewed data.
 *
 * Device memory for the duration of the call: 4 bytes per query (degrees), the scan's scratch, 4 bytes per
 * row beyond a wave, and for rows beyond LDS 16 bytes each plus the longest of them once plus the radix
 * sort's scratch.  The host variant adds what the device variant is handed: 8 bytes per query for row_start
 * and 4 per edge for the hits.  Everything is freed before the call returns, also when it fails.
 *
 * cmpr_neighbor_edges (context.h) hands count, scan and fill -- the rows not ordered -- to a caller inside the
 * library that orders them its own way (existence.hip).
 */
#include "context.h"

#include <hipcub/hipcub.hpp>

#include <chrono>
#include <new>

using namespace cmpr;

namespace {

constexpr uint32_t NB_WG = 256;
constexpr uint32_t LANE_MAX = 8;
constexpr uint32_t LDS_MAX = 8192;
constexpr uint32_t NB_PAD = 0xffffffffu;   /* behind a row's end while it is sorted: no sequence number (n2 < 2^32 - 64) */

template <typename T>
struct Tmp {
  DevBuf<T> b;
  ~Tmp() { b.release(); }
};

struct U32To64 {
  __host__ __device__ unsigned long long operator()(uint32_t v) const { return v; }
};

/* census[0] rows longer than a wave, [1] of those the rows longer than LDS, [2] the longest row when it is
   longer than LDS.  Real data has no such row: a wave that sees none touches nothing. */
__global__ void __launch_bounds__(NB_WG)
nb_census_kernel(const uint32_t *degree, uint64_t n, unsigned long long *census)
{
  const uint64_t i = (uint64_t)blockIdx.x * NB_WG + threadIdx.x;
  const uint32_t d = i < n ? degree[i] : 0u;
  const uint64_t big = __ballot(d > WAVE);
  if (!big)
    return;
  const uint64_t lng = __ballot(d > LDS_MAX);
  if (lane_id() == 0) {
    atomicAdd(census + 0, (unsigned long long)__popcll(big));
    if (lng)
      atomicAdd(census + 1, (unsigned long long)__popcll(lng));
  }
  if (d > LDS_MAX)
    atomicMax(census + 2, (unsigned long long)d);
}

/* the fill step's cursors: the hits of row i still to come */
__global__ void __launch_bounds__(NB_WG)
nb_cursor_kernel(const uint64_t *row_start, uint32_t *degree, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * NB_WG + threadIdx.x;
  if (i < n)
    degree[i] = (uint32_t)(row_start[i + 1] - row_start[i]);
}

__device__ __forceinline__ void nb_cx(uint32_t &a, uint32_t &b)
{
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

/* One lane per row.  Rows of 2 .. LANE_MAX: sorted by their lane.  Rows of up to WAVE: by the wave, one after
   the other.  Longer rows: listed for nb_sort_lds_kernel (big_rows, as many as the census counted) or, beyond
   LDS, with start and length for the host (long_desc); the order of the lists is that of arrival and does not
   show in the result. */
__global__ void __launch_bounds__(NB_WG)
nb_sort_short_kernel(const uint64_t *row_start, uint32_t *hit, uint64_t n, uint32_t *big_rows, uint64_t big_cap,
                     unsigned long long *long_desc, uint64_t long_cap, unsigned long long *list_ctr)
{
  const uint64_t i = (uint64_t)blockIdx.x * NB_WG + threadIdx.x;
  const uint32_t lane = lane_id();
  uint64_t start = 0, len = 0;
  if (i < n) {
    start = row_start[i];
    len = row_start[i + 1] - start;
  }
  if (len >= 2 && len <= LANE_MAX) {
    uint32_t v[LANE_MAX];
#pragma unroll
    for (uint32_t k = 0; k < LANE_MAX; k++)
      v[k] = k < len ? hit[start + k] : NB_PAD;
    /* 19 comparators in 6 layers (Knuth, TAOCP 3, 5.3.4) */
    nb_cx(v[0], v[1]); nb_cx(v[2], v[3]); nb_cx(v[4], v[5]); nb_cx(v[6], v[7]);
    nb_cx(v[0], v[2]); nb_cx(v[1], v[3]); nb_cx(v[4], v[6]); nb_cx(v[5], v[7]);
    nb_cx(v[1], v[2]); nb_cx(v[5], v[6]); nb_cx(v[0], v[4]); nb_cx(v[3], v[7]);
    nb_cx(v[1], v[5]); nb_cx(v[2], v[6]);
    nb_cx(v[1], v[4]); nb_cx(v[3], v[6]);
    nb_cx(v[2], v[4]); nb_cx(v[3], v[5]);
    nb_cx(v[3], v[4]);
#pragma unroll
    for (uint32_t k = 0; k < LANE_MAX; k++)
      if (k < len)
        hit[start + k] = v[k];
  } else if (len > WAVE) {
    if (len > LDS_MAX) {
      const unsigned long long k = atomicAdd(list_ctr + 1, 1ull);
      if (k < long_cap) {
        long_desc[2 * k] = start;
        long_desc[2 * k + 1] = len;
      }
    } else {
      const unsigned long long k = atomicAdd(list_ctr + 0, 1ull);
      if (k < big_cap)
        big_rows[k] = (uint32_t)i;
    }
  }
  /* the wave's rows of LANE_MAX + 1 .. WAVE */
  uint64_t todo = __ballot(len > LANE_MAX && len <= WAVE);
  while (todo) {
    const uint32_t src = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
    todo &= todo - 1;
    const uint64_t s = __shfl(start, src, WAVE);
    const uint32_t m = (uint32_t)__shfl(len, src, WAVE);
    uint32_t v = lane < m ? hit[s + lane] : NB_PAD;
    for (uint32_t k = 2; k <= WAVE; k <<= 1)
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        const uint32_t other = __shfl_xor(v, j, WAVE);
        const bool up = (lane & k) == 0, low = (lane & j) == 0;
        v = (up == low) ? (v < other ? v : other) : (v < other ? other : v);
      }
    if (lane < m)
      hit[s + lane] = v;
  }
}

/* One workgroup per listed row of WAVE + 1 .. LDS_MAX hits: bitonic in LDS over the next power of two. */
__global__ void __launch_bounds__(NB_WG)
nb_sort_lds_kernel(const uint64_t *row_start, uint32_t *hit, const uint32_t *big_rows)
{
  __shared__ uint32_t s[LDS_MAX];
  const uint32_t row = big_rows[blockIdx.x];
  const uint64_t start = row_start[row];
  const uint64_t len64 = row_start[row + 1] - start;
  if (len64 > LDS_MAX)
    return;                                  /* (the list holds no such row; nothing is indexed beyond s) */
  const uint32_t len = (uint32_t)len64;
  uint32_t np = 2 * WAVE;
  while (np < len)
    np <<= 1;
  for (uint32_t t = threadIdx.x; t < np; t += NB_WG)
    s[t] = t < len ? hit[start + t] : NB_PAD;
  __syncthreads();
  for (uint32_t k = 2; k <= np; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < np; t += NB_WG) {
        const uint32_t u = t ^ j;
        if (u > t) {
          const uint32_t a = s[t], b = s[u];
          if (((t & k) == 0) == (a > b)) {
            s[t] = b;
            s[u] = a;
          }
        }
      }
      __syncthreads();
    }
  for (uint32_t t = threadIdx.x; t < len; t += NB_WG)
    hit[start + t] = s[t];
}

uint32_t blocks_for(uint64_t n)
{
  return (uint32_t)((n + NB_WG - 1) / NB_WG);
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

/* ---- count; scan, census ---- the degrees and the scan's scratch are allocated here; row_start[n1 + 1] is device
   memory, host_rows (or NULL) receives a copy in the same wait that brings the edge count and the census */
int nb_count(cmpr_context *c, NeighborEdges &e, uint64_t *row_start, uint64_t *host_rows)
{
  int rc;
  const uint64_t n1 = c->n1;
  /* TEST ONLY (tunable "assume_never_overflows"): the pretence is used up by the first launch it meets; it is
     renewed for the fill step, so that the repeat of either step can be provoked (tests/test_neighbors_gpu.py) */
  e.pretend_no_redo = c->force_no_redo;
  for (double &t : c->nb_ms)
    t = 0;
  if ((rc = dev_alloc(c, e.degree, (size_t)(n1 + 1)))) return rc;
  if ((rc = dev_alloc(c, e.census, 5))) return rc;      /* [0..2] the census, [3..4] the list counters */
  uint32_t *const degree = e.degree.p;
  hipcub::TransformInputIterator<unsigned long long, U32To64, const uint32_t *> wide(degree, U32To64());
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, e.scan_bytes, wide, (unsigned long long *)row_start,
                                              (size_t)(n1 + 1), c->stream));
  if ((rc = dev_alloc(c, e.scan_tmp, e.scan_bytes))) return rc;

  auto t0 = std::chrono::steady_clock::now();
  if ((rc = cmpr_neighbor_step(c, degree, nullptr, nullptr, [&]() -> int {
         HIP_TRY(c, hipMemsetAsync(degree, 0, (size_t)(n1 + 1) * sizeof(uint32_t), c->stream));
         return CMPR_OK;
       })))
    return rc;
  c->nb_ms[0] = ms_since(t0);

  t0 = std::chrono::steady_clock::now();
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(e.scan_tmp.p, e.scan_bytes, wide, (unsigned long long *)row_start,
                                              (size_t)(n1 + 1), c->stream));
  HIP_TRY(c, hipMemsetAsync(e.census.p, 0, 5 * sizeof(unsigned long long), c->stream));
  if (n1) {
    hipLaunchKernelGGL(nb_census_kernel, dim3(blocks_for(n1)), dim3(NB_WG), 0, c->stream, degree, n1, e.census.p);
    HIP_TRY(c, hipGetLastError());
  }
  unsigned long long total = 0, seen[3] = {0, 0, 0};
  HIP_TRY(c, hipMemcpyAsync(&total, row_start + n1, sizeof total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(seen, e.census.p, sizeof seen, hipMemcpyDeviceToHost, c->stream));
  if (host_rows)
    HIP_TRY(c, hipMemcpyAsync(host_rows, row_start, (size_t)(n1 + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                              c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->nb_ms[1] = ms_since(t0);
  e.total = total;
  e.n_long = seen[1];
  e.n_big = seen[0] - seen[1];
  e.longest = seen[2];
  return CMPR_OK;
}

/* ---- fill ---- every hit into its row, in the order of arrival */
int nb_fill(cmpr_context *c, NeighborEdges &e, const uint64_t *row_start, uint32_t *hit)
{
  int rc;
  const uint64_t n1 = c->n1;
  uint32_t *const degree = e.degree.p;
  if (e.pretend_no_redo) {
    c->force_no_redo = true;
    c->usage_pending = false;
  }
  const auto t0 = std::chrono::steady_clock::now();
  if ((rc = cmpr_neighbor_step(c, degree, row_start, hit, [&]() -> int {
         hipLaunchKernelGGL(nb_cursor_kernel, dim3(blocks_for(n1)), dim3(NB_WG), 0, c->stream, row_start, degree, n1);
         HIP_TRY(c, hipGetLastError());
         return CMPR_OK;
       })))
    return rc;
  c->nb_ms[2] = ms_since(t0);
  return CMPR_OK;
}

int neighbors_impl(cmpr_context *c, uint64_t capacity, uint64_t *row_start_out, uint32_t *hit_out,
                   uint64_t *n_edges_out, bool on_device)
{
  if (!c)
    return CMPR_EINVAL;
  if (!n_edges_out)
    return fail(c, CMPR_EINVAL, "cmpr_neighbors: n_edges_out is NULL");
  *n_edges_out = 0;
  if (capacity && !hit_out)
    return fail(c, CMPR_EINVAL, "cmpr_neighbors: hit_out is NULL with a capacity");
  int rc;
  if ((rc = cmpr_check_ready(c)))
    return rc;
  if (c->work_shard_count > 1)
    return fail(c, CMPR_EUNSUPPORTED, "cmpr_neighbors: a work shard holds part of each row (work_shard_count > 1)");
  if (c->routed)
    return fail(c, CMPR_EUNSUPPORTED, "cmpr_neighbors: a routed query set holds part of each row "
                                      "(cmpr_set_queries_routed)");
  const uint64_t n1 = c->n1;

  NeighborEdges e;
  uint64_t *row_start = on_device ? row_start_out : nullptr;
  if (!row_start) {
    if ((rc = dev_alloc(c, e.row_start, (size_t)(n1 + 1)))) return rc;
    row_start = e.row_start.p;
  }
  if ((rc = nb_count(c, e, row_start, on_device ? nullptr : row_start_out)))
    return rc;
  const uint64_t total = e.total;
  *n_edges_out = total;
  /* degrees only, nothing to list, or no room for it: row_start says what to allocate */
  if (!hit_out || total == 0 || total > capacity)
    return CMPR_OK;

  const uint64_t n_long = e.n_long, n_big = e.n_big, longest = e.longest;
  Tmp<uint32_t> big_rows, scratch;
  Tmp<unsigned long long> long_desc;
  Tmp<char> sort_tmp;
  size_t sort_bytes = 0;
  uint32_t *hit = on_device ? hit_out : nullptr;
  if (!hit) {
    if ((rc = dev_alloc(c, e.hit, (size_t)total))) return rc;
    hit = e.hit.p;
  }
  if (n_big && (rc = dev_alloc(c, big_rows.b, (size_t)n_big))) return rc;
  if (n_long) {
    if ((rc = dev_alloc(c, long_desc.b, (size_t)(2 * n_long)))) return rc;
    if ((rc = dev_alloc(c, scratch.b, (size_t)longest))) return rc;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                 (size_t)longest, 0, 32, c->stream));
    if ((rc = dev_alloc(c, sort_tmp.b, sort_bytes))) return rc;
  }
  if ((rc = nb_fill(c, e, row_start, hit)))
    return rc;

  /* ---- order the rows ---- */
  auto t0 = std::chrono::steady_clock::now();
  unsigned long long *list_ctr = e.census.p + 3;       /* (zero since the census) */
  hipLaunchKernelGGL(nb_sort_short_kernel, dim3(blocks_for(n1)), dim3(NB_WG), 0, c->stream, row_start, hit, n1,
                     big_rows.b.p, n_big, long_desc.b.p, n_long, list_ctr);
  HIP_TRY(c, hipGetLastError());
  if (n_big) {
    hipLaunchKernelGGL(nb_sort_lds_kernel, dim3((uint32_t)n_big), dim3(NB_WG), 0, c->stream, row_start, hit,
                       big_rows.b.p);
    HIP_TRY(c, hipGetLastError());
  }
  if (n_long) {
    std::vector<unsigned long long> desc((size_t)(2 * n_long));
    HIP_TRY(c, hipMemcpyAsync(desc.data(), long_desc.b.p, desc.size() * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (uint64_t k = 0; k < n_long; k++) {
      const uint64_t start = desc[2 * k], len = desc[2 * k + 1];
      if (len > longest || start + len > total)
        return fail(c, CMPR_EDEVICE, "cmpr_neighbors: a listed row lies outside the hits");
      size_t b = sort_bytes;
      HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(sort_tmp.b.p, b, (const uint32_t *)(hit + start), scratch.b.p,
                                                   (size_t)len, 0, 32, c->stream));
      HIP_TRY(c, hipMemcpyAsync(hit + start, scratch.b.p, (size_t)len * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                                c->stream));
    }
  }
  if (!on_device)
    HIP_TRY(c, hipMemcpyAsync(hit_out, hit, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->nb_ms[3] = ms_since(t0);
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

int cmpr_neighbor_edges(cmpr_context *c, NeighborEdges &e)
{
  int rc;
  if ((rc = dev_alloc(c, e.row_start, (size_t)(c->n1 + 1)))) return rc;
  if ((rc = nb_count(c, e, e.row_start.p, nullptr))) return rc;
  if (e.total == 0)
    return CMPR_OK;
  if ((rc = dev_alloc(c, e.hit, (size_t)e.total))) return rc;
  return nb_fill(c, e, e.row_start.p, e.hit.p);
}

extern "C" int cmpr_neighbors(cmpr_context *c, uint64_t capacity, uint64_t *row_start_out, uint32_t *hit_out,
                              uint64_t *n_edges_out)
{
  return guarded(c, [&] { return neighbors_impl(c, capacity, row_start_out, hit_out, n_edges_out, false); });
}

extern "C" int cmpr_neighbors_device(cmpr_context *c, uint64_t capacity, uint64_t *d_row_start_out,
                                     uint32_t *d_hit_out, uint64_t *n_edges_out)
{
  return guarded(c, [&] { return neighbors_impl(c, capacity, d_row_start_out, d_hit_out, n_edges_out, true); });
}
