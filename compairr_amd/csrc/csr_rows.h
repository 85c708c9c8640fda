/*
 * csr_rows.h -- the passes over CSR rows of hits that neighbors.hip, existence.hip and allpairs.hip share: every row
 * sorted in place by a key of its hits, on one of four paths by the row's length n.  The thresholds are what each path
 * holds, and this is their only definition: the census that sizes the lists (rows_census_kernel) counts by them.
 *
 *   n <= 1              nothing.  Real data: most rows.
 *   n <= LANE_MAX = 8   one lane per row, the row in eight registers, a 19-comparator network
 *                       (rows_sort_short_kernel).  Eight is where real data ends (20 000 CDR3 against themselves,
 *                       d = 1 -i: longest row 9), a network of 16 costs 60 comparators for every lane of a
 *                       wave that has one such row, and neighbouring lanes read neighbouring rows.
 *   n <= WAVE = 64      one element per lane, a bitonic sort with 21 shuffle steps (two shuffles each for a 64-bit
 *                       key); the wave takes the rows of its 64 lanes that need it one after the other (same
 *                       kernel).  No LDS, no workgroup.
 *   n <= LDS_MAX = 8192 one workgroup of 256 lanes per row, bitonic in LDS over the next power of two
 *                       (rows_sort_lds_kernel).  With 32-bit keys that is 32 KiB of the CU's 160, which leaves room
 *                       for four such workgroups per CU (with 40 960 words one would fit); at 8192 words a
 *                       single-workgroup bitonic sort is 91 passes of 32 elements per lane, and beyond that the
 *                       device-wide radix sort, which has the whole GPU for one row, is the better tool.  With
 *                       64-bit keys 8192 of them are 64 KiB -- what a workgroup may declare statically, and two
 *                       such workgroups still fit the CU; a lane reads s[t] and s[t ^ j] as 8-byte words at
 *                       consecutive t: a half-wave covers one 256-byte bank row, no conflict.  These rows are
 *                       listed by the short-row kernel (big_rows: the census sized the list exactly), so rows of 0
 *                       and 1 cost a lane, not a workgroup.
 *   longer              no limit: the rows' (start, length, row) are listed too, come to the host (24 bytes per
 *                       such row, rows_fetch_long) and the caller hands each to hipcub, the whole GPU for one row.
 *                       A handful of rows in skewed data.
 *
 * What differs between the callers is a policy struct `Rows`, passed to the kernels by value.  It owns the arrays of
 * the edges -- the hits, and whatever lies beside each hit -- and the passes know positions only:
 *
 *   Key, PAD            the sort key of a position, and a value above every key (behind a row's end while it is sorted)
 *   load(pos)           the key of what lies at position `pos` of the edges
 *   store(pos, key)     the element that key stands for, put at `pos`
 *   COUNT_HEADS         whether the sorted row's heads -- the positions p with !same_run(key[p - 1], key[p]), and
 *                       position 0 -- are counted into ncell[row].  With it the short kernel runs over n + 1 lanes
 *                       and writes every word of ncell[0 .. n]: the heads of the rows it sorted, 0 for the listed
 *                       rows (the LDS kernel adds theirs) and for the word behind the last row.
 */
#ifndef COMPAIRR_AMD_CSR_ROWS_H
#define COMPAIRR_AMD_CSR_ROWS_H

#include "context.h"

#include <hipcub/hipcub.hpp>

namespace cmpr {

constexpr uint32_t ROW_WG = 256;
constexpr uint32_t LANE_MAX = 8;
constexpr uint32_t LDS_MAX = 8192;
constexpr uint32_t LONG_WORDS = 3;      /* of a long_desc entry: start, length, row */

/* the lists of the rows beyond a wave, as the kernels see them: big_cap and long_cap are what the census counted,
   ctr[0] / ctr[1] the entries taken so far (zero before the short kernel) */
struct RowLists {
  uint32_t           *big_rows;
  uint64_t            big_cap;
  unsigned long long *long_desc;
  uint64_t            long_cap;
  unsigned long long *ctr;
};

template <typename Key>
__device__ __forceinline__ void row_cx(Key &a, Key &b)
{
  const Key lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

/* 19 comparators in 6 layers (Knuth, TAOCP 3, 5.3.4) */
template <typename Key>
__device__ __forceinline__ void row_sort8(Key (&v)[LANE_MAX])
{
  row_cx(v[0], v[1]); row_cx(v[2], v[3]); row_cx(v[4], v[5]); row_cx(v[6], v[7]);
  row_cx(v[0], v[2]); row_cx(v[1], v[3]); row_cx(v[4], v[6]); row_cx(v[5], v[7]);
  row_cx(v[1], v[2]); row_cx(v[5], v[6]); row_cx(v[0], v[4]); row_cx(v[3], v[7]);
  row_cx(v[1], v[5]); row_cx(v[2], v[6]);
  row_cx(v[1], v[4]); row_cx(v[3], v[6]);
  row_cx(v[2], v[4]); row_cx(v[3], v[5]);
  row_cx(v[3], v[4]);
}

/* one key per lane in, the wave's keys in increasing order of the lane out */
template <typename Key>
__device__ __forceinline__ Key wave_sort(Key v, uint32_t lane)
{
  for (uint32_t k = 2; k <= WAVE; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      const Key other = __shfl_xor(v, j, WAVE);
      const bool up = (lane & k) == 0, low = (lane & j) == 0;
      v = (up == low) ? (v < other ? v : other) : (v < other ? other : v);
    }
  return v;
}

/* Every lane brings its row.  The rows of this wave's lanes whose length lies in (LANE_MAX, WAVE], one after the
   other and by the whole wave: f(the row's lane, its start, its length). */
template <typename F>
__device__ __forceinline__ void for_each_wave_row(uint64_t start, uint64_t len, F f)
{
  uint64_t todo = __ballot(len > LANE_MAX && len <= WAVE);
  while (todo) {
    const uint32_t src = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
    todo &= todo - 1;
    const uint64_t s = __shfl(start, src, WAVE);
    f(src, s, (uint32_t)__shfl(len, src, WAVE));
  }
}

/* One lane per row.  Rows of 2 .. LANE_MAX: sorted by their lane.  Rows of up to WAVE: by the wave, one after the
   other.  Longer rows: listed for rows_sort_lds_kernel (big_rows, as many as the census counted) or, beyond LDS,
   with start, length and row for the host (long_desc); the order of the lists is that of arrival and does not
   show in the result. */
template <typename Rows>
__global__ void __launch_bounds__(ROW_WG)
rows_sort_short_kernel(const uint64_t *row_start, uint64_t n, const RowLists L, const Rows R)
{
  using Key = typename Rows::Key;
  const uint64_t i = (uint64_t)blockIdx.x * ROW_WG + threadIdx.x;
  const uint32_t lane = lane_id();
  uint64_t start = 0, len = 0;
  if (i < n) {
    start = row_start[i];
    len = row_start[i + 1] - start;
  }
  [[maybe_unused]] uint32_t cells = len == 1 ? 1u : 0u;
  if (len >= 2 && len <= LANE_MAX) {
    Key v[LANE_MAX];
#pragma unroll
    for (uint32_t k = 0; k < LANE_MAX; k++)
      v[k] = k < len ? R.load(start + k) : Rows::PAD;
    row_sort8(v);
    cells = 1;
#pragma unroll
    for (uint32_t k = 0; k < LANE_MAX; k++)
      if (k < len) {
        R.store(start + k, v[k]);
        if constexpr (Rows::COUNT_HEADS)
          if (k > 0 && !Rows::same_run(v[k - 1], v[k]))
            cells++;
      }
  } else if (len > WAVE) {
    if (len > LDS_MAX) {
      const unsigned long long k = atomicAdd(L.ctr + 1, 1ull);
      if (k < L.long_cap) {
        L.long_desc[LONG_WORDS * k] = start;
        L.long_desc[LONG_WORDS * k + 1] = len;
        L.long_desc[LONG_WORDS * k + 2] = i;
      }
    } else {
      const unsigned long long k = atomicAdd(L.ctr + 0, 1ull);
      if (k < L.big_cap)
        L.big_rows[k] = (uint32_t)i;
    }
  }
  for_each_wave_row(start, len, [&](uint32_t src, uint64_t s, uint32_t m) {
    const Key v = wave_sort(lane < m ? R.load(s + lane) : Rows::PAD, lane);
    if constexpr (Rows::COUNT_HEADS) {
      const Key before = __shfl_up(v, 1, WAVE);
      const uint64_t heads = __ballot(lane < m && (lane == 0 || !Rows::same_run(before, v)));
      if (lane == src)
        cells = (uint32_t)__popcll(heads);
    }
    if (lane < m)
      R.store(s + lane, v);
  });
  if constexpr (Rows::COUNT_HEADS)
    if (i <= n)
      R.ncell[i] = cells;
}

/* One workgroup per listed row of WAVE + 1 .. LDS_MAX hits: bitonic in LDS over the next power of two. */
template <typename Rows>
__global__ void __launch_bounds__(ROW_WG)
rows_sort_lds_kernel(const uint64_t *row_start, const uint32_t *big_rows, const Rows R)
{
  using Key = typename Rows::Key;
  __shared__ Key s[LDS_MAX];
  const uint32_t row = big_rows[blockIdx.x];
  const uint64_t start = row_start[row];
  const uint64_t len64 = row_start[row + 1] - start;
  if (len64 > LDS_MAX)
    return;                                  /* (the list holds no such row; nothing is indexed beyond s) */
  const uint32_t len = (uint32_t)len64;
  uint32_t np = 2 * WAVE;
  while (np < len)
    np <<= 1;
  for (uint32_t t = threadIdx.x; t < np; t += ROW_WG)
    s[t] = t < len ? R.load(start + t) : Rows::PAD;
  __syncthreads();
  for (uint32_t k = 2; k <= np; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < np; t += ROW_WG) {
        const uint32_t u = t ^ j;
        if (u > t) {
          const Key a = s[t], b = s[u];
          if (((t & k) == 0) == (a > b)) {
            s[t] = b;
            s[u] = a;
          }
        }
      }
      __syncthreads();
    }
  [[maybe_unused]] uint32_t heads = 0;
  for (uint32_t t = threadIdx.x; t < len; t += ROW_WG) {
    R.store(start + t, s[t]);
    if constexpr (Rows::COUNT_HEADS)
      if (t == 0 || !Rows::same_run(s[t - 1], s[t]))
        heads++;
  }
  if constexpr (Rows::COUNT_HEADS) {
#pragma unroll
    for (uint32_t off = WAVE / 2; off > 0; off >>= 1)
      heads += __shfl_xor(heads, off, WAVE);
    if (lane_id() == 0 && heads)
      atomicAdd(R.ncell + row, heads);         /* (zero since the short kernel; four adders, integers) */
  }
}

/* ---- host ---- */

/* both kernels over the n rows; L.ctr is zero */
template <typename Rows>
int rows_sort(cmpr_context *c, const uint64_t *row_start, uint64_t n, const RowLists &L, const Rows &R)
{
  const uint64_t lanes = n + (Rows::COUNT_HEADS ? 1 : 0);
  hipLaunchKernelGGL(rows_sort_short_kernel<Rows>, dim3(blocks_for(lanes, ROW_WG)), dim3(ROW_WG), 0, c->stream,
                     row_start, n, L, R);
  HIP_TRY(c, hipGetLastError());
  if (L.big_cap) {
    hipLaunchKernelGGL(rows_sort_lds_kernel<Rows>, dim3((uint32_t)L.big_cap), dim3(ROW_WG), 0, c->stream, row_start,
                       L.big_rows, R);
    HIP_TRY(c, hipGetLastError());
  }
  return CMPR_OK;
}

/* a row beyond LDS as rows_sort_short_kernel listed it */
struct LongRow {
  uint64_t start, len, row;
};

/* The listed long rows on the host (one wait), each checked against what the census and the sum said: no longer
   than `longest`, inside the `total` hits, a row of the n rows.  `who`: the entry point, for the message. */
inline int rows_fetch_long(cmpr_context *c, const RowLists &L, uint64_t longest, uint64_t total, uint64_t n,
                           const char *who, std::vector<LongRow> &out)
{
  std::vector<unsigned long long> desc((size_t)(LONG_WORDS * L.long_cap));
  HIP_TRY(c, hipMemcpyAsync(desc.data(), L.long_desc, desc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  out.clear();
  for (uint64_t k = 0; k < L.long_cap; k++) {
    const LongRow r{desc[LONG_WORDS * k], desc[LONG_WORDS * k + 1], desc[LONG_WORDS * k + 2]};
    if (r.len > longest || r.start + r.len > total || r.row >= n)
      return fail(c, CMPR_EDEVICE, std::string(who) + ": a listed row lies outside the hits");
    out.push_back(r);
  }
  return CMPR_OK;
}

/* ---- the rows ordered by the hit itself (neighbors.hip, allpairs.hip) ---- */

/* nothing to gather, nothing kept */
struct HitRows {
  using Key = uint32_t;
  static constexpr Key  PAD = 0xffffffffu;   /* no sequence number (a set has fewer than 2^32 - 64 sequences) */
  static constexpr bool COUNT_HEADS = false;
  uint32_t *hit;
  __device__ Key load(uint64_t pos) const { return hit[pos]; }
  __device__ void store(uint64_t pos, Key key) const { hit[pos] = key; }
  __device__ static bool same_run(Key, Key) { return true; }
};

/* the same order with the distance of each edge (a D) carried along: a row never holds a hit twice, so the low bits
   of the key never decide */
template <typename D>
struct HitDistRows {
  using Key = unsigned long long;
  static constexpr Key  PAD = ~0ull;
  static constexpr bool COUNT_HEADS = false;
  uint32_t *hit;
  D        *dist;
  __device__ Key load(uint64_t pos) const { return (Key)hit[pos] << 8 * sizeof(D) | dist[pos]; }
  __device__ void store(uint64_t pos, Key key) const
  {
    hit[pos] = (uint32_t)(key >> 8 * sizeof(D));
    dist[pos] = (D)key;
  }
  __device__ static bool same_run(Key, Key) { return true; }
};

/* census[0] rows longer than a wave, [1] of those the rows longer than LDS, [2] the longest row when it is
   longer than LDS.  Real data has no such row: a wave that sees none touches nothing. */
static __global__ void __launch_bounds__(ROW_WG)
rows_census_kernel(const uint64_t *row_start, uint64_t n, unsigned long long *census)
{
  const uint64_t i = (uint64_t)blockIdx.x * ROW_WG + threadIdx.x;
  const uint64_t len = i < n ? row_start[i + 1] - row_start[i] : 0;
  const uint64_t big = __ballot(len > WAVE);
  if (!big)
    return;
  const uint64_t lng = __ballot(len > LDS_MAX);
  if (lane_id() == 0) {
    atomicAdd(census + 0, (unsigned long long)__popcll(big));
    if (lng)
      atomicAdd(census + 1, (unsigned long long)__popcll(lng));
  }
  if (len > LDS_MAX)
    atomicMax(census + 2, (unsigned long long)len);
}

/* queued behind what writes row_start: census[0..2] of the n rows, and [3..4], the two list counters, zero */
inline int rows_census(cmpr_context *c, const uint64_t *row_start, uint64_t n, unsigned long long *census)
{
  HIP_TRY(c, hipMemsetAsync(census, 0, 5 * sizeof(unsigned long long), c->stream));
  if (n) {
    hipLaunchKernelGGL(rows_census_kernel, dim3(blocks_for(n, ROW_WG)), dim3(ROW_WG), 0, c->stream, row_start, n, census);
    HIP_TRY(c, hipGetLastError());
  }
  return CMPR_OK;
}

/* The rows of a filled CSR put in increasing order of the hit, `dist` (or NULL: the hits alone) carried along.  Two
   steps, so that a caller allocates before it fills: reserve() once the census has reached the host (n_big rows of
   WAVE + 1 .. LDS_MAX hits, n_long longer ones, the longest of those), run() behind the fill; ctr: census + 3. */
template <typename D>
struct RowOrder {
  uint64_t n_big = 0, n_long = 0, longest = 0;
  Tmp<uint32_t> big_rows, scratch;
  Tmp<unsigned long long> long_desc;
  Tmp<D> dist_scratch;
  Tmp<char> sort_tmp;
  size_t sort_bytes = 0;

  int reserve(cmpr_context *c, uint64_t n_big_, uint64_t n_long_, uint64_t longest_, bool with_dist)
  {
    int rc;
    n_big = n_big_; n_long = n_long_; longest = longest_;
    if (n_big && (rc = dev_alloc(c, big_rows.b, (size_t)n_big))) return rc;
    if (!n_long)
      return CMPR_OK;
    if ((rc = dev_alloc(c, long_desc.b, (size_t)(LONG_WORDS * n_long)))) return rc;
    if ((rc = dev_alloc(c, scratch.b, (size_t)longest))) return rc;
    if (with_dist) {
      if ((rc = dev_alloc(c, dist_scratch.b, (size_t)longest))) return rc;
      HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                    (const D *)nullptr, (D *)nullptr, (size_t)longest, 0, 32, c->stream));
    } else {
      HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                   (size_t)longest, 0, 32, c->stream));
    }
    return dev_alloc(c, sort_tmp.b, sort_bytes);
  }

  /* queued, but for the one wait that brings the list of the rows beyond LDS when there are any: each of those
     through hipcub's device-wide sort into the scratch and back */
  int run(cmpr_context *c, const char *who, const uint64_t *row_start, uint64_t n, uint64_t total,
          unsigned long long *ctr, uint32_t *hit, D *dist)
  {
    int rc;
    const RowLists lists{big_rows.b.p, n_big, long_desc.b.p, n_long, ctr};   /* (counters: zero) */
    if ((rc = dist ? rows_sort(c, row_start, n, lists, HitDistRows<D>{hit, dist})
                   : rows_sort(c, row_start, n, lists, HitRows{hit})))
      return rc;
    if (!n_long)
      return CMPR_OK;
    std::vector<LongRow> lr;
    if ((rc = rows_fetch_long(c, lists, longest, total, n, who, lr)))
      return rc;
    for (const LongRow &r : lr) {
      size_t b = sort_bytes;
      if (dist) {
        HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(sort_tmp.b.p, b, (const uint32_t *)(hit + r.start), scratch.b.p,
                                                      (const D *)(dist + r.start), dist_scratch.b.p, (size_t)r.len, 0,
                                                      32, c->stream));
        HIP_TRY(c, hipMemcpyAsync(dist + r.start, dist_scratch.b.p, (size_t)r.len * sizeof(D), hipMemcpyDeviceToDevice,
                                  c->stream));
      } else {
        HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(sort_tmp.b.p, b, (const uint32_t *)(hit + r.start), scratch.b.p,
                                                     (size_t)r.len, 0, 32, c->stream));
      }
      HIP_TRY(c, hipMemcpyAsync(hit + r.start, scratch.b.p, (size_t)r.len * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                                c->stream));
    }
    return CMPR_OK;
  }
};

}  // namespace cmpr

#endif
