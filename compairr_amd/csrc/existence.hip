/*
 * existence.hip -- the -x table without its zeros.  cmpr_existence_csr / cmpr_existence_csr_device: per query, the
 * set-2 repertoires it has a match in and the integer cmpr_overlap_matrix() holds in that cell on a context with
 * options.existence (overlap.cc:218-231), as CSR: row_start[n1 + 1], and the cells of row i in
 * [row_start[i], row_start[i + 1]) in increasing order of the repertoire.  A post-pass over the neighbour rows of
 * neighbors.hip; no probe kernel knows about it, and the n1 x R2 matrix exists nowhere.
 *
 *   edges    the count step, the sum and the fill step of cmpr_neighbors into temporaries (cmpr_neighbor_edges):
 *            row i holds its hits in the order of arrival.  They are not put in order of the hit.
 *   group    each row sorted in place by (rep2[hit], hit): the key rep << 32 | hit is gathered once and only its
 *            low half is stored back, so a run of equal repertoires is a run of positions.  The cells of a row
 *            are the positions whose repertoire differs from the one before (heads); their number goes where the
 *            row's degree word was (zero since the fill step), counted by whoever sorted the row.
 *   count    row_start = exclusive 64-bit sum of those n1 + 1 words (hipcub).  The cell count reaches the host
 *            -- with the cell offsets of the rows beyond LDS -- in the call's one wait beyond those of the edges.
 *   reduce   only when the cells fit `capacity`: the head of run number k of row i writes the repertoire to
 *            row_start[i] + k, and the scores of the run's hits (kernels.h score_match with f = cnt1[i],
 *            g = cnt2[hit], or 1) are summed into the value there.  Integer sums: the order of the hits inside a
 *            run does not show.  cnt1 is scattered from the query records first (ex_cnt1_kernel; no per-query
 *            array of the caller survives cmpr_set_queries), unless the counts are ignored.
 *   copy-out for the host variant.
 *
 * Both passes over the rows take the paths of csr_rows.h, by the row's number of HITS n, with its thresholds (one
 * census, the one the edges come with, serves both files):
 *
 *   n <= LANE_MAX = 8   one lane per row.  group: rows_sort with the 64-bit key; reduce: the lane walks its row.
 *   n <= WAVE = 64      one hit per lane, the wave takes such rows of its 64 lanes one after the other.  group:
 *                       rows_sort; reduce: heads by ballot, the run sums by a segmented scan of six shuffle steps,
 *                       the last lane of a run stores.  No LDS, no atomics.
 *   n <= LDS_MAX = 8192 one workgroup of 256 lanes per listed row.  group: rows_sort, 64 KiB of LDS.
 *                       reduce: 256 positions per round; a round's heads are counted per wave (ballot) and summed
 *                       over the four waves through 16 bytes of LDS, which ranks every position; the segmented
 *                       scan as above, and the last lane of a run INSIDE a wave adds its sum to the value with
 *                       one atomicAdd (a run crosses waves and rounds).  These rows' values are zeroed by the
 *                       workgroup first; nothing else of value_out is.
 *   longer              on the host, row by row, the whole GPU for each: group = the repertoires gathered,
 *                       hipcub::DeviceRadixSort::SortPairs (key: repertoire, on its significant bits; value: hit),
 *                       the hits copied back, the heads counted; reduce = hipcub::DeviceReduce::ReduceByKey
 *                       straight into the row's cells.  (Ties are not ordered by the hit here: a sum does not ask.)
 *
 * Device memory for the duration of the call: per query 4 bytes (degrees, then cells per row) and 8 (row offsets of
 * the edges), 4 bytes per edge, 8 per query for cnt1 (not with ignore_counts), the sums' scratch, 4 bytes per row
 * of more than 64 hits, and for rows of more than 8192 hits 24 bytes each plus 12 times the longest of them plus the
 * scratch of the sort and of the reduction.  The host variant adds what the device variant is handed: 8 bytes per
 * query, 12 per cell.  Everything is freed before the call returns, also when it fails.
 */
#include "csr_rows.h"

#include <hipcub/hipcub.hpp>

using namespace cmpr;

namespace {

constexpr uint32_t EX_WAVES = ROW_WG / WAVE;

/* the rows grouped by the repertoire of the hit, each row's heads -- its cells -- counted (csr_rows.h) */
struct ExRows {
  using Key = unsigned long long;
  static constexpr Key  PAD = ~0ull;
  static constexpr bool COUNT_HEADS = true;
  uint32_t       *hit;
  const uint32_t *rep2;
  uint32_t       *ncell;
  __device__ Key load(uint64_t pos) const
  {
    const uint32_t h = hit[pos];
    return (Key)rep2[h] << 32 | h;
  }
  __device__ void store(uint64_t pos, Key key) const { hit[pos] = (uint32_t)key; }
  __device__ static bool same_run(Key a, Key b) { return (a >> 32) == (b >> 32); }
};

/* what a hit adds to its cell: score_match (kernels.h) with f the query's count and g the hit's */
struct ExScore {
  const uint64_t *cnt1, *cnt2;          /* NULL with ignore_counts */
  int32_t         score, ignore_counts;
  __device__ __forceinline__ unsigned long long of(unsigned long long f, uint32_t hit) const
  {
    if (ignore_counts)
      return 1;
    const unsigned long long g = cnt2[hit];
    switch (score) {
    case CMPR_SCORE_MIN: case CMPR_SCORE_JACCARD: return f < g ? f : g;
    case CMPR_SCORE_MAX:                          return f > g ? f : g;
    case CMPR_SCORE_MEAN:                         return f + g;
    default:                                      return f * g;
    }
  }
  __device__ __forceinline__ unsigned long long count_of(uint64_t row) const
  {
    return ignore_counts ? 1ull : (unsigned long long)cnt1[row];
  }
};

/* the long rows' values for hipcub: hit -> score, the query's count read where it lies */
struct ExScoreOfHit {
  ExScore         s;
  const uint64_t *f;                    /* cnt1 + row, or NULL */
  __device__ unsigned long long operator()(uint32_t hit) const { return s.of(f ? (unsigned long long)*f : 1ull, hit); }
};

/* cnt1[i] of the resident queries: lanes 0 .. nvalid - 1 of a tile are queries, the rest is padding */
__global__ void __launch_bounds__(ROW_WG)
ex_cnt1_kernel(const TileDesc *tiles, const QueryRec *qrec, uint64_t nslots, uint64_t n1, uint64_t *cnt1)
{
  const uint64_t slot = (uint64_t)blockIdx.x * ROW_WG + threadIdx.x;
  if (slot >= nslots || (uint32_t)(slot % WAVE) >= tiles[slot / WAVE].nvalid)
    return;
  const uint32_t orig = qrec[slot].orig;
  if (orig < n1)
    cnt1[orig] = qrec[slot].cnt;
}

/* bits 0 .. lane of a ballot */
__device__ __forceinline__ uint64_t ex_upto(uint32_t lane)
{
  return ~0ull >> (63u - lane);
}

/* Inclusive sums of v over the lanes of a wave, starting anew at every lane whose bit is set in `heads` (lane 0's
   is, or it starts a wave that continues a run): lane - off lies in the run of `lane` when no head lies in
   (lane - off, lane]. */
__device__ __forceinline__ unsigned long long ex_run_sums(unsigned long long v, uint64_t heads, uint32_t lane)
{
#pragma unroll
  for (uint32_t off = 1; off < WAVE; off <<= 1) {
    const unsigned long long below = __shfl_up(v, off, WAVE);
    if (lane >= off && ((heads >> (lane - off + 1u)) & ((1ull << off) - 1ull)) == 0)
      v += below;
  }
  return v;
}

/* group, rows beyond LDS: the repertoires of a row's hits as sort keys ... */
__global__ void __launch_bounds__(ROW_WG)
ex_gather_rep_kernel(const uint32_t *hit, uint64_t len, const uint32_t *rep2, uint32_t *key)
{
  const uint64_t p = (uint64_t)blockIdx.x * ROW_WG + threadIdx.x;
  if (p < len)
    key[p] = rep2[hit[p]];
}

/* ... and the heads of the sorted keys */
__global__ void __launch_bounds__(ROW_WG)
ex_count_heads_kernel(const uint32_t *key, uint64_t len, uint32_t *out)
{
  const uint64_t p = (uint64_t)blockIdx.x * ROW_WG + threadIdx.x;
  const uint64_t heads = __ballot(p < len && (p == 0 || key[p] != key[p - 1]));
  if (lane_id() == 0 && heads)
    atomicAdd(out, (uint32_t)__popcll(heads));
}

/* reduce, one lane per row: rows of up to LANE_MAX walked by their lane, rows of up to WAVE by the wave */
__global__ void __launch_bounds__(ROW_WG)
ex_reduce_short_kernel(const uint64_t *estart, const uint32_t *hit, const uint32_t *rep2, uint64_t n,
                       const uint64_t *cstart, uint32_t *rep_out, unsigned long long *val_out, const ExScore S)
{
  const uint64_t i = (uint64_t)blockIdx.x * ROW_WG + threadIdx.x;
  const uint32_t lane = lane_id();
  uint64_t start = 0, len = 0, c = 0;
  unsigned long long f = 1;
  if (i < n) {
    start = estart[i];
    len = estart[i + 1] - start;
    if (len) {
      c = cstart[i];
      f = S.count_of(i);
    }
  }
  if (len >= 1 && len <= LANE_MAX) {
    uint32_t cur = 0;
    unsigned long long sum = 0;
    uint64_t at = c;
    for (uint32_t k = 0; k < (uint32_t)len; k++) {
      const uint32_t h = hit[start + k], r = rep2[h];
      if (k > 0 && r != cur) {
        rep_out[at] = cur;
        val_out[at] = sum;
        at++;
        sum = 0;
      }
      cur = r;
      sum += S.of(f, h);
    }
    rep_out[at] = cur;
    val_out[at] = sum;
  }
  for_each_wave_row(start, len, [&](uint32_t src, uint64_t s, uint32_t m) {
    const uint64_t cs = __shfl(c, src, WAVE);
    const unsigned long long fs = __shfl(f, src, WAVE);
    const bool valid = lane < m;
    uint32_t r = 0xffffffffu;
    unsigned long long sc = 0;
    if (valid) {
      const uint32_t h = hit[s + lane];
      r = rep2[h];
      sc = S.of(fs, h);
    }
    const uint32_t before = __shfl_up(r, 1, WAVE);
    const bool head = valid && (lane == 0 || r != before);
    const uint64_t heads = __ballot(head);
    const unsigned long long sum = ex_run_sums(sc, heads, lane);
    const uint64_t at = cs + (uint32_t)__popcll(heads & ex_upto(lane)) - 1u;
    if (head)
      rep_out[at] = r;
    if (valid && (lane + 1 == m || ((heads >> (lane + 1u)) & 1ull)))
      val_out[at] = sum;
  });
}

/* reduce, one workgroup per listed row of WAVE + 1 .. LDS_MAX hits, ROW_WG positions per round */
__global__ void __launch_bounds__(ROW_WG)
ex_reduce_lds_kernel(const uint64_t *estart, const uint32_t *hit, const uint32_t *rep2, const uint32_t *big_rows,
                     const uint64_t *cstart, uint32_t *rep_out, unsigned long long *val_out, const ExScore S)
{
  __shared__ uint32_t wave_heads[2][EX_WAVES];
  const uint32_t row = big_rows[blockIdx.x];
  const uint64_t start = estart[row];
  const uint64_t len64 = estart[row + 1] - start;
  if (len64 > LDS_MAX)
    return;
  const uint32_t len = (uint32_t)len64;
  const uint64_t c = cstart[row];
  const uint32_t cells = (uint32_t)(cstart[row + 1] - c);
  const unsigned long long f = S.count_of(row);
  const uint32_t lane = lane_id(), wave = threadIdx.x / WAVE;
  for (uint32_t t = threadIdx.x; t < cells; t += ROW_WG)
    val_out[c + t] = 0;
  __syncthreads();                           /* (the zeros are in memory before any wave of this workgroup adds) */
  uint32_t base = 0;                         /* heads of the rounds so far */
  for (uint32_t t0 = 0, round = 0; t0 < len; t0 += ROW_WG, round++) {
    const uint32_t t = t0 + threadIdx.x;
    const bool valid = t < len;
    uint32_t r = 0xffffffffu;
    unsigned long long sc = 0;
    if (valid) {
      const uint32_t h = hit[start + t];
      r = rep2[h];
      sc = S.of(f, h);
    }
    uint32_t before = __shfl_up(r, 1, WAVE);
    if (lane == 0 && valid && t > 0)
      before = rep2[hit[start + t - 1]];
    const bool head = valid && (t == 0 || r != before);
    const uint64_t heads = __ballot(head);
    if (lane == 0)
      wave_heads[round & 1u][wave] = (uint32_t)__popcll(heads);
    __syncthreads();
    uint32_t mine = base;
#pragma unroll
    for (uint32_t w = 0; w < EX_WAVES; w++) {
      const uint32_t hw = wave_heads[round & 1u][w];
      mine += w < wave ? hw : 0u;
      base += hw;
    }
    /* a wave's first lane starts a sum whether or not it starts a run */
    const unsigned long long sum = ex_run_sums(sc, heads | 1ull, lane);
    const uint32_t rank = mine + (uint32_t)__popcll(heads & ex_upto(lane)) - 1u;
    if (head && rank < cells)
      rep_out[c + rank] = r;
    if (valid && rank < cells && (lane + 1 == WAVE || t + 1 == len || ((heads >> (lane + 1u)) & 1ull)))
      atomicAdd(val_out + c + rank, sum);
  }
}

int existence_impl(cmpr_context *c, uint64_t capacity, uint64_t *row_start_out, uint32_t *rep_out,
                   uint64_t *value_out, uint64_t *n_cells_out, bool on_device)
{
  if (!c)
    return CMPR_EINVAL;
  if (!n_cells_out)
    return fail(c, CMPR_EINVAL, "cmpr_existence_csr: n_cells_out is NULL");
  *n_cells_out = 0;
  if (capacity && !rep_out)
    return fail(c, CMPR_EINVAL, "cmpr_existence_csr: repertoire_out is NULL with a capacity");
  if (capacity && !value_out)
    return fail(c, CMPR_EINVAL, "cmpr_existence_csr: value_out is NULL with a capacity");
  int rc;
  if ((rc = cmpr_check_ready(c)))
    return rc;
  if (is_f64_score(c->opt))
    return fail(c, CMPR_EINVAL, "cmpr_existence_csr: ratio score needs cmpr_overlap_matrix_f64");
  if (c->work_shard_count > 1)
    return fail(c, CMPR_EUNSUPPORTED, "cmpr_existence_csr: a work shard holds part of each row (work_shard_count > 1)");
  if (c->routed)
    return fail(c, CMPR_EUNSUPPORTED, "cmpr_existence_csr: a routed query set holds part of each row "
                                      "(cmpr_set_queries_routed)");
  const uint64_t n1 = c->n1;
  for (double &t : c->ex_ms)
    t = 0;
  Out<uint64_t> rows(row_start_out, on_device);
  Out<uint32_t> reps(rep_out, on_device);
  Out<uint64_t> vals(value_out, on_device);

  /* ---- edges ---- */
  auto t0 = std::chrono::steady_clock::now();
  NeighborEdges e;
  if ((rc = cmpr_neighbor_edges(c, e)))
    return rc;
  c->ex_ms[0] = ms_since(t0);
  const uint64_t total = e.total, n_big = e.n_big, n_long = e.n_long, longest = e.longest;
  if (total == 0) {
    /* no match at all: every row is empty */
    if (rows.wanted()) {
      if ((rc = rows.zero(c, (size_t)(n1 + 1)))) return rc;
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return CMPR_OK;
  }
  const uint64_t *const estart = e.row_start.p;
  uint32_t *const hit = e.hit.p;
  uint32_t *const ncell = e.degree.p;         /* zero since the fill step */
  const uint32_t *const rep2 = c->rep2.p;

  /* ---- group ---- */
  t0 = std::chrono::steady_clock::now();
  Tmp<uint32_t> big_rows, key_a, key_b, hit_b, runs;
  Tmp<unsigned long long> long_desc;
  Tmp<char> sort_tmp, reduce_tmp;
  size_t sort_bytes = 0;
  if ((rc = rows.temp(c, (size_t)(n1 + 1)))) return rc;
  uint64_t *const cstart = rows.p;
  int rep_bits = 1;
  while (rep_bits < 32 && (c->R2 - 1u) >> rep_bits)
    rep_bits++;
  if (n_big && (rc = dev_alloc(c, big_rows.b, (size_t)n_big))) return rc;
  if (n_long) {
    if ((rc = dev_alloc(c, long_desc.b, (size_t)(LONG_WORDS * n_long)))) return rc;
    if ((rc = dev_alloc(c, key_a.b, (size_t)longest))) return rc;
    if ((rc = dev_alloc(c, key_b.b, (size_t)longest))) return rc;
    if ((rc = dev_alloc(c, hit_b.b, (size_t)longest))) return rc;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                  (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)longest, 0,
                                                  rep_bits, c->stream));
    if ((rc = dev_alloc(c, sort_tmp.b, sort_bytes))) return rc;
  }
  const RowLists lists{big_rows.b.p, n_big, long_desc.b.p, n_long, e.census.p + 3};   /* (counters: zero) */
  if ((rc = rows_sort(c, estart, n1, lists, ExRows{hit, rep2, ncell})))
    return rc;
  std::vector<LongRow> lr;
  if (n_long) {
    if ((rc = rows_fetch_long(c, lists, longest, total, n1, "cmpr_existence_csr", lr)))
      return rc;
    for (const LongRow &r : lr) {
      hipLaunchKernelGGL(ex_gather_rep_kernel, dim3(blocks_for(r.len, ROW_WG)), dim3(ROW_WG), 0, c->stream, hit + r.start,
                         r.len, rep2, key_a.b.p);
      HIP_TRY(c, hipGetLastError());
      size_t b = sort_bytes;
      HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(sort_tmp.b.p, b, (const uint32_t *)key_a.b.p, key_b.b.p,
                                                    (const uint32_t *)(hit + r.start), hit_b.b.p, (size_t)r.len, 0,
                                                    rep_bits, c->stream));
      HIP_TRY(c, hipMemcpyAsync(hit + r.start, hit_b.b.p, (size_t)r.len * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                                c->stream));
      hipLaunchKernelGGL(ex_count_heads_kernel, dim3(blocks_for(r.len, ROW_WG)), dim3(ROW_WG), 0, c->stream, key_b.b.p,
                         r.len, ncell + r.row);
      HIP_TRY(c, hipGetLastError());
    }
  }
  c->ex_ms[1] = ms_since(t0);

  /* ---- count ---- (the scratch of the edges' sum serves: the same n1 + 1 words of the same type) */
  t0 = std::chrono::steady_clock::now();
  hipcub::TransformInputIterator<unsigned long long, U32To64, const uint32_t *> wide(ncell, U32To64());
  size_t scan_bytes = e.scan_bytes;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(e.scan_tmp.p, scan_bytes, wide, (unsigned long long *)cstart,
                                              (size_t)(n1 + 1), c->stream));
  unsigned long long cells = 0;
  HIP_TRY(c, hipMemcpyAsync(&cells, cstart + n1, sizeof cells, hipMemcpyDeviceToHost, c->stream));
  std::vector<uint64_t> cell0(lr.size());              /* where the cells of the rows beyond LDS go */
  for (size_t k = 0; k < lr.size(); k++)
    HIP_TRY(c, hipMemcpyAsync(&cell0[k], cstart + lr[k].row, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  if ((rc = rows.copy_out(c, (size_t)(n1 + 1)))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->ex_ms[2] = ms_since(t0);
  *n_cells_out = cells;
  if (!rep_out || cells > capacity)
    return CMPR_OK;

  /* ---- reduce ---- */
  t0 = std::chrono::steady_clock::now();
  Tmp<uint64_t> cnt1;
  if ((rc = reps.temp(c, (size_t)cells))) return rc;
  if ((rc = vals.temp(c, (size_t)cells))) return rc;
  uint32_t *const d_rep = reps.p;
  unsigned long long *const d_val = (unsigned long long *)vals.p;
  ExScore S{nullptr, nullptr, c->opt.score, c->opt.ignore_counts ? 1 : 0};
  if (!S.ignore_counts) {
    if (!c->cnt2.p)
      return fail(c, CMPR_ESTATE, "cmpr_existence_csr: the reference set has no counts");
    if ((rc = dev_alloc(c, cnt1.b, (size_t)n1))) return rc;
    const uint64_t nslots = (uint64_t)c->ntiles * WAVE;
    hipLaunchKernelGGL(ex_cnt1_kernel, dim3(blocks_for(nslots, ROW_WG)), dim3(ROW_WG), 0, c->stream, c->tiles.p,
                       c->qrec.p, nslots, n1, cnt1.b.p);
    HIP_TRY(c, hipGetLastError());
    S.cnt1 = cnt1.b.p;
    S.cnt2 = c->cnt2.p;
  }
  hipLaunchKernelGGL(ex_reduce_short_kernel, dim3(blocks_for(n1, ROW_WG)), dim3(ROW_WG), 0, c->stream, estart, hit, rep2,
                     n1, cstart, d_rep, d_val, S);
  HIP_TRY(c, hipGetLastError());
  if (n_big) {
    hipLaunchKernelGGL(ex_reduce_lds_kernel, dim3((uint32_t)n_big), dim3(ROW_WG), 0, c->stream, estart, hit, rep2,
                       big_rows.b.p, cstart, d_rep, d_val, S);
    HIP_TRY(c, hipGetLastError());
  }
  if (n_long) {
    using ScoreIt = hipcub::TransformInputIterator<unsigned long long, ExScoreOfHit, const uint32_t *>;
    size_t reduce_bytes = 0;
    HIP_TRY(c, hipcub::DeviceReduce::ReduceByKey(nullptr, reduce_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                 ScoreIt(nullptr, ExScoreOfHit{S, nullptr}),
                                                 (unsigned long long *)nullptr, (uint32_t *)nullptr, hipcub::Sum(),
                                                 (size_t)longest, c->stream));
    if ((rc = dev_alloc(c, reduce_tmp.b, reduce_bytes))) return rc;
    if ((rc = dev_alloc(c, runs.b, 1))) return rc;
    for (size_t k = 0; k < lr.size(); k++) {
      const LongRow &r = lr[k];
      if (cell0[k] > cells)
        return fail(c, CMPR_EDEVICE, "cmpr_existence_csr: a listed row lies outside the cells");
      hipLaunchKernelGGL(ex_gather_rep_kernel, dim3(blocks_for(r.len, ROW_WG)), dim3(ROW_WG), 0, c->stream, hit + r.start,
                         r.len, rep2, key_a.b.p);
      HIP_TRY(c, hipGetLastError());
      size_t b = reduce_bytes;
      HIP_TRY(c, hipcub::DeviceReduce::ReduceByKey(reduce_tmp.b.p, b, (const uint32_t *)key_a.b.p, d_rep + cell0[k],
                                                   ScoreIt(hit + r.start, ExScoreOfHit{S, S.cnt1 ? S.cnt1 + r.row : nullptr}),
                                                   d_val + cell0[k], runs.b.p, hipcub::Sum(), (size_t)r.len, c->stream));
    }
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->ex_ms[3] = ms_since(t0);

  /* ---- copy-out ---- */
  if (!on_device && cells) {
    t0 = std::chrono::steady_clock::now();
    if ((rc = reps.copy_out(c, (size_t)cells))) return rc;
    if ((rc = vals.copy_out(c, (size_t)cells))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->ex_ms[4] = ms_since(t0);
  }
  return CMPR_OK;
}

}  // namespace

extern "C" int cmpr_existence_csr(cmpr_context *c, uint64_t capacity, uint64_t *row_start_out,
                                  uint32_t *repertoire_out, uint64_t *value_out, uint64_t *n_cells_out)
{
  return guarded(c, [&] {
    return existence_impl(c, capacity, row_start_out, repertoire_out, value_out, n_cells_out, false);
  });
}

extern "C" int cmpr_existence_csr_device(cmpr_context *c, uint64_t capacity, uint64_t *d_row_start_out,
                                         uint32_t *d_repertoire_out, uint64_t *d_value_out, uint64_t *n_cells_out)
{
  return guarded(c, [&] {
    return existence_impl(c, capacity, d_row_start_out, d_repertoire_out, d_value_out, n_cells_out, true);
  });
}
