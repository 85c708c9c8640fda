/*
 * allpairs.hip -- the host side of allpairs.h: the refusals, a staged set grouped and packed, the segment count, what
 * the job tables of edit.hip and tcrdist.hip are built from (the length limit, the query form, the lengths of a set),
 * and the drivers around a caller's compare kernel -- the matrix, the neighbours as CSR, the clusters, and the nearest
 * neighbours.
 */
#include "allpairs.h"
#include "csr_rows.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

using namespace cmpr;

/* words per sequence of a group of `len` residues: the next word count the register form is compiled for, or the
   words themselves beyond HAMMING_REG_WORDS */
uint32_t cmpr::stride_of(uint32_t len, uint32_t per_word)
{
  const uint32_t w = std::max<uint32_t>(1, (len + per_word - 1) / per_word);
  static const uint32_t forms[] = {1, 2, 3, 4, 5, 6, 8, 12, HAMMING_REG_WORDS};
  for (uint32_t f : forms)
    if (w <= f)
      return f;
  return w;
}

namespace {

/* ---- grouping and packing ---- */

struct KeyParams {
  const uint64_t *off;
  const uint32_t *v, *j;           /* NULL: not in the key */
  uint64_t        n, n_v, n_j;
  uint64_t       *key;
  uint32_t       *num;
};

__global__ void __launch_bounds__(PAIRS_WG)
hm_key_kernel(const KeyParams K)
{
  const uint64_t i = (uint64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (i >= K.n)
    return;
  uint64_t key = K.off[i + 1] - K.off[i];
  if (K.v)
    key = key * K.n_v + K.v[i];
  if (K.j)
    key = key * K.n_j + K.j[i];
  K.key[i] = key;
  K.num[i] = (uint32_t)i;
}

struct HmPackParams {
  const HmGroup  *groups;
  uint32_t        ngroups, per_word, bits;
  const uint8_t  *res;
  const uint64_t *off;
  const uint32_t *ord;
  uint64_t        words;
  uint32_t       *pk;
};

/* one thread per packed word: its group by the word offsets, its sequence and its place in it from there */
__global__ void __launch_bounds__(PAIRS_WG)
hm_pack_kernel(const HmPackParams K)
{
  const uint64_t w = (uint64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (w >= K.words)
    return;
  uint32_t lo = 0, hi = K.ngroups - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (K.groups[mid].pk_off <= w)
      lo = mid;
    else
      hi = mid - 1;
  }
  const HmGroup g = K.groups[lo];
  const uint64_t rel = w - g.pk_off;
  const uint32_t s = (uint32_t)(rel / g.stride), k = (uint32_t)(rel % g.stride);
  const uint64_t b = K.off[K.ord[g.start + s]];
  uint32_t word = 0;
  const uint32_t p0 = k * K.per_word;
  for (uint32_t t = 0; t < K.per_word && p0 + t < g.len; t++)
    word |= (uint32_t)K.res[b + p0 + t] << (t * K.bits);
  K.pk[w] = word;
}

/* row_start[i] = the offset of (query i, segment 0); row_start[n1] = the edge count */
__global__ void __launch_bounds__(PAIRS_WG)
pairs_rows_kernel(const unsigned long long *offs, uint64_t n1, uint32_t segments, uint64_t *row_start)
{
  const uint64_t i = (uint64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (i <= n1)
    row_start[i] = offs[i * segments];
}

/* the slots of a query folded: the smallest key, and the ties of the slots at its distance summed */
__global__ void __launch_bounds__(PAIRS_WG)
pairs_nearest_fold_kernel(const unsigned long long *key, const uint32_t *slot_ties, uint64_t n1, uint32_t segments,
                       uint32_t *nearest, uint16_t *dist, uint32_t *ties)
{
  const uint64_t i = (uint64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (i >= n1)
    return;
  unsigned long long best = ~0ull;
  for (uint32_t s = 0; s < segments; s++)
    best = min(best, key[i * segments + s]);
  const uint32_t d = (uint32_t)(best >> 32);
  uint32_t t = 0;
  for (uint32_t s = 0; s < segments; s++)
    t += (uint32_t)(key[i * segments + s] >> 32) == d ? slot_ties[i * segments + s] : 0u;
  const bool none = d == HM_NONE;
  if (nearest)
    nearest[i] = none ? HM_NONE : (uint32_t)best;
  if (dist)
    dist[i] = none ? (uint16_t)0xffffu : (uint16_t)d;
  if (ties)
    ties[i] = none ? 0u : t;
}

/* 1 for a query that has a candidate (hipcub::TransformInputIterator over the finished ties) */
struct HasTies {
  __host__ __device__ unsigned long long operator()(uint32_t t) const { return t ? 1ull : 0ull; }
};

}  // namespace

/* the staged set H grouped by `mode` and packed */
int cmpr::hm_prepare(cmpr_context *c, HmSet &H, HmKeyMode mode)
{
  int rc;
  if (H.n == 0)
    return CMPR_OK;
  if (H.n > 0x7fffffffull)
    return fail(c, CMPR_EUNSUPPORTED, "cmpr_hamming: more than 2^31-1 sequences in one set");

  /* keys, the stable sort, the runs */
  const uint64_t n = H.n;
  const bool with_v = mode != HM_KEY_LENGTH, with_j = mode == HM_KEY_LENGTH_V_J;
  const uint64_t n_v = std::max<uint32_t>(1, c->opt.n_v_genes), n_j = std::max<uint32_t>(1, c->opt.n_j_genes);
  H.per_len = (with_v ? n_v : 1) * (with_j ? n_j : 1);
  Tmp<uint64_t> key, key_sorted, run_key;
  Tmp<uint32_t> num, run_len, nruns;
  Tmp<char> scratch;
  if ((rc = dev_alloc(c, key.b, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, key_sorted.b, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, num.b, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, H.ord.b, (size_t)n))) return rc;
  KeyParams K{H.off.b.p, with_v ? H.v.b.p : nullptr, with_j ? H.j.b.p : nullptr, n, n_v, n_j, key.b.p, num.b.p};
  hipLaunchKernelGGL(hm_key_kernel, dim3(blocks_for(n, PAIRS_WG)), dim3(PAIRS_WG), 0, c->stream, K);
  HIP_TRY(c, hipGetLastError());
  const uint64_t key_max = ((uint64_t)H.longest + 1) * H.per_len;
  int end_bit = 1;
  while (end_bit < 64 && (key_max >> end_bit))
    end_bit++;
  size_t sort_bytes = 0, rle_bytes = 0;
  HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint64_t *)key.b.p, key_sorted.b.p,
                                                (const uint32_t *)num.b.p, H.ord.b.p, (size_t)n, 0, end_bit, c->stream));
  if ((rc = dev_alloc(c, run_key.b, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, run_len.b, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, nruns.b, 1))) return rc;
  HIP_TRY(c, hipcub::DeviceRunLengthEncode::Encode(nullptr, rle_bytes, (const uint64_t *)key_sorted.b.p, run_key.b.p,
                                                   run_len.b.p, nruns.b.p, (int)n, c->stream));
  if ((rc = dev_alloc(c, scratch.b, std::max(sort_bytes, rle_bytes)))) return rc;
  HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(scratch.b.p, sort_bytes, (const uint64_t *)key.b.p, key_sorted.b.p,
                                                (const uint32_t *)num.b.p, H.ord.b.p, (size_t)n, 0, end_bit, c->stream));
  HIP_TRY(c, hipcub::DeviceRunLengthEncode::Encode(scratch.b.p, rle_bytes, (const uint64_t *)key_sorted.b.p, run_key.b.p,
                                                   run_len.b.p, nruns.b.p, (int)n, c->stream));
  uint32_t G = 0;
  HIP_TRY(c, hipMemcpyAsync(&G, nruns.b.p, sizeof G, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (G == 0 || G > n)
    return fail(c, CMPR_EDEVICE, "cmpr_hamming: the group count is out of range");
  H.keys.resize(G);
  std::vector<uint32_t> lens(G);
  HIP_TRY(c, hipMemcpyAsync(H.keys.data(), run_key.b.p, (size_t)G * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(lens.data(), run_len.b.p, (size_t)G * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));

  /* the group table; the packed words */
  const uint32_t per_word = c->opt.alphabet_size == 4 ? NT_PER_WORD : AA_PER_WORD;
  H.groups.resize(G);
  uint64_t start = 0, words = 0;
  for (uint32_t g = 0; g < G; g++) {
    HmGroup &x = H.groups[g];
    x.len = (uint32_t)(H.keys[g] / H.per_len);
    x.stride = stride_of(x.len, per_word);
    x.start = (uint32_t)start;
    x.count = lens[g];
    x.pk_off = words;
    start += x.count;
    words += (uint64_t)x.count * x.stride;
  }
  if (start != n || H.groups.back().len > H.longest)
    return fail(c, CMPR_EDEVICE, "cmpr_hamming: the groups do not add up to the set");
  if (words > (1ull << 38))
    return fail(c, CMPR_EUNSUPPORTED, "cmpr_hamming: more than 2^38 packed words in one set");
  Tmp<HmGroup> d_groups;
  if ((rc = dev_upload(c, d_groups.b, H.groups.data(), H.groups.size()))) return rc;
  if ((rc = dev_alloc(c, H.pk.b, (size_t)words))) return rc;
  HmPackParams Q{d_groups.b.p, G, per_word, 32 / per_word, H.res.b.p, H.off.b.p, H.ord.b.p, words, H.pk.b.p};
  hipLaunchKernelGGL(hm_pack_kernel, dim3(blocks_for(words, PAIRS_WG)), dim3(PAIRS_WG), 0, c->stream, Q);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));             /* (d_groups and the sort's temporaries leave scope) */
  return CMPR_OK;
}

/* the refusals */
int cmpr::hm_refusals(cmpr_context *c, const std::string &who, const cmpr_set_view *set1, const cmpr_set_view *set2,
                      int64_t differences, HmKind kind, bool on_device, bool with_indels)
{
  if (differences < 0)
    return fail(c, CMPR_EINVAL, kind == HM_NEAREST ? who + ": min_distance cannot be negative"
                                                   : "Differences specified with -d or -differences cannot be negative.");
  if (c->opt.indels && !with_indels)
    return fail(c, CMPR_EINVAL, who + ": the all-against-all path has no indels");
  if (kind == HM_CLUSTERS && c->opt.existence)
    return fail(c, CMPR_EINVAL, "cmpr_cluster: clusters are not defined with options.existence");
  if (kind == HM_MATRIX && is_f64_score(c->opt))
    return fail(c, CMPR_EINVAL, who + ": ratio score needs cmpr_overlap_matrix_f64");
  if (kind != HM_CLUSTERS && kind != HM_NEAREST && differences > 0 &&
      (c->opt.score == CMPR_SCORE_MH || c->opt.score == CMPR_SCORE_JACCARD))
    return fail(c, CMPR_EINVAL, "The Morisita-Horn / Jaccard index is not defined when d>0");
  std::string why;
  int rc;
  if ((rc = validate_view(c->opt, set1, why, on_device)) || (rc = validate_view(c->opt, set2, why, on_device)))
    return fail(c, rc, why);
  if (c->work_shard_count > 1)
    return fail(c, CMPR_EUNSUPPORTED, who + ": the call sees whole sets, every shard would give the whole answer "
                                      "(work_shard_count > 1)");
  if (!c->opt.ignore_genes &&
      (uint64_t)std::max<uint32_t>(1, c->opt.n_v_genes) * std::max<uint32_t>(1, c->opt.n_j_genes) > (1ull << 46))
    return fail(c, CMPR_EUNSUPPORTED, who + ": (length, V, J) does not fit a 64-bit key (n_v_genes x n_j_genes > 2^46)");
  return CMPR_OK;
}

int cmpr::pairs_stage(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2, bool on_device, PairSets &W,
                      HmKeyMode mode, const std::function<int(const HmSet &)> &check)
{
  int rc;
  const auto stage = [&](const cmpr_set_view *set, HmSet &H) -> int {
    if ((rc = cmpr_stage_set(c, set, on_device, H)) || (check && (rc = check(H))))
      return rc;
    return hm_prepare(c, H, mode);
  };
  if ((rc = stage(set1, W.own1))) return rc;
  W.s1 = W.s2 = &W.own1;
  if (set2 != set1) {
    if ((rc = stage(set2, W.own2))) return rc;
    W.s2 = &W.own2;
  }
  return CMPR_OK;
}

std::function<int(const HmSet &)> cmpr::pairs_length_check(cmpr_context *c, const char *prefix)
{
  return [c, prefix](const HmSet &H) {
    return H.longest > PAIRS_MAX_LEN
        ? fail(c, CMPR_EUNSUPPORTED, std::string(prefix) + ": a sequence of more than 256 residues") : CMPR_OK;
  };
}

uint32_t cmpr::pairs_form_of(uint32_t len, uint32_t stride)
{
  if (len > PAIRS_REG_RESIDUES)
    return 0;
  for (uint32_t f : {2u, 4u, 8u, 16u})
    if (stride <= f)
      return f;
  return 0;
}

cmpr::PairLengths::PairLengths(const HmSet &S)
{
  for (size_t g = 0; g < S.groups.size(); g++)
    if (len.empty() || len.back() != S.groups[g].len) {
      len.push_back(S.groups[g].len);
      first.push_back(g);
    }
}

const HmGroup *cmpr::hm_group_of(const HmSet &S, uint64_t key)
{
  const auto k = std::lower_bound(S.keys.begin(), S.keys.end(), key);
  return k != S.keys.end() && *k == key ? &S.groups[(size_t)(k - S.keys.begin())] : nullptr;
}

int cmpr::pairs_neighbors_args(cmpr_context *c, const std::string &who, uint64_t capacity, const uint32_t *hit_out,
                               uint64_t *n_edges_out)
{
  if (!n_edges_out)
    return fail(c, CMPR_EINVAL, who + ": n_edges_out is NULL");
  *n_edges_out = 0;
  if (capacity && !hit_out)
    return fail(c, CMPR_EINVAL, who + ": hit_out is NULL with a capacity");
  return CMPR_OK;
}

uint32_t cmpr::pairs_segments(const cmpr_context *c, int64_t tunable, uint64_t blocks, uint32_t nr_max,
                              uint32_t longest_piece)
{
  if (tunable)
    return (uint32_t)tunable;
  if (!blocks)
    return 1;
  const uint64_t target = (uint64_t)c->cus * 8;
  uint32_t S = (uint32_t)std::min<uint64_t>(PAIRS_MAX_SEGMENTS, (target + blocks - 1) / blocks);
  S = std::max<uint32_t>(1, std::min<uint32_t>(S, (nr_max + 63) / 64));
  if (longest_piece)
    S = std::max(S, std::min<uint32_t>(PAIRS_MAX_SEGMENTS, (nr_max + longest_piece - 1) / longest_piece));
  return S;
}

int cmpr::pairs_matrix(cmpr_context *c, const PairSets &W, PairSinks &K, void *matrix_out, bool on_device,
                       const std::function<int()> &launch, double *ms, int copy_slot)
{
  int rc;
  auto t0 = std::chrono::steady_clock::now();
  const uint64_t rows = c->opt.existence ? W.s1->n : W.s1->R, cells = rows * W.s2->R;
  if (cells == 0)
    return CMPR_OK;
  Out<unsigned long long> matrix((unsigned long long *)matrix_out, on_device);
  if ((rc = matrix.temp(c, (size_t)cells))) return rc;
  HIP_TRY(c, hipMemsetAsync(matrix.p, 0, cells * sizeof(unsigned long long), c->stream));
  K.rep1 = W.s1->rep.b.p; K.rep2 = W.s2->rep.b.p;
  K.cnt1 = c->opt.ignore_counts ? nullptr : W.s1->cnt.b.p;
  K.cnt2 = c->opt.ignore_counts ? nullptr : W.s2->cnt.b.p;
  K.R2 = W.s2->R;
  K.score = (uint32_t)c->opt.score;
  K.existence = c->opt.existence ? 1u : 0u;
  K.mat_lds = !c->opt.existence && cells <= PAIRS_MAT_CELLS ? 1u : 0u;
  K.matrix = matrix.p;
  K.cells = (uint32_t)std::min<uint64_t>(cells, PAIRS_MAT_CELLS);
  if ((rc = launch()))
    return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  ms[1] = ms_since(t0);
  if (!on_device) {
    t0 = std::chrono::steady_clock::now();
    if ((rc = matrix.copy_out(c, (size_t)cells))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ms[copy_slot] = ms_since(t0);
  }
  return CMPR_OK;
}

int cmpr::pairs_neighbors(cmpr_context *c, const std::string &who, const PairSets &W, uint32_t segments, PairSinks &K,
                          uint64_t capacity, uint64_t *row_start_out, uint32_t *hit_out, uint16_t *dist_out,
                          uint64_t *n_edges_out, bool on_device, const std::function<int()> &launch, bool rows_always,
                          double *ms, int order_slot, int copy_slot)
{
  int rc;
  auto t0 = std::chrono::steady_clock::now();
  /* count per (query, segment); the sum; the rows */
  const uint64_t n1 = W.s1->n, S = segments, slots = n1 * S + 1;       /* (a zero behind the last: the sum's last is the total) */
  if (slots > 0x7fffffffull)
    return fail(c, CMPR_EUNSUPPORTED, who + ": more than 2^31-1 (query, segment) counts");
  Out<uint64_t> rows(row_start_out, on_device);
  Out<uint32_t> hit(hit_out, on_device);
  Out<uint16_t> dist(dist_out, on_device);
  Tmp<uint32_t> cnt;
  Tmp<unsigned long long> offs;
  Tmp<char> scan_tmp;
  if ((rc = dev_alloc(c, cnt.b, (size_t)slots))) return rc;
  if ((rc = dev_alloc(c, offs.b, (size_t)slots))) return rc;
  HIP_TRY(c, hipMemsetAsync(cnt.b.p, 0, slots * sizeof(uint32_t), c->stream));
  K.cnt = cnt.b.p;
  if ((rc = launch()))
    return rc;
  hipcub::TransformInputIterator<unsigned long long, U32To64, const uint32_t *> wide(cnt.b.p, U32To64());
  size_t scan_bytes = 0;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, wide, offs.b.p, (int)slots, c->stream));
  if ((rc = dev_alloc(c, scan_tmp.b, scan_bytes))) return rc;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(scan_tmp.b.p, scan_bytes, wide, offs.b.p, (int)slots, c->stream));
  if (rows_always || rows.wanted()) {
    if ((rc = rows.temp(c, (size_t)(n1 + 1)))) return rc;
    hipLaunchKernelGGL(pairs_rows_kernel, dim3(blocks_for(n1 + 1, PAIRS_WG)), dim3(PAIRS_WG), 0, c->stream, offs.b.p, n1,
                       (uint32_t)S, rows.p);
    HIP_TRY(c, hipGetLastError());
  }
  unsigned long long total = 0;
  HIP_TRY(c, hipMemcpyAsync(&total, offs.b.p + (slots - 1), sizeof total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *n_edges_out = total;

  /* the same walk again, every hit to its place -- when there is room for all of them */
  const bool fill = hit.wanted() && total && total <= capacity;
  if (fill) {
    if ((rc = hit.temp(c, (size_t)total))) return rc;
    if (dist.wanted() && (rc = dist.temp(c, (size_t)total))) return rc;
    K.offs = offs.b.p;
    K.hit = hit.p;
    K.dist = dist.p;
    if ((rc = launch()))
      return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  ms[1] = ms_since(t0);
  if (fill && order_slot >= 0) {
    /* every row in increasing order of the hit (csr_rows.h; the rows beyond LDS by hipcub) */
    t0 = std::chrono::steady_clock::now();
    Tmp<unsigned long long> census;
    RowOrder<uint16_t> order;
    unsigned long long seen[3] = {0, 0, 0};
    if ((rc = dev_alloc(c, census.b, 5))) return rc;       /* [0..2] the census, [3..4] the list counters */
    if ((rc = rows_census(c, rows.p, n1, census.b.p))) return rc;
    HIP_TRY(c, hipMemcpyAsync(seen, census.b.p, sizeof seen, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (seen[1] > seen[0] || seen[0] > n1 || seen[2] > total)
      return fail(c, CMPR_EDEVICE, who + ": the census of the rows is out of range");
    if ((rc = order.reserve(c, seen[0] - seen[1], seen[1], seen[2], dist.p != nullptr))) return rc;
    if ((rc = order.run(c, who.c_str(), rows.p, n1, total, census.b.p + 3, hit.p, dist.p))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));           /* (the temporaries leave scope) */
    ms[order_slot] = ms_since(t0);
  }
  if (!on_device) {
    t0 = std::chrono::steady_clock::now();
    if ((rc = rows.copy_out(c, (size_t)(n1 + 1)))) return rc;
    if (fill) {
      if ((rc = hit.copy_out(c, (size_t)total))) return rc;
      if ((rc = dist.copy_out(c, (size_t)total))) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ms[copy_slot] = ms_since(t0);
  }
  return CMPR_OK;
}

int cmpr::pairs_clusters(cmpr_context *c, const HmSet &S, bool snapshot, bool on_device, ClusterLinks &L,
                         ClusterTableOut *T, uint64_t *n_clusters_out,
                         const std::function<int(const PairLinks &)> &launch, double *ms, int copy_slot)
{
  int rc;
  auto t0 = std::chrono::steady_clock::now();
  const bool table = T != nullptr;
  const uint64_t n = S.n;
  if (n) {
    if ((rc = cmpr_cluster_forest(c, n, L))) return rc;
    if ((rc = launch(PairLinks{L.parent.b.p, snapshot ? 1u : 0u})))
      return rc;
    if ((rc = cmpr_cluster_flatten(c, n, table || L.size.wanted(), L)))
      return rc;
  }
  if (table)
    return cmpr_cluster_table_pass(c, L, c->opt.ignore_counts ? nullptr : S.cnt.b.p, *T, n_clusters_out, t0, &ms[1]);
  if (n && !on_device) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ms[1] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    if ((rc = cmpr_cluster_results(c, L, n_clusters_out)))
      return rc;
    ms[copy_slot] = ms_since(t0);
    return CMPR_OK;
  }
  if ((rc = cmpr_cluster_results(c, L, n_clusters_out)))
    return rc;
  ms[1] = ms_since(t0);
  return CMPR_OK;
}

int cmpr::pairs_nearest(cmpr_context *c, const PairSets &W, uint32_t segments, uint32_t *nearest_out, uint16_t *dist_out,
                        uint32_t *ties_out, uint64_t *n_found_out, bool on_device,
                        const std::function<int(const PairNearest &)> &launch, double *ms, int copy_slot)
{
  int rc;
  auto t0 = std::chrono::steady_clock::now();
  const uint64_t n1 = W.s1->n, S = segments;
  if (n1 == 0)
    return CMPR_OK;
  Out<uint32_t> nearest(nearest_out, on_device);
  Out<uint16_t> dist(dist_out, on_device);
  Out<uint32_t> ties(ties_out, on_device);
  if (nearest.wanted() && (rc = nearest.temp(c, (size_t)n1))) return rc;
  if (dist.wanted() && (rc = dist.temp(c, (size_t)n1))) return rc;
  if ((ties.wanted() || n_found_out) && (rc = ties.temp(c, (size_t)n1))) return rc;
  PairNearest N{};
  Tmp<unsigned long long> key, found;
  Tmp<uint32_t> slot_ties;
  Tmp<char> sum_tmp;
  if (S == 1) {
    /* "none" everywhere first: a query whose group set 2 lacks is no lane's */
    if (nearest.p) HIP_TRY(c, hipMemsetAsync(nearest.p, 0xff, n1 * sizeof(uint32_t), c->stream));
    if (dist.p) HIP_TRY(c, hipMemsetAsync(dist.p, 0xff, n1 * sizeof(uint16_t), c->stream));
    if (ties.p) HIP_TRY(c, hipMemsetAsync(ties.p, 0, n1 * sizeof(uint32_t), c->stream));
    N.nearest = nearest.p; N.dist = dist.p; N.ties = ties.p;
  } else {
    /* ... nor is a (query, segment) whose range is empty: the fold writes every query from its slots */
    if ((rc = dev_alloc(c, key.b, (size_t)(n1 * S)))) return rc;
    if ((rc = dev_alloc(c, slot_ties.b, (size_t)(n1 * S)))) return rc;
    HIP_TRY(c, hipMemsetAsync(key.b.p, 0xff, n1 * S * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipMemsetAsync(slot_ties.b.p, 0, n1 * S * sizeof(uint32_t), c->stream));
    N.key = key.b.p; N.slot_ties = slot_ties.b.p;
  }
  if ((rc = launch(N)))
    return rc;
  if (S > 1) {
    hipLaunchKernelGGL(pairs_nearest_fold_kernel, dim3(blocks_for(n1, PAIRS_WG)), dim3(PAIRS_WG), 0, c->stream,
                       (const unsigned long long *)key.b.p, (const uint32_t *)slot_ties.b.p, n1, (uint32_t)S,
                       nearest.p, dist.p, ties.p);
    HIP_TRY(c, hipGetLastError());
  }
  unsigned long long n_found = 0;
  if (n_found_out) {
    hipcub::TransformInputIterator<unsigned long long, HasTies, const uint32_t *> has(ties.p, HasTies());
    size_t sum_bytes = 0;
    if ((rc = dev_alloc(c, found.b, 1))) return rc;
    HIP_TRY(c, hipcub::DeviceReduce::Sum(nullptr, sum_bytes, has, found.b.p, (int)n1, c->stream));
    if ((rc = dev_alloc(c, sum_tmp.b, sum_bytes))) return rc;
    HIP_TRY(c, hipcub::DeviceReduce::Sum(sum_tmp.b.p, sum_bytes, has, found.b.p, (int)n1, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&n_found, found.b.p, sizeof n_found, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n_found_out)
    *n_found_out = n_found;
  ms[1] = ms_since(t0);
  if (!on_device) {
    t0 = std::chrono::steady_clock::now();
    if (nearest.wanted() && (rc = nearest.copy_out(c, (size_t)n1))) return rc;
    if (dist.wanted() && (rc = dist.copy_out(c, (size_t)n1))) return rc;
    if (ties.wanted() && (rc = ties.copy_out(c, (size_t)n1))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ms[copy_slot] = ms_since(t0);
  }
  return CMPR_OK;
}
