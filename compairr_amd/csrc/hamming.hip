/*
 * hamming.hip -- the reference's all-against-all path for any d (process_trad, overlap.cc:286-359; seq_diff,
 * util.cc:172-184) as library calls that take the distance as an argument: cmpr_hamming_matrix / _device and
 * cmpr_hamming_neighbors / _device; and the reference's clusters on that path (process_trad, cluster.cc:165-211, swept by
 * cluster.cc:276-410): cmpr_hamming_cluster / _device and cmpr_hamming_cluster_table / _device; and the nearest neighbour
 * of every sequence under that group relation, whatever its distance: cmpr_hamming_nearest / _device.  A pair (i of set 1,
 * j of set 2) matches when the two sequences have one length
 * (two empty ones included), the same V and J gene numbers unless ignore_genes, and differ at no more than
 * `differences` positions.  Nothing is hashed: every query is compared with every sequence of its group.
 *
 *   group, pack, the matrix and count / fill sinks, the segments: allpairs.h.  All hits of a query lie in ONE set-2
 *            group, walked in increasing sequence number: the rows of the neighbours come out sorted, without
 *            atomics and without a row sort.
 *   compare  hm_compare_kernel.  A workgroup of four waves takes four 64-query tiles of one group and one segment of
 *            the matching set-2 group; it stages the segment's packed sequences in LDS, HM_LDS_WORDS at a time, and
 *            every lane walks the staged references with its query's words in registers (register form) or read
 *            from global memory (generic form: groups of more than HAMMING_REG_WORDS words; a reference that does
 *            not fit the LDS buffer is staged in runs of words).  All lanes read the same reference word: an LDS
 *            broadcast.  Differing residues per word: xor, SWAR, popcount.
 *   sinks    link (the cluster calls: the set against itself, every group paired with itself): allpairs.h's sink, the
 *            forest of link_forest.h over the ORIGINAL sequence numbers.  Position order inside a group is number
 *            order, so the lane whose query sits at position qi links only references at positions above qi: every unordered pair
 *            once, (i, i) never.  The workgroup of the queries [256b, 256b + 256) walks [256b + 1, nr), its segments
 *            divide that range, and a wave skips what lies at or below its own first query.  Beside every staged
 *            reference lies a snapshot of its root; a lane keeps its own root in a register, skips a match whose
 *            snapshot equals it and looks its root up again after a link it made.  No count array, no pair list.
 *            What follows the launch is cluster.hip's: flatten, sizes, and for the table calls the table pass.
 *            nearest (cmpr_hamming_nearest): no threshold -- a lane keeps the smallest distance so far, the POSITION in
 *            the group of the first reference at it and the number of references at it: two compares and selects per
 *            reference, nothing indexed by the distance.  A reference that is no candidate (below the floor, the
 *            query itself in one-set mode, the query's own repertoire with the flag) takes part at an infinite
 *            distance.  Position order is number order, so the first reference at the minimum is the one of the
 *            smallest number, looked up in the group order once, at the end.  One segment: the lane writes its three
 *            results.  Several: every (query, segment) writes a slot -- the 64-bit key (distance << 32 | number) and
 *            the ties -- and pairs_nearest (allpairs.h) folds them: the smallest key of a query, the ties of the slots
 *            at its distance summed.  Outputs and slots are set to "none" on the stream first: what no lane visits
 *            stays so.
 */
#include "allpairs.h"

#include <algorithm>
#include <string>
#include <vector>

using namespace cmpr;

namespace {

constexpr uint32_t HM_LDS_WORDS = 4096;        /* packed words of references staged at a time (16 KiB) */
constexpr uint32_t HM_LINK_SEGMENT = 16384;    /* link sink: references of the longest automatic segment (32 pieces) */

/* a group of set 1 and the group of set 2 with the same key */
struct HmPair {
  uint64_t pk1, pk2;               /* first packed word of either group */
  uint32_t q0, nq, r0, nr;         /* positions in the two sorted orders */
  uint32_t stride, blk0;           /* words per sequence; first workgroup (grid x) of the pair */
};

struct HmParams {
  const HmPair   *pairs;
  uint32_t        npairs, segments;
  const uint32_t *pk1, *pk2;       /* packed words */
  const uint32_t *ord1, *ord2;     /* sequence numbers in group order */
  uint32_t        d, stage_refs;
  uint32_t        blk_base;        /* workgroup number of this launch's first workgroup */
  PairSinks       sink;            /* count / fill, matrix (allpairs.h); rep1, rep2 also of the nearest sink */
  PairLinks       link;            /* link (allpairs.h) */
  /* nearest (sink.rep1, sink.rep2 read with other_rep only) */
  uint32_t        floor;           /* a candidate differs at this many positions or more */
  uint32_t        one_set;         /* 1: set 2 IS set 1, a query is no candidate of its own */
  uint32_t        other_rep;       /* 1: a candidate comes from another repertoire than the query */
  PairNearest     nn;              /* where the results or the (query, segment) slots go (allpairs.h) */
};

/* differing residues of two packed words.  Amino acids: a byte each, codes below 0x80, so neither the xor nor the
   sum carries into the next byte and bit 7 says "this byte is not zero".  Nucleotides: two bits each. */
template <bool NT>
__device__ __forceinline__ uint32_t diff_word(uint32_t a, uint32_t b)
{
  const uint32_t x = a ^ b;
  if (NT)
    return (uint32_t)__popc((x | (x >> 1)) & 0x55555555u);
  return (uint32_t)__popc((x + 0x7f7f7f7fu) & 0x80808080u);
}

/* The sinks of hm_compare_kernel behind PairSink's interface (allpairs.h): the count / fill, matrix and link sinks ARE
   PairSink; the nearest one below is this file's own.  pr, qi: the workgroup's pair and the lane's query within its group. */
template <int SINK>
struct HmSink : PairSink<SINK> {
  __device__ __forceinline__ HmSink(const HmParams &P, const HmPair &, uint32_t, const PairLds &L, uint32_t *)
      : PairSink<SINK>(P.sink, P.segments, L) {}
};

/* link: allpairs.h's, with the forest and the snapshot flag of the parameters */
template <>
struct HmSink<SINK_LINK> : PairSink<SINK_LINK> {
  __device__ __forceinline__ HmSink(const HmParams &P, const HmPair &, uint32_t, const PairLds &L, uint32_t *st_root)
      : PairSink<SINK_LINK>(P.link, L, st_root) {}
};

/* nearest: no threshold, so near() for EVERY reference in place of match() for the matching ones.  The smallest
   distance so far, the position in the group of the first reference at it, how many at it */
template <>
struct HmSink<SINK_NEAREST> {
  const HmParams P;                /* (a copy, as PairSink's K) */
  const uint32_t *const ord2;      /* of the set-2 group */
  const Lds<uint32_t> st_rep;
  /* the position in the group that is the lane's own query (one-set mode: the group is paired with itself, as in the
     link sink) and the repertoire a candidate must not come from; HM_NONE is no position and no repertoire */
  const uint32_t nn_self;
  uint32_t nn_rep = HM_NONE;
  uint32_t best = HM_NONE, bpos = 0, ties = 0;
  __device__ __forceinline__ HmSink(const HmParams &P_, const HmPair &pr, uint32_t qi, const PairLds &L, uint32_t *)
      : P(P_), ord2(P_.ord2 + pr.r0), st_rep(L.rep), nn_self(P_.one_set ? qi : HM_NONE) {}
  __device__ __forceinline__ void zero_matrix() const {}
  __device__ __forceinline__ void init(uint32_t qorig, uint32_t)
  {
    nn_rep = P.other_rep ? P.sink.rep1[qorig] : HM_NONE;
  }
  __device__ __forceinline__ bool stages() const { return P.other_rep; }   /* (the number is looked up once, at the end) */
  __device__ __forceinline__ void stage(uint32_t r, uint32_t id) const { st_rep[r] = P.sink.rep2[id]; }
  /* the reference at position `pos` of the group, staged as r, differs at `dd` positions.  What is no candidate is
     infinitely far; then (smaller: the first at it) and (equal: one more at it), as selects */
  __device__ __forceinline__ void near(uint32_t pos, uint32_t r, uint32_t dd)
  {
    uint32_t rp = 0;                                                    /* (without the flag: not HM_NONE) */
    if (P.other_rep)                                                    /* (the same for every lane) */
      rp = st_rep[r];
    const bool ok = (dd >= P.floor) & (pos != nn_self) & (rp != nn_rep);
    const uint32_t de = ok ? dd : HM_NONE;
    const bool lt = de < best;
    ties = lt ? 1u : ties + (de == best ? 1u : 0u);                     /* (the ties of "none" are dropped at the end) */
    bpos = lt ? pos : bpos;
    best = lt ? de : best;
  }
  __device__ __forceinline__ void end(bool active, uint32_t qorig, uint32_t seg) const
  {
    if (active)                                                         /* (bpos is 0 while nobody was found) */
      pairs_nearest_end(P.nn, P.segments, qorig, seg, best, ord2[bpos], ties);
  }
};

/* NW: words per sequence held in registers (the group's stride), 0: the generic form */
template <int NW, int SINK, bool NT>
__global__ void __launch_bounds__(PAIRS_WG)
hm_compare_kernel(const HmParams P)
{
  __shared__ uint32_t st_words[HM_LDS_WORDS];
  __shared__ uint32_t st_id[PAIRS_STAGE_MAX];
  __shared__ uint32_t st_rep[SINK == SINK_MATRIX || SINK == SINK_NEAREST ? PAIRS_STAGE_MAX : 1];
  __shared__ unsigned long long st_cnt[SINK == SINK_MATRIX ? PAIRS_STAGE_MAX : 1];
  __shared__ unsigned long long st_mat[SINK == SINK_MATRIX ? PAIRS_MAT_CELLS : 1];
  __shared__ uint32_t st_root[SINK == SINK_LINK ? PAIRS_STAGE_MAX : 1];

  const uint32_t blk = P.blk_base + blockIdx.x;
  const HmPair pr = pairs_entry_of(P.pairs, P.npairs, blk);
  const uint32_t stride = NW ? (uint32_t)NW : pr.stride;
  const PairQuery Q(pr, blk, P.ord1);
  const uint32_t qi = Q.qi, qorig = Q.qorig;
  const bool active = Q.active();
  /* the segment of the set-2 group.  Link sink: set 2 IS set 1 and position order is number order (the stable
     sort), so an unordered pair is walked once, by the lane of its smaller position: the workgroup whose first
     query sits at position b walks the references behind b only, and its segments divide THAT range. */
  const uint32_t seg = blockIdx.y;
  const uint32_t w0 = SINK == SINK_LINK ? min((blk - pr.blk0) * PAIRS_WG + 1u, pr.nr) : 0u;
  uint32_t e0, e1;
  pairs_segment(pr.nr, w0, seg, P.segments, e0, e1);
  /* ... and a wave skips the staged references at or below its first query: no lane of it wants them */
  const uint32_t wave_q0 = SINK == SINK_LINK
      ? (uint32_t)__builtin_amdgcn_readfirstlane((int)((blk - pr.blk0) * PAIRS_WG + (threadIdx.x & ~(WAVE - 1u)))) : 0u;

  if (e0 >= e1)
    return;                                                             /* (the whole workgroup) */
  HmSink<SINK> S(P, pr, qi, PairLds(st_id, st_rep, st_cnt, st_mat), st_root);
  S.zero_matrix();                                                      /* (a barrier follows before the first match) */

  const PairWords<NW> QW(P.pk1, pr, Q, stride);                        /* (register form: the stride IS NW) */
  const uint32_t *const qw = QW.w;
  const uint32_t (&q)[NW ? NW : 1] = QW.q;

  S.init(qorig, seg);
  /* sequence numbers, repertoires and counts of the references e .. e + n - 1 of the group */
  auto stage_ids = [&](uint32_t e, uint32_t n) {
    if (S.stages())
      for (uint32_t r = threadIdx.x; r < n; r += PAIRS_WG)
        S.stage(r, P.ord2[pr.r0 + e + r]);
  };
  /* the reference at position `pos` of the group, staged as r, differs at `dd` positions */
  auto compared = [&](uint32_t pos, uint32_t r, uint32_t dd) {
    if constexpr (SINK == SINK_NEAREST)
      S.near(pos, r, dd);
    else if (dd <= P.d && active && (SINK != SINK_LINK || pos > qi))
      S.match(r, dd);
  };

  if (stride <= HM_LDS_WORDS) {
    /* whole references, R at a time */
    const uint32_t R = pairs_piece(HM_LDS_WORDS / stride, P.stage_refs);
    for (uint32_t e = e0; e < e1; e += R) {
      const uint32_t n = e1 - e < R ? e1 - e : R;
      __syncthreads();                                                  /* the previous piece has been read */
      const uint32_t *const src = P.pk2 + pr.pk2 + (uint64_t)e * stride;
      for (uint32_t k = threadIdx.x; k < n * stride; k += PAIRS_WG)
        st_words[k] = src[k];
      stage_ids(e, n);
      __syncthreads();
      const uint32_t r0 = SINK == SINK_LINK && wave_q0 >= e ? min(wave_q0 - e + 1u, n) : 0u;
      for (uint32_t r = r0; r < n; r++) {
        const uint32_t *const w = st_words + r * stride;
        uint32_t dd = 0;
        if (NW) {
#pragma unroll
          for (int k = 0; k < NW; k++)
            dd += diff_word<NT>(q[k], w[k]);
        } else {
          for (uint32_t k = 0; k < stride; k++)
            dd += diff_word<NT>(qw[k], w[k]);
        }
        compared(e + r, r, dd);
      }
    }
  } else {
    /* generic form only: a reference longer than the buffer, staged in runs of words */
    for (uint32_t e = e0; e < e1; e++) {
      uint32_t dd = 0;
      for (uint32_t k0 = 0; k0 < stride; k0 += HM_LDS_WORDS) {
        const uint32_t m = stride - k0 < HM_LDS_WORDS ? stride - k0 : HM_LDS_WORDS;
        __syncthreads();
        const uint32_t *const src = P.pk2 + pr.pk2 + (uint64_t)e * stride + k0;
        for (uint32_t k = threadIdx.x; k < m; k += PAIRS_WG)
          st_words[k] = src[k];
        if (k0 == 0)
          stage_ids(e, 1);
        __syncthreads();
        for (uint32_t k = 0; k < m; k++)
          dd += diff_word<NT>(qw[k0 + k], st_words[k]);
      }
      compared(e, 0, dd);
    }
  }
  S.end(active, qorig, seg);
}

typedef void (*HmKernel)(const HmParams);

template <int SINK, bool NT>
HmKernel hm_kernel_for(uint32_t nw)
{
  switch (nw) {
  case 1:  return hm_compare_kernel<1, SINK, NT>;
  case 2:  return hm_compare_kernel<2, SINK, NT>;
  case 3:  return hm_compare_kernel<3, SINK, NT>;
  case 4:  return hm_compare_kernel<4, SINK, NT>;
  case 5:  return hm_compare_kernel<5, SINK, NT>;
  case 6:  return hm_compare_kernel<6, SINK, NT>;
  case 8:  return hm_compare_kernel<8, SINK, NT>;
  case 12: return hm_compare_kernel<12, SINK, NT>;
  case 16: return hm_compare_kernel<16, SINK, NT>;
  default: return hm_compare_kernel<0, SINK, NT>;
  }
}

/* what the entry points share: both sets on the device, the pairs of groups */
struct HmJob : PairSets {
  Tmp<HmPair>    pairs;
  HmParams       P{};
  uint32_t       blocks = 0;
  PairRuns       runs;             /* form: the stride, 0 the generic form */
};

int hm_setup(cmpr_context *c, const std::string &who, const cmpr_set_view *set1, const cmpr_set_view *set2,
             int64_t differences, bool on_device, HmJob &J, bool triangular = false)
{
  int rc;
  if ((rc = pairs_stage(c, set1, set2, on_device, J, hm_key_mode(c)))) return rc;
  HmSet &A = *J.s1, &B = *J.s2;
  /* the groups of the two sets with one key; their workgroups, in runs of one form */
  std::vector<HmPair> pairs;
  uint64_t blocks = 0;
  uint32_t nr_max = 0;
  for (size_t a = 0, b = 0; a < A.keys.size() && b < B.keys.size();) {
    if (A.keys[a] < B.keys[b]) {
      a++;
    } else if (B.keys[b] < A.keys[a]) {
      b++;
    } else {
      const HmGroup &ga = A.groups[a], &gb = B.groups[b];
      HmPair p{ga.pk_off, gb.pk_off, ga.start, ga.count, gb.start, gb.count, ga.stride, (uint32_t)blocks};
      const uint32_t nb = blocks_for(ga.count, PAIRS_WG);
      const uint32_t form = c->hamming_generic || p.stride > HAMMING_REG_WORDS ? 0u : p.stride;
      J.runs.add(form, (uint32_t)blocks, nb);
      blocks += nb;
      nr_max = std::max(nr_max, gb.count);
      pairs.push_back(p);
      a++;
      b++;
    }
  }
  if (blocks > 0xffffffu)
    return fail(c, CMPR_EUNSUPPORTED, who + ": more than 2^24 workgroups of queries");
  J.blocks = (uint32_t)blocks;
  if (!pairs.empty()) {
    if ((rc = dev_upload(c, J.pairs.b, pairs.data(), pairs.size()))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));           /* (`pairs` leaves scope) */
  }
  /* the link sink's workgroups walk what lies behind them: the first of a group all of it, the last nothing, and
     the launch ends with the first ones of the largest group.  No segment longer than HM_LINK_SEGMENT references
     keeps those as short as everybody else's */
  const uint32_t S = pairs_segments(c, c->hamming_segments, blocks, nr_max, triangular ? HM_LINK_SEGMENT : 0u);
  const uint64_t longest = std::max(A.longest, B.longest);
  HmParams &P = J.P;
  P.pairs = J.pairs.b.p;
  P.npairs = (uint32_t)pairs.size();
  P.segments = S;
  P.pk1 = A.pk.b.p; P.pk2 = B.pk.b.p;
  P.ord1 = A.ord.b.p; P.ord2 = B.ord.b.p;
  P.d = (uint32_t)std::min<uint64_t>((uint64_t)differences, longest);   /* above the longest sequence: as that length */
  P.stage_refs = (uint32_t)c->hamming_stage_refs;
  return CMPR_OK;
}

/* the compare kernel over every pair of groups: a launch per run of pairs of one form */
template <int SINK>
int hm_launch(cmpr_context *c, const HmJob &J)
{
  const bool nt = c->opt.alphabet_size == 4;
  return pairs_launch(c, J.runs, J.P, [nt](uint32_t form) {
    return nt ? hm_kernel_for<SINK, true>(form) : hm_kernel_for<SINK, false>(form);
  });
}

int hamming_matrix_impl(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2, int64_t differences,
                        void *matrix_out, bool on_device)
{
  if (!c)
    return CMPR_EINVAL;
  const std::string who = "cmpr_hamming_matrix";
  int rc;
  if ((rc = hm_refusals(c, who, set1, set2, differences, HM_MATRIX, on_device)))
    return rc;
  if (!matrix_out)
    return fail(c, CMPR_EINVAL, who + ": matrix_out is NULL");
  HmJob J;
  if ((rc = pairs_timed_setup(c, c->hm_ms, false,
                              [&] { return hm_setup(c, who, set1, set2, differences, on_device, J); })))
    return rc;
  return pairs_matrix(c, J, J.P.sink, matrix_out, on_device, [&] { return hm_launch<SINK_MATRIX>(c, J); }, c->hm_ms, 2);
}

int hamming_neighbors_impl(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2, int64_t differences,
                           uint64_t capacity, uint64_t *row_start_out, uint32_t *hit_out, uint16_t *dist_out,
                           uint64_t *n_edges_out, bool on_device)
{
  if (!c)
    return CMPR_EINVAL;
  const std::string who = "cmpr_hamming_neighbors";
  int rc;
  if ((rc = pairs_neighbors_args(c, who, capacity, hit_out, n_edges_out)) ||
      (rc = hm_refusals(c, who, set1, set2, differences, HM_NEIGHBORS, on_device)))
    return rc;
  HmJob J;
  if ((rc = pairs_timed_setup(c, c->hm_ms, false,
                              [&] { return hm_setup(c, who, set1, set2, differences, on_device, J); })))
    return rc;
  /* rows only when asked for, and in order as the walk leaves them: no row order step */
  return pairs_neighbors(c, who, J, J.P.segments, J.P.sink, capacity, row_start_out, hit_out, dist_out, n_edges_out,
                         on_device, [&] { return hm_launch<SINK_CSR>(c, J); }, false, c->hm_ms, -1, 2);
}

/* cmpr_hamming_nearest*: one walk through the nearest sink; what surrounds the launch -- "none" everywhere first, with
   several segments the fold of the slots, the number of queries that found somebody -- is pairs_nearest (allpairs.h) */
int hamming_nearest_impl(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2, int64_t min_distance,
                         uint32_t flags, uint32_t *nearest_out, uint16_t *dist_out, uint32_t *ties_out,
                         uint64_t *n_found_out, bool on_device)
{
  if (!c)
    return CMPR_EINVAL;
  const std::string who = "cmpr_hamming_nearest";
  if (n_found_out)
    *n_found_out = 0;
  int rc;
  if ((rc = hm_refusals(c, who, set1, set2, min_distance, HM_NEAREST, on_device)))
    return rc;
  if (flags & ~(uint32_t)CMPR_NEAREST_OTHER_REPERTOIRE)
    return fail(c, CMPR_EINVAL, who + ": unknown bits in flags");
  const bool other_rep = (flags & CMPR_NEAREST_OTHER_REPERTOIRE) != 0;
  if (other_rep && set2 != set1)
    return fail(c, CMPR_EINVAL, who + ": CMPR_NEAREST_OTHER_REPERTOIRE needs set2 == set1 (two sets have two numberings "
                                      "of their repertoires)");
  HmJob J;
  if ((rc = pairs_timed_setup(c, c->hm_ms, false, [&] { return hm_setup(c, who, set1, set2, 0, on_device, J); })))
    return rc;
  HmParams &P = J.P;
  P.sink.rep1 = J.s1->rep.b.p; P.sink.rep2 = J.s2->rep.b.p;
  P.floor = (uint32_t)std::min<int64_t>(min_distance, 0x10000);        /* (no distance is above 65535) */
  P.one_set = J.s2 == J.s1 ? 1u : 0u;
  P.other_rep = other_rep ? 1u : 0u;
  return pairs_nearest(c, J, P.segments, nearest_out, dist_out, ties_out, n_found_out, on_device,
                       [&](const PairNearest &N) {
                         P.nn = N;
                         return hm_launch<SINK_NEAREST>(c, J);
                       },
                       c->hm_ms, 2);
}

/* cmpr_hamming_cluster* and cmpr_hamming_cluster_table*: the set against itself through the link sink, then
   pairs_clusters (allpairs.h): the flatten, size and table passes of cluster.hip.  The plain call (T == NULL) fills L's
   label / size, the table call T's four arrays from labels and sizes of nobody's. */
int hamming_cluster_impl(cmpr_context *c, const cmpr_set_view *set, int64_t differences, bool on_device,
                         ClusterLinks &L, ClusterTableOut *T, uint64_t *n_clusters_out)
{
  if (!c)
    return CMPR_EINVAL;
  const bool table = T != nullptr;
  const std::string who = table ? "cmpr_hamming_cluster_table" : "cmpr_hamming_cluster";
  if (n_clusters_out)
    *n_clusters_out = 0;
  int rc;
  if ((rc = hm_refusals(c, who, set, set, differences, HM_CLUSTERS, on_device)))
    return rc;
  HmJob J;
  if ((rc = pairs_timed_setup(c, c->hm_ms, table,
                              [&] { return hm_setup(c, who, set, set, differences, on_device, J, true); })))
    return rc;
  return pairs_clusters(c, *J.s1, c->hamming_link_snapshot != 0, on_device, L, T, n_clusters_out,
                        [&](const PairLinks &K) {
                          J.P.link = K;
                          return hm_launch<SINK_LINK>(c, J);
                        },
                        c->hm_ms, 2);
}

}  // namespace

extern "C" int cmpr_hamming_cluster(cmpr_context *c, const cmpr_set_view *set, int64_t differences,
                                    uint32_t *label_out, uint32_t *size_out, uint64_t *n_clusters_out)
{
  return guarded(c, [&] {
    ClusterLinks L(label_out, size_out, false);
    return hamming_cluster_impl(c, set, differences, false, L, nullptr, n_clusters_out);
  });
}

extern "C" int cmpr_hamming_cluster_device(cmpr_context *c, const cmpr_set_view *d_set, int64_t differences,
                                           uint32_t *d_label_out, uint32_t *d_size_out, uint64_t *n_clusters_out)
{
  return guarded(c, [&] {
    ClusterLinks L(d_label_out, d_size_out, true);
    return hamming_cluster_impl(c, d_set, differences, true, L, nullptr, n_clusters_out);
  });
}

extern "C" int cmpr_hamming_cluster_table(cmpr_context *c, const cmpr_set_view *set, int64_t differences,
                                          uint32_t *cluster_of_out, uint64_t *cluster_start_out,
                                          uint32_t *member_out, uint64_t *count_out, uint64_t *n_clusters_out)
{
  return guarded(c, [&] {
    ClusterLinks L(nullptr, nullptr, false);
    ClusterTableOut T(cluster_of_out, cluster_start_out, member_out, count_out, false);
    return hamming_cluster_impl(c, set, differences, false, L, &T, n_clusters_out);
  });
}

extern "C" int cmpr_hamming_cluster_table_device(cmpr_context *c, const cmpr_set_view *d_set, int64_t differences,
                                                 uint32_t *d_cluster_of_out, uint64_t *d_cluster_start_out,
                                                 uint32_t *d_member_out, uint64_t *d_count_out,
                                                 uint64_t *n_clusters_out)
{
  return guarded(c, [&] {
    ClusterLinks L(nullptr, nullptr, true);
    ClusterTableOut T(d_cluster_of_out, d_cluster_start_out, d_member_out, d_count_out, true);
    return hamming_cluster_impl(c, d_set, differences, true, L, &T, n_clusters_out);
  });
}

extern "C" int cmpr_hamming_matrix(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2,
                                   int64_t differences, uint64_t *matrix_out)
{
  return guarded(c, [&] { return hamming_matrix_impl(c, set1, set2, differences, matrix_out, false); });
}

extern "C" int cmpr_hamming_matrix_device(cmpr_context *c, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                                          int64_t differences, void *d_matrix)
{
  return guarded(c, [&] { return hamming_matrix_impl(c, d_set1, d_set2, differences, d_matrix, true); });
}

extern "C" int cmpr_hamming_neighbors(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2,
                                      int64_t differences, uint64_t capacity, uint64_t *row_start_out,
                                      uint32_t *hit_out, uint16_t *distance_out, uint64_t *n_edges_out)
{
  return guarded(c, [&] {
    return hamming_neighbors_impl(c, set1, set2, differences, capacity, row_start_out, hit_out, distance_out,
                                  n_edges_out, false);
  });
}

extern "C" int cmpr_hamming_neighbors_device(cmpr_context *c, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                                             int64_t differences, uint64_t capacity, uint64_t *d_row_start_out,
                                             uint32_t *d_hit_out, uint16_t *d_distance_out, uint64_t *n_edges_out)
{
  return guarded(c, [&] {
    return hamming_neighbors_impl(c, d_set1, d_set2, differences, capacity, d_row_start_out, d_hit_out,
                                  d_distance_out, n_edges_out, true);
  });
}

extern "C" int cmpr_hamming_nearest(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2,
                                    int64_t min_distance, uint32_t flags, uint32_t *nearest_out,
                                    uint16_t *distance_out, uint32_t *ties_out, uint64_t *n_found_out)
{
  return guarded(c, [&] {
    return hamming_nearest_impl(c, set1, set2, min_distance, flags, nearest_out, distance_out, ties_out, n_found_out,
                                false);
  });
}

extern "C" int cmpr_hamming_nearest_device(cmpr_context *c, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                                           int64_t min_distance, uint32_t flags, uint32_t *d_nearest_out,
                                           uint16_t *d_distance_out, uint32_t *d_ties_out, uint64_t *n_found_out)
{
  return guarded(c, [&] {
    return hamming_nearest_impl(c, d_set1, d_set2, min_distance, flags, d_nearest_out, d_distance_out, d_ties_out,
                                n_found_out, true);
  });
}
