/*
 * edit.hip -- the all-against-all path under EDIT distance, for any d: cmpr_edit_neighbors / _device,
 * cmpr_edit_matrix / _device, the single-linkage clusters of that relation, cmpr_edit_cluster / _device and
 * cmpr_edit_cluster_table / _device, and the nearest neighbour of every sequence under that distance, whatever it is:
 * cmpr_edit_nearest / _device.  A pair (i of set 1, j of set 2) matches when the two sequences have the same V and J
 * gene numbers unless ignore_genes and their Levenshtein distance -- substitution, insertion and deletion cost 1 each --
 * is at most `differences`.  The reference has indels at d = 1 only (its variant enumeration explodes beyond); nothing
 * is enumerated or hashed here: every query is compared with every sequence of every group it can match.
 *
 *   group    allpairs.h's: each set sorted by (length, V, J) with a stable radix sort, its residues packed in group
 *            order.  Sequences of more than PAIRS_MAX_LEN = 256 residues are refused.
 *   jobs     allpairs.h's frame (PairJob, pairs_jobs: the table, the runs of one query form, the limits, the upload;
 *            in the kernel PairWords, pairs_segment, pairs_piece), on the host, from the two group tables: a set-1
 *            group (L, V, J) and its PARTNERS.  This file's own is the partner rule: the set-2 groups (L', V, J) with
 *            |L - L'| <= d, found by binary search of the key for every length L' set 2 has (a huge d costs nothing).
 *            The partners of a job are contiguous in one array.
 *   compare  ed_compare_kernel.  A workgroup of four waves takes four 64-query tiles of one job and one segment
 *            (grid y) of EVERY partner, one partner after the other.  Of the staged references the workgroup builds
 *            Peq[reference][symbol][w] in LDS, ED_PEQ_WORDS 64-bit words at a time: bit i of word w is set where the
 *            reference holds the symbol at position 64 w + i (160 bytes per amino-acid reference of up to 64 residues:
 *            about a hundred references per 16 KiB piece, built once for 256 queries).  Every lane then runs the
 *            bit-vector edit distance (Myers 1999 in Hyyro's global form) with the reference as the pattern and its
 *            own query as the text: per query residue c one read of Peq[c] -- the only per-lane LDS address; equal
 *            addresses broadcast -- and some fifteen 64-bit operations per column word.  W = 1, 2 or 4 column words
 *            by the reference's length, the loops over W unrolled: the addition's carry and the two shifted-out top
 *            bits pass from word w to w + 1, the bits above the reference's length never reach lower ones (nothing
 *            is masked), and the score is read at bit (n - 1) % 64 of word (n - 1) / 64, which is the same for all
 *            lanes.  An empty reference is at the query's length.
 *            The query's packed words sit in registers (NW = 2, 4, 8, 16 words, the residues peeled by loops
 *            unrolled at compile time under the uniform `pos < len`) while it has at most PAIRS_REG_RESIDUES = 64
 *            residues: every CDR3 and junction of amino acids.  A longer query is read word by word from global
 *            memory (NW = 0: one load per four or sixteen column steps); unrolled, 256 steps of four column words
 *            would be straight-line code far beyond the instruction cache.  No instantiation indexes an array at
 *            run time: private_segment_fixed_size is 0 in every one of them, the nearest sink's included (checked in
 *            the code object's metadata).
 *   sinks    allpairs.h's matrix and count / fill.  The walk goes partner by partner, which is not number order, so
 *            the rows are sorted afterwards by csr_rows.h with the 64-bit key (hit << 16 | distance) -- the hit alone
 *            without distance_out --, rows beyond LDS_MAX by hipcub's device-wide sort.  The hits of a row are
 *            distinct: the order is total, the bytes do not depend on the schedule.
 *            link (the cluster calls: the set against itself): allpairs.h's forest sink.  A job keeps the partners of
 *            its own length and longer: an unordered pair of two lengths is seen from the shorter side, and a longer
 *            partner is walked in full.  The job's OWN group is walked as hm_compare_kernel walks a group under this
 *            sink: the workgroup of the queries [256b, 256b + 256) walks [256b + 1, nr), its segments divide that
 *            range, a wave skips the staged pieces at or below its first query, a lane links only positions above its
 *            own.  Every unordered pair once, (i, i) never; the empty group is linked among itself (the distance of
 *            two empty sequences is 0) and to the groups of up to d residues.  Behind the launch: pairs_clusters.
 *            nearest (cmpr_edit_nearest): no threshold -- the kernel hands EVERY reference's distance to the sink, and a
 *            lane keeps the smallest distance so far, the smallest ORIGINAL number at it (the staged st_id[r], one LDS
 *            address for the wave: position order is number order inside a partner only) and the number of references
 *            at it: compares and selects, nothing indexed by the distance.  A reference that is no candidate (below the
 *            floor, above the cap, the query itself in one-set mode, the query's own repertoire with the flag) takes
 *            part at an infinite distance.  The job's partners are those within the cap BY INCREASING LENGTH GAP: the
 *            Levenshtein distance is never below the gap, so in front of every partner the workgroup votes
 *            (__syncthreads_or) whether any lane's best still reaches that partner's gap, and leaves the loop when none
 *            does -- every later reference is further than what each lane holds, so it can neither improve on it nor tie
 *            with it.  A (workgroup, segment) stops on its own partial best, an upper bound of the final one.  One
 *            segment: the lane writes its three results; several: a slot per (query, segment), folded by pairs_nearest
 *            (allpairs.h), which also sets outputs or slots to "none" first and counts the queries that found somebody.
 *
 * Nothing here writes the resident sets, plans or statistics of the context.
 */
#include "allpairs.h"

#include <algorithm>
#include <string>
#include <vector>

using namespace cmpr;

namespace {

constexpr uint32_t ED_PEQ_WORDS = 2048;        /* 64-bit words of Peq staged at a time (16 KiB) */
/* link sink: references of the longest automatic segment.  A sixteenth of hamming.hip's HM_LINK_SEGMENT, as a reference
   costs some twenty times as much here: 1M CDR3aa at d = 3, V/J matched (the largest group of 13 154), link kernel
   132 ms with HM_LINK_SEGMENT (one segment), 63 ms from 16 segments on; with ignore_genes (196 330) 2 218 ms in 12
   segments, 2 202 in 64 (profiles/r23/edit_cluster.txt) */
constexpr uint32_t ED_LINK_SEGMENT = 1024;

/* a set-2 group a job is compared with */
struct EdPartner {
  uint64_t pk_off;                 /* first packed word of the group */
  uint32_t r0, nr;                 /* positions in set 2's sorted order */
  uint32_t len;                    /* residues per sequence */
  uint16_t stride, own;            /* packed words per sequence (at most 64); 1: the group IS the job's own one (the
                                      cluster calls: the set against itself) */
};

struct EdParams {
  const PairJob   *jobs;           /* a set-1 group and its partners (allpairs.h) */
  const EdPartner *partners;
  uint32_t        njobs, segments;
  const uint32_t *pk1, *pk2;       /* packed words */
  const uint32_t *ord1, *ord2;     /* sequence numbers in group order */
  uint32_t        d, stage_refs, min_words;
  uint32_t        blk_base;        /* workgroup number of this launch's first workgroup */
  PairSinks       sink;            /* count / fill, matrix (allpairs.h); rep1, rep2 also of the nearest sink */
  PairLinks       link;            /* link (allpairs.h) */
  /* nearest: d is the cap (sink.rep1, sink.rep2 read with other_rep only) */
  uint32_t        floor;           /* a candidate lies at this distance or further */
  uint32_t        one_set;         /* 1: set 2 IS set 1, a query is no candidate of its own */
  uint32_t        other_rep;       /* 1: a candidate comes from another repertoire than the query */
  uint32_t        prune;           /* 1: a workgroup leaves the partners once no lane's best reaches the length gap */
  PairNearest     nn;              /* where the results or the (query, segment) slots go (allpairs.h) */
};

/* the sinks of ed_compare_kernel: allpairs.h's, each built from its fields of the parameters */
template <int SINK>
struct EdSink : PairSink<SINK> {
  __device__ __forceinline__ EdSink(const EdParams &P, const PairLds &L, uint32_t *)
      : PairSink<SINK>(P.sink, P.segments, L) {}
};
template <>
struct EdSink<SINK_LINK> : PairSink<SINK_LINK> {
  __device__ __forceinline__ EdSink(const EdParams &P, const PairLds &L, uint32_t *st_root)
      : PairSink<SINK_LINK>(P.link, L, st_root) {}
};

/* nearest: no threshold, so near() for EVERY reference in place of match() for the matching ones.  The smallest
   distance so far, the smallest ORIGINAL number at it -- a walk goes partner by partner, so position order is not
   number order across partners, and the staged number st_id[r], one LDS address for the whole wave, is compared
   instead --, how many at it.  What is no candidate (below the floor, above the cap, the query itself in one-set
   mode, the query's own repertoire with the flag) is infinitely far.  Compares and selects only. */
template <>
struct EdSink<SINK_NEAREST> {
  const EdParams P;                /* (a copy, as PairSink's K) */
  const Lds<uint32_t> st_id, st_rep;
  /* the number that is the lane's own query (one-set mode) and the repertoire a candidate must not come from;
     HM_NONE is no number and no repertoire */
  uint32_t nn_self = HM_NONE, nn_rep = HM_NONE;
  uint32_t best = HM_NONE, bid = HM_NONE, ties = 0;
  __device__ __forceinline__ EdSink(const EdParams &P_, const PairLds &L, uint32_t *)
      : P(P_), st_id(L.id), st_rep(L.rep) {}
  __device__ __forceinline__ void zero_matrix() const {}
  __device__ __forceinline__ void init(uint32_t qorig, uint32_t)
  {
    nn_self = P.one_set ? qorig : HM_NONE;
    nn_rep = P.other_rep ? P.sink.rep1[qorig] : HM_NONE;
  }
  __device__ __forceinline__ void stage(uint32_t r, uint32_t id) const
  {
    st_id[r] = id;
    if (P.other_rep)
      st_rep[r] = P.sink.rep2[id];
  }
  /* the reference staged as r lies at distance `dd`: (smaller: its number) and (equal: the smaller number, one more
     at it), as selects.  While nobody has been found "equal" also holds between two infinities: what it leaves in bid
     and ties is overwritten by the first candidate and dropped at the end */
  __device__ __forceinline__ void near(uint32_t r, uint32_t dd)
  {
    const uint32_t id = st_id[r];
    uint32_t rp = 0;                                                    /* (without the flag: not HM_NONE) */
    if (P.other_rep)                                                    /* (the same for every lane) */
      rp = st_rep[r];
    const bool ok = (dd >= P.floor) & (dd <= P.d) & (id != nn_self) & (rp != nn_rep);
    const uint32_t de = ok ? dd : HM_NONE;
    const bool lt = de < best;
    ties = lt ? 1u : ties + (de == best ? 1u : 0u);
    bid = lt ? id : de == best ? min(id, bid) : bid;
    best = lt ? de : best;
  }
  /* (a partner whose sequences are `gap` residues longer or shorter than the query holds nothing below `gap`) */
  __device__ __forceinline__ bool wants(bool active, uint32_t gap) const { return active && best >= gap; }
  __device__ __forceinline__ void end(bool active, uint32_t qorig, uint32_t seg) const
  {
    if (active)
      pairs_nearest_end(P.nn, P.segments, qorig, seg, best, bid, ties);
  }
};

/* One column of the edit-distance matrix further: the text residue whose Peq words lie at `peq`.  pv / mv: the
   vertical +1 / -1 deltas of the column, W 64-bit words, bit i for row i + 1; the top row's horizontal delta is +1
   (global distance).  The column is one integer of 64 W bits: `carry` is the addition's, ph_in / mh_in the bits the
   shifts move across a word boundary.  sw, sb: word and bit of the last row, where the score follows the horizontal
   deltas. */
template <int W>
__device__ __forceinline__ void ed_step(const unsigned long long *peq, unsigned long long (&pv)[W],
                                        unsigned long long (&mv)[W], uint32_t &score, uint32_t sw, uint32_t sb)
{
  unsigned long long carry = 0, ph_in = 1, mh_in = 0, ph_s = 0, mh_s = 0;
#pragma unroll
  for (int w = 0; w < W; w++) {
    const unsigned long long eq = peq[w], p = pv[w], m = mv[w];
    const unsigned long long xv = eq | m;
    const unsigned long long a = eq & p;
    const unsigned long long t = a + p;
    const unsigned long long sum = t + carry;
    carry = (t < a ? 1ull : 0ull) | (sum < t ? 1ull : 0ull);
    const unsigned long long xh = (sum ^ p) | eq;
    unsigned long long ph = m | ~(xh | p);
    unsigned long long mh = p & xh;
    ph_s = W == 1 || (uint32_t)w == sw ? ph : ph_s;
    mh_s = W == 1 || (uint32_t)w == sw ? mh : mh_s;
    const unsigned long long ph_out = ph >> 63, mh_out = mh >> 63;
    ph = ph << 1 | ph_in;
    mh = mh << 1 | mh_in;
    ph_in = ph_out;
    mh_in = mh_out;
    pv[w] = mh | ~(xv | ph);
    mv[w] = ph & xv;
  }
  score += (uint32_t)(ph_s >> sb) & 1u;
  score -= (uint32_t)(mh_s >> sb) & 1u;
}

/* NW: words of the query held in registers, 0: the query is read from global memory */
template <int NW, int SINK, bool NT>
__global__ void __launch_bounds__(PAIRS_WG)
ed_compare_kernel(const EdParams P)
{
  constexpr uint32_t A = NT ? 4 : 20, PER = NT ? 16 : 4, BITS = NT ? 2 : 8, MASK = NT ? 3 : 0xff;
  __shared__ unsigned long long st_peq[ED_PEQ_WORDS];
  __shared__ uint32_t st_id[PAIRS_STAGE_MAX];
  __shared__ uint32_t st_rep[SINK == SINK_MATRIX || SINK == SINK_NEAREST ? PAIRS_STAGE_MAX : 1];
  __shared__ unsigned long long st_cnt[SINK == SINK_MATRIX ? PAIRS_STAGE_MAX : 1];
  __shared__ unsigned long long st_mat[SINK == SINK_MATRIX ? PAIRS_MAT_CELLS : 1];
  __shared__ uint32_t st_root[SINK == SINK_LINK ? PAIRS_STAGE_MAX : 1];

  const uint32_t blk = P.blk_base + blockIdx.x;
  const PairJob jb = pairs_entry_of(P.jobs, P.njobs, blk);
  const PairQuery Q(jb, blk, P.ord1);
  const uint32_t qi = Q.qi, qorig = Q.qorig;
  const bool active = Q.active();
  const uint32_t qlen = jb.len;
  const uint32_t seg = blockIdx.y;
  /* link sink, the job's own group: position order is number order (the stable sort), so an unordered pair is walked
     once, by the lane of its smaller position, and a wave skips the staged references at or below its first query */
  const uint32_t wg_q0 = (blk - jb.blk0) * PAIRS_WG;
  const uint32_t wave_q0 = SINK == SINK_LINK
      ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(wg_q0 + (threadIdx.x & ~(WAVE - 1u)))) : 0u;

  EdSink<SINK> S(P, PairLds(st_id, st_rep, st_cnt, st_mat), st_root);
  S.zero_matrix();                                                      /* (a barrier follows before the first match) */

  const PairWords<NW> QW(P.pk1, jb, Q, jb.stride);
  const uint32_t *const qw = QW.w;
  const uint32_t (&q)[NW ? NW : 1] = QW.q;

  S.init(qorig, seg);

  /* the references e0 .. e1 - 1 of partner pt, their columns W words long */
  auto walk = [&](const EdPartner &pt, uint32_t e0, uint32_t e1, auto words) {
    constexpr int W = decltype(words)::value;
    const bool own = SINK == SINK_LINK && pt.own;
    const uint32_t n = pt.len;
    const uint32_t sw = n ? (n - 1) >> 6 : 0u, sb = n ? (n - 1) & 63u : 0u;
    const uint32_t R = pairs_piece(ED_PEQ_WORDS / (A * W), P.stage_refs);
    for (uint32_t e = e0; e < e1; e += R) {
      const uint32_t cnt = e1 - e < R ? e1 - e : R;
      __syncthreads();                                                  /* the previous piece has been read */
      /* Peq: one thread per (reference, symbol, word); st_peq[(r x A + symbol) x W + w] */
      for (uint32_t it = threadIdx.x; it < cnt * A * W; it += PAIRS_WG) {
        const uint32_t r = it / (A * W), sym = it % (A * W) / W, w = it % W;
        const uint32_t *const src = P.pk2 + pt.pk_off + (uint64_t)(e + r) * pt.stride;
        unsigned long long bits = 0;
        for (uint32_t k = 0; k < 64 / PER; k++) {
          const uint32_t wi = w * (64 / PER) + k;                       /* packed word: residues wi x PER .. */
          if (wi * PER >= n)
            break;                                                      /* (n <= stride x PER: wi is inside the sequence) */
          const uint32_t word = src[wi];
#pragma unroll
          for (uint32_t t = 0; t < PER; t++)
            if (wi * PER + t < n && ((word >> (t * BITS)) & MASK) == sym)
              bits |= 1ull << (k * PER + t);
        }
        st_peq[it] = bits;
      }
      for (uint32_t r = threadIdx.x; r < cnt; r += PAIRS_WG)
        S.stage(r, P.ord2[pt.r0 + e + r]);
      __syncthreads();
      const uint32_t r0 = own && wave_q0 >= e ? min(wave_q0 - e + 1u, cnt) : 0u;
      for (uint32_t r = r0; r < cnt; r++) {
        uint32_t dd = n;
        if (n == 0) {
          dd = qlen;                                                    /* an empty reference: every residue inserted */
        } else {
          const unsigned long long *const pq = st_peq + r * (A * W);
          unsigned long long pv[W], mv[W];
#pragma unroll
          for (int w = 0; w < W; w++) {
            pv[w] = ~0ull;
            mv[w] = 0;
          }
          if (NW) {
#pragma unroll
            for (int k = 0; k < NW; k++)
              if ((uint32_t)k * PER < qlen) {
#pragma unroll
                for (uint32_t t = 0; t < PER; t++)
                  if ((uint32_t)k * PER + t < qlen)
                    ed_step<W>(pq + ((q[k] >> (t * BITS)) & MASK) * W, pv, mv, dd, sw, sb);
              }
          } else {
            for (uint32_t k = 0; k * PER < qlen; k++) {
              const uint32_t word = qw[k];
#pragma unroll
              for (uint32_t t = 0; t < PER; t++)
                if (k * PER + t < qlen)
                  ed_step<W>(pq + ((word >> (t * BITS)) & MASK) * W, pv, mv, dd, sw, sb);
            }
          }
        }
        if constexpr (SINK == SINK_NEAREST)
          S.near(r, dd);
        else if (dd <= P.d && active && (!own || e + r > qi))
          S.match(r, dd);
      }
    }
  };

  for (uint32_t p = jb.p0; p < jb.p0 + jb.np; p++) {
    const EdPartner pt = P.partners[p];
    if constexpr (SINK == SINK_NEAREST) {
      /* the partners come by increasing length gap, and no distance is below the gap: once no lane's best reaches
         it, nothing here or later can improve on or tie with what a lane holds.  The whole workgroup votes, in front
         of the staging barrier; an idle lane votes no.  (P.prune is the launch's: 0 walks every partner) */
      const uint32_t gap = pt.len > qlen ? pt.len - qlen : qlen - pt.len;
      if (P.prune && !__syncthreads_or(S.wants(active, gap)))
        break;
    }
    /* (the own group: the workgroup whose first query sits at position b walks the references behind b only, and its
       segments divide THAT range) */
    const uint32_t w0 = SINK == SINK_LINK && pt.own ? min(wg_q0 + 1u, pt.nr) : 0u;
    uint32_t e0, e1;
    pairs_segment(pt.nr, w0, seg, P.segments, e0, e1);
    if (e0 >= e1)
      continue;                                                         /* (the whole workgroup) */
    uint32_t words = pt.len <= 64 ? 1u : pt.len <= 128 ? 2u : 4u;
    if (words < P.min_words)
      words = P.min_words;
    if (words == 1)
      walk(pt, e0, e1, std::integral_constant<int, 1>());
    else if (words == 2)
      walk(pt, e0, e1, std::integral_constant<int, 2>());
    else
      walk(pt, e0, e1, std::integral_constant<int, 4>());
  }
  S.end(active, qorig, seg);
}

typedef void (*EdKernel)(const EdParams);

template <int SINK>
EdKernel ed_kernel_for(uint32_t nw, bool nt)
{
  if (nt) {                                    /* (64 nucleotides are four words) */
    switch (nw) {
    case 2:  return ed_compare_kernel<2, SINK, true>;
    case 4:  return ed_compare_kernel<4, SINK, true>;
    default: return ed_compare_kernel<0, SINK, true>;
    }
  }
  switch (nw) {
  case 2:  return ed_compare_kernel<2, SINK, false>;
  case 4:  return ed_compare_kernel<4, SINK, false>;
  case 8:  return ed_compare_kernel<8, SINK, false>;
  case 16: return ed_compare_kernel<16, SINK, false>;
  default: return ed_compare_kernel<0, SINK, false>;
  }
}

/* what the entry points share: both sets on the device, the jobs (allpairs.h) */
struct EdWork : PairJobs<EdPartner> {
  EdParams       P{};
};

/* the order of a job's partners.  ED_BY_LENGTH: by increasing length.  ED_TRIANGULAR (the cluster calls, set2 == set1):
   a job keeps the partners of its own length and longer -- an unordered pair of two lengths is seen from the shorter
   side -- and its own group is marked as such.  ED_BY_GAP (the nearest calls): by increasing |L - L'|, of two at one gap
   the shorter first, so that a walk can stop at the first gap above what it holds */
enum EdOrder { ED_BY_LENGTH, ED_TRIANGULAR, ED_BY_GAP };

int ed_setup(cmpr_context *c, const std::string &who, const cmpr_set_view *set1, const cmpr_set_view *set2,
             int64_t differences, bool on_device, EdWork &J, EdOrder order = ED_BY_LENGTH)
{
  const bool triangular = order == ED_TRIANGULAR;
  int rc;
  if ((rc = pairs_stage(c, set1, set2, on_device, J, hm_key_mode(c), pairs_length_check(c, "cmpr_edit"))))
    return rc;
  const HmSet &B = *J.s2;
  const uint64_t longest = std::max(J.s1->longest, B.longest);
  const uint32_t d = (uint32_t)std::min<uint64_t>((uint64_t)differences, longest);   /* above the longest sequence: as that length */
  EdParams &P = J.P;

  /* per set-1 group the set-2 groups of its V and J at the lengths within d, by binary search of their key */
  if ((rc = pairs_jobs(c, who, J, P, [&](const HmGroup &ga, uint64_t genes_of, const PairLengths &L2,
                                         std::vector<EdPartner> &partners) {
         const size_t p0 = partners.size();
         const uint32_t first = triangular ? ga.len : ga.len > d ? ga.len - d : 0u;
         for (auto it = std::lower_bound(L2.len.begin(), L2.len.end(), first);
              it != L2.len.end() && *it <= ga.len + d; ++it)
           if (const HmGroup *gb = hm_group_of(B, (uint64_t)*it * B.per_len + genes_of))
             partners.push_back(EdPartner{gb->pk_off, gb->start, gb->count, gb->len, (uint16_t)gb->stride,
                                          (uint16_t)(triangular && gb->len == ga.len ? 1u : 0u)});
         const auto gap = [&](const EdPartner &x) { return x.len > ga.len ? x.len - ga.len : ga.len - x.len; };
         if (order == ED_BY_GAP)
           std::stable_sort(partners.begin() + (ptrdiff_t)p0, partners.end(),
                            [&](const EdPartner &x, const EdPartner &y) { return gap(x) < gap(y); });
       })))
    return rc;
  /* (the link sink's workgroups walk what lies behind them in their own group: as hm_setup, no segment longer than
     ED_LINK_SEGMENT references) */
  P.segments = pairs_segments(c, c->edit_segments, J.blocks, J.nr_max, triangular ? ED_LINK_SEGMENT : 0u);
  P.d = d;
  P.stage_refs = (uint32_t)c->edit_stage_refs;
  P.min_words = (uint32_t)c->edit_words;
  return CMPR_OK;
}

/* the compare kernel over every job: a launch per run of jobs of one form */
template <int SINK>
int ed_launch(cmpr_context *c, const EdWork &J)
{
  const bool nt = c->opt.alphabet_size == 4;
  return pairs_launch(c, J.runs, J.P, [nt](uint32_t form) { return ed_kernel_for<SINK>(form, nt); });
}

int edit_matrix_impl(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2, int64_t differences,
                     void *matrix_out, bool on_device)
{
  if (!c)
    return CMPR_EINVAL;
  const std::string who = "cmpr_edit_matrix";
  int rc;
  if ((rc = hm_refusals(c, who, set1, set2, differences, HM_MATRIX, on_device, true)))
    return rc;
  if (!matrix_out)
    return fail(c, CMPR_EINVAL, who + ": matrix_out is NULL");
  EdWork J;
  if ((rc = pairs_timed_setup(c, c->ed_ms, false,
                              [&] { return ed_setup(c, who, set1, set2, differences, on_device, J); })))
    return rc;
  return pairs_matrix(c, J, J.P.sink, matrix_out, on_device, [&] { return ed_launch<SINK_MATRIX>(c, J); }, c->ed_ms, 3);
}

int edit_neighbors_impl(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2, int64_t differences,
                        uint64_t capacity, uint64_t *row_start_out, uint32_t *hit_out, uint16_t *dist_out,
                        uint64_t *n_edges_out, bool on_device)
{
  if (!c)
    return CMPR_EINVAL;
  const std::string who = "cmpr_edit_neighbors";
  int rc;
  if ((rc = pairs_neighbors_args(c, who, capacity, hit_out, n_edges_out)) ||
      (rc = hm_refusals(c, who, set1, set2, differences, HM_NEIGHBORS, on_device, true)))
    return rc;
  EdWork J;
  if ((rc = pairs_timed_setup(c, c->ed_ms, false,
                              [&] { return ed_setup(c, who, set1, set2, differences, on_device, J); })))
    return rc;
  /* the rows always (the row order reads them); the row order into ed_ms[2] */
  return pairs_neighbors(c, who, J, J.P.segments, J.P.sink, capacity, row_start_out, hit_out, dist_out, n_edges_out,
                         on_device, [&] { return ed_launch<SINK_CSR>(c, J); }, true, c->ed_ms, 2, 3);
}

/* cmpr_edit_cluster* and cmpr_edit_cluster_table*: the set against itself through the link sink, every unordered pair
   once; what follows the launch is pairs_clusters (allpairs.h).  The plain call (T == NULL) fills L's label / size, the
   table call T's four arrays from labels and sizes of nobody's. */
int edit_cluster_impl(cmpr_context *c, const cmpr_set_view *set, int64_t differences, bool on_device, ClusterLinks &L,
                      ClusterTableOut *T, uint64_t *n_clusters_out)
{
  if (!c)
    return CMPR_EINVAL;
  const std::string who = T ? "cmpr_edit_cluster_table" : "cmpr_edit_cluster";
  if (n_clusters_out)
    *n_clusters_out = 0;
  int rc;
  if ((rc = hm_refusals(c, who, set, set, differences, HM_CLUSTERS, on_device, true)))
    return rc;
  EdWork J;
  if ((rc = pairs_timed_setup(c, c->ed_ms, T != nullptr,
                              [&] { return ed_setup(c, who, set, set, differences, on_device, J, ED_TRIANGULAR); })))
    return rc;
  return pairs_clusters(c, *J.s1, c->edit_link_snapshot != 0, on_device, L, T, n_clusters_out,
                        [&](const PairLinks &K) {
                          J.P.link = K;
                          return ed_launch<SINK_LINK>(c, J);
                        },
                        c->ed_ms, 3);
}

/* cmpr_edit_nearest*: one walk through the nearest sink, the partners of a job by increasing length gap and no further
   than the cap; what surrounds the launch is pairs_nearest (allpairs.h) */
int edit_nearest_impl(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2, int64_t min_distance,
                      int64_t max_distance, uint32_t flags, uint32_t *nearest_out, uint16_t *dist_out,
                      uint32_t *ties_out, uint64_t *n_found_out, bool on_device)
{
  if (!c)
    return CMPR_EINVAL;
  const std::string who = "cmpr_edit_nearest";
  if (n_found_out)
    *n_found_out = 0;
  int rc;
  if ((rc = hm_refusals(c, who, set1, set2, min_distance, HM_NEAREST, on_device, true)))
    return rc;
  if (max_distance < 0)
    return fail(c, CMPR_EINVAL, who + ": max_distance cannot be negative");
  if (flags & ~(uint32_t)CMPR_NEAREST_OTHER_REPERTOIRE)
    return fail(c, CMPR_EINVAL, who + ": unknown bits in flags");
  const bool other_rep = (flags & CMPR_NEAREST_OTHER_REPERTOIRE) != 0;
  if (other_rep && set2 != set1)
    return fail(c, CMPR_EINVAL, who + ": CMPR_NEAREST_OTHER_REPERTOIRE needs set2 == set1 (two sets have two numberings "
                                      "of their repertoires)");
  EdWork J;
  if ((rc = pairs_timed_setup(c, c->ed_ms, false,
                              [&] { return ed_setup(c, who, set1, set2, max_distance, on_device, J, ED_BY_GAP); })))
    return rc;
  EdParams &P = J.P;
  P.sink.rep1 = J.s1->rep.b.p; P.sink.rep2 = J.s2->rep.b.p;
  P.floor = (uint32_t)std::min<int64_t>(min_distance, 0x10000);        /* (no distance is above 256) */
  P.one_set = J.s2 == J.s1 ? 1u : 0u;
  P.other_rep = other_rep ? 1u : 0u;
  P.prune = c->edit_nearest_prune ? 1u : 0u;
  return pairs_nearest(c, J, P.segments, nearest_out, dist_out, ties_out, n_found_out, on_device,
                       [&](const PairNearest &N) {
                         P.nn = N;
                         return ed_launch<SINK_NEAREST>(c, J);
                       },
                       c->ed_ms, 3);
}

}  // namespace

extern "C" int cmpr_edit_nearest(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2,
                                 int64_t min_distance, int64_t max_distance, uint32_t flags, uint32_t *nearest_out,
                                 uint16_t *distance_out, uint32_t *ties_out, uint64_t *n_found_out)
{
  return guarded(c, [&] {
    return edit_nearest_impl(c, set1, set2, min_distance, max_distance, flags, nearest_out, distance_out, ties_out,
                             n_found_out, false);
  });
}

extern "C" int cmpr_edit_nearest_device(cmpr_context *c, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                                        int64_t min_distance, int64_t max_distance, uint32_t flags,
                                        uint32_t *d_nearest_out, uint16_t *d_distance_out, uint32_t *d_ties_out,
                                        uint64_t *n_found_out)
{
  return guarded(c, [&] {
    return edit_nearest_impl(c, d_set1, d_set2, min_distance, max_distance, flags, d_nearest_out, d_distance_out,
                             d_ties_out, n_found_out, true);
  });
}

extern "C" int cmpr_edit_cluster(cmpr_context *c, const cmpr_set_view *set, int64_t differences, uint32_t *label_out,
                                 uint32_t *size_out, uint64_t *n_clusters_out)
{
  return guarded(c, [&] {
    ClusterLinks L(label_out, size_out, false);
    return edit_cluster_impl(c, set, differences, false, L, nullptr, n_clusters_out);
  });
}

extern "C" int cmpr_edit_cluster_device(cmpr_context *c, const cmpr_set_view *d_set, int64_t differences,
                                        uint32_t *d_label_out, uint32_t *d_size_out, uint64_t *n_clusters_out)
{
  return guarded(c, [&] {
    ClusterLinks L(d_label_out, d_size_out, true);
    return edit_cluster_impl(c, d_set, differences, true, L, nullptr, n_clusters_out);
  });
}

extern "C" int cmpr_edit_cluster_table(cmpr_context *c, const cmpr_set_view *set, int64_t differences,
                                       uint32_t *cluster_of_out, uint64_t *cluster_start_out, uint32_t *member_out,
                                       uint64_t *count_out, uint64_t *n_clusters_out)
{
  return guarded(c, [&] {
    ClusterLinks L(nullptr, nullptr, false);
    ClusterTableOut T(cluster_of_out, cluster_start_out, member_out, count_out, false);
    return edit_cluster_impl(c, set, differences, false, L, &T, n_clusters_out);
  });
}

extern "C" int cmpr_edit_cluster_table_device(cmpr_context *c, const cmpr_set_view *d_set, int64_t differences,
                                              uint32_t *d_cluster_of_out, uint64_t *d_cluster_start_out,
                                              uint32_t *d_member_out, uint64_t *d_count_out, uint64_t *n_clusters_out)
{
  return guarded(c, [&] {
    ClusterLinks L(nullptr, nullptr, true);
    ClusterTableOut T(d_cluster_of_out, d_cluster_start_out, d_member_out, d_count_out, true);
    return edit_cluster_impl(c, d_set, differences, true, L, &T, n_clusters_out);
  });
}

extern "C" int cmpr_edit_matrix(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2,
                                int64_t differences, uint64_t *matrix_out)
{
  return guarded(c, [&] { return edit_matrix_impl(c, set1, set2, differences, matrix_out, false); });
}

extern "C" int cmpr_edit_matrix_device(cmpr_context *c, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                                       int64_t differences, void *d_matrix)
{
  return guarded(c, [&] { return edit_matrix_impl(c, d_set1, d_set2, differences, d_matrix, true); });
}

extern "C" int cmpr_edit_neighbors(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2,
                                   int64_t differences, uint64_t capacity, uint64_t *row_start_out,
                                   uint32_t *hit_out, uint16_t *distance_out, uint64_t *n_edges_out)
{
  return guarded(c, [&] {
    return edit_neighbors_impl(c, set1, set2, differences, capacity, row_start_out, hit_out, distance_out,
                               n_edges_out, false);
  });
}

extern "C" int cmpr_edit_neighbors_device(cmpr_context *c, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                                          int64_t differences, uint64_t capacity, uint64_t *d_row_start_out,
                                          uint32_t *d_hit_out, uint16_t *d_distance_out, uint64_t *n_edges_out)
{
  return guarded(c, [&] {
    return edit_neighbors_impl(c, d_set1, d_set2, differences, capacity, d_row_start_out, d_hit_out,
                               d_distance_out, n_edges_out, true);
  });
}
