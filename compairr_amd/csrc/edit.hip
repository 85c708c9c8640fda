/*
 * edit.hip -- the all-against-all path under EDIT distance, for any d: cmpr_edit_neighbors / _device and
 * cmpr_edit_matrix / _device.  A pair (i of set 1, j of set 2) matches when the two sequences have the same V and J
 * gene numbers unless ignore_genes and their Levenshtein distance -- substitution, insertion and deletion cost 1 each --
 * is at most `differences`.  The reference has indels at d = 1 only (its variant enumeration explodes beyond); nothing
 * is enumerated or hashed here: every query is compared with every sequence of every group it can match.
 *
 *   group    hamming.hip's, through hamming_sets.h: each set sorted by (length, V, J) with a stable radix sort, its
 *            residues packed in group order.  Sequences of more than ED_MAX_LEN = 256 residues are refused.
 *   jobs     on the host, from the two group tables: a set-1 group (L, V, J) and its PARTNERS, the set-2 groups
 *            (L', V, J) with |L - L'| <= d, found by binary search of the key for every length L' set 2 has (a huge d
 *            costs nothing).  The partners of a job are contiguous in one array.
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
 *            unrolled at compile time under the uniform `pos < len`) while it has at most ED_REG_RESIDUES = 64
 *            residues: every CDR3 and junction of amino acids.  A longer query is read word by word from global
 *            memory (NW = 0: one load per four or sixteen column steps); unrolled, 256 steps of four column words
 *            would be straight-line code far beyond the instruction cache.  No instantiation indexes an array at
 *            run time: private_segment_fixed_size is 0 in every one of them (checked in the code object's metadata).
 *   sinks    matrix: hamming.hip's -- the score of a match is added to a per-lane sum that goes to its cell when the
 *            lane's next match lies in another set-2 repertoire and at the end, into a copy of the matrix in LDS
 *            when it has at most ED_MAT_CELLS cells, else with 64-bit global atomics.  Integer sums.
 *            count / fill: a lane counts the hits of its (query, segment), the counts are summed in (query,
 *            segment) order (hipcub) and the same walk writes every hit and its distance at the lane's running
 *            offset.  The walk goes partner by partner, which is not number order, so the rows are sorted
 *            afterwards by csr_rows.h with the 64-bit key (hit << 16 | distance) -- the hit alone without
 *            distance_out --, rows beyond LDS_MAX by hipcub's device-wide sort.  The hits of a row are distinct: the
 *            order is total, the bytes do not depend on the schedule.
 *
 * Nothing here writes the resident sets, plans or statistics of the context.
 */
#include "csr_rows.h"
#include "hamming_sets.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

using namespace cmpr;

namespace {

constexpr uint32_t ED_WG = 256;                /* four waves: four 64-query tiles of one job */
constexpr uint32_t ED_MAX_LEN = 256;           /* residues of the longest sequence: four 64-bit column words */
constexpr uint32_t ED_REG_RESIDUES = 64;       /* a query of more residues is read from global memory (NW = 0) */
constexpr uint32_t ED_PEQ_WORDS = 2048;        /* 64-bit words of Peq staged at a time (16 KiB) */
constexpr uint32_t ED_STAGE_MAX = 512;         /* ... and at most this many references */
constexpr uint32_t ED_MAT_CELLS = 1024;        /* a matrix of up to this many cells is privatised in LDS (8 KiB) */
constexpr uint32_t ED_MAX_SEGMENTS = 64;

/* a set-2 group a job is compared with */
struct EdPartner {
  uint64_t pk_off;                 /* first packed word of the group */
  uint32_t r0, nr;                 /* positions in set 2's sorted order */
  uint32_t len, stride;            /* residues and packed words per sequence */
};

/* a set-1 group and its partners */
struct EdJob {
  uint64_t pk1;                    /* first packed word of the group */
  uint32_t q0, nq;                 /* positions in set 1's sorted order */
  uint32_t len, stride;
  uint32_t p0, np;                 /* its partners in the partner array */
  uint32_t blk0, pad;              /* first workgroup (grid x) of the job */
};

struct EdParams {
  const EdJob     *jobs;
  const EdPartner *partners;
  uint32_t        njobs, segments;
  const uint32_t *pk1, *pk2;       /* packed words */
  const uint32_t *ord1, *ord2;     /* sequence numbers in group order */
  uint32_t        d, stage_refs, min_words;
  uint32_t        blk_base;        /* workgroup number of this launch's first workgroup */
  /* count / fill */
  uint32_t       *cnt;             /* [n1 x segments]: hits of (query, segment) */
  const unsigned long long *offs;  /* their exclusive sum; NULL: the count step */
  uint32_t       *hit;
  uint16_t       *dist;            /* may be NULL */
  /* matrix */
  const uint32_t *rep1, *rep2;
  const uint64_t *cnt1, *cnt2;     /* NULL: ignore_counts */
  uint32_t        R2, score, existence, mat_lds;
  unsigned long long *matrix;
  uint32_t        cells;
};

enum { SINK_CSR = 0, SINK_MATRIX = 1 };

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

/* what a lane keeps of its matches */
struct EdLaneSink {
  /* CSR */
  uint32_t hits = 0;
  unsigned long long pos = 0;
  /* matrix */
  unsigned long long acc = 0, row = 0, f = 1;
  uint32_t cur_rep = 0;
};

/* NW: words of the query held in registers, 0: the query is read from global memory */
template <int NW, int SINK, bool NT>
__global__ void __launch_bounds__(ED_WG)
ed_compare_kernel(const EdParams P)
{
  constexpr uint32_t A = NT ? 4 : 20, PER = NT ? 16 : 4, BITS = NT ? 2 : 8, MASK = NT ? 3 : 0xff;
  __shared__ unsigned long long st_peq[ED_PEQ_WORDS];
  __shared__ uint32_t st_id[ED_STAGE_MAX];
  __shared__ uint32_t st_rep[SINK == SINK_MATRIX ? ED_STAGE_MAX : 1];
  __shared__ unsigned long long st_cnt[SINK == SINK_MATRIX ? ED_STAGE_MAX : 1];
  __shared__ unsigned long long st_mat[SINK == SINK_MATRIX ? ED_MAT_CELLS : 1];

  /* the job of this workgroup: the last one whose first workgroup is not behind it */
  const uint32_t blk = P.blk_base + blockIdx.x;
  uint32_t lo = 0, hi = P.njobs - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (P.jobs[mid].blk0 <= blk)
      lo = mid;
    else
      hi = mid - 1;
  }
  const EdJob jb = P.jobs[lo];
  const uint32_t qi = (blk - jb.blk0) * ED_WG + threadIdx.x;            /* query within the group */
  const bool active = qi < jb.nq;
  const uint32_t qpos = jb.q0 + (active ? qi : 0u);                     /* (an idle lane reads the group's first query) */
  const uint32_t qorig = P.ord1[qpos];
  const uint32_t qlen = jb.len;
  const uint32_t seg = blockIdx.y;

  const bool mat_lds = SINK == SINK_MATRIX && P.mat_lds;
  if (mat_lds) {                                                        /* (a barrier follows before the first flush) */
    for (uint32_t k = threadIdx.x; k < P.cells; k += ED_WG)
      st_mat[k] = 0;
  }

  const uint32_t *const qw = P.pk1 + jb.pk1 + (uint64_t)(qpos - jb.q0) * jb.stride;
  uint32_t q[NW ? NW : 1];
  if (NW) {
#pragma unroll
    for (int k = 0; k < NW; k++)
      q[k] = (uint32_t)k < jb.stride ? qw[k] : 0u;
  }

  EdLaneSink S;
  if (SINK == SINK_CSR) {
    if (P.offs)
      S.pos = P.offs[(uint64_t)qorig * P.segments + seg];
  } else {
    S.row = P.existence ? (unsigned long long)qorig : (unsigned long long)P.rep1[qorig];
    S.f = P.cnt1 ? P.cnt1[qorig] : 1ull;
  }
  auto flush = [&]() {
    if (SINK == SINK_MATRIX && S.acc) {
      const uint64_t cell = S.row * P.R2 + S.cur_rep;
      if (mat_lds)
        atomicAdd(&st_mat[cell], S.acc);
      else
        atomicAdd(P.matrix + cell, S.acc);
      S.acc = 0;
    }
  };
  /* reference r of the staged piece matched at distance `dd` */
  auto sink = [&](uint32_t r, uint32_t dd) {
    if (SINK == SINK_CSR) {
      if (P.offs) {
        P.hit[S.pos] = st_id[r];
        if (P.dist)
          P.dist[S.pos] = (uint16_t)dd;
        S.pos++;
      } else {
        S.hits++;
      }
    } else {
      /* the lane's sum belongs to one set-2 repertoire: a match in another one sends it to its cell first */
      const uint32_t rp = st_rep[r];
      if (rp != S.cur_rep) {
        flush();
        S.cur_rep = rp;
      }
      S.acc += P.cnt1 ? pair_score(P.score, S.f, st_cnt[r]) : 1ull;
    }
  };

  /* the references e0 .. e1 - 1 of partner pt, their columns W words long */
  auto walk = [&](const EdPartner &pt, uint32_t e0, uint32_t e1, auto words) {
    constexpr int W = decltype(words)::value;
    const uint32_t n = pt.len;
    const uint32_t sw = n ? (n - 1) >> 6 : 0u, sb = n ? (n - 1) & 63u : 0u;
    uint32_t R = ED_PEQ_WORDS / (A * W);
    if (R > ED_STAGE_MAX) R = ED_STAGE_MAX;
    if (P.stage_refs && P.stage_refs < R) R = P.stage_refs;
    for (uint32_t e = e0; e < e1; e += R) {
      const uint32_t cnt = e1 - e < R ? e1 - e : R;
      __syncthreads();                                                  /* the previous piece has been read */
      /* Peq: one thread per (reference, symbol, word); st_peq[(r x A + symbol) x W + w] */
      for (uint32_t it = threadIdx.x; it < cnt * A * W; it += ED_WG) {
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
      for (uint32_t r = threadIdx.x; r < cnt; r += ED_WG) {
        const uint32_t id = P.ord2[pt.r0 + e + r];
        st_id[r] = id;
        if (SINK == SINK_MATRIX) {
          st_rep[r] = P.rep2[id];
          st_cnt[r] = P.cnt2 ? P.cnt2[id] : 1ull;
        }
      }
      __syncthreads();
      for (uint32_t r = 0; r < cnt; r++) {
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
        if (dd <= P.d && active)
          sink(r, dd);
      }
    }
  };

  for (uint32_t p = jb.p0; p < jb.p0 + jb.np; p++) {
    const EdPartner pt = P.partners[p];
    const uint32_t e0 = (uint32_t)((uint64_t)pt.nr * seg / P.segments);
    const uint32_t e1 = (uint32_t)((uint64_t)pt.nr * (seg + 1) / P.segments);
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

  if (SINK == SINK_CSR) {
    if (!P.offs && active)
      P.cnt[(uint64_t)qorig * P.segments + seg] = S.hits;
  } else {
    flush();
    if (mat_lds) {
      __syncthreads();
      for (uint32_t k = threadIdx.x; k < P.cells; k += ED_WG)
        if (st_mat[k])
          atomicAdd(P.matrix + k, st_mat[k]);
    }
  }
}

typedef void (*EdKernel)(const EdParams);

/* the register form of a query of `len` residues in `stride` packed words: 2, 4, 8, 16, or 0 */
uint32_t ed_form_of(uint32_t len, uint32_t stride)
{
  if (len > ED_REG_RESIDUES)
    return 0;
  for (uint32_t f : {2u, 4u, 8u, 16u})
    if (stride <= f)
      return f;
  return 0;
}

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

/* row_start[i] = the offset of (query i, segment 0); row_start[n1] = the edge count */
__global__ void __launch_bounds__(ED_WG)
ed_rows_kernel(const unsigned long long *offs, uint64_t n1, uint32_t segments, uint64_t *row_start)
{
  const uint64_t i = (uint64_t)blockIdx.x * ED_WG + threadIdx.x;
  if (i <= n1)
    row_start[i] = offs[i * segments];
}

/* census[0] rows longer than a wave, [1] of those the rows longer than LDS, [2] the longest row when it is longer than
   LDS (csr_rows.h sizes its lists by them) */
__global__ void __launch_bounds__(ROW_WG)
ed_census_kernel(const uint64_t *row_start, uint64_t n, unsigned long long *census)
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

/* the rows ordered by the hit, the distance of each edge carried along: a row never holds a hit twice, so the low
   sixteen bits of the key never decide (csr_rows.h) */
struct EdRows {
  using Key = unsigned long long;
  static constexpr Key  PAD = ~0ull;
  static constexpr bool COUNT_HEADS = false;
  uint32_t *hit;
  uint16_t *dist;
  __device__ Key load(uint64_t pos) const { return (Key)hit[pos] << 16 | dist[pos]; }
  __device__ void store(uint64_t pos, Key key) const
  {
    hit[pos] = (uint32_t)(key >> 16);
    dist[pos] = (uint16_t)key;
  }
  __device__ static bool same_run(Key, Key) { return true; }
};

/* ... without distance_out: the hits alone */
struct EdHitRows {
  using Key = uint32_t;
  static constexpr Key  PAD = 0xffffffffu;   /* no sequence number (a set has at most 2^31 - 1 sequences) */
  static constexpr bool COUNT_HEADS = false;
  uint32_t *hit;
  __device__ Key load(uint64_t pos) const { return hit[pos]; }
  __device__ void store(uint64_t pos, Key key) const { hit[pos] = key; }
  __device__ static bool same_run(Key, Key) { return true; }
};

/* what the four entry points share: both sets on the device, the jobs */
struct EdWork {
  HmSet          own1, own2;
  HmSet         *s1 = nullptr, *s2 = nullptr;
  Tmp<EdJob>     jobs;
  Tmp<EdPartner> partners;
  EdParams       P{};
  std::vector<std::pair<uint32_t, std::pair<uint32_t, uint32_t>>> runs;   /* form | first workgroup, workgroups */
};

int ed_stage(cmpr_context *c, const cmpr_set_view *set, bool on_device, HmSet &H)
{
  int rc;
  if ((rc = cmpr_stage_set(c, set, on_device, H)))
    return rc;
  if (H.longest > ED_MAX_LEN)
    return fail(c, CMPR_EUNSUPPORTED, "cmpr_edit: a sequence of more than 256 residues");
  return hm_prepare(c, H);
}

int ed_setup(cmpr_context *c, const std::string &who, const cmpr_set_view *set1, const cmpr_set_view *set2,
             int64_t differences, bool on_device, EdWork &J)
{
  int rc;
  if ((rc = ed_stage(c, set1, on_device, J.own1))) return rc;
  J.s1 = &J.own1;
  if (set2 == set1) {
    J.s2 = J.s1;
  } else {
    if ((rc = ed_stage(c, set2, on_device, J.own2))) return rc;
    J.s2 = &J.own2;
  }
  HmSet &A = *J.s1, &B = *J.s2;
  const uint64_t longest = std::max(A.longest, B.longest);
  const uint32_t d = (uint32_t)std::min<uint64_t>((uint64_t)differences, longest);   /* above the longest sequence: as that length */

  /* the lengths set 2 has (the keys increase with the length); per set-1 group the set-2 groups of its V and J at
     the lengths within d, by binary search of their key */
  const bool genes = !c->opt.ignore_genes;
  const uint64_t vj = genes ? (uint64_t)std::max<uint32_t>(1, c->opt.n_v_genes) * std::max<uint32_t>(1, c->opt.n_j_genes) : 1;
  std::vector<uint32_t> lens2;
  for (const HmGroup &g : B.groups)
    if (lens2.empty() || lens2.back() != g.len)
      lens2.push_back(g.len);
  std::vector<EdJob> jobs;
  std::vector<EdPartner> partners;
  uint64_t blocks = 0;
  uint32_t nr_max = 0;
  for (size_t a = 0; a < A.groups.size(); a++) {
    const HmGroup &ga = A.groups[a];
    const uint64_t genes_of = A.keys[a] % vj;
    const uint32_t first = ga.len > d ? ga.len - d : 0u;
    const size_t p0 = partners.size();
    for (auto it = std::lower_bound(lens2.begin(), lens2.end(), first); it != lens2.end() && *it <= ga.len + d; ++it) {
      const uint64_t key = (uint64_t)*it * vj + genes_of;
      const auto k = std::lower_bound(B.keys.begin(), B.keys.end(), key);
      if (k == B.keys.end() || *k != key)
        continue;
      const HmGroup &gb = B.groups[(size_t)(k - B.keys.begin())];
      partners.push_back(EdPartner{gb.pk_off, gb.start, gb.count, gb.len, gb.stride});
      nr_max = std::max(nr_max, gb.count);
    }
    if (partners.size() == p0)
      continue;
    const uint32_t nb = blocks_for(ga.count, ED_WG);
    const uint32_t form = ed_form_of(ga.len, ga.stride);
    if (!J.runs.empty() && J.runs.back().first == form)
      J.runs.back().second.second += nb;
    else
      J.runs.push_back({form, {(uint32_t)blocks, nb}});
    jobs.push_back(EdJob{ga.pk_off, ga.start, ga.count, ga.len, ga.stride, (uint32_t)p0,
                         (uint32_t)(partners.size() - p0), (uint32_t)blocks, 0u});
    blocks += nb;
    if (blocks > 0xffffffu)
      return fail(c, CMPR_EUNSUPPORTED, who + ": more than 2^24 workgroups of queries");
  }
  if (partners.size() > 0xffffffffull)
    return fail(c, CMPR_EUNSUPPORTED, who + ": more than 2^32-1 pairs of groups");
  if (!jobs.empty()) {
    if ((rc = dev_upload(c, J.jobs.b, jobs.data(), jobs.size()))) return rc;
    if ((rc = dev_upload(c, J.partners.b, partners.data(), partners.size()))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));           /* (the two vectors leave scope) */
  }
  /* segments: as many as fill the machine while the query tiles alone do not, none shorter than a wave of references */
  uint32_t S = 1;
  if (c->edit_segments) {
    S = (uint32_t)c->edit_segments;
  } else if (blocks) {
    const uint64_t target = (uint64_t)c->cus * 8;
    S = (uint32_t)std::min<uint64_t>(ED_MAX_SEGMENTS, (target + blocks - 1) / blocks);
    S = std::max<uint32_t>(1, std::min<uint32_t>(S, (nr_max + 63) / 64));
  }
  EdParams &P = J.P;
  P.jobs = J.jobs.b.p;
  P.partners = J.partners.b.p;
  P.njobs = (uint32_t)jobs.size();
  P.segments = S;
  P.pk1 = A.pk.b.p; P.pk2 = B.pk.b.p;
  P.ord1 = A.ord.b.p; P.ord2 = B.ord.b.p;
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
  for (const auto &run : J.runs) {
    const EdKernel fn = ed_kernel_for<SINK>(run.first, nt);
    EdParams P = J.P;
    P.blk_base = run.second.first;
    hipLaunchKernelGGL(fn, dim3(run.second.second, P.segments), dim3(ED_WG), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
  }
  return CMPR_OK;
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
  auto t0 = std::chrono::steady_clock::now();
  for (double &t : c->ed_ms)
    t = 0;
  EdWork J;
  if ((rc = ed_setup(c, who, set1, set2, differences, on_device, J)))
    return rc;
  c->ed_ms[0] = ms_since(t0);
  t0 = std::chrono::steady_clock::now();

  const uint64_t rows = c->opt.existence ? J.s1->n : J.s1->R, cells = rows * J.s2->R;
  if (cells == 0)
    return CMPR_OK;
  Out<unsigned long long> matrix((unsigned long long *)matrix_out, on_device);
  if ((rc = matrix.temp(c, (size_t)cells))) return rc;
  HIP_TRY(c, hipMemsetAsync(matrix.p, 0, cells * sizeof(unsigned long long), c->stream));
  EdParams &P = J.P;
  P.rep1 = J.s1->rep.b.p; P.rep2 = J.s2->rep.b.p;
  P.cnt1 = c->opt.ignore_counts ? nullptr : J.s1->cnt.b.p;
  P.cnt2 = c->opt.ignore_counts ? nullptr : J.s2->cnt.b.p;
  P.R2 = J.s2->R;
  P.score = (uint32_t)c->opt.score;
  P.existence = c->opt.existence ? 1u : 0u;
  P.mat_lds = !c->opt.existence && cells <= ED_MAT_CELLS ? 1u : 0u;
  P.matrix = matrix.p;
  P.cells = (uint32_t)std::min<uint64_t>(cells, ED_MAT_CELLS);
  if ((rc = ed_launch<SINK_MATRIX>(c, J)))
    return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->ed_ms[1] = ms_since(t0);
  if (!on_device) {
    t0 = std::chrono::steady_clock::now();
    if ((rc = matrix.copy_out(c, (size_t)cells))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->ed_ms[3] = ms_since(t0);
  }
  return CMPR_OK;
}

/* every row of the filled CSR put in increasing order of the hit (csr_rows.h; the rows beyond LDS by hipcub) */
int ed_order_rows(cmpr_context *c, const std::string &who, const uint64_t *row_start, uint64_t n1, uint64_t total,
                  uint32_t *hit, uint16_t *dist)
{
  int rc;
  Tmp<unsigned long long> census, long_desc;
  Tmp<uint32_t> big_rows, scratch;
  Tmp<uint16_t> dist_scratch;
  Tmp<char> sort_tmp;
  if ((rc = dev_alloc(c, census.b, 5))) return rc;         /* [0..2] the census, [3..4] the list counters */
  HIP_TRY(c, hipMemsetAsync(census.b.p, 0, 5 * sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(ed_census_kernel, dim3(blocks_for(n1, ROW_WG)), dim3(ROW_WG), 0, c->stream, row_start, n1,
                     census.b.p);
  HIP_TRY(c, hipGetLastError());
  unsigned long long seen[3] = {0, 0, 0};
  HIP_TRY(c, hipMemcpyAsync(seen, census.b.p, sizeof seen, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint64_t n_long = seen[1], n_big = seen[0] - seen[1], longest = seen[2];
  if (seen[1] > seen[0] || seen[0] > n1 || longest > total)
    return fail(c, CMPR_EDEVICE, who + ": the census of the rows is out of range");
  size_t sort_bytes = 0;
  if (n_big && (rc = dev_alloc(c, big_rows.b, (size_t)n_big))) return rc;
  if (n_long) {
    if ((rc = dev_alloc(c, long_desc.b, (size_t)(LONG_WORDS * n_long)))) return rc;
    if ((rc = dev_alloc(c, scratch.b, (size_t)longest))) return rc;
    if (dist) {
      if ((rc = dev_alloc(c, dist_scratch.b, (size_t)longest))) return rc;
      HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                    (const uint16_t *)nullptr, (uint16_t *)nullptr, (size_t)longest, 0,
                                                    32, c->stream));
    } else {
      HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                   (size_t)longest, 0, 32, c->stream));
    }
    if ((rc = dev_alloc(c, sort_tmp.b, sort_bytes))) return rc;
  }
  const RowLists lists{big_rows.b.p, n_big, long_desc.b.p, n_long, census.b.p + 3};   /* (counters: zero) */
  if ((rc = dist ? rows_sort(c, row_start, n1, lists, EdRows{hit, dist}) : rows_sort(c, row_start, n1, lists, EdHitRows{hit})))
    return rc;
  if (n_long) {
    std::vector<LongRow> lr;
    if ((rc = rows_fetch_long(c, lists, longest, total, n1, who.c_str(), lr)))
      return rc;
    for (const LongRow &r : lr) {
      size_t b = sort_bytes;
      if (dist) {
        HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(sort_tmp.b.p, b, (const uint32_t *)(hit + r.start), scratch.b.p,
                                                      (const uint16_t *)(dist + r.start), dist_scratch.b.p,
                                                      (size_t)r.len, 0, 32, c->stream));
        HIP_TRY(c, hipMemcpyAsync(dist + r.start, dist_scratch.b.p, (size_t)r.len * sizeof(uint16_t),
                                  hipMemcpyDeviceToDevice, c->stream));
      } else {
        HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(sort_tmp.b.p, b, (const uint32_t *)(hit + r.start), scratch.b.p,
                                                     (size_t)r.len, 0, 32, c->stream));
      }
      HIP_TRY(c, hipMemcpyAsync(hit + r.start, scratch.b.p, (size_t)r.len * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                                c->stream));
    }
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));             /* (the temporaries leave scope) */
  return CMPR_OK;
}

int edit_neighbors_impl(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2, int64_t differences,
                        uint64_t capacity, uint64_t *row_start_out, uint32_t *hit_out, uint16_t *dist_out,
                        uint64_t *n_edges_out, bool on_device)
{
  if (!c)
    return CMPR_EINVAL;
  const std::string who = "cmpr_edit_neighbors";
  if (!n_edges_out)
    return fail(c, CMPR_EINVAL, who + ": n_edges_out is NULL");
  *n_edges_out = 0;
  if (capacity && !hit_out)
    return fail(c, CMPR_EINVAL, who + ": hit_out is NULL with a capacity");
  int rc;
  if ((rc = hm_refusals(c, who, set1, set2, differences, HM_NEIGHBORS, on_device, true)))
    return rc;
  auto t0 = std::chrono::steady_clock::now();
  for (double &t : c->ed_ms)
    t = 0;
  EdWork J;
  if ((rc = ed_setup(c, who, set1, set2, differences, on_device, J)))
    return rc;
  c->ed_ms[0] = ms_since(t0);
  t0 = std::chrono::steady_clock::now();

  /* count per (query, segment); the sum; the rows (the row order below needs them, asked for or not) */
  const uint64_t n1 = J.s1->n, S = J.P.segments, slots = n1 * S + 1;   /* (a zero behind the last: the sum's last is the total) */
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
  EdParams &P = J.P;
  P.cnt = cnt.b.p;
  if ((rc = ed_launch<SINK_CSR>(c, J)))
    return rc;
  hipcub::TransformInputIterator<unsigned long long, U32To64, const uint32_t *> wide(cnt.b.p, U32To64());
  size_t scan_bytes = 0;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, wide, offs.b.p, (int)slots, c->stream));
  if ((rc = dev_alloc(c, scan_tmp.b, scan_bytes))) return rc;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(scan_tmp.b.p, scan_bytes, wide, offs.b.p, (int)slots, c->stream));
  if ((rc = rows.temp(c, (size_t)(n1 + 1)))) return rc;
  hipLaunchKernelGGL(ed_rows_kernel, dim3(blocks_for(n1 + 1, ED_WG)), dim3(ED_WG), 0, c->stream, offs.b.p, n1,
                     (uint32_t)S, rows.p);
  HIP_TRY(c, hipGetLastError());
  unsigned long long total = 0;
  HIP_TRY(c, hipMemcpyAsync(&total, offs.b.p + (slots - 1), sizeof total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *n_edges_out = total;

  /* the same walk again, every hit to its place -- when there is room for all of them --, then the rows in order */
  const bool fill = hit.wanted() && total && total <= capacity;
  if (fill) {
    if ((rc = hit.temp(c, (size_t)total))) return rc;
    if (dist.wanted() && (rc = dist.temp(c, (size_t)total))) return rc;
    P.offs = offs.b.p;
    P.hit = hit.p;
    P.dist = dist.p;
    if ((rc = ed_launch<SINK_CSR>(c, J)))
      return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  c->ed_ms[1] = ms_since(t0);
  if (fill) {
    t0 = std::chrono::steady_clock::now();
    if ((rc = ed_order_rows(c, who, rows.p, n1, total, hit.p, dist.p)))
      return rc;
    c->ed_ms[2] = ms_since(t0);
  }
  if (!on_device) {
    t0 = std::chrono::steady_clock::now();
    if ((rc = rows.copy_out(c, (size_t)(n1 + 1)))) return rc;
    if (fill) {
      if ((rc = hit.copy_out(c, (size_t)total))) return rc;
      if ((rc = dist.copy_out(c, (size_t)total))) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->ed_ms[3] = ms_since(t0);
  }
  return CMPR_OK;
}

}  // namespace

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
