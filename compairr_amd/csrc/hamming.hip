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
 *   group    every sequence gets the 64-bit key (length, V, J) -- the length alone with ignore_genes --; hipcub's
 *            stable radix sort of (key, sequence number) per set, so inside a group the sequences stay in increasing
 *            number; the runs of equal keys are the groups (hipcub run-length encode).  The host reads the two group
 *            tables -- as many entries as there are distinct keys, not sequences -- and matches them by key.
 *   pack     the residues of each set in group order, 32-bit words, a fixed number of words per sequence of a group:
 *            four amino acids (a byte each) or sixteen nucleotides (two bits each) per word.  The words are zeroed
 *            and the residues or-ed in: the padding of a last word is zero on both sides.  Groups of at most
 *            HAMMING_REG_WORDS words are padded to the next of the word counts the register form is compiled for.
 *   compare  hm_compare_kernel.  A workgroup of four waves takes four 64-query tiles of one group and one segment of
 *            the matching set-2 group; it stages the segment's packed sequences in LDS, HM_LDS_WORDS at a time, and
 *            every lane walks the staged references with its query's words in registers (register form) or read
 *            from global memory (generic form: groups of more than HAMMING_REG_WORDS words; a reference that does
 *            not fit the LDS buffer is staged in runs of words).  All lanes read the same reference word: an LDS
 *            broadcast.  Differing residues per word: xor, SWAR, popcount.
 *   sinks    matrix: the score of a match is added to a per-lane sum, which goes to its cell when the lane's next
 *            match lies in another set-2 repertoire and at the end -- into a copy of the matrix in LDS when it has
 *            at most HM_MAT_CELLS cells (added to the global one once per workgroup), else with 64-bit global
 *            atomics.  With `existence` the row is the lane's own.  Integer sums: the same in any order.
 *            count / fill: a lane counts the hits of its (query, segment), the counts are summed in (query,
 *            segment) order (hipcub), and the same walk writes every hit and its distance at the lane's running
 *            offset.  All hits of a query lie in ONE set-2 group, walked in increasing sequence number: the rows
 *            come out sorted, without atomics and without a row sort.
 *            link (the cluster calls: the set against itself, every group paired with itself): the forest of
 *            link_forest.h over the ORIGINAL sequence numbers.  Position order inside a group is number order, so the
 *            lane whose query sits at position qi links only references at positions above qi: every unordered pair
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
 *            the ties -- and hm_nearest_fold_kernel takes the smallest key of a query and sums the ties of the slots
 *            at its distance.  Outputs and slots are set to "none" on the stream first: what no lane visits stays so.
 *
 * The (query, segment) count array has n1 x S words, S <= HM_MAX_SEGMENTS; the automatic S is above 1 only while
 * the query tiles alone do not fill the machine (S <= ceil(8 x CUs / workgroups)), which bounds it by
 * 256 x (8 x CUs + workgroups) words.  Nothing here writes the resident sets, plans or statistics of the context.
 */
#include "hamming_sets.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

using namespace cmpr;

namespace {

constexpr uint32_t HM_WG = 256;                /* four waves: four 64-query tiles of one group */
constexpr uint32_t HAMMING_REG_WORDS = 16;     /* the bound between the two forms: a group of more words per sequence
                                                  (64 amino acids, 256 nucleotides) takes the generic form */
constexpr uint32_t HM_LDS_WORDS = 4096;        /* packed words of references staged at a time (16 KiB) */
constexpr uint32_t HM_STAGE_MAX = 512;         /* ... and at most this many references */
constexpr uint32_t HM_MAT_CELLS = 1024;        /* a matrix of up to this many cells is privatised in LDS (8 KiB) */
constexpr uint32_t HM_MAX_SEGMENTS = 64;
constexpr uint32_t HM_LINK_SEGMENT = 16384;    /* link sink: references of the longest automatic segment (32 pieces) */
constexpr uint32_t AA_PER_WORD = 4, NT_PER_WORD = 16;

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
  /* link */
  uint32_t       *parent;          /* the forest, over original sequence numbers (link_forest.h) */
  uint32_t        snapshot;        /* 1: matches whose two root snapshots are equal are skipped */
  /* nearest (rep1, rep2 as the matrix has them, read with other_rep only) */
  uint32_t        floor;           /* a candidate differs at this many positions or more */
  uint32_t        one_set;         /* 1: set 2 IS set 1, a query is no candidate of its own */
  uint32_t        other_rep;       /* 1: a candidate comes from another repertoire than the query */
  uint32_t       *nn_nearest;      /* one segment: the three results, each may be NULL */
  uint16_t       *nn_dist;
  uint32_t       *nn_ties;
  unsigned long long *nn_key;      /* several: [n1 x segments] (distance << 32 | number), all ones: none */
  uint32_t       *nn_slot_ties;    /* ... and the references of the segment at that distance */
};

enum { SINK_CSR = 0, SINK_MATRIX = 1, SINK_LINK = 2, SINK_NEAREST = 3 };

constexpr uint32_t HM_NONE = 0xffffffffu;      /* nearest sink: the infinite distance, and "no sequence" */

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

/* what a lane keeps of its matches */
struct LaneSink {
  /* CSR */
  uint32_t hits = 0;
  unsigned long long pos = 0;
  /* matrix */
  unsigned long long acc = 0, row = 0, f = 1;
  uint32_t cur_rep = 0;
  /* link: the root of the lane's query when it last looked */
  uint32_t root = 0;
  /* nearest: the smallest distance so far, the position in the group of the first reference at it, how many at it */
  uint32_t best = HM_NONE, bpos = 0, ties = 0;
};

/* NW: words per sequence held in registers (the group's stride), 0: the generic form */
template <int NW, int SINK, bool NT>
__global__ void __launch_bounds__(HM_WG)
hm_compare_kernel(const HmParams P)
{
  __shared__ uint32_t st_words[HM_LDS_WORDS];
  __shared__ uint32_t st_id[HM_STAGE_MAX];
  __shared__ uint32_t st_rep[SINK == SINK_MATRIX || SINK == SINK_NEAREST ? HM_STAGE_MAX : 1];
  __shared__ unsigned long long st_cnt[SINK == SINK_MATRIX ? HM_STAGE_MAX : 1];
  __shared__ unsigned long long st_mat[SINK == SINK_MATRIX ? HM_MAT_CELLS : 1];
  __shared__ uint32_t st_root[SINK == SINK_LINK ? HM_STAGE_MAX : 1];

  /* the pair of this workgroup: the last one whose first workgroup is not behind it */
  const uint32_t blk = P.blk_base + blockIdx.x;
  uint32_t lo = 0, hi = P.npairs - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (P.pairs[mid].blk0 <= blk)
      lo = mid;
    else
      hi = mid - 1;
  }
  const HmPair pr = P.pairs[lo];
  const uint32_t stride = NW ? (uint32_t)NW : pr.stride;
  const uint32_t qi = (blk - pr.blk0) * HM_WG + threadIdx.x;     /* query within the group */
  const bool active = qi < pr.nq;
  const uint32_t qpos = pr.q0 + (active ? qi : 0u);                     /* (an idle lane reads the group's first query) */
  const uint32_t qorig = P.ord1[qpos];
  /* the segment of the set-2 group.  Link sink: set 2 IS set 1 and position order is number order (the stable
     sort), so an unordered pair is walked once, by the lane of its smaller position: the workgroup whose first
     query sits at position b walks the references behind b only, and its segments divide THAT range. */
  const uint32_t seg = blockIdx.y;
  const uint32_t w0 = SINK == SINK_LINK ? min((blk - pr.blk0) * HM_WG + 1u, pr.nr) : 0u;
  const uint32_t e0 = w0 + (uint32_t)((uint64_t)(pr.nr - w0) * seg / P.segments);
  const uint32_t e1 = w0 + (uint32_t)((uint64_t)(pr.nr - w0) * (seg + 1) / P.segments);
  /* ... and a wave skips the staged references at or below its first query: no lane of it wants them */
  const uint32_t wave_q0 = SINK == SINK_LINK
      ? (uint32_t)__builtin_amdgcn_readfirstlane((int)((blk - pr.blk0) * HM_WG + (threadIdx.x & ~(WAVE - 1u)))) : 0u;

  if (e0 >= e1)
    return;                                                             /* (the whole workgroup) */
  const bool mat_lds = SINK == SINK_MATRIX && P.mat_lds;
  if (mat_lds) {                                                        /* (a barrier follows before the first flush) */
    for (uint32_t k = threadIdx.x; k < P.cells; k += HM_WG)
      st_mat[k] = 0;
  }

  const uint32_t *const qw = P.pk1 + pr.pk1 + (uint64_t)(qpos - pr.q0) * stride;
  uint32_t q[NW ? NW : 1];
  if (NW) {
#pragma unroll
    for (int k = 0; k < NW; k++)
      q[k] = qw[k];
  }

  LaneSink S;
  if (SINK == SINK_CSR) {
    if (P.offs)
      S.pos = P.offs[(uint64_t)qorig * P.segments + seg];
  } else if (SINK == SINK_LINK) {
    if (P.snapshot)
      S.root = link_root(P.parent, qorig);
  } else if (SINK == SINK_MATRIX) {
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
    } else if (SINK == SINK_LINK) {
      /* (cluster.cc:165-211 lists the pair, :276-410 walks the lists: here the two trees become one.)  In a dense
         group almost every match joins two sequences that share a root already: equal snapshots prove it --
         trees only merge, whatever was once under a root stays in its component -- and cost no walk; unequal
         ones, stale or not, fall through to link_pair, after which the lane looks its root up again. */
      if (!P.snapshot || st_root[r] != S.root) {
        link_pair(P.parent, qorig, st_id[r]);
        if (P.snapshot)
          S.root = link_root(P.parent, qorig);
      }
    } else {
      /* the lane's sum belongs to one set-2 repertoire: a match in another one sends it to its cell first (a
         reference that does not match costs the matrix sink nothing) */
      const uint32_t rp = st_rep[r];
      if (rp != S.cur_rep) {
        flush();
        S.cur_rep = rp;
      }
      S.acc += P.cnt1 ? pair_score(P.score, S.f, st_cnt[r]) : 1ull;
    }
  };
  /* nearest sink: the position in the group that is the lane's own query (one-set mode: the group is paired with
     itself, as in the link sink) and the repertoire a candidate must not come from; HM_NONE is no position and no
     repertoire */
  const uint32_t nn_self = SINK == SINK_NEAREST && P.one_set ? qi : HM_NONE;
  const uint32_t nn_rep = SINK == SINK_NEAREST && P.other_rep ? P.rep1[qorig] : HM_NONE;
  /* the reference at position `pos` of the group, staged as r, differs at `dd` positions.  What is no candidate is
     infinitely far; then (smaller: the first at it) and (equal: one more at it), as selects */
  auto nearest = [&](uint32_t pos, uint32_t r, uint32_t dd) {
    uint32_t rp = 0;                                                    /* (without the flag: not HM_NONE) */
    if (P.other_rep)                                                    /* (the same for every lane) */
      rp = st_rep[r];
    const bool ok = (dd >= P.floor) & (pos != nn_self) & (rp != nn_rep);
    const uint32_t de = ok ? dd : HM_NONE;
    const bool lt = de < S.best;
    S.ties = lt ? 1u : S.ties + (de == S.best ? 1u : 0u);              /* (the ties of "none" are dropped at the end) */
    S.bpos = lt ? pos : S.bpos;
    S.best = lt ? de : S.best;
  };
  /* sequence numbers, repertoires and counts of the references e .. e + n - 1 of the group */
  auto stage_ids = [&](uint32_t e, uint32_t n) {
    if (SINK == SINK_NEAREST) {                                         /* (the number is looked up once, at the end) */
      if (P.other_rep)
        for (uint32_t r = threadIdx.x; r < n; r += HM_WG)
          st_rep[r] = P.rep2[P.ord2[pr.r0 + e + r]];
      return;
    }
    for (uint32_t r = threadIdx.x; r < n; r += HM_WG) {
      const uint32_t id = P.ord2[pr.r0 + e + r];
      st_id[r] = id;
      if (SINK == SINK_MATRIX) {
        st_rep[r] = P.rep2[id];
        st_cnt[r] = P.cnt2 ? P.cnt2[id] : 1ull;
      }
      if (SINK == SINK_LINK && P.snapshot)
        st_root[r] = link_root(P.parent, id);
    }
  };

  if (stride <= HM_LDS_WORDS) {
    /* whole references, R at a time */
    uint32_t R = HM_LDS_WORDS / stride;
    if (R > HM_STAGE_MAX) R = HM_STAGE_MAX;
    if (P.stage_refs && P.stage_refs < R) R = P.stage_refs;
    for (uint32_t e = e0; e < e1; e += R) {
      const uint32_t n = e1 - e < R ? e1 - e : R;
      __syncthreads();                                                  /* the previous piece has been read */
      const uint32_t *const src = P.pk2 + pr.pk2 + (uint64_t)e * stride;
      for (uint32_t k = threadIdx.x; k < n * stride; k += HM_WG)
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
        if (SINK == SINK_NEAREST)
          nearest(e + r, r, dd);
        else if (dd <= P.d && active && (SINK != SINK_LINK || e + r > qi))
          sink(r, dd);
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
        for (uint32_t k = threadIdx.x; k < m; k += HM_WG)
          st_words[k] = src[k];
        if (k0 == 0)
          stage_ids(e, 1);
        __syncthreads();
        for (uint32_t k = 0; k < m; k++)
          dd += diff_word<NT>(qw[k0 + k], st_words[k]);
      }
      if (SINK == SINK_NEAREST)
        nearest(e, 0, dd);
      else if (dd <= P.d && active && (SINK != SINK_LINK || e > qi))
        sink(0, dd);
    }
  }

  if (SINK == SINK_CSR) {
    if (!P.offs && active)
      P.cnt[(uint64_t)qorig * P.segments + seg] = S.hits;
  } else if (SINK == SINK_MATRIX) {
    flush();
    if (mat_lds) {
      __syncthreads();
      for (uint32_t k = threadIdx.x; k < P.cells; k += HM_WG)
        if (st_mat[k])
          atomicAdd(P.matrix + k, st_mat[k]);
    }
  } else if (SINK == SINK_NEAREST) {
    if (active) {
      const bool none = S.best == HM_NONE;
      const uint32_t id = none ? HM_NONE : P.ord2[pr.r0 + S.bpos];
      const uint32_t ties = none ? 0u : S.ties;
      if (P.segments == 1) {
        if (P.nn_nearest)
          P.nn_nearest[qorig] = id;
        if (P.nn_dist)
          P.nn_dist[qorig] = none ? (uint16_t)0xffffu : (uint16_t)S.best;
        if (P.nn_ties)
          P.nn_ties[qorig] = ties;
      } else {
        const uint64_t slot = (uint64_t)qorig * P.segments + seg;
        P.nn_key[slot] = (unsigned long long)S.best << 32 | id;
        P.nn_slot_ties[slot] = ties;
      }
    }
  }
}

/* the slots of a query folded: the smallest key, and the ties of the slots at its distance summed */
__global__ void __launch_bounds__(HM_WG)
hm_nearest_fold_kernel(const unsigned long long *key, const uint32_t *slot_ties, uint64_t n1, uint32_t segments,
                       uint32_t *nearest, uint16_t *dist, uint32_t *ties)
{
  const uint64_t i = (uint64_t)blockIdx.x * HM_WG + threadIdx.x;
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

}  // namespace

/* words per sequence of a group of `len` residues: the next word count the register form is compiled for, or the
   words themselves beyond HAMMING_REG_WORDS (hamming_sets.h) */
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
  const uint32_t *v, *j;           /* NULL: ignore_genes */
  uint64_t        n, n_v, n_j;
  uint64_t       *key;
  uint32_t       *num;
};

__global__ void __launch_bounds__(HM_WG)
hm_key_kernel(const KeyParams K)
{
  const uint64_t i = (uint64_t)blockIdx.x * HM_WG + threadIdx.x;
  if (i >= K.n)
    return;
  uint64_t key = K.off[i + 1] - K.off[i];
  if (K.v)
    key = (key * K.n_v + K.v[i]) * K.n_j + K.j[i];
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
__global__ void __launch_bounds__(HM_WG)
hm_pack_kernel(const HmPackParams K)
{
  const uint64_t w = (uint64_t)blockIdx.x * HM_WG + threadIdx.x;
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
__global__ void __launch_bounds__(HM_WG)
hm_rows_kernel(const unsigned long long *offs, uint64_t n1, uint32_t segments, uint64_t *row_start)
{
  const uint64_t i = (uint64_t)blockIdx.x * HM_WG + threadIdx.x;
  if (i <= n1)
    row_start[i] = offs[i * segments];
}

}  // namespace

/* the staged set H grouped and packed (hamming_sets.h) */
int cmpr::hm_prepare(cmpr_context *c, HmSet &H)
{
  int rc;
  if (H.n == 0)
    return CMPR_OK;
  if (H.n > 0x7fffffffull)
    return fail(c, CMPR_EUNSUPPORTED, "cmpr_hamming: more than 2^31-1 sequences in one set");

  /* keys, the stable sort, the runs */
  const uint64_t n = H.n;
  const bool genes = !c->opt.ignore_genes;
  const uint64_t n_v = std::max<uint32_t>(1, c->opt.n_v_genes), n_j = std::max<uint32_t>(1, c->opt.n_j_genes);
  Tmp<uint64_t> key, key_sorted, run_key;
  Tmp<uint32_t> num, run_len, nruns;
  Tmp<char> scratch;
  if ((rc = dev_alloc(c, key.b, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, key_sorted.b, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, num.b, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, H.ord.b, (size_t)n))) return rc;
  KeyParams K{H.off.b.p, genes ? H.v.b.p : nullptr, genes ? H.j.b.p : nullptr, n, n_v, n_j, key.b.p, num.b.p};
  hipLaunchKernelGGL(hm_key_kernel, dim3(blocks_for(n, HM_WG)), dim3(HM_WG), 0, c->stream, K);
  HIP_TRY(c, hipGetLastError());
  const uint64_t key_max = genes ? ((uint64_t)H.longest + 1) * n_v * n_j : (uint64_t)H.longest + 1;
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
    x.len = (uint32_t)(genes ? H.keys[g] / (n_v * n_j) : H.keys[g]);
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
  hipLaunchKernelGGL(hm_pack_kernel, dim3(blocks_for(words, HM_WG)), dim3(HM_WG), 0, c->stream, Q);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));             /* (d_groups and the sort's temporaries leave scope) */
  return CMPR_OK;
}

/* the refusals (hamming_sets.h) */
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

namespace {

/* what the four entry points share: the refusals, both sets on the device, the pairs of groups */
struct HmJob {
  HmSet          own1, own2;
  HmSet         *s1 = nullptr, *s2 = nullptr;
  Tmp<HmPair>    pairs;
  HmParams       P{};
  uint32_t       blocks = 0;
  std::vector<std::pair<uint32_t, std::pair<uint32_t, uint32_t>>> runs;   /* stride | first workgroup, workgroups */
};

int hm_setup(cmpr_context *c, const std::string &who, const cmpr_set_view *set1, const cmpr_set_view *set2,
             int64_t differences, bool on_device, HmJob &J, bool triangular = false)
{
  int rc;
  /* (hm_refusals has refused a bad view of either set before the first is staged: the look at it there changes nothing) */
  if ((rc = cmpr_stage_set(c, set1, on_device, J.own1)) || (rc = hm_prepare(c, J.own1))) return rc;
  J.s1 = &J.own1;
  if (set2 == set1) {
    J.s2 = J.s1;
  } else {
    if ((rc = cmpr_stage_set(c, set2, on_device, J.own2)) || (rc = hm_prepare(c, J.own2))) return rc;
    J.s2 = &J.own2;
  }
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
      const uint32_t nb = blocks_for(ga.count, HM_WG);
      const uint32_t form = c->hamming_generic || p.stride > HAMMING_REG_WORDS ? 0u : p.stride;
      if (!J.runs.empty() && J.runs.back().first == form)
        J.runs.back().second.second += nb;
      else
        J.runs.push_back({form, {(uint32_t)blocks, nb}});
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
  /* segments: as many as fill the machine while the query tiles alone do not, none shorter than a wave of references */
  uint32_t S = 1;
  if (c->hamming_segments) {
    S = (uint32_t)c->hamming_segments;
  } else if (blocks) {
    const uint64_t target = (uint64_t)c->cus * 8;
    S = (uint32_t)std::min<uint64_t>(HM_MAX_SEGMENTS, (target + blocks - 1) / blocks);
    S = std::max<uint32_t>(1, std::min<uint32_t>(S, (nr_max + 63) / 64));
    /* the link sink's workgroups walk what lies behind them: the first of a group all of it, the last nothing, and
       the launch ends with the first ones of the largest group.  No segment longer than HM_LINK_SEGMENT references
       keeps those as short as everybody else's */
    if (triangular)
      S = std::max(S, std::min<uint32_t>(HM_MAX_SEGMENTS, (nr_max + HM_LINK_SEGMENT - 1) / HM_LINK_SEGMENT));
  }
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
  for (const auto &run : J.runs) {
    const HmKernel fn = nt ? hm_kernel_for<SINK, true>(run.first) : hm_kernel_for<SINK, false>(run.first);
    HmParams P = J.P;
    P.blk_base = run.second.first;
    hipLaunchKernelGGL(fn, dim3(run.second.second, P.segments), dim3(HM_WG), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
  }
  return CMPR_OK;
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
  auto t0 = std::chrono::steady_clock::now();
  c->hm_ms[0] = c->hm_ms[1] = c->hm_ms[2] = 0;
  HmJob J;
  if ((rc = hm_setup(c, who, set1, set2, differences, on_device, J)))
    return rc;
  c->hm_ms[0] = ms_since(t0);
  t0 = std::chrono::steady_clock::now();

  const uint64_t rows = c->opt.existence ? J.s1->n : J.s1->R, cells = rows * J.s2->R;
  if (cells == 0)
    return CMPR_OK;
  Out<unsigned long long> matrix((unsigned long long *)matrix_out, on_device);
  if ((rc = matrix.temp(c, (size_t)cells))) return rc;
  HIP_TRY(c, hipMemsetAsync(matrix.p, 0, cells * sizeof(unsigned long long), c->stream));
  HmParams &P = J.P;
  P.rep1 = J.s1->rep.b.p; P.rep2 = J.s2->rep.b.p;
  P.cnt1 = c->opt.ignore_counts ? nullptr : J.s1->cnt.b.p;
  P.cnt2 = c->opt.ignore_counts ? nullptr : J.s2->cnt.b.p;
  P.R2 = J.s2->R;
  P.score = (uint32_t)c->opt.score;
  P.existence = c->opt.existence ? 1u : 0u;
  P.mat_lds = !c->opt.existence && cells <= HM_MAT_CELLS ? 1u : 0u;
  P.matrix = matrix.p;
  P.cells = (uint32_t)std::min<uint64_t>(cells, HM_MAT_CELLS);
  if ((rc = hm_launch<SINK_MATRIX>(c, J)))
    return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->hm_ms[1] = ms_since(t0);
  if (!on_device) {
    t0 = std::chrono::steady_clock::now();
    if ((rc = matrix.copy_out(c, (size_t)cells))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->hm_ms[2] = ms_since(t0);
  }
  return CMPR_OK;
}

int hamming_neighbors_impl(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2, int64_t differences,
                           uint64_t capacity, uint64_t *row_start_out, uint32_t *hit_out, uint16_t *dist_out,
                           uint64_t *n_edges_out, bool on_device)
{
  if (!c)
    return CMPR_EINVAL;
  const std::string who = "cmpr_hamming_neighbors";
  if (!n_edges_out)
    return fail(c, CMPR_EINVAL, who + ": n_edges_out is NULL");
  *n_edges_out = 0;
  if (capacity && !hit_out)
    return fail(c, CMPR_EINVAL, who + ": hit_out is NULL with a capacity");
  int rc;
  if ((rc = hm_refusals(c, who, set1, set2, differences, HM_NEIGHBORS, on_device)))
    return rc;
  auto t0 = std::chrono::steady_clock::now();
  c->hm_ms[0] = c->hm_ms[1] = c->hm_ms[2] = 0;
  HmJob J;
  if ((rc = hm_setup(c, who, set1, set2, differences, on_device, J)))
    return rc;
  c->hm_ms[0] = ms_since(t0);
  t0 = std::chrono::steady_clock::now();

  /* count per (query, segment); the sum; the rows */
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
  HmParams &P = J.P;
  P.cnt = cnt.b.p;
  if ((rc = hm_launch<SINK_CSR>(c, J)))
    return rc;
  hipcub::TransformInputIterator<unsigned long long, U32To64, const uint32_t *> wide(cnt.b.p, U32To64());
  size_t scan_bytes = 0;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, wide, offs.b.p, (int)slots, c->stream));
  if ((rc = dev_alloc(c, scan_tmp.b, scan_bytes))) return rc;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(scan_tmp.b.p, scan_bytes, wide, offs.b.p, (int)slots, c->stream));
  if (rows.wanted()) {
    if ((rc = rows.temp(c, (size_t)(n1 + 1)))) return rc;
    hipLaunchKernelGGL(hm_rows_kernel, dim3(blocks_for(n1 + 1, HM_WG)), dim3(HM_WG), 0, c->stream, offs.b.p, n1,
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
    P.offs = offs.b.p;
    P.hit = hit.p;
    P.dist = dist.p;
    if ((rc = hm_launch<SINK_CSR>(c, J)))
      return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  c->hm_ms[1] = ms_since(t0);
  if (!on_device) {
    t0 = std::chrono::steady_clock::now();
    if ((rc = rows.copy_out(c, (size_t)(n1 + 1)))) return rc;
    if (fill) {
      if ((rc = hit.copy_out(c, (size_t)total))) return rc;
      if ((rc = dist.copy_out(c, (size_t)total))) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->hm_ms[2] = ms_since(t0);
  }
  return CMPR_OK;
}

/* cmpr_hamming_nearest*: one walk through the nearest sink, with several segments the fold of the slots behind it, and
   the number of queries that found somebody counted over the finished ties */
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
  auto t0 = std::chrono::steady_clock::now();
  c->hm_ms[0] = c->hm_ms[1] = c->hm_ms[2] = 0;
  HmJob J;
  if ((rc = hm_setup(c, who, set1, set2, 0, on_device, J)))
    return rc;
  c->hm_ms[0] = ms_since(t0);
  t0 = std::chrono::steady_clock::now();

  const uint64_t n1 = J.s1->n, S = J.P.segments;
  if (n1 == 0)
    return CMPR_OK;
  Out<uint32_t> nearest(nearest_out, on_device);
  Out<uint16_t> dist(dist_out, on_device);
  Out<uint32_t> ties(ties_out, on_device);
  if (nearest.wanted() && (rc = nearest.temp(c, (size_t)n1))) return rc;
  if (dist.wanted() && (rc = dist.temp(c, (size_t)n1))) return rc;
  if ((ties.wanted() || n_found_out) && (rc = ties.temp(c, (size_t)n1))) return rc;
  HmParams &P = J.P;
  P.rep1 = J.s1->rep.b.p; P.rep2 = J.s2->rep.b.p;
  P.floor = (uint32_t)std::min<int64_t>(min_distance, 0x10000);        /* (no distance is above 65535) */
  P.one_set = J.s2 == J.s1 ? 1u : 0u;
  P.other_rep = other_rep ? 1u : 0u;
  Tmp<unsigned long long> key, found;
  Tmp<uint32_t> slot_ties;
  Tmp<char> sum_tmp;
  if (S == 1) {
    /* "none" everywhere first: a query whose group set 2 lacks is no lane's */
    if (nearest.p) HIP_TRY(c, hipMemsetAsync(nearest.p, 0xff, n1 * sizeof(uint32_t), c->stream));
    if (dist.p) HIP_TRY(c, hipMemsetAsync(dist.p, 0xff, n1 * sizeof(uint16_t), c->stream));
    if (ties.p) HIP_TRY(c, hipMemsetAsync(ties.p, 0, n1 * sizeof(uint32_t), c->stream));
    P.nn_nearest = nearest.p; P.nn_dist = dist.p; P.nn_ties = ties.p;
  } else {
    /* ... nor is a (query, segment) whose range is empty: the fold writes every query from its slots */
    if ((rc = dev_alloc(c, key.b, (size_t)(n1 * S)))) return rc;
    if ((rc = dev_alloc(c, slot_ties.b, (size_t)(n1 * S)))) return rc;
    HIP_TRY(c, hipMemsetAsync(key.b.p, 0xff, n1 * S * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipMemsetAsync(slot_ties.b.p, 0, n1 * S * sizeof(uint32_t), c->stream));
    P.nn_key = key.b.p; P.nn_slot_ties = slot_ties.b.p;
  }
  if ((rc = hm_launch<SINK_NEAREST>(c, J)))
    return rc;
  if (S > 1) {
    hipLaunchKernelGGL(hm_nearest_fold_kernel, dim3(blocks_for(n1, HM_WG)), dim3(HM_WG), 0, c->stream,
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
  c->hm_ms[1] = ms_since(t0);
  if (!on_device) {
    t0 = std::chrono::steady_clock::now();
    if (nearest.wanted() && (rc = nearest.copy_out(c, (size_t)n1))) return rc;
    if (dist.wanted() && (rc = dist.copy_out(c, (size_t)n1))) return rc;
    if (ties.wanted() && (rc = ties.copy_out(c, (size_t)n1))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->hm_ms[2] = ms_since(t0);
  }
  return CMPR_OK;
}

/* cmpr_hamming_cluster* and cmpr_hamming_cluster_table*: the set against itself through the link sink, then the
   flatten, size and table passes of cluster.hip.  The plain call (T == NULL) fills L's label / size, the table call
   T's four arrays from labels and sizes of nobody's. */
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
  auto t0 = std::chrono::steady_clock::now();
  c->hm_ms[0] = c->hm_ms[1] = c->hm_ms[2] = 0;
  if (table)
    c->cl_ms[0] = c->cl_ms[1] = 0;
  HmJob J;
  if ((rc = hm_setup(c, who, set, set, differences, on_device, J, true)))
    return rc;
  c->hm_ms[0] = ms_since(t0);
  t0 = std::chrono::steady_clock::now();

  /* the forest over the original sequence numbers; every unordered pair of every group linked; labels and sizes */
  const uint64_t n = J.s1->n;
  if (n) {
    if ((rc = cmpr_cluster_forest(c, n, L))) return rc;
    J.P.parent = L.parent.b.p;
    J.P.snapshot = c->hamming_link_snapshot ? 1u : 0u;
    if ((rc = hm_launch<SINK_LINK>(c, J)))
      return rc;
    if ((rc = cmpr_cluster_flatten(c, n, table || L.size.wanted(), L)))
      return rc;
  }
  if (table)
    return cmpr_cluster_table_pass(c, L, c->opt.ignore_counts ? nullptr : J.s1->cnt.b.p, *T, n_clusters_out, t0,
                                   &c->hm_ms[1]);
  if (n && !on_device) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->hm_ms[1] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    if ((rc = cmpr_cluster_results(c, L, n_clusters_out)))
      return rc;
    c->hm_ms[2] = ms_since(t0);
    return CMPR_OK;
  }
  if ((rc = cmpr_cluster_results(c, L, n_clusters_out)))
    return rc;
  c->hm_ms[1] = ms_since(t0);
  return CMPR_OK;
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
