/*
 * allpairs.h -- what the all-against-all calls of hamming.hip (cmpr_hamming_*) and edit.hip (cmpr_edit_*) share in
 * front of and around their compare kernels; the host side is defined in allpairs.hip.  Nothing is hashed: every query
 * is compared with every sequence of the groups it can match, and the two files differ in the compare kernel only.
 *
 *   group    every sequence gets the 64-bit key (length, V, J) -- the length alone with ignore_genes --; hipcub's
 *            stable radix sort of (key, sequence number) per set, so inside a group the sequences stay in increasing
 *            number; the runs of equal keys are the groups (hipcub run-length encode).  The host reads the two group
 *            tables -- as many entries as there are distinct keys, not sequences -- and matches them by key.
 *   pack     the residues of each set in group order, 32-bit words, a fixed number of words per sequence of a group:
 *            four amino acids (a byte each) or sixteen nucleotides (two bits each) per word.  The words are zeroed
 *            and the residues or-ed in: the padding of a last word is zero on both sides.  Groups of at most
 *            HAMMING_REG_WORDS words are padded to the next of the word counts the register form is compiled for.
 *   compare  the caller's kernel: a workgroup of four waves takes four 64-query tiles of one entry of its table (a
 *            pair of groups, a job) and one segment (grid y) of the references; pairs_entry_of and PairQuery find
 *            the entry and the lane's query, and a launch per run of entries of one form covers the table.
 *   sinks    PairSink: what a lane makes of a match.
 *            matrix: the score of a match is added to a per-lane sum, which goes to its cell when the lane's next
 *            match lies in another set-2 repertoire and at the end -- into a copy of the matrix in LDS when it has
 *            at most PAIRS_MAT_CELLS cells (added to the global one once per workgroup), else with 64-bit global
 *            atomics.  With `existence` the row is the lane's own.  Integer sums: the same in any order.
 *            count / fill: a lane counts the hits of its (query, segment), the counts are summed in (query,
 *            segment) order (hipcub), and the same walk writes every hit and its distance at the lane's running
 *            offset.  A caller whose walk is not in number order has the rows sorted afterwards (csr_rows.h).
 *            link: the cluster calls, the set against itself: a match unites the two sequences' trees in the forest
 *            of link_forest.h over the ORIGINAL sequence numbers.  The caller's walk visits every unordered pair once.
 *            Beside every staged reference lies a snapshot of its root; a lane keeps its own root in a register,
 *            skips a match whose snapshot equals it and looks its root up again after a link it made.  No count
 *            array, no pair list.  What follows the launch is pairs_clusters (cluster.hip's passes).
 *            nearest: the sink itself is the caller's (HmSink / EdSink<SINK_NEAREST>: the walks differ in what "the
 *            first reference at the minimum" means); what surrounds the launch is pairs_nearest: the outputs or the
 *            (query, segment) slots set to "none", the fold of the slots, the count of the queries that found somebody.
 *
 * The (query, segment) count array has n1 x S words, S <= PAIRS_MAX_SEGMENTS; the automatic S is above 1 only while
 * the query tiles alone do not fill the machine (S <= ceil(8 x CUs / workgroups)), which bounds it by
 * 256 x (8 x CUs + workgroups) words.  Nothing here writes the resident sets, plans or statistics of the context.
 */
#ifndef COMPAIRR_AMD_ALLPAIRS_H
#define COMPAIRR_AMD_ALLPAIRS_H

#include "context.h"
#include "link_forest.h"

#include <algorithm>

namespace cmpr {

constexpr uint32_t PAIRS_WG = 256;             /* four waves: four 64-query tiles of one group */
constexpr uint32_t PAIRS_STAGE_MAX = 512;      /* references staged in LDS at a time, at most */
constexpr uint32_t PAIRS_MAT_CELLS = 1024;     /* a matrix of up to this many cells is privatised in LDS (8 KiB) */
constexpr uint32_t PAIRS_MAX_SEGMENTS = 64;
constexpr uint32_t HAMMING_REG_WORDS = 16;     /* the bound between the two forms: a group of more words per sequence
                                                  (64 amino acids, 256 nucleotides) takes the generic form */
constexpr uint32_t AA_PER_WORD = 4, NT_PER_WORD = 16;
/* the calls that walk jobs (edit.hip, tcrdist.hip) */
constexpr uint32_t PAIRS_MAX_LEN = 256;        /* residues of the longest sequence: four 64-bit column words */
constexpr uint32_t PAIRS_REG_RESIDUES = 64;    /* a query of more residues is read from global memory (NW = 0) */

/* a group of one set: the sequences at positions start .. start + count - 1 of the sorted order */
struct HmGroup {
  uint64_t pk_off;                 /* first packed word of the group */
  uint32_t start, count;
  uint32_t stride, len;            /* words per sequence; residues per sequence */
};

/* a set on the device, validated, grouped and packed */
struct HmSet : StagedSet {
  Tmp<uint32_t> ord, pk;           /* sequence numbers in group order; the packed words */
  std::vector<uint64_t> keys;      /* of the groups, increasing: ((length x n_v) + V) x n_j + J, the length with ignore_genes */
  std::vector<HmGroup>  groups;
  uint64_t per_len = 1;            /* keys per length: key / per_len is the length, key % per_len the genes */
};

/* what the key of a sequence holds: HM_KEY_LENGTH (ignore_genes), HM_KEY_LENGTH_V_J: ((length x n_v) + V) x n_j + J,
   HM_KEY_LENGTH_V: length x n_v + V (cmpr_tcrdist_* with a V table: the J gene plays no part) */
enum HmKeyMode { HM_KEY_LENGTH, HM_KEY_LENGTH_V_J, HM_KEY_LENGTH_V };

/* the mode of every call whose pairs share both genes unless ignore_genes */
inline HmKeyMode hm_key_mode(const cmpr_context *c) { return c->opt.ignore_genes ? HM_KEY_LENGTH : HM_KEY_LENGTH_V_J; }

/* words per sequence of a group of `len` residues: the next word count the register form is compiled for, or the
   words themselves beyond HAMMING_REG_WORDS */
uint32_t stride_of(uint32_t len, uint32_t per_word);

/* the staged set H grouped by `mode` and packed */
int hm_prepare(cmpr_context *c, HmSet &H, HmKeyMode mode);

/* what a call makes of the pairs: the clusters and the nearest neighbours take no score, so what the reference refuses
   of scores is not theirs.  HM_NEAREST: `differences` is the call's min_distance */
enum HmKind { HM_MATRIX, HM_NEIGHBORS, HM_CLUSTERS, HM_NEAREST };

/* the refusals of the all-against-all calls, before any device work.  with_indels: the call compares by edit
   distance (cmpr_edit_*), options.indels is not looked at */
int hm_refusals(cmpr_context *c, const std::string &who, const cmpr_set_view *set1, const cmpr_set_view *set2,
                int64_t differences, HmKind kind, bool on_device, bool with_indels = false);

/* both sets of a call on the device; set2 == set1: staged once */
struct PairSets {
  HmSet  own1, own2;
  HmSet *s1 = nullptr, *s2 = nullptr;
};

/* Each set staged, handed to `check` (or none) and prepared (grouped by `mode`), set 1 first: what `check` refuses of set 1 is refused
   before set 2 is staged.  (hm_refusals has refused a bad view of either set before the first is staged: the look
   at it in cmpr_stage_set changes nothing.) */
int pairs_stage(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2, bool on_device, PairSets &W,
                HmKeyMode mode, const std::function<int(const HmSet &)> &check = nullptr);

/* pairs_stage's `check` of the calls that walk jobs: a set with a sequence of more than PAIRS_MAX_LEN residues is
   refused, in the name of `prefix` (cmpr_edit, cmpr_tcrdist) */
std::function<int(const HmSet &)> pairs_length_check(cmpr_context *c, const char *prefix);

/* the workgroups of a call in runs of one form of the compare kernel: a launch each */
struct PairRuns {
  struct Run { uint32_t form, blk0, blocks; };
  std::vector<Run> runs;
  /* `blocks` workgroups from blk0 on, behind the last ones: one run with them when the form is theirs */
  void add(uint32_t form, uint32_t blk0, uint32_t blocks)
  {
    if (!runs.empty() && runs.back().form == form)
      runs.back().blocks += blocks;
    else
      runs.push_back({form, blk0, blocks});
  }
};

/* Segments: the tunable's value when it has one; else as many as fill the machine while the `blocks` workgroups of
   query tiles alone do not, none shorter than a wave of the nr_max references of the largest group -- and, with
   longest_piece, none longer than that many references. */
uint32_t pairs_segments(const cmpr_context *c, int64_t tunable, uint64_t blocks, uint32_t nr_max,
                        uint32_t longest_piece = 0);

/* ---- jobs: a set-1 group against SEVERAL set-2 groups (edit.hip, tcrdist.hip) ---- */

/* a set-1 group and its partners; what a partner record holds is the caller's (EdPartner, TdPartner: pk_off, r0 and nr
   of the set-2 group and what the compare needs of the two lengths) */
struct PairJob {
  uint64_t pk1;                    /* first packed word of the group */
  uint32_t q0, nq;                 /* positions in set 1's sorted order */
  uint32_t len, stride;
  uint32_t p0, np;                 /* its partners in the partner array */
  uint32_t blk0, pad;              /* first workgroup (grid x) of the job */
};

/* the register form of a query of `len` residues in `stride` packed words: 2, 4, 8, 16, or 0 */
uint32_t pairs_form_of(uint32_t len, uint32_t stride);

/* the lengths a set has, increasing, and the first group of each (the keys increase with the length) */
struct PairLengths {
  std::vector<uint32_t> len;
  std::vector<size_t>   first;
  explicit PairLengths(const HmSet &S);
};

/* the group of S with this key, or NULL: a binary search */
const HmGroup *hm_group_of(const HmSet &S, uint64_t key);

/* both sets of a call and its job table on the device */
template <typename Partner>
struct PairJobs : PairSets {
  Tmp<PairJob>   jobs;
  Tmp<Partner>   partners;
  PairRuns       runs;             /* form: pairs_form_of */
  uint64_t       blocks = 0;       /* workgroups of query tiles */
  uint32_t       nr_max = 0;       /* sequences of the largest partner: both for the caller's pairs_segments */
};

/* The job table of the two prepared sets of J.  partners_of(ga, genes, L2, partners) appends the partners of the set-1
   group ga, whose key holds `genes` behind the length, to `partners` -- L2: the lengths of set 2 -- and may reorder
   what it appended; a group it appends nothing for gets no job.  The jobs in set 1's group order, their workgroups in
   runs of one query form, the two tables uploaded, and the fields of the parameters every such kernel has: jobs,
   partners, njobs, pk1, pk2, ord1, ord2. */
template <typename Partner, typename Params, typename PartnersOf>
int pairs_jobs(cmpr_context *c, const std::string &who, PairJobs<Partner> &J, Params &P, PartnersOf partners_of)
{
  int rc;
  const HmSet &A = *J.s1, &B = *J.s2;
  const PairLengths L2(B);
  std::vector<PairJob> jobs;
  std::vector<Partner> partners;
  for (size_t a = 0; a < A.groups.size(); a++) {
    const HmGroup &ga = A.groups[a];
    const size_t p0 = partners.size();
    partners_of(ga, A.keys[a] % A.per_len, L2, partners);
    if (partners.size() == p0)
      continue;
    if (partners.size() > 0xffffffffull)
      return fail(c, CMPR_EUNSUPPORTED, who + ": more than 2^32-1 pairs of groups");
    for (size_t p = p0; p < partners.size(); p++)
      J.nr_max = std::max(J.nr_max, partners[p].nr);
    const uint32_t nb = blocks_for(ga.count, PAIRS_WG);
    J.runs.add(pairs_form_of(ga.len, ga.stride), (uint32_t)J.blocks, nb);
    jobs.push_back(PairJob{ga.pk_off, ga.start, ga.count, ga.len, ga.stride, (uint32_t)p0,
                           (uint32_t)(partners.size() - p0), (uint32_t)J.blocks, 0u});
    J.blocks += nb;
    if (J.blocks > 0xffffffu)
      return fail(c, CMPR_EUNSUPPORTED, who + ": more than 2^24 workgroups of queries");
  }
  if (!jobs.empty()) {
    if ((rc = dev_upload(c, J.jobs.b, jobs.data(), jobs.size()))) return rc;
    if ((rc = dev_upload(c, J.partners.b, partners.data(), partners.size()))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));           /* (the two vectors leave scope) */
  }
  P.jobs = J.jobs.b.p;
  P.partners = J.partners.b.p;
  P.njobs = (uint32_t)jobs.size();
  P.pk1 = A.pk.b.p; P.pk2 = B.pk.b.p;
  P.ord1 = A.ord.b.p; P.ord2 = B.ord.b.p;
  return CMPR_OK;
}

/* ---- what the entry points do around their setup ---- */

/* `setup` between the caller's timers zeroed -- and the cluster table's, for the table calls -- and ms[0], the time it
   took */
template <size_t N, typename Setup>
int pairs_timed_setup(cmpr_context *c, double (&ms)[N], bool table, Setup setup)
{
  const auto t0 = std::chrono::steady_clock::now();
  for (double &t : ms)
    t = 0;
  if (table)
    c->cl_ms[0] = c->cl_ms[1] = 0;
  const int rc = setup();
  if (!rc)
    ms[0] = ms_since(t0);
  return rc;
}

/* the argument checks of the *_neighbors calls, in front of their refusals; the edge count is zeroed */
int pairs_neighbors_args(cmpr_context *c, const std::string &who, uint64_t capacity, const uint32_t *hit_out,
                         uint64_t *n_edges_out);

/* the sink fields of a compare kernel's parameters */
struct PairSinks {
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

/* ... and of the link sink, beside them */
struct PairLinks {
  uint32_t       *parent;          /* the forest, over original sequence numbers (link_forest.h) */
  uint32_t        snapshot;        /* 1: matches whose two root snapshots are equal are skipped */
};

/* The compare kernel, Params::sink filled for the matrix, over the runs (`launch`), and the matrix to the caller.
   ms: the caller's timers, [1] the compare, [copy_slot] the copy-out of the host variant. */
int pairs_matrix(cmpr_context *c, const PairSets &W, PairSinks &K, void *matrix_out, bool on_device,
                 const std::function<int()> &launch, double *ms, int copy_slot);

/* Count, 64-bit sum, rows, and -- when `capacity` holds the edges -- fill: `launch` runs once or twice.  The two ways
   the callers differ:
     rows_always   row_start is worked out whether the caller asked for it or not (the row order reads it)
     order_slot    >= 0: the walk does not leave the rows in order; they are sorted behind the fill (csr_rows.h), timed
                   into ms[order_slot].  < 0: no such step
   ms[1]: count to fill; ms[copy_slot]: the copy-out of the host variant. */
int pairs_neighbors(cmpr_context *c, const std::string &who, const PairSets &W, uint32_t segments, PairSinks &K,
                    uint64_t capacity, uint64_t *row_start_out, uint32_t *hit_out, uint16_t *dist_out,
                    uint64_t *n_edges_out, bool on_device, const std::function<int()> &launch, bool rows_always,
                    double *ms, int order_slot, int copy_slot);

/* where a lane of a nearest sink (the callers' own, HmSink / EdSink<SINK_NEAREST>) leaves its results: filled by
   pairs_nearest and handed to its `launch` */
struct PairNearest {
  uint32_t       *nearest;         /* one segment: the three results, each may be NULL */
  uint16_t       *dist;
  uint32_t       *ties;
  unsigned long long *key;         /* several: [n1 x segments] (distance << 32 | number), all ones: none */
  uint32_t       *slot_ties;       /* ... and the references of the segment at that distance */
};

/* The nearest neighbour of every sequence of set 1: the three outputs (one segment) or the (query, segment) slots
   (several) set to "none" on the stream, `launch` -- the compare kernel with the caller's nearest sink over the runs,
   which writes where the PairNearest says --, with several segments the fold of a query's slots (the smallest key, the
   ties of the slots at its distance summed), and the number of queries that found somebody counted over the finished
   ties.  ms[1]: all of that; ms[copy_slot]: the copy-out of the host variant. */
int pairs_nearest(cmpr_context *c, const PairSets &W, uint32_t segments, uint32_t *nearest_out, uint16_t *dist_out,
                  uint32_t *ties_out, uint64_t *n_found_out, bool on_device,
                  const std::function<int(const PairNearest &)> &launch, double *ms, int copy_slot);

/* The clusters of set S against itself: the forest over the original sequence numbers (cluster.hip), `launch` -- the
   compare kernel with the link sink over the runs, every unordered matching pair united --, flat labels and sizes, and
   the results of the plain call (T == NULL: L's label / size) or the table pass (T's four arrays, from labels and sizes
   of nobody's).  ms[1]: the links, the flatten and the sizes; ms[copy_slot]: the copy-out of the host variant of the
   plain call; the table pass times itself (cl_ms[1]). */
int pairs_clusters(cmpr_context *c, const HmSet &S, bool snapshot, bool on_device, ClusterLinks &L, ClusterTableOut *T,
                   uint64_t *n_clusters_out, const std::function<int(const PairLinks &)> &launch, double *ms,
                   int copy_slot);

/* kernel_for(form) over every run: Params has blk_base and segments */
template <typename Params, typename KernelFor>
int pairs_launch(cmpr_context *c, const PairRuns &R, const Params &P0, KernelFor kernel_for)
{
  for (const PairRuns::Run &run : R.runs) {
    Params P = P0;
    P.blk_base = run.blk0;
    hipLaunchKernelGGL(kernel_for(run.form), dim3(run.blocks, P.segments), dim3(PAIRS_WG), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
  }
  return CMPR_OK;
}

/* ---- device ---- */

__device__ __forceinline__ unsigned long long pair_score(uint32_t score, unsigned long long f, unsigned long long g)
{
  switch (score) {
  case CMPR_SCORE_MIN: case CMPR_SCORE_JACCARD: return f < g ? f : g;
  case CMPR_SCORE_MAX:                          return f > g ? f : g;
  case CMPR_SCORE_MEAN:                         return f + g;             /* 2 x mean */
  default:                                      return f * g;             /* product, MH */
  }
}

/* the entry of workgroup `blk` in a table in increasing blk0: the last one whose first workgroup is not behind it */
template <typename T>
__device__ __forceinline__ T pairs_entry_of(const T *tab, uint32_t n, uint32_t blk)
{
  uint32_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (tab[mid].blk0 <= blk)
      lo = mid;
    else
      hi = mid - 1;
  }
  return tab[lo];
}

/* the lane's query: its place in the entry's set-1 group (a lane beyond the group's nq queries is idle and reads the
   group's first one), in set 1's sorted order, and its sequence number */
struct PairQuery {
  uint32_t qi, nq, qpos, qorig;
  template <typename T>
  __device__ __forceinline__ PairQuery(const T &t, uint32_t blk, const uint32_t *ord1)
      : qi((blk - t.blk0) * PAIRS_WG + threadIdx.x), nq(t.nq), qpos(t.q0 + (qi < nq ? qi : 0u)), qorig(ord1[qpos]) {}
  __device__ __forceinline__ bool active() const { return qi < nq; }
};

/* the lane's query in packed words: `w` its first one, `stride` of them; q[] the first NW in registers (zero beyond the
   stride), indexed at compile time only.  NW = 0: no registers, the words are read through w */
template <int NW>
struct PairWords {
  const uint32_t *const w;
  uint32_t q[NW ? NW : 1];
  template <typename T>
  __device__ __forceinline__ PairWords(const uint32_t *pk1, const T &t, const PairQuery &Q, uint32_t stride)
      : w(pk1 + t.pk1 + (uint64_t)(Q.qpos - t.q0) * stride)
  {
    if (NW) {
#pragma unroll
      for (int k = 0; k < NW; k++)
        q[k] = (uint32_t)k < stride ? w[k] : 0u;
    }
  }
};

/* segment `seg` of `segments`, [e0, e1), of the references behind w0 of a group of nr */
__device__ __forceinline__ void pairs_segment(uint32_t nr, uint32_t w0, uint32_t seg, uint32_t segments, uint32_t &e0,
                                              uint32_t &e1)
{
  e0 = w0 + (uint32_t)((uint64_t)(nr - w0) * seg / segments);
  e1 = w0 + (uint32_t)((uint64_t)(nr - w0) * (seg + 1) / segments);
}

/* references of a staged piece: as many as fit the kernel's buffer, the id arrays and the stage_refs tunable (0: none,
   it wraps to the largest number) */
__device__ __forceinline__ uint32_t pairs_piece(uint32_t fit, uint32_t stage_refs)
{
  const uint32_t R = fit > PAIRS_STAGE_MAX ? PAIRS_STAGE_MAX : fit;
  return stage_refs - 1u < R - 1u ? stage_refs : R;
}

/* (SINK_NEAREST: PairSink has no such form; hamming.hip and edit.hip each have a sink of their own behind its interface) */
enum { SINK_CSR = 0, SINK_MATRIX = 1, SINK_LINK = 2, SINK_NEAREST = 3 };

constexpr uint32_t HM_NONE = 0xffffffffu;      /* nearest sinks: the infinite distance, and "no sequence" */

/* the end of a nearest sink: the lane's smallest distance `best` (HM_NONE: nobody), the sequence `number` of the first
   reference at it and the references at it, to the three results (one segment) or the slot of (query, segment).  What
   the walk left in number and ties while nobody was found is dropped */
__device__ __forceinline__ void pairs_nearest_end(const PairNearest &N, uint32_t segments, uint32_t qorig, uint32_t seg,
                                                  uint32_t best, uint32_t number, uint32_t ties)
{
  const bool none = best == HM_NONE;
  const uint32_t id = none ? HM_NONE : number;
  const uint32_t t = none ? 0u : ties;
  if (segments == 1) {
    if (N.nearest)
      N.nearest[qorig] = id;
    if (N.dist)
      N.dist[qorig] = none ? (uint16_t)0xffffu : (uint16_t)best;
    if (N.ties)
      N.ties[qorig] = t;
  } else {
    const uint64_t slot = (uint64_t)qorig * segments + seg;
    N.key[slot] = (unsigned long long)best << 32 | id;
    N.slot_ties[slot] = t;
  }
}

/* a pointer into LDS, typed as such: what is reached through it stays an LDS instruction, also where the code chooses
   between it and a pointer to global memory (the cells of the matrix sink) */
template <typename T>
using Lds = __attribute__((address_space(3))) T *;

/* the kernel's __shared__ arrays a sink stages into: PAIRS_STAGE_MAX ids; repertoires and counts likewise and
   PAIRS_MAT_CELLS cells with SINK_MATRIX, one word each otherwise */
struct PairLds {
  Lds<uint32_t> id, rep;
  Lds<unsigned long long> cnt, mat;
  __device__ __forceinline__ PairLds(uint32_t *id_, uint32_t *rep_, unsigned long long *cnt_, unsigned long long *mat_)
      : id((Lds<uint32_t>)id_), rep((Lds<uint32_t>)rep_), cnt((Lds<unsigned long long>)cnt_),
        mat((Lds<unsigned long long>)mat_) {}
};

/* What a lane keeps of its matches and does with them.  The kernel calls, in this order: zero_matrix() (a barrier
   follows before the first match), init() with the lane's query and the workgroup's segment, per staged piece stage()
   for every reference of it and behind a barrier match() for every match, and at last end(). */
template <int SINK>
struct PairSink {
  const PairSinks  K;              /* (a copy, not a reference: a pointer to the kernel's parameters held in a struct
                                      delays their promotion, and each field is then loaded where it is used) */
  const uint32_t   segments;
  const PairLds    L;
  /* CSR */
  uint32_t hits = 0;
  unsigned long long pos = 0;
  /* matrix */
  unsigned long long acc = 0, row = 0, f = 1;
  uint32_t cur_rep = 0;

  __device__ __forceinline__ PairSink(const PairSinks &K_, uint32_t segments_, const PairLds &L_)
      : K(K_), segments(segments_), L(L_) {}
  __device__ __forceinline__ bool mat_lds() const { return SINK == SINK_MATRIX && K.mat_lds; }

  __device__ __forceinline__ void zero_matrix() const
  {
    if (mat_lds()) {
      for (uint32_t k = threadIdx.x; k < K.cells; k += PAIRS_WG)
        L.mat[k] = 0;
    }
  }
  __device__ __forceinline__ void init(uint32_t qorig, uint32_t seg)
  {
    if (SINK == SINK_CSR) {
      if (K.offs)
        pos = K.offs[(uint64_t)qorig * segments + seg];
    } else {
      row = K.existence ? (unsigned long long)qorig : (unsigned long long)K.rep1[qorig];
      f = K.cnt1 ? K.cnt1[qorig] : 1ull;
    }
  }
  __device__ __forceinline__ bool stages() const { return true; }
  /* sequence number, repertoire and count of the reference staged as r */
  __device__ __forceinline__ void stage(uint32_t r, uint32_t id) const
  {
    L.id[r] = id;
    if (SINK == SINK_MATRIX) {
      L.rep[r] = K.rep2[id];
      L.cnt[r] = K.cnt2 ? K.cnt2[id] : 1ull;
    }
  }
  __device__ __forceinline__ void flush()
  {
    if (SINK == SINK_MATRIX && acc) {
      const uint64_t cell = row * K.R2 + cur_rep;
      if (mat_lds())                                   /* (atomicAdd, on a pointer that is no generic one) */
        __hip_atomic_fetch_add(&L.mat[cell], acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else
        atomicAdd(K.matrix + cell, acc);
      acc = 0;
    }
  }
  /* reference r of the staged piece matched at distance `dd` */
  __device__ __forceinline__ void match(uint32_t r, uint32_t dd)
  {
    if (SINK == SINK_CSR) {
      if (K.offs) {
        K.hit[pos] = L.id[r];
        if (K.dist)
          K.dist[pos] = (uint16_t)dd;
        pos++;
      } else {
        hits++;
      }
    } else {
      /* the lane's sum belongs to one set-2 repertoire: a match in another one sends it to its cell first (a
         reference that does not match costs the matrix sink nothing) */
      const uint32_t rp = L.rep[r];
      if (rp != cur_rep) {
        flush();
        cur_rep = rp;
      }
      acc += K.cnt1 ? pair_score(K.score, f, L.cnt[r]) : 1ull;
    }
  }
  __device__ __forceinline__ void end(bool active, uint32_t qorig, uint32_t seg)
  {
    if (SINK == SINK_CSR) {
      if (!K.offs && active)
        K.cnt[(uint64_t)qorig * segments + seg] = hits;
    } else {
      flush();
      if (mat_lds()) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < K.cells; k += PAIRS_WG)
          if (L.mat[k])
            atomicAdd(K.matrix + k, L.mat[k]);
      }
    }
  }
};

/* link: st_root holds a snapshot of every staged reference's root, `root` the lane's own when it last looked.  The
   kernel's st_root array has PAIRS_STAGE_MAX words with SINK_LINK (one otherwise) */
template <>
struct PairSink<SINK_LINK> {
  const PairLinks K;               /* (a copy, as the other sinks' K) */
  const Lds<uint32_t> st_id, st_root;
  uint32_t qorig = 0, root = 0;
  __device__ __forceinline__ PairSink(const PairLinks &K_, const PairLds &L, uint32_t *st_root_)
      : K(K_), st_id(L.id), st_root((Lds<uint32_t>)st_root_) {}
  __device__ __forceinline__ void zero_matrix() const {}
  __device__ __forceinline__ void init(uint32_t qorig_, uint32_t)
  {
    qorig = qorig_;
    if (K.snapshot)
      root = link_root(K.parent, qorig);
  }
  __device__ __forceinline__ bool stages() const { return true; }
  __device__ __forceinline__ void stage(uint32_t r, uint32_t id) const
  {
    st_id[r] = id;
    if (K.snapshot)
      st_root[r] = link_root(K.parent, id);
  }
  /* (cluster.cc:165-211 lists the pair, :276-410 walks the lists: here the two trees become one.)  In a dense
     group almost every match joins two sequences that share a root already: equal snapshots prove it --
     trees only merge, whatever was once under a root stays in its component -- and cost no walk; unequal
     ones, stale or not, fall through to link_pair, after which the lane looks its root up again. */
  __device__ __forceinline__ void match(uint32_t r, uint32_t)
  {
    if (!K.snapshot || st_root[r] != root) {
      link_pair(K.parent, qorig, st_id[r]);
      if (K.snapshot)
        root = link_root(K.parent, qorig);
    }
  }
  __device__ __forceinline__ void end(bool, uint32_t, uint32_t) const {}
};

}  // namespace cmpr

#endif
