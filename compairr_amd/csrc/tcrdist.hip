/*
 * tcrdist.hip -- the all-against-all path under the WEIGHTED CDR3 distance of the TCR field (the metric behind tcrdist3
 * and scirpy's "tcrdist"): cmpr_tcrdist_neighbors / _device and cmpr_tcrdist_matrix / _device.  A pair (i of set 1, j of
 * set 2) has the distance D defined in include/compairr_hip.h -- a substitution-table-weighted mismatch sum over the
 * aligned positions, the ends trimmed, ONE gap block charged per residue of length difference, optionally a V-gene
 * term on top -- and matches when D <= cutoff and the genes admit it.  Nothing is hashed or enumerated.
 *
 *   group    allpairs.h's: each set sorted by (length, V, J) -- the length alone with ignore_genes, (length, V) with a
 *            V table: any two V genes pair at the table's price and the J gene plays no part --, its residues packed a
 *            byte each in group order.  Sequences of more than PAIRS_MAX_LEN = 256 residues are refused, as for edit.
 *   jobs     allpairs.h's frame, the one edit.hip walks (PairJob, pairs_jobs; in the kernel PairWords, pairs_segment,
 *            pairs_piece); this file's own is the partner rule: a set-1 group's PARTNERS are the set-2 groups whose
 *            base = |L - L'| x gap_penalty + V[v1][v2] (64 bits; the V term 0 without a table) is at most the cutoff:
 *            with a positive penalty that bounds the lengths, with 0 every length is a partner; with a table a partner
 *            can be any V at an admitted length.  Everything the alignment of a (job, partner) needs is uniform and
 *            worked out here once: base, which side is shorter and by how much, the positions k of the SHORTER
 *            sequence that pay W at the same position of the longer one (`diag`: [d0, d1)) and at position k + delta
 *            (`shift`: [s0, s1)), and the zone [lo, hi) of the gap positions SLIDING tries.  The kernel never touches
 *            genes.
 *   compare  td_compare_kernel: a workgroup of four waves takes four 64-query tiles
 *            of one job and one segment (grid y) of EVERY partner, one partner after the other; the references are
 *            staged as they are packed, TD_STAGE_WORDS words at a time.  W lies in LDS TRANSPOSED, a row of TD_WT_ROW =
 *            32 bytes per REFERENCE residue: every lane of a wave meets the same reference residue at the same step
 *            (one address: a broadcast), and the lanes' cost reads then fall into the 20 bytes of one row -- five
 *            consecutive dwords, five distinct banks, equal dwords broadcast: no bank conflict, whatever the queries
 *            hold.  The operand order never swaps: the cost is W[set-1 residue][set-2 residue] = Wt[reference][query],
 *            whichever of the two is shorter; only the positions that meet change.
 *            The query's packed words sit in registers (NW = 2, 4, 8, 16 words, the residues peeled by loops unrolled
 *            at compile time) while it has at most PAIRS_REG_RESIDUES = 64 residues.  The loop runs over the positions
 *            k of the shorter sequence; a query that is the LONGER one meets the reference's position k with its own
 *            positions k and k + delta, so per partner a second copy of its words is shifted down by delta residues --
 *            a logarithmic shifter over the words, each stage under a uniform condition, then a funnel shift of the
 *            bytes: compile-time register numbers only.  Which positions pay what is three uniform 64-bit masks per
 *            partner.  A longer query is read byte by byte from global memory (NW = 0).  No instantiation indexes a
 *            private array at run time: private_segment_fixed_size is 0 in every one (profiles/r25/tcrdist.txt).
 *            FIXED gap and equal lengths: one lookup and an add per position.  SLIDING: with d'(k), s'(k) the diag and
 *            shift costs where k pays them, cost(g) = sum_{k<lo} d' + sum_{k>=hi} s' + sum_{lo<=k<hi} s'
 *            + sum_{lo<=k<g} (d' - s'): one pass in increasing k that keeps the sum of the first three, the running
 *            last one and its minimum over g = lo .. hi (0 at g = lo) -- two lookups per position of the zone, one
 *            elsewhere, no array.  A match is base + sum <= cutoff in 32 bits (256 x 255 + 65535 fits).
 *   sinks    allpairs.h's matrix and count / fill, unchanged.  The walk goes partner by partner, which is not number
 *            order, so the rows are sorted afterwards by csr_rows.h with the key (hit << 16 | distance).
 *
 * Nothing here writes the resident sets, plans or statistics of the context.
 */
#include "allpairs.h"

#include <algorithm>
#include <string>
#include <vector>

using namespace cmpr;

namespace {

constexpr uint32_t TD_STAGE_WORDS = 4096;      /* packed words of references staged at a time (16 KiB) */
constexpr uint32_t TD_ALPHABET = 20;
constexpr uint32_t TD_WT_ROW = 32;             /* bytes of a row of the transposed table: 20 costs and the padding */
constexpr uint32_t TD_WT_WORDS = TD_ALPHABET * TD_WT_ROW / 4;

/* a set-2 group a job is compared with, and the alignment of the two lengths */
struct TdPartner {
  uint64_t pk_off;                 /* first packed word of the group */
  uint32_t r0, nr;                 /* positions in set 2's sorted order */
  uint32_t stride;                 /* packed words per sequence (at most 64) */
  uint32_t base;                   /* |L - L'| x gap_penalty + V[v1][v2]: at most the cutoff */
  uint32_t qshift, rshift;         /* delta on the side that is longer, 0 on the other: position k of the shorter
                                      sequence meets k + delta of the query (qshift) or of the reference (rshift) */
  uint32_t d0, d1;                 /* positions k of the shorter sequence that pay W against position k of the longer */
  uint32_t s0, s1;                 /* ... and against position k + delta */
  uint32_t lo, hi;                 /* SLIDING: the gap positions lo .. hi are tried; lo == hi: one position */
  uint32_t pad[2];
};

struct TdParams {
  const PairJob   *jobs;           /* a set-1 group and its partners (allpairs.h) */
  const TdPartner *partners;
  uint32_t        njobs, segments;
  const uint32_t *pk1, *pk2;       /* packed words */
  const uint32_t *ord1, *ord2;     /* sequence numbers in group order */
  const uint32_t *wt;              /* TD_WT_WORDS words: Wt[set-2 residue][set-1 residue], rows of TD_WT_ROW bytes */
  uint32_t        cutoff, stage_refs;
  uint32_t        blk_base;        /* workgroup number of this launch's first workgroup */
  PairSinks       sink;            /* count / fill, matrix (allpairs.h) */
};

/* bits a .. b - 1 of 64, 0 <= a, b <= 64 (empty when b <= a) */
__device__ __forceinline__ unsigned long long td_mask(uint32_t a, uint32_t b)
{
  const unsigned long long below_b = b >= 64 ? ~0ull : (1ull << b) - 1;
  const unsigned long long below_a = a >= 64 ? ~0ull : (1ull << a) - 1;
  return below_b & ~below_a;
}

/* NW: words of the query held in registers, 0: the query is read from global memory */
template <int NW, int SINK>
__global__ void __launch_bounds__(PAIRS_WG)
td_compare_kernel(const TdParams P)
{
  __shared__ uint32_t st_ref[TD_STAGE_WORDS];
  __shared__ uint32_t st_wt[TD_WT_WORDS];
  __shared__ uint32_t st_id[PAIRS_STAGE_MAX];
  __shared__ uint32_t st_rep[SINK == SINK_MATRIX ? PAIRS_STAGE_MAX : 1];
  __shared__ unsigned long long st_cnt[SINK == SINK_MATRIX ? PAIRS_STAGE_MAX : 1];
  __shared__ unsigned long long st_mat[SINK == SINK_MATRIX ? PAIRS_MAT_CELLS : 1];

  const uint32_t blk = P.blk_base + blockIdx.x;
  const PairJob jb = pairs_entry_of(P.jobs, P.njobs, blk);
  const PairQuery Q(jb, blk, P.ord1);
  const uint32_t qorig = Q.qorig;
  const bool active = Q.active();
  const uint32_t seg = blockIdx.y;

  PairSink<SINK> S(P.sink, P.segments, PairLds(st_id, st_rep, st_cnt, st_mat));
  S.zero_matrix();                                                      /* (a barrier follows before the first match) */
  for (uint32_t k = threadIdx.x; k < TD_WT_WORDS; k += PAIRS_WG)        /* (... and before the first lookup) */
    st_wt[k] = P.wt[k];
  const Lds<uint8_t> wt = (Lds<uint8_t>)st_wt;
  const Lds<uint32_t> refs = (Lds<uint32_t>)st_ref;

  const PairWords<NW> QW(P.pk1, jb, Q, jb.stride);
  const uint32_t *const qw = QW.w;
  const uint32_t (&q)[NW ? NW : 1] = QW.q;

  S.init(qorig, seg);

  for (uint32_t p = jb.p0; p < jb.p0 + jb.np; p++) {
    const TdPartner pt = P.partners[p];
    uint32_t e0, e1;
    pairs_segment(pt.nr, 0u, seg, P.segments, e0, e1);
    if (e0 >= e1)
      continue;                                                         /* (the whole workgroup) */
    const uint32_t stride = pt.stride;
    const uint32_t kend = max(pt.d1, pt.s1);                            /* no position from here on pays anything */

    /* the query's words shifted down by qshift residues: position k of qs is position k + qshift of q.  Word by word
       through a logarithmic shifter (qshift < 4 NW: the query is the longer sequence), then the bytes */
    uint32_t qs[NW ? NW : 1];
    if (NW) {
#pragma unroll
      for (int k = 0; k < NW; k++)
        qs[k] = q[k];
      const uint32_t ws = pt.qshift >> 2, bs = (pt.qshift & 3u) * 8u;
#pragma unroll
      for (int b = 1; b < NW; b <<= 1)
        if (ws & (uint32_t)b) {
#pragma unroll
          for (int k = 0; k < NW; k++)
            qs[k] = k + b < NW ? qs[k + b] : 0u;
        }
      if (bs) {
#pragma unroll
        for (int k = 0; k < NW; k++)
          qs[k] = qs[k] >> bs | (k + 1 < NW ? qs[k + 1] : 0u) << (32u - bs);
      }
    }
    const unsigned long long mD = td_mask(pt.d0, pt.d1), mS = td_mask(pt.s0, pt.s1), mZ = td_mask(pt.lo, pt.hi);

    const uint32_t R = pairs_piece(TD_STAGE_WORDS / stride, P.stage_refs);
    for (uint32_t e = e0; e < e1; e += R) {
      const uint32_t cnt = e1 - e < R ? e1 - e : R;
      __syncthreads();                                                  /* the previous piece has been read */
      const uint32_t *const src = P.pk2 + pt.pk_off + (uint64_t)e * stride;
      for (uint32_t it = threadIdx.x; it < cnt * stride; it += PAIRS_WG)
        st_ref[it] = src[it];
      for (uint32_t r = threadIdx.x; r < cnt; r += PAIRS_WG)
        S.stage(r, P.ord2[pt.r0 + e + r]);
      __syncthreads();
      for (uint32_t r = 0; r < cnt; r++) {
        const Lds<uint32_t> rw = refs + r * stride;
        const Lds<uint8_t> rb = (Lds<uint8_t>)rw;
        /* sum: what every gap position pays; run: sum_{lo <= k < g} (diag - shift), low: its minimum over g */
        int sum = 0, run = 0, low = 0;
        if (NW) {
#pragma unroll
          for (int w = 0; w < NW; w++)
            if ((uint32_t)w * 4 < kend) {
              const uint32_t word = (uint32_t)__builtin_amdgcn_readfirstlane((int)rw[w]);
#pragma unroll
              for (int t = 0; t < 4; t++) {
                const int k = w * 4 + t;
                int dv = 0, sv = 0;
                if (mD >> k & 1)
                  dv = wt[((word >> (t * 8)) & 0xffu) * TD_WT_ROW + ((q[w] >> (t * 8)) & 0xffu)];
                if (mS >> k & 1)
                  sv = wt[(uint32_t)rb[k + pt.rshift] * TD_WT_ROW + ((qs[w] >> (t * 8)) & 0xffu)];
                if (mZ >> k & 1) {
                  sum += sv;
                  run += dv - sv;
                  low = min(low, run);
                } else {
                  sum += dv + sv;
                }
              }
            }
        } else {
          const uint8_t *const qb = (const uint8_t *)qw;
          for (uint32_t k = min(pt.d0, pt.s0); k < kend; k++) {
            int dv = 0, sv = 0;
            if (k >= pt.d0 && k < pt.d1)
              dv = wt[(uint32_t)rb[k] * TD_WT_ROW + qb[k]];
            if (k >= pt.s0 && k < pt.s1)
              sv = wt[(uint32_t)rb[k + pt.rshift] * TD_WT_ROW + qb[k + pt.qshift]];
            if (k >= pt.lo && k < pt.hi) {
              sum += sv;
              run += dv - sv;
              low = min(low, run);
            } else {
              sum += dv + sv;
            }
          }
        }
        const uint32_t dd = pt.base + (uint32_t)(sum + low);
        if (dd <= P.cutoff && active)
          S.match(r, dd);
      }
    }
  }
  S.end(active, qorig, seg);
}

typedef void (*TdKernel)(const TdParams);

template <int SINK>
TdKernel td_kernel_for(uint32_t nw)
{
  switch (nw) {
  case 2:  return td_compare_kernel<2, SINK>;
  case 4:  return td_compare_kernel<4, SINK>;
  case 8:  return td_compare_kernel<8, SINK>;
  case 16: return td_compare_kernel<16, SINK>;
  default: return td_compare_kernel<0, SINK>;
  }
}

/* what the entry points share: both sets on the device, the jobs (allpairs.h), the table */
struct TdWork : PairJobs<TdPartner> {
  Tmp<uint32_t>  wt;
  TdParams       P{};
};

/* the alignment of a query of L residues with references of L2: the fields of the partner record behind `base` */
void td_align(const cmpr_tcrdist_params &T, uint32_t L, uint32_t L2, TdPartner &pt)
{
  const uint32_t Ls = std::min(L, L2), delta = std::max(L, L2) - Ls;
  const uint32_t nt = (uint32_t)std::min<uint64_t>(T.ntrim, Ls);                  /* first position behind the trim */
  const uint32_t ce = T.ctrim >= Ls ? 0u : Ls - T.ctrim;                          /* first position of the C trim */
  pt.qshift = L > L2 ? delta : 0u;
  pt.rshift = L < L2 ? delta : 0u;
  if (delta == 0) {
    pt.d0 = nt; pt.d1 = std::max(nt, ce);
    pt.s0 = pt.s1 = pt.lo = pt.hi = 0;
    return;
  }
  int lo, hi;
  if (T.gap_mode == CMPR_GAP_FIXED) {
    lo = hi = std::min(6, 3 + (((int)Ls - 5) >> 1));                              /* (the shift floors) */
  } else {
    for (lo = 5, hi = (int)Ls - 5; lo > hi; lo--, hi++) {}
  }
  pt.lo = (uint32_t)lo; pt.hi = (uint32_t)hi;
  pt.d0 = nt; pt.d1 = std::max(nt, pt.hi);
  pt.s0 = pt.lo; pt.s1 = std::max(pt.lo, ce);
}

int td_setup(cmpr_context *c, const std::string &who, const cmpr_set_view *set1, const cmpr_set_view *set2,
             const cmpr_tcrdist_params &T, int64_t cutoff, bool on_device, TdWork &J)
{
  const bool table = T.v_distance != nullptr;
  int rc;
  if ((rc = pairs_stage(c, set1, set2, on_device, J, table ? HM_KEY_LENGTH_V : hm_key_mode(c),
                        pairs_length_check(c, "cmpr_tcrdist"))))
    return rc;
  const HmSet &B = *J.s2;
  TdParams &P = J.P;

  /* per set-1 group the set-2 groups whose base is within the cutoff: of its V and J by binary search of their key,
     or with a table every V */
  const uint64_t per = B.per_len, n_v = std::max<uint32_t>(1, c->opt.n_v_genes);
  if ((rc = pairs_jobs(c, who, J, P, [&](const HmGroup &ga, uint64_t genes_of, const PairLengths &L2,
                                         std::vector<TdPartner> &partners) {
         for (size_t x = 0; x < L2.len.size(); x++) {
           const uint32_t len2 = L2.len[x];
           const uint64_t gap = (uint64_t)(ga.len > len2 ? ga.len - len2 : len2 - ga.len) * T.gap_penalty;
           if (gap > (uint64_t)cutoff)
             continue;
           TdPartner pt{};
           td_align(T, ga.len, len2, pt);
           const auto add = [&](const HmGroup &gb, uint64_t base) {
             pt.pk_off = gb.pk_off; pt.r0 = gb.start; pt.nr = gb.count; pt.stride = gb.stride;
             pt.base = (uint32_t)base;
             partners.push_back(pt);
           };
           if (table) {
             for (size_t b = L2.first[x]; b < B.groups.size() && B.groups[b].len == len2; b++) {
               const uint64_t base = gap + T.v_distance[genes_of * n_v + B.keys[b] % per];
               if (base <= (uint64_t)cutoff)
                 add(B.groups[b], base);
             }
           } else if (const HmGroup *gb = hm_group_of(B, (uint64_t)len2 * per + genes_of)) {
             add(*gb, gap);
           }
         }
       })))
    return rc;

  /* W transposed: a row per set-2 residue */
  std::vector<uint32_t> wt(TD_WT_WORDS, 0u);
  uint8_t *const wb = (uint8_t *)wt.data();
  for (uint32_t a1 = 0; a1 < TD_ALPHABET; a1++)
    for (uint32_t a2 = 0; a2 < TD_ALPHABET; a2++)
      wb[a2 * TD_WT_ROW + a1] = T.substitution[a1 * TD_ALPHABET + a2];
  if ((rc = dev_upload(c, J.wt.b, wt.data(), wt.size()))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));             /* (`wt` leaves scope) */
  P.segments = pairs_segments(c, c->tcrdist_segments, J.blocks, J.nr_max);
  P.wt = J.wt.b.p;
  P.cutoff = (uint32_t)cutoff;
  P.stage_refs = (uint32_t)c->tcrdist_stage_refs;
  return CMPR_OK;
}

/* the compare kernel over every job: a launch per run of jobs of one form */
template <int SINK>
int td_launch(cmpr_context *c, const TdWork &J)
{
  return pairs_launch(c, J.runs, J.P, [](uint32_t form) { return td_kernel_for<SINK>(form); });
}

/* the refusals of both calls, before any device work */
int td_refusals(cmpr_context *c, const std::string &who, const cmpr_set_view *set1, const cmpr_set_view *set2,
                const cmpr_tcrdist_params *T, int64_t cutoff, HmKind kind, bool on_device)
{
  int rc;
  if ((rc = hm_refusals(c, who, set1, set2, cutoff, kind, on_device, true)))
    return rc;
  if (!T)
    return fail(c, CMPR_EINVAL, who + ": params is NULL");
  if (!T->substitution)
    return fail(c, CMPR_EINVAL, who + ": params->substitution is NULL");
  if (cutoff > 65535)
    return fail(c, CMPR_EINVAL, who + ": cutoff above 65535 (the distance column is uint16)");
  for (uint32_t r : T->reserved)
    if (r)
      return fail(c, CMPR_EINVAL, who + ": params->reserved must be zero");
  if (T->gap_mode != CMPR_GAP_FIXED && T->gap_mode != CMPR_GAP_SLIDING)
    return fail(c, CMPR_EINVAL, who + ": params->gap_mode must be CMPR_GAP_FIXED or CMPR_GAP_SLIDING");
  if (T->v_distance && c->opt.ignore_genes)
    return fail(c, CMPR_EINVAL, who + ": params->v_distance with options.ignore_genes (there are no V gene numbers)");
  if (c->opt.alphabet_size == 4)
    return fail(c, CMPR_EUNSUPPORTED, "cmpr_tcrdist: amino acids only");
  return CMPR_OK;
}

int tcrdist_matrix_impl(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2,
                        const cmpr_tcrdist_params *T, int64_t cutoff, void *matrix_out, bool on_device)
{
  if (!c)
    return CMPR_EINVAL;
  const std::string who = "cmpr_tcrdist_matrix";
  int rc;
  if ((rc = td_refusals(c, who, set1, set2, T, cutoff, HM_MATRIX, on_device)))
    return rc;
  if (!matrix_out)
    return fail(c, CMPR_EINVAL, who + ": matrix_out is NULL");
  TdWork J;
  if ((rc = pairs_timed_setup(c, c->td_ms, false,
                              [&] { return td_setup(c, who, set1, set2, *T, cutoff, on_device, J); })))
    return rc;
  return pairs_matrix(c, J, J.P.sink, matrix_out, on_device, [&] { return td_launch<SINK_MATRIX>(c, J); }, c->td_ms, 3);
}

int tcrdist_neighbors_impl(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2,
                           const cmpr_tcrdist_params *T, int64_t cutoff, uint64_t capacity, uint64_t *row_start_out,
                           uint32_t *hit_out, uint16_t *dist_out, uint64_t *n_edges_out, bool on_device)
{
  if (!c)
    return CMPR_EINVAL;
  const std::string who = "cmpr_tcrdist_neighbors";
  int rc;
  if ((rc = pairs_neighbors_args(c, who, capacity, hit_out, n_edges_out)) ||
      (rc = td_refusals(c, who, set1, set2, T, cutoff, HM_NEIGHBORS, on_device)))
    return rc;
  TdWork J;
  if ((rc = pairs_timed_setup(c, c->td_ms, false,
                              [&] { return td_setup(c, who, set1, set2, *T, cutoff, on_device, J); })))
    return rc;
  /* the rows always (the row order reads them); the row order into td_ms[2] */
  return pairs_neighbors(c, who, J, J.P.segments, J.P.sink, capacity, row_start_out, hit_out, dist_out, n_edges_out,
                         on_device, [&] { return td_launch<SINK_CSR>(c, J); }, true, c->td_ms, 2, 3);
}

}  // namespace

extern "C" int cmpr_tcrdist_matrix(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2,
                                   const cmpr_tcrdist_params *params, int64_t cutoff, uint64_t *matrix_out)
{
  return guarded(c, [&] { return tcrdist_matrix_impl(c, set1, set2, params, cutoff, matrix_out, false); });
}

extern "C" int cmpr_tcrdist_matrix_device(cmpr_context *c, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                                          const cmpr_tcrdist_params *params, int64_t cutoff, void *d_matrix)
{
  return guarded(c, [&] { return tcrdist_matrix_impl(c, d_set1, d_set2, params, cutoff, d_matrix, true); });
}

extern "C" int cmpr_tcrdist_neighbors(cmpr_context *c, const cmpr_set_view *set1, const cmpr_set_view *set2,
                                      const cmpr_tcrdist_params *params, int64_t cutoff, uint64_t capacity,
                                      uint64_t *row_start_out, uint32_t *hit_out, uint16_t *distance_out,
                                      uint64_t *n_edges_out)
{
  return guarded(c, [&] {
    return tcrdist_neighbors_impl(c, set1, set2, params, cutoff, capacity, row_start_out, hit_out, distance_out,
                                  n_edges_out, false);
  });
}

extern "C" int cmpr_tcrdist_neighbors_device(cmpr_context *c, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                                             const cmpr_tcrdist_params *params, int64_t cutoff, uint64_t capacity,
                                             uint64_t *d_row_start_out, uint32_t *d_hit_out, uint16_t *d_distance_out,
                                             uint64_t *n_edges_out)
{
  return guarded(c, [&] {
    return tcrdist_neighbors_impl(c, d_set1, d_set2, params, cutoff, capacity, d_row_start_out, d_hit_out,
                                  d_distance_out, n_edges_out, true);
  });
}
