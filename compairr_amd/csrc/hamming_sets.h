/*
 * hamming_sets.h -- what the all-against-all calls of hamming.hip (cmpr_hamming_*) and edit.hip (cmpr_edit_*) share in
 * front of their compare kernels: a staged set grouped by (length, V, J) and packed in group order, the refusals, and
 * the score of a matching pair.  Defined in hamming.hip, whose head comment describes the grouping and the packing.
 */
#ifndef COMPAIRR_AMD_HAMMING_SETS_H
#define COMPAIRR_AMD_HAMMING_SETS_H

#include "context.h"

namespace cmpr {

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
};

/* words per sequence of a group of `len` residues: the next word count the register form is compiled for, or the
   words themselves beyond HAMMING_REG_WORDS */
uint32_t stride_of(uint32_t len, uint32_t per_word);

/* the staged set H grouped and packed */
int hm_prepare(cmpr_context *c, HmSet &H);

/* what a call makes of the pairs: the clusters and the nearest neighbours take no score, so what the reference refuses
   of scores is not theirs.  HM_NEAREST: `differences` is the call's min_distance */
enum HmKind { HM_MATRIX, HM_NEIGHBORS, HM_CLUSTERS, HM_NEAREST };

/* the refusals of the all-against-all calls, before any device work.  with_indels: the call compares by edit
   distance (cmpr_edit_*), options.indels is not looked at */
int hm_refusals(cmpr_context *c, const std::string &who, const cmpr_set_view *set1, const cmpr_set_view *set2,
                int64_t differences, HmKind kind, bool on_device, bool with_indels = false);

__device__ __forceinline__ unsigned long long pair_score(uint32_t score, unsigned long long f, unsigned long long g)
{
  switch (score) {
  case CMPR_SCORE_MIN: case CMPR_SCORE_JACCARD: return f < g ? f : g;
  case CMPR_SCORE_MAX:                          return f > g ? f : g;
  case CMPR_SCORE_MEAN:                         return f + g;             /* 2 x mean */
  default:                                      return f * g;             /* product, MH */
  }
}

}  // namespace cmpr

#endif
