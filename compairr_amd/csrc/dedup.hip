/*
 * dedup.hip -- cmpr_deduplicate / cmpr_deduplicate_device: the reference's --deduplicate
 * (dedup.cc:27-132, 184-199) for a set in host or in device memory.
 *
 * The reference inserts the sequences one after the other and links every sequence to the last equal one
 * before it (process(), dedup.cc:60-132); report() then prints a chain at its first member with the summed
 * count (dedup.cc:27-57).  In parallel there is no "before": here every equivalence class ends up owning ONE
 * slot of an open-addressing table, and that slot holds the smallest sequence number of the class, whatever
 * the schedule (dedup_insert_kernel).  Four kernels, one thread per sequence each:
 *
 *   dedup_insert_kernel   hash, walk the chain, claim an empty slot or join the class that owns one
 *   dedup_sum_kernel      the class's first member from the slot; duplicate_count added to its sum; the
 *                         first members counted per workgroup
 *   dedup_scan_kernel     exclusive scan of those counts (one workgroup)
 *   dedup_scatter_kernel  (first, count) of every class written in increasing `first`
 *
 * Nothing here reads or writes the resident sets, plans or statistics of the context.
 */
#include "context.h"

#include <algorithm>
#include <new>
#include <string>
#include <vector>

using namespace cmpr;

namespace {

constexpr uint32_t DEDUP_WG = 256;                        /* threads per workgroup, all four kernels but the scan */
constexpr uint32_t DEDUP_SCAN_WG = 1024;
constexpr unsigned long long DEDUP_EMPTY = ~0ull;         /* (tag << 32) | index is never this: index < 2^32 - 64 */
constexpr size_t DEDUP_ZOB_LDS_BYTES = 12288;             /* the Zobrist keys go to LDS up to this (query_layout.hip) */

struct DedupParams {
  const uint64_t *zob;
  uint32_t        A, zpos, n_v, use_genes;
  uint32_t        zob_lds, zob_words;      /* the keys (gene keys included) are copied to LDS */
  uint32_t        tag_drop;                /* 32 - dedup_tag_bits: the tag is the hash's low dword without its low bits */
  uint32_t        pad;
  const uint8_t  *res;
  const uint64_t *off;
  const uint32_t *v, *j, *rep;
  const uint64_t *cnt;                     /* NULL: every sequence counts 1 (ignore_counts) */
  uint64_t        n;
  unsigned long long *table;               /* (tag << 32) | sequence number, DEDUP_EMPTY: free */
  uint64_t        slot_mask;
  uint32_t       *slot;                    /* per sequence: its class's slot; after dedup_sum_kernel its class's first */
  unsigned long long *sum;                 /* per sequence number: the count of the class it is the first of */
  uint32_t       *blk;                     /* first members per workgroup of DEDUP_WG sequences, then their exclusive scan */
  unsigned long long *total;               /* number of classes */
  uint64_t        capacity;
  uint32_t       *first_out;
  uint64_t       *count_out;
};

/* sequence i (residues at b, length L) and sequence o are the same entry (dedup.cc:90-111) */
__device__ __forceinline__ bool same_entry(const DedupParams &P, uint64_t i, uint64_t o, uint64_t b, uint32_t L)
{
  if (P.rep[o] != P.rep[i])
    return false;
  if (P.use_genes && (P.v[o] != P.v[i] || P.j[o] != P.j[i]))
    return false;
  const uint64_t ob = P.off[o];
  if ((uint32_t)(P.off[o + 1] - ob) != L)
    return false;
  for (uint32_t p = 0; p < L; p++)
    if (P.res[ob + p] != P.res[b + p])
      return false;
  return true;
}

/* One thread per sequence: the hash of build_index_kernel (kernels.h; zobrist.cc:74-88), then the walk.
   A slot is claimed once (CAS on the empty word) and never freed, and from then on it belongs to the
   claimer's CLASS: the only later write is an atomicMin by a sequence that has compared itself equal to the
   slot's owner of the moment, so every owner a slot ever has is of one class, and a comparison against any
   of them decides.  Equal sequences hash alike and walk the same chain past the same foreign slots, so they
   all stop at the first slot of their class, and the minimum leaves the smallest number there.

   Other workgroups, on other XCDs, write the table while this kernel runs: its words are read with agent-
   scope atomic loads, never plain ones.  The set's own arrays are read-only here: plain loads. */
__global__ void __launch_bounds__(DEDUP_WG)
dedup_insert_kernel(const DedupParams P)
{
  extern __shared__ uint64_t dedup_zl[];
  if (P.zob_lds) {
    for (uint32_t k = threadIdx.x; k < P.zob_words; k += DEDUP_WG)
      dedup_zl[k] = P.zob[k];
    __syncthreads();
  }
  const uint64_t *const zt = P.zob_lds ? dedup_zl : P.zob;
  const uint64_t step = (uint64_t)gridDim.x * DEDUP_WG;
  for (uint64_t i = (uint64_t)blockIdx.x * DEDUP_WG + threadIdx.x; i < P.n; i += step) {
    const uint64_t b = P.off[i];
    const uint32_t L = (uint32_t)(P.off[i + 1] - b);
    uint64_t h = 0;
    if (P.use_genes) {
      const uint64_t *vk = zt + (uint64_t)P.A * P.zpos;
      h = vk[P.v[i]] ^ vk[P.n_v + P.j[i]];
    }
    for (uint32_t p = 0; p < L; p++)
      h ^= zt[P.A * p + P.res[b + p]];
    /* the slot from the high dword (hashtable.h:36-41), the tag from the low one: independent bits */
    const uint32_t tag = (uint32_t)((h & 0xffffffffull) >> P.tag_drop);
    const unsigned long long mine = ((unsigned long long)tag << 32) | (uint32_t)i;
    uint64_t slot = (h >> 32) & P.slot_mask;
    for (;;) {
      unsigned long long w = __hip_atomic_load(&P.table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (w == DEDUP_EMPTY) {
        w = atomicCAS(&P.table[slot], DEDUP_EMPTY, mine);
        if (w == DEDUP_EMPTY)
          break;                           /* claimed: the class's slot, this sequence its first so far */
        /* lost: w is what the winner put here -- the same slot is looked at again */
      }
      if ((uint32_t)(w >> 32) == tag && same_entry(P, i, w & 0xffffffffull, b, L)) {
        if (mine < w)                      /* (the word only ever gets smaller: nothing to do for a larger number) */
          atomicMin(&P.table[slot], mine);
        break;
      }
      slot = (slot + 1) & P.slot_mask;
    }
    P.slot[i] = (uint32_t)slot;
  }
}

/* The table is final (kernel boundary).  Per sequence: the first member of its class, kept in place of the
   slot; its count added to that member's sum -- integer adds, the same total in any order; the first members
   of this workgroup's DEDUP_WG sequences counted for the scan. */
__global__ void __launch_bounds__(DEDUP_WG)
dedup_sum_kernel(const DedupParams P)
{
  __shared__ uint32_t firsts;
  if (threadIdx.x == 0)
    firsts = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * DEDUP_WG + threadIdx.x;
  bool is_first = false;
  if (i < P.n) {
    const uint32_t first = (uint32_t)P.table[P.slot[i]];
    P.slot[i] = first;
    atomicAdd(&P.sum[first], (unsigned long long)(P.cnt ? P.cnt[i] : 1ull));
    is_first = first == (uint32_t)i;
  }
  const uint64_t m = __ballot(is_first);
  if (m && lane_id() == 0)
    atomicAdd(&firsts, (uint32_t)__popcll(m));
  __syncthreads();
  if (threadIdx.x == 0)
    P.blk[blockIdx.x] = firsts;
}

/* Exclusive scan of nblk counts in place, by one workgroup: DEDUP_SCAN_WG at a time, the running total
   carried along by every thread.  (The offsets fit 32 bits: there are fewer than 2^32 sequences.) */
__global__ void __launch_bounds__(DEDUP_SCAN_WG)
dedup_scan_kernel(uint32_t *blk, uint64_t nblk, unsigned long long *total)
{
  __shared__ uint32_t wave_sum[DEDUP_SCAN_WG / WAVE];
  const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  uint64_t run = 0;
  for (uint64_t base = 0; base < nblk; base += DEDUP_SCAN_WG) {
    const uint64_t k = base + threadIdx.x;
    const uint32_t x = k < nblk ? blk[k] : 0u;
    uint32_t incl = x;
    for (uint32_t d = 1; d < WAVE; d <<= 1) {
      const uint32_t y = __shfl_up(incl, d, WAVE);
      if (lane >= d)
        incl += y;
    }
    if (lane == WAVE - 1)
      wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < DEDUP_SCAN_WG / WAVE; w++) {
      const uint32_t s = wave_sum[w];
      before += w < wave ? s : 0u;
      all += s;
    }
    if (k < nblk)
      blk[k] = (uint32_t)(run + before + incl - x);
    run += all;
    __syncthreads();
  }
  if (threadIdx.x == 0)
    *total = run;
}

/* The first members in increasing number: position = firsts of the workgroups before + of the waves before
   + of the lanes before.  Only positions below the capacity are written. */
__global__ void __launch_bounds__(DEDUP_WG)
dedup_scatter_kernel(const DedupParams P)
{
  __shared__ uint32_t wave_cnt[DEDUP_WG / WAVE];
  const uint32_t wave = threadIdx.x / WAVE;
  const uint64_t i = (uint64_t)blockIdx.x * DEDUP_WG + threadIdx.x;
  const bool is_first = i < P.n && P.slot[i] == (uint32_t)i;
  const uint64_t m = __ballot(is_first);
  if (lane_id() == 0)
    wave_cnt[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  if (!is_first)
    return;
  uint64_t pos = (uint64_t)P.blk[blockIdx.x] + rank_below(m);
  for (uint32_t w = 0; w < wave; w++)
    pos += wave_cnt[w];
  if (pos < P.capacity) {
    P.first_out[pos] = (uint32_t)i;
    P.count_out[pos] = P.sum[i];
  }
}

int deduplicate_impl(cmpr_context *c, const cmpr_set_view *s, bool on_device, uint64_t capacity,
                     uint32_t *first_out, uint64_t *count_out, uint64_t *n_unique_out, uint64_t *merged_out)
{
  if (!c)
    return CMPR_EINVAL;
  std::string why;
  int rc;
  if ((rc = validate_view(c->opt, s, why, on_device)))
    return fail(c, rc, why);
  if (capacity && (!first_out || !count_out))
    return fail(c, CMPR_EINVAL, "cmpr_deduplicate: output arrays are NULL with a capacity");
  HIP_TRY(c, hipSetDevice(c->device));
  if (n_unique_out) *n_unique_out = 0;
  if (merged_out) *merged_out = 0;

  DevBuf<uint8_t> res;
  DevBuf<uint64_t> off, cnt, zob_own, d_count;
  DevBuf<uint32_t> v, j, rep, slot, blk, d_first;
  DevBuf<unsigned long long> table, sum, total;
  struct Cleanup {
    DevBuf<uint8_t> &a;
    DevBuf<uint64_t> &b1, &b2, &b3, &b4;
    DevBuf<uint32_t> &c1, &c2, &c3, &c4, &c5, &c6;
    DevBuf<unsigned long long> &d1, &d2, &d3;
    ~Cleanup()
    {
      a.release();
      b1.release(); b2.release(); b3.release(); b4.release();
      c1.release(); c2.release(); c3.release(); c4.release(); c5.release(); c6.release();
      d1.release(); d2.release(); d3.release();
    }
  } cleanup{res, off, cnt, zob_own, d_count, v, j, rep, slot, blk, d_first, table, sum, total};

  /* residues in all: offsets[n], which a device view keeps on the device (ref_index.hip) */
  uint64_t residues = 0;
  if (s->n && on_device) {
    uint64_t ends[2] = {0, 0};
    HIP_TRY(c, hipMemcpy(&ends[0], s->offsets, sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(&ends[1], s->offsets + s->n, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (ends[0] != 0)
      return fail(c, CMPR_EINVAL, "offsets[0] must be 0");
    if (ends[1] > 0xffffull * s->n)
      return fail(c, CMPR_EINVAL, "offsets not monotone");
    residues = ends[1];
  }
  /* upload (a device view: a copy inside the device) + validation on the device (query_layout.hip) */
  uint32_t longest = 0;
  std::vector<double> tot;
  if ((rc = cmpr_upload_and_validate(c, s, res, off, v, j, rep, cnt, longest, tot, on_device, residues)))
    return rc;
  const uint64_t n = s->n;
  if (n == 0)
    return CMPR_OK;

  /* own Zobrist keys when no reference set is resident or it is too short (cmpr_count_duplicates) */
  const uint32_t A = (uint32_t)c->opt.alphabet_size;
  const uint32_t n_v = c->opt.ignore_genes ? 0 : c->opt.n_v_genes;
  const uint32_t n_j = c->opt.ignore_genes ? 0 : c->opt.n_j_genes;
  uint32_t zpos = c->zpos;
  const uint64_t *zob = c->zob.p;
  if (!c->have_ref || longest + EXTRA_POSITIONS > c->zpos) {
    zpos = longest + EXTRA_POSITIONS;
    std::vector<uint64_t> z((size_t)A * zpos + n_v + n_j);
    SplitMix64 rng(0x6465647570ull);   /* "dedup" */
    for (auto &x : z)
      x = rng.next();
    if ((rc = dev_upload(c, zob_own, z.data(), z.size()))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));            /* (z leaves scope) */
    zob = zob_own.p;
  }

  /* one table under the 70 % rule of hashtable.cc:24; slot numbers are 32 bits, so beyond 0.7 x 2^32
     sequences it is fuller than that (never full: there are fewer classes than 2^32 - 64) */
  uint64_t slots = 4;
  while (FILL_PERCENT * slots < 100 * n && slots < (1ull << 32))
    slots <<= 1;
  const uint64_t nblk = (n + DEDUP_WG - 1) / DEDUP_WG;
  if ((rc = dev_alloc(c, table, (size_t)slots))) return rc;
  if ((rc = dev_alloc(c, slot, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, sum, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, blk, (size_t)nblk))) return rc;
  if ((rc = dev_alloc(c, total, 1))) return rc;
  HIP_TRY(c, hipMemsetAsync(table.p, 0xff, slots * sizeof(unsigned long long), c->stream));
  HIP_TRY(c, hipMemsetAsync(sum.p, 0, n * sizeof(unsigned long long), c->stream));

  DedupParams P{};
  P.zob = zob; P.A = A; P.zpos = zpos; P.n_v = n_v; P.use_genes = c->opt.ignore_genes ? 0u : 1u;
  P.zob_words = (uint32_t)((size_t)A * zpos + n_v + n_j);
  P.zob_lds = (size_t)P.zob_words * sizeof(uint64_t) <= DEDUP_ZOB_LDS_BYTES ? 1u : 0u;
  P.tag_drop = 32u - (uint32_t)c->dedup_tag_bits;
  P.res = res.p; P.off = off.p; P.v = v.p; P.j = j.p; P.rep = rep.p;
  P.cnt = c->opt.ignore_counts ? nullptr : cnt.p;
  P.n = n;
  P.table = table.p; P.slot_mask = slots - 1;
  P.slot = slot.p; P.sum = sum.p; P.blk = blk.p; P.total = total.p;

  const size_t lds = P.zob_lds ? (size_t)P.zob_words * sizeof(uint64_t) : 0;
  /* (the keys are copied once per workgroup: as many workgroups as are resident, each over many sequences) */
  const uint32_t igrid = (uint32_t)std::min<uint64_t>(nblk, (uint64_t)c->cus * 8);
  hipLaunchKernelGGL(dedup_insert_kernel, dim3(igrid), dim3(DEDUP_WG), lds, c->stream, P);
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(dedup_sum_kernel, dim3((uint32_t)nblk), dim3(DEDUP_WG), 0, c->stream, P);
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(dedup_scan_kernel, dim3(1), dim3(DEDUP_SCAN_WG), 0, c->stream, blk.p, nblk, total.p);
  HIP_TRY(c, hipGetLastError());
  unsigned long long classes = 0;
  HIP_TRY(c, hipMemcpyAsync(&classes, total.p, sizeof classes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));

  const uint64_t written = std::min<uint64_t>(capacity, classes);
  if (written) {
    P.capacity = written;
    if (on_device) {
      P.first_out = first_out;
      P.count_out = count_out;
    } else {
      if ((rc = dev_alloc(c, d_first, (size_t)written))) return rc;
      if ((rc = dev_alloc(c, d_count, (size_t)written))) return rc;
      P.first_out = d_first.p;
      P.count_out = d_count.p;
    }
    hipLaunchKernelGGL(dedup_scatter_kernel, dim3((uint32_t)nblk), dim3(DEDUP_WG), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    if (!on_device) {
      HIP_TRY(c, hipMemcpyAsync(first_out, d_first.p, written * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(count_out, d_count.p, written * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  if (n_unique_out) *n_unique_out = classes;
  if (merged_out) *merged_out = n - classes;
  return CMPR_OK;
}

int deduplicate_guarded(cmpr_context *c, const cmpr_set_view *s, bool on_device, uint64_t capacity,
                        uint32_t *first_out, uint64_t *count_out, uint64_t *n_unique_out, uint64_t *merged_out)
{
  /* the header promises CMPR_ENOMEM, not an exception across the C boundary */
  try {
    return deduplicate_impl(c, s, on_device, capacity, first_out, count_out, n_unique_out, merged_out);
  } catch (const std::bad_alloc &) {
    return fail(c, CMPR_ENOMEM, "out of host memory");
  }
}

}  // namespace

extern "C" int cmpr_deduplicate(cmpr_context *c, const cmpr_set_view *set, uint64_t capacity,
                                uint32_t *first_out, uint64_t *count_out,
                                uint64_t *n_unique_out, uint64_t *merged_out)
{
  return deduplicate_guarded(c, set, false, capacity, first_out, count_out, n_unique_out, merged_out);
}

extern "C" int cmpr_deduplicate_device(cmpr_context *c, const cmpr_set_view *d_set, uint64_t capacity,
                                       uint32_t *d_first_out, uint64_t *d_count_out,
                                       uint64_t *n_unique_out, uint64_t *merged_out)
{
  return deduplicate_guarded(c, d_set, true, capacity, d_first_out, d_count_out, n_unique_out, merged_out);
}
