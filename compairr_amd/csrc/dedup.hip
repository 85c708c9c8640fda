/*
 * dedup.hip -- the exact duplicates of one set.  cmpr_deduplicate / cmpr_deduplicate_device: the reference's
 * --deduplicate (dedup.cc:27-132, 184-199) for a set in host or in device memory.  cmpr_count_duplicates: the
 * number alone -- a lookup of every entry in the record tables of the resident reference, or in a table built
 * for a passed-in set (count_duplicates_kernel, at the end).
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
 * Nothing here writes the resident sets, plans or statistics of the context.
 */
#include "context.h"

#include <algorithm>
#include <string>
#include <vector>

using namespace cmpr;

namespace {

constexpr uint32_t DEDUP_WG = 256;                        /* threads per workgroup, all four kernels but the scan */
constexpr uint32_t DEDUP_SCAN_WG = 1024;
constexpr unsigned long long DEDUP_EMPTY = ~0ull;         /* (tag << 32) | index is never this: index < 2^32 - 64 */
constexpr size_t DEDUP_ZOB_LDS_BYTES = 12288;             /* the Zobrist keys go to LDS up to this (query_layout.hip) */

/* the entries of a set and the keys they are hashed with */
struct EntrySet {
  const uint64_t *zob;
  uint32_t        A, zpos, n_v, use_genes;
  const uint8_t  *res;
  const uint64_t *off;
  const uint32_t *v, *j, *rep;
};

struct DedupParams {
  EntrySet        S;
  uint32_t        zob_lds, zob_words;      /* the keys (gene keys included) are copied to LDS */
  uint32_t        tag_drop;                /* 32 - dedup_tag_bits: the tag is the hash's low dword without its low bits */
  uint32_t        pad;
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

/* Zobrist hash of entry i (residues at b, length L; zobrist.cc:74-88) with the keys at zt: S.zob or a copy of it */
__device__ __forceinline__ uint64_t entry_hash(const EntrySet &S, const uint64_t *zt, uint64_t i, uint64_t b, uint32_t L)
{
  uint64_t h = 0;
  if (S.use_genes) {
    const uint64_t *vk = zt + (uint64_t)S.A * S.zpos;
    h = vk[S.v[i]] ^ vk[S.n_v + S.j[i]];
  }
  for (uint32_t p = 0; p < L; p++)
    h ^= zt[S.A * p + S.res[b + p]];
  return h;
}

/* sequence i (residues at b, length L) and sequence o are the same entry (dedup.cc:90-111) */
__device__ __forceinline__ bool same_entry(const EntrySet &S, uint64_t i, uint64_t o, uint64_t b, uint32_t L)
{
  if (S.rep[o] != S.rep[i])
    return false;
  if (S.use_genes && (S.v[o] != S.v[i] || S.j[o] != S.j[i]))
    return false;
  const uint64_t ob = S.off[o];
  if ((uint32_t)(S.off[o + 1] - ob) != L)
    return false;
  for (uint32_t p = 0; p < L; p++)
    if (S.res[ob + p] != S.res[b + p])
      return false;
  return true;
}

/* One thread per sequence: its hash, then the walk.
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
      dedup_zl[k] = P.S.zob[k];
    __syncthreads();
  }
  const uint64_t *const zt = P.zob_lds ? dedup_zl : P.S.zob;
  const uint64_t step = (uint64_t)gridDim.x * DEDUP_WG;
  for (uint64_t i = (uint64_t)blockIdx.x * DEDUP_WG + threadIdx.x; i < P.n; i += step) {
    const uint64_t b = P.S.off[i];
    const uint32_t L = (uint32_t)(P.S.off[i + 1] - b);
    const uint64_t h = entry_hash(P.S, zt, i, b, L);
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
      if ((uint32_t)(w >> 32) == tag && same_entry(P.S, i, w & 0xffffffffull, b, L)) {
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

/* Exact duplicates counted, not merged: entry i counts when an entry j < i of the same repertoire has the same
   sequence (and V/J unless -g) -- what hash_insert reports while indexing (overlap.cc:76-115) and
   check_duplicates() sums (overlap.cc:579-605).  The reference finds j because it inserts in input order; the
   tables here are built in parallel, so every entry of the key's chain is inspected and "earlier" is decided
   by the number.  A set in parts has a table per part: entry i of part p is looked up in the tables of parts
   0 .. p -- the later parts hold only later entries.  A table is the record table of a resident part (global
   numbers in RefRec::idx) or the open-addressing table of a passed-in part (local numbers, `base` added). */
struct DupTable {
  const void *t;
  uint64_t    mask;                /* buckets - 1 (record table) / slots - 1 */
  uint64_t    base;                /* Slot tables: global number of the part's first entry */
  uint32_t    records;             /* 1: RefRec table, 0: Slot table */
  uint32_t    pad;
};

struct DupParams {
  EntrySet        S;               /* the whole set */
  uint64_t        first, n;        /* the entries of part p */
  DupTable        part0;           /* the table of part 0 */
  const DupTable *more;            /* those of parts 1 .. ntables - 1 */
  uint32_t        ntables;         /* p + 1 */
  unsigned long long *count;
};

__global__ void __launch_bounds__(BLOCK_THREADS)
count_duplicates_kernel(const DupParams B)
{
  const uint64_t t = (uint64_t)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  bool dup = false;
  if (t < B.n) {
    const uint64_t i = B.first + t;
    const uint64_t b = B.S.off[i];
    const uint32_t L = (uint32_t)(B.S.off[i + 1] - b);
    const uint64_t key = table_key(entry_hash(B.S, B.S.zob, i, b, L));
    for (uint32_t q = 0; q < B.ntables && !dup; q++) {
      const DupTable T = q ? B.more[q - 1] : B.part0;
      if (T.records) {
        const uint32_t bk = dir_bucket(key, (uint32_t)T.mask);
        /* the records of the key's bucket, one after the other (a slot behind the last bucket is empty) */
        for (const RefRec *r = (const RefRec *)T.t + bk;; r++) {
          const uint32_t ri = r->idx, rl = r->len, rh = r->home;
          if (ri == REC_EMPTY)
            break;
          if (rh == bk && (rl >> REC_TAG_SHIFT) == dir_tag(key) && ri < i && same_entry(B.S, i, ri, b, L)) {
            dup = true;
            break;
          }
          if (walk_ends(ri, rl, rh, bk))
            break;
        }
      } else {
        for (uint64_t slot = table_home(key, T.mask);; slot = (slot + 1) & T.mask) {
          const Slot sl = ((const Slot *)T.t)[slot];
          if (sl.key == EMPTY_KEY)
            break;
          if (sl.key == key && T.base + sl.val < i && same_entry(B.S, i, T.base + sl.val, b, L)) {
            dup = true;
            break;
          }
        }
      }
    }
  }
  const uint64_t m = __ballot(dup);
  if (m && lane_id() == 0)
    atomicAdd(B.count, (unsigned long long)__popcll(m));
}

/* The Zobrist keys for a set whose longest sequence has `longest` residues: the resident ones when a reference
   is resident and long enough, else a freshly drawn table in `own`.  (Every user compares the residues in
   full: no result depends on the keys.) */
int keys_for_set(cmpr_context *c, uint32_t longest, DevBuf<uint64_t> &own, const uint64_t *&zob, uint32_t &zpos)
{
  zob = c->zob.p;
  zpos = c->zpos;
  if (c->have_ref && longest + EXTRA_POSITIONS <= c->zpos)
    return CMPR_OK;
  zpos = longest + EXTRA_POSITIONS;
  const uint32_t genes = c->opt.ignore_genes ? 0 : c->opt.n_v_genes + c->opt.n_j_genes;
  std::vector<uint64_t> z((size_t)c->opt.alphabet_size * zpos + genes);
  SplitMix64 rng(0x6465647570ull);   /* "dedup" */
  for (auto &x : z)
    x = rng.next();
  int rc;
  if ((rc = dev_upload(c, own, z.data(), z.size()))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));            /* (z leaves scope) */
  zob = own.p;
  return CMPR_OK;
}

int deduplicate_impl(cmpr_context *c, const cmpr_set_view *s, bool on_device, uint64_t capacity,
                     uint32_t *first_out, uint64_t *count_out, uint64_t *n_unique_out, uint64_t *merged_out)
{
  if (!c)
    return CMPR_EINVAL;
  if (capacity && (!first_out || !count_out))
    return fail(c, CMPR_EINVAL, "cmpr_deduplicate: output arrays are NULL with a capacity");
  if (n_unique_out) *n_unique_out = 0;
  if (merged_out) *merged_out = 0;

  /* upload (a device view: a copy inside the device) + validation on the device (query_layout.hip) */
  StagedSet set;
  int rc;
  if ((rc = cmpr_stage_set(c, s, on_device, set)))
    return rc;
  Out<uint32_t> first(first_out, on_device);
  Out<uint64_t> count(count_out, on_device);
  Tmp<uint64_t> zob_own;
  Tmp<uint32_t> slot, blk;
  Tmp<unsigned long long> table, sum, total;
  const uint64_t n = s->n;
  if (n == 0)
    return CMPR_OK;

  DedupParams P{};
  P.S.A = (uint32_t)c->opt.alphabet_size;
  P.S.n_v = c->opt.ignore_genes ? 0 : c->opt.n_v_genes;
  P.S.use_genes = c->opt.ignore_genes ? 0u : 1u;
  if ((rc = keys_for_set(c, set.longest, zob_own.b, P.S.zob, P.S.zpos))) return rc;
  P.S.res = set.res.b.p; P.S.off = set.off.b.p; P.S.v = set.v.b.p; P.S.j = set.j.b.p; P.S.rep = set.rep.b.p;

  /* one table under the 70 % rule of hashtable.cc:24; slot numbers are 32 bits, so beyond 0.7 x 2^32
     sequences it is fuller than that (never full: there are fewer classes than 2^32 - 64) */
  uint64_t slots = 4;
  while (FILL_PERCENT * slots < 100 * n && slots < (1ull << 32))
    slots <<= 1;
  const uint64_t nblk = (n + DEDUP_WG - 1) / DEDUP_WG;
  if ((rc = dev_alloc(c, table.b, (size_t)slots))) return rc;
  if ((rc = dev_alloc(c, slot.b, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, sum.b, (size_t)n))) return rc;
  if ((rc = dev_alloc(c, blk.b, (size_t)nblk))) return rc;
  if ((rc = dev_alloc(c, total.b, 1))) return rc;
  HIP_TRY(c, hipMemsetAsync(table.b.p, 0xff, slots * sizeof(unsigned long long), c->stream));
  HIP_TRY(c, hipMemsetAsync(sum.b.p, 0, n * sizeof(unsigned long long), c->stream));

  P.zob_words = (uint32_t)((size_t)P.S.A * P.S.zpos + P.S.n_v + (c->opt.ignore_genes ? 0 : c->opt.n_j_genes));
  P.zob_lds = (size_t)P.zob_words * sizeof(uint64_t) <= DEDUP_ZOB_LDS_BYTES ? 1u : 0u;
  P.tag_drop = 32u - (uint32_t)c->dedup_tag_bits;
  P.cnt = c->opt.ignore_counts ? nullptr : set.cnt.b.p;
  P.n = n;
  P.table = table.b.p; P.slot_mask = slots - 1;
  P.slot = slot.b.p; P.sum = sum.b.p; P.blk = blk.b.p; P.total = total.b.p;

  const size_t lds = P.zob_lds ? (size_t)P.zob_words * sizeof(uint64_t) : 0;
  /* (the keys are copied once per workgroup: as many workgroups as are resident, each over many sequences) */
  const uint32_t igrid = (uint32_t)std::min<uint64_t>(nblk, (uint64_t)c->cus * 8);
  hipLaunchKernelGGL(dedup_insert_kernel, dim3(igrid), dim3(DEDUP_WG), lds, c->stream, P);
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(dedup_sum_kernel, dim3((uint32_t)nblk), dim3(DEDUP_WG), 0, c->stream, P);
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(dedup_scan_kernel, dim3(1), dim3(DEDUP_SCAN_WG), 0, c->stream, blk.b.p, nblk, total.b.p);
  HIP_TRY(c, hipGetLastError());
  unsigned long long classes = 0;
  HIP_TRY(c, hipMemcpyAsync(&classes, total.b.p, sizeof classes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));

  const uint64_t written = std::min<uint64_t>(capacity, classes);
  if (written) {
    P.capacity = written;
    if ((rc = first.temp(c, (size_t)written))) return rc;
    if ((rc = count.temp(c, (size_t)written))) return rc;
    P.first_out = first.p;
    P.count_out = count.p;
    hipLaunchKernelGGL(dedup_scatter_kernel, dim3((uint32_t)nblk), dim3(DEDUP_WG), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    if ((rc = first.copy_out(c, (size_t)written))) return rc;
    if ((rc = count.copy_out(c, (size_t)written))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  if (n_unique_out) *n_unique_out = classes;
  if (merged_out) *merged_out = n - classes;
  return CMPR_OK;
}

int count_duplicates_impl(cmpr_context *c, const cmpr_set_view *s, uint64_t *out)
{
  if (!c || !out)
    return CMPR_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  *out = 0;
  int rc;
  StagedSet set;
  Tmp<uint64_t> zob_own;
  Tmp<unsigned long long> count;
  Tmp<DupTable> more;
  std::vector<Tmp<Slot>> slots;                /* a passed-in set: the table of each part */

  DupParams B{};
  B.S.A = (uint32_t)c->opt.alphabet_size;
  B.S.n_v = c->opt.ignore_genes ? 0 : c->opt.n_v_genes;
  B.S.use_genes = c->opt.ignore_genes ? 0u : 1u;
  std::vector<DupTable> tabs;                  /* parts 0 .. */
  std::vector<uint64_t> first;                 /* their first entries, and the set's size */
  if (!s) {
    if (!c->have_ref)
      return fail(c, CMPR_ESTATE, "cmpr_set_reference must be called first");
    B.S.zob = c->zob.p; B.S.zpos = c->zpos;
    B.S.res = c->res2.p; B.S.off = c->off2.p; B.S.v = c->v2.p; B.S.j = c->j2.p; B.S.rep = c->rep2.p;
    tabs.push_back(DupTable{c->rec2.p, c->slots - 1, 0, 1u, 0u});
    first.push_back(0);
    for (const RefPart &rp : c->xparts) {
      tabs.push_back(DupTable{rp.rec.p, rp.slots - 1, 0, 1u, 0u});
      first.push_back(rp.first);
    }
    first.push_back(c->n2);
  } else {
    /* the view as host memory; upload + validation on the device (query_layout.hip) */
    if ((rc = cmpr_stage_set(c, s, false, set)))
      return rc;
    if ((rc = keys_for_set(c, set.longest, zob_own.b, B.S.zob, B.S.zpos))) return rc;
    B.S.res = set.res.b.p; B.S.off = set.off.b.p; B.S.v = set.v.b.p; B.S.j = set.j.b.p; B.S.rep = set.rep.b.p;
    /* a set larger than one table of at most 2^part_buckets_log2 slots: a table per contiguous part */
    const uint64_t per_part = (uint64_t)FILL_PERCENT * (1ull << c->part_buckets_log2) / 100;
    const uint64_t nparts = s->n > per_part ? (s->n + per_part - 1) / per_part : 1;
    if (nparts > 65536)
      return fail(c, CMPR_EUNSUPPORTED, "set needs more than 65536 parts (part_buckets_log2)");
    slots.resize((size_t)nparts);
    const uint64_t q = s->n / nparts, r = s->n % nparts;
    for (uint64_t p = 0; p <= nparts; p++)
      first.push_back(p * q + std::min(p, r));
    for (uint64_t p = 0; p < nparts; p++) {
      const uint64_t f = first[(size_t)p], n = first[(size_t)p + 1] - f;
      uint64_t ps = 4;                         /* chains start on 4-slot boundaries */
      while (FILL_PERCENT * ps < 100 * n)
        ps <<= 1;
      Slot *&table = slots[(size_t)p].b.p;
      if ((rc = dev_alloc(c, slots[(size_t)p].b, (size_t)ps))) return rc;
      HIP_TRY(c, hipMemsetAsync(table, 0xff, ps * sizeof(Slot), c->stream));
      BuildParams K{};
      K.zob = B.S.zob; K.A = B.S.A; K.zpos = B.S.zpos; K.n_v = B.S.n_v; K.use_genes = B.S.use_genes;
      K.res = B.S.res; K.off = B.S.off + f; K.v = B.S.v ? B.S.v + f : nullptr; K.j = B.S.j ? B.S.j + f : nullptr;
      K.n = n;
      K.table = table; K.slot_mask = ps - 1;       /* table only: no filter */
      if (n) {
        hipLaunchKernelGGL(build_index_kernel, dim3((uint32_t)((n + BLOCK_THREADS - 1) / BLOCK_THREADS)),
                           dim3(BLOCK_THREADS), 0, c->stream, K);
        HIP_TRY(c, hipGetLastError());
      }
      tabs.push_back(DupTable{table, ps - 1, f, 0u, 0u});
    }
  }

  /* one tail: part p's entries against the tables of parts 0 .. p, the counter copied back */
  if ((rc = dev_alloc(c, count.b, 1))) return rc;
  HIP_TRY(c, hipMemsetAsync(count.b.p, 0, sizeof(unsigned long long), c->stream));
  if (tabs.size() > 1 && (rc = dev_upload(c, more.b, tabs.data() + 1, tabs.size() - 1))) return rc;
  B.part0 = tabs[0];
  B.more = more.b.p;
  B.count = count.b.p;
  for (size_t p = 0; p < tabs.size(); p++) {
    B.first = first[p];
    B.n = first[p + 1] - first[p];
    B.ntables = (uint32_t)p + 1;
    if (B.n) {
      hipLaunchKernelGGL(count_duplicates_kernel, dim3((uint32_t)((B.n + BLOCK_THREADS - 1) / BLOCK_THREADS)),
                         dim3(BLOCK_THREADS), 0, c->stream, B);
      HIP_TRY(c, hipGetLastError());
    }
  }
  unsigned long long hc = 0;
  HIP_TRY(c, hipMemcpyAsync(&hc, count.b.p, sizeof hc, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *out = hc;
  return CMPR_OK;
}

}  // namespace

extern "C" int cmpr_count_duplicates(cmpr_context *c, const cmpr_set_view *s, uint64_t *out)
{
  return guarded(c, [&] { return count_duplicates_impl(c, s, out); });
}

extern "C" int cmpr_deduplicate(cmpr_context *c, const cmpr_set_view *set, uint64_t capacity,
                                uint32_t *first_out, uint64_t *count_out,
                                uint64_t *n_unique_out, uint64_t *merged_out)
{
  return guarded(c, [&] { return deduplicate_impl(c, set, false, capacity, first_out, count_out, n_unique_out, merged_out); });
}

extern "C" int cmpr_deduplicate_device(cmpr_context *c, const cmpr_set_view *d_set, uint64_t capacity,
                                       uint32_t *d_first_out, uint64_t *d_count_out,
                                       uint64_t *n_unique_out, uint64_t *merged_out)
{
  return guarded(c, [&] { return deduplicate_impl(c, d_set, true, capacity, d_first_out, d_count_out, n_unique_out, merged_out); });
}
