/*
 * context.h -- private to libcompairr_hip.so: the context behind the C ABI and
 * the helpers its translation units share (compairr_hip.hip: the entry points;
 * query_layout.hip: the device-side layout of set 1; ref_index.hip: the index
 * of set 2).
 */
#ifndef COMPAIRR_AMD_CONTEXT_H
#define COMPAIRR_AMD_CONTEXT_H

#include "../../include/compairr_hip.h"
#include "kernels.h"

#include "select.h"

#include <algorithm>
#include <chrono>
#include <functional>
#include <map>
#include <new>
#include <set>
#include <string>
#include <vector>

/* deterministic table contents; the result does not depend on them
   (check_variant makes matches hash-independent, variants.cc:166-240) */
struct SplitMix64 {
  uint64_t s;
  explicit SplitMix64(uint64_t seed) : s(seed) {}
  uint64_t next()
  {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
};

template <typename T>
struct DevBuf {
  T     *p = nullptr;
  size_t n = 0;
  size_t cap = 0;          /* elements allocated (>= n; dev_reserve keeps an allocation that is large enough) */
  void release()
  {
    if (p)
      (void)hipFree(p);
    p = nullptr;
    n = 0;
    cap = 0;
  }
};

/* device memory for the temporaries of a call, kept from call to call and grown when a
   call needs more (cmpr_set_queries: no hipMalloc / hipFree in the steady state) */
struct DevArena {
  char  *base = nullptr;
  size_t cap = 0;
  void release()
  {
    if (base)
      (void)hipFree(base);
    base = nullptr;
    cap = 0;
  }
};

using cmpr::Chunk;
using cmpr::PosEntry;
using cmpr::SliceGeom;
using cmpr::Slot;
using cmpr::TileDesc;

/* Everything about a step that does not change from launch to launch (kernels, grid,
   LDS, kernel arguments): worked out once after cmpr_set_queries, not per call. */
struct StepPlan {
  bool     valid = false;
  bool     will_launch = false, reduce_writes = false, deferred = false, redo_kind = false;
  size_t   cells = 0, ctr_blk = 0;
  cmpr::ProbeParams P{};            /* the per-launch fields are filled in at enqueue */
  cmpr::ProbeFn fn = nullptr, fn2 = nullptr, rfn = nullptr;
  uint32_t grid = 0, nw = 0, rgrid = 0;
  size_t   lds = 0, rlds = 0;
};

/* where cmpr_layout_queries takes the query set from */
struct LayoutSource {
  enum Kind { HOST, DEVICE, RECORDS } kind = HOST;
  const cmpr_set_view *view = nullptr;   /* HOST: the caller's arrays; DEVICE: device pointers on the context's device */
  /* RECORDS (cmpr_set_queries_routed): route_record_bytes() each, in device memory */
  const void   *d_records = nullptr;
  uint64_t      nrec = 0;
  uint32_t      n_rep = 0;
  uint64_t      n_total = 0;             /* sequences of the WHOLE query set (-x: the matrix has that many rows) */
  const double *totals = nullptr;        /* count totals per repertoire of the whole set, or NULL */
  /* cmpr_route_queries: key the share, count the records per destination, keep it for cmpr_route_pack */
  bool          route = false;
  uint64_t      first_index = 0;
  /* what the caller has to queue on the context's stream behind the layout (its per-launch scratch): run just
     before the layout's last wait, so that the call waits once at its end, not twice */
  std::function<int()> finish;
};

/* the keyed share cmpr_route_queries leaves in arena A for cmpr_route_pack */
struct RouteState {
  bool     valid = false;
  uint64_t n = 0, first_index = 0, total_records = 0;
  uint32_t n_dest = 0, record_bytes = 0;
  unsigned long long counts[64] = {};
  std::vector<double> rep_totals;
  const uint8_t  *res = nullptr;
  const uint64_t *off = nullptr, *cnt = nullptr;
  const uint32_t *v = nullptr, *j = nullptr, *rep = nullptr;
  const uint32_t *mask_lo = nullptr, *mask_hi = nullptr;
  unsigned long long *dest = nullptr;    /* [64] counts | [64] fill cursors */
};

/* A part of set 2 beyond the first (ref_index.hip): its own filter words, record table and bucket bitmap
   over the sequences first .. first + n - 1, built with the geometry of the whole set; RefRec::idx holds
   the global sequence number.  Part 0 lives in cmpr_context's own bloom / rec2 / bmap2 / slots. */
struct RefPart {
  uint64_t              first = 0, n = 0;
  uint64_t              slots = 0;      /* buckets of its record table (a power of two) */
  DevBuf<uint64_t>      bloom;
  DevBuf<unsigned char> rec;
  DevBuf<uint32_t>      bmap;
  void release()
  {
    bloom.release();
    rec.release();
    bmap.release();
  }
};

struct cmpr_context {
  cmpr_options opt{};
  int          device = 0;
  int          cus = 256;
  hipStream_t  stream = nullptr;
  hipEvent_t   ev_stop = nullptr;
  /* kernel-time events of the last TIME_RING calls (cmpr_get_kernel_times), so
     that a caller can time many launches without synchronising after each */
  static const uint32_t TIME_RING = 64;
  hipEvent_t   ring_k0[TIME_RING] = {}, ring_km[TIME_RING] = {}, ring_k1[TIME_RING] = {};
  hipEvent_t   ring_start[TIME_RING] = {};   /* start event of the call in this slot: its own k0, or the
                                                previous call's k1 when the two ran back to back */
  hipEvent_t   ring_mid[TIME_RING] = {};     /* end of its probe kernel: its km */
  uint64_t     calls = 0;            /* overlap launches so far */
  hipEvent_t   ev_k0 = nullptr, ev_km = nullptr, ev_k1 = nullptr;   /* = the ring entry of the last call */
  bool         events_valid = false;
  bool         stop_is_k1 = false;   /* the last call ended with the kernels (ev_k1), no copy behind them */
  /* the end event of a launch on a RETIRED query set that nobody has waited for yet (retire_queries): the
     layout of the next set waits for it where it first needs to (cmpr_settle_previous_launch), and it
     outlives a call that fails before that point.  Nothing records on a ring event while it is pending:
     launches need a query set, and no set is accepted without this wait */
  hipEvent_t   pending_launch = nullptr;
  std::string  err;

  /* tunables: each is set through its row of TUNABLES (compairr_hip.hip), which holds its range and when it locks */
  int64_t blocks_per_cu = 8;
  int64_t variant = -1;           /* 0: one global Bloom; 1: LDS-staged slices; 2: LDS-staged
                                     row filter (kernels_rows.h); -1: by alphabet */
  int64_t bloom_log2_delta = -100; /* -100: default (0 for variant 0, +2 sliced) */
  int64_t row_filter_x16 = 32;    /* variant 2: filter bytes per entry, in sixteenths (32 = 2 bytes: 16 bits per
                                     entry, eight of them set) */
  int64_t slice_pages = -1;       /* variant 2, d = 1: overfull slices get up to 2^this pages; -1 = up to 8, 0 = none */
  int64_t page_budget = 0;        /* entries a slice may hold before it gets pages; 0 = 20 per word (tests: small) */
  int64_t bucket_bitmap = -1;     /* resolve_kernel asks the bucket bitmap before it reads a slot of the record table:
                                     -1 = where most positives are false (d = 2), 0 never, 1 always */
  int64_t direct_slices_log2 = -1; /* d = 0 on variant 0: pseudo-slices of the query layout (-1: by the number of queries) */
  int64_t fill_slices = 1;        /* variant 2 at d = 2 (single rows): the slices take all the words their LDS buffer holds */
  int64_t class_residues = -1;    /* -1: choose from the data                  */
  int64_t class_anchor = -1;      /* c0, -1: from set 2's lengths              */
  int64_t heavy_threshold = -1;   /* class population above which it is split;
                                     -1: from the slice size, 0: every class   */
  int64_t chunk_tiles = 0;        /* 0: 8 x waves_per_block                    */
  int64_t waves_per_block = 8;
  bool    sub2_active = false;    /* ... and the query layout in effect lists them */
  int64_t sub2_items = -1;        /* variant 1, nt, d = 2: class-changing double substitutions as items
                                     (-1 = default = on; 0: probed where the filter lies) */
  int64_t work_shard_index = 0;   /* this context works on every work_shard_count-th work   */
  int64_t work_shard_count = 1;   /* item (chunk / small tile / tile) of the step, from here */
  int64_t small_slice_tiles = 0;  /* slices with <= this many tiles are not staged (wave phase): never pays since round 2 */
  int64_t class_rows_unstaged = 0; /* variant 2: class-row tiles read the filter where it lies */
  int64_t host_threads = 0;       /* threads of the host-side layout passes; set in cmpr_create */
  int64_t table_log2_delta = 1;   /* directory buckets = 2^delta x the 70 % rule of hashtable.cc:24 */
  int64_t deferred_resolve = 1;   /* Bloom positives walked by a second kernel   */
  int64_t chunk_deal = 1;         /* variant 2: 1 = beyond a workgroup's first four, chunks are handed out by a counter
                                     in list order (heaviest first); 0 = all of them dealt statically */
  int64_t pos_capacity = 0;       /* entries of the positives buffer; 0 = auto   */
  int64_t pos_grow = -1;          /* the buffer grows to what a launch showed: -1 = when its size was automatic,
                                     1 = also from a given pos_capacity (tests), 0 = never */
  int64_t resolve_blocks_per_cu = 5; /* what resolve_kernel's registers allow      */
  int64_t pos_segments = 64;      /* independently claimed parts of that buffer  */
  bool    waves_per_block_forced = false;
  int64_t debug = 0;              /* ablation switches (layout.h DBG_*), -DCMPR_ABLATION builds only */
  int64_t slice_words_log2 = -1;  /* -1: 12 (8-byte words, variant 1) / 11 (16-byte words, variant 2) */
  int64_t part_buckets_log2 = 30; /* set 2 in parts: the most buckets of one part's record table */
  int64_t d2_pairs = -1;          /* nucleotides, d = 2 on pair rows (kernels_pairs2.h): -1 auto, 0 off, 1 on */
  int64_t d2_buffers = 1;         /* slice buffers of that kernel (layout.h SliceGeom::nbuf; cfg5: 51 ms with one, 60 with two) */
  int64_t narrow_upload = -1;     /* the narrowed upload of cmpr_set_queries: -1 auto, 0 off, 1 on */
  /* of the query layout (query_layout.hip): item counters per workgroup in LDS, hashes worked out from the
     records by fill_tiles_kernel (both 1 = default; 0 = round 5's form, kept for A/B and the parity suite),
     and HIP events around its big kernels (default 0) */
  int64_t item_wg = 1, layout_recompute = 1, layout_timing = 0;
  int64_t layout_zob_lds = 1;     /* keys_kernel keeps the Zobrist keys in LDS when they fit */
  int64_t record_tiles = 1;       /* 1 = where the layout allows (layout.h rec_tiles), the hash in the record where
                                     the sequences leave room; 2 = never the hash (rows) */
  int64_t dedup_tag_bits = 32;    /* TEST ONLY: bits of the hash a table word of cmpr_deduplicate carries (dedup.hip) */
  /* TEST ONLY, of cmpr_hamming_* (hamming.hip): references staged per LDS piece (0 = as many as fit), the
     segment count (0 = automatic), 1 = every group through the long-sequence form */
  int64_t hamming_stage_refs = 0, hamming_segments = 0, hamming_generic = 0;
  int64_t hamming_link_snapshot = 1;  /* TEST ONLY, of cmpr_hamming_cluster*: 0 = every match goes to link_pair */
  /* TEST ONLY, of cmpr_edit_* (edit.hip): references staged per LDS piece (0 = as many as fit), the segment count
     (0 = automatic), at least this many 64-bit words per column (0 = from the reference's length) */
  int64_t edit_stage_refs = 0, edit_segments = 0, edit_words = 0;
  int64_t edit_link_snapshot = 1;     /* TEST ONLY, of cmpr_edit_cluster*: 0 = every match goes to link_pair */
  int64_t edit_nearest_prune = 1;     /* TEST ONLY, of cmpr_edit_nearest*: 0 = every partner within the cap is walked */
  /* TEST ONLY, of cmpr_tcrdist_* (tcrdist.hip): references staged per LDS piece (0 = as many as fit), the segment
     count (0 = automatic) */
  int64_t tcrdist_stage_refs = 0, tcrdist_segments = 0;
  uint32_t chunk_cap = 0;         /* tiles per chunk in effect since cmpr_set_queries */

  /* sliced Bloom layout (variant 1) */
  bool                  sliced = false;   /* variant 1 or 2 */
  bool                  rows = false;     /* variant 2 */
  uint32_t              npasses = 1;      /* variant 2: 1 + class-row passes */
  SliceGeom             geom{};
  std::vector<uint32_t> ctab;     /* host copy of the class tables             */
  DevBuf<uint32_t>      d_ctab;
  DevBuf<uint32_t>      page_tab;         /* variant 2, d = 1: pages of the overfull slices (layout.h SliceGeom) */
  uint64_t              page_slices = 0;  /* overflow pages behind the regular slices */
  DevBuf<Chunk>         chunks;
  DevBuf<cmpr::TileRef> tile_refs;    /* what the chunks list */
  DevBuf<uint32_t>      small_tiles;
  uint32_t              nsmall = 0;
  uint32_t              nchunks = 0;

  /* Zobrist + patterns */
  uint32_t          zpos = 0;
  DevBuf<uint64_t>  zob;

  /* set 2 + index */
  bool              have_ref = false;
  uint64_t          n2 = 0;
  uint32_t          R2 = 0, longest2 = 0;
  DevBuf<uint8_t>   res2;
  DevBuf<uint64_t>  off2, cnt2, bloom;
  DevBuf<uint32_t>  v2, j2, rep2;
  DevBuf<uint32_t>  bmap2;          /* one bit per bucket of the record table: it holds a record */
  DevBuf<unsigned char> rec2;      /* the record table (layout.h RefRec; ref_index.hip) */
  DevBuf<uint32_t>  voff2;          /* slot of sequence i in it */
  uint64_t          slots = 0, bloom_words = 0;     /* slots: buckets of the record table (a power of two) */
  /* set 2 in parts (ref_index.hip): when one record table cannot hold it, contiguous sequence ranges, each
     with its own filter words, records and bitmap; everything the query layout reads is shared */
  uint32_t          nparts = 1;
  uint64_t          part0_n = 0;              /* sequences of part 0 (first 0) */
  std::vector<RefPart> xparts;                /* parts 1 .. nparts - 1 */
  DevBuf<unsigned long long> stats_acc;       /* nparts > 1: the counters of a step, summed over its parts */

  /* set 1 tiles */
  bool              have_q = false;
  bool              routed = false;  /* the resident queries are this context's share (cmpr_set_queries_routed) */
  RouteState        route;
  uint64_t          n1 = 0;
  uint32_t          R1 = 0, ntiles = 0;
  DevBuf<TileDesc>  tiles;
  uint32_t          nmain_tiles = 0;     /* tiles of pass 0: slot = tile * 64 + lane */
  DevBuf<uint32_t>  qres, qv, qj;    /* qv, qj: variants 0 and 1 (their tiles read them) */
  DevBuf<uint64_t>  qgh;            /* per slot: V key ^ J key (variants 0, 1: one load, not
                                       two dependent ones) / the query's Zobrist hash
                                       (variant 2; db_hash, db.cc:903-916) */
  DevBuf<uint64_t>  qhins, qhdel;   /* variant 2 with -i: the two shifted hashes
                                       (zobrist.cc:90-104, 122-136) */
  DevBuf<uint16_t>  qlen;
  DevBuf<uint32_t>  qck;
  DevBuf<cmpr::QueryRec> qrec;     /* per slot: what verification reads, 64 bytes */
  /* variant 2, class rows: per item the row's blanked hash, the query's slot in
     pass 0 (~0: padding) and its residue at the class position | position << 8 */
  DevBuf<cmpr::ItemRec> items;
  DevBuf<uint32_t>  slice_items;     /* sub2 items: per slice {first item, blocks} (layout.h CHUNK_WITH_ITEMS) */
  DevBuf<cmpr::ResPack> cpk;             /* sub2 items: the query's residues, 2 bits each */
  DevBuf<cmpr::ResPack> qpk;             /* nucleotides, d = 2 on pair rows: per slot, the query's residues */
  bool              d2pairs = false;    /* ... that kernel is in use (kernels_pairs2.h; decided with the index) */
  uint64_t          algorithmic_bytes = 0;
  double            max_cell_bound = 0;   /* max_i total1[i] * max_j total2[j] */
  std::vector<double> tot1, tot2;

  /* per-launch scratch */
  DevBuf<unsigned long long> matrix;
  DevBuf<double>             matrix_f64;
  DevBuf<PosEntry>           pos_buf;      /* deferred resolve: queued Bloom positives */
  DevBuf<unsigned long long> pos_ctr;      /* per segment: [0] claimed, [1] ~first claim that did not fit */
  unsigned long long        *ctr_cur = nullptr, *ctr_other = nullptr;   /* this launch's block / the next one's */
  bool                       ctr_clean = false;        /* ctr_other and `part` are all zero */
  /* The redo launch of variant 2 (enqueue_overlap) is dropped once a finished launch on
     these sets has shown that the fullest segment of the positives buffer stays clear
     of its capacity by more than launches can differ (which wave ends up with which
     tile only moves the number of part-filled 64-entry blocks): */
  unsigned long long        *d_usage = nullptr;        /* [0] fullest segment of a launch (reduce kernel);
                                                          [1] sticky: a launch WITHOUT redo pass overflowed */
  unsigned long long        *h_usage = nullptr;        /* pinned copy of both */
  hipEvent_t                 ev_usage = nullptr;
  bool                       usage_pending = false, never_overflows = false;
  /* the margin argument holds for one static deal of the chunks: the grid and the waves
     per workgroup the usage was measured with / the shortcut was established for */
  uint32_t                   usage_grid = 0, usage_nw = 0, safe_grid = 0, safe_nw = 0;
  bool                       last_without_redo = false;   /* the last launch relied on never_overflows */
  bool                       force_no_redo = false;       /* test only (tunable "assume_never_overflows") */
  /* a cmpr_overlap_matrix_device launch without redo pass that cmpr_get_stats has not
     looked at yet / one such was found overflowed by a synchronous call's own check */
  bool                       async_unchecked = false, async_overflowed = false;
  hipStream_t                last_stream = nullptr;       /* stream of the last enqueue (launches of one */
  bool                       have_last_stream = false;    /* context are ordered one after the other)   */
  DevArena                   arena_a, arena_b;            /* temporaries of cmpr_set_queries */
  void                      *stage_host = nullptr;        /* pinned staging of the narrowed upload */
  size_t                     stage_host_bytes = 0;
  hipStream_t                copy_stream = nullptr;       /* uploads of cmpr_set_queries */
  static const uint32_t      NCOPY_EV = 4;
  hipEvent_t                 ev_copy[NCOPY_EV] = {};
  /* of the last cmpr_set_queries: host time inside the copies, from the last copy to the
     end (the device work the upload did not hide), and in all */
  double                     layout_upload_ms = 0, layout_tail_ms = 0, layout_total_ms = 0;
  bool                       rec_tiles = false;           /* the resident layout has no per-slot arrays: the probe
                                                             kernel reads the queries' records (layout.h ProbeParams) */
  bool                       rec_hash = false;            /* ... and the query's hash lies in the record (layout.h rec_tiles == 2) */
  /* what the runtime said about a kernel with a given dynamic LDS size (asked once: a plan is made per query
     set): workgroups per CU, and whether its LDS limit has been raised */
  std::map<std::pair<const void *, size_t>, int> occupancy_seen;
  std::map<const void *, size_t>                 lds_raised;     /* per function: the largest limit set */
  void                      *h_sizes = nullptr;           /* pinned: the layout's SizesBlock arrives here */
  size_t                     h_sizes_bytes = 0;
  hipEvent_t                 ev_layout[6] = {};
  uint32_t                   layout_marks = 0;
  float                      layout_kernel_ms[5] = {};    /* keys | sizes, slices | scatter | tiles | chunk order */
  StepPlan                   plan;
  unsigned long long        *d_stats = nullptr;        /* inside pos_ctr's allocation */
  uint32_t                  *d_tile_counter = nullptr; /* likewise */
  unsigned long long        *d_overflow = nullptr, *d_stats2 = nullptr;   /* redo pass (kernels_rows.h) */
  uint32_t                  *d_tile_counter2 = nullptr;
  unsigned long long        *d_deal = nullptr;         /* chunk counters of probe_rows_kernel (DEAL_WORDS) */
  DevBuf<unsigned long long> part;           /* NPART x part_stride partial results */
  uint32_t                   part_stride = 0;
  const void                *attr_fn2 = nullptr;
  size_t                     attr_lds2 = 0;
  uint64_t                   pos_cap = 0;
  uint32_t                   launches = 0;
  const void                *attr_fn = nullptr;   /* kernel whose LDS limit is raised */
  size_t                     attr_lds = 0;
  /* pairs mode, set only while cmpr_overlap_pairs runs */
  uint32_t           *pair_q = nullptr, *pair_h = nullptr;
  unsigned long long *pair_count = nullptr;
  uint64_t            pair_cap = 0;
  /* link mode, set only while cmpr_cluster runs its step (cluster.hip): the union-find forest the matches
     are linked in, in place of being listed */
  uint32_t           *link_parent = nullptr;
  /* neighbour mode, set only while cmpr_neighbors runs one of its two steps (neighbors.hip; layout.h
     ProbeParams::nb_*): the degrees / row cursors, and for the fill step the row offsets and the hits */
  uint32_t           *nb_degree = nullptr, *nb_hit = nullptr;
  const uint64_t     *nb_row_start = nullptr;
  uint8_t            *nb_dist = nullptr;   /* fill step of cmpr_neighbors_distance only */
  double              nb_ms[4] = {};   /* host time of the last cmpr_neighbors: count | scan | fill | order */
  double              ex_ms[5] = {};   /* ... of the last cmpr_existence_csr: edges | group | count | reduce | copy-out */
  double              cl_ms[2] = {};   /* ... of the last cmpr_cluster_table: labels and sizes | the table */
  double              hm_ms[3] = {};   /* ... of the last cmpr_hamming_*: upload, groups, packing | compare | copy-out */
  double              ed_ms[4] = {};   /* ... of the last cmpr_edit_*: upload, groups, packing, jobs | compare | row order | copy-out */
  double              td_ms[4] = {};   /* ... of the last cmpr_tcrdist_*: the same four */
};


/* What cmpr_warm_up_sized() reserved before any context existed (ABI v5): the pinned staging buffer of the
   narrowed upload and one block of device memory per device, taken over by the first context that needs them
   (query_layout.hip), released by the first cmpr_destroy() if nobody did.  Process-wide, under a mutex. */
struct WarmReservation {
  void  *host = nullptr;
  size_t host_bytes = 0;
  char  *dev = nullptr;
  size_t dev_bytes = 0;
  int    device = -1;
};
/* take what fits (nullptr: nothing reserved, or too small) */
void *cmpr_take_reserved_host(size_t need, size_t *got_bytes);
char *cmpr_take_reserved_device(int device, size_t need, size_t *got_bytes);
void cmpr_release_reservations();

/* message of a failed cmpr_create() (no context yet), per thread */
std::string &cmpr_create_error();

inline int fail(cmpr_context *c, int code, const std::string &msg)
{
  if (c)
    c->err = msg;
  else
    cmpr_create_error() = msg;
  return code;
}

#define HIP_TRY(c, call)                                                        \
  do {                                                                          \
    hipError_t e_ = (call);                                                     \
    if (e_ != hipSuccess)                                                       \
      return fail((c), e_ == hipErrorOutOfMemory ? CMPR_ENOMEM : CMPR_EDEVICE,  \
                  std::string(#call) + ": " + hipGetErrorString(e_));           \
  } while (0)

template <typename T>
int dev_alloc(cmpr_context *c, DevBuf<T> &b, size_t n)
{
  b.release();
  if (n == 0)
    n = 1;
  HIP_TRY(c, hipMalloc((void **)&b.p, n * sizeof(T)));
  b.n = n;
  b.cap = n;
  return CMPR_OK;
}

/* a device temporary of one call: freed when the call returns, also when it fails */
template <typename T>
struct Tmp {
  DevBuf<T> b;
  ~Tmp() { b.release(); }
};

/* the header promises CMPR_ENOMEM, not an exception across the C boundary */
template <typename F>
int guarded(cmpr_context *c, F call)
{
  try {
    return call();
  } catch (const std::bad_alloc &) {
    return fail(c, CMPR_ENOMEM, "out of host memory");
  }
}

inline double ms_since(std::chrono::steady_clock::time_point t0)
{
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

/* 32-bit words summed or scanned as 64 bits (hipcub::TransformInputIterator) */
struct U32To64 {
  __host__ __device__ unsigned long long operator()(uint32_t v) const { return v; }
};

/* workgroups of wg lanes for n items, one lane each: 0 for n = 0 (the callers skip such a launch).  The one-argument
   blocks_for(n) that query_layout.hip and ref_index.hip keep for themselves answers 1 there. */
inline uint32_t blocks_for(uint64_t n, uint32_t wg)
{
  return (uint32_t)((n + wg - 1) / wg);
}

/* The host waits for a launch on a retired query set that may still run on a caller's stream
   (cmpr_context::pending_launch): called before anything such a launch reads or writes is overwritten,
   freed or reallocated. */
inline int cmpr_wait_previous_launch(cmpr_context *c)
{
  if (c->pending_launch) {
    HIP_TRY(c, hipEventSynchronize(c->pending_launch));
    c->pending_launch = nullptr;
  }
  return CMPR_OK;
}

/* compairr_hip.hip: cmpr_wait_previous_launch, then the question about the sticky overflow word of the
   retired set's unasked launches (CMPR_ESTATE when one overflowed) */
int cmpr_settle_previous_launch(cmpr_context *c);

/* like dev_alloc, but an allocation that is large enough is kept (contents undefined) */
template <typename T>
int dev_reserve(cmpr_context *c, DevBuf<T> &b, size_t n)
{
  if (n == 0)
    n = 1;
  if (b.p && b.cap >= n) {
    b.n = n;
    return CMPR_OK;
  }
  b.release();
  const size_t want = n + n / 16;
  HIP_TRY(c, hipMalloc((void **)&b.p, want * sizeof(T)));
  b.n = n;
  b.cap = want;
  return CMPR_OK;
}

template <typename T>
int dev_upload(cmpr_context *c, DevBuf<T> &b, const T *src, size_t n)
{
  int rc = dev_alloc(c, b, n);
  if (rc)
    return rc;
  if (n)
    HIP_TRY(c, hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return CMPR_OK;
}

/* hipFuncSetAttribute(MaxDynamicSharedMemorySize) / hipOccupancyMaxActiveBlocksPerMultiprocessor, remembered.
   The attribute of a function only ever grows: set when a request exceeds the largest so far, never lowered */
inline int raise_lds_limit(cmpr_context *c, const void *fn, size_t lds)
{
  size_t &raised = c->lds_raised[fn];
  if (lds <= 48 * 1024 || lds <= raised)
    return CMPR_OK;
  HIP_TRY(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  raised = lds;
  return CMPR_OK;
}

inline int occupancy_of(cmpr_context *c, const void *fn, int threads, size_t lds)
{
  auto it = c->occupancy_seen.find({fn, lds});
  if (it != c->occupancy_seen.end())
    return it->second;
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, threads, lds) != hipSuccess)
    occ = 0;
  (void)hipGetLastError();
  c->occupancy_seen[{fn, lds}] = occ;
  return occ;
}

inline bool is_f64_score(const cmpr_options &o)
{
  return o.score == CMPR_SCORE_RATIO && !o.ignore_counts;
}

/* pointer / size sanity of a set view (no pass over the data); on_device: the arrays are
   device memory, nothing of them is read here */
int validate_view(const cmpr_options &o, const cmpr_set_view *s, std::string &why, bool on_device = false);

/* query_layout.hip: upload set 1, validate it and lay it out for the kernels,
   all on the device (cmpr_set_queries) */
int cmpr_layout_queries(cmpr_context *c, const LayoutSource &src);

/* query_layout.hip: the records of a keyed share into the caller's buffer (cmpr_route_pack) */
int cmpr_route_pack_impl(cmpr_context *c, void *d_send, uint64_t capacity_bytes);

/* query_layout.hip: the caller's arrays into the given device buffers, validated
   there (what a host pass over the set would check); longest sequence and count
   total per repertoire.  on_device: the view holds device pointers -- offsets[0] and
   offsets[n] are fetched and checked before anything is allocated or copied, the rest
   is a copy inside the device.  *residues (or NULL) = offsets[n], the residues in all. */
int cmpr_upload_and_validate(cmpr_context *c, const cmpr_set_view *s, DevBuf<uint8_t> &res,
                             DevBuf<uint64_t> &off, DevBuf<uint32_t> &v, DevBuf<uint32_t> &j,
                             DevBuf<uint32_t> &rep, DevBuf<uint64_t> &cnt, uint32_t &longest,
                             std::vector<double> &rep_total, bool on_device = false,
                             uint64_t *residues = nullptr);

/* A set staged for one call: the caller's arrays on the device, validated, in temporaries of the call
   (cmpr_deduplicate*, cmpr_count_duplicates, cmpr_hamming_*; the resident reference keeps its own res2 .. cnt2) */
struct StagedSet {
  Tmp<uint8_t>  res;
  Tmp<uint64_t> off, cnt;
  Tmp<uint32_t> v, j, rep;
  uint64_t      n = 0;
  uint32_t      R = 0, longest = 0;
  std::vector<double> totals;      /* count total per repertoire */
};

/* the view checked (validate_view), the context's device made current, the set uploaded and validated into S */
inline int cmpr_stage_set(cmpr_context *c, const cmpr_set_view *s, bool on_device, StagedSet &S)
{
  std::string why;
  int rc;
  if ((rc = validate_view(c->opt, s, why, on_device)))
    return fail(c, rc, why);
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = cmpr_upload_and_validate(c, s, S.res.b, S.off.b, S.v.b, S.j.b, S.rep.b, S.cnt.b, S.longest, S.totals,
                                     on_device)))
    return rc;
  S.n = s->n;
  S.R = s->n_repertoires;
  return CMPR_OK;
}

/* An output array of one call.  The host variant of an entry point takes host arrays, its _device twin device
   arrays, and any of them may be NULL: this is the only place that tells the two apart.  `p` is what the kernels
   write -- the caller's device array, or after temp() a temporary of the call; copy_out() brings a temporary's
   contents to the caller's host array.  Everything is queued on the context's stream; nothing here waits. */
template <typename T>
struct Out {
  T *p;
  Out(T *caller, bool on_device)
      : p(on_device ? caller : nullptr), host(on_device ? nullptr : caller), asked(caller != nullptr) {}
  Out(const Out &) = delete;
  Out &operator=(const Out &) = delete;
  /* the caller asked for the array */
  bool wanted() const { return asked; }
  /* no device array of the caller's: a temporary of `count` elements for the kernels */
  int temp(cmpr_context *c, size_t count)
  {
    if (p)
      return CMPR_OK;
    int rc = dev_alloc(c, tmp.b, count);
    p = tmp.b.p;
    return rc;
  }
  /* ... or `d`, device memory of the call's that outlives the copy-out */
  void lend(T *d)
  {
    if (!p)
      p = d;
  }
  /* `count` elements to the caller's host array, when there is one */
  int copy_out(cmpr_context *c, size_t count)
  {
    if (host)
      HIP_TRY(c, hipMemcpyAsync(host, p, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return CMPR_OK;
  }
  /* `count` zeros in the caller's array: queued for a device array, written at once to a host array */
  int zero(cmpr_context *c, size_t count)
  {
    if (host)
      std::fill(host, host + count, T(0));
    else if (asked)
      HIP_TRY(c, hipMemsetAsync(p, 0, count * sizeof(T), c->stream));
    return CMPR_OK;
  }

private:
  T     *host;
  bool   asked;
  Tmp<T> tmp;
};

/* compairr_hip.hip: the synchronous step in link mode (cmpr_cluster, cluster.hip) -- every matching pair of the
   resident sets united in `parent` (one word per sequence, parent[i] == i or a forest that earlier steps
   left); the same run_step_and_wait loop as the other synchronous entry points */
int cmpr_link_step(cmpr_context *c, uint32_t *parent);

/* cluster.hip: what cmpr_cluster*, cmpr_cluster_table* (cluster.hip) and cmpr_hamming_cluster* (hamming.hip) share
   around their link steps -- the forest, the flat labels and sizes, the results of the plain call, the table pass.
   Everything is queued on the context's stream; only the last two wait. */
struct ClusterLinks {
  Tmp<uint32_t> parent;
  Tmp<unsigned long long> roots;
  Out<uint32_t> label, size;       /* of cmpr_cluster*: the caller's arrays; of the table calls: nobody's (NULL, NULL) */
  uint64_t n = 0;
  ClusterLinks(uint32_t *label_out, uint32_t *size_out, bool on_device)
      : label(label_out, on_device), size(size_out, on_device) {}
};
/* the four arrays of cmpr_cluster_table* / cmpr_hamming_cluster_table* */
struct ClusterTableOut {
  Out<uint32_t> cluster_of, member;
  Out<uint64_t> cluster_start, count;
  ClusterTableOut(uint32_t *cluster_of_out, uint64_t *cluster_start_out, uint32_t *member_out, uint64_t *count_out,
                  bool on_device)
      : cluster_of(cluster_of_out, on_device), member(member_out, on_device), cluster_start(cluster_start_out, on_device),
        count(count_out, on_device) {}
};
/* the forest of n sequences and the root counter allocated, parent[i] = i queued (n > 0) */
int cmpr_cluster_forest(cmpr_context *c, uint64_t n, ClusterLinks &L);
/* behind the links: L.label.p[i] = the root of i, the roots counted and (want_size) L.size.p[i] = the members of i's
   tree.  Labels that are no device array of the caller's go to a temporary, such sizes to where the forest was.
   Sets L.n. */
int cmpr_cluster_flatten(cmpr_context *c, uint64_t n, bool want_size, ClusterLinks &L);
/* the end of cmpr_cluster / cmpr_hamming_cluster: labels and sizes to the host (host variant), the cluster
   count; waits */
int cmpr_cluster_results(cmpr_context *c, ClusterLinks &L, uint64_t *n_clusters_out);
/* the table pass of cmpr_cluster_table / cmpr_hamming_cluster_table over flat labels and sizes (L.n == 0: only
   cluster_start[0] = 0).  d_cnt: the duplicate_count of every sequence on the device (not looked at with
   ignore_counts).  *flat_ms = the host time since t0 at the wait after which labels and sizes are flat;
   cl_ms[1] = the time from there. */
int cmpr_cluster_table_pass(cmpr_context *c, ClusterLinks &L, const uint64_t *d_cnt, ClusterTableOut &T,
                            uint64_t *n_clusters_out, std::chrono::steady_clock::time_point t0, double *flat_ms);

/* compairr_hip.hip: the synchronous step in neighbour mode (cmpr_neighbors, neighbors.hip).  hit == NULL: the
   count step, every match adds one to degree[its query]; otherwise the fill step, every match takes a place of
   its query's row in `hit` (kernels.h score_match) and, when `dist` is not NULL, writes the pair's distance to the
   same place of `dist` (cmpr_neighbors_distance).  `before` queues on the context's stream what EVERY attempt
   of run_step_and_wait needs in front of its kernels: the degrees zeroed, or set to the row lengths. */
int cmpr_neighbor_step(cmpr_context *c, uint32_t *degree, const uint64_t *row_start, uint32_t *hit, uint8_t *dist,
                       const std::function<int()> &before);

/* neighbors.hip: the edges of the resident sets for a caller inside the library (cmpr_existence_csr,
   existence.hip) -- the count step, the sum and the fill step of cmpr_neighbors into buffers of its own, the rows
   NOT put in order.  The caller has asked cmpr_check_ready and refused shards and routed sets.  With no edge,
   `hit` stays empty.  Everything is released with the struct. */
struct NeighborEdges {
  DevBuf<uint32_t> degree;             /* n1 + 1 words; all zero once the fill step has run */
  Out<uint64_t>    row_start;          /* n1 + 1: cmpr_neighbors' array, or nobody's (a temporary) */
  Out<uint32_t>    hit;                /* `total`: likewise */
  DevBuf<unsigned long long> census;   /* [0] rows of more than 64 hits, [1] of those the rows of more than 8192,
                                          [2] the longest of the latter; [3..4] two list counters, zero */
  DevBuf<char>     scan_tmp;
  size_t           scan_bytes = 0;
  bool             pretend_no_redo = false;
  uint64_t         total = 0, n_big = 0, n_long = 0, longest = 0;   /* rows of 65 .. 8192 | longer | the longest such */
  explicit NeighborEdges(uint64_t *row_start_out = nullptr, uint32_t *hit_out = nullptr, bool on_device = false)
      : row_start(row_start_out, on_device), hit(hit_out, on_device) {}
  ~NeighborEdges()
  {
    degree.release();
    census.release();
    scan_tmp.release();
  }
};
int cmpr_neighbor_edges(cmpr_context *c, NeighborEdges &e);

/* compairr_hip.hip: what every entry point on the resident sets asks first (CMPR_ESTATE without them) */
int cmpr_check_ready(cmpr_context *c);

/* ref_index.hip: cmpr_set_reference (on_device: the view holds device pointers) */
int cmpr_build_reference(cmpr_context *c, const cmpr_set_view *s, uint32_t longest_query, bool on_device);

/* variant 2, d = 1 (with or without -i): the filter holds pair rows (kernels_rows.h); so does
   that of nucleotides at d = 2 when kernels_pairs2.h probes it */
inline bool pair_rows(const cmpr_context *c)
{
  return c->rows && (c->opt.differences == 1 || c->d2pairs);
}

#endif
