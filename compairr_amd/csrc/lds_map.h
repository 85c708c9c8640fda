/*
 * lds_map.h -- what lies where in the dynamic LDS of the probe and resolve kernels: one map per
 * kernel, read by make_plan (the launch's allocation) and by the index build (what a slice may
 * take).  The kernels still walk their regions with a chain of casts, in the map's order: a new
 * region is added here and in that chain, nowhere else (DESIGN.md 4.12 says why the chains stayed).
 * Plain C++17: compiles without hipcc (tests/test_lds_map_cpu.py).
 */
#ifndef COMPAIRR_AMD_LDS_MAP_H
#define COMPAIRR_AMD_LDS_MAP_H

#include "layout.h"

namespace cmpr {

constexpr uint32_t LDS_BYTES = 160 * 1024;      /* of a CU, and the most one workgroup may take */

/* ---- what the maps take the size of ---- */

constexpr int QCAP = 2 * WAVE;      /* per-wave queue of Bloom positives   */

struct WaveQueue {
  uint64_t hash[QCAP];
  uint32_t slot[QCAP];   /* query: tile * 64 + lane                          */
  uint32_t ca[QCAP];     /* kind | p1 << 3 | r1 << 24                        */
  uint32_t cb[QCAP];     /* p2 | r2 << 24                                    */
  uint32_t m[QCAP];      /* variant 2 (kernels_rows.h q_push): the entry's mask of positive variants */
};

/* (query, variant, set-2 sequence) triples whose table key equals the variant
   hash, waiting for verification -- one queue per wave, in LDS */
struct CandQueue {
  uint32_t slot[QCAP], ca[QCAP], cb[QCAP];
  uint32_t tagb[QCAP];                 /* the key's bucket | its tag << 17 ... (see verify_candidate) */
  uint32_t piece[QCAP];                /* the table slot to look at */
  uint32_t bucket[QCAP];
};
static_assert(sizeof(CandQueue) <= sizeof(WaveQueue), "the d = 0 kernel keeps a CandQueue where the others keep a WaveQueue");

constexpr uint32_t RING = 4;        /* probe_rows_kernel: slice buffers of a workgroup */

/* one buffer of the ring */
struct RingSlot {
  /* tag << 32 | ntiles << 16 | tiles handed out: claimed with ONE 64-bit LDS add,
     so that a claim names the tenant it belongs to; tag 0 = nothing yet, tags
     grow by one per tenant, RING_END = no more chunks */
  unsigned long long claim;
  uint32_t done;             /* tiles of the tenant finished */
  uint32_t slice, pass;
  uint32_t first;            /* class-row chunk: its first item (blocks of 64 items, no tile refs) */
  uint32_t pad[2];           /* ([0] of slot 0: the workgroup's staging counter; [0] of slot 1: buffers whose
                                chain of tenants has ended; [1]: item chunk: its blocks) */
  uint32_t next_chunk;       /* the chunk of the tenant after this one (P.deal: reserved when this one was staged) */
  uint32_t page;             /* the page of its slice the tenant holds | e of the slice << 4 (layout.h SliceGeom; 0: no pages) */
};

constexpr uint32_t P2_PZ = 20;                   /* pair-blank keys per pair: (qa, qb) -> qa | qb << 2; 16 + qa: no second position */

/* probe_pairs2_kernel: chunk descriptor and unit counter of one slice buffer */
struct P2Slot {
  uint32_t slice, first, ntiles, pass;
  uint32_t next_unit, units, pad[2];
};

/* keys per position of probe_rows_kernel's LDS copy of the Zobrist table: d = 2 stores a row twice
   (rotated reads); pair rows add a ZERO key for code A -- the residue code the layout pads
   a query with behind its end (query_layout.hip fill_tiles_kernel), so that a pair that
   hangs over the end hashes, and reads, without a test */
__host__ __device__ constexpr uint32_t zs_of(int A, int D, bool pairs)
{
  return D == 2 ? 2u * (uint32_t)A : (pairs ? (uint32_t)A + 1u : (uint32_t)A);
}

/* ---- the maps: byte offset of every region from LDS address 0, in the order they lie, and the
   end of the last one (64 bits: a table far too long for any LDS still compares as too long) ---- */

struct LdsCursor {
  uint64_t at = 0;
  __host__ __device__ uint64_t take(uint64_t n, uint64_t size)     /* n elements of `size` bytes */
  {
    const uint64_t o = at;
    at += n * size;
    return o;
  }
};

/* probe_kernel (variant 0; kernels.h) */
struct DirectLds {
  uint64_t zl;         /* A x zpos Zobrist position keys (d = 0: room kept, nothing copied -- the layout hashed) */
  uint64_t mat;        /* `cells` u64: the workgroup's copy of the matrix (0: none kept) */
  uint64_t queues;     /* one WaveQueue per wave (d = 0: a CandQueue in its place) */
  uint64_t bytes;
};
__host__ __device__ inline DirectLds direct_lds_map(uint32_t A, uint32_t zpos, uint32_t waves, uint32_t cells)
{
  LdsCursor c;
  DirectLds m;
  m.zl = c.take((uint64_t)A * zpos, sizeof(uint64_t));
  m.mat = c.take(cells, sizeof(unsigned long long));
  m.queues = c.take(waves, sizeof(WaveQueue));
  m.bytes = c.at;
  return m;
}

/* resolve_kernel (kernels.h) */
struct ResolveLds {
  uint64_t queues;     /* one CandQueue per wave */
  uint64_t mat;        /* `cells` u64: the workgroup's copy of the matrix (0: none kept) */
  uint64_t bytes;
};
__host__ __device__ inline ResolveLds resolve_lds_map(uint32_t waves, uint32_t cells)
{
  LdsCursor c;
  ResolveLds m;
  m.queues = c.take(waves, sizeof(CandQueue));
  m.mat = c.take(cells, sizeof(unsigned long long));
  m.bytes = c.at;
  return m;
}

/* probe_sliced_kernel (variant 1; kernels_sliced.h) */
struct SlicedLds {
  uint64_t slice;      /* the staged Bloom slice, 2^words_log2 u64 -- at LDS address 0: its reads need no base add */
  uint64_t zl;         /* zrow_stride(A) x zpos keys: amino acids store every row of keys twice in a line, so that
                          "residue (r + k) mod A" is entry r + k (row_lds_others) */
  uint64_t ze;         /* zdelta_entries(A) x zpos: nucleotides, per position and residue r the keys {Z[r],
                          Z[r]^Z[r+1], Z[r]^Z[r+2], Z[r]^Z[r+3]} (residues mod 4) */
  uint64_t mat;        /* `cells` u64: the workgroup's copy of the matrix (0: none kept) */
  uint64_t queues;     /* one WaveQueue per wave */
  uint64_t cr;         /* CR tables: MAX_CLASS_RES x A u32 */
  uint64_t hv;         /* heavy-class bitmap: HEAVY_WORDS u32 (room kept without -i too) */
  uint64_t bcast;      /* 4 u32: the chunk claimed, tiles of it handed out */
  uint64_t tref;       /* chunk_cap TileRefs: the tiles of the chunk */
  uint64_t bytes;
};
__host__ __device__ inline SlicedLds sliced_lds_map(uint32_t A, uint32_t zpos, uint32_t waves, uint32_t words_log2,
                                                    uint32_t cells, uint32_t chunk_cap)
{
  LdsCursor c;
  SlicedLds m;
  m.slice = c.take((uint64_t)1 << words_log2, sizeof(uint64_t));
  m.zl = c.take((uint64_t)zrow_stride((int)A) * zpos, sizeof(uint64_t));
  m.ze = c.take((uint64_t)zdelta_entries((int)A) * zpos, sizeof(uint64_t));
  m.mat = c.take(cells, sizeof(unsigned long long));
  m.queues = c.take(waves, sizeof(WaveQueue));
  m.cr = c.take(MAX_CLASS_RES * A, sizeof(uint32_t));
  m.hv = c.take(HEAVY_WORDS, sizeof(uint32_t));
  m.bcast = c.take(4, sizeof(uint32_t));
  m.tref = c.take(chunk_cap, sizeof(TileRef));
  m.bytes = c.at;
  return m;
}

/* probe_rows_kernel (variant 2; kernels_rows.h).  No copy of the matrix: the fast form scores nothing --
   resolve_kernel does -- and the form that resolves inline, the rare path, adds to the matrix where it lies. */
struct RowsLds {
  uint64_t slices;     /* RING slice buffers, rw_words x 32 B each (a multiple of 1 KiB: LDS-DMA pieces) -- at LDS
                          address 0: the slices are read at absolute addresses */
  uint64_t zl;         /* keys_per_pos (zs_of) x zpos Zobrist keys */
  uint64_t queues;     /* one WaveQueue per wave */
  uint64_t cr;         /* CR tables: MAX_CLASS_RES x A u32 */
  uint64_t hv;         /* -i: heavy-class bitmap, HEAVY_WORDS u32 */
  uint64_t ring;       /* RING RingSlots */
  uint64_t tref;       /* RING x chunk_cap TileRefs, copied in by LDS-DMA */
  uint64_t gk;         /* record tiles: the gene keys, u64 (the kernel works a tile's hashes out itself) */
  uint64_t cb;         /* record tiles with -i: the class tables in front of the class-residue rows -- CL | CV | CJ --,
                          u32 (a record tile works the query's class key out itself) */
  uint64_t bytes;
};
__host__ __device__ inline RowsLds rows_lds_map(uint32_t A, uint32_t keys_per_pos, uint32_t zpos, uint32_t waves,
                                                uint32_t rw_words, bool indels, uint32_t chunk_cap,
                                                uint32_t gene_keys, uint32_t class_words)
{
  LdsCursor c;
  RowsLds m;
  m.slices = c.take((uint64_t)RING * rw_words, ROW_WORD_BYTES);
  m.zl = c.take((uint64_t)keys_per_pos * zpos, sizeof(uint64_t));
  m.queues = c.take(waves, sizeof(WaveQueue));
  m.cr = c.take(MAX_CLASS_RES * A, sizeof(uint32_t));
  m.hv = c.take(indels ? HEAVY_WORDS : 0u, sizeof(uint32_t));
  m.ring = c.take(RING, sizeof(RingSlot));
  m.tref = c.take((uint64_t)RING * chunk_cap, sizeof(TileRef));
  m.gk = c.take(gene_keys, sizeof(uint64_t));
  m.cb = c.take(class_words, sizeof(uint32_t));
  m.bytes = c.at;
  return m;
}

/* probe_pairs2_kernel (nucleotides, d = 2, pair rows; kernels_pairs2.h) */
struct Pairs2Lds {
  uint64_t slices;     /* nbuf (1 or 2) slice buffers, rw_words x 32 B each -- at LDS address 0 */
  uint64_t ze;         /* 16 x zpos keys: per position and residue, own key and 3 replacement deltas */
  uint64_t pz;         /* P2_PZ x ceil(zpos / 2) pair-blank keys */
  uint64_t mat;        /* `cells` u64: the workgroup's copy of the matrix (0: none kept) -- the positives that do not
                          fit their buffer are resolved here, by the slow inline form */
  uint64_t queues;     /* one WaveQueue per wave */
  uint64_t cr;         /* CR tables: MAX_CLASS_RES x 4 u32 */
  uint64_t slots;      /* 2 P2Slots: {chunk descriptor, unit counter} */
  uint64_t tref;       /* 2 x chunk_cap TileRefs, copied in by LDS-DMA */
  uint64_t bytes;
};
__host__ __device__ inline Pairs2Lds pairs2_lds_map(uint32_t zpos, uint32_t waves, uint32_t nbuf, uint32_t rw_words,
                                                    uint32_t cells, uint32_t chunk_cap)
{
  LdsCursor c;
  Pairs2Lds m;
  m.slices = c.take((uint64_t)nbuf * rw_words, ROW_WORD_BYTES);
  m.ze = c.take(16 * (uint64_t)zpos, sizeof(uint64_t));
  m.pz = c.take(P2_PZ * (((uint64_t)zpos + 1) / 2), sizeof(uint64_t));
  m.mat = c.take(cells, sizeof(unsigned long long));
  m.queues = c.take(waves, sizeof(WaveQueue));
  m.cr = c.take(MAX_CLASS_RES * 4, sizeof(uint32_t));
  m.slots = c.take(2, sizeof(P2Slot));
  m.tref = c.take(2 * (uint64_t)chunk_cap, sizeof(TileRef));
  m.bytes = c.at;
  return m;
}

/* ---- the index build's estimates (cmpr_build_reference): the maps at worst-case arguments -- a matrix
   copy of 2048 cells, -i.  Where an argument is larger than the kernel's own, it is the
   estimate's number from before there was a map, kept so that no set changes its slices. ---- */
constexpr uint32_t EST_CELLS = 2048;                       /* the largest matrix copy (make_plan: lds_matrix) */
constexpr uint32_t EST_CHUNK_CAP = 64;                     /* tile references per chunk: chunk_tiles goes up to 512 and make_plan charges it */
constexpr uint32_t EST_ROWS_CHUNK_CAP = EST_CHUNK_CAP + EST_CHUNK_CAP / RING;   /* one chunk's references more than the ring's RING x 64 (variant 1's list was charged as well) */
constexpr uint32_t EST_ROWS_CLASS_WORDS = 4;               /* variant 1's 16 bytes of chunk broadcast, which the rows kernel has not (gene keys and class tables of record tiles: not charged) */
constexpr uint32_t EST_P2_CHUNK_CAP = EST_CHUNK_CAP + 17;  /* 2 x 17 references = 1088 bytes: slots charged at 64 bytes for P2Slot's 32, and 1024 of slack */

inline uint64_t sliced_lds_estimate(uint32_t A, uint32_t zpos, uint32_t words_log2)
{
  return sliced_lds_map(A, zpos, 4, words_log2, EST_CELLS, EST_CHUNK_CAP).bytes;
}
/* (2 * A keys per position: the kernel's is zs_of(), A + 1 at d = 1 with pair rows; no matrix copy) */
inline uint64_t rows_lds_estimate(uint32_t A, uint32_t zpos, uint32_t waves, uint32_t slice_words)
{
  return rows_lds_map(A, 2 * A, zpos, waves, slice_words, true, EST_ROWS_CHUNK_CAP, 0, EST_ROWS_CLASS_WORDS).bytes;
}
/* (the pair count was halved after multiplying: half a pair's keys more at even zpos, charged as cells) */
inline uint64_t pairs2_lds_estimate(uint32_t zpos, uint32_t nbuf, uint32_t slice_words)
{
  return pairs2_lds_map(zpos, 16, nbuf, slice_words, EST_CELLS + (zpos % 2 == 0 ? P2_PZ / 2 : 0), EST_P2_CHUNK_CAP).bytes;
}

}  // namespace cmpr
#endif
