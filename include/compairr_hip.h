/*
 * compairr_hip.h -- C ABI of libcompairr_hip.so, the MI355X (gfx950) drop-in
 * for CompAIRR's repertoire-overlap hot path.
 *
 * The reference has no FFI layer; its narrowest seam for this path is the
 * launch of sim_thread inside overlap() (/root/reference/src/overlap.cc:926-936):
 * everything before it (AIRR-TSV parse, db accessors) is the input, everything
 * after it (matrix dump, overlap.cc:944-1039) the output.  The entry points
 * below are what a binding at that seam needs; each cites the reference
 * interface it replaces.  Plain pointers and sizes only, no C++/torch types.
 *
 * Threading: a context is used from one host thread at a time; distinct
 * contexts are independent (no process-global state, unlike the file-static
 * state at overlap.cc:24-53).
 *
 * Ownership: the caller owns every array it passes in and the output matrix;
 * arrays may be freed as soon as the call that received them returns.  The
 * library owns all device memory; nothing is retained after cmpr_destroy().
 *
 * Errors: every int-returning function returns 0 on success and a non-zero
 * CMPR_E* code otherwise; cmpr_last_error() then gives the message.  The
 * reference convention (fatal(): "\nError: %s\n" + exit(1), util.cc:84-88) is
 * applied by the host program, not here.
 */
#ifndef COMPAIRR_HIP_H
#define COMPAIRR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Counts INCOMPATIBLE changes: entry points and tunables added since (cmpr_deduplicate*, cmpr_cluster*, cmpr_neighbors*, cmpr_neighbors_distance*, cmpr_existence_csr*, cmpr_cluster_table*, cmpr_hamming_matrix*, cmpr_hamming_neighbors*, cmpr_hamming_cluster*, cmpr_hamming_cluster_table*, cmpr_hamming_nearest*, cmpr_edit_neighbors*, cmpr_edit_matrix*, cmpr_edit_cluster*, cmpr_edit_cluster_table*, cmpr_edit_nearest*, cmpr_tcrdist_neighbors*, cmpr_tcrdist_matrix*) break
   no caller and leave it as it is. */
#define CMPR_ABI_VERSION 5

enum {
  CMPR_OK          = 0,
  CMPR_EINVAL      = 1,   /* illegal option / argument combination          */
  CMPR_ENOMEM      = 2,   /* host or device allocation failed               */
  CMPR_EDEVICE     = 3,   /* HIP runtime error (message has the HIP string) */
  CMPR_EUNSUPPORTED= 4,   /* legal for the reference, not on this path      */
  CMPR_ESTATE      = 5    /* calls out of order                             */
};

/* -s / --score, same numbering as the reference enum (compairr.h:125-135) */
enum {
  CMPR_SCORE_PRODUCT = 0,
  CMPR_SCORE_RATIO   = 1,
  CMPR_SCORE_MIN     = 2,
  CMPR_SCORE_MAX     = 3,
  CMPR_SCORE_MEAN    = 4,
  CMPR_SCORE_MH      = 5,
  CMPR_SCORE_JACCARD = 6
};

/*
 * The process-global opt_* flags the loop reads (compairr.h:139-162), as a POD.
 */
typedef struct cmpr_options {
  int32_t  differences;     /* opt_differences, 0..2 on this path             */
  int32_t  indels;          /* opt_indels (requires differences == 1)         */
  int32_t  ignore_genes;    /* opt_ignore_genes                               */
  int32_t  ignore_counts;   /* opt_ignore_counts                              */
  int32_t  score;           /* opt_score_int, CMPR_SCORE_*                    */
  int32_t  alphabet_size;   /* alphabet_size: 20 (aa) or 4 (-n)               */
  uint32_t n_v_genes;       /* db_get_v_gene_count() (db.cc:1018)             */
  uint32_t n_j_genes;       /* db_get_j_gene_count() (db.cc:1023)             */
  int32_t  device;          /* HIP device ordinal; -1 = current device        */
  int32_t  existence;       /* opt_existence (-x): matrix rows are the set-1
                               SEQUENCES, in input order (overlap.cc:226)       */
  int32_t  reserved[6];     /* must be zero                                   */
} cmpr_options;

/*
 * What the loop reads of a repertoire set through db_getsequence /
 * db_getsequencelen / db_get_v_gene / db_get_j_gene / db_get_count /
 * db_get_repertoire_id_no (db.cc:964-997), as structure-of-arrays in HOST
 * memory.  Residues are the reference's codes (map_aa / map_nt, db.cc:33-71),
 * not ASCII.
 */
typedef struct cmpr_set_view {
  uint64_t        n;              /* number of sequences                      */
  const uint8_t  *residues;       /* offsets[n] residue codes, concatenated   */
  const uint64_t *offsets;        /* n + 1 entries, offsets[0] == 0           */
  const uint32_t *v_gene;         /* n; may be NULL when ignore_genes         */
  const uint32_t *j_gene;         /* n; may be NULL when ignore_genes         */
  const uint32_t *repertoire;     /* n; values < n_repertoires                */
  const uint64_t *count;          /* n; >= 1; may be NULL when ignore_counts  */
  uint32_t        n_repertoires;
  uint32_t        reserved;
} cmpr_set_view;

/* Work and timing of the last cmpr_overlap_* call. */
typedef struct cmpr_stats {
  uint64_t queries;            /* set-1 sequences processed                   */
  uint64_t variants;           /* variant hashes held against the Bloom filter
                                  (executed tests, counted by the kernel)      */
  uint64_t bloom_positive;     /* probes that passed the Bloom filter         */
  uint64_t hash_equal;         /* hash slots equal to a variant hash          */
  uint64_t matches;            /* verified (query, hit) pairs                 */
  uint64_t algorithmic_bytes;  /* sum over queries of (L + 20) + 8 * V(L)     */
  double   kernel_ms;          /* HIP-event time of probe + resolve kernels   */
  double   total_ms;           /* first launch -> matrix ready on the stream  */
  uint32_t kernel_launches;
  uint32_t reserved;
  double   probe_ms;           /* HIP-event time of the probe kernel alone    */
  uint64_t filter_reads;       /* filter words read for those tests: one per
                                  variant (kernel variants 0, 1), one per ROW of
                                  up to alphabet_size variants (variant 2)      */
} cmpr_stats;

typedef struct cmpr_context cmpr_context;

/* ABI version of the loaded library (== CMPR_ABI_VERSION it was built with). */
int cmpr_abi_version(void);

/*
 * Create a context on one device.  Replaces the option globals + the
 * zobrist_init() call (overlap.cc:840, zobrist.cc:28-67).
 */
int cmpr_create(const cmpr_options *options, cmpr_context **out);

/* Frees device memory and the context (bloom_exit/hash_exit/zobrist_exit,
   overlap.cc:1044-1049).  NULL is a no-op. */
void cmpr_destroy(cmpr_context *ctx);

/* Message of the last failed call on this context ("" if none).  With
   ctx == NULL: message of the last failed cmpr_create() on this thread. */
const char *cmpr_last_error(const cmpr_context *ctx);

/*
 * Upload set 2 and build its index on the device: per-sequence Zobrist hash
 * (db_hash, db.cc:903-916), hash table + Bloom filter inserts (hash_init,
 * bloom_init, hash_insert loop, overlap.cc:861-873).  Every entry is inserted,
 * duplicates included.  `longest_query` is the longest set-1 sequence that
 * will be submitted (the Zobrist table needs max(longest1, longest2) + 3
 * positions, overlap.cc:840); pass 0 to size it from this set alone, in which
 * case later longer queries make cmpr_set_queries() fail with CMPR_EINVAL.
 *
 * Footprint: the record table holds one 64-byte slot per BUCKET, buckets = 2^table_log2_delta x the
 * smallest power of two >= n / 0.7 (hashtable.cc:24, 36-38) -- 183 to 366 bytes per reference sequence at
 * the default delta of 1 (10M: 2 GiB; 100M: 32 GiB) --, the row filter 2 bytes per residue position + 2 per
 * sequence (twice that with -i), the set itself ~45 bytes per sequence.  "table_log2_delta" = 0 halves the table.
 *
 * Size: at most 2^32-64 sequences (pair lists hold uint32 sequence numbers) and device memory.  A set whose
 * record table would exceed 2^"part_buckets_log2" buckets (default 2^30: ~375M sequences at delta 1) is
 * indexed in PARTS -- contiguous sequence ranges, as few as the cap allows or the count with the fewest
 * table bytes in all -- that share everything the query layout reads (Zobrist keys, class geometry, slice
 * count, pages) and differ in their filter words, record table and bucket bitmap; each part's filter is as
 * large as the whole set's.  Every cmpr_overlap_* call then makes one pass of its kernels per part, in
 * stream order, into the same matrix; cmpr_stats counts summed over the passes (`variants` and
 * `filter_reads` once per part).  "reference_parts" says how many are in effect.  Work shards compose
 * with parts: each context does its share of the slices for every part.  Beyond memory, CMPR_ENOMEM.
 */
int cmpr_set_reference(cmpr_context *ctx, const cmpr_set_view *set2,
                       uint32_t longest_query);

/*
 * Upload set 1 (the queries) and lay it out for the kernel.  Per call: at most 2^31-1 sequences, and the
 * layout's 32-bit counts and positions must hold -- fewer than 2^32 query slots (64 per tile; tiles are
 * padded per (slice, length) group, read-only tunable "query_slots"), 2^32 four-byte words of laid-out
 * residues, 2^32 class-item slots, 2^31 chunks and 2^31 (slice, length) groups --, else CMPR_EUNSUPPORTED
 * ("too many ..." / "... 32-bit ...").  Slots, residue words and chunks grow with the set plus a padding of
 * up to one tile per (slice, length) group, and the slice count comes from the reference: no set size is
 * accepted against every reference, so the bound is these checks, not a number.  Calls are independent: a larger set is handed over in contiguous batches whose matrices add up (-x rows and pair
 * lists number the sequences of the batch) -- bin/compairr halves a batch the layout refuses for its size.
 * After this call
 * the queries are resident in HBM; cmpr_overlap_* may be called repeatedly.
 * Passing the same view as set 2 gives the reference's one-file mode
 * (overlap.cc:799-825).  The context keeps its device allocations from call to
 * call (a second set of similar size costs no allocation).  With the work-shard
 * tunables set, only what this context works on is laid out (the queries are still
 * uploaded and keyed in full; cmpr_route_queries below divides that too).
 */
int cmpr_set_queries(cmpr_context *ctx, const cmpr_set_view *set1);

/*
 * The same two calls for sets that already live in HBM (a parser that writes to the
 * device, a previous stage of a pipeline, another library): every pointer of the view is
 * a DEVICE pointer on the context's device, same types and meaning as above.  Nothing
 * crosses PCIe but two offsets (offsets[0], offsets[n]) and the layout's sizes; the set is
 * validated on the device like a host set.  The reference set is copied (the library keeps
 * its own arrays); the query arrays are read where they lie during the call and may be
 * freed or overwritten once it has returned.  (The reference reads both sets where db.cc
 * left them, db.cc:964-997 -- this is that, for a caller whose "where" is the GPU.)
 */
int cmpr_set_reference_device(cmpr_context *ctx, const cmpr_set_view *d_set2,
                              uint32_t longest_query);
int cmpr_set_queries_device(cmpr_context *ctx, const cmpr_set_view *d_set1);

/*
 * Multi-GPU layout of ONE query set over N contexts (one per GPU, tunables
 * work_shard_count = N, work_shard_index = 0..N-1, the same reference set in each).
 * The reference hands chunks of 1000 queries to its threads (overlap.cc:421-433) and
 * sums their private matrices (overlap.cc:510-527); here the contexts divide the WORK of a
 * step by filter slice, and the queries go where their work is:
 *
 *   1. every context is given ANY share of the set (e.g. the i-th N-th of it):
 *      cmpr_route_queries() uploads and keys that share and says how many records go to
 *      each of the n_dest contexts (counts_out[n_dest]; a query goes to the context that
 *      works on its slice and to those that work on one of its class-position items --
 *      1 to 2 destinations on CDR3 amino acids), the size of a record (*record_bytes_out,
 *      a multiple of 16) and, if rep_totals_out is not NULL, the duplicate_count total
 *      per repertoire of the share (n_repertoires doubles; summed over the shares they
 *      bound the cells of the final matrix);
 *   2. cmpr_route_pack() writes those records into a DEVICE buffer of the caller, grouped
 *      by destination (destination d's run starts at record counts[0] + .. + counts[d-1]);
 *   3. the caller moves the runs to their destinations -- one all-to-all over xGMI (RCCL)
 *      or, inside one process, device-to-device copies;
 *   4. every context receives with cmpr_set_queries_routed(): n_records records in device
 *      memory (in any order), the number of repertoires and of sequences of the WHOLE set,
 *      and optionally the summed totals of step 1 (NULL: this context's own share bounds
 *      its own matrix only).
 * After step 4 the context holds exactly what it works on; cmpr_overlap_* gives its part of
 * the matrix, the parts add up to the whole (one sum-reduce), pair lists and -x rows carry
 * the sequence numbers of the whole set (first_index + position in the share).
 * Uploads and layout work divide by N; no context ever sees the whole set.
 */
int cmpr_route_queries(cmpr_context *ctx, const cmpr_set_view *share, uint64_t first_index,
                       uint32_t n_dest, uint64_t *counts_out, uint32_t *record_bytes_out,
                       double *rep_totals_out);
int cmpr_route_pack(cmpr_context *ctx, void *d_send, uint64_t capacity_bytes);
int cmpr_set_queries_routed(cmpr_context *ctx, const void *d_records, uint64_t n_records,
                            uint32_t n_repertoires, uint64_t n_total, const double *rep_totals);

/*
 * The per-query loop (sim_thread / process_variants / find_variant_matches,
 * overlap.cc:376-538, 253-284, 168-251).  Writes the R1 x R2 matrix,
 * row = set-1 repertoire number (with options.existence: R1 = number of set-1
 * sequences, row = sequence number), column = set-2 repertoire number
 * (overlap.cc:222-226), as exact integer sums:
 *   product, MH : sum of count1 * count2
 *   min, Jaccard: sum of min;  max: sum of max;  -f: number of pairs
 *   mean        : sum of (count1 + count2), i.e. TWICE the reference's cell
 * The matrix is overwritten, not accumulated into.  Host-memory output.
 * CMPR_SCORE_RATIO is not an integer sum: use cmpr_overlap_matrix_f64().
 */
int cmpr_overlap_matrix(cmpr_context *ctx, uint64_t *matrix_out);

/* Same loop, double-precision cells; the only form that supports ratio
   (order-dependent rounding, as in the threaded reference, overlap.cc:510-527). */
int cmpr_overlap_matrix_f64(cmpr_context *ctx, double *matrix_out);

/*
 * Same loop, result left in DEVICE memory: `d_matrix` points to
 * R1 * R2 uint64 on the context's device (e.g. a buffer a collective library
 * will reduce across GPUs).  The kernels are enqueued on `stream`
 * (a hipStream_t, NULL = the context's own stream) and the call returns
 * without synchronising when `stream` is not NULL.
 *
 * Launches of one context are ordered one after the other whatever streams they are
 * given (each uses state the previous one leaves behind; the library inserts the
 * event wait when the stream changes).
 *
 * Because this entry point does not wait, it cannot look at the one condition that
 * can invalidate a launch after the fact: amino acids with d >= 1 drop their redo
 * pass once a finished launch on the same sets has shown that the positives buffer
 * has room to spare; should a later launch overflow all the same, its matrix is
 * incomplete.  The device records that; the next cmpr_get_stats() then fails with
 * CMPR_ESTATE ("... overflowed in a launch without redo pass"), withdraws the
 * shortcut, and later launches carry the redo pass again.  Callers of this entry
 * point must therefore call cmpr_get_stats() before trusting a series of launches.
 * The synchronous entry points (cmpr_overlap_matrix, _f64, _pairs) check by
 * themselves and repeat the step with the redo pass: they never return such a result
 * (and a synchronous call that comes between such a launch and the question does not
 * take the answer away: cmpr_get_stats() still fails once).
 */
int cmpr_overlap_matrix_device(cmpr_context *ctx, void *d_matrix, void *stream);

/*
 * The matching (query, hit) pairs themselves -- what the reference appends to
 * its pairs list in find_variant_matches (overlap.cc:232-245) and prints with
 * -p/--pairs (overlap.cc:455-507).  Runs the same loop; up to `capacity` pairs are
 * written (query_out[k] = index into the set given to cmpr_set_queries,
 * hit_out[k] = index into the reference set; order unspecified, as in the
 * reference, README.md:163), *count_out = number of pairs found.  When
 * *count_out > capacity the arrays hold an arbitrary subset: call again with a
 * larger capacity (cmpr_stats.matches of a previous cmpr_overlap_matrix() call is
 * the exact number).  capacity == 0 with NULL arrays only counts.
 */
int cmpr_overlap_pairs(cmpr_context *ctx, uint64_t capacity, uint32_t *query_out,
                       uint32_t *hit_out, uint64_t *count_out);

/*
 * The same pairs as neighbour lists in CSR: who matched whom, per query, in order.  The edge set is exactly what
 * cmpr_overlap_pairs() lists for the resident sets under the context's options -- the pairs of
 * find_variant_matches (overlap.cc:232-245), the (i, i) pairs included when one set is resident as both; the call
 * filters nothing.  n1 is the n of the last cmpr_set_queries*().
 *   row_start_out[n1 + 1]  row_start[0] == 0, row_start[i + 1] - row_start[i] = the number of hits of query i.
 *                          Always written in full and always exact, whatever `capacity` is.  May be NULL when
 *                          only *n_edges_out is wanted.
 *   hit_out[capacity]      row i occupies [row_start[i], row_start[i + 1]): sequence numbers of the reference
 *                          set in strictly increasing order.  When there are more edges than `capacity`, NOTHING
 *                          is written here (cmpr_overlap_pairs() writes an arbitrary subset; this call does not):
 *                          the call still returns CMPR_OK with *n_edges_out > capacity, and row_start says what
 *                          to allocate.  capacity == 0 with hit_out == NULL is the degree-only call: one step, no
 *                          sort.  capacity > 0 with hit_out == NULL is CMPR_EINVAL.
 *   *n_edges_out           required (NULL: CMPR_EINVAL), a HOST pointer in both variants; == row_start[n1] ==
 *                          cmpr_stats.matches of the step.  cmpr_get_stats() afterwards describes the last step
 *                          the call ran.
 * cmpr_neighbors_device() takes both arrays as device memory on the context's device and writes only the
 * elements named above; only the edge count crosses PCIe.
 *
 * Results are bit-identical from run to run, under every tunable, and with set 2 indexed in parts.  The call
 * counts the hits per query in one step, sums the counts into row_start, runs the step again to put every hit
 * into its row, and sorts each row in place (compairr_amd/csrc/neighbors.hip): two steps where
 * cmpr_overlap_pairs() runs one, and no per-edge memory beyond the caller's hit_out (the host variant holds the
 * two arrays on the device for the duration of the call).  Temporaries: 4 bytes per query, the scratch of the
 * sum, 4 bytes per row of more than 64 hits, and for rows of more than 8192 hits 24 bytes each plus the longest
 * of them once.  Everything is freed before the call returns, also when it fails.
 *
 * Synchronous; needs both resident sets (CMPR_ESTATE as for cmpr_overlap_matrix()).  With the tunable
 * work_shard_count above 1, and after cmpr_set_queries_routed(), the call is CMPR_EUNSUPPORTED: such a context
 * holds part of each row, and rows do not add up by a sum.  options.existence and the scores play no part.  The
 * resident sets, the plan and the other entry points are as usable afterwards as before; the call may be
 * repeated.  An empty query set is CMPR_OK with row_start == {0} and no edges.
 */
int cmpr_neighbors(cmpr_context *ctx, uint64_t capacity,
                   uint64_t *row_start_out, uint32_t *hit_out, uint64_t *n_edges_out);
int cmpr_neighbors_device(cmpr_context *ctx, uint64_t capacity,
                          uint64_t *d_row_start_out, uint32_t *d_hit_out, uint64_t *n_edges_out);

/*
 * The neighbour lists with the distance of every edge: the `distance` column of the reference's --pairs --distance
 * (overlap.cc:491-502) beside each hit.  Everything said of cmpr_neighbors[_device]() holds word for word -- the
 * same edge set, the same row_start, strictly increasing rows, *n_edges_out == row_start[n1] ==
 * cmpr_stats.matches, the same state checks and CMPR_EUNSUPPORTED cases, an empty query set is CMPR_OK, results
 * bit-identical from run to run, under every tunable and with set 2 in parts, every temporary freed on every
 * return -- and in addition:
 *   distance_out[capacity]  distance_out[k] belongs to the pair (row of k, hit_out[k]): the number of positions at
 *                           which the two sequences differ when they have one length, and 1 otherwise.  0 ..
 *                           options.differences, so 0, 1 or 2.  One d = 2 call therefore holds the graphs at
 *                           d <= 0, <= 1 and <= 2, and the weights of an edge-weighted network.
 * The capacity protocol covers both arrays: with more edges than `capacity` NOTHING is written to hit_out or
 * distance_out; capacity == 0 with both NULL is the degree-only call (one step, no sort); capacity > 0 with either
 * of them NULL is CMPR_EINVAL, and cmpr_last_error() names the missing argument.  Elements behind the last edge
 * are not written.  The device variant takes all three arrays as device memory on the context's device.
 *
 * The distance costs no comparison of sequences: a pair is verified as a variant of one kind -- the sequence
 * itself, one substitution, one deletion or insertion, two substitutions --, a variant never puts a residue where
 * the query has it already, and the lane that places the hit writes the distance of that kind beside it.  On top of
 * the footprint of cmpr_neighbors(): 1 byte per edge (the host variant holds it on the device for the duration of
 * the call), and for rows of more than 8192 hits the payload of the longest of them in and out of the device-wide
 * sort (1 byte per hit of that row) plus the scratch of a pair sort instead of a key sort.  The timing tunables
 * "neighbors_*_us" describe this call as they describe cmpr_neighbors().
 */
int cmpr_neighbors_distance(cmpr_context *ctx, uint64_t capacity,
                            uint64_t *row_start_out, uint32_t *hit_out, uint8_t *distance_out,
                            uint64_t *n_edges_out);
int cmpr_neighbors_distance_device(cmpr_context *ctx, uint64_t capacity,
                                   uint64_t *d_row_start_out, uint32_t *d_hit_out, uint8_t *d_distance_out,
                                   uint64_t *n_edges_out);

/*
 * The -x table without its zeros: per query, the set-2 repertoires it has a match in and the cell's value, as CSR.
 * The rows are the n1 sequences of the last cmpr_set_queries*(), in input order, WHATEVER options.existence is: a
 * context created with existence = 0 never allocates the n1 x R2 matrix and is the intended caller; one created
 * with existence = 1 gives the same answer.
 *   row_start_out[n1 + 1]    row_start[0] == 0, row_start[i + 1] - row_start[i] = the number of cells of row i.
 *                            Always written in full and always exact, whatever `capacity` is.  May be NULL when
 *                            only *n_cells_out is wanted.
 *   repertoire_out[capacity] row i occupies [row_start[i], row_start[i + 1]): set-2 repertoire numbers in strictly
 *                            increasing order.
 *   value_out[capacity]      beside each: exactly the integer that cell (i, r) of cmpr_overlap_matrix() holds on a
 *                            context with options.existence = 1 and otherwise the same options -- the sums listed
 *                            there (mean as count1 + count2, 1 per pair with ignore_counts; uint64 arithmetic,
 *                            which wraps as the matrix's does).
 *                            A cell is listed if and only if at least one verified pair falls in it (a cell whose
 *                            sum wraps to zero is listed with 0), the (i, i) pair included when one set is resident
 *                            as both; the call filters nothing.  When there are more cells than `capacity`, NOTHING
 *                            is written to the two cell arrays: the call still returns CMPR_OK with
 *                            *n_cells_out > capacity, and row_start says what to allocate.  capacity == 0 with both
 *                            arrays NULL is the count-only call.  capacity > 0 with either array NULL is
 *                            CMPR_EINVAL.  Elements behind the last cell are not the call's to write.
 *   *n_cells_out             required (NULL: CMPR_EINVAL), a HOST pointer in both variants; == row_start[n1].
 * cmpr_existence_csr_device() takes the three arrays as device memory on the context's device and writes only the
 * elements named above; only the cell count crosses PCIe.
 *
 * Results are bit-identical from run to run, under every tunable, and with set 2 indexed in parts: a cell is a sum
 * of integers over the row's hits in one repertoire, and the cells of a row are in order.  The call is a pass over
 * the neighbour rows (compairr_amd/csrc/existence.hip): the count step, the sum and the fill step of
 * cmpr_neighbors() into temporaries, each row sorted in place by (repertoire of the hit, hit) -- by a lane, a wave,
 * a workgroup in LDS or the device-wide radix sort, by its number of hits --, the cells per row counted and summed
 * into row_start, and, only when the cells fit `capacity`, each run of equal repertoires reduced to its cell.  The
 * count-only call runs everything but that reduction.  cmpr_get_stats() afterwards describes the last step the call
 * ran (cmpr_stats.matches = the number of edges).
 *
 * Device memory for the duration of the call, unlike the dense path PER EDGE: 4 bytes per edge; per query 4 bytes
 * (degrees, then cells per row), 8 (row offsets of the edges) and 8 for the queries' counts (not with
 * ignore_counts); the scratch of the sums; 4 bytes per row of more than 64 hits; and for rows of more than 8192
 * hits 24 bytes each, 12 times the longest of them, and the scratch of its sort and reduction.  The host variant
 * adds what the device variant is handed: 8 bytes per query and 12 per cell.  Everything is freed before the call
 * returns, also when it fails.
 *
 * Synchronous; needs both resident sets (CMPR_ESTATE as for cmpr_overlap_matrix()).  CMPR_SCORE_RATIO (without
 * ignore_counts) is not an integer sum: CMPR_EINVAL, use cmpr_overlap_matrix_f64().  With the tunable
 * work_shard_count above 1, and after cmpr_set_queries_routed(), the call is CMPR_EUNSUPPORTED: such a context holds
 * part of each row.  The resident sets, the plan and the other entry points are as usable afterwards as before; the
 * call may be repeated.  An empty query set is CMPR_OK with row_start == {0} and no cells.
 */
int cmpr_existence_csr(cmpr_context *ctx, uint64_t capacity,
                       uint64_t *row_start_out, uint32_t *repertoire_out, uint64_t *value_out,
                       uint64_t *n_cells_out);
int cmpr_existence_csr_device(cmpr_context *ctx, uint64_t capacity,
                              uint64_t *d_row_start_out, uint32_t *d_repertoire_out, uint64_t *d_value_out,
                              uint64_t *n_cells_out);

/*
 * Exact duplicates inside one set: the number the reference reports as
 * "Warning: N duplicates detected in repertoire set K" -- sequences that repeat
 * an earlier one of the same repertoire with the same V, J (unless
 * ignore_genes) and residues (hash_insert's return value summed,
 * overlap.cc:76-115, 579-605, 865-873).  set == NULL: the resident reference
 * set (needs cmpr_set_reference); otherwise `set` is uploaded and indexed in a
 * temporary table that is freed before returning.  Does not disturb the
 * resident sets.
 */
int cmpr_count_duplicates(cmpr_context *ctx, const cmpr_set_view *set, uint64_t *out);

/*
 * The duplicates of one set MERGED: the reference's --deduplicate (process() and report(),
 * dedup.cc:27-132; the loops of dedup(), dedup.cc:184-199).  Two sequences of `set` are the same entry when
 * they have the same repertoire number, the same V and J gene numbers (unless ignore_genes), the same length
 * and the same residues (dedup.cc:90-111); never across repertoires, not even with ignore_genes.  Per
 * equivalence class, in increasing `first` -- the order the reference prints them in --:
 *   first_out[k]  the smallest sequence number of the class (the reference prints a class at its first
 *                 member, with that member's ids);
 *   count_out[k]  the sum of duplicate_count over the class, with ignore_counts the number of its members
 *                 (dedup.cc:34-43); uint64 arithmetic, which wraps as the reference's does.
 * Up to `capacity` classes are written; *n_unique_out = the number of classes, *merged_out = n - classes --
 * the reference's "Duplicates merged:" figure, and what cmpr_count_duplicates() returns for the same set --
 * are always exact, are HOST pointers in both variants, and either may be NULL.  capacity == 0 with NULL
 * arrays only counts, as in cmpr_overlap_pairs().  n == 0 is CMPR_OK with zero classes.
 *
 * `set` is required (NULL: CMPR_EINVAL) and means what it means in cmpr_set_queries(): a HOST view, uploaded
 * and validated like every other set (same codes and messages).  cmpr_deduplicate_device() takes a DEVICE
 * view as cmpr_set_queries_device() does, and writes d_first_out / d_count_out -- device memory of
 * `capacity` elements on the context's device -- where they lie: nothing crosses PCIe but two offsets and
 * the class count.  The caller's arrays are only read, and may be freed once the call has returned.
 *
 * Synchronous; may be called at any time after cmpr_create(); the options' `differences` and `indels` play
 * no part (the reference insists on d = 0 at its command line; here they are ignored).  Does not disturb
 * the resident sets, plans or statistics.  Every temporary is freed before the call returns, also when it
 * fails.  Results are identical from run to run (integer sums; the smallest number of a class does not
 * depend on the schedule).
 *
 * Footprint per sequence, for the duration of the call: the validated copy of the set (~45 bytes; also for
 * a device view), one 8-byte table word per slot of ONE open-addressing table under the 70 % rule of
 * hashtable.cc:24 (11.4 to 22.9 bytes), 4 bytes for its slot and 8 for its sum: 70 to 80 bytes, plus 12
 * per class written by the host variant.  At most 2^32-64 sequences (CMPR_EUNSUPPORTED, "more than 2^32-64
 * sequences in one set"); no parts: a table or temporary that does not fit is CMPR_ENOMEM.
 */
int cmpr_deduplicate(cmpr_context *ctx, const cmpr_set_view *set, uint64_t capacity,
                     uint32_t *first_out, uint64_t *count_out,
                     uint64_t *n_unique_out, uint64_t *merged_out);
int cmpr_deduplicate_device(cmpr_context *ctx, const cmpr_set_view *d_set, uint64_t capacity,
                            uint32_t *d_first_out, uint64_t *d_count_out,
                            uint64_t *n_unique_out, uint64_t *merged_out);

/*
 * The single-linkage clusters of one set: the reference's --cluster (cluster.cc:200-410) without its output
 * order.  Two sequences of `set` are linked when the per-query loop of the set against itself would report
 * them as a pair under the context's options: within `differences` (0..2; with `indels` at d = 1) and with the
 * same V and J gene numbers unless ignore_genes.  The repertoire numbers and the counts play no part.  A
 * cluster is a connected component of that graph (what the breadth-first sweep of cluster.cc:276-410 reaches
 * from a seed):
 *   label_out[i]     the smallest sequence number in the cluster of i -- the seed the reference's sweep, which
 *                    takes the seeds in increasing order, prints the cluster at;
 *   size_out[i]      the number of members of that cluster: the reference's cluster_size column;
 *   *n_clusters_out  the number of i with label_out[i] == i: the reference's "Clusters:" figure.
 * (The reference numbers its clusters by size descending, then by that smallest number ascending:
 * cmpr_cluster_table() below gives that numbering and the members of every cluster.)  Any of the three may be NULL; n_clusters_out is a
 * HOST pointer in both variants.  n == 0 is CMPR_OK with zero clusters.  Results are identical from run to
 * run and do not depend on any tunable (the smallest number of a component does not depend on the schedule).
 *
 * The call (1) indexes `set` as the reference, as cmpr_set_reference[_device](set, 0) does, (2) lays it out
 * as the queries, as cmpr_set_queries[_device](set) does -- the same validation, codes, messages and size
 * limits; a refusal of either passes through unchanged --, (3) runs one synchronous step in which every
 * verified pair, instead of being scored or listed, unites its two sequences in a union-find forest on the
 * device (no pair list exists, on the device or on the host), and (4) flattens the forest into the labels and
 * counts the sizes.  AFTERWARDS `set` IS RESIDENT AS BOTH SETS: cmpr_overlap_* may follow directly and give
 * what a fresh context gives that was handed the same set twice.  Whatever was resident before is replaced.
 *
 * `set` is required (NULL: CMPR_EINVAL); options.existence is CMPR_EINVAL; with the tunable work_shard_count
 * above 1 the call is CMPR_EUNSUPPORTED (the components of shares do not add up by a sum).  May be called
 * wherever cmpr_set_reference() may be called, also repeatedly on one context.  cmpr_cluster_device() takes
 * a DEVICE view as cmpr_set_queries_device() does and writes d_label_out / d_size_out -- device memory of n
 * uint32 each on the context's device -- where they lie: only the sizes the layout needs anyway and the
 * cluster count cross PCIe.
 *
 * Footprint beyond the two resident sets, for the duration of the call: 4 bytes per sequence for the forest,
 * which afterwards holds the sizes unless they go to the caller's device array, and 4 for the labels unless
 * they go to the caller's device array.  Every temporary is freed before the call returns, also when it fails.
 */
int cmpr_cluster(cmpr_context *ctx, const cmpr_set_view *set,
                 uint32_t *label_out, uint32_t *size_out, uint64_t *n_clusters_out);
int cmpr_cluster_device(cmpr_context *ctx, const cmpr_set_view *d_set,
                        uint32_t *d_label_out, uint32_t *d_size_out, uint64_t *n_clusters_out);

/*
 * The clusters of one set as the reference's --cluster prints them, without the member order of its sweep: the
 * partition of cmpr_cluster() on the same set and context -- the same links, the same options, the same
 * independence from tunables and from a reference indexed in parts -- numbered and grouped on the device.
 * The K clusters are numbered 0 .. K-1 by (number of members descending, smallest member ascending); number k
 * is the reference's cluster_no k + 1 (its qsort compares sizes only, and equal sizes stay in the order of
 * their seeds, which is increasing: cluster.cc:53-63, :422).
 *   cluster_of_out[n]     the number of the cluster of sequence i;
 *   cluster_start_out     the caller provides n + 1 elements (K <= n: no capacity to guess or ask for); the first
 *                         K + 1 are written, the rest are not the call's to write.  cluster_start[0] == 0,
 *                         cluster_start[K] == n, and cluster_start[k + 1] - cluster_start[k] is the cluster_size
 *                         of cluster k, non-increasing in k;
 *   member_out[n]         cluster k occupies [cluster_start[k], cluster_start[k + 1]): its sequence numbers in
 *                         strictly increasing order, so the first is the cluster's label in the sense of
 *                         cmpr_cluster().  (The reference lists the members in the breadth-first order of its
 *                         sweep, which is not reproduced.)
 *   count_out             the caller provides n elements, K are written: the sum of duplicate_count over the
 *                         members of cluster k, with ignore_counts the number of its members; uint64 arithmetic,
 *                         as cmpr_deduplicate()'s count_out;
 *   *n_clusters_out       K, a HOST pointer in both variants.
 * Any of the five may be NULL.  cmpr_cluster_table_device() takes a DEVICE view as cmpr_cluster_device() does and
 * writes the four arrays -- device memory on the context's device -- where they lie: only what
 * cmpr_cluster_device() already moves, K and the largest cluster's size cross PCIe.
 *
 * Everything else is as for cmpr_cluster(), word for word: the same validation of the set, the same refusals
 * with the same codes and texts (NULL set, options.existence, work_shard_count > 1; d > 2 at cmpr_create);
 * n == 0 is CMPR_OK with K = 0 and nothing written but cluster_start[0] = 0; AFTERWARDS `set` IS RESIDENT AS
 * BOTH SETS; synchronous; every temporary is freed before the call returns, also when it fails.  Results are
 * identical from run to run (stable sorts, integer sums).
 *
 * Footprint beyond the two resident sets, for the duration of the call: the 8 bytes per sequence of
 * cmpr_cluster() (forest and labels, both reused by the table pass), 4 each for cluster_of and the members
 * unless they go to the caller's device arrays, 8 and a few histograms for the radix sort's scratch; per
 * cluster 16 bytes (roots and keys, before and behind their sort), and in the host variant 8 each for
 * cluster_start and the counts.
 */
int cmpr_cluster_table(cmpr_context *ctx, const cmpr_set_view *set,
                       uint32_t *cluster_of_out, uint64_t *cluster_start_out,
                       uint32_t *member_out, uint64_t *count_out, uint64_t *n_clusters_out);
int cmpr_cluster_table_device(cmpr_context *ctx, const cmpr_set_view *d_set,
                              uint32_t *d_cluster_of_out, uint64_t *d_cluster_start_out,
                              uint32_t *d_member_out, uint64_t *d_count_out, uint64_t *n_clusters_out);

/*
 * The reference's all-against-all path, for ANY d: above d = 2 (MAXDIFF_HASH, overlap.cc:368) the reference stops
 * hashing variants and compares every query with every sequence of set 2 (process_trad, overlap.cc:286-359; seq_diff,
 * util.cc:172-184).  cmpr_create() still refuses options.differences > 2; these calls take the distance as an
 * ARGUMENT and the two sets as views, as cmpr_deduplicate() takes its set, and options.differences plays no part.
 *
 * The pair relation is that of process_trad (overlap.cc:286-359), nothing filtered: (i of set1, j of set2) is a pair
 * when the two sequences have the same length (two empty sequences included), the same V and J gene numbers unless
 * options.ignore_genes, and differ at no more than `differences` positions.  With set2 == set1 (the same pointer)
 * the set is uploaded once and the (i, i) pairs are included, as in the reference's one-file mode.
 *   differences   any value >= 0, also 0, 1 and 2; negative is CMPR_EINVAL ("Differences specified with -d or
 *                 -differences cannot be negative.").  A value above the longest sequence behaves as that length.
 *
 * cmpr_hamming_matrix() (overlap.cc:286-359 with the sums of overlap.cc:218-231) writes R1 x R2 uint64 -- n1 x R2
 * with options.existence -- of exactly the integer sums cmpr_overlap_matrix() documents: product, min, max, mean as
 * count1 + count2, 1 per pair with ignore_counts, uint64 arithmetic that wraps.  The output is overwritten.
 * cmpr_hamming_matrix_device() takes DEVICE views, as cmpr_set_queries_device() does, and d_matrix on the context's
 * device.
 *
 * cmpr_hamming_neighbors() (overlap.cc:286-359 with the pair list of overlap.cc:232-245) gives the pairs as CSR with
 * the distance of every edge, under the protocol of cmpr_neighbors_distance(), word for word:
 *   row_start_out[n1 + 1]   always written in full and always exact, whatever `capacity` is; may be NULL.
 *   hit_out[capacity]       row i occupies [row_start[i], row_start[i + 1]): sequence numbers of set2 in strictly
 *                           increasing order.  With more edges than `capacity` NOTHING is written to hit_out or
 *                           distance_out and the call still returns CMPR_OK with *n_edges_out > capacity.
 *                           capacity == 0 with both arrays NULL is the count-only call; capacity > 0 with hit_out
 *                           NULL is CMPR_EINVAL.  Elements behind the last edge are not written.
 *   distance_out[capacity]  the number of differing positions of the pair, 0 .. differences; uint16_t: validation
 *                           caps a sequence at 65535 residues, so a distance fits, and a byte does not once d > 255.
 *                           May be NULL (hits only).
 *   *n_edges_out            required (NULL: CMPR_EINVAL), a HOST pointer in both variants; == row_start[n1].
 * cmpr_hamming_neighbors_device() takes DEVICE views and the three arrays as device memory: nothing per sequence or
 * per edge crosses PCIe, only two offsets per set, the group tables (one entry per distinct (length, V, J)) and the
 * edge count.
 *
 * All four: synchronous; callable any time after cmpr_create(); the sets are validated as every other set (same
 * codes and texts, passed through unchanged); the resident sets, plans and statistics are not disturbed; every
 * temporary is freed on every return; results are bit-identical from run to run and under every tunable (integer
 * sums; a row is one walk over one group in increasing sequence number -- no atomics, no row sort).  n1 == 0 or
 * n2 == 0 is CMPR_OK with a zero matrix, or row_start all zero.  Refused before any device work: options.indels
 * (CMPR_EINVAL, "the all-against-all path has no indels"); CMPR_SCORE_RATIO without ignore_counts in _matrix
 * (CMPR_EINVAL, use cmpr_overlap_matrix_f64(): there is no f64 form of this call); MH / Jaccard with differences > 0
 * (CMPR_EINVAL); a NULL set (CMPR_EINVAL); the tunable work_shard_count above 1 (CMPR_EUNSUPPORTED: the call sees
 * whole sets, N sharded contexts would each give the whole answer); n_v_genes x n_j_genes above 2^46
 * (CMPR_EUNSUPPORTED: (length, V, J) must fit a 64-bit key).  At most 2^31-1 sequences per set.
 *
 * How (compairr_amd/csrc/hamming.hip): each set is sorted by (length, V, J) -- a stable radix sort, so a group keeps
 * its sequences in increasing number --, its residues are packed in group order (four amino acids or sixteen
 * nucleotides per 32-bit word), and a workgroup compares 256 queries of a group with a segment of the matching set-2
 * group staged in LDS, every lane its own query.  Device memory for the duration of the call, per sequence of either
 * set: the validated copy (~45 bytes), 24 bytes of keys and sequence numbers before and behind the sort, 12 of run
 * keys and lengths and the sort's scratch (these freed before the comparison), 4 for the group order, and the
 * packed residues (4 bytes per 4 amino acids or 16 nucleotides, rounded up to 1, 2, 3, 4, 5, 6, 8, 12 or 16 words
 * up to 64 amino acids / 256 nucleotides).  _neighbors adds 12 bytes per (query, segment) -- the segment count is 1
 * once set 1 alone fills the machine, and at most 64 --; the host variants add what the device variants are handed:
 * 8 bytes per matrix cell, or 8 per query and 6 per edge (4 without distances).
 */
int cmpr_hamming_matrix(cmpr_context *ctx, const cmpr_set_view *set1, const cmpr_set_view *set2,
                        int64_t differences, uint64_t *matrix_out);
int cmpr_hamming_matrix_device(cmpr_context *ctx, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                               int64_t differences, void *d_matrix);
int cmpr_hamming_neighbors(cmpr_context *ctx, const cmpr_set_view *set1, const cmpr_set_view *set2,
                           int64_t differences, uint64_t capacity, uint64_t *row_start_out,
                           uint32_t *hit_out, uint16_t *distance_out, uint64_t *n_edges_out);
int cmpr_hamming_neighbors_device(cmpr_context *ctx, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                                  int64_t differences, uint64_t capacity, uint64_t *d_row_start_out,
                                  uint32_t *d_hit_out, uint16_t *d_distance_out, uint64_t *n_edges_out);

/*
 * Single-linkage clusters for ANY d: above d = 2 (MAXDIFF_HASH) the reference's --cluster builds its network by the
 * all-against-all sweep instead of hashed variants (process_trad, cluster.cc:165-211; the switch, cluster.cc:213-223)
 * and sweeps it as before (cluster.cc:276-410).  cmpr_cluster*() get their links from the hashed step and stop at
 * d = 2, where cmpr_create() stops; these calls take the distance as an ARGUMENT, as the rest of cmpr_hamming_*().
 *
 * Sequences i and j of `set` are linked when cmpr_hamming_neighbors(set, set, differences) lists (i, j): one length
 * (two empty sequences included), the same V and J gene numbers unless options.ignore_genes, at most `differences`
 * differing positions.  A cluster is a connected component of that graph.
 *
 * cmpr_hamming_cluster() (cluster.cc:165-211, :276-410) gives label_out[n], size_out[n] and *n_clusters_out, which
 * mean, word for word, what they mean in cmpr_cluster(): the smallest sequence number of i's cluster, the number of
 * its members, the number of i with label_out[i] == i.  cmpr_hamming_cluster_device() (cluster.cc:165-211) takes a
 * DEVICE view and writes d_label_out / d_size_out, device memory of n uint32 each, where they lie.
 *
 * cmpr_hamming_cluster_table() (cluster.cc:165-211, :276-410, numbered as cluster.cc:53-63, :422) gives
 * cluster_of_out[n], cluster_start_out (n + 1 provided, K + 1 written), member_out[n], count_out (n provided, K
 * written) and *n_clusters_out = K, which mean, word for word, what they mean in cmpr_cluster_table(): the clusters
 * numbered by (members descending, smallest member ascending) -- the reference's cluster_no - 1 --, the members of
 * each as CSR in increasing order, the summed duplicate_count per cluster (the number of members with
 * ignore_counts).  cmpr_hamming_cluster_table_device() (cluster.cc:165-211) takes a DEVICE view and writes the four
 * arrays -- device memory on the context's device -- where they lie.
 *
 * All four: any output may be NULL; n_clusters_out is a HOST pointer in both variants; n == 0 is CMPR_OK with K = 0
 * and nothing written but cluster_start[0] = 0.  As the rest of cmpr_hamming_*() and UNLIKE cmpr_cluster():
 * `differences` is any value >= 0, also 0, 1 and 2 (a value above the longest sequence behaves as that length) and
 * options.differences plays no part; callable any time after cmpr_create(); the resident sets, plans and statistics
 * are not disturbed and `set` is NOT resident afterwards; synchronous; every temporary is freed on every return;
 * results are bit-identical from run to run and under every tunable (a root of the forest is the smallest number of
 * its tree whatever the schedule; stable sorts, integer sums).  Refused before any device work, with the codes and
 * texts of cmpr_hamming_neighbors(): a negative `differences`, options.indels, a NULL set, the tunable
 * work_shard_count above 1, n_v_genes x n_j_genes above 2^46; options.existence is CMPR_EINVAL ("clusters are not
 * defined with options.existence", as cmpr_cluster()).  No score plays a part: MH / Jaccard with differences > 0 and
 * the ratio score are NOT refused here.  The set is validated as every other set (same codes and texts, passed
 * through unchanged).  At most 2^31-1 sequences.
 *
 * How (compairr_amd/csrc/hamming.hip, the link sink of the compare kernel): the set is grouped and packed once and
 * every group is compared with itself; a lane walks only the references BEHIND its own query in the group -- each
 * unordered pair once, the (i, i) pair never -- and a match unites the two sequences in a union-find forest over the
 * original sequence numbers (link_forest.h) unless the snapshots of their roots, staged beside the references,
 * already agree.  No pair list and no (query, segment) count array exist.  The flatten, size and table passes are
 * those of cmpr_cluster*() (cluster.hip).  Device memory for the duration of the call: the set copy, group order and
 * packed words of cmpr_hamming_*() above, 8 bytes per sequence of forest and labels (the forest's words take the sizes
 * afterwards; either goes to the caller's device array where one is given), and for the table calls the terms of
 * cmpr_cluster_table(): 4 bytes per sequence each for cluster_of and the members unless they go to the caller's
 * device arrays, 8 and a few histograms for the radix sort's scratch, 16 per cluster, and in the host variant 8 each
 * per cluster for cluster_start and the counts.
 */
int cmpr_hamming_cluster(cmpr_context *ctx, const cmpr_set_view *set, int64_t differences,
                         uint32_t *label_out, uint32_t *size_out, uint64_t *n_clusters_out);
int cmpr_hamming_cluster_device(cmpr_context *ctx, const cmpr_set_view *d_set, int64_t differences,
                                uint32_t *d_label_out, uint32_t *d_size_out, uint64_t *n_clusters_out);
int cmpr_hamming_cluster_table(cmpr_context *ctx, const cmpr_set_view *set, int64_t differences,
                               uint32_t *cluster_of_out, uint64_t *cluster_start_out,
                               uint32_t *member_out, uint64_t *count_out, uint64_t *n_clusters_out);
int cmpr_hamming_cluster_table_device(cmpr_context *ctx, const cmpr_set_view *d_set, int64_t differences,
                                      uint32_t *d_cluster_of_out, uint64_t *d_cluster_start_out,
                                      uint32_t *d_member_out, uint64_t *d_count_out, uint64_t *n_clusters_out);

/*
 * The nearest neighbour of every sequence, at ANY distance: the question the calls above cannot answer, because each of
 * them takes a threshold -- and in repertoire analysis the threshold comes from the data: the histogram of the
 * distances to the nearest neighbour is bimodal and the valley between its modes is the clonal threshold ("distance
 * to nearest").  The group relation is that of process_trad (overlap.cc:286-359), the distance that of seq_diff
 * (util.cc:172-184), as the rest of cmpr_hamming_*(); no `differences` limits it.
 *
 * The candidates of sequence i of set1 are the sequences j of set2 that
 *   - have the same length as i (two empty sequences included) and the same V and J gene numbers unless
 *     options.ignore_genes (overlap.cc:286-359);
 *   - differ from i at `min_distance` or more positions: 0 admits everything, 1 leaves out the sequences with i's own
 *     residues (the usual setting); negative is CMPR_EINVAL ("min_distance cannot be negative"); a value above the
 *     longest sequence finds nobody;
 *   - with set2 == set1 (the same pointer; the set is uploaded once) are not i itself: UNLIKE the calls above, the
 *     (i, i) pair is NEVER a candidate.  Other sequences with i's residues are, at distance 0;
 *   - with CMPR_NEAREST_OTHER_REPERTOIRE in `flags` come from another repertoire than i.  The flag is defined only
 *     with set2 == set1 -- two sets have two numberings of their repertoires --: with two sets it is CMPR_EINVAL, and
 *     so is any other bit of `flags`.
 *
 * cmpr_hamming_nearest() (overlap.cc:286-359) writes n1 elements of each output; any of them may be NULL:
 *   distance_out[i]   the smallest distance D over the candidates of i.
 *   nearest_out[i]    the smallest sequence number of set2 among the candidates at distance D.
 *   ties_out[i]       the number of candidates at distance D.
 * A sequence without a candidate gets nearest = 0xFFFFFFFF, distance = 0xFFFF and ties = 0.  nearest_out and ties_out
 * are the authoritative test for "no candidate": validation admits sequences of 65535 residues, so 0xFFFF is also a
 * possible distance.  Elements behind n1 are not written.
 *   *n_found_out      a HOST pointer in both variants, may be NULL: the number of i that have a candidate.
 * cmpr_hamming_nearest_device() (overlap.cc:286-359) takes DEVICE views and the three arrays as device memory on the
 * context's device: nothing per sequence crosses PCIe.
 *
 * Both, as the rest of cmpr_hamming_*(): synchronous; callable any time after cmpr_create(); options.differences plays
 * no part; the resident sets, plans and statistics are not disturbed; the sets are validated as every other set (same
 * codes and texts, passed through unchanged); every temporary is freed on every return; results are bit-identical
 * from run to run and under every tunable ((smallest distance, then smallest number) is a minimum, a tie count is an
 * integer sum).  n1 == 0 or n2 == 0 is CMPR_OK with every i "none".  Refused before any device work, with the codes
 * and texts of cmpr_hamming_neighbors(): options.indels, a NULL set, the tunable work_shard_count above 1,
 * n_v_genes x n_j_genes above 2^46.  No score plays a part: MH, Jaccard, the ratio score and options.existence are
 * NOT refused.  At most 2^31-1 sequences per set.
 *
 * How (compairr_amd/csrc/hamming.hip, the nearest sink of the compare kernel): one walk of the compare kernel, which
 * computes the full distance of every pair of a group anyway.  A lane keeps three registers -- the smallest distance,
 * the position in the group of the first reference at it, the number of references at it --, updated by two compares
 * and selects per reference; a reference that is no candidate takes part at an infinite distance.  Position order in
 * a group is number order (the stable sort), so the sequence number is looked up once, at the end.  With several
 * segments every (query, segment) writes a slot and a small kernel folds them: the minimum of (distance << 32 |
 * number), the ties of the slots at that distance summed.  Device memory for the duration of the call: the set copies,
 * group order and packed words of cmpr_hamming_*() above, 12 bytes per (query, segment) when there are several
 * segments, and in the host variant the 10 bytes per query of the outputs.
 */
enum { CMPR_NEAREST_OTHER_REPERTOIRE = 1 };

int cmpr_hamming_nearest(cmpr_context *ctx, const cmpr_set_view *set1, const cmpr_set_view *set2,
                         int64_t min_distance, uint32_t flags,
                         uint32_t *nearest_out, uint16_t *distance_out, uint32_t *ties_out,
                         uint64_t *n_found_out);
int cmpr_hamming_nearest_device(cmpr_context *ctx, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                                int64_t min_distance, uint32_t flags,
                                uint32_t *d_nearest_out, uint16_t *d_distance_out, uint32_t *d_ties_out,
                                uint64_t *n_found_out);

/*
 * The all-against-all path under EDIT distance, for any d.  The reference allows indels at d = 1 only ("The -i option
 * is allowed only when d=1": its variant enumeration explodes beyond), and so do cmpr_create() and the hashed calls;
 * cmpr_hamming_*() take any d but count substitutions only.  These calls take the distance as an ARGUMENT and the two
 * sets as views, as cmpr_hamming_*() do, and compare by Levenshtein distance.
 *
 * The pair relation: (i of set1, j of set2) is a pair when the two sequences have the same V and J gene numbers unless
 * options.ignore_genes, and the Levenshtein distance of their residues -- substitution, insertion and deletion cost 1
 * each -- is at most `differences`.  The lengths may differ by up to `differences`; empty sequences take part.  With
 * set2 == set1 (the same pointer) the set is uploaded once and the (i, i) pairs are included, as in the other calls.
 *   differences   any value >= 0; negative is CMPR_EINVAL ("Differences specified with -d or -differences cannot be
 *                 negative.").  A value above the longest sequence behaves as that length.
 * options.differences and options.indels play no part and are NOT refused: this call is the indel call.
 *
 * Relation to the other calls.  At differences = 0 the edges are those of cmpr_hamming_neighbors() at 0; at every d
 * every edge of cmpr_hamming_neighbors(d) is an edge here, at a distance no larger.  At differences = 1 the edge set
 * is that of the reference's -d 1 -i -- the hashed calls on a context with options.indels, and
 * cmpr_neighbors_distance()'s distances -- with ONE exception: the reference generates no deletion from a sequence of
 * one residue (variants.cc:301, `if (seqlen > 1)`), so it does not pair a one-residue sequence of set1 with an empty
 * sequence of set2, while it does pair the reverse.  Levenshtein distance is symmetric: these calls pair both.
 *
 * cmpr_edit_neighbors() gives the pairs as CSR with the distance of every edge, under the protocol of
 * cmpr_hamming_neighbors(), word for word:
 *   row_start_out[n1 + 1]   always written in full and always exact, whatever `capacity` is; may be NULL.
 *   hit_out[capacity]       row i occupies [row_start[i], row_start[i + 1]): sequence numbers of set2 in strictly
 *                           increasing order.  With more edges than `capacity` NOTHING is written to hit_out or
 *                           distance_out and the call still returns CMPR_OK with *n_edges_out > capacity.
 *                           capacity == 0 with both arrays NULL is the count-only call; capacity > 0 with hit_out
 *                           NULL is CMPR_EINVAL.  Elements behind the last edge are not written.
 *   distance_out[capacity]  the Levenshtein distance of the pair, 0 .. differences.  May be NULL (hits only).
 *   *n_edges_out            required (NULL: CMPR_EINVAL), a HOST pointer in both variants; == row_start[n1].
 * cmpr_edit_neighbors_device() takes DEVICE views and the three arrays as device memory.
 *
 * cmpr_edit_matrix() writes R1 x R2 uint64 -- n1 x R2 with options.existence -- of the integer sums
 * cmpr_hamming_matrix() documents, over these pairs; the output is overwritten.  cmpr_edit_matrix_device() takes DEVICE
 * views and d_matrix on the context's device.
 *
 * All four: synchronous; callable any time after cmpr_create(); the sets are validated as every other set (same
 * codes and texts, passed through unchanged); the resident sets, plans and statistics are not disturbed; every
 * temporary is freed on every return; results are bit-identical from run to run and under every tunable (integer
 * sums; the hits of a row are distinct, so the row order is total).  n1 == 0 or n2 == 0 is CMPR_OK with a zero matrix,
 * or row_start all zero.  Refused before any device work, with the codes and texts of cmpr_hamming_neighbors(): a
 * negative `differences`; a NULL set; the tunable work_shard_count above 1; n_v_genes x n_j_genes above 2^46;
 * CMPR_SCORE_RATIO without ignore_counts in _matrix; MH / Jaccard with differences > 0.  A set whose longest sequence
 * has more than 256 residues is CMPR_EUNSUPPORTED ("cmpr_edit: a sequence of more than 256 residues"), decided when the
 * set has been validated on the device and before anything is compared: 256 residues are four 64-bit words of the
 * bit-vector column below, and cover every CDR3 and junction, amino acids or nucleotides.  At most 2^31-1 sequences
 * per set.
 *
 * How (compairr_amd/csrc/edit.hip): the sets are grouped by (length, V, J) and packed as for cmpr_hamming_*().  The
 * host pairs every set-1 group (L, V, J) with the set-2 groups (L', V, J), |L - L'| <= d, by binary search of the
 * group keys over the lengths set 2 has.  A workgroup compares 256 queries of a group with a segment of every such
 * partner, staged in LDS as match vectors (per reference and symbol, a bit per position), every lane its own query
 * through the bit-vector edit distance (Myers 1999; global form of Hyyro 2003): one LDS read and some fifteen 64-bit
 * operations per query residue and 64 reference residues.  A walk goes partner by partner, so the rows are sorted
 * afterwards (by the hit; distances carried along).  Device memory for the duration of the call: what
 * cmpr_hamming_neighbors() / _matrix() take, 40 bytes per set-1 group and 24 per pair of groups, and while the rows
 * are put in order 4 bytes per row of more than 64 hits and 6 bytes per hit of the longest row beyond 8192.
 */
int cmpr_edit_neighbors(cmpr_context *ctx, const cmpr_set_view *set1, const cmpr_set_view *set2,
                        int64_t differences, uint64_t capacity, uint64_t *row_start_out,
                        uint32_t *hit_out, uint16_t *distance_out, uint64_t *n_edges_out);
int cmpr_edit_neighbors_device(cmpr_context *ctx, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                               int64_t differences, uint64_t capacity, uint64_t *d_row_start_out,
                               uint32_t *d_hit_out, uint16_t *d_distance_out, uint64_t *n_edges_out);
int cmpr_edit_matrix(cmpr_context *ctx, const cmpr_set_view *set1, const cmpr_set_view *set2,
                     int64_t differences, uint64_t *matrix_out);
int cmpr_edit_matrix_device(cmpr_context *ctx, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                            int64_t differences, void *d_matrix);

/*
 * Single-linkage clusters under EDIT distance, at ANY d: the clusters of CDR3s that lie within d substitutions,
 * insertions and deletions of each other -- at d = 2 or 3 the usual TCR clustering question.  cmpr_cluster*() with
 * options.indels stops at d = 1, as the reference does; cmpr_hamming_cluster*() count substitutions only.  These calls
 * are to cmpr_edit_neighbors() what cmpr_hamming_cluster*() are to cmpr_hamming_neighbors().
 *
 * Sequences i and j of `set` are linked when cmpr_edit_neighbors(set, set, differences) lists (i, j): the same V and J
 * gene numbers unless options.ignore_genes, Levenshtein distance at most `differences`; the lengths may lie up to
 * `differences` apart, empty sequences included.  A cluster is a connected component of that graph.
 *
 * cmpr_edit_cluster() gives label_out[n], size_out[n] and *n_clusters_out, which mean, word for word, what they mean in
 * cmpr_cluster(): the smallest sequence number of i's cluster, the number of its members, the number of i with
 * label_out[i] == i.  cmpr_edit_cluster_device() takes a DEVICE view and writes d_label_out / d_size_out, device memory
 * of n uint32 each, where they lie.
 *
 * cmpr_edit_cluster_table() gives cluster_of_out[n], cluster_start_out (n + 1 provided, K + 1 written), member_out[n],
 * count_out (n provided, K written) and *n_clusters_out = K, which mean, word for word, what they mean in
 * cmpr_cluster_table(): the clusters numbered by (members descending, smallest member ascending), the members of each as
 * CSR in increasing order, the summed duplicate_count per cluster (the number of members with ignore_counts).
 * cmpr_edit_cluster_table_device() takes a DEVICE view and writes the four arrays -- device memory on the context's
 * device -- where they lie.
 *
 * Relation to the other calls.  At differences = 0 the partition is that of cmpr_hamming_cluster(set, 0).  At
 * differences = 1 it is the partition cmpr_cluster() gives on a context with differences = 1 and indels = 1, on every
 * set, without exception: the pair of a one-residue sequence and an empty one, which the reference's deletion rule
 * leaves out one way (variants.cc:301; see cmpr_edit_neighbors()), is found the other way, and a link has no direction.
 * At every d each cluster of cmpr_hamming_cluster(set, d) lies inside one cluster here.
 *
 * All four: any output may be NULL; n_clusters_out is a HOST pointer in both variants; n == 0 is CMPR_OK with K = 0
 * and nothing written but cluster_start[0] = 0.  As the rest of cmpr_edit_*() and cmpr_hamming_cluster*():
 * `differences` is any value >= 0 (a value above the longest sequence behaves as that length); options.differences and
 * options.indels play no part and are NOT refused; callable any time after cmpr_create(); the resident sets, plans and
 * statistics are not disturbed and `set` is NOT resident afterwards; synchronous; every temporary is freed on every
 * return; results are bit-identical from run to run and under every tunable (a root of the forest is the smallest
 * number of its tree whatever the schedule; stable sorts, integer sums).  Refused before any device work, with the
 * codes and texts of cmpr_hamming_cluster(): a negative `differences`, a NULL set, the tunable work_shard_count above
 * 1, n_v_genes x n_j_genes above 2^46; options.existence is CMPR_EINVAL ("clusters are not defined with
 * options.existence", as cmpr_cluster()).  No score plays a part: MH, Jaccard and the ratio score are NOT refused.  The
 * set is validated as every other set (same codes and texts, passed through unchanged).  A set whose longest sequence
 * has more than 256 residues is CMPR_EUNSUPPORTED ("cmpr_edit: a sequence of more than 256 residues"), as for
 * cmpr_edit_neighbors().  At most 2^31-1 sequences.
 *
 * How (compairr_amd/csrc/edit.hip, the link sink of allpairs.h on the compare kernel of cmpr_edit_*()): the set is
 * grouped and packed once.  A group (L, V, J) keeps as partners only the groups (L', V, J) with L <= L' <= L + d: a pair
 * of two lengths is seen from the shorter side, and a longer partner is walked in full.  In its own group a lane walks
 * only the references BEHIND its own query -- the workgroup of queries [256 b, 256 b + 256) walks the positions from
 * 256 b + 1 on, its segments divide that range, a wave skips the staged pieces at or below its first query -- so every
 * unordered pair is compared once and the (i, i) pair never.  A match unites the two sequences in a union-find forest
 * over the original sequence numbers (link_forest.h) unless the snapshots of their roots, staged beside the references,
 * already agree.  No pair list and no (query, segment) count array exist.  The flatten, size and table passes are those
 * of cmpr_cluster*() (cluster.hip).  Device memory for the duration of the call: the set copy, group order and packed
 * words of cmpr_edit_*() above, 40 bytes per group (job) and 24 per pair of groups, 8 bytes per sequence of forest and
 * labels (the forest's words take the sizes afterwards; either goes to the caller's device array where one is given),
 * and for the table calls the terms of cmpr_cluster_table(): 4 bytes per sequence each for cluster_of and the members
 * unless they go to the caller's device arrays, 8 and a few histograms for the radix sort's scratch, 16 per cluster, and
 * in the host variant 8 each per cluster for cluster_start and the counts.
 */
int cmpr_edit_cluster(cmpr_context *ctx, const cmpr_set_view *set, int64_t differences,
                      uint32_t *label_out, uint32_t *size_out, uint64_t *n_clusters_out);
int cmpr_edit_cluster_device(cmpr_context *ctx, const cmpr_set_view *d_set, int64_t differences,
                             uint32_t *d_label_out, uint32_t *d_size_out, uint64_t *n_clusters_out);
int cmpr_edit_cluster_table(cmpr_context *ctx, const cmpr_set_view *set, int64_t differences,
                            uint32_t *cluster_of_out, uint64_t *cluster_start_out,
                            uint32_t *member_out, uint64_t *count_out, uint64_t *n_clusters_out);
int cmpr_edit_cluster_table_device(cmpr_context *ctx, const cmpr_set_view *d_set, int64_t differences,
                                   uint32_t *d_cluster_of_out, uint64_t *d_cluster_start_out,
                                   uint32_t *d_member_out, uint64_t *d_count_out, uint64_t *n_clusters_out);

/*
 * The nearest neighbour of every sequence under EDIT distance: cmpr_hamming_nearest() with the Levenshtein distance of
 * cmpr_edit_*() in place of the number of differing positions.  cmpr_hamming_nearest() is blind to indels -- a CDR3
 * whose only close relative is one residue longer has a far neighbour there, or none --, and cmpr_edit_cluster*() and
 * cmpr_edit_neighbors() need a `differences`, which is read from the histogram of these distances.
 *
 * The candidates of sequence i of set1 are the sequences j of set2 that
 *   - have the same V and J gene numbers unless options.ignore_genes; their LENGTH may be any, empty sequences
 *     included;
 *   - lie at a Levenshtein distance from i -- substitution, insertion and deletion cost 1 each -- of `min_distance` or
 *     more and of `max_distance` or less.  min_distance: 0 admits everything, 1 leaves out the sequences with i's own
 *     residues; negative is CMPR_EINVAL ("min_distance cannot be negative").  max_distance: the cap; negative is
 *     CMPR_EINVAL ("max_distance cannot be negative"); a value above the longest sequence of either set behaves as that
 *     length -- no edit distance exceeds it --, which is the uncapped call (INT64_MAX).  min_distance > max_distance is
 *     CMPR_OK with nobody found;
 *   - with set2 == set1 (the same pointer; the set is uploaded once) are not i itself, as in cmpr_hamming_nearest();
 *   - with CMPR_NEAREST_OTHER_REPERTOIRE in `flags` come from another repertoire than i.  The flag is defined only
 *     with set2 == set1: with two sets it is CMPR_EINVAL, and so is any other bit of `flags`.
 *
 * cmpr_edit_nearest() writes n1 elements of each output; any of them may be NULL:
 *   distance_out[i]   the smallest distance D over the candidates of i.
 *   nearest_out[i]    the smallest sequence number of set2 among the candidates at distance D.
 *   ties_out[i]       the number of candidates at distance D.
 * A sequence without a candidate gets nearest = 0xFFFFFFFF, distance = 0xFFFF and ties = 0; HERE 0xFFFF is
 * unambiguous: the sequences have at most 256 residues, and so has every distance.  Elements behind n1 are not written.
 *   *n_found_out      a HOST pointer in both variants, may be NULL: the number of i that have a candidate.
 * cmpr_edit_nearest_device() takes DEVICE views and the three arrays as device memory on the context's device.
 *
 * Relation to the other calls.  The three arrays are what cmpr_edit_neighbors(differences = max_distance) gives when
 * every row is filtered (floor, self, repertoire) and reduced to its minimum.  Uncapped, every i that
 * cmpr_hamming_nearest() finds is found here, at a distance no larger.
 *
 * Both, as the rest of cmpr_edit_*(): synchronous; callable any time after cmpr_create(); options.differences and
 * options.indels play no part and are NOT refused; the resident sets, plans and statistics are not disturbed; the sets
 * are validated as every other set (same codes and texts, passed through unchanged); every temporary is freed on every
 * return; results are bit-identical from run to run and under every tunable ((smallest distance, then smallest number)
 * is a minimum, a tie count is an integer sum).  n1 == 0 or n2 == 0 is CMPR_OK with every i "none".  Refused before any
 * device work, with the codes and texts of cmpr_hamming_nearest(): a NULL set, the tunable work_shard_count above 1,
 * n_v_genes x n_j_genes above 2^46.  No score plays a part: MH, Jaccard, the ratio score and options.existence are NOT
 * refused.  A set whose longest sequence has more than 256 residues is CMPR_EUNSUPPORTED ("cmpr_edit: a sequence of
 * more than 256 residues"), as for cmpr_edit_neighbors().  At most 2^31-1 sequences per set.
 *
 * How (compairr_amd/csrc/edit.hip, the nearest sink of the compare kernel of cmpr_edit_*()): that kernel computes the
 * full distance of every pair it walks.  A lane keeps three registers -- the smallest distance, the smallest sequence
 * number at it, the number of references at it --, updated by compares and selects per reference; a walk goes partner
 * by partner, which is not number order, so the numbers themselves are compared (staged beside the references).  A
 * reference that is no candidate takes part at an infinite distance.  The partners of a group (L, V, J) are the set-2
 * groups (L', V, J) with |L - L'| <= max_distance IN ORDER OF |L - L'|: no distance is below the length gap, so a
 * workgroup leaves its partners at the first gap that no lane's smallest distance reaches any more -- exactly, nothing
 * behind it can improve on or tie with what a lane holds; Hamming, with one partner per group, has nothing of the kind.
 * With several segments every (query, segment) writes a slot and a small kernel folds them, as for
 * cmpr_hamming_nearest(); a (workgroup, segment) stops on its own partial minimum, an upper bound of the final one.
 * Device memory for the duration of the call: the set copies, group order, packed words, jobs and partners of
 * cmpr_edit_*() above, 12 bytes per (query, segment) when there are several segments, and in the host variant the 10
 * bytes per query of the outputs.
 */
int cmpr_edit_nearest(cmpr_context *ctx, const cmpr_set_view *set1, const cmpr_set_view *set2,
                      int64_t min_distance, int64_t max_distance, uint32_t flags,
                      uint32_t *nearest_out, uint16_t *distance_out, uint32_t *ties_out,
                      uint64_t *n_found_out);
int cmpr_edit_nearest_device(cmpr_context *ctx, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                             int64_t min_distance, int64_t max_distance, uint32_t flags,
                             uint32_t *d_nearest_out, uint16_t *d_distance_out, uint32_t *d_ties_out,
                             uint64_t *n_found_out);

/*
 * The all-against-all path under the WEIGHTED CDR3 distance of the TCR field -- the metric behind tcrdist3 and scirpy's
 * "tcrdist": a substitution-table-weighted mismatch sum over the CDR3, the ends trimmed, ONE gap block charged per
 * residue of length difference, optionally a V-gene term on top.  Neither cmpr_hamming_*() nor cmpr_edit_*() can
 * express it: there "L -> I" costs what "L -> D" costs, the conserved CAS... / ...QYF ends count, two lengths align with
 * free indels, and two V genes are equal or not.  The reference has no counterpart.
 *
 * The distance.  W = params->substitution, alphabet_size x alphabet_size uint8, indexed [residue of the set-1 sequence]
 * [residue of the set-2 sequence]; no symmetry and no zero diagonal are assumed.  For x of set 1 and y of set 2:
 *   equal length L     D = sum over k = ntrim .. L - 1 - ctrim of W[x_k][y_k]; an empty range gives 0.
 *   different lengths  s the shorter (Ls residues), l the longer, delta = Ll - Ls.  For a gap position g, 0 <= g <= Ls,
 *                        cost(g) = sum_{k = ntrim}^{g - 1} w(s_k, l_k) + sum_{k = g}^{Ls - 1 - ctrim} w(s_k, l_{k + delta})
 *                      where w is W indexed [set-1 residue][set-2 residue] WHICHEVER of the two is the shorter, and
 *                        D = min_{g = lo .. hi} cost(g) + delta x gap_penalty.
 *                      CMPR_GAP_FIXED:   lo = hi = min(6, 3 + floor((Ls - 5) / 2)) (a mathematical floor: Ls = 0 gives 0);
 *                      CMPR_GAP_SLIDING: lo = 5, hi = Ls - 5; while lo > hi: lo -= 1, hi += 1.
 *                      Both keep 0 <= lo <= hi <= Ls for every Ls.
 *   with a V table     D += params->v_distance[v1][v2], n_v_genes x n_v_genes uint16, v1 the V gene number of x.
 * (i, j) is a pair when D <= cutoff and the genes admit it: without v_distance the same V and J gene numbers unless
 * options.ignore_genes, as in every other call; WITH v_distance any two V genes pair, at the table's price, and the J
 * gene plays no part.  With set2 == set1 (the same pointer) the set is uploaded once and the (i, i) pairs are included.
 *
 * cmpr_tcrdist_neighbors() gives the pairs as CSR with the distance of every edge, under the protocol of
 * cmpr_edit_neighbors(), word for word: row_start_out[n1 + 1] always written in full and always exact, may be NULL;
 * hit_out[capacity] the rows, sequence numbers of set2 in strictly increasing order; with more edges than `capacity`
 * NOTHING is written to hit_out or distance_out and the call still returns CMPR_OK with *n_edges_out > capacity;
 * capacity == 0 with both arrays NULL is the count-only call; capacity > 0 with hit_out NULL is CMPR_EINVAL; elements
 * behind the last edge are not written; distance_out[capacity] is D, 0 .. cutoff, and may be NULL (hits only);
 * *n_edges_out is required (NULL: CMPR_EINVAL), a HOST pointer in both variants, == row_start[n1].
 * cmpr_tcrdist_matrix() writes R1 x R2 uint64 -- n1 x R2 with options.existence -- of the integer sums
 * cmpr_edit_matrix() documents, over these pairs; the output is overwritten.  The _device variants take DEVICE views
 * and device arrays; `params` and the two tables it points to are HOST memory in both variants, read during the call.
 *
 * All four: synchronous; callable any time after cmpr_create(); options.differences and options.indels play no part and
 * are NOT refused; the sets are validated as every other set; the resident sets, plans and statistics are not disturbed;
 * every temporary is freed on every return; results are bit-identical from run to run and under every tunable (integer
 * sums; the hits of a row are distinct, so the row order is total).  n1 == 0 or n2 == 0 is CMPR_OK with a zero matrix,
 * or row_start all zero.  Refused before any device work: what cmpr_edit_*() refuse, with `cutoff` in the place of
 * `differences` and the same codes and texts (negative; a NULL set; the tunable work_shard_count above 1;
 * n_v_genes x n_j_genes above 2^46; CMPR_SCORE_RATIO without ignore_counts in _matrix; MH / Jaccard with cutoff > 0);
 * NULL params or params->substitution (CMPR_EINVAL); cutoff > 65535 (CMPR_EINVAL: the distance column is uint16); a
 * nonzero reserved word or a gap_mode other than the two (CMPR_EINVAL); v_distance with options.ignore_genes
 * (CMPR_EINVAL: there are no V gene numbers); alphabet_size == 4 (CMPR_EUNSUPPORTED, "cmpr_tcrdist: amino acids only").
 * A set whose longest sequence has more than 256 residues is CMPR_EUNSUPPORTED
 * ("cmpr_tcrdist: a sequence of more than 256 residues"), decided when the set has been validated on the device, as for
 * cmpr_edit_neighbors().  At most 2^31-1 sequences per set.
 *
 * How (compairr_amd/csrc/tcrdist.hip): the sets are grouped by (length, V, J) -- (length, V) with a V table, the length
 * with ignore_genes -- and packed as for cmpr_edit_*().  The host pairs every set-1 group with the set-2 groups whose
 * base = |L - L'| x gap_penalty + V[v1][v2] (64 bits) is at most the cutoff -- a positive penalty bounds the lengths, 0
 * admits every length -- and works out, per pair of groups, everything the alignment needs: the kernel never touches
 * genes.  A workgroup compares 256 queries of a group with a segment of every such partner, staged in LDS as packed;
 * W lies in LDS transposed, a padded row per reference residue, so that the reference residue a wave meets is one
 * broadcast read and the lanes' costs come from one short row.  Per aligned position a lookup and an add, two in the
 * zone of gap positions SLIDING tries; the running minimum over the gap positions needs one pass and no array.  A walk
 * goes partner by partner, so the rows are sorted afterwards (by the hit; distances carried along).  Device memory for
 * the duration of the call: what cmpr_edit_neighbors() / _matrix() take, with 64 bytes per pair of groups.
 *
 * Out of scope: clusters and nearest neighbours under this metric; nucleotides; a shipped BLOSUM-derived default table
 * (the caller supplies W already multiplied by its weight); paired chains; the command line.
 */
enum { CMPR_GAP_FIXED = 0, CMPR_GAP_SLIDING = 1 };
typedef struct cmpr_tcrdist_params {
  const uint8_t  *substitution;  /* alphabet_size x alphabet_size, [set-1 residue][set-2 residue]; HOST memory in both variants */
  const uint16_t *v_distance;    /* n_v_genes x n_v_genes or NULL; HOST memory in both variants */
  uint32_t gap_penalty, ntrim, ctrim, gap_mode;
  uint32_t reserved[4];          /* must be zero */
} cmpr_tcrdist_params;

int cmpr_tcrdist_neighbors(cmpr_context *ctx, const cmpr_set_view *set1, const cmpr_set_view *set2,
                           const cmpr_tcrdist_params *params, int64_t cutoff, uint64_t capacity,
                           uint64_t *row_start_out, uint32_t *hit_out, uint16_t *distance_out,
                           uint64_t *n_edges_out);
int cmpr_tcrdist_neighbors_device(cmpr_context *ctx, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                                  const cmpr_tcrdist_params *params, int64_t cutoff, uint64_t capacity,
                                  uint64_t *d_row_start_out, uint32_t *d_hit_out, uint16_t *d_distance_out,
                                  uint64_t *n_edges_out);
int cmpr_tcrdist_matrix(cmpr_context *ctx, const cmpr_set_view *set1, const cmpr_set_view *set2,
                        const cmpr_tcrdist_params *params, int64_t cutoff, uint64_t *matrix_out);
int cmpr_tcrdist_matrix_device(cmpr_context *ctx, const cmpr_set_view *d_set1, const cmpr_set_view *d_set2,
                               const cmpr_tcrdist_params *params, int64_t cutoff, void *d_matrix);

/*
 * (ABI v4)  What a process pays once before its first launch, asked for early: the HIP
 * runtime, the device's context, the code objects of the kernels the given options will run.
 * The reference has no counterpart -- its threads start in microseconds (overlap.cc:926-936);
 * a GPU process needs ~0.4 s here, which a caller can spend while it still reads its input
 * (compairr_amd/host/overlap_host.cc does, on a thread of its own).  Only `differences`,
 * `indels`, `alphabet_size`, `ignore_genes` and `device` of `options` are looked at.  Creates
 * nothing the caller has to free.  Thread-safe against every other entry point.
 */
int cmpr_warm_up(const cmpr_options *options);

/*
 * (ABI v5)  cmpr_warm_up() for a caller that knows roughly how large its sets will be -- the host program
 * knows both file sizes before it parses a line (compairr_amd/host/overlap_host.cc) --: additionally
 * reserves what the first cmpr_set_queries() of a set of `n_queries_hint` sequences with
 * `residue_bytes_hint` residues would otherwise allocate while the caller waits (the page-locked staging
 * buffer of its upload, 12 bytes per query, and the device arena of the layout's temporaries).  The first
 * context that needs them takes them over; what nobody took is released by the first cmpr_destroy().
 * `n_refs_hint` is accepted for symmetry (the index build keeps nothing that could be reserved).  Hints
 * are hints: too small, and the call allocates as before; too large, and memory is held until taken or
 * released.  The reference has no counterpart (overlap.cc:840-887 allocates in microseconds).
 */
int cmpr_warm_up_sized(const cmpr_options *options, uint64_t n_queries_hint, uint64_t n_refs_hint,
                       uint64_t residue_bytes_hint);

/* Statistics of the last overlap call (synchronises the context's events). */
int cmpr_get_stats(cmpr_context *ctx, cmpr_stats *out);

/*
 * HIP-event kernel times of the last `max` (at most 63) cmpr_overlap_* calls,
 * oldest first: kernel_ms[k] = probe + resolve kernels, probe_ms[k] = the probe
 * kernel alone (either may be NULL).  Lets a caller queue many launches on a
 * stream without synchronising after each (the reference has one timed region,
 * "Analysing:", overlap.cc:906-938; this is its per-launch counterpart).
 */
int cmpr_get_kernel_times(cmpr_context *ctx, uint32_t max, double *kernel_ms,
                          double *probe_ms, uint32_t *count_out);

/* Sizes, for callers that allocate the matrix. */
uint32_t cmpr_rows(const cmpr_context *ctx);      /* R1, after set_queries   */
uint32_t cmpr_cols(const cmpr_context *ctx);      /* R2, after set_reference */

/* Tuning knobs (unknown names -> CMPR_EINVAL).  Results never depend on them.
     "variant"               0: one Bloom filter probed in HBM -- at d = 0 no filter at
                             all, the query looked up where its bucket lies (default
                             for d = 0); 1: class-keyed
                             32 KiB slices staged in LDS, one filter word per
                             variant (default for nucleotides at d >= 1); 2: the same
                             slices over the row filter, one filter word per
                             position (default for amino acids at d >= 1); -1: default
     "blocks_per_cu"         resident workgroups per CU the grid is sized for
     "bloom_bits_log2_delta" filter bytes = hash-table slots << delta
                             (default 0 for variant 0, +2 for variant 1)
     "class_residues"        -1 (default: from the data) or 0..4 amino acids / 0..8 nucleotides (four
                             amino-acid residues: variant 2 at d = 1, on kernel instantiations of
                             their own; anywhere else the value is clamped to three)
     "slice_words_log2"      log2 of the (largest) slice in filter words: 64-bit
                             words, default 12 (variant 1); 256-bit words,
                             -1 = default: sized to the LDS (<= 640 words), or
                             a power of two 1..13 (variant 2)
     "chunk_tiles"           tiles per workgroup work item (default 8 x waves)
     "waves_per_block"       4, 8 or 16 waves per workgroup (variants 1, 2;
                             default 8 / 16)
     "small_slice_tiles"     slices with at most this many tiles are probed where
                             they lie instead of being staged (default 0)
     "work_shard_count",     this context does the work filed under every
     "work_shard_index"      count-th share of the filter slices, share `index`
                             (default 1, 0: everything).  N contexts -- e.g. one
                             per GPU -- with the same sets and index 0..N-1
                             produce matrices, pair lists and counters that add
                             up to the unsharded ones (variants 1, 2).
     "sub2_items"            nucleotides, d = 2, variant 1: the double substitutions
                             that put a new residue on a class position are grouped
                             by the slice they land in and probed there (1, and
                             the default -1), or probed where the filter lies (0)
     "d2_pairs"              nucleotides, d = 2: -1 (default) / 1: pair rows probed by a workgroup per
                             tile (kernels_pairs2.h; sequences of at most 96 residues), 0: off
     "d2_buffers"            that kernel's slice buffers: 1 (default; slices twice the size: fuller
                             tiles) or 2 (the next slice is copied while this one is worked on)
     "chunk_deal"            variant 2: 1 (default): beyond a workgroup's first four, chunks are handed out
                             by counters in list order (heaviest first) -- on skewed data (the cdr3 law,
                             d = 1 -i) the probe kernel takes 1.5 ms where a static deal takes 2.5; 0: static
     "part_buckets_log2"     the most buckets one part's record table may have (2..30, default 30),
                             counted after table_log2_delta: a larger set 2 is indexed in parts (see
                             cmpr_set_reference; environment COMPAIRR_HIP_PART_BUCKETS_LOG2 at cmpr_create).
                             Read-only "reference_parts": the parts in effect (0 before cmpr_set_reference)
     "table_log2_delta"      buckets of the record table = 2^delta x the 70 % rule of hashtable.cc:24 (default 1:
                             at most 0.35 full -- one memory line per looked-up sequence); 0..3
     "bucket_bitmap"         resolve_kernel asks a bitmap (one bit per bucket: it holds a record) before it
                             reads a slot of the record table: -1 (default) where most Bloom positives are
                             false (d = 2), 0 never, 1 always
     "slice_pages"           variant 2, d = 1: a slice of the row filter that holds more than "page_budget"
                             entries is spread over up to 2^this pages by hash bits, its tiles worked on once
                             per page (-1 = default: 3; 0: no pages); "page_budget": entries, 0 = default
                             (20 per 32-byte word)
     "fill_slices"           variant 2, d = 2 on single rows: 1 (default) the slices take all the words their
                             LDS buffer holds (a sparser filter for the 38 000 tests of a query), 0 as many
                             as the entries ask for
     "row_filter_x16"        variant 2: bytes of filter per entry in sixteenths (default 32 = 2 bytes)
     "direct_slices_log2"    d = 0 (variant 0, the default there: no filter, every query looked up where its
                             bucket lies): the layout groups the queries by length and by 2^this pseudo-slices
                             -- bits of the hash --; -1 (default) one per 32 768 queries
     "pos_grow"              the positives buffer grows to what a launch showed when it overflowed:
                             -1 (default) when its size was automatic, 1 also from a given
                             "pos_capacity", 0 never
     "deferred_resolve"      1 (default): the filter's positives are queued and walked by a second kernel; 0: the
                             probe kernel resolves them itself
     "resolve_blocks_per_cu" resident workgroups per CU that second kernel's grid is sized for (1..8, default 5)
     "pos_segments"          independently claimed parts of the queue of positives: a power of two, 1..256 (default 64)
     "pos_capacity"          entries of that queue, all segments together (0 = default: from the number of queries)
     "heavy_threshold"       population above which a class is split over several slices (-1 = default: from
                             the slice size; 0: every class)
     "class_anchor"          first of the sequence positions the class is taken from (-1 = default: from the
                             lengths of set 2; up to 65535)
     "class_rows_unstaged"   variant 2: 1: the tiles of the class rows read the filter where it lies; 0 (default): staged
     "host_threads"          threads of the host-side passes over a set (1..256; default: the machine's, at most 16)
     "assume_never_overflows" TEST ONLY: the next launch runs without redo pass as if
                             the margin had been shown
     "dedup_tag_bits"        TEST ONLY: bits of the hash a table word of cmpr_deduplicate() carries beside the
                             sequence number (0..32, default 32).  At 0 every occupied slot of a chain passes
                             the tag test and is compared in full: the path a tag collision takes, a 2^-32
                             event otherwise
     "hamming_stage_refs"    TEST ONLY, cmpr_hamming_*(): references staged per LDS piece (0 = default: as many as
                             fit 16 KiB, at most 512; a larger value is clamped to that)
     "hamming_segments"      TEST ONLY: forces the number of segments a set-2 group is walked in (1..64; 0 = default:
                             automatic, from the number of query workgroups)
     "hamming_generic"       TEST ONLY: 1 sends every group through the long-sequence form (query words read from
                             global memory), 0 (default) only groups of more than 16 words per sequence
     "hamming_link_snapshot" TEST ONLY, cmpr_hamming_cluster*(): 1 (default) skips a match whose two staged root
                             snapshots agree, 0 sends every match to the forest; the partition is the same
     "edit_link_snapshot"    TEST ONLY, cmpr_edit_cluster*(): 1 (default) skips a match whose two staged root
                             snapshots agree, 0 sends every match to the forest; the partition is the same
     "edit_stage_refs"       TEST ONLY, cmpr_edit_*(): references staged per LDS piece (0 = default: as many match
                             vectors as fit 16 KiB, at most 512; a larger value is clamped to that)
     "edit_segments"         TEST ONLY: forces the number of segments every partner group is walked in (1..64; 0 =
                             default: automatic, from the number of query workgroups)
     "edit_words"            TEST ONLY: 2 or 4 forces at least that many 64-bit words per column, so that short
                             sequences run through the multiword forms; 0 (default): 1, 2 or 4 from the reference's
                             length
     "edit_nearest_prune"    TEST ONLY, cmpr_edit_nearest*(): 1 (default) a workgroup leaves its partners at the first
                             length gap no lane's smallest distance reaches; 0 walks every partner within the cap; the
                             results are the same
     "tcrdist_stage_refs"    TEST ONLY, cmpr_tcrdist_*(): references staged per LDS piece (0 = default: as many packed
                             sequences as fit 16 KiB, at most 512; a larger value is clamped to that)
     "tcrdist_segments"      TEST ONLY: forces the number of segments every partner group is walked in (1..64; 0 =
                             default: automatic, from the number of query workgroups)
   What locks when (a locked name is refused with CMPR_ESTATE; a value out of range with CMPR_EINVAL, whatever
   the state):
     before cmpr_set_reference():  "variant", "bloom_bits_log2_delta", "class_residues", "class_anchor",
                                   "heavy_threshold", "slice_words_log2", "d2_pairs", "d2_buffers", "table_log2_delta",
                                   "part_buckets_log2", "slice_pages", "page_budget", "fill_slices", "row_filter_x16"
     before cmpr_set_queries():    "chunk_tiles", "waves_per_block", "small_slice_tiles", "sub2_items",
                                   "class_rows_unstaged", "pos_segments", "pos_capacity", "work_shard_count",
                                   "work_shard_index", "record_tiles"
     at any time:                  every other name; "direct_slices_log2" takes effect at the next cmpr_set_queries()
   ("debug" exists only in a -DCMPR_ABLATION build of the library.) */
int cmpr_set_tunable(cmpr_context *ctx, const char *name, int64_t value);

/* Current value of a tunable (for the data-dependent ones, the value in effect
   after cmpr_set_reference / cmpr_set_queries), plus the read-only names
   "slices", "tiles", "chunks", "query_slots" (tiles x 64, padding included),
   "never_overflows" (1: the redo pass is currently dropped) and, of the last
   cmpr_set_queries* / cmpr_route_queries in microseconds, "layout_total_us",
   "layout_upload_us" (host time inside the copy calls) and "layout_tail_us" (from the
   last copy to the end: the device work the upload did not hide); host times of the parts of the last
   cmpr_neighbors*() in microseconds, each part ending in a wait: "neighbors_count_us", "neighbors_scan_us",
   "neighbors_fill_us", "neighbors_order_us" (a cmpr_existence_csr*() call sets the first three and zeroes the
   fourth); and of the last cmpr_existence_csr*(): "existence_edges_us" (those three together),
   "existence_group_us" (rows sorted by repertoire, cells per row), "existence_count_us" (their sum, the cell count
   to the host), "existence_reduce_us" (the cells; 0 when they did not fit) and "existence_copy_us" (host variant);
   and of the last cmpr_cluster_table*(), host times, each part ending in a wait: "cluster_links_us" (the set as
   both sets, the link step, labels and sizes flat on the device) and "cluster_table_us" (everything after: the
   numbering, the members, the counts and, in the host variant, their copies); and of the last cmpr_hamming_*(),
   host times, each part ending in a wait: "hamming_group_us" (upload, validation, keys, sort, groups, packing),
   "hamming_compare_us" (the compare kernel: once for a matrix, the count step, the sum and the fill step for
   neighbours; for cmpr_hamming_cluster*() the link kernel, the flatten and the sizes) and "hamming_copy_us" (host
   variant: the results copied out).  cmpr_hamming_cluster_table*() set these three as well, zero
   "cluster_links_us" and set "cluster_table_us" (the table pass, its copies included: "hamming_copy_us" stays 0);
   and of the last cmpr_edit_*(), host times, each part ending in a wait: "edit_group_us" (upload, validation, keys,
   sort, groups, packing, the jobs), "edit_compare_us" (the compare kernel: once for a matrix, the count step, the sum
   and the fill step for neighbours; for cmpr_edit_cluster*() the link kernel, the flatten and the sizes),
   "edit_order_us" (the rows sorted; 0 for a matrix, for clusters or when nothing was filled) and "edit_copy_us" (host
   variant: the results copied out).  cmpr_edit_cluster_table*() set these four as well, zero "cluster_links_us" and
   set "cluster_table_us" (the table pass, its copies included: "edit_copy_us" stays 0); cmpr_edit_nearest*() set
   "edit_group_us", "edit_compare_us" (the walk, the fold of the slots, the count of the found) and "edit_copy_us" and
   zero "edit_order_us"; no cmpr_edit_*() call touches the "hamming_*_us" timers; and of the last cmpr_tcrdist_*(), with
   the meaning of their edit_* twins: "tcrdist_group_us", "tcrdist_compare_us", "tcrdist_order_us" and
   "tcrdist_copy_us" (no cmpr_tcrdist_*() call touches the timers of another family). */
int cmpr_get_tunable(cmpr_context *ctx, const char *name, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif
