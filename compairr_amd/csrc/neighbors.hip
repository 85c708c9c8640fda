/*
 * neighbors.hip -- who matched whom, as CSR.  cmpr_neighbors / cmpr_neighbors_device: the pairs the reference
 * appends to its list in find_variant_matches (overlap.cc:232-245), per query and in increasing order of the
 * hit: row_start[n1 + 1] and the hits of row i in [row_start[i], row_start[i + 1]).  Exact, the same bits from
 * run to run and under every tunable, and without a capacity the caller has to guess.
 *
 * The resident sets are stepped over twice; the edges never exist anywhere but in their rows:
 *
 *   count   one synchronous step in neighbour mode (kernels.h score_match): degree[query] += 1 per match
 *   scan    row_start = exclusive 64-bit sum of the n1 + 1 degree words (the last one is zero, so
 *           row_start[n1] is the edge count), hipcub; behind it rows_census_kernel (csr_rows.h) counts the rows
 *           beyond a wave and beyond LDS.  The edge count and the census reach the host together: the call's one wait between
 *           the two steps, after which it knows whether `capacity` suffices and what the ordering will need
 *   fill    the step again: slot = row_start[q] + (atomicSub(degree + q, 1) - 1), hit[slot] = the hit.  The
 *           degree words are the cursors; every word is zero afterwards
 *   order   each row sorted in place (below)
 *
 * run_step_and_wait repeats a step whose no-redo shortcut overflowed.  What the first attempt counted or
 * placed must not survive: the hook in front of EVERY attempt zeroes the degrees (count) or sets them to the
 * row lengths again (fill, nb_cursor_kernel).
 *
 * Ordering the rows.  Which hit takes which place of its row depends on the schedule; the set of hits of a
 * row does not, and a row never holds a sequence twice, so sorting the rows makes the result unique.  The four
 * paths by row length and their thresholds (8, 64, 8192) are those of csr_rows.h, with the hit itself as the key:
 * rows of up to 8192 hits by rows_sort (a lane, a wave, a workgroup in 32 KiB of LDS), and each longer row
 * through hipcub::DeviceRadixSort into a scratch buffer the size of the longest of them and back.
 *
 * Device memory for the duration of the call: 4 bytes per query (degrees), the scan's scratch, 4 bytes per
 * row beyond a wave, and for rows beyond LDS 24 bytes each plus the longest of them once plus the radix
 * sort's scratch.  The host variant adds what the device variant is handed: 8 bytes per query for row_start
 * and 4 per edge for the hits.  Everything is freed before the call returns, also when it fails.
 *
 * cmpr_neighbors_distance / _device: the same call with one byte beside every hit, the reference's --distance of
 * the pair (overlap.cc:491-502).  Count, scan and census are the same code; the fill step also has nb_dist, and the
 * lane that places a hit writes the distance of the kind its variant was verified as beside it (kernels.h
 * kind_distance); the rows are ordered by the 64-bit key hit << 8 | distance (HitDistRows: 64 KiB of LDS on the
 * workgroup path, as existence.hip), and the rows beyond LDS through hipcub::DeviceRadixSort::SortPairs -- key the hit, value
 * the byte -- and back.  On top of the figures above: one byte per edge (the host variant holds them on the device
 * for the call), and for rows beyond LDS one byte per hit of the longest of them and the scratch of the pair sort.
 *
 * cmpr_neighbor_edges (context.h) hands count, scan and fill -- the rows not ordered -- to a caller inside the
 * library that orders them its own way (existence.hip).
 */
#include "csr_rows.h"

#include <hipcub/hipcub.hpp>

using namespace cmpr;

namespace {

/* the fill step's cursors: the hits of row i still to come */
__global__ void __launch_bounds__(ROW_WG)
nb_cursor_kernel(const uint64_t *row_start, uint32_t *degree, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * ROW_WG + threadIdx.x;
  if (i < n)
    degree[i] = (uint32_t)(row_start[i + 1] - row_start[i]);
}

/* ---- count; scan, census ---- the degrees and the scan's scratch are allocated here; e.row_start is n1 + 1 words of
   device memory, and a host array of the caller's receives them in the same wait that brings the edge count and the
   census */
int nb_count(cmpr_context *c, NeighborEdges &e)
{
  int rc;
  const uint64_t n1 = c->n1;
  uint64_t *const row_start = e.row_start.p;
  /* TEST ONLY (tunable "assume_never_overflows"): the pretence is used up by the first launch it meets; it is
     renewed for the fill step, so that the repeat of either step can be provoked (tests/test_neighbors_gpu.py) */
  e.pretend_no_redo = c->force_no_redo;
  for (double &t : c->nb_ms)
    t = 0;
  if ((rc = dev_alloc(c, e.degree, (size_t)(n1 + 1)))) return rc;
  if ((rc = dev_alloc(c, e.census, 5))) return rc;      /* [0..2] the census, [3..4] the list counters */
  uint32_t *const degree = e.degree.p;
  hipcub::TransformInputIterator<unsigned long long, U32To64, const uint32_t *> wide(degree, U32To64());
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, e.scan_bytes, wide, (unsigned long long *)row_start,
                                              (size_t)(n1 + 1), c->stream));
  if ((rc = dev_alloc(c, e.scan_tmp, e.scan_bytes))) return rc;

  auto t0 = std::chrono::steady_clock::now();
  if ((rc = cmpr_neighbor_step(c, degree, nullptr, nullptr, nullptr, [&]() -> int {
         HIP_TRY(c, hipMemsetAsync(degree, 0, (size_t)(n1 + 1) * sizeof(uint32_t), c->stream));
         return CMPR_OK;
       })))
    return rc;
  c->nb_ms[0] = ms_since(t0);

  t0 = std::chrono::steady_clock::now();
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(e.scan_tmp.p, e.scan_bytes, wide, (unsigned long long *)row_start,
                                              (size_t)(n1 + 1), c->stream));
  if ((rc = rows_census(c, row_start, n1, e.census.p))) return rc;
  unsigned long long total = 0, seen[3] = {0, 0, 0};
  HIP_TRY(c, hipMemcpyAsync(&total, row_start + n1, sizeof total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(seen, e.census.p, sizeof seen, hipMemcpyDeviceToHost, c->stream));
  if ((rc = e.row_start.copy_out(c, (size_t)(n1 + 1)))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->nb_ms[1] = ms_since(t0);
  e.total = total;
  e.n_long = seen[1];
  e.n_big = seen[0] - seen[1];
  e.longest = seen[2];
  return CMPR_OK;
}

/* ---- fill ---- every hit into its row of e.hit, in the order of arrival; dist (or NULL): its distance beside it */
int nb_fill(cmpr_context *c, NeighborEdges &e, uint8_t *dist)
{
  int rc;
  const uint64_t n1 = c->n1;
  const uint64_t *const row_start = e.row_start.p;
  uint32_t *const hit = e.hit.p;
  uint32_t *const degree = e.degree.p;
  if (e.pretend_no_redo) {
    c->force_no_redo = true;
    c->usage_pending = false;
  }
  const auto t0 = std::chrono::steady_clock::now();
  if ((rc = cmpr_neighbor_step(c, degree, row_start, hit, dist, [&]() -> int {
         hipLaunchKernelGGL(nb_cursor_kernel, dim3(blocks_for(n1, ROW_WG)), dim3(ROW_WG), 0, c->stream, row_start, degree, n1);
         HIP_TRY(c, hipGetLastError());
         return CMPR_OK;
       })))
    return rc;
  c->nb_ms[2] = ms_since(t0);
  return CMPR_OK;
}

/* with_dist: cmpr_neighbors_distance, dist_out beside hit_out; otherwise dist_out is NULL */
int neighbors_impl(cmpr_context *c, uint64_t capacity, uint64_t *row_start_out, uint32_t *hit_out, uint8_t *dist_out,
                   uint64_t *n_edges_out, bool on_device, bool with_dist)
{
  if (!c)
    return CMPR_EINVAL;
  const std::string who = with_dist ? "cmpr_neighbors_distance" : "cmpr_neighbors";
  if (!n_edges_out)
    return fail(c, CMPR_EINVAL, who + ": n_edges_out is NULL");
  *n_edges_out = 0;
  if (capacity && !hit_out)
    return fail(c, CMPR_EINVAL, who + ": hit_out is NULL with a capacity");
  if (with_dist && capacity && !dist_out)
    return fail(c, CMPR_EINVAL, who + ": distance_out is NULL with a capacity");
  int rc;
  if ((rc = cmpr_check_ready(c)))
    return rc;
  if (c->work_shard_count > 1)
    return fail(c, CMPR_EUNSUPPORTED, who + ": a work shard holds part of each row (work_shard_count > 1)");
  if (c->routed)
    return fail(c, CMPR_EUNSUPPORTED, who + ": a routed query set holds part of each row (cmpr_set_queries_routed)");
  const uint64_t n1 = c->n1;

  NeighborEdges e(row_start_out, hit_out, on_device);
  Out<uint8_t> dist_o(dist_out, on_device);
  if ((rc = e.row_start.temp(c, (size_t)(n1 + 1)))) return rc;
  if ((rc = nb_count(c, e)))
    return rc;
  const uint64_t total = e.total;
  *n_edges_out = total;
  /* degrees only, nothing to list, or no room for it: row_start says what to allocate */
  if (!hit_out || (with_dist && !dist_out) || total == 0 || total > capacity)
    return CMPR_OK;

  /* what the ordering needs is allocated in front of the fill */
  RowOrder<uint8_t> order;
  if ((rc = e.hit.temp(c, (size_t)total))) return rc;
  if (with_dist && (rc = dist_o.temp(c, (size_t)total))) return rc;
  if ((rc = order.reserve(c, e.n_big, e.n_long, e.longest, with_dist))) return rc;
  if ((rc = nb_fill(c, e, dist_o.p)))
    return rc;

  /* ---- order the rows ---- */
  auto t0 = std::chrono::steady_clock::now();
  if ((rc = order.run(c, who.c_str(), e.row_start.p, n1, total, e.census.p + 3, e.hit.p, dist_o.p)))
    return rc;
  if ((rc = e.hit.copy_out(c, (size_t)total))) return rc;
  if ((rc = dist_o.copy_out(c, (size_t)total))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->nb_ms[3] = ms_since(t0);
  return CMPR_OK;
}

}  // namespace

int cmpr_neighbor_edges(cmpr_context *c, NeighborEdges &e)
{
  int rc;
  if ((rc = e.row_start.temp(c, (size_t)(c->n1 + 1)))) return rc;
  if ((rc = nb_count(c, e))) return rc;
  if (e.total == 0)
    return CMPR_OK;
  if ((rc = e.hit.temp(c, (size_t)e.total))) return rc;
  return nb_fill(c, e, nullptr);
}

extern "C" int cmpr_neighbors(cmpr_context *c, uint64_t capacity, uint64_t *row_start_out, uint32_t *hit_out,
                              uint64_t *n_edges_out)
{
  return guarded(c, [&] { return neighbors_impl(c, capacity, row_start_out, hit_out, nullptr, n_edges_out, false, false); });
}

extern "C" int cmpr_neighbors_device(cmpr_context *c, uint64_t capacity, uint64_t *d_row_start_out,
                                     uint32_t *d_hit_out, uint64_t *n_edges_out)
{
  return guarded(c, [&] {
    return neighbors_impl(c, capacity, d_row_start_out, d_hit_out, nullptr, n_edges_out, true, false);
  });
}

extern "C" int cmpr_neighbors_distance(cmpr_context *c, uint64_t capacity, uint64_t *row_start_out, uint32_t *hit_out,
                                       uint8_t *distance_out, uint64_t *n_edges_out)
{
  return guarded(c, [&] {
    return neighbors_impl(c, capacity, row_start_out, hit_out, distance_out, n_edges_out, false, true);
  });
}

extern "C" int cmpr_neighbors_distance_device(cmpr_context *c, uint64_t capacity, uint64_t *d_row_start_out,
                                              uint32_t *d_hit_out, uint8_t *d_distance_out, uint64_t *n_edges_out)
{
  return guarded(c, [&] {
    return neighbors_impl(c, capacity, d_row_start_out, d_hit_out, d_distance_out, n_edges_out, true, true);
  });
}
