"""ctypes binding of the C ABI in ``include/compairr_hip.h``.

There is deliberately no fallback: if ``libcompairr_hip.so`` has not been built
(``make lib`` / ``__graft_entry__.build()``) or no HIP device is present, the
calls fail loudly."""

from __future__ import annotations

import contextlib
import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .sets import RepertoireSet

SCORES = {"product": 0, "ratio": 1, "min": 2, "max": 3, "mean": 4, "mh": 5, "jaccard": 6}

EXPORTS = [
    "cmpr_abi_version", "cmpr_create", "cmpr_destroy", "cmpr_last_error",
    "cmpr_set_reference", "cmpr_set_queries", "cmpr_overlap_matrix",
    "cmpr_overlap_matrix_f64", "cmpr_overlap_matrix_device", "cmpr_get_stats",
    "cmpr_get_kernel_times",
    "cmpr_rows", "cmpr_cols", "cmpr_set_tunable", "cmpr_get_tunable",
    "cmpr_count_duplicates", "cmpr_overlap_pairs",
    "cmpr_set_reference_device", "cmpr_set_queries_device",
    "cmpr_route_queries", "cmpr_route_pack", "cmpr_set_queries_routed",
    "cmpr_warm_up", "cmpr_warm_up_sized",
    "cmpr_deduplicate", "cmpr_deduplicate_device",
    "cmpr_cluster", "cmpr_cluster_device",
    "cmpr_neighbors", "cmpr_neighbors_device",
    "cmpr_existence_csr", "cmpr_existence_csr_device",
    "cmpr_cluster_table", "cmpr_cluster_table_device",
    "cmpr_neighbors_distance", "cmpr_neighbors_distance_device",
    "cmpr_hamming_matrix", "cmpr_hamming_matrix_device",
    "cmpr_hamming_neighbors", "cmpr_hamming_neighbors_device",
    "cmpr_hamming_cluster", "cmpr_hamming_cluster_device",
    "cmpr_hamming_cluster_table", "cmpr_hamming_cluster_table_device",
    "cmpr_hamming_nearest", "cmpr_hamming_nearest_device",
    "cmpr_edit_neighbors", "cmpr_edit_neighbors_device",
    "cmpr_edit_matrix", "cmpr_edit_matrix_device",
    "cmpr_edit_cluster", "cmpr_edit_cluster_device",
    "cmpr_edit_cluster_table", "cmpr_edit_cluster_table_device",
    "cmpr_edit_nearest", "cmpr_edit_nearest_device",
    "cmpr_tcrdist_neighbors", "cmpr_tcrdist_neighbors_device",
    "cmpr_tcrdist_matrix", "cmpr_tcrdist_matrix_device",
]

NEAREST_OTHER_REPERTOIRE = 1      # CMPR_NEAREST_OTHER_REPERTOIRE
UNCAPPED = 2 ** 63 - 1            # max_distance of cmpr_edit_nearest*: above every sequence, no cap
NO_NEAREST = 0xFFFFFFFF           # nearest of a sequence without a candidate (its ties are 0, its distance 0xFFFF)
GAP_FIXED, GAP_SLIDING = 0, 1     # CMPR_GAP_FIXED, CMPR_GAP_SLIDING


class HipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("libcompairr_hip error %d: %s" % (code, msg))
        self.code = code


class _Options(C.Structure):
    _fields_ = [("differences", C.c_int32), ("indels", C.c_int32),
                ("ignore_genes", C.c_int32), ("ignore_counts", C.c_int32),
                ("score", C.c_int32), ("alphabet_size", C.c_int32),
                ("n_v_genes", C.c_uint32), ("n_j_genes", C.c_uint32),
                ("device", C.c_int32), ("existence", C.c_int32),
                ("reserved", C.c_int32 * 6)]


class _SetView(C.Structure):
    _fields_ = [("n", C.c_uint64), ("residues", C.c_void_p), ("offsets", C.c_void_p),
                ("v_gene", C.c_void_p), ("j_gene", C.c_void_p),
                ("repertoire", C.c_void_p), ("count", C.c_void_p),
                ("n_repertoires", C.c_uint32), ("reserved", C.c_uint32)]


class _Stats(C.Structure):
    _fields_ = [("queries", C.c_uint64), ("variants", C.c_uint64),
                ("bloom_positive", C.c_uint64), ("hash_equal", C.c_uint64),
                ("matches", C.c_uint64), ("algorithmic_bytes", C.c_uint64),
                ("kernel_ms", C.c_double), ("total_ms", C.c_double),
                ("kernel_launches", C.c_uint32), ("reserved", C.c_uint32),
                ("probe_ms", C.c_double), ("filter_reads", C.c_uint64)]


class _TcrdistParams(C.Structure):
    _fields_ = [("substitution", C.c_void_p), ("v_distance", C.c_void_p),
                ("gap_penalty", C.c_uint32), ("ntrim", C.c_uint32), ("ctrim", C.c_uint32), ("gap_mode", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class TcrdistParams:
    """The parameters of tcrdist_neighbors() / tcrdist_matrix() (include/compairr_hip.h: cmpr_tcrdist_params):
    `substitution` uint8[A, A] indexed [set-1 residue][set-2 residue] (A = 20), optionally `v_distance`
    uint16[n_v_genes, n_v_genes] indexed [set-1 V][set-2 V], the gap penalty per residue of length difference, the
    trims and the gap mode.  Shapes and dtypes are checked here -- a table is converted only where no value changes
    -- and the holder keeps the arrays the C struct points to alive."""

    def __init__(self, substitution, gap_penalty: int, ntrim: int = 3, ctrim: int = 2, gap_mode: int = GAP_FIXED,
                 v_distance=None):
        self.substitution = self._table(substitution, np.uint8, "substitution")
        if self.substitution.shape[0] != 20:
            raise ValueError("substitution must be 20 x 20 (amino acids)")
        self.v_distance = None if v_distance is None else self._table(v_distance, np.uint16, "v_distance")
        for name, value in (("gap_penalty", gap_penalty), ("ntrim", ntrim), ("ctrim", ctrim), ("gap_mode", gap_mode)):
            if not 0 <= int(value) < 2 ** 32:
                raise ValueError("%s must fit an unsigned 32-bit word" % name)
        self.gap_penalty, self.ntrim, self.ctrim, self.gap_mode = int(gap_penalty), int(ntrim), int(ctrim), int(gap_mode)

    @staticmethod
    def _table(a, dtype, name):
        a = np.asarray(a)
        if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] == 0:
            raise ValueError("%s must be a square table" % name)
        if a.dtype.kind not in "iu" or a.min() < 0 or a.max() > np.iinfo(dtype).max:
            raise ValueError("%s must hold integers that fit %s" % (name, np.dtype(dtype).name))
        return np.ascontiguousarray(a, dtype=dtype)

    def struct(self, opt: "Options") -> _TcrdistParams:
        """the C struct for a context of these options: the V table must have the context's V genes (a context of
        nucleotides is the library's to refuse)"""
        if self.v_distance is not None and self.v_distance.shape[0] != max(1, opt.n_v_genes):
            raise ValueError("v_distance must be n_v_genes x n_v_genes")
        t = _TcrdistParams()
        t.substitution = self.substitution.ctypes.data
        t.v_distance = None if self.v_distance is None else self.v_distance.ctypes.data
        t.gap_penalty, t.ntrim, t.ctrim, t.gap_mode = self.gap_penalty, self.ntrim, self.ctrim, self.gap_mode
        return t


@dataclass
class Options:
    differences: int = 0
    indels: bool = False
    ignore_genes: bool = False
    ignore_counts: bool = False
    score: str = "product"
    nucleotides: bool = False
    n_v_genes: int = 1
    n_j_genes: int = 1
    device: int = -1
    existence: bool = False


@dataclass
class Stats:
    queries: int
    variants: int
    bloom_positive: int
    hash_equal: int
    matches: int
    algorithmic_bytes: int
    kernel_ms: float
    total_ms: float
    kernel_launches: int
    probe_ms: float = 0.0
    filter_reads: int = 0


def library_path() -> str:
    env = os.environ.get("COMPAIRR_HIP_LIB")
    if env:
        return env
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                        "libcompairr_hip.so")


_lib = None


def _argtypes() -> dict:
    """argtypes per entry point; a host variant and its _device twin that take the same arguments are written once."""
    ctx = ptr = C.c_void_p
    opts, view, u64p = C.POINTER(_Options), C.POINTER(_SetView), C.POINTER(C.c_uint64)
    tcr = C.POINTER(_TcrdistParams)
    table = {
        "cmpr_create": [opts, C.POINTER(C.c_void_p)],
        "cmpr_destroy": [ctx],
        "cmpr_last_error": [ctx],
        "cmpr_set_reference": [ctx, view, C.c_uint32],
        "cmpr_set_reference_device": [ctx, view, C.c_uint32],
        "cmpr_set_queries": [ctx, view],
        "cmpr_set_queries_device": [ctx, view],
        "cmpr_route_queries": [ctx, view, C.c_uint64, C.c_uint32, u64p, C.POINTER(C.c_uint32), ptr],
        "cmpr_route_pack": [ctx, ptr, C.c_uint64],
        "cmpr_set_queries_routed": [ctx, ptr, C.c_uint64, C.c_uint32, C.c_uint64, ptr],
        "cmpr_overlap_matrix": [ctx, ptr],
        "cmpr_overlap_matrix_f64": [ctx, ptr],
        "cmpr_overlap_matrix_device": [ctx, ptr, ptr],
        "cmpr_get_stats": [ctx, C.POINTER(_Stats)],
        "cmpr_get_kernel_times": [ctx, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(C.c_uint32)],
        "cmpr_overlap_pairs": [ctx, C.c_uint64, ptr, ptr, u64p],
        "cmpr_count_duplicates": [ctx, view, u64p],
        "cmpr_rows": [ctx],
        "cmpr_cols": [ctx],
        "cmpr_set_tunable": [ctx, C.c_char_p, C.c_int64],
        "cmpr_get_tunable": [ctx, C.c_char_p, C.POINTER(C.c_int64)],
        "cmpr_warm_up": [opts],
        "cmpr_warm_up_sized": [opts, C.c_uint64, C.c_uint64, C.c_uint64],
    }
    twins = {
        "cmpr_deduplicate": [ctx, view, C.c_uint64, ptr, ptr, u64p, u64p],
        "cmpr_cluster": [ctx, view, ptr, ptr, u64p],
        "cmpr_neighbors": [ctx, C.c_uint64, ptr, ptr, u64p],
        "cmpr_existence_csr": [ctx, C.c_uint64, ptr, ptr, ptr, u64p],
        "cmpr_cluster_table": [ctx, view, ptr, ptr, ptr, ptr, u64p],
        "cmpr_neighbors_distance": [ctx, C.c_uint64, ptr, ptr, ptr, u64p],
        "cmpr_hamming_matrix": [ctx, view, view, C.c_int64, ptr],
        "cmpr_hamming_neighbors": [ctx, view, view, C.c_int64, C.c_uint64, ptr, ptr, ptr, u64p],
        "cmpr_hamming_cluster": [ctx, view, C.c_int64, ptr, ptr, u64p],
        "cmpr_hamming_cluster_table": [ctx, view, C.c_int64, ptr, ptr, ptr, ptr, u64p],
        "cmpr_hamming_nearest": [ctx, view, view, C.c_int64, C.c_uint32, ptr, ptr, ptr, u64p],
        "cmpr_edit_neighbors": [ctx, view, view, C.c_int64, C.c_uint64, ptr, ptr, ptr, u64p],
        "cmpr_edit_matrix": [ctx, view, view, C.c_int64, ptr],
        "cmpr_edit_cluster": [ctx, view, C.c_int64, ptr, ptr, u64p],
        "cmpr_edit_cluster_table": [ctx, view, C.c_int64, ptr, ptr, ptr, ptr, u64p],
        "cmpr_edit_nearest": [ctx, view, view, C.c_int64, C.c_int64, C.c_uint32, ptr, ptr, ptr, u64p],
        "cmpr_tcrdist_neighbors": [ctx, view, view, tcr, C.c_int64, C.c_uint64, ptr, ptr, ptr, u64p],
        "cmpr_tcrdist_matrix": [ctx, view, view, tcr, C.c_int64, ptr],
    }
    for name, args in twins.items():
        table[name] = table[name + "_device"] = args
    return table


def load_library() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    # torch (used by the tests and bench.py for device buffers, streams and
    # torch.distributed) bundles its own libamdhip64 with the same SONAME; two HIP
    # runtimes in one process do not both see the GPU.  Loading torch first
    # makes this library bind to the runtime torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            "%s is missing: build it with `make lib` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback." % path)
    lib = C.CDLL(path)
    # (additions do not bump the ABI version: a version-5 library built before an entry point lacks it, and only the
    # callers of that entry point fail on it, with AttributeError -- tools/*_timing.py --against run the parent
    # commit's build through this binding)
    for name, args in _argtypes().items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.argtypes = args
    lib.cmpr_abi_version.restype = C.c_int
    lib.cmpr_destroy.restype = None
    lib.cmpr_last_error.restype = C.c_char_p
    lib.cmpr_rows.restype = C.c_uint32
    lib.cmpr_cols.restype = C.c_uint32
    if lib.cmpr_abi_version() != 5:
        raise RuntimeError("libcompairr_hip.so ABI version mismatch")
    _lib = lib
    return lib


def _view(s: RepertoireSet) -> _SetView:
    v = _SetView()
    v.n = s.n
    v.residues = s.residues.ctypes.data
    v.offsets = s.offsets.ctypes.data
    v.v_gene = s.v_gene.ctypes.data
    v.j_gene = s.j_gene.ctypes.data
    v.repertoire = s.repertoire.ctypes.data
    v.count = s.count.ctypes.data
    v.n_repertoires = s.n_repertoires
    return v


class HipOverlap:
    """One context of the C ABI: create -> set_reference -> set_queries ->
    overlap_matrix*, mirroring the reference's overlap() around sim_thread
    (/root/reference/src/overlap.cc:840-938)."""

    def __init__(self, opt: Options):
        self._lib = load_library()
        o = _Options()
        o.differences = opt.differences
        o.indels = int(opt.indels)
        o.ignore_genes = int(opt.ignore_genes)
        o.ignore_counts = int(opt.ignore_counts)
        o.score = SCORES[opt.score.lower()]
        o.alphabet_size = 4 if opt.nucleotides else 20
        o.n_v_genes = opt.n_v_genes
        o.n_j_genes = opt.n_j_genes
        o.device = opt.device
        o.existence = int(opt.existence)
        self.opt = opt
        self._ctx = C.c_void_p()
        rc = self._lib.cmpr_create(C.byref(o), C.byref(self._ctx))
        if rc:
            raise HipError(rc, self._lib.cmpr_last_error(None).decode())

    def _check(self, rc: int) -> None:
        if rc:
            raise HipError(rc, self._lib.cmpr_last_error(self._ctx).decode())

    def close(self) -> None:
        if self._ctx:
            self._lib.cmpr_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tunable(self, name: str, value: int) -> None:
        self._check(self._lib.cmpr_set_tunable(self._ctx, name.encode(), value))

    def get_tunable(self, name: str) -> int:
        v = C.c_int64()
        self._check(self._lib.cmpr_get_tunable(self._ctx, name.encode(), C.byref(v)))
        return v.value

    def layout(self) -> dict:
        return {k: self.get_tunable(k) for k in
                ("variant", "slices", "slice_words_log2", "class_residues",
                 "bloom_bits_log2_delta", "waves_per_block", "chunk_tiles",
                 "tiles", "chunks", "small_tiles", "query_slots", "class_anchor", "d2_pairs")}

    def set_reference(self, s: RepertoireSet, longest_query: int = 0) -> None:
        v = _view(s)
        self._check(self._lib.cmpr_set_reference(self._ctx, C.byref(v), longest_query))

    def set_queries(self, s: RepertoireSet) -> None:
        v = _view(s)
        self._check(self._lib.cmpr_set_queries(self._ctx, C.byref(v)))

    # ---- sets that already live in HBM (include/compairr_hip.h: cmpr_set_*_device) ----

    @staticmethod
    def device_view(s: RepertoireSet, device="cuda"):
        """(view of device pointers, the torch tensors that own the memory) of a set copied to
        the GPU with torch -- the stand-in for a caller whose sets live in HBM."""
        import torch
        keep = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(device)
                for a in (s.residues, s.offsets, s.v_gene, s.j_gene, s.repertoire, s.count)]
        v = _SetView()
        v.n = s.n
        (v.residues, v.offsets, v.v_gene, v.j_gene, v.repertoire, v.count) = [t.data_ptr() for t in keep]
        v.n_repertoires = s.n_repertoires
        torch.cuda.synchronize()
        return v, keep

    def set_reference_device(self, view: _SetView, longest_query: int = 0) -> None:
        self._check(self._lib.cmpr_set_reference_device(self._ctx, C.byref(view), longest_query))

    def set_queries_device(self, view: _SetView) -> None:
        self._check(self._lib.cmpr_set_queries_device(self._ctx, C.byref(view)))

    # ---- one query set over N contexts (cmpr_route_queries / _pack / cmpr_set_queries_routed) ----

    def route_queries(self, share: RepertoireSet, first_index: int, n_dest: int):
        """Key `share` (its first sequence is number `first_index` of the whole set); returns
        (records per destination, bytes per record, duplicate_count totals per repertoire)."""
        v = _view(share)
        counts = (C.c_uint64 * n_dest)()
        rb = C.c_uint32()
        tot = np.zeros(share.n_repertoires, dtype=np.float64)
        self._check(self._lib.cmpr_route_queries(self._ctx, C.byref(v), first_index, n_dest, counts,
                                                 C.byref(rb), tot.ctypes.data))
        return np.array(list(counts), dtype=np.int64), rb.value, tot

    def route_pack(self, d_send: int, capacity_bytes: int) -> None:
        self._check(self._lib.cmpr_route_pack(self._ctx, C.c_void_p(d_send), capacity_bytes))

    def set_queries_routed(self, d_records: int, n_records: int, n_repertoires: int, n_total: int,
                           rep_totals: Optional[np.ndarray] = None) -> None:
        t = None if rep_totals is None else np.ascontiguousarray(rep_totals, dtype=np.float64)
        self._check(self._lib.cmpr_set_queries_routed(
            self._ctx, C.c_void_p(d_records), n_records, n_repertoires, n_total,
            None if t is None else t.ctypes.data))

    @property
    def shape(self):
        return (self._lib.cmpr_rows(self._ctx), self._lib.cmpr_cols(self._ctx))

    def overlap_matrix(self) -> np.ndarray:
        out = np.zeros(self.shape, dtype=np.uint64)
        self._check(self._lib.cmpr_overlap_matrix(self._ctx, out.ctypes.data))
        return out

    def overlap_matrix_f64(self) -> np.ndarray:
        out = np.zeros(self.shape, dtype=np.float64)
        self._check(self._lib.cmpr_overlap_matrix_f64(self._ctx, out.ctypes.data))
        return out

    def overlap_matrix_device(self, d_matrix: int, stream: Optional[int] = None) -> None:
        self._check(self._lib.cmpr_overlap_matrix_device(
            self._ctx, C.c_void_p(d_matrix), C.c_void_p(stream or 0)))

    def _count_then_fill(self, fn, head, n_rows, dtypes):
        """The capacity protocol of fn(ctx, *head, capacity, [row_start,] *arrays, &n): one count-only call, then one
        with the exact capacity.  n_rows: None for an entry point without row_start, else a callable that gives the
        number of rows; dtypes: per array its dtype, None for one that is not wanted.  Returns [row_start,] *arrays."""
        n = C.c_uint64()
        lead = [] if n_rows is None else [None]
        self._check(fn(self._ctx, *head, 0, *lead, *[None] * len(dtypes), C.byref(n)))
        if n_rows is not None:
            lead = [np.zeros(n_rows() + 1, dtype=np.uint64)]
        arrays = [None if dt is None else np.zeros(n.value, dtype=dt) for dt in dtypes]
        self._check(fn(self._ctx, *head, n.value, *[a.ctypes.data for a in lead],
                       *[a.ctypes.data if a is not None and n.value else None for a in arrays], C.byref(n)))
        assert n.value == len(arrays[0])
        return lead + arrays

    def _into_device(self, fn, view: _SetView, extra, *pointers) -> int:
        """fn(ctx, view, *extra, *device pointers (0: not wanted), &count) -> count"""
        out = C.c_uint64()
        self._check(fn(self._ctx, C.byref(view), *extra, *[C.c_void_p(p or None) for p in pointers], C.byref(out)))
        return out.value

    def _labels(self, fn, s: RepertoireSet, *extra):
        """cluster() / hamming_cluster(): fn(ctx, view, *extra, label, size, &n_clusters)"""
        v = _view(s)
        label = np.zeros(s.n, dtype=np.uint32)
        size = np.zeros(s.n, dtype=np.uint32)
        clusters = C.c_uint64()
        self._check(fn(self._ctx, C.byref(v), *extra, label.ctypes.data, size.ctypes.data, C.byref(clusters)))
        return label, size, clusters.value

    def _table(self, fn, s: RepertoireSet, *extra):
        """cluster_table() / hamming_cluster_table(): fn(ctx, view, *extra, the four arrays, &n_clusters)"""
        v = _view(s)
        cluster_of = np.zeros(s.n, dtype=np.uint32)
        cluster_start = np.zeros(s.n + 1, dtype=np.uint64)
        members = np.zeros(s.n, dtype=np.uint32)
        count = np.zeros(s.n, dtype=np.uint64)
        clusters = C.c_uint64()
        self._check(fn(self._ctx, C.byref(v), *extra, cluster_of.ctypes.data, cluster_start.ctypes.data,
                       members.ctypes.data, count.ctypes.data, C.byref(clusters)))
        k = clusters.value
        return cluster_of, cluster_start[:k + 1].copy(), members, count[:k].copy()

    def overlap_pairs(self) -> np.ndarray:
        """(query index, hit index) of every matching pair, sorted."""
        q, h = self._count_then_fill(self._lib.cmpr_overlap_pairs, (), None, (np.uint32, np.uint32))
        out = np.stack([q, h], axis=1)
        return out[np.lexsort((out[:, 1], out[:, 0]))]

    def count_duplicates(self, s: Optional[RepertoireSet] = None) -> int:
        """Exact duplicates inside `s` (None: the resident reference set)."""
        out = C.c_uint64()
        v = _view(s) if s is not None else None
        self._check(self._lib.cmpr_count_duplicates(
            self._ctx, C.byref(v) if v is not None else None, C.byref(out)))
        return out.value

    # ---- the duplicates of a set merged (include/compairr_hip.h: cmpr_deduplicate*) ----

    def deduplicate(self, s: RepertoireSet):
        """(first uint32[n_unique], count uint64[n_unique], merged): per class of equal entries of `s`, in
        increasing `first`, its smallest sequence number and its summed duplicate_count (with ignore_counts
        its size); merged = n - n_unique, the reference's "Duplicates merged:" (dedup.cc:192)."""
        v = _view(s)
        first = np.zeros(s.n, dtype=np.uint32)
        count = np.zeros(s.n, dtype=np.uint64)
        unique, merged = C.c_uint64(), C.c_uint64()
        self._check(self._lib.cmpr_deduplicate(self._ctx, C.byref(v), s.n, first.ctypes.data, count.ctypes.data,
                                               C.byref(unique), C.byref(merged)))
        return first[:unique.value].copy(), count[:unique.value].copy(), merged.value

    def deduplicate_device(self, view: _SetView, capacity: int = 0, d_first: int = 0, d_count: int = 0):
        """The same for a view of device pointers (device_view): up to `capacity` classes are written to the
        device arrays d_first (uint32) and d_count (uint64); returns (n_unique, merged).  capacity = 0 with no
        arrays only counts."""
        unique, merged = C.c_uint64(), C.c_uint64()
        self._check(self._lib.cmpr_deduplicate_device(
            self._ctx, C.byref(view), capacity, C.c_void_p(d_first or None), C.c_void_p(d_count or None),
            C.byref(unique), C.byref(merged)))
        return unique.value, merged.value

    # ---- the single-linkage clusters of a set (include/compairr_hip.h: cmpr_cluster*) ----

    def cluster(self, s: RepertoireSet):
        """(label uint32[n], size uint32[n], n_clusters): per sequence of `s` the smallest sequence number of
        its cluster and the number of members of that cluster -- the reference's --cluster (cluster.cc) without
        its output order.  Afterwards `s` is resident as both sets."""
        return self._labels(self._lib.cmpr_cluster, s)

    def cluster_device(self, view: _SetView, d_label: int = 0, d_size: int = 0) -> int:
        """The same for a view of device pointers (device_view): labels and sizes are written to the device
        arrays d_label and d_size (uint32[n] each; 0: not wanted); returns n_clusters."""
        return self._into_device(self._lib.cmpr_cluster_device, view, (), d_label, d_size)

    # ---- the clusters numbered and grouped (include/compairr_hip.h: cmpr_cluster_table*) ----

    def cluster_table(self, s: RepertoireSet):
        """(cluster_of uint32[n], cluster_start uint64[K + 1], members uint32[n], count uint64[K]): the clusters
        of `s` numbered by (size descending, smallest member ascending) -- the reference's cluster_no - 1 --, the
        members of cluster k, increasing, in members[cluster_start[k]:cluster_start[k + 1]], and its summed
        duplicate_count (with ignore_counts its size).  Afterwards `s` is resident as both sets."""
        return self._table(self._lib.cmpr_cluster_table, s)

    def cluster_table_device(self, view: _SetView, d_cluster_of: int = 0, d_cluster_start: int = 0,
                             d_member: int = 0, d_count: int = 0) -> int:
        """The same for a view of device pointers (device_view), into device arrays: d_cluster_of and d_member
        (uint32[n]), d_cluster_start (uint64[n + 1], K + 1 written) and d_count (uint64[n], K written); 0: not
        wanted.  Returns K."""
        return self._into_device(self._lib.cmpr_cluster_table_device, view, (), d_cluster_of, d_cluster_start,
                                 d_member, d_count)

    # ---- the pairs as neighbour lists in CSR (include/compairr_hip.h: cmpr_neighbors*) ----

    def neighbors(self):
        """(row_start uint64[n1 + 1], hits uint32[E]) of the resident sets: the hits of query i, in increasing
        order, are hits[row_start[i]:row_start[i + 1]] -- the pairs of overlap_pairs() without a sort on the
        host.  One degree-only call, then one with the exact capacity."""
        return tuple(self._count_then_fill(self._lib.cmpr_neighbors, (), self._queries, (np.uint32,)))

    def neighbors_device(self, capacity: int = 0, d_row_start: int = 0, d_hits: int = 0) -> int:
        """The same into device arrays: d_row_start (uint64[n1 + 1]; 0: not wanted) and d_hits
        (uint32[capacity]; 0 with capacity 0: degrees only).  Returns the edge count; when it exceeds
        `capacity` nothing was written to d_hits."""
        n = C.c_uint64()
        self._check(self._lib.cmpr_neighbors_device(self._ctx, capacity, C.c_void_p(d_row_start or None),
                                                    C.c_void_p(d_hits or None), C.byref(n)))
        return n.value

    # ---- ... with the distance of every edge (include/compairr_hip.h: cmpr_neighbors_distance*) ----

    def neighbors_distance(self):
        """(row_start uint64[n1 + 1], hits uint32[E], distance uint8[E]): neighbors() and, beside every hit, the
        reference's --distance of the pair -- the number of differing positions when both sequences have one
        length, else 1.  One degree-only call, then one with the exact capacity."""
        return tuple(self._count_then_fill(self._lib.cmpr_neighbors_distance, (), self._queries,
                                           (np.uint32, np.uint8)))

    def neighbors_distance_device(self, capacity: int = 0, d_row_start: int = 0, d_hits: int = 0,
                                  d_distance: int = 0) -> int:
        """The same into device arrays: d_row_start (uint64[n1 + 1]; 0: not wanted), d_hits (uint32[capacity])
        and d_distance (uint8[capacity]; both 0 with capacity 0: degrees only).  Returns the edge count; when it
        exceeds `capacity` nothing was written to d_hits or d_distance."""
        n = C.c_uint64()
        self._check(self._lib.cmpr_neighbors_distance_device(self._ctx, capacity, C.c_void_p(d_row_start or None),
                                                             C.c_void_p(d_hits or None),
                                                             C.c_void_p(d_distance or None), C.byref(n)))
        return n.value

    # ---- the -x table as CSR (include/compairr_hip.h: cmpr_existence_csr*) ----

    def existence_csr(self):
        """(row_start uint64[n1 + 1], repertoire uint32[C], value uint64[C]) of the resident sets: the nonzero
        cells of the per-sequence table -- row i of overlap_matrix() on a context with existence=True -- are
        repertoire[row_start[i]:row_start[i + 1]], in increasing order, with their values beside them.  Works on
        a context without `existence`, which never holds the dense table.  One count-only call, then one with
        the exact capacity."""
        return tuple(self._count_then_fill(self._lib.cmpr_existence_csr, (), self._queries,
                                           (np.uint32, np.uint64)))

    def existence_csr_device(self, capacity: int = 0, d_row_start: int = 0, d_repertoire: int = 0,
                             d_value: int = 0) -> int:
        """The same into device arrays: d_row_start (uint64[n1 + 1]; 0: not wanted), d_repertoire
        (uint32[capacity]) and d_value (uint64[capacity]; both 0 with capacity 0: count only).  Returns the
        number of cells; when it exceeds `capacity` nothing was written to the two cell arrays."""
        n = C.c_uint64()
        self._check(self._lib.cmpr_existence_csr_device(self._ctx, capacity, C.c_void_p(d_row_start or None),
                                                        C.c_void_p(d_repertoire or None),
                                                        C.c_void_p(d_value or None), C.byref(n)))
        return n.value

    # ---- the all-against-all path for any d (include/compairr_hip.h: cmpr_hamming_*) ----

    def hamming_matrix(self, set1: RepertoireSet, set2: RepertoireSet, differences: int) -> np.ndarray:
        """The R1 x R2 matrix (n1 x R2 with `existence`) of set1 against set2 over the pairs of equal length, equal
        V and J (unless ignore_genes) and at most `differences` differing positions -- the integer sums of
        overlap_matrix().  `set2 is set1`: one-file mode, the (i, i) pairs included.  The context's own
        `differences` and resident sets play no part."""
        v1 = _view(set1)
        v2 = v1 if set2 is set1 else _view(set2)
        rows = set1.n if self.opt.existence else set1.n_repertoires
        out = np.zeros((rows, set2.n_repertoires), dtype=np.uint64)
        self._check(self._lib.cmpr_hamming_matrix(self._ctx, C.byref(v1), C.byref(v2), differences, out.ctypes.data))
        return out

    def hamming_matrix_device(self, view1: _SetView, view2: _SetView, differences: int, d_matrix: int) -> None:
        """The same for views of device pointers (device_view; the same object twice: one-file mode) into the
        device array d_matrix (uint64[R1 * R2], or [n1 * R2] with `existence`)."""
        self._check(self._lib.cmpr_hamming_matrix_device(self._ctx, C.byref(view1), C.byref(view2), differences,
                                                         C.c_void_p(d_matrix or None)))

    def hamming_neighbors(self, set1: RepertoireSet, set2: RepertoireSet, differences: int, distances: bool = True):
        """(row_start uint64[n1 + 1], hits uint32[E], distance uint16[E] or None): the same pairs as CSR -- the
        hits of sequence i of set1, increasing, are hits[row_start[i]:row_start[i + 1]], the number of differing
        positions beside each.  One count-only call, then one with the exact capacity."""
        v1 = _view(set1)
        v2 = v1 if set2 is set1 else _view(set2)
        return tuple(self._count_then_fill(self._lib.cmpr_hamming_neighbors, (C.byref(v1), C.byref(v2), differences),
                                           lambda: set1.n, (np.uint32, np.uint16 if distances else None)))

    def hamming_neighbors_device(self, view1: _SetView, view2: _SetView, differences: int, capacity: int = 0,
                                 d_row_start: int = 0, d_hits: int = 0, d_distance: int = 0) -> int:
        """The same for views of device pointers into device arrays: d_row_start (uint64[n1 + 1]; 0: not wanted),
        d_hits (uint32[capacity]; 0 with capacity 0: count only) and d_distance (uint16[capacity]; 0: hits only).
        Returns the edge count; when it exceeds `capacity` nothing was written to d_hits or d_distance."""
        n = C.c_uint64()
        self._check(self._lib.cmpr_hamming_neighbors_device(
            self._ctx, C.byref(view1), C.byref(view2), differences, capacity, C.c_void_p(d_row_start or None),
            C.c_void_p(d_hits or None), C.c_void_p(d_distance or None), C.byref(n)))
        return n.value

    # ---- single-linkage clusters at any d (include/compairr_hip.h: cmpr_hamming_cluster*) ----

    def hamming_cluster(self, s: RepertoireSet, differences: int):
        """(label uint32[n], size uint32[n], n_clusters) of `s` as cluster() gives them, under the pair relation of
        hamming_neighbors(s, s, differences): any `differences` >= 0.  The context's own `differences` and
        resident sets play no part, and `s` is not resident afterwards."""
        return self._labels(self._lib.cmpr_hamming_cluster, s, differences)

    def hamming_cluster_device(self, view: _SetView, differences: int, d_label: int = 0, d_size: int = 0) -> int:
        """The same for a view of device pointers (device_view): labels and sizes are written to the device
        arrays d_label and d_size (uint32[n] each; 0: not wanted); returns n_clusters."""
        return self._into_device(self._lib.cmpr_hamming_cluster_device, view, (differences,), d_label, d_size)

    def hamming_cluster_table(self, s: RepertoireSet, differences: int):
        """(cluster_of uint32[n], cluster_start uint64[K + 1], members uint32[n], count uint64[K]) of `s` as
        cluster_table() gives them, under the pair relation of hamming_neighbors(s, s, differences)."""
        return self._table(self._lib.cmpr_hamming_cluster_table, s, differences)

    def hamming_cluster_table_device(self, view: _SetView, differences: int, d_cluster_of: int = 0,
                                     d_cluster_start: int = 0, d_member: int = 0, d_count: int = 0) -> int:
        """The same for a view of device pointers (device_view), into device arrays: d_cluster_of and d_member
        (uint32[n]), d_cluster_start (uint64[n + 1], K + 1 written) and d_count (uint64[n], K written); 0: not
        wanted.  Returns K."""
        return self._into_device(self._lib.cmpr_hamming_cluster_table_device, view, (differences,), d_cluster_of,
                                 d_cluster_start, d_member, d_count)

    # ---- the nearest neighbour at any distance (include/compairr_hip.h: cmpr_hamming_nearest*) ----

    def hamming_nearest(self, set1: RepertoireSet, set2: RepertoireSet, min_distance: int = 0,
                        other_repertoire: bool = False):
        """(nearest uint32[n1], distance uint16[n1], ties uint32[n1]): for every sequence of set1 the smallest
        distance over the sequences of set2 of its length, V and J (unless ignore_genes) that differ at
        `min_distance` or more positions, the smallest sequence number at that distance and how many lie at it.
        `set2 is set1`: one-set mode, a sequence is never its own neighbour; `other_repertoire` (one-set mode only)
        admits only sequences of another repertoire.  Nobody: (NO_NEAREST, 0xFFFF, 0)."""
        v1 = _view(set1)
        v2 = v1 if set2 is set1 else _view(set2)
        nearest = np.zeros(set1.n, dtype=np.uint32)
        distance = np.zeros(set1.n, dtype=np.uint16)
        ties = np.zeros(set1.n, dtype=np.uint32)
        self._check(self._lib.cmpr_hamming_nearest(
            self._ctx, C.byref(v1), C.byref(v2), min_distance, NEAREST_OTHER_REPERTOIRE if other_repertoire else 0,
            nearest.ctypes.data, distance.ctypes.data, ties.ctypes.data, None))
        return nearest, distance, ties

    def hamming_nearest_device(self, view1: _SetView, view2: _SetView, min_distance: int, flags: int,
                               d_nearest: int = 0, d_distance: int = 0, d_ties: int = 0) -> int:
        """The same for views of device pointers (device_view; the same object twice: one-set mode) into the device
        arrays d_nearest (uint32[n1]), d_distance (uint16[n1]) and d_ties (uint32[n1]); 0: not wanted.  Returns the
        number of sequences of set1 that have a neighbour."""
        n = C.c_uint64()
        self._check(self._lib.cmpr_hamming_nearest_device(
            self._ctx, C.byref(view1), C.byref(view2), min_distance, flags, C.c_void_p(d_nearest or None),
            C.c_void_p(d_distance or None), C.c_void_p(d_ties or None), C.byref(n)))
        return n.value

    # ---- the all-against-all path under edit distance (include/compairr_hip.h: cmpr_edit_*) ----

    def edit_neighbors(self, set1: RepertoireSet, set2: RepertoireSet, differences: int, distances: bool = True):
        """(row_start uint64[n1 + 1], hits uint32[E], distance uint16[E] or None): the pairs of equal V and J (unless
        ignore_genes) at a Levenshtein distance of at most `differences` as CSR -- the hits of sequence i of set1,
        increasing, are hits[row_start[i]:row_start[i + 1]], the distance beside each.  `set2 is set1`: one-file
        mode, the (i, i) pairs included.  The context's own `differences`, `indels` and resident sets play no part.
        One count-only call, then one with the exact capacity."""
        v1 = _view(set1)
        v2 = v1 if set2 is set1 else _view(set2)
        return tuple(self._count_then_fill(self._lib.cmpr_edit_neighbors, (C.byref(v1), C.byref(v2), differences),
                                           lambda: set1.n, (np.uint32, np.uint16 if distances else None)))

    def edit_neighbors_device(self, view1: _SetView, view2: _SetView, differences: int, capacity: int = 0,
                              d_row_start: int = 0, d_hits: int = 0, d_distance: int = 0) -> int:
        """The same for views of device pointers into device arrays: d_row_start (uint64[n1 + 1]; 0: not wanted),
        d_hits (uint32[capacity]; 0 with capacity 0: count only) and d_distance (uint16[capacity]; 0: hits only).
        Returns the edge count; when it exceeds `capacity` nothing was written to d_hits or d_distance."""
        n = C.c_uint64()
        self._check(self._lib.cmpr_edit_neighbors_device(
            self._ctx, C.byref(view1), C.byref(view2), differences, capacity, C.c_void_p(d_row_start or None),
            C.c_void_p(d_hits or None), C.c_void_p(d_distance or None), C.byref(n)))
        return n.value

    def edit_matrix(self, set1: RepertoireSet, set2: RepertoireSet, differences: int) -> np.ndarray:
        """The R1 x R2 matrix (n1 x R2 with `existence`) of set1 against set2 over the pairs of edit_neighbors() --
        the integer sums of hamming_matrix()."""
        v1 = _view(set1)
        v2 = v1 if set2 is set1 else _view(set2)
        rows = set1.n if self.opt.existence else set1.n_repertoires
        out = np.zeros((rows, set2.n_repertoires), dtype=np.uint64)
        self._check(self._lib.cmpr_edit_matrix(self._ctx, C.byref(v1), C.byref(v2), differences, out.ctypes.data))
        return out

    def edit_matrix_device(self, view1: _SetView, view2: _SetView, differences: int, d_matrix: int) -> None:
        """The same for views of device pointers (device_view; the same object twice: one-file mode) into the
        device array d_matrix (uint64[R1 * R2], or [n1 * R2] with `existence`)."""
        self._check(self._lib.cmpr_edit_matrix_device(self._ctx, C.byref(view1), C.byref(view2), differences,
                                                      C.c_void_p(d_matrix or None)))

    # ---- single-linkage clusters under edit distance at any d (include/compairr_hip.h: cmpr_edit_cluster*) ----

    def edit_cluster(self, s: RepertoireSet, differences: int):
        """(label uint32[n], size uint32[n], n_clusters) of `s` as cluster() gives them, under the pair relation of
        edit_neighbors(s, s, differences): any `differences` >= 0.  The context's own `differences`, `indels` and
        resident sets play no part, and `s` is not resident afterwards."""
        return self._labels(self._lib.cmpr_edit_cluster, s, differences)

    def edit_cluster_device(self, view: _SetView, differences: int, d_label: int = 0, d_size: int = 0) -> int:
        """The same for a view of device pointers (device_view): labels and sizes are written to the device
        arrays d_label and d_size (uint32[n] each; 0: not wanted); returns n_clusters."""
        return self._into_device(self._lib.cmpr_edit_cluster_device, view, (differences,), d_label, d_size)

    def edit_cluster_table(self, s: RepertoireSet, differences: int):
        """(cluster_of uint32[n], cluster_start uint64[K + 1], members uint32[n], count uint64[K]) of `s` as
        cluster_table() gives them, under the pair relation of edit_neighbors(s, s, differences)."""
        return self._table(self._lib.cmpr_edit_cluster_table, s, differences)

    def edit_cluster_table_device(self, view: _SetView, differences: int, d_cluster_of: int = 0,
                                  d_cluster_start: int = 0, d_member: int = 0, d_count: int = 0) -> int:
        """The same for a view of device pointers (device_view), into device arrays: d_cluster_of and d_member
        (uint32[n]), d_cluster_start (uint64[n + 1], K + 1 written) and d_count (uint64[n], K written); 0: not
        wanted.  Returns K."""
        return self._into_device(self._lib.cmpr_edit_cluster_table_device, view, (differences,), d_cluster_of,
                                 d_cluster_start, d_member, d_count)

    # ---- the nearest neighbour under edit distance (include/compairr_hip.h: cmpr_edit_nearest*) ----

    def edit_nearest(self, set1: RepertoireSet, set2: Optional[RepertoireSet] = None, min_distance: int = 1,
                     max_distance: Optional[int] = None, other_repertoire: bool = False):
        """(nearest uint32[n1], distance uint16[n1], ties uint32[n1]): for every sequence of set1 the smallest
        Levenshtein distance over the sequences of set2 of its V and J (unless ignore_genes), of any length, that lie
        at `min_distance` or more and at `max_distance` or less (None: uncapped), the smallest sequence number at
        that distance and how many lie at it.  `set2` None or `set2 is set1`: one-set mode, a sequence is never its
        own neighbour; `other_repertoire` (one-set mode only) admits only sequences of another repertoire.  Nobody:
        (NO_NEAREST, 0xFFFF, 0).  The context's own `differences`, `indels` and resident sets play no part."""
        v1 = _view(set1)
        v2 = v1 if set2 is None or set2 is set1 else _view(set2)
        nearest = np.zeros(set1.n, dtype=np.uint32)
        distance = np.zeros(set1.n, dtype=np.uint16)
        ties = np.zeros(set1.n, dtype=np.uint32)
        self._check(self._lib.cmpr_edit_nearest(
            self._ctx, C.byref(v1), C.byref(v2), min_distance, UNCAPPED if max_distance is None else max_distance,
            NEAREST_OTHER_REPERTOIRE if other_repertoire else 0, nearest.ctypes.data, distance.ctypes.data,
            ties.ctypes.data, None))
        return nearest, distance, ties

    def edit_nearest_device(self, view1: _SetView, view2: _SetView, min_distance: int, max_distance: Optional[int],
                            flags: int, d_nearest: int = 0, d_distance: int = 0, d_ties: int = 0) -> int:
        """The same for views of device pointers (device_view; the same object twice: one-set mode) into the device
        arrays d_nearest (uint32[n1]), d_distance (uint16[n1]) and d_ties (uint32[n1]); 0: not wanted.  Returns the
        number of sequences of set1 that have a neighbour."""
        n = C.c_uint64()
        self._check(self._lib.cmpr_edit_nearest_device(
            self._ctx, C.byref(view1), C.byref(view2), min_distance,
            UNCAPPED if max_distance is None else max_distance, flags, C.c_void_p(d_nearest or None),
            C.c_void_p(d_distance or None), C.c_void_p(d_ties or None), C.byref(n)))
        return n.value

    # ---- the all-against-all path under the weighted CDR3 distance (include/compairr_hip.h: cmpr_tcrdist_*) ----

    def tcrdist_neighbors(self, set1: RepertoireSet, set2: RepertoireSet, params: TcrdistParams, cutoff: int,
                          distances: bool = True):
        """(row_start uint64[n1 + 1], hits uint32[E], distance uint16[E] or None): the pairs at a weighted CDR3
        distance of at most `cutoff` under `params` as CSR -- the hits of sequence i of set1, increasing, are
        hits[row_start[i]:row_start[i + 1]], the distance beside each.  Without a V table the pairs share V and J
        (unless ignore_genes); with one any two V genes pair at the table's price.  `set2 is set1`: one-file mode,
        the (i, i) pairs included.  One count-only call, then one with the exact capacity."""
        v1 = _view(set1)
        v2 = v1 if set2 is set1 else _view(set2)
        t = params.struct(self.opt)
        return tuple(self._count_then_fill(self._lib.cmpr_tcrdist_neighbors,
                                           (C.byref(v1), C.byref(v2), C.byref(t), cutoff),
                                           lambda: set1.n, (np.uint32, np.uint16 if distances else None)))

    def tcrdist_neighbors_device(self, view1: _SetView, view2: _SetView, params: TcrdistParams, cutoff: int,
                                 capacity: int = 0, d_row_start: int = 0, d_hits: int = 0, d_distance: int = 0) -> int:
        """The same for views of device pointers into device arrays: d_row_start (uint64[n1 + 1]; 0: not wanted),
        d_hits (uint32[capacity]; 0 with capacity 0: count only) and d_distance (uint16[capacity]; 0: hits only);
        `params` stays host memory.  Returns the edge count; when it exceeds `capacity` nothing was written to
        d_hits or d_distance."""
        n = C.c_uint64()
        t = params.struct(self.opt)
        self._check(self._lib.cmpr_tcrdist_neighbors_device(
            self._ctx, C.byref(view1), C.byref(view2), C.byref(t), cutoff, capacity, C.c_void_p(d_row_start or None),
            C.c_void_p(d_hits or None), C.c_void_p(d_distance or None), C.byref(n)))
        return n.value

    def tcrdist_matrix(self, set1: RepertoireSet, set2: RepertoireSet, params: TcrdistParams, cutoff: int) -> np.ndarray:
        """The R1 x R2 matrix (n1 x R2 with `existence`) of set1 against set2 over the pairs of tcrdist_neighbors()
        -- the integer sums of edit_matrix()."""
        v1 = _view(set1)
        v2 = v1 if set2 is set1 else _view(set2)
        t = params.struct(self.opt)
        rows = set1.n if self.opt.existence else set1.n_repertoires
        out = np.zeros((rows, set2.n_repertoires), dtype=np.uint64)
        self._check(self._lib.cmpr_tcrdist_matrix(self._ctx, C.byref(v1), C.byref(v2), C.byref(t), cutoff,
                                                  out.ctypes.data))
        return out

    def tcrdist_matrix_device(self, view1: _SetView, view2: _SetView, params: TcrdistParams, cutoff: int,
                              d_matrix: int) -> None:
        """The same for views of device pointers (device_view; the same object twice: one-file mode) into the
        device array d_matrix (uint64[R1 * R2], or [n1 * R2] with `existence`)."""
        t = params.struct(self.opt)
        self._check(self._lib.cmpr_tcrdist_matrix_device(self._ctx, C.byref(view1), C.byref(view2), C.byref(t), cutoff,
                                                         C.c_void_p(d_matrix or None)))

    def _queries(self) -> int:
        return self.stats().queries

    def kernel_times(self, max_calls: int = 64):
        """(kernel_ms[], probe_ms[]) of the last calls, oldest first (HIP events)."""
        n = min(max_calls, 63)
        k = (C.c_double * n)()
        p = (C.c_double * n)()
        got = C.c_uint32(0)
        self._check(self._lib.cmpr_get_kernel_times(self._ctx, n, k, p, C.byref(got)))
        return list(k[:got.value]), list(p[:got.value])

    def stats(self) -> Stats:
        st = _Stats()
        self._check(self._lib.cmpr_get_stats(self._ctx, C.byref(st)))
        return Stats(st.queries, st.variants, st.bloom_positive, st.hash_equal,
                     st.matches, st.algorithmic_bytes, st.kernel_ms, st.total_ms,
                     st.kernel_launches, st.probe_ms, st.filter_reads)


@contextlib.contextmanager
def _context(opt: Options, tunables: Optional[dict] = None, set1: Optional[RepertoireSet] = None,
             set2: Optional[RepertoireSet] = None):
    """A context of its own for one convenience call: `tunables` set on it first, then (when given) set2 resident
    as the reference and set1 as the queries."""
    with HipOverlap(opt) as h:
        for name, value in (tunables or {}).items():
            h.set_tunable(name, value)
        if set2 is not None:
            h.set_reference(set2, set1.longest)
            h.set_queries(set1)
        yield h


def overlap(set1: RepertoireSet, set2: RepertoireSet, opt: Options):
    """Convenience: the whole path once; returns (cells as float64 in the
    reference's units, Stats)."""
    with _context(opt, None, set1, set2) as h:
        m = h.overlap_matrix_f64()
        return m, h.stats()


def deduplicate(s: RepertoireSet, opt: Options, tunables: Optional[dict] = None):
    """Convenience: (merged_set, merged) -- `s` with every class of equal entries reduced to its first
    member, which carries the class's summed count (the reference's --deduplicate, dedup.cc).  `tunables`
    are set on the context first (the result never depends on them)."""
    with _context(opt, tunables) as h:
        first, count, merged = h.deduplicate(s)
    out = s.subset(first)
    out.count = count
    return out, merged


def cluster(s: RepertoireSet, opt: Options, tunables: Optional[dict] = None):
    """Convenience: (label, size, n_clusters) of `s` under `opt` (HipOverlap.cluster) on a context of its
    own.  `tunables` are set on the context first (the result never depends on them)."""
    with _context(opt, tunables) as h:
        return h.cluster(s)


def cluster_table(s: RepertoireSet, opt: Options, tunables: Optional[dict] = None):
    """Convenience: (cluster_of, cluster_start, members, count) of `s` under `opt` (HipOverlap.cluster_table) on
    a context of its own.  `tunables` are set on the context first (the result never depends on them)."""
    with _context(opt, tunables) as h:
        return h.cluster_table(s)


def neighbors(set1: RepertoireSet, set2: RepertoireSet, opt: Options, tunables: Optional[dict] = None):
    """Convenience: (row_start, hits) of set1 against set2 under `opt` (HipOverlap.neighbors) on a context of
    its own.  `tunables` are set on the context first (the result never depends on them)."""
    with _context(opt, tunables, set1, set2) as h:
        return h.neighbors()


def neighbors_distance(set1: RepertoireSet, set2: RepertoireSet, opt: Options, tunables: Optional[dict] = None):
    """Convenience: (row_start, hits, distance) of set1 against set2 under `opt` (HipOverlap.neighbors_distance)
    on a context of its own.  `tunables` are set on the context first (the result never depends on them)."""
    with _context(opt, tunables, set1, set2) as h:
        return h.neighbors_distance()


def hamming_matrix(set1: RepertoireSet, set2: RepertoireSet, opt: Options, differences: int,
                   tunables: Optional[dict] = None):
    """Convenience: the matrix of set1 against set2 at any `differences` (HipOverlap.hamming_matrix) on a context
    of its own; `opt.differences` plays no part.  `tunables` are set on the context first (the result never
    depends on them)."""
    with _context(opt, tunables) as h:
        return h.hamming_matrix(set1, set2, differences)


def hamming_neighbors(set1: RepertoireSet, set2: RepertoireSet, opt: Options, differences: int,
                      tunables: Optional[dict] = None, distances: bool = True):
    """Convenience: (row_start, hits, distance) of set1 against set2 at any `differences`
    (HipOverlap.hamming_neighbors) on a context of its own; `opt.differences` plays no part.  `tunables` are set on
    the context first (the result never depends on them)."""
    with _context(opt, tunables) as h:
        return h.hamming_neighbors(set1, set2, differences, distances)


def hamming_cluster(s: RepertoireSet, opt: Options, differences: int, tunables: Optional[dict] = None):
    """Convenience: (label, size, n_clusters) of `s` at any `differences` (HipOverlap.hamming_cluster) on a context
    of its own; `opt.differences` plays no part.  `tunables` are set on the context first (the result never depends
    on them)."""
    with _context(opt, tunables) as h:
        return h.hamming_cluster(s, differences)


def hamming_cluster_table(s: RepertoireSet, opt: Options, differences: int, tunables: Optional[dict] = None):
    """Convenience: (cluster_of, cluster_start, members, count) of `s` at any `differences`
    (HipOverlap.hamming_cluster_table) on a context of its own; `opt.differences` plays no part.  `tunables` are
    set on the context first (the result never depends on them)."""
    with _context(opt, tunables) as h:
        return h.hamming_cluster_table(s, differences)


def hamming_nearest(set1: RepertoireSet, set2: RepertoireSet, opt: Options, min_distance: int = 0,
                    other_repertoire: bool = False, tunables: Optional[dict] = None):
    """Convenience: (nearest, distance, ties) of set1 against set2 (HipOverlap.hamming_nearest) on a context of its
    own; `opt.differences` plays no part.  `tunables` are set on the context first (the result never depends on
    them)."""
    with _context(opt, tunables) as h:
        return h.hamming_nearest(set1, set2, min_distance, other_repertoire)


def edit_neighbors(set1: RepertoireSet, set2: RepertoireSet, opt: Options, differences: int,
                   tunables: Optional[dict] = None, distances: bool = True):
    """Convenience: (row_start, hits, distance) of set1 against set2 at a Levenshtein distance of at most
    `differences` (HipOverlap.edit_neighbors) on a context of its own; `opt.differences` and `opt.indels` play no
    part.  `tunables` are set on the context first (the result never depends on them)."""
    with _context(opt, tunables) as h:
        return h.edit_neighbors(set1, set2, differences, distances)


def edit_matrix(set1: RepertoireSet, set2: RepertoireSet, opt: Options, differences: int,
                tunables: Optional[dict] = None):
    """Convenience: the matrix of set1 against set2 over the pairs at a Levenshtein distance of at most
    `differences` (HipOverlap.edit_matrix) on a context of its own; `opt.differences` and `opt.indels` play no
    part.  `tunables` are set on the context first (the result never depends on them)."""
    with _context(opt, tunables) as h:
        return h.edit_matrix(set1, set2, differences)


def edit_cluster(s: RepertoireSet, opt: Options, differences: int, tunables: Optional[dict] = None):
    """Convenience: (label, size, n_clusters) of `s` at a Levenshtein distance of at most `differences`
    (HipOverlap.edit_cluster) on a context of its own; `opt.differences` and `opt.indels` play no part.  `tunables`
    are set on the context first (the result never depends on them)."""
    with _context(opt, tunables) as h:
        return h.edit_cluster(s, differences)


def edit_cluster_table(s: RepertoireSet, opt: Options, differences: int, tunables: Optional[dict] = None):
    """Convenience: (cluster_of, cluster_start, members, count) of `s` at a Levenshtein distance of at most
    `differences` (HipOverlap.edit_cluster_table) on a context of its own; `opt.differences` and `opt.indels` play
    no part.  `tunables` are set on the context first (the result never depends on them)."""
    with _context(opt, tunables) as h:
        return h.edit_cluster_table(s, differences)


def edit_nearest(set1: RepertoireSet, set2: Optional[RepertoireSet], opt: Options, min_distance: int = 1,
                 max_distance: Optional[int] = None, other_repertoire: bool = False,
                 tunables: Optional[dict] = None):
    """Convenience: (nearest, distance, ties) of set1 against set2 under edit distance (HipOverlap.edit_nearest) on a
    context of its own; `opt.differences` and `opt.indels` play no part.  `tunables` are set on the context first (the
    result never depends on them)."""
    with _context(opt, tunables) as h:
        return h.edit_nearest(set1, set2, min_distance, max_distance, other_repertoire)


def tcrdist_neighbors(set1: RepertoireSet, set2: RepertoireSet, opt: Options, params: TcrdistParams, cutoff: int,
                      distances: bool = True, tunables: Optional[dict] = None):
    """Convenience: (row_start, hits, distance) of set1 against set2 at a weighted CDR3 distance of at most `cutoff`
    (HipOverlap.tcrdist_neighbors) on a context of its own; `opt.differences` and `opt.indels` play no part.
    `tunables`: {name: value}."""
    with _context(opt, tunables) as h:
        return h.tcrdist_neighbors(set1, set2, params, cutoff, distances)


def tcrdist_matrix(set1: RepertoireSet, set2: RepertoireSet, opt: Options, params: TcrdistParams, cutoff: int,
                   tunables: Optional[dict] = None):
    """Convenience: the matrix of set1 against set2 over the pairs at a weighted CDR3 distance of at most `cutoff`
    (HipOverlap.tcrdist_matrix) on a context of its own; `opt.differences` and `opt.indels` play no part.
    `tunables`: {name: value}."""
    with _context(opt, tunables) as h:
        return h.tcrdist_matrix(set1, set2, params, cutoff)


def existence_csr(set1: RepertoireSet, set2: RepertoireSet, opt: Options, tunables: Optional[dict] = None):
    """Convenience: (row_start, repertoire, value) of set1 against set2 under `opt` (HipOverlap.existence_csr) on
    a context of its own.  `tunables` are set on the context first (the result never depends on them)."""
    with _context(opt, tunables, set1, set2) as h:
        return h.existence_csr()
