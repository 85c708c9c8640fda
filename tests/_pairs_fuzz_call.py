"""The all-against-all sweep on the GPU: a case of tests/_pairs_fuzz.py dispatched to its C entry point -- the host
one or its _device twin -- and the result compared with the expectation for exact equality.  Shared by the slice
(tests/test_pairs_fuzz_gpu.py) and the sweep by hand (tests/fuzz_pairs_gpu.py).

Every output array, host or device, carries PAD poison words behind its end, which must come back untouched; with a
capacity one short nothing may be written to the hits or the distances."""

import ctypes as C
import sys

import numpy as np

import _cluster_table
import _neighbors
import _pairs_fuzz as pf
from compairr_amd import HipError, HipOverlap, TcrdistParams
from compairr_amd.hip import NEAREST_OTHER_REPERTOIRE, UNCAPPED, _SetView, _view

PAD = 64
POISON = {2: 0x25A5, 4: 0x25A5A5A5, 8: 0x25A5A5A525A5A5A5}


class Mismatch(AssertionError):
    pass


class Out:
    """an output array of n elements and PAD poison words, in host memory or on the device"""

    def __init__(self, device, dtype, n):
        self.dtype, self.n = np.dtype(dtype), n
        self.poison = self.dtype.type(POISON[self.dtype.itemsize])
        host = np.full(n + PAD, self.poison, dtype=self.dtype)
        if device:
            import torch
            self.keep = torch.from_numpy(host.view(np.uint8)).to("cuda")
            self.ptr = self.keep.data_ptr()
        else:
            self.keep = host
            self.ptr = host.ctypes.data
        self.device = device

    def read(self):
        a = self.keep.cpu().numpy().view(self.dtype) if self.device else self.keep
        return a.copy()

    def written(self, name, m=None):
        """the first m elements (default: all n); everything behind them must still be poison"""
        m = self.n if m is None else m
        a = self.read()
        if not (a[m:] == self.poison).all():
            k = m + int(np.nonzero(a[m:] != self.poison)[0][0])
            raise Mismatch("%s: element %d, behind the %d the call may write, was written: %#x" % (name, k, m, int(a[k])))
        return a[:m]

    def untouched(self, name):
        self.written(name, 0)


def _device_view(s):
    """HipOverlap.device_view with PAD poison bytes behind every array: an array without an element -- the residues
    of a set of empty sequences -- is device memory all the same (a NULL `residues` in a device view is refused)"""
    import torch
    tail = np.full(PAD, 0xA5, dtype=np.uint8)
    keep = [torch.from_numpy(np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), tail])).to("cuda")
            for a in (s.residues, s.offsets, s.v_gene, s.j_gene, s.repertoire, s.count)]
    v = _SetView()
    v.n = s.n
    (v.residues, v.offsets, v.v_gene, v.j_gene, v.repertoire, v.count) = [t.data_ptr() for t in keep]
    v.n_repertoires = s.n_repertoires
    torch.cuda.synchronize()
    return v, keep


def _views(c):
    """(view 1, view 2, what keeps them alive): host or device views; the same object twice in one-file mode"""
    if c.entry == "device":
        v1, keep1 = _device_view(c.set1)
        if c.one_set:
            return v1, v1, [keep1]
        v2, keep2 = _device_view(c.set2)
        return v1, v2, [keep1, keep2]
    v1 = _view(c.set1)
    return v1, (v1 if c.one_set else _view(c.set2)), []


def _first_difference(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "%s: shape %s, want %s" % (name, got.shape, want.shape)
    where = np.argwhere(got != want)
    k = tuple(int(x) for x in where[0])
    return "%s%s: got %d, want %d (%d elements differ)" % (name, list(k), int(got[k]), int(want[k]), len(where))


def _same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape or got.tobytes() != want.tobytes():
        if got.dtype != want.dtype:
            raise Mismatch("%s: dtype %s, want %s" % (name, got.dtype, want.dtype))
        raise Mismatch(_first_difference(name, got, want))


def _csr_difference(c, got, want):
    """the first differing edge in words: row, hit, distance wanted and got"""
    def edges(csr):
        rows = np.asarray(csr[0]).astype(np.int64)
        q = np.repeat(np.arange(len(rows) - 1), np.diff(rows))
        return {(int(a), int(b)): int(d) for a, b, d in zip(q, csr[1], csr[2])}
    try:
        g, w = edges(got), edges(want)
    except Exception as e:
        return "malformed CSR: %r" % e
    for q, h in sorted(set(g) | set(w)):
        if g.get((q, h)) != w.get((q, h)):
            return ("row %d (%d residues) hit %d (%d residues): distance got %s, want %s; %d edges got, %d wanted"
                    % (q, int(c.set1.lengths[q]), h, int(c.set2.lengths[h]), g.get((q, h)), w.get((q, h)), len(g), len(w)))
    return "the same edges in another order"


def call(c, h, want):
    """the case's call on the context h: the result as a list of (name, array), after every check of the protocol"""
    lib, ctx, dev = h._lib, h._ctx, c.entry == "device"
    suffix = "_device" if dev else ""
    v1, v2, keep = _views(c)
    n1 = c.set1.n
    n_out = C.c_uint64(12345)
    head = [ctx, C.byref(v1)] + ([] if c.kind in ("cluster", "cluster_table") else [C.byref(v2)])
    if c.metric == "tcrdist":
        holder = TcrdistParams(c.W, c.gap_penalty, c.ntrim, c.ctrim, c.gap_mode, c.V)     # (keeps the two tables alive)
        params = holder.struct(h.opt)
        head += [C.byref(params), c.cutoff]
    elif c.kind == "nearest":
        head += [c.floor] + ([UNCAPPED if c.cap is None else c.cap] if c.metric == "edit" else [])
        head += [NEAREST_OTHER_REPERTOIRE if c.other_repertoire else 0]
    else:
        head += [c.differences]
    fn = getattr(lib, "cmpr_%s_%s%s" % (c.metric, c.kind, suffix))

    def check(rc):
        if rc:
            h._check(rc)                                               # (raises HipError with the library's text)

    try:
        if c.kind == "neighbors":
            edges = len(want.pairs[1])
            capacity = {"exact": edges, "short": max(edges - 1, 0), "generous": edges + 10}[c.capacity]
            rows, hits, dist = Out(dev, np.uint64, n1 + 1), Out(dev, np.uint32, capacity), Out(dev, np.uint16, capacity)
            check(fn(*head, capacity, C.c_void_p(rows.ptr), C.c_void_p(hits.ptr) if capacity else None,
                     C.c_void_p(dist.ptr) if capacity else None, C.byref(n_out)))
            got_rows = rows.written("row_start")
            if n_out.value != edges:
                raise Mismatch("n_edges: got %d, want %d" % (n_out.value, edges))
            _same("row_start", got_rows, want.pairs[0])
            if capacity < edges:                                       # one short: nothing may be written
                hits.untouched("hits")
                dist.untouched("distance")
                return [("row_start", got_rows)]
            got = (got_rows, hits.written("hits", edges), dist.written("distance", edges))
            if any(a.tobytes() != b.tobytes() for a, b in zip(got, want.pairs)):
                raise Mismatch(_csr_difference(c, got, want.pairs))
            _neighbors.assert_is_csr(got[0], got[1], n1)
            return list(zip(("row_start", "hits", "distance"), got))
        if c.kind == "matrix":
            cells = Out(dev, np.uint64, want.matrix.size)
            check(fn(*head, C.c_void_p(cells.ptr)))
            got = cells.written("matrix").reshape(want.matrix.shape)
            _same("matrix cell", got, want.matrix)
            return [("matrix", got)]
        if c.kind == "nearest":
            outs = [Out(dev, t, n1) for t in (np.uint32, np.uint16, np.uint32)]
            check(fn(*head, *[C.c_void_p(o.ptr) for o in outs], C.byref(n_out)))
            got = [o.written(name) for o, name in zip(outs, ("nearest", "distance", "ties"))]
            for i in range(n1):
                triple = tuple(int(a[i]) for a in got)
                wanted = tuple(int(a[i]) for a in want.nearest)
                if triple != wanted:
                    raise Mismatch("sequence %d (%d residues): (number, distance, ties) got %s, want %s"
                                   % (i, int(c.set1.lengths[i]), triple, wanted))
            if n_out.value != want.n_found:
                raise Mismatch("n_found: got %d, want %d" % (n_out.value, want.n_found))
            for g, w, name in zip(got, want.nearest, ("nearest", "distance", "ties")):
                _same(name, g, w)
            return list(zip(("nearest", "distance", "ties"), got))
        # the clusters: the partition from cmpr_*_cluster, and for cluster_table the table as well
        label, size = Out(dev, np.uint32, n1), Out(dev, np.uint32, n1)
        labels_fn = getattr(lib, "cmpr_%s_cluster%s" % (c.metric, suffix))
        check(labels_fn(*head, C.c_void_p(label.ptr), C.c_void_p(size.ptr), C.byref(n_out)))
        got = (label.written("label"), size.written("size"), n_out.value)
        differ = np.nonzero(got[0] != want.label)[0]
        if len(differ):
            i = int(differ[0])
            raise Mismatch("sequence %d (%d residues): label got %d, want %d (%d labels differ)"
                           % (i, int(c.set1.lengths[i]), int(got[0][i]), int(want.label[i]), len(differ)))
        _cluster_table.assert_partition(got, want.label)
        result = [("label", got[0]), ("size", got[1])]
        if c.kind == "cluster_table":
            k = len(want.table[3])
            outs = [Out(dev, np.uint32, n1), Out(dev, np.uint64, n1 + 1), Out(dev, np.uint32, n1), Out(dev, np.uint64, n1)]
            check(fn(*head, *[C.c_void_p(o.ptr) for o in outs], C.byref(n_out)))
            if n_out.value != k:
                raise Mismatch("n_clusters: got %d, want %d" % (n_out.value, k))
            table = [o.written(name, m) for o, name, m in zip(outs, _cluster_table.TABLE_NAMES, (n1, k + 1, n1, k))]
            for name, g, w in zip(_cluster_table.TABLE_NAMES, table, want.table):
                _same(name, g, w)
            _cluster_table.assert_table(table, want.table)
            result += list(zip(_cluster_table.TABLE_NAMES, table))
        return result
    finally:
        del keep


def run_with(c, want, tunables):
    with HipOverlap(pf.options_of(c, device=0)) as h:
        for name, value in tunables.items():
            h.set_tunable(name, value)
        return call(c, h, want)


def run_case(c, want=None):
    """the case's call checked against its expectation; every fourth case once more under its second setting of the
    tunables, every fourth once more unchanged: the same bytes.  Raises Mismatch with the case in full."""
    try:
        want = pf.expect(c) if want is None else want
        first = run_with(c, want, c.tunables)
        again = None
        if c.index % 4 == 0:
            again, what = run_with(c, want, c.tunables2), "under the tunables %r" % (c.tunables2,)
        elif c.index % 4 == 2:
            again, what = run_with(c, want, c.tunables), "in a second, unchanged call"
        if again is not None:
            for (name, a), (_, b) in zip(first, again):
                if a.tobytes() != b.tobytes():
                    raise Mismatch("%s differs %s: %s" % (name, what, _first_difference(name, b, a)))
    except AssertionError as e:
        raise Mismatch("%s\n%s" % (e, pf.describe(c))) from None
    except HipError:                                                   # (no drawn argument is refused: a finding)
        print("HipError in the case\n" + pf.describe(c), file=sys.stderr)
        raise
    return want
