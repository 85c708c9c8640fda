"""The two ends of a device view's offsets -- all the host sees of a set that lives on the device -- are checked by
every entry point that takes such a view, before anything of the view is read or copied on the device: offsets[0]
must be 0, and offsets[n] cannot exceed 65535 residues per sequence.  After the refusal the same context takes the
sound view and gives what the host variant gives on a fresh context.  Every comparison is for exact equality."""

import functools

import numpy as np
import pytest

from compairr_amd import HipError, HipOverlap, Options, RepertoireSet
from compairr_amd.sets import AA

pytestmark = pytest.mark.gpu

CMPR_EINVAL = 1
D = 1                                   # differences: of the context, and of the cmpr_hamming_* calls
SEQUENCES = ("CASSL", "CASSL", "CASSF", "CAWSL", "CASSLG", "CASSLG", "AAAAAA", "CASRF")
REPERTOIRE = (0, 0, 1, 0, 1, 1, 0, 1)


def the_set() -> RepertoireSet:
    n = len(SEQUENCES)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(q) for q in SEQUENCES], out=offsets[1:])
    residues = np.array([AA.index(ch) for q in SEQUENCES for ch in q], dtype=np.uint8)
    return RepertoireSet(residues, offsets, np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32),
                         np.array(REPERTOIRE, dtype=np.uint32), np.arange(1, n + 1, dtype=np.uint64), ["r1", "r2"],
                         ["V0"], ["J0"], AA)


def first_offset_one(s):
    s.offsets[0] = 1


def last_offset_beyond_any_set(s):
    s.offsets[s.n] = 0xffff * s.n + 1


BAD = {"offsets[0]=1": (first_offset_one, "offsets[0] must be 0"),
       "offsets[n]=0xffff*n+1": (last_offset_beyond_any_set, "offsets not monotone")}


def dev(count, dtype):
    import torch
    return torch.zeros(max(count, 1), dtype=dtype, device="cuda")


def host(t, count, dtype):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype)[:count].copy()


# ---- per entry point: the device call on a view, and the host call that says what it has to give ----

def reference_device(h, v, s):
    h.set_reference_device(v, s.longest)
    h.set_queries(s)
    return (h.overlap_matrix(),)


def reference_host(h, s):
    h.set_reference(s, s.longest)
    h.set_queries(s)
    return (h.overlap_matrix(),)


def deduplicate_device(h, v, s):
    import torch
    first, count = dev(s.n, torch.int32), dev(s.n, torch.int64)
    unique, merged = h.deduplicate_device(v, s.n, first.data_ptr(), count.data_ptr())
    return host(first, unique, np.uint32), host(count, unique, np.uint64), merged


def labels_device(method, extra, h, v, s):
    import torch
    label, size = dev(s.n, torch.int32), dev(s.n, torch.int32)
    clusters = getattr(h, method)(v, *extra, label.data_ptr(), size.data_ptr())
    return host(label, s.n, np.uint32), host(size, s.n, np.uint32), clusters


def table_device(method, extra, h, v, s):
    import torch
    of, start = dev(s.n, torch.int32), dev(s.n + 1, torch.int64)
    member, count = dev(s.n, torch.int32), dev(s.n, torch.int64)
    k = getattr(h, method)(v, *extra, of.data_ptr(), start.data_ptr(), member.data_ptr(), count.data_ptr())
    return (host(of, s.n, np.uint32), host(start, k + 1, np.uint64), host(member, s.n, np.uint32),
            host(count, k, np.uint64))


def hamming_matrix_device(h, v, s):
    import torch
    cells = s.n_repertoires * s.n_repertoires
    m = dev(cells, torch.int64)
    h.hamming_matrix_device(v, v, D, m.data_ptr())
    return (host(m, cells, np.uint64).reshape(s.n_repertoires, s.n_repertoires),)


def hamming_neighbors_device(h, v, s):
    import torch
    capacity = s.n * s.n                                  # (no set has more pairs)
    rows, hits, dist = dev(s.n + 1, torch.int64), dev(capacity, torch.int32), dev(capacity, torch.int16)
    edges = h.hamming_neighbors_device(v, v, D, capacity, rows.data_ptr(), hits.data_ptr(), dist.data_ptr())
    return host(rows, s.n + 1, np.uint64), host(hits, edges, np.uint32), host(dist, edges, np.uint16)


CALLS = {
    "set_reference_device": (reference_device, reference_host),
    "deduplicate_device": (deduplicate_device, lambda h, s: h.deduplicate(s)),
    "cluster_device": (functools.partial(labels_device, "cluster_device", ()), lambda h, s: h.cluster(s)),
    "cluster_table_device": (functools.partial(table_device, "cluster_table_device", ()),
                             lambda h, s: h.cluster_table(s)),
    "hamming_matrix_device": (hamming_matrix_device, lambda h, s: (h.hamming_matrix(s, s, D),)),
    "hamming_neighbors_device": (hamming_neighbors_device, lambda h, s: h.hamming_neighbors(s, s, D)),
    "hamming_cluster_device": (functools.partial(labels_device, "hamming_cluster_device", (D,)),
                               lambda h, s: h.hamming_cluster(s, D)),
    "hamming_cluster_table_device": (functools.partial(table_device, "hamming_cluster_table_device", (D,)),
                                     lambda h, s: h.hamming_cluster_table(s, D)),
}


@functools.lru_cache(maxsize=None)
def host_result(name):
    """what the host variant gives on a fresh context"""
    with HipOverlap(Options(differences=D, device=0)) as h:
        return CALLS[name][1](h, the_set())


@pytest.mark.parametrize("bad", list(BAD), ids=list(BAD))
@pytest.mark.parametrize("name", list(CALLS))
def test_bad_ends_are_refused_and_the_context_goes_on(name, bad):
    alter, text = BAD[bad]
    device_call = CALLS[name][0]
    s, broken = the_set(), the_set()
    alter(broken)
    with HipOverlap(Options(differences=D, device=0)) as h:
        v_bad, keep_bad = h.device_view(broken)
        with pytest.raises(HipError) as e:
            device_call(h, v_bad, s)
        assert e.value.code == CMPR_EINVAL
        assert text in str(e.value)
        v, keep = h.device_view(s)
        got, want = device_call(h, v, s), host_result(name)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            if isinstance(w, np.ndarray):
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
            else:
                assert g == w
