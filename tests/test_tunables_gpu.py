"""cmpr_set_tunable / cmpr_get_tunable, pinned name by name.

Every name the library knows is probed at the edges of its range and at the holes inside it, in
three states of a context (new; after cmpr_set_reference; after cmpr_set_queries): return code,
exact cmpr_last_error text, and the value read back after an accepted set.  The expectations are
in tests/golden/tunables_abi5.json, recorded by tests/golden/make_tunables.py from the library of
the commit named in that file -- never from the library under test -- with the probe list below.
"""

import ctypes as C
import functools
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from compairr_amd import hip as hipmod  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(HERE, "golden", "tunables_abi5.json")
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1

# settable name -> (least accepted value, greatest accepted value); None: no bound on that side.
# (amino acids: class_residues ends at 4)
SETTABLE = {
    "blocks_per_cu": (1, 16), "variant": (-1, 2), "class_residues": (-1, 4), "class_anchor": (-1, 65535),
    "heavy_threshold": (-1, None), "slice_words_log2": (-1, 13), "chunk_tiles": (0, 512),
    "debug": (None, None), "host_threads": (1, 256), "table_log2_delta": (0, 3),
    "part_buckets_log2": (2, 30), "deferred_resolve": (0, 1), "d2_pairs": (-1, 1), "d2_buffers": (1, 2),
    "chunk_deal": (0, 1), "narrow_upload": (-1, 1), "item_wg": (0, 1), "layout_recompute": (0, 1),
    "layout_timing": (0, 1), "layout_zob_lds": (0, 1), "record_tiles": (0, 2),
    "assume_never_overflows": (None, None), "resolve_blocks_per_cu": (1, 8), "pos_segments": (1, 256),
    "pos_grow": (-1, 1), "pos_capacity": (0, None), "work_shard_count": (1, 65535),
    "work_shard_index": (0, 65535), "small_slice_tiles": (0, 64), "sub2_items": (-1, 1),
    "class_rows_unstaged": (0, 1), "waves_per_block": (4, 16), "bloom_bits_log2_delta": (-4, 4),
    "slice_pages": (-1, 3), "page_budget": (0, 1 << 24), "bucket_bitmap": (-1, 1), "fill_slices": (0, 1),
    "direct_slices_log2": (-1, 12), "row_filter_x16": (8, 128),
}
# values inside (or beside) a range that follow a rule of their own
HOLES = {"slice_words_log2": (0,), "waves_per_block": (5, 8), "pos_segments": (3, 4), "work_shard_count": (0,),
         "record_tiles": (2, 3), "debug": (1,), "assume_never_overflows": (0, 1)}
UNKNOWN = ("no_such_tunable", "pt0")         # (pt0..pt7 exist in a -DCMPR_PHASE_TIMING build only)
TIMINGS = ("layout_upload_us", "layout_tail_us", "layout_total_us", "layout_keys_us", "layout_sizes_us",
           "layout_scatter_us", "layout_tiles_us", "layout_order_us")
READ_ONLY = TIMINGS + ("slice_bytes", "passes", "never_overflows", "heavy_buckets", "slices", "tiles", "chunks",
                       "small_tiles", "reference_parts", "page_slices", "query_slots", "items")
STATES = ("fresh", "reference", "queries")
ENVIRONMENT = (("COMPAIRR_HIP_VARIANT", "variant", "1"), ("COMPAIRR_HIP_VARIANT", "variant", "7"),
               ("COMPAIRR_HIP_VARIANT", "variant", "abc"),
               ("COMPAIRR_HIP_SLICE_WORDS_LOG2", "slice_words_log2", "0"),
               ("COMPAIRR_HIP_SLICE_WORDS_LOG2", "slice_words_log2", "5"),
               ("COMPAIRR_HIP_CLASS_RESIDUES", "class_residues", "99"))


def probe_values(name):
    """one below the least accepted value, that value, the greatest, one above it, the holes"""
    lo, hi = SETTABLE[name]
    values = [I64_MIN] if lo is None else [lo - 1, lo]
    values += [I64_MAX] if hi is None else [hi, hi + 1]
    return values + [v for v in HOLES.get(name, ()) if v not in values]


@functools.lru_cache(maxsize=None)
def sets():
    """(queries, reference): 100 sequences each, amino acids"""
    from compairr_amd import synth
    return synth.make_set(100, 1), synth.make_set(100, 2)


class Context:
    """a context of the C ABI whose calls report (code, text) where HipOverlap raises"""

    def __init__(self, state="fresh"):
        from compairr_amd import HipOverlap, Options, synth
        a, b = sets()
        self.h = HipOverlap(Options(differences=1, n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0))
        if state != "fresh":
            self.h.set_reference(b, a.longest)
        if state == "queries":
            self.h.set_queries(a)
        self.lib, self.ctx = self.h._lib, self.h._ctx

    def error(self):
        return self.lib.cmpr_last_error(self.ctx).decode()

    def set(self, name, value):
        rc = self.lib.cmpr_set_tunable(self.ctx, None if name is None else name.encode(), value)
        return [rc, self.error()]

    def get(self, name):
        """[code, value, text]; of the timings only that they are not negative"""
        v = C.c_int64(-12345)
        rc = self.lib.cmpr_get_tunable(self.ctx, name.encode(), C.byref(v))
        value = v.value
        if rc == 0 and name in TIMINGS:
            value = "not negative" if value >= 0 else value
        return [rc, value, self.error()]

    def close(self):
        self.h.close()


def observe_state(state):
    """{"set": {name: [[value, code, text, what get then returns or None], ...]}, "get": {name: [code, value, text]}}
    -- a context of its own per name, so that no probe sees what another stored"""
    set_rows = {}
    for name in SETTABLE:
        c = Context(state)
        rows = []
        for value in probe_values(name):
            rc, text = c.set(name, value)
            rows.append([value, rc, text, c.get(name) if rc == 0 else None])
        set_rows[name] = rows
        c.close()
    c = Context(state)
    set_rows["<unknown>"] = [[1] + c.set(UNKNOWN[0], 1) + [None]]
    set_rows["<null name>"] = [[1] + c.set(None, 1) + [None]]
    set_rows["<null context>"] = [[1, c.lib.cmpr_set_tunable(None, b"variant", 1), c.lib.cmpr_last_error(None).decode(), None]]
    c.close()
    c = Context(state)
    gets = {name: c.get(name) for name in tuple(SETTABLE) + READ_ONLY + UNKNOWN}
    host_threads = gets["host_threads"]        # (its default is the machine's: cmpr_create)
    if host_threads[1] == min(16, os.cpu_count() or 1):
        host_threads[1] = "of this machine"
    c.close()
    return {"set": set_rows, "get": gets}


def environment_child(name):
    """(in a process of its own) a new context: what the variable left in it"""
    lib = C.CDLL(hipmod.library_path())
    lib.cmpr_create.argtypes = [C.POINTER(hipmod._Options), C.POINTER(C.c_void_p)]
    lib.cmpr_last_error.argtypes = [C.c_void_p]
    lib.cmpr_last_error.restype = C.c_char_p
    lib.cmpr_get_tunable.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
    lib.cmpr_destroy.argtypes = [C.c_void_p]
    o = hipmod._Options(differences=1, alphabet_size=20, n_v_genes=1, n_j_genes=1, device=0)
    ctx, v = C.c_void_p(), C.c_int64(-12345)
    out = {"create": lib.cmpr_create(C.byref(o), C.byref(ctx))}
    out["get"] = lib.cmpr_get_tunable(ctx, name.encode(), C.byref(v))
    out["value"] = v.value
    out["error"] = lib.cmpr_last_error(ctx).decode()
    out["create_error"] = lib.cmpr_last_error(None).decode()
    lib.cmpr_destroy(ctx)
    print(json.dumps(out))


def observe_environment():
    """one fresh process per setting (they run side by side)"""
    children = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "environment-child", name],
                                 env=dict(os.environ, **{variable: text}), stdout=subprocess.PIPE)
                for variable, name, text in ENVIRONMENT]
    out = {}
    for (variable, name, text), child in zip(ENVIRONMENT, children):
        stdout, _ = child.communicate(timeout=120)
        assert child.returncode == 0, (variable, text, child.returncode)
        out["%s=%s" % (variable, text)] = json.loads(stdout.decode().strip().splitlines()[-1])
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_probe_list_is_the_recorded_one(recorded):
    assert recorded["probes"] == {name: probe_values(name) for name in SETTABLE}
    assert sorted(recorded["states"]) == sorted(STATES)


@pytest.mark.parametrize("state", STATES)
def test_tunables_behave_as_recorded(recorded, state):
    want, got = recorded["states"][state], json.loads(json.dumps(observe_state(state)))
    for name in want["set"]:
        assert got["set"].get(name) == want["set"][name], "set %s, %s" % (name, state)
    for name in want["get"]:
        assert got["get"].get(name) == want["get"][name], "get %s, %s" % (name, state)
    assert got == want
    for name in TIMINGS:
        assert got["get"][name][:2] == [0, "not negative"]


def test_environment_overrides_behave_as_recorded(recorded):
    assert observe_environment() == recorded["environment"]


if __name__ == "__main__" and sys.argv[1:2] == ["environment-child"]:
    environment_child(sys.argv[2])
