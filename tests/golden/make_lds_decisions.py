#!/usr/bin/env python3
"""Record tests/golden/lds_decisions.json: what a GIVEN library decides for the cases of
tests/test_lds_decisions_gpu.py (imported from there, so the two cannot drift).

The library is the one the change under test is compared WITH -- the parent commit's build, never the
library under test --, so it has to be named explicitly.  On a machine with the GPU, from the repository root:
    COMPAIRR_HIP_LIB=/path/to/parent/libcompairr_hip.so python tests/golden/make_lds_decisions.py PARENT_COMMIT [OUT]
A case whose matrix differs from the oracle's is not recorded: the recorder stops there.
"""

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _oracle  # noqa: E402
import test_lds_decisions_gpu as T  # noqa: E402


def main():
    if not os.environ.get("COMPAIRR_HIP_LIB") or len(sys.argv) < 2:
        sys.exit("usage: COMPAIRR_HIP_LIB=<the parent commit's library> make_lds_decisions.py <that commit> [out.json]")
    out = sys.argv[2] if len(sys.argv) > 2 else T.FIXTURE
    observed = {}
    for name in T.CASES:
        print(name, "...", flush=True)
        observed[name], matrix = T.observe(name)
        print(name, json.dumps(observed[name]), flush=True)
        if matrix is not None:
            a, b = T.sets_of(name)
            opt = T.options_of(name)
            want = _oracle.integer_cells(_oracle.overlap(a, b, opt, threads=2)[0], opt)
            if not np.array_equal(matrix, want):
                sys.exit("%s: the library's matrix is not the oracle's" % name)
    record = {"library_commit": sys.argv[1], "cases": {name: list(T.CASES[name]) for name in T.CASES},
              "observed": observed}
    with open(out, "w") as fh:
        json.dump(record, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
