#!/usr/bin/env python3
"""Record tests/golden/tunables_abi5.json: what cmpr_set_tunable / cmpr_get_tunable of a GIVEN library do
with the probe list of tests/test_tunables_gpu.py (imported from there, so the two cannot drift).

The library is the one the change under test is compared WITH -- the parent commit's build, never the
library under test --, so it has to be named explicitly.  On a machine with the GPU, from the repository root:
    COMPAIRR_HIP_LIB=/path/to/parent/libcompairr_hip.so python tests/golden/make_tunables.py PARENT_COMMIT [OUT]
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import test_tunables_gpu as T  # noqa: E402


def main():
    if not os.environ.get("COMPAIRR_HIP_LIB") or len(sys.argv) < 2:
        sys.exit("usage: COMPAIRR_HIP_LIB=<the parent commit's library> make_tunables.py <that commit> [out.json]")
    out = sys.argv[2] if len(sys.argv) > 2 else T.FIXTURE
    record = {"library_commit": sys.argv[1],
              "probes": {name: T.probe_values(name) for name in T.SETTABLE},
              "states": {state: T.observe_state(state) for state in T.STATES},
              "environment": T.observe_environment()}
    with open(out, "w") as fh:
        json.dump(record, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
