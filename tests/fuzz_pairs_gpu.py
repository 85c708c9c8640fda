#!/usr/bin/env python3
"""Randomised parity sweep of the all-against-all calls (cmpr_hamming_*, cmpr_edit_*, cmpr_tcrdist_*) on the GPU box:
the cases of tests/_pairs_fuzz.py through the C ABI against the numpy yardsticks.  Not collected by pytest: run it by
hand, `python tests/fuzz_pairs_gpu.py --seconds 300 --seed S`, or replay one case with `--seed S --case K`.  It stops
at the first mismatch and prints the case; a HipError -- no drawn argument is refused -- or any other failure ends it
at once, with a non-zero status and no retry.  At the end it prints the coverage tags it saw.  A seeded slice of it
runs in the GPU suite (tests/test_pairs_fuzz_gpu.py)."""

import argparse
import collections
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _pairs_fuzz as pf  # noqa: E402
import _pairs_fuzz_call  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--case", type=int, default=None, help="replay this one case of the seed")
    args = ap.parse_args()
    t0 = time.time()
    seen, combos = collections.Counter(), collections.Counter()
    n = yardstick = 0
    index = args.case if args.case is not None else 0
    while args.case is not None or time.time() - t0 < args.seconds:
        c = pf.case(args.seed, index)
        t1 = time.time()
        want = pf.expect(c)
        yardstick += time.time() - t1
        try:
            _pairs_fuzz_call.run_case(c, want)
        except _pairs_fuzz_call.Mismatch as e:
            print("MISMATCH after %d cases\n%s" % (n, e))
            sys.exit(1)
        tags = pf.classify(c, want)
        seen.update(tags)
        combos[(c.metric, c.kind, "vacuous" in tags)] += 1
        n += 1
        index += 1
        if args.case is not None:
            print(pf.describe(c))
            break
    print("tags seen: " + ", ".join("%s %d" % kv for kv in sorted(seen.items())))
    print("combinations (live + vacuous): " + ", ".join(
        "%s %s %d+%d" % (m, k, combos[(m, k, False)], combos[(m, k, True)]) for m, k in pf.COMBOS))
    print("%d random cases of seed %d, all bit-exact (%.0f s, %.0f s of them the yardsticks)"
          % (n, args.seed, time.time() - t0, yardstick))


if __name__ == "__main__":
    main()
