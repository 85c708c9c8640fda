#!/usr/bin/env python3
"""usage: tools/step_timeline.py <rocprofv3 kernel trace .csv> [steps to skip, default 8]

The timeline of bench.py's query-set step (cmpr_set_queries_device on the library's stream, then one launch on
the caller's) from a `rocprofv3 --kernel-trace` of the plain run: per steady step, where the kernels of the
layout of set k+1 lie relative to those of the launch on set k.  Medians over the steady steps, microseconds.
A negative "keys start - previous launch end" is the overlap; "first writer - previous launch end" must never be
negative (the layout's second half overwrites what a launch reads)."""

import csv
import re
import statistics
import sys


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    m = re.match(r"[\w:]+(<\d+u?>)?", name)
    return (m.group(0) if m else name).split("::")[-1]


def main():
    path = sys.argv[1]
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    ks = []
    for r in csv.DictReader(open(path)):
        ks.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r["Stream_Id"]))
    ks.sort()
    keys = [k for k in ks if k[2] == "keys_kernel"]
    if len(keys) < skip + 3:
        sys.exit("fewer than %d keys_kernel dispatches in the trace" % (skip + 3))
    lay_stream = keys[-1][3]
    probes = [k for k in ks if "probe" in k[2]]
    run_stream = probes[-1][3]
    lay = [k for k in ks if k[3] == lay_stream]
    run = [k for k in ks if k[3] == run_stream and k[0] >= keys[0][0]]

    # layout j: from the memset in front of keys_kernel j up to the same point of layout j + 1
    heads = []
    for k in keys:
        i = lay.index(k)
        if i and lay[i - 1][2].startswith("__amd_rocclr_fill"):      # (arena A's counters: always there)
            i -= 1
        heads.append(i)
    layouts = [lay[heads[j]:heads[j + 1]] for j in range(len(keys) - 1)]
    ends = [max(k[1] for k in L) for L in layouts]
    # launch j: enqueued when layout j is through and before layout j + 1 is begun
    launches = [[k for k in run if ends[j] <= k[0] < (ends[j + 1] if j + 1 < len(ends) else 1 << 62)]
                for j in range(len(layouts))]

    rows = {}

    def put(name, value):
        rows.setdefault(name, []).append(value / 1e3)

    early_writers = 0
    for j in range(max(skip, 1), len(layouts) - 1):
        L, R, Rprev = layouts[j], launches[j], launches[j - 1]
        if not R or not Rprev:
            continue
        prev_end = max(k[1] for k in Rprev)
        named = {k[2]: k for k in L}
        kk, sc = named["keys_kernel"], named["scatter_kernel"]
        sizes = named["sizes_kernel"]
        after_sizes = [k for k in L if k[0] >= sizes[1]]
        copy = after_sizes[0]                              # the SizesBlock on its way to the host
        writer = after_sizes[1]                            # the first kernel behind the round trip
        put("step period (keys start to keys start)", layouts[j + 1][0][0] - L[0][0])
        put("keys start - previous launch end", kk[0] - prev_end)
        put("first writer - previous launch end", writer[0] - prev_end)
        early_writers += writer[0] < prev_end
        put("keys_kernel (dispatch to end)", kk[1] - kk[0])
        put("sizes chain: keys end to SizesBlock copied", copy[1] - kk[1])
        put("  of which inside kernels", sum(k[1] - k[0] for k in L if kk[1] <= k[0] <= copy[0]))
        put("round trip: copy end to first writer", writer[0] - copy[1])
        put("writers up to scatter start", sc[0] - writer[0])
        put("scatter_kernel", sc[1] - sc[0])
        put("order chain: scatter end to layout end", ends[j] - sc[1])
        put("  of which inside kernels", sum(k[1] - k[0] for k in L if k[0] >= sc[1]))
        put("layout end to first launch kernel", R[0][0] - ends[j])
        big = max((k for k in R if "probe" in k[2]), key=lambda k: k[1] - k[0])
        put("launch start to probe start", big[0] - R[0][0])
        put("probe kernel", big[1] - big[0])
        res = [k for k in R if k[2] == "resolve_kernel"]
        red = [k for k in R if k[2] == "reduce_partials_kernel"]
        if res:
            put("probe end to resolve start", res[0][0] - big[1])
            put("resolve_kernel", res[0][1] - res[0][0])
        if red:
            put("reduce_partials_kernel", red[0][1] - red[0][0])
        put("launch: first kernel to last end", max(k[1] for k in R) - R[0][0])

    n = len(next(iter(rows.values())))
    print("%s: %d steady steps (the first %d skipped); median [min .. max], us" % (path, n, skip))
    for name, v in rows.items():
        print("%-46s %9.1f  [%9.1f .. %9.1f]" % (name, statistics.median(v), min(v), max(v)))
    print("steps whose first writer started before the previous launch ended: %d" % early_writers)


if __name__ == "__main__":
    main()
