#!/usr/bin/env python3
"""Record tests/golden/dedup/: what the reference's --deduplicate prints for inputs that already lie in
tests/golden/inputs/.

Runs oracle/_ref/compairr -z (the unmodified reference program compiled by oracle/Makefile) once per case and
keeps its standard output as dedup/<name>.tsv, plus one manifest.json row per case: file, args, and the
"Sequences:" and "Duplicates merged:" figures of its log.  Only recorded results are written, and only under
tests/golden/dedup/; the inputs and the other golden directories are left as they are.

    make -C oracle ref && python tests/golden/make_dedup.py
"""

import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "compairr")
INPUTS = os.path.join(HERE, "inputs")
OUT = os.path.join(HERE, "dedup")

# (name, input file, arguments)
CASES = [
    ("dups", "dups.tsv", ""),
    ("dups_f", "dups.tsv", "-f"),
    ("dups_g", "dups.tsv", "-g"),
    ("dups_n", "dups.tsv", "-n"),
    ("lower", "lower.tsv", ""),
    ("lower_n", "lower.tsv", "-n"),
    ("lower_n_g", "lower.tsv", "-n -g"),
    ("setb", "setb.tsv", ""),
    ("tiny_aa_a", "tiny_aa_a.tsv", ""),
    ("tiny_aa_a_g_f", "tiny_aa_a.tsv", "-g -f"),
    ("tiny_nt_a_n", "tiny_nt_a.tsv", "-n"),
    ("tiny_nt_b_n_g", "tiny_nt_b.tsv", "-n -g"),
    ("rand_aa_a", "rand_aa_a.tsv", ""),
    ("clus_aa", "clus_aa.tsv", ""),
    ("clus_nt_n", "clus_nt.tsv", "-n"),
    ("clus_nt_n_g", "clus_nt.tsv", "-n -g"),
    ("norep", "norep.tsv", ""),
    ("nogenes_g", "nogenes.tsv", "-g"),
    ("nocount_f", "nocount.tsv", "-f"),
    ("cdr3", "cdr3.tsv", "--cdr3"),
]


def figure(log, label):
    m = re.search(r"^%s:\s+(\d+)\s*$" % re.escape(label), log, flags=re.M)
    if not m:
        sys.exit("no '%s:' line in the reference's log" % label)
    return int(m.group(1))


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    os.makedirs(OUT, exist_ok=True)
    manifest = []
    for name, file, args in CASES:
        with tempfile.TemporaryDirectory() as tmp:
            logf = os.path.join(tmp, "log")
            p = subprocess.run([REF, "-z"] + args.split() + [file, "-l", logf], cwd=INPUTS,
                               stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
            if p.returncode != 0:
                sys.exit("%s: the reference exited with %d" % (name, p.returncode))
            log = open(logf, errors="replace").read()
        with open(os.path.join(OUT, name + ".tsv"), "wb") as fh:
            fh.write(p.stdout)
        manifest.append({"name": name, "file": file, "args": args,
                         "sequences": figure(log, "Sequences"),
                         "merged": figure(log, "Duplicates merged")})
        print("%-16s %-16s %-8s sequences %6d  merged %4d" % (name, file, args, manifest[-1]["sequences"],
                                                           manifest[-1]["merged"]))
    with open(os.path.join(OUT, "manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
