"""Generate tests/golden/dict.npz + dict.json FROM THE REFERENCE'S OWN DRIVERS: compress2_test.cpp and
compress3_test.cpp compiled as they are with the reference's binmat, pbm and GolombCoder sources (and
tests/cpp/gsl_shim for gsl_sf_lnchoose: GSL is not installed), run on small PBMs, their stdout parsed.

Run in the build container only (needs the reference tree):
    python tests/golden/make_golden_dict.py [reference/src]
Everything compiled lives in a temporary directory outside the repository and is deleted afterwards. The
two files hold data only: the input planes, per tile what the drivers print (bestk, bestd, |D|, both
lengths, the decision, the push), their summary lines, and the enumL table of that build (printed by a
probe compiled with the same header and flags, checked against tests/dropin_expect.enumL)."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dict_cases  # noqa: E402
import dropin_expect  # noqa: E402
from pnm_io import write_pbm  # noqa: E402

SHIM = os.path.join(ROOT, "tests", "cpp", "gsl_shim")
FLAGS = ["-O2", "-std=c++11", "-w"]
# ln C(n, r) / ln 2 through the build's own lnchoose (0 for r = 0, as the drivers' enumL), printed exactly
PROBE = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "gsl/gsl_sf_gamma.h"
int main(int argc, char** argv) {
  const unsigned n = (unsigned)atoi(argv[1]);
  for (unsigned r = 0; r <= n; ++r) printf("%a\n", r > 0 ? gsl_sf_lnchoose(n, r) * M_LOG2E : 0.0);
  return 0;
}
"""


TILE = re.compile(r"i=(\d+) j=(\d+) bestk=(\d+) bestd=(\d+) \|D\|=(\d+) ")
LENS = re.compile(r"nomatch len=(\d+) match_len=(\d+)")


def parse(text, nt):
    chunks = text.split("=" * 75)
    assert len(chunks) == nt + 1, (len(chunks), nt)
    rec = {k: np.zeros(nt, np.uint32) for k in ("i", "j", "bestk", "bestd", "dsize")}
    rec["nomatch_len"], rec["match_len"] = np.zeros(nt, np.uint64), np.zeros(nt, np.uint64)
    rec["has_lens"], rec["use_match"], rec["add"] = (np.zeros(nt, np.uint8) for _ in range(3))
    for t, c in enumerate(chunks[1:]):
        m = TILE.search(c)
        for k, v in zip(("i", "j", "bestk", "bestd", "dsize"), m.groups()):
            rec[k][t] = int(v)
        ln = LENS.search(c)
        if ln:
            rec["has_lens"][t] = 1
            rec["nomatch_len"][t], rec["match_len"][t] = int(ln.group(1)), int(ln.group(2))
        rec["use_match"][t] = "USE MATCH!" in c
        rec["add"][t] = "ADD TO DICT!" in c
    tail = chunks[-1]
    summary = {}
    for key, pat in (("comp", r"COMP CODELENGTH[^:]*: (\S+)"), ("raw", r"RAW CODELENGTH: (\S+)"),
                     ("ratio", r"RATIO: (\S+)"), ("matches", r"MATCHES: (\S+)"),
                     ("golomb_per_match", r"Avg\. Golomb/Match: (\S+)"),
                     ("golomb_per_nomatch", r"Avg\. Golomb/NoMatch: (\S+)")):
        m = re.search(pat, tail)
        if m:
            summary[key] = m.group(1)
    return rec, summary


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    arrays, meta = {}, []
    with tempfile.TemporaryDirectory(prefix="dict_golden_") as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
        inc = ["-I", ref, "-I", SHIM]
        for v in (2, 3):
            srcs = [os.path.join(ref, f) for f in (f"compress{v}_test.cpp", "binmat.cpp", "pbm.cpp", "GolombCoder.cpp")]
            subprocess.run(["g++", *FLAGS, *inc, *srcs, "-o", os.path.join(tmp, f"compress{v}")], check=True)
        with open(os.path.join(tmp, "probe.cpp"), "w") as f:
            f.write(PROBE)
        subprocess.run(["g++", *FLAGS, "-I", SHIM, os.path.join(tmp, "probe.cpp"), "-o", os.path.join(tmp, "probe")],
                       check=True)
        tables = {}
        for n, case in enumerate(dict_cases.CASES):
            plane, rows, cols = dict_cases.make_input(case)
            W, T = case["W"], case["T"]
            if W not in tables:
                out = subprocess.run([os.path.join(tmp, "probe"), str(W * W)], check=True, capture_output=True, text=True)
                tables[W] = np.array([float.fromhex(x) for x in out.stdout.split()], np.float64)
                assert tables[W].tolist() == [dropin_expect.enumL(W * W, r) for r in range(W * W + 1)]
                arrays[f"enuml_W{W}"] = tables[W]
            pbm = os.path.join(tmp, f"case{n}.pbm")
            write_pbm(pbm, plane, cols)
            nt = ((rows + W - 1) // W) * ((cols + W - 1) // W)
            arrays[f"c{n}_plane"] = plane
            entry = dict(case, rows=rows, cols=cols, variants={})
            for v in case["variants"]:
                argv = [os.path.join(tmp, f"compress{v}"), pbm, str(W)] + ([str(T)] if v == 3 else [])
                out = subprocess.run(argv, check=True, capture_output=True, text=True).stdout
                rec, summary = parse(out, nt)
                for k, a in rec.items():
                    arrays[f"c{n}_v{v}_{k}"] = a
                entry["variants"][str(v)] = summary
            meta.append(entry)
    np.savez_compressed(os.path.join(HERE, "dict.npz"), **arrays)
    with open(os.path.join(HERE, "dict.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote", len(arrays), "arrays,", os.path.getsize(os.path.join(HERE, "dict.npz")), "bytes")


if __name__ == "__main__":
    main()
