"""Timing of the PROXIMUS dictionary update (measurement for DESIGN.md §3, not a test): the planted image-mode
shape of tools/time_bsvd.py (n = 65536 samples of m = 256 bits, p = 512 atoms, made on the device), from two
start states:

  loop    the output of one sparse-coding call from (E = X, D, A = 0): the learning loop's case
  flips   A0 with 5 % of its bits flipped, E = X ^ A D, no sparse coding: many rounds per atom

Per repeat and start the state is restored, the device synced, and ONE call bracketed by two events, the calls
alternating in one process: bic_bsvd_update_dictionary (the steepest step, yardstick 1) and
bic_bsvd_update_dictionary_proximus with bic_set_bsvd_rounds 0 (automatic), 1, 2, 4 and 8. The call blocks, so
the host wall time is recorded as well. Then, in passes of their own with bic_prof_only (one kernel per pass):
the launches of both PROXIMUS kernels under the automatic budget (how many were enqueued; those beyond two per
round run left at once), the coefficient kernel on a converged model under budget 1 (every launch runs: one
full pass over E each, nothing written) and k_bsvd_xor over the same E (yardstick 2, through bic_bsvd_learn
with max_iter = 1). Last, bic_bsvd_learn_du with both rules from (X, D, A = 0).

One JSON line per (start, call, repeat), then one summary line per start and one for the passes.
--check runs the restatement (tests/bsvd_prox_ref.py) once at this size on the host from the loop start (minutes;
not part of the timing) and compares changed, rounds and every word of E, D and A.

Needs a device; fails without one.
Usage: python tools/time_bsvd_prox.py [--repeats 5] [--check] [--out profiles/r13/time_bsvd_prox.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-image-compression_amd"))

BUDGETS = (0, 1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--p", type=int, default=512)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "time_bsvd_prox.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import pybic
    ctx = pybic.Context(0)  # raises without a device
    n, m, p = args.n, args.m, args.p
    mw, pw = (m + 63) // 64, (p + 63) // 64
    gen = torch.Generator(device=ctx.dev)
    gen.manual_seed(0xB5D)
    shifts = (63 - torch.arange(64, device=ctx.dev, dtype=torch.int64))

    def pack(bits):
        """bool [rows, cols] -> int64 words [rows, ceil(cols/64)], column j at bit 63 - j % 64"""
        rows, cols = bits.shape
        w = (cols + 63) // 64
        b = torch.zeros(rows, w * 64, dtype=torch.int64, device=ctx.dev)
        b[:, :cols] = bits
        return (b.view(rows, w, 64) << shifts).sum(dim=2)

    def rand(rows, cols, density):
        return torch.rand(rows, cols, device=ctx.dev, generator=gen) < density

    # the draws of tools/time_bsvd.py, in its order, then the flipped A
    D0 = rand(p, m, 0.3)
    cnt = torch.randint(0, 3, (n,), device=ctx.dev, generator=gen)
    k1 = torch.randint(0, p, (n,), device=ctx.dev, generator=gen)
    k2 = (k1 + torch.randint(1, p, (n,), device=ctx.dev, generator=gen)) % p
    A0 = torch.zeros(n, p, dtype=torch.bool, device=ctx.dev)
    rows = torch.arange(n, device=ctx.dev)
    A0[rows[cnt >= 1], k1[cnt >= 1]] = True
    A0[rows[cnt >= 2], k2[cnt >= 2]] = True
    X = ctx.empty_i64(n, mw)
    ctx.gf2_mul(pybic.GF2_AB, pack(A0), p, pack(D0), m, X, m)
    X ^= pack(rand(n, m, 0.02))
    D_start = pack(D0 ^ rand(p, m, 0.05))
    A_zero = torch.zeros(n, pw, dtype=torch.int64, device=ctx.dev)
    ch = ctx.empty_i64(1)
    starts = {}
    E, A = X.clone(), A_zero.clone()
    ctx.bsvd_update_coefficients(E, m, D_start, A, p, changed=ch)
    starts["loop"] = (E, A)
    A = pack(A0 ^ rand(n, p, 0.05))
    E = ctx.empty_i64(n, mw)
    ctx.gf2_mul(pybic.GF2_AB, A, p, D_start, m, E, m)
    E ^= X
    starts["flips"] = (E, A)
    E, D, A = X.clone(), D_start.clone(), A_zero.clone()
    ctx.sync()

    def popcount(t):
        return int(np.unpackbits(pybic.as_u64(t).view(np.uint8)).sum())

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    f = open(args.out, "a")
    config = f"n={n} m={m} p={p} planted (D0 0.3, 0-2 atoms per row, noise 0.02, D flips 0.05)"

    def emit(d):
        line = json.dumps({"tool": "time_bsvd_prox", "config": config, **d})
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    def bracket(fn):
        ctx.sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, r

    def restore(start):
        E.copy_(starts[start][0])
        D.copy_(D_start)
        A.copy_(starts[start][1])

    def profiled(name, fn):
        ctx.sync()
        ctx.prof_collect()
        ctx.prof_only(name)
        ctx.prof_enable(True)
        r = fn()
        launches, ms = ctx.prof_collect().get(name, (0, 0.0))
        ctx.prof_enable(False)
        ctx.prof_only(None)
        return launches, ms, r

    if args.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import bsvd_prox_ref as P
        restore("loop")
        Eh, Dh, Ah = (P.unpack(pybic.as_u64(t)) for t in (E, D, A))
        t0 = time.perf_counter()
        want = P.update_dictionary_proximus(Eh, Dh, Ah, m, p)
        host_s = time.perf_counter() - t0
        got = ctx.bsvd_update_dictionary_proximus(E, m, D, A, p)
        same = {k: bool(np.array_equal(pybic.as_u64(t), P.pack(h))) for k, t, h in
                (("E", E, Eh), ("D", D, Dh), ("A", A, Ah))}
        ok = tuple(got) == tuple(want) and all(same.values())
        emit({"check": True, "start": "loop", "device_changed_rounds": list(got), "restatement_changed_rounds":
              list(want), "words_equal": same, "restatement_s": round(host_s, 1), "ok": ok})
        if not ok:
            sys.exit("the device and the restatement differ")

    for start in ("loop", "flips"):
        calls = ["steepest"] + [f"proximus_r{b}" for b in BUDGETS]
        ms = {c: [] for c in calls}
        wall = {c: [] for c in calls}
        info = {"weight_before": popcount(starts[start][0])}
        for r in range(args.repeats + 1):  # repeat 0 warms up (module load, the scratch's first size)
            for c in calls:
                restore(start)
                if c == "steepest":
                    t, w, _ = bracket(lambda: ctx.bsvd_update_dictionary(E, m, D, A, p, changed=ch))
                    info["steepest_atoms_changed"], info["weight_after_steepest"] = int(pybic.as_u64(ch)[0]), popcount(E)
                else:
                    ctx.set_bsvd_rounds(int(c.split("_r")[1]))
                    t, w, (_, rounds) = bracket(lambda: ctx.bsvd_update_dictionary_proximus(E, m, D, A, p, changed=ch))
                    ctx.set_bsvd_rounds(0)
                    res = (int(pybic.as_u64(ch)[0]), rounds, popcount(E))
                    assert info.setdefault("proximus", res) == res, (c, res, info["proximus"])  # every budget: same result
                if r:
                    ms[c].append(t)
                    wall[c].append(w)
                    emit({"start": start, "call": c, "repeat": r, "ms": round(t, 4), "host_wall_ms": round(w, 4)})
        changed, rounds, weight = info.pop("proximus")
        # the automatic budget's launches, one kernel per pass
        launches = {}
        for name in ("bsvd_prox_atom", "bsvd_prox_coef"):
            restore(start)
            launches[name] = profiled(name, lambda: ctx.bsvd_update_dictionary_proximus(E, m, D, A, p, changed=ch))[:2]
        enq = sum(v[0] for v in launches.values())
        per_round = min(ms["proximus_r0"]) / rounds
        per_atom = min(ms["steepest"]) / p
        emit({"start": start, "summary": True, **info, "atoms_changed": changed, "rounds": rounds,
              "rounds_per_atom": round(rounds / p, 3), "weight_after_proximus": weight,
              **{f"{c}_ms": [round(x, 4) for x in v] for c, v in ms.items()},
              **{f"{c}_host_wall_ms": [round(x, 4) for x in v] for c, v in wall.items()},
              "launches_enqueued": enq, "launches_left_at_once": enq - 2 * rounds,
              "kernel_launches_ms": {k: [v[0], round(v[1], 4)] for k, v in launches.items()},
              "us_per_executed_round": round(per_round * 1e3, 3), "steepest_us_per_atom": round(per_atom * 1e3, 3),
              "round_over_steepest_atom": round(per_round / per_atom, 3)})

    # yardstick 2: the coefficient kernel when every launch runs (a converged model, budget 1) against k_bsvd_xor
    restore("loop")
    calls_to_settle = 0
    while ctx.bsvd_update_dictionary_proximus(E, m, D, A, p, changed=ch)[1] != p and calls_to_settle < 50:
        calls_to_settle += 1
    ctx.set_bsvd_rounds(1)
    coef = []
    for _ in range(args.repeats):
        l, t, (_, rounds) = profiled("bsvd_prox_coef",
                                     lambda: ctx.bsvd_update_dictionary_proximus(E, m, D, A, p, changed=ch))
        coef.append((l, rounds, t))
    ctx.set_bsvd_rounds(0)
    xor = []
    for _ in range(args.repeats + 1):
        E2, D2, A2 = E.clone(), D.clone(), A.clone()
        xor.append(profiled("bsvd_xor", lambda: ctx.bsvd_learn(X, E2, m, D2, A2, p, max_iter=1))[:2])
    xor = xor[1:]
    emit({"passes": True, "calls_to_settle": calls_to_settle + 1, "e_bytes": n * mw * 8,
          "coef_launches_rounds_ms": [[l, r, round(t, 4)] for l, r, t in coef],
          "coef_us_per_launch": [round(t / l * 1e3, 3) for l, r, t in coef],
          "xor_launches_ms": [[l, round(t, 4)] for l, t in xor],
          "xor_us_per_launch": [round(t / l * 1e3, 3) for l, t in xor]})

    # the loop with either rule, from (X, D, A = 0)
    for du, name in ((pybic.BSVD_DU_STEEPEST, "steepest"), (pybic.BSVD_DU_PROXIMUS, "proximus")):
        res = []
        for r in range(args.repeats + 1):
            D.copy_(D_start)
            A.copy_(A_zero)
            t, w, iters = bracket(lambda: ctx.bsvd_learn(X, E, m, D, A, p, du=du))
            if r:
                res.append((t, w))
        emit({"learn": True, "rule": name, "iterations": iters, "ms": [round(t, 4) for t, _ in res],
              "host_wall_ms": [round(w, 4) for _, w in res], "weight_before": popcount(X),
              "weight_after": popcount(E)})
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
