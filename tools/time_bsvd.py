"""Timing of the dictionary learning steps (measurement for DESIGN.md §3, not a test): image mode, a
4096 x 4096 image in 16 x 16 patches, so n = 65536 samples of m = 256 bits and p = 512 atoms, on a planted
model made on the device (D0 at density 0.3, 0 to 2 atoms per row, X = A0 D0 ^ 2 % noise, D = D0 with 5 % of
its bits flipped, A = 0, E = X).

Per repeat the start state is restored, the device synced, and ONE call bracketed by two events:

  coefficients   bic_bsvd_update_coefficients from the start state
  dictionary     bic_bsvd_update_dictionary on that call's output
  learn          bic_bsvd_learn from the start state (it blocks: host wall time as well)

One JSON line per (step, repeat), then a summary line with

  * the work of one sparse-coding round, n p ceil(m/64) XOR + popcount word operations, and the rate the
    coefficients call reached: rounds are counted as one scan of all atoms per step taken (the bits of A the
    call changed; a coefficient toggled twice in one call would be missed) plus every row's last scan;
  * the number of kernel launches a dictionary update makes (every launch bracketed, a pass of its own).

Needs a device; fails without one.
Usage: python tools/time_bsvd.py [--repeats 5] [--out profiles/r11/time_bsvd.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-image-compression_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--p", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "time_bsvd.jsonl"))
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
    A_start = torch.zeros(n, pw, dtype=torch.int64, device=ctx.dev)
    E, D, A = X.clone(), D_start.clone(), A_start.clone()
    ch = ctx.empty_i64(1)
    ctx.sync()

    def popcount(t):
        return int(np.unpackbits(pybic.as_u64(t).view(np.uint8)).sum())

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    f = open(args.out, "a")
    config = f"n={n} m={m} p={p} planted (D0 0.3, 0-2 atoms per row, noise 0.02, D flips 0.05, A = 0)"

    def emit(d):
        line = json.dumps(d)
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

    def restore():
        E.copy_(X)
        D.copy_(D_start)
        A.copy_(A_start)

    ms = {"coefficients": [], "dictionary": [], "learn": []}
    info = {}
    for r in range(args.repeats + 1):  # repeat 0 warms up (module load, the scratch's first size)
        restore()
        t_c, _, _ = bracket(lambda: ctx.bsvd_update_coefficients(E, m, D, A, p, changed=ch))
        info["rows_changed"] = int(pybic.as_u64(ch)[0])
        info["steps_taken"] = popcount(A)
        info["weight_before"], info["weight_after_coefficients"] = popcount(X), popcount(E)
        t_d, _, _ = bracket(lambda: ctx.bsvd_update_dictionary(E, m, D, A, p, changed=ch))
        info["atoms_changed"] = int(pybic.as_u64(ch)[0])
        info["weight_after_dictionary"] = popcount(E)
        restore()
        t_l, wall_l, iters = bracket(lambda: ctx.bsvd_learn(X, E, m, D, A, p))
        info["learn_iterations"], info["weight_after_learn"] = iters, popcount(E)
        if r == 0:
            continue
        for step, t in (("coefficients", t_c), ("dictionary", t_d), ("learn", t_l)):
            ms[step].append(t)
            rec = {"tool": "time_bsvd", "config": config, "step": step, "repeat": r, "ms": round(t, 4)}
            if step == "learn":
                rec["host_wall_ms"], rec["iterations"] = round(wall_l, 4), iters
            emit(rec)
    # the dictionary update's launches: every launch bracketed, a pass of its own
    restore()
    ctx.bsvd_update_coefficients(E, m, D, A, p, changed=ch)
    ctx.sync()
    ctx.prof_collect()
    ctx.prof_enable(True)
    ctx.bsvd_update_dictionary(E, m, D, A, p, changed=ch)
    prof = ctx.prof_collect()
    ctx.prof_enable(False)
    round_ops = n * p * mw
    rounds = (n + info["steps_taken"]) / n
    best = min(ms["coefficients"])
    emit({"tool": "time_bsvd", "config": config, "summary": True,
          **{f"{k}_ms": [round(x, 4) for x in v] for k, v in ms.items()}, **info,
          "round_word_ops": round_ops, "rounds_per_call": round(rounds, 4),
          "coefficients_word_ops_per_s": round(round_ops * rounds / (best * 1e-3), 1),
          "coefficients_bit_ops_per_s": round(64 * round_ops * rounds / (best * 1e-3), 1),
          "dictionary_launches": {k: v[0] for k, v in sorted(prof.items())},
          "dictionary_kernel_ms": {k: round(v[1], 4) for k, v in sorted(prof.items())}})
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
