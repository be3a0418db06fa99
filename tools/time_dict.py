"""Timing of the growing-dictionary tile coder (measurement for DESIGN.md §3, not a test): bic_dict_encode on a
4096 x 4096 glyph-like plane, W = 16, T = 32, variants 2 and 3, atom_step 1 and W.

The plane: every 16 x 16 tile is noise (a share of --noise) or one of 64 random glyphs with 0, 1, 2, 3 or 40
pixels flipped, so the dictionary grows to tens of thousands of atoms and most tiles find a near atom.

Per (variant, atom_step): one warm-up call, then --repeats calls, each bracketed by two events after a sync; one
more call with every launch bracketed (bic_prof_*), which gives the launch count and the time per kernel; and
the same loop on the CPU, in-process, word-parallel (numpy: a tile as W*W/64 words, XOR + bitwise_count against
all atoms at once), whose |D|, matches and L must equal the device's.

One JSON line per (variant, atom_step, repeat), then one summary line per (variant, atom_step):
  * pairs            sum over tiles of |D| as the tile saw it (the drivers' loop without its early exit)
  * pairs_per_s      pairs / the best call
  * dist_pairs       what the distance kernels compute: per block, its tiles x the atoms at its start
  * dist_word_ops_per_s   dist_pairs * W / the distance kernels' time (one 64-bit word per patch row: the unit of
                     tools/time_bsvd.py's coefficients_word_ops_per_s)
  * resolve_share    the resolve kernels' share of the kernel time of the call

Needs a device; fails without one.
Usage: python tools/time_dict.py [--repeats 5] [--out profiles/r12/time_dict.jsonl]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-image-compression_amd"))


def make_bits(np, size, W, noise, seed=0xD1C7):
    rng = np.random.default_rng(seed)
    n = size // W
    glyphs = rng.random((64, W, W)) < 0.5
    kind = rng.random((n, n)) < noise
    which = rng.integers(0, 64, (n, n))
    nflip = rng.choice([0, 1, 2, 3, 40], (n, n))
    tiles = glyphs[which]                                  # n, n, W, W
    flat = tiles.reshape(n * n, W * W).copy()
    for f in (1, 2, 3, 40):                                # flip f distinct pixels of the tiles that ask for it
        idx = np.flatnonzero(nflip.reshape(-1) == f)
        pos = rng.random((len(idx), W * W)).argsort(axis=1)[:, :f]
        flat[idx[:, None], pos] ^= True
    tiles = flat.reshape(n, n, W, W)
    tiles[kind] = rng.random((int(kind.sum()), W, W)) < 0.5
    return tiles.transpose(0, 2, 1, 3).reshape(size, size)


def cpu_loop(np, bits, W, T, variant, step, enuml):
    """the drivers' loop, word-parallel: -> (|D|, matches, L, pairs, seconds)"""
    size = bits.shape[0]
    n, M = size // W, W * W
    mw = (M + 63) // 64

    def words(win):
        b = np.zeros(mw * 64, bool)
        b[:M] = win.reshape(-1)
        return np.packbits(b).view(np.uint64)

    P = np.packbits(bits.reshape(n, W, n, W).transpose(0, 2, 1, 3).reshape(n * n, M), axis=1)
    P = np.ascontiguousarray(np.pad(P, ((0, 0), (0, mw * 8 - P.shape[1])))).view(np.uint64)
    wt = np.bitwise_count(P).sum(axis=1)
    h = 0.5 * math.log2(float(M)) if variant == 2 else 0.0
    atoms = np.zeros((n * n, mw), np.uint64)
    nD = matches = L = pairs = 0
    t0 = time.perf_counter()
    for t in range(n * n):
        nm = int((1 + enuml[wt[t]]) + h)
        bestd, push = M, True
        if nD:
            d = np.bitwise_count(atoms[:nD] ^ P[t]).sum(axis=1)
            pairs += nD
            bestd = min(M, int(d.min()))
            ml = int(((1 + math.ceil(math.log2(nD))) + enuml[bestd]) + h)
            match = nm > ml
            matches += match
            L += ml if match else nm
            push = (not match) if variant == 2 else bestd > T
        else:
            L += nm
        if push:
            i, j = divmod(t, n)
            atoms[nD] = P[t] if step == W else words(bits[i * step:i * step + W, j * step:j * step + W])
            nD += 1
    return nD, int(matches), int(L), pairs, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--W", type=int, default=16)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--noise", type=float, default=0.25)
    ap.add_argument("--block", type=int, default=256, help="tiles per block (256 is what 0 = automatic gives)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "time_dict.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import pybic
    ctx = pybic.Context(0)  # raises without a device
    size, W, T = args.size, args.W, args.T
    assert size % 64 == 0 and size % W == 0 and size // W <= size - W  # (atom_step = 1 windows stay inside)
    bits = make_bits(np, size, W, args.noise)
    plane = np.packbits(bits, axis=1).view(">u8").astype(np.uint64)
    d_plane = ctx.to_dev(plane)
    enuml = pybic.enum_table(W)
    B = min(args.block, 4096 // ((W + 7) // 8 * 8), 1024)
    ctx.set_dict_block(B)
    nt = (size // W) ** 2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    f = open(args.out, "a")
    config = f"{size}x{size} glyph-like (64 glyphs, flips 0/1/2/3/40, noise {args.noise}) W={W} T={T} block={B}"

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    def bracket(fn):
        ctx.sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for variant in (2, 3):
        for step in (1, W):
            call = lambda: ctx.dict_encode(d_plane, size, variant, W, T, step, enuml)  # noqa: E731
            ms = []
            for r in range(args.repeats + 1):  # repeat 0 warms up (module load, the arena's first size)
                t, got = bracket(call)
                if r:
                    ms.append(t)
                    emit({"tool": "time_dict", "config": config, "variant": variant, "atom_step": step, "repeat": r,
                          "ms": round(t, 4)})
            ctx.sync()
            st = [int(x) for x in pybic.as_u64(got["stats"])]
            dsize = got["dsize"].cpu().numpy().view(np.uint32).astype(np.int64)
            pairs = int(dsize.sum())
            starts = np.arange(0, nt, B)
            dist_pairs = int((dsize[starts] * np.minimum(B, nt - starts)).sum())
            ctx.prof_collect()
            ctx.prof_enable(True)
            call()
            prof = ctx.prof_collect()
            ctx.prof_enable(False)
            kernel_ms = sum(v[1] for v in prof.values())
            best = min(ms)
            rec = {"tool": "time_dict", "config": config, "summary": True, "variant": variant, "atom_step": step,
                   "ms": [round(x, 4) for x in ms], "tiles": nt, "matches": st[0], "bits_match": st[1],
                   "bits_nomatch": st[2], "L": st[3], "D": st[4], "pairs": pairs,
                   "pairs_per_s": round(pairs / (best * 1e-3), 1), "dist_pairs": dist_pairs,
                   "dist_word_ops_per_s": round(dist_pairs * W / (prof["dict_dist"][1] * 1e-3), 1),
                   "launches": {k: v[0] for k, v in sorted(prof.items())},
                   "kernel_ms": {k: round(v[1], 4) for k, v in sorted(prof.items())},
                   "resolve_share": round(prof["dict_resolve"][1] / kernel_ms, 4)}
            if not args.no_cpu:
                nD, matches, L, cpu_pairs, sec = cpu_loop(np, bits, W, T, variant, step, enuml)
                rec.update(cpu_word_parallel_s=round(sec, 3), cpu_pairs_per_s=round(cpu_pairs / sec, 1),
                           cpu_agrees=[nD, matches, L, cpu_pairs] == [st[4], st[0], st[3], pairs])
            emit(rec)
    f.close()
    ctx.set_dict_block(0)
    ctx.close()


if __name__ == "__main__":
    main()
