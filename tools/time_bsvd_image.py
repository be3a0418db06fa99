"""Timing of the image mode (measurement for DESIGN.md §3 "Image mode", not a test): a 4096 x 4096 plane in 16 x 16
patches, n = 65536 samples of m = 256 bits, p = 512 atoms. The samples are the planted model of tools/time_bsvd.py
(the same generator, so the sparse-coding call below is that tool's call); the plane is their scatter.

Per repeat, alternating in one process, ONE call between two device syncs each, timed by two events around it:

  bic_patches_gather   the plane -> X (2 MiB in, 2 MiB out)
  bic_patches_scatter  X -> the plane (2 MiB in, 2 MiB out)
  bic_mosaic of D      512 x 256 -> a 391 x 391 image
  bic_mosaic of E      65536 x 256 -> a 4352 x 4352 image
  bic_bsvd_update_coefficients on the same samples, from the planted start: the yardstick

The criterion (the initialisers' criterion: forming the samples must not be what a learning run waits for): the
slowest repeat of the gather, and the slowest repeat of the scatter, each lie below the fastest repeat of the
sparse-coding call. Bytes moved over time is reported per kernel as a fraction of the 8 TB/s peak, for orientation:
at these sizes a call is bound by its launch, not by the memory system.

For information, the wall time of the two loops over the host binary_matrix (tests/cpp/patch_host_check.cpp, built
with g++ into a temporary directory) and of the upload of X they would need.

--check compares all three outputs at full size with tests/patch_ref.py.

Needs a device; fails without one.
Usage: python tools/time_bsvd_image.py [--repeats 5] [--check] [--out profiles/r17/time_bsvd_image.jsonl]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "binary-image-compression_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = 8e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--W", type=int, default=16)
    ap.add_argument("--p", type=int, default=512)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "time_bsvd_image.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import patch_ref as P
    import pybic
    from pnm_io import write_pbm
    ctx = pybic.Context(0)  # raises without a device
    rows = cols = args.side
    W, p = args.W, args.p
    m = W * W
    n = ((rows + W - 1) // W) * ((cols + W - 1) // W)
    mw, pw, used = (m + 63) // 64, (p + 63) // 64, (cols + 63) // 64

    # the planted model of tools/time_bsvd.py
    gen = torch.Generator(device=ctx.dev)
    gen.manual_seed(0xB5D)
    shifts = (63 - torch.arange(64, device=ctx.dev, dtype=torch.int64))

    def pack(bits):
        r, c = bits.shape
        w = (c + 63) // 64
        b = torch.zeros(r, w * 64, dtype=torch.int64, device=ctx.dev)
        b[:, :c] = bits
        return (b.view(r, w, 64) << shifts).sum(dim=2)

    def rand(r, c, density):
        return torch.rand(r, c, device=ctx.dev, generator=gen) < density

    D0 = rand(p, m, 0.3)
    cnt = torch.randint(0, 3, (n,), device=ctx.dev, generator=gen)
    k1 = torch.randint(0, p, (n,), device=ctx.dev, generator=gen)
    k2 = (k1 + torch.randint(1, p, (n,), device=ctx.dev, generator=gen)) % p
    A0 = torch.zeros(n, p, dtype=torch.bool, device=ctx.dev)
    idx = torch.arange(n, device=ctx.dev)
    A0[idx[cnt >= 1], k1[cnt >= 1]] = True
    A0[idx[cnt >= 2], k2[cnt >= 2]] = True
    X0 = ctx.empty_i64(n, mw)
    ctx.gf2_mul(pybic.GF2_AB, pack(A0), p, pack(D0), m, X0, m)
    X0 ^= pack(rand(n, m, 0.02))
    D_start = pack(D0 ^ rand(p, m, 0.05))
    A_start = torch.zeros(n, pw, dtype=torch.int64, device=ctx.dev)
    plane = ctx.patches_scatter(X0, W, rows, cols)
    X, back = ctx.empty_i64(n, mw), ctx.empty_i64(rows, used)
    E, D, A = X0.clone(), D_start.clone(), A_start.clone()
    ch = ctx.empty_i64(1)
    dr, dc = ctx.mosaic_dims(p, m)
    er, ec = ctx.mosaic_dims(n, m)
    img_d, img_e = ctx.empty_i64(dr, (dc + 63) // 64), ctx.empty_i64(er, (ec + 63) // 64)
    ctx.sync()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    f = open(args.out, "a")
    config = f"{rows}x{cols} plane, W={W}: n={n} m={m} p={p}, the planted samples of tools/time_bsvd.py"

    def emit(d):
        line = json.dumps({"tool": "time_bsvd_image", "config": config, **d})
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    def bracket(fn):
        """one call between two device syncs -> ms between two events around it"""
        ctx.sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ctx.sync()
        return e0.elapsed_time(e1)

    if args.check:
        Ih, Xh = pybic.as_u64(plane), pybic.as_u64(X0)
        Dh = pybic.as_u64(D_start)
        ctx.patches_gather(plane, cols, W, out=X)
        ctx.mosaic(D_start, m, out=img_d)
        ctx.mosaic(X0, m, out=img_e)
        ctx.sync()
        same = {"scatter": bool(np.array_equal(Ih, P.scatter(Xh, W, rows, cols))),
                "gather": bool(np.array_equal(pybic.as_u64(X), P.gather(Ih, cols, W))),
                "gather_returns_the_samples": bool(np.array_equal(pybic.as_u64(X), Xh)),
                "mosaic_D": bool(np.array_equal(pybic.as_u64(img_d), P.mosaic(Dh, m))),
                "mosaic_E": bool(np.array_equal(pybic.as_u64(img_e), P.mosaic(Xh, m)))}
        ok = all(same.values())
        emit({"check": True, "equal": same, "ok": ok})
        if not ok:
            sys.exit("the device and the restatement differ")

    calls = {
        "patches_gather": (lambda: ctx.patches_gather(plane, cols, W, out=X), rows * used * 8 + n * mw * 8),
        "patches_scatter": (lambda: ctx.patches_scatter(X0, W, rows, cols, out=back), rows * used * 8 + n * mw * 8),
        "mosaic_D": (lambda: ctx.mosaic(D_start, m, out=img_d), p * mw * 8 + img_d.numel() * 8),
        "mosaic_E": (lambda: ctx.mosaic(X0, m, out=img_e), n * mw * 8 + img_e.numel() * 8),
        "update_coefficients": (lambda: ctx.bsvd_update_coefficients(E, m, D, A, p, changed=ch), None),
    }
    ms = {c: [] for c in calls}
    for r in range(args.repeats + 1):  # repeat 0 warms up (module load, the scratch's first size)
        for name, (fn, nbytes) in calls.items():
            if name == "update_coefficients":
                E.copy_(X0)
                A.copy_(A_start)
            t = bracket(fn)
            if r:
                ms[name].append(t)
                d = {"call": name, "repeat": r, "ms": round(t, 4)}
                if nbytes:
                    d["bytes"] = nbytes
                    d["fraction_of_8TBps"] = round(nbytes / (t * 1e-3) / PEAK, 4)
                else:
                    d["rows_changed"] = int(pybic.as_u64(ch)[0])
                emit(d)
    yard = min(ms["update_coefficients"])
    emit({"summary": True,
          "criterion": "max of patches_gather and max of patches_scatter each < min of update_coefficients",
          "ms_min_max": {c: [round(min(v), 4), round(max(v), 4)] for c, v in ms.items()},
          "fraction_of_8TBps_at_min": {c: round(calls[c][1] / (min(ms[c]) * 1e-3) / PEAK, 4)
                                       for c in calls if calls[c][1]},
          "update_coefficients_min_ms": round(yard, 4),
          "met": {c: bool(max(ms[c]) < yard) for c in ("patches_gather", "patches_scatter")}})

    # for information: the two loops over the host binary_matrix, and the upload of X they would need
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "patch_host_check")
        src = [os.path.join(ROOT, "tests", "cpp", "patch_host_check.cpp")]
        src += [os.path.join(PKG, "host", s) for s in ("binmat.cpp", "util.cpp", "pbm.cpp")]
        subprocess.run(["g++", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe] + src, check=True)
        Ih = pybic.as_u64(plane)
        Ih[0, 0] |= np.uint64(1 << 63)  # (a first raster byte that is not white space)
        pbm = write_pbm(os.path.join(tmp, "I.pbm"), Ih, cols)
        out = subprocess.run([exe, "time", pbm, str(W)], capture_output=True, text=True, check=True).stdout
    host = {k: float(v) for k, v in (kv.split("=") for kv in out.split()[:2])}
    Xh = torch.from_numpy(pybic.as_u64(X0).view(np.int64)).pin_memory()
    ups = []
    for r in range(args.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X.copy_(Xh)
        torch.cuda.synchronize()
        ups.append((time.perf_counter() - t0) * 1e3)
    emit({"host_loops": True, "host_gather_ms": host["gather_ms"], "host_scatter_ms": host["scatter_ms"],
          "upload_X_pinned_ms_min": round(min(ups[1:]), 4)})
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
