"""What BIC_OPT_SAMPLE_PREDICT costs and what it buys (measurement for DESIGN.md §3 "Sample prediction", not a
test): tools/time_graycode.py's image -- 16384 x 16384 8-bit, device-resident, smooth with a little noise,
v = 128 + 60 sin(i / 97) + 50 cos(j / 131) + N(0, sigma), rounded and clipped -- all 8 planes.

  states   none, gray (BIC_OPT_GRAY_CODE), sp2 (BIC_SP_LEFT_FOLDED), sp2+gray
  encode   bic_encode_gray, planes NULL, both streams into slots (the default C3 step), in every state
  decode   bic_decode_gray from the image's packed EG streams, and from its packed Golomb streams with the row
           index bic_encode_gray_packed wrote, in the states none and sp2

The states alternate in ONE process, `--repeats` times, each repeat `--steps` calls between device syncs after a
warm-up; the encode runs on two images used in turn so that the Infinity Cache cannot serve a re-run. One JSON line
per (repeat, call, state), then the count pass's own time in every state and the inverse kernel's own time with its
share of the decode (bracketed launches, passes of their own), the Golomb and EG bits per plane and in total for
every state with `predict` 1 and 0, and a summary line.
--check round-trips the image bit-exactly through encode -> decode in every state, both coders, before anything is
timed (the run stops if a sample differs).
Needs a device; fails without one.
Usage: python tools/time_sample_predict.py [--check] [--steps 20] [--repeats 4] [--sigma 1.5]
                                           [--out profiles/r22/time_sample_predict.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-image-compression_amd"))

STATES = (("none", 0, 0), ("gray", 0, 1), ("sp2", 2, 0), ("sp2+gray", 2, 1))


def smooth_image(torch, dev, rows, cols, seed, sigma):
    """the tool's image, built row band by row band on the device (float temporaries of one band)"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    out = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
    j = torch.arange(cols, device=dev, dtype=torch.float32)
    cj = 50.0 * torch.cos(j / 131.0)
    band = 1024
    for r0 in range(0, rows, band):
        r1 = min(rows, r0 + band)
        i = torch.arange(r0, r1, device=dev, dtype=torch.float32)
        v = 128.0 + 60.0 * torch.sin(i / 97.0)[:, None] + cj[None, :]
        v = v + sigma * torch.randn((r1 - r0, cols), device=dev, generator=gen)
        out[r0:r1] = v.round().clamp_(0, 255).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--cols", type=int, default=16384)
    ap.add_argument("--sigma", type=float, default=1.5)
    ap.add_argument("--check", action="store_true", help="round-trip the image bit-exactly in every state")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "time_sample_predict.jsonl"))
    args = ap.parse_args()
    import torch
    import pybic
    ctx = pybic.Context(0)  # raises without a device
    ctx.set_encoder("staged")
    rows, cols, n = args.rows, args.cols, 8
    imgs = [smooth_image(torch, ctx.dev, rows, cols, 0x6C0DE + k, args.sigma) for k in range(2)]
    sg, se = ctx.slot_words(rows, cols, 0), ctx.slot_words(rows, cols, 1)
    og, oe = ctx.empty_i64(n, sg), ctx.empty_i64(n, se)
    bg, be = ctx.empty_i64(n), ctx.empty_i64(n)
    back = torch.zeros((rows, cols), dtype=torch.uint8, device=ctx.dev)
    v00 = int(imgs[0][0, 0])

    def state(name):
        _, sp, gc = next(s for s in STATES if s[0] == name)
        ctx.set_sample_predict(sp)
        ctx.set_gray_code(bool(gc))
        return sp, gc

    def encode(img, predict=True):
        ctx.encode_gray(img, predict=predict, store_planes=False, outs=(og, oe), bits=(bg, be))

    def pack(name):
        """imgs[0]'s packed streams in a state (what the decode calls read)"""
        sp, gc = state(name)
        idx = ctx.empty_i64(n * rows * 2)
        _, g, e = ctx.encode_gray_packed(imgs[0], row_index=idx, store_planes=False)
        p00 = torch.from_numpy(pybic.gray_p00(sp, gc, v00)).to(ctx.dev)
        ctx.sync()
        return g, e, idx, p00

    def decode_eg(p):
        _, (out, b, off), _, p00 = p
        ctx.decode_gray(pybic.CODER_EG, out, b, n, rows, cols, True, word_off=off, p00=p00, out=back)

    def decode_golomb(p):
        (out, b, off), _, idx, p00 = p
        ctx.decode_gray(pybic.CODER_GOLOMB, out, b, n, rows, cols, True, word_off=off, row_index=idx, p00=p00, out=back)

    checked = None
    if args.check:
        for name, _, _ in STATES:
            p = pack(name)
            for coder, fn in (("eg", decode_eg), ("golomb", decode_golomb)):
                back.zero_()
                fn(p)
                ctx.sync()
                if not torch.equal(back, imgs[0]):
                    raise SystemExit(f"time_sample_predict: the {coder} round trip in state {name} differs from the image")
            del p
        checked = True

    # bits per plane, every state, predict 1 and 0
    bits = {}
    for name, _, _ in STATES:
        state(name)
        for pr in (1, 0):
            encode(imgs[0], bool(pr))
            ctx.sync()
            bits[(name, pr)] = ([int(x) for x in pybic.as_u64(bg)], [int(x) for x in pybic.as_u64(be)])
    packed = {name: pack(name) for name in ("none", "sp2")}

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    f = open(args.out, "w")

    def emit(d):
        d = dict({"tool": "time_sample_predict",
                  "config": f"{rows}x{cols} 8-bit, smooth + N(0, {args.sigma}), 8 planes, Golomb + EG"}, **d)
        line = json.dumps(d)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    stream = torch.cuda.current_stream()

    def timed(fn):
        for i in range(args.warmup):
            fn(i)
        ctx.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(args.steps):
            fn(i)
        e1.record(stream)
        e1.synchronize()
        ctx.sync()
        return e0.elapsed_time(e1) / args.steps

    ms = {}
    for r in range(args.repeats):
        for name, _, _ in STATES:
            state(name)
            calls = [("encode", lambda i: encode(imgs[i & 1]))]
            if name in packed:
                calls += [("decode_eg", lambda i: decode_eg(packed[name])),
                          ("decode_golomb", lambda i: decode_golomb(packed[name]))]
            for c, fn in calls:
                t = timed(fn)
                ms.setdefault((c, name), []).append(t)
                emit({"repeat": r, "call": c, "state": name, "steps": args.steps, "ms_per_step": round(t, 4)})

    # single kernels (bracketed launches; passes of their own, after the A/B)
    def kernel_us(name, fn):
        ctx.prof_enable(True)
        ctx.prof_only(name)
        for i in range(args.steps):
            fn(i)
        prof = ctx.prof_collect()
        ctx.prof_only(None)
        ctx.prof_enable(False)
        cnt = prof.get(name, (0, 0.0))
        return round(cnt[1] * 1e3 / max(cnt[0], 1), 1)

    count = {}
    for name, _, _ in STATES:
        state(name)
        count[name] = kernel_us("bitplanes_count", lambda i: encode(imgs[i & 1]))
    emit({"count_pass_us": count, "steps": args.steps})
    state("sp2")
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    inv = {}
    for c, fn in (("decode_eg", decode_eg), ("decode_golomb", decode_golomb)):
        us = kernel_us("sample_unpredict", lambda i: fn(packed["sp2"]))
        inv[c] = {"inverse_us": us, "decode_ms": med(ms[(c, "sp2")]),
                  "share": round(us / 1e3 / med(ms[(c, "sp2")]), 4)}
    emit({"inverse_kernel": inv, "steps": args.steps})
    state("none")
    for coder, k in (("golomb", 0), ("eg", 1)):
        for pr in (1, 0):
            base = sum(bits[("none", pr)][k])
            emit({"stream_bits": coder, "predict": pr,
                  "per_plane": {name: bits[(name, pr)][k] for name, _, _ in STATES},
                  "total": {name: sum(bits[(name, pr)][k]) for name, _, _ in STATES},
                  "bits_per_pixel_plane": {name: round(sum(bits[(name, pr)][k]) / (rows * cols * n), 4) for name, _, _ in STATES},
                  "over_none": {name: round(sum(bits[(name, pr)][k]) / base, 4) for name, _, _ in STATES}})
    summary = {"summary": True, "round_trip_checked": checked}
    for (c, name), v in ms.items():
        summary.setdefault(c, {})[name] = {"ms": [round(x, 4) for x in v], "median_ms": med(v)}
    emit(summary)
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
