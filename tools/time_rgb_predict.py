"""What BIC_OPT_RGB_PREDICT costs and what it buys (measurement for DESIGN.md §3 "RGB sample prediction", not a
test): tools/time_rgb.py's smooth image -- 5456 x 16384 pixels of three one-byte samples, device-resident, a
luminance ramp shared by the channels with a slow chroma and noise of -1 .. 1 -- all 24 planes, and a batch of
64 frames of 1024 x 1408 pixels of the same kind.

  states   none, ct1+gray (BIC_CT_SUBTRACT_GREEN + BIC_OPT_GRAY_CODE: the best state without the option),
           rp2 (BIC_OPT_RGB_PREDICT = BIC_SP_LEFT_FOLDED), rp2+ct1
  encode   bic_encode_rgb / bic_encode_rgb_frames, planes NULL, both streams into slots, in every state
  decode   bic_decode_rgb / bic_decode_rgb_frames from the packed EG streams, and from the packed Golomb streams
           with the row index the packed encode wrote, in every state

The states alternate in ONE process, `--repeats` times, each repeat `--steps` calls between device syncs after a
warm-up; the single-image encode runs on two images used in turn so that the Infinity Cache cannot serve a re-run.
One JSON line per (shape, repeat, call, state), then per shape the count pass's own time in every state and the
inverse kernel's own time with its share of the decode (bracketed launches, passes of their own), the Golomb and
EG bits in total and per channel for every state with `predict` 1 and 0, and a summary line. Last, k_rgb_unpredict
against k_sample_unpredict on the same number of bytes (bic_planes_to_rgb on rows x cols pixels, bic_planes_to_gray
on rows x 3 cols samples), bracketed in the same process.
--check round-trips the inputs bit-exactly through encode -> decode in every state, both coders, before anything
is timed (the run stops if a sample differs).
Needs a device; fails without one.
Usage: python tools/time_rgb_predict.py [--check] [--steps 20] [--repeats 4]
                                        [--out profiles/r24/time_rgb_predict.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-image-compression_amd"))

# (name, BIC_OPT_RGB_PREDICT, BIC_OPT_COLOR_TRANSFORM, BIC_OPT_GRAY_CODE)
STATES = (("none", 0, 0, 0), ("ct1+gray", 0, 1, 1), ("rp2", 2, 0, 0), ("rp2+ct1", 2, 1, 0))


def smooth(torch, dev, gen, rows, cols, k):
    """tools/time_rgb.py's smooth image: [rows, cols, 3] uint8"""
    i = torch.arange(rows, device=dev, dtype=torch.float32)[:, None]
    j = torch.arange(cols, device=dev, dtype=torch.float32)[None, :]
    y = 24 + (i * (80 / rows)).floor() + (j * (120 / cols)).floor() + (8 * torch.sin(j / 37 + k)).trunc() + \
        (8 * torch.cos(i / 11)).trunc()
    n = torch.randint(0, 3, (3, rows, cols), device=dev, generator=gen).float() - 1
    r = y + (6 * torch.sin(i / 9 + j / 50)).trunc() + n[0]
    g = y + n[1] + 1
    b = y + (5 * torch.cos(i / 13 - j / 70)).trunc() + n[2]
    return torch.stack([r, g, b], dim=2).clamp(0, 255).to(torch.uint8).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--rows", type=int, default=5456)
    ap.add_argument("--cols", type=int, default=16384)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--frame-rows", type=int, default=1024)
    ap.add_argument("--frame-cols", type=int, default=1408)
    ap.add_argument("--check", action="store_true", help="round-trip the inputs bit-exactly in every state")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "time_rgb_predict.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import pybic
    from pybic import CODER_EG, CODER_GOLOMB, as_u64
    ctx = pybic.Context(0)  # raises without a device
    ctx.set_encoder("staged")
    gen = torch.Generator(device=ctx.dev)
    gen.manual_seed(0x526742)
    stream = torch.cuda.current_stream()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    f = open(args.out, "w")
    med = lambda v: round(sorted(v)[len(v) // 2], 4)  # noqa: E731

    def state(name):
        _, rp, ct, gc = next(s for s in STATES if s[0] == name)
        ctx.set_rgb_predict(rp)
        ctx.set_color_transform(ct)
        ctx.set_gray_code(bool(gc))
        return rp, ct, gc

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

    def report(shape, nf, rows, cols, imgs, count_name):
        """imgs: the inputs used in turn, each [nf, rows, cols, 3]; nf = 1: the single-image calls"""
        n = nf * 24
        wpr = (cols + 63) // 64
        config = f"{shape}: {nf} x {rows}x{cols} RGB, one-byte samples, smooth, {n} planes, Golomb + EG"
        sg, se = ctx.slot_words(rows, cols, 0), ctx.slot_words(rows, cols, 1)
        og, oe = ctx.empty_i64(n, sg), ctx.empty_i64(n, se)
        bg, be = ctx.empty_i64(n), ctx.empty_i64(n)
        back = torch.zeros((nf, rows, 3 * cols), dtype=torch.uint8, device=ctx.dev)
        flat = [im.reshape(-1) for im in imgs]
        first = [tuple(int(x) for x in px) for px in imgs[0][:, 0, 0, :].cpu().tolist()]  # every frame's first pixel

        def emit(d):
            line = json.dumps(dict({"tool": "time_rgb_predict", "config": config}, **d))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        def encode(i, predict=True):
            if nf == 1:
                ctx.encode_rgb(flat[i % len(flat)], rows=rows, cols=cols, predict=predict, store_planes=False, wpr=wpr,
                               outs=(og, oe), bits=(bg, be))
            else:
                ctx.encode_rgb_frames(flat[i % len(flat)], rows, cols, nframes=nf, predict=predict, wpr=wpr,
                                      outs=(og, oe), bits=(bg, be))

        def pack(name):
            """imgs[0]'s packed streams in a state (what the decode calls read)"""
            rp, ct, gc = state(name)
            idx = ctx.empty_i64(n * rows * 2)
            if nf == 1:
                _, g, e = ctx.encode_rgb_packed(flat[0], rows=rows, cols=cols, store_planes=False, wpr=wpr, row_index=idx)
            else:
                _, g, e = ctx.encode_rgb_frames_packed(flat[0], rows, cols, nframes=nf, wpr=wpr, row_index=idx)
            p00 = np.concatenate([pybic.rgb_p00_predict(ct, rp, gc, px) for px in first])
            ctx.sync()
            return g, e, idx, torch.from_numpy(p00).to(ctx.dev)

        def decode(coder, p):
            g, e, idx, p00 = p
            out, b, off = g if coder == CODER_GOLOMB else e
            ri = idx if coder == CODER_GOLOMB else None
            if nf == 1:
                ctx.decode_rgb(coder, out, b, 8, rows, cols, True, word_off=off, row_index=ri, p00=p00, out=back)
            else:
                ctx.decode_rgb_frames(coder, out, b, nf, 8, rows, cols, True, word_off=off, row_index=ri, p00=p00,
                                      out=back)

        checked = None
        if args.check:
            for name, *_ in STATES:
                p = pack(name)
                for cname, coder in (("eg", CODER_EG), ("golomb", CODER_GOLOMB)):
                    back.zero_()
                    decode(coder, p)
                    ctx.sync()
                    if not torch.equal(back.reshape(-1), flat[0]):
                        raise SystemExit(f"time_rgb_predict: {shape}: the {cname} round trip in state {name} differs "
                                         "from the input")
                del p
            checked = True

        bits = {}
        for name, *_ in STATES:
            state(name)
            for pr in (1, 0):
                encode(0, bool(pr))
                ctx.sync()
                bits[(name, pr)] = ([int(x) for x in as_u64(bg)], [int(x) for x in as_u64(be)])
        packed = {name: pack(name) for name, *_ in STATES}

        ms = {}
        for r in range(args.repeats):
            for name, *_ in STATES:
                state(name)
                for c, fn in (("encode", lambda i: encode(i)),
                              ("decode_eg", lambda i: decode(CODER_EG, packed[name])),
                              ("decode_golomb", lambda i: decode(CODER_GOLOMB, packed[name]))):
                    t = timed(fn)
                    ms.setdefault((c, name), []).append(t)
                    emit({"repeat": r, "call": c, "state": name, "steps": args.steps, "ms_per_step": round(t, 4)})

        count = {}
        for name, *_ in STATES:
            state(name)
            count[name] = kernel_us(count_name, lambda i: encode(i))
        emit({"count_pass_us": count, "count_pass": count_name, "steps": args.steps})
        inv = {}
        for name in ("rp2", "rp2+ct1"):
            state(name)
            for c, coder in (("decode_eg", CODER_EG), ("decode_golomb", CODER_GOLOMB)):
                us = kernel_us("rgb_unpredict", lambda i: decode(coder, packed[name]))
                inv[f"{name}/{c}"] = {"inverse_us": us, "decode_ms": med(ms[(c, name)]),
                                      "share": round(us / 1e3 / med(ms[(c, name)]), 4)}
        emit({"inverse_kernel": inv, "steps": args.steps})
        state("none")
        for cname, k in (("golomb", 0), ("eg", 1)):
            for pr in (1, 0):
                tot = {name: sum(bits[(name, pr)][k]) for name, *_ in STATES}
                emit({"stream_bits": cname, "predict": pr, "total": tot,
                      "per_channel": {name: [sum(sum(bits[(name, pr)][k][24 * fr + 8 * c:24 * fr + 8 * c + 8])
                                                 for fr in range(nf)) for c in range(3)] for name, *_ in STATES},
                      "bits_per_sample": {name: round(tot[name] / (nf * rows * cols * 3), 4) for name, *_ in STATES},
                      "over_none": {name: round(tot[name] / tot["none"], 4) for name, *_ in STATES},
                      "over_ct1_gray": {name: round(tot[name] / tot["ct1+gray"], 4) for name, *_ in STATES}})
        summary = {"summary": True, "round_trip_checked": checked}
        for (c, name), v in ms.items():
            summary.setdefault(c, {})[name] = {"ms": [round(x, 4) for x in v], "median_ms": med(v)}
        emit(summary)

    rows, cols = args.rows, args.cols
    imgs = [smooth(torch, ctx.dev, gen, rows, cols, k)[None] for k in range(2)]
    report("image", 1, rows, cols, imgs, "bitplanes_count")

    # the inverse kernel against the gray one on the same number of bytes (the stored bytes' values do not matter
    # to either: both read every byte of the rows and write it back)
    ctx.set_color_transform(0)
    ctx.set_gray_code(False)
    pl = torch.zeros((24, rows, (3 * cols + 63) // 64), dtype=torch.int64, device=ctx.dev)
    out = torch.zeros((rows, 3 * cols), dtype=torch.uint8, device=ctx.dev)
    ctx.set_rgb_predict(2)
    pl3 = pl[:, :, :(cols + 63) // 64].contiguous()
    rgb_us = kernel_us("rgb_unpredict", lambda i: ctx.planes_to_rgb(pl3, cols, out=out))
    ctx.set_rgb_predict(0)
    ctx.set_sample_predict(2)
    gray_us = kernel_us("sample_unpredict", lambda i: ctx.planes_to_gray(pl[:8], 3 * cols, out=out))
    ctx.set_sample_predict(0)
    line = json.dumps({"tool": "time_rgb_predict", "inverse_kernels": True, "bytes": rows * cols * 3,
                       "rgb_unpredict_us": rgb_us, "sample_unpredict_us": gray_us,
                       "ratio": round(rgb_us / max(gray_us, 1e-9), 3),
                       "rgb_unpredict_TBps": round(2 * rows * cols * 3 / max(rgb_us, 1e-9) / 1e6, 3)})
    print(line, flush=True)
    f.write(line + "\n")
    del imgs, pl, pl3, out

    nf, frows, fcols = args.frames, args.frame_rows, args.frame_cols
    frames = [torch.stack([smooth(torch, ctx.dev, gen, frows, fcols, k) for k in range(nf)])]
    report("frames", nf, frows, fcols, frames, "rgb_frames_count")
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
