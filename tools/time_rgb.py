"""A/B timing of the interleaved-RGB encode and decode (measurement for DESIGN.md §3, not a test): a
5456 x 16384 image of three one-byte samples per pixel (configs[2]'s input bytes to within 0.1 %, uniform,
device-resident), all 24 planes, planes NULL, both streams packed, with the row index --

  encode  one_call   bic_encode_rgb_packed
          two_call   bic_bitplanes_rgb, then bic_encode_planes_packed on the 24 planes
  decode  one_call   bic_decode_rgb                              (from the Golomb and from the EG streams)
          two_call   bic_decode_planes, then bic_planes_to_rgb

With --check the two encode paths' bit counts, offsets, packed words and row indices are first compared word
for word, and each decode path's image byte for byte with the input (the run stops if any differ). Then the
variants alternate in ONE process, `--repeats` times, each repeat `--steps` calls between device syncs after
a warm-up, on two input buffers used in turn so that the Infinity Cache cannot serve a re-run. One JSON line
per (stage, repeat, variant), then per stage a summary line (the criterion: the slowest one_call repeat below
the fastest two_call repeat) and the count pass's own time from the bracketed launches.
--color-transform {0,1,2} and --gray-code set BIC_OPT_COLOR_TRANSFORM / BIC_OPT_GRAY_CODE for every call (p00
then comes from bic_rgb_p00); with a transform on, a further stage alternates the one-call encode with the
transform on and off (encode_ct_on_off). --input smooth replaces the uniform bytes by a luminance ramp with a
small chroma and noise; --stream-bits records the one-call stream bits of that input for every (transform, Gray
code) pair before the timing.
Needs a device; fails without one.
Usage: python tools/time_rgb.py [--check] [--steps 20] [--repeats 5] [--color-transform 1] [--gray-code]
       [--input smooth] [--stream-bits] [--out profiles/r20/time_rgb_ct.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-image-compression_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=5456)
    ap.add_argument("--cols", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "time_rgb.jsonl"))
    ap.add_argument("--color-transform", type=int, choices=(0, 1, 2), default=0)
    ap.add_argument("--gray-code", action="store_true")
    ap.add_argument("--input", choices=("uniform", "smooth"), default="uniform")
    ap.add_argument("--stream-bits", action="store_true")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    args = ap.parse_args()
    assert args.steps >= 20 or args.rows < 5456, "at least 20 steps per variant at full size"
    import torch
    import pybic
    from pybic import CODER_EG, CODER_GOLOMB, as_u64
    ctx = pybic.Context(0)  # raises without a device
    rows, cols, n = args.rows, args.cols, 24
    wpr = (cols + 63) // 64
    gen = torch.Generator(device=ctx.dev)
    gen.manual_seed(0x526742)
    ct, gc = args.color_transform, args.gray_code
    ctx.set_color_transform(ct)
    ctx.set_gray_code(gc)

    def smooth(k):
        """a luminance ramp shared by the three channels, a slow chroma of a few levels and noise of -1 .. 1"""
        i = torch.arange(rows, device=ctx.dev, dtype=torch.float32)[:, None]
        j = torch.arange(cols, device=ctx.dev, dtype=torch.float32)[None, :]
        y = 24 + (i * (80 / rows)).floor() + (j * (120 / cols)).floor() + (8 * torch.sin(j / 37 + k)).trunc() + \
            (8 * torch.cos(i / 11)).trunc()
        n = torch.randint(0, 3, (3, rows, cols), device=ctx.dev, generator=gen).float() - 1
        r = y + (6 * torch.sin(i / 9 + j / 50)).trunc() + n[0]
        g = y + n[1] + 1
        b = y + (5 * torch.cos(i / 13 - j / 70)).trunc() + n[2]
        return torch.stack([r, g, b], dim=2).clamp(0, 255).to(torch.uint8).reshape(-1).contiguous()

    if args.input == "smooth":
        imgs = [smooth(k) for k in range(2)]
    else:
        imgs = [torch.randint(0, 256, (rows * cols * 3,), dtype=torch.uint8, device=ctx.dev, generator=gen)
                for _ in range(2)]
    sg, se = ctx.slot_words(rows, cols, 0), ctx.slot_words(rows, cols, 1)
    # one set of outputs per input buffer: the decoders then alternate between two sets of streams too
    sets = [dict(outs=(ctx.empty_i64(n * sg), ctx.empty_i64(n * se)), bits=(ctx.empty_i64(n), ctx.empty_i64(n)),
                 offs=(ctx.empty_i64(n + 1), ctx.empty_i64(n + 1)), row_index=ctx.empty_i64(n * rows * 2))
            for _ in range(2)]
    planes = ctx.empty_i64(n, rows, wpr)
    back = torch.empty((rows, 3 * cols), dtype=torch.uint8, device=ctx.dev)
    p00 = [torch.from_numpy(pybic.rgb_p00(ct, gc, im[:3].cpu().numpy())).to(ctx.dev) for im in imgs]

    def enc_one(i):
        ctx.encode_rgb_packed(imgs[i], rows=rows, cols=cols, store_planes=False, **sets[i])

    def enc_two(i):
        ctx.bitplanes_rgb(imgs[i], rows=rows, cols=cols, out=planes)
        ctx.encode_planes_packed(planes, cols, True, golomb=True, eg=True, **sets[i])

    def dec_args(coder, i):
        k = 0 if coder == CODER_GOLOMB else 1
        s = sets[i]
        return dict(word_off=s["offs"][k], row_index=s["row_index"] if k == 0 else None, p00=p00[i]), s["outs"][k], s["bits"][k]

    def dec_one(coder, i):
        a, o, b = dec_args(coder, i)
        ctx.decode_rgb(coder, o, b, 8, rows, cols, True, out=back, **a)

    def dec_two(coder, i):
        a, o, b = dec_args(coder, i)
        ctx.decode_planes(coder, o, b, n, rows, cols, True, out=planes, **a)
        ctx.planes_to_rgb(planes, cols, out=back)

    checked = False
    if args.check:
        res = {}
        for name, fn in (("one_call", enc_one), ("two_call", enc_two)):
            s0 = sets[0]
            (og, oe), (bg, be), (fg, fe), idx = s0["outs"], s0["bits"], s0["offs"], s0["row_index"]
            for t in (og, oe, idx):
                t.zero_()
            fn(0)
            ctx.sync()
            tg, te = int(as_u64(fg)[n]), int(as_u64(fe)[n])
            res[name] = [x.clone() for x in (bg, be, fg, fe, og[:tg], oe[:te], idx)]
        if not all(torch.equal(x, y) for x, y in zip(res["one_call"], res["two_call"])):
            raise SystemExit("time_rgb: the one-call and two-call outputs differ")
        del res
        want = imgs[0].view(rows, 3 * cols)
        for coder in (CODER_GOLOMB, CODER_EG):
            for name, fn in (("one_call", dec_one), ("two_call", dec_two)):
                back.zero_()
                fn(coder, 0)
                ctx.sync()
                if not torch.equal(back, want):
                    raise SystemExit(f"time_rgb: decode {name} (coder {coder}) does not give the image back")
        checked = True
    for i in range(2):
        enc_one(i)
    ctx.sync()
    stream_bytes = int(as_u64(sets[0]["bits"][0]).sum() + as_u64(sets[0]["bits"][1]).sum()) // 8

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    f = open(args.out, "a" if args.append else "w")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    stream = torch.cuda.current_stream()
    config = (f"{rows}x{cols} RGB, one-byte samples, {args.input}, 24 planes, Golomb + EG packed, row index, "
              f"color_transform {ct}, gray_code {int(gc)}")
    if args.stream_bits:
        for m in (0, 1, 2):
            for g in (False, True):
                ctx.set_color_transform(m)
                ctx.set_gray_code(g)
                enc_one(0)
                ctx.sync()
                emit({"tool": "time_rgb", "stage": "stream_bits", "input": args.input, "rows": rows, "cols": cols,
                      "color_transform": m, "gray_code": int(g), "golomb_bits": int(as_u64(sets[0]["bits"][0]).sum()),
                      "eg_bits": int(as_u64(sets[0]["bits"][1]).sum()), "raw_bits": rows * cols * 24})
        ctx.set_color_transform(ct)
        ctx.set_gray_code(gc)
        for i in range(2):
            enc_one(i)
        ctx.sync()

    def timed(fn):
        for i in range(args.warmup):
            fn(i & 1)
        ctx.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(args.steps):
            fn(i & 1)
        e1.record(stream)
        e1.synchronize()
        ctx.sync()
        return e0.elapsed_time(e1) / args.steps

    def ab(stage, one, two):
        ms = {"one_call": [], "two_call": []}
        for r in range(args.repeats):
            for name, fn in (("one_call", one), ("two_call", two)):
                t = timed(fn)
                ms[name].append(t)
                emit({"tool": "time_rgb", "stage": stage, "config": config, "repeat": r, "variant": name,
                      "steps": args.steps, "ms_per_step": round(t, 4), "checked": checked})
        return ms

    def summary(stage, ms, **more):
        emit({"tool": "time_rgb", "stage": stage, "config": config, "summary": True,
              "one_call_ms": [round(x, 4) for x in ms["one_call"]], "two_call_ms": [round(x, 4) for x in ms["two_call"]],
              "one_call_slowest_ms": round(max(ms["one_call"]), 4), "two_call_fastest_ms": round(min(ms["two_call"]), 4),
              "criterion_met": bool(max(ms["one_call"]) < min(ms["two_call"])), "checked": checked, **more})

    ms = ab("encode", enc_one, enc_two)
    if ct:  # the one-call encode with the transform on against off, alternating (the streams differ: encode only)
        def enc_off(i):
            ctx.set_color_transform(0)
            enc_one(i)
            ctx.set_color_transform(ct)

        mo = {"ct_on": [], "ct_off": []}
        for r in range(args.repeats):
            for name, fn in (("ct_on", enc_one), ("ct_off", enc_off)):
                t = timed(fn)
                mo[name].append(t)
                emit({"tool": "time_rgb", "stage": "encode_ct_on_off", "config": config, "repeat": r, "variant": name,
                      "steps": args.steps, "ms_per_step": round(t, 4)})
        emit({"tool": "time_rgb", "stage": "encode_ct_on_off", "config": config, "summary": True,
              "ct_on_ms": [round(x, 4) for x in mo["ct_on"]], "ct_off_ms": [round(x, 4) for x in mo["ct_off"]],
              "ratio_of_medians": round(sorted(mo["ct_on"])[len(mo["ct_on"]) // 2] /
                                        sorted(mo["ct_off"])[len(mo["ct_off"]) // 2], 4)})
        for i in range(2):  # the decoders below read the streams of the transform in force
            enc_one(i)
        ctx.sync()
    # the count pass alone (bracketed launches; a pass of its own, after the A/B)
    ctx.prof_enable(True)
    ctx.prof_only("bitplanes_count")
    for i in range(args.steps):
        enc_one(i & 1)
    prof = ctx.prof_collect()
    ctx.prof_only(None)
    ctx.prof_enable(False)
    cnt = prof.get("bitplanes_count", (0, 0.0))
    us = cnt[1] * 1e3 / max(cnt[0], 1)
    summary("encode", ms, count_pass_us=round(us, 1), count_pass_launches=cnt[0], input_bytes=rows * cols * 3,
            count_pass_read_TBps=round(rows * cols * 3 / max(us, 1e-9) / 1e6, 3),
            count_pass_fraction_of_8TBps=round(rows * cols * 3 / max(us, 1e-9) / 1e6 / 8.0, 3), stream_bytes=stream_bytes)
    for stage, coder in (("decode_golomb", CODER_GOLOMB), ("decode_eg", CODER_EG)):
        ms = ab(stage, lambda i, c=coder: dec_one(c, i), lambda i, c=coder: dec_two(c, i))
        summary(stage, ms, output_bytes=rows * cols * 3)
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
