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
Needs a device; fails without one.
Usage: python tools/time_rgb.py [--check] [--steps 20] [--repeats 5] [--out profiles/r19/time_rgb.jsonl]"""
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
    imgs = [torch.randint(0, 256, (rows * cols * 3,), dtype=torch.uint8, device=ctx.dev, generator=gen)
            for _ in range(2)]
    sg, se = ctx.slot_words(rows, cols, 0), ctx.slot_words(rows, cols, 1)
    # one set of outputs per input buffer: the decoders then alternate between two sets of streams too
    sets = [dict(outs=(ctx.empty_i64(n * sg), ctx.empty_i64(n * se)), bits=(ctx.empty_i64(n), ctx.empty_i64(n)),
                 offs=(ctx.empty_i64(n + 1), ctx.empty_i64(n + 1)), row_index=ctx.empty_i64(n * rows * 2))
            for _ in range(2)]
    planes = ctx.empty_i64(n, rows, wpr)
    back = torch.empty((rows, 3 * cols), dtype=torch.uint8, device=ctx.dev)
    p00 = [torch.stack([(im[c] >> b) & 1 for c in range(3) for b in range(8)]).contiguous() for im in imgs]

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
    f = open(args.out, "w")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    stream = torch.cuda.current_stream()
    config = f"{rows}x{cols} RGB, one-byte samples, uniform, 24 planes, Golomb + EG packed, row index"

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
