"""A/B timing of the 16-bit gray encode (measurement for DESIGN.md §3, not a test): an 8192 x 16384 image
of two-byte samples (the input bytes of configs[2], uniform, device-resident, big-endian as in a P5
file), all 16 planes, both streams --

  one_call   bic_encode_gray16, planes NULL, both streams into slots (the EG stream as the residual source)
  two_call   bic_pgm_bitplanes, then bic_encode_planes2 on the 16 planes

First both variants' streams and bit counts are compared word for word (the run stops if they differ).
Then the variants alternate in ONE process, `--repeats` times, each repeat `--steps` calls between
device syncs after a warm-up, on two input buffers used in turn so that the Infinity Cache cannot serve
a re-run. One JSON line per (repeat, variant), then a summary line (the criterion: the slowest one_call
repeat below the fastest two_call repeat) and the count pass's own time from the bracketed launches.
Needs a device; fails without one.
Usage: python tools/time_gray16.py [--steps 20] [--repeats 5] [--out profiles/r08/time_gray16.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-image-compression_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cols", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "time_gray16.jsonl"))
    args = ap.parse_args()
    assert args.steps >= 20 or args.rows < 8192, "at least 20 steps per variant at full size"
    import torch
    import pybic
    ctx = pybic.Context(0)  # raises without a device
    rows, cols, n = args.rows, args.cols, 16
    wpr = (cols + 63) // 64
    gen = torch.Generator(device=ctx.dev)
    gen.manual_seed(0x16B17)
    imgs = [torch.randint(0, 256, (rows * cols * 2,), dtype=torch.uint8, device=ctx.dev, generator=gen)
            for _ in range(2)]
    sg, se = ctx.slot_words(rows, cols, 0), ctx.slot_words(rows, cols, 1)
    og, oe = ctx.empty_i64(n, sg), ctx.empty_i64(n, se)
    bg, be = ctx.empty_i64(n), ctx.empty_i64(n)
    planes = ctx.empty_i64(n, rows, wpr)

    def one_call(img):
        ctx.encode_gray16(img, rows=rows, cols=cols, big_endian=True, store_planes=False, outs=(og, oe), bits=(bg, be))

    def two_call(img):
        ctx.pgm_bitplanes(img, rows, cols, 65535, n, out=planes)
        ctx.encode_planes2(planes, cols, True, outs=(og, oe), bits=(bg, be))

    # the two variants' streams, word for word
    res = {}
    for name, fn in (("one_call", one_call), ("two_call", two_call)):
        og.zero_()
        oe.zero_()
        fn(imgs[0])
        ctx.sync()
        nbg, nbe = pybic.as_u64(bg), pybic.as_u64(be)
        res[name] = (nbg, nbe, [og[k, :(int(nbg[k]) + 63) // 64].clone() for k in range(n)],
                     [oe[k, :(int(nbe[k]) + 63) // 64].clone() for k in range(n)])
    a, b = res["one_call"], res["two_call"]
    same = (a[0] == b[0]).all() and (a[1] == b[1]).all() and \
        all(torch.equal(x, y) for x, y in zip(a[2], b[2])) and all(torch.equal(x, y) for x, y in zip(a[3], b[3]))
    if not same:
        raise SystemExit("time_gray16: the one-call and two-call streams differ")
    stream_bytes = int(a[0].sum() + a[1].sum()) // 8
    del res, a, b

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    f = open(args.out, "w")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    stream = torch.cuda.current_stream()
    config = f"{rows}x{cols} two-byte samples, uniform, 16 planes, Golomb + EG"

    def timed(fn):
        for i in range(args.warmup):
            fn(imgs[i & 1])
        ctx.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(args.steps):
            fn(imgs[i & 1])
        e1.record(stream)
        e1.synchronize()
        ctx.sync()
        return e0.elapsed_time(e1) / args.steps

    ms = {"one_call": [], "two_call": []}
    for r in range(args.repeats):
        for name, fn in (("one_call", one_call), ("two_call", two_call)):
            t = timed(fn)
            ms[name].append(t)
            emit({"tool": "time_gray16", "config": config, "repeat": r, "variant": name, "steps": args.steps,
                  "ms_per_step": round(t, 4), "streams_equal": True})
    # the count pass alone (bracketed launches; a pass of its own, after the A/B)
    ctx.prof_enable(True)
    ctx.prof_only("bitplanes_count")
    for i in range(args.steps):
        one_call(imgs[i & 1])
    prof = ctx.prof_collect()
    ctx.prof_only(None)
    ctx.prof_enable(False)
    cnt = prof.get("bitplanes_count", (0, 0.0))
    emit({"tool": "time_gray16", "config": config, "summary": True,
          "one_call_ms": [round(x, 4) for x in ms["one_call"]], "two_call_ms": [round(x, 4) for x in ms["two_call"]],
          "one_call_slowest_ms": round(max(ms["one_call"]), 4), "two_call_fastest_ms": round(min(ms["two_call"]), 4),
          "criterion_met": bool(max(ms["one_call"]) < min(ms["two_call"])),
          "count_pass_us": round(cnt[1] * 1e3 / max(cnt[0], 1), 1), "count_pass_launches": cnt[0],
          "input_bytes": rows * cols * 2, "stream_bytes": stream_bytes})
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
