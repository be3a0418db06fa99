"""What BIC_OPT_GRAY_CODE costs and what it buys (measurement for DESIGN.md §3 "Gray code", not a test): one
16384 x 16384 8-bit image (configs[2]'s size, device-resident), smooth with a little noise --
v = 128 + 60 sin(i / 97) + 50 cos(j / 131) + N(0, 1.5), rounded and clipped -- all 8 planes.

  encode   bic_encode_gray, planes NULL, both streams into slots (the default C3 step)
  encode_same_streams
           the same call with the option on, on the image whose code is the tool's image (its samples sent
           through the inverse first): the streams are those of `encode` with the option off, word for word,
           so the difference from it is the transform's own cost and nothing the coded content changes
  decode   bic_decode_gray from that image's packed EG streams, and from its packed Golomb streams with the
           row index bic_encode_gray_packed wrote

The option alternates off / on in ONE process, `--repeats` times, each repeat `--steps` calls between
device syncs after a warm-up; the encode runs on two images used in turn so that the Infinity Cache cannot
serve a re-run. One JSON line per (repeat, call, option), then the count pass's own time off and on (bracketed
launches, a pass of its own), the Golomb and EG bits per plane and in total off and on, and a summary line.
--check round-trips the image bit-exactly through encode -> decode with the option off and on, both coders,
before anything is timed (the run stops if a sample differs).
Needs a device; fails without one.
Usage: python tools/time_graycode.py [--check] [--steps 20] [--repeats 4] [--out profiles/r18/time_graycode.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-image-compression_amd"))


def smooth_image(torch, dev, rows, cols, seed):
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
        v = v + 1.5 * torch.randn((r1 - r0, cols), device=dev, generator=gen)
        out[r0:r1] = v.round().clamp_(0, 255).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--cols", type=int, default=16384)
    ap.add_argument("--check", action="store_true", help="round-trip the image bit-exactly, option off and on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "time_graycode.jsonl"))
    args = ap.parse_args()
    import torch
    import pybic
    ctx = pybic.Context(0)  # raises without a device
    ctx.set_encoder("staged")
    rows, cols, n = args.rows, args.cols, 8
    imgs = [smooth_image(torch, ctx.dev, rows, cols, 0x6C0DE + k) for k in range(2)]
    sg, se = ctx.slot_words(rows, cols, 0), ctx.slot_words(rows, cols, 1)
    og, oe = ctx.empty_i64(n, sg), ctx.empty_i64(n, se)
    bg, be = ctx.empty_i64(n), ctx.empty_i64(n)
    back = torch.zeros((rows, cols), dtype=torch.uint8, device=ctx.dev)

    def encode(img):
        ctx.encode_gray(img, store_planes=False, outs=(og, oe), bits=(bg, be))

    def ungray(img):  # the inverse on the device: v = g ^ (g >> 1) ^ ... ^ (g >> 7)
        v = img ^ (img >> 1)
        v = v ^ (v >> 2)
        return v ^ (v >> 4)

    uimgs = [ungray(img) for img in imgs]
    # option on, on the inverse-coded image == option off, on the image: bit counts and every stream word
    res = []
    for on, src in ((0, imgs[0]), (1, uimgs[0])):
        ctx.set_gray_code(bool(on))
        og.zero_()
        oe.zero_()
        encode(src)
        ctx.sync()
        nbg, nbe = pybic.as_u64(bg).copy(), pybic.as_u64(be).copy()
        res.append((nbg, nbe, [og[k, :(int(nbg[k]) + 63) // 64].clone() for k in range(n)],
                    [oe[k, :(int(nbe[k]) + 63) // 64].clone() for k in range(n)]))
    a, b = res
    if not ((a[0] == b[0]).all() and (a[1] == b[1]).all() and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
            and all(torch.equal(x, y) for x, y in zip(a[3], b[3]))):
        raise SystemExit("time_graycode: option on, on the inverse-coded image, differs from option off on the image")
    del res, a, b

    # per option: imgs[0]'s packed streams (what the decode calls read) and its bits per plane
    packed, bits = {}, {}
    for on in (0, 1):
        ctx.set_gray_code(bool(on))
        idx = ctx.empty_i64(n * rows * 2)
        _, g, e = ctx.encode_gray_packed(imgs[0], row_index=idx, store_planes=False)
        v00 = int(imgs[0][0, 0])
        c00 = v00 ^ (v00 >> 1) if on else v00
        p00 = torch.tensor([(c00 >> b) & 1 for b in range(n)], dtype=torch.uint8, device=ctx.dev)
        ctx.sync()
        packed[on] = (g, e, idx, p00)
        bits[on] = ([int(x) for x in pybic.as_u64(g[1])], [int(x) for x in pybic.as_u64(e[1])])

    def decode_eg(on):
        _, (out, b, off), _, p00 = packed[on]
        ctx.decode_gray(pybic.CODER_EG, out, b, n, rows, cols, True, word_off=off, p00=p00, out=back)

    def decode_golomb(on):
        (out, b, off), _, idx, p00 = packed[on]
        ctx.decode_gray(pybic.CODER_GOLOMB, out, b, n, rows, cols, True, word_off=off, row_index=idx, p00=p00, out=back)

    checked = None
    if args.check:
        for on in (0, 1):
            ctx.set_gray_code(bool(on))
            for name, fn in (("eg", decode_eg), ("golomb", decode_golomb)):
                back.zero_()
                fn(on)
                ctx.sync()
                if not torch.equal(back, imgs[0]):
                    raise SystemExit(f"time_graycode: the {name} round trip with the option at {on} differs from the image")
        checked = True

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    f = open(args.out, "w")

    def emit(d):
        d = dict({"tool": "time_graycode", "config": f"{rows}x{cols} 8-bit, smooth + N(0, 1.5), 8 planes, Golomb + EG"}, **d)
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

    calls = ("encode", "encode_same_streams", "decode_eg", "decode_golomb")
    ms = {(c, on): [] for c in calls for on in (0, 1)}
    for r in range(args.repeats):
        for on in (0, 1):
            ctx.set_gray_code(bool(on))
            for c, fn in (("encode", lambda i: encode(imgs[i & 1])),
                          ("encode_same_streams", lambda i: encode((uimgs if on else imgs)[i & 1])),
                          ("decode_eg", lambda i: decode_eg(on)),
                          ("decode_golomb", lambda i: decode_golomb(on))):
                t = timed(fn)
                ms[(c, on)].append(t)
                emit({"repeat": r, "call": c, "gray_code": on, "steps": args.steps, "ms_per_step": round(t, 4)})
    # the count pass alone (bracketed launches; a pass of its own, after the A/B)
    kern = {}
    for on in (0, 1):
        ctx.set_gray_code(bool(on))
        for name, fn in (("bitplanes_count", lambda i: encode(imgs[i & 1])),):
            ctx.prof_enable(True)
            ctx.prof_only(name)
            for i in range(args.steps):
                fn(i)
            prof = ctx.prof_collect()
            ctx.prof_only(None)
            ctx.prof_enable(False)
            cnt = prof.get(name, (0, 0.0))
            kern[(name, on)] = round(cnt[1] * 1e3 / max(cnt[0], 1), 1)
    ctx.set_gray_code(False)
    emit({"count_pass_us": {"off": kern[("bitplanes_count", 0)], "on": kern[("bitplanes_count", 1)]}, "steps": args.steps})
    for coder, k in (("golomb", 0), ("eg", 1)):
        emit({"stream_bits": coder, "per_plane_off": bits[0][k], "per_plane_on": bits[1][k],
              "total_off": sum(bits[0][k]), "total_on": sum(bits[1][k]),
              "on_over_off": round(sum(bits[1][k]) / sum(bits[0][k]), 4)})
    summary = {"summary": True, "round_trip_checked": checked}
    for c in calls:
        off, on = ms[(c, 0)], ms[(c, 1)]
        summary[c] = {"off_ms": [round(x, 4) for x in off], "on_ms": [round(x, 4) for x in on],
                      "off_median_ms": round(sorted(off)[len(off) // 2], 4), "on_median_ms": round(sorted(on)[len(on) // 2], 4)}
    emit(summary)
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
