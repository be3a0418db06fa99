"""A/B timing of the PBM calls (measurement for DESIGN.md §3, not a test): configs[3]'s size, 64 frames of
4096 x 4096 pixels as P4 rasters (uniform bits, device-resident), packed Golomb + EG streams with the row
index, in two layouts --

  files      64 concatenated P4 files (header "P4\\n4096 4096\\n": an odd stride, every frame aligned differently)
  aligned    the rasters alone, back to back from a 16-byte aligned base

and per layout and direction two variants --

  encode  one_call   bic_encode_pbm_packed, planes NULL
          two_call   64 x bic_pbm_unpack, then bic_encode_planes_packed
  decode  one_call   bic_decode_pbm (Golomb streams)
          two_call   bic_decode_planes, then 64 x bic_pbm_pack

First the variants' results are compared (streams, bit counts, offsets and row index word for word, the
decoded rasters byte for byte; the run stops if they differ) and the decoded rasters with the input (frames
that differ are listed in the summary lines). Then the variants alternate in ONE process,
`--repeats` times, each repeat `--steps` calls between device syncs after a warm-up, on two input buffers
used in turn so that the Infinity Cache cannot serve a re-run. One JSON line per (layout, direction, repeat,
variant), then per (layout, direction) a summary line (the criterion: the slowest one_call repeat below the
fastest two_call repeat) with the variants' kernel time per step (every launch bracketed, a pass of its
own: the step without the host's launch cost) and the raster count kernel's own time.
Needs a device; fails without one.
Usage: python tools/time_pbm.py [--steps 20] [--repeats 5] [--out profiles/r10/time_pbm.jsonl]"""
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
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--cols", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "time_pbm.jsonl"))
    args = ap.parse_args()
    assert (args.steps >= 20 and args.repeats >= 5) or args.rows < 4096, "at least 5 x 20 steps at full size"
    import torch
    import pybic
    ctx = pybic.Context(0)  # raises without a device
    rows, cols, n = args.rows, args.cols, args.frames
    wpr, nb = (cols + 63) // 64, (cols + 7) // 8
    assert wpr % 2 == 0, "the one-read count pass needs an even row pitch"
    fb = rows * nb
    header = f"P4\n{cols} {rows}\n".encode()
    G = pybic.CODER_GOLOMB

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    f = open(args.out, "w")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    stream = torch.cuda.current_stream()
    gen = torch.Generator(device=ctx.dev)
    gen.manual_seed(0x9B4)
    planes = ctx.empty_i64(n, rows, wpr)
    idx = ctx.empty_i64(n * rows * 2)
    bufs = ctx._packed_bufs(n, rows, cols, True, True, (None, None), (None, None), (None, None), (None, None))
    (og, sg, bg, fg), (oe, se, be, fe) = bufs
    outs, bits, offs = (og, oe), (bg, be), (fg, fe)

    for layout in ("files", "aligned"):
        lead = len(header) if layout == "files" else 0
        stride = lead + fb
        total = n * stride
        imgs = []
        for _ in range(2):
            b = torch.randint(0, 256, (total + 64,), dtype=torch.uint8, device=ctx.dev, generator=gen)
            if lead:
                hdr = torch.tensor(list(header), dtype=torch.uint8, device=ctx.dev)
                for k in range(n):
                    b[k * stride:k * stride + lead] = hdr
            assert b.data_ptr() % 16 == 0
            imgs.append(b[lead:])  # frame 0's first raster byte
        back = torch.zeros(total + 64, dtype=torch.uint8, device=ctx.dev)[lead:]
        config = f"{n} frames {rows}x{cols} P4, uniform, layout {layout} (stride {stride}), packed Golomb + EG + row index"

        def enc_one(img):
            ctx.encode_pbm_packed(img, rows, cols, n, stride, True, planes=None, outs=outs, bits=bits, offs=offs,
                                  row_index=idx)

        def enc_two(img):
            for k in range(n):
                ctx.lib.bic_pbm_unpack(ctx.h, img.data_ptr() + k * stride, rows, cols, planes[k].data_ptr(), wpr)
            ctx.encode_planes_packed(planes, cols, True, golomb=True, eg=True, outs=outs, bits=bits, offs=offs,
                                     row_index=idx)

        # the two encodes, word for word
        res = {}
        for name, fn in (("one_call", enc_one), ("two_call", enc_two)):
            for t in (og, oe, idx):
                t.zero_()
            ctx._bind_stream()
            fn(imgs[0])
            ctx.sync()
            tg, te = int(pybic.as_u64(fg)[-1]), int(pybic.as_u64(fe)[-1])
            res[name] = [x.clone() for x in (bg, be, fg, fe, idx, og[:tg], oe[:te])]
        if not all(torch.equal(x, y) for x, y in zip(res["one_call"], res["two_call"])):
            raise SystemExit(f"time_pbm: the one-call and two-call encodes differ ({layout})")
        stream_bytes = 8 * (int(pybic.as_u64(fg)[-1]) + int(pybic.as_u64(fe)[-1]))
        del res
        p00 = torch.stack([imgs[0][k * stride] >> 7 for k in range(n)]).contiguous()

        def dec_one(img):
            ctx.decode_pbm(G, og, bg, n, rows, cols, True, word_off=fg, row_index=idx, p00=p00, out=back,
                           frame_stride=stride)

        def dec_two(img):
            ctx.decode_planes(G, og, bg, n, rows, cols, True, word_off=fg, row_index=idx, p00=p00, out=planes)
            for k in range(n):
                ctx.lib.bic_pbm_pack(ctx.h, planes[k].data_ptr(), rows, cols, wpr, back.data_ptr() + k * stride)

        # the two decodes, byte for byte, and against the input's rasters (the streams are imgs[0]'s). A frame
        # both decodes get wrong alike is the row decoders' (shared by the two variants): it is reported in
        # the summary lines, not hidden, and does not stop the timing
        dec = {}
        for name, fn in (("one_call", dec_one), ("two_call", dec_two)):
            back.zero_()
            fn(None)
            ctx.sync()
            dec[name] = back.clone()
        if not torch.equal(dec["one_call"], dec["two_call"]):
            raise SystemExit(f"time_pbm: the one-call and two-call decodes differ ({layout})")
        wrong = [k for k in range(n)
                 if not torch.equal(dec["one_call"][k * stride:k * stride + fb], imgs[0][k * stride:k * stride + fb])]
        del dec

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

        def kernel_ms(fn, only=None):
            """the step's kernels alone: every launch (or those named `only`) bracketed, per step"""
            ctx.sync()
            ctx.prof_collect()
            ctx.prof_enable(True)
            ctx.prof_only(only)
            for i in range(args.steps):
                fn(imgs[i & 1])
            prof = ctx.prof_collect()
            ctx.prof_only(None)
            ctx.prof_enable(False)
            # (the "<name>_stage" records repeat their kernels' time)
            return sum(v[1] for k, v in prof.items() if not k.endswith("_stage")) / args.steps, prof

        for direction, one, two in (("encode", enc_one, enc_two), ("decode", dec_one, dec_two)):
            ms = {"one_call": [], "two_call": []}
            for r in range(args.repeats):
                for name, fn in (("one_call", one), ("two_call", two)):
                    t = timed(fn)
                    ms[name].append(t)
                    emit({"tool": "time_pbm", "config": config, "layout": layout, "direction": direction, "repeat": r,
                          "variant": name, "steps": args.steps, "ms_per_step": round(t, 4), "results_equal": True})
            k1, prof1 = kernel_ms(one)
            k2, _ = kernel_ms(two)
            summary = {"tool": "time_pbm", "config": config, "layout": layout, "direction": direction, "summary": True,
                       "one_call_ms": [round(x, 4) for x in ms["one_call"]],
                       "two_call_ms": [round(x, 4) for x in ms["two_call"]],
                       "one_call_slowest_ms": round(max(ms["one_call"]), 4),
                       "two_call_fastest_ms": round(min(ms["two_call"]), 4),
                       "criterion_met": bool(max(ms["one_call"]) < min(ms["two_call"])),
                       "one_call_kernel_ms": round(k1, 4), "two_call_kernel_ms": round(k2, 4),
                       "one_call_kernels_us": {k: round(v[1] * 1e3 / args.steps, 1) for k, v in sorted(prof1.items())},
                       "raster_bytes": n * fb, "stream_bytes": stream_bytes,
                       "decoded_frames_differing_from_input": wrong}
            if direction == "encode":
                _, cp = kernel_ms(one, "bitplanes_count")
                cnt = cp.get("bitplanes_count", (0, 0.0))
                summary["count_pass_us"] = round(cnt[1] * 1e3 / max(cnt[0], 1), 1)
                summary["count_pass_launches"] = cnt[0]
            emit(summary)
        del imgs, back
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
