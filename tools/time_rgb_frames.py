"""A/B timing of the RGB-frame calls (measurement for DESIGN.md §3, not a test): 64 frames of 1024 rows x 1408
pixels of three one-byte samples (264 MiB, within 3 % of configs[2]'s input bytes; 22 plane words per row, an even
row pitch; uniform bytes, device-resident), packed Golomb + EG streams with the row index, in two layouts --

  files      64 concatenated P6 files (header "P6\\n1408 1024\\n255\\n": an odd stride, the frames misaligned)
  aligned    the frames alone, back to back from a 16-byte aligned base

and per layout --

  encode  one_call    bic_encode_rgb_frames_packed, planes NULL
          two_call    64 x bic_bitplanes_rgb into one buffer, then bic_encode_planes_packed
          per_frame   64 x bic_encode_rgb_packed (planes NULL) into per-frame buffers
  decode  one_call    bic_decode_rgb_frames                    } from the Golomb streams with the row index,
          two_call    bic_decode_planes, 64 x bic_planes_to_rgb } and from the EG streams

With --check the variants' results are first compared (bit counts, offsets, packed words and row index word for
word; per_frame frame by frame against the one call's words; the decoded frames byte for byte with one another
and with the input; the run stops at a difference). Then the variants alternate in ONE process, `--repeats`
times, each repeat `--steps` calls between device syncs after a warm-up, on two input buffers used in turn so
that the Infinity Cache cannot serve a re-run. One JSON line per (size, layout, direction, repeat, variant), then
per (size, layout, direction) a summary line. The criterion (judged at the first size only): the slowest
one_call repeat below the fastest repeat of every other variant. The encode summary also has the count
kernel's own time (bracketed launches) and its bytes (the samples read, the residual planes written) over that
time against the 8 TB/s peak. --color-transform M and --gray-code set BIC_OPT_COLOR_TRANSFORM / BIC_OPT_GRAY_CODE
for every call of the run.
Needs a device; fails without one.
Usage: python tools/time_rgb_frames.py [--check] [--color-transform M] [--gray-code] [--steps 20] [--repeats 5]
       [--out profiles/r23/time_rgb_frames.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binary-image-compression_amd"))

PEAK_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--color-transform", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--gray-code", action="store_true")
    ap.add_argument("--sizes", default="64x1024x1408", help="frames x rows x cols (pixels), the first one judged")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "time_rgb_frames.jsonl"))
    args = ap.parse_args()
    import torch
    import pybic
    ctx = pybic.Context(0)  # raises without a device
    ctx.set_color_transform(args.color_transform)
    ctx.set_gray_code(args.gray_code)
    lib, h = ctx.lib, ctx.h
    G, E = pybic.CODER_GOLOMB, pybic.CODER_EG

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    stream = torch.cuda.current_stream()
    gen = torch.Generator(device=ctx.dev)
    gen.manual_seed(0x6F21)

    for si, size in enumerate(args.sizes.split(",")):
        n, rows, cols = (int(x) for x in size.split("x"))
        judged = si == 0
        assert not judged or (args.steps >= 20 and args.repeats >= 5) or rows < 1024, "at least 5 x 20 steps at full size"
        wpr, pitch, fb, np8 = (cols + 63) // 64, 3 * cols, rows * cols * 3, n * 24
        assert wpr % 2 == 0 and cols % 64 == 0, "the one-read count pass needs an even row pitch and whole words"
        header = f"P6\n{cols} {rows}\n255\n".encode()
        planes = ctx.empty_i64(np8, rows, wpr)
        idx = ctx.empty_i64(np8 * rows * 2)
        (og, sg, bg, fg), (oe, se, be, fe) = ctx._packed_bufs(np8, rows, cols, True, True, (None, None), (None, None),
                                                              (None, None), (None, None))
        outs, bits, offs = (og, oe), (bg, be), (fg, fe)
        # per_frame: each frame's own packed buffers, offset tables and index
        pg, pe = ctx.empty_i64(n, 24 * sg), ctx.empty_i64(n, 24 * se)
        pbg, pbe, pfg, pfe = ctx.empty_i64(n, 24), ctx.empty_i64(n, 24), ctx.empty_i64(n, 25), ctx.empty_i64(n, 25)
        pidx = ctx.empty_i64(n, 24 * rows * 2)

        for layout in ("files", "aligned"):
            lead = len(header) if layout == "files" else 0
            stride = lead + fb
            total = n * stride
            imgs = []
            for _ in range(2):
                b = torch.randint(0, 256, (total + 256,), dtype=torch.uint8, device=ctx.dev, generator=gen)
                if lead:
                    hdr = torch.tensor(list(header), dtype=torch.uint8, device=ctx.dev)
                    for k in range(n):
                        b[k * stride:k * stride + lead] = hdr
                assert b.data_ptr() % 16 == 0
                imgs.append(b[lead:])  # frame 0's first sample
            back = torch.zeros(total + 256, dtype=torch.uint8, device=ctx.dev)[lead:]
            config = (f"{n} frames {rows}x{cols} RGB u8, uniform, layout {layout} (stride {stride}), color transform "
                      f"{args.color_transform}, gray code {int(args.gray_code)}, packed Golomb + EG + row index")

            def enc_one(img):
                ctx.encode_rgb_frames_packed(img, rows, cols, nframes=n, frame_stride=stride, planes=None, outs=outs,
                                             bits=bits, offs=offs, row_index=idx)

            def enc_two(img):
                for k in range(n):
                    rc = lib.bic_bitplanes_rgb(h, img.data_ptr() + k * stride, pitch, rows, cols, 0, 8,
                                               planes[24 * k].data_ptr(), wpr)
                    assert rc == 0, rc
                ctx.encode_planes_packed(planes, cols, True, golomb=True, eg=True, outs=outs, bits=bits, offs=offs,
                                         row_index=idx)

            def enc_per(img):
                for k in range(n):
                    rc = lib.bic_encode_rgb_packed(h, img.data_ptr() + k * stride, pitch, rows, cols, 0, 8, None, wpr, 1,
                                                   pg[k].data_ptr(), sg, pbg[k].data_ptr(), pfg[k].data_ptr(),
                                                   pe[k].data_ptr(), se, pbe[k].data_ptr(), pfe[k].data_ptr(),
                                                   pidx[k].data_ptr())
                    assert rc == 0, rc

            ctx._bind_stream()
            checked = False
            if args.check:
                res = {}
                for name, fn in (("one_call", enc_one), ("two_call", enc_two)):
                    for t in (og, oe, idx):
                        t.zero_()
                    fn(imgs[0])
                    ctx.sync()
                    tg, te = int(pybic.as_u64(fg)[-1]), int(pybic.as_u64(fe)[-1])
                    res[name] = [x.clone() for x in (bg, be, fg, fe, idx, og.reshape(-1)[:tg], oe.reshape(-1)[:te])]
                if not all(torch.equal(x, y) for x, y in zip(res["one_call"], res["two_call"])):
                    raise SystemExit(f"time_rgb_frames: the one-call and two-call encodes differ ({size}, {layout})")
                enc_per(imgs[0])
                ctx.sync()
                b1, e1, f1, fe1, i1, w1, we1 = res["one_call"]
                for k in range(n):
                    for ob, of, ow, fb_, ff, fw in ((b1, f1, w1, pbg, pfg, pg), (e1, fe1, we1, pbe, pfe, pe)):
                        lo, hi = int(of[24 * k]), int(of[24 * k + 24])
                        same = (torch.equal(ob[24 * k:24 * k + 24], fb_[k]) and torch.equal(of[24 * k:24 * k + 25] - lo, ff[k])
                                and torch.equal(ow[lo:hi], fw[k][:hi - lo]))
                        if not same:
                            raise SystemExit(f"time_rgb_frames: frame {k} differs from its own call ({size}, {layout})")
                    if not torch.equal(i1[k * 48 * rows:(k + 1) * 48 * rows], pidx[k]):
                        raise SystemExit(f"time_rgb_frames: frame {k}'s row index differs ({size}, {layout})")
                del res, b1, e1, f1, fe1, i1, w1, we1
            enc_one(imgs[0])  # the streams the decoders read: imgs[0]'s
            ctx.sync()
            stream_bytes = 8 * (int(pybic.as_u64(fg)[-1]) + int(pybic.as_u64(fe)[-1]))
            first = [imgs[0][k * stride:k * stride + 3].cpu().tolist() for k in range(n)]
            p00 = torch.from_numpy(pybic.rgb_frames_p00(args.color_transform, int(args.gray_code), first)).to(ctx.dev)

            def dec_one(coder):
                def fn(img):
                    ctx.decode_rgb_frames(coder, outs[coder == E], bits[coder == E], n, 8, rows, cols, True,
                                          word_off=offs[coder == E], row_index=idx if coder == G else None, p00=p00,
                                          out=back, pitch=pitch, frame_stride=stride)
                return fn

            def dec_two(coder):
                def fn(img):
                    ctx.decode_planes(coder, outs[coder == E], bits[coder == E], np8, rows, cols, True,
                                      word_off=offs[coder == E], row_index=idx if coder == G else None, p00=p00,
                                      out=planes)
                    for k in range(n):
                        rc = lib.bic_planes_to_rgb(h, planes[24 * k].data_ptr(), 0, 8, rows, cols, wpr,
                                                   back.data_ptr() + k * stride, pitch)
                        assert rc == 0, rc
                return fn

            if args.check:
                for coder in (G, E):
                    dec = {}
                    for name, fn in (("one_call", dec_one(coder)), ("two_call", dec_two(coder))):
                        back.zero_()
                        fn(None)
                        ctx.sync()
                        dec[name] = back.clone()
                    if not torch.equal(dec["one_call"], dec["two_call"]):
                        raise SystemExit(f"time_rgb_frames: the decodes differ (coder {coder}, {size}, {layout})")
                    for k in range(n):
                        if not torch.equal(dec["one_call"][k * stride:k * stride + fb], imgs[0][k * stride:k * stride + fb]):
                            raise SystemExit(f"time_rgb_frames: decoded frame {k} differs from the input (coder {coder})")
                    del dec
                checked = True

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
                return sum(v[1] for k, v in prof.items() if not k.endswith("_stage")) / args.steps, prof

            cases = [("encode", (("one_call", enc_one), ("two_call", enc_two), ("per_frame", enc_per))),
                     ("decode_golomb", (("one_call", dec_one(G)), ("two_call", dec_two(G)))),
                     ("decode_eg", (("one_call", dec_one(E)), ("two_call", dec_two(E))))]
            for direction, variants in cases:
                ms = {name: [] for name, _ in variants}
                for r in range(args.repeats):
                    for name, fn in variants:
                        t = timed(fn)
                        ms[name].append(t)
                        emit({"tool": "time_rgb_frames", "config": config, "size": size, "layout": layout,
                              "direction": direction, "repeat": r, "variant": name, "steps": args.steps,
                              "ms_per_step": round(t, 4), "checked": checked})
                others = [name for name, _ in variants if name != "one_call"]
                summary = {"tool": "time_rgb_frames", "config": config, "size": size, "layout": layout,
                           "direction": direction, "summary": True, "judged": judged, "checked": checked,
                           "one_call_slowest_ms": round(max(ms["one_call"]), 4),
                           "criterion_met": bool(all(max(ms["one_call"]) < min(ms[o]) for o in others)),
                           "sample_bytes_total": n * fb, "stream_bytes": stream_bytes}
                for name in ms:
                    summary[name + "_ms"] = [round(x, 4) for x in ms[name]]
                for o in others:
                    summary[o + "_fastest_ms"] = round(min(ms[o]), 4)
                k1, prof1 = kernel_ms(variants[0][1])
                summary["one_call_kernel_ms"] = round(k1, 4)
                summary["one_call_kernels_us"] = {k: round(v[1] * 1e3 / args.steps, 1) for k, v in sorted(prof1.items())}
                if direction == "encode":
                    _, cp = kernel_ms(enc_one, "rgb_frames_count")
                    cnt = cp.get("rgb_frames_count", (0, 0.0))
                    us = cnt[1] * 1e3 / max(cnt[0], 1)
                    moved = 2 * n * fb  # the samples read, the residual planes written (the records beside them)
                    summary["count_pass_us"] = round(us, 1)
                    summary["count_pass_launches_per_step"] = cnt[0] / args.steps
                    summary["count_pass_bytes"] = moved
                    summary["count_pass_tb_per_s"] = round(moved / (us * 1e-6) / 1e12, 3) if us else None
                    summary["count_pass_fraction_of_peak"] = round(moved / (us * 1e-6) / 1e12 / PEAK_TBS, 3) if us else None
                emit(summary)
            del imgs, back
        del planes, idx, og, oe, pg, pe, outs
    out.close()
    ctx.close()


if __name__ == "__main__":
    main()
