#!/usr/bin/env python
"""Measure the ICIP2023 DeformB path on one GPU (the numbers of DESIGN.md section 4f).

  python tools/icip2023_bench.py [--height 1088 --width 1920 --passes 10 --warmup 3 --level 2 --precision fp32]

Prints one JSON line: ``forward`` frames/s at the frame size for the fp32 modes "split" and "native" (synchronised wall clock over
``--passes`` passes after ``--warmup``, with the spread of the per-pass times), and the three vc_deform_pair launches of a frame
under HIP events against the unfused chain they replace (torch chunk / cat / sigmoid + two vc_deform_conv2d calls per level), in
the same run on the same tensors.  Seeded weights: the times do not depend on the values, the rates do.

``--precision fp16``: ``forward`` in fp16 mode (hip.set_conv_precision) with hip.HALF_DEFORM_PAIR on and off, and under HIP events the
three half pair launches INCLUDING their six vc_to_half_planar launches beside the three fp32 vc_deform_pair launches, in the same run
on the same tensors (the numbers behind the default of VC_HALF_DEFORM_PAIR)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-compression_amd"))


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "passes": len(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--height", type=int, default=1088)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--level", type=float, default=2)
    ap.add_argument("--precision", choices=("fp32", "fp16"), default="fp32")
    args = ap.parse_args()
    from vcamd import hip, icip2023
    from vcamd.seeding import seeded_state_dict
    dev = torch.device("cuda:0")
    model = icip2023.DeformB()
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=7))
    model = model.to(dev).eval()
    g = torch.Generator().manual_seed(11)
    h, w = args.height, args.width
    base = torch.nn.functional.avg_pool2d(torch.rand(1, 3, h + 32, w + 32, generator=g), 7, 1, 3)
    fr = [(base[:, :, 2 * t:2 * t + h, 3 * t:3 * t + w] + 0.01 * torch.randn(1, 3, h, w, generator=g)).clamp(0, 1).to(dev) for t in range(3)]
    result = {"model": "icip2023", "height": h, "width": w, "level": args.level, "device": torch.cuda.get_device_name(0),
              "precision": args.precision}

    def wall(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        st = _stats(times)
        return dict(st, frames_per_s=round(1e3 / st["median_ms"], 3))

    def events(fn):
        for _ in range(args.warmup):
            fn()
        times = []
        for _ in range(args.passes):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return _stats(times)

    if args.precision == "fp16":
        from vcamd.layers import BitCounter
        keep = hip.HALF_DEFORM_PAIR
        hip.set_conv_precision("fp16")
        try:
            with torch.no_grad():
                model.float()
                for flag in (True, False):
                    hip.HALF_DEFORM_PAIR = flag
                    result["forward_fp16_pair_" + ("half" if flag else "fp32")] = wall(lambda: model(fr[0], fr[2], fr[1], args.level))
                trace = {}
                t1, t2, tc = (hip.nchw_to_nhwc(x) for x in (fr[0], fr[2], fr[1]))
                model.forward_device(t1, t2, tc, args.level, BitCounter(dev, max_rows=12), trace=trace)
                # the model's own layout: per level one buffer [fref1 | fref2 | fcur], the features its channel windows
                F_, f1, f2, _ = model._features(t1, t2, tc)
                offs = trace["offsets"]
                outs = [hip.T.empty(1, f1[l].h, f1[l].w, 2 * f1[l].c, dev) for l in range(3)]

                def pairs():
                    return [model.get_deformed_maps_t(offs[l], f1[l], f2[l], l + 1, out=outs[l]) for l in range(3)]
                got = {}
                for name, flag in (("pair_half_with_conversions", True), ("pair_fp32", False)):
                    hip.HALF_DEFORM_PAIR = flag
                    got[name] = [hip.nhwc_to_nchw(t).clone() for t in pairs()]
                    result[name] = events(pairs)
                result["pair_half_vs_fp32_max_abs_diff"] = max((a - b).abs().max().item() for a, b in zip(*got.values()))
        finally:
            hip.HALF_DEFORM_PAIR = keep
            hip.set_conv_precision("fp32")
        print(json.dumps(result))
        return
    with torch.no_grad():
        for mode in ("split", "native"):
            hip.set_fp32_mode(mode)
            model.float()                                   # drops the packed-weight caches: the mode decides how layers are packed
            for _ in range(args.warmup):
                model(fr[0], fr[2], fr[1], args.level)
            torch.cuda.synchronize()
            times = []
            for _ in range(args.passes):
                t0 = time.perf_counter()
                model(fr[0], fr[2], fr[1], args.level)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            st = _stats(times)
            result[f"forward_{mode}"] = dict(st, frames_per_s=round(1e3 / st["median_ms"], 3))
        # the alignment step alone: real features and real offset heads of one pass
        trace = {}
        from vcamd.layers import BitCounter
        t1, t2, tc = (hip.nchw_to_nhwc(x) for x in (fr[0], fr[2], fr[1]))
        model.forward_device(t1, t2, tc, args.level, BitCounter(dev, max_rows=12), trace=trace)
        f1, f2 = model.feature_extractor.run(t1), model.feature_extractor.run(t2)
        offs = trace["offsets"]

        def fused():
            return [model.get_deformed_maps_t(offs[l], f1[l], f2[l], l + 1) for l in range(3)]

        def unfused():
            outs = []
            for l in range(3):
                off = hip.nhwc_to_nchw(offs[l])
                halves = []
                for r, (o, f) in enumerate(zip(torch.chunk(off, 2, dim=1), (f1[l], f2[l]))):
                    ox, oy, m = torch.chunk(o, 3, dim=1)
                    layer = getattr(model, f"deconv_l{l + 1}_{r + 1}").packed()
                    halves.append(hip.nhwc_to_nchw(layer.conv(f, hip.nchw_to_nhwc(torch.cat((ox, oy), 1)), hip.nchw_to_nhwc(torch.sigmoid(m)))))
                outs.append(torch.cat(halves, 1))
            return outs
        a, b = fused(), unfused()
        result["pair_vs_unfused_max_abs_diff"] = max((hip.nhwc_to_nchw(x) - y).abs().max().item() for x, y in zip(a, b))
        for name, fn in (("pair_fused", fused), ("pair_unfused_chain", unfused)):
            for _ in range(args.warmup):
                fn()
            times = []
            for _ in range(args.passes):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            result[name] = _stats(times)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
