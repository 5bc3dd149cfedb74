#!/usr/bin/env python
"""Measure the ICIP2023 DeformB path on one GPU (the numbers of DESIGN.md section 4f).

  python tools/icip2023_bench.py [--height 1088 --width 1920 --passes 10 --warmup 3 --level 2]

Prints one JSON line: ``forward`` frames/s at the frame size for the fp32 modes "split" and "native" (synchronised wall clock over
``--passes`` passes after ``--warmup``, with the spread of the per-pass times), and the three vc_deform_pair launches of a frame
under HIP events against the unfused chain they replace (torch chunk / cat / sigmoid + two vc_deform_conv2d calls per level), in
the same run on the same tensors.  Seeded weights: the times do not depend on the values, the rates do."""
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
    result = {"model": "icip2023", "height": h, "width": w, "level": args.level, "device": torch.cuda.get_device_name(0)}
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
