#!/usr/bin/env python
"""The device-coded ICIP2024 paths at 1088x1920, seeded weights, one GPU.  Two measurements:

  (a) ELIC I-frame compress / decompress: coder="host" (the numpy / one-host-thread path, the yardstick) against coder="device";
  (b) one FlowGuidedB.decompress(coder="device") on the three-launch chain vc_gc_indexes_ckbd -> vc_irans_decode -> vc_gc_dequant_ckbd
      per pass (the product's code; the yardstick) against the fused checkerboard decode (vc_irans_decode_gc_ckbd, one launch per
      pass: ``reader=icip2024.DeviceFusedReader`` handed to the same call).  The payloads are uploaded outside the timed span.
      The ELIC device decode is measured the other way round too: its own fused reader against ``DeviceChainReader``.

Every figure is the median over ``--reps`` runs after ``--warmup`` untimed ones, each run between two HIP events on the stream
(the host-coded ELIC calls synchronise inside, so their span contains the host's coding time, as a caller sees it).  Prints one
JSON line.  No gate and no required speed."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-compression_amd"))
from bench import synthetic_gop  # noqa: E402
from vcamd import icip2024  # noqa: E402
from vcamd.seeding import seeded_state_dict  # noqa: E402


def median_ms(fn, warmup, reps, setup=None):
    """median of ``reps`` event-timed runs of fn(setup()) after ``warmup`` untimed ones; (median, min, max)"""
    times = []
    for k in range(warmup + reps):
        arg = setup() if setup else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn(arg)
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": reps}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--s", type=float, default=2.0, help="quality level of the B-frame")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--waves", type=int, default=4)
    ap.add_argument("--hw", type=int, nargs=2, default=None, help="frame size before padding (default 1080 1920)")
    ap.add_argument("--skip-intra", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    frames = synthetic_gop(1234, 0, dev, hw=tuple(args.hw) if args.hw else None)
    x1, xc, x2 = frames[0], frames[4], frames[8]
    out = {"frame": [int(v) for v in xc.shape[2:]], "waves": args.waves, "warmup": args.warmup, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        # (b) B-frame decode: fused kernel against the chain, same uploaded payloads
        model = icip2024.FlowGuidedB()
        model.load_state_dict(seeded_state_dict(model.state_dict(), seed=1234))
        model = model.to(dev).eval()
        model.offset_compressor.update(force=True)
        model.residual_compressor.update(force=True)
        enc = model.compress(x1, x2, 0.5, 0.5, xc, args.s, None, coder="device", waves=args.waves)
        dr = enc["down_ratio"]

        def upload():
            return model.upload_payloads(enc["strings"], args.waves)

        def decode(decoders, reader=None):
            decode.x_hat = model.decompress(x1, x2, 0.5, 0.5, decoders, enc["shape"], args.s, dr, coder="device", waves=args.waves,
                                            reader=reader)["x_hat"]
        chain = median_ms(decode, args.warmup, args.reps, upload)
        same = bool(torch.equal(decode.x_hat, enc["x_hat"]))
        fused = median_ms(lambda d: decode(d, icip2024.DeviceFusedReader), args.warmup, args.reps, upload)
        same = same and bool(torch.equal(decode.x_hat, enc["x_hat"]))
        out["b_frame_decompress"] = {"down_ratio": dr, "fused": fused, "chain": chain, "bit_identical": same}
        del model
        if not args.skip_intra:
            # (a) ELIC I-frame: host coder against device coder
            intra = icip2024.ELIC()
            intra.load_state_dict(seeded_state_dict(intra.state_dict(), seed=4321, conv_gain=0.8))
            intra = intra.to(dev).eval()
            intra.update(force=True)
            res = {}
            for coder in ("host", "device"):
                kw = {"coder": coder, "waves": args.waves}
                coded = {}

                def compress(_):
                    coded["enc"] = intra.compress(xc, **kw)
                res[coder] = {"compress": median_ms(compress, args.warmup, args.reps)}
                e = coded["enc"]

                def decompress(_, reader=None):
                    coded["dec"] = intra.decompress(e["strings"], e["shape"], reader=reader, **kw)
                res[coder]["decompress"] = median_ms(decompress, args.warmup, args.reps)
                if coder == "device":          # the same decode with the chain in place of the fused kernel
                    fused_y = coded["dec"]["y_hat"]
                    res[coder]["decompress_on_the_chain"] = median_ms(lambda _: decompress(_, icip2024.DeviceChainReader), args.warmup, args.reps)
                    res[coder]["chain_bit_identical"] = all(bool(torch.equal(a, b)) for a, b in zip(fused_y, coded["dec"]["y_hat"]))
                strings = e["strings"] if coder == "device" else icip2024._flat_strings(e["strings"])
                res[coder]["bytes"] = sum(len(b) for b in strings)
                res[coder]["y_hat_round_trip"] = all(bool(torch.equal(a, b)) for a, b in zip(e["y_hat"], coded["dec"]["y_hat"]))
            out["elic_i_frame"] = res
    print(json.dumps(out))
    if not out["b_frame_decompress"]["bit_identical"]:
        raise SystemExit("a decoder's output differs from the encoder-side reconstruction")


if __name__ == "__main__":
    main()
