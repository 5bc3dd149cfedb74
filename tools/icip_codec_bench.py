#!/usr/bin/env python
"""Real-bitstream path of the ICIP2024 B-frame codec at 1088x1920 (FlowGuidedB.compress / decompress on one frame triple of the
synthetic GOP of bench.py): ms per frame of each, the container's bytes, the real size against the device's -log2 p of the coded
symbols and against forward()'s estimate, the PSNR of compress's reconstruction beside forward's, and -- for information -- how many
elements differ when image 1 of a batch-of-2 encode is decoded alone (a batch of one may take other tile configurations).  Prints
one JSON line.  No gate and no required speed."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-compression_amd"))
from bench import synthetic_gop  # noqa: E402
from vcamd import bitstream, hip, icip2024  # noqa: E402
from vcamd.seeding import seeded_state_dict  # noqa: E402


def _psnr(a, b):
    return float(10.0 * torch.log10(1.0 / ((a.double().clamp(0, 1) - b.double()) ** 2).mean()).item())


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--s", type=float, default=2.0, help="quality level")
    ap.add_argument("--down-ratio", type=int, default=None, help="flow resolution (default: searched on the device)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hw", type=int, nargs=2, default=None, help="frame size before padding (default 1080 1920)")
    ap.add_argument("--no-batch", action="store_true", help="skip the batch-of-2 block")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = icip2024.FlowGuidedB()
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=1234))
    model = model.to(dev).eval()
    model.offset_compressor.update(force=True)
    model.residual_compressor.update(force=True)
    frames = synthetic_gop(1234, 0, dev, hw=tuple(args.hw) if args.hw else None)
    x1, xc, x2 = frames[0], frames[4], frames[8]
    h, w = xc.shape[2:]
    out = {"frame": [int(h), int(w)], "s": args.s, "fp32_mode_of_the_coded_pass": hip.BITSTREAM_HS_MODE}
    with torch.no_grad():
        enc = model.compress(x1, x2, 0.5, 0.5, xc, args.s, args.down_ratio)            # warm-up: packs weights, tunes tile configurations
        dr = enc["down_ratio"]
        model.decompress(x1, x2, 0.5, 0.5, enc["strings"], enc["shape"], args.s, dr)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            enc = model.compress(x1, x2, 0.5, 0.5, xc, args.s, args.down_ratio)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.reps):
            dec = model.decompress(x1, x2, 0.5, 0.5, enc["strings"], enc["shape"], args.s, dr)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        fwd = model(x1, x2, 0.5, 0.5, xc, args.s, dr)
        c1, c2 = model.convert_scales(0.5, 0.5)
        blob = bitstream.pack_icip2024_frame(enc["strings"], enc["shape"], dr, args.s, c1, c2)
        out.update({"compress_ms": 1e3 * (t1 - t0) / args.reps, "decompress_ms": 1e3 * (t2 - t1) / args.reps, "down_ratio": dr,
                    "searched": args.down_ratio is None, "container_bytes": len(blob), "size_bits": enc["size"],
                    "bpp": enc["size"] / float(h * w), "size_over_size_estimate": enc["size"] / enc["size_estimate"],
                    "size_over_forward_size": enc["size"] / fwd["size"].item(),
                    "psnr_compress": _psnr(enc["x_hat"], xc), "psnr_forward": _psnr(fwd["x_hat"], xc),
                    "decoder_reproduces_encoder_bit_for_bit": bool(torch.equal(dec["x_hat"], enc["x_hat"]))})
        if not args.no_batch:
            xb1, xbc, xb2 = torch.cat([frames[0], frames[2]]), torch.cat([frames[4], frames[3]]), torch.cat([frames[8], frames[4]])
            enc2 = model.compress(xb1, xb2, 0.5, 0.5, xbc, args.s, dr)
            one = {c: [[[g[1]] for g in enc2["strings"][c][0]], [enc2["strings"][c][1][1]]] for c in enc2["strings"]}
            try:
                alone = model.decompress(xb1[1:2], xb2[1:2], 0.5, 0.5, one, enc2["shape"], args.s, dr)
                out["batch_image_decoded_alone_differing_elements"] = int((alone["x_hat"] != enc2["x_hat"][1:2]).sum().item())
            except hip.VcError as e:          # a desynchronised range decoder refuses the string
                out["batch_image_decoded_alone_differing_elements"] = f"not decodable alone: {e}"
    print(json.dumps(out))
    if not out["decoder_reproduces_encoder_bit_for_bit"]:
        raise SystemExit("decoder output differs from the encoder-side reconstruction")


if __name__ == "__main__":
    main()
