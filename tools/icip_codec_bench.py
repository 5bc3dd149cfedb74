#!/usr/bin/env python
"""Real-bitstream path of the ICIP2024 B-frame codec at 1088x1920 (FlowGuidedB.compress / decompress on one frame triple of the
synthetic GOP of bench.py): ms per frame of each, the container's bytes, the real size against the device's -log2 p of the coded
symbols and against forward()'s estimate, the PSNR of compress's reconstruction beside forward's, and -- for information -- how many
elements differ when image 1 of a batch-of-2 encode is decoded alone (a batch of one may take other tile configurations).
``--coder device`` measures the interleaved coder on the GPU instead and adds the time of its decode kernels
alone and of all bracketed launches of one decompress (HIP events, one pair per launch) beside that call's span and wall time; ``--coder both`` measures the two side by side
(the host coder's block first, the device coder's under "device").  Prints one JSON line.  No gate and no required speed."""
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


def measure_device(model, x1, xc, x2, args, dr):
    """compress / decompress with coder="device": the protocol of main() (one warm-up, ``reps`` timed calls)"""
    kw = {"coder": "device", "waves": args.waves}
    h, w = xc.shape[2:]
    enc = model.compress(x1, x2, 0.5, 0.5, xc, args.s, dr, **kw)
    model.decompress(x1, x2, 0.5, 0.5, enc["strings"], enc["shape"], args.s, dr, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        enc = model.compress(x1, x2, 0.5, 0.5, xc, args.s, dr, **kw)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(args.reps):
        dec = model.decompress(x1, x2, 0.5, 0.5, enc["strings"], enc["shape"], args.s, dr, **kw)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    # one more decode WITHOUT any per-launch events: its span between two stream events (which includes every interval the GPU
    # waited for the host to launch) beside its wall time ...
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    tw = time.perf_counter()
    e0.record()
    model.decompress(x1, x2, 0.5, 0.5, enc["strings"], enc["shape"], args.s, dr, **kw)
    e1.record()
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - tw)
    # ... and one under the KernelTimer: every bracketed launch between its own pair of events, i.e. the time the GPU is busy
    hip.timer = hip.KernelTimer()
    tw = time.perf_counter()
    model.decompress(x1, x2, 0.5, 0.5, enc["strings"], enc["shape"], args.s, dr, **kw)
    torch.cuda.synchronize()
    wall_bracketed = 1e3 * (time.perf_counter() - tw)
    table, hip.timer = hip.timer.table(), None
    # the upload alone (payloads into reused pinned staging, asynchronous copy, header launch), host time of the call
    torch.cuda.synchronize()
    tu = time.perf_counter()
    for _ in range(args.reps):
        decoders = model.upload_payloads(enc["strings"], enc["waves"])
    upload_host = 1e3 * (time.perf_counter() - tu) / args.reps
    torch.cuda.synchronize()
    del decoders
    c1, c2 = model.convert_scales(0.5, 0.5)
    blob = bitstream.pack_icip2024_frame_dev(enc["strings"], enc["shape"], dr, args.s, c1, c2, enc["waves"])
    payload = sum(len(b) for v in enc["strings"].values() for b in v)
    return {"waves": enc["waves"], "compress_ms": 1e3 * (t1 - t0) / args.reps, "decompress_ms": 1e3 * (t2 - t1) / args.reps,
            "container_bytes": len(blob), "size_bits": enc["size"], "bpp": enc["size"] / float(h * w),
            "format_overhead_bytes": 2 * enc["waves"] * hip.IRANS_SUBSTREAM_HEADER, "payload_bytes": payload,
            "size_over_size_estimate": enc["size"] / enc["size_estimate"],
            "decode_kernels_ms": table["irans decode"]["ms"], "decode_kernel_launches": table["irans decode"]["launches"],
            # every launch the KernelTimer brackets (convolutions, deformable fusion, memory-bound kernels, the decode kernels),
            # each timed by its own pair of events: time the GPU was busy with them, gaps between launches NOT included
            "bracketed_kernels_ms": sum(v["ms"] for v in table.values()), "bracketed_launches": sum(v["launches"] for v in table.values()),
            "decompress_wall_ms_of_the_bracketed_call": wall_bracketed,
            "decompress_span_ms_unbracketed": e0.elapsed_time(e1), "decompress_wall_ms_unbracketed": wall,
            "upload_host_ms": upload_host,
            "decoder_reproduces_encoder_bit_for_bit": bool(torch.equal(dec["x_hat"], enc["x_hat"])), "x_hat": enc["x_hat"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--s", type=float, default=2.0, help="quality level")
    ap.add_argument("--down-ratio", type=int, default=None, help="flow resolution (default: searched on the device)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hw", type=int, nargs=2, default=None, help="frame size before padding (default 1080 1920)")
    ap.add_argument("--no-batch", action="store_true", help="skip the batch-of-2 block")
    ap.add_argument("--coder", choices=("host", "device", "both"), default="host", help="range coder of the strings")
    ap.add_argument("--waves", type=int, default=4, help="sub-streams per payload of the device coder")
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
    if args.coder == "device":
        with torch.no_grad():
            dr = args.down_ratio or model.compress(x1, x2, 0.5, 0.5, xc, args.s, None, coder="device", waves=args.waves)["down_ratio"]
            block = measure_device(model, x1, xc, x2, args, dr)
        block.pop("x_hat")
        out.update(block, down_ratio=dr, coder="device")
        print(json.dumps(out))
        if not out["decoder_reproduces_encoder_bit_for_bit"]:
            raise SystemExit("decoder output differs from the encoder-side reconstruction")
        return
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
        if args.coder == "both":
            # the host-coded decompress under the same per-launch events: what its launches take without the gaps between them
            hip.timer = hip.KernelTimer()
            tw = time.perf_counter()
            model.decompress(x1, x2, 0.5, 0.5, enc["strings"], enc["shape"], args.s, dr)
            torch.cuda.synchronize()
            wall = 1e3 * (time.perf_counter() - tw)
            table, hip.timer = hip.timer.table(), None
            out.update({"bracketed_kernels_ms": sum(v["ms"] for v in table.values()),
                        "bracketed_launches": sum(v["launches"] for v in table.values()), "decompress_wall_ms_of_the_bracketed_call": wall})
            block = measure_device(model, x1, xc, x2, args, dr)
            block["x_hat_equals_host_coded"] = bool(torch.equal(block.pop("x_hat"), enc["x_hat"]))
            out["device"] = block
            if not block["decoder_reproduces_encoder_bit_for_bit"]:
                raise SystemExit("device coder: decoder output differs from the encoder-side reconstruction")
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
