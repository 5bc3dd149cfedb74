#!/usr/bin/env python
"""The LHBDC sequence codec at 1088x1920, seeded weights, one GPU.  Three measurements:

  (a) encode and decode frames/s of a 17-frame sequence (two GOPs, three I-frames) through sequence.LhbdcSequenceCodec, the frames
      already on the device; wall clock around the whole call, the device synchronised in front and behind;
  (b) the same decode with ``verify=True`` against ``verify=False`` -- the SAME build and file: what recomputing the picture hashes
      costs a decoder;
  (c) the hash kernel alone (hip.picture_hash between two HIP events): one decoded frame (25 MB, cache-resident between runs) and a
      batch of frames of about 1 GB (streamed from HBM), in GB/s of words read -- beside the copy and read figures of
      tools/micro/stream_rate.hip where ``--stream_rate PATH`` names its binary (run first, as a child process of its own).

Every figure is the median over ``--reps`` runs after ``--warmup`` untimed ones.  Prints one JSON line.  No gate and no required
speed."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-compression_amd"))
from bench import synthetic_gop  # noqa: E402
from vcamd import hip, sequence  # noqa: E402


def stream_rate_figures(path):
    """best copy / read GB/s per buffer size out of stream_rate's own lines"""
    text = subprocess.run([path], check=True, capture_output=True, text=True, timeout=300).stdout
    best, size = {}, None
    for line in text.splitlines():
        m = re.match(r"== X = (\d+) MB ==", line)
        if m:
            size = f"{m.group(1)} MB"
            continue
        m = re.match(r"(copy|read) .*?(\d+) GB/s\s*$", line)
        if m and size:
            key = best.setdefault(size, {})
            key[m.group(1)] = max(key.get(m.group(1), 0), int(m.group(2)))
    return best


def wall_ms(fn, warmup, reps):
    times = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": reps}


def event_ms(fn, warmup, reps):
    times = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": reps}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--waves", type=int, default=4)
    ap.add_argument("--hw", type=int, nargs=2, default=None, help="frame size before padding (default 1080 1920)")
    ap.add_argument("--stream_rate", default=None, help="binary built from tools/micro/stream_rate.hip, for the copy figure")
    args = ap.parse_args()
    out = {"frames": args.frames, "waves": args.waves, "warmup": args.warmup, "reps": args.reps}
    if args.stream_rate:
        out["stream_rate_best_gbps"] = stream_rate_figures(args.stream_rate)
    dev = torch.device("cuda:0")
    out["device"] = torch.cuda.get_device_name(0)
    hw = tuple(args.hw) if args.hw else (1080, 1920)
    frames = []
    for g in range(max(1, (args.frames + 6) // 8)):                            # GOP g holds frames 8g .. 8g + 8; its first is the last one's last
        frames.extend(synthetic_gop(1234, g, dev, hw=hw)[1 if g else 0:])
    frames = frames[:args.frames]
    out["frame"] = [int(v) for v in frames[0].shape[2:]]
    model, intra = sequence.load_lhbdc_models(seeded=1234, device=dev)
    codec = sequence.LhbdcSequenceCodec(model, intra, waves=args.waves)
    state = {}

    def encode():
        state["data"], state["recon"] = codec.encode(lambda i: frames[i], args.frames, *hw)

    def decode(verify):
        state["frames"] = codec.decode(state["data"], verify=verify)

    with torch.no_grad():
        enc = wall_ms(encode, args.warmup, args.reps)
        on = wall_ms(lambda: decode(True), args.warmup, args.reps)
        verified = codec.report["verified"]
        same = all(bool(torch.equal(state["frames"][o], state["recon"][o])) for o in range(args.frames))
        off = wall_ms(lambda: decode(False), args.warmup, args.reps)
        on2 = wall_ms(lambda: decode(True), args.warmup, args.reps)      # (once more behind the other arm: the order of the arms)
    fps = lambda r: args.frames / (r["median_ms"] / 1e3)                # noqa: E731
    out["file_bytes"] = len(state["data"])
    out["encode"] = {**enc, "frames_per_s": fps(enc)}
    out["decode_verify_on"] = {**on, "frames_per_s": fps(on)}
    out["decode_verify_off"] = {**off, "frames_per_s": fps(off)}
    out["decode_verify_on_again"] = {**on2, "frames_per_s": fps(on2)}
    out["verified"], out["bit_identical"] = verified, same
    # (c) the kernel alone
    one = state["recon"][0]
    n = max(2, (1 << 30) // (4 * one[0].numel()))
    many = torch.rand((n,) + tuple(one.shape[1:]), device=dev)
    sink1, sinkn = torch.empty(1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    for name, x, sink in (("one_frame", one, sink1), ("batch", many, sinkn)):
        r = event_ms(lambda: hip.picture_hash(x, out=sink), 3, 20)
        nbytes = 4 * x.numel()
        out[f"hash_{name}"] = {**r, "images": int(x.shape[0]), "bytes": nbytes, "gbps": nbytes / (r["median_ms"] * 1e-3) / 1e9}
    print(json.dumps(out))
    if not (same and verified):
        raise SystemExit("the decoder's output differs from the encoder-side reconstruction")


if __name__ == "__main__":
    main()
