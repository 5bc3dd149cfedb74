#!/usr/bin/env python
"""MS-SSIM of one 1080p frame (1x3x1080x1920 crop of a 1088x1920 frame): the HIP call (vc_msssim, six launches) against the same
definition written with torch operators on the device in fp32 (depthwise F.conv2d + F.avg_pool2d, ~130 launches).  Both are timed
with HIP events after a warm-up, per call, and reported as the median of ``--reps`` (>= 20) calls; the mean of the same calls issued
back to back is printed beside it.  Prints one JSON line.

    python tools/msssim_bench.py [--reps R] [--b_frame_ms MS]

``--b_frame_ms``: time of one B-frame of the headline run on the same box (1000 / frames-per-second of bench.py): the metric's cost
is then also printed relative to it.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-compression_amd"))
from vcamd import hip  # noqa: E402

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def torch_msssim(a, b, h, w):
    """the definition of csrc/metrics.hip with torch operators, in the tensors' dtype"""
    X = torch.round(a[..., :h, :w].clamp(0.0, 1.0) * 255.0)
    Y = torch.round(b[..., :h, :w].clamp(0.0, 1.0) * 255.0)
    c = X.shape[1]
    g = torch.exp(-(torch.arange(11, dtype=X.dtype, device=X.device) - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    g = g / g.sum()
    wr, wc = g.view(1, 1, 1, 11).repeat(c, 1, 1, 1), g.view(1, 1, 11, 1).repeat(c, 1, 1, 1)
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2

    def filt(t):
        return F.conv2d(F.conv2d(t, wr, groups=c), wc, groups=c)
    terms = []
    for s in range(5):
        mu1, mu2 = filt(X), filt(Y)
        s1, s2, s12 = filt(X * X) - mu1 * mu1, filt(Y * Y) - mu2 * mu2, filt(X * Y) - mu1 * mu2
        m = (2.0 * s12 + c2) / (s1 + s2 + c2)
        if s == 4:
            m = (2.0 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * m
        terms.append(torch.relu(m.mean((2, 3))))
        if s < 4:
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
    terms = torch.stack(terms, 1)
    return torch.prod(terms ** torch.tensor(WEIGHTS, dtype=X.dtype, device=X.device).view(1, 5, 1), 1).mean(1)


def time_calls(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in events:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    per_call = [e0.elapsed_time(e1) for e0, e1 in events]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return statistics.median(per_call), min(per_call), max(per_call), e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--b_frame_ms", type=float, default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if not torch.cuda.is_available():
        raise hip.VcError("msssim_bench measures on the device: no CUDA/ROCm device is visible")
    dev = torch.device("cuda:0")
    n, c, H, W, h, w = 1, 3, 1088, 1920, 1080, 1920
    g = torch.Generator().manual_seed(0)
    coarse = torch.rand(n, c, H // 16 + 2, W // 16 + 2, generator=g)
    x = (0.15 + 0.7 * F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False)).clamp(0.02, 0.98)
    y = x + 0.02 * torch.randn(n, c, H, W, generator=g)
    x, y = x.contiguous().to(dev), y.contiguous().to(dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    with torch.no_grad():
        hip_ms = time_calls(lambda: hip.msssim_uint8(y, x, h, w, out=out), args.reps)
        torch_ms = time_calls(lambda: torch_msssim(y, x, h, w), args.reps)
        v_hip, v_torch = hip.msssim_uint8(y, x, h, w).item(), torch_msssim(y, x, h, w).item()
    nbytes = 8.0 * n * c * h * w                       # both crops read once
    res = {"shape": [n, c, h, w], "frame": [H, W], "reps": args.reps,
           "hip_ms_median": hip_ms[0], "hip_ms_min": hip_ms[1], "hip_ms_max": hip_ms[2], "hip_ms_back_to_back": hip_ms[3],
           "torch_fp32_ms_median": torch_ms[0], "torch_fp32_ms_min": torch_ms[1], "torch_fp32_ms_max": torch_ms[2],
           "torch_fp32_ms_back_to_back": torch_ms[3],
           "speedup_median": torch_ms[0] / hip_ms[0],
           "algorithmic_bytes": nbytes, "hip_GBps_algorithmic": nbytes / (hip_ms[0] * 1e-3) / 1e9,
           "msssim_hip": v_hip, "msssim_torch_fp32": v_torch}
    if args.b_frame_ms:
        res["b_frame_ms"] = args.b_frame_ms
        res["share_of_b_frame"] = hip_ms[0] / args.b_frame_ms
    print(json.dumps(res))


if __name__ == "__main__":
    main()
