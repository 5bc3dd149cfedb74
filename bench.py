#!/usr/bin/env python
"""bench.py -- B-frame throughput of the LHBDC hot path on MI355X (BASELINE.json configs[1]).

One "step" = one pass of the hot path over one batch of synthetic 1080p video (SURVEY.md 8(d) Config 2): the 7 B-frames
of each GOP-8 coded in hierarchical order through Model.forward (flow -> warp -> mask/blend -> residual analysis ->
hyperprior -> likelihood/bit count -> synthesis), inputs resident in HBM, seeded random weights of the reference
architecture (pretrained weights and UVG are not available offline).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--scaling weak|strong] [--model ...] [--precision ...]
                    [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the line (`metric`, `value`, `unit`, `ms_per_step`, `quality`, ...).
--full adds everything else the line can carry: the `strong` block of the default LHBDC 1080p line, and at N = 1 the roofline /
kernel-table block, the native-fp32 comparison, the whole-GOP and bitstream rates, the CPU baseline and the parity against the
CPU oracle.  --dump-outputs DIR writes what the last timed step computed as .npy files (see :func:`dump_outputs`).

N > 1: one rank per GPU.  Started by `python -m torch.distributed.run` the ranks read RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_*; started plainly (`python bench.py --gpus 8`) this process launches that command itself as a CHILD -- before
anything touches the GPU -- and forwards rank 0's JSON line and the exit code.
  --scaling weak   (default) every rank codes its own GOPs per step: per-GPU work fixed, no data-path collective;
  --scaling strong BASELINE.json configs[3]: ONE fixed test set (LHBDC/test/testing.py:99-188: 7 sequences, every GOP-8,
                   I-frames included through the mbt2018_mean architecture) sharded by contiguous GOP ranges
                   (vcamd.gop.shard_gops / code_workload); a step = the whole set once.
In both modes the only exchange is the final all-gather of per-frame R-D records (RCCL over xGMI).
Rank 0 prints ONE JSON line.
"""
import argparse
import hashlib
import json
import os
import socket
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-compression_amd"))

PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: FP32 matrix peak (dense)
PEAK_F16_MFMA_TFLOPS = 2500.0    # BF16/FP16 matrix peak, dense
PEAK_HBM_GBPS = 8000.0           # HBM3E peak (same guide)
TRAFFIC_JSON = os.path.join(ROOT, "profiles", "r06", "traffic.json")
PMC_JSON = os.path.join(ROOT, "profiles", "r06", "b_pmc_split.json")     # SQ counters of the split kernels (tools/r06.sh split-pmc)
PMC_KEYS = {"conv k7 s1 32->64 @4x1088x1920": "k7_32_64", "conv k7 s1 64->32 @4x1088x1920": "k7_64_32",
            "conv k3 s1 128->128 @1x544x960": "k3_128_128", "conv k7 s1 32->16 @4x1088x1920": "k7_32_16"}


def fp32_algorithmic_bytes(key):
    """SURVEY.md 8(d)'s count for a convolution launch named "conv k<K> s<S> <cin>-><cout> @<n>x<h>x<w>": every operand once as fp32
    NHWC -- input, output, weights (4 bytes per element) -- whatever format the tensors have in HBM on the pipeline that ran."""
    import re
    m = re.match(r"conv k(\d+)(?:\+k1)? s(\d+) (\d+)->(\d+) @(\d+)x(\d+)x(\d+)", key)
    if not m:
        return None
    k, st, cin, cout, n, h, w = (int(v) for v in m.groups())
    ho, wo = (h + 2 * (k // 2) - k) // st + 1, (w + 2 * (k // 2) - k) // st + 1
    return 4.0 * (n * h * w * cin + n * ho * wo * cout + cout * cin * k * k)


def kernel_source_stamp():
    """Hash of the convolution kernel sources: profiles/*/traffic.json is valid for exactly one version of them."""
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "video-compression_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.startswith("conv") and name.endswith((".h", ".hip")):
            with open(os.path.join(csrc, name), "rb") as f:
                h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def synthetic_gop(seed, gop_index, device, frames_per_gop=9, hw=None, as_uint8=False):
    """Config 2: band-limited noise texture (Gaussian sigma=3 px) + global translation (1.5,0.75) px per
    frame + 2 % additive noise, quantised to uint8, then /255 and reflection-padded to 1088x1920.
    ``as_uint8``: the 8-bit RGB [h,w,3] frames themselves (what --data writes to PNG files)."""
    from scipy import ndimage
    H, W = hw if hw is not None else (1080, 1920)
    rng = np.random.default_rng(seed)
    margin = 32
    tex = rng.random((3, H + 2 * margin, W + 2 * margin)).astype(np.float32)
    tex = np.stack([ndimage.gaussian_filter(c, 3.0) for c in tex])
    tex = (tex - tex.min()) / (tex.max() - tex.min())
    frames = []
    for t in range(frames_per_gop):
        tt = gop_index * (frames_per_gop - 1) + t
        dx, dy = 1.5 * (tt % 16), 0.75 * (tt % 16)
        shifted = np.stack([ndimage.shift(c, (dy, dx), order=1, mode="nearest") for c in tex])
        f = shifted[:, margin:margin + H, margin:margin + W]
        noise = np.random.default_rng(seed + 1 + tt).standard_normal(f.shape).astype(np.float32) * 0.02
        u8 = np.clip(np.round((f + noise) * 255.0), 0, 255).astype(np.uint8)
        if as_uint8:
            frames.append(np.ascontiguousarray(u8.transpose(1, 2, 0)))
            continue
        x = torch.from_numpy(u8.astype(np.float32) / 255.0)[None]
        x = torch.nn.functional.pad(x, (0, (64 - W % 64) % 64, 0, (64 - H % 64) % 64), mode="reflect")
        frames.append(x.to(device))
    return frames


class SyntheticTestSet:
    """The fixed workload of --scaling strong: ``videos`` sequences of ``frames`` 8-bit frames each, generated ON THE
    DEVICE (same recipe as :func:`synthetic_gop`: band-limited texture, global translation, 2 % noise, 8-bit) and kept
    resident in HBM as uint8 (6.2 MB per 1080p frame: the full 7 x 593-frame set is 26 GB of the 288 GB).  Only the
    frames of this rank's GOP range are generated.  ``frame(video, idx)`` hands the padded fp32 NCHW tensor the codec
    takes (uint8 -> float, /255, reflection pad: the test loop's data loader, LHBDC/test/utils.py:190-203)."""

    def __init__(self, videos, frames, hw, device, seed=1234):
        self.videos, self.frames, self.hw, self.device, self.seed = videos, frames, hw, device, seed
        self.store = {}
        self._tex = {}

    def _texture(self, video):
        if video not in self._tex:
            H, W = self.hw
            g = torch.Generator(device="cpu").manual_seed(self.seed + 1000 * video)
            tex = torch.rand(1, 3, H + 64, W + 64, generator=g).to(self.device)
            k = torch.arange(-9, 10, dtype=torch.float32, device=self.device)
            k = torch.exp(-0.5 * (k / 3.0) ** 2)
            k = (k / k.sum())
            tex = torch.nn.functional.conv2d(tex.transpose(0, 1), k.view(1, 1, 1, -1), padding=(0, 9))
            tex = torch.nn.functional.conv2d(tex, k.view(1, 1, -1, 1), padding=(9, 0)).transpose(0, 1)
            self._tex = {video: (tex - tex.min()) / (tex.max() - tex.min())}       # keep one texture at a time
        return self._tex[video]

    def materialise(self, video, idx):
        key = (video, idx)
        if key in self.store:
            return
        H, W = self.hw
        tex = self._texture(video)
        dx, dy = 1.5 * (idx % 16), 0.75 * (idx % 16)
        ix, iy, fx, fy = int(dx), int(dy), dx - int(dx), dy - int(dy)

        def win(oy, ox):
            return tex[:, :, 32 - iy - oy:32 - iy - oy + H, 32 - ix - ox:32 - ix - ox + W]
        f = ((1 - fy) * ((1 - fx) * win(0, 0) + fx * win(0, 1)) + fy * ((1 - fx) * win(1, 0) + fx * win(1, 1)))
        g = torch.Generator(device=self.device).manual_seed(self.seed + 7919 * video + idx)
        f = f + 0.02 * torch.randn(f.shape, generator=g, device=self.device)
        self.store[key] = torch.clamp(torch.round(f * 255.0), 0, 255).to(torch.uint8)

    def frame(self, video, idx):
        H, W = self.hw
        x = self.store[(video, idx)].to(torch.float32) / 255.0
        return torch.nn.functional.pad(x, (0, (64 - W % 64) % 64, 0, (64 - H % 64) % 64), mode="reflect")


def rd_checksum(rows, frames_limit=None):
    """sha256 over the gathered per-frame R-D records (video, frame, gop, PSNR, bits, pixels, type) in (video, frame) order --
    PSNR and bits as the exact float64 bit patterns.  ``frames_limit``: only frames below that index of every sequence
    (the part of the set every world size codes when the set is sized by --seconds-per-step)."""
    rows = sorted((tuple(float(v) for v in r) for r in rows), key=lambda r: (r[0], r[1], r[6] if len(r) > 6 else 0.0))
    h = hashlib.sha256()
    n = 0
    for r in rows:
        if frames_limit is not None and r[1] >= frames_limit:
            continue
        h.update(np.asarray(r, dtype=np.float64).tobytes())
        n += 1
    return {"sha256": h.hexdigest()[:32], "records": n}


def strong_frames_per_sequence(seconds_per_step, world, sequences):
    per_seq = 17.0 * world * seconds_per_step / sequences
    return 8 * max(1, int(round((per_seq - 1) / 8))) + 1


def strong_hbm_plan(args, dev, world, rank, H, W, G, frames_per_sequence, head_pool_gb, limit=0.85):
    """Will the strong block fit?  need = this rank's resident frames (uint8) + one graph pool per captured pass size, each
    ``head_pool_gb`` (the headline's pool for G GOPs) x GOPs of the pass / G; budget = ``limit`` x device memory - what the process
    already holds.  Returns the (possibly shrunk) sizing and what was done: "none", "whole_passes" (frames per sequence moved to the
    nearest length at which this rank's GOP count is a multiple of G: one graph size instead of two) or "eager" (no graphs at all)."""
    from vcamd import gop as vgop
    total_gb = torch.cuda.get_device_properties(dev).total_memory / 2 ** 30
    held_gb = torch.cuda.memory_reserved(dev) / 2 ** 30
    budget_gb = limit * total_gb - held_gb

    def need(fps):
        plan = vgop.workload_plan([fps] * args.sequences)
        lo, hi = vgop.shard_gops(len(plan), world, rank)
        n = hi - lo
        frames = len({(v, i) for v, _, idxs in plan[lo:hi] for i in idxs})
        sizes = {min(G, n), n % G} - {0}
        return frames * H * W * 3 / 2 ** 30 + (0.0 if args.no_graph else head_pool_gb * sum(sizes) / G), sorted(sizes)
    out = {"device_gb": round(total_gb, 1), "held_before_gb": round(held_gb, 1), "limit": limit, "budget_gb": round(budget_gb, 1),
           "frames_per_sequence": frames_per_sequence, "action": "none"}
    est, sizes = need(frames_per_sequence)
    out.update({"estimated_gb": round(est, 1), "pass_sizes_gops": sizes})
    if est <= budget_gb:
        return out
    k0 = (frames_per_sequence - 1) // 8    # GOPs per sequence; the nearest count (shorter first) at which this rank codes whole passes only
    for k in sorted(range(1, k0 + G + 1), key=lambda k: (abs(k - k0), k)):
        fps = 8 * k + 1
        e2, s2 = need(fps)
        if len(s2) == 1 and e2 <= budget_gb:
            out.update({"frames_per_sequence": fps, "action": "whole_passes", "estimated_gb": round(e2, 1), "pass_sizes_gops": s2,
                        "message": f"estimated pool {est:.0f} GB + {held_gb:.0f} GB held exceeds {100 * limit:.0f} % of {total_gb:.0f} GB: "
                                   f"sequences resized from {frames_per_sequence} to {fps} frames (whole passes of {G} GOPs only, {e2:.0f} GB)"})
            return out
    frames_gb = need(frames_per_sequence)[0] - (0.0 if args.no_graph else head_pool_gb * sum(sizes) / G)
    out.update({"action": "eager", "estimated_gb": round(frames_gb, 1),
                "message": f"estimated pool {est:.0f} GB + {held_gb:.0f} GB held exceeds {100 * limit:.0f} % of {total_gb:.0f} GB even with one "
                           f"graph size: the block runs on eager launches (no graph pool; frames/s of the block is launch-bound)"})
    return out


class StrongWorkload:
    """BASELINE.json configs[3]: ONE fixed test set (LHBDC/test/testing.py:99-188: `sequences` sequences, every GOP-8,
    I-frames included through the mbt2018_mean architecture) cut into contiguous GOP ranges per rank (vcamd.gop.shard_gops /
    code_workload).  A step = the whole set once; the only exchange is the final gather of the R-D records."""

    def __init__(self, args, model, dev, world, rank, H, W, G, frames_per_sequence):
        from vcamd import gop as vgop, iframe
        from vcamd.seeding import calibrated_intra_state_dict
        self.vgop, self.world, self.rank, self.G = vgop, world, rank, G
        i_model = iframe.mbt2018_mean(7, "mse", pretrained=False)
        i_model.load_state_dict(calibrated_intra_state_dict(i_model.state_dict(), seed=4321))
        self.i_model = i_model.to(dev).eval()
        self.frames_per_sequence = frames_per_sequence
        self.plan = vgop.workload_plan([frames_per_sequence] * args.sequences)
        self.lo, self.hi = vgop.shard_gops(len(self.plan), world, rank)
        self.data = SyntheticTestSet(args.sequences, frames_per_sequence, (H, W), dev)
        for video, _, idxs in self.plan[self.lo:self.hi]:
            for i in idxs:
                self.data.materialise(video, i)
        self.coder = vgop.LhbdcWorkloadCoder(model, self.i_model, self.data.frame, H, W, graph=not args.no_graph)
        self.frames_total = len({(video, i) for video, _, idxs in self.plan for i in idxs})       # every frame of the set, coded once

    def capture(self):
        """capture the HIP graphs (full passes of G GOPs and the shorter last pass) before any clock starts"""
        n = self.hi - self.lo
        with torch.no_grad():
            for size in {min(self.G, n), n % self.G}:
                if size > 0:
                    self.vgop.code_workload(self.plan[self.lo:self.lo + size], 1, 0, self.coder.intra, self.coder.code_gops,
                                            gops_per_pass=self.G)

    def step(self, records=None):
        recs = self.vgop.code_workload(self.plan, self.world, self.rank, self.coder.intra, self.coder.code_gops, gops_per_pass=self.G)
        if records is not None:
            records.extend(recs)

    def per_rank_frames(self):
        return [len({(v, i) for v, _, idxs in self.plan[a:b] for i in idxs}) for a, b in
                (self.vgop.shard_gops(len(self.plan), self.world, r) for r in range(self.world))]

    def release(self):
        self.data.store.clear()
        self.coder = None


DUMP_SAMPLES = 1 << 22            # decoded-frame elements written by --dump-outputs (16 MB of float32)


def dump_outputs(out_dir, rows, decoded, seed=20240601):
    """--dump-outputs: what the last timed step computed, as .npy files in ``out_dir`` (the inputs are seeded: two builds given the
    same arguments can be compared file by file).
      rd_records.npy             float64 [frames, 6|7]: the gathered per-frame R-D records of the step in (video, frame) order --
                                 video, frame, hierarchy level, PSNR (dB), bits, pixels (strong scaling: + is_intra)
      b_frames_sample.npy        float32 [B-frames, S]: the decoded B-frames of this rank (GOP by GOP, in frame order), S elements of
                                 each at the same fixed, seeded flat positions of the padded NCHW frame
      b_frames_channel_mean.npy  float64 [B-frames, 3]: per-channel mean of each whole decoded B-frame
    (strong scaling hands back records only: no frame files)."""
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "rd_records.npy"), np.asarray(rows.numpy() if isinstance(rows, torch.Tensor) else rows, dtype=np.float64))
    if decoded is None:
        return
    gops = [decoded] if isinstance(decoded, dict) else list(decoded)
    # boundary frames (first / last key of a GOP) are the decoded I-frames the step was given, not what it computed
    b_frames = [g[k] for g in gops for k in sorted(g)[1:-1]]
    numel = b_frames[0].numel()
    per = min(numel, max(1, DUMP_SAMPLES // len(b_frames)))
    idx = np.sort(np.random.default_rng(seed).choice(numel, size=per, replace=False) if per < numel else np.arange(numel))
    idx = torch.from_numpy(idx).to(b_frames[0].device)
    with torch.no_grad():
        sample = torch.stack([f.reshape(-1).index_select(0, idx) for f in b_frames]).float().cpu().numpy()
        means = torch.stack([f.double().mean(dim=(0, 2, 3)) for f in b_frames]).cpu().numpy()
    np.save(os.path.join(out_dir, "b_frames_sample.npy"), sample.astype(np.float32))
    np.save(os.path.join(out_dir, "b_frames_channel_mean.npy"), means.astype(np.float64))


def physical_cores():
    try:
        import psutil
        n = psutil.cpu_count(logical=False)
        if n:
            return int(n)
    except Exception:  # noqa: BLE001
        pass
    return os.cpu_count() or 1


def launch_children(args):
    """`python bench.py --gpus N` started plainly: run the documented torch.distributed.run command as a child process
    (this process has not touched the GPU), forward rank 0's JSON line, exit with the child's code."""
    share = bool(int(os.environ.get("VC_BENCH_SHARE_GPU", "0")))
    if torch.cuda.device_count() < args.gpus and not share:      # (counting devices does not initialise the GPU)
        raise SystemExit(f"--gpus {args.gpus} but only {torch.cuda.device_count()} GPU(s) are visible")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if line is not None:
        print(line)
    sys.exit(proc.returncode if (proc.returncode != 0 or line is not None) else 1)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", choices=["lhbdc", "flex", "icip2024"], default="lhbdc",
                    help="lhbdc = BASELINE.json configs[1] (headline); flex = configs[2] (Flex-Rate, 4 rate points); "
                         "icip2024 = configs[4]'s model (FlowGuidedB, GOP-16, flow-resolution search, 5 quality levels)")
    ap.add_argument("--precision", choices=["fp32", "fp16"], default="fp32",
                    help="fp32 = exact path (headline); fp16 = half-precision MFMA conv path of BASELINE configs[4]")
    ap.add_argument("--fp32-mode", choices=["native", "split"], default=os.environ.get("VC_FP32_MODE", "split"),
                    help="fp32 path only: native = v_mfma_f32_* instances everywhere; split = the layers csrc/conv_split.h serves run on the "
                         "bf16 matrix pipe with exact bf16 x 3 operands (nine exact products, fp32 accumulate)")
    ap.add_argument("--resolution", choices=["1080p", "2160p"], default="1080p")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="strong = BASELINE configs[3]: a fixed multi-sequence test set GOP-sharded over the ranks (LHBDC)")
    ap.add_argument("--sequences", type=int, default=7, help="--scaling strong: sequences in the test set (UVG: 7)")
    ap.add_argument("--seconds-per-step", type=float, default=None,
                    help="--scaling strong: size the test set (frames per sequence, whole GOP-8s) so that ONE step takes about this "
                         "long at the given number of GPUs (assuming ~17 frames/s per GPU) instead of using --frames-per-sequence; "
                         "with the driver's --steps 20 --warmup 5 a value of 10 keeps the run inside a few minutes")
    ap.add_argument("--frames-per-sequence", type=int, default=593,
                    help="--scaling strong: frames per sequence (UVG: 600 -> 74 GOP-8s = 593 frames coded)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--checkpoint", choices=["calibrated", "seeded"], default="calibrated",
                    help="LHBDC / Flex-Rate weights: calibrated = seeded weights rescaled to trained-like statistics (default), seeded = plain")
    ap.add_argument("--byte-equality", action="store_true",
                    help="N = 1 extras: eight encode_B containers against the CPU oracle's, byte for byte (eight 1088x1920 oracle passes, "
                         "~50 s; tests/test_byte_equality_gpu.py asserts the same) -- off by default since round 5 to keep the driver's run short")
    ap.add_argument("--cpu-all-cores", action="store_true",
                    help="time the CPU oracle at all physical cores as well as at 8 threads (round 2-4 default; the 128-thread run was always slower)")
    ap.add_argument("--parity-both-checkpoints", action="store_true",
                    help="repeat the parity block on the other checkpoint kind (one more oracle pass)")
    ap.add_argument("--skip-extras", action="store_true",
                    help="--full, N = 1: skip the whole-GOP-with-I-frame and real-bitstream blocks (profiling runs: the trace then holds the timed "
                         "region and the one instrumented frame of the roofline block only)")
    ap.add_argument("--no-strong-block", action="store_true",
                    help="--full (weak) LHBDC 1080p line: skip the extra `strong` block (one pass over a configs[3] test set sized by "
                         "--strong-seconds, GOP-sharded over the ranks, R-D table checksum)")
    ap.add_argument("--strong-seconds", type=float, default=10.0,
                    help="size of the `strong` block's test set: about this many seconds per pass at the given number of GPUs")
    ap.add_argument("--gops-per-step", type=int, default=None,
                    help="LHBDC / Flex-Rate: independent GOPs coded per step and GPU with their hierarchy levels batched together "
                         "(default at 1080p: 4 / 2; 1 at 2160p)")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly instead of replaying a HIP graph")
    ap.add_argument("--poison", choices=["nan", "zero", "ones"], default=None,
                    help="debugging aid: fill 96 GB of device memory with this pattern and hand it back to the caching allocator before "
                         "anything else is allocated -- results must not depend on it (no kernel may read memory nobody wrote)")
    ap.add_argument("--data", default=None, metavar="DIR",
                    help="weak scaling, LHBDC: stream the frames of every step from PNG files through vcamd.data.SequenceReader "
                         "(decode workers -> pinned ring -> async H2D) instead of coding device-resident tensors; the synthetic clip "
                         "is written to DIR/<rank>/seq00/*.png first when it is not there yet")
    ap.add_argument("--data-workers", type=int, default=8)
    ap.add_argument("--kernel-table", default=None, help="--full: write the per-kernel event timing table here (json)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run every other measurement and check of the line: the `strong` block (default LHBDC "
                         "1080p line) and, at N = 1, roofline, native-fp32, whole-GOP, bitstream, CPU baseline and parity blocks; "
                         "a plain run times the headline steps only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last step computed to DIR/<name>.npy (rank 0): the gathered per-frame "
                         "R-D records and a fixed, seeded sample of the decoded B-frames")
    return ap.parse_args()


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        launch_children(args)          # never returns

    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # Functional check of the multi-rank path on a box with ONE GPU (tests / debugging, never a measurement):
    # VC_BENCH_SHARE_GPU=1 maps every rank onto the visible devices round-robin and VC_BENCH_BACKEND=gloo replaces RCCL
    # (which refuses two ranks on one device); the R-D gather then travels through host memory.
    backend = os.environ.get("VC_BENCH_BACKEND", "nccl")
    if bool(int(os.environ.get("VC_BENCH_SHARE_GPU", "0"))):
        local_rank = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    if args.poison:
        blocks = [torch.empty(1 << 30, dtype=torch.int32, device=f"cuda:{local_rank}") for _ in range(24)]       # 24 x 4 GB
        for b in blocks:
            b.fill_({"nan": 0x7fc00000, "zero": 0, "ones": 0x3f800000}[args.poison])
        torch.cuda.synchronize()
        del blocks                        # (back to the caching allocator, NOT to the driver: the next allocations are carved from it)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from vcamd import flex, hip, lhbdc
    from vcamd import gop as vgop
    from vcamd.seeding import calibrated_state_dict, seeded_state_dict

    H, W = (2160, 3840) if args.resolution == "2160p" else (1080, 1920)
    hip.set_conv_precision(args.precision)
    f16 = args.precision == "fp16"
    hip.set_fp32_mode("native" if f16 else args.fp32_mode)
    is_flex = args.model == "flex"
    is_icip = args.model == "icip2024"
    strong = args.scaling == "strong"
    if strong and (is_flex or is_icip):
        raise SystemExit("--scaling strong is BASELINE configs[3]: the LHBDC test loop")
    if is_icip:
        from vcamd import icip2024
        model = icip2024.FlowGuidedB()
    else:
        model = flex.BidirFlowRef(n=4) if is_flex else lhbdc.Model()
    # LHBDC / Flex-Rate: the checkpoint with TRAINED-LIKE statistics (vcamd.seeding.calibrated_state_dict: sub-pixel flow heads,
    # |y - mu| ~ 1, scales spread over the table, a decoded residual that is a small correction) -- kernel times do not depend on
    # the weights, the quality block and the parity figures do.  --checkpoint seeded = the plain seeded weights of rounds 1-3.
    checkpoint = "seeded" if is_icip else args.checkpoint
    sd = (calibrated_state_dict if checkpoint == "calibrated" else seeded_state_dict)(model.state_dict(), seed=1234)
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    per_gop = 15 if (is_flex or is_icip) else 7
    # GOPs per step and GPU (LHBDC): 4 at 1080p (+2.5 % over one: the single-frame level and the coarse layers get 4x
    # the work per launch), 1 at 2160p where a level pass is already four 1080p frames' worth of pixels
    G = 1 if is_icip else (args.gops_per_step or ((2 if is_flex else 4) if args.resolution == "1080p" else 1))

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    records = []
    if strong:
        # ---- BASELINE configs[3]: one fixed test set, contiguous GOP ranges per rank ----
        if args.seconds_per_step:
            args.frames_per_sequence = strong_frames_per_sequence(args.seconds_per_step, world, args.sequences)
        sw = StrongWorkload(args, model, dev, world, rank, H, W, G, args.frames_per_sequence)
        plan, lo, hi, frames_total = sw.plan, sw.lo, sw.hi, sw.frames_total

        def step(keep):
            sw.step(records if keep else None)
        n_warm = args.warmup
        sw.capture()
    else:
        # every rank codes its own GOPs (GOP index = rank * G + g): weak scaling, per-GPU work fixed
        frames = []
        for g in range(G):
            frames += synthetic_gop(1234, rank * G + g, dev, 17 if (is_flex or is_icip) else 9, (H, W))
        # Flex: 4 rate points selected purely through the gain units (n = 0..3, l = 1), one per step in turn
        rate_points = [{lvl: (n, 1.0) for lvl in range(4)} for n in range(4)]
        if is_icip:                     # quality levels 0..4 in turn; the per-frame flow-resolution search runs on the device
            pool = None if args.no_graph else torch.cuda.graph_pool_handle()   # the five graphs replay in turn: one memory pool
            runners = [None if args.no_graph else vgop.GopGraph(model, H, W, kind="icip2024", quality=lvl, pool=pool)
                       for lvl in range(5)]
        elif is_flex:
            runners = [None if args.no_graph else vgop.GopGraph(model, H, W, kind="flex", quality=q, gops=G) for q in rate_points]
        else:
            runners = [None if args.no_graph else vgop.GopGraph(model, H, W, gops=G)]
        counter = [0]
        last_out = [None]               # what the latest step handed back: the decoded frames (--dump-outputs)
        reader = None
        if args.data:
            if is_flex or is_icip:
                raise SystemExit("--data streams the LHBDC GOP-8 workload")
            from vcamd import data as vdata
            root = os.path.join(args.data, f"rank{rank}")
            seq = os.path.join(root, "seq00")
            if not (os.path.isdir(seq) and len(os.listdir(seq)) == 9 * G):
                clip = []
                for g in range(G):
                    clip += synthetic_gop(1234, rank * G + g, dev, 9, (H, W), as_uint8=True)
                vdata.write_synthetic_sequences(root, [clip], ["seq00"])
            # the G GOPs of a step are 9 consecutive files each; every step asks for all of them again, in order
            reader = vdata.SequenceReader(root, ["seq00"], gop_size=8, test_size=0, device=dev, workers=args.data_workers,
                                          depth=2 * 9 * G)
            keys = [(0, i) for i in range(9 * G)]
            reader.prefetch(keys)

        def step(keep):
            i = counter[0] % len(runners)
            counter[0] += 1
            recs = records if keep else None
            if reader is not None:
                # decoded straight into the GOP runner's static input tensors once they exist (no extra device copy)
                static = runners[i].static_in if (runners[i] is not None and getattr(runners[i], "static_in", None)) else [None] * len(keys)
                for j, k in enumerate(keys):
                    frames[j] = reader.load_frame(*k, out=static[j])
                reader.prefetch(keys)                       # the next step's frames decode while this step's GOPs are coded
            if runners[i] is not None:
                last_out[0] = runners[i].code(frames, gop_index=rank * G, records=recs)
            elif is_icip:
                last_out[0] = vgop.code_gop_icip2024(model, frames, frames[0], frames[16], H, W, i, recs, video=0, gop_index=rank)[0]
            elif is_flex:
                gops = [frames[17 * g:17 * g + 17] for g in range(G)]
                last_out[0] = vgop.code_gops_flex(model, gops, [(gp[0], gp[16]) for gp in gops], H, W, rate_points[i], recs, video=0,
                                                  first_gop_index=rank * G)
            else:
                gops = [frames[9 * g:9 * g + 9] for g in range(G)]
                last_out[0] = vgop.code_gops_lhbdc(model, gops, [(gp[0], gp[8]) for gp in gops], H, W, recs, video=0,
                                                   first_gop_index=rank * G)
        n_warm = max(args.warmup, len(runners))          # every graph is captured before the clock starts

    with torch.no_grad():
        for _ in range(n_warm):
            step(False)
        if not strong:
            counter[0] = 0
        barrier()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(i == args.steps - 1)
        torch.cuda.synchronize()
        t_coded = time.perf_counter() - t0              # this rank's own work, before it meets the others
        rows = vgop.gather_records(records, dev, width=7 if strong else 6)      # the only exchange: final R-D gather (RCCL)
        t_gathered = time.perf_counter() - t0
        barrier()
        elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, rows, None if strong else last_out[0])
    if os.environ.get("VC_BENCH_DUMP_RECORDS") and rank == 0:      # debugging aid: the gathered per-frame records, exact (float.hex)
        with open(os.environ["VC_BENCH_DUMP_RECORDS"], "w") as f:
            json.dump([[float(v).hex() for v in r] for r in sorted(rows.tolist())], f)
    rank_stats = None
    if world > 1:
        cdev = dev if backend == "nccl" else "cpu"
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        # per-rank view of the timed region (after the clock has stopped): a sub-linear point must be explainable from the line
        mine = torch.tensor([t_coded, t_gathered - t_coded, elapsed, float(len(records))], dtype=torch.float64, device=cdev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        allr = torch.stack(allr).cpu().tolist()
        rank_stats = {"coded_s": [round(r[0], 4) for r in allr], "gather_s": [round(r[1], 4) for r in allr],
                      "elapsed_s": [round(r[2], 4) for r in allr], "records_last_step": [int(r[3]) for r in allr]}
        elapsed = float(tmax.item())

    coded_frames = (frames_total if strong else per_gop * G * world) * args.steps
    try:        # the headline configuration reports BASELINE.json's metric verbatim (UVG itself is unavailable: see "data")
        with open(os.path.join(ROOT, "BASELINE.json")) as f:
            headline_metric = json.load(f)["metric"]
    except (OSError, KeyError, ValueError):
        headline_metric = "frames/sec + bpp/PSNR on UVG 1080p GOP-8, 1/2/4/8 MI355X"
    if strong:
        workload = (f"UVG-shaped test set, {args.sequences} sequences x {args.frames_per_sequence} frames at {args.resolution} "
                    f"({len(plan)} GOP-8s: I-frames through the mbt2018_mean q7 architecture + 7 B-frames through LHBDC "
                    f"Model.forward), contiguous GOP ranges per rank, {G} GOPs per batched pass")
    elif is_icip:
        workload = (f"ICIP2024 FlowGuidedB {args.resolution} GOP-16: 15 B-frames per GOP via FlowGuidedB.forward with the "
                    "per-frame flow-resolution search (5 flow+warp passes), quality level s=step%5, one GOP per GPU per step")
    elif is_flex:
        workload = (f"Flex-Rate b_model {args.resolution} GOP-16: 15 B-frames per GOP via BidirFlowRef.forward, rate point "
                    f"n=step%4 through the gain units, {G} independent GOP(s) per GPU per step, hierarchy levels batched")
    else:
        workload = (f"LHBDC {args.resolution} GOP-8 inference, single lambda: 7 B-frames per GOP via Model.forward, "
                    f"{G} independent GOP(s) per GPU per step, hierarchy levels batched across them")
    result = {
        # BASELINE.json: "frames/sec + bpp/PSNR on UVG 1080p GOP-8"; value = frames/s of the codec hot path (B-frames; in
        # the strong-scaling test-set mode every coded frame, I-frames included), bpp/PSNR of the same frames in "quality"
        "metric": (f"frames/sec + bpp/PSNR on {args.resolution} GOP-16 (ICIP2024 FlowGuidedB B-frame path, 5 quality levels)" if is_icip else
                   f"frames/sec + bpp/PSNR on {args.resolution} GOP-16 (Flex-Rate B-frame path, 4 rate points)" if is_flex else
                   headline_metric if (args.resolution == "1080p") else
                   f"frames/sec + bpp/PSNR on {args.resolution} GOP-8 (LHBDC B-frame codec path)"),
        "value": coded_frames / elapsed,
        "unit": "frames/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1000.0 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": ("f16 operands / f32 accumulate (eligible convolutions; activations between them and, VC_HALF_RESIDUAL=1, the identity "
                  "path of bottleneck chains stored as half), f32 elsewhere") if f16 else "f32",
        "fp32_mode": None if f16 else (args.fp32_mode + (" (f32 operands as exact sums of three bf16 pieces, all nine piece products -- each exact in f32 -- "
                                                         "accumulated in f32 on v_mfma_f32_16x16x32_bf16 for the layers csrc/conv_split.h serves; "
                                                         "native v_mfma_f32_* elsewhere)" if args.fp32_mode == "split" else " (v_mfma_f32_* everywhere)")),
        "data": f"synthetic (band-limited texture + global translation + 2% noise, {H}x{W} reflection-padded to x64); "
                + ("seeded random weights rescaled to trained-like statistics (vcamd.seeding.calibrated_state_dict)" if checkpoint == "calibrated"
                   else "seeded random weights"),
        "config": {"workload": workload,
                   "frames_per_step": (frames_total if strong else per_gop * G * world), "gop": 16 if (is_flex or is_icip) else 8,
                   "resolution": f"{W}x{H}", "precision": args.precision, "parallelism": f"gop-shard x{world}",
                   "launch": "eager" if args.no_graph else "hip-graph per GOP pass"},
    }
    if not strong and reader is not None:
        st = reader.stats
        n = max(1, st["frames"])
        result["data"] += f"; frames streamed from PNG files ({args.data}) through vcamd.data.SequenceReader"
        result["ingest"] = {"source": "png", "frames_loaded": st["frames"], "frames_per_step": len(keys), "workers": args.data_workers,
                            "decode_ms_per_frame_worker": round(1000.0 * st["decode_s"] / n, 2),
                            "h2d_ms_per_frame": round(1000.0 * st["h2d_s"] / n, 3),
                            "consumer_wait_ms_per_step": round(1000.0 * st["wait_s"] / max(1, counter[0] + n_warm), 2),
                            "what": "every step loads its 9*G frames from disk (decode threads -> pinned ring -> async H2D on a side "
                                    "stream -> uint8->fp32 pad kernel); the wait is the time load_frame blocked the coding thread, "
                                    "warm-up steps included"}
        reader.close()
    if world > 1:
        result["rccl_ranks" if backend == "nccl" else f"{backend}_ranks"] = world
        per_rank_frames = ([len({(v, i) for v, _, idxs in plan[a:b] for i in idxs}) for a, b in
                            (vgop.shard_gops(len(plan), world, r) for r in range(world))] if strong else [per_gop * G] * world)
        result["ranks"] = {"backend": backend, "world": world,
                           "frames_per_step_per_rank": per_rank_frames,          # (strong: a shard re-codes its first boundary I-frame)
                           "coded_s_min": min(rank_stats["coded_s"]), "coded_s_max": max(rank_stats["coded_s"]),
                           "gather_s_max": max(rank_stats["gather_s"]), **rank_stats,
                           "what": "coded_s = this rank's steps incl. its final device sync; gather_s = R-D record all-gather (waits for the "
                                   "slowest rank); elapsed_s = up to the closing barrier; value uses the MAX elapsed over ranks"}
    quality_note = ("calibrated seeded weights (trained-like statistics, vcamd.seeding): R-D values are parity references, not the "
                    "published curve" if checkpoint == "calibrated" else "seeded random weights: R-D values are parity references, not codec quality")
    if (args.full and not strong and not is_flex and not is_icip and args.resolution == "1080p" and not f16 and not args.no_strong_block
            and not args.data):
        # ---- the SAME line also carries BASELINE configs[3] (the metric's "1/2/4/8 MI355X" half as a fixed-work measurement):
        # ONE pass over a UVG-shaped test set sized to ~--strong-seconds at this number of GPUs, contiguous GOP ranges per
        # rank, I-frames included, R-D records gathered over RCCL.  Frames and records are functions of (sequence, index)
        # alone, so the checksum over the part of the set EVERY world size codes (the N = 1 sizing) must agree across N. ----
        # (the headline workload's high-water mark is taken BEFORE the strong block allocates its test set and graphs)
        result["peak_hbm_gb"] = round(torch.cuda.max_memory_reserved(dev) / 2 ** 30, 1)
        torch.cuda.reset_peak_memory_stats(dev)
        fps_n = strong_frames_per_sequence(args.strong_seconds, world, args.sequences)
        fps_1 = strong_frames_per_sequence(args.strong_seconds, 1, args.sequences)
        # ---- HBM headroom (round 6): the block's pool is estimated BEFORE anything is allocated -- the resident 8-bit frames plus one
        # graph pool per pass size, each like the headline's (measured above) scaled by its GOP count -- and the block is shrunk until
        # the device stays below 85 % of its memory: first to whole passes only (one graph size), then to eager launches (no graph
        # pool).  What was done is printed and recorded in the line. ----
        hbm_guard = strong_hbm_plan(args, dev, world, rank, H, W, G, fps_n, head_pool_gb=result["peak_hbm_gb"])
        if hbm_guard["action"] != "none":
            print(f"[bench] strong block: {hbm_guard['message']}", file=sys.stderr, flush=True)
        fps_n = hbm_guard["frames_per_sequence"]
        fps_1 = min(fps_1, fps_n)
        keep_graph = args.no_graph
        args.no_graph = args.no_graph or hbm_guard["action"] == "eager"
        sw = StrongWorkload(args, model, dev, world, rank, H, W, G, fps_n)
        args.no_graph = keep_graph
        sw.capture()
        s_records = []
        with torch.no_grad():
            barrier()
            t0 = time.perf_counter()
            sw.step(s_records)
            torch.cuda.synchronize()
            s_coded = time.perf_counter() - t0
            s_rows = vgop.gather_records(s_records, dev, width=7)
            s_gathered = time.perf_counter() - t0
            barrier()
            s_elapsed = time.perf_counter() - t0
        s_stats = [[s_coded, s_gathered - s_coded, s_elapsed]]
        if world > 1:
            cdev = dev if backend == "nccl" else "cpu"
            mine = torch.tensor(s_stats[0], dtype=torch.float64, device=cdev)
            allr = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(allr, mine)
            s_stats = torch.stack(allr).cpu().tolist()
        s_elapsed = max(r[2] for r in s_stats)
        table = vgop.RdTable()
        table.extend_from_records(s_rows.tolist(), level=7)
        allf = table.per_level()[7]
        if allf["frames"] != sw.frames_total:
            raise SystemExit(f"strong block: gathered {allf['frames']} frame records, the test set has {sw.frames_total}")
        result["strong"] = {
            "workload": f"BASELINE configs[3]: {args.sequences} sequences x {fps_n} frames at {args.resolution} ({len(sw.plan)} GOP-8s, I-frames "
                        f"through the mbt2018_mean q7 architecture + 7 B-frames through Model.forward each), contiguous GOP ranges per rank; "
                        f"ONE pass, sized to ~{args.strong_seconds:g} s at {world} GPU(s)",
            "scaling": "strong", "frames": sw.frames_total, "value": sw.frames_total / s_elapsed, "unit": "frames/s", "elapsed_s": round(s_elapsed, 4),
            ("rccl_ranks" if backend == "nccl" else f"{backend}_ranks"): world,
            "frames_per_rank": sw.per_rank_frames(),
            "coded_s": [round(r[0], 4) for r in s_stats], "gather_s": [round(r[1], 4) for r in s_stats],
            "quality": {"frames": allf["frames"], "bpp_estimated": allf["bpp"], "psnr_db": allf["psnr"], "note": quality_note},
            "rd_checksum": rd_checksum(s_rows.tolist()),
            "rd_checksum_common": dict(rd_checksum(s_rows.tolist(), frames_limit=fps_1), frames_per_sequence=fps_1,
                                       what="records of the frames every world size codes (the N = 1 sizing of the set): equal across N"),
        }
        result["strong"]["peak_hbm_gb"] = round(torch.cuda.max_memory_reserved(dev) / 2 ** 30, 1)   # test set + graphs of this block
        result["strong"]["hbm_guard"] = hbm_guard
        sw.release()
        del sw
        torch.cuda.empty_cache()          # (the test set and its graphs: ~100 GB of cached blocks nothing below needs)
    result.setdefault("peak_hbm_gb", round(torch.cuda.max_memory_reserved(dev) / 2 ** 30, 1))   # of 288 GB, this rank, graphs included
    if strong:
        table = vgop.RdTable()
        table.extend_from_records(rows.tolist(), level=7)
        agg = table.per_level_frame_type()
        allf = table.per_level()[7]
        result["quality"] = {"frames": allf["frames"], "bpp_estimated": allf["bpp"], "psnr_db": allf["psnr"],
                             "rd_table": {f"{k[1]}": v for k, v in agg.items()}, "note": quality_note}
        if allf["frames"] != frames_total:
            raise SystemExit(f"gathered {allf['frames']} frame records, the test set has {frames_total}")
        result["rd_checksum"] = rd_checksum(rows.tolist())
    else:
        q = vgop.summarize(rows)
        result["quality"] = {"b_frames": q["frames"], "bpp_estimated": q["bpp"], "psnr_db": q["psnr"], "note": quality_note}

    if args.full and rank == 0 and world == 1:
        if strong:
            frames = synthetic_gop(1234, 0, dev, 9, (H, W))
        single_gpu_extras(args, result, model, frames, sd, dev, H, W)
    if rank == 0:
        print(json.dumps(result))
    if world > 1:
        dist.destroy_process_group()


def single_gpu_extras(args, result, model, frames, sd, dev, H, W):
    """--full, N = 1 only: roofline of the dominant kernel (HIP events on the launch stream), whole-GOP rate with the I-frame,
    the CPU baseline (oracle timed on this host) and the parity of the same frame against it."""
    from vcamd import gop as vgop
    from vcamd import hip
    from vcamd.seeding import seeded_state_dict
    f16 = args.precision == "fp16"
    is_flex = args.model == "flex"
    is_icip = args.model == "icip2024"
    mid = 8 if (is_flex or is_icip) else 4

    def product_frame(trace=None):
        if is_icip:
            g = model(frames[0], frames[16], 0.5, 0.5, frames[8], 2, 1)
            return g["x_hat"], float(g["size"].item())
        if is_flex:
            x_hat, tot = model.forward_device(frames[0], frames[mid], frames[2 * mid], n=[1], l=1.0, trace=trace)
            return x_hat, float(tot.sum().item())
        x_hat, tot = model.forward_device(frames[0], frames[mid], frames[2 * mid], trace=trace)
        return x_hat, float(tot.sum().item())

    # ---- roofline of the dominant kernel: HIP events on the launch stream, instrumented B-frames ----
    # (three instrumented frames, averaged: a single launch of the dominant kernel varies by +-2 % with what ran before it)
    NFR = 3
    with torch.no_grad():
        product_frame()                  # (untimed: the first eager frame behind another workload runs 2-3 % slow)
        torch.cuda.synchronize()
        hip.timer = hip.KernelTimer()
        for _ in range(NFR):
            product_frame()
        table = hip.timer.table()
        hip.timer = None
    for v in table.values():
        v["ms"], v["flops"], v["bytes"], v["launches"] = v["ms"] / NFR, v["flops"] / NFR, v["bytes"] / NFR, max(1, v["launches"] // NFR)
    # memory-bound kernels (warp, resampling, SPyNet level input, Gaussian conditional): achieved GB/s of the algorithmic
    # traffic against the HBM peak, from the same HIP events (north star: "rocprof HBM GB/s ... against gfx950 peak")
    hbm = {k[4:]: v for k, v in table.items() if k.startswith("hbm ")}
    table = {k: v for k, v in table.items() if not k.startswith("hbm ")}
    result["hbm_kernels"] = {
        k: {"launches": v["launches"], "avg_us": round(1000.0 * v["ms"] / v["launches"], 2),
            "algorithmic_mb_per_launch": round(v["bytes"] / v["launches"] / 1e6, 2),
            "achieved_gbps": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1),
            "frac_of_hbm_peak": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9 / PEAK_HBM_GBPS, 3)}
        for k, v in sorted(hbm.items(), key=lambda kv: -kv[1]["ms"])[:8] if v["ms"] > 0}
    result["hbm_kernels_ms_per_frame"] = round(sum(v["ms"] for v in hbm.values()), 3)
    total_ms = sum(v["ms"] for v in table.values())
    ranked = sorted(table.items(), key=lambda kv: -kv[1]["ms"])
    key, dom = ranked[0]
    per_launch_flop = dom["flops"] / dom["launches"]
    per_launch_bytes = dom["bytes"] / dom["launches"]
    avg_ms = dom["ms"] / dom["launches"]
    peak = PEAK_F16_MFMA_TFLOPS if f16 else PEAK_F32_MFMA_TFLOPS
    dom_split = (not f16) and key in getattr(hip, "split_keys", set())
    if dom_split:
        # the dominant launch ran on the split-operand pipeline: an exact fp32 product costs NINE bf16 products there, so the
        # roof of the ALGORITHMIC fp32 FLOP rate is the dense bf16 matrix peak / 9
        peak = PEAK_F16_MFMA_TFLOPS / 9.0
    # which roofline bounds the dominant kernel: arithmetic intensity against the ridge peak_flops / peak_bandwidth
    intensity = per_launch_flop / max(per_launch_bytes, 1.0)
    if intensity >= peak * 1e12 / (PEAK_HBM_GBPS * 1e9):
        achieved = per_launch_flop / (avg_ms * 1e-3) / 1e12
        result["roofline"] = {"bound": "mfma", "kernel": key, "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
                              "frac": achieved / peak, "traffic": None}
    else:
        achieved = per_launch_bytes / (avg_ms * 1e-3) / 1e9
        result["roofline"] = {"bound": "hbm", "kernel": key, "achieved": achieved, "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                              "frac": achieved / PEAK_HBM_GBPS, "traffic": None}
    if dom_split:
        result["roofline"].update({
            "pipeline": "split operands (csrc/conv_split.h): 9 x v_mfma_f32_16x16x32_bf16 per 16 x 16 x 32 fp32 block",
            "peak_is": "dense bf16 MFMA peak (2500 TFLOP/s) / 9 products per exact fp32 product",
            "executed_bf16_tflops": 9.0 * result["roofline"]["achieved"],
            "native_fp32_mfma_peak": PEAK_F32_MFMA_TFLOPS,
            "achieved_over_native_fp32_peak": result["roofline"]["achieved"] / PEAK_F32_MFMA_TFLOPS})
    # which kernel instance the dominant launch ran, as a rocprofv3 trace names it: the committed trace of this command is matched on it
    # (tests/test_profiles_cpu.py); the instrumented frames are the last thing launched under --skip-extras, and within a frame the
    # dominant shape (finest pyramid level) is the LAST dispatch of its instance
    result["roofline"]["kernel_symbol"] = getattr(hip, "kernel_symbols", {}).get(key)
    result["roofline"].update({"launches_per_frame": dom["launches"], "avg_launch_ms": avg_ms,
                               "share_of_conv_time": dom["ms"] / total_ms,
                               "algorithmic_flop_per_launch": per_launch_flop,
                               "algorithmic_bytes_per_launch": per_launch_bytes,
                               "algorithmic_bytes_fp32": fp32_algorithmic_bytes(key),
                               "algorithmic_bytes_note": "algorithmic_bytes_per_launch counts the formats the tensors have in HBM on the pipeline "
                                                         "that ran (split tensors: 6 bytes per element); algorithmic_bytes_fp32 is SURVEY 8(d)'s "
                                                         "count, 4 bytes per element, input + output + weights",
                               "flop_per_byte": intensity})
    # executed matrix instructions per launch from the committed SQ counters: nine v_mfma_f32_16x16x32_bf16 (16 384 FLOP each) per exact
    # fp32 block -- the count shows that no piece product is dropped
    try:
        with open(PMC_JSON) as f:
            pk = json.load(f)["kernels"].get(PMC_KEYS.get(key, ""))
        if pk and dom_split:
            insts = pk["SQ_INSTS_MFMA"]
            result["roofline"].update({"mfma_insts": insts, "mfma_flop_executed": insts * 16384.0,
                                       "mfma_flop_executed_over_9x_algorithmic": insts * 16384.0 / (9.0 * per_launch_flop),
                                       "mfma_busy_fraction": pk.get("mfma_busy_fraction"),
                                       "mfma_insts_source": f"{os.path.relpath(PMC_JSON, ROOT)} (rocprofv3 --pmc SQ_INSTS_MFMA, per launch)"})
    except (OSError, KeyError, ValueError):
        pass
    # HBM bytes per launch of that kernel from the committed rocprofv3 --pmc passes (FETCH_SIZE and WRITE_SIZE collected
    # in separate runs and corrected as tools/pmc_traffic.py documents).  The file is stamped with a hash of the kernel
    # sources it was measured on: a stale one is refused rather than quoted.
    try:
        if f16 or is_flex or is_icip or args.resolution != "1080p":
            raise KeyError("the PMC passes measured the fp32 kernels of the headline configuration only")
        with open(TRAFFIC_JSON) as f:
            tj = json.load(f)
        if tj.get("kernel_source_stamp") != kernel_source_stamp():
            result["roofline"]["traffic_note"] = (f"{os.path.relpath(TRAFFIC_JSON, ROOT)} was measured on other kernel sources "
                                                  "(stamp mismatch): re-run tools/pmc_traffic.py")
        else:
            tr = tj["kernels"].get(key)
            if tr:
                result["roofline"]["traffic"] = tr["hbm_bytes_per_launch"]
                result["roofline"]["traffic_over_algorithmic"] = tr["hbm_bytes_per_launch"] / per_launch_bytes
                if fp32_algorithmic_bytes(key):
                    result["roofline"]["traffic_over_algorithmic_fp32"] = tr["hbm_bytes_per_launch"] / fp32_algorithmic_bytes(key)
                result["roofline"]["traffic_source"] = f"{os.path.relpath(TRAFFIC_JSON, ROOT)} (rocprofv3 --pmc, separate passes)"
            # the two dominant 7x7 kernels take turns at the top of the table: always show the worse traffic ratio of the pair
            pair = {k: v for k, v in tj["kernels"].items() if k.startswith("conv k7 s1") and k in table}
            if pair:
                worst = max(pair, key=lambda k: pair[k]["hbm_bytes_per_launch"] / (table[k]["bytes"] / table[k]["launches"]))
                result["roofline"]["worst_traffic_ratio"] = {
                    "kernel": worst, "traffic": pair[worst]["hbm_bytes_per_launch"],
                    "over_algorithmic": pair[worst]["hbm_bytes_per_launch"] / (table[worst]["bytes"] / table[worst]["launches"])}
    except (OSError, KeyError, ValueError):
        pass
    ns = [kv for kv in ranked if kv[0].startswith("conv k3 s1 128->128 @1x544x960")]
    if ns:
        v = ns[0][1]
        a = v["flops"] / v["launches"] / (v["ms"] / v["launches"] * 1e-3) / 1e12
        result["roofline_3x3_analysis_conv"] = {"kernel": ns[0][0], "achieved": a, "peak": peak,
                                                "unit": "TFLOP/s", "frac": a / peak,
                                                "avg_launch_ms": v["ms"] / v["launches"], "launches": v["launches"]}
    all_flops = sum(v["flops"] for v in table.values())
    result["conv_engine"] = {"frame_conv_ms": total_ms, "frame_conv_tflop": all_flops / 1e12,
                             "avg_tflops": all_flops / (total_ms * 1e-3) / 1e12,
                             "what": "one B-frame launched eagerly with HIP events around every convolution"}
    if args.scaling == "weak" and result.get("value"):      # (weak mode: value = B-frames/s of the codec hot path)
        # the timed region itself (level-batched HIP graph): algorithmic FLOP of one forward x B-frames/s.  A lower bound
        # of the rate the kernels ran at -- everything that is not a convolution of `forward` (resampling, entropy kernels,
        # the ICIP2024 per-frame flow-resolution search) is counted as time but not as work.
        result["conv_engine"]["timed_region_tflops"] = all_flops / 1e12 * result["value"]
    if args.kernel_table:
        with open(args.kernel_table, "w") as f:
            rows = {k: dict(v, avg_ms=v["ms"] / v["launches"], tflops=v["flops"] / max(v["ms"], 1e-9) / 1e9,
                            gbps=v["bytes"] / max(v["ms"], 1e-9) / 1e6, share_of_conv_time=v["ms"] / total_ms) for k, v in ranked}
            json.dump({"what": "one B-frame launched eagerly with HIP events around every launch (python bench.py --kernel-table ...)",
                       "model": args.model, "precision": args.precision, "resolution": args.resolution,
                       "conv_ms_per_frame": total_ms, "convolutions": rows, "hbm_kernels": result["hbm_kernels"]}, f, indent=1)

    if (not f16 and args.fp32_mode == "split" and not is_flex and not is_icip and args.scaling == "weak" and not args.no_graph
            and not args.skip_extras and len(frames) % 9 == 0):
        # ---- the same timed workload on the NATIVE fp32 instances (v_mfma_f32_* everywhere), side by side with `value` ----
        hip.set_fp32_mode("native")
        Gn = len(frames) // 9
        runner = vgop.GopGraph(model, H, W, gops=Gn)
        with torch.no_grad():
            for _ in range(2):
                runner.code(frames, gop_index=0, records=None)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(3):
                runner.code(frames, gop_index=0, records=None)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t1) / 3
        del runner
        hip.set_fp32_mode(args.fp32_mode)
        result["fp32_native"] = {"value": 7.0 * Gn / dt, "unit": "frames/s", "ms_per_step": 1000.0 * dt, "steps": 3, "warmup": 2,
                                 "what": "the timed workload with every fp32 layer on the native v_mfma_f32_* instances (hip.set_fp32_mode('native'), "
                                         "the round 1-4 headline path), same graphs, same frames",
                                 "split_over_native": result["value"] / (7.0 * Gn / dt)}

    if not is_flex and not is_icip and args.resolution == "1080p" and args.scaling == "weak" and not args.skip_extras:
        # ---- whole GOP as testing.py codes it: 1 I-frame (mbt2018_mean q7 architecture) + 7 B-frames ----
        from vcamd import iframe
        i_model = iframe.mbt2018_mean(7, "mse", pretrained=False)
        from vcamd.seeding import calibrated_intra_state_dict
        i_model.load_state_dict(calibrated_intra_state_dict(i_model.state_dict(), seed=4321))
        i_model = i_model.to(dev).eval()
        with torch.no_grad():
            def full_gop():
                dec_last, _ = i_model.forward_device(frames[8])
                return vgop.code_gop_lhbdc(model, frames, frames[0], dec_last, H, W)
            full_gop()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(2):
                full_gop()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t1) / 2
        result["full_gop"] = {"frames_per_s": 8.0 / dt, "ms_per_gop": 1000.0 * dt,
                              "what": "1 I-frame (mbt2018_mean q7 architecture, vcamd.seeding.calibrated_intra_state_dict) + 7 B-frames per GOP, eager launches"}

    if not is_flex and not is_icip and args.resolution == "1080p" and args.scaling == "weak" and not f16 and not args.skip_extras:
        # ---- the same GOP through the REAL bitstream (encode_B / decode_B containers), host range coder pipelined ----
        from vcamd import bitstream
        model.mv_compressor.update(force=True)
        model.residual_compressor.update(force=True)
        codec = bitstream.LhbdcStreamCodec(model, workers=8)
        with torch.no_grad():
            containers, recon = codec.encode_gop(frames, frames[0], frames[8])
            codec.decode_gop(containers, frames[0], frames[8])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(2):
                containers, recon = codec.encode_gop(frames, frames[0], frames[8])
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            for _ in range(2):
                decoded = codec.decode_gop(containers, frames[0], frames[8])
            torch.cuda.synchronize()
            t3 = time.perf_counter()
        codec.close()
        result["bitstream"] = {"encode_frames_per_s": 14.0 / (t2 - t1), "decode_frames_per_s": 14.0 / (t3 - t2),
                               "bpp_coded": 8.0 * sum(len(c) for c in containers.values()) / (7.0 * H * W),
                               "decoder_equals_encoder_reconstruction": all(torch.equal(decoded[o], recon[o]) for o in range(1, 8)),
                               "what": "7 B-frames of one GOP into / from bits_B.bin containers (CLI wiring of encode_B.py / decode_B.py), "
                                       "one analysis pass per codec, rANS on 8 host threads overlapped with the GPU (vcamd/bitstream.py)"}

    if is_icip and args.resolution == "1080p":
        # ---- whole GOP-16 as src/test.py codes it: 1 intra frame (ELIC architecture, seeded) + 15 B-frames ----
        from vcamd import icip2024
        from vcamd.layers import BitCounter
        i_model = icip2024.ELIC()
        i_model.load_state_dict(seeded_state_dict(i_model.state_dict(), seed=4321, conv_gain=0.7))
        i_model = i_model.to(dev).eval()
        with torch.no_grad():
            def full_gop():
                dec_last = hip.nhwc_to_nchw(i_model.forward_device(hip.nchw_to_nhwc(frames[16]), BitCounter(dev, 6)))
                return vgop.code_gop_icip2024(model, frames, frames[0], torch.clamp(dec_last, 0, 1), H, W, 2)
            full_gop()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(2):
                full_gop()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t1) / 2
        result["full_gop"] = {"frames_per_s": 16.0 / dt, "ms_per_gop": 1000.0 * dt,
                              "what": "1 I-frame (ELIC architecture of src/model/elic.py, seeded) + 15 B-frames per GOP-16, "
                                      "eager launches, quality level 2"}

    # ---- CPU baseline: the oracle (PyTorch-CPU restatement, tensor-equal to the reference), BASELINE.md section 3 ----
    if not args.no_cpu_baseline and args.resolution == "1080p":
        from oracle import flex as oracle_flex
        from oracle import lhbdc as oracle_lhbdc
        from oracle.cai.entropy_models import get_scale_table
        from oracle.trace import CallLog, CodecTrace, symbol_mismatch
        if is_icip:
            from oracle import icip2024 as oracle_icip
            ora = oracle_icip.FlowGuidedB().eval()
        else:
            ora = (oracle_flex.FlexModel(n=4) if is_flex else oracle_lhbdc.LhbdcModel()).eval()
        ora.load_state_dict(sd)
        xb, xc, xa = frames[0].cpu(), frames[mid].cpu(), frames[2 * mid].cpu()

        def oracle_frame():
            if is_icip:
                o = ora(xb, xa, 0.5, 0.5, xc, 2, 1)
                return o["x_hat"], float(o["size"].item())
            if is_flex:
                o = ora(xb, xc, xa, n=[1], l=1.0, train=False)
                return o["x_hat"], float(o["size"].item())
            x_hat, _, bits = ora(xb, xc, xa, False)
            return x_hat, float(bits)

        runs = {}
        ref_hat = ref_bits = None
        traces = None

        def traced_oracle_frame():
            """one call with the latent capture hooked in (the integer parity figures below): the untimed warm-up call"""
            if is_icip:
                return oracle_frame() + (None,)
            mv_name = "flow_compressor" if is_flex else "mv_compressor"
            with CodecTrace(getattr(ora, mv_name)) as t_mv, CodecTrace(ora.residual_compressor) as t_res, \
                    CallLog(ora.Mask if is_flex else ora.masknet) as t_mask:
                hat, bits = oracle_frame()
                table_s = get_scale_table()
                mask_ref = t_mask.outputs[-1]
                tr = {"mv": t_mv.latents(table_s), "res": t_res.latents(table_s),
                      "mask": torch.sigmoid(mask_ref) if is_flex else mask_ref}     # b_model.py:66 applies the sigmoid outside
            return hat, bits, tr

        with torch.no_grad():
            # bounded sample: 1 warm-up (the traced call) + 2 timed calls at 8 threads (comparable with BASELINE.md section 2);
            # --cpu-all-cores adds the all-physical-cores setting of rounds 2-4 (always the slower one on the 128-core hosts)
            settings = [min(8, physical_cores())]
            if args.cpu_all_cores and physical_cores() not in settings:
                settings.append(physical_cores())
            for threads in settings:
                torch.set_num_threads(threads)
                t1 = time.perf_counter()
                if traces is None:
                    ref_hat, ref_bits, traces = traced_oracle_frame()
                else:
                    oracle_frame()
                warm = time.perf_counter() - t1
                times = []
                for _ in range(2):
                    t1 = time.perf_counter()
                    ref_hat, ref_bits = oracle_frame()
                    times.append(time.perf_counter() - t1)
                runs[threads] = {"threads": threads, "median_s_per_frame": statistics.median(times), "times_s": times,
                                 "warmup_s": warm}
            torch.set_num_threads(min(runs.values(), key=lambda r: r["median_s_per_frame"])["threads"])
        best = min(runs.values(), key=lambda r: r["median_s_per_frame"])
        result["cpu_baseline"] = {"value": 1.0 / best["median_s_per_frame"], "unit": "frames/s", "cores": best["threads"],
                                  "kind": "port",
                                  "sample": "1 B-frame 1088x1920 (middle frame of the same GOP) through the PyTorch-CPU fp32 oracle "
                                            "(tensor-equal to the reference); 1 warm-up + 2 timed calls at 8 threads, their mean "
                                            "(--cpu-all-cores adds the all-cores setting: slower on every box so far)",
                                  "runs": list(runs.values()), "host_physical_cores": physical_cores()}
        def parity_block(gpu_hat, gpu_bits, trace, ref_hat, ref_bits, traces):
            src = frames[mid]
            d_psnr = abs(float(vgop.psnr_uint8(gpu_hat, src, H, W)) - float(vgop.psnr_uint8(ref_hat.to(dev), src, H, W)))
            diff = (gpu_hat.cpu() - ref_hat).abs()
            parity = {"d_psnr_db": d_psnr, "bits_rel": abs(gpu_bits - ref_bits) / abs(ref_bits),
                      "max_abs": float(diff.max()), "pixels_over_1e-3": float((diff > 1e-3).float().mean())}
            if traces is None:
                return parity
            # the integers of the bitstream: quantised symbols of y and z for the motion and the residual codec
            sym = {}
            for name, key in (("mv", "flow" if is_flex else "mv"), ("res", "res")):
                for which in ("y_sym", "z_sym"):
                    n_bad, frac = symbol_mismatch(trace[key][which].cpu(), traces[name][which])
                    sym[f"{name}_{which}"] = {"differ": n_bad, "of": int(traces[name][which].numel()), "fraction": frac}
            parity["symbols_differ"] = sym
            total = sum(v["of"] for v in sym.values())
            parity["symbols_differ_fraction"] = sum(v["differ"] for v in sym.values()) / total
            # first-order flips are boundary cases: the oracle's own (y - mu) within fp32 noise of a half-integer.  Only
            # meaningful while nothing upstream flipped (a flipped hyper-latent moves the means every y is rounded against;
            # tests/test_fullsize_gpu.py measures each codec alone on the oracle's input instead)
            upstream = sym["mv_y_sym"]["differ"] + sym["mv_z_sym"]["differ"] + sym["res_z_sym"]["differ"]
            if upstream == 0:
                v = traces["res"]["y"] - traces["res"]["means"]
                flipped = trace["res"]["y_sym"].cpu() != traces["res"]["y_sym"]
                dist = ((v - torch.floor(v)) - 0.5).abs()[flipped]
                parity["res_y_flips_farthest_from_rounding_boundary"] = float(dist.max()) if dist.numel() else 0.0
            else:
                parity["res_y_flips_farthest_from_rounding_boundary"] = None
                parity["note"] = (f"{upstream} upstream symbol(s) flipped: the residual y flips include their cascade (all means / the "
                                  "whole residual input moved), not only first-order rounding cases")
            parity["stage_max_abs"] = {
                "mask": float((hip.nhwc_to_nchw(trace["mask"]).cpu() - traces["mask"]).abs().max()),
                "residual_codec_input": float((hip.nhwc_to_nchw(trace["resid"]).cpu() - traces["res"]["x"]).abs().max()),
                "res_y": float((hip.nhwc_to_nchw(trace["res"]["y"]).cpu() - traces["res"]["y"]).abs().max()),
                "res_scales": float((hip.nhwc_to_nchw(trace["res"]["scales"]).cpu() - traces["res"]["scales"]).abs().max())}
            return parity

        with torch.no_grad():
            trace = {} if not is_icip else None
            gpu_hat, gpu_bits = product_frame(trace)
        result["parity_vs_cpu"] = parity_block(gpu_hat, gpu_bits, trace, ref_hat, ref_bits, traces)
        kind = "seeded" if is_icip else args.checkpoint
        result["parity_vs_cpu"]["checkpoint"] = f"{kind} (vcamd.seeding.{kind}_state_dict, seed 1234) -- the checkpoint of the timed region"
        if not is_icip:
            result["parity_vs_cpu"]["quality_of_this_frame"] = {
                "psnr_db": float(vgop.psnr_uint8(ref_hat.to(dev), frames[mid], H, W)), "bpp_estimated": float(ref_bits) / (H * W),
                "residual_symbols_nonzero": float((traces["res"]["y_sym"] != 0).float().mean()),
                "what": "middle frame of the GOP (references 4 / 8 frames away: the hardest level), CPU oracle's figures"}
        if not is_flex and not is_icip and not f16 and args.checkpoint == "calibrated" and args.byte_equality:
            # ---- byte-equality statistics: eight frame triples of the bench clip through encode_B on both sides (the CPU
            # oracle's eight passes side by side: oracle.pool), the bits_B containers compared byte for byte ----
            from oracle import pool
            from vcamd import lhbdc as vlhbdc
            picks = [(0, 4, 8), (0, 2, 4), (4, 6, 8), (0, 1, 2), (2, 3, 4), (4, 5, 6), (6, 7, 8)]
            picks.append((9, 13, 17) if len(frames) >= 18 else (1, 2, 3))
            model.mv_compressor.update(force=True)
            model.residual_compressor.update(force=True)
            t1 = time.perf_counter()
            refs = pool.run_jobs([tuple(frames[i].cpu() for i in pk) for pk in picks], pool.lhbdc_encode_job(sd))
            t_oracle = time.perf_counter() - t1
            same, per = 0, []
            flips, unaided = {False: 0, True: 0}, {False: 0, True: 0}
            with torch.no_grad():
                for pk, ref in zip(picks, refs):
                    # scale-table indexes against the CPU path's, and the CPU path's container through THIS decoder without handing
                    # it the encoder's indexes -- with plain fp32 scales and with vc_refine_scales (hip.SCALE_REFINE)
                    for refine in (False, True):
                        hip.SCALE_REFINE = refine          # (restored to True right below the loop)
                        t2 = {}
                        vlhbdc.encode_B(model, frames[pk[2]], frames[pk[1]], frames[pk[0]], trace=t2)
                        flips[refine] += sum(int((torch.from_numpy(t2[c]["y_idx"]).reshape(-1) != ref[c]["y_idx"].reshape(-1)).sum()) for c in ("mv", "res"))
                        _, s_mv, s_res, sh_mv, sh_res = vlhbdc.read_container(ref["container"])
                        try:
                            td = {}
                            vlhbdc.decode_B(frames[pk[0]], frames[pk[2]], model, s_mv, s_res, sh_mv, sh_res, trace=td)
                            ok = all(int((torch.from_numpy(td[c]["y_sym"]).reshape(-1) != ref[c]["y_sym"].reshape(-1)).sum()) == 0 for c in ("mv", "res"))
                        except hip.VcError:
                            ok = False
                        unaided[refine] += bool(ok)
                    hip.SCALE_REFINE = True
                    tr = {}
                    mv_b, res_b = vlhbdc.encode_B(model, frames[pk[2]], frames[pk[1]], frames[pk[0]], trace=tr)
                    blob = vlhbdc.write_container(None, 1626, mv_b, res_b)
                    nd = {k: sum(int((torch.from_numpy(tr[c][k]).reshape(-1) != ref[c][k].reshape(-1)).sum()) for c in ("mv", "res"))
                          for k in ("y_sym", "z_sym", "y_idx")}
                    same += blob == ref["container"]
                    per.append({"frames": list(pk), "identical": blob == ref["container"], "bytes": len(blob),
                                "symbols_differing": nd["y_sym"] + nd["z_sym"], "scale_indexes_differing": nd["y_idx"]})
            result["byte_equality"] = {"containers_identical": same, "of": len(picks), "triples": per, "oracle_s": round(t_oracle, 1),
                                       "scale_indexes_differing_plain_fp32_scales": flips[False], "scale_indexes_differing_with_vc_refine_scales": flips[True],
                                       "cpu_containers_decoded_unaided_plain": unaided[False], "cpu_containers_decoded_unaided_refined": unaided[True],
                                       "oracle_workers_x_threads": list(pool.plan(len(picks))),
                                       "what": "end-to-end encode_B (frames -> bits_B container) against the CPU oracle's container, byte for "
                                               "byte; calibrated checkpoint, 1088x1920, ~1.2 M coded integers per frame.  A scale within fp32 "
                                               "noise (3e-7) of one of the 64 log-spaced table entries falls into the neighbouring bin on "
                                               "another platform: ~5e-6 per element, i.e. a handful of indexes per 1080p frame (the stream "
                                               "carries no indexes: the CompressAI format's known cross-platform fragility); "
                                               "tests/test_byte_equality_gpu.py shows every differing integer to be such a boundary case and "
                                               ">= 6 of 8 containers identical at 192x256"}
        if not is_flex and not is_icip and args.parity_both_checkpoints:
            # ---- the same frame on the OTHER checkpoint kind (plain seeded weights when the timed region ran the calibrated
            # ones: latents in the hundreds, 6 dB -- the integer parity has to hold there too) ----
            from vcamd import lhbdc as vlhbdc
            from vcamd.seeding import calibrated_state_dict
            other = "seeded" if args.checkpoint == "calibrated" else "calibrated"
            fn = seeded_state_dict if other == "seeded" else calibrated_state_dict
            sd_o = fn(vlhbdc.Model().state_dict(), seed=1234)     # (a fresh module: empty CDF buffers)
            ora_o = oracle_lhbdc.LhbdcModel().eval()
            ora_o.load_state_dict(sd_o)
            prod_o = vlhbdc.Model()
            prod_o.load_state_dict(sd_o)
            prod_o = prod_o.to(dev).eval()
            with torch.no_grad():
                with CodecTrace(ora_o.mv_compressor) as t_mv, CodecTrace(ora_o.residual_compressor) as t_res, CallLog(ora_o.masknet) as t_mask:
                    ref_hat_o, _, ref_bits_o = ora_o(xb, xc, xa, False)
                    traces_o = {"mv": t_mv.latents(get_scale_table()), "res": t_res.latents(get_scale_table()), "mask": t_mask.outputs[-1]}
                trace_o = {}
                gpu_hat_o, tot_o = prod_o.forward_device(frames[0], frames[mid], frames[2 * mid], trace=trace_o)
            po = parity_block(gpu_hat_o, float(tot_o.sum().item()), trace_o, ref_hat_o, float(ref_bits_o), traces_o)
            po["checkpoint"] = f"{other} (vcamd.seeding.{other}_state_dict, seed 1234)"
            po["quality_of_this_frame"] = {"psnr_db": float(vgop.psnr_uint8(ref_hat_o.to(dev), frames[mid], H, W)),
                                           "bpp_estimated": float(ref_bits_o) / (H * W),
                                           "residual_symbols_nonzero": float((traces_o["res"]["y_sym"] != 0).float().mean())}
            result[f"parity_vs_cpu_{other}"] = po


if __name__ == "__main__":
    main()
