"""References, inputs and case tables of the element-wise kernel tests (tests/test_ew_cpu.py, tests/test_ew_gpu.py): the per-pixel
kernels of csrc/ew_kernels.hip (and vc_split3 of csrc/conv_split.hip) that produce the prediction, the residual and the half or
split features everything downstream codes.

Every reference restates the reference project's formula at the call site include/vc_hip.h cites, in float64 on float64 copies of
the very float32 inputs, from elementary arithmetic: the logistic as 1 / (1 + exp(-b)), rounding half to even from floor, the clamp
from two comparisons, the half conversion through numpy, the layouts as index permutations.  tests/test_ew_cpu.py pins each against
the torch operator the reference calls (torch.sigmoid, torch.round, .half(), torch.clamp, permute).  ``F32`` holds the same
operations as the fp32 torch expressions the reference project runs: what the exact kernels are compared with bit for bit, and what
test_ew_cpu.py holds inside the bounds so that a bound a kernel misses is the kernel's fault.

Bounds, u = 2^-24, |out - ref| <= k u M with M the magnitude of the terms in float64 (never 1 + |ref|):
  k = 8   vc_lhbdc_blend pred   M = |m fw| + |(1 - m) bw|                 (1 - m, two products, one sum: four roundings)
          vc_lhbdc_blend resid  M = M(pred) + |cur|
          vc_flex_motion_split  M = |k_a F01| + |k_b F10|                 (1 - t, coefficient, product, sum)
          vc_spynet_preprocess  M = (|x| + mean) / std                    (two rounded constants, difference, quotient)
  k = 16  vc_flex_blend pred    M = (|w1 xb| + |w2 xa|) / (w1 + w2 + 1e-8f)  (two products, sum, two sums below, quotient)
          vc_flex_blend resid   M = M(pred) + |cur|
          vc_attention_gate     M = |a| + |identity|                      (expf to 1 ulp, 1 + e, reciprocal, product, sum)
Everything else is exact.  Nothing here touches the GPU.
"""
import functools

import numpy as np
import torch

from resample_ref import (DENSE, NS, SENTINEL, SIZES, TINY, WIN_A, WIN_U, assert_untouched, bits, geom, place, rand,  # noqa: F401
                          read_window, rel_err, rowmap, split_host, unsplit)

F64 = torch.float64
U = 2.0 ** -24
K_TIGHT, K_WIDE = 8.0, 16.0
FLEX_EPS = float(np.float32(1e-8))          # the constant as the reference's fp32 tensor arithmetic sees it
MEANS = (0.406, 0.456, 0.485)               # flow.py:40-42, by INPUT channel (blue, green, red statistics)
STDS = (0.225, 0.224, 0.229)
ENTRY_POINTS = ["vc_lhbdc_blend", "vc_blend", "vc_flex_blend", "vc_flex_motion_split", "vc_attention_gate", "vc_quantize_mask",
                "vc_channel_scale", "vc_clamp01", "vc_to_half", "vc_to_half_planar", "vc_nchw_to_nhwc", "vc_nhwc_to_nchw",
                "vc_spynet_preprocess", "vc_split3", "vc_split3_pad"]
BOUND = {"vc_lhbdc_blend": K_TIGHT, "vc_blend": K_TIGHT, "vc_flex_motion_split": K_TIGHT, "vc_spynet_preprocess": K_TIGHT,
         "vc_flex_blend": K_WIDE, "vc_attention_gate": K_WIDE}


def units(out, ref, mag):
    """the largest |out - ref| / (u M); where M == 0 the result has to be the reference itself (inf otherwise)"""
    d = (out.double() - ref.double()).abs()
    mag = mag.double().expand_as(d)
    q = torch.where(mag > 0, d / (U * mag.clamp_min(1e-300)), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))))
    return q.max().item() if q.numel() else 0.0


# ------------------------------------------------------------------------------------------------
# references (NCHW, float64 unless stated)
# ------------------------------------------------------------------------------------------------
def sigmoid(b):
    return 1.0 / (1.0 + torch.exp(-b.to(F64)))


def round_half_even(x):
    """float64, ties to the even neighbour, the sign of a zero result is the argument's"""
    x = x.to(F64)
    r = torch.floor(x)
    d = x - r
    up = (d > 0.5) | ((d == 0.5) & (torch.remainder(r, 2) == 1))
    return torch.copysign(r + up.to(F64), x)


def clamp01(x):
    """two comparisons: a value that is neither below 0 nor above 1 passes as it is (-0.0 stays -0.0, as torch.clamp leaves it)"""
    return torch.where(x < 0, torch.zeros_like(x), torch.where(x > 1, torch.ones_like(x), x))


def lhbdc_blend(fw, bw, m, cur=None):
    """LHBDC m.py:63-67 -> pred, resid, M(pred), M(resid)"""
    fw, bw, m = fw.to(F64), bw.to(F64), m.to(F64)
    pred = m * fw + (1.0 - m) * bw
    mag = (m * fw).abs() + ((1.0 - m) * bw).abs()
    if cur is None:
        return pred, None, mag, None
    return pred, cur.to(F64) - pred, mag, mag + cur.to(F64).abs()


def flex_blend(xb, xa, mask, cur=None):
    """Flex b_model.py:70-73"""
    xb, xa, mask = xb.to(F64), xa.to(F64), mask.to(F64)
    w1, w2 = 0.5 * mask[:, 0:1], 0.5 * mask[:, 1:2]
    den = w1 + w2 + FLEX_EPS
    pred = (w1 * xb + w2 * xa) / den
    mag = ((w1 * xb).abs() + (w2 * xa).abs()) / den
    if cur is None:
        return pred, None, mag, None
    return pred, cur.to(F64) - pred, mag, mag + cur.to(F64).abs()


def motion_split(flow4, t):
    """Flex b_model.py:38-40; t is the fp32 number the entry point receives -> ft0, ft1, M0, M1"""
    f, t = flow4.to(F64), float(np.float32(t))
    f01, f10 = f[:, 0:2], f[:, 2:4]
    a0, b0 = -(1 - t) * t * f01, t * t * f10
    a1, b1 = (1 - t) * (1 - t) * f01, t * (1 - t) * f10
    return a0 + b0, a1 - b1, a0.abs() + b0.abs(), a1.abs() + b1.abs()


def attention_gate(a, b, identity):
    """compressai AttentionBlock (ICIP2024 elic.py:97-121): out = a * sigmoid(b) + identity -> out, M"""
    return a.to(F64) * sigmoid(b) + identity.to(F64), a.to(F64).abs() + identity.to(F64).abs()


def keep_mask(h, w, keep_parity):
    yx = torch.arange(h).view(h, 1) + torch.arange(w).view(1, w)
    return torch.ones(h, w, dtype=torch.bool) if keep_parity < 0 else (yx % 2 == keep_parity)


def quantize_mask(x, gain, keep_parity, do_round):
    """ICIP2024 compression_bottlenecks.py:237-246,268-269: round, THEN the gain, +0.0 at the positions that are not kept"""
    v = round_half_even(x) if do_round else x.to(F64)
    if gain is not None:
        v = v * gain.to(F64).view(1, -1, 1, 1)
    return torch.where(keep_mask(x.shape[2], x.shape[3], keep_parity), v, torch.zeros_like(v))


def channel_scale(x, gain):
    """Flex b_model/layers.py:54-73"""
    return gain.to(F64).view(1, -1, 1, 1) * x.to(F64)


def spynet_preprocess(x):
    """LHBDC flow.py:39-45 -> out (red, green, blue statistics order: input channel 2 first), M"""
    x = x.to(F64)
    ch = [(x[:, i:i + 1] - MEANS[i]) / STDS[i] for i in range(3)]
    mg = [(x[:, i:i + 1].abs() + MEANS[i]) / STDS[i] for i in range(3)]
    return torch.cat(ch[::-1], 1), torch.cat(mg[::-1], 1)


def to_nhwc(x):
    n, c, h, w = x.shape
    out = torch.empty(n, h, w, c, dtype=x.dtype)
    for k in range(c):
        out[..., k] = x[:, k]
    return out


def to_half(x):
    """dense [n][h][w][c] halves, as int16 bits"""
    return torch.from_numpy(to_nhwc(x).numpy().astype(np.float16).view(np.int16).copy())


def to_half_planar(x, cg):
    """[n][c / cg][h][w][cg] halves, as int16 bits"""
    n, c, h, w = x.shape
    planes = [to_nhwc(x[:, g * cg:(g + 1) * cg]) for g in range(c // cg)]
    return torch.from_numpy(torch.stack(planes, 1).numpy().astype(np.float16).view(np.int16).copy())


def split_pad_host(x, c_out):
    """the dense split tensor of x padded with +0.0 channels to c_out"""
    n, c, h, w = x.shape
    return split_host(torch.cat((x, torch.zeros(n, c_out - c, h, w)), 1))


def pieces(buf, n, c, h, w):
    """dense split tensor -> the three fp32 pieces [3][n][c][h][w]"""
    raw = np.frombuffer(buf.detach().cpu().contiguous().numpy().tobytes(), dtype="<u2")
    p = (raw.astype(np.uint32) << 16).view(np.float32).reshape(n, c // 8, h, w, 3, 8)
    return torch.from_numpy(p.transpose(4, 0, 1, 5, 2, 3).reshape(3, n, c, h, w).copy())


class F32:
    """the fp32 torch expressions of the reference project, on the CPU"""

    @staticmethod
    def lhbdc_blend(fw, bw, m, cur):
        pred = m * fw + (1.0 - m) * bw
        return pred, cur - pred

    @staticmethod
    def flex_blend(xb, xa, mask, cur):
        w1, w2 = 0.5 * mask[:, 0:1], 0.5 * mask[:, 1:2]
        pred = (w1 * xb + w2 * xa) / (w1 + w2 + 1e-8)
        return pred, cur - pred

    @staticmethod
    def motion_split(f, t):
        t = float(np.float32(t))
        f01, f10 = f[:, :2], f[:, 2:4]
        return -(1 - t) * t * f01 + t * t * f10, (1 - t) * (1 - t) * f01 - t * (1 - t) * f10

    @staticmethod
    def attention_gate(a, b, identity):
        return a * torch.sigmoid(b) + identity

    @staticmethod
    def quantize_mask(x, gain, keep_parity, do_round):
        v = torch.round(x) if do_round else x.clone()
        if gain is not None:
            v = v * gain.view(1, -1, 1, 1)
        if keep_parity >= 0:          # y_half[:, :, 0::2, 0::2] = 0; y_half[:, :, 1::2, 1::2] = 0 removes parity 0
            p = 1 - keep_parity
            v[:, :, 0::2, p::2] = 0
            v[:, :, 1::2, (1 - p)::2] = 0
        return v

    @staticmethod
    def channel_scale(x, gain):
        return gain.view(1, -1, 1, 1) * x

    @staticmethod
    def clamp01(x):
        return torch.clamp(x, 0, 1)

    @staticmethod
    def spynet_preprocess(x):
        blue, green, red = (x[:, 0:1] - 0.406) / 0.225, (x[:, 1:2] - 0.456) / 0.224, (x[:, 2:3] - 0.485) / 0.229
        return torch.cat([red, green, blue], 1)

    @staticmethod
    def to_half(x):
        return x.half().permute(0, 2, 3, 1).contiguous().view(torch.int16)

    @staticmethod
    def to_half_planar(x, cg):
        n, c, h, w = x.shape
        return x.half().view(n, c // cg, cg, h, w).permute(0, 1, 3, 4, 2).contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------
# shapes, views, row-map cases
# ------------------------------------------------------------------------------------------------
N = 2
SHAPES = SIZES + TINY
SPECS = [DENSE, WIN_A, WIN_U]
# a second 16-byte aligned window for the entry points that ask alignment of their input (half copies, vc_split3)
WIN_B = dict(c0=8, cpad=12, hpad=1, wpad=3, n0=1, npad=1)
ALIGNED = [DENSE, WIN_A, WIN_B]
VIEWSETS = ["dense", "rot0", "rot1", "rot2"]


def specs_of(viewset, count, table=SPECS):
    """argument i of `count` gets DENSE under "dense" and table[(i + j) % 3] under "rot<j>": over the three rotations every argument
    is a dense view, a channel slice and crop, and a window at an unaligned element offset"""
    if viewset == "dense":
        return [DENSE] * count
    j = int(viewset[3:])
    return [table[(i + j) % len(table)] for i in range(count)]


def _rm(ident, entry, n, c, h, w, per_px, regime, **kw):
    return NS(id=f"{entry}-{ident}", entry=entry, n=n, c=c, h=h, w=w, per_px=per_px, regime=regime, **kw)


# the kernels launched through VC_EW_LAUNCH and the work items per pixel each hands the row map.  "wide": several workgroups a row
# (w * per_px > 256, no multiple of it); "fallback": 65536 images or rows, the 64-bit linear index
ROWMAP_CASES = [  # (id, entry, n, c, h, w, work items per pixel, regime); the half copies take 4 channels (cg = 4: one group) per item
    _rm("wide", "vc_lhbdc_blend", 2, 3, 3, 87, 3, "wide"),
    _rm("n65536", "vc_lhbdc_blend", 65536, 3, 2, 3, 3, "fallback"),
    _rm("wide", "vc_flex_blend", 2, 3, 3, 87, 3, "wide"),
    _rm("h65536", "vc_flex_blend", 1, 3, 65536, 2, 3, "fallback"),
    _rm("wide", "vc_attention_gate", 2, 8, 3, 37, 8, "wide"),
    _rm("n65536", "vc_attention_gate", 65536, 5, 2, 3, 5, "fallback"),
    _rm("wide", "vc_quantize_mask", 2, 8, 3, 37, 8, "wide"),
    _rm("h65536", "vc_quantize_mask", 1, 5, 65536, 2, 5, "fallback"),
    _rm("wide", "vc_channel_scale", 2, 8, 3, 37, 8, "wide"),
    _rm("h65536", "vc_channel_scale", 1, 5, 65536, 2, 5, "fallback"),
    _rm("wide", "vc_clamp01", 2, 8, 3, 37, 8, "wide"),
    _rm("n65536", "vc_clamp01", 65536, 5, 2, 3, 5, "fallback"),
    _rm("wide", "vc_to_half", 2, 32, 3, 37, 8, "wide"),
    _rm("n65536", "vc_to_half", 65536, 4, 2, 3, 1, "fallback"),
    _rm("wide", "vc_to_half_planar", 2, 32, 3, 37, 8, "wide", cg=4),
    _rm("h65536", "vc_to_half_planar", 1, 8, 65536, 2, 2, "fallback", cg=4),
]
# the row loop, one representative: n = 64, 270 work items a row = 2 workgroups -> gridDim.y = 64 < h = 70 (resample_ref.AXPBY_ROWLOOP)
ROWLOOP = _rm("rowloop", "vc_clamp01", 64, 5, 70, 54, 5, "loop")

BLEND_LARGER = (2, 7, 10)           # n, h, w of the inputs whose top-left 5 x 7 a blend reads
PLANAR_CG = [4, 8, 12, 16]
LAYOUT_C = [1, 3, 5, 8]
SPLIT_PAD_C = [(1, 8), (3, 8), (6, 8), (9, 16), (13, 16), (6, 16)]
SPLIT_SPECIALS = [0.0, -0.0, 1e-30, -3e38, 2.0 ** -120, 1.0 + 2.0 ** -23, -(2.0 - 2.0 ** -23), 1.0]


# ------------------------------------------------------------------------------------------------
# inputs: seeded, with the edges of the arithmetic written over the first positions and cycled over the whole tensor in "edge" mode
# ------------------------------------------------------------------------------------------------
def _seed(*k):
    return 700000 + sum(int(v) * m for v, m in zip(k, (1, 37, 1009, 7, 100003)))


def _cycle(values, shape, stride=1):
    """values repeated over a tensor of `shape` in memory order, each held for `stride` elements"""
    count = int(np.prod(shape))
    idx = (torch.arange(count) // stride) % len(values)
    return torch.tensor(values, dtype=torch.float32)[idx].view(shape)


MASK_EDGES = [0.0, 1.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 0.25]


@functools.lru_cache(maxsize=None)
def lhbdc_inputs(n, h, w, edge=False):
    """frames of mixed sign in [-1, 1], a mask in [0, 1], the current frame in [0, 1].  edge: the mask walks through exactly 0,
    exactly 1, 2^-24, ...; in the second image cur == fw == bw, so the prediction is the frame and the residual (nearly) zero"""
    fw, bw = rand((n, 3, h, w), _seed(h, w, n, 1), -1, 1), rand((n, 3, h, w), _seed(h, w, n, 2), -1, 1)
    m, cur = rand((n, 1, h, w), _seed(h, w, n, 3)), rand((n, 3, h, w), _seed(h, w, n, 4))
    if edge:
        m = _cycle(MASK_EDGES, (n, 1, h, w))
        bw[n - 1] = fw[n - 1]
        cur[n - 1] = fw[n - 1]
    return fw, bw, m, cur


_HALF_UP = float(np.nextafter(np.float32(0.5), np.float32(1)))
FLEX_MASK_EDGES = [(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1e-7, 1e-7), (0.5, _HALF_UP), (_HALF_UP, 0.5), (1.0, 1.0), (1e-7, 0.0), (0.3, 0.9)]


@functools.lru_cache(maxsize=None)
def flex_inputs(n, h, w, edge=False):
    xb, xa = rand((n, 3, h, w), _seed(h, w, n, 5), -1, 1), rand((n, 3, h, w), _seed(h, w, n, 6), -1, 1)
    mask, cur = rand((n, 2, h, w), _seed(h, w, n, 7)), rand((n, 3, h, w), _seed(h, w, n, 8))
    if edge:
        mask = torch.stack((_cycle([p[0] for p in FLEX_MASK_EDGES], (n, h, w)), _cycle([p[1] for p in FLEX_MASK_EDGES], (n, h, w))), 1)
    return xb, xa, mask, cur


MOTION_T = [0.5, 0.0, 1.0, 0.3]


@functools.lru_cache(maxsize=None)
def motion_inputs(n, h, w, c=4):
    return rand((n, c, h, w), _seed(h, w, n, 9), -3, 3)


GATE_B_EDGES = [0.0, 1e-4, -1e-4, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0]


@functools.lru_cache(maxsize=None)
def gate_inputs(n, c, h, w, edge=False):
    """edge: b walks through the list (at -104 the gate underflows to 0); a == 0 in the first image: there the identity alone
    carries the value"""
    a, b = rand((n, c, h, w), _seed(h, w, n, 10, c), -2, 2), rand((n, c, h, w), _seed(h, w, n, 11, c), -6, 6)
    identity = rand((n, c, h, w), _seed(h, w, n, 12, c), -2, 2)
    if edge:
        b = _cycle(GATE_B_EDGES, (n, c, h, w))
        a[0] = 0.0
    return a, b, identity


QUANT_EDGES = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 2.0 ** 23 + 1, -0.0, 0.0, 0.49999997, -3.5, 1e-30]


@functools.lru_cache(maxsize=None)
def quant_inputs(n, c, h, w, edge=False):
    """values of a few units; a gain in [0.5, 1.5) that is no power of two (rounding after the gain gives other integers)"""
    x = rand((n, c, h, w), _seed(h, w, n, 13, c), -4, 4)
    if edge:
        x = torch.where(_cycle([1.0, 0.0], (n, c, h, w), 7) > 0, _cycle(QUANT_EDGES, (n, c, h, w)), x)
    return x, rand((c,), _seed(c, 14), 0.5, 1.5)


_ONE_UP, _ONE_DOWN = float(np.nextafter(np.float32(1), np.float32(2))), float(np.nextafter(np.float32(1), np.float32(0)))
CLAMP_EDGES = [-0.0, 0.0, 1.0, _ONE_UP, _ONE_DOWN, float("inf"), float("-inf"), 1e-40, -1e-40, 2.0 ** -149, -2.5, 0.5, 7.0]


@functools.lru_cache(maxsize=None)
def clamp_inputs(n, c, h, w, edge=False):
    x = rand((n, c, h, w), _seed(h, w, n, 15, c), -1, 2)
    return _cycle(CLAMP_EDGES, (n, c, h, w)) if edge else x


HALF_EDGES = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65504.0, 65520.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 0.0, -0.0, -(1 + 2.0 ** -11), -65520.0,
              3 * 2.0 ** -25, -2.0 ** -25, 2.0 ** -14 - 2.0 ** -25, 65519.0]


@functools.lru_cache(maxsize=None)
def half_inputs(n, c, h, w, edge=False):
    x = rand((n, c, h, w), _seed(h, w, n, 16, c), -3, 3)
    return _cycle(HALF_EDGES, (n, c, h, w)) if edge else x


def distinct(n, c, h, w):
    """every element another value, exact in fp32"""
    return torch.arange(n * c * h * w, dtype=torch.float32).view(n, c, h, w) * 0.25 - 3.0


@functools.lru_cache(maxsize=None)
def spynet_inputs(n, h, w, edge=False):
    """the three channels carry distinct values; edge: 0, 1 and each channel's own mean (as fp32) at walking positions"""
    x = rand((n, 3, h, w), _seed(h, w, n, 17))
    if edge:
        for i in range(3):
            x[:, i] = _cycle([0.0, 1.0, float(np.float32(MEANS[i])), 0.1 * (i + 1)], (n, h, w))
    return x


@functools.lru_cache(maxsize=None)
def split_inputs(n, c, h, w, edge=False):
    x = rand((n, c, h, w), _seed(h, w, n, 18, c), -2, 2) * 1e3 ** rand((n, c, h, w), _seed(h, w, n, 19, c), -1, 1)
    return _cycle(SPLIT_SPECIALS, (n, c, h, w)) if edge else x


# ------------------------------------------------------------------------------------------------
# coverage: the tests of tests/test_ew_gpu.py that run each entry point dense, on windows, on the edges of its arithmetic and
# against its argument contract (tests/test_ew_cpu.py asserts the table is complete and names tests that exist)
# ------------------------------------------------------------------------------------------------
def _cov(views, edge, contract):
    return {"dense": views, "window": views, "edge": edge, "contract": contract}


COVERAGE = {
    "vc_lhbdc_blend": _cov("test_lhbdc_blend_views", "test_lhbdc_blend_edges", "test_blend_contract"),
    "vc_blend": _cov("test_lhbdc_blend_views", "test_lhbdc_blend_edges", "test_blend_contract"),
    "vc_flex_blend": _cov("test_flex_blend_views", "test_flex_blend_edges", "test_blend_contract"),
    "vc_flex_motion_split": _cov("test_motion_split_views", "test_motion_split_views", "test_motion_split_contract"),
    "vc_attention_gate": _cov("test_attention_gate_views", "test_attention_gate_edges", "test_attention_gate_contract"),
    "vc_quantize_mask": _cov("test_quantize_mask_views", "test_quantize_mask_edges", "test_quantize_mask_contract"),
    "vc_channel_scale": _cov("test_channel_scale_views", "test_channel_scale_views", "test_clamp_and_scale_contract"),
    "vc_clamp01": _cov("test_clamp01_views", "test_clamp01_edges", "test_clamp_and_scale_contract"),
    "vc_to_half": _cov("test_to_half_views", "test_to_half_edges", "test_half_copies_contract"),
    "vc_to_half_planar": _cov("test_to_half_planar_views", "test_to_half_edges", "test_half_copies_contract"),
    "vc_nchw_to_nhwc": _cov("test_layouts_one_direction_at_a_time", "test_layouts_one_direction_at_a_time", "test_layout_and_preprocess_contract"),
    "vc_nhwc_to_nchw": _cov("test_layouts_one_direction_at_a_time", "test_layouts_one_direction_at_a_time", "test_layout_and_preprocess_contract"),
    "vc_spynet_preprocess": _cov("test_spynet_preprocess_views", "test_spynet_preprocess_views", "test_layout_and_preprocess_contract"),
    "vc_split3": _cov("test_split3_views", "test_split3_views", "test_split_contract"),
    "vc_split3_pad": _cov("test_split3_pad_views", "test_split3_pad_views", "test_split_contract"),
}
