"""Reference, seeded inputs and window builders of the deformable-convolution tests (tests/test_deform_cpu.py, tests/test_deform_gpu.py).

The reference is ``oracle.deform.deform_conv2d`` on float64 copies of the very float32 inputs; for the fused entry points the
preparation of ``oracle.icip2024.OffsetDiversity.prep`` (tanh * magnitude + flipped flow, sigmoid) is done in float64 too.  The
operator is continuous in the sampling position -- the bilinear weights go to zero at every validity boundary -- so the float64
result is a well-posed reference of the float32 kernels; ``dtype=torch.float32`` gives the restatement whose own distance from it
sizes the caps (pinned on the CPU by tests/test_deform_cpu.py).

A non-finite offset (or flow vector) makes its tap contribute nothing in the kernels (``py > -1 && py < H`` is false for NaN and
+-inf).  The oracle's arithmetic turns it into NaN * 0, so the reference is taken on inputs where such an offset is replaced by FAR,
a finite position outside every image: the tap then contributes exactly zero and the reference is finite everywhere.

Every tensor here is NCHW on the CPU.
"""
import torch

from oracle import deform as od

CAP_GENERIC = 2e-5          # |out - ref| / (1 + |ref|), the project's bound of vc_deform_conv2d (tests/test_icip2024_gpu.py)
CAP_FUSED = 5e-5            # ... of vc_offset_diversity and its half-feature forms
CAP_HALF_VS_F32 = 1e-6      # half-feature instance against the fp32 instance on features rounded to half beforehand
FAR = 1.0e6
SENTINEL = -12345.678
SIZES = [(9, 19), (3, 37)]  # no multiple of either pixel tile (8 x 8, 4 x 16), smaller than a tile in one direction
PAIRS = [(4, 2), (4, 4), (8, 4), (12, 6), (16, 8), (8, 8), (16, 4)]        # the (cg, og) switch of csrc/deform.hip: dispatch
TINY = [(1, 1), (1, 17)]
# (cg, og, groups) of the case table: the seven pairs at 8 groups; 20 and 32 groups (more than 8 per half: 1024-thread instances)
GENERIC_SHAPES = [(cg, og, 8) for cg, og in PAIRS] + [(8, 4, 20), (4, 2, 32)]
# ... and the record lengths 27 * groups / 2 of the fused entry: 216 (16 groups), 54 (4), 27 (2), 81 (6)
FUSED_SHAPES = [(cg, og, 8) for cg, og in PAIRS] + [(8, 4, 16), (8, 4, 4), (8, 4, 2), (8, 4, 6), (8, 4, 20), (4, 2, 32)]


def rel_err(out, ref):
    return ((out.double() - ref.double()).abs() / (1 + ref.double().abs())).max().item()


def _far(t):
    return torch.where(torch.isfinite(t), t, torch.full_like(t, FAR))


def _to(t, dtype):
    return None if t is None else t.to(dtype)


def ref_generic(x, off, wt, bias=None, mask=None, dtype=torch.float64):
    return od.deform_conv2d(_to(x, dtype), _far(_to(off, dtype)), _to(wt, dtype), _to(bias, dtype), padding=(1, 1), mask=_to(mask, dtype))


def prep(raw, flow, magnitude):
    """OffsetDiversity.prep of oracle/icip2024.py in the dtype of its inputs"""
    o1, o2, mask = torch.chunk(raw, 3, dim=1)
    offset = torch.tanh(torch.cat((o1, o2), dim=1)) * magnitude
    offset = offset + flow.flip(1).repeat(1, offset.size(1) // 2, 1, 1)
    return offset, torch.sigmoid(mask)


def ref_fused(x1, raw1, flow1, x2, raw2, flow2, magnitude, wt, bias=None, dtype=torch.float64, half_features=False):
    if half_features:
        x1, x2 = x1.half(), x2.half()
    o1, m1 = prep(_to(raw1, dtype), _far(_to(flow1, dtype)), magnitude)
    o2, m2 = prep(_to(raw2, dtype), _far(_to(flow2, dtype)), magnitude)
    return od.deform_conv2d(torch.cat((_to(x1, dtype), _to(x2, dtype)), 1), torch.cat((o1, o2), 1), _to(wt, dtype), _to(bias, dtype),
                            padding=(1, 1), mask=torch.cat((m1, m2), 1))


# ---- seeded inputs ----
def generic_inputs(cg, og, groups, h, w, n=2, seed=0):
    """offsets up to +-3 px: at these sizes about a third of the samples leave the image"""
    g = torch.Generator().manual_seed(1000 * cg + 100 * og + groups + 7 * h + seed)
    cin, cout = cg * groups, og * groups
    x = torch.randn(n, cin, h, w, generator=g)
    off = (torch.rand(n, groups * 18, h, w, generator=g) - 0.5) * 6
    msk = torch.rand(n, groups * 9, h, w, generator=g)
    wt = torch.randn(cout, cg, 3, 3, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    return x, off, msk, wt, b


FUSED_MAGNITUDE = 3.0


def fused_inputs(cg, og, groups, h, w, n=2, seed=0):
    """x1, raw1, flow1, x2, raw2, flow2, weight, bias: each reference carries groups / 2 groups of cg channels"""
    g = torch.Generator().manual_seed(2000 * cg + 100 * og + groups + 7 * h + seed)
    half = groups // 2
    c, cout = cg * half, og * groups
    x1, x2 = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g)
    r1, r2 = torch.randn(n, 27 * half, h, w, generator=g), torch.randn(n, 27 * half, h, w, generator=g)
    f1, f2 = torch.randn(n, 2, h, w, generator=g) * 1.5, torch.randn(n, 2, h, w, generator=g) * 1.5
    if h * w > 1:
        f1[0, :, 0, 0] = float("inf")                       # broken flow vectors: every tap of that reference at that pixel contributes nothing
        f2[n - 1, 0, h - 1, w // 2] = float("nan")
    wt =torch.randn(cout, cg, 3, 3, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    return x1, r1, f1, x2, r2, f2, wt, b


# ---- exact sampling boundaries (generic entry) ----
EPS = 2.0 ** -10


def boundary_values(size):
    """the positions of one axis of length ``size`` at which the sampling rule changes, all exact in float32"""
    return [-1.0, -1.0 + EPS, -0.5, 0.0, 0.5, size - 1.0, size - 1.0 + EPS, size - 0.5, float(size)]


def boundary_inputs(cg, og, groups, h, w, n=2, seed=0):
    """generic_inputs whose offsets are overwritten at chosen (image, group, tap, pixel) slots so that the sampling position
    (py, px) = (y - 1 + k // 3 + dy, x - 1 + k % 3 + dx) is EXACTLY a boundary value: dy = target - base is a small multiple of
    2^-10, so offset and position are exact in float32 and float64 alike and both precisions take the same branch.
    Returns (inputs..., slots, dead): ``slots`` = [(i, g, k, y, x, py, px)] of the crafted taps, ``dead`` = [(i, y, x)] of pixels whose
    nine taps of every group lie outside the image (output == bias exactly), and a NaN, a +inf and a -inf offset on top."""
    x, off, msk, wt, b = generic_inputs(cg, og, groups, h, w, n, seed)
    o = off.view(n, groups, 9, 2, h, w)
    ys, xs = boundary_values(h), boundary_values(w)
    inner_y = [0.25 * j for j in range(0, 4 * (h - 1) + 1)]          # exact interior positions for the other coordinate
    inner_x = [0.125 * j for j in range(0, 8 * (w - 1) + 1)]
    targets = [(py, inner_x[(5 * j + 3) % len(inner_x)]) for j, py in enumerate(ys)]
    targets += [(inner_y[(7 * j + 2) % len(inner_y)], px) for j, px in enumerate(xs)]
    corner_y = [-1.0, -1.0 + EPS, 0.0, h - 1.0, h - 1.0 + EPS, float(h)]
    corner_x = [-1.0, -1.0 + EPS, 0.0, w - 1.0, w - 1.0 + EPS, float(w)]
    targets += [(py, px) for py in corner_y for px in corner_x]                     # both coordinates at once, the four corners
    slots = []
    j = 0
    for rep in range(4):                                   # every target at four different slots (other pixels, taps, groups)
        for py, px in targets:
            i, g, k = j % n, (3 * j + rep) % groups, (2 * j + rep) % 9
            y, xx = (5 * j + rep) % h, (11 * j + 3 * rep) % w
            if (i, y, xx) in {(0, 1, 2), (1, h - 1, w - 1), (1, 0, 0)}:            # (the dead pixels below)
                xx = (xx + 3) % w
            o[i, g, k, 0, y, xx] = py - (y - 1 + k // 3)
            o[i, g, k, 1, y, xx] = px - (xx - 1 + k % 3)
            slots.append((i, g, k, y, xx, py, px))
            j += 1
    dead = [(0, 1, 2), (1, h - 1, w - 1), (1, 0, 0)]
    outside = [(-1.0, 0.5), (float(h), 1.0), (0.5, -1.0), (1.0, float(w)), (-1.0, -1.0), (float(h), float(w)), (-3.0, 0.0), (0.0, w + 2.5),
               (-1.0, float(w))]
    for i, y, xx in dead:
        for g in range(groups):
            for k in range(9):
                py, px = outside[(g + k) % len(outside)]
                o[i, g, k, 0, y, xx] = py - (y - 1 + k // 3)
                o[i, g, k, 1, y, xx] = px - (xx - 1 + k % 3)
    # non-finite offsets: the tap contributes nothing (and a dead pixel stays dead with them)
    o[0, 0, 4, 0, 2, 5] = float("nan")
    o[1, groups - 1, 0, 1, 0, 7] = float("inf")
    o[0, 1, 8, 0, h - 1, 3] = float("-inf")
    o[0, 0, 0, 1, 1, 2] = float("nan")
    return x, off, msk, wt, b, slots, dead


def corner_validity(off, h, w, dtype):
    """(py, px, inside, tl, tr, bl, br) of every tap in ``dtype``: the decisions of torchvision's bilinear_interpolate as
    oracle/deform.py and the kernel take them.  off: [n, G * 18, h, w]."""
    n = off.shape[0]
    groups = off.shape[1] // 18
    o = off.to(dtype).view(n, groups, 9, 2, h, w)
    k = torch.arange(9)
    by = (torch.arange(h, dtype=dtype).view(1, 1, 1, h, 1) - 1) + (k // 3).to(dtype).view(1, 1, 9, 1, 1)
    bx = (torch.arange(w, dtype=dtype).view(1, 1, 1, 1, w) - 1) + (k % 3).to(dtype).view(1, 1, 9, 1, 1)
    py, px = by + o[:, :, :, 0], bx + o[:, :, :, 1]
    inside = (py > -1) & (py < h) & (px > -1) & (px < w)
    y0, x0 = torch.floor(py), torch.floor(px)
    t, b_, l, r = y0 >= 0, y0 + 1 <= h - 1, x0 >= 0, x0 + 1 <= w - 1
    return py, px, inside, inside & t & l, inside & t & r, inside & b_ & l, inside & b_ & r


# ---- device windows ----
def place(x, dev, c0=0, cpad=0, hpad=0, wpad=0, n0=0, npad=0, fill=None, half=False, seed=0):
    """An NCHW CPU tensor as a channels-last device window: channels [c0, c0 + c) of a buffer cpad channels wider, the top-left crop
    of a buffer hpad rows / wpad columns larger, images [n0, n0 + n) of a buffer npad images longer.  What lies outside the window
    holds ``fill`` (default: seeded values around 1e3, which a stray read turns into a visible error).  Returns the vcamd.hip.T."""
    from vcamd import hip
    n, c, h, w = x.shape
    N, H, W, C = n + npad, h + hpad, w + wpad, c + cpad
    if fill is None:
        big = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(99 + seed)) * 1e3
    else:
        big = torch.full((N, H, W, C), float(fill))
    big[n0:n0 + n, :h, :w, c0:c0 + c] = x.permute(0, 2, 3, 1).float()
    buf = big.to(torch.float16 if half else torch.float32).flatten().to(dev)
    t = hip.T(buf, N, H, W, C, H * W * C, W * C, C, 0, "f16" if half else "f32")
    return t.images(n0, n0 + n).crop(h, w).channels(c0, c0 + c)


def read_window(t):
    """(window as NCHW CPU tensor, the buffer's elements OUTSIDE the window as a flat CPU tensor) of a float32 window made by place()"""
    full = t.buf.cpu()
    e = full.numel() // t.sn                       # images of the buffer (a window never changes sn / sh / sw)
    rows = t.sn // t.sh
    cols = t.sh // t.sw
    v = full.view(e, rows, cols, t.sw)
    n0 = t.off // t.sn
    c0 = t.off % t.sw
    win = v[n0:n0 + t.n, :t.h, :t.w, c0:c0 + t.c]
    keep = torch.ones_like(v, dtype=torch.bool)
    keep[n0:n0 + t.n, :t.h, :t.w, c0:c0 + t.c] = False
    return win.permute(0, 3, 1, 2).contiguous(), v[keep]


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_untouched(outside):
    want = torch.full_like(outside, SENTINEL)
    assert torch.equal(bits(outside), bits(want)), f"{(bits(outside) != bits(want)).sum().item()} elements outside the output window were written"
