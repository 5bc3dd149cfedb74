"""References, case tables and dispatch predicates of the resampling / pooling / warping tests (tests/test_resample_cpu.py,
tests/test_resample_gpu.py): the kernels of csrc/ew_kernels.hip whose index arithmetic and interpolation can go wrong.

Every reference is the torch operator the reference project calls at that site, evaluated in float64 on float64 copies of the very
float32 inputs, with the grid recipe restated in float64; ``dtype=torch.float32`` gives the restatement whose own distance from it is
pinned below the caps by tests/test_resample_cpu.py.  The operators are continuous in the sampling position (bilinear weights go to
zero at every validity boundary), so the float64 result is a well-posed reference of a float32 kernel.

Caps (the project's own, tests/test_ops_gpu.py): warping and the warped channels of the level input 2e-5, everything linear 1e-6,
both as |out - ref| / (1 + |ref|); max pooling exact.  The inputs are chosen so that the caps mean something: images uniform in
[0, 1], displacements of a few pixels plus the deliberate border cases, and -- because an fp32 source coordinate that is not exact
carries an error of half an ulp of the coordinate -- inexact up-sampling scales (align_corners, factor 3) only on inputs of at most
8 pixels a side and smooth coarse flows for the level input.

A window is described by the keyword arguments of deform_ref.place; ``geom`` restates the view place makes of them on a 16-byte
aligned buffer, and the ``*_form`` predicates restate the host-side dispatch of csrc/ew_kernels.hip on such views.  Nothing here
touches the GPU.
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from deform_ref import SENTINEL, assert_untouched, bits, place, read_window, rel_err  # noqa: F401  (used through this module)

CAP_WARP = 2e-5
CAP_LINEAR = 1e-6
EW_BLOCK = 256              # csrc/ew_rowmap.h
SIZES = [(9, 19), (3, 37)]  # no multiple of anything; one fits a wave, one is wider than it is high
TINY = [(1, 1), (1, 17), (9, 1)]
F64 = torch.float64


def NS(**kw):
    return types.SimpleNamespace(**kw)


def rand(shape, seed, lo=0.0, hi=1.0):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def warp(convention, img, flow, dtype=F64):
    """W1 LHBDC flow.py:15-25, W2 Flex b_model.py:99-112, W3 ICIP2024 m.py:262-282; image and flow of the same height and width"""
    img, flow = img.to(dtype), flow.to(dtype)
    _, _, h, w = flow.shape
    if convention == 2:
        x = torch.arange(w, dtype=dtype).view(1, 1, w) + flow[:, 0]
        y = torch.arange(h, dtype=dtype).view(1, h, 1) + flow[:, 1]
        grid = torch.stack((2 * (x / w - 0.5), 2 * (y / h - 0.5)), dim=3)
        return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    if convention == 1:
        gx, gy = torch.linspace(-1 + 1 / w, 1 - 1 / w, w, dtype=dtype), torch.linspace(-1 + 1 / h, 1 - 1 / h, h, dtype=dtype)
    else:
        gx, gy = torch.linspace(-1, 1, w, dtype=dtype), torch.linspace(-1, 1, h, dtype=dtype)
    x = gx.view(1, 1, w) + flow[:, 0] / ((w - 1) / 2)
    y = gy.view(1, h, 1) + flow[:, 1] / ((h - 1) / 2)
    return F.grid_sample(img, torch.stack((x, y), dim=3), mode="bilinear", padding_mode="border", align_corners=convention == 3)


def upsample(x, factor, align_corners, scale, dtype=F64):
    return scale * F.interpolate(x.to(dtype), scale_factor=factor, mode="bilinear", align_corners=align_corners)


def avgpool_reflectpad(x, k, scale, oh, ow, dtype=F64):
    y = x.to(dtype) * scale
    if k > 1:
        y = F.avg_pool2d(y, k)
    if (oh, ow) != tuple(y.shape[2:]):
        y = F.pad(y, (0, ow - y.shape[3], 0, oh - y.shape[2]), mode="reflect")
    return y


def maxpool2(x):
    return F.max_pool2d(x, 2, 2)


def axpby(a, b, alpha, beta, dtype=F64):
    v = alpha * a.to(dtype)
    return v if b is None else v + beta * b.to(dtype)


def level_input(first, second, flow_coarse, dtype=F64):
    """LHBDC flow.py:90-98 -> (feat [n, 8, h, w], up [n, 2, h, w])"""
    n, _, h, w = first.shape
    if flow_coarse is None:
        up = torch.zeros(n, 2, h, w, dtype=dtype)
    else:
        up = 2 * F.interpolate(flow_coarse.to(dtype), scale_factor=2, mode="bilinear", align_corners=True)
        if up.shape[2] != h:
            up = F.pad(up, (0, 0, 0, 1), mode="replicate")
        if up.shape[3] != w:
            up = F.pad(up, (0, 1, 0, 0), mode="replicate")
    return torch.cat((first.to(dtype), warp(1, second, up, dtype), up), 1), up


def unsplit(buf, n, c, h, w):
    """dense split tensor [n][c / 8][h][w][3][8] (three bf16 pieces hi, mid, lo per value, little-endian 2-byte elements) ->
    float64 NCHW, the exact sum of the pieces"""
    raw = np.frombuffer(buf.detach().cpu().contiguous().numpy().tobytes(), dtype="<u2")
    assert raw.size == n * c * h * w * 3, (raw.size, n, c, h, w)
    pieces = (raw.astype(np.uint32) << 16).view(np.float32).astype(np.float64).reshape(n, c // 8, h, w, 3, 8)
    return torch.from_numpy(pieces.sum(axis=4).transpose(0, 1, 4, 2, 3).reshape(n, c, h, w).copy())


def split_host(x):
    """float32 NCHW (c % 8 == 0) -> the int16 buffer of its dense split tensor: vc_split3 of csrc/common.h on the host"""
    n, c, h, w = x.shape
    v = x.permute(0, 2, 3, 1).reshape(n, h, w, c // 8, 8).permute(0, 3, 1, 2, 4).contiguous().numpy().astype(np.float32)
    hi = (v.view(np.uint32) & 0xffff0000).view(np.float32)
    r1 = v - hi
    mid = (r1.view(np.uint32) & 0xffff0000).view(np.float32)
    lo = r1 - mid
    rec = np.stack([(p.view(np.uint32) >> 16).astype("<u2") for p in (hi, mid, lo)], axis=4)          # [n][c/8][h][w][3][8]
    return torch.from_numpy(rec.view(np.int16).reshape(-1).copy())


# ------------------------------------------------------------------------------------------------
# views and dispatch, restated
# ------------------------------------------------------------------------------------------------
def geom(shape, c0=0, cpad=0, hpad=0, wpad=0, n0=0, npad=0, **_):
    """the view deform_ref.place makes of an NCHW shape: strides and offset in elements (the buffer itself is 16-byte aligned)"""
    n, c, h, w = shape
    assert 0 <= c0 <= cpad and 0 <= n0 <= npad, "the window lies inside its buffer"
    sw = c + cpad
    sh = (w + wpad) * sw
    sn = (h + hpad) * sh
    return NS(n=n, c=c, h=h, w=w, sn=sn, sh=sh, sw=sw, off=n0 * sn + c0)


def _aligned(g, e=4):
    return g.sw % e == 0 and g.sh % e == 0 and g.sn % e == 0 and g.off % e == 0


def vec4(g):                                         # view_vec4
    return g.c % 4 == 0 and _aligned(g)


def warp_form(img, out):                             # vc_warp
    if out.c % 4 == 0 and vec4(img) and vec4(out):
        return "v4"
    return "px3" if out.c == 3 else ("px" if out.c <= 4 else "generic")


def upsample_form(inp, out):                         # vc_upsample_bilinear
    return "v4" if out.c % 4 == 0 and vec4(inp) and vec4(out) else "scalar"


def upsample_sp3_pb(c):                              # vc_upsample_bilinear_sp3: planes per workgroup
    cg = c // 8
    return 8 if cg % 8 == 0 else (4 if cg % 4 == 0 else 1)


def maxpool_form(inp, out):                          # vc_maxpool2
    return "v4" if vec4(inp) and _aligned(out) else "scalar"


def axpby_form(a, b, out):                           # vc_axpby
    views = [v for v in (a, b, out) if v is not None]
    if (out.w * out.c) % 4 == 0 and all(v.sw == out.c and v.sh % 4 == 0 and v.sn % 4 == 0 and v.off % 4 == 0 for v in views):
        return "rows"
    return "v4" if out.c % 4 == 0 and all(vec4(v) for v in views) else "scalar"


def level_input_form(feat, up):                      # vc_spynet_level_input
    return "vec" if vec4(feat) and _aligned(up, 2) else "scalar"


def rowmap(n, h, w, per_px):
    """vc_rowmap_make + vc_rowmap_grid of csrc/ew_rowmap.h: None = the linear fallback, else workgroups per row, rows per grid
    step and whether the row loop runs a second iteration"""
    items = w * per_px
    if n > 65535 or h > 65535 or items >= 1 << 24 or items * per_px >= 1 << 32:
        return None
    bx = (items + EW_BLOCK - 1) // EW_BLOCK
    gy = min(h, max(1, (8192 + bx * n - 1) // (bx * n)))
    return NS(bx=bx, gy=gy, loops=h > gy, reciprocal=per_px > 1 and per_px & (per_px - 1) != 0)


# ------------------------------------------------------------------------------------------------
# windows used over and over
# ------------------------------------------------------------------------------------------------
DENSE = {}
# a channel slice of a concat buffer, a spatial crop and a run of images, 16-byte aligned (cpad and c0 multiples of 4)
WIN_A = dict(c0=4, cpad=8, hpad=2, wpad=1, n0=1, npad=2)
# the same at an odd channel offset
WIN_U = dict(c0=1, cpad=3, hpad=1, wpad=2, n0=2, npad=2)
OFF1 = dict(c0=1, cpad=4)                            # channel offset 1 of a buffer 4 channels wider: pointer 4 bytes off
OFF2 = dict(c0=2, cpad=4)


# ------------------------------------------------------------------------------------------------
# warp
# ------------------------------------------------------------------------------------------------
def _case(ident, **kw):
    return NS(id=ident, **kw)


# c_img > c: the kernel reads a channel slice of a wider image view
WARP_CASES = [
    _case("v4-c8", form="v4", c_img=8, c=8, img=DENSE, flow=DENSE, out=DENSE),
    _case("v4-c8-of-12-window", form="v4", c_img=12, c=8, img=dict(c0=4, cpad=4, hpad=1, wpad=2, n0=1, npad=1), flow=WIN_U, out=WIN_A),
    _case("px3-c3", form="px3", c_img=3, c=3, img=DENSE, flow=DENSE, out=DENSE),
    _case("px3-c3-of-5-window", form="px3", c_img=5, c=3, img=WIN_U, flow=WIN_A, out=dict(c0=2, cpad=3, hpad=2, wpad=1, n0=1, npad=2)),
    _case("px-c1", form="px", c_img=1, c=1, img=DENSE, flow=DENSE, out=DENSE),
    _case("px-c2-of-3-window", form="px", c_img=3, c=2, img=WIN_A, flow=WIN_U, out=WIN_U),
    _case("px-c4-at-channel-offset-1", form="px", c_img=4, c=4, img=OFF1, flow=DENSE, out=OFF1),
    _case("generic-c5", form="generic", c_img=5, c=5, img=DENSE, flow=DENSE, out=DENSE),
    _case("generic-c7-of-9-window", form="generic", c_img=9, c=7, img=WIN_U, flow=WIN_U, out=WIN_A),
    _case("generic-c8-at-channel-offset-2", form="generic", c_img=8, c=8, img=OFF2, flow=DENSE, out=OFF2),
]
# linear fallback of the row map (n > 65535): the large dimension on n, the coordinates stay tiny
WARP_FALLBACK = [
    _case("px3-c3-n65536", form="px3", c_img=3, c=3, img=DENSE, flow=DENSE, out=dict(cpad=1), n=65536, h=2, w=3),
    _case("v4-c8-n65536", form="v4", c_img=8, c=8, img=DENSE, flow=DENSE, out=dict(cpad=4), n=65536, h=2, w=3),
]


def _to_flow(convention, pos, h, w):
    """the flow that makes convention W sample at pixel position ``pos`` [n, 2 (x, y), h, w]:
    W1 samples at x + u W / (W - 1), W2 at x + u - 0.5, W3 at x + u"""
    ident = torch.stack((torch.arange(w, dtype=F64).view(1, w).expand(h, w), torch.arange(h, dtype=F64).view(h, 1).expand(h, w)))
    d = pos - ident
    if convention == 2:
        return d + 0.5
    if convention == 1:
        return d * torch.tensor([(w - 1) / w, (h - 1) / h], dtype=F64).view(1, 2, 1, 1)
    return d


@functools.lru_cache(maxsize=None)
def warp_inputs(convention, c, h, w, n=2):
    """image uniform in [0, 1]; sample positions within +-3 px of the pixel, and at chosen pixels: exactly on the first / last row
    and column, within (0, 1) px outside each border (W2: partial weights of the zero padding), far outside, both at once in the
    corners; a block of zero flow.  A 1-pixel-wide (-high) image divides by W - 1 = 0 under W1 / W3: there the flow along that
    axis is kept away from zero (0 / 0) and the sample lands on the only pixel."""
    g = torch.Generator().manual_seed(10000 * convention + 1000 * c + 37 * h + w)
    img = torch.rand(n, c, h, w, generator=g)
    ident = torch.stack((torch.arange(w, dtype=F64).view(1, w).expand(h, w), torch.arange(h, dtype=F64).view(h, 1).expand(h, w)))
    pos = ident + (torch.rand(n, 2, h, w, generator=g, dtype=F64) - 0.5) * 6
    xs = [0.0, w - 1.0, -0.25, -0.5, -0.75, w - 0.75, w - 0.5, w - 0.25, -50.0, w + 50.0]
    ys = [0.0, h - 1.0, -0.25, -0.5, -0.75, h - 0.75, h - 0.5, h - 0.25, -50.0, h + 50.0]
    targets = [(px, None) for px in xs] + [(None, py) for py in ys] + [(px, py) for px in xs[:8:2] for py in ys[1:8:2]]
    for j, (px, py) in enumerate(targets):
        i, y, x = j % n, (5 * j + 1) % h, (7 * j + 2) % w
        if px is not None:
            pos[i, 0, y, x] = px
        if py is not None:
            pos[i, 1, y, x] = py
    flow = _to_flow(convention, pos, h, w)
    flow[:, :, h // 2:h // 2 + 2, w // 3:w // 3 + 3] = 0.0
    if convention != 2:
        for axis, size in ((0, w), (1, h)):
            if size == 1:
                flow[:, axis] = torch.where(flow[:, axis].abs() < 0.25, torch.full_like(flow[:, axis], 0.5), flow[:, axis])
    return img, flow.float()


@functools.lru_cache(maxsize=None)
def warp_ref(convention, c, h, w, n=2):
    img, flow = warp_inputs(convention, c, h, w, n)
    return warp(convention, img, flow)


# ------------------------------------------------------------------------------------------------
# up-sampling
# ------------------------------------------------------------------------------------------------
def _up(ident, form, c, inp, out, n, h, w, factor, align, scale=1.0):
    return _case(ident, form=form, c=c, inp=inp, out=out, n=n, h=h, w=w, factor=factor, align=align, scale=scale)


UPSAMPLE_CASES = [
    # every form by name: channel count, stride and base alignment decide
    _up("scalar-c2", "scalar", 2, DENSE, DENSE, 2, 9, 19, 2, False),
    _up("scalar-c5-x4-scale", "scalar", 5, DENSE, DENSE, 2, 3, 37, 4, False, 0.5),
    _up("scalar-c8-at-channel-offset-1", "scalar", 8, OFF1, DENSE, 2, 9, 19, 2, False),
    _up("scalar-c8-out-at-channel-offset-1", "scalar", 8, DENSE, OFF1, 2, 3, 37, 2, False),
    _up("scalar-c5-window", "scalar", 5, WIN_U, WIN_A, 2, 9, 19, 2, False, 2.0),
    _up("v4-c4", "v4", 4, DENSE, DENSE, 2, 9, 19, 2, False),
    _up("v4-c128", "v4", 128, DENSE, DENSE, 2, 3, 5, 2, False, 2.0),
    _up("v4-c8-window-x4", "v4", 8, WIN_A, dict(c0=8, cpad=12, hpad=1, wpad=3, n0=1, npad=1), 2, 3, 37, 4, False, 0.5),
]
# the arithmetic: factors 1 .. 4, both align_corners, 1-pixel inputs, scale != 1 -- scalar (c = 3) and v4 (c = 4).  Exact scales
# (align_corners = False with factor 1, 2, 4) at the base sizes; inexact ones (factor 3, align_corners) at most 8 pixels a side
for _c, _form in ((3, "scalar"), (4, "v4")):
    for _f in (1, 2, 3, 4):
        for _al in (False, True):
            _exact = not _al and _f != 3
            for _h, _w in ((SIZES if _exact else [(5, 8), (7, 3)]) + TINY[:2] + [(8 if not _exact else 9, 1)]):
                UPSAMPLE_CASES.append(_up(f"{_form}-c{_c}-x{_f}-{'ac' if _al else 'hp'}-{_h}x{_w}", _form, _c, DENSE, DENSE, 2, _h, _w, _f, _al,
                                          1.0 if _f == 2 else 0.75))
# the row map under the scalar form: per_px = c in {3, 5, 6, 12}, out.w * c around and beyond one workgroup's 256 work items and no
# multiple of it; (n, h) small.  The output has one padding channel so that no view is dense.
UPSAMPLE_ROWMAP = [
    _up("scalar-c3-255", "scalar", 3, DENSE, dict(cpad=1), 2, 3, 85, 1, False),
    _up("scalar-c3-516", "scalar", 3, DENSE, dict(cpad=1), 2, 2, 43, 4, False),
    _up("scalar-c5-260", "scalar", 5, DENSE, dict(cpad=1), 2, 2, 13, 4, False),
    _up("scalar-c5-520", "scalar", 5, DENSE, dict(cpad=1), 2, 3, 26, 4, False),
    _up("scalar-c6-258", "scalar", 6, DENSE, dict(cpad=1), 2, 3, 43, 1, False),
    _up("scalar-c6-516", "scalar", 6, DENSE, dict(cpad=1), 2, 3, 43, 2, False),
    _up("scalar-c12-264", "scalar", 12, OFF1, dict(cpad=1), 2, 3, 11, 2, False),
    _up("scalar-c12-516", "scalar", 12, OFF1, dict(cpad=1), 2, 3, 43, 1, False),
]
# the row loop: n = 64 images, 270 work items a row = 2 workgroups -> gridDim.y = 8192 / (64 * 2) = 64 < out.h = 70
UPSAMPLE_ROWLOOP = _up("scalar-c5-rowloop", "scalar", 5, DENSE, dict(cpad=1), 64, 35, 27, 2, False)
# linear fallback: n = 65536 images of 2 x 3
UPSAMPLE_FALLBACK = _up("scalar-c1-n65536", "scalar", 1, DENSE, dict(cpad=1), 65536, 2, 3, 2, False, 0.5)

# split-tensor output: (id, c, n, in.h, in.w, factor, align, scale): output width below and just above a workgroup's 256 / PB pixels
UPSAMPLE_SP3 = [
    _case("pb8-c64-ow10", pb=8, c=64, n=2, h=3, w=5, factor=2, align=False, scale=1.0),
    _case("pb8-c64-ow34", pb=8, c=64, n=1, h=3, w=17, factor=2, align=False, scale=2.0),
    _case("pb4-c32-ow10", pb=4, c=32, n=2, h=3, w=5, factor=2, align=False, scale=1.0),
    _case("pb4-c32-ow68", pb=4, c=32, n=1, h=3, w=17, factor=4, align=False, scale=0.5),
    _case("pb1-c8-ow258", pb=1, c=8, n=2, h=2, w=129, factor=2, align=False, scale=1.0),
    _case("pb1-c24-ow38", pb=1, c=24, n=2, h=9, w=19, factor=2, align=False, scale=1.0),
    _case("pb1-c8-ac-x3", pb=1, c=8, n=2, h=5, w=8, factor=3, align=True, scale=0.75),
    _case("pb4-c32-1x1-ac", pb=4, c=32, n=2, h=1, w=1, factor=2, align=True, scale=1.0),
]


@functools.lru_cache(maxsize=None)
def upsample_inputs(c, n, h, w):
    return rand((n, c, h, w), 200000 + 1000 * c + 37 * h + w + 7 * n)


# ------------------------------------------------------------------------------------------------
# pooling
# ------------------------------------------------------------------------------------------------
def _ap(ident, c, k, h, w, oh, ow, scale=1.0, inp=DENSE, out=DENSE, n=2):
    return _case(ident, c=c, k=k, h=h, w=w, oh=oh, ow=ow, scale=scale, inp=inp, out=out, n=n)


AVGPOOL_CASES = []
for _k in (1, 2, 4):
    for _hp, _wp in SIZES:
        for _rem in ((0,) if _k == 1 else (0, _k - 1)):                 # in.h % k != 0, in.w % k != 0: the remainder is not read
            _h, _w = _hp * _k + _rem, _wp * _k + _rem
            # no padding, one row / column, the most reflection allows (pad == pooled size - 1), each direction on its own
            for _ph, _pw in ((0, 0), (1, 0), (0, 1), (_hp - 1, 0), (0, _wp - 1)):
                AVGPOOL_CASES.append(_ap(f"k{_k}-{_h}x{_w}-pad{_ph}+{_pw}", 3, _k, _h, _w, _hp + _ph, _wp + _pw, 0.5 if _k == 4 else 1.0))
    AVGPOOL_CASES.append(_ap(f"k{_k}-one-output-pixel", 5, _k, 2 * _k - 1, 2 * _k - 1, 1, 1, 1.0))
    AVGPOOL_CASES.append(_ap(f"k{_k}-window", 5, _k, 9 * _k, 19 * _k, 12, 20, 0.75, WIN_U, WIN_A))
# linear fallback: 65536 rows
AVGPOOL_FALLBACK = _ap("k1-h65536", 3, 1, 65536, 2, 65536, 2, 0.5, DENSE, dict(cpad=1), n=1)

MAXPOOL_CASES = [  # input sizes: even, odd (the last row / column is not read), one output pixel
    _case("v4-c8", form="v4", c=8, inp=DENSE, out=DENSE, sizes=[(18, 38), (7, 75), (2, 2)]),
    _case("v4-c8-window", form="v4", c=8, inp=WIN_A, out=dict(c0=8, cpad=12, hpad=1, wpad=3, n0=1, npad=1), sizes=[(19, 39)]),
    _case("scalar-c3", form="scalar", c=3, inp=DENSE, out=DENSE, sizes=[(18, 38), (7, 75), (3, 3)]),
    _case("scalar-c8-at-channel-offset-1", form="scalar", c=8, inp=OFF1, out=DENSE, sizes=[(19, 39)]),
    _case("scalar-c8-out-at-channel-offset-1", form="scalar", c=8, inp=DENSE, out=OFF1, sizes=[(18, 38)]),
    _case("scalar-c5-window", form="scalar", c=5, inp=WIN_U, out=WIN_A, sizes=[(19, 39)]),
]
# linear fallback: the OUTPUT has 65536 rows, the input 131072
MAXPOOL_FALLBACK = _case("scalar-c3-h65536", form="scalar", c=3, inp=DENSE, out=dict(cpad=1), sizes=[(131072, 4)])
POOL_SP3_SIZES = [(2, 16, 18, 38), (1, 8, 2, 2), (2, 24, 6, 74)]         # n, c, h, w (h, w even)


# ------------------------------------------------------------------------------------------------
# axpby
# ------------------------------------------------------------------------------------------------
ALPHA, BETA = 0.75, -1.25     # (exact in fp32: the reference scales by the very factors the kernel gets)


@functools.lru_cache(maxsize=None)
def axpby_inputs(c, n, h, w):
    return rand((n, c, h, w), 400000 + 1000 * c + 37 * h + w + 7 * n), rand((n, c, h, w), 500000 + 1000 * c + 37 * h + w + 7 * n, -1.0, 1.0)


def _ax(ident, form, c, n, h, w, a=DENSE, b=DENSE, out=DENSE):
    return _case(ident, form=form, c=c, n=n, h=h, w=w, a=a, b=b, out=out)


_ROWS_WIN = dict(hpad=2, wpad=4, n0=1, npad=1)       # dense rows inside a crop: the row pitch stays a multiple of 4 floats
AXPBY_CASES = [
    _ax("rows-c3-w8", "rows", 3, 2, 9, 8),
    _ax("rows-c3-w4-crop", "rows", 3, 2, 3, 4, _ROWS_WIN, _ROWS_WIN, _ROWS_WIN),
    _ax("rows-c5-w12", "rows", 5, 2, 3, 12),
    _ax("v4-c8-window", "v4", 8, 2, 9, 19, WIN_A, dict(c0=8, cpad=12, hpad=1, wpad=3, n0=1, npad=1), WIN_A),
    _ax("v4-c4-wide-pixels", "v4", 4, 2, 3, 37, dict(cpad=4), dict(cpad=4), dict(cpad=4)),
    _ax("scalar-c3-w19", "scalar", 3, 2, 9, 19),
    _ax("scalar-c5-window", "scalar", 5, 2, 3, 37, WIN_U, WIN_A, WIN_U),
    _ax("scalar-c8-a-at-channel-offset-1", "scalar", 8, 2, 9, 19, OFF1, dict(cpad=4), dict(cpad=4)),
    _ax("scalar-1x1", "scalar", 1, 1, 1, 1),
]
# the row map: per_px in {3, 5, 6, 12} (c under the scalar form, c / 4 under v4), w * per_px no multiple of 256, one and several
# workgroups a row
AXPBY_ROWMAP = [
    _ax("scalar-c3-255", "scalar", 3, 2, 3, 85, DENSE, DENSE, dict(cpad=1)),
    _ax("scalar-c3-513", "scalar", 3, 2, 3, 171, DENSE, DENSE, dict(cpad=1)),
    _ax("scalar-c5-255", "scalar", 5, 2, 3, 51, DENSE, DENSE, dict(cpad=1)),
    _ax("scalar-c5-515", "scalar", 5, 2, 2, 103, DENSE, DENSE, dict(cpad=1)),
    _ax("scalar-c6-258", "scalar", 6, 2, 3, 43, DENSE, DENSE, dict(cpad=1)),
    _ax("scalar-c12-516", "scalar", 12, 2, 3, 43, DENSE, DENSE, dict(cpad=1)),
    _ax("v4-c12-258", "v4", 12, 2, 3, 86, dict(cpad=4), dict(cpad=4), dict(cpad=4)),
    _ax("v4-c20-515", "v4", 20, 2, 3, 103, dict(cpad=4), dict(cpad=4), dict(cpad=4)),
    _ax("v4-c48-516", "v4", 48, 2, 2, 43, dict(cpad=4), dict(cpad=4), dict(cpad=4)),
]
# the row loop: n = 64, 270 work items a row = 2 workgroups -> gridDim.y = 8192 / (64 * 2) = 64 < h = 70
AXPBY_ROWLOOP = _ax("scalar-c5-rowloop", "scalar", 5, 64, 70, 54, DENSE, DENSE, dict(cpad=1))
# linear fallback: h = 65536 rows of 1 .. 3 pixels, one per form
AXPBY_FALLBACK = [
    _ax("rows-c4-h65536-w1", "rows", 4, 1, 65536, 1),
    _ax("scalar-c3-h65536-w2", "scalar", 3, 1, 65536, 2, DENSE, DENSE, dict(cpad=1)),
    _ax("v4-c4-h65536-w3", "v4", 4, 1, 65536, 3, dict(cpad=4), dict(cpad=4), dict(cpad=4)),
]


def axpby_per_px(case):
    return {"scalar": case.c, "v4": case.c // 4, "rows": 1}[case.form]


def axpby_width(case):
    return case.w * case.c // 4 if case.form == "rows" else case.w


# ------------------------------------------------------------------------------------------------
# SPyNet level input
# ------------------------------------------------------------------------------------------------
# (id, form, coarse size or None, level size, windows of first / second / coarse flow / feat / up)
def _li(ident, form, coarse, h, w, n=2, first=DENSE, second=DENSE, fc=DENSE, feat=DENSE, up=DENSE):
    return _case(ident, form=form, coarse=coarse, h=h, w=w, n=n, first=first, second=second, fc=fc, feat=feat, up=up)


_FEAT_1_8_OF_12 = dict(c0=1, cpad=4)
LEVEL_SHAPES = [("even", (4, 9), 8, 18), ("odd-h", (4, 9), 9, 18), ("odd-w", (4, 9), 8, 19), ("odd-both", (4, 9), 9, 19),
                ("no-coarse-flow", None, 9, 19), ("coarse-1x1", (1, 1), 3, 3)]
LEVEL_CASES = []
for _name, _coarse, _h, _w in LEVEL_SHAPES:
    LEVEL_CASES.append(_li(f"vec-{_name}", "vec", _coarse, _h, _w))
    LEVEL_CASES.append(_li(f"scalar-feat-1..8-of-12-{_name}", "scalar", _coarse, _h, _w, feat=_FEAT_1_8_OF_12))
LEVEL_CASES += [
    _li("scalar-up-at-odd-offset", "scalar", (4, 9), 9, 19, up=dict(c0=1, cpad=1)),
    _li("vec-windows", "vec", (4, 9), 9, 19, first=WIN_U, second=dict(c0=2, cpad=2, hpad=1, wpad=1, n0=1, npad=1), fc=WIN_U,
        feat=dict(c0=8, cpad=8, hpad=1, wpad=2, n0=1, npad=1), up=dict(c0=2, cpad=2, hpad=2, wpad=1, n0=1, npad=1)),
    _li("scalar-windows", "scalar", (4, 9), 8, 19, first=WIN_A, second=WIN_U, fc=WIN_A, feat=dict(c0=3, cpad=5, hpad=1, wpad=2, n0=1, npad=1),
        up=WIN_U),
    _li("vec-n1", "vec", (4, 9), 9, 18, n=1),
]


@functools.lru_cache(maxsize=None)
def level_inputs(coarse, h, w, n=2):
    """two frames uniform in [0, 1]; a smooth coarse flow of a few pixels (a ramp of at most 0.3 px per coarse pixel plus the
    image's own offset): the up-sampled flow's fp32 coordinate error times its gradient has to stay inside 1e-6"""
    g = torch.Generator().manual_seed(300000 + 37 * h + w + 7 * n + (0 if coarse is None else 1000 * coarse[0] + coarse[1]))
    first, second = torch.rand(n, 3, h, w, generator=g), torch.rand(n, 3, h, w, generator=g)
    if coarse is None:
        return first, second, None
    ch, cw = coarse
    ramp = torch.arange(ch, dtype=torch.float32).view(1, 1, ch, 1) * 0.2 - torch.arange(cw, dtype=torch.float32).view(1, 1, 1, cw) * 0.3
    fc = ramp * torch.tensor([1.0, -0.5]).view(1, 2, 1, 1) + (torch.rand(n, 2, 1, 1, generator=g) - 0.5) * 3 + torch.rand(n, 2, ch, cw, generator=g) * 0.1
    return first, second, fc
