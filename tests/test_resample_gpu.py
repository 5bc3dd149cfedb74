"""-m gpu: the resampling, pooling and warping kernels of csrc/ew_kernels.hip -- every form the host-side dispatch can select, the
row map of csrc/ew_rowmap.h in each of its regimes (reciprocal division, several workgroups a row, the row loop, the linear
fallback), windows into larger buffers, and the edges of the arithmetic -- against the float64 references of tests/resample_ref.py
(pinned on the CPU by tests/test_resample_cpu.py).

Every case says in its id which form it is meant to reach; the test asserts, from the views it really passes, that the restated
dispatch condition (resample_ref.*_form) says the same, so a case that silently lands on another kernel fails.  Outputs are windows
of buffers filled with a sentinel: everything outside the window must keep its bits.

Bounds (the project's own, tests/test_ops_gpu.py; none taken from the kernels): |out - ref| / (1 + |ref|) <= 2e-5 for warping and
the warped channels of the level input, <= 1e-6 for up-sampling, average pooling, axpby and the flow channels of the level input;
max pooling, copies, sentinels, bit equalities and return codes exact."""
import os

import pytest
import torch

import resample_ref as rr

pytestmark = pytest.mark.gpu
MAXIMA = {}
EINVAL = -1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda:0")
    for k in sorted(MAXIMA):
        print(f"\nlargest error seen, {k}: {MAXIMA[k]:.2e}", end="")


def _ids(case):
    return case.id


def _hold(entry, what, out, ref, cap):
    d = rr.rel_err(out, ref)
    MAXIMA[entry] = max(MAXIMA.get(entry, 0.0), d)
    print(f"{entry} {what}: {d:.2e}")
    assert d <= cap, f"{entry} {what}: {d:.3e} > {cap}"


def _ok(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def _out(shape, dev, spec):
    """an output window inside a buffer that holds the sentinel everywhere, the window included"""
    return rr.place(torch.full(shape, rr.SENTINEL), dev, fill=rr.SENTINEL, **spec)


def _as_geom(t, shape, spec):
    """the view really passed is the one the CPU-side dispatch predicate was evaluated on"""
    g = rr.geom(shape, **spec)
    assert (t.n, t.c, t.h, t.w, t.sn, t.sh, t.sw, t.off) == (g.n, g.c, g.h, g.w, g.sn, g.sh, g.sw, g.off) and t.buf.data_ptr() % 16 == 0
    assert (t.ptr % 16 == 0) == (g.off % 4 == 0)
    return g


def _finish(entry, what, t_out, ref, cap):
    win, outside = rr.read_window(t_out)
    rr.assert_untouched(outside)
    if cap == 0:
        assert torch.equal(win.double(), ref.double()), f"{entry} {what}: not exact"
    else:
        _hold(entry, what, win, ref, cap)
    return win


def _null(n=0, h=0, w=0, c=0):
    from vcamd import hip
    return hip.View(None, n, h, w, c, 0, 0, 0)


def _v(t, **over):
    v = t.view()
    for k, val in over.items():
        setattr(v, k, val)
    return v


def _refused(outs, calls):
    """every call returns VC_EINVAL and none of the output buffers changes a bit"""
    for what, rc in calls:
        assert rc == EINVAL, f"{what}: returned {rc}, not VC_EINVAL"
    torch.cuda.synchronize()
    for t in outs:
        rr.assert_untouched((t.buf if hasattr(t, "buf") else t).cpu().view(-1).view(torch.float32))


# ------------------------------------------------------------------------------------------------
# warp
# ------------------------------------------------------------------------------------------------
def _warp(dev, case, convention, h, w, n=2):
    from vcamd import hip
    img, flow = rr.warp_inputs(convention, case.c_img, h, w, n)
    ref = rr.warp_ref(convention, case.c_img, h, w, n)[:, :case.c]
    ti, tf = rr.place(img, dev, **case.img), rr.place(flow, dev, seed=1, **case.flow)
    to = _out((n, case.c, h, w), dev, case.out)
    gi, go = _as_geom(ti, (n, case.c_img, h, w), case.img), _as_geom(to, (n, case.c, h, w), case.out)
    assert rr.warp_form(gi, go) == case.form
    _ok(hip.lib().vc_warp(hip.stream(), convention, ti.view(), tf.view(), to.view()), "vc_warp")
    _finish(f"vc_warp W{convention}", f"{case.id} {n}x{h}x{w}", to, ref, rr.CAP_WARP)


@pytest.mark.parametrize("convention", [1, 2, 3])
@pytest.mark.parametrize("h,w", rr.SIZES)
@pytest.mark.parametrize("case", rr.WARP_CASES, ids=_ids)
def test_warp_every_form(dev, case, h, w, convention):
    """k_warp_v4 / k_warp_px3 / k_warp_px / k_warp under W1, W2, W3: zero flow, samples exactly on the last row and column, within a
    pixel outside every border (W2: partial weights), far outside; windows read a channel slice of a wider image"""
    _warp(dev, case, convention, h, w)


@pytest.mark.parametrize("convention", [1, 2, 3])
@pytest.mark.parametrize("h,w", rr.TINY)
@pytest.mark.parametrize("case", [rr.WARP_CASES[0], rr.WARP_CASES[2], rr.WARP_CASES[7]], ids=_ids)
def test_warp_one_pixel_images(dev, case, h, w, convention):
    """1-pixel-high / -wide images: W1 and W3 divide by W - 1 = 0 and land, like grid_sample, on the only pixel"""
    _warp(dev, case, convention, h, w)


@pytest.mark.parametrize("convention", [1, 2, 3])
@pytest.mark.parametrize("case", rr.WARP_FALLBACK, ids=_ids)
def test_warp_linear_fallback(dev, case, convention):
    """n = 65536 > 65535 images: ew_for_each<false>, the 64-bit linear index taken apart by division"""
    assert rr.rowmap(case.n, case.h, case.w, 1) is None
    _warp(dev, case, convention, case.h, case.w, case.n)


def test_warp_refusals(dev):
    from vcamd import hip
    L, s = hip.lib(), hip.stream()
    x = rr.rand((2, 4, 5, 7), 1)
    img, flow, out = rr.place(x, dev), rr.place(x[:, :2], dev), _out((2, 4, 5, 7), dev, {})
    _refused([out], [
        ("null image", L.vc_warp(s, 1, _null(2, 5, 7, 4), flow.view(), out.view())),
        ("null flow", L.vc_warp(s, 1, img.view(), _null(2, 5, 7, 2), out.view())),
        ("null output", L.vc_warp(s, 1, img.view(), flow.view(), _null(2, 5, 7, 4))),
        ("convention 0", L.vc_warp(s, 0, img.view(), flow.view(), out.view())),
        ("convention 4", L.vc_warp(s, 4, img.view(), flow.view(), out.view())),
        ("one flow channel", L.vc_warp(s, 1, img.view(), _v(flow, c=1), out.view())),
        ("more output channels than the image has", L.vc_warp(s, 1, _v(img, c=3), flow.view(), out.view())),
        ("no output channel", L.vc_warp(s, 1, img.view(), flow.view(), _v(out, c=0))),
        ("flow of another height", L.vc_warp(s, 1, img.view(), _v(flow, h=4), out.view())),
        ("flow of another width", L.vc_warp(s, 1, img.view(), _v(flow, w=6), out.view())),
        ("image count of the image", L.vc_warp(s, 1, _v(img, n=1), flow.view(), out.view())),
        ("image count of the flow", L.vc_warp(s, 1, img.view(), _v(flow, n=1), out.view())),
    ])


# ------------------------------------------------------------------------------------------------
# up-sampling
# ------------------------------------------------------------------------------------------------
def _upsample(dev, case):
    from vcamd import hip
    x = rr.upsample_inputs(case.c, case.n, case.h, case.w)
    ref = rr.upsample(x, case.factor, case.align, case.scale)
    oshape = (case.n, case.c, case.h * case.factor, case.w * case.factor)
    ti, to = rr.place(x, dev, **case.inp), _out(oshape, dev, case.out)
    assert rr.upsample_form(_as_geom(ti, tuple(x.shape), case.inp), _as_geom(to, oshape, case.out)) == case.form
    _ok(hip.lib().vc_upsample_bilinear(hip.stream(), ti.view(), to.view(), case.factor, int(case.align), case.scale), "vc_upsample_bilinear")
    _finish("vc_upsample_bilinear", case.id, to, ref, rr.CAP_LINEAR)


@pytest.mark.parametrize("case", rr.UPSAMPLE_CASES, ids=_ids)
def test_upsample_every_form_and_edge(dev, case):
    """k_upsample_bilinear / k_upsample_bilinear_v4: factors 1 .. 4, both align_corners, inputs of one row / column / pixel, scale"""
    _upsample(dev, case)


@pytest.mark.parametrize("case", rr.UPSAMPLE_ROWMAP, ids=_ids)
def test_upsample_row_map(dev, case):
    """per_px in {3, 5, 6, 12}: (x, c) by multiply-high with the host-made reciprocal, rows of one and of several workgroups"""
    m = rr.rowmap(case.n, case.h * case.factor, case.w * case.factor, case.c)
    assert m is not None and m.reciprocal and not m.loops
    _upsample(dev, case)


def test_upsample_row_loop(dev):
    """64 images x 2 workgroups a row -> gridDim.y = 64 < 70 output rows: rows 64 .. 69 come from the second pass of `y += gridDim.y`"""
    case = rr.UPSAMPLE_ROWLOOP
    m = rr.rowmap(case.n, case.h * case.factor, case.w * case.factor, case.c)
    assert m.loops and m.gy == 64 < case.h * case.factor
    _upsample(dev, case)


def test_upsample_linear_fallback(dev):
    case = rr.UPSAMPLE_FALLBACK
    assert rr.rowmap(case.n, case.h * case.factor, case.w * case.factor, case.c) is None
    _upsample(dev, case)


def _zero_planes(wide, n, lo, hi):
    """the planes of a split tensor outside [lo, hi) hold nothing but zero bytes"""
    planes = wide.buf.cpu().view(n, wide.sn, -1)
    return not bool(planes[:, :lo].any()) and not bool(planes[:, hi:].any())


@pytest.mark.parametrize("case", rr.UPSAMPLE_SP3, ids=_ids)
def test_upsample_into_a_split_tensor(dev, case):
    """k_upsample_bilinear_sp3<8 / 4 / 1>: into a window of planes of a wider, zero-filled split tensor (out_image_bytes != 0) and
    into a dense one; within the cap of float64 and bit for bit vc_split3 of the fp32 kernel's result"""
    from vcamd import hip
    L, s = hip.lib(), hip.stream()
    assert rr.upsample_sp3_pb(case.c) == case.pb
    x = rr.upsample_inputs(case.c, case.n, case.h, case.w)
    ref = rr.upsample(x, case.factor, case.align, case.scale)
    ti = rr.place(x, dev, **(rr.WIN_A if case.n == 2 else rr.DENSE))         # (16-byte aligned either way: the entry point asks for it)
    oh, ow, cw = case.h * case.factor, case.w * case.factor, case.c + 24
    wide = hip.T.empty(case.n, oh, ow, cw, dev, "sp3")
    wide.buf.zero_()
    win = wide.channels(8, 8 + case.c)
    assert win.image_bytes == (cw // 8) * oh * ow * 48
    _ok(L.vc_upsample_bilinear_sp3(s, ti.view(), win.ptr, win.image_bytes, case.factor, int(case.align), case.scale), "vc_upsample_bilinear_sp3")
    _hold("vc_upsample_bilinear_sp3", case.id, rr.unsplit(wide.buf, case.n, cw, oh, ow)[:, 8:8 + case.c], ref, rr.CAP_LINEAR)
    assert _zero_planes(wide, case.n, 1, 1 + case.c // 8)
    dense = hip.T.empty(case.n, oh, ow, case.c, dev, "sp3")
    dense.buf.fill_(0x7fff)
    _ok(L.vc_upsample_bilinear_sp3(s, ti.view(), dense.ptr, 0, case.factor, int(case.align), case.scale), "vc_upsample_bilinear_sp3")
    assert torch.equal(dense.buf.view(case.n, case.c // 8, -1), wide.buf.view(case.n, cw // 8, -1)[:, 1:1 + case.c // 8])
    f32 = hip.T.empty(case.n, oh, ow, case.c, dev)
    _ok(L.vc_upsample_bilinear(s, ti.view(), f32.view(), case.factor, int(case.align), case.scale), "vc_upsample_bilinear")
    assert torch.equal(hip.split3(f32).buf, dense.buf)


def test_upsample_refusals(dev):
    from vcamd import hip
    L, s = hip.lib(), hip.stream()
    x = rr.rand((2, 8, 3, 5), 2)
    ti, to = rr.place(x, dev), _out((2, 8, 6, 10), dev, {})
    up = L.vc_upsample_bilinear
    _refused([to], [
        ("null input", up(s, _null(2, 3, 5, 8), to.view(), 2, 0, 1.0)), ("null output", up(s, ti.view(), _null(2, 6, 10, 8), 2, 0, 1.0)),
        ("factor 0", up(s, ti.view(), to.view(), 0, 0, 1.0)), ("channels", up(s, _v(ti, c=4), to.view(), 2, 0, 1.0)),
        ("images", up(s, _v(ti, n=1), to.view(), 2, 0, 1.0)), ("height", up(s, ti.view(), _v(to, h=5), 2, 0, 1.0)),
        ("width", up(s, ti.view(), _v(to, w=9), 2, 0, 1.0)), ("factor 3 into a x2 output", up(s, ti.view(), to.view(), 3, 0, 1.0)),
    ])
    sp = hip.T.empty(2, 6, 10, 8, dev, "sp3")
    sp.buf.view(torch.float32).fill_(rr.SENTINEL)
    off1 = rr.place(x, dev, **rr.OFF1)
    us = L.vc_upsample_bilinear_sp3
    _refused([sp], [
        ("null input", us(s, _null(2, 3, 5, 8), sp.ptr, 0, 2, 0, 1.0)), ("null output", us(s, ti.view(), None, 0, 2, 0, 1.0)),
        ("factor 0", us(s, ti.view(), sp.ptr, 0, 0, 0, 1.0)), ("12 channels", us(s, _v(ti, c=12), sp.ptr, 0, 2, 0, 1.0)),
        ("input 4 bytes off", us(s, off1.view(), sp.ptr, 0, 2, 0, 1.0)), ("input pixel stride 9", us(s, _v(ti, sw=9), sp.ptr, 0, 2, 0, 1.0)),
        ("output 8 bytes off", us(s, ti.view(), sp.ptr + 8, 0, 2, 0, 1.0)), ("image pitch no multiple of 16", us(s, ti.view(), sp.ptr, 6 * 10 * 48 + 8, 2, 0, 1.0)),
    ])


# ------------------------------------------------------------------------------------------------
# pooling
# ------------------------------------------------------------------------------------------------
def _avgpool(dev, case):
    from vcamd import hip
    x = rr.upsample_inputs(case.c, case.n, case.h, case.w)
    ref = rr.avgpool_reflectpad(x, case.k, case.scale, case.oh, case.ow)
    ti, to = rr.place(x, dev, **case.inp), _out((case.n, case.c, case.oh, case.ow), dev, case.out)
    _ok(hip.lib().vc_avgpool_reflectpad(hip.stream(), ti.view(), to.view(), case.k, case.scale), "vc_avgpool_reflectpad")
    _finish("vc_avgpool_reflectpad", case.id, to, ref, rr.CAP_LINEAR)


@pytest.mark.parametrize("case", rr.AVGPOOL_CASES, ids=_ids)
def test_avgpool_reflectpad_edges(dev, case):
    """k in {1, 2, 4}; no padding, one row / column, the most reflection allows (pad == pooled size - 1) per direction; input sizes
    that are no multiple of k; windows"""
    _avgpool(dev, case)


def test_avgpool_reflectpad_linear_fallback(dev):
    case = rr.AVGPOOL_FALLBACK
    assert rr.rowmap(case.n, case.oh, case.ow, case.c) is None
    _avgpool(dev, case)


def test_avgpool_reflectpad_refusals(dev):
    from vcamd import hip
    L, s = hip.lib(), hip.stream()
    x = rr.rand((2, 3, 8, 12), 3)
    ti, to = rr.place(x, dev), _out((2, 3, 8, 12), dev, {})
    ap = L.vc_avgpool_reflectpad
    _refused([to], [
        ("null input", ap(s, _null(2, 8, 12, 3), to.view(), 2, 1.0)), ("null output", ap(s, ti.view(), _null(2, 4, 6, 3), 2, 1.0)),
        ("k = 0", ap(s, ti.view(), _v(to, h=4, w=6), 0, 1.0)), ("channels", ap(s, ti.view(), _v(to, h=4, w=6, c=2), 2, 1.0)),
        ("images", ap(s, ti.view(), _v(to, h=4, w=6, n=1), 2, 1.0)),
        ("pad == hp", ap(s, ti.view(), _v(to, h=8, w=6), 2, 1.0)), ("pad == wp", ap(s, ti.view(), _v(to, h=4, w=12), 2, 1.0)),
        ("pad > hp", ap(s, ti.view(), _v(to, h=8, w=3), 4, 1.0)),
        ("output smaller than the pooled size", ap(s, ti.view(), _v(to, h=3, w=6), 2, 1.0)),
        ("hp == 0", ap(s, _v(ti, h=3), _v(to, h=1, w=3), 4, 1.0)), ("wp == 0", ap(s, _v(ti, w=3), _v(to, h=2, w=1), 4, 1.0)),
        ("hp == 0, empty output", ap(s, _v(ti, h=3), _v(to, h=0, w=3), 4, 1.0)),
    ])


@pytest.mark.parametrize("case", rr.MAXPOOL_CASES + [rr.MAXPOOL_FALLBACK], ids=_ids)
def test_maxpool_every_form(dev, case):
    """k_maxpool2_v4 / k_maxpool2 (row map; with 65536 output rows the linear fallback): exact; odd input sizes leave the last row
    and column unread"""
    from vcamd import hip
    for h, w in case.sizes:
        n = 1 if h > 65535 else 2
        x = rr.upsample_inputs(case.c, n, h, w) - 0.5
        ti, to = rr.place(x, dev, **case.inp), _out((n, case.c, h // 2, w // 2), dev, case.out)
        assert rr.maxpool_form(_as_geom(ti, tuple(x.shape), case.inp), _as_geom(to, (n, case.c, h // 2, w // 2), case.out)) == case.form
        if case is rr.MAXPOOL_FALLBACK:
            assert rr.rowmap(n, h // 2, w // 2, case.c) is None
        _ok(hip.lib().vc_maxpool2(hip.stream(), ti.view(), to.view()), "vc_maxpool2")
        _finish("vc_maxpool2", f"{case.id} {h}x{w}", to, rr.maxpool2(x), 0)


def _guarded_split(n, h, w, c, dev, value):
    """a split tensor whose every fp32 word is `value`"""
    from vcamd import hip
    t = hip.T.empty(n, h, w, c, dev, "sp3")
    t.buf.view(torch.float32).fill_(value)
    return t


@pytest.mark.parametrize("n,c,h,w", rr.POOL_SP3_SIZES)
def test_pooling_of_split_tensors(dev, n, c, h, w):
    """vc_maxpool2_sp3 (exact) and vc_avgpool2_sp3 with split and with fp32 output, reading a dense split tensor and a window of
    planes of a wider one whose other planes hold large values; results into windows whose surroundings must not change"""
    from vcamd import hip
    L, s = hip.lib(), hip.stream()
    x = rr.upsample_inputs(c, n, h, w) - 0.5
    xt = rr.place(x, dev)
    src_dense = hip.split3(xt)
    src_wide = hip.T.empty(n, h, w, c + 16, dev, "sp3")
    src_wide.buf.fill_(0x4480)                                        # every piece 1024.0
    src_win = hip.split3(xt, out=src_wide.channels(8, 8 + c))
    oh, ow, cw = h // 2, w // 2, c + 16
    for src, in_bytes in ((src_dense, 0), (src_dense, src_dense.image_bytes), (src_win, src_win.image_bytes)):
        what = f"c={c} {n}x{h}x{w} {'window' if src is src_win else 'dense'}"
        wide = hip.T.empty(n, oh, ow, cw, dev, "sp3")
        wide.buf.zero_()
        win = wide.channels(8, 8 + c)
        _ok(L.vc_maxpool2_sp3(s, src.ptr, in_bytes, n, h, w, c, win.ptr, win.image_bytes), "vc_maxpool2_sp3")
        assert torch.equal(rr.unsplit(wide.buf, n, cw, oh, ow)[:, 8:8 + c], rr.maxpool2(x).double()), what
        assert _zero_planes(wide, n, 1, 1 + c // 8)
        dense = hip.T.empty(n, oh, ow, c, dev, "sp3")
        _ok(L.vc_maxpool2_sp3(s, src.ptr, in_bytes, n, h, w, c, dense.ptr, 0), "vc_maxpool2_sp3")
        assert torch.equal(dense.buf.view(n, c // 8, -1), wide.buf.view(n, cw // 8, -1)[:, 1:1 + c // 8])
        for scale in (1.0, 0.75):
            ref = rr.avgpool_reflectpad(x, 2, scale, oh, ow)
            wide.buf.zero_()
            _ok(L.vc_avgpool2_sp3(s, src.ptr, in_bytes, n, h, w, c, scale, win.ptr, win.image_bytes, _null()), "vc_avgpool2_sp3")
            _hold("vc_avgpool2_sp3, split output", f"{what} scale={scale}", rr.unsplit(wide.buf, n, cw, oh, ow)[:, 8:8 + c], ref, rr.CAP_LINEAR)
            assert _zero_planes(wide, n, 1, 1 + c // 8)
            to = _out((n, c, oh, ow), dev, rr.WIN_A)
            _ok(L.vc_avgpool2_sp3(s, src.ptr, in_bytes, n, h, w, c, scale, None, 0, to.view()), "vc_avgpool2_sp3")
            got = _finish("vc_avgpool2_sp3, fp32 output", f"{what} scale={scale}", to, ref, rr.CAP_LINEAR)
            assert torch.equal(got.double(), rr.unsplit(wide.buf, n, cw, oh, ow)[:, 8:8 + c])        # the split output holds the same values


def test_pooling_refusals(dev):
    from vcamd import hip
    L, s = hip.lib(), hip.stream()
    x = rr.rand((2, 8, 6, 10), 4)
    ti = rr.place(x, dev)
    to = _out((2, 8, 3, 5), dev, {})
    mp = L.vc_maxpool2
    _refused([to], [
        ("null input", mp(s, _null(2, 6, 10, 8), to.view())), ("null output", mp(s, ti.view(), _null(2, 3, 5, 8))),
        ("channels", mp(s, ti.view(), _v(to, c=4))), ("images", mp(s, ti.view(), _v(to, n=1))),
        ("height", mp(s, ti.view(), _v(to, h=2))), ("width", mp(s, ti.view(), _v(to, w=4))), ("not halved", mp(s, ti.view(), _v(to, h=6, w=10))),
    ])
    src = hip.split3(ti)
    osp = _guarded_split(2, 3, 5, 8, dev, rr.SENTINEL)
    ms = L.vc_maxpool2_sp3
    _refused([osp], [
        ("null input", ms(s, None, 0, 2, 6, 10, 8, osp.ptr, 0)), ("null output", ms(s, src.ptr, 0, 2, 6, 10, 8, None, 0)),
        ("no image", ms(s, src.ptr, 0, 0, 6, 10, 8, osp.ptr, 0)), ("odd height", ms(s, src.ptr, 0, 2, 5, 10, 8, osp.ptr, 0)),
        ("odd width", ms(s, src.ptr, 0, 2, 6, 9, 8, osp.ptr, 0)), ("one row", ms(s, src.ptr, 0, 2, 1, 10, 8, osp.ptr, 0)),
        ("one column", ms(s, src.ptr, 0, 2, 6, 1, 8, osp.ptr, 0)), ("12 channels", ms(s, src.ptr, 0, 2, 6, 10, 12, osp.ptr, 0)),
        ("input 4 bytes off", ms(s, src.ptr + 4, 0, 2, 6, 10, 8, osp.ptr, 0)), ("output 4 bytes off", ms(s, src.ptr, 0, 2, 6, 10, 8, osp.ptr + 4, 0)),
        ("input image pitch", ms(s, src.ptr, 6 * 10 * 48 + 4, 2, 6, 10, 8, osp.ptr, 0)),
        ("output image pitch", ms(s, src.ptr, 0, 2, 6, 10, 8, osp.ptr, 3 * 5 * 48 + 4)),
    ])
    av = L.vc_avgpool2_sp3
    nul = _null()
    off1 = _out((2, 8, 3, 5), dev, rr.OFF1)
    _refused([osp, to, off1], [
        ("null input", av(s, None, 0, 2, 6, 10, 8, 1.0, osp.ptr, 0, nul)), ("no image", av(s, src.ptr, 0, 0, 6, 10, 8, 1.0, osp.ptr, 0, nul)),
        ("odd height", av(s, src.ptr, 0, 2, 5, 10, 8, 1.0, osp.ptr, 0, nul)), ("odd width", av(s, src.ptr, 0, 2, 6, 9, 8, 1.0, osp.ptr, 0, nul)),
        ("one row", av(s, src.ptr, 0, 2, 1, 10, 8, 1.0, osp.ptr, 0, nul)), ("12 channels", av(s, src.ptr, 0, 2, 6, 10, 12, 1.0, osp.ptr, 0, nul)),
        ("input 4 bytes off", av(s, src.ptr + 4, 0, 2, 6, 10, 8, 1.0, osp.ptr, 0, nul)),
        ("input image pitch", av(s, src.ptr, 6 * 10 * 48 + 4, 2, 6, 10, 8, 1.0, osp.ptr, 0, nul)),
        ("both results", av(s, src.ptr, 0, 2, 6, 10, 8, 1.0, osp.ptr, 0, to.view())), ("no result", av(s, src.ptr, 0, 2, 6, 10, 8, 1.0, None, 0, nul)),
        ("split output 4 bytes off", av(s, src.ptr, 0, 2, 6, 10, 8, 1.0, osp.ptr + 4, 0, nul)),
        ("split output image pitch", av(s, src.ptr, 0, 2, 6, 10, 8, 1.0, osp.ptr, 3 * 5 * 48 + 4, nul)),
        ("fp32 output: images", av(s, src.ptr, 0, 2, 6, 10, 8, 1.0, None, 0, _v(to, n=1))),
        ("fp32 output: height", av(s, src.ptr, 0, 2, 6, 10, 8, 1.0, None, 0, _v(to, h=6))),
        ("fp32 output: width", av(s, src.ptr, 0, 2, 6, 10, 8, 1.0, None, 0, _v(to, w=4))),
        ("fp32 output: channels", av(s, src.ptr, 0, 2, 6, 10, 8, 1.0, None, 0, _v(to, c=4))),
        ("fp32 output 4 bytes off", av(s, src.ptr, 0, 2, 6, 10, 8, 1.0, None, 0, off1.view())),
        ("fp32 output: pixel stride 9", av(s, src.ptr, 0, 2, 6, 10, 8, 1.0, None, 0, _v(to, sw=9))),
    ])


# ------------------------------------------------------------------------------------------------
# axpby
# ------------------------------------------------------------------------------------------------
def _axpby(dev, case):
    from vcamd import hip
    shape = (case.n, case.c, case.h, case.w)
    a, b = rr.axpby_inputs(case.c, case.n, case.h, case.w)
    ta, tb = rr.place(a, dev, **case.a), rr.place(b, dev, seed=1, **case.b)
    ga, gb = _as_geom(ta, shape, case.a), _as_geom(tb, shape, case.b)
    for with_b in (True, False):
        to = _out(shape, dev, case.out)
        assert rr.axpby_form(ga, gb if with_b else None, _as_geom(to, shape, case.out)) == case.form
        _ok(hip.lib().vc_axpby(hip.stream(), ta.view(), tb.view() if with_b else _null(), to.view(), rr.ALPHA, rr.BETA), "vc_axpby")
        _finish("vc_axpby", f"{case.id} b={with_b}", to, rr.axpby(a, b if with_b else None, rr.ALPHA, rr.BETA), rr.CAP_LINEAR)


@pytest.mark.parametrize("case", rr.AXPBY_CASES, ids=_ids)
def test_axpby_every_form(dev, case):
    """dense rows ([h][w][c] read as [h][w c / 4][4]), k_axpby_v4 per pixel, k_axpby; with and without b; windows"""
    _axpby(dev, case)


@pytest.mark.parametrize("case", rr.AXPBY_ROWMAP, ids=_ids)
def test_axpby_row_map(dev, case):
    m = rr.rowmap(case.n, case.h, rr.axpby_width(case), rr.axpby_per_px(case))
    assert m is not None and m.reciprocal and not m.loops
    _axpby(dev, case)


def test_axpby_row_loop(dev):
    """64 images x 2 workgroups a row -> gridDim.y = 64 < h = 70: rows 64 .. 69 come from the second pass of `y += gridDim.y`"""
    case = rr.AXPBY_ROWLOOP
    m = rr.rowmap(case.n, case.h, case.w, case.c)
    assert m.loops and m.gy == 64 < case.h
    _axpby(dev, case)


@pytest.mark.parametrize("case", rr.AXPBY_FALLBACK, ids=_ids)
def test_axpby_linear_fallback(dev, case):
    assert rr.rowmap(case.n, case.h, rr.axpby_width(case), rr.axpby_per_px(case)) is None
    _axpby(dev, case)


def test_axpby_reads_the_top_left_of_larger_inputs(dev):
    """a and b may be larger than the output in every direction but n: the kernel reads their top-left window"""
    from vcamd import hip
    a, b = rr.rand((2, 7, 5, 9), 5), rr.rand((2, 6, 4, 8), 6)
    ta, tb, to = rr.place(a, dev), rr.place(b, dev), _out((2, 5, 3, 7), dev, rr.WIN_U)
    _ok(hip.lib().vc_axpby(hip.stream(), ta.view(), tb.view(), to.view(), rr.ALPHA, rr.BETA), "vc_axpby")
    _finish("vc_axpby", "larger inputs", to, rr.axpby(a[:, :5, :3, :7], b[:, :5, :3, :7], rr.ALPHA, rr.BETA), rr.CAP_LINEAR)


def test_axpby_refusals(dev):
    from vcamd import hip
    L, s = hip.lib(), hip.stream()
    x = rr.rand((2, 4, 5, 7), 7)
    ta, tb, to = rr.place(x, dev), rr.place(x, dev), _out((2, 4, 5, 7), dev, {})
    ax = L.vc_axpby
    calls = [("null a", ax(s, _null(2, 5, 7, 4), tb.view(), to.view(), 1.0, 1.0)), ("null output", ax(s, ta.view(), tb.view(), _null(2, 5, 7, 4), 1.0, 1.0))]
    for name, over in (("lower", dict(h=4)), ("narrower", dict(w=6)), ("fewer channels", dict(c=3)), ("another image count", dict(n=1)), ("more images", dict(n=3))):
        calls.append((f"a {name}", ax(s, _v(ta, **over), tb.view(), to.view(), 1.0, 1.0)))
        calls.append((f"a {name}, no b", ax(s, _v(ta, **over), _null(), to.view(), 1.0, 1.0)))
        calls.append((f"b {name}", ax(s, ta.view(), _v(tb, **over), to.view(), 1.0, 1.0)))
    _refused([to], calls)


# ------------------------------------------------------------------------------------------------
# SPyNet level input
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def default_level_form():
    for name in ("VC_LI_FORM", "VC_LI_VARIANT"):
        if os.environ.get(name):
            pytest.skip(f"{name} is set: these tests hold the default forms of the level input")


def _level_views(dev, coarse, h, w, n, first=rr.DENSE, second=rr.DENSE, fc=rr.DENSE):
    a, b, flow = rr.level_inputs(coarse, h, w, n)
    tf, ts = rr.place(a, dev, **first), rr.place(b, dev, seed=1, **second)
    tc = rr.place(flow, dev, seed=2, **fc) if flow is not None else None
    fcv = tc.view() if tc is not None else _null(n, h // 2, w // 2, 2)
    return (a, b, flow), (tf, ts, tc), fcv


def _hold_level(what, win, up_win, ins, ref_feat, ref_up):
    assert torch.equal(win[:, :3].double(), ins[0].double()), f"{what}: the first frame's channels are a copy"
    _hold("vc_spynet_level_input, warped", what, win[:, 3:6], ref_feat[:, 3:6], rr.CAP_WARP)
    _hold("vc_spynet_level_input, up", what, up_win, ref_up, rr.CAP_LINEAR)
    assert torch.equal(rr.bits(win[:, 6:8].float()), rr.bits(up_win)), f"{what}: channels 6, 7 and `up` hold the same flow"


@pytest.mark.parametrize("case", rr.LEVEL_CASES, ids=_ids)
def test_level_input_every_form(dev, default_level_form, case):
    """k_spynet_level_input<VEC>: no coarse flow, an even level, a level odd in h only, in w only, in both (replicate padding of the
    up-sampled flow), n = 1 and 2; scalar by a misaligned `feat` (channels 1 .. 8 of 12) or `up` at an odd float offset"""
    from vcamd import hip
    n, h, w = case.n, case.h, case.w
    ins, keep, fcv = _level_views(dev, case.coarse, h, w, n, case.first, case.second, case.fc)
    ref_feat, ref_up = rr.level_input(*ins)
    feat, up = _out((n, 8, h, w), dev, case.feat), _out((n, 2, h, w), dev, case.up)
    assert rr.level_input_form(_as_geom(feat, (n, 8, h, w), case.feat), _as_geom(up, (n, 2, h, w), case.up)) == case.form
    _ok(hip.lib().vc_spynet_level_input(hip.stream(), keep[0].view(), keep[1].view(), fcv, feat.view(), up.view()), "vc_spynet_level_input")
    win, outside = rr.read_window(feat)
    rr.assert_untouched(outside)
    up_win, outside = rr.read_window(up)
    rr.assert_untouched(outside)
    _hold_level(case.id, win, up_win, ins, ref_feat, ref_up)


@pytest.mark.parametrize("name,coarse,h,w", rr.LEVEL_SHAPES, ids=[s[0] for s in rr.LEVEL_SHAPES])
@pytest.mark.parametrize("n", [1, 2])
def test_level_input_split_record(dev, default_level_form, name, coarse, h, w, n):
    """vc_spynet_level_input_sp3 (default form): the record is bit for bit vc_split3 of the fp32 form's eight channels, within the
    caps of float64 through unsplit, `up` the same bits; nothing behind the last record is written.

    This equality did not hold before sample_bilinear<PIN>: channel 5, the third warped channel, differed by one ulp at 4-19 % of
    the pixels, because the compiler contracted the sum of that channel differently in the two instantiations."""
    from vcamd import hip
    L, s = hip.lib(), hip.stream()
    ins, keep, fcv = _level_views(dev, coarse, h, w, n, rr.WIN_U, rr.WIN_A, rr.WIN_U)
    ref_feat, ref_up = rr.level_input(*ins)
    records = n * h * w * 24
    buf = torch.full((records + 64,), 0x7f7f, dtype=torch.int16, device=dev)
    sp = hip.T(buf, n, h, w, 8, 1, 0, 0, 0, "sp3")
    up_spec = dict(c0=2, cpad=2, hpad=1, wpad=1, n0=1, npad=1)
    up = _out((n, 2, h, w), dev, up_spec)
    _ok(L.vc_spynet_level_input_sp3(s, keep[0].view(), keep[1].view(), fcv, sp.ptr, up.view()), "vc_spynet_level_input_sp3")
    assert bool((buf[records:] == 0x7f7f).all())
    up_win, outside = rr.read_window(up)
    rr.assert_untouched(outside)
    _hold_level(f"sp3 {name} n={n}", rr.unsplit(buf[:records], n, 8, h, w), up_win, ins, ref_feat, ref_up)
    feat32, up32 = hip.T.empty(n, h, w, 8, dev), hip.T.empty(n, h, w, 2, dev)
    assert rr.level_input_form(rr.geom((n, 8, h, w)), rr.geom((n, 2, h, w))) == "vec"
    _ok(L.vc_spynet_level_input(s, keep[0].view(), keep[1].view(), fcv, feat32.view(), up32.view()), "vc_spynet_level_input")
    assert torch.equal(rr.bits(hip.nhwc_to_nchw(up32).cpu()), rr.bits(up_win))
    got32 = hip.nhwc_to_nchw(feat32).cpu().double()
    differ = (rr.unsplit(buf[:records], n, 8, h, w) != got32).sum(dim=(0, 2, 3)).tolist()
    print(f"sp3 {name} n={n}: values differing from the fp32 form, per channel: {differ}")
    assert torch.equal(hip.split3(feat32).buf, buf[:records]), f"values differing from the fp32 form, per channel: {differ}"


def test_level_input_refusals(dev, default_level_form):
    from vcamd import hip
    L, s = hip.lib(), hip.stream()
    n, h, w = 2, 9, 19
    ins, (tf, ts, tc), fcv = _level_views(dev, (4, 9), h, w, n)
    feat, up = _out((n, 8, h, w), dev, {}), _out((n, 2, h, w), dev, {})
    li = L.vc_spynet_level_input
    bad_fc = [("three channels", dict(c=3)), ("too low", dict(h=3)), ("too high", dict(h=5)), ("too narrow", dict(w=8)), ("too wide", dict(w=10))]
    _refused([feat, up], [
        ("null first", li(s, _null(n, h, w, 3), ts.view(), fcv, feat.view(), up.view())),
        ("null second", li(s, tf.view(), _null(n, h, w, 3), fcv, feat.view(), up.view())),
        ("null feat", li(s, tf.view(), ts.view(), fcv, _null(n, h, w, 8), up.view())),
        ("null up", li(s, tf.view(), ts.view(), fcv, feat.view(), _null(n, h, w, 2))),
        ("first of 2 channels", li(s, _v(tf, c=2), ts.view(), fcv, feat.view(), up.view())),
        ("second of 2 channels", li(s, tf.view(), _v(ts, c=2), fcv, feat.view(), up.view())),
        ("feat of 7 channels", li(s, tf.view(), ts.view(), fcv, _v(feat, c=7), up.view())),
        ("up of 1 channel", li(s, tf.view(), ts.view(), fcv, feat.view(), _v(up, c=1))),
        ("first lower", li(s, _v(tf, h=8), ts.view(), fcv, feat.view(), up.view())),
        ("first narrower", li(s, _v(tf, w=18), ts.view(), fcv, feat.view(), up.view())),
        ("second lower", li(s, tf.view(), _v(ts, h=8), fcv, feat.view(), up.view())),
        ("second narrower", li(s, tf.view(), _v(ts, w=18), fcv, feat.view(), up.view())),
        ("up lower", li(s, tf.view(), ts.view(), fcv, feat.view(), _v(up, h=8))),
        ("up narrower", li(s, tf.view(), ts.view(), fcv, feat.view(), _v(up, w=18))),
    ] + [(f"coarse flow {name}", li(s, tf.view(), ts.view(), _v(tc, **over), feat.view(), up.view())) for name, over in bad_fc])
    sp = _guarded_split(n, h, w, 8, dev, rr.SENTINEL)
    odd = _out((n, 2, h, w), dev, dict(c0=1, cpad=1))
    ls = L.vc_spynet_level_input_sp3
    _refused([sp, up, odd], [
        ("null first", ls(s, _null(n, h, w, 3), ts.view(), fcv, sp.ptr, up.view())),
        ("null second", ls(s, tf.view(), _null(n, h, w, 3), fcv, sp.ptr, up.view())),
        ("null record", ls(s, tf.view(), ts.view(), fcv, None, up.view())),
        ("null up", ls(s, tf.view(), ts.view(), fcv, sp.ptr, _null(n, h, w, 2))),
        ("record 8 bytes off", ls(s, tf.view(), ts.view(), fcv, sp.ptr + 8, up.view())),
        ("first of 2 channels", ls(s, _v(tf, c=2), ts.view(), fcv, sp.ptr, up.view())),
        ("second of 4 channels", ls(s, tf.view(), _v(ts, c=4), fcv, sp.ptr, up.view())),
        ("up of 3 channels", ls(s, tf.view(), ts.view(), fcv, sp.ptr, _v(up, c=3))),
        ("second lower", ls(s, tf.view(), _v(ts, h=8), fcv, sp.ptr, up.view())),
        ("second narrower", ls(s, tf.view(), _v(ts, w=18), fcv, sp.ptr, up.view())),
        ("up lower", ls(s, tf.view(), ts.view(), fcv, sp.ptr, _v(up, h=8))),
        ("up narrower", ls(s, tf.view(), ts.view(), fcv, sp.ptr, _v(up, w=18))),
        ("up of another image count", ls(s, tf.view(), ts.view(), fcv, sp.ptr, _v(up, n=1))),
        ("up at an odd float offset", ls(s, tf.view(), ts.view(), fcv, sp.ptr, odd.view())),
        ("up with an odd pixel stride", ls(s, tf.view(), ts.view(), fcv, sp.ptr, _v(up, sw=3))),
    ] + [(f"coarse flow {name}", ls(s, tf.view(), ts.view(), _v(tc, **over), sp.ptr, up.view())) for name, over in bad_fc])
