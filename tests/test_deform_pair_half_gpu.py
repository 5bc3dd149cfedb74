"""-m gpu: vc_deform_pair_hxp (csrc/deform.hip: k_deform<cg, cg, MODE_PAIR, true, 4, 512, true>, cg = 4, 8, 12), the deformable pair of
ICIP2023's DeformB on group-planar HALF features, and its route through hip.PackedDeform.pair in fp16 mode.

Bounds: against the float64 oracle on features rounded to half beforehand, |out - ref| / (1 + |ref|) < deform_ref.CAP_FUSED (5e-5, the
project's bound of the fused half-feature forms); against the fp32 vc_deform_pair on the same half-rounded features < 1e-6
(deform_ref.CAP_HALF_VS_F32: the two instances differ in the choice of fused multiply-adds only).  Sentinels, bit equalities, call
counts and return codes are exact."""
import functools

import pytest
import torch

import deform_ref as dr
from test_deform_pair_gpu import pair_inputs, ref_pair

pytestmark = pytest.mark.gpu
PAIRS = [(4, 4), (8, 8), (12, 12)]
GROUPS, N = 16, 2
# one pixel, one row, an exact 4 x 16 tile, one column past it, several tiles in both directions
SIZES = dr.SIZES + dr.TINY + [(5, 16), (5, 17), (27, 44)]
MAXIMA = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda:0")
    for k in sorted(MAXIMA):
        print(f"\nlargest error seen, {k}: {MAXIMA[k]:.2e}", end="")


@functools.lru_cache(maxsize=None)
def _case(cg, og, h, w):
    """inputs with the features rounded to half, and the float64 reference on them (with bias)"""
    x1, r1, x2, r2, wt, b = pair_inputs(cg, og, GROUPS, h, w, N)
    x1, x2 = x1.half().float(), x2.half().float()
    ref = ref_pair(x1, r1, x2, r2, wt, b)
    assert torch.isfinite(ref).all()
    return (x1, r1, x2, r2), wt, b, ref


def _hold(key, what, out, ref, cap):
    d = dr.rel_err(out, ref)
    MAXIMA[key] = max(MAXIMA.get(key, 0.0), d)
    print(f"{key} {what}: {d:.2e}")
    assert d < cap, f"{key} {what}: {d:.3e} >= {cap}"


class _Switches:
    """fp16 precision and the three VC_HALF_DEFORM* switches for the duration of a block"""

    def __init__(self, precision="fp16", deform=True, planar=True, pair=True):
        self.want = (precision, deform, planar, pair)

    def __enter__(self):
        from vcamd import hip
        self.keep = (hip.conv_precision(), hip.HALF_DEFORM, hip.HALF_DEFORM_PLANAR, hip.HALF_DEFORM_PAIR)
        hip.set_conv_precision(self.want[0])
        hip.HALF_DEFORM, hip.HALF_DEFORM_PLANAR, hip.HALF_DEFORM_PAIR = self.want[1:]

    def __exit__(self, *exc):
        from vcamd import hip
        hip.set_conv_precision(self.keep[0])
        hip.HALF_DEFORM, hip.HALF_DEFORM_PLANAR, hip.HALF_DEFORM_PAIR = self.keep[1:]


def _planes(t, cg, half):
    """(planar half copy -- kept alive by the caller --, the view of ONE group's plane)"""
    from vcamd import hip
    p = hip.to_half_planar(t, cg)
    return p, hip.View(p.ptr, t.n, t.h, t.w, cg, half * t.h * t.w * cg, t.w * cg, cg)


def _direct(pk, ts, out):
    from vcamd import hip
    cg, half = pk.cin // pk.groups, pk.groups // 2
    p1, v1 = _planes(ts[0], cg, half)
    p2, v2 = _planes(ts[2], cg, half)
    rc = hip.lib().vc_deform_pair_hxp(hip.stream(), v1, ts[1].view(), v2, ts[3].view(), pk.wpk.data_ptr(), pk._bias_ptr(), pk.groups, out.view())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("cg,og", PAIRS)
def test_against_float64_and_fp32_pair(dev, cg, og, h, w):
    """16 groups, n = 2, offsets ~ N(0, 1.5 px), with and without bias: the fp16 route of PackedDeform.pair against the float64
    oracle and against the fp32 vc_deform_pair on the same half-rounded features; the library call on a planar copy made by
    hip.to_half_planar gives the route's bits"""
    from vcamd import hip
    (x1, r1, x2, r2), wt, b, ref = _case(cg, og, h, w)
    ts = [dr.place(x1, dev), dr.place(r1, dev), dr.place(x2, dev, seed=1), dr.place(r2, dev, seed=1)]
    for bias in (b, None):
        pk = hip.PackedDeform(wt, bias, GROUPS, dev)
        want = ref if bias is not None else ref - b.double().view(1, -1, 1, 1)
        f32 = hip.nhwc_to_nchw(pk.pair(*ts)).cpu()
        with _Switches():
            out = hip.nhwc_to_nchw(pk.pair(*ts)).cpu()
        what = f"cg={cg} {h}x{w} bias={bias is not None}"
        _hold("half pair vs float64", what, out, want, dr.CAP_FUSED)
        _hold("half pair vs fp32 pair", what, out, f32, dr.CAP_HALF_VS_F32)
        direct = hip.T.empty(N, h, w, og * GROUPS, dev)
        assert _direct(pk, ts, direct) == hip.VC_OK
        assert torch.equal(dr.bits(hip.nhwc_to_nchw(direct).cpu()), dr.bits(out))


@pytest.mark.parametrize("h,w", [dr.SIZES[0], (5, 17)])
@pytest.mark.parametrize("cg,og", PAIRS)
def test_on_windows_writes_only_its_window(dev, cg, og, h, w):
    """features as channel windows of ONE wider buffer per reference slot (the model's [fref1 | fref2 | fcur] layout at pixel stride
    3c), ``out`` a channel window of a wider sentinel-filled buffer: the dense call's bits, and nothing outside the window is written"""
    from vcamd import hip
    (x1, r1, x2, r2), wt, b, ref = _case(cg, og, h, w)
    c = 8 * cg
    pk = hip.PackedDeform(wt, b, GROUPS, dev)
    ts = [dr.place(x1, dev, c0=0, cpad=2 * c), dr.place(r1, dev, c0=4, cpad=8), dr.place(x2, dev, c0=c, cpad=2 * c, seed=1),
          dr.place(r2, dev, c0=0, cpad=4, seed=1)]
    out = dr.place(torch.full(ref.shape, dr.SENTINEL), dev, fill=dr.SENTINEL, c0=4, cpad=8, hpad=1, wpad=2, n0=1, npad=2)
    calls = []
    orig = hip.to_half_planar
    hip.to_half_planar = lambda t, g: (calls.append((t.c, g)), orig(t, g))[1]
    try:
        with _Switches():
            pk.pair(*ts, out=out)
            dense = hip.nhwc_to_nchw(pk.pair(dr.place(x1, dev), dr.place(r1, dev), dr.place(x2, dev), dr.place(r2, dev))).cpu()
    finally:
        hip.to_half_planar = orig
    assert calls == [(c, cg)] * 4
    got, outside = dr.read_window(out)
    dr.assert_untouched(outside)
    _hold("half pair vs float64", f"cg={cg} windows {h}x{w}", got, ref, dr.CAP_FUSED)
    assert torch.equal(dr.bits(got), dr.bits(dense))


def test_routing_follows_precision_and_switches(dev):
    """fp32 precision: no conversion launch and the bits of a plain vc_deform_pair call; fp16 with every switch set: to_half_planar
    exactly twice; with any one of HALF_DEFORM / HALF_DEFORM_PLANAR / HALF_DEFORM_PAIR off: never, and the fp32 call's bits"""
    from vcamd import hip
    cg, og = 8, 8
    h, w = dr.SIZES[0]
    (x1, r1, x2, r2), wt, b, ref = _case(cg, og, h, w)
    pk = hip.PackedDeform(wt, b, GROUPS, dev)
    ts = [dr.place(t, dev) for t in (x1, r1, x2, r2)]
    plain = hip.T.empty(N, h, w, og * GROUPS, dev)
    assert hip.lib().vc_deform_pair(hip.stream(), ts[0].view(), ts[1].view(), ts[2].view(), ts[3].view(), pk.wpk.data_ptr(), pk._bias_ptr(),
                                    GROUPS, plain.view()) == hip.VC_OK
    plain = dr.bits(hip.nhwc_to_nchw(plain).cpu())
    calls = []
    orig, orig_h = hip.to_half_planar, hip.to_half
    hip.to_half_planar = lambda t, g: (calls.append("planar"), orig(t, g))[1]
    hip.to_half = lambda t: (calls.append("interleaved"), orig_h(t))[1]
    try:
        assert hip.conv_precision() == "fp32"
        assert torch.equal(dr.bits(hip.nhwc_to_nchw(pk.pair(*ts)).cpu()), plain) and not calls
        with _Switches():
            on = hip.nhwc_to_nchw(pk.pair(*ts)).cpu()
            assert calls == ["planar"] * 2
        _hold("half pair vs float64", "routing", on, ref, dr.CAP_FUSED)
        for off in ("deform", "planar", "pair"):
            del calls[:]
            with _Switches(**{off: False}):
                got = hip.nhwc_to_nchw(pk.pair(*ts)).cpu()
            assert not calls, off
            assert torch.equal(dr.bits(got), plain), off
    finally:
        hip.to_half_planar, hip.to_half = orig, orig_h
    assert hip.conv_precision() == "fp32"


def _copy(v, **fields):
    from vcamd import hip
    c = hip.View.from_buffer_copy(v)
    for k, val in fields.items():
        setattr(c, k, val)
    return c


def test_argument_contract(dev):
    """each bad call returns VC_EINVAL on the host, before any launch: the sentinel-filled output is untouched, and a valid call right
    after it succeeds with the first valid call's bits"""
    from vcamd import hip
    L = hip.lib()
    n, h, w, cg = N, 3, 5, 8
    half = GROUPS // 2
    x1, r1, x2, r2, wt, b = pair_inputs(cg, cg, GROUPS, h, w, n)
    pk = hip.PackedDeform(wt, b, GROUPS, dev)
    t1, tr1, t2, tr2 = (dr.place(t, dev) for t in (x1, r1, x2, r2))
    p1, v1 = _planes(t1, cg, half)
    p2, v2 = _planes(t2, cg, half)
    # raw tensors as windows 1 / 2 floats into a 4-channel-wider buffer: pointers 4 and 8 bytes off a 16-byte boundary
    raw_off4, raw_off8 = dr.place(r1, dev, c0=1, cpad=4), dr.place(r1, dev, c0=2, cpad=4)
    # planes of 4 / 16 channels per group in the same memory (never read: refused on the host)
    thin = hip.View(p1.ptr, n, h, w, 4, half * h * w * 4, w * 4, 4)
    wide = hip.View(p1.ptr, n, h, w, 16, half * h * w * 16, w * 16, 16)
    v = [v1, tr1.view(), v2, tr2.view()]

    def call(v=v, groups=GROUPS, wpk=pk.wpk.data_ptr(), out=None, **out_fields):
        return L.vc_deform_pair_hxp(hip.stream(), v[0], v[1], v[2], v[3], wpk, pk._bias_ptr(), groups, _copy(out.view(), **out_fields))

    def sub(i, **fields):
        vv = list(v)
        vv[i] = _copy(v[i], **fields)
        return vv

    def sentinel_out():
        return dr.place(torch.full((n, 160, h, w), dr.SENTINEL), dev, fill=dr.SENTINEL)

    first = sentinel_out()
    assert call(out=first, c=128) == hip.VC_OK
    torch.cuda.synchronize()
    want = first.to_nchw()[:, :128].cpu()
    _hold("half pair vs float64", "contract shape", want, ref_pair(x1.half().float(), r1, x2.half().float(), r2, wt, b), dr.CAP_FUSED)
    r9 = hip.View(tr1.view().p, n, h, w, 27 * 9, tr1.view().sn, tr1.view().sh, tr1.view().sw)
    bad = {
        "null x1": dict(v=sub(0, p=None)), "null raw1": dict(v=sub(1, p=None)), "null x2": dict(v=sub(2, p=None)),
        "null raw2": dict(v=sub(3, p=None)), "null weights": dict(wpk=None), "null out": dict(p=None),
        "odd groups": dict(groups=15), "groups = 0": dict(groups=0),
        "raw1 channels != 27 * groups / 2": dict(v=sub(1, c=215)), "raw2 channels != 27 * groups / 2": dict(v=sub(3, c=217)),
        "x1: pixel stride != cg": dict(v=sub(0, sw=cg + 4)), "x2: row stride != w * cg": dict(v=sub(2, sh=(w + 1) * cg)),
        "x1: image stride of ONE plane": dict(v=sub(0, sn=h * w * cg)), "x2: padded image stride": dict(v=sub(2, sn=half * h * w * cg + 8)),
        "x1.c != x2.c": dict(v=[v[0], v[1], thin, v[3]]),
        "x1 height": dict(v=sub(0, h=h - 1)), "x2 width": dict(v=sub(2, w=w + 1)), "raw1 width": dict(v=sub(1, w=w - 1)),
        "raw2 height": dict(v=sub(3, h=h + 1)), "x1 batch": dict(v=sub(0, n=1)), "raw2 batch": dict(v=sub(3, n=3)),
        "raw1 4 bytes off (no RV < 4 half instance)": dict(v=[v[0], raw_off4.view(), v[2], v[3]]),
        "raw2 8 bytes off": dict(v=[v[0], v[1], v[2], raw_off8.view()]),
        "x1 4 bytes off": dict(v=sub(0, p=p1.ptr + 4)), "x2 4 bytes off": dict(v=sub(2, p=p2.ptr + 4)),
        "(cg, og) = (8, 4)": dict(c=64),
        "(cg, og) = (16, 8)": dict(v=[wide, v[1], wide, v[3]]),
        "18 groups": dict(groups=18, v=[v[0], r9, v[2], r9], c=144),
    }
    for what, kw in bad.items():
        out = sentinel_out()
        out_fields = {"c": kw.pop("c", 128)}
        if "p" in kw:
            out_fields["p"] = kw.pop("p")
        assert call(out=out, **kw, **out_fields) == -1, what
        torch.cuda.synchronize()
        win, outside = dr.read_window(out)
        dr.assert_untouched(win.flatten())
        dr.assert_untouched(outside)
        assert call(out=out, c=128) == hip.VC_OK, f"valid call after: {what}"
        torch.cuda.synchronize()
        assert torch.equal(dr.bits(out.to_nchw()[:, :128].cpu()), dr.bits(want)), what
