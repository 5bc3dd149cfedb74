"""-m gpu: every form of csrc/deform.hip's k_deform<CG, OG, MODE, VEC, RV, MAXT, XH> that the launcher can select, against the
float64 oracle (tests/deform_ref.py; pinned on the CPU by tests/test_deform_cpu.py).  The forms are reached by shaping the views --
alignment, strides, group count, record length -- and every case says in a comment which instance it runs.

Bounds: |out - ref| / (1 + |ref|) < 2e-5 (vc_deform_conv2d) / 5e-5 (vc_offset_diversity and its half-feature forms, the latter
against the reference on features rounded to half); half-feature instance against the fp32 instance on half-rounded features 1e-6.
Everything else -- sentinels, bit equalities, bias-only pixels, return codes -- is exact."""
import ctypes
import functools

import pytest
import torch

import deform_ref as dr

pytestmark = pytest.mark.gpu
MAG = dr.FUSED_MAGNITUDE
MAXIMA = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda:0")
    for k in sorted(MAXIMA):
        print(f"\nlargest error seen, {k}: {MAXIMA[k]:.2e}", end="")


def _hold(entry, what, out, ref, cap):
    d = dr.rel_err(out, ref)
    MAXIMA[entry] = max(MAXIMA.get(entry, 0.0), d)
    print(f"{entry} {what}: {d:.2e}")
    assert d < cap, f"{entry} {what}: {d:.3e} >= {cap}"


# how the features reach the kernel: `vec` dense and 16-byte aligned (VEC = true); `scalar` channels [1, 1 + c) of a buffer 4
# channels wider, the pointer 4 bytes off (VEC = false); `stride` an aligned pointer with a pixel stride of c + 1 floats (VEC = false)
X_FORMS = {"vec": {}, "scalar": dict(c0=1, cpad=4), "stride": dict(c0=0, cpad=1)}
# the raw offset tensors of the fused entry: windows of buffers 4 channels wider starting at channel 0 / 2 / 1 allow record pieces
# of RV = 4 / 2 / 1 floats (as far as the record length 27 * groups / 2 divides)
RAW_FORMS = {"dense": {}, "rv4": dict(c0=0, cpad=4), "rv2": dict(c0=2, cpad=4), "rv1": dict(c0=1, cpad=4)}


@functools.lru_cache(maxsize=None)
def _generic_case(cg, og, groups, h, w):
    """inputs and the float64 references {(mask?, bias?)}; without bias = with bias minus the bias, exact enough in float64"""
    x, off, msk, wt, b = dr.generic_inputs(cg, og, groups, h, w)
    rm, rn = dr.ref_generic(x, off, wt, b, msk), dr.ref_generic(x, off, wt, b, None)
    bb = b.double().view(1, -1, 1, 1)
    return (x, off, msk, wt, b), {(True, True): rm, (True, False): rm - bb, (False, True): rn, (False, False): rn - bb}


@functools.lru_cache(maxsize=None)
def _fused_case(cg, og, groups, h, w):
    *ins, wt, b = dr.fused_inputs(cg, og, groups, h, w)
    ref = dr.ref_fused(*ins, MAG, wt, b)
    assert torch.isfinite(ref).all()
    return tuple(ins), wt, b, ref


def _generic(dev, cg, og, groups, h, w, form):
    from vcamd import hip
    (x, off, msk, wt, b), refs = _generic_case(cg, og, groups, h, w)
    tx, to, tm = dr.place(x, dev, **X_FORMS[form]), dr.place(off, dev), dr.place(msk, dev)
    for with_bias in (True, False):
        pk = hip.PackedDeform(wt, b if with_bias else None, groups, dev)
        for with_mask in (True, False):
            out = hip.nhwc_to_nchw(pk.conv(tx, to, tm if with_mask else None)).cpu()
            _hold("vc_deform_conv2d", f"cg={cg} og={og} G={groups} {h}x{w} {form} mask={with_mask} bias={with_bias}", out,
                  refs[(with_mask, with_bias)], dr.CAP_GENERIC)


def _fused(dev, cg, og, groups, h, w, form, raw="dense", with_bias=True):
    from vcamd import hip
    (x1, r1, f1, x2, r2, f2), wt, b, ref = _fused_case(cg, og, groups, h, w)
    pk = hip.PackedDeform(wt, b if with_bias else None, groups, dev)
    out = pk.offset_diversity(dr.place(x1, dev, **X_FORMS[form]), dr.place(r1, dev, **RAW_FORMS[raw]), dr.place(f1, dev),
                              dr.place(x2, dev, seed=1, **X_FORMS[form]), dr.place(r2, dev, seed=1, **RAW_FORMS[raw]), dr.place(f2, dev), MAG)
    _hold("vc_offset_diversity", f"cg={cg} og={og} G={groups} {h}x{w} {form} raw={raw} bias={with_bias}", hip.nhwc_to_nchw(out).cpu(),
          ref if with_bias else ref - b.double().view(1, -1, 1, 1), dr.CAP_FUSED)


# ---- the seven channel pairs, vector and scalar ----
@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("form", ["vec", "scalar"])
@pytest.mark.parametrize("cg,og", dr.PAIRS)
def test_generic_channel_pairs(dev, cg, og, form, h, w):
    """8 groups, cin / cout = 32/16, 32/32, 64/32, 96/48, 128/64, 64/64, 128/32; with and without mask, with and without bias.
    vec: k_deform<cg, og, MODE_GENERIC, true, 1, 512>;  scalar: k_deform<cg, og, MODE_GENERIC, false, 1, 1024>"""
    _generic(dev, cg, og, 8, h, w, form)


@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("form", ["vec", "scalar"])
@pytest.mark.parametrize("cg,og", dr.PAIRS)
def test_fused_channel_pairs(dev, cg, og, form, h, w):
    """8 groups: records of 108 floats, dense raw tensors -> RV = 4.
    vec: k_deform<cg, og, MODE_OD, true, 4, 512>;  scalar: k_deform<cg, og, MODE_OD, false, 4, 1024>"""
    _fused(dev, cg, og, 8, h, w, form, with_bias=(h, w) == dr.SIZES[0] or og != 4)       # (bias == nullptr on some of them)


# ---- width of the record pieces ----
@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("form", ["vec", "scalar"])
@pytest.mark.parametrize("raw", ["rv4", "rv2", "rv1"])
def test_fused_record_width_by_alignment(dev, raw, form, h, w):
    """16 groups of 8 -> 4 channels (the ICIP2024 level-1 shape), records of 216 floats; the raw tensors' alignment decides RV.
    rv4: vec k_deform<8, 4, MODE_OD, true, 4, 512>, scalar <8, 4, MODE_OD, false, 4, 1024>
    rv2: vec k_deform<8, 4, MODE_OD, true, 2, 1024>, scalar <8, 4, MODE_OD, false, 2, 1024>
    rv1: vec k_deform<8, 4, MODE_OD, true, 1, 512> (single floats run 512 threads again: there is no <.., true, 2, 512> instance), scalar <8, 4, MODE_OD, false, 1, 1024>"""
    _fused(dev, 8, 4, 16, h, w, form, raw)


@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("form", ["vec", "scalar"])
@pytest.mark.parametrize("groups", [4, 2, 6])
def test_fused_record_width_by_length(dev, groups, form, h, w):
    """dense, aligned raw tensors whose record length alone limits the pieces: 4 groups (54 floats: RV = 2), 2 groups (27: RV = 1,
    ONE wave per workgroup), 6 groups (81: RV = 1, three waves, odd record arithmetic).
    G = 4: vec k_deform<8, 4, MODE_OD, true, 2, 1024>, scalar <8, 4, MODE_OD, false, 2, 1024>
    G = 2, 6: vec k_deform<8, 4, MODE_OD, true, 1, 512>, scalar <8, 4, MODE_OD, false, 1, 1024>"""
    _fused(dev, 8, 4, groups, h, w, form)


@pytest.mark.parametrize("groups", [2, 6])
def test_generic_one_and_three_waves(dev, groups):
    """half = 1 and 3 on the generic entry: k_deform<8, 4, MODE_GENERIC, true, 1, 512> / <8, 4, MODE_GENERIC, false, 1, 1024>"""
    for form in ("vec", "scalar"):
        _generic(dev, 8, 4, groups, 9, 19, form)


# ---- more than 8 groups per half: 1024-thread instances ----
@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("form", ["vec", "scalar"])
@pytest.mark.parametrize("cg,og,groups", [(8, 4, 20), (4, 2, 32)])
def test_generic_1024_threads(dev, cg, og, groups, form, h, w):
    """20 groups (160 -> 80 channels, 640 threads) and 32 groups (128 -> 64, 1024 threads).
    vec: k_deform<cg, og, MODE_GENERIC, true, 1, 1024>;  scalar: k_deform<cg, og, MODE_GENERIC, false, 1, 1024>"""
    _generic(dev, cg, og, groups, h, w, form)


@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("form", ["vec", "scalar"])
@pytest.mark.parametrize("cg,og,groups,raw", [(8, 4, 20, "dense"), (4, 2, 32, "dense"), (4, 2, 32, "rv1")])
def test_fused_1024_threads(dev, cg, og, groups, raw, form, h, w):
    """20 groups: records of 270 floats -> RV = 2: vec k_deform<8, 4, MODE_OD, true, 2, 1024>, scalar <8, 4, MODE_OD, false, 2, 1024>.
    32 groups: 432 floats -> RV = 4: vec k_deform<4, 2, MODE_OD, true, 4, 1024>, scalar <4, 2, MODE_OD, false, 4, 1024> -- 115 456 bytes of
    dynamic LDS at 1024 threads, above 64 KiB: through hipFuncSetAttribute.  The same with raw tensors 4 bytes off:
    vec k_deform<4, 2, MODE_OD, true, 1, 1024>, scalar <4, 2, MODE_OD, false, 1, 1024>."""
    _fused(dev, cg, og, groups, h, w, form, raw)


# ---- one-pixel and one-row images, the third feature form ----
@pytest.mark.parametrize("h,w", dr.TINY)
@pytest.mark.parametrize("form", ["vec", "scalar"])
def test_one_pixel_and_one_row(dev, form, h, w):
    """1 x 1 and 1 x 17: every sample has y0 = -1 or y1 = H.  generic k_deform<8, 4, MODE_GENERIC, VEC, 1, 512 | 1024> at 8 groups, fused
    k_deform<8, 4, MODE_OD, VEC, 4, 512 | 1024> at 16"""
    _generic(dev, 8, 4, 8, h, w, form)
    _fused(dev, 8, 4, 16, h, w, form)


@pytest.mark.parametrize("h,w", dr.SIZES)
def test_aligned_pointer_with_odd_pixel_stride_is_scalar(dev, h, w):
    """features at a 16-byte-aligned pointer but sw = c + 1: k_deform<8, 4, MODE_GENERIC, false, 1, 1024> and <8, 4, MODE_OD, false, 4, 1024>"""
    _generic(dev, 8, 4, 8, h, w, "stride")
    _fused(dev, 8, 4, 16, h, w, "stride")


# ---- half-precision features ----
def _lib_fused(dev, fn, v1, t_r1, t_f1, v2, t_r2, t_f2, pk, out, groups=None):
    from vcamd import hip
    return fn(hip.stream(), v1, t_r1.view(), t_f1.view(), v2, t_r2.view(), t_f2.view(), MAG, pk.wpk.data_ptr(), pk._bias_ptr(),
              pk.groups if groups is None else groups, out.view())


def _planar(x, cg, dev):
    """host-made group-planar half copy [n][G/2][h][w][cg] and the view of ONE group's plane (include/vc_hip.h)"""
    from vcamd import hip
    n, c, h, w = x.shape
    p = x.half().view(n, c // cg, cg, h, w).permute(0, 1, 3, 4, 2).contiguous().to(dev)
    return p, hip.View(p.data_ptr(), n, h, w, cg, (c // cg) * h * w * cg, w * cg, cg)


@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("cg,og", dr.PAIRS)
def test_half_features_every_pair(dev, cg, og, h, w):
    """vc_offset_diversity_hx (x_half = 1) and _hxp (x_half = 2), n = 2, 8 groups: k_deform<cg, og, MODE_OD, true, 4, 512, true>.
    cg = 4: ONE 8-byte gather per corner (V = 1 with TAIL8); 12: a 16-byte and an 8-byte one; 8, 16: one / two 16-byte ones.
    The Python gate asks cg >= 8, so the entry points are called directly."""
    from vcamd import hip
    L = hip.lib()
    (x1, r1, f1, x2, r2, f2), wt, b, _ = _fused_case(cg, og, 8, h, w)
    ref = dr.ref_fused(x1, r1, f1, x2, r2, f2, MAG, wt, b, half_features=True)
    pk = hip.PackedDeform(wt, b, 8, dev)
    rest = [dr.place(t, dev) for t in (r1, f1, r2, f2)]
    outs = {}
    for name, fn in (("hx", L.vc_offset_diversity_hx), ("hxp", L.vc_offset_diversity_hxp)):
        out = dr.place(torch.full(ref.shape, dr.SENTINEL), dev, fill=dr.SENTINEL)
        if name == "hx":
            keep = (dr.place(x1, dev, half=True), dr.place(x2, dev, half=True))
            v1, v2 = keep[0].view(True), keep[1].view(True)
        else:
            (p1, v1), (p2, v2) = _planar(x1, cg, dev), _planar(x2, cg, dev)
        assert _lib_fused(dev, fn, v1, rest[0], rest[1], v2, rest[2], rest[3], pk, out) == hip.VC_OK
        outs[name] = dr.read_window(out)[0]
        _hold("vc_offset_diversity_" + name, f"cg={cg} og={og} {h}x{w}", outs[name], ref, dr.CAP_FUSED)
    assert torch.equal(dr.bits(outs["hx"]), dr.bits(outs["hxp"]))
    # the fp32 instance on features rounded to half beforehand: the same values, fp32 everywhere else
    f32 = hip.nhwc_to_nchw(pk.offset_diversity(dr.place(x1.half().float(), dev), rest[0], rest[1], dr.place(x2.half().float(), dev),
                                               rest[2], rest[3], MAG)).cpu()
    d = dr.rel_err(outs["hx"], f32)
    print(f"half-feature instance against the fp32 instance cg={cg} og={og} {h}x{w}: {d:.2e}")
    assert d < dr.CAP_HALF_VS_F32


@pytest.mark.parametrize("c0,cpad", [(0, 8), (4, 8)])
@pytest.mark.parametrize("cg,og", [(4, 2), (8, 4), (12, 6)])
def test_half_features_as_a_channel_window(dev, cg, og, c0, cpad):
    """_hx on features that are channels [c0, c0 + c) of a half buffer 8 channels wider (sw != c): k_deform<cg, og, MODE_OD, true, 4, 512, true>.
    c0 = 4: the pointer is 8 bytes off a 16-byte boundary -- the rule of dispatch's aligned8h is 8 bytes (pointer and strides whole
    groups of four halves), which is all the 8- and 16-byte gathers need.  Bit-equal to the dense features' result."""
    from vcamd import hip
    L = hip.lib()
    h, w = dr.SIZES[0]
    (x1, r1, f1, x2, r2, f2), wt, b, _ = _fused_case(cg, og, 8, h, w)
    ref = dr.ref_fused(x1, r1, f1, x2, r2, f2, MAG, wt, b, half_features=True)
    pk = hip.PackedDeform(wt, b, 8, dev)
    rest = [dr.place(t, dev) for t in (r1, f1, r2, f2)]
    got = []
    for kw in (dict(c0=c0, cpad=cpad), {}):
        t1, t2 = dr.place(x1, dev, half=True, **kw), dr.place(x2, dev, half=True, seed=1, **kw)
        assert t1.ptr % 16 == (2 * kw.get("c0", 0)) % 16 and t1.sw == x1.shape[1] + kw.get("cpad", 0)
        out = dr.place(torch.full(ref.shape, dr.SENTINEL), dev, fill=dr.SENTINEL)
        assert _lib_fused(dev, L.vc_offset_diversity_hx, t1.view(True), rest[0], rest[1], t2.view(True), rest[2], rest[3], pk, out) == hip.VC_OK
        got.append(dr.read_window(out)[0])
    _hold("vc_offset_diversity_hx", f"cg={cg} og={og} window c0={c0} of c+{cpad}", got[0], ref, dr.CAP_FUSED)
    assert torch.equal(dr.bits(got[0]), dr.bits(got[1]))


# ---- every tensor a window; stray stores ----
ALIGNED = dict(c0=4, cpad=8, hpad=3, wpad=4, n0=1, npad=2)      # starts and strides whole float4s: the vector form
ODD = dict(c0=3, cpad=5, hpad=2, wpad=3, n0=1, npad=2)          # the scalar form


@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("win", ["aligned", "odd"])
def test_generic_on_windows_writes_only_its_window(dev, win, h, w):
    """features, offsets, mask and output are channel slices of wider buffers, crops of larger ones and images [1, 3) of four.
    aligned: k_deform<8, 4, MODE_GENERIC, true, 1, 512>, bit-equal to the dense call (the same instance, the same arithmetic);
    odd: k_deform<8, 4, MODE_GENERIC, false, 1, 1024>.  Outside its window the output buffer keeps the sentinel bit for bit."""
    from vcamd import hip
    kw = ALIGNED if win == "aligned" else ODD
    (x, off, msk, wt, b), refs = _generic_case(8, 4, 8, h, w)
    pk = hip.PackedDeform(wt, b, 8, dev)
    out = dr.place(torch.full(refs[(True, True)].shape, dr.SENTINEL), dev, fill=dr.SENTINEL, **kw)
    pk.conv(dr.place(x, dev, **kw), dr.place(off, dev, seed=1, **kw), dr.place(msk, dev, seed=2, **kw), out=out)
    got, outside = dr.read_window(out)
    dr.assert_untouched(outside)
    _hold("vc_deform_conv2d", f"windows ({win}) {h}x{w}", got, refs[(True, True)], dr.CAP_GENERIC)
    if win == "aligned":
        dense = hip.nhwc_to_nchw(pk.conv(dr.place(x, dev), dr.place(off, dev), dr.place(msk, dev))).cpu()
        assert torch.equal(dr.bits(got), dr.bits(dense))


@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("win", ["aligned", "odd"])
def test_fused_on_windows_writes_only_its_window(dev, win, h, w):
    """the same for vc_offset_diversity, 16 groups.  aligned: k_deform<8, 4, MODE_OD, true, 4, 512>, bit-equal to the dense call;
    odd: k_deform<8, 4, MODE_OD, false, 1, 1024>"""
    from vcamd import hip
    kw = ALIGNED if win == "aligned" else ODD
    (x1, r1, f1, x2, r2, f2), wt, b, ref = _fused_case(8, 4, 16, h, w)
    pk = hip.PackedDeform(wt, b, 16, dev)
    out = dr.place(torch.full(ref.shape, dr.SENTINEL), dev, fill=dr.SENTINEL, **kw)
    pk.offset_diversity(*[dr.place(t, dev, seed=i, **kw) for i, t in enumerate((x1, r1, f1, x2, r2, f2))], MAG, out=out)
    got, outside = dr.read_window(out)
    dr.assert_untouched(outside)
    _hold("vc_offset_diversity", f"windows ({win}) {h}x{w}", got, ref, dr.CAP_FUSED)
    if win == "aligned":
        dense = hip.nhwc_to_nchw(pk.offset_diversity(*[dr.place(t, dev) for t in (x1, r1, f1, x2, r2, f2)], MAG)).cpu()
        assert torch.equal(dr.bits(got), dr.bits(dense))


# ---- exact sampling boundaries ----
@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("form", ["vec", "scalar"])
def test_generic_exact_sampling_boundaries(dev, form, h, w):
    """positions exactly at -1, -1 + 2^-10, -0.5, 0, 0.5, S - 1, S - 1 + 2^-10, S - 0.5, S in each axis and in both at the corners
    (exact in float32: the float64 reference takes the kernel's branch at every one), a NaN, a +inf and a -inf offset; pixels whose
    nine taps all lie outside the image hold the bias exactly (0 without one).  k_deform<8, 4, MODE_GENERIC, true, 1, 512> /
    <8, 4, MODE_GENERIC, false, 1, 1024>"""
    from vcamd import hip
    x, off, msk, wt, b, slots, dead = dr.boundary_inputs(8, 4, 8, h, w)
    tx, to, tm = dr.place(x, dev, **X_FORMS[form]), dr.place(off, dev), dr.place(msk, dev)
    for bias in (b, None):
        for mask in (msk, None):
            ref = dr.ref_generic(x, off, wt, bias, mask)
            assert torch.isfinite(ref).all()
            out = hip.nhwc_to_nchw(hip.PackedDeform(wt, bias, 8, dev).conv(tx, to, None if mask is None else tm)).cpu()
            _hold("vc_deform_conv2d", f"boundaries {h}x{w} {form} mask={mask is not None} bias={bias is not None}", out, ref, dr.CAP_GENERIC)
            want = torch.zeros(out.shape[1]) if bias is None else b
            for i, y, xx in dead:
                assert torch.equal(out[i, :, y, xx], want), (i, y, xx)


# ---- argument contract ----
def _copy(v, **fields):
    from vcamd import hip
    c = hip.View.from_buffer_copy(v)
    for k, val in fields.items():
        setattr(c, k, val)
    return c


def _sentinel_out(dev, n, c, h, w):
    return dr.place(torch.full((n, c, h, w), dr.SENTINEL), dev, fill=dr.SENTINEL)


def _all_sentinel(out):
    torch.cuda.synchronize()
    win, outside = dr.read_window(out)
    dr.assert_untouched(win.flatten())
    dr.assert_untouched(outside)


def test_generic_argument_contract(dev):
    """each bad call returns VC_EINVAL on the host, before any launch: the sentinel-filled output is untouched and a valid call
    right after it succeeds with the first valid call's bits"""
    from vcamd import hip
    L = hip.lib()
    n, h, w, groups = 2, 3, 5, 8
    x, off, msk, wt, b = dr.generic_inputs(8, 4, groups, h, w)
    pk = hip.PackedDeform(wt, b, groups, dev)
    tx, to, tm = dr.place(x, dev), dr.place(off, dev), dr.place(msk, dev)
    vx, vo, vm = tx.view(), to.view(), tm.view()

    def call(vx=vx, vo=vo, vm=vm, groups=groups, wpk=pk.wpk.data_ptr(), out=None, **out_fields):
        return L.vc_deform_conv2d(hip.stream(), vx, vo, vm, wpk, pk._bias_ptr(), groups, _copy(out.view(), **out_fields))

    first = _sentinel_out(dev, n, 32, h, w)
    assert call(out=first) == hip.VC_OK
    torch.cuda.synchronize()
    want = dr.read_window(first)[0]
    # 34 groups of 4 -> 2 channels: consistent channel counts, refused for the group count alone (one wave per group of a half)
    x34, o34 = dr.place(torch.zeros(n, 136, h, w), dev), dr.place(torch.zeros(n, 34 * 18, h, w), dev)
    w34 = torch.zeros(34 * 9 * 4 * 2, device=dev)
    bad = {
        "odd groups": dict(groups=7),
        "groups = 34": dict(vx=x34.view(), vo=o34.view(), vm=hip.NULL_VIEW, groups=34, wpk=w34.data_ptr(), c=68),
        "groups = 0": dict(groups=0),
        "(cg, og) = (8, 2) is not in the switch": dict(c=16),
        "(cg, og) = (2, 4)": dict(vx=_copy(vx, c=16)),
        "mask channels != 9 * groups": dict(vm=_copy(vm, c=71)),
        "offset channels != 18 * groups": dict(vo=_copy(vo, c=143)),
        "feature height": dict(vx=_copy(vx, h=h - 1)),
        "feature width": dict(vx=_copy(vx, w=w + 1)),
        "offset height": dict(vo=_copy(vo, h=h - 1)),
        "offset width": dict(vo=_copy(vo, w=w - 1)),
        "mask height": dict(vm=_copy(vm, h=h + 1)),
        "mask width": dict(vm=_copy(vm, w=w - 1)),
        "feature batch": dict(vx=_copy(vx, n=1)),
        "offset batch": dict(vo=_copy(vo, n=1)),
        "mask batch": dict(vm=_copy(vm, n=3)),
        "null features": dict(vx=_copy(vx, p=None)),
        "null weights": dict(wpk=None),
    }
    for what, kw in bad.items():
        out = _sentinel_out(dev, n, 68, h, w)
        out_fields = {"c": kw.pop("c", 32)}
        assert call(out=out, **kw, **out_fields) == -1, what
        _all_sentinel(out)
        assert call(out=out, c=32) == hip.VC_OK, f"valid call after: {what}"
        torch.cuda.synchronize()
        assert torch.equal(dr.bits(out.to_nchw()[:, :32].cpu()), dr.bits(want)), what
    # half features have no generic entry: the binding refuses the tensor before it makes a view of it
    out = _sentinel_out(dev, n, 32, h, w)
    with pytest.raises(hip.VcError):
        pk.conv(dr.place(x, dev, half=True), to, tm, out=out)
    _all_sentinel(out)


def test_fused_argument_contract(dev):
    """the same for vc_offset_diversity, _hx and _hxp -- with the shape that needs more LDS than the device has (32 groups of
    16 -> 8 channels: 184 KB), refused on the host instead of failing in hipFuncSetAttribute and leaving its error behind"""
    from vcamd import hip
    L = hip.lib()
    n, h, w, groups, cg = 2, 3, 5, 8, 8
    x1, r1, f1, x2, r2, f2, wt, b = dr.fused_inputs(cg, 4, groups, h, w)
    pk = hip.PackedDeform(wt, b, groups, dev)
    ts = [dr.place(t, dev) for t in (x1, r1, f1, x2, r2, f2)]
    v = [t.view() for t in ts]
    th = [dr.place(x1, dev, half=True), dr.place(x2, dev, half=True)]
    th_off = [dr.place(x1, dev, half=True, c0=2, cpad=8), dr.place(x2, dev, half=True, c0=2, cpad=8)]      # 4 bytes off: no vector gathers
    (p1, vp1), (p2, vp2) = _planar(x1, cg, dev), _planar(x2, cg, dev)
    r_off = [dr.place(r1, dev, c0=2, cpad=4), dr.place(r2, dev, c0=2, cpad=4)]                              # RV = 2: not for half features

    def call(fn=L.vc_offset_diversity, v=v, groups=groups, wpk=pk.wpk.data_ptr(), out=None, **out_fields):
        return fn(hip.stream(), v[0], v[1], v[2], v[3], v[4], v[5], MAG, wpk, pk._bias_ptr(), groups, _copy(out.view(), **out_fields))

    def sub(i, **fields):
        vv = list(v)
        vv[i] = _copy(v[i], **fields)
        return vv

    first = _sentinel_out(dev, n, 32, h, w)
    assert call(out=first) == hip.VC_OK
    torch.cuda.synchronize()
    want = dr.read_window(first)[0]
    hxv = [th[0].view(True), v[1], v[2], th[1].view(True), v[4], v[5]]
    hxpv = [vp1, v[1], v[2], vp2, v[4], v[5]]
    alive = []

    def z(c):
        alive.append(dr.place(torch.zeros(n, c, h, w), dev))
        return alive[-1].view()


    zeros34 = [z(17 * 4), z(27 * 17), v[2], z(17 * 4), z(27 * 17), v[5]]
    zeros32 = [z(16 * 16), z(27 * 16), v[2], z(16 * 16), z(27 * 16), v[5]]
    wbig = torch.zeros(32 * 9 * 16 * 8, device=dev)
    bad = {
        "odd groups": dict(groups=7),
        "groups = 34": dict(v=zeros34, groups=34, wpk=wbig.data_ptr(), c=68),
        "32 groups of 16 -> 8 channels: 184 KB of LDS": dict(v=zeros32, groups=32, wpk=wbig.data_ptr(), c=256),
        "(cg, og) = (8, 2)": dict(c=16),
        "raw1 channels != 27 * groups / 2": dict(v=sub(1, c=107)),
        "raw2 channels != 27 * groups / 2": dict(v=sub(4, c=109)),
        "x1 and x2 of different widths": dict(v=sub(3, c=16)),
        "feature height": dict(v=sub(0, h=h - 1)),
        "raw width": dict(v=sub(4, w=w + 1)),
        "flow height": dict(v=sub(2, h=h + 1)),
        "flow with one channel": dict(v=sub(5, c=1)),
        "feature batch": dict(v=sub(3, n=1)),
        "raw batch": dict(v=sub(1, n=3)),
        "flow batch": dict(v=sub(5, n=1)),
        "null flow": dict(v=sub(2, p=None)),
        "hx: features 4 bytes off": dict(fn=L.vc_offset_diversity_hx, v=[th_off[0].view(True), v[1], v[2], th_off[1].view(True), v[4], v[5]]),
        "hx: raw tensors that allow only RV = 2": dict(fn=L.vc_offset_diversity_hx, v=[hxv[0], r_off[0].view(), v[2], hxv[3], r_off[1].view(), v[5]]),
        "hxp: pixel stride != cg": dict(fn=L.vc_offset_diversity_hxp, v=[_copy(vp1, sw=cg + 4)] + hxpv[1:]),
        "hxp: row stride != w * cg": dict(fn=L.vc_offset_diversity_hxp, v=hxpv[:3] + [_copy(vp2, sh=(w + 1) * cg)] + hxpv[4:]),
        "hxp: image stride != (G/2) * h * w * cg": dict(fn=L.vc_offset_diversity_hxp, v=[_copy(vp1, sn=h * w * cg)] + hxpv[1:]),
        "hxp: planes of different widths": dict(fn=L.vc_offset_diversity_hxp, v=hxpv[:3] + [_copy(vp2, c=4, sw=4, sh=4 * w, sn=16 * h * w)] + hxpv[4:]),
    }
    for what, kw in bad.items():
        out = _sentinel_out(dev, n, 256, h, w)
        out_fields = {"c": kw.pop("c", 32)}
        assert call(out=out, **kw, **out_fields) == -1, what
        _all_sentinel(out)
        assert call(out=out, c=32) == hip.VC_OK, f"valid call after: {what}"
        torch.cuda.synchronize()
        assert torch.equal(dr.bits(out.to_nchw()[:, :32].cpu()), dr.bits(want)), what
    # and the half-feature views used above are good ones: both entries accept them
    for fn, vv in ((L.vc_offset_diversity_hx, hxv), (L.vc_offset_diversity_hxp, hxpv)):
        out = _sentinel_out(dev, n, 32, h, w)
        assert call(fn=fn, v=vv, out=out) == hip.VC_OK
        torch.cuda.synchronize()
    assert ctypes.sizeof(hip.View) == 48
