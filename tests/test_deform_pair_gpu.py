"""-m gpu: vc_deform_pair (csrc/deform.hip: k_deform<CG, OG, MODE_PAIR, VEC, RV, MAXT>), the two plain modulated deformable layers
of ICIP2023's DeformB.get_deformed_maps in one launch, against the float64 oracle (oracle.deform.deform_conv2d through
tests/deform_ref.py) fed cat(x-block, y-block) and sigmoid(mask-block) computed in float64.

Bound: |out - ref| / (1 + |ref|) < 5e-5, the one tests/test_deform_gpu.py holds the fused forms to (deform_ref.CAP_FUSED).
Everything else -- sentinels, bit equalities, bias-only pixels, return codes -- is exact."""
import functools

import pytest
import torch

import deform_ref as dr

pytestmark = pytest.mark.gpu
MAXIMA = {}
PAIRS = [(4, 4), (8, 8), (12, 12)]        # c = 32, 64, 96 of the model: 8 groups per reference
X_FORMS = {"vec": {}, "scalar": dict(c0=1, cpad=4), "stride": dict(c0=0, cpad=1)}
RAW_FORMS = {"dense": {}, "rv4": dict(c0=0, cpad=4), "rv2": dict(c0=2, cpad=4), "rv1": dict(c0=1, cpad=4)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda:0")
    for k in sorted(MAXIMA):
        print(f"\nlargest error seen, {k}: {MAXIMA[k]:.2e}", end="")


def _hold(what, out, ref):
    d = dr.rel_err(out, ref)
    MAXIMA["vc_deform_pair"] = max(MAXIMA.get("vc_deform_pair", 0.0), d)
    print(f"vc_deform_pair {what}: {d:.2e}")
    assert d < dr.CAP_FUSED, f"vc_deform_pair {what}: {d:.3e} >= {dr.CAP_FUSED}"


def prep(raw):
    """DeformB.get_deformed_maps (m.py:75-82) of one reference in the dtype of its input: offsets as they come, logistic on the mask"""
    ox, oy, m = torch.chunk(raw, 3, dim=1)
    return torch.cat((ox, oy), dim=1), torch.sigmoid(m)


def ref_pair(x1, raw1, x2, raw2, wt, bias=None):
    o1, m1 = prep(raw1.double())
    o2, m2 = prep(raw2.double())
    return dr.ref_generic(torch.cat((x1, x2), 1), torch.cat((o1, o2), 1), wt, bias, torch.cat((m1, m2), 1))


def pair_inputs(cg, og, groups, h, w, n=2, seed=0):
    """x1, raw1, x2, raw2, weight, bias: offsets ~ N(0, 1.5 px), so a good part of the samples leaves these small images; the two
    images of the batch and the two halves of the weights are different draws"""
    g = torch.Generator().manual_seed(3000 * cg + 100 * og + groups + 7 * h + seed)
    half = groups // 2
    x1, x2 = torch.randn(n, cg * half, h, w, generator=g), torch.randn(n, cg * half, h, w, generator=g)
    r1, r2 = torch.randn(n, 27 * half, h, w, generator=g) * 1.5, torch.randn(n, 27 * half, h, w, generator=g) * 1.5
    wt = torch.randn(og * groups, cg, 3, 3, generator=g) * 0.2
    b = torch.randn(og * groups, generator=g)
    return x1, r1, x2, r2, wt, b


@functools.lru_cache(maxsize=None)
def _case(cg, og, groups, h, w):
    x1, r1, x2, r2, wt, b = pair_inputs(cg, og, groups, h, w)
    ref = ref_pair(x1, r1, x2, r2, wt, b)
    assert torch.isfinite(ref).all()
    return (x1, r1, x2, r2), wt, b, ref


def _run(dev, cg, og, groups, h, w, form, raw="dense", with_bias=True):
    from vcamd import hip
    (x1, r1, x2, r2), wt, b, ref = _case(cg, og, groups, h, w)
    pk = hip.PackedDeform(wt, b if with_bias else None, groups, dev)
    out = pk.pair(dr.place(x1, dev, **X_FORMS[form]), dr.place(r1, dev, **RAW_FORMS[raw]), dr.place(x2, dev, seed=1, **X_FORMS[form]),
                  dr.place(r2, dev, seed=1, **RAW_FORMS[raw]))
    _hold(f"cg={cg} og={og} G={groups} {h}x{w} {form} raw={raw} bias={with_bias}", hip.nhwc_to_nchw(out).cpu(),
          ref if with_bias else ref - b.double().view(1, -1, 1, 1))


@pytest.mark.parametrize("h,w", dr.SIZES + dr.TINY)
@pytest.mark.parametrize("form", ["vec", "scalar"])
@pytest.mark.parametrize("cg,og", PAIRS)
def test_model_channel_pairs(dev, cg, og, form, h, w):
    """16 groups (records of 216 floats, dense raw tensors -> RV = 4), n = 2, with and without bias.
    vec: k_deform<cg, og, MODE_PAIR, true, 4, 512>;  scalar: k_deform<cg, og, MODE_PAIR, false, 4, 1024>.  (12, 12) holds
    8 x 9 x 144 weights + 64 records = 97 KB of dynamic LDS: through hipFuncSetAttribute."""
    _run(dev, cg, og, 16, h, w, form, with_bias=True)
    _run(dev, cg, og, 16, h, w, form, with_bias=False)


@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("form", ["vec", "scalar"])
@pytest.mark.parametrize("groups", [2, 4, 6])
def test_record_width_by_length(dev, groups, form, h, w):
    """(4, 4) with dense, aligned raw tensors whose record length alone limits the pieces: 2 groups (27 floats: RV = 1, ONE wave per
    workgroup), 4 groups (54: RV = 2), 6 groups (81: RV = 1, three waves)."""
    _run(dev, 4, 4, groups, h, w, form)


@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("form", ["vec", "scalar"])
@pytest.mark.parametrize("raw", ["rv4", "rv2", "rv1"])
def test_record_width_by_alignment(dev, raw, form, h, w):
    """16 groups of (8, 8); the raw tensors are channel windows at 16-, 8- and 4-byte alignment: RV = 4 / 2 / 1"""
    _run(dev, 8, 8, 16, h, w, form, raw)


@pytest.mark.parametrize("cg,og", PAIRS)
def test_odd_windows_take_the_scalar_path_and_agree(dev, cg, og):
    """x1 / x2 as odd-offset channel windows and at an odd pixel stride: VEC = false; the same bound, and the two scalar forms are
    the same arithmetic on the same values: equal bit for bit"""
    from vcamd import hip
    h, w = dr.SIZES[0]
    (x1, r1, x2, r2), wt, b, ref = _case(cg, og, 16, h, w)
    pk = hip.PackedDeform(wt, b, 16, dev)
    got = {}
    for form in ("scalar", "stride", "vec"):
        got[form] = hip.nhwc_to_nchw(pk.pair(dr.place(x1, dev, **X_FORMS[form]), dr.place(r1, dev), dr.place(x2, dev, seed=1, **X_FORMS[form]),
                                             dr.place(r2, dev))).cpu()
        _hold(f"cg={cg} og={og} {form}", got[form], ref)
    assert torch.equal(dr.bits(got["scalar"]), dr.bits(got["stride"]))
    assert dr.rel_err(got["scalar"], got["vec"]) < dr.CAP_FUSED


ALIGNED = dict(c0=4, cpad=8, hpad=3, wpad=4, n0=1, npad=2)      # starts and strides whole float4s: the vector form
ODD = dict(c0=3, cpad=5, hpad=2, wpad=3, n0=1, npad=2)          # the scalar form


@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("win", ["aligned", "odd"])
@pytest.mark.parametrize("cg,og", [(8, 8), (12, 12)])
def test_on_windows_writes_only_its_window(dev, cg, og, win, h, w):
    """every tensor a channel slice of a wider buffer, a crop of a larger one and images [1, 3) of four; outside its window the
    output buffer keeps the sentinel bit for bit.  aligned: bit-equal to the dense call (the same instance)."""
    from vcamd import hip
    kw = ALIGNED if win == "aligned" else ODD
    (x1, r1, x2, r2), wt, b, ref = _case(cg, og, 16, h, w)
    pk = hip.PackedDeform(wt, b, 16, dev)
    out = dr.place(torch.full(ref.shape, dr.SENTINEL), dev, fill=dr.SENTINEL, **kw)
    pk.pair(*[dr.place(t, dev, seed=i, **kw) for i, t in enumerate((x1, r1, x2, r2))], out=out)
    got, outside = dr.read_window(out)
    dr.assert_untouched(outside)
    _hold(f"cg={cg} og={og} windows ({win}) {h}x{w}", got, ref)
    if win == "aligned":
        dense = hip.nhwc_to_nchw(pk.pair(*[dr.place(t, dev) for t in (x1, r1, x2, r2)])).cpu()
        assert torch.equal(dr.bits(got), dr.bits(dense))


def boundary_inputs(cg, og, groups, h, w, n=2):
    """pair_inputs whose offsets are overwritten at chosen slots so that the sampling position is EXACTLY an integer position, -1,
    h / w, or far outside (multiples of 2^-10: exact in float32 and float64, both take the same branch); ``dead`` pixels have all
    nine taps of every group of BOTH references outside the image (output == bias exactly).  A NaN and an inf offset on top."""
    x1, r1, x2, r2, wt, b = pair_inputs(cg, og, groups, h, w, n, seed=5)
    half = groups // 2
    offs = [r[:, :18 * half].view(n, half, 9, 2, h, w) for r in (r1, r2)]          # (views: writes land in r1 / r2)
    ys, xs = dr.boundary_values(h) + [0.0, 1.0, -7.0, h + 40.0], dr.boundary_values(w) + [2.0, 0.0, w + 9.0, -100.0]
    dead = [(0, 0, 0), (1, h - 1, w - 1), (0, h // 2, w // 2)]
    j = 0
    for rep in range(3):
        for py in ys:
            for px in xs[rep::3]:
                r, i, g, k = j % 2, (j // 2) % n, (3 * j + rep) % half, (2 * j + rep) % 9
                y, xx = (5 * j + rep) % h, (11 * j + 3 * rep) % w
                if (i, y, xx) in dead:
                    xx = (xx + 1) % w
                if (i, y, xx) not in dead:
                    offs[r][i, g, k, 0, y, xx] = py - (y - 1 + k // 3)
                    offs[r][i, g, k, 1, y, xx] = px - (xx - 1 + k % 3)
                j += 1
    outside = [(-1.0, 0.5), (float(h), 1.0), (0.5, -1.0), (1.0, float(w)), (-1.0, -1.0), (float(h), float(w)), (-3.0, 0.0), (0.0, w + 2.5)]
    for i, y, xx in dead:
        for o in offs:
            for g in range(half):
                for k in range(9):
                    py, px = outside[(g + k) % len(outside)]
                    o[i, g, k, 0, y, xx] = py - (y - 1 + k // 3)
                    o[i, g, k, 1, y, xx] = px - (xx - 1 + k % 3)
    if h * w > 4:
        offs[0][0, 0, 4, 0, h - 1, 1] = float("nan")
        offs[1][n - 1, half - 1, 0, 1, 0, w - 2] = float("inf")
    return x1, r1, x2, r2, wt, b, dead


@pytest.mark.parametrize("h,w", dr.SIZES)
@pytest.mark.parametrize("form", ["vec", "scalar"])
@pytest.mark.parametrize("cg,og", [(4, 4), (12, 12)])
def test_exact_sampling_boundaries(dev, cg, og, form, h, w):
    """torchvision semantics: contributions from outside the image are zero, a sample exactly at -1 or at h / w is outside, one on an
    integer position reads that pixel alone; a pixel with every tap outside holds the bias exactly (0 without one)"""
    from vcamd import hip
    x1, r1, x2, r2, wt, b, dead = boundary_inputs(cg, og, 16, h, w)
    far = lambda r: torch.cat([torch.where(torch.isfinite(r[:, :144]), r[:, :144], torch.full_like(r[:, :144], dr.FAR)), r[:, 144:]], 1)  # noqa: E731
    ts = [dr.place(x1, dev, **X_FORMS[form]), dr.place(r1, dev), dr.place(x2, dev, seed=1, **X_FORMS[form]), dr.place(r2, dev)]
    for bias in (b, None):
        ref = ref_pair(x1, far(r1), x2, far(r2), wt, bias)
        assert torch.isfinite(ref).all()
        out = hip.nhwc_to_nchw(hip.PackedDeform(wt, bias, 16, dev).pair(*ts)).cpu()
        _hold(f"boundaries cg={cg} {h}x{w} {form} bias={bias is not None}", out, ref)
        want = torch.zeros(out.shape[1]) if bias is None else b
        for i, y, xx in dead:
            assert torch.equal(out[i, :, y, xx], want), (i, y, xx)


@pytest.mark.parametrize("cg,og", PAIRS)
def test_each_half_uses_its_own_layer(dev, cg, og):
    """PackedDeform.from_pair of two different layers: groups 0..7 carry the first layer's weights and read x1, groups 8..15 the
    second's and read x2.  Swapping the layers changes the output, and each order matches its own reference."""
    from vcamd import hip, icip2024
    h, w = dr.SIZES[0]
    (x1, r1, x2, r2), wt, b, ref = _case(cg, og, 16, h, w)
    c = 8 * cg
    la, lb = icip2024.DeformConv2d(c, c, groups=8), icip2024.DeformConv2d(c, c, groups=8)
    with torch.no_grad():
        la.weight.copy_(wt[:c]), la.bias.copy_(b[:c]), lb.weight.copy_(wt[c:]), lb.bias.copy_(b[c:])
    ts = [dr.place(t, dev) for t in (x1, r1, x2, r2)]
    ab = hip.nhwc_to_nchw(hip.PackedDeform.from_pair(la.to(dev), lb.to(dev)).pair(*ts)).cpu()
    ba = hip.nhwc_to_nchw(hip.PackedDeform.from_pair(lb.to(dev), la.to(dev)).pair(*ts)).cpu()
    _hold(f"cg={cg} layers (a, b)", ab, ref)
    _hold(f"cg={cg} layers (b, a)", ba, ref_pair(x1, r1, x2, r2, torch.cat([wt[c:], wt[:c]]), torch.cat([b[c:], b[:c]])))
    assert dr.rel_err(ab, ba) > 1e-2
    # and each half is the plain modulated layer on its own input (the unfused chain: chunk / cat / sigmoid + vc_deform_conv2d)
    for r, (x, raw, layer) in enumerate(((x1, r1, la), (x2, r2, lb))):
        off, msk = prep(raw)
        single = hip.nhwc_to_nchw(layer.packed().conv(dr.place(x, dev), dr.place(off, dev), dr.place(msk, dev))).cpu()
        assert dr.rel_err(ab[:, r * c:(r + 1) * c], single) < dr.CAP_FUSED


def _copy(v, **fields):
    from vcamd import hip
    c = hip.View.from_buffer_copy(v)
    for k, val in fields.items():
        setattr(c, k, val)
    return c


def test_argument_contract(dev):
    """each bad call returns VC_EINVAL on the host, before any launch: the sentinel-filled output is untouched and a valid call
    right after it succeeds with the first valid call's bits"""
    from vcamd import hip
    L = hip.lib()
    n, h, w, groups = 2, 3, 5, 16
    x1, r1, x2, r2, wt, b = pair_inputs(8, 8, groups, h, w)
    pk = hip.PackedDeform(wt, b, groups, dev)
    ts = [dr.place(t, dev) for t in (x1, r1, x2, r2)]
    v = [t.view() for t in ts]

    def call(v=v, groups=groups, wpk=pk.wpk.data_ptr(), out=None, **out_fields):
        return L.vc_deform_pair(hip.stream(), v[0], v[1], v[2], v[3], wpk, pk._bias_ptr(), groups, _copy(out.view(), **out_fields))

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
    _hold("contract shape", want, ref_pair(x1, r1, x2, r2, wt, b))
    bad = {
        "null x1": dict(v=sub(0, p=None)), "null raw1": dict(v=sub(1, p=None)), "null x2": dict(v=sub(2, p=None)),
        "null raw2": dict(v=sub(3, p=None)), "null weights": dict(wpk=None), "null out": dict(p=None),
        "odd groups": dict(groups=15), "groups = 0": dict(groups=0), "groups = 1": dict(groups=1),
        "raw1 channels != 27 * groups / 2": dict(v=sub(1, c=215)), "raw2 channels != 27 * groups / 2": dict(v=sub(3, c=217)),
        "x1 and x2 of different widths": dict(v=sub(2, c=32)),
        "x channels not divisible by groups / 2": dict(v=[_copy(v[0], c=60), v[1], _copy(v[2], c=60), v[3]]),
        "out channels not divisible by groups": dict(c=120),
        "(cg, og) = (8, 2) is not in the switch": dict(c=32),
        "(cg, og) = (8, 10)": dict(c=160),
        "x1 height": dict(v=sub(0, h=h - 1)), "x2 width": dict(v=sub(2, w=w + 1)), "raw1 width": dict(v=sub(1, w=w - 1)),
        "raw2 height": dict(v=sub(3, h=h + 1)), "x1 batch": dict(v=sub(0, n=1)), "raw2 batch": dict(v=sub(3, n=3)),
        "x2 batch": dict(v=sub(2, n=1)), "raw1 batch": dict(v=sub(1, n=1)),
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
    # half-precision features have no entry here: the binding refuses the tensor before it makes a view of it
    with pytest.raises(hip.VcError):
        pk.pair(dr.place(x1, dev, half=True), ts[1], dr.place(x2, dev, half=True), ts[3])
