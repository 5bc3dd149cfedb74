"""-m gpu: the convolution engine behind vc_conv2d_nhwc -- every tile configuration and pipeline, every epilogue row and the view
forms -- against the float64 reference of the whole vc_conv_desc contract (tests/conv_ref.py; pinned on the CPU by
tests/test_conv_cpu.py).

One acceptance measure for every case:

    |out - ref| <= lip * 6e-7 * mag + 4 * 2**-23 * |ref|        (+ 2**-11 * |ref| where the output is stored as half)

mag = sum |a b| of the accumulator, lip a bound on |d out / d acc| (conv_ref.reference); 6e-7 is the fp32 accumulator error
tests/test_split_gpu.py asserts, the second term pays for expf, sqrtf, the divide and the final roundings.  Each test prints the
worst ratio of error to allowance; the module prints the worst per pipeline at the end.  The fp16 instances get operands that are
exact in half (an exact-product, fp32-accumulate kernel: the same bar) and, besides, may not exceed 1.5 x the worst ratio of the
native fp32 instance on the same operands -- where the form stores half, the fp32 instance's result rounded to half and judged with
the same allowance, so that both sides carry the one store rounding the form is allowed.

One case needs more than the allowance and has a bar of its own, twice what the fp32 torch operators on the CPU need on the same
case under the same formula (CPU_FP32 below): GDN / IGDN with a residual at 128 -> 128, 2 x 11 x 37 -- CPU 1.084 / 0.920, the MI355X
instances (general, PW, PWS: bit-identical) 1.710 / 1.235.

How a configuration is pinned.  PackedConv.__call__ retries a configuration the library refuses on the layer's general one, which
would hide both a refusal and which instance ran.  The tests therefore take the route and the descriptor from the binding
(PackedConv._route / _describe, what every model call uses), put ``cfg | CFG_EXACT | flags`` into it -- the word a ``tuned`` entry
holds -- and call vc_conv2d_nhwc themselves: a refusal surfaces as hip.VcError, never as another instance's result.  The split
pipeline is reached by handing the layer a split tensor, never by shape.  Every refusal is on an explicit list (REFUSALS, and the
unaligned view forms); anything else that raises fails the test."""
import ctypes
import functools

import pytest
import torch

import conv_ref as cr
import deform_ref as dr

pytestmark = pytest.mark.gpu
N128, N64, N32, N16, N4, N128B, PW, N32T16, DMA, PWS, SPLIT = range(11)
NAMES = ["N128", "N64", "N32", "N16", "N4", "N128B", "PW", "N32T16", "DMA", "PWS", "SPLIT"]
PIPELINE = {N128: "classic", N64: "classic", N32: "classic", N16: "classic", N4: "classic", N128B: "classic", N32T16: "classic",
            PW: "PW", PWS: "PWS", DMA: "DMA", SPLIT: "split"}
WORST = {}
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vcamd import hip
    keep = hip.fp32_mode()
    hip.set_fp32_mode("native")            # (an fp32 window must never drift to the split pipeline by its shape)
    yield torch.device("cuda:0")
    hip.set_fp32_mode(keep)
    for k in sorted(WORST):
        print(f"\nworst error / allowance, {k}: {WORST[k]:.3f}", end="")


def _note(pipe, what, ratio):
    WORST[pipe] = max(WORST.get(pipe, 0.0), ratio)
    print(f"{pipe} {what}: {ratio:.3f}")


# ---- layers, packings, launches ----
def L(cin, cout, k, stride=1, n=2, h=19, w=45, ps=False):
    return (cin, cout, k, stride, n, h, w, ps)


def _lid(layer):
    cin, cout, k, stride, n, h, w, ps = layer
    return f"k{k}s{stride}-{cin}to{cout}{'ps' if ps else ''}-{n}x{h}x{w}"


_PACKED = {}


def _packed(dev, layer, kind="plain", prec="fp32", half_exact=False):
    from vcamd import hip
    key = (layer, kind, prec, half_exact)
    if key not in _PACKED:
        cin, cout, k, stride, n, h, w, ps = layer
        ins = cr.inputs(cin, cout, k, stride, n, h, w, ps, kind, half_exact)
        hip.set_conv_precision(prec)
        try:
            _PACKED[key] = hip.PackedConv(ins["w"], ins["b"], stride=stride, pixelshuffle=ps, device=dev)
        finally:
            hip.set_conv_precision("fp32")
        assert (_PACKED[key].wpk16 is not None) == (prec == "fp16")
    return _PACKED[key]


@functools.lru_cache(maxsize=None)
def _case(layer, form, half_exact=False):
    """(inputs, float64 reference) of one layer under one named epilogue form: computed once, shared, never modified"""
    cin, cout, k, stride, n, h, w, ps = layer
    kind = cr.EPILOGUES[form].get("kind", "plain")
    ins = cr.inputs(cin, cout, k, stride, n, h, w, ps, kind, half_exact)
    ref = cr.reference_of(ins, form, stride, ps)
    assert torch.isfinite(ref.out).all() and bool((ref.mag >= (cr.shuffle2(ref.acc) if ps else ref.acc).abs()).all())
    return ins, ref


def _unsplit(t):
    """split tensor window -> NCHW fp32, the exact sum of its pieces: (lo + mid) + hi"""
    full = t.buf.view(-1)
    n, h, w, c = t.n, t.h, t.w, t.c
    per_img = t.sn * h * w * 24
    out = torch.empty(n, c, h, w)
    for i in range(n):
        start = i * per_img + t.off * h * w * 24
        rec = full[start:start + (c // 8) * h * w * 24].view(c // 8, h, w, 3, 8).to(torch.int32)
        pieces = (rec << 16).view(torch.float32)
        out[i] = ((pieces[..., 2, :] + pieces[..., 1, :]) + pieces[..., 0, :]).permute(0, 3, 1, 2).reshape(c, h, w).cpu()
    return out


# where the tensors of a call live.  "dense": each its own dense buffer.  Offsets 4 and 16: every window starts at that channel of a
# wider buffer, 16-byte aligned with strides that are whole float4s; 1 and 3: 4 and 12 bytes off (vec4 == 0, vec_out == 0) -- with
# offset 3 the strides themselves stay whole float4s: the views are misaligned, not narrow.  Input, output, residual and multiplier
# get buffers of different widths, heights, lengths and first images: strides of their own.
CPAD = {4: (8, 12, 4, 16), 16: (32, 20, 16, 24), 1: (5, 3, 2, 7), 3: (4, 8, 12, 5)}       # extra channels of x, out, res, mul
ROLE = [dict(hpad=2, wpad=3, n0=1, npad=2), dict(hpad=1, wpad=2, n0=0, npad=1), dict(hpad=3, wpad=1, n0=2, npad=3),
        dict(hpad=0, wpad=4, n0=1, npad=1)]


def _win(role, off):
    if off is None:
        return {}
    return dict(c0=off, cpad=CPAD[off][role], **ROLE[role])


def _run(dev, layer, cfg, form, off=None, prec="fp32", x_half=False, out_half=False, res_half=False, x_split=False, res_split=False,
         out_split=False, own_mul=False):
    """One launch of exactly ``cfg``.  -> worst error / allowance over the output window; raises hip.VcError where the binding or the
    library refuses.  The input window is surrounded by NaN, the output buffer pre-filled with a sentinel that must survive bit for
    bit outside the window."""
    from vcamd import hip
    f = cr.EPILOGUES[form]
    kind = f.get("kind", "plain")
    half_exact = prec == "fp16"
    ins, ref = _case(layer, form, half_exact)
    pc = _packed(dev, layer, kind, prec, half_exact)
    assert cfg == SPLIT or cfg == pc.cfg or cfg in pc.candidates, f"{NAMES[cfg]} does not read this layer's packing"
    # (vc_split3 reads 16-byte groups: the fp32 source of a split input is an aligned window also where the other views are not)
    xt = dr.place(ins["x"], dev, fill=NAN, half=x_half, **_win(0, 4 if (x_split and off in (1, 3)) else off))
    if x_split:                       # a window of planes and images of a wider split tensor whose other records are NaN
        n, h, w = xt.n, xt.h, xt.w
        wide = hip.T.empty(n + 2, h, w, pc.cin_split + 16, dev, "sp3")
        wide.buf.fill_(0x7fc0)
        xs = wide.images(1, 1 + n).channels(8, 8 + pc.cin_split)
        hip.split3(xt, out=xs, c_out=pc.cin_split)
        xt = xs
    res = mul = gain = None
    if f.get("res"):
        res = dr.place(ins["res"], dev, fill=NAN, half=res_half, seed=1, **_win(2, off))
        if res_split:
            res = hip.split3(res)
    if f.get("mul"):
        mul = dr.place(ins["mul"], dev, fill=NAN, seed=2, **_win(3, off)) if own_mul else xt
    if f.get("gain"):
        gain = ins["gain"].to(dev)
    shape = tuple(ref.out.shape)
    if out_split:
        out = hip.T.empty(shape[0], shape[2], shape[3], shape[1], dev, "sp3")
    else:
        out = dr.place(torch.full(shape, dr.SENTINEL), dev, fill=dr.SENTINEL, half=out_half, **_win(1, off))
    act = {"none": hip.ACT_NONE, "relu": hip.ACT_RELU, "lrelu": hip.ACT_LRELU, "sigmoid": hip.ACT_SIGMOID, "clamp01": hip.ACT_CLAMP01}[f.get("act", "none")]
    epi = {"none": hip.EPI_NONE, "gdn": hip.EPI_GDN, "igdn": hip.EPI_IGDN}[f.get("epi", "none")]
    xform = hip.IN_SQUARE if f.get("square") else hip.IN_NONE
    slope = f.get("slope", 0.01)
    r = pc._route(xt, out, act, slope, res, epi, mul, xform, gain, False, f.get("res_first", False), None, False)
    assert r.split == (cfg == SPLIT), "the route the binding takes is not the pipeline under test"
    d = pc._describe(r, xt, out, act, slope, res, epi, mul, xform, gain, None)
    d.cfg = r.cfg if r.split else (cfg | hip.CFG_EXACT | r.flags | pc._pack128)
    want = (hip.CFG_F16 if prec == "fp16" else 0) | (hip.CFG_IN_F16 if x_half else 0) | (hip.CFG_OUT_F16 if out_half else 0) | \
        (hip.CFG_RES_F16 if res_half else 0) | (hip.CFG_RES_FIRST if f.get("res_first") else 0)
    assert d.cfg & (hip.CFG_F16 | hip.CFG_IN_F16 | hip.CFG_OUT_F16 | hip.CFG_RES_F16 | hip.CFG_RES_FIRST) == want
    hip.check(hip.lib().vc_conv2d_nhwc(hip.stream(), ctypes.byref(d)), f"vc_conv2d_nhwc {NAMES[cfg]} {_lid(layer)} {form}")
    torch.cuda.synchronize()
    if out_split:
        got = _unsplit(out)
    else:
        got, outside = dr.read_window(out)
        if out_half:
            assert torch.equal(outside, torch.full_like(outside, dr.SENTINEL)), "elements outside the output window were written"
        else:
            dr.assert_untouched(outside)
    return cr.worst_ratio(got.float(), ref, out_half)


# Forms that legitimately need more than the allowance: the bar is then twice what the fp32 torch operators on the CPU need on the
# SAME case under the same formula (F.conv2d, x * (1 / sqrt(.)) or x * sqrt(.), + residual, all float32), never the kernel's own figure.
#   GDN / IGDN with a residual, 128 -> 128 at 2 x 11 x 37: CPU fp32 1.084 / 0.920 x the allowance; the MI355X instances (general,
#   PW and PWS: equal bit for bit) 1.710 / 1.235.  Why: a GDN accumulator sums non-negative terms, mag == acc, so lip * 6e-7 * mag is
#   3e-7 |v| of v = mul / sqrt(acc) -- all of it used up by an accumulator that is 6e-7 off -- and the roundings of sqrtf, the divide
#   and the product (1.5 ulp of |v|) are paid from 4 * 2**-23 * |ref| alone, which a residual of the opposite sign takes away.  The
#   same layers without a residual stay inside the allowance (0.59 on the CPU), as does the 64-channel case (CPU 1.071, GPU 0.986).
CPU_FP32 = {(L(128, 128, 1, h=11, w=37), "gdn+res"): 1.084, (L(128, 128, 1, h=11, w=37), "igdn+res"): 0.920}


def _hold(dev, layer, cfg, form, **kw):
    ratio = _run(dev, layer, cfg, form, **kw)
    tag = "fp16 " if kw.get("prec") == "fp16" else ""
    bar = max(1.0, 2.0 * CPU_FP32.get((layer, form), 0.0))
    _note(tag + PIPELINE[cfg] + (" (GDN + residual, 128 channels)" if bar > 1.0 else ""), f"{NAMES[cfg]} {_lid(layer)} {form} {kw if kw else ''}", ratio)
    assert ratio <= bar, f"{NAMES[cfg]} {_lid(layer)} {form} {kw}: error {ratio:.3f} x the allowance (bar {bar:.3f})"
    return ratio


# ---- dispatch forms, fp32 ----
# The smallest shapes with more than one tile in x and y, a ragged last tile in both, two images where the form loops over a batch:
# 8 x 32-pixel tiles (classic), 8 x 64 (N4), 16 x 32 (N32T16, the LDS-DMA pipeline), 12 / 16 / 24 x 32 (split).
CLASSIC = [
    (L(128, 128, 3), [N128, N64, N32, N128B, DMA]),
    (L(128, 12, 3, h=17, w=40), [N16]),                      # a last N-tile that is partly padding
    (L(128, 16, 3, h=17, w=40), [N16]),
    (L(128, 12, 3, n=1, h=17, w=33, ps=True), [N16]),        # shuffled to 3 channels per pixel: the scalar epilogue
    (L(128, 512, 3, n=1, h=17, w=35, ps=True), [N128, N64, N32, N128B, DMA]),
    (L(192, 768, 3, n=1, h=9, w=33, ps=True), [N128, N128B]),          # more than one block of 128
    (L(32, 4, 3, h=17, w=75), [N4]),
    (L(32, 2, 3, h=17, w=75), [N4]),
    (L(16, 2, 7, h=19, w=130), [N4]),
    (L(32, 1, 5, n=1, h=17, w=70), [N4]),
    (L(32, 64, 7, h=37), [N64, N32, N32T16, DMA]),
    (L(64, 32, 7, h=37), [N32, N32T16, DMA]),
    (L(8, 32, 7, h=21, w=40), [N32, N32T16]),                # SPyNet's first layer: the 8-channel chunk
    # stride 2; odd input sizes: the last output column and row read the padding
    (L(3, 128, 1, 2, h=17, w=33), [N128, N64, N32]),
    (L(128, 128, 1, 2, h=17, w=67), [N128, N64, N32]),
    (L(3, 128, 3, 2, h=33, w=67), [N128, N64, N32]),
    (L(128, 128, 3, 2, n=1, h=33, w=67), [N128, N64, N32]),
    (L(192, 192, 3, 2, n=1, h=33, w=67), [N64, N32]),
    (L(3, 128, 5, 2, h=33, w=67), [N128, N64, N32]),        # the I-frame codec's layers
    (L(128, 128, 5, 2, n=1, h=33, w=67), [N128, N64, N32]),
    (L(192, 192, 5, 2, n=1, h=17, w=67), [N64, N32]),
    # input channel counts that force the scalar staging path
    (L(6, 32, 5, h=17, w=40), [N32]),
    (L(6, 32, 3, h=17, w=40), [N32]),
    (L(19, 128, 3, 2, n=1, h=33, w=67), [N128, N64, N32]),
    # the other fp32 LDS-DMA instances
    (L(64, 64, 3), [N64, N32, DMA]),
    (L(32, 64, 3), [N64, N32, DMA]),
    (L(96, 32, 5), [N32, DMA]),
]
POINTWISE = [      # 1 x 1 stride 1: the general kernel, the streaming kernel and its LDS-DMA successor
    (L(32, 32, 1, n=3, h=16, w=50), [N32, PW, PWS]),
    (L(64, 64, 1, n=1, h=33, w=64), [N64, N32, PW, PWS]),
    (L(96, 64, 1, n=1, h=9, w=31), [N64, PW, PWS]),
    (L(96, 96, 1, h=20, w=50), [N128, PW, PWS]),
    (L(128, 96, 1, n=1, h=12, w=33), [N128, PW, PWS]),
    (L(128, 128, 1, h=17, w=45), [N128, N64, N32, PW, PWS]),
    (L(128, 32, 1, n=1, h=18, w=40), [N32, PW, PWS]),
    (L(64, 32, 1, n=1, h=8, w=129), [N32, PW, PWS]),
    (L(64, 64, 1, n=1, h=5, w=17), [N64, PW, PWS]),                    # a row shorter than one tile
    (L(128, 128, 1, n=1, h=300, w=250), [N128, PWS]),                  # more tiles than the 2048 persistent waves
]
DISPATCH = [(layer, cfg) for layer, cfgs in CLASSIC + POINTWISE for cfg in cfgs]


@pytest.mark.parametrize("layer,cfg", DISPATCH, ids=[f"{_lid(l)}-{NAMES[c]}" for l, c in DISPATCH])
def test_dispatch_forms_fp32(dev, layer, cfg):
    """every fp32 instance behind vc_conv2d_nhwc on dense views, under LeakyReLU + channel gain + residual (pixel-shuffle layers:
    ReLU + residual laid out like the shuffled output; no caller puts a gain on one, see tests/conv_ref.py) and under a plain
    LeakyReLU (0.01)"""
    ps = layer[7]
    _hold(dev, layer, cfg, "res" if ps else "gain+res")
    _hold(dev, layer, cfg, "lrelu.01")


def test_every_configuration_is_named_by_a_case_that_must_run():
    """static: every tile configuration and pipeline has at least one case in the tables of this module that no list excuses"""
    named = {c for _, c in DISPATCH} | {SPLIT}
    assert named == set(range(11))
    for pipe, (layer, gdn_layer, cfg) in EPI_PIPES.items():
        assert [f for f in FORMS_OF[pipe] if f not in REFUSALS.get(pipe, ())], pipe


# ---- split-operand pipeline ----
SPLIT_LAYERS = [
    L(128, 128, 3, h=29), L(64, 32, 3, h=29),     # 3x3 period instance (input channels a multiple of 32), blocks of 64 and 32
    L(48, 64, 3, h=29),                            # 3x3 per-chunk instance
    L(48, 64, 5, h=29), L(96, 32, 5, h=29),       # 5x5 period instance
    L(24, 32, 5, h=29),                            # 5x5 per-chunk (tap-padded) instance
    L(16, 32, 7, h=29), L(32, 128, 7, h=29),      # 7x7 period instance, one and two blocks of 64
    L(8, 32, 7, h=29),                             # 7x7 per-chunk instance
    L(32, 16, 7, h=29),                            # the 16-channel instance, 24-row tiles
    L(6, 32, 5, h=29), L(6, 32, 3, h=29),         # vc_split3_pad: 6 -> 8 / 16 channels, zero weights for the padding
]


@pytest.mark.parametrize("layer", SPLIT_LAYERS, ids=_lid)
def test_split_pipeline(dev, layer):
    """VC_CFG_SPLIT, reached by handing the layer a split tensor (a window of planes and images of a wider, NaN-filled one): fp32 and
    split residuals, fp32 and split output -- the split output read back as the exact sum of its pieces"""
    from vcamd import hip
    pc = _packed(dev, layer)
    assert pc.split_ok
    g = hip.split_geometry(layer[2], layer[1], layer[0])
    assert (layer[4] > 1) and (layer[5] + g.th - 1) // g.th > 1 and layer[5] % g.th and layer[6] > 32 and layer[6] % 32
    r = [_hold(dev, layer, SPLIT, "gain+res", x_split=True),
         _hold(dev, layer, SPLIT, "gain+res", x_split=True, res_split=True),
         _hold(dev, layer, SPLIT, "resfirst-relu", x_split=True, res_split=True, out_split=True),
         _hold(dev, layer, SPLIT, "lrelu.2", x_split=True, out_split=True)]
    assert len(r) == 4


# ---- epilogue forms ----
# pipeline -> (layer of the plain and wide forms, layer of the GDN forms or None, configuration)
EPI_PIPES = {
    "classic-vector": (L(64, 64, 3, h=11, w=37), L(64, 64, 1, h=11, w=37), N64),
    "classic-scalar": (L(64, 6, 3, h=11, w=37), L(6, 6, 1, h=11, w=37), N16),          # 6 channels per pixel: vec_out == 0
    "N4-vector": (L(32, 4, 3, h=11, w=70), None, N4),
    "N4-scalar": (L(32, 2, 3, h=11, w=70), None, N4),
    "PW": (L(64, 64, 1, h=11, w=37), L(128, 128, 1, h=11, w=37), PW),
    "PWS": (L(64, 64, 1, h=11, w=37), L(128, 128, 1, h=11, w=37), PWS),
    "DMA": (L(64, 64, 3, h=19, w=37), None, DMA),
    "split": (L(32, 64, 5, h=19, w=37), None, SPLIT),
}
ALL_FORMS = list(cr.EPILOGUES)
NO_GDN = [f for f in ALL_FORMS if cr.EPILOGUES[f].get("kind") != "gdn"]
FORMS_OF = {p: (ALL_FORMS if EPI_PIPES[p][1] is not None else NO_GDN) for p in EPI_PIPES}     # (no 1 x 1 layer: no GDN layer)
# what the library declines, by its own statement in include/vc_hip.h: the streaming 1 x 1 kernels and the split pipeline have
# plain / ReLU / LeakyReLU epilogues and -- GDN on the streaming kernels apart -- no input transform; the LDS-DMA pipeline copies
# its input as it lies (no transform)
_NO_SIGMOID = {"sigmoid", "clamp01", "sigmoid+gain+res", "square"}
REFUSALS = {"PW": _NO_SIGMOID, "PWS": _NO_SIGMOID, "split": _NO_SIGMOID, "DMA": {"square"}}
EPI_CASES = [(p, f) for p in EPI_PIPES for f in FORMS_OF[p]]


@pytest.mark.parametrize("pipe,form", EPI_CASES, ids=[f"{p}-{f}" for p, f in EPI_CASES])
def test_epilogue_forms(dev, pipe, form):
    """every row of the vc_conv_desc contract on a vector-epilogue and a scalar-epilogue instance of every pipeline that has one"""
    from vcamd import hip
    layer, gdn_layer, cfg = EPI_PIPES[pipe]
    f = cr.EPILOGUES[form]
    if f.get("kind") == "gdn":
        layer = gdn_layer
    kw = dict(x_split=True) if cfg == SPLIT else {}
    if form in REFUSALS.get(pipe, ()):
        with pytest.raises(hip.VcError):
            _run(dev, layer, cfg, form, **kw)
        return
    _, ref = _case(layer, form)
    if f.get("act") == "sigmoid" and not f.get("res"):
        assert float(ref.out.min()) < 0.01 and float(ref.out.max()) > 0.99, "the sigmoid case does not reach both saturations"
    if f.get("act") == "clamp01":
        assert bool((ref.out == 0).any()) and bool((ref.out == 1).any()) and bool(((ref.out > 0) & (ref.out < 1)).any())
        assert bool((ref.acc.abs() < 0.05).any()) and bool(((ref.acc - 1).abs() < 0.05).any()), "no accumulator near a clamp corner"
    _hold(dev, layer, cfg, form, **kw)
    if f.get("mul") and pipe.startswith("classic"):
        _hold(dev, layer, cfg, form, own_mul=True)        # a multiplier that is not the input window


# ---- view forms ----
VIEW_PIPES = {"classic": (L(64, 64, 3, h=11, w=37), N64), "classic-N128": (L(128, 128, 3, h=11, w=37), N128), "PW": (L(64, 64, 1, h=11, w=37), PW),
              "PWS": (L(64, 64, 1, h=11, w=37), PWS), "DMA": (L(64, 64, 3, h=19, w=37), DMA), "split": (L(32, 64, 5, h=19, w=37), SPLIT)}


@pytest.mark.parametrize("off", [4, 16, 1, 3])
@pytest.mark.parametrize("pipe", list(VIEW_PIPES))
def test_view_forms(dev, pipe, off):
    """input = channel slice, spatial crop and image range of a wider NaN-filled buffer; output, residual (and GDN multiplier) slices of
    differently shaped buffers with strides of their own; the sentinel around the output window survives bit for bit.  Offsets 4 and
    16 (16-byte aligned): every pipeline serves them.  Offsets 1 and 3 (vec4 == 0, vec_out == 0): the classic configurations serve
    them on their scalar staging path and scalar epilogue, the streaming, LDS-DMA and split pipelines decline with VcError."""
    from vcamd import hip
    layer, cfg = VIEW_PIPES[pipe]
    kw = dict(x_split=True) if cfg == SPLIT else {}
    if off in (1, 3) and not pipe.startswith("classic"):
        with pytest.raises(hip.VcError):
            _run(dev, layer, cfg, "gain+res", off=off, **kw)
        return
    _hold(dev, layer, cfg, "gain+res", off=off, **kw)
    if pipe == "classic":
        for form in ("gdn+res", "igdn+res"):
            _hold(dev, L(64, 64, 1, h=11, w=37), N64, form, off=off, own_mul=True)
        _hold(dev, layer, cfg, "sigmoid+gain+res", off=off)


def test_binding_serves_an_unaligned_view_on_the_general_configuration(dev):
    """PackedConv.__call__ with a ``tuned`` entry that pins the streaming kernel: on an unaligned window the library declines it and the
    binding's retry on the general configuration gives that configuration's bits"""
    from vcamd import hip
    layer = L(64, 64, 1, h=11, w=37)
    ins, ref = _case(layer, "gain+res")
    pc = _packed(dev, layer)
    outs = []
    for cfg in (PWS, pc.cfg):
        x = dr.place(ins["x"], dev, fill=NAN, **_win(0, 3))
        res = dr.place(ins["res"], dev, fill=NAN, **_win(2, 3))
        out = dr.place(torch.full(tuple(ref.out.shape), dr.SENTINEL), dev, fill=dr.SENTINEL, **_win(1, 3))
        pc.tuned = {(x.n, x.h, x.w, 0): cfg | hip.CFG_EXACT}
        pc(x, out=out, act=hip.ACT_LRELU, slope=0.2, res=res, chscale=ins["gain"].to(dev))
        torch.cuda.synchronize()
        got, outside = dr.read_window(out)
        dr.assert_untouched(outside)
        outs.append(got)
    pc.tuned = {}
    assert torch.equal(dr.bits(outs[0]), dr.bits(outs[1]))
    assert cr.worst_ratio(outs[0], ref) <= 1.0


# ---- fp16 path ----
F16_LAYERS = [       # layer, configurations
    (L(128, 128, 3), [N128, N64, N32, N128B, DMA]),
    (L(64, 64, 3), [N64, N32, DMA]),
    (L(96, 384, 3, n=1), [N128, N128B, DMA]),
    (L(128, 432, 3, n=1), [N128, N128B, DMA]),               # a partly padded last block of 128 (CFG_PACK128)
    (L(128, 512, 3, n=1, h=17, w=35, ps=True), [N128B, DMA]),
    (L(64, 32, 7, h=37), [N32, N32T16, DMA]),
    (L(32, 64, 7, h=37), [N64, N32, N32T16, DMA]),
    (L(32, 16, 7, h=17, w=40), [N16]),
    (L(192, 64, 5, n=1), [N64, N32]),
    (L(128, 128, 3, 2, n=1, h=33, w=67), [N128, N64, N32]),
    (L(32, 32, 1, n=3, h=16, w=50), [N32, PW, PWS]),
    (L(64, 64, 1, n=1, h=33, w=64), [N64, PW, PWS]),
    (L(96, 96, 1, h=20, w=50), [N128, PW, PWS]),
    (L(128, 128, 1, h=17, w=45), [N128, N32, PW, PWS]),
    (L(128, 64, 1, n=1, h=5, w=17), [N64, PW, PWS]),
]
F16_CASES = [(layer, cfg) for layer, cfgs in F16_LAYERS for cfg in cfgs]
_NATIVE = {}


def _native32(dev, layer, form):
    """the native fp32 instance (the layer's general configuration) on the SAME half-exact operands: its output, kept on the CPU"""
    from vcamd import hip
    key = (layer, form)
    if key not in _NATIVE:
        f = cr.EPILOGUES[form]
        ins, ref = _case(layer, form, True)
        pc = _packed(dev, layer, f.get("kind", "plain"), "fp32", True)
        x = dr.place(ins["x"], dev)
        res = dr.place(ins["res"], dev) if f.get("res") else None
        out = dr.place(torch.zeros(tuple(ref.out.shape)), dev)
        act = {"none": hip.ACT_NONE, "relu": hip.ACT_RELU, "lrelu": hip.ACT_LRELU, "sigmoid": hip.ACT_SIGMOID}[f.get("act", "none")]
        gain = ins["gain"].to(dev) if f.get("gain") else None
        slope = f.get("slope", 0.01)
        r = pc._route(x, out, act, slope, res, hip.EPI_NONE, None, hip.IN_NONE, gain, False, f.get("res_first", False), None, False)
        d = pc._describe(r, x, out, act, slope, res, hip.EPI_NONE, None, hip.IN_NONE, gain, None)
        d.cfg = pc.cfg | hip.CFG_EXACT | r.flags
        assert not r.split and not r.flags & hip.CFG_F16
        hip.check(hip.lib().vc_conv2d_nhwc(hip.stream(), ctypes.byref(d)), "the native fp32 instance")
        torch.cuda.synchronize()
        _NATIVE[key] = dr.read_window(out)[0]
    return _NATIVE[key]


def _hold16(dev, layer, cfg, form, **kw):
    ratio = _hold(dev, layer, cfg, form, prec="fp16", **kw)
    _, ref = _case(layer, form, True)
    out32 = _native32(dev, layer, form)
    half = bool(kw.get("out_half"))
    native = cr.worst_ratio(out32.half().float() if half else out32, ref, half)
    print(f"    native fp32 instance on the same operands{' (rounded to half)' if half else ''}: {native:.3f}")
    assert native <= 1.0
    assert ratio <= 1.5 * native, f"fp16 {NAMES[cfg]} {_lid(layer)} {form} {kw}: {ratio:.3f} against {native:.3f} of the native fp32 instance"


@pytest.mark.parametrize("layer,cfg", F16_CASES, ids=[f"{_lid(l)}-{NAMES[c]}" for l, c in F16_CASES])
def test_fp16_instances_on_half_exact_operands(dev, layer, cfg):
    """set_conv_precision("fp16") with x, w and the residual exact in half: the fp16 instances multiply what the reference multiplies
    and accumulate in fp32 -- the fp32 bar, and at most 1.5 x the native fp32 instance's worst ratio.  Every combination of
    CFG_IN_F16 and CFG_OUT_F16 (the LDS-DMA pipeline reads half only)."""
    ps = layer[7]
    form = "res" if ps else "gain+res"
    for x_half in ((True,) if cfg == DMA else (False, True)):
        for out_half in (False, True):
            _hold16(dev, layer, cfg, form, x_half=x_half, out_half=out_half)
    _hold16(dev, layer, cfg, "lrelu.01", x_half=cfg == DMA)


F16_EPI = [(L(128, 128, 3, h=19, w=37), N128B), (L(128, 128, 3, h=19, w=37), DMA), (L(64, 64, 1, h=11, w=37), PW), (L(64, 64, 1, h=11, w=37), PWS)]
F16_FORMS = ["none", "relu", "lrelu.2", "sigmoid", "gain", "res", "gain+res", "resfirst-none", "resfirst-relu", "resfirst-lrelu"]
F16_EPI_CASES = [(l, c, f) for l, c in F16_EPI for f in F16_FORMS]


@pytest.mark.parametrize("layer,cfg,form", F16_EPI_CASES, ids=[f"{NAMES[c]}-{f}" for l, c, f in F16_EPI_CASES])
def test_fp16_epilogue_forms(dev, layer, cfg, form):
    """the epilogue rows on the fp16 instances of each pipeline (half input, fp32 and half output); the streaming kernels decline the
    sigmoid as on the fp32 path"""
    from vcamd import hip
    if form == "sigmoid" and cfg in (PW, PWS):
        with pytest.raises(hip.VcError):
            _run(dev, layer, cfg, form, prec="fp16", x_half=True)
        return
    for out_half in (False, True):
        _hold16(dev, layer, cfg, form, x_half=True, out_half=out_half)


@pytest.mark.parametrize("layer,cfg", [(L(128, 128, 1, h=17, w=45), PWS), (L(64, 64, 1, n=1, h=33, w=64), PWS), (L(32, 32, 1, n=3, h=16, w=50), PWS),
                                       (L(128, 128, 3), DMA), (L(64, 64, 3), DMA)], ids=lambda v: _lid(v) if isinstance(v, tuple) else NAMES[v])
def test_fp16_half_precision_residual(dev, layer, cfg):
    """CFG_RES_F16 (the streaming 1 x 1 kernel and the LDS-DMA 3 x 3 kernel): the residual, exact in half, read as half -- residual
    after and (streaming kernel) before the activation, fp32 and half output, fp32 and half input"""
    from vcamd import hip
    for form in ("gain+res", "res") + (("resfirst-relu",) if cfg == PWS else ()):
        for x_half in ((True,) if cfg == DMA else (False, True)):
            for out_half in (False, True):
                _hold16(dev, layer, cfg, form, x_half=x_half, out_half=out_half, res_half=True)
    if cfg == DMA:            # stated in include/vc_hip.h: no half residual in front of the activation on this pipeline
        with pytest.raises(hip.VcError):
            _run(dev, layer, cfg, "resfirst-relu", prec="fp16", x_half=True, res_half=True)


def test_fp16_classic_instances_decline_a_half_precision_residual(dev):
    from vcamd import hip
    layer = L(128, 128, 1, h=17, w=45)
    for cfg in (N128, PW):
        with pytest.raises(hip.VcError):
            _run(dev, layer, cfg, "res", prec="fp16", x_half=True, res_half=True)
