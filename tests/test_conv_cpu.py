"""tests/conv_ref.py (the float64 reference tests/test_conv_gpu.py holds the convolution engine against) is itself checked here, with
no GPU: every epilogue row against the torch operator chain evaluated in float64 (F.conv2d, F.leaky_relu, torch.sigmoid,
F.pixel_shuffle, oracle.cai.layers.GDN) to 1e-12 relative, mag >= |acc|, lip by finite differences of the reference, and the
properties of the generated inputs the GPU module relies on."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as cr

RTOL = 1e-12


def _same(a, b, what):
    d = float(((a - b).abs() / (1.0 + b.abs())).max())
    assert a.shape == b.shape and d <= RTOL, f"{what}: {d:.2e}"


def _chain(ins, form, stride, shuffle):
    """the same form as torch operators in float64, written independently of conv_ref.reference"""
    f = cr.EPILOGUES[form]
    x, w, b = ins["x"].double(), ins["w"].double(), ins["b"].double()
    res = ins["res"].double() if f.get("res") else None
    v = F.conv2d(x * x if f.get("square") else x, w, b, stride=stride, padding=w.shape[-1] // 2)
    if f.get("res_first"):
        v = v + res
    act = f.get("act", "none")
    v = {"none": lambda t: t, "relu": F.relu, "lrelu": lambda t: F.leaky_relu(t, f.get("slope", 0.01)), "sigmoid": torch.sigmoid,
         "clamp01": lambda t: t.clamp(0, 1)}[act](v)
    if f.get("gain"):
        v = v * ins["gain"].double().view(1, -1, 1, 1)
    if shuffle:
        v = F.pixel_shuffle(v, 2)
    if res is not None and not f.get("res_first"):
        v = v + res
    return v


PLAIN_FORMS = [k for k, f in cr.EPILOGUES.items() if f.get("kind") != "gdn"]


@pytest.mark.parametrize("k", [1, 3, 5, 7])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("form", PLAIN_FORMS)
def test_every_epilogue_row_against_the_torch_chain(form, stride, k):
    """odd sizes (the last stride-2 output column reads the padding), two images, channel counts off every granule"""
    kind = cr.EPILOGUES[form].get("kind", "plain")
    ins = cr.inputs(6, 8, k, stride, 2, 9, 11, kind=kind)
    ref = cr.reference_of(ins, form, stride)
    _same(ref.out, _chain(ins, form, stride, False), f"{form} k{k} s{stride}")
    assert bool((ref.mag >= ref.acc.abs()).all())
    assert ref.out.dtype == ref.mag.dtype == ref.lip.dtype == torch.float64


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("form", ["none", "relu", "res", "gain", "gain+res", "sigmoid"])
def test_pixel_shuffle_rows(form, k):
    """shuffle alone, with a residual laid out like the shuffled output, and the documented gain row (gain per original channel, then
    the shuffle); mag and lip follow their elements through the shuffle"""
    kind = cr.EPILOGUES[form].get("kind", "plain")
    ins = cr.inputs(5, 12, k, 1, 2, 7, 9, shuffle=True, kind=kind)
    ref = cr.reference_of(ins, form, 1, shuffle=True)
    assert ref.out.shape == (2, 3, 14, 18) == ref.mag.shape == ref.lip.shape
    _same(ref.out, _chain(ins, form, 1, True), f"{form} k{k} shuffled")
    plain = cr.reference_of(ins, "none", 1)
    assert torch.equal(ref.mag, F.pixel_shuffle(plain.mag, 2)) and bool((ref.mag >= F.pixel_shuffle(ref.acc.abs(), 2)).all())
    if cr.EPILOGUES[form].get("gain"):
        assert torch.equal(ref.lip, F.pixel_shuffle(ins["gain"].double().abs().view(1, -1, 1, 1).expand(2, 12, 7, 9), 2))


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_gdn_rows_against_the_oracle_module(inverse, with_res):
    from oracle.cai.layers import GDN
    ins = cr.inputs(16, 16, 1, 1, 2, 7, 9, kind="gdn")
    m = GDN(16, inverse=inverse).double()
    with torch.no_grad():
        m.beta.copy_(m.beta_reparam.init(ins["b"].double()))
        m.gamma.copy_(m.gamma_reparam.init(ins["w"].double().view(16, 16)))
        beta, gamma = m.beta_reparam(m.beta), m.gamma_reparam(m.gamma)       # what the module uses, to the last bit
        want = m(ins["x"].double()) + (ins["res"].double() if with_res else 0)
    ref = cr.reference(ins["x"], gamma.view(16, 16, 1, 1), beta, square=True, epi="igdn" if inverse else "gdn", mul=ins["x"],
                       res=ins["res"] if with_res else None)
    _same(ref.out, want, "gdn")
    assert float((beta - ins["b"].double()).abs().max()) < 1e-9 and float((gamma.view(-1) - ins["w"].double().view(-1)).abs().max()) < 1e-9
    form = ("igdn+res" if inverse else "gdn+res") if with_res else "gdn"
    if not (inverse and not with_res):
        _same(cr.reference_of(ins, form).out, want, "gdn through the named form")
    assert bool((ref.mag >= ref.acc.abs()).all())


@pytest.mark.parametrize("c", [16, 64, 128])
def test_gdn_inputs_keep_the_accumulator_away_from_zero(c):
    """beta >= 0.5 and gamma >= 0 on x^2 >= 0: every accumulator >= 0.5, so lip is bounded (|mul| / (2 acc^1.5) <= 1.42 |mul|)"""
    ins = cr.inputs(c, c, 1, 1, 2, 9, 13, kind="gdn")
    assert float(ins["b"].min()) >= 0.5 and float(ins["w"].min()) >= 0.0
    ref = cr.reference_of(ins, "gdn+res")
    assert float(ref.acc.min()) >= 0.5 and bool(torch.isfinite(ref.lip).all())
    assert ins["mul"] is ins["x"]


@pytest.mark.parametrize("form", list(cr.EPILOGUES))
def test_lip_bounds_a_finite_difference_of_the_reference(form):
    """perturb the bias of one channel (= every accumulator of that channel) by +-d: |out(+d) - out(-d)| <= 2 d lip' with lip' the
    largest lip over the interval (the endpoints' and the centre's: the bounds are constants or monotone in acc); and on elements away
    from the kinks the slope is not much smaller than lip where lip is the exact derivative (sigmoid excluded: 1/4 is its maximum)"""
    f = cr.EPILOGUES[form]
    kind = f.get("kind", "plain")
    c = 8
    ins = cr.inputs(c, c, 1, 1, 1, 5, 7, kind=kind)
    d = 1e-6

    def at(delta):
        b = ins["b"].double().clone()
        b[3] += delta
        return cr.reference(ins["x"], ins["w"], b, act=f.get("act", "none"), slope=f.get("slope", 0.01), square=f.get("square", False),
                            epi=f.get("epi", "none"), mul=ins["mul"] if f.get("mul") else None, res=ins["res"] if f.get("res") else None,
                            res_first=f.get("res_first", False), chscale=ins["gain"] if f.get("gain") else None)
    lo, mid, hi = at(-d), at(0.0), at(d)
    diff = (hi.out - lo.out).abs()
    lip = torch.maximum(torch.maximum(lo.lip, hi.lip), mid.lip)
    assert bool((diff[:, 3] <= 2 * d * lip[:, 3] * (1 + 1e-6) + 1e-18).all()), form
    assert float(diff[:, :3].abs().max()) == 0.0 and float(diff[:, 4:].abs().max()) == 0.0        # other channels do not move
    if f.get("act", "none") == "none":      # identity / GDN / IGDN: lip is the derivative itself
        assert bool((diff[:, 3] >= 2 * d * mid.lip[:, 3] * (1 - 1e-4)).all()), form


def test_sigmoid_and_clamp_inputs_reach_both_ends():
    for c in (4, 32, 128):
        ins = cr.inputs(c, c, 3, 1, 1, 9, 13, kind="wide")
        acc = cr.reference_of(ins, "none").acc
        assert float(acc.min()) < -4 and float(acc.max()) > 5
        assert bool(((acc > 0) & (acc < 1)).any()) and bool(((acc - 1).abs() < 0.1).any()) and bool((acc.abs() < 0.1).any())


def test_half_exact_inputs_survive_the_round_trip():
    for kind in ("plain", "wide"):
        ins = cr.inputs(32, 32, 3, 1, 2, 9, 13, kind=kind, half_exact=True)
        for name in ("x", "w", "res"):
            t = ins[name]
            assert t.dtype == torch.float32 and torch.equal(t.half().float(), t), name
    plain = cr.inputs(32, 32, 3, 1, 2, 9, 13)
    assert not torch.equal(plain["x"].half().float(), plain["x"])        # (the property is not a vacuous one)


def test_gain_has_mixed_signs_and_the_stated_range():
    g = cr.inputs(64, 128, 3, 1, 1, 9, 13)["gain"]
    assert float(g.abs().min()) >= 0.01 and float(g.abs().max()) <= 3.0 and bool((g < 0).any()) and bool((g > 0).any())
    assert float(g.abs().min()) < 0.05 and float(g.abs().max()) > 1.0


def test_allowance_and_ratio():
    ins = cr.inputs(8, 8, 3, 1, 1, 5, 7)
    ref = cr.reference_of(ins, "gain+res")
    a = cr.allowance(ref)
    assert torch.equal(a, ref.lip * 6e-7 * ref.mag + 4 * 2.0 ** -23 * ref.out.abs())
    assert torch.equal(cr.allowance(ref, True), ref.lip * 6e-7 * ref.mag + (4 * 2.0 ** -23 + 2.0 ** -11) * ref.out.abs())
    assert cr.worst_ratio(ref.out, ref) == 0.0
    assert abs(cr.worst_ratio(ref.out + 0.5 * a, ref) - 0.5) < 1e-6
    with pytest.raises(AssertionError):
        bad = ref.out.clone()
        bad[0, 0, 0, 0] = float("nan")
        cr.worst_ratio(bad, ref)


def test_fp32_operator_chain_on_the_gdn_cases_with_a_residual():
    """tests/test_conv_gpu.py::CPU_FP32 records what the float32 torch operators need on the two GDN cases whose bar is twice that
    figure.  Measured again here (printed); the recorded figure may not be generous: at most 1.5 x what this CPU measures."""
    recorded = {"gdn+res": 1.084, "igdn+res": 0.920}
    ins = cr.inputs(128, 128, 1, 1, 2, 11, 37, False, "gdn")
    norm = F.conv2d(ins["x"] * ins["x"], ins["w"], ins["b"])
    for form, rec in recorded.items():
        v = ins["x"] * (torch.sqrt(norm) if form.startswith("igdn") else 1.0 / torch.sqrt(norm)) + ins["res"]
        measured = cr.worst_ratio(v, cr.reference_of(ins, form))
        print(f"fp32 torch chain, 128 -> 128 {form}: {measured:.3f} x the allowance (recorded {rec})")
        assert rec <= 1.5 * measured
