"""The references and case tables of tests/test_ew_gpu.py pinned on the CPU (tests/ew_ref.py): every float64 restatement equals the
torch operator the reference project calls, evaluated in float64 (torch.sigmoid, torch.round, .half(), torch.clamp, permute); every
row-map case lands in the regime its id names; on every input the GPU module uses, the reference project's own fp32 evaluation stays
inside the bound the kernel is held to -- so a kernel that misses a bound has no excuse in the inputs; the coverage table names, for
every entry point, a test that exists for each of dense, window, edge and contract."""
import ast
import inspect
import textwrap

import numpy as np
import pytest
import torch

import ew_ref as er
import resample_ref as rr

MAXIMA = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(MAXIMA):
        print(f"\nfp32 CPU expression against float64, largest |d| / (u M), {k}: {MAXIMA[k]:.2f} of {er.BOUND[k]:.0f}", end="")


def _hold(entry, what, out, ref, mag):
    assert torch.isfinite(ref).all(), f"{entry} {what}: the float64 reference is not finite"
    q = er.units(out, ref, mag)
    MAXIMA[entry] = max(MAXIMA.get(entry, 0.0), q)
    assert q <= er.BOUND[entry], f"{entry} {what}: the fp32 expression itself is {q:.2f} u M from float64, bound {er.BOUND[entry]}: a bad case"


def _same_bits64(a, b):
    return torch.equal(a.to(er.F64).contiguous().view(torch.int64), b.to(er.F64).contiguous().view(torch.int64))


BASE_SHAPES = [(er.N, h, w) for h, w in er.SHAPES]
ALL_SHAPES = BASE_SHAPES + [er.BLEND_LARGER] + sorted({(c.n, c.h, c.w) for c in er.ROWMAP_CASES if c.entry in ("vc_lhbdc_blend", "vc_flex_blend")})


# ---- the restatements are the torch operators ----
def test_logistic_rounding_and_clamp_are_the_torch_operators_in_float64():
    b = torch.cat((torch.tensor(er.GATE_B_EDGES), rr.rand((4096,), 1, -30, 30))).double()
    d = (er.sigmoid(b) - torch.sigmoid(b)).abs() / torch.sigmoid(b)
    assert float(d.max()) <= 4 * 2.0 ** -53, float(d.max())           # two roundings apart at most; -104 does not underflow in float64
    assert float(er.sigmoid(torch.tensor([-104.0]))) > 0
    x = torch.cat((torch.tensor(er.QUANT_EDGES), torch.arange(-9, 10) * 0.5, rr.rand((4096,), 2, -40, 40))).double()
    assert _same_bits64(er.round_half_even(x), torch.round(x))          # bits: round(-0.5) and round(-0.0) are -0.0
    ties = torch.tensor([0.5, -0.5, 1.5, -1.5, 2.5, -2.5])
    assert er.round_half_even(ties).tolist() == [0.0, -0.0, 2.0, -2.0, 2.0, -2.0]
    c = torch.tensor(er.CLAMP_EDGES).double()
    assert _same_bits64(er.clamp01(c), torch.clamp(c, 0, 1))
    c32 = torch.tensor(er.CLAMP_EDGES)
    assert torch.equal(rr.bits(er.clamp01(c32)), rr.bits(er.F32.clamp01(c32)))
    assert er.FLEX_EPS == float(np.float32(1e-8)) != 1e-8


def test_half_and_layout_restatements_are_the_torch_operators():
    for cg in er.PLANAR_CG:
        x = er.half_inputs(2, 2 * cg, 3, 5, edge=True)
        assert torch.equal(er.to_half(x), er.F32.to_half(x))
        assert torch.equal(er.to_half_planar(x, cg), er.F32.to_half_planar(x, cg))
    e = torch.tensor(er.HALF_EDGES).view(1, -1, 1, 1)
    got = dict(zip(er.HALF_EDGES, er.to_half(e).view(-1).tolist()))
    # ties to even, overflow to inf, the smallest normal, subnormal results rounded and not flushed
    assert got[1 + 2.0 ** -11] == 0x3c00 and got[1 + 3 * 2.0 ** -11] == 0x3c02 and got[65504.0] == 0x7bff and got[65520.0] == 0x7c00
    assert got[2.0 ** -14] == 0x0400 and got[2.0 ** -24] == 1 and got[2.0 ** -25] == 0 and got[3 * 2.0 ** -25] == 2
    for c in er.LAYOUT_C:
        x = er.distinct(2, c, 3, 5)
        assert x.unique().numel() == x.numel()
        assert torch.equal(er.to_nhwc(x), x.permute(0, 2, 3, 1))


def test_split_records_are_exact_on_the_special_values():
    x = er.split_inputs(2, 8, 3, 5, edge=True)
    rec = rr.split_host(x)
    assert torch.equal(rr.unsplit(rec, 2, 8, 3, 5), x.double())
    hi, mid, lo = er.pieces(rec, 2, 8, 3, 5)
    assert torch.equal(rr.bits((hi + mid) + lo), rr.bits(torch.where(x == 0, torch.zeros_like(x), x)))   # (-0 splits into +0 pieces' sum)
    p = er.split_pad_host(x[:, :3], 8)
    assert not bool(er.pieces(p, 2, 8, 3, 5)[:, :, 3:].view(torch.int32).any())


def test_quantize_mask_restatement_is_the_reference_slicing():
    for h, w in [(9, 19), (3, 37), (1, 1), (4, 6)]:
        x, gain = er.quant_inputs(2, 5, h, w, edge=True)
        for parity in (-1, 0, 1):
            for do_round in (0, 1):
                for g in (None, gain):
                    ref = er.quantize_mask(x, g, parity, do_round)
                    f32 = er.F32.quantize_mask(x, g, parity, do_round)
                    f64 = er.F32.quantize_mask(x.double(), None if g is None else g.double(), parity, do_round)
                    assert _same_bits64(ref, f64)
                    if g is None:
                        assert torch.equal(rr.bits(f32), rr.bits(ref.float()))
    # keep_parity 1 keeps (y + x) odd: the "anchors" slicing of the reference zeroes [0::2, 0::2] and [1::2, 1::2]
    k = er.keep_mask(3, 5, 1)
    assert not k[0, 0] and k[0, 1] and k[1, 0] and not k[1, 1] and not k[2, 4]
    # the gain comes after the rounding
    x, gain = er.quant_inputs(2, 5, 9, 19)
    assert not torch.equal(er.quantize_mask(x, gain, -1, 1), er.round_half_even(x.double() * gain.double().view(1, -1, 1, 1)))


# ---- the reference's fp32 evaluation stays inside the bounds on the inputs the GPU module uses ----
@pytest.mark.parametrize("edge", [False, True])
def test_blends_fp32_within_the_bounds(edge):
    for n, h, w in ALL_SHAPES:
        fw, bw, m, cur = er.lhbdc_inputs(n, h, w, edge)
        pred, resid, mp, mr = er.lhbdc_blend(fw, bw, m, cur)
        p32, r32 = er.F32.lhbdc_blend(fw, bw, m, cur)
        _hold("vc_lhbdc_blend", f"pred {n}x{h}x{w}", p32, pred, mp)
        _hold("vc_lhbdc_blend", f"resid {n}x{h}x{w}", r32, resid, mr)
        xb, xa, mask, cur = er.flex_inputs(n, h, w, edge)
        pred, resid, mp, mr = er.flex_blend(xb, xa, mask, cur)
        p32, r32 = er.F32.flex_blend(xb, xa, mask, cur)
        _hold("vc_flex_blend", f"pred {n}x{h}x{w}", p32, pred, mp)
        _hold("vc_flex_blend", f"resid {n}x{h}x{w}", r32, resid, mr)
    if edge:
        fw, bw, m, cur = er.lhbdc_inputs(2, 9, 19, True)
        assert {0.0, 1.0, 2.0 ** -24} <= set(m.unique().tolist()) and bool((fw < 0).any()) and bool((fw > 0).any())
        assert torch.equal(cur[1], fw[1]) and torch.equal(bw[1], fw[1])
        _, _, mask, _ = er.flex_inputs(2, 9, 19, True)
        pairs = {tuple(p) for p in mask.permute(0, 2, 3, 1).reshape(-1, 2).tolist()}
        assert pairs == {(float(np.float32(a)), float(np.float32(b))) for a, b in er.FLEX_MASK_EDGES}
        both0 = (mask == 0).all(1, keepdim=True).expand(-1, 3, -1, -1)
        assert bool(both0.any()) and not bool(er.flex_blend(*er.flex_inputs(2, 9, 19, True))[0][both0].any())


@pytest.mark.parametrize("t", er.MOTION_T)
def test_motion_split_fp32_within_the_bound(t):
    for n, h, w in BASE_SHAPES:
        f = er.motion_inputs(n, h, w, 6)
        ft0, ft1, m0, m1 = er.motion_split(f, t)
        a, b = er.F32.motion_split(f, t)
        _hold("vc_flex_motion_split", f"ft0 t={t}", a, ft0, m0)
        _hold("vc_flex_motion_split", f"ft1 t={t}", b, ft1, m1)


@pytest.mark.parametrize("edge", [False, True])
def test_attention_gate_and_preprocess_fp32_within_the_bounds(edge):
    for case in [c for c in er.ROWMAP_CASES if c.entry == "vc_attention_gate" and not edge]:
        a, b, identity = er.gate_inputs(case.n, case.c, case.h, case.w)
        ref, mag = er.attention_gate(a, b, identity)
        _hold("vc_attention_gate", case.id, er.F32.attention_gate(a, b, identity), ref, mag)
    for n, h, w in BASE_SHAPES:
        a, b, identity = er.gate_inputs(n, 5, h, w, edge)
        ref, mag = er.attention_gate(a, b, identity)
        _hold("vc_attention_gate", f"{n}x{h}x{w}", er.F32.attention_gate(a, b, identity), ref, mag)
        x = er.spynet_inputs(n, h, w, edge)
        ref, mag = er.spynet_preprocess(x)
        _hold("vc_spynet_preprocess", f"{n}x{h}x{w}", er.F32.spynet_preprocess(x), ref, mag)
    if edge:
        a, b, identity = er.gate_inputs(2, 5, 9, 19, True)
        assert set(b.unique().tolist()) == {float(np.float32(v)) for v in er.GATE_B_EDGES} and not bool(a[0].any())
        ref, _ = er.attention_gate(a, b, identity)
        assert torch.equal(ref[0], identity[0].double())                  # the identity alone carries the value
        x = er.spynet_inputs(2, 9, 19, True)
        out = er.F32.spynet_preprocess(x)
        for i in range(3):                                                # the input channel's own mean gives 0 in output channel 2 - i
            at = x[:, i] == np.float32(er.MEANS[i])
            assert bool(at.any()) and not bool(out[:, 2 - i][at].any())
        assert len({x[0, i, 0, 3].item() for i in range(3)}) == 3


# ---- the case tables ----
def test_every_row_map_case_lands_in_its_regime():
    for case in er.ROWMAP_CASES + [er.ROWLOOP]:
        m = rr.rowmap(case.n, case.h, case.w, case.per_px)
        if case.regime == "fallback":
            assert m is None, case.id
        elif case.regime == "wide":
            assert m is not None and m.bx > 1 and not m.loops and (case.w * case.per_px) % rr.EW_BLOCK, case.id
        else:
            assert m is not None and m.loops and m.gy == 64 < case.h, case.id
    entries = {c.entry for c in er.ROWMAP_CASES}
    assert entries == {"vc_lhbdc_blend", "vc_flex_blend", "vc_attention_gate", "vc_quantize_mask", "vc_channel_scale", "vc_clamp01",
                       "vc_to_half", "vc_to_half_planar"}
    for e in entries:
        assert {c.regime for c in er.ROWMAP_CASES if c.entry == e} == {"wide", "fallback"}
    base = rr.AXPBY_ROWLOOP
    assert (er.ROWLOOP.n, er.ROWLOOP.h, er.ROWLOOP.w, er.ROWLOOP.c) == (base.n, base.h, base.w, base.c)
    # the base shapes stay in the row form with one workgroup a row
    for h, w in er.SHAPES:
        m = rr.rowmap(er.N, h, w, 8)
        assert m is not None and not m.loops


def test_every_view_set_tries_every_argument_in_every_kind_of_view():
    for table in (er.SPECS, er.ALIGNED):
        for count in (2, 3, 5, 6):
            seen = [set() for _ in range(count)]
            for vs in er.VIEWSETS:
                for i, spec in enumerate(er.specs_of(vs, count, table)):
                    seen[i].add(id(spec))
            assert all(s == {id(t) for t in table} for s in seen)
    for spec in er.ALIGNED:
        g = rr.geom((2, 8, 3, 5), **spec)
        assert rr.vec4(g)
    assert not rr.vec4(rr.geom((2, 8, 3, 5), **rr.WIN_U))


def _names_used(gpu, fn, seen):
    """the attribute names and string constants (docstrings apart) in the code of `fn`, decorators included, and of every helper of
    tests/test_ew_gpu.py it reaches: what the test can call"""
    tree = ast.parse(textwrap.dedent(inspect.getsource(fn)))
    doc = ast.get_docstring(tree.body[0], clean=False) if isinstance(tree.body[0], ast.FunctionDef) else None
    out = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute):
            out.add(node.attr)
        elif isinstance(node, ast.Constant) and isinstance(node.value, str) and node.value != doc:
            out.add(node.value)
        elif isinstance(node, ast.Name) and node.id not in seen and not node.id.startswith("test_"):
            helper = getattr(gpu, node.id, None)
            if inspect.isfunction(helper) and helper.__module__ == gpu.__name__:
                seen.add(node.id)
                out |= _names_used(gpu, helper, seen)
    return out


def _views_run(fn):
    """the values of the `viewset` / `spec` parameter the test is parametrised over"""
    vals = set()
    for mark in getattr(fn, "pytestmark", []):
        if mark.name == "parametrize":
            names = [a.strip() for a in mark.args[0].split(",")]
            for key in ("viewset", "spec"):
                if key in names:
                    vals |= {v[names.index(key)] if len(names) > 1 else v for v in mark.args[1]}
    return vals


def test_every_entry_point_has_a_dense_a_window_an_edge_and_a_contract_test():
    """from what tests/test_ew_gpu.py runs, not from its docstrings: the code of each named test (and of the helpers it reaches)
    names the entry point as a call or as the parameter that selects it; the dense test is parametrised over a dense view set, the
    window test over both kinds of window.  The issue's fifteen entry points are fourteen by name; the fifteenth here is vc_blend,
    the operator spelling of vc_lhbdc_blend in csrc/abi_aliases.cpp."""
    import test_ew_gpu as gpu
    assert sorted(er.COVERAGE) == sorted(er.ENTRY_POINTS) and len(er.ENTRY_POINTS) == 15
    for entry, row in er.COVERAGE.items():
        assert set(row) == {"dense", "window", "edge", "contract"}, entry
        for kind, name in row.items():
            fn = getattr(gpu, name, None)
            assert callable(fn) and name.startswith("test_"), f"{entry} {kind}: tests/test_ew_gpu.py has no {name}"
            assert entry in _names_used(gpu, fn, set()), f"{entry} {kind}: the code of {name} never names the entry point"
            views = _views_run(fn)
            if kind == "dense":
                assert "dense" in views or 0 in views, f"{entry}: {name} runs no dense view"
            if kind == "window":
                assert {"rot0", "rot1", "rot2"} <= views or {1, 2} <= views, f"{entry}: {name} runs no windows"
    # a test whose body stopped calling its entry point is seen
    assert "vc_clamp01" not in _names_used(gpu, gpu.test_channel_scale_views, set())
