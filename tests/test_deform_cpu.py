"""Host side of the deformable convolution (csrc/deform.hip: vc_deform_pack_weights) and the reference of tests/test_deform_gpu.py
pinned on the CPU: the float32 oracle stays below the caps against the float64 oracle on the inputs of the GPU case table, and at
the crafted boundary positions both precisions take identical decisions -- so no GPU case has to be left out for the reference's sake."""
import ctypes

import numpy as np
import pytest
import torch

import deform_ref as dr
from vcamd import hip


def _pack(w, cout, cg, groups, dst):
    return hip.lib().vc_deform_pack_weights(None if w is None else w.ctypes.data, cout, cg, groups, None if dst is None else dst.ctypes.data)


@pytest.mark.parametrize("groups", [2, 6, 16, 32])
@pytest.mark.parametrize("cg,og", dr.PAIRS)
def test_pack_weights_is_the_transposition(cg, og, groups):
    """[G * og][cg][3][3] -> [G][9][cg][og]"""
    rng = np.random.default_rng(100 * cg + 10 * og + groups)
    w = rng.standard_normal((groups * og, cg, 3, 3)).astype(np.float32)
    dst = np.full(groups * 9 * cg * og + 8, np.float32(dr.SENTINEL))
    assert _pack(w, groups * og, cg, groups, dst) == hip.VC_OK
    want = w.reshape(groups, og, cg, 9).transpose(0, 3, 2, 1)
    assert np.array_equal(dst[:-8].reshape(groups, 9, cg, og), want)
    assert np.array_equal(dst[-8:], np.full(8, np.float32(dr.SENTINEL)))        # nothing behind the last weight


def test_pack_weights_refuses_bad_arguments():
    w = np.ones((8, 4, 3, 3), dtype=np.float32)
    dst = np.full(8 * 4 * 9, np.float32(dr.SENTINEL))
    for args in ((None, 8, 4, 2, dst), (w, 8, 4, 2, None), (w, 8, 4, 3, dst), (w, 8, 0, 2, dst), (w, 8, -4, 2, dst), (w, 8, 4, 0, dst),
                 (w, 8, 4, -2, dst)):
        assert _pack(*args) == -1, args[1:4]
        assert np.array_equal(dst, np.full_like(dst, np.float32(dr.SENTINEL)))
    assert _pack(w, 8, 4, 2, dst) == hip.VC_OK
    assert np.array_equal(dst, np.ones_like(dst))


@pytest.mark.parametrize("cg,og,groups", dr.GENERIC_SHAPES)
def test_float32_oracle_holds_the_generic_cap_against_float64(cg, og, groups):
    worst = 0.0
    for h, w in dr.SIZES + (dr.TINY if (cg, og) == (8, 4) else []):
        x, off, msk, wt, b = dr.generic_inputs(cg, og, groups, h, w)
        for m, bb in ((msk, b), (None, None)):
            worst = max(worst, dr.rel_err(dr.ref_generic(x, off, wt, bb, m, torch.float32), dr.ref_generic(x, off, wt, bb, m)))
    print(f"generic cg={cg} og={og} G={groups}: float32 oracle within {worst:.2e} of float64")
    assert worst < dr.CAP_GENERIC / 2


@pytest.mark.parametrize("cg,og,groups", dr.FUSED_SHAPES)
def test_float32_oracle_holds_the_fused_cap_against_float64(cg, og, groups):
    worst = 0.0
    for h, w in dr.SIZES + (dr.TINY if (cg, og) == (8, 4) else []):
        *ins, wt, b = dr.fused_inputs(cg, og, groups, h, w)
        assert (h, w) == (1, 1) or not (torch.isfinite(ins[2]).all() or torch.isfinite(ins[5]).all())     # (the broken flow vectors)
        r64 = dr.ref_fused(*ins, dr.FUSED_MAGNITUDE, wt, b)
        assert r64.dtype == torch.float64 and torch.isfinite(r64).all()
        worst = max(worst, dr.rel_err(dr.ref_fused(*ins, dr.FUSED_MAGNITUDE, wt, b, torch.float32), r64))
        worst = max(worst, dr.rel_err(dr.ref_fused(*ins, dr.FUSED_MAGNITUDE, wt, b, torch.float32, half_features=True),
                                      dr.ref_fused(*ins, dr.FUSED_MAGNITUDE, wt, b, half_features=True)))
    print(f"fused cg={cg} og={og} G={groups}: float32 oracle within {worst:.2e} of float64")
    assert worst < dr.CAP_FUSED / 2


def test_fused_reference_is_the_oracle_module():
    """ref_fused in float32 == oracle.icip2024.OffsetDiversity.forward (16 groups) bit for bit: the same preparation, the same
    operator -- except at the two pixels with a broken flow vector, where the module's arithmetic gives NaN (inf - inf in the bilinear
    weights) and ref_fused, like the kernels, drops the taps"""
    from oracle import icip2024 as oi
    *ins, wt, b = dr.fused_inputs(8, 4, 16, 9, 19)
    m = oi.OffsetDiversity(64, dr.FUSED_MAGNITUDE)
    with torch.no_grad():
        m.fusion.weight.copy_(wt)
        m.fusion.bias.copy_(b)
        want = m(*ins)
    got = dr.ref_fused(*ins, dr.FUSED_MAGNITUDE, wt, b, torch.float32)
    broken = ~torch.isfinite(want)
    assert torch.isfinite(got).all() and 0 < broken.sum().item() <= 2 * want.shape[1]
    assert torch.equal(got[~broken], want[~broken])


@pytest.mark.parametrize("h,w", dr.SIZES)
def test_boundary_positions_are_exact_and_decided_alike_in_both_precisions(h, w):
    x, off, msk, wt, b, slots, dead = dr.boundary_inputs(8, 4, 8, h, w)
    p32, p64 = dr.corner_validity(off, h, w, torch.float32), dr.corner_validity(off, h, w, torch.float64)
    idx = tuple(torch.tensor(v) for v in zip(*[(i, g, k, y, xx) for i, g, k, y, xx, _, _ in slots]))
    for a32, a64 in zip(p32[:2], p64[:2]):                     # positions: exact
        assert torch.equal(a32[idx].double().nan_to_num(7e7), a64[idx].nan_to_num(7e7))
    for a32, a64 in zip(p32[2:], p64[2:]):                     # inside + four corner decisions: identical at EVERY tap of the tensor
        assert torch.equal(a32, a64)
    py, px = p64[0][idx], p64[1][idx]
    for ty in dr.boundary_values(h):                            # every boundary value is really sampled (slots can overwrite each other)
        assert (py == ty).any(), ty
    for tx in dr.boundary_values(w):
        assert (px == tx).any(), tx
    for ty in (-1.0, h - 1.0 + dr.EPS, float(h)):
        for tx in (-1.0, w - 1.0 + dr.EPS, float(w)):
            assert ((py == ty) & (px == tx)).any(), (ty, tx)
    inside = p64[2]
    for i, y, xx in dead:
        assert not inside[i, :, :, y, xx].any()
    assert not torch.isfinite(off).all()
    r64 = dr.ref_generic(x, off, wt, b, msk)
    assert torch.isfinite(r64).all()
    for i, y, xx in dead:
        assert torch.equal(r64[i, :, y, xx], b.double())
    d = dr.rel_err(dr.ref_generic(x, off, wt, b, msk, torch.float32), r64)
    print(f"boundary inputs {h}x{w}: float32 oracle within {d:.2e} of float64")
    assert d < dr.CAP_GENERIC / 2


def test_window_helpers_round_trip():
    """place / read_window of deform_ref.py (CPU 'device'): the window holds the tensor, everything else the fill value"""
    x = torch.randn(2, 6, 3, 5)
    t = dr.place(x, "cpu", c0=1, cpad=4, hpad=2, wpad=3, n0=1, npad=2, fill=dr.SENTINEL)
    assert (t.n, t.h, t.w, t.c, t.sw, t.sh, t.sn) == (2, 3, 5, 6, 10, 80, 400) and t.off == 401
    win, outside = dr.read_window(t)
    assert torch.equal(win, x) and outside.numel() == 4 * 5 * 8 * 10 - x.numel()
    dr.assert_untouched(outside)
    assert ctypes.sizeof(hip.View) == 48
