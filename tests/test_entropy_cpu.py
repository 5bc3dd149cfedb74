"""The plain entropy reference (tests/entropy_ref.py) kept honest without a GPU, and the conditions its input generators promise to
tests/test_entropy_gpu.py:

  * the reference agrees with the oracle's fp32 EntropyBottleneck / GaussianConditional modules: integers and de-quantised values
    exact, likelihoods within 4 * K_ref * m_i of the float64 ones (K_ref measured on the reference run in float32, see the GPU
    module's docstring for the error model);
  * >= 256 double-rounding ties in every contraction probe; zero near-ties in every generated tensor; >= 1 000 Gaussian elements in
    every likelihood bucket of the range case;
  * the layout guard of sym_src in vcamd/layers.py.
"""
import numpy as np
import pytest
import torch

import entropy_ref as R

SHAPES = [(1, 1, 1, 1), (1, 3, 5, 7), (3, 20, 9, 11), (2, 96, 37, 37)]
RANGE_SHAPE = (2, 96, 37, 37)


def _oracle_eb(params_from_module_seed, c):
    from oracle.cai.entropy_models import EntropyBottleneck as OEB
    from vcamd.layers import EntropyBottleneck
    from vcamd.seeding import seeded_state_dict
    o = OEB(c)
    sd = seeded_state_dict(o.state_dict(), params_from_module_seed)
    o.load_state_dict(sd)
    eb = EntropyBottleneck(c)
    eb.load_state_dict(sd)
    return o.eval(), eb.device_params().cpu()


def test_reference_matches_the_oracle_entropy_bottleneck():
    c = 20
    o, params = _oracle_eb(41, c)
    assert params.shape == (c, R.EB_STRIDE)
    assert torch.equal(params[:, 58], o.quantiles[:, 0, 1].detach())
    z = R.eb_inputs((3, c, 9, 11), params, 5, wide=True)
    with torch.no_grad():
        z_ref, lik_o = o(z)
    sym, q, hat = R.quantise(z, params[:, 58].reshape(1, -1, 1, 1))
    assert torch.equal(hat, z_ref) and torch.equal(q, z_ref)
    assert torch.equal(sym, torch.round(z - params[:, 58].reshape(1, -1, 1, 1)).int())
    lik64, U, L = R.eb_likelihood(q, params, R.F64)
    lik32, _, _ = R.eb_likelihood(q, params, R.F32)
    m = R.error_model(lik64, U, L)
    k_ref = float(R.k_of(lik32, lik64, m).max())
    k_oracle = float(R.k_of(lik_o, lik64, m).max())
    print(f"EB oracle table: K_ref {k_ref:.2f}, oracle module K {k_oracle:.2f}")
    assert k_ref > 0 and k_oracle <= 4 * k_ref
    rb = float((-torch.log2(lik_o.double())).sum())
    assert abs(R.bits(lik64) - rb) / rb < 1e-5


def test_reference_matches_the_oracle_gaussian_conditional():
    from oracle.cai.entropy_models import GaussianConditional as OGC, get_scale_table
    gc = OGC(None)
    gc.update_scale_table(get_scale_table(), force=True)
    table = R.scale_table()
    assert torch.equal(table, gc.scale_table)
    y, s, mu = R.gc_inputs(RANGE_SHAPE, 11, wide=True)
    with torch.no_grad():
        y_ref, lik_o = gc(y, s, means=mu)
        idx_o = gc.build_indexes(s)
    sym, q, hat = R.quantise(y, mu)
    assert torch.equal(hat, y_ref)
    assert torch.equal(sym, torch.round(y - mu).int())
    assert torch.equal(R.scale_indexes(s, table), idx_o)
    lik64, U, L = R.gc_likelihood(q, mu, s, R.F64)
    lik32, _, _ = R.gc_likelihood(q, mu, s, R.F32)
    m = R.error_model(lik64, U, L)
    k_ref = float(R.k_of(lik32, lik64, m).max())
    k_oracle = float(R.k_of(lik_o, lik64, m).max())
    print(f"GC: K_ref {k_ref:.2f}, oracle module K {k_oracle:.2f}")
    assert k_ref > 0 and k_oracle <= 4 * k_ref
    rb = float((-torch.log2(lik_o.double())).sum())
    assert abs(R.bits(lik64) - rb) / rb < 1e-5
    for name, mask in R.bucket_masks(lik64).items():
        rel = float(((lik32.double() - lik64).abs() / lik64)[mask].max())
        print(f"GC restatement, bucket {name}: {int(mask.sum())} elements, max relative error {rel:.2e}")


def test_index_probe_against_the_oracle():
    from oracle.cai.entropy_models import GaussianConditional as OGC, get_scale_table
    gc = OGC(None)
    gc.update_scale_table(get_scale_table(), force=True)
    table = R.scale_table()
    s = R.index_probe_scales(table)
    idx = R.scale_indexes(s, table)
    assert torch.equal(idx, gc.build_indexes(s))
    # s <= t is inclusive: an entry maps to its own index, one ulp above it to the next
    n = table.numel()
    assert idx[:n].tolist() == list(range(n))
    assert idx[n:2 * n].tolist() == [min(i + 1, n - 1) for i in range(n)]
    assert idx[2 * n:3 * n].tolist() == list(range(n))
    assert idx[3 * n:].tolist() == [0, 0, 0, 0, 0, n - 1, n - 1, n - 1, n - 1]


def test_gc_range_case_fills_every_likelihood_bucket():
    y, s, mu = R.gc_inputs(RANGE_SHAPE, 11, wide=True)
    assert y.numel() < 300_000 and bool(torch.isfinite(y).all())
    assert float((y - mu).abs().max()) < 2.0 ** 23
    for lit in (0.0, -3.0, 0.11, 256.0, 1e4):
        assert int((s == lit).sum()) >= 64
    assert float(s[s > 0].min()) < 0.06 and float(s[s < 1e3].max()) > 250.0
    _, q, _ = R.quantise(y, mu)
    lik64, _, _ = R.gc_likelihood(q, mu, s)
    counts = {k: int(v.sum()) for k, v in R.bucket_masks(lik64).items()}
    print("GC range case buckets:", counts)
    assert all(v >= 1000 for v in counts.values()), counts
    assert float(lik64.max()) > 0.99


def test_eb_range_case_saturates_and_clamps():
    params = R.hand_made_eb_table(96, 3)
    z = R.eb_inputs(RANGE_SHAPE, params, 7, wide=True)
    med = params[:, 58].reshape(1, -1, 1, 1)
    assert float((z - med).abs().max()) > 9e3 and float((z - med).abs().max()) < 2.0 ** 23
    _, q, _ = R.quantise(z, med)
    lik64, U, L = R.eb_likelihood(q, params)
    counts = {k: int(v.sum()) for k, v in R.bucket_masks(lik64).items()}
    print("EB range case buckets:", counts)
    assert counts["clamped"] > 0 and counts["ge1e-3"] > 0
    # both sigmoids saturated somewhere (the difference is exactly zero before the clamp)
    assert int(((U - L) == 0).sum()) > 0


def test_hand_made_tables_have_positive_matrices_small_factors_and_dyadic_medians():
    p = R.hand_made_eb_table(20, 3)
    mats = torch.cat([p[:, 0:3], p[:, 9:18], p[:, 24:33], p[:, 39:48], p[:, 54:57]], 1)
    facs = torch.cat([p[:, 6:9], p[:, 21:24], p[:, 36:39], p[:, 51:54]], 1)
    assert bool((mats > 0).all()) and bool((facs.abs() < 1).all())
    assert bool((p[:, 58] * 4 == torch.round(p[:, 58] * 4)).all()) and bool((p[:, 59] == 0).all())


@pytest.mark.parametrize("per_element", [False, True], ids=["median", "mu"])
def test_double_rounding_probe_yields_enough_ties(per_element):
    z, gain, centre, q = R.double_rounding_draws(96, 2084, 21, per_element)       # 200 064 draws
    n = int(q.sum())
    print(f"double-rounding ties: {n} of {q.numel()} draws")
    assert n >= 256
    # what the mark means, restated with numpy on the qualifying draws
    zz, cc = z[q].numpy(), (centre.expand_as(z) if not per_element else centre)[q].numpy()
    gg = gain.reshape(-1, 1).expand_as(z)[q].numpy()
    two = (zz * gg).astype(np.float32) - cc
    assert two.dtype == np.float32 and np.all(two - np.floor(two) == 0.5)
    one = (zz.astype(np.float64) * gg.astype(np.float64) - cc.astype(np.float64)).astype(np.float32)
    assert np.all(np.rint(one) != np.rint(two))
    for shape in ((96, 37, 37), (32, 24, 32)):
        zt, gt, ct, qt = R.double_rounding_tensor(*shape, 21, per_element)
        assert int(qt.sum()) >= 256, int(qt.sum())
        assert int(R.near_ties(zt, ct, gt).sum()) == 0
        sym, _, _ = R.quantise(zt, ct, gt)
        fused = torch.round((zt.double() * gt.double().reshape(1, -1, 1, 1) - ct.double()).float()).int()
        assert bool((sym[qt] != fused[qt]).all())


def test_generators_leave_no_near_ties():
    """No element of any generated tensor lies within 1e-3 of a half-integer unless it lies on it: the integer comparison of the GPU
    module excludes nothing."""
    excluded = 0
    for i, shape in enumerate(SHAPES):
        c = shape[1]
        params = R.hand_made_eb_table(c, 3)
        med = params[:, 58].reshape(1, -1, 1, 1)
        for ig in (None, R.gains(c, 50)):
            z = R.eb_inputs(shape, params, 7 + i, in_gain=ig, wide=(shape == RANGE_SHAPE))
            excluded += int(R.near_ties(z, med, ig).sum())
            y, s, mu = R.gc_inputs(shape, 11 + i, in_gain=ig, wide=(shape == RANGE_SHAPE))
            excluded += int(R.near_ties(y, mu, ig).sum())
            assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(y).all())
    assert excluded == 0
    # the other draws of the GPU module, seed for seed (gains, decoder agreement, sym_src, the seeded module table).  The generators
    # hold this by construction as well: clear_near_ties returns only a clean tensor and raises otherwise.
    shape, c = (3, 20, 9, 11), 20
    params = R.hand_made_eb_table(c, 3)
    med = params[:, 58].reshape(1, -1, 1, 1)
    for ig in (None, R.gains(c, 50)):
        excluded += int(R.near_ties(R.eb_inputs(shape, params, 31, in_gain=ig), med, ig).sum())
        y, _, mu = R.gc_inputs(shape, 32, in_gain=ig)
        excluded += int(R.near_ties(y, mu, ig).sum())
    excluded += int(R.near_ties(R.eb_inputs(shape, params, 41), med).sum())
    for seed in (42, 43):
        y, _, mu = R.gc_inputs(shape, seed)
        excluded += int(R.near_ties(y, mu).sum())
    gain = R.gains(c, 50)
    y_raw = R.clear_near_ties(y, [(mu, None), (mu, gain)])                       # sym_src: seed 43, clean both gained and un-gained
    excluded += int(R.near_ties(y_raw, mu).sum()) + int(R.near_ties(y_raw * gain.reshape(1, -1, 1, 1), mu).sum())
    from vcamd.layers import EntropyBottleneck
    from vcamd.seeding import seeded_state_dict
    eb = EntropyBottleneck(96)
    eb.load_state_dict(seeded_state_dict(eb.state_dict(), 41))
    params = eb.device_params().cpu()
    z = R.eb_inputs(RANGE_SHAPE, params, 9, wide=True)
    excluded += int(R.near_ties(z, params[:, 58].reshape(1, -1, 1, 1)).sum())
    assert excluded == 0


def test_exact_ties_round_half_to_even():
    g = np.random.default_rng(2)
    gain = torch.tensor([1.0, 2.0, 1.0, 2.0])
    for centre in (R.dyadic(g, (1, 4, 1, 1)), R.dyadic(g, (1, 4, 2, 81))):
        v = R.exact_ties(centre, gain)
        assert int((v < 0).sum()) > 100
        sym, q, _ = R.quantise(v, centre, gain)
        d = (v.double() * gain.double().reshape(1, -1, 1, 1) - centre.double())
        assert bool((d - torch.floor(d) == 0.5).all())
        lo = torch.floor(d).long()
        want = torch.where(lo % 2 == 0, lo, lo + 1)
        assert torch.equal(sym.long(), want)
        assert int((sym < 0).sum()) > 100 and int((sym % 2 != 0).sum()) == 0


def test_sym_src_must_share_the_layout_of_y():
    """k_gc_forward reads sym_src at y's element offsets: the host refuses an un-gained latent laid out differently."""
    from vcamd import hip
    from vcamd.layers import MeanScaleHyperprior
    check = MeanScaleHyperprior._check_sym_src_layout
    y = hip.T.empty(2, 4, 6, 8, "cpu")
    check(y, None)
    check(y, hip.T.empty(2, 4, 6, 8, "cpu"))
    wide = hip.T.empty(2, 4, 6, 24, "cpu")
    check(wide.channels(0, 8), wide.channels(8, 16))
    with pytest.raises(hip.VcError):
        check(y, wide.channels(8, 16))
    with pytest.raises(hip.VcError):
        check(wide.channels(8, 16), y)
    with pytest.raises(hip.VcError):
        check(y, hip.T.empty(2, 4, 6, 16, "cpu").channels(0, 8))
    with pytest.raises(hip.VcError):
        check(y, hip.T.empty(2, 4, 3, 8, "cpu"))
