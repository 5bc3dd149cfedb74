"""Plain reference of the entropy-model entry points (include/vc_hip.h, "Entropy models"), shared by tests/test_entropy_cpu.py and
tests/test_entropy_gpu.py, and the seeded input generators of both.

Written from the contract in the header, not by calling oracle/cai:

  quantisation   emulated in float32 one IEEE operation at a time, so every integer and every stored value is compared exactly:
                 p = fl32(v * in_gain), sym = rint(fl32(p - c)), q = fl32(sym + c), hat = fl32(q * out_gain);
                 c = the channel's median (factorised prior) or mu (Gaussian conditional)
  likelihoods    from the float32 q, in ``dtype`` (float64 = the reference, float32 = the restatement whose own error sizes the bound)
  indexes        (n_scales - 1) - #{t in table[:-1] : s <= t} on the float32 max(s, 0.11)

Every tensor is NCHW on the CPU.  Per-channel vectors (gains, medians) are 1-D of length C.
"""
import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
LIK_BOUND = 1e-9
SCALE_BOUND = 0.11
EB_STRIDE = 60                 # VC_EB_PARAMS_PER_CHANNEL
NEAR = 1e-3                    # no generated element lies this close to a half-integer unless it lies ON it
BUCKETS = ("ge1e-3", "1e-6..1e-3", "1e-9..1e-6", "clamped")


def _pc(v):
    """per-channel vector -> broadcastable over NCHW"""
    return None if v is None else v.reshape(1, -1, 1, 1)


def quantise(v, centre, in_gain=None, out_gain=None):
    """(sym int32, q, hat): the float32 emulation.  ``centre`` broadcasts against v (a [1,C,1,1] median or a full mu tensor)."""
    assert v.dtype == F32 and centre.dtype == F32
    p = v if in_gain is None else v * _pc(in_gain)            # one rounding
    d = p - centre                                            # a second one
    sym = torch.round(d)                                      # half to even
    q = sym + centre
    hat = q if out_gain is None else q * _pc(out_gain)
    for t in (p, d, q, hat):
        assert t.dtype == F32
    return sym.to(torch.int32), q, hat


def dequantise(sym, centre, out_gain=None):
    q = sym.to(F32) + centre
    return q if out_gain is None else q * _pc(out_gain)


def tie_distance(v, centre, in_gain=None):
    """| frac(d) - 1/2 | of the float32 d = fl32(fl32(v * gain) - c): 0 on an exact tie"""
    p = v if in_gain is None else v * _pc(in_gain)
    d = (p - centre).double()
    return ((d - torch.floor(d)) - 0.5).abs()


def near_ties(v, centre, in_gain=None):
    """elements that are close to a rounding boundary without being on it: the integer comparison never excludes an element, so the
    generators leave none of these"""
    t = tie_distance(v, centre, in_gain)
    return (t > 0) & (t < NEAR)


def clear_near_ties(v, conditions):
    """Move every element that is a near-tie under one of ``conditions`` (a list of (centre, in_gain)) until none is.  Exact ties stay."""
    v = v.clone()
    for it in range(64):
        bad = torch.zeros_like(v, dtype=torch.bool)
        for centre, gain in conditions:
            bad |= near_ties(v, centre, gain)
        if not bool(bad.any()):
            return v
        v = torch.where(bad, v + (0.137 + 0.01 * it), v)
    raise AssertionError("near-ties could not be cleared")


# ------------------------------------------------------------------------------------------------------------------------------
# likelihoods
# ------------------------------------------------------------------------------------------------------------------------------
def eb_logits(params, x, dtype):
    """the 1-3-3-3-3-1 cumulative MLP of one [C,60] table at x [N,C,H,W] (matrices row-major [out][in])"""
    P = params.to(dtype)
    col = lambda k: P[:, k].reshape(1, -1, 1, 1)
    x = x.to(dtype)
    l = []
    for i in range(3):
        t = col(i) * x + col(3 + i)
        l.append(t + col(6 + i) * torch.tanh(t))
    r = 9
    for _ in range(3):
        m = []
        for i in range(3):
            t = col(r + 3 * i) * l[0]
            t = t + col(r + 3 * i + 1) * l[1]
            t = t + col(r + 3 * i + 2) * l[2]
            t = t + col(r + 9 + i)
            m.append(t + col(r + 12 + i) * torch.tanh(t))
        l = m
        r += 15
    t = col(r) * l[0]
    t = t + col(r + 1) * l[1]
    t = t + col(r + 2) * l[2]
    return t + col(r + 3)


def eb_likelihood(q, params, dtype=F64):
    """(lik clamped at 1e-9, U, L) with U, L the two sigmoids before the subtraction.  The +-1/2 are applied in float32 like the
    float32 module does (exact whenever |q| < 2^22)."""
    assert q.dtype == F32
    lower = eb_logits(params, q - 0.5, dtype)
    upper = eb_logits(params, q + 0.5, dtype)
    sign = -torch.sign(lower + upper)
    U, L = torch.sigmoid(sign * upper), torch.sigmoid(sign * lower)
    lik = torch.clamp((U - L).abs(), min=LIK_BOUND)
    return lik, U, L


def gc_likelihood(q, mu, scales, dtype=F64):
    """(lik clamped at 1e-9, U, L): s = max(s, 0.11), a = |fl32(q - mu)|, Phi((.5 - a) / s) - Phi((-.5 - a) / s)"""
    assert q.dtype == F32 and mu.dtype == F32 and scales.dtype == F32
    s = torch.clamp(scales, min=SCALE_BOUND).to(dtype)
    a = (q - mu).abs().to(dtype)
    kc = float(-(2 ** -0.5))
    U = 0.5 * torch.erfc(kc * ((0.5 - a) / s))
    L = 0.5 * torch.erfc(kc * ((-0.5 - a) / s))
    lik = torch.clamp(U - L, min=LIK_BOUND)
    return lik, U, L


def bits(lik64):
    return float((-torch.log2(lik64.double())).sum())


def error_model(lik64, U, L):
    """m_i = 2^-24 (|U_i| + |L_i|) + 2^-23 lik_i: the cancellation floor of a float32 difference plus a relative term for the tail"""
    return 2.0 ** -24 * (U.abs() + L.abs()).double() + 2.0 ** -23 * lik64.double()


def k_of(lik, lik64, m):
    """observed error in units of the model, per element"""
    return (lik.double() - lik64.double()).abs() / m


def bucket_masks(lik64):
    l = lik64.double()
    return {"ge1e-3": l >= 1e-3, "1e-6..1e-3": (l >= 1e-6) & (l < 1e-3), "1e-9..1e-6": (l > LIK_BOUND) & (l < 1e-6),
            "clamped": l <= LIK_BOUND}


def scale_indexes(scales, table):
    assert scales.dtype == F32 and table.dtype == F32
    s = torch.clamp(scales, min=SCALE_BOUND)
    idx = torch.full(s.shape, table.numel() - 1, dtype=torch.int32)
    for t in table[:-1]:
        idx -= (s <= t).to(torch.int32)
    return idx


def scale_table(lo=0.11, hi=256.0, levels=64):
    return torch.exp(torch.linspace(np.log(lo), np.log(hi), levels)).to(F32)


def sse_clamp01(pred, cur):
    """float64 sum of the float32 terms d * d, d = fl32(clamp(pred, 0, 1) - cur)"""
    d = torch.clamp(pred, 0.0, 1.0) - cur
    sq = d * d
    assert sq.dtype == F32
    return float(sq.double().sum())


# ------------------------------------------------------------------------------------------------------------------------------
# input generators (seeded; the conditions they promise are asserted in tests/test_entropy_cpu.py)
# ------------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def dyadic(g, shape, span=4.0):
    """multiples of 1/4 in [-span, span]"""
    return _t(g.integers(int(-4 * span), int(4 * span) + 1, size=shape) / 4.0)


def hand_made_eb_table(c, seed):
    """[C,60] table: positive matrices, biases, factors in (-1, 1), dyadic medians"""
    g = _rng(seed)
    p = np.zeros((c, EB_STRIDE), dtype=np.float32)
    k = 0
    for n_mat, n_vec, has_factor in ((3, 3, True), (9, 3, True), (9, 3, True), (9, 3, True), (3, 1, False)):
        p[:, k:k + n_mat] = g.uniform(0.15, 1.6, (c, n_mat)); k += n_mat
        p[:, k:k + n_vec] = g.uniform(-0.5, 0.5, (c, n_vec)); k += n_vec
        if has_factor:
            p[:, k:k + n_vec] = g.uniform(-0.95, 0.95, (c, n_vec)); k += n_vec
    assert k == 58
    p[:, 58] = g.integers(-16, 17, c) / 4.0
    return torch.from_numpy(p)


def medians_of(params):
    return params[:, 58].clone()


def gains(c, seed):
    return _t(_rng(seed).uniform(0.3, 3.0, c))


def eb_inputs(shape, params, seed, in_gain=None, wide=False):
    """z around the medians: |z * gain - median| = 10^U(-0.5, 1.5), or out to 1e4 with ``wide`` (both sigmoids saturate)"""
    g = _rng(seed)
    n, c, h, w = shape
    med = _pc(medians_of(params))
    mag = 10.0 ** g.uniform(-0.5, 4.0 if wide else 1.5, shape)
    d = _t(mag * g.choice([-1.0, 1.0], shape))
    z = d + med
    if in_gain is not None:
        z = z / _pc(in_gain)
    return clear_near_ties(z, [(med, in_gain)])


def gc_inputs(shape, seed, in_gain=None, wide=False):
    """(y, scales, mu).  Plain: scales log-uniform in [0.3, 30], offsets 0.5 .. 6 scale units (every likelihood is well inside (1e-9, 1):
    a launch of one element still has a bit count of order 0.1 or more, which the 1e-5 relative bar on a sum of float32 likelihoods
    needs).  ``wide``: scales log-uniform in [0.05, 300] plus the literal 0, -3, 0.11, 256 and 1e4, offsets 0 .. 40 scale units."""
    g = _rng(seed)
    mu = _t(g.standard_normal(shape) * 2.0)
    if wide:
        s = np.exp(g.uniform(np.log(0.05), np.log(300.0), shape))
        flat = s.reshape(-1)
        lit = np.array([0.0, -3.0, 0.11, 256.0, 1e4])
        flat[: 5 * 64] = np.tile(lit, 64)
        t = np.where(g.random(shape) < 0.5, g.uniform(0.0, 40.0, shape), g.uniform(0.0, 8.0, shape))
    else:
        s = np.exp(g.uniform(np.log(0.3), np.log(30.0), shape))
        t = g.uniform(0.5, 6.0, shape)
    s = _t(s)
    off = _t(t) * torch.clamp(s, min=SCALE_BOUND) * _t(g.choice([-1.0, 1.0], shape))
    y = mu + off
    if in_gain is not None:
        y = y / _pc(in_gain)
    return clear_near_ties(y, [(mu, in_gain)]), s, mu


def exact_ties(centres_dyadic, gain):
    """v with fl32(v * gain) - c = k +- 1/2 exactly, k in -40 .. 40 (gain a power of two, c dyadic: every step is exact).
    centres_dyadic: [1,C,2,81] (full tensor) or [1,C,1,1]; gain: [C] of 1.0 / 2.0.  Returns v [1,C,2,81]."""
    k = torch.arange(-40, 41, dtype=F32).reshape(1, 1, 1, 81)
    half = torch.tensor([0.5, -0.5]).reshape(1, 1, 2, 1)
    v = (centres_dyadic + k + half) / _pc(gain)
    assert bool((tie_distance(v, centres_dyadic, gain) == 0).all())
    return v


def double_rounding_draws(c, per_channel, seed, centre_per_element=False):
    """The contraction probe.  z = fl32((c + k + 1/2) / gain), gain in [0.3, 3], c dyadic, k in -40 .. 40.
    Returns (z [C,D], gain [C], centre [C,1] or [C,D], qualifies [C,D] bool) where ``qualifies`` marks the draws with
      fl32(fl32(z * gain) - c) an exact k + 1/2, the float64 z * gain - c not, and
      rint(fl32(z * gain - c)) -- one rounding: what a fused multiply-add gives -- different from the two-step integer."""
    g = _rng(seed)
    gain = gains(c, seed + 1)
    centre = dyadic(g, (c, per_channel) if centre_per_element else (c, 1))
    k = _t(g.integers(-40, 41, (c, per_channel)))
    z = ((centre.double() + k.double() + 0.5) / gain.double().reshape(-1, 1)).float()
    gcol = gain.reshape(-1, 1)
    two_step = (z * gcol) - centre                                              # float32, two roundings
    exact = z.double() * gcol.double() - centre.double()                        # exact in float64 (48-bit product, dyadic centre)
    assert bool(((exact + centre.double()) == z.double() * gcol.double()).all())
    fused = exact.float()                                                       # one rounding
    tie = ((two_step.double() - torch.floor(two_step.double())) == 0.5) & (exact != two_step.double())
    qualifies = tie & (torch.round(fused) != torch.round(two_step))
    return z, gain, centre, qualifies


def double_rounding_tensor(c, h, w, seed, centre_per_element=False):
    """[1,C,H,W] tensor of probe draws, each channel's qualifying draws first; (z, gain, centre NCHW-broadcastable, qualifies)."""
    z, gain, centre, q = double_rounding_draws(c, 4 * h * w, seed, centre_per_element)
    order = torch.argsort((~q).to(torch.int8), dim=1, stable=True)[:, : h * w]
    pick = lambda a: torch.gather(a, 1, order).reshape(1, c, h, w)
    z, q = pick(z), pick(q)
    centre = pick(centre) if centre_per_element else centre.reshape(1, c, 1, 1)
    # (what is left of the draws -- one or two ulp off a tie -- is moved away; ties stay)
    z2 = clear_near_ties(z, [(centre, gain)])
    assert torch.equal(z2[q], z[q])
    return z2, gain, centre, q


def index_probe_scales(table):
    """every table entry, one float32 ulp either side of it, below the bound, negative, above the top entry, inf"""
    t = table.numpy()
    vals = np.concatenate([t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf)),
                           np.array([0.0, 0.05, 0.1099, -3.0, -0.0, 256.5, 1e4, 3e38, np.inf], dtype=np.float32)])
    return torch.from_numpy(vals.astype(np.float32))
