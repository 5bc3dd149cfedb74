"""-m gpu: the entropy kernels of csrc/entropy.hip against the plain float64 reference of tests/entropy_ref.py.

What is compared, and how exactly:
  * symbols, scale-table indexes and every stored z_hat / y_hat value: bit for bit against the float32 emulation of the quantiser
    (no element is excluded: the generators leave no near-tie, tests/test_entropy_cpu.py asserts it);
  * likelihoods, per element: | lik_gpu - lik64 | <= 4 * K_ref * m_i with m_i = 2^-24 (|U_i| + |L_i|) + 2^-23 lik_i (U, L: the float64
    cumulative values before the subtraction -- the cancellation floor -- plus a relative term for the tail) and
    K_ref = max_i | lik32_i - lik64_i | / m_i measured on the CPU on the reference run in float32 over the range case of that kernel
    (the seeded device_params table: over its own case).  The factor 4 covers device expf / tanhf / erfcf a few ulp off libm and FMA
    contraction inside the MLP; it is never measured against the kernel;
  * bits per launch: 1e-5 relative against the float64 sum (the bar of tests/test_ops_gpu.py);
  * every launch starts from a row of 1e300 partial sums: all 1024 slots must have been rewritten.

K_ref of every case but the seeded table is the range case's of that kernel: the plain inputs of the small shapes and of the gains,
ties and sym_src cases lie inside the families the range cases draw from (a launch of one element has no K_ref of its own).

Measured on an MI355X (K = max_i | lik_i - lik64_i | / m_i per bucket of lik64; range cases, (2, 96, 37, 37) = 262 848 elements):
                                    K_ref    lik >= 1e-3      [1e-6, 1e-3)     (1e-9, 1e-6)     clamped           bits rel err
                                             count   K        count   K        count   K        count    K        kernel   float32 ref
  vc_eb_forward, hand-made table    18.67    11837   9.05     4543   17.62     4623   18.67     241845   0.24     4.25e-8  1.15e-9
  vc_gc_forward                     39.70    63151   8.06    43919   22.20    21698   39.15     134080   0.24     3.70e-8  4.78e-9
  vc_eb_forward, device_params()    44.07   125286   9.66    23213   21.09    12072   36.53     102277   0.24     4.09e-8     -
(K_ref is the float32 reference's own worst K; the bound is 4 * K_ref.)  No kernel K exceeds its K_ref by more than rounding of the figures above; the worst
K of the smaller cases is 34.1 (vc_gc_forward, (3, 20, 9, 11)) and their worst bits error 7.2e-8 against the 1e-5 bar.
vc_sse_clamp01: relative error 0 against the 1e-12 bar.
The compiler does not fuse the quantiser's multiply and subtract today: in the gfx950 code of k_eb_forward, k_gc_forward and
k_refine_symbols the gain's v_mul_f32 sits in a branch of its own (taken when in_gain is given), followed by v_sub_f32 and
v_rndne_f32.  The double-rounding cases stay as the guard.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import entropy_ref as R

pytestmark = pytest.mark.gpu

EINVAL = -1
CANARY = -7777.25
FILL = 6151.5                 # what surrounds an input window: a kernel that reads outside it gets integers nowhere near
SHAPES = [(1, 1, 1, 1), (1, 3, 5, 7), (3, 20, 9, 11), (2, 96, 37, 37)]
RANGE_SHAPE = (2, 96, 37, 37)
LAYOUTS = ["dense", "channels", "images"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------------------------------
# windows: "channels" = channels [8, 8 + c) of a buffer 16 channels wider; "images" = images [1, 1 + n) of n + 2 (and the channel
# window on top); the pair (scales, means) is always the two halves of ONE 2c-channel buffer unless the layout is dense
# ------------------------------------------------------------------------------------------------------------------------------
def _geometry(layout, n, c):
    c_lo, c_pad = (0, 0) if layout == "dense" else (8, 16)
    n_lo, n_pad = (1, 2) if layout == "images" else (0, 0)
    return c_lo, c_pad, n_lo, n_pad


def _place(x, dev, layout, fill=FILL):
    """NCHW CPU tensor -> (wide T, window T holding x)"""
    from vcamd import hip
    n, c, h, w = x.shape
    c_lo, c_pad, n_lo, n_pad = _geometry(layout, n, c)
    wide = torch.full((n + n_pad, c + c_pad, h, w), fill, dtype=torch.float32)
    wide[n_lo:n_lo + n, c_lo:c_lo + c] = x
    t = hip.nchw_to_nhwc(wide.to(dev))
    return t, t.channels(c_lo, c_lo + c).images(n_lo, n_lo + n)


def _place_pair(a, b, dev, layout):
    """(scales, means): the two channel halves of one buffer (the output of the hyper-synthesis transform)"""
    from vcamd import hip
    if layout == "dense":
        return _place(a, dev, layout)[1], _place(b, dev, layout)[1]
    n, c, h, w = a.shape
    n_lo, n_pad = (1, 2) if layout == "images" else (0, 0)
    wide = torch.full((n + n_pad, 2 * c, h, w), FILL, dtype=torch.float32)
    wide[n_lo:n_lo + n, :c] = a
    wide[n_lo:n_lo + n, c:] = b
    t = hip.nchw_to_nhwc(wide.to(dev))
    return t.channels(0, c).images(n_lo, n_lo + n), t.channels(c, 2 * c).images(n_lo, n_lo + n)


def _out_window(shape, dev, layout):
    from vcamd import hip
    n, c, h, w = shape
    c_lo, c_pad, n_lo, n_pad = _geometry(layout, n, c)
    wide = hip.T.empty(n + n_pad, h, w, c + c_pad, dev)
    wide.buf.fill_(CANARY)
    return wide, wide.channels(c_lo, c_lo + c).images(n_lo, n_lo + n)


def _read_window(wide, shape, layout):
    """the window's content (NCHW, CPU) after checking that nothing around it was written"""
    from vcamd import hip
    n, c, h, w = shape
    c_lo, c_pad, n_lo, n_pad = _geometry(layout, n, c)
    full = hip.nhwc_to_nchw(wide).cpu()
    inside = torch.zeros(full.shape, dtype=torch.bool)
    inside[n_lo:n_lo + n, c_lo:c_lo + c] = True
    assert bool((full[~inside] == CANARY).all()), "the kernel wrote outside the output window"
    return full[n_lo:n_lo + n, c_lo:c_lo + c].contiguous()


def _fresh_partial(dev):
    from vcamd import hip
    slots = hip.lib().vc_bits_slots()
    assert slots == 1024
    return torch.full((slots,), 1e300, dtype=torch.float64, device=dev), slots


def _fold(partial, slots, dev):
    from vcamd import hip
    out = torch.empty(1, dtype=torch.float64, device=dev)
    hip.check(hip.lib().vc_bits_reduce(hip.stream(), partial.data_ptr(), slots, 1, out.data_ptr()), "vc_bits_reduce")
    return out


def launch_eb(dev, z, params, in_gain=None, out_gain=None, layout="dense"):
    from vcamd import hip
    L = hip.lib()
    _, zt = _place(z, dev, layout)
    wide, hat = _out_window(z.shape, dev, layout)
    p_d = params.to(dev).contiguous()
    ig, og = (None if g is None else g.to(dev) for g in (in_gain, out_gain))
    sym = torch.full((z.numel(),), -12345, dtype=torch.int32, device=dev)
    lik = torch.full(z.shape, -1.0, dtype=torch.float32, device=dev)
    partial, slots = _fresh_partial(dev)
    hip.check(L.vc_eb_forward(hip.stream(), zt.view(), p_d.data_ptr(), _ptr(ig), _ptr(og), hat.view(), sym.data_ptr(),
                              partial.data_ptr(), slots, lik.data_ptr()), "vc_eb_forward")
    total = _fold(partial, slots, dev)
    torch.cuda.synchronize()
    return SimpleNamespace(sym=sym.cpu().view(z.shape), sym_dev=sym, lik=lik.cpu(), hat=_read_window(wide, z.shape, layout),
                           partial=partial.cpu(), bits=float(total.item()), params_dev=p_d)


def launch_gc(dev, y, s, mu, table, in_gain=None, out_gain=None, layout="dense", sym_src=None):
    from vcamd import hip
    L = hip.lib()
    _, yt = _place(y, dev, layout)
    st, mt = _place_pair(s, mu, dev, layout)
    wide, hat = _out_window(y.shape, dev, layout)
    src = None if sym_src is None else _place(sym_src, dev, layout, fill=-FILL)[1]
    if src is not None:
        assert (src.sn, src.sh, src.sw) == (yt.sn, yt.sh, yt.sw) and src.buf.data_ptr() != yt.buf.data_ptr()
    ig, og = (None if g is None else g.to(dev) for g in (in_gain, out_gain))
    t_d = table.to(dev)
    sym = torch.full((y.numel(),), -12345, dtype=torch.int32, device=dev)
    idx = torch.full((y.numel(),), -12345, dtype=torch.int32, device=dev)
    lik = torch.full(y.shape, -1.0, dtype=torch.float32, device=dev)
    partial, slots = _fresh_partial(dev)
    hip.check(L.vc_gc_forward(hip.stream(), yt.view(), st.view(), mt.view(), _ptr(ig), _ptr(og), hat.view(), partial.data_ptr(), slots,
                              None if src is None else src.ptr, sym.data_ptr(), idx.data_ptr(), t_d.data_ptr(), t_d.numel(),
                              lik.data_ptr()), "vc_gc_forward")
    total = _fold(partial, slots, dev)
    torch.cuda.synchronize()
    return SimpleNamespace(sym=sym.cpu().view(y.shape), sym_dev=sym, idx=idx.cpu().view(y.shape), lik=lik.cpu(),
                           hat=_read_window(wide, y.shape, layout), partial=partial.cpu(), bits=float(total.item()), means_t=mt)


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement's own error (CPU): K_ref per kernel, over the range case
# ------------------------------------------------------------------------------------------------------------------------------
def _k_ref(lik32, lik64, U, L):
    return float(R.k_of(lik32, lik64, R.error_model(lik64, U, L)).max())


@pytest.fixture(scope="module")
def table():
    return R.scale_table()


@pytest.fixture(scope="module")
def eb_range():
    params = R.hand_made_eb_table(96, 3)
    z = R.eb_inputs(RANGE_SHAPE, params, 7, wide=True)
    _, q, _ = R.quantise(z, params[:, 58].reshape(1, -1, 1, 1))
    lik64, U, L = R.eb_likelihood(q, params, R.F64)
    lik32, _, _ = R.eb_likelihood(q, params, R.F32)
    k = _k_ref(lik32, lik64, U, L)
    rb = abs(R.bits(lik32) - R.bits(lik64)) / R.bits(lik64)
    print(f"\n[entropy] EB K_ref = {k:.2f}; restatement bits rel err {rb:.2e}")
    assert k > 0
    return SimpleNamespace(params=params, z=z, k_ref=k)


@pytest.fixture(scope="module")
def gc_range():
    y, s, mu = R.gc_inputs(RANGE_SHAPE, 11, wide=True)
    _, q, _ = R.quantise(y, mu)
    lik64, U, L = R.gc_likelihood(q, mu, s, R.F64)
    lik32, _, _ = R.gc_likelihood(q, mu, s, R.F32)
    k = _k_ref(lik32, lik64, U, L)
    rb = abs(R.bits(lik32) - R.bits(lik64)) / R.bits(lik64)
    print(f"\n[entropy] GC K_ref = {k:.2f}; restatement bits rel err {rb:.2e}")
    assert k > 0
    return SimpleNamespace(y=y, s=s, mu=mu, k_ref=k)


def _check_lik_and_bits(out, lik64, U, L, k_ref, what):
    m = R.error_model(lik64, U, L)
    k = R.k_of(out.lik, lik64, m)
    per_bucket = {name: (int(mask.sum()), float(k[mask].max()) if bool(mask.any()) else 0.0) for name, mask in R.bucket_masks(lik64).items()}
    want_bits = R.bits(lik64)
    rel = abs(out.bits - want_bits) / want_bits
    print(f"[entropy] {what}: K_ref {k_ref:.2f}, kernel K per bucket (count, K) {per_bucket}, bits rel err {rel:.2e}")
    assert bool(torch.isfinite(out.lik).all()) and float(out.lik.min()) >= np.float32(1e-9) * (1 - 1e-6)
    worst = float(k.max())
    assert worst <= 4 * k_ref, f"{what}: likelihood error {worst:.2f} model units > 4 x K_ref = {4 * k_ref:.2f}"
    assert rel <= 1e-5, f"{what}: bits {out.bits!r} against {want_bits!r}: {rel:.3e}"
    # every slot rewritten, the folded total is the slots' sum, a workgroup without elements wrote zero
    p = out.partial
    assert bool((p < 1e299).all()) and bool((p >= 0).all()), f"{what}: {int((p >= 1e299).sum())} stale partial sums"
    blocks = min(1024, (lik64.numel() + 255) // 256)
    assert bool((p[blocks:] == 0).all())
    assert abs(float(p.sum()) - out.bits) <= 1e-12 * max(out.bits, 1.0)


def check_eb(out, z, params, k_ref, what, in_gain=None, out_gain=None):
    med = params[:, 58].reshape(1, -1, 1, 1)
    sym, q, hat = R.quantise(z, med, in_gain, out_gain)
    assert torch.equal(out.sym, sym), f"{what}: {int((out.sym != sym).sum())} symbols differ"
    assert _bits_equal(out.hat, hat), f"{what}: z_hat"
    lik64, U, L = R.eb_likelihood(q, params)
    _check_lik_and_bits(out, lik64, U, L, k_ref, what)


def check_gc(out, y, s, mu, table, k_ref, what, in_gain=None, out_gain=None, sym_src=None):
    sym, q, hat = R.quantise(y, mu, in_gain, out_gain)
    if sym_src is not None:
        sym = R.quantise(sym_src, mu)[0]
    assert torch.equal(out.sym, sym), f"{what}: {int((out.sym != sym).sum())} symbols differ"
    assert _bits_equal(out.hat, hat), f"{what}: y_hat"
    assert torch.equal(out.idx, R.scale_indexes(s, table)), f"{what}: indexes"
    lik64, U, L = R.gc_likelihood(q, mu, s)
    _check_lik_and_bits(out, lik64, U, L, k_ref, what)


def _same(a, b):
    for k in ("sym", "lik", "hat", "partial"):
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x, y) if x.dtype != torch.float32 else _bits_equal(x, y), k
    assert a.bits == b.bits
    if hasattr(a, "idx"):
        assert torch.equal(a.idx, b.idx)


# ------------------------------------------------------------------------------------------------------------------------------
# shapes x layouts
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eb_forward_shapes_and_windows(dev, eb_range, shape):
    """one element, less than a workgroup, a batch, 704 elements past one sweep of the grid -- dense, as a channel window and as an
    image window: the same bits every time"""
    if shape == RANGE_SHAPE:
        params, z = eb_range.params, eb_range.z
    else:
        params = R.hand_made_eb_table(shape[1], 3)
        z = R.eb_inputs(shape, params, 7 + SHAPES.index(shape))
    outs = [launch_eb(dev, z, params, layout=lay) for lay in LAYOUTS]
    check_eb(outs[0], z, params, eb_range.k_ref, f"EB {shape}")
    for o in outs[1:]:
        _same(outs[0], o)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gc_forward_shapes_and_windows(dev, gc_range, table, shape):
    if shape == RANGE_SHAPE:
        y, s, mu = gc_range.y, gc_range.s, gc_range.mu
    else:
        y, s, mu = R.gc_inputs(shape, 11 + SHAPES.index(shape))
    outs = [launch_gc(dev, y, s, mu, table, layout=lay) for lay in LAYOUTS]
    check_gc(outs[0], y, s, mu, table, gc_range.k_ref, f"GC {shape}")
    for o in outs[1:]:
        _same(outs[0], o)


def test_eb_forward_seeded_module_table(dev):
    """a table from EntropyBottleneck.device_params() with seeded weights (K_ref from this table's own float32 run)"""
    from vcamd.layers import EntropyBottleneck
    from vcamd.seeding import seeded_state_dict
    eb = EntropyBottleneck(96)
    eb.load_state_dict(seeded_state_dict(eb.state_dict(), 41))
    params = eb.device_params().cpu()
    z = R.eb_inputs(RANGE_SHAPE, params, 9, wide=True)
    _, q, _ = R.quantise(z, params[:, 58].reshape(1, -1, 1, 1))
    lik64, U, L = R.eb_likelihood(q, params, R.F64)
    k_ref = _k_ref(R.eb_likelihood(q, params, R.F32)[0], lik64, U, L)
    assert k_ref > 0
    check_eb(launch_eb(dev, z, params, layout="channels"), z, params, k_ref, "EB seeded table")


# ------------------------------------------------------------------------------------------------------------------------------
# gains
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_out", [False, True], ids=["out_none", "out_gain"])
@pytest.mark.parametrize("with_in", [False, True], ids=["in_none", "in_gain"])
def test_eb_forward_gains(dev, eb_range, with_in, with_out):
    shape = (3, 20, 9, 11)
    ig = R.gains(20, 50) if with_in else None
    og = R.gains(20, 51) if with_out else None
    params = R.hand_made_eb_table(20, 3)
    z = R.eb_inputs(shape, params, 31, in_gain=ig)
    out = launch_eb(dev, z, params, ig, og, layout="channels")
    check_eb(out, z, params, eb_range.k_ref, f"EB gains in={with_in} out={with_out}", ig, og)


@pytest.mark.parametrize("with_out", [False, True], ids=["out_none", "out_gain"])
@pytest.mark.parametrize("with_in", [False, True], ids=["in_none", "in_gain"])
def test_gc_forward_gains(dev, gc_range, table, with_in, with_out):
    shape = (3, 20, 9, 11)
    ig = R.gains(20, 50) if with_in else None
    og = R.gains(20, 51) if with_out else None
    y, s, mu = R.gc_inputs(shape, 32, in_gain=ig)
    out = launch_gc(dev, y, s, mu, table, ig, og, layout="channels")
    check_gc(out, y, s, mu, table, gc_range.k_ref, f"GC gains in={with_in} out={with_out}", ig, og)


# ------------------------------------------------------------------------------------------------------------------------------
# ties
# ------------------------------------------------------------------------------------------------------------------------------
def _half_even(v, centre, gain):
    d = v.double() * gain.double().reshape(1, -1, 1, 1) - centre.double()
    lo = torch.floor(d).long()
    assert bool((d - lo == 0.5).all())
    return torch.where(lo % 2 == 0, lo, lo + 1).int()


def test_exact_ties_round_half_to_even(dev, eb_range, gc_range, table):
    """v - c = k +- 1/2, k in -40 .. 40, dyadic centres, gains 1 and 2: every step is exact, every symbol is the even neighbour"""
    g = np.random.default_rng(2)
    gain = torch.tensor([1.0, 2.0, 1.0, 2.0])
    params = R.hand_made_eb_table(4, 3)
    med = params[:, 58].reshape(1, -1, 1, 1)
    z = R.exact_ties(med, gain)
    out = launch_eb(dev, z, params, gain, None, layout="channels")
    assert torch.equal(out.sym, _half_even(z, med, gain))
    check_eb(out, z, params, eb_range.k_ref, "EB exact ties", gain)
    mu = R.dyadic(g, (1, 4, 2, 81))
    y = R.exact_ties(mu, gain)
    s = torch.full(y.shape, 7.0)
    out = launch_gc(dev, y, s, mu, table, gain, None, layout="channels")
    assert torch.equal(out.sym, _half_even(y, mu, gain))
    check_gc(out, y, s, mu, table, gc_range.k_ref, "GC exact ties", gain)


def test_double_rounding_ties_take_the_two_step_integer(dev, eb_range, gc_range, table):
    """The contraction probe: fl32(fl32(z * gain) - c) is an exact tie while z * gain - c is not, and a fused multiply-add would round
    to the other integer.  The kernels must round twice like the reference."""
    z, gain, med, q = R.double_rounding_tensor(96, 37, 37, 21)
    assert int(q.sum()) >= 256
    params = R.hand_made_eb_table(96, 3)
    params[:, 58] = med.reshape(-1)
    out = launch_eb(dev, z, params, gain, None)
    want = R.quantise(z, med, gain)[0]
    assert torch.equal(out.sym[q], want[q]), f"EB: {int((out.sym[q] != want[q]).sum())} of {int(q.sum())} double-rounding ties went the fused way"
    check_eb(out, z, params, eb_range.k_ref, "EB double-rounding ties", gain)

    y, gain, mu, q = R.double_rounding_tensor(96, 37, 37, 22, centre_per_element=True)
    assert int(q.sum()) >= 256
    s = torch.full(y.shape, 9.0)
    out = launch_gc(dev, y, s, mu, table, gain, None)
    want = R.quantise(y, mu, gain)[0]
    assert torch.equal(out.sym[q], want[q]), f"GC: {int((out.sym[q] != want[q]).sum())} of {int(q.sum())} double-rounding ties went the fused way"
    check_gc(out, y, s, mu, table, gc_range.k_ref, "GC double-rounding ties", gain)


def test_double_rounding_ties_in_symbol_refinement(dev):
    """vc_refine_z_symbols with in_gain through a 1x1 identity layer (the fp64 recomputation returns z itself).  eps is tiny, so `near`
    holds exactly on the two-step ties: a fused `near` test would miss the probe's elements (their fused distance is not zero), a
    fused final rint(a - m) would give the other integer."""
    from vcamd import hip
    L = hip.lib()
    c, h, w = 32, 24, 32
    z, gain, med, q = R.double_rounding_tensor(c, h, w, 23)
    assert int(q.sum()) >= 256
    out_gain = R.gains(c, 52)
    ties = R.tie_distance(z, med, gain) == 0
    assert bool(ties[q].all()) and int(R.near_ties(z, med, gain).sum()) == 0
    want_sym = R.quantise(z, med, gain)[0]
    params = torch.zeros(c, R.EB_STRIDE)
    params[:, 58] = med.reshape(-1)
    tz = hip.nchw_to_nhwc(z.to(dev))
    eye = torch.eye(c).reshape(c, c, 1, 1).contiguous().to(dev)
    p_d, g_d, og_d = params.to(dev), gain.to(dev), out_gain.to(dev)
    sym = torch.full((z.numel(),), -999, dtype=torch.int32, device=dev)
    wide, hat = _out_window(z.shape, dev, "channels")
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    layer = hip.RefineLayer(tz.view(), eye.data_ptr(), None, 1, 1, 0)
    hip.check(L.vc_refine_z_symbols(hip.stream(), tz.view(), layer, p_d.data_ptr(), g_d.data_ptr(), 1e-30, sym.data_ptr(), hat.view(),
                                    og_d.data_ptr(), counter.data_ptr()), "vc_refine_z_symbols")
    torch.cuda.synchronize()
    got = sym.cpu().view(z.shape)
    assert int(counter.item()) == int(ties.sum()), "the `near` test must see the two-step difference"
    assert torch.equal(got[ties], want_sym[ties]) and bool((got[~ties] == -999).all())
    got_hat = _read_window(wide, z.shape, "channels")
    want_hat = R.dequantise(want_sym, med, out_gain)
    assert _bits_equal(got_hat[ties], want_hat[ties]) and bool((got_hat[~ties] == CANARY).all())


# ------------------------------------------------------------------------------------------------------------------------------
# indexes
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "channels"])
def test_scale_indexes_at_the_table_entries(dev, gc_range, table, layout):
    """scales equal to each of the 64 entries (s <= t is inclusive), one float32 ulp either side, below the bound, negative, above
    the top entry, inf: vc_gc_indexes == the indexes of vc_gc_forward == the reference"""
    from vcamd import hip
    probe = R.index_probe_scales(table)
    assert probe.numel() == 201
    s = probe.reshape(1, 3, 1, 67).contiguous()
    mu = torch.zeros_like(s)
    y = torch.full(s.shape, 0.25)
    want = R.scale_indexes(s, table)
    out = launch_gc(dev, y, s, mu, table, layout=layout)
    st, _ = _place_pair(s, mu, dev, layout)
    t_d = table.to(dev)
    idx = torch.full((s.numel(),), -12345, dtype=torch.int32, device=dev)
    hip.check(hip.lib().vc_gc_indexes(hip.stream(), st.view(), t_d.data_ptr(), t_d.numel(), idx.data_ptr()), "vc_gc_indexes")
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu().view(s.shape), want)
    assert torch.equal(out.idx, want)


# ------------------------------------------------------------------------------------------------------------------------------
# decoder agreement
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_out", [False, True], ids=["out_none", "out_gain"])
def test_dequant_rebuilds_the_encoder_side_tensor(dev, table, with_out):
    from vcamd import hip
    L = hip.lib()
    shape = (3, 20, 9, 11)
    og = R.gains(20, 51) if with_out else None
    og_d = None if og is None else og.to(dev)
    params = R.hand_made_eb_table(20, 3)
    z = R.eb_inputs(shape, params, 41)
    enc = launch_eb(dev, z, params, None, og, layout="channels")
    for layout in ("channels", "images"):
        wide, hat = _out_window(shape, dev, layout)
        hip.check(L.vc_eb_dequant(hip.stream(), enc.sym_dev.data_ptr(), enc.params_dev.data_ptr(), _ptr(og_d), hat.view()), "vc_eb_dequant")
        torch.cuda.synchronize()
        got = _read_window(wide, shape, layout)
        assert _bits_equal(got, enc.hat)
        assert _bits_equal(got, R.dequantise(enc.sym, params[:, 58].reshape(1, -1, 1, 1), og))

    y, s, mu = R.gc_inputs(shape, 42)
    enc = launch_gc(dev, y, s, mu, table, None, og, layout="channels")
    for layout in ("channels", "images"):
        _, mt = _place_pair(s, mu, dev, layout)
        wide, hat = _out_window(shape, dev, layout)
        hip.check(L.vc_gc_dequant(hip.stream(), enc.sym_dev.data_ptr(), mt.view(), _ptr(og_d), hat.view()), "vc_gc_dequant")
        torch.cuda.synchronize()
        got = _read_window(wide, shape, layout)
        assert _bits_equal(got, enc.hat)
        assert _bits_equal(got, R.dequantise(enc.sym, mu, og))


# ------------------------------------------------------------------------------------------------------------------------------
# sym_src
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "channels"], ids=["same_layout", "equal_slices_of_wide_buffers"])
def test_sym_src_codes_the_ungained_latent(dev, gc_range, table, layout):
    """y gained, sym_src the un-gained tensor: symbols = rint(fl32(sym_src - mu)) while y_hat, likelihoods and bits come from y"""
    shape = (3, 20, 9, 11)
    gain, inv = R.gains(20, 50), R.gains(20, 51)
    y_raw, s, mu = R.gc_inputs(shape, 43)
    y_raw = R.clear_near_ties(y_raw, [(mu, None), (mu, gain)])
    y = y_raw * gain.reshape(1, -1, 1, 1)
    assert int(R.near_ties(y, mu).sum()) == 0 and int(R.near_ties(y_raw, mu).sum()) == 0
    assert int((R.quantise(y, mu)[0] != R.quantise(y_raw, mu)[0]).sum()) > 1000
    out = launch_gc(dev, y, s, mu, table, None, inv, layout=layout, sym_src=y_raw)
    check_gc(out, y, s, mu, table, gc_range.k_ref, f"GC sym_src {layout}", None, inv, sym_src=y_raw)


# ------------------------------------------------------------------------------------------------------------------------------
# reductions
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [1, 255, 1024])
def test_bits_reduce_rows(dev, slots):
    from vcamd import hip
    g = np.random.default_rng(slots)
    rows = 5
    part = g.integers(-2 ** 40, 2 ** 40, (rows, slots)).astype(np.float64)      # integer-valued: every order of summation is exact
    want = part.sum(axis=1)
    p_d = torch.from_numpy(part).to(dev)
    out = torch.full((rows + 1,), 1e300, dtype=torch.float64, device=dev)
    hip.check(hip.lib().vc_bits_reduce(hip.stream(), p_d.data_ptr(), slots, rows, out.data_ptr()), "vc_bits_reduce")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:rows], want) and got[rows] == 1e300


def test_sse_clamp01_on_windows(dev):
    from vcamd import hip
    g = np.random.default_rng(61)
    shape = (2, 3, 19, 23)
    pred = torch.from_numpy(g.uniform(-0.5, 1.5, shape).astype(np.float32))
    cur = torch.from_numpy(g.uniform(0.0, 1.0, shape).astype(np.float32))
    assert float(pred.min()) < -0.45 and float(pred.max()) > 1.45
    want = R.sse_clamp01(pred, cur)
    _, pt = _place(pred, dev, "channels")
    _, ct = _place(cur, dev, "images")
    partial, slots = _fresh_partial(dev)
    hip.check(hip.lib().vc_sse_clamp01(hip.stream(), pt.view(), ct.view(), partial.data_ptr(), slots), "vc_sse_clamp01")
    total = _fold(partial, slots, dev)
    torch.cuda.synchronize()
    assert bool((partial.cpu() < 1e299).all())
    rel = abs(float(total.item()) - want) / want
    print(f"[entropy] vc_sse_clamp01 rel err {rel:.2e}")
    assert rel <= 1e-12


# ------------------------------------------------------------------------------------------------------------------------------
# argument checks
# ------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(dev, table):
    from vcamd import hip
    L = hip.lib()
    st = hip.stream()
    t = hip.T.empty(1, 4, 4, 8, dev)
    t.buf.fill_(1.0)
    v = t.view()
    null = hip.NULL_VIEW
    params = R.hand_made_eb_table(8, 3).to(dev)
    t_d = table.to(dev)
    sym = torch.zeros(128, dtype=torch.int32, device=dev)
    part = torch.zeros(2048, dtype=torch.float64, device=dev)
    slots = L.vc_bits_slots()
    pp, sp, tp, n_t = params.data_ptr(), sym.data_ptr(), t_d.data_ptr(), t_d.numel()
    # null tensors / tables
    assert L.vc_eb_forward(st, null, pp, None, None, v, sp, None, 0, None) == EINVAL
    assert L.vc_eb_forward(st, v, None, None, None, v, sp, None, 0, None) == EINVAL
    assert L.vc_eb_dequant(st, None, pp, None, v) == EINVAL
    assert L.vc_eb_dequant(st, sp, None, None, v) == EINVAL
    assert L.vc_eb_dequant(st, sp, pp, None, null) == EINVAL
    for views in ((null, v, v), (v, null, v), (v, v, null)):
        assert L.vc_gc_forward(st, *views, None, None, v, None, 0, None, sp, None, None, 0, None) == EINVAL
    assert L.vc_gc_forward(st, v, v, v, None, None, v, None, 0, None, sp, sp, None, n_t, None) == EINVAL      # indexes, no table
    assert L.vc_gc_forward(st, v, v, v, None, None, v, None, 0, None, sp, sp, tp, 1, None) == EINVAL
    assert L.vc_gc_indexes(st, null, tp, n_t, sp) == EINVAL
    assert L.vc_gc_indexes(st, v, None, n_t, sp) == EINVAL
    assert L.vc_gc_indexes(st, v, tp, n_t, None) == EINVAL
    assert L.vc_gc_dequant(st, None, v, None, v) == EINVAL
    assert L.vc_gc_dequant(st, sp, null, None, v) == EINVAL
    assert L.vc_gc_dequant(st, sp, v, None, null) == EINVAL
    assert L.vc_bits_reduce(st, None, slots, 1, part.data_ptr()) == EINVAL
    assert L.vc_bits_reduce(st, part.data_ptr(), slots, 1, None) == EINVAL
    assert L.vc_bits_reduce(st, part.data_ptr(), 0, 1, part.data_ptr()) == EINVAL
    assert L.vc_sse_clamp01(st, null, v, part.data_ptr(), slots) == EINVAL
    assert L.vc_sse_clamp01(st, v, v, None, slots) == EINVAL
    # a row of partial sums of another size than vc_bits_slots()
    for bad in (slots - 1, slots + 1, 0):
        assert L.vc_eb_forward(st, v, pp, None, None, v, sp, part.data_ptr(), bad, None) == EINVAL
        assert L.vc_gc_forward(st, v, v, v, None, None, v, part.data_ptr(), bad, None, sp, None, None, 0, None) == EINVAL
        assert L.vc_sse_clamp01(st, v, v, part.data_ptr(), bad) == EINVAL
    # sym_src without symbols
    assert L.vc_gc_forward(st, v, v, v, None, None, v, None, 0, t.ptr, None, None, None, 0, None) == EINVAL
    torch.cuda.synchronize()
    assert bool((t.buf == 1.0).all()) and int(sym.abs().sum()) == 0 and float(part.abs().sum()) == 0.0
