"""-m gpu: the checkerboard entropy kernels of csrc/entropy.hip (vc_gc_forward_ckbd / vc_gc_indexes_ckbd / vc_gc_dequant_ckbd)
against a numpy restatement: the full-tensor formulae of k_gc_forward / k_gc_indexes / k_gc_dequant in float32, then the slicing
into the squeezed order include/vc_hip.h documents for these kernels ([n][c][h][w/2]).

Inputs are channel windows of wider tensors, as the model passes them: y = channels [8, 8 + c) of a buffer 16 channels wider,
(scales, means) = the two halves of one 2c-channel buffer, y_hat = a window of a buffer pre-filled with a sentinel.  The latents
are built as y = (k + u + mu) / gain with integers k in [-40, 40] and |u| <= 0.4: no element sits within 0.1 of a rounding
boundary, so neither the float32 rounding of y nor a fused multiply-subtract in the kernel can flip a symbol.  The scales that
feed the index are table entries times 1.05 (5 % from the nearest comparison) or values below the 0.11 bound.

  * symbols and indexes: equal to the restatement, integer for integer; nothing is written behind the squeezed tensors;
  * y_hat: the selected parity within 1 ulp of the float32 restatement (q + mu) * out_gain -- an add and a multiply, nothing to
    fuse, so exact equality is expected; the worst difference is printed.  The other parity and everything around the window keep
    the sentinel bit for bit;
  * bits: the folded bits_partial row against the sum over the parity of -log2 of the `likelihoods` tensor the existing
    vc_gc_forward writes for the same inputs (log2 in float32 as the kernels take it, summed in float64): 1e-9 relative.  The row
    starts as 1e300 in every slot: all 1024 must have been rewritten;
  * vc_gc_dequant_ckbd on the squeezed symbols rebuilds the bits vc_gc_forward_ckbd stored.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL = -1
SENTINEL = -7777.25
FILL = 6151.5
GUARD = 64                      # int32 words behind every squeezed tensor that must keep their fill
SHAPES = [(2, 6, 5, 8), (1, 80, 4, 12), (1, 12, 3, 2), (1, 24, 1, 64)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def table():
    from vcamd.layers import get_scale_table
    return get_scale_table().float().contiguous()


def squeeze(t, parity):
    """the squeezed order of the *_ckbd kernels (include/vc_hip.h): parity 1 = anchors ((row + col) odd)"""
    out = np.empty(t.shape[:3] + (t.shape[3] // 2,), dtype=t.dtype)
    out[:, :, 0::2, :] = t[:, :, 0::2, parity::2]
    out[:, :, 1::2, :] = t[:, :, 1::2, (1 - parity)::2]
    return out


def parity_mask(shape, parity):
    n, c, h, w = shape
    iy, ix = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.broadcast_to(((iy + ix) & 1) == parity, shape)


def make_case(shape, gains, table, seed):
    n, c, h, w = shape
    g = np.random.default_rng(seed)
    f32 = np.float32
    mu = g.uniform(-3, 3, shape).astype(f32)
    k = g.integers(-40, 41, shape)
    u = g.uniform(-0.4, 0.4, shape)
    in_gain = g.uniform(0.5, 2.0, c).astype(f32) if gains else None
    out_gain = g.uniform(0.5, 2.0, c).astype(f32) if gains else None
    y = (k + u + mu.astype(np.float64)) / (in_gain.astype(np.float64).reshape(1, c, 1, 1) if gains else 1.0)
    y = y.astype(f32)
    tab = table.numpy()
    sc = (tab[g.integers(0, tab.size, shape)] * f32(1.05)).astype(f32)
    low = g.random(shape) < 0.25
    sc[low] = g.uniform(-0.05, 0.1, int(low.sum())).astype(f32)
    # ---- the restatement (float32, full tensor) ----
    v = y * in_gain.reshape(1, c, 1, 1) if gains else y
    d = (v - mu).astype(f32)
    assert np.abs(d.astype(np.float64) - np.rint(d)).max() <= 0.41, "the generator left a near-tie"
    q = np.rint(d).astype(f32)
    yq = (q + mu).astype(f32)
    y_hat = (yq * out_gain.reshape(1, c, 1, 1)).astype(f32) if gains else yq
    s = np.maximum(sc, f32(0.11))
    idx = (tab.size - 1 - (s[..., None] <= tab[:-1]).sum(-1)).astype(np.int32)
    return dict(y=y, mu=mu, sc=sc, in_gain=in_gain, out_gain=out_gain, sym=q.astype(np.int32), idx=idx, y_hat=y_hat)


def place(x, dev, c_lo, c_pad):
    from vcamd import hip
    n, c, h, w = x.shape
    wide = torch.full((n, c + c_pad, h, w), FILL, dtype=torch.float32)
    wide[:, c_lo:c_lo + c] = torch.from_numpy(x)
    return hip.nchw_to_nhwc(wide.to(dev)).channels(c_lo, c_lo + c)


def place_pair(a, b, dev):
    from vcamd import hip
    c = a.shape[1]
    t = hip.nchw_to_nhwc(torch.from_numpy(np.concatenate([a, b], axis=1)).to(dev))
    return t.channels(0, c), t.channels(c, 2 * c)


def out_window(shape, dev):
    from vcamd import hip
    n, c, h, w = shape
    wide = hip.T.empty(n, h, w, c + 16, dev)
    wide.buf.fill_(SENTINEL)
    return wide, wide.channels(8, 8 + c)


def squeezed_buffer(shape, dev):
    n, c, h, w = shape
    return torch.full((n * c * h * (w // 2) + GUARD,), -12345, dtype=torch.int32, device=dev)


def read_squeezed(buf, shape):
    n, c, h, w = shape
    host = buf.cpu().numpy()
    assert (host[-GUARD:] == -12345).all(), "the kernel wrote behind the squeezed tensor"
    return host[:-GUARD].reshape(n, c, h, w // 2)


def ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def check_y_hat(wide, shape, parity, want, what):
    from vcamd import hip
    n, c, h, w = shape
    full = hip.nhwc_to_nchw(wide).cpu().numpy()
    sel = np.zeros(full.shape, dtype=bool)
    sel[:, 8:8 + c] = parity_mask(shape, parity)
    assert np.array_equal(full[~sel].view(np.int32), np.full((~sel).sum(), SENTINEL, np.float32).view(np.int32)), \
        f"{what}: a position outside the selected parity was written"
    got = full[:, 8:8 + c][parity_mask(shape, parity)]
    worst = int(ulps(got, want[parity_mask(shape, parity)]).max())
    print(f"{what} {shape} parity {parity}: worst y_hat difference {worst} ulp")
    assert worst <= 1
    return full[:, 8:8 + c]


@pytest.fixture(scope="module")
def cases(table):
    """one restatement per (shape, gains), shared by the tests"""
    return {(shape, gains): make_case(shape, gains, table, seed=100 * i + gains)
            for i, shape in enumerate(SHAPES) for gains in (False, True)}


def launch_forward(dev, case, shape, parity, table_d, want_bits=True, want_y_hat=True):
    from vcamd import hip
    L = hip.lib()
    yt = place(case["y"], dev, 8, 16)
    st, mt = place_pair(case["sc"], case["mu"], dev)
    ig, og = (None if v is None else torch.from_numpy(v).to(dev) for v in (case["in_gain"], case["out_gain"]))
    wide, hat = out_window(shape, dev)
    sym, idx = squeezed_buffer(shape, dev), squeezed_buffer(shape, dev)
    slots = L.vc_bits_slots()
    partial = torch.full((slots,), 1e300, dtype=torch.float64, device=dev)
    hip.check(L.vc_gc_forward_ckbd(hip.stream(), yt.view(), st.view(), mt.view(), None if ig is None else ig.data_ptr(),
                                   None if og is None else og.data_ptr(), hat.view() if want_y_hat else hip.NULL_VIEW, parity,
                                   partial.data_ptr() if want_bits else None, slots, sym.data_ptr(), idx.data_ptr(),
                                   table_d.data_ptr(), table_d.numel()), "vc_gc_forward_ckbd")
    torch.cuda.synchronize()
    return dict(views=(yt, st, mt), gains=(ig, og), wide=wide, sym=sym, idx=idx, partial=partial, slots=slots)


@pytest.mark.parametrize("gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("parity", [1, 0], ids=["anchors", "nonanchors"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_indexes_dequant(dev, table, cases, shape, parity, gains):
    from vcamd import hip
    L = hip.lib()
    case = cases[(shape, gains)]
    table_d = table.to(dev)
    r = launch_forward(dev, case, shape, parity, table_d)
    yt, st, mt = r["views"]
    ig, og = r["gains"]
    # integers
    assert np.array_equal(read_squeezed(r["sym"], shape), squeeze(case["sym"], parity))
    assert np.array_equal(read_squeezed(r["idx"], shape), squeeze(case["idx"], parity))
    # y_hat
    stored = check_y_hat(r["wide"], shape, parity, case["y_hat"], "vc_gc_forward_ckbd")
    # bits against the likelihood tensor of the full-tensor kernel
    n, c, h, w = shape
    lik = torch.empty(shape, dtype=torch.float32, device=dev)
    hip.check(L.vc_gc_forward(hip.stream(), yt.view(), st.view(), mt.view(), None if ig is None else ig.data_ptr(), None,
                              hip.NULL_VIEW, None, 0, None, None, None, None, 0, lik.data_ptr()), "vc_gc_forward")
    mask = torch.from_numpy(parity_mask(shape, parity).copy()).to(dev)
    want = float((-torch.log2(lik)).double()[mask].sum().item())
    want64 = float(-np.log2(lik.cpu().numpy().astype(np.float64))[parity_mask(shape, parity)].sum())
    out = torch.empty(1, dtype=torch.float64, device=dev)
    hip.check(L.vc_bits_reduce(hip.stream(), r["partial"].data_ptr(), r["slots"], 1, out.data_ptr()), "vc_bits_reduce")
    got = float(out.item())
    print(f"bits {shape} parity {parity}: kernel {got:.12e}, likelihood sum {want:.12e} (rel {abs(got - want) / want:.2e}; "
          f"against float64 logarithms {abs(got - want64) / want64:.2e})")
    assert float(r["partial"].max().item()) < 1e299, "a slot of the partial-sum row was not rewritten"
    assert abs(got - want) <= 1e-9 * want
    # the decoder's index kernel
    idx2 = squeezed_buffer(shape, dev)
    hip.check(L.vc_gc_indexes_ckbd(hip.stream(), st.view(), parity, table_d.data_ptr(), table_d.numel(), idx2.data_ptr()),
              "vc_gc_indexes_ckbd")
    assert np.array_equal(read_squeezed(idx2, shape), squeeze(case["idx"], parity))
    # the decoder's de-quantiser rebuilds the stored bits
    wide2, hat2 = out_window(shape, dev)
    hip.check(L.vc_gc_dequant_ckbd(hip.stream(), r["sym"].data_ptr(), mt.view(), None if og is None else og.data_ptr(), parity,
                                   hat2.view()), "vc_gc_dequant_ckbd")
    rebuilt = check_y_hat(wide2, shape, parity, case["y_hat"], "vc_gc_dequant_ckbd")
    assert np.array_equal(rebuilt.view(np.int32), stored.view(np.int32))


def test_optional_outputs_may_be_absent(dev, table, cases):
    """y_hat.p and bits_partial are nullable: the integers do not change, the partial-sum row is not touched"""
    shape = SHAPES[0]
    case = cases[(shape, True)]
    r = launch_forward(dev, case, shape, 1, table.to(dev), want_bits=False, want_y_hat=False)
    assert np.array_equal(read_squeezed(r["sym"], shape), squeeze(case["sym"], 1))
    assert np.array_equal(read_squeezed(r["idx"], shape), squeeze(case["idx"], 1))
    assert bool((r["partial"] == 1e300).all()) and bool((r["wide"].buf == SENTINEL).all())


def test_two_passes_fill_one_tensor(dev, table, cases):
    """anchors then non-anchors into ONE y_hat window: together the full-tensor result, no merge launch"""
    from vcamd import hip
    L = hip.lib()
    shape = SHAPES[1]
    case = cases[(shape, False)]
    table_d = table.to(dev)
    yt = place(case["y"], dev, 8, 16)
    st, mt = place_pair(case["sc"], case["mu"], dev)
    wide, hat = out_window(shape, dev)
    for parity in (1, 0):
        sym, idx = squeezed_buffer(shape, dev), squeezed_buffer(shape, dev)
        hip.check(L.vc_gc_forward_ckbd(hip.stream(), yt.view(), st.view(), mt.view(), None, None, hat.view(), parity, None, 0,
                                       sym.data_ptr(), idx.data_ptr(), table_d.data_ptr(), table_d.numel()), "vc_gc_forward_ckbd")
    got = hip.nhwc_to_nchw(hat).cpu().numpy()
    assert np.array_equal(got.view(np.int32), case["y_hat"].view(np.int32))


def test_bad_arguments_are_refused(dev, table):
    from vcamd import hip
    L = hip.lib()
    table_d = table.to(dev)
    n, c, h, w = 1, 4, 3, 6
    buf = hip.T.empty(n, h, w, c, dev)
    buf.buf.fill_(1.25)
    ints = torch.zeros(n * c * h * w, dtype=torch.int32, device=dev)
    part = torch.zeros(L.vc_bits_slots(), dtype=torch.float64, device=dev)
    v, null = buf.view(), hip.NULL_VIEW
    odd = hip.View(buf.ptr, n, h, w - 1, c, buf.sn, buf.sh, buf.sw)
    other = hip.View(buf.ptr, n, h - 1, w, c, buf.sn, buf.sh, buf.sw)
    S, t, nt, ip = hip.stream(), table_d.data_ptr(), table_d.numel(), ints.data_ptr()

    def fwd(y=v, sc=v, mu=v, hat=null, parity=1, partial=None, slots=0, sym=ip, idx=ip, tab=t, ntab=nt):
        return L.vc_gc_forward_ckbd(S, y, sc, mu, None, None, hat, parity, partial, slots, sym, idx, tab, ntab)

    assert fwd() == 0
    assert fwd(y=odd, sc=odd, mu=odd) == EINVAL                                    # odd width
    for kw in (dict(y=null), dict(sc=null), dict(mu=null), dict(sym=None), dict(idx=None), dict(tab=None), dict(ntab=1),
               dict(parity=2), dict(parity=-1), dict(mu=other), dict(sc=other), dict(hat=other),
               dict(partial=part.data_ptr(), slots=L.vc_bits_slots() - 1)):
        assert fwd(**kw) == EINVAL, kw
    assert L.vc_gc_indexes_ckbd(S, v, 0, t, nt, ip) == 0
    assert L.vc_gc_indexes_ckbd(S, odd, 0, t, nt, ip) == EINVAL
    for args in ((null, 0, t, nt, ip), (v, 0, None, nt, ip), (v, 0, t, nt, None), (v, 0, t, 1, ip), (v, 2, t, nt, ip)):
        assert L.vc_gc_indexes_ckbd(S, *args) == EINVAL, args
    assert L.vc_gc_dequant_ckbd(S, ip, v, None, 0, v) == 0
    assert L.vc_gc_dequant_ckbd(S, ip, odd, None, 0, odd) == EINVAL
    for args in ((None, v, None, 0, v), (ip, null, None, 0, v), (ip, v, None, 0, null), (ip, other, None, 0, v), (ip, v, None, 3, v)):
        assert L.vc_gc_dequant_ckbd(S, *args) == EINVAL, args
    torch.cuda.synchronize()
