"""-m gpu: the per-pixel kernels of csrc/ew_kernels.hip (blends, motion split, attention gate, quantise-and-mask, channel scale, clamp,
half copies, layouts, SPyNet pre-processing) and the split records of vc_split3 / vc_split3_pad against the float64 references of
tests/ew_ref.py (pinned on the CPU by tests/test_ew_cpu.py): every argument dense, as a channel slice and crop, and at an unaligned
element offset; the row map of csrc/ew_rowmap.h with several workgroups a row, in the row loop (one representative) and in the linear
fallback; the edges of each operation's arithmetic; the argument contract.  Every output is a window of a buffer filled with a
sentinel (or lies between guard values): everything outside must keep its bits.

Bounds (derived in tests/ew_ref.py, u = 2^-24, M the magnitude of the terms in float64): |out - ref| <= 8 u M for vc_lhbdc_blend,
vc_flex_motion_split, vc_spynet_preprocess; <= 16 u M for vc_flex_blend, vc_attention_gate; everything else bit for bit the fp32 /
fp16 torch expression on the CPU, every sentinel and every return code exact.

Largest |out - ref| / (u M) seen on the MI355X, per entry point (printed at teardown):
  vc_attention_gate 2.19 of 16, vc_blend 1.89 of 8, vc_flex_blend 3.31 of 16, vc_flex_motion_split 1.77 of 8, vc_lhbdc_blend 1.94 of 8,
  vc_spynet_preprocess 1.24 of 8."""
import pytest
import torch

import ew_ref as er

pytestmark = pytest.mark.gpu
MAXIMA = {}
EINVAL = -1
GUARD = 0x7b7b          # int16 pattern around half / split outputs
PAD = 16                # guard elements in front of and behind a dense output


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda:0")
    for k in sorted(MAXIMA):
        print(f"\nlargest |out - ref| / (u M) seen, {k}: {MAXIMA[k]:.2f} of {er.BOUND[k]:.0f}", end="")


def _api():
    from vcamd import hip
    return hip, hip.lib(), hip.stream()


def _ok(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def _out(shape, dev, spec):
    """an output window inside a buffer that holds the sentinel everywhere, the window included"""
    return er.place(torch.full(shape, er.SENTINEL), dev, fill=er.SENTINEL, **spec)


def _null(n=0, h=0, w=0, c=0):
    from vcamd import hip
    return hip.View(None, n, h, w, c, 0, 0, 0)


def _v(t, **over):
    v = t.view()
    for k, val in over.items():
        setattr(v, k, val)
    return v


def _same_bits(a, b):
    return torch.equal(er.bits(a.float()), er.bits(b.float()))


def _finish(entry, what, t_out, ref, mag=None):
    """the window against its reference -- within BOUND[entry] u M, or bit for bit without a magnitude --, the rest untouched"""
    win, outside = er.read_window(t_out)
    er.assert_untouched(outside)
    if mag is None:
        bad = (er.bits(win) != er.bits(ref.float())).sum().item()
        assert bad == 0, f"{entry} {what}: {bad} values differ in their bits from the fp32 expression"
        return win
    q = er.units(win, ref, mag)
    MAXIMA[entry] = max(MAXIMA.get(entry, 0.0), q)
    print(f"{entry} {what}: {q:.2f} u M")
    assert q <= er.BOUND[entry], f"{entry} {what}: {q:.2f} u M > {er.BOUND[entry]}"
    return win


def _untouched(*ts):
    torch.cuda.synchronize()
    for t in ts:
        er.assert_untouched((t.buf if hasattr(t, "buf") else t).cpu().view(-1).view(torch.float32))


def _refused(outs, calls):
    """every call returns VC_EINVAL and none of the output buffers changes a bit"""
    for what, rc in calls:
        assert rc == EINVAL, f"{what}: returned {rc}, not VC_EINVAL"
    _untouched(*outs)


def _empty_ok(outs, calls):
    """zero-sized views: VC_OK and nothing written"""
    for what, rc in calls:
        assert rc == 0, f"{what}: returned {rc}, not VC_OK"
    _untouched(*outs)


def _guarded(count, dev, dtype, skew=0):
    """a dense output of `count` elements between guard elements -> (buffer, pointer of the output, check).  skew: elements the
    output starts behind the 16-byte aligned position"""
    buf = torch.empty(count + 2 * PAD + skew, dtype=dtype, device=dev)
    raw = buf.view(torch.int16)
    raw.fill_(GUARD)
    per = buf.element_size() // 2

    def check():
        got = raw.cpu()
        lo, hi = (PAD + skew) * per, (PAD + skew + count) * per
        assert bool((got[:lo] == GUARD).all()) and bool((got[hi:] == GUARD).all()), "guard elements around the output were written"
        return buf[PAD + skew:PAD + skew + count].cpu()
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + (PAD + skew) * buf.element_size(), check


SHAPE_VIEWS = [(h, w, vs) for h, w in er.SHAPES for vs in er.VIEWSETS]
_sv = pytest.mark.parametrize("h,w,viewset", SHAPE_VIEWS, ids=[f"{h}x{w}-{vs}" for h, w, vs in SHAPE_VIEWS])
_rowmap = lambda entry: pytest.mark.parametrize("case", [c for c in er.ROWMAP_CASES + [er.ROWLOOP] if c.entry == entry], ids=lambda c: c.id)  # noqa: E731
ROW_SPECS = [er.DENSE, er.DENSE, er.DENSE, dict(cpad=1), dict(cpad=1), er.DENSE]       # row-map cases: dense inputs, no dense output


def _regime(case):
    m = er.rowmap(case.n, case.h, case.w, case.per_px)
    assert (m is None) == (case.regime == "fallback") and (m is None or m.loops == (case.regime == "loop")) and (case.regime != "wide" or m.bx > 1)


# ------------------------------------------------------------------------------------------------
# blends
# ------------------------------------------------------------------------------------------------
def _blend_fn(L, entry):
    """vc_blend is the operator spelling of vc_lhbdc_blend (csrc/abi_aliases.cpp): the same prototype"""
    f = getattr(L, entry)
    f.argtypes, f.restype = L.vc_lhbdc_blend.argtypes, L.vc_lhbdc_blend.restype
    return f


def _lhbdc(dev, n, h, w, specs, edge=False, resid=True, cur=True, entry="vc_lhbdc_blend"):
    hip, L, s = _api()
    fw, bw, m, c = er.lhbdc_inputs(n, h, w, edge)
    rp, rr_, mp, mr = er.lhbdc_blend(fw, bw, m, c)
    tf, tm, tc = er.place(torch.cat((fw, bw), 1), dev, **specs[0]), er.place(m, dev, seed=1, **specs[1]), er.place(c, dev, seed=2, **specs[2])
    tp, tr = _out((n, 3, h, w), dev, specs[3]), _out((n, 3, h, w), dev, specs[4])
    _ok(_blend_fn(L, entry)(s, tf.view(), tm.view(), tc.view() if cur else _null(), tp.view(), tr.view() if resid else _null()), entry)
    what = f"{n}x{h}x{w} edge={edge} resid={resid}"
    _finish(entry, "pred " + what, tp, rp, mp)
    if not resid:
        return _untouched(tr)
    got = _finish(entry, "resid " + what, tr, rr_, mr)
    if edge:                  # cur == fw == bw in the last image: a mask of exactly 0 or 1 gives the frame itself and a residual of 0
        sure = ((m[n - 1] == 0) | (m[n - 1] == 1)).expand(3, -1, -1)
        assert bool(sure.any()) and not bool(got[n - 1][sure].any())


@_sv
@pytest.mark.parametrize("entry", ["vc_lhbdc_blend", "vc_blend"])
def test_lhbdc_blend_views(dev, entry, h, w, viewset):
    """vc_lhbdc_blend and its alias vc_blend: fwbw, mask, cur, pred, resid each dense, a channel slice and crop, at an unaligned
    offset; with resid, without it (cur given and absent)"""
    specs = er.specs_of(viewset, 5)
    _lhbdc(dev, er.N, h, w, specs, entry=entry)
    if entry == "vc_lhbdc_blend":
        _lhbdc(dev, er.N, h, w, specs, resid=False)
        _lhbdc(dev, er.N, h, w, specs, resid=False, cur=False)


@pytest.mark.parametrize("entry", ["vc_lhbdc_blend", "vc_blend"])
@pytest.mark.parametrize("h,w", er.SIZES)
def test_lhbdc_blend_edges(dev, entry, h, w):
    """vc_lhbdc_blend / vc_blend: a mask of exactly 0, exactly 1 and 2^-24, frames of mixed sign, cur == pred"""
    _lhbdc(dev, er.N, h, w, er.specs_of("rot1", 5), edge=True, entry=entry)


@_rowmap("vc_lhbdc_blend")
def test_lhbdc_blend_row_map(dev, case):
    _regime(case)
    _lhbdc(dev, case.n, case.h, case.w, ROW_SPECS)


def _flex(dev, n, h, w, specs, edge=False, resid=True):
    hip, L, s = _api()
    xb, xa, mask, c = er.flex_inputs(n, h, w, edge)
    rp, rr_, mp, mr = er.flex_blend(xb, xa, mask, c)
    tb, ta = er.place(xb, dev, **specs[0]), er.place(xa, dev, seed=1, **specs[1])
    tm, tc = er.place(mask, dev, seed=2, **specs[2]), er.place(c, dev, seed=3, **specs[5])
    tp, tr = _out((n, 3, h, w), dev, specs[3]), _out((n, 3, h, w), dev, specs[4])
    _ok(L.vc_flex_blend(s, tb.view(), ta.view(), tm.view(), tc.view(), tp.view(), tr.view() if resid else _null()), "vc_flex_blend")
    what = f"{n}x{h}x{w} edge={edge} resid={resid}"
    got = _finish("vc_flex_blend", "pred " + what, tp, rp, mp)
    if edge:                                         # both masks 0: the denominator is the constant alone and the result 0
        both0 = (mask == 0).all(1, keepdim=True).expand(-1, 3, -1, -1)
        assert bool(both0.any()) and not bool(got[both0].any())
    if resid:
        _finish("vc_flex_blend", "resid " + what, tr, rr_, mr)
    else:
        _untouched(tr)


@_sv
def test_flex_blend_views(dev, h, w, viewset):
    """vc_flex_blend: xb, xa, mask, cur, pred, resid in every kind of view; with and without resid"""
    specs = er.specs_of(viewset, 6)
    _flex(dev, er.N, h, w, specs)
    _flex(dev, er.N, h, w, specs, resid=False)


@pytest.mark.parametrize("h,w", er.SIZES)
def test_flex_blend_edges(dev, h, w):
    """vc_flex_blend: both masks 0, one 0 and the other 1, masks of 1e-7, masks one ulp apart"""
    _flex(dev, er.N, h, w, er.specs_of("rot2", 6), edge=True)


@_rowmap("vc_flex_blend")
def test_flex_blend_row_map(dev, case):
    _regime(case)
    _flex(dev, case.n, case.h, case.w, ROW_SPECS)


def test_blend_contract(dev):
    """vc_lhbdc_blend, vc_blend, vc_flex_blend: null pointers, pred.c != 3, fwbw.c < 6, mask.c < 2, resid without cur, every view of
    another image count, lower or narrower than pred (cur also where no resid is asked for), cur.c < 3; empty views"""
    hip, L, s = _api()
    n, h, w = 2, 5, 7
    fw, bw, m, c = er.lhbdc_inputs(n, h, w)
    tf, tm, tc = er.place(torch.cat((fw, bw), 1), dev), er.place(m, dev), er.place(c, dev)
    tp, tr = _out((n, 3, h, w), dev, {}), _out((n, 3, h, w), dev, {})
    p4 = _out((n, 4, h, w), dev, {})
    small = [("another image count", dict(n=1)), ("more images", dict(n=3)), ("lower", dict(h=4)), ("narrower", dict(w=6))]
    for name in ("vc_lhbdc_blend", "vc_blend"):
        f = _blend_fn(L, name)
        V = dict(fwbw=tf.view(), mask=tm.view(), cur=tc.view(), pred=tp.view(), resid=tr.view())
        call = lambda **o: f(s, *[o.get(k, V[k]) for k in ("fwbw", "mask", "cur", "pred", "resid")])  # noqa: E731
        calls = [("null fwbw", call(fwbw=_null(n, h, w, 6))), ("null mask", call(mask=_null(n, h, w, 1))), ("null pred", call(pred=_null(n, h, w, 3))),
                 ("fwbw of 5 channels", call(fwbw=_v(tf, c=5))), ("pred of 2 channels", call(pred=_v(tp, c=2))), ("pred of 4 channels", call(pred=p4.view())),
                 ("resid without cur", call(cur=_null(n, h, w, 3))), ("cur of 2 channels", call(cur=_v(tc, c=2))), ("resid of 2 channels", call(resid=_v(tr, c=2))),
                 ("mask without a channel", call(mask=_v(tm, c=0)))]
        for what, over in small:
            calls += [(f"{k} {what}", call(**{k: _v(t, **over)})) for k, t in (("fwbw", tf), ("mask", tm), ("cur", tc), ("resid", tr))]
            calls.append((f"cur {what}, no resid", call(cur=_v(tc, **over), resid=_null())))
        _refused([tp, tr, p4], calls)
        _empty_ok([tp, tr], [("no row", call(pred=_v(tp, h=0))), ("no column", call(pred=_v(tp, w=0))),
                             ("no image", f(s, _v(tf, n=0), _v(tm, n=0), _v(tc, n=0), _v(tp, n=0), _v(tr, n=0)))])
    xb, xa, mask, c = er.flex_inputs(n, h, w)
    tb, ta, tk = er.place(xb, dev), er.place(xa, dev), er.place(mask, dev)
    V = dict(xb=tb.view(), xa=ta.view(), mask=tk.view(), cur=tc.view(), pred=tp.view(), resid=tr.view())
    call = lambda **o: L.vc_flex_blend(s, *[o.get(k, V[k]) for k in ("xb", "xa", "mask", "cur", "pred", "resid")])  # noqa: E731
    calls = [("null xb", call(xb=_null(n, h, w, 3))), ("null xa", call(xa=_null(n, h, w, 3))), ("null mask", call(mask=_null(n, h, w, 2))),
             ("null pred", call(pred=_null(n, h, w, 3))), ("mask of 1 channel", call(mask=_v(tk, c=1))), ("pred of 2 channels", call(pred=_v(tp, c=2))),
             ("pred of 4 channels", call(pred=p4.view())), ("resid without cur", call(cur=_null(n, h, w, 3))), ("cur of 2 channels", call(cur=_v(tc, c=2))),
             ("xb of 2 channels", call(xb=_v(tb, c=2))), ("xa of 2 channels", call(xa=_v(ta, c=2))), ("resid of 2 channels", call(resid=_v(tr, c=2)))]
    for what, over in small:
        calls += [(f"{k} {what}", call(**{k: _v(t, **over)})) for k, t in (("xb", tb), ("xa", ta), ("mask", tk), ("cur", tc), ("resid", tr))]
        calls.append((f"cur {what}, no resid", call(cur=_v(tc, **over), resid=_null())))
    _refused([tp, tr, p4], calls)
    _empty_ok([tp, tr], [("no row", call(pred=_v(tp, h=0))), ("no column", call(pred=_v(tp, w=0)))])


def test_blends_read_the_top_left_of_larger_inputs(dev):
    """a larger fwbw / mask / cur / xb / xa stays allowed, as vc_axpby allows it"""
    hip, L, s = _api()
    n, h, w = 2, 5, 7
    assert er.BLEND_LARGER == (n, h + 2, w + 3)
    fw, bw, m, c = er.lhbdc_inputs(*er.BLEND_LARGER)
    tf, tm, tc = er.place(torch.cat((fw, bw, fw), 1), dev), er.place(torch.cat((m, m + 1), 1), dev), er.place(torch.cat((c, c), 1), dev)
    tp, tr = _out((n, 3, h, w), dev, er.WIN_U), _out((n, 3, h, w), dev, er.WIN_A)
    _ok(L.vc_lhbdc_blend(s, tf.view(), tm.view(), tc.view(), tp.view(), tr.view()), "vc_lhbdc_blend")
    rp, rr_, mp, mr = er.lhbdc_blend(fw[:, :, :h, :w], bw[:, :, :h, :w], m[:, :, :h, :w], c[:, :, :h, :w])
    _finish("vc_lhbdc_blend", "larger inputs, pred", tp, rp, mp)
    _finish("vc_lhbdc_blend", "larger inputs, resid", tr, rr_, mr)


# ------------------------------------------------------------------------------------------------
# motion split
# ------------------------------------------------------------------------------------------------
@_sv
def test_motion_split_views(dev, h, w, viewset):
    """vc_flex_motion_split: t = 0.5 (the model's), 0, 1 and 0.3; flow4 (the first 4 of 6 channels), ft0, ft1 in every kind of view"""
    hip, L, s = _api()
    f = er.motion_inputs(er.N, h, w, 6)
    specs = er.specs_of(viewset, 3)
    tf = er.place(f, dev, **specs[0])
    for t in er.MOTION_T:
        r0, r1, m0, m1 = er.motion_split(f, t)
        t0, t1 = _out((er.N, 2, h, w), dev, specs[1]), _out((er.N, 2, h, w), dev, specs[2])
        _ok(L.vc_flex_motion_split(s, tf.view(), t0.view(), t1.view(), t), "vc_flex_motion_split")
        _finish("vc_flex_motion_split", f"ft0 t={t}", t0, r0, m0)
        _finish("vc_flex_motion_split", f"ft1 t={t}", t1, r1, m1)


def test_motion_split_contract(dev):
    """vc_flex_motion_split: null pointers, f4.c < 4, ft0.c / ft1.c < 2, an ft of another image count, lower or narrower; empty views"""
    hip, L, s = _api()
    n, h, w = 2, 5, 7
    tf = er.place(er.motion_inputs(n, h, w), dev)
    t0, t1 = _out((n, 2, h, w), dev, {}), _out((n, 2, h, w), dev, {})
    ms = L.vc_flex_motion_split
    calls = [("null flow", ms(s, _null(n, h, w, 4), t0.view(), t1.view(), 0.5)), ("null ft0", ms(s, tf.view(), _null(n, h, w, 2), t1.view(), 0.5)),
             ("null ft1", ms(s, tf.view(), t0.view(), _null(n, h, w, 2), 0.5)), ("flow of 3 channels", ms(s, _v(tf, c=3), t0.view(), t1.view(), 0.5)),
             ("ft0 of 1 channel", ms(s, tf.view(), _v(t0, c=1), t1.view(), 0.5)), ("ft1 of 1 channel", ms(s, tf.view(), t0.view(), _v(t1, c=1), 0.5))]
    for what, over in (("another image count", dict(n=1)), ("more images", dict(n=3)), ("lower", dict(h=4)), ("narrower", dict(w=6))):
        calls += [(f"ft0 {what}", ms(s, tf.view(), _v(t0, **over), t1.view(), 0.5)), (f"ft1 {what}", ms(s, tf.view(), t0.view(), _v(t1, **over), 0.5))]
    _refused([t0, t1], calls)
    _empty_ok([t0, t1], [("no row", ms(s, _v(tf, h=0), t0.view(), t1.view(), 0.5)), ("no column", ms(s, _v(tf, w=0), t0.view(), t1.view(), 0.5)),
                         ("no image", ms(s, _v(tf, n=0), _v(t0, n=0), _v(t1, n=0), 0.5))])


# ------------------------------------------------------------------------------------------------
# attention gate
# ------------------------------------------------------------------------------------------------
def _gate(dev, n, c, h, w, specs, edge=False):
    hip, L, s = _api()
    a, b, identity = er.gate_inputs(n, c, h, w, edge)
    ref, mag = er.attention_gate(a, b, identity)
    ta, tb, ti = er.place(a, dev, **specs[0]), er.place(b, dev, seed=1, **specs[1]), er.place(identity, dev, seed=2, **specs[2])
    to = _out((n, c, h, w), dev, specs[3])
    _ok(L.vc_attention_gate(s, ta.view(), tb.view(), ti.view(), to.view()), "vc_attention_gate")
    got = _finish("vc_attention_gate", f"{n}x{c}x{h}x{w} edge={edge}", to, ref, mag)
    if edge:                                       # a == 0 in the first image, and wherever the gate underflows: the identity alone
        assert _same_bits(got[0], identity[0]) and _same_bits(got[b == -104.0], identity[b == -104.0])


@_sv
def test_attention_gate_views(dev, h, w, viewset):
    """vc_attention_gate: a, b, identity, out in every kind of view"""
    _gate(dev, er.N, 5, h, w, er.specs_of(viewset, 4))


@pytest.mark.parametrize("h,w", er.SIZES)
def test_attention_gate_edges(dev, h, w):
    """vc_attention_gate: b = 0, +-1e-4, +-20, +-88, +-104 (the gate underflows at -104), a = 0"""
    _gate(dev, er.N, 5, h, w, er.specs_of("rot1", 4), edge=True)


@_rowmap("vc_attention_gate")
def test_attention_gate_row_map(dev, case):
    _regime(case)
    _gate(dev, case.n, case.c, case.h, case.w, ROW_SPECS[:3] + [dict(cpad=1)])


def test_attention_gate_contract(dev):
    """vc_attention_gate: null pointers, an input of another n / h / w or with fewer channels than out; empty views"""
    hip, L, s = _api()
    n, c, h, w = 2, 4, 5, 7
    a, b, identity = er.gate_inputs(n, c, h, w)
    ts = [er.place(a, dev), er.place(b, dev), er.place(identity, dev)]
    to = _out((n, c, h, w), dev, {})
    ag = L.vc_attention_gate
    base = [t.view() for t in ts]
    calls = [("null out", ag(s, *base, _null(n, h, w, c)))]
    for i, name in enumerate(("a", "b", "identity")):
        for what, v in [("null", _null(n, h, w, c))] + [(k, _v(ts[i], **o)) for k, o in (("n", dict(n=1)), ("lower", dict(h=4)), ("higher", dict(h=6)),
                                                                                         ("narrower", dict(w=6)), ("wider", dict(w=8)), ("fewer channels", dict(c=3)))]:
            calls.append((f"{name} {what}", ag(s, *[v if j == i else base[j] for j in range(3)], to.view())))
    _refused([to], calls)
    _empty_ok([to], [("no row", ag(s, *[_v(t, h=0) for t in ts], _v(to, h=0))), ("no channel", ag(s, *base, _v(to, c=0)))])


# ------------------------------------------------------------------------------------------------
# quantise-and-mask
# ------------------------------------------------------------------------------------------------
MODES = [(p, r, g) for p in (-1, 0, 1) for r in (0, 1) for g in (False, True)]


def _quant(dev, n, c, h, w, specs, edge=False, modes=MODES, c_in=None):
    hip, L, s = _api()
    x, gain = er.quant_inputs(n, c_in or c, h, w, edge)
    gd = gain.to(dev)
    ti = er.place(x, dev, **specs[0])
    for parity, do_round, with_gain in modes:
        ref = er.F32.quantize_mask(x, gain if with_gain else None, parity, do_round)[:, :c]
        what = f"{n}x{c}x{h}x{w} parity={parity} round={do_round} gain={with_gain}"
        to = _out((n, c, h, w), dev, specs[1])
        _ok(L.vc_quantize_mask(s, ti.view(), to.view(), gd.data_ptr() if with_gain else None, parity, do_round), "vc_quantize_mask")
        got = _finish("vc_quantize_mask", what, to, ref)
        # (an integer-valued float times an fp32 gain is exact in float64: rounded once it is the IEEE product)
        assert _same_bits(got, er.quantize_mask(x, gain if with_gain else None, parity, do_round)[:, :c])
        if c_in is None:                                        # in place: `in` aliases `out`
            tio = er.place(x, dev, fill=er.SENTINEL, **specs[1])
            _ok(L.vc_quantize_mask(s, tio.view(), tio.view(), gd.data_ptr() if with_gain else None, parity, do_round), "vc_quantize_mask")
            _finish("vc_quantize_mask", what + " in place", tio, ref)


@_sv
def test_quantize_mask_views(dev, h, w, viewset):
    """vc_quantize_mask: keep_parity -1 / 0 / 1 x do_round 0 / 1 x gain absent / present, in and out in every kind of view, in place;
    odd h and w: the parity of the last row and column"""
    _quant(dev, er.N, 5, h, w, er.specs_of(viewset, 2))


@pytest.mark.parametrize("h,w", er.SIZES)
def test_quantize_mask_edges(dev, h, w):
    """vc_quantize_mask: exact ties +-0.5, +-1.5, +-2.5, 2^23 + 1, -0.0, the gain applied after the rounding; an input with more
    channels than the output"""
    _quant(dev, er.N, 5, h, w, er.specs_of("rot2", 2), edge=True)
    _quant(dev, er.N, 5, h, w, er.specs_of("rot1", 2), edge=True, c_in=7)


@_rowmap("vc_quantize_mask")
def test_quantize_mask_row_map(dev, case):
    _regime(case)
    _quant(dev, case.n, case.c, case.h, case.w, [er.DENSE, dict(cpad=1)], modes=[(1, 1, True), (0, 1, False)])


def test_quantize_mask_contract(dev):
    """vc_quantize_mask: null pointers, keep_parity outside -1 .. 1, a size mismatch, fewer input channels; empty views"""
    hip, L, s = _api()
    n, c, h, w = 2, 4, 5, 7
    x, gain = er.quant_inputs(n, c, h, w)
    ti, to = er.place(x, dev), _out((n, c, h, w), dev, {})
    qm = L.vc_quantize_mask
    calls = [("null in", qm(s, _null(n, h, w, c), to.view(), None, -1, 1)), ("null out", qm(s, ti.view(), _null(n, h, w, c), None, -1, 1)),
             ("keep_parity -2", qm(s, ti.view(), to.view(), None, -2, 1)), ("keep_parity 2", qm(s, ti.view(), to.view(), None, 2, 1))]
    for what, over in (("n", dict(n=1)), ("lower", dict(h=4)), ("higher", dict(h=6)), ("narrower", dict(w=6)), ("wider", dict(w=8)), ("fewer channels", dict(c=3))):
        calls.append((f"in {what}", qm(s, _v(ti, **over), to.view(), None, -1, 1)))
    _refused([to], calls)
    _empty_ok([to], [("no row", qm(s, _v(ti, h=0), _v(to, h=0), None, 0, 1)), ("no channel", qm(s, ti.view(), _v(to, c=0), None, 0, 1))])


# ------------------------------------------------------------------------------------------------
# channel scale, clamp
# ------------------------------------------------------------------------------------------------
def _scale(dev, n, c, h, w, specs, larger=False):
    hip, L, s = _api()
    x, gain = er.quant_inputs(n, c + 2 * larger, h + larger, w + 2 * larger)
    gd = gain.to(dev)
    ti, to = er.place(x, dev, **specs[0]), _out((n, c, h, w), dev, specs[1])
    _ok(L.vc_channel_scale(s, ti.view(), gd.data_ptr(), to.view()), "vc_channel_scale")
    got = _finish("vc_channel_scale", f"{n}x{c}x{h}x{w}", to, er.F32.channel_scale(x, gain)[:, :c, :h, :w])
    assert torch.equal(got.double(), er.channel_scale(x, gain)[:, :c, :h, :w].float().double())      # one IEEE product: the float64 product rounded once


@_sv
def test_channel_scale_views(dev, h, w, viewset):
    """vc_channel_scale: one IEEE product per value, bit for bit; a and out in every kind of view; the top-left of a larger input
    with more channels"""
    _scale(dev, er.N, 5, h, w, er.specs_of(viewset, 2))
    _scale(dev, er.N, 5, h, w, er.specs_of(viewset, 2), larger=True)


@_rowmap("vc_channel_scale")
def test_channel_scale_row_map(dev, case):
    _regime(case)
    _scale(dev, case.n, case.c, case.h, case.w, [er.DENSE, dict(cpad=1)])


def _clamp(dev, n, c, h, w, specs, edge=False, larger=False):
    hip, L, s = _api()
    x = er.clamp_inputs(n, c + 2 * larger, h + larger, w + 2 * larger, edge)
    ref = er.F32.clamp01(x)[:, :c, :h, :w]
    assert _same_bits(ref, er.clamp01(x)[:, :c, :h, :w])
    ti, to = er.place(x, dev, **specs[0]), _out((n, c, h, w), dev, specs[1])
    _ok(L.vc_clamp01(s, ti.view(), to.view()), "vc_clamp01")
    _finish("vc_clamp01", f"{n}x{c}x{h}x{w} edge={edge}", to, ref)
    if not larger:
        tio = er.place(x, dev, fill=er.SENTINEL, **specs[1])
        _ok(L.vc_clamp01(s, tio.view(), tio.view()), "vc_clamp01")
        _finish("vc_clamp01", f"{n}x{c}x{h}x{w} edge={edge} in place", tio, ref)


@_sv
def test_clamp01_views(dev, h, w, viewset):
    """vc_clamp01: a and out in every kind of view, in place, the top-left of a larger input"""
    _clamp(dev, er.N, 5, h, w, er.specs_of(viewset, 2))
    _clamp(dev, er.N, 5, h, w, er.specs_of(viewset, 2), larger=True)


@pytest.mark.parametrize("h,w", er.SIZES)
def test_clamp01_edges(dev, h, w):
    """vc_clamp01: -0.0, 0, 1, 1 +- 1 ulp, +-inf, subnormals"""
    _clamp(dev, er.N, 5, h, w, er.specs_of("rot1", 2), edge=True)


@_rowmap("vc_clamp01")
def test_clamp01_row_map(dev, case):
    """several workgroups a row, the linear fallback and -- for this kernel as the one representative -- the row loop"""
    _regime(case)
    _clamp(dev, case.n, case.c, case.h, case.w, [er.DENSE, dict(cpad=1)], edge=True)


def test_clamp_and_scale_contract(dev):
    """vc_clamp01, vc_channel_scale: null pointers, an input lower / narrower / with fewer channels than out or of another image
    count; empty views"""
    hip, L, s = _api()
    n, c, h, w = 2, 4, 5, 7
    x, gain = er.quant_inputs(n, c, h, w)
    gd = gain.to(dev)
    ti, to = er.place(x, dev), _out((n, c, h, w), dev, {})
    cl, cs = L.vc_clamp01, L.vc_channel_scale
    calls = [("clamp: null a", cl(s, _null(n, h, w, c), to.view())), ("clamp: null out", cl(s, ti.view(), _null(n, h, w, c))),
             ("scale: null a", cs(s, _null(n, h, w, c), gd.data_ptr(), to.view())), ("scale: null gain", cs(s, ti.view(), None, to.view())),
             ("scale: null out", cs(s, ti.view(), gd.data_ptr(), _null(n, h, w, c)))]
    for what, over in (("n", dict(n=1)), ("more images", dict(n=3)), ("lower", dict(h=4)), ("narrower", dict(w=6)), ("fewer channels", dict(c=3))):
        calls += [(f"clamp: a {what}", cl(s, _v(ti, **over), to.view())), (f"scale: a {what}", cs(s, _v(ti, **over), gd.data_ptr(), to.view()))]
    _refused([to], calls)
    _empty_ok([to], [("clamp: no row", cl(s, ti.view(), _v(to, h=0))), ("scale: no column", cs(s, ti.view(), gd.data_ptr(), _v(to, w=0)))])


# ------------------------------------------------------------------------------------------------
# half copies
# ------------------------------------------------------------------------------------------------
def _half(dev, n, c, h, w, spec, cg=None, edge=False, skew=0):
    hip, L, s = _api()
    x = er.half_inputs(n, c, h, w, edge)
    ti = er.place(x, dev, **spec)
    buf, ptr, check = _guarded(n * c * h * w, dev, torch.float16, skew)
    if cg is None:
        _ok(L.vc_to_half(s, ti.view(), ptr), "vc_to_half")
        ref = er.F32.to_half(x)
        assert torch.equal(ref, er.to_half(x))
    else:
        _ok(L.vc_to_half_planar(s, ti.view(), cg, ptr), "vc_to_half_planar")
        ref = er.F32.to_half_planar(x, cg)
        assert torch.equal(ref, er.to_half_planar(x, cg))
    got = check().view(torch.int16)
    bad = (got != ref.reshape(-1)).sum().item()
    assert bad == 0, f"{'vc_to_half' if cg is None else f'vc_to_half_planar cg={cg}'} {n}x{c}x{h}x{w}: {bad} halves differ from x.half()"


@pytest.mark.parametrize("spec", range(3))
@pytest.mark.parametrize("h,w", er.SHAPES)
def test_to_half_views(dev, h, w, spec):
    """vc_to_half: the input dense and as two 16-byte aligned windows; the output 16- and 8-byte aligned"""
    _half(dev, er.N, 8, h, w, er.ALIGNED[spec], skew=4 * (spec == 1))


@pytest.mark.parametrize("cg", er.PLANAR_CG)
@pytest.mark.parametrize("spec", range(3))
@pytest.mark.parametrize("h,w", er.SHAPES)
def test_to_half_planar_views(dev, h, w, spec, cg):
    """vc_to_half_planar: every cg in {4, 8, 12, 16}, three groups, the input dense and as aligned windows"""
    _half(dev, er.N, 3 * cg, h, w, er.ALIGNED[spec], cg=cg, skew=4 * (spec == 2))


@pytest.mark.parametrize("cg", [None] + er.PLANAR_CG)
def test_to_half_edges(dev, cg):
    """vc_to_half, vc_to_half_planar: ties (1 + 2^-11, 1 + 3 2^-11), 65504, 65520 -> inf, 2^-14, 2^-24, 2^-25 -> what x.half() gives
    (subnormal results rounded half to even, not flushed), +-0; the input a window"""
    _half(dev, er.N, 2 * (cg or 4), 3, 37, er.WIN_A, cg=cg, edge=True)


@pytest.mark.parametrize("case", [c for c in er.ROWMAP_CASES if c.entry.startswith("vc_to_half")], ids=lambda c: c.id)
def test_half_copies_row_map(dev, case):
    _regime(case)
    _half(dev, case.n, case.c, case.h, case.w, er.DENSE, cg=case.cg if case.entry == "vc_to_half_planar" else None)


def test_half_copies_contract(dev):
    """vc_to_half, vc_to_half_planar: null pointers, c % 4, c % cg, cg outside {4, 8, 12, 16}, unaligned pointers and strides;
    empty views"""
    hip, L, s = _api()
    n, c, h, w = 2, 48, 3, 5
    x = er.half_inputs(n, c, h, w)
    ti, off1 = er.place(x, dev), er.place(x, dev, c0=1, cpad=4)
    buf, ptr, check = _guarded(n * c * h * w, dev, torch.float16)
    th, tp = L.vc_to_half, L.vc_to_half_planar
    bad = [("6 channels", _v(ti, c=6)), ("pixel stride 49", _v(ti, sw=49)), ("row pitch + 2", _v(ti, sh=ti.sh + 2)), ("image pitch + 1", _v(ti, sn=ti.sn + 1)),
           ("input 4 bytes off", off1.view()), ("null input", _null(n, h, w, c))]
    calls = [(f"to_half: {k}", th(s, v, ptr)) for k, v in bad] + [(f"planar: {k}", tp(s, v, 4 if k == "6 channels" else 8, ptr)) for k, v in bad]
    calls += [("to_half: null output", th(s, ti.view(), None)), ("to_half: output 4 bytes off", th(s, ti.view(), ptr + 4)),
              ("planar: null output", tp(s, ti.view(), 8, None)), ("planar: output 2 bytes off", tp(s, ti.view(), 8, ptr + 2)),
              ("planar: 48 % 20", tp(s, ti.view(), 20, ptr)), ("planar: 16 % 12", tp(s, _v(ti, c=16), 12, ptr)),
              ("planar: cg = 0", tp(s, ti.view(), 0, ptr)), ("planar: cg = -4", tp(s, ti.view(), -4, ptr)), ("planar: cg = 2", tp(s, ti.view(), 2, ptr)),
              ("planar: cg = 6", tp(s, ti.view(), 6, ptr)), ("planar: cg = 24", tp(s, ti.view(), 24, ptr)), ("planar: cg = 20 of 40", tp(s, _v(ti, c=40), 20, ptr))]
    for what, rc in calls:
        assert rc == EINVAL, f"{what}: returned {rc}"
    for what, rc in [("to_half: no row", th(s, _v(ti, h=0), ptr)), ("planar: no image", tp(s, _v(ti, n=0), 8, ptr))]:
        assert rc == 0, f"{what}: returned {rc}, not VC_OK"
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int16) == GUARD).all())


# ------------------------------------------------------------------------------------------------
# layouts, SPyNet pre-processing
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", er.LAYOUT_C)
@pytest.mark.parametrize("spec", range(3))
@pytest.mark.parametrize("h,w", er.SHAPES)
def test_layouts_one_direction_at_a_time(dev, h, w, spec, c):
    """vc_nchw_to_nhwc into a window and vc_nhwc_to_nchw out of one, each against permute on its own (a round trip cannot see a
    permutation both share); every element another value; c in {1, 3, 5, 8}"""
    hip, L, s = _api()
    x = er.distinct(er.N, c, h, w)
    to = _out((er.N, c, h, w), dev, er.SPECS[spec])
    src = x.contiguous().to(dev)
    _ok(L.vc_nchw_to_nhwc(s, src.data_ptr(), to.view()), "vc_nchw_to_nhwc")
    win, outside = er.read_window(to)
    er.assert_untouched(outside)
    assert torch.equal(win, x)                        # (read_window and place index the channels-last buffer through torch, not through a kernel)
    ti = er.place(x, dev, **er.SPECS[spec])
    buf, ptr, check = _guarded(x.numel(), dev, torch.float32)
    _ok(L.vc_nhwc_to_nchw(s, ti.view(), ptr), "vc_nhwc_to_nchw")
    assert torch.equal(check().view(er.N, c, h, w), x)


def _spynet(dev, n, h, w, spec, edge=False):
    hip, L, s = _api()
    x = er.spynet_inputs(n, h, w, edge)
    ref, mag = er.spynet_preprocess(x)
    src, to = x.contiguous().to(dev), _out((n, 3, h, w), dev, spec)
    _ok(L.vc_spynet_preprocess(s, src.data_ptr(), to.view()), "vc_spynet_preprocess")
    got = _finish("vc_spynet_preprocess", f"{n}x{h}x{w} edge={edge}", to, ref, mag)
    if edge:                                     # an input channel at its own mean gives exactly 0 in output channel 2 - i
        for i in range(3):
            at = x[:, i] == torch.tensor(er.MEANS[i], dtype=torch.float32)
            assert (bool(at.any()) or at.numel() < 4) and not bool(got[:, 2 - i][at].any())      # (a 1 x 1 image holds two of the four values)


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("spec", range(3))
@pytest.mark.parametrize("h,w", er.SHAPES)
def test_spynet_preprocess_views(dev, h, w, spec, edge):
    """vc_spynet_preprocess: three channels of distinct values (the flip, and the pairing of mean and std with the channel); 0, 1
    and the means themselves; dst in every kind of view"""
    _spynet(dev, er.N, h, w, er.SPECS[spec], edge)


def test_layout_and_preprocess_contract(dev):
    """vc_nchw_to_nhwc, vc_nhwc_to_nchw, vc_spynet_preprocess: null pointers, dst.c != 3; views with a non-positive size return
    VC_OK without a launch"""
    hip, L, s = _api()
    n, c, h, w = 2, 3, 5, 7
    x = er.distinct(n, c, h, w)
    src, ti, to = x.to(dev), er.place(x, dev), _out((n, c, h, w), dev, {})
    t4 = _out((n, 4, h, w), dev, {})
    dense = torch.full((x.numel(),), er.SENTINEL, device=dev)
    a, b, p = L.vc_nchw_to_nhwc, L.vc_nhwc_to_nchw, L.vc_spynet_preprocess
    _refused([to, t4, dense], [
        ("nchw_to_nhwc: null src", a(s, None, to.view())), ("nchw_to_nhwc: null dst", a(s, src.data_ptr(), _null(n, h, w, c))),
        ("nhwc_to_nchw: null src", b(s, _null(n, h, w, c), dense.data_ptr())), ("nhwc_to_nchw: null dst", b(s, ti.view(), None)),
        ("preprocess: null src", p(s, None, to.view())), ("preprocess: null dst", p(s, src.data_ptr(), _null(n, h, w, 3))),
        ("preprocess: dst of 2 channels", p(s, src.data_ptr(), _v(to, c=2))), ("preprocess: dst of 4 channels", p(s, src.data_ptr(), t4.view())),
    ])
    empty = [dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(h=-2), dict(w=-3)]
    calls = []
    for o in empty + [dict(c=0), dict(c=-1)]:
        calls += [(f"nchw_to_nhwc {o}", a(s, src.data_ptr(), _v(to, **o))), (f"nhwc_to_nchw {o}", b(s, _v(ti, **o), dense.data_ptr()))]
    calls += [(f"preprocess {o}", p(s, src.data_ptr(), _v(to, **o))) for o in empty]
    _empty_ok([to, dense], calls)


# ------------------------------------------------------------------------------------------------
# split records
# ------------------------------------------------------------------------------------------------
def _split_out(dev, n, h, w, c, wide):
    """a split tensor filled with the guard: dense, or planes 1 .. of a tensor 16 channels wider -> (whole tensor, window, first plane)"""
    from vcamd import hip
    t = hip.T.empty(n, h, w, c + 16 * wide, dev, "sp3")
    t.buf.fill_(GUARD)
    return t, (t.channels(8, 8 + c) if wide else t), int(wide)


def _check_split(whole, first, n, h, w, c, want):
    """planes [first, first + c / 8) of every image equal `want` (the host's dense split tensor), every other plane keeps the guard"""
    got = whole.buf.cpu().view(n, whole.sn, h * w * 24)
    assert torch.equal(got[:, first:first + c // 8].reshape(-1), want), "the record differs from the host's split"
    assert bool((got[:, :first] == GUARD).all()) and bool((got[:, first + c // 8:] == GUARD).all()), "planes outside the window were written"


def _specials_in_image_0(n, c, h, w):
    x = er.split_inputs(n, c, h, w).clone()
    x[0] = er.split_inputs(n, c, h, w, True)[0]
    return x


@pytest.mark.parametrize("c", [8, 16, 32, 64])
@pytest.mark.parametrize("spec", range(3))
@pytest.mark.parametrize("h,w", er.SHAPES)
def test_split3_views(dev, h, w, spec, c):
    """vc_split3: 1, 2, 4 and 8 planes a workgroup; the special values 0, -0, 1e-30, -3e38, 2^-120, 1 + 2^-23, -(2 - 2^-23):
    hi + mid + lo == x bit for bit, the record equal to the host's; dense and into a window of planes of a wider split tensor
    (out_image_bytes != 0) whose other planes keep their guard; the input dense and as aligned windows"""
    hip, L, s = _api()
    n = er.N
    x = _specials_in_image_0(n, c, h, w)
    ti = er.place(x, dev, **er.ALIGNED[spec])
    want = er.split_host(x)
    for wide in (False, True):
        whole, win, first = _split_out(dev, n, h, w, c, wide)
        _ok(L.vc_split3(s, ti.view(), win.ptr, win.image_bytes if wide else 0), "vc_split3")
        _check_split(whole, first, n, h, w, c, want)
    hi, mid, lo = er.pieces(whole.buf.cpu().view(n, whole.sn, -1)[:, 1:1 + c // 8].reshape(-1), n, c, h, w)
    assert _same_bits((hi + mid) + lo, torch.where(x == 0, torch.zeros_like(x), x))        # (the pieces of -0.0 sum to +0.0)
    assert torch.equal(er.unsplit(whole.buf.cpu().view(n, whole.sn, -1)[:, 1:1 + c // 8].reshape(-1), n, c, h, w), x.double())


@pytest.mark.parametrize("c,c_out", er.SPLIT_PAD_C)
@pytest.mark.parametrize("spec", range(3))
@pytest.mark.parametrize("h,w", er.SHAPES)
def test_split3_pad_views(dev, h, w, spec, c, c_out):
    """vc_split3_pad: c in {1, 3, 6, 9, 13} padded to 8 / 16, the channels past c +0.0 in all three pieces, the special values, the
    input dense, a window and an UNALIGNED window (the kernel asks no alignment of it), dense and into a window of planes"""
    hip, L, s = _api()
    n = er.N
    x = _specials_in_image_0(n, c, h, w)
    ti = er.place(x, dev, **er.SPECS[spec])
    want = er.split_pad_host(x, c_out)
    assert not bool(er.pieces(want, n, c_out, h, w)[:, :, c:].view(torch.int32).any())
    for wide in (False, True):
        whole, win, first = _split_out(dev, n, h, w, c_out, wide)
        _ok(L.vc_split3_pad(s, ti.view(), win.ptr, win.image_bytes if wide else 0, c_out), "vc_split3_pad")
        _check_split(whole, first, n, h, w, c_out, want)
    assert torch.equal(er.unsplit(whole.buf.cpu().view(n, whole.sn, -1)[:, 1:1 + c_out // 8].reshape(-1), n, c_out, h, w)[:, :c], x.double())


def test_split_contract(dev):
    """vc_split3, vc_split3_pad: null pointers, c % 8, unaligned input pointer and strides (vc_split3), an unaligned output, an image
    pitch that is no multiple of 16, c_out < c, c_out % 8, no channel; empty views"""
    hip, L, s = _api()
    n, c, h, w = 2, 16, 3, 5
    x = er.split_inputs(n, c, h, w)
    ti, off1 = er.place(x, dev), er.place(x, dev, c0=1, cpad=4)
    whole, win, _ = _split_out(dev, n, h, w, c, False)
    s3, sp = L.vc_split3, L.vc_split3_pad
    calls = [("split3: null input", s3(s, _null(n, h, w, c), win.ptr, 0)), ("split3: null output", s3(s, ti.view(), None, 0)),
             ("split3: 12 channels", s3(s, _v(ti, c=12), win.ptr, 0)), ("split3: pixel stride 17", s3(s, _v(ti, sw=17), win.ptr, 0)),
             ("split3: row pitch + 2", s3(s, _v(ti, sh=ti.sh + 2), win.ptr, 0)), ("split3: image pitch + 1", s3(s, _v(ti, sn=ti.sn + 1), win.ptr, 0)),
             ("split3: input 4 bytes off", s3(s, off1.view(), win.ptr, 0)), ("split3: output 8 bytes off", s3(s, ti.view(), win.ptr + 8, 0)),
             ("split3: output image pitch + 8", s3(s, ti.view(), win.ptr, win.image_bytes + 8)),
             ("pad: null input", sp(s, _null(n, h, w, c), win.ptr, 0, 16)), ("pad: null output", sp(s, ti.view(), None, 0, 16)),
             ("pad: c_out < c", sp(s, ti.view(), win.ptr, 0, 8)), ("pad: c_out % 8", sp(s, _v(ti, c=9), win.ptr, 0, 12)),
             ("pad: no channel", sp(s, _v(ti, c=0), win.ptr, 0, 8)), ("pad: output 8 bytes off", sp(s, _v(ti, c=9), win.ptr + 8, 0, 16)),
             ("pad: output image pitch + 8", sp(s, _v(ti, c=9), win.ptr, win.image_bytes + 8, 16))]
    for what, rc in calls:
        assert rc == EINVAL, f"{what}: returned {rc}"
    for what, rc in [("split3: no row", s3(s, _v(ti, h=0), win.ptr, 0)), ("split3: no image", s3(s, _v(ti, n=0), win.ptr, 0)),
                     ("pad: no column", sp(s, _v(ti, w=0, c=9), win.ptr, 0, 16))]:
        assert rc == 0, f"{what}: returned {rc}, not VC_OK"
    torch.cuda.synchronize()
    assert bool((whole.buf == GUARD).all())
