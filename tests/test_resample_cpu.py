"""The references and case tables of tests/test_resample_gpu.py pinned on the CPU (tests/resample_ref.py): on every case's inputs the
fp32 torch operator the reference project calls stays inside the cap the kernel is held to, measured against the float64 reference
-- so a kernel that misses a cap has no excuse in the reference; ``unsplit`` reads a host-made split record exactly; every case lands
on the dispatch form its id names; every row-loop and fallback shape satisfies the inequality that makes it one."""
import pytest
import torch
import torch.nn.functional as F

import resample_ref as rr

MAXIMA = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(MAXIMA):
        print(f"\nfp32 CPU operator against float64, largest |d| / (1 + |ref|), {k}: {MAXIMA[k]:.2e}", end="")


def _hold(entry, what, out, ref, cap):
    assert torch.isfinite(ref).all(), f"{entry} {what}: the float64 reference is not finite"
    d = rr.rel_err(out, ref)
    MAXIMA[entry] = max(MAXIMA.get(entry, 0.0), d)
    assert d <= cap, f"{entry} {what}: the fp32 operator itself is {d:.3e} > {cap} from float64: a bad case"


def _ids(case):
    return case.id


# ---- the fp32 operators stay inside the caps ----
def _w3(img, flow):
    from oracle.icip2024 import warp_w3
    return warp_w3(img, flow)


def _fp32_warp(convention):
    from oracle.flex import warp_w2
    from oracle.lhbdc import warp_w1
    return {1: warp_w1, 2: warp_w2, 3: _w3}[convention]


@pytest.mark.parametrize("convention", [1, 2, 3])
def test_warp_cases_fp32_within_the_cap(convention):
    shapes = {(c.c_img, h, w, 2) for c in rr.WARP_CASES for h, w in rr.SIZES}
    shapes |= {(c, h, w, 2) for c in (3, 5, 8) for h, w in rr.TINY}
    shapes |= {(c.c_img, c.h, c.w, c.n) for c in rr.WARP_FALLBACK}
    for c, h, w, n in sorted(shapes):
        img, flow = rr.warp_inputs(convention, c, h, w, n)
        assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0
        ref = rr.warp_ref(convention, c, h, w, n)
        _hold(f"warp W{convention}", f"c={c} {n}x{h}x{w}", _fp32_warp(convention)(img, flow), ref, rr.CAP_WARP)
        # the restated recipe in fp32 is the oracle's
        assert torch.equal(rr.warp(convention, img, flow, torch.float32), _fp32_warp(convention)(img, flow))


def test_warp_inputs_hold_the_edges():
    """zero flow, samples on the last row / column, within a pixel outside every border, far outside -- on every base size"""
    for h, w in rr.SIZES:
        _, flow = rr.warp_inputs(3, 3, h, w)                      # W3: position = pixel + flow
        px = flow[:, 0].double() + torch.arange(w).view(1, 1, w)
        py = flow[:, 1].double() + torch.arange(h).view(1, h, 1)
        assert bool((flow == 0).all(1).any())
        for p, size in ((px, w), (py, h)):
            assert bool((p == size - 1).any()) and bool((p == 0).any())
            assert bool(((p > -1) & (p < 0)).any()) and bool(((p > size - 1) & (p < size)).any())
            assert bool((p < -10).any()) and bool((p > size + 10).any())
        _, f2 = rr.warp_inputs(2, 3, h, w)                        # W2: position = pixel + flow - 0.5; partial weights of the zero padding
        p2 = f2[:, 0].double() + torch.arange(w).view(1, 1, w) - 0.5
        assert bool(((p2 > -1) & (p2 < 0)).any()) and bool(((p2 > w - 1) & (p2 < w)).any())


@pytest.mark.parametrize("case", rr.UPSAMPLE_CASES + rr.UPSAMPLE_ROWMAP + [rr.UPSAMPLE_ROWLOOP, rr.UPSAMPLE_FALLBACK], ids=_ids)
def test_upsample_cases_fp32_within_the_cap(case):
    x = rr.upsample_inputs(case.c, case.n, case.h, case.w)
    ref = rr.upsample(x, case.factor, case.align, case.scale)
    out = case.scale * F.interpolate(x, scale_factor=case.factor, mode="bilinear", align_corners=case.align)
    _hold("upsample", case.id, out, ref, rr.CAP_LINEAR)


@pytest.mark.parametrize("case", rr.UPSAMPLE_SP3, ids=_ids)
def test_upsample_sp3_cases_fp32_within_the_cap(case):
    x = rr.upsample_inputs(case.c, case.n, case.h, case.w)
    out = case.scale * F.interpolate(x, scale_factor=case.factor, mode="bilinear", align_corners=case.align)
    _hold("upsample", case.id, out, rr.upsample(x, case.factor, case.align, case.scale), rr.CAP_LINEAR)


def test_upsample_table_covers_the_arithmetic():
    t = rr.UPSAMPLE_CASES
    assert {c.factor for c in t} == {1, 2, 3, 4} and {c.align for c in t} == {False, True}
    for form in ("scalar", "v4"):
        for al in (False, True):
            mine = [c for c in t if c.form == form and c.align == al]
            assert any(c.h == 1 and c.w == 1 for c in mine) and any(c.h == 1 and c.w > 1 for c in mine) and any(c.w == 1 and c.h > 1 for c in mine)
            assert any(c.scale != 1.0 for c in mine) and {c.factor for c in mine} == {1, 2, 3, 4}


@pytest.mark.parametrize("case", rr.AVGPOOL_CASES + [rr.AVGPOOL_FALLBACK], ids=_ids)
def test_avgpool_cases_fp32_within_the_cap(case):
    x = rr.upsample_inputs(case.c, case.n, case.h, case.w)
    ref = rr.avgpool_reflectpad(x, case.k, case.scale, case.oh, case.ow)
    assert ref.shape[2:] == (case.oh, case.ow)
    y = F.avg_pool2d(x * case.scale, case.k) if case.k > 1 else x * case.scale
    if y.shape[2:] != ref.shape[2:]:
        y = F.pad(y, (0, case.ow - y.shape[3], 0, case.oh - y.shape[2]), mode="reflect")
    _hold("avgpool_reflectpad", case.id, y, ref, rr.CAP_LINEAR)


def test_avgpool_table_covers_the_padding():
    for k in (1, 2, 4):
        mine = [c for c in rr.AVGPOOL_CASES if c.k == k]
        hp = [(c.h // k, c.w // k, c) for c in mine]
        assert any(c.oh == p and c.ow == q for p, q, c in hp) and any(c.oh == p + 1 and c.ow == q for p, q, c in hp)
        assert any(c.oh == 2 * p - 1 and p > 2 and c.ow == q for p, q, c in hp) and any(c.ow == 2 * q - 1 and q > 2 and c.oh == p for p, q, c in hp)
        assert k == 1 or any(c.h % k and c.w % k for c in mine)
        assert all(c.oh - p < p and c.ow - q < q for p, q, c in hp)            # (what reflection allows: the refusals are GPU tests)


def test_pool_sp3_cases_fp32_within_the_cap():
    for n, c, h, w in rr.POOL_SP3_SIZES:
        x = rr.upsample_inputs(c, n, h, w)
        for scale in (1.0, 0.75):
            _hold("avgpool2_sp3", f"c={c} {n}x{h}x{w}", F.avg_pool2d(x * scale, 2), rr.avgpool_reflectpad(x, 2, scale, h // 2, w // 2), rr.CAP_LINEAR)


@pytest.mark.parametrize("case", rr.AXPBY_CASES + rr.AXPBY_ROWMAP + [rr.AXPBY_ROWLOOP] + rr.AXPBY_FALLBACK, ids=_ids)
def test_axpby_cases_fp32_within_the_cap(case):
    a, b = rr.axpby_inputs(case.c, case.n, case.h, case.w)
    _hold("axpby", case.id, rr.ALPHA * a + rr.BETA * b, rr.axpby(a, b, rr.ALPHA, rr.BETA), rr.CAP_LINEAR)
    _hold("axpby", case.id, rr.ALPHA * a, rr.axpby(a, None, rr.ALPHA, rr.BETA), rr.CAP_LINEAR)


@pytest.mark.parametrize("case", rr.LEVEL_CASES, ids=_ids)
def test_level_input_cases_fp32_within_the_caps(case):
    from oracle.lhbdc import warp_w1
    first, second, fc = rr.level_inputs(case.coarse, case.h, case.w, case.n)
    feat, up = rr.level_input(first, second, fc)
    assert feat.shape == (case.n, 8, case.h, case.w) and up.shape == (case.n, 2, case.h, case.w)
    if fc is None:
        up32 = torch.zeros(case.n, 2, case.h, case.w)
    else:
        up32 = 2 * F.interpolate(fc, scale_factor=2, mode="bilinear", align_corners=True)
        up32 = F.pad(up32, (0, case.w - up32.shape[3], 0, case.h - up32.shape[2]), mode="replicate")
        assert float(up32.abs().max()) > 1.0                       # a displacement of pixels, not of nothing
    _hold("level input, up", case.id, up32, up, rr.CAP_LINEAR)
    _hold("level input, warped", case.id, warp_w1(second, up32), feat[:, 3:6], rr.CAP_WARP)
    assert torch.equal(feat[:, :3], first.double()) and torch.equal(feat[:, 6:], up)


def test_level_table_covers_the_shapes():
    t = rr.LEVEL_CASES
    for form in ("vec", "scalar"):
        mine = [c for c in t if c.form == form]
        assert any(c.coarse is None for c in mine)
        for dh, dw in ((0, 0), (1, 0), (0, 1), (1, 1)):
            assert any(c.coarse and c.h == 2 * c.coarse[0] + dh and c.w == 2 * c.coarse[1] + dw for c in mine), (form, dh, dw)
    assert {c.n for c in t} >= {1, 2}


# ---- unsplit ----
def test_unsplit_reads_a_host_made_split_tensor_exactly():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 16, 3, 5, generator=g)
    x[0, :8, 0, 0] = torch.tensor([0.0, -0.0, 1e-30, -3e38, 1.0, 2.0 ** -120, 1.0 + 2.0 ** -23, -(2.0 - 2.0 ** -23)])
    buf = rr.split_host(x)
    assert buf.dtype == torch.int16 and buf.numel() == x.numel() * 3
    assert torch.equal(rr.unsplit(buf, 2, 16, 3, 5), x.double())
    # the layout: image, plane of 8 channels, row, pixel, piece (hi, mid, lo), channel; each piece the top 16 bits of what is left
    one = torch.zeros(1, 8, 1, 2)
    one[0, 3, 0, 1] = 1.0 + 2.0 ** -8 + 2.0 ** -16
    rec = rr.split_host(one).view(1, 1, 1, 2, 3, 8)
    assert rec[0, 0, 0, 1, :, 3].tolist() == [0x3f80, 0x3b80, 0x3780] and int(rec.ne(0).sum()) == 3


# ---- dispatch forms ----
@pytest.mark.parametrize("case", rr.WARP_CASES + rr.WARP_FALLBACK, ids=_ids)
def test_warp_cases_reach_the_form_they_name(case):
    for h, w in ([(case.h, case.w)] if hasattr(case, "h") else rr.SIZES):
        img, out = rr.geom((2, case.c_img, h, w), **case.img), rr.geom((2, case.c, h, w), **case.out)
        assert rr.warp_form(img, out) == case.form and case.id.startswith(case.form + "-")
    assert case.c_img >= case.c


def test_warp_table_names_every_form():
    by_form = {f: {c.c for c in rr.WARP_CASES if c.form == f} for f in ("v4", "px3", "px", "generic")}
    assert by_form == {"v4": {8}, "px3": {3}, "px": {1, 2, 4}, "generic": {5, 7, 8}}
    assert any(c.c_img > c.c and c.out for c in rr.WARP_CASES if c.form == "v4")


@pytest.mark.parametrize("case", rr.UPSAMPLE_CASES + rr.UPSAMPLE_ROWMAP + [rr.UPSAMPLE_ROWLOOP, rr.UPSAMPLE_FALLBACK], ids=_ids)
def test_upsample_cases_reach_the_form_they_name(case):
    inp = rr.geom((case.n, case.c, case.h, case.w), **case.inp)
    out = rr.geom((case.n, case.c, case.h * case.factor, case.w * case.factor), **case.out)
    assert rr.upsample_form(inp, out) == case.form and case.id.startswith(case.form + "-")


def test_upsample_sp3_cases_reach_the_instance_they_name():
    for case in rr.UPSAMPLE_SP3:
        assert rr.upsample_sp3_pb(case.c) == case.pb and case.id.startswith(f"pb{case.pb}-")
    run = {pb: {(c.w * c.factor > rr.EW_BLOCK // pb) for c in rr.UPSAMPLE_SP3 if c.pb == pb} for pb in (8, 4, 1)}
    assert run == {8: {False, True}, 4: {False, True}, 1: {False, True}}          # below and above one workgroup's run of pixels
    assert any(c.pb == 8 and c.w * c.factor == 34 for c in rr.UPSAMPLE_SP3) and any(c.pb == 1 and c.w == 129 and c.factor == 2 for c in rr.UPSAMPLE_SP3)


@pytest.mark.parametrize("case", rr.MAXPOOL_CASES + [rr.MAXPOOL_FALLBACK], ids=_ids)
def test_maxpool_cases_reach_the_form_they_name(case):
    for h, w in case.sizes:
        inp, out = rr.geom((2, case.c, h, w), **case.inp), rr.geom((2, case.c, h // 2, w // 2), **case.out)
        assert rr.maxpool_form(inp, out) == case.form and case.id.startswith(case.form + "-")


@pytest.mark.parametrize("case", rr.AXPBY_CASES + rr.AXPBY_ROWMAP + [rr.AXPBY_ROWLOOP] + rr.AXPBY_FALLBACK, ids=_ids)
def test_axpby_cases_reach_the_form_they_name(case):
    shape = (case.n, case.c, case.h, case.w)
    a, b, out = rr.geom(shape, **case.a), rr.geom(shape, **case.b), rr.geom(shape, **case.out)
    assert rr.axpby_form(a, b, out) == case.form and rr.axpby_form(a, None, out) == case.form and case.id.startswith(case.form + "-")


@pytest.mark.parametrize("case", rr.LEVEL_CASES, ids=_ids)
def test_level_input_cases_reach_the_form_they_name(case):
    feat, up = rr.geom((case.n, 8, case.h, case.w), **case.feat), rr.geom((case.n, 2, case.h, case.w), **case.up)
    assert rr.level_input_form(feat, up) == case.form and case.id.startswith(case.form + "-")
    # the split form asks for what the vec form asks of `up`
    assert case.form != "vec" or up.off % 2 == 0


# ---- row map ----
def test_rowmap_cases_divide_by_a_reciprocal_and_span_workgroups():
    seen = set()
    for case in rr.AXPBY_ROWMAP:
        m = rr.rowmap(case.n, case.h, rr.axpby_width(case), rr.axpby_per_px(case))
        assert m is not None and m.reciprocal and (rr.axpby_width(case) * rr.axpby_per_px(case)) % rr.EW_BLOCK and not m.loops
        seen.add((rr.axpby_per_px(case), m.bx))
    assert {p for p, _ in seen} == {3, 5, 6, 12} and {b for _, b in seen} >= {1, 2, 3}
    seen = set()
    for case in rr.UPSAMPLE_ROWMAP:
        m = rr.rowmap(case.n, case.h * case.factor, case.w * case.factor, case.c)
        assert m is not None and m.reciprocal and (case.w * case.factor * case.c) % rr.EW_BLOCK and not m.loops
        seen.add((case.c, m.bx))
    assert {p for p, _ in seen} == {3, 5, 6, 12} and {b for _, b in seen} >= {1, 2, 3}


def test_every_base_case_is_one_pass_of_the_row_loop():
    """the small cases never loop over rows (h <= 8192 / (n * workgroups per row)): only the row-loop cases below test the increment"""
    for h, w in rr.SIZES + rr.TINY:
        for per_px in (1, 2, 3, 5, 7, 8, 32):
            m = rr.rowmap(2, 4 * h, 4 * w, per_px)
            assert m is not None and not m.loops


def test_rowloop_cases_iterate():
    c = rr.AXPBY_ROWLOOP
    m = rr.rowmap(c.n, c.h, c.w, c.c)
    assert c.w * c.c == 270 and (m.bx, m.gy) == (2, 64) and m.gy < c.h and m.loops and m.reciprocal
    assert c.h > 8192 // (c.n * m.bx)                                          # the inequality of csrc/ew_rowmap.h: vc_rowmap_grid
    u = rr.UPSAMPLE_ROWLOOP
    oh, ow = u.h * u.factor, u.w * u.factor
    m = rr.rowmap(u.n, oh, ow, u.c)
    assert ow * u.c == 270 and (m.bx, m.gy) == (2, 64) and oh == 70 and m.gy < oh and m.loops
    assert oh > 8192 // (u.n * m.bx)


def test_fallback_cases_leave_the_row_map():
    for c in rr.AXPBY_FALLBACK:
        assert c.h == 65536 > 65535 and rr.rowmap(c.n, c.h, rr.axpby_width(c), rr.axpby_per_px(c)) is None
    assert sorted(c.w for c in rr.AXPBY_FALLBACK) == [1, 2, 3] and {c.form for c in rr.AXPBY_FALLBACK} == {"rows", "scalar", "v4"}
    (h, w), = rr.MAXPOOL_FALLBACK.sizes
    assert (h // 2, w // 2) == (65536, 2) and rr.rowmap(2, h // 2, w // 2, rr.MAXPOOL_FALLBACK.c) is None
    assert rr.rowmap(2, 65535, w // 2, rr.MAXPOOL_FALLBACK.c) is not None                   # (one row fewer: the row map)
    a = rr.AVGPOOL_FALLBACK
    assert (a.k, a.oh, a.ow) == (1, 65536, 2) and rr.rowmap(a.n, a.oh, a.ow, a.c) is None
    for c in rr.WARP_FALLBACK:
        assert (c.n, c.h, c.w) == (65536, 2, 3) and rr.rowmap(c.n, c.h, c.w, 1 if c.form == "px3" else c.c // 4) is None
    u = rr.UPSAMPLE_FALLBACK
    assert (u.n, u.h, u.w) == (65536, 2, 3) and rr.rowmap(u.n, u.h * u.factor, u.w * u.factor, u.c) is None


def test_rowmap_reciprocal_is_exact_where_the_host_allows_it():
    """x = umulhi(j, 2^32 / per_px + 1) == j / per_px for every work item of every row-map case (the host's bound: items * per_px < 2^32)"""
    for per_px, items in [(3, 513), (5, 520), (6, 516), (12, 516), (5, 270), (3, (1 << 24) - 1), (255, (1 << 24) - 1)]:
        magic = (1 << 32) // per_px + 1
        j = torch.arange(max(0, items - 70000), items, dtype=torch.int64)
        j = torch.cat((torch.arange(min(items, 70000), dtype=torch.int64), j))
        assert items * per_px < 1 << 32 and torch.equal((j * magic) >> 32, j // per_px)
