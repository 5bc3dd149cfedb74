"""-m gpu: MS-SSIM of the evaluation loops (vc_msssim, csrc/metrics.hip) against an fp64 CPU restatement of the definition
(pytorch-msssim's ``ms_ssim`` with its default arguments, data range 255) built from F.conv2d and F.avg_pool2d.

Bound on every case: |HIP - fp64| <= 1e-6 on the value and on each of the 5*C per-scale terms.  Derivation: the published
figures carry four decimals, so an error must stay below 5e-5; 1e-6 is 50x inside that, 6x above what even an fp32 evaluation
reaches on textured input (1.6e-7) and 700x below the fp32 failure on the flat frame (7.4e-4: F(XX) - mu^2 cancels there).

Every case prints its measured maxima (run with -s).  The kernel accumulates the window sums in fp64 on exact fp32 pixels, so
with quantised input only summation order separates it from the restatement; with quantize=False the kernel forms v * 255 in
fp32 (relative 6e-8 per pixel, ~1e-7 on a term by the argument in DESIGN section 4b) where the restatement forms it in fp64.
"""
import pytest
import torch
import torch.nn.functional as F

from helpers import lhbdc_pair

pytestmark = pytest.mark.gpu

BOUND = 1e-6
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def ref_msssim(a, b, h, w, quantize=True):
    """fp64 restatement: returns (values [N], terms [N,5,C])."""
    def prep(t):
        t = t[..., :h, :w]
        if quantize:
            return torch.round(t.clamp(0.0, 1.0) * 255.0).double()       # fp32 clamp / scale / round half to even, like the loops
        return t.double() * 255.0
    X, Y = prep(a), prep(b)
    c = X.shape[1]
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    g = g / g.sum()
    wr, wc = g.view(1, 1, 1, 11).repeat(c, 1, 1, 1), g.view(1, 1, 11, 1).repeat(c, 1, 1, 1)
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2

    def filt(t):
        return F.conv2d(F.conv2d(t, wr, groups=c), wc, groups=c)
    terms = []
    for s in range(5):
        mu1, mu2 = filt(X), filt(Y)
        s1, s2, s12 = filt(X * X) - mu1 * mu1, filt(Y * Y) - mu2 * mu2, filt(X * Y) - mu1 * mu2
        m = (2.0 * s12 + c2) / (s1 + s2 + c2)
        if s == 4:
            m = (2.0 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * m
        terms.append(torch.relu(m.mean((2, 3))))
        if s < 4:
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
    terms = torch.stack(terms, 1)                                                    # [N,5,C]
    val = torch.prod(terms ** torch.tensor(WEIGHTS, dtype=torch.float64).view(1, 5, 1), 1).mean(1)
    return val, terms


def textured(n, c, H, W, sigma, seed):
    """a smooth random field and the same plus Gaussian noise of ``sigma`` (of full scale)"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(n, c, H // 16 + 2, W // 16 + 2, generator=g)
    x = (0.15 + 0.7 * F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False)).clamp(0.02, 0.98).contiguous()
    y = (x + sigma * torch.randn(n, c, H, W, generator=g)).contiguous()
    return y, x


def check(dev, a, b, h, w, quantize=True, tag=""):
    from vcamd import hip
    val, terms = hip.msssim_uint8(a.to(dev), b.to(dev), h, w, quantize=quantize, terms=True)
    rv, rt = ref_msssim(a, b, h, w, quantize)
    ev, et = (val.cpu() - rv).abs().max().item(), (terms.cpu() - rt).abs().max().item()
    print(f"msssim {tag}: value {val.cpu().tolist()} |d value| {ev:.3e} |d terms| {et:.3e} min term {rt.min().item():.6f}")
    assert val.dtype == torch.float64 and tuple(val.shape) == (a.shape[0],) and tuple(terms.shape) == (a.shape[0], 5, a.shape[1])
    assert ev <= BOUND and et <= BOUND
    return val.cpu(), rv, rt


@pytest.mark.parametrize("sigma", [0.004, 0.02, 0.1])
def test_odd_at_every_level(dev, sigma):
    """161 -> 81 -> 41 -> 21 -> 11: every pool pads, the last map is a single row."""
    a, b = textured(1, 3, 192, 256, sigma, 11)
    _, _, rt = check(dev, a, b, 161, 163, tag=f"odd sigma {sigma}")
    assert rt.min().item() > 0.0        # no term at the clamp


@pytest.mark.parametrize("sigma", [0.004, 0.02, 0.1])
def test_1080p_parity_pattern_small_two_images(dev, sigma):
    """270, 135, 68, 34, 17 x 180, 90, 45, 23, 12: the even / odd sequence of 1080 rows; two different images in one call."""
    a, b = textured(2, 3, 320, 192, sigma, 12)
    val, _, _ = check(dev, a, b, 270, 180, tag=f"parity sigma {sigma}")
    assert val[0].item() != val[1].item()


def test_no_crop_one_channel(dev):
    a, b = textured(1, 1, 192, 192, 0.02, 13)
    check(dev, a, b, 192, 192, tag="192x192 c1")


def test_full_size(dev):
    a, b = textured(1, 3, 1088, 1920, 0.02, 14)
    check(dev, a, b, 1080, 1920, tag="1080p")


def test_flat_frame(dev):
    """0.9 everywhere against the same with every second column one code lower: F(XX) - mu^2 cancels to 0 / 0.25 -- an fp32
    evaluation of the window sums is off by 7.4e-4 here."""
    a = torch.full((1, 3, 192, 256), 230.0 / 255.0)
    b = a.clone()
    b[..., 1::2] = 229.0 / 255.0
    val, _, _ = check(dev, a, b, 161, 163, tag="flat")
    assert abs(val.item() - 0.99980845) <= BOUND


def test_identical_images(dev):
    a, _ = textured(1, 3, 192, 256, 0.02, 15)
    val, _, _ = check(dev, a, a.clone(), 161, 163, tag="identical")
    assert abs(val.item() - 1.0) <= BOUND


def test_anticorrelated_images_give_zero_not_nan(dev):
    from vcamd import hip
    x = torch.rand(1, 3, 192, 256, generator=torch.Generator().manual_seed(16))
    val, terms = hip.msssim_uint8((1.0 - x).to(dev), x.to(dev), 161, 163, terms=True)
    rv, rt = ref_msssim(1.0 - x, x, 161, 163)
    print(f"msssim anti: value {val.item()} terms {terms.cpu().flatten().tolist()}")
    assert rv.item() == 0.0 and val.item() == 0.0
    assert (terms.cpu()[0, 0] == 0.0).all() and (terms.cpu() - rt).abs().max().item() <= BOUND


def test_quantisation(dev):
    """values outside [0,1] clamp, (k + 0.5) / 255 rounds half to even, quantize=False takes v * 255 as it is"""
    a, b = textured(1, 3, 192, 256, 0.3, 17)                      # noise of 0.3: a good part of `a` leaves [0,1]
    assert (a < 0).any() and (a > 1).any()
    check(dev, a, b, 161, 163, tag="out of range")
    k = torch.randint(0, 255, (1, 3, 192, 256), generator=torch.Generator().manual_seed(18)).float()
    half = (k + 0.5) / 255.0
    check(dev, half, b, 161, 163, tag="half codes")
    c, d = textured(1, 3, 192, 256, 0.02, 19)
    vq, _, _ = check(dev, c, d, 161, 163, tag="quantised")
    vu, _, _ = check(dev, c, d, 161, 163, quantize=False, tag="unquantised")
    assert vq.item() != vu.item()


def test_refusals_and_out_slot(dev):
    from vcamd import hip
    a, b = textured(1, 3, 192, 256, 0.02, 20)
    with pytest.raises(hip.VcError):
        hip.msssim_uint8(a, b, 161, 163)                                   # CPU tensors
    with pytest.raises(hip.VcError):
        hip.msssim_uint8(a.to(dev), b.to(dev), 160, 163)                   # min(h, w) = 160
    with pytest.raises(hip.VcError):
        hip.msssim_uint8(a.to(dev), b.to(dev), 161, 160)
    with pytest.raises(hip.VcError):
        hip.msssim_uint8(a.to(dev), b[..., :190, :].contiguous().to(dev), 161, 163)     # mismatched shapes
    with pytest.raises(hip.VcError):
        hip.msssim_uint8(a.to(dev), torch.cat([b, b]).to(dev), 161, 163)
    slots = torch.full((4,), -1.0, dtype=torch.float64, device=dev)
    ret = hip.msssim_uint8(a.to(dev), b.to(dev), 161, 163, out=slots[2:3])
    want = hip.msssim_uint8(a.to(dev), b.to(dev), 161, 163)
    assert ret.data_ptr() == slots[2:3].data_ptr()
    assert slots[2].item() == want.item() and slots[0].item() == -1.0 and slots[1].item() == -1.0 and slots[3].item() == -1.0


def test_deterministic(dev):
    from vcamd import hip
    a, b = textured(2, 3, 320, 192, 0.02, 21)
    a, b = a.to(dev), b.to(dev)
    v1, t1 = hip.msssim_uint8(a, b, 270, 180, terms=True)
    v2, t2 = hip.msssim_uint8(a, b, 270, 180, terms=True)
    assert torch.equal(v1, v2) and torch.equal(t1, t2)


def test_graph_capture_and_replay_on_new_contents(dev):
    from vcamd import hip
    a, b = textured(1, 3, 192, 256, 0.02, 22)
    a2, b2 = textured(1, 3, 192, 256, 0.1, 23)
    sa, sb = a.to(dev), b.to(dev)
    hip.msssim_uint8(sa, sb, 161, 163)                       # eager warm-up: loads the code object
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = hip.msssim_uint8(sa, sb, 161, 163)
    sa.copy_(a2.to(dev))
    sb.copy_(b2.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    got = out.clone()
    eager = hip.msssim_uint8(a2.to(dev), b2.to(dev), 161, 163)
    old = hip.msssim_uint8(a.to(dev), b.to(dev), 161, 163)
    assert torch.equal(got, eager) and not torch.equal(got, old)


def test_loops_record_msssim(dev):
    """code_gop_lhbdc / GopGraph with msssim=True: 8-field records, field 7 == a stand-alone call on that decoded / source pair,
    fields 0..5 identical to the msssim=False run."""
    from vcamd import gop as vgop
    from vcamd import hip
    _, prod = lhbdc_pair(1234, dev)
    g = torch.Generator().manual_seed(9)
    base = F.avg_pool2d(torch.rand(1, 3, 200, 280, generator=g), 9, 1)
    frames = [base[..., :192, i:i + 256].contiguous().to(dev) for i in range(9)]
    h, w = 161, 163
    with torch.no_grad():
        plain, ext = [], []
        vgop.code_gop_lhbdc(prod, frames, frames[0], frames[8], h, w, plain)
        dec = vgop.code_gop_lhbdc(prod, frames, frames[0], frames[8], h, w, ext, msssim=True)
        dec = {k: v.clone() for k, v in dec.items()}
        assert len(plain) == len(ext) == 7
        for p, e in zip(plain, ext):
            assert len(p) == 6 and len(e) == 8 and e[6] == 0
            assert p[:3] == e[:3] and torch.equal(p[3], e[3]) and torch.equal(p[4], e[4]) and p[5] == e[5]
            alone = hip.msssim_uint8(dec[e[1]], frames[e[1]], h, w)[0]
            assert e[7].dtype == torch.float64 and torch.equal(e[7], alone)
            assert 0.0 < e[7].item() <= 1.0
        runner = vgop.GopGraph(prod, h, w, msssim=True)
        rec_g = []
        runner.code(frames, records=rec_g)
        for e, r in zip(ext, rec_g):
            assert len(r) == 8 and r[:3] == e[:3] and r[5] == e[5] and r[6] == 0
            assert torch.equal(r[3], e[3]) and torch.equal(r[4], e[4]) and torch.equal(r[7], e[7])
    rows = vgop.gather_records(rec_g, dev)
    s = vgop.summarize(rows)
    assert rows.shape == (7, 8) and abs(s["msssim"] - sum(e[7].item() for e in ext) / 7) < 1e-15
