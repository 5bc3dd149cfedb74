"""-m gpu: the ICIP2023 DeformB path (vcamd/icip2023.py) over the HIP kernels against the fixtures recorded from the reference
(tools/gen_icip2023_golden.py), and the closed-loop properties of its bitstream.

The seeded checkpoint of the fixture puts latents next to rounding boundaries at every crop of the scan (the fixture records the
smallest distances: margin_y / margin_z), so the stages BEHIND the compressors are compared teacher-forced: the integers the HIP
path would round its latents to are counted against the fixture's (<= 2 differences per tensor, the project's rule) and replaced by
them.  Bounds are those of tests/test_icip2024_gpu.py: 2e-4 (relative form) for features and offsets, 5e-5 for the aligned maps,
|dPSNR| < 1e-3 dB for x_hat against the fixture's own reconstruction, 2e-3 relative for size and rate; the sequence loop 2e-2 dB /
5e-3 over all frames and 1e-3 dB over the first six.  Bit equalities are exact."""
import pytest
import torch

from helpers import frame_tensor, load_fixture, psnr

pytestmark = pytest.mark.gpu
PSNR_TOL_DB = 1e-3
TAGS = ["s0", "s25", "s4"]
WORST_DEVIATION, FLUSH_BITS_PER_STRING = 0.20001, 8 * 16      # the size band of tests/test_icip2024_bitstream_gpu.py


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return load_fixture("icip2023_forward_a.npz")


@pytest.fixture(scope="module")
def prod(dev, fx):
    from vcamd import icip2023
    from vcamd.seeding import seeded_state_dict
    m = icip2023.DeformB()
    m.load_state_dict(seeded_state_dict(m.state_dict(), seed=int(fx["seed"])))
    m = m.to(dev).eval()
    m.offset_compressor.update(force=True)
    m.residual_compressor.update(force=True)
    return m


@pytest.fixture(scope="module")
def frames(dev, fx):
    return tuple(frame_tensor(fx[k]).to(dev) for k in ("ref_1", "ref_2", "current"))


def _strided(t):
    """a T window as a writable NCHW torch view of its buffer"""
    return torch.as_strided(t.buf[t.off:], (t.n, t.c, t.h, t.w), (t.sn, 1, t.sh, t.sw))


def _rel(out, ref):
    return ((out.double() - ref.double()).abs() / (1 + ref.double().abs())).max().item()


def _sub(t, step):
    from vcamd import hip
    return hip.nhwc_to_nchw(t).cpu().reshape(-1)[::step]


@pytest.mark.parametrize("tag", TAGS)
def test_forward_matches_reference_fixture(dev, prod, fx, frames, tag):
    from vcamd import hip
    from vcamd.layers import BitCounter
    x1, x2, xc = frames
    s = float(fx[f"s_{tag}"])
    flips = {}

    def forcer(codec):
        def force(name, t):
            v = _strided(t)
            want = torch.from_numpy(fx[f"{codec}_{name}_round_{tag}"]).to(dev).float()
            d = want - torch.round(v)
            flips[(codec, name)] = int((d != 0).sum().item())
            v += d                                  # moves only the latents whose integer differs, by whole steps
        return force
    trace = {}
    bits = BitCounter(dev, max_rows=12)
    with torch.no_grad():
        x_hat = hip.nhwc_to_nchw(prod.forward_device(hip.nchw_to_nhwc(x1), hip.nchw_to_nhwc(x2), hip.nchw_to_nhwc(xc), s, bits, trace=trace,
                                                     force={"offset": forcer("offset"), "residual": forcer("residual")})).cpu()
    size = bits.totals().sum().item()
    print(f"icip2023 {tag}: symbols that differ from the fixture's {flips} (fixture margins y {float(fx['margin_y']):.1e} z {float(fx['margin_z']):.1e})")
    assert all(v <= 2 for v in flips.values()), flips
    for name, key, cap in (("fcur", "fcur", 2e-4), ("offset", "offsets", 2e-4), ("xcomp", "x_comp", 5e-5)):
        for l in range(3):
            ref = torch.from_numpy(fx[f"{name}{l + 1}_{tag}"])
            d = _rel(_sub(trace[key][l], int(fx[f"{name}{l + 1}_step_{tag}"])), ref)
            print(f"icip2023 {tag}: {name} level {l + 1}: {d:.2e} over {ref.numel()} samples")
            assert d < cap, (name, l, d)
    step = int(fx["x_hat_row_step"])
    ref = torch.from_numpy(fx[f"x_hat_{tag}"])
    src = xc.cpu()[:, :, ::step]
    d_psnr = abs(psnr(x_hat[:, :, ::step], src) - psnr(ref, src))
    rel = abs(size - float(fx[f"size_{tag}"])) / float(fx[f"size_{tag}"])
    rate = size / (xc.shape[2] * xc.shape[3])
    print(f"icip2023 {tag}: max|d x_hat|={(x_hat[:, :, ::step] - ref).abs().max():.3e} dPSNR={d_psnr:.2e} size rel={rel:.2e}")
    assert d_psnr < PSNR_TOL_DB and rel < 2e-3
    assert abs(rate - float(fx[f"rate_{tag}"])) / float(fx[f"rate_{tag}"]) < 2e-3
    # forward() is the same pass without trace and forcing: equal to it bit for bit when nothing was forced
    with torch.no_grad():
        out = prod(x1, x2, xc, s)
    assert set(out) >= {"x_hat", "size", "rate", "size_offset", "size_residual"}
    if not any(flips.values()):
        assert torch.equal(out["x_hat"].cpu(), x_hat) and abs(out["size"].item() - size) / size < 1e-6
    assert abs(out["rate"].item() - out["size"].item() / (xc.shape[2] * xc.shape[3])) / out["rate"].item() < 1e-6


def test_batch_of_two_equals_two_single_passes(dev, prod, frames):
    x1, x2, xc = frames
    with torch.no_grad():
        a = prod(x1, x2, xc, 2.5)
        b = prod(x2.flip(-1), x1.flip(-1), xc.flip(-1), 2.5)
        both = prod(torch.cat([x1, x2.flip(-1)]), torch.cat([x2, x1.flip(-1)]), torch.cat([xc, xc.flip(-1)]), 2.5)
    assert torch.equal(both["x_hat"][0:1], a["x_hat"]) and torch.equal(both["x_hat"][1:2], b["x_hat"])
    assert not torch.equal(a["x_hat"], b["x_hat"].flip(-1))
    assert abs(both["size"].item() - a["size"].item() - b["size"].item()) / both["size"].item() < 1e-6


def test_cached_reference_features_equal_recomputation(dev, prod, frames):
    from vcamd import hip
    from vcamd.layers import BitCounter
    x1, x2, xc = frames
    t1, t2, tc = (hip.nchw_to_nhwc(x) for x in (x1, x2, xc))
    with torch.no_grad():
        f1, f2 = prod.feature_extractor.run(t1), prod.feature_extractor.run(t2)
        b1, b2 = BitCounter(dev, max_rows=12), BitCounter(dev, max_rows=12)
        a = hip.nhwc_to_nchw(prod.forward_device(t1, t2, tc, 1, b1))
        b = hip.nhwc_to_nchw(prod.forward_device(t1, t2, tc, 1, b2, feats1=[f1], feats2=[f2]))
    assert torch.equal(a, b) and torch.equal(b1.totals(), b2.totals())


def test_rejects_cpu_tensors_and_unpadded_frames(dev, prod):
    from vcamd import hip
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(hip.VcError):
        prod(x, x, x, 1)
    y = torch.zeros(1, 3, 72, 64, device=dev)
    with pytest.raises(hip.VcError):
        prod(y, y, y, 1)
    with pytest.raises(hip.VcError):
        prod.compress(y, y, y, 1)


@pytest.fixture(scope="module")
def coded(dev, prod, frames):
    """64x128 crop, one image, and the 128x192 frames as a batch of two: each encoded once per coder"""
    x1, x2, xc = frames
    inputs = {"crop": tuple(t[..., :64, :128].contiguous() for t in (x1, x2, xc)) + (1.5,),
              "batch2": (torch.cat([x1, x2.flip(-1)]), torch.cat([x2, x1.flip(-1)]), torch.cat([xc, xc.flip(-1)]), 4.0)}
    cache = {}

    def get(name, coder):
        if (name, coder) not in cache:
            trace = {}
            with torch.no_grad():
                a1, a2, ac, s = inputs[name]
                cache[(name, coder)] = (inputs[name], prod.compress(a1, a2, ac, s, trace=trace, coder=coder), trace)
        return cache[(name, coder)]
    return get


@pytest.mark.parametrize("name", ["crop", "batch2"])
def test_bitstream_round_trip_both_coders(dev, prod, coded, name):
    """the decoder never sees the current frame and rebuilds the encoder's x_hat (and latents) bit for bit, with the host coder
    and with the device coder; the two coders' reconstructions are equal; the real size tracks the -log2 p sum"""
    (x1, x2, xc, s), host, th = coded(name, "host")
    _, devc, _ = coded(name, "device")
    n = xc.shape[0]
    assert tuple(host["shape"]) == (xc.shape[2] // 64, xc.shape[3] // 64) and "coder" not in host
    for codec in ("offset", "residual"):
        groups, z = host["strings"][codec]
        assert len(groups) == 5 and len(z) == n and all(len(g) == n and all(isinstance(b, bytes) for b in g) for g in groups)
        assert len(devc["strings"][codec]) == n and all(isinstance(b, bytes) for b in devc["strings"][codec])
    td = {}
    with torch.no_grad():
        dec_h = prod.decompress(x1, x2, host["strings"], host["shape"], s, trace=td)
        dec_d = prod.decompress(x1, x2, devc["strings"], devc["shape"], s, coder="device", waves=devc["waves"])
    assert set(dec_h) == {"x_hat"} and torch.equal(dec_h["x_hat"], host["x_hat"]) and bool(torch.isfinite(host["x_hat"]).all())
    assert torch.equal(dec_d["x_hat"], devc["x_hat"]) and torch.equal(devc["x_hat"], host["x_hat"])
    for codec in ("offset", "residual"):
        assert torch.equal(td[codec]["z_hat"], th[codec]["z_hat"])
        assert all(torch.equal(a, b) for a, b in zip(td[codec]["y_hat"], th[codec]["y_hat"]))
    est = host["size_estimate"]
    band = 2 * WORST_DEVIATION * est + FLUSH_BITS_PER_STRING * 12 * n
    print(f"icip2023 {name}: size {host['size']} bits (device coder {devc['size']}), size_estimate {est:.1f}, ratio {host['size'] / est:.5f}")
    assert abs(host["size"] - est) <= band                  # (the band is the host coder's: the device payloads carry sub-stream headers)
    assert devc["size"] == 8 * sum(len(b) for v in devc["strings"].values() for b in v)


def test_a_truncated_device_payload_is_reported_after_the_call(dev, prod, coded):
    from vcamd import hip
    (x1, x2, xc, s), out, _ = coded("crop", "device")
    cut = {"offset": out["strings"]["offset"], "residual": [out["strings"]["residual"][0][:-64]]}
    with torch.no_grad(), pytest.raises(hip.VcError):
        prod.decompress(x1, x2, cut, out["shape"], s, coder="device", waves=out["waves"])
    with pytest.raises(hip.VcError):
        prod.decompress(x1, x2, out["strings"], out["shape"], s, coder="device", waves=3)
    with pytest.raises(hip.VcError):
        prod.compress(x1, x2, xc, s, coder="gpu")
    with torch.no_grad():                               # and the device is fine afterwards
        again = prod.decompress(x1, x2, out["strings"], out["shape"], s, coder="device", waves=out["waves"])
    assert torch.equal(again["x_hat"], out["x_hat"])


def test_sequence_loop_matches_reference_fixture(dev):
    """code_sequence_icip2023 against the reference's own val_sequence_level output: 20 frames = I, I, a full hierarchical GOP-16
    and an irregular tail, ELIC intra frames"""
    from vcamd import gop as vgop, icip2023, icip2024
    from vcamd.seeding import seeded_state_dict
    sq = load_fixture("icip2023_sequence_a.npz")
    model = icip2023.DeformB()
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=int(sq["seed"])))
    model = model.to(dev).eval()
    intra = icip2024.ELIC()
    intra.load_state_dict(seeded_state_dict(intra.state_dict(), seed=int(sq["intra_seed"]), conv_gain=float(sq["intra_conv_gain"])))
    intra = intra.to(dev).eval()
    clip = [(torch.from_numpy(f.astype("float32"))[None] / 255.0).to(dev) for f in sq["clip_u8"]]
    order, typ = icip2023.get_order_typ_list(16, len(clip))
    assert order == sq["order"].tolist() and "".join(typ) == str(sq["typ"])
    with torch.no_grad():
        ps, size = vgop.code_sequence_icip2023(model, [intra] * 5, lambda i: clip[i], len(clip), int(sq["level"]))
        ps_n, size_n = vgop.code_sequence_icip2023(model, [intra] * 5, lambda i: clip[i], len(clip), int(sq["level"]), cache_features=False)
    assert ps == ps_n and size == size_n                      # cached features change nothing
    d_psnr = max(abs(a - b) for a, b in zip(ps, sq["psnr"].tolist()))
    rel = max(abs(a - b) / b for a, b in zip(size, sq["size"].tolist()))
    early = sq["order"].tolist()[:6]
    d_early = max(abs(ps[o] - sq["psnr"][o]) for o in early)
    print(f"icip2023 sequence loop: max dPSNR={d_psnr:.2e} dB (first six coded frames {d_early:.2e}), max size rel={rel:.2e} over {len(clip)} frames")
    assert d_psnr < 2e-2 and rel < 5e-3                       # decoding errors compound down the hierarchy
    assert d_early < 1e-3
    # msssim=: a third list, the device-side MS-SSIM of the same crops (192x256: the smallest size five scales allow is above 160)
    g = torch.Generator().manual_seed(3)
    base = torch.nn.functional.avg_pool2d(torch.rand(1, 3, 200, 264, generator=g), 5, 1, 2)
    big = [base[:, :, 2 * t:2 * t + 192, 3 * t:3 * t + 256].contiguous().to(dev) for t in range(3)]
    with torch.no_grad():
        p3, s3, m3 = vgop.code_sequence_icip2023(model, [intra] * 5, lambda i: big[i], 3, 1, h=192, w=256, msssim=True)
        p2, s2 = vgop.code_sequence_icip2023(model, [intra] * 5, lambda i: big[i], 3, 1, h=192, w=256)
    assert p3 == p2 and s3 == s2 and len(m3) == 3 and all(v == v and abs(v) <= 1.0 for v in m3)


def test_full_size_properties_1080p(dev, prod):
    """one frame at 1088x1920, no fixture: the rate rows add up to size, rate = size / pixels, the output is finite"""
    from vcamd import hip
    from vcamd.layers import BitCounter
    g = torch.Generator().manual_seed(11)
    base = torch.nn.functional.avg_pool2d(torch.rand(1, 3, 1088 + 32, 1920 + 32, generator=g), 7, 1, 3)
    fr = [(base[:, :, 2 * t:2 * t + 1088, 3 * t:3 * t + 1920] + 0.01 * torch.randn(1, 3, 1088, 1920, generator=g)).clamp(0, 1).to(dev)
          for t in range(3)]
    with torch.no_grad():
        a = prod(fr[0], fr[2], fr[1], 2)
        bits = BitCounter(dev, max_rows=12)
        again = hip.nhwc_to_nchw(prod.forward_device(hip.nchw_to_nhwc(fr[0]), hip.nchw_to_nhwc(fr[2]), hip.nchw_to_nhwc(fr[1]), 2, bits))
    rows = bits.totals()
    assert rows.numel() == 12 and torch.equal(again, a["x_hat"])
    assert abs(rows.sum().item() - a["size"].item()) / a["size"].item() < 1e-6
    assert abs((a["size_offset"] + a["size_residual"]).item() - a["size"].item()) / a["size"].item() < 1e-6
    assert abs(a["rate"].item() - a["size"].item() / (1088 * 1920)) / a["rate"].item() < 1e-6
    assert a["x_hat"].shape == fr[1].shape and bool(torch.isfinite(a["x_hat"]).all()) and a["size"].item() > 0
