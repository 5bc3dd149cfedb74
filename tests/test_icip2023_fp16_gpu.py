"""-m gpu: the ICIP2023 DeformB family (vcamd/icip2023.py) under hip.set_conv_precision("fp16"): forward against the fp32 path of the
same build (which tests/test_icip2023_gpu.py pins to the reference), the mode being in use, the closed loop of the bitstream with
both coders, and the sequence loop.  Seeded weights, the 128x192 frames of tests/golden/icip2023_forward_a.npz.

Bounds are the project's own fp16 bounds (tests/test_fp16_gpu.py): |dPSNR| < 0.05 dB, relative size difference < 0.02.  Bit
equalities and call counts are exact.  Models are packed while fp16 is active; precision and switches are restored in ``finally``."""
import pytest
import torch

from helpers import frame_tensor, load_fixture, psnr
from test_fp16_gpu import BITS_TOL, PSNR_TOL_DB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return load_fixture("icip2023_forward_a.npz")


@pytest.fixture(scope="module")
def frames(dev, fx):
    return tuple(frame_tensor(fx[k]).to(dev) for k in ("ref_1", "ref_2", "current"))


def _model(dev, seed):
    from vcamd import icip2023
    from vcamd.seeding import seeded_state_dict
    m = icip2023.DeformB()
    m.load_state_dict(seeded_state_dict(m.state_dict(), seed=seed))
    m = m.to(dev).eval()
    m.offset_compressor.update(force=True)
    m.residual_compressor.update(force=True)
    return m


class _Fp16:
    """fp16 precision with hip.HALF_DEFORM_PAIR set as asked; both restored on exit"""

    def __init__(self, pair=True):
        self.pair = pair

    def __enter__(self):
        from vcamd import hip
        self.keep = (hip.conv_precision(), hip.HALF_DEFORM_PAIR)
        hip.set_conv_precision("fp16")
        hip.HALF_DEFORM_PAIR = self.pair

    def __exit__(self, *exc):
        from vcamd import hip
        hip.set_conv_precision(self.keep[0])
        hip.HALF_DEFORM_PAIR = self.keep[1]


@pytest.fixture(scope="module")
def fp32_out(dev, fx, frames):
    """the fp32 path of this build on the frames, computed once"""
    x1, x2, xc = frames
    with torch.no_grad():
        out = _model(dev, int(fx["seed"]))(x1, x2, xc, float(fx["s_s25"]))
    return out["x_hat"].cpu(), float(out["size"])


@pytest.fixture(scope="module")
def prod16(dev, fx, frames):
    """a model whose layers were packed while fp16 was active (models pack on first use)"""
    x1, x2, xc = frames
    with _Fp16(), torch.no_grad():
        m = _model(dev, int(fx["seed"]))
        m(x1, x2, xc, float(fx["s_s25"]))
    return m


def _packed_convs(model):
    from vcamd import hip
    found, seen = [], set()

    def walk(o, depth=0):
        if id(o) in seen or depth > 5:
            return
        seen.add(id(o))
        if isinstance(o, hip.PackedConv):
            found.append(o)
            walk(vars(o), depth + 1)
        elif isinstance(o, (list, tuple)):
            for q in o:
                walk(q, depth + 1)
        elif isinstance(o, dict):
            for q in o.values():
                walk(q, depth + 1)
    for mod in model.modules():
        for k, v in vars(mod).items():
            if k not in ("_modules", "_parameters", "_buffers"):
                walk(v)
    return found


@pytest.mark.parametrize("pair", [True, False])
def test_forward_fp16_against_fp32_path(dev, fx, frames, prod16, fp32_out, pair):
    from vcamd import hip
    x1, x2, xc = frames
    ref, size32 = fp32_out
    calls = []
    orig = hip.to_half_planar
    hip.to_half_planar = lambda t, cg: (calls.append(t.c), orig(t, cg))[1]
    try:
        with _Fp16(pair), torch.no_grad():
            out = prod16(x1, x2, xc, float(fx["s_s25"]))
    finally:
        hip.to_half_planar = orig
    src = xc.cpu()
    x16 = out["x_hat"].cpu()
    d_psnr = abs(psnr(x16, src) - psnr(ref, src))
    rel = abs(float(out["size"]) - size32) / size32
    print(f"icip2023 fp16 (HALF_DEFORM_PAIR={pair}): dPSNR={d_psnr:.4f} dB, size rel={rel:.4f}, PSNR(fp16 vs fp32 output)={psnr(x16, ref):.2f} dB, "
          f"size {float(out['size']):.1f} vs {size32:.1f}")
    assert bool(torch.isfinite(x16).all())
    assert calls == ([96, 96, 64, 64, 32, 32] if pair else [])         # levels 3, 2, 1: both references of each
    assert d_psnr < PSNR_TOL_DB and rel < BITS_TOL
    assert hip.conv_precision() == "fp32"


def test_the_mode_is_in_use(dev, prod16):
    packs = _packed_convs(prod16)
    half = [p for p in packs if p.wpk16 is not None]
    print(f"icip2023 fp16: {len(half)} of {len(packs)} PackedConv objects carry half weights")
    assert 0 < len(half) < len(packs)


def test_cached_reference_features_equal_recomputation_fp16(dev, fx, frames, prod16):
    from vcamd import hip
    from vcamd.layers import BitCounter
    t1, t2, tc = (hip.nchw_to_nhwc(x) for x in frames)
    with _Fp16(), torch.no_grad():
        f1, f2 = prod16.feature_extractor.run(t1), prod16.feature_extractor.run(t2)
        b1, b2 = BitCounter(dev, max_rows=12), BitCounter(dev, max_rows=12)
        a = hip.nhwc_to_nchw(prod16.forward_device(t1, t2, tc, 1, b1))
        b = hip.nhwc_to_nchw(prod16.forward_device(t1, t2, tc, 1, b2, feats1=[f1], feats2=[f2]))
    assert torch.equal(a, b) and torch.equal(b1.totals(), b2.totals())


def test_closed_loop_in_fp16_both_coders(dev, fx, frames, prod16):
    """the decoder rebuilds the encoder's x_hat bit for bit with the host coder and with the device coder, the two coders'
    reconstructions are equal, size is 8 x the payload bytes"""
    from vcamd.icip2024 import _flat_strings
    x1, x2, xc = frames
    s = 1.5
    got = {}
    with _Fp16(), torch.no_grad():
        for coder in ("host", "device"):
            enc = prod16.compress(x1, x2, xc, s, coder=coder)
            kw = dict(coder="device", waves=enc["waves"]) if coder == "device" else {}
            dec = prod16.decompress(x1, x2, enc["strings"], enc["shape"], s, **kw)
            assert torch.equal(dec["x_hat"], enc["x_hat"]), coder
            assert bool(torch.isfinite(enc["x_hat"]).all())
            payload = sum(len(b) for k in enc["strings"] for b in (enc["strings"][k] if coder == "device" else _flat_strings(enc["strings"][k])))
            assert enc["size"] == 8 * payload, coder
            got[coder] = enc
    assert torch.equal(got["device"]["x_hat"], got["host"]["x_hat"])
    print(f"icip2023 fp16 bitstream: host {got['host']['size']} bits, device {got['device']['size']} bits, estimate {got['host']['size_estimate']:.1f}")


def test_sequence_loop_fp16_against_fp32(dev):
    """code_sequence_icip2023 over the first 5 frames of the sequence fixture (bitstream.sequence_plan(16, 5) accepts them), models
    built and packed in each precision: per frame within the two bounds of the fp32 run of the same call"""
    from vcamd import bitstream, gop as vgop, icip2024
    from vcamd.seeding import seeded_state_dict
    sq = load_fixture("icip2023_sequence_a.npz")
    n = 5
    assert len(bitstream.sequence_plan(16, n)) == n
    clip = [(torch.from_numpy(f.astype("float32"))[None] / 255.0).to(dev) for f in sq["clip_u8"][:n]]

    def run():
        model = _model(dev, int(sq["seed"]))
        intra = icip2024.ELIC()
        intra.load_state_dict(seeded_state_dict(intra.state_dict(), seed=int(sq["intra_seed"]), conv_gain=float(sq["intra_conv_gain"])))
        intra = intra.to(dev).eval()
        with torch.no_grad():
            return vgop.code_sequence_icip2023(model, [intra] * 5, lambda i: clip[i], n, int(sq["level"]))
    ps32, size32 = run()
    with _Fp16():
        ps16, size16 = run()
    d_psnr = max(abs(a - b) for a, b in zip(ps16, ps32))
    rel = max(abs(a - b) / b for a, b in zip(size16, size32))
    print(f"icip2023 fp16 sequence loop: max dPSNR={d_psnr:.4f} dB, max size rel={rel:.4f} over {n} frames")
    assert len(ps16) == n and all(v == v for v in ps16)
    assert d_psnr < PSNR_TOL_DB and rel < BITS_TOL
