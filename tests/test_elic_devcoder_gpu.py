"""-m gpu: the ELIC intra codec with the interleaved coder on the device (vcamd/icip2024.py: ELIC.compress / decompress with
coder="device") against its own trace, the host reference coder and the host-coded path of the same class.

Cases: the image of icip2024_elic_codec_a.npz and a batch of two different 128x192 crops of the bundled frames.

Size band (test_size_tracks_the_estimate): the rule of tests/test_icip2024_bitstream_gpu.py -- twice the worst MEASURED deviation
of size / "bits" from 1, plus the payload's fixed overhead W * 516 bytes per image.  Measured on an MI355X (seeded weights):

    case      frame(s)        size (bits)   "bits" (estimate)   size / estimate   (size - overhead) / estimate
    fixture   1 x 128x192        72 896          68 874.5           1.05839               0.81865
    batch2    2 x 128x192       156 896         149 636.9           1.04851               0.82782

Worst deviation of size / estimate from 1: 0.05839 (fixture), so the bound is 0.11678 * estimate + W * 516 * 8 bits per image.
"""
import numpy as np
import pytest
import torch

from helpers import load_fixture, frame_tensor
from vcamd import hip

pytestmark = pytest.mark.gpu

WAVES = 4
WORST_DEVIATION = 0.05839        # the table above


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return load_fixture("icip2024_elic_codec_a.npz")


@pytest.fixture(scope="module")
def prod(dev, fx):
    from vcamd import icip2024
    from vcamd.seeding import seeded_state_dict
    m = icip2024.ELIC()
    m.load_state_dict(seeded_state_dict(m.state_dict(), seed=int(fx["seed"]), conv_gain=float(fx["conv_gain"])))
    m = m.to(dev).eval()
    m.update(force=True)
    return m


def _inputs(name, fx, dev):
    if name == "fixture":
        return frame_tensor(fx["current"]).to(dev)
    import os
    from helpers import GOLDEN
    from vcamd.data import read_png
    a = read_png(os.path.join(GOLDEN, "frames", "current.png"))
    b = read_png(os.path.join(GOLDEN, "frames", "ref_1.png"))
    return torch.cat([frame_tensor(a[:128, :192]), frame_tensor(b[64:192, 32:224])]).to(dev)


CASES = ("fixture", "batch2")


@pytest.fixture(scope="module")
def coded(dev, prod, fx):
    """per case: (x, device-coded result, its trace, host-coded result, host decode of it) -- computed once, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            x = _inputs(name, fx, dev)
            trace = {}
            with torch.no_grad():
                out = prod.compress(x, coder="device", waves=WAVES, trace=trace)
                host = [prod.compress(x[j:j + 1]) for j in range(x.shape[0])]
                host_dec = [prod.decompress(h["strings"], h["shape"]) for h in host]
            cache[name] = (x, out, trace, host, host_dec)
        return cache[name]
    return get


@pytest.mark.parametrize("name", CASES)
def test_round_trip_rebuilds_the_encoders_trace(prod, coded, name):
    x, out, trace, _, _ = coded(name)
    assert len(out["strings"]) == x.shape[0] and tuple(out["shape"]) == (x.shape[2] // 64, x.shape[3] // 64)
    back = {}
    with torch.no_grad():
        dec = prod.decompress(out["strings"], out["shape"], coder="device", waves=WAVES, trace=back)
    assert torch.equal(back["z_hat"], trace["z_hat"]) and torch.equal(back["x_hat"], trace["x_hat"])
    assert len(back["y_hat"]) == 5
    for a, b, c, d in zip(back["y_hat"], trace["y_hat"], dec["y_hat"], out["y_hat"]):
        assert torch.equal(a, b) and torch.equal(c, d) and torch.equal(a, c)
    assert torch.equal(dec["x_hat"], out["x_hat"]) and torch.equal(out["x_hat"], trace["x_hat"])


@pytest.mark.parametrize("name", CASES)
def test_payload_is_the_host_reference_coding_of_the_trace(prod, coded, name):
    x, out, trace, _, _ = coded(name)
    sets = [prod.entropy_bottleneck.tables(), prod.gaussian_conditional.tables()]
    assert len(trace["coded"]) == 11
    host = [(sym.cpu().numpy(), idx.cpu().numpy()) for sym, idx in trace["coded"]]
    for j in range(x.shape[0]):
        segments = [(sym[j], idx[j], 0 if k == 0 else 1) for k, (sym, idx) in enumerate(host)]
        assert hip.irans_encode_host(segments, sets, WAVES) == out["strings"][j]


@pytest.mark.parametrize("name", CASES)
def test_integers_are_the_squeezed_symbols_of_the_host_coded_path(prod, coded, name):
    """the payload decoded on the host (indexes of the trace) = what the host-coded compress put into its strings: z, then per group
    anchors | non-anchors"""
    x, out, trace, host, _ = coded(name)
    sets = [prod.entropy_bottleneck.tables(), prod.gaussian_conditional.tables()]
    idx = [i.cpu().numpy() for _, i in trace["coded"]]
    for j in range(x.shape[0]):
        ints = hip.irans_decode_host(out["strings"][j], [(ix[j], 0 if k == 0 else 1) for k, ix in enumerate(idx)], sets, WAVES)
        groups, z = host[j]["strings"]
        assert np.array_equal(ints[0], hip.rans_decode(z[0], idx[0][j], *sets[0]))
        for g in range(5):
            gi = np.concatenate([idx[1 + 2 * g][j], idx[2 + 2 * g][j]])
            want = hip.rans_decode(groups[g][0], gi, *sets[1])
            assert np.array_equal(np.concatenate([ints[1 + 2 * g], ints[2 + 2 * g]]), want), g


@pytest.mark.parametrize("name", CASES)
def test_reconstruction_equals_the_host_paths(prod, coded, name):
    x, out, _, host, host_dec = coded(name)
    for j in range(x.shape[0]):
        for g in range(5):
            assert torch.equal(out["y_hat"][g][j:j + 1], host_dec[j]["y_hat"][g]), (j, g)
        assert torch.equal(out["x_hat"][j:j + 1], host_dec[j]["x_hat"]), j


def test_host_coded_batch_is_one_string_per_group_for_the_whole_call(prod, coded):
    """the host-coded format of a batch: one z string per image, ONE string per group for the call -- the anchor integers of all
    images in [n][c][h][w/2] order, then the non-anchor integers likewise; decoding it rebuilds the single-image decodes"""
    x, _, trace, host, host_dec = coded("batch2")
    with torch.no_grad():
        both = prod.compress(x)
        dec = prod.decompress(both["strings"], both["shape"])
    groups, z = both["strings"]
    assert list(z) == [h["strings"][1][0] for h in host] and isinstance(both["shape"], torch.Size)
    tables = prod.gaussian_conditional.tables()
    passes = [(sym.cpu().numpy(), idx.cpu().numpy()) for sym, idx in trace["coded"][1:]]
    assert len(groups) == 5
    for g in range(5):
        (sa, ia), (sn, in_) = passes[2 * g], passes[2 * g + 1]
        want = hip.rans_encode(np.concatenate([sa.reshape(-1), sn.reshape(-1)]), np.concatenate([ia.reshape(-1), in_.reshape(-1)]), *tables)
        assert list(groups[g]) == [want], g
    for g in range(5):
        assert torch.equal(dec["y_hat"][g], torch.cat([d["y_hat"][g] for d in host_dec])), g
    assert torch.equal(dec["x_hat"], torch.cat([d["x_hat"] for d in host_dec]))


def test_encode_and_decode_do_not_synchronise_early(dev, prod, coded):
    """torch raises on any synchronising call in this mode: the encoder runs up to the collection of the payloads (the launch of
    the coder included) and the decoder from after the upload to x_hat without one (a first pass of the shape has run before:
    packing weights and tuning happen once per shape)"""
    x, out, _, _, _ = coded("batch2")
    real_collect = hip.irans_encode_collect
    seen = {}

    def collect(jobs):                         # the first and only synchronisation of the encoder
        seen["mode"] = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode(before)
        return real_collect(jobs)
    before = torch.cuda.get_sync_debug_mode()
    with torch.no_grad():
        hip.irans_encode_collect = collect
        torch.cuda.set_sync_debug_mode("error")
        try:
            again = prod.compress(x, coder="device", waves=WAVES)
        finally:
            torch.cuda.set_sync_debug_mode(before)
            hip.irans_encode_collect = real_collect
        assert seen and again["strings"] == out["strings"]
        decoder = hip.IransDecoder(out["strings"], WAVES, dev)
        torch.cuda.set_sync_debug_mode("error")
        try:
            dec = prod.decompress(decoder, out["shape"], coder="device", waves=WAVES)
        finally:
            torch.cuda.set_sync_debug_mode(before)
    decoder.finish()
    assert torch.equal(dec["x_hat"], out["x_hat"])


@pytest.mark.parametrize("name", CASES)
def test_size_tracks_the_estimate(coded, name):
    x, out, _, _, _ = coded(name)
    size = 8 * sum(len(p) for p in out["strings"])
    estimate = float(out["bits"].item())
    overhead = x.shape[0] * WAVES * hip.IRANS_SUBSTREAM_HEADER * 8
    print(f"ELIC device coder, {name}: size {size} bits, estimate {estimate:.1f} bits, size/estimate {size / estimate:.5f}, "
          f"(size - overhead)/estimate {(size - overhead) / estimate:.5f}")
    assert abs(size - estimate) <= 2 * WORST_DEVIATION * estimate + overhead


def test_a_corrupt_payload_raises_at_finish(dev, prod, coded):
    x, out, _, _, _ = coded("fixture")
    cut = [out["strings"][0][:-64]]
    with torch.no_grad():
        with pytest.raises(hip.VcError):
            prod.decompress(cut, out["shape"], coder="device", waves=WAVES)
        decoder = hip.IransDecoder(cut, WAVES, dev)
        prod.decompress(decoder, out["shape"], coder="device", waves=WAVES)      # launches only: nothing is raised here
        with pytest.raises(hip.VcError):
            decoder.finish()


def test_the_other_coders_strings_are_refused_by_name(prod, coded):
    x, out, _, host, _ = coded("fixture")
    with torch.no_grad():
        with pytest.raises(hip.VcError, match="host-coded"):
            prod.decompress(host[0]["strings"], host[0]["shape"], coder="device", waves=WAVES)
        with pytest.raises(hip.VcError, match='coder="device"'):
            prod.decompress(out["strings"], out["shape"])
        with pytest.raises(hip.VcError):
            prod.compress(x, coder="gpu")
        with pytest.raises(hip.VcError):
            prod.decompress(out["strings"], out["shape"], coder="device", waves=3)
