"""-m gpu: the device-side coder of the ICIP2024 B-frame bitstream (FlowGuidedB.compress / decompress with coder="device",
_Elic.compress_t / decompress_t on uploaded payloads, the VCID container) on the seeded checkpoint and the frame sizes of
tests/test_icip2024_bitstream_gpu.py: the decoder rebuilds the encoder's x_hat bit for bit, the payloads hold the integers of the
host-coded strings, x_hat is that of the host-coded path, and the decode is launches only (torch's sync debug mode)."""
import numpy as np
import pytest
import torch

from test_icip2024_bitstream_gpu import _case_inputs

pytestmark = pytest.mark.gpu

CASES = ["crop_dr1", "crop_dr16", "a", "batch2"]           # 64x128 at down_ratio 1 and 16, 128x192, a batch of two


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def prod(dev):
    from vcamd import icip2024
    from vcamd.seeding import seeded_state_dict
    m = icip2024.FlowGuidedB()
    m.load_state_dict(seeded_state_dict(m.state_dict(), seed=1234))
    m = m.to(dev).eval()
    m.offset_compressor.update(force=True)
    m.residual_compressor.update(force=True)
    return m


@pytest.fixture(scope="module")
def coded(dev, prod):
    """every case is encoded once per coder (with its trace) and shared by the tests"""
    cache = {}

    def get(name, coder, waves=4):
        key = (name, coder, waves)
        if key not in cache:
            trace = {}
            with torch.no_grad():
                out = prod.compress(*_case_inputs(name, dev), trace=trace, coder=coder, waves=waves)
            cache[key] = (out, trace)
        return cache[key]
    return get


@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("name", CASES)
def test_decoder_rebuilds_the_encoder(dev, prod, coded, name, waves):
    x1, x2, s1, s2, xc, lvl, dr = _case_inputs(name, dev)
    out, te = coded(name, "device", waves)
    n = xc.shape[0]
    assert out["coder"] == "device" and out["waves"] == waves and out["down_ratio"] == dr
    assert set(out["strings"]) == {"offset", "residual"} and all(len(v) == n and all(isinstance(b, bytes) for b in v) for v in out["strings"].values())
    assert out["size"] == 8 * sum(len(b) for v in out["strings"].values() for b in v)
    td = {}
    with torch.no_grad():
        dec = prod.decompress(x1, x2, s1, s2, out["strings"], out["shape"], lvl, dr, trace=td, coder="device", waves=waves)
    assert set(dec) == {"x_hat"} and torch.equal(dec["x_hat"], out["x_hat"])
    for codec in ("offset", "residual"):
        assert torch.equal(td[codec]["z_hat"], te[codec]["z_hat"])
        assert all(torch.equal(a, b) for a, b in zip(td[codec]["y_hat"], te[codec]["y_hat"]))
    # the host-coded path of the same arguments: the same reconstruction, bit for bit
    host, _ = coded(name, "host")
    assert torch.equal(out["x_hat"], host["x_hat"]) and "coder" not in host


@pytest.mark.parametrize("name", CASES)
def test_payloads_hold_the_symbols_of_the_host_coded_strings(dev, prod, coded, name):
    from vcamd import hip
    host, th = coded(name, "host")
    for waves in (1, 4):
        out, td = coded(name, "device", waves)
        for codec, comp in (("offset", prod.offset_compressor), ("residual", prod.residual_compressor)):
            sets = [comp.entropy_bottleneck.tables(), comp.gaussian_conditional.tables()]
            seg_d = [(s.cpu().numpy(), i.cpu().numpy()) for s, i in td[codec]["coded"]]
            seg_h = [(s.cpu().numpy(), i.cpu().numpy()) for s, i in th[codec]["coded"]]
            groups, z = host["strings"][codec]
            for j, payload in enumerate(out["strings"][codec]):
                got = hip.irans_decode_host(payload, [(i[j], int(k > 0)) for k, (_, i) in enumerate(seg_d)], sets, waves)
                # what the host-coded strings of the same call decode to: z, then per group its two passes
                want = [hip.rans_decode(z[j], seg_h[0][1][j], *sets[0])]
                for g in range(5):
                    both = hip.rans_decode(groups[g][j], np.concatenate([seg_h[1 + 2 * g][1][j], seg_h[2 + 2 * g][1][j]]), *sets[1])
                    cut = seg_h[1 + 2 * g][1][j].size
                    want += [both[:cut], both[cut:]]
                assert len(got) == len(want) == 11 and all(np.array_equal(a, b) for a, b in zip(got, want)), f"{codec} image {j}"
                assert all(np.array_equal(a, s[j]) for a, (s, _) in zip(got, seg_d))


def test_container_round_trip_and_magics(dev, prod, coded):
    from vcamd import bitstream, hip
    x1, x2, s1, s2, xc, lvl, dr = _case_inputs("batch2", dev)
    out, _ = coded("batch2", "device", 4)
    host, _ = coded("batch2", "host")
    c1, c2 = prod.convert_scales(s1, s2)
    back = []
    for j in range(xc.shape[0]):
        blob = bitstream.pack_icip2024_frame_dev(out["strings"], out["shape"], dr, lvl, c1, c2, out["waves"], image=j)
        got = bitstream.unpack_icip2024_frame_dev(blob)
        assert got["waves"] == 4 and got["shape"] == tuple(out["shape"]) and got["down_ratio"] == dr
        assert (got["s"], got["scale1"], got["scale2"]) == (lvl, c1, c2)
        assert got["strings"] == {c: [out["strings"][c][j]] for c in ("offset", "residual")}
        assert len(blob) == 31 + sum(len(out["strings"][c][j]) for c in ("offset", "residual"))
        with pytest.raises(hip.VcError):
            bitstream.unpack_icip2024_frame(blob)                      # each reader refuses the other's magic
        with pytest.raises(hip.VcError):
            bitstream.unpack_icip2024_frame_dev(bitstream.pack_icip2024_frame(host["strings"], host["shape"], dr, lvl, c1, c2, image=j))
        for bad in (blob[:30], blob[:-4], blob + b"\0\0\0\0", blob[:22] + b"\x03" + blob[23:], blob[:4] + b"\x02" + blob[5:]):
            with pytest.raises(hip.VcError):
                bitstream.unpack_icip2024_frame_dev(bad)
        back.append(got)
    strings = {c: [b["strings"][c][0] for b in back] for c in ("offset", "residual")}
    with torch.no_grad():
        dec = prod.decompress(x1, x2, back[0]["scale1"], back[0]["scale2"], strings, back[0]["shape"], back[0]["s"], back[0]["down_ratio"],
                              coder="device", waves=back[0]["waves"])
    assert torch.equal(dec["x_hat"], out["x_hat"])


def test_decode_is_launches_only(dev, prod, coded):
    """from after the upload until x_hat is enqueued nothing synchronises: torch raises on any synchronising call in this mode
    (a first decode of the shape has run before: packing weights and tuning tile configurations happen once per shape)"""
    x1, x2, s1, s2, xc, lvl, dr = _case_inputs("crop_dr1", dev)
    out, _ = coded("crop_dr1", "device", 4)
    with torch.no_grad():
        prod.decompress(x1, x2, s1, s2, out["strings"], out["shape"], lvl, dr, coder="device", waves=4)
        decoders = prod.upload_payloads(out["strings"], 4)
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            dec = prod.decompress(x1, x2, s1, s2, decoders, out["shape"], lvl, dr, coder="device", waves=4)
        finally:
            torch.cuda.set_sync_debug_mode(before)
    for d in decoders.values():
        d.finish()
    assert torch.equal(dec["x_hat"], out["x_hat"])


def test_a_corrupt_payload_is_reported_after_the_reconstruction(dev, prod, coded):
    from vcamd import hip
    x1, x2, s1, s2, xc, lvl, dr = _case_inputs("crop_dr1", dev)
    out, _ = coded("crop_dr1", "device", 4)
    cut = {"offset": out["strings"]["offset"], "residual": [out["strings"]["residual"][0][:-64]]}
    with torch.no_grad(), pytest.raises(hip.VcError):
        prod.decompress(x1, x2, s1, s2, cut, out["shape"], lvl, dr, coder="device", waves=4)
    with pytest.raises(hip.VcError):
        prod.decompress(x1, x2, s1, s2, out["strings"], out["shape"], lvl, dr, coder="device", waves=3)
    with pytest.raises(hip.VcError):
        prod.compress(x1, x2, s1, s2, xc, lvl, dr, coder="gpu")
