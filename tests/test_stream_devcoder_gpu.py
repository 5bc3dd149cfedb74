"""-m gpu: LhbdcStreamCodec(coder="device") (vcamd/bitstream.py) against the host-coded path on the 192x256
GOP of tests/test_stream_gpu.py: the same reconstructions, the same integers in both formats, a decoder that only launches, and
corrupt containers that end in VcError.

Size (test_size_on_the_calibrated_checkpoint).  For the GOP, VCLD bytes <= bits_B.bin bytes of the same frames + (W * 516 +
4 * 64 * W) per payload + 4 bytes per escaped symbol: the payload's stated overhead (W sub-stream headers) and its one-word-per-
lane freedom, and the format's fixed 32 bits per escaped value against the sequential coder's nibble code (which is never longer
than that plus its own escape slot).  The escaped symbols are counted from the integers and the tables' ranges."""
import numpy as np
import pytest
import torch

from helpers import lhbdc_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _model(dev, calibrated=False):
    _, prod = lhbdc_pair(1234, dev, calibrated=calibrated)
    prod.mv_compressor.update(force=True)
    prod.residual_compressor.update(force=True)
    return prod


@pytest.fixture(scope="module")
def model(dev):
    return _model(dev)


def _gop(dev, seed, h=192, w=256):
    g = torch.Generator().manual_seed(seed)
    base = torch.nn.functional.avg_pool2d(torch.rand(1, 3, h + 8, w + 24, generator=g), 9, 1)
    return [base[..., :h, 2 * i:2 * i + w].contiguous().to(dev) for i in range(9)]


@pytest.fixture(scope="module")
def coded(dev, model):
    """the GOP coded once by each coder (and at W = 1): {key: (containers, reconstructions)}"""
    from vcamd import bitstream
    frames = _gop(dev, 5)
    out = {"frames": frames}
    with torch.no_grad():
        for key, kw in (("host", {}), ("dev4", {"coder": "device", "waves": 4}), ("dev1", {"coder": "device", "waves": 1})):
            codec = bitstream.LhbdcStreamCodec(model, workers=4, **kw)
            out[key] = codec.encode_gop(frames, frames[0], frames[8])
            codec.close()
    return out


def test_both_encoders_give_the_same_reconstructions(coded):
    for key in ("dev4", "dev1"):
        containers, recon = coded[key]
        assert sorted(containers) == [1, 2, 3, 4, 5, 6, 7] and all(c[:4] == b"VCLD" for c in containers.values())
        for o in range(1, 8):
            assert torch.equal(recon[o], coded["host"][1][o]), (key, o)


@pytest.mark.parametrize("key,waves", [("dev1", 1), ("dev4", 4)])
def test_the_decoder_rebuilds_the_encoder(dev, model, coded, key, waves):
    """(the decoding codec is built with another wave count: the decoder takes W from the containers)"""
    from vcamd import bitstream
    frames = coded["frames"]
    containers, recon = coded[key]
    codec = bitstream.LhbdcStreamCodec(model, coder="device", waves=2)
    with torch.no_grad():
        decoded = codec.decode_gop(containers, frames[0], frames[8])
        for o in range(1, 8):
            assert torch.equal(decoded[o], recon[o]), o
        one = codec.decode_frames(frames[0], frames[8], [containers[4]])
        assert torch.equal(one, recon[4])
    assert bitstream.unpack_lhbdc_frame_dev(containers[4], 192, 256)["waves"] == waves


def _integers_of_both_formats(model, host_blob, dev_blob):
    """[(integers from the bits_B.bin strings, integers from the VCLD payload)] for (mv z, mv y, res z, res y); the y indexes are
    taken from a decode of the host strings on the device (they are not in either container)"""
    from vcamd import bitstream, hip, lhbdc
    _, s_mv, s_res, sh_mv, sh_res = lhbdc.read_container(host_blob)
    d = bitstream.unpack_lhbdc_frame_dev(dev_blob, 192, 256)
    out = []
    for codec, strings, shape, payload in ((model.mv_compressor, s_mv, sh_mv, d["mv"]), (model.residual_compressor, s_res, sh_res, d["res"])):
        eb, gc = codec.entropy_bottleneck.tables(), codec.gaussian_conditional.tables()
        z_idx = np.repeat(np.arange(codec.N, dtype=np.int32), int(shape[0]) * int(shape[1]))
        z = hip.rans_decode(strings[1][0], z_idx, *eb)
        _, idx_d = codec.hyper_decode_t(torch.from_numpy(z[None]).to(codec.entropy_bottleneck.quantiles.device), 1, shape)
        y_idx = idx_d.cpu().numpy()[0]
        y = hip.rans_decode(strings[0][0], y_idx, *gc)
        z2, y2 = hip.irans_decode_host(payload, [(z_idx, 0), (y_idx, 1)], [eb, gc], d["waves"])
        out.append((z, z2, y, y2, y_idx, eb, gc, z_idx))
    return out


def test_both_formats_hold_the_same_integers(model, coded):
    with torch.no_grad():
        for o in (1, 4, 6):
            for z, z2, y, y2, *_ in _integers_of_both_formats(model, coded["host"][0][o], coded["dev4"][0][o]):
                assert np.array_equal(z, z2) and np.array_equal(y, y2), o


def test_decode_is_launches_only(dev, model, coded):
    """from after the uploads until finish nothing synchronises: torch raises on any synchronising call in this mode (a first
    decode of the shapes has run before: packing weights and tuning tile configurations happen once per shape)"""
    from vcamd import bitstream
    frames = coded["frames"]
    containers, recon = coded["dev4"]
    codec = bitstream.LhbdcStreamCodec(model, coder="device")
    with torch.no_grad():
        codec.decode_gop(containers, frames[0], frames[8])
        up = codec.upload_gop(containers, frames[0])
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            decoded = codec.decode_gop(up, frames[0], frames[8], finish=False)
        finally:
            torch.cuda.set_sync_debug_mode(before)
        up.finish()
    for o in range(1, 8):
        assert torch.equal(decoded[o], recon[o]), o


def test_corrupt_containers(dev, model, coded):
    from vcamd import bitstream, hip
    frames = coded["frames"]
    containers, recon = coded["dev4"]
    dev_codec = bitstream.LhbdcStreamCodec(model, coder="device")
    host_codec = bitstream.LhbdcStreamCodec(model, workers=2)
    with torch.no_grad():
        # a payload cut short (the lengths still add up): VcError after the frames -- the GOP is enqueued to its end, nothing faults
        c = containers[2]
        n_mv, n_res = np.frombuffer(c[18:26], dtype=np.uint32)
        cut = bytearray(c[:-64])
        cut[22:26] = np.array([n_res - 64], dtype=np.uint32).tobytes()
        bad = dict(containers)
        bad[2] = bytes(cut)
        up = dev_codec.upload_gop(bad, frames[0])
        decoded = dev_codec.decode_gop(up, frames[0], frames[8], finish=False)
        assert sorted(decoded) == list(range(9)) and torch.equal(decoded[4], recon[4])      # (level 0 does not depend on frame 2)
        with pytest.raises(hip.VcError):
            up.finish()
        with pytest.raises(hip.VcError):
            dev_codec.decode_gop(bad, frames[0], frames[8])
        # refused before any launch: a flipped magic, the other coder's container (the refusal names both formats), mixed shapes
        flipped = dict(containers)
        flipped[4] = b"VCLX" + containers[4][4:]
        with pytest.raises(hip.VcError):
            dev_codec.upload_gop(flipped, frames[0])
        with pytest.raises(hip.VcError, match=r"(?s)bits_B\.bin.*VCLD|VCLD.*bits_B\.bin"):
            dev_codec.decode_gop(coded["host"][0], frames[0], frames[8])
        with pytest.raises(hip.VcError, match=r"(?s)bits_B\.bin.*VCLD|VCLD.*bits_B\.bin"):
            host_codec.decode_gop(containers, frames[0], frames[8])
        with pytest.raises(hip.VcError, match=r"(?s)bits_B\.bin.*VCLD|VCLD.*bits_B\.bin"):
            host_codec.decode_frames(frames[0], frames[8], [containers[4]])
        other = bytearray(containers[1])
        other[14:18] = np.array([3, 5], dtype=np.uint16).tobytes()                              # a residual shape of another frame size
        with pytest.raises(hip.VcError):
            dev_codec.upload_frames([containers[3], bytes(other)], frames[0])
        w1 = coded["dev1"][0]
        with pytest.raises(hip.VcError):                                                        # mixed wave counts within a level
            dev_codec.upload_frames([containers[1], w1[3]], frames[0])
        with pytest.raises(hip.VcError):
            dev_codec.decode_frames(torch.cat([frames[0], frames[0]], 0), torch.cat([frames[2], frames[2]], 0), [containers[1]])
        with pytest.raises(hip.VcError):
            bitstream.LhbdcStreamCodec(model, coder="gpu")
        with pytest.raises(hip.VcError):
            bitstream.LhbdcStreamCodec(model, coder="device", waves=3)
    host_codec.close()


def test_size_on_the_calibrated_checkpoint(dev):
    from vcamd import bitstream
    model = _model(dev, calibrated=True)
    frames = _gop(dev, 5)
    waves = 4
    with torch.no_grad():
        host = bitstream.LhbdcStreamCodec(model, workers=4)
        h_containers, h_recon = host.encode_gop(frames, frames[0], frames[8])
        host.close()
        d_containers, d_recon = bitstream.LhbdcStreamCodec(model, coder="device", waves=waves).encode_gop(frames, frames[0], frames[8])
        escaped = symbols = 0
        for o in range(1, 8):
            assert torch.equal(h_recon[o], d_recon[o])
            for z, z2, y, y2, y_idx, eb, gc, z_idx in _integers_of_both_formats(model, h_containers[o], d_containers[o]):
                assert np.array_equal(z, z2) and np.array_equal(y, y2)
                for sym, idx, (_, sizes, offs) in ((z, z_idx, eb), (y, y_idx, gc)):
                    v = sym.astype(np.int64) - offs[idx]
                    escaped += int(((v < 0) | (v >= sizes[idx] - 2)).sum())
                    symbols += sym.size
    old = sum(len(c) for c in h_containers.values())
    new = sum(len(c) for c in d_containers.values())
    bound = old + 14 * (waves * 516 + 4 * 64 * waves) + 4 * escaped
    print(f"calibrated GOP: bits_B.bin {old} bytes, VCLD {new} bytes (W = {waves}), ratio {new / old:.4f}, {escaped} escaped of {symbols} symbols, "
          f"bound {bound} bytes")
    assert new <= bound
