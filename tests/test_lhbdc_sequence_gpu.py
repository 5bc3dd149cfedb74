"""-m gpu: the LHBDC sequence codec (vcamd/sequence.py: LhbdcSequenceCodec; VCLS file of vcamd/containers.py) end to end on a
synthetic 192x256 clip with seeded checkpoints: device-coded mbt2018_mean I-frames against the host-coded path, the file against the
encoder's reconstructions, and the decoded picture hash -- a damaged stored hash and a decoder whose model differs from the
encoder's both end in a VcError that names the first bad frame, where the entropy decode alone reports nothing.  All comparisons
are exact.

N = 19 is two GOPs that share I(8), plus two tail I-frames: coding order 0, 8, 4, 2, 6, 1, 3, 5, 7, 16, 12, 10, 14, 9, 11, 13, 15,
17, 18.  N = 9 is the one-GOP file the payload-damage and command-line tests share."""
import os
import re
import struct

import numpy as np
import pytest
import torch

from vcamd import containers, hip

pytestmark = pytest.mark.gpu

H, W, SEED, LMBDA, I_QUAL = 192, 256, 1234, 1626, 7
HEADER = 19
M64 = 0xffffffffffffffff


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def clip():
    """19 uint8 [192,256,3] frames: a window that moves 2 px per frame over a smooth random picture"""
    g = torch.Generator().manual_seed(5)
    base = torch.nn.functional.avg_pool2d(torch.rand(1, 3, H + 8, W + 48, generator=g), 9, 1)
    u8 = (base[0].permute(1, 2, 0) * 255.0).round().to(torch.uint8).numpy()
    return [np.ascontiguousarray(u8[:H, 2 * i:2 * i + W]) for i in range(19)]


@pytest.fixture(scope="module")
def models(dev):
    from vcamd import sequence
    return sequence.load_lhbdc_models(seeded=SEED, i_qual=I_QUAL, lmbda=LMBDA, device=dev)


@pytest.fixture(scope="module")
def codec(models):
    from vcamd import sequence
    return sequence.LhbdcSequenceCodec(*models, lmbda=LMBDA, waves=4, intra_quality=I_QUAL)


def _loader(clip, dev):
    return lambda i: hip.frame_from_uint8(torch.from_numpy(clip[i]).to(dev))


@pytest.fixture(scope="module")
def coded(dev, codec, clip):
    """per frame count (data, the encoder's reconstructions, the encoder's report, the decoded frames, the decoder's report):
    computed once, never modified"""
    cache = {}

    def get(n):
        if n not in cache:
            with torch.no_grad():
                data, recon = codec.encode(_loader(clip, dev), n, H, W)
                report = codec.report
                frames = codec.decode(data)                            # nothing but the bytes and the two models
            cache[n] = (data, recon, report, frames, codec.report)
        return cache[n]
    return get


def _perturbed(which, dev):
    """the B-model ("b") or the I-model ("i") of load_lhbdc_models(seeded=SEED) once more, loaded (load_state_dict: the packed-weight
    caches are rebuilt) from a state dict in which ONE bias element of the last layer of (residual_compressor.)g_s is moved by 1e-3"""
    from vcamd import lhbdc
    from vcamd.iframe import mbt2018_mean
    from vcamd.seeding import seeded_state_dict
    if which == "b":
        model, prefix = lhbdc.Model(), "residual_compressor.g_s."
        sd = seeded_state_dict(model.state_dict(), seed=SEED)
    else:
        model, prefix = mbt2018_mean(I_QUAL, "mse", pretrained=False), "g_s."
        sd = seeded_state_dict(model.state_dict(), seed=SEED, conv_gain=0.8)
    sd = {k: v.detach().clone() for k, v in sd.items()}
    layers = [(int(m.group(1)), k) for k in sd for m in [re.match(re.escape(prefix) + r"(\d+)\.(?:.*\.)?bias$", k)] if m]
    key = max(layers)[1]
    sd[key][0] += 1e-3
    model.load_state_dict(sd)
    for m in ([model.mv_compressor, model.residual_compressor] if which == "b" else [model]):
        m.update(force=True)
    return model.to(dev).float().eval()


# ---- the I-frame path -------------------------------------------------------------------------------------------------------
def test_device_coded_intra_frames(dev, models, clip):
    _, intra = models
    x = _loader(clip, dev)(3)
    with torch.no_grad():
        out = intra.compress(x, coder="device", waves=4)
        assert sorted(out) == ["bits", "coder", "shape", "strings", "waves", "x_hat"] and tuple(out["shape"]) == (H // 64, W // 64)
        assert len(out["strings"]) == 1 and isinstance(out["strings"][0], bytes)
        back = intra.decompress(out["strings"], out["shape"], coder="device", waves=4)
        assert torch.equal(back["x_hat"], out["x_hat"])                # the encoder's reconstruction is the decoder's, bit for bit
        assert float(out["x_hat"].min()) >= 0.0 and float(out["x_hat"].max()) <= 1.0
        dec = hip.IransDecoder(out["strings"], 4, dev)                 # an uploaded decoder in place of the bytes: the caller reads
        again = intra.decompress(dec, out["shape"], coder="device")
        containers.finish_all([dec])
        assert torch.equal(again["x_hat"], out["x_hat"])
        for waves in (1, 2):                                           # another wave count: another payload, the same picture
            o = intra.compress(x, coder="device", waves=waves)
            assert torch.equal(o["x_hat"], out["x_hat"])
            assert torch.equal(intra.decompress(o["strings"], o["shape"], coder="device", waves=waves)["x_hat"], out["x_hat"])
        # the host-coded strings of the same image hold the same integers
        host = intra.compress(x)
        assert sorted(host) == ["shape", "strings"] and tuple(host["shape"]) == tuple(out["shape"])
        eb, gc = intra.entropy_bottleneck.tables(), intra.gaussian_conditional.tables()
        hz, wz = out["shape"]
        z_idx = np.repeat(np.arange(intra.N, dtype=np.int32), hz * wz)
        z = hip.rans_decode(host["strings"][1][0], z_idx, *eb)
        _, idx_d = intra.hyper_decode_t(torch.from_numpy(z[None]).to(dev), 1, (hz, wz))
        y_idx = idx_d.cpu().numpy()[0]
        y = hip.rans_decode(host["strings"][0][0], y_idx, *gc)
        z2, y2 = hip.irans_decode_host(out["strings"][0], [(z_idx, 0), (y_idx, 1)], [eb, gc], 4)
        assert np.array_equal(z, z2) and np.array_equal(y, y2)
        # coder="host" is today's path: the same strings as compress_t, the same picture as decompress_t, and that picture is the
        # device coder's
        strings, shape = intra.compress_t(hip.nchw_to_nhwc(x.contiguous().float()))
        assert host["strings"] == strings and intra.compress(x, coder="host")["strings"] == strings and tuple(shape) == (hz, wz)
        x_host = intra.decompress(host["strings"], host["shape"])["x_hat"]
        assert torch.equal(x_host, hip.nhwc_to_nchw(intra.decompress_t(strings, shape, dev, final_act=hip.ACT_CLAMP01)))
        assert torch.equal(x_host, out["x_hat"])
        # the estimate: the entropy kernels' -log2 p sums, a 0-dim float64 device tensor, finite and positive
        bits = out["bits"]
        assert bits.dtype == torch.float64 and bits.dim() == 0 and bits.is_cuda
        print(f"I-frame: payload {8 * len(out['strings'][0])} bits, device estimate {float(bits):.1f} bits")
        assert np.isfinite(float(bits)) and float(bits) > 0.0
        for bad in ({"coder": "gpu"}, {"coder": "device", "waves": 3}):
            with pytest.raises(hip.VcError):
                intra.compress(x, **bad)
        with pytest.raises(hip.VcError):
            intra.decompress(host["strings"], host["shape"], coder="device", waves=4)
        with pytest.raises(hip.VcError):
            intra.decompress(out["strings"], out["shape"], coder="device", waves=3)


def test_intra_decode_is_launches_only(dev, models, clip):
    _, intra = models
    with torch.no_grad():
        out = intra.compress(_loader(clip, dev)(3), coder="device", waves=4)
        dec = hip.IransDecoder(out["strings"], 4, dev)
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            x_hat = intra.decompress(dec, out["shape"], coder="device")["x_hat"]
            digest = hip.picture_hash(x_hat)
        finally:
            torch.cuda.set_sync_debug_mode(before)
        dec.finish()
    assert torch.equal(x_hat, out["x_hat"])
    assert int(digest.cpu()[0]) & M64 == hip.picture_hash_host(x_hat.cpu().numpy())


# ---- the file ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [19, 1, 9])
def test_decode_rebuilds_the_encoders_reconstructions(coded, n):
    data, recon, report, frames, decoded_report = coded(n)
    assert sorted(frames) == sorted(recon) == list(range(n))
    for order in range(n):
        assert tuple(frames[order].shape) == (1, 3, H, W) and torch.equal(frames[order], recon[order]), order
    plan = containers.lhbdc_sequence_plan(n)
    intra_orders = sorted(o for o, t in plan if t == "I")
    assert sorted(report["size_bits"]) == sorted(report["hash"]) == list(range(n))
    assert sorted(report["estimate_bits"]) == intra_orders              # the device estimate exists for the I-frames alone
    assert all(np.isfinite(report["estimate_bits"][o]) and report["estimate_bits"][o] > 0.0 for o in intra_orders)
    for order in range(n):
        assert report["hash"][order] == hip.picture_hash_host(frames[order].cpu().numpy()), order
    assert decoded_report["verified"] is True and decoded_report["hash"] == report["hash"]
    # the layout
    seq = containers.unpack_lhbdc_sequence(data)
    assert (seq["flags"], seq["width"], seq["height"], seq["frames"], seq["lmbda"], seq["intra_quality"]) == (1, W, H, n, LMBDA, I_QUAL)
    assert len(data) == HEADER + sum(9 + 8 + len(b) for _, _, b in seq["records"])
    assert [(o, t) for t, o, _ in seq["records"]] == plan and seq["hashes"] == report["hash"]
    for t, o, blob in seq["records"]:
        assert blob[:4] == (b"VCLI" if t == "I" else b"VCLD") and report["size_bits"][o] == 8 * len(blob)


def test_a_codec_built_with_another_wave_count_decodes_the_file(models, coded):
    from vcamd import sequence
    data, recon, _, _, _ = coded(19)
    other = sequence.LhbdcSequenceCodec(*models, lmbda=LMBDA, waves=1, intra_quality=I_QUAL)
    with torch.no_grad():
        frames = other.decode(data)
    assert other.report["verified"] is True
    for order in range(19):
        assert torch.equal(frames[order], recon[order]), order


def _record_offsets(data):
    """{display order: (offset of the record, type, length)} of a VCLS file with hashes"""
    out, pos = {}, HEADER
    for t, o, blob in containers.unpack_lhbdc_sequence(data)["records"]:
        out[o] = (pos, t, len(blob))
        pos += 17 + len(blob)
    return out


def test_a_damaged_stored_hash_names_its_frame(codec, coded):
    data, recon, _, _, _ = coded(19)
    at = _record_offsets(data)[6][0] + 9                               # the u64 behind (type, order, length) of the record of order 6
    bad = data[:at + 3] + bytes([data[at + 3] ^ 0x10]) + data[at + 4:]
    frames = {}
    with torch.no_grad():
        with pytest.raises(hip.VcError, match=r"frame 6\b.*picture hash"):
            codec.decode(bad, frames=frames)
        assert codec.report["verified"] is False
        assert sorted(frames) == list(range(19))
        for order in range(19):                                        # (the pictures themselves are the encoder's)
            assert torch.equal(frames[order], recon[order]), order
        silent = codec.decode(bad, verify=False)
        assert codec.report == {"verified": False}
    for order in range(19):
        assert torch.equal(silent[order], recon[order]), order


def test_a_drifting_b_model_is_caught_at_the_first_b_frame(dev, models, coded):
    """no payload error -- the entropy decode never looks at the references or at g_s -- and a VcError that names frame 4, the first
    B-frame in coding order; I-frames 0 and 8 come before it and pass"""
    from vcamd import sequence
    data, recon, _, _, _ = coded(19)
    model, intra = models
    drifting = sequence.LhbdcSequenceCodec(_perturbed("b", dev), intra, lmbda=LMBDA, intra_quality=I_QUAL)
    frames = {}
    with torch.no_grad():
        with pytest.raises(hip.VcError, match=r"frame 4\b.*picture hash"):
            drifting.decode(data, frames=frames)
        assert sorted(frames) == list(range(19))
        for order in (0, 8, 16, 17, 18):                               # the I-frames are the encoder's
            assert torch.equal(frames[order], recon[order]), order
        assert not torch.equal(frames[4], recon[4])
        got = drifting.report["hash"]
        assert [o for o, _ in containers.lhbdc_sequence_plan(19) if got[o] != coded(19)[2]["hash"][o]][0] == 4
        silent = drifting.decode(data, verify=False)                   # without the hash the same decode says nothing
    assert not torch.equal(silent[4], recon[4])


def test_a_drifting_i_model_is_caught_at_frame_0(dev, models, coded):
    from vcamd import sequence
    data, recon, _, _, _ = coded(19)
    model, intra = models
    drifting = sequence.LhbdcSequenceCodec(model, _perturbed("i", dev), lmbda=LMBDA, intra_quality=I_QUAL)
    frames = {}
    with torch.no_grad(), pytest.raises(hip.VcError, match=r"frame 0\b.*picture hash"):
        drifting.decode(data, frames=frames)
    assert sorted(frames) == list(range(19)) and not torch.equal(frames[0], recon[0])


def test_format_checks_come_before_any_launch(dev, models, codec, clip, coded):
    from vcamd import sequence
    data, recon, _, _, _ = coded(9)
    with torch.no_grad():
        plain = sequence.LhbdcSequenceCodec(*models, lmbda=LMBDA, intra_quality=I_QUAL, picture_hash=False)
        unhashed, plain_recon = plain.encode(_loader(clip, dev), 9, H, W)
        assert "hash" not in plain.report and containers.unpack_lhbdc_sequence(unhashed)["hashes"] is None
        assert len(unhashed) == len(data) - 9 * 8
        frames = codec.decode(unhashed)                                # verify=True on a file without hashes is no error
        assert codec.report["verified"] is False
        for order in range(9):
            assert torch.equal(frames[order], recon[order]) and torch.equal(plain_recon[order], recon[order]), order
    others = [sequence.LhbdcSequenceCodec(*models, **{"lmbda": LMBDA, "intra_quality": I_QUAL, **kw}) for kw in ({"lmbda": 845}, {"intra_quality": 6})]
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                            # (nothing below gets as far as reading from the device)
    try:
        for other in others:
            with pytest.raises(hip.VcError):
                other.decode(data)
        offsets = _record_offsets(data)
        at = offsets[4][0] + 17 + 6                                    # the lambda of the VCLD record of order 4
        with pytest.raises(hip.VcError, match="lambda"):
            codec.decode(data[:at] + struct.pack("<I", 845) + data[at + 4:])
        at = offsets[8][0] + 17 + 6                                    # the hyper-latent shape of the VCLI record of order 8
        with pytest.raises(hip.VcError):
            codec.decode(data[:at] + struct.pack("<HH", 4, 4) + data[at + 4:])
        at = offsets[6][0] + 17 + 5                                    # waves of order 6: its level (2, 6) no longer agrees
        with pytest.raises(hip.VcError):
            codec.decode(data[:at] + b"\x02" + data[at + 1:])
        with pytest.raises(hip.VcError):
            codec.decode(data[:-4])
        with pytest.raises(hip.VcError):
            codec.encode(lambda i: torch.zeros(1, 3, H, W + 64, device=dev), 1, H, W)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    for bad in ({"waves": 3}, {"intra_quality": 0}, {"intra_quality": 9}, {"lmbda": -1}):
        with pytest.raises(hip.VcError):
            sequence.LhbdcSequenceCodec(*models, **bad)


# Positions inside the VCLD record of order 2, relative to its two payloads (include/vc_hip.h, "Interleaved range coder": a sub-stream
# is u32 word count | 64 x u64 states | the words in the order the decoder reads them): the low byte of the first sub-stream's word
# count (the header walk fails); bits 40..47 of lane 0's initial state and bits 24..31 of the first word either payload's first
# sub-stream reads (the state behind the next step is off by a multiple of 2^24 frequencies: every later symbol of that lane is
# another one).  The words a lane reads behind its LAST symbol only feed a state nothing is decoded from -- the tail of a sub-stream
# is no place for this test.
FLIPS = (("mv", 0), ("mv", 4 + 5), ("mv", 516 + 3), ("res", 516 + 3))


@pytest.mark.parametrize("which,where", FLIPS)
def test_a_flipped_payload_byte_ends_in_vcerror(codec, coded, which, where):
    data, recon, _, _, _ = coded(9)
    start, typ, length = _record_offsets(data)[2]
    assert typ == "B"
    blob = start + 17
    n_mv, n_res = struct.unpack_from("<II", data, blob + 18)
    assert 26 + n_mv + n_res == length
    first, size = (blob + 26, n_mv) if which == "mv" else (blob + 26 + n_mv, n_res)
    assert 0 <= where < size
    at = first + where
    bad = data[:at] + bytes([data[at] ^ 0xff]) + data[at + 1:]
    frames = {}
    with torch.no_grad(), pytest.raises(hip.VcError):
        codec.decode(bad, frames=frames)
    assert sorted(frames) == list(range(9))                            # everything was enqueued before the one read
    for order in (0, 8, 4, 6):                                         # what frame 2 is not a reference of is whole
        assert torch.equal(frames[order], recon[order]), order


def test_cli_round_trip(tmp_path, clip, models, coded, monkeypatch):
    """encode_seq_lhbdc / decode_seq_lhbdc through cli.main: argument parsing, the PNG folder in name order, the file, the PNGs of
    the decoded pictures.  The subcommands get the module's models in place of a fresh load (sequence.load_lhbdc_models itself
    built the ones handed over)."""
    from vcamd import cli, sequence
    from vcamd.data import read_png, write_synthetic_sequences
    asked = []
    monkeypatch.setattr(sequence, "load_lhbdc_models", lambda *a, **k: asked.append(a) or models)
    n = 9
    write_synthetic_sequences(str(tmp_path), [clip[:n]], names=["in"])
    out_bin, out_dir = str(tmp_path / "clip.vcls"), str(tmp_path / "out")
    blob = cli.main(["encode_seq_lhbdc", "--frames", str(tmp_path / "in"), "--out", out_bin, "--seeded", str(SEED)])
    data, recon, _, _, _ = coded(n)
    assert blob == data and open(out_bin, "rb").read() == data         # the same models and frames: the same file
    cli.main(["decode_seq_lhbdc", "--bin", out_bin, "--out", out_dir, "--seeded", str(SEED)])
    names = sorted(os.listdir(out_dir))
    assert names == [f"im{k + 1:05d}.png" for k in range(n)]
    for k, name in enumerate(names):
        assert np.array_equal(read_png(os.path.join(out_dir, name)), sequence.crop_uint8(recon[k], H, W)), k
    assert [(a[0], a[3], a[4]) for a in asked] == [(SEED, I_QUAL, LMBDA)] * 2
    # the existing subcommand keeps its required --level
    with pytest.raises(SystemExit):
        cli.main(["encode_seq", "--frames", str(tmp_path / "in"), "--out", out_bin, "--seeded", str(SEED)])
    no_hash = cli.main(["encode_seq_lhbdc", "--frames", str(tmp_path / "in"), "--out", out_bin, "--seeded", str(SEED), "--no_hash"])
    assert containers.unpack_lhbdc_sequence(no_hash)["hashes"] is None
    cli.main(["decode_seq_lhbdc", "--bin", out_bin, "--out", out_dir, "--seeded", str(SEED), "--no_verify"])
