"""-m gpu: the ICIP2024 sequence codec (vcamd/sequence.py: Icip2024SequenceCodec; VCSQ file of vcamd/bitstream.py) end to end on a
synthetic clip: shifted 64x128 crops of the bundled frame, seeded weights.

(n_frames, intra_size) = (5, 16) and (7, 16): icip2024.get_order_typ_list follows the reference's GOP-16 order and names frames past
the end of the sequence for intra_size below 16 -- (4, 5) gives [0, 16, 8, 4, 12] -- so such pairs are refused by
bitstream.sequence_plan (tests/test_sequence_container_cpu.py).  Both pairs used here end in the irregular tail the function builds
for a sequence shorter than a GOP: (5, 16) codes 0, 4, 3, 2, 1 and (7, 16) codes 0, 6, 5, 4, 3, 2, 1, every B-frame from the two
nearest decoded frames, whichever they are."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from vcamd import bitstream, hip, icip2024

pytestmark = pytest.mark.gpu

H, W, LEVEL, SEED = 64, 128, 2.0, 1234
CASES = ((5, 16), (7, 16))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def clip():
    """seven uint8 [64,128,3] frames: a window that moves 3 px right and 2 px down per frame"""
    from vcamd.data import read_png
    rgb = read_png(os.path.join(GOLDEN, "frames", "current.png"))
    return [np.ascontiguousarray(rgb[300 + 2 * k:300 + 2 * k + H, 600 + 3 * k:600 + 3 * k + W]) for k in range(7)]


@pytest.fixture(scope="module")
def codec(dev):
    from vcamd import sequence
    model, intra = sequence.load_models(seeded=SEED, device=dev)
    return sequence.Icip2024SequenceCodec(model, intra, waves=4, intra_quality=3)


@pytest.fixture(scope="module")
def coded(dev, codec, clip):
    """per case (data, the encoder's reconstructions, the report, the decoded frames): computed once, never modified"""
    cache = {}

    def get(n_frames, intra_size):
        if (n_frames, intra_size) not in cache:
            def load(i):
                return hip.frame_from_uint8(torch.from_numpy(clip[i]).to(dev))
            with torch.no_grad():
                data, recon = codec.encode(load, n_frames, LEVEL, H, W, intra_size=intra_size)
                report = codec.report
                frames = codec.decode(data)                            # nothing but the bytes and the two models
            cache[(n_frames, intra_size)] = (data, recon, report, frames)
        return cache[(n_frames, intra_size)]
    return get


@pytest.mark.parametrize("n_frames,intra_size", CASES)
def test_decode_rebuilds_the_encoders_reconstructions(coded, n_frames, intra_size):
    data, recon, report, frames = coded(n_frames, intra_size)
    assert sorted(frames) == sorted(recon) == list(range(n_frames))
    for order in range(n_frames):
        assert tuple(frames[order].shape) == (1, 3, H, W) and torch.equal(frames[order], recon[order]), order
    assert sorted(report["size_bits"]) == sorted(report["estimate_bits"]) == list(range(n_frames))


@pytest.mark.parametrize("n_frames,intra_size", CASES)
def test_file_layout(coded, n_frames, intra_size):
    data, _, report, _ = coded(n_frames, intra_size)
    seq = bitstream.unpack_sequence(data)
    assert (seq["family"], seq["width"], seq["height"], seq["frames"], seq["intra_size"], seq["s"], seq["intra_quality"]) == \
        (1, W, H, n_frames, intra_size, LEVEL, 3)
    assert len(data) == bitstream.SEQUENCE_HEADER.size + sum(bitstream.SEQUENCE_RECORD.size + len(b) for _, _, b in seq["records"])
    order, typ = icip2024.get_order_typ_list(intra_size, n_frames)
    assert [o for _, o, _ in seq["records"]] == order and [t for t, _, _ in seq["records"]] == [typ[o] for o in order]
    for t, o, blob in seq["records"]:
        assert blob[:4] == (b"VCII" if t == "I" else b"VCID") and report["size_bits"][o] == 8 * len(blob)


def test_a_flipped_payload_byte_raises_and_leaves_the_frames_before_it(codec, coded):
    """the low byte of the first sub-stream's word count of the LAST coded frame's first payload: the header walk of that payload
    fails (deterministically: the counts no longer add up to the length), every earlier frame is decoded as before"""
    data, recon, _, _ = coded(5, 16)
    seq = bitstream.unpack_sequence(data)
    typ, last, blob = seq["records"][-1]
    assert typ == "B"
    at = len(data) - len(blob) + 31                                    # VCID: 31 header bytes, then the offset payload
    bad = data[:at] + bytes([data[at] ^ 0xff]) + data[at + 1:]
    frames = {}
    with torch.no_grad(), pytest.raises(hip.VcError):
        codec.decode(bad, frames=frames)
    assert sorted(frames) == list(range(5))                            # everything was enqueued before the one read
    for _, order, _ in seq["records"][:-1]:
        assert torch.equal(frames[order], recon[order]), order
    with pytest.raises(hip.VcError):                                   # another I-frame model: refused before anything runs
        type(codec)(codec.model, codec.i_model, waves=4, intra_quality=2).decode(data)


def test_cli_round_trip(tmp_path, clip, codec, coded, monkeypatch):
    """encode_seq / decode_seq through cli.main: argument parsing, the PNG folder in name order, the file, the PNGs of the unpadded
    crops.  The subcommands get the module's models in place of a fresh load (loading and packing two more pairs of seeded models
    would be most of this test's time; sequence.load_models itself built the ones handed over)."""
    from vcamd import cli, sequence
    from vcamd.data import read_png, write_synthetic_sequences
    asked = []
    monkeypatch.setattr(sequence, "load_models", lambda *a, **k: asked.append(a) or (codec.model, codec.i_model))
    n = 5
    write_synthetic_sequences(str(tmp_path), [clip[:n]], names=["in"])
    out_bin, out_dir = str(tmp_path / "clip.vcsq"), str(tmp_path / "out")
    blob = cli.main(["encode_seq", "--frames", str(tmp_path / "in"), "--out", out_bin, "--level", str(LEVEL), "--intra_size", "16",
                     "--seeded", str(SEED), "--i_qual", "3"])
    data, _, _, frames = coded(5, 16)
    assert blob == data and open(out_bin, "rb").read() == data         # the same models, frames and level: the same file
    cli.main(["decode_seq", "--bin", out_bin, "--out", out_dir, "--seeded", str(SEED), "--i_qual", "3"])
    names = sorted(os.listdir(out_dir))
    assert names == [f"im{k + 1:05d}.png" for k in range(n)]
    for k, name in enumerate(names):
        assert np.array_equal(read_png(os.path.join(out_dir, name)), sequence.crop_uint8(frames[k], H, W)), k
    assert [a[0] for a in asked] == [SEED, SEED]                       # both subcommands asked for the seeded checkpoints
