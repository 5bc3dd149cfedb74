"""The byte formats of vcamd/containers.py, frozen: one hand-written input per format, its header against a literal built here from
the layout tables of INTEGRATION.md (not from the module's Struct objects) and its whole blob against a SHA-256 that was recorded by
running the same input through the functions of the commit before the formats moved out of vcamd/bitstream.py.  Then the pieces the
formats share: every reader's label in its short-buffer / magic / version refusals, the interleaved coder's payload rule in each of
its three containers, the one bits_B.bin writer and finish_all.  No GPU: the payloads are opaque bytes."""
import hashlib
import struct

import pytest

from vcamd import containers, hip, lhbdc

WAVES = 4
PA = (bytes(range(256)) * 9)[:WAVES * 516 + 16]                  # 2080 bytes each: the four sub-stream headers and four words
PB = (bytes(range(255, -1, -1)) * 9)[:WAVES * 516 + 16]
H, W = 192, 256                                                   # the frame whose hyper-latents are 1x1 (motion) and 3x4 (residual)
BITS_B = (bytes(range(40)), bytes(range(7)), bytes(range(100)), bytes(range(13)))       # mv_y, mv_z, res_y, res_z
VCIB_STRINGS = {c: [[[bytes(range(k, k + 5 + 7 * i))] for i in range(5)], [bytes(range(k, k + 9))]]
                for k, c in ((0, "offset"), (1, "residual"))}
NUMBERS = ((17, 30), 4, 1.5, 0.75, 0.25)                          # shape, down_ratio, s, scale1, scale2


def _bits_b():
    return containers.pack_bits_b(1626, (1, 1), (3, 4), *BITS_B)


def _vcld():
    return containers.pack_lhbdc_frame_dev(1626, (1, 1), (3, 4), WAVES, PA, PB)


def _vcib():
    return containers.pack_icip2024_frame(VCIB_STRINGS, *NUMBERS)


def _vcid():
    return containers.pack_icip2024_frame_dev({"offset": [PA], "residual": [PB]}, *NUMBERS, WAVES)


def _vcii():
    return containers.pack_icip2024_intra_dev(PA, (2, 3), WAVES)


def _vcsq():
    frame = {"I": _vcii(), "B": _vcid()}
    return containers.pack_sequence([(t, o, frame[t]) for o, t in containers.sequence_plan(16, 5)], 1920, 1080, 16, 1.5, 3)


FROZEN = {
    "bits_B": (_bits_b, struct.pack("<IHHIIHHI", 1626, 1, 1, 40, 7, 3, 4, 100),
               "54c39924d6f668096ed5c47adff2caed28dc682520d9b83bd39eacbe6f413841"),
    "VCLD": (_vcld, struct.pack("<4sBBIHHHHII", b"VCLD", 1, WAVES, 1626, 1, 1, 3, 4, 2080, 2080),
             "bb4a16952c9a7b309aaac527c7d8206ea345c4c744c7ff9625776f9c20c0a3c7"),
    "VCIB": (_vcib, struct.pack("<4sBBHHfff12I", b"VCIB", 1, 4, 17, 30, 1.5, 0.75, 0.25, 9, 5, 12, 19, 26, 33, 9, 5, 12, 19, 26, 33),
             "89c9fdc483c94ce934c43891c18674bd31830ce86beca837d9a5d9adb79189d7"),
    "VCID": (_vcid, struct.pack("<4sBBHHfffBII", b"VCID", 1, 4, 17, 30, 1.5, 0.75, 0.25, WAVES, 2080, 2080),
             "91d396f7498615deefe65df2cb284250250220ece93d90da9a10954a57f3835e"),
    "VCII": (_vcii, struct.pack("<4sBBHHI", b"VCII", 1, WAVES, 2, 3, 2080),
             "6030349286053b9266a4c70afff91f8c07ad017cd1b6fdd2b7df2e24249e63c6"),
    # plan of (16, 5): I 0, I 4, B 3, B 2, B 1 -- the first record's header follows the file's
    "VCSQ": (_vcsq, struct.pack("<4sBBHHIHfB", b"VCSQ", 1, 1, 1920, 1080, 5, 16, 1.5, 3) + struct.pack("<BII", 0, 0, 14 + 2080),
             "cc9f98c393eee2b226430efbb281f78b2a380599ddee166603b3733718267dfa"),
}


@pytest.mark.parametrize("name", list(FROZEN))
def test_frozen_bytes(name):
    pack, header, digest = FROZEN[name]
    blob = pack()
    assert blob[:len(header)] == header
    assert hashlib.sha256(blob).hexdigest() == digest


def test_one_bits_b_writer():
    mv_y, mv_z, res_y, res_z = BITS_B
    mv_bits, res_bits = {"strings": [[mv_y], [mv_z]], "shape": (1, 1)}, {"strings": [[res_y], [res_z]], "shape": (3, 4)}
    blob = lhbdc.write_container(None, 1626, mv_bits, res_bits)
    assert blob == _bits_b()
    lmbda, mv, res, shape_mv, shape_res = lhbdc.read_container(blob)
    assert (lmbda, mv, res, tuple(shape_mv), tuple(shape_res)) == (1626, [[mv_y], [mv_z]], [[res_y], [res_z]], (1, 1), (3, 4))


READERS = {
    "VCLD container": (lambda b: containers.unpack_lhbdc_frame_dev(b, H, W), _vcld, 26),
    "ICIP2024 container": (containers.unpack_icip2024_frame, _vcib, 70),
    "ICIP2024 device-coded container": (containers.unpack_icip2024_frame_dev, _vcid, 31),
    "ICIP2024 I-frame container": (containers.unpack_icip2024_intra_dev, _vcii, 14),
    "sequence file": (containers.unpack_sequence, _vcsq, 21),
}


@pytest.mark.parametrize("label", list(READERS))
def test_every_reader_names_its_format(label):
    unpack, pack, fixed = READERS[label]
    good = pack()
    unpack(good)
    for bad in (good[:fixed - 1], b"VCXX" + good[4:], good[:4] + b"\x02" + good[5:]):
        with pytest.raises(hip.VcError) as e:
            unpack(bad)
        assert label + ":" in str(e.value)


# (reader, blob, offset of the wave count, offset of the first of the payload lengths; a container with one payload has no second)
PAYLOAD_RULE = {
    "VCLD": (READERS["VCLD container"][0], _vcld, 5, (18, 22)),
    "VCID": (containers.unpack_icip2024_frame_dev, _vcid, 22, (23, 27)),
    "VCII": (containers.unpack_icip2024_intra_dev, _vcii, 5, (10,)),
}


def _with_u32(blob, at, value):
    return blob[:at] + struct.pack("<I", value) + blob[at + 4:]


@pytest.mark.parametrize("name", list(PAYLOAD_RULE))
def test_payload_rule(name):
    unpack, pack, at_waves, at_len = PAYLOAD_RULE[name]
    good = pack()
    assert isinstance(unpack(good), dict)
    bad = [good + b"\0\0\0\0", good[:-4],                                            # the buffer is 4 bytes longer / shorter than the lengths
           _with_u32(good, at_len[0], 2080 + 4), _with_u32(good, at_len[0], 2080 - 4),          # the lengths are 4 bytes more / less than the buffer
           good[:at_waves] + b"\x08" + good[at_waves + 1:]]                                     # 8 x 516 = 4128 > 2080
    if len(at_len) == 2:                                                                        # not whole words, the sum still fits
        bad.append(_with_u32(_with_u32(good, at_len[0], 2080 + 2), at_len[1], 2080 - 2))
    else:                                                                                       # one payload: the buffer follows it
        bad.append(_with_u32(good, at_len[0], 2080 - 2)[:-2])
    for b in bad:
        with pytest.raises(hip.VcError):
            unpack(b)


def test_the_intra_writer_keeps_the_payload_rule():
    for payload, waves in ((PA[:-2], 4), (PA, 8), (PA, 3)):
        with pytest.raises(hip.VcError):
            containers.pack_icip2024_intra_dev(payload, (2, 3), waves)


def test_finish_all_reads_every_decoder_before_it_raises_the_first_error():
    called = []

    class Stub:
        def __init__(self, name, error=None):
            self.name, self.error = name, error

        def finish(self):
            called.append(self.name)
            if self.error is not None:
                raise self.error

    first, third = hip.VcError("first"), hip.VcError("third")
    with pytest.raises(hip.VcError) as e:
        containers.finish_all([Stub("a", first), Stub("b"), Stub("c", third)])
    assert called == ["a", "b", "c"] and e.value is first
    containers.finish_all([Stub("d")])
    containers.finish_all([])
    assert called == ["a", "b", "c", "d"]
