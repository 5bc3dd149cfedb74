"""The containers of the ICIP2024 sequence file (vcamd/containers.py): VCII (one device-coded ELIC I-frame) and VCSQ (the frames of a
sequence in coding order): pack / unpack round trips and every refusal.  No GPU: the payloads are opaque bytes here."""
import struct

import pytest

from vcamd import containers, hip, icip2024

PAYLOAD = bytes(range(256)) * 9                # 2304 bytes: a multiple of 4, at least 4 * 516


def _records(intra_size, n):
    return [(t, o, bytes([o]) * (8 + 4 * o)) for o, t in containers.sequence_plan(intra_size, n)]


def test_intra_round_trip_and_refusals():
    blob = containers.pack_icip2024_intra_dev(PAYLOAD, (2, 3), 4)
    assert len(blob) == 14 + len(PAYLOAD) and blob[:4] == b"VCII"
    assert containers.unpack_icip2024_intra_dev(blob) == {"payload": PAYLOAD, "waves": 4, "shape": (2, 3)}
    bad = [blob[:13], b"VCID" + blob[4:], blob[:4] + b"\x02" + blob[5:], blob[:5] + b"\x03" + blob[6:], blob[:5] + b"\x00" + blob[6:],
           blob[:5] + b"\x08" + blob[6:],                              # 8 waves need 4128 bytes
           blob[:-4], blob + b"\0\0\0\0", blob[:10] + struct.pack("<I", len(PAYLOAD) - 4) + blob[14:],
           blob[:10] + struct.pack("<I", len(PAYLOAD) - 2) + blob[14:-2],                # not a multiple of 4
           blob[:6] + b"\0\0" + blob[8:]]
    for b in bad:
        with pytest.raises(hip.VcError):
            containers.unpack_icip2024_intra_dev(b)
    for args in ((PAYLOAD, (2, 3), 3), (PAYLOAD[:-2], (2, 3), 4), (PAYLOAD[:2000], (2, 3), 4), (PAYLOAD, (0, 3), 4), (PAYLOAD, (2, 70000), 4)):
        with pytest.raises(hip.VcError):
            containers.pack_icip2024_intra_dev(*args)
    with pytest.raises(hip.VcError):
        containers.unpack_icip2024_frame_dev(blob)                      # each reader refuses the other's magic


@pytest.mark.parametrize("intra_size,n", [(16, 1), (16, 5), (16, 7), (16, 17), (16, 22), (8, 17)])
def test_sequence_round_trip(intra_size, n):
    records = _records(intra_size, n)
    if n > 1:
        order, typ = icip2024.get_order_typ_list(intra_size, n)
        assert [o for _, o, _ in records] == order and [t for t, _, _ in records] == [typ[o] for o in order]
    blob = containers.pack_sequence(records, 1920, 1080, intra_size, 2.5, 3)
    assert len(blob) == 21 + sum(9 + len(b) for _, _, b in records) and blob[:4] == b"VCSQ"
    got = containers.unpack_sequence(blob)
    assert got == {"family": 1, "width": 1920, "height": 1080, "frames": n, "intra_size": intra_size, "s": 2.5, "intra_quality": 3,
                   "records": records}


def test_sequence_refusals():
    records = _records(16, 7)
    blob = containers.pack_sequence(records, 128, 64, 16, 1.0, 0)
    first = 21                                                         # offset of the first record
    second = first + 9 + len(records[0][2])
    bad = {
        "short header": blob[:20],
        "magic": b"VCSX" + blob[4:],
        "version": blob[:4] + b"\x02" + blob[5:],
        "family 2": blob[:5] + b"\x02" + blob[6:],
        "family 0": blob[:5] + b"\x00" + blob[6:],
        "zero width": blob[:6] + b"\0\0" + blob[8:],
        "zero intra_size": blob[:14] + b"\0\0" + blob[16:],
        "level not finite": blob[:16] + struct.pack("<f", float("nan")) + blob[20:],
        "frame count 0": blob[:10] + struct.pack("<I", 0) + blob[14:],
        "frame count 6": blob[:10] + struct.pack("<I", 6) + blob[14:],                   # other plan, trailing record
        "frame count 8": blob[:10] + struct.pack("<I", 8) + blob[14:],
        "frame count huge": blob[:10] + struct.pack("<I", 0xffffffff) + blob[14:],
        "truncated": blob[:-1],
        "cut inside a record header": blob[:second + 4],
        "trailing": blob + b"\0",
        "length overruns": blob[:first + 5] + struct.pack("<I", len(blob)) + blob[first + 9:],
        "length falls short": blob[:first + 5] + struct.pack("<I", len(records[0][2]) - 1) + blob[first + 9:],
        "type": blob[:first] + b"\x01" + blob[first + 1:],
        "unknown type": blob[:first] + b"\x07" + blob[first + 1:],
        "order": blob[:second + 1] + struct.pack("<I", 5) + blob[second + 5:],
    }
    for what, b in bad.items():
        with pytest.raises(hip.VcError):
            containers.unpack_sequence(b)
            pytest.fail(what)
    swapped = [records[0], records[2], records[1]] + records[3:]
    for args in ((swapped, 128, 64, 16, 1.0, 0), (records[:-1], 128, 64, 16, 1.0, 0), (records, 0, 64, 16, 1.0, 0), (records, 128, 64, 0, 1.0, 0),
                 (records, 128, 64, 16, float("inf"), 0), (records, 128, 64, 16, 1.0, 256), ([], 128, 64, 16, 1.0, 0)):
        with pytest.raises(hip.VcError):
            containers.pack_sequence(*args)
    with pytest.raises(hip.VcError):
        containers.pack_sequence(records, 128, 64, 16, 1.0, 0, family=2)


def test_a_plan_that_is_no_coding_order_is_refused():
    """get_order_typ_list follows the reference's GOP-16 order: for some (intra_size, frame count) pairs it names frames past the end
    of the sequence -- (4, 5) gives [0, 16, 8, 4, 12].  Neither side codes such a pair."""
    assert containers.sequence_plan(16, 5) == [(0, "I"), (4, "I"), (3, "B"), (2, "B"), (1, "B")]
    for intra_size, n in ((4, 5), (4, 7), (0, 5), (16, 0)):
        with pytest.raises(hip.VcError):
            containers.sequence_plan(intra_size, n)
