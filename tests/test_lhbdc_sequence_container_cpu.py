"""The containers of the LHBDC sequence file (vcamd/containers.py): VCLI (one device-coded mbt2018_mean I-frame) and VCLS (the frames
of a sequence in coding order, with or without a hash of every decoded picture): pack / unpack round trips and every refusal.  No
GPU: the payloads are opaque bytes here."""
import struct

import pytest

from vcamd import containers, hip
from vcamd.gop import LEVEL_GROUPS

PAYLOAD = bytes(range(256)) * 9                # 2304 bytes: a multiple of 4, at least 4 * 516
HEADER = 19                                    # bytes of the VCLS header: offset of the first record
SIZES = [1, 2, 9, 12, 17, 19]


def _records(n):
    return [(t, o, bytes([o]) * (8 + 4 * o)) for o, t in containers.lhbdc_sequence_plan(n)]


def _hashes(n):
    return {o: (0x9E3779B97F4A7C15 * (o + 1)) & 0xffffffffffffffff for o in range(n)}


def test_intra_round_trip_and_refusals():
    blob = containers.pack_lhbdc_intra_dev(PAYLOAD, (2, 3), 4)
    assert len(blob) == 14 + len(PAYLOAD) and blob[:4] == b"VCLI"
    assert containers.unpack_lhbdc_intra_dev(blob) == {"payload": PAYLOAD, "waves": 4, "shape": (2, 3)}
    bad = [blob[:13], b"VCII" + blob[4:], b"VCLD" + blob[4:], blob[:4] + b"\x02" + blob[5:], blob[:5] + b"\x03" + blob[6:],
           blob[:5] + b"\x00" + blob[6:],
           blob[:5] + b"\x08" + blob[6:],                              # 8 waves need 4128 bytes
           blob[:-4], blob + b"\0\0\0\0", blob[:10] + struct.pack("<I", len(PAYLOAD) - 4) + blob[14:],
           blob[:10] + struct.pack("<I", len(PAYLOAD) - 2) + blob[14:-2],                # not a multiple of 4
           blob[:6] + b"\0\0" + blob[8:], blob[:8] + b"\0\0" + blob[10:]]
    for b in bad:
        with pytest.raises(hip.VcError):
            containers.unpack_lhbdc_intra_dev(b)
    for args in ((PAYLOAD, (2, 3), 3), (PAYLOAD[:-2], (2, 3), 4), (PAYLOAD[:2000], (2, 3), 4), (PAYLOAD, (0, 3), 4), (PAYLOAD, (2, 70000), 4)):
        with pytest.raises(hip.VcError):
            containers.pack_lhbdc_intra_dev(*args)
    # each reader refuses the others' magic
    with pytest.raises(hip.VcError):
        containers.unpack_icip2024_intra_dev(blob)
    with pytest.raises(hip.VcError):
        containers.unpack_lhbdc_frame_dev(blob, 128, 192)
    with pytest.raises(hip.VcError):
        containers.unpack_lhbdc_intra_dev(containers.pack_icip2024_intra_dev(PAYLOAD, (2, 3), 4))


@pytest.mark.parametrize("n", SIZES + [8, 10, 16, 25])
def test_plan_visits_every_order_once_with_b_frames_inside_whole_gops(n):
    plan = containers.lhbdc_sequence_plan(n)
    assert sorted(o for o, _ in plan) == list(range(n))
    gops = (n - 1) // 8
    for o, t in plan:
        assert t == ("B" if o % 8 and o < 8 * gops else "I"), (n, o)
    # coding order: a B-frame comes behind both frames it references, level by level
    at = {o: k for k, (o, _) in enumerate(plan)}
    assert plan[0] == (0, "I")
    for k in range(gops):
        seven = [8 * k + o for group in LEVEL_GROUPS for o in group]
        first = at[8 * k + 8]
        assert [o for o, _ in plan[first + 1:first + 8]] == seven
        assert at[8 * k] < first
    assert [o for o, _ in plan[1 + 8 * gops:]] == list(range(8 * gops + 1, n))


def test_plan_of_19_frames_spelled_out():
    assert [o for o, _ in containers.lhbdc_sequence_plan(19)] == [0, 8, 4, 2, 6, 1, 3, 5, 7, 16, 12, 10, 14, 9, 11, 13, 15, 17, 18]
    for n in (0, -1):
        with pytest.raises(hip.VcError):
            containers.lhbdc_sequence_plan(n)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("hashed", [False, True])
def test_sequence_round_trip(n, hashed):
    records = _records(n)
    hashes = _hashes(n) if hashed else None
    blob = containers.pack_lhbdc_sequence(records, 1920, 1080, 1626, 7, hashes)
    assert blob[:4] == b"VCLS" and blob[5] == (1 if hashed else 0)
    assert len(blob) == HEADER + sum(9 + (8 if hashed else 0) + len(b) for _, _, b in records)
    got = containers.unpack_lhbdc_sequence(blob)
    assert got == {"flags": 1 if hashed else 0, "width": 1920, "height": 1080, "frames": n, "lmbda": 1626, "intra_quality": 7,
                   "records": records, "hashes": hashes}


@pytest.mark.parametrize("hashed", [False, True])
def test_sequence_refusals(hashed):
    n = 12
    records = _records(n)
    blob = containers.pack_lhbdc_sequence(records, 128, 64, 1626, 7, _hashes(n) if hashed else None)
    fixed = 9 + (8 if hashed else 0)
    starts, pos = [], HEADER                                           # offset of every record
    for _, _, b in records:
        starts.append(pos)
        pos += fixed + len(b)
    first, second = starts[0], starts[1]
    bad = {
        "short header": blob[:HEADER - 1],
        "magic": b"VCLX" + blob[4:],
        "the ICIP2024 file's magic": b"VCSQ" + blob[4:],
        "version": blob[:4] + b"\x02" + blob[5:],
        "spare flag bit 1": blob[:5] + bytes([blob[5] | 2]) + blob[6:],
        "spare flag bit 7": blob[:5] + bytes([blob[5] | 0x80]) + blob[6:],
        "the other hash flag": blob[:5] + bytes([blob[5] ^ 1]) + blob[6:],           # the records no longer line up
        "zero width": blob[:6] + b"\0\0" + blob[8:],
        "zero height": blob[:8] + b"\0\0" + blob[10:],
        "intra quality 0": blob[:18] + b"\x00" + blob[19:],
        "intra quality 9": blob[:18] + b"\x09" + blob[19:],
        "frame count 0": blob[:10] + struct.pack("<I", 0) + blob[14:],
        "frame count 11": blob[:10] + struct.pack("<I", 11) + blob[14:],             # trailing record
        "frame count 13": blob[:10] + struct.pack("<I", 13) + blob[14:],
        "frame count huge": blob[:10] + struct.pack("<I", 0xffffffff) + blob[14:],   # refused against the length, nothing is sized
        "truncated": blob[:-1],
        "trailing": blob + b"\0",
        "length overruns": blob[:first + 5] + struct.pack("<I", len(blob)) + blob[first + 9:],
        "length falls short": blob[:first + 5] + struct.pack("<I", len(records[0][2]) - 1) + blob[first + 9:],
        "type": blob[:first] + b"\x01" + blob[first + 1:],
        "B coded as I": blob[:starts[2]] + b"\x00" + blob[starts[2] + 1:],
        "unknown type": blob[:first] + b"\x07" + blob[first + 1:],
        "order": blob[:second + 1] + struct.pack("<I", 5) + blob[second + 5:],
    }
    for k, s in enumerate(starts):                                     # truncation at every record boundary, and inside every record header
        bad[f"cut in front of record {k}"] = blob[:s]
        bad[f"cut inside the header of record {k}"] = blob[:s + 4]
        bad[f"cut behind the header of record {k}"] = blob[:s + fixed]
    for what, b in bad.items():
        with pytest.raises(hip.VcError):
            containers.unpack_lhbdc_sequence(b)
            pytest.fail(what)
    swapped = [records[0], records[2], records[1]] + records[3:]
    for args in ((swapped, 128, 64, 1626, 7), (records[:-2] + records[-1:], 128, 64, 1626, 7), (records, 0, 64, 1626, 7),
                 (records, 128, 70000, 1626, 7), (records, 128, 64, -1, 7), (records, 128, 64, 1 << 32, 7), (records, 128, 64, 1626, 0),
                 (records, 128, 64, 1626, 9), ([], 128, 64, 1626, 7)):
        with pytest.raises(hip.VcError):
            containers.pack_lhbdc_sequence(*args)
    for hashes in ({o: 1 for o in range(n - 1)}, {**_hashes(n), 3: 1 << 64}, {**_hashes(n), 3: -1}):
        with pytest.raises(hip.VcError):
            containers.pack_lhbdc_sequence(records, 128, 64, 1626, 7, hashes)


def test_stored_hash_is_where_the_layout_says():
    records = _records(9)
    hashes = _hashes(9)
    blob = containers.pack_lhbdc_sequence(records, 128, 64, 1626, 7, hashes)
    pos = HEADER
    for t, o, b in records:
        assert struct.unpack_from("<BII", blob, pos) == (0 if t == "I" else 1, o, len(b))
        assert struct.unpack_from("<Q", blob, pos + 9) == (hashes[o],)
        assert blob[pos + 17:pos + 17 + len(b)] == b
        pos += 17 + len(b)
    assert pos == len(blob)
    assert struct.unpack_from("<4sBBHHIIB", blob, 0) == (b"VCLS", 1, 1, 128, 64, 9, 1626, 7)


def test_the_two_sequence_readers_refuse_each_other():
    vcls = containers.pack_lhbdc_sequence(_records(9), 128, 64, 1626, 7, _hashes(9))
    order_typ = containers.sequence_plan(16, 5)
    vcsq = containers.pack_sequence([(t, o, bytes(8)) for o, t in order_typ], 128, 64, 16, 1.0, 0)
    with pytest.raises(hip.VcError):
        containers.unpack_sequence(vcls)
    with pytest.raises(hip.VcError):
        containers.unpack_lhbdc_sequence(vcsq)
