"""The ICIP2024 B-frame container (vcamd/containers.py: pack_icip2024_frame / unpack_icip2024_frame) on synthetic strings:
round trip, the header layout INTEGRATION.md states, and the refusals of a reader that trusts nothing in the buffer."""
import os
import re
import struct

import numpy as np
import pytest

from vcamd import containers, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _strings(seed, empty=()):
    g = np.random.default_rng(seed)
    out = {}
    for k, codec in enumerate(("offset", "residual")):
        groups = [[b"" if (codec, i) in empty else g.integers(0, 256, 5 + 7 * i + k, dtype=np.uint8).tobytes()] for i in range(5)]
        z = [b"" if (codec, "z") in empty else g.integers(0, 256, 9 + k, dtype=np.uint8).tobytes()]
        out[codec] = [groups, z]
    return out


def _pack(strings, **kw):
    args = dict(shape=(17, 30), down_ratio=4, s=1.5, scale1=0.75, scale2=0.25)
    args.update(kw)
    return containers.pack_icip2024_frame(strings, **args)


@pytest.mark.parametrize("empty", [(), (("offset", "z"),), (("residual", 4), ("offset", 0)),
                                   tuple((c, k) for c in ("offset", "residual") for k in ("z", 0, 1, 2, 3, 4))])
def test_round_trip(empty):
    strings = _strings(3, empty)
    got = containers.unpack_icip2024_frame(_pack(strings))
    assert got["strings"] == strings
    assert got["shape"] == (17, 30) and got["down_ratio"] == 4
    assert (got["s"], got["scale1"], got["scale2"]) == (1.5, 0.75, 0.25)


def test_numbers_are_stored_as_fp32():
    got = containers.unpack_icip2024_frame(_pack(_strings(1), s=1.3, scale1=0.67, scale2=0.33))
    assert (got["s"], got["scale1"], got["scale2"]) == tuple(float(np.float32(v)) for v in (1.3, 0.67, 0.33))


def test_picks_the_image_of_a_batch():
    a, b = _strings(5), _strings(6)
    both = {c: [[a[c][0][i] + b[c][0][i] for i in range(5)], a[c][1] + b[c][1]] for c in a}
    assert containers.unpack_icip2024_frame(_pack(both, image=0))["strings"] == a
    assert containers.unpack_icip2024_frame(_pack(both, image=1))["strings"] == b


def test_header_layout_is_the_documented_one():
    """70 bytes in front of the payloads: magic 0, version 4, down_ratio 5, shape 6 / 8, s 10, scale1 14, scale2 18, lengths 22."""
    strings = _strings(7)
    data = _pack(strings)
    assert data[0:4] == b"VCIB" and data[4] == 1 and data[5] == 4
    assert struct.unpack_from("<HH", data, 6) == (17, 30)
    assert struct.unpack_from("<fff", data, 10) == (1.5, 0.75, 0.25)
    lengths = struct.unpack_from("<12I", data, 22)
    order = [strings[c][1][0] if k == "z" else strings[c][0][k][0] for c in ("offset", "residual") for k in ("z", 0, 1, 2, 3, 4)]
    assert list(lengths) == [len(b) for b in order]
    assert data[70:] == b"".join(order) and len(data) == 70 + sum(lengths)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("ICIP2024 B-frame container"):]
    rows = dict((name, int(off)) for off, name in re.findall(r"^\|\s*(\d+)\s*\|\s*`?([a-z0-9_ ]+?)`?\s*\|", sec, flags=re.M))
    assert rows == {"magic": 0, "version": 4, "down_ratio": 5, "shape": 6, "s": 10, "scale1": 14, "scale2": 18, "lengths": 22,
                    "payloads": 70}


def test_reader_refuses_what_it_cannot_trust():
    data = _pack(_strings(9))
    containers.unpack_icip2024_frame(data)
    bad = {
        "magic": b"VCIX" + data[4:],
        "version": data[:4] + bytes([2]) + data[5:],
        "down_ratio": data[:5] + bytes([3]) + data[6:],
        "zero shape": data[:6] + struct.pack("<HH", 0, 30) + data[10:],
        "truncated header": data[:40],
        "empty": b"",
        "truncated payload": data[:-1],
        "trailing bytes": data + b"\0",
        "length table overruns": data[:22] + struct.pack("<I", 0xffffffff) + data[26:],
        "not finite": data[:10] + struct.pack("<f", float("nan")) + data[14:],
    }
    for what, buf in bad.items():
        with pytest.raises(hip.VcError):
            containers.unpack_icip2024_frame(buf)
            pytest.fail(f"{what}: accepted")


def test_writer_refuses_fields_that_do_not_fit():
    for kw in ({"down_ratio": 3}, {"shape": (0, 4)}, {"shape": (70000, 4)}):
        with pytest.raises(hip.VcError):
            _pack(_strings(2), **kw)
    broken = _strings(2)
    broken["offset"][0].pop()
    with pytest.raises(hip.VcError):
        _pack(broken)
