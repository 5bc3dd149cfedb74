"""The VCLD container of the LHBDC stream codec's coder="device" (vcamd/containers.py: pack_lhbdc_frame_dev /
unpack_lhbdc_frame_dev) and the two-segment payload it carries, through the host reference of the
interleaved coder -- no GPU.

Size accounting (test_size_of_a_two_segment_payload).  The 200 000 escape-free symbols of
tests/test_irans_cpu.py::test_size_against_the_sequential_coder (Gaussian tables, seed 7; 114 300 bytes from the sequential
coder), cut into the payload's two segments behind symbol 128.  The bound is that test's: its measured ratio for the
wave count + 256 W / sequential bytes -- the arithmetic is the same, the only freedom is where each of the 64 W lanes'
renormalisation boundaries fall (one 32-bit word per lane), and restarting the lanes at a segment boundary only moves those."""
import struct

import numpy as np
import pytest

from test_irans_cpu import MEASURED_RATIO, SEQUENTIAL_BYTES, _gaussian_tables, draw, make_set
from vcamd import containers, hip

H, W = 192, 256                        # the frame of tests/test_stream_gpu.py: hyper-latents 1x1 (motion) and 3x4 (residual)
MV_SHAPE, RES_SHAPE = (1, 1), (3, 4)


def _payload(waves, seed=0, words=40):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, waves * 516 + 4 * words, dtype=np.uint8).tobytes()


def test_round_trip():
    for waves in (1, 2, 4, 8, 16):
        mv, res = _payload(waves, 1, 10), _payload(waves, 2, 77)
        blob = containers.pack_lhbdc_frame_dev(1626, MV_SHAPE, RES_SHAPE, waves, mv, res)
        assert blob[:4] == b"VCLD" and len(blob) == 26 + len(mv) + len(res)
        got = containers.unpack_lhbdc_frame_dev(blob, H, W)
        assert got == {"lmbda": 1626, "waves": waves, "mv_shape": MV_SHAPE, "res_shape": RES_SHAPE, "mv": mv, "res": res}
    for bad_waves in (0, 3, 32):
        with pytest.raises(hip.VcError):
            containers.pack_lhbdc_frame_dev(1626, MV_SHAPE, RES_SHAPE, bad_waves, mv, res)
    with pytest.raises(hip.VcError):
        containers.pack_lhbdc_frame_dev(1626, (0, 1), RES_SHAPE, 4, mv, res)


def test_refusals():
    mv, res = _payload(4, 3), _payload(4, 4)
    good = containers.pack_lhbdc_frame_dev(1626, MV_SHAPE, RES_SHAPE, 4, mv, res)
    containers.unpack_lhbdc_frame_dev(good, H, W)

    def refused(blob, h=H, w=W):
        with pytest.raises(hip.VcError):
            containers.unpack_lhbdc_frame_dev(blob, h, w)

    refused(b"VCLX" + good[4:])                                        # magic
    refused(b"VCIB" + good[4:])
    refused(good[:4] + b"\x02" + good[5:])                             # version
    for waves in (0, 3, 5, 17, 32, 255):                               # waves: not a power of two in 1..16
        refused(good[:5] + bytes([waves]) + good[6:])
    refused(good[:5] + bytes([8]) + good[6:])                          # a wave count whose headers alone exceed the payloads
    refused(good[:-4])                                                 # lengths overrun the data
    refused(good[:25])
    refused(b"")
    big = bytearray(good)
    big[18:22] = struct.pack("<I", len(mv) + 4)
    refused(bytes(big))
    big[18:22] = struct.pack("<I", 0xffffffff)
    refused(bytes(big))
    refused(good + b"\0\0\0\0")                                        # trailing bytes
    refused(good + b"\0")
    odd = bytearray(good)                                              # lengths that add up but are not whole words
    odd[18:22] = struct.pack("<I", len(mv) + 2)
    odd[22:26] = struct.pack("<I", len(res) - 2)
    refused(bytes(odd))
    for at, shape in ((10, (2, 1)), (10, (65535, 65535)), (14, (3, 5)), (14, (0, 4))):       # shapes of another frame size
        bad = bytearray(good)
        bad[at:at + 4] = struct.pack("<HH", *shape)
        refused(bytes(bad))
    refused(good, 256, 256)


def _layout(rng, eb, gc, n_z, hw_z, n_y, hw_y):
    """(z segment, y segment) as the codec lays them out: z index = the channel, y index drawn over the Gaussian tables; every 17th
    z symbol and a twentieth of the y symbols lie outside every table's range (escapes)"""
    cdfs, sizes, offs = eb
    z_idx = np.repeat(np.arange(n_z, dtype=np.int32), hw_z)
    u = rng.integers(0, 65536, z_idx.size)
    z_sym = np.array([min(np.searchsorted(cdfs[t, :sizes[t]], v, side="right") - 1, sizes[t] - 3) + offs[t] for t, v in zip(z_idx, u)],
                     dtype=np.int32)
    z_sym[::17] = rng.choice([-65000, 65000, 2 ** 31 - 1, -(2 ** 31)], z_sym[::17].size)
    y_sym, y_idx = draw(rng, gc, n_y * hw_y, 0.05)
    return (z_sym, z_idx, 0), (y_sym, y_idx, 1)


@pytest.mark.parametrize("waves", [1, 4, 16])
def test_segment_layout_through_the_host_reference(waves):
    """z: 128 symbols (one per channel, 1x1), then y: 128 x 4 x 4 -- at W = 4 and 16 whole waves idle through the z segment, whose
    only round is partial (y fills its rounds: 2048 = 8 x 256 = 2 x 1024; the second case, 5 x 4 x 4 = 80 symbols behind 2 x 3 x 5
    = 30, ends both segments in a partial round at every W).  A twentieth of the symbols lies outside every table: escapes."""
    eb, gc = make_set(11, [40] * 128, ones=2), _gaussian_tables()
    rng = np.random.default_rng(20 + waves)
    for n_z, hw_z, n_y, hw_y in ((128, 1, 128, 16), (2, 15, 5, 16)):
        segs = _layout(rng, eb, gc, n_z, hw_z, n_y, hw_y)
        payload = hip.irans_encode_host(list(segs), [eb, gc], waves)
        got = hip.irans_decode_host(payload, [(idx, k) for _, idx, k in segs], [eb, gc], waves)
        for (sym, _, _), g in zip(segs, got):
            assert np.array_equal(g, sym)
        blob = containers.pack_lhbdc_frame_dev(1626, MV_SHAPE, RES_SHAPE, waves, payload, payload)
        assert containers.unpack_lhbdc_frame_dev(blob, H, W)["res"] == payload
        # the segments are not interchangeable: decoding them in the other order is refused or gives other integers
        try:
            other = hip.irans_decode_host(payload, [(segs[1][1], 1), (segs[0][1], 0)], [eb, gc], waves)
            assert not np.array_equal(other[1], segs[0][0])
        except hip.VcError:
            pass


def test_size_of_a_two_segment_payload():
    tables = _gaussian_tables()
    rng = np.random.default_rng(7)
    sym, idx = draw(rng, tables, 200_000, escapes=0.0)
    old = hip.rans_encode(sym, idx, *tables)
    assert len(old) == SEQUENTIAL_BYTES
    for waves in (1, 4):
        segs = [(sym[:128], idx[:128], 0), (sym[128:], idx[128:], 1)]
        new = hip.irans_encode_host(segs, [tables, tables], waves)
        got = hip.irans_decode_host(new, [(i, k) for _, i, k in segs], [tables, tables], waves)
        assert np.array_equal(np.concatenate(got), sym)
        ratio = (len(new) - waves * 516) / len(old)
        print(f"W = {waves}: payload {len(new)} bytes, (payload - W * 516) / sequential = {ratio:.6f}")
        assert ratio <= MEASURED_RATIO[waves] + 256 * waves / len(old)
