"""-m gpu: the kernels of the interleaved range coder (csrc/rans_device.hip: vc_irans_encode, vc_irans_decode_begin,
vc_irans_decode) against the host reference of the format (vc_irans_encode_host / vc_irans_decode_host, tested on the CPU by
tests/test_irans_cpu.py together with the sanitizer fuzz of the per-lane steps both sides share): byte-identical payloads, the
same symbols from host-written payloads with the device state chained over the segments, both table residencies (LDS and
global memory), batches, and a payload that ends early."""
import numpy as np
import pytest
import torch

from test_irans_cpu import SETS, draw, make_set
from vcamd import hip

pytestmark = pytest.mark.gpu

BIG = make_set(4, [1200] * 30, ones=7)          # 36 000 u16 entries = 72 KB: read from global memory, not staged in LDS
FULL = make_set(5, [1024] * 32, ones=3)         # 32 768 u16 entries = exactly the 64 KiB of LDS the staged path may ask for


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cases(waves):
    """name -> (host segment tables of two images, table sets)"""
    rng = np.random.default_rng(100 + waves)
    out = {}
    for name in sorted(SETS):
        for count in (1, 63, 64, 65, 64 * waves - 1, 64 * waves + 1, 4099):
            out[f"{name}-{count}"] = ([[draw(rng, SETS[name], count) + (0,)] for _ in range(2)], [SETS[name]])
    sets = [SETS["long"], SETS["nine"], BIG]
    counts = [257, 0, 64 * waves + 1, 1, 63, 700, 64, 65, 5, 1000, 64 * waves - 1]
    out["eleven"] = ([[draw(rng, sets[k % 3], c) + (k % 3,) for k, c in enumerate(counts)] for _ in range(2)], sets)
    n = 64 * waves * 3 + 17
    idx = rng.integers(0, 3, n).astype(np.int32)
    every = (rng.integers(1000, 2 ** 20, n) * rng.choice([-1, 1], n)).astype(np.int32)
    lane = draw(rng, SETS["nine"], n, escapes=0.0)
    lane[0][5::64 * waves] = 12345
    extreme = draw(rng, SETS["nine"], n, escapes=0.0)
    extreme[0][:8] = [2 ** 30, -(2 ** 30), -(2 ** 31) + 1, 2 ** 31 - 1, -(2 ** 31), 0, 2 ** 31 - 2, -1]
    out["escapes"] = ([[(every, idx, 0), lane + (0,)], [extreme + (0,), draw(rng, SETS["nine"], n, escapes=0.0) + (0,)]], [SETS["nine"]])
    out["global-tables"] = ([[draw(rng, BIG, 3000) + (0,)] for _ in range(2)], [BIG])
    out["lds-limit"] = ([[draw(rng, FULL, 3000) + (0,)] for _ in range(2)], [FULL])
    return out


def _device_segments(images, dev):
    """per-image host segment tables -> [(symbols [n, count], indexes [n, count], table_set)] on the device"""
    segs = []
    for k in range(len(images[0])):
        sym = torch.from_numpy(np.stack([im[k][0] for im in images])).to(dev)
        idx = torch.from_numpy(np.stack([im[k][1] for im in images])).to(dev)
        segs.append((sym.contiguous(), idx.contiguous(), images[0][k][2]))
    return segs


@pytest.mark.parametrize("waves", [1, 4])
def test_kernels_against_the_host_reference(dev, waves):
    residencies = set()
    for name, (images, sets) in _cases(waves).items():
        want = [hip.irans_encode_host(im, sets, waves) for im in images]
        dsets = [hip.IransTables(*s, dev) for s in sets]
        segs = _device_segments(images, dev)
        # encoder: a batch of two gives the two host payloads byte for byte, and so does each image alone
        assert hip.irans_encode(segs, dsets, waves) == want, name
        assert hip.irans_encode([(s[1:], i[1:], k) for s, i, k in segs], dsets, waves) == want[1:], name
        # decoder: host-written payloads, one launch per segment, the state struct carried from one to the next
        dec = hip.IransDecoder(want, waves, dev)
        got = [dec.decode(idx, dsets[k]) for _, idx, k in segs]
        dec.finish()
        for (sym, _, k), g in zip(segs, got):
            assert torch.equal(g, sym), name
            residencies.add(dsets[k].in_lds)
        host = hip.irans_decode_host(want[0], [(i, k) for _, i, k in images[0]], sets, waves)
        assert all(np.array_equal(h, g[0].cpu().numpy()) for h, g in zip(host, got)), name
    assert residencies == {True, False}
    full = hip.IransTables(*FULL, dev)
    assert full.entries == 32768 and full.in_lds and not hip.IransTables(*BIG, dev).in_lds


def test_a_payload_that_ends_early_sets_the_error_word_and_decodes_zeros(dev):
    """W = 1, the word count lowered by 40 and the last 40 words removed: every header fits the length, the sub-stream runs out
    behind the first segment.  No fault: the segments before decode as written, everything after the break is zero,
    the error word is set and finish() raises; an out-of-range index and a truncated upload end the same way."""
    rng = np.random.default_rng(3)
    tables = SETS["long"]
    images = [[draw(rng, tables, 2000) + (0,), draw(rng, tables, 3000) + (0,), draw(rng, tables, 500) + (0,)]]
    good = hip.irans_encode_host(images[0], [tables], 1)
    count = int(np.frombuffer(good[:4], dtype=np.uint32)[0])
    short = np.array([count - 40], dtype=np.uint32).tobytes() + good[4:len(good) - 160]
    with pytest.raises(hip.VcError):
        hip.irans_decode_host(short, [(i, k) for _, i, k in images[0]], [tables], 1)
    dt = hip.IransTables(*tables, dev)
    segs = _device_segments(images, dev)
    dec = hip.IransDecoder([short], 1, dev)
    got = [dec.decode(idx, dt).cpu().numpy()[0] for _, idx, _ in segs]
    broke = False
    for g, (want, _, _) in zip(got, images[0]):
        if broke:
            assert not g.any()                                       # every later segment: zeros
        elif (g != want).any():
            start = int(np.argmax(g != want)) // 64 * 64             # the round in which the sub-stream ran out
            assert np.array_equal(g[:start], want[:start]) and not g[start:].any()
            broke = True
    assert broke and np.array_equal(got[0], images[0][0][0])
    head = dec.states[:8].cpu().numpy().view(np.uint32)
    assert head[0] == 2 and head[1] == 1
    with pytest.raises(hip.VcError):
        dec.finish()
    # an index past the tables: error 4, zeros from that round on
    dec = hip.IransDecoder([good], 1, dev)
    bad = segs[0][1].clone()
    bad[0, 1000] = 4
    out = dec.decode(bad, dt).cpu().numpy()[0]
    assert np.array_equal(out[:960], images[0][0][0][:960]) and not out[960:].any()
    assert dec.states[:4].cpu().numpy().view(np.uint32)[0] == 4
    with pytest.raises(hip.VcError):
        dec.finish()
    # a truncated upload: refused by the header walk, every symbol zero
    dec = hip.IransDecoder([good[:len(good) // 2 // 4 * 4]], 1, dev)
    assert not dec.decode(segs[0][1], dt).any() and dec.states[:4].cpu().numpy().view(np.uint32)[0] == 1
    with pytest.raises(hip.VcError):
        dec.finish()
    # an untouched payload that is not read to its end: the cursor check of finish()
    dec = hip.IransDecoder([good], 1, dev)
    dec.decode(segs[0][1], dt)
    with pytest.raises(hip.VcError):
        dec.finish()


def test_zeros_behind_a_violation_do_not_depend_on_timing(dev):
    """W = 4, wave 1's word count lowered by 30 and its last 30 words removed: wave 1 runs out inside some segment.  In that launch
    only wave 1 goes to zeros (from the round of the break on), its siblings finish the segment as written; every wave decodes
    zeros in all later launches.  Two runs give the same symbols."""
    rng = np.random.default_rng(8)
    tables, waves = SETS["long"], 4
    images = [[draw(rng, tables, 4000) + (0,), draw(rng, tables, 6000) + (0,), draw(rng, tables, 4000) + (0,), draw(rng, tables, 700) + (0,)]]
    good = hip.irans_encode_host(images[0], [tables], waves)
    c0 = int(np.frombuffer(good[:4], dtype=np.uint32)[0])
    at1 = 516 + 4 * c0                                                   # sub-stream 1
    c1 = int(np.frombuffer(good[at1:at1 + 4], dtype=np.uint32)[0])
    end1 = at1 + 516 + 4 * c1
    short = good[:at1] + np.array([c1 - 30], dtype=np.uint32).tobytes() + good[at1 + 4:end1 - 120] + good[end1:]
    dt = hip.IransTables(*tables, dev)
    segs = _device_segments(images, dev)
    runs = []
    for _ in range(2):
        dec = hip.IransDecoder([short], waves, dev)
        runs.append([dec.decode(idx, dt).cpu().numpy()[0] for _, idx, _ in segs])
        assert dec.states[:4].cpu().numpy().view(np.uint32)[0] == 2
        with pytest.raises(hip.VcError):
            dec.finish()
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    broke = False
    for g, (want, _, _) in zip(runs[0], images[0]):
        wave = (np.arange(g.size) // 64) % waves
        if broke:
            assert not g.any()
        elif (g != want).any():
            assert np.array_equal(g[wave != 1], want[wave != 1])         # the siblings of that launch are untouched
            mine, truth = g[wave == 1], want[wave == 1]
            start = int(np.argmax(mine != truth)) // 64 * 64
            assert np.array_equal(mine[:start], truth[:start]) and not mine[start:].any()
            broke = True
    assert broke and not runs[0][-1].any()
