"""-m gpu: the vc_picture_hash kernel against its host twin (vc_picture_hash_host, itself checked against the formula in
tests/test_picture_hash_cpu.py) on every path the kernel has: the words in front of the first 16-byte boundary, the 16-byte body,
the words behind it, images at different 16-byte phases (base offset x image pitch), one and several workgroups per image, one
and several images.  Guard words in front of, between and behind the images would change the hash if a lane read them.  All
comparisons are exact."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4 * 256 * 7 + 3, 3 * 192 * 256]
GUARD = 0xA5A5A5A5
PAD = 8                       # guard words in front of the first image


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _planted(count, seed):
    """fp32 data with NaN, +-0, inf and denormals planted, as its 32-bit words"""
    g = np.random.default_rng(seed)
    x = g.standard_normal(count).astype(np.float32)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-45], dtype=np.float32)
    at = g.permutation(count)[: min(count, 2 * special.size)]
    x[at] = special[np.arange(at.size) % special.size]
    w = x.view(np.uint32).copy()
    if count > 8:
        w[count // 2] = 0x7fc00001             # a NaN with a payload: hashed as its bits
    return w


def _launch(hip, buf, offset, n, count, pitch, slots=None, out=None, partials=None):
    """the raw entry point on words [offset, ...) of the int32 device tensor ``buf``"""
    L = hip.lib()
    slots = L.vc_bits_slots() if slots is None else slots
    partials = torch.empty(max(n, 1) * L.vc_bits_slots(), dtype=torch.int64, device=buf.device) if partials is None else partials
    out = torch.zeros(max(n, 1), dtype=torch.int64, device=buf.device) if out is None else out
    rc = L.vc_picture_hash(hip.stream(), buf.data_ptr() + 4 * offset, n, count, pitch, partials.data_ptr(), slots, out.data_ptr())
    return rc, out


@pytest.mark.parametrize("count", COUNTS)
def test_kernel_against_host_twin(dev, count):
    from vcamd import hip
    for n in (1, 3):
        images = [_planted(count, 100 * n + k) for k in range(n)]
        want = [hip.picture_hash_host(w) for w in images]
        for extra in (0, 1, 5):
            pitch = count + extra
            for base in range(4):
                host = np.full(PAD + base + n * pitch + PAD, GUARD, dtype=np.uint32)
                for k, w in enumerate(images):
                    host[PAD + base + k * pitch: PAD + base + k * pitch + count] = w
                buf = torch.from_numpy(host.view(np.int32)).to(dev)
                rc, out = _launch(hip, buf, PAD + base, n, count, pitch)
                assert rc == hip.VC_OK
                rc, again = _launch(hip, buf, PAD + base, n, count, pitch)
                assert rc == hip.VC_OK
                got = [int(v) & 0xffffffffffffffff for v in out.cpu().tolist()]
                assert got == want, (n, extra, base)
                assert torch.equal(out, again)


def test_guard_words_would_change_the_hash(dev):
    """(what the guards are worth: a hash that took one of them in, as word `count`, is another hash)"""
    from vcamd import hip
    w = _planted(65, 1)
    assert hip.picture_hash_host(np.concatenate([w, np.array([GUARD], np.uint32)])) != hip.picture_hash_host(w)


def test_python_entry_point(dev):
    from vcamd import hip
    g = torch.Generator().manual_seed(3)
    x = torch.rand(3, 3, 20, 37, generator=g).to(dev)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = hip.picture_hash(x)
        into = torch.empty(3, dtype=torch.int64, device=dev)
        assert hip.picture_hash(x, out=into) is into
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert out.dtype == torch.int64 and tuple(out.shape) == (3,)
    host = x.cpu().numpy()
    assert [int(v) & 0xffffffffffffffff for v in out.cpu().tolist()] == [hip.picture_hash_host(host[k]) for k in range(3)]
    assert torch.equal(out, into)
    i32 = torch.arange(-40, 37, dtype=torch.int32, device=dev).view(1, -1)
    assert int(hip.picture_hash(i32).cpu()[0]) & 0xffffffffffffffff == hip.picture_hash_host(i32.cpu().numpy())
    one = hip.picture_hash(x[1:2])                       # an image hashes the same alone as in a batch
    assert int(one.cpu()[0]) == int(out.cpu()[1])
    for bad in (x.double(), x.half(), x.to(torch.uint8), x.cpu(), x[:, :, :, ::2], x.to(torch.int64)):
        with pytest.raises(hip.VcError):
            hip.picture_hash(bad)
    with pytest.raises(hip.VcError):
        hip.picture_hash(x, out=torch.empty(2, dtype=torch.int64, device=dev))
    with pytest.raises(hip.VcError):
        hip.picture_hash(x, out=torch.empty(3, dtype=torch.int32, device=dev))
    with pytest.raises(hip.VcError):
        hip.picture_hash(torch.empty(0, 4, device=dev))


def test_refused_before_any_launch(dev):
    from vcamd import hip
    L = hip.lib()
    slots = L.vc_bits_slots()
    buf = torch.zeros(64, dtype=torch.int32, device=dev)
    partials = torch.full((slots,), -1, dtype=torch.int64, device=dev)
    out = torch.full((1,), -1, dtype=torch.int64, device=dev)
    s, p, q, o = hip.stream(), buf.data_ptr(), partials.data_ptr(), out.data_ptr()
    cases = {
        "null words": (s, None, 1, 16, 16, q, slots, o),
        "null partials": (s, p, 1, 16, 16, None, slots, o),
        "null out": (s, p, 1, 16, 16, q, slots, None),
        "n < 1": (s, p, 0, 16, 16, q, slots, o),
        "count < 1": (s, p, 1, 0, 16, q, slots, o),
        "count >= 2^32": (s, p, 1, 1 << 32, 1 << 32, q, slots, o),
        "pitch < count": (s, p, 1, 16, 15, q, slots, o),
        "slots": (s, p, 1, 16, 16, q, slots - 1, o),
        "unaligned": (s, ctypes.c_void_p(p + 2), 1, 16, 16, q, slots, o),
    }
    for name, args in cases.items():
        assert L.vc_picture_hash(*args) == -1, name                    # VC_EINVAL
    assert L.vc_picture_hash(s, p, 1, 16, 16, q, slots, o) == hip.VC_OK
    torch.cuda.synchronize()
    assert int(out.cpu()[0]) & 0xffffffffffffffff == hip.picture_hash_host(np.zeros(16, np.uint32))
