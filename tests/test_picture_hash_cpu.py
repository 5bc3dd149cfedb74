"""The decoded picture hash (include/vc_hip.h: "Decoded picture hash") through its host twin, which needs no GPU: the library's
vc_picture_hash_host against a numpy uint64 restatement of the formula written here, and the properties a picture hash is there for
-- every single-bit change, a swap of two words and an appended word change it.  All comparisons are exact."""
import numpy as np
import pytest

from vcamd import hip

M64 = (1 << 64) - 1


def _mix(t):
    """numpy uint64, wrapping"""
    with np.errstate(over="ignore"):
        t = t + np.uint64(0x9E3779B97F4A7C15)
        t = (t ^ (t >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        t = (t ^ (t >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return t ^ (t >> np.uint64(31))


def reference_hash(words):
    """hash(w[0..count)) = mix(count) + sum_i mix((i << 32) | w[i])  (mod 2^64)"""
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1).astype(np.uint64)
    i = np.arange(w.size, dtype=np.uint64)
    terms = _mix((i << np.uint64(32)) | w)
    with np.errstate(over="ignore"):
        return int(_mix(np.array([w.size], dtype=np.uint64))[0] + terms.sum(dtype=np.uint64))


SPECIAL = np.array([0, 0x80000000, 0x7fc00000, 0xffffffff], dtype=np.uint32)


def _words(count, seed=0):
    w = np.random.default_rng(seed).integers(0, 1 << 32, size=count, dtype=np.uint64).astype(np.uint32)
    w[:: 3] = SPECIAL[np.arange(w[:: 3].size) % 4]            # the special words at every third place, whatever the count
    return w


def test_mix_restatement_against_plain_integers():
    """the numpy restatement itself against Python integers (no wrapping tricks to trust)"""
    def mix(t):
        t = (t + 0x9E3779B97F4A7C15) & M64
        t = ((t ^ (t >> 30)) * 0xBF58476D1CE4E5B9) & M64
        t = ((t ^ (t >> 27)) * 0x94D049BB133111EB) & M64
        return t ^ (t >> 31)
    w = _words(5)
    want = (mix(5) + sum(mix((i << 32) | int(v)) for i, v in enumerate(w))) & M64
    assert reference_hash(w) == want


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 63, 64, 65, 1023, 1025])
def test_host_twin_against_the_formula(count):
    w = _words(count, seed=count)
    assert hip.picture_hash_host(w) == reference_hash(w)
    assert hip.picture_hash_host(w.view(np.int32)) == reference_hash(w)
    assert hip.picture_hash_host(w.view(np.float32)) == reference_hash(w)          # NaN payloads and -0 are words like any other


@pytest.mark.parametrize("word", [int(v) for v in SPECIAL])
def test_special_words_alone(word):
    for count in (1, 4, 65):
        w = np.full(count, word, dtype=np.uint32)
        assert hip.picture_hash_host(w) == reference_hash(w)


def test_every_single_bit_flip_changes_the_hash():
    w = _words(257, seed=11)
    base = reference_hash(w)
    assert hip.picture_hash_host(w) == base
    seen = {base}
    for i in range(257):
        for b in range(32):
            v = w.copy()
            v[i] ^= np.uint32(1 << b)
            h = hip.picture_hash_host(v)
            assert h != base, (i, b)
            assert h == reference_hash(v), (i, b)          # (the restatement says the same of every flip)
            seen.add(h)
    assert len(seen) == 257 * 32 + 1           # (and no two flips collide)


def test_swapping_two_unequal_words_changes_the_hash():
    w = _words(64, seed=3)
    base = hip.picture_hash_host(w)
    for i, j in ((0, 1), (0, 63), (17, 40), (1, 2)):
        assert w[i] != w[j]
        v = w.copy()
        v[i], v[j] = w[j], w[i]
        assert hip.picture_hash_host(v) != base, (i, j)


def test_appending_a_zero_word_changes_the_hash():
    for count in (1, 4, 63):
        w = _words(count, seed=5)
        assert hip.picture_hash_host(np.concatenate([w, np.zeros(1, np.uint32)])) != hip.picture_hash_host(w)
    z = np.zeros(8, dtype=np.uint32)
    assert len({hip.picture_hash_host(z[:k]) for k in range(1, 9)}) == 8       # all-zero pictures of different sizes differ


def test_refusals():
    with pytest.raises(hip.VcError):
        hip.picture_hash_host(np.zeros(4, dtype=np.uint8))
    with pytest.raises(hip.VcError):
        hip.picture_hash_host(np.zeros(4, dtype=np.float64))
    with pytest.raises(hip.VcError):
        hip.picture_hash_host(np.zeros(0, dtype=np.uint32))
    assert {"vc_picture_hash", "vc_picture_hash_host"} <= set(hip.EXPORTED_SYMBOLS)
