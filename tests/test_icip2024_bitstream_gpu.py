"""-m gpu: the real bitstream of the ICIP2024 B-frame codec (FlowGuidedB.compress / decompress, _Elic.compress_t / decompress_t,
the container of vcamd/bitstream.py) on the seeded checkpoint of tests/test_icip2024_gpu.py.

The reference has no bitstream for this model, so the checks are closed-loop: the decoder -- which never sees the current frame --
must rebuild the encoder's x_hat, y_hat and z_hat bit for bit, the strings must hold exactly the integers the existing
full-tensor kernel (vc_gc_forward) derives from the encoder's own (scales, means), and the real size must track the device's
-log2 p of those very symbols.

Size band (test_size_tracks_the_estimate).  size / size_estimate was MEASURED on an MI355X for the cases below (seeded weights: most
symbols fall outside the tables' ranges and take the escape path, whose Exp-Golomb bypass bits cost more than the -log2 of the
clamped tail mass the estimate counts -- the band cannot be derived from the coder's precision):
  case        frame      n  down_ratio  s     size (bits)  size_estimate  size / size_estimate
  a           128x192    1  1           1.0   334656       418294.5       0.80005
  b           128x192    1  2           2.5   332896       415766.7       0.80068
  c           128x192    1  4           4.0   329600       411042.9       0.80186
  lhbdc       256x192    1  2           1.5   677984       846381.8       0.80104
  crop_dr1    64x128     1  1           1.5   110336       137730.7       0.80110
  crop_dr16   64x128     1  16          1.5   110016       137489.0       0.80018
  batch2      128x192    2  2           1.0   670240       837808.2       0.79999
(an escaped symbol costs the estimate the clamped 1e-9 = 29.9 bits and the coder about 24: the ratio sits at 0.80 for every case;
size / forward()["size"] was 0.8003 .. 0.8027, printed only -- forward() codes round(y) around other context values.)  Worst
deviation from 1: 0.20001 (batch2), so the chosen bound is 0.40002 * size_estimate + 128 bits per string.
The bound is twice the worst deviation from 1 of that list plus 16 bytes for each of the twelve strings per image (the coder's
flush): | size - size_estimate | <= 2 * WORST_DEVIATION * size_estimate + 8 * 16 * strings.
"""
import numpy as np
import pytest
import torch

from helpers import frame_tensor, load_fixture

pytestmark = pytest.mark.gpu

WORST_DEVIATION = 0.20001        # max | size / size_estimate - 1 | over CASES, measured (module docstring)
FLUSH_BITS_PER_STRING = 8 * 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def prod(dev):
    from vcamd import icip2024
    from vcamd.seeding import seeded_state_dict
    m = icip2024.FlowGuidedB()
    m.load_state_dict(seeded_state_dict(m.state_dict(), seed=1234))
    m = m.to(dev).eval()
    m.offset_compressor.update(force=True)
    m.residual_compressor.update(force=True)
    return m


def _frames(name, dev, crop=None):
    fx = load_fixture(name)
    x1, xc, x2 = (frame_tensor(fx[k]) for k in ("ref_1", "current", "ref_2"))
    if crop is not None:
        x1, xc, x2 = (t[..., :crop[0], :crop[1]].contiguous() for t in (x1, xc, x2))
    return x1.to(dev), xc.to(dev), x2.to(dev)


def _case_inputs(name, dev):
    """(xref1, xref2, scale1, scale2, xcur, s, down_ratio)"""
    if name in ("a", "b", "c"):
        fx = load_fixture("icip2024_forward_a.npz")
        s1, s2, lvl, dr = (float(v) for v in fx[f"cfg_{name}"])
        x1, xc, x2 = _frames("icip2024_forward_a.npz", dev)
        return x1, x2, s1, s2, xc, lvl, int(dr)
    if name == "lhbdc":
        x1, xc, x2 = _frames("lhbdc_forward_b.npz", dev)
        return x1, x2, 0.75, 0.25, xc, 1.5, 2
    if name in ("crop_dr1", "crop_dr16"):
        x1, xc, x2 = _frames("lhbdc_forward_b.npz", dev, crop=(64, 128))
        return x1, x2, 0.75, 0.25, xc, 1.5, int(name[7:])
    if name == "batch2":                                   # image 1: the same triple mirrored and played backwards
        x1, xc, x2 = _frames("icip2024_forward_a.npz", dev)
        return (torch.cat([x1, x2.flip(-1)]), torch.cat([x2, x1.flip(-1)]), 0.5, 0.5, torch.cat([xc, xc.flip(-1)]), 1.0, 2)
    raise KeyError(name)


CASES = ["a", "b", "c", "lhbdc", "crop_dr1", "crop_dr16", "batch2"]


@pytest.fixture(scope="module")
def coded(dev, prod):
    """every case is encoded once (with its trace) and shared by the tests"""
    cache = {}

    def get(name):
        if name not in cache:
            args = _case_inputs(name, dev)
            trace = {}
            with torch.no_grad():
                out = prod.compress(*args, trace=trace)
            cache[name] = (args, out, trace)
        return cache[name]
    return get


def squeeze(t, parity):
    """the squeezed order of the *_ckbd kernels (include/vc_hip.h): parity 1 = anchors ((row + col) odd)"""
    out = np.empty(t.shape[:3] + (t.shape[3] // 2,), dtype=t.dtype)
    out[:, :, 0::2, :] = t[:, :, 0::2, parity::2]
    out[:, :, 1::2, :] = t[:, :, 1::2, (1 - parity)::2]
    return out


def _all_strings(strings):
    return [b for codec in ("offset", "residual") for g in strings[codec][0] for b in g] + \
           [b for codec in ("offset", "residual") for b in strings[codec][1]]


@pytest.mark.parametrize("name", CASES)
def test_decoder_rebuilds_the_encoder(dev, prod, coded, name):
    (x1, x2, s1, s2, xc, lvl, dr), out, te = coded(name)
    n = xc.shape[0]
    assert out["down_ratio"] == dr and tuple(out["shape"]) == (xc.shape[2] // 64, xc.shape[3] // 64)
    for codec in ("offset", "residual"):
        groups, z = out["strings"][codec]
        assert len(groups) == 5 and len(z) == n and all(len(g) == n and all(isinstance(b, bytes) for b in g) for g in groups)
    td = {}
    with torch.no_grad():
        dec = prod.decompress(x1, x2, s1, s2, out["strings"], out["shape"], lvl, out["down_ratio"], trace=td)
    assert set(dec) == {"x_hat"}
    for codec in ("offset", "residual"):
        assert torch.equal(td[codec]["z_hat"], te[codec]["z_hat"]), f"{codec}: z_hat"
        for i in range(5):
            assert torch.equal(td[codec]["y_hat"][i], te[codec]["y_hat"][i]), f"{codec}: y_hat of group {i}"
    assert dec["x_hat"].shape == xc.shape and torch.equal(dec["x_hat"], out["x_hat"])
    assert bool(torch.isfinite(out["x_hat"]).all())


@pytest.mark.parametrize("name", ["lhbdc", "batch2"])
def test_strings_hold_the_symbols_of_the_full_tensor_kernel(dev, prod, coded, name):
    """vc_gc_forward on the encoder's own (y, scales, means) of every pass: its symbols and indexes, squeezed on the host into the
    order the *_ckbd kernels document, are what the group strings decode to -- both parities, every image."""
    from vcamd import hip
    L = hip.lib()
    _, out, te = coded(name)
    for codec, comp in (("offset", prod.offset_compressor), ("residual", prod.residual_compressor)):
        table = comp._scale_table_dev()
        gc_tables = comp.gaussian_conditional.tables()
        per_group = {}
        for p in te[codec]["passes"]:
            y, sc, mu = p["y"], p["scales"], p["means"]
            sym = torch.empty((y.n, y.c, y.h, y.w), dtype=torch.int32, device=dev)
            idx = torch.empty_like(sym)
            hip.check(L.vc_gc_forward(hip.stream(), y.view(), sc.view(), mu.view(), None, None, hip.NULL_VIEW, None, 0, None,
                                      sym.data_ptr(), idx.data_ptr(), table.data_ptr(), table.numel(), None), "vc_gc_forward")
            per_group.setdefault(p["group"], []).append((squeeze(sym.cpu().numpy(), p["parity"]), squeeze(idx.cpu().numpy(), p["parity"])))
        assert sorted(per_group) == [0, 1, 2, 3, 4] and all(len(v) == 2 for v in per_group.values())
        for i, passes in per_group.items():
            for j, string in enumerate(out["strings"][codec][0][i]):
                want = np.concatenate([s[j].reshape(-1) for s, _ in passes])
                index = np.concatenate([ix[j].reshape(-1) for _, ix in passes])
                got = hip.rans_decode(string, index, *gc_tables)
                assert np.array_equal(got, want), f"{codec} group {i} image {j}"


def test_search_path(dev, prod):
    from vcamd import hip
    x1, x2, s1, s2, xc, lvl, _ = _case_inputs("a", dev)
    with torch.no_grad():
        _, choice, _ = prod.search_flow_t(hip.nchw_to_nhwc(xc), hip.nchw_to_nhwc(x1), hip.nchw_to_nhwc(x2), s1, s2, prod.SEARCH_RATIOS)
        best = prod.SEARCH_RATIOS[int(choice.item())]
        out = prod.compress(x1, x2, s1, s2, xc, lvl)
        assert out["down_ratio"] == best == int(load_fixture("icip2024_forward_a.npz")["best_down_ratio"])
        dec = prod.decompress(x1, x2, s1, s2, out["strings"], out["shape"], lvl, out["down_ratio"])
    assert torch.equal(dec["x_hat"], out["x_hat"])


@pytest.mark.parametrize("name", CASES)
def test_size_tracks_the_estimate(dev, prod, coded, name):
    (x1, x2, s1, s2, xc, lvl, dr), out, _ = coded(name)
    strings = _all_strings(out["strings"])
    assert len(strings) == 12 * xc.shape[0]
    assert out["size"] == 8 * sum(len(b) for b in strings)
    est = out["size_estimate"]
    assert est > 0 and np.isfinite(est)
    with torch.no_grad():
        fwd = prod(x1, x2, s1, s2, xc, lvl, dr)
    ratio = out["size"] / est
    print(f"{name}: size {out['size']} bits, size_estimate {est:.1f}, size / size_estimate = {ratio:.5f}, "
          f"size / forward()['size'] = {out['size'] / fwd['size'].item():.5f}")
    assert abs(out["size"] - est) <= 2 * WORST_DEVIATION * est + FLUSH_BITS_PER_STRING * len(strings)


@pytest.mark.parametrize("name", ["lhbdc", "batch2"])
def test_container_round_trip(dev, prod, coded, name):
    """one container per image; the strings that come back out of the containers decode to what the direct decode gives"""
    from vcamd import bitstream
    (x1, x2, s1, s2, xc, lvl, dr), out, _ = coded(name)
    c1, c2 = prod.convert_scales(s1, s2)
    n = xc.shape[0]
    back = []
    for j in range(n):
        blob = bitstream.pack_icip2024_frame(out["strings"], out["shape"], out["down_ratio"], lvl, c1, c2, image=j)
        got = bitstream.unpack_icip2024_frame(blob)
        assert got["shape"] == tuple(out["shape"]) and got["down_ratio"] == dr
        assert (got["s"], got["scale1"], got["scale2"]) == (lvl, c1, c2)
        for codec in ("offset", "residual"):
            assert got["strings"][codec][1] == [out["strings"][codec][1][j]]
            assert got["strings"][codec][0] == [[g[j]] for g in out["strings"][codec][0]]
        assert len(blob) == 70 + sum(len(b) for b in _all_strings(got["strings"]))
        back.append(got)
    strings = {c: [[[b["strings"][c][0][i][0] for b in back] for i in range(5)], [b["strings"][c][1][0] for b in back]]
               for c in ("offset", "residual")}
    with torch.no_grad():
        dec = prod.decompress(x1, x2, back[0]["scale1"], back[0]["scale2"], strings, back[0]["shape"], back[0]["s"], back[0]["down_ratio"])
        direct = prod.decompress(x1, x2, s1, s2, out["strings"], out["shape"], lvl, dr)
    assert torch.equal(dec["x_hat"], direct["x_hat"]) and torch.equal(dec["x_hat"], out["x_hat"])


def test_decoder_refuses_what_does_not_fit(dev, prod, coded):
    from vcamd import hip
    (x1, x2, s1, s2, xc, lvl, dr), out, _ = coded("crop_dr1")
    with pytest.raises(hip.VcError):
        prod.decompress(x1, x2, s1, s2, out["strings"], (2, 2), lvl, dr)                 # shape of another frame size
    with pytest.raises(hip.VcError):
        prod.decompress(x1, x2, s1, s2, out["strings"], out["shape"], lvl, 3)            # not a flow resolution
    with pytest.raises(hip.VcError):
        prod.decompress(x1, x2, s1, s2, {"offset": out["strings"]["offset"]}, out["shape"], lvl, dr)
    with pytest.raises(hip.VcError):
        prod.decompress(x1.cpu(), x2.cpu(), s1, s2, out["strings"], out["shape"], lvl, dr)
