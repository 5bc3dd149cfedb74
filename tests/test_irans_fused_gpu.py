"""-m gpu: the fused decode kernels of the interleaved range coder (csrc/rans_device.hip: vc_irans_decode_eb, vc_irans_decode_gc)
against the unfused chains on the same two-segment payload, bit for bit:

    z:  channel index tensor -> vc_irans_decode -> vc_eb_dequant
    y:  vc_gc_indexes        -> vc_irans_decode -> vc_gc_dequant

Payloads come from the host reference (vc_irans_encode_host).  Outputs, scales and means are channel windows or plane windows
of larger sentinel-filled tensors, each with its own geometry; the float output AND symbols_out are compared, the sentinel
around every output must survive.  Every case names the form it must reach -- tables staged in LDS or read from global
memory -- and the condition restated here (2 bytes per entry within 64 KiB, for all three kernels: the Gaussian form opts in to
the 256 bytes of its scale table past 64 KiB) is asserted against vc_irans_tables_in_lds, on both sides of the boundary."""
import numpy as np
import pytest
import torch

from test_irans_cpu import _gaussian_tables, make_set
from vcamd import hip
from vcamd.hip import T

pytestmark = pytest.mark.gpu

SENTINEL = 777.25
SHAPES = ((1, 1), (1, 2), (3, 5))            # (hz, wz); the y grid is four times that
CHANNELS = (128, 5, 16)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _window(kind, n, h, w, c, dev, seed, fill=None):
    """(T window [n,h,w,c], backing tensor, bool mask of the backing's elements outside the window).  ``kind``: "channels" = channels
    c0 .. c0 + c of a wider tensor, "planes" = an h x w window inside larger planes.  ``fill``: values of the window (numpy [n,h,w,c])."""
    k = seed % 3
    if kind == "channels":
        hh, ww, cc, y0, x0, c0 = h, w, c + 3 + k, 0, 0, 1 + k
    else:
        hh, ww, cc, y0, x0, c0 = h + 2 + k, w + 3, c, 1 + k, 2, 0
    backing = torch.full((n, hh, ww, cc), SENTINEL, dtype=torch.float32, device=dev)
    if fill is not None:
        backing[:, y0:y0 + h, x0:x0 + w, c0:c0 + c] = torch.from_numpy(fill).to(dev)
    outside = torch.ones_like(backing, dtype=torch.bool)
    outside[:, y0:y0 + h, x0:x0 + w, c0:c0 + c] = False
    t = T(backing.view(-1), n, h, w, c, hh * ww * cc, ww * cc, cc, (y0 * ww + x0) * cc + c0)
    return t, backing, outside


def _draw_for(rng, tables, idx, escapes):
    """symbols distributed like the table each index names, a fraction ``escapes`` of them outside every table's range"""
    cdfs, sizes, offs = tables
    u = rng.integers(0, 65536, idx.shape)
    sym = np.empty(idx.shape, dtype=np.int32)
    for t in np.unique(idx):
        m = idx == t
        slot = np.minimum(np.searchsorted(cdfs[t, :sizes[t]], u[m], side="right") - 1, sizes[t] - 3)
        sym[m] = slot + offs[t]
    esc = rng.random(idx.shape) < escapes
    sym[esc] = rng.choice([-70000, 70000, 12345, -(2 ** 31), 2 ** 31 - 1], int(esc.sum()))
    return sym


def _scale_table(n):
    from oracle.cai.entropy_models import get_scale_table
    full = np.asarray(get_scale_table(), dtype=np.float32)
    return full if n == 64 else np.ascontiguousarray(full[np.linspace(0, 63, n).astype(int)])


def _entries(tables):
    cdfs, sizes, offs = tables
    return -(-int(np.sum(sizes)) // 8) * 8


class Case:
    """one two-segment payload per image and both ways of decoding it"""

    def __init__(self, dev, seed, n, shape, c, kind, waves, gain, eb, gc, forms):
        rng = np.random.default_rng(seed)
        L = hip.lib()
        self.dev, self.n, self.c, self.kind, self.waves, self.seed = dev, n, c, kind, waves, seed
        self.hz, self.wz = shape
        self.hy, self.wy = 4 * shape[0], 4 * shape[1]
        self.eb, self.gc = eb, gc
        self.eb_dev, self.gc_dev = hip.IransTables(*eb, dev), hip.IransTables(*gc, dev)
        for tables, dt, form in ((eb, self.eb_dev, forms[0]), (gc, self.gc_dev, forms[1])):
            assert dt.entries == _entries(tables)
            assert (2 * dt.entries <= 64 * 1024) == (form == "lds") == bool(L.vc_irans_tables_in_lds(dt.entries)) == dt.in_lds
        n_scales = len(gc[1])
        table = _scale_table(n_scales)
        self.table = torch.from_numpy(table).to(dev)
        # scales: log-uniform across the table, some exactly on entries, some below the first (and the 0.11 bound), some above the last
        s = np.exp(rng.uniform(np.log(0.05), np.log(table[-1] * 2), (n, self.hy, self.wy, c))).astype(np.float32)
        flat = s.reshape(-1)
        on = rng.random(flat.size) < 0.3
        flat[on] = rng.choice(table, int(on.sum()))
        flat[:4] = [0.01, table[0], table[-1], table[-1] * 4][:flat.size]
        means = rng.normal(0, 3, (n, self.hy, self.wy, c)).astype(np.float32)
        self.scales, _, _ = _window(kind, n, self.hy, self.wy, c, dev, seed + 1, s)
        self.means, _, _ = _window("planes" if kind == "channels" else "channels", n, self.hy, self.wy, c, dev, seed + 2, means)
        params = rng.normal(0, 1, (c, hip.EB_PARAMS_PER_CHANNEL)).astype(np.float32)
        self.params = torch.from_numpy(params).to(dev)
        self.gain_z = torch.from_numpy(rng.uniform(0.5, 2, c).astype(np.float32)).to(dev) if gain else None
        self.gain_y = torch.from_numpy(rng.uniform(0.5, 2, c).astype(np.float32)).to(dev) if gain else None
        # the integers: z by channel, y by the indexes the device itself derives from the scales
        self.z_idx = torch.arange(c, dtype=torch.int32, device=dev).view(1, c, 1).expand(n, c, self.hz * self.wz).reshape(n, -1).contiguous()
        self.y_idx = torch.empty((n, c * self.hy * self.wy), dtype=torch.int32, device=dev)
        hip.check(L.vc_gc_indexes(hip.stream(), self.scales.view(), self.table.data_ptr(), n_scales, self.y_idx.data_ptr()), "vc_gc_indexes")
        z_idx_h, y_idx_h = self.z_idx.cpu().numpy(), self.y_idx.cpu().numpy()
        clamped = np.maximum(s, np.float32(0.11)).transpose(0, 3, 1, 2).reshape(n, -1)
        want_idx = (n_scales - 1) - (clamped[..., None] <= table[None, None, :-1]).sum(-1)
        assert np.array_equal(y_idx_h, want_idx) and {0, n_scales - 1} <= set(np.unique(y_idx_h).tolist())
        self.z_sym, self.y_sym = _draw_for(rng, eb, z_idx_h, 0.05), _draw_for(rng, gc, y_idx_h, 0.05)
        self.payloads = [hip.irans_encode_host([(self.z_sym[j], z_idx_h[j], 0), (self.y_sym[j], y_idx_h[j], 1)], [eb, gc], waves)
                         for j in range(n)]

    def outputs(self):
        z = _window(self.kind, self.n, self.hz, self.wz, self.c, self.dev, self.seed + 3)
        y = _window(self.kind, self.n, self.hy, self.wy, self.c, self.dev, self.seed + 4)
        return z, y

    def unfused(self, payloads):
        L = hip.lib()
        (zt, zb, zo), (yt, yb, yo) = self.outputs()
        dec = hip.IransDecoder(payloads, self.waves, self.dev)
        z_sym = dec.decode(self.z_idx, self.eb_dev)
        hip.check(L.vc_eb_dequant(hip.stream(), z_sym.data_ptr(), self.params.data_ptr(), None if self.gain_z is None else self.gain_z.data_ptr(),
                                  zt.view()), "vc_eb_dequant")
        y_sym = dec.decode(self.y_idx, self.gc_dev)
        hip.check(L.vc_gc_dequant(hip.stream(), y_sym.data_ptr(), self.means.view(), None if self.gain_y is None else self.gain_y.data_ptr(),
                                  yt.view()), "vc_gc_dequant")
        return dec, zb, yb, z_sym, y_sym

    def fused(self, payloads):
        (zt, zb, zo), (yt, yb, yo) = self.outputs()
        dec = hip.IransDecoder(payloads, self.waves, self.dev)
        z_sym = torch.full_like(self.z_idx, -99)
        y_sym = torch.full_like(self.y_idx, -99)
        dec.decode_eb(self.eb_dev, self.params, self.gain_z, zt, symbols_out=z_sym)
        dec.decode_gc(self.gc_dev, self.scales, self.means, self.table, self.gain_y, yt, symbols_out=y_sym)
        assert (zb[zo] == SENTINEL).all() and (yb[yo] == SENTINEL).all()           # nothing outside the windows
        assert not (zb[~zo] == SENTINEL).any() and not (yb[~yo] == SENTINEL).any()  # everything inside
        return dec, zb, yb, z_sym, y_sym

    def compare(self, payloads):
        a, b = self.unfused(payloads), self.fused(payloads)
        for x, y in zip(a[1:], b[1:]):
            assert torch.equal(x, y)
        return a, b


TABLE_SETS = {}


def _tables(c, form, which):
    """eb: one table per channel; gc: 64 Gaussian tables (LDS) or a set too large for LDS"""
    key = (c, form, which)
    if key not in TABLE_SETS:
        if which == "gc":
            TABLE_SETS[key] = _gaussian_tables() if form == "lds" else make_set(4, [1200] * 30, ones=7)
        else:
            TABLE_SETS[key] = make_set(30 + c, [40] * c, ones=2) if form == "lds" else make_set(31 + c, [-(-34000 // c)] * c, ones=3)
    return TABLE_SETS[key]


@pytest.mark.parametrize("kind", ["channels", "planes"])
@pytest.mark.parametrize("waves", [1, 4, 16])
def test_fused_kernels_equal_the_unfused_chains(dev, waves, kind):
    k = 0
    for n in (1, 3):
        for shape in SHAPES:
            for c in CHANNELS:
                for form in ("lds", "global"):
                    k += 1
                    case = Case(dev, 1000 * waves + k, n, shape, c, kind, waves, gain=bool((k + n) & 1), eb=_tables(c, form, "eb"),
                                gc=_tables(c, form, "gc"), forms=(form, form))
                    (da, _, _, z_sym, y_sym), (db, *_rest) = case.compare(case.payloads)
                    assert np.array_equal(z_sym.cpu().numpy(), case.z_sym) and np.array_equal(y_sym.cpu().numpy(), case.y_sym)
                    da.finish()
                    db.finish()


@pytest.mark.parametrize("sizes,form", [([1024] * 32, "lds"), ([1024] * 32 + [9], "global")])
def test_both_sides_of_the_lds_boundary(dev, sizes, form):
    """32 768 entries = exactly 64 KiB: staged, and the Gaussian form keeps its scale table in the 256 bytes behind them; one more
    table: 32 784 entries, read from global memory"""
    gc = make_set(5, sizes, ones=3)
    assert _entries(gc) == (32768 if form == "lds" else 32784)
    case = Case(dev, 77, 2, (1, 2), 5, "channels", 4, True, _tables(5, "lds", "eb"), gc, ("lds", form))
    (da, *_), (db, *_) = case.compare(case.payloads)
    da.finish()
    db.finish()


def test_violations_give_the_error_word_and_the_dequantisation_of_zeros(dev):
    """The pair of cases tests/test_irans_gpu.py runs for the unfused kernel: W = 1 with the word count lowered by 40 and the last 40
    words removed (the sub-stream runs out inside the y segment), and a truncated upload (refused by the header walk)."""
    case = Case(dev, 5, 1, (3, 5), 16, "planes", 1, True, _tables(16, "lds", "eb"), _tables(16, "lds", "gc"), ("lds", "lds"))
    good = case.payloads[0]
    count = int(np.frombuffer(good[:4], dtype=np.uint32)[0])
    short = np.array([count - 40], dtype=np.uint32).tobytes() + good[4:len(good) - 160]
    for payload, word in ((short, 2), (good[:len(good) // 2 // 4 * 4], 1)):
        a, b = case.compare([payload])
        for dec in (a[0], b[0]):
            assert dec.states[:4].cpu().numpy().view(np.uint32)[0] == word
        head = 4 * (2 + 5 * 16)                # error, waves and the five per-wave arrays of vc_irans_dstate
        assert torch.equal(a[0].states[:head], b[0].states[:head])
        y_sym = b[4].cpu().numpy()[0]
        if word == 2:                          # decoded as written up to the round of the break, zeros behind it
            start = int(np.argmax(y_sym != case.y_sym[0])) // 64 * 64
            assert 0 < start and np.array_equal(y_sym[:start], case.y_sym[0][:start]) and not y_sym[start:].any()
            assert np.array_equal(b[3].cpu().numpy(), case.z_sym)
        else:
            assert not y_sym.any() and not b[3].any()
        with pytest.raises(hip.VcError):
            b[0].finish()


def test_refused_arguments_write_nothing(dev):
    L = hip.lib()
    case = Case(dev, 9, 2, (1, 2), 5, "channels", 4, False, _tables(5, "lds", "eb"), _tables(5, "lds", "gc"), ("lds", "lds"))
    (zt, zb, _), (yt, yb, _) = case.outputs()
    dec = hip.IransDecoder(case.payloads, 4, dev)
    before = dec.states.clone()
    buf, st, et, gt = dec.buf.data_ptr(), dec.states.data_ptr(), case.eb_dev.struct(), case.gc_dev.struct()
    nz, ny = 5 * 1 * 2, 5 * 4 * 8

    def view(t, **kw):
        v = t.view()
        for k_, val in kw.items():
            setattr(v, k_, val)
        return v

    def eb(payloads=buf, states=st, images=2, waves=4, count=nz, tables=et, params=case.params.data_ptr(), z=None):
        return L.vc_irans_decode_eb(hip.stream(), payloads, states, images, waves, count, tables, params, None, z or zt.view(), None)

    def gc(payloads=buf, states=st, images=2, waves=4, count=ny, tables=gt, sc=None, mu=None, table=case.table.data_ptr(), n_scales=64, y=None):
        return L.vc_irans_decode_gc(hip.stream(), payloads, states, images, waves, count, tables, sc or case.scales.view(),
                                    mu or case.means.view(), table, n_scales, None, y or yt.view(), None)

    bad_tables = hip.IransDTables(None, case.eb_dev.rows.data_ptr(), 5, case.eb_dev.entries)
    eb_calls = [eb(payloads=None), eb(states=None), eb(params=None), eb(z=view(zt, p=None)), eb(images=0), eb(images=3), eb(waves=3),
                eb(count=nz + 1), eb(count=0), eb(z=view(zt, c=0)), eb(z=view(zt, h=-1)), eb(z=view(zt, w=0)), eb(tables=bad_tables)]
    gc_calls = [gc(payloads=None), gc(states=None), gc(table=None), gc(n_scales=1), gc(n_scales=65), gc(sc=view(case.scales, p=None)),
                gc(mu=view(case.means, p=None)), gc(y=view(yt, p=None)), gc(images=1), gc(waves=0), gc(count=ny - 1),
                gc(sc=view(case.scales, h=3)), gc(mu=view(case.means, c=4)), gc(mu=view(case.means, w=7)), gc(y=view(yt, c=0)),
                gc(y=view(yt, h=0))]
    assert all(rc == -1 for rc in eb_calls + gc_calls), (eb_calls, gc_calls)
    torch.cuda.synchronize()
    assert (zb == SENTINEL).all() and (yb == SENTINEL).all() and torch.equal(dec.states, before)
    assert eb() == 0 and gc() == 0                                     # (the same calls with nothing wrong)
    dec.finish()


def test_the_unfused_kernel_still_matches_the_host_reference(dev):
    """vc_irans_decode is one instantiation of the shared round loop: byte for byte what vc_irans_decode_host decodes"""
    for form in ("lds", "global"):
        case = Case(dev, 13, 3, (3, 5), 16, "channels", 4, False, _tables(16, form, "eb"), _tables(16, form, "gc"), (form, form))
        dec, _, _, z_sym, y_sym = case.unfused(case.payloads)
        dec.finish()
        for j, p in enumerate(case.payloads):
            host = hip.irans_decode_host(p, [(case.z_idx[j].cpu().numpy(), 0), (case.y_idx[j].cpu().numpy(), 1)], [case.eb, case.gc], 4)
            assert host[0].tobytes() == z_sym[j].cpu().numpy().tobytes() and host[1].tobytes() == y_sym[j].cpu().numpy().tobytes()
