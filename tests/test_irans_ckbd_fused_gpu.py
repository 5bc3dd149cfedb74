"""-m gpu: the fused checkerboard decode of the interleaved range coder (csrc/rans_device.hip: vc_irans_decode_gc_ckbd) against
the chain it replaces, bit for bit, on one parity of NHWC views:

    vc_gc_indexes_ckbd -> vc_irans_decode -> vc_gc_dequant_ckbd

Payloads come from the host reference (vc_irans_encode_host): one segment, the symbols of the parity in the squeezed order
[c][h][w/2].  Compared: y_hat (the whole backing tensor, so the other parity and everything outside a channel window must keep
its sentinel bit pattern), symbols_out and the final vc_irans_dstate bytes.  Scales straddle the 0.11 bound and both ends of the
scale table; symbols include escapes and negative values."""
import numpy as np
import pytest
import torch

from test_irans_cpu import _gaussian_tables, make_set
from test_irans_fused_gpu import _draw_for, _entries, _scale_table
from vcamd import hip
from vcamd.hip import T

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-1234.5625)
# (n, h, w, c), (channels of the backing tensor, first channel of the window)
SHAPES = (((2, 5, 6, 16), (40, 8)),        # odd h, a channel window; 240 symbols: less than one round at W = 16
          ((1, 7, 10, 24), (24, 0)),       # 840 symbols: a ragged last round
          ((2, 8, 12, 32), (32, 0)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _window(values, cc, c0, dev):
    """T window [n,h,w,c] at channels c0.. of a sentinel-filled [n,h,w,cc] tensor holding ``values`` (None: sentinel only)"""
    n, h, w, c = values if isinstance(values, tuple) else values.shape
    backing = torch.full((n, h, w, cc), float(SENTINEL), dtype=torch.float32, device=dev)
    if not isinstance(values, tuple):
        backing[..., c0:c0 + c] = torch.from_numpy(values).to(dev)
    return T(backing.view(-1), n, h, w, c, h * w * cc, w * cc, cc, c0), backing


def _squeeze(full, parity):
    """[n,h,w,c] -> squeezed order [n, c*h*(w/2)] of one parity: column 2 xs + ((y ^ parity) & 1)"""
    n, h, w, c = full.shape
    ys = np.arange(h)[:, None]
    xs = 2 * np.arange(w // 2)[None, :] + ((ys ^ parity) & 1)
    return np.ascontiguousarray(full[:, ys, xs, :].transpose(0, 3, 1, 2)).reshape(n, -1)


class Case:
    def __init__(self, dev, seed, shape, window, parity, waves, gc, gain):
        rng = np.random.default_rng(seed)
        n, h, w, c = shape
        self.dev, self.shape, self.window, self.parity, self.waves, self.gc = dev, shape, window, parity, waves, gc
        self.gc_dev = hip.IransTables(*gc, dev)
        self.count = c * h * (w // 2)
        n_scales = len(gc[1])
        table = _scale_table(n_scales)
        self.table = torch.from_numpy(table).to(dev)
        s = np.exp(rng.uniform(np.log(0.05), np.log(table[-1] * 2), shape)).astype(np.float32)
        flat = s.reshape(-1)
        on = rng.random(flat.size) < 0.3
        flat[on] = rng.choice(table, int(on.sum()))
        near = rng.random(flat.size) < 0.1                               # either side of the lower bound
        flat[near] = rng.choice(np.float32([0.1, 0.10999999, 0.11, 0.11000001, 0.12]), int(near.sum()))
        for y in range(2):                                               # both parities see both ends of the table
            s[0, y, :4, 0] = [0.01, table[0], table[-1], table[-1] * 4]
            s[0, y, :4, 1] = [table[-1] * 4, table[-1], 0.01, table[0]]
        means = rng.normal(0, 3, shape).astype(np.float32)
        cc, c0 = window
        self.scales, _ = _window(s, cc + 1, min(c0, 1), dev)            # every view has a geometry of its own
        self.means, _ = _window(means, cc, c0, dev)
        self.gain = torch.from_numpy(rng.uniform(0.5, 2, c).astype(np.float32)).to(dev) if gain else None
        clamped = np.maximum(_squeeze(s, parity), np.float32(0.11))
        self.idx_h = ((n_scales - 1) - (clamped[..., None] <= table[None, None, :-1]).sum(-1)).astype(np.int32)
        assert {0, n_scales - 1} <= set(np.unique(self.idx_h).tolist())
        self.sym_h = _draw_for(rng, gc, self.idx_h, 0.05)
        assert (self.sym_h < 0).any() and (np.abs(self.sym_h.astype(np.int64)) >= 12345).any()
        self.payloads = [hip.irans_encode_host([(self.sym_h[j], self.idx_h[j], 0)], [gc], waves) for j in range(n)]

    def _gain_ptr(self):
        return None if self.gain is None else self.gain.data_ptr()

    def chain(self, payloads):
        L = hip.lib()
        n = self.shape[0]
        yt, yb = _window(self.shape, *self.window, self.dev)
        dec = hip.IransDecoder(payloads, self.waves, self.dev)
        idx = torch.full((n, self.count), -5, dtype=torch.int32, device=self.dev)
        hip.check(L.vc_gc_indexes_ckbd(hip.stream(), self.scales.view(), self.parity, self.table.data_ptr(), self.table.numel(),
                                       idx.data_ptr()), "vc_gc_indexes_ckbd")
        sym = dec.decode(idx, self.gc_dev)
        hip.check(L.vc_gc_dequant_ckbd(hip.stream(), sym.data_ptr(), self.means.view(), self._gain_ptr(), self.parity, yt.view()),
                  "vc_gc_dequant_ckbd")
        return dec, yb, sym, idx

    def fused(self, payloads):
        yt, yb = _window(self.shape, *self.window, self.dev)
        dec = hip.IransDecoder(payloads, self.waves, self.dev)
        sym = torch.full((self.shape[0], self.count), -99, dtype=torch.int32, device=self.dev)
        dec.decode_gc_ckbd(self.gc_dev, self.scales, self.means, self.parity, self.table, self.gain, yt, symbols_out=sym)
        return dec, yb, sym

    def check_untouched(self, yb):
        """the other parity and the channels outside the window keep the sentinel's bits; the coded parity holds none"""
        n, h, w, c = self.shape
        cc, c0 = self.window
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
        coded = torch.from_numpy(((xs ^ ys ^ self.parity) & 1) == 0).to(self.dev)        # x & 1 == (y ^ parity) & 1
        inside = torch.zeros((n, h, w, cc), dtype=torch.bool, device=self.dev)
        inside[..., c0:c0 + c] = coded[None, :, :, None]
        bits = yb.view(torch.int32)
        sentinel = int(np.float32(SENTINEL).view(np.int32))
        assert (bits[~inside] == sentinel).all() and not (bits[inside] == sentinel).any()

    def compare(self, payloads):
        a, b = self.chain(payloads), self.fused(payloads)
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2])
        # the final vc_irans_dstate of every image: error, waves, the five per-wave arrays and the states of the W waves in use (the
        # pad words and the states of the other waves are never written by anyone)
        head, x0 = 4 * (2 + 5 * 16), 4 * (2 + 5 * 16 + 2)
        sa, sb = (d.states.view(d.images, hip.IRANS_STATE_BYTES) for d in (a[0], b[0]))
        assert torch.equal(sa[:, :head], sb[:, :head]) and torch.equal(sa[:, x0:x0 + 512 * self.waves], sb[:, x0:x0 + 512 * self.waves])
        self.check_untouched(b[1])
        return a, b


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("waves", [1, 4, 16])
def test_fused_equals_the_chain(dev, waves, parity):
    gc = _gaussian_tables()
    for k, (shape, window) in enumerate(SHAPES):
        case = Case(dev, 100 * waves + 10 * parity + k, shape, window, parity, waves, gc, gain=bool(k & 1))
        (da, _, sym, idx), (db, _, _) = case.compare(case.payloads)
        assert np.array_equal(idx.cpu().numpy(), case.idx_h) and np.array_equal(sym.cpu().numpy(), case.sym_h)
        da.finish()
        db.finish()


@pytest.mark.parametrize("sizes,form", [([1024] * 32, "lds"), ([1024] * 32 + [9], "global")])
def test_both_sides_of_the_lds_boundary(dev, sizes, form):
    """32 768 entries = exactly 64 KiB: staged, the scale table in the 256 bytes behind them; one more table: global memory"""
    gc = make_set(5, sizes, ones=3)
    assert _entries(gc) == (32768 if form == "lds" else 32784)
    for parity in (0, 1):
        case = Case(dev, 77 + parity, (2, 5, 6, 16), (40, 8), parity, 4, gc, True)
        assert case.gc_dev.in_lds == (form == "lds") == bool(hip.lib().vc_irans_tables_in_lds(case.gc_dev.entries))
        (da, _, sym, _), (db, *_) = case.compare(case.payloads)
        assert np.array_equal(sym.cpu().numpy(), case.sym_h)
        da.finish()
        db.finish()


def test_truncated_payload_gives_the_error_word_and_the_dequantisation_of_zeros(dev):
    """The cases of tests/test_irans_fused_gpu.py: W = 1 with the word count lowered and the last words removed (the sub-stream runs out
    inside the segment), and a truncated upload (refused by the header walk)."""
    case = Case(dev, 5, (1, 7, 10, 24), (24, 0), 1, 1, _gaussian_tables(), True)
    good = case.payloads[0]
    count = int(np.frombuffer(good[:4], dtype=np.uint32)[0])
    assert count > 60
    short = np.array([count - 40], dtype=np.uint32).tobytes() + good[4:len(good) - 160]
    for payload, word in ((short, 2), (good[:len(good) // 2 // 4 * 4], 1)):
        a, b = case.compare([payload])
        for dec in (a[0], b[0]):
            assert dec.states[:4].cpu().numpy().view(np.uint32)[0] == word
        sym = b[2].cpu().numpy()[0]
        if word == 2:
            start = int(np.argmax(sym != case.sym_h[0])) // 64 * 64
            assert 0 < start and np.array_equal(sym[:start], case.sym_h[0][:start]) and not sym[start:].any()
        else:
            assert not sym.any()
            # the de-quantisation of zeros: what the chain's last kernel writes for an all-zero symbol tensor
            yt, yb = _window(case.shape, *case.window, dev)
            zero = torch.zeros((1, case.count), dtype=torch.int32, device=dev)
            hip.check(hip.lib().vc_gc_dequant_ckbd(hip.stream(), zero.data_ptr(), case.means.view(), case.gain.data_ptr(), 1, yt.view()),
                      "vc_gc_dequant_ckbd")
            assert torch.equal(yb.view(torch.int32), b[1].view(torch.int32))
        with pytest.raises(hip.VcError):
            b[0].finish()


def test_refused_arguments_write_nothing(dev):
    L = hip.lib()
    case = Case(dev, 9, (2, 5, 6, 16), (40, 8), 0, 4, _gaussian_tables(), False)
    yt, yb = _window(case.shape, *case.window, dev)
    dec = hip.IransDecoder(case.payloads, 4, dev)
    before = dec.states.clone()
    sym = torch.full((2, case.count), -99, dtype=torch.int32, device=dev)

    def view(t, **kw):
        v = t.view()
        for k_, val in kw.items():
            setattr(v, k_, val)
        return v

    def call(payloads=dec.buf.data_ptr(), states=dec.states.data_ptr(), images=2, waves=4, count=case.count, tables=None, sc=None, mu=None,
             parity=0, table=case.table.data_ptr(), n_scales=64, y=None):
        return L.vc_irans_decode_gc_ckbd(hip.stream(), payloads, states, images, waves, count, tables or case.gc_dev.struct(),
                                         sc or case.scales.view(), mu or case.means.view(), parity, table, n_scales, None, y or yt.view(),
                                         sym.data_ptr())

    bad_tables = hip.IransDTables(None, case.gc_dev.rows.data_ptr(), 64, case.gc_dev.entries)
    odd = dict(w=5)
    calls = [call(payloads=None), call(states=None), call(table=None), call(tables=bad_tables), call(sc=view(case.scales, p=None)),
             call(mu=view(case.means, p=None)), call(y=view(yt, p=None)),
             call(sc=view(case.scales, **odd), mu=view(case.means, **odd), y=view(yt, **odd), count=16 * 5 * 2),      # w odd
             call(parity=2), call(parity=-1), call(count=case.count - 1), call(count=2 * case.count), call(count=0),
             call(sc=view(case.scales, h=4)), call(mu=view(case.means, c=15)), call(mu=view(case.means, w=8)), call(y=view(yt, c=8)),
             call(images=1), call(images=3), call(waves=3), call(waves=0), call(n_scales=1), call(n_scales=65)]
    assert all(rc == -1 for rc in calls), calls
    torch.cuda.synchronize()
    assert (yb == float(SENTINEL)).all() and (sym == -99).all() and torch.equal(dec.states, before)
    assert call() == 0                                                 # (the same call with nothing wrong)
    dec.finish()
    assert np.array_equal(sym.cpu().numpy(), case.sym_h)
