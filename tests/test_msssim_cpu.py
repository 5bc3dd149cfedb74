"""No GPU: the host side of the MS-SSIM metric -- argument checks of the C entry (refused before any launch, so a null stream and
made-up device addresses are never touched), the workspace size, the record plumbing (summarize / RdTable / gather_records) and
the CLI flag."""
import ctypes

import pytest
import torch

from vcamd import gop as vgop
from vcamd import hip

VC_EINVAL = -1
FAKE = 0x1000          # a non-null "device address": every call below must be refused before anything dereferences it


def _call(L, a=FAKE, b=FAKE, n=1, c=3, H=192, W=256, h=161, w=163, pitch=None, quantize=1, ws=FAKE, ws_bytes=None, terms=None, out=FAKE):
    if pitch is None:
        pitch = c * H * W
    if ws_bytes is None:
        ws_bytes = L.vc_msssim_workspace_bytes(n, c, h, w)
    return L.vc_msssim(None, a, b, n, c, H, W, h, w, pitch, quantize, ws, ws_bytes, terms, out)


@pytest.mark.parametrize("bad", [
    dict(a=None), dict(b=None), dict(ws=None), dict(out=None),
    dict(n=0), dict(n=-1), dict(c=0),
    dict(h=193), dict(w=257),
    dict(h=160), dict(w=160), dict(h=160, w=160),
    dict(quantize=2), dict(quantize=-1),
    dict(ws_bytes=0), dict(ws_bytes=1023),
])
def test_c_entry_refuses_before_any_launch(bad):
    L = hip.lib()
    if "ws_bytes" in bad and bad["ws_bytes"]:
        assert L.vc_msssim_workspace_bytes(1, 3, 161, 163) > bad["ws_bytes"]
    assert _call(L, **bad) == VC_EINVAL


def test_workspace_one_byte_short_is_refused():
    L = hip.lib()
    need = L.vc_msssim_workspace_bytes(2, 3, 270, 180)
    assert need > 0
    assert _call(L, n=2, H=320, W=192, h=270, w=180, ws_bytes=need - 1) == VC_EINVAL


def test_workspace_grows_with_n_and_holds_the_pyramids():
    L = hip.lib()
    sizes = [L.vc_msssim_workspace_bytes(n, 3, 1080, 1920) for n in (1, 2, 3, 8)]
    assert all(b > a > 0 for a, b in zip(sizes, sizes[1:]))
    assert sizes[1] - sizes[0] == sizes[2] - sizes[1]
    # pooled planes of both images: 540x960 + 270x480 + 135x240 + 68x120 floats per channel, at least
    assert sizes[0] >= 2 * 3 * 4 * (540 * 960 + 270 * 480 + 135 * 240 + 68 * 120)
    assert L.vc_msssim_workspace_bytes(1, 3, 160, 1920) == 0 and L.vc_msssim_workspace_bytes(0, 3, 1080, 1920) == 0


def _rows(width):
    base = [[0, 1, 2, 30.0, 1000.0, 100.0, 0, 0.95], [0, 2, 1, 32.0, 3000.0, 100.0, 0, 0.97], [0, 8, -1, 40.0, 9000.0, 100.0, 1, 0.99]]
    return torch.tensor([r[:width] for r in base], dtype=torch.float64)


def test_summarize_adds_msssim_only_for_eight_columns():
    s8 = vgop.summarize(_rows(8))
    assert s8 == {"frames": 3, "bpp": 13000.0 / 300.0, "psnr": 102.0 / 3, "msssim": (0.95 + 0.97 + 0.99) / 3}
    for width in (6, 7):
        assert vgop.summarize(_rows(width)) == {"frames": 3, "bpp": 13000.0 / 300.0, "psnr": 102.0 / 3}
    assert "msssim" not in vgop.summarize(torch.zeros((0, 8), dtype=torch.float64))


def test_rdtable_groups_carry_msssim_only_for_eight_columns():
    t8 = vgop.RdTable()
    t8.extend_from_records(_rows(8).tolist(), level=3)
    got = t8.per_level()
    assert got == {3: {"psnr": 102.0 / 3, "bpp": 13000.0 / 300.0, "frames": 3, "msssim": (0.95 + 0.97 + 0.99) / 3}}
    assert t8.per_level_frame_type()[(3, "I")] == {"psnr": 40.0, "bpp": 90.0, "frames": 1, "msssim": 0.99}
    for width in (6, 7):
        t = vgop.RdTable()
        t.extend_from_records(_rows(width).tolist(), level=3)
        assert t.per_level() == {3: {"psnr": 102.0 / 3, "bpp": 13000.0 / 300.0, "frames": 3}}
        assert all(len(r) == 7 for r in t.rows)
    t = vgop.RdTable()
    t.update("B", 1, 0, 0, 30.0, 1000.0, 100.0)                   # the positional call of today's callers
    t.update("B", 2, 0, 0, 32.0, 1000.0, 100.0, msssim=0.9)
    assert "msssim" not in t.per_level()[0]                       # a group with a row that lacks the value reports none


def test_gather_records_width_eight_single_process():
    recs = [(0, 5, 2, torch.tensor(31.0, dtype=torch.float64), torch.tensor(10.0), 100.0, 0, torch.tensor(0.96, dtype=torch.float64)),
            (0, 1, 2, torch.tensor(30.0, dtype=torch.float64), torch.tensor(20.0), 100.0, 0, torch.tensor(0.95, dtype=torch.float64))]
    rows = vgop.gather_records(recs, torch.device("cpu"))
    assert rows.shape == (2, 8) and rows[:, 1].tolist() == [1.0, 5.0] and rows[:, 7].tolist() == [0.95, 0.96]
    assert vgop.summarize(rows)["msssim"] == (0.95 + 0.96) / 2


def test_code_workload_passes_extended_records_and_intra_tails():
    plan = vgop.workload_plan([17], gop_size=8, test_size=0)

    def intra(video, idx):
        return ("dec", idx), (40.0, 9000.0, 100.0, 0.99)

    def code_gops(items, bounds):
        return [(v, g * 8 + 4, 0, 30.0, 1000.0, 100.0, 0, 0.95) for v, g, _ in items]

    recs = vgop.code_workload(plan, 1, 0, intra, code_gops)
    assert all(len(r) == 8 for r in recs)
    assert [r for r in recs if r[6] == 1][0] == (0, 0, -1, 40.0, 9000.0, 100.0, 1, 0.99)
    assert [r for r in recs if r[6] == 0] == [(0, 4, 0, 30.0, 1000.0, 100.0, 0, 0.95), (0, 12, 0, 30.0, 1000.0, 100.0, 0, 0.95)]
    # today's layout: 3-element tails and 6-field records give 7-field records
    old = vgop.code_workload(plan, 1, 0, lambda v, i: (("dec", i), (40.0, 9000.0, 100.0)),
                             lambda items, bounds: [(v, g * 8 + 4, 0, 30.0, 1000.0, 100.0) for v, g, _ in items])
    assert all(len(r) == 7 for r in old) and old[0] == (0, 0, -1, 40.0, 9000.0, 100.0, 1)


def test_cli_accepts_msssim_flag():
    from vcamd import cli
    ap = cli.build_parser()
    assert ap.parse_args(["test", "--msssim"]).msssim is True
    assert ap.parse_args(["test"]).msssim is False


def test_binding_refuses_cpu_tensors_without_a_device():
    x = torch.zeros(1, 3, 192, 256)
    with pytest.raises(hip.VcError):
        hip.msssim_uint8(x, x, 161, 163)
    assert {"vc_msssim", "vc_msssim_workspace_bytes"} <= set(hip.EXPORTED_SYMBOLS)
    assert ctypes.sizeof(ctypes.c_size_t) == 8
