"""CPU: the host side of the ICIP2023 DeformB path (vcamd/icip2023.py) -- state_dict schema against the one recorded from the
reference, the ICIP2024 classes unchanged by their new parameters, the shared ``src.model.m`` import path, refusals, and the 3x3
transposed convolution of the reconstructor restated as a sub-pixel convolution.  None of it needs the built library."""
import os

import pytest
import torch

from helpers import GOLDEN
from vcamd import hip, icip2023, icip2024, layers
from vcamd.seeding import seeded_state_dict


def _schema(name):
    return [l.strip() for l in open(os.path.join(GOLDEN, name))]


def test_state_dict_schema_equals_reference_schema():
    ref = _schema("icip2023_state_schema.txt")
    mine = sorted(f"{k} {list(v.shape)}" for k, v in icip2023.DeformB().state_dict().items())
    assert mine == ref and len(mine) == 1034
    assert sum(v.numel() for k, v in icip2023.DeformB().state_dict().items()) > 70e6


def test_reference_shaped_checkpoint_loads_strict():
    """a checkpoint built from the recorded names and shapes alone (what torch.load of the reference's file gives)"""
    sd = {}
    for line in _schema("icip2023_state_schema.txt"):
        name, shape = line.split(" ", 1)
        sd[name] = torch.zeros([int(v) for v in shape.strip("[]").split(",") if v.strip()])
    model = icip2023.DeformB()
    model.load_state_dict(sd, strict=True)
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=7), strict=True)
    for name in ("feature_extractor", "offset_temp_encoder", "offset_compressor", "reconstructor", "residual_temp_encoder",
                 "residual_compressor") + tuple(f"deconv_l{l}_{r}" for l in (1, 2, 3) for r in (1, 2)):
        assert hasattr(model, name), name
    assert model.deconv_l3_1.weight.shape == (96, 12, 3, 3) and model.deconv_l1_2.groups == 8


def test_icip2024_classes_keep_their_schema():
    """the parameters DeformB needed (feature widths, the g_a0 stem, the reconstructor's upsampling layer) change nothing at the
    ICIP2024 arguments"""
    ref = _schema("icip2024_state_schema.txt")
    mine = sorted(f"{k} {list(v.shape)}" for k, v in icip2024.FlowGuidedB().state_dict().items())
    assert mine == ref and len(mine) == 1126
    assert not hasattr(icip2024.Res_ELIC(), "g_a0") and hasattr(icip2023.Res_ELIC(), "g_a0")
    assert icip2024.Offset_ELIC().g_a1[0].in_channels == 320 and icip2023.Offset_ELIC().g_a1[0].in_channels == 96
    assert icip2023.Res_ELIC().g_a1[0].in_channels == 128 + 96


def test_shared_import_path_resolves_both_models():
    """ICIP2023/src/test.py:159 calls ``m.DeformB()``, ICIP2024's ``m.FlowGuidedB()``: one module path, both classes"""
    from src.model import m
    assert m.DeformB is icip2023.DeformB and m.FlowGuidedB is icip2024.FlowGuidedB


def test_no_cpu_path_and_no_unpadded_frames():
    model = icip2023.DeformB()
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(hip.VcError):
        model(x, x, x, 1)
    with pytest.raises(hip.VcError):
        model.compress(x, x, x, 1)
    with pytest.raises(hip.VcError):
        model.decompress(x, x, {"offset": [], "residual": []}, (1, 1), 1)
    y = torch.zeros(1, 3, 72, 64)
    with pytest.raises(hip.VcError):
        model(y, y, y, 1)


@pytest.mark.parametrize("k,p", [(3, 1), (5, 2)])
def test_transposed_convolution_as_subpixel_convolution(k, p):
    """layers.deconv_as_subpel_weights: ConvTranspose2d(k, stride 2, padding p, output_padding 1) == conv3x3(pad 1) to 4 * cout
    channels + PixelShuffle(2), for the reconstructor's k = 3 as for the codecs' k = 5 (float64: exact up to summation order)"""
    g = torch.Generator().manual_seed(k)
    dc = torch.nn.ConvTranspose2d(6, 5, kernel_size=k, stride=2, padding=p, output_padding=1).double()
    with torch.no_grad():
        dc.weight.copy_(torch.randn(dc.weight.shape, generator=g, dtype=torch.float64))
        dc.bias.copy_(torch.randn(5, generator=g, dtype=torch.float64))
    x = torch.randn(2, 6, 7, 9, generator=g, dtype=torch.float64)
    w3, b3 = layers.deconv_as_subpel_weights(dc)                  # (float32 copies of the weights)
    got = torch.nn.functional.pixel_shuffle(torch.nn.functional.conv2d(x, w3.double(), b3.double(), padding=1), 2)
    # the same tap table restated from the float64 layer: the helper's weights are its float32 roundings, and it is exact
    w64 = torch.zeros(5, 2, 2, 6, 3, 3, dtype=torch.float64)
    for dy in range(2):
        for dx in range(2):
            for jy in range(3):
                for jx in range(3):
                    ky, kx = p + 2 - 2 * jy + dy, p + 2 - 2 * jx + dx
                    if 0 <= ky < k and 0 <= kx < k:
                        w64[:, dy, dx, :, jy, jx] = dc.weight[:, :, ky, kx].t()
    assert torch.equal(w3, w64.reshape(20, 6, 3, 3).float())
    want = dc(x)
    assert got.shape == want.shape and (got - want).abs().max().item() < 1e-5
    exact = torch.nn.functional.pixel_shuffle(torch.nn.functional.conv2d(x, w64.reshape(20, 6, 3, 3), dc.bias.repeat_interleave(4), padding=1), 2)
    assert (exact - want).abs().max().item() < 1e-12
