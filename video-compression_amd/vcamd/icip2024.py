"""ICIP2024 flow-guided deformable B-frame codec on MI355X -- host-side mirror of the reference surface.

Drop-in for (under /root/reference/ICIP2024/src):
  model/m.py:31-282                        FlowGuidedB                      -> :class:`FlowGuidedB`
  model/helpers.py:35-259                  OffsetDiversity, MS_Feature, FlowNET, OffsetTemproalEnc,
                                           ResidualTemproalEnc, Reconstuctor -> same names
  model/elic.py:69-83                      ResidualBottleneckBlock          -> same name
  model/layers.py:6-29                     CheckerboardContext              -> same name
  model/compression_bottlenecks.py:72-551  Offset_ELIC / Res_ELIC           -> same names
  model/elic.py:85-260                     ELIC intra codec (forward / rate estimate, via utils.image_compress) -> :class:`ELIC`
  opt_helpers.py:23-51                     prediction_flowonly, get_best_down_ratio_prediction
  utils.py:153-250                         select_references, update_buffer, get_order_typ_list, get_scales
Attribute names reproduce the reference's state_dict keys (1126 entries, tests/golden/icip2024_state_schema.txt),
including the never-executed g_a / g_s / context_prediction members the compressors inherit from CompressAI's
JointAutoregressiveHierarchicalPriors.  The modules only hold parameters; compute goes through libvc_hip.so.

torch.cat of the reference is never materialised at 1/2 and 1/4 resolution: producers write straight into channel
slices of the concat buffers, and a convolution over ``cat([a, b])`` whose operands live in different buffers runs
as two launches (weights split along the input channels, the second accumulating through the residual input).
The reference has no compress() for this model (rate = likelihood estimate only).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import hip
from .hip import T
from .layers import (GDN, BitCounter, EntropyBottleneck, GaussianConditional, _Prepared, conv1x1, conv3x3, pack_conv,
                     run_sequential, subpel_conv3x3)
from .lhbdc import _require_cuda, _require_frames


def conv(in_channels, out_channels, kernel_size=5, stride=2):
    return nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=kernel_size // 2)


def deconv(in_channels, out_channels, kernel_size=5, stride=2):
    return nn.ConvTranspose2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride,
                              output_padding=stride - 1, padding=kernel_size // 2)


class ResidualBottleneckBlock(_Prepared):
    """1x1 -> ReLU -> 3x3 -> ReLU -> 1x1, plus identity (elic.py:69-83); the add rides in the last epilogue."""
    vc_block = True

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.BottleneckBlock = nn.Sequential(conv1x1(in_ch, out_ch), nn.ReLU(inplace=True), conv3x3(out_ch, out_ch),
                                             nn.ReLU(inplace=True), conv1x1(out_ch, out_ch))

    def _pack(self):
        if self._packed is None:
            b = self.BottleneckBlock
            self._packed = (pack_conv(b[0]), pack_conv(b[2]), pack_conv(b[4]))
        return self._packed

    def half_stream_ok(self):
        """fp16 path: the block can take its input -- first layer's operand AND the identity -- as a half-precision tensor
        and hand its result on as one (hip.HALF_RESIDUAL; the streaming 1x1 kernel adds the half identity)."""
        c1, c2, c3 = self._pack()
        return hip.HALF_RESIDUAL and hip.HALF_ACTIVATIONS and c1.half_ok and c2.half_ok and c3.half_res_ok and c3.cout % 8 == 0

    def run(self, x, out=None, out_f16=False):
        c1, c2, c3 = self._pack()
        if x.dtype == "f16" and not self.half_stream_ok():
            raise hip.VcError("a half-precision tensor reached a bottleneck block that keeps its identity path in fp32")
        t = c1(x, act=hip.ACT_RELU, out_f16=c2.half_ok, out_sp3=hip.wants_split(c2, x))        # both intermediates feed one convolution each:
        if t.dtype == "f16" and c2.can_fuse_tail(c3) and (x.dtype == "f32" or self.half_stream_ok()):
            # fp16 path, 128 channels: the trailing 1x1 + identity in the 3x3 layer's epilogue (hip.FUSE_TAIL) -- the 3x3
            # layer's output (rounded to half exactly as it would be stored) never leaves the CU
            try:
                return c2(t, act=hip.ACT_RELU, tail=c3, res=x, out=out, out_f16=bool(out_f16 and out is None and self.half_stream_ok()))
            except hip.VcError as e:           # (views the fused launch cannot take -- unaligned slices: the two launches below can)
                if "VC_EINVAL" not in str(e):
                    raise
        t = c2(t, act=hip.ACT_RELU, out_f16=c3.half_ok)        # half-precision storage on the fp16 path
        return c3(t, res=x, out=out, out_f16=bool(out_f16 and out is None and self.half_stream_ok()))


def _rbb(c, n=3):
    return [ResidualBottleneckBlock(c, c) for _ in range(n)]


class CheckerboardContext(nn.Conv2d):
    """layers.py:6-29: 5x5 convolution with the weights masked to the (row+col) odd taps (mask is a buffer)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.register_buffer("mask", torch.zeros_like(self.weight.data))
        self.mask[:, :, 0::2, 1::2] = 1
        self.mask[:, :, 1::2, 0::2] = 1


class MaskedConv2d(nn.Conv2d):
    """compressai.layers.MaskedConv2d: parameter/buffer holder only (dead member of the parent class)."""

    def __init__(self, *args, mask_type="A", **kwargs):
        super().__init__(*args, **kwargs)
        self.register_buffer("mask", torch.ones_like(self.weight.data))
        _, _, h, w = self.mask.size()
        self.mask[:, :, h // 2, w // 2 + (mask_type == "B"):] = 0
        self.mask[:, :, h // 2 + 1:] = 0


class _Seq(_Prepared):
    """Owner of the packed-weight caches of its nn.Sequential members."""

    def __init__(self):
        super().__init__()
        self._caches = {}

    def _load_from_state_dict(self, *args, **kwargs):
        self._caches = {}
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *a, **k):
        self._caches = {}
        return super()._apply(fn, *a, **k)

    def seq(self, name, x, **kw):
        return run_sequential(getattr(self, name), x, self._caches.setdefault(name, {}), **kw)

    def seq_cat(self, name, parts, **kw):
        """``getattr(self, name)(torch.cat(parts, 1))`` without the cat: the first layer (a Conv2d not followed
        by an activation in every use of the reference) runs once per part on its slice of the weights."""
        mods = list(getattr(self, name))
        first = mods[0]
        cache = self._caches.setdefault(name + ":split", {})
        key = tuple(p.c for p in parts)
        if key not in cache:
            if sum(key) != first.in_channels:
                raise hip.VcError(f"{name}: concat of {key} channels does not match the layer ({first.in_channels})")
            packs, c0 = [], 0
            for i, c in enumerate(key):
                packs.append(hip.PackedConv(first.weight[:, c0:c0 + c], first.bias if i == 0 else None,
                                            stride=first.stride[0], device=first.weight.device))
                c0 += c
            cache[key] = packs
        # (fp16 path: when a bottleneck chain follows, the LAST partial sum is the chain's input and leaves as half)
        half_tail = len(mods) > 1 and hasattr(mods[1], "half_stream_ok") and mods[1].half_stream_ok()
        acc = None
        for i, (pk, part) in enumerate(zip(cache[key], parts)):
            acc = pk(part, res=acc, out_f16=bool(half_tail and i == len(parts) - 1))
        return run_sequential(nn.Sequential(*mods[1:]), acc, self._caches.setdefault(name + ":tail", {}), **kw)


# ------------------------------------------------------------------------------------------------
# helpers.py
# ------------------------------------------------------------------------------------------------
class DeformConv2d(_Prepared):
    """Parameter holder with torchvision's names; executed by vc_offset_diversity / vc_deform_conv2d."""

    def __init__(self, in_channels, out_channels, kernel_size=3, padding=1, groups=1):
        super().__init__()
        if kernel_size != 3 or padding != 1:
            raise hip.VcError("only DeformConv2d(kernel_size=3, padding=1) is on the path")
        self.groups = groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, 3, 3))
        self.bias = nn.Parameter(torch.empty(out_channels))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        nn.init.uniform_(self.bias, -0.1, 0.1)

    def packed(self):
        if self._packed is None:
            self._packed = hip.PackedDeform(self.weight, self.bias, self.groups, self.weight.device)
        return self._packed


class OffsetDiversity(nn.Module):
    def __init__(self, in_channel, magnitude):
        super().__init__()
        self.in_channel, self.magnitude = in_channel, magnitude
        self.fusion = DeformConv2d(in_channel * 2, in_channel, kernel_size=3, padding=1, groups=2 * 8)

    def run(self, x1, offset1, flow1, x2, offset2, flow2, out=None):
        """helpers.py:43-58 in one launch (offset preparation fused into the gather)."""
        return self.fusion.packed().offset_diversity(x1, offset1, flow1, x2, offset2, flow2, self.magnitude, out=out)


class MS_Feature(_Seq):
    def __init__(self, chans=(64, 96, 128)):
        """``chans``: widths of the three pyramid levels (ICIP2023's DeformB: 32 / 64 / 96)"""
        super().__init__()
        c1, c2, c3 = chans
        self.layer1 = nn.Sequential(conv(3, c1, kernel_size=3, stride=2), *_rbb(c1))
        self.layer2 = nn.Sequential(conv(c1, c2, kernel_size=3, stride=2), *_rbb(c2))
        self.layer3 = nn.Sequential(conv(c2, c3, kernel_size=3, stride=2), *_rbb(c3))

    def run(self, x, outs=(None, None, None)):
        l1 = self.seq("layer1", x, out=outs[0])
        l2 = self.seq("layer2", l1, out=outs[1])
        return l1, l2, self.seq("layer3", l2, out=outs[2])


class FlowNET(_Seq):
    def __init__(self):
        super().__init__()
        self.down0 = nn.Sequential(conv(6, 32, kernel_size=3, stride=2), *_rbb(32, 2))
        self.down1 = nn.Sequential(conv(32, 64, kernel_size=3, stride=2), *_rbb(64, 2))
        self.down2 = nn.Sequential(conv(64, 128, kernel_size=3, stride=2), *_rbb(128, 2))
        self.down3 = nn.Sequential(conv(128, 192, kernel_size=3, stride=2), *_rbb(192, 2))
        self.up0 = nn.Sequential(*_rbb(192, 2), subpel_conv3x3(192, 128, 2))
        self.up1 = nn.Sequential(conv(256, 128, 1, 1), *_rbb(128, 2), subpel_conv3x3(128, 64, 2))
        self.up2 = nn.Sequential(conv(128, 64, 1, 1), *_rbb(64, 2), subpel_conv3x3(64, 32, 2))
        self.up3 = nn.Sequential(conv(64, 32, 1, 1), *_rbb(32, 2), subpel_conv3x3(32, 4, 2))

    def run(self, inp):
        """helpers.py:163-172; every skip tensor is written next to the slot the up-path fills (no cat)."""
        dev, n = inp.buf.device, inp.n
        if inp.h % 16 or inp.w % 16:
            raise hip.VcError("FlowNET input must be a multiple of 16 (FlowGuidedB.pad_flow)")
        cat3 = T.empty(n, inp.h // 2, inp.w // 2, 64, dev)       # [up2 out | s0]
        cat2 = T.empty(n, inp.h // 4, inp.w // 4, 128, dev)      # [up1 out | s1]
        cat1 = T.empty(n, inp.h // 8, inp.w // 8, 256, dev)      # [up0 out | s2]
        s0 = self.seq("down0", inp, out=cat3.channels(32, 64))
        s1 = self.seq("down1", s0, out=cat2.channels(64, 128))
        s2 = self.seq("down2", s1, out=cat1.channels(128, 256))
        s3 = self.seq("down3", s2)
        self.seq("up0", s3, out=cat1.channels(0, 128))
        self.seq("up1", cat1, out=cat2.channels(0, 64))
        self.seq("up2", cat2, out=cat3.channels(0, 32))
        return self.seq("up3", cat3)


class _TemporalEnc(_Seq):
    def __init__(self, mult, N=128, M=128, chans=(64, 96, 128)):
        super().__init__()
        c1, c2, c3 = chans
        self.g_a1 = nn.Sequential(conv(c1 * mult, N, kernel_size=5, stride=2), *_rbb(N))
        self.g_a2 = nn.Sequential(conv(N + c2 * mult, N, kernel_size=5, stride=2), *_rbb(N))
        self.g_a3 = nn.Sequential(conv(N + c3 * mult, M, kernel_size=5, stride=2), *_rbb(M))

    def run(self, l1, l2, l3, out=None):
        y = self.seq("g_a1", l1)
        y = self.seq_cat("g_a2", [y, l2])
        return self.seq_cat("g_a3", [y, l3], out=out)


class OffsetTemproalEnc(_TemporalEnc):
    def __init__(self, N=128, M=128):
        super().__init__(4, N, M)


class ResidualTemproalEnc(_TemporalEnc):
    def __init__(self, N=128, M=128):
        super().__init__(1, N, M)


class Reconstuctor(_Seq):
    def __init__(self, widths=(64, 96, 128), up=None):
        """``widths``: channels of x_comp_l1 / l2 / l3; ``up(cin, cout)``: the x2 upsampling layer that ends a level (default: the
        sub-pixel convolution of ICIP2024; ICIP2023 ends its levels with a 3x3 transposed convolution)."""
        super().__init__()
        w1, w2, w3 = widths
        up = up or (lambda cin, cout: subpel_conv3x3(cin, cout, 2))
        self.layer3 = nn.Sequential(*_rbb(w3), up(w3, w3))
        self.layer2 = nn.Sequential(conv(w3 + w2, w2, 1, 1), *_rbb(w2), up(w2, w2))
        self.layer1 = nn.Sequential(conv(w2 + w1, w1, 1, 1), *_rbb(w1), up(w1, 3))

    def run(self, x_comp_l1, x_comp_l2, x_comp_l3):
        l3 = self.seq("layer3", x_comp_l3)
        l2 = self.seq_cat("layer2", [x_comp_l2, l3])
        return self.seq_cat("layer1", [x_comp_l1, l2])


# ------------------------------------------------------------------------------------------------
# compression_bottlenecks.py
# ------------------------------------------------------------------------------------------------
GROUPS = (0, 6, 12, 24, 48)
CODERS = ("host", "device")


def _check_coder(coder, waves):
    if coder not in CODERS or not hip.irans_waves_ok(waves):
        raise hip.VcError(f"coder {coder!r} / waves {waves!r}: one of {CODERS}, waves a power of two in 1..16")


# ---- the three pass readers of the checkerboard decoder (JointAutoregressiveHierarchicalPriors._decode_passes) ----------------
# reader(group, parity, scales, means, out): fills the pass's parity of ``out`` (the group's channel window of y_hat) with
# symbol + mean, the symbols taken from where the reader's coder left them, in the squeezed order vc_gc_forward_ckbd wrote.
class HostStreamReader:
    """Host-coded strings: vc_gc_indexes_ckbd -> indexes to the host -> RansStreamDecoder.decode_stream -> symbols back ->
    vc_gc_dequant_ckbd; one decoder per group string, continued from the anchor pass to the non-anchor pass.  ``groups``: per
    group the list of its strings -- one per image (``per_image``) or one for the whole call."""

    def __init__(self, model, groups, per_image):
        self.table, self.tables = model._scale_table_dev(), model.gaussian_conditional.tables()
        self.groups, self.per_image = groups, per_image
        self.decoders, self.keep = None, []

    def __call__(self, group, parity, scales, means, out):
        if parity == 1:
            self.decoders = [hip.RansStreamDecoder(b) for b in self.groups[group]]
        idx = torch.empty((out.n, out.c * out.h * (out.w // 2)), dtype=torch.int32, device=out.buf.device)
        hip.check(hip.lib().vc_gc_indexes_ckbd(hip.stream(), scales.view(), parity, self.table.data_ptr(), self.table.numel(),
                                               idx.data_ptr()), "vc_gc_indexes_ckbd")
        rows = idx.cpu().numpy().reshape(out.n if self.per_image else 1, -1)
        sym = torch.from_numpy(np.stack([d.decode_stream(r, *self.tables) for d, r in zip(self.decoders, rows)])).to(idx.device)
        self.keep.append(sym)                                          # (must outlive the launch that reads it)
        hip.check(hip.lib().vc_gc_dequant_ckbd(hip.stream(), sym.data_ptr(), means.view(), None, parity, out.view()), "vc_gc_dequant_ckbd")


class DeviceChainReader:
    """Uploaded payloads (hip.IransDecoder), three launches per pass: vc_gc_indexes_ckbd -> vc_irans_decode -> vc_gc_dequant_ckbd.
    Nothing crosses to the host.  The B-frame decoders' reader (the fused launch measured slower there)."""

    def __init__(self, model, dec):
        self.table, self.tables, self.dec = model._scale_table_dev(), model.gaussian_conditional.irans_tables(), dec

    def __call__(self, group, parity, scales, means, out):
        idx = torch.empty((out.n, out.c * out.h * (out.w // 2)), dtype=torch.int32, device=out.buf.device)
        hip.check(hip.lib().vc_gc_indexes_ckbd(hip.stream(), scales.view(), parity, self.table.data_ptr(), self.table.numel(),
                                               idx.data_ptr()), "vc_gc_indexes_ckbd")
        sym = self.dec.decode(idx, self.tables)                        # (torch's allocator keeps the block until the stream is past it)
        hip.check(hip.lib().vc_gc_dequant_ckbd(hip.stream(), sym.data_ptr(), means.view(), None, parity, out.view()), "vc_gc_dequant_ckbd")


class DeviceFusedReader:
    """Uploaded payloads, one launch per pass: vc_irans_decode_gc_ckbd.  The intra codec's reader."""

    def __init__(self, model, dec):
        self.table, self.tables, self.dec = model._scale_table_dev(), model.gaussian_conditional.irans_tables(), dec

    def __call__(self, group, parity, scales, means, out):
        self.dec.decode_gc_ckbd(self.tables, scales, means, parity, self.table, None, out)


class JointAutoregressiveHierarchicalPriors(_Seq):
    """Members (and therefore state_dict keys) of compressai.models.JointAutoregressiveHierarchicalPriors(N, M);
    the ICIP2024 subclasses replace h_a / h_s / entropy_parameters and never run g_a / g_s / context_prediction.

    It also holds the ONE walk of the five-group, two-parity checkerboard entropy model both subclasses code with (_Elic: the
    B-frame compressors, ELIC: the intra codec), parametrised by ``GROUPS`` (the lower channel bounds of the groups):
    :meth:`_rate_passes` (the rate estimate), :meth:`_passes` (the ten entropy-parameter passes of the bitstream path),
    :meth:`_encode_passes` and :meth:`_decode_passes` (what fills y_hat pass by pass: vc_gc_forward_ckbd / one of the three
    readers above).  How the hyper slice gets into the networks' input buffers (pin0, pin) stays with the subclass."""
    GROUPS = None                      # set by the subclasses
    STRINGS_PER_IMAGE = True           # host-coded group strings: one per image, or one for the whole call (ELIC, as the reference)

    def __init__(self, N=192, M=192):
        super().__init__()
        self.entropy_bottleneck = EntropyBottleneck(N)
        self.g_a = nn.Sequential(conv(3, N), GDN(N), conv(N, N), GDN(N), conv(N, N), GDN(N), conv(N, M))
        self.g_s = nn.Sequential(deconv(M, N), GDN(N, inverse=True), deconv(N, N), GDN(N, inverse=True),
                                 deconv(N, N), GDN(N, inverse=True), deconv(N, 3))
        self.h_a = nn.Sequential()
        self.h_s = nn.Sequential()
        self.entropy_parameters = nn.Sequential()
        self.context_prediction = MaskedConv2d(M, 2 * M, kernel_size=5, padding=2, stride=1)
        self.gaussian_conditional = GaussianConditional(None)
        self.N, self.M = int(N), int(M)

    def update(self, scale_table=None, force=False):
        """compressai JointAutoregressiveHierarchicalPriors.update: range-coder tables of both entropy models."""
        from .layers import get_scale_table
        updated = self.gaussian_conditional.update_scale_table(get_scale_table() if scale_table is None else scale_table, force=force)
        updated |= self.entropy_bottleneck.update(force=force)
        return updated

    def _bounds(self):
        return self.GROUPS + (self.M,)

    def _sub(self, name, i, x, **kw):
        return run_sequential(getattr(self, name)[i], x, self._caches.setdefault(f"{name}.{i}", {}), **kw)

    def _ctx_conv(self, i):
        key = f"ctx.{i}"
        if key not in self._caches:
            self._caches[key] = pack_conv(self.context_prediction_models[i])
        return self._caches[key]

    def _rate_passes(self, y, pin0, pin, bits, y_hat=None):
        """The rate estimate of the five groups on (pin0, pin) that already hold the hyper slice: appends 5 x n rows to ``bits``
        (y_0 .. y_4 of every image) and returns round(y).  The channel context reads round(y) of the groups in front -- or, with
        ``y_hat`` (forward_stage2; receives round(y - mu) + mu group by group), round(y_hat) of them."""
        L, M = hip.lib(), self.M
        y_round = hip.quantize_mask(y)                                 # ste_round(y)
        y_half = hip.quantize_mask(y, keep_parity=1)                   # anchors only (non-anchors zeroed)
        bounds = self._bounds()
        for i in range(5):
            c0, c1 = bounds[i], bounds[i + 1]
            p = pin0 if i == 0 else pin
            ctx = self._ctx_conv(i)(y_half.channels(c0, c1), out=p.channels(0, 2 * M))
            hip.quantize_mask(ctx, out=ctx, keep_parity=0, do_round=False)
            if i > 0:
                prev = y_round.channels(0, c0) if y_hat is None else hip.quantize_mask(y_hat.channels(0, c0))
                self._sub("channel_context_models", i - 1, prev, out=p.channels(2 * M, 4 * M))
            gp = self._sub("entropy_parameters", i, p)
            half = c1 - c0
            for j in range(y.n):
                hip.check(L.vc_gc_forward(hip.stream(), y.channels(c0, c1).images(j, j + 1).view(),
                                          gp.channels(0, half).images(j, j + 1).view(),
                                          gp.channels(half, 2 * half).images(j, j + 1).view(), None, None,
                                          hip.NULL_VIEW if y_hat is None else y_hat.channels(c0, c1).images(j, j + 1).view(),
                                          bits.next_row_ptr(), bits.slots, None, None, None, None, 0, None), "vc_gc_forward")
        return y_round

    # ---- the walk of the bitstream paths ---------------------------------------------------------------------------------------
    # One string / segment for the hyper-latents, then per channel group the anchor symbols (checkerboard positions with (row + col)
    # odd, coded with the checkerboard-context slice at zero) followed by the non-anchor symbols (coded with the checkerboard
    # context of the just-decoded anchors).  The integers exist in the format's squeezed order only ([n][c][h][w/2], what the
    # *_ckbd kernels write and read: csrc/entropy.hip): the two passes of a group fill ONE zero-initialised y_hat, no parity mask,
    # merge or re-ordering in between.  Encoder and decoder walk the one generator: the same launches on the same layouts.
    def _scale_table_dev(self):
        gc = self.gaussian_conditional
        if gc._packed is None:
            if gc.scale_table.numel() == 0:
                raise hip.VcError("scale table is empty: call update(force=True) after loading weights")
            gc._packed = gc.scale_table.detach().float().contiguous().to(gc.scale_bound.device)
        return gc._packed

    def _z_index_dev(self, n, hw, dev):
        """table index of every hyper-latent symbol, [n, N * hw] on the device: the channel (no synchronisation)"""
        return torch.arange(self.N, dtype=torch.int32, device=dev).view(1, self.N, 1).expand(n, self.N, hw).reshape(n, -1).contiguous()

    def _trace_latents(self, trace, y_hat, z_hat):
        bounds = self._bounds()
        trace["y_hat"] = [hip.nhwc_to_nchw(y_hat.channels(bounds[i], bounds[i + 1])) for i in range(5)]
        trace["z_hat"] = hip.nhwc_to_nchw(z_hat)

    def _encode_z(self, y, z, bits, out_gain=None):
        """(z_hat, symbols int32 [n, N * hz * wz]) of the hyper-latents z of the latents y; one row of ``bits``"""
        if (y.h, y.w) != (4 * z.h, 4 * z.w) or y.w % 2:
            raise hip.VcError(f"latent {y.h}x{y.w} / hyper-latent {z.h}x{z.w}: the frame must be a multiple of 64")
        z_hat = T.empty(z.n, z.h, z.w, z.c, z.buf.device)
        z_sym = torch.empty((z.n, z.c * z.h * z.w), dtype=torch.int32, device=z.buf.device)
        hip.check(hip.lib().vc_eb_forward(hip.stream(), z.view(), self.entropy_bottleneck.device_params().data_ptr(), None,
                                          None if out_gain is None else out_gain.data_ptr(), z_hat.view(), z_sym.data_ptr(),
                                          bits.next_row_ptr(), bits.slots, None), "vc_eb_forward")
        return z_hat, z_sym

    def _passes(self, pin0, pin, y_hat):
        """The ten entropy-parameter passes of a frame, in coding order: yields (group, c0, c1, parity, scales, means) with the two
        Gaussian-parameter views of the pass.  (pin0, pin) = [ctx | hyper] of group 0 and [ctx | channel ctx | hyper] of the others,
        the hyper slices filled.  The caller fills ``y_hat`` (zero-initialised) at the pass's parity of channels c0:c1 before it
        asks for the next pass: the non-anchor pass and the later groups read it."""
        M = self.M
        bounds = self._bounds()
        for i in range(5):
            c0, c1 = bounds[i], bounds[i + 1]
            cg = c1 - c0
            p = pin0 if i == 0 else pin
            hip.axpby(p.channels(p.c - 2 * M, p.c), None, alpha=0.0, out=p.channels(0, 2 * M))   # anchor pass: ctx = 0 (hyper is finite)
            if i > 0:
                self._sub("channel_context_models", i - 1, y_hat.channels(0, c0), out=p.channels(2 * M, 4 * M))
            for parity in (1, 0):
                if parity == 0:                    # the group's anchors are in y_hat, its non-anchors still zero
                    self._ctx_conv(i)(y_hat.channels(c0, c1), out=p.channels(0, 2 * M))
                gp = self._sub("entropy_parameters", i, p)
                yield i, c0, c1, parity, gp.channels(0, cg), gp.channels(cg, 2 * cg)

    def _zero_latents(self, pin):
        n, h, w, M = pin.n, pin.h, pin.w, self.M
        return T(torch.zeros(n * h * w * M, dtype=torch.float32, device=pin.buf.device), n, h, w, M, h * w * M, w * M, M)

    def _encode_passes(self, y, pin0, pin, bits, passes=None):
        """Encoder body: (y_hat, coded) with ``coded`` the segment table of the ten passes, (symbols, indexes) int32 device tensors
        [n, count] in squeezed order; one row of ``bits`` per pass.  ``passes`` (a list): receives per pass a dict group / c0 / c1 /
        parity / y / scales / means of views."""
        table = self._scale_table_dev()
        y_hat, coded = self._zero_latents(pin), []
        for i, c0, c1, parity, scales, means in self._passes(pin0, pin, y_hat):
            sym = torch.empty((y.n, (c1 - c0) * y.h * (y.w // 2)), dtype=torch.int32, device=y.buf.device)
            idx = torch.empty_like(sym)
            hip.check(hip.lib().vc_gc_forward_ckbd(hip.stream(), y.channels(c0, c1).view(), scales.view(), means.view(), None, None,
                                                   y_hat.channels(c0, c1).view(), parity, bits.next_row_ptr(), bits.slots,
                                                   sym.data_ptr(), idx.data_ptr(), table.data_ptr(), table.numel()), "vc_gc_forward_ckbd")
            coded.append((sym, idx))
            if passes is not None:
                passes.append({"group": i, "c0": c0, "c1": c1, "parity": parity, "y": y.channels(c0, c1), "scales": scales, "means": means})
        return y_hat, coded

    def _decode_passes(self, pin0, pin, reader):
        """Decoder body: y_hat, every pass filled by ``reader`` (one of the three pass readers)"""
        y_hat = self._zero_latents(pin)
        for i, c0, c1, parity, scales, means in self._passes(pin0, pin, y_hat):
            reader(i, parity, scales, means, y_hat.channels(c0, c1))
        return y_hat

    def _code_strings(self, z_sym, coded, coder, waves, trace):
        """The strings of a call from its segment table (z, then the ten passes of :meth:`_encode_passes`); ``trace`` receives the
        table as "coded", (symbols, indexes) per segment.
        ``coder="device"``: one payload of the interleaved coder per image -- the hyper-latent segment (table set 0, index =
        channel), then the ten passes (table set 1) -- from one launch of vc_irans_encode on the integers where they lie;
        collecting the payloads is the one synchronisation.
        ``coder="host"``: [[g0 strings], ..., [g4 strings]], [z string per image]] of the sequential coder; a group string holds the
        anchor integers, then the non-anchor integers -- of one image each (``STRINGS_PER_IMAGE``) or of all images of the call.
        The only device -> host traffic of the encoder: squeezed int32 tensors (one synchronisation, after the last launch)."""
        device = coder == "device"
        if device or trace is not None:
            table = [(z_sym, self._z_index_dev(z_sym.shape[0], z_sym.shape[1] // self.N, z_sym.device))] + coded
            if trace is not None:
                trace["coded"] = table
        if device:
            return hip.irans_encode([(sym, idx, int(k > 0)) for k, (sym, idx) in enumerate(table)],
                                    [self.entropy_bottleneck.irans_tables(), self.gaussian_conditional.irans_tables()], waves)
        gc_tables = self.gaussian_conditional.tables()
        z_index = np.repeat(np.arange(self.N, dtype=np.int32), z_sym.shape[1] // self.N)
        z_strings = [hip.rans_encode(row, z_index, *self.entropy_bottleneck.tables()) for row in z_sym.cpu().numpy()]
        rows = z_sym.shape[0] if self.STRINGS_PER_IMAGE else 1
        strings = []
        for g in range(5):
            host = [(sym.cpu().numpy().reshape(rows, -1), idx.cpu().numpy().reshape(rows, -1)) for sym, idx in coded[2 * g:2 * g + 2]]
            strings.append([hip.rans_encode(np.concatenate([sy[j] for sy, _ in host]), np.concatenate([ix[j] for _, ix in host]),
                                            *gc_tables) for j in range(rows)])
        return [strings, z_strings]


class _Elic(JointAutoregressiveHierarchicalPriors):
    """Body shared by Offset_ELIC (enc_mult 5, dec_mult 4, three 432-channel offset heads) and Res_ELIC
    (enc_mult 2, dec_mult 1, residual heads of 64/96/128 channels)."""
    GROUPS = GROUPS

    def __init__(self, enc_mult, dec_mult, outs, N=128, M=128, chans=(64, 96, 128), stem=False):
        """``chans``: widths of the three feature levels the multipliers count in.  ``stem`` (ICIP2023's Res_ELIC): a g_a0 stage
        takes the frame itself (the first member of ``enc1``) to N channels at half resolution in front of g_a1, which then reads
        [g_a0 output | rest of enc1]."""
        super().__init__(N, M)
        c1, c2, c3 = chans
        self.stem = bool(stem)
        if stem:
            self.g_a0 = nn.Sequential(conv(3, N, kernel_size=5, stride=2), *_rbb(N))
        self.g_a1 = nn.Sequential(conv((N if stem else 0) + c1 * enc_mult, N, kernel_size=5, stride=2), *_rbb(N))
        self.g_a2 = nn.Sequential(conv(N + c2 * enc_mult, N, kernel_size=5, stride=2), *_rbb(N))
        self.g_a3 = nn.Sequential(conv(N + c3 * enc_mult, M, kernel_size=5, stride=2), *_rbb(M))
        self.g_s3 = nn.Sequential(*_rbb(M), deconv(M, N, kernel_size=5, stride=2))
        self.g_o3 = nn.Sequential(conv(N + c3 * dec_mult, N, kernel_size=3, stride=1), *_rbb(N),
                                  conv(N, outs[2], kernel_size=3, stride=1))
        self.g_s2 = nn.Sequential(conv(N + c3 * dec_mult, N, kernel_size=1, stride=1), *_rbb(N),
                                  deconv(N, N, kernel_size=5, stride=2))
        self.g_o2 = nn.Sequential(conv(N + c2 * dec_mult, N, kernel_size=3, stride=1), *_rbb(N),
                                  conv(N, outs[1], kernel_size=3, stride=1))
        self.g_s1 = nn.Sequential(conv(N + c2 * dec_mult, N, kernel_size=1, stride=1), *_rbb(N),
                                  deconv(N, N, kernel_size=5, stride=2))
        self.g_o1 = nn.Sequential(conv(N + c1 * dec_mult, N, kernel_size=3, stride=1), *_rbb(N),
                                  conv(N, outs[0], kernel_size=3, stride=1))
        self.h_a = nn.Sequential(conv(M, N, stride=1, kernel_size=3), nn.ReLU(inplace=True),
                                 conv(N, N, stride=2, kernel_size=5), nn.ReLU(inplace=True),
                                 conv(N, N, stride=2, kernel_size=5))
        self.h_s = nn.Sequential(deconv(N, M, stride=2, kernel_size=5), nn.ReLU(inplace=True),
                                 deconv(M, M, stride=2, kernel_size=5), nn.ReLU(inplace=True),
                                 conv(M, M, stride=1, kernel_size=3))
        self.prior_fusion = nn.Sequential(conv(2 * M, 2 * M, stride=1, kernel_size=3), *_rbb(2 * M),
                                          conv(M * 2, M * 2, stride=1, kernel_size=3))
        self.entropy_parameters = nn.ModuleList(
            nn.Sequential(nn.Conv2d(cin, M * 10 // 3, 1), nn.LeakyReLU(inplace=True),
                          nn.Conv2d(M * 10 // 3, M * 8 // 3, 1), nn.LeakyReLU(inplace=True),
                          nn.Conv2d(M * 8 // 3, cout * 6 // 3, 1))
            for cin, cout in [(M * 4, 6), (M * 6, 6), (M * 6, 12), (M * 6, 24), (M * 6, M - 48)])
        self.channel_context_models = nn.ModuleList(
            nn.Sequential(conv(cin, N, kernel_size=5, stride=1), nn.ReLU(inplace=True),
                          conv(N, N, kernel_size=5, stride=1), nn.ReLU(inplace=True),
                          conv(N, M * 2, kernel_size=5, stride=1)) for cin in [6, 12, 24, 48])
        self.context_prediction_models = nn.ModuleList(
            CheckerboardContext(in_channels=cin, out_channels=M * 2, kernel_size=5, stride=1, padding=2)
            for cin in [6, 6, 12, 24, M - 48])
        self.levels = 5
        self.Gain = nn.Parameter(torch.ones(self.levels, M))
        self.InverseGain = nn.Parameter(torch.ones(self.levels, M))
        self.HyperGain = nn.Parameter(torch.ones(self.levels, N))
        self.InverseHyperGain = nn.Parameter(torch.ones(self.levels, N))
        self._gain_cache = {}

    def _load_from_state_dict(self, *args, **kwargs):
        self._gain_cache = {}
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *a, **k):
        self._gain_cache = {}
        return super()._apply(fn, *a, **k)

    def interpolate_gain(self, s):
        """compression_bottlenecks.py:296-318, evaluated on the host once per quality level (cached), fp32 like
        the reference; returns device vectors (gain, hypergain, invhypergain, invgain)."""
        s = max(min(s, self.levels - 1), 0)
        if s not in self._gain_cache:
            upper = int(min(math.ceil(s), self.levels - 1))
            lower = int(max(math.floor(s), 0))
            out = []
            with torch.no_grad():
                for m in (self.Gain, self.HyperGain, self.InverseHyperGain, self.InverseGain):
                    m = m.detach().to("cpu", torch.float32)
                    if upper == lower:
                        v = torch.abs(m[int(s)])
                    else:
                        l = upper - s
                        v = torch.abs(m[upper]) ** (1 - l) * torch.abs(m[lower]) ** l
                    out.append(v.contiguous().to(self.Gain.device))
            self._gain_cache[s] = tuple(out)
        return self._gain_cache[s]

    def _analysis(self, enc1, enc2, enc3):
        """g_a1 .. g_a3 (behind g_a0 where the codec has one) on the lists of views whose concatenation the reference feeds them"""
        if self.stem:
            enc1 = [self.seq("g_a0", enc1[0])] + list(enc1[1:])
        y = self.seq_cat("g_a1", enc1) if len(enc1) > 1 else self.seq("g_a1", enc1[0])
        y = self.seq_cat("g_a2", [y] + list(enc2))
        return self.seq_cat("g_a3", [y] + list(enc3))

    def code(self, enc1, enc2, enc3, f1d, f2d, f3d, temporal_into, s, bits, res=(None, None, None), trace=None, force=None):
        """Encoder, entropy model and the three decoder heads.

        enc1/enc2/enc3: lists of views whose concatenation the reference feeds to g_a1 / (after y) g_a2 / g_a3;
        f*d: decoder-side conditioning views; temporal_into(view): callback that makes the temporal conditioner
        write its output into the given slice of the prior-fusion input; res: optional views added to the three
        heads' outputs (Res_ELIC: x_comp + res fused into the last convolution).  Returns (head1, head2, head3).
        ``trace``: a dict that receives the gained latents "y" / "z" (what the quantiser rounds) and "heads".
        ``force``: a callable ``force(name, view)`` that sees the gained latents "y" and "z" before anything rounds them and may
        move them in place -- teacher forcing for stage-wise parity checks on checkpoints whose latents sit next to rounding boundaries.
        Appends 6 x n rows to ``bits`` (n = batch size): z of every image, then y_0 .. y_4 of every image."""
        L = hip.lib()
        gain, hypergain, invhypergain, invgain = self.interpolate_gain(s)
        y = self._analysis(enc1, enc2, enc3)
        y = hip.channel_scale(y, gain, out=y)
        z = self.seq("h_a", y, final_chscale=hypergain)
        if force is not None:
            force("y", y)
            force("z", z)
        for i in range(y.n):                                         # one counter row per image and tensor
            hip.check(L.vc_eb_forward(hip.stream(), z.images(i, i + 1).view(), self.entropy_bottleneck.device_params().data_ptr(),
                                      None, None, hip.NULL_VIEW, None, bits.next_row_ptr(), bits.slots, None), "vc_eb_forward")
        z_hat = hip.quantize_mask(z, gain=invhypergain)
        pin0, pin = self._hyper_buffers(z_hat, temporal_into)
        if trace is not None:
            trace.update({"y": y, "z": z})
        self._rate_passes(y, pin0, pin, bits)
        heads = self._synthesis_heads(hip.quantize_mask(y, gain=invgain), f1d, f2d, f3d, res)
        if trace is not None:
            trace["heads"] = heads
        return heads

    def _head(self, name, parts, res):
        t = self.seq_cat(name, parts)
        if res is None:
            return t
        return hip.axpby(t, res, out=t)

    # ---- real bitstream ------------------------------------------------------------------------------------------------------
    # The reference only estimates this model's rate; the format is this project's own and follows the intra
    # codec's conventions -- the walk of the base class -- with per image of the batch its own strings.  Coded values: z symbols =
    # round(z * hypergain - median), z_hat = (symbol + median) * invhypergain; y symbols = round(y * gain - mu), decoder-side latents
    # round(y - mu) + mu in the gained domain (what the channel and checkerboard contexts read), synthesis and heads read them times
    # invgain.
    def _hyper_buffers(self, z_hat, temporal_into):
        """hyper = prior_fusion([h_s(z_hat) | temporal condition]) in the inputs of the entropy-parameter networks: (pin0, pin) =
        [ctx | hyper] of group 0 and [ctx | channel ctx | hyper] of the others.  Rate estimate, encoder and decoder build them
        through this one function: the same launches on the same layouts."""
        M = self.M
        dev, n, h, w = z_hat.buf.device, z_hat.n, 4 * z_hat.h, 4 * z_hat.w
        fusion_in = T.empty(n, h, w, 2 * M, dev)                       # [h_s(z_hat) | temporal condition]
        self.seq("h_s", z_hat, out=fusion_in.channels(0, M))
        temporal_into(fusion_in.channels(M, 2 * M))
        pin = T.empty(n, h, w, 6 * M, dev)
        hyper = self.seq("prior_fusion", fusion_in, out=pin.channels(4 * M, 6 * M))
        pin0 = T.empty(n, h, w, 4 * M, dev)
        hip.axpby(hyper, None, out=pin0.channels(2 * M, 4 * M))
        return pin0, pin

    def _synthesis_heads(self, y_syn, f1d, f2d, f3d, res):
        """the three decoder heads from the latents the synthesis reads (inverse gain applied)"""
        xhat3 = self.seq("g_s3", y_syn)
        head3 = self._head("g_o3", [xhat3, f3d], res[2])
        xhat2 = self.seq_cat("g_s2", [xhat3, f3d])
        head2 = self._head("g_o2", [xhat2, f2d], res[1])
        xhat1 = self.seq_cat("g_s1", [xhat2, f2d])
        head1 = self._head("g_o1", [xhat1, f1d], res[0])
        return head1, head2, head3

    def compress_t(self, enc1, enc2, enc3, f1d, f2d, f3d, temporal_into, s, res=(None, None, None), trace=None, coder="host", waves=4):
        """Encoder of the bitstream path on channels-last views (arguments as :meth:`code`).  Returns ``{"strings": [[[g0 per
        image], ..., [g4 per image]], [z per image]], "shape": (hz, wz), "heads": the three decoder heads computed from the y_hat
        the decoder rebuilds (closed loop), "bits": 0-dim float64 device tensor, the -log2 p sum of exactly the coded symbols (the
        z row + two parity rows per group)}``.  ``trace``: receives "y_hat" (five NCHW tensors, gained domain), "z_hat" and
        "passes" (per pass a dict group / c0 / c1 / parity / y / scales / means of views) and "coded" (the segment table: (symbols,
        indexes) int32 device tensors [n, count] of z and of the ten passes in coding order).  ``coder="device"``: "strings" is
        one payload per image of the interleaved coder instead (:meth:`_code_strings`)."""
        gain, hypergain, invhypergain, invgain = self.interpolate_gain(s)
        y = self._analysis(enc1, enc2, enc3)
        y = hip.channel_scale(y, gain, out=y)
        z = self.seq("h_a", y, final_chscale=hypergain)
        bits = BitCounter(y.buf.device, max_rows=11)
        z_hat, z_sym = self._encode_z(y, z, bits, invhypergain)
        pin0, pin = self._hyper_buffers(z_hat, temporal_into)
        if trace is not None:
            trace["passes"] = []
        y_hat, coded = self._encode_passes(y, pin0, pin, bits, None if trace is None else trace["passes"])
        heads = self._synthesis_heads(hip.channel_scale(y_hat, invgain), f1d, f2d, f3d, res)
        total = bits.totals().sum()
        if trace is not None:
            self._trace_latents(trace, y_hat, z_hat)
            trace["heads"] = heads
        return {"strings": self._code_strings(z_sym, coded, coder, waves, trace), "shape": (z.h, z.w), "heads": heads, "bits": total}

    def decompress_t(self, strings, shape, f1d, f2d, f3d, temporal_into, s, res=(None, None, None), trace=None, reader=None):
        """Decoder of :meth:`compress_t`: decoder-side inputs only.  Returns the three heads.  ``strings``: the host-coded lists
        (HostStreamReader: two decode_stream calls per group string on one RansStreamDecoder per image) or the payloads of
        ``coder="device"``, already uploaded (hip.IransDecoder): nothing crosses to the host, the caller reads the decoder's error
        words once, after the reconstruction.  ``reader``: the pass reader of uploaded payloads, DeviceChainReader unless given."""
        dev = self.Gain.device
        _, _, invhypergain, invgain = self.interpolate_gain(s)
        hz, wz = int(shape[0]), int(shape[1])
        uploaded = isinstance(strings, hip.IransDecoder)
        if not uploaded and (len(strings) != 2 or len(strings[0]) != 5 or not strings[1] or any(len(g) != len(strings[1]) for g in strings[0])):
            raise hip.VcError("strings: [[g0, ..., g4], z] with one byte string per image in each of the six lists")
        if not (1 <= hz <= 4096 and 1 <= wz <= 4096):
            raise hip.VcError(f"hyper-latent shape {hz}x{wz} is outside 1..4096")
        if uploaded:
            n = strings.images
            z_sym = strings.decode(self._z_index_dev(n, hz * wz, dev), self.entropy_bottleneck.irans_tables())
            reader = (reader or DeviceChainReader)(self, strings)
        else:
            n = len(strings[1])
            z_index = np.repeat(np.arange(self.N, dtype=np.int32), hz * wz)
            z_sym = torch.from_numpy(np.stack([hip.rans_decode(b, z_index, *self.entropy_bottleneck.tables()) for b in strings[1]])).to(dev)
            reader = HostStreamReader(self, strings[0], self.STRINGS_PER_IMAGE)
        z_hat = T.empty(n, hz, wz, self.N, dev)
        hip.check(hip.lib().vc_eb_dequant(hip.stream(), z_sym.data_ptr(), self.entropy_bottleneck.device_params().data_ptr(),
                                          invhypergain.data_ptr(), z_hat.view()), "vc_eb_dequant")
        pin0, pin = self._hyper_buffers(z_hat, temporal_into)
        y_hat = self._decode_passes(pin0, pin, reader)
        heads = self._synthesis_heads(hip.channel_scale(y_hat, invgain), f1d, f2d, f3d, res)
        if trace is not None:
            self._trace_latents(trace, y_hat, z_hat)
            trace["heads"] = heads
        return heads


class Offset_ELIC(_Elic):
    def __init__(self, N=128, M=128, **kwargs):
        super().__init__(5, 4, (27 * 8 * 2,) * 3, N, M)


class Res_ELIC(_Elic):
    def __init__(self, N=128, M=128, **kwargs):
        super().__init__(2, 1, (64, 96, 128), N, M)


# ------------------------------------------------------------------------------------------------
# elic.py: the intra codec of the ICIP2024 test loop
# ------------------------------------------------------------------------------------------------
class _ResidualUnit(_Prepared):
    """compressai AttentionBlock.ResidualUnit: relu(conv1x1 -> ReLU -> conv3x3 -> ReLU -> conv1x1 + x)."""

    def __init__(self, N):
        super().__init__()
        self.conv = nn.Sequential(conv1x1(N, N // 2), nn.ReLU(inplace=True), conv3x3(N // 2, N // 2), nn.ReLU(inplace=True),
                                  conv1x1(N // 2, N))
        self.relu = nn.ReLU(inplace=True)

    def run(self, x):
        if self._packed is None:
            self._packed = (pack_conv(self.conv[0]), pack_conv(self.conv[2]), pack_conv(self.conv[4]))
        c1, c2, c3 = self._packed
        t = c1(x, act=hip.ACT_RELU, out_f16=c2.half_ok, out_sp3=hip.wants_split(c2, x))
        t = c2(t, act=hip.ACT_RELU, out_f16=c3.half_ok)
        return c3(t, act=hip.ACT_RELU, res=x, res_first=True)        # the ReLU comes AFTER the skip addition


class AttentionBlock(_Prepared):
    """compressai.layers.AttentionBlock: conv_a(x) * sigmoid(conv_b(x)) + x (elic.py:97-121 uses it four times)."""
    vc_block = True

    def __init__(self, N):
        super().__init__()
        self.conv_a = nn.Sequential(_ResidualUnit(N), _ResidualUnit(N), _ResidualUnit(N))
        self.conv_b = nn.Sequential(_ResidualUnit(N), _ResidualUnit(N), _ResidualUnit(N), conv1x1(N, N))

    def run(self, x, out=None):
        if self._packed is None:
            self._packed = pack_conv(self.conv_b[3])
        a = b = x
        for u in self.conv_a:
            a = u.run(a)
        for u in list(self.conv_b)[:3]:
            b = u.run(b)
        return hip.attention_gate(a, self._packed(b), x, out=out)


ELIC_GROUPS = (0, 16, 32, 64, 128)


class ELIC(JointAutoregressiveHierarchicalPriors):
    """elic.py:85-596: forward (rate estimate, what utils.image_compress calls for the I-frames), forward_stage2, and the
    two-pass checkerboard bitstream codec compress / decompress."""
    GROUPS = ELIC_GROUPS
    STRINGS_PER_IMAGE = False

    def __init__(self, N=192, M=320, **kwargs):
        super().__init__(N, M)
        self.g_a = nn.Sequential(conv(3, N), *_rbb(N), conv(N, N), *_rbb(N), AttentionBlock(N), conv(N, N), *_rbb(N),
                                 conv(N, M), AttentionBlock(M))
        self.g_s = nn.Sequential(AttentionBlock(M), deconv(M, N), *_rbb(N), deconv(N, N), AttentionBlock(N), *_rbb(N),
                                 deconv(N, N), *_rbb(N), deconv(N, 3))
        self.h_a = nn.Sequential(conv(M, N, stride=1, kernel_size=3), nn.ReLU(inplace=True), conv(N, N), nn.ReLU(inplace=True),
                                 conv(N, N))
        self.h_s = nn.Sequential(deconv(N, M), nn.ReLU(inplace=True), deconv(M, M * 3 // 2), nn.ReLU(inplace=True),
                                 conv(M * 3 // 2, M * 2, stride=1, kernel_size=3))
        self.entropy_parameters = nn.ModuleList(
            nn.Sequential(nn.Conv2d(cin, M * 10 // 3, 1), nn.LeakyReLU(inplace=True),
                          nn.Conv2d(M * 10 // 3, M * 8 // 3, 1), nn.LeakyReLU(inplace=True),
                          nn.Conv2d(M * 8 // 3, cout * 6 // 3, 1))
            for cin, cout in [(M * 4, 16), (M * 6, 16), (M * 6, 32), (M * 6, 64), (M * 6, M - 128)])
        self.channel_context_models = nn.ModuleList(
            nn.Sequential(conv(cin, N, kernel_size=5, stride=1), nn.ReLU(inplace=True),
                          conv(N, N, kernel_size=5, stride=1), nn.ReLU(inplace=True),
                          conv(N, M * 2, kernel_size=5, stride=1)) for cin in [16, 32, 64, 128])
        self.context_prediction_models = nn.ModuleList(
            CheckerboardContext(in_channels=cin, out_channels=M * 2, kernel_size=5, stride=1, padding=2)
            for cin in [16, 16, 32, 64, M - 128])

    def forward_device(self, x, bits, stage2=False):
        """x: T [n,H,W,3] (H, W multiples of 64) -> x_hat T; appends 6 x n rows to ``bits`` (z, y_0..y_4 per image).
        ``stage2`` = forward_stage2 (elic.py:247-305): the channel context sees round(round(y - mu) + mu) of the groups
        already processed and the synthesis their round(y - mu) + mu, instead of round(y)."""
        L, M = hip.lib(), self.M
        y = self.seq("g_a", x)
        z = self.seq("h_a", y)
        dev, n, h, w = y.buf.device, y.n, y.h, y.w
        for i in range(n):
            hip.check(L.vc_eb_forward(hip.stream(), z.images(i, i + 1).view(), self.entropy_bottleneck.device_params().data_ptr(),
                                      None, None, hip.NULL_VIEW, None, bits.next_row_ptr(), bits.slots, None), "vc_eb_forward")
        params_in = T.empty(n, h, w, 6 * M, dev)                       # [ctx | channel ctx | hyper]
        hyper = self.seq("h_s", hip.quantize_mask(z), out=params_in.channels(4 * M, 6 * M))
        params_in0 = T.empty(n, h, w, 4 * M, dev)                      # group 0: [ctx | hyper]
        hip.axpby(hyper, None, out=params_in0.channels(2 * M, 4 * M))
        y_hat = T.empty(n, h, w, M, dev) if stage2 else None            # round(y - mu) + mu, group by group
        y_round = self._rate_passes(y, params_in0, params_in, bits, y_hat)
        return self.seq("g_s", y_hat if stage2 else y_round)

    def forward_stage2(self, x):
        """elic.py:247-305 -- same return structure as forward."""
        _require_frames(x)
        bits = BitCounter(x.device, max_rows=6 * x.shape[0])
        x_hat = hip.nhwc_to_nchw(self.forward_device(hip.nchw_to_nhwc(x), bits, stage2=True))
        return {"x_hat": x_hat, "size": bits.totals().sum().float()}

    # ---- real bitstream (elic.py:307-496): the walk of the base class, no gains, no temporal condition ------------------------------
    # coder="host": the reference's strings -- one z string per image and ONE string per channel group for the whole call (the anchor
    # integers of all images, then the non-anchor integers).  coder="device" (DESIGN.md section 4g): one payload of the interleaved
    # coder per image; nothing crosses to the host before the payloads are collected / the error words are read.
    def _hyper_buffers(self, z_hat):
        """(pin0, pin) = [ctx | hyper] of group 0 and [ctx | channel ctx | hyper] of the others, hyper = h_s(z_hat) copied into both"""
        M = self.M
        hyper = self.seq("h_s", z_hat)
        n, h, w, dev = hyper.n, hyper.h, hyper.w, hyper.buf.device
        pin = T.empty(n, h, w, 6 * M, dev)
        hip.axpby(hyper, None, out=pin.channels(4 * M, 6 * M))
        pin0 = T.empty(n, h, w, 4 * M, dev)
        hip.axpby(hyper, None, out=pin0.channels(2 * M, 4 * M))
        return pin0, pin

    def _nchw_groups(self, y_hat):
        bounds = self._bounds()
        return [hip.nhwc_to_nchw(y_hat.channels(bounds[i], bounds[i + 1])) for i in range(5)]

    def compress(self, x, coder="host", waves=4, trace=None):
        """{"strings": [[[g0], [g1], [g2], [g3], [g4]], [z]], "shape", "y_hat": 5 NCHW tensors} like elic.py:307-414.

        ``coder="device"``: "strings" is one payload of the interleaved coder per image (hyper-latent segment, then the ten passes),
        coded by one vc_irans_encode launch on the integers where they lie; the result gains "x_hat" (the synthesis of the y_hat
        that was coded), "bits" (0-dim float64 device tensor: -log2 p of the coded symbols), "coder" and "waves".  ``trace``
        (device coder): receives "coded" (the segment table: (symbols, indexes) of z and of the ten passes), "y_hat", "z_hat",
        "x_hat".  ``waves`` and ``trace`` belong to the device coder: the host coder ignores the first and refuses the second."""
        _require_frames(x)
        device = coder != "host"
        if device:
            _check_coder(coder, waves)
        elif trace is not None:
            raise hip.VcError('ELIC.compress: trace= belongs to coder="device" (the host-coded path returns its latents in "y_hat")')
        y = self.seq("g_a", hip.nchw_to_nhwc(x.contiguous().float()))
        z = self.seq("h_a", y)
        bits = BitCounter(y.buf.device, max_rows=11)
        z_hat, z_sym = self._encode_z(y, z, bits)
        pin0, pin = self._hyper_buffers(z_hat)
        y_hat, coded = self._encode_passes(y, pin0, pin, bits)
        result = {"shape": torch.Size([z.h, z.w]), "y_hat": self._nchw_groups(y_hat)}
        if device:
            x_hat = hip.nhwc_to_nchw(self.seq("g_s", y_hat))
            result.update({"x_hat": x_hat, "bits": bits.totals().sum(), "coder": "device", "waves": int(waves)})
            if trace is not None:
                self._trace_latents(trace, y_hat, z_hat)
                trace["x_hat"] = x_hat
        result["strings"] = self._code_strings(z_sym, coded, coder, waves, trace)      # the one synchronisation, after the last launch
        return result

    def decompress(self, strings, shape, coder="host", waves=4, trace=None, reader=None):
        """{"x_hat", "cost_time", "y_hat"} like elic.py:416-496 (HostStreamReader: two decode_stream calls per group string).

        ``coder="device"`` reads the payloads of ``compress(coder="device")`` (or a hip.IransDecoder that already uploaded them):
        one upload, then launches only, {"x_hat", "y_hat"}; the decoder's error words are read once at the end (VcError) -- by
        the caller (``finish()``) when it handed in the uploaded decoder.  ``trace``: receives "y_hat", "z_hat", "x_hat".
        ``reader``: the pass reader of the payloads, DeviceFusedReader unless given."""
        import time
        dev = self.entropy_bottleneck.quantiles.device
        device = coder != "host"
        uploaded = isinstance(strings, hip.IransDecoder)
        if device:
            _check_coder(coder, waves)
            hz, wz = int(shape[0]), int(shape[1])
            if not (1 <= hz <= 4096 and 1 <= wz <= 4096):
                raise hip.VcError(f"hyper-latent shape {hz}x{wz} is outside 1..4096")
            if not uploaded and not (isinstance(strings, (list, tuple)) and strings and all(isinstance(b, (bytes, bytearray)) for b in strings)):
                raise hip.VcError('ELIC.decompress(coder="device"): strings is one payload (bytes) per image, as compress(coder="device") '
                                  "returns it -- this looks like the host-coded [[g0, ..., g4], z] lists")
            dec = strings if uploaded else hip.IransDecoder(strings, waves, dev)
            if dec.waves != int(waves):
                raise hip.VcError(f"the uploaded payloads were read with waves {dec.waves}, not {waves}")
            z_hat = T.empty(dec.images, hz, wz, self.N, dev)
            dec.decode_eb(self.entropy_bottleneck.irans_tables(), self.entropy_bottleneck.device_params(), None, z_hat)
            reader = (reader or DeviceFusedReader)(self, dec)
        else:
            if trace is not None:
                raise hip.VcError('ELIC.decompress: trace= belongs to coder="device" (the host-coded path returns its latents in "y_hat")')
            if uploaded or len(strings) != 2 or len(strings[0]) != 5 or \
                    not all(isinstance(g, (list, tuple)) for g in list(strings[0]) + [strings[1]]):
                raise hip.VcError('ELIC.decompress(coder="host"): strings is [[g0, ..., g4], z] with one byte string per image in each list '
                                  '-- pass coder="device" for the payloads of compress(coder="device")')
            t0 = time.process_time()
            hz, wz = int(shape[0]), int(shape[1])
            z_index = np.repeat(np.arange(self.N, dtype=np.int32), hz * wz)
            z_sym = torch.from_numpy(np.stack([hip.rans_decode(b, z_index, *self.entropy_bottleneck.tables()) for b in strings[1]])).to(dev)
            z_hat = T.empty(len(strings[1]), hz, wz, self.N, dev)     # (z_sym is bound to a local: it must outlive the launch that reads it)
            hip.check(hip.lib().vc_eb_dequant(hip.stream(), z_sym.data_ptr(), self.entropy_bottleneck.device_params().data_ptr(),
                                              None, z_hat.view()), "vc_eb_dequant")
            reader = HostStreamReader(self, strings[0], self.STRINGS_PER_IMAGE)
        y_hat = self._decode_passes(*self._hyper_buffers(z_hat), reader)
        x_hat = hip.nhwc_to_nchw(self.seq("g_s", y_hat))
        if not device:
            torch.cuda.synchronize()
            return {"x_hat": x_hat, "cost_time": time.process_time() - t0, "y_hat": self._nchw_groups(y_hat)}
        if trace is not None:
            self._trace_latents(trace, y_hat, z_hat)
            trace["x_hat"] = x_hat
        result = {"x_hat": x_hat, "y_hat": self._nchw_groups(y_hat)}
        if not uploaded:                           # the one read, after everything is enqueued
            dec.finish()
        return result

    def forward(self, x):
        """NCHW CUDA tensor in; ``{"x_hat", "size"}`` out (``size`` = the -log2 likelihood sum the reference's
        image_compress derives from the likelihood tensors, which are not materialised here)."""
        _require_frames(x)
        bits = BitCounter(x.device, max_rows=6 * x.shape[0])
        x_hat = hip.nhwc_to_nchw(self.forward_device(hip.nchw_to_nhwc(x), bits))
        return {"x_hat": x_hat, "size": bits.totals().sum().float()}


def image_compress(im, compressors, n):
    """utils.py:306-316: (reconstruction, estimated size in bits) of an intra-coded frame at quality index n."""
    out = compressors[n](im)
    return out["x_hat"], out["size"]


# ------------------------------------------------------------------------------------------------
# m.py
# ------------------------------------------------------------------------------------------------
def _f32_round2(v):
    """convert_scales (m.py:71-82): fp32 value rounded to two decimals, as a python float."""
    t = torch.tensor([v], dtype=torch.float32) if not torch.is_tensor(v) else v.reshape(-1)[:1].to("cpu", torch.float32)
    return float((torch.round(t * 10 ** 2) / (10 ** 2)).item())


def _flat_strings(codec_strings):
    """[[[g0], ..., [g4]], [z]] -> every byte string of it"""
    groups, z = codec_strings
    return [b for g in groups for b in g] + list(z)


class _BFrameBitstream(nn.Module):
    """The real-bitstream surface the two B-frame models share (FlowGuidedB here, DeformB in icip2023.py): both code an offset
    latent and a residual latent with two _Elic compressors, ``offset_compressor`` and ``residual_compressor``, an alignment step
    between them and ``reconstructor`` behind them.  Each model keeps its features, its alignment and its frame-level checks."""

    @staticmethod
    def _coding_level(s):
        """the quality level as the container stores it (fp32): both sides interpolate the gains from the same number"""
        return float(np.float32(s))

    def _coded_tail(self, F_, cond, off_temporal, align, res_lead, res_temporal, s, strings, shape, trace, coder, waves, reader):
        """offset codec -> ``align(offset heads)`` = the three aligned maps -> residual codec -> reconstructor, on the compressors'
        bitstream paths.  Encoder: ``F_`` the per-level buffers the offset encoder reads, ``res_lead`` per level the views the
        residual encoder reads in front of the aligned map; decoder: both None, ``strings`` / ``shape`` instead.  ``cond``: the three
        decoder-side views of the offset codec; ``*_temporal``: the two temporal conditioners.  Returns ``{"offset", "residual"}``
        (encoder: the results of compress_t) and "x_hat" (NCHW)."""
        enc = F_ is not None
        t_off, t_res = ({}, {}) if trace is not None else (None, None)
        oc, rc = self.offset_compressor, self.residual_compressor
        off_cond = lambda dst: off_temporal.run(*cond, out=dst)  # noqa: E731
        out = {}
        if enc:
            out["offset"] = oc.compress_t([F_[0]], [F_[1]], [F_[2]], *cond, off_cond, s, trace=t_off, coder=coder, waves=waves)
            offs = out["offset"]["heads"]
        else:
            offs = oc.decompress_t(strings["offset"], shape, *cond, off_cond, s, trace=t_off, reader=reader)
        comp = align(offs)
        res_cond = lambda dst: res_temporal.run(*comp, out=dst)  # noqa: E731
        if enc:
            out["residual"] = rc.compress_t(*[list(lead) + [c] for lead, c in zip(res_lead, comp)], *comp, res_cond, s, res=tuple(comp),
                                            trace=t_res, coder=coder, waves=waves)
            xs = out["residual"]["heads"]
        else:
            xs = rc.decompress_t(strings["residual"], shape, *comp, res_cond, s, res=tuple(comp), trace=t_res, reader=reader)
        if trace is not None:
            trace.update({"offset": t_off, "residual": t_res})
        out["x_hat"] = hip.nhwc_to_nchw(self.reconstructor.run(*xs))
        return out

    @staticmethod
    def _compress_result(out, coder, waves):
        """compress()'s result from the encoder's :meth:`_coded_tail`: "size" is the real bit count (8 x string bytes),
        "size_estimate" -log2 p of the coded symbols on the device; the device coder adds "coder" and "waves"."""
        strings = {k: out[k]["strings"] for k in ("offset", "residual")}
        device = coder == "device"
        nbytes = sum(len(b) for k in strings for b in (strings[k] if device else _flat_strings(strings[k])))
        result = {"strings": strings, "shape": out["offset"]["shape"], "x_hat": out["x_hat"], "size": 8 * nbytes,
                  "size_estimate": float((out["offset"]["bits"] + out["residual"]["bits"]).item())}
        if device:
            result.update({"coder": coder, "waves": int(waves)})
        return result

    def upload_payloads(self, strings, waves=4):
        """The payloads of ``compress(coder="device")`` on their way to the device (pinned, non-blocking) and their sub-stream
        headers read there: ``{"offset", "residual"}`` of hip.IransDecoder.  ``decompress`` takes the result in place of the
        strings; the caller then owns the one look at the error words, ``finish()`` of both, after it has used x_hat."""
        _check_coder("device", waves)
        if not isinstance(strings, dict) or set(strings) != {"offset", "residual"} or len(strings["offset"]) != len(strings["residual"]) \
                or not all(isinstance(b, (bytes, bytearray)) for k in strings for b in strings[k]) or not strings["offset"]:
            raise hip.VcError('strings: {"offset": [payload per image], "residual": [payload per image]}')
        dev = self.offset_compressor.Gain.device
        return {k: hip.IransDecoder(strings[k], waves, dev) for k in ("offset", "residual")}

    def _decoder_inputs(self, strings, shape, coder, waves, xref1):
        """decompress()'s strings checked against the references: (what the compressors' decompress_t take -- the host-coded lists
        or uploaded decoders --, (hz, wz), the decoders whose error words this call has to read at its end)"""
        if not isinstance(strings, dict) or set(strings) != {"offset", "residual"}:
            raise hip.VcError('strings: {"offset": ..., "residual": ...}')
        hz, wz = int(shape[0]), int(shape[1])
        mine = []
        if coder == "device":
            if not all(isinstance(v, hip.IransDecoder) for v in strings.values()):
                strings = self.upload_payloads(strings, waves)
                mine = list(strings.values())
            images = strings["offset"].images
            fits = all(d.images == xref1.shape[0] and d.waves == int(waves) for d in strings.values())
        else:
            images = len(strings["offset"][1]) if len(strings["offset"]) == 2 else None
            fits = images == xref1.shape[0]
        if (64 * hz, 64 * wz) != tuple(xref1.shape[2:]) or not fits:
            raise hip.VcError(f"hyper-latent shape {hz}x{wz} / {images} image(s) / waves {waves} do not belong to references "
                              f"{tuple(xref1.shape)} and the strings")
        return strings, (hz, wz), mine


class FlowGuidedB(_BFrameBitstream):
    def __init__(self):
        super().__init__()
        self.feature_extractor = MS_Feature()
        self.flow_estimator = FlowNET()
        self.offset_temporal_conditioner = OffsetTemproalEnc()
        self.offset_compressor = Offset_ELIC()
        self.offset_diversity_l3 = OffsetDiversity(in_channel=128, magnitude=10)
        self.offset_diversity_l2 = OffsetDiversity(in_channel=96, magnitude=20)
        self.offset_diversity_l1 = OffsetDiversity(in_channel=64, magnitude=40)
        self.residue_temporal_conditioner = ResidualTemproalEnc()
        self.residual_compressor = Res_ELIC()
        self.reconstructor = Reconstuctor()

    # -- reference helpers with tensor arguments -----------------------------------------------------------
    def convert_scales(self, scale1, scale2, x=None):
        return _f32_round2(scale1), _f32_round2(scale2)

    def warp(self, img, flow):
        """m.py:262-282 on NCHW CUDA tensors."""
        _require_cuda(img)
        _require_cuda(flow)
        return hip.nhwc_to_nchw(hip.warp(hip.WARP_W3, hip.nchw_to_nhwc(img), hip.nchw_to_nhwc(flow)))

    def estimate_flow(self, xref1, xref2, down_ratio):
        _require_cuda(xref1)
        _require_cuda(xref2)
        return hip.nhwc_to_nchw(self.estimate_flow_t(hip.nchw_to_nhwc(xref1), hip.nchw_to_nhwc(xref2), down_ratio))

    # -- device path -----------------------------------------------------------------------------------------
    def estimate_flow_t(self, r1, r2, down_ratio):
        """m.py:84-102: both references pooled by 2*down_ratio into one zero-padded (x16) 6-channel buffer,
        FlowNET, crop, bilinear x down_ratio with the vectors scaled by down_ratio."""
        k = 2 * int(down_ratio)
        if r1.h % k or r1.w % k:
            raise hip.VcError(f"frame {r1.h}x{r1.w} is not divisible by 2*down_ratio={k}")
        h, w = r1.h // k, r1.w // k
        hp, wp = -(-h // 16) * 16, -(-w // 16) * 16
        buf = torch.zeros(r1.n * hp * wp * 6, dtype=torch.float32, device=r1.buf.device)
        pair = T(buf, r1.n, hp, wp, 6, hp * wp * 6, wp * 6, 6)
        L = hip.lib()
        for r, c0 in ((r1, 0), (r2, 3)):
            hip.check(L.vc_avgpool_reflectpad(hip.stream(), r.view(), pair.crop(h, w).channels(c0, c0 + 3).view(), k, 1.0),
                      "vc_avgpool_reflectpad")
        flow = self.flow_estimator.run(pair).crop(h, w)
        if down_ratio == 1:
            return flow
        return hip.upsample_bilinear(flow, int(down_ratio), align_corners=False, scale=float(down_ratio))

    def forward_device(self, xref1, xref2, scale1, scale2, xcur, s, down_ratio, bits, flow=None, feats1=None, feats2=None,
                       trace=None):
        """Synchronisation-free body of :meth:`forward` on channels-last views; returns x_hat (T) and appends
        12 x n rows to ``bits`` (offset: z, y_0..y_4; residual: z, y_0..y_4; each for the n images of the batch --
        independent frames of one hierarchy level can share a pass, see gop.code_gop_icip2024).

        ``flow`` (optional): the 4-channel half-resolution flow already chosen by :meth:`search_flow_t` (the
        reference recomputes estimate_flow(best down_ratio), the same function of the same inputs).
        ``feats1`` / ``feats2`` (optional): per image of the batch the ``feature_extractor`` outputs (l1, l2, l3) of
        its reference computed earlier -- a decoded frame serves several B-frames of a GOP as reference and its
        features do not change.
        ``trace``: a dict that receives the stages of the pass ("flow", "cond" = per level [wref1|wref2|fref1|fref2],
        "fcur", "offsets", "aligned", "offset" / "residual" = the codecs' own traces) for stage-wise parity checks."""
        dev, n = xcur.buf.device, xcur.n
        if xcur.h % 64 or xcur.w % 64:
            raise hip.VcError("frame size must be a multiple of 64 (the reference pads with utils.pad)")
        s1, s2 = self.convert_scales(scale1, scale2)
        if flow is None:
            flow = self.estimate_flow_t(xref1, xref2, down_ratio)
        if trace is not None:
            trace["flow"] = flow
        t_off, t_res = ({}, {}) if trace is not None else (None, None)
        chans = (64, 96, 128)
        # per level one buffer [wref1 | wref2 | fref1 | fref2 | fcur]: f_cond_inp = first four, f_inp = all five
        F_ = [T.empty(n, xcur.h >> (l + 1), xcur.w >> (l + 1), 5 * c, dev) for l, c in enumerate(chans)]
        sl = lambda l, j: F_[l].channels(j * chans[l], (j + 1) * chans[l])  # noqa: E731
        fref = []
        for j, (x, feats) in enumerate(((xref1, feats1), (xref2, feats2))):
            if feats is None:
                fref.append(self.feature_extractor.run(x, outs=[sl(l, 2 + j) for l in range(3)]))
            else:                                  # feats: per image a triple of single-image views
                for i, triple in enumerate(feats):
                    for l in range(3):
                        hip.axpby(triple[l], None, out=sl(l, 2 + j).images(i, i + 1))
                fref.append([sl(l, 2 + j) for l in range(3)])
        fref1, fref2 = fref
        fcur = self.feature_extractor.run(xcur, outs=[sl(l, 4) for l in range(3)])
        flows = []
        for l in range(3):                                   # get_warpedrefs_at_layer (m.py:104-119)
            fc1 = hip.axpby(flow.channels(0, 2), None, alpha=s1)
            fc2 = hip.axpby(flow.channels(2, 4), None, alpha=s2)
            flows.append((fc1, fc2))
            hip.warp(hip.WARP_W3, fref1[l], fc1, out=sl(l, 0))
            hip.warp(hip.WARP_W3, fref2[l], fc2, out=sl(l, 1))
            if l < 2:                                        # F.interpolate(scale_factor=0.5, bilinear) * 0.5
                flow = hip.avgpool_reflectpad(flow, 2, scale=0.5)
        cond = [F_[l].channels(0, 4 * chans[l]) for l in range(3)]
        oc = self.offset_compressor
        o1, o2, o3 = oc.code([F_[0]], [F_[1]], [F_[2]], cond[0], cond[1], cond[2],
                             lambda dst: self.offset_temporal_conditioner.run(cond[0], cond[1], cond[2], out=dst), s, bits,
                             trace=t_off)
        comp = []
        for l, (off, div) in enumerate(((o1, self.offset_diversity_l1), (o2, self.offset_diversity_l2),
                                        (o3, self.offset_diversity_l3))):
            hc = off.c // 2
            comp.append(div.run(fref1[l], off.channels(0, hc), flows[l][0], fref2[l], off.channels(hc, 2 * hc), flows[l][1]))
        rc = self.residual_compressor
        x1, x2, x3 = rc.code([fcur[0], comp[0]], [fcur[1], comp[1]], [fcur[2], comp[2]], comp[0], comp[1], comp[2],
                             lambda dst: self.residue_temporal_conditioner.run(comp[0], comp[1], comp[2], out=dst), s, bits,
                             res=(comp[0], comp[1], comp[2]), trace=t_res)
        if trace is not None:
            trace.update({"cond": cond, "fcur": fcur, "offsets": (o1, o2, o3), "aligned": comp, "offset": t_off, "residual": t_res})
        return self.reconstructor.run(x1, x2, x3)

    def forward(self, xref1, xref2, scale1, scale2, xcur, s, down_ratio):
        """m.py:181-260: NCHW CUDA tensors in, ``{"x_hat", "size", "rate"}`` out."""
        _require_frames(xref1, xref2, xcur)
        b, _, h, w = xcur.shape
        bits = BitCounter(xcur.device, max_rows=12 * b)
        x_hat = self.forward_device(hip.nchw_to_nhwc(xref1), hip.nchw_to_nhwc(xref2), scale1, scale2,
                                    hip.nchw_to_nhwc(xcur), s, down_ratio, bits)
        rows = bits.totals()
        size_offset, size_res = rows[:6 * b].sum(), rows[6 * b:].sum()
        num_pixels = h * w * b
        return {"x_hat": hip.nhwc_to_nchw(x_hat), "size": (size_offset + size_res).float(),
                "rate": (size_offset / num_pixels + size_res / num_pixels).float(),
                "size_offset": size_offset, "size_residual": size_res}

    # -- real bitstream (this project's own format: the reference has none for this model) ----------------
    SEARCH_RATIOS = (1, 2, 4, 8, 16)

    def _bitstream_pass(self, xref1, xref2, scale1, scale2, xcur, s, down_ratio, strings=None, shape=None, trace=None, coder="host",
                        waves=4, reader=None):
        """The stages of :meth:`forward_device` with the two compressors on their bitstream paths; ``xcur`` is None on the decoder,
        which runs the reference-only stages through the same launches on the same buffer layouts (the per-level buffers keep
        their fcur slice, unused): every tensor the entropy path reads comes out of the same kernel instances on both sides."""
        enc = xcur is not None
        dev, n = xref1.buf.device, xref1.n
        if xref1.h % 64 or xref1.w % 64 or (xref2.n, xref2.h, xref2.w) != (n, xref1.h, xref1.w):
            raise hip.VcError("frame size must be a multiple of 64 (the reference pads with utils.pad), both references alike")
        s1, s2 = self.convert_scales(scale1, scale2)
        flow = self.estimate_flow_t(xref1, xref2, down_ratio)
        chans = (64, 96, 128)
        # per level one buffer [wref1 | wref2 | fref1 | fref2 | fcur], as forward_device lays it out
        F_ = [T.empty(n, xref1.h >> (l + 1), xref1.w >> (l + 1), 5 * c, dev) for l, c in enumerate(chans)]
        sl = lambda l, j: F_[l].channels(j * chans[l], (j + 1) * chans[l])  # noqa: E731
        fref1 = self.feature_extractor.run(xref1, outs=[sl(l, 2) for l in range(3)])
        fref2 = self.feature_extractor.run(xref2, outs=[sl(l, 3) for l in range(3)])
        fcur = self.feature_extractor.run(xcur, outs=[sl(l, 4) for l in range(3)]) if enc else None
        flows = []
        for l in range(3):                                   # get_warpedrefs_at_layer (m.py:104-119)
            fc1 = hip.axpby(flow.channels(0, 2), None, alpha=s1)
            fc2 = hip.axpby(flow.channels(2, 4), None, alpha=s2)
            flows.append((fc1, fc2))
            hip.warp(hip.WARP_W3, fref1[l], fc1, out=sl(l, 0))
            hip.warp(hip.WARP_W3, fref2[l], fc2, out=sl(l, 1))
            if l < 2:
                flow = hip.avgpool_reflectpad(flow, 2, scale=0.5)
        cond = [F_[l].channels(0, 4 * chans[l]) for l in range(3)]

        def align(offs):
            comp = []
            for l, (off, div) in enumerate(zip(offs, (self.offset_diversity_l1, self.offset_diversity_l2, self.offset_diversity_l3))):
                hc = off.c // 2
                comp.append(div.run(fref1[l], off.channels(0, hc), flows[l][0], fref2[l], off.channels(hc, 2 * hc), flows[l][1]))
            return comp
        return self._coded_tail(F_ if enc else None, cond, self.offset_temporal_conditioner, align, [[f] for f in fcur] if enc else None,
                                self.residue_temporal_conditioner, s, strings, shape, trace, coder, waves, reader)

    def _checked_down_ratio(self, down_ratio):
        down_ratio = int(down_ratio)
        if down_ratio not in self.SEARCH_RATIOS:
            raise hip.VcError(f"down_ratio {down_ratio} is not one of {self.SEARCH_RATIOS}")
        return down_ratio

    def compress(self, xref1, xref2, scale1, scale2, xcur, s, down_ratio=None, trace=None, coder="host", waves=4):
        """Encode a B-frame for real.  NCHW CUDA tensors and host numbers as :meth:`forward`; ``down_ratio=None`` searches the
        flow resolution on the device (:meth:`search_flow_t`) and reads the choice to the host.  Returns ``{"strings": {"offset",
        "residual"} each [[[g0], ..., [g4]], [z]] with one byte string per image in every inner list, "shape": hyper-latent
        (h, w), "down_ratio", "x_hat": the reconstruction :meth:`decompress` rebuilds, "size": the real bit count (8 x string
        bytes), "size_estimate": -log2 p of the coded symbols on the device}``.  The convolutions run on the pipeline of
        hip.BITSTREAM_HS_MODE whatever VC_FP32_MODE says: both compressors' entropy parameters depend on every stage in front
        of them, so the whole pass decides how the strings are read.

        ``coder="device"`` codes the same integers with the interleaved coder on the GPU: "strings" is then
        ``{"offset": [payload per image], "residual": [...]}``, the result gains "coder" and "waves" (the wave count the decoder needs),
        "size" is still 8 x the bytes of all payloads and x_hat is bit for bit that of the host-coded call."""
        _require_frames(xref1, xref2, xcur)
        _check_coder(coder, waves)
        s = self._coding_level(s)
        r1, r2, c = hip.nchw_to_nhwc(xref1), hip.nchw_to_nhwc(xref2), hip.nchw_to_nhwc(xcur)
        if down_ratio is None:                 # (the choice travels in the stream: the search itself needs no pinning)
            _, choice, _ = self.search_flow_t(c, r1, r2, scale1, scale2, self.SEARCH_RATIOS)
            picks = sorted({self.SEARCH_RATIOS[int(k)] for k in choice.cpu().tolist()})
            if len(picks) != 1:
                raise hip.VcError(f"the images of the batch choose different flow resolutions {picks}: encode them one by one")
            down_ratio = picks[0]
        down_ratio = self._checked_down_ratio(down_ratio)
        with hip.fp32_mode_pinned(hip.BITSTREAM_HS_MODE):
            out = self._bitstream_pass(r1, r2, scale1, scale2, c, s, down_ratio, trace=trace, coder=coder, waves=waves)
        result = self._compress_result(out, coder, waves)
        result["down_ratio"] = down_ratio
        return result

    def decompress(self, xref1, xref2, scale1, scale2, strings, shape, s, down_ratio, trace=None, coder="host", waves=4, reader=None):
        """Decode the strings of :meth:`compress` from the two references alone: ``{"x_hat"}``.  ``coder="device"`` reads the
        payloads of ``compress(coder="device")`` (``waves`` as it returned it): one upload, then launches only -- no copy to the
        host and no synchronisation until x_hat is enqueued -- and one read of the decoders' error words at the end (VcError).
        ``strings`` may be the result of :meth:`upload_payloads`; that last read is then the caller's.  ``reader``: the pass reader
        of the payloads in place of the compressors' own (DeviceChainReader); tools/seq_codec_bench.py measures the other."""
        _require_frames(xref1, xref2)
        _check_coder(coder, waves)
        s = self._coding_level(s)
        down_ratio = self._checked_down_ratio(down_ratio)
        strings, shape, mine = self._decoder_inputs(strings, shape, coder, waves, xref1)
        with hip.fp32_mode_pinned(hip.BITSTREAM_HS_MODE):
            out = self._bitstream_pass(hip.nchw_to_nhwc(xref1), hip.nchw_to_nhwc(xref2), scale1, scale2, None, s, down_ratio,
                                       strings=strings, shape=shape, trace=trace, reader=reader)
        for d in mine:
            d.finish()
        return {"x_hat": out["x_hat"]}

    # -- motion-adaptive flow resolution (opt_helpers.py:23-51) --------------------------------------------
    def _predict_from_flow(self, flow, xref1, xref2, s1, s2):
        f21 = hip.upsample_bilinear(flow.channels(0, 2), 2, align_corners=False, scale=2.0)
        f12 = hip.upsample_bilinear(flow.channels(2, 4), 2, align_corners=False, scale=2.0)
        f21 = hip.axpby(f21, None, alpha=s1, out=f21)
        f12 = hip.axpby(f12, None, alpha=s2, out=f12)
        w1 = hip.warp(hip.WARP_W3, xref1, f21)
        w2 = hip.warp(hip.WARP_W3, xref2, f12)
        return hip.axpby(w1, w2, alpha=0.5, beta=0.5, out=w1)

    def prediction_flowonly_t(self, xcur, xref1, xref2, scale1, scale2, down_ratio):
        s1, s2 = self.convert_scales(scale1, scale2)
        return self._predict_from_flow(self.estimate_flow_t(xref1, xref2, down_ratio), xref1, xref2, s1, s2)

    def search_flow_t(self, xcur, xref1, xref2, scale1, scale2, ratios=(1, 2, 4, 8, 16)):
        """get_best_down_ratio_prediction (opt_helpers.py:41-51) without a host round trip: every candidate
        flow is estimated and scored (MSE of the clamped warped-average prediction) on the device, and
        vc_select_flow copies the winner (per image of the batch).  Returns (flow T [n,H/2,W/2,4], choice int32[n] =
        index into ``ratios``, sse float64[n, len(ratios)]); the flow feeds forward_device(flow=...)."""
        s1, s2 = self.convert_scales(scale1, scale2)
        L, dev = hip.lib(), xcur.buf.device
        slots = L.vc_bits_slots()
        n, nr = xcur.n, len(ratios)
        partial = torch.empty(n * nr * slots, dtype=torch.float64, device=dev)
        sse = torch.empty(n * nr, dtype=torch.float64, device=dev)         # [image][ratio]
        flows = []
        for i, dr in enumerate(ratios):
            flow = self.estimate_flow_t(xref1, xref2, dr)
            pred = self._predict_from_flow(flow, xref1, xref2, s1, s2)
            for j in range(n):                                                # every frame of the batch decides for itself
                hip.check(L.vc_sse_clamp01(hip.stream(), pred.images(j, j + 1).view(), xcur.images(j, j + 1).view(),
                                           partial.data_ptr() + 8 * (j * nr + i) * slots, slots), "vc_sse_clamp01")
            flows.append(flow)
        hip.check(L.vc_bits_reduce(hip.stream(), partial.data_ptr(), slots, n * nr, sse.data_ptr()), "vc_bits_reduce")
        out = T.empty(n, flows[0].h, flows[0].w, 4, dev)
        choice = torch.empty(n, dtype=torch.int32, device=dev)
        for j in range(n):
            views = (hip.View * nr)(*[f.images(j, j + 1).view() for f in flows])
            hip.check(L.vc_select_flow(hip.stream(), sse.data_ptr() + 8 * j * nr, nr, float(xcur.h * xcur.w * xcur.c), views,
                                       out.images(j, j + 1).view(), choice.data_ptr() + 4 * j), "vc_select_flow")
        return out, choice, sse.view(n, nr)


def prediction_flowonly(model, xcur, xref1, xref2, scale1, scale2, down_ratio):
    """opt_helpers.py:23-38 on NCHW CUDA tensors."""
    _require_frames(xref1, xref2, xcur)
    t = model.prediction_flowonly_t(hip.nchw_to_nhwc(xcur), hip.nchw_to_nhwc(xref1), hip.nchw_to_nhwc(xref2),
                                    scale1, scale2, down_ratio)
    return hip.nhwc_to_nchw(t)


def get_best_down_ratio_prediction(model, xref1, xref2, scale1, scale2, xcur, level=None, beta=None):
    """opt_helpers.py:41-51: the flow resolution whose warped-average prediction has the best PSNR.
    The five candidate predictions are computed on the device; the five MSE scalars are compared on the host."""
    _require_frames(xref1, xref2, xcur)
    c, r1, r2 = hip.nchw_to_nhwc(xcur), hip.nchw_to_nhwc(xref1), hip.nchw_to_nhwc(xref2)
    L, ratios = hip.lib(), (1, 2, 4, 8, 16)
    slots = L.vc_bits_slots()
    partial = torch.empty(len(ratios) * slots, dtype=torch.float64, device=xcur.device)
    sse = torch.empty(len(ratios), dtype=torch.float64, device=xcur.device)
    for i, down_ratio in enumerate(ratios):       # squared error of the clamped prediction: vc_sse_clamp01, no torch operator on pixels
        pred = model.prediction_flowonly_t(c, r1, r2, scale1, scale2, down_ratio)
        hip.check(L.vc_sse_clamp01(hip.stream(), pred.view(), c.view(), partial.data_ptr() + 8 * i * slots, slots), "vc_sse_clamp01")
    hip.check(L.vc_bits_reduce(hip.stream(), partial.data_ptr(), slots, len(ratios), sse.data_ptr()), "vc_bits_reduce")
    count = float(xcur.numel())
    best, best_ratio = 0.0, None
    for down_ratio, e in zip(ratios, sse.cpu().tolist()):
        psnr = float(np.float32(10.0) * np.log10(np.float32(1.0) / np.float32(e / count))) if e > 0 else float("inf")
        if psnr > best:
            best, best_ratio = psnr, down_ratio
    return best_ratio, torch.tensor(best, dtype=torch.float32)        # (a tensor, as opt_helpers.py:51 returns one)


# ------------------------------------------------------------------------------------------------
# utils.py: GOP-16 bookkeeping of the test loop (src/test.py:37-101)
# ------------------------------------------------------------------------------------------------
def get_scales(order, order1, order2):
    if order2 - order1 == 0:
        return 0, 0
    return (order - order1) / (order2 - order1), (order - order2) / (order1 - order2)


def select_references(xcur, order, buffer, buffer_order):
    """utils.py:153-177: the two buffered frames closest in display order (ties broken like torch.topk on the
    |distance| list), returned as (past-side ref, future-side ref, their orders)."""
    d = [abs(i - order) for i in buffer_order]
    k = 1 if len(buffer) == 1 else 2
    ind = list(torch.topk(torch.from_numpy(np.array(d)), k, largest=False).indices.numpy())
    if k == 1:
        return buffer[ind[0]], buffer[ind[0]], buffer_order[ind[0]], buffer_order[ind[0]]
    lo, hi = ind[1], ind[0]
    if buffer_order[ind[0]] < buffer_order[ind[1]]:
        lo, hi = ind[0], ind[1]
    return buffer[lo], buffer[hi], buffer_order[lo], buffer_order[hi]


def update_buffer(buffer, buffer_order, new_frame, order, l=32):
    nb, no = buffer + [new_frame], buffer_order + [order]
    return (nb, no) if len(buffer) < l else (nb[1:], no[1:])


def get_order_typ_list(intra_size, frame_number):
    """utils.py:188-221 including the hard-coded tails for 300- and 600-frame UVG sequences."""
    order = [16, 8, 4, 12, 2, 14, 6, 10, 1, 15, 3, 13, 5, 11, 7, 9]
    o = [0] + [order[i % 16] + (i // 16) * 16 for i in range(frame_number - 1)]
    ff = (frame_number - 1) % intra_size
    if ff != 0:
        m = max(o[:-ff])
        o[-ff:] = [m + ff - i for i in range(ff)]
    typ = ["I" if i % intra_size == 0 else "B" for i in range(frame_number)]
    typ[-1] = "I"
    if frame_number == 300:
        o[-11:] = [299, 293, 290, 296, 289, 291, 292, 294, 295, 297, 298]
    if frame_number == 600:
        o[-7:] = [599, 595, 593, 597, 594, 596, 598]
    return o, typ
