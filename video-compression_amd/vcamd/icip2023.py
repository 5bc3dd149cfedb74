"""ICIP2023 multi-scale deformable B-frame codec on MI355X -- host-side mirror of the reference surface.

Drop-in for (under ICIP2023/src of the reference):
  model/m.py:20-137              DeformB                                              -> :class:`DeformB`
  model/helpers.py:15-147        MS_Feature, Reconstuctor, OffsetTemproalEnc, ResidualTemproalEnc -> same names
  model/offset_res_elic.py       Offset_ELIC / Res_ELIC                               -> same names
  model/elic.py                  ResidualBottleneckBlock, the ELIC intra codec        -> vcamd.icip2024 (the files are identical)
  test.py:36-94                  val_sequence_level                                   -> vcamd.gop.code_sequence_icip2023
DeformB is the ancestor of ICIP2024's FlowGuidedB: the same pyramid, temporal conditioners, compressors and reconstructor at
other widths, no flow network, and in place of OffsetDiversity two plain modulated DeformConv2d(c, c, 3, groups=8) layers per
level whose outputs are concatenated.  Every class here is the ICIP2024 class built with DeformB's arguments; the state_dict
keys are the reference's (1034 entries, tests/golden/icip2023_state_schema.txt).

Per level the two deformable layers run as ONE launch (vc_deform_pair: a grouped deformable convolution of 16 groups, groups 0..7
on fref1 with the first layer's weights, 8..15 on fref2 with the second's; offsets used as they come, logistic on the mask; in fp16
mode on group-planar half copies of the two references, vc_deform_pair_hxp -- hip.HALF_DEFORM_PAIR).
Per level one buffer [fref1 | fref2 | fcur] holds what the reference concatenates: f_inp is the buffer, f_cond_inp its first two
thirds, so no concatenation is launched.  The reference has no compress() for this model; compress / decompress here are the
twelve strings per frame of FlowGuidedB's format (vcamd/icip2024.py: _Elic.compress_t / decompress_t), without a container.
"""
from . import hip, icip2024
from .hip import T
from .icip2024 import DeformConv2d, deconv, get_order_typ_list, select_references, update_buffer  # noqa: F401
from .layers import BitCounter
from .lhbdc import _require_frames

CHANS = (32, 64, 96)              # feature widths of the three pyramid levels (1/2, 1/4, 1/8 resolution)
OFFSET_HEAD = 27 * 8 * 2          # per level: for each reference 8 groups x 9 taps x (x, y, mask)


class MS_Feature(icip2024.MS_Feature):
    def __init__(self):
        super().__init__(CHANS)


class OffsetTemproalEnc(icip2024._TemporalEnc):
    """helpers.py:94-119: reads f_cond_inp = [fref1 | fref2] of every level"""

    def __init__(self, N=128, M=128):
        super().__init__(2, N, M, CHANS)


class ResidualTemproalEnc(icip2024._TemporalEnc):
    """helpers.py:122-147: reads x_comp = [aligned fref1 | aligned fref2] of every level"""

    def __init__(self, N=128, M=128):
        super().__init__(2, N, M, CHANS)


class Reconstuctor(icip2024.Reconstuctor):
    """helpers.py:55-91: widths 64 / 128 / 192 (x_comp is 2c wide), levels end with a 3x3 transposed convolution"""

    def __init__(self):
        super().__init__(tuple(2 * c for c in CHANS), up=lambda cin, cout: deconv(cin, cout, kernel_size=3, stride=2))


class Offset_ELIC(icip2024._Elic):
    """offset_res_elic.py:72-315: encoder on [fref1 | fref2 | fcur] (3c), decoder side input [fref1 | fref2] (2c)"""

    def __init__(self, N=128, M=128, **kwargs):
        super().__init__(3, 2, (OFFSET_HEAD,) * 3, N, M, chans=CHANS)


class Res_ELIC(icip2024._Elic):
    """offset_res_elic.py:318-566: g_a0 on the frame, then [y | fcur | x_comp] (N + 3c) per level; heads of 2c channels"""

    def __init__(self, N=128, M=128, **kwargs):
        super().__init__(3, 2, tuple(2 * c for c in CHANS), N, M, chans=CHANS, stem=True)


class DeformB(icip2024._BFrameBitstream):
    def __init__(self):
        super().__init__()
        self.feature_extractor = MS_Feature()
        self.offset_temp_encoder = OffsetTemproalEnc()
        self.offset_compressor = Offset_ELIC()
        for level, c in zip((3, 2, 1), reversed(CHANS)):
            for r in (1, 2):
                setattr(self, f"deconv_l{level}_{r}", DeformConv2d(c, c, kernel_size=3, padding=1, groups=8))
        self.reconstructor = Reconstuctor()
        self.residual_temp_encoder = ResidualTemproalEnc()
        self.residual_compressor = Res_ELIC()
        self._pairs = {}

    def _load_from_state_dict(self, *args, **kwargs):
        self._pairs = {}
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *a, **k):
        self._pairs = {}
        return super()._apply(fn, *a, **k)

    def _pair(self, level):
        """the two layers of a level packed as one 16-group convolution (hip.PackedDeform.from_pair)"""
        if level not in self._pairs:
            self._pairs[level] = hip.PackedDeform.from_pair(getattr(self, f"deconv_l{level}_1"), getattr(self, f"deconv_l{level}_2"))
        return self._pairs[level]

    def get_deformed_maps_t(self, offset, fref1, fref2, level, out=None):
        """m.py:72-86 on channels-last views in one launch: ``offset`` is the level's 432-channel head, its halves the raw records
        [x-block | y-block | mask-block] of the two references."""
        hc = offset.c // 2
        return self._pair(level).pair(fref1, offset.channels(0, hc), fref2, offset.channels(hc, 2 * hc), out=out)

    # -- device path -----------------------------------------------------------------------------------------
    def _features(self, xref1, xref2, xcur, feats1=None, feats2=None):
        """per level one buffer [fref1 | fref2 | fcur]; returns (buffers, fref1, fref2, fcur or None)"""
        dev, n = xref1.buf.device, xref1.n
        F_ = [T.empty(n, xref1.h >> (l + 1), xref1.w >> (l + 1), 3 * c, dev) for l, c in enumerate(CHANS)]
        sl = lambda l, j: F_[l].channels(j * CHANS[l], (j + 1) * CHANS[l])  # noqa: E731
        fref = []
        for j, (x, feats) in enumerate(((xref1, feats1), (xref2, feats2))):
            if feats is None:
                fref.append(self.feature_extractor.run(x, outs=[sl(l, j) for l in range(3)]))
            else:                                  # feats: per image a triple of single-image views
                for i, triple in enumerate(feats):
                    for l in range(3):
                        hip.axpby(triple[l], None, out=sl(l, j).images(i, i + 1))
                fref.append([sl(l, j) for l in range(3)])
        fcur = self.feature_extractor.run(xcur, outs=[sl(l, 2) for l in range(3)]) if xcur is not None else None
        return F_, fref[0], fref[1], fcur

    def forward_device(self, xref1, xref2, xcur, s, bits, feats1=None, feats2=None, trace=None, force=None):
        """Synchronisation-free body of :meth:`forward` on channels-last views; returns x_hat (T) and appends 12 x n rows to
        ``bits`` (offset: z, y_0..y_4; residual: z, y_0..y_4; each for the n images of the batch).

        ``feats1`` / ``feats2`` (optional): per image of the batch the ``feature_extractor`` outputs (l1, l2, l3) of its reference
        computed earlier.  ``trace``: a dict that receives "fcur" (three levels), "offsets" (the three heads), "x_comp" (the three
        aligned maps BEFORE the residual is added) and "offset" / "residual", the codecs' own traces.  ``force``: ``{"offset": fn,
        "residual": fn}`` handed to the two codecs (icip2024._Elic.code: teacher forcing of the latents for parity checks)."""
        if xcur.h % 64 or xcur.w % 64:
            raise hip.VcError("frame size must be a multiple of 64 (the reference pads with utils.pad)")
        t_off, t_res = ({}, {}) if trace is not None else (None, None)
        F_, fref1, fref2, fcur = self._features(xref1, xref2, xcur, feats1, feats2)
        cond = [F_[l].channels(0, 2 * CHANS[l]) for l in range(3)]
        offs = self.offset_compressor.code([F_[0]], [F_[1]], [F_[2]], cond[0], cond[1], cond[2],
                                           lambda dst: self.offset_temp_encoder.run(cond[0], cond[1], cond[2], out=dst), s, bits,
                                           trace=t_off, force=force and force.get("offset"))
        comp = [self.get_deformed_maps_t(offs[l], fref1[l], fref2[l], l + 1) for l in (2, 1, 0)][::-1]
        xs = self.residual_compressor.code([xcur, fcur[0], comp[0]], [fcur[1], comp[1]], [fcur[2], comp[2]], comp[0], comp[1], comp[2],
                                           lambda dst: self.residual_temp_encoder.run(comp[0], comp[1], comp[2], out=dst), s, bits,
                                           res=tuple(comp), trace=t_res, force=force and force.get("residual"))
        if trace is not None:
            trace.update({"fcur": fcur, "offsets": offs, "x_comp": comp, "offset": t_off, "residual": t_res})
        return self.reconstructor.run(*xs)

    def forward(self, xref1, xref2, xcur, s):
        """m.py:96-137: NCHW CUDA tensors in, ``{"x_hat", "size", "rate"}`` out (plus the two codecs' shares of the size)."""
        _require_frames(xref1, xref2, xcur)
        b, _, h, w = xcur.shape
        bits = BitCounter(xcur.device, max_rows=12 * b)
        x_hat = self.forward_device(hip.nchw_to_nhwc(xref1), hip.nchw_to_nhwc(xref2), hip.nchw_to_nhwc(xcur), s, bits)
        rows = bits.totals()
        size_offset, size_res = rows[:6 * b].sum(), rows[6 * b:].sum()
        num_pixels = h * w * b
        return {"x_hat": hip.nhwc_to_nchw(x_hat), "size": (size_offset + size_res).float(),
                "rate": (size_offset / num_pixels + size_res / num_pixels).float(),
                "size_offset": size_offset, "size_residual": size_res}

    # -- real bitstream (FlowGuidedB's strings; the reference has none for this model) ---------------------------------------
    def _bitstream_pass(self, xref1, xref2, xcur, s, strings=None, shape=None, trace=None, coder="host", waves=4, reader=None):
        """The stages of :meth:`forward_device` with the two compressors on their bitstream paths; ``xcur`` is None on the decoder,
        which runs the reference-only stages through the same launches on the same buffer layouts (the per-level buffers keep
        their fcur slice, unused)."""
        enc = xcur is not None
        if xref1.h % 64 or xref1.w % 64 or (xref2.n, xref2.h, xref2.w) != (xref1.n, xref1.h, xref1.w):
            raise hip.VcError("frame size must be a multiple of 64 (the reference pads with utils.pad), both references alike")
        F_, fref1, fref2, fcur = self._features(xref1, xref2, xcur)
        cond = [F_[l].channels(0, 2 * CHANS[l]) for l in range(3)]
        align = lambda offs: [self.get_deformed_maps_t(offs[l], fref1[l], fref2[l], l + 1) for l in (2, 1, 0)][::-1]  # noqa: E731
        return self._coded_tail(F_ if enc else None, cond, self.offset_temp_encoder, align,
                                [[xcur, fcur[0]], [fcur[1]], [fcur[2]]] if enc else None, self.residual_temp_encoder, s, strings, shape,
                                trace, coder, waves, reader)

    def compress(self, xref1, xref2, xcur, s, trace=None, coder="host", waves=4):
        """Encode a B-frame for real.  NCHW CUDA tensors as :meth:`forward`.  Returns ``{"strings": {"offset", "residual"} each
        [[[g0], ..., [g4]], [z]] with one byte string per image in every inner list, "shape": hyper-latent (h, w), "x_hat": the
        reconstruction :meth:`decompress` rebuilds, "size": the real bit count (8 x string bytes), "size_estimate": -log2 p of the
        coded symbols on the device}``.  The convolutions run on the pipeline of hip.BITSTREAM_HS_MODE, as FlowGuidedB.compress
        explains.  ``coder="device"``: "strings" is ``{"offset": [payload per image], "residual": [...]}`` of the interleaved coder,
        the result gains "coder" and "waves"; x_hat is bit for bit that of the host-coded call."""
        _require_frames(xref1, xref2, xcur)
        icip2024._check_coder(coder, waves)
        s = self._coding_level(s)
        with hip.fp32_mode_pinned(hip.BITSTREAM_HS_MODE):
            out = self._bitstream_pass(hip.nchw_to_nhwc(xref1), hip.nchw_to_nhwc(xref2), hip.nchw_to_nhwc(xcur), s, trace=trace,
                                       coder=coder, waves=waves)
        return self._compress_result(out, coder, waves)

    def decompress(self, xref1, xref2, strings, shape, s, trace=None, coder="host", waves=4, reader=None):
        """Decode the strings of :meth:`compress` (or the result of ``upload_payloads``) from the two references alone: ``{"x_hat"}``.
        ``coder="device"`` reads the payloads of ``compress(coder="device")`` (one upload, then launches only) and looks at the
        decoders' error words once, at the end: a damaged payload raises VcError after the reconstruction is enqueued.  ``reader``:
        as FlowGuidedB.decompress."""
        _require_frames(xref1, xref2)
        icip2024._check_coder(coder, waves)
        s = self._coding_level(s)
        strings, shape, mine = self._decoder_inputs(strings, shape, coder, waves, xref1)
        with hip.fp32_mode_pinned(hip.BITSTREAM_HS_MODE):
            out = self._bitstream_pass(hip.nchw_to_nhwc(xref1), hip.nchw_to_nhwc(xref2), None, s, strings=strings, shape=shape,
                                       trace=trace, reader=reader)
        for d in mine:
            d.finish()
        return {"x_hat": out["x_hat"]}
