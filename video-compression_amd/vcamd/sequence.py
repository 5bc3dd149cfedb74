"""The ICIP2024 models as an end-to-end codec: a sequence of frames in, ONE byte string out (the ``VCSQ`` file of vcamd.containers;
layout in INTEGRATION.md), and the frames back from that string and the two models alone.

The loop is the reference's ``val_sequence_level`` as gop.code_sequence_icip2024 walks it -- coding order and frame types from
icip2024.get_order_typ_list, references = the two decoded frames (clamped to [0, 1], at most 32 kept) closest in display order
(select_references / update_buffer), scales from get_scales -- with real bits in place of the -log2 p sums: I-frames through
``ELIC.compress(coder="device")`` (``VCII`` records), B-frames through ``FlowGuidedB.compress(down_ratio=None, coder="device")``, the
device search (``VCID`` records).  The decoder derives order, types, references and scales exactly as the encoder does; per frame it
uploads the payloads once and enqueues launches only, and it reads the decoders' error words after the last frame is enqueued.

:class:`LhbdcSequenceCodec` (below) does the same for LHBDC -- GOP-8 B-frames between mbt2018_mean I-frames, the ``VCLS`` file -- and
stores a hash of every decoded picture that the decoder recomputes."""
import torch

from . import containers, hip, icip2024
from .gop import LEVEL_GROUPS

INTRA_QUALITIES = 256


class Icip2024SequenceCodec:
    """``model``: icip2024.FlowGuidedB, ``i_model``: icip2024.ELIC (both on the device, ``update(force=True)`` done); ``waves``: the
    sub-streams per payload; ``intra_quality``: the quality index of ``i_model``, carried in the file and checked by the decoder (a
    file coded with another I-frame model is refused)."""

    def __init__(self, model, i_model, waves=4, intra_quality=0):
        if not hip.irans_waves_ok(waves) or not 0 <= int(intra_quality) < INTRA_QUALITIES:
            raise hip.VcError(f"waves {waves!r} (a power of two in 1..16) / intra quality index {intra_quality!r} (0..255)")
        self.model, self.i_model, self.waves, self.intra_quality = model, i_model, int(waves), int(intra_quality)
        self.report = None

    @staticmethod
    def _padded(h, w):
        return h + (64 - h % 64) % 64, w + (64 - w % 64) % 64

    def encode(self, load_frame, n_frames, level, h, w, intra_size=16):
        """``load_frame(i)``: the padded NCHW CUDA frame of display order i (one image); ``h`` x ``w``: the picture before padding.
        Returns ``(data, {order: x_hat})``: the file and the reconstruction of every frame (padded NCHW, as the decoder rebuilds
        it).  ``self.report`` then holds, per display order, ``"size_bits"`` (8 x the record's container bytes) and
        ``"estimate_bits"`` (the device's -log2 p of the coded symbols)."""
        plan = containers.sequence_plan(intra_size, n_frames)
        level = self.model._coding_level(level)
        hp, wp = self._padded(int(h), int(w))
        records, recon, sizes, estimates = [], {}, {}, {}
        buffer, buffer_order = [], []
        for order, typ in plan:
            cur = load_frame(order)
            if tuple(cur.shape) != (1, 3, hp, wp):
                raise hip.VcError(f"frame {order}: {tuple(cur.shape)} is not the padded picture (1, 3, {hp}, {wp})")
            if typ == "I":
                out = self.i_model.compress(cur, coder="device", waves=self.waves)
                blob = containers.pack_icip2024_intra_dev(out["strings"][0], out["shape"], self.waves)
                estimate = out["bits"]
            else:
                ref1, ref2, o1, o2 = icip2024.select_references(None, order, buffer, buffer_order)
                s1, s2 = icip2024.get_scales(order, o1, o2)
                out = self.model.compress(ref1, ref2, s1, s2, cur, level, down_ratio=None, coder="device", waves=self.waves)
                c1, c2 = self.model.convert_scales(s1, s2)
                blob = containers.pack_icip2024_frame_dev(out["strings"], out["shape"], out["down_ratio"], level, c1, c2, self.waves)
                estimate = out["size_estimate"]
            records.append((typ, order, blob))
            recon[order] = out["x_hat"]
            sizes[order], estimates[order] = 8 * len(blob), estimate
            buffer, buffer_order = icip2024.update_buffer(buffer, buffer_order, hip.clamp01_nchw(out["x_hat"]), order)
        self.report = {"size_bits": sizes, "estimate_bits": {o: float(e) for o, e in estimates.items()}}
        return containers.pack_sequence(records, w, h, intra_size, level, self.intra_quality), recon

    def decode(self, data, frames=None):
        """The frames of :meth:`encode`'s file, ``{order: x_hat}`` (padded NCHW), from the bytes alone.  Every container is
        validated before anything is enqueued; per frame one upload, then launches only; the error words of all decoders are read
        after the last frame is enqueued, every one of them before the first VcError is raised.  ``frames``: a dict that receives
        the frames as well -- it stays filled when a VcError is raised (the frames in front of a corrupt payload are whole, it and
        the frames that reference it are not)."""
        seq = containers.unpack_sequence(data)
        if seq["intra_quality"] != self.intra_quality:
            raise hip.VcError(f"sequence file: coded with I-frame quality index {seq['intra_quality']}, this codec holds {self.intra_quality}")
        hp, wp = self._padded(seq["height"], seq["width"])
        shape = (hp // 64, wp // 64)
        parsed = []
        for typ, order, blob in seq["records"]:
            got = containers.unpack_icip2024_intra_dev(blob) if typ == "I" else containers.unpack_icip2024_frame_dev(blob)
            if tuple(got["shape"]) != shape:
                raise hip.VcError(f"frame {order}: hyper-latent shape {got['shape']} does not belong to a {seq['width']}x{seq['height']} picture")
            if typ == "B" and got["s"] != seq["s"]:
                raise hip.VcError(f"frame {order}: quality level {got['s']} is not the file's {seq['s']}")
            parsed.append((typ, order, got))
        dev = self.i_model.entropy_bottleneck.quantiles.device
        frames = {} if frames is None else frames
        decoders, buffer, buffer_order = [], [], []
        for typ, order, got in parsed:
            if typ == "I":
                dec = hip.IransDecoder([got["payload"]], got["waves"], dev)
                decoders.append(dec)
                x_hat = self.i_model.decompress(dec, got["shape"], coder="device", waves=got["waves"])["x_hat"]
            else:
                ref1, ref2, o1, o2 = icip2024.select_references(None, order, buffer, buffer_order)
                s1, s2 = icip2024.get_scales(order, o1, o2)
                if (got["scale1"], got["scale2"]) != self.model.convert_scales(s1, s2):
                    raise hip.VcError(f"frame {order}: scales {got['scale1']}, {got['scale2']} are not those of references {o1}, {o2}")
                uploaded = self.model.upload_payloads(got["strings"], got["waves"])
                decoders.extend(uploaded.values())
                x_hat = self.model.decompress(ref1, ref2, s1, s2, uploaded, got["shape"], got["s"], got["down_ratio"], coder="device",
                                              waves=got["waves"])["x_hat"]
            frames[order] = x_hat
            buffer, buffer_order = icip2024.update_buffer(buffer, buffer_order, hip.clamp01_nchw(x_hat), order)
        containers.finish_all(decoders)
        return frames


def crop_uint8(x_hat, h, w):
    """uint8 RGB [h, w, 3] (host) of the unpadded picture of one decoded frame"""
    return hip.frame_to_uint8(x_hat[:1], int(h), int(w)).cpu().numpy()


def load_models(seeded=None, weights=None, i_weights=None, device=None):
    """(FlowGuidedB, ELIC) ready to code: checkpoints (a state dict, or a dict with one under "state_dict"), or with ``seeded`` the
    deterministic synthetic checkpoints of vcamd.seeding (encoder and decoder must use the same seed)."""
    from .seeding import seeded_state_dict
    device = device or torch.device("cuda")
    model, intra = icip2024.FlowGuidedB(), icip2024.ELIC()
    if seeded is not None:
        model.load_state_dict(seeded_state_dict(model.state_dict(), seed=int(seeded)))
        intra.load_state_dict(seeded_state_dict(intra.state_dict(), seed=int(seeded), conv_gain=0.8))
    else:
        if not weights or not i_weights:
            raise hip.VcError("the ICIP2024 checkpoints are a separate download: pass --weights PATH and --i_weights PATH, or --seeded SEED "
                              "for the synthetic checkpoints")
        for m, path in ((model, weights), (intra, i_weights)):
            sd = torch.load(path, map_location="cpu")
            m.load_state_dict(sd["state_dict"] if isinstance(sd, dict) and "state_dict" in sd else sd)
    model, intra = model.to(device).eval(), intra.to(device).eval()
    model.offset_compressor.update(force=True)
    model.residual_compressor.update(force=True)
    intra.update(force=True)
    return model, intra


# ------------------------------------------------------------------------------------------------
# LHBDC: GOP-8 B-frames between mbt2018_mean I-frames, one ``VCLS`` file, a hash of every decoded picture
# ------------------------------------------------------------------------------------------------
class LhbdcSequenceCodec:
    """``model``: lhbdc.Model, ``i_model``: iframe.ImageMeanScaleHyperprior (both on the device, ``update(force=True)`` done);
    ``lmbda``: the B-model's operating point, carried in the file and in every ``VCLD`` record; ``waves``: the sub-streams per payload
    (the decoder takes the count from the containers); ``intra_quality``: the mbt2018_mean quality of ``i_model`` (1..8), carried in
    the file and checked by the decoder; ``picture_hash``: store hip.picture_hash of every reconstruction in the file.

    The loop is gop.code_sequence_lhbdc's with real bits (containers.lhbdc_sequence_plan): I-frames through
    ``ImageMeanScaleHyperprior.compress(coder="device")`` (``VCLI`` records), the seven B-frames of every whole GOP through
    ``LhbdcStreamCodec(coder="device")`` (``VCLD`` records) between the DECODED I-frames, a boundary I-frame coded once; the frames
    behind the last whole GOP are I-frames.

    Why the hash: the entropy decode of an LHBDC frame depends on its own hyper-latents alone, never on the reference frames, so a
    decoder whose reconstructions drift from the encoder's (another VC_FP32_MODE, another build, another checkpoint, a damaged
    payload that still parses) decodes every symbol without an error word and returns wrong pictures.  The encoder therefore hashes
    each reconstruction on the device and the decoder recomputes it: the drift becomes a VcError that names the first bad frame."""

    def __init__(self, model, i_model, lmbda=1626, waves=4, intra_quality=7, picture_hash=True):
        from .bitstream import LhbdcStreamCodec
        if not hip.irans_waves_ok(waves) or not 1 <= int(intra_quality) <= 8 or not 0 <= int(lmbda) <= 0xffffffff:
            raise hip.VcError(f"waves {waves!r} (a power of two in 1..16) / intra quality {intra_quality!r} (1..8) / lambda {lmbda!r}")
        self.model, self.i_model, self.lmbda, self.waves = model, i_model, int(lmbda), int(waves)
        self.intra_quality, self.picture_hash = int(intra_quality), bool(picture_hash)
        self.stream = LhbdcStreamCodec(model, lmbda=self.lmbda, coder="device", waves=self.waves)
        self.report = None

    _padded = staticmethod(Icip2024SequenceCodec._padded)

    @staticmethod
    def _u64(values):
        return [int(v) & 0xffffffffffffffff for v in values]

    def encode(self, load_frame, n_frames, h, w):
        """``load_frame(i)``: the padded NCHW CUDA frame of display order i (one image, padded to multiples of 64); ``h`` x ``w``:
        the picture before padding.  Returns ``(data, {order: x_hat})``: the file and the reconstruction of every frame (padded
        NCHW, as the decoder rebuilds it).  ``self.report`` then holds ``"size_bits"`` (per display order, 8 x the record's
        container bytes), ``"estimate_bits"`` (the device's -log2 p, for the I-frames alone: the B-frame path has no estimate) and,
        with picture hashes, ``"hash"`` (per display order, the stored hash).  The hashes are read back once, after the last frame."""
        plan = containers.lhbdc_sequence_plan(n_frames)
        hp, wp = self._padded(int(h), int(w))
        blobs, recon, estimates, hashed = {}, {}, {}, []

        def load(order):
            cur = load_frame(order)
            if not isinstance(cur, torch.Tensor) or tuple(cur.shape) != (1, 3, hp, wp):
                raise hip.VcError(f"frame {order}: {tuple(getattr(cur, 'shape', ()))} is not the padded picture (1, 3, {hp}, {wp})")
            return cur

        def done(order, x_hat):
            recon[order] = x_hat
            if self.picture_hash:
                hashed.append((order, hip.picture_hash(x_hat)))

        def intra(order):
            out = self.i_model.compress(load(order), coder="device", waves=self.waves)
            blobs[order] = containers.pack_lhbdc_intra_dev(out["strings"][0], out["shape"], self.waves)
            estimates[order] = out["bits"]
            done(order, out["x_hat"])

        intra(0)
        for k in range((len(plan) - 1) // containers.LHBDC_GOP):
            first = containers.LHBDC_GOP * k
            intra(first + 8)
            gop = [None] + [load(first + o) for o in range(1, 8)] + [None]              # (the boundary frames enter decoded)
            coded, decoded = self.stream.encode_gop(gop, recon[first], recon[first + 8])
            for group in LEVEL_GROUPS:
                for o in group:
                    blobs[first + o] = coded[o]
                    done(first + o, decoded[o])
        for order, _ in plan[1 + 8 * ((len(plan) - 1) // containers.LHBDC_GOP):]:
            intra(order)
        hashes = None
        if self.picture_hash:
            hashes = dict(zip((o for o, _ in hashed), self._u64(torch.cat([t for _, t in hashed]).cpu().tolist())))
        est = torch.stack([estimates[o] for o in sorted(estimates)]).cpu().tolist()
        self.report = {"size_bits": {o: 8 * len(blobs[o]) for o, _ in plan}, "estimate_bits": dict(zip(sorted(estimates), est))}
        if hashes is not None:
            self.report["hash"] = hashes
        data = containers.pack_lhbdc_sequence([(t, o, blobs[o]) for o, t in plan], w, h, self.lmbda, self.intra_quality, hashes)
        return data, recon

    def decode(self, data, frames=None, verify=True):
        """The frames of :meth:`encode`'s file, ``{order: x_hat}`` (padded NCHW), from the bytes alone.  Every container is parsed
        and validated before anything is enqueued (the file's lambda against every ``VCLD`` record and against this codec, the intra
        quality against this codec, the latent shapes against the picture); per GOP uploads, then launches only; with ``verify``
        and hashes in the file one picture_hash launch behind every I-frame and every level.  The error words of all decoders and
        all hashes are read after the last frame is enqueued: a payload error is raised first, then ``VcError("frame <order>:
        decoded picture hash ...")`` for the first mismatching frame in coding order.  ``frames``: a dict that receives the frames
        as well -- it stays filled when a VcError is raised.  ``self.report``: ``{"verified": bool}`` -- False where nothing was
        compared (``verify=False``, or a file without hashes, which is no error) or a hash did not match -- and ``"hash"``, the
        recomputed hashes per display order, where they were computed."""
        from .bitstream import _walk_gop
        seq = containers.unpack_lhbdc_sequence(data)
        if seq["lmbda"] != self.lmbda or seq["intra_quality"] != self.intra_quality:
            raise hip.VcError(f"LHBDC sequence file: coded with lambda {seq['lmbda']} and I-frame quality {seq['intra_quality']}, this codec "
                              f"holds lambda {self.lmbda} and quality {self.intra_quality}")
        hp, wp = self._padded(seq["height"], seq["width"])
        parsed = {}
        for typ, order, blob in seq["records"]:
            if typ == "I":
                got = containers.unpack_lhbdc_intra_dev(blob)
                if tuple(got["shape"]) != (hp // 64, wp // 64):
                    raise hip.VcError(f"frame {order}: hyper-latent shape {got['shape']} does not belong to a {seq['width']}x{seq['height']} picture")
            else:
                got = containers.unpack_lhbdc_frame_dev(blob, hp, wp)
                if got["lmbda"] != seq["lmbda"]:
                    raise hip.VcError(f"frame {order}: lambda {got['lmbda']} is not the file's {seq['lmbda']}")
            parsed[order] = (blob, got)
        gops = (seq["frames"] - 1) // containers.LHBDC_GOP
        for k in range(gops):                      # (what upload_frames asks of the frames of one level, asked before the first launch)
            for group in LEVEL_GROUPS:
                heads = {(g["mv_shape"], g["res_shape"], g["waves"]) for g in (parsed[8 * k + o][1] for o in group)}
                if len(heads) != 1:
                    raise hip.VcError(f"frames {[8 * k + o for o in group]}: one level, different latent shapes or wave counts")
        dev = self.i_model.entropy_bottleneck.quantiles.device
        frames = {} if frames is None else frames
        check = bool(verify) and seq["hashes"] is not None
        decoders, hashed = [], []

        def done(orders, x_hat):
            if check:
                hashed.append((orders, hip.picture_hash(x_hat)))

        def intra(order):
            got = parsed[order][1]
            dec = hip.IransDecoder([got["payload"]], got["waves"], dev)
            decoders.append(dec)
            frames[order] = self.i_model.decompress(dec, got["shape"], coder="device", waves=got["waves"])["x_hat"]
            done([order], frames[order])

        intra(0)
        for k in range(gops):
            first = containers.LHBDC_GOP * k
            intra(first + 8)
            up = self.stream.upload_gop({o: parsed[first + o][0] for o in range(1, 8)}, frames[first])
            decoders.append(up)

            def level(j, group, xb, xa, up=up, first=first):
                x_hat = self.stream._decode_level_dev(xb, xa, up.levels[j])
                done([first + o for o in group], x_hat)
                return x_hat

            decoded = _walk_gop(frames[first], frames[first + 8], level)
            for o in range(1, 8):
                frames[first + o] = decoded[o]
        for order in range(containers.LHBDC_GOP * gops + 1, seq["frames"]):
            intra(order)
        # the one read: every error word, then every hash
        self.report = {"verified": False}
        payload_error = None
        try:
            containers.finish_all(decoders)
        except hip.VcError as e:
            payload_error = e
        if check:
            orders = [o for group, _ in hashed for o in group]
            self.report["hash"] = dict(zip(orders, self._u64(torch.cat([t for _, t in hashed]).cpu().tolist())))
        if payload_error is not None:
            raise payload_error
        if check:
            for order in orders:
                got, want = self.report["hash"][order], seq["hashes"][order]
                if got != want:
                    raise hip.VcError(f"frame {order}: decoded picture hash {got:#018x} is not the {want:#018x} the encoder stored -- this "
                                      "decoder's reconstruction differs from the encoder's (another checkpoint, build or VC_FP32_MODE, or a "
                                      "damaged file); this frame and every frame that references it are not the encoder's pictures")
            self.report["verified"] = True
        return frames


def load_lhbdc_models(seeded=None, weights=None, i_weights=None, i_qual=7, lmbda=1626, device=None):
    """(lhbdc.Model, mbt2018_mean(i_qual)) ready to code: checkpoints (``weights``: the reference's, a dict with the state dict under
    "state_dict", default ``pretrained_weights/compression_<lmbda>.pth``; ``i_weights``: a state dict of the CompressAI model), or
    with ``seeded`` the deterministic synthetic checkpoints of vcamd.seeding (encoder and decoder must use the same seed)."""
    import os

    from . import lhbdc
    from .iframe import mbt2018_mean
    from .seeding import seeded_state_dict
    device = device or torch.device("cuda")
    if not 1 <= int(i_qual) <= 8:
        raise hip.VcError(f"I-frame quality {i_qual!r}: 1..8")
    model, intra = lhbdc.Model(), mbt2018_mean(int(i_qual), "mse", pretrained=False)
    if seeded is not None:
        model.load_state_dict(seeded_state_dict(model.state_dict(), seed=int(seeded)))
        intra.load_state_dict(seeded_state_dict(intra.state_dict(), seed=int(seeded), conv_gain=0.8))
    else:
        path = weights or f"pretrained_weights/compression_{int(lmbda)}.pth"
        if not os.path.exists(path) or not i_weights:
            raise hip.VcError(f"the LHBDC checkpoint ({path}) and the mbt2018_mean weights are separate downloads: pass --weights PATH and "
                              "--i_weights PATH, or --seeded SEED for the synthetic checkpoints")
        sd = torch.load(path, map_location="cpu")
        model.load_state_dict(sd["state_dict"] if isinstance(sd, dict) and "state_dict" in sd else sd)
        sd = torch.load(i_weights, map_location="cpu")
        intra.load_state_dict(sd["state_dict"] if isinstance(sd, dict) and "state_dict" in sd else sd)
    model.mv_compressor.update(force=True)
    model.residual_compressor.update(force=True)
    intra.update(force=True)
    return model.to(device).float().eval(), intra.to(device).float().eval()
