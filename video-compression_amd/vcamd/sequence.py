"""The ICIP2024 models as an end-to-end codec: a sequence of frames in, ONE byte string out (the ``VCSQ`` file of vcamd.containers;
layout in INTEGRATION.md), and the frames back from that string and the two models alone.

The loop is the reference's ``val_sequence_level`` as gop.code_sequence_icip2024 walks it -- coding order and frame types from
icip2024.get_order_typ_list, references = the two decoded frames (clamped to [0, 1], at most 32 kept) closest in display order
(select_references / update_buffer), scales from get_scales -- with real bits in place of the -log2 p sums: I-frames through
``ELIC.compress(coder="device")`` (``VCII`` records), B-frames through ``FlowGuidedB.compress(down_ratio=None, coder="device")``, the
device search (``VCID`` records).  The decoder derives order, types, references and scales exactly as the encoder does; per frame it
uploads the payloads once and enqueues launches only, and it reads the decoders' error words after the last frame is enqueued."""
import torch

from . import containers, hip, icip2024

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
