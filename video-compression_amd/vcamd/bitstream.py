"""Real-bitstream GOP coding for LHBDC with the host range coder OFF the GPU's critical path.

The reference's CLI (LHBDC/encode_B.py:71-126, decode_B.py:63-104) codes one B-frame per process call and its test loop
(test/testing.py) only estimates rate, so nothing there overlaps entropy coding with the networks.  Here a GOP is coded
into / from the same ``bits_B.bin`` containers with

* ONE analysis pass per codec on the encoder (``MeanScaleHyperprior.code_t``): the reconstruction the next hierarchy level
  needs and the integers of the bitstream come out of the same launch sequence; the integers travel to pinned host memory on a
  side stream and are range-coded by worker threads (``vc_rans_*`` through ctypes releases the GIL) while the GPU is
  already coding the next level -- the encoder never waits for the coder;
* a decoder that enqueues the (tiny) hyper-synthesis of BOTH codecs first, so the scale-table indexes are on the host
  while the GPU estimates the predictor flows, decodes the y strings of all frames of the level in parallel threads, and
  only then enqueues the synthesis transforms;
* the frames of one hierarchy level batched through the same kernels, as in ``gop.code_gop_lhbdc``.

Wiring = the CLI's (both flow predictors equal pad(flow_ab): SURVEY.md Appendix B.1), so every container is decodable by
the reference's decode_B.py and vice versa.  The encoder-side reconstruction equals the decoder's output bit for bit
(same integers, same kernels) -- asserted in tests/test_stream_gpu.py.

``LhbdcStreamCodec(coder="device")`` (opt-in) keeps the entropy coding on the GPU instead: the same integers in
``VCLD`` containers of the project's own interleaved coder, one ``vc_irans_encode`` launch per compressor on the encoder and two fused
decode kernels per compressor on the decoder (``vc_irans_decode_eb`` / ``vc_irans_decode_gc``: no index tensor, no symbol tensor),
so a GOP decodes as uploads, then launches only, then one read of the error words.

Flex-Rate is not offered here on purpose: its compress() codes the UN-gained latent while forward() quantises the gained
one (quirk B.6), so the reference's own encoder and decoder disagree on the reconstruction whenever the gain differs from
one -- there is no closed loop to pipeline.

This module is the GPU pipeline only (streams, events, the thread pool, launch order); the bytes of ``bits_B.bin``, ``VCLD`` and the
other containers are written and read in containers.py.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import hip
# the byte formats live in containers.py; their names stay importable from here
from .containers import (ICIP2024_DEV_MAGIC, ICIP2024_DEV_TAIL, ICIP2024_DOWN_RATIOS, ICIP2024_HEADER, ICIP2024_INTRA_HEADER,  # noqa: F401
                         ICIP2024_INTRA_MAGIC, ICIP2024_INTRA_VERSION, ICIP2024_LENGTHS, ICIP2024_MAGIC, ICIP2024_VERSION, LHBDC_DEV_HEADER,
                         LHBDC_DEV_MAGIC, LHBDC_DEV_VERSION, SEQUENCE_FAMILY_ICIP2024, SEQUENCE_HEADER, SEQUENCE_MAGIC, SEQUENCE_RECORD,
                         SEQUENCE_TYPES, SEQUENCE_VERSION, finish_all, pack_bits_b, pack_icip2024_frame, pack_icip2024_frame_dev,
                         pack_icip2024_intra_dev, pack_lhbdc_frame_dev, pack_sequence, sequence_plan, unpack_icip2024_frame,
                         unpack_icip2024_frame_dev, unpack_icip2024_intra_dev, unpack_lhbdc_frame_dev, unpack_sequence)
from .gop import DECODING_INFO, LEVEL_GROUPS
from .lhbdc import Model, _cli_predictors, _count, _motion_difference, check_container_shapes, frame_list, read_container


class _Tables:
    """Host copies of a codec's range-coder tables (read once; the model must have been update()d)."""

    def __init__(self, codec):
        self.eb = codec.entropy_bottleneck.tables()
        self.gc = codec.gaussian_conditional.tables()
        self.channels = codec.N

    def z_index(self, hz, wz):
        return np.repeat(np.arange(self.channels, dtype=np.int32), hz * wz)


class PendingContainers:
    """Containers of one encoded level pass; ``result()`` blocks until the worker threads have written them."""

    def __init__(self, futures, keep_alive):
        self._futures, self._keep = futures, keep_alive

    def result(self):
        out = [f.result() for f in self._futures]
        self._keep = None
        return out


class LhbdcStreamCodec:
    """``coder="host"`` (default): bits_B.bin containers, the host range coder on worker threads, as described above.
    ``coder="device"``: VCLD containers (containers.py) coded and decoded by the interleaved range coder's kernels -- the same integers,
    the same reconstructions; ``waves`` sub-streams per payload on the encoder (the decoder takes the count from the container).
    The worker pool is not created: nothing is coded on the host."""
    CODERS = ("host", "device")

    def __init__(self, model: Model, lmbda=1626, workers=4, coder="host", waves=4):
        if coder not in self.CODERS or not hip.irans_waves_ok(waves):
            raise hip.VcError(f"coder {coder!r} / waves {waves!r}: one of {self.CODERS}, waves a power of two in 1..16")
        self.model, self.lmbda = model, int(lmbda)
        self.coder, self.waves = coder, int(waves)
        self.pool = ThreadPoolExecutor(max_workers=workers) if coder == "host" else None
        self.copy_stream = None
        self.t_mv = _Tables(model.mv_compressor)
        self.t_res = _Tables(model.residual_compressor)

    # -- plumbing: device int32 tensors -> pinned host memory on a side stream --------------------------------
    def _to_host_async(self, tensors):
        """Start the D2H copies behind everything enqueued so far; returns (pinned arrays, event to wait on)."""
        if self.copy_stream is None:
            self.copy_stream = torch.cuda.Stream()
        ready = torch.cuda.Event()
        ready.record()
        host = []
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(ready)
            for t in tensors:
                h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                h.copy_(t, non_blocking=True)
                t.record_stream(self.copy_stream)
                host.append(h)
            done = torch.cuda.Event()
            done.record()
        return host, done

    # -- encoder ------------------------------------------------------------------------------------------
    def _encode_level(self, x_before, x_current, x_after, hand_over):
        """The launches of one encoded level, whichever coder takes the integers: ``hand_over(codec, sym)`` is called right behind
        each compressor's code_t -- the motion integers leave before the NHWC conversion and the prediction are enqueued, the
        residual's before the final addition.  Returns (x_hat NCHW, n, (mv_sym, res_sym), what the two calls returned)."""
        m = self.model
        xb_, xc_, xa_ = (frame_list(t) for t in (x_before, x_current, x_after))      # tensors or lists of frames
        n, dev = _count(xc_), xc_[0].device
        diff, flow_ba, flow_ab, hh, ww = _motion_difference(m, {"b": xb_, "c": xc_, "a": xa_}, n, dev)
        mv_hat, mv_sym = m.mv_compressor.code_t(diff)
        handed_mv = hand_over(m.mv_compressor, mv_sym)
        xb, xc, xa = hip.nchw_frames_to_nhwc(xb_), hip.nchw_frames_to_nhwc(xc_), hip.nchw_frames_to_nhwc(xa_)
        pred, resid = m._predict(xb, xa, mv_hat, flow_ab, flow_ba, hh, ww, cur=xc)
        res_hat, res_sym = m.residual_compressor.code_t(resid)
        handed_res = hand_over(m.residual_compressor, res_sym)
        x_hat = hip.nhwc_to_nchw(hip.axpby(res_hat, pred))
        return x_hat, n, (mv_sym, res_sym), (handed_mv, handed_res)

    def encode_frames(self, x_before, x_current, x_after):
        """n independent B-frames (one hierarchy level).  Returns (x_hat NCHW = what decode_frames will output,
        PendingContainers).  No host synchronisation: the caller can enqueue the next level at once."""
        if self.coder == "device":
            return self._encode_frames_dev(x_before, x_current, x_after)
        x_hat, n, (mv_sym, res_sym), ((host_mv, ev_mv), (host_res, ev_res)) = self._encode_level(
            x_before, x_current, x_after, lambda codec, sym: self._to_host_async([sym["y_sym"], sym["y_idx"], sym["z_sym"]]))
        mv_shape, res_shape = mv_sym["shape"], res_sym["shape"]
        zi_mv, zi_res = self.t_mv.z_index(*mv_shape), self.t_res.z_index(*res_shape)

        def code_one(i):
            ev_mv.synchronize()
            y, idx, z = (h.numpy() for h in host_mv)
            mv_z = hip.rans_encode(z[i], zi_mv, *self.t_mv.eb)
            mv_y = hip.rans_encode(y[i], idx[i], *self.t_mv.gc)
            ev_res.synchronize()
            y, idx, z = (h.numpy() for h in host_res)
            res_z = hip.rans_encode(z[i], zi_res, *self.t_res.eb)
            res_y = hip.rans_encode(y[i], idx[i], *self.t_res.gc)
            return pack_bits_b(self.lmbda, mv_shape, res_shape, mv_y, mv_z, res_y, res_z)

        futures = [self.pool.submit(code_one, i) for i in range(n)]
        return x_hat, PendingContainers(futures, (mv_sym, res_sym, host_mv, host_res))

    # -- decoder ------------------------------------------------------------------------------------------
    def decode_frames(self, x_before, x_after, containers):
        """n independent B-frames from their containers (bytes).  Returns x_hat NCHW [n,3,H,W].  ``coder="device"``: upload,
        launches only, then the one read of the decoders' error words (VcError, after x_hat is enqueued); an
        :class:`UploadedLevel` in place of the containers skips the upload."""
        if self.coder == "device":
            level = containers if isinstance(containers, UploadedLevel) else self.upload_frames(containers, x_before)
            x_hat = self._decode_level_dev(x_before, x_after, level)
            level.finish()
            return x_hat
        _refuse_container_of_other_coder(containers, "host")
        m = self.model
        xb_, xa_ = frame_list(x_before), frame_list(x_after)
        n, dev = _count(xb_), xb_[0].device
        if len(containers) != n:
            raise hip.VcError("one container per frame")
        parsed = [read_container(c) for c in containers]
        mv_shape, res_shape = tuple(parsed[0][3]), tuple(parsed[0][4])
        if any(tuple(p[3]) != mv_shape or tuple(p[4]) != res_shape for p in parsed):
            raise hip.VcError("frames of one pass must have the same latent shapes")
        check_container_shapes(mv_shape, res_shape, xb_[0].shape[-2], xb_[0].shape[-1])   # before anything is allocated from them
        zi_mv, zi_res = self.t_mv.z_index(*mv_shape), self.t_res.z_index(*res_shape)
        # 1. hyper-latents: fixed tables, a few thousand symbols per frame -- decoded at once, in parallel
        fz = [self.pool.submit(lambda p=p: (hip.rans_decode(p[1][1][0], zi_mv, *self.t_mv.eb),
                                            hip.rans_decode(p[2][1][0], zi_res, *self.t_res.eb))) for p in parsed]
        zs = [f.result() for f in fz]
        z_mv = torch.from_numpy(np.stack([z[0] for z in zs])).to(dev)
        z_res = torch.from_numpy(np.stack([z[1] for z in zs])).to(dev)
        # 2. device: both hyper-syntheses FIRST (tiny), their indexes start travelling to the host ...
        means_mv, idx_mv = m.mv_compressor.hyper_decode_t(z_mv, n, mv_shape)
        means_res, idx_res = m.residual_compressor.hyper_decode_t(z_res, n, res_shape)
        (h_idx_mv, h_idx_res), ev_idx = self._to_host_async([idx_mv, idx_res])
        # 3. ... while the GPU estimates the predictor flows (the heavy part that needs no bitstream at all)
        flow_ba, flow_ab, hh, ww = _cli_predictors(m, {"b": xb_, "a": xa_}, n)
        xb, xa = hip.nchw_frames_to_nhwc(xb_), hip.nchw_frames_to_nhwc(xa_)
        # 4. host: every y string of the level in its own worker, in parallel with (3)
        ev_idx.synchronize()
        i_mv, i_res = h_idx_mv.numpy(), h_idx_res.numpy()
        f_mv = [self.pool.submit(hip.rans_decode, parsed[i][1][0][0], i_mv[i], *self.t_mv.gc) for i in range(n)]
        f_res = [self.pool.submit(hip.rans_decode, parsed[i][2][0][0], i_res[i], *self.t_res.gc) for i in range(n)]
        y_mv = torch.from_numpy(np.stack([f.result() for f in f_mv])).to(dev)
        mv_hat = m.mv_compressor.synth_decode_t(y_mv, means_mv)
        pred, _ = m._predict(xb, xa, mv_hat, flow_ab, flow_ba, hh, ww)
        y_res = torch.from_numpy(np.stack([f.result() for f in f_res])).to(dev)
        res_hat = m.residual_compressor.synth_decode_t(y_res, means_res)
        return hip.nhwc_to_nchw(hip.axpby(res_hat, pred))

    # -- coder="device": the interleaved range coder's kernels on both sides -----------------
    def _encode_frames_dev(self, x_before, x_current, x_after):
        """encode_frames with the integers coded where they lie: per compressor one vc_irans_encode launch over two segments (z with
        the factorised tables, y with the Gaussian ones) on the tensors of code_t.  Nothing is read back here: the one host
        synchronisation of the level, the read of both compressors' word counts, happens in ``PendingDevContainers.result()``."""
        x_hat, _, (mv_sym, res_sym), jobs = self._encode_level(x_before, x_current, x_after, self._encode_job)
        return x_hat, PendingDevContainers(list(jobs), self.lmbda, mv_sym["shape"], res_sym["shape"], self.waves, (mv_sym, res_sym))

    def _encode_job(self, codec, sym):
        n, dev = sym["z_sym"].shape[0], sym["z_sym"].device
        segments = [(sym["z_sym"], codec.z_index_dev(n, sym["shape"], dev), 0), (sym["y_sym"], sym["y_idx"], 1)]
        return hip.irans_encode_launch(segments, [codec.entropy_bottleneck.irans_tables(), codec.gaussian_conditional.irans_tables()], self.waves)

    def upload_frames(self, containers, like):
        """The containers of n frames of one level on their way to the device: parsed and validated (VcError before anything is
        allocated or launched), one hip.IransDecoder per compressor.  ``like``: a frame (or frames) of the sequence, for its size
        and device."""
        if self.coder != "device":
            raise hip.VcError('upload_frames belongs to coder="device"')
        like = frame_list(like)
        h, w, dev = like[0].shape[-2], like[0].shape[-1], like[0].device
        _refuse_container_of_other_coder(containers, "device")
        parsed = [unpack_lhbdc_frame_dev(c, h, w) for c in containers]
        if not parsed:
            raise hip.VcError("one container per frame")
        first = parsed[0]
        if any((p["mv_shape"], p["res_shape"], p["waves"]) != (first["mv_shape"], first["res_shape"], first["waves"]) for p in parsed):
            raise hip.VcError("frames of one pass must have the same latent shapes and wave count")
        return UploadedLevel(hip.IransDecoder([p["mv"] for p in parsed], first["waves"], dev),
                             hip.IransDecoder([p["res"] for p in parsed], first["waves"], dev), first["mv_shape"], first["res_shape"])

    def upload_gop(self, containers, like):
        """Every payload of a GOP ({order: container}) uploaded, level by level: what :meth:`decode_gop` then only launches on."""
        return UploadedGop([self.upload_frames([containers[o] for o in group], like) for group in LEVEL_GROUPS])

    def _decode_level_dev(self, x_before, x_after, level):
        """Launches only: per compressor vc_irans_decode_eb -> hyper-synthesis -> vc_irans_decode_gc -> synthesis."""
        m = self.model
        xb_, xa_ = frame_list(x_before), frame_list(x_after)
        n = _count(xb_)
        if level.mv.images != n or level.res.images != n:
            raise hip.VcError("one container per frame")
        check_container_shapes(level.mv_shape, level.res_shape, xb_[0].shape[-2], xb_[0].shape[-1])
        scales_mv, means_mv = m.mv_compressor.hyper_decode_dev_t(level.mv, level.mv_shape)
        scales_res, means_res = m.residual_compressor.hyper_decode_dev_t(level.res, level.res_shape)
        flow_ba, flow_ab, hh, ww = _cli_predictors(m, {"b": xb_, "a": xa_}, n)
        xb, xa = hip.nchw_frames_to_nhwc(xb_), hip.nchw_frames_to_nhwc(xa_)
        mv_hat = m.mv_compressor.synth_decode_dev_t(level.mv, scales_mv, means_mv)
        pred, _ = m._predict(xb, xa, mv_hat, flow_ab, flow_ba, hh, ww)
        res_hat = m.residual_compressor.synth_decode_dev_t(level.res, scales_res, means_res)
        return hip.nhwc_to_nchw(hip.axpby(res_hat, pred))

    # -- GOP-8 in hierarchical order ------------------------------------------------------------------------
    def encode_gop(self, gop, dec_first, dec_last):
        """``gop``: 9 padded NCHW frames.  Returns ({order: container bytes}, {order: reconstruction}).  The host coding of
        level l runs while the GPU codes level l+1; the only synchronisation is the final collection."""
        pending = []

        def level(k, group, xb, xa):
            x_hat, pend = self.encode_frames(xb, [gop[o] for o in group], xa)
            pending.append(pend)
            return x_hat

        decoded = _walk_gop(dec_first, dec_last, level)
        containers = {o: c for group, pend in zip(LEVEL_GROUPS, pending) for o, c in zip(group, pend.result())}
        return containers, decoded

    def decode_gop(self, containers, dec_first, dec_last, finish=True):
        """``coder="device"``: every payload of the GOP is uploaded first (:meth:`upload_gop`; an :class:`UploadedGop` in place of
        the containers skips that), the whole GOP is then enqueued as launches only, and ``finish`` reads every decoder's error
        words once, after the last reconstruction has been enqueued: a corrupt container raises VcError THERE (the frames
        behind the violation are decoded from zeros), never a fault.  ``finish=False`` leaves that read to the caller
        (``UploadedGop.finish``)."""
        if self.coder == "device":
            up = containers if isinstance(containers, UploadedGop) else self.upload_gop(containers, dec_first)
            decoded = _walk_gop(dec_first, dec_last, lambda k, group, xb, xa: self._decode_level_dev(xb, xa, up.levels[k]))
            if finish:
                up.finish()
            return decoded
        return _walk_gop(dec_first, dec_last, lambda k, group, xb, xa: self.decode_frames(xb, xa, [containers[o] for o in group]))

    def close(self):
        if self.pool is not None:
            self.pool.shutdown(wait=True)


def _walk_gop(dec_first, dec_last, code_level):
    """The hierarchy of a GOP-8, level by level: ``code_level(k, group, xb, xa)`` gets the display orders of level k and the decoded
    reference frames in front of and behind each of them and returns their reconstructions [len(group), 3, H, W], which the levels
    below then reference.  Returns {order: reconstruction}, the two boundary frames included."""
    decoded = {0: dec_first, 8: dec_last}
    for k, group in enumerate(LEVEL_GROUPS):
        xb = [decoded[DECODING_INFO[o][0]] for o in group]
        xa = [decoded[DECODING_INFO[o][1]] for o in group]
        x_hat = code_level(k, group, xb, xa)
        for i, o in enumerate(group):
            decoded[o] = x_hat[i:i + 1]
    return decoded


_FORMATS = {"host": "bits_B.bin", "device": "VCLD"}


def _refuse_container_of_other_coder(containers, coder):
    """A VCLD container handed to the host-coded path (or a bits_B.bin one to the device-coded path) would be parsed as the other
    format's header: refuse it by name.  (The first field of bits_B.bin is lambda: "VCLD" there would be 1 145 848 662.)"""
    if isinstance(containers, (UploadedLevel, UploadedGop)):
        raise hip.VcError(f'uploaded {_FORMATS["device"]} payloads belong to coder="device", this codec reads {_FORMATS[coder]}')
    for c in containers:
        is_dev = bytes(c[:4]) == LHBDC_DEV_MAGIC
        if is_dev != (coder == "device"):
            other = "host" if coder == "device" else "device"
            raise hip.VcError(f'this codec was built with coder="{coder}" and reads {_FORMATS[coder]} containers; this one '
                              f'{"is" if is_dev else "is not"} a {_FORMATS["device"]} container (magic {bytes(c[:4])!r}): decode '
                              f'{_FORMATS[other]} with coder="{other}"')


class PendingDevContainers:
    """Containers of one level coded on the device; ``result()`` does the level's one host synchronisation (the read of both
    compressors' word counts), copies the used tails and packs the VCLD containers."""

    def __init__(self, jobs, lmbda, mv_shape, res_shape, waves, keep_alive):
        self._jobs, self._head, self._keep = jobs, (lmbda, mv_shape, res_shape, waves), keep_alive

    def result(self):
        mv, res = hip.irans_encode_collect(self._jobs)
        self._keep = None
        return [pack_lhbdc_frame_dev(*self._head, a, b) for a, b in zip(mv, res)]


class UploadedLevel:
    """The payloads of one level on the device: one hip.IransDecoder per compressor (one payload per frame each)."""

    def __init__(self, mv, res, mv_shape, res_shape):
        self.mv, self.res, self.mv_shape, self.res_shape = mv, res, tuple(mv_shape), tuple(res_shape)

    def finish(self):
        """the one read per decoder: VcError when a payload was corrupt (every decoder is read before the first error is raised)"""
        finish_all((self.mv, self.res))


class UploadedGop:
    def __init__(self, levels):
        self.levels = levels

    def finish(self):
        finish_all(self.levels)
