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
"""
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import hip
from .gop import DECODING_INFO, LEVEL_GROUPS
from .hip import T
from .lhbdc import Model, _cli_predictors, _count, check_container_shapes, frame_list, read_container


def _pack_container(lmbda, mv_shape, res_shape, mv_y, mv_z, res_y, res_z):
    """bits_B.bin (encode_B.py:114-126); see lhbdc.write_container."""
    head = (np.array(lmbda, dtype=np.uint32).tobytes() + np.array(tuple(mv_shape), dtype=np.uint16).tobytes() +
            np.array(len(mv_y), dtype=np.uint32).tobytes() + np.array(len(mv_z), dtype=np.uint32).tobytes() +
            np.array(tuple(res_shape), dtype=np.uint16).tobytes() + np.array(len(res_y), dtype=np.uint32).tobytes())
    return head + mv_y + mv_z + res_y + res_z


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
    ``coder="device"``: VCLD containers (below) coded and decoded by the interleaved range coder's kernels -- the same integers,
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
    def encode_frames(self, x_before, x_current, x_after):
        """n independent B-frames (one hierarchy level).  Returns (x_hat NCHW = what decode_frames will output,
        PendingContainers).  No host synchronisation: the caller can enqueue the next level at once."""
        if self.coder == "device":
            return self._encode_frames_dev(x_before, x_current, x_after)
        m = self.model
        xb_, xc_, xa_ = (frame_list(t) for t in (x_before, x_current, x_after))      # tensors or lists of frames
        n, dev = _count(xc_), xc_[0].device
        frames = {"b": xb_, "c": xc_, "a": xa_}
        flow_ba, flow_ab, hh, ww = _cli_predictors(m, frames, n)
        cur = m._flows(frames, [("c", "b"), ("c", "a")])
        cur_flows, _, _ = Model._pool_pad(cur, 1.0)
        diff = T.empty(n, flow_ab.h, flow_ab.w, 4, dev)
        hip.axpby(cur_flows.images(0, n), flow_ab, 1.0, -1.0, out=diff.channels(0, 2))
        hip.axpby(cur_flows.images(n, 2 * n), flow_ba, 1.0, -1.0, out=diff.channels(2, 4))
        mv_hat, mv_sym = m.mv_compressor.code_t(diff)
        host_mv, ev_mv = self._to_host_async([mv_sym["y_sym"], mv_sym["y_idx"], mv_sym["z_sym"]])
        xb, xc, xa = hip.nchw_frames_to_nhwc(xb_), hip.nchw_frames_to_nhwc(xc_), hip.nchw_frames_to_nhwc(xa_)
        pred, resid = m._predict(xb, xa, mv_hat, flow_ab, flow_ba, hh, ww, cur=xc)
        res_hat, res_sym = m.residual_compressor.code_t(resid)
        host_res, ev_res = self._to_host_async([res_sym["y_sym"], res_sym["y_idx"], res_sym["z_sym"]])
        x_hat = hip.nhwc_to_nchw(hip.axpby(res_hat, pred))
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
            return _pack_container(self.lmbda, mv_shape, res_shape, mv_y, mv_z, res_y, res_z)

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
        m = self.model
        xb_, xc_, xa_ = (frame_list(t) for t in (x_before, x_current, x_after))
        n, dev = _count(xc_), xc_[0].device
        frames = {"b": xb_, "c": xc_, "a": xa_}
        flow_ba, flow_ab, hh, ww = _cli_predictors(m, frames, n)
        cur = m._flows(frames, [("c", "b"), ("c", "a")])
        cur_flows, _, _ = Model._pool_pad(cur, 1.0)
        diff = T.empty(n, flow_ab.h, flow_ab.w, 4, dev)
        hip.axpby(cur_flows.images(0, n), flow_ab, 1.0, -1.0, out=diff.channels(0, 2))
        hip.axpby(cur_flows.images(n, 2 * n), flow_ba, 1.0, -1.0, out=diff.channels(2, 4))
        mv_hat, mv_sym = m.mv_compressor.code_t(diff)
        job_mv = self._encode_job(m.mv_compressor, mv_sym, n, dev)
        xb, xc, xa = hip.nchw_frames_to_nhwc(xb_), hip.nchw_frames_to_nhwc(xc_), hip.nchw_frames_to_nhwc(xa_)
        pred, resid = m._predict(xb, xa, mv_hat, flow_ab, flow_ba, hh, ww, cur=xc)
        res_hat, res_sym = m.residual_compressor.code_t(resid)
        job_res = self._encode_job(m.residual_compressor, res_sym, n, dev)
        x_hat = hip.nhwc_to_nchw(hip.axpby(res_hat, pred))
        return x_hat, PendingDevContainers([job_mv, job_res], self.lmbda, mv_sym["shape"], res_sym["shape"], self.waves, (mv_sym, res_sym))

    def _encode_job(self, codec, sym, n, dev):
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
        decoded, pending = {0: dec_first, 8: dec_last}, []
        for group in LEVEL_GROUPS:
            xb = [decoded[DECODING_INFO[o][0]] for o in group]
            xc = [gop[o] for o in group]
            xa = [decoded[DECODING_INFO[o][1]] for o in group]
            x_hat, pend = self.encode_frames(xb, xc, xa)
            for i, o in enumerate(group):
                decoded[o] = x_hat[i:i + 1]
            pending.append((group, pend))
        containers = {}
        for group, pend in pending:
            for o, c in zip(group, pend.result()):
                containers[o] = c
        return containers, decoded

    def decode_gop(self, containers, dec_first, dec_last, finish=True):
        """``coder="device"``: every payload of the GOP is uploaded first (:meth:`upload_gop`; an :class:`UploadedGop` in place of
        the containers skips that), the whole GOP is then enqueued as launches only, and ``finish`` reads every decoder's error
        words once, after the last reconstruction has been enqueued: a corrupt container raises VcError THERE (the frames
        behind the violation are decoded from zeros), never a fault.  ``finish=False`` leaves that read to the caller
        (``UploadedGop.finish``)."""
        if self.coder == "device":
            up = containers if isinstance(containers, UploadedGop) else self.upload_gop(containers, dec_first)
            decoded = {0: dec_first, 8: dec_last}
            for group, level in zip(LEVEL_GROUPS, up.levels):
                xb = [decoded[DECODING_INFO[o][0]] for o in group]
                xa = [decoded[DECODING_INFO[o][1]] for o in group]
                x_hat = self._decode_level_dev(xb, xa, level)
                for i, o in enumerate(group):
                    decoded[o] = x_hat[i:i + 1]
            if finish:
                up.finish()
            return decoded
        decoded = {0: dec_first, 8: dec_last}
        for group in LEVEL_GROUPS:
            xb = [decoded[DECODING_INFO[o][0]] for o in group]
            xa = [decoded[DECODING_INFO[o][1]] for o in group]
            x_hat = self.decode_frames(xb, xa, [containers[o] for o in group])
            for i, o in enumerate(group):
                decoded[o] = x_hat[i:i + 1]
        return decoded

    def close(self):
        if self.pool is not None:
            self.pool.shutdown(wait=True)


# ------------------------------------------------------------------------------------------------
# Device-coded LHBDC B-frame container (this project's own format; bits_B.bin stays the default and the reference's)
# ------------------------------------------------------------------------------------------------
# One byte string per coded frame, little-endian:
#   offset  0  4 bytes  magic "VCLD"
#           4  u8       version (1)
#           5  u8       waves W (1, 2, 4, 8 or 16): sub-streams per payload
#           6  u32      lambda (as bits_B.bin)
#          10  u16 x 2  hyper-latent shape (h, w) of the motion compressor
#          14  u16 x 2  hyper-latent shape (h, w) of the residual compressor
#          18  u32 x 2  payload lengths: motion, residual
#          26  the two payloads in that order
# A payload is one interleaved-rANS payload (include/vc_hip.h: "Interleaved range coder") of two segments, states and cursors
# continuing from the first to the second: the hyper-latent z (table set 0 = the factorised tables, index of symbol i =
# i / (hz * wz), its channel), then the latent y (table set 1 = the Gaussian tables, index from the scales); symbol order = the int32
# tensors of MeanScaleHyperprior.code_t (NCHW raster).
LHBDC_DEV_MAGIC = b"VCLD"
LHBDC_DEV_VERSION = 1
LHBDC_DEV_HEADER = struct.Struct("<4sBBIHHHHII")
_FORMATS = {"host": "bits_B.bin", "device": "VCLD"}


def pack_lhbdc_frame_dev(lmbda, mv_shape, res_shape, waves, mv_payload, res_payload):
    """The VCLD container of one frame from the two payloads of ``LhbdcStreamCodec(coder="device")``."""
    shapes = tuple(int(v) for v in tuple(mv_shape) + tuple(res_shape))
    if len(shapes) != 4 or not all(1 <= v <= 0xffff for v in shapes) or not hip.irans_waves_ok(waves) or not 0 <= int(lmbda) <= 0xffffffff:
        raise hip.VcError(f"lambda {lmbda} / hyper-latent shapes {shapes} / waves {waves} do not fit the container")
    mv_payload, res_payload = bytes(mv_payload), bytes(res_payload)
    if max(len(mv_payload), len(res_payload)) > 0xffffffff:
        raise hip.VcError("a payload is longer than the container's 32-bit length field")
    return LHBDC_DEV_HEADER.pack(LHBDC_DEV_MAGIC, LHBDC_DEV_VERSION, int(waves), int(lmbda), *shapes, len(mv_payload),
                                 len(res_payload)) + mv_payload + res_payload


def unpack_lhbdc_frame_dev(data, h, w):
    """Inverse of :func:`pack_lhbdc_frame_dev` for a (padded) h x w frame: ``{"lmbda", "waves", "mv_shape", "res_shape", "mv", "res"}``.
    Magic, version, wave count, the lengths against the data (no trailing bytes, whole words, at least the W sub-stream headers)
    and the shapes against the frame size (lhbdc.check_container_shapes) are validated before anything is returned, so before
    anything is allocated from the header (VcError)."""
    data = bytes(data)
    if len(data) < LHBDC_DEV_HEADER.size:
        raise hip.VcError(f"VCLD container: {len(data)} bytes is shorter than the {LHBDC_DEV_HEADER.size}-byte header")
    magic, version, waves, lmbda, mh, mw, rh, rw, n_mv, n_res = LHBDC_DEV_HEADER.unpack_from(data, 0)
    if magic != LHBDC_DEV_MAGIC:
        raise hip.VcError(f"VCLD container: magic {magic!r} is not {LHBDC_DEV_MAGIC!r}")
    if version != LHBDC_DEV_VERSION:
        raise hip.VcError(f"VCLD container: version {version} (this reader knows {LHBDC_DEV_VERSION})")
    if not hip.irans_waves_ok(waves):
        raise hip.VcError(f"VCLD container: waves {waves} is not a power of two in 1..16")
    fixed = LHBDC_DEV_HEADER.size
    if fixed + n_mv + n_res != len(data) or min(n_mv, n_res) < waves * hip.IRANS_SUBSTREAM_HEADER or n_mv % 4 or n_res % 4:
        raise hip.VcError(f"VCLD container: payload lengths {n_mv} + {n_res} do not fit {len(data)} bytes / {waves} waves")
    check_container_shapes((mh, mw), (rh, rw), h, w)
    return {"lmbda": lmbda, "waves": waves, "mv_shape": (mh, mw), "res_shape": (rh, rw), "mv": data[fixed:fixed + n_mv],
            "res": data[fixed + n_mv:]}


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
        errors = []
        for d in (self.mv, self.res):
            try:
                d.finish()
            except hip.VcError as e:
                errors.append(e)
        if errors:
            raise errors[0]


class UploadedGop:
    def __init__(self, levels):
        self.levels = levels

    def finish(self):
        errors = []
        for level in self.levels:
            try:
                level.finish()
            except hip.VcError as e:
                errors.append(e)
        if errors:
            raise errors[0]


# ------------------------------------------------------------------------------------------------
# ICIP2024 B-frame container (this project's own format: the reference has no bitstream for FlowGuidedB)
# ------------------------------------------------------------------------------------------------
# One byte string per coded frame, little-endian:
#   offset  0  4 bytes  magic "VCIB"
#           4  u8       version (1)
#           5  u8       down_ratio (1, 2, 4, 8 or 16)
#           6  u16 x 2  hyper-latent shape (h, w) = frame / 64
#          10  f32 x 3  s (quality level), scale1, scale2 (both after FlowGuidedB.convert_scales)
#          22  u32 x 12 string lengths: offset z, offset g0..g4, residual z, residual g0..g4
#          70  the twelve payloads in that order
ICIP2024_MAGIC = b"VCIB"
ICIP2024_VERSION = 1
ICIP2024_HEADER = struct.Struct("<4sBBHHfff")
ICIP2024_LENGTHS = struct.Struct("<12I")
ICIP2024_DOWN_RATIOS = (1, 2, 4, 8, 16)


def _icip2024_payloads(strings, image):
    out = []
    for codec in ("offset", "residual"):
        groups, z = strings[codec]
        if len(groups) != 5:
            raise hip.VcError(f"{codec}: five group strings per image, got {len(groups)}")
        out.append(z[image])
        out.extend(g[image] for g in groups)
    return [bytes(b) for b in out]


def pack_icip2024_frame(strings, shape, down_ratio, s, scale1, scale2, image=0):
    """The container of image ``image`` of a FlowGuidedB.compress result: ``strings`` / ``shape`` / ``down_ratio`` as it returns
    them, ``s`` the quality level and ``scale1`` / ``scale2`` the converted scales (FlowGuidedB.convert_scales) it was called
    with.  The three numbers are stored as fp32 -- compress() and decompress() round the level to fp32 themselves and the
    converted scales are fp32 values, so a decoder fed from the container uses the encoder's numbers."""
    hz, wz = int(shape[0]), int(shape[1])
    if int(down_ratio) not in ICIP2024_DOWN_RATIOS or not (1 <= hz <= 0xffff and 1 <= wz <= 0xffff):
        raise hip.VcError(f"down_ratio {down_ratio} / hyper-latent shape {hz}x{wz} do not fit the container")
    payloads = _icip2024_payloads(strings, image)
    if any(len(p) > 0xffffffff for p in payloads):
        raise hip.VcError("a string is longer than the container's 32-bit length field")
    head = ICIP2024_HEADER.pack(ICIP2024_MAGIC, ICIP2024_VERSION, int(down_ratio), hz, wz, float(s), float(scale1), float(scale2))
    return head + ICIP2024_LENGTHS.pack(*(len(p) for p in payloads)) + b"".join(payloads)


def unpack_icip2024_frame(data):
    """Inverse of :func:`pack_icip2024_frame`: ``{"strings" (one image per list), "shape", "down_ratio", "s", "scale1", "scale2"}``.
    Magic, version, field ranges and the total length are validated before anything is returned (VcError)."""
    data = bytes(data)
    fixed = ICIP2024_HEADER.size + ICIP2024_LENGTHS.size
    if len(data) < fixed:
        raise hip.VcError(f"ICIP2024 container: {len(data)} bytes is shorter than the {fixed}-byte header")
    magic, version, down_ratio, hz, wz, s, scale1, scale2 = ICIP2024_HEADER.unpack_from(data, 0)
    if magic != ICIP2024_MAGIC:
        raise hip.VcError(f"ICIP2024 container: magic {magic!r} is not {ICIP2024_MAGIC!r}")
    if version != ICIP2024_VERSION:
        raise hip.VcError(f"ICIP2024 container: version {version} (this reader knows {ICIP2024_VERSION})")
    if down_ratio not in ICIP2024_DOWN_RATIOS or hz < 1 or wz < 1:
        raise hip.VcError(f"ICIP2024 container: down_ratio {down_ratio} / hyper-latent shape {hz}x{wz} out of range")
    if not all(np.isfinite(v) for v in (s, scale1, scale2)):
        raise hip.VcError("ICIP2024 container: a header number is not finite")
    lengths = ICIP2024_LENGTHS.unpack_from(data, ICIP2024_HEADER.size)
    if fixed + sum(lengths) != len(data):
        raise hip.VcError(f"ICIP2024 container: the length table asks for {fixed + sum(lengths)} bytes, the buffer has {len(data)}")
    parts, pos = [], fixed
    for n in lengths:
        parts.append(data[pos:pos + n])
        pos += n
    strings = {"offset": [[[p] for p in parts[1:6]], [parts[0]]], "residual": [[[p] for p in parts[7:12]], [parts[6]]]}
    return {"strings": strings, "shape": (hz, wz), "down_ratio": down_ratio, "s": s, "scale1": scale1, "scale2": scale2}


# Container of the device-coded frames (FlowGuidedB.compress(coder="device"); payload format: DESIGN.md section 4d).  Its own
# magic: a VCIB reader refuses it and this reader refuses VCIB.  Little-endian:
#   offset  0  the 22 header bytes of VCIB with magic "VCID": version (1), down_ratio, hyper-latent shape, s, scale1, scale2
#          22  u8       waves W (1, 2, 4, 8 or 16): sub-streams per payload
#          23  u32 x 2  payload lengths: offset, residual
#          31  the two payloads in that order
ICIP2024_DEV_MAGIC = b"VCID"
ICIP2024_DEV_TAIL = struct.Struct("<BII")


def pack_icip2024_frame_dev(strings, shape, down_ratio, s, scale1, scale2, waves, image=0):
    """The container of image ``image`` of a ``FlowGuidedB.compress(coder="device")`` result (``waves`` as it returns it)."""
    hz, wz = int(shape[0]), int(shape[1])
    if int(down_ratio) not in ICIP2024_DOWN_RATIOS or not (1 <= hz <= 0xffff and 1 <= wz <= 0xffff) or not hip.irans_waves_ok(waves):
        raise hip.VcError(f"down_ratio {down_ratio} / hyper-latent shape {hz}x{wz} / waves {waves} do not fit the container")
    if not isinstance(strings, dict) or set(strings) != {"offset", "residual"}:
        raise hip.VcError('strings: {"offset": [payload per image], "residual": [payload per image]}')
    payloads = [bytes(strings[c][image]) for c in ("offset", "residual")]
    if any(len(p) > 0xffffffff for p in payloads):
        raise hip.VcError("a payload is longer than the container's 32-bit length field")
    head = ICIP2024_HEADER.pack(ICIP2024_DEV_MAGIC, ICIP2024_VERSION, int(down_ratio), hz, wz, float(s), float(scale1), float(scale2))
    return head + ICIP2024_DEV_TAIL.pack(int(waves), *(len(p) for p in payloads)) + b"".join(payloads)


def unpack_icip2024_frame_dev(data):
    """Inverse of :func:`pack_icip2024_frame_dev`: ``{"strings" (one image per list), "waves", "shape", "down_ratio", "s", "scale1",
    "scale2"}``; magic, version, field ranges, the wave count, the smallest possible payload and the total length are validated
    before anything is returned (VcError)."""
    data = bytes(data)
    fixed = ICIP2024_HEADER.size + ICIP2024_DEV_TAIL.size
    if len(data) < fixed:
        raise hip.VcError(f"ICIP2024 device-coded container: {len(data)} bytes is shorter than the {fixed}-byte header")
    magic, version, down_ratio, hz, wz, s, scale1, scale2 = ICIP2024_HEADER.unpack_from(data, 0)
    if magic != ICIP2024_DEV_MAGIC:
        raise hip.VcError(f"ICIP2024 device-coded container: magic {magic!r} is not {ICIP2024_DEV_MAGIC!r}")
    if version != ICIP2024_VERSION:
        raise hip.VcError(f"ICIP2024 device-coded container: version {version} (this reader knows {ICIP2024_VERSION})")
    if down_ratio not in ICIP2024_DOWN_RATIOS or hz < 1 or wz < 1:
        raise hip.VcError(f"ICIP2024 device-coded container: down_ratio {down_ratio} / hyper-latent shape {hz}x{wz} out of range")
    if not all(np.isfinite(v) for v in (s, scale1, scale2)):
        raise hip.VcError("ICIP2024 device-coded container: a header number is not finite")
    waves, n_off, n_res = ICIP2024_DEV_TAIL.unpack_from(data, ICIP2024_HEADER.size)
    if not hip.irans_waves_ok(waves):
        raise hip.VcError(f"ICIP2024 device-coded container: waves {waves} is not a power of two in 1..16")
    if fixed + n_off + n_res != len(data) or min(n_off, n_res) < waves * hip.IRANS_SUBSTREAM_HEADER or n_off % 4 or n_res % 4:
        raise hip.VcError(f"ICIP2024 device-coded container: payload lengths {n_off} + {n_res} do not fit {len(data)} bytes / {waves} waves")
    strings = {"offset": [data[fixed:fixed + n_off]], "residual": [data[fixed + n_off:]]}
    return {"strings": strings, "waves": waves, "shape": (hz, wz), "down_ratio": down_ratio, "s": s, "scale1": scale1, "scale2": scale2}


# ------------------------------------------------------------------------------------------------
# ICIP2024 sequence file: device-coded ELIC I-frames (VCII) and B-frames (VCID) in coding order (VCSQ).  Layout: INTEGRATION.md
# ------------------------------------------------------------------------------------------------
# I-frame container, little-endian:
#   offset  0  4 bytes  magic "VCII"
#           4  u8       version (1)
#           5  u8       waves W (1, 2, 4, 8 or 16)
#           6  u16 x 2  hyper-latent shape (h, w) = frame / 64
#          10  u32      payload length
#          14  the payload of ELIC.compress(coder="device") for one image
ICIP2024_INTRA_MAGIC = b"VCII"
ICIP2024_INTRA_VERSION = 1
ICIP2024_INTRA_HEADER = struct.Struct("<4sBBHHI")


def pack_icip2024_intra_dev(payload, shape, waves):
    """The container of one image of an ``ELIC.compress(coder="device")`` result: its payload, "shape" and "waves"."""
    hz, wz = int(shape[0]), int(shape[1])
    payload = bytes(payload)
    if not (1 <= hz <= 0xffff and 1 <= wz <= 0xffff) or not hip.irans_waves_ok(waves):
        raise hip.VcError(f"hyper-latent shape {hz}x{wz} / waves {waves} do not fit the container")
    if len(payload) > 0xffffffff or len(payload) % 4 or len(payload) < int(waves) * hip.IRANS_SUBSTREAM_HEADER:
        raise hip.VcError(f"a payload of {len(payload)} bytes is not one of the interleaved coder with {waves} waves")
    return ICIP2024_INTRA_HEADER.pack(ICIP2024_INTRA_MAGIC, ICIP2024_INTRA_VERSION, int(waves), hz, wz, len(payload)) + payload


def unpack_icip2024_intra_dev(data):
    """Inverse of :func:`pack_icip2024_intra_dev`: ``{"payload", "waves", "shape"}``; magic, version, the wave count, the smallest
    possible payload and the total length are validated before anything is returned (VcError)."""
    data = bytes(data)
    fixed = ICIP2024_INTRA_HEADER.size
    if len(data) < fixed:
        raise hip.VcError(f"ICIP2024 I-frame container: {len(data)} bytes is shorter than the {fixed}-byte header")
    magic, version, waves, hz, wz, length = ICIP2024_INTRA_HEADER.unpack_from(data, 0)
    if magic != ICIP2024_INTRA_MAGIC:
        raise hip.VcError(f"ICIP2024 I-frame container: magic {magic!r} is not {ICIP2024_INTRA_MAGIC!r}")
    if version != ICIP2024_INTRA_VERSION:
        raise hip.VcError(f"ICIP2024 I-frame container: version {version} (this reader knows {ICIP2024_INTRA_VERSION})")
    if not hip.irans_waves_ok(waves):
        raise hip.VcError(f"ICIP2024 I-frame container: waves {waves} is not a power of two in 1..16")
    if hz < 1 or wz < 1:
        raise hip.VcError(f"ICIP2024 I-frame container: hyper-latent shape {hz}x{wz} out of range")
    if fixed + length != len(data) or length % 4 or length < waves * hip.IRANS_SUBSTREAM_HEADER:
        raise hip.VcError(f"ICIP2024 I-frame container: payload length {length} does not fit {len(data)} bytes / {waves} waves")
    return {"payload": data[fixed:], "waves": waves, "shape": (hz, wz)}


# Sequence file, little-endian:
#   offset  0  4 bytes  magic "VCSQ"
#           4  u8       version (1)
#           5  u8       model family (1 = ICIP2024; every other value is refused)
#           6  u16 x 2  picture width, height (unpadded)
#          10  u32      frame count
#          14  u16      intra_size
#          16  f32      quality level s
#          20  u8       intra quality index
#          21  one record per frame in CODING order:  u8 type (0 = I, 1 = B) | u32 display order | u32 length | VCII / VCID bytes
SEQUENCE_MAGIC = b"VCSQ"
SEQUENCE_VERSION = 1
SEQUENCE_FAMILY_ICIP2024 = 1
SEQUENCE_HEADER = struct.Struct("<4sBBHHIHfB")
SEQUENCE_RECORD = struct.Struct("<BII")
SEQUENCE_TYPES = ("I", "B")


def sequence_plan(intra_size, n_frames):
    """[(display order, "I" | "B")] in coding order, as the encoder's loop walks it (icip2024.get_order_typ_list).  VcError where
    that function gives no coding order for the pair: every frame exactly once, the first one an I-frame."""
    from . import icip2024
    intra_size, n_frames = int(intra_size), int(n_frames)
    if intra_size < 1 or n_frames < 1:
        raise hip.VcError(f"intra_size {intra_size} / {n_frames} frames: both at least 1")
    if n_frames == 1:
        return [(0, "I")]
    order, typ = icip2024.get_order_typ_list(intra_size, n_frames)
    if sorted(order) != list(range(n_frames)) or len(typ) != n_frames or typ[order[0]] != "I":
        raise hip.VcError(f"get_order_typ_list({intra_size}, {n_frames}) is no coding order of {n_frames} frames: {order}")
    return [(o, typ[o]) for o in order]


def pack_sequence(records, width, height, intra_size, s, intra_quality, family=SEQUENCE_FAMILY_ICIP2024):
    """``records``: [(type "I" | "B", display order, container bytes)] in coding order -- checked against :func:`sequence_plan`."""
    records = [(t, int(o), bytes(b)) for t, o, b in records]
    if family != SEQUENCE_FAMILY_ICIP2024:
        raise hip.VcError(f"sequence file: model family {family} (only {SEQUENCE_FAMILY_ICIP2024} = ICIP2024 is defined)")
    if not (1 <= int(width) <= 0xffff and 1 <= int(height) <= 0xffff and 1 <= int(intra_size) <= 0xffff and 0 <= int(intra_quality) <= 0xff) \
            or not np.isfinite(float(s)) or not 1 <= len(records) <= 0xffffffff:
        raise hip.VcError("sequence file: a header field is out of range")
    if [(o, t) for t, o, _ in records] != sequence_plan(intra_size, len(records)):
        raise hip.VcError("sequence file: the records are not in the coding order of get_order_typ_list")
    if any(len(b) > 0xffffffff for _, _, b in records):
        raise hip.VcError("sequence file: a frame is longer than the 32-bit length field")
    head = SEQUENCE_HEADER.pack(SEQUENCE_MAGIC, SEQUENCE_VERSION, family, int(width), int(height), len(records), int(intra_size), float(s),
                                int(intra_quality))
    return head + b"".join(SEQUENCE_RECORD.pack(SEQUENCE_TYPES.index(t), o, len(b)) + b for t, o, b in records)


def unpack_sequence(data):
    """Inverse of :func:`pack_sequence`: ``{"family", "width", "height", "frames", "intra_size", "s", "intra_quality", "records":
    [(type, display order, container bytes)] in coding order}``.  Magic, version, family, field ranges, the frame count against the
    buffer's length (before anything is sized by it), every record's length against the data that is left, the record sequence
    against :func:`sequence_plan` and the absence of trailing bytes are validated before anything is returned (VcError)."""
    data = bytes(data)
    fixed = SEQUENCE_HEADER.size
    if len(data) < fixed:
        raise hip.VcError(f"sequence file: {len(data)} bytes is shorter than the {fixed}-byte header")
    magic, version, family, width, height, frames, intra_size, s, intra_quality = SEQUENCE_HEADER.unpack_from(data, 0)
    if magic != SEQUENCE_MAGIC:
        raise hip.VcError(f"sequence file: magic {magic!r} is not {SEQUENCE_MAGIC!r}")
    if version != SEQUENCE_VERSION:
        raise hip.VcError(f"sequence file: version {version} (this reader knows {SEQUENCE_VERSION})")
    if family != SEQUENCE_FAMILY_ICIP2024:
        raise hip.VcError(f"sequence file: model family {family} (only {SEQUENCE_FAMILY_ICIP2024} = ICIP2024 is defined)")
    if width < 1 or height < 1 or intra_size < 1 or not np.isfinite(s):
        raise hip.VcError(f"sequence file: picture {width}x{height} / intra_size {intra_size} / level {s} out of range")
    if frames < 1 or fixed + frames * SEQUENCE_RECORD.size > len(data):
        raise hip.VcError(f"sequence file: {frames} frames do not fit {len(data)} bytes")
    plan = sequence_plan(intra_size, frames)
    records, pos = [], fixed
    for k, (order, typ) in enumerate(plan):
        if pos + SEQUENCE_RECORD.size > len(data):
            raise hip.VcError(f"sequence file: the data ends before record {k} of {frames}")
        t, o, length = SEQUENCE_RECORD.unpack_from(data, pos)
        pos += SEQUENCE_RECORD.size
        if t >= len(SEQUENCE_TYPES) or (o, SEQUENCE_TYPES[t]) != (order, typ):
            raise hip.VcError(f"sequence file: record {k} is (order {o}, type {t}), the coding order asks for ({order}, {typ})")
        if length > len(data) - pos:
            raise hip.VcError(f"sequence file: record {k} asks for {length} bytes, {len(data) - pos} are left")
        records.append((typ, o, data[pos:pos + length]))
        pos += length
    if pos != len(data):
        raise hip.VcError(f"sequence file: {len(data) - pos} trailing bytes behind the last record")
    return {"family": family, "width": width, "height": height, "frames": frames, "intra_size": intra_size, "s": s,
            "intra_quality": intra_quality, "records": records}
