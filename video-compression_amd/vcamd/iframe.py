"""I-frame codec of the evaluation loop: CompressAI's ``mbt2018_mean`` architecture on MI355X.

The reference codes the GOP boundary frames with ``compressai.zoo.mbt2018_mean(quality, "mse",
pretrained=True)`` (LHBDC/test/testing.py:78-86,209; Flex-Rate.../test/testing.py:237) -- SURVEY.md section 8(f)
row 2.  This is the same mean-scale hyperprior entropy path as the B-frame compressors with 5x5 stride-2
(transposed) convolutions and GDN; module/attribute names follow compressai.models.MeanScaleHyperprior so
the zoo checkpoints' state_dict keys load unchanged.  The zoo weights are downloaded from S3 by CompressAI and
are not available offline: ``pretrained=True`` raises, benchmarks use seeded weights.
"""
import torch
import torch.nn as nn

from . import hip
from .layers import GDN, BitCounter, MeanScaleHyperprior
from .lhbdc import _require_cuda


def conv(in_channels, out_channels, kernel_size=5, stride=2):
    return nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=kernel_size // 2)


def deconv(in_channels, out_channels, kernel_size=5, stride=2):
    return nn.ConvTranspose2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride,
                              output_padding=stride - 1, padding=kernel_size // 2)


class ImageMeanScaleHyperprior(MeanScaleHyperprior):
    def __init__(self, N, M, **kwargs):
        super().__init__(N=N, M=M, **kwargs)
        self.g_a = nn.Sequential(conv(3, N), GDN(N), conv(N, N), GDN(N), conv(N, N), GDN(N), conv(N, M))
        self.g_s = nn.Sequential(deconv(M, N), GDN(N, inverse=True), deconv(N, N), GDN(N, inverse=True),
                                 deconv(N, N), GDN(N, inverse=True), deconv(N, 3))
        self.h_a = nn.Sequential(conv(M, N, stride=1, kernel_size=3), nn.LeakyReLU(inplace=True), conv(N, N),
                                 nn.LeakyReLU(inplace=True), conv(N, N))
        self.h_s = nn.Sequential(deconv(N, M), nn.LeakyReLU(inplace=True), deconv(M, M * 3 // 2),
                                 nn.LeakyReLU(inplace=True), conv(M * 3 // 2, M * 2, stride=1, kernel_size=3))

    def forward_device(self, x, likelihoods=None):
        """(x_hat NCHW, bits float64 device tensor [n, 2] = per image (y, z)); no host sync."""
        _require_cuda(x)
        n = x.shape[0]
        bits = BitCounter(x.device, max_rows=2 * n)
        x_hat = self.forward_t(hip.nchw_to_nhwc(x.contiguous().float()), bits, likelihoods=likelihoods)
        return hip.nhwc_to_nchw(x_hat), bits.totals().view(n, 2)

    def forward(self, x):
        """{"x_hat", "likelihoods": {"y","z"}} as compressai's MeanScaleHyperprior.forward returns (what image_compress
        reads: LHBDC/test/testing.py:58-63), plus "bits" = their -log2 sums reduced on the device."""
        lik = {}
        x_hat, tot = self.forward_device(x, likelihoods=lik)
        return {"x_hat": x_hat, "likelihoods": lik, "bits": {"y": tot[:, 0].sum(), "z": tot[:, 1].sum()}}

    CODERS = ("host", "device")

    def _check_coder(self, coder, waves):
        if coder not in self.CODERS or not hip.irans_waves_ok(waves):
            raise hip.VcError(f"coder {coder!r} / waves {waves!r}: one of {self.CODERS}, waves a power of two in 1..16")

    def compress(self, x, coder="host", waves=4):
        """``coder="host"`` (default): CompressAI's ``{"strings": [y strings, z strings], "shape"}`` from the host range coder.

        ``coder="device"``: "strings" is one payload of the interleaved coder per image -- two segments, z with the factorised tables
        then y with the Gaussian ones, one vc_irans_encode launch on the tensors of code_t, as a payload of a ``VCLD`` container --
        and the result gains "x_hat" (the clamped reconstruction: bit for bit what ``decompress(coder="device")`` returns), "bits"
        (0-dim float64 device tensor: -log2 p of the coded symbols), "coder" and "waves"."""
        _require_cuda(x)
        if coder != "host":
            self._check_coder(coder, waves)
            return self._compress_device(x, waves)
        strings, (hz, wz) = self.compress_t(hip.nchw_to_nhwc(x.contiguous().float()))
        return {"strings": strings, "shape": torch.Size([hz, wz])}

    def decompress(self, strings, shape, coder="host", waves=None):
        """``coder="device"`` reads the payloads of ``compress(coder="device")`` (``waves`` as it returned it), or a
        hip.IransDecoder that already uploaded them: launches only; the decoder's error words are read once at the end (VcError)
        -- by the caller (``finish()`` / containers.finish_all) when it handed in the uploaded decoder."""
        if coder != "host":
            if coder not in self.CODERS:
                raise hip.VcError(f"coder {coder!r}: one of {self.CODERS}")
            return self._decompress_device(strings, shape, waves)
        assert isinstance(strings, list) and len(strings) == 2
        dev = self.entropy_bottleneck.quantiles.device
        # compressai's MeanScaleHyperprior.decompress clamps the reconstruction to [0, 1]
        return {"x_hat": hip.nhwc_to_nchw(self.decompress_t(strings, shape, dev, final_act=hip.ACT_CLAMP01))}

    # ---- coder="device": the interleaved coder's kernels on both sides, as bitstream.LhbdcStreamCodec(coder="device") ----------
    def _compress_device(self, x, waves):
        bits = BitCounter(x.device, max_rows=2)
        x_hat, sym = self.code_t(hip.nchw_to_nhwc(x.contiguous().float()), bits=bits)
        n, dev = sym["z_sym"].shape[0], sym["z_sym"].device
        total = bits.totals().sum()
        x_hat = hip.nhwc_to_nchw(hip.clamp01(x_hat))           # (exact: equals the decoder's fused ACT_CLAMP01)
        segments = [(sym["z_sym"], self.z_index_dev(n, sym["shape"], dev), 0), (sym["y_sym"], sym["y_idx"], 1)]
        tables = [self.entropy_bottleneck.irans_tables(), self.gaussian_conditional.irans_tables()]
        # the one synchronisation of the pass: the word counts of the payloads, after the last launch
        payloads = hip.irans_encode(segments, tables, waves)
        return {"strings": payloads, "shape": torch.Size(sym["shape"]), "x_hat": x_hat, "bits": total, "coder": "device", "waves": int(waves)}

    def _decompress_device(self, strings, shape, waves):
        hz, wz = int(shape[0]), int(shape[1])
        if not (1 <= hz <= 4096 and 1 <= wz <= 4096):
            raise hip.VcError(f"hyper-latent shape {hz}x{wz} is outside 1..4096")
        uploaded = isinstance(strings, hip.IransDecoder)
        if not uploaded:
            if not (isinstance(strings, (list, tuple)) and strings and all(isinstance(b, (bytes, bytearray)) for b in strings)):
                raise hip.VcError('decompress(coder="device"): strings is one payload (bytes) per image, as compress(coder="device") '
                                  "returns it -- this looks like the host-coded [y strings, z strings] lists")
            self._check_coder("device", waves)
        dec = strings if uploaded else hip.IransDecoder(strings, waves, self.entropy_bottleneck.quantiles.device)
        if waves is not None and dec.waves != int(waves):
            raise hip.VcError(f"the uploaded payloads were read with waves {dec.waves}, not {waves}")
        scales, means = self.hyper_decode_dev_t(dec, (hz, wz))
        x_hat = hip.nhwc_to_nchw(self.synth_decode_dev_t(dec, scales, means, final_act=hip.ACT_CLAMP01))
        if not uploaded:                           # the one read, after everything is enqueued
            dec.finish()
        return {"x_hat": x_hat}


# compressai.zoo.image.cfgs["mbt2018-mean"]: quality -> (N, M)
_CFGS = {1: (128, 192), 2: (128, 192), 3: (128, 192), 4: (128, 192), 5: (192, 320), 6: (192, 320), 7: (192, 320), 8: (192, 320)}


def mbt2018_mean(quality, metric="mse", pretrained=False, progress=True, **kwargs):
    if metric not in ("mse", "ms-ssim"):
        raise ValueError(f'Invalid metric "{metric}"')
    if quality not in _CFGS:
        raise ValueError(f'Invalid quality "{quality}", should be between (1, 8)')
    if pretrained:
        raise hip.VcError("the CompressAI model-zoo weights are fetched from the network and are not available "
                          "offline; build with pretrained=False and load a state_dict")
    return ImageMeanScaleHyperprior(*_CFGS[quality], **kwargs)
