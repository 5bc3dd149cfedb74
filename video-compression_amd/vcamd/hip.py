"""ctypes binding of libvc_hip.so (C ABI declared in include/vc_hip.h).

This is the only door to the compute path: there is NO CPU fallback.  If the library is missing the
import of any model module fails loudly with instructions to build it.
"""
import collections
import contextlib
import ctypes
import functools
import os
import threading

import numpy as np
import torch

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# VC_HIP_LIB lets a developer A/B two builds of the same ABI on one device; it must still be a HIP build.
LIB_PATH = os.environ.get("VC_HIP_LIB") or os.path.join(_PKG_DIR, "libvc_hip.so")

VC_OK = 0
ABI_VERSION = 6          # VC_ABI_VERSION of include/vc_hip.h (struct layouts below)
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_SIGMOID, ACT_CLAMP01 = 0, 1, 2, 3, 4
EPI_NONE, EPI_GDN, EPI_IGDN = 0, 1, 2
IN_NONE, IN_SQUARE = 0, 1
OUT_PLAIN, OUT_PIXELSHUFFLE2 = 0, 1
WARP_W1, WARP_W2, WARP_W3 = 1, 2, 3
EB_PARAMS_PER_CHANNEL = 60

_ERR = {-1: "VC_EINVAL (bad argument / unsupported shape)", -2: "VC_ELAUNCH (HIP launch failure)",
        -3: "VC_ENOMEM", -4: "VC_EDATA (corrupt bitstream / degenerate pmf)"}


class VcError(RuntimeError):
    pass


class View(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("n", ctypes.c_int), ("h", ctypes.c_int), ("w", ctypes.c_int),
                ("c", ctypes.c_int), ("sn", ctypes.c_longlong), ("sh", ctypes.c_longlong),
                ("sw", ctypes.c_longlong)]


class ConvDesc(ctypes.Structure):
    _fields_ = [("inp", View), ("out", View), ("wpk", ctypes.c_void_p), ("bias", ctypes.c_void_p),
                ("res", ctypes.c_void_p), ("res_sn", ctypes.c_longlong), ("res_sh", ctypes.c_longlong),
                ("res_sw", ctypes.c_longlong),
                ("mul", ctypes.c_void_p), ("mul_sn", ctypes.c_longlong), ("mul_sh", ctypes.c_longlong),
                ("mul_sw", ctypes.c_longlong),
                ("chscale", ctypes.c_void_p),
                ("kh", ctypes.c_int), ("kw", ctypes.c_int), ("stride", ctypes.c_int),
                ("act", ctypes.c_int), ("slope", ctypes.c_float),
                ("epi", ctypes.c_int), ("in_xform", ctypes.c_int), ("out_mode", ctypes.c_int),
                ("cfg", ctypes.c_int),
                ("tail_wpk", ctypes.c_void_p), ("tail_bias", ctypes.c_void_p)]      # fused 1x1 tail (VC_CFG_DMA), include/vc_hip.h


class RefineLayer(ctypes.Structure):
    """vc_refine_layer of include/vc_hip.h: the convolution whose output is recomputed in fp64 for boundary-case symbols"""
    _fields_ = [("inp", View), ("w_oihw", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("k", ctypes.c_int), ("stride", ctypes.c_int),
                ("c0", ctypes.c_int)]


_lib = None


class IransTablesC(ctypes.Structure):
    """vc_irans_tables: one host table set"""
    _fields_ = [("cdfs", ctypes.c_void_p), ("n_tables", ctypes.c_int), ("cdf_stride", ctypes.c_int),
                ("cdf_sizes", ctypes.c_void_p), ("offsets", ctypes.c_void_p)]


class IransSegmentC(ctypes.Structure):
    """vc_irans_segment (host)"""
    _fields_ = [("symbols", ctypes.c_void_p), ("indexes", ctypes.c_void_p), ("count", ctypes.c_size_t), ("table_set", ctypes.c_int)]


class IransDTables(ctypes.Structure):
    """vc_irans_dtables: device copies of a packed table set"""
    _fields_ = [("cdf16", ctypes.c_void_p), ("rows", ctypes.c_void_p), ("n_tables", ctypes.c_int), ("entries", ctypes.c_int)]


class IransDSegment(ctypes.Structure):
    """vc_irans_dsegment (device tensors)"""
    _fields_ = [("symbols", ctypes.c_void_p), ("indexes", ctypes.c_void_p), ("count", ctypes.c_uint32), ("table_set", ctypes.c_int)]


IRANS_MAX_WAVES = 16
IRANS_SUBSTREAM_HEADER = 516
IRANS_STATE_HEADER_WORDS = 2 + 5 * IRANS_MAX_WAVES + 2              # vc_irans_dstate in front of its states
IRANS_STATE_BYTES = 4 * IRANS_STATE_HEADER_WORDS + 8 * 64 * IRANS_MAX_WAVES
IRANS_ERRORS = {1: "sub-stream headers / word counts do not fit the payload", 2: "a sub-stream ended early", 4: "table index out of range"}


class KernelTimer:
    """Opt-in per-launch timing with HIP events recorded on the stream the kernels are launched on
    (torch's current stream).  Used by bench.py for the roofline line; never active in production."""

    def __init__(self):
        self.items = []

    def bracket(self, key, flops, launch, nbytes=0.0):
        """``flops`` / ``nbytes``: algorithmic work of the launch (bytes = each operand read once + the result
        written once, in the dtypes actually stored)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = launch()
        e1.record()
        self.items.append((key, flops, e0, e1, nbytes))
        return out

    def table(self):
        torch.cuda.synchronize()
        agg = {}
        for key, flops, e0, e1, nbytes in self.items:
            a = agg.setdefault(key, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            a["launches"] += 1
            a["ms"] += e0.elapsed_time(e1)
            a["flops"] += flops
            a["bytes"] += nbytes
        return agg


timer = None  # set to a KernelTimer() to collect
split_keys = set()   # (while a KernelTimer collects) the timing keys of launches that ran on the split-operand pipeline
kernel_symbols = {}  # timing key -> a prefix of the kernel symbol the launch ran (what a rocprofv3 trace names it)


def timed_hbm(key, nbytes, launch):
    """Run ``launch`` -- bracketed by HIP events under the key "hbm <key>" while a KernelTimer collects (bench.py's
    ``hbm_kernels`` block: achieved GB/s of the memory-bound kernels against the HBM peak); ``nbytes`` = algorithmic
    traffic (every operand read once, the result written once)."""
    if timer is None:
        return launch()
    return timer.bracket("hbm " + key, 0.0, launch, nbytes)


def lib():
    """Load libvc_hip.so once; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VcError(
            f"{LIB_PATH} not found: the HIP extension is the only compute path (no CPU fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C video-compression_amd/csrc`.")
    L = ctypes.CDLL(LIB_PATH)
    vp, ci, cf, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    sz = ctypes.c_size_t

    def sig(name, res, *args):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = list(args)

    sig("vc_version", ctypes.c_char_p)
    sig("vc_abi_version", ci)
    if L.vc_abi_version() != ABI_VERSION:
        raise VcError(f"{LIB_PATH} has ABI {L.vc_abi_version()}, this binding was written against {ABI_VERSION} (include/vc_hip.h: "
                      "VC_ABI_VERSION): rebuild with `make -C video-compression_amd/csrc`")
    sig("vc_target_arch", ctypes.c_char_p)
    sig("vc_conv_select_cfg", ci, ci, ci, ci, ci)
    sig("vc_conv_chunk", ci, ci, ci, ci, ci)
    sig("vc_conv_packed_weight_floats", sz, ci, ci, ci, ci, ci, ci)
    sig("vc_conv_packed_bias_floats", sz, ci, ci)
    sig("vc_conv_pack_weights", ci, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp)
    sig("vc_conv_packed_weight_bytes_f16", sz, ci, ci, ci, ci, ci, ci)
    sig("vc_conv_pack_weights_f16", ci, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp)
    sig("vc_conv_pack_tail_f16", ci, vp, vp, ci, ci, vp, vp)
    sig("vc_conv2d_nhwc", ci, vp, ctypes.POINTER(ConvDesc))
    sig("vc_conv_packed_weight_bytes_split", sz, ci, ci, ci)
    sig("vc_conv_pack_weights_split", ci, vp, vp, ci, ci, ci, ci, vp, vp)
    sig("vc_split3", ci, vp, View, vp, cll)
    sig("vc_split3_pad", ci, vp, View, vp, cll, ci)
    sig("vc_nchw_to_nhwc", ci, vp, vp, View)
    sig("vc_nhwc_to_nchw", ci, vp, View, vp)
    sig("vc_u8hwc_to_f32nchw_pad", ci, vp, vp, ci, ci, vp, ci, ci)
    sig("vc_f32nchw_to_u8hwc", ci, vp, vp, ci, ci, vp, ci, ci)
    sig("vc_avgpool_reflectpad", ci, vp, View, View, ci, cf)
    sig("vc_maxpool2", ci, vp, View, View)
    sig("vc_maxpool2_sp3", ci, vp, vp, cll, ci, ci, ci, ci, vp, cll)
    sig("vc_avgpool2_sp3", ci, vp, vp, cll, ci, ci, ci, ci, cf, vp, cll, View)
    sig("vc_upsample_bilinear_sp3", ci, vp, View, vp, cll, ci, ci, cf)
    sig("vc_upsample_bilinear", ci, vp, View, View, ci, ci, cf)
    sig("vc_axpby", ci, vp, View, View, View, cf, cf)
    sig("vc_clamp01", ci, vp, View, View)
    sig("vc_channel_scale", ci, vp, View, vp, View)
    sig("vc_warp", ci, vp, ci, View, View, View)
    sig("vc_spynet_preprocess", ci, vp, vp, View)
    sig("vc_spynet_level_input", ci, vp, View, View, View, View, View)
    sig("vc_spynet_level_input_sp3", ci, vp, View, View, View, vp, View)
    sig("vc_lhbdc_blend", ci, vp, View, View, View, View, View)
    sig("vc_flex_blend", ci, vp, View, View, View, View, View, View)
    sig("vc_flex_motion_split", ci, vp, View, View, View, cf)
    sig("vc_quantize_mask", ci, vp, View, View, vp, ci, ci)
    sig("vc_deform_pack_weights", ci, vp, ci, ci, ci, vp)
    sig("vc_deform_conv2d", ci, vp, View, View, View, vp, vp, ci, View)
    sig("vc_offset_diversity", ci, vp, View, View, View, View, View, View, cf, vp, vp, ci, View)
    sig("vc_deform_pair", ci, vp, View, View, View, View, vp, vp, ci, View)
    sig("vc_offset_diversity_hx", ci, vp, View, View, View, View, View, View, cf, vp, vp, ci, View)
    sig("vc_to_half", ci, vp, View, vp)
    sig("vc_offset_diversity_hxp", ci, vp, View, View, View, View, View, View, cf, vp, vp, ci, View)
    sig("vc_to_half_planar", ci, vp, View, ci, vp)
    sig("vc_deform_pair_hxp", ci, vp, View, View, View, View, vp, vp, ci, View)
    sig("vc_deform_select", ci, ci, ci, ci, ci, ci, ci, ci)
    sig("vc_attention_gate", ci, vp, View, View, View, View)
    sig("vc_sse_clamp01", ci, vp, View, View, vp, ci)
    sig("vc_select_flow", ci, vp, vp, ci, ctypes.c_double, ctypes.POINTER(View), View, vp)
    sig("vc_eb_forward", ci, vp, View, vp, vp, vp, View, vp, vp, ci, vp)
    sig("vc_eb_dequant", ci, vp, vp, vp, vp, View)
    sig("vc_gc_forward", ci, vp, View, View, View, vp, vp, View, vp, ci, vp, vp, vp, vp, ci, vp)
    sig("vc_gc_indexes", ci, vp, View, vp, ci, vp)
    sig("vc_refine_scales", ci, vp, View, View, vp, vp, vp, ci, cf, vp)
    sig("vc_gc_dequant", ci, vp, vp, View, vp, View)
    sig("vc_gc_forward_ckbd", ci, vp, View, View, View, vp, vp, View, ci, vp, ci, vp, vp, vp, ci)
    sig("vc_gc_indexes_ckbd", ci, vp, View, ci, vp, ci, vp)
    sig("vc_gc_dequant_ckbd", ci, vp, vp, View, vp, ci, View)
    sig("vc_refine_y_symbols", ci, vp, View, RefineLayer, View, RefineLayer, cf, vp, View, vp, vp)
    sig("vc_refine_z_symbols", ci, vp, View, RefineLayer, vp, vp, cf, vp, View, vp, vp)
    sig("vc_bits_reduce", ci, vp, vp, ci, ci, vp)
    sig("vc_bits_slots", ci)
    sig("vc_psnr_uint8", ci, vp, vp, vp, ci, ci, ci, ci, ci, vp, ci, vp)
    sig("vc_msssim_workspace_bytes", sz, ci, ci, ci, ci)
    sig("vc_msssim", ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, cll, ci, vp, sz, vp, vp)
    sig("vc_picture_hash", ci, vp, vp, ci, sz, sz, vp, ci, vp)
    sig("vc_picture_hash_host", ctypes.c_uint64, vp, sz)
    sig("vc_gdn", ci, vp, View, vp, vp, ci, View, View)
    sig("vc_pad", ci, vp, View, View)
    sig("vc_pmf_to_quantized_cdf", ci, vp, ci, ci, vp)
    sig("vc_rans_bound", sz, sz)
    sig("vc_rans_encode_with_indexes", cll, vp, vp, sz, vp, ci, ci, vp, vp, vp, sz)
    sig("vc_rans_decode_with_indexes", ci, vp, sz, vp, sz, vp, ci, ci, vp, vp, vp)
    sig("vc_rans_decode_stream", ci, vp, sz, vp, vp, sz, vp, ci, ci, vp, vp, vp)
    sig("vc_irans_bound", sz, sz, ci)
    sig("vc_irans_wave_words", sz, sz, ci)
    sig("vc_irans_encode_host", cll, vp, ci, vp, ci, ci, vp, sz)
    sig("vc_irans_decode_host", ci, vp, sz, vp, ci, vp, ci, ci)
    sig("vc_irans_pack_tables", cll, vp, ci, ci, vp, vp, vp, vp)
    sig("vc_irans_tables_in_lds", ci, ci)
    sig("vc_irans_encode", ci, vp, vp, ci, vp, ci, ci, ci, vp, sz, vp)
    sig("vc_irans_decode_begin", ci, vp, vp, sz, vp, ci, ci, vp)
    sig("vc_irans_decode", ci, vp, vp, vp, ci, ci, vp, sz, IransDTables, vp)
    sig("vc_irans_decode_eb", ci, vp, vp, vp, ci, ci, sz, IransDTables, vp, vp, View, vp)
    sig("vc_irans_decode_gc", ci, vp, vp, vp, ci, ci, sz, IransDTables, View, View, vp, ci, vp, View, vp)
    sig("vc_irans_decode_gc_ckbd", ci, vp, vp, vp, ci, ci, sz, IransDTables, View, View, ci, vp, ci, vp, View, vp)
    _lib = L
    return L


EXPORTED_SYMBOLS = [
    "vc_version", "vc_abi_version", "vc_target_arch", "vc_conv_select_cfg", "vc_conv_chunk", "vc_conv_packed_weight_floats",
    "vc_conv_packed_bias_floats", "vc_conv_pack_weights", "vc_conv_packed_weight_bytes_f16",
    "vc_conv_pack_weights_f16", "vc_conv_pack_tail_f16", "vc_conv2d_nhwc", "vc_conv_packed_weight_bytes_split",
    "vc_conv_pack_weights_split", "vc_split3", "vc_split3_pad", "vc_nchw_to_nhwc",
    "vc_nhwc_to_nchw", "vc_u8hwc_to_f32nchw_pad", "vc_f32nchw_to_u8hwc", "vc_avgpool_reflectpad", "vc_maxpool2", "vc_maxpool2_sp3", "vc_avgpool2_sp3", "vc_upsample_bilinear", "vc_upsample_bilinear_sp3", "vc_axpby", "vc_clamp01", "vc_channel_scale", "vc_warp",
    "vc_spynet_preprocess", "vc_spynet_level_input", "vc_spynet_level_input_sp3", "vc_lhbdc_blend", "vc_flex_blend",
    "vc_flex_motion_split", "vc_quantize_mask", "vc_deform_pack_weights", "vc_deform_conv2d", "vc_offset_diversity", "vc_deform_pair", "vc_offset_diversity_hx", "vc_to_half", "vc_offset_diversity_hxp", "vc_to_half_planar", "vc_deform_pair_hxp", "vc_deform_select",
    "vc_attention_gate", "vc_sse_clamp01", "vc_select_flow", "vc_eb_forward", "vc_eb_dequant", "vc_gc_forward", "vc_gc_indexes", "vc_refine_scales",
    "vc_refine_y_symbols", "vc_refine_z_symbols", "vc_gc_dequant", "vc_gc_forward_ckbd", "vc_gc_indexes_ckbd", "vc_gc_dequant_ckbd", "vc_bits_reduce", "vc_bits_slots", "vc_psnr_uint8", "vc_msssim_workspace_bytes", "vc_msssim", "vc_picture_hash", "vc_picture_hash_host", "vc_pmf_to_quantized_cdf", "vc_rans_bound",
    "vc_rans_encode_with_indexes", "vc_rans_decode_with_indexes", "vc_rans_decode_stream",
    "vc_irans_bound", "vc_irans_wave_words", "vc_irans_encode_host", "vc_irans_decode_host", "vc_irans_pack_tables",
    "vc_irans_tables_in_lds", "vc_irans_encode", "vc_irans_decode_begin", "vc_irans_decode",
    "vc_irans_decode_eb", "vc_irans_decode_gc", "vc_irans_decode_gc_ckbd",
    # the operator spellings of SURVEY.md 8(b), thin forwards (csrc/abi_aliases.cpp)
    "vc_gdn", "vc_spynet_level", "vc_pool", "vc_upsample", "vc_pad", "vc_blend", "vc_factorized_bits", "vc_gaussian_symbols",
]


DEBUG_SYNC = bool(int(os.environ.get("VC_DEBUG_SYNC", "0")))   # synchronise after every launch to localise a fault


def check(rc, what):
    if rc != VC_OK:
        raise VcError(f"{what} failed: {_ERR.get(rc, rc)}")
    if DEBUG_SYNC:
        try:
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            raise VcError(f"device fault during {what}: {e}") from e


def stream():
    """The HIP stream torch is currently enqueuing on (so torch allocations and our kernels order)."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------
# device tensors: channels-last fp32 buffers addressed through views
# ------------------------------------------------------------------------------------------------
class T:
    """A channels-last window into a flat device buffer: shape (n,h,w,c), strides in ELEMENTS, element offset.
    ``dtype`` is "f32" everywhere except for activations that only feed fp16-path convolutions ("f16", see
    VC_CFG_IN_F16 / VC_CFG_OUT_F16): those are produced and consumed by vc_conv2d_nhwc alone."""
    __slots__ = ("buf", "n", "h", "w", "c", "sn", "sh", "sw", "off", "dtype")

    def __init__(self, buf, n, h, w, c, sn, sh, sw, off=0, dtype="f32"):
        self.buf, self.n, self.h, self.w, self.c = buf, n, h, w, c
        self.sn, self.sh, self.sw, self.off, self.dtype = sn, sh, sw, off, dtype

    @staticmethod
    def empty(n, h, w, c, device, dtype="f32"):
        if dtype == "sp3":     # split tensor of the split-operand fp32 path: dense [n][c/8][h][w][3][8] bf16 (csrc/conv_split.h)
            if c % 8:
                raise VcError("a split tensor holds groups of 8 channels")
            # sn = planes of 8 channels per image of the underlying buffer, off = first plane of this window
            return T(torch.empty(n * h * w * c * 3, dtype=torch.int16, device=device), n, h, w, c, c // 8, 0, 0, 0, dtype)
        buf = torch.empty(n * h * w * c, dtype=torch.float16 if dtype == "f16" else torch.float32, device=device)
        return T(buf, n, h, w, c, h * w * c, w * c, c, 0, dtype)

    def channels(self, c0, c1):
        if self.dtype == "sp3":          # a window of planes: the split form of a channel slice of a concat buffer
            if c0 % 8 or c1 % 8:
                raise VcError("a split tensor is sliced in groups of 8 channels")
            return T(self.buf, self.n, self.h, self.w, c1 - c0, self.sn, 0, 0, self.off + c0 // 8, self.dtype)
        return T(self.buf, self.n, self.h, self.w, c1 - c0, self.sn, self.sh, self.sw, self.off + c0, self.dtype)

    def crop(self, h, w):
        if self.dtype == "sp3":
            raise VcError("a split tensor is plane-major: it has no crop window")
        return T(self.buf, self.n, h, w, self.c, self.sn, self.sh, self.sw, self.off, self.dtype)

    def images(self, n0, n1):
        if self.dtype == "sp3":
            return T(self.buf, n1 - n0, self.h, self.w, self.c, self.sn, 0, 0, self.off + n0 * self.sn, self.dtype)
        return T(self.buf, n1 - n0, self.h, self.w, self.c, self.sn, self.sh, self.sw, self.off + n0 * self.sn, self.dtype)

    @property
    def ptr(self):
        if self.dtype == "sp3":
            return self.buf.data_ptr() + self.off * self.h * self.w * 48
        return self.buf.data_ptr() + (2 if self.dtype == "f16" else 4) * self.off

    def view(self, allow_half=False):
        if self.dtype == "sp3":
            raise VcError("split tensors are private to the convolution engine (split_view)")
        if self.dtype != "f32" and not allow_half:
            raise VcError("half-precision activations are private to the fp16 convolution path")
        return View(self.ptr, self.n, self.h, self.w, self.c, self.sn, self.sh, self.sw)

    @property
    def image_bytes(self):
        """split tensors: distance between images in bytes"""
        return self.sn * self.h * self.w * 48

    def split_view(self):
        return View(self.ptr, self.n, self.h, self.w, self.c, self.image_bytes, 0, 0)

    def to_nchw(self):
        """Debug/inspection helper (torch indexing, not on the hot path)."""
        if self.dtype == "sp3":
            raise VcError("to_nchw reads fp32 / half windows (a split tensor holds three bf16 pieces per value)")
        full = self.buf[self.off:]
        return torch.as_strided(full, (self.n, self.c, self.h, self.w), (self.sn, 1, self.sh, self.sw)).contiguous().float()


NULL_VIEW = View(None, 0, 0, 0, 0, 0, 0, 0)


def nchw_to_nhwc(x):
    x = x.contiguous().float()
    n, c, h, w = x.shape
    out = T.empty(n, h, w, c, x.device)
    check(lib().vc_nchw_to_nhwc(stream(), x.data_ptr(), out.view()), "vc_nchw_to_nhwc")
    return out


def nhwc_to_nchw(t):
    out = torch.empty((t.n, t.c, t.h, t.w), dtype=torch.float32, device=t.buf.device)
    check(lib().vc_nhwc_to_nchw(stream(), t.view(), out.data_ptr()), "vc_nhwc_to_nchw")
    return out


def frame_from_uint8(u8_hwc, hp=None, wp=None, out=None):
    """uint8 RGB [h,w,3] CUDA tensor -> padded fp32 NCHW [1,3,hp,wp] (x/255, reflection pad to multiples of 64):
    ``process_frame`` of LHBDC/encode_B.py:58-64 without a torch operator."""
    h, w, c = u8_hwc.shape
    if c != 3 or u8_hwc.dtype != torch.uint8 or not u8_hwc.is_cuda or not u8_hwc.is_contiguous():
        raise VcError("frame_from_uint8 takes a contiguous uint8 [h,w,3] CUDA tensor")
    hp = hp or h + (64 - h % 64) % 64
    wp = wp or w + (64 - w % 64) % 64
    if out is None:
        out = torch.empty((1, 3, hp, wp), dtype=torch.float32, device=u8_hwc.device)
    check(lib().vc_u8hwc_to_f32nchw_pad(stream(), u8_hwc.data_ptr(), h, w, out.data_ptr(), hp, wp), "vc_u8hwc_to_f32nchw_pad")
    return out


def frame_to_uint8(x_nchw, h, w):
    """fp32 NCHW [1,3,hp,wp] CUDA frame -> uint8 RGB [h,w,3] of its top-left window (``float_to_uint8`` + crop of
    LHBDC/decode_B.py:35-38,122-123)."""
    _, c, hp, wp = x_nchw.shape
    if c != 3 or x_nchw.dtype != torch.float32 or not x_nchw.is_cuda:
        raise VcError("frame_to_uint8 takes an fp32 [1,3,hp,wp] CUDA tensor")
    x_nchw = x_nchw.contiguous()
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=x_nchw.device)
    check(lib().vc_f32nchw_to_u8hwc(stream(), x_nchw.data_ptr(), hp, wp, out.data_ptr(), h, w), "vc_f32nchw_to_u8hwc")
    return out


# ------------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------------
# tile configurations: the enum of include/vc_hip.h under the same names
CFG_N128, CFG_N64, CFG_N32, CFG_N16, CFG_N4, CFG_N128B, CFG_PW, CFG_N32T16 = range(8)
CFG_EXACT = 0x100
CFG_F16 = 0x200
CFG_IN_F16 = 0x400
CFG_OUT_F16 = 0x800
CFG_RES_FIRST = 0x1000
CFG_RES_F16 = 0x2000        # fp16 path, VC_CFG_PWS only: `res` is a half-precision tensor (the identity path of a bottleneck chain)
CFG_PACK128 = 0x4000        # with CFG_DMA: weights / bias packed with the 128-channel configuration (padded to blocks of 128)
CFG_SPLIT = 10            # fp32 on the bf16 matrix pipe with split operands (csrc/conv_split.h); input: a split tensor (dtype "sp3")
CFG_IN_SP3 = 0x8000
CFG_OUT_SP3 = 0x10000
CFG_RES_SP3 = 0x20000
# "native": v_mfma_f32_* instances everywhere (rounds 1-4).  "split" (default since round 5, after the reference-parity tests
# came out equal on it: tests/test_reference_1080p_gpu.py): the layers the split-operand pipeline serves (5x5 / 7x7
# stride 1, cin % 8 == 0, cout % 32 == 0) run on it -- exact bf16 x 3 pieces, nine exact products, fp32 accumulate; same precision
# class, different summation order.  VC_FP32_MODE / set_fp32_mode().
_FP32_MODE = os.environ.get("VC_FP32_MODE", "split")
CFG_DMA = 8               # fp16 path: LDS-DMA pipeline, one persistent workgroup per CU (csrc/conv_dma.h); half-precision input only
CFG_PWS = 9               # streaming 1x1 kernel with LDS-DMA activation rings (csrc/conv_pws.hip)
AUTOTUNE = bool(int(os.environ.get("VC_AUTOTUNE", "1")))
# "fp32" (default, exact fp32 FMA chains like the reference) or "fp16" (BASELINE.json configs[4]: half-precision MFMA
# with fp32 accumulate for every eligible layer; judged on PSNR/bpp tolerance, never the headline number).
_PRECISION = os.environ.get("VC_CONV_PRECISION", "fp32")


# fp16 path only: keep activations whose sole consumers are fp16-path convolutions as half in HBM (bit-identical
# results, see VC_CFG_OUT_F16); VC_HALF_ACTIVATIONS=0 stores them as fp32 like every other tensor (A/B, tests).
HALF_ACTIVATIONS = bool(int(os.environ.get("VC_HALF_ACTIVATIONS", "1")))
# fp16 path only: keep the identity path of a chain of bottleneck blocks (x + f(x) per block, ICIP2024/src/model/elic.py:69-83)
# as half in HBM too.  NOT bit-neutral (one more rounding of the identity per block; VC_CFG_RES_F16): part of the fp16 mode's
# stated tolerance.  VC_HALF_RESIDUAL=0 keeps the identity fp32 (A/B, tests).
HALF_RESIDUAL = bool(int(os.environ.get("VC_HALF_RESIDUAL", "1")))
# fp16 path: the trailing 1x1 layer of a bottleneck block (ICIP2024/src/model/elic.py:69-83) rides in the epilogue of the block's
# 3x3 layer (LDS-DMA kernel, vc_conv_desc.tail_wpk): the 3x3 layer's output never reaches HBM.  VC_FUSE_TAIL=0 = three launches.
FUSE_TAIL = bool(int(os.environ.get("VC_FUSE_TAIL", "1")))
# fp16 path only: the deformable fusion of ICIP2024 gathers from HALF-precision copies of its feature maps (8 / 16 channels per
# group: one 16-byte gather per corner instead of two; the kernel is bound by its gathers).  Offsets, modulation, bilinear
# weights and accumulation stay fp32.  VC_HALF_DEFORM=0 gathers fp32 features (A/B, tests).
HALF_DEFORM = bool(int(os.environ.get("VC_HALF_DEFORM", "1")))
HALF_DEFORM_PLANAR = bool(int(os.environ.get("VC_HALF_DEFORM_PLANAR", "1")))   # group-planar half features under the deformable gathers
# fp16 path only: the deformable pairs of ICIP2023 (PackedDeform.pair) gather from group-planar half copies of the two references
# too (vc_deform_pair_hxp; needs HALF_DEFORM and HALF_DEFORM_PLANAR).  VC_HALF_DEFORM_PAIR=0 keeps the fp32 vc_deform_pair in
# fp16 mode (A/B, tests); the measurement behind the default is in DESIGN.md 4f.
HALF_DEFORM_PAIR = bool(int(os.environ.get("VC_HALF_DEFORM_PAIR", "1")))
# Bitstream paths (compress / decompress): scales within SCALE_REFINE_EPS (relative) of a scale-table entry are recomputed in fp64
# from the last hyper-synthesis layer's input (vc_refine_scales): this side's table indexes stop depending on its summation order.
# VC_SCALE_REFINE=0 keeps the plain fp32 scales (A/B, tests).
SCALE_REFINE = bool(int(os.environ.get("VC_SCALE_REFINE", "1")))
SCALE_REFINE_EPS = 2e-5
# Encoder side of the bitstream paths: latents whose difference with their centre (mu / the channel's median) lies within
# SYMBOL_REFINE_EPS of a half-integer are recomputed in fp64 from the inputs of the layers that produced them
# (vc_refine_y_symbols / vc_refine_z_symbols): the coded integer stops depending on this side's summation order in those layers.
# VC_SYMBOL_REFINE=0 keeps the plain fp32 rounding (A/B, tests).
SYMBOL_REFINE = bool(int(os.environ.get("VC_SYMBOL_REFINE", "1")))
SYMBOL_REFINE_EPS = 2e-5


def set_conv_precision(mode):
    """Applies to PackedConv objects created afterwards (models pack lazily: set it before the first forward, or
    call ``model.float()`` to drop the caches)."""
    global _PRECISION
    if mode not in ("fp32", "fp16"):
        raise ValueError("precision must be 'fp32' or 'fp16'")
    _PRECISION = mode


def conv_precision():
    return _PRECISION


def set_fp32_mode(mode):
    """"native" or "split" (see CFG_SPLIT); applies to calls made afterwards (the split packing is made on first use)."""
    global _FP32_MODE
    if mode not in ("native", "split"):
        raise ValueError("fp32 mode must be 'native' or 'split'")
    _FP32_MODE = mode


def fp32_mode():
    return _FP32_MODE


# The hyper-synthesis transform of the BITSTREAM paths always runs on this pipeline, whatever VC_FP32_MODE says: the scale-table
# indexes a decoder derives from it are part of the stream's meaning (the CompressAI format carries none), so a stream written
# under one fp32 mode must decode under the other.  (The transform is five small layers: its cost is nothing.)
BITSTREAM_HS_MODE = "native"


@contextlib.contextmanager
def fp32_mode_pinned(mode):
    global _FP32_MODE
    keep = _FP32_MODE
    _FP32_MODE = mode
    try:
        yield
    finally:
        _FP32_MODE = keep


def wants_split_at(pc, n, h, w):
    """Will the layer ``pc`` run on the split-operand pipeline for n images of h x w?  The hint a producer needs to leave its result
    as a split tensor (``out_sp3``)."""
    return _FP32_MODE == "split" and pc is not None and pc.split_ok and pc.cin_split == pc.cin and pc.split_pays(n, h, w)     # (a producer cannot write padding channels)


def wants_split(pc, x, h=None, w=None, _at=wants_split_at):
    """wants_split_at for an input of x's batch at h x w (default: x's own size).  (Bound to the predicate itself: replacing the module
    attribute ``wants_split_at`` redirects the call sites that name it, not this function's.)"""
    return _at(pc, x.n, x.h if h is None else h, x.w if w is None else w)


SplitGeometry = collections.namedtuple("SplitGeometry", "served chunk cin_split bn ntw cpl th period")      # see split_geometry
# What PackedConv._route decides: ``split``: the split-operand pipeline (else the classic one); ``out_dtype`` of the result; ``flags``:
# the VC_CFG_* flag bits; ``cfg``: the whole word where the configuration is forced; ``key``: of PackedConv.tuned (None: not consulted)
Route = collections.namedtuple("Route", "split out_dtype flags cfg key")


@functools.lru_cache(maxsize=None)
def _split_padded():
    """VC_SPLIT_PADDED=1 (first name VC_SPLIT3_PADDED): the per-chunk padded split instances for every layer.  Read ONCE per process,
    like split_period() of csrc/conv_split.hip: packing and every later launch must agree on the choice."""
    return any(os.environ.get(name, "")[:1] not in ("", "0") for name in ("VC_SPLIT_PADDED", "VC_SPLIT3_PADDED"))


def split_geometry(k, cout, cin):
    """The split-operand instance of a k x k layer -- this side's one statement of what csrc/conv_split.hip (split_cpl, split_block,
    split_period, ``th`` of conv_dispatch_split) and vc_conv_chunk(VC_CFG_SPLIT) decide.  ``served``: an instance exists (stride 1 is
    the caller's business); ``chunk``: input channels per chunk of ``cpl`` planes of 8, ``cin_split``: cin padded to it; ``bn``: output
    channels per workgroup = ``ntw`` N-tiles of 16; ``th``: rows of a 32-pixel tile; ``period``: the two-chunks-per-period instance."""
    cpl = 2 if k == 3 else 1
    chunk = 8 * cpl
    cin_split = (cin + chunk - 1) // chunk * chunk
    bn = 64 if cout % 64 == 0 else (32 if cout % 32 == 0 else 16)
    served = (k in (3, 5) and bn >= 32) or (k == 7 and cout % 16 == 0)
    th = 12 if k == 3 else (24 if bn == 16 else 16)
    return SplitGeometry(served, chunk, cin_split, bn, bn // 16, cpl, th, bn > 16 and cin_split % (2 * chunk) == 0 and not _split_padded())


def _vec16(t):
    """an fp32 window the split pipeline can touch in 16-byte groups (split windows are always aligned)"""
    return t is None or t.dtype == "sp3" or (t.dtype == "f32" and t.ptr % 16 == 0 and t.sn % 4 == 0 and t.sh % 4 == 0 and t.sw % 4 == 0)


def split3(x, out=None, c_out=None):
    """fp32 channels-last window -> split tensor (three bf16 pieces per value, exact): the input format of CFG_SPLIT layers.
    ``c_out`` (a multiple of 8, >= x.c): pad with zero channels (a layer whose weights are packed with zero rows for them)."""
    if c_out is not None and c_out != x.c or x.c % 8:
        c_out = c_out or (x.c + 7) // 8 * 8
        if out is None:
            out = T.empty(x.n, x.h, x.w, c_out, x.buf.device, "sp3")
        timed_hbm(f"k_split3_pad c{x.c}->{c_out} @{x.n}x{x.h}x{x.w}", x.n * x.h * x.w * (4.0 * x.c + 6.0 * c_out),
                  lambda: check(lib().vc_split3_pad(stream(), x.view(), out.ptr, out.image_bytes, c_out), "vc_split3_pad"))
        return out
    if out is None:
        out = T.empty(x.n, x.h, x.w, x.c, x.buf.device, "sp3")
    timed_hbm(f"k_split3 c{x.c} @{x.n}x{x.h}x{x.w}", 10.0 * x.n * x.h * x.w * x.c,
              lambda: check(lib().vc_split3(stream(), x.view(), out.ptr, out.image_bytes), "vc_split3"))
    return out


class PackedConv:
    """Weights of one nn.Conv2d re-laid out for the MFMA kernel (done once per model load).

    The three 32-wide tile configurations (128/64/32 output channels per workgroup) read the same packed
    weights and give bit-identical results; which one is fastest depends on how the launch quantises over
    256 CUs (tail effects), so the first eager call per input shape times the candidates on the device and
    keeps the winner (never during graph capture)."""

    def __init__(self, weight, bias, stride=1, pixelshuffle=False, device=None):
        L = lib()
        w = weight.detach().to("cpu", torch.float32).contiguous()
        cout, cin, kh, kw = w.shape
        self.cout, self.cin, self.k, self.stride, self.ps = cout, cin, kh, stride, bool(pixelshuffle)
        self.cfg = L.vc_conv_select_cfg(cout, cin, kh, stride)
        nw = L.vc_conv_packed_weight_floats(self.cfg, cout, cin, kh, kw, stride)
        nb = L.vc_conv_packed_bias_floats(self.cfg, cout)
        if nw == 0:
            raise VcError(f"unsupported convolution {cout}x{cin}x{kh}x{kw} stride {stride}")
        wpk = np.empty(nw, dtype=np.float32)
        bpk = np.empty(nb, dtype=np.float32)
        wnp = w.numpy()
        bnp = None if bias is None else bias.detach().to("cpu", torch.float32).contiguous().numpy()
        check(L.vc_conv_pack_weights(wnp.ctypes.data, None if bnp is None else bnp.ctypes.data, cout, cin, kh, kw,
                                     stride, self.cfg, int(self.ps), wpk.ctypes.data, bpk.ctypes.data),
              "vc_conv_pack_weights")
        self.wpk = torch.from_numpy(wpk).to(device)
        self.bias = torch.from_numpy(bpk).to(device)
        self.wpk16 = None
        if _PRECISION == "fp16":
            nbytes = L.vc_conv_packed_weight_bytes_f16(self.cfg, cout, cin, kh, kw, stride)
            if nbytes:
                w16 = np.empty(nbytes // 2, dtype=np.float16)
                check(L.vc_conv_pack_weights_f16(wnp.ctypes.data, None if bnp is None else bnp.ctypes.data, cout, cin, kh,
                                                 kw, stride, self.cfg, int(self.ps), w16.ctypes.data, bpk.ctypes.data),
                      "vc_conv_pack_weights_f16")
                self.wpk16 = torch.from_numpy(w16).to(device)
        self.tuned = {}
        self._tail = None
        self._wsplit = None
        # input channels are padded to the chunk of the split instance (8 for 5x5 / 7x7, 16 for 3x3) with zero weights: first layers
        # with 6 channels (LHBDC mask U-Net, Flex-Rate U-Net) run on the split pipeline behind vc_split3_pad
        self._split = split_geometry(kh, cout, cin)
        self.cin_split = self._split.cin_split
        split_shape = self._split.served and stride == 1 and not (pixelshuffle and kh != 3)
        if split_shape and self.cin_split != cin:
            wpad = np.zeros((cout, self.cin_split, kh, kw), dtype=np.float32)
            wpad[:, :cin] = wnp.reshape(cout, cin, kh, kw)
            self._raw32 = (wpad, bnp)
        else:
            self._raw32 = (wnp, bnp) if split_shape else None
        self._raw = (wnp, bnp) if (_PRECISION == "fp16" and kh == 1 and stride == 1 and cout == cin and cin in (64, 128) and not pixelshuffle) else None
        self._device = device
        ck = L.vc_conv_chunk(self.cfg, kh, stride, cin)
        self._pack128 = CFG_PACK128 if self.cfg == CFG_N128 else 0
        self.candidates = [c for c in range(self.cfg, CFG_N32 + 1) if L.vc_conv_chunk(c, kh, stride, cin) == ck] if self.cfg <= CFG_N32 else []
        if self.cfg == CFG_N128 and kh == 3 and stride == 1:
            self.candidates.append(CFG_N128B)  # 128-channel block with the waves arranged 2x2
        if self.candidates and kh == 1 and stride == 1 and not self.ps and 32 <= cin <= 128 and cout <= 128 and cin % 8 == 0:
            self.candidates.append(CFG_PW)     # streaming 1x1 kernel (skipped by the tuner when the call is not eligible)
            if cin % 32 == 0 and cout % 32 == 0 and os.environ.get("VC_PWS_KERNELS", "1") != "0":
                self.candidates.append(CFG_PWS)  # the same through per-wave LDS-DMA rings
        if self.candidates and kh == 7 and stride == 1:
            self.candidates.append(CFG_N32T16) # 16-row tiles (less halo per output)
        # VC_CFG_DMA (fp16 path, half-precision input; the library refuses shapes it has no instance for): 32 / 64 output channels,
        # blocks of 128, or -- plain output on the N128 packing, which pads weights and bias to 128s -- a partly padded last block
        dma_cout = cout in (32, 64) or cout % 128 == 0 or (cout >= 96 and cout % 4 == 0 and self.cfg == CFG_N128 and not self.ps)
        if (self.candidates and kh in (3, 7) and stride == 1 and cin % 32 == 0 and dma_cout
                and os.environ.get("VC_DMA_KERNELS", "1") != "0"):
            self.candidates.append(CFG_DMA)
        # the exact fp32 instances of the same pipeline (csrc/conv_dma.h, DmaCfg::F32): SPyNet's two big 7x7 layers
        # (7x7: 64 -> 32, 32 -> 64; 3x3: 64 / 128 / 256 input channels to 64 or a multiple of 128 output channels, pixel shuffle
        #  included -- the library declines what it has no instance for and the tuner skips it)
        f32_shape = ((kh == 7 and (cin, cout) in ((64, 32), (32, 64)) and not self.ps) or
                     (kh == 3 and cin in (64, 128, 256) and (cout == 64 or cout % 128 == 0) and self.cfg in (CFG_N128, CFG_N64)) or
                     (kh == 3 and (cin, cout) == (32, 64) and not self.ps) or
                     (kh == 5 and (cin, cout) in ((96, 32), (192, 64), (32, 64)) and not self.ps))
        self.dma_f32 = (bool(self.candidates) and stride == 1 and f32_shape
                        and os.environ.get("VC_DMA_KERNELS", "1") != "0" and os.environ.get("VC_DMA_F32", "1") != "0")
        if self.dma_f32 and CFG_DMA not in self.candidates:
            self.candidates.append(CFG_DMA)
        # every alternative must read THIS packing: same channel chunk (the zero padding of cin depends on it)
        self.candidates = [c for c in self.candidates if L.vc_conv_chunk(c, kh, stride, cin) == ck]

    def _pick_cfg(self, d, r):
        """The configuration word of a route that leaves the choice to ``tuned`` / the tuner."""
        if r.key in self.tuned:
            return self.tuned[r.key]
        if r.cfg is not None:
            return r.cfg
        flags, cands = r.flags | self._pack128, self.candidates
        if flags & CFG_F16 and CFG_N128B in cands:
            cands = [c for c in cands if c != CFG_N128]     # the 4x1 128-channel fp16 instance spills registers
        if not (flags & CFG_F16 and flags & CFG_IN_F16) and not (self.dma_f32 and not flags & CFG_F16):
            cands = [c for c in cands if c != CFG_DMA]   # the LDS-DMA pipeline copies pixels as they are: half tensors, or fp32 on its fp32 instances
        if flags & CFG_OUT_SP3:      # split output: the classic instances' and the streaming 1x1 kernel's epilogue
            cands = [c for c in cands if c in (CFG_N128, CFG_N64, CFG_N32, CFG_N16, CFG_N128B, CFG_N32T16, CFG_PWS)]
        if not AUTOTUNE or len(cands) < 2 or torch.cuda.is_current_stream_capturing():
            return (cands[0] if cands else self.cfg) | flags
        best, best_ms = self.cfg, float("inf")
        for c in cands:
            d.cfg = c | CFG_EXACT | flags
            if lib().vc_conv2d_nhwc(stream(), ctypes.byref(d)) != VC_OK:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                lib().vc_conv2d_nhwc(stream(), ctypes.byref(d))
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms < best_ms:
                best, best_ms = c, ms
        self.tuned[r.key] = best | CFG_EXACT | flags
        return self.tuned[r.key]

    @property
    def split_ok(self):
        """True when the split-operand fp32 pipeline (CFG_SPLIT) serves this layer."""
        return self._raw32 is not None and self.wpk16 is None

    def split_pays(self, n, h, w):
        """The split pipeline walks 16 x 32-pixel tiles with one workgroup per CU: on coarse pyramid levels (few tiles) the native
        instances with their 8-row tiles and several workgroups per CU are faster.  Decided per IMAGE, never by the batch: a
        frame must get the same bits whether it is coded alone or in a level-batched pass."""
        g = self._split
        return ((h + g.th - 1) // g.th) * ((w + 31) // 32) * (self.cout // g.bn) >= 48

    def split_pack(self):
        if self._wsplit is None:
            if self._raw32 is None:
                raise VcError("no split-operand instance for this layer")
            wnp, bnp = self._raw32
            nbytes = lib().vc_conv_packed_weight_bytes_split(self.cout, self.cin_split, self.k)
            if not nbytes:
                raise VcError("no split-operand instance for this layer")
            w = np.zeros(nbytes // 2, dtype=np.int16)
            b = np.empty(self.cout, dtype=np.float32)
            check(lib().vc_conv_pack_weights_split(wnp.ctypes.data, None if bnp is None else bnp.ctypes.data, self.cout, self.cin_split, self.k,
                                                   int(self.ps), w.ctypes.data, b.ctypes.data), "vc_conv_pack_weights_split")
            self._wsplit = (torch.from_numpy(w).to(self._device), torch.from_numpy(b).to(self._device))
        return self._wsplit

    def tail_pack(self):
        """This 1x1 C -> C layer (C = 64 or 128) as the fused tail of a 3x3 layer (vc_conv_pack_tail_f16): (weights, bias) on the device."""
        if self._tail is None:
            if self._raw is None:
                raise VcError("only a 1x1 64 -> 64 / 128 -> 128 layer of the fp16 path can be fused behind a 3x3 layer")
            wnp, bnp = self._raw
            c = self.cout
            w16 = np.empty(c * c, dtype=np.float16)
            b = np.empty(c, dtype=np.float32)
            check(lib().vc_conv_pack_tail_f16(np.ascontiguousarray(wnp.reshape(c, c)).ctypes.data, None if bnp is None else bnp.ctypes.data,
                                              c, c, w16.ctypes.data, b.ctypes.data), "vc_conv_pack_tail_f16")
            self._tail = (torch.from_numpy(w16).to(self._device), torch.from_numpy(b).to(self._device))
        return self._tail

    def can_fuse_tail(self, tail):
        """True when ``tail`` (a 1x1 PackedConv) can ride in this 3x3 layer's epilogue: fp16 path, C -> C -> C with C = 64 / 128."""
        return (FUSE_TAIL and self.wpk16 is not None and self.k == 3 and self.stride == 1 and not self.ps and self.cin == self.cout
                and self.cin in (64, 128) and CFG_DMA in self.candidates and tail._raw is not None and tail.cin == self.cout
                and tail.wpk16 is not None)

    def out_shape(self, h, w):
        k, s = self.k, self.stride
        ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
        return (2 * ho, 2 * wo, self.cout // 4) if self.ps else (ho, wo, self.cout)

    @property
    def half_ok(self):
        """True when this layer runs on the fp16 path and can therefore read a half-precision activation."""
        return self.wpk16 is not None

    @property
    def half_res_ok(self):
        """True when this layer can add a HALF-precision residual (fp16 path; streaming 1x1 kernel, or the LDS-DMA kernel for a 3x3
        layer with a half-precision input): the last layer of a bottleneck / residual block whose identity path is kept as half
        (see VC_CFG_RES_F16 in include/vc_hip.h)."""
        return self.wpk16 is not None and (CFG_PWS in self.candidates or (self.k == 3 and self.stride == 1 and CFG_DMA in self.candidates))

    def _route(self, x, out=None, act=ACT_NONE, slope=0.01, res=None, epi=EPI_NONE, mul=None, in_xform=IN_NONE, chscale=None,
               out_f16=False, res_first=False, tail=None, out_sp3=False):
        """Decide one call (the arguments of ``__call__``): pipeline, output dtype, flag word, forced configuration -- a Route.
        Refuses what no kernel serves; allocates nothing and calls nothing in the library."""
        ho, wo, co = self.out_shape(x.h, x.w)
        plain = epi == EPI_NONE and in_xform == IN_NONE and act < ACT_SIGMOID and mul is None and tail is None
        first = CFG_RES_FIRST if res_first else 0      # out = act(conv + res) instead of act(conv) + res
        # the split-operand pipeline: a split tensor left by the layer in front, or an fp32 window (converted by __call__) where it pays
        if x.dtype == "sp3" or (_FP32_MODE == "split" and self.split_ok and self.split_pays(x.n, x.h, x.w) and plain
                                and (out is None or out.dtype != "f16") and _vec16(out) and _vec16(res) and co % 4 == 0
                                and x.dtype == "f32" and x.c == self.cin and (self.cin_split != self.cin or (x.c % 8 == 0 and _vec16(x)))):
            if not plain:
                raise VcError("the split-operand pipeline has plain / (Leaky)ReLU epilogues only: no GDN, multiplier, input transform, "
                              "fused tail, sigmoid or clamp (a split tensor reached a layer that needs one)")
            if out is not None and out.dtype == "f16":
                raise VcError("the split-operand pipeline stores fp32 or split tensors")
            if not self.split_ok:
                raise VcError("a split tensor reached a layer the split-operand pipeline does not serve")
            if x.dtype == "sp3" and x.c != self.cin_split:
                raise VcError("a split tensor must bring the layer's (padded) channel count")
            if res is not None and res.dtype == "f16":
                raise VcError("the split-operand pipeline adds fp32 or split residuals")
            # (``out_f16`` is a hint, like on the classic pipeline: the result of a split layer stays fp32 / split)
            dt = out.dtype if out is not None else ("sp3" if out_sp3 else "f32")
            flags = (CFG_IN_SP3 | (CFG_OUT_SP3 if dt == "sp3" else 0) | first | (CFG_RES_SP3 if res is not None and res.dtype == "sp3" else 0))
            return Route(True, dt, flags, CFG_SPLIT | CFG_EXACT | flags, None)
        half_in = x.dtype == "f16"
        esz = 8 if half_in else 4
        use16 = (self.wpk16 is not None and in_xform == IN_NONE and x.sw % esz == 0 and x.sh % esz == 0 and x.sn % esz == 0
                 and x.ptr % 16 == 0)
        if half_in and not use16:
            raise VcError("a half-precision activation reached a layer that is not on the fp16 path")
        # fp16 mode: the fp32 GDN / IGDN instance of the streaming 1x1 kernel may STORE half (the input -- operand and identity -- of a
        # residual block that runs on the fp16 path; part of that mode's tolerance like every VC_HALF_RESIDUAL tensor)
        gdn_half_ok = (_PRECISION == "fp16" and HALF_ACTIVATIONS and HALF_RESIDUAL and epi != EPI_NONE and self.k == 1 and self.cin == 128
                       and self.cout == 128 and CFG_PWS in self.candidates and mul is x and x.dtype == "f32" and not res_first and chscale is None
                       and (res is None or res.dtype == "f32"))
        # a split consumer behind a NATIVE fp32 layer (stride-2 / 1x1 / GDN / small-cin layers): the classic instances write the three
        # bf16 pieces themselves (CFG_OUT_SP3); the streaming / LDS-DMA configurations do not, so the tuner is held to the classic ones
        sp_hint = (out_sp3 and _FP32_MODE == "split" and not use16 and co % 8 == 0 and self.cfg in (CFG_N128, CFG_N64, CFG_N32, CFG_N16)
                   and (res is None or res.dtype == "f32"))
        dt = out.dtype if out is not None else ("sp3" if sp_hint else
                                                ("f16" if (out_f16 and HALF_ACTIVATIONS and (use16 or gdn_half_ok) and co % 4 == 0) else "f32"))
        half_out = dt == "f16"
        gdn_half = half_out and not use16 and gdn_half_ok
        if half_out and not use16 and not gdn_half:
            raise VcError("a half-precision output needs the fp16 path")
        res_half = res is not None and res.dtype == "f16"
        if tail is not None and not (self.can_fuse_tail(tail) and use16 and half_in and epi == EPI_NONE and act < ACT_SIGMOID
                                     and chscale is None and not res_first):
            raise VcError("fused tail: a half-precision activation through a 3x3 C -> C layer of the fp16 path (PackedConv.can_fuse_tail)")
        if res_half and tail is None and not (use16 and self.half_res_ok and epi == EPI_NONE and act < ACT_SIGMOID):
            raise VcError("a half-precision residual needs the fp16 path's streaming 1x1 kernel (PackedConv.half_res_ok)")
        flags = first | (CFG_OUT_SP3 if dt == "sp3" else 0)
        if use16:
            flags |= CFG_F16 | (CFG_IN_F16 if half_in else 0) | (CFG_OUT_F16 if half_out else 0) | (CFG_RES_F16 if res_half else 0)
        # (the tuned choice is per shape AND per epilogue class: the streaming 1x1 kernel, for one, takes plain / ReLU / GDN epilogues but
        #  not sigmoid or clamp, so a layer called both ways must not share one entry.  Not in the key: CFG_PACK128, stated on every call of
        #  a layer packed with the 128-channel configuration -- the LDS-DMA kernel's blocks of 128 may run into the padding of 96 / 160 ...)
        key = (x.n, x.h, x.w, flags) if (act < ACT_SIGMOID and epi == EPI_NONE) else (x.n, x.h, x.w, flags, act, epi)
        if gdn_half:                  # the fp32 GDN instance of the streaming kernel, half store
            return Route(False, dt, flags | CFG_OUT_F16, CFG_PWS | CFG_EXACT | flags | CFG_OUT_F16, None)
        if tail is not None:          # out = tail(act(conv3x3(x))) + res in ONE launch of the LDS-DMA kernel
            return Route(False, dt, flags, CFG_DMA | CFG_EXACT | flags | self._pack128, None)
        # a half-precision residual: the streaming 1x1 kernel / the LDS-DMA 3x3 kernel (unless ``tuned`` pins the shape)
        forced = ((CFG_PWS if self.k == 1 else CFG_DMA) | CFG_EXACT | flags | self._pack128) if flags & CFG_RES_F16 else None
        return Route(False, dt, flags, forced, key)

    def _describe(self, r, x, out, act, slope, res, epi, mul, in_xform, chscale, tail):
        """The descriptor of a routed call, all but its configuration word (split windows: image distances in bytes)."""
        d = ConvDesc()
        d.inp = x.split_view() if x.dtype == "sp3" else x.view(True)
        d.out = out.split_view() if out.dtype == "sp3" else out.view(True)
        wpk, bias = self.split_pack() if r.split else (self.wpk16 if r.flags & CFG_F16 else self.wpk, self.bias)
        d.wpk, d.bias = wpk.data_ptr(), bias.data_ptr()
        if res is not None:
            d.res, d.res_sn, d.res_sh, d.res_sw = (res.ptr, res.image_bytes, 0, 0) if r.flags & CFG_RES_SP3 else (res.ptr, res.sn, res.sh, res.sw)
        if mul is not None:
            d.mul, d.mul_sn, d.mul_sh, d.mul_sw = mul.ptr, mul.sn, mul.sh, mul.sw
        if chscale is not None:
            d.chscale = chscale.data_ptr()
        if tail is not None:
            d.tail_wpk, d.tail_bias = (t.data_ptr() for t in tail.tail_pack())
        d.kh, d.kw, d.stride, d.out_mode = self.k, self.k, self.stride, (OUT_PIXELSHUFFLE2 if self.ps else OUT_PLAIN)
        d.act, d.slope, d.epi, d.in_xform = act, slope, epi, in_xform
        return d

    def _launch(self, d, r, x, out, res, mul, tail):
        """Launch a described call (and, while a KernelTimer collects, account for it under the layer's profiler key)."""
        ho, wo, co = self.out_shape(x.h, x.w)
        what = (f"vc_conv2d_nhwc(split k={self.k},{self.cin}->{self.cout})" if r.split else
                f"vc_conv2d_nhwc(k={self.k},s={self.stride},{self.cin}->{self.cout}{'+1x1 tail' if tail is not None else ''})")

        def launch_once():
            # A tuned choice is keyed by shape and flags, not by the alignment class of the views: a later call of the same shape
            # on a sliced / unaligned view may be refused by a configuration that needs 16-byte accesses (LDS-DMA, streaming 1x1).
            # The general configuration of this packing takes any view: retry on it instead of failing the layer.
            rc = lib().vc_conv2d_nhwc(stream(), ctypes.byref(d))
            if rc == -1 and tail is None and not r.split and (d.cfg & 0xff) != self.cfg:
                d.cfg = self.cfg | (d.cfg & ~0x1ff)
                rc = lib().vc_conv2d_nhwc(stream(), ctypes.byref(d))
            return rc
        if timer is None:
            return check(launch_once(), what)
        hq, wq = (ho // 2, wo // 2) if self.ps else (ho, wo)
        flops = 2.0 * x.n * hq * wq * self.cout * (self.cin * self.k * self.k + (tail.cin if tail is not None else 0))
        key = f"conv k{self.k}{'+k1' if tail is not None else ''} s{self.stride} {self.cin}->{self.cout} @{x.n}x{x.h}x{x.w}"
        # bytes per element as stored: split tensors 6 (a classic layer's split store is counted as the fp32 values it holds), half 2
        b_in, b_w = (6, 6) if r.split else (2 if r.flags & CFG_IN_F16 else 4, 2 if r.flags & CFG_F16 else 4)
        b_out = 6 if r.split and r.flags & CFG_OUT_SP3 else (2 if r.flags & CFG_OUT_F16 else 4)
        b_res = 6 if r.flags & CFG_RES_SP3 else (2 if r.flags & CFG_RES_F16 else 4)
        nbytes = (x.n * x.h * x.w * self.cin * b_in + x.n * ho * wo * co * b_out + self.cout * self.cin * self.k * self.k * b_w
                  + (x.n * ho * wo * co * b_res if res is not None else 0) + (x.n * ho * wo * co * 4 if mul is not None else 0))
        if r.split:
            g = self._split
            split_keys.add(key)
            kernel_symbols[key] = (f"conv_split_period_kernel<SplitPeriodCfg<{self.k}, {g.ntw}, {g.th}," if g.period else
                                   f"conv_split_kernel<SplitCfg<{self.k}, {g.ntw}, {g.cpl}, {g.th},")
        else:
            kernel_symbols[key] = {CFG_DMA: f"conv_dma_kernel<DmaCfg<{self.k}, {self.k}, {self.cin // (32 if r.flags & CFG_F16 else 16)},",
                                   CFG_PWS: "conv_pws_kernel<", CFG_N32T16: f"conv_mfma_kernel<{self.k}, {self.k}, 1, 16, TileCfg<32, 16",
                                   }.get(d.cfg & 0xff, f"conv_mfma_kernel<{self.k}, {self.k}, {self.stride},")
        timer.bracket(key, flops, lambda: check(launch_once(), what), nbytes)

    def __call__(self, x, out=None, act=ACT_NONE, slope=0.01, res=None, epi=EPI_NONE, mul=None,
                 in_xform=IN_NONE, chscale=None, out_f16=False, res_first=False, tail=None, out_sp3=False):
        """``out_f16``: a hint that every consumer of the result is an fp16-path convolution (``half_ok``), so the result may be stored
        as half (bit-identical downstream, half the traffic).  Honoured only when this layer itself runs on the fp16 path and allocates
        its own output; otherwise the result stays fp32.  ``out_sp3``: the same for a consumer on the split-operand pipeline."""
        r = self._route(x, out, act, slope, res, epi, mul, in_xform, chscale, out_f16, res_first, tail, out_sp3)
        if r.split and x.dtype != "sp3":
            x = split3(x, c_out=self.cin_split)
        if out is None:
            out = T.empty(x.n, *self.out_shape(x.h, x.w), x.buf.device, r.out_dtype)
        d = self._describe(r, x, out, act, slope, res, epi, mul, in_xform, chscale, tail)
        d.cfg = r.cfg if r.key is None else self._pick_cfg(d, r) | self._pack128
        self._launch(d, r, x, out, res, mul, tail)
        return out


# ------------------------------------------------------------------------------------------------
# thin wrappers
# ------------------------------------------------------------------------------------------------
def avgpool_reflectpad(x, k, scale=1.0, out_h=None, out_w=None):
    hp, wp = x.h // k, x.w // k
    out = T.empty(x.n, out_h or hp, out_w or wp, x.c, x.buf.device)
    check(lib().vc_avgpool_reflectpad(stream(), x.view(), out.view(), k, scale), "vc_avgpool_reflectpad")
    return out


def avgpool2_split(x, out_sp3):
    """F.avg_pool2d(x, 2) of a split tensor (window): split or fp32 result."""
    out = T.empty(x.n, x.h // 2, x.w // 2, x.c, x.buf.device, "sp3" if out_sp3 else "f32")
    timed_hbm(f"k_avgpool2_sp3 c{x.c} @{x.n}x{x.h}x{x.w}", x.n * x.c * (6.0 * x.h * x.w + (6.0 if out_sp3 else 4.0) * out.h * out.w),
              lambda: check(lib().vc_avgpool2_sp3(stream(), x.ptr, x.image_bytes, x.n, x.h, x.w, x.c, 1.0, out.ptr if out_sp3 else None,
                                                  out.image_bytes if out_sp3 else 0, NULL_VIEW if out_sp3 else out.view()), "vc_avgpool2_sp3"))
    return out


def maxpool2(x):
    if x.dtype == "sp3":          # between split-operand layers: split in, split out (exactly maxpool + vc_split3)
        out = T.empty(x.n, x.h // 2, x.w // 2, x.c, x.buf.device, "sp3")
        timed_hbm(f"k_maxpool2_sp3 c{x.c} @{x.n}x{x.h}x{x.w}", 6.0 * x.n * x.c * (x.h * x.w + out.h * out.w),
                  lambda: check(lib().vc_maxpool2_sp3(stream(), x.ptr, x.image_bytes, x.n, x.h, x.w, x.c, out.ptr, out.image_bytes), "vc_maxpool2_sp3"))
        return out
    out = T.empty(x.n, x.h // 2, x.w // 2, x.c, x.buf.device)
    check(lib().vc_maxpool2(stream(), x.view(), out.view()), "vc_maxpool2")
    return out


def upsample_bilinear(x, factor, align_corners=False, scale=1.0, out=None):
    if out is None:
        out = T.empty(x.n, x.h * factor, x.w * factor, x.c, x.buf.device)
    if out.dtype == "sp3":        # the up-sampled part of a concat buffer a split-operand convolution reads
        timed_hbm(f"k_upsample_bilinear_sp3 x{factor} c{x.c} @{x.n}x{x.h}x{x.w}", x.n * x.c * (4.0 * x.h * x.w + 6.0 * out.h * out.w),
                  lambda: check(lib().vc_upsample_bilinear_sp3(stream(), x.view(), out.ptr, out.image_bytes, factor, int(align_corners), scale),
                                "vc_upsample_bilinear_sp3"))
        return out
    timed_hbm(f"k_upsample_bilinear x{factor} c{x.c} @{x.n}x{x.h}x{x.w}", 4.0 * x.n * x.c * (x.h * x.w + out.h * out.w),
              lambda: check(lib().vc_upsample_bilinear(stream(), x.view(), out.view(), factor, int(align_corners), scale),
                            "vc_upsample_bilinear"))
    return out


def axpby(a, b, alpha=1.0, beta=1.0, out=None):
    if out is None:
        out = T.empty(a.n, a.h, a.w, a.c, a.buf.device)
    check(lib().vc_axpby(stream(), a.view(), b.view() if b is not None else NULL_VIEW, out.view(), alpha, beta),
          "vc_axpby")
    return out


def to_half(x):
    """Dense half-precision copy of a channels-last fp32 window (round to nearest even): the features the fp16-path
    deformable fusion gathers from."""
    out = T.empty(x.n, x.h, x.w, x.c, x.buf.device, "f16")
    check(lib().vc_to_half(stream(), x.view(), out.ptr), "vc_to_half")
    return out


def to_half_planar(x, cg):
    """Group-planar half-precision copy [n][c / cg][h][w][cg] of a channels-last fp32 window (vc_to_half_planar)."""
    out = T.empty(x.n, x.h, x.w, x.c, x.buf.device, "f16")
    check(lib().vc_to_half_planar(stream(), x.view(), int(cg), out.ptr), "vc_to_half_planar")
    return out


def clamp01(x, out=None):
    """clamp(x, 0, 1) of a channels-last window (``torch.clamp(x_hat, 0, 1)`` of ICIP2024/src/test.py:94 on the device path)."""
    if out is None:
        out = T.empty(x.n, x.h, x.w, x.c, x.buf.device)
    check(lib().vc_clamp01(stream(), x.view(), out.view()), "vc_clamp01")
    return out


def clamp01_nchw(x):
    """The same for a contiguous fp32 CUDA tensor of any shape (a decoded NCHW frame entering the reference buffer)."""
    x = x.contiguous()
    out = torch.empty_like(x)
    n = x.numel()
    check(lib().vc_clamp01(stream(), View(x.data_ptr(), 1, 1, n, 1, n, n, 1), View(out.data_ptr(), 1, 1, n, 1, n, n, 1)), "vc_clamp01")
    return out


def stack_images(items, out=None):
    """Windows of k images each -> ONE batched window, image by image (the batch of a level pass assembled by the
    layout kernel: no torch.cat of the frames)."""
    if len(items) == 1 and out is None:
        return items[0]
    total = sum(t.n for t in items)
    t0 = items[0]
    if out is None:
        out = T.empty(total, t0.h, t0.w, t0.c, t0.buf.device)
    i = 0
    for t in items:
        check(lib().vc_axpby(stream(), t.view(), NULL_VIEW, out.images(i, i + t.n).view(), 1.0, 0.0), "vc_axpby")
        i += t.n
    return out


def warp(convention, img, flow, out=None):
    if out is None:
        out = T.empty(img.n, flow.h, flow.w, img.c, img.buf.device)
    timed_hbm(f"k_warp W{convention} c{img.c} @{img.n}x{img.h}x{img.w}", 4.0 * img.n * img.h * img.w * (2 * img.c + 2),
              lambda: check(lib().vc_warp(stream(), convention, img.view(), flow.view(), out.view()), "vc_warp"))
    return out


def channel_scale(x, gain, out=None):
    if out is None:
        out = T.empty(x.n, x.h, x.w, x.c, x.buf.device)
    check(lib().vc_channel_scale(stream(), x.view(), gain.data_ptr(), out.view()), "vc_channel_scale")
    return out


def psnr_uint8(x_hat, x, h, w, out=None):
    """PSNR of the first image of two NCHW fp32 CUDA tensors on the uint8-rounded [:h,:w] crop (vc_psnr_uint8); returns a
    0-dim float64 device tensor (``out``: a 0-dim float64 view to write into) -- no host synchronisation."""
    if x_hat.dtype != torch.float32 or x.dtype != torch.float32 or not x_hat.is_cuda or not x.is_cuda:
        raise VcError("psnr_uint8 takes fp32 CUDA tensors")
    if x_hat.dim() != 4 or x.shape[1:] != x_hat.shape[1:]:
        raise VcError("psnr_uint8: NCHW tensors of the same frame size")
    a, b = x_hat[0], x[0]
    if not a.is_contiguous() or not b.is_contiguous():
        a, b = a.contiguous(), b.contiguous()
    h, w = min(int(h), a.shape[1]), min(int(w), a.shape[2])      # the loops slice [:h, :w]: a crop larger than the frame is the frame
    slots = lib().vc_bits_slots()
    scratch = torch.empty(slots, dtype=torch.float64, device=x.device)
    if out is None:
        out = torch.empty((), dtype=torch.float64, device=x.device)
    check(lib().vc_psnr_uint8(stream(), a.data_ptr(), b.data_ptr(), a.shape[0], a.shape[1], a.shape[2], int(h), int(w),
                              scratch.data_ptr(), slots, out.data_ptr()), "vc_psnr_uint8")
    return out


def msssim_uint8(x_hat, x, h, w, out=None, quantize=True, terms=False):
    """MS-SSIM (pytorch-msssim's ``ms_ssim`` with its defaults, data range 255; csrc/metrics.hip) of every image pair of two NCHW
    fp32 CUDA tensors on the [:h,:w] crop -- uint8-rounded like :func:`psnr_uint8` unless ``quantize=False`` (then v * 255).  All N
    images are scored by one call (six launches); returns a float64 device tensor [N] (``out``: a float64 view of that shape to write
    into) -- no host synchronisation, capturable.  ``terms=True``: returns (values, [N,5,C] per-scale terms after the clamp at 0)."""
    if x_hat.dtype != torch.float32 or x.dtype != torch.float32 or not x_hat.is_cuda or not x.is_cuda:
        raise VcError("msssim_uint8 takes fp32 CUDA tensors")
    if x_hat.dim() != 4 or x.shape != x_hat.shape:
        raise VcError("msssim_uint8: NCHW tensors of the same shape")
    a, b = x_hat.contiguous(), x.contiguous()
    n, c, H, W = a.shape
    h, w = min(int(h), H), min(int(w), W)      # the loops slice [:h, :w]: a crop larger than the frame is the frame
    if min(h, w) <= 160:
        raise VcError("msssim_uint8: five scales with an 11-tap window need min(h, w) > 160")
    nbytes = lib().vc_msssim_workspace_bytes(n, c, h, w)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=x.device)
    elif out.dtype != torch.float64 or out.numel() != n or not out.is_contiguous() or out.device != x.device:
        raise VcError("msssim_uint8: out is a contiguous float64 view with one element per image")
    t = torch.empty((n, 5, c), dtype=torch.float64, device=x.device) if terms else None
    timed_hbm(f"k_msssim c{c} @{n}x{h}x{w}", 8.0 * n * c * h * w,
              lambda: check(lib().vc_msssim(stream(), a.data_ptr(), b.data_ptr(), n, c, H, W, h, w, c * H * W, int(bool(quantize)),
                                            workspace.data_ptr(), nbytes, None if t is None else t.data_ptr(), out.data_ptr()),
                            "vc_msssim"))
    return (out, t) if terms else out


def picture_hash(x, out=None):
    """The decoded picture hash (include/vc_hip.h: "Decoded picture hash") of every image of a contiguous fp32 or int32 CUDA tensor
    [n, ...], its elements taken as 32-bit words: an int64 device tensor [n] holding the uint64 bits (``out``: a contiguous int64
    view of that shape to write into).  Two launches for any n, no host synchronisation."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in (torch.float32, torch.int32) or x.dim() < 1:
        raise VcError("picture_hash takes a fp32 or int32 CUDA tensor [n, ...]")
    if not x.is_contiguous():
        raise VcError("picture_hash: the tensor must be contiguous (the hash is one of its words in memory order)")
    n = x.shape[0]
    count = x.numel() // n if n else 0
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=x.device)
    elif out.dtype != torch.int64 or out.numel() != n or not out.is_contiguous() or out.device != x.device:
        raise VcError("picture_hash: out is a contiguous int64 view with one element per image")
    slots = lib().vc_bits_slots()
    partials = torch.empty(max(n, 1) * slots, dtype=torch.int64, device=x.device)
    check(lib().vc_picture_hash(stream(), x.data_ptr(), n, count, count, partials.data_ptr(), slots, out.data_ptr()), "vc_picture_hash")
    return out


def picture_hash_host(array):
    """The same hash of ONE image held in a numpy array of a 4-byte element type (float32, int32, uint32), through the library's
    host twin (vc_picture_hash_host): a Python int in 0 .. 2^64 - 1.  Needs no GPU."""
    a = np.ascontiguousarray(array)
    if a.dtype.itemsize != 4 or a.dtype.kind not in "fiu" or a.size < 1:
        raise VcError("picture_hash_host takes a non-empty array of float32, int32 or uint32")
    return int(lib().vc_picture_hash_host(a.ctypes.data, a.size))


def nchw_frames_to_nhwc(frames, out=None):
    """A list of [k,C,H,W] fp32 CUDA tensors -> ONE batched channels-last window, image by image: the batch of a level pass
    is assembled by the layout kernel itself (no torch.cat copy of the frames)."""
    total = sum(int(f.shape[0]) for f in frames)
    _, c, h, w = frames[0].shape
    if out is None:
        out = T.empty(total, h, w, c, frames[0].device)
    i = 0
    for f in frames:
        f = f.contiguous().float()
        if tuple(f.shape[1:]) != (c, h, w):
            raise VcError("frames of one pass must have the same shape")
        check(lib().vc_nchw_to_nhwc(stream(), f.data_ptr(), out.images(i, i + f.shape[0]).view()), "vc_nchw_to_nhwc")
        i += f.shape[0]
    return out


def attention_gate(a, b, identity, out=None):
    """out = a * sigmoid(b) + identity (compressai AttentionBlock)."""
    if out is None:
        out = T.empty(a.n, a.h, a.w, a.c, a.buf.device)
    check(lib().vc_attention_gate(stream(), a.view(), b.view(), identity.view(), out.view()), "vc_attention_gate")
    return out


def quantize_mask(x, out=None, gain=None, keep_parity=-1, do_round=True):
    """ICIP2024 entropy-model glue: out = keep ? round(x) * gain : 0 (see vc_quantize_mask)."""
    if out is None:
        out = T.empty(x.n, x.h, x.w, x.c, x.buf.device)
    check(lib().vc_quantize_mask(stream(), x.view(), out.view(), None if gain is None else gain.data_ptr(),
                                 keep_parity, int(do_round)), "vc_quantize_mask")
    return out


class PackedDeform:
    """Weights of a torchvision DeformConv2d(k=3, padding=1, groups=G) re-laid out per group for vc_deform_conv2d."""

    def __init__(self, weight, bias, groups, device):
        w = weight.detach().to("cpu", torch.float32).contiguous().numpy()
        cout, cg, kh, kw = w.shape
        if (kh, kw) != (3, 3) or cout % groups:
            raise VcError("only 3x3 grouped deformable convolutions are supported")
        dst = np.empty(groups * 9 * cg * (cout // groups), dtype=np.float32)
        check(lib().vc_deform_pack_weights(w.ctypes.data, cout, cg, groups, dst.ctypes.data), "vc_deform_pack_weights")
        self.wpk = torch.from_numpy(dst).to(device)
        self.bias = None if bias is None else bias.detach().to(device, torch.float32).contiguous()
        self.groups, self.cout, self.cin = groups, cout, cg * groups

    @classmethod
    def from_pair(cls, layer1, layer2):
        """Two DeformConv2d(c, c, 3, padding=1, groups=G/2) layers (parameter holders with weight / bias / groups) as ONE packed
        convolution of G groups for :meth:`pair`: weights and biases concatenated along the output channels."""
        if layer1.groups != layer2.groups or layer1.weight.shape != layer2.weight.shape or (layer1.bias is None) != (layer2.bias is None):
            raise VcError("a deformable pair needs two layers of the same shape")
        bias = None if layer1.bias is None else torch.cat([layer1.bias.detach(), layer2.bias.detach()])
        return cls(torch.cat([layer1.weight.detach(), layer2.weight.detach()]), bias, 2 * layer1.groups, layer1.weight.device)

    def _bias_ptr(self):
        return None if self.bias is None else self.bias.data_ptr()

    def _half_ok(self, x1, raw1, x2, raw2):
        """fp16 path: may this call gather from half copies of its fp32 features?  The half-feature instances of csrc/deform.hip
        (vector gathers, <= 8 groups per reference, offset records fetched in 16-byte pieces) and the kernels that make the copies
        need features AND both raw offset tensors 16-byte aligned, with strides and channel counts in whole float4s."""
        return (_PRECISION == "fp16" and HALF_DEFORM and self.groups <= 16 and x1.dtype == "f32" and x2.dtype == "f32"
                and all(t.ptr % 16 == 0 and t.sw % 4 == 0 and t.sh % 4 == 0 and t.sn % 4 == 0 and t.c % 4 == 0 for t in (x1, x2, raw1, raw2)))

    def _planar(self, x):
        """(group-planar half copy of the features ``x``, the view of ONE group's plane of it that the _hxp entries take)"""
        cg, hg = self.cin // self.groups, self.groups // 2
        p = to_half_planar(x, cg)
        return p, View(p.ptr, x.n, x.h, x.w, cg, hg * x.h * x.w * cg, x.w * cg, cg)

    def _timed(self, key, x, bytes_per_pixel, launch):
        if timer is None:
            launch()
        else:
            flops = 2.0 * x.n * x.h * x.w * self.cout * (self.cin // self.groups) * 9
            timer.bracket(f"{key} k3 {self.cin}->{self.cout} g{self.groups} @{x.n}x{x.h}x{x.w}", flops, launch, x.n * x.h * x.w * bytes_per_pixel)

    def pair(self, x1, raw1, x2, raw2, out=None):
        """vc_deform_pair: ICIP2023 DeformB.get_deformed_maps in one launch (fp32 features in; on the fp16 path the kernel gathers
        from group-planar half copies made here, vc_deform_pair_hxp)."""
        if x1.dtype != "f32" or x2.dtype != "f32":
            raise VcError("vc_deform_pair reads fp32 features")
        if out is None:
            out = T.empty(x1.n, x1.h, x1.w, self.cout, x1.buf.device)
        cg, og = self.cin // self.groups, self.cout // self.groups
        # the half-feature entry has one instance per shape of the model: (4, 4), (8, 8), (12, 12)
        planar = HALF_DEFORM_PLANAR and HALF_DEFORM_PAIR and cg == og and cg in (4, 8, 12) and self._half_ok(x1, raw1, x2, raw2)
        name = "vc_deform_pair_hxp" if planar else "vc_deform_pair"
        if planar:
            (_p1, v1), (_p2, v2) = self._planar(x1), self._planar(x2)       # (the copies live until this call returns)
        else:
            v1, v2 = x1.view(), x2.view()

        def launch():
            check(getattr(lib(), name)(stream(), v1, raw1.view(), v2, raw2.view(), self.wpk.data_ptr(), self._bias_ptr(), self.groups,
                                       out.view()), name)
        self._timed("deform pair", x1, (2.0 if planar else 4.0) * self.cin + 4.0 * (raw1.c + raw2.c + self.cout), launch)
        return out

    def conv(self, x, offset, mask=None, out=None):
        if out is None:
            out = T.empty(x.n, x.h, x.w, self.cout, x.buf.device)
        check(lib().vc_deform_conv2d(stream(), x.view(), offset.view(), NULL_VIEW if mask is None else mask.view(),
                                     self.wpk.data_ptr(), self._bias_ptr(), self.groups, out.view()), "vc_deform_conv2d")
        return out

    def offset_diversity(self, x1, raw1, flow1, x2, raw2, flow2, magnitude, out=None):
        if out is None:
            out = T.empty(x1.n, x1.h, x1.w, self.cout, x1.buf.device)
        cg = self.cin // self.groups
        half_x = cg % 4 == 0 and cg >= 8 and self._half_ok(x1, raw1, x2, raw2)
        planar = half_x and HALF_DEFORM_PLANAR
        name = "vc_offset_diversity_hxp" if planar else ("vc_offset_diversity_hx" if half_x else "vc_offset_diversity")
        if planar:
            (_p1, v1), (_p2, v2) = self._planar(x1), self._planar(x2)       # (the copies live until this call returns)
        else:
            if half_x:
                x1, x2 = to_half(x1), to_half(x2)
            v1, v2 = x1.view(True), x2.view(True)

        def launch():
            check(getattr(lib(), name)(stream(), v1, raw1.view(), flow1.view(), v2, raw2.view(), flow2.view(), float(magnitude),
                                       self.wpk.data_ptr(), self._bias_ptr(), self.groups, out.view()), name)
        self._timed("deform", x1, (2.0 if half_x else 4.0) * self.cin + 4.0 * (raw1.c + raw2.c + 4 + self.cout), launch)
        return out


# ------------------------------------------------------------------------------------------------
# host range coder
# ------------------------------------------------------------------------------------------------
def pmf_to_quantized_cdf(pmf, precision=16):
    p = np.ascontiguousarray(np.asarray(pmf, dtype=np.float32))
    cdf = np.empty(p.size + 1, dtype=np.uint32)
    check(lib().vc_pmf_to_quantized_cdf(p.ctypes.data, p.size, precision, cdf.ctypes.data), "vc_pmf_to_quantized_cdf")
    return cdf


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _tables(cdfs, cdf_sizes, offsets):
    cdfs = _i32(cdfs)
    sizes, offs = _i32(cdf_sizes).reshape(-1), _i32(offsets).reshape(-1)
    if cdfs.ndim != 2 or sizes.size != cdfs.shape[0] or offs.size != cdfs.shape[0]:
        raise VcError("range-coder tables: cdfs must be [n_tables, stride] with one size and one offset per table")
    return cdfs, sizes, offs


def rans_encode(symbols, indexes, cdfs, cdf_sizes, offsets):
    sym, idx = _i32(symbols).reshape(-1), _i32(indexes).reshape(-1)
    if sym.size != idx.size:
        raise VcError("range coder: one table index per symbol")
    cdfs, sizes, offs = _tables(cdfs, cdf_sizes, offsets)
    cap = lib().vc_rans_bound(sym.size)
    out = np.empty(cap // 4, dtype=np.uint32)
    n = lib().vc_rans_encode_with_indexes(sym.ctypes.data, idx.ctypes.data, sym.size, cdfs.ctypes.data, cdfs.shape[0],
                                          cdfs.shape[1], sizes.ctypes.data, offs.ctypes.data, out.ctypes.data, cap)
    if n < 0:
        check(int(n), "vc_rans_encode_with_indexes")
    return out.view(np.uint8)[:n].tobytes()


def rans_decode(data, indexes, cdfs, cdf_sizes, offsets):
    idx = _i32(indexes).reshape(-1)
    cdfs, sizes, offs = _tables(cdfs, cdf_sizes, offsets)
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(idx.size, dtype=np.int32)
    check(lib().vc_rans_decode_with_indexes(buf.ctypes.data, buf.size, idx.ctypes.data, idx.size, cdfs.ctypes.data,
                                            cdfs.shape[0], cdfs.shape[1], sizes.ctypes.data, offs.ctypes.data, out.ctypes.data),
          "vc_rans_decode_with_indexes")
    return out


class RansStreamDecoder:
    """compressai.ans.RansDecoder with set_stream / decode_stream (ICIP2024/src/model/elic.py:428-429): several decode calls
    over ONE string, each continuing where the previous stopped."""

    def __init__(self, data):
        self.buf = np.frombuffer(bytes(data), dtype=np.uint8)
        self.state = np.zeros(2, dtype=np.uint64)

    def decode_stream(self, indexes, cdfs, cdf_sizes, offsets):
        idx = _i32(indexes).reshape(-1)
        cdfs, sizes, offs = _tables(cdfs, cdf_sizes, offsets)
        out = np.empty(idx.size, dtype=np.int32)
        check(lib().vc_rans_decode_stream(self.buf.ctypes.data, self.buf.size, self.state.ctypes.data, idx.ctypes.data, idx.size,
                                          cdfs.ctypes.data, cdfs.shape[0], cdfs.shape[1], sizes.ctypes.data, offs.ctypes.data,
                                          out.ctypes.data), "vc_rans_decode_stream")
        return out


# ------------------------------------------------------------------------------------------------
# interleaved range coder (include/vc_hip.h): host reference and device kernels
# ------------------------------------------------------------------------------------------------
def irans_waves_ok(waves):
    return isinstance(waves, (int, np.integer)) and 1 <= waves <= IRANS_MAX_WAVES and (waves & (waves - 1)) == 0


def _irans_host_args(segments, table_sets, writable):
    """segments: [(symbols, indexes, table_set)] (decoder: symbols = None, allocated here); table_sets: [(cdfs, sizes, offsets)]"""
    keep, sets = [], (IransTablesC * max(len(table_sets), 1))()
    for k, ts in enumerate(table_sets):
        cdfs, sizes, offs = _tables(*ts)
        keep.append((cdfs, sizes, offs))
        sets[k] = IransTablesC(cdfs.ctypes.data, cdfs.shape[0], cdfs.shape[1], sizes.ctypes.data, offs.ctypes.data)
    segs = (IransSegmentC * max(len(segments), 1))()
    arrays = []
    for k, (sym, idx, which) in enumerate(segments):
        idx = _i32(idx).reshape(-1)
        sym = np.empty(idx.size, dtype=np.int32) if writable else _i32(sym).reshape(-1)
        if sym.size != idx.size:
            raise VcError("range coder: one table index per symbol")
        arrays.append((sym, idx))
        segs[k] = IransSegmentC(sym.ctypes.data, idx.ctypes.data, idx.size, int(which))
    return segs, sets, arrays, keep


def irans_encode_host(segments, table_sets, waves=4):
    """Host reference encoder: ``segments`` = [(symbols, indexes, table_set)], ``table_sets`` = [(cdfs, cdf_sizes, offsets)];
    returns the payload (bytes)."""
    segs, sets, arrays, keep = _irans_host_args(segments, table_sets, False)
    cap = sum(lib().vc_irans_bound(sym.size, int(waves)) for sym, _ in arrays) or lib().vc_irans_bound(0, int(waves))
    out = np.empty(max(cap, 4) // 4, dtype=np.uint32)
    n = lib().vc_irans_encode_host(segs, len(segments), sets, len(table_sets), int(waves), out.ctypes.data, cap)
    if n < 0:
        check(int(n), "vc_irans_encode_host")
    return out.view(np.uint8)[:n].tobytes()


def irans_decode_host(data, segments, table_sets, waves=4):
    """Host reference decoder: ``segments`` = [(indexes, table_set)]; returns one int32 array per segment."""
    segs, sets, arrays, keep = _irans_host_args([(None, idx, which) for idx, which in segments], table_sets, True)
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    check(lib().vc_irans_decode_host(buf.ctypes.data if buf.size else None, buf.size, segs, len(segments), sets, len(table_sets), int(waves)),
          "vc_irans_decode_host")
    return [sym for sym, _ in arrays]


class IransTables:
    """A table set packed for the kernels (vc_irans_pack_tables) and resident on ``device``: the used entries of every cdf row as
    u16 and per table (first entry, cdf_size, offset, mode).  The entropy models cache one and drop it in update()."""

    def __init__(self, cdfs, cdf_sizes, offsets, device):
        cdfs, sizes, offs = _tables(cdfs, cdf_sizes, offsets)
        args = (cdfs.ctypes.data, cdfs.shape[0], cdfs.shape[1], sizes.ctypes.data, offs.ctypes.data)
        n = lib().vc_irans_pack_tables(*args, None, None)
        if n < 0:
            check(int(n), "vc_irans_pack_tables")
        cdf16 = np.empty(n, dtype=np.uint16)
        rows = np.empty((cdfs.shape[0], 4), dtype=np.int32)
        lib().vc_irans_pack_tables(*args, cdf16.ctypes.data, rows.ctypes.data)
        self.entries, self.n_tables = int(n), int(cdfs.shape[0])
        self.cdf16 = torch.from_numpy(cdf16.view(np.int16)).to(device)
        self.rows = torch.from_numpy(rows).to(device)
        self.in_lds = bool(lib().vc_irans_tables_in_lds(self.entries))

    def struct(self):
        return IransDTables(self.cdf16.data_ptr(), self.rows.data_ptr(), self.n_tables, self.entries)


def irans_encode_launch(segments, table_sets, waves=4):
    """The launch of :func:`irans_encode` alone: nothing is read back.  Returns the job :func:`irans_encode_collect` takes, so that
    several payload sets (the two compressors of an LHBDC level) share ONE read of their word counts."""
    if not segments or not irans_waves_ok(waves):
        raise VcError("irans_encode: at least one segment, waves a power of two in 1..16")
    images, dev = int(segments[0][0].shape[0]), segments[0][0].device
    segs = (IransDSegment * len(segments))()
    cap = 0
    for k, (sym, idx, which) in enumerate(segments):
        if sym.dtype != torch.int32 or idx.dtype != torch.int32 or sym.shape != idx.shape or sym.dim() != 2 or sym.shape[0] != images \
                or not (sym.is_contiguous() and idx.is_contiguous() and sym.is_cuda and idx.is_cuda):
            raise VcError("irans_encode: symbols / indexes are dense int32 CUDA tensors [images, count]")
        segs[k] = IransDSegment(sym.data_ptr(), idx.data_ptr(), int(sym.shape[1]), int(which))
        cap += lib().vc_irans_wave_words(int(sym.shape[1]), int(waves))
    sets = (IransDTables * len(table_sets))(*[t.struct() for t in table_sets])
    region = IRANS_SUBSTREAM_HEADER // 4 + cap
    out = torch.empty((images * waves, region), dtype=torch.int32, device=dev)
    counts = torch.empty(images * waves, dtype=torch.int32, device=dev)
    check(lib().vc_irans_encode(stream(), segs, len(segments), sets, len(table_sets), images, int(waves), out.data_ptr(), cap,
                                counts.data_ptr()), "vc_irans_encode")
    return out, counts, cap, images, int(waves)


def irans_encode_collect(jobs):
    """One read of the word counts of every job (the one synchronisation), one copy of the used tails; returns, per job, one
    payload (bytes) per image."""
    used = torch.cat([j[1] for j in jobs]).cpu().numpy().astype(np.int64) & 0xffffffff
    if (used == 0xffffffff).any():
        raise VcError("vc_irans_encode: a table index is out of range")
    parts, at = [], 0
    for out, _, cap, images, waves in jobs:
        parts.extend(out[k, cap - int(c):] for k, c in enumerate(used[at:at + images * waves]))
        at += images * waves
    tails, result, at, pos = torch.cat(parts).cpu().numpy().tobytes(), [], 0, 0
    for _, _, _, images, waves in jobs:
        sizes = IRANS_SUBSTREAM_HEADER + 4 * used[at:at + images * waves].reshape(images, waves)
        ends = pos + np.concatenate([[0], np.cumsum(sizes.sum(axis=1))])
        result.append([tails[ends[j]:ends[j + 1]] for j in range(images)])
        at, pos = at + images * waves, int(ends[-1])
    return result


def irans_encode(segments, table_sets, waves=4):
    """Device encoder (vc_irans_encode): ``segments`` = [(symbols, indexes, table_set)] of int32 CUDA tensors [images, count],
    ``table_sets`` = [IransTables].  One launch, one read of the images x W word counts, one copy of the used tails; returns one
    payload (bytes) per image."""
    return irans_encode_collect([irans_encode_launch(segments, table_sets, waves)])[0]


class _PinnedStage:
    """Pinned host staging for the payload uploads, reused from call to call (pinning is an allocation of its own and costs more
    than the copy): two buffers in turn, each guarded by an event recorded behind the asynchronous copy that last read it."""

    def __init__(self):
        self.slots = [[None, None], [None, None]]                      # [pinned uint8 tensor, event of its last copy]
        self.turn = 0
        self.lock = threading.Lock()                                     # held from take() to release(): one upload fills a slot at a time

    def take(self, nbytes):
        self.lock.acquire()
        self.turn ^= 1
        slot = self.slots[self.turn]
        if slot[1] is not None:
            slot[1].synchronize()                                        # (a copy enqueued two uploads ago: long done)
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(max(1 << 20, 1 << (int(nbytes) - 1).bit_length()), dtype=torch.uint8).pin_memory()
        return slot

    def release(self, slot):
        slot[1] = torch.cuda.Event()
        slot[1].record()
        self.lock.release()


_stage = _PinnedStage()


class IransDecoder:
    """Device decoder of one payload per image: uploads the payloads once (pinned, non-blocking), reads the sub-stream headers
    into the device state (vc_irans_decode_begin), then :meth:`decode` is one launch per segment and nothing comes back to the
    host until :meth:`finish` reads the states' error words and cursors -- one copy, after everything that used the symbols.
    The constructor stages the payloads in pinned memory shared by the whole process (two buffers in turn, under a lock, so
    threads may build decoders concurrently): before it refills a buffer it waits on the host for the copy that last read it,
    enqueued two uploads earlier -- the one place this class may block, and it lies in front of the launches-only part."""

    def __init__(self, payloads, waves, device):
        if not payloads or not irans_waves_ok(waves):
            raise VcError("IransDecoder: at least one payload, waves a power of two in 1..16")
        self.images, self.waves = len(payloads), int(waves)
        where, pos = np.zeros((self.images, 2), dtype=np.int64), 0
        for j, p in enumerate(payloads):
            where[j] = (pos, len(p))
            pos += -(-len(p) // 16) * 4 + 4                              # every payload starts on a 16-byte boundary
        if pos > 0x7fffffff or max(len(p) for p in payloads) > 0xffffffff:
            raise VcError("IransDecoder: the payloads exceed the 32-bit word offsets of the format")
        nbytes = 4 * pos + 4 * where.size
        slot = _stage.take(nbytes)
        try:
            view = slot[0].numpy()
            for j, p in enumerate(payloads):                             # (the padding between payloads is never read)
                view[4 * where[j, 0]:4 * where[j, 0] + len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
            view[4 * pos:nbytes] = where.astype(np.uint32).reshape(-1).view(np.uint8)
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self.buf.copy_(slot[0][:nbytes], non_blocking=True)
        finally:
            _stage.release(slot)
        self.words = pos
        self.states = torch.empty(self.images * IRANS_STATE_BYTES, dtype=torch.uint8, device=device)
        check(lib().vc_irans_decode_begin(stream(), self.buf.data_ptr(), pos, self.buf.data_ptr() + 4 * pos, self.images, self.waves,
                                          self.states.data_ptr()), "vc_irans_decode_begin")

    def decode(self, indexes, tables, out=None):
        """indexes: int32 CUDA tensor [images, count]; returns the symbols, same shape (``out`` when given)."""
        if indexes.dtype != torch.int32 or indexes.dim() != 2 or indexes.shape[0] != self.images or not indexes.is_contiguous():
            raise VcError("IransDecoder.decode: indexes is a dense int32 tensor [images, count]")
        if out is None:
            out = torch.empty_like(indexes)

        def launch():
            check(lib().vc_irans_decode(stream(), self.buf.data_ptr(), self.states.data_ptr(), self.images, self.waves, indexes.data_ptr(),
                                        int(indexes.shape[1]), tables.struct(), out.data_ptr()), "vc_irans_decode")
        if timer is None:
            launch()
        else:                                  # (tools/icip_codec_bench.py: the decode kernels alone, from HIP events)
            timer.bracket("irans decode", 0.0, launch, 8.0 * indexes.numel())
        return out

    def _fused(self, key, nbytes, launch):
        if timer is None:
            launch()
        else:                                  # (tools/codec_bench.py: the fused decode kernels alone, from HIP events)
            timer.bracket(key, 0.0, launch, nbytes)

    def _symbols_out(self, symbols_out, count):
        if symbols_out is None:
            return None
        if symbols_out.dtype != torch.int32 or tuple(symbols_out.shape) != (self.images, count) or not symbols_out.is_contiguous():
            raise VcError("IransDecoder: symbols_out is a dense int32 tensor [images, count]")
        return symbols_out.data_ptr()

    def decode_eb(self, tables, eb_params, out_gain, z_hat, symbols_out=None):
        """The hyper-latent segment, fused (vc_irans_decode_eb): the table of a symbol is its channel's, ``z_hat`` (a T window
        [images, hz, wz, C]) receives what vc_eb_dequant would write.  ``symbols_out``: int32 [images, C*hz*wz] for tests / traces."""
        count = z_hat.c * z_hat.h * z_hat.w
        sym = self._symbols_out(symbols_out, count)
        self._fused("irans decode eb", 4.0 * self.images * count, lambda: check(lib().vc_irans_decode_eb(
            stream(), self.buf.data_ptr(), self.states.data_ptr(), self.images, self.waves, count, tables.struct(), eb_params.data_ptr(),
            None if out_gain is None else out_gain.data_ptr(), z_hat.view(), sym), "vc_irans_decode_eb"))
        return z_hat

    def decode_gc(self, tables, scales, means, scale_table, out_gain, y_hat, symbols_out=None):
        """The latent segment, fused (vc_irans_decode_gc): the table index of a symbol comes from ``scales``, ``y_hat`` receives
        what vc_gc_dequant would write from ``means`` (all three T windows [images, hy, wy, M]).  ``scale_table``: fp32 device
        tensor of at most 64 entries."""
        count = y_hat.c * y_hat.h * y_hat.w
        sym = self._symbols_out(symbols_out, count)
        self._fused("irans decode gc", 12.0 * self.images * count, lambda: check(lib().vc_irans_decode_gc(
            stream(), self.buf.data_ptr(), self.states.data_ptr(), self.images, self.waves, count, tables.struct(), scales.view(), means.view(),
            scale_table.data_ptr(), int(scale_table.numel()), None if out_gain is None else out_gain.data_ptr(), y_hat.view(), sym),
            "vc_irans_decode_gc"))
        return y_hat

    def decode_gc_ckbd(self, tables, scales, means, parity, scale_table, out_gain, y_hat, symbols_out=None):
        """One checkerboard parity of the latent segment, fused (vc_irans_decode_gc_ckbd): the symbols are in the squeezed order
        vc_gc_forward_ckbd writes, the table index of each comes from ``scales`` at its full-resolution position, ``y_hat`` receives
        what vc_gc_dequant_ckbd would write from ``means`` there and keeps the other parity (all three T windows [images, hy, wy, C],
        wy even).  ``symbols_out``: int32 [images, C*hy*wy/2] for tests / traces."""
        count = y_hat.c * y_hat.h * (y_hat.w // 2)
        sym = self._symbols_out(symbols_out, count)
        self._fused("irans decode gc ckbd", 12.0 * self.images * count, lambda: check(lib().vc_irans_decode_gc_ckbd(
            stream(), self.buf.data_ptr(), self.states.data_ptr(), self.images, self.waves, count, tables.struct(), scales.view(), means.view(),
            int(parity), scale_table.data_ptr(), int(scale_table.numel()), None if out_gain is None else out_gain.data_ptr(), y_hat.view(), sym),
            "vc_irans_decode_gc_ckbd"))
        return y_hat

    def finish(self):
        """The one read: VcError when a violation was met or a sub-stream was not consumed to its last word."""
        head = self.states.view(self.images, IRANS_STATE_BYTES)[:, :4 * IRANS_STATE_HEADER_WORDS].cpu().numpy().view(np.uint32)
        for j in range(self.images):
            err = int(head[j, 0])
            if err:
                what = "; ".join(v for k, v in IRANS_ERRORS.items() if err & k)
                raise VcError(f"interleaved range decoder, image {j}: {what} (the symbols behind the violation are zeros)")
            count, cursor = head[j, 2 + 16:2 + 16 + self.waves], head[j, 2 + 32:2 + 32 + self.waves]
            if not np.array_equal(count, cursor):
                raise VcError(f"interleaved range decoder, image {j}: consumed {cursor.tolist()} of {count.tolist()} words")
