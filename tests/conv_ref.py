"""Float64 reference of the whole vc_conv_desc contract (include/vc_hip.h), with the two tensors the acceptance bar of
tests/test_conv_gpu.py needs.  Plain torch on the CPU: no code of vcamd or of oracle/ is used here, and the convolution itself is a
loop over the taps (one float64 matrix product per tap), not F.conv2d -- tests/test_conv_cpu.py holds it against the torch operator
chain.

    acc = conv(xform(x), w, stride, pad k//2) + bias        xform = identity | square
    v   = GDN:  mul / sqrt(acc)   IGDN: mul * sqrt(acc)     (no activation with these)
          else: res_first ? act(acc + res) : act(acc)       act = none | relu | lrelu(slope) | sigmoid | clamp01
    v   = v * chscale                                       per ORIGINAL output channel, before the shuffle
    v   = pixel_shuffle(v, 2) if requested
    out = v + res   (unless res_first)                      res laid out like the (shuffled) output

Channel gain with pixel shuffle.  The row above is the documented order (gain per output channel of the convolution, then the
shuffle).  The library does something else: vc_conv_pack_weights moves original channel c * 4 + pos to packed channel
pos * cout/4 + c, and every epilogue (conv_epilogue of csrc/conv_mfma.h and its coalesced, LDS-DMA and split-operand twins) reads
chscale at the PACKED index, so a gain vector given in the original order lands on the wrong channels; a caller would have to
permute it like the bias.  No caller does either: the only gains are final_chscale of vcamd.layers.run_sequential (the last, stride-2
layers of g_a / h_a in vcamd/layers.py and vcamd/icip2024.py), never on a pixel-shuffle layer, and the existing tests leave the
combination out as well.  The library's behaviour there is an accident of the packing, so the GPU module tests gain on plain outputs
only; this reference implements the documented row and tests/test_conv_cpu.py checks it against F.pixel_shuffle.

mag = conv(|xform(x)|, |w|) + |bias|: sum |a b| of the accumulator, the measure tests/test_split_gpu.py uses.
lip = a bound on |d out / d acc| per element: 1 for none / ReLU / LeakyReLU (slope <= 1) / clamp, 1/4 for sigmoid, |mul| / (2 acc^1.5)
for GDN, |mul| / (2 sqrt(acc)) for IGDN, each times |chscale|.  Lipschitz constants: the ReLU kink and the clamp corners need no
exclusion.  Both are returned in the layout of ``out`` (shuffled where it is)."""
import collections
import functools

import torch

Ref = collections.namedtuple("Ref", "out mag lip acc")
ACC_BOUND = 6e-7                 # fp32 accumulator error over sum |a b| (asserted by tests/test_split_gpu.py)
ROUNDINGS = 4 * 2.0 ** -23       # expf, sqrtf, the divide and the final roundings, relative to |ref|
HALF_STORE = 2.0 ** -11          # a result stored as half, relative to |ref|


def conv64(x, w, stride=1):
    """sum over taps of x_shifted @ w_tap in float64; "same" padding k // 2 (the only one the engine has)"""
    x, w = x.double(), w.double()
    n, cin, h, wd = x.shape
    cout, _, k, _ = w.shape
    p = k // 2
    ho, wo = (h + 2 * p - k) // stride + 1, (wd + 2 * p - k) // stride + 1
    xp = torch.zeros(n, h + 2 * p, wd + 2 * p, cin, dtype=torch.float64)
    xp[:, p:p + h, p:p + wd] = x.permute(0, 2, 3, 1)
    acc = torch.zeros(n, ho, wo, cout, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            tap = xp[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride]
            acc += tap @ w[:, :, ky, kx].t()
    return acc.permute(0, 3, 1, 2).contiguous()


def shuffle2(v):
    """nn.PixelShuffle(2): channel c * 4 + dy * 2 + dx of pixel (y, x) -> channel c of pixel (2 y + dy, 2 x + dx)"""
    n, c4, h, w = v.shape
    c = c4 // 4
    return v.view(n, c, 2, 2, h, w).permute(0, 1, 4, 2, 5, 3).reshape(n, c, 2 * h, 2 * w)


def reference(x, w, bias, stride=1, act="none", slope=0.01, square=False, epi="none", mul=None, res=None, res_first=False,
              chscale=None, shuffle=False):
    """-> Ref(out, mag, lip, acc), all float64 NCHW; out / mag / lip in the layout of the output, acc of the convolution."""
    if epi != "none" and (act != "none" or mul is None):
        raise ValueError("GDN / IGDN take a multiplier and no activation")
    if res_first and (res is None or epi != "none" or act in ("sigmoid", "clamp01") or shuffle):
        raise ValueError("res_first: a residual in front of none / ReLU / LeakyReLU, laid out like the accumulator")
    xx = x.double() ** 2 if square else x.double()
    b = torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else bias.double()
    acc = conv64(xx, w, stride) + b.view(1, -1, 1, 1)
    mag = conv64(xx.abs(), w.double().abs(), stride) + b.abs().view(1, -1, 1, 1)
    lip = torch.ones_like(acc)
    if epi == "gdn":
        m = mul.double()
        v, lip = m / acc.sqrt(), m.abs() / (2 * acc ** 1.5)
    elif epi == "igdn":
        m = mul.double()
        v, lip = m * acc.sqrt(), m.abs() / (2 * acc.sqrt())
    else:
        v = acc + res.double() if res_first else acc
        if act == "relu":
            v = torch.where(v >= 0, v, torch.zeros_like(v))
        elif act == "lrelu":
            if not 0 <= slope <= 1:
                raise ValueError("lip = 1 needs a slope in [0, 1]")
            v = torch.where(v >= 0, v, v * slope)
        elif act == "sigmoid":
            v, lip = 1 / (1 + torch.exp(-v)), lip * 0.25
        elif act == "clamp01":
            v = v.clamp(0, 1)
        elif act != "none":
            raise ValueError(act)
    if chscale is not None:
        g = chscale.double().view(1, -1, 1, 1)
        v, lip = v * g, lip * g.abs()
    if shuffle:
        v, mag, lip = shuffle2(v), shuffle2(mag), shuffle2(lip)
    if res is not None and not res_first:
        v = v + res.double()
    return Ref(v, mag, lip, acc)


def allowance(ref, half_out=False):
    """the acceptance bar of tests/test_conv_gpu.py, per element"""
    return ref.lip * ACC_BOUND * ref.mag + (ROUNDINGS + (HALF_STORE if half_out else 0.0)) * ref.out.abs()


def worst_ratio(out, ref, half_out=False):
    """max |out - ref| / allowance (an element whose allowance is 0 must be exact)"""
    err, allow = (out.double() - ref.out).abs(), allowance(ref, half_out)
    assert torch.isfinite(out).all(), "NaN / inf in the output window"
    r = torch.where(err == 0, torch.zeros_like(err), err / allow.clamp_min(1e-300))
    return float(r.max())


# ---- epilogue forms (names used as test ids) ----
# kind: which inputs the form needs -- "plain": accumulators of about unit size; "wide": accumulators spread over about +-6 and around
# 0 and 1 (both saturations of the sigmoid, both corners of the clamp); "gdn": cin == cout, gamma >= 0, beta >= 0.5
EPILOGUES = {
    "none": dict(),
    "relu": dict(act="relu"),
    "lrelu.01": dict(act="lrelu", slope=0.01),
    "lrelu.2": dict(act="lrelu", slope=0.2),
    "sigmoid": dict(act="sigmoid", kind="wide"),
    "clamp01": dict(act="clamp01", kind="wide"),
    "gain": dict(act="lrelu", slope=0.01, gain=True),
    "res": dict(act="relu", res=True),
    "gain+res": dict(act="lrelu", slope=0.2, gain=True, res=True),
    "sigmoid+gain+res": dict(act="sigmoid", kind="wide", gain=True, res=True),
    "resfirst-none": dict(res=True, res_first=True),
    "resfirst-relu": dict(act="relu", res=True, res_first=True),
    "resfirst-lrelu": dict(act="lrelu", slope=0.2, res=True, res_first=True, gain=True),
    "square": dict(square=True, act="lrelu", slope=0.01),
    "gdn": dict(square=True, epi="gdn", mul=True, kind="gdn"),
    "gdn+res": dict(square=True, epi="gdn", mul=True, res=True, kind="gdn"),
    "igdn+res": dict(square=True, epi="igdn", mul=True, res=True, kind="gdn"),
}


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


@functools.lru_cache(maxsize=None)
def inputs(cin, cout, k, stride, n, h, w, shuffle=False, kind="plain", half_exact=False, seed=0):
    """-> dict x, w, b, res, mul, gain (float32 CPU tensors, NCHW / OIHW).  res is laid out like the output (shuffled where it is),
    mul like the accumulator.  gain: mixed signs, magnitudes 0.01 .. 3 (the range of the calibrated checkpoint).  half_exact:
    x, w and res survive .half().float() unchanged (the fp16 instances then multiply exactly what the reference multiplies)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * cin + 13 * cout + k + (50 if kind != "plain" else 0))
    x = _randn(g, n, cin, h, w)
    fan = cin * k * k
    if kind == "gdn":
        if cin != cout or k != 1:
            raise ValueError("a GDN layer is a 1 x 1 contraction C -> C")
        wt = (0.1 * torch.eye(cin) + 0.004 * torch.rand(cin, cin, generator=g)).view(cout, cin, 1, 1)
        b = 0.5 + torch.rand(cout, generator=g)
        x = 2.0 * x
    else:
        wt = _randn(g, cout, cin, k, k) * ((3.0 if kind == "wide" else 1.0) / fan ** 0.5)
        b = _randn(g, cout) * 0.1 + (0.5 if kind == "wide" else 0.0)
    p = k // 2
    ho, wo = (h + 2 * p - k) // stride + 1, (w + 2 * p - k) // stride + 1
    res = _randn(g, n, cout // 4, 2 * ho, 2 * wo) if shuffle else _randn(g, n, cout, ho, wo)
    mul = x if kind == "gdn" else _randn(g, n, cout, ho, wo)
    mag = torch.exp(torch.rand(cout, generator=g) * (torch.log(torch.tensor(3.0 / 0.01)))) * 0.01
    sign = torch.where(torch.rand(cout, generator=g) < 0.5, -1.0, 1.0)
    gain = mag * sign
    if half_exact:
        x, wt, res = x.half().float(), wt.half().float(), res.half().float()
        mul = x if kind == "gdn" else mul
    return dict(x=x, w=wt, b=b, res=res, mul=mul, gain=gain)


def reference_of(ins, form, stride=1, shuffle=False):
    """the reference of one named epilogue form on inputs()"""
    f = EPILOGUES[form]
    return reference(ins["x"], ins["w"], ins["b"], stride=stride, act=f.get("act", "none"), slope=f.get("slope", 0.01),
                     square=f.get("square", False), epi=f.get("epi", "none"), mul=ins["mul"] if f.get("mul") else None,
                     res=ins["res"] if f.get("res") else None, res_first=f.get("res_first", False),
                     chscale=ins["gain"] if f.get("gain") else None, shuffle=shuffle)
