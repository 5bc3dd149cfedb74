#!/usr/bin/env python3
"""Write tests/golden/conv_routes.json: what every convolution of the three model families asks the library for.

No GPU: ``vc_*`` launches are replaced by a recorder that returns VC_OK (host-side packing still goes to the real library),
tensors live on the CPU device and are never read.  The script observes the LIBRARY BOUNDARY only -- descriptors handed to
vc_conv2d_nhwc, the order of entry points, the profiler's bookkeeping in hip.kernel_symbols / hip.split_keys -- so it gives the
same file before and after a change of how PackedConv decides; tests/test_conv_routing_cpu.py compares against it.

    python tools/dump_conv_routes.py [--out tests/golden/conv_routes.json]
"""
import argparse
import contextlib
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-compression_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vcamd import hip  # noqa: E402

# entry points that run on the host (weight packing, table construction, the range coder): never stubbed
HOST = {"vc_version", "vc_abi_version", "vc_target_arch", "vc_conv_select_cfg", "vc_conv_chunk", "vc_conv_packed_weight_floats",
        "vc_conv_packed_bias_floats", "vc_conv_pack_weights", "vc_conv_packed_weight_bytes_f16", "vc_conv_pack_weights_f16",
        "vc_conv_pack_tail_f16", "vc_conv_packed_weight_bytes_split", "vc_conv_pack_weights_split", "vc_deform_pack_weights", "vc_deform_select",
        "vc_bits_slots", "vc_msssim_workspace_bytes", "vc_pmf_to_quantized_cdf", "vc_rans_bound", "vc_rans_encode_with_indexes",
        "vc_rans_decode_with_indexes", "vc_rans_decode_stream"}

SMALL, LARGE = (1, 34, 60), (2, 128, 256)          # split_pays is false at the first for every layer, true at the second
MODES = (("fp32", "native"), ("fp32", "split"), ("fp16", "native"))
# (k, cin, cout, stride, pixel shuffle): SPyNet, the mask / flow U-Nets, the hyperprior codecs, the ELIC blocks
LAYERS = [(7, 8, 32, 1, 0), (7, 32, 64, 1, 0), (7, 64, 32, 1, 0), (7, 32, 16, 1, 0), (7, 16, 2, 1, 0),
          (5, 6, 32, 1, 0), (5, 32, 64, 1, 0), (5, 32, 1, 1, 0),
          (3, 128, 128, 1, 0), (3, 128, 128, 2, 0), (3, 3, 128, 2, 0), (3, 128, 12, 1, 1), (3, 128, 512, 1, 1), (3, 64, 64, 1, 0),
          (1, 128, 128, 1, 0), (1, 3, 128, 2, 0), (1, 64, 64, 1, 0)]


def layer_name(k, cin, cout, stride, ps):
    return f"k{k} s{stride} {cin}->{cout}" + (" ps" if ps else "")


class Recorder:
    """Stands in for the ctypes library: launches are recorded and answer VC_OK, host-side entry points pass through."""

    def __init__(self, real):
        self.real, self.events = real, []

    def __getattr__(self, name):
        f = getattr(self.real, name)
        if name in HOST or not name.startswith("vc_"):
            return f

        def stub(*args):
            self.events.append((name, args))
            return hip.VC_OK
        return stub


class StubTimer:
    """hip.timer without events: runs the launch, keeps the accounting it was handed."""

    def __init__(self):
        self.items = []

    def bracket(self, key, flops, launch, nbytes=0.0):
        self.items.append((key, flops, nbytes))
        return launch()


class _Event:
    def __init__(self, enable_timing=False):
        pass

    def record(self):
        pass

    def synchronize(self):
        pass

    def elapsed_time(self, other):
        return 1.0


@contextlib.contextmanager
def recording():
    """The library behind a Recorder, no stream, no tuner; everything this script changes in vcamd is put back on exit."""
    from vcamd import flex, icip2024, lhbdc
    keep = (hip._lib, hip.stream, hip.AUTOTUNE, hip.timer, hip.conv_precision(), hip.fp32_mode(), hip.rans_decode, lhbdc._require_cuda,
            dict(hip.kernel_symbols), set(hip.split_keys))
    rec = Recorder(hip.lib())
    hip._lib, hip.stream, hip.AUTOTUNE, hip.timer = rec, (lambda: None), False, None
    lhbdc._require_cuda = flex._require_cuda = icip2024._require_cuda = lambda x: None     # (the frames are CPU tensors here)
    try:
        yield rec
    finally:
        hip._lib, hip.stream, hip.AUTOTUNE, hip.timer = keep[:4]
        hip.set_conv_precision(keep[4])
        hip.set_fp32_mode(keep[5])
        hip.rans_decode = keep[6]
        lhbdc._require_cuda = flex._require_cuda = icip2024._require_cuda = keep[7]
        hip.kernel_symbols.clear(), hip.kernel_symbols.update(keep[8])
        hip.split_keys.clear(), hip.split_keys.update(keep[9])


def conv_row(d):
    """the descriptor fields a route is made of"""
    s = f"cfg={d.cfg:#x} k{d.kh} s{d.stride} act{d.act} epi{d.epi} xf{d.in_xform} om{d.out_mode}"
    s += " " + "".join(ch if getattr(d, f) else "-" for ch, f in (("R", "res"), ("M", "mul"), ("C", "chscale"), ("T", "tail_wpk")))
    if d.res:
        # fp32 / half residuals: strides in elements of a dense window; split residuals: the image distance in bytes, 0, 0
        s += f" rs={d.res_sn},{d.res_sh},{d.res_sw}"
    return s


def t_row(t):
    return f"{t.dtype} {t.n}x{t.h}x{t.w}x{t.c}"


# ------------------------------------------------------------------------------------------------------------------------
# route table
# ------------------------------------------------------------------------------------------------------------------------
def make_pc(k, cin, cout, stride, ps, seed=0):
    g = torch.Generator().manual_seed(seed)
    return hip.PackedConv(torch.randn(cout, cin, k, k, generator=g) * 0.05, torch.randn(cout, generator=g) * 0.1, stride=stride,
                          pixelshuffle=bool(ps), device="cpu")


def variants(pc, size, tail):
    """name -> a function that makes the call (operands are allocated inside: a refused allocation is part of the record)"""
    n, h, w = size
    ho, wo, co = pc.out_shape(h, w)
    E = hip.T.empty

    def x(dt="f32"):
        return E(n, h, w, pc.cin_split if dt == "sp3" else pc.cin, "cpu", dt)

    def o(dt="f32"):
        return E(n, ho, wo, co, "cpu", dt)
    lrelu = dict(act=hip.ACT_LRELU, slope=0.1)
    v = {"plain": lambda: pc(x()),
         "in f16": lambda: pc(x("f16"), **lrelu),
         "in sp3": lambda: pc(x("sp3"), **lrelu),
         "lrelu": lambda: pc(x(), **lrelu),
         "sigmoid": lambda: pc(x(), act=hip.ACT_SIGMOID),
         "out_sp3": lambda: pc(x(), out_sp3=True, **lrelu),
         "out_f16": lambda: pc(x(), out_f16=True, **lrelu),
         "in f16 out_f16": lambda: pc(x("f16"), out_f16=True, **lrelu),
         "in sp3 out_sp3": lambda: pc(x("sp3"), out_sp3=True, **lrelu),
         "in sp3 out_f16": lambda: pc(x("sp3"), out_f16=True),
         "chscale": lambda: pc(x(), chscale=torch.ones(pc.cout)),
         "out slice": lambda: pc(x(), out=E(n, ho, wo, co + 3, "cpu").channels(1, 1 + co), **lrelu),
         "in slice": lambda: pc(E(n, h, w, pc.cin + 3, "cpu").channels(1, 1 + pc.cin), **lrelu)}
    for dt in ("f32", "f16", "sp3"):
        v[f"out {dt}"] = lambda dt=dt: pc(x(), out=o(dt), **lrelu)
        v[f"res {dt}"] = lambda dt=dt: pc(x(), res=o(dt), **lrelu)
        v[f"res {dt} first"] = lambda dt=dt: pc(x(), res=o(dt), res_first=True, act=hip.ACT_RELU)
        v[f"in {dt} res {dt}"] = lambda dt=dt: pc(x(dt), res=o(dt), **lrelu)
    v["in f16 out f16"] = lambda: pc(x("f16"), out=o("f16"))
    v["in sp3 out sp3 res sp3"] = lambda: pc(x("sp3"), out=o("sp3"), res=o("sp3"), **lrelu)
    v["res f32 out_sp3"] = lambda: pc(x(), res=o(), out_sp3=True)
    v["res slice"] = lambda: pc(x(), res=E(n, ho, wo, co + 3, "cpu").channels(1, 1 + co))
    if pc.k == 1 and pc.cin == pc.cout and pc.stride == 1:         # the layer as a GDN / IGDN contraction (layers.GDN.run)
        for name, epi in (("gdn", hip.EPI_GDN), ("igdn", hip.EPI_IGDN)):
            def gdn(epi=epi, **kw):
                t = x()
                return pc(t, epi=epi, mul=t, in_xform=hip.IN_SQUARE, **kw)
            v[name] = gdn
            v[f"{name} res f32"] = lambda gdn=gdn: gdn(res=o())
            v[f"{name} out_sp3"] = lambda gdn=gdn: gdn(res=o(), out_sp3=True)
            v[f"{name} out_f16"] = lambda gdn=gdn: gdn(res=o(), out_f16=True)
            v[f"{name} out f16"] = lambda gdn=gdn: gdn(out=o("f16"))
            v[f"{name} res f16"] = lambda gdn=gdn: gdn(res=o("f16"))
    if tail is not None:                                            # the 1x1 layer behind this 3x3 layer, in one launch
        v["tail"] = lambda: pc(x(), tail=tail, **lrelu)
        v["tail in f16"] = lambda: pc(x("f16"), tail=tail, **lrelu)
        v["tail in f16 res f16 out_f16"] = lambda: pc(x("f16"), tail=tail, res=o("f16"), out_f16=True, **lrelu)
        v["tail in f16 res f32"] = lambda: pc(x("f16"), tail=tail, res=o())
        v["tail in f16 sigmoid"] = lambda: pc(x("f16"), tail=tail, act=hip.ACT_SIGMOID)
    return v


def drive(rec, call):
    """one call of a layer -> one row: the descriptor(s) that reached the library and the result, or the error"""
    del rec.events[:]
    hip.timer = StubTimer()
    hip.split_keys.clear()
    hip.kernel_symbols.clear()
    try:
        out = call()
    except hip.VcError as e:
        return "VcError: " + str(e)
    finally:
        timer, hip.timer = hip.timer, None
    parts = []
    for name, args in rec.events:
        parts.append(conv_row(args[1]._obj) if name == "vc_conv2d_nhwc" else name)
    parts.append("-> " + t_row(out))
    for key, flops, nbytes in timer.items:
        parts.append(f"[{key}] flops={flops:.0f} bytes={nbytes:.0f} sym={hip.kernel_symbols.get(key)}" + (" split" if key in hip.split_keys else ""))
    return " | ".join(parts)


def tuner_candidates(rec, call):
    """The configurations the tuner would time for this call, in order: with the tuner on, every candidate its filter leaves is
    launched through the library (each answers VC_OK in 1 ms, so the first one is kept)."""
    del rec.events[:]
    keep = torch.cuda.Event, torch.cuda.is_current_stream_capturing
    torch.cuda.Event, torch.cuda.is_current_stream_capturing = _Event, lambda: False
    hip.AUTOTUNE = True
    try:
        call()
    except hip.VcError as e:
        return "VcError: " + str(e)
    finally:
        hip.AUTOTUNE = False
        torch.cuda.Event, torch.cuda.is_current_stream_capturing = keep
    seen = []
    for name, args in rec.events:
        if name == "vc_conv2d_nhwc" and f"{args[1]._obj.cfg:#x}" not in seen:
            seen.append(f"{args[1]._obj.cfg:#x}")
    return " ".join(seen)


def route_table(rec):
    rows, index = [], {}

    def ref(row):
        if row not in index:
            index[row] = len(rows)
            rows.append(row)
        return index[row]
    layers = {}
    for precision, mode in MODES:
        hip.set_conv_precision(precision)
        hip.set_fp32_mode(mode)
        mname = precision if precision == "fp16" else f"{precision}/{mode}"
        tail = make_pc(1, 64, 64, 1, 0, seed=1)
        for spec in LAYERS:
            pc = make_pc(*spec)
            entry = layers.setdefault(layer_name(*spec), {})
            e = entry[mname] = {"cfg": pc.cfg, "candidates": list(pc.candidates), "cin_split": pc.cin_split, "split_ok": bool(pc.split_ok),
                                "dma_f32": bool(pc.dma_f32), "half_ok": bool(pc.half_ok), "half_res_ok": bool(pc.half_res_ok),
                                "split_pays": [bool(pc.split_pays(*SMALL)), bool(pc.split_pays(*LARGE))]}
            with_tail = tail if spec == (3, 64, 64, 1, 0) else None
            e["can_fuse_tail"] = bool(pc.can_fuse_tail(tail))
            for size in (SMALL, LARGE):
                e["routes @%dx%dx%d" % size] = {name: ref(drive(rec, call)) for name, call in variants(pc, size, with_tail).items()}
                pc.tuned = {}
            # the tuner's filtered candidate list per flag word (fresh layer per call: nothing tuned yet)
            tuned = {}
            for name in ("plain", "in f16", "out_sp3", "out_f16", "in f16 out_f16", "res f32 first", "res f16", "in f16 res f16", "sigmoid",
                         "gdn", "gdn out_sp3", "out slice"):
                pc = make_pc(*spec)
                v = variants(pc, LARGE, None)
                if name in v:
                    tuned[name] = ref(tuner_candidates(rec, v[name]))
            e["tuner @%dx%dx%d" % LARGE] = tuned
    return {"rows": rows, "layers": layers}


# ------------------------------------------------------------------------------------------------------------------------
# whole-frame traces
# ------------------------------------------------------------------------------------------------------------------------
def frame_events(rec):
    """ordered (symbol, configuration word and shape for convolutions, output dtype)"""
    out = []
    for name, args in rec.events:
        if name != "vc_conv2d_nhwc":
            out.append(name)
            continue
        d = args[1]._obj
        dt = "sp3" if d.cfg & hip.CFG_OUT_SP3 else ("f16" if d.cfg & hip.CFG_OUT_F16 else "f32")
        out.append(f"conv {d.cfg:#x} k{d.kh} s{d.stride} {d.inp.c}->{d.out.c} @{d.inp.n}x{d.inp.h}x{d.inp.w} {dt}")
    return out


def int_args(args):
    """integer / float / view arguments of a call; addresses only as set or null"""
    out = []
    for a in args:
        if isinstance(a, hip.View):
            out.append([a.n, a.h, a.w, a.c, a.sn, a.sh, a.sw] if a.p else "null view")
        elif isinstance(a, hip.RefineLayer):
            out.append(["layer", a.k, a.stride, a.c0])
        elif a is None or isinstance(a, ctypes.c_void_p):
            out.append("null")
        elif isinstance(a, float):
            out.append(repr(a))
        elif isinstance(a, int):
            out.append(a if abs(a) < (1 << 20) else "ptr")
        elif hasattr(a, "_obj"):
            out.append(conv_row(a._obj))
        else:
            out.append(type(a).__name__)
    return out


def compact(seqs):
    """{name: [strings]} -> a table of distinct strings and index lists"""
    table, index, out = [], {}, {}
    for name, seq in seqs.items():
        ids = []
        for s in seq:
            s = s if isinstance(s, str) else json.dumps(s)
            if s not in index:
                index[s] = len(table)
                table.append(s)
            ids.append(index[s])
        out[name] = ids
    return {"events": table, "traces": out}


def frame_traces(rec):
    from vcamd import flex, icip2024, lhbdc
    from vcamd.seeding import seeded_state_dict
    h, w = 128, 192
    g = torch.Generator().manual_seed(3)
    xb, xc, xa = (torch.rand(1, 3, h, w, generator=g) for _ in range(3))
    seqs = {}

    def run(name, make, call):
        model = make()
        model.load_state_dict(seeded_state_dict(model.state_dict(), seed=1234))
        model.eval()
        del rec.events[:]
        with torch.no_grad():
            call(model)
        seqs[name] = frame_events(rec)
        return model
    for mode in ("native", "split"):
        hip.set_conv_precision("fp32")
        hip.set_fp32_mode(mode)
        run(f"lhbdc forward fp32/{mode}", lhbdc.Model, lambda m: m(xb, xc, xa, False))
        run(f"flex forward fp32/{mode}", flex.BidirFlowRef, lambda m: m(xb, xc, xa, n=[2], l=1))
    hip.set_fp32_mode("split")
    for precision in ("fp32", "fp16"):
        hip.set_conv_precision(precision)
        run(f"icip2024 forward {precision}", icip2024.FlowGuidedB, lambda m: m(xb, xa, 0.5, 0.5, xc, 1, 2))
    hip.set_conv_precision("fp32")

    # one decompress_t of a hyperprior codec, the host coder stubbed to symbols of zeros: entry points and their integer arguments
    hip.rans_decode = lambda data, indexes, cdfs, cdf_sizes, offsets: np.zeros(len(indexes), dtype=np.int32)
    codec = lhbdc.ResidualCompressor()
    codec.load_state_dict(seeded_state_dict(codec.state_dict(), seed=1234))
    codec.eval()
    codec.update(force=True)
    del rec.events[:]
    with torch.no_grad():
        codec.decompress_t([[b""], [b""]], (2, 3), "cpu", trace={})
    seqs["lhbdc residual decompress_t"] = [[name] + int_args(args) for name, args in rec.events]
    return compact(seqs)


def build():
    with recording() as rec:
        return {"route_table": route_table(rec), "frames": frame_traces(rec)}


def dumps(doc):
    """one line per leaf mapping / list: a diff of the file names the layer and the call that changed"""
    def enc(v, depth):
        if isinstance(v, dict) and depth < 4 and any(isinstance(x, (dict, list)) for x in v.values()):
            pad = " " * (depth + 1)
            return "{\n" + ",\n".join(f"{pad}{json.dumps(k)}: {enc(x, depth + 1)}" for k, x in v.items()) + "\n" + " " * depth + "}"
        if isinstance(v, list) and v and isinstance(v[0], str):
            pad = " " * (depth + 1)
            return "[\n" + ",\n".join(pad + json.dumps(x) for x in v) + "\n" + " " * depth + "]"
        return json.dumps(v)
    return enc(doc, 0) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv_routes.json"))
    a = ap.parse_args()
    with open(a.out, "w") as f:
        f.write(dumps(build()))
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
