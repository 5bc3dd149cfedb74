"""Which kernel every convolution asks the library for, pinned without a GPU.

Three parts: the names and the split geometry of vcamd/hip.py against the C side; the route table -- every layer shape of the three
families x precision regime x tensor format x call variant -> the descriptor handed to vc_conv2d_nhwc (or the VcError) --; whole-frame
traces (ordered launches of one forward per family).  The last two compare against tests/golden/conv_routes.json, written by
tools/dump_conv_routes.py, which observes the library boundary only: a change of how PackedConv decides must reproduce the file."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from vcamd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("dump_conv_routes", os.path.join(ROOT, "tools", "dump_conv_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "conv_routes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def current():
    """the same document from the code under test (one run shared by the comparisons)"""
    return json.loads(_tool().dumps(_tool().build()))


def _header_enum():
    """VC_CFG_<NAME> = <int> entries of the tile-configuration enum of include/vc_hip.h"""
    text = open(os.path.join(ROOT, "include", "vc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {name: int(val) for name, val in re.findall(r"\bVC_CFG_([A-Z0-9]+)\s*=\s*(\d+)", text)}


def test_configuration_names_equal_the_header():
    enum = _header_enum()
    assert sorted(enum.values()) == list(range(11)), enum
    for name, val in enum.items():
        assert getattr(hip, "CFG_" + name) == val, name
    defines = dict(re.findall(r"#define\s+VC_CFG_([A-Z0-9_]+)\s+(0x[0-9a-fA-F]+)", open(os.path.join(ROOT, "include", "vc_hip.h")).read()))
    assert len(defines) >= 10
    for name, val in defines.items():
        assert getattr(hip, "CFG_" + name) == int(val, 16), name


def test_split_geometry_equals_the_c_side():
    """split_geometry says "served" exactly where the library has a split instance to pack (vc_conv_packed_weight_bytes_split > 0 and
    vc_conv_pack_weights_split == VC_OK on zero weights, which take neither a stride nor refuse a pixel shuffle), and its chunk is
    vc_conv_chunk(VC_CFG_SPLIT).  PackedConv narrows that by policy only: stride 1, no pixel-shuffled 5x5 / 7x7 layer."""
    L = hip.lib()
    served = 0
    for k in (1, 3, 5, 7):
        for cout in (2, 12, 16, 32, 48, 64, 96, 128, 512):
            for cin in (3, 6, 8, 16, 19, 32, 64, 128):
                g = hip.split_geometry(k, cout, cin)
                assert g.cin_split % 8 == 0 and 0 <= g.cin_split - cin < g.chunk
                nbytes = L.vc_conv_packed_weight_bytes_split(cout, g.cin_split, k)
                for ps in ((0, 1) if cout % 4 == 0 else (0,)):
                    w = np.zeros((cout, g.cin_split, k, k), dtype=np.float32)
                    wpk, b = np.zeros(max(nbytes, 2) // 2, dtype=np.int16), np.zeros(cout, dtype=np.float32)
                    rc = L.vc_conv_pack_weights_split(w.ctypes.data, None, cout, g.cin_split, k, ps, wpk.ctypes.data, b.ctypes.data)
                    assert g.served == (nbytes > 0 and rc == hip.VC_OK), (k, cout, cin, ps, nbytes, rc)
                if g.served:
                    served += 1
                    assert g.chunk == L.vc_conv_chunk(hip.CFG_SPLIT, k, 1, cin) == 8 * g.cpl
                    assert g.bn == 16 * g.ntw and cout % g.bn == 0
                    assert L.vc_conv_chunk(hip.CFG_SPLIT, k, 2, cin) == -1
                for stride in (1, 2):
                    for ps in ((False, True) if cout % 4 == 0 else (False,)):
                        pc = hip.PackedConv(torch.zeros(cout, cin, k, k), None, stride=stride, pixelshuffle=ps, device="cpu")
                        assert pc.cin_split == g.cin_split
                        assert pc.split_ok == (g.served and stride == 1 and not (ps and k != 3) and pc.wpk16 is None), (k, cout, cin, stride, ps)
    assert served > 100


def test_route_decides_without_touching_the_library():
    """_route allocates nothing and launches nothing; __call__ then makes exactly the launch the route names."""
    tool = _tool()
    with tool.recording() as rec:
        hip.set_conv_precision("fp32")
        hip.set_fp32_mode("split")
        pc = tool.make_pc(3, 128, 128, 1, 0)
        x = hip.T.empty(*tool.LARGE, 128, "cpu")
        pc.split_pack()
        del rec.events[:]
        r = pc._route(x, act=hip.ACT_LRELU, out_sp3=True)
        assert rec.events == []
        assert r.split and r.out_dtype == "sp3" and r.cfg == hip.CFG_SPLIT | hip.CFG_EXACT | hip.CFG_IN_SP3 | hip.CFG_OUT_SP3 and r.key is None
        out = pc(x, act=hip.ACT_LRELU, out_sp3=True)
        assert [name for name, _ in rec.events] == ["vc_split3", "vc_conv2d_nhwc"]
        assert rec.events[1][1][1]._obj.cfg == r.cfg and out.dtype == "sp3"
        small = hip.T.empty(*tool.SMALL, 128, "cpu")
        r = pc._route(small, res=hip.T.empty(*tool.SMALL, 128, "cpu"), res_first=True)
        assert not r.split and r.cfg is None and r.flags == hip.CFG_RES_FIRST and r.key == (*tool.SMALL, hip.CFG_RES_FIRST)
    assert not isinstance(hip.lib(), tool.Recorder)


def _diff(want, got, path=""):
    """paths at which two JSON documents differ (first few: the assertion message names the layer and the call)"""
    if isinstance(want, dict) and isinstance(got, dict):
        out = []
        for key in sorted(set(want) | set(got)):
            if key not in want or key not in got:
                out.append(f"{path}/{key}: only in {'golden' if key in want else 'current'}")
            else:
                out += _diff(want[key], got[key], f"{path}/{key}")
        return out
    return [] if want == got else [f"{path}: golden {want!r} != current {got!r}"]


def _resolved(table):
    """route table with the row indexes replaced by the rows"""
    rows = table["rows"]

    def walk(v):
        if isinstance(v, dict):
            return {k: ({n: rows[i] for n, i in x.items()} if k.startswith(("routes", "tuner")) else walk(x)) for k, x in v.items()}
        return v
    return walk(table["layers"])


def test_route_table_equals_golden(golden, current):
    want, got = _resolved(golden["route_table"]), _resolved(current["route_table"])
    assert len(golden["route_table"]["rows"]) >= 200 and len(want) >= 17
    d = _diff(want, got)
    assert not d, "\n".join(d[:20])


def test_frame_traces_equal_golden(golden, current):
    def resolved(fr):
        return {name: [fr["events"][i] for i in ids] for name, ids in fr["traces"].items()}
    want, got = resolved(golden["frames"]), resolved(current["frames"])
    assert len(want) == 7 and all(len(v) > 10 for v in want.values())
    for name in want:
        assert name in got, name
        assert len(want[name]) == len(got[name]), (name, len(want[name]), len(got[name]))
        for i, (a, b) in enumerate(zip(want[name], got[name])):
            assert a == b, (name, i, a, b)
    assert golden == current
