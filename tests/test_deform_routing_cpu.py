"""Which k_deform<CG, OG, MODE, VEC, RV, MAXT, XH> every deformable call selects, pinned without a GPU.

vc_deform_select (include/vc_hip.h) is the rule the launcher of csrc/deform.hip follows, as a pure host function.  The whole table --
mode x (cg, og) x groups x x_half x vec x rv -- is compared against tests/golden/deform_routes.json, written by
tools/dump_deform_routes.py from the two launch ladders this function replaced; the rows the GPU tests name in their comments are
spelled out below.  A change that selects another instance, correct but perhaps slower, fails here."""
import importlib.util
import json
import os
import re

import pytest

from vcamd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, OD, PAIR = 0, 1, 2
EINVAL = -1


def _tool():
    spec = importlib.util.spec_from_file_location("dump_deform_routes", os.path.join(ROOT, "tools", "dump_deform_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "deform_routes.json")) as f:
        return json.load(f)


def code(vec, rv, maxt, xh=False):
    """the encoding include/vc_hip.h documents"""
    assert rv in (1, 2, 4) and maxt in (512, 1024)
    return int(vec) | rv << 1 | (maxt == 512) << 4 | int(xh) << 5


def select(mode, cg, og, groups, x_half=0, vec=1, rv=4):
    return hip.lib().vc_deform_select(mode, cg, og, groups, x_half, vec, rv)


def test_declared_with_its_encoding_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "vc_hip.h")).read()
    assert re.search(r"\bint\s+vc_deform_select\s*\(\s*int mode, int cg, int og, int groups, int x_half, int vec, int rv\s*\)\s*;", text)
    assert "VEC | RV << 1 | (MAXT == 512) << 4 | XH << 5" in text
    assert "vc_deform_select" in hip.EXPORTED_SYMBOLS
    assert len(hip.lib().vc_deform_select.argtypes) == 7


def test_table_equals_golden(golden):
    tool = _tool()
    current = json.loads(tool.dumps(tool.build()))
    assert current["axes"] == golden["axes"]
    assert len(golden["routes"]) == 3 * 9 * 9 and all(len(v) == 18 for v in golden["routes"].values())
    wrong = [f"{k}: golden {golden['routes'][k]} != current {current['routes'].get(k)}" for k in golden["routes"]
             if golden["routes"][k] != current["routes"].get(k)]
    assert not wrong, "\n".join(wrong[:20])
    assert current == golden
    codes = {c for v in golden["routes"].values() for c in v}
    # every (VEC, RV, MAXT) without half features, the one half-feature form, and the refusal
    assert codes == {EINVAL, code(1, 4, 512, True)} | {code(v, rv, t) for v in (0, 1) for rv in (1, 2, 4) for t in (512, 1024)}


def test_icip2024_levels():
    """vc_offset_diversity at 16 groups (tests/test_deform_gpu.py): the vector form runs 512 threads with 16- and 4-byte record pieces
    and 1024 with 8-byte ones (there is no <.., true, 2, 512> instance below 144 products per tap); the scalar form always 1024."""
    for cg, og in ((8, 4), (12, 6), (16, 8)):
        assert select(OD, cg, og, 16, vec=1, rv=4) == code(1, 4, 512)
        assert select(OD, cg, og, 16, vec=1, rv=2) == code(1, 2, 1024)
        assert select(OD, cg, og, 16, vec=1, rv=1) == code(1, 1, 512)
        for rv in (4, 2, 1):
            assert select(OD, cg, og, 16, vec=0, rv=rv) == code(0, rv, 1024)
        # half features, pixel-interleaved and group-planar: the fast instance or nothing
        for x_half in (1, 2):
            assert select(OD, cg, og, 16, x_half, vec=1, rv=4) == code(1, 4, 512, True)
            assert select(OD, cg, og, 16, x_half, vec=1, rv=2) == select(OD, cg, og, 16, x_half, vec=0, rv=4) == EINVAL
            assert select(OD, cg, og, 18, x_half, vec=1, rv=4) == EINVAL


def test_more_than_eight_groups_per_reference_and_short_records():
    assert select(OD, 4, 2, 32, vec=1, rv=4) == code(1, 4, 1024) and select(OD, 4, 2, 32, vec=0, rv=1) == code(0, 1, 1024)
    assert select(GENERIC, 8, 4, 8, vec=1) == code(1, 1, 512) and select(GENERIC, 8, 4, 8, vec=0) == code(0, 1, 1024)
    assert select(GENERIC, 4, 2, 32, vec=1) == code(1, 1, 1024)
    # the record length bounds the pieces: 27 * G/2 floats -- G = 4: 54 (pairs), G = 2, 6: odd (single floats), G = 20: 270 (pairs)
    assert select(OD, 8, 4, 4, vec=1, rv=4) == code(1, 2, 1024) and select(OD, 8, 4, 20, vec=1, rv=4) == code(1, 2, 1024)
    assert select(OD, 8, 4, 2, vec=1, rv=4) == select(OD, 8, 4, 6, vec=1, rv=4) == code(1, 1, 512)
    # rv does not exist for the generic mode
    assert {select(GENERIC, 8, 4, 16, vec=1, rv=rv) for rv in (1, 2, 4, 0, 3)} == {code(1, 1, 512)}


def test_deform_pair_half_planar_shapes():
    """vc_deform_pair_hxp (tests/test_deform_pair_half_gpu.py): one instance for each shape of the ICIP2023 model, nothing behind it."""
    for cg in (4, 8, 12):
        assert select(PAIR, cg, cg, 16, 2, vec=1, rv=4) == code(1, 4, 512, True)
        assert select(PAIR, cg, cg, 16, 1, vec=1, rv=4) == EINVAL           # group-planar features only
        assert select(PAIR, cg, cg, 16, 2, vec=1, rv=2) == EINVAL           # no RV < 4 half instance
        assert select(PAIR, cg, cg, 16, 2, vec=0, rv=4) == EINVAL
        assert select(PAIR, cg, cg, 18, 2, vec=1, rv=4) == EINVAL           # at most 8 groups per reference
    assert select(PAIR, 8, 4, 16, 2, vec=1, rv=4) == select(PAIR, 16, 8, 16, 2, vec=1, rv=4) == EINVAL
    assert select(OD, 12, 12, 16, 2, vec=1, rv=4) == EINVAL


def test_twelve_by_twelve_runs_512_threads_only():
    """(12, 12), tests/test_deform_pair_gpu.py: the scalar form spills at 1024 threads, so every instance of the pair has the
    512-thread bound and more than 8 groups per reference are refused."""
    for mode in (GENERIC, OD, PAIR):
        for vec in (0, 1):
            for rv in (1, 2, 4):
                assert select(mode, 12, 12, 16, vec=vec, rv=rv) == code(vec, 1 if mode == GENERIC else rv, 512)
                assert select(mode, 12, 12, 18, vec=vec, rv=rv) == EINVAL
    assert select(PAIR, 8, 8, 16, vec=1, rv=4) == code(1, 4, 512) and select(PAIR, 8, 8, 16, vec=0, rv=4) == code(0, 4, 1024)


def test_refusals():
    assert select(OD, 8, 6, 16) == EINVAL                                   # (cg, og) without an instance
    for groups in (0, 1, 3, 15, 34, -2):
        assert select(OD, 8, 4, groups) == EINVAL, groups
    assert select(GENERIC, 8, 4, 16, 1) == select(GENERIC, 8, 4, 16, 2) == EINVAL      # half features: fused entries only
    assert select(3, 8, 4, 16) == select(-1, 8, 4, 16) == select(OD, 8, 4, 16, 3) == select(OD, 8, 4, 16, rv=3) == EINVAL
