#!/usr/bin/env python3
"""Write tests/golden/deform_routes.json: which k_deform instance every deformable call selects.

No GPU: vc_deform_select (include/vc_hip.h) is a pure host function -- the rule the launcher of csrc/deform.hip follows, asked
for every combination of the axes below.  tests/test_deform_routing_cpu.py compares the library against the file, so a change of
the launcher that picks another instance -- correct, but perhaps slower -- fails a test that needs no device.

    python tools/dump_deform_routes.py [--out tests/golden/deform_routes.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-compression_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from vcamd import hip  # noqa: E402

MODES = {"generic": 0, "od": 1, "pair": 2}
# the eight (cg, og) pairs the library serves and one it does not
SHAPES = [(4, 2), (4, 4), (8, 4), (8, 8), (12, 6), (12, 12), (16, 4), (16, 8), (8, 6)]
GROUPS = [2, 3, 4, 6, 8, 16, 18, 32, 34]
X_HALF, VEC, RV = [0, 1, 2], [0, 1], [1, 2, 4]


def build():
    """{"axes": ..., "routes": {"<mode> <cg> <og> g<groups>": [code for x_half in X_HALF for vec in VEC for rv in RV]}}"""
    L = hip.lib()
    routes = {}
    for mname, mode in MODES.items():
        for cg, og in SHAPES:
            for groups in GROUPS:
                routes[f"{mname} {cg} {og} g{groups}"] = [L.vc_deform_select(mode, cg, og, groups, xh, vec, rv)
                                                          for xh in X_HALF for vec in VEC for rv in RV]
    return {"axes": {"mode": MODES, "shape": [list(s) for s in SHAPES], "groups": GROUPS, "x_half": X_HALF, "vec": VEC, "rv": RV},
            "code": "-1: VC_EINVAL; else VEC | RV << 1 | (MAXT == 512) << 4 | XH << 5",
            "routes": routes}


def dumps(doc):
    """one line per (mode, shape, groups): a diff of the file names the calls that changed"""
    lines = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in doc["routes"].items())
    return ('{\n "axes": %s,\n "code": %s,\n "routes": {\n%s\n }\n}\n' % (json.dumps(doc["axes"]), json.dumps(doc["code"]), lines))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "deform_routes.json"))
    a = ap.parse_args()
    with open(a.out, "w") as f:
        f.write(dumps(build()))
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
