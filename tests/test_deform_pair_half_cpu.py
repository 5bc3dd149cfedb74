"""vc_deform_pair_hxp without a GPU: the header declares it, the library exports it, vcamd.hip binds it, and every argument it
refuses is refused on the host -- VC_EINVAL before any device call (the pointers below are host memory and never read)."""
import ctypes
import os
import re

from vcamd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "vc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+vc_deform_pair_hxp\s*\(\s*vc_stream s, vc_view x1, vc_view raw1, vc_view x2, vc_view raw2,\s*const float \*wpk, "
                     r"const float \*bias,\s*int groups, vc_view out\)\s*;", text)
    assert "vc_deform_pair_hxp" in hip.EXPORTED_SYMBOLS
    fn = hip.lib().vc_deform_pair_hxp
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert [t for t in fn.argtypes if t is hip.View] == [hip.View] * 5
    assert isinstance(hip.HALF_DEFORM_PAIR, bool)


def test_refusals_before_any_device_call():
    L = hip.lib()
    n, h, w, cg, groups = 2, 4, 6, 8, 16
    hg = groups // 2
    buf = (ctypes.c_float * (n * h * w * 27 * hg + 16))()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    good = hip.View(p, n, h, w, cg, hg * h * w * cg, w * cg, cg)
    raw = hip.View(p, n, h, w, 27 * hg, h * w * 27 * hg, w * 27 * hg, 27 * hg)
    out = hip.View(p, n, h, w, groups * cg, h * w * groups * cg, w * groups * cg, groups * cg)

    def v(base, **fields):
        c = hip.View.from_buffer_copy(base)
        for k, val in fields.items():
            setattr(c, k, val)
        return c

    def call(x1=good, r1=raw, x2=good, r2=raw, wpk=p, g=groups, o=out):
        return L.vc_deform_pair_hxp(None, x1, r1, x2, r2, wpk, None, g, o)

    bad = {
        "null x1": dict(x1=v(good, p=None)), "null raw1": dict(r1=v(raw, p=None)), "null x2": dict(x2=v(good, p=None)),
        "null raw2": dict(r2=v(raw, p=None)), "null weights": dict(wpk=None), "null out": dict(o=v(out, p=None)),
        "odd groups": dict(g=15), "groups = 0": dict(g=0),
        "raw1.c != 27 * groups / 2": dict(r1=v(raw, c=215)), "raw2.c != 27 * groups / 2": dict(r2=v(raw, c=217)),
        "x1: sw != c": dict(x1=v(good, sw=cg + 4)), "x2: sw != c": dict(x2=v(good, sw=cg + 4)),
        "x1: sh != w * c": dict(x1=v(good, sh=(w + 1) * cg)), "x2: sh != w * c": dict(x2=v(good, sh=w * cg + 8)),
        "x1: sn of ONE plane": dict(x1=v(good, sn=h * w * cg)), "x2: sn of a padded image": dict(x2=v(good, sn=hg * h * w * cg + 8)),
        "x1.c != x2.c": dict(x2=hip.View(p, n, h, w, 4, hg * h * w * 4, w * 4, 4)),
        "x1 height": dict(x1=hip.View(p, n, h - 1, w, cg, hg * (h - 1) * w * cg, w * cg, cg)),
        "x2 width": dict(x2=hip.View(p, n, h, w + 1, cg, hg * h * (w + 1) * cg, (w + 1) * cg, cg)),
        "x1 batch": dict(x1=v(good, n=1)), "raw1 width": dict(r1=v(raw, w=w - 1)), "raw2 height": dict(r2=v(raw, h=h + 1)),
        "raw2 batch": dict(r2=v(raw, n=3)), "out batch": dict(o=v(out, n=1)),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what
