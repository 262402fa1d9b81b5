"""The calls of tests/golden/segment_arg_errors.json: every cs_segment_* entry point with a NULL handle and one argument rule
broken, or two rules broken at once (which of them answers is part of the ABI).  tools/make_golden_segment_arg_errors.py records
the status and the cs_last_error() text of each call, test_segment_cpu.py replays them.  No call here has valid arguments: with
a NULL handle those reach the device check, whose answer depends on the machine.

A case is a dict of overrides on the entry point's valid arguments; its name is that dict written out.  Pointers are None (NULL)
or left alone, parameter structs are tuples of their fields in the header's order (None: NULL); cs_smooth_params is (radius,
median, reserved, ((k, weight), ...)) with the weights laid over the valid table of radius 4."""
import ctypes as C

import numpy as np

from cellscreen import _lib as L
from cellscreen import segment as S

B, H, W, CN = 1, 8, 8, 3
_IMG = np.zeros((B, H, W, CN), np.uint16)
_LAB = np.zeros((B, H, W), np.int32)          # large enough for every kind of output plane
_N = np.zeros(B, np.int32)
_THR = np.zeros(B, np.int32)
_DIST = np.zeros((B, H, W), np.uint8)
_KEEP = []                                    # the structs of the call in flight

SMOOTH_TABLE = S.smooth_weights(1.0)          # radius 4


def _struct(cls, fields):
    if fields is None:
        return None
    p = cls()
    for (name, _), v in zip(cls._fields_, fields):
        if isinstance(v, tuple):
            for k, x in enumerate(v):
                getattr(p, name)[k] = x
        else:
            setattr(p, name, v)
    _KEEP.append(p)
    return C.pointer(p)


def _smooth(fields):
    if fields is None:
        return None
    radius, median, reserved, over = fields
    p = L.CSSmoothParams()
    p.radius, p.median, p.reserved = radius, median, reserved
    for k, v in enumerate(SMOOTH_TABLE):
        p.weights[k] = v
    for k, v in over:
        p.weights[k] = v
    _KEEP.append(p)
    return C.pointer(p)


STRUCTS = {"seg": lambda f: _struct(L.CSSegmentParams, f), "split": lambda f: _struct(L.CSSplitParams, f),
           "si": lambda f: _struct(L.CSSplitIntensityParams, f), "bg": lambda f: _struct(L.CSBackgroundParams, f),
           "loc": lambda f: _struct(L.CSLocalParams, f), "clean": lambda f: _struct(L.CSCleanParams, f),
           "hys": lambda f: _struct(L.CSHysteresisParams, f), "smooth": _smooth}

IMAGE = dict(image=_IMG.ctypes.data, pt=1, C=CN, ch=2, B=B, H=H, W=W, kind=0)
IMAGE_ORDER = ["image", "pt", "C", "ch", "B", "H", "W", "kind"]
SEG = (L.THRESH_OTSU, 0, 1, 1)
LABELS = dict(labels=_LAB.ctypes.data, okind=0, n=_N.ctypes.data, thr=_THR.ctypes.data)
PLANE = dict(out=_LAB.ctypes.data, okind=0)

# entry point -> (argument order after the handle, valid arguments, name of the output pointer)
ENTRIES = {
    "cs_segment_threshold": (IMAGE_ORDER + ["seg", "labels", "okind", "n", "thr"], dict(IMAGE, seg=SEG, **LABELS), "labels"),
    "cs_segment_split": (IMAGE_ORDER + ["seg", "split", "labels", "okind", "n", "thr", "dist"],
                         dict(IMAGE, seg=SEG, split=(3,), dist=_DIST.ctypes.data, **LABELS), "labels"),
    "cs_segment_split_intensity": (IMAGE_ORDER + ["seg", "si", "guide", "gpt", "gC", "gch", "labels", "okind", "n", "thr", "dist"],
                                   dict(IMAGE, seg=SEG, si=(16, 0, (0, 0)), guide=_IMG.ctypes.data, gpt=1, gC=CN, gch=2,
                                        dist=_DIST.ctypes.data, **LABELS), "labels"),
    "cs_segment_background": (IMAGE_ORDER + ["bg", "out", "okind"], dict(IMAGE, bg=(5, 0), **PLANE), "out"),
    "cs_segment_local": (IMAGE_ORDER + ["loc", "out", "okind"], dict(IMAGE, loc=(8, 0, -1, 0), **PLANE), "out"),
    "cs_segment_clean": (IMAGE_ORDER + ["seg", "clean", "out", "okind", "thr"],
                         dict(IMAGE, seg=SEG, clean=(1, 2, 4), thr=_THR.ctypes.data, **PLANE), "out"),
    "cs_segment_hysteresis": (IMAGE_ORDER + ["seg", "loc", "hys", "out", "okind", "thr"],
                              dict(IMAGE, seg=SEG, loc=None, hys=(L.WEAK_FRACTION, 32768, (0, 0)), thr=_THR.ctypes.data, **PLANE), "out"),
    "cs_segment_smooth": (IMAGE_ORDER + ["smooth", "out", "okind"], dict(IMAGE, smooth=(4, 0, 0, ()), **PLANE), "out"),
}

# one rule of the image arguments broken at a time, then pairs of them in the order the rules are written
COMMON = [dict(image=None), dict(pt=2), dict(pt=-1), dict(kind=2), dict(kind=-1), dict(okind=2), dict(okind=-1), dict(C=0),
          dict(ch=-1), dict(ch=CN), dict(B=0), dict(H=0), dict(W=0), dict(H=4097), dict(W=4097), dict(B=65536),
          dict(image=None, pt=2), dict(pt=2, kind=2), dict(kind=2, ch=CN), dict(okind=2, C=0), dict(ch=CN, B=0), dict(W=0, H=4097),
          dict(H=4097, B=65536), dict(B=0, W=4097)]
LIMITS = [dict(H=4097), dict(B=0)]       # each competes with a stage rule: the limits come after some of them, the sizes before

SEG_BAD = [(2, 0, 1, 1), (-1, 0, 1, 1), (L.THRESH_FIXED, -1, 1, 1), (L.THRESH_FIXED, 65536, 1, 1), (0, 0, 0, 1), (0, 0, 3, 1),
           (0, 0, 1, -1), (0, 0, 1, 2)]
LOC_BAD = [(0, 0, -1, 0), (256, 0, -1, 0), (8, -65536, -1, 0), (8, 65536, -1, 0), (8, 0, -2, 0), (8, 0, 65536, 0), (8, 0, -1, -1),
           (8, 0, -1, 2), (0, 65536, -2, 2)]

STAGE = {
    "cs_segment_threshold": [dict(seg=s) for s in SEG_BAD] + [dict(n=None), dict(n=None, pt=2)],
    "cs_segment_split": [dict(seg=s) for s in SEG_BAD] + [dict(n=None), dict(split=(0,)), dict(split=(256,)), dict(split=(-1,)),
                                                          dict(split=(0,), seg=SEG_BAD[5])],
    "cs_segment_split_intensity": [dict(seg=s) for s in SEG_BAD] + [
        dict(n=None), dict(si=None), dict(guide=None), dict(si=(0, 0, (0, 0))), dict(si=(255, 0, (0, 0))), dict(si=(16, -1, (0, 0))),
        dict(si=(16, 65536, (0, 0))), dict(si=(16, 0, (1, 0))), dict(si=(16, 0, (0, 1))), dict(gpt=2), dict(gpt=-1), dict(gC=0),
        dict(gch=-1), dict(gch=CN), dict(si=(0, 0, (0, 0)), guide=None), dict(si=(0, -1, (1, 0))), dict(si=(255, 0, (0, 0)), gpt=2),
        dict(gpt=2, gC=0), dict(si=None, seg=SEG_BAD[0])],
    "cs_segment_background": [dict(bg=None), dict(bg=(0, 0)), dict(bg=(256, 0)), dict(bg=(5, -1)), dict(bg=(5, 2)), dict(bg=(0, 2)),
                              dict(bg=None, pt=2), dict(bg=None, out=None)],
    "cs_segment_local": [dict(loc=None), dict(loc=None, out=None)] + [dict(loc=v) for v in LOC_BAD],
    "cs_segment_clean": [dict(seg=s) for s in SEG_BAD] + [
        dict(clean=None), dict(clean=(-1, 2, 4)), dict(clean=(16, 2, 4)), dict(clean=(1, 0, 4)), dict(clean=(1, 3, 4)),
        dict(clean=(1, 2, -1)), dict(clean=(1, 2, (1 << 24) + 1)), dict(clean=(0, 2, 0)), dict(clean=(16, 3, -1)),
        dict(clean=None, image=None), dict(clean=None, out=None), dict(clean=(16, 2, 4), seg=SEG_BAD[5])],
    "cs_segment_hysteresis": [dict(seg=s) for s in SEG_BAD] + [
        dict(hys=None), dict(hys=None, image=None), dict(hys=(3, 32768, (0, 0))), dict(hys=(-1, 32768, (0, 0))),
        dict(hys=(L.WEAK_FRACTION, 32768, (1, 0))), dict(hys=(L.WEAK_FRACTION, 32768, (0, 1))), dict(hys=(L.WEAK_FRACTION, 0, (0, 0))),
        dict(hys=(L.WEAK_FRACTION, 65536, (0, 0))), dict(hys=(L.WEAK_ABSOLUTE, -1, (0, 0))), dict(hys=(L.WEAK_ABSOLUTE, 65536, (0, 0))),
        dict(hys=(L.WEAK_ABSOLUTE, 401, (0, 0)), seg=(L.THRESH_FIXED, 400, 1, 1)), dict(hys=(L.WEAK_LOCAL, 0, (0, 0))),
        dict(loc=(8, 0, -1, 0)), dict(hys=(L.WEAK_ABSOLUTE, 5, (0, 0)), loc=(8, 0, -1, 0)),
        dict(hys=(L.WEAK_LOCAL, 1, (0, 0)), loc=(8, 0, -1, 0)), dict(hys=(L.WEAK_LOCAL, -65536, (0, 0)), loc=(8, 0, -1, 0)),
        dict(hys=(L.WEAK_LOCAL, 65536, (0, 0)), loc=(8, 65535, -1, 0)), dict(hys=(3, 32768, (1, 0)), seg=SEG_BAD[5])] +
        [dict(hys=(L.WEAK_LOCAL, -65536, (0, 0)), loc=v) for v in LOC_BAD],
    "cs_segment_smooth": [dict(smooth=None), dict(smooth=None, out=None), dict(smooth=(0, 0, 0, ())), dict(smooth=(65, 0, 0, ())),
                          dict(smooth=(4, -1, 0, ())), dict(smooth=(4, 2, 0, ())), dict(smooth=(4, 0, 1, ())),
                          dict(smooth=(4, 0, 0, ((2, -1),))), dict(smooth=(3, 0, 0, ())), dict(smooth=(4, 0, 0, ((5, 1),))),
                          dict(smooth=(1, 0, 0, ((0, 0), (1, 32768), (2, 0), (3, 0), (4, 0)))), dict(smooth=(4, 0, 0, ((0, SMOOTH_TABLE[0] + 1),))),
                          dict(smooth=(0, 2, 1, ((2, -1),)))],
}


def case_name(over):
    return ", ".join(f"{k}={over[k]!r}" for k in sorted(over))


def cases():
    """[(entry point, case name, overrides)] in a fixed order, without repeats."""
    out, seen = [], set()
    for entry, (order, base, outp) in ENTRIES.items():
        stage = STAGE[entry]
        overs = [dict(o) for o in COMMON] + [{outp: None}, {outp: None, "pt": 2}] + stage
        overs += [dict(s, **lim) for s in stage for lim in LIMITS if not set(s) & set(lim)]
        for o in overs:
            key = (entry, case_name(o))
            if key not in seen:
                seen.add(key)
                out.append((entry, key[1], o))
    return out


def call(lib, entry, over):
    """(status, cs_last_error() text) of the entry point with a NULL handle and `over` laid over its valid arguments."""
    order, base, _ = ENTRIES[entry]
    a = dict(base, **over)
    del _KEEP[:]
    args = [STRUCTS[k](a[k]) if k in STRUCTS else a[k] for k in order]
    status = getattr(lib, entry)(None, *args)
    return int(status), lib.cs_last_error().decode()
