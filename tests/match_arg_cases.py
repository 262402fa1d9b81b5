"""cs_label_match with a NULL handle and one argument rule broken, or two at once, in the style of tests/noise_arg_cases.py: which
rule answers is part of the ABI.  The status and the cs_last_error() text of every call are written out below, from the rules'
own order: NULL pointers, the two kinds, the sizes, the two maxima, cs_match_params field by field, the size limits, the table
limits, the handle.  tests/test_match_cpu.py replays them.  No call here has valid arguments: with a NULL handle those reach the
device check, whose answer depends on the machine."""
import ctypes as C

import numpy as np

from cellscreen import _lib as L

B, H, W, MP, MT = 1, 8, 8, 4, 5
_PRED = np.zeros((B, H, W), np.int32)
_TRUTH = np.zeros((B, H, W), np.int32)
_PTAB = np.zeros((B, MP, 4), np.int32)
_TTAB = np.zeros((B, MT, 4), np.int32)
_PAIRS = np.zeros(B, np.int64)
_KEEP = []

ORDER = ["pred", "truth", "B", "H", "W", "kind", "mp", "mt", "params", "ptab", "ttab", "tkind", "pairs"]
VALID = dict(pred=_PRED.ctypes.data, truth=_TRUTH.ctypes.data, B=B, H=H, W=W, kind=0, mp=MP, mt=MT, params=(0, 0),
             ptab=_PTAB.ctypes.data, ttab=_TTAB.ctypes.data, tkind=0, pairs=_PAIRS.ctypes.data)

INVALID, UNSUPPORTED = -1, -6
NULL = "NULL argument"
KIND = "in_kind / table_kind must be CS_MEM_HOST or CS_MEM_DEVICE"
RESERVED = "cs_match_params.reserved must be 0"


def _log2(v):
    return f"table_log2 {v}: 0 (automatic) or 10..26"


def _cap(side, m, b):
    return f"max_{side} {m} x batch {b}: the tables are capped at 1048576 labels per image and 4194304 per batch"


# (overrides, status, text)
CASES = [
    (dict(pred=None), INVALID, NULL), (dict(truth=None), INVALID, NULL), (dict(ptab=None), INVALID, NULL), (dict(ttab=None), INVALID, NULL),
    (dict(kind=2), INVALID, KIND), (dict(kind=-1), INVALID, KIND), (dict(tkind=2), INVALID, KIND), (dict(tkind=-1), INVALID, KIND),
    (dict(B=0), INVALID, "batch 0, height 8, width 8: all must be >= 1"),
    (dict(B=-3), INVALID, "batch -3, height 8, width 8: all must be >= 1"),
    (dict(H=0), INVALID, "batch 1, height 0, width 8: all must be >= 1"),
    (dict(W=0), INVALID, "batch 1, height 8, width 0: all must be >= 1"),
    (dict(mp=0), INVALID, "max_pred 0, max_truth 5: both must be >= 1"),
    (dict(mt=0), INVALID, "max_pred 4, max_truth 0: both must be >= 1"),
    (dict(mp=-1), INVALID, "max_pred -1, max_truth 5: both must be >= 1"),
    (dict(params=(0, 1)), INVALID, RESERVED), (dict(params=(12, -1)), INVALID, RESERVED),
    (dict(params=(9, 0)), INVALID, _log2(9)), (dict(params=(27, 0)), INVALID, _log2(27)), (dict(params=(-1, 0)), INVALID, _log2(-1)),
    (dict(params=(1, 0)), INVALID, _log2(1)),
    (dict(H=4097), UNSUPPORTED, "image 4097x8: sides above 4096 are not supported"),
    (dict(W=4097), UNSUPPORTED, "image 8x4097: sides above 4096 are not supported"),
    (dict(B=65536), UNSUPPORTED, "batch 65536: at most 65535 images per call"),
    (dict(mp=(1 << 20) + 1), UNSUPPORTED, _cap("pred", (1 << 20) + 1, 1)),
    (dict(mt=(1 << 20) + 1), UNSUPPORTED, _cap("truth", (1 << 20) + 1, 1)),
    (dict(B=5, mp=1 << 20), UNSUPPORTED, _cap("pred", 1 << 20, 5)),
    (dict(B=4097, mt=1024), UNSUPPORTED, _cap("truth", 1024, 4097)),
    # two at once: the first rule in the order above answers
    (dict(pred=None, kind=2), INVALID, NULL), (dict(ttab=None, B=0), INVALID, NULL), (dict(kind=2, H=0), INVALID, KIND),
    (dict(tkind=2, params=(9, 0)), INVALID, KIND), (dict(W=0, mp=0), INVALID, "batch 1, height 8, width 0: all must be >= 1"),
    (dict(W=0, H=4097), INVALID, "batch 1, height 4097, width 0: all must be >= 1"),
    (dict(mp=0, params=(0, 1)), INVALID, "max_pred 0, max_truth 5: both must be >= 1"),
    (dict(params=(9, 1)), INVALID, RESERVED), (dict(params=(9, 0), H=4097), INVALID, _log2(9)),
    (dict(params=(0, 1), mp=(1 << 20) + 1), INVALID, RESERVED),
    (dict(H=4097, B=65536), UNSUPPORTED, "image 4097x8: sides above 4096 are not supported"),
    (dict(B=65536, mp=(1 << 20) + 1), UNSUPPORTED, "batch 65536: at most 65535 images per call"),
    (dict(mp=(1 << 20) + 1, mt=(1 << 20) + 1), UNSUPPORTED, _cap("pred", (1 << 20) + 1, 1)),
]


def call(lib, over):
    """(status, cs_last_error() text) of cs_label_match with a NULL handle and `over` laid over its valid arguments."""
    a = dict(VALID, **over)
    del _KEEP[:]
    args = []
    for k in ORDER:
        v = a[k]
        if k == "params" and v is not None:
            s = L.CSMatchParams(*v)
            _KEEP.append(s)
            v = C.pointer(s)
        args.append(v)
    status = lib.cs_label_match(None, *args)
    return int(status), lib.cs_last_error().decode()
