"""cs_segment_noise with a NULL handle and one argument rule broken, or two at once, in the style of tests/segment_arg_cases.py
(whose valid image arguments and struct builder are used here): which rule answers is part of the ABI.  Unlike that file's
recorded golden, the status and the cs_last_error() text of every call are written out below, from the rules' own order:
NULL pointers, the image arguments up to the sizes, cs_noise_params field by field, the size limits, the handle.
tests/test_noise_cpu.py replays them.  No call here has valid arguments: with a NULL handle those reach the device check,
whose answer depends on the machine."""

import numpy as np

import segment_arg_cases as AC
from cellscreen import _lib as L

_MESH = np.zeros((AC.B, 2, 1, 1), np.int32)
ORDER = AC.IMAGE_ORDER + ["noise", "out", "okind", "mesh"]
NOISE = (64, 1280, -1, 256, 1, (0, 0, 0))               # tile, k8, weak_k8, floor8, connectivity, reserved
VALID = dict(AC.IMAGE, noise=NOISE, mesh=_MESH.ctypes.data, **AC.PLANE)

INVALID, UNSUPPORTED = -1, -6
NULL = "NULL argument"
PIX = "pixel_type must be CS_PIX_U8 or CS_PIX_U16"
KIND = "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE"
RESERVED = "cs_noise_params.reserved must be 0"


def noise(tile=64, k8=1280, weak8=-1, floor8=256, conn=1, reserved=(0, 0, 0)):
    return (tile, k8, weak8, floor8, conn, reserved)


def _tile(t):
    return f"noise tile {t}: a power of two in 16..256"


# (overrides, status, text)
CASES = [
    # the shared rules, with cs_segment_local's texts
    (dict(image=None), INVALID, NULL), (dict(out=None), INVALID, NULL), (dict(noise=None), INVALID, NULL),
    (dict(pt=2), INVALID, PIX), (dict(pt=-1), INVALID, PIX), (dict(kind=2), INVALID, KIND), (dict(kind=-1), INVALID, KIND),
    (dict(okind=2), INVALID, KIND), (dict(okind=-1), INVALID, KIND),
    (dict(C=0), INVALID, "channel 2 of 0: need 0 <= channel < channels"),
    (dict(ch=-1), INVALID, "channel -1 of 3: need 0 <= channel < channels"),
    (dict(ch=3), INVALID, "channel 3 of 3: need 0 <= channel < channels"),
    (dict(B=0), INVALID, "batch 0, height 8, width 8: all must be >= 1"),
    (dict(H=0), INVALID, "batch 1, height 0, width 8: all must be >= 1"),
    (dict(W=0), INVALID, "batch 1, height 8, width 0: all must be >= 1"),
    (dict(H=4097), UNSUPPORTED, "image 4097x8: sides above 4096 are not supported"),
    (dict(W=4097), UNSUPPORTED, "image 8x4097: sides above 4096 are not supported"),
    (dict(B=65536), UNSUPPORTED, "batch 65536: at most 65535 images per call"),
    # cs_noise_params, field by field
    (dict(noise=noise(tile=8)), INVALID, _tile(8)), (dict(noise=noise(tile=512)), INVALID, _tile(512)),
    (dict(noise=noise(tile=48)), INVALID, _tile(48)), (dict(noise=noise(tile=0)), INVALID, _tile(0)),
    (dict(noise=noise(tile=-64)), INVALID, _tile(-64)),
    (dict(noise=noise(k8=0)), INVALID, "noise k8 0 outside 1..16383"),
    (dict(noise=noise(k8=16384)), INVALID, "noise k8 16384 outside 1..16383"),
    (dict(noise=noise(weak8=0)), INVALID, "weak k8 0: -1 (no weak rule) or 1..k8 = 1280"),
    (dict(noise=noise(weak8=-2)), INVALID, "weak k8 -2: -1 (no weak rule) or 1..k8 = 1280"),
    (dict(noise=noise(weak8=1281)), INVALID, "weak k8 1281: -1 (no weak rule) or 1..k8 = 1280"),
    (dict(noise=noise(floor8=-1)), INVALID, "noise floor8 -1 outside 0..1048320"),
    (dict(noise=noise(floor8=1048321)), INVALID, "noise floor8 1048321 outside 0..1048320"),
    (dict(noise=noise(weak8=640, conn=0)), INVALID, "connectivity 0: 1 or 2"),
    (dict(noise=noise(weak8=640, conn=3)), INVALID, "connectivity 3: 1 or 2"),
    (dict(noise=noise(reserved=(1, 0, 0))), INVALID, RESERVED), (dict(noise=noise(reserved=(0, 1, 0))), INVALID, RESERVED),
    (dict(noise=noise(reserved=(0, 0, 1))), INVALID, RESERVED),
    (dict(noise=noise(conn=3, reserved=(0, 0, 1))), INVALID, RESERVED),                  # without a weak rule the connectivity is not read
    # two at once: the first rule in the order above answers
    (dict(noise=None, image=None), INVALID, NULL), (dict(noise=None, pt=2), INVALID, NULL), (dict(out=None, pt=2), INVALID, NULL),
    (dict(image=None, noise=noise(tile=8)), INVALID, NULL), (dict(pt=2, kind=2), INVALID, PIX), (dict(kind=2, ch=3), INVALID, KIND),
    (dict(pt=2, noise=noise(tile=8)), INVALID, PIX), (dict(B=0, noise=noise(k8=0)), INVALID, "batch 0, height 8, width 8: all must be >= 1"),
    (dict(noise=noise(tile=8, k8=0)), INVALID, _tile(8)),
    (dict(noise=noise(k8=0, weak8=0)), INVALID, "noise k8 0 outside 1..16383"),
    (dict(noise=noise(weak8=0, floor8=-1)), INVALID, "weak k8 0: -1 (no weak rule) or 1..k8 = 1280"),
    (dict(noise=noise(floor8=-1, reserved=(1, 0, 0))), INVALID, "noise floor8 -1 outside 0..1048320"),
    (dict(noise=noise(weak8=640, conn=3, reserved=(1, 0, 0))), INVALID, "connectivity 3: 1 or 2"),
    (dict(noise=noise(tile=8), H=4097), INVALID, _tile(8)),                              # the parameters come before the limits
    (dict(noise=noise(reserved=(0, 0, 1)), B=65536), INVALID, RESERVED),
    (dict(W=0, H=4097), INVALID, "batch 1, height 4097, width 0: all must be >= 1"),    # the sizes before them
    (dict(H=4097, B=65536), UNSUPPORTED, "image 4097x8: sides above 4096 are not supported"),
]


def call(lib, over):
    """(status, cs_last_error() text) of cs_segment_noise with a NULL handle and `over` laid over its valid arguments."""
    a = dict(VALID, **over)
    del AC._KEEP[:]
    args = [AC._struct(L.CSNoiseParams, a[k]) if k == "noise" else a[k] for k in ORDER]
    status = lib.cs_segment_noise(None, *args)
    return int(status), lib.cs_last_error().decode()
