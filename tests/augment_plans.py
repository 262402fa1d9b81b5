"""The training augmentation (csrc/train.hip augment_kernel / fit_gather_kernel, csrc/train_api.hip fit_transform,
cellscreen/augment.py) on every shape the trainers accept and on the transforms at which its clamp, its `min(floor, H - 2)` branch and
its H-against-W bookkeeping decide: the shapes, the image contents, the transform families and the expected pictures of
tests/test_gpu_augment_sweep.py, and the one-mistake restatements tests/test_augment_plans_cpu.py uses to prove that every family can fail.

Test code only; nothing here touches a GPU (keyed_c_rows calls cs_train_draw_transforms, the library's host-only entry).

The reference is scipy.ndimage.affine_transform(order=1, mode="nearest") followed by the flips.  Outputs are convex combinations of
values in [0, 1]; kernel and SciPy each round a float64 value that differs from the exact one by far less than a float32 ulp, so both
land on one of the same two neighbouring floats, at most 2^-24 = 5.96e-8 apart below 1: BAR, for every family.
"""
from dataclasses import dataclass, field
from functools import lru_cache
from typing import List, Optional, Tuple

import numpy as np
from scipy import ndimage

import generic_plans as GP
import train_plans as TP
from cellscreen.augment import ImageDataGenerator, counter_uniforms
from oracle import augment_oracle as ao

BAR = 6e-8
MOVED = 100 * BAR                 # a mutant "moves" a picture when some pixel differs from the oracle's by more than this
AFFINE = ImageDataGenerator.AFFINE_DTYPE


# ---------------------------------------------------------------- shapes
def _shapes():
    """(hw, channels, n_enc): 64 x 64, every distinct input_hw of train_plans.GENERIC_CASES with the channel list whose batch buffers
    are the smallest (the augmentation never looks at the channels: they only decide what cs_train_create costs), and the
    transposes of those shapes that generic_plans.describe_trainer (the restatement of cs_train_create's refusals) accepts."""
    known = {}
    for hw, ch, n_enc, _why in TP.GENERIC_CASES:
        known.setdefault(tuple(hw), []).append((tuple(ch), n_enc))
    cost = lambda hw, c: TP.generic_train_bytes(hw, c[0], c[1], 1)
    out = [GP.REF]
    for hw, lists in known.items():
        ch, n_enc = min(lists, key=lambda c: cost(hw, c))
        out.append((hw, ch, n_enc))
    tall, refused = [], []
    for hw, lists in known.items():
        t = (hw[1], hw[0])
        if t in known or t == (64, 64):
            continue
        ok = [c for c in lists if GP.describe_trainer(t, c[0], c[1]) is None]
        if ok:
            ch, n_enc = min(ok, key=lambda c: cost(t, c))
            tall.append((t, ch, n_enc))
        else:
            refused.append((t, [GP.describe_trainer(t, c[0], c[1]) for c in lists]))
    return out + tall, tall, refused


SHAPES, TALL, TALL_REFUSED = _shapes()
HWS = [s[0] for s in SHAPES]
SMALLEST = min(HWS, key=lambda hw: hw[0] * hw[1])
RECT = [hw for hw in HWS if hw[0] != hw[1]]


def shape_id(hw):
    return f"{hw[0]}x{hw[1]}"


# ---------------------------------------------------------------- contents
CONTENTS = ("noise", "blob", "ramp", "constant", "frame")


@lru_cache(maxsize=None)
def content(name, hw, seed=0):
    """One float32 picture in [0, 1]."""
    from cellscreen import synth
    H, W = hw
    if name == "noise":
        img = np.random.default_rng(1000 + seed).random(hw, dtype=np.float32)
    elif name == "blob":
        img = synth.blob_crops(7 + seed, 1, hw=hw)[0]
    elif name == "ramp":                     # an index mistake is exact and visible
        img = (np.arange(H * W, dtype=np.float64).reshape(H, W) / (H * W)).astype(np.float32)
    elif name == "constant":
        img = np.full(hw, 0.625, np.float32)
    elif name == "frame":                    # a clamp one short of the edge moves the bright line
        img = np.full(hw, 0.125, np.float32)
        img[0, :] = img[-1, :] = 1.0
        img[:, 0] = img[:, -1] = 0.75
    else:
        raise KeyError(name)
    img = np.ascontiguousarray(img, np.float32)
    assert img.shape == tuple(hw) and img.min() >= 0.0 and img.max() <= 1.0
    img.setflags(write=False)
    return img


# ---------------------------------------------------------------- transform families
@dataclass
class Family:
    name: str
    hw: Tuple[int, int]
    rows: np.ndarray                                            # AFFINE_DTYPE, what the kernel is handed
    params: List[Optional[dict]] = field(default_factory=list)  # the Keras parameters a row was packed from; None: a raw row
    center: List[float] = field(default_factory=list)
    frac: List[Tuple[bool, bool]] = field(default_factory=list)  # (tx, ty) was drawn as a fraction of (H, W)
    exact: List[Optional[tuple]] = field(default_factory=list)  # ("shift", tx, ty) / ("pixel", r, c): a statement with no rounding in it
    note: List[str] = field(default_factory=list)

    def __len__(self):
        return len(self.rows)


def _p(theta=0.0, tx=0.0, ty=0.0, zx=1.0, zy=1.0, flip_h=False, flip_v=False):
    return dict(theta=float(theta), tx=float(tx), ty=float(ty), zx=float(zx), zy=float(zy), flip_h=bool(flip_h), flip_v=bool(flip_v))


def pack_rows(params, hw, center):
    arr = ImageDataGenerator(center=center).pack(params, hw[0], hw[1])
    return np.frombuffer(bytes(arr), AFFINE).copy() if len(params) else np.zeros(0, AFFINE)


class _Builder:
    def __init__(self, name, hw):
        self.f = Family(name, tuple(hw), np.zeros(0, AFFINE))
        self._rows = []

    def add(self, p, center=-0.5, frac=(False, False), exact=None, note=""):
        self._rows.append(pack_rows([p], self.f.hw, center))
        self._meta(p, center, frac, exact, note)

    def raw(self, m, off, exact=None, note=""):
        r = np.zeros(1, AFFINE)
        r["m"][0], r["off"][0] = m, off
        self._rows.append(r)
        self._meta(None, -0.5, (False, False), exact, note)

    def row(self, r, p, center, frac, note=""):
        self._rows.append(np.array([r], AFFINE))
        self._meta(p, center, frac, None, note)

    def _meta(self, p, center, frac, exact, note):
        f = self.f
        f.params.append(p); f.center.append(center); f.frac.append(frac); f.exact.append(exact); f.note.append(note)

    def done(self):
        self.f.rows = np.concatenate(self._rows)
        self.f.rows.setflags(write=False)
        return self.f


WIDE = dict(rotation_range=40, width_shift_range=0.4, height_shift_range=0.4, zoom_range=(0.5, 1.5), horizontal_flip=True, vertical_flip=True)
# (name, generator): both centre constants, and shift ranges >= 1, which Keras reads as pixels and not as fractions of the side
GENERATORS = (
    ("wide", ImageDataGenerator(center=-0.5, **WIDE)),
    ("wide, centre +0.5", ImageDataGenerator(center=+0.5, **WIDE)),
    ("pixel shifts", ImageDataGenerator(center=-0.5, **dict(WIDE, height_shift_range=5.0, width_shift_range=3.0))),
)
DRAWS_PER_GENERATOR = 12
KEYS = ((42, 0), (43, 1249), (2 ** 40 + 7, 10 ** 9))            # (seed, step) as in test_augment_cpu.py
KEYED_N = 8


def _frac(g):
    return (g.height_shift_range < 1, g.width_shift_range < 1)


@lru_cache(maxsize=None)
def draws(hw):
    b = _Builder("draws", hw)
    for gi, (name, g) in enumerate(GENERATORS):
        rng = np.random.RandomState(100 + gi)
        for _ in range(DRAWS_PER_GENERATOR):
            b.add(g.get_random_transform(hw, rng), g.center, _frac(g), note=name)
    return b.done()


def keyed_params(g, seed, step, n, hw):
    """The Keras parameters behind keyed_transforms(seed, step, n, hw): counter_uniforms in get_random_transform's order."""
    u = counter_uniforms(seed, step, n)
    r, hs, ws, (zl, zh) = g.rotation_range, g.height_shift_range, g.width_shift_range, g.zoom_range
    out = []
    for k in range(n):
        out.append(_p(theta=(-r + 2 * r * u[k, 0]) if r else 0.0,
                      tx=(-hs + 2 * hs * u[k, 1]) * (hw[0] if hs < 1 else 1.0) if hs else 0.0,
                      ty=(-ws + 2 * ws * u[k, 2]) * (hw[1] if ws < 1 else 1.0) if ws else 0.0,
                      zx=zl + (zh - zl) * u[k, 3] if (zl, zh) != (1.0, 1.0) else 1.0,
                      zy=zl + (zh - zl) * u[k, 4] if (zl, zh) != (1.0, 1.0) else 1.0,
                      flip_h=bool(u[k, 5] < 0.5) and g.horizontal_flip, flip_v=bool(u[k, 6] < 0.5) and g.vertical_flip))
    return out


@lru_cache(maxsize=None)
def keyed(hw, c_draw=False):
    """What fit_step itself draws: the Python mirror's rows, or (c_draw) cs_train_draw_transforms' own."""
    from cellscreen.augment import draw_transforms_c
    b = _Builder("keyed", hw)
    for name, g in GENERATORS:
        for seed, step in KEYS:
            rows = draw_transforms_c(g, seed, step, KEYED_N, hw) if c_draw else g.keyed_transforms(seed, step, KEYED_N, hw)
            for r, p in zip(rows, keyed_params(g, seed, step, KEYED_N, hw)):
                b.row(r, p, g.center, _frac(g), note=f"{name} ({seed}, {step})")
    return b.done()


@lru_cache(maxsize=None)
def lattice(hw):
    """Sample points exactly on the pixel lattice: fr = 0 and fr = 1, r0 = H - 2 at rr = H - 1, coordinates on both edges."""
    H, W = hw
    b = _Builder("lattice", hw)
    rs, cs = range(-(H + 1), H + 2), range(-(W + 1), W + 2)
    for k in rs:
        b.add(_p(tx=k), exact=("shift", k, 0), note="row shift")
    for k in cs:
        b.add(_p(ty=k), exact=("shift", 0, k), note="column shift")
    rng = np.random.default_rng(H * 1000 + W)
    pairs = [(k, int(rng.integers(-(W + 1), W + 2))) for k in rs]
    pairs += [(sr * a, sc * c) for a, c in ((H + 1, W + 1), (H - 1, W - 1), (H, W), (1, 1)) for sr in (-1, 1) for sc in (-1, 1)]
    for tx, ty in pairs:
        b.add(_p(tx=tx, ty=ty), exact=("shift", tx, ty), note="paired shift")
    for theta in (90.0, -90.0, 180.0):
        for center in (-0.5, 0.5):
            b.add(_p(theta=theta), center, note="quarter turns")
    for zx, zy in ((2, 1), (1, 2), (0.5, 0.5)):
        b.add(_p(zx=zx, zy=zy), note="zoom on the lattice")
    # beyond the listed cases: rotations whose sample points fall on or next to lattice lines, where the oracle and SciPy were seen to
    # round differently
    for theta in (45.0, 0.5, 179.999):
        b.add(_p(theta=theta), note="near the lattice")
        b.add(_p(theta=theta, tx=3, ty=-2), note="near the lattice")
        b.add(_p(theta=theta, zx=2, zy=2), 0.5, note="near the lattice")
    return b.done()


@lru_cache(maxsize=None)
def outside(hw):
    """The clamp on each side of each axis; where the output is constant it is one named input pixel."""
    H, W = hw
    b = _Builder("outside", hw)
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            if sx or sy:
                px = ("pixel", 0 if sx < 0 else H - 1, 0 if sy < 0 else W - 1) if sx and sy else None
                b.add(_p(tx=1000 * sx, ty=1000 * sy), exact=px or ("shift", 1000 * sx, 1000 * sy), note="pushed outside")
    zero = (0.0, 0.0, 0.0, 0.0)
    for (orow, ocol), px in (((2.0, 3.0), (2, 3)), ((0.0, 0.0), (0, 0)), ((H - 1.0, W - 1.0), (H - 1, W - 1)), ((H - 1.0, 0.0), (H - 1, 0)),
                             ((0.0, W - 1.0), (0, W - 1)), ((-5.0, W + 7.0), (0, W - 1)), ((H + 3.0, -2.0), (H - 1, 0)),
                             ((-1e6, -1e6), (0, 0)), ((1e6, 1e6), (H - 1, W - 1)), ((3.0, W + 0.5), (3, W - 1)), ((H - 0.5, 5.0), (H - 1, 5))):
        b.raw(zero, (orow, ocol), exact=("pixel",) + px, note="zero matrix")
    b.raw(zero, (1.5, 2.25), note="zero matrix, between pixels")
    b.raw(zero, (H - 1.25, W - 1.75), note="zero matrix, between pixels")
    for zx, zy in ((0.25, 4.0), (4.0, 0.25)):
        b.add(_p(zx=zx, zy=zy), note="anisotropic zoom")
        b.add(_p(zx=zx, zy=zy), 0.5, note="anisotropic zoom")
    return b.done()


@lru_cache(maxsize=None)
def flips(hw):
    """Flips act on the output index, after the resampling: H - 1 - r against W - 1 - c."""
    b = _Builder("flips", hw)
    for fh in (False, True):
        for fv in (False, True):
            b.add(_p(flip_h=fh, flip_v=fv), note="flips alone")
            b.add(_p(theta=7.0, tx=1.5, ty=-2.25, flip_h=fh, flip_v=fv), note="flips after a rotation")
    return b.done()


FAMILIES = {"draws": draws, "lattice": lattice, "outside": outside, "flips": flips, "keyed": keyed}


def family(name, hw, **kw):
    return FAMILIES[name](tuple(hw), **kw)


# ---------------------------------------------------------------- expected pictures
def _flip(out, fh, fv):
    if fh:
        out = out[:, ::-1]
    if fv:
        out = out[::-1, :]
    return out


def scipy_apply(img, row):
    out = img if row["identity"] else ndimage.affine_transform(img, row["m"].reshape(2, 2), row["off"], order=1, mode="nearest")
    return np.ascontiguousarray(_flip(out, row["flip_h"], row["flip_v"]))


def oracle_apply(img, row):
    out = img if row["identity"] else ao.affine_nearest_order1(img, row["m"].reshape(2, 2), row["off"])
    return np.ascontiguousarray(_flip(out, row["flip_h"], row["flip_v"]))


def shift_gather(img, tx, ty):
    """theta = 0, zoom 1, integer shifts: img[clip(r + tx), clip(c + ty)].  The offset (ox + tx) - ox is exact in float64 (ox is a
    half-integer), so no rounding enters and the kernel must give these bits."""
    H, W = img.shape
    r = np.clip(np.arange(H) + int(tx), 0, H - 1)
    c = np.clip(np.arange(W) + int(ty), 0, W - 1)
    return np.ascontiguousarray(img[r[:, None], c[None, :]])


def exact_picture(img, ex):
    if ex is None:
        return None
    if ex[0] == "shift":
        return shift_gather(img, ex[1], ex[2])
    return np.full(img.shape, img[ex[1], ex[2]], img.dtype)


def batch(fam, contents=CONTENTS):
    """(x [len(contents) * len(fam), H, W], rows): every content under every transform of the family, content-major."""
    x = np.concatenate([np.broadcast_to(content(c, fam.hw), (len(fam),) + fam.hw) for c in contents])
    return np.ascontiguousarray(x), np.ascontiguousarray(np.tile(fam.rows, len(contents)))


@lru_cache(maxsize=None)
def expected(name, hw, **kw):
    """SciPy's pictures of batch(family(name, hw)), computed once; read-only."""
    fam = family(name, hw, **kw)
    out = np.stack([scipy_apply(content(c, fam.hw), r) for c in CONTENTS for r in fam.rows])
    out.setflags(write=False)
    return out


def exact_expected(fam, contents=CONTENTS):
    """[(index into batch(fam), picture)] for the rows that have an exact statement."""
    out = []
    for ci, c in enumerate(contents):
        for k, ex in enumerate(fam.exact):
            if ex is not None:
                out.append((ci * len(fam) + k, exact_picture(content(c, fam.hw), ex)))
    return out


# ---------------------------------------------------------------- one mistake at a time
# (name: what the kernel / the draw would have written).  RECT_ONLY: no mistake at all while H == W.
MISTAKES = {
    "oy_from_h": "oy = h / 2 + c in the centre (fit_transform, random_transforms, keyed_transforms)",
    "tx_by_w": "the fractional height shift scaled by the width",
    "stride_h": "r0 * H as the row stride of the four reads",
    "clamp_rows_h2": "rr clamped to H - 2",
    "clamp_cols_h1": "cc clamped to H - 1",
    "flips_first": "the flips applied to the input, before the resampling",
    "flip_h_about_h": "flip_h as H - 1 - c",
    "center_plus": "centre constant +0.5 where -0.5 was asked",
    "r0_uncapped": "r0 = floor(rr) without min(., H - 2): at rr = H - 1 row H is read (taken as row H - 1)",
}
MATRIX_MISTAKES = ("oy_from_h", "tx_by_w", "center_plus")
RECT_ONLY = ("oy_from_h", "tx_by_w", "stride_h", "clamp_cols_h1", "flip_h_about_h")


def matrix_with(p, h, w, center=-0.5, mistake=None, frac=(False, False)):
    """ao.affine_matrix with one mistake switched in (none: the same operations in the same order, the same bits)."""
    tx = p["tx"]
    if mistake == "tx_by_w" and frac[0]:
        tx = tx / h * w
    if mistake == "center_plus" and center == -0.5:
        center = 0.5
    m = None
    if p["theta"] != 0:
        t = np.deg2rad(p["theta"])
        m = np.array([[np.cos(t), -np.sin(t), 0.0], [np.sin(t), np.cos(t), 0.0], [0.0, 0.0, 1.0]])
    if tx != 0 or p["ty"] != 0:
        s = np.array([[1.0, 0.0, tx], [0.0, 1.0, p["ty"]], [0.0, 0.0, 1.0]])
        m = s if m is None else m @ s
    if p["zx"] != 1 or p["zy"] != 1:
        z = np.array([[p["zx"], 0.0, 0.0], [0.0, p["zy"], 0.0], [0.0, 0.0, 1.0]])
        m = z if m is None else m @ z
    if m is None:
        return None
    ox, oy = float(h) / 2 + center, float(h if mistake == "oy_from_h" else w) / 2 + center
    off = np.array([[1.0, 0.0, ox], [0.0, 1.0, oy], [0.0, 0.0, 1.0]])
    rst = np.array([[1.0, 0.0, -ox], [0.0, 1.0, -oy], [0.0, 0.0, 1.0]])
    m = off @ m @ rst
    return m[:2, :2].copy(), m[:2, 2].copy()


def resample_with(img, am, flip_h, flip_v, mistake=None):
    """ao.apply_transform's resampling + flips (am: (matrix, offset) or None for the identity) with one mistake switched in."""
    h, w = img.shape
    src = _flip(img, flip_h, flip_v) if mistake == "flips_first" else img
    if am is None:
        out = src
    else:
        mat, offset = am
        r, c = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        rr = mat[0, 0] * r + mat[0, 1] * c + offset[0]
        cc = mat[1, 0] * r + mat[1, 1] * c + offset[1]
        rr = np.clip(rr, 0.0, (h - 2.0) if mistake == "clamp_rows_h2" else (h - 1.0))
        cc = np.clip(cc, 0.0, (h - 1.0) if mistake == "clamp_cols_h1" else (w - 1.0))
        r0 = np.floor(rr).astype(np.int64) if mistake == "r0_uncapped" else np.minimum(np.floor(rr), h - 2).astype(np.int64)
        c0 = np.minimum(np.floor(cc), w - 2).astype(np.int64)
        fr, fc = rr - r0, cc - c0
        x = src.astype(np.float64)
        r1, c1 = np.minimum(r0 + 1, h - 1), np.minimum(c0 + 1, w - 1)
        if mistake == "stride_h":
            flat = x.ravel()
            at = lambda a, b_: flat.take(a * h + b_, mode="clip")
        else:
            at = lambda a, b_: x[a, b_]
        out = (1 - fr) * ((1 - fc) * at(r0, c0) + fc * at(r0, c1)) + fr * ((1 - fc) * at(r1, c0) + fc * at(r1, c1))
        out = out.astype(img.dtype)
    if mistake == "flips_first":
        return np.ascontiguousarray(out)
    if mistake == "flip_h_about_h" and flip_h:
        # the kernel's store dst[ro * W + co] with co = H - 1 - c: a flat index; what falls outside the picture is dropped here
        ro = (h - 1 - np.arange(h) if flip_v else np.arange(h))[:, None]
        idx = ro * w + (h - 1 - np.arange(w))[None, :]
        ok = (idx >= 0) & (idx < h * w)
        wrong = np.zeros(h * w, out.dtype)
        wrong[idx[ok]] = out[ok]
        return wrong.reshape(h, w)
    return np.ascontiguousarray(_flip(out, flip_h, flip_v))


def mutant_apply(img, fam, k, mistake=None):
    """Row k of the family on img as the oracle with `mistake` would compute it.  A matrix mistake needs the Keras parameters: raw rows
    (the zero matrices of `outside`) are beyond its reach and come out as the oracle's."""
    row, p = fam.rows[k], fam.params[k]
    if p is not None and mistake in MATRIX_MISTAKES:
        am = matrix_with(p, fam.hw[0], fam.hw[1], fam.center[k], mistake, fam.frac[k])
    else:
        am = None if row["identity"] else (row["m"].reshape(2, 2), row["off"])
    return resample_with(img, am, bool(row["flip_h"]), bool(row["flip_v"]), None if mistake in MATRIX_MISTAKES else mistake)


def mutant_subset(fam, most=24):
    """The rows the mutants are evaluated on: every row but the integer shifts, of which lattice has 6 H + ... : an even stride through
    those (first and last kept)."""
    shifts = [k for k, ex in enumerate(fam.exact) if ex is not None and ex[0] == "shift"]
    rest = [k for k, ex in enumerate(fam.exact) if ex is None or ex[0] != "shift"]
    if len(shifts) > most:
        shifts = [shifts[i] for i in sorted(set(np.linspace(0, len(shifts) - 1, most).astype(int).tolist()))]
    return sorted(shifts + rest)


# Where each mistake must show (tests/test_augment_plans_cpu.py asserts it on every shape named): family -> which shapes.
#   "all": every plan shape; "rect": every H != W shape; "wide": H < W; "tall": H > W
# r0_uncapped shows nowhere, and cannot: floor(rr) = H - 1 only at rr = H - 1 exactly (rr is clamped), where fr = rr - r0 = 0, so the
# row read out of range has weight 0 and the picture is (1 - 0) * row[H - 1] + 0 * row[H], the capped form's 0 * row[H - 2] +
# 1 * row[H - 1], bit for bit, for every finite row[H].  The cap is a memory-safety property, held by reading the kernel
# (train.hip: `min((int)floor(rr), H - 2)` in both kernels), not one a picture can show.
MUST_MOVE = {
    "oy_from_h": {"draws": "rect", "keyed": "rect", "lattice": "rect", "flips": "rect", "outside": "rect"},
    "tx_by_w": {"draws": "rect", "keyed": "rect"},
    "stride_h": {"draws": "rect", "keyed": "rect", "lattice": "rect", "flips": "rect", "outside": "rect"},
    "clamp_rows_h2": {"draws": "all", "keyed": "all", "lattice": "all", "flips": "all", "outside": "all"},
    "clamp_cols_h1": {"draws": "rect", "keyed": "rect", "lattice": "rect", "flips": "rect", "outside": "rect"},
    "flips_first": {"draws": "all", "keyed": "all", "flips": "all"},
    "flip_h_about_h": {"draws": "rect", "keyed": "rect", "flips": "rect"},
    "center_plus": {"draws": "all", "keyed": "all", "lattice": "all", "flips": "all", "outside": "all"},
    "r0_uncapped": {},
}


def shapes_of(which):
    return {"all": HWS, "rect": RECT, "wide": [hw for hw in HWS if hw[0] < hw[1]], "tall": [hw for hw in HWS if hw[0] > hw[1]]}[which]


# ---------------------------------------------------------------- fit_step's gather
FIT_TRAIN = 200
FIT_BATCHES = (1, 32, 33)
FIT_STEPS = (0, 1249)
FIT_SEED = 77


def fit_train_set(hw):
    """200 resident crops: noise and the ramp alternating, every crop different (a ramp scaled per crop)."""
    H, W = hw
    rng = np.random.default_rng(H * 7 + W)
    x = rng.random((FIT_TRAIN, H, W), dtype=np.float32)
    ramp = content("ramp", tuple(hw))
    for k in range(1, FIT_TRAIN, 2):
        x[k] = ramp * np.float32(1.0 - k / (2.0 * FIT_TRAIN))
    return x


def fit_idx(batch_size, step):
    """Indices with repeats, the first and the last crop, in no order."""
    rng = np.random.default_rng(batch_size * 10007 + step)
    idx = rng.integers(0, FIT_TRAIN, batch_size)
    if batch_size >= 4:
        idx[rng.permutation(batch_size)[:4]] = (0, FIT_TRAIN - 1, idx[0], FIT_TRAIN - 1)
    else:
        idx[0] = FIT_TRAIN - 1 if step else 0
    return idx.astype(np.int32)


# ---------------------------------------------------------------- sequences: the pinned rings behind more than one call
# PinnedRing<8> aug_ring: call 9 is the first to get a slot back (calls 9..12 reuse the slots of 1..4); call 13 needs more bytes and
# reallocates the ring; calls 21..24 reuse the slots of 13..16.
SEQ_AUG_N = (4,) * 12 + (64,) * 12
# PinnedRing<16> fit_ring: step 17 is the first to get a slot back; step 18 needs more bytes and reallocates; two steps follow it.
SEQ_FIT_BATCHES = (8,) * 17 + (40,) + (8,) * 2
SEQ_SHAPE = (8, 64)


def seq_rows(hw, call, n):
    """Call number `call` gets its own n transforms: the wide generators' draws, seeded by the call."""
    g = GENERATORS[call % len(GENERATORS)][1]
    return g.random_transforms(n, hw, np.random.default_rng(500 + call))


def seq_input(hw, call, n):
    return np.random.default_rng(900 + call).random((n,) + tuple(hw), dtype=np.float32)


# ---------------------------------------------------------------- many images in one call
MANY_N = 70000
MANY_PROTOS = 16
MANY_MARKED = (0, 65534, 65535, 65536, 69999)        # non-identity transforms here: either side of 2^16 and both ends


@lru_cache(maxsize=None)
def many_plan(hw=None):
    """(prototype crops [16, H, W], their transforms [16], index map [70000]): the big batch is the prototypes gathered by the map.
    Prototypes 0..3 are the identity with the four flip pairs, 4..15 draws of the wide generators."""
    hw = tuple(hw or SMALLEST)
    d = draws(hw)
    nonid = [k for k in range(len(d)) if not d.rows[k]["identity"]][::3][:MANY_PROTOS - 4]
    rows = np.concatenate([flips(hw).rows[0::2], d.rows[nonid]])
    assert len(rows) == MANY_PROTOS and rows["identity"][:4].all() and not rows["identity"][4:].any()
    crops = np.stack([np.array(content(CONTENTS[k % 3], hw, seed=k // 3)) for k in range(MANY_PROTOS)])
    crops[[k for k in range(MANY_PROTOS) if k % 3 == 2]] *= np.linspace(0.5, 1.0, len(range(2, MANY_PROTOS, 3)), dtype=np.float32)[:, None, None]
    imap = np.random.default_rng(70000).integers(0, MANY_PROTOS, MANY_N)
    for j, i in enumerate(MANY_MARKED):
        imap[i] = 4 + (5 * j) % (MANY_PROTOS - 4)
    return crops, rows, imap


@lru_cache(maxsize=None)
def many_expected(hw=None):
    crops, rows, _ = many_plan(hw)
    return np.stack([scipy_apply(c, r) for c, r in zip(crops, rows)])
