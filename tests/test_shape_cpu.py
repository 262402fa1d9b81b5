"""CPU tests of the per-object shape records (cs_label_shape, cellscreen/shape.py): the restatement of
tests/shape_reference.py against its slow form and against its record tests/golden/golden_shape.npz, the perimeter classes against
a literal SciPy transcription of skimage.measure.perimeter's rule, the Euler numbers against scipy.ndimage.label, the hull records
against tests/extract_reference.convex_area and a brute force over all edge midpoints, closed forms, the values the package derives
against exact rationals, and the wrapper's and the C ABI's refusals before any device work.

The derived floats' tolerance is DERIVED_REL = 16 * 1.8e-14: 1.8e-14 bounds the largest relative difference between
cellscreen.shape.shape_table and shape_reference.derive_slow (every rational value a Fraction rounded once, every irrational one by
one libm call from such a value) over the cases of seed 1 below (1.74e-14, measured on the CPU); the factor 16 is for the other
seeds.  Hu's invariants do not set it: the package takes each from one exact integer numerator, so they agree to the bit, as do
the central moments.  It is the smaller eigenvalue of the inertia tensor that is largest, on the object in two far pieces: the
prescribed closed form takes it as mean - rad, two rounded numbers fifty times its size.  Every other value stays below 3e-16 but the
minor axis, its square root (8.7e-15).  No device code is involved."""
import ctypes as C
import math
import os

import numpy as np
import pytest
from scipy import ndimage as ndi

import extract_reference as ER
import shape_reference as SR
from cellscreen import _lib as L
from cellscreen import shape as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_shape.npz")
DERIVED_REL = 16 * 1.8e-14
NAMES = ("moments", "box", "quads", "perim", "hull")
DTYPES = (np.int64, np.int32, np.int32, np.int32, np.int64)


def small_cases(seed=10):
    """(name, labels [2,H,W], exclude or None)"""
    out = []
    for k, shape in enumerate(((13, 17), (12, 15), (9, 20), (1, 1), (6, 7), (1, 9), (8, 1))):
        for name, lab in SR.contents(shape, seed + k):
            labels = np.stack([lab, np.roll(lab, 1, axis=1)])
            ex = np.stack([(lab > 0) & (np.arange(shape[1])[None, :] % 3 == 0), np.zeros(shape, bool)]).astype(np.int32) * -9
            out.append((f"{shape} {name}", labels, ex if k % 2 else None))
    return out


def same(a, b, name=""):
    assert len(a) == len(b) == 5
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), name
        if x is not None:
            assert x.dtype == y.dtype == DTYPES[k] and x.shape == y.shape, (name, NAMES[k])
            assert np.array_equal(x, y), (name, NAMES[k])


def perimeter_classes_scipy(mask):
    """the three class counts of skimage.measure.perimeter(mask, neighbourhood=4), transcribed literally"""
    mask = np.asarray(mask, bool)
    cross = ndi.generate_binary_structure(2, 1)
    border = mask.astype(np.uint8) - ndi.binary_erosion(mask, cross, border_value=0).astype(np.uint8)
    conv = ndi.convolve(border, np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]]), mode="constant", cval=0)
    hist = np.bincount(conv.ravel(), minlength=50)
    return [int(hist[[5, 7, 15, 17, 25, 27]].sum()), int(hist[[21, 33]].sum()), int(hist[[13, 23]].sum())]


def objects(labels, exclude):
    """(b, label, mask [H,W]) of the objects of a batch"""
    e = np.where(exclude == 0, labels, 0) if exclude is not None else labels
    return [(b, int(m), e[b] == m) for b in range(e.shape[0]) for m in np.unique(e[b]) if m > 0]


def one(mask, hull=True):
    """the records' rows of a single mask, as lists"""
    rec = SR.measure(np.asarray(mask, np.int32)[None], hull=hull)
    return [None if x is None else x[0, 0].tolist() for x in rec], rec


def test_restatement_equals_the_slow_form():
    for name, labels, ex in small_cases():
        same(SR.measure(labels, ex), SR.measure_slow(labels, ex), name)
    lab = np.array([[[1, 1, 0], [1, 0, 2]]], np.int32)
    m, bx, q, p, h = SR.measure(lab, max_label=3)
    assert m[0].tolist() == [[3, 1, 1, 1, 0, 1, 1, 0, 0, 1], [1, 1, 2, 1, 2, 4, 1, 2, 4, 8], [0] * 10]
    assert bx[0].tolist() == [[0, 0, 2, 2], [1, 2, 2, 3], [0, 0, 0, 0]]
    # label 1: corners (-1,-1) 8, (-1,0) 10, (-1,1) 2, (0,-1) 12, (0,0) 7, (0,1) 1, (1,-1) 4, (1,0) 1
    assert q[0, 0].tolist() == [0, 2, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0, 0, 0] and q[0, 1].tolist() == [0, 1, 1, 0, 1, 0, 0, 0, 1] + [0] * 7
    assert not q[0, 2].any() and not p[0, 2].any() and not h[0, 2].any() and h[0, 1].tolist() == [1, 4, 2, 2]
    none = SR.measure(lab, exclude=lab, max_label=3)
    assert all(not x.any() for x in none) and SR.measure(lab, hull=False)[4] is None
    for bad in (-1, 4):
        lab2 = lab.copy()
        lab2[0, 0, 2] = bad
        with pytest.raises(ValueError):
            SR.measure(lab2, exclude=np.ones_like(lab), max_label=3)     # refused whatever exclude holds there
        with pytest.raises(ValueError):
            SR.measure_slow(lab2, max_label=3)


def test_perimeter_classes_equal_the_scipy_transcription():
    assert perimeter_classes_scipy(np.ones((7, 12), bool)) == [34, 0, 0] and perimeter_classes_scipy(np.ones((1, 1), bool)) == [0, 0, 0]
    seen = np.zeros(3, np.int64)
    for name, labels, ex in small_cases() + small_cases(40):
        perim = SR.measure(labels, ex, hull=False)[3]
        for b, m, mask in objects(labels, ex):
            assert perim[b, m - 1].tolist() == perimeter_classes_scipy(mask), (name, b, m)
            seen += perim[b, m - 1]
    assert (seen > 0).all()                                              # every class occurs
    rng = np.random.default_rng(5)
    for _ in range(50):
        mask = rng.random((17, 23)) < rng.choice([0.3, 0.6, 0.9])
        assert one(mask, hull=False)[0][3] == perimeter_classes_scipy(mask)


def test_euler_numbers_equal_components_minus_holes():
    rng = np.random.default_rng(8)
    four, eight = ndi.generate_binary_structure(2, 1), np.ones((3, 3), bool)
    for _ in range(60):
        mask = rng.random((17, 23)) < rng.choice([0.3, 0.5, 0.8])
        if not mask.any():
            continue
        t = SH.shape_table(*SR.measure(mask.astype(np.int32)[None], hull=False))
        pad = np.pad(~mask, 1, constant_values=True)                     # the holes: background components but the outer one
        assert t.euler_number[0] == ndi.label(mask, eight)[1] - (ndi.label(pad, four)[1] - 1)
        assert t.euler_number_4[0] == ndi.label(mask, four)[1] - (ndi.label(pad, eight)[1] - 1)
        q1, q3, qd = SH.gray_counts(t.quads[0])
        assert (q1 - q3) % 4 == 2 * qd % 4 and t.quads[0, 0] == 0


def all_midpoints(mask):
    rr, cc = np.nonzero(mask)
    return np.unique(np.concatenate([np.stack([2 * rr + dy, 2 * cc + dx], 1) for dy, dx in SR.MIDPOINTS]), axis=0).astype(np.int64)


def test_hull_records_against_extract_reference_and_brute_force():
    n = 0
    for name, labels, ex in small_cases():
        hull = SR.measure(labels, ex)[4]
        for b, m, mask in objects(labels, ex):
            rr, cc = np.nonzero(mask)
            crop = mask[rr.min():rr.max() + 1, cc.min():cc.max() + 1]
            assert hull[b, m - 1, 0] == ER.convex_area(crop), (name, b, m)
            p = all_midpoints(mask)
            d = p[:, None, :] - p[None, :, :]
            assert hull[b, m - 1, 1] == (d * d).sum(axis=2).max(), (name, b, m)
            # the smallest width over ALL directions is taken on an edge of the hull: no pair of midpoints spans a narrower strip
            w, den = int(hull[b, m - 1, 2]), int(hull[b, m - 1, 3])
            for a0 in range(0, len(p), 3):
                for e in (p[a0 + 1:] - p[a0])[:7]:
                    if e.any():
                        width = np.ptp((p - p[a0]) @ np.array([-e[1], e[0]]))        # of the strip with direction e, times |e|
                        assert int(width) ** 2 * den >= w * w * int(e @ e), (name, b, m)
            n += 1
    assert n > 50


def test_closed_forms():
    for h, w in ((7, 12), (12, 7), (5, 5), (3, 40)):
        mask = np.zeros((h + 3, w + 5), np.int32)
        mask[2:2 + h, 1:1 + w] = 1
        rows, rec = one(mask)
        assert rows == [list(x) for x in SR.rectangle_records(2, 1, h, w)], (h, w)
        t = SH.shape_table(*rec)
        assert t.perimeter[0] == 2 * (h + w) - 4 and t.extent[0] == 1.0 and t.solidity[0] == 1.0 and t.area[0] == h * w
        assert t.euler_number[0] == 1 and t.euler_number_4[0] == 1 and t.bbox[0].tolist() == [2, 1, 2 + h, 1 + w] and t.bbox_area[0] == h * w
        assert t.orientation[0] == (0.0 if h >= w else math.pi / 2) and t.centroid[0].tolist() == [2 + (h - 1) / 2, 1 + (w - 1) / 2]
        assert t.mu[0].tolist() == [h * w * (h * h - 1) / 12, 0.0, h * w * (w * w - 1) / 12, 0.0, 0.0, 0.0, 0.0]
        assert np.isclose(t.major_axis_length[0], math.sqrt(4 * (max(h, w) ** 2 - 1) / 3), rtol=1e-15)
        assert np.isclose(t.minor_axis_length[0], math.sqrt(4 * (min(h, w) ** 2 - 1) / 3), rtol=1e-15)
        assert not t.hu[0, 2:].any() and t.hu[0, 0] == (h * h + w * w - 2) / (12 * h * w)      # symmetric: the odd invariants vanish
        assert t.form_factor[0] == 4 * math.pi * h * w / (2 * (h + w) - 4) ** 2
        assert t.feret_diameter_max[0] == math.sqrt(4 * max(h, w) ** 2 + (2 * min(h, w) - 2) ** 2) / 2
        assert t.feret_diameter_min[0] == min(h, w)                      # a long side is an edge of the hull: the width across it
        holed = mask.copy()
        holed[3, 3] = 0
        th = SH.shape_table(*SR.measure(holed[None]))
        assert th.euler_number[0] == 0 and th.euler_number_4[0] == 0 and th.convex_area[0] == h * w and th.solidity[0] == (h * w - 1) / (h * w)
    rows, rec = one(np.ones((1, 1)))                                     # the single pixel
    assert rows == [list(x) for x in SR.rectangle_records(0, 0, 1, 1)] and rows[3] == [0, 0, 0] and rows[4] == [1, 4, 2, 2]
    t = SH.shape_table(*rec)
    assert t.perimeter[0] == 0 and np.isnan(t.form_factor[0]) and t.convex_area[0] == 1 and t.feret_diameter_max[0] == 1.0
    assert t.feret_diameter_min[0] == 2 / (2 * math.sqrt(2)) and t.eccentricity[0] == 0 and t.major_axis_length[0] == 0 and not t.hu[0].any()
    assert t.euler_number[0] == 1 and t.orientation[0] == 0.0 and t.equivalent_diameter[0] == math.sqrt(4 / math.pi)
    for n in (2, 9, 40):                                                 # the 1 x n and n x 1 lines
        for shape in ((1, n), (n, 1)):
            rows, rec = one(np.ones(shape))
            t = SH.shape_table(*rec)
            assert rows[3] == perimeter_classes_scipy(np.ones(shape, bool)) and rows[4][0] == n and rows[4][1] == 4 * n * n
            assert rows[3] == [max(n - 2, 0), 0, 0]                       # an end pixel has one neighbour, 3: no class holds it
            assert t.eccentricity[0] == 1.0 and t.minor_axis_length[0] == 0.0 and t.solidity[0] == 1.0 and t.euler_number[0] == 1
            assert t.orientation[0] == (math.pi / 2 if shape[0] == 1 else 0.0) and t.feret_diameter_max[0] == n
            assert t.feret_diameter_min[0] == 1.0 and np.isclose(t.major_axis_length[0], math.sqrt(4 * (n * n - 1) / 3), rtol=1e-15)
    for n in (2, 5, 12):                                                 # a diagonal staircase: mu20 = mu02, the sign of mu11 decides
        down = np.eye(n, dtype=np.int32)
        for mask, sign in ((down, 1.0), (down[::-1], -1.0)):
            t = SH.shape_table(*SR.measure(np.ascontiguousarray(mask)[None]))
            assert t.mu[0, 0] == t.mu[0, 2] and t.orientation[0] == sign * math.pi / 4 and t.perim[0].tolist() == [0, max(n - 2, 0), 0]
            assert t.euler_number[0] == 1 and t.euler_number_4[0] == n and t.eccentricity[0] == 1.0
    ring = np.ones((9, 11), np.int32)                                    # a one-pixel-wide ring
    ring[1:-1, 1:-1] = 0
    t = SH.shape_table(*SR.measure(ring[None]))
    assert t.euler_number[0] == 0 and t.euler_number_4[0] == 0 and t.perimeter[0] == 2 * (9 + 11) - 4 and t.convex_area[0] == 99


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_derived_values_equal_the_exact_rationals(seed):
    worst, which = 0.0, ""
    for name, labels, ex in small_cases(100 * seed):
        for hull in (True, False):
            rec = SR.measure(labels, ex, hull=hull)
            got, want = SR.derive(*rec), SR.derive_slow(*rec)
            assert list(got) == list(want)
            for k in got:
                g, w = got[k], want[k]
                assert g.dtype == w.dtype and g.shape == w.shape, (name, k)
                if k in SR.INT_FIELDS or k in ("convex_area", "hu", "mu", "centroid", "extent", "solidity"):
                    assert np.array_equal(g, w, equal_nan=True), (name, k)        # integers, and rationals rounded once on both sides
                    continue
                assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g == 0, w == 0), (name, k)
                ok = ~np.isnan(w) & (w != 0)
                rel = np.abs(g[ok] - w[ok]) / np.abs(w[ok])
                if rel.size and rel.max() > worst:
                    worst, which = float(rel.max()), k
                assert (rel <= DERIVED_REL).all(), (name, k, rel.max())
    print(f"seed {seed}: largest relative difference of a derived value {worst:.3e} ({which})")


def test_table_shapes_and_refusals():
    rec = SR.measure(np.zeros((2, 5, 6), np.int32), max_label=3)
    t = SH.shape_table(*rec)
    assert len(t) == 0 and t.hu.shape == (0, 7) and t.bbox.shape == (0, 4) and t.inertia_tensor.shape == (0, 2, 2) and t.hull.shape == (0, 4)
    t = SH.shape_table(*rec[:4])
    assert t.convex_area is None and t.solidity is None and t.feret_diameter_max is None and t.feret_diameter_min is None and t.hull is None
    m, bx, q, p, h = rec
    with pytest.raises(TypeError):
        SH.shape_table(m.astype(np.int32), bx, q, p, h)
    with pytest.raises(TypeError):
        SH.shape_table(m, bx, q, p, h.astype(np.float64))
    with pytest.raises(ValueError):
        SH.shape_table(m, bx, q[:, :, :15], p, h)
    with pytest.raises(ValueError):
        SH.shape_table(m, bx, q, p, h[:1])


def test_golden_file_matches():
    g = np.load(GOLDEN)
    assert int(g["n_cases"]) == 5 and "pinned to the rule" in str(g["note"]) and "not to a library" in str(g["note"])
    assert os.path.getsize(GOLDEN) < 20_000
    objects_seen = 0
    for i in range(int(g["n_cases"])):
        labels, ex = g[f"labels_{i}"], g[f"exclude_{i}"]
        got = SR.measure(labels, ex)
        for k, key in enumerate(NAMES):
            want = g[f"{key}_{i}"]
            assert got[k].dtype == want.dtype and got[k].shape == want.shape and np.array_equal(got[k], want), (str(g[f"name_{i}"]), key)
        objects_seen += int((got[0][:, :, 0] > 0).sum())
    assert objects_seen >= 15


# ---- the package's argument checks ------------------------------------------------------------------------------------------------
def test_measurer_refusals_before_a_handle_exists():
    import torch

    import cellscreen
    assert cellscreen.ShapeMeasurer is SH.ShapeMeasurer and cellscreen.ShapeTable is SH.ShapeTable and cellscreen.shape_table is SH.shape_table
    m = SH.ShapeMeasurer(0)
    lab = np.zeros((2, 8, 12), np.int32)
    cpu_t = torch.zeros((2, 8, 12), dtype=torch.int32)
    for labels, kw, exc in (
            (lab.astype(np.int64), {}, TypeError), (lab.astype(np.uint8), {}, TypeError), (list(lab), {}, TypeError),
            (lab, dict(exclude=lab.astype(bool)), TypeError), (lab, dict(exclude=list(lab)), TypeError), (lab, dict(exclude=cpu_t), ValueError),
            (lab[0], {}, ValueError), (lab[:, :, ::2], {}, ValueError), (lab, dict(exclude=lab[:, :, :11].copy()), ValueError),
            (lab, dict(exclude=lab[:1]), ValueError), (cpu_t, {}, ValueError), (np.zeros((1, 2, 4097), np.int32), {}, ValueError),
            (np.zeros((1, 4097, 2), np.int32), {}, ValueError), (np.zeros((0, 4, 4), np.int32), {}, ValueError),
            (lab, dict(max_label=0), ValueError), (lab, dict(max_label=-3), ValueError), (lab, dict(max_label=2.0), TypeError),
            (lab, dict(max_label=True), TypeError), (lab, dict(max_label=(1 << 20) + 1), ValueError),
            (np.zeros((5, 2, 2), np.int32), dict(max_label=1 << 20), ValueError)):                        # 5 x 2^20 rows
        for call in (m.measure_batch, m.measure_dense):
            with pytest.raises(exc):
                call(labels, **kw)
    lab2 = lab.copy()
    lab2[0, 0, 0] = (1 << 20) + 1                                        # max_label=None: the labels' maximum meets the same limits
    with pytest.raises(ValueError):
        m.measure_batch(lab2)
    assert m._pre is None
    with pytest.raises(ValueError):
        SH.ShapeMeasurer(1, extractor=type("E", (), {"device_id": 0})())
    m.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2 and lib.cs_profile_kernel_count() == 13
    raw = C.CDLL(L.LIB_PATH)
    for name in ("cs_label_shape", "cs_label_shape_last_timing"):
        assert hasattr(raw, name) and name in L.SIGNATURES
    assert len(L.SIGNATURES["cs_label_shape"][1]) == 15 and len(L.SIGNATURES["cs_label_shape_last_timing"][1]) == 3


def test_the_prototypes_are_in_the_header():
    with open(os.path.join(ROOT, "include", "cellscreen.h")) as f:
        text = " ".join(f.read().split())
    assert ("int cs_label_shape(cs_preproc *p, const int32_t *labels, const int32_t *exclude /* or NULL */, int32_t batch, int32_t height, "
            "int32_t width, int in_kind, int32_t max_label, int want_hull, int64_t *moments, int32_t *box, int32_t *quads, int32_t *perim, "
            "int64_t *hull /* or NULL */, int out_kind);") in text
    assert "int cs_label_shape_last_timing(const cs_preproc *p, double *moments_ms, double *outline_ms);" in text
    assert "#define CS_ABI_VERSION 2 " in text
    assert "[e(r,c)==L] + 2 [e(r+1,c)==L] + 4 [e(r,c+1)==L] + 8 [e(r+1,c+1)==L]" in text                 # the rule is stated there
    assert "{5, 7, 15, 17, 25, 27}" in text and "below 2^59" in text and " * cs_label_shape " in text


def _call(lib, labels=True, moments=True, box=True, quads=True, perim=True, hull=True, want_hull=1, exclude=False, B=1, H=8, W=8, in_kind=0,
          out_kind=0, max_label=4):
    a = np.zeros(64, np.int64)                                           # never read: every call here ends before the device
    p = a.ctypes.data
    rc = lib.cs_label_shape(None, p if labels else None, p if exclude else None, B, H, W, in_kind, max_label, want_hull, p if moments else None,
                            p if box else None, p if quads else None, p if perim else None, p if hull else None, out_kind)
    return rc, lib.cs_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_the_handle():
    lib = L.load_library()
    for over, status in ((dict(labels=False), -1), (dict(moments=False), -1), (dict(box=False), -1), (dict(quads=False), -1), (dict(perim=False), -1),
                         (dict(hull=False), -1), (dict(want_hull=0), -1),                                 # hull iff want_hull
                         (dict(in_kind=2), -1), (dict(out_kind=-1), -1), (dict(B=0), -1), (dict(H=0), -1), (dict(W=-1), -1),
                         (dict(max_label=0), -1), (dict(max_label=-5), -1),
                         (dict(max_label=(1 << 20) + 1), -6), (dict(B=5, max_label=1 << 20), -6), (dict(B=(1 << 12) + 1, max_label=1 << 10), -6),
                         (dict(H=4097), -6), (dict(W=4097), -6), (dict(B=65536), -6)):
        rc, text = _call(lib, **over)
        assert rc == status and text, over
    # the order of the rules: the earlier one answers
    for over, status in ((dict(labels=False, H=4097), -1), (dict(in_kind=7, H=4097), -1), (dict(H=4097, max_label=0), -1), (dict(B=0, max_label=1 << 21), -1),
                         (dict(hull=False, B=65536), -1), (dict(H=4097, max_label=(1 << 20) + 1), -6)):
        assert _call(lib, **over)[0] == status, over
    assert "max_label 0: must be >= 1" in _call(lib, max_label=0)[1] and "capped at 1048576 labels per image and 4194304 rows" in _call(lib, B=5, max_label=1 << 20)[1]
    assert "hull is required with want_hull" in _call(lib, hull=False)[1] and "sides above 4096" in _call(lib, H=4097)[1]
    assert "capped at" in _call(lib, H=4097, max_label=(1 << 20) + 1)[1]                                # the cap answers before the image's limits
    assert lib.cs_label_shape_last_timing(None, None, None) == -1


def test_a_null_handle_reports_no_device_for_valid_arguments():
    lib = L.load_library()
    no_dev = lib.cs_device_count() <= 0
    for over in (dict(), dict(exclude=True), dict(want_hull=0, hull=False), dict(max_label=1 << 20), dict(B=4, max_label=1 << 20),
                 dict(B=1 << 12, max_label=1 << 10), dict(in_kind=1, out_kind=1), dict(H=4096, W=4096), dict(B=65535, H=1, W=1, max_label=64)):
        assert _call(lib, **over)[0] == (-4 if no_dev else -1), over      # no handle: no device here, else a NULL handle
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            SH.ShapeMeasurer(0).measure_batch(np.zeros((1, 8, 8), np.int32))
        assert ei.value.status == -4
