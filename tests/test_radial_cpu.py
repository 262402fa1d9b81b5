"""CPU tests of the per-object radial distribution and edge intensities (cs_label_radial, cellscreen/radial.py): the
restatement of tests/radial_reference.py against its slow form in Python ints and Fractions and against SciPy's record
tests/golden/golden_radial.npz, the integer ring rule against the float form, the edge pixels against the border pixels of the
shape and neighbour references, the one difference from CellProfiler on a U-shaped object, the floats the package derives
against a 50-digit decimal form of the same integers, and the wrapper's and the C ABI's refusals before any device work.

The floats.  With u = 2^-53: a quotient of two Python ints is correctly rounded, relative error <= u (frac_at_d, mean_frac,
edge_mean: each is one quotient of two exact integers).  radial_cv and edge_std are the root of one such quotient: the quotient
carries (1 + d1), |d1| <= u, its root sqrt(1 + d1) <= 1 + u / 2, and the root's own rounding (1 + d2), |d2| <= u: at most 1.5 u
and second-order terms, so ROOT_BOUND = 2 u."""
import ctypes as C
import decimal
import math
import os

import numpy as np
import pytest

import intensity_reference as IR
import neighbors_reference as NR
import radial_reference as RR
import shape_reference as SR
from cellscreen import _lib as L
from cellscreen import radial as RA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_radial.npz")
U = 2.0 ** -53
RATIO_BOUND = U
ROOT_BOUND = 2 * U


def same(got, want):
    assert len(got) == len(want) == 5
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


def small_cases():
    """(image [2,H,W,C], labels, exclude or None, kwargs): small enough for the slow form"""
    out = []
    for k, (shape, nc, dtype) in enumerate((((9, 14), 2, np.uint8), ((12, 11), 3, np.uint16), ((7, 20), 4, np.uint8), ((13, 13), 1, np.uint16))):
        lab = np.stack([IR.disks(shape, 5, k, radii=(2, 4)), IR.contents(shape, k + 1)[1][1]])
        if k == 3:
            lab[0] = 1                                   # an object that fills its image: every nearest position is outside
        image = IR.noise((2,) + shape, nc, dtype, 20 + k)
        ex = (IR.disks(shape, 3, k + 7, radii=(1, 2)) > 0).astype(np.int32)
        ex = np.stack([ex, np.zeros_like(ex)])
        m = int(lab.max())
        ctr = np.stack([np.random.default_rng(k).integers(0, shape[0], (2, m)), np.random.default_rng(k + 9).integers(0, shape[1], (2, m))], axis=-1)
        for kw in (dict(), dict(bins=1), dict(bins=16), dict(bins=5, centers=ctr.astype(np.int32)), dict(bins=3)):
            out.append((image, lab, ex if "bins" in kw and kw["bins"] in (16, 3) else None, kw))
    return out


def rel(x, d):
    """|x - d| / |d| of a float against a Decimal; 0 where both are 0"""
    if d == 0:
        return 0.0 if x == 0.0 else math.inf
    return float(abs(decimal.Decimal(x) - d) / abs(d))


# ---- the restatement against its slow form and against SciPy ---------------------------------------------------------------------------
def test_restatement_equals_the_slow_form_in_python_ints_and_fractions():
    for image, lab, ex, kw in small_cases():
        same(RR.measure(image, lab, ex, **kw), RR.measure_slow(image, lab, ex, **kw))


def test_restatement_equals_scipy_on_the_golden_scenes():
    g = np.load(GOLDEN)
    assert str(g["scipy_version"]) == "1.15.3" and int(g["n_cases"]) == 4 and os.path.getsize(GOLDEN) < 100 * 1024
    for i in range(int(g["n_cases"])):
        image, lab, ex, bins = g[f"image_{i}"], g[f"labels_{i}"], g[f"exclude_{i}"], int(g[f"bins_{i}"])
        geom, center, ring, edge, d2 = RR.measure(image[None], lab[None], ex[None], bins=bins)
        rows = g[f"index_{i}"] - 1
        present = np.zeros(geom.shape[1], bool)
        present[rows] = True
        assert np.array_equal(d2[0], g[f"d2_{i}"]) and np.array_equal(center[0, rows], g[f"center_{i}"]), str(g[f"name_{i}"])
        assert np.array_equal(ring[0, rows], g[f"ring_{i}"]) and np.array_equal(edge[0, rows], g[f"edge_{i}"])
        assert not geom[0, ~present].any() and not center[0, ~present].any() and not ring[0, ~present].any() and not edge[0, ~present].any()
        assert np.array_equal(ring[0, rows][..., 0].sum(axis=(1, 2)), geom[0, rows, 0])


def test_depth_is_one_exactly_on_the_border_pixels_of_the_shape_and_neighbour_rules():
    for shape, seed in (((40, 70), 1), ((33, 258), 2), ((1, 40), 3), ((40, 1), 4)):
        for name, lab in NR.contents(shape, seed) + IR.contents(shape, seed):
            lab = np.ascontiguousarray(lab, np.int32)
            geom, center, ring, edge, d2 = RR.measure(np.zeros((1,) + shape, np.uint8), lab[None])
            border = NR.border_mask(lab)
            assert np.array_equal(d2[0] == 1, border), name
            for l in np.unique(lab[lab > 0]):
                assert center[0, l - 1, 3] == (border & (lab == l)).sum(), name
    # shape_reference's perimeter classes hold every border pixel of a rectangle with sides >= 3
    rect = np.zeros((1, 30, 50), np.int32)
    rect[0, 0:3, 0:3] = 1
    rect[0, 5:25, 10:45] = 2
    rect[0, 26:30, 0:50] = 3
    perim = SR.measure(rect, hull=False)[3]
    assert np.array_equal(perim.sum(axis=-1), RR.measure(np.zeros((1, 30, 50), np.uint8), rect)[1][..., 3])
    # an excluded pixel is foreign: its neighbours are edge pixels
    ex = np.zeros_like(rect)
    ex[0, 15, 20] = 1
    d2 = RR.measure(np.zeros((1, 30, 50), np.uint8), rect, ex)[4][0]
    assert d2[15, 20] == 0 and d2[15, 19] == d2[15, 21] == d2[14, 20] == d2[16, 20] == 1 and d2[14, 19] == 2


def test_the_integer_ring_rule_equals_the_float_form():
    checked = ties = 0
    for seed, shape in ((1, (60, 90)), (2, (90, 140))):
        lab = IR.disks(shape, 12, seed, radii=(3, 14))
        geom, center, ring, edge, d2 = RR.measure(np.zeros((1,) + shape, np.uint8), lab[None])
        for l in np.unique(lab[lab > 0]):
            rr, cc = np.nonzero(lab == l)
            c2 = (rr - int(center[0, l - 1, 0])) ** 2 + (cc - int(center[0, l - 1, 1])) ** 2
            e2 = d2[0][rr, cc].astype(np.int64)
            for bins in (1, 2, 3, 4, 7, 16):
                exact, flt = RR.ring_of(bins, c2, e2), RR.ring_float(bins, c2, e2)
                differ = exact != flt
                # the float form can only err where B dc / (dc + de) is an integer, which it may miss by a rounding
                tie = np.zeros(c2.shape, bool)
                for k in range(1, bins):
                    tie |= (bins - k) ** 2 * c2 == k * k * e2
                assert not (differ & ~tie).any() and (np.abs(exact - flt)[differ] == 1).all(), (seed, l, bins)
                assert (exact[c2 == 0] == 0).all() and exact.max() <= bins - 1
                checked += c2.size
                ties += int(tie.sum())
    assert checked > 20000 and ties > 0
    # an exact multiple belongs to the outer ring: dc = de at B = 2, dc = 3 de at B = 4
    assert RR.ring_of(2, np.array([9]), np.array([9]))[0] == 1 and RR.ring_of(4, np.array([81]), np.array([9]))[0] == 3
    assert RR.ring_of(4, np.array([80]), np.array([9]))[0] == 2 and RR.ring_of(16, np.array([2 * 4095 ** 2]), np.array([1]))[0] == 15


def test_straight_line_and_propagated_distance_differ_on_a_u_shape():
    """The one deliberate difference from CellProfiler: C2 is taken along the straight line, CellProfiler's along paths inside
    the object.  In the centre's own arm the two agree; across the gap the straight line is shorter, so those pixels fall into
    inner rings."""
    lab = RR.u_shape()
    own = lab > 0
    geom, center, ring, edge, d2 = RR.measure(np.zeros((1,) + lab.shape, np.uint8), lab[None], bins=4)
    rc, cc = int(center[0, 0, 0]), int(center[0, 0, 1])
    assert (rc, cc, int(center[0, 0, 2])) == (3, 3, 9)                    # the first of the deepest pixels: the top of the left arm
    rr, cc_ = np.nonzero(own)
    straight = np.sqrt((rr - rc) ** 2 + (cc_ - cc) ** 2)
    inside = RR.geodesic_c2(own, rc, cc)[rr, cc_]
    assert np.isfinite(inside).all() and (inside >= straight - 1e-9).all()
    same_column = cc_ == cc
    assert np.allclose(inside[same_column], straight[same_column])       # the segment stays inside: the same distance
    far_arm = (cc_ >= 13) & (rr <= 5)                                     # the top of the other arm: 10 to 14 px across the gap, 34 to 39 px round it
    assert (inside[far_arm] > 2 * straight[far_arm]).all()
    e2 = d2[0][rr, cc_].astype(np.float64)
    ring_straight = RR.ring_of(16, (rr - rc) ** 2 + (cc_ - cc) ** 2, d2[0][rr, cc_].astype(np.int64))
    ring_inside = np.minimum(np.floor(16 * inside / (inside + np.sqrt(e2))), 15).astype(np.int64)
    assert (ring_inside >= ring_straight).all() and (ring_inside[far_arm] > ring_straight[far_arm]).any()
    assert np.array_equal(ring_inside[same_column], ring_straight[same_column])


# ---- the floats ---------------------------------------------------------------------------------------------------------------------------
def test_derived_floats_against_the_decimal_form():
    worst = {"ratio": 0.0, "root": 0.0}
    n_obj = 0
    scenes = [(IR.noise((2, 48, 100), 3, np.uint16, 5), np.stack([IR.disks((48, 100), 14, k) for k in (1, 2)]), 4),
              (IR.noise((2, 40, 64), 2, np.uint8, 7, spread=9), np.stack([IR.disks((40, 64), 7, k, radii=(3, 8)) for k in (3, 4)]), 16),
              (IR.noise((2, 30, 30), 1, np.uint16, 8, base=65000), np.stack([IR.disks((30, 30), 3, k, radii=(4, 9)) for k in (5, 6)]), 7)]
    for image, lab, bins in scenes:
        tables = RR.measure(image, lab, bins=bins)[:4]
        t = RA.radial_table(*tables)
        d = RR.derive(*tables)
        assert all(np.array_equal(getattr(t, k), v, equal_nan=v.dtype.kind == "f") for k, v in d.items())
        assert np.array_equal(t.ring[..., 0].sum(axis=(1, 2)), t.area) and np.array_equal(t.geom[:, 0], t.area)
        exact = RR.derive_exact(*tables)
        n_obj += len(exact)
        for k, o in enumerate(exact):
            for r in range(bins):
                for ch in range(image.shape[3]):
                    for field, key, root in (("frac_at_d", "frac_at_d", False), ("mean_frac", "mean_frac", False), ("radial_cv", "radial_cv2", True)):
                        x, f = float(getattr(t, field)[k, r, ch]), o[key][r][ch]
                        assert (f is None) == math.isnan(x), (field, k, r, ch)
                        if f is not None:
                            which = "root" if root else "ratio"
                            worst[which] = max(worst[which], rel(x, RR.to_decimal(f, root)))
            for ch in range(image.shape[3]):
                worst["ratio"] = max(worst["ratio"], rel(float(t.edge_mean[k, ch]), RR.to_decimal(o["edge_mean"][ch])))
                worst["root"] = max(worst["root"], rel(float(t.edge_std[k, ch]), RR.to_decimal(o["edge_var"][ch], True)))
            assert abs(np.nansum(t.frac_at_d[k, :, 0]) - 1.0) < 1e-12
    print(f"objects {n_obj}: worst relative error of the quotients {worst['ratio'] / U:.3f} u, of the roots {worst['root'] / U:.3f} u")
    assert n_obj > 40 and 0.0 < worst["ratio"] <= RATIO_BOUND and 0.0 < worst["root"] <= ROOT_BOUND


def test_closed_forms_and_nans():
    # a uniform disk-like square: every ring's mean_frac is 1, every radial_cv 0; a dark object: NaN throughout
    lab = np.zeros((1, 21, 21), np.int32)
    lab[0, 2:19, 2:19] = 1
    image = np.full((1, 21, 21, 2), 100, np.uint8)
    image[..., 1] = 0
    t = RA.radial_table(*RR.measure(image, lab, bins=4)[:4])
    assert t.center_rc.tolist() == [[10, 10]] and t.max_d2.tolist() == [81] and t.edge_count.tolist() == [64]
    assert np.array_equal(t.mean_frac[0, :, 0], np.ones(4)) and np.array_equal(t.radial_cv[0, :, 0], np.zeros(4))
    assert np.isnan(t.frac_at_d[0, :, 1]).all() and np.isnan(t.mean_frac[0, :, 1]).all() and np.isnan(t.radial_cv[0, :, 1]).all()
    assert t.edge_mean.tolist() == [[100.0, 0.0]] and t.edge_std.tolist() == [[0.0, 0.0]] and t.edge_min.tolist() == [[100, 0]]
    assert t.ring[0, 0, :, 0].sum() > 0 and RR.ring_of(4, np.array([0]), np.array([81]))[0] == 0          # the centre itself: ring 0
    # a ring without pixels: a single pixel at 4 bins has rings 1..3 empty
    one = np.zeros((1, 3, 3), np.int32)
    one[0, 1, 1] = 1
    t = RA.radial_table(*RR.measure(np.full((1, 3, 3), 7, np.uint8), one, bins=4)[:4])
    assert t.frac_at_d[0, :, 0].tolist()[0] == 1.0 and t.frac_at_d[0, 1:, 0].tolist() == [0.0] * 3 and np.isnan(t.mean_frac[0, 1:, 0]).all()
    assert np.isnan(t.radial_cv[0, 1:, 0]).all() and t.radial_cv[0, 0, 0] == 0.0 and t.edge_integrated.tolist() == [[7]]
    # wedges: the eight around a centre given by the caller
    full = np.ones((1, 5, 5), np.int32)
    w = RR.measure(np.ones((1, 5, 5), np.uint8), full, bins=1, centers=np.array([[[2, 2]]], np.int32))[2][0, 0, 0, :, 0]
    assert w.tolist() == [6, 3, 5, 3, 3, 3, 1, 1] and w.sum() == 25      # the centre's row and column and the diagonals fall to the lower wedges
    with pytest.raises(RR.TooDeep):
        RR.measure(np.zeros((1, 255, 255), np.uint8), np.ones((1, 255, 255), np.int32))


# ---- the package's argument checks ------------------------------------------------------------------------------------------------------
def test_measurer_refusals_before_a_handle_exists():
    """RadialMeasurer refuses what IntensityMeasurer refuses, with the same exceptions, before either makes a handle."""
    import torch

    import cellscreen
    from cellscreen import intensity as IN
    assert cellscreen.RadialMeasurer is RA.RadialMeasurer and cellscreen.RadialTable is RA.RadialTable
    assert cellscreen.radial_table is RA.radial_table and cellscreen.radial_params is RA.radial_params
    assert RA.RadialMeasurer.MAX_D2 == RA.MAX_D2 == RR.MAX_D2 == 127 * 127 and RA.RadialMeasurer.MAX_BINS == RR.MAX_BINS == 16
    m, s = RA.RadialMeasurer(0), IN.IntensityMeasurer(0)
    lab = np.zeros((2, 8, 12), np.int32)
    img = np.zeros((2, 8, 12, 3), np.uint8)
    for image, labels, kw, exc in (
            (img.astype(np.float32), lab, {}, TypeError), (img.astype(np.int16), lab, {}, TypeError), (img, lab.astype(np.int64), {}, TypeError),
            (list(img), lab, {}, TypeError), (img, list(lab), {}, TypeError), (img, torch.zeros((2, 8, 12), dtype=torch.int32), {}, TypeError),
            (img[0], lab, {}, ValueError), (img, lab[0], {}, ValueError), (img[:, :4], lab, {}, ValueError), (img, lab[:, :, ::2], {}, ValueError),
            (img, lab, dict(exclude=lab[:1]), ValueError),
            (img, lab, dict(exclude=lab.astype(np.uint8)), TypeError), (np.zeros((1, 2, 4097, 2), np.uint8), np.zeros((1, 2, 4097), np.int32), {}, ValueError),
            (np.zeros((0, 4, 4, 2), np.uint8), np.zeros((0, 4, 4), np.int32), {}, ValueError), (np.zeros((2, 8, 12, 5), np.uint8), lab, {}, ValueError),
            (img, lab, dict(max_label=0), ValueError), (img, lab, dict(max_label=2.0), TypeError), (img, lab, dict(max_label=True), TypeError),
            (img, lab, dict(max_label=(1 << 20) + 1), ValueError), (img, lab, dict(max_label=1 << 20), ValueError)):       # 2 x 2^20 x 3 cells
        for call in (m.measure_batch, m.measure_dense, s.measure_dense):
            with pytest.raises(exc):
                call(image, labels, **kw)
    ctr = np.zeros((2, 4, 2), np.int32)
    for kw, exc in ((dict(bins=0), ValueError), (dict(bins=17), ValueError), (dict(bins=-1), ValueError), (dict(bins=4.0), TypeError),
                    (dict(bins=True), TypeError), (dict(bins=None), TypeError), (dict(centers=ctr.astype(np.int64)), TypeError),
                    (dict(centers=ctr.tolist()), TypeError), (dict(centers=torch.zeros((2, 4, 2), dtype=torch.int32)), TypeError),
                    (dict(centers=ctr[:1]), ValueError), (dict(centers=ctr[:, :3]), ValueError), (dict(centers=ctr[..., :1]), ValueError),
                    (dict(centers=np.zeros((2, 4, 4), np.int32)[..., ::2]), ValueError), (dict(centers=ctr - 1), ValueError),
                    (dict(centers=ctr + np.array([8, 0], np.int32)), ValueError), (dict(centers=ctr + np.array([0, 12], np.int32)), ValueError)):
        for call in (m.measure_batch, m.measure_dense):
            with pytest.raises(exc):
                call(img, lab, max_label=4, **kw)
    with pytest.raises(ValueError, match="split the batch"):             # 2^18 x 16 x 8 x 5 x 8 bytes is above 1 GiB
        m.measure_dense(np.zeros((1, 1, 1, 4), np.uint8), np.zeros((1, 1, 1), np.int32), max_label=1 << 18, bins=16)
    assert m._pre is None and s._pre is None
    p = RA.radial_params()
    assert (p.bins, p.reserved) == (4, 0) and C.sizeof(p) == 8 and RA.radial_params(np.int64(16)).bins == 16
    with pytest.raises(ValueError):
        RA.RadialMeasurer(1, extractor=type("E", (), {"device_id": 0})())
    with pytest.raises(TypeError):
        RA.radial_table(np.zeros((1, 1, 3), np.int32), np.zeros((1, 1, 4), np.int32), np.zeros((1, 1, 4, 8, 2), np.int64), np.zeros((1, 1, 1, 4), np.int64))
    with pytest.raises(ValueError):
        RA.radial_table(np.zeros((1, 1, 3), np.int64), np.zeros((1, 1, 4), np.int32), np.zeros((1, 1, 4, 8, 3), np.int64), np.zeros((1, 1, 1, 4), np.int64))
    m.close()
    s.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
SYMBOLS = {"cs_label_radial": 19, "cs_label_radial_last_timing": 4}


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2 and lib.cs_profile_kernel_count() == 13
    raw = C.CDLL(L.LIB_PATH)
    for name, n_args in SYMBOLS.items():
        assert hasattr(raw, name) and name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == n_args, name
    assert [f[0] for f in L.CSRadialParams._fields_] == ["bins", "reserved"] and C.sizeof(L.CSRadialParams) == 8


def test_the_prototypes_are_in_the_header():
    with open(os.path.join(ROOT, "include", "cellscreen.h")) as f:
        text = " ".join(f.read().split())
    assert ("int cs_label_radial(cs_preproc *p, const void *image, int pixel_type, int32_t channels, const int32_t *labels, "
            "const int32_t *exclude /* or NULL */, int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, "
            "const cs_radial_params *params, const int32_t *centers /* or NULL */, int64_t *geom, int32_t *center, int64_t *ring, "
            "int64_t *edge, uint16_t *d2 /* or NULL */, int out_kind);") in text
    assert "int cs_label_radial_last_timing(const cs_preproc *p, double *columns_ms, double *rows_ms, double *bins_ms);" in text
    assert "typedef struct cs_radial_params { int32_t bins; /* 1..CS_RADIAL_MAX_BINS */ int32_t reserved; /* must be 0 */ } cs_radial_params;" in text
    assert f"#define CS_RADIAL_MAX_D2 {RA.MAX_D2} " in text and f"#define CS_RADIAL_MAX_BINS {RA.MAX_BINS}" in text
    assert "#define CS_ABI_VERSION 2 " in text and " * cs_label_radial " in text
    assert "(B - k)^2 * C2 >= k^2 * E2" in text and "(r > rc) + 2 * (c > cc) + 4 * (|r - rc| > |c - cc|)" in text   # the rule is stated there
    # the ctypes signature follows the prototype: pointers, ints and int32 in the header's order
    proto = text[text.index("int cs_label_radial(") + len("int cs_label_radial("):]
    proto = proto[:proto.index(");")]
    kinds = []
    for arg in proto.split(","):
        arg = arg.replace("/* or NULL */", "").strip()
        kinds.append("ptr" if "*" in arg else "i32" if arg.startswith("int32_t") else "int")
    want = {"ptr": (L._P, C.POINTER(L.CSRadialParams)), "i32": (C.c_int32,), "int": (L._I,)}
    sig = L.SIGNATURES["cs_label_radial"][1]
    assert len(sig) == len(kinds) == 19 and all(s in want[k] for s, k in zip(sig, kinds)) and sig[11] is C.POINTER(L.CSRadialParams)


def _call(lib, image=True, labels=True, params=True, geom=True, center=True, ring=True, edge=True, ptype=1, channels=2, B=1, H=8, W=8, in_kind=0,
          out_kind=0, max_label=4, bins=4, reserved=0, centers=None):
    a = np.zeros(64, np.int64)                                           # never read: every call here ends before the device
    p = a.ctypes.data
    prm = L.CSRadialParams()
    prm.bins, prm.reserved = bins, reserved
    ctr = None if centers is None else np.ascontiguousarray(centers, np.int32)
    rc = lib.cs_label_radial(None, p if image else None, ptype, channels, p if labels else None, None, B, H, W, in_kind, max_label,
                             C.byref(prm) if params else None, None if ctr is None else ctr.ctypes.data, p if geom else None,
                             p if center else None, p if ring else None, p if edge else None, None, out_kind)
    return rc, lib.cs_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_the_handle():
    lib = L.load_library()
    inside = np.zeros((4, 2), np.int32)
    for over, status in ((dict(image=False), -1), (dict(labels=False), -1), (dict(params=False), -1), (dict(geom=False), -1), (dict(center=False), -1),
                         (dict(ring=False), -1), (dict(edge=False), -1), (dict(ptype=2), -1), (dict(in_kind=2), -1), (dict(out_kind=-1), -1),
                         (dict(channels=0), -1), (dict(B=0), -1), (dict(H=0), -1), (dict(W=-1), -1), (dict(max_label=0), -1),
                         (dict(channels=5), -6), (dict(bins=0), -1), (dict(bins=-3), -1), (dict(reserved=1), -1), (dict(bins=17), -6),
                         (dict(H=4097), -6), (dict(W=4097), -6), (dict(B=65536), -6), (dict(max_label=(1 << 20) + 1), -6),
                         (dict(B=3, max_label=1 << 20), -6), (dict(channels=4, bins=16, max_label=1 << 18), -6),
                         (dict(centers=inside + np.array([8, 0], np.int32)), -1), (dict(centers=inside + np.array([0, 8], np.int32)), -1),
                         (dict(centers=inside - 1), -1)):
        rc, text = _call(lib, **over)
        assert rc == status and text, over
    # the order of the rules: the earlier one answers
    for over, status in ((dict(channels=0, H=4097), -1), (dict(channels=5, max_label=0), -1), (dict(channels=5, bins=0), -6), (dict(bins=0, H=4097), -1),
                         (dict(bins=17, reserved=1), -1), (dict(bins=17, H=4097), -6), (dict(H=4097, centers=inside - 1), -6),
                         (dict(channels=4, bins=16, max_label=1 << 18, centers=np.full((1 << 18, 2), -1, np.int32)), -6)):
        assert _call(lib, **over)[0] == status, over
    assert "at most 4 are measured per call" in _call(lib, channels=5)[1] and "at most 16 rings" in _call(lib, bins=17)[1]
    assert "split the batch" in _call(lib, channels=4, bins=16, max_label=1 << 18)[1] and "outside the image" in _call(lib, centers=inside - 1)[1]
    assert "reserved must be 0" in _call(lib, reserved=1)[1]
    assert lib.cs_label_radial_last_timing(None, None, None, None) == -1


def test_a_null_handle_reports_no_device_for_valid_arguments():
    lib = L.load_library()
    no_dev = lib.cs_device_count() <= 0
    for over in (dict(), dict(channels=1), dict(channels=4), dict(ptype=0), dict(bins=1), dict(bins=16), dict(centers=np.zeros((4, 2), np.int32)),
                 dict(centers=np.full((4, 2), 7, np.int32)), dict(B=2, max_label=1 << 20, channels=1, bins=1), dict(in_kind=1, out_kind=1),
                 dict(H=4096, W=4096), dict(channels=4, bins=16, max_label=(1 << 18) - (1 << 16))):
        rc, text = _call(lib, **over)
        assert rc == (-4 if no_dev else -1) and (not no_dev or "gfx950" in text or "device" in text), over
