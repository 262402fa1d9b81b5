"""CPU tests of the per-object neighbour records (cs_label_neighbors, cellscreen/neighbors.py): the restatement of
tests/neighbors_reference.py against its slow form (all pairs of pixels) and against tests/golden/golden_neighbors.npz, whose records
come from SciPy alone (tools/make_golden_neighbors.py), its invariants, closed forms, the values the package derives against a
hand-made scene and against an object-by-object derivation, and the wrapper's and the C ABI's refusals before any device work.

Every record is an integer and is compared with np.array_equal.  Of the derived floats only the angle has a tolerance, ANGLE_ABS =
1e-12 degrees: the package takes it with numpy's arccos and degrees, the object-by-object derivation with math.acos and math.degrees
from the same quotient, each within an ulp or two of the exact value; at 180 degrees an ulp is 2.8e-14.  The square roots and the
quotients are correctly rounded on both sides and agree to the bit.  No device code is involved."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import intensity_reference as IR
import neighbors_reference as NR
from cellscreen import _lib as L
from cellscreen import neighbors as NB
from cellscreen import shape as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_neighbors.npz")
NAMES = ("geom", "objects", "offsets", "pairs")
DTYPES = (np.int64, np.int32, np.int64, np.int32)
ANGLE_ABS = 1e-12


def same(a, b, name=""):
    assert len(a) == len(b) == 4
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype == DTYPES[k] and x.shape == y.shape, (name, NAMES[k])
        assert np.array_equal(x, y), (name, NAMES[k])


def random_scenes(shape, seed, n=6):
    """labels [2,H,W]: dense and sparse random pixels of a few labels, and the generators' kinds"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        lab = rng.integers(0, 5, (2,) + shape).astype(np.int32)
        if t % 2:
            lab[rng.random(lab.shape) < 0.7] = 0
        out.append((f"random {t}", lab))
    for (name, a), (_, b) in zip(NR.contents(shape, seed), NR.contents(shape, seed + 1)):
        out.append((name, np.stack([a, b])))
    return out


def rows_of(rec):
    """{(image, label): {neighbour: (D2, n_near)}} of the records"""
    geom, objects, offsets, pairs = rec
    B, M = geom.shape[:2]
    return {(b, a): {int(nb): (int(d), int(n)) for nb, d, n in pairs[offsets[b * M + a - 1]:offsets[b * M + a]]}
            for b in range(B) for a in range(1, M + 1)}


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_d2", [1, 2, 5, 9])
def test_restatement_equals_its_slow_form(max_d2):
    for name, lab in random_scenes((12, 17), 20 + max_d2):
        same(NR.measure(lab, max_d2), NR.measure_slow(lab, max_d2), f"{name} max_d2={max_d2}")
    lab = random_scenes((12, 17), 3)[0][1]
    same(NR.measure(lab, max_d2, max_label=9), NR.measure_slow(lab, max_d2, max_label=9), "a larger max_label")
    one = np.full((1, 1, 1), 3, np.int32)
    same(NR.measure(one, max_d2), NR.measure_slow(one, max_d2), "one pixel")


def test_restatement_equals_the_golden_file():
    g = np.load(GOLDEN)
    assert "SciPy alone" in str(g["note"]) and "scikit-image and CellProfiler took no part" in str(g["note"])
    assert os.path.getsize(GOLDEN) < 100_000
    pairs_seen = 0
    for i in range(int(g["n_scenes"])):
        labels = g[f"labels_{i}"]
        assert labels.shape[1:] == (40, 60)
        for d2 in g["max_d2"].tolist():
            got = NR.measure(labels, d2)
            same(got, tuple(g[f"{k}_{i}_{d2}"] for k in NAMES), f"{g[f'name_{i}']} max_d2={d2}")
            pairs_seen += got[3].shape[0]
    assert pairs_seen > 500 and set(g["max_d2"].tolist()) >= {1, 2, 25, 1000, 1024}


def test_invariants_on_random_scenes():
    for name, lab in random_scenes((23, 31), 5, n=4):
        image = np.zeros(lab.shape, np.uint8)
        before = None
        for max_d2 in (1, 2, 4, 8, 13, 50):
            rec = NR.measure(lab, max_d2)
            geom, objects, offsets, pairs = rec
            rows = rows_of(rec)
            assert np.array_equal(geom, IR.measure(image, lab)[0]), name                 # cs_label_intensity's geom
            assert offsets[0] == 0 and offsets[-1] == pairs.shape[0] and (np.diff(offsets) >= 0).all()
            assert np.array_equal(np.diff(offsets).reshape(objects.shape[:2]), objects[:, :, 2])      # degree = row length
            assert (objects[:, :, 1] <= objects[:, :, 0]).all() and (objects[:, :, 0] <= geom[:, :, 0]).all()
            assert ((geom[:, :, 0] > 0) == (objects[:, :, 0] > 0)).all()                 # every object has a border pixel
            for (b, a), row in rows.items():
                assert list(row) == sorted(row), name                                    # sorted by neighbour label, no label twice
                assert sum(n for _, n in row.values()) == objects[b, a - 1, 1]           # the n_near of a row sum to touching
                for nb, (d, _) in row.items():
                    assert nb != a and 1 <= d <= max_d2 and rows[(b, nb)][a][0] == d, name           # symmetric, with equal D2
            if before is not None:                                                       # a larger distance keeps every neighbour, and its D2
                for key, row in before.items():
                    assert all(nb in rows[key] and rows[key][nb][0] == d for nb, (d, _) in row.items()), name
            before = rows


def test_border_is_shapes_border_pixel():
    """`border` counts cs_label_shape's border pixels: the three perimeter classes plus the border pixels in none, not
    `perim` itself."""
    import shape_reference as SR
    for name, lab in random_scenes((23, 31), 8, n=2):
        _, objects, _, _ = NR.measure(lab, 1)
        perim = SR.measure(lab, hull=False)[3]
        assert (perim.sum(axis=2) <= objects[:, :, 0]).all(), name
        for b in range(lab.shape[0]):
            mask = NR.border_mask(lab[b])
            assert np.array_equal(np.bincount(lab[b][mask], minlength=objects.shape[1] + 1)[1:], objects[b, :, 0])
    full = np.ones((1, 5, 7), np.int32)
    assert NR.measure(full, 2)[1][0, 0].tolist() == [2 * (5 + 7) - 4, 0, 0] and SR.measure(full, hull=False)[3][0, 0].tolist() == [20, 0, 0]
    dot = np.ones((1, 1, 1), np.int32)                                   # a single pixel: a border pixel in no perimeter class
    assert NR.measure(dot, 2)[1][0, 0].tolist() == [1, 0, 0] and SR.measure(dot, hull=False)[3][0, 0].tolist() == [0, 0, 0]


@pytest.mark.parametrize("gap", [0, 1, 3, 7, 31])
def test_two_rectangles_in_closed_form(gap):
    h, w = 6, 4
    lab = NR.two_rectangles(h, w, gap)
    d2 = (gap + 1) ** 2
    geom, objects, offsets, pairs = NR.measure(lab, d2)                  # max_d2 exactly D2
    border = 2 * (h + w) - 4
    assert objects[0].tolist() == [[border, h, 1], [border, h, 1]] and offsets.tolist() == [0, 1, 2]
    assert pairs.tolist() == [[2, d2, h], [1, d2, h]]
    if d2 > 1:                                                           # one below: no neighbours, nothing touches
        geom, objects, offsets, pairs = NR.measure(lab, d2 - 1)
        assert objects[0].tolist() == [[border, 0, 0], [border, 0, 0]] and offsets.tolist() == [0, 0, 0] and pairs.shape == (0, 3)
    same(NR.measure(lab, d2), NR.measure_slow(lab, d2), "slow")


def test_an_object_between_two_others_does_not_hide_them():
    lab = np.zeros((1, 9, 12), np.int32)
    lab[0, 2:7, 1:3] = 1
    lab[0, 3:6, 4:6] = 2                                                 # between 1 and 3
    lab[0, 2:7, 7:9] = 3
    rows = rows_of(NR.measure(lab, 25))
    assert rows[(0, 1)] == {2: (4, 10), 3: (25, 0)} and rows[(0, 3)] == {1: (25, 0), 2: (4, 10)}       # all ten pixels are border pixels
    assert rows[(0, 2)] == {1: (4, 3), 3: (4, 3)}                        # 2's left column looks at 1, its right column at 3
    assert 3 not in rows_of(NR.measure(lab, 24))[(0, 1)]
    same(NR.measure(lab, 25), NR.measure_slow(lab, 25))


# ---- the package's host half --------------------------------------------------------------------------------------------------------
def test_derive_on_a_hand_made_scene():
    lab = np.zeros((2, 12, 16), np.int32)
    lab[0, 1:4, 1:4] = 1                                                 # centroid (2, 2)
    lab[0, 1:4, 5:8] = 2                                                 # (2, 6): 4 right of 1
    lab[0, 7:10, 1:4] = 4                                                # (8, 2): 6 below 1
    lab[1, 5, 5] = 3                                                     # alone in its image
    rec = NR.measure(lab, 4, max_label=5)
    t = NB.neighbor_table(*rec)
    assert len(t) == 4 and t.image.tolist() == [0, 0, 0, 1] and t.label.tolist() == [1, 2, 4, 3]
    assert t.area.tolist() == [9, 9, 9, 1] and t.centroid.tolist() == [[2.0, 2.0], [2.0, 6.0], [8.0, 2.0], [5.0, 5.0]]
    assert t.border.tolist() == [8, 8, 8, 1] and t.touching.tolist() == [3, 3, 0, 0] and t.number_of_neighbors.tolist() == [1, 1, 0, 0]
    assert t.percent_touching.tolist() == [37.5, 37.5, 0.0, 0.0]
    assert t.nearest_edge_label.tolist() == [2, 1, 0, 0] and t.nearest_edge_distance[:2].tolist() == [2.0, 2.0]
    assert np.isnan(t.nearest_edge_distance[2:]).all()
    # over all objects of the image by centroid distance, neighbours or not
    assert t.first_closest_label.tolist() == [2, 1, 1, 0] and t.second_closest_label.tolist() == [4, 4, 2, 0]
    assert t.first_closest_distance[:3].tolist() == [4.0, 4.0, 6.0] and np.isnan(t.first_closest_distance[3])
    assert t.second_closest_distance[:3].tolist() == [6.0, math.sqrt(52.0), math.sqrt(52.0)] and np.isnan(t.second_closest_distance[3])
    want = [90.0, math.degrees(math.acos(4.0 / math.sqrt(52.0))), math.degrees(math.acos(6.0 / math.sqrt(52.0)))]
    assert np.allclose(t.angle_between_neighbors[:3], want, rtol=0.0, atol=ANGLE_ABS) and np.isnan(t.angle_between_neighbors[3])
    assert [x.tolist() for x in t.neighbors_of(0)] == [[2], [4], [3]] and [x.tolist() for x in t.neighbors_of(2)] == [[], [], []]
    two = lab[:1].copy()
    two[two == 4] = 0                                                    # two objects: no second closest, no angle
    t = NB.neighbor_table(*NR.measure(two, 1))
    assert t.first_closest_label.tolist() == [2, 1] and t.second_closest_label.tolist() == [0, 0]
    assert np.isnan(t.second_closest_distance).all() and np.isnan(t.angle_between_neighbors).all() and (t.number_of_neighbors == 0).all()
    tie = np.zeros((1, 5, 9), np.int32)                                  # equal distances: the smaller label is first; 180 degrees
    tie[0, 2, 4], tie[0, 2, 1], tie[0, 2, 7] = 2, 5, 3
    t = NB.neighbor_table(*NR.measure(tie, 9))
    assert t.label.tolist() == [2, 3, 5] and t.first_closest_label.tolist() == [3, 2, 2] and t.second_closest_label.tolist() == [5, 5, 3]
    assert abs(t.angle_between_neighbors[0] - 180.0) <= ANGLE_ABS and t.angle_between_neighbors[1:].tolist() == [0.0, 0.0]
    assert t.nearest_edge_label.tolist() == [3, 2, 2]                    # 2 sees 3 and 5 at D2 9 both
    same_centroid = np.zeros((1, 5, 5), np.int32)                        # a ring around a pixel: one centroid, no angle there
    same_centroid[0, 1:4, 1:4] = 1
    same_centroid[0, 2, 2] = 2
    same_centroid[0, 0, 0] = 3
    t = NB.neighbor_table(*NR.measure(same_centroid, 1))
    assert t.first_closest_distance[:2].tolist() == [0.0, 0.0] and np.isnan(t.angle_between_neighbors[:2]).all()
    empty = NB.neighbor_table(*NR.measure(np.zeros((2, 4, 4), np.int32), 1))
    assert len(empty) == 0 and empty.pairs.shape == (0, 3) and empty.centroid.shape == (0, 2)


def test_derive_equals_the_object_by_object_derivation():
    for name, lab in random_scenes((23, 31), 11, n=2) + [("golden", np.load(GOLDEN)["labels_1"])]:
        for max_d2 in (2, 50):
            rec = NR.measure(lab, max_d2, max_label=int(lab.max()) + 2)
            d, s = NR.derive(*rec), NR.derive_slow(*rec)
            assert set(d) == set(s) == set(NR.INT_FIELDS + NR.FLOAT_FIELDS)
            for k in d:
                assert d[k].dtype == s[k].dtype and d[k].shape == s[k].shape, (name, k)
                if k == "angle_between_neighbors":
                    assert np.array_equal(np.isnan(d[k]), np.isnan(s[k])) and np.allclose(d[k], s[k], rtol=0.0, atol=ANGLE_ABS, equal_nan=True), name
                else:
                    assert np.array_equal(d[k], s[k], equal_nan=True), (name, k)
    with pytest.raises(TypeError):
        NB.neighbor_table(rec[0], rec[1].astype(np.int64), rec[2], rec[3])
    with pytest.raises(ValueError):
        NB.neighbor_table(rec[0], rec[1], rec[2], rec[3][:-1])


def test_distance_becomes_max_d2_as_the_expander_takes_it():
    from cellscreen import expand as EX
    for d in (1, 1.0, 1.5, 2, 2.9, 5, 31.99, 32, 32.0, np.float32(3.5), np.int64(7)):
        p = NB.neighbor_params(d)
        assert p.max_d2 == EX.expand_params(d).max_d2 and p.table_log2 == 0 and p.reserved == 0
    assert [NB.neighbor_params(d).max_d2 for d in (1, 1.5, 2.9, 32)] == [1, 2, 8, 1024]
    assert all(NB.neighbor_params(math.sqrt(n)).max_d2 == n for n in range(1, 1025))
    assert NB.neighbor_params(3, table_log2=10).table_log2 == 10 and C.sizeof(L.CSNeighborsParams) == 12
    for bad, exc in ((0, ValueError), (0.99, ValueError), (32.01, ValueError), (33, ValueError), (200, ValueError), (math.nan, ValueError),
                     (math.inf, ValueError), (-2, ValueError), (True, TypeError), ("3", TypeError), (None, TypeError)):
        with pytest.raises(exc):
            NB.neighbor_params(bad)
    for bad, exc in ((9, ValueError), (27, ValueError), (-1, ValueError), (12.0, TypeError), (True, TypeError)):
        with pytest.raises(exc):
            NB.neighbor_params(3, table_log2=bad)


# ---- the package's argument checks ------------------------------------------------------------------------------------------------
def test_measurer_refusals_before_a_handle_exists():
    """NeighborMeasurer refuses what ShapeMeasurer refuses, with the same exceptions, before either makes a handle."""
    import torch

    import cellscreen
    assert cellscreen.NeighborMeasurer is NB.NeighborMeasurer and cellscreen.NeighborTable is NB.NeighborTable
    assert cellscreen.neighbor_table is NB.neighbor_table and cellscreen.neighbor_params is NB.neighbor_params
    m, s = NB.NeighborMeasurer(0), SH.ShapeMeasurer(0)
    lab = np.zeros((2, 8, 12), np.int32)
    cpu_t = torch.zeros((2, 8, 12), dtype=torch.int32)
    for labels, kw, exc in (
            (lab.astype(np.int64), {}, TypeError), (lab.astype(np.uint8), {}, TypeError), (list(lab), {}, TypeError),
            (lab[0], {}, ValueError), (lab[:, :, ::2], {}, ValueError), (cpu_t, {}, ValueError), (np.zeros((1, 2, 4097), np.int32), {}, ValueError),
            (np.zeros((1, 4097, 2), np.int32), {}, ValueError), (np.zeros((0, 4, 4), np.int32), {}, ValueError),
            (lab, dict(max_label=0), ValueError), (lab, dict(max_label=-3), ValueError), (lab, dict(max_label=2.0), TypeError),
            (lab, dict(max_label=True), TypeError), (lab, dict(max_label=(1 << 20) + 1), ValueError),
            (np.zeros((5, 2, 2), np.int32), dict(max_label=1 << 20), ValueError)):                        # 5 x 2^20 rows
        for call in (m.measure_batch, m.measure_dense):
            with pytest.raises(exc):
                call(labels, 3, **kw)
        with pytest.raises(exc):
            s.measure_dense(labels, **kw)
    for bad, exc in ((0, ValueError), (33, ValueError), (math.nan, ValueError), ("2", TypeError), (False, TypeError)):
        for call in (m.measure_batch, m.measure_dense):
            with pytest.raises(exc):
                call(lab, bad)
    with pytest.raises(ValueError):
        m.measure_dense(lab, 3, table_log2=5)
    lab2 = lab.copy()
    lab2[0, 0, 0] = (1 << 20) + 1                                        # max_label=None: the labels' maximum meets the same limits
    with pytest.raises(ValueError):
        m.measure_batch(lab2, 3)
    assert m._pre is None and s._pre is None
    with pytest.raises(ValueError):
        NB.NeighborMeasurer(1, extractor=type("E", (), {"device_id": 0})())
    m.close()
    s.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
SYMBOLS = {"cs_label_neighbors": 13, "cs_label_neighbors_pairs": 4, "cs_label_neighbors_last_timing": 3, "cs_label_neighbors_last_table": 3}


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2 and lib.cs_profile_kernel_count() == 13
    raw = C.CDLL(L.LIB_PATH)
    for name, n_args in SYMBOLS.items():
        assert hasattr(raw, name) and name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == n_args, name


def test_the_prototypes_are_in_the_header():
    with open(os.path.join(ROOT, "include", "cellscreen.h")) as f:
        text = " ".join(f.read().split())
    assert ("int cs_label_neighbors(cs_preproc *p, const int32_t *labels, int32_t batch, int32_t height, int32_t width, int in_kind, "
            "int32_t max_label, const cs_neighbors_params *params, int64_t *geom, int32_t *objects, int64_t *offsets, int out_kind, "
            "int64_t *n_pairs);") in text
    assert "int cs_label_neighbors_pairs(cs_preproc *p, int32_t *pairs, int64_t capacity, int pairs_kind);" in text
    assert "int cs_label_neighbors_last_timing(const cs_preproc *p, double *scan_ms, double *rows_ms);" in text
    assert "int cs_label_neighbors_last_table(const cs_preproc *p, int32_t *table_log2, int32_t *grows);" in text
    assert "#define CS_ABI_VERSION 2 " in text and " * cs_label_neighbors / cs_label_neighbors_pairs " in text
    assert "smallest (d2, label)" in text and "max_d2 1..1024" in text                                   # the rule is stated there


def _call(lib, labels=True, params=True, geom=True, objects=True, offsets=True, n_pairs=True, B=1, H=8, W=8, in_kind=0, out_kind=0, max_label=4,
          max_d2=4, table_log2=0, reserved=0):
    a = np.zeros(64, np.int64)                                           # never read: every call here ends before the device
    p = a.ctypes.data
    prm = L.CSNeighborsParams()
    prm.max_d2, prm.table_log2, prm.reserved = max_d2, table_log2, reserved
    n = C.c_int64(-7)
    rc = lib.cs_label_neighbors(None, p if labels else None, B, H, W, in_kind, max_label, C.byref(prm) if params else None, p if geom else None,
                                p if objects else None, p if offsets else None, out_kind, C.byref(n) if n_pairs else None)
    assert n.value == -7
    return rc, lib.cs_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_the_handle():
    lib = L.load_library()
    for over, status in ((dict(labels=False), -1), (dict(params=False), -1), (dict(geom=False), -1), (dict(objects=False), -1),
                         (dict(offsets=False), -1), (dict(n_pairs=False), -1),
                         (dict(in_kind=2), -1), (dict(out_kind=-1), -1), (dict(B=0), -1), (dict(H=0), -1), (dict(W=-1), -1),
                         (dict(max_label=0), -1), (dict(max_label=-5), -1), (dict(max_d2=0), -1), (dict(max_d2=-4), -1), (dict(reserved=1), -1),
                         (dict(table_log2=9), -1), (dict(table_log2=27), -1),
                         (dict(H=4097), -6), (dict(W=4097), -6), (dict(B=65536), -6),
                         (dict(max_label=(1 << 20) + 1), -6), (dict(B=5, max_label=1 << 20), -6), (dict(B=(1 << 12) + 1, max_label=1 << 10), -6),
                         (dict(max_d2=1025), -6), (dict(max_d2=1 << 30), -6)):
        rc, text = _call(lib, **over)
        assert rc == status and text, over
    # the order of the rules: the earlier one answers
    for over, status in ((dict(labels=False, H=4097), -1), (dict(in_kind=7, H=4097), -1), (dict(H=4097, max_label=0), -1), (dict(B=0, max_label=1 << 21), -1),
                         (dict(max_d2=0, H=4097), -1), (dict(max_d2=0, max_label=1 << 21), -1), (dict(reserved=3, max_d2=1025), -1),
                         (dict(H=4097, max_d2=1025), -6)):
        assert _call(lib, **over)[0] == status, over
    assert "max_label 0: must be >= 1" in _call(lib, max_label=0)[1] and "capped at 1048576 labels per image and 4194304 rows" in _call(lib, B=5, max_label=1 << 20)[1]
    assert "max_d2 0: must be >= 1" in _call(lib, max_d2=0)[1] and "max_d2 1025: distances above 32 px" in _call(lib, max_d2=1025)[1]
    assert "sides above 4096" in _call(lib, H=4097, max_d2=1025)[1] and "reserved must be 0" in _call(lib, reserved=1)[1]
    a = np.zeros(8, np.int32)
    assert lib.cs_label_neighbors_pairs(None, None, 4, 0) == -1 and lib.cs_label_neighbors_pairs(None, a.ctypes.data, 4, 5) == -1
    assert lib.cs_label_neighbors_pairs(None, a.ctypes.data, -1, 0) == -1
    assert lib.cs_label_neighbors_last_timing(None, None, None) == -1 and lib.cs_label_neighbors_last_table(None, None, None) == -1


def test_a_null_handle_reports_no_device_for_valid_arguments():
    lib = L.load_library()
    no_dev = lib.cs_device_count() <= 0
    for over in (dict(), dict(max_d2=1), dict(max_d2=1024), dict(table_log2=10), dict(table_log2=26), dict(max_label=1 << 20), dict(B=4, max_label=1 << 20),
                 dict(B=1 << 12, max_label=1 << 10), dict(in_kind=1, out_kind=1), dict(H=4096, W=4096), dict(B=65535, H=1, W=1, max_label=64)):
        assert _call(lib, **over)[0] == (-4 if no_dev else -1), over      # no handle: no device here, else a NULL handle
    a = np.zeros(8, np.int32)
    assert lib.cs_label_neighbors_pairs(None, a.ctypes.data, 2, 0) == (-4 if no_dev else -1)
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            NB.NeighborMeasurer(0).measure_batch(np.zeros((1, 8, 8), np.int32), 2)
        assert ei.value.status == -4
