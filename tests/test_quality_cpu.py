"""CPU tests of the image and per-object focus and saturation records (cs_image_quality, cs_object_focus, cellscreen/quality.py,
DESIGN 3zh): the restatement of tests/quality_reference.py against its slow form, against SciPy's record in
tests/golden/golden_quality.npz and against closed forms, the mesh's grid rule against CellProfiler's float form, the values the
package derives from the integers, and the wrapper's and the C ABI's refusals before any device work.  Integers are compared
exactly; a derived float must equal float(Fraction) of its integers, bit for bit."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import intensity_reference as IR
import quality_reference as QR
from cellscreen import _lib as L
from cellscreen import quality as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_quality.npz")


def same(a, b):
    """Equal floats, NaN equal to NaN."""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_slow_form():
    for k, (shape, nc, dt, tile) in enumerate((((1, 1), 1, np.uint8, 0), ((2, 5), 2, np.uint16, 16), ((3, 3), 1, np.uint16, 0),
                                               ((3, 4), 3, np.uint8, 16), ((5, 7), 4, np.uint16, 0), ((19, 35), 2, np.uint16, 16),
                                               ((18, 40), 1, np.uint8, 17))):
        image = QR.noise((2,) + shape, nc, dt, 30 + k)
        sat = [QR.top_of(dt) - 3 * c for c in range(nc)]
        r, m = QR.measure_image(image, tile, sat)
        r2, m2 = QR.measure_image_slow(image, tile, sat)
        assert r.dtype == np.int64 and r.shape == (2, nc, 13) and np.array_equal(r, r2), shape
        assert (m is None and m2 is None) if tile == 0 else (m.dtype == np.int64 and np.array_equal(m, m2)), shape
        if shape[0] < 3 or shape[1] < 3:
            assert not r[:, :, 8:].any()                                  # no interior: n_int and every focus sum are 0
    r, m = QR.measure_image(QR.noise((1, 9, 11), 1, np.uint8, 1)[..., 0])  # [B,H,W] is one channel
    assert r.shape == (1, 1, 13) and m is None and r[0, 0, 0] == 99 and r[0, 0, 8] == 7 * 9


def test_golden_file_matches():
    g = np.load(GOLDEN)
    assert str(g["scipy_version"]) == "1.15.3" and int(g["n_cases"]) == 4 and os.path.getsize(GOLDEN) < 100_000
    dtypes = set()
    for i in range(int(g["n_cases"])):
        name = str(g[f"name_{i}"])
        image, labels, ex, sat, tile = g[f"image_{i}"], g[f"labels_{i}"], g[f"exclude_{i}"], g[f"sat_{i}"], int(g[f"tile_{i}"])
        dtypes.add((image.dtype.name, image.shape[2]))
        rec, mesh = QR.measure_image(image[None], tile, sat)
        assert np.array_equal(rec[0], g[f"image_rec_{i}"]), name
        assert np.array_equal(mesh[0], g[f"mesh_{i}"]), name              # SciPy's sums over CellProfiler's float grid
        geom, focus = QR.measure_objects(image[None], labels[None], ex[None])
        index = g[f"index_{i}"]
        assert np.array_equal(np.nonzero(geom[0, :, 0])[0] + 1, index) and np.array_equal(focus[0][index - 1], g[f"focus_{i}"]), name
        assert np.array_equal(geom, IR.measure(image[None], labels[None], ex[None])[0]), name     # cs_label_intensity's geom
    assert dtypes == {("uint16", 3), ("uint16", 1), ("uint8", 4), ("uint8", 2)}


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_closed_forms(dtype):
    H, W, top = 21, 30, QR.top_of(dtype)
    n, n_int = H * W, (H - 2) * (W - 2)
    r = QR.measure_image(np.full((1, H, W), 7, dtype))[0][0, 0]
    assert r.tolist() == [n, 7 * n, 49 * n, 7, 7, n, n, 0, n_int, 0, 0, 0, 0]              # a constant plane: every focus sum 0
    ramp = (3 * np.arange(H)[:, None] + 2 * np.arange(W)[None, :]).astype(dtype)[None]      # v = 3 r + 2 c <= 118
    r = QR.measure_image(ramp)[0][0, 0]
    g = (8 * 2) ** 2 + (8 * 3) ** 2                                                        # Sobel: 8 times the slope, either axis
    assert r[8:].tolist() == [n_int, 0, 0, g * n_int, (16 + 36) * n_int]
    _, lap, gg, br = QR.focus_planes(ramp[0])
    assert not lap.any() and (gg[1:-1, 1:-1] == g).all() and (br[1:-1, 1:-1] == 52).all()
    inside, lap, gg, br = QR.focus_planes(QR.checkerboard((H, W), dtype))
    assert (np.abs(lap[inside]) == 4 * top).all() and not gg.any() and not br.any()
    r = QR.measure_image(QR.checkerboard((1, H, W)[1:], dtype)[None])[0][0, 0]
    assert r[8:].tolist() == [n_int, 0, 16 * top * top * n_int, 0, 0] and r[3:7].tolist() == [0, top, n // 2, n // 2]
    assert r[7] == n // 2                                                                  # the top is the default level
    inside, lap, gg, br = QR.focus_planes(QR.stripes4((H, W), dtype))
    assert (gg[inside] == 16 * top * top).all() and (np.abs(lap[inside]) == top).all() and (br[inside] == top * top).all()


def test_grid_rule_equals_cellprofilers_float_form():
    for tile in (16, 17, 100, 256):
        for side in range(1, 4097):
            m = -(-side // tile)
            i = np.arange(side, dtype=np.int64)
            float_form = (i * float(m) / float(side)).astype(np.int64)     # int(i * float(m) / float(side)), truncation of >= 0
            got = QR.tile_index(side, m)
            assert np.array_equal(got, float_form), (tile, side)
            counts = np.bincount(got, minlength=m)
            assert counts.min() >= 1 and counts.max() <= tile, (tile, side)


def test_tile_records_sum_to_the_image_record():
    for k, (shape, tile) in enumerate((((130, 515), 16), ((130, 515), 17), ((130, 515), 64), ((130, 515), 256), ((40, 16), 16))):
        image = QR.noise((2,) + shape, 2, np.uint16, 40 + k)
        rec, mesh = QR.measure_image(image, tile)
        assert mesh.shape[2:4] == QR.mesh_dims(*shape, tile)
        assert np.array_equal(mesh.sum(axis=(2, 3)), rec[:, :, [0, 1, 2, 8, 9, 10, 11, 12]])
        assert np.array_equal(rec, QR.measure_image(image)[0])            # the image record does not depend on the mesh


# ---- the derived values ---------------------------------------------------------------------------------------------------------
def F(num, den):
    return float(Fraction(int(num), int(den))) if den else math.nan


def test_every_derived_float_is_one_rounded_quotient():
    image = QR.noise((2, 37, 50), 3, np.uint16, 50)
    image[1, :, :, 2] = 0                                                  # sum v = 0: focus_score NaN, its tiles left out
    rec, mesh = QR.measure_image(image, 16, [65535, 30000, 0])
    t = Q.image_quality_table(rec, mesh, 16)
    assert isinstance(t, Q.ImageQualityTable) and len(t) == 2 and t.tile == 16 and t.mesh is mesh and t.records is rec
    assert t.n.tolist() == [37 * 50] * 2 and t.n_interior.tolist() == [35 * 48] * 2
    for b in range(2):
        for c in range(3):
            n, sv, sv2, lo, hi, n_lo, n_hi, n_sat, ni, sl, sl2, sg, sbr = (int(x) for x in rec[b, c])
            assert t.mean[b, c] == F(sv, n) and QR.is_rounded_sqrt(float(t.std[b, c]), n * sv2 - sv * sv, n * n)     # one rounding
            assert same(t.focus_score[b, c], F(n * sv2 - sv * sv, n * sv))
            assert t.laplacian_variance[b, c] == F(ni * sl2 - sl * sl, ni * ni)
            assert t.tenengrad[b, c] == F(sg, ni) and t.brenner[b, c] == F(sbr, ni)
            assert t.percent_minimal[b, c] == F(100 * n_lo, n) and t.percent_maximal[b, c] == F(100 * n_hi, n)
            assert t.percent_saturated[b, c] == F(100 * n_sat, n) and (t.min[b, c], t.max[b, c]) == (lo, hi)
            d = QR.derive_record(n, sv, sv2, ni, sl, sl2, sg, sbr)
            for k, v in d.items():
                assert same(getattr(t, k)[b, c], v), k
            for r in range(mesh.shape[2]):
                for q in range(mesh.shape[3]):
                    d = QR.derive_record(*mesh[b, c, r, q])
                    for k, v in d.items():
                        assert same(getattr(t, "tile_" + k)[b, c, r, q], v), k
            assert same(t.local_focus_score[b, c], QR.local_focus_score(mesh[b, c]))
    assert math.isnan(t.focus_score[1, 2]) and math.isnan(t.local_focus_score[1, 2]) and t.percent_saturated[1, 2] == 100.0
    assert t.percent_minimal[1, 2] == 100.0 and t.percent_maximal[1, 2] == 100.0
    # local_focus_score by hand: three tiles with nv = 1, 3, (dark), 8 -> median 3, variance 26 / 3 of (1, 3, 8) around 4
    tiles = np.zeros((4, 8), np.int64)
    for i, (n, sv, sv2) in enumerate(((2, 2, 4), (2, 4, 20), (5, 0, 0), (2, 8, 96))):     # (n sv2 - sv^2) / (n sv) = 1, 3, -, 8
        tiles[i, :3] = n, sv, sv2
    assert QR.local_focus_score(tiles) == float(Fraction(26, 9)) == Q._local_focus(tiles)
    tiles[:, 2] = tiles[:, 1] ** 2 // np.maximum(tiles[:, 0], 1)          # every tile flat: the median is 0
    assert Q._local_focus(tiles) == 0.0 == QR.local_focus_score(tiles)
    # the largest sums: n_int * sum L^2 is near 2^84
    big = np.zeros((1, 1, 13), np.int64)
    n, top = 1 << 24, 65535
    ni = 4094 * 4094
    big[0, 0] = n, n * top // 2, n * top * top // 2, 0, top, n // 2, n // 2, n // 2, ni, 0, 16 * top * top * ni, 0, 0
    t = Q.image_quality_table(big)
    assert t.laplacian_variance[0, 0] == float(16 * top * top) and t.mean[0, 0] == F(n * top // 2, n) and t.mesh is None
    assert t.local_focus_score is None and t.percent_saturated[0, 0] == 50.0
    with pytest.raises(TypeError):
        Q.image_quality_table(big.astype(np.int32))
    with pytest.raises(ValueError):
        Q.image_quality_table(big[0])
    with pytest.raises(ValueError):
        Q.image_quality_table(big, np.zeros((2, 1, 1, 1, 8), np.int64))


def test_quotients_and_roots_round_once_and_the_local_score_equals_the_fractions():
    import random
    rng, big = np.random.default_rng(7), random.Random(7)
    for _ in range(2000):                                                # the quotient: any sizes, either sign
        nb, db = (int(x) for x in rng.integers(1, 200, 2))
        num, den = big.getrandbits(nb), big.getrandbits(db) + 1          # up to 200 bits each
        for s in (1, -1):
            assert Q._ratio(s * num, den) == float(Fraction(s * num, den))
    assert math.isnan(Q._ratio(5, 0)) and math.isnan(Q._sqrt_ratio(5, 0)) and Q._sqrt_ratio(0, 9) == 0.0
    twice = 0
    for _ in range(4000):                                                # the root: held to the midpoints of its neighbours
        num, den = int(rng.integers(1, 1 << int(rng.integers(2, 63)))), int(rng.integers(1, 1 << int(rng.integers(2, 63))))
        f = Q._sqrt_ratio(num, den)
        assert QR.is_rounded_sqrt(f, num, den) and f == QR.sqrt_ratio(num, den), (num, den)
        twice += f != math.sqrt(num / den)
    assert twice > 0                                                     # cases where the root of the rounded quotient is another float
    assert Q._sqrt_ratio(1 << 200, 1 << 100) == 2.0 ** 50 and Q._sqrt_ratio(49, 4) == 3.5 and Q._sqrt_ratio(1, 1 << 300) == 2.0 ** -150
    tiles = np.zeros((256, 8), np.int64)                                 # 256 tiles of 64 x 64 pixels of uint16 noise: every denominator differs
    v = rng.integers(0, 65536, (256, 4096))
    tiles[:, 0], tiles[:, 1], tiles[:, 2] = 4096, v.sum(axis=1), (v * v).sum(axis=1)
    tiles[3, 1:3] = 0                                                    # a dark tile is left out
    assert Q._local_focus(tiles) == QR.local_focus_score(tiles) and Q._local_focus(tiles[:255]) == QR.local_focus_score(tiles[:255])


def test_nan_cases_and_the_object_table():
    for shape in ((1, 1), (2, 5), (9, 2)):
        rec, mesh = QR.measure_image(QR.noise((1,) + shape, 1, np.uint8, 3), 16)
        t = Q.image_quality_table(rec, mesh, 16)
        assert t.n_interior[0] == 0 and all(math.isnan(getattr(t, k)[0, 0]) for k in ("laplacian_variance", "tenengrad", "brenner"))
        assert math.isnan(t.tile_tenengrad[0, 0, 0, 0]) and not math.isnan(t.mean[0, 0])
    t = Q.image_quality_table(*QR.measure_image(np.zeros((1, 20, 20), np.uint16), 16), 16)
    assert math.isnan(t.focus_score[0, 0]) and math.isnan(t.local_focus_score[0, 0]) and t.std[0, 0] == 0.0 and t.tenengrad[0, 0] == 0.0
    t = Q.image_quality_table(np.zeros((0, 2, 13), np.int64), np.zeros((0, 2, 1, 1, 8), np.int64), 16)     # empty tables
    assert len(t) == 0 and t.mean.shape == (0, 2) and t.tile_mean.shape == (0, 2, 1, 1) and t.local_focus_score.shape == (0, 2)
    # objects: one to the image border (fewer interior pixels than area), one single border pixel (n_int 0: NaN), one absent
    image = QR.noise((1, 12, 15), 2, np.uint16, 4)
    lab = np.zeros((1, 12, 15), np.int32)
    lab[0, 0:4, 0:5] = 1
    lab[0, 11, 14] = 2
    lab[0, 5:8, 5:9] = 4
    geom, focus = QR.measure_objects(image, lab)
    o = Q.object_focus_table(geom, focus)
    assert isinstance(o, Q.ObjectFocusTable) and len(o) == 3 and o.label.tolist() == [1, 2, 4] and o.image.tolist() == [0, 0, 0]
    assert o.area.tolist() == [20, 1, 12] and o.n_interior.tolist() == [12, 0, 12]
    assert np.isnan(o.tenengrad[1]).all() and np.isnan(o.laplacian_variance[1]).all() and np.isnan(o.brenner[1]).all()
    for i, row in enumerate((0, 1, 3)):
        for c in range(2):
            ni, sl, sl2, sg, sbr = (int(x) for x in focus[0, row, c])
            assert same(o.laplacian_variance[i, c], F(ni * sl2 - sl * sl, ni * ni))
            assert same(o.tenengrad[i, c], F(sg, ni)) and same(o.brenner[i, c], F(sbr, ni))
    assert np.array_equal(o.geom, geom[0][[0, 1, 3]]) and np.array_equal(o.focus, focus[0][[0, 1, 3]])
    e = Q.object_focus_table(np.zeros((2, 3, 3), np.int64), np.zeros((2, 3, 1, 5), np.int64))
    assert len(e) == 0 and e.tenengrad.shape == (0, 1)
    with pytest.raises(TypeError):
        Q.object_focus_table(geom.astype(np.int32), focus)
    with pytest.raises(ValueError):
        Q.object_focus_table(geom, focus[..., :4])
    with pytest.raises(ValueError):
        QR.measure_objects(image, lab, max_label=3)


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------
def test_measurer_refusals_before_a_handle_exists():
    import torch

    import cellscreen
    assert cellscreen.ImageQualityMeasurer is Q.ImageQualityMeasurer and cellscreen.ImageQualityTable is Q.ImageQualityTable
    assert cellscreen.ObjectFocusTable is Q.ObjectFocusTable
    m = Q.ImageQualityMeasurer(0)
    img = np.zeros((2, 8, 12, 3), np.uint16)
    lab = np.zeros((2, 8, 12), np.int32)
    cpu_t = torch.zeros((2, 8, 12), dtype=torch.int32)
    for image, kw, exc in (
            (img.astype(np.float32), {}, TypeError), (img.astype(np.int16), {}, TypeError), (list(img), {}, TypeError),
            (img[0, 0], {}, ValueError), (img[..., None], {}, ValueError), (img[:0], {}, ValueError), (img[:, :, :, :0], {}, ValueError),
            (img[:, :, ::2], {}, ValueError), (img[:, :, :, :2], {}, ValueError), (np.zeros((2, 8, 12, 5), np.uint8), {}, ValueError),
            (np.zeros((1, 2, 4097), np.uint8), {}, ValueError), (np.zeros((1, 4097, 2), np.uint8), {}, ValueError),
            (torch.zeros((2, 8, 12), dtype=torch.uint8), {}, ValueError), (torch.zeros((2, 8, 12), dtype=torch.float32), {}, TypeError),
            (img, dict(tile=15), ValueError), (img, dict(tile=1025), ValueError), (img, dict(tile=-16), ValueError),
            (img, dict(tile=16.0), TypeError), (img, dict(tile=True), TypeError), (img, dict(tile=None), TypeError),
            (img, dict(sat_level=[1, 2]), ValueError), (img, dict(sat_level=[1, 2, 65537]), ValueError), (img, dict(sat_level=[1, 2, -1]), ValueError),
            (img, dict(sat_level=-1), ValueError), (img, dict(sat_level=[1, 2, 3.0]), TypeError), (img, dict(sat_level=2.5), TypeError),
            (img, dict(sat_level="255"), TypeError), (img, dict(sat_level=[1, True, 3]), TypeError),
            (img, dict(tile=8), ValueError)):
        with pytest.raises(exc):
            m.measure_batch(image, **kw)
    with pytest.raises(ValueError):                                       # the mesh cap: 2^10 images of 32 x 32 tiles and a channel more
        m._check_image(np.zeros((1 << 10, 512, 512, 2), np.uint8), 16, None)      # never touched: no page is mapped
    for image, labels, kw, exc in (
            (img.astype(np.float32), lab, {}, TypeError), (img, lab.astype(np.int64), {}, TypeError), (img, lab, dict(exclude=lab.astype(bool)), TypeError),
            (img, list(lab), {}, TypeError), (img[0], lab, {}, ValueError), (img, lab[0], {}, ValueError), (img, lab[:, :, :11], {}, ValueError),
            (img, lab, dict(exclude=lab[:1]), ValueError), (np.zeros((2, 8, 12, 5), np.uint8), lab, {}, ValueError), (img, cpu_t, {}, TypeError),
            (torch.zeros((2, 8, 12), dtype=torch.uint8), cpu_t, {}, ValueError), (img, lab, dict(max_label=0), ValueError),
            (img, lab, dict(max_label=2.0), TypeError), (img, lab, dict(max_label=(1 << 20) + 1), ValueError),
            (img, lab, dict(max_label=1 << 20), ValueError)):
        with pytest.raises(exc):
            m.measure_objects(image, labels, **kw)
    assert m._pre is None
    with pytest.raises(ValueError):
        Q.ImageQualityMeasurer(1, extractor=type("E", (), {"device_id": 0})())
    m.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
NAMES = {"cs_image_quality": 13, "cs_image_quality_last_timing": 3, "cs_object_focus": 14, "cs_object_focus_last_timing": 3}


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2 and lib.cs_profile_kernel_count() == 13
    raw = C.CDLL(L.LIB_PATH)
    for name, n_args in NAMES.items():
        assert hasattr(raw, name) and hasattr(lib, name) and name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == n_args, name


def test_the_prototypes_are_in_the_header():
    with open(os.path.join(ROOT, "include", "cellscreen.h")) as f:
        text = " ".join(f.read().split())
    assert ("int cs_image_quality(cs_preproc *p, const void *image, int pixel_type, int32_t channels, int32_t batch, int32_t height, "
            "int32_t width, int in_kind, int32_t tile, const int32_t *sat_level /* or NULL */, int64_t *records, "
            "int64_t *mesh /* or NULL */, int out_kind);") in text
    assert "int cs_image_quality_last_timing(const cs_preproc *p, double *clear_ms, double *pass_ms);" in text
    assert ("int cs_object_focus(cs_preproc *p, const void *image, int pixel_type, int32_t channels, const int32_t *labels, "
            "const int32_t *exclude /* or NULL */, int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, "
            "int64_t *geom, int64_t *focus, int out_kind);") in text
    assert "int cs_object_focus_last_timing(const cs_preproc *p, double *clear_ms, double *pass_ms);" in text
    assert "#define CS_QUALITY_RECORD 13 " in text and "#define CS_QUALITY_TILE 8 " in text and "#define CS_QUALITY_FOCUS 5 " in text
    assert "#define CS_ABI_VERSION 2 " in text


def _quality(lib, image=True, records=True, mesh=True, sat=None, ptype=1, Cn=1, B=1, H=8, W=8, in_kind=0, out_kind=0, tile=0):
    a = np.zeros(64, np.int64)                                           # never read: every call here ends before the device
    p = a.ctypes.data
    s = None if sat is None else np.array(sat, np.int32)
    rc = lib.cs_image_quality(None, p if image else None, ptype, Cn, B, H, W, in_kind, tile, None if s is None else s.ctypes.data,
                              p if records else None, p if mesh else None, out_kind)
    return rc, lib.cs_last_error().decode()


def _focus(lib, image=True, labels=True, geom=True, focus=True, exclude=False, ptype=1, Cn=1, B=1, H=8, W=8, in_kind=0, out_kind=0, max_label=4):
    a = np.zeros(64, np.int64)
    p = a.ctypes.data
    rc = lib.cs_object_focus(None, p if image else None, ptype, Cn, p if labels else None, p if exclude else None, B, H, W, in_kind,
                            max_label, p if geom else None, p if focus else None, out_kind)
    return rc, lib.cs_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_the_handle():
    lib = L.load_library()
    for over, status in ((dict(image=False), -1), (dict(records=False), -1), (dict(mesh=False, tile=16), -1), (dict(Cn=0), -1), (dict(Cn=-1), -1),
                         (dict(Cn=5), -6), (dict(in_kind=2), -1), (dict(out_kind=-1), -1), (dict(ptype=2), -1), (dict(ptype=-1), -1),
                         (dict(B=0), -1), (dict(H=0), -1), (dict(W=-1), -1), (dict(tile=15), -1), (dict(tile=1025), -1), (dict(tile=-1), -1),
                         (dict(sat=[-1]), -1), (dict(sat=[65537]), -1), (dict(Cn=2, sat=[5, 70000]), -1),
                         (dict(H=4097), -6), (dict(W=4097), -6), (dict(B=65536), -6),
                         (dict(B=1 << 10, H=512, W=512, Cn=2, tile=16), -6), (dict(B=17, H=4096, W=4096, tile=16), -6)):
        rc, text = _quality(lib, **over)
        assert rc == status and text, over
    assert "tile 15" in _quality(lib, tile=15)[1] and "channels 5: at most 4" in _quality(lib, Cn=5)[1]
    for over, status in ((dict(image=False), -1), (dict(labels=False), -1), (dict(geom=False), -1), (dict(focus=False), -1),
                         (dict(Cn=0), -1), (dict(Cn=5), -6), (dict(in_kind=2), -1), (dict(out_kind=-1), -1), (dict(ptype=2), -1),
                         (dict(B=0), -1), (dict(H=0), -1), (dict(W=-1), -1), (dict(max_label=0), -1), (dict(max_label=-5), -1),
                         (dict(max_label=(1 << 20) + 1), -6), (dict(B=5, max_label=1 << 20), -6), (dict(B=2, Cn=3, max_label=1 << 20), -6),
                         (dict(B=1 << 12, Cn=4, max_label=257), -6), (dict(H=4097), -6), (dict(W=4097), -6), (dict(B=65536), -6)):
        rc, text = _focus(lib, **over)
        assert rc == status and text, over
    assert lib.cs_image_quality_last_timing(None, None, None) == -1 and lib.cs_object_focus_last_timing(None, None, None) == -1


def test_a_null_handle_reports_no_device_for_valid_arguments():
    lib = L.load_library()
    no_dev = lib.cs_device_count() <= 0
    want = -4 if no_dev else -1                                          # no handle: no device here, else a NULL handle
    for over in (dict(), dict(mesh=False), dict(tile=16), dict(tile=1024, H=4096, W=4096), dict(ptype=0, Cn=4, sat=[0, 1, 255, 65536]),
                 dict(B=1 << 10, H=512, W=512, tile=16), dict(B=16, H=4096, W=4096, tile=16), dict(in_kind=1, out_kind=1), dict(B=65535, H=1, W=1)):
        assert _quality(lib, **over)[0] == want, over
    for over in (dict(), dict(exclude=True), dict(ptype=0, Cn=3), dict(Cn=4, max_label=1 << 20), dict(B=4, max_label=1 << 20),
                 dict(in_kind=1, out_kind=1), dict(H=4096, W=4096)):
        assert _focus(lib, **over)[0] == want, over
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            Q.ImageQualityMeasurer(0).measure_batch(np.zeros((1, 8, 8), np.uint8))
        assert ei.value.status == -4
        with pytest.raises(L.CellScreenError) as ei:
            Q.ImageQualityMeasurer(0).measure_objects(np.zeros((1, 8, 8), np.uint8), np.zeros((1, 8, 8), np.int32))
        assert ei.value.status == -4
