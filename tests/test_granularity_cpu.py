"""CPU tests of the per-object granularity spectrum (cs_label_granularity, cellscreen/granularity.py): the restatement
of tests/granularity_reference.py against its independent slow form by threshold decomposition, against SciPy's grey erosion and
against SciPy's record tests/golden/golden_granularity.npz; closed forms of the rule; the floats the package derives against
Fractions of the same integers; and the wrapper's and the C ABI's refusals before any device work.

The records are integers, so every comparison of records is np.array_equal.  A derived float is one quotient of two exact
integers, correctly rounded: it is compared for equality with float(Fraction)."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage as ndi

import granularity_reference as GR
import intensity_reference as IR
from cellscreen import _lib as L
from cellscreen import granularity as GA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_granularity.npz")


def tiny_planes():
    """(E, P) pairs with E <= P, few levels, small enough for the threshold decomposition"""
    out = []
    for k, shape in enumerate(((1, 1), (1, 9), (9, 1), (7, 11), (12, 12), (5, 16))):
        rng = np.random.default_rng(k)
        for levels in (2, 4, 7):
            p = rng.integers(0, levels, shape).astype(np.uint16) * 9001
            e = np.minimum(p, rng.integers(0, levels, shape).astype(np.uint16) * 9001)
            out.append((e, p))
            out.append((GR.erode(p).astype(np.uint16), p))
    return out


# ---- the restatement against its slow form and against SciPy ---------------------------------------------------------------------------
def test_reconstruction_equals_the_threshold_decomposition_on_tiny_planes():
    for e, p in tiny_planes():
        r = GR.reconstruct(e, p)
        assert np.array_equal(r, GR.reconstruct_by_thresholds(e, p))
        assert (r >= e).all() and (r <= p).all()
    # whole spectra too
    for k, shape in enumerate(((6, 9), (10, 10))):
        p = (np.random.default_rng(k).integers(0, 5, shape) * 13000).astype(np.uint16)
        assert np.array_equal(GR.spectrum_planes(p, 3), GR.spectrum_planes(p, 3, recon=GR.reconstruct_by_thresholds))


def test_erosion_equals_scipys_grey_erosion_with_reflection():
    for k, shape in enumerate(((1, 1), (1, 7), (8, 1), (9, 13), (2, 2))):
        for dtype in (np.uint8, np.uint16):
            e = IR.noise(shape, 1, dtype, k)[..., 0]
            for _ in range(3):
                want = ndi.grey_erosion(e.astype(np.int64), footprint=GR.CROSS, mode="reflect")
                e = GR.erode(e)
                assert np.array_equal(e, want)


def test_restatement_equals_scipy_on_the_golden_scenes():
    g = np.load(GOLDEN)
    assert str(g["scipy_version"]) == "1.15.3" and int(g["n_cases"]) == 4
    for i in range(int(g["n_cases"])):
        image, lab, ex = g[f"image_{i}"], g[f"labels_{i}"], g[f"exclude_{i}"]
        kw = dict(steps=int(g[f"steps_{i}"]), subsample=int(g[f"subsample_{i}"]), masked=bool(g[f"masked_{i}"]))
        geom, sums, isums, planes = GR.measure(image[None], lab[None], ex[None], **kw)
        index = g[f"index_{i}"]
        assert np.array_equal(np.flatnonzero(geom[0, :, 0]) + 1, index), str(g[f"name_{i}"])
        assert np.array_equal(planes[0], g[f"planes_{i}"]) and planes.dtype == np.uint16
        assert np.array_equal(sums[0, index - 1], g[f"sums_{i}"]) and np.array_equal(isums[0], g[f"image_sums_{i}"])
        absent = np.setdiff1d(np.arange(1, geom.shape[1] + 1), index)
        assert not sums[0, absent - 1].any()


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------
def test_a_constant_plane_has_an_all_zero_spectrum():
    lab = np.zeros((1, 9, 12), np.int32)
    lab[0, 2:7, 3:10] = 1
    for s in (1, 2, 4):
        geom, sums, isums, planes = GR.measure(np.full((1, 9, 12, 2), 777, np.uint16), lab, steps=4, subsample=s)
        assert (planes == 777).all() and (sums[0, 0] == 35 * 777).all()
        d = GA.derive(geom, sums, isums)
        assert (d["spectrum"] == 0.0).all() and (d["image_spectrum"] == 0.0).all() and (d["start_mean"] == 777.0).all()


@pytest.mark.parametrize("m", [0, 1, 2, 3])
def test_an_isolated_square_of_side_2m_plus_1_leaves_at_step_m_plus_1(m):
    side = 2 * m + 1
    image = np.zeros((1, 15, 17), np.uint16)
    image[0, 4:4 + side, 5:5 + side] = 5000
    lab = np.zeros((1, 15, 17), np.int32)
    lab[0, 1:14, 2:16] = 1
    geom, sums, isums, _ = GR.measure(image, lab, steps=6)
    d = GA.derive(geom, sums, isums)
    want = [100.0 if k == m + 1 else 0.0 for k in range(1, 7)]            # the cross takes a square of side 2m + 1 away in m + 1 erosions
    assert d["spectrum"][0, :, 0].tolist() == want and d["image_spectrum"][0, :, 0].tolist() == want
    assert sums[0, 0, :, 0].tolist() == [side * side * 5000] * (m + 1) + [0] * (6 - m)


def test_sums_do_not_increase_and_the_spectrum_stays_within_100():
    shape = (23, 31)
    lab = np.stack([IR.disks(shape, 6, 1), IR.disks(shape, 6, 2)])
    for nc, dtype, s, masked in ((2, np.uint16, 1, False), (1, np.uint8, 2, True), (3, np.uint8, 4, False)):
        image = IR.noise((2,) + shape, nc, dtype, 3)
        geom, sums, isums, planes = GR.measure(image, lab, steps=8, subsample=s, masked=masked)
        assert (np.diff(sums, axis=2) <= 0).all() and (np.diff(isums, axis=1) <= 0).all() and (np.diff(planes.astype(np.int64), axis=1) <= 0).all()
        d = GA.derive(geom, sums, isums)
        assert (np.nansum(d["spectrum"], axis=1) <= 100.0 + 1e-9).all() and (d["spectrum"][~np.isnan(d["spectrum"])] >= 0.0).all()


@pytest.mark.parametrize("s", [2, 4])
def test_block_means_on_sides_that_are_no_multiple_of_the_block(s):
    H, W = 4 * s + 1, 3 * s + s // 2
    image = IR.noise((1, H, W), 2, np.uint16, s)
    lab = np.zeros((1, H, W), np.int32)
    lab[0, 1:H - 1, 1:W - 2] = 1
    ex = np.zeros_like(lab)
    ex[0, 2, :] = 4
    for masked in (False, True):
        P = GR.working_plane(image, lab, ex, s, masked)
        assert P.shape == (1, 2, -(-H // s), -(-W // s)) and P.dtype == np.uint16
        for ch in range(2):
            for R in range(P.shape[2]):
                for Cc in range(P.shape[3]):
                    blk = [(int(image[0, r, c, ch]) if not masked or (lab[0, r, c] and not ex[0, r, c]) else 0)
                           for r in range(R * s, min(H, R * s + s)) for c in range(Cc * s, min(W, Cc * s + s))]
                    f = Fraction(sum(blk), len(blk))
                    assert P[0, ch, R, Cc] == int(f + Fraction(1, 2))      # the rounded mean, halves up
        geom, sums, isums, planes = GR.measure(image, lab, ex, steps=2, subsample=s, masked=masked)
        assert np.array_equal(planes[:, 0], P) and np.array_equal(isums[:, 0], P.astype(np.int64).sum(axis=(2, 3)))
        rr, cc = np.nonzero((lab[0] > 0) & (ex[0] == 0))
        assert np.array_equal(sums[0, 0, 0], P[0][:, rr // s, cc // s].astype(np.int64).sum(axis=1))    # read back by the nearest block


# ---- derive ------------------------------------------------------------------------------------------------------------------------------
def test_derive_is_correctly_rounded_against_fractions():
    rng = np.random.default_rng(5)
    B, M, K, nc = 2, 5, 6, 3
    geom = np.zeros((B, M, 3), np.int64)
    geom[..., 0] = rng.integers(0, 3, (B, M)) * rng.integers(1, 10 ** 6, (B, M))        # some rows absent
    drops = rng.integers(0, 10 ** 12, (B, M, K + 1, nc))
    sums = np.cumsum(drops[:, :, ::-1], axis=2)[:, :, ::-1].copy()                       # non-increasing, up to 7e12: past float32, not a power of two
    sums[0, 0] = 0                                                                       # S_0 = 0
    geom[0, 0, 0] = 7
    isums = np.cumsum(rng.integers(0, 10 ** 13, (B, K + 1, nc))[:, ::-1], axis=1)[:, ::-1].copy()
    isums[1, :, 2] = 0
    d = GA.derive(geom, sums, isums)
    want = GR.derive(geom, sums, isums)
    assert set(d) == set(want)
    for k, v in want.items():
        assert d[k].dtype == v.dtype and d[k].shape == v.shape and np.array_equal(d[k], v, equal_nan=v.dtype.kind == "f"), k
    n = len(d["label"])
    assert n == int((geom[..., 0] > 0).sum()) and np.isnan(d["image_spectrum"][1, :, 2]).all()
    for i in range(n):
        b, m = int(d["image"][i]), int(d["label"][i]) - 1
        for ch in range(nc):
            s0 = int(sums[b, m, 0, ch])
            if s0 == 0:
                assert np.isnan(d["spectrum"][i, :, ch]).all() and np.isnan(d["start_mean"][i, ch])
                continue
            assert d["start_mean"][i, ch] == float(Fraction(s0, int(geom[b, m, 0])))
            for k in range(1, K + 1):
                assert d["spectrum"][i, k - 1, ch] == float(Fraction(100 * (int(sums[b, m, k - 1, ch]) - int(sums[b, m, k, ch])), s0))
    t = GA.granularity_table(geom, sums, isums)
    assert len(t) == n and all(np.array_equal(getattr(t, k), v, equal_nan=v.dtype.kind == "f") for k, v in want.items())


def test_derive_gives_nan_where_the_start_sum_is_zero_and_empty_tables_without_objects():
    lab = np.zeros((2, 6, 7), np.int32)
    lab[0, 1:3, 1:3] = 2
    image = np.zeros((2, 6, 7, 2), np.uint8)
    image[0, :, :, 1] = 9
    t = GA.granularity_table(*GR.measure(image, lab, steps=3)[:3])
    assert len(t) == 1 and t.label.tolist() == [2] and t.area.tolist() == [4]
    assert np.isnan(t.spectrum[0, :, 0]).all() and np.isnan(t.start_mean[0, 0]) and t.start_mean[0, 1] == 9.0 and (t.spectrum[0, :, 1] == 0.0).all()
    assert np.isnan(t.image_spectrum[1]).all() and np.isnan(t.image_spectrum[0, :, 0]).all() and (t.image_spectrum[0, :, 1] == 0.0).all()
    t = GA.granularity_table(*GR.measure(image, np.zeros_like(lab), steps=3)[:3])
    assert len(t) == 0 and t.spectrum.shape == (0, 3, 2) and t.start_mean.shape == (0, 2) and t.image_spectrum.shape == (2, 3, 2)
    assert t.sums.shape == (0, 4, 2) and t.geom.shape == (0, 3) and t.image.dtype == np.int32
    with pytest.raises(TypeError):
        GA.derive(np.zeros((1, 1, 3), np.int32), np.zeros((1, 1, 2, 1), np.int64), np.zeros((1, 2, 1), np.int64))
    with pytest.raises(ValueError):
        GA.derive(np.zeros((1, 1, 3), np.int64), np.zeros((1, 1, 2, 1), np.int64), np.zeros((1, 3, 1), np.int64))


# ---- the package's argument checks ------------------------------------------------------------------------------------------------------
def test_measurer_refusals_before_a_handle_exists():
    """GranularityMeasurer refuses what IntensityMeasurer refuses, with the same exceptions, before it makes a handle."""
    import torch

    import cellscreen
    assert cellscreen.GranularityMeasurer is GA.GranularityMeasurer and cellscreen.GranularityTable is GA.GranularityTable
    assert cellscreen.granularity_table is GA.granularity_table and cellscreen.granularity_params is GA.granularity_params
    assert GA.GranularityMeasurer.MAX_STEPS == GA.MAX_STEPS == GR.MAX_STEPS == 64 and GA.SUBSAMPLES == GR.SUBSAMPLES == (1, 2, 4, 8)
    m = GA.GranularityMeasurer(0)
    lab = np.zeros((2, 8, 12), np.int32)
    img = np.zeros((2, 8, 12, 3), np.uint8)
    for image, labels, kw, exc in (
            (img.astype(np.float32), lab, {}, TypeError), (img.astype(np.int16), lab, {}, TypeError), (img, lab.astype(np.int64), {}, TypeError),
            (list(img), lab, {}, TypeError), (img, list(lab), {}, TypeError), (img, torch.zeros((2, 8, 12), dtype=torch.int32), {}, TypeError),
            (img[0], lab, {}, ValueError), (img, lab[0], {}, ValueError), (img[:, :4], lab, {}, ValueError), (img, lab[:, :, ::2], {}, ValueError),
            (img, lab, dict(exclude=lab[:1]), ValueError), (img, lab, dict(exclude=lab.astype(np.uint8)), TypeError),
            (np.zeros((1, 2, 4097, 2), np.uint8), np.zeros((1, 2, 4097), np.int32), {}, ValueError),
            (np.zeros((0, 4, 4, 2), np.uint8), np.zeros((0, 4, 4), np.int32), {}, ValueError), (np.zeros((2, 8, 12, 5), np.uint8), lab, {}, ValueError),
            (img, lab, dict(max_label=0), ValueError), (img, lab, dict(max_label=2.0), TypeError), (img, lab, dict(max_label=True), TypeError),
            (img, lab, dict(max_label=(1 << 20) + 1), ValueError), (img, lab, dict(max_label=1 << 20), ValueError),
            (img, lab, dict(steps=0), ValueError), (img, lab, dict(steps=65), ValueError), (img, lab, dict(steps=-1), ValueError),
            (img, lab, dict(steps=4.0), TypeError), (img, lab, dict(steps=True), TypeError), (img, lab, dict(steps=None), TypeError),
            (img, lab, dict(subsample=3), ValueError), (img, lab, dict(subsample=0), ValueError), (img, lab, dict(subsample=16), ValueError),
            (img, lab, dict(subsample=2.0), TypeError), (img, lab, dict(subsample=True), TypeError), (img, lab, dict(masked=1), TypeError),
            (img, lab, dict(masked=None), TypeError)):
        for call in (m.measure_batch, m.measure_dense):
            with pytest.raises(exc):
                call(image, labels, **kw)
    with pytest.raises(TypeError):
        m.measure_dense(img, lab, want_planes=1)
    with pytest.raises(ValueError, match="split the batch"):             # 2^20 x 65 x 4 x 8 bytes is above 1 GiB
        m.measure_dense(np.zeros((1, 1, 1, 4), np.uint8), np.zeros((1, 1, 1), np.int32), max_label=1 << 20, steps=64)
    with pytest.raises(ValueError, match="split the batch"):             # 9 x 17 x 4 x 2048 x 2048 x 2 bytes
        m.measure_dense(np.zeros((9, 2048, 2048, 4), np.uint8), np.zeros((9, 2048, 2048), np.int32), max_label=1, steps=16, want_planes=True)
    assert m._pre is None
    p = GA.granularity_params()
    assert (p.steps, p.subsample, p.masked, p.reserved) == (16, 1, 0, 0) and C.sizeof(p) == 16
    p = GA.granularity_params(np.int64(64), np.int32(8), np.bool_(True))
    assert (p.steps, p.subsample, p.masked) == (64, 8, 1)
    with pytest.raises(ValueError):
        GA.GranularityMeasurer(1, extractor=type("E", (), {"device_id": 0})())
    m.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
SYMBOLS = {"cs_label_granularity": 17, "cs_label_granularity_last_timing": 4, "cs_label_granularity_last_rounds": 3}


def test_symbols_are_exported():
    lib = L.load_library()
    raw = C.CDLL(L.LIB_PATH)
    for name, n_args in SYMBOLS.items():
        assert hasattr(raw, name) and hasattr(lib, name) and name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == n_args, name
    assert [f[0] for f in L.CSGranularityParams._fields_] == ["steps", "subsample", "masked", "reserved"] and C.sizeof(L.CSGranularityParams) == 16


def test_the_prototypes_are_in_the_header():
    with open(os.path.join(ROOT, "include", "cellscreen.h")) as f:
        text = " ".join(f.read().split())
    assert ("int cs_label_granularity(cs_preproc *p, const void *image, int pixel_type, int32_t channels, const int32_t *labels, "
            "const int32_t *exclude /* or NULL */, int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, "
            "const cs_granularity_params *params, int64_t *geom, int64_t *sums, int64_t *image_sums, uint16_t *planes /* or NULL */, "
            "int out_kind);") in text
    assert "int cs_label_granularity_last_timing(const cs_preproc *p, double *prepare_ms, double *steps_ms, double *sums_ms);" in text
    assert "int cs_label_granularity_last_rounds(const cs_preproc *p, int32_t *rounds, int32_t *reads);" in text
    assert f"#define CS_GRANULARITY_MAX_STEPS {GA.MAX_STEPS} " in text and " * cs_label_granularity " in text
    assert text.index("int cs_label_radial_last_timing(") < text.index("int cs_label_granularity(")      # after the radial block
    assert "P[R][C] = (2 * sum v + n) / (2 * n)" in text and "R <- min(max over the cross of R, P)" in text   # the rule is stated there
    proto = text[text.index("int cs_label_granularity(") + len("int cs_label_granularity("):]
    proto = proto[:proto.index(");")]
    kinds = []
    for arg in proto.split(","):
        arg = arg.replace("/* or NULL */", "").strip()
        kinds.append("ptr" if "*" in arg else "i32" if arg.startswith("int32_t") else "int")
    want = {"ptr": (L._P, C.POINTER(L.CSGranularityParams)), "i32": (C.c_int32,), "int": (L._I,)}
    sig = L.SIGNATURES["cs_label_granularity"][1]
    assert len(sig) == len(kinds) == 17 and all(s in want[k] for s, k in zip(sig, kinds)) and sig[11] is C.POINTER(L.CSGranularityParams)


def _call(lib, image=True, labels=True, params=True, geom=True, sums=True, image_sums=True, planes=False, ptype=1, channels=2, B=1, H=8, W=8,
          in_kind=0, out_kind=0, max_label=4, steps=4, subsample=1, masked=0, reserved=0):
    a = np.zeros(64, np.int64)                                           # never read: every call here ends before the device
    p = a.ctypes.data
    prm = L.CSGranularityParams()
    prm.steps, prm.subsample, prm.masked, prm.reserved = steps, subsample, masked, reserved
    rc = lib.cs_label_granularity(None, p if image else None, ptype, channels, p if labels else None, None, B, H, W, in_kind, max_label,
                                  C.byref(prm) if params else None, p if geom else None, p if sums else None, p if image_sums else None,
                                  p if planes else None, out_kind)
    return rc, lib.cs_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_the_handle():
    lib = L.load_library()
    for over, status in ((dict(image=False), -1), (dict(labels=False), -1), (dict(params=False), -1), (dict(geom=False), -1), (dict(sums=False), -1),
                         (dict(image_sums=False), -1), (dict(ptype=2), -1), (dict(in_kind=2), -1), (dict(out_kind=-1), -1),
                         (dict(channels=0), -1), (dict(B=0), -1), (dict(H=0), -1), (dict(W=-1), -1), (dict(max_label=0), -1),
                         (dict(channels=5), -6), (dict(steps=0), -1), (dict(steps=-3), -1), (dict(subsample=3), -1), (dict(subsample=0), -1),
                         (dict(subsample=16), -1), (dict(masked=2), -1), (dict(masked=-1), -1), (dict(reserved=1), -1), (dict(steps=65), -6),
                         (dict(H=4097), -6), (dict(W=4097), -6), (dict(B=65536), -6), (dict(max_label=(1 << 20) + 1), -6),
                         (dict(B=3, max_label=1 << 20), -6), (dict(channels=4, steps=64, max_label=1 << 20), -6),
                         (dict(planes=True, B=9, H=2048, W=2048, channels=4, steps=16), -6)):
        rc, text = _call(lib, **over)
        assert rc == status and text, over
    # the order of the rules: the earlier one answers
    for over, status in ((dict(channels=0, H=4097), -1), (dict(channels=5, max_label=0), -1), (dict(channels=5, steps=0), -6), (dict(steps=0, H=4097), -1),
                         (dict(steps=65, reserved=1), -1), (dict(steps=65, subsample=3), -1), (dict(steps=65, H=4097), -6),
                         (dict(H=4097, channels=4, steps=64, max_label=1 << 20), -6)):
        assert _call(lib, **over)[0] == status, over
    assert "at most 4 are measured per call" in _call(lib, channels=5)[1] and "at most 64 steps" in _call(lib, steps=65)[1]
    assert "split the batch" in _call(lib, channels=4, steps=64, max_label=1 << 20)[1] and "sums table" in _call(lib, channels=4, steps=64, max_label=1 << 20)[1]
    assert "split the batch" in _call(lib, planes=True, B=9, H=2048, W=2048, channels=4, steps=16)[1]
    assert "sides above 4096" in _call(lib, H=4097, channels=4, steps=64, max_label=1 << 20)[1]            # the caps in the header's order
    assert "reserved must be 0" in _call(lib, reserved=1)[1] and "must be 1, 2, 4 or 8" in _call(lib, subsample=3)[1]
    assert _call(lib)[0] in (-4, -1)                                     # nothing wrong but the handle: no device, or a NULL handle
    assert lib.cs_label_granularity_last_timing(None, None, None, None) == -1 and lib.cs_label_granularity_last_rounds(None, None, None) == -1
