"""CPU tests of the per-object intensities (cs_label_intensity, cellscreen/intensity.py): the restatement of
tests/intensity_reference.py against its slow form, against scipy.ndimage's labelled statistics and against their record in
tests/golden/golden_intensity.npz, the table the package derives from the integers, and the wrapper's and the C ABI's refusals
before any device work.

The float comparisons use rtol 1e-12: on random disks with uniform uint16 noise and on a bright low-contrast plane
(60000 + U[0,600)) the worst relative difference between SciPy's float64 sums and the exact integers was 3.7e-16, measured
against SciPy alone before there was code to test; 1e-12 leaves room for other summation orders."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
from scipy import ndimage as ndi

import intensity_reference as IR
from cellscreen import _lib as L
from cellscreen import intensity as IN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_intensity.npz")
RTOL = 1e-12


def small_cases():
    """(name, image [B,H,W,C], labels, exclude or None)"""
    out = []
    for k, (shape, nc, dt) in enumerate((((17, 23), 1, np.uint8), ((20, 31), 3, np.uint16), ((9, 40), 4, np.uint8), ((1, 1), 2, np.uint16))):
        for name, lab in IR.contents(shape, 10 + k):
            labels = np.stack([lab, np.roll(lab, 1, axis=1)])
            ex = np.stack([(lab > 0) & (np.arange(shape[1])[None, :] % 3 == 0), np.zeros(shape, bool)]).astype(np.int32) * 9
            out.append((f"{shape} {name} C{nc} {np.dtype(dt).name}", IR.noise((2,) + shape, nc, dt, 20 + k), labels, ex if k % 2 else None))
    return out


def test_restatement_equals_the_slow_form():
    for name, image, labels, ex in small_cases():
        g, s = IR.measure(image, labels, ex)
        g2, s2 = IR.measure_slow(image, labels, ex)
        assert g.dtype == s.dtype == np.int64 and g.shape == g2.shape and s.shape == s2.shape, name
        assert np.array_equal(g, g2) and np.array_equal(s, s2), name
    img = IR.noise((1, 4, 5), 1, np.uint8, 1)
    lab = np.zeros((1, 4, 5), np.int32)
    lab[0, 1, 2] = 2
    g, s = IR.measure(img[..., 0], lab, max_label=3)                     # [B,H,W] is one channel; rows of absent labels are zero
    v = int(img[0, 1, 2, 0])
    assert g.tolist() == [[[0, 0, 0], [1, 1, 2], [0, 0, 0]]] and s[0, 1, 0].tolist() == [v, v * v, v, 2 * v, v, v]
    assert not s[0, 0].any() and not s[0, 2].any()
    g, s = IR.measure(img, lab, exclude=lab)                             # swallowed whole: all zero, the minimum included
    assert not g.any() and not s.any()
    for bad in (-1, 4):
        lab2 = lab.copy()
        lab2[0, 0, 0] = bad
        with pytest.raises(ValueError):
            IR.measure(img, lab2, exclude=np.ones_like(lab), max_label=3)   # refused whatever exclude holds there
        with pytest.raises(ValueError):
            IR.measure_slow(img, lab2, max_label=3)


def scipy_table(image, labels, exclude):
    """scipy.ndimage on float64 copies of one image [H,W,C]: what a caller without the device computes."""
    lab = labels if exclude is None else np.where(exclude != 0, 0, labels)
    index = np.unique(lab[lab > 0])
    ones = np.ones(lab.shape)
    t = dict(index=index, area=np.asarray(ndi.sum(ones, lab, index)), centroid=np.asarray(ndi.center_of_mass(ones, lab, index)).reshape(-1, 2))
    for k in ("sum", "mean", "std", "min", "max", "wc"):
        t[k] = []
    for ch in range(image.shape[2]):
        v = image[:, :, ch].astype(np.float64)
        t["sum"].append(ndi.sum(v, lab, index))
        t["mean"].append(ndi.mean(v, lab, index))
        t["std"].append(ndi.standard_deviation(v, lab, index))
        t["min"].append(ndi.minimum(v, lab, index))
        t["max"].append(ndi.maximum(v, lab, index))
        with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
            warnings.simplefilter("ignore")
            t["wc"].append(np.asarray(ndi.center_of_mass(v, lab, index)).reshape(-1, 2))
    for k in ("sum", "mean", "std", "min", "max", "wc"):
        t[k] = np.stack([np.asarray(x, np.float64) for x in t[k]], axis=1)
    return t


def assert_table_matches_scipy(d, t, name):
    """d: a derived table of ONE image (IR.derive's dict or an ObjectTable's fields); t: the SciPy values."""
    assert np.array_equal(d["label"], t["index"]), name
    assert np.array_equal(d["area"], t["area"]) and np.array_equal(d["integrated"], t["sum"]), name      # integer-valued: exactly
    assert np.array_equal(d["min"], t["min"]) and np.array_equal(d["max"], t["max"]), name
    np.testing.assert_allclose(d["centroid"], t["centroid"], rtol=RTOL, atol=0, err_msg=name)
    np.testing.assert_allclose(d["mean"], t["mean"], rtol=RTOL, atol=0, err_msg=name)
    pos = t["std"] > 0
    np.testing.assert_allclose(d["std"][pos], t["std"][pos], rtol=RTOL, atol=0, err_msg=name)
    assert (d["std"][~pos] == 0).all(), name
    assert np.array_equal(np.isnan(d["weighted_centroid"]), np.isnan(t["wc"])), name
    np.testing.assert_allclose(d["weighted_centroid"], t["wc"], rtol=RTOL, atol=0, equal_nan=True, err_msg=name)


def test_restatement_equals_scipy():
    lab = IR.disks((70, 300), 40, 1)
    ring = IR.disks((70, 300), 40, 1, radii=(1, 2))
    cases = [("uint16 noise C3", IR.noise(lab.shape, 3, np.uint16, 2), lab, None),
             ("uint16 bright low contrast", IR.noise(lab.shape, 1, np.uint16, 3, base=60000, spread=600), lab, None),
             ("uint8 noise C4, exclude", IR.noise(lab.shape, 4, np.uint8, 4), lab, ring),
             ("uint8 constant", np.full(lab.shape + (1,), 7, np.uint8), lab, None),
             ("uint8 dark", np.zeros(lab.shape + (2,), np.uint8), lab, None)]
    for name, image, labels, ex in cases:
        g, s = IR.measure(image[None], labels[None], None if ex is None else ex[None])
        d = IR.derive(g, s)
        assert (d["image"] == 0).all()
        assert_table_matches_scipy(d, scipy_table(image, labels, ex), name)


def test_the_package_derives_the_same_table_from_the_integers():
    for name, image, labels, ex in small_cases():
        g, s = IR.measure(image, labels, ex)
        d, t = IR.derive(g, s), IN.object_table(g, s)
        assert isinstance(t, IN.ObjectTable) and len(t) == len(d["label"])
        for k, v in d.items():
            got = getattr(t, k)
            assert got.dtype == v.dtype and got.shape == v.shape and np.array_equal(got, v, equal_nan=v.dtype.kind == "f"), (name, k)
        order = np.lexsort((t.label, t.image))
        assert np.array_equal(order, np.arange(len(t)))                  # (image, label) order
    big = np.zeros((1, 1, 3), np.int64), np.zeros((1, 1, 1, 6), np.int64)
    n, v = 1 << 24, 65535                                                # the largest sums: n * sum v^2 is near 2^80
    big[0][0, 0] = n, 4095 * n // 2, 4095 * n // 2
    big[1][0, 0, 0] = n * v - 1, n * v * v - 2 * v + 1, 0, 0, v - 1, v   # one pixel of v - 1 among n - 1 of v
    t = IN.object_table(*big)
    want = np.sqrt(float(n - 1)) / n                                     # n (sum v^2) - (sum v)^2 = n - 1, exactly
    assert t.std[0, 0] == want and t.mean[0, 0] == (n * v - 1) / n and t.centroid.tolist() == [[2047.5, 2047.5]]
    with pytest.raises(TypeError):
        IN.object_table(big[0].astype(np.int32), big[1])
    with pytest.raises(ValueError):
        IN.object_table(big[0], big[1][0])


def test_golden_file_matches():
    g = np.load(GOLDEN)
    assert str(g["scipy_version"]) == "1.15.3" and int(g["n_cases"]) == 4 and os.path.getsize(GOLDEN) < 100_000
    dtypes, nans = set(), 0
    for i in range(int(g["n_cases"])):
        image, labels, ex = g[f"image_{i}"], g[f"labels_{i}"], g[f"exclude_{i}"]
        dtypes.add((image.dtype.name, image.shape[2]))
        t = {k: g[f"{k}_{i}"] for k in ("index", "area", "centroid", "sum", "mean", "std", "min", "max", "wc")}
        d = IR.derive(*IR.measure(image[None], labels[None], ex[None]))
        assert_table_matches_scipy(d, t, str(g[f"name_{i}"]))
        nans += int(np.isnan(t["wc"]).sum())
        assert len(t["index"]) >= 5
    assert dtypes == {("uint16", 3), ("uint16", 1), ("uint8", 4), ("uint8", 2)} and nans > 0


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------
def test_measurer_refusals_before_a_handle_exists():
    import torch

    import cellscreen
    assert cellscreen.IntensityMeasurer is IN.IntensityMeasurer and cellscreen.ObjectTable is IN.ObjectTable
    m = IN.IntensityMeasurer(0)
    img = np.zeros((2, 8, 12, 3), np.uint16)
    lab = np.zeros((2, 8, 12), np.int32)
    cpu_t = torch.zeros((2, 8, 12), dtype=torch.int32)
    for image, labels, kw, exc in (
            (img.astype(np.float32), lab, {}, TypeError), (img.astype(np.int16), lab, {}, TypeError), (img, lab.astype(np.int64), {}, TypeError),
            (img, lab.astype(np.uint16), {}, TypeError), (img, lab, dict(exclude=lab.astype(bool)), TypeError),
            (list(img), lab, {}, TypeError), (img, list(lab), {}, TypeError), (img, lab, dict(exclude=[0]), TypeError),
            (img[0], lab, {}, ValueError), (img[..., None], lab, {}, ValueError), (img, lab[0], {}, ValueError),
            (img, lab[:, :, :11], {}, ValueError), (img, lab, dict(exclude=lab[:1]), ValueError), (img[:0], lab[:0], {}, ValueError),
            (img[:, :, :, :0], lab, {}, ValueError), (img[:, :, ::2], lab[:, :, ::2], {}, ValueError),
            (img[:, :, :, :2], lab, {}, ValueError),                                                         # a channel slice: not contiguous
            (img, np.zeros((2, 12, 8), np.int32).transpose(0, 2, 1), {}, ValueError),
            (img, lab, dict(exclude=np.zeros((2, 8, 24), np.int32)[:, :, ::2]), ValueError),
            (np.zeros((2, 8, 12, 5), np.uint8), lab, {}, ValueError),                                         # channels > 4
            (np.zeros((1, 2, 4097), np.uint8), np.zeros((1, 2, 4097), np.int32), {}, ValueError),
            (np.zeros((1, 4097, 2), np.uint8), np.zeros((1, 4097, 2), np.int32), {}, ValueError),
            (img, cpu_t, {}, TypeError), (img, lab, dict(exclude=cpu_t), TypeError),                             # mixed numpy / tensor
            (torch.zeros((2, 8, 12), dtype=torch.uint8), cpu_t, {}, ValueError),                              # CPU tensors
            (torch.zeros((2, 8, 12), dtype=torch.float32), cpu_t, {}, TypeError),
            (img, lab, dict(max_label=0), ValueError), (img, lab, dict(max_label=-3), ValueError), (img, lab, dict(max_label=2.0), TypeError),
            (img, lab, dict(max_label=True), TypeError), (img, lab, dict(max_label=(1 << 20) + 1), ValueError),
            (img, lab, dict(max_label=1 << 20), ValueError),                                                  # 2 x 2^20 x 3 cells
            (img[:, :, :, :1].copy(), lab, dict(max_label=(1 << 21) + 1), ValueError)):
        with pytest.raises(exc):
            m.measure_batch(image, labels, **kw)
    lab2 = lab.copy()
    lab2[0, 0, 0] = (1 << 20) + 1                                        # max_label=None: the labels' maximum meets the same limits
    with pytest.raises(ValueError):
        m.measure_batch(img, lab2)
    assert m._pre is None
    with pytest.raises(ValueError):
        IN.IntensityMeasurer(1, extractor=type("E", (), {"device_id": 0})())
    m.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2 and lib.cs_profile_kernel_count() == 13
    raw = C.CDLL(L.LIB_PATH)
    for name in ("cs_label_intensity", "cs_label_intensity_last_timing"):
        assert hasattr(raw, name) and name in L.SIGNATURES


def test_the_prototypes_are_in_the_header():
    with open(os.path.join(ROOT, "include", "cellscreen.h")) as f:
        text = " ".join(f.read().split())
    assert ("int cs_label_intensity(cs_preproc *p, const void *image, int pixel_type, int32_t channels, const int32_t *labels, "
            "const int32_t *exclude /* or NULL */, int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, "
            "int64_t *geom, int64_t *stats, int out_kind);") in text
    assert "int cs_label_intensity_last_timing(const cs_preproc *p, double *clear_ms, double *pass_ms);" in text
    assert "#define CS_ABI_VERSION 2 " in text


def _call(lib, image=True, labels=True, geom=True, stats=True, exclude=False, ptype=1, Cn=1, B=1, H=8, W=8, in_kind=0, out_kind=0, max_label=4):
    a = np.zeros(64, np.int64)                                           # never read: every call here ends before the device
    p = a.ctypes.data
    rc = lib.cs_label_intensity(None, p if image else None, ptype, Cn, p if labels else None, p if exclude else None, B, H, W, in_kind,
                                max_label, p if geom else None, p if stats else None, out_kind)
    return rc, lib.cs_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_the_handle():
    lib = L.load_library()
    for over, status in ((dict(image=False), -1), (dict(labels=False), -1), (dict(geom=False), -1), (dict(stats=False), -1),
                         (dict(Cn=0), -1), (dict(Cn=-1), -1), (dict(Cn=5), -6), (dict(in_kind=2), -1), (dict(out_kind=-1), -1),
                         (dict(ptype=2), -1), (dict(ptype=-1), -1), (dict(B=0), -1), (dict(H=0), -1), (dict(W=-1), -1),
                         (dict(max_label=0), -1), (dict(max_label=-5), -1), (dict(max_label=(1 << 20) + 1), -6),
                         (dict(B=5, max_label=1 << 20), -6), (dict(B=2, Cn=3, max_label=1 << 20), -6), (dict(Cn=4, max_label=(1 << 20) + 1), -6),
                         (dict(B=4, Cn=1, max_label=(1 << 20) + 1), -6), (dict(B=1 << 12, Cn=4, max_label=257), -6),
                         (dict(H=4097), -6), (dict(W=4097), -6), (dict(B=65536), -6)):
        rc, text = _call(lib, **over)
        assert rc == status and text, over
    assert "channels 5: at most 4" in _call(lib, Cn=5)[1]
    assert lib.cs_label_intensity_last_timing(None, None, None) == -1


def test_a_null_handle_reports_no_device_for_valid_arguments():
    lib = L.load_library()
    no_dev = lib.cs_device_count() <= 0
    for over in (dict(), dict(exclude=True), dict(ptype=0, Cn=3), dict(Cn=4, max_label=1 << 20), dict(B=4, max_label=1 << 20),
                 dict(B=1 << 12, Cn=4, max_label=256), dict(in_kind=1, out_kind=1), dict(H=4096, W=4096), dict(B=65535, H=1, W=1, max_label=64)):
        assert _call(lib, **over)[0] == (-4 if no_dev else -1), over      # no handle: no device here, else a NULL handle
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            IN.IntensityMeasurer(0).measure_batch(np.zeros((1, 8, 8), np.uint8), np.zeros((1, 8, 8), np.int32))
        assert ei.value.status == -4
