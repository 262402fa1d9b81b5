"""CPU tests of the per-object order statistics (cs_label_quantiles, cellscreen/quantile.py): the restatement of
tests/quantile_reference.py against its slow form, against numpy.quantile / numpy.median / scipy.stats.median_abs_deviation
live and in their record tests/golden/golden_quantiles.npz, the table the package derives from the integers, the conversion of
floats to fractions, and the wrapper's and the C ABI's refusals before any device work.

Against numpy: s[lo] and s[hi] equal method="lower" and "higher" wherever numpy's float index (n - 1) * q falls on the same
side of an integer as the exact one -- always for the dyadic quantiles (den 1, 2, 4), whose index is exact -- and the
interpolated value equals method="linear" bit for bit for the dyadic ones, as does the MAD.  For the other quantiles numpy rounds
its index in float64: it is off by at most n * 2^-52, times the largest step between neighbours (65535), with a factor 2 for the
interpolation, so the bound is 65535 * n * 2^-51 per object; "lower" and "higher" are then compared where the exact index is
not an integer (where it is, numpy's rounded index may fall on either side)."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest
from scipy import stats

import quantile_reference as QR
from cellscreen import _lib as L
from cellscreen import quantile as QN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_quantiles.npz")
DYADIC = (1, 2, 4)


def small_cases():
    """(name, image [B,H,W,C], labels, exclude or None)"""
    out = []
    for k, (shape, nc, dt) in enumerate((((17, 23), 1, np.uint8), ((20, 31), 3, np.uint16), ((9, 40), 4, np.uint8), ((1, 1), 2, np.uint16))):
        for name, lab in QR.contents(shape, 10 + k):
            labels = np.stack([lab, np.roll(lab, 1, axis=1)])
            ex = np.stack([(lab > 0) & (np.arange(shape[1])[None, :] % 3 == 0), np.zeros(shape, bool)]).astype(np.int32) * 9
            out.append((f"{shape} {name} C{nc} {np.dtype(dt).name}", QR.noise((2,) + shape, nc, dt, 20 + k), labels, ex if k % 2 else None))
    return out


def tiny():
    """one image with objects of 1, 2 and 3 pixels (labels 1, 2, 3) and an absent label 4"""
    lab = np.zeros((1, 3, 4), np.int32)
    lab[0, 0, 0] = 1
    lab[0, 1, 0:2] = 2
    lab[0, 2, 0:3] = 3
    img = np.zeros((1, 3, 4), np.uint16)
    img[0, 0, 0] = 500
    img[0, 1, 0:2] = 70, 10
    img[0, 2, 0:3] = 65535, 0, 256
    return img, lab


def same(a, b, name=""):
    for x, y in zip(a, b):
        assert (x is None) == (y is None), name
        if x is not None:
            assert x.dtype == y.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y), name


def test_restatement_equals_the_slow_form():
    for name, image, labels, ex in small_cases():
        for q, mad in ((QR.QUANTILES, True), (QR.TWELVE[:8], False), (((1, 2),), True)):
            same(QR.measure(image, labels, q, mad, ex), QR.measure_slow(image, labels, q, mad, ex), name)
    img, lab = tiny()
    q = ((0, 1), (1, 1), (1, 2), (1, 2), (3, 4), (1, 4), (1, 3), (65535, 65536))       # q = 0 and 1, a duplicate, unsorted
    c, o, m = QR.measure(img, lab, q, True, max_label=4)
    same((c, o, m), QR.measure_slow(img, lab, q, True, max_label=4))
    assert c.tolist() == [[1, 2, 3, 0]]
    assert (o[0, 0, 0] == 500).all() and m[0, 0, 0].tolist() == [500, 500, 0, 0]         # n = 1: every rank is 0
    assert o[0, 1, 0].tolist() == [[10, 10], [70, 70], [10, 70], [10, 70], [10, 70], [10, 70], [10, 70], [10, 70]]
    assert m[0, 1, 0].tolist() == [10, 70, 60, 60]                                       # median 40, |2 v - 80| = 60, 60: MAD 30
    assert o[0, 2, 0].tolist() == [[0, 0], [65535, 65535], [256, 256], [256, 256], [256, 65535], [0, 256], [0, 256], [256, 65535]]
    assert m[0, 2, 0].tolist() == [256, 256, 512, 512]                                   # d = 130558, 512, 0: the 17th bit among them
    assert not c[0, 3] and not o[0, 3].any() and not m[0, 3].any()
    same(QR.measure(img, lab, q, True, exclude=lab, max_label=4), (np.zeros_like(c), np.zeros_like(o), np.zeros_like(m)))
    assert QR.measure(img, lab, q, False)[2] is None
    for bad in (-1, 5):
        lab2 = lab.copy()
        lab2[0, 0, 3] = bad
        with pytest.raises(ValueError):
            QR.measure(img, lab2, q, exclude=np.ones_like(lab), max_label=4)              # refused whatever exclude holds there
        with pytest.raises(ValueError):
            QR.measure_slow(img, lab2, q, max_label=4)
    for bad_q in (((2, 1),), ((-1, 4),), ((1, 0),), ((1, 65537),), ()):
        with pytest.raises(ValueError):
            QR.measure(img, lab, bad_q)


def numpy_check(image, labels, exclude, t, name):
    """One image [H,W,C] against numpy / SciPy values t (make_golden_quantiles.numpy_table's fields) under the module's tolerances."""
    quantiles = QR.TWELVE
    count, order, mad = QR.measure(image[None], labels[None], quantiles, True, None if exclude is None else exclude[None])
    d = QR.derive(count, order, mad, quantiles)
    assert np.array_equal(d["label"], t["index"]) and np.array_equal(d["count"], t["count"]), name
    assert np.array_equal(d["median"], t["median"]) and np.array_equal(d["mad"], t["mad"]), name
    n = d["count"].astype(np.int64)
    for k, (num, den) in enumerate(quantiles):
        if den in DYADIC:
            for mine, theirs in (("value", "linear"), ("lower", "lower"), ("upper", "higher")):
                assert np.array_equal(d[mine][:, :, k], t[theirs][:, :, k]), (name, num, den, mine)
        else:
            bound = 65535.0 * n * 2.0 ** -51
            assert (np.abs(d["value"][:, :, k] - t["linear"][:, :, k]) <= bound[:, None]).all(), (name, num, den)
            inexact = (num * (n - 1)) % den != 0
            for mine, theirs in (("lower", "lower"), ("upper", "higher")):
                assert np.array_equal(d[mine][inexact, :, k], t[theirs][inexact, :, k]), (name, num, den, mine)
    assert np.array_equal(d["value"][:, :, 2], d["median"])                              # q = 1/2 is the median


def test_restatement_equals_numpy_and_scipy():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from make_golden_quantiles import numpy_table
    finally:
        sys.path.pop(0)
    lab = QR.disks((70, 300), 40, 1)
    ring = QR.disks((70, 300), 40, 1, radii=(1, 2))
    cases = [("uint16 noise C3", QR.noise(lab.shape, 3, np.uint16, 2), lab, None),
             ("uint16 bright low contrast", QR.noise(lab.shape, 1, np.uint16, 3, base=60000, spread=600), lab, None),
             ("uint8 noise C4, exclude", QR.noise(lab.shape, 4, np.uint8, 4), lab, ring),
             ("uint8 constant", np.full(lab.shape + (1,), 7, np.uint8), lab, None),
             ("uint16 one object over the plane", QR.noise((50, 60), 1, np.uint16, 5), np.ones((50, 60), np.int32), None)]
    for name, image, labels, ex in cases:
        numpy_check(image, labels, ex, numpy_table(image, labels, np.zeros_like(labels) if ex is None else ex), name)
    rng = np.random.default_rng(7)                                       # the MAD of single objects, scipy and its definition
    for n in (1, 2, 3, 4, 5, 100, 101):
        v = rng.integers(0, 65536, n).astype(np.uint16)
        _, _, m = QR.measure(v.reshape(1, 1, n), np.ones((1, 1, n), np.int32), ((1, 2),), True)
        got = (int(m[0, 0, 0, 2]) + int(m[0, 0, 0, 3])) / 4
        f = v.astype(np.float64)
        assert got == stats.median_abs_deviation(f) == np.median(np.abs(f - np.median(f))), n


def test_golden_file_matches():
    g = np.load(GOLDEN)
    assert str(g["numpy_version"]) == "2.2.6" and str(g["scipy_version"]) == "1.15.3" and int(g["n_cases"]) == 4
    assert os.path.getsize(GOLDEN) < 100_000
    assert [(int(a), int(b)) for a, b in zip(g["q_num"], g["q_den"])] == list(QR.TWELVE)
    dtypes = set()
    for i in range(int(g["n_cases"])):
        image, labels, ex = g[f"image_{i}"], g[f"labels_{i}"], g[f"exclude_{i}"]
        dtypes.add((image.dtype.name, image.shape[2]))
        t = {k: g[f"{k}_{i}"] for k in ("index", "count", "linear", "lower", "higher", "median", "mad")}
        numpy_check(image, labels, ex, t, str(g[f"name_{i}"]))
        assert len(t["index"]) >= 5
    assert dtypes == {("uint16", 3), ("uint16", 1), ("uint8", 4), ("uint8", 2)}


# ---- the package's host half ----------------------------------------------------------------------------------------------------
def test_the_package_derives_the_same_table_from_the_integers():
    for name, image, labels, ex in small_cases():
        for q, mad in ((QR.QUANTILES, True), (((3, 4), (0, 1), (1, 1), (3, 4), (1, 3)), False)):
            c, o, m = QR.measure(image, labels, q, mad, ex)
            d = QR.derive(c, o, m, q)
            t = QN.quantile_table(c, o, m, q)
            assert isinstance(t, QN.QuantileTable) and len(t) == len(d["label"]) and t.fractions == tuple(Fraction(a, b) for a, b in q)
            for k, v in d.items():
                got = getattr(t, k)
                assert got.dtype == v.dtype and got.shape == v.shape and np.array_equal(got, v), (name, k)
            if not mad:
                assert t.median is None and t.mad is None and t.mad_raw is None
            assert np.array_equal(np.lexsort((t.label, t.image)), np.arange(len(t)))     # (image, label) order
            assert np.array_equal(t.value, QR.values(t.count[:, None], t.lower, t.upper, q))
    img, lab = tiny()
    q = ((0, 1), (1, 1), (1, 2), (1, 2), (3, 4), (1, 4), (1, 3), (65535, 65536))
    t = QN.quantile_table(*QR.measure(img, lab, q, True, max_label=4), q)
    assert t.label.tolist() == [1, 2, 3] and t.count.tolist() == [1, 2, 3] and t.image.tolist() == [0, 0, 0]
    assert t.value[0, 0].tolist() == [500.0] * 8
    assert t.value[1, 0].tolist() == [10.0, 70.0, 40.0, 40.0, 55.0, 25.0, 30.0, 10 + 60 * 65535 / 65536]
    assert t.value[2, 0].tolist() == [0.0, 65535.0, 256.0, 256.0, 256 + 65279 / 2, 128.0, 256 * 2 / 3, 256 + 65279 * 65534 / 65536]
    assert t.median[:, 0].tolist() == [500.0, 40.0, 256.0] and t.mad[:, 0].tolist() == [0.0, 30.0, 256.0]
    f = img[0, 2, 0:3].astype(np.float64)
    assert t.mad[2, 0] == stats.median_abs_deviation(f) and t.value[2, 0, 4] == np.quantile(f, 0.75)
    c, o, m = QR.measure(img, lab, q, True, max_label=4)
    with pytest.raises(TypeError):
        QN.quantile_table(c.astype(np.int64), o, m, q)
    with pytest.raises(ValueError):
        QN.quantile_table(c, o[:, :, :, :3], m, q)
    with pytest.raises(ValueError):
        QN.quantile_table(c, o, m[:, :1], q)


def test_floats_become_fractions():
    F = Fraction
    for q, want in ((0.01, F(1, 100)), (0.95, F(19, 20)), (1 / 3, F(1, 3)), (0.25, F(1, 4)), (0.5, F(1, 2)), (0.0, F(0)), (1.0, F(1)),
                    (0, F(0)), (1, F(1)), (np.float32(0.75), F(3, 4)), (np.float64(0.99), F(99, 100)), (F(2, 7), F(2, 7)),
                    ((3, 9), F(1, 3)), ([1, 65536], F(1, 65536)), ((0, 5), F(0)), ((7, 7), F(1)), (1e-9, F(0)), (0.1, F(1, 10))):
        got = QN.as_fraction(q)
        assert got == want and isinstance(got, F) and got.denominator <= 65536, q
    for q, exc in ((float("nan"), ValueError), (-0.1, ValueError), (1.0000001, ValueError), (float("inf"), ValueError), (2, ValueError),
                   (-1, ValueError), (F(3, 2), ValueError), (F(-1, 2), ValueError), (F(1, 65537), ValueError), ((1, 0), ValueError),
                   ((5, 4), ValueError), ((-1, 4), ValueError), ((1, 2, 3), TypeError), ((0.5, 1), TypeError), ("0.5", TypeError),
                   (None, TypeError), (True, TypeError), ((1, 65537), ValueError)):
        with pytest.raises(exc):
            QN.as_fraction(q)
    assert QN.as_fractions((0.75, 0.25, 0.75)) == (F(3, 4), F(1, 4), F(3, 4))            # duplicates and any order are kept
    assert QN.as_fractions(np.array([0.5, 0.01])) == (F(1, 2), F(1, 100)) and len(QN.as_fractions([0.5] * 8)) == 8
    for q, exc in (((), ValueError), ([0.5] * 9, ValueError), (0.5, TypeError), ("0.5", TypeError), (None, TypeError)):
        with pytest.raises(exc):
            QN.as_fractions(q)


def test_measurer_refusals_before_a_handle_exists():
    import torch

    import cellscreen
    assert cellscreen.QuantileMeasurer is QN.QuantileMeasurer and cellscreen.QuantileTable is QN.QuantileTable
    m = QN.QuantileMeasurer(0)
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
            (img, lab, dict(quantiles=()), ValueError), (img, lab, dict(quantiles=[0.5] * 9), ValueError),
            (img, lab, dict(quantiles=(0.5, float("nan"))), ValueError), (img, lab, dict(quantiles=(1.5,)), ValueError),
            (img, lab, dict(quantiles=(-0.25,)), ValueError), (img, lab, dict(quantiles=0.5), TypeError),
            (img, lab, dict(quantiles=("median",)), TypeError), (img, lab, dict(quantiles=((1, 0),)), ValueError),
            (img, lab, dict(quantiles=(Fraction(1, 65537),)), ValueError),
            (img, lab, dict(max_label=0), ValueError), (img, lab, dict(max_label=-3), ValueError), (img, lab, dict(max_label=2.0), TypeError),
            (img, lab, dict(max_label=True), TypeError), (img, lab, dict(max_label=(1 << 20) + 1), ValueError),
            (img, lab, dict(max_label=1 << 18), ValueError),                                                  # 2 x 2^18 x 3 x 3 cells
            (img, lab, dict(max_label=1 << 19, quantiles=(0.5, 0.5)), ValueError),
            (img[:, :, :, :1].copy(), lab, dict(max_label=(1 << 21) + 1, quantiles=(0.5,)), ValueError)):
        for call in (m.measure_batch, m.measure_dense):
            with pytest.raises(exc):
                call(image, labels, **kw)
    lab2 = lab.copy()
    lab2[0, 0, 0] = (1 << 20) + 1                                        # max_label=None: the labels' maximum meets the same limits
    with pytest.raises(ValueError):
        m.measure_batch(img, lab2)
    assert m._pre is None
    with pytest.raises(ValueError):
        QN.QuantileMeasurer(1, extractor=type("E", (), {"device_id": 0})())
    m.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2 and lib.cs_profile_kernel_count() == 13
    raw = C.CDLL(L.LIB_PATH)
    for name in ("cs_label_quantiles", "cs_label_quantiles_last_timing"):
        assert hasattr(raw, name) and name in L.SIGNATURES
    assert len(L.SIGNATURES["cs_label_quantiles"][1]) == 19 and len(L.SIGNATURES["cs_label_quantiles_last_timing"][1]) == 4


def test_the_prototypes_are_in_the_header():
    with open(os.path.join(ROOT, "include", "cellscreen.h")) as f:
        text = " ".join(f.read().split())
    assert ("int cs_label_quantiles(cs_preproc *p, const void *image, int pixel_type, int32_t channels, const int32_t *labels, "
            "const int32_t *exclude /* or NULL */, int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, "
            "const int32_t *q_num, const int32_t *q_den, int32_t n_q, int want_mad, int32_t *count, int32_t *order, "
            "int32_t *mad /* or NULL */, int out_kind);") in text
    assert "int cs_label_quantiles_last_timing(const cs_preproc *p, double *count_ms, double *scatter_ms, double *select_ms);" in text
    assert "#define CS_ABI_VERSION 2 " in text
    assert "t = num * (n - 1)" in text and "lo = t / den, rem = t % den, hi = lo + (rem > 0)" in text      # the rule is stated there


def _call(lib, image=True, labels=True, q_num=True, q_den=True, count=True, order=True, mad=True, exclude=False, ptype=1, Cn=1, B=1, H=8,
          W=8, in_kind=0, out_kind=0, max_label=4, q=((1, 2),), n_q=None, want_mad=0):
    a = np.zeros(64, np.int64)                                           # never read: every call here ends before the device
    p = a.ctypes.data
    num = np.array([x for x, _ in q] + [0], np.int32)
    den = np.array([y for _, y in q] + [1], np.int32)
    rc = lib.cs_label_quantiles(None, p if image else None, ptype, Cn, p if labels else None, p if exclude else None, B, H, W, in_kind,
                                max_label, num.ctypes.data if q_num else None, den.ctypes.data if q_den else None,
                                len(q) if n_q is None else n_q, want_mad, p if count else None, p if order else None, p if mad else None,
                                out_kind)
    return rc, lib.cs_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_the_handle():
    lib = L.load_library()
    nine = ((1, 2),) * 9
    for over, status in ((dict(image=False), -1), (dict(labels=False), -1), (dict(q_num=False), -1), (dict(q_den=False), -1),
                         (dict(count=False), -1), (dict(order=False), -1), (dict(mad=False, want_mad=1), -1),
                         (dict(ptype=2), -1), (dict(ptype=-1), -1), (dict(in_kind=2), -1), (dict(out_kind=-1), -1),
                         (dict(Cn=0), -1), (dict(Cn=-1), -1), (dict(n_q=0), -1), (dict(n_q=-2), -1),
                         (dict(q=((2, 1),)), -1), (dict(q=((-1, 2),)), -1), (dict(q=((0, 0),)), -1), (dict(q=((1, 65537),)), -1),
                         (dict(q=((1, 2), (1, -4))), -1), (dict(q=nine[:8] + ((3, 2),)), -1),                  # the range before the count
                         (dict(B=0), -1), (dict(H=0), -1), (dict(W=-1), -1), (dict(max_label=0), -1), (dict(max_label=-5), -1),
                         (dict(Cn=5), -6), (dict(q=nine), -6), (dict(max_label=(1 << 20) + 1), -6),
                         (dict(B=5, max_label=1 << 20), -6), (dict(B=2, Cn=3, max_label=1 << 20), -6),
                         (dict(max_label=1 << 20, q=((1, 2),) * 5), -6), (dict(B=2, Cn=2, max_label=1 << 18, q=((1, 2),) * 5), -6),
                         (dict(B=1 << 12, Cn=4, max_label=257), -6), (dict(H=4097), -6), (dict(W=4097), -6), (dict(B=65536), -6)):
        rc, text = _call(lib, **over)
        assert rc == status and text, over
    # the order of the rules: the earlier one answers
    for over, status in ((dict(Cn=0, q=nine), -1), (dict(Cn=5, q=((2, 1),)), -1), (dict(Cn=5, B=0), -1), (dict(q=nine, max_label=0), -1),
                         (dict(H=4097, max_label=0), -1), (dict(image=False, Cn=5), -1), (dict(ptype=7, H=4097), -1)):
        assert _call(lib, **over)[0] == status, over
    assert "channels 5: at most 4" in _call(lib, Cn=5)[1] and "at most 8 quantiles" in _call(lib, q=nine)[1]
    assert "quantile 1 is 1/-4" in _call(lib, q=((1, 2), (1, -4)))[1]
    assert lib.cs_label_quantiles_last_timing(None, None, None, None) == -1


def test_a_null_handle_reports_no_device_for_valid_arguments():
    lib = L.load_library()
    no_dev = lib.cs_device_count() <= 0
    for over in (dict(), dict(exclude=True), dict(ptype=0, Cn=3), dict(mad=False), dict(want_mad=1), dict(q=((1, 2),) * 8),
                 dict(q=((0, 1), (1, 1), (65536, 65536), (0, 65536), (65535, 65536))), dict(Cn=4, max_label=1 << 20),
                 dict(B=4, max_label=1 << 20), dict(B=1 << 12, Cn=4, max_label=256), dict(B=2, Cn=2, max_label=1 << 17, q=((1, 2),) * 8),
                 dict(in_kind=1, out_kind=1), dict(H=4096, W=4096), dict(B=65535, H=1, W=1, max_label=64)):
        assert _call(lib, **over)[0] == (-4 if no_dev else -1), over      # no handle: no device here, else a NULL handle
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            QN.QuantileMeasurer(0).measure_batch(np.zeros((1, 8, 8), np.uint8), np.zeros((1, 8, 8), np.int32))
        assert ei.value.status == -4
