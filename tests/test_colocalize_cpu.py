"""CPU tests of the per-object colocalization (cs_label_colocalize, cellscreen/colocalize.py): the restatement of
tests/colocalize_reference.py against its slow form in Python ints and Fractions and against SciPy's record
tests/golden/golden_colocalize.npz, the floats the package derives against a 50-digit decimal form of the same integers, closed
forms and invariants of the rule, and the wrapper's and the C ABI's refusals before any device work.

The floats.  With u = 2^-53: a quotient of two Python ints is correctly rounded, relative error <= u.  The two with a root
(pearson, overlap) take the product of two ints to float64 (u), its root (half of that, plus u), the numerator to float64 (u) and
one division (u): at most 3.5 u and second-order terms, so ROOT_BOUND = 4 u.  SciPy's floats come from float sums and are
compared at twice SciPy's own distance from the decimal form on the golden scenes, which tools/make_golden_colocalize.py
measures and the golden file carries."""
import ctypes as C
import decimal
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import colocalize_reference as CR
import intensity_reference as IR
from cellscreen import _lib as L
from cellscreen import colocalize as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_colocalize.npz")
U = 2.0 ** -53
RATIO_BOUND = U
ROOT_BOUND = 4 * U
ROOT_FIELDS = ("pearson", "overlap")
SCIPY_PEARSON_DISTANCE = 3.574e-16      # printed by tools/make_golden_colocalize.py (3.573e-16, 3.681e-16), rounded up
SCIPY_SLOPE_DISTANCE = 3.682e-16


def same(got, want):
    for g, w in zip(got[:4], want[:4]):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


def small_cases():
    """(image [2,H,W,C], labels, exclude or None, kwargs): small enough for the slow form"""
    out = []
    for k, (shape, nc, dtype) in enumerate((((9, 14), 2, np.uint8), ((12, 11), 3, np.uint16), ((7, 20), 4, np.uint8), ((10, 10), 2, np.uint16))):
        lab = np.stack([IR.disks(shape, 5, k, radii=(2, 3)), IR.contents(shape, k + 1)[1][1]])
        image = IR.noise((2,) + shape, nc, dtype, 20 + k, spread=40 if k == 2 else None)    # few values: ties in the ranks
        ex = (IR.disks(shape, 3, k + 7, radii=(1, 2)) > 0).astype(np.int32)
        ex = np.stack([ex, np.zeros_like(ex)])
        top = int(np.iinfo(dtype).max)
        for kw in (dict(), dict(threshold=(1, 2)), dict(threshold=(0, 1)), dict(threshold=(1, 1)), dict(absolute=[top // 3] * nc),
                   dict(absolute=[0] * nc), dict(absolute=[65536] * nc), dict(rwc=False)):
            out.append((image, lab, ex if len(kw) != 1 or "rwc" in kw else None, kw))
    return out


def rel(x, d):
    """|x - d| / |d| of a float against a Decimal; 0 where both are 0"""
    if d == 0:
        return 0.0 if x == 0.0 else math.inf
    return float(abs(decimal.Decimal(x) - d) / abs(d))


def float_errors(tables, rwc=True):
    """the largest relative error of derive()'s floats against the decimal form: (of the quotients, of the two with a root)"""
    d, dec = CR.derive(*tables, rwc=rwc), CR.derive_decimal(*tables, rwc=rwc)
    worst = [0.0, 0.0]
    for f in CR.FIELDS:
        for k, row in enumerate(dec[f]):
            for p, x in enumerate(row):
                assert (x is None) == bool(np.isnan(d[f][k, p])), (f, k, p)
                if x is not None:
                    worst[f in ROOT_FIELDS] = max(worst[f in ROOT_FIELDS], rel(float(d[f][k, p]), x))
    return worst


# ---- the restatement against its slow form ------------------------------------------------------------------------------------------
def test_restatement_equals_the_slow_form_in_python_ints_and_fractions():
    for image, lab, ex, kw in small_cases():
        fast = CR.measure(image, lab, ex, **kw)
        slow = CR.measure_slow(image, lab, ex, **kw)
        same(fast, slow)
        rwc = kw.get("rwc", True)
        assert (fast[3] > 0).all() if rwc else not fast[3].any() and not fast[2][..., 7:].any()
        d = CR.derive(*fast, rwc=rwc)
        pp = CR.pairs_of(image.shape[3])
        for k in range(len(d["label"])):
            for p in range(len(pp)):
                x = slow[4][(int(d["image"][k]), int(d["label"][k]), p)]
                for f in ("slope", "k1", "k2", "manders1", "manders2", "rwc1", "rwc2"):       # both correctly rounded: equal
                    got = d[f][k, p]
                    assert (np.isnan(got) if x[f] is None else got == float(x[f])), (f, kw)
                for f in ROOT_FIELDS:
                    got, sq = d[f][k, p], x[f + "2"]
                    if sq is None:
                        assert np.isnan(got)
                    else:
                        assert abs(Fraction(got) ** 2 - sq) <= 2 * ROOT_BOUND * sq * (1 + ROOT_BOUND), (f, kw)
                        assert f != "pearson" or np.sign(got) == x["pearson_sign"] and abs(got) <= 1.0 + ROOT_BOUND


def test_the_package_table_equals_the_restatements_derivation():
    for image, lab, ex, kw in small_cases()[:12]:
        tables = CR.measure(image, lab, ex, **kw)
        rwc = kw.get("rwc", True)
        t, d = CO.colocalization_table(*tables, rwc=rwc), CR.derive(*tables, rwc=rwc)
        assert len(t) == len(d["label"]) and t.pairs == CR.pairs_of(image.shape[3]) == CO.pairs_of(image.shape[3])
        assert all(np.array_equal(getattr(t, k), v, equal_nan=v.dtype.kind == "f") for k, v in d.items())
        assert np.array_equal(t.levels, tables[3]) and t.pearson.dtype == np.float64 and t.pearson.shape == (len(t), len(t.pairs))
    with pytest.raises(TypeError):
        CO.colocalization_table(tables[0].astype(np.int32), *tables[1:])
    with pytest.raises(ValueError):
        CO.colocalization_table(tables[0], tables[1], tables[2][:, :, :0], tables[3])
    with pytest.raises(ValueError):
        CO.colocalization_table(tables[0], tables[1], tables[2], tables[3][:, :1])


# ---- the golden record of SciPy -----------------------------------------------------------------------------------------------------
def golden_cases():
    g = np.load(GOLDEN)
    for i in range(int(g["n_cases"])):
        rule = [int(x) for x in g[f"rule_{i}"]]
        kw = dict(threshold=(rule[0], rule[1])) if rule[0] >= 0 else dict(absolute=rule[2:])
        yield g, i, str(g[f"name_{i}"]), g[f"image_{i}"], g[f"labels_{i}"], g[f"exclude_{i}"], kw


# the objects of the last golden scene and what they leave undefined: (label, field) -> the pairs that are NaN
SPECIAL_NAN = {(1, "pearson"): {(0, 1), (1, 2)}, (1, "slope"): {(1, 2)},                     # channel 1 constant
               (2, "pearson"): {(0, 2), (1, 2)}, (2, "overlap"): {(0, 2), (1, 2)}, (2, "k2"): {(0, 2), (1, 2)},      # channel 2 dark
               (2, "manders2"): {(0, 2), (1, 2)}, (2, "rwc2"): {(0, 2), (1, 2)},
               (3, "overlap"): {(0, 1)}, (3, "k1"): {(0, 1)}, (3, "k2"): {(0, 1)}}           # no pixel above in both of 0 and 1


def test_golden_file_matches():
    g = np.load(GOLDEN)
    assert str(g["numpy_version"]) == "2.2.6" and str(g["scipy_version"]) == "1.15.3" and int(g["n_cases"]) == 4
    assert os.path.getsize(GOLDEN) < 200_000
    assert float(g["scipy_pearson_distance"]) <= SCIPY_PEARSON_DISTANCE and float(g["scipy_slope_distance"]) <= SCIPY_SLOPE_DISTANCE
    worst = [0.0, 0.0]
    for g, i, name, image, lab, ex, kw in golden_cases():
        geom, chan, pair, levels = CR.measure(image[None], lab[None], ex[None], **kw)
        d = CR.derive(geom, chan, pair, levels)
        pp = CR.pairs_of(image.shape[2])
        assert np.array_equal(d["label"], g[f"index_{i}"]), name
        assert np.array_equal(d["chan"], g[f"chan_{i}"]) and np.array_equal(d["pair"], g[f"pair_{i}"]), name      # the boolean masks
        assert np.array_equal(levels[0], g[f"levels_{i}"]), name                                                  # rankdata(method='dense')
        on = (lab > 0) & (ex == 0)
        for c in range(image.shape[2]):
            vals = np.unique(image[:, :, c][on])
            assert np.array_equal(np.searchsorted(vals, image[:, :, c][on]), g[f"rank_{i}"][:, :, c][on]), name
        sp, ss = g[f"pearson_{i}"], g[f"slope_{i}"]
        assert np.array_equal(np.isnan(d["pearson"]), np.isnan(sp)) and np.array_equal(np.isnan(d["slope"]), np.isnan(ss)), name
        for k in range(len(d["label"])):
            a = int(d["area"][k])
            for p, (ci, cj) in enumerate(pp):
                if not np.isnan(sp[k, p]):
                    worst[0] = max(worst[0], abs(d["pearson"][k, p] - sp[k, p]))
                if not np.isnan(ss[k, p]):
                    di = a * int(d["chan"][k, ci, 1]) - int(d["chan"][k, ci, 0]) ** 2
                    dj = a * int(d["chan"][k, cj, 1]) - int(d["chan"][k, cj, 0]) ** 2
                    worst[1] = max(worst[1], abs(d["slope"][k, p] - ss[k, p]) / (math.sqrt(dj / di) if dj else 1.0))
        # exactly the intended values are undefined
        for f in CR.FIELDS:
            for k, label in enumerate(d["label"]):
                want = SPECIAL_NAN.get((int(label), f), set()) if i == 3 else set()
                assert {pp[p] for p in range(len(pp)) if np.isnan(d[f][k, p])} == want, (name, f, int(label))
    print(f"against SciPy: pearson {worst[0]:.3e}, slope {worst[1]:.3e} (in units of the spreads' ratio)")
    assert worst[0] <= 2 * SCIPY_PEARSON_DISTANCE and worst[1] <= 2 * SCIPY_SLOPE_DISTANCE


def test_restatement_equals_scipy_live():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(4)
    x = rng.integers(0, 65536, 500)
    y = (x // 3 + rng.integers(0, 20000, 500)).astype(np.int64)
    image = np.stack([x, y], axis=-1).astype(np.uint16).reshape(1, 20, 25, 2)
    lab = np.ones((1, 20, 25), np.int32)
    tables = CR.measure(image, lab)
    d = CR.derive(*tables)
    assert abs(d["pearson"][0, 0] - stats.pearsonr(x.astype(float), y.astype(float)).statistic) <= 2 * SCIPY_PEARSON_DISTANCE
    assert abs(d["slope"][0, 0] - stats.linregress(x.astype(float), y.astype(float)).slope) <= 2 * SCIPY_SLOPE_DISTANCE
    assert int(tables[3][0, 0]) == int(stats.rankdata(x, method="dense").max()) and int(tables[3][0, 1]) == int(stats.rankdata(y, method="dense").max())


# ---- the floats against the decimal form ----------------------------------------------------------------------------------------------
def test_derived_floats_stay_within_the_bound_of_one_division_and_a_root():
    worst = [0.0, 0.0]
    for g, i, name, image, lab, ex, kw in golden_cases():
        worst = [max(a, b) for a, b in zip(worst, float_errors(CR.measure(image[None], lab[None], ex[None], **kw)))]
    for image, lab, ex, kw in small_cases():
        worst = [max(a, b) for a, b in zip(worst, float_errors(CR.measure(image, lab, ex, **kw), kw.get("rwc", True)))]
    shape = (64, 96)                                                     # large values: the products pass 2^53
    image = IR.noise((1,) + shape, 3, np.uint16, 3, base=60000, spread=5536)
    worst = [max(a, b) for a, b in zip(worst, float_errors(CR.measure(image, IR.disks(shape, 6, 2, radii=(8, 14))[None])))]
    print(f"relative error in units of 2^-53: quotients {worst[0] / U:.3f}, pearson / overlap {worst[1] / U:.3f}")
    assert worst[0] <= RATIO_BOUND and worst[1] <= ROOT_BOUND


# ---- closed forms and invariants ------------------------------------------------------------------------------------------------------
def test_a_multiple_of_a_channel_is_fully_correlated():
    shape = (20, 30)
    lab = IR.disks(shape, 5, 1)[None]
    base = IR.noise((1,) + shape, 1, np.uint8, 2, base=1)[..., 0].astype(np.uint16)
    for a in (1, 2, 3, 200):
        image = np.stack([base, a * base], axis=-1)
        d = CR.derive(*CR.measure(image, lab))
        assert len(d["label"]) > 2
        assert (d["pearson"] == 1.0).all() and (d["slope"] == float(a)).all() and (d["overlap"] == 1.0).all()
        assert (d["k1"] == float(a)).all() and (d["k2"] == 1.0 / a).all()
        assert (d["manders1"] == 1.0).all() and (d["manders2"] == 1.0).all()       # v_j = a v_i: above in one is above in the other
        assert (d["rwc1"] == 1.0).all() and (d["rwc2"] == 1.0).all()               # equal ranks: w = R


def test_threshold_zero_puts_every_pixel_above():
    for image, lab, ex, kw in small_cases()[::8]:
        for rule in (dict(threshold=(0, 1)), dict(absolute=[0] * image.shape[3])):
            geom, chan, pair, levels = CR.measure(image, lab, ex, **rule)
            assert np.array_equal(chan[..., 3], geom[..., 0:1].repeat(image.shape[3], axis=2)) and np.array_equal(chan[..., 4], chan[..., 0])
            assert np.array_equal(pair[..., 6], pair[..., 0]) and np.array_equal(pair[..., 1], geom[..., 0:1].repeat(pair.shape[2], axis=2))
            for p, (i, j) in enumerate(CR.pairs_of(image.shape[3])):
                assert np.array_equal(pair[:, :, p, 2], chan[:, :, i, 0]) and np.array_equal(pair[:, :, p, 3], chan[:, :, j, 0])
                assert np.array_equal(pair[:, :, p, 4], chan[:, :, i, 1]) and np.array_equal(pair[:, :, p, 5], chan[:, :, j, 1])
            d = CR.derive(geom, chan, pair, levels)
            ok = d["chan"][:, :, 0] > 0                                  # M is 0 / 0 only where a channel is dark on the object
            for p, (i, j) in enumerate(CR.pairs_of(image.shape[3])):
                assert (d["manders1"][ok[:, i], p] == 1.0).all() and (d["manders2"][ok[:, j], p] == 1.0).all()
        none = CR.measure(image, lab, ex, absolute=[65536] * image.shape[3])
        assert not none[1][..., 3:].any() and not none[2][..., 1:].any()


def test_swapping_two_channels_swaps_the_fields():
    image, lab, ex, _ = small_cases()[0]
    a = CR.derive(*CR.measure(image, lab, ex))
    b = CR.derive(*CR.measure(np.ascontiguousarray(image[..., ::-1]), lab, ex))
    for f, g in (("k1", "k2"), ("manders1", "manders2"), ("rwc1", "rwc2")):
        assert np.array_equal(a[f], b[g], equal_nan=True) and np.array_equal(a[g], b[f], equal_nan=True)
    assert np.array_equal(a["pearson"], b["pearson"], equal_nan=True) and np.array_equal(a["overlap"], b["overlap"], equal_nan=True)
    assert np.array_equal(a["chan"], b["chan"][:, ::-1]) and np.array_equal(a["pair"][..., [0, 1, 6]], b["pair"][..., [0, 1, 6]])
    assert np.array_equal(a["pair"][..., [2, 4, 7]], b["pair"][..., [3, 5, 8]])
    image3 = IR.noise((2,) + lab.shape[1:], 3, np.uint8, 5)              # at three channels the pairs move too: (0,1),(0,2),(1,2) -> swap 0 and 2
    a = CR.derive(*CR.measure(image3, lab))
    b = CR.derive(*CR.measure(np.ascontiguousarray(image3[..., ::-1]), lab))
    assert np.array_equal(a["manders1"], b["manders2"][:, ::-1], equal_nan=True) and np.array_equal(a["slope"][:, 1] * b["slope"][:, 1] > 0, a["pearson"][:, 1] != 0)


def test_an_image_alone_equals_its_rows_in_the_batch():
    for image, lab, ex, kw in small_cases()[:16:3]:
        whole = CR.measure(image, lab, ex, **kw)
        m = whole[0].shape[1]
        for b in range(2):
            one = CR.measure(image[b:b + 1], lab[b:b + 1], None if ex is None else ex[b:b + 1], max_label=m, **kw)
            assert all(np.array_equal(x[0], y[b]) for x, y in zip(one, whole))         # the ranks are per image


def test_ranks_ignore_background_and_excluded_pixels():
    lab = np.zeros((1, 4, 6), np.int32)
    lab[0, 1:3, 1:5] = 1
    image = np.full((1, 4, 6, 2), 9, np.uint8)
    image[0, 1:3, 1:5, 0] = [[1, 2, 3, 4], [1, 2, 3, 4]]
    image[0, 1:3, 1:5, 1] = [[5, 5, 6, 6], [7, 7, 8, 8]]
    image[0, 0, 0] = 200, 100                                            # background: no rank
    ex = np.zeros_like(lab)
    ex[0, 1, 4] = -3                                                     # the only 4 of channel 0 in row 1 ...
    ex[0, 2, 4] = 1                                                      # ... and in row 2: excluded, no rank
    geom, chan, pair, levels = CR.measure(image, lab, ex, threshold=(0, 1))
    assert levels.tolist() == [[3, 4]] and geom[0, 0, 0] == 6
    w = [4 - abs(a - b) for a, b in ((0, 0), (1, 0), (2, 1), (0, 2), (1, 2), (2, 3))]
    v0, v1 = [1, 2, 3, 1, 2, 3], [5, 5, 6, 7, 7, 8]
    assert pair[0, 0, 0, 7] == sum(a * b for a, b in zip(v0, w)) and pair[0, 0, 0, 8] == sum(a * b for a, b in zip(v1, w))


# ---- the unsigned arithmetic of the device, each product at its extreme -----------------------------------------------------------------
def test_every_product_stays_below_two_to_the_32():
    top = 2 ** 32
    assert 65535 * 65535 < top and 65535 * 65536 < top and 65536 * 65535 < top          # v_i v_j; v den and v w; num max
    for a, b in ((65535, 65535), (65535, 65536), (65536, 65535)):
        assert int(np.uint32(a) * np.uint32(b)) == a * b
    # v den and num max at their extremes: threshold 65536 / 65536 of a maximum of 65535 -- only the maximum itself is above
    lab = np.ones((1, 2, 3), np.int32)
    image = np.zeros((1, 2, 3, 2), np.uint16)
    image[0, :, :, 0] = [[65535, 65534, 0], [65535, 1, 65534]]
    image[0, :, :, 1] = [[65535, 65535, 65535], [65534, 65535, 0]]
    geom, chan, pair, levels = CR.measure(image, lab, threshold=(65536, 65536))
    assert chan[0, 0, :, 2:].tolist() == [[65535, 2, 2 * 65535], [65535, 4, 4 * 65535]] and pair[0, 0, 0, 1:4].tolist() == [1, 65535, 65535]
    same(CR.measure(image, lab, threshold=(65536, 65536)), CR.measure_slow(image, lab, threshold=(65536, 65536)))
    # v w at its extreme: 65536 distinct values in one channel, equal ranks: w = R = 65536 on a pixel of 65535
    ramp = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    image = np.stack([ramp, ramp], axis=-1)
    geom, chan, pair, levels = CR.measure(image, np.ones((1, 256, 256), np.int32), threshold=(0, 1))
    s1 = 65535 * 65536 // 2
    assert levels.tolist() == [[65536, 65536]] and pair[0, 0, 0, 7] == pair[0, 0, 0, 8] == 65536 * s1
    d = CR.derive(geom, chan, pair, levels)
    assert d["rwc1"][0, 0] == d["rwc2"][0, 0] == 1.0 and d["pearson"][0, 0] == 1.0


# ---- the package's argument checks ------------------------------------------------------------------------------------------------------
def test_thresholds_become_fractions_once():
    assert CO.as_threshold((15, 100)) == (15, 100) and CO.as_threshold(0.15) == (3, 20) and CO.as_threshold(Fraction(1, 3)) == (1, 3)
    assert CO.as_threshold(0) == (0, 1) and CO.as_threshold(1) == (1, 1) and CO.as_threshold(1.0) == (1, 1) and CO.as_threshold((65536, 65536)) == (65536, 65536)
    assert CO.as_threshold(1 / 3) == (1, 3) and CO.as_threshold(np.float32(0.5)) == (1, 2)
    for bad, exc in ((1.5, ValueError), (-0.1, ValueError), (math.nan, ValueError), ((3, 2), ValueError), ((1, 0), ValueError), ((-1, 4), ValueError),
                     ((1, 65537), ValueError), (Fraction(1, 65537), ValueError), (2, ValueError), (True, TypeError), ("0.1", TypeError),
                     ((1.0, 2), TypeError), ((1, 2, 3), TypeError), (None, TypeError)):
        with pytest.raises(exc):
            CO.as_threshold(bad)
    p = CO.colocalize_params(3)
    assert (p.thr_num, p.thr_den, p.absolute, p.rwc, list(p.abs_thr)) == (15, 100, 0, 1, [0, 0, 0, 0]) and C.sizeof(p) == 32
    p = CO.colocalize_params(3, absolute=[0, 65536, 7], rwc=False)
    assert (p.absolute, p.rwc, list(p.abs_thr)) == (1, 0, [0, 65536, 7, 0])
    for kw, exc in ((dict(absolute=[1, 2]), ValueError), (dict(absolute=[1, 2, 65537]), ValueError), (dict(absolute=[1, -1, 2]), ValueError),
                    (dict(absolute=[1.0, 2, 3]), TypeError), (dict(absolute=5), TypeError), (dict(absolute="123"), TypeError), (dict(rwc=1), TypeError),
                    (dict(rwc=None), TypeError)):
        with pytest.raises(exc):
            CO.colocalize_params(3, **kw)


def test_measurer_refusals_before_a_handle_exists():
    """ColocalizationMeasurer refuses what IntensityMeasurer refuses, with the same exceptions, before either makes a handle."""
    import torch

    import cellscreen
    from cellscreen import intensity as IN
    assert cellscreen.ColocalizationMeasurer is CO.ColocalizationMeasurer and cellscreen.ColocalizationTable is CO.ColocalizationTable
    assert cellscreen.colocalization_table is CO.colocalization_table and cellscreen.colocalize_params is CO.colocalize_params
    m, s = CO.ColocalizationMeasurer(0), IN.IntensityMeasurer(0)
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
    for image, kw, exc in ((img[..., 0], {}, ValueError), (img[..., :1], {}, ValueError),                                  # one channel: nothing to pair
                           (img, dict(threshold=1.5), ValueError), (img, dict(threshold=(1, 0)), ValueError), (img, dict(threshold="x"), TypeError),
                           (img, dict(absolute=[1, 2]), ValueError), (img, dict(absolute=[1, 2, 70000]), ValueError), (img, dict(rwc=2), TypeError)):
        for call in (m.measure_batch, m.measure_dense):
            with pytest.raises(exc):
                call(np.ascontiguousarray(image), lab, **kw)
    many = 2731                                                          # 2731 x 2 x 192 KB is just above 1 GiB
    with pytest.raises(ValueError, match="split the batch"):
        m.measure_dense(np.zeros((many, 1, 1, 2), np.uint8), np.zeros((many, 1, 1), np.int32), max_label=1)
    assert (many - 1) * 2 * CO.SCRATCH_PER_PLANE <= CO.MAX_SCRATCH < many * 2 * CO.SCRATCH_PER_PLANE
    assert m._pre is None and s._pre is None
    with pytest.raises(ValueError):
        CO.ColocalizationMeasurer(1, extractor=type("E", (), {"device_id": 0})())
    m.close()
    s.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
SYMBOLS = {"cs_label_colocalize": 17, "cs_label_colocalize_last_timing": 5}


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2 and lib.cs_profile_kernel_count() == 13
    raw = C.CDLL(L.LIB_PATH)
    for name, n_args in SYMBOLS.items():
        assert hasattr(raw, name) and name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == n_args, name


def test_the_prototypes_are_in_the_header():
    with open(os.path.join(ROOT, "include", "cellscreen.h")) as f:
        text = " ".join(f.read().split())
    assert ("int cs_label_colocalize(cs_preproc *p, const void *image, int pixel_type, int32_t channels, const int32_t *labels, "
            "const int32_t *exclude /* or NULL */, int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, "
            "const cs_colocalize_params *params, int64_t *geom, int64_t *chan, int64_t *pair, int32_t *levels, int out_kind);") in text
    assert ("int cs_label_colocalize_last_timing(const cs_preproc *p, double *clear_ms, double *moments_ms, double *ranks_ms, "
            "double *thresholded_ms);") in text
    assert "#define CS_ABI_VERSION 2 " in text and " * cs_label_colocalize " in text
    assert "v * thr_den >= thr_num * max_c" in text and "w = R - |rank_i - rank_j|" in text              # the rule is stated there


def _call(lib, image=True, labels=True, params=True, geom=True, chan=True, pair=True, levels=True, ptype=1, channels=2, B=1, H=8, W=8, in_kind=0,
          out_kind=0, max_label=4, num=15, den=100, absolute=0, abs_thr=(0, 0, 0, 0), rwc=1):
    a = np.zeros(64, np.int64)                                           # never read: every call here ends before the device
    p = a.ctypes.data
    prm = L.CSColocalizeParams()
    prm.thr_num, prm.thr_den, prm.absolute, prm.rwc = num, den, absolute, rwc
    for c, x in enumerate(abs_thr):
        prm.abs_thr[c] = x
    rc = lib.cs_label_colocalize(None, p if image else None, ptype, channels, p if labels else None, None, B, H, W, in_kind, max_label,
                                 C.byref(prm) if params else None, p if geom else None, p if chan else None, p if pair else None,
                                 p if levels else None, out_kind)
    return rc, lib.cs_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_the_handle():
    lib = L.load_library()
    for over, status in ((dict(image=False), -1), (dict(labels=False), -1), (dict(params=False), -1), (dict(geom=False), -1), (dict(chan=False), -1),
                         (dict(pair=False), -1), (dict(levels=False), -1), (dict(ptype=2), -1), (dict(in_kind=2), -1), (dict(out_kind=-1), -1),
                         (dict(channels=1), -1), (dict(channels=0), -1), (dict(B=0), -1), (dict(H=0), -1), (dict(W=-1), -1), (dict(max_label=0), -1),
                         (dict(channels=5), -6), (dict(absolute=2), -1), (dict(rwc=-1), -1), (dict(den=0), -1), (dict(num=-1), -1), (dict(num=101), -1),
                         (dict(den=65537, num=1), -1), (dict(absolute=1, abs_thr=(0, 65537, 0, 0)), -1), (dict(absolute=1, abs_thr=(-1, 0, 0, 0)), -1),
                         (dict(H=4097), -6), (dict(W=4097), -6), (dict(B=65536), -6), (dict(max_label=(1 << 20) + 1), -6),
                         (dict(B=3, max_label=1 << 20), -6), (dict(B=2731, H=1, W=1, max_label=1), -6), (dict(B=1366, channels=4, H=1, W=1, max_label=1), -6)):
        rc, text = _call(lib, **over)
        assert rc == status and text, over
    # the order of the rules: the earlier one answers
    for over, status in ((dict(channels=1, H=4097), -1), (dict(channels=5, max_label=0), -1), (dict(channels=5, den=0), -6), (dict(den=0, H=4097), -1),
                         (dict(H=4097, B=2731), -6), (dict(absolute=1, abs_thr=(0, 0, 65537, 0)), -4 if lib.cs_device_count() <= 0 else -1)):
        assert _call(lib, **over)[0] == status, over                     # the last: a threshold beyond the call's channels is not read
    assert "needs at least 2" in _call(lib, channels=1)[1] and "at most 4 are measured per call" in _call(lib, channels=5)[1]
    assert "split the batch" in _call(lib, B=2731, H=1, W=1, max_label=1)[1] and "0 <= num <= den" in _call(lib, num=101)[1]
    assert "abs_thr[1] = 65537" in _call(lib, absolute=1, abs_thr=(0, 65537, 0, 0))[1]
    assert lib.cs_label_colocalize_last_timing(None, None, None, None, None) == -1


def test_a_null_handle_reports_no_device_for_valid_arguments():
    lib = L.load_library()
    no_dev = lib.cs_device_count() <= 0
    for over in (dict(), dict(channels=4), dict(ptype=0), dict(num=0, den=1), dict(num=65536, den=65536), dict(absolute=1, abs_thr=(0, 65536, 0, 0)),
                 dict(rwc=0), dict(B=2731, H=1, W=1, max_label=1, rwc=0), dict(B=2730, H=1, W=1, max_label=1), dict(B=2, max_label=1 << 20),
                 dict(in_kind=1, out_kind=1), dict(H=4096, W=4096)):
        rc, text = _call(lib, **over)
        assert rc == (-4 if no_dev else -1) and (not no_dev or "gfx950" in text or "device" in text), over
