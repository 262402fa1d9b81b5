"""CPU tests of the per-object texture records (cs_label_texture, cellscreen/texture.py): the restatement of
tests/texture_reference.py against its slow form and against its record tests/golden/golden_texture.npz, the marginals against
the full matrices in integers, the 13 features the package derives from the records against Haralick's double sums over
p = G / N, the degenerate cases, the quantisation against its definition in Python ints, and the wrapper's and the C ABI's
refusals before any device work.

The features' tolerance is FEATURE_REL = 16 * 4.4e-14: 4.4e-14 bounds the largest relative difference between the package's
derivation and the textbook sums (the rational features exact in fractions.Fraction and rounded once, the entropies by math.fsum)
over the cases of seed 1 below (4.33e-14, measured on the CPU); the factor 16 is for the other seeds.  It is the information measures' that
is largest: they subtract entropies of about 7 bits that agree in their first digits.  No device code is involved."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import texture_reference as TR
from cellscreen import _lib as L
from cellscreen import texture as TX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_texture.npz")
FEATURE_REL = 16 * 4.4e-14
CLOGC_REL = 2.0 ** -40


def small_cases():
    """(name, image [B,H,W,C], labels, exclude or None, distance, levels, ranges)"""
    out = []
    for k, (shape, nc, dt, d, lv) in enumerate((((13, 17), 1, np.uint8, 1, 8), ((12, 15), 3, np.uint16, 2, 5), ((9, 20), 4, np.uint8, 3, 64),
                                                ((1, 1), 2, np.uint16, 1, 2), ((6, 7), 2, np.uint16, 9, 32))):
        for name, lab in TR.contents(shape, 10 + k):
            labels = np.stack([lab, np.roll(lab, 1, axis=1)])
            ex = np.stack([(lab > 0) & (np.arange(shape[1])[None, :] % 3 == 0), np.zeros(shape, bool)]).astype(np.int32) * 9
            top = int(np.iinfo(dt).max)
            ranges = [(0, top), (top // 10, top // 2), (7, 7), (0, top - 1)][:nc]
            out.append((f"{shape} {name} C{nc} {np.dtype(dt).name}", TR.noise((2,) + shape, nc, dt, 20 + k), labels, ex if k % 2 else None, d,
                        lv, ranges))
    return out


def same(a, b, name=""):
    assert len(a) == len(b) == 5
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), name
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape, (name, k)
            assert np.array_equal(x, y), (name, k)                       # clogc too: both are math.fsum of the same float64 terms


def test_restatement_equals_the_slow_form():
    for name, image, labels, ex, d, lv, ranges in small_cases():
        same(TR.measure(image, labels, d, lv, ranges, ex, glcm=True), TR.measure_slow(image, labels, d, lv, ranges, ex, glcm=True), name)
    img = np.array([[[10, 10, 200], [10, 200, 200]]], np.uint8)         # one object of 6 pixels, two levels at L = 2
    lab = np.ones((1, 2, 3), np.int32)
    c, m, s, cl, g = TR.measure(img, lab, 1, 2, [(0, 255)], max_label=2, glcm=True)
    assert c.tolist() == [[6, 0]]
    # (0, 1): (10,10) (10,200) (10,200) (200,200); (1, 1): (10,200) (10,200); (1, 0): (10,10) (10,200) (200,200); (1, -1): (10,10) (200,200)
    assert g[0, 0, 0].tolist() == [[[2, 2], [2, 2]], [[0, 2], [2, 0]], [[2, 1], [1, 2]], [[2, 0], [0, 2]]]
    assert m[0, 0, 0, 0].tolist() == [4, 4, 2, 4, 2, 0, 4, 4]           # px, ps and its padding, pd
    assert s[0, 0, 0].tolist() == [16, 8, 10, 8] and cl[0, 0, 0].tolist() == [8.0, 4.0, 4.0, 4.0]
    assert not m[0, 1].any() and not s[0, 1].any() and not cl[0, 1].any() and not g[0, 1].any()      # the absent label
    none = TR.measure(img, lab, 1, 2, [(0, 255)], exclude=lab, max_label=2, glcm=True)
    assert all(not x.any() for x in none)
    assert TR.measure(img, lab, 1, 2, [(0, 255)])[4] is None
    for bad in (-1, 3):
        lab2 = lab.copy()
        lab2[0, 0, 2] = bad
        with pytest.raises(ValueError):
            TR.measure(img, lab2, 1, 2, [(0, 255)], exclude=np.ones_like(lab), max_label=2)      # refused whatever exclude holds there
        with pytest.raises(ValueError):
            TR.measure_slow(img, lab2, 1, 2, [(0, 255)], max_label=2)
    for d, lv, ranges in ((0, 8, [(0, 255)]), (128, 8, [(0, 255)]), (1, 1, [(0, 255)]), (1, 65, [(0, 255)]), (1, 8, [(9, 8)]), (1, 8, [(-1, 8)]),
                          (1, 8, [(0, 65536)]), (1, 8, []), (1, 8, [(0, 255)] * 2)):
        with pytest.raises(ValueError):
            TR.measure(img, lab, d, lv, ranges)


def test_marginal_identities_against_the_full_matrices():
    for name, image, labels, ex, d, lv, ranges in small_cases():
        c, m, s, cl, g = TR.measure(image, labels, d, lv, ranges, ex, glcm=True)
        G = g.astype(np.int64)
        i = np.arange(lv, dtype=np.int64)
        px, ps, pd = (m[..., a:b].astype(np.int64) for a, b in ((0, lv), (lv, 3 * lv), (3 * lv, 4 * lv)))
        N = G.sum(axis=(-1, -2))
        assert np.array_equal(px.sum(-1), N) and np.array_equal(ps.sum(-1), N) and np.array_equal(pd.sum(-1), N), name
        assert not ps[..., 2 * lv - 1].any() and (N % 2 == 0).all() and np.array_equal(G, np.swapaxes(G, -1, -2)), name
        sij = (G * np.multiply.outer(i, i)).sum(axis=(-1, -2))           # sum ij G from the matrix
        twice = 2 * (i * i * px).sum(-1) - (i * i * pd).sum(-1)
        assert (twice % 2 == 0).all() and np.array_equal(sij, twice // 2), name
        assert np.array_equal(s, (G * G).sum(axis=(-1, -2))), name
        assert np.array_equal(px, G.sum(-1)), name


def noise_objects(seed):
    """(levels, matrices [n, L, L]) of noise with at least 8 occupied levels"""
    out = []
    for shape, lv, d in (((24, 24), 8, 1), ((24, 24), 13, 2), ((20, 28), 32, 1)):
        img = TR.noise((1,) + shape, 1, np.uint8, seed)
        lab = np.ones((1,) + shape, np.int32)
        lab[0, :, shape[1] // 2:] = 2
        rec = TR.measure(img, lab, d, lv, [(0, 255)], glcm=True)
        assert (rec[1][0, :, 0, :, :lv] > 0).sum(axis=-1).min() >= 8
        out.append((lv, rec))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_features_from_the_records_equal_the_textbook_sums(seed):
    worst = 0.0
    for lv, (c, m, s, cl, g) in noise_objects(seed):
        f = TX.texture_features(m, s, cl, lv)
        assert f.shape == (1, 2, 1, 4, 13) and f.dtype == np.float64
        for obj in range(2):
            for k in range(4):
                want = np.array(TR.textbook(g[0, obj, 0, k].tolist()))
                rel = np.abs(f[0, obj, 0, k] - want) / np.abs(want)
                worst = max(worst, float(rel.max()))
                assert (rel <= FEATURE_REL).all(), (seed, lv, obj, k, rel)
    print(f"seed {seed}: largest relative difference of a feature {worst:.3e}")
    t = TX.texture_table(c, m, s, cl, lv)
    d = TR.derive(c, m, s, cl, lv)
    assert len(t) == 2 and t.FEATURE_NAMES == TX.FEATURE_NAMES and len(TX.FEATURE_NAMES) == 13 and t.levels == lv
    assert all(np.array_equal(getattr(t, k), v) for k, v in d.items())
    assert np.array_equal(t.features, f[0]) and np.array_equal(t.pairs, m[0, :, :, :, :lv].sum(-1) // 2)
    assert np.allclose(t.mean, f[0].mean(axis=2), rtol=1e-15, atol=0)                              # every direction has pairs here


def test_degenerate_cases():
    img = np.full((1, 9, 11, 2), 77, np.uint8)
    img[..., 1] = TR.noise((1, 9, 11), 1, np.uint8, 3)[..., 0]
    lab = np.ones((1, 9, 11), np.int32)
    lab[0, 0, 0] = 3                                                     # a single pixel: no direction has pairs
    c, m, s, cl, _ = TR.measure(img, lab, 1, 16, [(0, 255)] * 2)
    t = TX.texture_table(c, m, s, cl, 16)
    assert t.label.tolist() == [1, 3] and t.count.tolist() == [98, 1] and t.image.tolist() == [0, 0]
    f = t.features[0, 0]                                                 # the flat channel of the large object, all four directions
    names = TX.FEATURE_NAMES
    for name, value in (("angular_second_moment", 1.0), ("contrast", 0.0), ("correlation", 1.0), ("variance", 0.0), ("entropy", 0.0),
                        ("sum_entropy", 0.0), ("difference_entropy", 0.0), ("info_measure_1", 0.0), ("info_measure_2", 0.0),
                        ("inverse_difference_moment", 1.0), ("sum_average", 2.0 * (77 * 16 // 256)), ("sum_variance", 0.0),
                        ("difference_variance", 0.0)):
        assert (f[:, names.index(name)] == value).all(), name
    assert np.array_equal(t.mean[0, 0], f[0]) and np.isfinite(t.features[0, 1]).all()
    assert np.isnan(t.features[1]).all() and np.isnan(t.mean[1]).all() and not t.pairs[1].any()    # the single pixel
    # flat objects of sizes whose N log2 N rounds: the entropy stays exactly 0, not a rounding error below it
    for n in (3, 5, 7, 11, 100, 1000):
        one = np.full((1, 1, n), 9, np.uint16)
        rec = TR.measure(one, np.ones((1, 1, n), np.int32), 1, 64, [(0, 65535)])
        ft = TX.texture_table(*rec[:4], 64).features[0, 0]
        assert ft[0, 8] == 0.0 and ft[0, 11] == 0.0 and ft[0, 12] == 0.0 and np.isnan(ft[1:]).all(), n
    # a direction without pairs: an object one pixel thick has pairs along itself only, and the mean is over that direction
    line = np.zeros((1, 7, 9), np.int32)
    line[0, 3, 1:8] = 1
    rec = TR.measure(TR.noise((1, 7, 9), 1, np.uint8, 1), line, 2, 8, [(0, 255)])
    t = TX.texture_table(*rec[:4], 8)
    assert t.pairs[0, 0].tolist() == [5, 0, 0, 0] and np.isfinite(t.features[0, 0, 0]).all() and np.isnan(t.features[0, 0, 1:]).all()
    assert np.array_equal(t.mean[0, 0], t.features[0, 0, 0])
    empty = TX.texture_table(*TR.measure(img, np.zeros_like(lab), 1, 16, [(0, 255)] * 2)[:4], 16)
    assert len(empty) == 0 and empty.features.shape == (0, 2, 4, 13) and empty.mean.shape == (0, 2, 13) and empty.pairs.shape == (0, 2, 4)
    c, m, s, cl, _ = TR.measure(img, lab, 1, 16, [(0, 255)] * 2)
    with pytest.raises(TypeError):
        TX.texture_table(c.astype(np.int64), m, s, cl, 16)
    with pytest.raises(TypeError):
        TX.texture_table(c, m, s, cl.astype(np.float32), 16)
    with pytest.raises(ValueError):
        TX.texture_table(c, m, s, cl, 8)
    with pytest.raises(ValueError):
        TX.texture_table(c, m, s[:, :1], cl, 16)
    with pytest.raises(ValueError):
        TX.texture_table(c, m, s, cl, 65)


SPANS = ((0, 65535), (0, 4095), (1000, 50000), (0, 255), (17, 17), (3, 65533))


def test_quantisation_is_the_definition_for_every_uint16_value():
    v = np.arange(65536)
    for levels in (2, 7, 32, 64):
        for lo, hi in SPANS:
            want = [((min(max(x, lo), hi) - lo) * levels) // (hi - lo + 1) for x in range(65536)]         # Python ints
            got = TR.quantise(v.astype(np.uint16), lo, hi, levels)
            assert got.dtype == np.int64 and got.tolist() == want, (levels, lo, hi)
            assert want[0] == 0 and want[-1] == (levels - 1 if hi > lo else 0) and max(want) < levels


def test_the_multiply_shift_of_the_kernel_is_the_division():
    # csrc/texture.hip takes n // span, n = v' * levels < 2^22, as (n * m) >> 40 with m = 2^40 // span + 1 (the proof is in its
    # header): here every n of the rule's range for the spans above and the two ends, in uint64 as on the device
    n = np.arange(1 << 22, dtype=np.uint64)
    for span in sorted({hi - lo + 1 for lo, hi in SPANS} | {1, 2, 3, 65535, 65536, 48271}):
        m = np.uint64((1 << 40) // span + 1)
        top = min(1 << 22, span * 64)                                    # v' < span and levels <= 64
        assert int(n[top - 1]) * int(m) < 1 << 63
        assert np.array_equal((n[:top] * m) >> np.uint64(40), n[:top] // np.uint64(span)), span


def test_golden_file_matches():
    g = np.load(GOLDEN)
    assert int(g["n_cases"]) == 4 and "pinned to the rule" in str(g["note"]) and "not to a library" in str(g["note"])
    assert os.path.getsize(GOLDEN) < 100_000
    kinds = set()
    for i in range(int(g["n_cases"])):
        image, labels, ex = g[f"image_{i}"], g[f"labels_{i}"], g[f"exclude_{i}"]
        d, lv, ranges = int(g[f"distance_{i}"]), int(g[f"levels_{i}"]), [tuple(int(x) for x in r) for r in g[f"ranges_{i}"]]
        kinds.add((image.dtype.name, image.shape[3], d, lv))
        got = TR.measure(image, labels, d, lv, ranges, ex, glcm=True)
        name = str(g[f"name_{i}"])
        for k, key in enumerate(("count", "marg", "sumsq", "clogc", "glcm")):
            want = g[f"{key}_{i}"]
            assert got[k].dtype == want.dtype and got[k].shape == want.shape, (name, key)
            if key == "clogc":                                           # log2 may differ in the last bit between libraries
                assert (np.abs(got[k] - want) <= CLOGC_REL * want).all(), name
            else:
                assert np.array_equal(got[k], want), (name, key)
        assert got[0].sum() > 0 and got[1].any()
    assert kinds == {("uint8", 2, 1, 8), ("uint16", 1, 2, 13), ("uint16", 1, 3, 64), ("uint8", 3, 5, 2)}


# ---- the package's argument checks ------------------------------------------------------------------------------------------------
def test_measurer_refusals_before_a_handle_exists():
    import torch

    import cellscreen
    assert cellscreen.TextureMeasurer is TX.TextureMeasurer and cellscreen.TextureTable is TX.TextureTable
    assert cellscreen.texture_table is TX.texture_table and TX.TextureMeasurer.FEATURE_NAMES == TX.FEATURE_NAMES
    m = TX.TextureMeasurer(0)
    img = np.zeros((2, 8, 12, 3), np.uint16)
    lab = np.zeros((2, 8, 12), np.int32)
    one = img[:, :, :, :1].copy()
    cpu_t = torch.zeros((2, 8, 12), dtype=torch.int32)
    for image, labels, kw, exc in (
            (img.astype(np.float32), lab, {}, TypeError), (img, lab.astype(np.int64), {}, TypeError), (img, lab, dict(exclude=lab.astype(bool)), TypeError),
            (list(img), lab, {}, TypeError), (img[0], lab, {}, ValueError), (img, lab[0], {}, ValueError), (img, lab[:, :, :11], {}, ValueError),
            (img[:, :, ::2], lab[:, :, ::2], {}, ValueError), (np.zeros((2, 8, 12, 5), np.uint8), lab, {}, ValueError),
            (np.zeros((1, 2, 4097), np.uint8), np.zeros((1, 2, 4097), np.int32), {}, ValueError),
            (img, cpu_t, {}, TypeError), (torch.zeros((2, 8, 12), dtype=torch.uint8), cpu_t, {}, ValueError),
            (img, lab, dict(levels=1), ValueError), (img, lab, dict(levels=65), ValueError), (img, lab, dict(levels=0), ValueError),
            (img, lab, dict(levels=8.0), TypeError), (img, lab, dict(levels=True), TypeError), (img, lab, dict(levels=None), TypeError),
            (img, lab, dict(distance=0), ValueError), (img, lab, dict(distance=128), ValueError), (img, lab, dict(distance=-1), ValueError),
            (img, lab, dict(distance=1.5), TypeError), (img, lab, dict(distance="1"), TypeError),
            (img, lab, dict(value_range=(9, 8)), ValueError), (img, lab, dict(value_range=[(0, 9), (0, 9), (5, 4)]), ValueError),
            (img, lab, dict(value_range=(-1, 8)), ValueError), (img, lab, dict(value_range=(0, 65536)), ValueError),
            (img, lab, dict(value_range=[(0, 9), (0, 9)]), ValueError), (img, lab, dict(value_range=[(0, 9)] * 4), ValueError),   # a wrong count
            (one, lab, dict(value_range=[(0, 9), (0, 9)]), ValueError), (img, lab, dict(value_range=[]), ValueError),
            (img, lab, dict(value_range=(0.0, 9.0)), TypeError), (img, lab, dict(value_range=7), TypeError),
            (img, lab, dict(value_range="ab"), TypeError), (img, lab, dict(value_range=[(0, 9), (0, 9), (0, 9, 9)]), TypeError),
            (img, lab, dict(max_label=0), ValueError), (img, lab, dict(max_label=2.0), TypeError), (img, lab, dict(max_label=True), TypeError),
            (img, lab, dict(max_label=(1 << 20) + 1), ValueError),
            (img, lab, dict(max_label=1 << 17), ValueError),                                                  # 2 x 2^17 x 3 x 32 entries
            (one, lab, dict(max_label=1 << 20, levels=16), ValueError),                                       # 2 x 2^20 x 1 x 16
            (one, lab, dict(max_label=(1 << 17) + 1, levels=64, distance=2), ValueError)):
        for call in (m.measure_batch, m.measure_dense):
            with pytest.raises(exc):
                call(image, labels, **kw)
    # the cap of the matrices: 2 x 2^12 x 3 x 32^2 cells, refused with glcm=True alone
    with pytest.raises(ValueError, match="glcm=False"):
        m.measure_dense(img, lab, max_label=1 << 12, glcm=True)
    lab2 = lab.copy()
    lab2[0, 0, 0] = (1 << 20) + 1                                        # max_label=None: the labels' maximum meets the same limits
    with pytest.raises(ValueError):
        m.measure_batch(img, lab2)
    assert m._pre is None
    assert TX.as_ranges(None, 3, 255).tolist() == [[0, 255]] * 3 and TX.as_ranges((5, 9), 2, 255).tolist() == [[5, 9]] * 2
    assert TX.as_ranges([(0, 1), (2, 3)], 2, 65535).tolist() == [[0, 1], [2, 3]] and TX.as_ranges(np.array([[7, 7]]), 1, 255).tolist() == [[7, 7]]
    with pytest.raises(ValueError):
        TX.TextureMeasurer(1, extractor=type("E", (), {"device_id": 0})())
    m.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2 and lib.cs_profile_kernel_count() == 13
    raw = C.CDLL(L.LIB_PATH)
    for name in ("cs_label_texture", "cs_label_texture_last_timing"):
        assert hasattr(raw, name) and name in L.SIGNATURES
    assert len(L.SIGNATURES["cs_label_texture"][1]) == 21 and len(L.SIGNATURES["cs_label_texture_last_timing"][1]) == 3


def test_the_prototypes_are_in_the_header():
    with open(os.path.join(ROOT, "include", "cellscreen.h")) as f:
        text = " ".join(f.read().split())
    assert ("int cs_label_texture(cs_preproc *p, const void *image, int pixel_type, int32_t channels, const int32_t *labels, "
            "const int32_t *exclude /* or NULL */, int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, "
            "int32_t levels, int32_t distance, const int32_t *range_lo, const int32_t *range_hi, int32_t *count, int32_t *marg, "
            "int64_t *sumsq, double *clogc, int32_t *glcm /* or NULL */, int out_kind);") in text
    assert "int cs_label_texture_last_timing(const cs_preproc *p, double *boxes_ms, double *matrices_ms);" in text
    assert "#define CS_ABI_VERSION 2 " in text
    assert "q(v) = ((min(max(v, lo[c]), hi[c]) - lo[c]) * levels) / (hi[c] - lo[c] + 1)" in text                # the rule is stated there
    assert "(0, d), (d, d), (d, 0), (d, -d)" in text


def _call(lib, image=True, labels=True, lo=True, hi=True, count=True, marg=True, sumsq=True, clogc=True, glcm=False, exclude=False, ptype=1,
          Cn=1, B=1, H=8, W=8, in_kind=0, out_kind=0, max_label=4, levels=8, distance=1, ranges=((0, 65535),) * 4):
    a = np.zeros(64, np.int64)                                           # never read: every call here ends before the device
    p = a.ctypes.data
    rlo = np.array([x for x, _ in ranges] + [0], np.int32)
    rhi = np.array([y for _, y in ranges] + [0], np.int32)
    rc = lib.cs_label_texture(None, p if image else None, ptype, Cn, p if labels else None, p if exclude else None, B, H, W, in_kind,
                              max_label, levels, distance, rlo.ctypes.data if lo else None, rhi.ctypes.data if hi else None,
                              p if count else None, p if marg else None, p if sumsq else None, p if clogc else None, p if glcm else None,
                              out_kind)
    return rc, lib.cs_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_the_handle():
    lib = L.load_library()
    for over, status in ((dict(image=False), -1), (dict(labels=False), -1), (dict(lo=False), -1), (dict(hi=False), -1), (dict(count=False), -1),
                         (dict(marg=False), -1), (dict(sumsq=False), -1), (dict(clogc=False), -1),
                         (dict(ptype=2), -1), (dict(ptype=-1), -1), (dict(in_kind=2), -1), (dict(out_kind=-1), -1),
                         (dict(Cn=0), -1), (dict(Cn=-1), -1), (dict(B=0), -1), (dict(H=0), -1), (dict(W=-1), -1),
                         (dict(max_label=0), -1), (dict(max_label=-5), -1),
                         (dict(levels=1), -1), (dict(levels=65), -1), (dict(levels=0), -1), (dict(levels=-8), -1),
                         (dict(distance=0), -1), (dict(distance=128), -1), (dict(distance=-1), -1),
                         (dict(ranges=((9, 8),)), -1), (dict(ranges=((-1, 8),)), -1), (dict(ranges=((0, 65536),)), -1),
                         (dict(Cn=3, ranges=((0, 9), (0, 9), (5, 4))), -1),
                         (dict(Cn=5), -6), (dict(max_label=(1 << 20) + 1), -6),
                         (dict(B=3, max_label=1 << 20), -6), (dict(B=2, Cn=3, max_label=1 << 19), -6), (dict(max_label=1 << 20, levels=17), -6),
                         (dict(max_label=(1 << 18) + 1, levels=64), -6),
                         (dict(glcm=True, max_label=(1 << 18) + 1), -6), (dict(glcm=True, max_label=(1 << 12) + 1, levels=64), -6),
                         (dict(glcm=True, B=2, Cn=2, max_label=(1 << 12) + 1, levels=32), -6),
                         (dict(H=4097), -6), (dict(W=4097), -6), (dict(B=65536), -6)):
        rc, text = _call(lib, **over)
        assert rc == status and text, over
    # the order of the rules: the earlier one answers
    for over, status in ((dict(Cn=0, levels=1), -1), (dict(Cn=5, levels=1), -6), (dict(Cn=5, B=0), -1), (dict(levels=1, max_label=0), -1),
                         (dict(levels=65, max_label=(1 << 20) + 1), -1), (dict(H=4097, distance=0), -1), (dict(H=4097, max_label=0), -1),
                         (dict(image=False, Cn=5), -1), (dict(ptype=7, H=4097), -1), (dict(ranges=((9, 8),), max_label=(1 << 20) + 1), -1)):
        assert _call(lib, **over)[0] == status, over
    assert "channels 5: at most 4" in _call(lib, Cn=5)[1] and "levels 65: must lie in 2..64" in _call(lib, levels=65)[1]
    assert "distance 128: must lie in 1..127" in _call(lib, distance=128)[1]
    assert "range of channel 2 is 5..4" in _call(lib, Cn=3, ranges=((0, 9), (0, 9), (5, 4)))[1]
    assert "cells of the matrices" in _call(lib, glcm=True, max_label=(1 << 18) + 1)[1]
    assert lib.cs_label_texture_last_timing(None, None, None) == -1


def test_a_null_handle_reports_no_device_for_valid_arguments():
    lib = L.load_library()
    no_dev = lib.cs_device_count() <= 0
    for over in (dict(), dict(exclude=True), dict(ptype=0, Cn=3), dict(glcm=True), dict(levels=2), dict(levels=64, distance=127),
                 dict(ranges=((0, 0),)), dict(ranges=((65535, 65535),)), dict(Cn=4, ranges=((0, 255), (1, 2), (1000, 50000), (0, 65535))),
                 dict(max_label=1 << 20, levels=16), dict(B=2, Cn=4, max_label=1 << 16, levels=32), dict(max_label=1 << 18, levels=64),
                 dict(glcm=True, max_label=1 << 18), dict(glcm=True, max_label=1 << 12, levels=64),
                 dict(in_kind=1, out_kind=1), dict(H=4096, W=4096), dict(B=65535, H=1, W=1, max_label=32)):
        assert _call(lib, **over)[0] == (-4 if no_dev else -1), over      # no handle: no device here, else a NULL handle
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            TX.TextureMeasurer(0).measure_batch(np.zeros((1, 8, 8), np.uint8), np.zeros((1, 8, 8), np.int32))
        assert ei.value.status == -4
