"""CPU tests of the segmenter's noise-adaptive threshold (cs_segment_noise, ThresholdSegmenter(threshold="noise", ...)): the
restatement of tests/noise_reference.py against a slow independent form in exact rationals and against its golden
(tests/golden/golden_noise.npz), the degenerate cases and the tie rule, the scene table of DESIGN 3r, and the wrapper's and the
C ABI's refusals before any device work."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import noise_arg_cases as NA
import noise_reference as NR
import segment_reference as R
from cellscreen import _lib as L
from cellscreen import segment as S
from test_local_cpu import dim_cell_scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_noise.npz")


# ---- the slow form: plain Python, exact rationals, no code shared with the restatement ---------------------------------------------
def slow_tiles(n, T):
    m = max(1, n // T)
    return [(i * T, n if i == m - 1 else (i + 1) * T) for i in range(m)]


def slow_mesh(x, T, floor):
    """(B, S) as lists of lists of Fractions in counts, after the 3 x 3 filter; floor in counts as a Fraction."""
    ty, tx = slow_tiles(x.shape[0], T), slow_tiles(x.shape[1], T)
    B, Sg = [], []
    for y0, y1 in ty:
        B.append([])
        Sg.append([])
        for x0, x1 in tx:
            v = sorted(int(x[y, xx]) for y in range(y0, y1) for xx in range(x0, x1))
            r = (len(v) - 1) // 2
            med = v[r]
            dev = sorted(abs(q - med) for q in v)[r]
            B[-1].append(Fraction(med))
            Sg[-1].append(max(Fraction((dev * 97164) >> 8, 256), floor))          # the one rounding of the definition
    my, mx = len(ty), len(tx)

    def filt(a):
        clamp = lambda i, n: min(max(i, 0), n - 1)
        return [[sorted(a[clamp(j + dj, my)][clamp(i + di, mx)] for dj in (-1, 0, 1) for di in (-1, 0, 1))[4] for i in range(mx)]
                for j in range(my)]

    return filt(B), filt(Sg), ty, tx


def slow_axis(p, tiles):
    """[(node, weight)] of pixel p: linear between the tile centres, constant outside the outer ones."""
    centres = [Fraction(s + e - 1, 2) for s, e in tiles]
    if len(centres) == 1 or p <= centres[0]:
        return [(0, Fraction(1))]
    if p >= centres[-1]:
        return [(len(centres) - 1, Fraction(1))]
    i = max(k for k, c in enumerate(centres) if c <= p)
    t = (p - centres[i]) / (centres[i + 1] - centres[i])
    return [(i, 1 - t), (i + 1, t)]


def slow_levels(x, T, k8, weak8, floor8):
    B, Sg, ty, tx = slow_mesh(x, T, Fraction(floor8, 256))
    k, kw = Fraction(k8, 256), (None if weak8 is None else Fraction(weak8, 256))
    out = np.zeros(x.shape, np.uint8)
    for y in range(x.shape[0]):
        wy = slow_axis(y, ty)
        for xx in range(x.shape[1]):
            wx = slow_axis(xx, tx)
            b = sum(a * c * B[j][i] for j, a in wy for i, c in wx)
            s = sum(a * c * Sg[j][i] for j, a in wy for i, c in wx)
            v = int(x[y, xx])
            out[y, xx] = int(v - b > k * s) + (0 if kw is None else int(v - b > kw * s))
    return out, B, Sg


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_restatement_equals_the_slow_form_in_exact_rationals(dtype):
    seen = set()
    for shape in ((1, 1), (1, 40), (40, 1), (16, 16), (15, 17), (17, 33), (33, 31), (32, 48), (40, 40)):
        x = NR.noise_field(shape, dtype, seed=3)
        for k8, weak8, floor8 in ((1280, None, 256), (1536, 768, 256), (300, 77, 0), (16383, 1, 1000)):
            want, B, Sg = slow_levels(x, 16, k8, weak8, floor8)
            m = NR.mesh(x, 16, floor8)
            assert m.dtype == np.int32 and m.shape == (2, len(B), len(B[0]))
            assert [[Fraction(int(q), 256) for q in row] for row in m[0]] == B
            assert [[Fraction(int(q), 256) for q in row] for row in m[1]] == Sg
            got = NR.levels(x, 16, k8, weak8, floor8)
            assert np.array_equal(got, want), (shape, k8, weak8, floor8, int((got != want).sum()))
            seen |= set(int(q) for q in np.unique(got))
    assert seen == {0, 1, 2}


def test_restatement_equals_its_golden():
    g = np.load(GOLDEN)
    inputs = NR.golden_inputs()
    rules = [(int(k), None if w < 0 else int(w), int(f), int(c)) for k, w, f, c in g["rules"]]
    assert int(g["n"]) == len(inputs) == 16 and rules == NR.GOLDEN_RULES
    for i, (x, T) in enumerate(inputs):
        assert np.array_equal(g[f"x_{i}"], x) and g[f"x_{i}"].dtype == x.dtype and int(g[f"tile_{i}"]) == T
        for f in (0, 256):
            assert np.array_equal(NR.mesh(x, T, f), g[f"mesh_{f}_{i}"]), (i, f)
        for r, (k8, weak8, f, c) in enumerate(rules):
            want = np.unpackbits(g[f"p_{r}_{i}"])[:x.size].reshape(x.shape)
            assert np.array_equal(NR.noise_mask(x, T, k8, weak8, f, c), want), (i, r)


def test_mesh_geometry():
    assert NR.axis_tiles(1, 16) == [(0, 1)] and NR.axis_tiles(15, 16) == [(0, 15)] and NR.axis_tiles(31, 16) == [(0, 31)]
    assert NR.axis_tiles(32, 16) == [(0, 16), (16, 32)] and NR.axis_tiles(47, 16) == [(0, 16), (16, 47)]
    assert NR.axis_tiles(49, 16) == [(0, 16), (16, 32), (32, 49)] and NR.axis_tiles(767, 256)[-1] == (256, 767)
    for n, T in ((1, 16), (31, 16), (32, 16), (47, 16), (49, 16), (300, 64), (767, 256)):
        i0, i1, w0, w1, D = NR.axis_weights(n, T)
        assert (w0 + w1 == D).all() and (w0 >= 0).all() and (w1 >= 0).all() and (D >= 1).all() and int(D.max()) <= 3 * T - 1
        assert (w0[0], w1[0]) == (D[0], 0) and (n // T < 2 or (w0[-1], w1[-1]) == (0, D[-1]))        # constant outside the centres
    # a mesh that is linear in the node's centre is reproduced exactly between the outer centres
    x = np.zeros((1, 100), np.uint16)
    c2 = np.array([s + e - 1 for s, e in NR.axis_tiles(100, 16)], np.int64)
    m = np.stack([c2[None, :] * 128, c2[None, :] * 0 + 256]).astype(np.int32)                      # B8 = 256 * centre
    NB, NS, D = NR.maps(x, 16, 256, m)
    inner = slice(int(c2[0] + 1) // 2, int(c2[-1]) // 2 + 1)
    assert np.array_equal(NB[0, inner], (256 * np.arange(100) * D[0])[inner]) and np.array_equal(NS, 256 * D)


def test_degenerate_images_and_the_tie_rule():
    for dtype in (np.uint8, np.uint16):
        for shape in ((1, 1), (1, 50), (50, 1), (9, 14), (33, 47)):
            x = np.full(shape, 77, dtype)
            for T in (16, 64):
                assert not NR.noise_mask(x, T).any()                    # a constant image is all background
                assert not NR.noise_mask(x, T, 1, None, 0).any()        # even at the least k without a floor: 0 > 0 is a tie
                m = NR.mesh(x, T, 256)
                assert (m[0] == 77 * 256).all() and (m[1] == 256).all() and NR.segment(x, T)[1:] == (0, -1)
        b = 100
        x = np.full((40, 56), b, dtype)                                 # MAD 0, floor 1 count, k = 5: the cut is b + 5
        x[3, 5], x[17, 17], x[20, 30], x[39, 55] = b + 5, b + 5, b + 6, b + 6
        for T in (16, 32, 64):
            plane = NR.noise_mask(x, T)
            assert plane.sum() == 2 and plane[20, 30] == 1 and plane[39, 55] == 1
        assert NR.noise_mask(x, 16, 1279).sum() == 4                    # a hair under 5 sigmas lets the tie through
        lv = NR.levels(x, 16, 1536, 1279)
        assert (lv == 1).sum() == 4 and not (lv == 2).any() and not NR.noise_mask(x, 16, 1536, 1279).any()
    one = np.array([[5, 5, 5, 9, 5, 200, 5]], np.uint8)                 # one tile, a single row: med 5, dev 0
    assert NR.noise_mask(one, 16).tolist() == [[0, 0, 0, 0, 0, 1, 0]] and NR.noise_mask(one.T.copy(), 16).T.tolist() == [[0, 0, 0, 0, 0, 1, 0]]
    assert NR.noise_mask(one, 16, 768).tolist() == [[0, 0, 0, 1, 0, 1, 0]]
    two = np.array([[10, 20, 10, 20]], np.uint16)                       # the lower median and the lower deviation
    assert NR.mesh(two, 16, 0).ravel().tolist() == [2560, 0]
    with pytest.raises(ValueError):
        NR.mesh(two, 48, 0)
    with pytest.raises(ValueError):
        NR.levels(two, 16, 1280, 1281)
    with pytest.raises(TypeError):
        NR.mesh(two.astype(np.int32), 16, 0)


# ---- the scene table of DESIGN 3r -------------------------------------------------------------------------------------------------
TABLE = {                                                               # (components per seed 0 / 1 / 2, cells covered at their centres)
    ("otsu", "flat"): ((20, 20, 20), 20), ("otsu", "sloped"): ((20, 20, 20), 20),
    ("k5", "flat"): ((43, 48, 45), 40), ("k5", "sloped"): ((41, 40, 40), 40),
    ("k6w3", "flat"): ((40, 38, 39), 40), ("k6w3", "sloped"): ((40, 40, 40), 40),
}


@pytest.mark.parametrize("scene", ["flat", "sloped"])
def test_scene_table(scene):
    got = {rule: [] for rule in ("otsu", "k5", "k6w3")}
    for seed in (0, 1, 2):
        img, cells = dim_cell_scene(seed)
        if scene == "sloped":
            yy, xx = np.mgrid[0:512, 0:512]
            img = np.clip(img.astype(np.int64) + 3 * xx + 2 * yy, 0, 65535).astype(np.uint16)
        t = R.otsu(img)
        assert (2572 <= t <= 2575) if scene == "flat" else (3825 <= t <= 3905)
        m = NR.mesh(img, 64, 256)
        if scene == "flat":
            assert 300 * 256 <= m[0].min() and m[0].max() <= 320 * 256 and 25.2 * 256 <= m[1].min() and m[1].max() <= 55 * 256
        else:
            assert 74 * 256 <= m[1].min() and m[1].max() <= 135 * 256     # a slope inside a tile inflates the sigma: the noise is 25
        planes = {"otsu": img > t, "k5": NR.noise_mask(img, 64, 1280) > 0, "k6w3": NR.noise_mask(img, 64, 1536, 768) > 0}
        for rule, plane in planes.items():
            got[rule].append((R.label_mask(plane, 1)[1], sum(int(plane[y, x]) for y, x, _, _ in cells)))
    for rule, rows in got.items():
        comps, covered = TABLE[rule, scene]
        assert tuple(r[0] for r in rows) == comps and all(r[1] == covered for r in rows), (rule, scene, rows)


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------
def test_noise_params_refuses_every_bad_value():
    nan = float("nan")
    for kw, exc in ((dict(noise_k=0), ValueError), (dict(noise_k=0.001), ValueError), (dict(noise_k=-5.0), ValueError),
                    (dict(noise_k=64.0), ValueError), (dict(noise_k=1e30), ValueError), (dict(noise_k=nan), ValueError),
                    (dict(noise_k=float("inf")), ValueError), (dict(noise_k=True), TypeError), (dict(noise_k="5"), TypeError),
                    (dict(noise_k=None), TypeError),
                    (dict(noise_tile=8), ValueError), (dict(noise_tile=48), ValueError), (dict(noise_tile=512), ValueError),
                    (dict(noise_tile=0), ValueError), (dict(noise_tile=64.0), TypeError), (dict(noise_tile=True), TypeError),
                    (dict(noise_tile=None), TypeError), (dict(noise_tile="64"), TypeError),
                    (dict(noise_floor=-0.5), ValueError), (dict(noise_floor=4095.5), ValueError), (dict(noise_floor=nan), ValueError),
                    (dict(noise_floor=False), TypeError), (dict(noise_floor=None), TypeError), (dict(noise_floor="1"), TypeError),
                    (dict(weak_k=0), ValueError), (dict(weak_k=5.01), ValueError), (dict(weak_k=-1.0), ValueError),
                    (dict(weak_k=nan), ValueError), (dict(weak_k=True), TypeError), (dict(weak_k="3"), TypeError),
                    (dict(noise_k=3.0, weak_k=4.0), ValueError)):
        with pytest.raises(exc):
            S.noise_params(**kw)
        with pytest.raises(exc):
            S.ThresholdSegmenter(0, threshold="noise", **kw)
        with pytest.raises(exc):
            S.threshold_cell_extractor(0, threshold="noise", **kw)
    for c in (0, 3, True, None):
        with pytest.raises(ValueError):
            S.noise_params(connectivity=c)
    p = S.noise_params()
    assert (p.tile, p.k8, p.weak_k8, p.floor8, p.connectivity, list(p.reserved)) == (64, 1280, -1, 256, 1, [0, 0, 0])
    assert C.sizeof(L.CSNoiseParams) == 32
    p = S.noise_params(np.float32(6.0), np.int64(256), 0, 3, 2)
    assert (p.tile, p.k8, p.weak_k8, p.floor8, p.connectivity) == (256, 1536, 768, 0, 2)
    p = S.noise_params(63.99, 16, 4095, 63.99)
    assert (p.k8, p.weak_k8, p.floor8) == (16381, 16381, 4095 * 256)
    assert S.noise_params(1 / 256).k8 == 1 and S.noise_params(0.002).k8 == 1 and S.noise_params(5, weak_k=5).weak_k8 == 1280
    for k in (0.5, 2.25, 5.0, 6.0, 63.9):
        assert S.noise_params(k).k8 == NR.k8_of(k)


def test_segmenter_modes_and_refusals_before_a_handle_exists():
    for kw in (dict(noise_k=6.0), dict(noise_tile=32), dict(noise_floor=2.0), dict(weak_k=3.0), dict(threshold=500, noise_k=4.0),
               dict(threshold="local", local_radius=25, weak_k=3.0), dict(noise_floor=0)):
        with pytest.raises(ValueError):
            S.ThresholdSegmenter(0, **kw)                             # noise_* with another threshold
        with pytest.raises(ValueError):
            S.threshold_cell_extractor(0, **kw)
    for kw in (dict(local_radius=25), dict(local_delta=5), dict(local_floor=0), dict(weak_threshold=0.5), dict(weak_threshold=100),
               dict(weak_delta=3), dict(denoise=True)):
        with pytest.raises(ValueError):
            S.ThresholdSegmenter(0, threshold="noise", **kw)          # another rule's numbers with "noise"; denoise needs its stage
        with pytest.raises(ValueError):
            S.threshold_cell_extractor(0, threshold="noise", **kw)
    with pytest.raises(ValueError) as ei:
        S.segment_params("noise")                                     # the global parameters know no such mode, and say what they said
    assert str(ei.value) == "threshold must be 'otsu' or an integer, got 'noise'"
    s = S.ThresholdSegmenter(0, threshold="noise", noise_k=6, noise_tile=128, noise_floor=2.5, weak_k=3, connectivity=2, fill_holes=False)
    assert (s._noise.tile, s._noise.k8, s._noise.weak_k8, s._noise.floor8, s._noise.connectivity) == (128, 1536, 768, 640, 2)
    assert (s._params.threshold_mode, s._params.threshold, s._params.connectivity, s._params.fill_holes) == (L.THRESH_FIXED, 0, 2, 0)
    assert s._local is None and s._hysteresis is None and s._background is None and s._smooth is None
    assert s.threshold == "noise" and (s.noise_k, s.noise_tile, s.noise_floor, s.weak_k) == (6.0, 128, 2.5, 3.0)
    s = S.ThresholdSegmenter(0, threshold="noise", background_radius=51, denoise=True, smooth_sigma=1.5, min_area=20, split_touching=True,
                             split_by="intensity")
    assert s._noise.weak_k8 == -1 and s._background.median == 0 and s._smooth.median == 1 and s._clean.min_area == 20   # the median runs once
    assert S.ThresholdSegmenter(0, threshold="noise", background_radius=51, denoise=True)._background.median == 1
    img = np.zeros((1, 16, 16, 3), np.uint16)
    for im, ch, exc in ((img.astype(np.float32), None, TypeError), (img[..., :2].copy(), None, ValueError), (img, 3, ValueError),
                        (img[:, :, :8], None, ValueError), (np.zeros((1, 2, 4097), np.uint8), None, ValueError)):
        for fn in (s.noise_mask_batch, s.noise_mesh_batch, s.segment_batch):
            with pytest.raises(exc):
                fn(im, channel=ch)
    plain = S.ThresholdSegmenter(0)
    for fn in (plain.noise_mask_batch, plain.noise_mesh_batch):
        with pytest.raises(ValueError):
            fn(img)                                                   # no noise rule: no mask and no mesh
    assert s._pre is None and plain._pre is None
    assert plain._noise is None and (plain.noise_k, plain.noise_tile, plain.noise_floor, plain.weak_k) == (5.0, 64, 1.0, None)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2
    raw = C.CDLL(L.LIB_PATH)
    assert hasattr(raw, "cs_segment_noise") and hasattr(raw, "cs_segment_noise_last_timing")
    assert "cs_segment_noise" in L.SIGNATURES and "cs_segment_noise_last_timing" in L.SIGNATURES


def test_c_abi_refusals_status_and_text():
    lib = L.load_library()
    names = set()
    for over, status, text in NA.CASES:
        assert NA.call(lib, over) == (status, text), over
        names.add(tuple(sorted((k, repr(v)) for k, v in over.items())))
    assert len(names) == len(NA.CASES) >= 50                          # no case twice
    assert lib.cs_segment_noise_last_timing(None, None, None, None) == -1


def test_c_abi_reports_no_device_for_valid_arguments():
    lib = L.load_library()
    no_dev = lib.cs_device_count() <= 0
    for over in (dict(), dict(noise=NA.noise(16, 1, -1, 0)), dict(noise=NA.noise(256, 16383, 16383, 4095 * 256, 2)), dict(mesh=None),
                 dict(okind=1), dict(noise=NA.noise(conn=7))):
        assert NA.call(lib, over)[0] == (-4 if no_dev else -1), over  # no handle: no device here, else a NULL handle
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            S.ThresholdSegmenter(0, threshold="noise").noise_mask_batch(np.zeros((1, 32, 32), np.uint16))
        assert ei.value.status == -4
