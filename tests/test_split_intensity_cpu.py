"""CPU tests of the segmenter's split_by="intensity" option (cs_segment_split_intensity): the restatement of
tests/split_intensity_reference.py on the scene the option was specified on, the properties the definition promises,
tests/golden/golden_split_intensity.npz, and the wrapper's and the C ABI's refusals before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

import segment_reference as R
import smooth_reference as MR
import split_intensity_reference as IR
import split_reference as SR
from cellscreen import _lib as L
from cellscreen import segment as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_split_intensity.npz")


@pytest.fixture(scope="module")
def smoothed():
    """(guide, mask, plain labels) of the scene with noise 60, smoothed with sigma 1.5 and cut by Otsu: computed once."""
    g = MR.smooth_sigma(IR.scene(60.0), 1.5)
    m = R.mask_of(g, R.otsu(g), True)
    return g, m, R.label_mask(m, 1)[0]


def test_distance_split_leaves_the_scene_whole_and_the_intensity_split_finds_its_cells(smoothed):
    """5 components without one neck: the distance split at h 3 returns them unchanged.  The intensity split at the default
    depth returns 10 regions for the 11 cells (the 1500-count cell beside the 3500-count one is a shoulder of it after the
    smoothing, not a core of its own), with the sizes recorded here from the restatement, in label order."""
    g, m, plain = smoothed
    assert plain.max() == 5
    lab, n, _ = SR.split_mask(m, 1, 3)
    assert n == 5 and np.array_equal(lab, plain)
    lab, n, hq = IR.split_intensity(m, g, 1, S.SPLIT_DEPTH)
    assert S.SPLIT_DEPTH == 16 and 9 <= n <= 11
    assert n == 10
    assert list(np.bincount(lab.ravel())[1:]) == [534, 510, 256, 205, 340, 1123, 531, 480, 407, 334]
    assert [int(lab[cy, cx]) for cy, cx, _, _ in IR.CELLS] == [1, 2, 6, 6, 5, 4, 3, 8, 9, 7, 10]
    assert np.array_equal(lab > 0, m) and hq.dtype == np.uint8 and hq[m].min() == 1 and hq[m].max() == 255 and not hq[~m].any()
    owner = np.zeros(n + 1, np.int64)
    owner[lab[m]] = plain[m]
    assert np.array_equal(owner[lab][m], plain[m])                          # no region spans two components
    for depth in (8, 12, 20):                                               # the default sits inside a stable range
        assert IR.split_intensity(m, g, 1, depth)[1] == 10
    assert IR.split_intensity(m, g, 1, 64)[1] == 9


def test_batch_function_is_the_stages_in_order(smoothed):
    g, m, _ = smoothed
    lab, n, thr, hq, guide = IR.segment_batch(IR.scene(60.0)[None], smooth_sigma=1.5)
    assert np.array_equal(guide[0], g) and thr[0] == R.otsu(g) and n[0] == 10
    assert np.array_equal(lab[0], IR.split_intensity(m, g, 1, 16)[0]) and np.array_equal(hq[0], IR.heights(m, g, 1, 0))
    noisy = IR.segment_batch(IR.scene(150.0)[None])[1][0]                   # no smoothing: every noise peak is a seed
    assert noisy > 40


def test_consequences_of_the_definition(smoothed):
    """depth 254, a constant guide and a contrast floor that leaves a component fewer levels than the depth all give one seed
    per component: the plain labels bit for bit.  Adding a constant to the guide changes nothing.

    The contrast rule, exactly: a component whose heights span (hi - lo) * 254 // max(hi - lo, m, 1) <= depth levels has a
    marker that nowhere exceeds its lowest height, so the reconstruction is one plateau.  A floor of at least 254 times the
    image's range therefore gives plain labels at every depth >= 1; a floor of merely the range does not (it leaves the full 254
    levels), which the last assertion records."""
    g, m, plain = smoothed
    rng = np.random.default_rng(3)
    cases = [(m, g), (rng.random((40, 50)) < 0.7, rng.integers(0, 65536, (40, 50)).astype(np.uint16)),
             (np.ones((9, 11), bool), rng.integers(0, 256, (9, 11)).astype(np.uint8)), (np.zeros((4, 5), bool), np.zeros((4, 5), np.uint8))]
    for mask, guide in cases:
        for c in (1, 2):
            el, en = R.label_mask(mask, c)
            lab, n, _ = IR.split_intensity(mask, guide, c, 254)
            assert n == en and np.array_equal(lab, el)
            lab, n, hq = IR.split_intensity(mask, np.full_like(guide, 777 if guide.dtype == np.uint16 else 77), c, 1)
            assert n == en and np.array_equal(lab, el) and set(np.unique(hq[mask])) <= {1}
    rng_all = int(g.max()) - int(g.min())
    assert 254 * rng_all > 65535                                            # the uint16 scene is too wide for a floor of 254 ranges
    lab, n, _ = IR.split_intensity(m, g, 1, 16, 65535)                      # 2597 * 254 // 65535 = 10 levels <= 16
    assert n == 5 and np.array_equal(lab, plain)
    g8 = MR.smooth_sigma(IR.scene(60.0, dtype=np.uint8), 1.5)
    m8 = R.mask_of(g8, R.otsu(g8), True)
    assert IR.split_intensity(m8, g8, 1, 16)[1] == 10
    lab, n, hq = IR.split_intensity(m8, g8, 1, 1, 254 * 255)                # at least 254 ranges: at most 2 levels, depth 1 is enough
    assert n == R.label_mask(m8, 1)[1] and np.array_equal(lab, R.label_mask(m8, 1)[0]) and hq.max() <= 2
    assert IR.split_intensity(m, g, 1, 16, rng_all)[1] == 9                 # a floor of the range itself still splits
    shifted = (g.astype(np.int64) + 20000).astype(np.uint16)
    for c in (1, 2):
        a, b = IR.split_intensity(m, g, c, 16, 40), IR.split_intensity(m, shifted, c, 16, 40)
        assert a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


def test_heights_scale_every_component_on_its_own():
    g = np.array([[10, 20, 30, 0, 1000, 3000, 65535], [0, 0, 0, 0, 0, 0, 0], [5, 0, 7, 7, 0, 0, 65535]], np.uint16)
    m = g > 0
    hq = IR.heights(m, g, 1, 0)
    assert list(hq[0]) == [1, 128, 255, 0, 1, 1 + (2000 * 254) // 64535, 255] and list(hq[2]) == [1, 0, 1, 1, 0, 0, 1]
    assert list(IR.heights(m, g, 1, 40)[0][:3]) == [1, 1 + 2540 // 40, 1 + 5080 // 40]
    full = np.array([[0, 65535, 12345]], np.uint16)
    assert list(IR.heights(np.ones((1, 3), bool), full, 1, 0)[0]) == [1, 255, 1 + (12345 * 254) // 65535]
    with pytest.raises(TypeError):
        IR.heights(m, g.astype(np.int32))
    with pytest.raises(ValueError):
        IR.split_intensity(m, g, 1, 255)


def test_golden():
    gold = np.load(GOLDEN)
    n = int(gold["n"])
    assert n >= 10 and gold["versions"][0] == "scipy 1.15.3" and "SciPy 1.15.3" in str(gold["note"])
    names = list(gold["names"])
    assert {"scene", "dim_bright", "saturated", "flat", "one_pixel"} <= set(names)
    split_somewhere = False
    for i in range(n):
        g, m, contrast = gold[f"guide_{i}"], gold[f"mask_{i}"], int(gold[f"contrast_{i}"])
        assert m.dtype == bool and g.dtype in (np.uint8, np.uint16)
        for c in (1, 2):
            assert R.label_mask(m, c)[1] == int(gold[f"base_{c}_{i}"])
            assert np.array_equal(IR.heights(m, g, c, contrast), gold[f"hq_{c}_{i}"]), (names[i], c)
            for d in (4, 16, 64):
                lab, k, hq = IR.split_intensity(m, g, c, d, contrast)
                assert lab.dtype == np.int32 and np.array_equal(lab, gold[f"lab_{c}_{d}_{i}"]) and k == int(gold[f"n_{c}_{d}_{i}"]), (names[i], c, d)
                assert np.array_equal(hq, gold[f"hq_{c}_{i}"])
                split_somewhere |= k > int(gold[f"base_{c}_{i}"])
    assert split_somewhere
    i = names.index("dim_bright")                                           # the dim pair splits beside the bright one
    assert int(gold[f"n_1_16_{i}"]) == 4 and int(gold[f"base_1_{i}"]) == 2
    i = names.index("flat")
    assert set(np.unique(gold[f"hq_1_{i}"])) == {0, 1}
    i, j = names.index("faint"), names.index("faint_guarded")
    assert int(gold[f"n_1_4_{i}"]) > int(gold[f"n_1_4_{j}"]) == int(gold[f"base_1_{j}"])


def test_symbols_signatures_and_abi_version():
    lib = L.load_library()
    for name in ("cs_segment_split_intensity", "cs_segment_split_intensity_last_timing", "cs_segment_split_last_syncs"):
        assert name in L.SIGNATURES and getattr(lib, name) is not None
    assert lib.cs_abi_version() == 2
    assert C.sizeof(L.CSSplitIntensityParams) == 16
    assert len(L.SIGNATURES["cs_segment_split_intensity"][1]) == 20


def test_wrapper_refuses_bad_arguments_before_device_work():
    on = dict(split_touching=True, split_by="intensity")
    bad_value = [dict(split_by="intensity"),                                # needs split_touching
                 dict(split_touching=True, split_by="gradient"), dict(split_by="Distance"),
                 dict(split_depth=8), dict(split_contrast=40), dict(split_touching=True, split_depth=8),        # belong to "intensity"
                 dict(split_touching=True, split_by="distance", split_contrast=1),
                 dict(on, split_h=4), dict(on, split_h=1),                  # belongs to "distance"
                 dict(on, split_depth=0), dict(on, split_depth=255), dict(on, split_depth=-1),
                 dict(on, split_contrast=-1), dict(on, split_contrast=65536),
                 dict(split_depth=0), dict(split_contrast=70000)]
    for kw in bad_value:
        with pytest.raises(ValueError):
            S.ThresholdSegmenter(0, **kw)
        with pytest.raises(ValueError):
            S.threshold_cell_extractor(0, **kw)
    for kw in (dict(on, split_depth=2.5), dict(on, split_depth=True), dict(on, split_contrast=1.0), dict(on, split_contrast=None),
               dict(split_touching=True, split_by=1), dict(split_by=None), dict(on, split_h=3.0)):
        with pytest.raises(TypeError):
            S.ThresholdSegmenter(0, **kw)
        with pytest.raises(TypeError):
            S.threshold_cell_extractor(0, **kw)
    assert S.split_intensity_params() is None and S.split_intensity_params(True, "distance", 7) is None
    p = S.split_intensity_params(True, "intensity", 3, 25, 300)
    assert (p.depth, p.min_contrast, p.reserved[0], p.reserved[1]) == (25, 300, 0, 0)
    s = S.ThresholdSegmenter(0, smooth_sigma=1.5, split_depth=32, split_contrast=5, **on)
    assert (s.split_by, s.split_depth, s.split_contrast, s.split_touching) == ("intensity", 32, 5, True)
    d = S.ThresholdSegmenter(0, split_touching=True, split_h=5)
    assert (d.split_by, d.split_depth, d.split_contrast) == ("distance", 16, 0) and d._split_intensity is None
    img = IR.scene(0.0)[None]
    for im, exc in ((img.astype(np.float32), TypeError), (img[:, :, :100], ValueError), (np.zeros((1, 2, 4097), np.uint8), ValueError)):
        with pytest.raises(exc):
            s.segment_batch(im, return_distance=True)
    with pytest.raises(ValueError):
        S.ThresholdSegmenter(0).segment_batch(img, return_distance=True)
    with pytest.raises(ValueError):
        S.ThresholdSegmenter(0).last_host_syncs()                           # the plain segmenter has no rounds to count
    assert s._pre is None and d._pre is None
    S.threshold_cell_extractor(0, smooth_sigma=1.5, **on)                   # valid: no handle either, nothing to close


def test_c_abi_refuses_and_reports_no_device():
    lib = L.load_library()
    img = IR.scene(0.0)[None]
    H, W = img.shape[1:]
    labels, hq = np.zeros((1, H, W), np.int32), np.zeros((1, H, W), np.uint8)
    n, thr = np.zeros(1, np.int32), np.zeros(1, np.int32)

    def params(mode=0, threshold=0, connectivity=1, fill_holes=0):
        p = L.CSSegmentParams()
        p.threshold_mode, p.threshold, p.connectivity, p.fill_holes = mode, threshold, connectivity, fill_holes
        return C.pointer(p)

    def split(depth=16, contrast=0, r0=0, r1=0):
        p = L.CSSplitIntensityParams()
        p.depth, p.min_contrast, p.reserved[0], p.reserved[1] = depth, contrast, r0, r1
        return C.pointer(p)

    base = dict(p=None, image=img.ctypes.data, pt=1, C=1, ch=0, B=1, H=H, W=W, kind=0, par=None, sp=split(), guide=img.ctypes.data, gpt=1,
                gC=1, gch=0, lab=labels.ctypes.data, lkind=0, n=n.ctypes.data, thr=thr.ctypes.data, hq=hq.ctypes.data)

    def call(**kw):
        a = dict(base, **kw)
        return lib.cs_segment_split_intensity(a["p"], a["image"], a["pt"], a["C"], a["ch"], a["B"], a["H"], a["W"], a["kind"], a["par"],
                                              a["sp"], a["guide"], a["gpt"], a["gC"], a["gch"], a["lab"], a["lkind"], a["n"], a["thr"],
                                              a["hq"])

    invalid = [dict(pt=2), dict(ch=1), dict(ch=-1), dict(C=0), dict(B=0), dict(H=0), dict(W=0), dict(kind=2), dict(lkind=2),
               dict(image=None), dict(lab=None), dict(n=None),
               dict(par=params(connectivity=0)), dict(par=params(connectivity=3)), dict(par=params(mode=2)),
               dict(par=params(mode=1, threshold=-1)), dict(par=params(mode=1, threshold=65536)), dict(par=params(fill_holes=2)),
               dict(sp=None), dict(guide=None),
               dict(sp=split(0)), dict(sp=split(255)), dict(sp=split(-1)), dict(sp=split(16, -1)), dict(sp=split(16, 65536)),
               dict(sp=split(16, 0, 1, 0)), dict(sp=split(16, 0, 0, 7)),
               dict(gpt=2), dict(gpt=-1), dict(gC=0), dict(gch=1), dict(gch=-1), dict(gC=3, gch=3)]
    for kw in invalid:
        assert call(**kw) == -1, kw                             # CS_ERR_INVALID
    assert call(sp=split(0)) == -1 and b"1..254" in lib.cs_last_error()
    assert call(sp=split(16, 65536)) == -1 and b"0..65535" in lib.cs_last_error()
    assert call(W=4097) == -6 and call(H=5000) == -6            # CS_ERR_UNSUPPORTED
    no_dev = lib.cs_device_count() <= 0
    for kw in (dict(), dict(thr=None), dict(hq=None), dict(sp=split(1)), dict(sp=split(254, 65535)), dict(gpt=0),
               dict(par=params(mode=1, threshold=65535, connectivity=2, fill_holes=1), sp=split(8, 100))):
        assert call(**kw) == (-4 if no_dev else -1), kw         # no handle: no device here, else a NULL handle
    assert lib.cs_segment_split_intensity_last_timing(None, None, None, None, None) == -1
    assert lib.cs_segment_split_last_syncs(None, None, None) == -1
    assert not labels.any() and not hq.any() and n[0] == 0
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            S.ThresholdSegmenter(0, split_touching=True, split_by="intensity").segment_batch(img)
        assert ei.value.status == -4
