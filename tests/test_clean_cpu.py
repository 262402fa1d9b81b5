"""CPU tests of the segmenter's mask cleanup (cs_segment_clean, ThresholdSegmenter(open_radius=..., min_area=...)): the
restatement of tests/clean_reference.py against SciPy's recorded answers (tests/golden/golden_clean.npz) and against SciPy
itself, the properties of the two steps on inputs that cannot satisfy them vacuously, the speckled field that the option exists
for, and the wrapper's and the C ABI's refusals before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

import clean_reference as CR
import local_reference as LR
import segment_reference as R
from cellscreen import _lib as L
from cellscreen import segment as S
from test_local_cpu import SCENE_DELTA, SCENE_R, dim_cell_scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_clean.npz")
SHAPES = [(1, 1), (1, 9), (9, 1), (37, 53), (17, 65), (40, 70)]
RK = [(r, k) for r in (1, 2, 3, 7, 8, 15) for k in (1, 2)]


def disk_field(shape=(180, 180), radius=24):
    """Three by three disks of `radius` (centres at 30, 90, 150), joined by bridges 1 and 2 pixels thick, over noise of density
    0.1: what an opening of any radius up to 15 changes (speckle and bridges go) but does not empty (a disk of radius 24 holds
    the square of side 31, whose corners are 21.2 from its centre)."""
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    pitch = 2 * radius + 12
    cy, cx = yy // pitch * pitch + pitch // 2, xx // pitch * pitch + pitch // 2
    m = (yy - cy) ** 2 + (xx - cx) ** 2 <= radius * radius
    m |= yy % pitch == pitch // 2
    m |= (xx % pitch == pitch // 2) | (xx % pitch == pitch // 2 + 1)
    m |= np.random.default_rng(7).random(shape) < 0.1
    return m.astype(np.uint8)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_golden_on_every_pixel():
    g = np.load(GOLDEN)
    assert "scipy 1.15.3" in list(g["versions"])
    radii, areas = [int(v) for v in g["radii"]], [int(v) for v in g["areas"]]
    assert radii == [1, 2, 3, 7] and areas == [1, 2, 5, 64] and int(g["n"]) == 8 * len(SHAPES)
    shapes, changed = set(), set()
    for i in range(int(g["n"])):
        shape = tuple(int(v) for v in g[f"shape_{i}"])
        shapes.add(shape)
        unpack = lambda a: np.unpackbits(a)[:shape[0] * shape[1]].reshape(shape)
        x = unpack(g[f"x_{i}"])
        for k in (1, 2):
            for r in radii:
                want = unpack(g[f"o_{r}_{k}_{i}"])
                assert np.array_equal(CR.opening(x, r, k), want), (i, r, k)
                if want.any() and not np.array_equal(want, x):
                    changed.add(("o", r, k))
        for c in (1, 2):
            for a in areas:
                want = unpack(g[f"d_{a}_{c}_{i}"])
                assert np.array_equal(CR.drop_small(x, a, c), want), (i, a, c)
                if want.any() and not np.array_equal(want, x):
                    changed.add(("d", a, c))
    assert shapes == set(SHAPES)
    assert changed == {("o", r, k) for r in radii for k in (1, 2)} | {("d", a, c) for a in areas[1:] for c in (1, 2)}


def test_restatement_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    masks = [m for shape in SHAPES for _, m in CR.mask_inputs(shape, seed=1)] + [disk_field()]
    for x in masks:
        for r, k in RK:
            st = ndimage.generate_binary_structure(2, k)
            want = ndimage.binary_opening(x, st, iterations=r)
            assert np.array_equal(CR.opening(x, r, k), want), (x.shape, r, k)
            if r in (2, 7):
                assert np.array_equal(want, ndimage.binary_opening(x, ndimage.iterate_structure(st, r))), (x.shape, r, k)
        for c in (1, 2):
            lab, _ = ndimage.label(x, structure=ndimage.generate_binary_structure(2, c))
            sizes = np.bincount(lab.ravel())
            for a in (1, 2, 5, 64, 200, 1 << 24):
                keep = sizes >= a
                keep[0] = False
                assert np.array_equal(CR.drop_small(x, a, c), keep[lab]), (x.shape, a, c)


# ---- properties -----------------------------------------------------------------------------------------------------------------
def test_opening_changes_without_emptying_and_is_idempotent_and_anti_extensive():
    x = disk_field()
    for r, k in RK:
        o = CR.opening(x, r, k)
        assert o.any() and not np.array_equal(o, x), (r, k)          # neither empty nor the input
        assert not (o & ~x & 1).any(), (r, k)                         # anti-extensive: nothing new
        assert np.array_equal(CR.opening(o, r, k), o), (r, k)         # idempotent
        lab = R.label_mask(o, 1)[0]
        assert lab[30, 30] > 0 and lab[30, 90] > 0 and lab[90, 30] > 0, (r, k)       # the disks' centres stay
        assert lab[30, 30] != lab[30, 90] and lab[30, 30] != lab[90, 30], (r, k)     # the bridges between them are cut
    lab = R.label_mask(x, 1)[0]
    assert lab[30, 30] == lab[30, 90] == lab[90, 30] > 0              # which held the field together
    assert CR.opening(x, 1, 2).sum() < CR.opening(x, 1, 1).sum()      # the square takes more than the cross


def test_all_foreground_and_the_image_border():
    full = np.ones((40, 50), np.uint8)
    for r in (1, 7, 15):
        assert CR.opening(full, r, 2).all()                           # the border erodes r pixels and the square grows them back
        o = CR.opening(full, r, 1)
        assert o.sum() == full.size - 4 * (r * (r + 1) // 2), r       # the diamond rounds the image's four corners
        assert not o[0, 0] and o[0, r] and o[r, 0]
    assert not CR.opening(np.ones((9, 50), np.uint8), 5, 2).any()     # 9 rows do not survive 5 erosions from both borders
    # foreground touching the border erodes from the border: a bar of 3 rows along the top edge is 3 thick, not endless
    bar = np.zeros((20, 30), np.uint8)
    bar[0:3] = 1
    assert np.array_equal(CR.opening(bar, 1, 2), bar) and not CR.opening(bar, 2, 2).any()
    assert np.array_equal(CR.erode(bar, 2)[:, 5], np.r_[0, 1, np.zeros(18, int)].astype(bool))       # row 0 goes: outside is 0
    inner = np.zeros((20, 30), np.uint8)
    inner[5:8] = 1
    assert np.array_equal(CR.erode(inner, 2)[:, 5], np.r_[np.zeros(6, int), 1, np.zeros(13, int)].astype(bool))     # as inside


def test_min_area_counts_are_exact():
    masks = [m for shape in SHAPES for _, m in CR.mask_inputs(shape)] + [disk_field()]
    for x in masks:
        for c in (1, 2):
            assert np.array_equal(CR.drop_small(x, 1, c), x), (x.shape, c)      # min_area = 1 is the identity
    for a in (2, 5, 64, 200):
        x = np.zeros((30, 260), np.uint8)
        x[3, 2:2 + a - 1] = 1                                         # a - 1 pixels: goes
        x[9, 2:2 + a] = 1                                             # a pixels: stays
        x[15:17, 2:2 + a] = 1                                         # 2a pixels: stays
        got = CR.drop_small(x, a)
        assert not got[3].any() and np.array_equal(got[9], x[9]) and np.array_equal(got[15:17], x[15:17]), a
        assert int(got.sum()) == 3 * a
    assert not CR.drop_small(np.ones((40, 50), np.uint8), 2001).any() and CR.drop_small(np.ones((40, 50), np.uint8), 2000).all()


def test_a_diagonal_chain_is_one_component_under_connectivity_2_only():
    n = 9
    x = np.eye(n, dtype=np.uint8)
    assert R.label_mask(x, 2)[1] == 1 and R.label_mask(x, 1)[1] == n
    assert np.array_equal(CR.drop_small(x, n, 2), x) and not CR.drop_small(x, n + 1, 2).any()
    assert np.array_equal(CR.drop_small(x, 1, 1), x) and not CR.drop_small(x, 2, 1).any()


def test_clean_applies_the_opening_first():
    x = disk_field()
    assert np.array_equal(CR.clean(x, 2, 2, 50, 1), CR.drop_small(CR.opening(x, 2, 2), 50, 1))
    assert np.array_equal(CR.clean(x, None, 2, 50, 2), CR.drop_small(x, 50, 2))
    assert np.array_equal(CR.clean(x, 3, 1, None), CR.opening(x, 3, 1))
    assert np.array_equal(CR.clean(x * 7), x)                         # anything non-zero is foreground; nothing to do
    assert R.label_mask(CR.clean(x, 2, 2, 50), 1)[1] == 9             # the nine disks, apart and alone
    # the order matters: two squares of 49 pixels on a one-pixel bridge are 100 pixels together and 49 each once opened
    pair = np.zeros((12, 24), np.uint8)
    pair[2:9, 2:9] = pair[2:9, 12:19] = 1
    pair[5, 9:12] = 1
    assert int(pair.sum()) == 101 and not CR.clean(pair, 1, 2, 50).any()
    assert int(CR.opening(CR.drop_small(pair, 50), 1, 2).sum()) == 98


# ---- the field the option exists for -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_speckle_of_the_local_threshold_leaves_before_the_labels(seed):
    img, cells = dim_cell_scene(seed)
    assert len(cells) == 40
    mask = R.ndimage.binary_fill_holes(LR.local_mask(img, SCENE_R, SCENE_DELTA) > 0).astype(np.uint8)
    assert R.label_mask(mask, 1)[1] > 800                             # each cell travels with some twenty junk regions
    for kw in (dict(a=50), dict(r=1, k=2)):
        cleaned = CR.clean(mask, **kw)
        assert R.label_mask(cleaned, 1)[1] == 40, kw
        assert all(cleaned[y, x] for y, x, _, _ in cells), kw         # every painted cell is still there


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------
def test_clean_params_refuses_every_bad_value():
    for kw, exc in ((dict(open_radius=0), ValueError), (dict(open_radius=16), ValueError), (dict(open_radius=-1), ValueError),
                    (dict(open_radius=True), TypeError), (dict(open_radius=2.0), TypeError), (dict(open_radius="2"), TypeError),
                    (dict(open_radius=2, open_connectivity=0), ValueError), (dict(open_radius=2, open_connectivity=3), ValueError),
                    (dict(open_connectivity=3), ValueError), (dict(open_connectivity=True), TypeError),
                    (dict(open_connectivity=None), TypeError), (dict(open_connectivity=1.0), TypeError),
                    (dict(min_area=0), ValueError), (dict(min_area=(1 << 24) + 1), ValueError), (dict(min_area=-5), ValueError),
                    (dict(min_area=False), TypeError), (dict(min_area=50.0), TypeError), (dict(min_area="50"), TypeError)):
        with pytest.raises(exc):
            S.clean_params(**kw)
        with pytest.raises(exc):
            S.ThresholdSegmenter(0, **kw)
        if "min_area" in kw:
            kw = dict(mask_min_area=kw["min_area"])                   # min_area is the extraction's own rule there
        with pytest.raises(exc):
            S.threshold_cell_extractor(0, **kw)
    assert S.clean_params() is None and S.clean_params(open_connectivity=1) is None       # a default alone asks for nothing
    p = S.clean_params(np.int64(15), np.int32(1), 1 << 24)
    assert (p.open_radius, p.open_connectivity, p.min_area) == (15, 1, 1 << 24) and C.sizeof(L.CSCleanParams) == 12
    p = S.clean_params(min_area=1)
    assert (p.open_radius, p.open_connectivity, p.min_area) == (0, 2, 1)
    p = S.clean_params(open_radius=1)
    assert (p.open_radius, p.open_connectivity, p.min_area) == (1, 2, 0)
    S.threshold_cell_extractor(0, open_radius=2, open_connectivity=1, mask_min_area=50, min_area=100)     # both areas, apart


def test_segmenter_modes_and_refusals_before_a_handle_exists():
    plain = S.ThresholdSegmenter(0)
    assert plain._clean is None and plain.open_radius is None and plain.min_area is None and plain.open_connectivity == 2
    s = S.ThresholdSegmenter(0, threshold=500, connectivity=2, fill_holes=True, open_radius=3, open_connectivity=1, min_area=50)
    assert (s._clean.open_radius, s._clean.open_connectivity, s._clean.min_area) == (3, 1, 50)
    assert (s.open_radius, s.open_connectivity, s.min_area) == (3, 1, 50)
    # the cleanup's mask is the segmenter's own; what labels the cleaned plane cuts at 0 and fills nothing a second time
    assert (s._params.threshold_mode, s._params.threshold, s._params.connectivity, s._params.fill_holes) == (L.THRESH_FIXED, 500, 2, 1)
    a = s._after_clean
    assert (a.threshold_mode, a.threshold, a.connectivity, a.fill_holes) == (L.THRESH_FIXED, 0, 2, 0)
    s = S.ThresholdSegmenter(0, threshold="local", local_radius=25, min_area=50, split_touching=True, background_radius=40)
    assert s._local is not None and s._split is not None and s._background is not None and s._clean.min_area == 50
    img = np.zeros((1, 16, 16, 3), np.uint16)
    for im, ch, exc in ((img.astype(np.float32), None, TypeError), (img[..., :2].copy(), None, ValueError), (img, 3, ValueError),
                        (img[:, :, :8], None, ValueError), (np.zeros((1, 2, 4097), np.uint8), None, ValueError)):
        with pytest.raises(exc):
            s.clean_mask_batch(im, channel=ch)
        with pytest.raises(exc):
            s.segment_batch(im, channel=ch)
    with pytest.raises(ValueError):
        plain.clean_mask_batch(img)                                   # no step set: no cleaned mask
    with pytest.raises(ValueError):
        S.ThresholdSegmenter(0, open_connectivity=1).clean_mask_batch(img)
    assert s._pre is None and plain._pre is None


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2
    raw = C.CDLL(L.LIB_PATH)
    assert hasattr(raw, "cs_segment_clean") and hasattr(raw, "cs_segment_clean_last_timing")
    assert "cs_segment_clean" in L.SIGNATURES and "cs_segment_clean_last_timing" in L.SIGNATURES


def test_c_abi_refuses_and_reports_no_device():
    lib = L.load_library()
    img = np.zeros((1, 32, 32, 3), np.uint16)
    out = np.full((1, 32, 32), 7, np.uint8)
    thr = np.full(1, 7, np.int32)

    def seg(mode=L.THRESH_OTSU, threshold=0, connectivity=1, fill_holes=1):
        p = L.CSSegmentParams()
        p.threshold_mode, p.threshold, p.connectivity, p.fill_holes = mode, threshold, connectivity, fill_holes
        return C.pointer(p)

    def clean(open_radius=1, open_connectivity=2, min_area=50):
        p = L.CSCleanParams()
        p.open_radius, p.open_connectivity, p.min_area = open_radius, open_connectivity, min_area
        return C.pointer(p)

    base = dict(p=None, image=img.ctypes.data, pt=1, C=3, ch=2, B=1, H=32, W=32, kind=0, par=seg(), cl=clean(), out=out.ctypes.data,
                okind=0, thr=thr.ctypes.data)

    def call(**kw):
        a = dict(base, **kw)
        return lib.cs_segment_clean(a["p"], a["image"], a["pt"], a["C"], a["ch"], a["B"], a["H"], a["W"], a["kind"], a["par"], a["cl"],
                                    a["out"], a["okind"], a["thr"])

    invalid = [dict(cl=None), dict(cl=clean(0, 2, 0)), dict(cl=clean(0, 1, 0)), dict(cl=clean(16)), dict(cl=clean(-1)),
               dict(cl=clean(1, 0)), dict(cl=clean(1, 3)), dict(cl=clean(0, 3, 50)), dict(cl=clean(1, 2, -1)),
               dict(cl=clean(1, 2, (1 << 24) + 1)), dict(par=seg(mode=2)), dict(par=seg(L.THRESH_FIXED, 65536)),
               dict(par=seg(connectivity=3)), dict(par=seg(fill_holes=2)), dict(ch=3), dict(ch=-1), dict(C=0), dict(pt=2), dict(B=0),
               dict(H=0), dict(W=0), dict(kind=2), dict(okind=2), dict(image=None), dict(out=None)]
    for kw in invalid:
        assert call(**kw) == -1, kw                               # CS_ERR_INVALID
    assert call(W=4097) == -6 and call(H=5000) == -6              # CS_ERR_UNSUPPORTED, as its neighbours
    assert b"4096" in lib.cs_last_error()
    assert call(B=65536) == -6
    no_dev = lib.cs_device_count() <= 0
    for kw in (dict(), dict(par=None), dict(thr=None), dict(cl=clean(15, 1, 0)), dict(cl=clean(0, 2, 1 << 24)), dict(okind=1),
               dict(par=seg(L.THRESH_FIXED, 65535, 2, 0))):
        assert call(**kw) == (-4 if no_dev else -1), kw           # no handle: no device here, else a NULL handle
    assert lib.cs_segment_clean_last_timing(None, None, None, None) == -1
    assert (out == 7).all() and (thr == 7).all()
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            S.ThresholdSegmenter(0, min_area=50).clean_mask_batch(img)
        assert ei.value.status == -4
        with pytest.raises(L.CellScreenError) as ei:
            S.ThresholdSegmenter(0, open_radius=1).segment_batch(img)
        assert ei.value.status == -4
