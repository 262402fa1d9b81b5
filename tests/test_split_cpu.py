"""CPU tests of the segmenter's split_touching option (cs_segment_split): the restatement of
tests/split_reference.py against tests/golden/golden_split.npz (SciPy's distance transform, scikit-image 0.18.3's
reconstruction and local maxima), the properties the definition promises, the ten-disk scene the option was specified on, and the
wrapper's and the C ABI's refusals before any device work."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import ndimage

import segment_reference as R
import split_reference as SR
from cellscreen import _lib as L
from cellscreen import segment as S
from cellscreen import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_split.npz")
DISKS = [(60, 60, 20), (60, 95, 20), (150, 60, 30), (150, 98, 10), (100, 200, 25), (60, 250, 6), (60, 262, 7), (150, 250, 15),
         (165, 270, 15), (140, 275, 15)]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_restatement_equals_the_libraries_and_the_recorded_labels(golden):
    n = int(golden["n"])
    assert n >= 10 and golden["versions"][0] == "scikit-image 0.18.3"
    split_somewhere = False
    for i in range(n):
        m = golden[f"mask_{i}"]
        assert m.dtype == bool and max(m.shape) <= 128
        Dq, d2 = SR.dq(m)
        assert Dq.dtype == np.uint8 and np.array_equal(Dq, golden[f"dq_{i}"]), i
        assert np.array_equal(np.minimum(d2, 2 ** 30), golden[f"d2_{i}"]), i
        for c in (1, 2):
            for h in (1, 3, 8):
                r = SR.reconstruct(Dq, h, c)
                assert np.array_equal(r, golden[f"r_{c}_{h}_{i}"]), (i, c, h)
                s, ns = SR.seeds(r, m, c)
                assert np.array_equal(s > 0, golden[f"seed_{c}_{h}_{i}"]), (i, c, h)
                assert ns == ndimage.label(s > 0, structure=R.STRUCTURES[c])[1]
                lab, cnt, dq2 = SR.split_mask(m, c, h)
                assert lab.dtype == np.int32 and np.array_equal(lab, golden[f"lab_{c}_{h}_{i}"]) and cnt == ns, (i, c, h)
                assert np.array_equal(dq2, Dq)
                split_somewhere |= cnt > R.label_mask(m, c)[1]
    assert split_somewhere


def test_squared_distance_is_exact_by_brute_force():
    rng = np.random.default_rng(11)
    for shape, p in (((23, 31), 0.9), ((40, 17), 0.97), ((1, 40), 0.8), ((30, 1), 0.8)):
        m = rng.random(shape) < p
        m[rng.integers(shape[0]), rng.integers(shape[1])] = False
        by, bx = np.nonzero(~m)
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        d2 = ((yy[..., None] - by) ** 2 + (xx[..., None] - bx) ** 2).min(axis=-1)
        Dq, got = SR.dq(m)
        assert np.array_equal(got, d2)
        assert np.array_equal(Dq, [[min(int(np.floor(np.sqrt(4.0 * v) + 1e-9)), 255) for v in row] for row in d2])
    assert SR.dq(np.ones((5, 7), bool))[0].min() == 255 and SR.dq(np.zeros((5, 7), bool))[0].max() == 0
    deep = np.ones((300, 300), bool)
    deep[0, 0] = False
    assert SR.dq(deep)[0][200, 200] == 255 and SR.dq(deep)[0][0, 127] == 254 and SR.dq(deep)[0][0, 128] == 255


def test_ten_disk_scene_splits_into_its_disks():
    """conn 1, h 3: exactly 10 regions from 5 components, with the areas the option's specification records (1226 1226 148 112 1961
    2833 628 573 792 294 in label order); h 2 over-splits the triple (11), h 4 under-splits it (8).

    Area bound, recomputed from the restatement when this test was written.  "Owned" is a disk's pixel count minus half of
    each overlap with another disk; region / owned in disk order is
        1.000 1.000 1.006 0.944 1.000 1.000 1.000 | 0.860 1.207 0.936.
    The seven disks that stand alone or in a pair are within the specified 6 % (worst 0.944, the R = 10 disk beside the R = 30
    one, the 0.94 the specification names).  The three disks of the triple are not, and cannot be under this definition: the specification's
    own table gives them 628, 573 and 792 pixels against 707-pixel disks, because the watershed line between three mutually
    overlapping disks follows the distance map's ridges, not the chords.  For them the test pins the exact areas (stricter
    than any ratio) and that the three regions together are the triple's component; the 6 % is asserted for the other seven."""
    mask, each = SR.ten_disks()
    assert R.label_mask(mask, 1)[1] == 5
    lab, n, _ = SR.split_mask(mask, 1, 3)
    assert n == 10
    assert list(np.bincount(lab.ravel())[1:]) == [1226, 1226, 148, 112, 1961, 2833, 628, 573, 792, 294]
    owned = []
    for i, d in enumerate(each):
        o = float(d.sum())
        for j, e in enumerate(each):
            if j != i:
                o -= 0.5 * float((d & e).sum())
        owned.append(o)
    ratios = []
    for (cy, cx, _), o in zip(DISKS, owned):
        region = int((lab == lab[cy, cx]).sum())
        ratios.append(region / o)
    print("region / owned:", " ".join(f"{r:.3f}" for r in ratios))
    assert len({int(lab[cy, cx]) for cy, cx, _ in DISKS}) == 10
    assert all(abs(r - 1.0) <= 0.06 for r in ratios[:7]), ratios
    triple = sorted(int((lab == lab[cy, cx]).sum()) for cy, cx, _ in DISKS[7:])
    assert triple == [573, 628, 792] and sum(triple) == int((each[7] | each[8] | each[9]).sum())
    assert SR.split_mask(mask, 1, 2)[1] == 11 and SR.split_mask(mask, 1, 4)[1] == 8
    a = np.bincount(SR.split_mask(mask, 2, 3)[0].ravel())
    assert sorted(a[1:3]) == [1132, 1320]                         # connectivity 2 skews the equal pair


def _masks():
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:90, 0:120]
    out = [rng.random((61, 47)) < d for d in (0.4, 0.593, 0.8)]
    m = np.zeros((90, 120), bool)
    for _ in range(14):
        cy, cx, r = rng.uniform(5, 85), rng.uniform(5, 115), rng.uniform(4, 13)
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    out.append(m)
    out.append(SR.ten_disks()[0])
    return out


def test_every_mask_pixel_is_labelled_inside_its_component_and_regions_are_connected():
    for m in _masks():
        for c in (1, 2):
            base, nb = R.label_mask(m, c)
            for h in (1, 3, 8):
                lab, n, Dq = SR.split_mask(m, c, h)
                assert np.array_equal(lab > 0, m) and n >= nb
                assert np.array_equal(np.unique(lab[m]), np.arange(1, n + 1))
                owner = np.zeros(n + 1, np.int64)
                owner[lab[m]] = base[m]
                assert np.array_equal(owner[lab][m], base[m])                      # no region spans two components
                assert R.label_mask(lab > 0, c)[1] == nb
                pieces = sum(ndimage.label(lab == k, structure=R.STRUCTURES[c])[1] for k in range(1, n + 1))
                assert pieces == n                                                  # every region is connected
                first = R.first_pixels(lab)
                assert np.all(np.diff(first) > 0)                                   # numbered by first pixel


def test_identity_with_plain_labelling_where_nothing_splits():
    yy, xx = np.mgrid[0:80, 0:100]
    two = ((yy - 25) ** 2 + (xx - 25) ** 2 <= 15 ** 2) | ((yy - 50) ** 2 + (xx - 70) ** 2 <= 20 ** 2)
    rng = np.random.default_rng(2)
    for m in (two, rng.random((50, 60)) < 0.3, np.ones((9, 9), bool), np.zeros((4, 5), bool)):
        for c in (1, 2):
            lab, n, _ = SR.split_mask(m, c, 3)
            el, en = R.label_mask(m, c)
            if n == en:
                assert np.array_equal(lab, el)
    assert SR.split_mask(two, 1, 3)[1] == 2 and SR.split_mask(np.ones((9, 9), bool), 1, 3)[1] == 1
    imgs, _ = synth.label_images(7, 1)
    lab, n, thr, _ = SR.split_batch(imgs, connectivity=1, fill_holes=False, h=255)    # no saddle is 127 px deep: nothing splits
    el, en, ethr = R.segment_batch(imgs, connectivity=1, fill_holes=False)
    assert np.array_equal(lab, el) and np.array_equal(n, en) and np.array_equal(thr, ethr)


def test_wrapper_refuses_bad_split_arguments_before_device_work():
    for kw in (dict(split_h=0), dict(split_h=256), dict(split_h=-3), dict(split_touching=True, split_h=0)):
        with pytest.raises(ValueError):
            S.ThresholdSegmenter(0, **kw)
        with pytest.raises(ValueError):
            S.threshold_cell_extractor(0, **kw)
    for kw in (dict(split_h=2.5), dict(split_h=True), dict(split_touching=1), dict(split_touching="yes")):
        with pytest.raises(TypeError):
            S.ThresholdSegmenter(0, **kw)
        with pytest.raises(TypeError):
            S.threshold_cell_extractor(0, **kw)
    assert S.split_params(False, 3) is None and S.split_params(True, 5).h == 5 and C.sizeof(L.CSSplitParams) == 4
    imgs, _ = synth.label_images(1, 1, hw=(96, 96), n_cells=3)
    plain = S.ThresholdSegmenter(0)
    with pytest.raises(ValueError):
        plain.segment_batch(imgs, return_distance=True)           # no distances without the split
    s = S.ThresholdSegmenter(0, split_touching=True, split_h=4)
    assert s.split_touching and s.split_h == 4 and not plain.split_touching
    for im, exc in ((imgs.astype(np.float32), TypeError), (imgs[:, :, :48], ValueError), (np.zeros((1, 2, 4097), np.uint8), ValueError)):
        with pytest.raises(exc):
            s.segment_batch(im, return_distance=True)
    assert s._pre is None and plain._pre is None


def test_c_abi_of_the_split_refuses_and_reports_no_device():
    lib = L.load_library()
    imgs, _ = synth.label_images(1, 1, hw=(96, 96), n_cells=3)
    labels = np.zeros((1, 96, 96), np.int32)
    dist = np.zeros((1, 96, 96), np.uint8)
    n, thr = np.zeros(1, np.int32), np.zeros(1, np.int32)

    def params(mode=0, threshold=0, connectivity=1, fill_holes=0):
        p = L.CSSegmentParams()
        p.threshold_mode, p.threshold, p.connectivity, p.fill_holes = mode, threshold, connectivity, fill_holes
        return C.pointer(p)

    def split(h):
        p = L.CSSplitParams()
        p.h = h
        return C.pointer(p)

    base = dict(p=None, image=imgs.ctypes.data, pt=1, C=3, ch=2, B=1, H=96, W=96, kind=0, par=None, sp=None, lab=labels.ctypes.data,
                lkind=0, n=n.ctypes.data, thr=thr.ctypes.data, dist=dist.ctypes.data)

    def call(**kw):
        a = dict(base, **kw)
        return lib.cs_segment_split(a["p"], a["image"], a["pt"], a["C"], a["ch"], a["B"], a["H"], a["W"], a["kind"], a["par"], a["sp"],
                                    a["lab"], a["lkind"], a["n"], a["thr"], a["dist"])

    invalid = [dict(pt=2), dict(ch=3), dict(ch=-1), dict(C=0), dict(B=0), dict(H=0), dict(W=0), dict(kind=2), dict(lkind=2),
               dict(image=None), dict(lab=None), dict(n=None),
               dict(par=params(connectivity=0)), dict(par=params(connectivity=3)), dict(par=params(mode=2)),
               dict(par=params(mode=1, threshold=-1)), dict(par=params(mode=1, threshold=65536)), dict(par=params(fill_holes=2)),
               dict(sp=split(0)), dict(sp=split(256)), dict(sp=split(-1))]
    for kw in invalid:
        assert call(**kw) == -1, kw                             # CS_ERR_INVALID
    assert call(sp=split(0)) == -1 and b"1..255" in lib.cs_last_error()
    assert call(W=4097) == -6 and call(H=5000) == -6            # CS_ERR_UNSUPPORTED
    assert b"4096" in lib.cs_last_error()
    no_dev = lib.cs_device_count() <= 0
    for kw in (dict(), dict(thr=None), dict(dist=None), dict(sp=split(1)), dict(sp=split(255)),
               dict(par=params(mode=1, threshold=65535, connectivity=2, fill_holes=1), sp=split(8))):
        assert call(**kw) == (-4 if no_dev else -1), kw         # no handle: no device here, else a NULL handle
    assert lib.cs_segment_split_last_timing(None, None, None, None, None) == -1
    assert not labels.any() and not dist.any() and n[0] == 0
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            S.ThresholdSegmenter(0, split_touching=True).segment_batch(imgs)
        assert ei.value.status == -4
