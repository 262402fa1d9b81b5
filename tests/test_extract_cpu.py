"""CPU tests of the quality-cell extraction (cellscreen/extract.py, csrc/extract.hip): the restatement of
tests/extract_reference.py on hand-built shapes with closed-form answers, the QC rules one region at a time, the
synthetic label images, and the wrapper's and the C ABI's refusals before any device work."""
import ctypes as C
import math

import numpy as np
import pytest

import extract_reference as R
from cellscreen import _lib as L
from cellscreen import extract as X
from cellscreen import synth


def _one(mask, ana=None):
    lab = mask.astype(np.int32)
    ana = np.full(mask.shape, 1000, np.uint16) if ana is None else ana
    (r,) = R.regions(lab, ana)
    return r


def test_rectangle_area_bbox_eccentricity_solidity():
    m = np.zeros((60, 70), bool)
    m[12:32, 15:55] = True                                     # 20 rows x 40 columns
    r = _one(m)
    assert (r["minr"], r["minc"], r["maxr"], r["maxc"]) == (12, 15, 32, 55) and r["area"] == 800
    # central moments of a filled a x b rectangle: (a^2 - 1)/12 and (b^2 - 1)/12 per pixel, no mixed term
    l1, l2 = (40 ** 2 - 1) / 12, (20 ** 2 - 1) / 12
    assert abs(r["eccentricity"] - math.sqrt(1 - l2 / l1)) <= 1e-15
    assert abs(R.eccentricity_eigvalsh(*np.nonzero(m)) - r["eccentricity"]) <= 1e-12
    assert r["convex_area"] == 800 and r["solidity"] == 1.0
    sq = np.zeros((30, 30), bool)
    sq[10:20, 10:20] = True
    assert _one(sq)["eccentricity"] == 0.0
    line = np.zeros((30, 30), bool)
    line[15, 5:25] = True
    assert _one(line)["eccentricity"] == 1.0


def test_disc_solidity():
    # the digital disc r^2 + c^2 <= 4 (13 pixels): its edge midpoints (-2.5, 0), (-2, 1/2), (-1.5, 1), (-1, 1.5), (-1/2, 2),
    # (0, 2.5) all lie on |r| + |c| = 2.5, so the hull is that diamond and holds exactly the 13 centres with |r| + |c| <= 2
    yy, xx = np.mgrid[0:30, 0:30]
    disc = (yy - 15) ** 2 + (xx - 15) ** 2 <= 4
    r = _one(disc)
    assert r["area"] == 13 and r["convex_area"] == 13 and r["solidity"] == 1.0 and r["eccentricity"] == 0.0
    # a large digital disc is not convex in this sense: the hull takes in centres just outside its staircase rim
    yy, xx = np.mgrid[0:41, 0:41]
    disc = (yy - 20) ** 2 + (xx - 20) ** 2 <= 15 ** 2
    r = _one(disc)
    assert r["area"] == disc.sum() == 709 and 0.95 < r["solidity"] < 1.0 and r["eccentricity"] < 1e-7


def test_convex_area_of_an_l_shape_and_of_two_blobs_by_hand():
    # L: column 0 of rows 0-3 and row 3 of columns 0-3.  The hull of the edge midpoints is bounded by c = r + 1/2 on the
    # upper right, so the centres inside or on it are 0 <= c <= r <= 3: 1 + 2 + 3 + 4 = 10
    L_ = np.zeros((4, 4), bool)
    L_[:, 0] = True
    L_[3, :] = True
    assert R.convex_area(L_) == 10
    # two single pixels on a diagonal, one label: the hull is the band |c - r| <= 1/2 between them -> the 4 diagonal centres
    d = np.zeros((4, 4), bool)
    d[0, 0] = d[3, 3] = True
    assert R.convex_area(d) == 4
    # two 2x2 blobs in one row band: every centre of the 2 x 7 bbox
    two = np.zeros((2, 7), bool)
    two[:, 0:2] = two[:, 5:7] = True
    assert R.convex_area(two) == 14
    assert R.convex_area(np.ones((1, 1), bool)) == 1


def test_each_rule_fails_exactly_its_own_region():
    H = W = 200
    lab = np.zeros((H, W), np.int32)
    rng = np.random.default_rng(0)
    ana = rng.integers(500, 3000, (H, W), dtype=np.uint16)
    lab[40:60, 40:60] = 1                                      # good
    lab[2:22, 100:120] = 2                                     # border
    lab[100:108, 30:38] = 3                                    # area 64 < 200
    lab[150:154, 60:140] = 4                                   # 4 x 80: area 320, eccentricity > 0.95
    lab[100:120, 100:120] = 5                                  # dark: analysis channel 0 over the bbox
    ana[100:120, 100:120] = 0
    lab[100:120, 150:170] = 6                                  # flat: constant over the bbox
    ana[100:120, 150:170] = 777
    lab[30:130, 160:190] = np.where(lab[30:130, 160:190] == 0, 0, lab[30:130, 160:190])
    got = {r["label"]: r["failed"] for r in R.regions(lab, ana)}
    assert got == {1: 0, 2: R.QC_BORDER, 3: R.QC_AREA, 4: R.QC_ECCENTRICITY, 5: R.QC_INTENSITY, 6: R.QC_INTENSITY}
    assert [r["label"] for r in R.regions(lab, ana)] == [1, 2, 3, 4, 5, 6]
    crops, regs, st = R.extract(lab, ana)
    assert st == R.IMAGE_OK and len(crops) == 1 and crops[0].shape == (20, 20)


def test_reference_thresholds_leave_no_narrow_passing_region():
    """Area >= 200 with eccentricity <= 0.95 rules out a bbox side below 8 (the whole-image 'no cells' rule): the thinnest
    passing rectangle of 7 rows would need 200/7 > 28 columns, and a 7 x 29 rectangle is already too eccentric; shapes
    that are not rectangles only spread their second moments further."""
    for h in range(1, 8):
        w = -(-200 // h)
        l1, l2 = (max(h, w) ** 2 - 1) / 12, (min(h, w) ** 2 - 1) / 12
        assert math.sqrt(1 - l2 / l1) > 0.95, (h, w)
    for h in range(8, 12):                                     # and 8 rows do pass: the rule binds exactly below 8
        w = -(-200 // h)
        l1, l2 = (max(h, w) ** 2 - 1) / 12, (min(h, w) ** 2 - 1) / 12
        if math.sqrt(1 - l2 / l1) <= 0.95:
            break
    else:
        pytest.fail("no passing rectangle of 8-11 rows")


def test_mean_and_std_are_numpy_s():
    rng = np.random.default_rng(3)
    for dt in (np.uint8, np.uint16):
        crop = rng.integers(0, np.iinfo(dt).max, (37, 23), dtype=dt)
        mean, std = R.intensity(crop)
        assert mean == np.mean(crop)                             # the reference's np.mean: exact sum, one division
        assert abs(std - np.std(crop)) <= 1e-12 * std


def test_label_images_exercise_every_rule():
    imgs, labs = synth.label_images(5, 2)
    assert imgs.shape == (2, 256, 256, 3) and imgs.dtype == np.uint16 and labs.dtype == np.int32
    for b in range(2):
        ids = np.unique(labs[b])[1:]
        assert not np.array_equal(ids, np.arange(1, len(ids) + 1))          # non-consecutive
        regs = R.regions(labs[b], imgs[b, ..., 1])
        bits = {r["failed"] for r in regs}
        for bit in (R.QC_BORDER, R.QC_AREA, R.QC_ECCENTRICITY, R.QC_INTENSITY):
            assert any(f & bit for f in bits), bit
        from scipy import ndimage
        assert any(ndimage.label(labs[b] == r["label"])[1] >= 2 for r in regs)          # a label of separated blobs
        assert min(r["solidity"] for r in regs) < 0.6
    a, b = synth.label_images(5, 2)
    assert np.array_equal(a, imgs) and np.array_equal(b, labs)


def test_wrapper_refuses_bad_arguments_before_device_work():
    e = X.CellExtractor(0)                                     # creates no handle: the first call does, after its checks
    imgs, labs = synth.label_images(1, 1, hw=(96, 96), n_cells=3)
    bad = [
        (imgs.astype(np.float32), labs, TypeError),
        (imgs.astype(np.int32), labs, TypeError),
        (imgs, labs.astype(np.float64), TypeError),
        (imgs, labs[:, :48], ValueError),
        (imgs[:, :, :48], labs[:, :, :48].copy(), ValueError),                # non-contiguous image
        (imgs[..., :2].copy(), labs, ValueError),                             # 2 channels: channel ambiguous
        (imgs, labs[0], ValueError),
        (imgs, -labs, ValueError),                                            # negative labels
        (list(imgs), labs, TypeError),
    ]
    for im, lb, exc in bad:
        with pytest.raises(exc):
            e.extract_batch(im, lb)
    with pytest.raises(ValueError):
        e.extract_batch(imgs, labs, channel=3)
    with pytest.raises(ValueError):
        X.CellExtractor(0, min_areas=3)
    assert e._pre is None
    with pytest.raises(ValueError):
        X.split_channels(np.zeros((8, 8, 2), np.uint16))
    try:
        import torch
    except ImportError:
        return
    with pytest.raises(TypeError):
        e.extract_batch(torch.from_numpy(imgs.view(np.int16)), labs)                           # mixed kinds
    with pytest.raises(ValueError):
        e.extract_batch(torch.from_numpy(imgs.view(np.int16)), torch.from_numpy(labs))         # CPU tensors
    assert e._pre is None


def test_c_abi_refuses_and_reports_no_device():
    lib = L.load_library()
    imgs, labs = synth.label_images(1, 1, hw=(96, 96), n_cells=3)
    nr, nc = C.c_int64(), C.c_int64()
    args = lambda **kw: dict(dict(p=None, image=imgs.ctypes.data, pt=1, C=3, ch=1, lab=labs.ctypes.data, B=1, H=96, W=96, kind=0,
                                  maxl=int(labs.max()), qc=None), **kw)
    call = lambda a: lib.cs_extract_measure(a["p"], a["image"], a["pt"], a["C"], a["ch"], a["lab"], a["B"], a["H"], a["W"], a["kind"],
                                            a["maxl"], a["qc"], C.byref(nr), C.byref(nc))
    for kw in (dict(pt=2), dict(ch=3), dict(C=0), dict(B=0), dict(kind=2), dict(maxl=-1), dict(image=None)):
        assert call(args(**kw)) == -1, kw                       # CS_ERR_INVALID
    assert call(args(H=5000)) == -6 and call(args(maxl=(1 << 20) + 1)) == -6      # CS_ERR_UNSUPPORTED
    q = X.qc_params()
    q.reserved = 1
    assert call(args(qc=C.pointer(q))) == -1
    rc = call(args())
    assert rc == (-4 if lib.cs_device_count() <= 0 else -1)     # no handle: no device here, else a NULL handle
    assert lib.cs_extract_fill(None, None, None, 0, None, None, 0) == (-4 if lib.cs_device_count() <= 0 else -1)
    assert lib.cs_extract_fill(None, None, None, 3, None, None, 0) == -1
    assert C.sizeof(L.CSQcParams) == 48 and L.REGION_DTYPE.itemsize == 80
    if lib.cs_device_count() <= 0:
        with pytest.raises(L.CellScreenError) as ei:
            X.CellExtractor(0).extract_batch(imgs, labs)
        assert ei.value.status == -4


def test_create_training_dataset_writes_the_reference_csvs(tmp_path):
    import pandas as pd
    from cellscreen.training import ImprovedAnomalyDetectionTraining
    d = tmp_path / "imgs"
    d.mkdir()
    for name in ("b.npy", "a.npy", "c.npy"):
        np.save(d / name, np.zeros((4, 4), np.uint8))
    calls = []

    def fake(path):
        calls.append(path)
        if path.endswith("c.npy"):
            raise RuntimeError("unreadable")
        k = 2 if path.endswith("a.npy") else 1
        return [np.full((64, 64), 0.5 * i) for i in range(k)], [{"area": 300 + i, "eccentricity": 0.5, "solidity": 0.9,
                                                                 "mean_intensity": 10.0 + i, "std_intensity": 2.0} for i in range(k)]

    tr = ImprovedAnomalyDetectionTraining.__new__(ImprovedAnomalyDetectionTraining)
    tr.output_dir = str(tmp_path)
    cells, df = tr.create_training_dataset(str(d), fake, file_pattern="*.npy")
    assert [p.rsplit("/", 1)[1] for p in calls] == ["a.npy", "b.npy", "c.npy"]
    assert cells.shape == (3, 64, 64)
    assert list(df.columns) == ["area", "eccentricity", "solidity", "mean_intensity", "std_intensity", "file"]
    assert list(df["file"]) == ["a.npy", "a.npy", "b.npy"]
    assert pd.read_csv(tmp_path / "cell_statistics.csv").equals(df)
    fs = pd.read_csv(tmp_path / "file_summary.csv")
    assert list(fs.columns) == ["filename", "cells_extracted", "mean_cell_intensity"]
    assert list(fs["cells_extracted"]) == [2, 1, 0] and list(fs["mean_cell_intensity"]) == [10.5, 10.0, 0.0]
