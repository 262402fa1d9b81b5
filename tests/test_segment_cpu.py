"""CPU tests of the built-in segmenter (cellscreen/segment.py, csrc/segment.hip): the restatement of
tests/segment_reference.py against tests/golden/golden_segment.npz (scikit-image 0.18.3 + SciPy 1.7.1), the numbering rule of
the labels, and the wrapper's and the C ABI's refusals before any device work; for all eight cs_segment_* entry points, the
recorded status and text of every refusal (tests/golden/segment_arg_errors.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import segment_arg_cases as AC
import segment_reference as R
from cellscreen import _lib as L
from cellscreen import segment as S
from cellscreen import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_segment.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_restatement_equals_the_libraries_bit_for_bit(golden):
    n = int(golden["n"])
    assert n >= 10 and golden["versions"][0] == "scikit-image 0.18.3"
    kinds = set()
    for i in range(n):
        img = golden[f"image_{i}"]
        assert img.dtype in (np.uint8, np.uint16) and max(img.shape) <= 128
        kinds.add(img.dtype.name)
        t = R.otsu(img)
        assert t == int(golden[f"thr_{i}"]), i
        assert np.array_equal(R.mask_of(img, t, True), golden[f"fill_{i}"]), i
        for c in (1, 2):
            lab, cnt = R.label_mask(img > t, c)
            assert lab.dtype == np.int32 and np.array_equal(lab, golden[f"lab{c}_{i}"]) and cnt == golden[f"lab{c}_{i}"].max(), (i, c)
            lab, cnt, t2 = R.segment(img, "otsu", c, True)
            assert t2 == t and np.array_equal(lab, golden[f"flab{c}_{i}"]), (i, c)
    assert kinds == {"uint8", "uint16"}
    # the set is not trivial: holes that get filled, components that only 8-connectivity joins, a constant image
    assert any((golden[f"fill_{i}"] != (golden[f"image_{i}"] > golden[f"thr_{i}"])).any() for i in range(n))
    assert any(golden[f"lab1_{i}"].max() > golden[f"lab2_{i}"].max() for i in range(n))
    assert any(golden[f"lab1_{i}"].max() == 0 for i in range(n))


def test_constant_image_gives_its_value_and_no_labels():
    for dt, v in ((np.uint8, 0), (np.uint8, 255), (np.uint16, 65535), (np.uint16, 1234)):
        img = np.full((9, 13), v, dt)
        lab, n, t = R.segment(img)
        assert t == v and n == 0 and not lab.any()


def test_label_ids_ascend_with_the_minimum_linear_index(golden):
    rng = np.random.default_rng(5)
    masks = [rng.random((61, 47)) < d for d in (0.3, 0.5, 0.593)]
    masks += [golden[f"image_{i}"] > golden[f"thr_{i}"] for i in range(int(golden["n"]))]
    for m in masks:
        for c in (1, 2):
            lab, n = R.label_mask(m, c)
            first = R.first_pixels(lab)
            assert len(first) == n and np.all(np.diff(first) > 0)
            assert np.array_equal(np.unique(lab), np.arange(0 if (lab == 0).any() else 1, n + 1))


def test_synthetic_label_images_segment_into_cells():
    """Otsu + 4-connectivity (no hole filling) on synth.label_images(7, 2): 10 components per image, 9 and 10 of them with
    area >= 200, so the end-to-end comparisons of tests/test_gpu_segment.py are not over an empty set.  Two filled
    pixels join two of the first image's components."""
    imgs, _ = synth.label_images(7, 2)
    assert list(R.segment_batch(imgs, connectivity=1, fill_holes=True)[1]) == [9, 10]
    labs, n, thr = R.segment_batch(imgs, connectivity=1, fill_holes=False)
    assert list(n) == [10, 10]
    big = [int((np.bincount(labs[b].ravel())[1:] >= 200).sum()) for b in range(2)]
    assert big == [9, 10]
    assert np.all(thr > 0.05 * 65535) and np.all(thr < 0.7 * 65535)


def test_wrapper_refuses_bad_arguments_before_device_work():
    for kw in (dict(connectivity=0), dict(connectivity=3), dict(threshold=-1), dict(threshold=65536), dict(threshold="li")):
        with pytest.raises(ValueError):
            S.ThresholdSegmenter(0, **kw)
        with pytest.raises(ValueError):
            S.threshold_cell_extractor(0, **kw)
    with pytest.raises(TypeError):
        S.ThresholdSegmenter(0, threshold=0.5)
    with pytest.raises(ValueError):
        S.threshold_cell_extractor(0, out_hw=(4, 64))
    with pytest.raises(ValueError):
        S.threshold_cell_extractor(0, min_areas=3)
    s = S.ThresholdSegmenter(0)                                # creates no handle: the first call does, after its checks
    imgs, _ = synth.label_images(1, 1, hw=(96, 96), n_cells=3)
    bad = [
        (imgs.astype(np.float32), None, TypeError),                           # wrong dtype
        (imgs.astype(np.int32), None, TypeError),
        (list(imgs), None, TypeError),
        (imgs[:, :, :48], None, ValueError),                                  # non-contiguous
        (imgs[..., 1], None, ValueError),                                     # non-contiguous channel view
        (imgs[..., :2].copy(), None, ValueError),                             # 2 channels: channel ambiguous
        (imgs, 3, ValueError), (imgs, -1, ValueError),                        # channel out of range
        (imgs[0, 0, 0], None, ValueError),                                    # not a stack
        (np.zeros((1, 0, 8), np.uint8), None, ValueError),                    # H = 0
        (np.zeros((1, 2, 4097), np.uint8), None, ValueError),                 # W = 4097
        (np.zeros((0, 8, 8), np.uint8), None, ValueError),
    ]
    for im, ch, exc in bad:
        with pytest.raises(exc):
            s.segment_batch(im, channel=ch)
    assert s._pre is None
    try:
        import torch
    except ImportError:
        return
    with pytest.raises(ValueError):
        s.segment_batch(torch.from_numpy(imgs.view(np.int16)))               # a CPU tensor
    with pytest.raises(TypeError):
        s.segment_batch(torch.zeros((1, 8, 8), dtype=torch.float32))
    assert s._pre is None


def test_c_abi_refuses_and_reports_no_device():
    lib = L.load_library()
    imgs, _ = synth.label_images(1, 1, hw=(96, 96), n_cells=3)
    labels = np.zeros((1, 96, 96), np.int32)
    n, thr = np.zeros(1, np.int32), np.zeros(1, np.int32)

    def params(mode=0, threshold=0, connectivity=1, fill_holes=0):
        p = L.CSSegmentParams()
        p.threshold_mode, p.threshold, p.connectivity, p.fill_holes = mode, threshold, connectivity, fill_holes
        return C.pointer(p)

    base = dict(p=None, image=imgs.ctypes.data, pt=1, C=3, ch=2, B=1, H=96, W=96, kind=0, par=None, lab=labels.ctypes.data, lkind=0,
                n=n.ctypes.data, thr=thr.ctypes.data)

    def call(**kw):
        a = dict(base, **kw)
        return lib.cs_segment_threshold(a["p"], a["image"], a["pt"], a["C"], a["ch"], a["B"], a["H"], a["W"], a["kind"], a["par"],
                                        a["lab"], a["lkind"], a["n"], a["thr"])

    invalid = [dict(pt=2), dict(ch=3), dict(ch=-1), dict(C=0), dict(B=0), dict(H=0), dict(W=0), dict(kind=2), dict(lkind=2),
               dict(image=None), dict(lab=None), dict(n=None),
               dict(par=params(connectivity=0)), dict(par=params(connectivity=3)), dict(par=params(mode=2)),
               dict(par=params(mode=1, threshold=-1)), dict(par=params(mode=1, threshold=65536)), dict(par=params(fill_holes=2))]
    for kw in invalid:
        assert call(**kw) == -1, kw                             # CS_ERR_INVALID
    assert call(W=4097) == -6 and call(H=5000) == -6            # CS_ERR_UNSUPPORTED, as cs_extract_measure
    assert b"4096" in lib.cs_last_error()
    no_dev = lib.cs_device_count() <= 0
    for kw in (dict(), dict(thr=None), dict(par=params(mode=1, threshold=65535, connectivity=2, fill_holes=1)),
               dict(par=params(mode=0, threshold=-7))):         # OTSU ignores the threshold field
        assert call(**kw) == (-4 if no_dev else -1), kw         # no handle: no device here, else a NULL handle
    assert lib.cs_segment_last_timing(None, None, None) == -1
    assert C.sizeof(L.CSSegmentParams) == 16
    assert not labels.any() and n[0] == 0
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            S.ThresholdSegmenter(0).segment_batch(imgs)
        assert ei.value.status == -4


def test_every_entry_point_refuses_with_the_recorded_status_and_text():
    """tools/make_golden_segment_arg_errors.py: one or two argument rules broken per call, a NULL handle; which rule answers,
    with which status and in which words, is the ABI's and stays."""
    with open(os.path.join(os.path.dirname(GOLDEN), "segment_arg_errors.json")) as f:
        recorded = json.load(f)
    cases = AC.cases()
    assert sorted(recorded) == sorted(AC.ENTRIES) and len(AC.ENTRIES) == 8
    assert [(e, name) for e, name, _ in cases] == [(e, row[0]) for e, rows in recorded.items() for row in rows]
    want = {(e, row[0]): (row[1], row[2]) for e, rows in recorded.items() for row in rows}
    assert len(want) == len(cases) >= 600 and {s for s, _ in want.values()} == {-1, -6}
    lib = L.load_library()
    for entry, name, over in cases:
        assert AC.call(lib, entry, over) == want[entry, name], (entry, name)
