"""CPU tests of the label expansion (cs_label_expand, cellscreen/expand.py): the restatement of
tests/expand_reference.py against skimage.segmentation.expand_labels as recorded in tests/golden/golden_expand.npz (equal off
the ties, the smallest label on them, d2 and support equal everywhere), the distance's integer form, and the wrapper's and the
C ABI's refusals before any device work."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import expand_reference as ER
from cellscreen import _lib as L
from cellscreen import expand as EX
from cellscreen import extract as X
from cellscreen import segment as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_expand.npz")


def golden_cases():
    g = np.load(GOLDEN)
    for i in range(int(g["n_cases"])):
        yield (str(g[f"name_{i}"]), g[f"labels_{i}"], float(g[f"distance_{i}"]), int(g[f"max_d2_{i}"]), g[f"lib_{i}"], g[f"d2_{i}"],
               g[f"tie_{i}"])


# ---- one pixel from the definition: the distance plane of that pixel, no code shared with the restatement ------------------------------
def smallest_nearest_label(lab, y, x):
    yy, xx = np.mgrid[0:lab.shape[0], 0:lab.shape[1]]
    d = np.where(lab > 0, (yy - y) ** 2 + (xx - x) ** 2, np.iinfo(np.int64).max)
    return int(d.min()), int(lab[d == d.min()].min())


def test_restatement_equals_the_library_off_the_ties_and_takes_the_smallest_label_on_them():
    seen_ties, names = 0, set()
    for name, lab, distance, max_d2, lib, d2, tie in golden_cases():
        names.add(name)
        assert lab.dtype == np.int32 and lab.size <= 70 * 300 and max_d2 == ER.max_d2_of(distance)
        got, got_d2 = ER.expand(lab, max_d2)
        assert got.dtype == np.int32 and got_d2.dtype == np.uint16
        assert np.array_equal(got[~tie], lib[~tie]), name
        assert np.array_equal(got_d2, d2), name                          # d2 has no ties: equal everywhere
        assert np.array_equal(got > 0, lib > 0), name                    # and so is the support
        assert np.array_equal(got[lab > 0], lab[lab > 0]) and not tie[lab > 0].any()
        for y, x in zip(*np.nonzero(tie)):
            dist, who = smallest_nearest_label(lab, int(y), int(x))
            assert (int(got_d2[y, x]), int(got[y, x])) == (dist, who), (name, y, x)
            seen_ties += 1
    assert len(names) == 9 and seen_ties > 500


def test_ties_are_few_in_every_golden_case():
    # the condition under which "the library off the ties" is a witness at all, not a measurement
    for name, lab, distance, max_d2, lib, d2, tie in golden_cases():
        grown = (lib > 0) & (lab == 0)
        assert grown.sum() > 300 and not tie[~grown].any()
        assert 20 * int(tie.sum()) <= int(grown.sum()), name             # at most 5 %


def test_restatement_edge_cases():
    z = np.zeros((5, 7), np.int32)
    g, d = ER.expand(z, 25)
    assert not g.any() and (d == ER.FAR).all()
    f = np.arange(1, 36, dtype=np.int32).reshape(5, 7)
    g, d = ER.expand(f, 25)
    assert np.array_equal(g, f) and not d.any()
    row = np.zeros((1, 9), np.int32)
    row[0, 2], row[0, 6] = 5, 3
    g, d = ER.expand(row, 4)
    assert g.tolist() == [[5, 5, 5, 5, 3, 3, 3, 3, 3]] and d.tolist() == [[4, 1, 0, 1, 4, 1, 0, 1, 4]]     # the middle pixel: the tie to 3
    g, d = ER.expand(row, 1)
    assert g.tolist() == [[0, 5, 5, 5, 0, 3, 3, 3, 0]] and d[0, 0] == ER.FAR and d[0, 4] == ER.FAR
    g3, d3 = ER.expand(np.stack([row, np.zeros_like(row), row[:, ::-1]]), 4)                       # a batch: image by image
    assert np.array_equal(g3[0], ER.expand(row, 4)[0]) and not g3[1].any() and g3[2].tolist() == [[3, 3, 3, 3, 3, 5, 5, 5, 5]]
    with pytest.raises(ValueError):
        ER.expand(np.full((2, 2), -1, np.int32), 4)


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------
def test_expand_params_integers_floats_and_every_refusal():
    for d in (1, 2, 5, 12, 127, np.int64(7), np.int32(127)):
        assert EX.expand_params(d).max_d2 == int(d) * int(d) == ER.max_d2_of(d)
    for d, n in ((1.5, 2), (2.9, 8), (127.0, 16129), (1.0, 1), (math.sqrt(2), 2), (np.float32(2.5), 6), (np.float64(3.0), 9),
                 (2.2360679, 4), (2.23606798, 5), (126.99999, 16128)):
        p = EX.expand_params(d)
        assert (p.max_d2, p.reserved) == (n, 0) and ER.max_d2_of(d) == n, d
        assert math.sqrt(n) <= float(d) < math.sqrt(n + 1)               # the library's `distances <= distance`, exactly
    rng = np.random.default_rng(3)
    for d in rng.uniform(1, 127, 2000):
        n = EX.expand_params(float(d)).max_d2
        assert math.sqrt(n) <= d < math.sqrt(n + 1) and n == ER.max_d2_of(float(d))
    assert C.sizeof(L.CSExpandParams) == 8
    for d, exc in ((True, TypeError), (False, TypeError), (np.True_, TypeError), ("5", TypeError), ([5], TypeError),
                   (5 + 0j, TypeError), (float("nan"), ValueError), (float("inf"), ValueError), (-float("inf"), ValueError), (0, ValueError),
                   (0.999, ValueError), (-3, ValueError), (128, ValueError), (127.001, ValueError), (1 << 40, ValueError)):
        with pytest.raises(exc):
            EX.expand_params(d)
        with pytest.raises(exc):                                        # the wiring: refused where it is given, before a handle exists
            S.ThresholdSegmenter(0, expand_distance=d)
        with pytest.raises(exc):
            S.threshold_cell_extractor(expand_distance=d)
        with pytest.raises(exc):
            X.label_cell_extractor(lambda seg: seg, expand_distance=d)
    with pytest.raises(TypeError):
        EX.expand_params(None)                                          # None means "off" only where the argument is optional


def test_expand_distance_is_accepted_and_defaults_to_off():
    import cellscreen
    assert cellscreen.LabelExpander is EX.LabelExpander and cellscreen.expand_params is EX.expand_params
    s = S.ThresholdSegmenter(0)
    assert s.expand_distance is None and s._expand is None and s._pre is None
    s = S.ThresholdSegmenter(0, expand_distance=2.9, split_touching=True)
    assert s.expand_distance == 2.9 and s._expand.max_d2 == 8 and s._pre is None and s._expander._pre is None
    assert callable(S.threshold_cell_extractor(expand_distance=6, min_area=100))
    assert callable(X.label_cell_extractor(lambda seg: seg, expand_distance=6.5, min_area=100))


def test_expander_refusals_before_a_handle_exists():
    import torch
    e = EX.LabelExpander(0)
    a = np.zeros((2, 8, 12), np.int32)
    ro = a.copy()
    ro.flags.writeable = False
    for labels, kw, exc in ((a.astype(np.int64), {}, TypeError), (a.astype(np.uint16), {}, TypeError), (a[:, :, ::2], {}, ValueError),
                            (a.transpose(0, 2, 1), {}, ValueError), (a[0], {}, ValueError), (a[:0], {}, ValueError), (list(a), {}, TypeError),
                            (torch.zeros((2, 8, 12), dtype=torch.int32), {}, ValueError),                        # a CPU tensor
                            (np.zeros((1, 2, 4097), np.int32), {}, ValueError), (np.zeros((1, 4097, 2), np.int32), {}, ValueError),
                            (a, dict(out=a[:1].copy()), ValueError), (a, dict(out=a.astype(np.int64)), TypeError),
                            (a, dict(out=torch.zeros((2, 8, 12), dtype=torch.int32)), ValueError), (a, dict(out=ro), ValueError),
                            (a, dict(out=np.zeros((2, 8, 24), np.int32)[:, :, ::2]), ValueError), (a, dict(return_d2=1), TypeError)):
        with pytest.raises(exc):
            e.expand_batch(labels, 3, **kw)
    for d, exc in ((0, ValueError), (128, ValueError), (True, TypeError), (float("nan"), ValueError)):
        with pytest.raises(exc):
            e.expand_batch(a, d)
    assert e._pre is None
    e.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2
    raw = C.CDLL(L.LIB_PATH)
    for name in ("cs_label_expand", "cs_label_expand_last_timing"):
        assert hasattr(raw, name) and name in L.SIGNATURES


def test_the_struct_and_the_prototypes_are_in_the_header():
    with open(os.path.join(ROOT, "include", "cellscreen.h")) as f:
        text = " ".join(f.read().split())
    assert "typedef struct cs_expand_params { int32_t max_d2; /* 1..16129 */ int32_t reserved; /* 0 */ } cs_expand_params;" in text
    assert ("int cs_label_expand(cs_preproc *p, const int32_t *labels, int32_t batch, int32_t height, int32_t width, int in_kind, "
            "const cs_expand_params *params, int32_t *out, uint16_t *d2 /* or NULL */, int out_kind);") in text
    assert "int cs_label_expand_last_timing(const cs_preproc *p, double *columns_ms, double *rows_ms);" in text
    assert "#define CS_ABI_VERSION 2 " in text


def _call(lib, labels=True, out=True, B=1, H=8, W=8, in_kind=0, out_kind=0, params=(9, 0), d2=False):
    a = np.zeros((max(B, 1), max(H, 1), max(W, 1)), np.int32) if B * H * W <= 1 << 20 else np.zeros(1, np.int32)
    p = None if params is None else L.CSExpandParams(*params)
    d = np.zeros(a.shape, np.uint16)
    rc = lib.cs_label_expand(None, a.ctypes.data if labels else None, B, H, W, in_kind, None if p is None else C.byref(p),
                             a.ctypes.data if out else None, d.ctypes.data if d2 else None, out_kind)
    return rc, lib.cs_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_the_handle():
    lib = L.load_library()
    for over, status in ((dict(labels=False), -1), (dict(out=False), -1), (dict(params=None), -1), (dict(in_kind=2), -1), (dict(out_kind=-1), -1),
                         (dict(B=0), -1), (dict(H=0), -1), (dict(W=-1), -1), (dict(params=(0, 0)), -1), (dict(params=(16130, 0)), -1),
                         (dict(params=(-4, 0)), -1), (dict(params=(9, 1)), -1), (dict(H=4097), -6), (dict(W=4097), -6), (dict(B=65536), -6)):
        rc, text = _call(lib, **over)
        assert rc == status and text, over
    assert "max_d2 16130 outside 1..16129" in _call(lib, params=(16130, 0))[1]
    assert lib.cs_label_expand_last_timing(None, None, None) == -1


def test_a_null_handle_reports_no_device_for_valid_arguments():
    lib = L.load_library()
    no_dev = lib.cs_device_count() <= 0
    for over in (dict(), dict(params=(1, 0)), dict(params=(16129, 0)), dict(d2=True), dict(in_kind=1, out_kind=1), dict(H=4096, W=4096),
                 dict(B=65535, H=1, W=1)):
        assert _call(lib, **over)[0] == (-4 if no_dev else -1), over      # no handle: no device here, else a NULL handle
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            EX.LabelExpander(0).expand_batch(np.zeros((1, 8, 8), np.int32), 3)
        assert ei.value.status == -4
