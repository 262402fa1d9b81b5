"""The crop preprocess at any output size, the parts that need no GPU: the rectangular CPU reference
(tests/preprocess_sized_reference.py) against real scikit-image 0.18.3 / SciPy 1.7.1 outputs
(tests/golden/golden_preprocess_sized.npz), the two new C-ABI symbols, and the Python argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import preprocess_sized_reference as PR
from conftest import GOLDEN, ROOT
from cellscreen import _lib as L
from cellscreen import extract as X
from cellscreen import preprocess as pp
from oracle import preprocess_oracle as po

TOL_REF = 1e-12         # restatement vs scikit-image in float64; 1.4e-13 measured over 24 crops x 9 sizes when the bound was set
TOL_OUT = 6e-8          # tests/test_gpu_preprocess.py: one float32 rounding below 1.0


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_preprocess_sized.npz"))


def test_fixture_covers_what_it_claims(gold):
    n = int(gold["n"])
    assert n >= 16
    up = down = mixed = ratio16 = nonsquare = const = 0
    sizes = set()
    for i in range(n):
        c, (oh, ow) = gold[f"crop_{i}"], (int(v) for v in gold[f"hw_{i}"])
        assert gold[f"out_{i}"].dtype == np.float64 and gold[f"out_{i}"].shape == (oh, ow)
        sizes.add((oh, ow))
        H, W = c.shape
        up += H < oh and W < ow
        down += H > oh and W > ow
        mixed += (H < oh) != (W < ow) and H != oh and W != ow
        ratio16 += H == 16 * oh or W == 16 * ow
        nonsquare += oh != ow
        const += c.min() == c.max()
    assert up and down and mixed >= 2 and ratio16 >= 2 and nonsquare >= 4 and const
    assert (8, 8) in sizes and (256, 256) in sizes and (128, 128) in sizes and (64, 128) in sizes
    assert os.path.getsize(os.path.join(GOLDEN, "golden_preprocess_sized.npz")) < 1_000_000


def test_restatement_matches_scikit_image_at_every_fixture_size(gold):
    worst = 0.0
    for i in range(int(gold["n"])):
        c, hw = gold[f"crop_{i}"], tuple(int(v) for v in gold[f"hw_{i}"])
        ref = PR.preprocess_crop(c, hw, float(gold["clip_limit"]))
        err = np.abs(ref - gold[f"out_{i}"]).max()
        worst = max(worst, err)
        print(f"fixture {i} {c.shape} -> {hw}: {err:.3e}")
        assert err <= TOL_REF, f"fixture {i} {c.shape} -> {hw}: {err:.3e}"
        e32 = np.abs(ref.astype(np.float32).astype(np.float64) - gold[f"out_{i}"]).max()
        assert e32 <= TOL_OUT, f"fixture {i} after the float32 cast: {e32:.3e}"
    print(f"worst float64 difference {worst:.3e}")


def test_restatement_is_the_oracle_for_square_sizes():
    rng = np.random.default_rng(3)
    for shape in ((8, 8), (30, 77), (64, 64), (150, 41), (257, 255)):
        x = rng.random(shape)
        for s in (8, 32, 64, 128, 200):
            a, b = PR.resize_to(x, s, s), po.resize_to_64(x, s)
            assert a.shape == (s, s) and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (shape, s)
    c = (rng.random((40, 52)) * 65535).astype(np.uint16)
    assert np.array_equal(PR.preprocess_crop(c, (64, 64)), po.preprocess_crop(c))
    assert np.array_equal(PR.preprocess_crops([c], (64, 64)), po.preprocess_crops([c]))
    # the axes are independent: a rectangular output is the square one of each axis
    x = rng.random((45, 90))
    r = PR.resize_to(x, 32, 128)
    assert r.shape == (32, 128)
    assert np.abs(r - PR.resize_to(PR.resize_to(x, 32, 90), 32, 128)).max() <= 1e-12     # rows first, then columns


def test_header_declares_and_library_exports_the_size_calls():
    src = open(os.path.join(ROOT, "include", "cellscreen.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+cs_preproc_set_output_size\s*\(\s*cs_preproc\s*\*\s*p\s*,\s*int32_t\s+out_h\s*,\s*int32_t\s+out_w\s*\)\s*;", code)
    assert re.search(r"int\s+cs_preproc_get_output_size\s*\(\s*const\s+cs_preproc\s*\*\s*p\s*,\s*int32_t\s*\*\s*out_h\s*,"
                     r"\s*int32_t\s*\*\s*out_w\s*\)\s*;", code)
    assert "[n][out_h][out_w]" in src and "[n_cells][out_h][out_w]" in src
    lib = L.load_library()
    assert L.SIGNATURES["cs_preproc_set_output_size"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32])
    assert L.SIGNATURES["cs_preproc_get_output_size"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)])
    for name in ("cs_preproc_set_output_size", "cs_preproc_get_output_size"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == L.SIGNATURES[name][1]
    assert lib.cs_abi_version() == 2 and lib.cs_profile_kernel_count() == 13
    # without a handle they fail as the other handle calls do (cs_preproc_last_timing: CS_ERR_INVALID)
    h, w = C.c_int32(-5), C.c_int32(-5)
    assert lib.cs_preproc_last_timing(None, None, None) == -1
    assert lib.cs_preproc_set_output_size(None, 128, 128) == -1
    assert b"NULL" in lib.cs_last_error()
    assert lib.cs_preproc_get_output_size(None, C.byref(h), C.byref(w)) == -1 and (h.value, w.value) == (-5, -5)
    if lib.cs_device_count() <= 0:
        with pytest.raises(L.CellScreenError) as ei:
            pp.Preprocessor(0, out_hw=(128, 128))
        assert ei.value.status == -4                              # CS_ERR_NO_DEVICE, from cs_preproc_create


@pytest.mark.parametrize("bad", [(7, 64), (64, 7), (513, 64), (64, 513), (64.0, 64), ("64", 64), (True, 64), (64,), (64, 64, 1), 64, None,
                                 (0, 0), (-64, 64)])
def test_python_refuses_bad_output_sizes_before_the_library(bad, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(L, "load_library", no_library)
    with pytest.raises(ValueError):
        pp.Preprocessor(0, out_hw=bad)
    with pytest.raises(ValueError):
        X.CellExtractor(0, out_hw=bad)
    with pytest.raises(ValueError):
        X.label_cell_extractor(lambda seg: seg, 0, out_hw=bad)


def test_python_defaults_and_accepted_sizes():
    assert pp.OUT_SIDE == 64 and (pp.OUT_MIN, pp.OUT_MAX, pp.MAX_RATIO) == (8, 512, 16)
    assert pp.check_out_hw((8, 512)) == (8, 512) and pp.check_out_hw([np.int32(128), np.int64(64)]) == (128, 64)
    assert all(type(v) is int for v in pp.check_out_hw(np.array([32, 128])))
    e = X.CellExtractor(0)                                   # positional calls of today keep their meaning
    assert e.out_hw == (64, 64) and e._pre is None
    e = X.CellExtractor(0, (32, 128), min_area=10)
    assert e.out_hw == (32, 128) and e.qc["min_area"] == 10 and e._pre is None
    e = X.CellExtractor(0, min_area=10)
    assert e.out_hw == (64, 64) and e.qc["min_area"] == 10
