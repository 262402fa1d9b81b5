"""The crop preprocess and the label-image extraction at the model's own input size (Preprocessor(out_hw=...),
CellExtractor(out_hw=...), cs_preproc_set_output_size) against real scikit-image 0.18.3 outputs
(tests/golden/golden_preprocess_sized.npz) and the rectangular CPU reference (tests/preprocess_sized_reference.py).

Bars as in tests/test_gpu_preprocess.py: the CLAHE stage tap is bit-exact (it does not depend on the output size), and
|float32(kernel) - float64 reference| <= 6e-8, one float32 rounding below 1.0.

Where a compiled-in 64 could survive, and the test that sees it: the anti-aliasing sigma and the warp factors -- the
fixture pairs, the seeded crops and the ratio-rule test; the output stride -- the non-square sizes of the seeded crops; the
chunk loop's offsets and its staging size -- the chunk tests; the extraction's cell buffer and its copy size -- the
extraction tests."""
import os

import numpy as np
import pytest

import extract_reference as R
import helpers as H
import preprocess_sized_reference as PR
from conftest import GOLDEN
from cellscreen import _lib as L
from cellscreen import extract as X
from cellscreen import preprocess as pp
from cellscreen import synth
from oracle import preprocess_oracle as po

pytestmark = pytest.mark.gpu

TOL_OUT = 6e-8          # |fp32(hip fp64 result) - reference fp64 result|: one float32 rounding below 1.0 (test_gpu_preprocess.py)
SIZES = [(128, 128), (64, 128), (128, 64), (32, 32), (8, 8), (96, 48), (256, 256), (512, 16)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_preprocess_sized.npz"))


def _run(proc, crops, clip=0.02):
    pix, off, hs, ws = pp.pack_crops(crops)
    out, cl = proc.run_packed(pix, off, hs, ws, clip, want_clahe=True)
    return out, pp.split_clahe(cl, off, hs, ws)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1: real scikit-image outputs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.uint8, np.uint16])
def test_golden_pairs(gold, dt):
    idx = [i for i in range(int(gold["n"])) if gold[f"crop_{i}"].dtype == dt]
    assert len(idx) >= 6
    p = pp.Preprocessor(0)
    try:
        for i in idx:
            c, hw = gold[f"crop_{i}"], tuple(int(v) for v in gold[f"hw_{i}"])
            p.out_hw = hw
            out, cl = _run(p, [c], float(gold["clip_limit"]))
            assert out.dtype == np.float32 and out.shape == (1,) + hw
            assert np.array_equal(cl[0], po.clahe_u16(c)), f"CLAHE stage of fixture {i} is not bit-exact"
            err = np.abs(out[0].astype(np.float64) - gold[f"out_{i}"]).max()
            print(f"fixture {i} {c.shape} -> {hw}: {err:.3e}")
            assert err <= TOL_OUT, f"fixture {i} {c.shape} -> {hw}: {err:.3e}"
    finally:
        p.close()


# ---- 2: seeded ragged crops at eight sizes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k,hw", list(enumerate(SIZES)))
def test_seeded_ragged_crops_against_the_reference(k, hw):
    dt = (np.uint8, np.uint16)[k % 2]
    lim = tuple(min(300, pp.MAX_RATIO * o) for o in hw)          # every crop inside the ratio rule, per axis
    raw = synth.raw_crops(100 + k, 20, dt, 8, max(lim), flat_every=5)
    crops = [np.ascontiguousarray(c[:lim[0], :lim[1]]) for c in raw]
    p = pp.Preprocessor(0, out_hw=hw)
    try:
        out, cl = _run(p, crops)
    finally:
        p.close()
    assert out.shape == (len(crops),) + hw
    worst = 0.0
    for i, c in enumerate(crops):
        assert np.array_equal(cl[i], po.clahe_u16(c)), f"crop {i} {c.shape}"
        err = np.abs(out[i].astype(np.float64) - PR.preprocess_crop(c, hw)).max()
        worst = max(worst, err)
        assert err <= TOL_OUT, f"crop {i} {c.shape} -> {hw}: {err:.3e}"
    print(f"{hw}: worst {worst:.3e}")
    assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0


# ---- 3: the default is untouched; the size is state of the handle ----------------------------------------------------------------
def test_default_size_and_switching_sizes_on_one_handle():
    import ctypes as C
    crops = synth.raw_crops(7, 24, np.uint16, 8, 200, flat_every=4)
    d = pp.Preprocessor(0)
    e = pp.Preprocessor(0, out_hw=(64, 64))
    f = pp.Preprocessor(0, out_hw=(128, 128))
    s = pp.Preprocessor(0)
    try:
        assert d.out_hw == e.out_hw == (64, 64) and f.out_hw == (128, 128)
        base, base_cl = _run(d, crops)
        assert base.shape == (24, 64, 64)
        assert np.abs(base.astype(np.float64) - po.preprocess_crops(crops)).max() <= TOL_OUT
        o64, cl64 = _run(e, crops)
        assert np.array_equal(_bits(o64), _bits(base)) and all(np.array_equal(a, b) for a, b in zip(cl64, base_cl))
        big = f(crops)
        assert big.shape == (24, 128, 128)
        for hw, want in (((64, 64), base), ((128, 128), big), ((64, 64), base), ((64, 128), None), ((128, 128), big)):
            s.out_hw = hw
            h, w = C.c_int32(), C.c_int32()
            L.check(s._lib.cs_preproc_get_output_size(s._h, C.byref(h), C.byref(w)))
            assert (h.value, w.value) == hw == s.out_hw
            got = s(crops)
            assert got.shape == (24,) + hw
            if want is not None:
                assert np.array_equal(_bits(got), _bits(want)), hw
        # refused sizes leave the handle as it was
        for bad in ((7, 64), (64, 513), (0, 0)):
            assert s._lib.cs_preproc_set_output_size(s._h, *bad) == -1
        L.check(s._lib.cs_preproc_get_output_size(s._h, C.byref(h), C.byref(w)))
        assert (h.value, w.value) == (128, 128)
        with pytest.raises(ValueError):
            s.out_hw = (64, 7)
        assert s([]).shape == (0, 128, 128)
        import torch
        with pytest.raises(ValueError, match="128"):
            pix, off, hs, ws = pp.pack_crops(crops[:2])
            s.run_packed(torch.from_numpy(pix.view(np.int16)).cuda(), off, hs, ws, out=torch.empty((2, 64, 64), device="cuda"))
    finally:
        for q in (d, e, f, s):
            q.close()


# ---- 4: the ratio rule ----------------------------------------------------------------------------------------------------------
def test_ratio_rule_accepts_sixteen_and_refuses_beyond():
    import torch
    rng = np.random.default_rng(4)
    p = pp.Preprocessor(0, out_hw=(8, 8))
    q = pp.Preprocessor(0, out_hw=(32, 64))
    try:
        ok = [rng.integers(0, 256, (128, 128)).astype(np.uint8), rng.integers(0, 256, (128, 9)).astype(np.uint8),
              rng.integers(0, 256, (8, 128)).astype(np.uint8)]
        out = p(ok)
        for i, c in enumerate(ok):
            err = np.abs(out[i].astype(np.float64) - PR.preprocess_crop(c, (8, 8))).max()
            assert err <= TOL_OUT, f"{c.shape} -> (8, 8): {err:.3e}"
        # 512 x 1024 = (16 x 32, 16 x 64): two different blob crops side by side under noise, so that no half repeats the other
        a, b = synth.raw_crops(9, 2, np.uint16, 512, 512)
        wide = np.concatenate([a, b], axis=1) // 2 + rng.integers(0, 32768, (512, 1024)).astype(np.uint16)
        assert wide.shape == (512, 1024) and wide.dtype == np.uint16 and not np.array_equal(wide[:, :512], wide[:, 512:])
        out, cl = _run(q, [wide])
        assert np.array_equal(cl[0], po.clahe_u16(wide)), "CLAHE stage of the 512 x 1024 crop is not bit-exact"
        err = np.abs(out[0].astype(np.float64) - PR.preprocess_crop(wide, (32, 64))).max()
        assert err <= TOL_OUT, f"(512, 1024) -> (32, 64): {err:.3e}"
        # one more pixel on either axis: CS_ERR_UNSUPPORTED naming the crop, the side and the output size; nothing written
        for proc, shape, hw in ((p, (129, 20), (8, 8)), (p, (20, 129), (8, 8)), (q, (513, 64), (32, 64))):
            crops = [np.full((16, 16), 9, np.uint8), np.zeros(shape, np.uint8)]
            pix, off, hs, ws = pp.pack_crops(crops)
            dout = torch.full((2,) + hw, -1.0, device="cuda")
            with pytest.raises(L.CellScreenError) as ei:
                proc.run_packed(torch.from_numpy(pix).cuda(), off, hs, ws, out=dout)
            assert ei.value.status == -6, str(ei.value)                 # CS_ERR_UNSUPPORTED
            msg = str(ei.value)
            assert "crop 1" in msg and f"{shape[0]}x{shape[1]}" in msg and f"{hw[0]}x{hw[1]}" in msg, msg
            torch.cuda.synchronize()
            assert bool((dout == -1.0).all())
        with pytest.raises(RuntimeError, match="above 1024"):            # the absolute limit keeps its text
            q([np.zeros((8, 1025), np.uint8)])
        with pytest.raises(RuntimeError, match="below 8 px"):
            q([np.zeros((7, 30), np.uint8)])
    finally:
        p.close()
        q.close()


# ---- 5: the chunk loop at another size ----------------------------------------------------------------------------------------
def _small_crops(seed, n, lo, hi):
    rng = np.random.default_rng(seed)
    hs = rng.integers(lo, hi + 1, n).astype(np.int32)
    ws = rng.integers(lo, hi + 1, n).astype(np.int32)
    sizes = hs.astype(np.int64) * ws
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    pix = rng.integers(0, 256, int(sizes.sum()), dtype=np.uint8)
    return pix, off, hs, ws


def test_more_crops_than_one_chunk_at_a_rectangular_size():
    """A chunk holds 65,536 crops: cells on both sides of the boundary and the last one equal the same crops run alone."""
    import torch
    n, hw = 65536 + 300, (16, 32)
    pix, off, hs, ws = _small_crops(55, n, 8, 12)
    p = pp.Preprocessor(0, out_hw=hw)
    try:
        dout = torch.full((n,) + hw, -1.0, device="cuda")
        p.run_packed(torch.from_numpy(pix).cuda(), off, hs, ws, out=dout)
        torch.cuda.synchronize()
        pick = [0, 1, 65534, 65535, 65536, 65537, n - 2, n - 1]
        got = dout[pick].cpu().numpy()
        crops = [pix[off[i]:off[i] + int(hs[i]) * int(ws[i])].reshape(hs[i], ws[i]) for i in pick]
        alone = p(crops)
        assert np.array_equal(_bits(got), _bits(alone))
        for k in (0, 3, 4, 7):
            assert np.abs(got[k].astype(np.float64) - PR.preprocess_crop(crops[k], hw)).max() <= TOL_OUT
        assert float(dout.min()) >= 0.0 and float(dout.max()) <= 1.0      # every cell was written
        # host output goes through the staging buffer of a chunk
        m = 65536 + 40
        host = p.run_packed(pix, off[:m], hs[:m], ws[:m])
        assert host.shape == (m,) + hw
        assert np.array_equal(_bits(host[65530:m]), _bits(dout[65530:m].cpu().numpy()))
    finally:
        p.close()


def test_a_chunk_is_bounded_in_output_bytes():
    """1,030 crops at 512 x 512 are 1.08 GB of output: more than the 1 GiB a chunk may produce (1,024 such cells)."""
    import torch
    n, hw = 1030, (512, 512)
    pix, off, hs, ws = _small_crops(56, n, 8, 8)
    p = pp.Preprocessor(0, out_hw=hw)
    try:
        dout = torch.full((n,) + hw, -1.0, device="cuda")
        p.run_packed(torch.from_numpy(pix).cuda(), off, hs, ws, out=dout)
        torch.cuda.synchronize()
        for i in (0, 1022, 1023, 1024, 1025, n - 1):
            c = pix[off[i]:off[i] + 64].reshape(8, 8)
            err = np.abs(dout[i].cpu().numpy().astype(np.float64) - PR.preprocess_crop(c, hw)).max()
            assert err <= TOL_OUT, f"crop {i}: {err:.3e}"
        assert float(dout.min()) >= 0.0
    finally:
        p.close()


# ---- 6: extraction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(128, 128), (64, 128)])
def test_extraction_at_another_size(hw):
    import torch
    imgs, labs = synth.label_images(17, 3)
    e64 = X.CellExtractor(0)
    e = X.CellExtractor(0, out_hw=hw)
    p = pp.Preprocessor(0, out_hw=hw)
    try:
        r0 = e64.extract_batch(imgs, labs)
        r = e.extract_batch(imgs, labs)
        assert np.array_equal(r.regions, r0.regions) and np.array_equal(r.status, r0.status) and np.array_equal(r.cell_image, r0.cell_image)
        crops = []
        for b in range(3):
            c, _, st = R.extract(labs[b], imgs[b, ..., 1])
            assert st == R.IMAGE_OK == r.status[b]
            crops += c
        assert len(crops) == len(r.cells) > 10 and r.cells.shape == (len(crops),) + hw and r.cells.dtype == np.float32
        ref = p(crops)
        assert np.array_equal(_bits(r.cells), _bits(ref))
        assert np.abs(r.cells[:6].astype(np.float64) - np.stack([PR.preprocess_crop(c, hw) for c in crops[:6]])).max() <= TOL_OUT
        # CUDA tensors in, cells left on the device; then into a caller's tensor
        dev = torch.device("cuda", 0)
        ti, tl = torch.from_numpy(imgs.view(np.int16)).to(dev), torch.from_numpy(labs).to(dev)
        r1 = e.extract_batch(ti, tl)
        assert r1.cells.is_cuda and tuple(r1.cells.shape) == (len(crops),) + hw
        assert np.array_equal(_bits(r1.cells.cpu().numpy()), _bits(ref)) and np.array_equal(r1.regions, r0.regions)
        out = torch.full((len(crops) + 2,) + hw, -1.0, device=dev)
        r2 = e.extract_batch(ti, tl, out=out)
        assert torch.equal(out[:len(crops)], r1.cells) and bool((out[len(crops):] == -1).all()) and len(r2.cells) == len(crops)
        with pytest.raises(ValueError):
            e.extract_batch(ti, tl, out=torch.empty((len(crops), 64, 64), device=dev))
        cells, stats = e.extract(imgs[0], labs[0])
        assert cells.shape[1:] == hw and len(stats) == len(cells)
    finally:
        for q in (e64, e, p):
            q.close()


def test_extraction_marks_an_image_beyond_the_ratio_unsupported():
    """A passing region 30 x 140: fine at 64 x 64, beyond 16 x 8 columns at (8, 8).  The other image of the batch keeps its cells."""
    Hh = Ww = 200
    lab = np.zeros((2, Hh, Ww), np.int32)
    lab[0, 20:50, 30:170] = 3
    lab[0, 100:130, 100:140] = 5
    lab[1, 60:100, 50:90] = 2
    rng = np.random.default_rng(3)
    img = rng.integers(100, 60000, (2, Hh, Ww), dtype=np.uint16)
    qc = dict(max_eccentricity=1.0)
    e64 = X.CellExtractor(0, **qc)
    e8 = X.CellExtractor(0, (8, 8), **qc)
    p8 = pp.Preprocessor(0, out_hw=(8, 8))
    try:
        r0 = e64.extract_batch(img, lab)
        assert list(r0.status) == [X.IMAGE_OK, X.IMAGE_OK] and len(r0.cells) == 3
        r = e8.extract_batch(img, lab)
        assert list(r.status) == [X.IMAGE_UNSUPPORTED, X.IMAGE_OK]
        assert list(r.regions["failed"]) == [0, 0, 0] and list(r.regions["cell"]) == [-1, -1, 0]
        assert r.cells.shape == (1, 8, 8) and np.array_equal(_bits(r.cells), _bits(p8([img[1, 60:100, 50:90]])))
        with pytest.raises(ValueError, match="8x8"):
            e8.extract(img[0], lab[0])
        with pytest.raises(L.CellScreenError) as ei:                     # the host check of cs_preprocess says the same of that crop
            p8([np.ascontiguousarray(img[0, 20:50, 30:170])])
        assert ei.value.status == -6
        # a size set between the measure and its fill is refused; afterwards it is accepted
        import ctypes as C
        nr, nc = C.c_int64(), C.c_int64()
        h = e8._handle
        lib = e8._lib
        L.check(lib.cs_extract_measure(h, img.ctypes.data, 1, 1, 0, lab.ctypes.data, 2, Hh, Ww, 0, 5, C.byref(e8._qc), C.byref(nr), C.byref(nc)))
        assert (nr.value, nc.value) == (3, 1)
        assert lib.cs_preproc_set_output_size(h, 64, 64) == -1 and b"cs_extract_fill" in lib.cs_last_error()
        cells = np.full((1, 8, 8), -1.0, np.float32)
        L.check(lib.cs_extract_fill(h, None, None, 0, cells.ctypes.data, None, 0))
        assert np.array_equal(_bits(cells), _bits(r.cells))
        assert lib.cs_preproc_set_output_size(h, 8, 8) == 0
    finally:
        for q in (e64, e8, p8):
            q.close()


# ---- 7: end to end ---------------------------------------------------------------------------------------------------------------
def _threshold_segmenter(seg):
    from scipy import ndimage
    lab, _ = ndimage.label(seg > int(seg.max()) // 2)
    return lab.astype(np.int32)


def test_label_images_to_flags_end_to_end_on_a_rectangular_model(tmp_path):
    """From label images to flags with a model whose input is 32 x 128 (the reference's seven convs, 4 x 16 x 32 = 2,048
    features): the training set, two epochs, the detector fit and the screening all take their cells from
    label_cell_extractor(out_hw=(32, 128)); the screening against the CPU chain reference -> CAE / detector oracle."""
    from cellscreen import model_io
    from cellscreen.screening import ProductionMutantScreening
    from cellscreen.training import ImprovedAnomalyDetectionTraining
    from oracle import oracle
    hw = (32, 128)
    d = tmp_path / "train"
    d.mkdir()
    imgs, _ = synth.label_images(61, 10, hw=(384, 384))            # ~14 cells per image survive the threshold segmenter
    crops = []
    for i in range(len(imgs)):
        np.save(d / f"f{i:02d}.npy", imgs[i])
        c, _, st = R.extract(_threshold_segmenter(imgs[i, ..., 2]), imgs[i, ..., 1])
        assert st == R.IMAGE_OK
        crops += c
    out = str(tmp_path / "models")
    t = ImprovedAnomalyDetectionTraining(out, epochs=2, verbose=0)
    cells, df = t.create_training_dataset(str(d), X.label_cell_extractor(_threshold_segmenter, out_hw=hw), file_pattern="*.npy")
    assert cells.shape == (len(crops),) + hw and len(crops) >= 100 and len(df) == len(crops)
    ref64 = np.stack([PR.preprocess_crop(c, hw) for c in crops])
    assert np.abs(cells.astype(np.float64) - ref64).max() <= TOL_OUT
    x_ref = ref64.astype(np.float32)
    autoencoder, encoder, history = t.train_autoencoder(cells)
    assert autoencoder.input_hw == hw and len(history.history["loss"]) == 2 and np.isfinite(history.history["val_loss"]).all()
    t.create_anomaly_detector(encoder, cells)
    s = ProductionMutantScreening(out, cell_extractor=X.label_cell_extractor(_threshold_segmenter, out_hw=hw), file_pattern="*.npy")
    assert (s.engine.info.height, s.engine.info.width) == hw and s.engine.info.feature_dim == 2048
    n_img = 3
    got_cells = []
    for i in range(n_img):
        c, stats = s.extract_quality_cells(str(d / f"f{i:02d}.npy"))
        assert len(c) == len(stats) > 0
        got_cells += c
    n = len(got_cells)
    assert np.array_equal(_bits(np.stack(got_cells)), _bits(cells[:n].astype(np.float32)))
    r = s.compute_anomaly_scores(got_cells)
    # preprocess_crops of the screening class follows the loaded model's size
    assert np.array_equal(_bits(s.preprocess_crops(crops[:n])), _bits(np.stack(got_cells)))
    ae, enc, det = model_io.load_model_dir(out)
    ref = oracle.screen(ae, enc, det, x_ref[:n], acc64=True)
    H.assert_rel(r["reconstruction_mse"], ref["mse"], H.TOL_ERR_REL, "mse")
    H.assert_rel(r["reconstruction_mae"], ref["mae"], H.TOL_ERR_REL, "mae")
    for name, key, p in (("cons", "conservative", det.conservative), ("mod", "moderate", det.moderate)):
        tol = H.TOL_DEC_E2E * np.abs(p.dual_coef).sum()
        assert np.abs(r[f"{key}_scores"] - ref[f"{name}_score"]).max() <= tol, name
        H.flags_agree(-r[f"{key}_scores"], r[f"{key}_predictions"], ref[f"{name}_dec"], ref[f"{name}_pred"], tol, name)
    s.screen_mutant_samples({"S": str(d)}, str(tmp_path / "screen"))
    import pandas as pd
    assert len(pd.read_csv(tmp_path / "screen" / "detailed_cell_results.csv")) == len(crops)


def test_raw_crops_to_the_large_model_on_the_device():
    """Raw crops -> Preprocessor(out_hw=(128, 128)) -> the 128 x 128 / 128-channel model, crops resident in HBM in between,
    against the CPU chain (reference at (128, 128) -> CAE oracle)."""
    import torch
    from cellscreen.engine import Engine
    from oracle import oracle
    hw = (128, 128)
    w = synth.random_cae(seed=5, hw=hw, channels=(32, 64, 128, 128, 64, 32, 1), n_enc=3)
    raw = synth.raw_crops(71, 6, np.uint16, 30, 90, flat_every=4) + synth.raw_crops(72, 2, np.uint16, 150, 260)
    pix, off, hs, ws = pp.pack_crops(raw)
    p = pp.Preprocessor(0, out_hw=hw)
    e = Engine.from_weights(w)
    try:
        d_out = torch.empty((len(raw),) + hw, dtype=torch.float32, device="cuda")
        p.run_packed(torch.from_numpy(pix.view(np.int16)).cuda(), off, hs, ws, out=d_out)
        _, mse, mae = e.reconstruct(d_out, want_recon=False)
        feats = e.encode(d_out, which=0)
        ref64 = np.stack([PR.preprocess_crop(c, hw) for c in raw])
        assert np.abs(d_out.cpu().numpy().astype(np.float64) - ref64).max() <= TOL_OUT
        x_ref = ref64.astype(np.float32)
        ref = oracle.cae_forward(w, x_ref, acc64=True, want=("features", "mse", "mae"))
        H.assert_rel(mse.cpu().numpy(), ref["mse"], H.TOL_ERR_REL, "mse")
        H.assert_rel(mae.cpu().numpy(), ref["mae"], H.TOL_ERR_REL, "mae")
        H.assert_close_scaled(feats.cpu().numpy(), ref["features"].reshape(len(raw), -1), H.TOL_FEATURES, "features")
    finally:
        e.close()
        p.close()
