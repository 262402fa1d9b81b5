"""Parity tests proper: the HIP path (through the C ABI) against the CPU oracle on the same
seeded inputs and against the committed golden vectors.  Run on the GPU box: -m gpu.
Tolerances are the stated ones (helpers.py / SURVEY.md Appendix G); integer and
bookkeeping results are bit-exact."""
import os

import numpy as np
import pytest

import helpers as H
from cellscreen import _lib as L
from cellscreen import model_io, spec, synth
from cellscreen.engine import Engine
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def weights():
    return synth.random_cae(seed=42)


@pytest.fixture(scope="module")
def det(golden_det):
    return H.det_from_golden(golden_det)


PRECISIONS = ["split16", "fp32_exact"]


@pytest.fixture(scope="module", params=PRECISIONS)
def engine(request, weights, det):
    """Every test that takes `engine` runs in BOTH precisions of cs_model_options at the SAME tolerances: "split16" (the default:
    two-term fp16 splits on the 16-bit matrix instructions) and "fp32_exact" (every contraction on v_mfma_f32_16x16x4_f32)."""
    e = Engine.from_weights(weights, None, det, precision=request.param)
    assert e.precision == request.param
    yield e
    e.close()


@pytest.fixture(scope="module")
def crops():
    return np.concatenate([synth.synth_crops(42, 0, 40), synth.blob_crops(4, 8)])


def test_native_library_is_loaded_and_on_gfx950(engine):
    assert engine.info.shared_encoder == 1 and engine.info.has_detector == 1
    assert engine.info.feature_dim == 2048 and engine.info.n_components == 100
    maps = open("/proc/self/maps").read()
    assert "libcellscreen.so" in maps


def test_synth_crops_bit_exact(engine):
    import torch
    t = torch.empty((33, 64, 64), dtype=torch.float32, device="cuda")
    engine.synth_crops(42, 123456, t)
    assert np.array_equal(t.cpu().numpy(), oracle.synth_crops(42, 123456, 33))


@pytest.mark.parametrize("layer", range(7))
def test_each_layer_against_oracle(engine, weights, crops, layer):
    ref = oracle.cae_forward(weights, crops, acc64=True, layers=True)["layers"][layer]
    got = engine.layer_output(crops, layer)
    if layer == 6:
        got = got[..., 0] if got.ndim == 4 else got
        ref = ref[..., 0]
        assert np.abs(got.astype(np.float64) - ref).max() <= H.TOL_RECON
    else:
        H.assert_close_scaled(got, ref, 1e-5, f"layer {layer}")


def test_conv4_split_contraction_is_in_the_fp32_error_class(weights, crops):
    """conv4 takes its fp32 contraction on the 16-bit matrix pipe as a two-term fp16 split (three products, exact power-of-two
    operand scales: conv4_h2_kernel) with precision="split16", on the fp32 matrix instructions with "fp32_exact".  Each is compared
    with a float64 conv of the p3 the SAME engine produced, so only conv4's arithmetic is in the error: both must sit at fp32
    rounding level, far inside the 1e-5 layer tolerance."""
    k = weights.kernels[3].astype(np.float64)
    s = weights.bn_gamma[3].astype(np.float64) / np.sqrt(weights.bn_var[3].astype(np.float64) + weights.bn_eps)

    def conv4_error(precision):
        e = Engine.from_weights(weights, precision=precision)
        p3, a4 = e.layer_output(crops, 2), e.layer_output(crops, 3)
        prof = e.profile()["conv4_relu_bn"]
        e.close()
        xp = np.pad(p3.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
        z = sum(np.einsum("nyxc,co->nyxo", xp[:, dy:dy + 8, dx:dx + 8, :], k[dy, dx]) for dy in range(3) for dx in range(3))
        ref = np.maximum(z + weights.biases[3], 0.0) * s + (weights.bn_beta[3] - weights.bn_mean[3] * s)
        return H.assert_close_scaled(a4, ref, 2e-6, "conv4, " + precision), prof, a4

    eh, ph, h4 = conv4_error("split16")
    eb, pb, b4 = conv4_error("fp32_exact")
    assert ph["bf16_mfma_per_cell"] == 216 and ph["mfma_per_cell"] == 0          # the option really switches kernels
    assert pb["bf16_mfma_per_cell"] == 0 and pb["mfma_per_cell"] == 576
    assert not np.array_equal(h4, b4)
    print(f"conv4 max err / max|ref|: split16 {eh:.3e}, fp32 MFMA {eb:.3e}")


@pytest.mark.parametrize("scale", [1.0, 255.0, 3.0e-4, 1.0e6])
def test_fp16_split_kernels_scale_with_the_data(weights, det, scale):
    """The two-term fp16 split needs its operands inside fp16's range, so the kernels scale every staged strip / cell by an exact
    power of two taken from its own maximum.  The same bars must therefore hold when the crops are not in [0,1] at all -- raw
    8-bit values, tiny values, huge ones -- and when one cell of a batch is 10^9 times smaller than its neighbour (a scale per
    batch would flush it).  All seven layer outputs and the error sums against the fp64-evaluated oracle."""
    x = oracle.synth_crops(7, 100, 12) * np.float32(scale)
    x[3] *= np.float32(1e-9)            # a cell far below its neighbours
    x[5] = 0.0                          # an all-zero cell
    x[7, :32] = 0.0                     # strips that are entirely zero next to strips that are not
    e = Engine.from_weights(weights)
    ref = oracle.cae_forward(weights, x, acc64=True, want=("features", "recon", "mse", "mae"), layers=True)
    try:
        for layer in range(6):
            got = e.layer_output(x, layer)
            for c in range(len(x)):         # per cell: a small cell must be right at ITS scale
                rc = ref["layers"][layer][c]
                # BatchNormalization's shift is a floor under every activation: the bar is relative to the cell's range
                H.assert_close_scaled(got[c], rc, H.TOL_FEATURES, f"layer {layer}, cell {c}, input scale {scale:g}")
        rec, mse, mae = e.reconstruct(x)
        # the fused screening kernels (conv6 + conv7 + error in one: conv6 there is the fp16-split kernel) on the same crops
        e2 = Engine.from_weights(weights, None, det)
        r = e2.screen(x)
        e2.close()
        if scale <= 1.0:
            # the absolute bar on the reconstruction presumes crops in [0,1] (improved_detection.py:98-99 makes them so): the
            # sigmoid's argument then is O(1).  With crops of 1e6 it is O(1e5) and ANY fp32 evaluation of it is off by ~0.1
            # where it crosses zero -- not a property of these kernels (the layer checks above are relative to the range)
            assert np.abs(rec - ref["recon"]).max() <= H.TOL_RECON
            H.assert_rel(mse, ref["mse"], H.TOL_ERR_REL, "mse")
            H.assert_rel(mae, ref["mae"], H.TOL_ERR_REL, "mae")
            H.assert_rel(r["mse"], ref["mse"], H.TOL_ERR_REL, "fused mse")
            H.assert_rel(r["mae"], ref["mae"], H.TOL_ERR_REL, "fused mae")
        else:
            assert np.isfinite(rec).all() and np.isfinite(r["mse"]).all()
            live = ref["mse"] > 0
            H.assert_rel(r["mse"][live], mse[live], 1e-4, "fused vs two-kernel mse")     # the two evaluations agree with each other
    finally:
        e.close()


def test_fp16_split_results_do_not_depend_on_the_batch(weights, det):
    """A cell's scales come from its own data, so its results are bit-identical whatever else is screened with it."""
    x = oracle.synth_crops(11, 0, 40)
    x[1] *= np.float32(1000.0)
    e = Engine.from_weights(weights, None, det)
    try:
        whole = e.screen(x)
        for idx in ([0], [1], [2, 3], list(range(5, 40))):
            part = e.screen(x[idx])
            for k in whole:
                assert np.array_equal(part[k], whole[k][idx]), k
    finally:
        e.close()


@pytest.mark.parametrize("scale", [1.0, 255.0])
def test_fused_conv4_conv5_equals_the_two_kernels(weights, scale):
    """conv4 + conv5 run as one kernel whenever a4 itself is not asked for (conv45_h2_kernel: a4 goes through the same per-cell
    maximum -> power-of-two scale -> [hi | lo] planes inside LDS that conv5_h2_kernel builds from HBM): the same arithmetic in the
    same order, so a5 and everything downstream are bit-identical to the two-kernel path behind CS_DEBUG_NO_FUSE45."""
    x = (oracle.synth_crops(31, 0, 70) * np.float32(scale)).astype(np.float32)
    e = Engine.from_weights(weights)
    a5 = e.layer_output(x, 4)
    a4 = e.layer_output(x, 3)                 # last = 3: the stand-alone conv4
    rec = e.reconstruct(x)
    e.close()
    e2 = Engine.from_weights(weights, debug_flags=L.DEBUG_NO_FUSE45)
    assert e2.info.debug_flags == L.DEBUG_NO_FUSE45
    try:
        assert np.array_equal(e2.layer_output(x, 3), a4)
        assert np.array_equal(e2.layer_output(x, 4), a5)
        rec2 = e2.reconstruct(x)
        for got, want in zip(rec, rec2):
            assert np.array_equal(got, want)
    finally:
        e2.close()


def test_small_calls_run_the_detector_tail_split_with_identical_results(weights, det):
    """A call of at most 16,384 cells runs the PCA GEMM's feature ranges and the SVMs' support-vector ranges side by side in separate
    workgroups (a 128-cell call is otherwise two workgroups / one workgroup walking everything in sequence) and adds the range sums in
    the order the one-workgroup kernels add them: every output is bit-identical to the same cells screened inside a large call, and to
    the one-workgroup form forced by CS_DEBUG_NO_SMALL_SPLIT.  Host input runs in passes of 16,384 cells unless the pass size is
    set (api.hip:410-413), so the large calls set it to the whole call: one pass of 17,084 cells, above the limit."""
    n_big = 16384 + 700
    x = oracle.synth_crops(23, 0, n_big)
    e = Engine.from_weights(weights, None, det)
    try:
        e.set_chunk(n_big)
        whole = e.screen(x)                                  # one pass above the limit: the one-workgroup kernels
        pca_big = e.scaler_pca(e.encode(x))[:300]            # the same cells inside 17,084: not split
        e.set_chunk(0)
        f = e.encode(x[:300])
        pca_small = e.scaler_pca(f)                          # 300 cells: split
        assert np.array_equal(pca_small, pca_big)
        for idx in (slice(0, 1), slice(0, 300), slice(300, 1337), slice(0, 16384)):
            part = e.screen(x[idx])
            for k in whole:
                assert np.array_equal(part[k], whole[k][idx]), (k, idx)
    finally:
        e.close()
    e1 = Engine.from_weights(weights, None, det, debug_flags=L.DEBUG_NO_SMALL_SPLIT)
    try:
        one = e1.screen(x[:300])
        for k in whole:
            assert np.array_equal(one[k], whole[k][:300]), k
    finally:
        e1.close()


def test_conv3_winograd_on_the_16_bit_pipe_is_in_the_fp32_error_class(weights, crops):
    """conv3 = the feature vector.  Its Winograd F(2x2,3x3) contraction runs as a two-term fp16 split with precision="split16"
    (conv3_wino_h2_kernel, 768 MFMAs per cell) and on fp32 MFMAs with "fp32_exact" (2,048): each against a float64 conv + ReLU + BN +
    max-pool of the p2 the SAME engine made."""
    k = weights.kernels[2].astype(np.float64)
    s = weights.bn_gamma[2].astype(np.float64) / np.sqrt(weights.bn_var[2].astype(np.float64) + weights.bn_eps)

    def conv3_error(precision):
        e = Engine.from_weights(weights, precision=precision)
        p2, p3 = e.layer_output(crops, 1), e.layer_output(crops, 2)
        prof = e.profile()["conv3_relu_bn_pool"]
        e.close()
        xp = np.pad(p2.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
        z = sum(np.einsum("nyxc,co->nyxo", xp[:, dy:dy + 16, dx:dx + 16, :], k[dy, dx]) for dy in range(3) for dx in range(3))
        a = np.maximum(z + weights.biases[2], 0.0) * s + (weights.bn_beta[2] - weights.bn_mean[2] * s)
        ref = a.reshape(len(a), 8, 2, 8, 2, 32).max(axis=(2, 4))
        return H.assert_close_scaled(p3, ref, 3e-6, "conv3, " + precision), prof, p3

    eh, ph, h3 = conv3_error("split16")
    eb, pb, b3 = conv3_error("fp32_exact")
    assert ph["bf16_mfma_per_cell"] == 768 and ph["mfma_per_cell"] == 0 and pb["bf16_mfma_per_cell"] == 0 and pb["mfma_per_cell"] == 2048
    assert not np.array_equal(h3, b3)
    print(f"conv3 max err / max|ref|: split16 {eh:.3e}, fp32 MFMAs {eb:.3e}")


@pytest.mark.parametrize("n", [1, 3, 769, 1537])
def test_bottleneck_split_kernels_at_odd_cell_counts(weights, n):
    """conv4 / conv5 (csrc/conv45_h2.hip) are persistent workgroups that prefetch the next cell while one is in the matrix
    phase: counts below, at and past their resident grids (2 and 1 workgroups per CU x 256 CUs) against the oracle."""
    x = synth.synth_crops(23, 4242, n)
    ref = oracle.cae_forward(weights, x, acc64=True, layers=True)["layers"]
    e = Engine.from_weights(weights)
    try:
        for l in (3, 4):
            H.assert_close_scaled(e.layer_output(x, l), ref[l], 1e-5, f"layer {l}, {n} cells")
    finally:
        e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_golden_cae_vectors(golden_cae, precision):
    g = golden_cae
    e = Engine.from_weights(H.cae_from_golden(g), precision=precision)
    feats = e.encode(g["crops"], which=0)
    H.assert_close_scaled(feats, g["features"], H.TOL_FEATURES, "golden features")
    rec, mse, mae = e.reconstruct(g["crops"])
    assert np.abs(rec.astype(np.float64) - g["recon"]).max() <= H.TOL_RECON
    H.assert_rel(mse, g["mse"], H.TOL_ERR_REL, "golden mse")
    H.assert_rel(mae, g["mae"], H.TOL_ERR_REL, "golden mae")
    for l in range(6):
        flat = e.layer_output(g["crops"], l).reshape(len(g["crops"]), -1).astype(np.float64)
        H.assert_close_scaled(flat[:, :64], g[f"layer{l}_first64"], 1e-5, f"golden layer{l} head")
        H.assert_rel(flat.sum(axis=1), g[f"layer{l}_sum"], 1e-5, f"golden layer{l} sum")
    e.close()


def test_golden_detector_stages(engine, det, golden_det):
    g = golden_det
    pca = engine.scaler_pca(g["test_features"])
    H.assert_close_scaled(pca, g["pca"], H.TOL_STAGE, "scaler+pca stage vs sklearn")
    dc, dm = engine.svm_decision(g["pca"])
    for name, dec, p in (("cons", dc, det.conservative), ("mod", dm, det.moderate)):
        tol = H.TOL_DEC_STAGE * np.abs(p.dual_coef).sum()
        assert np.abs(dec - g[f"{name}_dec"]).max() <= tol, name
        pred = np.where(dec > 0, 1, -1)
        H.flags_agree(dec, pred, g[f"{name}_dec"], g[f"{name}_pred"], tol, name)


def test_screen_end_to_end_against_oracle(engine, weights, det, crops):
    ref = oracle.screen(weights, None, det, crops, acc64=True)
    r = engine.screen(crops)
    H.assert_rel(r["mse"], ref["mse"], H.TOL_ERR_REL, "mse")
    H.assert_rel(r["mae"], ref["mae"], H.TOL_ERR_REL, "mae")
    skipped = 0
    for name, p in (("cons", det.conservative), ("mod", det.moderate)):
        tol = H.TOL_DEC_E2E * np.abs(p.dual_coef).sum()
        assert np.abs(r[f"{name}_score"] - ref[f"{name}_score"]).max() <= tol, name
        assert r[f"{name}_pred"].dtype == np.int8 and set(np.unique(r[f"{name}_pred"])) <= {-1, 1}
        skipped += H.flags_agree(-r[f"{name}_score"], r[f"{name}_pred"], ref[f"{name}_dec"], ref[f"{name}_pred"], tol, name)
        # label is exactly the sign rule applied to the returned score (svm.cpp:2838)
        assert np.array_equal(r[f"{name}_pred"], np.where(-r[f"{name}_score"] > 0, 1, -1))
    print("labels within tolerance of 0 (not compared):", skipped)


def test_host_input_pipeline_is_chunk_invariant(engine, crops):
    """Host crops go through two staging buffers with the copy of chunk i+1 overlapping the kernels of
    chunk i; any chunking must give the same bits as one pass, for host and device inputs alike."""
    import torch
    whole = engine.screen(crops)
    try:
        for chunk in (1, 5, 16, 47):
            engine.set_chunk(chunk)
            part = engine.screen(crops)
            for k in whole:
                assert np.array_equal(part[k], whole[k]), f"chunk {chunk}: {k}"
        dev = engine.screen(torch.from_numpy(crops).cuda())
        for k in whole:
            assert np.array_equal(dev[k].cpu().numpy(), whole[k]), f"device input: {k}"
    finally:
        engine.set_chunk(16384)


def test_separate_encoder_weight_set(weights, det, crops):
    """encoder.keras != autoencoder's encoder half (CAE...:270-275 vs :300): features must come
    from the encoder set, reconstruction errors from the autoencoder set."""
    enc = synth.perturbed_encoder(weights)
    e = Engine.from_weights(weights, enc, det)
    assert e.info.shared_encoder == 0
    x = crops[:12]
    ref = oracle.screen(weights, enc, det, x, acc64=True)
    r = e.screen(x)
    H.assert_rel(r["mse"], ref["mse"], H.TOL_ERR_REL, "mse (autoencoder weights)")
    H.assert_close_scaled(e.encode(x, which=1), ref["features"], H.TOL_FEATURES, "features (encoder.keras weights)")
    fa = oracle.cae_forward(weights, x, acc64=True, want=("features",))["features"]
    H.assert_close_scaled(e.encode(x, which=0), fa, H.TOL_FEATURES, "features (autoencoder half)")
    tol = H.TOL_DEC_E2E * np.abs(det.conservative.dual_coef).sum()
    assert np.abs(r["cons_score"] - ref["cons_score"]).max() <= tol
    # identical weight sets are detected as shared
    e2 = Engine.from_weights(weights, weights.encoder_half(), det)
    assert e2.info.shared_encoder == 1
    e.close(); e2.close()


def test_chunking_and_ragged_sizes(engine, weights, det):
    """Results must not depend on the internal chunk size; n = 0, 1 and non-multiples work."""
    x = synth.synth_crops(5, 0, 37)
    engine.set_chunk(4096)
    base = engine.screen(x)
    for ch in (1, 5, 16, 36, 37):
        engine.set_chunk(ch)
        r = engine.screen(x)
        for k in base:
            assert np.array_equal(r[k], base[k]), (ch, k)
    engine.set_chunk(4096)
    one = engine.screen(x[:1])
    assert np.array_equal(one["mse"], base["mse"][:1]) and np.array_equal(one["cons_score"], base["cons_score"][:1])
    empty = engine.screen(np.zeros((0, 64, 64), np.float32))
    assert all(len(v) == 0 for v in empty.values())


def test_device_resident_buffers_match_host_path(engine):
    import torch
    x = synth.synth_crops(8, 0, 50)
    host = engine.screen(x)
    xd = torch.from_numpy(x).cuda()
    dev = engine.screen(xd)
    for k in host:
        assert dev[k].is_cuda
        assert np.array_equal(dev[k].cpu().numpy(), host[k]), k


def test_extreme_inputs(engine, weights):
    """All-zero, all-one and a single bright pixel at each corner (zero padding at the borders)."""
    x = np.zeros((6, 64, 64), np.float32)
    x[1] = 1.0
    x[2, 0, 0] = 1.0; x[3, 0, 63] = 1.0; x[4, 63, 0] = 1.0; x[5, 63, 63] = 1.0
    ref = oracle.cae_forward(weights, x, acc64=True)
    rec, mse, mae = engine.reconstruct(x)
    assert np.abs(rec.astype(np.float64) - ref["recon"]).max() <= H.TOL_RECON
    H.assert_rel(mse, ref["mse"], H.TOL_ERR_REL, "mse")
    H.assert_close_scaled(engine.encode(x, which=0), ref["features"], H.TOL_FEATURES, "features")


def test_non_finite_and_negative_crops_inside_a_batch(engine, weights, det):
    """A NaN crop, a crop with one +Inf pixel and a negative crop inside a batch of 40 (both precisions).  The reference would raise
    for the whole call (pca.transform: "Input X contains NaN", improved_detection.py:135); here the non-finite cell alone is marked --
    mse / mae NaN or Inf (NumPy's mean over a non-finite difference, :126-127), both scores NaN, both flags -1 -- and EVERY other
    cell is bit-identical to the batch without it (the persistent workgroups carry LDS images from cell to cell: the pixel is
    taken as 0 when a crop is staged).  A negative crop is an ordinary input: oracle parity at the usual bars."""
    x = oracle.synth_crops(19, 0, 40)
    x[7] = -x[7]                                            # a negative crop
    clean = engine.screen(x)
    ref = oracle.screen(weights, None, det, x[7:8], acc64=True)
    H.assert_rel(clean["mse"][7:8], ref["mse"], H.TOL_ERR_REL, "mse of the negative crop")
    assert abs(clean["cons_score"][7] - ref["cons_score"][0]) <= H.TOL_DEC_E2E * np.abs(det.conservative.dual_coef).sum()
    for poison in ("nan_crop", "inf_pixel", "nan_pixel_first_cell", "nan_pixel_last_cell"):
        y = x.copy()
        if poison == "nan_crop":
            bad = 13; y[bad] = np.nan
        elif poison == "inf_pixel":
            bad = 22; y[bad, 31, 5] = np.inf
        elif poison == "nan_pixel_first_cell":
            bad = 0; y[bad, 0, 0] = np.nan
        else:
            bad = 39; y[bad, 63, 63] = -np.inf
        for inp in (y, np.concatenate([y] * 20)):           # 40 cells: one per workgroup; 800: cells follow each other in a workgroup
            r = engine.screen(inp)
            for rep in range(len(inp) // 40):
                sl = slice(40 * rep, 40 * rep + 40)
                assert not np.isfinite(r["mse"][sl][bad]) and not np.isfinite(r["mae"][sl][bad]), poison
                assert np.isnan(r["cons_score"][sl][bad]) and np.isnan(r["mod_score"][sl][bad]), poison
                assert r["cons_pred"][sl][bad] == -1 and r["mod_pred"][sl][bad] == -1
                keep = np.arange(40) != bad
                for k in clean:
                    assert np.array_equal(r[k][sl][keep], clean[k][keep]), (poison, k, rep)
        # the other entry points: features / reconstruction errors of the other cells are untouched too
        f = engine.encode(y, which=0)
        assert np.array_equal(f[keep], engine.encode(x, which=0)[keep]) and np.isfinite(f).all()
        _, mse, _ = engine.reconstruct(y, want_recon=False)
        assert np.array_equal(mse[keep], clean["mse"][keep]) and not np.isfinite(mse[bad])


def test_negative_bn_scale(det):
    """BN between ReLU and pool with negative gamma: pool must see BN output (SURVEY finding 2)."""
    w = synth.random_cae(seed=5)
    for l in range(6):
        w.bn_gamma[l][::2] *= -1.0
    e = Engine.from_weights(w)
    x = synth.synth_crops(3, 0, 4)
    ref = oracle.cae_forward(w, x, acc64=True)
    H.assert_close_scaled(e.encode(x, which=0), ref["features"], H.TOL_FEATURES, "features, negative gamma")
    _, mse, _ = e.reconstruct(x, want_recon=False)
    H.assert_rel(mse, ref["mse"], H.TOL_ERR_REL, "mse, negative gamma")
    e.close()


def test_model_dir_load_and_csv_out(tmp_path, weights, det):
    """model_dir-load / screen / CSV-out through the host mirror of the reference class."""
    import pandas as pd
    from cellscreen.screening import ProductionMutantScreening
    mdir = str(tmp_path / "models")
    model_io.save_model_dir(mdir, weights, None, det)
    a = tmp_path / "strainA"; b = tmp_path / "strainB"
    a.mkdir(); b.mkdir()
    xa, xb = synth.synth_crops(1, 0, 9), synth.blob_crops(2, 6)
    np.save(a / "f1.npy", xa[:4]); np.save(a / "f2.npy", xa[4:]); np.save(b / "g.npy", xb)
    s = ProductionMutantScreening(mdir, file_pattern="*.npy")
    results, detailed = s.screen_mutant_samples({"A": str(a), "B": str(b)}, str(tmp_path / "out"))
    ref = oracle.screen(weights, None, det, xa, acc64=True)
    H.assert_rel([d["mse"] for d in detailed[:9]], ref["mse"], H.TOL_ERR_REL, "csv mse")
    assert [d["cell_id"] for d in detailed] == list(range(9)) + list(range(6))
    assert results["A"]["total_cells"] == 9 and results["A"]["files_processed"] == 2
    # flags: identical to the oracle's wherever its decision is further from 0 than the end-to-end score tolerance; the rate the
    # reference prints is then the count of anomaly flags over the cells (improved_detection.py:152-153), bit for bit
    for name, p in (("conservative", det.conservative), ("moderate", det.moderate)):
        key = name[:4] if name == "conservative" else name[:3]
        tol = H.TOL_DEC_E2E * float(np.abs(p.dual_coef).sum())
        flags = np.array([d[f"{name}_anomaly"] for d in detailed[:9]])
        scores = np.array([d[f"{name}_score"] for d in detailed[:9]])
        assert np.abs(scores - ref[f"{key}_score"]).max() <= tol
        sure = np.abs(ref[f"{key}_score"]) > tol
        assert sure.any() and np.array_equal(flags[sure], (ref[f"{key}_pred"] == -1)[sure]), name
        assert results["A"][f"{name}_anomaly_rate"] == np.sum(flags) / 9
        if sure.all():
            assert results["A"][f"{name}_anomaly_rate"] == np.mean(ref[f"{key}_pred"] == -1)
    df = pd.read_csv(tmp_path / "out" / "detailed_cell_results.csv")
    assert tuple(df.columns) == spec.DETAIL_COLUMNS and len(df) == 15
    sm = pd.read_csv(tmp_path / "out" / "screening_summary.csv", index_col=0)
    assert tuple(sm.columns) == spec.SUMMARY_COLUMNS


def test_full_size_properties(engine, weights, det):
    """Size-independent properties at BASELINE.json configs[2]'s full size (1,000,000 cells, device resident, the
    automatic 65,536-cell pass): determinism, shard-concatenation equality (the multi-GPU partition, section 8e, incl.
    an uneven 8-way split as configs[3] shards it), and oracle parity on a random sample."""
    import torch
    from cellscreen import dist as csdist
    n = 1_000_000
    x = torch.empty((n, 64, 64), dtype=torch.float32, device="cuda")
    engine.synth_crops(42, 0, x)
    engine.set_chunk(65536)
    r1 = engine.screen(x)
    r2 = engine.screen(x)
    for k in r1:
        assert torch.equal(r1[k], r2[k]), f"{k}: not deterministic"
    # contiguous shards concatenated == whole: 2 halves, and the 8 ranges shard_range gives a 1,000,003-cell job's first 1M
    h = n // 2
    ra, rb = engine.screen(x[:h]), engine.screen(x[h:])
    for k in r1:
        assert torch.equal(torch.cat([ra[k], rb[k]]), r1[k]), f"{k}: shard concat differs"
    parts = [engine.screen(x[lo:hi]) for lo, hi in (csdist.shard_range(n, r, 8) for r in range(8))]
    for k in r1:
        assert torch.equal(torch.cat([p[k] for p in parts]), r1[k]), f"{k}: 8-way shard concat differs"
    idx = np.sort(np.random.default_rng(0).choice(n, 64, replace=False))
    xs = np.stack([oracle.synth_crops(42, int(i), 1)[0] for i in idx])
    assert np.array_equal(x[torch.from_numpy(idx).cuda()].cpu().numpy(), xs)
    ref = oracle.screen(weights, None, det, xs, acc64=True)
    H.assert_rel(r1["mse"].cpu().numpy()[idx], ref["mse"], H.TOL_ERR_REL, "sampled mse")
    H.assert_rel(r1["mae"].cpu().numpy()[idx], ref["mae"], H.TOL_ERR_REL, "sampled mae")
    for name, p in (("cons", det.conservative), ("mod", det.moderate)):
        tol = H.TOL_DEC_E2E * np.abs(p.dual_coef).sum()
        assert np.abs(r1[f"{name}_score"].cpu().numpy()[idx] - ref[f"{name}_score"]).max() <= tol
        H.flags_agree(-r1[f"{name}_score"].cpu().numpy()[idx], r1[f"{name}_pred"].cpu().numpy()[idx], ref[f"{name}_dec"], ref[f"{name}_pred"], tol, name)
    rate = float((r1["cons_pred"] == -1).float().mean())
    assert 0.0 <= rate <= 1.0
    engine.set_chunk(0)


def test_plain_c_program_screens_through_the_abi(tmp_path, weights, det):
    """examples/screen_demo.c: gcc-built, no Python in the process -- loads the native model dir and screens."""
    import subprocess
    from test_host_logic import _build_c_demo
    d = str(tmp_path / "model")
    model_io.save_model_dir(d, weights, None, det)
    r = subprocess.run([_build_c_demo(), d, "300"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "reference-graph kernels" in r.stdout and "total_cells 300" in r.stdout


def test_scaler_is_bit_exact_through_one_hot_pca(weights, det):
    """The scaler inside the PCA kernels divides the float32 centred feature by the float64 scale_ in double and rounds
    once (detector.hip:67-68, 194-195); with one-hot PCA rows and zero mean projection the kernel's output IS the scaled
    feature, so it can be compared bit-for-bit with numpy's float32((x - center) / float64 scale) on two million values."""
    import copy
    rng = np.random.default_rng(123)
    F, C = 2048, 100
    d = copy.deepcopy(det)
    d.scaler_center = rng.normal(0.3, 0.2, F).astype(np.float32)
    d.scaler_scale = np.exp(rng.normal(0.0, 2.0, F)).astype(np.float64) * (1.0 + 2.0 ** -30)   # awkward divisors
    d.scaler_scale[:8] = [1.0, 3.0, 0.1, 7.0, 1e-3, 1e3, 1.0 / 3.0, 2.0 ** -20]
    comps = np.zeros((C, F), np.float32)
    cols = rng.choice(F, C, replace=False)
    cols[:8] = np.arange(8)
    comps[np.arange(C), cols] = 1.0
    d.pca_components = comps
    d.pca_mean = np.zeros(F, np.float32)
    d.pca_mean_proj = np.zeros(C, np.float32)
    e = Engine.from_weights(weights, None, d)
    try:
        x = rng.normal(0.3, 1.0, (20000, F)).astype(np.float32)
        x[:50, :8] = d.scaler_center[:8]                       # exact zeros after centring
        got = e.scaler_pca(x)
    finally:
        e.close()
    t = (x[:, cols] - d.scaler_center[cols]).astype(np.float32)
    want = (t.astype(np.float64) / d.scaler_scale[cols]).astype(np.float32)
    assert np.array_equal(got, want), f"{(got != want).sum()} of {got.size} scaled values differ"


def test_fused_conv6_conv7_error_matches_the_two_kernel_path(engine, weights):
    """cs_screen / cs_reconstruct without a reconstruction buffer run conv6 + conv7 + the error sums as ONE kernel (a6
    and the reconstruction never reach HBM; conv7 as a 32 -> 16 channel contraction plus a gather, hardware exp2 / rcp
    sigmoid); with a reconstruction buffer the two separate kernels run.  Same numbers up to fp32 summation order:
    1e-6 relative on MSE / MAE (the oracle bar for either is 1e-5)."""
    from oracle import oracle as orc
    for n in (1, 255, 256, 257, 1500):                     # below, at and above one cell per CU; a ragged tail
        x = synth.synth_crops(9, 1000, n)
        x[0] = 0.0
        if n > 2:
            x[1] = 1.0
            x[2, :, ::2] = 0.0                             # stripes: every phase / halo column of the gather matters
        _, mse_f, mae_f = engine.reconstruct(x, want_recon=False)
        rec, mse_u, mae_u = engine.reconstruct(x, want_recon=True)
        assert np.abs(mse_f - mse_u).max() <= 1e-6 * np.abs(mse_u).max()
        assert np.abs(mae_f - mae_u).max() <= 1e-6 * np.abs(mae_u).max()
        if n <= 257:
            ref = orc.cae_forward(weights, x, acc64=True, want=("mse", "mae"))
            assert np.abs(mse_f - ref["mse"]).max() <= 1e-5 * np.abs(ref["mse"]).max()
            assert np.abs(mae_f - ref["mae"]).max() <= 1e-5 * np.abs(ref["mae"]).max()


def test_automatic_chunk_by_input_kind(weights, det):
    """Without cs_model_set_chunk the pass size follows the input: 16,384 cells for host buffers (pipelined staging),
    as many as a ~28 GB workspace holds (65,536 for the reference graph) for device-resident crops.  Same results."""
    import torch
    e = Engine.from_weights(weights, None, det)
    try:
        assert e.info.chunk_cells == 65536
        x = synth.synth_crops(3, 500, 20000)                       # more than one host chunk, less than one device chunk
        r_host = e.screen(x)
        r_dev = e.screen(torch.from_numpy(x).cuda())
        for k in ("mse", "mae", "cons_score", "mod_score", "cons_pred", "mod_pred"):
            assert np.array_equal(np.asarray(r_host[k]), r_dev[k].cpu().numpy()), k
        e.set_chunk(4096)
        assert e.info.chunk_cells == 4096
        r_small = e.screen(x)
        assert np.array_equal(r_small["mse"], r_host["mse"]) and np.array_equal(r_small["mod_score"], r_host["mod_score"])
    finally:
        e.close()


def test_fused_conv1_conv2_every_output_of_more_than_two_residencies(weights):
    """conv1 + conv2 run as ONE kernel (conv12_fused.hip: conv2 as Winograd F(4x4,3x3), p1 rows produced into an LDS ring and
    never written to HBM; both contractions as two-term fp16 splits with precision="split16", on fp32 MFMAs with "fp32_exact")
    whenever p1 itself is not asked for.  Every element of p2 -- 600 cells = more than two cells per
    persistent workgroup (256 CUs x 1), so the ring wrap between cells, the crop prefetch and every workgroup are
    covered -- against the fp64-evaluated oracle at the layer bar, in both precisions, and against the two-kernel path
    (CS_DEBUG_NO_FUSE12: conv1 kernel -> p1 in HBM -> F(2x2,3x3) conv2).  p1 of the stand-alone conv1 kernel (what layer_output(0)
    and training use) gets the same full-coverage compare: 600 cells = 2,400 strips > 2 x its 1,024 resident workgroups."""
    n = 600
    x = synth.synth_crops(11, 7000, n)
    x[0] = 0.0
    x[1] = 1.0
    x[2, ::2] = 0.0                                        # row stripes: every row of the ring matters
    x[3, :, ::2] = 0.0                                     # column stripes: halo columns / patch columns
    x[4:40] = synth.blob_crops(5, 36)
    ref = oracle.cae_forward(weights, x, acc64=True, want=("features",), layers=True)["layers"]
    e = Engine.from_weights(weights)
    e2 = Engine.from_weights(weights, debug_flags=L.DEBUG_NO_FUSE12)
    e3 = Engine.from_weights(weights, precision="fp32_exact")        # the fused kernel on the fp32 matrix instructions
    try:
        p1 = e.layer_output(x, 0)
        p2 = e.layer_output(x, 1)
        p2_two = e2.layer_output(x, 1)
        p2_c1f32 = e3.layer_output(x, 1)
        # conv1 as a two-term fp16 split: 66 conv rows x 8 (x-tile, slice) x 2 MFMAs = 1,056 16-bit MFMAs per cell;
        # conv2 likewise: 36 points x 4 tile groups x 4 slices x 3 products = 1,728 more
        assert e.profile()["conv1_conv2_fused"]["bf16_mfma_per_cell"] == 1056 + 1728 and e.profile()["conv1_conv2_fused"]["mfma_per_cell"] == 0
        assert e3.profile()["conv1_conv2_fused"]["bf16_mfma_per_cell"] == 0 and e3.profile()["conv1_conv2_fused"]["mfma_per_cell"] > 4608
    finally:
        e.close(); e2.close(); e3.close()
    s1, s2 = np.abs(ref[0]).max(), np.abs(ref[1]).max()
    e1 = np.abs(p1.astype(np.float64) - ref[0]).max(axis=(1, 2, 3)) / s1
    ef = np.abs(p2.astype(np.float64) - ref[1]).max(axis=(1, 2, 3)) / s2
    et = np.abs(p2_two.astype(np.float64) - ref[1]).max(axis=(1, 2, 3)) / s2
    e3f = np.abs(p2_c1f32.astype(np.float64) - ref[1]).max(axis=(1, 2, 3)) / s2
    print("p1 max err / range %.2e; p2 fused %.2e (worst cell %d), fused on fp32 MFMAs %.2e, two-kernel %.2e"
          % (e1.max(), ef.max(), int(ef.argmax()), e3f.max(), et.max()))
    assert e3f.max() <= 1e-5 and not np.array_equal(p2, p2_c1f32)
    assert e1.max() <= 1e-5, f"conv1: cell {int(e1.argmax())}"
    assert et.max() <= 1e-5
    assert ef.max() <= 1e-5, f"fused conv1+conv2: cell {int(ef.argmax())} off by {ef.max():.3e} of the range"
    assert not np.array_equal(p2, p2_two), "the debug flag did not select a different kernel"
