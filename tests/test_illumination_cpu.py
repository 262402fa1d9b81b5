"""CPU tests of the flat-field correction (cs_illum_tile_stats, cs_illum_reduce, cs_illum_apply, cellscreen/illumination.py,
DESIGN 3zj): the restatement of tests/illumination_reference.py against a slow form in exact rationals that shares no code with
it, its optional filters against SciPy, a plate with a known function, the golden file, the package's host side against the
restatement, and the wrapper's and the C ABI's refusals before any device work.  Integers are compared exactly."""
import ctypes as C
import os
from fractions import Fraction
from math import floor

import numpy as np
import pytest
from scipy import ndimage as ndi

import illumination_caps as IC
import illumination_reference as IR
import smooth_reference as SR
from cellscreen import _lib as L
from cellscreen import illumination as IL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_illumination.npz")


# ---- the slow form: ranks from sorted(), the function per pixel in Fractions, the quotient as floor(x + 1/2) ---------------------
def slow_tiles(n, T):
    m = max(1, n // T)
    return [(i * T, n if i == m - 1 else (i + 1) * T) for i in range(m)]


def slow_rank(values, num, den):
    v = sorted(int(x) for x in values)
    return v[(num * (len(v) - 1)) // den]


def slow_function(F8c, tiles_y, tiles_x, y, x):
    """The function at pixel (y, x) in 1/256 counts, a Fraction: linear between the tile centres (s + e - 1) / 2 and beyond the
    outer ones, along each axis in turn."""
    def along(tiles, p):
        if len(tiles) == 1:
            return 0, 0, Fraction(0)
        c = [Fraction(s + e - 1, 2) for s, e in tiles]
        i = 0
        while i < len(tiles) - 2 and p >= c[i + 1]:
            i += 1
        return i, i + 1, (p - c[i]) / (c[i + 1] - c[i])
    j0, j1, ty = along(tiles_y, y)
    i0, i1, tx = along(tiles_x, x)
    top = (1 - tx) * int(F8c[j0][i0]) + tx * int(F8c[j0][i1])
    bottom = (1 - tx) * int(F8c[j1][i0]) + tx * int(F8c[j1][i1])
    return (1 - ty) * top + ty * bottom


def slow_correct(images, T, q, rule, offset, floor_, normalize, pedestal):
    x = images if images.ndim == 4 else images[..., None]
    B, H, W, Cn = x.shape
    ty, tx = slow_tiles(H, T), slow_tiles(W, T)
    top = 255 if x.dtype == np.uint8 else 65535
    out = np.zeros_like(x)
    clipped = np.zeros((B, Cn, 2), np.int64)
    F8 = [[[0] * len(tx) for _ in ty] for _ in range(Cn)]
    for c in range(Cn):
        for j, (y0, y1) in enumerate(ty):
            for i, (x0, x1) in enumerate(tx):
                per_image = [slow_rank(x[b, y0:y1, x0:x1, c].ravel(), *q) for b in range(B)]
                value = (2 * sum(per_image) + B) // (2 * B) if rule == "mean" else slow_rank(per_image, *rule)
                F8[c][j][i] = 256 * max(value - offset[c], floor_)
        flat = sorted(v for row in F8[c] for v in row)
        G = {"mean": floor(Fraction(sum(flat), len(flat)) + Fraction(1, 2)), "median": flat[(len(flat) - 1) // 2], "max": flat[-1],
             "min": flat[0]}[normalize] if isinstance(normalize, str) else normalize
        for y in range(H):
            for xx in range(W):
                f = max(slow_function(F8[c], ty, tx, y, xx), Fraction(256 * floor_))
                for b in range(B):
                    v = pedestal[c] + floor(Fraction((int(x[b, y, xx, c]) - offset[c]) * G) / f + Fraction(1, 2))
                    clipped[b, c, 0] += v < 0
                    clipped[b, c, 1] += v > top
                    out[b, y, xx, c] = min(max(v, 0), top)
    return out.reshape(images.shape), clipped, np.array(F8, np.int32)


SLOW_CASES = [  # shape, dtype, q, rule, offset, floor, normalize, pedestal
    ((2, 1, 1), np.uint8, (1, 2), (1, 2), [0], 1, "mean", [0]),
    ((3, 40, 40), np.uint16, (1, 2), (1, 2), [100], 1, "mean", [100]),
    ((2, 17, 33, 2), np.uint8, (0, 1), "mean", [3, 200], 2, "min", [0, 9]),
    ((4, 31, 16), np.uint16, (1, 4), (1, 1), [0], 1, "max", [5]),
    ((3, 15, 40, 3), np.uint16, (65535, 65536), (0, 1), [0, 7, 65535], 4095, "median", [65535, 0, 1]),
    ((2, 32, 39), np.uint8, (1, 1), (1, 3), [1], 1, 777, [2]),
]


@pytest.mark.parametrize("case", range(len(SLOW_CASES)))
def test_restatement_equals_the_slow_form(case):
    shape, dt, q, rule, offset, floor_, normalize, pedestal = SLOW_CASES[case]
    if shape[1] * shape[2] == 1:
        images = np.array([[[200]], [[3]]], dt)                          # one pixel: one tile, one node on either axis
    else:
        images = IR.golden_field(shape, dt, seed=50 + case)              # case 2: every v of channel 1 is below its offset
    out, clipped, F8, G8 = IR.correct(images, 16, q, rule, offset, floor_, False, None, normalize, pedestal)
    out2, clipped2, F82 = slow_correct(images, 16, q, rule, offset, floor_, normalize, pedestal)
    assert F8.dtype == np.int32 and np.array_equal(F8, F82)
    assert out.dtype == images.dtype and out.shape == images.shape and np.array_equal(out, out2)
    assert np.array_equal(clipped, clipped2)


def test_extrapolation_is_linear_and_the_floor_holds():
    """Outside the outer centres w1 leaves 0..D; a function that falls steeply goes negative there and N is pinned at its floor."""
    i0, i1, w0, w1, D = IR.axis_weights(49, 16)
    assert w1.min() == -15 and w1[0] == -15 and w0[0] == D[0] + 15 and (w0 + w1 == D).all()
    assert w1[-1] == 2 * 48 - (2 * 16 + 15) and w1[-1] > D[-1] and w0[-1] < 0     # the last tile is 17 wide: D = 33
    F8 = np.array([[256 * 4000, 256 * 10]], np.int32)                   # 1 x 2 nodes on 16 x 32
    N, D2 = IR.maps(F8, 16, 32, 16, floor=3)
    assert (N[:, -8:] == 256 * 3 * D2[:, -8:]).all() and (N[:, :8] > 256 * 4000 * D2[:, :8]).all()
    Nc, _ = IR.maps(F8, 16, 32, 16, floor=3, constant=True)
    assert (Nc[:, :8] == 256 * 4000 * D2[:, :8]).all() and (Nc[:, -8:] == 256 * 10 * D2[:, -8:]).all()
    # the widest last tile: 767 pixels at T = 256, |w| < 5 T and the sums inside their bounds
    _, _, w0, w1, D = IR.axis_weights(767, 256)
    assert D.max() == 767 and w1.max() == 1277 and w0.min() == -510 and max(abs(w0).max(), abs(w1).max()) < 5 * 256


def test_mesh_filters_equal_scipy():
    rng = np.random.default_rng(5)
    for shape in ((1, 1), (1, 7), (2, 2), (5, 9), (16, 16), (3, 40)):
        F = (256 * rng.integers(1, 65536, shape)).astype(np.int64)
        assert np.array_equal(IR.filter3(F), ndi.median_filter(F, size=3, mode="nearest")), shape
        for sigma in (0.5, 1.0, 2.5, 16.0):                              # 16: radius 64, above every side here
            w = SR.smooth_weights(sigma)
            got = IR.smooth_mesh(F, w, 1)
            want = ndi.gaussian_filter(F.astype(np.float64), sigma, mode="reflect", truncate=4.0)
            assert np.abs(got - want).max() <= SR.bound(w, sigma, int(F.max())), (shape, sigma)
    assert (IR.smooth_mesh(np.full((3, 4), 256 * 77, np.int64), SR.smooth_weights(2.0), 1) == 256 * 77).all()     # a fixed point
    assert (IR.smooth_mesh(np.full((3, 4), 256, np.int64), SR.smooth_weights(2.0), 9) == 256 * 9).all()           # floored again


# ---- a plate with a known function ------------------------------------------------------------------------------------------------
SCENES = [(0, 8, 0.43), (1, 30, 0.6), (2, 30, 0.43)]                     # seed, cells per field, the vignette at the far corner
MARGIN = 0.05            # measured on the restatement: 4.17 %, 2.11 %, 4.08 % at roll-offs of 57 %, 40 %, 57 %; rounded up


@pytest.mark.parametrize("seed,cells,edge", SCENES)
def test_a_plate_with_a_known_function(seed, cells, edge):
    """16 fields of 256 x 256, T = 32, cells elsewhere in every field, a dark level of 100 and noise of sigma 12 under an off-centre
    vignette.  The estimate stays within MARGIN of the truth everywhere, the corrected plate's own estimate is flat within it, and
    the margin is at most a fifth of the roll-off.  The constant continuation and each default-off filter are worse in the outer
    half-tile band: the defaults rest on that."""
    T, bg, dark = 32, 2000.0, 100
    fields, truth = IR.plate(seed, 16, 256, cells, edge, dark, 12.0, bg)
    assert MARGIN <= (1.0 - edge) / 5.0
    stack = IR.tile_stats(fields, T)
    band = np.ones((256, 256), bool)
    band[T // 2:-(T // 2), T // 2:-(T // 2)] = False

    def error(constant=False, **kw):
        F8 = IR.reduce(stack, (1, 2), dark, 1, **kw)
        N, D = IR.maps(F8[0], 256, 256, T, 1, constant)
        return np.abs(N / D / 256.0 / (bg * truth) - 1.0)

    e = error()
    print(f"seed {seed}: worst {e.max():.4f}, border band {e[band].max():.4f}, inside {e[~band].max():.4f}")
    assert e.max() <= MARGIN
    for name, other in (("constant", error(constant=True)), ("mesh median", error(mesh_median=True)),
                        ("gaussian", error(weights=SR.smooth_weights(1.0)))):
        print(f"  {name}: border band {other[band].max():.4f}")
        assert other[band].max() > e[band].max(), name
    F8 = IR.reduce(stack, (1, 2), dark, 1)
    G8 = IR.scale(F8)
    out, clipped = IR.apply(fields, F8, G8, T, dark)
    again = IR.reduce(IR.tile_stats(out, T), (1, 2), dark, 1)
    flat = np.abs(again[0] / G8[0] - 1.0).max()
    print(f"  corrected plate: its own estimate within {flat:.4f} of G8")
    assert flat <= MARGIN and not clipped.any()


def test_golden_file():
    with np.load(GOLDEN) as z:
        assert int(z["n_cases"]) == len(IR.GOLDEN_CASES)
        for i, (case, (out, clipped, F8, G8)) in enumerate(zip(IR.GOLDEN_CASES, IR.golden_outputs())):
            assert (z[f"image_{i}"] == IR.golden_field(case[0], case[1])).all(), i
            assert z[f"out_{i}"].dtype == out.dtype and (z[f"out_{i}"] == out).all(), i
            assert (z[f"clipped_{i}"] == clipped).all() and (z[f"F8_{i}"] == F8).all() and z[f"G8_{i}"].tolist() == G8, i


# ---- the package's host side ------------------------------------------------------------------------------------------------------
def _function(shape=(40, 70), T=16, Cn=2, dt=np.uint16, seed=3):
    rng = np.random.default_rng(seed)
    my, mx = max(1, shape[0] // T), max(1, shape[1] // T)
    F8 = (256 * rng.integers(50, 4000, (Cn, my, mx))).astype(np.int32)
    return IL.IlluminationFunction(tile=T, shape=shape, channels=Cn, dtype=dt, F8=F8, G8=[IL.scale_of(F8[c]) for c in range(Cn)],
                                   offset=[7] * Cn, floor=2, n_images=5,
                                   params=dict(quantile=(1, 2), across="mean", mesh_median=False, smooth_sigma=0.0, normalize="mean"))


def test_host_side_equals_the_restatement():
    import cellscreen
    assert cellscreen.IlluminationCorrector is IL.IlluminationCorrector and cellscreen.IlluminationFunction is IL.IlluminationFunction
    assert IL.smooth_weights(1.0) == SR.smooth_weights(1.0)
    fn = _function()
    for how in IL.NORMALIZE + (12345,):
        assert [IL.scale_of(fn.F8[c], how) for c in range(2)] == IR.scale(fn.F8, how)
    for n, T in ((1, 16), (15, 16), (16, 16), (33, 16), (49, 16), (767, 256), (300, 64)):
        for a, b in zip(IL._axis(n, T), IR.axis_weights(n, T)):
            assert np.array_equal(a, b), (n, T)
    for c in range(2):
        N, D = IR.maps(fn.F8[c], 40, 70, 16, 2)
        N2, D2 = fn.maps(c)
        assert np.array_equal(N, N2) and np.array_equal(D, D2)
        assert np.array_equal(fn.gain_map(c), fn.G8[c] * D.astype(np.float64) / N.astype(np.float64)) and fn.gain_map(c).dtype == np.float64
    rp = IL.reduce_params(3, (1, 3), [1, 2, 3], 9, True, 2.5)
    assert (rp.a_num, rp.a_den, rp.mean, list(rp.offset), rp.floor, rp.mesh_median, rp.radius) == (1, 3, 0, [1, 2, 3, 0], 9, 1, 10)
    assert list(rp.weights)[:11] == SR.smooth_weights(2.5) and not any(list(rp.weights)[11:]) and list(rp.reserved) == [0, 0]
    rp = IL.reduce_params(1, "mean")
    assert (rp.mean, rp.radius, list(rp.offset), rp.floor, rp.mesh_median) == (1, 0, [0, 0, 0, 0], 1, 0)
    assert C.sizeof(L.CSIllumReduceParams) == 4 * (10 + 65 + 2) and C.sizeof(L.CSIllumApplyParams) == 4 * 16


def test_save_and_load_round_trip(tmp_path):
    fn = _function()
    path = str(tmp_path / "plate.npz")
    fn.save(path)
    back = IL.IlluminationFunction.load(path)
    assert (back.tile, back.shape, back.channels, back.dtype, back.G8, back.offset, back.floor, back.n_images, back.params) == \
           (fn.tile, fn.shape, fn.channels, fn.dtype, fn.G8, fn.offset, fn.floor, fn.n_images, fn.params)
    assert back.F8.dtype == np.int32 and np.array_equal(back.F8, fn.F8)
    with np.load(path, allow_pickle=False) as z:                         # a plain .npz: nothing pickled
        assert set(z.files) == {"tile", "shape", "channels", "dtype", "F8", "G8", "offset", "floor", "n_images", "params"}


def test_python_refuses_bad_arguments_before_a_handle_exists():
    import torch
    ic = IL.IlluminationCorrector(0)
    img = np.zeros((2, 40, 70, 2), np.uint16)
    fn = _function()
    for image, kw, exc in (
            (img.astype(np.float32), {}, TypeError), (img.astype(np.int16), {}, TypeError), (list(img), {}, TypeError),
            (img[0, 0], {}, ValueError), (img[..., None], {}, ValueError), (img[:0], {}, ValueError), (img[:, :, ::2], {}, ValueError),
            (np.zeros((2, 8, 12, 5), np.uint8), {}, ValueError), (np.zeros((1, 2, 4097), np.uint8), {}, ValueError),
            (torch.zeros((2, 8, 12), dtype=torch.uint8), {}, ValueError), (torch.zeros((2, 8, 12), dtype=torch.float32), {}, TypeError),
            (img, dict(tile=8), ValueError), (img, dict(tile=48), ValueError), (img, dict(tile=512), ValueError), (img, dict(tile=64.0), TypeError),
            (img, dict(tile=True), TypeError), (img, dict(quantile=0.5), TypeError), (img, dict(quantile=(1, 0)), ValueError),
            (img, dict(quantile=(3, 2)), ValueError), (img, dict(quantile=(-1, 2)), ValueError), (img, dict(quantile=(1, 65537)), ValueError),
            (img, dict(quantile=(1.0, 2)), TypeError), (img, dict(quantile=(True, 2)), TypeError), (img, dict(quantile=(1, 2, 3)), TypeError)):
        with pytest.raises(exc):
            ic.tile_stats_batch(image, **kw)
        with pytest.raises(exc):
            ic.add_batch(image, **kw)
    with pytest.raises(ValueError):
        ic.finish()                                                      # nothing was added
    for kw, exc in ((dict(across="median"), ValueError), (dict(across=(2, 1)), ValueError), (dict(across=0.5), TypeError),
                    (dict(offset=-1), ValueError), (dict(offset=65536), ValueError), (dict(offset=[1]), ValueError), (dict(offset=1.0), TypeError),
                    (dict(offset=[1, True]), TypeError), (dict(floor=0), ValueError), (dict(floor=4096), ValueError), (dict(floor=1.5), TypeError),
                    (dict(floor=True), TypeError), (dict(mesh_median=1), TypeError), (dict(smooth_sigma=float("nan")), ValueError),
                    (dict(smooth_sigma=-1.0), ValueError), (dict(smooth_sigma=16.5), ValueError), (dict(smooth_sigma="1"), TypeError),
                    (dict(smooth_sigma=True), TypeError)):
        with pytest.raises(exc):
            IL.reduce_params(2, **kw)
    for how, exc in (("mode", ValueError), (0, ValueError), (1 << 24, ValueError), (2.0, TypeError), (True, TypeError)):
        with pytest.raises(exc):
            IL.scale_of(fn.F8[0], how)
    for image, kw, exc in (
            (img, dict(function=None), TypeError), (img[..., :1], {}, ValueError), (img.astype(np.uint8), {}, ValueError),
            (img[:, :39], {}, ValueError), (img, dict(pedestal=-1), ValueError), (img, dict(pedestal=65536), ValueError),
            (img, dict(pedestal=[1]), ValueError), (img, dict(pedestal=1.0), TypeError), (img, dict(return_clipped=1), TypeError),
            (img, dict(out=np.zeros((2, 40, 70, 2), np.uint8)), ValueError), (img, dict(out=np.zeros((1, 40, 70, 2), np.uint16)), ValueError),
            (img, dict(out=torch.zeros((2, 40, 70, 2), dtype=torch.uint8)), ValueError)):
        with pytest.raises(exc):
            ic.apply_batch(np.ascontiguousarray(image), **dict(dict(function=fn), **kw))
    for bad, exc in ((np.zeros((2, 2, 2, 2), np.int64), TypeError), (np.zeros((2, 2, 2), np.int32), ValueError),
                     (np.zeros((2, 5, 2, 2), np.int32), ValueError), (np.zeros((2, 2, 4, 2), np.int32)[:, :, ::2], TypeError)):
        with pytest.raises(exc):
            ic.reduce_stack(bad, IL.reduce_params(2))
    for kw, exc in ((dict(tile=48), ValueError), (dict(dtype=np.float32), TypeError), (dict(F8=fn.F8.astype(np.int64)), TypeError),
                    (dict(F8=fn.F8[:, :1]), ValueError), (dict(F8=fn.F8 * 0 + 255), ValueError), (dict(F8=fn.F8 * 0 + (1 << 24)), ValueError),
                    (dict(G8=[1]), ValueError), (dict(G8=[0, 1]), ValueError), (dict(offset=[0, 65536]), ValueError), (dict(floor=0), ValueError)):
        base = dict(tile=16, shape=(40, 70), channels=2, dtype=np.uint16, F8=fn.F8, G8=fn.G8, offset=fn.offset, floor=2)
        with pytest.raises(exc):
            IL.IlluminationFunction(**dict(base, **kw))
    assert ic._pre is None and ic.n_images == 0
    with pytest.raises(ValueError):
        IL.IlluminationCorrector(1, extractor=type("E", (), {"device_id": 0})())
    ic.close()


# ---- the caps ---------------------------------------------------------------------------------------------------------------------
def test_caps_are_read_from_the_sources_and_every_tool_has_its_scenes():
    """What tests/label_caps.py's guard does for the tools before these: a cs_illum_* entry point that runs a batch on the handle
    is one that opens the shared state through il_begin, each is a tool of tests/illumination_caps.py, and each tool and each cap
    has a scene that tests/test_gpu_illumination_caps.py runs."""
    c = IC.read_caps()
    assert c == IC.CAPS == dict(kIlMaxChannels=4, kIlMaxImages=16384, kIlMaxMesh=256, kIlMaxStack=1 << 28)
    assert (IL.MAX_CHANNELS, IL.MAX_IMAGES, IL.MAX_STACK, IL.MAX_SIDE, IL.MAX_BATCH) == \
           (c["kIlMaxChannels"], c["kIlMaxImages"], c["kIlMaxStack"], IC.MAX_SIDE, IC.MAX_BATCH)
    assert c["kIlMaxMesh"] == IC.MAX_SIDE // min(IL.TILES)
    assert sorted(t["entry"] for t in IC.TOOLS.values()) == IC.declared_entry_points() and len(IC.TOOLS) == 3
    assert IC.declared_entry_points() == sorted(n for n in L.SIGNATURES if n.startswith("cs_illum_") and "_last_" not in n)
    for t in IC.TOOLS.values():
        assert set(t["caps"]) <= set(c)
    met = {s["cap"] for s in IC.SCENES.values()}
    assert met == {"kMaxSide", "kMaxBatch", "kIlMaxChannels", "kIlMaxImages", "kIlMaxMesh"}        # kIlMaxStack: its refusal, above
    assert {t for s in IC.SCENES.values() for t in s["tools"]} == set(IC.TOOLS)
    for s in IC.SCENES.values():
        assert ("image" in s) != ("stack" in s)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
NAMES = {"cs_illum_tile_stats": 13, "cs_illum_reduce": 10, "cs_illum_apply": 15, "cs_illum_last_timing": 4}
INVALID, UNSUPPORTED, NO_DEVICE = -1, -6, -4
_BUF = np.full(4096, 300, np.int32)                                      # never written: every call here ends before the device


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2 and lib.cs_profile_kernel_count() == 13
    raw = C.CDLL(L.LIB_PATH)
    for name, n_args in NAMES.items():
        assert hasattr(raw, name) and hasattr(lib, name) and name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == n_args, name
    with open(os.path.join(ROOT, "include", "cellscreen.h")) as f:
        text = " ".join(f.read().split())
    assert ("int cs_illum_tile_stats(cs_preproc *p, const void *image, int pixel_type, int32_t channels, int32_t batch, int32_t height, "
            "int32_t width, int in_kind, int32_t tile, int32_t q_num, int32_t q_den, int32_t *mesh, int out_kind);") in text
    assert ("int cs_illum_reduce(cs_preproc *p, const int32_t *stack, int32_t n, int32_t channels, int32_t m_y, int32_t m_x, int in_kind, "
            "const cs_illum_reduce_params *params, int32_t *f8, int out_kind);") in text
    assert ("int cs_illum_apply(cs_preproc *p, const void *image, int pixel_type, int32_t channels, int32_t batch, int32_t height, "
            "int32_t width, int kind, const int32_t *f8, int32_t m_y, int32_t m_x, int mesh_kind, const cs_illum_apply_params *params, "
            "void *out, int64_t *clipped /* or NULL */);") in text
    assert "int cs_illum_last_timing(const cs_preproc *p, double *stats_ms, double *reduce_ms, double *apply_ms);" in text
    assert "#define CS_ABI_VERSION 2 " in text and "#define CS_ILLUM_MAX_RADIUS 64 " in text and "#define CS_ILLUM_MAX_IMAGES 16384 " in text


def _stats(lib, image=True, mesh=True, pt=1, Cn=1, B=1, H=40, W=40, kind=0, okind=0, tile=16, q=(1, 2)):
    p = _BUF.ctypes.data
    rc = lib.cs_illum_tile_stats(None, p if image else None, pt, Cn, B, H, W, kind, tile, q[0], q[1], p if mesh else None, okind)
    return int(rc), lib.cs_last_error().decode()


def _rparams(a=(1, 2), mean=0, offset=(0, 0, 0, 0), floor_=1, median=0, weights=None, radius=None, reserved=(0, 0)):
    rp = L.CSIllumReduceParams()
    rp.a_num, rp.a_den, rp.mean, rp.floor, rp.mesh_median = a[0], a[1], mean, floor_, median
    for c in range(4):
        rp.offset[c] = offset[c]
    for k, v in enumerate(weights or []):
        rp.weights[k] = v
    rp.radius = (len(weights) - 1 if weights else 0) if radius is None else radius
    rp.reserved[0], rp.reserved[1] = reserved
    return rp


def _reduce(lib, stack=True, params=True, f8=True, n=3, Cn=1, my=2, mx=3, kind=0, okind=0, values=None, **kw):
    buf = _BUF if values is None else np.array(values, np.int32)
    p = buf.ctypes.data
    rp = _rparams(**kw)
    rc = lib.cs_illum_reduce(None, p if stack else None, n, Cn, my, mx, kind, C.byref(rp) if params else None, _BUF.ctypes.data if f8 else None, okind)
    return int(rc), lib.cs_last_error().decode()


def _apply(lib, image=True, f8=True, params=True, out=True, clipped=False, pt=1, Cn=1, B=1, H=40, W=40, kind=0, mkind=0, my=2, mx=2, tile=16,
           floor_=1, g8=(256, 256, 256, 256), offset=(0, 0, 0, 0), pedestal=(0, 0, 0, 0), reserved=(0, 0), values=None):
    buf = _BUF if values is None else np.array(values, np.int32)
    p = _BUF.ctypes.data
    ap = L.CSIllumApplyParams()
    ap.tile, ap.floor = tile, floor_
    for c in range(4):
        ap.g8[c], ap.offset[c], ap.pedestal[c] = g8[c], offset[c], pedestal[c]
    ap.reserved[0], ap.reserved[1] = reserved
    rc = lib.cs_illum_apply(None, p if image else None, pt, Cn, B, H, W, kind, buf.ctypes.data if f8 else None, my, mx, mkind,
                            C.byref(ap) if params else None, p if out else None, p if clipped else None)
    return int(rc), lib.cs_last_error().decode()


NULL = "NULL argument"
PIX = "pixel_type must be CS_PIX_U8 or CS_PIX_U16"
W1 = SR.smooth_weights(1.0)
WEIGHTS = "weights must be non-negative with w[0] >= 1, 0 beyond the radius and w[0] + 2 * sum(w[1..radius]) == 65536"

# (overrides, status, text): the rules in their order, one broken or two at once
STATS_CASES = [
    (dict(image=False), INVALID, NULL), (dict(mesh=False), INVALID, NULL), (dict(pt=2), INVALID, PIX), (dict(pt=-1), INVALID, PIX),
    (dict(kind=2), INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE"),
    (dict(okind=-1), INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE"),
    (dict(Cn=0), INVALID, "channels 0: must be >= 1"), (dict(B=0), INVALID, "batch 0, height 40, width 40: all must be >= 1"),
    (dict(H=0), INVALID, "batch 1, height 0, width 40: all must be >= 1"), (dict(W=-1), INVALID, "batch 1, height 40, width -1: all must be >= 1"),
    (dict(tile=8), INVALID, "tile 8: a power of two in 16..256"), (dict(tile=48), INVALID, "tile 48: a power of two in 16..256"),
    (dict(tile=512), INVALID, "tile 512: a power of two in 16..256"), (dict(tile=0), INVALID, "tile 0: a power of two in 16..256"),
    (dict(q=(1, 0)), INVALID, "quantile 1 / 0: need 0 <= q_num <= q_den <= 65536"),
    (dict(q=(3, 2)), INVALID, "quantile 3 / 2: need 0 <= q_num <= q_den <= 65536"),
    (dict(q=(-1, 2)), INVALID, "quantile -1 / 2: need 0 <= q_num <= q_den <= 65536"),
    (dict(q=(1, 65537)), INVALID, "quantile 1 / 65537: need 0 <= q_num <= q_den <= 65536"),
    (dict(Cn=5), UNSUPPORTED, "channels 5: at most 4 are corrected per call (split the stack)"),
    (dict(H=4097), UNSUPPORTED, "image 4097x40: sides above 4096 are not supported"),
    (dict(W=4097), UNSUPPORTED, "image 40x4097: sides above 4096 are not supported"),
    (dict(B=65536), UNSUPPORTED, "batch 65536: at most 65535 images per call"),
    (dict(image=False, pt=2), INVALID, NULL), (dict(pt=2, kind=2), INVALID, PIX), (dict(tile=8, Cn=5), INVALID, "tile 8: a power of two in 16..256"),
    (dict(q=(3, 2), H=4097), INVALID, "quantile 3 / 2: need 0 <= q_num <= q_den <= 65536"),
    (dict(Cn=5, H=4097), UNSUPPORTED, "channels 5: at most 4 are corrected per call (split the stack)"),
]
REDUCE_CASES = [
    (dict(stack=False), INVALID, NULL), (dict(params=False), INVALID, NULL), (dict(f8=False), INVALID, NULL),
    (dict(kind=2), INVALID, "in_kind / out_kind must be CS_MEM_HOST or CS_MEM_DEVICE"), (dict(Cn=0), INVALID, "channels 0: must be >= 1"),
    (dict(n=0), INVALID, "n 0, mesh 2 x 3: all must be >= 1"), (dict(my=0), INVALID, "n 3, mesh 0 x 3: all must be >= 1"),
    (dict(mean=2), INVALID, "mean 2: 0 or 1"), (dict(a=(2, 1)), INVALID, "across 2 / 1: need 0 <= a_num <= a_den <= 65536"),
    (dict(a=(0, 0)), INVALID, "across 0 / 0: need 0 <= a_num <= a_den <= 65536"),
    (dict(offset=(0, 0, -1, 0)), INVALID, "offset[2] = -1: must be 0..65535"), (dict(offset=(65536, 0, 0, 0)), INVALID, "offset[0] = 65536: must be 0..65535"),
    (dict(floor_=0), INVALID, "floor 0 outside 1..4095"), (dict(floor_=4096), INVALID, "floor 4096 outside 1..4095"),
    (dict(median=2), INVALID, "mesh_median 2: 0 or 1"), (dict(radius=65), INVALID, "radius 65 outside 0..64"), (dict(radius=-1), INVALID, "radius -1 outside 0..64"),
    (dict(weights=[65535, 1]), INVALID, WEIGHTS), (dict(weights=W1[:-1] + [-1]), INVALID, WEIGHTS), (dict(weights=W1, radius=2), INVALID, WEIGHTS),
    (dict(weights=[0, 32768]), INVALID, WEIGHTS),
    (dict(reserved=(0, 1)), INVALID, "cs_illum_reduce_params.reserved must be 0"), (dict(reserved=(1, 0)), INVALID, "cs_illum_reduce_params.reserved must be 0"),
    (dict(values=[0, 5, 65536, 1, 1, 1], n=1), INVALID, "a value of the stack is outside 0..65535"),
    (dict(values=[0, 5, -1, 1, 1, 1], n=1), INVALID, "a value of the stack is outside 0..65535"),
    (dict(Cn=5), UNSUPPORTED, "channels 5: at most 4 are corrected per call (split the stack)"),
    (dict(my=257), UNSUPPORTED, "mesh 257 x 3: at most 256 nodes along an axis"), (dict(n=16385), UNSUPPORTED, "n 16385: at most 16384 meshes per call"),
    (dict(n=16384, Cn=4, my=256, mx=256, kind=1), UNSUPPORTED, "n 16384 x channels 4 x mesh 256 x 256: the stack is capped at 268435456 values"),
    (dict(a=(2, 1), mean=1, floor_=0), INVALID, "floor 0 outside 1..4095"),                   # the mean does not read the rank
    (dict(mean=2, n=0), INVALID, "n 0, mesh 2 x 3: all must be >= 1"), (dict(floor_=0, n=16385), INVALID, "floor 0 outside 1..4095"),
    (dict(reserved=(0, 1), Cn=5), INVALID, "cs_illum_reduce_params.reserved must be 0"),
]
APPLY_CASES = [
    (dict(image=False), INVALID, NULL), (dict(f8=False), INVALID, NULL), (dict(params=False), INVALID, NULL), (dict(out=False), INVALID, NULL),
    (dict(pt=2), INVALID, PIX), (dict(kind=2), INVALID, "kind / mesh_kind must be CS_MEM_HOST or CS_MEM_DEVICE"),
    (dict(mkind=-1), INVALID, "kind / mesh_kind must be CS_MEM_HOST or CS_MEM_DEVICE"), (dict(Cn=0), INVALID, "channels 0: must be >= 1"),
    (dict(B=0), INVALID, "batch 0, height 40, width 40: all must be >= 1"), (dict(tile=24), INVALID, "tile 24: a power of two in 16..256"),
    (dict(floor_=0), INVALID, "floor 0 outside 1..4095"), (dict(g8=(0, 1, 1, 1)), INVALID, "g8[0] = 0: must be in [1, 2^24)"),
    (dict(g8=(1, 1 << 24, 1, 1), Cn=2), INVALID, "g8[1] = 16777216: must be in [1, 2^24)"),
    (dict(offset=(0, 0, 0, 65536)), INVALID, "offset[3] = 65536: must be 0..65535"), (dict(pedestal=(-1, 0, 0, 0)), INVALID, "pedestal[0] = -1: must be 0..65535"),
    (dict(reserved=(1, 0)), INVALID, "cs_illum_apply_params.reserved must be 0"),
    (dict(Cn=5), UNSUPPORTED, "channels 5: at most 4 are corrected per call (split the stack)"),
    (dict(H=4097, my=256), UNSUPPORTED, "image 4097x40: sides above 4096 are not supported"), (dict(B=65536), UNSUPPORTED, "batch 65536: at most 65535 images per call"),
    (dict(my=3), INVALID, "mesh 3 x 2: an image of 40 x 40 has 2 x 2 tiles of side 16"),
    (dict(H=15, my=2), INVALID, "mesh 2 x 2: an image of 15 x 40 has 1 x 2 tiles of side 16"),
    (dict(values=[256, 255, 256, 256]), INVALID, "a value of the function is outside [256, 2^24)"),
    (dict(values=[256, 256, 256, 1 << 24]), INVALID, "a value of the function is outside [256, 2^24)"),
    (dict(image=False, pt=2), INVALID, NULL), (dict(tile=24, Cn=5), INVALID, "tile 24: a power of two in 16..256"),
    (dict(reserved=(0, 1), my=3), INVALID, "cs_illum_apply_params.reserved must be 0"), (dict(Cn=5, my=3), UNSUPPORTED, "channels 5: at most 4 are corrected per call (split the stack)"),
]


def test_c_abi_refuses_bad_arguments_before_the_handle():
    lib = L.load_library()
    for fn, cases in ((_stats, STATS_CASES), (_reduce, REDUCE_CASES), (_apply, APPLY_CASES)):
        for over, status, text in cases:
            assert fn(lib, **over) == (status, text), (fn.__name__, over)
    assert lib.cs_illum_last_timing(None, None, None, None) == INVALID


def test_a_null_handle_reports_no_device_for_valid_arguments():
    lib = L.load_library()
    no_dev = lib.cs_device_count() <= 0
    want = NO_DEVICE if no_dev else INVALID                               # no handle: no device here, else a NULL handle
    for over in (dict(), dict(pt=0, Cn=4), dict(tile=256, H=4096, W=4096), dict(q=(0, 1)), dict(q=(65536, 65536)), dict(kind=1, okind=1), dict(B=65535, H=1, W=1)):
        assert _stats(lib, **over)[0] == want, over
    for over in (dict(), dict(mean=1, a=(9, 1)), dict(weights=W1), dict(weights=SR.smooth_weights(16.0), median=1), dict(n=16384, kind=1), dict(Cn=4, offset=(1, 2, 3, 65535)),
                 dict(floor_=4095)):
        assert _reduce(lib, **over)[0] == want, over
    for over in (dict(), dict(clipped=True), dict(g8=((1 << 24) - 1, 0, 0, 0)), dict(Cn=4, pedestal=(65535, 0, 1, 2)), dict(H=15, my=1), dict(tile=256, H=767, W=256, my=2, mx=1),
                 dict(kind=1, mkind=1, values=[0, 0, 0, 0])):            # a device function is not read on the host
        assert _apply(lib, **over)[0] == want, over
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            IL.IlluminationCorrector(0).tile_stats_batch(np.zeros((1, 40, 40), np.uint8), tile=16)
        assert ei.value.status == NO_DEVICE
        with pytest.raises(L.CellScreenError) as ei:
            IL.IlluminationCorrector(0).apply_batch(np.zeros((2, 40, 70, 2), np.uint16), _function())
        assert ei.value.status == NO_DEVICE
