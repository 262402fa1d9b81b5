"""The segmenter's noise-adaptive threshold on the device (cs_segment_noise through cellscreen.segment) against the CPU
restatement of tests/noise_reference.py, which tests/test_noise_cpu.py holds to a slow form in exact rationals.

Every output is an integer (meshes, planes, labels, counts, thresholds), so every comparison is np.array_equal: no tolerances."""
import ctypes as C

import numpy as np
import pytest

import background_reference as BR
import clean_reference as CR
import noise_reference as NR
import segment_reference as R
import smooth_reference as MR
import split_intensity_reference as IR
import split_reference as SR
from cellscreen import _lib as L
from cellscreen import extract as X
from cellscreen import segment as S
from test_local_cpu import dim_cell_scene

pytestmark = pytest.mark.gpu

# T = 16: the smallest shapes that cross one tile, the absorbed remainder and a third node, each one short, equal and one past
SIDES = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49]
PAIRS = list(zip(SIDES, SIDES[3:] + SIDES[:3]))          # every side once as a height and once as a width, no square


@pytest.fixture(scope="module")
def segs():
    """ThresholdSegmenter per option set, made on demand, all on one handle and one stream: an extractor's."""
    made = {}
    ext = X.CellExtractor(0)

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            made[key] = S.ThresholdSegmenter(0, extractor=ext, **kw)
        return made[key]

    yield get
    ext.close()


@pytest.fixture(scope="module")
def scene():
    """The field of bright and dim cells (seed 0) and the restatement's labels at the defaults."""
    img, cells = dim_cell_scene(0)
    want = NR.segment(img)
    img.setflags(write=False)
    return img, cells, want


def as_tensor(imgs):
    import torch
    return torch.from_numpy(imgs.view(np.int16) if imgs.dtype == np.uint16 else imgs).to(torch.device("cuda", 0))


def field(shape, dtype, seed, slope=0.0):
    """[B,H,W]: a noisy background that differs from image to image, with a few bright blocks and single hot pixels."""
    rng = np.random.default_rng(seed)
    top = int(np.iinfo(dtype).max)
    B, H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty(shape, dtype)
    for b in range(B):
        f = top * (0.1 + 0.05 * b) + rng.normal(0.0, top * 0.01 * (b + 1), (H, W)) + slope * (xx + 2 * yy)
        for _ in range(max(1, H * W // 300)):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            f[y:y + int(rng.integers(1, 6)), x:x + int(rng.integers(1, 6))] += top * rng.uniform(0.02, 0.5)
        out[b] = np.clip(np.rint(f), 0, top).astype(dtype)
    return out


def blobs(shape, dtype, seed):
    """[B,H,W]: Gaussian blobs (two of them overlapping) and two overlapping flat disks on a noisy slope."""
    rng = np.random.default_rng(seed)
    top = int(np.iinfo(dtype).max)
    B, H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty(shape, dtype)
    for b in range(B):
        f = top * 0.1 + rng.normal(0.0, top * 0.004, (H, W)) + top * 0.0002 * xx
        centres = [(int(rng.integers(10, H - 10)), int(rng.integers(10, W - 10))) for _ in range(6)]
        centres.append((centres[0][0], min(centres[0][1] + 11, W - 8)))
        for cy, cx in centres:
            f += top * 0.4 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 3.0 ** 2))
        for cx in (W // 2 - 6, W // 2 + 7):                                             # two flat disks of radius 8 with a neck between
            f[(yy - H // 2) ** 2 + (xx - cx) ** 2 <= 64] += top * 0.3
        out[b] = np.clip(np.rint(f), 0, top).astype(dtype)
    return out


def check(segs, imgs, tile, noise_k=5.0, weak_k=None, noise_floor=1.0, connectivity=1):
    """Mesh and plane of the device against the restatement; returns the plane."""
    s = segs(threshold="noise", noise_tile=tile, noise_k=noise_k, weak_k=weak_k, noise_floor=noise_floor, connectivity=connectivity,
             fill_holes=False)
    k8, weak8, floor8 = NR.k8_of(noise_k), (None if weak_k is None else NR.k8_of(weak_k)), NR.k8_of(noise_floor)
    mesh, plane = s.noise_mesh_batch(imgs), s.noise_mask_batch(imgs)
    assert mesh.dtype == np.int32 and plane.dtype == np.uint8 and plane.shape == imgs.shape[:3]
    want_mesh = NR.mesh_batch(imgs, tile, floor8)
    assert mesh.shape == want_mesh.shape and np.array_equal(mesh, want_mesh), (imgs.shape, tile, np.argwhere(mesh != want_mesh)[:4])
    want = NR.noise_mask_batch(imgs, T=tile, k8=k8, weak8=weak8, floor8=floor8, connectivity=connectivity)
    assert np.array_equal(plane, want), (imgs.shape, tile, noise_k, weak_k, int((plane != want).sum()))
    return plane


# ---- shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PAIRS)
def test_tile_16_across_one_tile_the_remainder_and_a_third_node(segs, shape):
    seen = set()
    for dtype in (np.uint8, np.uint16):
        imgs = field((3,) + shape, dtype, 100 * shape[0] + shape[1])
        assert not np.array_equal(imgs[0], imgs[1]) or shape == (1, 1)
        seen |= set(np.unique(check(segs, imgs, 16)))
        for c in (1, 2):
            seen |= set(np.unique(check(segs, imgs, 16, 6.0, 3.0, connectivity=c)))
        seen |= set(np.unique(check(segs, imgs, 16, 1.5, 0.25, noise_floor=0.0)))
    assert seen == {0, 1}                                   # neither side of the rule is vacuous


@pytest.mark.parametrize("shape", [(511, 300), (512, 512), (767, 256)])
def test_tile_256(segs, shape):
    # 511 x 300 is one tile and 767 x 256 ends in a 511 x 256 one: the tiles that are read again in every pass
    imgs = field((2,) + shape, np.uint16, shape[0], slope=2.0)
    assert check(segs, imgs, 256).any()
    assert check(segs, imgs[:1], 256, 6.0, 3.0).any()
    assert check(segs, field((1,) + shape, np.uint8, shape[1]), 256, 4.0, 2.0).any()


def test_default_tile_on_the_scene(segs, scene, tmp_path):
    img, cells, (elab, en, _) = scene
    s = segs(threshold="noise")
    lab, n, thr = s.segment_batch(img[None])
    assert int(n[0]) == en and np.array_equal(lab[0], elab) and int(thr[0]) == -1
    assert all(lab[0][y, x] > 0 for y, x, _, _ in cells)                                # the 20 dim cells too
    assert np.array_equal(s.noise_mesh_batch(img[None])[0], NR.mesh(img, 64, 256))
    t = s.last_timing()
    assert set(t) == {"threshold_ms", "label_ms", "noise_mesh_ms", "noise_cut_ms", "noise_link_ms"}
    assert t["noise_mesh_ms"] > 0.0 and t["noise_cut_ms"] > 0.0 and t["noise_link_ms"] == 0.0
    weak = segs(threshold="noise", noise_k=6.0, weak_k=3.0)
    lab, n, thr = weak.segment_batch(img[None])
    wlab, wn, _ = NR.segment(img, 64, 1536, 768)
    assert int(n[0]) == wn == 40 and np.array_equal(lab[0], wlab) and weak.last_timing()["noise_link_ms"] > 0.0
    path = str(tmp_path / "plate.npy")
    np.save(path, img)
    got, got_stats = S.threshold_cell_extractor(threshold="noise", noise_k=6.0, weak_k=3.0)(path)
    want, want_stats = X.label_cell_extractor(lambda seg: NR.segment(np.ascontiguousarray(seg), 64, 1536, 768)[0])(path)
    assert len(got) == len(want) > 20 and got_stats == want_stats
    assert np.array_equal(np.stack(got).view(np.uint32), np.stack(want).view(np.uint32))


# ---- values that stress the selection -----------------------------------------------------------------------------------------
def stress_tiles(side_y, side_x):
    """Single-tile uint16 images: values on both sides of a byte border at the bottom and at the top of the range, two values,
    and more than half saturated."""
    rng = np.random.default_rng(side_y * 1000 + side_x)
    shape = (side_y, side_x)
    low = rng.choice(np.array([255, 256, 257], np.uint16), shape)
    high = rng.choice(np.array([0xFEFF, 0xFF00, 0xFFFF], np.uint16), shape)
    both = np.where(rng.random(shape) < 0.5, low, high).astype(np.uint16)
    two = np.where(rng.random(shape) < 0.5, 1000, 1300).astype(np.uint16)
    sat = np.where(rng.random(shape) < 0.6, 65535, rng.integers(0, 65536, shape)).astype(np.uint16)
    return np.stack([low, high, both, two, sat])


@pytest.mark.parametrize("tile,shape", [(16, (16, 16)), (16, (31, 31)), (64, (64, 64)), (64, (65, 64)), (64, (127, 127))])
def test_selection_on_single_tiles(segs, tile, shape):
    # one tile: the filter is the identity and the mesh is the tile's own pair.  64 x 64 is the largest tile that stays in
    # registers, 65 x 64 the smallest that does not
    imgs = stress_tiles(*shape)
    s = segs(threshold="noise", noise_tile=tile, noise_floor=0.0, fill_holes=False)
    mesh = s.noise_mesh_batch(imgs)
    assert mesh.shape == (5, 2, 1, 1)
    for b, x in enumerate(imgs):
        v = sorted(int(q) for q in x.ravel())
        r = (len(v) - 1) // 2
        dev = sorted(abs(q - v[r]) for q in v)[r]
        assert (int(mesh[b, 0, 0, 0]), int(mesh[b, 1, 0, 0])) == (256 * v[r], (dev * 97164) >> 8), (b, v[r], dev)
    check(segs, imgs, tile, 1.0, 0.5, noise_floor=0.0)
    u8 = np.stack([np.where(x > 40000, 255, x & 1).astype(np.uint8) for x in imgs] + [(imgs[4] >> 8).astype(np.uint8)])
    check(segs, u8, tile, 2.0)


def test_selection_in_every_tile_of_a_mesh(segs):
    rng = np.random.default_rng(5)
    tiles = stress_tiles(16, 16)
    img = np.concatenate([np.concatenate([tiles[int(rng.integers(0, 5))] for _ in range(5)], axis=1) for _ in range(4)], axis=0)
    check(segs, np.stack([img[:, :70], img[:, 5:75]]), 16, 2.0, 1.0)


def test_exact_tie_is_background(segs):
    for dtype, b in ((np.uint8, 100), (np.uint16, 30000)):
        img = np.full((1, 40, 56), b, dtype)
        img[0, 3, 5], img[0, 20, 30], img[0, 39, 55] = b + 5, b + 6, b + 6
        img[0, 17, 17] = b + 5
        plane = check(segs, img, 16)                        # MAD 0: sigma is the floor of one count, the cut b + 5
        assert plane.sum() == 2 and plane[0, 20, 30] == 1 and plane[0, 39, 55] == 1
        assert not check(segs, np.full((2, 33, 17), b, dtype), 16).any()                 # a constant image is all background


# ---- the weak rule ------------------------------------------------------------------------------------------------------------
def serpentine(strong=True):
    """130 x 200 uint16 on a constant background of 500 (sigma: the floor): one line 4 counts up through every 16 x 16 tile of
    the mesh and every 64 x 16 tile of the union-find, joined at alternate ends; its only pixel 7 counts up is its last."""
    H, W = 130, 200
    img = np.full((H, W), 500, np.uint16)
    rows = list(range(8, H, 16))[:8] + [H - 1]
    for j, y in enumerate(rows):
        img[y, :] = 504
        if j:
            img[rows[j - 1]:y + 1, (W - 1) if j % 2 else 0] = 504
    if strong:
        img[H - 1, W - 1] = 507
    return img


def test_weak_component_through_every_tile_and_no_flag_between_images(segs):
    first, second = serpentine(), serpentine(strong=False)
    for order in ((first, second), (second, first), (first, second, first, second)):
        imgs = np.stack(order)
        for c in (1, 2):
            plane = check(segs, imgs, 16, 6.0, 3.0, connectivity=c)
            for img, got in zip(order, plane):
                assert np.array_equal(got, (img > 500).astype(np.uint8) * int(img.max() == 507))
    assert int(check(segs, first[None], 16, 6.0, 3.0).sum()) > 9 * 200


# ---- transport ----------------------------------------------------------------------------------------------------------------
def test_numpy_equals_tensor_and_two_runs(segs, scene):
    import torch
    stack = np.stack([scene[0], dim_cell_scene(1)[0]])
    t = as_tensor(stack.copy())
    for kw in (dict(), dict(noise_k=6.0, weak_k=3.0, connectivity=2), dict(noise_tile=128, noise_k=4.0, min_area=20)):
        s = segs(threshold="noise", **kw)
        mask = s.noise_mask_batch(t)
        assert mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == stack.shape
        host = s.noise_mask_batch(stack)
        assert host.any() and np.array_equal(mask.cpu().numpy(), host) and torch.equal(s.noise_mask_batch(t), mask)
        mesh = s.noise_mesh_batch(t)
        assert np.array_equal(mesh, s.noise_mesh_batch(stack)) and np.array_equal(mesh, s.noise_mesh_batch(t))
        out_d, out_h, again = s.segment_batch(t), s.segment_batch(stack), s.segment_batch(t)
        assert out_d[0].is_cuda and np.array_equal(out_d[0].cpu().numpy(), out_h[0]) and torch.equal(out_d[0], again[0])
        for k in (1, 2):
            assert np.array_equal(out_d[k], out_h[k]) and np.array_equal(out_d[k], again[k])
        assert (out_d[2] == -1).all() and s.last_timing() == s.last_timing()
    chan = np.stack([stack[0]] * 3 + [stack[1]], axis=-1)[None]                         # [1,H,W,4]: channel 2 by default, 3 on request
    s = segs(threshold="noise")
    assert np.array_equal(s.noise_mask_batch(chan)[0], s.noise_mask_batch(stack)[0])
    assert np.array_equal(s.noise_mask_batch(as_tensor(chan.copy()), channel=3).cpu().numpy()[0], s.noise_mask_batch(stack)[1])


# ---- the stages in front and behind -------------------------------------------------------------------------------------------
def test_with_the_other_stages(segs):
    imgs = blobs((2, 96, 160), np.uint16, 3)
    noise = dict(threshold="noise", noise_tile=32, noise_k=6.0, weak_k=3.0)
    ref = dict(T=32, k8=1536, weak8=768)
    fill = R.ndimage.binary_fill_holes

    def run(**kw):
        s = segs(**noise, **kw)
        out = s.segment_batch(imgs, return_distance=kw.get("split_touching", False))
        assert (out[2] == -1).all()
        return out

    got = run(smooth_sigma=1.5)
    for b, raw in enumerate(imgs):
        elab, en, _ = NR.segment(MR.smooth_sigma(raw, 1.5), **ref)
        assert en >= 2 and int(got[1][b]) == en and np.array_equal(got[0][b], elab)
    got = run(background_radius=12)
    for b, raw in enumerate(imgs):
        elab, en, _ = NR.segment(BR.correct(raw, 12, False), **ref)
        assert en >= 2 and int(got[1][b]) == en and np.array_equal(got[0][b], elab)
    speckled = dict(threshold="noise", noise_tile=32, noise_k=2.5)
    got = segs(**speckled, min_area=12).segment_batch(imgs)
    for b, raw in enumerate(imgs):
        filled = fill(NR.noise_mask(raw, 32, 640) > 0)
        elab, en = R.label_mask(CR.clean(filled, None, 2, 12, 1) > 0, 1)
        assert 2 <= en < R.label_mask(filled, 1)[1] and int(got[1][b]) == en and np.array_equal(got[0][b], elab)
    got = run(split_touching=True)
    for b, raw in enumerate(imgs):
        m = fill(NR.noise_mask(raw, **ref) > 0)
        elab, en, edq = SR.split_mask(m, 1, 3)
        assert en > R.label_mask(m, 1)[1] and int(got[1][b]) == en and np.array_equal(got[0][b], elab) and np.array_equal(got[3][b], edq)
    got = run(split_touching=True, split_by="intensity", smooth_sigma=1.5)
    for b, raw in enumerate(imgs):
        x = MR.smooth_sigma(raw, 1.5)
        m = fill(NR.noise_mask(x, **ref) > 0)
        elab, en, ehq = IR.split_intensity(m, x, 1, 16, 0)                              # the guide is the plane the stage saw
        assert en > R.label_mask(m, 1)[1] and int(got[1][b]) == en and np.array_equal(got[0][b], elab) and np.array_equal(got[3][b], ehq)


def test_stage_off_is_the_segmenter_as_it_was(segs, scene):
    img = scene[0]
    for kw in (dict(), dict(threshold=900, connectivity=2)):
        s = segs(**kw)
        assert s._noise is None
        lab, n, thr = s.segment_batch(img[None])
        elab, en, ethr = R.segment(img, **kw)
        assert np.array_equal(lab[0], elab) and int(n[0]) == en and int(thr[0]) == ethr
        assert set(s.last_timing()) == {"threshold_ms", "label_ms"}
        with pytest.raises(ValueError):
            s.noise_mask_batch(img[None])
        with pytest.raises(ValueError):
            s.noise_mesh_batch(img[None])


# ---- the C ABI with a device ------------------------------------------------------------------------------------------------------
def test_error_codes_with_a_handle():
    lib = L.load_library()
    h = C.c_void_p()
    assert lib.cs_preproc_create(0, C.byref(h)) == 0
    try:
        img = np.full((1, 32, 32), 50, np.uint16)
        img[0, 16, 16] = 56
        out = np.full((1, 32, 32), 7, np.uint8)
        mesh = np.full((1, 2, 2, 2), 7, np.int32)

        def par(tile=16, k8=1280, weak8=-1, floor8=256, conn=1, r2=0):
            p = L.CSNoiseParams()
            p.tile, p.k8, p.weak_k8, p.floor8, p.connectivity, p.reserved[2] = tile, k8, weak8, floor8, conn, r2
            return C.pointer(p)

        def call(p, H=32, W=32, m=mesh.ctypes.data):
            return lib.cs_segment_noise(h, img.ctypes.data, 1, 1, 0, 1, H, W, 0, p, out.ctypes.data, 0, m)

        for p in (None, par(tile=8), par(tile=48), par(tile=512), par(k8=0), par(k8=16384), par(weak8=0), par(weak8=1281), par(weak8=-2),
                  par(floor8=-1), par(floor8=4095 * 256 + 1), par(weak8=640, conn=3), par(r2=1)):
            assert call(p) == -1                                      # CS_ERR_INVALID
        assert call(par(), W=4097) == -6 and call(par(), H=4097) == -6               # CS_ERR_UNSUPPORTED
        assert (out == 7).all() and (mesh == 7).all()                 # nothing ran
        assert call(par()) == 0 and out.sum() == 1 and out[0, 16, 16] == 1           # and the handle still works
        assert (mesh[0, 0] == 50 * 256).all() and (mesh[0, 1] == 256).all()
        assert call(par(conn=3), m=None) == 0 and out.sum() == 1      # without a weak rule the connectivity is not read
        assert call(par(k8=1536)) == 0 and out.sum() == 0             # six counts up ties at k = 6
        assert call(par(k8=1536, weak8=1535, conn=2)) == 0 and out.sum() == 0         # weak, and no strong pixel
        ms = [C.c_double(-1.0) for _ in range(3)]
        assert lib.cs_segment_noise_last_timing(h, *(C.byref(v) for v in ms)) == 0
        assert ms[0].value > 0.0 and ms[1].value > 0.0 and ms[2].value > 0.0
    finally:
        lib.cs_preproc_free(h)
