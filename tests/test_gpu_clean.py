"""The segmenter's mask cleanup on the device (cs_segment_clean through cellscreen.segment) against the CPU restatement of
tests/clean_reference.py, which tests/test_clean_cpu.py holds to SciPy.

Every output is an integer (planes, counts, labels), so every comparison is np.array_equal: no tolerances."""
import ctypes as C

import numpy as np
import pytest

import background_reference as BR
import clean_reference as CR
import local_reference as LR
import segment_reference as R
import split_reference as SR
from cellscreen import _lib as L
from cellscreen import extract as X
from cellscreen import segment as S
from test_clean_cpu import disk_field
from test_local_cpu import SCENE_DELTA, SCENE_R, dim_cell_scene

pytestmark = pytest.mark.gpu

# csrc/segment.hip's own lengths: where the kernels take another path
CL_WORD = 64                                            # pixels of a packed word: one ballot of a wave (cl_open)
CL_TW, CL_TH = 256, 32                                  # a tile of cl_open: four words by 32 rows, one workgroup
CL_MAX_HALO = 30                                        # rows above and below a tile at r = 15 (2r); left and right: one word
SG_TW, SG_TH = 64, 16                                   # a tile of the union-find that the area step's components come from
SG_CHUNK = 1024                                         # pixels per workgroup of cl_count / cl_drop
SHAPES = [(1, 1), (1, 300), (300, 1), (37, 53), (17, 65), (3, 4096), (4096, 3), (257, 513)]
SHAPES += [(5, CL_WORD - 1), (5, CL_WORD), (CL_TH - 1, CL_TW - 1), (CL_TH, CL_TW), (CL_TH + 1, CL_TW + 1)]      # with (17, 65) and
#                                                         (257, 513): one short of, equal to and one past a word, a tile's
#                                                         width and its rows; 257 x 513 is one row and one column past 8 x 2 tiles
SHAPES += [(CL_TH + CL_MAX_HALO - 1, 70), (CL_TH + CL_MAX_HALO, 66), (CL_TH + CL_MAX_HALO + 1, 40)]     # the image ends one row
#                                                         inside, at the end of and one row past the first tile's lower halo at
#                                                         r = 15; at smaller r the halo of the second tile's upper side moves
SHAPES += [(2 * CL_TH + 3, CL_TW + CL_WORD + 1)]        # a second tile column that is one pixel past its first word
RADII = [1, 2, 3, 7, 8, 15]
AREAS = [1, 2, 5, 64, 200, 1 << 24]


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

    get.extractor = ext
    yield get
    ext.close()


def on_mask(segs, **kw):
    """A segmenter whose mask is the 0 / 1 input itself: pixel > 0, nothing filled."""
    return segs(threshold=0, fill_holes=False, **kw)


@pytest.fixture(scope="module")
def scenes():
    """Two speckled fields of bright and dim cells as one [2,512,512] uint16 stack, and their painted cells."""
    made = [dim_cell_scene(seed) for seed in range(2)]
    stack = np.stack([m[0] for m in made])
    stack.setflags(write=False)
    return stack, [m[1] for m in made]


LOCAL = dict(threshold="local", local_radius=SCENE_R, local_delta=SCENE_DELTA)


def as_tensor(imgs):
    import torch
    return torch.from_numpy(imgs.view(np.int16) if imgs.dtype == np.uint16 else imgs).to(torch.device("cuda", 0))


def serpentine(cut=False):
    """One line through every 64 x 16 tile of a 130 x 200 image: rows 8, 24, .. 120 and 129, joined at alternate ends.  cut:
    a pixel taken out at every tile border, which leaves pieces that stay inside one tile each."""
    H, W = 130, 200
    m = np.zeros((H, W), np.uint8)
    rows = list(range(8, H, SG_TH))[:8] + [H - 1]
    for j, y in enumerate(rows):
        m[y, :] = 1
        if j:
            m[rows[j - 1]:y + 1, (W - 1) if j % 2 else 0] = 1
    if cut:
        m[:, SG_TW::SG_TW] = 0
        m[SG_TH::SG_TH, :] = 0
        m[:, SG_TW - 1::SG_TW] = 0                         # and the pixel before it: no diagonal step across either
        m[SG_TH - 1::SG_TH, :] = 0
    return m


# ---- the opening ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_opening_equals_the_restatement(segs, shape):
    named = CR.mask_inputs(shape)                             # noise 0.5 / 0.9, bridged blobs, full, empty, checkerboard, two frames
    stack = np.stack([m for _, m in named])                   # as one batch
    for k in (1, 2):
        for r in RADII:
            got = on_mask(segs, open_radius=r, open_connectivity=k).clean_mask_batch(stack)
            assert got.dtype == np.uint8 and got.shape == stack.shape
            for i, (name, m) in enumerate(named):
                want = CR.opening(m, r, k)
                assert np.array_equal(got[i], want), (name, r, k, int((got[i] != want).sum()))


def test_opening_of_a_field_of_disks(segs):
    """Every (r, k) on an input it neither empties nor leaves alone, at a shape of several tiles."""
    x = np.zeros((200, 600), np.uint8)
    x[10:190, 5:185] = x[10:190, 300:480] = disk_field()
    x[100, :] = 1                                                     # a bridge across the tile columns
    for k in (1, 2):
        for r in RADII:
            got = on_mask(segs, open_radius=r, open_connectivity=k).clean_mask_batch(x[None])[0]
            want = CR.opening(x, r, k)
            assert want.any() and not np.array_equal(want, x) and np.array_equal(got, want), (r, k)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_both_pixel_types_through_a_fixed_threshold(segs, dtype):
    top = int(np.iinfo(dtype).max)
    img = np.random.default_rng(11).integers(0, top + 1, (2, 97, 300, 3)).astype(dtype)
    t = int(top * 0.3)
    for fill in (False, True):
        for kw in (dict(open_radius=1, open_connectivity=1), dict(min_area=30), dict(open_radius=1, min_area=30, connectivity=2)):
            s = segs(threshold=t, fill_holes=fill, **kw)
            got = s.clean_mask_batch(img, channel=1)
            for b in range(2):
                want = CR.clean(R.mask_of(img[b, :, :, 1], t, fill), kw.get("open_radius"), kw.get("open_connectivity", 2),
                                kw.get("min_area"), kw.get("connectivity", 1))
                assert want.any() and np.array_equal(got[b], want), (fill, kw, b)


# ---- the minimum area -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_min_area_equals_the_restatement(segs, shape):
    named = CR.mask_inputs(shape)
    stack = np.stack([m for _, m in named])
    for c in (1, 2):
        labs = [R.label_mask(m, c)[0] for m in stack]
        sizes = [np.bincount(lab.ravel()) for lab in labs]            # the reference's components, computed once
        for a in AREAS:
            got = on_mask(segs, min_area=a, connectivity=c).clean_mask_batch(stack)
            for i, (name, m) in enumerate(named):
                keep = sizes[i] >= a
                keep[0] = False
                assert np.array_equal(got[i], keep[labs[i]]), (name, a, c)
            if a == 1:
                assert np.array_equal(got, stack)                     # the identity
            if a == 1 << 24:
                assert not got.any()


def test_a_component_smaller_than_min_area_in_every_tile_survives_whole(segs):
    whole, pieces = serpentine(), serpentine(cut=True)
    total = int(whole.sum())
    per_tile = max(int(whole[y:y + SG_TH, x:x + SG_TW].sum()) for y in range(0, 130, SG_TH) for x in range(0, 200, SG_TW))
    assert all(whole[y:y + SG_TH, x:x + SG_TW].any() for y in range(0, 130, SG_TH) for x in range(0, 200, SG_TW))
    assert per_tile < 200 <= total and R.label_mask(whole, 1)[1] == 1
    n_pieces, biggest = R.label_mask(pieces, 2)[1], int(np.bincount(R.label_mask(pieces, 2)[0].ravel())[1:].max())
    assert n_pieces >= 9 * 4 and biggest < 200
    stack = np.stack([whole, pieces])
    for c in (1, 2):
        got = on_mask(segs, min_area=200, connectivity=c).clean_mask_batch(stack)
        assert np.array_equal(got[0], whole) and not got[1].any(), c
        got = on_mask(segs, min_area=total, connectivity=c).clean_mask_batch(stack)      # exact at a and a + 1
        assert np.array_equal(got[0], whole), c
        assert not on_mask(segs, min_area=total + 1, connectivity=c).clean_mask_batch(stack).any(), c
        got = on_mask(segs, min_area=biggest, connectivity=c).clean_mask_batch(stack)
        assert np.array_equal(got[1], CR.drop_small(pieces, biggest, c)) and got[1].any(), c


def test_counts_are_exact_at_a_minus_one_and_a(segs):
    for a in (2, 5, 64, 200):
        x = np.zeros((40, 260), np.uint8)
        x[3, 2:2 + a - 1] = 1                                         # a - 1 pixels: goes
        x[9, 2:2 + a] = 1                                             # a pixels: stays
        x[15:17, 2:2 + a] = 1                                         # 2a pixels over two rows: stays
        d = np.arange(min(a, 38))
        x[1 + d, 259 - d] |= (a <= 38)                                # a diagonal chain of a pixels, where it fits
        for c in (1, 2):
            got = on_mask(segs, min_area=a, connectivity=c).clean_mask_batch(x[None])[0]
            assert np.array_equal(got, CR.drop_small(x, a, c)), (a, c)
            assert not got[3, :220].any() and np.array_equal(got[9, :220], x[9, :220]) and np.array_equal(got[15:17, :220], x[15:17, :220])
            if a <= 38:
                assert bool(got[1, 259]) == (c == 2), (a, c)          # one component of a under 8 neighbours, a singletons under 4


# ---- the chain: labels, split, local, background, Otsu ---------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [1, 2])
def test_labels_are_those_of_the_cleaned_mask(segs, connectivity):
    x = np.zeros((2, 200, 600), np.uint8)
    x[0, 10:190, 5:185] = x[0, 10:190, 300:480] = disk_field()
    x[1] = CR.mask_inputs((200, 600))[1][1]                           # noise of density 0.9: some of it survives a 5 x 5 square
    for kw in (dict(open_radius=2), dict(min_area=30), dict(open_radius=1, open_connectivity=1, min_area=64)):
        for fill in (False, True):
            s = segs(threshold=0, fill_holes=fill, connectivity=connectivity, **kw)
            lab, n, thr = s.segment_batch(x)
            assert (thr == 0).all() and lab.dtype == np.int32
            for b in range(2):
                m = R.mask_of(x[b], 0, fill)
                cleaned = CR.clean(m, kw.get("open_radius"), kw.get("open_connectivity", 2), kw.get("min_area"), connectivity)
                elab, en = R.label_mask(cleaned, connectivity)
                assert en > 0 and int(n[b]) == en and np.array_equal(lab[b], elab), (kw, fill, b)
            t = s.last_timing()
            assert set(t) == {"threshold_ms", "label_ms", "open_ms", "min_area_ms"}
            assert (t["open_ms"] > 0.0) == ("open_radius" in kw) and (t["min_area_ms"] > 0.0) == ("min_area" in kw)


def test_split_touching_sees_the_cleaned_mask(segs):
    disks = SR.ten_disks()[0]
    rng = np.random.default_rng(5)
    img = (disks | (rng.random(disks.shape) < 0.03)).astype(np.uint8)          # the ten disks under speckle
    img[100, :] = 1                                                   # and a thread through the field
    s = segs(threshold=0, fill_holes=False, split_touching=True, open_radius=1, min_area=20)
    lab, n, thr, dist = s.segment_batch(img[None], return_distance=True)
    cleaned = CR.clean(img, 1, 2, 20, 1)
    elab, en, edq = SR.split_mask(cleaned > 0, 1, 3)
    assert en == 10 and int(n[0]) == en and int(thr[0]) == 0
    assert np.array_equal(lab[0], elab) and np.array_equal(dist[0], edq)
    assert set(s.last_timing()) == {"threshold_ms", "distance_ms", "seed_ms", "flood_ms", "open_ms", "min_area_ms"}
    raw = segs(threshold=0, fill_holes=False, split_touching=True).segment_batch(img[None])
    assert int(raw[1][0]) > 10 * en                                   # the speckle it would have flooded


def test_local_threshold_behind_the_cleanup(segs, scenes):
    stack, cells = scenes
    for kw in (dict(min_area=50), dict(open_radius=1)):
        s = segs(**LOCAL, **kw)
        mask = s.clean_mask_batch(stack)
        lab, n, thr = s.segment_batch(stack)
        assert (thr == -1).all()
        for b in range(2):
            m = R.ndimage.binary_fill_holes(LR.local_mask(stack[b], SCENE_R, SCENE_DELTA) > 0)
            cleaned = CR.clean(m, kw.get("open_radius"), 2, kw.get("min_area"), 1)
            elab, en = R.label_mask(cleaned, 1)
            assert np.array_equal(mask[b], cleaned) and en == 40 and int(n[b]) == en and np.array_equal(lab[b], elab), (kw, b)
            assert all(lab[b][y, x] > 0 for y, x, _, _ in cells[b])
        assert set(s.last_timing()) == {"threshold_ms", "label_ms", "local_median_ms", "local_ms", "open_ms", "min_area_ms"}
    _, n_raw, _ = segs(**LOCAL).segment_batch(stack)
    assert (n_raw > 800).all()


def test_cleanup_behind_the_background_correction(segs, scenes):
    stack, _ = scenes
    slope = (np.arange(512, dtype=np.int64) * 4)[None, None, :]
    imgs = np.minimum(stack + slope, 65535).astype(np.uint16)
    s = segs(background_radius=40, open_radius=2, min_area=50)
    lab, n, thr = s.segment_batch(imgs)
    mask = s.clean_mask_batch(imgs)
    _, _, thr_plain = segs(background_radius=40).segment_batch(imgs)
    assert np.array_equal(thr, thr_plain)
    for b in range(2):
        plane = BR.correct(imgs[b], 40, False)
        t = R.otsu(plane)
        cleaned = CR.clean(R.mask_of(plane, t, True), 2, 2, 50, 1)
        elab, en = R.label_mask(cleaned, 1)
        assert int(thr[b]) == t and np.array_equal(mask[b], cleaned) and int(n[b]) == en and np.array_equal(lab[b], elab), b


def test_otsu_thresholds_are_the_uncleaned_call_s(segs, scenes):
    stack, _ = scenes
    imgs = np.stack([stack[0], stack[1] // 2 + 100, stack[0] // 3]).astype(np.uint16)
    _, n0, thr0 = segs().segment_batch(imgs)
    lab, n, thr = segs(min_area=500).segment_batch(imgs)
    assert np.array_equal(thr, thr0) and len(set(thr.tolist())) == 3 and thr.dtype == np.int32
    for b in range(3):
        assert int(thr[b]) == R.otsu(imgs[b])
        elab, en = R.label_mask(CR.clean(R.mask_of(imgs[b], int(thr[b]), True), a=500), 1)
        assert int(n[b]) == en and np.array_equal(lab[b], elab)
    t = as_tensor(imgs)
    lab_d, n_d, thr_d = segs(min_area=500).segment_batch(t)
    assert np.array_equal(thr_d, thr0) and np.array_equal(n_d, n) and np.array_equal(lab_d.cpu().numpy(), lab)


# ---- the invariant: what the extraction returns -----------------------------------------------------------------------------------
def test_extraction_is_unchanged_by_its_own_area_bound_as_min_area(segs, scenes):
    stack, _ = scenes
    ext = segs.extractor
    assert X.REFERENCE_QC["min_area"] == 200
    t = as_tensor(stack.copy())
    lab0, n0, _ = segs(**LOCAL).segment_batch(t)
    lab1, n1, _ = segs(**LOCAL, min_area=200).segment_batch(t)
    assert (n1 == 40).all() and (n0 > 800).all()
    r0 = ext.extract_batch(t, lab0)
    cells0, image0, stats0, status0 = r0.cells.cpu().numpy(), r0.cell_image.copy(), X.region_stats(r0.regions), r0.status.copy()
    r1 = ext.extract_batch(t, lab1)
    assert len(stats0) > 0 and X.region_stats(r1.regions) == stats0
    assert np.array_equal(r1.cells.cpu().numpy().view(np.uint32), cells0.view(np.uint32))
    assert np.array_equal(r1.cell_image, image0) and np.array_equal(r1.status, status0)
    assert len(r1.regions) == 80 and len(r0.regions) == int(n0.sum())


def test_threshold_cell_extractor_passes_the_cleanup_through(tmp_path, scenes):
    stack, _ = scenes
    path = str(tmp_path / "plate.npy")
    np.save(path, stack[0])
    kw = dict(threshold="local", local_radius=SCENE_R, local_delta=SCENE_DELTA)
    plain, plain_stats = S.threshold_cell_extractor(**kw)(path)
    got, got_stats = S.threshold_cell_extractor(mask_min_area=200, **kw)(path)      # min_area stays the extraction's own rule
    assert len(plain) > 0 and len(got) == len(plain) and got_stats == plain_stats
    assert np.array_equal(np.stack(got).view(np.uint32), np.stack(plain).view(np.uint32))
    # both areas, apart: the mask's components below 300 px go, and the extraction's rule sits at 100
    got, got_stats = S.threshold_cell_extractor(open_radius=2, open_connectivity=1, mask_min_area=300, min_area=100, **kw)(path)
    want100, want100_stats = X.label_cell_extractor(lambda seg: R.label_mask(CR.clean(
        R.ndimage.binary_fill_holes(LR.local_mask(np.ascontiguousarray(seg), SCENE_R, SCENE_DELTA) > 0), 2, 1, 300, 1), 1)[0],
        min_area=100)(path)
    assert len(got) == len(want100) > 0 and got_stats == want100_stats
    assert np.array_equal(np.stack(got).view(np.uint32), np.stack(want100).view(np.uint32))
    assert len(got) < len(plain)                                      # cells of fewer than 300 px left with the speckle


# ---- transport ----------------------------------------------------------------------------------------------------------------
def test_device_tensors_in_and_out_and_two_runs(segs, scenes):
    import torch
    stack, _ = scenes
    t = as_tensor(stack.copy())
    for kw in (dict(open_radius=1, min_area=50, connectivity=2), dict(min_area=50, split_touching=True)):
        s = segs(**LOCAL, **kw)
        mask = s.clean_mask_batch(t)
        assert mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == stack.shape
        host = s.clean_mask_batch(stack)
        assert np.array_equal(mask.cpu().numpy(), host) and torch.equal(s.clean_mask_batch(t), mask)
        out_d, out_h, again = s.segment_batch(t), s.segment_batch(stack), s.segment_batch(t)
        assert out_d[0].is_cuda and np.array_equal(out_d[0].cpu().numpy(), out_h[0]) and torch.equal(out_d[0], again[0])
        assert np.array_equal(out_d[1], out_h[1]) and np.array_equal(out_d[1], again[1]) and np.array_equal(out_d[2], out_h[2])
        # the cleaned plane left on the device, labelled as a one-channel image at the fixed threshold 0, is the one-call form
        if "split_touching" not in kw:
            lab2, n2, _ = segs(threshold=0, fill_holes=False, connectivity=2).segment_batch(mask, channel=0)
            assert torch.equal(lab2, out_d[0]) and np.array_equal(n2, out_d[1])
    tm = s.last_timing()
    assert tm["min_area_ms"] > 0.0 and tm["open_ms"] == 0.0


def test_cleanup_off_is_the_segmenter_as_it_was(segs, scenes):
    stack, _ = scenes
    rng = np.random.default_rng(9)
    noise = rng.integers(0, 256, (2, 130, 200, 3)).astype(np.uint8)
    for kw in (dict(), dict(open_connectivity=1), dict(connectivity=2, fill_holes=False)):
        s = segs(**kw)
        assert s._clean is None
        ref_kw = {k: v for k, v in kw.items() if k != "open_connectivity"}
        for imgs in (stack, noise):
            lab, n, thr = s.segment_batch(imgs)
            elab, en, ethr = R.segment_batch(imgs, **ref_kw)
            assert np.array_equal(lab, elab) and np.array_equal(n, en) and np.array_equal(thr, ethr)
        assert set(s.last_timing()) == {"threshold_ms", "label_ms"}
        with pytest.raises(ValueError):
            s.clean_mask_batch(stack)


# ---- the C ABI with a device ------------------------------------------------------------------------------------------------------
def test_error_codes_with_a_handle():
    lib = L.load_library()
    h = C.c_void_p()
    assert lib.cs_preproc_create(0, C.byref(h)) == 0
    try:
        img = np.ones((1, 32, 32), np.uint16)
        out = np.full((1, 32, 32), 7, np.uint8)
        thr = np.full(1, 7, np.int32)
        par = L.CSSegmentParams()
        par.threshold_mode, par.threshold, par.connectivity, par.fill_holes = L.THRESH_FIXED, 0, 1, 0

        def clean(open_radius=1, open_connectivity=2, min_area=0):
            p = L.CSCleanParams()
            p.open_radius, p.open_connectivity, p.min_area = open_radius, open_connectivity, min_area
            return C.pointer(p)

        def call(cl, H=32, W=32):
            return lib.cs_segment_clean(h, img.ctypes.data, 1, 1, 0, 1, H, W, 0, C.byref(par), cl, out.ctypes.data, 0, thr.ctypes.data)

        for cl in (None, clean(0, 2, 0), clean(16), clean(-1), clean(1, 0), clean(1, 3), clean(1, 2, -1), clean(1, 2, (1 << 24) + 1)):
            assert call(cl) == -1                                     # CS_ERR_INVALID
        assert call(clean(), W=4097) == -6 and call(clean(), H=4097) == -6               # CS_ERR_UNSUPPORTED
        assert (out == 7).all() and (thr == 7).all()                  # nothing ran
        assert call(clean(15, 2, 1024)) == 0 and (out == 1).all() and int(thr[0]) == 0   # and the handle still works
        assert call(clean(15, 1, 0)) == 0 and out.sum() == 32 * 32 - 4 * 120             # the diamond rounds the four corners
        assert call(clean(0, 2, 1025)) == 0 and (out == 0).all()
        ms = [C.c_double(-1.0) for _ in range(3)]
        assert lib.cs_segment_clean_last_timing(h, *(C.byref(v) for v in ms)) == 0
        assert ms[0].value > 0.0 and ms[1].value == 0.0 and ms[2].value > 0.0
    finally:
        lib.cs_preproc_free(h)
