"""CPU proofs about the scenes of tests/extract_scenes.py: each reaches the loop or the limit of csrc/extract.hip that
tests/test_gpu_extract_sweep.py runs it for, by the scene's own arithmetic; a scene that drifts off its target fails here.
Then the restatement's eccentricity: from closed-form sums, and against the eigvalsh evaluation on the gallery."""
import numpy as np
import pytest

import extract_reference as R
import extract_scenes as S


def _bboxes(lab):
    """{id: (h, w)} of one label plane."""
    out = {}
    for i in np.unique(lab)[1:]:
        rr, cc = np.nonzero(lab == i)
        out[int(i)] = (int(rr.max() - rr.min()) + 1, int(cc.max() - cc.min()) + 1)
    return out


def test_mirrored_constants_are_the_library_s():
    from cellscreen import _labels
    from cellscreen import extract as X
    assert S.MAX_SLOTS == X.MAX_SLOTS and S.MAX_BATCH == _labels.MAX_BATCH and S.PLANE == _labels.MAX_SIDE


@pytest.mark.parametrize("M,per,empty", [(1023, 1, 1), (1024, 1, 0), (1025, 2, 511), (2047, 2, 0), (2048, 2, 0), (2049, 3, 341),
                                         (3001, 3, 23)])
def test_slot_table_scenes_give_scan_threads_more_than_one_slot(M, per, empty):
    assert M in S.SLOT_MAX_LABELS
    img, lab, qc = S.slot_table_scene(M)
    assert lab.shape == (1, 128, 512) and int(lab.max()) == M           # used as given: one image, max_label = M < the caps
    assert S.scan_per(M) == per and S.scan_empty_threads(M) == empty
    ids = set(np.unique(lab)[1:].tolist())
    absent = set(range(1, M + 1)) - ids
    assert len(absent) >= M // 7 - 15 and all(i % 7 == 0 for i in absent)           # empty slots all along the table
    squares = S.slot_square_ids(M)
    assert 10 <= len(squares) <= 15 and {1, M} <= set(squares) <= ids
    box = _bboxes(lab[0])
    assert all(box[i] == (12, 12) for i in squares) and all(box[i] == (2, 2) for i in ids - set(squares))
    # passing squares in the last slot of one scan thread and the first of the next, for several threads
    pairs = [(a, b) for a, b in zip(squares, squares[1:]) if b == a + 1 and a % per == 0]
    assert len(pairs) >= 4, pairs
    for a, b in pairs:
        t = a // per
        assert S.scan_run(t - 1, M)[1] - 1 == a - 1 and S.scan_run(t, M)[0] == b - 1
    regs = R.regions(lab[0, :40], img[0, :40], qc)                      # the band of squares and the first block rows
    assert [r["label"] for r in regs if r["failed"] == 0] == squares


def test_straddle_scene_runs_cross_both_image_boundaries():
    img, lab, qc = S.straddle_scene()
    n = S.STRADDLE_PER_IMAGE
    assert lab.shape == (3, 400, 400) and [int(lab[b].max()) for b in range(3)] == [n, n, n]
    nslots = 3 * n
    assert nslots == 2883 and S.scan_per(nslots) == 3 and n % 3 != 0
    assert S.scan_straddles(nslots, n) == [320, 640]                    # runs [960, 963) and [1920, 1923)
    assert len(np.unique(lab[0])) == n + 1 and len(np.unique(lab[2])) == n + 1
    assert tuple(np.unique(lab[1])[1:]) == S.STRADDLE_MIDDLE_IDS        # ~950 empty slots in the middle of the table
    # the straddling runs hold passing regions on both sides: ids 961 | 1, 2 and 960, 961 | 1
    assert {1, 2, 960, 961} <= set(S.STRADDLE_MIDDLE_IDS)
    assert _bboxes(lab[2])[500] == (40, 6)
    regs = R.regions(lab[2, 190:260], img[2, 190:260], qc)
    assert [r["failed"] for r in regs if r["label"] == 500] == [0] and R.image_status(regs) == R.IMAGE_NO_CELLS


@pytest.mark.parametrize("top_id", [64, 65])
def test_cap_scene_reaches_the_grid_and_batch_caps(top_id):
    img, lab, qc = S.cap_scene(top_id)
    B = S.MAX_BATCH
    assert lab.shape == (B, 8, 8) and img.shape == (B, 8, 8) and int(lab.max()) == top_id
    if top_id == 64:
        nslots = B * 64
        assert nslots == 4194240 <= S.MAX_SLOTS                          # used as given
        assert S.grid_rounds(nslots) == 4 and S.scan_per(nslots) == 4096
    else:
        assert B * top_id > S.MAX_SLOTS                                  # the wrapper relabels: at most 2 ids per image
        assert max(len(np.unique(p)) - 1 for p in S.cap_prototypes(top_id)[1]) == 2
        assert S.grid_rounds(B * 2) == 1
    assert S.status_rounds(B) == 64
    p = S.cap_prototype_of()
    covered = p // S.CAP_VARIANTS == 3
    assert covered[B - 1] and 1900 <= covered.sum() <= 2100               # the last image yields a crop: about 2,000 cells
    assert set(p.tolist()) == set(range(4 * S.CAP_VARIANTS))
    pimg, plab = S.cap_prototypes(top_id)
    for k in range(len(plab)):
        crops, regs, st = R.extract(plab[k], pimg[k], qc)
        assert st == R.IMAGE_OK and len(crops) == (1 if k // S.CAP_VARIANTS == 3 else 0)
        assert all(c.shape == (8, 8) for c in crops)


def test_status_scene_differs_beyond_the_first_scan_round():
    img, lab, qc = S.status_scene()
    B = S.STATUS_BATCH
    assert lab.shape == (B, 16, 16) and S.status_rounds(B) == 2
    st = [R.extract(lab[b], img[b], qc)[2] for b in range(1020, B)]
    assert set(st[4:]) == {R.IMAGE_OK, R.IMAGE_NO_CELLS}                 # images 1024..1099
    assert S.scan_per(B * int(lab.max())) == 4


def test_gallery_holds_every_degenerate_region():
    lab = S.gallery_labels()
    H, W = S.GALLERY_HW
    assert lab.shape == (H, W) and S.region_lds_bytes(H) < S.LDS_DEFAULT
    box = _bboxes(lab)
    assert len(box) == 18
    hs, ws = {h for h, _ in box.values()}, {w for _, w in box.values()}
    assert {1, 2, 3} <= hs and 1 in ws and {64, 65, 129} <= ws            # h < 4; the column loop's 64 / 65 / 129
    assert box[18] == (H, W)                                              # the frame: the bbox is the image
    assert box[13] == (46, 126) and (lab == 13).sum() == 2                # most rows of the window are empty
    branches = {"l1 == 0": 0, "l2 <= 0": 0, "sqrt": 0}
    for i in box:
        rad, l1, l2 = R.inertia_eigenvalues(*S.moment_sums(*np.nonzero(lab == i)))
        branches["l1 == 0" if l1 == 0.0 else "l2 <= 0" if l2 <= 0.0 else "sqrt"] += 1
    assert branches["l1 == 0"] == 1 and branches["l2 <= 0"] >= 5 and branches["sqrt"] >= 8, branches
    # the triangle's hypotenuse: its edge midpoints are collinear, so centres lie exactly on the hull
    img, labs, qc = S.gallery_scene(np.uint8)
    regs = {r["label"]: r for r in R.regions(labs[0], img[0], qc)}
    assert regs[11]["area"] == 40 * 41 // 2 and regs[11]["convex_area"] == regs[11]["area"]
    assert all(r["failed"] == 0 for r in regs.values()) and R.image_status(list(regs.values())) == R.IMAGE_NO_CELLS
    default = {r["label"]: r["failed"] for r in R.regions(labs[0], img[0], None)}
    assert len(set(default.values())) >= 6                                # the failed bits differ per region


def test_flush_scene_touches_every_edge_of_the_last_image():
    img, lab, qc = S.flush_scene()
    H, W = S.FLUSH_HW
    assert lab.shape == (2, H, W) and img.shape == (2, H, W, 3) and qc["border"] == 0
    crops, regs, st = R.extract(lab[1], img[1, ..., 1], qc)
    assert st == R.IMAGE_OK and len(crops) == len(regs) == 8 and all(c.shape == (16, 16) for c in crops)
    assert sum(r["minr"] == 0 for r in regs) == 3 and sum(r["maxr"] == H for r in regs) == 3
    assert sum(r["minc"] == 0 for r in regs) == 3 and sum(r["maxc"] == W for r in regs) == 3
    assert any(r["maxr"] == H and r["maxc"] == W for r in regs)          # the last pixel of the allocation is in a crop


def test_tall_and_wide_scenes_reach_the_lds_and_loop_limits():
    _, lab, _ = S.tall_scene()
    H, W = S.TALL_HW
    assert S.region_lds_bytes(H) == 81936 > S.LDS_DEFAULT
    box = _bboxes(lab[0])
    assert box == {1: (4096, 61), 2: (4096, 1)} and box[1][0] > 256
    assert -(-H // S.EX_THREADS) == 16                                    # rounds of the convex-count loop
    rr, cc = np.nonzero(lab[0] == 1)
    left = np.full(H, W)
    np.minimum.at(left, rr, cc)
    assert left[0] == left[-1] == 40 and left.min() == 0
    assert len(np.flatnonzero(np.diff(left) != 0)) == 80                  # a convex edge of 40 steps down and 40 up:
    assert S.left_chain_length(lab[0], 1) == 62                           # the left chain keeps 62 points (a rectangle's: 4)
    _, lab, _ = S.wide_scene()
    assert S.region_lds_bytes(S.WIDE_HW[0]) < S.LDS_DEFAULT
    assert _bboxes(lab[0]) == {5: (1, 4096)} and 4096 // 64 == 64         # rounds of the column loop; pack_pt's largest x + 1 = 8192
    assert 2 * (4096 - 1) + 1 + 1 == 8192


def test_fan_scene_keeps_a_long_chain():
    """Andrew's chain keeps a point per change of slope.  The number of slopes a convex lattice edge can take grows only with
    the cube root of its box's area, so several hundred points need a box of thousands of pixels both ways, which the
    restatement does not count in seconds: the fan keeps 102 points, the tall scene 62."""
    _, lab, _ = S.fan_scene()
    assert _bboxes(lab[0]) == {3: (201, 2530)} and (lab == 3).sum() == 402
    assert S.left_chain_length(lab[0], 3) == 102
    assert S.region_lds_bytes(S.FAN_HW[0]) < S.LDS_DEFAULT


@pytest.mark.parametrize("h,w", [(1024, 1024), (1025, 1024), (1024, 1025)])
def test_sides_scenes_sit_on_the_side_rule(h, w):
    _, lab, _ = S.sides_scene(h, w)
    assert lab.shape == (1, 1100, 1100) and S.region_lds_bytes(1100) < S.LDS_DEFAULT
    assert _bboxes(lab[0]) == {7: (h, w)} and (lab == 7).sum() == 256 and h > 256


def test_plane_scenes_carry_the_largest_operands():
    n = S.PLANE * S.PLANE
    assert S.region_lds_bytes(S.PLANE) == 81936 > S.LDS_DEFAULT
    sx, sxx = (n // 2) * 65535, (n // 2) * 65535 ** 2                      # 'halves'
    assert 2 ** 77 < n * sxx - sx * sx < 2 ** 78 < n * sxx < 2 ** 80
    assert float(sx) / float(n) == 32767.5 and (float(n * sxx - sx * sx) / float(n * n)) ** 0.5 == 32767.5
    s = S.rectangle_sums(S.PLANE, S.PLANE)
    assert 2 ** 69 < s[0] * s[3] < 2 ** 71                                 # N * S2 of the moments
    assert R.eccentricity_from_sums(*s) == 0.0
    e = R.eccentricity_from_sums(*S.rectangle_sums(S.PLANE, S.PLANE // 2))
    assert abs(e - (1.0 - (2048.0 ** 2 - 1.0) / (4096.0 ** 2 - 1.0)) ** 0.5) <= 1e-15


@pytest.mark.parametrize("h,w", [(1, 1), (1, 2), (2, 1), (1, 70), (3, 3), (4, 64), (5, 65), (3, 129), (20, 40), (70, 7)])
def test_eccentricity_from_closed_form_sums_is_the_pixel_lists(h, w):
    rr, cc = np.nonzero(np.ones((h, w), bool))
    assert S.rectangle_sums(h, w) == S.moment_sums(rr, cc)
    assert R.eccentricity_from_sums(*S.rectangle_sums(h, w)) == R.eccentricity(rr, cc)


GALLERY_EIGVALSH_BAR = 10 * 1.2e-16


def test_gallery_eccentricity_agrees_with_eigvalsh():
    """R.eccentricity against the way skimage evaluates it (float moments, np.linalg.eigvalsh) on the 18 gallery regions.
    The largest difference measured is 1.11e-16 (one ulp below 1); the bar is ten times that, for BLAS differences between
    machines.  It guards the restatement only: the device is held to the restatement exactly and at 1e-12 relative."""
    lab = S.gallery_labels()
    worst = 0.0
    for i in np.unique(lab)[1:]:
        rr, cc = np.nonzero(lab == i)
        worst = max(worst, abs(R.eccentricity(rr, cc) - R.eccentricity_eigvalsh(rr, cc)))
    print("largest difference", worst)
    assert worst <= GALLERY_EIGVALSH_BAR


def test_only_the_4096_row_scenes_raise_the_lds_limit():
    heights = {"slots": S.SLOT_HW[0], "straddle": S.STRADDLE_HW[0], "caps": S.CAP_SIDE, "status": 16, "gallery": S.GALLERY_HW[0],
               "flush": S.FLUSH_HW[0], "wide": S.WIDE_HW[0], "fan": S.FAN_HW[0], "sides": S.SIDES_HW[0], "tall": S.TALL_HW[0],
               "planes": S.PLANE}
    above = {k for k, h in heights.items() if S.region_lds_bytes(h) > S.LDS_DEFAULT}
    assert above == {"tall", "planes"}
    assert S.region_lds_bytes(3270) <= S.LDS_DEFAULT < S.region_lds_bytes(3280)
