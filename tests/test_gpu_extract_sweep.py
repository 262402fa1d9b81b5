"""Cell extraction on the device (csrc/extract.hip through cellscreen.extract.CellExtractor) where its kernels loop and at its
limits, on the scenes of tests/extract_scenes.py.  The reference is the restatement of tests/extract_reference.py, every region
of every image and every field, at the bars of test_gpu_extract.py (check_against_restatement: integers, mean and solidity exact,
eccentricity and std at 1e-12 relative, cells bit-identical to Preprocessor on the host-cut crops); the 4096 x 4096 planes are held
to closed forms.  What each scene reaches -- the figures tests/test_extract_scenes_cpu.py asserts:

* slot tables, max_label M in 1023 / 1024 / 1025 / 2047 / 2048 / 2049 / 3001 on one 128 x 512 image: ex_scan gives a thread
  per = 1, 1, 2, 2, 2, 3, 3 slots; 1, 0, 511, 0, 0, 341, 23 threads have a clamped-empty run; every seventh slot is empty;
  passing 12 x 12 squares sit in the last slot of one thread's run and the first of the next, so the cell index and the crop
  offset are carried from thread to thread.
* straddle, 3 images x 961 slots = 2883, per = 3: the runs of threads 320 and 640 hold slots of two images; image 1 leaves ~950
  empty slots in the middle; image 2 passes 961 regions but is IMAGE_NO_CELLS, and the numbering does not advance through it.
* caps, 65535 images of 8 x 8 with max_label 64: 4,194,240 slots (kMaxSlots is 4,194,304), ex_init and ex_compact go round 4
  times, per = 4096, blockIdx.z of the label pass reaches 65534, the status loop goes round 64 times, 1986 cells, the last
  image's crop ends at the last pixel of the allocation.  With one id raised to 65 the wrapper relabels (2 slots per image).
* status, 1100 images of 16 x 16: the status loop's second round holds both IMAGE_OK and IMAGE_NO_CELLS; per = 4.
* gallery, 18 degenerate regions on 220 x 330: h of 1, 2, 3; w of 1, 64, 65, 129; windows whose rows are mostly empty; a
  triangle with pixel centres exactly on the hull; all three branches of the eccentricity; a frame whose bbox is the image.
* flush, border = 0: crops in all four corners and on all four sides of the last image of a batch.
* tall, 4096 x 64: 81,936 B of dynamic LDS (above the 65,536 default), h = 4096 > 256, the convex-count loop goes round 16
  times, the left chain keeps 62 points.  wide, 3 x 4096: the column loop goes round 64 times, pack_pt's x + 1 = 8192.
* fan, 205 x 2540: the left chain keeps 102 points, chain_segment's binary search runs over them; most of the window is empty.
* sides, 1100 x 1100: a passing bbox of 1024 x 1024 is cut, 1025 on either axis is IMAGE_UNSUPPORTED.
* planes, 4096 x 4096 uint16: N * Sxx = 2^79 and N * S2 = 2^70 in the 128-bit helpers, 81,936 B of LDS.

The caps and the plane cases allocate a few hundred MB on the device (about 460 MB of slot tables; 96 MB of image and labels)."""
import numpy as np
import pytest

import extract_reference as R
import extract_scenes as S
from cellscreen import extract as X
from cellscreen import preprocess as pp
from test_gpu_extract import check_against_restatement

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def proc():
    p = pp.Preprocessor(0)
    yield p
    p.close()


def _run(scene):
    images, labels, qc = scene
    e = X.CellExtractor(0, **qc)
    try:
        return e.extract_batch(images, labels)
    finally:
        e.close()


def _check(scene, proc):
    images, labels, qc = scene
    r = _run(scene)
    return r, check_against_restatement(r, images, labels, proc, qc=qc)


# ---- 1. slot tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", S.SLOT_MAX_LABELS)
def test_slot_tables_past_one_slot_per_scan_thread(proc, M):
    r, n = _check(S.slot_table_scene(M), proc)
    squares = S.slot_square_ids(M)
    assert n == len(squares) and list(r.regions["label"][r.regions["cell"] >= 0]) == squares
    assert r.status[0] == X.IMAGE_OK


def test_scan_runs_straddling_image_boundaries(proc):
    scene = S.straddle_scene()
    r, n = _check(scene, proc)
    assert list(r.status) == [X.IMAGE_OK, X.IMAGE_OK, X.IMAGE_NO_CELLS]
    assert n == S.STRADDLE_PER_IMAGE + len(S.STRADDLE_MIDDLE_IDS)
    reg = r.regions
    assert np.all(reg["cell"][reg["image"] == 2] == -1) and np.all(reg["failed"][(reg["image"] == 2) & (reg["label"] == 500)] == 0)
    assert list(reg["cell"][reg["image"] == 1]) == list(range(S.STRADDLE_PER_IMAGE, n))


# ---- 2. the caps -------------------------------------------------------------------------------------------------------------------
def _prototype_tables(pimg, plab, qc):
    """Per prototype: its regions as a REGION_DTYPE table (image and cell left 0), its status, its crops."""
    from cellscreen import _lib as L
    tables, status, crops = [], [], []
    for k in range(len(plab)):
        c, regs, st = R.extract(plab[k], pimg[k], qc)
        t = np.zeros(len(regs), L.REGION_DTYPE)
        for i, e in enumerate(regs):
            for f in e:
                t[f][i] = e[f]
        tables.append(t)
        status.append(st)
        crops.append(c)
    return tables, np.array(status, np.int32), crops


def _check_against_prototypes(r, pimg, plab, proto_of, qc, proc):
    """check_against_restatement's comparisons for a batch built as prototype[proto_of[b]]: the restatement runs on the
    prototypes, the expected table is theirs with the image index substituted, in image order."""
    tables, pstatus, pcrops = _prototype_tables(pimg, plab, qc)
    B = len(proto_of)
    assert np.array_equal(r.status, pstatus[proto_of])
    counts = np.array([len(t) for t in tables])[proto_of]
    start = np.concatenate([[0], np.cumsum([len(t) for t in tables])])[:-1]
    allt = np.concatenate(tables)
    image = np.repeat(np.arange(B), counts)
    within = np.arange(counts.sum()) - np.repeat(np.cumsum(counts) - counts, counts)
    exp = allt[start[proto_of[image]] + within]
    got = r.regions
    assert len(got) == len(exp)
    assert np.array_equal(got["image"], image)
    for f in ("label", "minr", "minc", "maxr", "maxc", "area", "convex_area", "failed", "mean_intensity", "solidity"):
        assert np.array_equal(got[f], exp[f]), f
    for f in ("eccentricity", "std_intensity"):
        assert np.all(np.abs(got[f] - exp[f]) <= 1e-12 * np.maximum(np.abs(exp[f]), 1e-300)), f
    passing = (exp["failed"] == 0) & (pstatus[proto_of[image]] == R.IMAGE_OK)
    assert np.array_equal(got["cell"], np.where(passing, np.cumsum(passing) - 1, -1))
    n = int(passing.sum())
    assert len(r.cells) == n == len(r.cell_image) and np.array_equal(r.cell_image, image[passing])
    owners = [k for k in range(len(plab)) if pcrops[k]]
    assert all(len(pcrops[k]) == 1 for k in owners)                       # at most one cell per prototype here
    ref = np.zeros((len(plab),) + r.cells.shape[1:], np.float32)
    ref[owners] = proc([pcrops[k][0] for k in owners], clip_limit=qc.get("clip_limit", pp.CLIP_LIMIT))
    assert np.array_equal(r.cells.view(np.uint32), ref[proto_of[image[passing]]].view(np.uint32))
    return n


@pytest.mark.parametrize("top_id", [64, 65])
def test_batch_and_slot_caps(proc, top_id):
    """top_id 64: the labels are used as given, 65535 x 64 slots.  top_id 65: batch x max_label is above the cap, the wrapper
    relabels per image and maps the ids back."""
    pimg, plab = S.cap_prototypes(top_id)
    proto_of = S.cap_prototype_of()
    scene = S.cap_scene(top_id)
    n = _check_against_prototypes(_run(scene), pimg, plab, proto_of, scene[2], proc)
    assert n == 1986


def test_status_of_more_images_than_scan_threads(proc):
    r, n = _check(S.status_scene(), proc)
    assert n == S.STATUS_BATCH - S.STATUS_BATCH // 10
    assert np.array_equal(r.status == X.IMAGE_NO_CELLS, np.arange(S.STATUS_BATCH) % 10 == 7)


# ---- 3. degenerate regions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("qc", ["open", "default"])
def test_gallery_of_degenerate_regions(proc, dtype, qc):
    scene = S.gallery_scene(dtype, None if qc == "open" else {})
    r, n = _check(scene, proc)
    assert len(r.regions) == 18
    if qc == "open":
        assert n == 0 and r.status[0] == X.IMAGE_NO_CELLS and np.all(r.regions["failed"] == 0)
    else:
        assert n == 3 and r.status[0] == X.IMAGE_OK and len(set(r.regions["failed"])) >= 6


def test_crops_flush_with_the_edges_of_the_last_image(proc):
    r, n = _check(S.flush_scene(), proc)
    assert n == 10 and list(r.status) == [X.IMAGE_OK, X.IMAGE_OK]


# ---- 4. tall, wide and largest -----------------------------------------------------------------------------------------------------
def test_tall_image_above_the_default_lds(proc):
    r, n = _check(S.tall_scene(), proc)
    assert n == 0 and r.status[0] == X.IMAGE_NO_CELLS and list(r.regions["failed"]) == [0, 0]


def test_one_row_over_the_widest_image(proc):
    r, n = _check(S.wide_scene(), proc)
    assert n == 0 and r.status[0] == X.IMAGE_NO_CELLS and r.regions["maxc"][0] == 4096 and r.regions["eccentricity"][0] == 1.0


def test_left_chain_of_a_hundred_points(proc):
    r, n = _check(S.fan_scene(), proc)
    assert n == 0 and r.status[0] == X.IMAGE_UNSUPPORTED and list(r.regions["area"]) == [402]


@pytest.mark.parametrize("h,w,status,cells", [(1024, 1024, X.IMAGE_OK, 1), (1025, 1024, X.IMAGE_UNSUPPORTED, 0),
                                              (1024, 1025, X.IMAGE_UNSUPPORTED, 0)])
def test_side_rule_at_its_edge(proc, h, w, status, cells):
    r, n = _check(S.sides_scene(h, w), proc)
    assert n == cells and r.status[0] == status and list(r.regions["failed"]) == [0]
    assert (r.regions["maxr"][0] - r.regions["minr"][0], r.regions["maxc"][0] - r.regions["minc"][0]) == (h, w)


@pytest.mark.parametrize("image,labelled", [("constant", "all"), ("halves", "all"), ("halves", "left")])
def test_whole_plane_against_closed_forms(image, labelled):
    """The largest operands of central_num and exact_diff_to_double.  The whole plane: area = convex area = 2^24, solidity 1,
    eccentricity 0; mean 65535 and std 0 of the constant image, 32767.5 both of the halves.  The left half: the eccentricity of
    the 4096 x 2048 rectangle from its closed-form sums, mean and std 0 (its window is the dark half)."""
    r = _run(S.plane_scene(image, labelled))
    assert r.status[0] == X.IMAGE_OK and len(r.cells) == 0 and len(r.regions) == 1
    g = r.regions[0]
    w = S.PLANE if labelled == "all" else S.PLANE // 2
    assert (g["image"], g["label"], g["minr"], g["minc"], g["maxr"], g["maxc"], g["cell"]) == (0, 1, 0, 0, S.PLANE, w, -1)
    assert g["area"] == g["convex_area"] == S.PLANE * w and g["solidity"] == 1.0
    dark_or_flat = (image, labelled) != ("halves", "all")
    assert g["failed"] == X.QC_BORDER | X.QC_AREA | (X.QC_INTENSITY if dark_or_flat else 0)
    ecc = R.eccentricity_from_sums(*S.rectangle_sums(S.PLANE, w))
    assert abs(g["eccentricity"] - ecc) <= 1e-12 * ecc and (labelled == "left" or g["eccentricity"] == 0.0)
    mean, std = {("constant", "all"): (65535.0, 0.0), ("halves", "all"): (32767.5, 32767.5), ("halves", "left"): (0.0, 0.0)}[image, labelled]
    assert g["mean_intensity"] == mean and g["std_intensity"] == std
