"""Seeded scenes for the cell extraction (csrc/extract.hip) where its kernels loop and at its limits, and the arithmetic
that says what each scene reaches.  Every builder returns (images, labels, qc): what CellExtractor(**qc).extract_batch takes.
tests/test_extract_scenes_cpu.py proves on the CPU that each scene reaches what it is meant to; tests/test_gpu_extract_sweep.py
runs them on the device against tests/extract_reference.py."""
import numpy as np

# ---- the launch arithmetic of csrc/extract.hip, mirrored -------------------------------------------------------------------
SCAN_THREADS = 1024                                     # ex_scan: one workgroup
EX_THREADS = 256                                        # ex_init / ex_compact / ex_region_pass / ex_gather
EX_WAVES = EX_THREADS // 64
GRID_CAP = 4096                                         # blocks of ex_init and ex_compact
MAX_SLOTS = 1 << 22
MAX_BATCH = 65535
LDS_DEFAULT = 65536                                     # dynamic LDS a kernel may ask for without raising its limit


def scan_per(nslots: int) -> int:
    """Consecutive slots per thread of ex_scan."""
    return -(-nslots // SCAN_THREADS)


def scan_run(t: int, nslots: int):
    """[s0, s1) of scan thread t."""
    per = scan_per(nslots)
    s0 = min(t * per, nslots)
    return s0, min(s0 + per, nslots)


def scan_empty_threads(nslots: int) -> int:
    """Scan threads whose clamped run is empty."""
    return sum(1 for t in range(SCAN_THREADS) if scan_run(t, nslots)[0] == scan_run(t, nslots)[1])


def scan_straddles(nslots: int, max_label: int):
    """Scan threads whose run holds slots of more than one image."""
    out = []
    for t in range(SCAN_THREADS):
        s0, s1 = scan_run(t, nslots)
        if s1 > s0 and s0 // max_label != (s1 - 1) // max_label:
            out.append(t)
    return out


def grid_rounds(nslots: int) -> int:
    """Rounds of the grid-stride loops of ex_init and ex_compact."""
    blocks = min(-(-nslots // EX_THREADS), GRID_CAP)
    return -(-nslots // (blocks * EX_THREADS))


def status_rounds(batch: int) -> int:
    """Rounds of ex_scan's status[b] loop."""
    return -(-batch // SCAN_THREADS)


def region_lds_bytes(H: int) -> int:
    """Dynamic LDS of ex_region_pass for an image of H rows: rowL / rowR int16 [H] each, two chains of 2H + 2 ints."""
    return ((4 * H + 15) & ~15) + 2 * (2 * H + 2) * 4


def moment_sums(rr, cc):
    """(n, si, sj, sii, sjj, sij) of a pixel list as Python ints."""
    i = [int(x) for x in rr]
    j = [int(x) for x in cc]
    return (len(i), sum(i), sum(j), sum(x * x for x in i), sum(x * x for x in j), sum(x * y for x, y in zip(i, j)))


def rectangle_sums(h: int, w: int):
    """The same sums of a filled h x w rectangle at the origin, in closed form."""
    s1 = lambda m: m * (m - 1) // 2
    s2 = lambda m: (m - 1) * m * (2 * m - 1) // 6
    return (h * w, w * s1(h), h * s1(w), w * s2(h), h * s2(w), s1(h) * s1(w))


def _texture(rng, shape, dtype):
    """Pixels whose mean and spread pass the intensity rule on any window."""
    hi = 250 if dtype == np.uint8 else 4000
    return rng.integers(hi // 10, hi, shape, dtype=dtype)


# ---- 1. slot tables past one slot per scan thread ------------------------------------------------------------------------------
SLOT_MAX_LABELS = (1023, 1024, 1025, 2047, 2048, 2049, 3001)
SLOT_HW = (128, 512)
SLOT_QC = dict(min_area=100)


def slot_square_ids(M: int):
    """The ids that get a passing 12 x 12 square: 1, M, and the ids on either side of the boundaries between the runs of
    scan threads t - 1 and t (slots t * per - 1 and t * per are ids t * per and t * per + 1)."""
    per = scan_per(M)
    last = -(-M // per) - 1                                  # the last thread with a slot
    ids = {1, M}
    for t in (1, 3, 37, 150, 300, last):
        for i in (t * per, t * per + 1):
            if 1 <= i <= M:
                ids.add(i)
    if per >= 3:
        ids.add(37 * per + 2)                                # and one in the middle of a run
    return sorted(ids)


def slot_table_scene(M: int, seed: int = 0):
    """One 128 x 512 image with max_label = M: 2 x 2 blocks that fail the area rule, every seventh id absent, and 12 x 12
    passing squares on slot_square_ids(M)."""
    H, W = SLOT_HW
    rng = np.random.default_rng(1000 + M + seed)
    lab = np.zeros((1, H, W), np.int32)
    squares = slot_square_ids(M)
    assert len(squares) <= 30
    for k, i in enumerate(squares):                          # one band of squares, clear of the border rule
        lab[0, 14:26, 14 + 16 * k:26 + 16 * k] = i
    per_row = W // 2
    k = 0
    for i in range(1, M + 1):
        if i in squares or i % 7 == 0:
            continue
        r, c = 32 + 2 * (k // per_row), 2 * (k % per_row)
        assert r + 2 <= H
        lab[0, r:r + 2, c:c + 2] = i
        k += 1
    if M not in squares:                                     # max_label is the largest id present
        raise AssertionError
    return _texture(rng, (1, H, W), np.uint16), lab, dict(SLOT_QC)


STRADDLE_HW = (400, 400)
STRADDLE_PER_IMAGE = 31 * 31
STRADDLE_QC = dict(min_area=100, max_eccentricity=1.0)
STRADDLE_MIDDLE_IDS = (1, 2, 480, 960, 961)


def straddle_scene(seed: int = 0):
    """Three 400 x 400 images of 10 x 10 squares on a 12-pixel pitch, ids 1..961 in raster order.  Image 0 is full, image 1
    holds five ids, image 2 is full but its id 500 is painted 40 x 6: it passes with a side below 8, so the image yields no cell."""
    H, W = STRADDLE_HW
    rng = np.random.default_rng(2000 + seed)
    lab = np.zeros((3, H, W), np.int32)
    for i in range(1, STRADDLE_PER_IMAGE + 1):
        r, c = 14 + 12 * ((i - 1) // 31), 14 + 12 * ((i - 1) % 31)
        for b in (0, 2):
            lab[b, r:r + 10, c:c + 10] = i
        if i in STRADDLE_MIDDLE_IDS:
            lab[1, r:r + 10, c:c + 10] = i
    r, c = 14 + 12 * (499 // 31), 14 + 12 * (499 % 31)
    lab[2][lab[2] == 500] = 0
    lab[2, r:r + 40, c:c + 6] = 500                          # over parts of the three squares below it
    return _texture(rng, (3, H, W), np.uint16), lab, dict(STRADDLE_QC)


# ---- 2. grids and batches at the caps ----------------------------------------------------------------------------------------
CAP_BATCH = MAX_BATCH
CAP_SIDE = 8
CAP_MAX_LABEL = 64
CAP_QC = dict(border=0, min_area=60, min_mean=0, min_std=0)
CAP_VARIANTS = 5                                            # pixel contents per label prototype
CAP_COVERED_EVERY, CAP_COVERED_AT = 33, 29                   # images b % 33 == 29, the last one among them: 1986 cells


def cap_prototypes(top_id: int = CAP_MAX_LABEL, seed: int = 0):
    """(images [P,8,8] uint16, labels [P,8,8] int32): four hand-made label planes -- empty; ids 1 and top_id as single pixels;
    a 2 x 3 block of id 7 and a diagonal of id 33; wholly covered by id 64 -- each under CAP_VARIANTS pixel contents.
    Prototype p = kind * CAP_VARIANTS + variant."""
    rng = np.random.default_rng(3000 + seed)
    kinds = np.zeros((4, CAP_SIDE, CAP_SIDE), np.int32)
    kinds[1, 0, 0] = 1
    kinds[1, 7, 7] = top_id
    kinds[2, 2:4, 3:6] = 7
    kinds[2, [4, 5, 6], [0, 1, 2]] = 33
    kinds[3] = 64
    pix = rng.integers(0, 65536, (CAP_VARIANTS, CAP_SIDE, CAP_SIDE), dtype=np.uint16)
    pix[:, 7, 7] = (65535, 0, 1, 40000, 65535)               # the last pixel of the allocation is not a repeat of its neighbours
    labs = np.repeat(kinds, CAP_VARIANTS, axis=0)
    imgs = np.tile(pix, (4, 1, 1))
    return imgs, labs


def cap_prototype_of(batch: int = CAP_BATCH):
    """The prototype index of every image."""
    b = np.arange(batch)
    kind = np.where(b % CAP_COVERED_EVERY == CAP_COVERED_AT, 3, b % 3)
    return kind * CAP_VARIANTS + b % CAP_VARIANTS


def cap_scene(top_id: int = CAP_MAX_LABEL, seed: int = 0):
    """65535 images of 8 x 8 built from cap_prototypes.  top_id = 65 puts batch * max_label above MAX_SLOTS: the wrapper relabels."""
    imgs, labs = cap_prototypes(top_id, seed)
    p = cap_prototype_of()
    return imgs[p], labs[p], dict(CAP_QC)


STATUS_BATCH = 1100
STATUS_QC = dict(border=0, min_area=30, max_eccentricity=1.0, min_mean=0, min_std=0)


def status_scene(seed: int = 0):
    """1100 images of 16 x 16: a passing 10 x 10 square in each, a single pixel in every fourth, and in every tenth a passing
    12 x 3 region, which leaves that image without cells."""
    rng = np.random.default_rng(4000 + seed)
    lab = np.zeros((STATUS_BATCH, 16, 16), np.int32)
    lab[:, 1:11, 2:12] = 1
    lab[7::10, 2:14, 13:16] = 2
    lab[0::4, 13, 5] = 3
    return rng.integers(0, 256, (STATUS_BATCH, 16, 16), dtype=np.uint8), lab, dict(STATUS_QC)


# ---- 3. degenerate regions -----------------------------------------------------------------------------------------------------
GALLERY_HW = (220, 330)
GALLERY_OPEN_QC = dict(border=0, min_area=1, max_area=10 ** 9, max_eccentricity=1.0, min_mean=0, min_std=0)


def gallery_labels():
    """One label each: see the comments.  The last id is a one-pixel frame round the whole image."""
    H, W = GALLERY_HW
    lab = np.zeros((H, W), np.int32)
    rr, cc = np.mgrid[0:H, 0:W]
    lab[3, 3] = 1                                            # a single pixel
    lab[3, 6:8] = 2                                          # 1 x 2
    lab[6, 3] = lab[7, 4] = 3                                # a two-pixel diagonal
    lab[10, 3:73] = 4                                        # 1 x 70
    lab[14:84, 3] = 5                                        # 70 x 1
    k = np.arange(40)
    lab[14 + k, 8 + k] = 6                                   # a 40-pixel diagonal
    lab[14 + k, 100 - k] = 7                                 # and an anti-diagonal
    lab[20:41, 130] = 8                                      # a plus
    lab[30, 120:141] = 8
    lab[14:45, 150:153] = 9                                  # a C
    lab[14:17, 150:176] = 9
    lab[42:45, 150:176] = 9
    d2 = (rr - 30) ** 2 + (cc - 210) ** 2
    lab[(d2 >= 8 ** 2) & (d2 <= 14 ** 2)] = 10               # a ring
    tri = (rr >= 14) & (rr < 54) & (cc >= 240) & (cc - 240 <= rr - 14)
    lab[tri] = 11                                            # a right triangle: legs on the left and at the bottom
    chk = (rr >= 60) & (rr < 69) & (cc >= 60) & (cc < 69) & ((rr + cc) % 2 == 0)
    lab[chk] = 12                                            # a 9 x 9 checkerboard
    lab[90, 100] = lab[135, 225] = 13                        # two pixels 45 rows and 125 columns apart
    lab[90:94, 10:74] = 14                                   # 4 x 64
    lab[100:105, 10:75] = 15                                 # 5 x 65
    lab[110:113, 10:139] = 16                                # 3 x 129
    lab[120:123, 10:13] = 17                                 # 3 x 3
    lab[0, :] = lab[H - 1, :] = 18                           # the frame: its bbox is the image
    lab[:, 0] = lab[:, W - 1] = 18
    return lab


def gallery_scene(dtype, qc=None, seed: int = 0):
    rng = np.random.default_rng(5000 + seed)
    lab = gallery_labels()[None]
    return _texture(rng, lab.shape, dtype), lab, dict(GALLERY_OPEN_QC if qc is None else qc)


FLUSH_HW = (70, 90)
FLUSH_QC = dict(border=0, min_area=100)


def flush_scene(seed: int = 0):
    """Two 70 x 90 three-channel images, border = 0.  The last one has passing 16 x 16 regions in its four corners and in the
    middle of its four sides; the first one in one corner and in the middle."""
    H, W = FLUSH_HW
    rng = np.random.default_rng(6000 + seed)
    lab = np.zeros((2, H, W), np.int32)
    lab[0, 0:16, 0:16] = 4
    lab[0, 30:46, 40:56] = 9
    spots = [(0, 0), (0, 37), (0, W - 16), (27, 0), (27, W - 16), (H - 16, 0), (H - 16, 37), (H - 16, W - 16)]
    for i, (r, c) in enumerate(spots):
        lab[1, r:r + 16, c:c + 16] = 2 * i + 1
    return _texture(rng, (2, H, W, 3), np.uint8), lab, dict(FLUSH_QC)


# ---- 4. tall, wide and largest -----------------------------------------------------------------------------------------------------
TALL_HW = (4096, 64)
TALL_QC = dict(border=0, max_area=10 ** 9, max_eccentricity=1.0)


def tall_scene(seed: int = 0):
    """4096 x 64: id 1 between a parabolic left edge, left(i) = rint(40 ((i - 2047.5) / 2047.5)^2), and column 60; id 2 is column 63."""
    H, W = TALL_HW
    rng = np.random.default_rng(7000 + seed)
    i = np.arange(H)
    left = np.rint(40.0 * ((i - 2047.5) / 2047.5) ** 2).astype(np.int64)
    cc = np.arange(W)[None, :]
    lab = np.zeros((1, H, W), np.int32)
    lab[0][(cc >= left[:, None]) & (cc <= 60)] = 1
    lab[0, :, 63] = 2
    return _texture(rng, (1, H, W), np.uint16), lab, dict(TALL_QC)


WIDE_HW = (3, 4096)


def wide_scene(seed: int = 0):
    """3 x 4096: one label over the whole middle row."""
    H, W = WIDE_HW
    rng = np.random.default_rng(8000 + seed)
    lab = np.zeros((1, H, W), np.int32)
    lab[0, 1, :] = 5
    return _texture(rng, (1, H, W), np.uint8), lab, dict(TALL_QC)


FAN_HW = (205, 2540)


def fan_scene(seed: int = 0):
    """205 x 2540: one label of two pixels per row, the left one at (i - 100)^2 // 4 and the right one in a straight column.  The
    slope of the left edge changes in every row or two, so the left chain keeps about a hundred points."""
    H, W = FAN_HW
    rng = np.random.default_rng(8500 + seed)
    i = np.arange(201)
    lab = np.zeros((1, H, W), np.int32)
    lab[0, 2 + i, 5 + (i - 100) ** 2 // 4] = 3
    lab[0, 2 + i, W - 6] = 3
    return _texture(rng, (1, H, W), np.uint16), lab, dict(TALL_QC)


SIDES_HW = (1100, 1100)
SIDES_QC = dict(max_area=10 ** 9)


def sides_scene(h: int, w: int, seed: int = 0):
    """1100 x 1100: four 8 x 8 blobs under one label in the corners of an h x w bounding box, clear of the border rule."""
    H, W = SIDES_HW
    rng = np.random.default_rng(9000 + seed)
    lab = np.zeros((1, H, W), np.int32)
    r0, c0 = 30, 40
    for r in (r0, r0 + h - 8):
        for c in (c0, c0 + w - 8):
            lab[0, r:r + 8, c:c + 8] = 7
    return _texture(rng, (1, H, W), np.uint16), lab, dict(SIDES_QC)


PLANE = 4096


def plane_scene(image: str, labelled: str):
    """4096 x 4096 uint16 under the default QC.  image: 'constant' (65535 everywhere) or 'halves' (the left half 0, the right half
    65535); labelled: 'all' or 'left' (the left 4096 x 2048 half), id 1."""
    img = np.full((1, PLANE, PLANE), 65535, np.uint16)
    if image == "halves":
        img[:, :, :PLANE // 2] = 0
    lab = np.ones((1, PLANE, PLANE), np.int32)
    if labelled == "left":
        lab[:, :, PLANE // 2:] = 0
    return img, lab, {}


def left_chain_length(lab_plane, label: int) -> int:
    """Points that the left monotone chain of hull_chain.hpp keeps for one region: the convex minorant of the left pixel-edge
    midpoints, in doubled window coordinates (y = 2i +- 1 at x = 2j, y = 2i at x = 2j - 1), collinear points dropped."""
    rr, cc = np.nonzero(lab_plane == label)
    r0, h = int(rr.min()), int(rr.max() - rr.min()) + 1
    left = {}
    for r, c in zip(rr - r0, cc - cc.min()):
        left[int(r)] = min(left.get(int(r), 1 << 30), int(c))
    pts = {}
    for i, j in left.items():
        for y, x in ((2 * i - 1, 2 * j), (2 * i, 2 * j - 1), (2 * i + 1, 2 * j)):
            pts[y] = min(pts.get(y, 1 << 30), x)
    ch = []
    for y in sorted(pts):
        x = pts[y]
        while len(ch) >= 2:
            (oy, ox), (ay, ax) = ch[-2], ch[-1]
            if (ay - oy) * (x - ox) - (ax - ox) * (y - oy) <= 0:
                ch.pop()
            else:
                break
        ch.append((y, x))
    return len(ch)
