"""tests/preprocess_plans.py without a device: the limits are the sources', every class the plan names has a case, every case is
legal, the LDS plan and the packing of the tile tables hold for every accepted side, and every family can fail: one named mistake
per family, restated on the CPU, moves the expected result on the family's own crops by more than the bar."""
import numpy as np

import preprocess_plans as PL
import preprocess_sized_reference as PR
from oracle import preprocess_oracle as po

ALL_CASES = [c for f in PL.FAMILIES for c in PL.cases(f)]


# ---- the limits -----------------------------------------------------------------------------------------------------------------
def test_limits_are_read_from_the_sources_and_pinned():
    c = PL.read_limits()
    assert c == PL.LIMITS and set(c) == set(PL.LIMIT_SOURCES)
    assert (c["PP_THREADS"], c["PP_WAVES"], c["PP_NBINS"], c["PP_GRAY"], c["PP_MAX_TAPS"]) == (512, 8, 256, 1 << 14, 32)
    assert (c["kPreprocMin"], c["kPreprocMax"], c["kPreprocMaxRatio"], c["kPreprocOutMin"], c["kPreprocOutMax"]) == (8, 1024, 16, 8, 512)
    assert (c["kChunkPixels"], c["kChunkCrops"], c["kChunkOutBytes"]) == (256 << 20, 1 << 16, 1 << 30)
    assert PL.BIN_SIZE == 65 == po.NR_OF_GRAY // po.NBINS + 1 and PL.GRAY == po.NR_OF_GRAY and PL.NBINS == po.NBINS


def test_python_limits_equal_the_kernels():
    assert PL.read_python_limits() == dict(OUT_SIDE=PL.OUT, MAX_RATIO=PL.MAX_RATIO, OUT_MIN=PL.OUT_MIN, OUT_MAX=PL.OUT_MAX)
    # the wrapper keeps no crop-side limit of its own: 8 and 1024 are the library's to refuse (tests/test_gpu_preprocess_sweep.py).
    # The contract the header publishes and the sentence the extractor's wrapper says about a region are today's values
    with open(PL.os.path.join(PL.H.ROOT, "include", "cellscreen.h")) as f:
        header = f.read()
    assert f"output   {PL.OUT_MIN} <= out_h, out_w <= {PL.OUT_MAX}, independent of each other" in header
    assert f"crops    {PL.SIDE_MIN} <= side <= {PL.SIDE_MAX} per axis" in header and f"side <= {PL.MAX_RATIO} * out on that axis" in header
    with open(PL.os.path.join(PL.PKG, "extract.py")) as f:
        assert f"bounding-box side above {PL.SIDE_MAX} px or above {{MAX_RATIO}} x the output size" in f.read()


# ---- the LDS plan ---------------------------------------------------------------------------------------------------------------
def test_static_arrays_are_the_kernels_declarations():
    assert PL.read_static_lds() == PL.STATIC_LDS
    assert PL.static_lds_bytes() == 8192 + 64 + 528 + 2048 + 4096


def test_lds_fits_for_every_accepted_shape_and_the_plan_holds_the_largest():
    sides = np.arange(PL.SIDE_MIN, PL.SIDE_MAX + 1)
    nt = np.array([PL.tile(n)[1] for n in sides])
    dyn = np.maximum(nt[:, None] * nt[None, :] * PL.NBINS * 2, PL.WAVES * sides[None, :] * 8)
    total = dyn + PL.static_lds_bytes()
    assert total.max() <= PL.LDS_BYTES
    ih, iw = np.unravel_index(np.argmax(dyn), dyn.shape)
    worst = (int(sides[ih]), int(sides[iw]))
    assert worst == (15, 15) and int(dyn.max()) == 225 * 512 == PL.lds_bytes(15, 15) and (dyn == dyn.max()).sum() == 1
    assert int(dyn[:, -1].min()) == PL.WAVES * 1024 * 8 == PL.lds_bytes(8, 1024)       # the widest line of the resize
    for family in ("mixed", "tiles"):
        assert worst in {c["shape"] for c in PL.cases(family)}, family
    for n in (8, 15, 16, 100, 1024):                     # lds_bytes is the table's entry
        assert PL.lds_bytes(n, 1000) == dyn[n - 8, 1000 - 8]


def test_tile_tables_pack_for_every_side():
    """rowtab / coltab hold (block << 8) | offset in 16 bits, crow / ccol one weight per in-tile offset."""
    rows, crow = PL.STATIC_LDS["rowtab"][1][0], PL.STATIC_LDS["crow"][1][0]
    assert PL.STATIC_LDS["coltab"][1][0] == rows >= PL.SIDE_MAX and PL.STATIC_LDS["ccol"][1][0] == crow
    for n in range(PL.SIDE_MIN, PL.SIDE_MAX + 1):
        k, nt, pad, off = PL.tile(n)
        assert 1 <= k <= crow and 8 <= nt <= 15 and 0 <= pad < k and nt * k == n + pad and off == k // 2
        pr = np.arange(n) + off
        block, inner = pr // k, pr % k
        assert block.max() <= nt and block.max() < 256 and inner.max() < min(256, crow)
        packed = ((block << 8) | inner).astype(np.uint16)
        assert np.array_equal(packed >> 8, block) and np.array_equal(packed & 255, inner)
        # the oracle's padded frame is the kernel's: nt tiles, the last one reflected once past the end
        kk = n // 8
        assert (n + kk // 2 + (kk - n % kk) % kk + (kk + 1) // 2) // kk - 1 == nt and pad < n


def test_every_radius_an_accepted_side_takes_has_a_table_entry():
    seen = set()
    for out in range(PL.OUT_MIN, PL.OUT_MAX + 1):
        for n in range(PL.SIDE_MIN, min(PL.SIDE_MAX, PL.MAX_RATIO * out) + 1):
            sigma, lw = PL.gauss(n, out)
            seen.add(lw)
            assert (lw == -1) == (n <= out) and lw < n - 1    # one reflection is enough (preprocess.hip, mirror_once)
    assert seen == set(PL.RADII) and max(seen) <= PL.STATIC_LDS["wts"][1][1] - 1 == PL.MAX_TAPS


# ---- coverage -------------------------------------------------------------------------------------------------------------------
def test_every_case_is_legal_and_named_once():
    assert len({c["name"] for c in ALL_CASES}) == len(ALL_CASES)
    for c in ALL_CASES:
        assert PL.legal(c["shape"], c["hw"]), c["name"]
        assert c["dtype"] in ("uint8", "uint16") and c["clip"] in PL.CLIPS
    assert not PL.legal((1025, 8), (64, 64)) and not PL.legal((7, 8), (64, 64)) and not PL.legal((129, 8), (8, 8))
    assert not PL.legal((513, 64), (32, 64)) and PL.legal((512, 1024), (32, 64))


def test_tiles_cover_every_class_per_axis():
    sides = PL.TILE_SIDES
    assert {PL.tile(n)[1] for n in sides} == set(range(8, 16))
    assert {n % 8 for n in sides if PL.tile(n)[0] >= 16} == set(range(8))
    assert {8, 9, 15, 16, 63, 64, 65} <= set(sides)
    assert {PL.tile(n)[2] for n in sides} >= {0, 1, 7} and {PL.tile(n)[3] for n in sides} >= {0, 1, 3, 4, 8}
    assert {PL.gauss(n, PL.OUT)[1] for n in sides} == {-1, 0, 2}       # the radius family has the rest
    got = {(c["shape"], c["dtype"]) for c in PL.cases("tiles")}
    assert got == {((h, w), dt) for h in sides for w in sides for dt in ("uint8", "uint16")}
    assert all(c["hw"] == (64, 64) and c["clip"] == 0.02 for c in PL.cases("tiles"))
    assert {c["content"] for c in PL.cases("tiles")} == set(PL.TILE_CONTENTS)


def test_large_holds_the_shapes_the_sizes_and_no_periodic_crop():
    cs = PL.cases("large")
    assert len(cs) <= 20 and all(max(c["shape"]) > 300 for c in cs)
    at64 = {c["shape"] for c in cs if c["hw"] == (64, 64)}
    assert at64 >= {(1024, 1024), (1023, 1017), (1016, 513), (1024, 8), (8, 1024), (15, 1024), (1024, 15), (600, 333), (301, 1000)}
    sized = {(c["shape"], c["hw"]) for c in cs if c["hw"] != (64, 64)}
    assert {hw for _, hw in sized} == {(128, 128), (512, 512), (32, 64), (8, 512)}
    assert ((512, 1024), (32, 64)) in sized and ((128, 1024), (8, 512)) in sized
    for dt in ("uint8", "uint16"):
        assert {"noise", "blobs", "low"} <= {c["content"] for c in cs if c["dtype"] == dt}
        assert any(c["shape"] == (1024, 1024) and c["dtype"] == dt for c in cs)
    for c in cs:
        x = PL.crop(c)
        assert x.shape == c["shape"] and x.dtype == np.dtype(c["dtype"]) and not x.flags.writeable
        assert PL.periods(x) == [], c["name"]
        assert PL.THREADS * 16 <= x.size <= PL.THREADS * 2048                           # the pixel loops take 16 to 2048 trips
    assert PL.periods(np.tile(PL.crop(cs[4]), (1, 2))) != []                            # the check sees a tiled crop


def test_radius_covers_every_lw_on_both_axes_at_both_sizes():
    cs = PL.cases("radius")
    for out, widths in ((64, PL.RADIUS_WIDTHS), (8, (PL.RADIUS_WIDTH_8,))):
        assert min(widths) <= out or out == 8
        for axis in (0, 1):
            for w in widths:
                mine = [c for c in cs if c["hw"] == (out, out) and c["axis"] == axis and c["shape"][1 - axis] == w]
                assert sorted(c["lw"] for c in mine) == list(PL.RADII), (out, axis, w)
                for c in mine:
                    assert PL.gauss(c["shape"][axis], out)[1] == c["lw"] and c["content"] == "edges"
    assert PL.RADIUS_WIDTHS[0] < 64 < PL.RADIUS_WIDTHS[1]
    assert [PL.side_of_radius(lw, 64) for lw in (-1, 0, 30)] == [64, 79, 1024] and PL.side_of_radius(30, 8) == 128
    assert {c["dtype"] for c in cs if c["lw"] == 30} == {"uint8", "uint16"}
    x = PL.crop(cs[9])
    top = np.iinfo(x.dtype).max
    assert (x[0] == top).all() and (x[-1] == top).all() and (x[1:-1, 1:-1] < top // 2).all() and (x[1:-1, 0] > top // 2).all()


def test_ties_search_and_every_crop_holds_its_pixel():
    u8, u16 = PL.bin_deciding_ties(np.uint8), PL.bin_deciding_ties(np.uint16)
    # numpy rounds half to even: where `goes` is k a kernel that rounded ties up would differ, where it is k + 1 one that rounded down
    assert sum(1 for t in u16 if t[3] == t[2]) == 1596 and sum(1 for t in u16 if t[3] == t[2] + 1) == 1092
    assert [t for t in u8 if t[3] == t[2]] == [(22102, 7453, 5524, 5524), (44204, 14906, 5524, 5524), (65278, 257, 64, 64)]
    assert len(u8) == 4 and (65278, 257, 64, 64) == (254 * 257, 1 * 257, 64, 64)        # min 0, max 254, a pixel of 1: 64.5
    for rng_, a, k, goes in u8 + u16:
        assert rng_ % 2 == 0 and 0 < a < rng_ and goes == (k if k % 2 == 0 else k + 1)   # the float64 path lands on the even level
    # an independent count on one range: every odd a of range 32766 is a tie a / 2, a bin decider where (a + 1) / 2 is a multiple of 65
    assert sorted(t[1] for t in u16 if t[0] == 32766) == list(range(129, 32766, 130))
    brute = [(r, a) for r in range(2, 600, 2) for a in range(1, r)
             if 2 * ((a * 16383) % r) == r and ((a * 16383) // r + 1) % 65 == 0]
    assert brute == [t[:2] for t in u16 if t[0] < 600] and len(brute) > 0
    cs = PL.cases("ties")
    assert [(c["range"], c["a"]) for c in cs if c["dtype"] == "uint8"] == [t[:2] for t in u8]
    mine = [c for c in cs if c["dtype"] == "uint16"]
    ranges = {c["range"] for c in mine}
    assert len(ranges) >= 32 and {min(t[0] for t in u16), max(t[0] for t in u16), 32766} <= ranges
    for dt in ("uint8", "uint16"):
        assert {c["goes"] - c["k"] for c in cs if c["dtype"] == dt} == {0, 1}            # both mistakes have crops that show them
    for c in cs:
        x = po.img_as_uint16(PL.crop(c)).astype(np.int64)
        assert int(x.max() - x.min()) == c["range"] and (x - x.min() == c["a"]).sum() >= 2, c["name"]
        g = po._rescale_to_14bit(x.astype(np.uint16))[x - x.min() == c["a"]]
        assert (g == c["goes"]).all() and (c["k"] + 1) // 65 - c["k"] // 65 == 1


def test_clip_and_mixed_are_what_the_plan_says():
    cs = PL.cases("clip")
    assert {(c["shape"], c["content"]) for c in cs} == {(s, k) for s in ((1024, 1024), (120, 88)) for k in ("const", "two", "low", "noise")}
    for shape, content in {(c["shape"], c["content"]) for c in cs}:
        assert sorted(c["clip"] for c in cs if (c["shape"], c["content"]) == (shape, content)) == sorted(PL.CLIPS)
    assert PL.tile(1024)[0] ** 2 == 16384 and [PL.clip_limit_of(c, 16384) for c in PL.CLIPS] == [16384, 1, 81, 327, 1638, 16384]
    assert [PL.clip_limit_of(c, 15 * 11) for c in PL.CLIPS] == [165, 1, 1, 3, 16, 165]
    x = PL.crop([c for c in cs if c["content"] == "two" and c["shape"] == (120, 88)][0])
    assert len(np.unique(x)) == 2 and len(np.unique(PL.crop([c for c in cs if c["content"] == "const"][0]))) == 1
    for dt in ("uint8", "uint16"):
        mine = [c for c in PL.cases("mixed") if c["dtype"] == dt]
        assert [c["shape"] for c in mine] == [(15, 15), (8, 8), (15, 1024), (1024, 1024), (23, 15)]
        assert sum(int(np.prod(c["shape"])) for c in mine) < PL.CHUNK_PIXELS and len(mine) < PL.LIMITS["kChunkCrops"]
        need = [PL.lds_bytes(*c["shape"]) for c in mine]
        assert need[0] == 225 * 512 == max(need) and need[1] == min(need) == 64 * 512 and need[2] == need[3] == 65536


# ---- the restatements with nothing switched in are the oracle -------------------------------------------------------------------
def test_the_restatements_without_a_mistake_are_the_oracle():
    picks = [PL.cases("tiles")[i] for i in (0, 15 * 42 + 29, 400, 881)] + list(PL.cases("ties")[:5]) + [PL.cases("large")[8]] + \
        [c for c in PL.cases("clip") if c["shape"] == (120, 88)][::5] + list(PL.cases("radius")[60:64])
    for c in picks:
        x = PL.crop(c)
        assert np.array_equal(PL.clahe_with(x, c["clip"]), po.clahe_u16(x, c["clip"])), c["name"]
        eq = po.equalize_adapthist(x, c["clip"])
        assert np.array_equal(PL.resize_with(eq, c["hw"]), PR.resize_to(eq, *c["hw"])), c["name"]
    x = po.img_as_uint16(PL.crop(PL.cases("large")[8])).astype(np.int64)                # away from ties the three roundings agree
    rng_ = int(x.max() - x.min())
    tie = 2 * (((x - x.min()) * 16383) % rng_) == rng_
    for mode in ("up", "down"):
        assert np.array_equal(PL.gray_levels(x.astype(np.uint16), mode)[~tie], po._rescale_to_14bit(x.astype(np.uint16))[~tie])


# ---- every family can fail ------------------------------------------------------------------------------------------------------
def _planes_differ(c, mistake):
    x = PL.crop(c)
    return not np.array_equal(PL.clahe_with(x, c["clip"], mistake), po.clahe_u16(x, c["clip"]))


def test_ties_a_kernel_that_rounded_ties_up_or_down_changes_the_plane():
    for c in PL.cases("ties"):
        # the other rounding is the right one for this pixel, so both kinds of tie are in the family (test_ties_search_...)
        assert _planes_differ(c, "ties_up" if c["goes"] == c["k"] else "ties_down"), c["name"]


def test_radius_a_wrong_reflection_or_a_short_kernel_moves_the_output():
    worst = {m: 1.0 for m in PL.MISTAKES["radius"]}
    for c in PL.cases("radius"):
        eq = po.equalize_adapthist(PL.crop(c), c["clip"])
        good = PR.resize_to(eq, *c["hw"])
        for m in PL.MISTAKES["radius"]:
            d = np.abs(PL.resize_with(eq, c["hw"], m) - good).max()
            if c["lw"] >= 1:
                worst[m] = min(worst[m], d)
                assert d > 100 * PL.TOL_OUT, (c["name"], m, d)
            elif c["lw"] == -1 and PL.gauss(c["shape"][1 - c["axis"]], c["hw"][0])[1] < 1:
                assert d == 0.0                          # no filter on either axis: nothing to get wrong
    print("smallest change over lw >= 1:", worst)


def _tile_beyond_eight_weighs(n):
    """Whether a tile of index >= 8 enters the blend of a side n with a weight above zero.  All sides with nt > 8 but 9: there k = 1,
    the in-tile offset is always 0, so pixel c reads tile c - 1 alone and the ninth tile is built and never weighed."""
    k, nt, _, off = PL.tile(n)
    pr = np.arange(n) + off
    return bool(((np.minimum(pr // k - 1, nt - 1) >= 8) | ((np.minimum(pr // k, nt - 1) >= 8) & (pr % k > 0))).any())


def test_tiles_a_dropped_offset_or_eight_tiles_changes_the_plane():
    """Over a cross of the product (every height with three widths, every width with three heights), dtypes alternating."""
    assert [n for n in range(8, 1025) if (PL.tile(n)[1] > 8) != _tile_beyond_eight_weighs(n)] == [9]
    sides = PL.TILE_SIDES
    cross = {(h, w) for h in sides for w in (8, 64, 131)} | {(h, w) for w in sides for h in (8, 64, 131)}
    n = 0
    for c in PL.cases("tiles"):
        h, w = c["shape"]
        if (h, w) not in cross or (c["dtype"] == "uint8") != ((h + w) % 2 == 0) or c["content"] in ("low", "two"):
            continue
        n += 1
        padded = _tile_beyond_eight_weighs(h) or _tile_beyond_eight_weighs(w)            # every class with padding, and sides 10..15
        shifted = PL.tile(h)[3] > 0 or PL.tile(w)[3] > 0
        assert _planes_differ(c, "nt8") == padded, c["name"]
        assert _planes_differ(c, "offset_dropped") == shifted, c["name"]
    assert n >= 80


def test_large_a_short_pixel_loop_or_a_quotient_one_short_changes_the_plane():
    for c in PL.cases("large"):
        x = PL.crop(c)
        assert x.size > PL.THREADS
        if c["hw"] != (64, 64) and c["shape"] != (1024, 1024):
            continue                                     # phases A to C do not depend on the output size
        plane, bins = PL.clahe_with(x, c["clip"], None, want_bins=True)
        one_trip = np.concatenate([plane.ravel()[:PL.THREADS], bins.ravel()[PL.THREADS:].astype(np.uint16)]).reshape(x.shape)
        assert (one_trip != plane).mean() > 0.9, c["name"]
        if x.size == 1 << 20:                            # p reaches 2^20 - W only here
            short = PL.clahe_with(x, c["clip"], "quotient_short")
            assert np.array_equal(short[:-1], plane[:-1]) and (short[-1] != plane[-1]).sum() > 100, c["name"]
    x = PL.crop(PL.cases("large")[2])
    assert np.array_equal(PL.clahe_with(x, 0.02, "one_trip")[1:], (po._rescale_to_14bit(po.img_as_uint16(x)) // 65)[1:])


def test_clip_a_redistribution_that_stops_after_index_zero_changes_the_plane():
    """Which (content, clip limit) see it is a property of skimage's rule, listed here: where nothing is clipped (0, 1), where every
    bin ends on the limit before the loop (1e-5 at 16384 pixels) and on a constant crop there is no walk to cut short."""
    shows, trips = set(), []
    for c in PL.cases("clip"):
        if c["shape"] == (1024, 1024) and (c["clip"] in (0.0, 1.0) or c["content"] in ("const", "two")):
            continue                                     # kept off the clock; the 120 x 88 crops stand for them
        x = PL.crop(c)
        if not np.array_equal(PL.clahe_with(x, c["clip"], "first_index", trips), po.clahe_u16(x, c["clip"])):
            shows.add((c["shape"], c["content"], c["clip"]))
    print(sorted(shows), "outer trips at most", max(trips))
    for shape in ((1024, 1024), (120, 88)):
        assert {(k, cl) for s, k, cl in shows if s == shape} >= {(1024, 1024): {("low", 0.02), ("low", 0.1)},
                                                                 (120, 88): {("low", 0.005), ("low", 0.02), ("noise", 0.005)}}[shape], shape
    assert not any(cl in (0.0, 1.0) for _, _, cl in shows)
    assert max(trips) == 1                               # no tile of the family needs a second trip of the outer loop
