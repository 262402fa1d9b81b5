"""What tests/test_gpu_augment_sweep.py stands on, checked without a GPU (tests/augment_plans.py): the oracle's resampling against
SciPy on every (shape, family, content); the exact statements against SciPy bit for bit; the Python mirrors of the transform draw
against the C draw and Keras's matrix algebra at every plan shape; and, for each mistake the kernels could hold, the families and
shapes on which the picture moves -- with, for the H != W mistakes, the proof that nothing moves at 64 x 64."""
import numpy as np
import pytest

import augment_plans as AP
import generic_plans as GP
import train_plans as TP
from cellscreen import augment as A
from oracle import augment_oracle as ao

FAMILY_NAMES = tuple(AP.FAMILIES)


def test_shapes_cover_every_trainer_size_and_one_taller_than_wide():
    assert AP.HWS[0] == (64, 64) and len(set(AP.HWS)) == len(AP.HWS)
    assert {tuple(c[0]) for c in TP.GENERIC_CASES} <= set(AP.HWS)
    for hw, ch, n_enc in AP.SHAPES:
        assert GP.describe_trainer(hw, ch, n_enc) is None, (hw, ch)
    assert [s[0] for s in AP.TALL] == [(128, 64)] and all(hw[0] > hw[1] for hw, _, _ in AP.TALL)
    # the other transposes are 8 wide: conv_generic_supported refuses the grid (W % 16, W >= 16) under every channel list the plan knows
    assert sorted(t for t, _ in AP.TALL_REFUSED) == [(32, 8), (64, 8), (64, 32), (128, 8)]
    for t, why in AP.TALL_REFUSED:
        assert all(r is not None and r.rule.endswith("grid") for r in why), (t, why)
    assert AP.SMALLEST == (8, 32) and AP.MANY_N * 8 * 32 * 4 > 70e6


def test_contents_are_float32_in_the_unit_interval_and_tell_pixels_apart():
    for hw in AP.HWS:
        H, W = hw
        for c in AP.CONTENTS:
            img = AP.content(c, hw)
            assert img.dtype == np.float32 and img.shape == hw and 0.0 <= img.min() and img.max() <= 1.0 and not img.flags.writeable
        ramp = AP.content("ramp", hw)
        assert len(np.unique(ramp)) == H * W and np.all(np.diff(ramp.ravel()) > 0)          # any index mistake is visible
        fr = AP.content("frame", hw)
        assert fr[0, 5] != fr[1, 5] and fr[-1, 5] != fr[-2, 5] and fr[3, 0] != fr[3, 1] and fr[3, -1] != fr[3, -2]
        assert len(np.unique(AP.content("constant", hw))) == 1


def test_families_hold_what_the_plan_says():
    for hw in AP.HWS:
        H, W = hw
        for name in FAMILY_NAMES:
            fam = AP.family(name, hw)
            n = len(fam)
            assert n > 0 and fam.rows.dtype == AP.AFFINE and all(len(v) == n for v in (fam.params, fam.center, fam.frac, fam.exact, fam.note))
            assert np.isfinite(fam.rows["m"]).all() and np.isfinite(fam.rows["off"]).all()
        d = AP.draws(hw)
        assert {c for c in d.center} == {-0.5, 0.5} and {f for f in d.frac} == {(True, True), (False, False)}
        px = [p for p, note in zip(d.params, d.note) if note == "pixel shifts"]
        assert max(abs(p["tx"]) for p in px) > 3.0 >= max(abs(p["ty"]) for p in px)           # height range 5, width range 3: pixels
        assert d.rows["flip_h"].any() and d.rows["flip_v"].any() and not d.rows["identity"].any()
        lat = AP.lattice(hw)
        sh = {(e[1], e[2]) for e in lat.exact if e is not None}
        assert {(k, 0) for k in range(-(H + 1), H + 2)} <= sh and {(0, k) for k in range(-(W + 1), W + 2)} <= sh
        assert sum(1 for a, b in sh if a and b) >= 2 * H + 3 and {(H - 1, W - 1), (-(H - 1), -(W - 1)), (H + 1, -(W + 1))} <= sh
        assert {-90.0, 0.0, 90.0, 180.0} <= {p["theta"] for p in lat.params}
        assert {(1.0, 1.0), (2.0, 1.0), (1.0, 2.0), (0.5, 0.5)} <= {(p["zx"], p["zy"]) for p in lat.params}
        out = AP.outside(hw)
        assert {(np.sign(p["tx"]), np.sign(p["ty"])) for p, n_ in zip(out.params, out.note) if n_ == "pushed outside"} == \
            {(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)} - {(0, 0)}
        assert sum(1 for n_ in out.note if n_.startswith("zero matrix")) >= 9
        fl = AP.flips(hw)
        assert {(int(r["flip_h"]), int(r["flip_v"]), int(r["identity"])) for r in fl.rows} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_oracle_resampling_is_within_one_rounding_of_scipy(name):
    """ao.apply_transform / affine_nearest_order1 against scipy.ndimage.affine_transform on every (shape, family, content): within
    6e-8 everywhere; bit-identical throughout on `draws` and `keyed`; elsewhere the transforms and pixels that are not are counted
    (DESIGN.md holds the counts: they sit where a rotation or a zoom puts sample points on the lattice)."""
    n_tf = n_px = tf_diff = px_diff = 0
    worst = 0.0
    for hw in AP.HWS:
        fam = AP.family(name, hw)
        want = AP.expected(name, hw)
        for ci, c in enumerate(AP.CONTENTS):
            img = AP.content(c, hw)
            for k in range(len(fam)):
                if fam.params[k] is not None and name != "keyed":           # from the Keras parameters; raw and keyed rows from their packed matrix
                    got = ao.apply_transform(img, fam.params[k], fam.center[k])
                    if ci == 0:                                             # ... which is the same matrix: the same bits
                        assert np.array_equal(got, AP.oracle_apply(img, fam.rows[k])), (hw, name, k)
                else:
                    got = AP.oracle_apply(img, fam.rows[k])
                ref = want[ci * len(fam) + k]
                d = got != ref
                n_tf += 1; n_px += d.size
                if d.any():
                    tf_diff += 1; px_diff += int(d.sum())
                    worst = max(worst, float(np.abs(got.astype(np.float64) - ref).max()))
    print(f"\naugment oracle vs SciPy, {name}: {tf_diff} of {n_tf} (content, transform) pairs and {px_diff} of {n_px} pixels differ, worst {worst:.3e}")
    assert worst <= AP.BAR
    if name in ("draws", "keyed"):
        assert tf_diff == 0


def test_exact_statements_are_scipy_bit_for_bit():
    """The integer-shift gather img[clip(r + tx), clip(c + ty)] on all of lattice's shift cases, and the named pixel / the replicated
    edge of `outside`, against SciPy."""
    n = 0
    for hw in AP.HWS:
        for name in ("lattice", "outside"):
            fam = AP.family(name, hw)
            want = AP.expected(name, hw)
            ex = AP.exact_expected(fam)
            assert len(ex) == len(AP.CONTENTS) * sum(e is not None for e in fam.exact)
            for i, pic in ex:
                assert np.array_equal(pic, want[i]), (hw, name, i % len(fam), fam.exact[i % len(fam)])
                n += 1
        lat = AP.lattice(hw)
        assert sum(e is not None for e in lat.exact) >= 2 * (2 * hw[0] + 3) + (2 * hw[1] + 3)
    assert n > 10000
    # the gather is what it says, on a picture small enough to write down
    img = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert np.array_equal(AP.shift_gather(img, 1, -2), [[4, 4, 4, 5], [8, 8, 8, 9], [8, 8, 8, 9]])


def _replay(arrays):
    class Replay:                      # hands the arrays out in the order random_transforms asks for them
        def __init__(self):
            self.seq = list(arrays)

        def uniform(self, lo, hi, size=None):
            v = self.seq.pop(0)
            assert len(v) == size and (v >= lo).all() and (v <= hi).all()
            return v
    return Replay()


def test_python_mirrors_match_the_c_draw_and_the_keras_matrix_at_every_shape():
    """keyed_transforms, cs_train_draw_transforms and random_transforms against affine() on the same parameters, at every plan shape
    (the tall one included) for the wide, the centre +0.5 and the pixel-shift generator: 1e-12 on the matrix, 1e-10 on the offset."""
    for hw in AP.HWS:
        H, W = hw
        for name, g in AP.GENERATORS:
            for seed, step in AP.KEYS:
                n = AP.KEYED_N
                py, c = g.keyed_transforms(seed, step, n, hw), A.draw_transforms_c(g, seed, step, n, hw)
                for k, p in enumerate(AP.keyed_params(g, seed, step, n, hw)):
                    m, off = g.affine(p, H, W)
                    for rows in (py, c):
                        assert np.abs(rows["m"][k] - np.ravel(m)).max() <= 1e-12 and np.abs(rows["off"][k] - off).max() <= 1e-10, (hw, name, seed, k)
                        assert (rows["flip_h"][k], rows["flip_v"][k], rows["identity"][k]) == (p["flip_h"], p["flip_v"], 0)
            n = 40
            rng = np.random.default_rng(H + W)
            r, hs, ws, (zl, zh) = g.rotation_range, g.height_shift_range, g.width_shift_range, g.zoom_range
            th, tx, ty = rng.uniform(-r, r, n), rng.uniform(-hs, hs, n), rng.uniform(-ws, ws, n)
            zx, zy, u1, u2 = rng.uniform(zl, zh, n), rng.uniform(zl, zh, n), rng.uniform(0, 1, n), rng.uniform(0, 1, n)
            arr = g.random_transforms(n, hw, _replay([th, tx, ty, zx, zy, u1, u2]))
            for i in range(n):
                p = dict(theta=th[i], tx=tx[i] * (H if hs < 1 else 1.0), ty=ty[i] * (W if ws < 1 else 1.0), zx=zx[i], zy=zy[i],
                         flip_h=u1[i] < .5, flip_v=u2[i] < .5)
                m, off = g.affine(p, H, W)
                assert np.abs(arr["m"][i] - np.ravel(m)).max() <= 1e-12 and np.abs(arr["off"][i] - off).max() <= 1e-10, (hw, name, i)
                assert arr["flip_h"][i] == int(p["flip_h"]) and arr["flip_v"][i] == int(p["flip_v"]) and arr["identity"][i] == 0
        # the family the GPU test runs is these rows, in this order
        kp, kc = AP.keyed(hw), AP.keyed(hw, c_draw=True)
        assert len(kp) == len(kc) == len(AP.GENERATORS) * len(AP.KEYS) * AP.KEYED_N
        assert np.abs(kp.rows["m"] - kc.rows["m"]).max() <= 1e-12 and np.abs(kp.rows["off"] - kc.rows["off"]).max() <= 1e-10


_ORACLE = {}


def _oracle_pictures(name, hw, contents):
    key = (name, hw)
    if key not in _ORACLE:
        fam = AP.family(name, hw)
        _ORACLE[key] = {(c, k): AP.oracle_apply(AP.content(c, hw), fam.rows[k]) for c in contents for k in AP.mutant_subset(fam)}
    return _ORACLE[key]


MUTANT_CONTENTS = ("noise", "ramp", "frame")


def _moves(mistake, name, hw):
    fam = AP.family(name, hw)
    base = _oracle_pictures(name, hw, MUTANT_CONTENTS)
    worst = 0.0
    for (c, k), ref in base.items():
        got = AP.mutant_apply(AP.content(c, hw), fam, k, mistake)
        worst = max(worst, float(np.abs(got.astype(np.float64) - ref).max()))
    return worst


def test_the_restatement_without_a_mistake_is_the_oracle_bit_for_bit():
    for hw in AP.HWS:
        for name in FAMILY_NAMES:
            fam = AP.family(name, hw)
            assert _moves(None, name, hw) == 0.0, (hw, name)
            for k in AP.mutant_subset(fam):
                if fam.params[k] is not None:
                    a, b = AP.matrix_with(fam.params[k], hw[0], hw[1], fam.center[k]), ao.affine_matrix(fam.params[k], hw[0], hw[1], fam.center[k])
                    assert (a is None and b is None) or (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    fam = AP.lattice((8, 32))                               # the mutants run on a stride through the integer shifts and on every other row
    sub = AP.mutant_subset(fam)
    assert len(sub) < len(fam) and {0, len(fam) - 1} <= set(sub) and {k for k, e in enumerate(fam.exact) if e is None} <= set(sub)


@pytest.mark.parametrize("mistake", list(AP.MISTAKES))
def test_each_mistake_moves_its_families_and_the_rectangular_ones_move_nothing_at_64x64(mistake):
    """The oracle with one mistake switched in, against the oracle: on which (family, shape) some pixel moves by more than 100 x the
    bar.  MUST_MOVE is asserted; the mistakes that are mistakes only when H != W leave every picture at 64 x 64 bit-identical, which
    is why the square cases were not enough; r0 without its cap moves nothing anywhere (augment_plans.MUST_MOVE says why)."""
    table = {(name, hw): _moves(mistake, name, hw) for name in FAMILY_NAMES for hw in AP.HWS}
    print(f"\n{mistake} ({AP.MISTAKES[mistake]}): worst |mutant - oracle|")
    for name in FAMILY_NAMES:
        print(f"  {name:8s} " + "  ".join(f"{AP.shape_id(hw)} {table[name, hw]:.1e}" for hw in AP.HWS))
    for name, which in AP.MUST_MOVE[mistake].items():
        for hw in AP.shapes_of(which):
            assert table[name, hw] > AP.MOVED, (mistake, name, hw, table[name, hw])
    if mistake in AP.RECT_ONLY:
        assert all(table[name, (64, 64)] == 0.0 for name in FAMILY_NAMES)
        assert any(AP.MUST_MOVE[mistake].values())
    if mistake == "r0_uncapped":
        assert all(v == 0.0 for v in table.values())
    # a family the table does not name for this mistake is not claimed to see it
    assert set(AP.MUST_MOVE[mistake]) <= set(FAMILY_NAMES)


def test_every_mistake_but_the_invisible_one_is_seen_at_a_rectangular_shape_by_some_family():
    assert set(AP.MUST_MOVE) == set(AP.MISTAKES) and set(AP.RECT_ONLY) <= set(AP.MISTAKES) and set(AP.MATRIX_MISTAKES) <= set(AP.MISTAKES)
    assert [m for m in AP.MISTAKES if not AP.MUST_MOVE[m]] == ["r0_uncapped"]
    assert AP.RECT and any(hw[0] > hw[1] for hw in AP.RECT) and any(hw[0] < hw[1] for hw in AP.RECT)


def test_fit_step_plan_gathers_out_of_order_with_repeats_and_both_ends():
    for hw in AP.HWS:
        x = AP.fit_train_set(hw)
        assert x.shape == (AP.FIT_TRAIN,) + hw and x.dtype == np.float32 and 0 <= x.min() and x.max() <= 1
        assert len({x[k].tobytes() for k in range(AP.FIT_TRAIN)}) == AP.FIT_TRAIN          # a crop gathered from the wrong index is a different crop
    for b in AP.FIT_BATCHES + tuple(set(AP.SEQ_FIT_BATCHES)):
        for step in AP.FIT_STEPS:
            idx = AP.fit_idx(b, step)
            assert idx.dtype == np.int32 and idx.shape == (b,) and idx.min() >= 0 and idx.max() < AP.FIT_TRAIN
            if b >= 8:
                assert 0 in idx and AP.FIT_TRAIN - 1 in idx and len(set(idx.tolist())) < b and np.any(np.diff(idx) < 0)
    assert AP.fit_idx(1, 0)[0] == 0 and AP.fit_idx(1, 1249)[0] == AP.FIT_TRAIN - 1


def _ring(n_slots, sizes):
    """PinnedRing<N>::acquire (train_internal.hpp) on a sequence of byte counts: per call (slot, reused a slot whose event is pending,
    reallocated)."""
    slot_bytes, used, nxt, out = 0, [False] * n_slots, 0, []
    for b in sizes:
        grew = b > slot_bytes
        if grew:
            slot_bytes, used = b, [False] * n_slots
        cur, nxt = nxt, (nxt + 1) % n_slots
        out.append((cur, used[cur], grew))
        used[cur] = True
    return out


def test_sequences_wrap_the_rings_before_and_after_they_grow():
    aug = _ring(8, [64 * n for n in AP.SEQ_AUG_N])
    assert len(aug) == 24 and [k for k, (_, _, g) in enumerate(aug) if g] == [0, 12]
    assert [k for k, (_, r, _) in enumerate(aug) if r] == [8, 9, 10, 11, 20, 21, 22, 23]        # a slot handed out again: before the growth and after
    fit = _ring(16, [68 * b for b in AP.SEQ_FIT_BATCHES])
    assert len(fit) == 20 and [k for k, (_, _, g) in enumerate(fit) if g] == [0, 17]
    assert [k for k, (_, r, _) in enumerate(fit) if r] == [16]
    for call, n in enumerate(AP.SEQ_AUG_N):
        rows = AP.seq_rows(AP.SEQ_SHAPE, call, n)
        assert rows.dtype == AP.AFFINE and len(rows) == n and not rows["identity"].any()
    assert not np.array_equal(AP.seq_rows(AP.SEQ_SHAPE, 3, 4)["m"], AP.seq_rows(AP.SEQ_SHAPE, 11, 4)["m"])


def test_many_images_are_the_prototypes_gathered_by_the_map():
    crops, rows, imap = AP.many_plan()
    hw = AP.SMALLEST
    assert crops.shape == (AP.MANY_PROTOS,) + hw and crops.dtype == np.float32 and 0 <= crops.min() and crops.max() <= 1
    assert imap.shape == (AP.MANY_N,) and set(imap.tolist()) == set(range(AP.MANY_PROTOS))
    assert len({c.tobytes() for c in crops}) == AP.MANY_PROTOS
    assert all(not rows["identity"][imap[i]] for i in AP.MANY_MARKED) and len({int(imap[i]) for i in AP.MANY_MARKED}) == len(AP.MANY_MARKED)
    want = AP.many_expected()
    assert all(not np.array_equal(want[imap[i]], crops[imap[i]]) for i in AP.MANY_MARKED)
    x, tf = crops[imap], rows[imap]
    assert x.nbytes > 70e6
    for i in list(range(300)) + list(range(AP.MANY_N - 300, AP.MANY_N)):
        assert np.array_equal(want[imap[i]], AP.scipy_apply(x[i], tf[i])), i
