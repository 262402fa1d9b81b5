"""tests/pipeline_reference.py held to what it is composed from, without a device: its cases cover every pair of option levels the
package accepts, it returns what the per-stage device tests compose by hand pair by pair, and on its scenes no stage of any case
is idle, so that tests/test_gpu_pipeline.py cannot pass with a stage that does nothing."""
import functools

import numpy as np
import pytest
from scipy import ndimage

import background_reference as BR
import clean_reference as CR
import expand_reference as ER
import hysteresis_reference as HR
import local_reference as LR
import noise_reference as NR
import pipeline_reference as P
import segment_reference as R
import smooth_reference as MR
import split_intensity_reference as IR
import split_reference as SR

fill = ndimage.binary_fill_holes


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def test_cases_are_the_generator_s_and_cover_every_allowed_pair():
    assert P.CASES == P.generate()
    assert all(P.allowed(c) for c in P.CASES) and len(set(P.CASES)) == len(P.CASES)
    want = P.all_allowed_pairs()
    got = set().union(*(P.pairs_of(c) for c in P.CASES))
    assert got == want
    # every pair of levels of two factors is allowed, but for the median without a stage to run in
    every = {((a, u), (b, v)) for a in range(len(P.FACTORS)) for b in range(a + 1, len(P.FACTORS))
             for u in P.FACTORS[a][1] for v in P.FACTORS[b][1]}
    assert every == want
    assert not P.allowed((0, 0, 1, "otsu", 0, "off", 1, 1, "off", 0, "uint8"))
    assert not P.allowed((0, 0, 1, "noise", 0, "off", 1, 1, "off", 0, "uint8"))
    assert P.allowed((0, 0, 1, "local", 0, "off", 1, 1, "off", 0, "uint8"))


def test_one_full_chain_per_rule_and_shapes_in_rotation():
    for k, rule in enumerate(("otsu", "fixed", "local", "noise")):
        c = dict(zip(P.NAMES, P.CASES[k]))
        assert c["rule"] == rule and c["smooth"] and c["correct"] and c["denoise"] and c["weak"] and c["clean"] == "both"
        assert c["fill"] and c["split"] != "off" and c["expand"]
    shapes = [P.options(c, i)[1] for i, c in enumerate(P.CASES)]
    assert shapes[:4] == [s for s, _ in P.SHAPES] and all(shapes[i] == shapes[i % 4] for i in range(len(shapes)))
    for i, c in enumerate(P.CASES):
        kw, (H, W), _ = P.options(c, i)
        if kw.get("threshold") == "noise":
            assert H // kw["noise_tile"] >= 2 and W // kw["noise_tile"] >= 2      # two mesh tiles a side
    weak = {k for c in P.CASES for k in P.options(c, 0)[0] if k.startswith("weak")}
    assert weak == {"weak_threshold", "weak_delta", "weak_k"}
    kinds = {type(P.options(c, 0)[0]["weak_threshold"]) for c in P.CASES if "weak_threshold" in P.options(c, 0)[0]}
    assert kinds == {int, float}                                                  # counts and a fraction


# ---- agreement with the compositions that the per-stage device tests write out by hand -------------------------------------------
@pytest.fixture(scope="module")
def imgs():
    x = P.scene((67, 131), np.uint16, 3)
    x.setflags(write=False)
    return x


def per_image(imgs, one):
    """[(labels, n, threshold, heights or None)] of a hand composition image by image, stacked as segment_batch stacks them."""
    out = [one(np.ascontiguousarray(x)) for x in imgs]
    res = [np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int32)]
    if len(out[0]) > 3:
        res.append(np.stack([o[3] for o in out]))
    return res


def agree(imgs, one, **kw):
    want = per_image(imgs, one)
    got = P.segment_batch(imgs, return_distance=len(want) == 4, **kw)
    assert len(got) == len(want) + 1
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), kw
    assert (got[1] >= 2).all(), kw
    return got


NOISE = dict(threshold="noise", noise_tile=32, noise_k=6.0, weak_k=3.0)
NREF = dict(T=32, k8=1536, weak8=768)


def test_single_stages_are_their_own_restatements(imgs):
    for kw in (dict(), dict(connectivity=2, fill_holes=False), dict(threshold=20000)):
        want = R.segment_batch(imgs, **kw)
        got = P.segment_batch(imgs, **kw)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[3] == {}
    want = BR.segment_batch(imgs, 11, False, connectivity=2)
    assert all(np.array_equal(g, w) for g, w in zip(P.segment_batch(imgs, background_radius=11, connectivity=2), want))
    agree(imgs, lambda x: LR.segment(x, 13, 5000, -1, True, 2, False), threshold="local", local_radius=13, local_delta=5000,
          denoise=True, connectivity=2, fill_holes=False)
    want = HR.segment_batch(imgs, threshold="otsu", weak_threshold=0.5, connectivity=2)
    assert all(np.array_equal(g, w) for g, w in zip(P.segment_batch(imgs, weak_threshold=0.5, connectivity=2), want))
    agree(imgs, lambda x: HR.segment_local(x, 13, 8000, 3000, -1, False, 1, True), threshold="local", local_radius=13,
          local_delta=8000, weak_delta=3000)
    agree(imgs, lambda x: NR.segment(x, **NREF), **NOISE)
    want = SR.split_batch(imgs, connectivity=2, h=2)
    got = P.segment_batch(imgs, return_distance=True, split_touching=True, split_h=2, connectivity=2)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    agree(imgs, lambda x: (ER.expand(R.segment(x)[0], ER.max_d2_of(3))[0],) + R.segment(x)[1:], expand_distance=3)


def test_smoothing_in_front(imgs):
    # test_gpu_smooth.py: the Gaussian (with the median, once) before Otsu, before the correction, before local + cleanup + split
    for med in (False, True):
        agree(imgs, lambda x: R.segment(MR.smooth_sigma(x, 1.5, med)), smooth_sigma=1.5, denoise=med)
        agree(imgs, lambda x: R.segment(BR.correct(MR.smooth_sigma(x, 1.5, med), 11, False)), smooth_sigma=1.5, denoise=med,
              background_radius=11)

    def local_clean_split(x):
        s = MR.smooth_sigma(x, 1.5, True)
        m = CR.clean(fill(LR.local_mask(s, 13, 4000) > 0), 1, 2, 30, 1) > 0
        lab, n, dq = SR.split_mask(m, 1, 3)
        return lab, n, -1, dq

    agree(imgs, local_clean_split, smooth_sigma=1.5, denoise=True, threshold="local", local_radius=13, local_delta=4000, open_radius=1,
          min_area=30, split_touching=True)


def test_correction_in_front(imgs):
    # test_gpu_background.py / test_gpu_local.py / test_gpu_clean.py: the top-hat before the split, the local rule, the cleanup
    def split(x):
        lab, n, t, dq = SR.split(BR.correct(x, 11, True))
        return lab, n, t, dq

    agree(imgs, split, background_radius=11, denoise=True, split_touching=True)
    agree(imgs, lambda x: LR.segment(BR.correct(x, 11, True), 13, 4000, -1, False), background_radius=11, denoise=True,
          threshold="local", local_radius=13, local_delta=4000)                  # the median ran in the correction, not again

    def cleaned(x):
        p = BR.correct(x, 11, False)
        t = R.otsu(p)
        return R.label_mask(CR.clean(R.mask_of(p, t, True), 2, 1, 25, 2) > 0, 2) + (t,)

    agree(imgs, cleaned, background_radius=11, open_radius=2, open_connectivity=1, min_area=25, connectivity=2)


def test_cleanup_between_the_hole_filling_and_the_labels(imgs):
    # test_gpu_clean.py: the split and the labels see the cleaned mask, the thresholds are the uncleaned call's
    def split(x):
        t = R.otsu(x)
        lab, n, dq = SR.split_mask(CR.clean(R.mask_of(x, t, True), 1, 2, 30, 1) > 0, 1, 3)
        return lab, n, t, dq

    got = agree(imgs, split, open_radius=1, min_area=30, split_touching=True)
    assert np.array_equal(got[2], R.segment_batch(imgs)[2])
    agree(imgs, lambda x: R.label_mask(CR.clean(fill(LR.local_mask(x, 13, 4000) > 0), None, 2, 30, 1) > 0, 1) + (-1,),
          threshold="local", local_radius=13, local_delta=4000, min_area=30)
    # the cleaned plane is cut at 0, not at the image's threshold again: a fixed threshold above 1 would leave nothing
    x = np.zeros((1, 20, 20), np.uint8)
    x[0, 3:17, 3:17] = 200
    x[0, 1, 1] = 200                                       # and a speck that the opening takes
    lab, n, thr = P.segment_batch(x, threshold=100, open_radius=1)[:3]
    assert n[0] == 1 and thr[0] == 100 and lab[0, 5, 5] == 1 and lab[0, 1, 1] == 0 and (lab > 0).sum() == 14 * 14


def test_hysteresis_in_the_rule_s_place(imgs):
    # test_gpu_hysteresis.py: behind smoothing and correction, in front of hole filling and cleanup, under both splits
    def front(x):
        plane, t = HR.hysteresis_global(BR.correct(MR.smooth_sigma(x, 1.5), 11, False), "otsu", 0.3, 1)
        return LR.label_plane(plane, 1, True)[:2] + (t,)

    got = agree(imgs, front, smooth_sigma=1.5, background_radius=11, weak_threshold=0.3)
    assert np.array_equal(got[2], P.segment_batch(imgs, smooth_sigma=1.5, background_radius=11)[2])      # the strong rule's
    for kw in (dict(), dict(min_area=30), dict(open_radius=2, open_connectivity=1, min_area=60, connectivity=2)):
        c = kw.get("connectivity", 1)

        def behind(x):
            filled = fill(HR.hysteresis(HR.levels_local(x, 13, 8000, 3000), c) > 0)
            m = CR.clean(filled, kw.get("open_radius"), kw.get("open_connectivity", 2), kw.get("min_area"), c) if kw else filled
            return R.label_mask(m > 0, c) + (-1,)

        got = agree(imgs, behind, threshold="local", local_radius=13, local_delta=8000, weak_delta=3000, **kw)
        planes = got[-1]
        for b, x in enumerate(imgs):
            assert np.array_equal(planes["hysteresis_mask_batch"][b], HR.hysteresis(HR.levels_local(x, 13, 8000, 3000), c))
            assert np.array_equal(planes["local_mask_batch"][b], LR.local_mask(x, 13, 8000))

    def split(x):
        plane, t = HR.hysteresis_global(x, 22000, 15000, 1)
        lab, n, dq = SR.split_mask(plane > 0, 1, 3)
        return lab, n, t, dq

    agree(imgs, split, threshold=22000, weak_threshold=15000, fill_holes=False, split_touching=True)
    for kw in (dict(weak_threshold=0.5), dict(threshold="local", local_radius=13, local_delta=8000, weak_delta=3000)):
        def guided(x):
            s = MR.smooth_sigma(x, 1.5)
            plane, t = HR.hysteresis_global(s, "otsu", 0.5, 1) if "weak_threshold" in kw else \
                (HR.hysteresis(HR.levels_local(s, 13, 8000, 3000), 1), -1)
            lab, n, hq = IR.split_intensity(fill(plane > 0), s, 1, 16, 0)
            return lab, n, t, hq

        agree(imgs, guided, split_touching=True, split_by="intensity", smooth_sigma=1.5, **kw)


def test_noise_rule_with_the_other_stages(imgs):
    # test_gpu_noise.py::test_with_the_other_stages, composition by composition
    agree(imgs, lambda x: NR.segment(MR.smooth_sigma(x, 1.5), **NREF), smooth_sigma=1.5, **NOISE)
    agree(imgs, lambda x: NR.segment(BR.correct(x, 12, False), **NREF), background_radius=12, **NOISE)
    agree(imgs, lambda x: R.label_mask(CR.clean(fill(NR.noise_mask(x, 32, 640) > 0), None, 2, 12, 1) > 0, 1) + (-1,),
          threshold="noise", noise_tile=32, noise_k=2.5, min_area=12)

    def split(x):
        lab, n, dq = SR.split_mask(fill(NR.noise_mask(x, **NREF) > 0), 1, 3)
        return lab, n, -1, dq

    agree(imgs, split, split_touching=True, **NOISE)

    def guided(x):
        s = MR.smooth_sigma(x, 1.5)
        lab, n, hq = IR.split_intensity(fill(NR.noise_mask(s, **NREF) > 0), s, 1, 16, 0)
        return lab, n, -1, hq

    agree(imgs, guided, split_touching=True, split_by="intensity", smooth_sigma=1.5, **NOISE)


def test_split_intensity_reference_s_own_composition(imgs):
    # split_intensity_reference.segment_batch composes smoothing, correction, the local rule and the cleanup itself
    for kw in (dict(smooth_sigma=1.5), dict(background_radius=11, denoise=True),
               dict(smooth_sigma=1.5, denoise=True, threshold="local", local_radius=13, local_delta=4000, min_area=30, open_radius=1),
               dict(threshold=20000, connectivity=2, fill_holes=False)):
        want = IR.segment_batch(imgs, **kw)[:4]
        got = P.segment_batch(imgs, return_distance=True, split_touching=True, split_by="intensity", **kw)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), kw
    three = np.stack([imgs, imgs[::-1], imgs], axis=-1)                          # channel 2 by default, any on request
    assert np.array_equal(P.segment_batch(three)[0], P.segment_batch(imgs)[0])
    assert np.array_equal(P.segment_batch(three, channel=1)[0], P.segment_batch(imgs[::-1])[0])


def test_growth_comes_last_and_leaves_the_counts_and_heights(imgs):
    kw = dict(split_touching=True, min_area=30)
    plain = P.segment_batch(imgs, return_distance=True, **kw)
    grown = P.segment_batch(imgs, return_distance=True, expand_distance=3, **kw)
    assert np.array_equal(grown[0], ER.expand(plain[0], ER.max_d2_of(3))[0]) and (grown[0] != plain[0]).any()
    assert all(np.array_equal(grown[k], plain[k]) for k in (1, 2, 3))


def test_arguments():
    x = np.zeros((1, 8, 8), np.uint8)
    with pytest.raises(TypeError):
        P.segment_batch(x, sigma=2)
    with pytest.raises(ValueError):
        P.segment_batch(x, return_distance=True)
    with pytest.raises(ValueError):
        P.segment_batch(x, denoise=True)                                         # no stage to run the median in


# ---- no stage is idle ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_of(shape, dtype, index):
    x = P.scene(shape, np.dtype(dtype).type, index)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def labels_of(case, index):
    kw, shape, dtype = P.options(case, index)
    return P.segment_batch(scene_of(shape, np.dtype(dtype).name, index), **kw)[:2]


def without(case):
    """[(stage, the case with that one stage off)]; a median whose only host goes is taken off with it."""
    c = dict(zip(P.NAMES, case))
    out = []

    def off(name, **change):
        d = dict(c, **change)
        if d["denoise"] and not (d["smooth"] or d["correct"] or d["rule"] == "local"):
            d["denoise"] = 0
        out.append((name, tuple(d[n] for n in P.NAMES)))

    for name in ("smooth", "correct", "denoise", "weak", "fill", "expand"):
        if c[name]:
            off(name, **{name: 0})
    if c["clean"] == "both":
        off("opening", clean="area")
        off("min_area", clean="open")
    elif c["clean"] != "off":
        off("cleanup", clean="off")
    if c["split"] != "off":
        off("split", split="off")
    return out


@pytest.mark.parametrize("index", range(len(P.CASES)))
def test_no_stage_is_idle(index):
    case = P.CASES[index]
    lab, n = labels_of(case, index)
    assert (n >= 3).all(), (case, n)
    for stage, other in without(case):
        assert not np.array_equal(labels_of(other, index)[0], lab), (case, stage)
