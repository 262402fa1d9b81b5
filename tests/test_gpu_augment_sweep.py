"""The training augmentation's kernels (csrc/train.hip: augment_kernel behind cs_train_augment, fit_gather_kernel behind
cs_train_fit_step) on every trainer shape and every transform family of tests/augment_plans.py, against
scipy.ndimage.affine_transform(order=1, mode="nearest") + flips within one float32 rounding (6e-8) and, where the plan has a
statement with no rounding in it, bit for bit; the pinned rings behind back-to-back calls; 70,000 crops in one call.
tests/test_augment_plans_cpu.py proves on the CPU that each family fails on the mistakes it is there for."""
import time

import numpy as np
import pytest

import augment_plans as AP
from cellscreen import _lib as L
from cellscreen import synth
from cellscreen.augment import draw_transforms_c
from cellscreen.trainer import Trainer

pytestmark = pytest.mark.gpu

SHAPE_OF = {s[0]: s for s in AP.SHAPES}
_REPORT = {}                      # family -> [worst |kernel - SciPy|, bit-identical pixels, pixels]


def _new_trainer(hw):
    hw, ch, n_enc = SHAPE_OF[tuple(hw)]
    return Trainer(synth.random_cae(seed=12, hw=hw, channels=ch, n_enc=n_enc, trivial_bn=True))


@pytest.fixture(scope="module")
def trainers():
    """One trainer per (shape, role), built on first use and closed at the end of the module."""
    made = {}

    def get(hw, role="main"):
        key = (tuple(hw), role)
        if key not in made:
            made[key] = _new_trainer(hw)
        return made[key]
    yield get
    for t in made.values():
        t.close()


def _check_pictures(got, n, hw):
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (n,) + tuple(hw)
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0


def _against_scipy(got, want, family, what):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    per = err.reshape(len(err), -1).max(axis=1)
    rec = _REPORT.setdefault(family, [0.0, 0, 0])
    rec[0] = max(rec[0], float(per.max(initial=0.0)))
    rec[1] += int((got == want).sum()); rec[2] += got.size
    print(f"\n{what}: worst |kernel - SciPy| {per.max(initial=0.0):.3e}, bit-identical {(got == want).mean():.6f} of {got.size} pixels")
    assert per.max(initial=0.0) <= AP.BAR, f"{what}: image {int(per.argmax())} is off by {per.max():.3e}"


@pytest.mark.parametrize("name", list(AP.FAMILIES))
@pytest.mark.parametrize("hw", AP.HWS, ids=AP.shape_id)
def test_augment_kernel_on_every_shape_family_and_content(trainers, hw, name):
    """Every content under every transform of the family in ONE call, host in/out: against SciPy within 6e-8, against the exact
    statements of `lattice` and `outside` bit for bit; device in/out gives the same bits.  `keyed` runs the Python mirror's rows and
    cs_train_draw_transforms' own."""
    import torch
    t = trainers(hw)
    for kw in ({}, {"c_draw": True}) if name == "keyed" else ({},):
        fam = AP.family(name, hw, **kw)
        x, rows = AP.batch(fam)
        got = t.augment(x, rows)
        _check_pictures(got, len(x), hw)
        _against_scipy(got, AP.expected(name, hw, **kw), name, f"{AP.shape_id(hw)} {name}{' (C draw)' if kw else ''}, {len(x)} images")
        for i, pic in AP.exact_expected(fam):
            assert np.array_equal(got[i], pic), (i % len(fam), fam.exact[i % len(fam)], AP.CONTENTS[i // len(fam)])
        dev = t.augment(torch.from_numpy(x).cuda(), rows)
        assert dev.is_cuda and dev.dtype == torch.float32 and np.array_equal(dev.cpu().numpy(), got)
        assert not np.array_equal(got, x)
    if name == "flips":                       # the ctypes form of the same transforms (ImageDataGenerator.pack): the same bits
        packed = (L.CSAugAffine * len(rows)).from_buffer_copy(rows.tobytes())
        assert np.array_equal(t.augment(x, packed), got)


@pytest.mark.parametrize("gi", range(len(AP.GENERATORS)), ids=[g[0].replace(" ", "_").replace(",", "") for g in AP.GENERATORS])
@pytest.mark.parametrize("hw", AP.HWS, ids=AP.shape_id)
def test_fit_step_gathers_and_resamples_what_the_plan_says(trainers, hw, gi):
    """cs_train_fit_step's own input and target, read back (cs_train_tensor 5 and 6): y is train[idx] bit for bit; x is SciPy's picture
    of train[idx] under cs_train_draw_transforms(seed, step) within 6e-8, and the stand-alone kernel's (Trainer.augment on a second
    trainer) bit for bit; without a generator x is y."""
    import torch
    name, g = AP.GENERATORS[gi]
    a, b = trainers(hw, "fit"), trainers(hw, "twin")
    train = AP.fit_train_set(hw)
    dev = torch.from_numpy(train).cuda()
    for bs in AP.FIT_BATCHES:
        for step in AP.FIT_STEPS:
            idx = AP.fit_idx(bs, step)
            a.fit_step(dev, idx, g.config(), seed=AP.FIT_SEED, step=step, lr=1e-3)
            y, x = a.tensor(6, 0, bs), a.tensor(5, 0, bs)
            assert np.array_equal(y, train[idx]), (bs, step)
            _check_pictures(x, bs, hw)
            rows = draw_transforms_c(g, AP.FIT_SEED, step, bs, hw)
            want = np.stack([AP.scipy_apply(im, r) for im, r in zip(train[idx], rows)])
            _against_scipy(x, want, "fit_step", f"{AP.shape_id(hw)} fit_step {name}, batch {bs}, step {step}")
            assert np.array_equal(x, b.augment(train[idx], rows)), (bs, step)
            assert not np.array_equal(x, y)
    idx = AP.fit_idx(33, 7)
    a.fit_step(dev, idx, None, seed=AP.FIT_SEED, step=7, lr=1e-3)
    y, x = a.tensor(6, 0, 33), a.tensor(5, 0, 33)
    assert np.array_equal(y, train[idx]) and np.array_equal(x, y)
    with pytest.raises(L.CellScreenError):
        a.tensor(5, 1, 33)                       # the input and the target have no layer


def test_24_device_calls_back_to_back_keep_their_own_transforms():
    """(a) 24 cs_train_augment calls on device memory with no host wait between them, each with its own transforms and its own output;
    the ring of pinned slots hands a slot out again at call 9, is reallocated at call 13 (64 images after 4) and wraps again at call
    21.  All outputs are compared afterwards."""
    import torch
    hw = AP.SEQ_SHAPE
    t, ref = _new_trainer(hw), _new_trainer(hw)
    try:
        xs = [AP.seq_input(hw, k, n) for k, n in enumerate(AP.SEQ_AUG_N)]
        tfs = [AP.seq_rows(hw, k, n) for k, n in enumerate(AP.SEQ_AUG_N)]
        dx = [torch.from_numpy(x).cuda() for x in xs]
        torch.cuda.synchronize()
        outs = [t.augment(d, tf) for d, tf in zip(dx, tfs)]
        got = [o.cpu().numpy() for o in outs]
        for k, (x, tf, g) in enumerate(zip(xs, tfs, got)):
            _check_pictures(g, len(x), hw)
            want = np.stack([AP.scipy_apply(im, r) for im, r in zip(x, tf)])
            _against_scipy(g, want, "sequence", f"call {k + 1} of 24, {len(x)} images")
            assert np.array_equal(g, ref.augment(x, tf)), k
    finally:
        t.close(); ref.close()


def test_20_fit_steps_back_to_back_are_the_twin_fed_by_augment_and_step_async():
    """(b) 20 cs_train_fit_step calls with batches 8 x 17, 40, 8, 8 and no host wait: the ring of 16 pinned slots wraps at step 17 and
    is reallocated at step 18.  Weights and moving statistics equal, bit for bit, those of a twin fed by Trainer.augment +
    step_async; x and y of the last step are read back."""
    import torch
    hw = AP.SEQ_SHAPE
    g = AP.GENERATORS[0][1]
    a, b = _new_trainer(hw), _new_trainer(hw)
    try:
        train = AP.fit_train_set(hw)
        dev = torch.from_numpy(train).cuda()
        idxs = [AP.fit_idx(bs, 100 + k) for k, bs in enumerate(AP.SEQ_FIT_BATCHES)]
        torch.cuda.synchronize()
        for k, idx in enumerate(idxs):
            a.fit_step(dev, idx, g.config(), seed=AP.FIT_SEED, step=k, lr=1e-3)
        for k, idx in enumerate(idxs):
            yb = dev[torch.from_numpy(idx.astype(np.int64)).cuda()].contiguous()
            xb = b.augment(yb, draw_transforms_c(g, AP.FIT_SEED, k, len(idx), hw))
            b.step_async(xb, yb, 1e-3)
        n = len(idxs[-1])
        assert np.array_equal(a.tensor(6, 0, n), train[idxs[-1]]) and np.array_equal(a.tensor(5, 0, n), xb.cpu().numpy())
        (pa, ma), (pb, mb) = a.export_flat(), b.export_flat()
        assert np.isfinite(pa).all() and np.array_equal(pa, pb) and np.array_equal(ma, mb)
        assert a.read_metrics() == b.read_metrics()
    finally:
        a.close(); b.close()


def test_host_device_host_on_one_trainer_is_each_call_alone():
    """(c) a host call, a device call and a host call on one trainer give the bits each gives alone on a fresh trainer."""
    import torch
    hw = AP.SEQ_SHAPE
    calls = [(AP.seq_input(hw, 40 + k, n), AP.seq_rows(hw, 40 + k, n), on_device) for k, (n, on_device) in enumerate(((9, False), (33, True), (5, False)))]

    def run(t, x, tf, on_device):
        return t.augment(torch.from_numpy(x).cuda(), tf).cpu().numpy() if on_device else t.augment(x, tf)
    t = _new_trainer(hw)
    try:
        together = [run(t, *c) for c in calls]
    finally:
        t.close()
    for c, got in zip(calls, together):
        alone = _new_trainer(hw)
        try:
            assert np.array_equal(run(alone, *c), got)
        finally:
            alone.close()
        want = np.stack([AP.scipy_apply(im, r) for im, r in zip(c[0], c[1])])
        assert np.abs(got.astype(np.float64) - want).max() <= AP.BAR


def test_70000_crops_in_one_call(trainers):
    """cs_train_augment has no batch cap: 70,000 crops of the smallest shape (72 MB) in one call, 16 prototype (crop, transform) pairs
    spread by a seeded map with non-identity ones at images 0, 65,534, 65,535, 65,536 and 69,999."""
    hw = AP.SMALLEST
    crops, rows, imap = AP.many_plan()
    x, tf = np.ascontiguousarray(crops[imap]), np.ascontiguousarray(rows[imap])
    t0 = time.perf_counter()
    got = trainers(hw).augment(x, tf)
    print(f"\n70,000 crops: {time.perf_counter() - t0:.3f} s")
    _check_pictures(got, AP.MANY_N, hw)
    want = AP.many_expected()[imap]
    _against_scipy(got, want, "many", f"{AP.shape_id(hw)}, {AP.MANY_N} images")
    for i in AP.MANY_MARKED:
        assert not np.array_equal(got[i], x[i])


@pytest.mark.parametrize("hw", AP.HWS, ids=AP.shape_id)
def test_no_images_give_an_empty_array_of_the_trainers_size(trainers, hw):
    import torch
    t = trainers(hw)
    for tf in (np.zeros(0, AP.AFFINE), (L.CSAugAffine * 0)()):
        out = t.augment(np.zeros((0,) + tuple(hw), np.float32), tf)
        assert isinstance(out, np.ndarray) and out.shape == (0,) + tuple(hw) and out.dtype == np.float32
    out = t.augment(torch.zeros((0,) + tuple(hw), device="cuda"), np.zeros(0, AP.AFFINE))
    assert out.is_cuda and tuple(out.shape) == (0,) + tuple(hw)


def test_report_per_family():
    """The figures DESIGN.md quotes: worst |kernel - SciPy| and the share of bit-identical pixels per family (reported, not asserted:
    the bar is asserted where each picture is compared)."""
    for name, (worst, same, total) in _REPORT.items():
        print(f"\nfamily {name}: worst {worst:.3e}, bit-identical {same / max(total, 1):.8f} of {total} pixels ({total - same} differ)")
    if set(AP.FAMILIES) <= set(_REPORT):                       # the whole file ran, not one node of it
        assert all(v[0] <= AP.BAR for v in _REPORT.values())
