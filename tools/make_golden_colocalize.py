"""Generates tests/golden/golden_colocalize.npz: small scenes measured by SciPy and by boolean masks, the outside witness of
tests/colocalize_reference.py (cs_label_colocalize).

    python tools/make_golden_colocalize.py

SciPy 1.15.3 / numpy 2.2.6 wrote the committed file.  Per case i (one image), with `index` the labels present once the pixels
under `exclude` are taken out, C channels and the P pairs (a, b), a < b, in lexicographic order:
    image_i     uint8 / uint16 [H,W,C]     labels_i   int32 [H,W]     exclude_i   int32 [H,W] (all zero: none)
    rule_i      int64 [2 + C]: num, den of the fraction of the object's maximum, then the absolute thresholds, -1 each where the
                other rule holds
    index_i     int32 [n]
    pearson_i   float64 [n,P]: scipy.stats.pearsonr(v_a, v_b).statistic over the object's pixels as float64 (NaN where SciPy
                reports a constant input)
    slope_i     float64 [n,P]: scipy.stats.linregress(v_a, v_b).slope (NaN where SciPy refuses identical x values)
    levels_i    int32 [C]: the distinct values of the channel on the object pixels
    rank_i      int32 [H,W,C]: scipy.stats.rankdata(method='dense') - 1 of the channel over the object pixels, -1 elsewhere
    chan_i      int64 [n,C,5], pair_i  int64 [n,P,9]: the records of tests/colocalize_reference.py, by a boolean mask per object
    name_i
n_cases counts them.  scipy_pearson_distance and scipy_slope_distance: the largest distance of SciPy's floats from the 50-digit
decimal form of the same integers (colocalize_reference.derive_decimal) over all cases -- |r - r_exact|, and
|slope - slope_exact| / sqrt(d_b / d_a), the slope in units of the spreads' ratio.  The tests compare SciPy's floats at twice
these distances: the error is SciPy's."""
import os
import sys
import warnings

import numpy as np
import scipy
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import colocalize_reference as CR                                              # noqa: E402
import expand_reference as ER                                                  # noqa: E402
import intensity_reference as IR                                               # noqa: E402


def scipy_table(image, labels, exclude, threshold=(15, 100), absolute=None):
    """SciPy and boolean masks on one image [H,W,C]."""
    lab = np.where(exclude != 0, 0, labels)
    index = np.unique(lab[lab > 0]).astype(np.int32)
    C = image.shape[2]
    pp = CR.pairs_of(C)
    on = lab > 0
    rank = np.full(image.shape, -1, np.int32)
    levels = np.zeros(C, np.int32)
    for c in range(C):
        rank[:, :, c][on] = stats.rankdata(image[:, :, c][on], method="dense") - 1
        levels[c] = len(set(image[:, :, c][on].tolist()))
    n = len(index)
    out = dict(index=index, pearson=np.full((n, len(pp)), np.nan), slope=np.full((n, len(pp)), np.nan), levels=levels, rank=rank,
               chan=np.zeros((n, C, 5), np.int64), pair=np.zeros((n, len(pp), 9), np.int64))
    for k, label in enumerate(index):
        m = lab == label
        v = [image[:, :, c][m].astype(np.int64) for c in range(C)]
        if absolute is None:
            up = [v[c] * threshold[1] >= threshold[0] * v[c].max() for c in range(C)]
        else:
            up = [v[c] >= absolute[c] for c in range(C)]
        for c in range(C):
            out["chan"][k, c] = v[c].sum(), (v[c] ** 2).sum(), v[c].max(), up[c].sum(), v[c][up[c]].sum()
        for p, (a, b) in enumerate(pp):
            x, y = v[a].astype(np.float64), v[b].astype(np.float64)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out["pearson"][k, p] = stats.pearsonr(x, y).statistic
                try:
                    out["slope"][k, p] = stats.linregress(x, y).slope
                except ValueError:
                    pass                                                        # identical x values
            both = up[a] & up[b]
            w = max(levels[a], levels[b]) - np.abs(rank[:, :, a][m].astype(np.int64) - rank[:, :, b][m])
            va, vb, w = v[a][both], v[b][both], w[both]
            out["pair"][k, p] = ((v[a] * v[b]).sum(), both.sum(), va.sum(), vb.sum(), (va * va).sum(), (vb * vb).sum(), (va * vb).sum(),
                                 (va * w).sum(), (vb * w).sum())
    return out


def special_scene():
    """24 x 40 uint8, 3 channels, four rectangles: 1 with channel 1 constant, 2 with channel 2 all zero, 3 without a pixel above
    in both of channels 0 and 1, 4 plain."""
    rng = np.random.default_rng(11)
    lab = np.zeros((24, 40), np.int32)
    img = rng.integers(60, 256, (24, 40, 3)).astype(np.uint8)
    lab[2:10, 2:14] = 1
    img[2:10, 2:14, 1] = 7
    lab[2:10, 20:36] = 2
    img[2:10, 20:36, 2] = 0
    lab[14:22, 2:14] = 3
    img[14:22, 2:8, 0] = rng.integers(200, 256, (8, 6))
    img[14:22, 2:8, 1] = rng.integers(0, 10, (8, 6))
    img[14:22, 8:14, 0] = rng.integers(0, 10, (8, 6))
    img[14:22, 8:14, 1] = rng.integers(200, 256, (8, 6))
    lab[14:22, 20:36] = 4
    return img, lab


def cases():
    """(name, image, labels, exclude, threshold, absolute)"""
    a = ER.disks((48, 100), 14, 1)
    nuclei = ER.disks((40, 64), 7, 3, radii=(2, 4))
    grown = ER.expand(nuclei, 16)[0]
    b = ER.disks((40, 60), 8, 2)
    base = IR.noise(b.shape, 1, np.uint16, 6, base=5000, spread=40000)[..., 0].astype(np.int64)
    mixed = np.stack([base, base // 2 + IR.noise(b.shape, 1, np.uint16, 7, spread=9000)[..., 0]], axis=-1).astype(np.uint16)
    img, lab = special_scene()
    return [("48x100 disks, uint16 noise, 3 channels", IR.noise(a.shape, 3, np.uint16, 5), a, np.zeros_like(a), (15, 100), None),
            ("40x64 rings: grown cells less their nuclei, uint8, 4 channels", IR.noise(grown.shape, 4, np.uint8, 7), grown, nuclei, (15, 100), None),
            ("40x60 disks, uint16, channel 1 follows channel 0, absolute thresholds", mixed, b, np.zeros_like(b), None, [20000, 12000]),
            ("24x40 rectangles: a constant channel, a dark channel, no pixel above in both", img, lab, np.zeros_like(lab), (15, 100), None)]


def scipy_distance(image, labels, exclude, threshold, absolute, t):
    """(pearson, slope): the largest distance of SciPy's floats in t from the decimal form (the module's docstring)"""
    geom, chan, pair, levels = CR.measure(image[None], labels[None], exclude[None], None, threshold or (15, 100), absolute)
    dec = CR.derive_decimal(geom, chan, pair, levels)
    d = CR.derive(geom, chan, pair, levels)
    worst = [0.0, 0.0]
    for k in range(len(t["index"])):
        a = int(d["area"][k])
        for p, (i, j) in enumerate(CR.pairs_of(image.shape[2])):
            if dec["pearson"][k][p] is not None and not np.isnan(t["pearson"][k, p]):
                worst[0] = max(worst[0], abs(float(dec["pearson"][k][p] - _dec(t["pearson"][k, p]))))
            if dec["slope"][k][p] is not None and not np.isnan(t["slope"][k, p]):
                di = a * int(d["chan"][k, i, 1]) - int(d["chan"][k, i, 0]) ** 2
                dj = a * int(d["chan"][k, j, 1]) - int(d["chan"][k, j, 0]) ** 2
                unit = (dj / di) ** 0.5 if dj else 1.0
                worst[1] = max(worst[1], abs(float(dec["slope"][k][p] - _dec(t["slope"][k, p]))) / unit)
    return worst


def _dec(x):
    import decimal
    return decimal.Decimal(float(x))


def main():
    out = {}
    cs = cases()
    worst = [0.0, 0.0]
    for i, (name, image, labels, exclude, threshold, absolute) in enumerate(cs):
        t = scipy_table(image, labels, exclude, threshold or (15, 100), absolute)
        dist = scipy_distance(image, labels, exclude, threshold, absolute, t)
        worst = [max(a, b) for a, b in zip(worst, dist)]
        C = image.shape[2]
        rule = np.array(list(threshold or (-1, -1)) + list(absolute or [-1] * C), np.int64)
        print(f"{name}: {len(t['index'])} objects, {image.dtype} x {C}, smallest object {int(t['chan'][:, 0, 3].min())} pixels above in "
              f"channel 0; SciPy's distance: pearson {dist[0]:.3e}, slope {dist[1]:.3e}")
        out.update({f"name_{i}": name, f"image_{i}": image, f"labels_{i}": labels.astype(np.int32), f"exclude_{i}": exclude.astype(np.int32),
                    f"rule_{i}": rule})
        out.update({f"{k}_{i}": v for k, v in t.items()})
    out["n_cases"] = np.int64(len(cs))
    out["scipy_version"] = scipy.__version__
    out["numpy_version"] = np.__version__
    out["scipy_pearson_distance"] = np.float64(worst[0])
    out["scipy_slope_distance"] = np.float64(worst[1])
    print(f"SciPy's largest distance from the 50-digit form: pearson {worst[0]:.3e}, slope {worst[1]:.3e}")
    path = os.path.join(ROOT, "tests", "golden", "golden_colocalize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
