"""The rule of cs_label_granularity restated in numpy and SciPy: whole planes, no tiles, no rounds in groups and no
tables in between, so that it shares nothing with the kernels.

An object is the set of pixels of one image with one label > 0, connected or not, less the pixels where `exclude` is non-zero; a
pixel's effective label is 0 where `exclude` is set.  With s = subsample, Hs = ceil(H / s), Ws = ceil(W / s), per channel:

    P[R][C]   = (2 * sum v + n) // (2 * n) over the in-image pixels of the s x s block, n their count; with masked a pixel whose
                effective label is 0 contributes v = 0 and still counts in n
    E_k       = the erosion of E_(k-1) by the 3 x 3 cross, E_0 = P, neighbours outside the plane ignored
                (scipy.ndimage.grey_erosion(E, footprint=CROSS, mode='reflect'))
    R_k       = the reconstruction by dilation of E_k under P with the cross: the fixed point of R <- min(max over the cross of R,
                P) from R = E_k; R_0 = P

    geom       [B, max_label, 3]            int64   area, sum r, sum c (cs_label_intensity's)
    sums       [B, max_label, steps+1, C]   int64   the sum over the object's pixels (r, c) of R_k[r // s][c // s]
    image_sums [B, steps+1, C]              int64   the sum of R_k over the working plane
    planes     [B, steps+1, C, Hs, Ws]      uint16  the R_k

reconstruct() iterates whole planes to the fixed point; reconstruct_by_thresholds() is the independent slow form by threshold
decomposition: R(p) is the largest t such that p's 4-connected component of {P >= t} (scipy.ndimage.label) holds a pixel with
E >= t.  derive() takes the spectrum from the integers with Fractions."""
from fractions import Fraction

import numpy as np
from scipy import ndimage as ndi

import intensity_reference as IR

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
MAX_STEPS = 64
SUBSAMPLES = (1, 2, 4, 8)


def working_plane(image, labels, exclude, subsample, masked):
    """image [B,H,W,C], labels and exclude [B,H,W] -> P uint16 [B,C,Hs,Ws]."""
    B, H, W, C = image.shape
    s = subsample
    hs, ws = -(-H // s), -(-W // s)
    v = image.astype(np.int64)
    if masked:
        v = v * ((labels != 0) & (exclude == 0))[..., None]
    tot = np.zeros((B, hs * s, ws * s, C), np.int64)
    cnt = np.zeros((hs * s, ws * s), np.int64)
    tot[:, :H, :W] = v
    cnt[:H, :W] = 1
    tot = tot.reshape(B, hs, s, ws, s, C).sum(axis=(2, 4))
    cnt = cnt.reshape(hs, s, ws, s).sum(axis=(1, 3))[None, :, :, None]
    return np.ascontiguousarray(((2 * tot + cnt) // (2 * cnt)).transpose(0, 3, 1, 2)).astype(np.uint16)


def _neighbours(a, fill):
    """the four cross neighbours of every pixel of a [H,W], `fill` outside the plane"""
    p = np.pad(a, 1, constant_values=fill)
    return p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]


def erode(e):
    """One erosion of a plane [H,W] by the cross, neighbours outside ignored."""
    e = e.astype(np.int64)
    return np.minimum.reduce((e,) + _neighbours(e, 1 << 20))


def reconstruct(e, p):
    """The reconstruction by dilation of e under p (e <= p), planes [H,W]: whole-plane rounds to the fixed point."""
    p = p.astype(np.int64)
    r = e.astype(np.int64)
    assert (r <= p).all()
    while True:
        n = np.minimum(np.maximum.reduce((r,) + _neighbours(r, -1)), p)
        if np.array_equal(n, r):
            return r
        r = n


def reconstruct_by_thresholds(e, p):
    """The same by threshold decomposition, for tiny planes with few levels."""
    e, p = e.astype(np.int64), p.astype(np.int64)
    r = np.full(p.shape, -1, np.int64)
    for t in np.unique(np.concatenate([e.reshape(-1), p.reshape(-1)])):
        comp, _ = ndi.label(p >= t, structure=CROSS)
        hit = np.unique(comp[(e >= t) & (comp > 0)])
        r[np.isin(comp, hit) & (comp > 0)] = t          # t rises: the largest one stays
    assert (r >= 0).all()
    return r


def spectrum_planes(p, steps, recon=reconstruct):
    """R_0..R_steps of one working plane [Hs,Ws] -> int64 [steps+1,Hs,Ws]."""
    out = [p.astype(np.int64)]
    e = p
    for _ in range(steps):
        e = erode(e)
        out.append(recon(e, p))
    return np.stack(out)


def measure(image, labels, exclude=None, steps=16, subsample=1, masked=False, max_label=None):
    """(geom, sums, image_sums, planes) of image [B,H,W] or [B,H,W,C], labels [B,H,W] and exclude (None or [B,H,W])."""
    image, labels, exclude, max_label = IR._planes(image, labels, exclude, max_label)
    if not 1 <= steps <= MAX_STEPS or subsample not in SUBSAMPLES:
        raise ValueError("steps must be 1..64 and subsample 1, 2, 4 or 8")
    B, H, W, C = image.shape
    s = subsample
    P = working_plane(image, labels, exclude, s, masked)
    planes = np.stack([np.stack([spectrum_planes(P[b, ch], steps) for ch in range(C)], axis=1) for b in range(B)])      # [B,K+1,C,Hs,Ws]
    geom = IR.measure(image, labels, exclude, max_label)[0]
    sums = np.zeros((B, max_label, steps + 1, C), np.int64)
    eff = np.where(exclude != 0, 0, labels)
    for b in range(B):
        rr, cc = np.nonzero(eff[b] > 0)
        if rr.size == 0:
            continue
        lab = eff[b][rr, cc]
        vals = planes[b][:, :, rr // s, cc // s]         # [K+1,C,n]
        for k in range(steps + 1):
            for ch in range(C):
                sums[b, :, k, ch] = _bin_sum(lab, vals[k, ch], max_label)
    return geom, sums, planes.sum(axis=(3, 4)), planes.astype(np.uint16)


def _bin_sum(lab, v, max_label):
    """sum of the int64 values v per label 1..max_label, exact (no float weights)"""
    order = np.argsort(lab, kind="stable")
    lab, v = lab[order], v[order]
    starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
    out = np.zeros(max_label, np.int64)
    out[lab[starts] - 1] = np.add.reduceat(v, starts)
    return out


def _spectrum(v):
    """S_0..S_K as Python ints -> the K values 100 (S_(k-1) - S_k) / S_0, each a correctly rounded Fraction; NaN where S_0 = 0"""
    if v[0] == 0:
        return [float("nan")] * (len(v) - 1)
    return [float(Fraction(100 * (v[k - 1] - v[k]), v[0])) for k in range(1, len(v))]


def derive(geom, sums, image_sums):
    """The present objects in (image, label) order as a dict of arrays: image, label, area, start_mean [n,C], spectrum [n,K,C],
    image_spectrum [B,K,C], geom [n,3], sums [n,K+1,C], image_sums [B,K+1,C]."""
    B, M, K1, C = sums.shape
    keys = [(b, m) for b in range(B) for m in range(M) if geom[b, m, 0] > 0]
    n = len(keys)
    out = dict(image=np.array([b for b, _ in keys], np.int32).reshape(n), label=np.array([m + 1 for _, m in keys], np.int32).reshape(n),
               area=np.zeros(n, np.int64), start_mean=np.full((n, C), np.nan), spectrum=np.full((n, K1 - 1, C), np.nan),
               image_spectrum=np.full((B, K1 - 1, C), np.nan), geom=np.zeros((n, 3), np.int64), sums=np.zeros((n, K1, C), np.int64),
               image_sums=np.array(image_sums, np.int64).reshape(B, K1, C))
    for i, (b, m) in enumerate(keys):
        a = int(geom[b, m, 0])
        out["area"][i] = a
        out["geom"][i] = geom[b, m]
        out["sums"][i] = sums[b, m]
        for ch in range(C):
            v = [int(x) for x in sums[b, m, :, ch]]
            if v[0] != 0:
                out["start_mean"][i, ch] = float(Fraction(v[0], a))
            out["spectrum"][i, :, ch] = _spectrum(v)
    for b in range(B):
        for ch in range(C):
            out["image_spectrum"][b, :, ch] = _spectrum([int(x) for x in image_sums[b, :, ch]])
    return out
