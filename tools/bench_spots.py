"""Throughput of the spot detector (cs_spot_detect / cs_spot_fill, cellscreen/spots.py, csrc/spots.hip) and writes
profiles/spots_bench.json.  The workload is the label tools': --images fields of 2048 x 2048 with 640 cells each
(synth.label_images), channel 2 (the bright cells) as uint16, resident on the device; the objects are the painted labels grown by 6 px
(LabelExpander); --puncta synthetic puncta per field (a 3 x 3 bump of 16000 counts at the centre, about 12 sigmas of the fields' pixel noise) are added inside the objects.
The threshold is 4 sigmas of the pixel noise through dog_noise_gain, the noise estimated from the horizontal first differences of
one field (1.4826 MAD / sqrt 2).  A 512 x 640 crop of one field is compared with tests/spots_reference.py in every configuration
first.  Then for sigma 1 and 2 (coarse 1.6 sigma), min_distance 2 and 5, without and with labels:

  response_ms_per_image, peaks_ms_per_image, records_ms_per_image   HIP-event times of the three stages: median and [min, max]
  call_ms_per_image             detect_dense, wall clock: the stages, the tables and the list to the host
  spots_per_image
  smooth2_ms_per_image          two cs_segment_smooth calls (ThresholdSegmenter.smooth_batch) with the same two tables on the same
                                fields, their smooth_ms summed, same run
  response_ratio_to_two_smooths response_ms / smooth2_ms: the fused response reads the image once and writes one plane where the
                                two calls read it twice and write two
  intensity_pass_ms_per_image   cs_label_intensity's pass on the same fields and labels, same run
  ratio_to_intensity_pass       (response + peaks + records) / intensity_pass
  dense_peaks_ms_per_image, dense_records_ms_per_image, dense_spots_per_image   without labels: the same call at a threshold of
                                1/256 count, where every positive response is a candidate and the list is as long as it gets
  host_scipy_ms_per_image       the SciPy form on --host-images of the fields: gaussian_filter twice (float64), maximum_filter, the
                                comparison and a gather by label (np.bincount)
No time is a pass condition.

Usage: python tools/bench_spots.py [--images 8] [--side 2048] [--cells 640] [--puncta 2500] [--reps 10] [--warmup 2] [--host-images 1]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cell-image-analysis_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GROW = 6
SIGMAS = (1.0, 2.0)
RATIO = 1.6
DISTANCES = (2, 5)
CROP = (512, 640)
STAGES = ("response", "peaks", "records")


def add_puncta(plane, inside, n, rng):
    """n bumps of 16000 / 6000 / 2500 counts (centre, edge, corner of a 3 x 3) at random pixels of `inside`, away from the border."""
    rr, cc = np.nonzero(inside[1:-1, 1:-1])
    pick = rng.choice(len(rr), size=min(n, len(rr)), replace=False)
    f = plane.astype(np.int64)
    for dr, dc, v in ((0, 0, 16000), (0, 1, 6000), (0, -1, 6000), (1, 0, 6000), (-1, 0, 6000), (1, 1, 2500), (1, -1, 2500), (-1, 1, 2500), (-1, -1, 2500)):
        np.add.at(f, (rr[pick] + 1 + dr, cc[pick] + 1 + dc), v)
    return np.clip(f, 0, 65535).astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=640)
    ap.add_argument("--puncta", type=int, default=2500)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-images", type=int, default=1)
    a = ap.parse_args()

    import torch
    from scipy import ndimage as ndi

    import spots_reference as SR
    from build import source_hash
    from cellscreen import expand as EX
    from cellscreen import intensity as IN
    from cellscreen import segment as SG
    from cellscreen import spots as SP
    from cellscreen import synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_spots needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    span = lambda v: [float(np.min(v)), float(np.max(v))]
    imgs, labs = synth.label_images(2024, a.images, hw=(a.side, a.side), n_cells=a.cells)
    tl = torch.from_numpy(labs).to(dev)
    grown = EX.LabelExpander(0).expand_batch(tl, GROW)
    h_grown = grown.cpu().numpy()
    max_label = int(labs.max())
    rng = np.random.default_rng(7)
    h_img = np.stack([add_puncta(np.ascontiguousarray(imgs[b, :, :, 2]), h_grown[b] > 0, a.puncta, rng) for b in range(a.images)])
    t_img = torch.from_numpy(h_img.view(np.int16)).to(dev)
    d = np.diff(h_img[0].astype(np.float64), axis=1)
    noise_sd = 1.4826 * float(np.median(np.abs(d - np.median(d)))) / np.sqrt(2.0)
    det, inten = SP.SpotDetector(0), IN.IntensityMeasurer(0)

    def timed(fn, timing):
        walls, stages = [], []
        for k in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= a.warmup:
                walls.append(time.perf_counter() - t0)
                stages.append(timing())
        return walls, stages

    res = {"tool": "bench_spots", "source_hash": source_hash(), "images": a.images, "side": a.side, "cells": a.cells, "puncta": a.puncta,
           "reps": a.reps, "warmup": a.warmup, "pixel_type": "uint16", "grown_by": GROW, "max_label": max_label, "noise_sd": noise_sd,
           "labelled_fraction": float((h_grown > 0).mean()),
           "checked": "every output on a 512 x 640 crop of one field equals tests/spots_reference.py in every configuration", "configs": []}
    _, i_stages = timed(lambda: inten.measure_dense(t_img, grown, max_label=max_label), inten.last_timing)
    ipass = med([s["intensity_pass_ms"] / a.images for s in i_stages])
    crop_i = np.ascontiguousarray(h_img[:1, :CROP[0], :CROP[1]])
    crop_l = np.ascontiguousarray(h_grown[:1, :CROP[0], :CROP[1]])
    for sigma in SIGMAS:
        smooth2 = 0.0
        for s in (sigma, RATIO * sigma):
            seg = SG.ThresholdSegmenter(0, smooth_sigma=s)
            _, s_stages = timed(lambda: seg.smooth_batch(t_img), seg.last_timing)
            smooth2 += med([x["smooth_ms"] / a.images for x in s_stages])
            seg.close()
        for m in DISTANCES:
            p = SP.spot_params(sigma, RATIO, min_distance=m)
            thr = max(4.0 * noise_sd * SP.dog_noise_gain(p), 1.0 / 256.0)
            T = int(round(thr * 256))
            wa, wb = SP.tables_of(p)
            for with_labels in (False, True):
                lab_c, lab_t = (crop_l, grown) if with_labels else (None, None)
                got = det.detect_dense(crop_i, thr, lab_c, None, max_label if with_labels else None, p, True)
                want = SR.detect(crop_i, [T], wa, wb, m, 0, lab_c, None, max_label if with_labels else None)
                if not all((g is None and w is None) or np.array_equal(g, w) for g, w in zip(got, want)):
                    raise SystemExit(f"the outputs differ from tests/spots_reference.py at sigma {sigma}, min_distance {m}, labels {with_labels}")
                host = []
                for b in range(min(a.host_images, a.images)):
                    t0 = time.perf_counter()
                    x = h_img[b].astype(np.float64)
                    dog = ndi.gaussian_filter(x, sigma, mode="reflect") - ndi.gaussian_filter(x, RATIO * sigma, mode="reflect")
                    peak = (dog == ndi.maximum_filter(dog, 2 * m + 1, mode="constant", cval=-np.inf)) & (dog >= thr)
                    if with_labels:
                        np.bincount(h_grown[b][peak], minlength=max_label + 1)
                    host.append(time.perf_counter() - t0)
                kw = dict(labels=lab_t, max_label=max_label if with_labels else None, params=p)
                n_spots = int(det.detect_dense(t_img, thr, **kw)[0][:, 0].sum())
                walls, stages = timed(lambda: det.detect_dense(t_img, thr, **kw), det.last_timing)
                per = {k: [s[f"spot_{k}_ms"] / a.images for s in stages] for k in STAGES}
                total = [sum(x) for x in zip(*per.values())]
                cfg = {"sigma": sigma, "sigma_coarse": RATIO * sigma, "radius_a": p.radius_a, "radius_b": p.radius_b, "min_distance": m,
                       "labels": with_labels, "threshold_counts": thr, "spots_per_image": n_spots / a.images}
                for k, v in per.items():
                    cfg[f"{k}_ms_per_image"] = med(v)
                    cfg[f"{k}_ms_per_image_range"] = span(v)
                cfg.update({"device_ms_per_image": med(total), "call_ms_per_image": 1e3 * med(walls) / a.images,
                            "smooth2_ms_per_image": smooth2, "response_ratio_to_two_smooths": med(per["response"]) / smooth2,
                            "intensity_pass_ms_per_image": ipass, "ratio_to_intensity_pass": med(total) / ipass,
                            "host_images": len(host), "host_scipy_ms_per_image": 1e3 * med(host)})
                if not with_labels:                     # the same call at the lowest threshold: every positive response is a candidate
                    n_dense = int(det.detect_dense(t_img, 1.0 / 256.0, params=p)[0][:, 0].sum())
                    _, d_stages = timed(lambda: det.detect_dense(t_img, 1.0 / 256.0, params=p), det.last_timing)
                    cfg.update({"dense_spots_per_image": n_dense / a.images,
                                "dense_peaks_ms_per_image": med([s["spot_peaks_ms"] / a.images for s in d_stages]),
                                "dense_records_ms_per_image": med([s["spot_records_ms"] / a.images for s in d_stages])})
                res["configs"].append(cfg)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "spots_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
