"""Throughput of the built-in segmenter (cellscreen.segment, csrc/segment.hip) on tools/bench_extract.py's workload: 32 images
of 2048 x 2048 x 3 uint16 (synth.label_images, about 1,000 cells each), resident on the device.  Prints one JSON line and
writes it to profiles/segment_bench.json:

  segment_images_per_s                  segmentation alone (one library call, wall clock), median of --reps
  threshold_ms, label_ms                HIP-event times of histogram + Otsu + mask, and of hole filling + labelling + renumbering:
                                        median and [min, max] over the repetitions
  segment_extract_images_per_s          segmentation + extraction to the [n,64,64] cells, labels never leaving the device
  host_path_images_per_s                the path this replaces, in the same run, on --host-images images: the image's channel
                                        on the host, the Otsu restatement + scipy.ndimage (tests/segment_reference.py), upload of
                                        the labels, CellExtractor on the device-resident image
  host_segment_images_per_s             its segmentation part alone
The device and the host path are compared on their outputs first: equal labels, equal region tables.

--split measures the split_touching option (cs_segment_split) in its place and writes profiles/segment_split_bench.json: per
workload -- the one above, and one with --split-cells cells per image, where most cells touch another -- the unsplit
segmenter's images/s of the same run, the split's images/s and its four stage times (threshold, distance, seeds, flood), the
split + extraction images/s, the ratio of the split's time to the unsplit one's, and the time of the host restatement
(tests/split_reference.py) on one image, whose labels the device's are compared with first.

--background R [--denoise] measures the background correction (cs_segment_background, ThresholdSegmenter(background_radius=R))
in its place and writes profiles/segment_background_bench.json: one image's corrected plane and labels are compared with the
host restatement (tests/background_reference.py) first; then the images/s of the segmenter without and with the correction in
the same run, their ratio, and the two new stage times (median, top-hat) at R and at the radii 8, 32 and 128 side by side,
which show whether the cost is flat in the radius.  No time is a pass condition.

--local R [--delta D] [--denoise] measures the local mean threshold (cs_segment_local, ThresholdSegmenter(threshold="local",
local_radius=R, local_delta=D)) in its place and writes profiles/segment_local_bench.json: one image's mask and labels are
compared with the host restatement (tests/local_reference.py) first; then, in the same run, the images/s of the plain Otsu
segmenter, of the segmenter with the top-hat of radius 51 (--background 51's figure) and of the local segmenter, the stage times
of each, and the local stage's time as a ratio to the top-hat's.  No time is a pass condition.

--clean [--open R] [--min-area A] [--delta D] measures the mask cleanup (cs_segment_clean, ThresholdSegmenter(open_radius=R,
min_area=A); --min-area 50 when neither is given) and writes profiles/segment_clean_bench.json.  The scene is speckled: every
image is 16 fields of tests/test_local_cpu.py's dim_cell_scene (512 x 512, 40 bright and dim cells, noise sigma 25) side by side,
cut by the local threshold of radius 25 and --delta D (60 by default).  One image's cleaned mask and labels are compared with
the host restatement (tests/clean_reference.py) first; then, in the same run, the segmenter without cleanup (what it was before
the option) and with it: images/s of segment_batch and of segment + extract, the label counts, the stage times, open_ms and
min_area_ms per image, and the ratios of the cleaned figures to the uncleaned ones; with --min-area up to the extraction's own
bound and no opening, the extracted cells are compared too.  Then open_ms alone at the radii 1, 3, 7 and 15 with both
structures, which shows what the radius costs.  No time is a pass condition.

--hysteresis [--weak-delta W] [--strong-delta D] measures the hysteresis threshold (cs_segment_hysteresis,
ThresholdSegmenter(threshold="local", local_delta=D, weak_delta=W); 40 and 200 by default) on --clean's speckled scene and
writes profiles/segment_hysteresis_bench.json.  One image's plane and labels are compared with the host restatement
(tests/hysteresis_reference.py) first; then, in the same run, three segmenters of radius 25: the local rule at delta W alone,
the same with min_area=50, and weak W / strong D: images/s of segment_batch and of segment + extract, the label counts and the
stage times of each, the two new stage times per image, and the ratios of the third to the other two.  The first two are
--clean --delta 40's configurations (profiles/segment_clean_delta40_bench.json).  No time is a pass condition.

--smooth SIGMA [--denoise] measures the Gaussian smoothing (cs_segment_smooth, ThresholdSegmenter(smooth_sigma=SIGMA)) and writes
profiles/segment_smooth_bench.json.  The scene is faint cells in noise: every image is 16 fields of
tests/test_smooth_cpu.py's faint_cell_scene (512 x 512, 40 cells of peak 250 over noise of sigma 100) side by side, cut by
Otsu's threshold.  One image's smoothed plane and labels are compared with the host restatement (tests/smooth_reference.py)
first; then, in the same run, the segmenter without smoothing (what it was before the option) and with it: images/s of
segment_batch and of segment + extract, the label counts, the stage times, smooth_ms per image, and the ratios of the smoothed
figures to the unsmoothed ones.  Then smooth_ms alone at the sigmas 0.25, 1, 2, 4, 8 and 15.875 (radii 1 to 64), which shows
what the radius costs.  No time is a pass condition.

--split-intensity measures split_by="intensity" (cs_segment_split_intensity) beside the distance split and writes
profiles/segment_split_intensity_bench.json.  The scene is a field of touching cells with bright cores: every image is
tests/split_intensity_reference.py's scene (170 x 260, 11 Gaussian cells that overlap without a neck, 5 components) tiled to
the image's size, with Gaussian noise of 60 counts, smoothed with sigma 1.5 and cut by Otsu's threshold.  One scene's labels and
heights are compared with the host restatement first (and the distance split's labels with tests/split_reference.py); then, in
the same run, split_by="distance" (--split's mode) and split_by="intensity": images/s of segment_batch and of segment + extract,
the regions found, the stage times and the host synchronisations per call.  No time is a pass condition.

--noise [--noise-k K] [--tile T] measures the noise-adaptive threshold (cs_segment_noise, ThresholdSegmenter(threshold="noise",
noise_k=K, noise_tile=T); 5 and 64 by default) in its place and writes profiles/segment_noise_bench.json.  On the scene --local
uses, one image's mesh, mask and labels are compared with the host restatement (tests/noise_reference.py) first; then, in the
same run, three segmenters: the noise rule, the local rule of radius 25 (the figure to set it beside), and the top-hat of radius
51 with Otsu, with the stage times of each in milliseconds per image.  No time is a pass condition.

--score measures the label scoring (cs_label_match, cellscreen/score.py) and writes profiles/segment_score_bench.json.  On the
scene --local uses (whose painted labels are the truth), one image's tables are compared with the host restatement
(tests/match_reference.py) first; then, in the same run: images/s of segment_batch, of LabelMatcher.match_batch on its labels
(with the two device stage times per image and the pair table's capacity), of score_batch (segment + match + the statistics),
and of the numpy restatement on --host-images images.  No time is a pass condition.

Usage: python tools/bench_segment.py [--images 32] [--side 2048] [--cells 1000] [--reps 10] [--warmup 2] [--host-images 4]
                                     [--split [--split-cells 3000] [--split-h 3]] [--background R [--denoise]]
                                     [--local R [--delta D] [--denoise]] [--clean [--open R] [--min-area A] [--delta D]] [--smooth SIGMA [--denoise]]
                                     [--split-intensity [--split-depth 16] [--split-contrast 0]]
                                     [--hysteresis [--weak-delta 40] [--strong-delta 200]] [--noise [--noise-k 5] [--tile 64]] [--score]"""
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


def split_leg(a):
    import torch
    import split_reference as SR
    from build import source_hash
    from cellscreen import extract as X
    from cellscreen import segment as S
    from cellscreen import synth

    fill = not a.no_fill_holes
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    res = {"tool": "bench_segment --split", "source_hash": source_hash(), "images": a.images, "side": a.side,
           "connectivity": a.connectivity, "fill_holes": fill, "split_h": a.split_h, "reps": a.reps, "warmup": a.warmup, "workloads": []}
    for name, cells in (("cells", a.cells), ("touching", a.split_cells)):
        imgs, _ = synth.label_images(2024, a.images, hw=(a.side, a.side), n_cells=cells)
        ti = torch.from_numpy(imgs.view(np.int16)).to(dev)
        torch.cuda.synchronize()
        ext = X.CellExtractor(0)
        plain = S.ThresholdSegmenter(0, "otsu", a.connectivity, fill, extractor=ext)
        split = S.ThresholdSegmenter(0, "otsu", a.connectivity, fill, extractor=ext, split_touching=True, split_h=a.split_h)

        def timed(fn, seg):
            walls, stages = [], []
            for k in range(a.warmup + a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                if k >= a.warmup:
                    walls.append(time.perf_counter() - t0)
                    stages.append(seg.last_timing())
            return out, walls, stages

        (_, n_plain, _), plain_walls, _ = timed(lambda: plain.segment_batch(ti), plain)
        (labels, n_split, _), split_walls, stages = timed(lambda: split.segment_batch(ti), split)
        _, plain_chain, _ = timed(lambda: ext.extract_batch(ti, plain.segment_batch(ti)[0]), plain)
        r, split_chain, _ = timed(lambda: ext.extract_batch(ti, split.segment_batch(ti)[0]), split)
        t0 = time.perf_counter()
        hl, hn, _, _ = SR.split(np.ascontiguousarray(imgs[0, ..., 2]), "otsu", a.connectivity, fill, a.split_h)
        host_s = time.perf_counter() - t0
        assert hn == int(n_split[0]) and np.array_equal(labels[0].cpu().numpy(), hl), "device labels differ from the host restatement"
        spread = lambda k: [round(med([t[k] for t in stages]), 4), round(min(t[k] for t in stages), 4), round(max(t[k] for t in stages), 4)]
        res["workloads"].append({
            "name": name, "cells_painted_per_image": cells, "components": int(n_plain.sum()), "regions_split": int(n_split.sum()),
            "cells_extracted_split": int(r.cells.shape[0]),
            "unsplit_images_per_s": round(a.images / med(plain_walls), 2), "split_images_per_s": round(a.images / med(split_walls), 2),
            "split_wall_ms": [round(med(split_walls) * 1e3, 3), round(min(split_walls) * 1e3, 3), round(max(split_walls) * 1e3, 3)],
            "threshold_ms": spread("threshold_ms"), "distance_ms": spread("distance_ms"), "seed_ms": spread("seed_ms"),
            "flood_ms": spread("flood_ms"),
            "split_over_unsplit_time": round(med(split_walls) / med(plain_walls), 2),
            "unsplit_extract_images_per_s": round(a.images / med(plain_chain), 2),
            "split_extract_images_per_s": round(a.images / med(split_chain), 2),
            "host_restatement_s_per_image": round(host_s, 2),
            "speedup_over_host_restatement": round(host_s / (med(split_walls) / a.images), 1), "outputs_equal": True})
        ext.close()
        del ti
    line = json.dumps(res)
    out = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "segment_split_bench.json")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


def split_intensity_leg(a):
    import torch
    import smooth_reference as SM
    import split_intensity_reference as IR
    import split_reference as SR
    from build import source_hash
    from cellscreen import extract as X
    from cellscreen import segment as S

    fill = not a.no_fill_holes
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    sigma, noise = 1.5, 60.0
    sh, sw = IR.SCENE_SHAPE                                                 # the scene's own margins are background: it tiles seamlessly
    field = np.tile(IR.scene(0.0).astype(np.float64), (-(-a.side // sh), -(-a.side // sw)))[:a.side, :a.side]
    base = field + np.random.default_rng(2024).normal(0.0, noise, (a.side, a.side))
    base = np.rint(np.clip(base, 0, 65535)).astype(np.uint16)
    variants = [base, base[::-1], base[:, ::-1], base[::-1, ::-1]]          # four distinct images from one painting
    imgs = np.ascontiguousarray(np.stack([variants[b % 4] for b in range(a.images)]))
    ti = torch.from_numpy(imgs.view(np.int16)).to(dev)
    torch.cuda.synchronize()
    common = dict(threshold="otsu", connectivity=a.connectivity, fill_holes=fill, smooth_sigma=sigma, split_touching=True)
    ext = X.CellExtractor(0)
    dist = S.ThresholdSegmenter(0, extractor=ext, split_h=a.split_h, **common)
    inten = S.ThresholdSegmenter(0, extractor=ext, split_by="intensity", split_depth=a.split_depth, split_contrast=a.split_contrast, **common)

    # outputs first: one scene's labels and heights against the host restatements
    one = np.ascontiguousarray(IR.scene(noise)[None])
    t1 = torch.from_numpy(one.view(np.int16)).to(dev)
    labels, n, thr, hq = inten.segment_batch(t1, return_distance=True)
    el, en, et, eh, _ = IR.segment_batch(one, threshold="otsu", connectivity=a.connectivity, fill_holes=fill, depth=a.split_depth,
                                         min_contrast=a.split_contrast, smooth_sigma=sigma)
    assert np.array_equal(n, en) and np.array_equal(thr, et) and np.array_equal(labels.cpu().numpy(), el) and \
        np.array_equal(hq.cpu().numpy(), eh), "intensity split differs from the restatement"
    dl, dn, _ = dist.segment_batch(t1)
    hl, hn, _, _ = SR.split(SM.smooth_sigma(one[0], sigma), "otsu", a.connectivity, fill, a.split_h)
    assert hn == int(dn[0]) and np.array_equal(dl[0].cpu().numpy(), hl), "distance split differs from the restatement"

    def timed(fn, seg):
        walls, stages, syncs = [], [], []
        for k in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k >= a.warmup:
                walls.append(time.perf_counter() - t0)
                stages.append(seg.last_timing())
                syncs.append(seg.last_host_syncs())
        return out, walls, stages, syncs

    spread = lambda stages, k: [round(med([t[k] for t in stages]), 4), round(min(t[k] for t in stages), 4),
                                round(max(t[k] for t in stages), 4)]
    wall3 = lambda walls: [round(med(walls) * 1e3, 3), round(min(walls) * 1e3, 3), round(max(walls) * 1e3, 3)]
    res = {"tool": "bench_segment --split-intensity", "source_hash": source_hash(), "images": a.images, "side": a.side,
           "connectivity": a.connectivity, "fill_holes": fill, "smooth_sigma": sigma, "noise_sigma": noise, "split_h": a.split_h,
           "split_depth": a.split_depth, "split_contrast": a.split_contrast, "whole_scenes_per_image": (a.side // sh) * (a.side // sw), "cells_per_scene": len(IR.CELLS),
           "scene_regions": {"distance": int(dn[0]), "intensity": int(n[0])}, "reps": a.reps, "warmup": a.warmup, "outputs_equal": True}
    legs = {}
    for name, seg in (("distance", dist), ("intensity", inten)):
        (_, n_lab, _), walls, stages, syncs = timed(lambda: seg.segment_batch(ti), seg)
        r, chain, _, _ = timed(lambda: ext.extract_batch(ti, seg.segment_batch(ti)[0]), seg)
        legs[name] = walls
        res[name] = {"regions_per_image": round(float(n_lab.mean()), 1), "cells_extracted": int(r.cells.shape[0]),
                     "segment_images_per_s": round(a.images / med(walls), 2), "segment_wall_ms": wall3(walls),
                     "segment_extract_images_per_s": round(a.images / med(chain), 2), "segment_extract_wall_ms": wall3(chain),
                     "host_syncs_per_call": [int(med(syncs)), int(min(syncs)), int(max(syncs))],
                     **{k: spread(stages, k) for k in sorted(stages[0])}}
    res["intensity_over_distance_segment_time"] = round(med(legs["intensity"]) / med(legs["distance"]), 3)
    ext.close()
    line = json.dumps(res)
    out = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "segment_split_intensity_bench.json")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


def background_leg(a):
    import torch
    import background_reference as BR
    from build import source_hash
    from cellscreen import segment as S
    from cellscreen import synth

    fill = not a.no_fill_holes
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    imgs, _ = synth.label_images(2024, a.images, hw=(a.side, a.side), n_cells=a.cells)
    ti = torch.from_numpy(imgs.view(np.int16)).to(dev)
    torch.cuda.synchronize()

    def timed(seg, fn):
        walls, stages = [], []
        for k in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(seg)
            torch.cuda.synchronize()
            if k >= a.warmup:
                walls.append(time.perf_counter() - t0)
                stages.append(seg.last_timing())
        return out, walls, stages

    spread = lambda stages, k: [round(med([t[k] for t in stages]), 4), round(min(t[k] for t in stages), 4),
                                round(max(t[k] for t in stages), 4)]
    plain = S.ThresholdSegmenter(0, "otsu", a.connectivity, fill)
    (_, n_plain, _), plain_walls, _ = timed(plain, lambda s: s.segment_batch(ti))
    plain.close()
    res = {"tool": "bench_segment --background", "source_hash": source_hash(), "images": a.images, "side": a.side,
           "connectivity": a.connectivity, "fill_holes": fill, "denoise": bool(a.denoise), "reps": a.reps, "warmup": a.warmup,
           "components_uncorrected": int(n_plain.sum()), "uncorrected_images_per_s": round(a.images / med(plain_walls), 2),
           "uncorrected_wall_ms": [round(med(plain_walls) * 1e3, 3), round(min(plain_walls) * 1e3, 3), round(max(plain_walls) * 1e3, 3)],
           "radii": []}
    for r in sorted({a.background, 8, 32, 128}):
        seg = S.ThresholdSegmenter(0, "otsu", a.connectivity, fill, background_radius=r, denoise=a.denoise)
        entry = {"radius": r}
        if r == a.background:
            # outputs first: one image's plane and labels against the host restatement
            plane = seg.correct_batch(ti[:1].contiguous())
            labels, n, thr = seg.segment_batch(ti[:1].contiguous())
            chan = np.ascontiguousarray(imgs[0, ..., 2])
            assert np.array_equal(plane[0].cpu().numpy().view(np.uint16), BR.correct(chan, r, a.denoise)), "plane differs from the restatement"
            hl, hn, ht = BR.segment(chan, r, a.denoise, "otsu", a.connectivity, fill)
            assert hn == int(n[0]) and ht == int(thr[0]) and np.array_equal(labels[0].cpu().numpy(), hl), "labels differ from the restatement"
            entry["outputs_equal"] = True
        (_, n_corr, _), walls, stages = timed(seg, lambda s: s.segment_batch(ti))
        _, plane_walls, _ = timed(seg, lambda s: s.correct_batch(ti))
        seg.close()
        entry.update({
            "components": int(n_corr.sum()), "corrected_images_per_s": round(a.images / med(walls), 2),
            "corrected_wall_ms": [round(med(walls) * 1e3, 3), round(min(walls) * 1e3, 3), round(max(walls) * 1e3, 3)],
            "corrected_over_uncorrected_time": round(med(walls) / med(plain_walls), 3),
            "correct_batch_wall_ms": [round(med(plane_walls) * 1e3, 3), round(min(plane_walls) * 1e3, 3), round(max(plane_walls) * 1e3, 3)],
            "median_ms": spread(stages, "median_ms"), "background_ms": spread(stages, "background_ms"),
            "threshold_ms": spread(stages, "threshold_ms"), "label_ms": spread(stages, "label_ms")})
        res["radii"].append(entry)
    line = json.dumps(res)
    out = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "segment_background_bench.json")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


def local_leg(a):
    import torch
    import local_reference as LR
    from build import source_hash
    from cellscreen import segment as S
    from cellscreen import synth

    fill = not a.no_fill_holes
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    imgs, _ = synth.label_images(2024, a.images, hw=(a.side, a.side), n_cells=a.cells)
    ti = torch.from_numpy(imgs.view(np.int16)).to(dev)
    torch.cuda.synchronize()

    def timed(seg, fn):
        walls, stages = [], []
        for k in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(seg)
            torch.cuda.synchronize()
            if k >= a.warmup:
                walls.append(time.perf_counter() - t0)
                stages.append(seg.last_timing())
        return out, walls, stages

    spread = lambda stages, k: [round(med([t[k] for t in stages]), 4), round(min(t[k] for t in stages), 4),
                                round(max(t[k] for t in stages), 4)]
    wall3 = lambda walls: [round(med(walls) * 1e3, 3), round(min(walls) * 1e3, 3), round(max(walls) * 1e3, 3)]
    res = {"tool": "bench_segment --local", "source_hash": source_hash(), "images": a.images, "side": a.side,
           "connectivity": a.connectivity, "fill_holes": fill, "local_radius": a.local, "local_delta": a.delta,
           "denoise": bool(a.denoise), "reps": a.reps, "warmup": a.warmup}

    plain = S.ThresholdSegmenter(0, "otsu", a.connectivity, fill)
    (_, n_plain, _), plain_walls, plain_stages = timed(plain, lambda s: s.segment_batch(ti))
    plain.close()
    res["otsu"] = {"components": int(n_plain.sum()), "images_per_s": round(a.images / med(plain_walls), 2), "wall_ms": wall3(plain_walls),
                   "threshold_ms": spread(plain_stages, "threshold_ms"), "label_ms": spread(plain_stages, "label_ms")}

    tophat = S.ThresholdSegmenter(0, "otsu", a.connectivity, fill, background_radius=TOPHAT_RADIUS)
    (_, n_top, _), top_walls, top_stages = timed(tophat, lambda s: s.segment_batch(ti))
    tophat.close()
    res["background"] = {"radius": TOPHAT_RADIUS, "components": int(n_top.sum()), "images_per_s": round(a.images / med(top_walls), 2),
                         "wall_ms": wall3(top_walls), "background_ms": spread(top_stages, "background_ms"),
                         "threshold_ms": spread(top_stages, "threshold_ms"), "label_ms": spread(top_stages, "label_ms")}

    seg = S.ThresholdSegmenter(0, "local", a.connectivity, fill, local_radius=a.local, local_delta=a.delta, denoise=a.denoise)
    # outputs first: one image's mask and labels against the host restatement
    one = ti[:1].contiguous()
    mask = seg.local_mask_batch(one)
    labels, n, thr = seg.segment_batch(one)
    chan = np.ascontiguousarray(imgs[0, ..., 2])
    assert np.array_equal(mask[0].cpu().numpy(), LR.local_mask(chan, a.local, a.delta, -1, a.denoise)), "mask differs from the restatement"
    hl, hn, _ = LR.segment(chan, a.local, a.delta, -1, a.denoise, a.connectivity, fill)
    assert hn == int(n[0]) and int(thr[0]) == -1 and np.array_equal(labels[0].cpu().numpy(), hl), "labels differ from the restatement"
    (_, n_loc, _), walls, stages = timed(seg, lambda s: s.segment_batch(ti))
    _, mask_walls, _ = timed(seg, lambda s: s.local_mask_batch(ti))
    seg.close()
    px = a.images * a.side * a.side
    local_ms, top_ms = med([t["local_ms"] for t in stages]), med([t["background_ms"] for t in top_stages])
    res["local"] = {"outputs_equal": True, "components": int(n_loc.sum()), "images_per_s": round(a.images / med(walls), 2),
                    "wall_ms": wall3(walls), "local_mask_batch_wall_ms": wall3(mask_walls),
                    "local_median_ms": spread(stages, "local_median_ms"), "local_ms": spread(stages, "local_ms"),
                    "threshold_ms": spread(stages, "threshold_ms"), "label_ms": spread(stages, "label_ms"),
                    "local_ns_per_pixel": round(local_ms * 1e6 / px, 4)}
    res["local_over_tophat_stage_time"] = round(local_ms / top_ms, 3)
    res["local_over_otsu_wall_time"] = round(med(walls) / med(plain_walls), 3)
    line = json.dumps(res)
    out = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "segment_local_bench.json")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


NOISE_LOCAL_RADIUS = 25                                 # the local rule that --noise is set beside


def noise_leg(a):
    import torch
    import noise_reference as NR
    from build import source_hash
    from cellscreen import segment as S
    from cellscreen import synth

    fill = not a.no_fill_holes
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    imgs, _ = synth.label_images(2024, a.images, hw=(a.side, a.side), n_cells=a.cells)
    ti = torch.from_numpy(imgs.view(np.int16)).to(dev)
    torch.cuda.synchronize()

    def timed(seg):
        walls, stages = [], []
        for k in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = seg.segment_batch(ti)
            torch.cuda.synchronize()
            if k >= a.warmup:
                walls.append(time.perf_counter() - t0)
                stages.append(seg.last_timing())
        return out, walls, stages

    def row(out, walls, stages):
        per_image = {k: round(med([t[k] for t in stages]) / a.images, 5) for k in stages[0]}
        return dict(components=int(out[1].sum()), images_per_s=round(a.images / med(walls), 2),
                    wall_ms_per_image=[round(f(walls) * 1e3 / a.images, 4) for f in (med, min, max)], stage_ms_per_image=per_image)

    res = {"tool": "bench_segment --noise", "source_hash": source_hash(), "images": a.images, "side": a.side,
           "connectivity": a.connectivity, "fill_holes": fill, "noise_k": a.noise_k, "noise_tile": a.tile, "reps": a.reps,
           "warmup": a.warmup}
    seg = S.ThresholdSegmenter(0, "noise", a.connectivity, fill, noise_k=a.noise_k, noise_tile=a.tile)
    # outputs first: one image's mesh, mask and labels against the host restatement
    one = ti[:1].contiguous()
    chan = np.ascontiguousarray(imgs[0, ..., 2])
    k8 = NR.k8_of(a.noise_k)
    assert np.array_equal(seg.noise_mesh_batch(one)[0], NR.mesh(chan, a.tile, 256)), "mesh differs from the restatement"
    assert np.array_equal(seg.noise_mask_batch(one)[0].cpu().numpy(), NR.noise_mask(chan, a.tile, k8)), "mask differs from the restatement"
    labels, n, thr = seg.segment_batch(one)
    hl, hn, _ = NR.segment(chan, a.tile, k8, None, 256, a.connectivity, fill)
    assert hn == int(n[0]) and int(thr[0]) == -1 and np.array_equal(labels[0].cpu().numpy(), hl), "labels differ from the restatement"
    res["noise"] = dict(row(*timed(seg)), outputs_equal=True)
    seg.close()
    local = S.ThresholdSegmenter(0, "local", a.connectivity, fill, local_radius=NOISE_LOCAL_RADIUS)
    res["local"] = dict(row(*timed(local)), radius=NOISE_LOCAL_RADIUS)
    local.close()
    tophat = S.ThresholdSegmenter(0, "otsu", a.connectivity, fill, background_radius=TOPHAT_RADIUS)
    res["background"] = dict(row(*timed(tophat)), radius=TOPHAT_RADIUS)
    tophat.close()
    stage = lambda r, keys: sum(r["stage_ms_per_image"][k] for k in keys)
    noise_ms, local_ms = stage(res["noise"], ("noise_mesh_ms", "noise_cut_ms", "noise_link_ms")), stage(res["local"], ("local_median_ms", "local_ms"))
    res["noise_stage_ms_per_image"], res["local_stage_ms_per_image"] = round(noise_ms, 5), round(local_ms, 5)
    res["noise_over_local_stage_time"] = round(noise_ms / local_ms, 3)
    res["noise_over_local_wall_time"] = round(res["noise"]["wall_ms_per_image"][0] / res["local"]["wall_ms_per_image"][0], 3)
    line = json.dumps(res)
    out = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "segment_noise_bench.json")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


def clean_leg(a):
    import torch
    import clean_reference as CR
    import local_reference as LR
    import segment_reference as R
    from build import source_hash
    from cellscreen import extract as X
    from cellscreen import segment as S
    from test_local_cpu import dim_cell_scene

    fill = not a.no_fill_holes
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    tiles = a.side // 512
    if tiles < 1 or a.side % 512:
        raise SystemExit("--clean needs --side a multiple of 512: the scene is made of 512 x 512 fields")
    fields = [dim_cell_scene(seed)[0] for seed in range(tiles * tiles)]
    base = np.block([[fields[i * tiles + j] for j in range(tiles)] for i in range(tiles)])
    variants = [base, base[::-1], base[:, ::-1], base[::-1, ::-1]]          # four distinct images from one painting
    imgs = np.ascontiguousarray(np.stack([variants[b % 4] for b in range(a.images)]))
    ti = torch.from_numpy(imgs.view(np.int16)).to(dev)
    torch.cuda.synchronize()
    radius, delta = 25, a.delta or 60
    open_r, min_area = a.open, a.min_area
    if open_r is None and min_area is None:
        min_area = 50
    local = dict(threshold="local", connectivity=a.connectivity, fill_holes=fill, local_radius=radius, local_delta=delta)
    ext = X.CellExtractor(0)
    plain = S.ThresholdSegmenter(0, extractor=ext, **local)
    clean = S.ThresholdSegmenter(0, extractor=ext, open_radius=open_r, min_area=min_area, **local)

    def timed(fn, seg):
        walls, stages = [], []
        for k in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k >= a.warmup:
                walls.append(time.perf_counter() - t0)
                stages.append(seg.last_timing())
        return out, walls, stages

    # outputs first: one image's cleaned mask and labels against the host restatement
    one = ti[:1].contiguous()
    mask = clean.clean_mask_batch(one)
    labels, n, _ = clean.segment_batch(one)
    m = LR.local_mask(imgs[0], radius, delta) > 0
    want = CR.clean(R.ndimage.binary_fill_holes(m) if fill else m, open_r, 2, min_area, a.connectivity)
    hl, hn = R.label_mask(want, a.connectivity)
    assert np.array_equal(mask[0].cpu().numpy(), want), "cleaned mask differs from the restatement"
    assert hn == int(n[0]) and np.array_equal(labels[0].cpu().numpy(), hl), "labels differ from the restatement"

    spread = lambda stages, k: [round(med([t[k] for t in stages]), 4), round(min(t[k] for t in stages), 4),
                                round(max(t[k] for t in stages), 4)]
    wall3 = lambda walls: [round(med(walls) * 1e3, 3), round(min(walls) * 1e3, 3), round(max(walls) * 1e3, 3)]
    res = {"tool": "bench_segment --clean", "source_hash": source_hash(), "images": a.images, "side": a.side,
           "connectivity": a.connectivity, "fill_holes": fill, "local_radius": radius, "local_delta": delta, "open_radius": open_r,
           "open_connectivity": 2, "min_area": min_area, "cells_painted_per_image": 40 * tiles * tiles, "reps": a.reps,
           "warmup": a.warmup, "outputs_equal": True}
    legs = {}
    for name, seg in (("uncleaned", plain), ("cleaned", clean)):
        (_, n_lab, _), walls, stages = timed(lambda: seg.segment_batch(ti), seg)
        r, chain, _ = timed(lambda: ext.extract_batch(ti, seg.segment_batch(ti)[0]), seg)
        legs[name] = dict(walls=walls, chain=chain, cells=r.cells.cpu().numpy(), stats=X.region_stats(r.regions))
        res[name] = {"labels_per_image": round(float(n_lab.mean()), 1), "regions_measured": len(r.regions),
                     "cells_extracted": int(r.cells.shape[0]), "segment_images_per_s": round(a.images / med(walls), 2),
                     "segment_wall_ms": wall3(walls), "segment_extract_images_per_s": round(a.images / med(chain), 2),
                     "segment_extract_wall_ms": wall3(chain),
                     **{k: spread(stages, k) for k in sorted(stages[0])}}
    st = res["cleaned"]
    res["open_ms_per_image"] = round(st["open_ms"][0] / a.images, 5)
    res["min_area_ms_per_image"] = round(st["min_area_ms"][0] / a.images, 5)
    res["cleaned_over_uncleaned_segment_time"] = round(med(legs["cleaned"]["walls"]) / med(legs["uncleaned"]["walls"]), 3)
    res["cleaned_over_uncleaned_segment_extract_time"] = round(med(legs["cleaned"]["chain"]) / med(legs["uncleaned"]["chain"]), 3)
    res["cleaned_over_uncleaned_segment_extract_images_per_s"] = round(
        res["cleaned"]["segment_extract_images_per_s"] / res["uncleaned"]["segment_extract_images_per_s"], 3)
    if open_r is None and min_area <= X.REFERENCE_QC["min_area"]:
        assert legs["cleaned"]["stats"] == legs["uncleaned"]["stats"] and np.array_equal(legs["cleaned"]["cells"], legs["uncleaned"]["cells"]), \
            "the extraction changed under a min_area within its own area bound"
        res["extraction_equal"] = True
    plain_ms = med(legs["uncleaned"]["walls"]) * 1e3 / a.images
    res["open_radius_sweep"] = []
    for k in (1, 2):
        for r_ in (1, 3, 7, 15):
            seg = S.ThresholdSegmenter(0, extractor=ext, open_radius=r_, open_connectivity=k, **local)
            _, _, stages = timed(lambda: seg.clean_mask_batch(ti), seg)
            per = med([t["open_ms"] for t in stages]) / a.images
            res["open_radius_sweep"].append({"open_connectivity": k, "open_radius": r_, "open_ms_per_image": round(per, 5),
                                             "open_ns_per_pixel": round(per * 1e6 / (a.side * a.side), 4),
                                             "over_uncleaned_segment_time": round(per / plain_ms, 4)})
    ext.close()
    line = json.dumps(res)
    out = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "segment_clean_bench.json")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


def hysteresis_leg(a):
    import torch
    import hysteresis_reference as HR
    import segment_reference as R
    from build import source_hash
    from cellscreen import extract as X
    from cellscreen import segment as S
    from test_local_cpu import dim_cell_scene

    fill = not a.no_fill_holes
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    tiles = a.side // 512
    if tiles < 1 or a.side % 512:
        raise SystemExit("--hysteresis needs --side a multiple of 512: the scene is made of 512 x 512 fields")
    fields = [dim_cell_scene(seed)[0] for seed in range(tiles * tiles)]
    base = np.block([[fields[i * tiles + j] for j in range(tiles)] for i in range(tiles)])
    variants = [base, base[::-1], base[:, ::-1], base[::-1, ::-1]]          # four distinct images from one painting
    imgs = np.ascontiguousarray(np.stack([variants[b % 4] for b in range(a.images)]))
    ti = torch.from_numpy(imgs.view(np.int16)).to(dev)
    torch.cuda.synchronize()
    radius, weak, strong, min_area = 25, a.weak_delta, a.strong_delta, 50
    common = dict(threshold="local", connectivity=a.connectivity, fill_holes=fill, local_radius=radius)
    ext = X.CellExtractor(0)
    configs = (("weak_alone", S.ThresholdSegmenter(0, extractor=ext, local_delta=weak, **common)),
               ("weak_min_area", S.ThresholdSegmenter(0, extractor=ext, local_delta=weak, min_area=min_area, **common)),
               ("hysteresis", S.ThresholdSegmenter(0, extractor=ext, local_delta=strong, weak_delta=weak, **common)))

    def timed(fn, seg):
        walls, stages = [], []
        for k in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k >= a.warmup:
                walls.append(time.perf_counter() - t0)
                stages.append(seg.last_timing())
        return out, walls, stages

    # outputs first: one image's plane and labels against the host restatement
    hyst = configs[2][1]
    one = ti[:1].contiguous()
    plane = hyst.hysteresis_mask_batch(one)
    labels, n, _ = hyst.segment_batch(one)
    want = HR.hysteresis(HR.levels_local(imgs[0], radius, strong, weak), a.connectivity)
    hl, hn = R.label_mask(R.ndimage.binary_fill_holes(want > 0) if fill else want > 0, a.connectivity)
    assert np.array_equal(plane[0].cpu().numpy(), want), "plane differs from the restatement"
    assert hn == int(n[0]) and np.array_equal(labels[0].cpu().numpy(), hl), "labels differ from the restatement"

    spread = lambda stages, k: [round(med([t[k] for t in stages]), 4), round(min(t[k] for t in stages), 4),
                                round(max(t[k] for t in stages), 4)]
    wall3 = lambda walls: [round(med(walls) * 1e3, 3), round(min(walls) * 1e3, 3), round(max(walls) * 1e3, 3)]
    res = {"tool": "bench_segment --hysteresis", "source_hash": source_hash(), "images": a.images, "side": a.side,
           "connectivity": a.connectivity, "fill_holes": fill, "local_radius": radius, "weak_delta": weak, "strong_delta": strong,
           "min_area": min_area, "cells_painted_per_image": 40 * tiles * tiles, "reps": a.reps, "warmup": a.warmup,
           "outputs_equal": True}
    walls_of, chain_of = {}, {}
    for name, seg in configs:
        (_, n_lab, _), walls, stages = timed(lambda: seg.segment_batch(ti), seg)
        r, chain, _ = timed(lambda: ext.extract_batch(ti, seg.segment_batch(ti)[0]), seg)
        walls_of[name], chain_of[name] = med(walls), med(chain)
        res[name] = {"labels_per_image": round(float(n_lab.mean()), 1), "regions_measured": len(r.regions),
                     "cells_extracted": int(r.cells.shape[0]), "segment_images_per_s": round(a.images / med(walls), 2),
                     "segment_wall_ms": wall3(walls), "segment_extract_images_per_s": round(a.images / med(chain), 2),
                     "segment_extract_wall_ms": wall3(chain),
                     **{k: spread(stages, k) for k in sorted(stages[0])}}
    st = res["hysteresis"]
    res["hysteresis_level_ms_per_image"] = round(st["hysteresis_level_ms"][0] / a.images, 5)
    res["hysteresis_link_ms_per_image"] = round(st["hysteresis_link_ms"][0] / a.images, 5)
    res["min_area_ms_per_image"] = round(res["weak_min_area"]["min_area_ms"][0] / a.images, 5)
    for other in ("weak_alone", "weak_min_area"):
        res[f"hysteresis_over_{other}_segment_time"] = round(walls_of["hysteresis"] / walls_of[other], 3)
        res[f"hysteresis_over_{other}_segment_extract_time"] = round(chain_of["hysteresis"] / chain_of[other], 3)
    ext.close()
    line = json.dumps(res)
    out = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "segment_hysteresis_bench.json")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


def smooth_leg(a):
    import torch
    import segment_reference as R
    import smooth_reference as SM
    from build import source_hash
    from cellscreen import extract as X
    from cellscreen import segment as S
    from test_smooth_cpu import faint_cell_scene

    fill = not a.no_fill_holes
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    tiles = a.side // 512
    if tiles < 1 or a.side % 512:
        raise SystemExit("--smooth needs --side a multiple of 512: the scene is made of 512 x 512 fields")
    fields = [faint_cell_scene(seed)[0] for seed in range(tiles * tiles)]
    base = np.block([[fields[i * tiles + j] for j in range(tiles)] for i in range(tiles)])
    variants = [base, base[::-1], base[:, ::-1], base[::-1, ::-1]]          # four distinct images from one painting
    imgs = np.ascontiguousarray(np.stack([variants[b % 4] for b in range(a.images)]))
    ti = torch.from_numpy(imgs.view(np.int16)).to(dev)
    torch.cuda.synchronize()
    common = dict(threshold="otsu", connectivity=a.connectivity, fill_holes=fill)
    ext = X.CellExtractor(0)
    plain = S.ThresholdSegmenter(0, extractor=ext, **common)
    smooth = S.ThresholdSegmenter(0, extractor=ext, smooth_sigma=a.smooth, denoise=a.denoise, **common)

    def timed(fn, seg):
        walls, stages = [], []
        for k in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k >= a.warmup:
                walls.append(time.perf_counter() - t0)
                stages.append(seg.last_timing())
        return out, walls, stages

    # outputs first: one image's smoothed plane and labels against the host restatement
    one = ti[:1].contiguous()
    plane = smooth.smooth_batch(one)
    labels, n, thr = smooth.segment_batch(one)
    want = SM.smooth_sigma(imgs[0], a.smooth, median=a.denoise)
    assert np.array_equal(plane[0].cpu().numpy().view(np.uint16), want), "smoothed plane differs from the restatement"
    hl, hn, ht = R.segment(want, "otsu", a.connectivity, fill)
    assert hn == int(n[0]) and ht == int(thr[0]) and np.array_equal(labels[0].cpu().numpy(), hl), "labels differ from the restatement"

    spread = lambda stages, k: [round(med([t[k] for t in stages]), 4), round(min(t[k] for t in stages), 4),
                                round(max(t[k] for t in stages), 4)]
    wall3 = lambda walls: [round(med(walls) * 1e3, 3), round(min(walls) * 1e3, 3), round(max(walls) * 1e3, 3)]
    res = {"tool": "bench_segment --smooth", "source_hash": source_hash(), "images": a.images, "side": a.side,
           "connectivity": a.connectivity, "fill_holes": fill, "smooth_sigma": a.smooth, "smooth_radius": len(S.smooth_weights(a.smooth)) - 1,
           "denoise": bool(a.denoise), "cells_painted_per_image": 40 * tiles * tiles, "reps": a.reps, "warmup": a.warmup,
           "outputs_equal": True}
    legs = {}
    for name, seg in (("unsmoothed", plain), ("smoothed", smooth)):
        (_, n_lab, _), walls, stages = timed(lambda: seg.segment_batch(ti), seg)
        r, chain, _ = timed(lambda: ext.extract_batch(ti, seg.segment_batch(ti)[0]), seg)
        legs[name] = dict(walls=walls, chain=chain)
        res[name] = {"labels_per_image": round(float(n_lab.mean()), 1), "regions_measured": len(r.regions),
                     "cells_extracted": int(r.cells.shape[0]), "segment_images_per_s": round(a.images / med(walls), 2),
                     "segment_wall_ms": wall3(walls), "segment_extract_images_per_s": round(a.images / med(chain), 2),
                     "segment_extract_wall_ms": wall3(chain),
                     **{k: spread(stages, k) for k in sorted(stages[0])}}
    px = a.side * a.side
    res["smooth_ms_per_image"] = round(res["smoothed"]["smooth_ms"][0] / a.images, 5)
    res["smooth_ns_per_pixel"] = round(res["smoothed"]["smooth_ms"][0] * 1e6 / (a.images * px), 4)
    res["smoothed_over_unsmoothed_segment_time"] = round(med(legs["smoothed"]["walls"]) / med(legs["unsmoothed"]["walls"]), 3)
    res["smoothed_over_unsmoothed_segment_extract_time"] = round(med(legs["smoothed"]["chain"]) / med(legs["unsmoothed"]["chain"]), 3)
    plain_ms = med(legs["unsmoothed"]["walls"]) * 1e3 / a.images
    res["sigma_sweep"] = []
    for sigma in (0.25, 1, 2, 4, 8, 15.875):
        seg = S.ThresholdSegmenter(0, extractor=ext, smooth_sigma=sigma, **common)
        _, _, stages = timed(lambda: seg.smooth_batch(ti), seg)
        per = med([t["smooth_ms"] for t in stages]) / a.images
        res["sigma_sweep"].append({"smooth_sigma": sigma, "radius": len(S.smooth_weights(sigma)) - 1, "smooth_ms_per_image": round(per, 5),
                                   "smooth_ns_per_pixel": round(per * 1e6 / px, 4),
                                   "effective_gb_per_s": round(12.0 * px / (per * 1e-3) / 1e9, 1),       # 2 + 4 + 4 + 2 bytes per pixel
                                   "over_unsmoothed_segment_time": round(per / plain_ms, 4)})
    ext.close()
    line = json.dumps(res)
    out = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "segment_smooth_bench.json")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


DEFAULT_OUT = os.path.join(ROOT, "profiles", "segment_bench.json")
TOPHAT_RADIUS = 51                                      # the top-hat that --local is set beside: --background 51's figure


def score_leg(a):
    import torch
    import match_reference as MR
    from build import source_hash
    from cellscreen import score as SC
    from cellscreen import segment as S
    from cellscreen import synth

    fill = not a.no_fill_holes
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    imgs, labs = synth.label_images(2024, a.images, hw=(a.side, a.side), n_cells=a.cells)
    ti = torch.from_numpy(imgs.view(np.int16)).to(dev)
    tl = torch.from_numpy(labs).to(dev)
    max_truth = int(labs.max())
    torch.cuda.synchronize()
    seg = S.ThresholdSegmenter(0, "otsu", a.connectivity, fill)
    matcher = SC.LabelMatcher(0, extractor=seg)

    def timed(fn, timing=None):
        walls, stages = [], []
        for k in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k >= a.warmup:
                walls.append(time.perf_counter() - t0)
                stages.append(timing() if timing else {})
        return out, walls, stages

    wall3 = lambda walls: [round(f(walls) * 1e3 / a.images, 4) for f in (med, min, max)]
    per_image = lambda stages: {k: round(med([t[k] for t in stages]) / a.images, 5) for k in stages[0]}
    (labels, n_labels, _), seg_walls, seg_stages = timed(lambda: seg.segment_batch(ti), seg.last_timing)
    max_pred = max(1, int(n_labels.max()))
    # outputs first: one image's tables against the host restatement
    one = matcher.match_batch(labels[:1].contiguous(), tl[:1].contiguous(), max_pred=max_pred, max_truth=max_truth)
    hp, ht, hn = MR.tables(labels[0].cpu().numpy(), labs[0], max_pred, max_truth)
    assert np.array_equal(one.pred, hp) and np.array_equal(one.truth, ht) and np.array_equal(one.n_pairs, hn), "tables differ from the restatement"
    m, match_walls, match_stages = timed(lambda: matcher.match_batch(labels, tl, max_pred=max_pred, max_truth=max_truth), matcher.last_timing)
    log2, grows = matcher.last_table()
    (stats, _, _), score_walls, _ = timed(lambda: seg.score_batch(ti, tl, max_truth=max_truth))
    nh = max(1, min(a.host_images, a.images))
    host_labels = labels[:nh].cpu().numpy()
    host_walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        MR.tables(host_labels, labs[:nh], max_pred, max_truth)
        host_walls.append(time.perf_counter() - t0)
    seg.close()
    tot = stats["total"]
    res = {"tool": "bench_segment --score", "source_hash": source_hash(), "images": a.images, "side": a.side, "cells": a.cells,
           "connectivity": a.connectivity, "fill_holes": fill, "reps": a.reps, "warmup": a.warmup, "outputs_equal": True,
           "max_pred": max_pred, "max_truth": max_truth, "pairs": int(m.n_pairs.sum()), "table_log2": log2, "grows": grows,
           "segment": {"images_per_s": round(a.images / med(seg_walls), 2), "wall_ms_per_image": wall3(seg_walls),
                       "stage_ms_per_image": per_image(seg_stages)},
           "match": {"images_per_s": round(a.images / med(match_walls), 2), "wall_ms_per_image": wall3(match_walls),
                     "stage_ms_per_image": per_image(match_stages)},
           "score_batch": {"images_per_s": round(a.images / med(score_walls), 2), "wall_ms_per_image": wall3(score_walls)},
           "host_images": nh, "host_restatement_ms_per_image": round(med(host_walls) * 1e3 / nh, 2),
           "host_note": "tests/match_reference.py: numpy.unique on the pair codes per image, one process, labels already on the host",
           "n_pred": tot["n_pred"], "n_true": tot["n_true"], "merged": tot["merged"], "split": tot["split"],
           "by_threshold": [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()} for r in tot["by_threshold"]]}
    res["match_over_segment_wall_time"] = round(med(match_walls) / med(seg_walls), 3)
    res["host_over_device_match_time"] = round(med(host_walls) / nh / (med(match_walls) / a.images), 1)
    line = json.dumps(res)
    out = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "segment_score_bench.json")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-images", type=int, default=4)
    ap.add_argument("--connectivity", type=int, default=1)
    ap.add_argument("--no-fill-holes", action="store_true")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--split", action="store_true", help="measure the split_touching option (profiles/segment_split_bench.json)")
    ap.add_argument("--split-cells", type=int, default=3000)
    ap.add_argument("--split-h", type=int, default=3)
    ap.add_argument("--split-intensity", action="store_true",
                    help="measure split_by='intensity' beside the distance split (profiles/segment_split_intensity_bench.json)")
    ap.add_argument("--split-depth", type=int, default=16)
    ap.add_argument("--split-contrast", type=int, default=0)
    ap.add_argument("--background", type=int, default=None, metavar="R",
                    help="measure the background correction of radius R (profiles/segment_background_bench.json)")
    ap.add_argument("--denoise", action="store_true", help="with --background, --local or --smooth: the 3 x 3 median first")
    ap.add_argument("--local", type=int, default=None, metavar="R",
                    help="measure the local mean threshold of radius R (profiles/segment_local_bench.json)")
    ap.add_argument("--delta", type=int, default=0, metavar="D", help="with --local or --clean: counts above the local mean")
    ap.add_argument("--clean", action="store_true", help="measure the mask cleanup on a speckled scene (profiles/segment_clean_bench.json)")
    ap.add_argument("--open", type=int, default=None, metavar="R", help="with --clean: open_radius")
    ap.add_argument("--min-area", type=int, default=None, metavar="A", help="with --clean: min_area (50 when --open is not given either)")
    ap.add_argument("--smooth", type=float, default=None, metavar="SIGMA",
                    help="measure the Gaussian smoothing on a field of faint cells in noise (profiles/segment_smooth_bench.json)")
    ap.add_argument("--hysteresis", action="store_true",
                    help="measure the hysteresis threshold on --clean's speckled scene (profiles/segment_hysteresis_bench.json)")
    ap.add_argument("--weak-delta", type=int, default=40, metavar="W", help="with --hysteresis: the weak delta")
    ap.add_argument("--strong-delta", type=int, default=200, metavar="D", help="with --hysteresis: the strong delta")
    ap.add_argument("--noise", action="store_true",
                    help="measure the noise-adaptive threshold beside the local rule and the top-hat (profiles/segment_noise_bench.json)")
    ap.add_argument("--noise-k", type=float, default=5.0, metavar="K", help="with --noise: sigmas above the local background")
    ap.add_argument("--tile", type=int, default=64, metavar="T", help="with --noise: the mesh tile's side")
    ap.add_argument("--score", action="store_true", help="measure the label scoring beside the segmentation (profiles/segment_score_bench.json)")
    a = ap.parse_args()
    if a.score:
        if (a.noise or a.split or a.split_intensity or a.background is not None or a.local is not None or a.clean or a.delta or a.hysteresis
                or a.smooth is not None or a.denoise or a.open is not None or a.min_area is not None):
            ap.error("--score is measured on its own")
        return score_leg(a)
    if a.noise:
        if (a.split or a.split_intensity or a.background is not None or a.local is not None or a.clean or a.delta or a.hysteresis
                or a.smooth is not None or a.denoise or a.open is not None or a.min_area is not None):
            ap.error("--noise is measured on its own")
        return noise_leg(a)
    if a.noise_k != 5.0 or a.tile != 64:
        ap.error("--noise-k and --tile need --noise")
    if a.hysteresis:
        if (a.split or a.split_intensity or a.background is not None or a.local is not None or a.clean or a.delta
                or a.smooth is not None or a.denoise or a.open is not None or a.min_area is not None):
            ap.error("--hysteresis is measured on its own")
        return hysteresis_leg(a)
    if a.split_intensity:
        if a.split or a.background is not None or a.local is not None or a.clean or a.delta or a.smooth is not None or a.denoise:
            ap.error("--split-intensity is measured on its own")
        return split_intensity_leg(a)
    if a.smooth is not None:
        if a.split or a.background is not None or a.local is not None or a.clean or a.delta:
            ap.error("--smooth is measured on its own")
        return smooth_leg(a)
    if (a.open is not None or a.min_area is not None) and not a.clean:
        ap.error("--open and --min-area need --clean")
    if a.clean:
        if a.split or a.background is not None or a.local is not None or a.denoise:
            ap.error("--clean is measured on its own")
        return clean_leg(a)
    if a.denoise and a.background is None and a.local is None:
        ap.error("--denoise needs --background R or --local R")
    if a.delta and a.local is None:
        ap.error("--delta needs --local R or --clean")
    if a.local is not None and (a.split or a.background is not None):
        ap.error("--local is measured on its own")
    if a.split:
        return split_leg(a)
    if a.background is not None:
        return background_leg(a)
    if a.local is not None:
        return local_leg(a)

    import torch
    import segment_reference as R
    from cellscreen import extract as X
    from cellscreen import segment as S
    from cellscreen import synth

    fill = not a.no_fill_holes
    imgs, _ = synth.label_images(2024, a.images, hw=(a.side, a.side), n_cells=a.cells)
    dev = torch.device("cuda", 0)
    ti = torch.from_numpy(imgs.view(np.int16)).to(dev)
    torch.cuda.synchronize()
    ext = X.CellExtractor(0)
    seg = S.ThresholdSegmenter(0, "otsu", a.connectivity, fill, extractor=ext)

    def timed(fn, reps):
        walls, extra = [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
            extra.append(seg.last_timing())
        return out, walls, extra

    def device_chain():
        labels, _, _ = seg.segment_batch(ti)
        return ext.extract_batch(ti, labels)

    for _ in range(a.warmup):
        seg.segment_batch(ti)
        device_chain()
    (labels, n_labels, thr), seg_walls, seg_times = timed(lambda: seg.segment_batch(ti), a.reps)
    r, chain_walls, _ = timed(device_chain, a.reps)

    # the host path on the first --host-images images: outputs first, then time
    nh = max(1, min(a.host_images, a.images))
    th = ti[:nh].contiguous()
    kw = dict(threshold="otsu", connectivity=a.connectivity, fill_holes=fill)

    def host_segment():
        return np.stack([R.segment(imgs[b, ..., 2], **kw)[0] for b in range(nh)])

    def host_chain():
        hl = host_segment()
        return ext.extract_batch(th, torch.from_numpy(hl).to(dev))

    hl = host_segment()
    assert np.array_equal(labels[:nh].cpu().numpy(), hl), "device labels differ from the host restatement"
    rh = host_chain()
    rd = ext.extract_batch(th, labels[:nh].contiguous())
    assert np.array_equal(rh.regions, rd.regions) and torch.equal(rh.cells, rd.cells), "extraction differs between the two paths"
    host_seg_walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        host_segment()
        host_seg_walls.append(time.perf_counter() - t0)
    _, host_walls, _ = timed(host_chain, 2)

    med = lambda v: float(np.median(v))
    spread = lambda k: [round(med([t[k] for t in seg_times]), 4), round(min(t[k] for t in seg_times), 4),
                        round(max(t[k] for t in seg_times), 4)]
    from build import source_hash
    res = {
        "tool": "bench_segment", "source_hash": source_hash(), "images": a.images, "side": a.side,
        "connectivity": a.connectivity, "fill_holes": fill,
        "components": int(n_labels.sum()), "regions": len(r.regions), "cells": int(r.cells.shape[0]),
        "segment_images_per_s": round(a.images / med(seg_walls), 2),
        "segment_wall_ms": [round(med(seg_walls) * 1e3, 3), round(min(seg_walls) * 1e3, 3), round(max(seg_walls) * 1e3, 3)],
        "threshold_ms": spread("threshold_ms"), "label_ms": spread("label_ms"),
        "threshold_images_per_s": round(a.images / (med([t["threshold_ms"] for t in seg_times]) * 1e-3), 1),
        "label_images_per_s": round(a.images / (med([t["label_ms"] for t in seg_times]) * 1e-3), 1),
        "segment_extract_images_per_s": round(a.images / med(chain_walls), 2),
        "segment_extract_wall_ms": [round(med(chain_walls) * 1e3, 3), round(min(chain_walls) * 1e3, 3), round(max(chain_walls) * 1e3, 3)],
        "host_images": nh,
        "host_segment_images_per_s": round(nh / med(host_seg_walls), 3),
        "host_path_images_per_s": round(nh / med(host_walls), 3),
        "host_path_note": "Otsu restatement + scipy.ndimage (one process) on the host, labels uploaded, CellExtractor on the device",
        "outputs_equal": True, "reps": a.reps, "warmup": a.warmup,
    }
    res["speedup_over_host_path"] = round(res["segment_extract_images_per_s"] / res["host_path_images_per_s"], 1)
    ext.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
