#!/usr/bin/env python3
"""Time the distance module at the workload's shape against the host round trip it replaces ("Distance transform,
surface metrics, root traits"; the result is kept as profiles/distance_edt.json).

Two 608 x 968 masks in one batch: a sparse noise map and a map of drawn roots (seeded random walks 3 to 9 pixels thick); the truth
of the surface distances is the same batch moved by (2, 3) pixels.  ``distance_transform``, ``surface_distances`` and ``skeletonize``
are each warmed up and then bracketed by events on the stream; beside them, on the same box and the same maps, ``.cpu()`` +
``scipy.ndimage.distance_transform_edt``, the MedPy recipe of the surface distances written out with scipy, and ``thin_reference``.
Needs a real MI355X: without a device it fails, it does not fall back.

    python tools/measure_distance.py --out profiles/distance_edt.json [--repeats 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H_, W_ = 608, 968


def drawn_roots(h, w, seed=5, walks=14):
    rng = np.random.RandomState(seed)
    a = np.zeros((h, w), dtype=bool)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(walks):
        y, x, ang = 0.0, rng.uniform(0.1, 0.9) * w, np.pi / 2 + rng.uniform(-0.5, 0.5)
        r = rng.uniform(1.5, 4.5)
        while 0 <= y < h and 0 <= x < w:
            y0, y1, x0, x1 = int(max(0, y - 6)), int(min(h, y + 7)), int(max(0, x - 6)), int(min(w, x + 7))
            a[y0:y1, x0:x1] |= (yy[y0:y1, x0:x1] - y) ** 2 + (xx[y0:y1, x0:x1] - x) ** 2 <= r * r
            ang += rng.uniform(-0.25, 0.25)
            y, x = y + 1.5 * np.sin(ang), x + 1.5 * np.cos(ang)
    return a


def device_ms(fn, repeats):
    import torch
    fn()                                        # warm-up: code objects, allocator
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(repeats):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / repeats


def host_ms(fn, repeats):
    fn()
    t = time.perf_counter()
    for _ in range(repeats):
        fn()
    return (time.perf_counter() - t) * 1e3 / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    import torch
    from scipy import ndimage
    import hyperpri_amd as H
    if not torch.cuda.is_available():
        raise SystemExit("measure_distance: no ROCm device")
    dev = "cuda:0"
    maps = np.stack([np.random.RandomState(1).rand(H_, W_) < 0.02, drawn_roots(H_, W_)])
    truth = np.roll(maps, (2, 3), axis=(1, 2))
    pred_d = torch.from_numpy(maps.astype(np.uint8)).to(dev)
    truth_d = torch.from_numpy(truth.astype(np.uint8)).to(dev)
    cross = ndimage.generate_binary_structure(2, 1)

    def host_edt():
        a = pred_d.cpu().numpy().astype(bool)
        return [ndimage.distance_transform_edt(a[n]) for n in range(2)]

    def host_surface():
        a, b = pred_d.cpu().numpy().astype(bool), truth_d.cpu().numpy().astype(bool)
        out = []
        for n in range(2):
            sa = a[n] & ~ndimage.binary_erosion(a[n], cross, border_value=0)
            sb = b[n] & ~ndimage.binary_erosion(b[n], cross, border_value=0)
            ab, ba = ndimage.distance_transform_edt(~sb)[sa], ndimage.distance_transform_edt(~sa)[sb]
            both = np.concatenate([ab, ba])
            out.append((both.max(), np.percentile(both, 95), 0.5 * (ab.mean() + ba.mean())))
        return out

    def host_thin():
        return H.thin_reference(pred_d.cpu().numpy())

    skel, pairs = H.skeletonize(pred_d, return_pairs=True)
    _, pairs_roots = H.skeletonize(pred_d[1], return_pairs=True)
    m = H.surface_metrics_from_hist(H.surface_distances(pred_d, None, truth_d)["hist"])
    res = {
        "shape": [2, H_, W_], "maps": ["noise 0.02", "drawn roots"], "repeats": args.repeats,
        "foreground_pixels": [int(v) for v in maps.sum(axis=(1, 2))],
        "device_ms": {
            "distance_transform": device_ms(lambda: H.distance_transform(pred_d), args.repeats),
            "surface_distances": device_ms(lambda: H.surface_distances(pred_d, None, truth_d), args.repeats),
            "skeletonize": device_ms(lambda: H.skeletonize(pred_d), args.repeats),
        },
        "host_ms": {
            "cpu_scipy_distance_transform_edt": host_ms(host_edt, max(1, args.repeats // 3)),
            "cpu_scipy_surface_recipe": host_ms(host_surface, max(1, args.repeats // 3)),
            "cpu_thin_reference": host_ms(host_thin, 1),
        },
        "thinning_pairs": {"batch": pairs, "drawn_roots": pairs_roots},
        "skeleton_pixels": [int(v) for v in skel.sum(dim=(1, 2)).tolist()],
        "surface": {k: [float(v) for v in m[k]] for k in ("hd", "hd95", "assd")},
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
