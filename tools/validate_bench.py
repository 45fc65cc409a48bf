"""Validation as the reference Trainer runs it after every epoch (trainer.py:349-445), timed on
synthetic cases: the per-threshold path (sliding window -> numpy -> mask -> calculate_metrics once
per threshold; what l3u_plugin.install() gives without fast_validate) against the device-resident
path (sliding window with output="device" and a forward cache -> lesion.sweep_metrics).

    python tools/validate_bench.py [--cases 3] [--shape 128 128 256] [--epochs 3]

The two stages are timed separately, each path on the same inputs:
  * inference: a seed-42 Lightweight3DUNet over synthetic volumes, patch 48, overlap 0.5;
  * metrics: 7 thresholds over blob-shaped probability maps (Gaussian blobs of mixed height, so
    components merge and split across the thresholds), body masks on.  The old path gets the maps
    as numpy arrays (its sliding window returns numpy), the new path as device tensors (its
    sliding window leaves them there).
`copies` isolates what the old path moves over PCIe per epoch: one map download and one upload
per threshold per case, timed on their own.  Prints one JSON line.  Not part of bench.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-3d-unet-front_amd"))

THRESHOLDS = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7]


def blob_case(shape, seed, nblob):
    rng = np.random.default_rng(seed)
    ax = [np.arange(s, dtype=np.float32) for s in shape]
    prob = np.zeros(shape, np.float32)
    label = np.zeros(shape, np.float32)
    for b in range(nblob):
        c = [rng.uniform(6, s - 6) for s in shape]
        sig, amp = rng.uniform(2.0, 6.0), rng.uniform(0.25, 0.95)
        g = [np.exp(-((a - ci) ** 2) / (2 * sig ** 2)).astype(np.float32) for a, ci in zip(ax, c)]
        np.maximum(prob, amp * np.einsum("i,j,k->ijk", *g), out=prob)
        if b % 2 == 0:
            r = sig * rng.uniform(0.5, 0.9)
            d = [(a - ci) ** 2 for a, ci in zip(ax, c)]
            label[(d[0][:, None, None] + d[1][None, :, None] + d[2][None, None, :]) <= r * r] = 1.0
    prob = np.clip(prob + 0.04 * rng.random(shape, dtype=np.float32), 0, 0.999).astype(np.float32)
    mask = np.ones(shape, np.float32)
    mask[:, :8], mask[:, -8:] = 0.0, 0.0
    image = rng.random(shape, dtype=np.float32)
    return image, prob, label, mask


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 256])
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--patch", type=int, default=48)
    ap.add_argument("--blobs", type=int, default=40)
    a = ap.parse_args()

    from light_unet import lesion
    from light_unet.models.unet3d import Lightweight3DUNet
    from light_unet.utils import sliding_window_inference_3d as sw

    dev = torch.device("cuda", 0)
    torch.manual_seed(42)
    model = Lightweight3DUNet(dropout_p=0.0).to(dev)
    shape, patch = tuple(a.shape), (a.patch,) * 3
    cases = [blob_case(shape, 100 + i, a.blobs) for i in range(a.cases)]
    images, probs, labels, masks = (list(x) for x in zip(*cases))
    spacing = [(4.0, 4.0, 4.0)] * a.cases

    def old_inference():
        return [sw(img, model, patch, 0.5, dev, True) for img in images]

    def old_metrics():
        maps = [p * m for p, m in zip(probs, masks)]
        return [lesion.calculate_metrics(maps, labels, threshold=t, spacing=spacing)
                for t in THRESHOLDS]

    fwd_cache, tgt_cache = {}, {}

    def new_inference():
        return [sw(img, model, patch, 0.5, dev, True, output="device", forward_cache=fwd_cache)
                for img in images]

    probs_d = [torch.from_numpy(p).to(dev) for p in probs]
    masks_d = [torch.from_numpy(m).to(dev) for m in masks]

    def new_metrics():
        return lesion.sweep_metrics(probs_d, labels, THRESHOLDS, spacing=spacing, body_masks=masks_d,
                                    target_cache=tgt_cache)

    def copies():
        for p in probs_d:
            host = p.cpu().numpy()
            for _ in THRESHOLDS:
                torch.from_numpy(host).to(dev)

    rows = {k: [] for k in ("old_inference", "old_metrics", "new_inference", "new_metrics", "copies")}
    ref = got = None
    for _ in range(a.epochs):
        t, maps_old = timed(old_inference)
        rows["old_inference"].append(t)
        t, ref = timed(old_metrics)
        rows["old_metrics"].append(t)
        t, maps_new = timed(new_inference)
        rows["new_inference"].append(t)
        t, got = timed(new_metrics)
        rows["new_metrics"].append(t)
        t, _ = timed(copies)
        rows["copies"].append(t)
        for x, y in zip(maps_old, maps_new):
            assert np.array_equal(x, y.cpu().numpy()), "device / cached sliding window differs"
    assert got == ref, "sweep_metrics differs from the per-threshold path"

    def ms(v):
        return round(1e3 * v, 2)
    warm = {k: ms(min(v[1:]) if len(v) > 1 else v[0]) for k, v in rows.items()}
    out = {"tool": "validate_bench", "device": torch.cuda.get_device_name(0), "cases": a.cases,
           "shape": list(shape), "patch": a.patch, "thresholds": len(THRESHOLDS),
           "first_epoch_ms": {k: ms(v[0]) for k, v in rows.items()},
           "warm_epoch_ms": warm,
           "old_total_ms": round(warm["old_inference"] + warm["old_metrics"], 2),
           "new_total_ms": round(warm["new_inference"] + warm["new_metrics"], 2),
           "components_per_threshold": [m["tp"] + m["fp"] for m in ref]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
