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
per threshold per case, timed on their own.

A third leg times the sliding window with a body mask (`body_mask=`: windows without a mask voxel
are not run) next to the same call without one, alternating, `--repeats` times in the same
process: an ellipsoid body (the semi-axes of the 256^3 benchmark volume: 0.45 / 0.35 / 0.3 of the
axes) and a mask of ones, which keeps every window and so prices the occupancy pass and its
read-back.  The masked maps must equal the unmasked ones times the mask.  `masked_inference` in the
output holds windows / kept, the times, the spread of the unmasked repeats and whether the
full-mask leg stays within it.  Prints one JSON line.  Not part of bench.py.
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


def ellipsoid_mask(shape):
    """A central ellipsoid with semi-axes 0.45 / 0.35 / 0.3 of the axes, as float32 0 / 1."""
    g = np.ogrid[tuple(slice(0, s) for s in shape)]
    r = sum(((a - s / 2) / (f * s)) ** 2 for a, s, f in zip(g, shape, (0.45, 0.35, 0.3)))
    return (r <= 1).astype(np.float32)


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
    ap.add_argument("--repeats", type=int, default=10, help="repeats of the masked-inference legs")
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

    # ---- masked inference next to the unmasked call (the path above), alternating
    images_d = [torch.from_numpy(img).to(dev) for img in images]
    body_d = torch.from_numpy(ellipsoid_mask(shape)).to(dev)
    ones_d = torch.ones(shape, device=dev)
    stats = {"body": {}, "full": {}}

    def infer(mask, st=None):
        return [sw(img, model, patch, 0.5, dev, True, output="device", forward_cache=fwd_cache,
                   body_mask=mask, stats=st) for img in images_d]

    legs = {"unmasked": lambda: infer(None), "body": lambda: infer(body_d, stats["body"]),
            "full": lambda: infer(ones_d, stats["full"])}
    plain = legs["unmasked"]()
    for name, mask in (("body", body_d), ("full", ones_d)):
        for x, y in zip(plain, legs[name]()):
            assert torch.equal(y, x * mask), f"masked map ({name}) differs from unmasked * mask"
    times = {k: [] for k in legs}
    for _ in range(a.repeats):
        for name, fn in legs.items():
            times[name].append(timed(fn)[0])
    # what a masked call adds, timed on its own per case: the occupancy pass (launch to completion),
    # the read-back of its flags, and the masked blend against the plain one (device events, random
    # predictions, every window kept)
    from light_unet import _native as nat
    from light_unet.utils import window_positions
    grid = [window_positions(s, a.patch, a.patch // 2) for s in shape]
    gt = [torch.tensor(g, dtype=torch.int32, device=dev) for g in grid]
    keep = torch.empty(len(grid[0]) * len(grid[1]) * len(grid[2]), dtype=torch.int32, device=dev)

    def occupancy(mask):
        nat.call("l3u_window_occupancy", mask.data_ptr(), 0, *shape, gt[0].data_ptr(), len(grid[0]),
                 gt[1].data_ptr(), len(grid[1]), gt[2].data_ptr(), len(grid[2]), *patch,
                 keep.data_ptr(), nat.stream())
    occ = {k: min(timed(lambda: occupancy(m))[0] for _ in range(a.repeats))
           for k, m in (("body", body_d), ("full", ones_d))}
    readback = min(timed(keep.cpu)[0] for _ in range(a.repeats))
    nwin, P = keep.numel(), a.patch ** 3
    preds, prob = torch.rand(nwin, P, device=dev), torch.empty(shape, device=dev)
    imp = torch.ones(P, device=dev)
    slot = torch.arange(nwin, dtype=torch.int32, device=dev)
    gargs = (gt[0].data_ptr(), len(grid[0]), gt[1].data_ptr(), len(grid[1]), gt[2].data_ptr(),
             len(grid[2]), imp.data_ptr())

    def blend_us(masked_blend):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(a.repeats + 1):      # the first call warms up
            if i == 1:
                ev[0].record()
            if masked_blend:
                nat.call("l3u_window_blend_masked", preds.data_ptr(), slot.data_ptr(), *gargs,
                         ones_d.data_ptr(), 0, *shape, *patch, prob.data_ptr(), nat.stream())
            else:
                nat.call("l3u_window_blend", preds.data_ptr(), *gargs, *shape, *patch,
                         prob.data_ptr(), nat.stream())
        ev[1].record()
        torch.cuda.synchronize()
        return round(1e3 * ev[0].elapsed_time(ev[1]) / a.repeats, 1)
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = max(times["unmasked"]) - min(times["unmasked"])
    over = med["full"] - med["unmasked"]
    masked = {"mask": "ellipsoid 0.45/0.35/0.3", "repeats": a.repeats,
              "windows": a.cases * stats["body"]["windows"], "kept": a.cases * stats["body"]["kept"],
              "voxels_inside": round(float(body_d.mean()), 3),
              "unmasked_ms": {"median": ms(med["unmasked"]), "min": ms(min(times["unmasked"])),
                              "max": ms(max(times["unmasked"])), "spread": ms(spread)},
              "masked_ms": {"median": ms(med["body"]), "min": ms(min(times["body"])),
                            "max": ms(max(times["body"]))},
              "full_mask_ms": {"median": ms(med["full"]), "min": ms(min(times["full"])),
                               "max": ms(max(times["full"])), "kept": a.cases * stats["full"]["kept"],
                               "over_unmasked": ms(over), "within_spread": bool(over <= spread)},
              "per_case_us": {"occupancy_body": round(1e6 * occ["body"], 1),
                              "occupancy_full": round(1e6 * occ["full"], 1),
                              "readback": round(1e6 * readback, 1),
                              "blend": blend_us(False), "blend_full_mask": blend_us(True)}}
    warm = {k: ms(min(v[1:]) if len(v) > 1 else v[0]) for k, v in rows.items()}
    out = {"tool": "validate_bench", "device": torch.cuda.get_device_name(0), "cases": a.cases,
           "shape": list(shape), "patch": a.patch, "thresholds": len(THRESHOLDS),
           "first_epoch_ms": {k: ms(v[0]) for k, v in rows.items()},
           "warm_epoch_ms": warm,
           "old_total_ms": round(warm["old_inference"] + warm["old_metrics"], 2),
           "new_total_ms": round(warm["new_inference"] + warm["new_metrics"], 2),
           "components_per_threshold": [m["tp"] + m["fp"] for m in ref],
           "masked_inference": masked}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
