"""The training-patch loaders timed against the step they feed: host draws (DevicePatchDataset,
draws="host": the reference's RNG calls in Python, an upload of the records and the float64
noise, one l3u_aug_patches launch pair) against device draws (draws="device": one replay of the
captured l3u_aug_draw -> l3u_aug_patches -> l3u_counter_add chain), in the same run.

    python tools/patch_loader_bench.py [--cases 6] [--shape 96 96 128] [--epochs 5]

Synthetic cases resident in HBM, the reference augmentation config, patch 48^3, batch 4, the
flagship Lightweight3DUNet with FocalTverskyLoss and AdamW.  Both datasets hold the same cases
and the same sampled locations (trimmed to whole batches, so every step is a replayed one); they
differ only in where the per-item draws are made.  Per epoch of `batches` batches, each figure
the median over --epochs repetitions after one warm-up epoch of everything (captures, code
objects, allocator), host and device epochs alternating, one device synchronise at the end of
each timed epoch:
  * loader_ms_per_batch: iterating the loader alone;
  * epoch_ms_per_step: fast_trainer.FastLoop fed by the loader (copy into the static inputs +
    graph replay per batch, the losses read once at the end) -- what Trainer.train_epoch runs;
  * step_alone_ms: the same number of TrainStep replays on a static batch, no loader.
`over_step_alone_ms` is how far each epoch stays above the step alone, i.e. the loader cost the
asynchronous replay did NOT hide.  Prints one JSON line.  Not part of bench.py.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-3d-unet-front_amd"))

REF_AUG = {"gaussian_noise": {"enabled": True, "prob": 0.3, "sigma": 0.01},
           "intensity_shift": {"enabled": True, "prob": 0.5, "shift_range": [-0.1, 0.1]},
           "random_flip": {"enabled": True, "prob": 0.5, "axes": [0, 1, 2]},
           "random_rotation": {"enabled": True, "prob": 0.5, "angle_range": [-15, 15],
                               "axes": [[0, 1], [0, 2], [1, 2]]},
           "random_scale": {"enabled": True, "prob": 0.3, "scale_range": [0.9, 1.1]}}


def synthetic_case(shape, seed):
    rng = np.random.default_rng(seed)
    img = rng.random(shape, dtype=np.float32) * 0.3
    lab = np.zeros(shape, np.float32)
    ax = [np.arange(s) for s in shape]
    for _ in range(6):
        c = [rng.integers(8, s - 8) for s in shape]
        r = rng.uniform(3, 7)
        m = ((ax[0][:, None, None] - c[0]) ** 2 + (ax[1][None, :, None] - c[1]) ** 2 +
             (ax[2][None, None, :] - c[2]) ** 2) <= r * r
        lab[m] = 1.0
        img[m] = rng.uniform(0.6, 1.0)
    return img, lab


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=6)
    ap.add_argument("--shape", type=int, nargs=3, default=[96, 96, 128])
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--patch", type=int, default=48)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--max-batches", type=int, default=400)
    a = ap.parse_args()

    from light_unet.fast_trainer import FastLoop
    from light_unet.models.losses import FocalTverskyLoss
    from light_unet.models.unet3d import Lightweight3DUNet
    from light_unet.patches import DevicePatchDataset, DevicePatchLoader

    dev = torch.device("cuda", 0)
    patch = (a.patch,) * 3
    cases = [synthetic_case(tuple(a.shape), 100 + i) for i in range(a.cases)]
    host_ds = DevicePatchDataset(cases, patch, 0.5, REF_AUG, seed=42, device=dev)
    # whole batches only (a ragged last batch would run one eager step per epoch in both loops)
    les, bg = list(host_ds.lesion_locations), list(host_ds.background_locations)
    n = min((len(les) + len(bg)) // a.batch, a.max_batches) * a.batch
    les = les[:min(len(les), n // 2)]
    bg = bg[:n - len(les)]
    host_ds.lesion_locations, host_ds.background_locations = les, bg
    dev_ds = DevicePatchDataset(cases, patch, 0.5, REF_AUG, seed=42, device=dev, locations=(les, bg),
                                draws="device")
    loaders = {"host": DevicePatchLoader(host_ds, a.batch), "device": DevicePatchLoader(dev_ds, a.batch)}
    nb = len(loaders["host"])
    assert nb == len(loaders["device"]) == n // a.batch and n % a.batch == 0

    class Trainer:
        pass
    tr = Trainer()
    torch.manual_seed(42)
    tr.model = Lightweight3DUNet().to(dev).train()
    tr.criterion = FocalTverskyLoss()
    tr.optimizer = torch.optim.AdamW(tr.model.parameters(), lr=1e-4, weight_decay=1e-5)
    loop = FastLoop(tr)

    def loader_epoch(kind):
        for _ in loaders[kind]:
            pass

    def train_epoch(kind):
        loop.begin_epoch(1e-4, nb)
        for x, t in loaders[kind]:
            loop.run(x, t)
        loop.losses()

    def step_alone():
        for _ in range(nb):
            loop.step.replay()

    runs = {"loader_host": lambda: loader_epoch("host"), "loader_device": lambda: loader_epoch("device"),
            "epoch_host": lambda: train_epoch("host"), "epoch_device": lambda: train_epoch("device"),
            "step_alone": step_alone}
    order = ["loader_host", "loader_device", "epoch_host", "epoch_device", "step_alone"]
    first = {k: timed(runs[k]) for k in order}          # warm-up: captures, code objects, allocator
    rows = {k: [] for k in order}
    for _ in range(a.epochs):
        for k in order:
            rows[k].append(timed(runs[k]))

    def ms(v):
        return round(1e3 * v / nb, 4)
    med = {k: ms(statistics.median(v)) for k, v in rows.items()}
    out = {"tool": "patch_loader_bench", "device": torch.cuda.get_device_name(0), "cases": a.cases,
           "shape": list(a.shape), "patch": a.patch, "batch": a.batch, "batches": nb,
           "epochs": a.epochs,
           "loader_ms_per_batch": {"host": med["loader_host"], "device": med["loader_device"]},
           "epoch_ms_per_step": {"host": med["epoch_host"], "device": med["epoch_device"]},
           "step_alone_ms": med["step_alone"],
           "over_step_alone_ms": {"host": round(med["epoch_host"] - med["step_alone"], 4),
                                  "device": round(med["epoch_device"] - med["step_alone"], 4)},
           "device_epoch_faster": med["epoch_device"] < med["epoch_host"],
           "min_max_ms": {k: [ms(min(v)), ms(max(v))] for k, v in rows.items()},
           "warmup_epoch_ms": {k: ms(v) for k, v in first.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
