"""Mirror test-time augmentation in the sliding window (`tta_flips`), timed on synthetic cases
shaped like those of tools/validate_bench.py: 3 volumes of 128 x 128 x 256 (its uniform-noise
images, without the blob maps the metrics need), a seed-42 Lightweight3DUNet, patch 48, overlap
0.5, device-resident images and maps, one forward cache for all legs.

    python tools/tta_bench.py [--repeats 10] [--parent-root DIR] [--out profiles/tta_bench.json]

Legs, run alternating `--repeats` times in one process, medians reported: `tta_flips` off, (2,)
(K = 2) and "all" (K = 8).  `ratio` is t_K / (K * t_off): 1.0 means the augmentation costs exactly
its K forwards.  `per_case_us` times what the augmentation adds besides the forwards, on its own
with device events: the flipped gathers plus the merges of one case (every forward's launch pair,
no network in between), next to the plain gathers plus the copies into the prediction buffer.

`--parent-root DIR` (a built checkout of the parent commit) adds the plain path against that
commit: child processes (`--role plain`, which times only the plain leg) are started alternately on
DIR's package and this one's, `--ab-rounds` times each, before this process touches the device.
`plain_vs_parent.within_spread` says whether the two medians differ by no more than the parent's
own min-max spread.  Prints one JSON line and writes it to `--out`.  Not part of bench.py.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_ROOT = os.environ.get("L3U_BENCH_ROOT", ROOT)
sys.path.insert(0, os.path.join(PKG_ROOT, "light-3d-unet-front_amd"))
sys.path.insert(1, os.path.join(ROOT, "tools"))


def ms(v):
    return round(1e3 * v, 2)


def summary(times):
    return {"median": ms(float(np.median(times))), "min": ms(min(times)), "max": ms(max(times)),
            "spread": ms(max(times) - min(times))}


def plain_children(parent_root, rounds, repeats, shape, cases):
    """Plain-leg times of child processes on the parent's package and on this one's, alternating."""
    rows = {"parent": [], "this": []}
    for _ in range(rounds):
        for name, root in (("parent", parent_root), ("this", ROOT)):
            env = dict(os.environ, L3U_BENCH_ROOT=os.path.abspath(root))
            env.pop("L3U_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--role", "plain", "--repeats",
                   str(repeats), "--cases", str(cases), "--shape", *[str(s) for s in shape]]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"plain child ({name}) failed: {r.stderr[-2000:]}")
            rows[name] += json.loads(r.stdout.strip().splitlines()[-1])["plain_s"]
    med = {k: float(np.median(v)) for k, v in rows.items()}
    spread = max(rows["parent"]) - min(rows["parent"])
    return {"rounds": rounds, "repeats_per_round": repeats, "parent_ms": summary(rows["parent"]),
            "this_ms": summary(rows["this"]), "this_over_parent_ms": ms(med["this"] - med["parent"]),
            "within_spread": bool(abs(med["this"] - med["parent"]) <= spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 256])
    ap.add_argument("--patch", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--role", choices=["all", "plain"], default="all")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_bench.json"))
    a = ap.parse_args()
    shape, patch = tuple(a.shape), (a.patch,) * 3

    ab = None
    if a.role == "all" and a.parent_root:
        ab = plain_children(a.parent_root, a.ab_rounds, max(3, a.repeats // 2), shape, a.cases)

    import torch
    from light_unet import _native as nat
    from light_unet.models.unet3d import Lightweight3DUNet
    from light_unet.utils import sliding_window_inference_3d as sw, window_positions
    from validate_bench import blob_case, timed

    dev = torch.device("cuda", 0)
    torch.manual_seed(42)
    model = Lightweight3DUNet(dropout_p=0.0).to(dev)
    images = [torch.from_numpy(blob_case(shape, 100 + i, 0)[0]).to(dev) for i in range(a.cases)]
    cache = {}

    def infer(flips, st=None):
        kw = {} if flips is None else {"tta_flips": flips}      # the parent has no such keyword
        return [sw(img, model, patch, 0.5, dev, True, output="device", forward_cache=cache,
                   stats=st, **kw) for img in images]

    if a.role == "plain":
        infer(None)
        print(json.dumps({"plain_s": [timed(lambda: infer(None))[0] for _ in range(a.repeats)]}))
        return

    legs = {"off": None, "w": (2,), "all": "all"}
    stats = {k: {} for k in legs}
    maps = {k: infer(f, stats[k]) for k, f in legs.items()}       # warm-up and captures
    change = {k: max(float((x - y).abs().max()) for x, y in zip(maps[k], maps["off"]))
              for k in ("w", "all")}
    del maps
    times = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, f in legs.items():
            times[k].append(timed(lambda: infer(f))[0])
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread_off = max(times["off"]) - min(times["off"])
    ratios = {}
    for k, K in (("w", 2), ("all", 8)):
        r = [t / (K * med["off"]) for t in times[k]]
        ratios[k] = {"K": K, "ratio": round(med[k] / (K * med["off"]), 4),
                     "ratio_min": round(min(r), 4), "ratio_max": round(max(r), 4),
                     # the relative spread of the plain leg carries over to the ratio
                     "plain_relative_spread": round(spread_off / med["off"], 4),
                     "forwards_per_case": stats[k]["forwards"]}

    # ---- what the augmentation adds per case besides the forwards: gathers and merges on their own
    grid = [window_positions(s, a.patch, a.patch // 2) for s in shape]
    order = [(z, y, x) for z in grid[0] for y in grid[1] for x in grid[2]]
    nwin, P, B = len(order), a.patch ** 3, 16
    vol = images[0]
    preds = torch.empty(nwin + B, P, device=dev)

    def extra_us(K):
        wpf = B // K
        R = wpf * K
        codes = [c for c in range(8) if c & ~{1: 0, 2: 4, 8: 7}[K] == 0]
        pos = torch.tensor(order + [order[-1]] * ((-nwin) % wpf), dtype=torch.int32, device=dev)
        pos = pos.repeat_interleave(K, dim=0)
        x = torch.empty(R, P, device=dev)
        rows = torch.rand(R, P, device=dev)
        rc, mc = (ctypes.c_int * R)(*(codes * wpf)), (ctypes.c_int * K)(*codes)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(a.repeats + 1):      # the first pass warms up
            if i == 1:
                ev[0].record()
            for b0 in range(0, nwin, wpf):
                p = pos[b0 * K:(b0 + wpf) * K]
                if K == 1:
                    nat.call("l3u_window_gather", vol.data_ptr(), *shape, p.data_ptr(), R, *patch,
                             x.data_ptr(), nat.stream())
                    preds[b0:b0 + wpf].copy_(rows)
                else:
                    nat.call("l3u_window_gather_flip", vol.data_ptr(), *shape, p.data_ptr(), rc, R,
                             *patch, x.data_ptr(), nat.stream())
                    nat.call("l3u_window_tta_merge", rows.data_ptr(), mc, K, wpf, *patch,
                             nat.ptr(preds, b0 * P), nat.stream())
        ev[1].record()
        torch.cuda.synchronize()
        return round(1e3 * ev[0].elapsed_time(ev[1]) / a.repeats, 1)

    per_case = {"plain_gather_copy": extra_us(1), "flip_gather_merge_K2": extra_us(2),
                "flip_gather_merge_K8": extra_us(8)}
    out = {"tool": "tta_bench", "device": torch.cuda.get_device_name(0), "cases": a.cases,
           "shape": list(shape), "patch": a.patch, "window_batch": 16, "repeats": a.repeats,
           "windows_per_case": nwin,
           "off_ms": summary(times["off"]), "K2_ms": summary(times["w"]), "K8_ms": summary(times["all"]),
           "K2": ratios["w"], "K8": ratios["all"],
           "max_change_from_plain": {"K2": round(change["w"], 4), "K8": round(change["all"], 4)},
           "per_case_us": per_case, "plain_vs_parent": ab}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
