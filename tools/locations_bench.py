"""Patch-location sampling timed on the host against the device, and the count launch against
its bytes (csrc/locate.hip; light_unet/patches.py locate="host" / "device").

    python tools/locations_bench.py [--cases 6] [--shape 168 168 400] [--out FILE]

Synthetic whole-body-sized cases with body masks (an ellipsoid body, a few lesion balls).  All
figures come from one run, after one warm-up of every path (code objects, allocator):
  * construct_*_ms: DevicePatchDataset(...) on the host clock, ending in a device synchronise,
    median / min / max of --reps: locate="host" and locate="device" from the same numpy cases
    (both upload image and label), and locate="device" from cases that are already device
    tensors with torch.bool masks (what preprocess_volume(output="device") leaves in HBM);
  * locate_*_ms: the location step alone: DevicePatchDataset._sample_locations on the numpy
    cases against sample_locations_device on the resident ones;
  * count_us: one l3u_loc_count call (count launches + the scan launch) by HIP events around a
    replayed hipGraph of one call per case (a replay is bounded by the device, not by the
    host's enqueue rate; the six cases' 340 MB of labels and masks do not fit the 256 MB
    last-level cache together, so a call does not find its volume cached), median of
    --count-reps replays, beside its algorithmic bytes n * (sizeof(label) + 1) and the fraction
    of the 8 TB/s peak that implies; float32 and float64 labels;
  * copy_us: torch's copy_ of the same float32 volumes (1 read + 1 write stream, as
    tools/membw.py's copy) timed the same way: the practical ceiling of this box.
The host and device datasets are checked to hold the same locations.  Prints one JSON line (and
writes it to --out).  Needs the GPU; not part of bench.py.
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

PEAK_BPS = 8e12


def synthetic_case(shape, seed):
    rng = np.random.default_rng(seed)
    img = rng.random(shape, dtype=np.float32) * 0.3
    lab = np.zeros(shape, np.float32)
    ax = [np.arange(s, dtype=np.float32) for s in shape]
    for _ in range(8):
        c = [rng.integers(10, s - 10) for s in shape]
        r = rng.uniform(4, 9)
        m = ((ax[0][:, None, None] - c[0]) ** 2 + (ax[1][None, :, None] - c[1]) ** 2 +
             (ax[2][None, None, :] - c[2]) ** 2) <= r * r
        lab[m] = 1.0
    body = (((ax[0][:, None, None] - shape[0] / 2) / (0.45 * shape[0])) ** 2 +
            ((ax[1][None, :, None] - shape[1] / 2) / (0.45 * shape[1])) ** 2 +
            ((ax[2][None, None, :] - shape[2] / 2) / (0.5 * shape[2])) ** 2) <= 1.0
    return img, lab, body


def host_ms(fn, reps):
    fn()                                            # warm-up
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(out), "min": min(out), "max": max(out)}


def graphed(fn):
    """fn's launches captured into one hipGraph (after a warm-up on a side stream), so that a
    timed window is bounded by the device and not by the host's enqueue rate."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        fn()
    return g.replay


def window_us(fn, calls, reps):
    """fn() launches `calls` calls; per-call microseconds by HIP events, median of reps windows."""
    fn = graphed(fn)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return {"median": statistics.median(out), "min": min(out), "max": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=6)
    ap.add_argument("--shape", type=int, nargs=3, default=[168, 168, 400])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count-reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("locations_bench needs the ROCm GPU")
    from light_unet import patches as P

    dev = torch.device("cuda:0")
    shape = tuple(a.shape)
    n = int(np.prod(shape))
    cases = [synthetic_case(shape, 100 + k) for k in range(a.cases)]
    resident = [tuple(torch.from_numpy(v).to(dev) for v in c) for c in cases]
    kw = dict(patch_size=(48, 48, 48), seed=42)

    res = {"box": torch.cuda.get_device_name(0), "cases": a.cases, "shape": list(shape), "voxels": n,
           "reps": a.reps, "count_reps": a.count_reps}
    host = P.DevicePatchDataset(cases, locate="host", **kw)
    devd = P.DevicePatchDataset(resident, locate="device", **kw)
    same = all(len(x) == len(y) and all(c == d and (p == q).all() for (c, p), (d, q) in zip(x, y))
               for x, y in ((host.lesion_locations, devd.lesion_locations),
                            (host.background_locations, devd.background_locations)))
    if not same:
        raise SystemExit("host and device locations differ")
    res["locations"] = {"lesion": len(host.lesion_locations), "background": len(host.background_locations),
                        "host_equals_device": same}
    cnt = P.location_counts([c[1] for c in resident], [c[2] for c in resident])
    res["voxels_per_case"] = {"lesion": cnt[:, 0].tolist(), "background": cnt[:, 1].tolist()}
    del host, devd

    res["construct_host_ms"] = host_ms(lambda: P.DevicePatchDataset(cases, locate="host", **kw), a.reps)
    res["construct_device_ms"] = host_ms(lambda: P.DevicePatchDataset(cases, locate="device", **kw), a.reps)
    res["construct_device_resident_ms"] = host_ms(
        lambda: P.DevicePatchDataset(resident, locate="device", **kw), a.reps)

    def loc_host():
        np.random.seed(42)
        P.DevicePatchDataset._sample_locations(cases)

    def loc_dev():
        np.random.seed(42)
        P.sample_locations_device([c[1] for c in resident], [c[2] for c in resident])
    res["locate_host_ms"] = host_ms(loc_host, a.reps)
    res["locate_device_ms"] = host_ms(loc_dev, a.reps)

    # ---- the count call against its bytes
    labels = {"float32": [c[1] for c in resident],
              "float64": [c[1].double() for c in resident]}
    bodies = [c[2] for c in resident]
    for name, labs in labels.items():
        inputs = P._loc_inputs(labs, bodies)
        keep = []                                   # the captured calls' workspaces

        def counts():
            keep.append(P._loc_count_launch(inputs))
        t = window_us(counts, a.cases, a.count_reps)
        nbytes = n * (labs[0].element_size() + 1)
        t["bytes"] = nbytes
        t["GBps"] = nbytes / t["median"] / 1e3
        t["fraction_of_8TBps"] = nbytes / (t["median"] * 1e-6) / PEAK_BPS
        res[f"count_us_{name}"] = t
    dst = [torch.empty_like(c[1]) for c in resident]

    def copies():
        for d, c in zip(dst, resident):
            d.copy_(c[1])
    t = window_us(copies, a.cases, a.count_reps)
    t["bytes"] = 8 * n
    t["GBps"] = 8 * n / t["median"] / 1e3
    t["fraction_of_8TBps"] = 8 * n / (t["median"] * 1e-6) / PEAK_BPS
    res["copy_us_float32"] = t

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
