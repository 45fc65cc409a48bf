"""Per-stage device times of case preprocessing (light_unet/preprocess.py) on a synthetic PET-like
168 x 168 x 400 volume, for float32 and float64 inputs, next to each stage's algorithmic bytes.

    python tools/preprocess_bench.py [--repeat 30] [--out profiles/preprocess_bench.json]

Stage times are HIP events around the stage's launches on the current stream (median of
--repeat after a warm-up); "end_to_end" is a host clock around preprocess_volume ending in a
device synchronise (output="device") or in the copies to numpy (output="numpy", input upload
included).  Bytes are what the algorithm has to move (inputs read once per sweep, outputs written
once), not what the kernels moved.  Where scipy imports, the numpy / scipy restatement of the
reference's calls is timed once on the same array.  Needs a GPU: there is no fallback.
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

from light_unet import _native as nat          # noqa: E402
from light_unet import lesion                  # noqa: E402
from light_unet import preprocess as PP        # noqa: E402

SHAPE = (168, 168, 400)
CFG = {"intensity": {"clip_percentile_low": 0.5, "clip_percentile_high": 99.5,
                     "normalization_range": [0, 1]},
       "body_mask": {"enabled": True, "threshold": 0.02, "closing_voxels": 5,
                     "keep_largest_component": True, "dilate_voxels": 3},
       "volume_threshold": {"train_cc": 0.5, "inference_cc": 0.1}}


def synthetic(shape, seed=7):
    """Air = exact 0 (more than half), a noisy body ellipsoid, hot spots, a detached table."""
    rng = np.random.default_rng(seed)
    D, H, W = shape
    z, y, x = np.ogrid[:D, :H, :W]
    body = ((z - D / 2) / (D * 0.30)) ** 2 + ((y - H * 0.42) / (H * 0.22)) ** 2 \
        + ((x - W / 2) / (W * 0.45)) ** 2 <= 1.0
    v = np.zeros(shape, np.float32)
    v[body] = rng.gamma(2.0, 0.4, size=int(body.sum())).astype(np.float32) + np.float32(0.05)
    for _ in range(12):
        c = (rng.integers(int(D * 0.3), int(D * 0.7)), rng.integers(int(H * 0.3), int(H * 0.55)),
             rng.integers(int(W * 0.2), int(W * 0.8)))
        r = rng.uniform(2.0, 5.0)
        hot = (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r
        v[hot] = rng.uniform(8.0, 25.0, size=int(hot.sum())).astype(np.float32)
    v[int(D * 0.2):int(D * 0.8), H - 14:H - 10, 20:W - 20] = np.float32(0.6)
    return v


def timed(fn, repeat, warmup=3):
    """Median / min device milliseconds of fn() (HIP events on the current stream)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms)}


def rate(rec, nbytes):
    rec["algorithmic_bytes"] = int(nbytes)
    rec["GB_per_s_at_median"] = nbytes / (rec["median_ms"] * 1e-3) / 1e9
    return rec


def stages(vol, repeat):
    """Per-stage times of preprocess_volume's device work on the device volume `vol`."""
    dev, st = vol.device, nat.stream()
    D, H, W = vol.shape
    n, esz = vol.numel(), vol.element_size()
    f64 = int(vol.dtype == torch.float64)
    packed = D * H * ((W + 63) // 64) * 8
    out = {}
    # exact selection of the four order statistics behind the two percentiles
    l0, l1, _ = PP.percentile_ranks(n, 0.5)
    h0, h1, _ = PP.percentile_ranks(n, 99.5)
    ws = torch.empty(nat.query("l3u_pp_select_ws_bytes") // 8, dtype=torch.int64, device=dev)
    sel = torch.empty(5, dtype=torch.float64, device=dev)
    out["select"] = rate(timed(lambda: nat.call(
        "l3u_pp_select", vol.data_ptr(), f64, n, 4, l0, l1, h0, h1, ws.data_ptr(), sel.data_ptr(), st),
        repeat), esz * n * esz)   # key bytes x n x passes (one pass per key byte)
    out["select"]["passes"] = esz
    lo, hi = PP._clip_values(vol, 0.5, 99.5)
    clip = torch.tensor([lo, hi], dtype=torch.float64).to(dev)
    o32 = torch.empty(vol.shape, dtype=torch.float32, device=dev)
    bits = PP._new_bits(D, H, W, dev)
    out["normalize_f32_and_mask"] = rate(timed(lambda: nat.call(
        "l3u_pp_normalize", vol.data_ptr(), f64, clip.data_ptr(), 1.0, 0.0, 0.02, None,
        o32.data_ptr(), bits.data_ptr(), D, H, W, st), repeat), n * (esz + 4) + packed)
    o64 = torch.empty(vol.shape, dtype=torch.float64, device=dev)
    out["normalize_f64"] = rate(timed(lambda: nat.call(
        "l3u_pp_normalize", vol.data_ptr(), f64, clip.data_ptr(), 1.0, 0.0, 0.02, o64.data_ptr(),
        None, None, D, H, W, st), repeat), n * (esz + 8))
    del o64
    out["closing_dilate5"] = rate(timed(lambda: PP.morph(bits, vol.shape, 5), repeat), 2 * packed)
    dil = PP.morph(bits, vol.shape, 5)
    out["closing_erode5"] = rate(timed(lambda: PP.morph(dil, vol.shape, 5, erode=True), repeat), 2 * packed)
    closed = PP.morph(dil, vol.shape, 5, erode=True)

    def largest():
        comp = lesion.label(PP.unpack(closed, vol.shape, torch.float32), 0.5)
        return PP.pack(comp.labels, "eq", int(np.argmax(comp.sizes())) + 1)
    # unpack (4n written), label + stats (lesion.label: its own passes and two host reads), pack (4n read)
    out["largest_component"] = rate(timed(largest, repeat), 2 * packed + 8 * n)
    out["largest_component"]["note"] = "lesion.label with its host read-backs; bytes: unpack + pack only"
    big = largest()
    out["dilate3"] = rate(timed(lambda: PP.morph(big, vol.shape, 3), repeat), 2 * packed)
    s = torch.empty(7, dtype=torch.int64, device=dev)
    out["mask_stats"] = rate(timed(lambda: PP._stats_into(s, big, vol.shape), repeat), packed)
    out["device_stage_sum_ms"] = sum(out[k]["median_ms"] for k in (
        "select", "normalize_f32_and_mask", "closing_dilate5", "closing_erode5",
        "largest_component", "dilate3")) + 4 * out["mask_stats"]["median_ms"]
    return out


def end_to_end(image, repeat):
    res = {}
    dvol = torch.from_numpy(image).cuda()
    for name, src, output in (("device_in_device_out", dvol, "device"), ("numpy_in_numpy_out", image, "numpy")):
        ms = []
        for i in range(repeat + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            PP.preprocess_volume(src, CFG, spacing=[4.0, 4.0, 4.0], output=output)
            torch.cuda.synchronize()
            if i >= 2:
                ms.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"median_ms": statistics.median(ms), "min_ms": min(ms)}
    return res


def host_restatement(image64):
    """The reference's numpy / scipy calls, restated, timed once each on the same array."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    t = {}
    t0 = time.perf_counter()
    lo, hi = np.percentile(image64, 0.5), np.percentile(image64, 99.5)
    norm = (np.clip(image64, lo, hi) - lo) / (hi - lo)
    norm = norm * 1 + 0
    t["normalize_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    m = norm > 0.02
    cross = ndimage.generate_binary_structure(3, 1)
    m = ndimage.binary_closing(m, structure=ndimage.iterate_structure(cross, 5))
    t["closing_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    lab, num = ndimage.label(m)
    sizes = ndimage.sum(m, lab, range(1, num + 1))
    m = lab == (np.argmax(sizes) + 1)
    t["largest_component_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    m = ndimage.binary_dilation(m, structure=cross, iterations=3)
    t["dilate_s"] = time.perf_counter() - t0
    t["total_s"] = sum(t.values())
    t["final_voxels"] = int(m.sum())
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy / scipy restatement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench needs a ROCm GPU")
    image = synthetic(SHAPE)
    res = {"shape": list(SHAPE), "voxels": int(image.size), "zeros_fraction": float((image == 0).mean()),
           "device": torch.cuda.get_device_name(0), "repeat": a.repeat}
    for name, img in (("float32", image), ("float64", image.astype(np.float64))):
        vol = torch.from_numpy(img).cuda()
        r = stages(vol, a.repeat)
        r["end_to_end"] = end_to_end(img, max(5, a.repeat // 3))
        _, mask, meta = PP.preprocess_volume(vol, CFG, output="device")
        r["final_voxels"] = meta["body_mask"]["voxel_counts"]["final"]
        r["clip_values"] = [meta["clip_values"]["min"], meta["clip_values"]["max"]]
        res[name] = r
        del vol
    if not a.no_host:
        res["numpy_scipy_restatement_float64"] = host_restatement(image.astype(np.float64))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
