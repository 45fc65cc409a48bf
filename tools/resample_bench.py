"""Device times of resampling a case to the network's grid and a map back
(light_unet/resample.py, csrc/resample.hip) on a synthetic 400 x 400 x 600 volume at
2.04 x 2.04 x 3 mm, to 4 mm (204 x 204 x 450) and back, for float32 and float64 sources, next to
the algorithmic bytes of each leg.

    python tools/resample_bench.py [--repeat 10] [--out profiles/resample_bench.json]

"kernel" is HIP events around the one l3u_resample launch with the tables already on the device
(median of --repeat after a warm-up); "call" is a host clock around resample_volume(device tensor,
output="device") ending in a device synchronise: table construction and upload included.
Algorithmic bytes are the source elements the output actually references, once each, plus the
destination; the fraction is of the 8 TB/s HBM peak.  Where scipy imports, scipy.ndimage.zoom is
timed once on the host for the same arrays and its result compared.  Needs a GPU: no fallback.

    python tools/resample_bench.py --spline [--repeat 10] [--out profiles/spline_bench.json]

runs the order-3 legs instead (resample_spline, csrc/spline.hip) at the same two sizes: HIP events
around l3u_spline_prefilter_passes for each axis pass on its own, around the whole
l3u_spline_prefilter and around the l3u_resample_spline gather with the tables on the device
(medians of --repeat after a warm-up), the host clock around resample_spline(device tensor,
output="device"), and scipy.ndimage.zoom(order=3) once on the host for the float32 legs.
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
from light_unet import resample as RS          # noqa: E402

SHAPE = (400, 400, 600)
SPACING = (2.04, 2.04, 3.0)
TARGET = (4.0, 4.0, 4.0)
HBM_PEAK = 8e12


def referenced(shape, out_shape, order):
    """Source elements the output reads (a product set: every referenced z, y, x combination)."""
    n = 1
    for a, b in zip(shape, out_shape):
        tab = RS.axis_table(a, b, order)
        idx = tab if order == 0 else np.concatenate(tab[:2])
        n *= len(np.unique(idx))
    return n


def leg(src, out_shape, order, repeat):
    shape = tuple(src.shape)
    dst_dtype = torch.float32 if order == 1 else src.dtype
    dst = torch.empty(out_shape, dtype=dst_dtype, device=src.device)
    tab, (lo, hi, t) = RS._tables(shape, out_shape, order, src.device)
    base = tab.data_ptr()
    args = (src.data_ptr(), RS._CODE[src.dtype], *shape, dst.data_ptr(), RS._CODE[dst_dtype],
            *out_shape, order, base + lo, None if hi is None else base + hi,
            None if t is None else base + t, nat.stream())
    for _ in range(3):
        nat.call("l3u_resample", *args)
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        nat.call("l3u_resample", *args)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    call_ms = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = RS.resample_volume(src, out_shape, order=order, output="device")
        torch.cuda.synchronize()
        call_ms.append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(out, dst)
    nbytes = referenced(shape, out_shape, order) * src.element_size() + dst.numel() * dst.element_size()
    med = statistics.median(ms)
    rec = {"shape": list(shape), "out_shape": list(out_shape), "order": order,
           "src_dtype": str(src.dtype).replace("torch.", ""),
           "kernel_median_ms": med, "kernel_min_ms": min(ms),
           "call_median_ms": statistics.median(call_ms),
           "algorithmic_bytes": int(nbytes), "TB_per_s_at_median": nbytes / (med * 1e-3) / 1e12,
           "fraction_of_8TBps": nbytes / (med * 1e-3) / HBM_PEAK}
    return rec, dst


def host_zoom(x, out_shape, order, got):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    t0 = time.perf_counter()
    ref = ndimage.zoom(x, [o / n for o, n in zip(out_shape, x.shape)], order=order, mode="nearest",
                       grid_mode=True)
    s = time.perf_counter() - t0
    ref = ref.astype(got.dtype)
    return {"scipy_zoom_s": s, "voxels_differing_from_scipy": int((ref != got).sum()),
            "max_abs_difference": float(np.abs(ref.astype(np.float64) - got.astype(np.float64)).max())}


def events_ms(fn, repeat):
    """Median and minimum of HIP-event times around fn(), after 2 warm-up calls."""
    for _ in range(2):
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
    return statistics.median(ms), min(ms)


def spline_leg(src, out_shape, repeat):
    shape = tuple(src.shape)
    pad = RS.SPLINE_PAD
    coef = torch.empty(tuple(n + 2 * pad for n in shape), dtype=torch.float64, device=src.device)
    dst = torch.empty(out_shape, dtype=torch.float32, device=src.device)
    tab, start = RS._spline_tables(shape, out_shape)
    tab = tab.to(src.device)
    pre = (src.data_ptr(), RS._CODE[src.dtype], *shape, coef.data_ptr(), *RS.spline_constants())
    rec = {"shape": list(shape), "out_shape": list(out_shape), "order": 3,
           "src_dtype": str(src.dtype).replace("torch.", ""),
           "coefficient_bytes": coef.numel() * 8}
    # axis 0 writes coef from src; axes 1 and 2 run in place on what coef holds (timing only: the
    # values of a pass that is repeated are not the coefficients)
    for name, bit in (("axis0", 1), ("axis1", 2), ("axis2", 4)):
        med, lo = events_ms(lambda: nat.call("l3u_spline_prefilter_passes", *pre, bit, nat.stream()),
                            repeat)
        rec[f"prefilter_{name}_median_ms"], rec[f"prefilter_{name}_min_ms"] = med, lo
    med, lo = events_ms(lambda: nat.call("l3u_spline_prefilter", *pre, nat.stream()), repeat)
    rec["prefilter_median_ms"], rec["prefilter_min_ms"] = med, lo
    gather = (coef.data_ptr(), *shape, dst.data_ptr(), *out_shape, tab.data_ptr() + start,
              tab.data_ptr(), 0.0, 0.0, 0)
    med, lo = events_ms(lambda: nat.call("l3u_resample_spline", *gather, nat.stream()), repeat)
    rec["gather_median_ms"], rec["gather_min_ms"] = med, lo
    del coef
    call_ms = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = RS.resample_spline(src, out_shape, output="device")
        torch.cuda.synchronize()
        call_ms.append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(out, dst)
    rec["call_median_ms"] = statistics.median(call_ms)
    return rec, dst


def spline_main(a, shape, small, image):
    res = {"shape": list(shape), "spacing": list(SPACING), "target_spacing": list(TARGET),
           "target_shape": list(small), "device": torch.cuda.get_device_name(0), "repeat": a.repeat,
           "note": "one run on one box; no speed gate; scipy on the host for the float32 legs only"}
    for name, img in (("float32", image), ("float64", image.astype(np.float64))):
        src = torch.from_numpy(img).cuda()
        down, low = spline_leg(src, small, a.repeat)
        print(f"spline {name} down: done", flush=True)
        host = not a.no_host and name == "float32"
        if host:
            down["host"] = host_zoom(img, small, 3, low.cpu().numpy())
            print("scipy down: done", flush=True)
        del src
        back_src = low if name == "float32" else low.to(torch.float64)
        up, native = spline_leg(back_src, shape, a.repeat)
        print(f"spline {name} up: done", flush=True)
        if host:
            up["host"] = host_zoom(back_src.cpu().numpy(), shape, 3, native.cpu().numpy())
            print("scipy up: done", flush=True)
        res[name] = {"down": down, "up": up}
        del back_src, native, low
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, nargs=3, default=list(SHAPE))
    ap.add_argument("--no-host", action="store_true", help="skip scipy.ndimage.zoom on the host")
    ap.add_argument("--spline", action="store_true", help="the order-3 legs (resample_spline) instead")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs a ROCm GPU")
    shape = tuple(a.shape)
    small = RS.resampled_shape(shape, SPACING, TARGET)
    rng = np.random.default_rng(7)
    image = rng.random(shape, dtype=np.float32)
    if a.spline:
        return finish(spline_main(a, shape, small, image), a.out)
    res = {"shape": list(shape), "spacing": list(SPACING), "target_spacing": list(TARGET),
           "target_shape": list(small), "device": torch.cuda.get_device_name(0), "repeat": a.repeat,
           "note": "one run on one box; no speed gate"}
    for name, img in (("float32", image), ("float64", image.astype(np.float64))):
        src = torch.from_numpy(img).cuda()
        down, low = leg(src, small, 1, a.repeat)
        low_np = low.cpu().numpy()
        if not a.no_host:
            down["host"] = host_zoom(img, small, 1, low_np)
        del src
        # the way back: the 4 mm map (float32 or, for the float64 leg, its float64 copy) to native
        back_src = low if name == "float32" else low.to(torch.float64)
        up, native = leg(back_src, shape, 1, a.repeat)
        if not a.no_host:
            up["host"] = host_zoom(back_src.cpu().numpy(), shape, 1, native.cpu().numpy())
        res[name] = {"down": down, "up": up}
        del back_src, native, low
    label = torch.from_numpy((image > 0.97).astype(np.uint8)).cuda()
    res["label_uint8_order0_down"], _ = leg(label, small, 0, a.repeat)
    finish(res, a.out)


def finish(res, out):
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
