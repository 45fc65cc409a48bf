"""Device times of the Gaussian smoothing (light_unet/smooth.py, csrc/smooth.hip) at the two sizes
of the other benches: 204 x 204 x 450 at 4 mm with a 6 mm FWHM (radii 3, 3, 3) and 400 x 400 x 600
at (3, 2.04, 2.04) mm with 7 mm (radii 4, 6, 6), float32 gamma noise with the lesions of
tools/surface_bench.py 6 units hotter (tools/quantify_bench.py's uptake).

    python tools/smooth_bench.py [--repeat 10] [--out profiles/smooth_bench.json] [--no-host]
    python tools/smooth_bench.py --ab-parent DIR [--ab-rounds 3]

Medians of --repeat runs after a warm-up, HIP events around the native calls: each l3u_gauss_axis
launch alone (on the source: the time of a launch does not depend on the values), the three in a
row, and a host clock (ending in a device synchronise) around a whole gaussian_filter call on a
device tensor.  Algorithmic bytes of a launch = the source once plus the destination once, over
the 8 TB/s peak.  Where scipy imports, scipy.ndimage.gaussian_filter is timed once on the host for
the same array and the voxels that differ from the device's are counted.  lesion_uptake is timed
with smooth_fwhm_mm and without.  Needs a GPU: no fallback.

--ab-parent DIR: the untouched path.  DIR holds another build of this repository (the parent
commit); tools/quantify_bench.py's 204 x 204 x 450 case (lesion_uptake without smoothing) runs in
child processes alternating between DIR and this tree, --ab-rounds each.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from light_unet import _native as nat          # noqa: E402
from light_unet import quantify as QT          # noqa: E402
from light_unet import smooth as SM            # noqa: E402
from quantify_bench import uptake_of           # noqa: E402
from resegment_bench import ab                 # noqa: E402
from surface_bench import CASES, HBM_PEAK, blobs, timed  # noqa: E402

FWHM = {CASES[0][0]: 6.0, CASES[1][0]: 7.0}


def host_clock(fn, repeat):
    ms = []
    for _ in range(repeat + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms[1:]), "min_ms": min(ms[1:]), "max_ms": max(ms[1:])}


def case(name, shape, spacing, repeat, host):
    dev = torch.device("cuda", torch.cuda.current_device())
    mask = blobs(shape, spacing, dev)
    up = uptake_of(mask)
    fwhm = FWHM[name]
    sig = SM.fwhm_sigma(fwhm, spacing)
    tables = SM.weight_tables(sig)
    radii = [(len(w) - 1) // 2 for w in tables]
    nbytes = 2 * up.numel() * 4
    rec = {"shape": list(shape), "spacing": list(spacing), "voxels": up.numel(), "fwhm_mm": fwhm,
           "sigma_voxels": list(sig), "radii": radii, "dtype": "float32", "mode": "reflect",
           "algorithmic_bytes_per_launch": nbytes}
    wd = [torch.from_numpy(w).to(dev) for w in tables]
    a, b = torch.empty_like(up), torch.empty_like(up)

    def axis(src, dst, ax):
        nat.call("l3u_gauss_axis", src.data_ptr(), dst.data_ptr(), 0, *shape, ax, wd[ax].data_ptr(),
                 radii[ax], SM.MODES["reflect"], 0.0, nat.stream())

    for ax in range(3):
        t = timed(lambda: axis(up, a, ax), repeat)
        t["fraction_of_peak"] = nbytes / (t["median_ms"] * 1e-3) / HBM_PEAK
        rec[f"axis{ax}"] = t

    def three():
        axis(up, a, 0)
        axis(a, b, 1)
        axis(b, a, 2)

    rec["three_launches"] = timed(three, repeat)
    rec["sum_of_axis_medians_ms"] = sum(rec[f"axis{ax}"]["median_ms"] for ax in range(3))
    del a, b
    rec["gaussian_filter_call"] = host_clock(
        lambda: SM.gaussian_filter(up, sig, output="device"), repeat)
    comp_kw = dict(spacing=spacing)
    rec["lesion_uptake_call"] = host_clock(lambda: QT.lesion_uptake(up, mask, **comp_kw), repeat)
    rec["lesion_uptake_smoothed_call"] = host_clock(
        lambda: QT.lesion_uptake(up, mask, smooth_fwhm_mm=fwhm, **comp_kw), repeat)
    if host:
        try:
            from scipy import ndimage as ndi
        except ImportError:
            rec["host"] = None
            return rec
        got = SM.gaussian_filter(up, sig)
        x = up.cpu().numpy()
        t0 = time.perf_counter()
        want = ndi.gaussian_filter(x, sig, mode="reflect")
        rec["host"] = {"scipy_gaussian_filter_s": time.perf_counter() - t0,
                       "differing_voxels": int((got.view(np.uint32) != want.view(np.uint32)).sum())}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip scipy on the host")
    ap.add_argument("--no-large", action="store_true", help="skip the 400 x 400 x 600 case")
    ap.add_argument("--ab-parent", default=None, help="a built tree of the parent commit")
    ap.add_argument("--ab-rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smooth_bench needs a ROCm GPU")
    if a.ab_parent:
        res = {"device": torch.cuda.get_device_name(0),
               "lesion_uptake_untouched": ab(os.path.abspath(a.ab_parent), a.ab_rounds, a.repeat)}
    else:
        res = {"device": torch.cuda.get_device_name(0), "repeat": a.repeat,
               "note": "one run on one box; no speed gate"}
        for name, shape, spacing in CASES:
            if a.no_large and name != CASES[0][0]:
                continue
            try:
                res[name] = case(name, shape, spacing, a.repeat, not a.no_host)
            except torch.cuda.OutOfMemoryError:
                res[name] = {"skipped": "out of device memory"}
                torch.cuda.empty_cache()
            print(name, json.dumps(res[name]), flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
