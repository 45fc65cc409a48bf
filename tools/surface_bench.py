"""Device times of the surface-distance metrics (light_unet/surface.py, csrc/surface.hip) on a
synthetic case of blobs: 204 x 204 x 450 voxels at 4 mm, and the same case as 400 x 400 x 600 at
(3, 2.04, 2.04) mm where the memory allows (--no-large skips it).

    python tools/surface_bench.py [--repeat 10] [--out profiles/surface_bench.json] [--no-host]

Medians of --repeat runs after a warm-up, HIP events around the native calls: one l3u_edt of the
target's surface (the transform surface_distances runs), each of its three passes on the buffers
the previous pass left, and l3u_surf_reduce; a host clock (ending in a device synchronise) around a
whole surface_distances call on device-resident masks.  Algorithmic bytes of the transform are the
packed mask read once and the float64 map written once; the fraction is of the 8 TB/s HBM peak.
Where scipy imports, scipy.ndimage.distance_transform_edt is timed once on the host for the same
mask, the voxels that differ from it are counted (and, where there are any, the brute-force float
minimum of the contract is evaluated at up to 64 of them), and the whole metric is evaluated on the host
with scipy and numpy for comparison.  Needs a GPU: no fallback.
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
from light_unet import surface as SF           # noqa: E402

CASES = [("204x204x450_4mm", (204, 204, 450), (4.0, 4.0, 4.0)),
         ("400x400x600_3x2.04mm", (400, 400, 600), (3.0, 2.04, 2.04))]
TOLERANCES = (2.0, 4.0)
HBM_PEAK = 8e12


def blobs(shape, spacing, dev, shift_mm=(0.0, 0.0, 0.0), scale=1.0, skip=0, seed=11):
    """A union of ellipsoids placed in mm (the same bodies on either grid), as a bool device
    volume; evaluated on the device from three 1-D coordinate vectors."""
    rng = np.random.default_rng(seed)
    ext = [n * s for n, s in zip(shape, spacing)]
    ax = [(torch.arange(n, device=dev, dtype=torch.float32) + 0.5) * s for n, s in zip(shape, spacing)]
    m = torch.zeros(shape, dtype=torch.bool, device=dev)
    for i in range(40):
        c = [rng.uniform(0.1 * e, 0.9 * e) for e in ext]
        r = [rng.uniform(8.0, 40.0) * scale for _ in range(3)]
        if i < skip:
            continue
        d = (((ax[0] - c[0] - shift_mm[0]) / r[0]) ** 2)[:, None, None] \
            + (((ax[1] - c[1] - shift_mm[1]) / r[1]) ** 2)[None, :, None] \
            + (((ax[2] - c[2] - shift_mm[2]) / r[2]) ** 2)[None, None, :]
        m |= d <= 1.0
    return m


def timed(fn, repeat):
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
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def host_metrics(pred, target, spacing, q=95.0):
    from scipy import ndimage as ndi
    cross = ndi.generate_binary_structure(3, 1)
    t_all = time.perf_counter()
    sp, st = pred & ~ndi.binary_erosion(pred, cross), target & ~ndi.binary_erosion(target, cross)
    t0 = time.perf_counter()
    edt_t = ndi.distance_transform_edt(~st, sampling=spacing)
    edt_s = time.perf_counter() - t0
    d_pt, d_tp = edt_t[sp], ndi.distance_transform_edt(~sp, sampling=spacing)[st]
    n = len(d_pt) + len(d_tp)
    res = {"hd": float(max(d_pt.max(), d_tp.max())),
           "hd95": float(max(np.percentile(d_pt, q), np.percentile(d_tp, q))),
           "assd": float((d_pt.sum() + d_tp.sum()) / n),
           "nsd": [(int((d_pt <= t).sum()) + int((d_tp <= t).sum())) / n for t in TOLERANCES],
           "n_pred": len(d_pt), "n_target": len(d_tp)}
    return edt_t, edt_s, time.perf_counter() - t_all, res, st


def contract_at(voxels, feat, spacing):
    """The float minimum l3u_edt is defined as (include/l3u.h), by brute force over every feature
    voxel, at the given voxels: numpy float64, each product and sum rounded once, z, y, x order."""
    f = np.argwhere(feat).astype(np.float64)
    s = np.asarray(spacing, dtype=np.float64)
    out = []
    for v in voxels:
        d = (np.asarray(v, dtype=np.float64) - f) * s
        d = d * d
        out.append(float(np.sqrt(((d[:, 0] + d[:, 1]) + d[:, 2]).min())))
    return np.asarray(out)


def case(shape, spacing, repeat, host):
    dev = torch.device("cuda", torch.cuda.current_device())
    target = blobs(shape, spacing, dev)
    pred = blobs(shape, spacing, dev, shift_mm=(3.0, -5.0, 4.0), scale=1.08, skip=2)
    n = target.numel()
    st = SF.surface_mask(target)
    n_pred, n_target = SF._counts([SF.surface_mask(pred), st], shape)
    out = torch.empty(shape, dtype=torch.float64, device=dev)
    tmp = torch.empty_like(out)
    rec = {"shape": list(shape), "spacing": list(spacing), "voxels": n,
           "surface_voxels": {"pred": n_pred, "target": n_target}}
    rec["edt"] = timed(lambda: SF._edt_bits(st, shape, spacing, 7, out, tmp), repeat)
    for name, bit in (("edt_pass_z", 1), ("edt_pass_y", 2), ("edt_pass_x", 4)):
        # z leaves its result in out, y reads out and writes tmp, x reads tmp: each pass is timed
        # on what the one before it wrote
        rec[name] = timed(lambda: SF._edt_bits(st, shape, spacing, bit, out, tmp), repeat)
    nbytes = st.numel() * 8 + n * 8
    med = rec["edt"]["median_ms"] * 1e-3
    rec["edt"].update(algorithmic_bytes=int(nbytes), TB_per_s_at_median=nbytes / med / 1e12,
                      fraction_of_8TBps=nbytes / med / HBM_PEAK)
    edt = out.clone()
    sd = torch.empty_like(edt)
    part = torch.empty(nat.query("l3u_surf_nblocks", n) * 12, dtype=torch.float64, device=dev)
    res = torch.empty(11, dtype=torch.float64, device=dev)
    tol = np.asarray(TOLERANCES, dtype=np.float64)
    sp_bits = SF.surface_mask(pred)
    rec["surf_reduce"] = timed(lambda: nat.call(
        "l3u_surf_reduce", edt.data_ptr(), sp_bits.data_ptr(), tol.ctypes.data, len(tol),
        sd.data_ptr(), part.data_ptr(), res.data_ptr(), *shape, nat.stream()), repeat)
    del sd, part, tmp, out
    calls = []
    for _ in range(repeat + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = SF.surface_distances(pred, target, spacing=spacing, tolerances_mm=TOLERANCES)
        torch.cuda.synchronize()
        calls.append((time.perf_counter() - t0) * 1e3)
    rec["surface_distances_call"] = {"median_ms": statistics.median(calls[1:]), "min_ms": min(calls[1:]),
                                     "max_ms": max(calls[1:]), "result": got}
    if host:
        try:
            ref_edt, edt_s, whole_s, ref, st_host = host_metrics(pred.cpu().numpy(), target.cpu().numpy(),
                                                        spacing)
        except ImportError:
            rec["host"] = None
            return rec
        dev_edt = edt.cpu().numpy()
        # where the two maps differ, the contract decides: the brute-force float minimum there
        where = np.argwhere(dev_edt.view(np.uint64) != ref_edt.view(np.uint64))[:64]
        differing = None
        if len(where):
            bf = contract_at(where, st_host, spacing)
            dv, sv = dev_edt[tuple(where.T)], ref_edt[tuple(where.T)]
            differing = {"checked": len(where), "device_equals_contract": int((dv == bf).sum()),
                         "scipy_equals_contract": int((sv == bf).sum()),
                         "first": {"voxel": where[0].tolist(), "device": float(dv[0]).hex(),
                                   "scipy": float(sv[0]).hex(), "contract": float(bf[0]).hex()}}
        rec["host"] = {"differing_voxels_against_the_contract": differing,
                       "scipy_edt_s": edt_s, "scipy_numpy_surface_distances_s": whole_s,
                       "edt_voxels_differing_from_scipy":
                           int((dev_edt.view(np.uint64) != ref_edt.view(np.uint64)).sum()),
                       "result": ref,
                       "exact_keys_equal": all(got[k] == ref[k] for k in
                                               ("hd", "hd95", "nsd", "n_pred", "n_target")),
                       "assd_relative_difference": abs(got["assd"] - ref["assd"]) / ref["assd"]}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip scipy on the host")
    ap.add_argument("--no-large", action="store_true", help="skip the 400 x 400 x 600 case")
    ap.add_argument("--only", default=None, help="run the one case of this name")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_bench needs a ROCm GPU")
    res = {"device": torch.cuda.get_device_name(0), "repeat": a.repeat, "tolerances_mm": list(TOLERANCES),
           "note": "one run on one box; no speed gate"}
    for name, shape, spacing in CASES:
        if (a.no_large and name != CASES[0][0]) or (a.only and name != a.only):
            continue
        try:
            res[name] = case(shape, spacing, a.repeat, not a.no_host)
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
