"""Writes tests/golden/surface.npz: inputs and expected results for the surface-distance metrics
(light_unet/surface.py, csrc/surface.hip), from scipy and numpy on the CPU.

    python tests/golden/make_surface_goldens.py

Every distance map that is stored, or that a stored metric is computed from, is also evaluated by
brute force as the contract of l3u_edt states it,

    sqrt(min over features f of fl(fl(((z-fz) sz)^2 + ((y-fy) sy)^2) + ((x-fx) sx)^2)),

and the generator asserts that scipy.ndimage.distance_transform_edt gives exactly that map before
it writes anything: the file holds only inputs where scipy's answer is the contract's answer.
Masks are stored bit-packed (np.packbits over the flat C order), floats of the metric dicts as
float.hex strings in one JSON document.  Written with scipy 1.15.3 / numpy.
"""
import json
import os

import numpy as np
from scipy import ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
SPACINGS = [(1.0, 1.0, 1.0), (4.0, 4.0, 4.0), (3.27, 2.0364, 2.0364)]
METRIC_SPACINGS = [(4.0, 4.0, 4.0), (3.27, 2.0364, 2.0364)]
TOLERANCES = (2.0, 4.0)
CROSS = ndi.generate_binary_structure(3, 1)


# ---------------------------------------------------------------- the contract, by brute force
def brute_edt(feat, spacing, chunk=1024):
    """The float minimum over all feature voxels, every product and sum rounded once (numpy float64
    never fuses), summed in z, y, x order; +inf without a feature."""
    feat = np.asarray(feat, dtype=bool)
    D, H, W = feat.shape
    f = np.argwhere(feat)
    out = np.full(feat.size, np.inf)
    if len(f) == 0:
        return out.reshape(feat.shape)
    sq = []
    for n, s in zip((D, H, W), spacing):
        d = (np.arange(n)[:, None] - np.arange(n)[None, :]).astype(np.float64) * np.float64(s)
        sq.append(d * d)
    vz, vy, vx = np.unravel_index(np.arange(feat.size), feat.shape)
    for lo in range(0, feat.size, chunk):
        hi = min(lo + chunk, feat.size)
        a = sq[0][vz[lo:hi]][:, f[:, 0]]
        a = a + sq[1][vy[lo:hi]][:, f[:, 1]]
        a = a + sq[2][vx[lo:hi]][:, f[:, 2]]
        out[lo:hi] = a.min(axis=1)
    return np.sqrt(out).reshape(feat.shape)


def checked_edt(feat, spacing):
    """scipy's distance to the nearest feature voxel, asserted equal to the contract bit for bit."""
    feat = np.asarray(feat, dtype=bool)
    assert feat.any()
    ref = ndi.distance_transform_edt(~feat, sampling=spacing)
    bf = brute_edt(feat, spacing)
    assert ref.dtype == np.float64 and np.array_equal(ref.view(np.uint64), bf.view(np.uint64)), \
        (feat.shape, spacing, int((ref != bf).sum()))
    return ref


# ---------------------------------------------------------------- metrics, as the issue defines them
def surface(a):
    a = np.asarray(a, dtype=bool)
    return a & ~ndi.binary_erosion(a, CROSS)


def metrics(pred, target, spacing, tolerances, q):
    sp, st = surface(pred), surface(target)
    n_p, n_t = int(sp.sum()), int(st.sum())
    if n_p == 0 and n_t == 0:
        return {"hd": 0.0, "hd95": 0.0, "assd": 0.0, "nsd": [1.0] * len(tolerances),
                "n_pred": 0, "n_target": 0}
    if n_p == 0 or n_t == 0:
        inf = float("inf")
        return {"hd": inf, "hd95": inf, "assd": inf, "nsd": [0.0] * len(tolerances),
                "n_pred": n_p, "n_target": n_t}
    d_pt = checked_edt(st, spacing)[sp]
    d_tp = checked_edt(sp, spacing)[st]
    return {"hd": float(max(d_pt.max(), d_tp.max())),
            "hd95": float(max(np.percentile(d_pt, q), np.percentile(d_tp, q))),
            "assd": float((d_pt.sum() + d_tp.sum()) / (n_p + n_t)),
            "nsd": [(int((d_pt <= t).sum()) + int((d_tp <= t).sum())) / (n_p + n_t)
                    for t in tolerances],
            "n_pred": n_p, "n_target": n_t}


def hexed(d):
    return {k: ([float(x).hex() for x in v] if isinstance(v, list)
                else (float(v).hex() if isinstance(v, float) else v)) for k, v in d.items()}


# ---------------------------------------------------------------- inputs
def blobs(shape, rng, count, rmin, rmax):
    zz, yy, xx = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    spec = []
    for _ in range(count):
        c = [rng.uniform(0.15 * n, 0.85 * n) for n in shape]
        r = [rng.uniform(rmin, rmax) for _ in shape]
        spec.append((c, r))

    def draw(spec, shift=(0, 0, 0), scale=1.0):
        m = np.zeros(shape, dtype=bool)
        for c, r in spec:
            m |= (((zz - c[0] - shift[0]) / (r[0] * scale)) ** 2
                  + ((yy - c[1] - shift[1]) / (r[1] * scale)) ** 2
                  + ((xx - c[2] - shift[2]) / (r[2] * scale)) ** 2) <= 1.0
        return m
    return spec, draw


def pair(shape, seed):
    """A blob target and a shifted, perturbed prediction: one blob missed, one spurious, the rest
    moved and grown, and a sprinkle of flipped voxels next to the boundary."""
    rng = np.random.default_rng(seed)
    spec, draw = blobs(shape, rng, 6, 3.0, 8.0)
    target = draw(spec)
    extra, _ = blobs(shape, rng, 1, 2.0, 4.0)
    pred = draw(spec[1:] + extra, shift=(1, 2, -1), scale=1.1)
    near = ndi.binary_dilation(pred, CROSS) ^ ndi.binary_erosion(pred, CROSS)
    pred ^= near & (rng.random(shape) < 0.05)
    return pred, target


def main():
    rng = np.random.default_rng(20250611)
    arrays, index = {}, {"edt": [], "metrics": [], "sweep": None}

    def put_mask(name, m):
        arrays[name] = np.packbits(np.asarray(m, dtype=bool).ravel())

    # ---- distance maps
    def edt_case(tag, feat):
        put_mask(f"edt_{tag}_feat", feat)
        for si, s in enumerate(SPACINGS):
            arrays[f"edt_{tag}_s{si}"] = checked_edt(feat, s)
            index["edt"].append({"feat": f"edt_{tag}_feat", "map": f"edt_{tag}_s{si}",
                                 "shape": list(feat.shape), "spacing": list(s)})

    for shape in ((5, 9, 70), (1, 1, 5)):
        for di, dens in enumerate((0.3, 0.02, 0.001)):
            feat = rng.random(shape) < dens
            if not feat.any():
                feat.flat[rng.integers(feat.size)] = True
            edt_case("x".join(map(str, shape)) + f"_d{di}", feat)
    # 300: longer than a workgroup's outputs on each axis in turn; 600: longer than the 512
    # elements of a line the y and x passes stage whole, so the windowed form runs
    for axis, shape in ((2, (3, 4, 300)), (1, (3, 300, 5)), (0, (300, 3, 4)), (2, (1, 2, 600)),
                        (1, (1, 600, 2))):
        feat = rng.random(shape) < 0.3          # features near one end only: far candidates win
        cut = [slice(None)] * 3
        cut[axis] = slice(3, None)
        feat[tuple(cut)] = False
        feat[0, 0, 0] |= not feat.any()
        edt_case("x".join(map(str, shape)), feat)
        if shape[axis] == 600:                  # and near the other end: the scan's upward side
            edt_case("x".join(map(str, shape)) + "_far", np.flip(feat, axis=axis).copy())
    edt_case("16x16x16_dense", rng.random((16, 16, 16)) < 0.5)
    single = np.zeros((20, 24, 40), dtype=bool)
    single[13, 5, 31] = True
    edt_case("20x24x40_single", single)
    # either side of the 512 elements at which a line is no longer staged whole
    for shape in ((1, 512, 2), (1, 513, 2), (1, 2, 512), (1, 2, 513)):
        edt_case("x".join(map(str, shape)), rng.random(shape) < 0.02)

    # ---- metric dicts
    def metric_case(tag, pred, target, spacings=METRIC_SPACINGS, percentiles=(95.0, 50.0)):
        put_mask(f"m_{tag}_pred", pred)
        put_mask(f"m_{tag}_target", target)
        put_mask(f"m_{tag}_spred", surface(pred))
        put_mask(f"m_{tag}_starget", surface(target))
        for s in spacings:
            for q in percentiles:
                index["metrics"].append({"tag": tag, "shape": list(pred.shape), "spacing": list(s),
                                         "percentile": q, "tolerances": list(TOLERANCES),
                                         "expected": hexed(metrics(pred, target, s, TOLERANCES, q))})

    pa, ta = pair((40, 52, 70), 1)
    pb, tb = pair((64, 56, 72), 2)
    metric_case("a", pa, ta)
    metric_case("b", pb, tb)
    # a crop a host test can recompute with an O(n^2) distance
    z0, y0, x0 = (int(v) for v in np.argwhere(surface(ta) & ~pa)[0])
    z0, y0, x0 = min(max(z0 - 6, 0), 40 - 12), min(max(y0 - 7, 0), 52 - 14), min(max(x0 - 9, 0), 70 - 18)
    crop = (slice(z0, z0 + 12), slice(y0, y0 + 14), slice(x0, x0 + 18))
    assert surface(pa[crop]).any() and surface(ta[crop]).any()
    metric_case("crop", pa[crop], ta[crop])
    one = [METRIC_SPACINGS[1]], (95.0,)
    empty = np.zeros((40, 52, 70), dtype=bool)
    metric_case("both_empty", empty, empty, *one)
    metric_case("pred_empty", empty, ta, *one)
    metric_case("target_empty", pa, empty, *one)
    metric_case("equal", ta, ta, *one)
    faces = np.zeros((40, 52, 70), dtype=bool)      # touches every face: border voxels are surface
    faces[:, 20:30, 30:41] = True
    faces[15:24, :, 30:41] = True
    faces[15:24, 20:30, :] = True
    metric_case("faces", faces, ta, *one)
    metric_case("full", np.ones((40, 52, 70), dtype=bool), ta, *one)
    metric_case("full_full", np.ones((12, 14, 18), dtype=bool), np.ones((12, 14, 18), dtype=bool), *one)

    # ---- a sweep_metrics case: three cases, three thresholds, one empty target.  A map holds a
    # few float32 levels (stored as their uint8 index): the blobs of a pair, nested by erosion.
    levels = np.asarray([0.0, 0.2, 0.4, 0.6, 0.8], dtype=np.float32)
    thresholds = [0.3, 0.5, 0.7]
    spacing = METRIC_SPACINGS[1]
    per_case = []
    for ci in range(3):
        p, t = pair((40, 52, 70), 10 + ci)
        if ci == 1:
            t = np.zeros_like(t)
        lv = np.zeros(p.shape, dtype=np.uint8)
        cur = ndi.binary_dilation(p, CROSS)
        for k in range(1, 5):
            lv[cur] = k
            cur = ndi.binary_erosion(cur, CROSS)
        arrays[f"sweep_level_{ci}"] = lv
        put_mask(f"sweep_target_{ci}", t)
        prob = levels[lv]
        per_case.append([metrics(prob >= np.float32(thr), t, spacing, TOLERANCES, 95.0)
                         for thr in thresholds])
    expected = []
    for k in range(len(thresholds)):
        rows = [c[k] for c in per_case]
        both = [r for r in rows if r["n_pred"] > 0 and r["n_target"] > 0]
        some = [r for r in rows if r["n_pred"] > 0 or r["n_target"] > 0]
        nan = float("nan")
        expected.append(hexed({
            "hd95_mean": float(np.mean([r["hd95"] for r in both])) if both else nan,
            "assd_mean": float(np.mean([r["assd"] for r in both])) if both else nan,
            "nsd_mean": [float(np.mean([r["nsd"][i] for r in some])) if some else nan
                         for i in range(len(TOLERANCES))],
            "surface_cases": len(both)}))
    index["sweep"] = {"shape": [40, 52, 70], "levels": [float(v) for v in levels],
                      "thresholds": thresholds, "spacing": list(spacing),
                      "tolerances": list(TOLERANCES), "percentile": 95.0, "cases": 3,
                      "expected": expected,
                      "per_case": [[hexed(r) for r in c] for c in per_case]}

    arrays["index"] = np.frombuffer(json.dumps(index).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "surface.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(index['edt'])} maps, "
          f"{len(index['metrics'])} metric dicts")


if __name__ == "__main__":
    main()
