"""Golden fixture for the cubic B-spline resampling (light_unet/resample.py: resample_spline,
csrc/spline.hip), made by scipy itself:

    scipy.ndimage.zoom(x, zoom, order=3, mode="nearest", grid_mode=True)

with zoom = out / in per axis, so that scipy's own round(n * zoom) gives the out shape.  Run with
scipy installed (made with 1.15.3):

    python tests/golden/make_spline_goldens.py        # writes tests/golden/spline.npz

Per case `k` and image `m` (u: float32 U[0, 1); g: float32 gamma(0.7, 3.0), the long-tailed
histogram of an uptake volume, in steps of 1 / 1024 as stored integers times a rescale slope
give, from 1 / 1024 up: where the source is exactly 0 the float64 sum is rounding noise of either
sign, in scipy too, and the identity case would not return the source; default_rng(43)) the file
holds the seeded input k/m and scipy's
outputs: k/m/s32 (order 3 of the float32 image) and k/m/d64, the int8 distance in float32 ulps
from s32 to scipy's order 3 of the float64 image (the float32 one widened) rounded to float32 --
scipy computes both in float64, so the two agree almost everywhere and the distance is what
compresses; scipy64() puts the array back together.  The uniform images of the cases a-f are those of
make_resample_goldens.inputs() (stored in resample.npz and checked there), not stored again.  Case
g is the way back: its inputs are case a's s32 outputs.  `meta` is JSON: shapes, and per case and
source type how many float32 voxels of the plain numpy transcription of the module's definition
(transcription(), below) differ from scipy, and the largest difference of the raw float64 sums
over max|x| (scipy's float64 output against the transcription's sum before its rounding).
"""
import json
import math
import os

import numpy as np

import make_resample_goldens as R

# the shapes of the order-1 goldens (axis length 1, identity, up, down, the way back), then:
# h: a padded row of 324, longer than any x chunk of the prefilter, in a volume with few rows;
# i: output rows wider than one workgroup's 1024 columns, width not a multiple of 4
CASES = {k: v[:2] for k, v in R.CASES.items()}
CASES["h"] = ((2, 3, 300), (5, 2, 130))
CASES["i"] = ((3, 2, 70), (2, 3, 1030))
IMAGES = ("u", "g")
NP = 12     # scipy's pad for mode="nearest": np.pad(x, 12, mode="edge")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "spline.npz")


def inputs():
    """{case: {"u": float32 image, "g": float32 image}} for every case but g."""
    rng = np.random.default_rng(43)
    first = R.inputs()
    out = {}
    for k, (shape, _) in CASES.items():
        if k == "g":
            continue
        u = first[k][0] if k in first else rng.random(shape, dtype=np.float32)
        g = np.maximum(np.round(rng.gamma(0.7, 3.0, shape) * 1024.0), 1.0) / 1024.0
        out[k] = {"u": u, "g": g.astype(np.float32)}
    return out


def stored_inputs():
    """The (case, image) pairs whose input is an array of this file."""
    return [(k, m) for k in CASES if k != "g" for m in IMAGES if not (m == "u" and k in R.CASES)]


def scipy_zoom(x, out_shape):
    from scipy import ndimage
    zoom = [o / n for o, n in zip(out_shape, x.shape)]
    y = ndimage.zoom(x, zoom, order=3, mode="nearest", grid_mode=True)
    assert y.shape == tuple(out_shape), (y.shape, out_shape)
    return y


def scipy64(z, k, m):
    """scipy's order 3 of the float64 image, rounded to float32, from the stored ulp distances."""
    s32 = z[f"{k}/{m}/s32"]
    return (s32.view(np.int32) + z[f"{k}/{m}/d64"].astype(np.int32)).view(np.float32)


def constants():
    z = math.sqrt(3.0) - 2.0
    return z, (1.0 - z) * (1.0 - 1.0 / z), 1.0 / (1.0 - z), z / (z - 1.0)


def coefficients(x):
    """The padded float64 coefficients [D + 24, H + 24, W + 24] of the module's definition: the
    recursion along axis 0, then 1, then 2, vectorised over lines, every product, sum and
    difference a numpy operation of its own."""
    z, lam, k0, kn = constants()
    p = np.pad(x.astype(np.float64), NP, mode="edge")
    for axis in range(3):
        c = np.moveaxis(p, axis, 0)      # a view: the lines of `axis` are c[:, j, k]
        n = c.shape[0]
        c[...] = c * lam
        c[0] = c[0] * k0
        for i in range(1, n):
            c[i] = c[i] + z * c[i - 1]
        c[n - 1] = kn * c[n - 1]
        for i in range(n - 2, -1, -1):
            c[i] = z * (c[i + 1] - c[i])
    return p


def axis_table(n_in, n_out):
    """(start int64, w float64 [n_out, 4]) of one axis."""
    o = np.arange(n_out, dtype=np.float64)
    cc = (o + 0.5) * (n_in / n_out) - 0.5
    f = np.floor(cc)
    y = cc - f
    u = 1.0 - y
    w0 = u * u * u / 6.0
    w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0
    w3 = 1.0 - w0 - w1 - w2
    return f.astype(np.int64) - 1 + NP, np.stack([w0, w1, w2, w3], axis=1)


def transcription(x, out_shape, raw=False, coef=None):
    """The module's definition in plain numpy: the 64-term float64 sum as 64 array operations in
    C order (axis 0 slowest), each term ((coef * w0) * w1) * w2, rounded once to float32 (raw:
    the float64 sum itself)."""
    coef = coefficients(x) if coef is None else coef
    tabs = [axis_table(n, m) for n, m in zip(x.shape, out_shape)]
    acc = np.zeros(out_shape, np.float64)
    for a in range(4):
        for b in range(4):
            for c in range(4):
                v = coef[np.ix_(tabs[0][0] + a, tabs[1][0] + b, tabs[2][0] + c)]
                acc = acc + ((v * tabs[0][1][:, a][:, None, None]) * tabs[1][1][:, b][None, :, None]) \
                    * tabs[2][1][:, c][None, None, :]
    return acc if raw else acc.astype(np.float32)


def build():
    """{array name: array} of the whole fixture, `meta` included."""
    arrays, meta = {}, {"cases": {}}
    ins = inputs()
    stored = set(stored_inputs())
    for k, (shape, out_shape) in CASES.items():
        rec = {"shape": list(shape), "out_shape": list(out_shape)}
        for m in IMAGES:
            img = arrays[f"a/{m}/s32"] if k == "g" else ins[k][m]
            assert img.shape == tuple(shape) and img.dtype == np.float32
            if (k, m) in stored:
                arrays[f"{k}/{m}"] = img
            img64 = img.astype(np.float64)
            s32, s64 = scipy_zoom(img, out_shape), scipy_zoom(img64, out_shape)
            assert s32.dtype == np.float32 and s64.dtype == np.float64
            s64r = s64.astype(np.float32)
            d = s64r.view(np.int32).astype(np.int64) - s32.view(np.int32)
            assert np.abs(d).max() <= 127
            arrays[f"{k}/{m}/s32"], arrays[f"{k}/{m}/d64"] = s32, d.astype(np.int8)
            raw = transcription(img, out_shape, raw=True)
            assert np.array_equal(raw, transcription(img64, out_shape, raw=True))   # widened alike
            t = raw.astype(np.float32)
            rec[m] = {"transcription_differs_s32": int((t != s32).sum()),
                      "transcription_differs_s64": int((t != s64r).sum()),
                      "raw_float64_difference_over_max": float(np.abs(raw - s64).max()
                                                               / np.abs(img64).max())}
        meta["cases"][k] = rec
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return arrays


if __name__ == "__main__":
    arrays = build()
    np.savez_compressed(OUT, **arrays)
    print(json.dumps(json.loads(bytes(arrays["meta"]).decode()), indent=1))
    print(OUT, os.path.getsize(OUT), "bytes")
