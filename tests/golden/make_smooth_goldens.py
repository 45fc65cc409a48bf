"""Golden fixture for the Gaussian smoothing (light_unet/smooth.py: gaussian_filter,
csrc/smooth.hip), made by scipy itself:

    scipy.ndimage.gaussian_filter(x, sigma, mode=mode, cval=cval)

Run with scipy installed (made with scipy 1.15.3, numpy 2.2.6):

    python tests/golden/make_smooth_goldens.py        # writes tests/golden/smooth.npz

Per shape `s` (SHAPES) and image `m` (u: U[0, 1); g: gamma(0.7, 3.0), the long-tailed histogram of
an uptake volume; default_rng(47), drawn in float64) the file holds the input in/s/m as float32;
the float64 cases of the small shapes filter that array widened.  Per case (cases(), named
s/m/k/mode/dtype with k the index of the sigma triple) it holds scipy's output under the case's
name.  w/k/a is the float64 weight table of sigma triple k on axis a (absent where the sigma is 0:
the axis is skipped), checked here against scipy.ndimage._filters._gaussian_kernel1d.  `meta` is
JSON: the case list, scipy's and numpy's versions.

Every stored output equals the numpy transcription of the module's definition (transcription(),
below, the one the tests import) bit for bit; build() asserts that before it writes anything.

What is stored is cut to stay under 1 MB: the three small shapes carry every sigma triple, image
and mode in float32 and every sigma triple and mode in float64 (the image alternating); (9, 20,
67) one case per mode in float32, the sigma triples and the images rotating; (24, 21, 130) one
float32 case, the gamma image with the 6 mm FWHM triple in `reflect`, the consumers' call.  So
every mode, the zero sigma, radii larger than the axis, an axis of length 1 and both dtypes are
there.
"""
import json
import os

import numpy as np

SHAPES = {"a": (1, 3, 70), "b": (3, 2, 4), "c": (5, 7, 9), "d": (9, 20, 67), "e": (24, 21, 130)}
SMALL = ("a", "b", "c")
SIGMAS = ((0.45, 0.45, 0.45), (1.3, 0.0, 2.2), (0.75, 1.06, 1.06), (3.0, 0.6, 1.0))
IMAGES = ("u", "g")
MODES = ("reflect", "mirror", "nearest", "constant")
CVAL = 0.25
TRUNCATE = 4.0
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "smooth.npz")


def inputs():
    """{shape key: {"u": float32 image, "g": float32 image}}."""
    rng = np.random.default_rng(47)
    out = {}
    for s, shape in SHAPES.items():
        out[s] = {"u": rng.random(shape).astype(np.float32),
                  "g": rng.gamma(0.7, 3.0, shape).astype(np.float32)}
    return out


def cases():
    """[(shape key, image, sigma index, mode, dtype name)] of the stored outputs."""
    out = []
    for s in SMALL:
        for k in range(len(SIGMAS)):
            for i, mode in enumerate(MODES):
                for m in IMAGES:
                    out.append((s, m, k, mode, "f32"))
                out.append((s, IMAGES[(k + i) % 2], k, mode, "f64"))
    for i, mode in enumerate(MODES):
        out.append(("d", IMAGES[i % 2], i, mode, "f32"))
    out.append(("e", "g", 2, "reflect", "f32"))
    return out


def name(case):
    s, m, k, mode, dt = case
    return f"{s}/{m}/{k}/{mode}/{dt}"


def case_input(z, case):
    """The array a case filters: the stored float32 image, widened for a float64 case."""
    s, m, _, _, dt = case
    x = z[f"in/{s}/{m}"]
    return x.astype(np.float64) if dt == "f64" else x


# ------------------------------------------------------------------ the definition, in numpy
def radius_of(sigma, truncate=TRUNCATE):
    return int(truncate * float(sigma) + 0.5)


def weights(sigma, radius):
    """The float64 table w[2r + 1] of one axis."""
    sigma = float(sigma)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def weight_tables(sigmas, truncate=TRUNCATE):
    """[w or None per axis]: None where the axis is skipped (sigma <= 1e-15)."""
    return [weights(s, radius_of(s, truncate)) if s > 1e-15 else None for s in sigmas]


def tap_index(k, n, mode):
    """(in-volume index, outside flag) of the taps k (any integers) on an axis of length n."""
    k = np.asarray(k, dtype=np.int64)
    outside = (k < 0) | (k >= n)
    if mode == "reflect":
        m = np.mod(k, 2 * n)
        m = np.where(m >= n, 2 * n - 1 - m, m)
    elif mode == "mirror":
        if n == 1:
            m = np.zeros_like(k)
        else:
            m = np.mod(k, 2 * n - 2)
            m = np.where(m >= n, 2 * n - 2 - m, m)
    elif mode in ("nearest", "constant"):
        m = np.clip(k, 0, n - 1)
    else:
        raise ValueError(mode)
    return m, outside


def line_pass(v, w, axis, mode, cval):
    """One axis of the definition: v (float32 or float64) -> the same dtype."""
    r = (len(w) - 1) // 2
    n = v.shape[axis]
    i = np.arange(n)
    wide = v.astype(np.float64)
    shape = [1, 1, 1]
    shape[axis] = n

    def tap(k):
        m, outside = tap_index(k, n, mode)
        t = np.take(wide, m, axis=axis)
        if mode == "constant":
            t = np.where(outside.reshape(shape), np.float64(cval), t)
        return t

    t = wide * w[r]
    for j in range(-r, 0):
        t = t + (tap(i + j) + tap(i - j)) * w[j + r]
    return t.astype(v.dtype)


def transcription(v, tables, mode="reflect", cval=0.0):
    """The definition on a [D, H, W] array: tables = [w or None per axis]."""
    out = np.array(v)
    for axis, w in enumerate(tables):
        if w is not None:
            out = line_pass(out, np.asarray(w, dtype=np.float64), axis, mode, cval)
    return out


# ------------------------------------------------------------------ the fixture
def build():
    import scipy
    from scipy import ndimage
    from scipy.ndimage._filters import _gaussian_kernel1d
    arrays = {}
    ins = inputs()
    for s in SHAPES:
        for m in IMAGES:
            if any(c[0] == s and c[1] == m for c in cases()):
                arrays[f"in/{s}/{m}"] = ins[s][m]
    tables = []
    for k, sig in enumerate(SIGMAS):
        tabs = weight_tables(sig)
        for a, w in enumerate(tabs):
            if w is not None:
                r = radius_of(sig[a])
                assert np.array_equal(w, _gaussian_kernel1d(sig[a], 0, r)), (k, a)
                assert np.array_equal(w, w[::-1]), (k, a)        # symmetric bit for bit
                arrays[f"w/{k}/{a}"] = w
        tables.append(tabs)
    total = 0
    for c in cases():
        s, m, k, mode, dt = c
        x = case_input(arrays, c)
        want = ndimage.gaussian_filter(x, SIGMAS[k], mode=mode, cval=CVAL)
        assert want.dtype == x.dtype
        got = transcription(x, tables[k], mode, CVAL)
        view = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
        differing = int((got.view(view) != want.view(view)).sum())
        assert differing == 0, (c, differing)
        total += want.size
        arrays[name(c)] = want
    meta = {"cases": [list(c) for c in cases()], "scipy": scipy.__version__,
            "numpy": np.__version__, "voxels": total, "cval": CVAL, "truncate": TRUNCATE}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    return arrays


if __name__ == "__main__":
    a = build()
    np.savez_compressed(OUT, **a)
    size = os.path.getsize(OUT)
    assert size < 1000000, size
    print(f"{OUT}: {len(a)} arrays, {size} bytes")
