"""Golden fixture for the device resampling (light_unet/resample.py, csrc/resample.hip), made by
scipy itself:

    scipy.ndimage.zoom(x, zoom, order=order, mode="nearest", grid_mode=True)

with zoom = out / in per axis, so that scipy's own round(n * zoom) gives the out shape.  Run with
scipy installed (made with 1.15.3):

    python tests/golden/make_resample_goldens.py        # writes tests/golden/resample.npz

Per case `k` the file holds the seeded inputs (default_rng(42): a float32 image U[0, 1) and a uint8
label of blobs; the float64 image is the float32 one widened, which the tests redo) and scipy's
outputs: k/lin32 (order 1 of the float32 image), k/lin64 (order 1 of the float64 image, rounded to
float32), k/near32 (order 0 of the float32 image) and k/near8 (order 0 of the label).  Order 0 of
the float64 image is near32 widened; build() below asserts that instead of storing it.  Case g is
the way back: its inputs are case a's outputs.  `meta` is JSON: shapes, spacings, and how many
voxels of the plain numpy transcription of the module's definition (transcription(), below)
differ from scipy, per case and source type.
"""
import json
import os

import numpy as np

# name: (in shape, out shape, spacing or None); target spacing 4 mm where a spacing is given
CASES = {
    "a": ((13, 17, 23), (6, 11, 19), (2.0, 2.7, 3.3)),
    "b": ((33, 30, 41), (17, 15, 31), (2.0364, 2.0364, 3.0)),
    "c": ((7, 8, 9), (14, 16, 12), None),
    "d": ((20, 9, 31), (25, 9, 19), None),
    "e": ((1, 5, 4), (3, 1, 8), None),
    "f": ((12, 10, 16), (12, 10, 16), None),
    "g": ((6, 11, 19), (13, 17, 23), None),
}
TARGET = (4.0, 4.0, 4.0)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resample.npz")


def blobs(rng, shape):
    """A uint8 label: a few boxes and balls of labels 1..3 over 0."""
    lab = np.zeros(shape, np.uint8)
    grid = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    for i in range(4):
        c = [rng.integers(0, s) for s in shape]
        r = rng.uniform(1.5, max(2.0, 0.3 * max(shape)))
        ball = sum((g - ci) ** 2 for g, ci in zip(grid, c)) <= r * r
        lab[ball] = 1 + i % 3
    return lab


def inputs():
    """{case: (float32 image, uint8 label)} for the cases that do not take another's output."""
    rng = np.random.default_rng(42)
    out = {}
    for k, (shape, _, _) in CASES.items():
        if k != "g":
            out[k] = (rng.random(shape, dtype=np.float32), blobs(rng, shape))
    return out


def scipy_zoom(x, out_shape, order):
    from scipy import ndimage
    zoom = [o / n for o, n in zip(out_shape, x.shape)]
    y = ndimage.zoom(x, zoom, order=order, mode="nearest", grid_mode=True)
    assert y.shape == tuple(out_shape), (y.shape, out_shape)
    return y


def transcription(x, out_shape, order):
    """The module's definition in plain numpy (float64 arithmetic in the stated order).  It equals
    scipy bit for bit, raw float64 sums included; multiplying the weights first,
    ((w0 * w1) * w2) * src, moves about three float32 results in ten thousand by one ulp."""
    idx = []
    for n_in, n_out in zip(x.shape, out_shape):
        c = (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5
        if order == 0:
            idx.append(np.clip(np.floor(c + 0.5), 0, n_in - 1).astype(np.int64))
        else:
            f = np.floor(c)
            idx.append((np.clip(f, 0, n_in - 1).astype(np.int64),
                        np.clip(f + 1, 0, n_in - 1).astype(np.int64), c - f))
    if order == 0:
        return x[np.ix_(*idx)]
    acc = np.zeros(out_shape, np.float64)
    for corner in range(8):
        bits = (corner >> 2 & 1, corner >> 1 & 1, corner & 1)
        w = [ax[2] if b else 1.0 - ax[2] for ax, b in zip(idx, bits)]
        src = x[np.ix_(*[ax[1] if b else ax[0] for ax, b in zip(idx, bits)])].astype(np.float64)
        acc = acc + ((src * w[0][:, None, None]) * w[1][None, :, None]) * w[2][None, None, :]
    return acc.astype(np.float32)


def build():
    """{array name: array} of the whole fixture, `meta` included."""
    arrays, meta = {}, {"target_spacing": list(TARGET), "cases": {}}
    ins = inputs()
    for k, (shape, out_shape, spacing) in CASES.items():
        if k == "g":
            img, lab = arrays["a/lin32"], arrays["a/near8"]
        else:
            img, lab = ins[k]
            arrays[f"{k}/image"], arrays[f"{k}/label"] = img, lab
        assert img.shape == tuple(shape)
        img64 = img.astype(np.float64)
        lin32 = scipy_zoom(img, out_shape, 1)
        lin64 = scipy_zoom(img64, out_shape, 1)
        near32 = scipy_zoom(img, out_shape, 0)
        assert lin32.dtype == np.float32 and lin64.dtype == np.float64
        assert np.array_equal(scipy_zoom(img64, out_shape, 0), near32.astype(np.float64))
        arrays[f"{k}/lin32"] = lin32
        arrays[f"{k}/lin64"] = lin64.astype(np.float32)
        arrays[f"{k}/near32"] = near32
        arrays[f"{k}/near8"] = scipy_zoom(lab, out_shape, 0)
        t32, t64 = transcription(img, out_shape, 1), transcription(img64, out_shape, 1)
        meta["cases"][k] = {
            "shape": list(shape), "out_shape": list(out_shape),
            "spacing": None if spacing is None else list(spacing),
            "transcription_differs_lin32": int((t32 != lin32).sum()),
            "transcription_differs_lin64": int((t64 != arrays[f"{k}/lin64"]).sum()),
            "transcription_differs_near": int((transcription(img, out_shape, 0) != near32).sum()
                                              + (transcription(lab, out_shape, 0)
                                                 != arrays[f"{k}/near8"]).sum()),
            "label_voxels": int((lab > 0).sum()),
        }
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return arrays


if __name__ == "__main__":
    arrays = build()
    np.savez_compressed(OUT, **arrays)
    print(json.dumps(json.loads(bytes(arrays["meta"]).decode()), indent=1))
    print(OUT, os.path.getsize(OUT), "bytes")
