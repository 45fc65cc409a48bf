"""Resampling a case to another voxel grid on the MI355X, and maps back to the scanner's grid.

The reference only warns when a header's spacing is not the network's (preprocess_data.py:
preprocess_case prints a warning beyond 0.1 mm of data.spacing.target); this module puts a case on
the target grid and a probability map back on the native one.  The semantics are those of

    scipy.ndimage.zoom(x, zoom, order=order, mode="nearest", grid_mode=True)

for order 0 (labels and masks: one source voxel, copied) and order 1 (images and maps):

    output index o of an axis with n_in source and n_out output samples reads the source
    coordinate c = (o + 0.5) * (n_in / n_out) - 0.5 in float64, NOT clamped;
    order 0: source index clamp(floor(c + 0.5), 0, n_in - 1);
    order 1: f = floor(c), t = c - f, corners clamp(f, 0, n_in - 1) and clamp(f + 1, 0, n_in - 1);
             the float64 sum over the 8 corners in C order (axis 0 the slowest bit) of
             ((src * w0) * w1) * w2 with w = 1 - t or t, rounded once to float32.

That is scipy's own operation order (with the weights multiplied first, ((w0 * w1) * w2) * src,
about three voxels in ten thousand land one float32 ulp away), so both orders equal scipy bit for bit,
for float32 and float64 sources (tests/golden/resample.npz).  The per-axis coordinates are
evaluated here, in numpy float64, into tables the kernel (csrc/resample.hip, l3u_resample) gathers
through.  Inputs are numpy arrays (uploaded once) or device tensors; there is
no CPU fallback.

Order 3 (resample_spline: images and maps whose small, hot lesions order 1 would blur) is cubic
B-spline interpolation, scipy.ndimage.zoom's own default, by the project's own definition (not a
transcription of scipy's C code, whose boundary initialisation and rounding order differ in the
last bits of float64; the float32 results equal scipy 1.15.3's at every voxel of
tests/golden/spline.npz and the raw float64 sums agree to a few 1e-14 max|x|):

  1. Padding.  NP = 12: the padded volume p[i0, i1, i2] = float64(src[clamp(i0 - 12),
     clamp(i1 - 12), clamp(i2 - 12)]) of shape [D + 24, H + 24, W + 24], np.pad(x, 12, mode="edge").
  2. Prefilter.  Along axis 0, then 1, then 2, every line c of length n of the padded volume is
     filtered in place in float64, every product, sum and difference rounded on its own (no fused
     multiply-add, no reassociation, no scan), with spline_constants() = (z, lam, k0, kn), computed
     in Python floats: z = sqrt(3.0) - 2.0, lam = (1.0 - z) * (1.0 - 1.0 / z), k0 = 1.0 / (1.0 - z),
     kn = z / (z - 1.0):
         c[i] = c[i] * lam                      for all i
         c[0] = c[0] * k0
         c[i] = c[i] + z * c[i-1]               i = 1 .. n-1
         c[n-1] = kn * c[n-1]
         c[i] = z * (c[i+1] - c[i])             i = n-2 .. 0
     The causal start is the closed form for a line extended by its first value; it differs from
     scipy's only inside the outer pad, which nothing reads (the smallest tap index is 10).
  3. Tables (spline_axis_table, numpy float64, per axis and output index o):
     cc = (o + 0.5) * (n_in / n_out) - 0.5, f = floor(cc), y = cc - f, u = 1.0 - y,
     start = int(f) - 1 + 12 (checked to lie in [0, n_in + 20]), w0 = u*u*u/6.0,
     w1 = (y*y*(y-2.0)*3.0+4.0)/6.0, w2 = (u*u*(u-2.0)*3.0+4.0)/6.0, w3 = 1.0 - w0 - w1 - w2.
  4. Interpolation.  out = float32 of the float64 sum, started at 0.0 and accumulated term by term
     over a, b, c in 0..3 in C order (a slowest), of
     ((coef[s0+a, s1+b, s2+c] * w_axis0[a]) * w_axis1[b]) * w_axis2[c]; an optional clip (lo, hi)
     is applied to the float32 result, min(max(v, lo), hi): a spline overshoots, so a probability
     map can leave [0, 1].

With equal shapes the weights are (1/6, 4/6, 1/6, ~0) and the sum undoes the prefilter to within
1e-16 max|x|: the result is the source's float32 bits, as scipy's is, except where a source value
is so small against its neighbourhood (an exact 0 among them) that this noise shows in float32.
The kernels are csrc/spline.hip (l3u_spline_prefilter, l3u_resample_spline).
"""
import math

import numpy as np
import torch

from . import _native as nat

# l3u_resample's dtype codes (l3u_pp_pack's)
_CODE = {torch.float32: 0, torch.float64: 1, torch.uint8: 2}
_ORDER_DTYPES = {0: (torch.uint8, torch.float32, torch.float64), 1: (torch.float32, torch.float64)}


def _device():
    if not torch.cuda.is_available():
        raise nat.NativeError("resampling runs on the ROCm device; no GPU is visible "
                              "(there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _shape3(shape, what):
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"{what} must be three positive sizes [D, H, W], got {shape}")
    return shape


def resampled_shape(shape, spacing, target_spacing):
    """The [D, H, W] shape of a volume of `shape` and `spacing` (one value per array axis, as the
    reference applies header.get_zooms()[:3]) on the `target_spacing` grid:
    max(1, round(n * s_in / s_out)) per axis, Python's round (scipy's).  Host only."""
    shape = _shape3(shape, "shape")
    if len(spacing) != 3 or len(target_spacing) != 3:
        raise ValueError("spacing and target_spacing take one value per array axis")
    if min(spacing) <= 0 or min(target_spacing) <= 0:
        raise ValueError("spacings must be positive")
    return tuple(max(1, int(round(n * float(s) / float(t))))
                 for n, s, t in zip(shape, spacing, target_spacing))


def axis_table(n_in, n_out, order):
    """The coordinates of one axis as defined above: order 0 -> the int32 source index per output
    index; order 1 -> (lo int32, hi int32, t float64)."""
    o = np.arange(n_out, dtype=np.float64)
    c = (o + 0.5) * (n_in / n_out) - 0.5
    if order == 0:
        return np.clip(np.floor(c + 0.5), 0, n_in - 1).astype(np.int32)
    f = np.floor(c)
    return (np.clip(f, 0, n_in - 1).astype(np.int32), np.clip(f + 1, 0, n_in - 1).astype(np.int32),
            c - f)


def _tables(shape, out_shape, order, dev):
    """One upload: the int32 indices (lo, then hi for order 1) of the three axes, then t; returns
    the device buffer and the byte offsets of (lo, hi, t) in it (hi / t None for order 0)."""
    n = sum(out_shape)
    per_axis = [axis_table(a, b, order) for a, b in zip(shape, out_shape)]
    if order == 0:
        buf = np.concatenate(per_axis).view(np.uint8)
        offs = (0, None, None)
    else:
        lo = np.concatenate([p[0] for p in per_axis])
        hi = np.concatenate([p[1] for p in per_axis])
        t = np.concatenate([p[2] for p in per_axis])
        buf = np.concatenate([lo.view(np.uint8), hi.view(np.uint8), t.view(np.uint8)])
        offs = (0, 4 * n, 8 * n)    # t starts on an 8-byte boundary
    return torch.from_numpy(buf).to(dev), offs


def _source(vol, order):
    """(contiguous tensor of a kernel dtype, still where `vol` lives; was_bool)."""
    if isinstance(vol, torch.Tensor):
        t = vol
    else:
        try:
            t = torch.from_numpy(np.ascontiguousarray(vol))
        except TypeError as e:
            raise ValueError(f"resample_volume does not take dtype {np.asarray(vol).dtype}") from e
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"expected a non-empty [D, H, W] volume, got shape {tuple(t.shape)}")
    was_bool = t.dtype == torch.bool
    if was_bool:
        t = t.contiguous().view(torch.uint8)
    if order not in _ORDER_DTYPES:
        raise ValueError("order must be 0 (nearest) or 1 (linear); cubic B-spline "
                         "interpolation (order 3) is resample_spline")
    if t.dtype not in _ORDER_DTYPES[order]:
        raise ValueError(f"order {order} takes " + " / ".join(
            str(d).replace("torch.", "") for d in _ORDER_DTYPES[order])
            + (" / bool" if order == 0 else "") + " volumes, got "
            + ("bool" if was_bool else str(t.dtype).replace("torch.", "")))
    return t.contiguous(), was_bool


def resample_volume(vol, out_shape=None, *, spacing=None, target_spacing=None, order=1,
                    output="numpy"):
    """`vol` [D, H, W] (numpy array or device tensor) on the grid of `out_shape`, or of
    resampled_shape(vol.shape, spacing, target_spacing) when no shape is given (the way back to
    the native grid passes the native shape).  order 1: float32 / float64 in, float32 out.
    order 0: uint8 / bool / float32 / float64 in, the same dtype out.  output="device" keeps the
    result on the device.  Rank and dtype errors are ValueErrors raised before the device is
    touched; without a GPU the call raises NativeError."""
    if output not in ("numpy", "device"):
        raise ValueError("output must be 'numpy' or 'device'")
    src, was_bool = _source(vol, order)
    shape = tuple(int(v) for v in src.shape)
    if out_shape is None:
        if spacing is None or target_spacing is None:
            raise ValueError("resample_volume needs out_shape, or both spacing and target_spacing")
        out_shape = resampled_shape(shape, spacing, target_spacing)
    else:
        out_shape = _shape3(out_shape, "out_shape")
    dev = src.device if src.is_cuda else _device()
    src = src.to(dev)
    dst = torch.empty(out_shape, dtype=torch.float32 if order == 1 else src.dtype, device=dev)
    tab, (lo, hi, t) = _tables(shape, out_shape, order, dev)
    base = tab.data_ptr()
    nat.call("l3u_resample", src.data_ptr(), _CODE[src.dtype], *shape, dst.data_ptr(),
             _CODE[dst.dtype], *out_shape, order, base + lo, None if hi is None else base + hi,
             None if t is None else base + t, nat.stream())
    if was_bool:
        dst = dst.view(torch.bool)
    return dst if output == "device" else dst.cpu().numpy()


# ------------------------------------------------------------------ order 3: cubic B-spline
SPLINE_PAD = 12     # NP: edge voxels per side of the coefficient volume


def spline_constants():
    """(z, lam, k0, kn) of the cubic B-spline prefilter, in Python floats (IEEE doubles)."""
    z = math.sqrt(3.0) - 2.0
    return z, (1.0 - z) * (1.0 - 1.0 / z), 1.0 / (1.0 - z), z / (z - 1.0)


def spline_axis_table(n_in, n_out):
    """One axis of step 3 above: (start int32 [n_out], w float64 [n_out, 4])."""
    o = np.arange(n_out, dtype=np.float64)
    cc = (o + 0.5) * (n_in / n_out) - 0.5
    f = np.floor(cc)
    y = cc - f
    u = 1.0 - y
    w0 = u * u * u / 6.0
    w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0
    w3 = 1.0 - w0 - w1 - w2
    start = f.astype(np.int64) - 1 + SPLINE_PAD
    if start.min() < 0 or start.max() > n_in + 2 * SPLINE_PAD - 4:
        raise ValueError(f"spline taps of {n_in} -> {n_out} samples leave the padded line")
    return start.astype(np.int32), np.stack([w0, w1, w2, w3], axis=1)


def _spline_tables(shape, out_shape):
    """The tables of the three axes as one host buffer, one upload: w [sum(out_shape), 4] float64,
    then start int32; (uint8 tensor, byte offset of start)."""
    per_axis = [spline_axis_table(a, b) for a, b in zip(shape, out_shape)]
    w = np.concatenate([p[1] for p in per_axis])
    start = np.concatenate([p[0] for p in per_axis])
    buf = np.concatenate([w.reshape(-1).view(np.uint8), start.view(np.uint8)])
    return torch.from_numpy(buf), w.nbytes


def _spline_source(vol):
    """`vol` as a contiguous float32 / float64 [D, H, W] tensor, still where it lives."""
    t = vol if isinstance(vol, torch.Tensor) else None
    if t is None:
        a = np.asarray(vol)
        if a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"cubic B-spline resampling takes float32 / float64 volumes, got "
                             f"{a.dtype} (labels and masks stay on order 0)")
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError("cubic B-spline resampling takes float32 / float64 volumes, got "
                         + str(t.dtype).replace("torch.", "") + " (labels and masks stay on order 0)")
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"expected a non-empty [D, H, W] volume, got shape {tuple(t.shape)}")
    return t.contiguous()


def _prefilter(src, dev):
    shape = tuple(int(v) for v in src.shape)
    coef = torch.empty(tuple(n + 2 * SPLINE_PAD for n in shape), dtype=torch.float64, device=dev)
    nat.call("l3u_spline_prefilter", src.data_ptr(), _CODE[src.dtype], *shape, coef.data_ptr(),
             *spline_constants(), nat.stream())
    return coef


def spline_coefficients(vol, output="numpy"):
    """Steps 1 and 2 above: the float64 [D + 24, H + 24, W + 24] B-spline coefficients of `vol`
    [D, H, W] (float32 / float64, numpy array or device tensor).  One prefilter can serve several
    output grids: pass the result (output="device") to resample_spline(coefficients=).  The padded
    float64 volume of a 400 x 400 x 600 case is 0.9 GB."""
    if output not in ("numpy", "device"):
        raise ValueError("output must be 'numpy' or 'device'")
    src = _spline_source(vol)
    dev = src.device if src.is_cuda else _device()
    coef = _prefilter(src.to(dev), dev)
    return coef if output == "device" else coef.cpu().numpy()


def resample_spline(vol, out_shape=None, *, spacing=None, target_spacing=None, clip=None,
                    coefficients=None, output="numpy"):
    """`vol` [D, H, W] (numpy array or device tensor, float32 / float64) on the grid of
    `out_shape`, or of resampled_shape(vol.shape, spacing, target_spacing) when no shape is given,
    by cubic B-spline interpolation as defined in the module's docstring: float32 out.  clip =
    (lo, hi) bounds the float32 result (a spline overshoots).  coefficients = the device tensor
    spline_coefficients(vol, output="device") returned skips the prefilter (`vol` then gives the
    shape alone).  The coefficients are a float64 volume padded by 12 voxels per side, 0.9 GB for
    a 400 x 400 x 600 case, on top of the source and the result.  Every other dtype is a
    ValueError raised before the device is touched, bool and uint8 included: labels stay on
    order 0 (resample_volume).  Without a GPU the call raises NativeError."""
    if output not in ("numpy", "device"):
        raise ValueError("output must be 'numpy' or 'device'")
    src = _spline_source(vol)
    shape = tuple(int(v) for v in src.shape)
    if out_shape is None:
        if spacing is None or target_spacing is None:
            raise ValueError("resample_spline needs out_shape, or both spacing and target_spacing")
        out_shape = resampled_shape(shape, spacing, target_spacing)
    else:
        out_shape = _shape3(out_shape, "out_shape")
    if clip is not None:
        if len(clip) != 2 or not float(clip[0]) <= float(clip[1]):
            raise ValueError("clip must be (lo, hi) with lo <= hi")
    if coefficients is not None:
        want = tuple(n + 2 * SPLINE_PAD for n in shape)
        if not isinstance(coefficients, torch.Tensor) or coefficients.dtype != torch.float64 \
                or tuple(coefficients.shape) != want or not coefficients.is_cuda:
            raise ValueError(f"coefficients must be the float64 {want} device tensor of "
                             "spline_coefficients(vol, output='device')")
    tab, start = _spline_tables(shape, out_shape)
    if coefficients is None:
        dev = src.device if src.is_cuda else _device()
        coefficients = _prefilter(src.to(dev), dev)
    coefficients = coefficients.contiguous()
    dev = coefficients.device
    dst = torch.empty(out_shape, dtype=torch.float32, device=dev)
    tab = tab.to(dev)
    lo, hi = (0.0, 0.0) if clip is None else (float(clip[0]), float(clip[1]))
    nat.call("l3u_resample_spline", coefficients.data_ptr(), *shape, dst.data_ptr(), *out_shape,
             tab.data_ptr() + start, tab.data_ptr(), lo, hi, 0 if clip is None else 1, nat.stream())
    return dst if output == "device" else dst.cpu().numpy()
