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
"""
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
        raise ValueError("order must be 0 (nearest) or 1 (linear)")
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
