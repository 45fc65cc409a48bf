"""Gaussian smoothing on the MI355X: scipy.ndimage.gaussian_filter of a [D, H, W] volume, bit for
bit, and the FWHM post-filter that makes uptake numbers of two scanners comparable.

    gaussian_weights   the float64 weight table of one axis
    gaussian_filter    the filter; numpy or device tensor in, numpy or device tensor out
    fwhm_sigma         a full width at half maximum in mm -> sigma in voxels, per axis
    smooth_fwhm        gaussian_filter by FWHM and spacing (EARL / EQ.PET style harmonisation)

The definition (the project's own; its results equal scipy 1.15.3's bit for bit on
tests/golden/smooth.npz, float32 and float64, all four modes).  For each axis a = 0, 1, 2 in that
order with sigma[a] > 1e-15 (another axis is skipped, not run with a unit kernel):

    weights     on the host in float64: r = int(truncate * sigma + 0.5), or the given radius;
                x = np.arange(-r, r + 1); phi = np.exp(-0.5 / (sigma * sigma) * x ** 2);
                w = phi / phi.sum(); symmetric bit for bit.
    line pass   along a over the current array, every operation float64 and rounded on its own:
                t = v[i] * w[r], then for j = -r, -r + 1, .., -1 in that order
                t = t + (v[i + j] + v[i - j]) * w[j + r]; t is rounded to the array's dtype and
                stored, and the next axis reads the rounded values (the symmetric branch of
                scipy's correlate1d, the outermost pair added first).
    boundary    a tap v[k] outside an axis of length n: `reflect` k mod 2n, then 2n - 1 - k where
                that is >= n; `mirror` k mod (2n - 2), then 2n - 2 - k where >= n, and voxel 0 for
                n == 1; `nearest` k clamped; `constant` the value cval as a float64.  r may exceed
                n many times over.  `wrap` and the `grid-*` modes are not taken.

float32 in gives float32 out, float64 in float64 out; any other dtype is a ValueError (scipy would
round into integers).  Inputs must be finite.  A radius above MAX_RADIUS (64, the halo a workgroup
of csrc/smooth.hip stages; 6.4 voxels of FWHM at truncate 4) is a ValueError.

One launch per filtered axis (include/l3u.h, l3u_gauss_axis), each from one buffer into another:
the source is never modified, and a call takes one extra volume of scratch for one filtered axis
and two for two or three (the result is one of them).  There is no `path=` argument and no fused
single launch: one was built, gave the same bits and measured slower than the three launches
(README), so it was deleted.  Inputs are numpy arrays (uploaded once) or
device tensors; argument errors are ValueErrors raised before the device is touched; there is no
CPU fallback.
"""
import functools
import inspect
import math

import numpy as np
import torch

from . import _native as nat

MODES = {"reflect": 0, "mirror": 1, "nearest": 2, "constant": 3}   # l3u_gauss_axis's codes
MAX_RADIUS = 64          # csrc/smooth.hip kMaxR (l3u_gauss_max_radius)
_SKIP = 1e-15            # scipy's own test: an axis with sigma <= 1e-15 is not filtered


# ------------------------------------------------------------------ argument checks (host only)
def _per_axis(v, what, conv):
    try:
        vals = [conv(v)] * 3 if np.ndim(v) == 0 else [conv(s) for s in v]
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what} takes a scalar or one value per array axis") from e
    if len(vals) != 3:
        raise ValueError(f"{what} takes a scalar or one value per array axis, got {len(vals)}")
    return vals


def _sigmas(sigma):
    s = _per_axis(sigma, "sigma", float)
    if not all(math.isfinite(v) and v >= 0.0 for v in s):
        raise ValueError(f"sigma must be finite and >= 0, got {s}")
    return s


def _radius_of(sigma, truncate, radius):
    if radius is None:
        r = int(truncate * sigma + 0.5)
    else:
        if isinstance(radius, bool) or int(radius) != radius or radius < 0:
            raise ValueError(f"radius must be a non-negative integer, got {radius!r}")
        r = int(radius)
    if r > MAX_RADIUS:
        raise ValueError(f"a radius of {r} voxels is above the {MAX_RADIUS} the kernel stages")
    return r


def _truncate(truncate):
    t = float(truncate)
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError(f"truncate must be positive, got {truncate!r}")
    return t


def gaussian_weights(sigma, truncate=4.0, radius=None):
    """The float64 weight table w[2r + 1] of one axis, as the module docstring defines it."""
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"sigma must be positive, got {sigma!r}")
    r = _radius_of(sigma, _truncate(truncate), radius)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def weight_tables(sigma, truncate=4.0, radius=None):
    """[w or None per axis] for a scalar or per-axis sigma: None where the axis is skipped."""
    s = _sigmas(sigma)
    rad = [None] * 3 if radius is None else _per_axis(radius, "radius", lambda v: v)
    return [gaussian_weights(s[a], truncate, rad[a]) if s[a] > _SKIP else None for a in range(3)]


def _checked(vol, tables, mode, output):
    """(source as a tensor, shape, checked float64 tables); ValueErrors only."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    if output not in ("numpy", "device"):
        raise ValueError('output must be "numpy" or "device"')
    if isinstance(vol, torch.Tensor):
        t = vol
    else:
        a = np.asarray(vol)
        if a.dtype not in (np.float32, np.float64):
            raise ValueError(f"the volume must be float32 or float64, got {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"the volume must be float32 or float64, got {t.dtype}")
    shape = tuple(int(v) for v in t.shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"the volume must be a non-empty [D, H, W] array, got shape {shape}")
    if len(tables) != 3:
        raise ValueError("one weight table (or None) per array axis")
    out = []
    for w in tables:
        if w is not None:
            w = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
            if w.ndim != 1 or w.size % 2 != 1:
                raise ValueError("a weight table holds 2 r + 1 values")
            if (w.size - 1) // 2 > MAX_RADIUS:
                raise ValueError(f"a radius of {(w.size - 1) // 2} voxels is above the {MAX_RADIUS} "
                                 "the kernel stages")
            if not np.array_equal(w, w[::-1]):
                raise ValueError("a weight table must be symmetric")
        out.append(w)
    return t, shape, out


def _device():
    if not torch.cuda.is_available():
        raise nat.NativeError("Gaussian smoothing runs on the ROCm device; no GPU is visible "
                              "(there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _filter_weights(vol, tables, mode="reflect", cval=0.0, output="numpy"):
    """gaussian_filter with the three weight tables given ([w or None per axis], None skips the
    axis) instead of sigmas: what a comparison with another machine's scipy needs, so that it does
    not depend on either machine's np.exp."""
    t, shape, tables = _checked(vol, tables, mode, output)
    cval = float(cval)
    dev = t.device if t.is_cuda else _device()
    cur = t.to(dev).contiguous()          # a host array's upload, or the caller's own tensor
    dtype = 0 if cur.dtype == torch.float32 else 1
    spare = None
    for axis, w in enumerate(tables):
        if w is None:
            continue
        dst = spare if spare is not None else torch.empty(shape, dtype=cur.dtype, device=dev)
        wd = torch.from_numpy(w).to(dev)
        nat.call("l3u_gauss_axis", cur.data_ptr(), dst.data_ptr(), dtype, *shape, axis,
                 wd.data_ptr(), (w.size - 1) // 2, MODES[mode], cval, nat.stream())
        # the buffer just read is the next destination, unless it is the source itself
        spare = cur if cur is not t and cur.data_ptr() != t.data_ptr() else None
        cur = dst
    if cur.data_ptr() == t.data_ptr():    # nothing was filtered: scipy returns a copy
        cur = cur.clone()
    return cur if output == "device" else cur.cpu().numpy()


def gaussian_filter(vol, sigma, mode="reflect", cval=0.0, truncate=4.0, radius=None,
                    output="numpy"):
    """scipy.ndimage.gaussian_filter(vol, sigma, mode=mode, cval=cval, truncate=truncate,
    radius=radius) of a [D, H, W] float32 or float64 volume (numpy or device tensor), bit for bit;
    sigma and radius a scalar or one value per axis.  The source is never modified; the result is
    a new array of the source's dtype, on the host or (output="device") on the device."""
    return _filter_weights(vol, weight_tables(sigma, truncate, radius), mode, cval, output)


def fwhm_sigma(fwhm_mm, spacing):
    """Sigma in voxels per axis of a Gaussian of fwhm_mm (a scalar or one value per axis; 0 skips
    the axis): fwhm_mm / (2.0 * math.sqrt(2.0 * math.log(2.0))) / spacing[a], in float64."""
    f = _per_axis(fwhm_mm, "fwhm_mm", float)
    if not all(math.isfinite(v) and v >= 0.0 for v in f):
        raise ValueError(f"fwhm_mm must be finite and >= 0, got {f}")
    sp = _per_axis(spacing, "spacing", float)
    if np.ndim(spacing) == 0 or not all(math.isfinite(s) and s > 0.0 for s in sp):
        raise ValueError(f"spacing takes one positive value per array axis, got {spacing!r}")
    return tuple(f[a] / (2.0 * math.sqrt(2.0 * math.log(2.0))) / sp[a] for a in range(3))


def smooth_fwhm(vol, spacing, fwhm_mm, **kw):
    """gaussian_filter(vol, fwhm_sigma(fwhm_mm, spacing), **kw)."""
    return gaussian_filter(vol, fwhm_sigma(fwhm_mm, spacing), **kw)


def smooth_record(fwhm_mm, spacing, truncate=4.0):
    """What a report says about its post-filter: {"fwhm_mm", "sigma_voxels", "radius"}, one value
    per axis (radius 0 on a skipped axis).  Raises the ValueErrors of the filter's arguments."""
    sig = fwhm_sigma(fwhm_mm, spacing)
    rad = [_radius_of(s, _truncate(truncate), None) if s > _SKIP else 0 for s in sig]
    return {"fwhm_mm": _per_axis(fwhm_mm, "fwhm_mm", float), "sigma_voxels": list(sig),
            "radius": rad}


def takes_smooth_fwhm(fn):
    """Decorator of a consumer fn(uptake, mask, spacing=..., ...) (quantify.lesion_uptake,
    resegment.resegment_lesions): adds the keyword-only option smooth_fwhm_mm (default None: fn is
    called as it is) in front of it, as a stage of its own, so that fn and its parameter list stay
    what they were.  With a FWHM in mm (a scalar or one value per axis) the uptake is taken as
    float32 on the device, as fn takes it, filtered once (smooth_fwhm, mode "reflect") and handed
    to fn as a device tensor; everything fn reads is the filtered volume, the mask, the seeds and
    the caller's uptake are untouched, and the result gains `smooth` = smooth_record(...): a key
    of a dict, an attribute otherwise.  The filter's arguments are checked before the device is
    touched."""
    params = inspect.signature(fn).parameters

    @functools.wraps(fn)
    def call(uptake, mask, *args, smooth_fwhm_mm=None, **kw):
        if smooth_fwhm_mm is None:
            return fn(uptake, mask, *args, **kw)
        spacing = args[0] if args else kw.get("spacing", params["spacing"].default)
        rec = smooth_record(smooth_fwhm_mm, spacing)
        t = uptake if isinstance(uptake, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(uptake)))
        shape = tuple(int(v) for v in t.shape)
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError(f"uptake must be a non-empty [D, H, W] volume, got shape {shape}")
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        dev = t.device if t.is_cuda else _device()
        up = gaussian_filter(t.to(device=dev, dtype=torch.float32), rec["sigma_voxels"],
                             mode="reflect", output="device")
        out = fn(up, mask, *args, **kw)
        if isinstance(out, dict):
            out["smooth"] = rec
        else:
            out.smooth = rec
        return out
    return call
