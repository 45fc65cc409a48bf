"""Lesion uptake on the MI355X: what a reader of an FDG-PET lymphoma segmentation wants from it.

    lesion_uptake   per lesion: voxels, volume_ml, suv_max, suv_mean, suv_peak, tlg, centroid_mm;
                    per case: n_lesions, tmtv_ml, tlg_total, suv_max, suv_peak, dmax_mm
    check_config    validates {"peak_ml": ..., "dmax": ...} (inference.infer_volume's `quantify`)

Lesions are the components of mask >= threshold with at least min_size voxels, labelled by
lesion.label: 6-connectivity and scipy's numbering, the numbering of extract_bboxes' mask_id.  The
per-voxel and per-pair work runs in csrc/quantify.hip (include/l3u.h, l3u_qt_*):

    suv_peak   the largest mean of the uptake over a sphere of peak_ml millilitres centred on a
               voxel of the lesion (PERCIST's peak: the sphere is clipped to the volume, not to the
               lesion).  r = cbrt(3000 peak_ml / (4 pi)) mm; the sphere is the set O of integer
               offsets with fl(fl((dz sz)^2 + (dy sy)^2) + (dx sx)^2) <= r^2 in C order
               (sphere_offsets, built here in float64 and uploaded as a table); the mean at c is
               the float64 sum of uptake[c + o], from +0.0 and in the order of O, over the offsets
               that stay inside the volume, divided in float64 by their count.
    suv_max    the largest uptake of the lesion; suv_mean its float64 sum over the voxel count;
               tlg = suv_mean * volume_ml.  *_voxel is [z, y, x] of the smallest flat index
               attaining the maximum.
    dmax_mm    sqrt of the largest d2 = fl(fl(fl(dz sz)^2 + fl(dy sy)^2) + fl(dx sx)^2) over pairs
               of voxels of the kept lesions; dmax_voxels the pair with the smallest flat index i,
               then the smallest j > i.  Searched over the mask's corner voxels only (mask voxels
               with, on every axis, a neighbour outside the mask), which is exact.

The sums are float64 in a fixed order and there are no float atomics: the same input gives the
same bits.  Inputs are numpy arrays (uploaded once) or device tensors; argument errors are
ValueErrors raised before the device is touched; there is no CPU fallback.  The uptake must be
finite: results with NaN or infinities are unspecified.
"""
import math

import numpy as np
import torch

from . import _native as nat
from . import lesion
from . import preprocess as pp
from . import smooth as _smooth

MAX_RADIUS_VOXELS = 4     # csrc/quantify.hip kMaxR: the halo the sphere mean stages
MAX_CANDIDATES = 1 << 18  # csrc/quantify.hip kMaxCand
SLAB_VOXELS = 1 << 15     # box voxels per reduction item (a plane of the box at least)
_VALS = 8                 # l3u_qt_reduce's res row: count, sum, max, voxel, peak, voxel, 0, 0


# ------------------------------------------------------------------ argument checks (host only)
def _shape_of(vol, what):
    shape = tuple(int(v) for v in vol.shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"{what} must be a non-empty [D, H, W] volume, got shape {shape}")
    if shape[0] * shape[1] * shape[2] >= 1 << 31:
        raise ValueError(f"{what} holds {shape[0] * shape[1] * shape[2]} voxels; the uptake kernels "
                         "take fewer than 2^31")
    return shape


def _spacing3(spacing):
    try:
        sp = tuple(float(s) for s in spacing)
    except TypeError as e:
        raise ValueError("spacing takes one value per array axis") from e
    if len(sp) != 3:
        raise ValueError(f"spacing takes one value per array axis, got {len(sp)}")
    if not all(np.isfinite(s) and s > 0 for s in sp):
        raise ValueError(f"spacing must be positive, got {sp}")
    return sp


def _peak_ml(peak_ml):
    if peak_ml is None:
        return None
    v = float(peak_ml)
    if not (np.isfinite(v) and v > 0.0):
        raise ValueError(f"peak_ml must be a positive volume in ml (or None), got {peak_ml}")
    return v


def sphere_offsets(spacing, peak_ml=1.0):
    """The offset set O of the peak sphere as int32 [n, 3] rows (dz, dy, dx) in C order, and its
    per-axis reach (rz, ry, rx) in voxels.  A sphere that spans more than 4 voxels from its centre
    on an axis is a ValueError: the spacing is r / 5 or less there and the case should be resampled
    first."""
    sz, sy, sx = (np.float64(s) for s in _spacing3(spacing))
    r = float(np.cbrt(3000.0 * _peak_ml(peak_ml) / (4.0 * np.pi)))
    r2 = r * r
    k = np.arange(-(MAX_RADIUS_VOXELS + 1), MAX_RADIUS_VOXELS + 2, dtype=np.int32)
    dz, dy, dx = np.meshgrid(k, k, k, indexing="ij")
    az, ay, ax = dz.astype(np.float64) * sz, dy.astype(np.float64) * sy, dx.astype(np.float64) * sx
    keep = ((az * az + ay * ay) + ax * ax) <= r2
    offs = np.stack([dz[keep], dy[keep], dx[keep]], axis=1).astype(np.int32)   # C order: dz, dy, dx
    reach = tuple(int(v) for v in np.abs(offs).max(axis=0))
    if max(reach) > MAX_RADIUS_VOXELS:
        axis = int(np.argmax(reach))
        raise ValueError(f"the {peak_ml} ml peak sphere (r = {r:.3f} mm) spans more than "
                         f"{MAX_RADIUS_VOXELS} voxels on axis {axis} at spacing {spacing[axis]} mm "
                         f"(r / {MAX_RADIUS_VOXELS + 1} or less): resample the case first")
    return np.ascontiguousarray(offs), reach


def check_config(cfg):
    """inference.infer_volume's `quantify` argument: {"peak_ml": 1.0 or None, "dmax": True} ->
    (peak_ml, dmax).  None is the defaults."""
    if cfg is None:
        return 1.0, True
    if not isinstance(cfg, dict):
        raise ValueError("quantify must be a dict with peak_ml and / or dmax")
    unknown = set(cfg) - {"peak_ml", "dmax"}
    if unknown:
        raise ValueError(f"quantify has unknown keys {sorted(unknown)}")
    return _peak_ml(cfg.get("peak_ml", 1.0)), bool(cfg.get("dmax", True))


# ------------------------------------------------------------------ device helpers
def _device():
    if not torch.cuda.is_available():
        raise nat.NativeError("lesion uptake runs on the ROCm device; no GPU is visible "
                              "(there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _peak_map(up, labels, offs, reach, shape):
    """l3u_qt_peak: the float64 sphere-mean map, defined at labelled voxels only."""
    dev = up.device
    out = torch.empty(shape, dtype=torch.float64, device=dev)
    offs_d = torch.from_numpy(offs).to(dev)
    nat.call("l3u_qt_peak", up.data_ptr(), labels.data_ptr(), offs_d.data_ptr(), int(offs.shape[0]),
             *reach, out.data_ptr(), *shape, nat.stream())
    return out


def _items(stats):
    """The reduction items of the lesions' bounding boxes: int32 [n, 8] rows (label, z0, z1, y0,
    y1, x0, x1, 0), every box cut into z-slabs of at most SLAB_VOXELS voxels (one plane at least),
    and first[l] = the first item of label l + 1."""
    rows, first = [], [0]
    for i, s in enumerate(stats):
        z0, y0, x0 = (int(v) for v in s[lesion._MIN])
        z1, y1, x1 = (int(v) + 1 for v in s[lesion._MAX])
        step = max(1, SLAB_VOXELS // ((y1 - y0) * (x1 - x0)))
        for z in range(z0, z1, step):
            rows.append((i + 1, z, min(z + step, z1), y0, y1, x0, x1, 0))
        first.append(len(rows))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 8), np.asarray(first, dtype=np.int32)


def _reduce(up, labels, peak, stats, shape):
    """l3u_qt_reduce over every lesion: float64 [num, 8] on the host (one download)."""
    dev = up.device
    items, first = _items(stats)
    part = torch.empty(items.shape[0] * _VALS, dtype=torch.float64, device=dev)
    res = torch.empty((len(stats), _VALS), dtype=torch.float64, device=dev)
    items_d, first_d = torch.from_numpy(items).to(dev), torch.from_numpy(first).to(dev)
    nat.call("l3u_qt_reduce", up.data_ptr(), labels.data_ptr(), nat.ptr(peak), items_d.data_ptr(),
             int(items.shape[0]), first_d.data_ptr(), len(stats), part.data_ptr(), res.data_ptr(),
             *shape, nat.stream())
    return res.cpu().numpy()


def _corner_bits(bits, shape):
    """l3u_qt_corners: (packed corner mask, prefix counts on the device, corner voxels)."""
    nb = nat.query("l3u_qt_corner_blocks", *shape)
    out = torch.empty_like(bits)
    cnt = torch.empty(nb, dtype=torch.int32, device=bits.device)
    pre = torch.empty(nb + 1, dtype=torch.int32, device=bits.device)
    nat.call("l3u_qt_corners", bits.data_ptr(), out.data_ptr(), cnt.data_ptr(), pre.data_ptr(),
             *shape, nat.stream())
    return out, pre, int(pre[nb].item())


def _candidates(corner, pre, n, shape):
    """l3u_qt_compact: int32 [n, 4] rows (z, y, x, flat index), ascending."""
    cand = torch.empty((n, 4), dtype=torch.int32, device=corner.device)
    nat.call("l3u_qt_compact", corner.data_ptr(), pre.data_ptr(), cand.data_ptr(), n, *shape,
             nat.stream())
    return cand


def _farthest(cand, n, spacing):
    """l3u_qt_farthest: float64 [3] on the device (d2, flat i, flat j)."""
    part = torch.empty(nat.query("l3u_qt_pair_parts", n) * 2, dtype=torch.int64, device=cand.device)
    res = torch.empty(3, dtype=torch.float64, device=cand.device)
    nat.call("l3u_qt_farthest", cand.data_ptr(), n, *spacing, part.data_ptr(), res.data_ptr(),
             nat.stream())
    return res


def _dmax(labels, shape, spacing):
    """(dmax_mm, dmax_voxels) over the voxels with a label."""
    corner, pre, n = _corner_bits(pp.pack(labels), shape)
    if n > MAX_CANDIDATES:
        raise ValueError(f"the mask has {n} corner voxels; the farthest-pair search takes at most "
                         f"{MAX_CANDIDATES}")
    if n < 2:   # fewer than two mask voxels: every voxel of a smaller mask is a corner
        return 0.0, None
    d2, i, j = _farthest(_candidates(corner, pre, n, shape), n, spacing).cpu().tolist()
    if not (d2 > 0.0 and 0 <= i < j):
        raise nat.NativeError("the farthest-pair search found no pair among two or more candidates")
    return math.sqrt(d2), [_zyx(int(i), shape), _zyx(int(j), shape)]


def _zyx(flat, shape):
    return [int(v) for v in np.unravel_index(int(flat), shape)]


# ------------------------------------------------------------------ the public entry point
@_smooth.takes_smooth_fwhm
def lesion_uptake(uptake, mask, spacing=(4.0, 4.0, 4.0), threshold=0.5, min_size=0, peak_ml=1.0,
                  dmax=True, resegment=None):
    """The uptake report of one case.

    uptake: [D, H, W] volume (SUV, or whatever unit the caller holds), numpy or device tensor, taken
    as float32 (other dtypes are converted as lesion.label converts its volume).  It must be
    finite: results with NaN or infinities are unspecified.
    mask: a [D, H, W] probability map or binary mask of the same shape, or a lesion.Components
    already on the device (threshold and min_size are not applied again then).  Lesions are the
    components of mask >= threshold with at least min_size voxels.

    Returns {"lesions": [{"label", "voxels", "volume_ml", "suv_max", "suv_max_voxel", "suv_mean",
    "suv_peak", "suv_peak_voxel", "tlg", "centroid_mm"} per lesion in label order], "n_lesions",
    "tmtv_ml", "tlg_total", "suv_max", "suv_peak", "dmax_mm", "dmax_voxels", "dmax_centroid_mm"},
    as the module docstring defines them.  Without a lesion the list is empty and the maxima are
    0.0; with fewer than two mask voxels dmax_mm is 0.0 and dmax_voxels None; dmax_centroid_mm is
    the largest distance between two centroids (0.0 with fewer than two lesions).  peak_ml=None
    leaves the suv_peak keys out, dmax=False the dmax_mm and dmax_voxels keys.

    resegment (default None: nothing changes) = {"method": "fixed" or "relative", "value": ...,
    "grow_mm": ... or None} (resegment.check_resegment) measures the lesions as
    resegment.resegment_lesions redraws them on the uptake, seeded by the lesions above: the report
    is that of its regions, every lesion row gains "seed_label", "seed_voxels" and "threshold", and
    the report "resegment": {"method", "value", "grow_mm", "below_threshold", "absorbed"}, the two
    lists holding the labels of the seeds that left no region.

    Keyword only, added by smooth.takes_smooth_fwhm: smooth_fwhm_mm (default None: nothing
    changes) = the FWHM in mm, a scalar or one value per axis, of a Gaussian post-filter
    (smooth.smooth_fwhm, mode "reflect") applied once, on the device, to the float32 uptake before
    anything reads it: the peak, the reductions and the resegmentation with its relative
    thresholds all see the filtered volume, and the report gains "smooth": {"fwhm_mm",
    "sigma_voxels", "radius"}, one value per axis.  The mask, the seeds and the caller's uptake
    are untouched."""
    sp = _spacing3(spacing)
    peak_ml = _peak_ml(peak_ml)
    rs_cfg = None
    if resegment is not None:
        from . import resegment as _rs
        rs_cfg = _rs.check_resegment(resegment)
    up_t = uptake if isinstance(uptake, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(np.asarray(uptake)))
    shape = _shape_of(up_t, "uptake")
    given = isinstance(mask, lesion.Components)
    if not given and not isinstance(mask, torch.Tensor):
        mask = np.asarray(mask)
    mshape = tuple(int(v) for v in (mask.labels.shape if given else mask.shape))
    if len(mshape) != 3:
        raise ValueError(f"mask must be a [D, H, W] volume, got shape {mshape}")
    if mshape != shape:
        raise ValueError(f"uptake and mask differ in shape: {shape} and {mshape}")
    offs = reach = None
    if peak_ml is not None:
        offs, reach = sphere_offsets(sp, peak_ml)

    dev = mask.labels.device if given else _device()
    up = lesion._volume(up_t, dev)
    comp = mask if given else lesion.label(mask, threshold, min_size)
    rs = None
    if rs_cfg is not None:
        rs = _rs.resegment_lesions(up, comp, sp, method=rs_cfg[0], value=rs_cfg[1], grow_mm=rs_cfg[2])
        comp = rs.components
    voxel_ml = sp[0] * sp[1] * sp[2] / 1000.0
    sp_arr = np.asarray(sp, dtype=np.float64)
    lesions = []
    if comp.num > 0:
        labels = comp.labels.contiguous()
        peak = _peak_map(up, labels, offs, reach, shape) if peak_ml is not None else None
        res = _reduce(up, labels, peak, comp.stats, shape)
        sizes = comp.sizes()
        if not np.array_equal(res[:, 0].astype(np.int64), sizes):
            raise nat.NativeError("uptake reductions disagree with the lesion sizes")
        centers = comp.centers() * sp_arr
        for i in range(comp.num):
            voxels = int(sizes[i])
            volume_ml = float(np.int64(voxels) * voxel_ml)
            suv_mean = float(res[i, 1]) / voxels
            row = {"label": i + 1, "voxels": voxels, "volume_ml": volume_ml,
                   "suv_max": float(res[i, 2]), "suv_max_voxel": _zyx(res[i, 3], shape),
                   "suv_mean": suv_mean}
            if peak_ml is not None:
                row["suv_peak"] = float(res[i, 4])
                row["suv_peak_voxel"] = _zyx(res[i, 5], shape)
            row["tlg"] = suv_mean * volume_ml
            row["centroid_mm"] = [float(v) for v in centers[i]]
            if rs is not None:
                seed = int(rs.seed_label[i])
                row["seed_label"] = seed
                row["seed_voxels"] = int(rs.seed_voxels[seed - 1])
                row["threshold"] = float(rs.thresholds[seed - 1])
            lesions.append(row)
    total = sum(r["voxels"] for r in lesions)
    out = {"lesions": lesions, "n_lesions": len(lesions),
           "tmtv_ml": float(np.int64(total) * voxel_ml),
           "tlg_total": float(sum(r["tlg"] for r in lesions)),
           "suv_max": max((r["suv_max"] for r in lesions), default=0.0)}
    if peak_ml is not None:
        out["suv_peak"] = max((r["suv_peak"] for r in lesions), default=0.0)
    if dmax:
        out["dmax_mm"], out["dmax_voxels"] = (_dmax(comp.labels.contiguous(), shape, sp)
                                              if total >= 2 else (0.0, None))
    out["dmax_centroid_mm"] = centroid_dmax([r["centroid_mm"] for r in lesions])
    if rs is not None:
        out["resegment"] = {"method": rs_cfg[0], "value": rs_cfg[1], "grow_mm": rs_cfg[2],
                            "below_threshold": [int(i) + 1 for i in np.flatnonzero(rs.status == 1)],
                            "absorbed": [int(i) + 1 for i in np.flatnonzero(rs.status == 2)]}
    return out


def centroid_dmax(centroids_mm):
    """The largest distance between two of the centroids, float64 on the host; 0.0 below two."""
    if len(centroids_mm) < 2:
        return 0.0
    c = np.asarray(centroids_mm, dtype=np.float64)
    d = c[:, None, :] - c[None, :, :]
    d = d * d
    return float(np.sqrt((d[..., 0] + d[..., 1]) + d[..., 2]).max())
