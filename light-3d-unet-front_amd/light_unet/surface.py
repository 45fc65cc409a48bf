"""Surface-distance metrics on the MI355X: exact Euclidean distance transform, Hausdorff distance,
its percentile (HD95), average symmetric surface distance (ASSD) and surface Dice at a tolerance
in mm (NSD).

    distance_transform_edt   scipy.ndimage.distance_transform_edt(vol, sampling), bit for bit
    surface_mask             mask & ~binary_erosion(mask, generate_binary_structure(3, 1))
    surface_distances        the four metrics of one (prediction, target) pair
    case_surface_metrics     the same for every threshold of a probability map

The per-voxel work runs in csrc/surface.hip (include/l3u.h: l3u_edt, l3u_surf_mask,
l3u_surf_reduce) on bit-packed masks (preprocess.pack); the percentile's two order statistics come
from the radix selection of csrc/preprocess.hip (l3u_pp_select) over a map that holds the distance
at surface voxels and +inf elsewhere, so no compaction pass is needed.  What stays on the host is
O(1) per pair: np.percentile's interpolation (preprocess.percentile_ranks / percentile_lerp) and
the divisions.  With Sp and St the surfaces of prediction and target:

    d_pt = EDT(~St, spacing)[Sp], d_tp = EDT(~Sp, spacing)[St]
    hd   = max(max d_pt, max d_tp)
    hd95 = max(np.percentile(d_pt, q), np.percentile(d_tp, q))     (the two directed percentiles
           first, then their maximum: MONAI's convention)
    assd = (sum d_pt + sum d_tp) / (|Sp| + |St|)
    nsd  = (#(d_pt <= tol) + #(d_tp <= tol)) / (|Sp| + |St|)       per tolerance
    both surfaces empty: hd = hd95 = assd = 0, nsd = 1; exactly one empty: inf, inf, inf, 0.

The sums are float64 in a fixed order (the same input gives the same bits).  Inputs are numpy
arrays (uploaded once) or device tensors; argument errors are ValueErrors raised before the device
is touched; there is no CPU fallback.
"""
import numpy as np
import torch

from . import _native as nat
from . import preprocess as pp

MAX_TOLERANCES = 8   # csrc/surface.hip kMaxTol
_RES = 11            # l3u_surf_reduce's res: count, max, sum, 8 counts


# ------------------------------------------------------------------ argument checks (host only)
def _shape_of(vol, what):
    shape = tuple(int(v) for v in vol.shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"{what} must be a non-empty [D, H, W] volume, got shape {shape}")
    if shape[0] * shape[1] * shape[2] >= 1 << 31:
        raise ValueError(f"{what} holds {shape[0] * shape[1] * shape[2]} voxels; the surface kernels "
                         "take fewer than 2^31")
    return shape


def _spacing3(spacing, what="spacing"):
    if isinstance(spacing, (int, float, np.integer, np.floating)):
        spacing = (spacing,) * 3
    try:
        sp = tuple(float(s) for s in spacing)
    except TypeError as e:
        raise ValueError(f"{what} takes one value per array axis") from e
    if len(sp) != 3:
        raise ValueError(f"{what} takes one value per array axis, got {len(sp)}")
    if not all(np.isfinite(s) and s > 0 for s in sp):
        raise ValueError(f"{what} must be positive, got {sp}")
    return sp


def _tolerances(tolerances_mm):
    tol = [float(t) for t in tolerances_mm]
    if len(tol) > MAX_TOLERANCES:
        raise ValueError(f"at most {MAX_TOLERANCES} tolerances per call, got {len(tol)}")
    if any(np.isnan(t) for t in tol):
        raise ValueError("tolerances must not be NaN")
    return tol


def _percentile(q):
    q = float(q)
    if not 0.0 <= q <= 100.0:
        raise ValueError("Percentiles must be in the range [0, 100]")
    return q


def _as_tensor(vol, what):
    """`vol` as a torch tensor, still where it lives; ValueError for what torch cannot hold."""
    if isinstance(vol, torch.Tensor):
        return vol
    try:
        return torch.from_numpy(np.ascontiguousarray(vol))
    except TypeError as e:
        raise ValueError(f"{what} has dtype {np.asarray(vol).dtype}, which the device does not take") from e


def _check_pair(pred, target, spacing, tolerances_mm, percentile):
    p, t = _as_tensor(pred, "pred"), _as_tensor(target, "target")
    shape = _shape_of(p, "pred")
    if _shape_of(t, "target") != shape:
        raise ValueError(f"pred and target differ in shape: {shape} and {tuple(t.shape)}")
    return p, t, shape, _spacing3(spacing), _tolerances(tolerances_mm), _percentile(percentile)


# ------------------------------------------------------------------ device helpers
def _device():
    if not torch.cuda.is_available():
        raise nat.NativeError("surface metrics run on the ROCm device; no GPU is visible "
                              "(there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _packable(t, dev):
    """The tensor on the device in a dtype l3u_pp_pack takes, with the same zero voxels."""
    if t.dtype == torch.bool:
        t = t.contiguous().view(torch.uint8)
    elif t.dtype not in pp._PACK_DTYPE:
        t = (t != 0).to(torch.uint8)
    return t.to(dev).contiguous()


def _edt_bits(feat, shape, spacing, passes=7, out=None, tmp=None):
    """l3u_edt over the packed feature mask: the float64 [D, H, W] map."""
    D, H, W = shape
    out = torch.empty(shape, dtype=torch.float64, device=feat.device) if out is None else out
    tmp = torch.empty_like(out) if tmp is None else tmp
    nat.call("l3u_edt", feat.data_ptr(), *spacing, out.data_ptr(), tmp.data_ptr(), D, H, W,
             int(passes), nat.stream())
    return out


def _surface_bits(bits, shape):
    out = torch.empty_like(bits)
    nat.call("l3u_surf_mask", bits.data_ptr(), out.data_ptr(), *shape, nat.stream())
    return out


def _counts(bits_list, shape):
    """Set voxels of each packed mask: one download for all of them."""
    stats = torch.empty((len(bits_list), 7), dtype=torch.int64, device=bits_list[0].device)
    for row, b in zip(stats, bits_list):
        pp._stats_into(row, b, shape)
    return [int(v) for v in stats[:, 0].cpu().tolist()]


def _directed(dist, surf, n_surf, tol, q, shape):
    """The reductions of `dist` over the `n_surf` > 0 voxels of the packed surface and the two
    order statistics of np.percentile(., q), left on the device: (float64 [16], weight g) with
    [0:11] l3u_surf_reduce's res and [11:16] l3u_pp_select's out."""
    dev = dist.device
    n = dist.numel()
    sd = torch.empty_like(dist)
    part = torch.empty(nat.query("l3u_surf_nblocks", n) * 12, dtype=torch.float64, device=dev)
    buf = torch.empty(_RES + 5, dtype=torch.float64, device=dev)
    tol_h = np.ascontiguousarray(tol, dtype=np.float64)
    nat.call("l3u_surf_reduce", dist.data_ptr(), surf.data_ptr(), tol_h.ctypes.data, len(tol),
             sd.data_ptr(), part.data_ptr(), buf.data_ptr(), *shape, nat.stream())
    lo, hi, g = pp.percentile_ranks(n_surf, q)
    ws = torch.empty(nat.query("l3u_pp_select_ws_bytes") // 8, dtype=torch.int64, device=dev)
    nat.call("l3u_pp_select", sd.data_ptr(), 1, n, 2, lo, hi, 0, 0, ws.data_ptr(),
             nat.ptr(buf, _RES), nat.stream())
    return buf, g


def _empty_result(n_pred, n_target, ntol):
    if n_pred == 0 and n_target == 0:
        return {"hd": 0.0, "hd95": 0.0, "assd": 0.0, "nsd": [1.0] * ntol, "n_pred": 0, "n_target": 0}
    inf = float("inf")
    return {"hd": inf, "hd95": inf, "assd": inf, "nsd": [0.0] * ntol, "n_pred": n_pred,
            "n_target": n_target}


def _pair(sp_bits, n_pred, st_bits, n_target, edt_t, shape, spacing, tol, q):
    """One (prediction, target) pair from its packed surfaces; edt_t = EDT(~St) or None."""
    if n_pred == 0 or n_target == 0:
        return _empty_result(n_pred, n_target, len(tol))
    if edt_t is None:
        edt_t = _edt_bits(st_bits, shape, spacing)
    b_pt, g_pt = _directed(edt_t, sp_bits, n_pred, tol, q, shape)
    edt_p = _edt_bits(sp_bits, shape, spacing)
    b_tp, g_tp = _directed(edt_p, st_bits, n_target, tol, q, shape)
    v = torch.cat([b_pt, b_tp]).cpu().tolist()        # the pair's one download
    a, b = v[:_RES + 5], v[_RES + 5:]
    if int(a[0]) != n_pred or int(b[0]) != n_target or a[_RES + 4] != 0.0 or b[_RES + 4] != 0.0:
        raise nat.NativeError("surface reductions disagree with the surface counts")
    total = n_pred + n_target
    return {"hd": max(a[1], b[1]),
            "hd95": max(pp.percentile_lerp(a[_RES], a[_RES + 1], g_pt),
                        pp.percentile_lerp(b[_RES], b[_RES + 1], g_tp)),
            "assd": (a[2] + b[2]) / total,
            "nsd": [(int(a[3 + i]) + int(b[3 + i])) / total for i in range(len(tol))],
            "n_pred": n_pred, "n_target": n_target}


# ------------------------------------------------------------------ public entry points
def distance_transform_edt(vol, sampling=(1, 1, 1), output="numpy"):
    """scipy.ndimage.distance_transform_edt(vol, sampling=sampling): per nonzero voxel the distance
    to the nearest zero voxel, 0 at zero voxels, float64, bit for bit (+inf everywhere when no
    voxel is zero, where scipy's output is meaningless).  `vol`: numpy array or device tensor, any
    dtype preprocess.pack takes, or bool.  output="device" keeps the map on the device."""
    if output not in ("numpy", "device"):
        raise ValueError("output must be 'numpy' or 'device'")
    t = _as_tensor(vol, "vol")
    shape = _shape_of(t, "vol")
    sp = _spacing3(sampling, "sampling")
    src = _packable(t, t.device if t.is_cuda else _device())
    out = _edt_bits(pp.pack(src, "eq", 0.0), shape, sp)
    return out if output == "device" else out.cpu().numpy()


def surface_mask(mask):
    """The packed surface bits (int64 [D, H, ceil(W / 64)], preprocess.unpack reads them) of the
    nonzero voxels of `mask`: mask voxels with a 6-neighbour outside the mask, the outside of the
    volume counting as outside."""
    t = _as_tensor(mask, "mask")
    shape = _shape_of(t, "mask")
    src = _packable(t, t.device if t.is_cuda else _device())
    return _surface_bits(pp.pack(src), shape)


def surface_distances(pred, target, spacing=(4.0, 4.0, 4.0), tolerances_mm=(4.0,), percentile=95.0):
    """{"hd", "hd95", "assd", "nsd": [one per tolerance], "n_pred", "n_target"} of two binary
    volumes (nonzero = foreground; numpy or device), as defined in the module docstring."""
    p, t, shape, sp, tol, q = _check_pair(pred, target, spacing, tolerances_mm, percentile)
    dev = p.device if p.is_cuda else (t.device if t.is_cuda else _device())
    sp_bits = _surface_bits(pp.pack(_packable(p, dev)), shape)
    st_bits = _surface_bits(pp.pack(_packable(t, dev)), shape)
    n_pred, n_target = _counts([sp_bits, st_bits], shape)
    return _pair(sp_bits, n_pred, st_bits, n_target, None, shape, sp, tol, q)


def case_surface_metrics(prob, target, thresholds, spacing=(4.0, 4.0, 4.0), tolerances_mm=(4.0,),
                         percentile=95.0, body_mask=None):
    """[surface_distances(prob (* body_mask) >= t, target >= 0.5, ...) for t in thresholds] of one
    case.  The map is compared in float32 (a float64 map, or a float64 mask, in float64 and against
    the thresholds as given), as lesion.py binarises.  The target's surface and its distance
    transform are computed once; the surface counts of all thresholds come back in one download
    and every threshold with two non-empty surfaces costs one more."""
    p, t, shape, sp, tol, q = _check_pair(prob, target, spacing, tolerances_mm, percentile)
    thr = [float(v) for v in thresholds]
    m = None
    if body_mask is not None:
        m = _as_tensor(body_mask, "body_mask")
        if _shape_of(m, "body_mask") != shape:
            raise ValueError(f"body_mask and prob differ in shape: {tuple(m.shape)} and {shape}")
    if not p.dtype.is_floating_point:
        raise ValueError(f"prob must be a floating-point map, got {p.dtype}")
    if not thr:
        return []
    dev = p.device if p.is_cuda else _device()
    wide = p.dtype == torch.float64 or (m is not None and m.dtype == torch.float64)
    kind = torch.float64 if wide else torch.float32
    pv = p.to(dev).to(kind)
    if m is not None:
        pv = pv * m.to(dev).to(kind)
    tv = t.to(dev)
    tv = tv if tv.dtype.is_floating_point else tv.to(torch.float32)
    st_bits = _surface_bits(pp.pack((tv >= 0.5).to(torch.uint8)), shape)
    sp_bits = [_surface_bits(pp.pack((pv >= (v if wide else float(np.float32(v)))).to(torch.uint8)),
                             shape) for v in thr]
    counts = _counts([st_bits] + sp_bits, shape)
    n_target = counts[0]
    edt_t = _edt_bits(st_bits, shape, sp) if n_target > 0 and any(counts[1:]) else None
    return [_pair(b, n, st_bits, n_target, edt_t, shape, sp, tol, q)
            for b, n in zip(sp_bits, counts[1:])]


# ------------------------------------------------------------------ aggregation over cases
def check_config(surface):
    """The `surface` argument of lesion.sweep_metrics / the config key validation.surface_metrics:
    {"tolerances_mm": [...], "percentile": 95.0} -> (tolerances, percentile)."""
    if not isinstance(surface, dict):
        raise ValueError("surface must be a dict with tolerances_mm and (optionally) percentile")
    unknown = set(surface) - {"tolerances_mm", "percentile"}
    if unknown:
        raise ValueError(f"surface has unknown keys {sorted(unknown)}")
    return _tolerances(surface.get("tolerances_mm", (4.0,))), _percentile(surface.get("percentile", 95.0))


def aggregate(per_case, ntol):
    """The four keys lesion.sweep_metrics adds at one threshold from the cases' dicts: hd95_mean
    and assd_mean over the cases whose two surfaces are both non-empty (nan when there are none),
    nsd_mean per tolerance over the cases where not both are empty, surface_cases the former count."""
    both = [r for r in per_case if r["n_pred"] > 0 and r["n_target"] > 0]
    some = [r for r in per_case if r["n_pred"] > 0 or r["n_target"] > 0]
    nan = float("nan")
    return {"hd95_mean": float(np.mean([r["hd95"] for r in both])) if both else nan,
            "assd_mean": float(np.mean([r["assd"] for r in both])) if both else nan,
            "nsd_mean": [float(np.mean([r["nsd"][i] for r in some])) if some else nan
                         for i in range(ntol)],
            "surface_cases": len(both)}
