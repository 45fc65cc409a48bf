"""Case preprocessing on the MI355X, mirroring the reference's host functions

    clip_and_normalize           scripts/preprocess_data.py:21-59
    calculate_voxel_thresholds   scripts/preprocess_data.py:62-88
    generate_body_mask           scripts/preprocess_data.py:91-174

with the same signatures and results, bit for bit.  The per-voxel work runs in the HIP kernels of
csrc/preprocess.hip (include/l3u.h, l3u_pp_*): exact order statistics for np.percentile (a radix
descent over monotone keys), the fp64 clip + normalise (every operation rounded on its own, as
numpy evaluates it), and the body mask as a bit-packed volume -- 6-neighbour dilation / erosion
iterated in LDS, population count and bounding box with integer atomics.  The largest component
comes from lesion.label (csrc/lesion.hip, scipy's numbering).  What stays on the host is O(1): the
interpolation between two order statistics and the metadata dicts.  Inputs are numpy arrays
(uploaded once) or device tensors; there is no CPU fallback.

binary_closing with iterate_structure(cross, r) is r cross dilations followed by r cross erosions,
both with everything outside the volume reading as 0 (scipy's border_value = 0): the closing eats
voxels within r of a volume face, exactly as the reference's does.
"""
import math

import numpy as np
import torch

from . import _native as nat
from . import lesion
from . import resample

_PACK_DTYPE = {torch.float32: 0, torch.float64: 1, torch.uint8: 2, torch.int32: 3}


def _device():
    if not torch.cuda.is_available():
        raise nat.NativeError("preprocessing runs on the ROCm device; no GPU is visible "
                              "(there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _volume(image, dev):
    """The [D, H, W] image on the device as float64, or float32 when it is float32 (widened
    exactly inside the kernels, which is what get_fdata() does with a float32 NIfTI); any other
    dtype becomes float64 on the host first, as numpy would promote it."""
    if isinstance(image, torch.Tensor):
        t = image if image.dtype in (torch.float32, torch.float64) else image.to(torch.float64)
    else:
        a = np.asarray(image)
        if a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            a = a.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"expected a non-empty [D, H, W] volume, got shape {tuple(t.shape)}")
    return t.to(dev).contiguous()


# ------------------------------------------------------------------ np.percentile
def percentile_ranks(n, q):
    """np.percentile's (method='linear') two order statistics and weight for n values:
    (lo, hi, g) with the virtual index (q / 100) * (n - 1) = lo + g."""
    if not 0.0 <= q <= 100.0:
        raise ValueError("Percentiles must be in the range [0, 100]")
    vi = (q / 100) * (n - 1)
    lo = int(math.floor(vi))
    lo = min(max(lo, 0), n - 1)
    return lo, min(lo + 1, n - 1), vi - lo


def percentile_lerp(a, b, g):
    """numpy's _lerp between the order statistics a <= b (Python floats are IEEE doubles and
    never fuse a multiply with an add)."""
    d = b - a
    return b - d * (1 - g) if g >= 0.5 else a + d * g


def order_statistics(vol, ranks):
    """The values of the flattened device volume (float32 / float64) at the 0-based sorted
    positions `ranks` (1..4 of them) as Python floats, bit-exact; raises ValueError on NaNs."""
    ranks = [int(r) for r in ranks]
    if not 1 <= len(ranks) <= 4:
        raise ValueError("1..4 ranks per selection")
    nat.require_device(vol)
    if vol.dtype not in (torch.float32, torch.float64) or not vol.is_contiguous():
        raise ValueError("order_statistics takes a contiguous float32 / float64 device tensor")
    n = vol.numel()
    if any(not 0 <= r < n for r in ranks):
        raise ValueError(f"ranks must lie in 0..{n - 1}")
    ws = torch.empty(nat.query("l3u_pp_select_ws_bytes") // 8, dtype=torch.int64, device=vol.device)
    out = torch.empty(5, dtype=torch.float64, device=vol.device)
    r4 = ranks + [0] * (4 - len(ranks))
    nat.call("l3u_pp_select", vol.data_ptr(), int(vol.dtype == torch.float64), n, len(ranks),
             *r4, ws.data_ptr(), out.data_ptr(), nat.stream())
    vals = out.cpu().tolist()
    if vals[4] != 0.0:
        raise ValueError(f"the volume holds {int(vals[4])} NaN values")
    return vals[:len(ranks)]


def _clip_values(vol, low_percentile, high_percentile):
    n = vol.numel()
    l0, l1, lg = percentile_ranks(n, low_percentile)
    h0, h1, hg = percentile_ranks(n, high_percentile)
    a0, a1, b0, b1 = order_statistics(vol, [l0, l1, h0, h1])
    return percentile_lerp(a0, a1, lg), percentile_lerp(b0, b1, hg)


def _meta(clip_min, clip_max, low_percentile, high_percentile, target_range):
    return {"clip_values": {"min": float(clip_min), "max": float(clip_max),
                            "low_percentile": low_percentile, "high_percentile": high_percentile},
            "normalization_range": list(target_range)}


def _normalize(vol, clip_min, clip_max, target_range, want64, want32, threshold=None):
    """(float64 or None, float32 or None, packed `float64 value > threshold` or None)."""
    dev = vol.device
    D, H, W = (int(v) for v in vol.shape)
    bits = _new_bits(D, H, W, dev) if threshold is not None else None
    if clip_max > clip_min:
        o64 = torch.empty(vol.shape, dtype=torch.float64, device=dev) if want64 else None
        o32 = torch.empty(vol.shape, dtype=torch.float32, device=dev) if want32 else None
        clip = torch.tensor([clip_min, clip_max], dtype=torch.float64).to(dev)
        scale = target_range[1] - target_range[0]
        nat.call("l3u_pp_normalize", vol.data_ptr(), int(vol.dtype == torch.float64), clip.data_ptr(),
                 float(scale), float(target_range[0]), float(threshold or 0.0), nat.ptr(o64),
                 nat.ptr(o32), nat.ptr(bits), D, H, W, nat.stream())
        return o64, o32, bits
    # np.ones_like(clipped) * target_range[0]
    v = float(1.0 * target_range[0])
    o64 = torch.full(vol.shape, v, dtype=torch.float64, device=dev)
    if bits is not None:
        _pack_into(bits, o64, 1, threshold)
    return (o64 if want64 else None,
            o64.to(torch.float32) if want32 else None, bits)


def clip_and_normalize(image, low_percentile=0.5, high_percentile=99.5, target_range=(0, 1),
                       output="numpy"):
    """preprocess_data.py:21-59: (normalized float64, metadata).  output="device" keeps the
    result on the device."""
    vol = _volume(image, _device())
    clip_min, clip_max = _clip_values(vol, low_percentile, high_percentile)
    o64, _, _ = _normalize(vol, clip_min, clip_max, target_range, True, False)
    return _out(o64, output), _meta(clip_min, clip_max, low_percentile, high_percentile, target_range)


def _out(t, output):
    if output == "device":
        return t
    if output != "numpy":
        raise ValueError("output must be 'numpy' or 'device'")
    return t.cpu().numpy()


# ------------------------------------------------------------------ packed masks
def _new_bits(D, H, W, dev):
    return torch.empty((D, H, (W + 63) // 64), dtype=torch.int64, device=dev)


def _pack_into(bits, src, op, arg):
    D, H, W = (int(v) for v in src.shape)
    nat.call("l3u_pp_pack", src.data_ptr(), _PACK_DTYPE[src.dtype], op, float(arg), bits.data_ptr(),
             D, H, W, nat.stream())


def pack(src, op="nonzero", arg=0.0):
    """Packed mask (int64 [D, H, ceil(W / 64)]) of a contiguous [D, H, W] device tensor (float32,
    float64, uint8 or int32): op "nonzero" (v != 0), "gt" (v > arg) or "eq" (v == arg)."""
    nat.require_device(src)
    if src.dim() != 3 or src.dtype not in _PACK_DTYPE or not src.is_contiguous():
        raise ValueError("pack takes a contiguous [D, H, W] float32 / float64 / uint8 / int32 tensor")
    bits = _new_bits(*(int(v) for v in src.shape), src.device)
    _pack_into(bits, src, {"nonzero": 0, "gt": 1, "eq": 2}[op], arg)
    return bits


def unpack(bits, shape, dtype=torch.uint8):
    """The packed mask as a 0 / 1 device tensor of `shape` (uint8, bool or float32)."""
    D, H, W = (int(v) for v in shape)
    _check_bits(bits, D, H, W)
    kind = torch.uint8 if dtype == torch.bool else dtype
    if kind not in (torch.uint8, torch.float32):
        raise ValueError("unpack gives uint8, bool or float32")
    out = torch.empty((D, H, W), dtype=kind, device=bits.device)
    nat.call("l3u_pp_unpack", bits.data_ptr(), out.data_ptr(), _PACK_DTYPE[kind], D, H, W, nat.stream())
    return out.view(torch.bool) if dtype == torch.bool else out


def _check_bits(bits, D, H, W):
    nat.require_device(bits)
    if bits.dtype != torch.int64 or tuple(bits.shape) != (D, H, (W + 63) // 64) \
            or not bits.is_contiguous():
        raise ValueError(f"expected a packed int64 [{D}, {H}, {(W + 63) // 64}] mask")


def max_morph_iterations(W):
    """Iterations one l3u_pp_morph launch takes for rows of W voxels (its LDS tile's halo)."""
    return nat.query("l3u_pp_morph_max_iters", int(W))


def morph(bits, shape, iterations, erode=False):
    """`iterations` 6-neighbour dilations (or erosions) of the packed mask; outside the volume is
    0.  As many iterations per launch as the LDS tile allows, chained for more."""
    D, H, W = (int(v) for v in shape)
    _check_bits(bits, D, H, W)
    left = int(iterations)
    if left <= 0:
        return bits
    cap = max_morph_iterations(W)
    if cap < 1:
        raise ValueError(f"rows of {W} voxels are wider than the morphology kernel's LDS tile")
    cur, other = bits, torch.empty_like(bits)
    while left > 0:
        it = min(left, cap)
        nat.call("l3u_pp_morph", cur.data_ptr(), other.data_ptr(), int(bool(erode)), it, D, H, W,
                 nat.stream())
        cur, other = other, (torch.empty_like(bits) if cur is bits else cur)
        left -= it
    return cur


def _stats_into(stats_row, bits, shape):
    D, H, W = (int(v) for v in shape)
    nat.call("l3u_pp_mask_stats", bits.data_ptr(), stats_row.data_ptr(), D, H, W, nat.stream())


def mask_stats(bits, shape):
    """(set voxels, bbox min [z, y, x] or None, bbox max [z, y, x] or None) of a packed mask."""
    _check_bits(bits, *(int(v) for v in shape))
    s = torch.empty(7, dtype=torch.int64, device=bits.device)
    _stats_into(s, bits, shape)
    s = s.cpu().tolist()
    if s[0] == 0:
        return 0, None, None
    return s[0], s[1:4], s[4:7]


# ------------------------------------------------------------------ the body mask
def _body_mask_from_bits(bits, shape, body_mask_config, output):
    """preprocess_data.py:122-174 from the packed initial mask on."""
    threshold = body_mask_config.get("threshold", 0.02)
    closing_voxels = body_mask_config.get("closing_voxels", 5)
    keep_largest = body_mask_config.get("keep_largest_component", True)
    dilate_voxels = body_mask_config.get("dilate_voxels", 3)
    dev = bits.device
    stats = torch.empty((4, 7), dtype=torch.int64, device=dev)   # initial, closed, largest, final
    _stats_into(stats[0], bits, shape)
    if closing_voxels > 0:
        bits = morph(morph(bits, shape, closing_voxels), shape, closing_voxels, erode=True)
    _stats_into(stats[1], bits, shape)
    took_largest = False
    if keep_largest:
        comp = lesion.label(unpack(bits, shape, torch.float32), 0.5)
        if comp.num > 0:
            largest = int(np.argmax(comp.sizes())) + 1   # the lowest label among the largest
            bits = pack(comp.labels, "eq", largest)
            took_largest = True
            _stats_into(stats[2], bits, shape)
    if dilate_voxels > 0:
        bits = morph(bits, shape, dilate_voxels)
    _stats_into(stats[3], bits, shape)
    s = stats.cpu().tolist()
    final = s[3]
    if final[0] > 0:
        bbox_min, bbox_max = final[1:4], final[4:7]
    else:
        bbox_min, bbox_max = [0, 0, 0], [int(v) for v in shape]
    meta = {
        "threshold": float(threshold),
        "closing_voxels": int(closing_voxels),
        "keep_largest_component": bool(keep_largest),
        "dilate_voxels": int(dilate_voxels),
        "voxel_counts": {"initial": int(s[0][0]), "after_closing": int(s[1][0]),
                         "after_largest_component": int(s[2][0] if took_largest else s[1][0]),
                         "final": int(final[0])},
        "bbox": {"min": bbox_min, "max": bbox_max},
    }
    return _out(unpack(bits, shape, torch.bool), output), meta


def _initial_bits(normalized_image, threshold, dev):
    """`normalized_image > threshold` as numpy evaluates it: a float64 image compares in float64,
    a float32 image against the threshold rounded to float32."""
    vol = _volume(normalized_image, dev)
    thr = float(np.float32(threshold)) if vol.dtype == torch.float32 else float(threshold)
    return pack(vol, "gt", thr)


def generate_body_mask(normalized_image, body_mask_config, output="numpy"):
    """preprocess_data.py:91-174: (bool mask, mask_metadata).  output="device" gives a torch.bool
    device tensor."""
    dev = _device()
    shape = tuple(int(v) for v in normalized_image.shape)
    bits = _initial_bits(normalized_image, body_mask_config.get("threshold", 0.02), dev)
    return _body_mask_from_bits(bits, shape, body_mask_config, output)


def calculate_voxel_thresholds(spacing, volume_cc_list):
    """preprocess_data.py:62-88 (host only)."""
    voxel_volume_mm3 = spacing[0] * spacing[1] * spacing[2]
    voxel_volume_cc = voxel_volume_mm3 / 1000.0
    thresholds = {}
    for volume_cc in volume_cc_list:
        voxel_count = volume_cc / voxel_volume_cc
        thresholds[f"{volume_cc}cc"] = {
            "volume_cc": volume_cc,
            "voxel_count": int(np.ceil(voxel_count)),
            "formula": f"ceil({volume_cc}cc / {voxel_volume_cc:.6f}cc/voxel)",
        }
    return thresholds


def preprocess_volume(image, config, spacing=None, output="numpy", target_spacing=None,
                      resample_order=None):
    """One case of preprocess_case (preprocess_data.py:243-294) without the file I/O:
    (normalized float32 -- what the reference writes to disk --, body mask or None, metadata with
    clip_values, normalization_range, body_mask when enabled and voxel_thresholds when `spacing`
    is given).  The volume is uploaded once, the initial mask comes out of the normalise launch
    (compared in float64, before the rounding to float32), and only the requested outputs and
    O(1) statistics return to the host.  config: the reference preprocessing config's
    `intensity`, `body_mask` and `volume_threshold` sections.

    `target_spacing` (default None: nothing changes) puts the case on the network's grid first,
    where the reference only warns: with `spacing` (required then, one value per array axis) not
    np.allclose(spacing, target_spacing, atol=0.1), the uploaded image is resampled on the device
    (resample.resample_volume, order 1, to float32) to resample.resampled_shape(...), and the
    percentiles, the normalisation and the body mask run on the resampled volume;
    voxel_thresholds then use the grid's real spacing (target_spacing when resampled, else
    spacing).  metadata["resample"] = {"orig_shape", "orig_spacing", "shape", "spacing",
    "applied"}.  The label is the caller's to resample, to the same shape and with order 0:
    resample_volume(label, metadata["resample"]["shape"], order=0, output="device").
    `resample_order` (default None: order 1, and nothing changes) = 3 resamples the image by cubic
    B-spline interpolation instead (resample.resample_spline), which keeps the peaks of small, hot
    lesions that order 1 flattens; passing it, 1 included, also records it as
    metadata["resample"]["order"]."""
    if target_spacing is not None and spacing is None:
        raise ValueError("target_spacing needs the image's spacing")
    if resample_order not in (None, 1, 3):
        raise ValueError("resample_order must be 1 (linear) or 3 (cubic B-spline)")
    if resample_order is not None and target_spacing is None:
        raise ValueError("resample_order needs target_spacing")
    vol = _volume(image, _device())
    rs_meta = None
    if target_spacing is not None:
        orig_shape = tuple(int(v) for v in vol.shape)
        new_shape = resample.resampled_shape(orig_shape, spacing, target_spacing)
        applied = not np.allclose(spacing, target_spacing, atol=0.1)
        if applied and resample_order == 3:
            vol = resample.resample_spline(vol, new_shape, output="device")
        elif applied:
            vol = resample.resample_volume(vol, new_shape, order=1, output="device")
        rs_meta = {"orig_shape": list(orig_shape), "orig_spacing": [float(s) for s in spacing],
                   "shape": list(new_shape if applied else orig_shape),
                   "spacing": [float(s) for s in (target_spacing if applied else spacing)],
                   "applied": bool(applied)}
        if resample_order is not None:
            rs_meta["order"] = int(resample_order)
        if applied:
            spacing = target_spacing
    inten = config["intensity"]
    low, high = inten["clip_percentile_low"], inten["clip_percentile_high"]
    target_range = inten["normalization_range"]
    bm_cfg = config.get("body_mask", {})
    enabled = bool(bm_cfg.get("enabled", False))
    clip_min, clip_max = _clip_values(vol, low, high)
    _, o32, bits = _normalize(vol, clip_min, clip_max, target_range, False, True,
                              bm_cfg.get("threshold", 0.02) if enabled else None)
    meta = _meta(clip_min, clip_max, low, high, target_range)
    mask = None
    if enabled:
        mask, meta["body_mask"] = _body_mask_from_bits(bits, tuple(vol.shape), bm_cfg, output)
    if spacing is not None:
        vt = config["volume_threshold"]
        meta["voxel_thresholds"] = calculate_voxel_thresholds(
            spacing, [vt["train_cc"], vt["inference_cc"]])
    if rs_meta is not None:
        meta["resample"] = rs_meta
    return _out(o32, output), mask, meta
