"""Lesions resegmented by an uptake threshold on the MI355X: the delineation a PET report's volumes
are defined on, seeded by the network's lesions.

    resegment_lesions   seeds (a mask / probability map, or a lesion.Components) + uptake ->
                        Resegmented: the regions as a lesion.Components and, per seed, its status,
                        threshold, voxel count and the voxels it reached
    check_resegment     validates {"method": ..., "value": ..., "grow_mm": ...}
                        (quantify.lesion_uptake's and inference.infer_volume's `resegment`)

The seeds are the lesions L_1..L_n = lesion.label(mask, threshold, min_size): 6-connectivity and
scipy's numbering, the numbering of extract_bboxes' mask_id.  Per seed i:

    threshold   thr_i = float64(value) for method "fixed" (the "SUV 4.0" volume), and
                float64(value) * float64(m_i) for "relative" (the "41 % SUVmax" volume), m_i the
                float32 maximum of the uptake over L_i; one float64 multiply on the host.
    candidates  cand_i(v) = float64(uptake[v]) >= thr_i, and body_mask[v] != 0 when one is given.
    box         the seed's bounding box grown by ceil(grow_mm / spacing[a]) voxels on both sides of
                axis a and clipped to the volume (grow_mm = 0: the seed's own box).
    region      R_i = the candidates in the box joined to a candidate voxel of L_i by a 6-neighbour
                path of candidates inside the box; connectivity through voxels outside the box does
                not count.  grow_mm = None grows nothing: R_i = the candidates of L_i.
    ownership   label(v) = the smallest i with v in R_i; reached_i = |R_i|, owned_i the voxels
                labelled i.  Status 0 kept (owned_i > 0), 1 below threshold (no candidate in L_i),
                2 absorbed (reached_i > 0, every voxel owned by smaller labels).  The kept seeds
                are renumbered 1..m in seed order; a region may be disconnected once ownership is
                resolved.

The growing runs in csrc/resegment.hip (include/l3u.h, l3u_rs_*): bitmaps of each box in LDS, or,
for a box that does not fit, tiled through a global arena with the host relaunching until a launch
changes nothing.  It is integer and bit work with integer atomics only: the same input gives the
same bits.  Inputs are numpy arrays (uploaded once) or device tensors; argument errors are
ValueErrors raised before the device is touched; there is no CPU fallback.  The uptake must be
finite.
"""
import math

import numpy as np
import torch

from . import _native as nat
from . import lesion
from . import quantify as _qt
from . import smooth as _smooth
from .utils import _checked_body_mask

METHODS = ("fixed", "relative")
MAX_LDS_BYTES = 64 * 1024   # csrc/resegment.hip kLdsMax
_TILE = (8, 8, 4)           # csrc/resegment.hip kTZ, kTY, kTW: rows, rows and words of a tile
_SWEEP_BATCH = 4            # tiled launches between two reads of their counters
STATUS_KEPT, STATUS_BELOW, STATUS_ABSORBED = 0, 1, 2


# ------------------------------------------------------------------ argument checks (host only)
def _method_value(method, value):
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    try:
        v = float(value)
    except (TypeError, ValueError) as e:
        raise ValueError(f"value must be a positive number, got {value!r}") from e
    if not (np.isfinite(v) and v > 0.0):
        raise ValueError(f"value must be a positive number, got {value!r}")
    if method == "relative" and v > 1.0:
        raise ValueError(f"a relative value is a fraction of the seed's maximum in (0, 1], got {value!r}")
    return method, v


def _grow_mm(grow_mm):
    if grow_mm is None:
        return None
    try:
        g = float(grow_mm)
    except (TypeError, ValueError) as e:
        raise ValueError(f"grow_mm must be a distance in mm >= 0 (or None), got {grow_mm!r}") from e
    if not (np.isfinite(g) and g >= 0.0):
        raise ValueError(f"grow_mm must be a distance in mm >= 0 (or None), got {grow_mm!r}")
    return g


def check_resegment(cfg):
    """The `resegment` argument of quantify.lesion_uptake and inference.infer_volume:
    {"method": "fixed" or "relative", "value": ..., "grow_mm": ... or None} -> (method, value,
    grow_mm), with the defaults of resegment_lesions for missing keys.  None is off (-> None)."""
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("resegment must be a dict with method, value and / or grow_mm")
    unknown = set(cfg) - {"method", "value", "grow_mm"}
    if unknown:
        raise ValueError(f"resegment has unknown keys {sorted(unknown)}")
    method, value = _method_value(cfg.get("method", "fixed"), cfg.get("value", 4.0))
    return method, value, _grow_mm(cfg.get("grow_mm", None))


def box_padding(grow_mm, spacing):
    """Voxels the seed's box grows by on both sides of each axis: ceil(grow_mm / spacing[a])."""
    return tuple(int(math.ceil(grow_mm / s)) for s in spacing)


def thresholds_for(method, value, seed_max):
    """thr_i as float64 [n]; seed_max: the float32 maxima of the uptake over the seeds."""
    m = np.asarray(seed_max, dtype=np.float32).astype(np.float64)
    if method == "fixed":
        return np.full(m.shape, np.float64(value), dtype=np.float64)
    return np.float64(value) * m


def seed_boxes(stats, pad, shape):
    """int32 [n, 6] half-open boxes (z0, z1, y0, y1, x0, x1): the seeds' bounding boxes from
    Components.stats grown by pad[a] voxels on both sides and clipped to the volume."""
    out = np.zeros((len(stats), 6), dtype=np.int32)
    for i, s in enumerate(stats):
        lo = [int(v) for v in s[lesion._MIN]]
        hi = [int(v) for v in s[lesion._MAX]]
        for a in range(3):
            out[i, 2 * a] = max(0, lo[a] - pad[a])
            out[i, 2 * a + 1] = min(int(shape[a]), hi[a] + 1 + pad[a])
    return out


def _max_lds(max_lds_bytes):
    v = int(max_lds_bytes)
    if v != 0 and not (16 <= v <= MAX_LDS_BYTES):
        raise ValueError(f"max_lds_bytes must be 0 (the default, {MAX_LDS_BYTES}) or 16..{MAX_LDS_BYTES}, "
                         f"got {max_lds_bytes}")
    return v


class Resegmented:
    """What resegment_lesions returns.  components: a lesion.Components on the device (int32
    labels 1..m, stats as l3u_ccl_stats_b writes them); seed_label int32 [m]: the seed of each
    region; per seed (n of them): status int8 (0 kept, 1 below threshold, 2 absorbed), thresholds
    float64, seed_voxels and reached int64; path int8 (0 LDS, 1 tiled) and sweeps int32 (the
    sweeps, or for tiled seeds the launches, that changed a word) say how the device got there.
    smooth: None, or {"fwhm_mm", "sigma_voxels", "radius"} of the post-filter the uptake went
    through first (resegment_lesions' smooth_fwhm_mm)."""

    def __init__(self, components, seed_label, status, thresholds, seed_voxels, reached, path, sweeps):
        self.components, self.seed_label, self.status = components, seed_label, status
        self.thresholds, self.seed_voxels, self.reached = thresholds, seed_voxels, reached
        self.path, self.sweeps = path, sweeps
        self.smooth = None


def _empty(labels):
    z = np.zeros(0, dtype=np.int64)
    return Resegmented(lesion.Components(labels, 0, np.zeros((0, 12), dtype=np.uint64)),
                       np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int8),
                       np.zeros(0, dtype=np.float64), z, z.copy(), np.zeros(0, dtype=np.int8),
                       np.zeros(0, dtype=np.int32))


# ------------------------------------------------------------------ device helpers
def _plan(boxes, max_lds_bytes):
    """(items int32 [n, 8], tiles int32 [T, 4], aoff int64 [n], arena words)."""
    n = len(boxes)
    items = np.zeros((n, 8), dtype=np.int32)
    items[:, 0] = np.arange(1, n + 1)
    items[:, 1:7] = boxes
    aoff = np.zeros(n, dtype=np.int64)
    tiles, words = [], 0
    for i, (z0, z1, y0, y1, x0, x1) in enumerate(boxes.tolist()):
        nz, ny, nx = z1 - z0, y1 - y0, x1 - x0
        path = nat.query("l3u_rs_path", nz, ny, nx, max_lds_bytes)
        if path not in (0, 1):
            raise nat.NativeError(f"l3u_rs_path refused the box {(nz, ny, nx)} of seed {i + 1}")
        items[i, 7] = path
        if path == 1:
            wpr = (nx + 63) // 64
            aoff[i] = words
            words += 3 * nz * ny * wpr
            mine = [(i, z, y, w) for z in range(0, nz, _TILE[0]) for y in range(0, ny, _TILE[1])
                    for w in range(0, wpr, _TILE[2])]
            if len(mine) != nat.query("l3u_rs_tiles", nz, ny, nx):
                raise nat.NativeError("the tile table disagrees with l3u_rs_tiles")
            tiles += mine
    return items, np.asarray(tiles, dtype=np.int32).reshape(-1, 4), aoff, words


def _grow(up, seeds, body, items, tiles, aoff, words, thr, grow, max_lds_bytes, shape):
    """The native calls: (own: the int32 key map, reached int64 [n], sweeps int32 [n])."""
    dev, st, n, nt = up.device, nat.stream(), len(items), len(tiles)
    own = torch.zeros(shape, dtype=torch.int32, device=dev)
    reached = torch.zeros(n, dtype=torch.int64, device=dev)
    sweeps = torch.zeros(n, dtype=torch.int32, device=dev)
    items_d = torch.from_numpy(items).to(dev)
    thr_d = torch.from_numpy(thr).to(dev)
    tiles_d = torch.from_numpy(tiles).to(dev) if nt else None
    aoff_d = torch.from_numpy(aoff).to(dev) if nt else None
    arena = torch.empty(words, dtype=torch.int64, device=dev) if nt else None
    body_dt = 0 if body is None or body.dtype == torch.float32 else 2
    nat.call("l3u_rs_grow", up.data_ptr(), seeds.data_ptr(), nat.ptr(body), body_dt,
             items_d.data_ptr(), thr_d.data_ptr(), n, int(grow), own.data_ptr(), reached.data_ptr(),
             sweeps.data_ptr(), nat.ptr(tiles_d), nt, nat.ptr(aoff_d), nat.ptr(arena), max_lds_bytes,
             *shape, st)
    launches = 0
    if nt:
        flip, done = 0, not grow
        while not done:
            counters = torch.zeros(_SWEEP_BATCH, dtype=torch.int32, device=dev)
            for j in range(_SWEEP_BATCH):
                nat.call("l3u_rs_sweep", items_d.data_ptr(), n, tiles_d.data_ptr(), nt,
                         aoff_d.data_ptr(), arena.data_ptr(), flip, nat.ptr(counters, j), *shape, st)
                flip ^= 1
            for c in counters.cpu().tolist():   # a launch that changed nothing ends the growing
                if c == 0:
                    done = True
                    break
                launches += 1
        nat.call("l3u_rs_commit", items_d.data_ptr(), n, tiles_d.data_ptr(), nt, aoff_d.data_ptr(),
                 arena.data_ptr(), flip, own.data_ptr(), reached.data_ptr(), *shape, st)
    sw = sweeps.cpu().numpy()
    sw[items[:, 7] == 1] = launches
    return own, reached.cpu().numpy(), sw


def _stats(lab, remap, num, shape):
    """l3u_ccl_stats_b with its remap argument: the labels renumbered in place, uint64 [num, 12]."""
    dev = lab.device
    stats = torch.empty(num * 12, dtype=torch.int64, device=dev)
    rm = torch.from_numpy(remap).to(dev)
    nat.call("l3u_ccl_stats_b", lab.data_ptr(), rm.data_ptr(), None, stats.data_ptr(), num, 1,
             *shape, 0, nat.stream())
    return stats.view(num, 12).cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------ the public entry point
@_smooth.takes_smooth_fwhm
def resegment_lesions(uptake, mask, spacing=(4.0, 4.0, 4.0), method="fixed", value=4.0, grow_mm=None,
                      threshold=0.5, min_size=0, body_mask=None, max_lds_bytes=0):
    """The seeds of `mask` resegmented on `uptake`, as the module docstring defines it.

    uptake: [D, H, W] volume, numpy or device tensor, taken as float32; it must be finite.
    mask: a [D, H, W] probability map or binary mask of the same shape (the seeds are the
    components of mask >= threshold with at least min_size voxels), or a lesion.Components already
    on the device (threshold and min_size are not applied again then).
    method, value: "fixed" (voxels with uptake >= value) or "relative" (>= value x the seed's
    maximum, 0 < value <= 1).  grow_mm: how far the seed's box grows, None for no growth at all.
    body_mask: optional [D, H, W] mask of a dtype the sliding window takes (bool, uint8, int8,
    int16, float32); voxels where it is 0 are no candidates.
    max_lds_bytes: the LDS a seed's two box bitmaps may take before the seed goes the tiled way
    (0: the default and the most, 64 KiB); the result does not depend on it.
    Keyword only, added by smooth.takes_smooth_fwhm: smooth_fwhm_mm (default None: nothing
    changes), the FWHM in mm, a scalar or one value per axis, of a Gaussian post-filter
    (smooth.smooth_fwhm, mode "reflect") applied once, on the device, to the float32 uptake: the
    seed maxima, the thresholds and the growing read the filtered volume; the seeds and the
    caller's uptake are untouched, and the result's `smooth` says what ran.

    Returns a Resegmented.  With no seeds everything is empty and the label map is zeros."""
    sp = _qt._spacing3(spacing)
    method, value = _method_value(method, value)
    grow_mm = _grow_mm(grow_mm)
    max_lds_bytes = _max_lds(max_lds_bytes)
    up_t = uptake if isinstance(uptake, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(np.asarray(uptake)))
    shape = _qt._shape_of(up_t, "uptake")
    given = isinstance(mask, lesion.Components)
    if not given and not isinstance(mask, torch.Tensor):
        mask = np.asarray(mask)
    mshape = tuple(int(v) for v in (mask.labels.shape if given else mask.shape))
    if len(mshape) != 3:
        raise ValueError(f"mask must be a [D, H, W] volume, got shape {mshape}")
    if mshape != shape:
        raise ValueError(f"uptake and mask differ in shape: {shape} and {mshape}")
    if body_mask is not None:
        body_mask = _checked_body_mask(body_mask, shape)
    pad = (0, 0, 0) if grow_mm is None else box_padding(grow_mm, sp)

    dev = mask.labels.device if given else _qt._device()
    up = lesion._volume(up_t, dev)
    comp = mask if given else lesion.label(mask, threshold, min_size)
    n = comp.num
    if n == 0:
        return _empty(torch.zeros(shape, dtype=torch.int32, device=dev))
    seeds = comp.labels.contiguous()
    body = None
    if body_mask is not None:
        body = (body_mask if isinstance(body_mask, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(body_mask))).to(dev).contiguous()
    seed_max = np.zeros(n, dtype=np.float32)
    if method == "relative":
        seed_max = _qt._reduce(up, seeds, None, comp.stats, shape)[:, 2].astype(np.float32)
    thr = thresholds_for(method, value, seed_max)
    items, tiles, aoff, words = _plan(seed_boxes(comp.stats, pad, shape), max_lds_bytes)
    own, reached, sweeps = _grow(up, seeds, body, items, tiles, aoff, words, thr,
                                 grow_mm is not None, max_lds_bytes, shape)

    # own holds n + 1 - label: the first pass maps it back and counts the voxels every seed owns
    back = np.zeros(n + 1, dtype=np.int32)
    back[1:] = np.arange(n, 0, -1, dtype=np.int32)
    stats = _stats(own, back, n, shape)
    owned = stats[:, lesion._SIZE].astype(np.int64)
    reached = reached.astype(np.int64)
    if np.any(owned > reached):
        raise nat.NativeError("a seed owns more voxels than it reached")
    status = np.where(owned > 0, STATUS_KEPT,
                      np.where(reached == 0, STATUS_BELOW, STATUS_ABSORBED)).astype(np.int8)
    keep = owned > 0
    m = int(keep.sum())
    if m < n:
        if m == 0:   # nothing reached: the map is zeros already
            stats = np.zeros((0, 12), dtype=np.uint64)
        else:
            remap = np.zeros(n + 1, dtype=np.int32)
            remap[1:][keep] = np.arange(1, m + 1, dtype=np.int32)
            stats = _stats(own, remap, m, shape)
    return Resegmented(lesion.Components(own, m, stats), (np.flatnonzero(keep) + 1).astype(np.int32),
                       status, thr, comp.sizes(), reached, items[:, 7].astype(np.int8), sweeps)
