"""Training patches on the MI355X: class-balanced sampling, crop and augmentation of whole case
volumes resident in HBM, mirroring PatchDataset
(light_unet/datasets/patch_dataset.py:17-220).

The reference cuts every patch on the host in a DataLoader worker (numpy crop, scipy rotate /
zoom, numpy noise) and ships it over PCIe.  Here the case volumes are uploaded once, the random
draws stay on the host and are made with the reference's own RNG calls in its order (python
`random` for the flip / rotation axes, numpy's global generator for everything else), and one
launch pair of csrc/augment.hip (l3u_aug_patches) cuts and augments a whole batch from HBM into
the model's [B, 1, pz, py, px] input.  Given the same RNG state, batch element k is the patch the
reference's k-th __getitem__ would return (num_workers = 0 semantics), with scipy's float64
interpolation restated in the kernels (tests/test_patches_gpu.py).

draws="device" is a second draw mode: the same decisions with the same probabilities, made on
the device by the counter-based generator of include/l3u.h ("Training-patch draws on the device",
csrc/augdraw.hip l3u_aug_draw) from (draw_seed, a device step counter, item index).  A batch is
then l3u_aug_draw -> l3u_aug_patches -> l3u_counter_add on persistent buffers: no host RNG call,
no upload, no allocation and no host sync, and DevicePatchLoader replays that chain as one
hipGraph.  It is a third patch stream (neither the reference's 16-worker stream nor the
num_workers = 0 one): the same distribution, different samples.  restate_draws() restates the
generator in pure Python, so which patch a given (seed, step, item) was can be reproduced
without a GPU.

locate="device" moves _sample_locations (patch_dataset.py:74-100) off the host's voxels: the
reference's randint calls are made on voxel counts from l3u_loc_count and the drawn rows come
from l3u_loc_select (csrc/locate.hip), the same lists as the host pass with ==.
"""
import ctypes
import math
import random

import numpy as np
import torch

from . import _native as nat
from .engine import _splitmix64, stream_seed


class AugDraw:
    """One patch's augmentation, as PatchDataset._augment draws it (patch_dataset.py:156-220)."""
    __slots__ = ("flip_axis", "angle", "rot_axes", "scale", "shift", "noise")

    def __init__(self):
        self.flip_axis, self.angle, self.rot_axes = -1, 0.0, None
        self.scale = self.shift = self.noise = None


def draw_augmentation(aug, patch):
    """The reference's RNG calls of _augment, in order; returns the drawn AugDraw."""
    d = AugDraw()
    if not aug:
        return d
    f = aug.get("random_flip", {})
    if f.get("enabled", False) and np.random.rand() < f.get("prob", 0.5):
        d.flip_axis = int(random.choice(f.get("axes", [0, 1, 2])))
    r = aug.get("random_rotation", {})
    if r.get("enabled", False) and np.random.rand() < r.get("prob", 0.5):
        lo, hi = r.get("angle_range", [-15, 15])
        d.angle = float(np.random.uniform(lo, hi))
        d.rot_axes = tuple(random.choice(r.get("axes", [[0, 1], [0, 2], [1, 2]])))
    s = aug.get("random_scale", {})
    if s.get("enabled", False) and np.random.rand() < s.get("prob", 0.3):
        lo, hi = s.get("scale_range", [0.9, 1.1])
        d.scale = float(np.random.uniform(lo, hi))
    sh = aug.get("intensity_shift", {})
    if sh.get("enabled", False) and np.random.rand() < sh.get("prob", 0.5):
        lo, hi = sh.get("shift_range", [-0.1, 0.1])
        d.shift = float(np.random.uniform(lo, hi))
    g = aug.get("gaussian_noise", {})
    if g.get("enabled", False) and np.random.rand() < g.get("prob", 0.3):
        d.noise = np.random.normal(0, g.get("sigma", 0.01), tuple(patch))
    return d


def _cosdg_sindg(angle):
    """scipy.ndimage.rotate's rotation constants, `special.cosdg(angle), special.sindg(angle)`
    (the cephes degree functions, the reference's own dependency).  Without scipy: exact at
    multiples of 90 degrees, np.cos / np.sin of the radians otherwise (may differ in the last
    ulp)."""
    try:
        from scipy import special
    except ImportError:
        special = None
    if special is not None:
        return float(special.cosdg(angle)), float(special.sindg(angle))
    if angle % 90 == 0:
        k = int(angle // 90) % 4
        return [1.0, 0.0, -1.0, 0.0][k], [0.0, 1.0, 0.0, -1.0][k]
    rad = np.deg2rad(angle)
    return float(np.cos(rad)), float(np.sin(rad))


def aug_param(img_t, lab_t, center, patch, d):
    """The l3u_aug_param record of one patch (crop: patch_dataset.py:136-154; rotate / zoom
    constants computed in float64 exactly as scipy.ndimage.rotate / zoom compute them)."""
    p = nat.AugParam()
    p.image, p.label = img_t.data_ptr(), lab_t.data_ptr()
    sd, sh, sw = img_t.shape
    pz, py, px = patch
    z, y, x = (int(v) for v in center)
    p.z0, p.y0, p.x0 = max(0, z - pz // 2), max(0, y - py // 2), max(0, x - px // 2)
    p.sd, p.sh, p.sw = sd, sh, sw
    p.pz, p.py, p.px = pz, py, px
    p.flip = d.flip_axis
    if d.rot_axes is not None:
        a0, a1 = sorted(int(a) for a in d.rot_axes)
        c, s = _cosdg_sindg(d.angle)
        ic = (np.array([patch[a0], patch[a1]], np.float64) - 1) / 2
        oc = np.array([[c, s], [-s, c]]) @ ic
        off = ic - oc
        p.rot_a0, p.rot_a1 = a0, a1
        p.rot_c, p.rot_s, p.rot_off0, p.rot_off1 = c, s, float(off[0]), float(off[1])
    else:
        p.rot_a0 = p.rot_a1 = -1
    if d.scale is not None:
        zs = [int(round(n * d.scale)) for n in patch]
        p.zoom = 1
        for k in range(3):
            p.zs[k] = zs[k]
            p.zst[k] = (zs[k] - patch[k]) // 2 if zs[k] > patch[k] else 0
            p.zf[k] = (patch[k] - 1) / (zs[k] - 1) if zs[k] != 1 else 1.0
    p.shift_on = 1 if d.shift is not None else 0
    p.shift = d.shift if d.shift is not None else 0.0
    p.noise_on = 1 if d.noise is not None else 0
    return p


# ---------------------------------------------------------------- device draws, restated in Python
# The generator of include/l3u.h ("Training-patch draws on the device"), with Python ints and
# floats only.  Slot numbers: L3U_DRAW_*.
_M64 = (1 << 64) - 1
(SLOT_DOMAIN, SLOT_TABLE, SLOT_LOCATION, SLOT_FLIP_ON, SLOT_FLIP_AXIS, SLOT_ROT_ON, SLOT_ROT_ANGLE,
 SLOT_ROT_PLANE, SLOT_SCALE_ON, SLOT_SCALE, SLOT_SHIFT_ON, SLOT_SHIFT, SLOT_NOISE_ON, SLOT_NOISE_U1,
 SLOT_NOISE_U2) = range(15)
_TWO_PI = 6.283185307179586
DRAW_MODES = ("host", "device")


def draw_key(seed, step, item):
    """key(seed, step, item) = S(seed ^ S(uint32(step) << 32 | uint32(item)))."""
    return _splitmix64((int(seed) & _M64) ^
                       _splitmix64(((int(step) & 0xFFFFFFFF) << 32) | (int(item) & 0xFFFFFFFF)))


def draw_bits(key, slot, v=0):
    """h(slot, v) = S(key ^ S(v << 8 | slot)): the 64 random bits of one draw."""
    return _splitmix64(key ^ _splitmix64(((int(v) << 8) | int(slot)) & _M64))


def _unit(h):
    return (h >> 11) * 2.0 ** -53          # [0, 1), exact


def _choice(h, n):
    return (h * int(n)) >> 64              # the high 64 bits of the 128-bit product


def _range(lo, hi, u):
    return float(lo) + (float(hi) - float(lo)) * u   # three float64 roundings, as numpy's uniform


def aug_settings(aug):
    """The augmentation config as draw_augmentation reads it (same keys and defaults), flattened:
    {flip|rot|scale|shift|noise: (enabled, prob, ...)}."""
    aug = aug or {}
    f, r = aug.get("random_flip", {}), aug.get("random_rotation", {})
    s, sh, g = aug.get("random_scale", {}), aug.get("intensity_shift", {}), aug.get("gaussian_noise", {})
    return {
        "flip": (bool(f.get("enabled", False)), float(f.get("prob", 0.5)),
                 [int(a) for a in f.get("axes", [0, 1, 2])]),
        "rot": (bool(r.get("enabled", False)), float(r.get("prob", 0.5)),
                [float(v) for v in r.get("angle_range", [-15, 15])],
                [(int(p[0]), int(p[1])) for p in r.get("axes", [[0, 1], [0, 2], [1, 2]])]),
        "scale": (bool(s.get("enabled", False)), float(s.get("prob", 0.3)),
                  [float(v) for v in s.get("scale_range", [0.9, 1.1])]),
        "shift": (bool(sh.get("enabled", False)), float(sh.get("prob", 0.5)),
                  [float(v) for v in sh.get("shift_range", [-0.1, 0.1])]),
        "noise": (bool(g.get("enabled", False)), float(g.get("prob", 0.3)),
                  float(g.get("sigma", 0.01))),
    }


class DrawSpec:
    """One dataset as the draws see it: its location lists [(case, (z, y, x)), ...] (lesion,
    background), lesion_patch_ratio and augmentation config."""

    def __init__(self, lesion, background, lesion_patch_ratio=0.5, augmentation=None):
        self.lesion = [(int(c), tuple(int(v) for v in zyx)) for c, zyx in lesion]
        self.background = [(int(c), tuple(int(v) for v in zyx)) for c, zyx in background]
        self.lesion_patch_ratio = float(lesion_patch_ratio)
        self.settings = aug_settings(augmentation)

    def __len__(self):
        return len(self.lesion) + len(self.background)


class DrawRecord:
    """struct l3u_aug_draw_rec: what was drawn for one item (no derived constants)."""
    FIELDS = ("domain", "case_idx", "table", "loc", "cz", "cy", "cx", "flip_on", "flip_axis",
              "rot_on", "rot_a0", "rot_a1", "scale_on", "shift_on", "noise_on", "step", "angle",
              "scale", "shift")
    __slots__ = FIELDS

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw[k])

    def astuple(self):
        return tuple(getattr(self, k) for k in self.FIELDS)

    def __eq__(self, other):
        return isinstance(other, DrawRecord) and self.astuple() == other.astuple()

    def __repr__(self):
        return "DrawRecord(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.FIELDS) + ")"

    @property
    def center(self):
        return (self.cz, self.cy, self.cx)

    def aug_draw(self, noise=None):
        """The AugDraw of this record (noise: the item's float64 array when noise_on)."""
        d = AugDraw()
        d.flip_axis = self.flip_axis if self.flip_on else -1
        if self.rot_on:
            d.angle, d.rot_axes = self.angle, (self.rot_a0, self.rot_a1)
        d.scale = self.scale if self.scale_on else None
        d.shift = self.shift if self.shift_on else None
        d.noise = noise if self.noise_on else None
        return d


def restate_draws(seed, step, B, specs, fl_ratio=None):
    """The DrawRecords l3u_aug_draw writes for a batch of B items at (seed, step), computed from
    the definition in include/l3u.h with Python ints and floats (no GPU, no numpy RNG).
    specs: one DrawSpec, or the pair (FL, DLBCL) with fl_ratio for the mixed dataset."""
    if isinstance(specs, DrawSpec):
        specs = [specs]
    specs = list(specs)
    if len(specs) not in (1, 2) or (len(specs) == 2) != (fl_ratio is not None):
        raise ValueError("specs: one DrawSpec, or two with fl_ratio")
    if sum(len(s) for s in specs) == 0 or (len(specs) == 1 and len(specs[0]) == 0):
        raise ValueError("no locations to draw from")
    out = []
    for b in range(int(B)):
        key = draw_key(seed, step, b)

        def u(slot):
            return _unit(draw_bits(key, slot))
        dom = 0
        if len(specs) == 2:
            if u(SLOT_DOMAIN) < fl_ratio and len(specs[0]) > 0:
                dom = 0
            elif len(specs[1]) > 0:
                dom = 1
        sp = specs[dom]
        if u(SLOT_TABLE) < sp.lesion_patch_ratio and len(sp.lesion) > 0:
            table = 0
        elif len(sp.background) > 0:
            table = 1
        else:
            table = 0
        rows = sp.background if table else sp.lesion
        loc = _choice(draw_bits(key, SLOT_LOCATION), len(rows))
        case_idx, (cz, cy, cx) = rows[loc]
        st = sp.settings
        r = dict(domain=dom, case_idx=case_idx, table=table, loc=loc, cz=cz, cy=cy, cx=cx,
                 step=int(step), flip_axis=-1, rot_a0=-1, rot_a1=-1, angle=0.0, scale=0.0, shift=0.0)
        on, prob, axes = st["flip"]
        r["flip_on"] = int(on and u(SLOT_FLIP_ON) < prob)
        if r["flip_on"]:
            r["flip_axis"] = axes[_choice(draw_bits(key, SLOT_FLIP_AXIS), len(axes))]
        on, prob, (lo, hi), planes = st["rot"]
        r["rot_on"] = int(on and u(SLOT_ROT_ON) < prob)
        if r["rot_on"]:
            r["angle"] = _range(lo, hi, u(SLOT_ROT_ANGLE))
            r["rot_a0"], r["rot_a1"] = planes[_choice(draw_bits(key, SLOT_ROT_PLANE), len(planes))]
        on, prob, (lo, hi) = st["scale"]
        r["scale_on"] = int(on and u(SLOT_SCALE_ON) < prob)
        if r["scale_on"]:
            r["scale"] = _range(lo, hi, u(SLOT_SCALE))
        on, prob, (lo, hi) = st["shift"]
        r["shift_on"] = int(on and u(SLOT_SHIFT_ON) < prob)
        if r["shift_on"]:
            r["shift"] = _range(lo, hi, u(SLOT_SHIFT))
        on, prob, _ = st["noise"]
        r["noise_on"] = int(on and u(SLOT_NOISE_ON) < prob)
        out.append(DrawRecord(**r))
    return out


def restate_noise(seed, step, item, nvox, sigma):
    """The item's Box-Muller noise values [nvox] (z-major voxel order) as l3u_aug_draw defines
    them; libm's log / cos may differ from the device's in the last ulps."""
    key = draw_key(seed, step, item)
    out = []
    for v in range(int(nvox)):
        u1 = ((draw_bits(key, SLOT_NOISE_U1, v) >> 11) + 1) * 2.0 ** -53      # (0, 1]
        u2 = _unit(draw_bits(key, SLOT_NOISE_U2, v))
        out.append(float(sigma) * (math.sqrt(-2.0 * math.log(u1)) * math.cos(_TWO_PI * u2)))
    return out


def _check_mode(draws):
    if draws not in DRAW_MODES:
        raise ValueError(f"draws must be one of {DRAW_MODES}, got {draws!r}")
    return draws


# ---------------------------------------------------------------- patch locations on the device
# PatchDataset._sample_locations (patch_dataset.py:74-100) without its host pass over the voxels:
# row k of np.argwhere(m) is the k-th set voxel of m in C order, so the rows the reference keeps
# are rank queries (csrc/locate.hip: l3u_loc_count / l3u_loc_select).
LOCATE_MODES = ("host", "device")
_LOC_DTYPES = {torch.float32: 0, torch.float64: 1}
_NP_OF = {torch.float32: np.float32, torch.float64: np.float64, torch.bool: np.bool_}


def _check_locate(locate):
    if locate not in LOCATE_MODES:
        raise ValueError(f"locate must be one of {LOCATE_MODES}, got {locate!r}")
    return locate


def _loc_inputs(vols, body_masks):
    """[(label, body or None)]: contiguous device tensors, float32 / float64 labels and one-byte
    masks of the label's shape.  vols: label volumes, or (image, label) pairs."""
    labels = [v[1] if isinstance(v, (tuple, list)) else v for v in vols]
    if body_masks is None:
        body_masks = [None] * len(labels)
    if len(body_masks) != len(labels):
        raise ValueError("one body mask (or None) per case")
    out = []
    for lab, body in zip(labels, body_masks):
        if not torch.is_tensor(lab) or not lab.is_cuda or lab.dtype not in _LOC_DTYPES:
            raise nat.NativeError("locations on the device need float32 / float64 ROCm device "
                                  "labels; there is no CPU fallback")
        if lab.ndim != 3 or lab.numel() == 0 or lab.numel() >= 2 ** 31:
            raise ValueError("a label must be a 3D volume of 1 .. 2^31 - 1 voxels")
        if body is not None:
            if not torch.is_tensor(body) or body.device != lab.device or \
                    body.dtype not in (torch.bool, torch.uint8):
                raise nat.NativeError("a body mask must be a torch.bool / uint8 tensor on the "
                                      "label's device")
            if body.shape != lab.shape:
                raise ValueError("a body mask must have its label's shape")
            body = body.contiguous()
        out.append((lab.contiguous(), body))
    return out


def _loc_count_launch(inputs):
    """l3u_loc_count of every case on the current stream, no sync: (one int32 workspace holding
    every case's uint32 prefix [2][nblocks + 1], the cases' offsets into it, their block counts)."""
    nbs = [nat.query("l3u_loc_nblocks", lab.numel()) for lab, _ in inputs]
    offs = [0]
    for nb in nbs:
        offs.append(offs[-1] + 2 * (nb + 1))
    dev = inputs[0][0].device if inputs else None
    ws = torch.empty(max(offs[-1], 1), dtype=torch.int32, device=dev)
    s = nat.stream()
    for (lab, body), off in zip(inputs, offs):
        nat.call("l3u_loc_count", lab.data_ptr(), _LOC_DTYPES[lab.dtype], nat.ptr(body),
                 lab.numel(), nat.ptr(ws, off), s)
    return ws, offs, nbs


def _loc_totals(ws, offs, nbs):
    """int64 [ncases, 2] (lesion, background) voxel counts: ONE read-back for all cases."""
    if not nbs:
        return np.zeros((0, 2), np.int64)
    idx = [o + c * (nb + 1) + nb for o, nb in zip(offs, nbs) for c in (0, 1)]
    return torch.stack([ws[i] for i in idx]).cpu().numpy().astype(np.int64).reshape(-1, 2)


def location_counts(vols, body_masks=None):
    """The number of lesion voxels (label > 0) and of background voxels (label == 0, inside the
    body mask where one is given) of every case: int64 [ncases, 2].  vols: device label volumes
    (float32 / float64; or (image, label) pairs), body_masks: per case None or a torch.bool /
    uint8 device tensor.  The counts of all cases are launched without a sync in between and
    read back once."""
    return _loc_totals(*_loc_count_launch(_loc_inputs(vols, body_masks)))


def draw_location_ranks(counts, rng=np.random):
    """_sample_locations' random draws (patch_dataset.py:83-98) from the per-case voxel counts
    [(n_lesion, n_background)]: per case rng.randint(n_les, size=max(10, n_les // 1000)) only if
    n_les > 0, then rng.randint(n_bg, size=max(10, n_bg // 5000)) only if n_bg > 0 -- the
    reference's calls in the reference's order, so the generator ends in the reference's state.
    Returns per case (lesion ranks, background ranks): indices into np.argwhere's rows, i.e.
    0-based C-order ranks among the class's voxels (empty int64 arrays where nothing is drawn).
    No GPU use."""
    out = []
    for n_les, n_bg in counts:
        n_les, n_bg = int(n_les), int(n_bg)
        les = bg = np.zeros(0, np.int64)
        if n_les > 0:
            les = np.asarray(rng.randint(n_les, size=max(10, n_les // 1000)), np.int64)
        if n_bg > 0:
            bg = np.asarray(rng.randint(n_bg, size=max(10, n_bg // 5000)), np.int64)
        out.append((les, bg))
    return out


def sample_locations_device(vols, body_masks=None, rng=np.random):
    """_sample_locations (patch_dataset.py:74-100) on device-resident cases: counts (one
    read-back) -> draw_location_ranks on the host -> one upload of all ranks -> the select
    launches.  Returns two int32 [n, 4] device tables of (case index, z, y, x) rows, lesion and
    background, in the reference's row order (per case, in draw order): the rows the reference's
    lists hold, given the same generator state.  Arguments as location_counts."""
    inputs = _loc_inputs(vols, body_masks)
    ws, offs, nbs = _loc_count_launch(inputs)
    ranks = draw_location_ranks(_loc_totals(ws, offs, nbs), rng)
    dev = inputs[0][0].device if inputs else torch.device("cuda", torch.cuda.current_device())
    flat = np.concatenate([r for pair in ranks for r in pair] + [np.zeros(1, np.int64)])
    ranks_t = torch.from_numpy(flat).to(dev)
    tabs = [torch.empty(max(sum(len(p[c]) for p in ranks), 1), 4, dtype=torch.int32, device=dev)
            for c in (0, 1)]
    s = nat.stream()
    at, row = 0, [0, 0]
    for ci, ((lab, body), off, pair) in enumerate(zip(inputs, offs, ranks)):
        for c in (0, 1):
            R = len(pair[c])
            nat.call("l3u_loc_select", lab.data_ptr(), _LOC_DTYPES[lab.dtype], nat.ptr(body),
                     *lab.shape, nat.ptr(ws, off), c, nat.ptr(ranks_t, at), R, ci,
                     nat.ptr(tabs[c], 4 * row[c]), s)
            at += R
            row[c] += R
    return tabs[0][:row[0]], tabs[1][:row[1]]


def _rows_to_locations(rows):
    """An int [n, 4] table as the reference's list [(case index, np.int64 [z, y, x])]."""
    return [(int(r[0]), np.array(r[1:], np.int64)) for r in np.asarray(rows)]


def bind_sample_locations(PatchDataset):
    """Replace PatchDataset._sample_locations (patch_dataset.py:74-100) with the device form.
    Each case's label and body mask are read exactly as the reference reads them
    (`nib.load(case["label_path"]).get_fdata()` through the nibabel module PatchDataset's own
    module imported, and self._load_body_mask_array(case)), uploaded with the label as float64
    (so the predicate is the reference's), and the rows are selected on the device with the
    reference's randint calls: the same two lists, the same numpy generator state afterwards.
    All labels of the dataset are in HBM at once (8 bytes per voxel) until the method returns.
    The original stays reachable as PatchDataset._l3u_reference_sample_locations."""
    import sys
    mod = sys.modules[PatchDataset.__module__]
    if not hasattr(PatchDataset, "_l3u_reference_sample_locations"):
        PatchDataset._l3u_reference_sample_locations = PatchDataset._sample_locations

    def _sample_locations(self):
        if not torch.cuda.is_available():
            raise nat.NativeError("device locations need the ROCm device (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
        labels, bodies = [], []
        for case in self.cases:
            label = np.asarray(mod.nib.load(case["label_path"]).get_fdata(), np.float64)
            body = self._load_body_mask_array(case)
            labels.append(torch.from_numpy(np.ascontiguousarray(label)).to(dev))
            bodies.append(None if body is None else
                          torch.from_numpy(np.ascontiguousarray(np.asarray(body).astype(bool))).to(dev))
        les, bg = sample_locations_device(labels, bodies)
        both = torch.cat([les, bg]).cpu().numpy()
        return _rows_to_locations(both[:len(les)]), _rows_to_locations(both[len(les):])
    PatchDataset._sample_locations = _sample_locations
    return _sample_locations


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _cfg_struct(spec):
    """struct l3u_aug_cfg of a DrawSpec."""
    st, c = spec.settings, nat.AugCfg()
    c.lesion_ratio = spec.lesion_patch_ratio
    c.flip_on, c.flip_prob, axes = st["flip"]
    c.rot_on, c.rot_prob, (c.rot_lo, c.rot_hi), planes = st["rot"]
    c.scale_on, c.scale_prob, (c.scale_lo, c.scale_hi) = st["scale"]
    c.shift_on, c.shift_prob, (c.shift_lo, c.shift_hi) = st["shift"]
    c.noise_on, c.noise_prob, c.noise_sigma = st["noise"]
    if c.flip_on and not (1 <= len(axes) <= nat.DRAW_MAX_AXES and all(0 <= a <= 2 for a in axes)):
        raise ValueError(f"random_flip axes {axes}: 1..{nat.DRAW_MAX_AXES} axes out of 0, 1, 2")
    if c.rot_on and not (1 <= len(planes) <= nat.DRAW_MAX_AXES and
                         all(0 <= a <= 2 and 0 <= b <= 2 and a != b for a, b in planes)):
        raise ValueError(f"random_rotation axes {planes}: 1..{nat.DRAW_MAX_AXES} pairs of 0, 1, 2")
    c.flip_naxes = len(axes) if c.flip_on else 0
    c.rot_nplanes = len(planes) if c.rot_on else 0
    for k in range(c.flip_naxes):
        c.flip_axes[k] = axes[k]
    for k in range(c.rot_nplanes):
        c.rot_planes[k][0], c.rot_planes[k][1] = planes[k]
    return c


class _DeviceDraws:
    """draws="device" state of one DevicePatchDataset (or the two of a DeviceMixedPatchDataset):
    the device tables, the step and count counters and the persistent per-batch-size buffers,
    and the launch chain l3u_aug_draw -> l3u_aug_patches -> l3u_counter_add."""

    def __init__(self, datasets, fl_ratio, seed):
        self.datasets = list(datasets)
        self.fl_ratio = fl_ratio
        self.dev, self.patch = self.datasets[0].dev, self.datasets[0].patch_size
        if any(d.patch_size != self.patch for d in self.datasets):
            raise ValueError("the two datasets must share one patch size")
        self.specs = [d.draw_spec() for d in self.datasets]
        if sum(len(s) for s in self.specs) == 0:
            raise ValueError("no locations to draw from")
        self.seed = stream_seed(int(seed) & _M64, _rank())
        self._keep = []                        # the device tables the structs point into
        self.tables = (nat.AugTables * len(self.datasets))()
        self.cfgs = (nat.AugCfg * len(self.datasets))()
        for k, (ds, sp) in enumerate(zip(self.datasets, self.specs)):
            self.cfgs[k] = _cfg_struct(sp)
            cases = (nat.AugCase * max(len(ds.vols), 1))()
            for i, (img, lab) in enumerate(ds.vols):
                cases[i].image, cases[i].label = img.data_ptr(), lab.data_ptr()
                cases[i].sd, cases[i].sh, cases[i].sw = img.shape
            ct = torch.frombuffer(bytearray(cases), dtype=torch.uint8).to(self.dev)
            if getattr(ds, "location_tables", None) is not None:
                # selected on the device from the case volumes themselves: in range by
                # construction, already in HBM (an empty table still needs a valid pointer)
                tabs = [t if len(t) else torch.zeros(4, dtype=torch.int32, device=self.dev)
                        for t in ds.location_tables]
            else:
                tabs = [self._rows(ds, rows) for rows in (sp.lesion, sp.background)]
            self._keep += [ct] + tabs
            t = self.tables[k]
            t.cases, t.lesion, t.background = ct.data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr()
            t.n_lesion, t.n_background = len(sp.lesion), len(sp.background)
        self.step_t = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.counts_t = torch.zeros(2, dtype=torch.int32, device=self.dev)
        self._bufs, self._graphs, self.last_B = {}, {}, 0

    def _rows(self, ds, rows):
        """int32 (case, z, y, x) rows on the device; every row is checked against its volume here,
        once, because the kernels index with them unchecked."""
        a = np.array([(c, *zyx) for c, zyx in rows], np.int64).reshape(-1, 4)
        for c, z, y, x in a:
            if not (0 <= c < len(ds.vols)) or not all(0 <= v < s for v, s in
                                                     zip((z, y, x), ds.vols[c][0].shape)):
                raise ValueError(f"location {(c, z, y, x)} lies outside its case volume")
        if len(a) == 0:                        # a valid pointer for an empty table
            return torch.zeros(4, dtype=torch.int32, device=self.dev)
        return torch.from_numpy(a.astype(np.int32)).to(self.dev)

    def buffers(self, B, cut=True):
        pz, py, px = self.patch
        P = pz * py * px
        if B not in self._bufs:
            self._bufs[B] = {
                "recs": torch.zeros(B * ctypes.sizeof(nat.AugDrawRec), dtype=torch.uint8, device=self.dev),
                "prm": torch.zeros(B * ctypes.sizeof(nat.AugParam), dtype=torch.uint8, device=self.dev),
                "noise": torch.zeros(B, P, dtype=torch.float64, device=self.dev)}
        buf = self._bufs[B]
        if cut and "out" not in buf:
            buf["tmp"] = torch.empty(2, B, P, dtype=torch.float32, device=self.dev)
            buf["out"] = torch.empty(2, B, 1, pz, py, px, dtype=torch.float32, device=self.dev)
        return buf

    def launch(self, B, cut=True):
        """One batch on the current stream (capturable once buffers(B) exists): the draws, the
        patches (cut=False: draws only) and the counter advance."""
        buf = self.buffers(B, cut)
        pz, py, px = self.patch
        s = nat.stream()
        nat.call("l3u_aug_draw", self.tables, self.cfgs, len(self.datasets),
                 float(self.fl_ratio or 0.0), self.seed, self.step_t.data_ptr(), B, pz, py, px,
                 buf["recs"].data_ptr(), buf["prm"].data_ptr(), buf["noise"].data_ptr(),
                 self.counts_t.data_ptr(), s)
        if cut:
            nat.call("l3u_aug_patches", buf["prm"].data_ptr(), B, pz, py, px, buf["noise"].data_ptr(),
                     buf["tmp"][0].data_ptr(), buf["tmp"][1].data_ptr(), buf["out"][0].data_ptr(),
                     buf["out"][1].data_ptr(), s)
        nat.call("l3u_counter_add", self.step_t.data_ptr(), 1, s)
        self.last_B = B
        return (buf["out"][0], buf["out"][1]) if cut else None

    def replay(self, B):
        """The same batch as launch(B), replayed from a hipGraph captured on first use (a linear
        chain of five kernel nodes).  The warm-up run leaves no trace on the counters."""
        g = self._graphs.get(B)
        if g is None:
            self.buffers(B)
            saved = (self.step_t.clone(), self.counts_t.clone())
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self.launch(B)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.step_t.copy_(saved[0])
            self.counts_t.copy_(saved[1])
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self.launch(B)
            self._graphs[B] = g
        g.replay()
        self.last_B = B
        buf = self._bufs[B]
        return buf["out"][0], buf["out"][1]

    # ---- read-backs (each one synchronises; none is on the per-batch path)
    def records(self):
        """The DrawRecords of the last batch, read back from the device."""
        if not self.last_B:
            return []
        raw = self._bufs[self.last_B]["recs"].cpu().numpy().tobytes()
        arr = (nat.AugDrawRec * self.last_B).from_buffer_copy(raw)
        return [DrawRecord(**{k: getattr(r, k) for k in DrawRecord.FIELDS}) for r in arr]

    def params(self):
        """The l3u_aug_param records of the last batch (nat.AugParam array)."""
        raw = self._bufs[self.last_B]["prm"].cpu().numpy().tobytes()
        return (nat.AugParam * self.last_B).from_buffer_copy(raw)

    def noise(self):
        """The last batch's noise buffer [B, pz, py, px] float64 (rows of noise-off items are
        stale)."""
        return self._bufs[self.last_B]["noise"].cpu().numpy().reshape(self.last_B, *self.patch)

    def last_draws(self):
        recs = self.records()
        nz = self.noise() if any(r.noise_on for r in recs) else None
        return [(r.case_idx, r.center, r.aug_draw(nz[k] if r.noise_on else None))
                for k, r in enumerate(recs)]

    def state(self):
        return self.seed, int(self.step_t.item())

    def set_state(self, state):
        seed, step = state
        seed = int(seed) & _M64
        if seed != self.seed:                  # the seed is a kernel argument of the captured chain
            self._graphs.clear()
        self.seed = seed
        self.step_t.fill_(int(step))

    def take_counts(self):
        """The per-domain item counts accumulated on the device since the last call (zeroed)."""
        c = self.counts_t.cpu().tolist()
        self.counts_t.zero_()
        return c


class DevicePatchDataset:
    """PatchDataset (patch_dataset.py:17-154) over case volumes resident on the device.

    cases: list of (image, label[, body_mask]) numpy volumes (the NIfTI contents the reference
    loads per item).  Seeding, location sampling (_sample_locations, :74-100) and the per-item
    draws follow the reference; sample_batch(B) returns device tensors [B, 1, *patch_size].
    from_reference() takes a constructed reference PatchDataset instead: its sampled locations
    are kept as they are and each case is read once.

    draws="device": the per-item draws are made on the device (l3u_aug_draw) from draw_seed
    (default: `seed`; mixed with the data-parallel rank by engine.stream_seed) and a device step
    counter; the locations above become device tables once, here.  sample_batch(B) then launches
    draw -> cut on persistent buffers and returns THOSE buffers (valid until the next batch of the
    same size; copy what must outlive it), last_draws reads the device records back when
    accessed, and draw_state() / set_draw_state() expose (seed, step) for a resumed run.

    locate="device": _sample_locations runs on the device (sample_locations_device: the
    reference's randint calls on voxel counts, the rows by rank-select, no np.argwhere).  The
    cases may then be numpy arrays or device tensors, the optional third element a numpy bool /
    uint8 mask or a torch.bool / uint8 device tensor -- what preprocess_volume(output="device")
    returns; labels are tested in the float32 the dataset holds.  The device tables stay on
    `location_tables` (draws="device" uses them as they are); lesion_locations /
    background_locations are the same rows read back once.  Same lists and the same numpy
    generator state as locate="host"."""

    def __init__(self, cases, patch_size=(48, 48, 48), lesion_patch_ratio=0.5, augmentation=None,
                 seed=42, device=None, locations=None, draws="host", draw_seed=None, locate="host"):
        self.draws = _check_mode(draws)
        self.locate = _check_locate(locate)
        self.location_tables = None
        if not torch.cuda.is_available():
            raise nat.NativeError("DevicePatchDataset needs the ROCm device (no CPU fallback)")
        self.dev = device or torch.device("cuda", torch.cuda.current_device())
        self.patch_size = tuple(int(v) for v in patch_size)
        self.lesion_patch_ratio = lesion_patch_ratio
        self.augmentation = augmentation
        if locations is None:
            random.seed(seed)
            np.random.seed(seed)
        self.vols = []
        if self.locate == "device":
            locations = self._upload_and_locate(cases, locations)
        else:
            for case in cases:
                img, lab = np.asarray(case[0], np.float32), np.asarray(case[1], np.float32)
                if img.shape != lab.shape or img.ndim != 3:
                    raise ValueError("image and label must be matching 3D volumes")
                self.vols.append((torch.from_numpy(np.ascontiguousarray(img)).to(self.dev),
                                  torch.from_numpy(np.ascontiguousarray(lab)).to(self.dev)))
            if locations is None:
                locations = self._sample_locations(cases)
        self.lesion_locations, self.background_locations = locations
        self.seed = seed
        self._last_draws = []
        self._dd = None
        if self.draws == "device":
            self._dd = _DeviceDraws([self], None, seed if draw_seed is None else draw_seed)

    @property
    def last_draws(self):
        """[(case index, centre, AugDraw)] of the last batch (device draws: read back on access)."""
        return self._dd.last_draws() if self._dd is not None else self._last_draws

    @last_draws.setter
    def last_draws(self, v):
        self._last_draws = v

    def draw_spec(self):
        return DrawSpec(self.lesion_locations, self.background_locations, self.lesion_patch_ratio,
                        self.augmentation)

    def _device_draws(self):
        if self._dd is None:
            raise ValueError('this dataset draws on the host (construct it with draws="device")')
        return self._dd

    def draw_state(self):
        """(seed, step) of the device draw stream: the next batch is drawn at `step`."""
        return self._device_draws().state()

    def set_draw_state(self, state):
        self._device_draws().set_state(state)

    @property
    def last_records(self):
        """The raw DrawRecords of the last batch (device draws)."""
        return self._device_draws().records()

    @classmethod
    def from_reference(cls, ds, read=None, device=None, draws="host", draw_seed=None):
        """The device twin of a constructed reference PatchDataset `ds`: the same cases,
        locations (ds.lesion_locations / background_locations, drawn by its __init__), patch
        size, lesion ratio and augmentation config.  Each case is read ONCE with
        read(path) -> float32 volume (default: `nib.load(path).get_fdata().astype(np.float32)`
        through the nibabel module the reference module imported, patch_dataset.py:129-130)
        and stays in HBM.  Consumes no random numbers.  draws / draw_seed as the constructor's
        (draw_seed defaults to the reference dataset's seed)."""
        _check_mode(draws)
        if read is None:
            import sys
            nib = sys.modules[type(ds).__module__].nib

            def read(path):
                return nib.load(path).get_fdata().astype(np.float32)
        cases = [(read(c["image_path"]), read(c["label_path"])) for c in ds.cases]
        return cls(cases, ds.patch_size, ds.lesion_patch_ratio, ds.augmentation,
                   seed=getattr(ds, "seed", 42), device=device,
                   locations=(list(ds.lesion_locations), list(ds.background_locations)),
                   draws=draws, draw_seed=draw_seed)

    def _to_dev(self, a, dtype):
        if torch.is_tensor(a):
            return a.to(device=self.dev, dtype=dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=_NP_OF[dtype]))).to(self.dev)

    def _upload_and_locate(self, cases, locations):
        """locate="device": the cases (numpy arrays or device tensors, float32 in HBM) and, unless
        `locations` is given, their locations by sample_locations_device over the float32 labels:
        the device tables stay on `location_tables`, the lists are the same rows read back once."""
        bodies = []
        for case in cases:
            img, lab = self._to_dev(case[0], torch.float32), self._to_dev(case[1], torch.float32)
            if img.shape != lab.shape or img.ndim != 3:
                raise ValueError("image and label must be matching 3D volumes")
            body = case[2] if len(case) > 2 else None
            if body is not None:
                if torch.is_tensor(body) and body.dtype == torch.uint8:
                    body = body.to(self.dev).contiguous()
                else:                          # numpy: .astype(bool), as _load_body_mask_array
                    body = self._to_dev(body, torch.bool)
            self.vols.append((img, lab))
            bodies.append(body)
        if locations is not None:
            return locations
        les, bg = sample_locations_device([lab for _, lab in self.vols], bodies)
        self.location_tables = (les, bg)
        both = torch.cat([les, bg]).cpu().numpy()
        return _rows_to_locations(both[:len(les)]), _rows_to_locations(both[len(les):])

    @staticmethod
    def _sample_locations(cases):
        lesion, bg = [], []
        for ci, case in enumerate(cases):
            lab = np.asarray(case[1])
            body = np.asarray(case[2]).astype(bool) if len(case) > 2 and case[2] is not None else None
            lc = np.argwhere(lab > 0)
            if len(lc) > 0:
                for i in np.random.randint(len(lc), size=max(10, len(lc) // 1000)):
                    lesion.append((ci, lc[i]))
            bc = np.argwhere((lab == 0) & body) if body is not None else np.argwhere(lab == 0)
            if len(bc) > 0:
                for i in np.random.randint(len(bc), size=max(10, len(bc) // 5000)):
                    bg.append((ci, bc[i]))
        return lesion, bg

    def __len__(self):
        return len(self.lesion_locations) + len(self.background_locations)

    def _draw_location(self):
        """__getitem__'s location draw (patch_dataset.py:115-124)."""
        if np.random.rand() < self.lesion_patch_ratio and len(self.lesion_locations) > 0:
            return self.lesion_locations[np.random.randint(len(self.lesion_locations))]
        if len(self.background_locations) > 0:
            return self.background_locations[np.random.randint(len(self.background_locations))]
        return self.lesion_locations[np.random.randint(len(self.lesion_locations))]

    def draw_item(self):
        """One __getitem__'s random draws (location, then _augment's), in the reference's order:
        ((case index, centre, AugDraw), its l3u_aug_param record)."""
        case_idx, center = self._draw_location()
        d = draw_augmentation(self.augmentation, self.patch_size)
        img_t, lab_t = self.vols[case_idx]
        return (case_idx, tuple(int(v) for v in center), d), aug_param(img_t, lab_t, center,
                                                                      self.patch_size, d)

    def sample_batch(self, B):
        """B consecutive __getitem__ draws, cut and augmented on the device in one launch pair
        (device draws: B items of the next step, drawn on the device too)."""
        if self._dd is not None:
            return self._dd.launch(B)
        items = [self.draw_item() for _ in range(B)]
        self.last_draws = [i[0] for i in items]
        return cut_patches(items, self.patch_size, self.dev)

    def replay_batch(self, B):
        """sample_batch(B) of the device draws as one hipGraph replay (captured on first use)."""
        return self._device_draws().replay(B)

    def draw_records(self, B):
        """One step of the device draw stream WITHOUT cutting patches: the B DrawRecords."""
        self._device_draws().launch(B, cut=False)
        return self._dd.records()


def cut_patches(items, patch, dev):
    """One l3u_aug_patches launch pair over [(draw, AugParam)] (the records may point into
    different datasets' volumes): device tensors images, labels [B, 1, *patch]."""
    B = len(items)
    arr = (nat.AugParam * B)(*[p for _, p in items])
    prm = torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(dev)
    pz, py, px = patch
    P = pz * py * px
    noise = None
    if any(d.noise is not None for (_, _, d), _ in items):
        nz = np.zeros((B, P), np.float64)
        for k, ((_, _, d), _) in enumerate(items):
            if d.noise is not None:
                nz[k] = d.noise.reshape(-1)
        noise = torch.from_numpy(nz).to(dev)
    tmp = torch.empty(2, B, P, dtype=torch.float32, device=dev)
    out = torch.empty(2, B, 1, pz, py, px, dtype=torch.float32, device=dev)
    nat.call("l3u_aug_patches", prm.data_ptr(), B, pz, py, px,
             noise.data_ptr() if noise is not None else None, tmp[0].data_ptr(),
             tmp[1].data_ptr(), out[0].data_ptr(), out[1].data_ptr(), nat.stream())
    return out[0], out[1]


class DeviceMixedPatchDataset:
    """MixedPatchDataset (patch_dataset.py:223-268) over two DevicePatchDatasets: per item,
    np.random.rand() < fl_ratio picks the FL stream (else DLBCL), the reference's (unused) index
    draw np.random.randint(len(sub)) is made, then the sub-dataset's __getitem__ draws.  The
    per-domain sample counts are kept on `counts` (the reference MixedPatchDataset object when
    built by from_reference, so Trainer.train_epoch reads them there, trainer.py:210-256)."""

    def __init__(self, fl, dlbcl, fl_ratio=0.5, counts=None, draws="host", draw_seed=None):
        self.draws = _check_mode(draws)
        self.fl, self.dlbcl, self.fl_ratio = fl, dlbcl, fl_ratio
        self.patch_size, self.dev = fl.patch_size, fl.dev
        self.counts = counts if counts is not None else self
        self._dd = None
        if counts is None:
            self.reset_sample_counts()
        self._last_draws = []
        if self.draws == "device":
            self._dd = _DeviceDraws([fl, dlbcl], float(fl_ratio),
                                    fl.seed if draw_seed is None else draw_seed)

    @classmethod
    def from_reference(cls, ds, read=None, device=None, draws="host", draw_seed=None):
        _check_mode(draws)
        return cls(DevicePatchDataset.from_reference(ds.fl_dataset, read, device),
                   DevicePatchDataset.from_reference(ds.dlbcl_dataset, read, device),
                   ds.fl_ratio, counts=ds, draws=draws, draw_seed=draw_seed)

    @property
    def last_draws(self):
        """[(case index in its domain's dataset, centre, AugDraw)] of the last batch."""
        return self._dd.last_draws() if self._dd is not None else self._last_draws

    @last_draws.setter
    def last_draws(self, v):
        self._last_draws = v

    def _device_draws(self):
        if self._dd is None:
            raise ValueError('this dataset draws on the host (construct it with draws="device")')
        return self._dd

    def draw_state(self):
        return self._device_draws().state()

    def set_draw_state(self, state):
        self._device_draws().set_state(state)

    @property
    def last_records(self):
        return self._device_draws().records()

    def flush_counts(self):
        """Device draws: move the item counts accumulated on the device onto `counts` (one
        device read; DevicePatchLoader calls it once per epoch, after the last batch)."""
        if self._dd is not None:
            fl, dl = self._dd.take_counts()
            self.counts.fl_sample_count += fl
            self.counts.dlbcl_sample_count += dl

    def reset_sample_counts(self):
        self.fl_sample_count = 0
        self.dlbcl_sample_count = 0
        if self._dd is not None:
            self._dd.counts_t.zero_()

    def get_sample_counts(self):
        self.flush_counts()
        c = self.counts
        return {"fl_samples": c.fl_sample_count, "dlbcl_samples": c.dlbcl_sample_count,
                "total_samples": c.fl_sample_count + c.dlbcl_sample_count}

    def __len__(self):
        return len(self.fl) + len(self.dlbcl)

    def draw_item(self):
        if np.random.rand() < self.fl_ratio and len(self.fl) > 0:
            self.counts.fl_sample_count += 1
            np.random.randint(len(self.fl))
            return self.fl.draw_item()
        if len(self.dlbcl) > 0:
            self.counts.dlbcl_sample_count += 1
            np.random.randint(len(self.dlbcl))
            return self.dlbcl.draw_item()
        np.random.randint(len(self.fl))
        return self.fl.draw_item()

    def sample_batch(self, B):
        if self._dd is not None:
            return self._dd.launch(B)
        items = [self.draw_item() for _ in range(B)]
        self.last_draws = [i[0] for i in items]
        return cut_patches(items, self.patch_size, self.dev)

    def replay_batch(self, B):
        return self._device_draws().replay(B)

    def draw_records(self, B):
        self._device_draws().launch(B, cut=False)
        return self._dd.records()


class DevicePatchLoader:
    """The training DataLoader of loader.py:9-10 (batch_size, shuffle=True, drop_last=False)
    over a device dataset, with num_workers = 0 semantics: batch k holds the next batch_size
    __getitem__ draws of the process's global numpy / python RNGs (the sampler's index order is
    irrelevant: __getitem__ ignores its index, patch_dataset.py:114-124, :254-261), the last batch
    is ragged, and each epoch takes the two int64 seeds a torch DataLoader iterator draws from
    torch's global generator (the iterator's base seed and RandomSampler's seed), so the torch
    RNG stream after an epoch is the host loader's.  Batches are device tensors
    (images, labels) [b, 1, *patch_size].

    Over a draws="device" dataset the batches are the device stream's instead (the global numpy /
    python RNGs are not touched): every full batch is one replay of the dataset's captured
    draw -> cut -> counter chain (captured once per batch size), the ragged last batch runs the
    same chain eagerly, and the batch tensors are the dataset's persistent buffers (consume a
    batch before asking for the next).  The mixed dataset's domain counts are moved from the
    device onto its `counts` object once, after the last batch."""

    def __init__(self, dataset, batch_size):
        self.dataset, self.batch_size = dataset, int(batch_size)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        torch.empty((), dtype=torch.int64).random_()   # _BaseDataLoaderIter._base_seed
        torch.empty((), dtype=torch.int64).random_()   # RandomSampler's generator seed
        n = len(self.dataset)
        device = getattr(self.dataset, "draws", "host") == "device"
        for b0 in range(0, n, self.batch_size):
            b = min(self.batch_size, n - b0)
            if device and b == self.batch_size:
                yield self.dataset.replay_batch(b)
            else:
                yield self.dataset.sample_batch(b)
        if device and hasattr(self.dataset, "flush_counts"):
            self.dataset.flush_counts()


def device_loader(dataset, batch_size, read=None, device=None, draws="host", draw_seed=None):
    """A DevicePatchLoader for a reference PatchDataset / MixedPatchDataset (by duck type:
    MixedPatchDataset carries fl_dataset / dlbcl_dataset).  draws="device": the device draw
    stream (draw_seed defaults to the reference dataset's seed)."""
    _check_mode(draws)
    if hasattr(dataset, "fl_dataset") and hasattr(dataset, "dlbcl_dataset"):
        dd = DeviceMixedPatchDataset.from_reference(dataset, read, device, draws, draw_seed)
    else:
        dd = DevicePatchDataset.from_reference(dataset, read, device, draws, draw_seed)
    return DevicePatchLoader(dd, batch_size)
