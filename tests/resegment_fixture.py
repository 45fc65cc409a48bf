"""Readers of tests/golden/resegment.npz (tests/golden/make_resegment_goldens.py) and the contract of
light_unet/resegment.py restated as a plain numpy breadth-first search, shared by the host and the
device tests.  Nothing here needs scipy or a device."""
import json
import math
import os

import numpy as np

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resegment.npz")
_CACHE = {}

ARRAYS = ("labels", "status", "reached", "owned", "thresholds", "seed_label")


def load():
    """(npz, index): loaded once per session and never modified."""
    if not _CACHE:
        z = np.load(_PATH, allow_pickle=False)
        _CACHE["z"] = z
        _CACHE["index"] = json.loads(bytes(z["index"]).decode())
    return _CACHE["z"], _CACHE["index"]


def cases(family=None):
    return [c for c in load()[1]["cases"] if family is None or c["family"] == family]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def uptake(c):
    """The float32 volume; quantised ones are stored as int16 multiples of 2^-8."""
    key = ("up", c["uptake"])
    if key not in _CACHE:
        z, _ = load()
        if "upq_" + c["uptake"] in z.files:
            v = (z["upq_" + c["uptake"]].astype(np.float64) / 256.0).astype(np.float32)
        else:
            v = z["up_" + c["uptake"]]
        _CACHE[key] = v
    return _CACHE[key]


def seeds(c):
    """The seeds' int32 label map (scipy's numbering of the seed mask's components)."""
    return load()[0]["seeds_" + c["seeds"]].astype(np.int32)


def body(c):
    """The uint8 body mask, or None."""
    return None if c["body"] is None else load()[0]["body_" + c["body"]]


def expected(c):
    z, _ = load()
    return {k: z[f"{k}_{c['name']}"] for k in ARRAYS}


def padding(grow_mm, spacing):
    return tuple(int(math.ceil(grow_mm / float(s))) for s in spacing)


def reference(up, seed_labels, spacing, method, value, grow_mm, body_mask=None):
    """The contract on the host: {"labels" uint8, "status" int8, "reached", "owned" int64,
    "thresholds" float64, "seed_label" int32}.  up float32 [D, H, W], seed_labels int [D, H, W]."""
    up = np.asarray(up, dtype=np.float32)
    shape = up.shape
    n = int(seed_labels.max()) if seed_labels.size else 0
    up64 = up.astype(np.float64)
    thr = np.zeros(n, dtype=np.float64)
    regions = []
    for i in range(n):
        seed = seed_labels == i + 1
        if method == "fixed":
            thr[i] = np.float64(value)
        else:
            thr[i] = np.float64(value) * np.float64(up[seed].max())
        cand = up64 >= thr[i]
        if body_mask is not None:
            cand &= np.asarray(body_mask) != 0
        start = seed & cand
        if grow_mm is None:
            regions.append(start)
            continue
        pad = padding(grow_mm, spacing)
        zz = np.argwhere(seed)
        lo = [max(0, int(zz[:, a].min()) - pad[a]) for a in range(3)]
        hi = [min(shape[a], int(zz[:, a].max()) + 1 + pad[a]) for a in range(3)]
        box = tuple(slice(lo[a], hi[a]) for a in range(3))
        c, r = cand[box], start[box].copy()
        frontier = r.copy()
        while frontier.any():   # breadth first: one 6-neighbour step per round, inside the box
            nb = np.zeros_like(frontier)
            nb[1:] |= frontier[:-1]
            nb[:-1] |= frontier[1:]
            nb[:, 1:] |= frontier[:, :-1]
            nb[:, :-1] |= frontier[:, 1:]
            nb[:, :, 1:] |= frontier[:, :, :-1]
            nb[:, :, :-1] |= frontier[:, :, 1:]
            frontier = nb & c & ~r
            r |= frontier
        full = np.zeros(shape, dtype=bool)
        full[box] = r
        regions.append(full)
    first = np.zeros(shape, dtype=np.int64)
    for i in reversed(range(n)):
        first[regions[i]] = i + 1
    reached = np.asarray([int(r.sum()) for r in regions], dtype=np.int64)
    owned = np.bincount(first.ravel(), minlength=n + 1)[1:n + 1].astype(np.int64)
    status = np.where(owned > 0, 0, np.where(reached == 0, 1, 2)).astype(np.int8)
    keep = np.flatnonzero(owned > 0)
    remap = np.zeros(n + 1, dtype=np.int64)
    remap[keep + 1] = np.arange(1, len(keep) + 1)
    assert len(keep) <= 255
    return {"labels": remap[first].astype(np.uint8), "status": status, "reached": reached,
            "owned": owned, "thresholds": thr, "seed_label": (keep + 1).astype(np.int32)}


def check_result(rs, exp, what=""):
    """A light_unet.resegment.Resegmented against the expected arrays: every one equal, the
    thresholds as bits, and the Components consistent with its own label map."""
    lab = rs.components.numpy()
    assert lab.dtype == np.int32 and lab.shape == exp["labels"].shape, what
    differ = int((lab != exp["labels"]).sum())
    assert differ == 0, (what, differ)
    assert rs.status.dtype == np.int8 and np.array_equal(rs.status, exp["status"]), \
        (what, rs.status, exp["status"])
    assert rs.reached.dtype == np.int64 and np.array_equal(rs.reached, exp["reached"]), \
        (what, rs.reached, exp["reached"])
    assert rs.thresholds.dtype == np.float64 and np.array_equal(
        rs.thresholds.view(np.uint64), exp["thresholds"].view(np.uint64)), what
    assert rs.seed_label.dtype == np.int32 and np.array_equal(rs.seed_label, exp["seed_label"]), \
        (what, rs.seed_label, exp["seed_label"])
    kept = exp["owned"][exp["owned"] > 0]
    assert rs.components.num == len(kept) and np.array_equal(rs.components.sizes(), kept), what
    assert rs.seed_voxels.dtype == np.int64 and len(rs.seed_voxels) == len(exp["status"]), what
    for k in range(rs.components.num):   # the stats are those of the label map
        zz = np.argwhere(lab == k + 1)
        s = rs.components.stats[k]
        assert [int(v) for v in s[4:7]] == zz.min(axis=0).tolist(), what
        assert [int(v) for v in s[7:10]] == zz.max(axis=0).tolist(), what
        assert [int(v) for v in s[1:4]] == zz.sum(axis=0).tolist(), what
