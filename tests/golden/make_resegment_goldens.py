"""Writes tests/golden/resegment.npz: the inputs and expected results of light_unet/resegment.py,
from numpy and scipy 1.15.3 only (scipy.ndimage.label, once for the seeds and once per box for the
candidates).  Run from the repository root:  python tests/golden/make_resegment_goldens.py

Per case `name`: labels_<name> uint8 (the regions, kept seeds renumbered), status_<name> int8,
reached_<name>, owned_<name> int64, thresholds_<name> float64, seed_label_<name> int32.  Inputs are
shared between cases: up_<key> float32 or upq_<key> int16 (multiples of 2^-8), seeds_<key> uint8
(scipy's labelling of the seed mask), body_<key> uint8.  `index` is the JSON list of the cases."""
import json
import math
import os

import numpy as np
from scipy import ndimage

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resegment.npz")
arrays, cases = {}, []


def resegment(up, seed_labels, spacing, method, value, grow_mm, body=None):
    shape, n = up.shape, int(seed_labels.max())
    thr = np.zeros(n, np.float64)
    regions = []
    for i in range(n):
        seed = seed_labels == i + 1
        m = np.float32(up[seed].max())
        thr[i] = np.float64(value) if method == "fixed" else np.float64(value) * np.float64(m)
        cand = up.astype(np.float64) >= thr[i]
        if body is not None:
            cand &= body != 0
        if grow_mm is None:
            regions.append(seed & cand)
            continue
        sl = ndimage.find_objects(seed.astype(np.int32))[0]
        box = tuple(slice(max(0, s.start - int(math.ceil(grow_mm / spacing[a]))),
                          min(shape[a], s.stop + int(math.ceil(grow_mm / spacing[a]))))
                    for a, s in enumerate(sl))
        comp, _ = ndimage.label(cand[box])   # 6-connectivity inside the box only
        hit = np.unique(comp[seed[box] & cand[box]])
        full = np.zeros(shape, bool)
        full[box] = np.isin(comp, hit[hit > 0])
        regions.append(full)
    first = np.zeros(shape, np.int64)
    for i in reversed(range(n)):
        first[regions[i]] = i + 1
    reached = np.asarray([r.sum() for r in regions], np.int64)
    owned = np.bincount(first.ravel(), minlength=n + 1)[1:n + 1].astype(np.int64)
    status = np.where(owned > 0, 0, np.where(reached == 0, 1, 2)).astype(np.int8)
    keep = np.flatnonzero(owned > 0)
    remap = np.zeros(n + 1, np.int64)
    remap[keep + 1] = np.arange(1, len(keep) + 1)
    assert len(keep) <= 255
    return {"labels": remap[first].astype(np.uint8), "status": status, "reached": reached,
            "owned": owned, "thresholds": thr, "seed_label": (keep + 1).astype(np.int32)}


def add_inputs(key, up, mask, body=None, quantised=False):
    up = np.ascontiguousarray(up, np.float32)
    if quantised:
        q = np.round(up.astype(np.float64) * 256.0)
        assert np.abs(q).max() < 32768
        arrays["upq_" + key] = q.astype(np.int16)
        up = (q / 256.0).astype(np.float32)
    else:
        arrays["up_" + key] = up
    lab, n = ndimage.label(mask)
    assert n <= 255
    arrays["seeds_" + key] = lab.astype(np.uint8)
    if body is not None:
        arrays["body_" + key] = body.astype(np.uint8)
    return up, lab.astype(np.int32), n


def add_case(family, name, key, up, lab, spacing, method, value, grow_mm, body_key=None, report=False):
    body = arrays["body_" + body_key] if body_key else None
    res = resegment(up, lab, spacing, method, value, grow_mm, body)
    for k, v in res.items():
        arrays[f"{k}_{name}"] = v
    c = {"family": family, "name": name, "uptake": key, "seeds": key, "body": body_key,
         "shape": list(up.shape), "spacing": list(spacing), "method": method, "value": value,
         "grow_mm": grow_mm}
    if report:   # what lesion_uptake(..., resegment=) reports exactly
        voxel_ml = spacing[0] * spacing[1] * spacing[2] / 1000.0
        rows = []
        for k, s in enumerate(res["seed_label"]):
            region = res["labels"] == k + 1
            rows.append({"label": k + 1, "voxels": int(region.sum()),
                         "suv_max": float(up[region].max()), "seed_label": int(s),
                         "seed_voxels": int((lab == s).sum()),
                         "threshold": float(res["thresholds"][s - 1])})
        c["report"] = {"lesions": rows,
                       "tmtv_ml": float(np.int64(sum(r["voxels"] for r in rows)) * voxel_ml),
                       "below_threshold": [int(i) + 1 for i in np.flatnonzero(res["status"] == 1)],
                       "absorbed": [int(i) + 1 for i in np.flatnonzero(res["status"] == 2)]}
    cases.append(c)
    return res


ISO = (4.0, 4.0, 4.0)

# 1. the seam of two 64-bit words and the padding bits of the last one
up = np.ones((12, 12, 70), np.float32)
up[:, :, 5:70] = 5.0
mask = np.zeros(up.shape, bool)
mask[6, 6, 60:69] = True
up, lab, n = add_inputs("seam", up, mask)
r = add_case("seam", "seam", "seam", up, lab, ISO, "fixed", 4.0, 1000.0)
assert n == 1 and r["reached"].tolist() == [12 * 12 * 65]

# 2. a serpentine path of candidates through a 10 x 12 x 20 box, the seed its first voxel
path, xdir, xend = [], 1, 0
for p in range(5):
    ys = [0, 2, 4, 6, 8, 10] if p % 2 == 0 else [10, 8, 6, 4, 2, 0]
    for j, y in enumerate(ys):
        xs = list(range(20)) if xdir > 0 else list(range(19, -1, -1))
        path += [(2 * p, y, x) for x in xs]
        xend, xdir = xs[-1], -xdir
        if j < 5:
            path.append((2 * p, (y + ys[j + 1]) // 2, xend))
    if p < 4:
        path.append((2 * p + 1, ys[-1], xend))
assert len(path) == len(set(path)) and len(path) >= 300
up = np.ones((10, 12, 20), np.float32)
up[tuple(np.asarray(path).T)] = 5.0
mask = np.zeros(up.shape, bool)
mask[path[0]] = True
up, lab, n = add_inputs("serpentine", up, mask)
r = add_case("serpentine", "serpentine", "serpentine", up, lab, ISO, "fixed", 4.0, 1000.0)
assert r["reached"].tolist() == [len(path)]
cand = up >= 4.0
steps, seen = 0, mask.copy()   # the geodesic length: one dilation per step
while True:
    grown = ndimage.binary_dilation(seen, mask=cand) | seen
    if (grown == seen).all():
        break
    seen, steps = grown, steps + 1
assert steps == len(path) - 1 >= 300

# 3. a blob inside the padded box that joins the seed only through voxels outside the box
up = np.ones((8, 8, 40), np.float32)
mask = np.zeros(up.shape, bool)
mask[4, 4, 10:13] = True
detour = [(4, 4, x) for x in range(10, 16)] + [(z, 4, 15) for z in (3, 2, 1)] + \
         [(1, 4, x) for x in range(14, 7, -1)] + [(1, 3, 8), (1, 2, 8), (2, 2, 8)]
up[tuple(np.asarray(detour).T)] = 5.0
up, lab, n = add_inputs("boxcut", up, mask)
r = add_case("boxcut", "boxcut", "boxcut", up, lab, ISO, "fixed", 4.0, 8.0)
whole, _ = ndimage.label(up >= 4.0)
assert whole[2, 2, 8] == whole[4, 4, 10] > 0            # joined in the whole volume,
assert 2 <= 2 <= 6 and 8 <= 8 <= 14                      # inside the box z 2..6, y 2..6, x 8..14,
assert r["labels"][2, 2, 8] == 0 and r["labels"][4, 4, 14] == 1 and r["reached"].tolist() == [5]

# 4. two seeds with overlapping padded boxes in one hot region
up = np.ones((8, 8, 48), np.float32)
up[2:6, 2:6, 4:45] = 6.0
mask = np.zeros(up.shape, bool)
mask[3, 3, 10:13] = True
mask[3, 3, 20:23] = True
up, lab, n = add_inputs("overlap_keep", up, mask)
r = add_case("overlap", "overlap_keep", "overlap_keep", up, lab, ISO, "fixed", 4.0, 16.0)
assert n == 2 and r["status"].tolist() == [0, 0] and r["labels"][3, 3, 16] == 1
assert r["labels"][3, 3, 17] == 2 and r["owned"][1] < r["reached"][1]
up = np.ones((8, 8, 48), np.float32)
up[2:6, 2:5, 4:45] = 6.0
mask = np.zeros(up.shape, bool)
mask[2:6, 2, 8:31] = True
mask[3, 4, 20] = True
mask[3, 4, 40:42] = True
up, lab, n = add_inputs("overlap_absorb", up, mask)
r = add_case("overlap", "overlap_absorb", "overlap_absorb", up, lab, ISO, "fixed", 4.0, 8.0)
assert n == 3 and r["status"].tolist() == [0, 2, 0] and r["seed_label"].tolist() == [1, 3]
assert r["labels"][3, 4, 40] == 2 and r["labels"][3, 4, 20] == 1

# 5. a seed whose maximum lies below the fixed threshold
up = np.ones((6, 6, 10), np.float32)
up[1:3, 1:3, 1:3] = 3.0
up[3:5, 3:5, 6:9] = 6.0
mask = np.zeros(up.shape, bool)
mask[1:3, 1:3, 1:3] = True
mask[3:5, 3:5, 6:8] = True
up, lab, n = add_inputs("below", up, mask)
r = add_case("below", "below", "below", up, lab, ISO, "fixed", 4.0, 8.0)
assert r["status"].tolist() == [1, 0] and r["seed_label"].tolist() == [2] and r["reached"][0] == 0

# 6. a body mask that cuts a region
up = np.ones((8, 8, 40), np.float32)
up[2:6, 2:6, 4:36] = 5.0
mask = np.zeros(up.shape, bool)
mask[3, 3, 8:11] = True
bm = np.ones(up.shape, np.uint8)
bm[:, :, 20] = 0
up, lab, n = add_inputs("body", up, mask, body=bm)
r = add_case("body", "body", "body", up, lab, ISO, "fixed", 4.0, 1000.0, body_key="body")
assert r["reached"].tolist() == [4 * 4 * 16]
r = add_case("body", "body_off", "body", up, lab, ISO, "fixed", 4.0, 1000.0)
assert r["reached"].tolist() == [4 * 4 * 32]

# 7. seeds on the faces of the volume: clipped boxes
up = np.ones((6, 7, 9), np.float32)
up[0], up[5] = 5.0, 5.0
up[:, 0, 0], up[:, 6, 8] = 5.0, 5.0
mask = np.zeros(up.shape, bool)
for v in ((0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (5, 6, 8), (5, 5, 8), (5, 6, 7), (4, 6, 8)):
    mask[v] = True
up, lab, n = add_inputs("faces", up, mask)
for g, tag in ((None, "none"), (0.0, "0"), (1000.0, "1000")):
    r = add_case("faces", "faces_" + tag, "faces", up, lab, ISO, "fixed", 4.0, g)
    if g is None:
        assert r["reached"].tolist() == [4, 4]
    elif g == 0.0:
        assert r["reached"].tolist() == [5, 5] and r["status"].tolist() == [0, 0]
    else:
        assert r["status"].tolist() == [0, 2] and r["reached"][0] == r["reached"][1] == (up > 4).sum()

# 8. the witness of the float64 comparison: float64(u) >= 0.41 * float64(m) is false where the
#    float32 comparison u >= float32(0.41 * m) is true
rng = np.random.default_rng(41)
witness = None
for m in (rng.random(4000, dtype=np.float32) * np.float32(20.0) + np.float32(2.0)):
    t64 = np.float64(0.41) * np.float64(m)
    u = np.float32(t64)
    if np.float64(u) < t64:
        witness = (np.float32(m), u)
        break
assert witness is not None
m, u = witness
assert not (np.float64(u) >= np.float64(0.41) * np.float64(m)) and u >= np.float32(np.float64(0.41) * np.float64(m))
above = np.nextafter(u, np.float32(np.inf))
assert np.float64(above) >= np.float64(0.41) * np.float64(m)
up = np.zeros((3, 3, 5), np.float32)
up[1, 1, 2] = m
up[1, 1, 1] = u        # adjacent to the seed, just below the float64 threshold: stays out
up[1, 1, 3] = above    # adjacent, one float32 step higher: comes in
mask = np.zeros(up.shape, bool)
mask[1, 1, 2] = True
up, lab, n = add_inputs("witness", up, mask)
r = add_case("witness", "witness", "witness", up, lab, ISO, "relative", 0.41, 4.0)
assert r["labels"][1, 1].tolist() == [0, 0, 1, 1, 0]

# 9. relative at 1.0: the voxels equal to the maximum joined to one in the seed; and a voxel exactly
#    at the threshold
up = np.ones((4, 4, 12), np.float32)
up[1, 1, 2:6] = (3.0, 7.0, 7.0, 3.0)
up[1, 2, 3] = 7.0      # outside the seed, next to a maximum of the seed: in
up[2, 2, 5] = 7.0      # inside the box, joined to nothing: out
up[1, 1, 8] = 7.0      # outside the box
mask = np.zeros(up.shape, bool)
mask[1, 1, 2:6] = True
up, lab, n = add_inputs("rel_one", up, mask)
r = add_case("relative", "rel_one", "rel_one", up, lab, ISO, "relative", 1.0, 4.0)
assert r["reached"].tolist() == [3] and r["labels"][1, 2, 3] == 1 and r["labels"][2, 2, 5] == 0
up = np.ones((4, 4, 12), np.float32)
up[1, 1, 2:5] = (8.0, 4.0, np.nextafter(np.float32(4.0), np.float32(0.0)))
mask = np.zeros(up.shape, bool)
mask[1, 1, 2] = True
up, lab, n = add_inputs("rel_half", up, mask)
r = add_case("relative", "rel_half", "rel_half", up, lab, ISO, "relative", 0.5, 8.0)
assert r["thresholds"].tolist() == [4.0] and r["labels"][1, 1, 2:5].tolist() == [1, 1, 0]

# 10. a random case: smooth blobs plus noise, 10 seeds from a blob probability map
rng = np.random.default_rng(10)
shape = (40, 44, 70)
zz, yy, xx = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")
centres = [(6, 8, 10), (6, 30, 30), (8, 12, 55), (18, 22, 20), (20, 36, 60), (22, 8, 38),
           (30, 14, 12), (32, 34, 32), (33, 10, 62), (30, 28, 40)]
bump = np.zeros(shape)
prob = np.zeros(shape)
for k, (cz, cy, cx) in enumerate(centres):
    s = 2.0 + 0.35 * k
    d2 = ((zz - cz) * 1.4) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2
    bump += (0.5 if k == 2 else 5.0 + 1.3 * k) * np.exp(-d2 / (2.0 * s * s))
    prob = np.maximum(prob, np.exp(-d2 / (2.0 * (0.6 * s) ** 2)))
up = 1.0 + 0.4 * rng.gamma(2.0, 1.0, shape) + bump
up, lab, n = add_inputs("random", up, prob >= 0.5, quantised=True)
assert n == 10
kinds = set()
for sp, stag in (((3.0, 2.04, 2.04), "a"), (ISO, "i")):
    for method, value in (("fixed", 4.0), ("relative", 0.41)):
        for g in (None, 8.0, 16.0, 1000.0):
            name = f"random_{stag}_{method}_{'none' if g is None else int(g)}"
            r = add_case("random", name, "random", up, lab, sp, method, value, g,
                         report=(stag == "i" and g == 16.0))
            kinds |= set(r["status"].tolist())
            print(name, r["status"].tolist(), r["reached"].tolist(), r["owned"].tolist())
assert kinds == {0, 1, 2}, kinds

arrays["index"] = np.frombuffer(json.dumps({"cases": cases}).encode(), dtype=np.uint8)
np.savez_compressed(OUT, **arrays)
print(len(cases), "cases,", os.path.getsize(OUT), "bytes")
assert os.path.getsize(OUT) < 1000000
