"""Writes tests/golden/quantify.npz: inputs and expected results for the lesion uptake report
(light_unet/quantify.py, csrc/quantify.hip), from scipy and numpy on the CPU, written straight from
the definitions in light_unet/quantify.py's docstring.

    python tests/golden/make_quantify_goldens.py

    lesions      scipy.ndimage.label (6-connectivity), components below min_size dropped and the
                 rest renumbered in order
    peak map     zero-padded shifted float64 copies accumulated in the order of the offset set,
                 divided by the accumulated in-volume count (asserted equal, bit for bit, to a direct
                 per-voxel loop that skips the offsets outside the volume)
    suv_mean     math.fsum, the correctly rounded sum, over the voxel count; the sum of |v| is stored
                 next to it for the summation bound of the unquantised family
    Dmax         brute force over all voxel pairs of the mask in numpy float64 (which never fuses),
                 asserted equal -- value and pair -- to brute force over the corner voxels alone

Before anything is written the generator also asserts that no integer offset's squared length lies
within 1e-9 relative of the sphere's r^2 (the offset set does not hinge on a rounding).  Masks are
stored bit-packed (np.packbits over the flat C order), quantised uptake as int32 multiples of 2^-10,
floats of the expected dicts as float.hex strings in one JSON document.  Written with scipy 1.15.3.
"""
import json
import math
import os

import numpy as np
from scipy import ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
SPACINGS = [(4.0, 4.0, 4.0), (3.27, 2.0364, 2.0364), (2.0, 2.0, 2.0)]
N_OFFSETS = [19, 71, 123]
SHAPES = [(5, 9, 70), (3, 40, 129), (12, 20, 70), (24, 40, 40), (2, 3, 600)]
PEAK_ML = 1.0


# ---------------------------------------------------------------- the definitions
def offsets(spacing, peak_ml=PEAK_ML):
    r = float(np.cbrt(3000.0 * peak_ml / (4.0 * np.pi)))
    r2 = r * r
    sz, sy, sx = (np.float64(s) for s in spacing)
    out = []
    for dz in range(-6, 7):
        for dy in range(-6, 7):
            for dx in range(-6, 7):
                a, b, c = np.float64(dz) * sz, np.float64(dy) * sy, np.float64(dx) * sx
                q = (a * a + b * b) + c * c
                assert abs(q - r2) > 1e-9 * r2, (spacing, dz, dy, dx)
                if q <= r2:
                    out.append((dz, dy, dx))
    assert max(abs(v) for o in out for v in o) <= 4
    return out


def peak_map(up, offs):
    D, H, W = up.shape
    P = np.pad(up.astype(np.float64), 6)
    ones = np.pad(np.ones(up.shape, dtype=np.int64), 6)
    S = np.zeros(up.shape, dtype=np.float64)
    n = np.zeros(up.shape, dtype=np.int64)
    for dz, dy, dx in offs:
        cut = (slice(6 + dz, 6 + dz + D), slice(6 + dy, 6 + dy + H), slice(6 + dx, 6 + dx + W))
        S = S + P[cut]
        n += ones[cut]
    return S / n.astype(np.float64)


def peak_loop(up, offs):
    """The same map by the definition's own words: per voxel, skip what leaves the volume."""
    D, H, W = up.shape
    out = np.empty(up.shape, dtype=np.float64)
    for z in range(D):
        for y in range(H):
            for x in range(W):
                s, n = np.float64(0.0), 0
                for dz, dy, dx in offs:
                    a, b, c = z + dz, y + dy, x + dx
                    if 0 <= a < D and 0 <= b < H and 0 <= c < W:
                        s = s + np.float64(up[a, b, c])
                        n += 1
                out[z, y, x] = s / np.float64(n)
    return out


def lesions_of(mask, min_size):
    lab, num = ndi.label(mask)
    if min_size > 0 and num:
        sizes = np.bincount(lab.ravel(), minlength=num + 1)
        keep = sizes >= min_size
        keep[0] = False
        remap = np.zeros(num + 1, dtype=lab.dtype)
        remap[keep] = np.arange(1, int(keep.sum()) + 1)
        lab, num = remap[lab], int(keep.sum())
    return lab, num


def d2_rows(a, b, spacing):
    sz, sy, sx = (np.float64(s) for s in spacing)
    dz = (a[:, None, 0] - b[None, :, 0]).astype(np.float64) * sz
    dy = (a[:, None, 1] - b[None, :, 1]).astype(np.float64) * sy
    dx = (a[:, None, 2] - b[None, :, 2]).astype(np.float64) * sx
    return (dz * dz + dy * dy) + dx * dx


def farthest(vox, spacing, chunk=512):
    """(d2, i, j) over the rows of `vox` (ascending flat index): the largest d2, then the smallest
    i, then the smallest j > i; None below two rows."""
    n = len(vox)
    if n < 2:
        return None
    best = (-1.0, -1, -1)
    cols = np.arange(n)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        d = d2_rows(vox[lo:hi], vox, spacing)
        d[cols[None, :] <= np.arange(lo, hi)[:, None]] = -1.0
        k = int(np.argmax(d))           # the first maximum in row-major order: smallest i, then j
        v = float(d.flat[k])
        if v > best[0]:
            best = (v, lo + k // n, k % n)
    return best


def corners(mask):
    p = np.pad(mask, 1)
    c = p[1:-1, 1:-1, 1:-1]
    return (c & ~(p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1]) & ~(p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1])
            & ~(p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:]))


def report(up, mask, spacing, min_size, offs):
    """(expected dict, per-lesion (exact sums, sums of |v|), peak map, labels, corner mask)."""
    shape = up.shape
    lab, num = lesions_of(mask, min_size)
    pm = peak_map(up, offs)
    voxel_ml = spacing[0] * spacing[1] * spacing[2] / 1000.0
    sp = np.asarray(spacing, dtype=np.float64)
    rows, sum_abs, sums = [], [], []
    for l in range(1, num + 1):
        idx = np.flatnonzero(lab.ravel() == l)
        vals = up.ravel()[idx]
        voxels = len(idx)
        volume_ml = float(np.int64(voxels) * voxel_ml)
        sums.append(math.fsum(float(v) for v in vals))
        suv_mean = sums[-1] / voxels
        sum_abs.append(math.fsum(abs(float(v)) for v in vals))
        k, kp = int(np.argmax(vals)), int(np.argmax(pm.ravel()[idx]))
        zyx = np.stack(np.unravel_index(idx, shape), axis=1)
        rows.append({"label": l, "voxels": voxels, "volume_ml": volume_ml,
                     "suv_max": float(vals[k]),
                     "suv_max_voxel": [int(v) for v in zyx[k]],
                     "suv_mean": suv_mean,
                     "suv_peak": float(pm.ravel()[idx][kp]),
                     "suv_peak_voxel": [int(v) for v in zyx[kp]],
                     "tlg": suv_mean * volume_ml,
                     "centroid_mm": [float(v) for v in
                                     zyx.sum(axis=0).astype(np.float64) / np.float64(voxels) * sp]})
    M = lab > 0
    vox = np.argwhere(M)
    cm = corners(M)
    far = farthest(vox, spacing)
    far_c = farthest(np.argwhere(cm), spacing)
    if far is None:
        assert far_c is None
        dmax_mm, dmax_voxels = 0.0, None
    else:
        cv = np.argwhere(cm)
        pair = [[int(v) for v in vox[far[1]]], [int(v) for v in vox[far[2]]]]
        assert far_c is not None and far_c[0] == far[0]
        assert pair == [[int(v) for v in cv[far_c[1]]], [int(v) for v in cv[far_c[2]]]]
        dmax_mm, dmax_voxels = float(np.sqrt(np.float64(far[0]))), pair
    cd = 0.0
    for i in range(num):
        for j in range(i + 1, num):
            a, b = rows[i]["centroid_mm"], rows[j]["centroid_mm"]
            dz, dy, dx = a[0] - b[0], a[1] - b[1], a[2] - b[2]
            cd = max(cd, math.sqrt((dz * dz + dy * dy) + dx * dx))
    total = int(M.sum())
    exp = {"lesions": rows, "n_lesions": num, "tmtv_ml": float(np.int64(total) * voxel_ml),
           "tlg_total": float(sum(r["tlg"] for r in rows)),
           "suv_max": max((r["suv_max"] for r in rows), default=0.0),
           "suv_peak": max((r["suv_peak"] for r in rows), default=0.0),
           "dmax_mm": dmax_mm, "dmax_voxels": dmax_voxels, "dmax_centroid_mm": cd}
    return exp, (sums, sum_abs), pm, lab, cm


def hexed(v):
    if isinstance(v, float):
        return {"f": v.hex()}
    if isinstance(v, dict):
        return {k: hexed(x) for k, x in v.items()}
    if isinstance(v, list):
        return [hexed(x) for x in v]
    return v


# ---------------------------------------------------------------- inputs
def blob_mask(shape, rng):
    """3-6 ellipsoid lesions, at least two of them cut by the border of the volume."""
    zz, yy, xx = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    for _ in range(1000):
        m = np.zeros(shape, dtype=bool)
        for _ in range(int(rng.integers(4, 8))):
            c = [rng.uniform(-0.05 * n, 1.05 * n) for n in shape]
            r = [rng.uniform(1.2, max(2.0, min(0.22 * n, 7.0))) for n in shape]
            m |= (((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2) <= 1.0
        lab, num = ndi.label(m)
        cut = 0
        for sl in ndi.find_objects(lab):
            cut += any(s.start == 0 or s.stop == n for s, n in zip(sl, shape) if n > 3)
        if 3 <= num <= 6 and cut >= 2:
            return m
    raise AssertionError(shape)


def hot_spots(shape, rng, count=4):
    zz, yy, xx = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    out = np.zeros(shape, dtype=np.float64)
    for _ in range(count):
        c = [rng.uniform(0, n - 1) for n in shape]
        out += rng.uniform(4.0, 12.0) * np.exp(-((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2)
                                               / rng.uniform(3.0, 12.0))
    return out


def quantised(shape, rng):
    """Multiples of 2^-10 below 2^10 (here below 32): every float64 sum is exact in any order."""
    k = rng.integers(0, 1 << 12, size=shape) + np.floor(hot_spots(shape, rng) * 1024.0).astype(np.int64)
    assert k.min() >= 0 and k.max() < 1 << 20
    return k.astype(np.int32)


def main():
    rng = np.random.default_rng(20251020)
    arrays, entries, offs_index = {}, [], []
    offs = [offsets(s) for s in SPACINGS]
    for s, o, n in zip(SPACINGS, offs, N_OFFSETS):
        assert len(o) == n, (s, len(o))
        offs_index.append({"spacing": list(s), "peak_ml": PEAK_ML, "offsets": [list(v) for v in o]})
    assert len(offsets((3.0, 1.5, 1.5))) == 157

    ups, masks = {}, {}

    def put_mask(name, m):
        masks[name] = np.asarray(m, dtype=bool)
        arrays["mask_" + name] = np.packbits(masks[name].ravel())

    def put_up(name, vol=None, k=None):
        if k is not None:                      # quantised: the int32 multiples of 2^-10
            arrays["upq_" + name] = k
            vol = (k.astype(np.float64) / 1024.0).astype(np.float32)
            assert np.array_equal(vol.astype(np.float64) * 1024.0, k.astype(np.float64))
        else:
            arrays["up_" + name] = vol
        assert vol.dtype == np.float32 and np.all(np.isfinite(vol))
        ups[name] = vol

    peak_stored = set()

    def entry(up_name, mask_name, si, family, min_size=0, store_peak=False):
        up, mask, spacing = ups[up_name], masks[mask_name], SPACINGS[si]
        exp, (sums, sum_abs), pm, lab, cm = report(up, mask, spacing, min_size, offs[si])
        name = f"{up_name}__{mask_name}__s{si}__m{min_size}"
        e = {"name": name, "shape": list(up.shape), "spacing": list(spacing), "uptake": up_name,
             "mask": mask_name, "min_size": min_size, "family": family, "peak_ml": PEAK_ML,
             "expected": hexed(exp), "sum": hexed(sums), "sum_abs": hexed(sum_abs)}
        ckey = f"corner_{mask_name}__m{min_size}"
        if ckey not in arrays:
            arrays[ckey] = np.packbits(cm.ravel())
        e["corner"] = ckey
        if store_peak:
            arrays["peak_" + name] = pm[lab > 0]       # at labelled voxels, ascending flat index
            e["peak"] = "peak_" + name
            peak_stored.add(si)
        entries.append(e)
        return exp

    # the substitution of padding for skipping, checked against the per-voxel loop once
    small = rng.gamma(2.0, 1.0, size=(5, 9, 12)).astype(np.float32)
    small[rng.random(small.shape) < 0.1] *= -1.0
    for o in offs:
        a, b = peak_map(small, o), peak_loop(small, o)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))

    # ---- blob masks on every shape, both uptake families, every spacing
    for shape in SHAPES:
        tag = "x".join(map(str, shape))
        m = blob_mask(shape, rng)
        if shape == (5, 9, 70):   # lesions on every face, and a run across the 64-bit word
            m[0, 4, 10] = m[4, 4, 20] = m[2, 0, 30] = m[2, 8, 40] = m[2, 4, 0] = m[2, 4, 69] = True
            m[1, 6, 60:68] = True
        put_mask("blobs_" + tag, m)
        put_up("q_" + tag, k=quantised(shape, rng))
        g = (rng.gamma(2.0, 1.0, size=shape) + hot_spots(shape, rng)).astype(np.float32)
        put_up("g_" + tag, vol=g)
        for si in range(3):
            big = shape == (12, 20, 70)
            entry("q_" + tag, "blobs_" + tag, si, "a", store_peak=big)
            exp = entry("g_" + tag, "blobs_" + tag, si, "b")
        if shape != (5, 9, 70):
            assert 3 <= exp["n_lesions"] <= 6

    # ---- a min_size that drops some lesions
    tag = "24x40x40"
    sizes = sorted(r["voxels"] for r in entry("g_" + tag, "blobs_" + tag, 0, "b")["lesions"])
    entries.pop()
    cut = sizes[len(sizes) // 2]
    exp = entry("g_" + tag, "blobs_" + tag, 1, "b", min_size=cut)
    assert 0 < exp["n_lesions"] < len(sizes)
    entry("q_" + tag, "blobs_" + tag, 2, "a", min_size=cut)

    # ---- a constant volume (every maximum ties: the first index wins) and one with negative values
    shape, tag = (12, 20, 70), "12x20x70"
    put_up("const_" + tag, k=np.full(shape, 2560, dtype=np.int32))
    put_up("neg_" + tag, k=arrays["upq_q_" + tag] - (8 << 10))
    assert ups["neg_" + tag].min() < -4.0
    for si in range(3):
        exp = entry("const_" + tag, "blobs_" + tag, si, "a")
        assert all(r["suv_max"] == 2.5 == r["suv_peak"] == r["suv_mean"] for r in exp["lesions"])
        entry("neg_" + tag, "blobs_" + tag, si, "a")

    # ---- the empty mask, the full volume, a single voxel, two voxels in opposite corners
    shape, tag = (5, 9, 70), "5x9x70"
    put_mask("empty_" + tag, np.zeros(shape, bool))
    put_mask("full_" + tag, np.ones(shape, bool))
    one = np.zeros(shape, bool)
    one[3, 8, 64] = True
    put_mask("single_" + tag, one)
    two = np.zeros(shape, bool)
    two[0, 0, 0] = two[4, 8, 69] = True
    put_mask("two_" + tag, two)
    for name in ("empty_", "full_", "single_", "two_"):
        for si, fam in ((0, "a"), (1, "b"), (2, "a")):
            entry(("q_" if fam == "a" else "g_") + tag, name + tag, si, fam)

    # ---- one row of five voxels
    shape, tag = (1, 1, 5), "1x1x5"
    put_up("q_" + tag, k=np.asarray([[[1024, 5120, 3, 5120, 2048]]], dtype=np.int32))
    put_up("g_" + tag, vol=rng.gamma(2.0, 1.0, size=shape).astype(np.float32))
    put_mask("full_" + tag, np.ones(shape, bool))
    put_mask("split_" + tag, np.asarray([[[1, 1, 0, 1, 0]]], dtype=bool))
    put_mask("two_" + tag, np.asarray([[[1, 0, 0, 0, 1]]], dtype=bool))
    put_mask("empty_" + tag, np.zeros(shape, bool))
    for name in ("full_", "split_", "two_", "empty_"):
        for si in range(3):
            entry("q_" + tag, name + tag, si, "a")
        entry("g_" + tag, name + tag, 1, "b")

    assert peak_stored == {0, 1, 2}
    index = {"offsets": offs_index, "entries": entries}
    arrays["index"] = np.frombuffer(json.dumps(index).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "quantify.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(entries)} entries")
    assert os.path.getsize(path) < 700_000


if __name__ == "__main__":
    main()
