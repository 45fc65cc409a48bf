"""Golden fixtures for case preprocessing, made by the REFERENCE's own code.

Run where a checkout of the reference exists, with scipy:
    L3U_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_preprocess_goldens.py
It loads the reference's scripts/preprocess_data.py by file path, unmodified, with stand-ins for
modules that only do I/O or configuration around the functions under test (`nibabel`, `tqdm`,
`light_unet.core.config`), and calls its clip_and_normalize, generate_body_mask and
calculate_voxel_thresholds on synthetic volumes.

tests/golden/preprocess.npz holds data only:
  * per normalisation case `<case>/image` (float32 or float64), `<case>/norm64` (the reference's
    float64 result; what it writes to disk is norm64.astype(float32)), `<case>/clip` (clip_min,
    clip_max as float64) and `<case>/mask` (np.packbits of the body mask of norm64);
  * per body-mask-only case `<case>/image` (the normalized input) and `<case>/mask`;
  * per morphology case `<case>/dil<i>` / `<case>/ero<i>`, i = 1..5: scipy's binary_dilation /
    binary_erosion (cross structure, border_value = 0, i iterations) of `<case>/image` > 0.5
    (of `tiles/morph_input`, the packed norm64 > 0.02, for `tiles`);
  * `meta` (JSON as uint8): per case the shape, arguments, the reference's metadata dicts, and
    `checks`: the measured count behind every discriminating condition, each asserted > 0 here so
    a fixture that stopped discriminating fails at generation time.
Volumes are built from few distinct values (quantised noise, flat regions) so that the float64
arrays compress; the arithmetic they pin does not depend on the entropy of the input.
"""
import importlib.util
import json
import os
import sys
import types
from fractions import Fraction

sys.dont_write_bytecode = True

import numpy as np
from scipy import ndimage

REF = os.environ.get("L3U_REFERENCE")
OUT = os.path.dirname(os.path.abspath(__file__))
DEFAULT_CFG = {"threshold": 0.02, "closing_voxels": 5, "keep_largest_component": True,
               "dilate_voxels": 3}
CROSS = ndimage.generate_binary_structure(3, 1)


def load_reference():
    for name in ("nibabel", "tqdm"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.tqdm = lambda it, **k: it
            sys.modules[name] = m
    for name in ("light_unet", "light_unet.core", "light_unet.core.config"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["light_unet.core.config"].ConfigManager = type("ConfigManager", (), {})
    spec = importlib.util.spec_from_file_location(
        "ref_preprocess_data", os.path.join(REF, "scripts", "preprocess_data.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in ("light_unet", "light_unet.core", "light_unet.core.config"):
        del sys.modules[name]
    return mod


def grid(shape):
    return np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")


def ball(shape, c, r):
    z, y, x = grid(shape)
    return ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0


# ---------------------------------------------------------------- the volumes
def vol_gauss(rng):
    return np.round(rng.normal(size=(40, 44, 36)) * 256.0) / 256.0


def vol_pet(rng, shape=(36, 40, 70)):
    """PET-like float32: air = exact 0, a body blob of quantised low uptake, hot spots, and a
    detached slab (the table) far enough from the body that closing does not join them."""
    v = np.zeros(shape, np.float32)
    D, H, W = shape
    body = ball(shape, (D / 2, H / 2 - 6, W / 2), (D * 0.30, H * 0.18, W * 0.40))
    v[body] = (rng.integers(16, 80, size=int(body.sum())) / 64.0).astype(np.float32)
    core = ball(shape, (D / 2, H / 2 - 6, W / 2), (D * 0.22, H * 0.13, W * 0.32))
    v[body & ~core] = np.float32(0.0625)   # a faint rim: above 0.02 normalised, below 0.1
    for _ in range(3):
        c = (rng.integers(D // 2 - 4, D // 2 + 4), rng.integers(H // 2 - 9, H // 2 - 3),
             rng.integers(W // 4, 3 * W // 4))
        hot = ball(shape, c, (2.0, 2.0, 2.5))
        v[hot] = (rng.integers(600, 1200, size=int(hot.sum())) / 64.0).astype(np.float32)
    v[ball(shape, (D / 2, H / 2 - 6, W / 2 + 8), (4, 4, 6))] = 0.0   # a cavity only closing fills
    v[8:D - 8, H - 7:H - 5, 8:W - 8] = np.float32(0.75)   # the slab
    return v


def vol_range(rng):
    return np.round((rng.random((12, 14, 20)) * 9.0 - 4.0) * 128.0) / 128.0


def vol_intidx(rng):
    return (rng.integers(0, 4096, size=(3, 3, 889)) / 256.0).astype(np.float32)


def vol_plant(rng):
    shape = (20, 20, 24)
    v = np.round(rng.random(shape) * 1024.0) / 1024.0
    u = rng.random(shape)
    v[u < 0.30] = 0.0
    v[u > 0.70] = 1.0
    v[(u > 0.30) & (u < 0.36)] = 0.02 + 1e-12
    v[(u > 0.36) & (u < 0.40)] = 0.02
    return v


def vol_tie():
    v = np.zeros((16, 16, 40), np.float64)
    v[6:10, 6:10, 6:10] = 1.0
    v[6:10, 6:10, 28:32] = 1.0
    return v


def vol_faces(rng):
    v = np.zeros((20, 24, 28), np.float64)
    v[0:12, 0:15, 5:28] = 1.0
    v[3:6, 3:7, 10:14] = 0.0   # a hole the closing fills
    return v


def vol_blobs(rng, shape, n=5):
    """A 0 / 1 float64 image: random boxes, holes and specks (both morphology directions work)."""
    m = np.zeros(shape, bool)
    for _ in range(n):
        lo = [int(rng.integers(0, max(1, s - 2))) for s in shape]
        hi = [min(s, l + int(rng.integers(2, max(3, s // 2 + 2)))) for s, l in zip(shape, lo)]
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    m ^= rng.random(shape) < 0.03
    return m.astype(np.float64)


def vol_tiles(rng):
    shape = (48, 56, 96)
    v = np.zeros(shape, np.float32)
    body = ball(shape, (24, 27, 48), (17, 19, 40))
    v[body] = (rng.integers(8, 40, size=int(body.sum())) / 32.0).astype(np.float32)
    v[ball(shape, (20, 24, 30), (3, 3, 4))] = np.float32(12.5)
    v[ball(shape, (30, 30, 70), (2, 3, 3))] = np.float32(20.0)
    v[ball(shape, (24, 27, 50), (4, 5, 6))] = 0.0          # a cavity
    v[6:42, 52:54, 4:92] = np.float32(0.5)                 # the table
    v[rng.random(shape) < 0.002] = np.float32(0.25)        # specks
    return v


# ---------------------------------------------------------------- recording
def jsonable(o):
    if isinstance(o, dict):
        return {k: jsonable(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [jsonable(v) for v in o]
    if isinstance(o, np.generic):
        return o.item()
    return o


def record_mask(ref, out, meta, case, image, cfg):
    mask, mm = ref.generate_body_mask(image, cfg)
    assert mask.dtype == bool and mask.shape == image.shape
    out[case + "/mask"] = np.packbits(mask)
    meta[case]["body_mask_config"] = cfg
    meta[case]["body_mask"] = jsonable(mm)
    return mask, mm


def record_norm(ref, out, meta, case, image, cfg=None, **kw):
    # the reference reads every volume with get_fdata(): a float32 image reaches it widened
    norm, m = ref.clip_and_normalize(np.asarray(image, dtype=np.float64), **kw)
    assert norm.dtype == np.float64
    out[case + "/image"] = image
    out[case + "/norm64"] = norm
    out[case + "/clip"] = np.array([m["clip_values"]["min"], m["clip_values"]["max"]], np.float64)
    meta[case] = {"shape": list(image.shape), "kind": "norm", "args": jsonable(kw),
                  "metadata": jsonable(m), "checks": {}}
    mask, mm = record_mask(ref, out, meta, case, norm, dict(cfg or DEFAULT_CFG))
    return norm, m, mask, mm


def record_image_mask(ref, out, meta, case, image, cfg=None):
    out[case + "/image"] = image
    meta[case] = {"shape": list(image.shape), "kind": "mask", "checks": {}}
    return record_mask(ref, out, meta, case, image, dict(cfg or DEFAULT_CFG))


def record_morph(out, meta, case, m0):
    for i in range(1, 6):
        out[f"{case}/dil{i}"] = np.packbits(ndimage.binary_dilation(m0, structure=CROSS, iterations=i))
        out[f"{case}/ero{i}"] = np.packbits(ndimage.binary_erosion(m0, structure=CROSS, iterations=i))
    meta[case]["morph"] = True
    # the equivalence the device pipeline rests on: closing with the radius-r structure is r cross
    # dilations then r cross erosions, both with outside = 0
    for r in (2, 5):
        st = ndimage.iterate_structure(CROSS, r)
        a = ndimage.binary_closing(m0, structure=st)
        b = ndimage.binary_erosion(ndimage.binary_dilation(m0, structure=CROSS, iterations=r),
                                   structure=CROSS, iterations=r)
        assert np.array_equal(a, b), (case, r)


def check(meta, case, name, value):
    value = int(value)
    assert value > 0, (case, name, value)
    meta[case]["checks"][name] = value


def closed(m0, r, border=0):
    d = ndimage.binary_dilation(m0, structure=CROSS, iterations=r)
    return ndimage.binary_erosion(d, structure=CROSS, iterations=r, border_value=border)


def main():
    if not REF:
        raise SystemExit("set L3U_REFERENCE to a checkout of the reference repository")
    ref = load_reference()
    rng = np.random.default_rng(20251019)
    out, meta = {}, {}

    # ---- plain fp64 path
    g = vol_gauss(rng)
    record_norm(ref, out, meta, "gauss", g)
    check(meta, "gauss", "distinct_values", len(np.unique(g)))

    # ---- PET-like float32: heavy ties, W = 70 tail bits, the largest-component step drops a slab
    pet = vol_pet(rng)
    assert pet.dtype == np.float32
    norm, m, mask, mm = record_norm(ref, out, meta, "pet", pet)
    check(meta, "pet", "zeros_above_half", int((pet == 0).sum()) * 2 - pet.size)
    vc = mm["voxel_counts"]
    check(meta, "pet", "largest_component_drops", vc["after_closing"] - vc["after_largest_component"])
    check(meta, "pet", "tail_bits", pet.shape[2] % 64)
    # ---- every branch of generate_body_mask on the pet volume
    variants = {"close0": {"closing_voxels": 0}, "close2": {"closing_voxels": 2},
                "keepall": {"keep_largest_component": False}, "dil0": {"dilate_voxels": 0},
                "dil1": {"dilate_voxels": 1}, "thr01": {"threshold": 0.1}}
    meta["pet"]["variants"] = {}
    for name, delta in variants.items():
        cfg = dict(DEFAULT_CFG, **delta)
        vmask, vmm = ref.generate_body_mask(norm, cfg)
        out[f"pet/variant/{name}"] = np.packbits(vmask)
        meta["pet"]["variants"][name] = {"config": cfg, "body_mask": jsonable(vmm)}
        check(meta, "pet", "variant_differs_" + name, int((vmask != mask).sum()))

    # ---- constant volume: clip_max == clip_min, empty mask, empty bbox
    const = np.full((6, 7, 9), 3.0, np.float32)
    norm, m, mask, mm = record_norm(ref, out, meta, "const", const)
    assert m["clip_values"]["min"] == m["clip_values"]["max"] and not mask.any()
    assert mm["bbox"] == {"min": [0, 0, 0], "max": [6, 7, 9]}
    check(meta, "const", "empty_mask", int(mask.size - mask.sum()))

    # ---- non-default arguments: separate multiply and add
    rv = vol_range(rng)
    norm, m, _, _ = record_norm(ref, out, meta, "range", rv, low_percentile=1.0,
                                high_percentile=99.0, target_range=(-1, 1))
    lo, hi = m["clip_values"]["min"], m["clip_values"]["max"]
    q = (np.clip(rv, lo, hi) - lo) / (hi - lo)
    # a reciprocal multiply in place of the true divide would differ here
    recip = (np.clip(rv, lo, hi) - lo) * (1.0 / (hi - lo))
    check(meta, "range", "reciprocal_multiply_differs", int((recip != q).sum()))
    check(meta, "range", "negative_inputs", int((rv < 0).sum()))
    # q * 2 is exact, so a fused multiply-add cannot show with the range (-1, 1); the same volume
    # with a scale that is no power of two pins the separate multiply and add
    norm, m, _, _ = record_norm(ref, out, meta, "scale", rv, low_percentile=1.0,
                                high_percentile=99.0, target_range=(0.1, 0.8))
    uq = np.unique(q)
    fused = np.array([float(Fraction(float(x)) * Fraction(0.8 - 0.1) + Fraction(0.1)) for x in uq])
    check(meta, "scale", "fused_multiply_add_differs", int((fused != uq * (0.8 - 0.1) + 0.1).sum()))

    # ---- n = 8001: the virtual index is an exact integer at q = 0.5 and 99.5 (g = 0)
    iv = vol_intidx(rng)
    record_norm(ref, out, meta, "intidx", iv)
    n = iv.size
    assert (0.5 / 100) * (n - 1) == 40.0 and (99.5 / 100) * (n - 1) == 7960.0
    check(meta, "intidx", "n", n)

    # ---- fp64 compare of the initial mask
    pv = vol_plant(rng)
    norm, m, _, _ = record_norm(ref, out, meta, "plant", pv)
    assert m["clip_values"]["min"] == 0.0 and m["clip_values"]["max"] == 1.0
    assert np.array_equal(norm, pv)
    check(meta, "plant", "float32_compare_differs",
          int(((norm.astype(np.float32) > np.float32(0.02)) != (norm > 0.02)).sum()))

    # ---- two identical components: the lowest label wins
    tv = vol_tie()
    mask, mm = record_image_mask(ref, out, meta, "tie", tv)
    lab, num = ndimage.label(closed(tv > 0.02, 5))
    sizes = ndimage.sum(np.ones_like(lab), lab, range(1, num + 1))
    assert num == 2 and sizes[0] == sizes[1]
    check(meta, "tie", "second_component_dropped", int(sizes[1]))
    assert mask[8, 8, 8] and not mask[8, 8, 30]

    # ---- a body on several volume faces: erosion with outside = 0
    fv = vol_faces(rng)
    record_image_mask(ref, out, meta, "faces", fv)
    check(meta, "faces", "outside1_erosion_differs",
          int((closed(fv > 0.02, 5, 0) != closed(fv > 0.02, 5, 1)).sum()))
    record_morph(out, meta, "faces", fv > 0.5)

    # ---- word tails, single-word rows, a volume thinner than the halo
    for name, shape in (("w9", (10, 11, 9)), ("w32", (9, 12, 32)), ("w33", (11, 10, 33)),
                        ("w64", (10, 9, 64)), ("w65", (9, 11, 65)), ("d3", (3, 12, 20))):
        bv = vol_blobs(rng, shape)
        record_image_mask(ref, out, meta, name, bv)
        record_morph(out, meta, name, bv > 0.5)
        check(meta, name, "set_voxels", int((bv > 0.5).sum()))

    # ---- several LDS tiles in z and y
    tl = vol_tiles(rng)
    norm, m, mask, mm = record_norm(ref, out, meta, "tiles", tl)
    record_morph(out, meta, "tiles", norm > 0.02)
    out["tiles/morph_input"] = np.packbits(norm > 0.02)
    vc = mm["voxel_counts"]
    check(meta, "tiles", "largest_component_drops", vc["after_closing"] - vc["after_largest_component"])
    check(meta, "tiles", "closing_changes", int((closed(norm > 0.02, 5) != (norm > 0.02)).sum()))
    check(meta, "tiles", "tiles_z", -(-tl.shape[0] // 8) - 1)
    check(meta, "tiles", "tiles_y", -(-tl.shape[1] // 8) - 1)

    # ---- calculate_voxel_thresholds
    meta["voxel_thresholds"] = [
        {"spacing": sp, "volumes": vols, "result": jsonable(ref.calculate_voxel_thresholds(sp, vols))}
        for sp, vols in (([4.0, 4.0, 4.0], [0.5, 0.1]), ([2.0364, 2.0364, 3.0], [0.5, 0.1]),
                         ((4.0728, 4.0728, 3.0), [1, 0.25, 2.5]))]

    out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    path = os.path.join(OUT, "preprocess.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    for k in meta:
        if isinstance(meta[k], dict) and "checks" in meta[k]:
            print(" ", k, meta[k]["shape"], meta[k]["checks"])
    assert size < 1 << 20, size


if __name__ == "__main__":
    main()
