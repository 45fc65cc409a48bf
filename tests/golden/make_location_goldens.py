"""Golden fixture for the patch-location sampling, made by the REFERENCE's own code
(PatchDataset.__init__ / _sample_locations / _load_body_mask_array, patch_dataset.py:17-109).

Run where the reference tree exists (L3U_REFERENCE, default /root/reference) with
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_location_goldens.py
Like make_loop_goldens.py it imports the reference package itself, unmodified, by path, with one
stand-in for a module that is absent from this image and only does I/O around the path:
`nibabel`, whose `load(path).get_fdata()` returns the float64 array of a .npy payload.

It writes small synthetic cases under the reference's layout, WITH body-mask files
(body_masks/<id>.nii.gz), builds the reference's PatchDataset on them (CPU) and records in
tests/golden/locations.npz, as data only:
  * the cases' labels and body masks (uint8; `case/<id>/label`, `case/<id>/body`, the latter
    absent for the case without a mask file);
  * the seed, and the dataset's lesion_locations / background_locations as int32 [n, 4] rows
    (case index, z, y, x) in list order;
  * the global numpy generator's state right after construction (`rng_after/np_keys`,
    `rng_after/np_misc` = pos, has_gauss, cached_gaussian).
The cases pin both branches that skip a randint call by the reference itself: one case has no
lesion voxel, one has a body mask that excludes every label-0 voxel.  Two cases are large enough
for n // 1000 > 10 lesion and n // 5000 > 10 background samples; one has no mask file.
The JSON part is stored as a uint8 array `meta`.
"""
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True

import numpy as np

REF = os.environ.get("L3U_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 11
PATCH = (16, 16, 16)
# id -> (shape, kind)
CASES = {"0001": ((40, 36, 44), "plain"),        # two small lesions, ellipsoid body
         "0002": ((48, 48, 48), "big"),          # > 11000 lesion voxels, > 55000 background voxels
         "0003": ((20, 24, 28), "no_lesion"),    # no randint call for the lesion class
         "0004": ((24, 20, 28), "no_background"),  # body excludes every label-0 voxel
         "0005": ((17, 19, 23), "no_mask_file")}  # body_mask_path is None


class _Img:
    def __init__(self, a):
        self._a = a

    def get_fdata(self):
        return np.asarray(self._a, dtype=np.float64)


def _install_stubs():
    nib = types.ModuleType("nibabel")
    nib.load = lambda path: _Img(np.load(str(path), allow_pickle=False))
    sys.modules["nibabel"] = nib


def _ball(shape, c, r):
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    return (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r


def make_cases():
    """{id: (label uint8, body uint8 or None)}."""
    rng = np.random.default_rng(314)
    out = {}
    for cid, (shape, kind) in CASES.items():
        lab = np.zeros(shape, np.uint8)
        if kind == "big":
            lab[_ball(shape, [s // 2 for s in shape], 14.5)] = 1
        elif kind != "no_lesion":
            for v in (1, 2):
                c = [int(rng.integers(5, s - 5)) for s in shape]
                lab[_ball(shape, c, float(rng.uniform(2.5, 4.5)))] = v
        half = [s / 2 for s in shape]
        zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
        body = (((zz - half[0]) / (0.55 * shape[0])) ** 2 + ((yy - half[1]) / (0.5 * shape[1])) ** 2 +
                ((xx - half[2]) / (0.5 * shape[2])) ** 2 <= 1.0).astype(np.uint8)
        if kind == "big":                        # a box: everything but a 2-voxel border
            body = np.zeros(shape, np.uint8)
            body[2:-2, 2:-2, 2:-2] = 1
        if kind == "no_background":
            body = (lab > 0).astype(np.uint8)
        if kind == "no_mask_file":
            body = None
        out[cid] = (lab, body)
    return out


def _write(root, cases):
    for sub in ("images", "labels", "body_masks"):
        os.makedirs(os.path.join(root, "data", sub))
    for cid, (lab, body) in cases.items():
        files = [("images", f"{cid}_0000.nii.gz", np.zeros(lab.shape, np.float32)),
                 ("labels", f"{cid}.nii.gz", lab)]
        if body is not None:
            files.append(("body_masks", f"{cid}.nii.gz", body))
        for sub, name, arr in files:
            with open(os.path.join(root, "data", sub, name), "wb") as f:
                np.save(f, arr)
    split = os.path.join(root, "train_list.txt")
    with open(split, "w") as f:
        f.write("\n".join(cases) + "\n")
    return os.path.join(root, "data"), split


def _rows(locs):
    return np.array([[ci, *map(int, c)] for ci, c in locs], np.int32).reshape(-1, 4)


def main():
    _install_stubs()
    sys.path.insert(0, REF)
    from light_unet.datasets.patch_dataset import PatchDataset

    cases = make_cases()
    out, meta = {}, {"case_ids": list(cases), "seed": SEED, "patch": list(PATCH)}
    with tempfile.TemporaryDirectory() as root:
        data_dir, split = _write(root, cases)
        ds = PatchDataset(data_dir, split, patch_size=PATCH, lesion_patch_ratio=0.5, augmentation=None,
                          seed=SEED,
                          body_mask_config={"enabled": True, "apply_to_training_sampling": False})
        _, keys, pos, has_g, cached = np.random.get_state()
        assert [c["case_id"] for c in ds.cases] == list(cases)
        meta["has_body"] = [c["body_mask_path"] is not None for c in ds.cases]
    for cid, (lab, body) in cases.items():
        out[f"case/{cid}/label"] = lab
        if body is not None:
            out[f"case/{cid}/body"] = body
    out["lesion"] = _rows(ds.lesion_locations)
    out["background"] = _rows(ds.background_locations)
    out["rng_after/np_keys"] = np.asarray(keys, np.uint32)
    out["rng_after/np_misc"] = np.array([pos, has_g, cached], np.float64)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    path = os.path.join(OUT, "locations.npz")
    np.savez_compressed(path, **out)
    per_case = [(int((out["lesion"][:, 0] == k).sum()), int((out["background"][:, 0] == k).sum()))
                for k in range(len(cases))]
    print("rows per case (lesion, background):", per_case)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
