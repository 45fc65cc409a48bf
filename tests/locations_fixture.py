"""Reader of tests/golden/locations.npz (made by tests/golden/make_location_goldens.py from the
reference's own PatchDataset) and the numpy restatement of _sample_locations on voxel counts.
Shared by tests/test_locations_host.py (CPU) and tests/test_locations_gpu.py."""
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "locations.npz")


def load():
    z = np.load(PATH, allow_pickle=False)
    return z, json.loads(z["meta"].tobytes().decode())


def cases(z, meta):
    """[(label float32, body bool or None)] in dataset order."""
    out = []
    for cid, has in zip(meta["case_ids"], meta["has_body"]):
        out.append((z[f"case/{cid}/label"].astype(np.float32),
                    z[f"case/{cid}/body"].astype(bool) if has else None))
    return out


def rows(locs):
    """A list [(case, zyx)] as an int64 [n, 4] array."""
    return np.array([[c, *map(int, zyx)] for c, zyx in locs], np.int64).reshape(-1, 4)


def class_masks(label, body):
    """The reference's two predicates (patch_dataset.py:82, :89-92)."""
    bg = (label == 0) & body if body is not None else label == 0
    return label > 0, bg


def counts(labels_bodies):
    return np.array([[int(m.sum()) for m in class_masks(l, b)] for l, b in labels_bodies],
                    np.int64).reshape(-1, 2)


def rows_of_ranks(labels_bodies, ranks):
    """The ranks mapped through np.argwhere: int64 [n, 4] lesion and background rows."""
    out = ([], [])
    for ci, ((lab, body), pair) in enumerate(zip(labels_bodies, ranks)):
        for c, m in enumerate(class_masks(lab, body)):
            coords = np.argwhere(m)
            out[c].extend([ci, *coords[i]] for i in pair[c])
    return tuple(np.array(o, np.int64).reshape(-1, 4) for o in out)


def np_state_matches(keys, misc):
    """The global numpy generator's state equals the recorded (keys, [pos, has_gauss, cached])."""
    _, k, pos, has_g, cached = np.random.get_state()
    return (np.array_equal(k, keys) and int(pos) == int(misc[0]) and int(has_g) == int(misc[1])
            and (not has_g or float(cached) == float(misc[2])))
