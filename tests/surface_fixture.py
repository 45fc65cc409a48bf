"""Readers of tests/golden/surface.npz (tests/golden/make_surface_goldens.py) shared by the host
and the device tests of the surface-distance metrics."""
import json
import math
import os

import numpy as np

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "surface.npz")
_CACHE = {}


def load():
    """(npz, index): loaded once per session and never modified."""
    if not _CACHE:
        z = np.load(_PATH, allow_pickle=False)
        _CACHE["z"] = z
        _CACHE["index"] = json.loads(bytes(z["index"]).decode())
    return _CACHE["z"], _CACHE["index"]


def mask(name, shape):
    z, _ = load()
    n = int(np.prod(shape))
    return np.unpackbits(z[name])[:n].reshape(shape).astype(bool)


def unhex(d):
    out = {}
    for k, v in d.items():
        if isinstance(v, list):
            out[k] = [float.fromhex(x) for x in v]
        else:
            out[k] = float.fromhex(v) if isinstance(v, str) else v
    return out


def same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def close_sum(a, b):
    """assd: numpy sums pairwise, the device in its fixed order; either is within n * 2^-53
    <= 2.9e-11 (n <= 2^18 surface voxels) of the exact sum of positive terms."""
    if math.isinf(b) or math.isnan(b) or b == 0.0:
        return same_float(a, b)
    return abs(a - b) <= 1e-10 * abs(b)


def check_metrics(got, exp):
    assert set(got) == {"hd", "hd95", "assd", "nsd", "n_pred", "n_target"}, got
    for k in ("hd", "hd95", "n_pred", "n_target"):
        assert got[k] == exp[k], (k, got[k], exp[k])
    assert list(got["nsd"]) == list(exp["nsd"]), (got["nsd"], exp["nsd"])
    print("assd", got["assd"], exp["assd"])
    assert close_sum(got["assd"], exp["assd"]), (got["assd"], exp["assd"])


SWEEP_KEYS = ("hd95_mean", "assd_mean", "nsd_mean", "surface_cases")


def check_sweep(got, exp):
    assert same_float(got["hd95_mean"], exp["hd95_mean"]), (got["hd95_mean"], exp["hd95_mean"])
    assert len(got["nsd_mean"]) == len(exp["nsd_mean"])
    for a, b in zip(got["nsd_mean"], exp["nsd_mean"]):
        assert same_float(a, b), (a, b)
    assert got["surface_cases"] == exp["surface_cases"]
    print("assd_mean", got["assd_mean"], exp["assd_mean"])
    assert close_sum(got["assd_mean"], exp["assd_mean"]), (got["assd_mean"], exp["assd_mean"])
