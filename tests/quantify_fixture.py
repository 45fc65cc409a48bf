"""Readers of tests/golden/quantify.npz (tests/golden/make_quantify_goldens.py) shared by the host
and the device tests of the lesion uptake report."""
import json
import os

import numpy as np

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantify.npz")
_CACHE = {}

EXACT_LESION_KEYS = ("label", "voxels", "volume_ml", "suv_max", "suv_max_voxel", "suv_peak",
                     "suv_peak_voxel", "centroid_mm")
EXACT_CASE_KEYS = ("n_lesions", "tmtv_ml", "suv_max", "suv_peak", "dmax_mm", "dmax_voxels",
                   "dmax_centroid_mm")
LESION_KEYS = set(EXACT_LESION_KEYS) | {"suv_mean", "tlg"}
CASE_KEYS = set(EXACT_CASE_KEYS) | {"lesions", "tlg_total"}


def load():
    """(npz, index): loaded once per session and never modified."""
    if not _CACHE:
        z = np.load(_PATH, allow_pickle=False)
        _CACHE["z"] = z
        _CACHE["index"] = json.loads(bytes(z["index"]).decode())
    return _CACHE["z"], _CACHE["index"]


def entries():
    return load()[1]["entries"]


def bits(name, shape):
    z, _ = load()
    return np.unpackbits(z[name])[:int(np.prod(shape))].reshape(shape).astype(bool)


def mask(entry):
    return bits("mask_" + entry["mask"], tuple(entry["shape"]))


def uptake(entry):
    """The float32 volume; quantised ones are stored as int32 multiples of 2^-10."""
    key = ("up", entry["uptake"])
    if key not in _CACHE:
        z, _ = load()
        if "upq_" + entry["uptake"] in z.files:
            v = (z["upq_" + entry["uptake"]].astype(np.float64) / 1024.0).astype(np.float32)
        else:
            v = z["up_" + entry["uptake"]]
        _CACHE[key] = v
    return _CACHE[key]


def unhex(v):
    if isinstance(v, dict):
        if set(v) == {"f"}:
            return float.fromhex(v["f"])
        return {k: unhex(x) for k, x in v.items()}
    if isinstance(v, list):
        return [unhex(x) for x in v]
    return v


def check_report(got, entry):
    """The report against the entry's expected dict: everything `==` but the float64 sums of the
    unquantised family, |suv_mean * voxels - fsum| <= voxels * 2^-53 * sum |v|: the bound of
    any-order recursive summation against the exact sum (fsum and sum |v| are in the golden)."""
    exp, sums, sum_abs = unhex(entry["expected"]), unhex(entry["sum"]), unhex(entry["sum_abs"])
    assert set(got) == CASE_KEYS, sorted(got)
    for k in EXACT_CASE_KEYS:
        assert got[k] == exp[k], (entry["name"], k, got[k], exp[k])
    assert len(got["lesions"]) == len(exp["lesions"]) == got["n_lesions"]
    for g, e, fs, sa in zip(got["lesions"], exp["lesions"], sums, sum_abs):
        assert set(g) == LESION_KEYS, sorted(g)
        for k in EXACT_LESION_KEYS:
            assert g[k] == e[k], (entry["name"], e["label"], k, g[k], e[k])
        if entry["family"] == "a":
            assert g["suv_mean"] == e["suv_mean"] and g["tlg"] == e["tlg"], (entry["name"], g, e)
        else:
            n = e["voxels"]
            err = abs(g["suv_mean"] * n - fs)
            bound = n * 2.0 ** -53 * sa
            print(entry["name"], e["label"], "suv_mean", g["suv_mean"], e["suv_mean"], err, bound)
            assert err <= bound, (entry["name"], e["label"], g["suv_mean"], e["suv_mean"], err, bound)
            assert g["tlg"] == g["suv_mean"] * g["volume_ml"]
    if entry["family"] == "a":
        assert got["tlg_total"] == exp["tlg_total"], (entry["name"], got["tlg_total"], exp["tlg_total"])
    else:
        assert got["tlg_total"] == float(sum(g["tlg"] for g in got["lesions"]))
