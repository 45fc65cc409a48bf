"""Surface-distance metrics, the parts that need no GPU: argument errors are raised before any
device access, the golden file agrees with an independent numpy-only evaluation, the percentile's
end points, and the C header."""
import os
import re

import numpy as np
import pytest

import surface_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def no_device(monkeypatch):
    """Any device access of the module under test fails the test (also where a GPU is present)."""
    from light_unet import _native, surface

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(surface, "_device", boom)
    monkeypatch.setattr(_native, "call", boom)
    monkeypatch.setattr(_native, "query", boom)
    return surface


def test_argument_errors_come_before_the_device(no_device):
    surface = no_device
    a = np.zeros((4, 5, 6), np.uint8)
    with pytest.raises(ValueError, match="differ in shape"):
        surface.surface_distances(a, np.zeros((4, 5, 7), np.uint8))
    with pytest.raises(ValueError, match=r"\[D, H, W\]"):
        surface.surface_distances(np.zeros((5, 6), np.uint8), np.zeros((5, 6), np.uint8))
    with pytest.raises(ValueError, match=r"\[D, H, W\]"):
        surface.surface_distances(np.zeros((1, 4, 5, 6), np.uint8), np.zeros((1, 4, 5, 6), np.uint8))
    with pytest.raises(ValueError, match=r"\[D, H, W\]"):
        surface.surface_distances(np.zeros((0, 5, 6), np.uint8), np.zeros((0, 5, 6), np.uint8))
    for bad in ((4.0, 0.0, 4.0), (4.0, -1.0, 4.0), (4.0, 4.0), (4.0, float("nan"), 4.0)):
        with pytest.raises(ValueError, match="spacing"):
            surface.surface_distances(a, a, spacing=bad)
    with pytest.raises(ValueError, match="at most 8 tolerances"):
        surface.surface_distances(a, a, tolerances_mm=[1.0] * 9)
    for q in (-0.5, 100.5):
        with pytest.raises(ValueError, match="range"):
            surface.surface_distances(a, a, percentile=q)
    # the other entry points
    with pytest.raises(ValueError, match=r"\[D, H, W\]"):
        surface.distance_transform_edt(np.zeros((5, 6)))
    with pytest.raises(ValueError, match="sampling"):
        surface.distance_transform_edt(a, sampling=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="output"):
        surface.distance_transform_edt(a, output="host")
    with pytest.raises(ValueError, match=r"\[D, H, W\]"):
        surface.surface_mask(np.zeros((6,), np.uint8))
    p = np.zeros((4, 5, 6), np.float32)
    with pytest.raises(ValueError, match="differ in shape"):
        surface.case_surface_metrics(p, np.zeros((4, 5, 5), np.float32), [0.5])
    with pytest.raises(ValueError, match="differ in shape"):
        surface.case_surface_metrics(p, p, [0.5], body_mask=np.ones((4, 5, 5), np.float32))
    with pytest.raises(ValueError, match="at most 8 tolerances"):
        surface.case_surface_metrics(p, p, [0.5], tolerances_mm=range(9))
    with pytest.raises(ValueError, match="range"):
        surface.case_surface_metrics(p, p, [0.5], percentile=101)
    with pytest.raises(ValueError, match="spacing"):
        surface.case_surface_metrics(p, p, [0.5], spacing=(0, 1, 1))


def test_sweep_metrics_checks_the_surface_argument_first(no_device):
    from light_unet import lesion
    p = [np.zeros((4, 5, 6), np.float32)]
    with pytest.raises(ValueError, match="at most 8 tolerances"):
        lesion.sweep_metrics(p, p, [0.5], surface={"tolerances_mm": [1.0] * 9})
    with pytest.raises(ValueError, match="range"):
        lesion.sweep_metrics(p, p, [0.5], surface={"tolerances_mm": [4.0], "percentile": 120})
    with pytest.raises(ValueError, match="unknown keys"):
        lesion.sweep_metrics(p, p, [0.5], surface={"tolerance": [4.0]})
    with pytest.raises(ValueError, match="dict"):
        lesion.sweep_metrics(p, p, [0.5], surface=[4.0])


# ---------------------------------------------------------------- numpy only, O(n^2)
def _erode6(a):
    p = np.pad(a, 1)
    c = p[1:-1, 1:-1, 1:-1]
    return (c & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1]
            & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])


def _directed(src, dst, spacing):
    """Per voxel of `src` the distance to the nearest voxel of `dst`: all pairs."""
    a, b = np.argwhere(src), np.argwhere(dst)
    d = (a[:, None, :] - b[None, :, :]).astype(np.float64) * np.asarray(spacing, np.float64)
    d = d * d
    return np.sqrt(((d[..., 0] + d[..., 1]) + d[..., 2]).min(axis=1))


def _metrics(pred, target, spacing, tolerances, q):
    sp, st = pred & ~_erode6(pred), target & ~_erode6(target)
    d_pt, d_tp = _directed(sp, st, spacing), _directed(st, sp, spacing)
    n = len(d_pt) + len(d_tp)
    return sp, st, {"hd": float(max(d_pt.max(), d_tp.max())),
                    "hd95": float(max(np.percentile(d_pt, q), np.percentile(d_tp, q))),
                    "assd": float((d_pt.sum() + d_tp.sum()) / n),
                    "nsd": [(int((d_pt <= t).sum()) + int((d_tp <= t).sum())) / n for t in tolerances],
                    "n_pred": len(d_pt), "n_target": len(d_tp)}


def test_golden_file_is_self_consistent():
    _, index = fx.load()
    crops = [m for m in index["metrics"] if m["tag"] == "crop"]
    assert len(crops) == 4 and tuple(crops[0]["shape"]) == (12, 14, 18)
    shape = (12, 14, 18)
    pred, target = fx.mask("m_crop_pred", shape), fx.mask("m_crop_target", shape)
    for m in crops:
        sp, st, got = _metrics(pred, target, m["spacing"], m["tolerances"], m["percentile"])
        assert np.array_equal(sp, fx.mask("m_crop_spred", shape))
        assert np.array_equal(st, fx.mask("m_crop_starget", shape))
        assert got["n_pred"] > 0 and got["n_target"] > 0
        fx.check_metrics(got, fx.unhex(m["expected"]))
    # the crop is cut out of the stored full-size pair
    full_p, full_t = fx.mask("m_a_pred", (40, 52, 70)), fx.mask("m_a_target", (40, 52, 70))
    hits = [(z, y, x) for z in range(29) for y in range(39) for x in range(53)
            if full_p[z, y, x] == pred[0, 0, 0] and np.array_equal(full_p[z:z + 12, y:y + 14, x:x + 18], pred)
            and np.array_equal(full_t[z:z + 12, y:y + 14, x:x + 18], target)]
    assert hits
    # the conventions for empty surfaces
    for m in index["metrics"]:
        e = fx.unhex(m["expected"])
        if e["n_pred"] == 0 and e["n_target"] == 0:
            assert (e["hd"], e["hd95"], e["assd"], e["nsd"]) == (0.0, 0.0, 0.0, [1.0, 1.0])
        elif e["n_pred"] == 0 or e["n_target"] == 0:
            assert (e["hd"], e["hd95"], e["assd"], e["nsd"]) == (np.inf, np.inf, np.inf, [0.0, 0.0])
    equal = fx.unhex(next(m for m in index["metrics"] if m["tag"] == "equal")["expected"])
    assert (equal["hd"], equal["hd95"], equal["assd"], equal["nsd"]) == (0.0, 0.0, 0.0, [1.0, 1.0])


def test_sweep_golden_aggregates_its_cases():
    from light_unet import surface
    _, index = fx.load()
    s = index["sweep"]
    for k, exp in enumerate(s["expected"]):
        rows = [fx.unhex(c[k]) for c in s["per_case"]]
        fx.check_sweep(surface.aggregate(rows, len(s["tolerances"])), fx.unhex(exp))
    nan = surface.aggregate([{"hd": 0.0, "hd95": 0.0, "assd": 0.0, "nsd": [1.0], "n_pred": 0,
                              "n_target": 0}], 1)
    assert np.isnan(nan["hd95_mean"]) and np.isnan(nan["assd_mean"]) and np.isnan(nan["nsd_mean"][0])
    assert nan["surface_cases"] == 0


def test_percentile_end_points_are_min_and_max():
    from light_unet import preprocess as pp
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 1000):
        d = np.sort(rng.random(n) * 50.0)
        for q, want in ((0.0, d[0]), (100.0, d[-1])):
            lo, hi, g = pp.percentile_ranks(n, q)
            assert 0 <= lo <= hi < n
            got = pp.percentile_lerp(float(d[lo]), float(d[hi]), g)
            assert got == want == np.percentile(d, q)
        lo, hi, g = pp.percentile_ranks(n, 95.0)
        assert pp.percentile_lerp(float(d[lo]), float(d[hi]), g) == np.percentile(d, 95.0)


def test_header_declares_the_surface_exports():
    from light_unet import _native
    src = open(os.path.join(ROOT, "include", "l3u.h")).read()
    for name in ("l3u_edt", "l3u_surf_mask", "l3u_surf_nblocks", "l3u_surf_reduce"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _native.exported_symbols()
    assert re.search(r"#define\s+L3U_ABI_VERSION\s+5\b", src)
    assert _native.ABI_VERSION == 5 and _native.query("l3u_abi_version") == 5
    assert _native.query("l3u_surf_nblocks", 1) == 1
    assert _native.query("l3u_surf_nblocks", 4097) == 2
    assert _native.query("l3u_surf_nblocks", 1 << 31) == 0
