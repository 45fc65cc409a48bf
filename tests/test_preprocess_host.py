"""The host side of case preprocessing (light_unet/preprocess.py, l3u_plugin.bind_preprocess) and
the fixture's own discriminating conditions; no GPU."""
import json
import types

import numpy as np
import pytest


@pytest.fixture(scope="module")
def meta(golden):
    return json.loads(bytes(golden("preprocess.npz")["meta"]).decode())


def test_calculate_voxel_thresholds_matches_reference(meta):
    from light_unet import preprocess as PP
    assert len(meta["voxel_thresholds"]) >= 3
    for rec in meta["voxel_thresholds"]:
        assert PP.calculate_voxel_thresholds(rec["spacing"], rec["volumes"]) == rec["result"]


def test_bind_preprocess_returns_bound_names():
    import l3u_plugin
    mod = types.ModuleType("preprocess_data")
    names = l3u_plugin.bind_preprocess(mod)
    assert sorted(names) == ["calculate_voxel_thresholds", "clip_and_normalize", "generate_body_mask"]
    pre = l3u_plugin.load().preprocess
    for n in names:
        assert getattr(mod, n) is getattr(pre, n)
    assert mod.calculate_voxel_thresholds([4.0, 4.0, 4.0], [0.5])["0.5cc"]["voxel_count"] == 8


def test_fixture_still_discriminates(meta):
    """Every condition a case exists for was measured at generation time and is non-zero."""
    want = {"pet": ["zeros_above_half", "largest_component_drops", "tail_bits"],
            "const": ["empty_mask"], "range": ["reciprocal_multiply_differs", "negative_inputs"],
            "scale": ["fused_multiply_add_differs"], "intidx": ["n"],
            "plant": ["float32_compare_differs"], "tie": ["second_component_dropped"],
            "faces": ["outside1_erosion_differs"],
            "tiles": ["largest_component_drops", "closing_changes", "tiles_z", "tiles_y"]}
    want["pet"] += ["variant_differs_" + v for v in ("close0", "close2", "keepall", "dil0", "dil1",
                                                     "thr01")]
    for case, names in want.items():
        for n in names:
            assert meta[case]["checks"][n] > 0, (case, n)
    assert meta["intidx"]["checks"]["n"] == 8001
    for case, m in meta.items():
        if isinstance(m, dict) and "checks" in m:
            assert all(v > 0 for v in m["checks"].values()), case


def test_percentile_interpolation_matches_numpy():
    """np.percentile from two order statistics: ranks, weight and numpy's two-sided lerp."""
    from light_unet import preprocess as PP
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 7, 200, 201, 8001, 10007):
        a = rng.normal(size=n) if n % 2 else rng.normal(size=n).astype(np.float32).astype(np.float64)
        s = np.sort(a)
        for q in (0.0, 0.5, 1.0, 37.3, 50.0, 99.0, 99.5, 100.0):
            lo, hi, g = PP.percentile_ranks(n, q)
            got = PP.percentile_lerp(float(s[lo]), float(s[hi]), g)
            assert got == float(np.percentile(a, q)), (n, q)


def test_no_gpu_raises_native_error(monkeypatch):
    import torch
    from light_unet import _native, preprocess as PP
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_native.NativeError):
        PP.clip_and_normalize(np.zeros((2, 3, 4)))
    with pytest.raises(_native.NativeError):
        PP.generate_body_mask(np.zeros((2, 3, 4)), {})
