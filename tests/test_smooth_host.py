"""Host side of the Gaussian smoothing (light_unet/smooth.py: gaussian_filter): the numpy
transcription of the module's definition against scipy's outputs in tests/golden/smooth.npz (made
by tests/golden/make_smooth_goldens.py), the weight tables, fwhm_sigma, argument errors and the
declarations; no GPU.

Bounds: the definition fixes every float64 operation and its order, and reproduces scipy's
gaussian_filter bit for bit, so the outputs are compared with == on the bits.  The weight tables
go through np.exp, which another numpy build may round differently: one ulp per weight is allowed
there (== holds with the numpy the fixture was made with).
"""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_smooth_goldens as G   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("smooth.npz")
    return z, json.loads(bytes(z["meta"]).decode())


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def stored_tables(z, k):
    return [z[f"w/{k}/{a}"] if f"w/{k}/{a}" in z.files else None for a in range(3)]


def test_fixture_holds_what_the_issue_lists(fx):
    z, meta = fx
    assert os.path.getsize(G.OUT) < 1000000
    cases = [tuple(c) for c in meta["cases"]]
    assert cases == G.cases() and meta["cval"] == G.CVAL == 0.25
    assert {c[3] for c in cases} == set(G.MODES)                       # every mode
    assert {c[4] for c in cases} == {"f32", "f64"}                     # both dtypes
    assert {c[0] for c in cases} == set(G.SHAPES)
    assert {c[0] for c in cases if c[4] == "f64"} == set(G.SMALL)
    assert any(G.SIGMAS[c[2]][1] == 0.0 for c in cases)                # the zero sigma
    # radius 12 on the axis of length 1, and axes shorter than the radius
    assert G.radius_of(3.0) == 12 and G.SHAPES["a"][0] == 1 and ("a", "g", 3, "mirror", "f32") in cases
    assert G.radius_of(2.2) == 9 and G.SHAPES["b"][2] == 4
    ins = G.inputs()
    for c in cases:
        x, want = G.case_input(z, c), z[G.name(c)]
        assert x.shape == G.SHAPES[c[0]] == want.shape
        assert x.dtype == want.dtype == {"f32": np.float32, "f64": np.float64}[c[4]]
        assert np.array_equal(_bits(z[f"in/{c[0]}/{c[1]}"]), _bits(ins[c[0]][c[1]]))
        assert np.isfinite(want).all()


def test_transcription_equals_scipy_bit_for_bit(fx):
    z, meta = fx
    total = 0
    for c in G.cases():
        got = G.transcription(G.case_input(z, c), stored_tables(z, c[2]), c[3], G.CVAL)
        want = z[G.name(c)]
        assert got.dtype == want.dtype
        assert np.array_equal(_bits(got), _bits(want)), c
        total += want.size
    assert total == meta["voxels"]


def test_weights_equal_the_stored_tables(fx):
    from light_unet.smooth import gaussian_weights, weight_tables
    z, _ = fx
    for k, sig in enumerate(G.SIGMAS):
        got = weight_tables(sig)
        for a in range(3):
            if sig[a] == 0.0:
                assert got[a] is None and f"w/{k}/{a}" not in z.files
                continue
            want = z[f"w/{k}/{a}"]
            r = int(4.0 * sig[a] + 0.5)
            assert got[a].dtype == np.float64 and got[a].shape == want.shape == (2 * r + 1,)
            print(f"sigma {sig[a]}: {int((got[a] != want).sum())} of {want.size} weights differ")
            assert (np.abs(got[a] - want) <= np.spacing(want)).all()
            assert np.array_equal(got[a], got[a][::-1])                # symmetric bit for bit
            assert np.array_equal(got[a], G.weights(sig[a], r))        # the maker's, same machine
            assert np.array_equal(gaussian_weights(sig[a]), got[a])
    w = gaussian_weights(0.8, radius=7)
    assert w.shape == (15,) and np.array_equal(w, G.weights(0.8, 7))
    assert np.array_equal(gaussian_weights(2.0, truncate=2.5), G.weights(2.0, 5))
    assert np.array_equal(gaussian_weights(1.0, radius=0), np.ones(1))
    per_axis = weight_tables((1.0, 1.0, 1.0), radius=(2, None, 5))
    assert [len(w) for w in per_axis] == [5, 9, 11]
    assert weight_tables(0.0) == [None, None, None]
    assert len(gaussian_weights(16.0)) == 129                          # the cap itself


def test_fwhm_sigma_values():
    from light_unet.smooth import fwhm_sigma, smooth_record
    k = 2.0 * math.sqrt(2.0 * math.log(2.0))
    assert abs(k - 2.3548200450309493) < 1e-15
    assert fwhm_sigma(6.0, (4.0, 4.0, 4.0)) == (6.0 / k / 4.0,) * 3
    assert fwhm_sigma(7.0, (3.0, 2.04, 2.04)) == (7.0 / k / 3.0, 7.0 / k / 2.04, 7.0 / k / 2.04)
    assert fwhm_sigma((6.0, 0.0, 5.0), (4.0, 2.0, 1.0)) == (6.0 / k / 4.0, 0.0, 5.0 / k / 1.0)
    assert all(isinstance(v, float) for v in fwhm_sigma(np.float32(6.0), np.array([4, 4, 4])))
    # the benchmark's two sizes: radii 3 at 4 mm, (4, 6, 6) at (3, 2.04, 2.04) mm
    assert smooth_record(6.0, (4.0, 4.0, 4.0))["radius"] == [3, 3, 3]
    assert smooth_record(7.0, (3.0, 2.04, 2.04))["radius"] == [4, 6, 6]
    rec = smooth_record((6.0, 0.0, 6.0), (4.0, 4.0, 4.0))
    assert rec == {"fwhm_mm": [6.0, 0.0, 6.0], "radius": [3, 0, 3],
                   "sigma_voxels": [6.0 / k / 4.0, 0.0, 6.0 / k / 4.0]}
    for bad in (-1.0, float("nan"), float("inf"), (6.0, 6.0), "x"):
        with pytest.raises(ValueError):
            fwhm_sigma(bad, (4.0, 4.0, 4.0))
    for bad in ((4.0, 4.0), (4.0, 0.0, 4.0), (4.0, -1.0, 4.0), 4.0, None):
        with pytest.raises(ValueError):
            fwhm_sigma(6.0, bad)


def test_argument_errors_come_before_the_device(monkeypatch):
    """Mode, dtype, rank, sigma, radius and output errors are ValueErrors with or without a GPU; a
    valid call without one raises NativeError (there is no CPU fallback)."""
    import torch
    from light_unet import _native, inference, quantify, resegment, smooth
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    vol = np.zeros((3, 4, 5), np.float32)
    for mode in ("wrap", "grid-wrap", "grid-mirror", "grid-constant", "edge", None):
        with pytest.raises(ValueError):
            smooth.gaussian_filter(vol, 1.0, mode=mode)
    for dt in (np.int16, np.int32, np.int64, np.float16, np.uint16, np.uint8, bool):
        with pytest.raises(ValueError):
            smooth.gaussian_filter(np.zeros((3, 4, 5), dt), 1.0)
    for dt in (torch.uint8, torch.bool, torch.int64, torch.float16, torch.bfloat16):
        with pytest.raises(ValueError):
            smooth.gaussian_filter(torch.zeros(3, 4, 5, dtype=dt), 1.0)
    for bad in (np.zeros((4, 5), np.float32), np.zeros((1, 3, 4, 5), np.float32),
                np.zeros((0, 4, 5), np.float32), torch.zeros(2, 3)):
        with pytest.raises(ValueError):
            smooth.gaussian_filter(bad, 1.0)
    for sigma in (-1.0, (1.0, 1.0), (1.0, 1.0, 1.0, 1.0), float("nan"), float("inf"), "s"):
        with pytest.raises(ValueError):
            smooth.gaussian_filter(vol, sigma)
    assert smooth.MAX_RADIUS == 64
    with pytest.raises(ValueError):
        smooth.gaussian_filter(vol, 16.2)                       # int(4 * 16.2 + 0.5) = 65
    with pytest.raises(ValueError):
        smooth.gaussian_filter(vol, 1.0, radius=65)
    with pytest.raises(ValueError):
        smooth.gaussian_filter(vol, (1.0, 0.5, 1.0), radius=(2, 2, 65))
    for radius in (-1, 1.5, (1, 2), True):
        with pytest.raises(ValueError):
            smooth.gaussian_filter(vol, 1.0, radius=radius)
    for truncate in (0.0, -4.0, float("nan")):
        with pytest.raises(ValueError):
            smooth.gaussian_filter(vol, 1.0, truncate=truncate)
    with pytest.raises(ValueError):
        smooth.gaussian_filter(vol, 1.0, output="cpu")
    with pytest.raises(TypeError):
        smooth.gaussian_filter(vol, 1.0, path="fused")          # the fused path was not kept
    with pytest.raises(ValueError):
        smooth.gaussian_weights(0.0)
    w = smooth.gaussian_weights(1.0)
    for tables in ([w, w], [w, w[:-1], w], [w, w[:-2] * 1.0, np.arange(5.0)], [np.ones(131), w, w],
                   [w.reshape(1, -1), w, w]):
        with pytest.raises(ValueError):
            smooth._filter_weights(vol, tables)
    # the consumers check the filter's arguments first as well
    mask = np.zeros((3, 4, 5), np.float32)
    for bad in (-6.0, (6.0, 6.0), float("nan"), 700.0):         # 700 mm at 4 mm: radius 297
        with pytest.raises(ValueError):
            quantify.lesion_uptake(vol, mask, smooth_fwhm_mm=bad)
        with pytest.raises(ValueError):
            resegment.resegment_lesions(vol, mask, smooth_fwhm_mm=bad)
    with pytest.raises(ValueError):
        inference.infer_volume(vol, None, {}, smooth_fwhm_mm=6.0)                   # no uptake
    with pytest.raises(ValueError):
        inference.infer_volume(vol, None, {}, uptake=vol, smooth_fwhm_mm=-6.0)
    for call in (lambda: smooth.gaussian_filter(vol, 1.0),
                 lambda: smooth.gaussian_filter(vol.astype(np.float64), (1.0, 0.0, 2.0), mode="constant",
                                                cval=0.25),
                 lambda: smooth.smooth_fwhm(vol, (4.0, 4.0, 4.0), 6.0),
                 lambda: smooth._filter_weights(vol, [w, None, w]),
                 lambda: quantify.lesion_uptake(vol, mask, smooth_fwhm_mm=6.0)):
        with pytest.raises(_native.NativeError):
            call()


def test_consumers_take_the_option_as_a_keyword_stage_in_front():
    """smooth_fwhm_mm is keyword only, taken by smooth.takes_smooth_fwhm before the consumer runs:
    the consumers' own parameter lists are what they were."""
    from light_unet import quantify, resegment, smooth
    vol = np.zeros((3, 4, 5), np.float32)
    for fn in (quantify.lesion_uptake, resegment.resegment_lesions):
        assert "smooth_fwhm_mm" in fn.__doc__ and callable(fn.__wrapped__)
        with pytest.raises(TypeError):
            fn(vol, vol, (4.0, 4.0, 4.0), None, None, None, None, None, None, None, 6.0)
    seen = []

    @smooth.takes_smooth_fwhm
    def consumer(uptake, mask, spacing=(4.0, 4.0, 4.0), extra=1):
        seen.append((uptake, mask, spacing, extra))
        return {}

    assert consumer(vol, "m", extra=2) == {} and seen[-1][0] is vol and seen[-1][1:] == ("m", (4.0, 4.0, 4.0), 2)
    assert consumer(vol, "m", (2.0, 2.0, 2.0), smooth_fwhm_mm=None) == {} and seen[-1][0] is vol
    for bad in (np.zeros((4, 5), np.float32), np.zeros((0, 4, 5), np.float32)):
        with pytest.raises(ValueError):
            consumer(bad, "m", smooth_fwhm_mm=6.0)
    with pytest.raises(ValueError):
        consumer(vol, "m", (4.0, 0.0, 4.0), smooth_fwhm_mm=6.0)
    assert len(seen) == 2


def test_exports_are_declared_and_bound():
    from light_unet import _native, smooth
    with open(os.path.join(ROOT, "include", "l3u.h")) as f:
        header = f.read()
    assert "int l3u_gauss_axis(" in header and "int l3u_gauss_max_radius(void);" in header
    assert "#define L3U_ABI_VERSION 5" in header and _native.ABI_VERSION == 5
    assert len(_native._SIGS["l3u_gauss_axis"]) == 12 and _native._SIGS["l3u_gauss_max_radius"] == []
    assert _native._SIGS["l3u_gauss_axis"][7:11] == [_native.P, _native.I, _native.I, _native.D]
    lib = _native.load()
    for name in ("l3u_gauss_axis", "l3u_gauss_max_radius"):
        assert hasattr(lib, name)
    assert _native.query("l3u_gauss_max_radius") == smooth.MAX_RADIUS
    assert "l3u_gauss3" not in header and not hasattr(lib, "l3u_gauss3")    # measured, not kept
    with open(os.path.join(ROOT, "light-3d-unet-front_amd", "Makefile")) as f:
        assert "build/smooth.o: FLAGS += -ffp-contract=off" in f.read()
    assert smooth.MODES == {m: i for i, m in enumerate(G.MODES)}
