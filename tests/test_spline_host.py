"""Host side of the cubic B-spline resampling (light_unet/resample.py: resample_spline): the golden
fixture against its generator, the numpy transcription of the module's definition against scipy's
outputs in the fixture, the per-axis tables, argument errors and the declarations; no GPU.

Bounds: the definition is the project's own (scipy's boundary initialisation and rounding order
differ in the last bits of float64), so a float32 result may land on the other side of a rounding
boundary: every voxel within one float32 ulp of scipy's, at most 1 voxel in 10 000 per case
differing.  The transcription alone gives 0 of every case's voxels, which the fixture records and
this file asserts as well.
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_spline_goldens as G   # noqa: E402


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("spline.npz")
    return z, json.loads(bytes(z["meta"]).decode())


def source(z, golden, k, m):
    """The float32 input of case k, image m: stored here, in resample.npz (the uniform images of
    the order-1 cases), or case a's output (g, the way back)."""
    if k == "g":
        return z[f"a/{m}/s32"]
    if (k, m) in G.stored_inputs():
        return z[f"{k}/{m}"]
    return golden("resample.npz")[f"{k}/image"]


def test_golden_file_is_what_the_generator_makes(fx, golden):
    """The fixture's inputs are the generator's seeded inputs; with scipy importable the whole
    file is regenerated and compared array by array (scipy's zoom is what the goldens are)."""
    z, meta = fx
    assert set(meta["cases"]) == set(G.CASES) == set("abcdefghi")
    assert os.path.getsize(G.OUT) < os.path.getsize(os.path.join(os.path.dirname(G.OUT), "resample.npz"))
    ins = G.inputs()
    for k, (shape, out_shape) in G.CASES.items():
        for m in G.IMAGES:
            img = source(z, golden, k, m)
            assert img.dtype == np.float32 and img.shape == tuple(shape), (k, m)
            if k != "g":
                assert np.array_equal(img.view(np.uint32), ins[k][m].view(np.uint32)), (k, m)
            assert z[f"{k}/{m}/s32"].shape == tuple(out_shape) and z[f"{k}/{m}/s32"].dtype == np.float32
            assert z[f"{k}/{m}/d64"].shape == tuple(out_shape) and z[f"{k}/{m}/d64"].dtype == np.int8
    try:
        import scipy.ndimage  # noqa: F401
    except ImportError:
        return
    again = G.build()
    assert set(again) == set(z.files)
    for name in z.files:
        assert again[name].dtype == z[name].dtype and np.array_equal(again[name], z[name]), name


@pytest.mark.parametrize("k", sorted(G.CASES))
def test_definition_in_numpy_against_scipy(fx, golden, k):
    z, meta = fx
    out_shape = G.CASES[k][1]
    for m in G.IMAGES:
        img = source(z, golden, k, m)
        got = G.transcription(img, out_shape)
        assert np.array_equal(got, G.transcription(img.astype(np.float64), out_shape))
        for name, want in (("s32", z[f"{k}/{m}/s32"]), ("s64", G.scipy64(z, k, m))):
            differing = int((got != want).sum())
            print(f"case {k}/{m}/{name}: {differing} of {want.size} float32 voxels differ from scipy")
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
            assert differing * 10000 <= want.size
            assert differing == meta["cases"][k][m][f"transcription_differs_{name}"] == 0
        assert meta["cases"][k][m]["raw_float64_difference_over_max"] < 1e-13


def test_identity_case_is_the_source(fx, golden):
    z, _ = fx
    for m in G.IMAGES:
        img = source(z, golden, "f", m)
        assert np.array_equal(z[f"f/{m}/s32"].view(np.uint32), img.view(np.uint32))
        assert np.array_equal(G.transcription(img, img.shape).view(np.uint32), img.view(np.uint32))
        assert not z[f"f/{m}/d64"].any()


def test_module_tables_and_constants_are_the_transcriptions():
    from light_unet import resample as RS
    assert RS.spline_constants() == G.constants() and RS.SPLINE_PAD == G.NP == 12
    z, lam, k0, kn = RS.spline_constants()
    assert -0.27 < z < -0.26 and abs(lam - 6.0) < 1e-14 and 0 < k0 < 1 and 0 < kn < 1
    for shape, out_shape in G.CASES.values():
        for n_in, n_out in zip(shape, out_shape):
            start, w = RS.spline_axis_table(n_in, n_out)
            gs, gw = G.axis_table(n_in, n_out)
            assert start.dtype == np.int32 and w.dtype == np.float64 and w.shape == (n_out, 4)
            assert np.array_equal(start, gs) and np.array_equal(w.view(np.uint64), gw.view(np.uint64))


@pytest.mark.parametrize("n_in,n_out", sorted({p for s, o in G.CASES.values() for p in zip(s, o)}
                                              | {(400, 204), (204, 400), (600, 450), (450, 600)}))
def test_axis_table(n_in, n_out):
    """No tap reads the outer pad (start >= 10, start + 3 <= n_in + 13); the four weights sum to 1
    within 2 ulp and are non-negative within 1e-16."""
    from light_unet.resample import spline_axis_table
    start, w = spline_axis_table(n_in, n_out)
    assert start.min() >= 10 and start.max() + 3 <= n_in + 13
    assert (np.abs(w.sum(axis=1) - 1.0) <= 2 * np.spacing(1.0)).all()
    assert w.min() >= -1e-16 and w.max() <= 4.0 / 6.0 + 1e-16
    if n_in == n_out:
        assert np.array_equal(start, np.arange(n_in) + 11)
        assert (w[:, :3] == np.array([1.0 / 6.0, 4.0 / 6.0, 1.0 / 6.0])).all() and (np.abs(w[:, 3]) < 1e-16).all()


def test_argument_errors_come_before_the_device(monkeypatch):
    """Rank, dtype, shape, clip and coefficient errors are ValueErrors with or without a GPU; a
    valid call without one raises NativeError (there is no CPU fallback)."""
    import torch
    from light_unet import _native, preprocess as PP
    from light_unet.resample import resample_spline, resample_volume, spline_coefficients
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    vol = np.zeros((3, 4, 5), np.float32)
    for bad in (np.zeros((4, 5), np.float32), np.zeros((1, 3, 4, 5), np.float32),
                np.zeros((0, 4, 5), np.float32), torch.zeros(2, 3)):
        with pytest.raises(ValueError):
            resample_spline(bad, (2, 2, 2))
        with pytest.raises(ValueError):
            spline_coefficients(bad)
    for dt in (np.int16, np.int32, np.int64, np.float16, np.uint16, np.uint8, bool):
        with pytest.raises(ValueError):
            resample_spline(np.zeros((3, 4, 5), dt), (2, 2, 2))
        with pytest.raises(ValueError):
            spline_coefficients(np.zeros((3, 4, 5), dt))
    for dt in (torch.uint8, torch.bool, torch.int64, torch.float16, torch.bfloat16):
        with pytest.raises(ValueError):
            resample_spline(torch.zeros(3, 4, 5, dtype=dt), (2, 2, 2))
    with pytest.raises(ValueError):
        resample_spline(vol)                                        # neither a shape nor spacings
    with pytest.raises(ValueError):
        resample_spline(vol, spacing=(2.0, 2.0, 2.0))               # no target
    with pytest.raises(ValueError):
        resample_spline(vol, target_spacing=(4.0, 4.0, 4.0))        # no source spacing
    for bad_shape in ((2, 2), (2, 0, 2)):
        with pytest.raises(ValueError):
            resample_spline(vol, bad_shape)
    with pytest.raises(ValueError):
        resample_spline(vol, (2, 2, 2), output="cpu")
    with pytest.raises(ValueError):
        spline_coefficients(vol, output="cpu")
    for bad_clip in ((1.0,), (1.0, 0.0), (0.0, 1.0, 2.0)):
        with pytest.raises(ValueError):
            resample_spline(vol, (2, 2, 2), clip=bad_clip)
    for bad_coef in (np.zeros((27, 28, 29)), torch.zeros(27, 28, 29), torch.zeros(27, 28, 29, dtype=torch.float64),
                     torch.zeros(3, 4, 5, dtype=torch.float64)):      # not a device tensor / shape
        with pytest.raises(ValueError):
            resample_spline(vol, (2, 2, 2), coefficients=bad_coef)
    with pytest.raises(ValueError) as e:
        resample_volume(vol, (2, 2, 2), order=3)                    # still not resample_volume's
    assert "resample_spline" in str(e.value)
    with pytest.raises(ValueError):
        PP.preprocess_volume(vol, {}, (2.0, 2.0, 2.0), target_spacing=(4.0, 4.0, 4.0), resample_order=2)
    with pytest.raises(ValueError):
        PP.preprocess_volume(vol, {}, (2.0, 2.0, 2.0), resample_order=3)     # no target
    with pytest.raises(_native.NativeError):
        resample_spline(vol, (2, 2, 2))
    with pytest.raises(_native.NativeError):
        resample_spline(vol.astype(np.float64), spacing=(2.0, 2.0, 2.0), target_spacing=(4.0, 4.0, 4.0),
                        clip=(0.0, 1.0))
    with pytest.raises(_native.NativeError):
        spline_coefficients(vol)


def test_infer_volume_checks_the_order_first():
    from light_unet import inference
    with pytest.raises(ValueError):
        inference.infer_volume(np.zeros((4, 4, 4), np.float32), None, {}, resample_order=2)


def test_exports_are_declared_and_bound():
    from light_unet import _native
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "l3u.h")) as f:
        header = f.read()
    assert "int l3u_spline_prefilter(" in header and "int l3u_resample_spline(" in header
    assert "#define L3U_ABI_VERSION 5" in header and _native.ABI_VERSION == 5
    assert len(_native._SIGS["l3u_spline_prefilter"]) == 11
    assert len(_native._SIGS["l3u_spline_prefilter_passes"]) == 12
    assert len(_native._SIGS["l3u_resample_spline"]) == 14
    assert _native._SIGS["l3u_spline_prefilter"][6:10] == [_native.D] * 4
    assert _native._SIGS["l3u_resample_spline"][10:13] == [_native.F, _native.F, _native.I]
    lib = _native.load()
    for name in ("l3u_spline_prefilter", "l3u_spline_prefilter_passes", "l3u_resample_spline"):
        assert hasattr(lib, name)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                           "light-3d-unet-front_amd", "Makefile")) as f:
        assert "build/spline.o: FLAGS += -ffp-contract=off" in f.read()
