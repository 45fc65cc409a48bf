"""Host side of the device resampling (light_unet/resample.py): shapes from spacings, the per-axis
coordinate tables, argument errors, and the golden fixture against scipy where it imports; no GPU."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_resample_goldens as G   # noqa: E402

CFG = {"intensity": {"clip_percentile_low": 0.5, "clip_percentile_high": 99.5,
                     "normalization_range": [0, 1]}}


def test_resampled_shape_matches_the_cases():
    from light_unet.resample import resampled_shape
    for k, (shape, out_shape, spacing) in G.CASES.items():
        if spacing is not None:
            assert resampled_shape(shape, spacing, G.TARGET) == tuple(out_shape), k
    # Python's round: halves go to the even neighbour (13 * 2 / 4 = 6.5 -> 6, 15 * 2 / 4 = 7.5 -> 8)
    assert resampled_shape((13, 15, 3), (2.0, 2.0, 2.0), (4.0, 4.0, 4.0)) == (6, 8, 2)
    assert resampled_shape((1, 2, 400), (1.0, 0.5, 2.04), (4.0, 4.0, 4.0)) == (1, 1, 204)   # never 0
    assert resampled_shape((48, 48, 48), (4.0, 4.0, 4.0), (4.0, 4.0, 4.0)) == (48, 48, 48)
    assert resampled_shape((204, 204, 450), (4.0, 4.0, 4.0), (2.04, 2.04, 3.0)) == (400, 400, 600)
    for bad in (((4, 4), (1, 1, 1), (1, 1, 1)), ((4, 4, 4), (1, 1), (1, 1, 1)),
                ((4, 4, 4), (1, 1, 1), (1, 0, 1)), ((4, 0, 4), (1, 1, 1), (1, 1, 1))):
        with pytest.raises(ValueError):
            resampled_shape(*bad)


@pytest.mark.parametrize("n_in,n_out", [(13, 6), (7, 14), (9, 9), (1, 3), (5, 1), (31, 19), (400, 204),
                                        (204, 400)])
def test_axis_table_is_the_closed_form(n_in, n_out):
    from light_unet.resample import axis_table
    near = axis_table(n_in, n_out, 0)
    lo, hi, t = axis_table(n_in, n_out, 1)
    assert near.dtype == lo.dtype == hi.dtype == np.int32 and t.dtype == np.float64
    assert near.shape == lo.shape == hi.shape == t.shape == (n_out,)
    for o in range(n_out):
        c = (o + 0.5) * (n_in / n_out) - 0.5          # Python floats are IEEE doubles
        assert near[o] == min(max(math.floor(c + 0.5), 0), n_in - 1)
        f = math.floor(c)
        assert lo[o] == min(max(f, 0), n_in - 1) and hi[o] == min(max(f + 1, 0), n_in - 1)
        assert t[o] == c - f and 0.0 <= t[o] < 1.0
    if n_in == n_out:
        assert np.array_equal(near, np.arange(n_in)) and np.array_equal(lo, near) and not t.any()
    if n_out > n_in:      # the coordinate itself is not clamped: it leaves the source at both ends
        assert (0.5 * (n_in / n_out) - 0.5) < 0 and t[0] > 0 and lo[0] == hi[0] == 0
        assert lo[-1] == hi[-1] == n_in - 1


def test_argument_errors_come_before_the_device(monkeypatch):
    """Rank, dtype and missing-spacing errors are ValueErrors with or without a GPU; a valid call
    without one raises NativeError (there is no CPU fallback)."""
    import torch
    from light_unet import _native, preprocess as PP
    from light_unet.resample import resample_volume
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    vol = np.zeros((3, 4, 5), np.float32)
    for bad in (np.zeros((4, 5), np.float32), np.zeros((1, 3, 4, 5), np.float32),
                np.zeros((0, 4, 5), np.float32), torch.zeros(2, 3)):
        with pytest.raises(ValueError):
            resample_volume(bad, (2, 2, 2))
    for dt in (np.int16, np.int32, np.float16, np.uint16, np.uint8, bool):     # order 1: floats only
        with pytest.raises(ValueError):
            resample_volume(np.zeros((3, 4, 5), dt), (2, 2, 2), order=1)
    for dt in (np.int16, np.int32, np.int64, np.float16):
        with pytest.raises(ValueError):
            resample_volume(np.zeros((3, 4, 5), dt), (2, 2, 2), order=0)
    with pytest.raises(ValueError):
        resample_volume(torch.zeros(3, 4, 5, dtype=torch.int64), (2, 2, 2), order=0)
    with pytest.raises(ValueError):
        resample_volume(vol, (2, 2, 2), order=3)
    with pytest.raises(ValueError):
        resample_volume(vol)                                        # neither a shape nor spacings
    with pytest.raises(ValueError):
        resample_volume(vol, spacing=(2.0, 2.0, 2.0))               # no target
    with pytest.raises(ValueError):
        resample_volume(vol, target_spacing=(4.0, 4.0, 4.0))        # no source spacing
    for bad_shape in ((2, 2), (2, 0, 2)):
        with pytest.raises(ValueError):
            resample_volume(vol, bad_shape)
    with pytest.raises(ValueError):
        resample_volume(vol, (2, 2, 2), output="cpu")
    with pytest.raises(ValueError):     # target_spacing without spacing, before anything is uploaded
        PP.preprocess_volume(vol, CFG, target_spacing=(4.0, 4.0, 4.0))
    with pytest.raises(_native.NativeError):
        resample_volume(vol, (2, 2, 2))
    with pytest.raises(_native.NativeError):
        resample_volume(vol.astype(bool), spacing=(2.0, 2.0, 2.0), target_spacing=(4.0, 4.0, 4.0),
                        order=0)


def test_extract_bboxes_checks_the_expansion_on_the_host(monkeypatch):
    import torch
    from light_unet import lesion
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    prob = np.zeros((4, 5, 6), np.float32)
    for bad in ((1, 2), [1, 2, 3, 4], np.array([3])):
        with pytest.raises(ValueError):
            lesion.extract_bboxes(prob, expansion_voxels=bad)


def test_export_is_declared_and_bound():
    from light_unet import _native
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "l3u.h")) as f:
        header = f.read()
    assert "int l3u_resample(" in header and "#define L3U_ABI_VERSION 5" in header
    assert len(_native._SIGS["l3u_resample"]) == 15 and _native.ABI_VERSION == 5


def test_golden_file_is_what_the_generator_makes(golden):
    """The fixture's inputs are the generator's seeded inputs; with scipy importable the whole
    file is regenerated and compared array by array (scipy's zoom is what the goldens are)."""
    z = golden("resample.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    assert set(meta["cases"]) == set(G.CASES)
    for k, (img, lab) in G.inputs().items():
        assert np.array_equal(z[f"{k}/image"], img) and np.array_equal(z[f"{k}/label"], lab), k
        assert (lab > 0).any() and (lab == 0).any(), k
    for k, (shape, out_shape, _) in G.CASES.items():
        for name, dt in (("lin32", np.float32), ("lin64", np.float32), ("near32", np.float32),
                         ("near8", np.uint8)):
            assert z[f"{k}/{name}"].shape == tuple(out_shape) and z[f"{k}/{name}"].dtype == dt
    try:
        import scipy.ndimage  # noqa: F401
    except ImportError:
        return
    again = G.build()
    assert set(again) == set(z.files)
    for name in z.files:
        assert again[name].dtype == z[name].dtype and np.array_equal(again[name], z[name]), name


def test_definition_in_numpy_equals_the_goldens(golden):
    """The module's definition, transcribed in numpy, against scipy's outputs in the fixture: equal
    at every voxel, both orders and both source types."""
    z = golden("resample.npz")
    for k, (_, out_shape, _) in G.CASES.items():
        img = z["a/lin32"] if k == "g" else z[f"{k}/image"]
        lab = z["a/near8"] if k == "g" else z[f"{k}/label"]
        assert np.array_equal(G.transcription(img, out_shape, 1), z[f"{k}/lin32"]), k
        assert np.array_equal(G.transcription(img.astype(np.float64), out_shape, 1), z[f"{k}/lin64"]), k
        assert np.array_equal(G.transcription(img, out_shape, 0), z[f"{k}/near32"]), k
        assert np.array_equal(G.transcription(lab, out_shape, 0), z[f"{k}/near8"]), k
    assert np.array_equal(z["f/lin32"], z["f/image"]) and np.array_equal(z["f/near8"], z["f/label"])
