"""The body-mask checks of sliding_window_inference_3d run before any device call: a wrong shape
or a dtype numpy would promote to float64 raises ValueError on a machine without a GPU."""
import numpy as np
import pytest
import torch


def _call(image, mask):
    from light_unet.utils import sliding_window_inference_3d
    model = torch.nn.Conv3d(1, 1, 1)      # on the CPU: a device call would raise NativeError
    return sliding_window_inference_3d(image, model, (16, 16, 16), 0.5, body_mask=mask)


def test_body_mask_shape_and_dtype_are_checked_first():
    img = np.zeros((20, 24, 18), np.float32)
    with pytest.raises(ValueError, match="shape"):
        _call(img, np.ones((20, 24, 17), np.float32))
    with pytest.raises(ValueError, match="shape"):
        _call(img[None], torch.ones(2, 20, 24, 18))
    for bad in (np.ones(img.shape, np.float64), np.ones(img.shape, np.int32),
                np.ones(img.shape, np.float16), torch.ones(img.shape, dtype=torch.float64),
                torch.ones(img.shape, dtype=torch.int64)):
        with pytest.raises(ValueError, match="bool, uint8, int8, int16, float32"):
            _call(img, bad)
    # an accepted mask passes the checks and reaches the device requirement
    from light_unet._native import NativeError
    with pytest.raises(NativeError):
        _call(img, np.ones((1,) + img.shape, bool))


def test_plugin_loads_the_inference_module():
    import sys

    import l3u_plugin
    l3u_plugin.load()
    assert callable(sys.modules[l3u_plugin.ALIAS + ".inference"].infer_volume)


def test_body_mask_conversions_are_exact():
    from light_unet.utils import _checked_body_mask
    rng = np.random.default_rng(0)
    shape = (3, 4, 5)
    for dt, want in ((np.bool_, np.uint8), (np.uint8, np.uint8), (np.int8, np.float32),
                     (np.int16, np.float32), (np.float32, np.float32)):
        m = (rng.integers(-3, 4, shape) if dt != np.bool_ else rng.integers(0, 2, shape)).astype(dt)
        for src in (m, torch.from_numpy(m), m[None]):
            got = _checked_body_mask(src, shape)
            got = got.numpy() if isinstance(got, torch.Tensor) else got
            assert got.dtype == want and got.shape == shape
            # the float32 value per voxel is the one numpy's float32 product multiplies by
            assert np.array_equal(got.astype(np.float32), np.float32(1) * m)
            assert (np.float32(1) * m).dtype == np.float32
