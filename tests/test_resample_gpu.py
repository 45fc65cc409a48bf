"""Device resampling (csrc/resample.hip, light_unet/resample.py) against scipy's zoom
(tests/golden/resample.npz, made by tests/golden/make_resample_goldens.py), and its two consumers:
preprocess_volume(target_spacing=...) and infer_volume(native_shape=...).

Bounds: order 0 copies values, so it must equal scipy; order 1 from float64 must equal scipy's
float64 result rounded to float32.  Order 1 from float32 may differ from scipy by at most one
float32 ulp of the golden (what a re-associated float64 sum of 8 products can move a single float32
rounding by); the kernel keeps scipy's own operation order, the count of differing voxels is
printed (pytest -s) and was 0 in every case, so that assertion is == as well.
"""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_resample_goldens as G   # noqa: E402

pytestmark = pytest.mark.gpu

CASES = "abcdefg"
PATCH = (16, 16, 16)
SHAPE = (40, 36, 44)          # tests/test_sliding_mask_gpu.py's volume and patch


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("resample.npz")
    return z, json.loads(bytes(z["meta"]).decode())


def _inputs(z, k):
    """(float32 image, uint8 label) of a case; g takes a's outputs (the way back)."""
    return (z["a/lin32"], z["a/near8"]) if k == "g" else (z[f"{k}/image"], z[f"{k}/label"])


@pytest.mark.parametrize("k", CASES)
def test_order0_equals_scipy(cuda, fx, k):
    from light_unet.resample import resample_volume
    z, meta = fx
    img, lab = _inputs(z, k)
    out_shape = tuple(meta["cases"][k]["out_shape"])
    got = resample_volume(lab, out_shape, order=0)
    assert got.dtype == np.uint8 and np.array_equal(got, z[f"{k}/near8"])
    got = resample_volume(img, out_shape, order=0)
    assert got.dtype == np.float32 and np.array_equal(got, z[f"{k}/near32"])
    got = resample_volume(img.astype(np.float64), out_shape, order=0)
    assert got.dtype == np.float64 and np.array_equal(got, z[f"{k}/near32"].astype(np.float64))
    # bool goes in as uint8 and comes back as bool, from numpy and from a device tensor
    want = z[f"{k}/near8"] > 0
    got = resample_volume(lab > 0, out_shape, order=0)
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    got = resample_volume(torch.from_numpy(lab > 0).to(cuda), out_shape, order=0, output="device")
    assert got.dtype == torch.bool and got.is_cuda and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("k", CASES)
def test_order1_equals_scipy(cuda, fx, k):
    from light_unet.resample import resample_volume
    z, meta = fx
    img, _ = _inputs(z, k)
    c = meta["cases"][k]
    out_shape = tuple(c["out_shape"])
    got64 = resample_volume(img.astype(np.float64), out_shape, order=1)
    assert got64.dtype == np.float32 and np.array_equal(got64, z[f"{k}/lin64"])
    got32 = resample_volume(img, out_shape, order=1)
    want = z[f"{k}/lin32"]
    differing = int((got32 != want).sum())
    print(f"case {k}: {differing} of {want.size} float32 voxels differ from scipy")
    assert got32.dtype == np.float32
    assert (np.abs(got32.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want)).all()
    assert differing == 0      # 0 in every case on the MI355X: tightened to ==
    if c["spacing"] is not None:       # the shape from the spacings is the golden's
        by_spacing = resample_volume(torch.from_numpy(img).to(cuda), spacing=c["spacing"],
                                     target_spacing=meta["target_spacing"], output="device")
        assert by_spacing.dtype == torch.float32 and np.array_equal(by_spacing.cpu().numpy(), want)


def test_identity_returns_the_source_bits(cuda, fx):
    from light_unet.resample import resample_volume
    z, _ = fx
    img, lab = _inputs(z, "f")
    assert np.array_equal(resample_volume(img, img.shape, order=1).view(np.uint32), img.view(np.uint32))
    assert np.array_equal(resample_volume(img, img.shape, order=0).view(np.uint32), img.view(np.uint32))
    img64 = np.random.default_rng(3).random(img.shape)              # full float64 mantissas
    assert np.array_equal(resample_volume(img64, img.shape, order=1), img64.astype(np.float32))
    assert np.array_equal(resample_volume(img64, img.shape, order=0).view(np.uint64), img64.view(np.uint64))
    assert np.array_equal(resample_volume(lab, lab.shape, order=0), lab)
    # equal spacings give the same shape and the same bits
    assert np.array_equal(resample_volume(img, spacing=(4.0, 4.0, 4.0), target_spacing=(4.0, 4.0, 4.0)), img)


@pytest.mark.parametrize("k", ["a", "c", "d"])    # oW = 19 (tails), 12 (whole quads), 19
def test_unaligned_storage_equals_aligned(cuda, fx, k):
    """A source and a destination 4 bytes off a 16-byte boundary (the scalar-store path) give the
    aligned call's bits; through the C ABI, as resample_volume allocates its own destination."""
    from light_unet import _native as nat
    from light_unet.resample import _tables, resample_volume
    z, meta = fx
    img, lab = _inputs(z, k)
    shape, out_shape = img.shape, tuple(meta["cases"][k]["out_shape"])
    n_out = int(np.prod(out_shape))
    for src_np, order in ((img, 1), (img.astype(np.float64), 1), (img, 0), (lab, 0)):
        want = resample_volume(src_np, out_shape, order=order)
        esz = src_np.dtype.itemsize
        off = max(1, 4 // esz)                                      # 4 bytes (8 for float64)
        sbuf = torch.zeros(src_np.size + 8, dtype=torch.from_numpy(src_np).dtype, device=cuda)
        src = sbuf[off:off + src_np.size].view(shape)
        src.copy_(torch.from_numpy(src_np))
        assert src.data_ptr() % 16 != 0 and src.is_contiguous()
        # a tensor with a storage offset goes through resample_volume as it is
        assert np.array_equal(resample_volume(src, out_shape, order=order), want)
        ddt = torch.float32 if order == 1 else sbuf.dtype
        doff = max(1, 4 // ddt.itemsize)
        dbuf = torch.full((n_out + 8,), 7, dtype=ddt, device=cuda)
        dst = dbuf[doff:doff + n_out]
        assert dst.data_ptr() % 16 != 0
        tab, (lo, hi, t) = _tables(shape, out_shape, order, cuda)
        code = {torch.float32: 0, torch.float64: 1, torch.uint8: 2}
        nat.call("l3u_resample", src.data_ptr(), code[src.dtype], *shape, dst.data_ptr(), code[ddt],
                 *out_shape, order, tab.data_ptr() + lo, None if hi is None else tab.data_ptr() + hi,
                 None if t is None else tab.data_ptr() + t, nat.stream())
        got = dbuf.cpu().numpy()
        assert np.array_equal(got[doff:doff + n_out].reshape(out_shape), want), (k, src_np.dtype, order)
        assert (got[:doff] == 7).all() and (got[doff + n_out:] == 7).all()    # nothing written outside


def test_non_contiguous_and_wide_rows(cuda):
    """A permuted device tensor is made contiguous; rows wider than one workgroup's 1024 columns
    take the outer column loop (oW = 1030 > 4 * 256, not a multiple of 4)."""
    from light_unet.resample import resample_volume
    rng = np.random.default_rng(8)
    a = rng.random((9, 7, 11), dtype=np.float32)
    t = torch.from_numpy(a).to(cuda).permute(2, 0, 1)
    assert not t.is_contiguous()
    assert np.array_equal(resample_volume(t, (5, 13, 6)),
                          resample_volume(np.ascontiguousarray(a.transpose(2, 0, 1)), (5, 13, 6)))
    w = rng.random((2, 3, 700), dtype=np.float32)
    for order in (0, 1):
        got = resample_volume(w, (3, 2, 1030), order=order)
        assert np.array_equal(got, G.transcription(w, (3, 2, 1030), order)), order


def test_bad_abi_arguments_are_rejected(cuda):
    from light_unet import _native as nat
    lib = nat.load()
    s = torch.zeros(4 * 4 * 4, dtype=torch.float64, device=cuda)
    d = torch.zeros(4 * 4 * 4, dtype=torch.float64, device=cuda)
    ti = torch.zeros(12, dtype=torch.int32, device=cuda)
    tt = torch.zeros(12, dtype=torch.float64, device=cuda)
    def rc(sdt, ddt, order, D=4, oD=4, hi=True):   # noqa: E306
        return lib.l3u_resample(s.data_ptr(), sdt, D, 4, 4, d.data_ptr(), ddt, oD, 4, 4, order,
                                ti.data_ptr(), ti.data_ptr() if hi else None, tt.data_ptr(),
                                nat.stream())
    assert rc(0, 0, 1) == 0 and rc(1, 0, 1) == 0 and rc(2, 2, 0) == 0 and rc(1, 1, 0) == 0
    assert rc(2, 0, 1) == 1 and rc(0, 1, 1) == 1 and rc(3, 0, 1) == 1      # order 1: float(64) -> float
    assert rc(0, 1, 0) == 1 and rc(3, 3, 0) == 1 and rc(-1, -1, 0) == 1    # order 0: same dtype, 0..2
    assert rc(0, 0, 2) == 1 and rc(0, 0, -1) == 1
    assert rc(0, 0, 1, D=0) == 1 and rc(0, 0, 1, oD=0) == 1 and rc(0, 0, 1, hi=False) == 1
    torch.cuda.synchronize()


def test_two_runs_are_bitwise_identical(cuda, fx):
    from light_unet.resample import resample_volume
    z, _ = fx
    img, lab = _inputs(z, "b")
    dimg = torch.from_numpy(img).to(cuda)
    for order, src in ((1, dimg), (0, dimg), (0, torch.from_numpy(lab).to(cuda))):
        a = resample_volume(src, (17, 15, 31), order=order, output="device")
        b = resample_volume(src, (17, 15, 31), order=order, output="device")
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


# ------------------------------------------------------------------ preprocess_volume
PP_CFG = {"intensity": {"clip_percentile_low": 0.5, "clip_percentile_high": 99.5,
                        "normalization_range": [0, 1]},
          "body_mask": {"enabled": True, "threshold": 0.3, "closing_voxels": 2,
                        "keep_largest_component": True, "dilate_voxels": 1},
          "volume_threshold": {"train_cc": 0.5, "inference_cc": 0.1}}


def _same_outputs(a, b, drop_resample):
    (ia, ma, ea), (ib, mb, eb) = a, b
    assert ia.dtype == ib.dtype == np.float32 and np.array_equal(ia, ib)
    assert ma.dtype == mb.dtype == np.bool_ and np.array_equal(ma, mb)
    ea, eb = dict(ea), dict(eb)
    if drop_resample:
        ea.pop("resample", None)
        eb.pop("resample", None)
    assert ea == eb


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_preprocess_volume_resamples_first(cuda, fx, dtype):
    from light_unet import preprocess as PP
    from light_unet.resample import resample_volume
    z, meta = fx
    img = z["b/image"].astype(dtype)
    spacing, target = meta["cases"]["b"]["spacing"], meta["target_spacing"]
    got = PP.preprocess_volume(img, PP_CFG, spacing, target_spacing=target)
    assert got[2]["resample"] == {"orig_shape": [33, 30, 41], "orig_spacing": spacing,
                                  "shape": [17, 15, 31], "spacing": target, "applied": True}
    assert got[0].shape == got[1].shape == (17, 15, 31) and got[1].any()
    two = PP.preprocess_volume(resample_volume(img, spacing=spacing, target_spacing=target),
                               PP_CFG, target)
    assert "resample" not in two[2]
    _same_outputs(got, two, drop_resample=True)
    # the thresholds are the target grid's: 0.5 cc of 4 mm voxels
    assert got[2]["voxel_thresholds"]["0.5cc"]["voxel_count"] == 8
    # device in, device out
    dev = PP.preprocess_volume(torch.from_numpy(img).to(cuda), PP_CFG, spacing, output="device",
                               target_spacing=target)
    assert dev[0].is_cuda and dev[1].is_cuda and dev[2] == got[2]
    assert np.array_equal(dev[0].cpu().numpy(), got[0]) and np.array_equal(dev[1].cpu().numpy(), got[1])
    # the label is the caller's, with the shape from the metadata
    lab = resample_volume(z["b/label"], got[2]["resample"]["shape"], order=0, output="device")
    assert np.array_equal(lab.cpu().numpy(), z["b/near8"])


def test_preprocess_volume_within_a_tenth_of_a_millimetre_is_left_alone(cuda, fx):
    from light_unet import preprocess as PP
    z, meta = fx
    img = z["b/image"]
    near = (4.05, 3.95, 4.0999)
    plain = PP.preprocess_volume(img, PP_CFG, near)
    got = PP.preprocess_volume(img, PP_CFG, near, target_spacing=(4.0, 4.0, 4.0))
    assert got[2]["resample"] == {"orig_shape": [33, 30, 41], "orig_spacing": list(near),
                                  "shape": [33, 30, 41], "spacing": list(near), "applied": False}
    assert "resample" not in plain[2]
    _same_outputs(got, plain, drop_resample=True)       # thresholds from the real spacing included
    # without target_spacing nothing changed: no "resample" key, the same arrays with or without
    # a spacing
    bare = PP.preprocess_volume(img, PP_CFG)
    assert "resample" not in bare[2] and np.array_equal(bare[0], plain[0])
    # 0.11 mm off on one axis: resampled
    far = PP.preprocess_volume(img, PP_CFG, (4.0, 4.0, 4.11), target_spacing=(4.0, 4.0, 4.0))
    assert far[2]["resample"]["applied"] and far[2]["resample"]["shape"] == [33, 30, 42]
    assert far[0].shape == (33, 30, 42)
    with pytest.raises(ValueError):
        PP.preprocess_volume(img, PP_CFG, target_spacing=(4.0, 4.0, 4.0))


# ------------------------------------------------------------------ infer_volume
def _model(cuda):
    from light_unet.models.unet3d import Lightweight3DUNet
    torch.manual_seed(42)
    return Lightweight3DUNet(dropout_p=0.0).to(cuda)


def _volume(shape, seed):
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(s, dtype=np.float32) for s in shape], indexing="ij")
    v = 0.3 * rng.random(shape, dtype=np.float32)
    for _ in range(3):
        c = [rng.uniform(3, s - 3) for s in shape]
        v += np.exp(-((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2) / 12.0).astype(np.float32)
    return v.astype(np.float32)


def test_infer_volume_maps_back_to_the_native_grid(cuda):
    from light_unet import inference, lesion
    from light_unet.resample import resample_volume, resampled_shape
    from light_unet.utils import sliding_window_inference_3d as sw
    model, img = _model(cuda), _volume(SHAPE, 5)
    mask = np.zeros(SHAPE, bool)
    mask[4:, :30, 6:40] = True
    mask[20:, :, :20] = False
    native_spacing = (2.04, 2.04, 3.0)
    native_shape = resampled_shape(SHAPE, (4.0, 4.0, 4.0), native_spacing)
    assert native_shape == (78, 71, 59)
    base = {"patch_size": list(PATCH), "bbox_expansion_voxels": 2, "bbox_expansion_mm": 10.0,
            "volume_threshold": {"inference_cc": 0.5},
            "body_mask": {"enabled": True, "apply_to_inference": True}}
    cfg = {"data": base, "validation": {"default_threshold": 0.5}}
    cache = {}
    # without native_shape the call is what it was: the int expansion on the network's grid
    plain_map, plain_boxes = inference.infer_volume(img, model, cfg, body_mask=mask, forward_cache=cache)
    assert np.array_equal(plain_map, sw(img, model, PATCH, 0.5, cuda, True) * mask)
    assert plain_boxes == lesion.extract_bboxes(plain_map, 0.5, 0.5, (4.0, 4.0, 4.0), 2)
    thr = float(np.quantile(plain_map[mask], 0.7))

    got_map, got = inference.infer_volume(img, model, cfg, body_mask=mask, spacing=native_spacing,
                                          threshold=thr, forward_cache=cache,
                                          native_shape=native_shape)
    want_map = resample_volume(plain_map, native_shape, order=1)
    assert isinstance(got_map, np.ndarray) and got_map.dtype == np.float32
    assert got_map.shape == native_shape and np.array_equal(got_map, want_map)
    expansion = [math.ceil(10.0 / s) for s in native_spacing]
    assert expansion == [5, 5, 4]
    want = lesion.extract_bboxes(want_map, thr, 0.5, native_spacing, expansion)
    assert got == want and len(want) > 0
    for b in got:
        zl, zh, yl, yh, xl, xh = b["bbox_voxel"]
        assert 0 <= zl <= zh < native_shape[0] and 0 <= yl <= yh < native_shape[1]
        assert 0 <= xl <= xh < native_shape[2]
    # the sequence form with equal entries is the int form; a box grows per axis
    assert lesion.extract_bboxes(want_map, thr, 0.5, native_spacing, (3, 3, 3)) == \
        lesion.extract_bboxes(want_map, thr, 0.5, native_spacing, 3)
    tight = lesion.extract_bboxes(want_map, thr, 0.5, native_spacing, 0)
    for b0, b1 in zip(tight, want):
        for a in range(3):
            assert b1["bbox_voxel"][2 * a] == max(0, b0["bbox_voxel"][2 * a] - expansion[a])
            assert b1["bbox_voxel"][2 * a + 1] == min(native_shape[a] - 1,
                                                      b0["bbox_voxel"][2 * a + 1] + expansion[a])
    # at the network's own 4 mm the per-axis expansion is the reference's 3 voxels
    same_map, same = inference.infer_volume(img, model, cfg, body_mask=mask, threshold=thr,
                                            forward_cache=cache, native_shape=SHAPE)
    assert np.array_equal(same_map, plain_map)
    assert same == lesion.extract_bboxes(plain_map, thr, 0.5, (4.0, 4.0, 4.0), 3)
