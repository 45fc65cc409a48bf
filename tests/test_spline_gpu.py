"""Cubic B-spline resampling on the device (csrc/spline.hip, light_unet/resample.py:
spline_coefficients, resample_spline) against the numpy transcription of the module's definition
and scipy's zoom(order=3) (tests/golden/spline.npz, made by tests/golden/make_spline_goldens.py),
and its two consumers: preprocess_volume(resample_order=3) and infer_volume(resample_order=3).

Bounds: the definition fixes every float64 operation and its order, so the coefficients and the
float32 output must equal the transcription's bit for bit, for float32 and float64 sources.
Against scipy the definition allows one float32 ulp at a voxel and 1 differing voxel in 10 000 per
case (tests/test_spline_host.py); the count is printed (pytest -s) and was 0 of every case's voxels
on the MI355X, for both images and both source types, so that assertion is == as well.
"""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_spline_goldens as G   # noqa: E402

pytestmark = pytest.mark.gpu

CASES = sorted(G.CASES)
PATCH = (16, 16, 16)
SHAPE = (40, 36, 44)          # tests/test_resample_gpu.py's volume and patch


@pytest.fixture(scope="module")
def fx(golden):
    """(fixture file, meta, {(case, image): (float32 source, transcription's coefficients, its
    float32 output)}), computed once and left unchanged."""
    z = golden("spline.npz")
    first = golden("resample.npz")
    ref = {}
    for k, (_, out_shape) in G.CASES.items():
        for m in G.IMAGES:
            if k == "g":
                img = z[f"a/{m}/s32"]
            elif (k, m) in G.stored_inputs():
                img = z[f"{k}/{m}"]
            else:
                img = first[f"{k}/image"]
            coef = G.coefficients(img)
            ref[k, m] = (img, coef, G.transcription(img, out_shape, coef=coef))
    return z, json.loads(bytes(z["meta"]).decode()), ref


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize("k", CASES)
def test_coefficients_equal_the_transcription(cuda, fx, k):
    from light_unet.resample import spline_coefficients
    for m in G.IMAGES:
        img, coef, _ = fx[2][k, m]
        want = _bits(coef)
        got = spline_coefficients(img)
        assert got.dtype == np.float64 and got.shape == tuple(n + 24 for n in img.shape)
        assert np.array_equal(_bits(got), want), (k, m, "float32 numpy")
        assert np.array_equal(_bits(spline_coefficients(img.astype(np.float64))), want), (k, m)
        for dt in (torch.float32, torch.float64):
            dev = spline_coefficients(torch.from_numpy(np.array(img)).to(cuda, dt), output="device")
            assert dev.is_cuda and dev.dtype == torch.float64
            assert np.array_equal(_bits(dev), want), (k, m, dt)


@pytest.mark.parametrize("k", CASES)
def test_output_equals_the_transcription_and_scipy(cuda, fx, k):
    from light_unet.resample import resample_spline
    z, meta, ref = fx
    out_shape = tuple(meta["cases"][k]["out_shape"])
    for m in G.IMAGES:
        img, _, want = ref[k, m]
        got32 = resample_spline(img, out_shape)
        got64 = resample_spline(img.astype(np.float64), out_shape)
        assert got32.dtype == got64.dtype == np.float32 and got32.shape == out_shape
        assert np.array_equal(_bits(got32), _bits(want)), (k, m)
        assert np.array_equal(_bits(got64), _bits(want)), (k, m)
        dev = resample_spline(torch.from_numpy(np.array(img)).to(cuda), out_shape, output="device")
        assert dev.is_cuda and dev.dtype == torch.float32 and np.array_equal(_bits(dev), _bits(want))
        for name, gold in (("s32", z[f"{k}/{m}/s32"]), ("s64", G.scipy64(z, k, m))):
            differing = int((got32 != gold).sum())
            print(f"case {k}/{m}/{name}: {differing} of {gold.size} float32 voxels differ from scipy")
            assert (np.abs(got32.astype(np.float64) - gold.astype(np.float64))
                    <= np.spacing(np.abs(gold))).all()
            assert differing * 10000 <= gold.size
            assert differing == 0      # 0 in every case on the MI355X: tightened to ==


def test_by_spacing_gives_the_shape_of_the_order1_cases(cuda, fx):
    from light_unet.resample import resample_spline
    import make_resample_goldens as R
    for k in "ab":
        img, _, want = fx[2][k, "g"]
        got = resample_spline(img, spacing=R.CASES[k][2], target_spacing=R.TARGET)
        assert np.array_equal(_bits(got), _bits(want))


def test_identity_returns_the_source_bits(cuda, fx):
    from light_unet.resample import resample_spline
    for m in G.IMAGES:
        img = fx[2]["f", m][0]
        assert np.array_equal(_bits(resample_spline(img, img.shape)), _bits(img))
        assert np.array_equal(_bits(resample_spline(img, spacing=(4.0, 4.0, 4.0),
                                                    target_spacing=(4.0, 4.0, 4.0))), _bits(img))
    img64 = 0.5 + np.random.default_rng(3).random((12, 10, 16))     # full float64 mantissas
    assert np.array_equal(resample_spline(img64, img64.shape), img64.astype(np.float32))


@pytest.mark.parametrize("k", ["a", "c", "g"])
def test_clip_is_np_clip_of_the_unclipped_result(cuda, fx, k):
    from light_unet.resample import resample_spline
    img, _, want = fx[2][k, "u"]
    out_shape = want.shape
    lo, hi = 0.25, 0.75                      # exact in float32; the uniform image spans [0, 1)
    got = resample_spline(img, out_shape, clip=(lo, hi))
    assert (want < lo).any() and (want > hi).any()
    assert np.array_equal(_bits(got), _bits(np.clip(want, np.float32(lo), np.float32(hi))))
    # the clip to the source's own range takes a spline's overshoot back
    boxed = resample_spline(img, out_shape, clip=(float(img.min()), float(img.max())))
    assert boxed.min() >= img.min() and boxed.max() <= img.max()
    assert np.array_equal(_bits(boxed), _bits(np.clip(want, img.min(), img.max())))


def test_coefficients_are_reused_across_output_shapes(cuda, fx):
    from light_unet.resample import resample_spline, spline_coefficients
    img = fx[2]["b", "g"][0]
    dimg = torch.from_numpy(np.array(img)).to(cuda)
    coef = spline_coefficients(dimg, output="device")
    before = coef.clone()
    for out_shape in ((17, 15, 31), (40, 33, 50)):
        full = resample_spline(dimg, out_shape, output="device")
        again = resample_spline(dimg, out_shape, coefficients=coef, output="device")
        assert full.data_ptr() != again.data_ptr() and torch.equal(full.view(torch.int32),
                                                                   again.view(torch.int32))
        # with coefficients the volume gives the shape alone
        shape_only = resample_spline(np.zeros(img.shape, np.float32), out_shape, coefficients=coef)
        assert np.array_equal(_bits(shape_only), _bits(full))
    assert torch.equal(coef, before)
    assert np.array_equal(_bits(resample_spline(dimg, (17, 15, 31))), _bits(fx[2]["b", "g"][2]))


@pytest.mark.parametrize("k", ["a", "c", "h"])    # oW = 19 (tails), 12 (whole quads), 130
def test_unaligned_storage_equals_aligned(cuda, fx, k):
    """A source, a coefficient buffer and a destination 8 bytes off a 16-byte boundary give the
    aligned call's bits, through the C ABI (resample_spline allocates its own buffers); the guard
    values before and after the coefficient and destination buffers are unchanged."""
    from light_unet import _native as nat
    from light_unet.resample import _spline_tables, spline_constants
    for m, sdt in (("u", torch.float32), ("g", torch.float64)):
        img, coef, want = fx[2][k, m]
        shape, out_shape = img.shape, want.shape
        n_coef, n_out = coef.size, want.size
        sbuf = torch.zeros(img.size + 8, dtype=sdt, device=cuda)
        soff = 8 // sbuf.element_size()
        src = sbuf[soff:soff + img.size].view(shape)
        src.copy_(torch.from_numpy(np.array(img)))
        cbuf = torch.full((n_coef + 6,), 7.0, dtype=torch.float64, device=cuda)
        dbuf = torch.full((n_out + 8,), 7.0, dtype=torch.float32, device=cuda)
        cof, dst = cbuf[3:3 + n_coef], dbuf[2:2 + n_out]
        for t in (src, cof, dst):
            assert t.data_ptr() % 16 == 8 and t.is_contiguous()
        nat.call("l3u_spline_prefilter", src.data_ptr(), 0 if sdt == torch.float32 else 1, *shape,
                 cof.data_ptr(), *spline_constants(), nat.stream())
        tab, start = _spline_tables(shape, out_shape)
        tab = tab.to(cuda)
        nat.call("l3u_resample_spline", cof.data_ptr(), *shape, dst.data_ptr(), *out_shape,
                 tab.data_ptr() + start, tab.data_ptr(), 0.0, 0.0, 0, nat.stream())
        c, d = cbuf.cpu().numpy(), dbuf.cpu().numpy()
        assert np.array_equal(_bits(c[3:3 + n_coef]), _bits(coef.reshape(-1))), (k, m)
        assert np.array_equal(_bits(d[2:2 + n_out]), _bits(want.reshape(-1))), (k, m)
        assert (c[:3] == 7.0).all() and (c[3 + n_coef:] == 7.0).all()       # nothing written outside
        assert (d[:2] == 7.0).all() and (d[2 + n_out:] == 7.0).all()
        assert torch.equal(src.cpu(), torch.from_numpy(np.array(img)).to(sdt))   # the source is read only


def test_a_bad_table_reads_nothing_outside_the_coefficients(cuda, fx):
    """start entries outside [0, n_in + 20] are clamped again on load: the call succeeds and equals
    the call with the clamped table."""
    from light_unet import _native as nat
    from light_unet.resample import _spline_tables
    img, coef, want = fx[2]["a", "u"]
    shape, out_shape = img.shape, want.shape
    n = sum(out_shape)
    tab, start = _spline_tables(shape, out_shape)
    raw = tab.numpy().copy()
    st = raw[start:].view(np.int32)
    st[0::3] = -5
    st[1::3] = 10 ** 6
    limit = np.concatenate([np.full(o, s + 20, np.int32) for s, o in zip(shape, out_shape)])
    fixed = raw.copy()
    fixed[start:].view(np.int32)[:] = np.clip(st, 0, limit)
    dcoef = torch.from_numpy(np.array(coef)).to(cuda)
    outs = []
    for t in (raw, fixed):
        dt = torch.from_numpy(t).to(cuda)
        dst = torch.zeros(out_shape, dtype=torch.float32, device=cuda)
        nat.call("l3u_resample_spline", dcoef.data_ptr(), *shape, dst.data_ptr(), *out_shape,
                 dt.data_ptr() + start, dt.data_ptr(), 0.0, 0.0, 0, nat.stream())
        outs.append(dst.cpu().numpy())
    assert len(st) == n and np.array_equal(_bits(outs[0]), _bits(outs[1]))


def test_a_permuted_device_tensor_is_its_contiguous_copy(cuda):
    from light_unet.resample import resample_spline, spline_coefficients
    a = np.random.default_rng(8).random((9, 7, 11), dtype=np.float32)
    t = torch.from_numpy(a).to(cuda).permute(2, 0, 1)
    assert not t.is_contiguous()
    c = np.ascontiguousarray(a.transpose(2, 0, 1))
    assert np.array_equal(_bits(resample_spline(t, (5, 13, 6))), _bits(resample_spline(c, (5, 13, 6))))
    assert np.array_equal(_bits(resample_spline(c, (5, 13, 6))), _bits(G.transcription(c, (5, 13, 6))))
    assert np.array_equal(_bits(spline_coefficients(t)), _bits(G.coefficients(c)))


def test_two_runs_are_bitwise_identical(cuda, fx):
    from light_unet.resample import resample_spline, spline_coefficients
    dimg = torch.from_numpy(np.array(fx[2]["b", "u"][0])).to(cuda)
    ca = spline_coefficients(dimg, output="device")
    cb = spline_coefficients(dimg, output="device")
    assert ca.data_ptr() != cb.data_ptr() and torch.equal(ca.view(torch.int64), cb.view(torch.int64))
    a = resample_spline(dimg, (17, 15, 31), output="device")
    b = resample_spline(dimg, (17, 15, 31), output="device")
    assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_bad_abi_arguments_are_rejected(cuda):
    from light_unet import _native as nat
    from light_unet.resample import spline_constants
    lib = nat.load()
    s = torch.zeros(4 * 4 * 4, dtype=torch.float64, device=cuda)
    c = torch.zeros(28 * 28 * 28, dtype=torch.float64, device=cuda)
    d = torch.zeros(4 * 4 * 4, dtype=torch.float32, device=cuda)
    ti = torch.full((12,), 12, dtype=torch.int32, device=cuda)
    tw = torch.zeros(12 * 4, dtype=torch.float64, device=cuda)
    k = spline_constants()

    def pre(src=s.data_ptr(), dtype=1, D=4, coef=c.data_ptr()):
        return lib.l3u_spline_prefilter(src, dtype, D, 4, 4, coef, *k, nat.stream())

    def gat(coef=c.data_ptr(), D=4, dst=d.data_ptr(), oD=4, start=ti.data_ptr(), w=tw.data_ptr()):
        return lib.l3u_resample_spline(coef, D, 4, 4, dst, oD, 4, 4, start, w, 0.0, 1.0, 1, nat.stream())

    assert pre() == 0 and pre(dtype=0) == 0 and gat() == 0
    assert pre(src=None) == 1 and pre(coef=None) == 1 and pre(src=c.data_ptr()) == 1   # NULL, aliased
    assert pre(dtype=2) == 1 and pre(dtype=-1) == 1 and pre(D=0) == 1 and pre(D=-3) == 1
    assert lib.l3u_spline_prefilter_passes(s.data_ptr(), 1, 4, 4, 4, c.data_ptr(), *k, 0, nat.stream()) == 1
    assert lib.l3u_spline_prefilter_passes(s.data_ptr(), 1, 4, 4, 4, c.data_ptr(), *k, 8, nat.stream()) == 1
    assert gat(coef=None) == 1 and gat(dst=None) == 1 and gat(dst=c.data_ptr()) == 1
    assert gat(start=None) == 1 and gat(w=None) == 1 and gat(D=0) == 1 and gat(oD=0) == 1
    torch.cuda.synchronize()


def test_the_passes_compose_the_prefilter(cuda, fx):
    """l3u_spline_prefilter_passes (the timing entry point): the three axis passes one call each
    give the bits of the whole prefilter."""
    from light_unet import _native as nat
    from light_unet.resample import spline_constants
    img, coef, _ = fx[2]["d", "g"]
    src = torch.from_numpy(np.array(img)).to(cuda)
    out = torch.zeros(coef.shape, dtype=torch.float64, device=cuda)
    for bit in (1, 2, 4):
        nat.call("l3u_spline_prefilter_passes", src.data_ptr(), 0, *img.shape, out.data_ptr(),
                 *spline_constants(), bit, nat.stream())
    assert np.array_equal(_bits(out), _bits(coef))


# ------------------------------------------------------------------ preprocess_volume
PP_CFG = {"intensity": {"clip_percentile_low": 0.5, "clip_percentile_high": 99.5,
                        "normalization_range": [0, 1]},
          "body_mask": {"enabled": True, "threshold": 0.3, "closing_voxels": 2,
                        "keep_largest_component": True, "dilate_voxels": 1},
          "volume_threshold": {"train_cc": 0.5, "inference_cc": 0.1}}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_preprocess_volume_resamples_with_the_spline_first(cuda, golden, dtype):
    from light_unet import preprocess as PP
    from light_unet.resample import resample_spline
    first = golden("resample.npz")
    meta = json.loads(bytes(first["meta"]).decode())
    img = first["b/image"].astype(dtype)
    spacing, target = meta["cases"]["b"]["spacing"], meta["target_spacing"]
    got = PP.preprocess_volume(img, PP_CFG, spacing, target_spacing=target, resample_order=3)
    assert got[2]["resample"] == {"orig_shape": [33, 30, 41], "orig_spacing": spacing,
                                  "shape": [17, 15, 31], "spacing": target, "applied": True,
                                  "order": 3}
    two = PP.preprocess_volume(resample_spline(img, spacing=spacing, target_spacing=target),
                               PP_CFG, target)
    assert got[0].dtype == np.float32 and np.array_equal(_bits(got[0]), _bits(two[0]))
    assert got[1].dtype == np.bool_ and np.array_equal(got[1], two[1]) and got[1].any()
    rest = dict(got[2])
    rest.pop("resample")
    assert rest == two[2]
    # without resample_order the call and its metadata are what they were: order 1, no "order"
    plain = PP.preprocess_volume(img, PP_CFG, spacing, target_spacing=target)
    assert plain[2]["resample"] == {"orig_shape": [33, 30, 41], "orig_spacing": spacing,
                                    "shape": [17, 15, 31], "spacing": target, "applied": True}
    one = PP.preprocess_volume(img, PP_CFG, spacing, target_spacing=target, resample_order=1)
    assert one[2]["resample"] == dict(plain[2]["resample"], order=1)
    assert np.array_equal(_bits(one[0]), _bits(plain[0])) and not np.array_equal(got[0], plain[0])
    # device in, device out
    dev = PP.preprocess_volume(torch.from_numpy(img).to(cuda), PP_CFG, spacing, output="device",
                               target_spacing=target, resample_order=3)
    assert dev[0].is_cuda and dev[1].is_cuda and dev[2] == got[2]
    assert np.array_equal(_bits(dev[0]), _bits(got[0])) and np.array_equal(dev[1].cpu().numpy(), got[1])


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


def test_infer_volume_maps_back_with_the_spline(cuda):
    from light_unet import inference, lesion
    from light_unet.resample import resample_spline, resample_volume, resampled_shape
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
    plain_map, _ = inference.infer_volume(img, model, cfg, body_mask=mask, forward_cache=cache)
    thr = float(np.quantile(plain_map[mask], 0.7))
    got_map, got = inference.infer_volume(img, model, cfg, body_mask=mask, spacing=native_spacing,
                                          threshold=thr, forward_cache=cache,
                                          native_shape=native_shape, resample_order=3)
    want_map = resample_spline(plain_map, native_shape, clip=(0.0, 1.0))
    assert isinstance(got_map, np.ndarray) and got_map.dtype == np.float32
    assert got_map.shape == native_shape and np.array_equal(_bits(got_map), _bits(want_map))
    assert got_map.min() >= 0.0 and got_map.max() <= 1.0
    expansion = [math.ceil(10.0 / s) for s in native_spacing]
    want = lesion.extract_bboxes(want_map, thr, 0.5, native_spacing, expansion)
    assert got == want and len(want) > 0
    # the default call is unchanged: order 1
    lin_map, lin = inference.infer_volume(img, model, cfg, body_mask=mask, spacing=native_spacing,
                                          threshold=thr, forward_cache=cache,
                                          native_shape=native_shape)
    want_lin = resample_volume(plain_map, native_shape, order=1)
    assert np.array_equal(_bits(lin_map), _bits(want_lin)) and not np.array_equal(lin_map, got_map)
    assert lin == lesion.extract_bboxes(want_lin, thr, 0.5, native_spacing, expansion)
