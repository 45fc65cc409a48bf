"""Sliding-window inference with a body mask: windows without a nonzero mask voxel are not run
(l3u_window_occupancy, l3u_window_blend_masked, utils.sliding_window_inference_3d(body_mask=...)),
and the map is bit for bit the unmasked map times the mask.  Also the two consumers:
fast_trainer.validate and inference.infer_volume."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PATCH = (16, 16, 16)
SHAPE = (40, 36, 44)          # 4 x 4 x 5 = 80 windows at patch 16, overlap 0.5


def _grid(shape, patch=PATCH, overlap=0.5):
    from light_unet.utils import window_positions
    return [window_positions(s, p, max(1, int(p * (1 - overlap)))) for s, p in zip(shape, patch)]


def _np_keep(mask, patch=PATCH):
    """The occupancy flags restated: numpy slicing clips the box to the volume, NaN != 0."""
    zs, ys, xs = _grid(mask.shape, patch)
    return np.array([int((mask[z:z + patch[0], y:y + patch[1], x:x + patch[2]] != 0).any())
                     for z in zs for y in ys for x in xs], dtype=np.int32)


def _dev_i32(v, cuda):
    return torch.tensor(v, dtype=torch.int32, device=cuda)


def _occupancy(mask_t, shape, cuda, patch=PATCH):
    from light_unet import _native as nat
    zs, ys, xs = _grid(shape, patch)
    zt, yt, xt = (_dev_i32(v, cuda) for v in (zs, ys, xs))
    keep = torch.full((len(zs) * len(ys) * len(xs),), -7, dtype=torch.int32, device=cuda)
    code = {torch.float32: 0, torch.uint8: 2}[mask_t.dtype]
    nat.call("l3u_window_occupancy", mask_t.data_ptr(), code, *shape, zt.data_ptr(), len(zs),
             yt.data_ptr(), len(ys), xt.data_ptr(), len(xs), *patch, keep.data_ptr(), nat.stream())
    return keep.cpu().numpy()


def _occupancy_masks(shape):
    rng = np.random.default_rng(3)
    out = {"empty": np.zeros(shape, np.float32), "full": np.ones(shape, np.float32)}
    for c in range(8):
        m = np.zeros(shape, np.float32)
        m[tuple(-(c >> a & 1) for a in range(3))] = 1.0      # index 0 or -1 per axis
        out[f"corner{c}"] = m
    box = np.zeros(shape, np.float32)
    box[:8, :8, :8] = 1.0
    out["box"] = box
    out["random"] = (rng.random(shape) < 0.01).astype(np.float32)
    odd = np.full(shape, -0.0, np.float32)                    # -0.0 is zero
    odd[tuple(s // 2 for s in shape)] = np.nan                # a NaN is not
    odd[shape[0] - 1, 0, shape[2] // 3] = -3.0
    out["nan_negative"] = odd
    return out


@pytest.mark.parametrize("shape", [(40, 36, 44), (33, 17, 50), (12, 20, 16)])
def test_occupancy_matches_numpy(cuda, shape):
    for name, m in _occupancy_masks(shape).items():
        ref = _np_keep(m)
        got = _occupancy(torch.from_numpy(m).to(cuda), shape, cuda)
        assert np.array_equal(got, ref), (name, "float32")
        if name != "nan_negative":
            got = _occupancy(torch.from_numpy(m.astype(np.uint8)).to(cuda), shape, cuda)
            assert np.array_equal(got, ref), (name, "uint8")
    # masks that do not start on a 16-byte boundary: every row's wide loads shift
    m = _occupancy_masks(shape)["random"]
    n = m.size
    for dt in (np.float32, np.uint8):
        for off in (1, 3):
            buf = torch.zeros(n + 4, dtype=torch.from_numpy(np.zeros(1, dt)).dtype, device=cuda)
            buf[off:off + n] = torch.from_numpy(m.astype(dt).ravel()).to(cuda)
            assert np.array_equal(_occupancy(buf[off:off + n], shape, cuda), _np_keep(m)), (dt, off)


def test_occupancy_rejects_bad_arguments(cuda):
    from light_unet import _native as nat
    lib = nat.load()
    t = _dev_i32([0], cuda)
    m = torch.zeros(8, 8, 8, device=cuda)
    keep = torch.zeros(1, dtype=torch.int32, device=cuda)
    def rc(dtype, D, pd):   # noqa: E306
        return lib.l3u_window_occupancy(m.data_ptr(), dtype, D, 8, 8, t.data_ptr(), 1, t.data_ptr(),
                                        1, t.data_ptr(), 1, pd, 8, 8, keep.data_ptr(), nat.stream())
    assert rc(0, 8, 8) == 0
    assert rc(1, 8, 8) == 1 and rc(3, 8, 8) == 1        # hipErrorInvalidValue: double / int32 masks
    assert rc(0, 0, 8) == 1 and rc(0, 8, -1) == 1
    torch.cuda.synchronize()


@pytest.mark.parametrize("gaussian", [True, False])
def test_blend_masked_equals_blend_times_mask(cuda, gaussian):
    from light_unet import _native as nat
    from light_unet.utils import _get_gaussian_importance_map
    rng = np.random.default_rng(11)
    shape = SHAPE
    zs, ys, xs = _grid(shape)
    nwin, P = len(zs) * len(ys) * len(xs), PATCH[0] * PATCH[1] * PATCH[2]
    assert nwin == 80
    preds = rng.random((nwin, P), dtype=np.float32)
    mask = np.zeros(shape, np.float32)
    mask[4:20, 10:30, :12] = rng.choice(np.float32([0.0, 0.5, 1.0, 2.0]), (16, 20, 12))
    mask[-1, -1, -1] = 1.0
    imp = _get_gaussian_importance_map(PATCH) if gaussian else np.ones(PATCH, np.float32)
    zt, yt, xt = (_dev_i32(v, cuda) for v in (zs, ys, xs))
    impt, preds_t = torch.from_numpy(imp).to(cuda), torch.from_numpy(preds).to(cuda)
    full = torch.empty(shape, device=cuda)
    nat.call("l3u_window_blend", preds_t.data_ptr(), zt.data_ptr(), len(zs), yt.data_ptr(), len(ys),
             xt.data_ptr(), len(xs), impt.data_ptr(), *shape, *PATCH, full.data_ptr(), nat.stream())
    full = full.cpu().numpy()
    for m in (mask, (mask != 0).astype(np.uint8)):
        kept = np.flatnonzero(_np_keep(m))
        assert 0 < len(kept) < nwin
        slot = np.full(nwin, -1, np.int32)
        slot[kept] = np.arange(len(kept), dtype=np.int32)
        compact = torch.from_numpy(preds[kept]).to(cuda)
        mt, st = torch.from_numpy(m).to(cuda), torch.from_numpy(slot).to(cuda)
        got = torch.full(shape, 7.0, device=cuda)
        nat.call("l3u_window_blend_masked", compact.data_ptr(), st.data_ptr(), zt.data_ptr(), len(zs),
                 yt.data_ptr(), len(ys), xt.data_ptr(), len(xs), impt.data_ptr(), mt.data_ptr(),
                 0 if m.dtype == np.float32 else 2, *shape, *PATCH, got.data_ptr(), nat.stream())
        want = full * m.astype(np.float32)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), m.dtype


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


@pytest.fixture(scope="module")
def e2e(cuda):
    """The seeded patch-16 model, one volume and its unmasked map (computed once, never changed)."""
    from light_unet.utils import sliding_window_inference_3d as sw
    model = _model(cuda)
    img = _volume(SHAPE, 5)
    ref = sw(img, model, PATCH, 0.5, cuda, True)
    ref.setflags(write=False)
    return model, img, ref, {}


def _e2e_masks():
    rng = np.random.default_rng(17)
    box = np.zeros(SHAPE, bool)
    box[:8, :8, :8] = True
    far = np.zeros(SHAPE, bool)
    far[-1, -1, -1] = True
    values = np.zeros(SHAPE, np.float32)
    values[8:30, :20, 20:] = rng.choice(np.float32([0.0, 0.5, 2.0]), (22, 20, 24))
    return {"box": box, "far_corner": far, "empty": np.zeros(SHAPE, bool),
            "full": np.ones(SHAPE, bool), "values": values}


def _as_input(m, kind, cuda):
    if m.dtype == np.float32:     # the float mask: numpy, device tensor, or a [1, D, H, W] array
        return [m, torch.from_numpy(m).to(cuda), m[None]][kind]
    return [m, torch.from_numpy(m.astype(np.uint8)).to(cuda), m.astype(np.int16)][kind]


@pytest.mark.parametrize("name", ["box", "far_corner", "empty", "full", "values"])
def test_masked_sliding_window_equals_product(cuda, e2e, name):
    from light_unet.utils import sliding_window_inference_3d as sw
    model, img, ref, cache = e2e
    m = _e2e_masks()[name]
    want = ref * m.astype(np.float32)
    windows, kept = 80, int(_np_keep(m).sum())
    for i, wb in enumerate((1, 5, 16)):        # mask input kinds and output modes rotate with it
        stats = {}
        out = ("numpy", "device")[(i + len(name)) % 2]
        got = sw(img, model, PATCH, 0.5, cuda, True, window_batch=wb, output=out,
                 forward_cache=cache, body_mask=_as_input(m, i, cuda), stats=stats)
        if out == "device":
            assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32
            got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == SHAPE
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, wb)
        assert stats == {"windows": windows, "kept": kept, "forwards": math.ceil(kept / wb)}
    if name in ("box", "far_corner"):
        assert kept == 1
    assert kept < windows or name == "full"
    assert (kept == 0) == (name == "empty")
    assert model.training
    # without a forward cache (the graph that holds the gather), both output modes
    for out in ("numpy", "device"):
        got = sw(img, model, PATCH, 0.5, cuda, True, window_batch=5, output=out, body_mask=m)
        got = got.cpu().numpy() if out == "device" else got
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, out)


def test_stats_without_mask(cuda, e2e):
    from light_unet.utils import sliding_window_inference_3d as sw
    model, img, ref, cache = e2e
    stats = {}
    got = sw(img, model, PATCH, 0.5, cuda, True, window_batch=16, forward_cache=cache, stats=stats)
    assert np.array_equal(got, ref)
    assert stats == {"windows": 80, "kept": 80, "forwards": 5}


def test_masked_call_reuses_the_cached_forward(cuda, e2e):
    from light_unet import utils
    sw = utils.sliding_window_inference_3d
    model, img, ref, _ = e2e
    m = _e2e_masks()["values"]
    cache = {}
    n0 = utils._CachedForward.captures
    a = sw(img, model, PATCH, 0.5, cuda, True, window_batch=4, forward_cache=cache)
    assert utils._CachedForward.captures == n0 + 1
    stats = {}
    b = sw(img, model, PATCH, 0.5, cuda, True, window_batch=4, forward_cache=cache, body_mask=m,
           stats=stats)
    assert utils._CachedForward.captures == n0 + 1 and len(cache) == 1
    assert stats["kept"] < stats["windows"]
    assert np.array_equal(a, ref) and np.array_equal(b, ref * m)
    # an empty mask: no forward and no capture, even on a cold cache
    cold, stats = {}, {}
    z = sw(img, model, PATCH, 0.5, cuda, True, forward_cache=cold, body_mask=np.zeros(SHAPE, bool),
           stats=stats)
    assert utils._CachedForward.captures == n0 + 1 and cold == {} and stats["forwards"] == 0
    assert z.dtype == np.float32 and not z.any()


def _golden_model(z, cuda):
    from light_unet.models.unet3d import Lightweight3DUNet
    m = Lightweight3DUNet()
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")})
    return m.to(cuda)


def _golden_mask(shape):
    m = np.ones(shape, np.float32)
    m[16:] = 0.0
    return m


def test_masked_sliding_window_at_patch_48(cuda, golden):
    """The workload's patch size on the reference's own map (sliding.npz, 2 x 2 x 2 windows)."""
    from light_unet.utils import sliding_window_inference_3d as sw
    z = golden("sliding.npz")
    model = _golden_model(z, cuda)
    ref = z["v64_56_72/prob"]
    mask = _golden_mask(ref.shape)
    stats = {}
    got = sw(z["v64_56_72/image"], model, (48, 48, 48), 0.5, cuda, True, body_mask=mask, stats=stats)
    assert stats == {"windows": 8, "kept": 4, "forwards": 1}
    np.testing.assert_allclose(got, ref * mask, atol=1e-5, rtol=0)
    assert not got[mask == 0].any() and got[mask != 0].min() > 0


def test_masked_sliding_window_sharded_over_ranks(cuda, golden, tmp_path):
    """Two ranks (gloo, both on this GPU) split the kept batches: the one-process masked map to
    the sharded tolerance of test_sliding_gpu.py, exact zeros outside the mask."""
    from light_unet.utils import sliding_window_inference_3d as sw
    z = golden("sliding.npz")
    mask = _golden_mask(z["v64_56_72/prob"].shape)
    np.save(tmp_path / "mask.npy", mask)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = tmp_path / "prob.npy"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tests", "_sliding_mask_dist_worker.py"), str(tmp_path / "mask.npy"),
           str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    prob = np.load(out)
    one = sw(z["v64_56_72/image"], _golden_model(z, cuda), (48, 48, 48), 0.5, cuda, True,
             window_batch=2, body_mask=mask)
    np.testing.assert_allclose(prob, one, atol=1e-5, rtol=0)
    assert not prob[mask == 0].any() and prob[mask != 0].min() > 0
    assert np.load(tmp_path / "prob.npy.forwards.npy").tolist() == [1, 1]   # one batch per rank


VAL_SHAPES = [(24, 28, 20), (20, 24, 28), (28, 20, 24)]
VAL_SPACINGS = [(4.0, 4.0, 4.0), (3.0, 4.0, 5.0), (2.0, 2.0, 2.0)]


def _val_cases():
    rng = np.random.default_rng(9)
    out = []
    for i, shape in enumerate(VAL_SHAPES):
        img = _volume(shape, 10 + i)
        lab = (_volume(shape, 20 + i) > 0.9).astype(np.float32)
        mask = np.ones(shape, np.float32)
        mask[rng.random(shape) < 0.05] = 0.0
        if i == 0:
            mask[8:] = 0.0            # empties the windows that start at z = 8
        if i == 1:
            mask[:2], mask[:, :, -3:] = 0.0, 0.0
        out.append((img, lab, mask))
    return out


def test_fast_validate_passes_the_mask_to_the_sliding_window(cuda, monkeypatch):
    import test_fast_validate_gpu as FV
    from light_unet import fast_trainer, lesion
    from light_unet.utils import sliding_window_inference_3d as sw
    model = _model(cuda)
    cases = _val_cases()
    maps = [sw(c[0], model, PATCH, 0.5, cuda, True) * c[2] for c in cases]
    labels = [c[1] for c in cases]
    allv = np.concatenate([m[c[2] > 0] for m, c in zip(maps, cases)])
    # float32 values, so the float64 comparisons of the float64-mask path decide alike
    thresholds = [float(np.float32(q)) for q in np.quantile(allv, [0.2, 0.4, 0.6, 0.8])]
    assert len(set(thresholds)) == 4

    # Trainer.validate written out: metrics per threshold, then the selection loop
    best_t = thresholds[0]
    ref = lesion.calculate_metrics(maps, labels, threshold=best_t, spacing=VAL_SPACINGS)
    best_r, best_d = ref["lesion_wise_recall"], ref["voxel_wise_dsc_macro"]
    for t in thresholds[1:]:
        m = lesion.calculate_metrics(maps, labels, threshold=t, spacing=VAL_SPACINGS)
        if FV._is_better(m["lesion_wise_recall"], m["voxel_wise_dsc_macro"], best_r, best_d, 0.01)[0]:
            best_r, best_d, best_t, ref = m["lesion_wise_recall"], m["voxel_wise_dsc_macro"], t, m
    ref.update(best_threshold=best_t, best_recall=best_r, best_dsc_macro=best_d)

    cls = type("MaskedValidateTrainer", (FV.StandInTrainer,), {"validate": lambda self, e: None})
    fast_trainer.bind_validate(cls)
    calls = []
    real_sw = fast_trainer.sliding_window_inference_3d

    def spy(**kw):
        st = {}
        out = real_sw(**kw, stats=st)
        calls.append((kw.get("body_mask"), st, out))
        return out
    monkeypatch.setattr(fast_trainer, "sliding_window_inference_3d", spy)

    def batches(dtype):
        f = lambda a: torch.from_numpy(a)[None, None]   # noqa: E731
        return [(f(img), f(lab), [f"{i:04d}"], torch.tensor([VAL_SPACINGS[i]]), f(mask.astype(dtype)))
                for i, (img, lab, mask) in enumerate(cases)]

    for dtype, masked_sw in ((np.float32, True), (np.uint8, True), (np.float64, False)):
        calls.clear()
        loss, got = cls(cuda, model, batches(dtype), thresholds).validate(0)
        assert loss == 0.0 and len(calls) == len(cases)
        for (bm, st, out), c, r in zip(calls, cases, maps):
            assert (bm is not None) == masked_sw, dtype
            q = out.cpu().numpy()
            assert np.array_equal(q if masked_sw else q * c[2], r)
        if masked_sw:
            assert calls[0][1]["kept"] < calls[0][1]["windows"]
        else:
            assert all(st["kept"] == st["windows"] for _, st, _ in calls)
        FV._same(got, ref)

    # masks switched off in the config: no mask reaches the sliding window
    calls.clear()
    cls(cuda, model, batches(np.float32), thresholds, masks_on=False).validate(0)
    assert all(bm is None for bm, _, _ in calls)


def test_infer_volume(cuda, e2e):
    from light_unet import inference, lesion
    model, img, ref, _ = e2e
    ref = ref.copy()
    mask = np.zeros(SHAPE, bool)
    mask[4:, :30, 6:40] = True
    mask[20:, :, :20] = False
    thr = float(np.quantile(ref[mask], 0.7))
    spacing = (4.0, 4.0, 4.0)
    cfg = {"data": {"patch_size": list(PATCH), "bbox_expansion_voxels": 2,
                    "volume_threshold": {"inference_cc": 0.5},
                    "body_mask": {"enabled": True, "apply_to_inference": True}},
           "validation": {"default_threshold": thr}}
    want_map = ref * mask
    want = lesion.extract_bboxes(want_map, thr, 0.5, spacing, 2)
    assert len(want) > 0
    for im, bm in ((img, mask), (torch.from_numpy(img).to(cuda), torch.from_numpy(mask).to(cuda))):
        got_map, got = inference.infer_volume(im, model, cfg, body_mask=bm, spacing=spacing)
        assert isinstance(got_map, np.ndarray) and got_map.dtype == np.float32
        assert np.array_equal(got_map, want_map) and got == want
    # an explicit threshold and a forward cache
    cache = {}
    got_map, got = inference.infer_volume(img, model, cfg, body_mask=mask, spacing=(2.0, 3.0, 4.0),
                                          threshold=0.9 * thr, forward_cache=cache)
    assert len(cache) == 1 and np.array_equal(got_map, want_map)
    assert got == lesion.extract_bboxes(want_map, 0.9 * thr, 0.5, (2.0, 3.0, 4.0), 2)
    # the mask is the reference's decision: without apply_to_inference it is ignored
    for bm_cfg in ({"enabled": True, "apply_to_inference": False}, {"apply_to_inference": True}, {}):
        cfg2 = {"data": dict(cfg["data"], body_mask=bm_cfg), "validation": cfg["validation"]}
        got_map, got = inference.infer_volume(img, model, cfg2, body_mask=mask, spacing=spacing)
        assert np.array_equal(got_map, ref)
        assert got == lesion.extract_bboxes(ref, thr, 0.5, spacing, 2)
    with pytest.raises(ValueError):     # a float64 product is not this path's
        inference.infer_volume(img, model, cfg, body_mask=mask.astype(np.float64), spacing=spacing)
