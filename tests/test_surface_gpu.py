"""Surface-distance metrics on the device (light_unet/surface.py, csrc/surface.hip) against scipy's
stored results (tests/golden/surface.npz, written by tests/golden/make_surface_goldens.py)."""
import numpy as np
import pytest
import torch

import surface_fixture as fx

pytestmark = pytest.mark.gpu


def _pack(mask, cuda):
    from light_unet import preprocess as pp
    return pp.pack(torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(cuda))


def _edt(bits, shape, spacing, passes=7):
    from light_unet import _native as nat
    out = torch.empty(shape, dtype=torch.float64, device=bits.device)
    tmp = torch.empty_like(out)
    nat.call("l3u_edt", bits.data_ptr(), *(float(s) for s in spacing), out.data_ptr(), tmp.data_ptr(),
             *shape, passes, nat.stream())
    return out.cpu().numpy()


def test_edt_equals_every_golden_map_bit_for_bit(cuda):
    z, index = fx.load()
    assert len(index["edt"]) >= 30
    packed = {}
    for e in index["edt"]:
        shape = tuple(e["shape"])
        if e["feat"] not in packed:
            packed[e["feat"]] = _pack(fx.mask(e["feat"], shape), cuda)
        got = _edt(packed[e["feat"]], shape, e["spacing"])
        ref = z[e["map"]]
        differ = int((got.view(np.uint64) != ref.view(np.uint64)).sum())
        assert differ == 0, (e["map"], differ)


@pytest.mark.parametrize("shape", [(5, 9, 70), (1, 1, 5), (3, 40, 129), (2, 3, 600), (2, 600, 3)])
def test_edt_without_and_with_only_features(cuda, shape):
    none = _edt(_pack(np.zeros(shape, bool), cuda), shape, (3.27, 2.0364, 2.0364))
    assert none.shape == shape and np.all(np.isposinf(none))
    every = _edt(_pack(np.ones(shape, bool), cuda), shape, (3.27, 2.0364, 2.0364))
    assert np.array_equal(every.view(np.uint64), np.zeros(shape, np.uint64))


def test_distance_transform_edt_wrapper(cuda):
    from light_unet import surface
    z, index = fx.load()
    e = next(e for e in index["edt"] if e["shape"] == [5, 9, 70] and e["spacing"][0] == 3.27
             and e["map"].endswith("d0_s2"))
    shape = tuple(e["shape"])
    vol = ~fx.mask(e["feat"], shape)                 # scipy's input: the distance to the zeros
    ref = z[e["map"]]
    got = surface.distance_transform_edt(vol, sampling=e["spacing"])
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))
    for arr in (vol.astype(np.uint8), vol.astype(np.float32) * 0.25, vol):
        a = surface.distance_transform_edt(arr, sampling=e["spacing"])
        b = surface.distance_transform_edt(torch.from_numpy(arr).to(cuda), sampling=e["spacing"])
        assert np.array_equal(a.view(np.uint64), ref.view(np.uint64)), arr.dtype
        assert np.array_equal(b.view(np.uint64), ref.view(np.uint64)), arr.dtype
    dev = surface.distance_transform_edt(torch.from_numpy(vol).to(cuda), sampling=e["spacing"],
                                         output="device")
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float64
    assert np.array_equal(dev.cpu().numpy().view(np.uint64), ref.view(np.uint64))
    # the default sampling is scipy's (1, 1, 1)
    e1 = next(x for x in index["edt"] if x["feat"] == e["feat"] and x["spacing"] == [1.0, 1.0, 1.0])
    assert np.array_equal(surface.distance_transform_edt(vol).view(np.uint64),
                          z[e1["map"]].view(np.uint64))


def _tags(index):
    seen = {}
    for m in index["metrics"]:
        seen.setdefault(m["tag"], tuple(m["shape"]))
    return seen


def test_surface_mask_equals_scipy(cuda):
    from light_unet import preprocess as pp
    from light_unet import surface
    _, index = fx.load()
    tags = _tags(index)
    assert {"faces", "full", "a", "b"} <= set(tags)
    for tag, shape in tags.items():
        for side in ("pred", "target"):
            m = fx.mask(f"m_{tag}_{side}", shape)
            bits = surface.surface_mask(m if side == "pred" else torch.from_numpy(m).to(cuda))
            assert bits.dtype == torch.int64 and tuple(bits.shape) == (shape[0], shape[1],
                                                                       (shape[2] + 63) // 64)
            got = pp.unpack(bits, shape, torch.bool).cpu().numpy()
            assert np.array_equal(got, fx.mask(f"m_{tag}_s{side}", shape)), (tag, side)


def test_surface_distances_equal_the_golden_dicts(cuda):
    from light_unet import surface
    _, index = fx.load()
    held = {}
    for m in index["metrics"]:
        shape = tuple(m["shape"])
        if m["tag"] not in held:
            held[m["tag"]] = tuple(torch.from_numpy(fx.mask(f"m_{m['tag']}_{s}", shape)).to(cuda)
                                   for s in ("pred", "target"))
        pred, target = held[m["tag"]]
        got = surface.surface_distances(pred, target, spacing=m["spacing"],
                                        tolerances_mm=m["tolerances"], percentile=m["percentile"])
        exp = fx.unhex(m["expected"])
        assert exp["n_pred"] <= 1 << 18 and exp["n_target"] <= 1 << 18
        print(m["tag"], m["spacing"], m["percentile"], got)
        fx.check_metrics(got, exp)
    # numpy inputs give the same dict
    m = next(m for m in index["metrics"] if m["tag"] == "crop")
    shape = tuple(m["shape"])
    got = surface.surface_distances(fx.mask("m_crop_pred", shape).astype(np.float32),
                                    fx.mask("m_crop_target", shape).astype(np.uint8),
                                    spacing=m["spacing"], tolerances_mm=m["tolerances"],
                                    percentile=m["percentile"])
    fx.check_metrics(got, fx.unhex(m["expected"]))


def test_surface_distances_repeat_bit_for_bit(cuda):
    from light_unet import surface
    pred = torch.from_numpy(fx.mask("m_b_pred", (64, 56, 72))).to(cuda)
    target = torch.from_numpy(fx.mask("m_b_target", (64, 56, 72))).to(cuda)
    kw = dict(spacing=(3.27, 2.0364, 2.0364), tolerances_mm=(2.0, 4.0, 7.5))
    a = surface.surface_distances(pred, target, **kw)
    b = surface.surface_distances(pred, target, **kw)
    assert a == b and np.float64(a["assd"]).view(np.uint64) == np.float64(b["assd"]).view(np.uint64)


def _sweep_inputs():
    z, index = fx.load()
    s = index["sweep"]
    shape = tuple(s["shape"])
    levels = np.asarray(s["levels"], dtype=np.float32)
    probs = [levels[z[f"sweep_level_{i}"]] for i in range(s["cases"])]
    labels = [fx.mask(f"sweep_target_{i}", shape).astype(np.float32) for i in range(s["cases"])]
    return s, probs, labels


def test_case_surface_metrics_equals_one_call_per_threshold(cuda):
    from light_unet import surface
    s, probs, labels = _sweep_inputs()
    kw = dict(spacing=s["spacing"], tolerances_mm=s["tolerances"], percentile=s["percentile"])
    got = surface.case_surface_metrics(torch.from_numpy(probs[0]).to(cuda), labels[0],
                                       s["thresholds"], **kw)
    assert len(got) == 3
    for g, thr, exp in zip(got, s["thresholds"], s["per_case"][0]):
        one = surface.surface_distances(probs[0] >= np.float32(thr), labels[0] >= 0.5, **kw)
        assert g == one, (thr, g, one)
        fx.check_metrics(g, fx.unhex(exp))
    # a body mask multiplies the map in float32 before the comparison
    mask = np.ones(probs[0].shape, np.float32)
    mask[:, :26] = 0.0
    got = surface.case_surface_metrics(probs[0], labels[0], s["thresholds"], body_mask=mask, **kw)
    for g, thr in zip(got, s["thresholds"]):
        one = surface.surface_distances((probs[0] * mask) >= np.float32(thr), labels[0] >= 0.5, **kw)
        assert g == one, (thr, g, one)


def test_sweep_metrics_surface_keys(cuda):
    from light_unet import lesion
    s, probs, labels = _sweep_inputs()
    dev = [torch.from_numpy(p).to(cuda) for p in probs]
    plain = lesion.sweep_metrics(dev, labels, s["thresholds"], spacing=tuple(s["spacing"]))
    none = lesion.sweep_metrics(dev, labels, s["thresholds"], spacing=tuple(s["spacing"]),
                                surface=None)
    assert len(plain) == len(none) == 3
    for a, b in zip(plain, none):
        assert set(a) == set(b) and not set(fx.SWEEP_KEYS) & set(a)
        for k in a:
            assert a[k] == b[k], k
    got = lesion.sweep_metrics(dev, labels, s["thresholds"], spacing=tuple(s["spacing"]),
                               surface={"tolerances_mm": s["tolerances"],
                                        "percentile": s["percentile"]})
    for g, a, exp in zip(got, plain, s["expected"]):
        assert set(g) == set(a) | set(fx.SWEEP_KEYS)
        for k in a:
            assert g[k] == a[k], k
        fx.check_sweep(g, fx.unhex(exp))
    assert got[0]["surface_cases"] == 2          # one of the three targets is empty


def test_validate_passes_surface_metrics_through(cuda):
    """Trainer.validate as l3u_plugin.install(fast_validate=True) binds it
    (fast_trainer.bind_validate), on the stand-in of tests/test_fast_validate_gpu.py at its
    smallest case: with validation.surface_metrics the returned dict carries the extra keys, and
    they are what sweep_metrics gives for the same maps."""
    from light_unet import fast_trainer, lesion
    from test_fast_validate_gpu import SPACINGS, StandInTrainer, _cases, _model
    model = _model(cuda)
    case = _cases()[0]
    batch = [(torch.from_numpy(case[0])[None], torch.from_numpy(case[1])[None], ["0000"],
              torch.tensor([SPACINGS[0]]))]
    cfg = {"tolerances_mm": [4.0, 8.0], "percentile": 95.0}
    cls = type("SurfaceValidateTrainer", (StandInTrainer,), {"validate": lambda self, e: "reference"})
    fast_trainer.bind_validate(cls)
    seen = []
    real_sw = fast_trainer.sliding_window_inference_3d

    def spy(**kw):
        seen.append(real_sw(**kw))
        return seen[-1]
    plain = cls(cuda, model, batch, [0.5], masks_on=False).validate(0)[1]
    assert not set(fx.SWEEP_KEYS) & set(plain)
    tr = cls(cuda, model, batch, [0.5], masks_on=False)
    tr.config["validation"]["surface_metrics"] = cfg
    fast_trainer.sliding_window_inference_3d = spy
    try:
        got = tr.validate(0)[1]
    finally:
        fast_trainer.sliding_window_inference_3d = real_sw
    assert set(got) == set(plain) | set(fx.SWEEP_KEYS)
    for k in plain:
        assert got[k] == plain[k], k
    ref = lesion.sweep_metrics(seen, [case[1]], [0.5], spacing=[SPACINGS[0]], surface=cfg)[0]
    for k in fx.SWEEP_KEYS:
        assert got[k] == ref[k] or (got[k] != got[k] and ref[k] != ref[k]), k
    assert len(got["nsd_mean"]) == 2
