"""Device-resident validation: fast_trainer.evaluate_maps against the reference Trainer.validate's
stored results (tests/golden/validate.npz), the sliding window's device / cache keywords, and
fast_trainer.validate end to end against the composition of the existing public functions."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-8


def _is_better(recall, dsc, best_recall, best_dsc, tie_threshold):
    """Trainer._is_better_metric (trainer.py:183-189)."""
    tie_margin = tie_threshold + EPS
    if recall > best_recall + EPS:
        return True, True
    if abs(recall - best_recall) <= tie_margin and dsc > best_dsc + EPS:
        return True, False
    return False, False


def _same(got, ref):
    assert set(got) == set(ref)
    for k, v in ref.items():
        assert got[k] == v, (k, got[k], v)


def test_evaluate_maps_equals_reference_validate(cuda, golden):
    from light_unet import fast_trainer
    z = golden("validate.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    n = len(meta["shapes"])
    probs = [z[f"case{i}/prob"] for i in range(n)]
    labels = [z[f"case{i}/label"].astype(np.float32) for i in range(n)]
    masks = [z[f"case{i}/mask"].astype(np.float32) for i in range(n)]
    spacings = [tuple(s) for s in meta["spacings"]]
    chosen = []
    for run in meta["validate_masked"]:
        best = fast_trainer.evaluate_maps([torch.from_numpy(p).to(cuda) for p in probs], labels,
                                          spacings, meta["thresholds"], run["tie_threshold"],
                                          _is_better, body_masks=masks)
        _same(best, run["result"])
        chosen.append(best["best_threshold"])
    assert chosen[0] != chosen[1]
    for run in meta["validate_plain"]:
        best = fast_trainer.evaluate_maps(probs, labels, spacings, meta["thresholds"],
                                          run["tie_threshold"], _is_better)
        _same(best, run["result"])


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


def test_sliding_window_device_and_cache_keywords(cuda):
    from light_unet import utils
    sw = utils.sliding_window_inference_3d
    model = _model(cuda)
    a, b = _volume((24, 28, 20), 1), _volume((28, 20, 24), 2)
    ref_a = sw(a, model, (16, 16, 16), 0.5, cuda, True, window_batch=4)
    ref_b = sw(b, model, (16, 16, 16), 0.5, cuda, True, window_batch=4)
    assert isinstance(ref_a, np.ndarray) and ref_a.dtype == np.float32
    dev_a = sw(a, model, (16, 16, 16), 0.5, cuda, True, window_batch=4, output="device")
    assert isinstance(dev_a, torch.Tensor) and dev_a.is_cuda and dev_a.dtype == torch.float32
    assert np.array_equal(dev_a.cpu().numpy(), ref_a)
    from_dev = sw(torch.from_numpy(a).to(cuda), model, (16, 16, 16), 0.5, cuda, True, window_batch=4)
    assert np.array_equal(from_dev, ref_a)
    cache = {}
    n0 = utils._CachedForward.captures
    got_a = sw(a, model, (16, 16, 16), 0.5, cuda, True, window_batch=4, forward_cache=cache)
    assert utils._CachedForward.captures == n0 + 1 and len(cache) == 1
    fwd = next(iter(cache.values()))
    x_ptr, flat_ptr = fwd.x.data_ptr(), fwd.flat.data_ptr()
    got_b = sw(torch.from_numpy(b).to(cuda), model, (16, 16, 16), 0.5, cuda, True, window_batch=4,
               forward_cache=cache, output="device")
    assert utils._CachedForward.captures == n0 + 1 and len(cache) == 1     # no new capture
    assert next(iter(cache.values())) is fwd
    assert fwd.x.data_ptr() == x_ptr and fwd.flat.data_ptr() == flat_ptr
    assert flat_ptr == model.flat_parameters().data_ptr()
    assert np.array_equal(got_a, ref_a)
    assert np.array_equal(got_b.cpu().numpy(), ref_b)
    with pytest.raises(ValueError):
        sw(a, model, (16, 16, 16), 0.5, cuda, True, output="host")
    assert model.training


class StandInTrainer:
    """The attributes Trainer.validate reads (trainer.py:349-445)."""
    EPS = EPS

    def __init__(self, cuda, model, batches, thresholds, masks_on=True, tie=0.01):
        self.device, self.model, self.val_loader = cuda, model, batches
        self.config = {"validation": {"default_threshold": 0.3,
                                      "threshold_sensitivity_range": list(thresholds)},
                       "data": {"patch_size": [16, 16, 16],
                                "body_mask": {"enabled": masks_on, "apply_to_validation": masks_on},
                                "spacing": {"target": [4.0, 4.0, 4.0]}},
                       "metrics": {"model_selection": {"tie_threshold": tie}}}
        self.better_calls = 0

    def _is_better_metric(self, recall, dsc, best_recall, best_dsc, tie_threshold):
        self.better_calls += 1
        return _is_better(recall, dsc, best_recall, best_dsc, tie_threshold)

    def _get_target_spacing(self):
        return tuple(self.config["data"]["spacing"]["target"])

    def _resolve_spacing_value(self, spacings, index, target_spacing):
        v = spacings[index] if len(spacings) > index else target_spacing
        if isinstance(v, torch.Tensor):
            v = v.tolist()
        return tuple(float(s) for s in v)


SHAPES = [(24, 28, 20), (20, 24, 28), (28, 20, 24)]
SPACINGS = [(4.0, 4.0, 4.0), (3.0, 4.0, 5.0), (2.0, 2.0, 2.0)]


def _cases():
    rng = np.random.default_rng(9)
    out = []
    for i, shape in enumerate(SHAPES):
        img = _volume(shape, 10 + i)
        lab = (_volume(shape, 20 + i) > 0.9).astype(np.float32)
        mask = np.ones(shape, np.float32)
        mask[:2], mask[:, :, -3:] = 0.0, 0.0
        mask[rng.random(shape) < 0.05] = 0.0
        out.append((img, lab, mask))
    return out


def _slow_path(model, cuda, cases, thresholds, spacings, masks_on, tie):
    """Trainer.validate written out with the existing public functions: sliding window -> numpy
    -> mask -> lesion.calculate_metrics per threshold -> the selection loop."""
    from light_unet import lesion
    from light_unet.utils import sliding_window_inference_3d
    maps = []
    for img, _, mask in cases:
        p = sliding_window_inference_3d(image=img, model=model, patch_size=(16, 16, 16), overlap=0.5,
                                        device=cuda, use_gaussian=True)
        maps.append(p * mask if masks_on else p)
    labels = [c[1] for c in cases]
    best_t = thresholds[0]
    best = lesion.calculate_metrics(maps, labels, threshold=best_t, spacing=spacings)
    best_r, best_d = best["lesion_wise_recall"], best["voxel_wise_dsc_macro"]
    for t in thresholds[1:]:
        m = lesion.calculate_metrics(maps, labels, threshold=t, spacing=spacings)
        if _is_better(m["lesion_wise_recall"], m["voxel_wise_dsc_macro"], best_r, best_d, tie)[0]:
            best_r, best_d, best_t, best = m["lesion_wise_recall"], m["voxel_wise_dsc_macro"], t, m
    best.update(best_threshold=best_t, best_recall=best_r, best_dsc_macro=best_d)
    return maps, best


def test_fast_validate_end_to_end(cuda, monkeypatch):
    from light_unet import fast_trainer, utils
    model = _model(cuda)
    cases = _cases()
    # thresholds from the slow path's own (masked) maps, so every level has components
    maps0, _ = _slow_path(model, cuda, cases, [0.5], SPACINGS, True, 0.01)
    allv = np.concatenate([m[c[2] > 0] for m, c in zip(maps0, cases)])
    thresholds = [float(q) for q in np.quantile(allv, [0.2, 0.4, 0.6, 0.8])]
    assert len(set(np.float32(thresholds))) == 4

    cls = type("FastValidateTrainer", (StandInTrainer,), {"validate": lambda self, e: "reference"})
    fast_trainer.bind_validate(cls)
    assert cls._l3u_reference_validate(None, 0) == "reference"

    seen = []
    real_sw = fast_trainer.sliding_window_inference_3d

    def spy(**kw):
        out = real_sw(**kw)
        seen.append(out)
        return out
    monkeypatch.setattr(fast_trainer, "sliding_window_inference_3d", spy)

    def t5(i, img, lab, mask):
        f = lambda a: torch.from_numpy(a)[None, None]   # noqa: E731
        return (f(img), f(lab), [f"{i:04d}"], torch.tensor([SPACINGS[i]]), f(mask))
    five = [t5(i, *c) for i, c in enumerate(cases)]
    four = [(torch.from_numpy(c[0])[None], torch.from_numpy(c[1])[None], [f"{i:04d}"],
             torch.tensor([SPACINGS[i]])) for i, c in enumerate(cases)]           # ndim 4, no masks

    for batches, masks_on in ((five, True), (four, False)):
        ref_maps, ref = _slow_path(model, cuda, cases, thresholds, SPACINGS, masks_on, 0.01)
        tr = cls(cuda, model, batches, thresholds, masks_on=masks_on)
        n0 = utils._CachedForward.captures
        for epoch in (0, 1):         # the second epoch runs on warm caches
            seen.clear()
            tr.better_calls = 0
            loss, got = tr.validate(epoch)
            assert loss == 0.0 and tr.better_calls == len(thresholds) - 1
            assert len(seen) == len(cases)
            for p, c, r in zip(seen, cases, ref_maps):      # the maps first, bitwise
                assert p.is_cuda
                q = p.cpu().numpy()
                assert np.array_equal(q * c[2] if masks_on else q, r)
            _same(got, ref)
        assert utils._CachedForward.captures - n0 <= 2      # one per window batch size, not per case
        assert len(tr._l3u_validate["targets"]) == len(cases)

    # a 2-tuple batch: target spacing, no ids (cache keyed by position)
    two = [(b[0], b[1]) for b in five]
    _, ref = _slow_path(model, cuda, cases, thresholds, [(4.0, 4.0, 4.0)] * 3, False, 0.01)
    tr = cls(cuda, model, two, thresholds, masks_on=True)
    _same(tr.validate(0)[1], ref)
    assert set(tr._l3u_validate["targets"]) == {("pos", i) for i in range(3)}

    # an empty loader: the reference's zero dict
    loss, got = cls(cuda, model, [], thresholds).validate(0)
    assert loss == 0.0 and got == {
        "lesion_wise_recall": 0.0, "lesion_wise_precision": 0.0, "voxel_wise_dsc_macro": 0.0,
        "voxel_wise_dsc_micro": 0.0, "fp_per_case": 0.0, "best_threshold": 0.3, "best_recall": 0.0,
        "best_dsc_macro": 0.0}
