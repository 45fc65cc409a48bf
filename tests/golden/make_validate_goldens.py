"""Golden fixture for the validation threshold sweep, made by the REFERENCE's own code on the CPU.

Run where the reference checkout exists (L3U_REFERENCE, default /root/reference) with
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_validate_goldens.py
It imports the reference package unmodified (`light_unet.models.metrics`,
`light_unet.core.trainer`) with the two I/O stand-ins of make_loop_goldens.py (nibabel,
torch.utils.tensorboard) and writes tests/golden/validate.npz, data only:

  * six synthetic cases (five of unequal shapes near (24, 28, 20), one (40, 36, 44)): a smooth
    float32 blob probability map whose components merge and split across the seven thresholds
    0.1 .. 0.7 of the reference configs, a binary label, a body mask and a spacing per case.
    Several voxels per case sit exactly at float32(t) and at the next float32 below t.  Case 2 has
    an empty target, case 3 stays below the top threshold (no prediction there), case 4 lies
    above the lowest threshold everywhere (one component: the whole volume; its mask is all ones);
  * `metrics.calculate_metrics` of the reference at each threshold, with `prob * mask` (numpy
    float32, as trainer.py:401-402 forms it) and with the plain maps;
  * the return value of the reference `Trainer.validate` itself (trainer.py:349-445) on a Trainer
    whose `val_loader` yields these cases as 5-tuples and whose module-level
    `sliding_window_inference_3d` is replaced by a function that replays the stored maps, for two
    `tie_threshold` values that choose different thresholds, and once for 4-tuple batches (no
    masks).
The JSON part (dicts, thresholds, spacings) is stored as a uint8 array `meta`.
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

REF = os.environ.get("L3U_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
THRESHOLDS = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7]
SHAPES = [(24, 28, 20), (20, 24, 28), (28, 20, 24), (24, 24, 24), (22, 26, 21), (40, 36, 44)]
SPACINGS = [(4.0, 4.0, 4.0), (3.0, 4.0, 5.0), (4.0, 2.5, 2.5), (2.0, 2.0, 2.0), (5.0, 4.0, 3.0),
            (4.0, 4.0, 4.0)]
EMPTY_TARGET, BELOW_TOP, WHOLE_VOLUME = 2, 3, 4
TIES = [0.0, 0.01, 0.05, 0.1, 0.2, 0.3, 0.5, 1.0]


def _install_stubs():
    nib = types.ModuleType("nibabel")
    nib.load = lambda path: None
    sys.modules["nibabel"] = nib
    tb = types.ModuleType("torch.utils.tensorboard")

    class SummaryWriter:
        def __init__(self, *a, **k):
            pass

        def add_scalar(self, *a, **k):
            pass

        def close(self):
            pass
    tb.SummaryWriter = SummaryWriter
    sys.modules["torch.utils.tensorboard"] = tb


def _case(i, shape, rng):
    zz, yy, xx = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    nblob = 6 if max(shape) < 40 else 14
    prob = np.zeros(shape, np.float64)
    label = np.zeros(shape, np.uint8)
    for b in range(nblob):
        c = [rng.uniform(3, s - 3) for s in shape]
        sig = rng.uniform(1.5, 3.5)
        amp = rng.uniform(0.25, 0.95)
        r2 = (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2
        prob = np.maximum(prob, amp * np.exp(-r2 / (2 * sig ** 2)))
        if b % 2 == 0:   # a target lesion near every other blob, shifted a little
            d = rng.uniform(-1.0, 1.0, size=3)
            label[(zz - c[0] - d[0]) ** 2 + (yy - c[1] - d[1]) ** 2 + (xx - c[2] - d[2]) ** 2
                  <= (sig * rng.uniform(0.5, 0.8)) ** 2] = 1
    prob = prob + 0.04 * rng.random(shape)          # ragged rims: small components at low levels
    if i == BELOW_TOP:
        prob = prob * (0.65 / prob.max())
    if i == WHOLE_VOLUME:
        prob = 0.12 + 0.85 * prob
    if i == EMPTY_TARGET:
        label[:] = 0
    prob = np.clip(prob, 0.0, 0.999).astype(np.float32)
    # voxels exactly at float32(t) and one float32 below it
    flat = prob.reshape(-1)
    picks = rng.choice(flat.size, size=2 * 4, replace=False)
    for j, t in enumerate((0.1, 0.3, 0.5, 0.7)):
        if i == BELOW_TOP and t == 0.7:
            continue
        t32 = np.float32(t)
        below = np.nextafter(t32, np.float32(0.0))
        if i == WHOLE_VOLUME and t == 0.1:
            below = t32   # keep the whole volume above the lowest threshold
        flat[picks[2 * j]] = t32
        flat[picks[2 * j + 1]] = below
    if i == WHOLE_VOLUME:
        mask = np.ones(shape, np.uint8)
    else:
        ctr = [(s - 1) / 2.0 for s in shape]
        mask = (((zz - ctr[0]) / (0.48 * shape[0])) ** 2 + ((yy - ctr[1]) / (0.45 * shape[1])) ** 2
                + ((xx - ctr[2]) / (0.47 * shape[2])) ** 2 <= 1.0).astype(np.uint8)
    return prob, label, mask


def _jsonable(d):
    out = {}
    for k, v in d.items():
        out[k] = int(v) if isinstance(v, (int, np.integer)) and not isinstance(v, bool) else float(v)
    return out


def main():
    _install_stubs()
    sys.path.insert(0, REF)
    from light_unet.models import metrics as M
    from light_unet.core import trainer as TR

    rng = np.random.default_rng(20261019)
    out, meta = {}, {"thresholds": THRESHOLDS, "spacings": [list(s) for s in SPACINGS],
                     "shapes": [list(s) for s in SHAPES], "empty_target": EMPTY_TARGET,
                     "below_top": BELOW_TOP, "whole_volume": WHOLE_VOLUME}
    probs, labels, masks = [], [], []
    for i, shape in enumerate(SHAPES):
        p, l, m = _case(i, shape, rng)
        probs.append(p), labels.append(l), masks.append(m)
        out[f"case{i}/prob"], out[f"case{i}/label"], out[f"case{i}/mask"] = p, l, m
    assert labels[EMPTY_TARGET].sum() == 0
    assert probs[BELOW_TOP].max() < np.float32(0.7)
    assert probs[WHOLE_VOLUME].min() >= np.float32(0.1)

    lab32 = [l.astype(np.float32) for l in labels]
    masked = [p * m.astype(np.float32) for p, m in zip(probs, masks)]   # float32 product
    assert all(a.dtype == np.float32 for a in masked)
    spacing = [tuple(s) for s in SPACINGS]
    meta["metrics_plain"] = [_jsonable(M.calculate_metrics(probs, lab32, threshold=t, spacing=spacing))
                             for t in THRESHOLDS]
    meta["metrics_masked"] = [_jsonable(M.calculate_metrics(masked, lab32, threshold=t, spacing=spacing))
                              for t in THRESHOLDS]

    # ---- Trainer.validate itself, with the sliding window replaced by a replay of the maps
    def make_trainer(tie, with_masks):
        t = object.__new__(TR.Trainer)   # validate() reads only the attributes set here
        t.config = {"validation": {"default_threshold": 0.3,
                                   "threshold_sensitivity_range": list(THRESHOLDS)},
                    "data": {"patch_size": [16, 16, 16],
                             "body_mask": {"enabled": True, "apply_to_validation": True},
                             "spacing": {"target": [4.0, 4.0, 4.0]}},
                    "metrics": {"model_selection": {"tie_threshold": tie}}}
        t.model = torch.nn.Identity()
        t.device = torch.device("cpu")
        batches = []
        for i in range(len(SHAPES)):
            b = [torch.from_numpy(probs[i])[None, None], torch.from_numpy(lab32[i])[None, None],
                 [f"{i:04d}"], torch.tensor([SPACINGS[i]], dtype=torch.float64)]
            if with_masks:
                b.append(torch.from_numpy(masks[i].astype(np.float32))[None, None])
            batches.append(tuple(b))
        t.val_loader = batches
        return t

    calls = {"n": 0}

    def replay(image, model, patch_size, overlap, device, use_gaussian):
        i = calls["n"] % len(SHAPES)
        calls["n"] += 1
        assert tuple(image.shape) == SHAPES[i]
        return probs[i].copy()
    TR.sliding_window_inference_3d = replay

    runs = {}
    for tie in TIES:
        _, best = make_trainer(tie, True).validate(0)
        runs[tie] = _jsonable(best)
    chosen = {tie: r["best_threshold"] for tie, r in runs.items()}
    print("best thresholds per tie_threshold:", chosen)
    first = 0.01
    other = next(t for t in TIES if chosen[t] != chosen[first])   # a tie that changes the choice
    meta["validate_masked"] = [{"tie_threshold": first, "result": runs[first]},
                               {"tie_threshold": other, "result": runs[other]}]
    _, best = make_trainer(first, False).validate(0)
    meta["validate_plain"] = [{"tie_threshold": first, "result": _jsonable(best)}]

    for name in ("metrics_plain", "metrics_masked"):
        print(name, [(m["tp"], m["fp"], m["fn"], round(m["lesion_wise_recall"], 3),
                      round(m["voxel_wise_dsc_macro"], 3)) for m in meta[name]])
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    path = os.path.join(OUT, "validate.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
