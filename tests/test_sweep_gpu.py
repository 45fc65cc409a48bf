"""The validation threshold sweep on the device: l3u_thr_levels, the level-batched labelling /
statistics / overlap counts and lesion.sweep_metrics, against numpy, the per-threshold path
(lesion.label / calculate_metrics), the CPU labelling and the reference results stored in
tests/golden/validate.npz.  Integer work: everything is compared exactly."""
import json

import numpy as np
import pytest
import torch

from oracle import lesion_oracle as L

pytestmark = pytest.mark.gpu

THR7 = np.asarray([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7], np.float32)


def _thr(K):
    if K == 1:
        return np.asarray([0.3], np.float32)
    if K == 7:
        return THR7
    return np.linspace(0.02, 0.95, K).astype(np.float32)


def _blobs(shape, seed, nblob=5):
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    p = np.zeros(shape)
    for _ in range(nblob):
        c = [rng.uniform(1, s - 1) for s in shape]
        r2 = (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2
        p = np.maximum(p, rng.uniform(0.3, 0.98) * np.exp(-r2 / (2 * rng.uniform(1.2, 3.5) ** 2)))
    return np.clip(p + 0.05 * rng.random(shape), 0, 0.999).astype(np.float32)


def _np_levels(p, thr, mask, target):
    q = p if mask is None else p * mask
    assert q.dtype == np.float32
    with np.errstate(invalid="ignore"):
        level = sum((q >= t).astype(np.uint8) for t in thr)
    tb = (target >= 0.5).astype(np.int64) if target is not None else np.zeros(p.shape, np.int64)
    hist = np.zeros((len(thr) + 1, 2), np.int64)
    np.add.at(hist, (level.reshape(-1).astype(np.int64), tb.reshape(-1)), 1)
    return level, hist, q


@pytest.mark.parametrize("shape", [(13, 9, 7), (40, 36, 44)])
@pytest.mark.parametrize("K", [1, 7, 32])
def test_thr_levels_match_numpy(cuda, shape, K):
    from light_unet import lesion
    thr = _thr(K)
    rng = np.random.default_rng(K * 100 + shape[0])
    p = _blobs(shape, seed=K + shape[0])
    flat = p.reshape(-1)
    idx = rng.choice(flat.size, size=2 * len(thr) + 1, replace=False)
    for k, t in enumerate(thr):          # exactly at the threshold and one float32 below
        flat[idx[2 * k]] = t
        flat[idx[2 * k + 1]] = np.nextafter(t, np.float32(0))
    flat[idx[-1]] = np.nan
    mask = (rng.random(shape) < 0.8).astype(np.float32)
    mask[rng.random(shape) < 0.1] = 0.5          # a real product, not only 0 / 1
    target = (rng.random(shape) < 0.2).astype(np.float32)
    pd, md, td = (torch.from_numpy(a).to(cuda) for a in (p, mask, target))
    for m_np, m_d in ((None, None), (mask, md)):
        for t_np, t_d in ((None, None), (target, td)):
            level, hist, masked = lesion.level_map(pd, thr, mask=m_d, target=t_d, want_masked=True)
            ref_level, ref_hist, ref_q = _np_levels(p, thr, m_np, t_np)
            assert np.array_equal(level.cpu().numpy(), ref_level)
            assert np.array_equal(hist.cpu().numpy(), ref_hist)
            assert np.array_equal(masked.cpu().numpy(), ref_q, equal_nan=True)
            assert int(hist.sum()) == p.size
    assert level.cpu().numpy().reshape(-1)[idx[-1]] == 0      # NaN: below every threshold


def _level_inputs():
    rng = np.random.default_rng(3116)
    out = {}
    # 32^3 site percolation: the random field binarised at 1 - 0.3116 is at the critical density
    f = rng.random((32, 32, 32)).astype(np.float32)
    out["percolation32"] = (f, np.asarray([0.5, 1 - 0.3116, 0.8, 0.9], np.float32))
    out["blobs40"] = (_blobs((40, 36, 44), 1, nblob=12), THR7)
    out["blobs13"] = (_blobs((13, 9, 7), 2, nblob=3), THR7)
    # lowest level = the whole volume (one component), top level = nothing
    g = np.clip(_blobs((13, 9, 7), 5, nblob=3), 0.15, 0.6)
    out["whole_and_empty"] = (g, np.asarray([0.1, 0.3, 0.5, 0.7], np.float32))
    return out


@pytest.mark.parametrize("name", ["percolation32", "blobs40", "blobs13", "whole_and_empty"])
def test_level_batched_labels_stats_pairs(cuda, name):
    from light_unet import lesion
    p, thr = _level_inputs()[name]
    K = len(thr)
    rng = np.random.default_rng(7)
    target = (_blobs(p.shape, 11, nblob=4) >= 0.35).astype(np.float32)
    if name == "percolation32":
        target = (rng.random(p.shape) < 0.2).astype(np.float32)
    pd = torch.from_numpy(p).to(cuda)
    tc = lesion.label(target, 0.5)
    assert tc.num > 0
    level, _, _ = lesion.level_map(pd, thr)
    comps, tables = lesion.label_levels(level, K, prob=pd, target=tc)
    assert len(comps) == len(tables) == K
    nums = []
    for k in range(K):
        one = lesion.label(p, float(thr[k]), prob=p)
        ref, nref = L.get_connected_components(p >= thr[k])
        lab = comps[k].numpy()
        assert comps[k].num == one.num == nref
        assert np.array_equal(lab, one.numpy())
        assert np.array_equal(lab, ref)
        assert comps[k].stats.shape == one.stats.shape and np.array_equal(comps[k].stats, one.stats)
        assert np.array_equal(tables[k], lesion._intersections(one, tc))
        nums.append(one.num)
    if name == "whole_and_empty":
        assert nums[0] == 1 and (comps[0].numpy() == 1).all() and nums[-1] == 0
    # a second run is bitwise the same, and so is a run in two groups of levels
    comps2, tables2 = lesion.label_levels(level, K, prob=pd, target=tc)
    h = K // 2
    ca, ta = lesion.label_levels(level, h, k0=0, prob=pd, target=tc)
    cb, tb = lesion.label_levels(level, K - h, k0=h, prob=pd, target=tc)
    for k, (c, t) in enumerate(zip(ca + cb, ta + tb)):
        for other, table in ((comps2[k], tables2[k]), (c, t)):
            assert torch.equal(other.labels, comps[k].labels)
            assert np.array_equal(other.stats, comps[k].stats)
            assert np.array_equal(table, tables[k])


# ---------------------------------------------------------------- sweep_metrics on the golden
@pytest.fixture(scope="module")
def val(golden):
    z = golden("validate.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    n = len(meta["shapes"])
    return {"meta": meta,
            "prob": [z[f"case{i}/prob"] for i in range(n)],
            "label": [z[f"case{i}/label"].astype(np.float32) for i in range(n)],
            "mask": [z[f"case{i}/mask"].astype(np.float32) for i in range(n)],
            "spacing": [tuple(s) for s in meta["spacings"]],
            "thr": list(meta["thresholds"])}


def _same(got, ref):
    assert set(got) == set(ref)
    for k, v in ref.items():
        assert got[k] == v, (k, got[k], v)


@pytest.fixture(scope="module")
def swept(cuda, val):
    """One sweep of the golden cases, shared by the tests below (plain and masked)."""
    from light_unet import lesion
    plain = lesion.sweep_metrics(val["prob"], val["label"], val["thr"], spacing=val["spacing"])
    masked = lesion.sweep_metrics(val["prob"], val["label"], val["thr"], spacing=val["spacing"],
                                  body_masks=val["mask"])
    return plain, masked


def test_sweep_equals_reference_dicts(val, swept):
    for got, name in zip(swept, ("metrics_plain", "metrics_masked")):
        assert len(got) == 7
        for g, r in zip(got, val["meta"][name]):
            _same(g, r)


def test_sweep_equals_per_threshold_path(cuda, val, swept):
    from light_unet import lesion
    masked = [p * m for p, m in zip(val["prob"], val["mask"])]
    for k, t in enumerate(val["thr"]):
        _same(swept[0][k], lesion.calculate_metrics(val["prob"], val["label"], threshold=t,
                                                    spacing=val["spacing"]))
        _same(swept[1][k], lesion.calculate_metrics(masked, val["label"], threshold=t,
                                                    spacing=val["spacing"]))


def test_sweep_order_duplicates_and_device_inputs(cuda, val, swept):
    from light_unet import lesion
    order = [0.5, 0.1, 0.7, 0.5, 0.3]
    preds = [torch.from_numpy(p).to(cuda) for p in val["prob"]]       # device tensors
    labels = [torch.from_numpy(l).to(cuda) for l in val["label"]]
    got = lesion.sweep_metrics(preds, labels, order, spacing=val["spacing"])
    assert len(got) == len(order)
    for g, t in zip(got, order):
        _same(g, swept[0][val["thr"].index(t)])
    assert got[0] is not got[3]


def test_sweep_call_count_does_not_depend_on_k(cuda, val, monkeypatch):
    from light_unet import _native, lesion
    calls = []
    real = _native.call

    def counting(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(_native, "call", counting)
    counts = {}
    for K in (2, 7):
        calls.clear()
        lesion.sweep_metrics(val["prob"], val["label"], val["thr"][:K], spacing=val["spacing"])
        counts[K] = list(calls)
    assert len(counts[2]) == len(counts[7]) > 0
    assert sorted(counts[2]) == sorted(counts[7])
    assert counts[7].count("l3u_thr_levels") == len(val["prob"])
    assert counts[7].count("l3u_ccl_label_lv") == len(val["prob"])
    # with a target cache the second sweep labels no target
    cache = {}
    calls.clear()
    first = lesion.sweep_metrics(val["prob"], val["label"], val["thr"], spacing=val["spacing"],
                                 target_cache=cache)
    assert calls.count("l3u_ccl_label_b") == len(val["prob"]) == len(cache)
    calls.clear()
    second = lesion.sweep_metrics(val["prob"], val["label"], val["thr"], spacing=val["spacing"],
                                  target_cache=cache)
    assert not [c for c in calls if c.startswith("l3u_ccl_label") and c != "l3u_ccl_label_lv"]
    for a, b in zip(first, second):
        _same(a, b)


def test_sweep_float64_and_batched_cases(cuda, val):
    from light_unet import lesion
    thr = val["thr"]
    # float64 maps compare in float64: values between float32(t) and t classify as numpy does
    p64 = [p.astype(np.float64) for p in val["prob"][:3]]
    for p in p64:
        f = p.reshape(-1)
        f[5], f[6] = 0.3, float(np.float32(0.3))       # float32(0.3) > 0.3
        f[7], f[8] = 0.1, float(np.float32(0.1))
    m64 = [m.astype(np.float64) for m in val["mask"][:3]]
    for preds, masks in ((p64, None), (val["prob"][:3], m64), (p64, val["mask"][:3])):
        got = lesion.sweep_metrics(preds, val["label"][:3], thr, spacing=val["spacing"][:3],
                                   body_masks=masks)
        prod = preds if masks is None else [p * m for p, m in zip(preds, masks)]
        assert prod[0].dtype == np.float64
        for g, t in zip(got, thr):
            _same(g, lesion.calculate_metrics(prod, val["label"][:3], threshold=t,
                                              spacing=val["spacing"][:3]))
    # a [2, D, H, W] case is labelled as one 4-dimensional array by the reference: the loop
    rng = np.random.default_rng(0)
    pb = [np.stack([_blobs((12, 10, 9), s), _blobs((12, 10, 9), s + 1)]) for s in (20, 30)]
    tb = [(rng.random((2, 12, 10, 9)) < 0.15).astype(np.float32) for _ in pb]
    got = lesion.sweep_metrics(pb, tb, thr[:3])
    for g, t in zip(got, thr[:3]):
        _same(g, lesion.calculate_metrics(pb, tb, threshold=t))
    # more than 32 distinct thresholds: the loop as well
    many = [0.02 * i for i in range(1, 35)]
    got = lesion.sweep_metrics(val["prob"][:1], val["label"][:1], many)
    for i in (0, 16, 33):
        _same(got[i], lesion.calculate_metrics(val["prob"][:1], val["label"][:1], threshold=many[i]))


def test_sweep_in_level_groups(cuda, val, swept, monkeypatch):
    from light_unet import _native, lesion
    calls = []
    real = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    got = lesion.sweep_metrics(val["prob"], val["label"], val["thr"], spacing=val["spacing"],
                               body_masks=val["mask"], max_workspace_bytes=1)
    # one level at a time: K labellings per case
    assert calls.count("l3u_ccl_label_lv") == 7 * len(val["prob"])
    for g, r in zip(got, swept[1]):
        _same(g, r)
    n = val["prob"][-1].size
    three = 3 * (n * 8 + (_native.query("l3u_ccl_nchunks", n) + 1) * 4)
    got = lesion.sweep_metrics(val["prob"][-1:], val["label"][-1:], val["thr"],
                               spacing=val["spacing"][-1:], max_workspace_bytes=three)
    ref = lesion.sweep_metrics(val["prob"][-1:], val["label"][-1:], val["thr"],
                               spacing=val["spacing"][-1:])
    for g, r in zip(got, ref):
        _same(g, r)
