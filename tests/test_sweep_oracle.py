"""The level / histogram definition of the threshold sweep, checked in numpy against the reference
results stored in tests/golden/validate.npz (made by tests/golden/make_validate_goldens.py), and
the host parts of the sweep that need no GPU."""
import json

import numpy as np

from oracle import lesion_oracle as L


def _load(golden):
    z = golden("validate.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    cases = [(z[f"case{i}/prob"], z[f"case{i}/label"], z[f"case{i}/mask"])
             for i in range(len(meta["shapes"]))]
    return meta, cases


def levels_and_hist(prob, thr32, mask=None, target=None):
    """The definition l3u_thr_levels implements: level = #{k: p >= thr[k]} with p = prob * mask in
    float32, hist[level, target >= 0.5] = voxel count."""
    p = prob.astype(np.float32)
    if mask is not None:
        p = p * mask.astype(np.float32)
    assert p.dtype == np.float32
    level = np.zeros(p.shape, np.uint8)
    for t in thr32:
        level += (p >= t)
    tb = (target >= 0.5).astype(np.int64) if target is not None else np.zeros(p.shape, np.int64)
    hist = np.zeros((len(thr32) + 1, 2), np.int64)
    np.add.at(hist, (level.reshape(-1).astype(np.int64), tb.reshape(-1)), 1)
    return level, hist


def test_fixture_has_the_cases_the_sweep_must_survive(golden):
    meta, cases = _load(golden)
    thr = np.asarray(meta["thresholds"], np.float32)
    assert len(thr) == 7 and len(cases) == 6
    assert cases[meta["empty_target"]][1].sum() == 0
    assert not (cases[meta["below_top"]][0] >= thr[-1]).any()
    assert (cases[meta["whole_volume"]][0] >= thr[0]).all()
    assert len({c[0].shape for c in cases}) == len(cases)
    for p, _, _ in cases:
        assert p.dtype == np.float32
        hits = sum(int((p == t).any()) + int((p == np.nextafter(t, np.float32(0))).any()) for t in thr)
        assert hits >= 4     # voxels exactly at a threshold and one float32 below
    chosen = [r["result"]["best_threshold"] for r in meta["validate_masked"]]
    assert chosen[0] != chosen[1]     # the second tie_threshold changes the selection


def test_histogram_suffix_sums_give_the_stored_dsc(golden):
    """ps / ts / overlap at threshold k are suffix sums of the (level, target) histogram; with
    them calculate_metrics' own DSC expressions give the stored values exactly."""
    meta, cases = _load(golden)
    thr = np.asarray(meta["thresholds"], np.float32)
    smooth = 1e-6
    for masked, name in ((False, "metrics_plain"), (True, "metrics_masked")):
        hists = []
        for p, l, m in cases:
            level, h = levels_and_hist(p, thr, m if masked else None, l)
            pm = p * m.astype(np.float32) if masked else p
            for k, t in enumerate(thr):       # the level encodes every binarisation
                assert np.array_equal(level >= k + 1, pm >= t)
            hists.append(h)
        for k in range(len(thr)):
            inter_sum = union_sum = 0.0
            per_case = []
            for h in hists:
                ge = np.cumsum(h[::-1], axis=0)[::-1]
                ps, inter, ts = int(ge[k + 1].sum()), int(ge[k + 1, 1]), int(h[:, 1].sum())
                inter_sum += inter
                union_sum += ps + ts
                per_case.append((2.0 * inter + smooth) / ((ps + ts) + smooth))
            ref = meta[name][k]
            assert (2.0 * inter_sum + smooth) / (union_sum + smooth) == ref["voxel_wise_dsc_micro"]
            assert float(np.mean(per_case)) == ref["voxel_wise_dsc_macro"]


def test_aggregate_of_host_rows_equals_the_stored_dicts(golden):
    """lesion._aggregate (the host end of sweep_metrics) on rows built in numpy (histogram sums +
    the CPU labelling's lesion counts) gives the reference's dict, every key."""
    from light_unet import lesion
    meta, cases = _load(golden)
    thr = np.asarray(meta["thresholds"], np.float32)
    for k in (0, 3, 6):
        rows = []
        for (p, l, m), sp in zip(cases, meta["spacings"]):
            pm = p * m.astype(np.float32)
            _, h = levels_and_hist(p, thr, m, l)
            ge = np.cumsum(h[::-1], axis=0)[::-1]
            lm = L.lesion_metrics(pm, l.astype(np.float32), float(thr[k]), spacing=tuple(sp))
            rows.append((int(ge[k + 1].sum()), int(h[:, 1].sum()), int(ge[k + 1, 1]),
                         lm["tp"], lm["fp"], lm["fn"]))
        got = lesion._aggregate(rows, len(rows))
        ref = meta["metrics_masked"][k]
        assert set(got) == set(ref)
        for key, v in ref.items():
            assert got[key] == v, (k, key)


def test_level_workspace_query_without_gpu():
    from light_unet import _native
    n = 40 * 36 * 44
    per = n * 8 + (_native.query("l3u_ccl_nchunks", n) + 1) * 4
    assert _native.query("l3u_ccl_lv_max_levels", n, 7 * per) == 7
    assert _native.query("l3u_ccl_lv_max_levels", n, 7 * per - 1) == 6
    assert _native.query("l3u_ccl_lv_max_levels", n, 1) == 1           # never below one level
    assert _native.query("l3u_ccl_lv_max_levels", n, 1 << 40) == 32    # never above the level limit
    for name in ("l3u_thr_levels", "l3u_ccl_label_lv", "l3u_ccl_stats_lv", "l3u_ccl_pairs_lv"):
        assert name in _native.exported_symbols()
