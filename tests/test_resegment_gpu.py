"""Resegmentation by an uptake threshold on the device (light_unet/resegment.py,
csrc/resegment.hip) against the stored numpy / scipy results (tests/golden/resegment.npz,
tests/golden/make_resegment_goldens.py).  Every comparison is exact."""
import math

import numpy as np
import pytest
import torch

import resegment_fixture as fx

pytestmark = pytest.mark.gpu

TILED = 16   # max_lds_bytes at which no box fits the LDS: every seed goes the tiled way


def _inputs(c, cuda, held={}):
    """The case's uptake and seed mask on the device, uploaded once per volume."""
    if c["uptake"] not in held:
        held[c["uptake"]] = (torch.from_numpy(np.ascontiguousarray(fx.uptake(c))).to(cuda),
                             torch.from_numpy((fx.seeds(c) > 0).astype(np.float32)).to(cuda))
    return held[c["uptake"]]


def _run(c, cuda, **kw):
    from light_unet import resegment
    up, mask = _inputs(c, cuda)
    kw.setdefault("body_mask", fx.body(c))
    return resegment.resegment_lesions(up, mask, spacing=c["spacing"], method=c["method"],
                                       value=c["value"], grow_mm=c["grow_mm"], **kw)


def _check(c, cuda, **kw):
    rs = _run(c, cuda, **kw)
    fx.check_result(rs, fx.expected(c), (c["name"], kw))
    assert np.array_equal(rs.seed_voxels, np.bincount(fx.seeds(c).ravel())[1:])
    return rs


def test_word_seam_and_padding_bits(cuda):
    c = fx.case("seam")
    assert c["shape"] == [12, 12, 70]
    rs = _check(c, cuda)
    assert rs.path.tolist() == [0] and rs.reached.tolist() == [12 * 12 * 65]
    lab = rs.components.numpy()
    assert lab[:, :, :5].max() == 0 and lab[:, :, 5:].min() == 1
    assert _check(c, cuda, max_lds_bytes=TILED).path.tolist() == [1]


def test_serpentine_path_is_followed_to_its_end(cuda):
    c = fx.case("serpentine")
    exp = fx.expected(c)
    assert c["shape"] == [10, 12, 20] and exp["reached"][0] >= 300 and int((fx.seeds(c) > 0).sum()) == 1
    lds = _check(c, cuda)
    assert lds.path.tolist() == [0] and lds.sweeps[0] >= 1
    tiled = _check(c, cuda, max_lds_bytes=TILED)
    # the seed's tile and the tile of the path's end differ, and a launch carries a bit one tile far
    assert tiled.path.tolist() == [1] and tiled.sweeps[0] >= 2
    print("serpentine: sweeps", int(lds.sweeps[0]), "tiled launches", int(tiled.sweeps[0]))
    mixed = _check(c, cuda, max_lds_bytes=16 + 16 * 64)       # 64 words: the 120 of this box do not fit
    assert mixed.path.tolist() == [1]


def test_connectivity_through_voxels_outside_the_box_does_not_count(cuda):
    c = fx.case("boxcut")
    for lds in (0, TILED):
        lab = _check(c, cuda, max_lds_bytes=lds).components.numpy()
        assert fx.uptake(c)[2, 2, 8] >= 4.0 and lab[2, 2, 8] == 0 and lab[4, 4, 14] == 1


def test_overlapping_boxes_the_smaller_label_owns(cuda):
    for lds in (0, TILED):
        keep = _check(fx.case("overlap_keep"), cuda, max_lds_bytes=lds)
        assert keep.status.tolist() == [0, 0] and keep.seed_label.tolist() == [1, 2]
        lab = keep.components.numpy()
        assert lab[3, 3, 16] == 1 and lab[3, 3, 17] == 2
        gone = _check(fx.case("overlap_absorb"), cuda, max_lds_bytes=lds)
        assert gone.status.tolist() == [0, 2, 0] and gone.seed_label.tolist() == [1, 3]
        assert gone.components.num == 2 and gone.components.numpy()[3, 4, 40] == 2


def test_seed_below_the_fixed_threshold(cuda):
    for lds in (0, TILED):
        rs = _check(fx.case("below"), cuda, max_lds_bytes=lds)
        assert rs.status.tolist() == [1, 0] and rs.reached[0] == 0 and rs.seed_label.tolist() == [2]


def test_body_mask_cuts_a_region_whatever_its_dtype(cuda):
    c = fx.case("body")
    bm = fx.body(c)
    assert _check(fx.case("body_off"), cuda).reached[0] == 2 * _check(c, cuda).reached[0]
    for mask in (bm.astype(np.float32), bm, bm.astype(bool), bm.astype(np.int8),
                 torch.from_numpy(bm.astype(bool)).to(cuda), torch.from_numpy(bm).to(cuda)):
        for lds in (0, TILED):
            _check(c, cuda, body_mask=mask, max_lds_bytes=lds)


def test_boxes_clipped_at_every_face(cuda):
    grows = []
    for c in fx.cases("faces"):
        grows.append(c["grow_mm"])
        for lds in (0, TILED):
            _check(c, cuda, max_lds_bytes=lds)
    assert grows == [None, 0.0, 1000.0]
    assert max(c["shape"]) * 4.0 < 1000.0


def test_relative_threshold_is_compared_in_float64(cuda):
    c = fx.case("witness")
    up = fx.uptake(c)
    thr = np.float64(0.41) * np.float64(up[1, 1, 2])
    assert not (np.float64(up[1, 1, 1]) >= thr) and up[1, 1, 1] >= np.float32(thr)
    for lds in (0, TILED):
        rs = _check(c, cuda, max_lds_bytes=lds)
        assert rs.components.numpy()[1, 1].tolist() == [0, 0, 1, 1, 0]
        assert rs.thresholds.view(np.uint64).tolist() == [thr.view(np.uint64)]


def test_relative_at_one_and_exactly_at_the_threshold(cuda):
    for lds in (0, TILED):
        one = _check(fx.case("rel_one"), cuda, max_lds_bytes=lds)
        lab = one.components.numpy()
        assert one.reached.tolist() == [3] and lab[1, 2, 3] == 1 and lab[2, 2, 5] == 0 and lab[1, 1, 8] == 0
        half = _check(fx.case("rel_half"), cuda, max_lds_bytes=lds)
        assert half.thresholds.tolist() == [4.0] and half.components.numpy()[1, 1, 2:5].tolist() == [1, 1, 0]


@pytest.mark.parametrize("spacing", ["a", "i"])
def test_random_case_equals_the_goldens(cuda, spacing):
    cases = [c for c in fx.cases("random") if c["name"].startswith(f"random_{spacing}_")]
    assert len(cases) == 8 and {c["grow_mm"] for c in cases} == {None, 8.0, 16.0, 1000.0}
    assert {c["method"] for c in cases} == {"fixed", "relative"}
    assert cases[0]["spacing"] == ([3.0, 2.04, 2.04] if spacing == "a" else [4.0, 4.0, 4.0])
    for c in cases:
        a = _check(c, cuda)
        b = _run(c, cuda)
        assert torch.equal(a.components.labels, b.components.labels), c["name"]
        for k in ("status", "reached", "seed_label", "thresholds", "seed_voxels"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), (c["name"], k)
        assert np.array_equal(a.components.stats, b.components.stats)
        t = _check(c, cuda, max_lds_bytes=TILED)
        assert torch.equal(a.components.labels, t.components.labels), c["name"]
        assert set(t.path.tolist()) == {1}
    # the whole volume as one box, 40 x 44 x 2 words, fits 64 KiB of LDS and not 32 KiB
    whole = next(c for c in cases if c["grow_mm"] == 1000.0)
    assert set(_run(whole, cuda).path.tolist()) == {0}
    assert set(_run(whole, cuda, max_lds_bytes=32 * 1024).path.tolist()) == {1}


def test_no_seeds_and_components_in_place_of_a_mask(cuda):
    from light_unet import lesion, resegment
    c = fx.case("random_i_fixed_16")
    up, mask = _inputs(c, cuda)
    none = resegment.resegment_lesions(up, torch.zeros_like(mask))
    assert none.components.num == 0 and int(none.components.labels.abs().sum()) == 0
    assert none.components.labels.dtype == torch.int32 and none.components.stats.shape == (0, 12)
    for k, dt in (("seed_label", np.int32), ("status", np.int8), ("thresholds", np.float64),
                  ("seed_voxels", np.int64), ("reached", np.int64)):
        assert getattr(none, k).shape == (0,) and getattr(none, k).dtype == dt, k
    gone = resegment.resegment_lesions(up, mask, min_size=10 ** 6)
    assert gone.components.num == 0 and gone.status.shape == (0,)
    comp = lesion.label(mask, 0.5)
    seeds_before = comp.labels.clone()
    rs = resegment.resegment_lesions(up, comp, spacing=c["spacing"], method=c["method"],
                                     value=c["value"], grow_mm=c["grow_mm"], threshold=0.99,
                                     min_size=10 ** 6)
    fx.check_result(rs, fx.expected(c), "components")
    assert torch.equal(comp.labels, seeds_before)   # the seeds are read, not written
    # a probability map against its threshold, and numpy inputs
    prob = np.where(fx.seeds(c) > 0, np.float32(0.75), np.float32(0.25))
    rs = resegment.resegment_lesions(fx.uptake(c).astype(np.float64), prob, spacing=c["spacing"],
                                     method=c["method"], value=c["value"], grow_mm=c["grow_mm"],
                                     threshold=0.6)
    fx.check_result(rs, fx.expected(c), "numpy")
    # every seed below the threshold: an empty map
    rs = resegment.resegment_lesions(up, mask, value=1000.0, grow_mm=8.0)
    assert rs.components.num == 0 and set(rs.status.tolist()) == {1}
    assert int(rs.components.labels.abs().sum()) == 0 and rs.seed_label.shape == (0,)


def test_lesion_uptake_reports_the_resegmented_lesions(cuda):
    from light_unet import quantify
    for c in (c for c in fx.cases() if "report" in c):
        up, mask = _inputs(c, cuda)
        cfg = {"method": c["method"], "value": c["value"], "grow_mm": c["grow_mm"]}
        plain = quantify.lesion_uptake(up, mask, spacing=c["spacing"])
        got = quantify.lesion_uptake(up, mask, spacing=c["spacing"], resegment=cfg)
        assert quantify.lesion_uptake(up, mask, spacing=c["spacing"], resegment=None) == plain
        want = c["report"]
        assert set(got) == set(plain) | {"resegment"}
        assert got["resegment"] == {"method": c["method"], "value": c["value"], "grow_mm": c["grow_mm"],
                                    "below_threshold": want["below_threshold"],
                                    "absorbed": want["absorbed"]}
        assert got["tmtv_ml"] == want["tmtv_ml"] and got["n_lesions"] == len(want["lesions"])
        labels, host = fx.expected(c)["labels"], fx.uptake(c).astype(np.float64)
        for g, w in zip(got["lesions"], want["lesions"]):
            assert set(g) == set(plain["lesions"][0]) | {"seed_label", "seed_voxels", "threshold"}
            for k in ("label", "voxels", "suv_max", "seed_label", "seed_voxels", "threshold"):
                assert g[k] == w[k], (c["name"], w["label"], k, g[k], w[k])
            # tests/test_quantify_gpu.py's summation bound, against the exact sum
            v = host[labels == w["label"]]
            err = abs(g["suv_mean"] * w["voxels"] - math.fsum(v))
            bound = w["voxels"] * 2.0 ** -53 * math.fsum(np.abs(v))
            print(c["name"], w["label"], "suv_mean", g["suv_mean"], err, bound)
            assert err <= bound, (c["name"], w["label"], err, bound)
            assert g["tlg"] == g["suv_mean"] * g["volume_ml"]


def test_infer_volume_reports_the_seed_of_every_lesion(cuda):
    """On tests/test_sliding_mask_gpu.py's volume and graph-captured model, the smallest the
    infer_volume tests use."""
    from light_unet import inference
    from test_sliding_mask_gpu import PATCH, SHAPE, _model, _volume
    model, img = _model(cuda), _volume(SHAPE, 5)
    rng = np.random.default_rng(11)
    suv = (rng.gamma(2.0, 1.0, SHAPE) + 6.0 * img).astype(np.float32)
    spacing = (4.0, 4.0, 4.0)
    cfg = {"data": {"patch_size": list(PATCH), "bbox_expansion_voxels": 2,
                    "volume_threshold": {"inference_cc": 0.5}, "body_mask": {}},
           "validation": {"default_threshold": 0.5}}
    cache = {}
    first = inference.infer_volume(img, model, cfg, spacing=spacing, forward_cache=cache)
    thr = float(np.quantile(first[0], 0.9))
    kw = dict(spacing=spacing, threshold=thr, forward_cache=cache, uptake=suv)
    plain = inference.infer_volume(img, model, cfg, **kw)
    rcfg = {"method": "relative", "value": 0.41, "grow_mm": 8.0}
    got = inference.infer_volume(img, model, cfg, resegment=rcfg, **kw)
    assert len(got) == 3 and len(plain[1]) > 0
    assert np.array_equal(got[0].view(np.uint32), plain[0].view(np.uint32)) and got[1] == plain[1]
    ids = [b["mask_id"] for b in plain[1]]
    report = got[2]
    assert report["resegment"]["method"] == "relative" and "resegment" not in plain[2]
    gone = report["resegment"]["below_threshold"] + report["resegment"]["absorbed"]
    assert report["resegment"]["below_threshold"] == []    # a seed's maximum is a candidate of its own
    assert [r["seed_label"] for r in report["lesions"]] == [i for i in ids if i not in gone]
    assert report["n_lesions"] >= 1
    seed_rows = {r["label"]: r for r in plain[2]["lesions"]}
    for r in report["lesions"]:
        s = seed_rows[r["seed_label"]]
        assert r["seed_voxels"] == s["voxels"]
        assert r["threshold"] == float(np.float64(0.41) * np.float64(np.float32(s["suv_max"])))
