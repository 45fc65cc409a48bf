"""The lesion uptake report on the device (light_unet/quantify.py, csrc/quantify.hip) against the
stored numpy / scipy results (tests/golden/quantify.npz, tests/golden/make_quantify_goldens.py)."""
import numpy as np
import pytest
import torch

import quantify_fixture as fx

pytestmark = pytest.mark.gpu


def _inputs(e, cuda, held={}):
    """The entry's uptake and mask on the device, uploaded once per volume."""
    for key, make in ((("u", e["uptake"]), lambda: fx.uptake(e)),
                      (("m", e["mask"]), lambda: fx.mask(e).astype(np.float32))):
        if key not in held:
            held[key] = torch.from_numpy(np.ascontiguousarray(make())).to(cuda)
    return held[("u", e["uptake"])], held[("m", e["mask"])]


def _call(e, cuda, **kw):
    from light_unet import quantify
    up, mask = _inputs(e, cuda)
    return quantify.lesion_uptake(up, mask, spacing=e["spacing"], min_size=e["min_size"],
                                  peak_ml=e["peak_ml"], **kw)


def test_every_golden_entry(cuda):
    entries = fx.entries()
    assert len(entries) >= 60
    for e in entries:
        fx.check_report(_call(e, cuda), e)


def test_peak_map_equals_the_golden_at_every_labelled_voxel(cuda):
    from light_unet import lesion, quantify
    z, _ = fx.load()
    stored = [e for e in fx.entries() if "peak" in e]
    assert sorted(tuple(e["spacing"]) for e in stored) == sorted(
        [(4.0, 4.0, 4.0), (3.27, 2.0364, 2.0364), (2.0, 2.0, 2.0)])
    for e in stored:
        shape = tuple(e["shape"])
        up, mask = _inputs(e, cuda)
        comp = lesion.label(mask, 0.5, e["min_size"])
        offs, reach = quantify.sphere_offsets(e["spacing"], e["peak_ml"])
        got = quantify._peak_map(up, comp.labels, offs, reach, shape).cpu().numpy()
        on = comp.numpy() > 0
        assert np.array_equal(on, fx.mask(e))
        ref = z[e["peak"]]
        differ = int((got[on].view(np.uint64) != ref.view(np.uint64)).sum())
        assert differ == 0, (e["name"], differ)


def test_candidate_mask_equals_the_golden_corner_mask(cuda):
    from light_unet import lesion, quantify
    from light_unet import preprocess as pp
    seen = set()
    for e in fx.entries():
        if e["corner"] in seen:
            continue
        seen.add(e["corner"])
        shape = tuple(e["shape"])
        _, mask = _inputs(e, cuda)
        comp = lesion.label(mask, 0.5, e["min_size"])
        bits, pre, n = quantify._corner_bits(pp.pack(comp.labels), shape)
        ref = fx.bits(e["corner"], shape)
        got = pp.unpack(bits, shape, torch.bool).cpu().numpy()
        assert np.array_equal(got, ref), e["corner"]
        assert n == int(ref.sum())
        if n:   # the coordinate list: every corner voxel once, in ascending flat index
            cand = quantify._candidates(bits, pre, n, shape).cpu().numpy()
            want = np.argwhere(ref)
            assert np.array_equal(cand[:, :3], want), e["corner"]
            assert np.array_equal(cand[:, 3], np.flatnonzero(ref.ravel())), e["corner"]
    assert len(seen) >= 12


def _entry(name):
    return next(e for e in fx.entries() if e["name"] == name)


def test_input_kinds_give_the_same_dict(cuda):
    from light_unet import lesion, quantify
    e = _entry("g_12x20x70__blobs_12x20x70__s1__m0")
    up, mask = fx.uptake(e), fx.mask(e)
    kw = dict(spacing=e["spacing"], peak_ml=e["peak_ml"])
    base = quantify.lesion_uptake(up, mask.astype(np.float32), **kw)
    fx.check_report(base, e)
    up_d = torch.from_numpy(up).to(cuda)
    assert quantify.lesion_uptake(up_d, torch.from_numpy(mask).to(cuda), **kw) == base
    assert quantify.lesion_uptake(up.astype(np.float64), mask.astype(np.uint8), **kw) == base
    # a probability map against its threshold, and a labelling that is on the device already
    prob = np.where(mask, np.float32(0.75), np.float32(0.25))
    assert quantify.lesion_uptake(up, prob, threshold=0.6, **kw) == base
    assert quantify.lesion_uptake(up, prob, threshold=0.2, **kw)["n_lesions"] == 1
    comp = lesion.label(torch.from_numpy(prob).to(cuda), 0.6)
    assert quantify.lesion_uptake(up_d, comp, **kw) == base
    assert quantify.lesion_uptake(up, comp, threshold=0.99, min_size=10 ** 6, **kw) == base


def test_two_calls_give_the_same_bits(cuda):
    e = _entry("g_24x40x40__blobs_24x40x40__s2__m0")
    a, b = _call(e, cuda), _call(e, cuda)
    assert a == b
    for ra, rb in zip(a["lesions"], b["lesions"]):
        for k in ("suv_mean", "suv_peak", "tlg"):
            assert np.float64(ra[k]).view(np.uint64) == np.float64(rb[k]).view(np.uint64)
    assert np.float64(a["dmax_mm"]).view(np.uint64) == np.float64(b["dmax_mm"]).view(np.uint64)


def test_peak_and_dmax_can_be_left_out(cuda):
    e = _entry("g_12x20x70__blobs_12x20x70__s0__m0")
    full = _call(e, cuda)
    up, mask = _inputs(e, cuda)
    from light_unet import quantify
    kw = dict(spacing=e["spacing"], min_size=e["min_size"])
    no_peak = quantify.lesion_uptake(up, mask, peak_ml=None, **kw)
    no_dmax = quantify.lesion_uptake(up, mask, peak_ml=e["peak_ml"], dmax=False, **kw)
    neither = quantify.lesion_uptake(up, mask, peak_ml=None, dmax=False, **kw)
    peak_keys, dmax_keys = {"suv_peak", "suv_peak_voxel"}, {"dmax_mm", "dmax_voxels"}

    def without(d, case_keys, lesion_keys):
        out = {k: v for k, v in d.items() if k not in case_keys}
        out["lesions"] = [{k: v for k, v in r.items() if k not in lesion_keys} for r in d["lesions"]]
        return out
    assert no_peak == without(full, {"suv_peak"}, peak_keys)
    assert no_dmax == without(full, dmax_keys, set())
    assert neither == without(full, dmax_keys | {"suv_peak"}, peak_keys)
    assert "dmax_centroid_mm" in neither and len(full["lesions"]) >= 3


def test_more_than_one_slab_and_tile_per_lesion(cuda, monkeypatch):
    """The slab size only changes how a lesion's voxels are grouped: with slabs of one plane the
    exact keys do not move and the sums stay within the summation bound."""
    from light_unet import quantify
    e = _entry("g_24x40x40__blobs_24x40x40__s1__m0")
    monkeypatch.setattr(quantify, "SLAB_VOXELS", 1)
    fx.check_report(_call(e, cuda), e)
    e = _entry("q_24x40x40__blobs_24x40x40__s2__m0")
    fx.check_report(_call(e, cuda), e)


def test_farthest_pair_over_many_tiles(cuda):
    """More candidates than one workgroup's group of j-tiles (8 tiles of 256): 2300 random voxels
    of a long volume, against numpy, so that a second j-group and a partial last tile are walked."""
    from light_unet import quantify
    rng = np.random.default_rng(5)
    shape = (7, 11, 3200)
    flat = np.sort(rng.choice(shape[0] * shape[1] * shape[2], 2300, replace=False))
    zyx = np.stack(np.unravel_index(flat, shape), axis=1)
    cand = torch.from_numpy(np.concatenate([zyx, flat[:, None]], axis=1).astype(np.int32)).to(cuda)
    for spacing in ((4.0, 4.0, 4.0), (3.27, 2.0364, 2.0364)):
        d2, i, j = quantify._farthest(cand, len(flat), spacing).cpu().tolist()
        d = (zyx[:, None, :] - zyx[None, :, :]).astype(np.float64) * np.asarray(spacing)
        d = d * d
        d = (d[..., 0] + d[..., 1]) + d[..., 2]
        d[np.tril_indices(len(flat))] = -1.0
        k = int(np.argmax(d))
        assert d2 == d.flat[k] and (int(i), int(j)) == (flat[k // len(flat)], flat[k % len(flat)])


def test_infer_volume_reports_the_uptake(cuda):
    """On tests/test_sliding_mask_gpu.py's volume, the smallest the infer_volume tests use."""
    from light_unet import inference, lesion, quantify
    from test_sliding_mask_gpu import PATCH, SHAPE, _model, _volume
    model, img = _model(cuda), _volume(SHAPE, 5)
    rng = np.random.default_rng(11)
    suv = (rng.gamma(2.0, 1.0, SHAPE) + 6.0 * img).astype(np.float32)
    spacing = (4.0, 4.0, 4.0)
    cfg = {"data": {"patch_size": list(PATCH), "bbox_expansion_voxels": 2,
                    "volume_threshold": {"inference_cc": 0.5}, "body_mask": {}},
           "validation": {"default_threshold": 0.5}}
    cache = {}
    plain = inference.infer_volume(img, model, cfg, spacing=spacing, forward_cache=cache)
    assert isinstance(plain, tuple) and len(plain) == 2
    thr = float(np.quantile(plain[0], 0.9))
    plain_map, plain_boxes = inference.infer_volume(img, model, cfg, spacing=spacing, threshold=thr,
                                                    forward_cache=cache)
    assert len(plain_boxes) > 0
    got = inference.infer_volume(img, model, cfg, spacing=spacing, threshold=thr, forward_cache=cache,
                                 uptake=torch.from_numpy(suv).to(cuda))
    assert len(got) == 3
    assert np.array_equal(got[0].view(np.uint32), plain_map.view(np.uint32)) and got[1] == plain_boxes
    report = got[2]
    want = quantify.lesion_uptake(suv, plain_map, spacing=spacing, threshold=thr,
                                  min_size=lesion.min_voxels_for(0.5, spacing))
    assert report == want
    assert [r["label"] for r in report["lesions"]] == [b["mask_id"] for b in plain_boxes]
    for r, b in zip(report["lesions"], plain_boxes):
        assert r["volume_ml"] == b["volume_cc"]
    # the options pass through
    got = inference.infer_volume(img, model, cfg, spacing=spacing, threshold=thr, forward_cache=cache,
                                 uptake=suv, quantify={"peak_ml": None, "dmax": False})
    assert got[1] == plain_boxes and "dmax_mm" not in got[2] and "suv_peak" not in got[2]
    assert got[2]["tmtv_ml"] == report["tmtv_ml"] and got[2]["tlg_total"] == report["tlg_total"]
