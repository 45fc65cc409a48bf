"""Resegmentation by an uptake threshold, the parts that need no GPU: argument errors come before
any device access, the box padding and the threshold arithmetic are the contract's, the numpy
restatement of the contract equals the stored scipy results array by array, and the additions to
lesion_uptake, check_config and the C header leave what was there as it was."""
import inspect
import os
import re

import numpy as np
import pytest

import resegment_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def no_device(monkeypatch):
    """Any device access of the modules under test fails the test (also where a GPU is present)."""
    from light_unet import _native, lesion, quantify, resegment

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(quantify, "_device", boom)
    monkeypatch.setattr(lesion, "_device", boom)
    monkeypatch.setattr(_native, "call", boom)
    monkeypatch.setattr(_native, "query", boom)
    return resegment


def test_check_resegment(no_device):
    rs = no_device
    assert rs.check_resegment(None) is None
    assert rs.check_resegment({}) == ("fixed", 4.0, None)
    assert rs.check_resegment({"method": "relative", "value": 0.41, "grow_mm": 20}) == \
        ("relative", 0.41, 20.0)
    assert rs.check_resegment({"method": "relative", "value": 1.0, "grow_mm": 0}) == ("relative", 1.0, 0.0)
    assert rs.check_resegment({"value": 2.5, "grow_mm": None}) == ("fixed", 2.5, None)
    with pytest.raises(ValueError, match="unknown keys"):
        rs.check_resegment({"threshold": 4.0})
    with pytest.raises(ValueError, match="dict"):
        rs.check_resegment(["fixed", 4.0])
    with pytest.raises(ValueError, match="method"):
        rs.check_resegment({"method": "percist"})
    for bad in (0.0, -1.0, float("nan"), float("inf"), "four", None):
        with pytest.raises(ValueError, match="value"):
            rs.check_resegment({"value": bad})
    with pytest.raises(ValueError, match="relative"):
        rs.check_resegment({"method": "relative", "value": 1.01})
    with pytest.raises(ValueError, match="relative"):
        rs.check_resegment({"method": "relative"})   # the default value, 4.0, is no fraction
    for bad in (-0.5, float("nan"), float("inf"), "far"):
        with pytest.raises(ValueError, match="grow_mm"):
            rs.check_resegment({"grow_mm": bad})


def test_argument_errors_come_before_the_device(no_device):
    rs = no_device
    u = np.zeros((4, 5, 6), np.float32)
    with pytest.raises(ValueError, match="differ in shape"):
        rs.resegment_lesions(u, np.zeros((4, 5, 7), np.float32))
    with pytest.raises(ValueError, match=r"\[D, H, W\]"):
        rs.resegment_lesions(np.zeros((5, 6), np.float32), np.zeros((5, 6), np.float32))
    with pytest.raises(ValueError, match=r"\[D, H, W\]"):
        rs.resegment_lesions(np.zeros((0, 5, 6), np.float32), np.zeros((0, 5, 6), np.float32))
    with pytest.raises(ValueError, match=r"\[D, H, W\]"):
        rs.resegment_lesions(u, np.zeros((1, 4, 5, 6), np.float32))
    for bad in ((4.0, 0.0, 4.0), (4.0, 4.0), (4.0, float("nan"), 4.0), 4.0):
        with pytest.raises(ValueError, match="spacing"):
            rs.resegment_lesions(u, u, spacing=bad)
    with pytest.raises(ValueError, match="method"):
        rs.resegment_lesions(u, u, method="absolute")
    for bad in (0.0, -4.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="value"):
            rs.resegment_lesions(u, u, value=bad)
    with pytest.raises(ValueError, match="relative"):
        rs.resegment_lesions(u, u, method="relative", value=4.0)
    with pytest.raises(ValueError, match="grow_mm"):
        rs.resegment_lesions(u, u, grow_mm=-1.0)
    with pytest.raises(ValueError, match="body_mask has shape"):
        rs.resegment_lesions(u, u, body_mask=np.ones((4, 5, 7), np.uint8))
    with pytest.raises(ValueError, match="body_mask dtype"):
        rs.resegment_lesions(u, u, body_mask=np.ones((4, 5, 6), np.float64))
    for bad in (8, -1, 64 * 1024 + 1):
        with pytest.raises(ValueError, match="max_lds_bytes"):
            rs.resegment_lesions(u, u, max_lds_bytes=bad)


def test_report_arguments_come_before_the_device(no_device):
    from light_unet import inference, quantify
    u = np.zeros((4, 5, 6), np.float32)
    with pytest.raises(ValueError, match="unknown keys"):
        quantify.lesion_uptake(u, u, resegment={"grow": 4.0})
    with pytest.raises(ValueError, match="relative"):
        quantify.lesion_uptake(u, u, resegment={"method": "relative", "value": 41.0})
    img = np.zeros((8, 8, 8), np.float32)
    with pytest.raises(ValueError, match="uptake"):
        inference.infer_volume(img, None, {}, resegment={"value": 4.0})
    with pytest.raises(ValueError, match="unknown keys"):
        inference.infer_volume(img, None, {}, uptake=img, resegment={"suv": 4.0})
    with pytest.raises(ValueError, match="grow_mm"):
        inference.infer_volume(img, None, {}, uptake=img, resegment={"grow_mm": -2})


def test_native_error_without_a_device(monkeypatch):
    import torch
    from light_unet import _native, resegment
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    u = np.zeros((4, 5, 6), np.float32)
    with pytest.raises(_native.NativeError, match="no GPU"):
        resegment.resegment_lesions(u, u)


def test_box_padding_and_boxes(no_device):
    rs = no_device
    assert rs.box_padding(20.0, (3.0, 2.04, 2.04)) == (7, 10, 10)
    assert rs.box_padding(20.0, (4.0, 4.0, 4.0)) == (5, 5, 5)
    assert rs.box_padding(0.0, (3.0, 2.04, 2.04)) == (0, 0, 0)
    assert rs.box_padding(8.0, (4.0, 4.0, 4.0)) == (2, 2, 2)
    assert rs.box_padding(20.0, (3.0, 2.04, 2.04)) == fx.padding(20.0, (3.0, 2.04, 2.04))
    stats = np.zeros((3, 12), dtype=np.uint64)
    stats[0, 4:7], stats[0, 7:10] = (0, 0, 0), (0, 0, 0)            # a voxel in the first corner
    stats[1, 4:7], stats[1, 7:10] = (10, 20, 30), (12, 25, 40)
    stats[2, 4:7], stats[2, 7:10] = (38, 40, 60), (39, 43, 69)      # touches the last corner
    boxes = rs.seed_boxes(stats, (7, 10, 10), (40, 44, 70))
    assert boxes.dtype == np.int32
    assert boxes.tolist() == [[0, 8, 0, 11, 0, 11], [3, 20, 10, 36, 20, 51], [31, 40, 30, 44, 50, 70]]
    assert rs.seed_boxes(stats, (0, 0, 0), (40, 44, 70)).tolist() == \
        [[0, 1, 0, 1, 0, 1], [10, 13, 20, 26, 30, 41], [38, 40, 40, 44, 60, 70]]
    assert rs.seed_boxes(stats, (491, 491, 491), (40, 44, 70)).tolist() == [[0, 40, 0, 44, 0, 70]] * 3


def test_threshold_arithmetic(no_device):
    rs = no_device
    m = np.asarray([7.3, 12.125, 2.0000002], dtype=np.float32)
    fixed = rs.thresholds_for("fixed", 4.0, m)
    assert fixed.dtype == np.float64 and fixed.tolist() == [4.0, 4.0, 4.0]
    rel = rs.thresholds_for("relative", 0.41, m)
    assert rel.dtype == np.float64
    for t, v in zip(rel, m):   # one float64 multiply of the float32 maximum
        assert t.view(np.uint64) == (np.float64(0.41) * np.float64(v)).view(np.uint64)
        assert t != np.float64(np.float32(0.41) * v)
    assert rs.thresholds_for("relative", 1.0, m).tolist() == m.astype(np.float64).tolist()
    # the stored witness: the float64 and the float32 comparison disagree on a voxel next to the seed
    c = fx.case("witness")
    up, exp = fx.uptake(c), fx.expected(c)
    m, u = up[1, 1, 2], up[1, 1, 1]
    thr = rs.thresholds_for("relative", c["value"], [m])
    assert thr.view(np.uint64).tolist() == exp["thresholds"].view(np.uint64).tolist()
    assert not (np.float64(u) >= thr[0]) and u >= np.float32(thr[0])
    assert exp["labels"][1, 1].tolist() == [0, 0, 1, 1, 0]


def test_fixture_equals_the_goldens_array_by_array():
    cases = fx.cases()
    assert len(cases) == 30
    assert {c["family"] for c in cases} == {"seam", "serpentine", "boxcut", "overlap", "below", "body",
                                            "faces", "witness", "relative", "random"}
    statuses = set()
    for c in cases:
        exp = fx.expected(c)
        got = fx.reference(fx.uptake(c), fx.seeds(c), c["spacing"], c["method"], c["value"],
                           c["grow_mm"], fx.body(c))
        assert set(got) == set(fx.ARRAYS)
        for k in fx.ARRAYS:
            assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (c["name"], k)
            assert np.array_equal(got[k].view(np.uint64) if k == "thresholds" else got[k],
                                  exp[k].view(np.uint64) if k == "thresholds" else exp[k]), (c["name"], k)
        statuses |= set(exp["status"].tolist())
        assert np.array_equal(np.bincount(exp["labels"].ravel(), minlength=len(exp["seed_label"]) + 1)[1:],
                              exp["owned"][exp["owned"] > 0]), c["name"]
        assert np.all(exp["owned"] <= exp["reached"])
    assert statuses == {0, 1, 2}
    random = fx.cases("random")
    assert len(random) == 16 and {tuple(c["shape"]) for c in random} == {(40, 44, 70)}
    assert int(fx.seeds(random[0]).max()) == 10
    assert sum("report" in c for c in cases) == 2
    assert os.path.getsize(fx._PATH) < 1000000


def test_existing_signatures_and_check_config_are_unchanged(no_device):
    from light_unet import inference, quantify
    sig = inspect.signature(quantify.lesion_uptake)
    assert list(sig.parameters) == ["uptake", "mask", "spacing", "threshold", "min_size", "peak_ml",
                                    "dmax", "resegment"]
    assert sig.parameters["resegment"].default is None
    assert inspect.signature(inference.infer_volume).parameters["resegment"].default is None
    assert quantify.check_config(None) == (1.0, True)
    assert quantify.check_config({"peak_ml": None, "dmax": False}) == (None, False)
    for key in ("resegment", "method", "value", "grow_mm"):
        with pytest.raises(ValueError, match="unknown keys"):
            quantify.check_config({key: 1.0})
    sig = inspect.signature(no_device.resegment_lesions)
    assert [(k, p.default) for k, p in sig.parameters.items() if p.default is not inspect._empty] == \
        [("spacing", (4.0, 4.0, 4.0)), ("method", "fixed"), ("value", 4.0), ("grow_mm", None),
         ("threshold", 0.5), ("min_size", 0), ("body_mask", None), ("max_lds_bytes", 0)]


def test_header_declares_the_resegment_exports():
    from light_unet import _native
    src = open(os.path.join(ROOT, "include", "l3u.h")).read()
    for name in ("l3u_rs_path", "l3u_rs_tiles", "l3u_rs_grow", "l3u_rs_sweep", "l3u_rs_commit"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _native.exported_symbols()
    assert re.search(r"#define\s+L3U_ABI_VERSION\s+5\b", src)
    assert _native.ABI_VERSION == 5 and _native.query("l3u_abi_version") == 5
    # two bitmaps and a 16-byte header in 64 KiB: 4095 words of 64 voxels
    assert _native.query("l3u_rs_path", 63, 65, 64, 0) == 0          # 4095 words
    assert _native.query("l3u_rs_path", 64, 64, 64, 0) == 1          # 4096
    assert _native.query("l3u_rs_path", 64, 64, 65, 0) == 1          # two words per row
    assert _native.query("l3u_rs_path", 10, 12, 20, 0) == 0
    assert _native.query("l3u_rs_path", 10, 12, 20, 16) == 1         # nothing fits: every seed tiled
    assert _native.query("l3u_rs_path", 1, 1, 64, 32) == 0
    assert _native.query("l3u_rs_path", 1, 1, 65, 32) == 1
    assert _native.query("l3u_rs_path", 10, 12, 20, 8) == -1
    assert _native.query("l3u_rs_path", 10, 12, 20, 64 * 1024 + 1) == -1
    assert _native.query("l3u_rs_path", 0, 12, 20, 0) == -1
    assert _native.query("l3u_rs_tiles", 10, 12, 20) == 2 * 2 * 1
    assert _native.query("l3u_rs_tiles", 8, 8, 256) == 1
    assert _native.query("l3u_rs_tiles", 9, 8, 257) == 2 * 1 * 2
    assert _native.query("l3u_rs_tiles", 0, 8, 8) == 0


def test_plan_partitions_the_tiled_boxes():
    from light_unet import resegment
    boxes = np.asarray([[0, 10, 0, 12, 0, 20], [2, 3, 4, 5, 6, 7], [0, 9, 0, 17, 3, 330]], np.int32)
    items, tiles, aoff, words = resegment._plan(boxes, 1024)   # 63 words per bitmap at the most
    assert items[:, 0].tolist() == [1, 2, 3] and items[:, 1:7].tolist() == boxes.tolist()
    assert items[:, 7].tolist() == [1, 0, 1]
    nw = [10 * 12 * 1, 1, 9 * 17 * 6]
    assert aoff.tolist() == [0, 0, 3 * nw[0]] and words == 3 * (nw[0] + nw[2])
    for i, (nz, ny, wpr) in ((0, (10, 12, 1)), (2, (9, 17, 6))):
        seen = np.zeros((nz, ny, wpr), np.int32)
        for _, z, y, w in tiles[tiles[:, 0] == i].tolist():
            seen[z:z + 8, y:y + 8, w:w + 4] += 1
        assert (seen == 1).all()
    assert not (tiles[:, 0] == 1).any()
    items, tiles, aoff, words = resegment._plan(boxes, 0)
    assert items[:, 7].tolist() == [0, 0, 0] and len(tiles) == 0 and words == 0
