"""The lesion uptake report, the parts that need no GPU: argument errors are raised before any
device access, the host-built offset table equals the golden's, the golden file is consistent with
itself, and the C header declares the exports."""
import os
import re

import numpy as np
import pytest

import quantify_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def no_device(monkeypatch):
    """Any device access of the module under test fails the test (also where a GPU is present)."""
    from light_unet import _native, lesion, quantify

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(quantify, "_device", boom)
    monkeypatch.setattr(lesion, "_device", boom)
    monkeypatch.setattr(_native, "call", boom)
    monkeypatch.setattr(_native, "query", boom)
    return quantify


def test_argument_errors_come_before_the_device(no_device):
    q = no_device
    u = np.zeros((4, 5, 6), np.float32)
    with pytest.raises(ValueError, match="differ in shape"):
        q.lesion_uptake(u, np.zeros((4, 5, 7), np.float32))
    with pytest.raises(ValueError, match=r"\[D, H, W\]"):
        q.lesion_uptake(np.zeros((5, 6), np.float32), np.zeros((5, 6), np.float32))
    with pytest.raises(ValueError, match=r"\[D, H, W\]"):
        q.lesion_uptake(np.zeros((1, 4, 5, 6), np.float32), np.zeros((1, 4, 5, 6), np.float32))
    with pytest.raises(ValueError, match=r"\[D, H, W\]"):
        q.lesion_uptake(np.zeros((0, 5, 6), np.float32), np.zeros((0, 5, 6), np.float32))
    with pytest.raises(ValueError, match=r"\[D, H, W\]"):
        q.lesion_uptake(u, np.zeros((1, 4, 5, 6), np.float32))
    for bad in ((4.0, 0.0, 4.0), (4.0, -1.0, 4.0), (4.0, 4.0), (4.0, float("nan"), 4.0), 4.0):
        with pytest.raises(ValueError, match="spacing"):
            q.lesion_uptake(u, u, spacing=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="peak_ml"):
            q.lesion_uptake(u, u, peak_ml=bad)
    # 1 ml is r = 6.204 mm: at 1.24 mm or less on an axis the sphere reaches a fifth voxel
    with pytest.raises(ValueError, match="resample"):
        q.lesion_uptake(u, u, spacing=(4.0, 4.0, 1.24))
    assert q.sphere_offsets((4.0, 4.0, 1.25))[1] == (1, 1, 4)
    with pytest.raises(ValueError, match="axis 0"):
        q.lesion_uptake(u, u, spacing=(1.2, 4.0, 4.0))
    with pytest.raises(ValueError, match="resample"):
        q.lesion_uptake(u, u, spacing=(4.0, 4.0, 4.0), peak_ml=40.0)
    with pytest.raises(ValueError, match="resample"):
        q.sphere_offsets((0.1, 0.1, 0.1))
    assert q.sphere_offsets((4.0, 4.0, 1.56))[1] == (1, 1, 3)


def test_check_config(no_device):
    q = no_device
    assert q.check_config(None) == (1.0, True)
    assert q.check_config({}) == (1.0, True)
    assert q.check_config({"peak_ml": None, "dmax": False}) == (None, False)
    assert q.check_config({"peak_ml": 0.5}) == (0.5, True)
    with pytest.raises(ValueError, match="unknown keys"):
        q.check_config({"peak": 1.0})
    with pytest.raises(ValueError, match="dict"):
        q.check_config([1.0])
    with pytest.raises(ValueError, match="peak_ml"):
        q.check_config({"peak_ml": 0.0})


def test_infer_volume_checks_the_uptake_arguments_first(no_device):
    from light_unet import inference
    img = np.zeros((8, 8, 8), np.float32)
    with pytest.raises(ValueError, match="unknown keys"):
        inference.infer_volume(img, None, {}, uptake=img, quantify={"peak": 1.0})
    with pytest.raises(ValueError, match="grid"):
        inference.infer_volume(img, None, {}, uptake=np.zeros((8, 8, 9), np.float32))
    with pytest.raises(ValueError, match="grid"):
        inference.infer_volume(img, None, {}, uptake=img, native_shape=(9, 9, 9))
    with pytest.raises(ValueError, match="uptake"):
        inference.infer_volume(img, None, {}, quantify={"dmax": False})


def test_offset_table_equals_the_golden(no_device):
    q = no_device
    _, index = fx.load()
    assert [len(o["offsets"]) for o in index["offsets"]] == [19, 71, 123]
    for o in index["offsets"]:
        offs, reach = q.sphere_offsets(o["spacing"], o["peak_ml"])
        assert offs.dtype == np.int32 and offs.flags.c_contiguous
        assert offs.tolist() == o["offsets"]
        assert reach == tuple(int(v) for v in np.abs(np.asarray(o["offsets"])).max(axis=0))
        assert sorted(map(tuple, offs.tolist())) == list(map(tuple, offs.tolist()))   # C order
    assert len(q.sphere_offsets((3.0, 1.5, 1.5))[0]) == 157
    assert q.sphere_offsets((2.0, 2.0, 2.0))[1] == (3, 3, 3)


def test_native_error_without_a_device(monkeypatch):
    import torch
    from light_unet import _native, quantify
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    u = np.zeros((4, 5, 6), np.float32)
    with pytest.raises(_native.NativeError, match="no GPU"):
        quantify.lesion_uptake(u, u)


def test_items_partition_every_box():
    from light_unet import quantify
    stats = np.zeros((3, 12), dtype=np.uint64)
    stats[0, 4:7], stats[0, 7:10] = (0, 0, 0), (0, 0, 0)                 # one voxel
    stats[1, 4:7], stats[1, 7:10] = (2, 3, 4), (40, 66, 67)              # 39 planes of 64 x 64
    stats[2, 4:7], stats[2, 7:10] = (1, 0, 0), (3, 399, 599)             # planes above the slab size
    items, first = quantify._items(stats)
    assert items.dtype == np.int32 and items.shape[1] == 8 and first.tolist()[0] == 0
    assert first.tolist() == [0, 1, 1 + 5, 1 + 5 + 3]                    # 8 planes per slab; 1 each
    for l in range(3):
        rows = items[first[l]:first[l + 1]]
        assert np.all(rows[:, 0] == l + 1) and np.all(rows[:, 7] == 0)
        assert rows[0, 1] == stats[l, 4] and rows[-1, 2] == stats[l, 7] + 1
        assert np.all(rows[1:, 1] == rows[:-1, 2]) and np.all(rows[:, 2] > rows[:, 1])
        assert np.all(rows[:, 3:7] == [stats[l, 5], stats[l, 8] + 1, stats[l, 6], stats[l, 9] + 1])
        planes = (rows[:, 2] - rows[:, 1]).max()
        assert planes == 1 or planes * (rows[0, 4] - rows[0, 3]) * (rows[0, 6] - rows[0, 5]) \
            <= quantify.SLAB_VOXELS


# ---------------------------------------------------------------- the golden file, numpy only
def _farthest(vox, spacing):
    d = (vox[:, None, :] - vox[None, :, :]).astype(np.float64) * np.asarray(spacing, np.float64)
    d = d * d
    d = (d[..., 0] + d[..., 1]) + d[..., 2]
    d[np.tril_indices(len(vox))] = -1.0
    k = int(np.argmax(d))
    return float(d.flat[k]), vox[k // len(vox)].tolist(), vox[k % len(vox)].tolist()


def test_golden_file_is_self_consistent():
    entries = fx.entries()
    assert len(entries) >= 60
    assert {tuple(e["shape"]) for e in entries} == {(1, 1, 5), (5, 9, 70), (3, 40, 129), (12, 20, 70),
                                                    (24, 40, 40), (2, 3, 600)}
    assert {e["family"] for e in entries} == {"a", "b"}
    assert any(e["min_size"] > 0 for e in entries) and sum("peak" in e for e in entries) == 3
    checked = 0
    for e in entries:
        shape, exp = tuple(e["shape"]), fx.unhex(e["expected"])
        corner = fx.bits(e["corner"], shape)
        m = fx.mask(e)
        assert not (corner & ~m).any()
        assert exp["n_lesions"] == len(exp["lesions"])
        total = sum(r["voxels"] for r in exp["lesions"])
        if e["min_size"] == 0:
            assert total == int(m.sum())
        assert all(r["voxels"] >= e["min_size"] for r in exp["lesions"])
        assert exp["tmtv_ml"] == float(np.int64(total) * (e["spacing"][0] * e["spacing"][1]
                                                          * e["spacing"][2] / 1000.0))
        up = fx.uptake(e)
        for r in exp["lesions"]:
            assert float(up[tuple(r["suv_max_voxel"])]) == r["suv_max"]
            assert m[tuple(r["suv_max_voxel"])] and m[tuple(r["suv_peak_voxel"])]
            assert r["tlg"] == r["suv_mean"] * r["volume_ml"]
        if e["family"] == "a":      # multiples of 2^-10: every sum is exact
            assert np.array_equal(up.astype(np.float64) * 1024.0, np.round(up.astype(np.float64) * 1024.0))
        # the stored corner mask reproduces the stored Dmax by brute force
        vox = np.argwhere(corner)
        if total < 2:
            assert exp["dmax_mm"] == 0.0 and exp["dmax_voxels"] is None and len(vox) == total
        elif len(vox) <= 2500:
            d2, a, b = _farthest(vox, e["spacing"])
            assert float(np.sqrt(d2)) == exp["dmax_mm"] and [a, b] == exp["dmax_voxels"], e["name"]
            checked += 1
    assert checked >= 40
    const = [e for e in entries if e["uptake"].startswith("const_")]
    assert len(const) == 3
    for e in const:
        for r in fx.unhex(e["expected"])["lesions"]:
            assert r["suv_max"] == r["suv_peak"] == r["suv_mean"] == 2.5
            # every maximum ties: the first voxel of the lesion wins
            assert r["suv_max_voxel"] == r["suv_peak_voxel"]
    assert any(fx.uptake(e).min() < 0 for e in entries if e["family"] == "a")


def test_header_declares_the_quantify_exports():
    from light_unet import _native
    src = open(os.path.join(ROOT, "include", "l3u.h")).read()
    for name in ("l3u_qt_peak", "l3u_qt_reduce", "l3u_qt_corner_blocks", "l3u_qt_corners",
                 "l3u_qt_compact", "l3u_qt_pair_parts", "l3u_qt_farthest"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _native.exported_symbols()
    assert re.search(r"#define\s+L3U_ABI_VERSION\s+5\b", src)
    assert _native.ABI_VERSION == 5 and _native.query("l3u_abi_version") == 5
    assert _native.query("l3u_qt_corner_blocks", 5, 9, 70) == 1          # 90 words
    assert _native.query("l3u_qt_corner_blocks", 204, 204, 450) == 1301  # 8 words per row
    assert _native.query("l3u_qt_corner_blocks", 2048, 1024, 1024) == 0  # 2^31 voxels
    assert _native.query("l3u_qt_pair_parts", 1) == 0
    assert _native.query("l3u_qt_pair_parts", 2) == 1
    assert _native.query("l3u_qt_pair_parts", 257) == 2
    assert _native.query("l3u_qt_pair_parts", 1 << 18) == 1024 * 128
    assert _native.query("l3u_qt_pair_parts", (1 << 18) + 1) == 0
