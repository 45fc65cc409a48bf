"""Patch locations on the device (csrc/locate.hip, light_unet/patches.py locate="device"):
l3u_loc_count / l3u_loc_select against np.flatnonzero + np.unravel_index, and the dataset paths
against the reference's recorded _sample_locations results.  Every check is ==."""
import sys
import types

import numpy as np
import pytest
import torch

import locations_fixture as LF
import loops_fixture as F
from light_unet import _native as nat
from light_unet import patches as P

pytestmark = pytest.mark.gpu

BLOCK = 4096
SHAPES = [(5, 7, 9),          # under one block, n % 64 != 0
          (17, 16, 16),       # 4352 voxels: one block plus a 256-voxel tail
          (33, 31, 29),       # odd everywhere
          (40, 44, 36),
          (96, 96, 128)]      # 288 blocks
NP_DT = {"f32": np.float32, "f64": np.float64}


# ------------------------------------------------------------------------------- helpers
def make_case(shape, dtype, with_body, seed=0):
    """A label with lesion values, NaN, negatives, set voxels at flat 0 and n - 1 and (from 6
    blocks on) two all-zero 4096-blocks in the middle; a body mask that is zero over that run
    too, so both classes' prefixes have a plateau there."""
    rng = np.random.default_rng(seed + 17 * int(np.prod(shape)))
    n = int(np.prod(shape))
    lab = np.zeros(n, dtype)
    u = rng.random(n)
    lab[u < 0.06] = 1.0
    lab[(u >= 0.06) & (u < 0.08)] = 2.5
    lab[(u >= 0.08) & (u < 0.09)] = np.nan
    lab[(u >= 0.09) & (u < 0.11)] = -1.0
    lab[(u >= 0.11) & (u < 0.12)] = -0.0
    body = None
    if with_body:
        body = rng.choice(np.array([0, 1, 3], np.uint8), size=n, p=[0.3, 0.5, 0.2])
    nb = -(-n // BLOCK)
    if nb >= 6:
        lab[2 * BLOCK:4 * BLOCK] = 0.0
        if with_body:
            body[2 * BLOCK:4 * BLOCK] = 0
    lab[0] = lab[n - 1] = 1.0
    return lab.reshape(shape), (body.reshape(shape) if with_body else None)


def masks_of(lab, body):
    return LF.class_masks(lab, None if body is None else body != 0)


def ref_prefix(lab, body):
    """uint32-valued [2, nblocks + 1] exclusive prefix of the per-block class counts."""
    n = lab.size
    nb = -(-n // BLOCK)
    out = np.zeros((2, nb + 1), np.int64)
    for c, m in enumerate(masks_of(lab, body)):
        pad = np.zeros(nb * BLOCK, np.int64)
        pad[:n] = m.reshape(-1)
        out[c, 1:] = np.cumsum(pad.reshape(nb, BLOCK).sum(1))
    return out


def ref_rows(lab, body, cls, ranks, case_idx):
    flat = np.flatnonzero(masks_of(lab, body)[cls].reshape(-1))
    out = np.full((len(ranks), 4), -1, np.int64)
    out[:, 0] = case_idx
    for k, r in enumerate(ranks):
        if 0 <= r < len(flat):
            out[k, 1:] = np.unravel_index(flat[r], lab.shape)
    return out


def dev_count(lab_t, body_t):
    nb = nat.query("l3u_loc_nblocks", lab_t.numel())
    prefix = torch.full((2 * (nb + 1),), -1, dtype=torch.int32, device=lab_t.device)
    nat.call("l3u_loc_count", lab_t.data_ptr(), P._LOC_DTYPES[lab_t.dtype], nat.ptr(body_t),
             lab_t.numel(), prefix.data_ptr(), nat.stream())
    return prefix


def as_counts(prefix):
    return prefix.cpu().numpy().view(np.uint32).astype(np.int64).reshape(2, -1)


def dev_select(lab_t, body_t, prefix, cls, ranks, case_idx):
    R = len(ranks)
    rows = torch.full((R + 1, 4), -7, dtype=torch.int32, device=lab_t.device)
    rk = torch.tensor(list(ranks) + [0], dtype=torch.int64, device=lab_t.device)
    nat.call("l3u_loc_select", lab_t.data_ptr(), P._LOC_DTYPES[lab_t.dtype], nat.ptr(body_t),
             *lab_t.shape, prefix.data_ptr(), cls, rk.data_ptr(), R, case_idx, rows.data_ptr(),
             nat.stream())
    out = rows.cpu().numpy().astype(np.int64)
    assert (out[R] == -7).all()                      # nothing written past the R rows
    return out[:R]


def rank_set(pre, every):
    """Ranks to ask for, from one class's reference prefix: 0 and total - 1, a duplicate, the
    last voxel of a block and the first of the next non-empty one (across every plateau too),
    `total` and -1 (out of range); every rank when `every`."""
    total = int(pre[-1])
    if total == 0:
        return [0, -1]
    if every:
        return list(range(total)) + [total, -1]
    ranks = [0, total - 1, total // 2, total // 2, total, -1, total + 5]
    edges = sorted({int(v) for v in pre[1:-1] if 0 < v < total})
    pick = edges[:3] + edges[-2:] + [int(pre[2])] if len(pre) > 3 else edges
    for e in pick:
        if 0 < e < total:
            ranks += [e - 1, e]
    return ranks


def upload(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("with_body", [False, True], ids=["nobody", "body"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_count_and_select(cuda, shape, dt, with_body):
    lab, body = make_case(shape, NP_DT[dt], with_body)
    if with_body and dt == "f32":
        body = body != 0                               # torch.bool storage; f64 keeps uint8 0 / 1 / 3
    lab_t, body_t = upload(lab, cuda), upload(body, cuda)
    pre = ref_prefix(lab, body)
    prefix = dev_count(lab_t, body_t)
    assert np.array_equal(as_counts(prefix), pre)
    if pre.shape[1] - 1 >= 6:                          # the plateau is there, in both classes
        assert pre[0, 2] == pre[0, 3] == pre[0, 4]
        assert not with_body or pre[1, 2] == pre[1, 3] == pre[1, 4]
    for cls in (0, 1):
        ranks = rank_set(pre[cls], every=shape == SHAPES[0])
        got = dev_select(lab_t, body_t, prefix, cls, ranks, case_idx=3 + cls)
        assert np.array_equal(got, ref_rows(lab, body, cls, ranks, 3 + cls))
    flat0 = dev_select(lab_t, body_t, prefix, 0, [0, int(pre[0, -1]) - 1], 0)
    assert tuple(flat0[0, 1:]) == (0, 0, 0) and tuple(flat0[1, 1:]) == tuple(s - 1 for s in shape)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_unaligned_pointers_take_the_scalar_path(cuda, dt):
    """A label one element and a mask one byte off a 16-byte boundary: every block, whole ones
    too, goes through the clamped one-voxel-per-lane loads."""
    shape = (17, 16, 16)
    lab, body = make_case(shape, NP_DT[dt], True, seed=5)
    n = lab.size
    lbuf = torch.zeros(n + 1, dtype=torch.float32 if dt == "f32" else torch.float64, device=cuda)
    bbuf = torch.zeros(n + 1, dtype=torch.uint8, device=cuda)
    lbuf[1:] = upload(lab.reshape(-1), cuda)
    bbuf[1:] = upload(body.reshape(-1), cuda)
    lab_t, body_t = lbuf[1:].view(shape), bbuf[1:].view(shape)
    assert lab_t.data_ptr() % 16 != 0 and body_t.data_ptr() % 2 != 0
    pre = ref_prefix(lab, body)
    prefix = dev_count(lab_t, body_t)
    assert np.array_equal(as_counts(prefix), pre)
    for cls in (0, 1):
        ranks = rank_set(pre[cls], every=False)
        assert np.array_equal(dev_select(lab_t, body_t, prefix, cls, ranks, 1),
                              ref_rows(lab, body, cls, ranks, 1))


def test_empty_classes_and_no_ranks(cuda):
    shape = (17, 16, 16)
    n = int(np.prod(shape))
    ones, zeros = np.ones(shape, np.float32), np.zeros(shape, np.float32)
    nobody = np.zeros(shape, bool)
    for lab, body, totals in ((ones, None, (n, 0)), (zeros, None, (0, n)), (zeros, nobody, (0, 0)),
                              (ones, nobody, (n, 0))):
        lab_t, body_t = upload(lab, cuda), upload(body, cuda)
        prefix = dev_count(lab_t, body_t)
        assert np.array_equal(as_counts(prefix), ref_prefix(lab, body))
        assert tuple(as_counts(prefix)[:, -1]) == totals
        for cls in (0, 1):
            ranks = [0, totals[cls] - 1, totals[cls], -1]
            assert np.array_equal(dev_select(lab_t, body_t, prefix, cls, ranks, 2),
                                  ref_rows(lab, body, cls, ranks, 2))
            assert dev_select(lab_t, body_t, prefix, cls, [], 2).shape == (0, 4)   # R = 0
    # R = 0 is a success without a launch: no pointer is looked at
    assert nat.load().l3u_loc_select(None, 0, None, 4, 4, 4, None, 0, None, 0, 0, None, None) == 0


def test_out_of_range_sizes_are_refused(cuda):
    lib = nat.load()
    assert nat.query("l3u_loc_nblocks", 2 ** 31) == 0 and nat.query("l3u_loc_nblocks", 0) == 0
    assert nat.query("l3u_loc_nblocks", 2 ** 31 - 1) == 2 ** 19
    assert nat.query("l3u_loc_nblocks", 4097) == 2
    for n in (2 ** 31, 2 ** 33, 0, -1):
        assert lib.l3u_loc_count(None, 0, None, n, None, None) != 0
    assert lib.l3u_loc_select(None, 0, None, 2048, 1024, 1024, None, 0, None, 1, 0, None, None) != 0
    assert lib.l3u_loc_select(None, 0, None, 0, 4, 4, None, 0, None, 1, 0, None, None) != 0
    torch.cuda.synchronize()                           # nothing was launched: nothing can fault


# ------------------------------------------------------------------------------- the host paths
@pytest.fixture(scope="module")
def loc_golden():
    z, meta = LF.load()
    return z, meta, LF.cases(z, meta)


@pytest.fixture(scope="module")
def loops_golden():
    z, meta = F.load()
    st = F.dataset_state(z, meta, "loader/standard/train_loader/")
    vols = F.cases(z, meta)
    return z, st, [vols[cid] for cid in st["case_ids"]]


def test_location_counts(cuda, loc_golden):
    z, meta, lb = loc_golden
    got = P.location_counts([upload(l, cuda) for l, _ in lb], [upload(b, cuda) for _, b in lb])
    assert got.dtype == np.int64 and np.array_equal(got, LF.counts(lb))
    got64 = P.location_counts([upload(l.astype(np.float64), cuda) for l, _ in lb],
                              [upload(b, cuda) for _, b in lb])
    assert np.array_equal(got64, LF.counts(lb))


def test_sample_locations_device_on_locations_golden(cuda, loc_golden):
    z, meta, lb = loc_golden
    np.random.seed(meta["seed"])
    les, bg = P.sample_locations_device([upload(l, cuda) for l, _ in lb],
                                        [upload(b, cuda) for _, b in lb])
    assert les.dtype == bg.dtype == torch.int32 and les.is_cuda and bg.is_cuda
    assert np.array_equal(les.cpu().numpy(), z["lesion"])
    assert np.array_equal(bg.cpu().numpy(), z["background"])
    assert LF.np_state_matches(z["rng_after/np_keys"], z["rng_after/np_misc"])


def test_sample_locations_device_on_loops_golden(cuda, loops_golden):
    z, st, vols = loops_golden
    np.random.seed(7)
    les, bg = P.sample_locations_device([upload(lab, cuda) for _, lab in vols])
    assert np.array_equal(les.cpu().numpy(), LF.rows(st["lesion"]))
    assert np.array_equal(bg.cpu().numpy(), LF.rows(st["background"]))
    assert LF.np_state_matches(z["loader/standard/rng_before/np_keys"],
                               z["loader/standard/rng_before/np_misc"])


def _check_dataset(ds, lesion_rows, background_rows):
    assert np.array_equal(LF.rows(ds.lesion_locations), lesion_rows)
    assert np.array_equal(LF.rows(ds.background_locations), background_rows)
    assert all(isinstance(c, int) and zyx.dtype == np.int64 and zyx.shape == (3,)
               for c, zyx in ds.lesion_locations + ds.background_locations)
    les, bg = ds.location_tables
    assert np.array_equal(les.cpu().numpy(), lesion_rows) and np.array_equal(bg.cpu().numpy(), background_rows)
    assert len(ds) == len(lesion_rows) + len(background_rows)


def test_dataset_locate_device_on_goldens(cuda, loc_golden, loops_golden):
    z, meta, lb = loc_golden
    cases = [(np.zeros_like(l), l, b) for l, b in lb]
    ds = P.DevicePatchDataset(cases, patch_size=(8, 8, 8), seed=meta["seed"], locate="device")
    _check_dataset(ds, z["lesion"], z["background"])
    assert LF.np_state_matches(z["rng_after/np_keys"], z["rng_after/np_misc"])
    host = P.DevicePatchDataset(cases, patch_size=(8, 8, 8), seed=meta["seed"])
    assert host.locate == "host" and host.location_tables is None
    assert np.array_equal(LF.rows(host.lesion_locations), z["lesion"])
    assert LF.np_state_matches(z["rng_after/np_keys"], z["rng_after/np_misc"])
    zl, st, vols = loops_golden
    ds = P.DevicePatchDataset(vols, patch_size=(16, 16, 16), seed=7, locate="device")
    _check_dataset(ds, LF.rows(st["lesion"]), LF.rows(st["background"]))
    assert LF.np_state_matches(zl["loader/standard/rng_before/np_keys"],
                               zl["loader/standard/rng_before/np_misc"])


def test_dataset_takes_device_tensors_and_bool_masks(cuda, loc_golden):
    z, meta, lb = loc_golden
    cases = []
    for l, b in lb:
        lab_t = upload(l, cuda)
        case = (torch.zeros_like(lab_t), lab_t)
        cases.append(case if b is None else case + (upload(b, cuda),))
    assert any(len(c) == 3 and c[2].dtype == torch.bool for c in cases)
    ds = P.DevicePatchDataset(cases, patch_size=(8, 8, 8), seed=meta["seed"], locate="device")
    _check_dataset(ds, z["lesion"], z["background"])
    assert ds.vols[0][1].data_ptr() == cases[0][1].data_ptr()      # no copy of a float32 device case
    x, t = ds.sample_batch(3)                                      # host draws work on top of it
    assert x.shape == t.shape == (3, 1, 8, 8, 8)


def test_device_draws_use_the_device_tables(cuda, loc_golden):
    """Same tables => same draws: the first batch's records equal those of a locate="host"
    dataset with the same seeds, and the draw tables ARE the location tables (no second upload)."""
    z, meta, lb = loc_golden
    aug = {"random_flip": {"enabled": True, "prob": 0.5, "axes": [0, 1, 2]},
           "intensity_shift": {"enabled": True, "prob": 0.5, "shift_range": [-0.1, 0.1]}}
    cases = [(np.zeros_like(l), l, b) for l, b in lb]
    kw = dict(patch_size=(8, 8, 8), augmentation=aug, seed=meta["seed"], draws="device", draw_seed=99)
    dev = P.DevicePatchDataset(cases, locate="device", **kw)
    host = P.DevicePatchDataset(cases, locate="host", **kw)
    ra, rb = dev.draw_records(16), host.draw_records(16)
    assert ra == rb and {r.table for r in ra} == {0, 1}
    t = dev._dd.tables[0]
    assert (t.lesion, t.background) == tuple(x.data_ptr() for x in dev.location_tables)
    assert (t.n_lesion, t.n_background) == tuple(len(x) for x in dev.location_tables)


def test_bind_sample_locations_on_a_stand_in(cuda, loc_golden):
    """A stand-in PatchDataset with the reference's attribute names (cases with label_path /
    body_mask_path, _load_body_mask_array, _sample_locations) in a module with a `nib` stand-in."""
    z, meta, lb = loc_golden
    store = {}
    for cid, (l, b) in zip(meta["case_ids"], lb):
        store[f"lab/{cid}"] = l
        if b is not None:
            store[f"body/{cid}"] = b.astype(np.uint8)

    class _Img:
        def __init__(self, a):
            self.a = a

        def get_fdata(self):
            return np.asarray(self.a, np.float64)

    mod = types.ModuleType("l3u_test_patch_dataset")
    mod.nib = types.SimpleNamespace(load=lambda path: _Img(store[path]))
    sys.modules[mod.__name__] = mod

    class PatchDataset:
        def __init__(self):
            self.cases = [{"case_id": cid, "label_path": f"lab/{cid}",
                           "body_mask_path": f"body/{cid}" if f"body/{cid}" in store else None}
                          for cid in meta["case_ids"]]

        def _load_body_mask_array(self, case):
            if case["body_mask_path"] is not None:
                return mod.nib.load(case["body_mask_path"]).get_fdata().astype(bool)
            return None

        def _sample_locations(self):               # the numpy form, on the same reads
            return P.DevicePatchDataset._sample_locations(
                [(None, mod.nib.load(c["label_path"]).get_fdata(), self._load_body_mask_array(c))
                 for c in self.cases])
    PatchDataset.__module__ = mod.__name__
    mod.PatchDataset = PatchDataset
    try:
        original = PatchDataset._sample_locations
        P.bind_sample_locations(PatchDataset)
        assert PatchDataset._l3u_reference_sample_locations is original
        assert PatchDataset._sample_locations is not original
        ds = PatchDataset()
        np.random.seed(meta["seed"])
        exp = ds._l3u_reference_sample_locations()
        state = np.random.get_state()
        np.random.seed(meta["seed"])
        got = ds._sample_locations()
        for g, e, rows in zip(got, exp, (z["lesion"], z["background"])):
            assert np.array_equal(LF.rows(g), LF.rows(e)) and np.array_equal(LF.rows(g), rows)
            assert all(isinstance(c, int) and zyx.dtype == np.int64 for c, zyx in g)
        assert LF.np_state_matches(state[1], state[2:])
        P.bind_sample_locations(PatchDataset)          # binding twice keeps the original reachable
        assert PatchDataset._l3u_reference_sample_locations is original
    finally:
        del sys.modules[mod.__name__]
