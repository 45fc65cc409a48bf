"""draw_location_ranks (light_unet/patches.py) against the reference's own _sample_locations
results (patch_dataset.py:74-100), without a GPU: the ranks it draws from numpy-computed voxel
counts, mapped through np.argwhere, are the reference's recorded rows, and the global numpy
generator ends in the recorded state.  Every check is ==."""
import numpy as np
import pytest

import locations_fixture as LF
import loops_fixture as F
from light_unet import patches as P


def test_ranks_reproduce_loops_golden():
    """loops.npz, the standard-mode training dataset (no body masks): PatchDataset.__init__ seeds
    numpy with the config seed, and nothing draws from numpy between its construction and the
    recorded `rng_before` state (the DataLoader is built with num_workers = 0)."""
    z, meta = F.load()
    pre = "loader/standard/train_loader/"
    st = F.dataset_state(z, meta, pre)
    vols = F.cases(z, meta)
    lb = [(vols[cid][1], None) for cid in st["case_ids"]]
    np.random.seed(7)                      # make_loop_goldens._config: experiment.seed
    ranks = P.draw_location_ranks(LF.counts(lb))
    les, bg = LF.rows_of_ranks(lb, ranks)
    assert np.array_equal(les, LF.rows(st["lesion"]))
    assert np.array_equal(bg, LF.rows(st["background"]))
    assert LF.np_state_matches(z["loader/standard/rng_before/np_keys"],
                               z["loader/standard/rng_before/np_misc"])


def test_ranks_reproduce_locations_golden():
    """locations.npz: body masks, a case without lesions and one without background (both
    skipped randint calls), n // 1000 > 10 and n // 5000 > 10 sample counts."""
    z, meta = LF.load()
    lb = LF.cases(z, meta)
    cnt = LF.counts(lb)
    assert (cnt[:, 0] == 0).any() and (cnt[:, 1] == 0).any()
    assert (cnt[:, 0] // 1000 > 10).any() and (cnt[:, 1] // 5000 > 10).any()
    np.random.seed(meta["seed"])
    ranks = P.draw_location_ranks(cnt)
    assert [len(r[0]) for r in ranks] == [max(10, n // 1000) if n else 0 for n in cnt[:, 0]]
    assert [len(r[1]) for r in ranks] == [max(10, n // 5000) if n else 0 for n in cnt[:, 1]]
    les, bg = LF.rows_of_ranks(lb, ranks)
    assert np.array_equal(les, z["lesion"])
    assert np.array_equal(bg, z["background"])
    assert LF.np_state_matches(z["rng_after/np_keys"], z["rng_after/np_misc"])


def test_ranks_take_a_private_generator():
    rs = np.random.RandomState(3)
    before = np.random.get_state()[1].copy()
    ranks = P.draw_location_ranks([(2500, 0), (0, 0), (1, 60000)], rng=rs)
    assert np.array_equal(np.random.get_state()[1], before)
    exp = np.random.RandomState(3)
    assert np.array_equal(ranks[0][0], exp.randint(2500, size=10)) and len(ranks[0][1]) == 0
    assert len(ranks[1][0]) == 0 and len(ranks[1][1]) == 0
    assert np.array_equal(ranks[2][0], exp.randint(1, size=10))
    assert np.array_equal(ranks[2][1], exp.randint(60000, size=12))
    assert all(r.dtype == np.int64 for pair in ranks for r in pair)


def test_bad_locate_is_rejected():
    with pytest.raises(ValueError, match="locate"):
        P.DevicePatchDataset([], locate="bogus")


def test_bad_device_locations_is_rejected():
    import l3u_plugin
    for bad in ("x", 1, None):
        with pytest.raises(ValueError, match="device_locations"):
            l3u_plugin.install(device_locations=bad)
