"""The device draw stream's definition, restated on the host (light_unet.patches.restate_draws,
include/l3u.h "Training-patch draws on the device"): no GPU here.

  * the first records of one seed, pinned to values computed by hand from the definition (a
    separate C program of the splitmix64 composition, the 128-bit choice product and the three
    roundings of a range draw gave the same numbers);
  * the frequency of every decision over 4096 items of the mixed dataset: within
    5 * sqrt(p (1 - p) / N) of its configured probability, ranges and table indices in bounds
    (tests/test_aug_draw_gpu.py runs the same check on the device records, same seed);
  * argument handling that needs no device: an unknown `draws` / `device_patches` raises ValueError;
  * the ctypes mirrors have the sizes csrc/augdraw.hip asserts for the C structs."""
import ctypes
import math

import pytest

REF_AUG = {"gaussian_noise": {"enabled": True, "prob": 0.3, "sigma": 0.01},
           "intensity_shift": {"enabled": True, "prob": 0.5, "shift_range": [-0.1, 0.1]},
           "random_flip": {"enabled": True, "prob": 0.5, "axes": [0, 1, 2]},
           "random_rotation": {"enabled": True, "prob": 0.5, "angle_range": [-15, 15],
                               "axes": [[0, 1], [0, 2], [1, 2]]},
           "random_scale": {"enabled": True, "prob": 0.3, "scale_range": [0.9, 1.1]}}

FREQ_SEED, FREQ_B, FL_RATIO = 2024, 4096, 0.6


def freq_specs():
    """Two domains with tables of different sizes (all four non-empty)."""
    from light_unet.patches import DrawSpec
    fl = DrawSpec([(k % 2, (k, k + 1, k + 2)) for k in range(23)],
                  [(k % 2, (k + 3, k, k + 1)) for k in range(31)], 0.5, REF_AUG)
    dl = DrawSpec([(0, (k, 2 * k, k)) for k in range(11)],
                  [(0, (2 * k, k, k)) for k in range(17)], 0.5, REF_AUG)
    return fl, dl


def check_frequencies(recs, specs, fl_ratio, aug=REF_AUG):
    """Every decision's share of the N records against its probability (5 sigma of the binomial),
    the ranges and the table indices.  Both domains use `aug` and lesion ratio 0.5, so a decision's
    share over all items is its configured probability whatever the domain mix."""
    N = len(recs)

    def near(count, p, what):
        tol = 5.0 * math.sqrt(p * (1.0 - p) / N)
        assert abs(count / N - p) <= tol, (what, count / N, p, tol)

    near(sum(r.domain == 0 for r in recs), fl_ratio, "FL domain")
    near(sum(r.table == 0 for r in recs), 0.5, "lesion table")
    f, ro = aug["random_flip"], aug["random_rotation"]
    near(sum(r.flip_on for r in recs), f["prob"], "flip on")
    for ax in f["axes"]:
        near(sum(r.flip_axis == ax for r in recs), f["prob"] / len(f["axes"]), ("flip axis", ax))
    near(sum(r.rot_on for r in recs), ro["prob"], "rotation on")
    for pl in ro["axes"]:
        near(sum((r.rot_a0, r.rot_a1) == tuple(pl) for r in recs), ro["prob"] / len(ro["axes"]),
             ("rotation plane", pl))
    near(sum(r.scale_on for r in recs), aug["random_scale"]["prob"], "scale on")
    near(sum(r.shift_on for r in recs), aug["intensity_shift"]["prob"], "shift on")
    near(sum(r.noise_on for r in recs), aug["gaussian_noise"]["prob"], "noise on")
    for r in recs:
        sp = specs[r.domain]
        rows = sp.background if r.table else sp.lesion
        assert 0 <= r.loc < len(rows) and rows[r.loc] == (r.case_idx, (r.cz, r.cy, r.cx)), r
        if r.rot_on:
            assert ro["angle_range"][0] <= r.angle < ro["angle_range"][1], r
        else:
            assert r.angle == 0.0 and r.rot_a0 == r.rot_a1 == -1, r
        lo, hi = aug["random_scale"]["scale_range"]
        assert (lo <= r.scale < hi) if r.scale_on else r.scale == 0.0, r
        lo, hi = aug["intensity_shift"]["shift_range"]
        assert (lo <= r.shift < hi) if r.shift_on else r.shift == 0.0, r
        assert (r.flip_axis in f["axes"]) if r.flip_on else r.flip_axis == -1, r


def test_restatement_first_records_by_hand():
    from light_unet import patches as P
    # the splitmix64 composition itself
    key = P.draw_key(7, 0, 0)
    assert key == 0x64BF61B512FFABE7
    assert P.draw_bits(key, P.SLOT_LOCATION) == 0x651F268F5BD8D2F2
    assert (0x651F268F5BD8D2F2 * 3) >> 64 == 1                       # the row chosen among 3
    assert P.draw_bits(key, P.SLOT_NOISE_U1, 1) == 0x7A496346E01A7E2D
    sp =P.DrawSpec([(0, (1, 2, 3)), (1, (4, 5, 6))], [(0, (7, 8, 9))] * 3, 0.5, REF_AUG)
    r0, r1, r2 = P.restate_draws(7, 0, 3, sp)
    # item 0: u(TABLE) >= 0.5 -> background table, row (h * 3) >> 64 = 1; only the shift is on:
    # -0.1 + (0.1 - -0.1) * u(SHIFT)
    assert r0.astuple() == (0, 0, 1, 1, 7, 8, 9, 0, -1, 0, -1, -1, 0, 1, 0, 0, 0.0, 0.0,
                            0.07019310506708701)
    # item 1: lesion table row 0, flip about axis 0, nothing else
    assert r1.astuple() == (0, 0, 0, 0, 1, 2, 3, 1, 0, 0, -1, -1, 0, 0, 0, 0, 0.0, 0.0, 0.0)
    # item 2: background row 2, scale 0.9 + (1.1 - 0.9) * u(SCALE)
    assert r2.astuple() == (0, 0, 1, 2, 7, 8, 9, 0, -1, 0, -1, -1, 1, 0, 0, 0, 0.0,
                            1.05591828493923, 0.0)
    # Box-Muller of item 0's first voxels at sigma 0.01 (libm: compared to 4 ulp)
    nz = P.restate_noise(7, 0, 0, 3, 0.01)
    for got, want in zip(nz, [0.018427796167631398, -0.011756994969801949, 0.0005391633316625136]):
        assert abs(got - want) <= 4 * math.ulp(want), (got, want)
    # another step or item is another key
    assert P.restate_draws(7, 1, 3, sp) != [r0, r1, r2]
    assert len({P.draw_key(7, 0, 0), P.draw_key(7, 0, 1), P.draw_key(7, 1, 0), P.draw_key(8, 0, 0)}) == 4


def test_restatement_primitives():
    from light_unet import patches as P
    assert P._unit(0) == 0.0 and P._unit((1 << 64) - 1) == 1.0 - 2.0 ** -53
    for n in (1, 3, 7, 1000003):
        assert P._choice(0, n) == 0 and P._choice((1 << 64) - 1, n) == n - 1
    assert P._choice(1 << 63, 10) == 5
    # a single dataset makes no domain draw and an empty lesion table falls back to the background
    sp = P.DrawSpec([], [(0, (1, 1, 1)), (0, (2, 2, 2))], 1.0, None)
    recs = P.restate_draws(3, 5, 64, sp)
    assert all(r.table == 1 and r.domain == 0 and r.step == 5 for r in recs)
    assert all(not (r.flip_on or r.rot_on or r.scale_on or r.shift_on or r.noise_on) for r in recs)
    assert {r.loc for r in recs} == {0, 1}
    # ... and an empty background table to the lesion table, whatever the ratio
    sp = P.DrawSpec([(0, (1, 1, 1))], [], 0.0, None)
    assert all(r.table == 0 for r in P.restate_draws(3, 5, 16, sp))
    # mixed: an empty FL dataset always yields DLBCL and vice versa
    e, full = P.DrawSpec([], [], 0.5, None), P.DrawSpec([(0, (1, 1, 1))], [], 0.5, None)
    assert all(r.domain == 1 for r in P.restate_draws(3, 0, 32, (e, full), 0.9))
    assert all(r.domain == 0 for r in P.restate_draws(3, 0, 32, (full, e), 0.1))
    with pytest.raises(ValueError):
        P.restate_draws(3, 0, 4, (e, e), 0.5)
    with pytest.raises(ValueError):
        P.restate_draws(3, 0, 4, (full, full))


def test_restatement_frequencies():
    from light_unet.patches import restate_draws
    specs = freq_specs()
    recs = restate_draws(FREQ_SEED, 0, FREQ_B, specs, FL_RATIO)
    check_frequencies(recs, specs, FL_RATIO)


def test_unknown_draw_mode_raises_without_gpu():
    from light_unet import patches as P
    with pytest.raises(ValueError):
        P.DevicePatchDataset([], draws="gpu")
    with pytest.raises(ValueError):
        P.DeviceMixedPatchDataset(None, None, draws="both")
    with pytest.raises(ValueError):
        P.device_loader(object(), 4, draws="workers")
    with pytest.raises(ValueError):
        P.DevicePatchDataset.from_reference(object(), draws="")
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "l3u_plugin_argcheck", os.path.join(root, "light-3d-unet-front_amd", "l3u_plugin.py"))
    plug = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(plug)
    with pytest.raises(ValueError):
        plug.install(device_patches="device")


def test_ctypes_mirrors_have_the_c_sizes():
    from light_unet import _native as nat
    assert ctypes.sizeof(nat.AugCase) == 32 and ctypes.sizeof(nat.AugTables) == 32
    assert ctypes.sizeof(nat.AugCfg) == 232 and ctypes.sizeof(nat.AugDrawRec) == 88
    assert nat.AugDrawRec.angle.offset == 64 and nat.AugCfg.flip_axes.offset == 132
