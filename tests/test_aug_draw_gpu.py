"""Training-patch draws on the device (csrc/augdraw.hip l3u_aug_draw, light_unet/patches.py
draws="device") against the host restatement of the generator (patches.restate_draws), the host
aug_param and the augmentation oracle (oracle/augment_oracle.py, pinned to scipy).

Shapes: patch (24, 20, 28) -- non-cubic, so an axis mix-up shows -- over two cases of
(40, 36, 44) and (30, 26, 32); the smaller one is under two patches wide, so crops clamp at 0 and
are zero-padded at the far end.  Patches are checked with tests/test_patches_gpu.py's tolerances
(images <= 1e-6, labels differing in <= 1e-4 of the voxels, crops bit-exact).

Two bounds are measurements with a factor-4 margin, because neither side pins the last ulp of
cos / sin / log (device ocml vs scipy's cephes cosdg / sindg and libm):
  * ROT_BOUND: largest |device - aug_param| over rot_c, rot_s, rot_off0, rot_off1 of the draws of
    test_draws_equal_restatement; measured 1.776e-15 on the MI355X (both configurations), so the
    bound is 7.105e-15.
  * NOISE_REL_BOUND: largest |device - restate_noise| / |restate_noise| over one 13,440-voxel
    patch; measured 4.306e-16, so the bound is 1.722e-15."""
import numpy as np
import pytest
import torch

from oracle import augment_oracle as A
from test_aug_draw import FL_RATIO, FREQ_B, FREQ_SEED, check_frequencies, freq_specs
from test_patches_gpu import ALL_ON, REF_AUG, _check

pytestmark = pytest.mark.gpu

PATCH = (24, 20, 28)
MEASURED_ROT = 1.7763568394002505e-15        # 2^-49: one ulp of an offset between 8 and 16
MEASURED_NOISE_REL = 4.305636500770773e-16   # about two ulps
ROT_BOUND = 4 * MEASURED_ROT
NOISE_REL_BOUND = 4 * MEASURED_NOISE_REL


def _cases(seed=0):
    """tests/test_patches_gpu.py _cases at the small shapes."""
    rng = np.random.default_rng(seed)
    out = []
    for shape in [(40, 36, 44), (30, 26, 32)]:
        img = rng.random(shape, dtype=np.float32) * 0.3
        lab = np.zeros(shape, np.float32)
        zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
        for _ in range(4):
            c = [rng.integers(0, s) for s in shape]
            r = rng.uniform(2, 5)
            m = (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r
            lab[m] = 1.0
            img[m] = rng.uniform(0.6, 1.0)
        out.append((img, lab))
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


def _ds(cases, aug, seed=11, **kw):
    from light_unet.patches import DevicePatchDataset
    return DevicePatchDataset(cases, PATCH, 0.5, aug, seed=seed, draws="device", **kw)


def _mixed(cases, aug, seed=11, fl_ratio=0.6, patch=PATCH):
    from light_unet.patches import DeviceMixedPatchDataset, DevicePatchDataset
    fl = DevicePatchDataset(cases, patch, 0.5, aug, seed=seed)
    dl = DevicePatchDataset(cases[::-1], patch, 0.5, aug, seed=seed + 1)
    return DeviceMixedPatchDataset(fl, dl, fl_ratio, draws="device")


INT_FIELDS = ("z0", "y0", "x0", "sd", "sh", "sw", "pz", "py", "px", "flip", "rot_a0", "rot_a1",
              "zoom", "shift_on", "noise_on", "image", "label")


@pytest.mark.parametrize("aug", [REF_AUG, ALL_ON], ids=["ref_aug", "all_on"])
def test_draws_equal_restatement(cuda, cases, aug):
    """B = 8 at three consecutive steps: every field of the device records == restate_draws; the
    l3u_aug_param integer fields, zs / zst / zf and the float shift == aug_param of the same draw;
    rot_c / rot_s / offsets within ROT_BOUND of aug_param's (scipy cosdg / sindg): the largest
    difference measured over these draws is 1.776e-15, the bound four times that."""
    from light_unet.patches import aug_param, restate_draws
    ds = _ds(cases, aug)
    seed, step0 = ds.draw_state()
    assert step0 == 0
    worst = 0.0
    for step in range(3):
        ds.sample_batch(8)
        recs = ds.last_records
        want = restate_draws(seed, step, 8, ds.draw_spec())
        for k, (r, w) in enumerate(zip(recs, want)):
            assert r.astuple() == w.astuple(), (step, k, r, w)
        prm = ds._dd.params()
        for k, r in enumerate(recs):
            img_t, lab_t = ds.vols[r.case_idx]
            hp = aug_param(img_t, lab_t, r.center, PATCH, r.aug_draw(noise=True))
            p = prm[k]
            for f in INT_FIELDS:
                assert getattr(p, f) == getattr(hp, f), (step, k, f)
            assert list(p.zs) == list(hp.zs) and list(p.zst) == list(hp.zst), (step, k)
            assert list(p.zf) == list(hp.zf), (step, k, list(p.zf), list(hp.zf))
            assert p.shift == hp.shift, (step, k)
            for f in ("rot_c", "rot_s", "rot_off0", "rot_off1"):
                worst = max(worst, abs(getattr(p, f) - getattr(hp, f)))
        if aug is ALL_ON:
            assert all(r.flip_on and r.rot_on and r.scale_on and r.shift_on and r.noise_on for r in recs)
    assert ds.draw_state() == (seed, 3)
    print(f"MEASURE rot max |device - aug_param| = {worst:.3e}")
    assert worst <= ROT_BOUND, (worst, ROT_BOUND)


@pytest.mark.parametrize("aug", [REF_AUG, ALL_ON], ids=["ref_aug", "all_on"])
def test_patches_equal_oracle_teacher_forced(cuda, cases, aug):
    """The records and the noise buffer read back as AugDraws drive the oracle."""
    ds = _ds(cases, aug, seed=5)
    for _ in range(2):
        imgs, labs = ds.sample_batch(8)
        assert imgs.shape == labs.shape == (8, 1) + PATCH
        _check(ds, cases, imgs, labs)
    assert {d[0] for d in ds.last_draws} <= {0, 1}


def test_crops_bit_exact_without_augmentation(cuda, cases):
    ds = _ds(cases, None, seed=6)
    imgs, labs = ds.sample_batch(12)
    _check(ds, cases, imgs, labs, exact=True)
    recs = ds.last_records
    # both cases are drawn from; some crop clamps at 0 and some is zero-padded at the far end
    assert {r.case_idx for r in recs} == {0, 1}
    shapes = [c[0].shape for c in cases]
    assert any(c - p // 2 < 0 for r in recs for c, p in zip(r.center, PATCH))
    assert any(max(0, c - p // 2) + p > s for r in recs
               for c, p, s in zip(r.center, PATCH, shapes[r.case_idx]))


def test_mixed_patches_equal_oracle(cuda, cases):
    mx = _mixed(cases, REF_AUG, seed=8)
    imgs, labs = mx.sample_batch(8)
    imgs, labs = imgs.cpu().numpy(), labs.cpu().numpy()
    recs, draws = mx.last_records, mx.last_draws
    doms = [cases, cases[::-1]]
    for k, (r, (ci, center, d)) in enumerate(zip(recs, draws)):
        img, lab = A.extract_patch(doms[r.domain][ci][0], doms[r.domain][ci][1], center, PATCH)
        ri, rl = A.augment(img, lab, d, PATCH)
        assert np.abs(imgs[k, 0] - ri.astype(np.float32)).max() <= 1e-6, k
        assert (labs[k, 0] != rl).sum() <= 1e-4 * rl.size, k


def test_noise_matches_box_muller(cuda, cases):
    """One patch of 13,440 voxels with noise on: the values against restate_noise (relative,
    NOISE_REL_BOUND = 4 x the measured 4.306e-16: the device's and libm's log / cos differ by
    ulps) and the sample mean / std against sigma (5 standard errors)."""
    from light_unet.patches import restate_noise
    sigma = 0.01
    ds = _ds(cases, {"gaussian_noise": {"enabled": True, "prob": 1.0, "sigma": sigma}}, seed=21)
    seed, step = ds.draw_state()
    ds.sample_batch(2)
    assert all(r.noise_on for r in ds.last_records)
    got = ds._dd.noise()[1].reshape(-1)
    N = got.size
    assert N == 13440
    want = np.array(restate_noise(seed, step, 1, N, sigma))
    rel = float(np.max(np.abs(got - want) / np.abs(want)))
    print(f"MEASURE noise max relative |device - restate| = {rel:.3e}")
    assert abs(got.mean()) <= 5 * sigma / np.sqrt(N), got.mean()
    assert abs(got.std() - sigma) <= 5 * sigma / np.sqrt(2 * N), got.std()
    assert rel <= NOISE_REL_BOUND, (rel, NOISE_REL_BOUND)


def test_decision_frequencies(cuda):
    """One draw-only call with B = 4096 in the mixed form: the check of tests/test_aug_draw.py on
    the device records (which must also equal the restatement's, record for record)."""
    from light_unet.patches import DeviceMixedPatchDataset, DevicePatchDataset, restate_draws
    specs = freq_specs()
    vols = [(np.zeros((40, 64, 40), np.float32),) * 2, (np.zeros((40, 64, 40), np.float32),) * 2]
    sub = [DevicePatchDataset(vols, (4, 4, 4), sp.lesion_patch_ratio, REF_AUG,
                              locations=(sp.lesion, sp.background)) for sp in specs]
    mx = DeviceMixedPatchDataset(sub[0], sub[1], FL_RATIO, draws="device", draw_seed=FREQ_SEED)
    recs = mx.draw_records(FREQ_B)
    check_frequencies(recs, specs, FL_RATIO)
    want = restate_draws(FREQ_SEED, 0, FREQ_B, specs, FL_RATIO)
    assert [r.astuple() for r in recs] == [w.astuple() for w in want]
    c = mx.get_sample_counts()
    assert c["fl_samples"] == sum(r.domain == 0 for r in recs) and c["total_samples"] == FREQ_B


def test_stream_properties(cuda, cases):
    from light_unet.engine import stream_seed
    a, b = _ds(cases, REF_AUG, seed=9), _ds(cases, REF_AUG, seed=9)
    xa, ta = (t.clone() for t in a.sample_batch(6))
    xb, tb = (t.clone() for t in b.sample_batch(6))
    assert torch.equal(xa, xb) and torch.equal(ta, tb)            # same seed and step
    xa2, ta2 = (t.clone() for t in a.sample_batch(6))
    assert not torch.equal(xa, xa2)                               # the next step
    r1 = _ds(cases, REF_AUG, seed=9, draw_seed=stream_seed(9, 1))
    assert r1.draw_state()[0] != a.draw_state()[0]
    assert not torch.equal(r1.sample_batch(6)[0], xa)             # rank 1's seed
    state = a.draw_state()
    assert state == (9, 2)
    b.set_draw_state((9, 1))
    xb2, tb2 = b.sample_batch(6)
    assert torch.equal(xb2, xa2) and torch.equal(tb2, ta2)        # a resumed stream
    assert b.draw_state() == state
    from light_unet.patches import DevicePatchDataset
    with pytest.raises(ValueError):                               # a host-draw dataset has none
        DevicePatchDataset(cases, PATCH, 0.5, REF_AUG, seed=9).draw_state()


@pytest.mark.parametrize("mixed", [False, True], ids=["single", "mixed"])
def test_replayed_loader_equals_eager_batches(cuda, cases, mixed):
    """Two epochs of the graph-replayed loader == the eager sample_batch sequence, bit for bit,
    ragged last batch included; mixed: the domain counts equal the records' counts."""
    from light_unet.patches import DevicePatchLoader
    mk = (lambda: _mixed(cases, REF_AUG, seed=13)) if mixed else (lambda: _ds(cases, REF_AUG, seed=13))
    lo, eager = DevicePatchLoader(mk(), 8), mk()
    n = len(eager)
    sizes = [min(8, n - b0) for b0 in range(0, n, 8)]
    assert len(lo) == len(sizes) and sizes[-1] != 8 and len(sizes) >= 3
    fl = 0
    for _ in range(2):
        got = [(x.clone(), t.clone()) for x, t in lo]
        assert [g[0].shape[0] for g in got] == sizes
        for (x, t), b in zip(got, sizes):
            xe, te = eager.sample_batch(b)
            assert torch.equal(x, xe) and torch.equal(t, te)
            fl += sum(r.domain == 0 for r in eager.last_records)
    assert lo.dataset.draw_state() == eager.draw_state() == (13, 2 * len(sizes))
    if mixed:
        c, ce = lo.dataset.get_sample_counts(), eager.get_sample_counts()
        assert c == ce and c["fl_samples"] == fl and c["total_samples"] == 2 * n
        lo.dataset.reset_sample_counts()
        assert lo.dataset.get_sample_counts()["total_samples"] == 0
