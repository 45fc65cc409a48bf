"""Device preprocessing (light_unet/preprocess.py -> csrc/preprocess.hip, l3u_pp_*) against the
reference's own outputs (tests/golden/preprocess.npz, made by tests/golden/make_preprocess_goldens.py
from scripts/preprocess_data.py and scipy).  Every check is exact: the work is selection, integer
counting and correctly rounded fp64 arithmetic."""
import functools
import json
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NORM = ["gauss", "pet", "const", "range", "scale", "intidx", "plant", "tiles"]
MASK_ONLY = ["tie", "faces", "w9", "w32", "w33", "w64", "w65", "d3"]
MORPH = ["faces", "w9", "w32", "w33", "w64", "w65", "d3", "tiles"]
VARIANTS = ["close0", "close2", "keepall", "dil0", "dil1", "thr01"]


@functools.lru_cache(maxsize=None)
def _load(loader):
    z = loader("preprocess.npz")
    return z, json.loads(bytes(z["meta"]).decode())


@pytest.fixture(scope="module")
def fixture(golden):
    """(the npz, its JSON part), read once for the module."""
    return _load(golden)


def unpackbits(z, key, shape):
    return np.unpackbits(z[key])[:int(np.prod(shape))].reshape(shape).astype(bool)


def same_bits(a, b):
    """Bitwise equality of two float arrays (NaN-safe, sign-of-zero strict)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


def norm_kwargs(meta, case):
    kw = dict(meta[case]["args"])
    if "target_range" in kw:
        kw["target_range"] = tuple(kw["target_range"])
    return kw


def check_mask(mask, mm, want_mask, want_mm):
    assert mask.dtype == bool and mask.shape == want_mask.shape
    assert int((mask != want_mask).sum()) == 0
    assert mm == want_mm


@pytest.mark.parametrize("case", NORM)
def test_clip_and_normalize_matches_reference(cuda, fixture, case):
    from light_unet import preprocess as PP
    z, meta = fixture
    image, want = z[f"{case}/image"], z[f"{case}/norm64"]
    norm, m = PP.clip_and_normalize(image, **norm_kwargs(meta, case))
    clip = z[f"{case}/clip"]
    got = np.array([m["clip_values"]["min"], m["clip_values"]["max"]], np.float64)
    assert type(m["clip_values"]["min"]) is float and type(m["clip_values"]["max"]) is float
    assert same_bits(got, clip), (got.tolist(), clip.tolist())
    want_m = meta[case]["metadata"]
    assert m["clip_values"] == want_m["clip_values"]
    assert m["normalization_range"] == want_m["normalization_range"]
    assert norm.dtype == np.float64
    assert same_bits(norm, want), int((norm != want).sum())
    # what the reference writes to disk: the float32 rounding, from the fused path
    cfg = {"intensity": {"clip_percentile_low": m["clip_values"]["low_percentile"],
                         "clip_percentile_high": m["clip_values"]["high_percentile"],
                         "normalization_range": m["normalization_range"]}}
    n32, none, _ = PP.preprocess_volume(image, cfg)
    assert none is None and same_bits(n32, want.astype(np.float32))


@pytest.mark.parametrize("case", NORM + MASK_ONLY)
def test_generate_body_mask_matches_reference(cuda, fixture, case):
    from light_unet import preprocess as PP
    z, meta = fixture
    shape = tuple(meta[case]["shape"])
    image = z[f"{case}/norm64"] if meta[case]["kind"] == "norm" else z[f"{case}/image"]
    mask, mm = PP.generate_body_mask(image, meta[case]["body_mask_config"])
    check_mask(mask, mm, unpackbits(z, f"{case}/mask", shape), meta[case]["body_mask"])


@pytest.mark.parametrize("variant", VARIANTS)
def test_generate_body_mask_config_variants(cuda, fixture, variant):
    from light_unet import preprocess as PP
    z, meta = fixture
    v = meta["pet"]["variants"][variant]
    mask, mm = PP.generate_body_mask(z["pet/norm64"], v["config"])
    check_mask(mask, mm, unpackbits(z, f"pet/variant/{variant}", tuple(meta["pet"]["shape"])),
               v["body_mask"])


@pytest.mark.parametrize("case", MORPH)
def test_morphology_matches_scipy_intermediates(cuda, fixture, case):
    """l3u_pp_morph alone: 1..5 iterations in one launch, dilation and erosion (outside = 0)."""
    from light_unet import preprocess as PP
    z, meta = fixture
    shape = tuple(meta[case]["shape"])
    m0 = unpackbits(z, "tiles/morph_input", shape) if case == "tiles" else z[f"{case}/image"] > 0.5
    src = torch.from_numpy(m0.astype(np.uint8)).to(cuda)
    bits = PP.pack(src)
    assert np.array_equal(PP.unpack(bits, shape, torch.bool).cpu().numpy(), m0)
    assert np.array_equal(PP.unpack(bits, shape, torch.float32).cpu().numpy(), m0.astype(np.float32))
    n, lo, hi = PP.mask_stats(bits, shape)
    co = np.argwhere(m0)
    assert n == int(m0.sum()) and lo == co.min(axis=0).tolist() and hi == co.max(axis=0).tolist()
    cap = PP.max_morph_iterations(shape[2])
    assert cap >= 5
    for i in range(1, 6):
        for name, erode in (("dil", False), ("ero", True)):
            got = PP.unpack(PP.morph(bits, shape, i, erode=erode), shape, torch.bool).cpu().numpy()
            want = unpackbits(z, f"{case}/{name}{i}", shape)
            assert int((got != want).sum()) == 0, (name, i)
    # more iterations than one launch takes are chained: the same as two shorter calls
    assert torch.equal(PP.morph(PP.morph(bits, shape, 2), shape, 3), PP.morph(bits, shape, 5))
    assert torch.equal(PP.morph(PP.morph(bits, shape, cap), shape, 2), PP.morph(bits, shape, cap + 2))
    # padding bits stay zero
    w = shape[2] % 64
    if w:
        tail = PP.morph(bits, shape, 5)[..., -1].cpu().numpy().view(np.uint64)
        assert int((tail >> np.uint64(w)).max()) == 0


def test_pack_sources_and_label_compare(cuda):
    from light_unet import preprocess as PP
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 4, size=(5, 6, 70)).astype(np.int32)
    t = torch.from_numpy(lab).to(cuda)
    for k in (0, 2, 3):
        got = PP.unpack(PP.pack(t, "eq", k), lab.shape, torch.bool).cpu().numpy()
        assert np.array_equal(got, lab == k)
    f = torch.from_numpy((lab == 1).astype(np.float32)).to(cuda)
    assert np.array_equal(PP.unpack(PP.pack(f), lab.shape).cpu().numpy(), (lab == 1).astype(np.uint8))
    n, lo, hi = PP.mask_stats(PP.pack(torch.zeros((3, 4, 5), dtype=torch.uint8, device=cuda)), (3, 4, 5))
    assert (n, lo, hi) == (0, None, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_order_statistics_are_exact(cuda, dtype):
    """Heavy ties (more than half exact zeros), negatives, infinities and denormals."""
    from light_unet import preprocess as PP
    rng = np.random.default_rng(11)
    a = rng.normal(size=70001).astype(dtype)
    a[rng.random(a.size) < 0.55] = 0.0
    a[:6] = [np.inf, -np.inf, np.finfo(dtype).tiny / 4, -np.finfo(dtype).tiny / 4,
             np.finfo(dtype).max, 1.0]
    s = np.sort(a)
    t = torch.from_numpy(a).to(cuda)
    for ranks in ([0, a.size - 1, a.size // 2, 350], [1, 2], [35000], [69999, 69998, 3, 0]):
        got = PP.order_statistics(t, ranks)
        assert [float(s[r]) for r in ranks] == got, ranks


@pytest.mark.parametrize("case", ["pet", "gauss", "const"])
@pytest.mark.parametrize("output", ["numpy", "device"])
def test_preprocess_volume_equals_the_two_calls(cuda, fixture, case, output):
    from light_unet import preprocess as PP
    z, meta = fixture
    image = z[f"{case}/image"]
    bm = dict(meta[case]["body_mask_config"], enabled=True)
    cfg = {"intensity": {"clip_percentile_low": 0.5, "clip_percentile_high": 99.5,
                         "normalization_range": [0, 1]},
           "body_mask": bm, "volume_threshold": {"train_cc": 0.5, "inference_cc": 0.1}}
    src = torch.from_numpy(image).to(cuda) if output == "device" else image
    n32, mask, m = PP.preprocess_volume(src, cfg, spacing=[4.0, 4.0, 4.0], output=output)
    norm, nm = PP.clip_and_normalize(src, 0.5, 99.5, [0, 1], output=output)
    mask2, mm = PP.generate_body_mask(norm, bm, output=output)
    if output == "device":
        assert n32.is_cuda and n32.dtype == torch.float32 and mask.is_cuda and mask.dtype == torch.bool
        assert norm.is_cuda and norm.dtype == torch.float64
        n32, mask, norm, mask2 = (t.cpu().numpy() for t in (n32, mask, norm, mask2))
    shape = tuple(meta[case]["shape"])
    assert same_bits(n32, z[f"{case}/norm64"].astype(np.float32))
    assert same_bits(n32, norm.astype(np.float32))
    assert np.array_equal(mask, mask2) and np.array_equal(mask, unpackbits(z, f"{case}/mask", shape))
    assert m["clip_values"] == nm["clip_values"] == meta[case]["metadata"]["clip_values"]
    assert m["normalization_range"] == nm["normalization_range"]
    assert m["body_mask"] == mm == meta[case]["body_mask"]
    assert m["voxel_thresholds"] == PP.calculate_voxel_thresholds([4.0, 4.0, 4.0], [0.5, 0.1])
    off = dict(cfg, body_mask={"enabled": False})
    _, none, m0 = PP.preprocess_volume(src, off, output=output)
    assert none is None and "body_mask" not in m0 and "voxel_thresholds" not in m0


def test_nan_input_raises(cuda, fixture):
    from light_unet import preprocess as PP
    z, _ = fixture
    for key in ("pet/image", "gauss/image"):
        a = z[key].copy()
        a[3, 4, 5] = np.nan
        with pytest.raises(ValueError):
            PP.clip_and_normalize(a)
        with pytest.raises(ValueError):
            PP.preprocess_volume(a, {"intensity": {"clip_percentile_low": 0.5,
                                                   "clip_percentile_high": 99.5,
                                                   "normalization_range": [0, 1]}})


def test_two_runs_are_bitwise_identical(cuda, fixture):
    from light_unet import preprocess as PP
    z, meta = fixture
    cfg = {"intensity": {"clip_percentile_low": 0.5, "clip_percentile_high": 99.5,
                         "normalization_range": [0, 1]},
           "body_mask": dict(meta["tiles"]["body_mask_config"], enabled=True)}
    runs = [PP.preprocess_volume(z["tiles/image"], cfg) for _ in range(2)]
    assert same_bits(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2]


def test_bind_preprocess_calls_through(cuda, fixture):
    import l3u_plugin
    z, meta = fixture
    mod = types.ModuleType("preprocess_data")
    mod.clip_and_normalize = mod.generate_body_mask = mod.calculate_voxel_thresholds = None
    mod.untouched = object()
    keep = mod.untouched
    names = l3u_plugin.bind_preprocess(mod)
    assert sorted(names) == ["calculate_voxel_thresholds", "clip_and_normalize", "generate_body_mask"]
    assert mod.untouched is keep
    norm, m = mod.clip_and_normalize(z["range/image"], low_percentile=1.0, high_percentile=99.0,
                                     target_range=(-1, 1))
    assert same_bits(norm, z["range/norm64"]) and m == meta["range"]["metadata"]
    mask, mm = mod.generate_body_mask(norm, meta["range"]["body_mask_config"])
    check_mask(mask, mm, unpackbits(z, "range/mask", tuple(meta["range"]["shape"])),
               meta["range"]["body_mask"])
