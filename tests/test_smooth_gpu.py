"""Gaussian smoothing on the device (csrc/smooth.hip, light_unet/smooth.py: gaussian_filter)
against scipy's stored outputs (tests/golden/smooth.npz, made by
tests/golden/make_smooth_goldens.py) and the numpy transcription of the module's definition, and
its consumers: lesion_uptake, resegment_lesions and infer_volume with smooth_fwhm_mm.

Bounds: the definition fixes every float64 operation and its order and reproduces scipy bit for
bit (tests/test_smooth_host.py), so every comparison here is == on the bits and allows nothing.
Every native call of the filter runs inside fenced.fence().
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import fenced
import quantify_fixture as qfx

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_smooth_goldens as G   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("smooth.npz")
    return z, json.loads(bytes(z["meta"]).decode())


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _tables(z, k):
    return [z[f"w/{k}/{a}"] if f"w/{k}/{a}" in z.files else None for a in range(3)]


@pytest.mark.parametrize("s", sorted(G.SHAPES))
def test_stored_cases_equal_scipy(cuda, fx, s):
    """Through the weight tables of the fixture, so that no machine's np.exp takes part."""
    from light_unet import smooth
    z, _ = fx
    mine = [c for c in G.cases() if c[0] == s]
    assert mine
    launches = 0
    with fenced.fence() as f:
        for c in mine:
            x, want = G.case_input(z, c), z[G.name(c)]
            tables = _tables(z, c[2])
            got = smooth._filter_weights(x, tables, c[3], G.CVAL)
            assert got.dtype == want.dtype and got.shape == want.shape
            differing = int((_bits(got) != _bits(want)).sum())
            print(f"case {G.name(c)}: {differing} of {want.size} voxels differ from scipy")
            assert differing == 0, c
            launches += sum(w is not None for w in tables)      # a zero sigma: no launch
    assert f.calls == launches


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_public_call_equals_the_transcription(cuda, fx, dtype):
    """gaussian_filter by sigma against the transcription with this machine's weights."""
    from light_unet import smooth
    z, _ = fx
    x = z["in/c/g"].astype(dtype)
    with fenced.fence():
        for k, sig in enumerate(G.SIGMAS):
            for mode in G.MODES:
                got = smooth.gaussian_filter(x, sig, mode=mode, cval=G.CVAL)
                want = G.transcription(x, G.weight_tables(sig), mode, G.CVAL)
                assert got.dtype == dtype and np.array_equal(_bits(got), _bits(want)), (k, mode)
        # a scalar sigma, truncate and radius
        got = smooth.gaussian_filter(x, 0.9, truncate=2.0, mode="mirror")
        assert np.array_equal(_bits(got), _bits(G.transcription(x, [G.weights(0.9, 2)] * 3, "mirror")))
        got = smooth.gaussian_filter(x, (0.9, 0.0, 1.4), radius=(5, 1, 2), mode="nearest")
        want = G.transcription(x, [G.weights(0.9, 5), None, G.weights(1.4, 2)], "nearest")
        assert np.array_equal(_bits(got), _bits(want))
        # nothing to filter: a copy
        same = smooth.gaussian_filter(x, 0.0)
        assert same is not x and np.array_equal(_bits(same), _bits(x))


# more than one tile along every axis (64 outputs along z and y, 256 along x, 16 rows), column
# tiles with a tail (64 floats / 32 doubles), the radius cap, and a radius of many axis lengths
EXTRA = [((70, 5, 9), (2.0, 0.0, 0.0), None), ((3, 131, 5), (0.0, 1.1, 0.0), None),
         ((2, 9, 261), (0.0, 0.0, 0.8), None), ((3, 6, 300), (0.7, 0.7, 16.0), None),
         ((2, 3, 5), (1.0, 1.0, 1.0), (64, 64, 64)), ((67, 66, 70), (0.8, 0.8, 0.8), None)]


@pytest.mark.parametrize("shape,sigma,radius", EXTRA)
def test_tiles_tails_and_the_radius_cap(cuda, shape, sigma, radius):
    from light_unet import smooth
    rng = np.random.default_rng(5)
    x32 = rng.gamma(0.7, 3.0, shape).astype(np.float32)
    rad = [None] * 3 if radius is None else radius
    tables = [G.weights(s, G.radius_of(s) if r is None else r) if s > 0 else None
              for s, r in zip(sigma, rad)]
    with fenced.fence():
        for x in (x32, x32.astype(np.float64)):
            for mode in G.MODES:
                got = smooth.gaussian_filter(x, sigma, mode=mode, cval=G.CVAL, radius=radius)
                want = G.transcription(x, tables, mode, G.CVAL)
                assert np.array_equal(_bits(got), _bits(want)), (shape, mode, x.dtype)


@pytest.mark.parametrize("mode", G.MODES)
def test_small_radii_on_the_spot(cuda, mode):
    """(20, 19, 150) with radii (2, 3, 4), then skipped axes, a radius of 0 and axes shorter than
    the halo, against the transcription computed here."""
    from light_unet import smooth
    rng = np.random.default_rng(9)
    with fenced.fence() as f:
        for shape, radii in (((20, 19, 150), (2, 3, 4)), ((15, 16, 9), (None, None, 3)),
                             ((3, 30, 70), (None, 4, None)), ((30, 2, 61), (1, None, 0)),
                             ((5, 7, 9), (4, 4, 4)), ((1, 3, 70), (3, 2, 1))):
            x = rng.gamma(0.7, 3.0, shape).astype(np.float32)
            tables = [None if r is None else G.weights(max(r, 1) / 3.0, r) for r in radii]
            want = G.transcription(x, tables, mode, G.CVAL)
            dev = torch.from_numpy(x).to(cuda)
            got = smooth._filter_weights(dev, tables, mode, G.CVAL, output="device")
            assert got.data_ptr() != dev.data_ptr() and torch.equal(dev.cpu(), torch.from_numpy(x))
            assert np.array_equal(_bits(got), _bits(want)), (shape, radii)
    assert f.calls == 3 + 1 + 1 + 2 + 3 + 3


def test_input_and_output_kinds_agree_and_the_source_is_unchanged(cuda, fx):
    from light_unet import smooth
    z, _ = fx
    c = ("d", "u", 2, "nearest", "f32")
    assert c in G.cases()
    x, want = G.case_input(z, c), z[G.name(c)]
    tables = _tables(z, 2)
    dev = torch.from_numpy(np.array(x)).to(cuda)
    before = dev.clone()
    with fenced.fence():
        outs = [smooth._filter_weights(x, tables, "nearest"),
                smooth._filter_weights(dev, tables, "nearest"),
                smooth._filter_weights(x, tables, "nearest", output="device"),
                smooth._filter_weights(dev, tables, "nearest", output="device")]
        one_axis = smooth._filter_weights(dev, [None, tables[1], None], "nearest", output="device")
        perm = smooth._filter_weights(dev.permute(2, 0, 1), [tables[2], tables[0], tables[1]], "nearest")
    assert isinstance(outs[0], np.ndarray) and isinstance(outs[1], np.ndarray)
    assert outs[2].is_cuda and outs[3].is_cuda and outs[3].dtype == torch.float32
    for o in outs:
        assert np.array_equal(_bits(o), _bits(want))
    assert outs[3].data_ptr() != dev.data_ptr() and one_axis.data_ptr() != dev.data_ptr()
    assert torch.equal(dev.view(torch.int32), before.view(torch.int32))       # the source is read only
    assert np.array_equal(_bits(one_axis), _bits(G.transcription(x, [None, tables[1], None], "nearest")))
    # a permuted tensor is its contiguous copy (the axes then run in another order: other roundings)
    assert np.array_equal(_bits(perm), _bits(G.transcription(
        np.ascontiguousarray(x.transpose(2, 0, 1)), [tables[2], tables[0], tables[1]], "nearest")))
    # two runs give the same bits
    again = smooth._filter_weights(dev, tables, "nearest", output="device")
    assert again.data_ptr() != outs[3].data_ptr() and torch.equal(again.view(torch.int32),
                                                                  outs[3].view(torch.int32))


def test_bad_abi_arguments_are_rejected_before_any_launch(cuda):
    """An aliased or overlapping destination, an over-cap radius and the other argument errors
    return hipErrorInvalidValue (1) from the C entry point; the destination keeps its guard."""
    from light_unet import _native as nat
    lib = nat.load()
    n = 4 * 5 * 6
    buf = torch.full((2 * n,), 7.0, dtype=torch.float32, device=cuda)
    src, dst = buf[:n], buf[n:]
    w = torch.from_numpy(G.weights(1.0, 64)).to(cuda)
    assert w.numel() == 129 and nat.query("l3u_gauss_max_radius") == 64

    def call(src=src.data_ptr(), dst=dst.data_ptr(), dtype=0, D=4, axis=0, w=w.data_ptr(), radius=4,
             mode=0):
        return lib.l3u_gauss_axis(src, dst, dtype, D, 5, 6, axis, w, radius, mode, 0.0, nat.stream())

    assert call(dst=src.data_ptr()) == 1                           # aliased
    assert call(dst=src.data_ptr() + 4 * (n - 1)) == 1             # overlapping by one element
    assert call(src=dst.data_ptr() + 4, dst=dst.data_ptr()) == 1
    assert call(radius=65) == 1 and call(radius=-1) == 1
    assert call(src=None) == 1 and call(dst=None) == 1 and call(w=None) == 1
    assert call(dtype=2) == 1 and call(dtype=-1) == 1 and call(D=0) == 1 and call(D=-2) == 1
    assert call(axis=3) == 1 and call(axis=-1) == 1 and call(mode=4) == 1 and call(mode=-1) == 1
    torch.cuda.synchronize()
    assert (buf == 7.0).all()                                      # nothing was launched
    assert call(radius=64) == 0 and call(radius=0, axis=2, mode=3) == 0
    torch.cuda.synchronize()
    assert (src == 7.0).all()


# ------------------------------------------------------------------ the consumers
def _entry():
    """A stored uptake case with six lesions on a gamma image, at 4 mm."""
    return {e["name"]: e for e in qfx.entries()}["g_24x40x40__blobs_24x40x40__s0__m0"]


def test_lesion_uptake_filters_the_uptake_first(cuda):
    from light_unet import quantify, smooth
    e = _entry()
    up, mask = qfx.uptake(e).astype(np.float32), qfx.mask(e).astype(np.float32)
    sp = tuple(e["spacing"])
    kw = dict(spacing=sp, min_size=e["min_size"], peak_ml=e["peak_ml"])
    before = up.copy()
    got = quantify.lesion_uptake(up, mask, smooth_fwhm_mm=6.0, **kw)
    filtered = smooth.gaussian_filter(up, smooth.fwhm_sigma(6.0, sp))
    want = quantify.lesion_uptake(filtered, mask, **kw)
    assert got["smooth"] == smooth.smooth_record(6.0, sp) and got["smooth"]["radius"] == \
        [smooth.gaussian_weights(s).size // 2 for s in smooth.fwhm_sigma(6.0, sp)]
    assert "smooth" not in want and got["n_lesions"] == want["n_lesions"] > 0
    rest = dict(got)
    rest.pop("smooth")
    assert rest == want                                            # value for value
    assert np.array_equal(up, before)
    # it did filter: the maximum of a smoothed lesion is lower
    plain = quantify.lesion_uptake(up, mask, smooth_fwhm_mm=None, **kw)
    assert "smooth" not in plain and plain["suv_max"] > got["suv_max"]
    qfx.check_report(plain, e)                                     # and None is today's report
    # device tensors in, a per-axis FWHM with a skipped axis
    dev = quantify.lesion_uptake(torch.from_numpy(up).to(cuda), torch.from_numpy(mask).to(cuda),
                                 smooth_fwhm_mm=(6.0, 0.0, 5.0), **kw)
    two = quantify.lesion_uptake(smooth.smooth_fwhm(up, sp, (6.0, 0.0, 5.0)), mask, **kw)
    assert dev.pop("smooth")["radius"] == [3, 0, 2] and dev == two


@pytest.mark.parametrize("cfg", [{"method": "relative", "value": 0.41, "grow_mm": 8.0},
                                 {"method": "fixed", "value": 1.0, "grow_mm": None}])
def test_resegmentation_reads_the_filtered_uptake(cuda, cfg):
    from light_unet import quantify, resegment, smooth
    e = _entry()
    up, mask = qfx.uptake(e).astype(np.float32), qfx.mask(e).astype(np.float32)
    sp = tuple(e["spacing"])
    kw = dict(spacing=sp, min_size=e["min_size"], peak_ml=e["peak_ml"], resegment=cfg)
    filtered = smooth.gaussian_filter(up, smooth.fwhm_sigma(6.0, sp))
    got = quantify.lesion_uptake(up, mask, smooth_fwhm_mm=6.0, **kw)
    want = quantify.lesion_uptake(filtered, mask, **kw)
    assert got.pop("smooth") == smooth.smooth_record(6.0, sp)
    assert got == want and got["resegment"]["method"] == cfg["method"]
    # resegment_lesions called alone
    rkw = dict(spacing=sp, method=cfg["method"], value=cfg["value"], grow_mm=cfg["grow_mm"],
               min_size=e["min_size"])
    a = resegment.resegment_lesions(up, mask, smooth_fwhm_mm=6.0, **rkw)
    b = resegment.resegment_lesions(filtered, mask, **rkw)
    assert a.smooth == smooth.smooth_record(6.0, sp) and b.smooth is None
    assert torch.equal(a.components.labels, b.components.labels) and a.components.num == b.components.num
    assert np.array_equal(a.thresholds, b.thresholds) and np.array_equal(a.status, b.status)
    assert np.array_equal(a.reached, b.reached) and np.array_equal(a.seed_label, b.seed_label)


def test_infer_volume_passes_the_filter_through(cuda):
    """On tests/test_quantify_gpu.py's infer_volume case."""
    from light_unet import inference, lesion, quantify, smooth
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
    thr = float(np.quantile(plain[0], 0.9))
    base = inference.infer_volume(img, model, cfg, spacing=spacing, threshold=thr, forward_cache=cache,
                                  uptake=suv)
    got = inference.infer_volume(img, model, cfg, spacing=spacing, threshold=thr, forward_cache=cache,
                                 uptake=suv, smooth_fwhm_mm=6.0)
    assert len(got) == 3 and np.array_equal(_bits(got[0]), _bits(base[0])) and got[1] == base[1]
    want = quantify.lesion_uptake(smooth.smooth_fwhm(suv, spacing, 6.0), base[0], spacing=spacing,
                                  threshold=thr, min_size=lesion.min_voxels_for(0.5, spacing))
    report = dict(got[2])
    assert report.pop("smooth") == smooth.smooth_record(6.0, spacing)
    assert report == want and len(want["lesions"]) > 0 and "smooth" not in base[2]
    assert report["suv_max"] < base[2]["suv_max"]
