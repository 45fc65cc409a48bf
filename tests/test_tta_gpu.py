"""Mirror test-time augmentation in the sliding window (utils.sliding_window_inference_3d's
`tta_flips`, l3u_window_gather_flip, l3u_window_tta_merge): the two kernels against numpy, the
map against the reference's own sliding window run on a flip-mean module (tests/golden/tta*.npz),
against the plain device path run on such a module, an equivariance property, the composition
with the body mask, the forward cache and the two consumers, and two ranks."""
import ctypes
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PATCH = (16, 16, 16)
SHAPE = (40, 36, 44)          # 4 x 4 x 5 = 80 windows at patch 16, overlap 0.5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _np_flip(a, c):
    """F_c on the last three axes."""
    ax = tuple(a.ndim - 3 + i for i in range(3) if c >> i & 1)
    return np.flip(a, ax) if ax else a


# ---- 1. the kernels against numpy -------------------------------------------------------------------

def _np_windows(img, pos, codes, patch):
    out = np.zeros((len(pos),) + tuple(patch), np.float32)
    for r, ((z, y, x), c) in enumerate(zip(pos, codes)):
        cut = img[z:z + patch[0], y:y + patch[1], x:x + patch[2]]
        win = np.zeros(patch, np.float32)
        win[:cut.shape[0], :cut.shape[1], :cut.shape[2]] = cut
        out[r] = _np_flip(win, c)
    return out


def _gather_flip(vol, shape, pos, codes, patch, cuda, offset):
    """Rows written `offset` floats past a 16-byte boundary, with guard floats around them."""
    from light_unet import _native as nat
    R, P = len(pos), patch[0] * patch[1] * patch[2]
    pos_t = torch.tensor(pos, dtype=torch.int32, device=cuda)
    buf = torch.full((R * P + 8,), 7.0, device=cuda)
    assert buf.data_ptr() % 16 == 0
    out = buf[offset:offset + R * P]
    nat.call("l3u_window_gather_flip", vol.data_ptr(), *shape, pos_t.data_ptr(),
             (ctypes.c_int * R)(*codes), R, *patch, out.data_ptr(), nat.stream())
    host = buf.cpu().numpy()
    assert (host[:offset] == 7.0).all() and (host[offset + R * P:] == 7.0).all()
    return host[offset:offset + R * P].reshape((R,) + tuple(patch))


CODES11 = [0, 1, 2, 3, 4, 5, 6, 7, 5, 3, 6]


@pytest.mark.parametrize("patch,shape,pos,offsets", [
    # the volume is smaller than the patch along D; the origin, a window that overhangs H, one that
    # starts at the last voxel of W (pw = 7: the element-wise path)
    ((5, 6, 7), (4, 9, 7),
     [(0, 0, 0), (0, 5, 0), (0, 0, 6), (3, 8, 6), (0, 3, 2), (1, 4, 0), (0, 3, 0), (2, 0, 3),
      (0, 8, 1), (3, 0, 0), (0, 5, 6)], (0, 1)),
    # pw = 8: the 16-byte path when the rows are aligned (offset 0), the element-wise one when not;
    # W = 13 and W = 12 volumes give quads of every source alignment, inside and across the edge
    ((4, 4, 8), (6, 7, 13),
     [(0, 0, 0), (0, 5, 0), (0, 0, 12), (5, 6, 12), (2, 3, 5), (1, 1, 4), (3, 0, 8), (0, 4, 1),
      (4, 2, 6), (2, 2, 7), (5, 0, 3)], (0, 1, 2)),
    ((4, 4, 8), (5, 6, 12),
     [(0, 0, 0), (0, 4, 0), (0, 0, 11), (4, 5, 11), (1, 2, 4), (1, 1, 8), (3, 0, 2), (0, 3, 1),
      (2, 2, 6), (2, 1, 4), (4, 0, 0)], (0, 3)),
])
def test_gather_flip_matches_numpy(cuda, patch, shape, pos, offsets):
    from light_unet import _native as nat
    img = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    img[0, 0, 0] = -0.0
    vol = torch.from_numpy(img).to(cuda)
    assert len(pos) == 11 and set(CODES11) == set(range(8))
    want = _np_windows(img, pos, CODES11, patch)
    for off in offsets:
        got = _gather_flip(vol, shape, pos, CODES11, patch, cuda, off)
        assert np.array_equal(_bits(got), _bits(want)), off
    # every code 0: bit for bit the plain gather
    R, P = len(pos), patch[0] * patch[1] * patch[2]
    pos_t = torch.tensor(pos, dtype=torch.int32, device=cuda)
    plain = torch.full((R * P,), 7.0, device=cuda)
    nat.call("l3u_window_gather", vol.data_ptr(), *shape, pos_t.data_ptr(), R, *patch,
             plain.data_ptr(), nat.stream())
    got = _gather_flip(vol, shape, pos, [0] * R, patch, cuda, 0)
    assert np.array_equal(_bits(got.ravel()), _bits(plain.cpu().numpy()))
    assert np.array_equal(_bits(got), _bits(_np_windows(img, pos, [0] * R, patch)))


MERGE_CODES = {1: [[0]], 2: [[0, 4], [0, 1], [3, 6]], 4: [[0, 1, 2, 3], [0, 2, 4, 6], [7, 0, 5, 2]],
               8: [list(range(8)), [7, 6, 5, 4, 3, 2, 1, 0]]}


@pytest.mark.parametrize("K", [1, 2, 4, 8])
@pytest.mark.parametrize("patch", [(5, 6, 7), (4, 4, 8), (3, 5, 12)])
def test_tta_merge_matches_numpy(cuda, K, patch):
    from light_unet import _native as nat
    G, P = 3, patch[0] * patch[1] * patch[2]
    rng = np.random.default_rng(10 * K + patch[2])
    rows = rng.random((G * K,) + patch, dtype=np.float32)
    rows[0, 0, 0, 0] = -0.0
    for codes in MERGE_CODES[K]:
        want = np.empty((G,) + patch, np.float32)
        for g in range(G):
            acc = _np_flip(rows[g * K], codes[0]).copy()
            for j in range(1, K):
                acc = acc + _np_flip(rows[g * K + j], codes[j])      # fp32 adds, in term order
            want[g] = acc * np.float32(1.0 / K)
        for src_off, dst_off in ((0, 0), (1, 0), (0, 1), (3, 2)):     # aligned and not
            src = torch.zeros(G * K * P + 4, device=cuda)
            src[src_off:src_off + G * K * P] = torch.from_numpy(rows.ravel()).to(cuda)
            buf = torch.full((G * P + 8,), 7.0, device=cuda)
            assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
            nat.call("l3u_window_tta_merge", nat.ptr(src, src_off), (ctypes.c_int * K)(*codes), K,
                     G, *patch, nat.ptr(buf, dst_off), nat.stream())
            host = buf.cpu().numpy()
            assert (host[:dst_off] == 7.0).all() and (host[dst_off + G * P:] == 7.0).all()
            got = host[dst_off:dst_off + G * P].reshape(want.shape)
            assert np.array_equal(_bits(got), _bits(want)), (codes, src_off, dst_off)
    if K == 1:      # a copy
        assert np.array_equal(_bits(want), _bits(rows))


def test_tta_kernels_reject_bad_arguments(cuda):
    """Argument checks on the host side of the exports: nothing is launched."""
    from light_unet import _native as nat
    lib = nat.load()
    vol = torch.zeros(4, 4, 4, device=cuda)
    pos = torch.zeros(2, 3, dtype=torch.int32, device=cuda)
    out = torch.full((2 * 64,), 7.0, device=cuda)

    def gather(codes, R, pd=4):
        return lib.l3u_window_gather_flip(vol.data_ptr(), 4, 4, 4, pos.data_ptr(),
                                          (ctypes.c_int * max(1, len(codes)))(*codes), R, pd, 4, 4,
                                          out.data_ptr(), nat.stream())

    def merge(codes, K, G=1):
        return lib.l3u_window_tta_merge(out.data_ptr(), (ctypes.c_int * len(codes))(*codes), K, G,
                                        4, 4, 2, vol.data_ptr(), nat.stream())
    assert gather([0, 8], 2) == 1 and gather([-1, 0], 2) == 1        # hipErrorInvalidValue
    assert gather([0, 0], 0) == 1 and gather([0, 0], 2, pd=0) == 1
    assert merge([0, 1, 2], 3) == 1 and merge([0] * 16, 16) == 1 and merge([0, 8], 2) == 1
    assert merge([0, 4], 2, G=0) == 1
    torch.cuda.synchronize()
    assert (out == 7.0).all() and not vol.any()
    assert gather([0, 7], 2) == 0 and merge([0, 4], 2) == 0
    torch.cuda.synchronize()


# ---- 2. the reference's map ---------------------------------------------------------------------------

def _golden_model(z, cuda):
    from light_unet.models.unet3d import Lightweight3DUNet
    m = Lightweight3DUNet()
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")})
    return m.to(cuda)


@pytest.fixture(scope="module")
def g48(cuda, golden):
    """The golden weights at patch 48, a forward cache and the plain device maps (computed once)."""
    from light_unet.utils import sliding_window_inference_3d as sw
    z = golden("sliding.npz")
    model = _golden_model(z, cuda)
    cache = {}
    plain = {}
    for name in ("v40_52_48", "v64_56_72"):
        plain[name] = sw(z[f"{name}/image"], model, (48, 48, 48), 0.5, cuda, True, forward_cache=cache)
        plain[name].setflags(write=False)
    return z, model, cache, plain


@pytest.mark.parametrize("case", ["v40_52_48/2", "v40_52_48/0,1", "v40_52_48/0,1,2", "v64_56_72/0,1,2"])
def test_tta_matches_reference(cuda, golden, g48, case):
    from light_unet.utils import sliding_window_inference_3d as sw
    z, model, cache, plain = g48
    idx = golden("tta.npz")
    cases = [str(c) for c in idx["cases"]]
    gz = golden(str(idx["files"][cases.index(case)]))
    name, axes = case.split("/")
    axes = tuple(int(a) for a in axes.split(","))
    ref = gz["prob"]
    stats = {}
    prob = sw(z[f"{name}/image"], model, (48, 48, 48), 0.5, cuda, True, forward_cache=cache,
              tta_flips=axes, stats=stats)
    assert prob.shape == ref.shape and prob.dtype == np.float32
    assert stats["tta"] == 2 ** len(axes)
    print(case, "max |device - reference|", float(np.abs(prob - ref).max()),
          "max |tta - plain|", float(np.abs(prob - plain[name]).max()))
    np.testing.assert_allclose(prob, ref, atol=1e-5, rtol=0)
    for thr in (0.1, 0.3, 0.5, 0.7):      # masks bit-exact away from the threshold
        far = np.abs(ref - thr) > 1e-4
        assert (~far).mean() <= 1e-3
        want = np.unpackbits(gz[f"mask_{thr}"])[:ref.size].reshape(ref.shape).astype(bool)
        assert np.array_equal((prob >= thr)[far], want[far])
    assert np.abs(prob - plain[name]).max() > 1e-2      # the flips took effect
    assert model.training


# ---- 3. device against device ---------------------------------------------------------------------

class _FlipMean(torch.nn.Module):
    """forward(x) = (F_c0(M(F_c0 x)) + F_c1(M(F_c1 x)) + ...) * float32(1 / K), in code order."""

    def __init__(self, model, codes):
        super().__init__()
        self.model, self.codes = model, list(codes)

    def forward(self, x):
        acc = None
        for c in self.codes:
            dims = [2 + a for a in range(3) if c >> a & 1]
            y = self.model(torch.flip(x, dims) if dims else x)
            y = torch.flip(y, dims) if dims else y
            acc = y if acc is None else acc + y
        return acc * (1.0 / len(self.codes)) if len(self.codes) > 1 else acc


def _seeded_model(cuda):
    from light_unet.models.unet3d import Lightweight3DUNet
    torch.manual_seed(42)
    return Lightweight3DUNet(dropout_p=0.0).to(cuda)


def _volume(shape, seed):
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(s, dtype=np.float32) for s in shape], indexing="ij")
    v = 0.3 * rng.random(shape, dtype=np.float32)
    for _ in range(3):
        c = [rng.uniform(3, s - 3) for s in shape]
        v += np.exp(-((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2) / 12.0).astype(np.float32)
    return v.astype(np.float32)


@pytest.fixture(scope="module")
def e2e(cuda):
    """The seeded patch-16 model, one volume, its plain map and its map under all eight flips
    (computed once, never changed), and a forward cache."""
    from light_unet.utils import sliding_window_inference_3d as sw
    model = _seeded_model(cuda)
    img = _volume(SHAPE, 5)
    cache = {}
    plain = sw(img, model, PATCH, 0.5, cuda, True, forward_cache=cache)
    tta = sw(img, model, PATCH, 0.5, cuda, True, forward_cache=cache, tta_flips="all")
    plain.setflags(write=False)
    tta.setflags(write=False)
    return model, img, plain, tta, cache


@pytest.mark.parametrize("patch,shape", [(PATCH, SHAPE), ((16, 24, 32), (20, 50, 40))])
def test_tta_equals_plain_path_on_a_flip_mean_module(cuda, patch, shape):
    from light_unet.utils import sliding_window_inference_3d as sw, tta_codes
    model = _seeded_model(cuda)
    img = _volume(shape, 6)
    plain = sw(img, model, patch, 0.5, cuda, True)
    # off is the plain call
    assert np.array_equal(_bits(sw(img, model, patch, 0.5, cuda, True, tta_flips=())), _bits(plain))
    # the window batching does not change the map
    cache = {}      # one capture for both 8-row forwards; the 16-row one holds its gather itself
    maps = [sw(img, model, patch, 0.5, cuda, True, window_batch=wb, tta_flips="all",
               forward_cache=None if wb == 16 else cache) for wb in (1, 3, 16)]
    assert len(cache) == 1
    assert np.array_equal(_bits(maps[0]), _bits(maps[1])) and np.array_equal(_bits(maps[0]), _bits(maps[2]))
    assert np.abs(maps[0] - plain).max() > 1e-3
    # the plain sliding window on an eagerly called module: first the identity, which tells whether
    # eager and captured forwards agree in bits here, then the flip mean
    ident = sw(img, _FlipMean(model, [0]), patch, 0.5, cuda, True)
    bitwise = np.array_equal(_bits(ident), _bits(plain))
    print(patch, "eager identity wrapper reproduces the captured plain map bitwise:", bitwise)
    for flips in ("all", (1,), (2, 0)):
        want = sw(img, _FlipMean(model, tta_codes(flips)), patch, 0.5, cuda, True, window_batch=4)
        got = maps[0] if flips == "all" else sw(img, model, patch, 0.5, cuda, True, tta_flips=flips,
                                                forward_cache=cache)
        print(patch, flips, "max |tta - wrapper|", float(np.abs(got - want).max()))
        if bitwise:
            assert np.array_equal(_bits(got), _bits(want)), flips
        else:       # the bound test_sliding_window_uniform_weights gives eager forwards
            np.testing.assert_allclose(got, want, atol=1e-6, rtol=0)
    assert model.training


# ---- 4. equivariance --------------------------------------------------------------------------------

def test_tta_makes_the_map_flip_equivariant(cuda, g48):
    """A volume whose window grid is mirror-symmetric and unpadded along D ((72, 48, 48), patch 48:
    D grid [0, 24]), uniform blend weights, tta_flips=(0,): the map of the D-reversed volume,
    reversed back, is the map.  Window w of the reversed volume is the reversed window w' of the
    mirrored grid position, so its two terms are the two terms of w' swapped and flipped; two-term
    fp32 sums commute exactly.  What can remain is the order in which a voxel's covering windows
    are added in the blend: at most 8 unit-weight adds of values below 1, divided by their count,
    i.e. under 8 * 2^-24 * 8 / 8 < 3e-7 (here at most two windows cover a voxel, and a two-term
    sum commutes too), so 1e-6 holds with room."""
    from light_unet.utils import sliding_window_inference_3d as sw
    z, model, cache, _ = g48
    vol = np.random.default_rng(12).random((72, 48, 48), dtype=np.float32) * 0.3
    rev = np.ascontiguousarray(vol[::-1])

    def run(v, flips):
        return sw(v, model, (48, 48, 48), 0.5, cuda, False, forward_cache=cache, tta_flips=flips)
    a, b = run(vol, (0,)), run(rev, (0,))[::-1]
    print("equivariance: max |map - unflipped map of the flipped volume|", float(np.abs(a - b).max()))
    np.testing.assert_allclose(a, b, atol=1e-6, rtol=0)
    # the plain model is far from equivariant: the property comes from the augmentation
    p, q = run(vol, None), run(rev, None)[::-1]
    assert np.abs(p - q).max() > 1e-2


# ---- 5. composition ---------------------------------------------------------------------------------

def _box_mask():
    m = np.zeros(SHAPE, np.float32)
    m[:24, :20, :26] = 1.0          # 12,480 of 63,360 voxels: about a fifth
    return m


def test_tta_with_a_body_mask(cuda, e2e):
    from light_unet import utils
    sw = utils.sliding_window_inference_3d
    model, img, plain, tta, cache = e2e
    mask = _box_mask()
    assert 0.15 < mask.mean() < 0.25
    ps = {}
    pm = sw(img, model, PATCH, 0.5, cuda, True, forward_cache=cache, body_mask=mask, stats=ps)
    assert np.array_equal(_bits(pm), _bits(plain * mask)) and "tta" not in ps
    for wb in (16, 5, 32):
        st = {}
        got = sw(img, model, PATCH, 0.5, cuda, True, window_batch=wb, forward_cache=cache,
                 body_mask=mask, stats=st, tta_flips="all")
        assert np.array_equal(_bits(got), _bits(tta * mask)), wb
        per_forward = max(1, min(wb, 80) // 8)          # R // K windows per forward
        assert st == {"windows": 80, "kept": ps["kept"], "tta": 8,
                      "forwards": math.ceil(ps["kept"] / per_forward)}
    assert 0 < ps["kept"] < 80
    # an all-zero mask: no forward runs and nothing is captured, even on a cold cache
    cold, st = {}, {}
    n0 = utils._CachedForward.captures
    zero = sw(img, model, PATCH, 0.5, cuda, True, forward_cache=cold, body_mask=np.zeros(SHAPE, bool),
              stats=st, tta_flips="all")
    assert st["forwards"] == 0 and st["kept"] == 0 and cold == {}
    assert utils._CachedForward.captures == n0 and not zero.any()


def test_tta_reuses_the_plain_capture(cuda, e2e):
    from light_unet import utils
    sw = utils.sliding_window_inference_3d
    model, img, plain, tta, _ = e2e
    cache = {}
    n0 = utils._CachedForward.captures
    a = sw(img, model, PATCH, 0.5, cuda, True, window_batch=16, forward_cache=cache)
    assert utils._CachedForward.captures == n0 + 1
    st = {}
    b = sw(img, model, PATCH, 0.5, cuda, True, window_batch=16, forward_cache=cache, tta_flips="all",
           stats=st)
    assert utils._CachedForward.captures == n0 + 1 and len(cache) == 1     # K divides B: same batch
    assert st == {"windows": 80, "kept": 80, "tta": 8, "forwards": 40}
    assert np.array_equal(_bits(a), _bits(plain)) and np.array_equal(_bits(b), _bits(tta))
    # the plain call after it is still the plain map
    assert np.array_equal(_bits(sw(img, model, PATCH, 0.5, cuda, True, window_batch=16,
                                   forward_cache=cache)), _bits(plain))
    # and the uncached forward (the graph that holds the flipped gather) gives the same map
    c = sw(img, model, PATCH, 0.5, cuda, True, window_batch=16, tta_flips="all", output="device")
    assert isinstance(c, torch.Tensor) and np.array_equal(_bits(c.cpu().numpy()), _bits(tta))


def test_infer_volume_with_tta(cuda, e2e):
    from light_unet import inference, lesion
    model, img, plain, tta, cache = e2e
    thr = float(np.quantile(tta, 0.8))
    spacing = (4.0, 4.0, 4.0)
    cfg = {"data": {"patch_size": list(PATCH), "bbox_expansion_voxels": 2,
                    "volume_threshold": {"inference_cc": 0.5}},
           "validation": {"default_threshold": thr}}
    want = lesion.extract_bboxes(np.array(tta), thr, 0.5, spacing, 2)
    assert len(want) > 0
    got_map, got = inference.infer_volume(img, model, cfg, spacing=spacing, forward_cache=cache,
                                          tta_flips="all")
    assert np.array_equal(_bits(got_map), _bits(tta)) and got == want
    # the default stays off
    got_map, _ = inference.infer_volume(img, model, cfg, spacing=spacing, forward_cache=cache)
    assert np.array_equal(_bits(got_map), _bits(plain))


def test_fast_validate_reads_validation_tta_flips(cuda, monkeypatch):
    import test_fast_validate_gpu as FV
    from light_unet import fast_trainer
    from light_unet.utils import sliding_window_inference_3d as sw
    model = _seeded_model(cuda)
    shape = (24, 28, 20)
    img = _volume(shape, 10)
    lab = (_volume(shape, 20) > 0.9).astype(np.float32)
    cls = type("TtaValidateTrainer", (FV.StandInTrainer,), {"validate": lambda self, e: None})
    fast_trainer.bind_validate(cls)
    calls = []
    real_sw = fast_trainer.sliding_window_inference_3d

    def spy(**kw):
        out = real_sw(**kw)
        calls.append((kw, out))
        return out
    monkeypatch.setattr(fast_trainer, "sliding_window_inference_3d", spy)
    f = lambda a: torch.from_numpy(a)[None, None]   # noqa: E731
    batches = [(f(img), f(lab), ["0000"], torch.tensor([(4.0, 4.0, 4.0)]))]
    for flips in ([2, 0], "all"):
        calls.clear()
        t = cls(cuda, model, batches, [0.3, 0.5], masks_on=False)
        t.config["validation"]["tta_flips"] = flips
        t.validate(0)
        assert len(calls) == 1 and calls[0][0]["tta_flips"] == flips
        want = sw(img, model, PATCH, 0.5, cuda, True, tta_flips=flips)
        assert np.array_equal(_bits(calls[0][1].cpu().numpy()), _bits(want))
    # the reference configs have no such key: nothing is passed
    calls.clear()
    cls(cuda, model, batches, [0.3, 0.5], masks_on=False).validate(0)
    assert len(calls) == 1 and "tta_flips" not in calls[0][0]
    assert np.array_equal(_bits(calls[0][1].cpu().numpy()), _bits(sw(img, model, PATCH, 0.5, cuda, True)))


# ---- 6. two ranks -----------------------------------------------------------------------------------

def test_tta_sharded_over_ranks(cuda, golden, tmp_path):
    """Two ranks (gloo, both on this GPU) split the two 8-row forwards of v40_52_48 under all
    three flips; the all-reduced map against the reference's."""
    idx = golden("tta.npz")
    cases = [str(c) for c in idx["cases"]]
    ref = golden(str(idx["files"][cases.index("v40_52_48/0,1,2")]))["prob"]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = tmp_path / "prob.npy"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tests", "_tta_dist_worker.py"), str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    prob = np.load(out)
    np.testing.assert_allclose(prob, ref, atol=1e-5, rtol=0)
    assert np.load(str(out) + ".forwards.npy").tolist() == [1, 1]   # one forward per rank
