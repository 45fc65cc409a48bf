"""Mirror test-time augmentation of the sliding window, the parts that need no GPU: the flip codes,
the argument checks (made before any device call), the contract restated in numpy on the
reference-free oracle, and the golden files' own consistency."""
import numpy as np
import pytest
import torch


def test_tta_codes():
    from light_unet.utils import tta_codes
    assert tta_codes(None) == [0]
    assert tta_codes(()) == [0]
    assert tta_codes([]) == [0]
    assert tta_codes((2,)) == [0, 4]
    assert tta_codes((1, 0)) == [0, 1, 2, 3]
    assert tta_codes([0, 2]) == [0, 1, 4, 5]
    assert tta_codes("all") == list(range(8))
    assert tta_codes((0, 1, 2)) == list(range(8))
    assert tta_codes(np.array([1])) == [0, 2]


@pytest.mark.parametrize("bad", [(3,), (0, 0), "x", (-1,), (1.0,), 2, ("0",), (True,)])
def test_tta_codes_rejects(bad):
    from light_unet.utils import tta_codes
    with pytest.raises(ValueError):
        tta_codes(bad)


def test_sliding_window_checks_tta_flips_before_any_device_call():
    from light_unet._native import NativeError
    from light_unet.utils import sliding_window_inference_3d
    model = torch.nn.Conv3d(1, 1, 1)      # on the CPU: a device call would raise NativeError
    img = np.zeros((20, 24, 18), np.float32)
    for bad in ((3,), (0, 0), "x"):
        with pytest.raises(ValueError, match="tta_flips"):
            sliding_window_inference_3d(img, model, (16, 16, 16), 0.5, tta_flips=bad)
    # accepted values pass the check and reach the device requirement
    for ok in (None, (), "all", (2,), [1, 0]):
        with pytest.raises(NativeError):
            sliding_window_inference_3d(img, model, (16, 16, 16), 0.5, tta_flips=ok)


def _analytic(x):
    """A cheap 'model' that is not flip-equivariant along any axis: sigmoid of running sums."""
    x = x.astype(np.float32)
    s = np.cumsum(x, axis=-1, dtype=np.float32) + np.float32(0.5) * np.cumsum(x, axis=-2, dtype=np.float32) \
        - np.float32(0.25) * np.cumsum(x, axis=-3, dtype=np.float32)
    return (np.float32(1) / (np.float32(1) + np.exp(-s))).astype(np.float32)


def _flip(a, c):
    """F_c on the last three axes."""
    ax = tuple(a.ndim - 3 + i for i in range(3) if c >> i & 1)
    return np.flip(a, ax) if ax else a


def _flip_mean(x, codes):
    acc = None
    for c in codes:
        y = _flip(_analytic(_flip(x, c)), c)
        acc = y.copy() if acc is None else acc + y
    return acc * np.float32(1.0 / len(codes))


@pytest.mark.parametrize("flips", [(2,), (0, 1), "all"])
@pytest.mark.parametrize("gaussian", [True, False])
def test_contract_restated_on_the_oracle(flips, gaussian):
    """oracle.sliding_oracle.sliding_window driven by a flip-mean forward equals the contract
    written out window by window: zero-pad at the high end, flip the PADDED window, predict,
    flip back, add in code order from the code-0 term, times float32(1 / K), then the blend."""
    from light_unet.utils import tta_codes, window_positions
    from oracle.sliding_oracle import gaussian_importance_map, sliding_window
    codes = tta_codes(flips)
    patch, shape = (5, 6, 8), (4, 9, 13)     # smaller than the patch along D, ragged along H and W
    img = np.random.default_rng(7).random(shape, dtype=np.float32)
    got = sliding_window(img, lambda x: _flip_mean(x, codes), patch, 0.5, gaussian)

    imp = gaussian_importance_map(patch) if gaussian else np.ones(patch, np.float32)
    acc, cnt = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    grids = [window_positions(s, p, max(1, int(p * 0.5))) for s, p in zip(shape, patch)]
    for z in grids[0]:
        for y in grids[1]:
            for x in grids[2]:
                win = np.zeros(patch, np.float32)
                cut = img[z:z + patch[0], y:y + patch[1], x:x + patch[2]]
                ad, ah, aw = cut.shape
                win[:ad, :ah, :aw] = cut
                total = None
                for c in codes:
                    idx = tuple(slice(None, None, -1) if c >> a & 1 else slice(None) for a in range(3))
                    term = _analytic(win[idx][None, None])[0, 0][idx]
                    total = term.copy() if total is None else total + term
                p = total * np.float32(1.0 / len(codes))
                acc[z:z + ad, y:y + ah, x:x + aw] += p[:ad, :ah, :aw] * imp[:ad, :ah, :aw]
                cnt[z:z + ad, y:y + ah, x:x + aw] += imp[:ad, :ah, :aw]
    want = acc / cnt
    assert got.dtype == np.float32 and np.array_equal(got, want)
    # the flips matter for this forward: the plain map differs
    plain = sliding_window(img, _analytic, patch, 0.5, gaussian)
    assert np.abs(got - plain).max() > 1e-2


def test_golden_files_are_consistent(golden):
    """tta.npz lists its cases; every case file holds a map of its image's shape, inside (0, 1),
    different from the plain map, with the packed masks the map implies."""
    idx = golden("tta.npz")
    plain = golden("sliding.npz")
    cases = [str(c) for c in idx["cases"]]
    assert cases == ["v40_52_48/2", "v40_52_48/0,1", "v40_52_48/0,1,2", "v64_56_72/0,1,2"]
    for case, fname in zip(cases, idx["files"]):
        name, axes = case.split("/")
        z = golden(str(fname))
        prob = z["prob"]
        assert z["axes"].tolist() == [int(a) for a in axes.split(",")]
        assert prob.dtype == np.float32 and prob.shape == plain[f"{name}/image"].shape
        assert 0.0 < prob.min() and prob.max() < 1.0
        assert np.abs(prob - plain[f"{name}/prob"]).max() > 0.3
        for thr in idx["thresholds"]:
            m = np.unpackbits(z[f"mask_{thr}"])[:prob.size].reshape(prob.shape).astype(bool)
            assert np.array_equal(m, prob >= thr)
            # the share of voxels the parity test leaves out stays below 0.1 %
            assert (np.abs(prob - thr) <= 1e-4).mean() <= 1e-3
