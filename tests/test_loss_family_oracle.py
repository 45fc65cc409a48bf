"""The loss family on four sums (FocalTversky / CombinedLoss / DiceLoss), CPU side.

tests/golden/losses.npz holds the REFERENCE losses.py's fp64 losses and autograd gradients
(tests/golden/make_loss_goldens.py); tests/_loss_family_ref.py restates the closed form the HIP
kernels implement.  Tolerances: the restatement is fp64 against fp64, so loss 1e-9 relative and
gradient 1e-7 relative L2 (the saturated-logit group sits at 4e-9: autograd's BCE gradient divides
by the 1e-12 clamp where p is exactly 0 or 1, the same expression here).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _loss_family_ref as R  # noqa: E402

GROUPS = ("a", "b")


@pytest.mark.parametrize("grp", GROUPS)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_reproduces_reference_golden(golden, grp, name):
    z = golden("losses.npz")
    p, t = torch.from_numpy(z[f"{grp}/pred"]), torch.from_numpy(z[f"{grp}/target"])
    kind, kw = R.CASES[name]
    loss, g = R.loss_and_grad(p, t, R.descriptor(kind, p.numel(), **kw))
    l64 = float(z[f"{grp}/{name}/loss64"])
    g64 = z[f"{grp}/{name}/grad64"]
    assert abs(loss - l64) <= 1e-9 * abs(l64), (loss, l64)
    gerr = np.linalg.norm(g.numpy() - g64) / np.linalg.norm(g64)
    assert gerr <= 1e-7, gerr
    # the reference's own fp32 loss sits within fp32 rounding of it
    assert abs(float(z[f"{grp}/{name}/loss32"]) - l64) <= 1e-6 * abs(l64)


def test_saturated_group_holds_exact_zero_and_one(golden):
    z = golden("losses.npz")
    p = z["b/pred"].reshape(-1)
    assert p[:200].min() == 0.0 and p[:200].max() == 1.0
    assert set(np.unique(z["b/target"].reshape(-1)[:200])) == {0.0, 1.0}


def test_autograd_restatement_matches_closed_form(golden):
    z = golden("losses.npz")
    p, t = torch.from_numpy(z["a/pred"]), torch.from_numpy(z["a/target"])
    for kind, kw in list(R.CASES.values()) + [("FocalTverskyLoss", {})]:
        d = R.descriptor(kind, p.numel(), **kw)
        loss, g = R.loss_and_grad(p, t, d)
        pa = p.double().requires_grad_(True)
        la = R.loss_autograd(pa, t, d)
        la.backward()
        assert abs(la.item() - loss) <= 1e-12 * abs(loss)
        assert float((pa.grad - g).norm() / g.norm()) <= 1e-12


@pytest.mark.parametrize("case", ["rand", "sat", "params"])
def test_focal_tversky_member_matches_ftl_golden(golden, case):
    """(1, 0, 0) is today's FocalTversky: the reference's fp64 loss and gradient of ftl.npz."""
    z = golden("ftl.npz")
    p, t = torch.from_numpy(z[f"{case}/pred"]), torch.from_numpy(z[f"{case}/target"])
    al, be, ga = [float(v) for v in z[f"{case}/abg"]]
    d = R.descriptor("FocalTverskyLoss", p.numel(), alpha=al, beta=be, gamma=ga)
    loss, g = R.loss_and_grad(p, t, d)
    l64, g64 = float(z[f"{case}/loss"]), z[f"{case}/dpred"]
    assert abs(loss - l64) <= 1e-9 * abs(l64)
    assert np.linalg.norm(g.numpy() - g64) <= 1e-7 * np.linalg.norm(g64)


def test_loss_factory_routes_and_constructor_errors(golden):
    from light_unet.models import losses
    c = losses.get_loss_function({"use_combined_loss": True})
    assert type(c) is losses.CombinedLoss and (c.ftl_weight, c.bce_weight) == (0.8, 0.2)
    assert type(c.focal_tversky) is losses.FocalTverskyLoss and isinstance(c.bce, torch.nn.BCELoss)
    c = losses.get_loss_function({"name": "DiceLoss", "use_combined_loss": True, "alpha": 0.6,
                                  "beta": 0.4, "gamma": 1.0,
                                  "combined_loss_weights": {"focal_tversky": 0.5, "bce": 0.5}})
    assert type(c) is losses.CombinedLoss and c.ftl_weight == 0.5
    assert (c.focal_tversky.alpha, c.focal_tversky.beta, c.focal_tversky.gamma) == (0.6, 0.4, 1.0)
    d = losses.get_loss_function({"name": "DiceLoss"})
    assert type(d) is losses.DiceLoss and d.smooth == 1e-6
    assert losses.DiceLoss(smooth=1.0).smooth == 1.0
    assert type(losses.get_loss_function({})) is losses.FocalTverskyLoss
    with pytest.raises(ValueError):
        losses.get_loss_function({"name": "BCELoss"})
    z = golden("losses.npz")
    for (wf, wb), raises in zip(z["bad_weights"], z["bad_weights_raise"]):
        assert raises == 1
        with pytest.raises(AssertionError):
            losses.CombinedLoss(ftl_weight=float(wf), bce_weight=float(wb))
    with pytest.raises(AssertionError):
        losses.CombinedLoss(alpha=0.6, beta=0.3)
    for crit in (losses.CombinedLoss(), losses.DiceLoss()):
        assert crit.reduce_hook is None and crit.hook_grad_scale == 1.0


def test_family_descriptors():
    from light_unet.models import losses
    assert losses.loss_family(losses.FocalTverskyLoss(0.6, 0.4, 1.0), 10) == \
        (1.0, 0.6, 0.4, 1.0, 1e-6, 0.0, 10.0, 0.0, 0.0)
    assert losses.loss_family(losses.CombinedLoss(0.5, 0.5, 0.6, 0.4, 1.0), 7) == \
        R.descriptor("CombinedLoss", 7, **R.CASES["comb_half"][1])
    d = losses.loss_family(losses.DiceLoss(smooth=1.0), 3)
    assert (d[0], d[5], d[6], d[7], d[8]) == (0.0, 0.0, 3.0, 1.0, 1.0)

    class Other(losses.DiceLoss):
        pass
    with pytest.raises(TypeError):
        losses.loss_family(Other())


@pytest.mark.parametrize("cls", ["CombinedLoss", "DiceLoss"])
def test_cpu_and_noncontiguous_inputs_raise(cls):
    from light_unet import _native
    from light_unet.models import losses
    f = getattr(losses, cls)()
    with pytest.raises(_native.NativeError):
        f(torch.rand(1, 1, 4, 4, 4), torch.rand(1, 1, 4, 4, 4))   # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        f(torch.rand(1, 1, 4, 4, 8)[..., ::2], torch.rand(1, 1, 4, 4, 4))  # non-contiguous (view)


def test_abi_version_and_new_symbols():
    from light_unet import _native
    assert _native.query("l3u_abi_version") == _native.ABI_VERSION == 5
    lib = _native.load()
    names = ["l3u_loss4_sums", "l3u_loss4_reduce", "l3u_loss4_value", "l3u_loss4_bwd",
             "l3u_outconv_fwd_loss4", "l3u_outconv_bwd_loss4", "l3u_outconv_bwd_loss4_dz",
             "l3u_outconv_bwd_loss4p", "l3u_outconv_bwd_loss4p_dz"]
    for n in names:
        assert n in _native._SIGS and hasattr(lib, n), n
    for n in names[4:]:
        assert n in _native.BF16_TWINS and hasattr(lib, n + "_bf16"), n


def test_trainstep_loss_config_parsing():
    from light_unet.models import losses
    from light_unet.train_step import parse_loss
    assert parse_loss(None) == ((0.7, 0.3, 0.75, 1e-6), None)
    assert parse_loss({"name": "FocalTverskyLoss", "alpha": 0.6, "beta": 0.4, "gamma": 1.0}) == \
        ((0.6, 0.4, 1.0, 1e-6), None)
    assert parse_loss(losses.FocalTverskyLoss(0.6, 0.4)) == ((0.6, 0.4, 0.75, 1e-6), None)
    abgs, fam = parse_loss({"use_combined_loss": True})
    assert abgs is None and fam == R.descriptor("CombinedLoss", 1)
    _, fam = parse_loss({"use_combined_loss": True, "alpha": 0.6, "beta": 0.4, "gamma": 1.0,
                         "combined_loss_weights": {"focal_tversky": 0.5, "bce": 0.5}})
    assert fam == R.descriptor("CombinedLoss", 1, **R.CASES["comb_half"][1])
    _, fam = parse_loss({"name": "DiceLoss"})
    assert (fam[0], fam[5], fam[7], fam[8]) == (0.0, 0.0, 1.0, 1e-6)
    assert parse_loss(losses.DiceLoss(smooth=1.0))[1][8] == 1.0
    assert parse_loss(losses.CombinedLoss())[1] == R.descriptor("CombinedLoss", 1)
    with pytest.raises(ValueError):
        parse_loss({"name": "BCELoss"})
    with pytest.raises(AssertionError):
        parse_loss({"use_combined_loss": True,
                    "combined_loss_weights": {"focal_tversky": 0.8, "bce": 0.3}})


def test_trainstep_rejects_unknown_loss_name():
    """TrainStep parses the loss before it touches the model or the device."""
    from light_unet.train_step import TrainStep
    with pytest.raises(ValueError):
        TrainStep(None, {"name": "BCELoss"})
    with pytest.raises(AssertionError):
        TrainStep(None, {"use_combined_loss": True,
                         "combined_loss_weights": {"focal_tversky": 0.9, "bce": 0.2}})


def test_fast_trainer_accepts_exactly_the_family():
    from light_unet import fast_trainer
    from light_unet.models import losses

    class T:
        pass
    t = T()
    for crit in (losses.FocalTverskyLoss(), losses.CombinedLoss(), losses.DiceLoss()):
        t.criterion = crit
        assert fast_trainer._usable(t)
    t.criterion = torch.nn.BCELoss()
    assert not fast_trainer._usable(t)
    t.criterion = type("Sub", (losses.CombinedLoss,), {})()
    assert not fast_trainer._usable(t)
    t.criterion = losses.CombinedLoss()
    t.criterion.reduce_hook = lambda s: s
    assert not fast_trainer._usable(t)
