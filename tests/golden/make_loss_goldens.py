"""Generate tests/golden/losses.npz from the REFERENCE light_unet/models/losses.py.

Run where the reference checkout exists:  python tests/golden/make_loss_goldens.py
It imports the reference's losses.py BY FILE PATH (as make_goldens.py does) and writes inputs and
expected outputs as .npz DATA only (no reference source is copied).  Nothing under tests/ or on the
GPU box imports the reference; only this generator does.

Cases: CombinedLoss() (0.8 / 0.2), CombinedLoss(0.5, 0.5, 0.6, 0.4, 1.0), DiceLoss(),
DiceLoss(smooth=1.0), each on two input groups:
  a  pred = sigmoid(random logits), ~5 % Bernoulli targets, [2, 1, 12, 12, 12] fp32;
  b  the same, but the first 200 logits run from -120 to 120 (fp32 sigmoid gives exact 0.0 and 1.0
     there) with alternating targets.
Recorded per case: the fp32 loss, the fp64 loss and the fp64 autograd gradient w.r.t. pred (the
fp64 run is on the fp32 pred widened exactly).  Also the reference's constructor error cases.
"""
import importlib.util
import os

import numpy as np
import torch

REF = os.environ.get("L3U_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {"comb_default": ("CombinedLoss", {}),
         "comb_half": ("CombinedLoss", dict(ftl_weight=0.5, bce_weight=0.5, alpha=0.6, beta=0.4,
                                            gamma=1.0)),
         "dice_default": ("DiceLoss", {}),
         "dice_smooth1": ("DiceLoss", dict(smooth=1.0))}
# constructor arguments the reference rejects (weights not summing to 1)
BAD_WEIGHTS = [(0.8, 0.3), (0.5, 0.4), (1.0, 0.1)]


def load_ref():
    spec = importlib.util.spec_from_file_location(
        "ref_losses", os.path.join(REF, "light_unet/models/losses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs():
    shape = (2, 1, 12, 12, 12)
    g = torch.Generator().manual_seed(1234)
    za = torch.randn(shape, generator=g) * 3.0
    ta = (torch.rand(shape, generator=g) < 0.05).float()
    zb = torch.randn(shape, generator=g) * 3.0
    tb = (torch.rand(shape, generator=g) < 0.05).float()
    zb.view(-1)[:200] = torch.linspace(-120.0, 120.0, 200)
    tb.view(-1)[:200] = (torch.arange(200) % 2).float()
    pa, pb = torch.sigmoid(za), torch.sigmoid(zb)
    assert float(pb.min()) == 0.0 and float(pb.max()) == 1.0
    return {"a": (pa, ta), "b": (pb, tb)}


def main():
    R = load_ref()
    out = {}
    for grp, (p, t) in inputs().items():
        out[f"{grp}/pred"] = p.numpy()
        out[f"{grp}/target"] = t.numpy()
        for name, (cls, kw) in CASES.items():
            crit = getattr(R, cls)(**kw)
            with torch.no_grad():
                out[f"{grp}/{name}/loss32"] = np.float32(crit(p, t).item())
            p64 = p.double().requires_grad_(True)
            loss = crit(p64, t.double())
            loss.backward()
            out[f"{grp}/{name}/loss64"] = np.float64(loss.item())
            out[f"{grp}/{name}/grad64"] = p64.grad.numpy()
    bad = []
    for wf, wb in BAD_WEIGHTS:
        try:
            R.CombinedLoss(ftl_weight=wf, bce_weight=wb)
            bad.append(0)
        except AssertionError:
            bad.append(1)
    out["bad_weights"] = np.array(BAD_WEIGHTS, dtype=np.float64)
    out["bad_weights_raise"] = np.array(bad, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "losses.npz"), **out)
    print("wrote losses.npz:", {k: np.shape(v) for k, v in out.items() if k.endswith("loss64")})


if __name__ == "__main__":
    main()
