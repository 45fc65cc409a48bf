"""Plain-torch fp64 restatement of the loss family on four sums (not a test module).

sums: s0 = sum p t, s1 = sum p, s2 = sum t, s3 = sum e,
  e_i = -(t max(ln p, -100) + (1 - t) max(ln(1 - p), -100))     (nn.BCELoss's clamp)
  L   = w_f (1 - TI)^gamma + w_b s3 / M + w_d (1 - (2 s0 + sd) / (s1 + s2 + sd)),
  TI  = (s0 + sf) / (s0 + alpha (s2 - s0) + beta (s1 - s0) + sf)
  dL/dp_i = cA t_i + cB (1 - t_i) + cE (p_i - t_i) / max(p_i (1 - p_i), 1e-12)
A descriptor is the tuple (w_f, alpha, beta, gamma, sf, w_b, M, w_d, sd) of include/l3u.h.
"""
import torch

# (kind, constructor kwargs) of the cases in tests/golden/losses.npz
CASES = {"comb_default": ("CombinedLoss", {}),
         "comb_half": ("CombinedLoss", dict(ftl_weight=0.5, bce_weight=0.5, alpha=0.6, beta=0.4,
                                            gamma=1.0)),
         "dice_default": ("DiceLoss", {}),
         "dice_smooth1": ("DiceLoss", dict(smooth=1.0))}


def descriptor(kind, numel, ftl_weight=0.8, bce_weight=0.2, alpha=0.7, beta=0.3, gamma=0.75,
               smooth=1e-6):
    if kind == "FocalTverskyLoss":
        return (1.0, alpha, beta, gamma, smooth, 0.0, float(numel), 0.0, 0.0)
    if kind == "CombinedLoss":
        return (ftl_weight, alpha, beta, gamma, 1e-6, bce_weight, float(numel), 0.0, 0.0)
    if kind == "DiceLoss":
        return (0.0, 0.7, 0.3, 0.75, 1e-6, 0.0, float(numel), 1.0, smooth)
    raise ValueError(kind)


def sums4(p, t):
    p, t = p.double().reshape(-1), t.double().reshape(-1)
    lp = torch.clamp(torch.log(p), min=-100.0)
    lq = torch.clamp(torch.log(1.0 - p), min=-100.0)
    e = -(t * lp + (1.0 - t) * lq)
    return torch.stack([(p * t).sum(), p.sum(), t.sum(), e.sum()])


def coefficients(s, d):
    """(loss, cA, cB, cE) from the four sums (fp64 tensor or list) and a descriptor."""
    wf, al, be, ga, sf, wb, M, wd, sd = d
    s0, s1, s2, s3 = [float(v) for v in s]
    loss = cA = cB = cE = 0.0
    if wf != 0.0:
        dn = s0 + al * (s2 - s0) + be * (s1 - s0) + sf
        om = 1.0 - (s0 + sf) / dn
        pre = -ga * om ** (ga - 1.0) / (dn * dn)
        loss += wf * om ** ga
        cA += wf * pre * (dn - (s0 + sf) * (1.0 - al))
        cB += wf * pre * (-(s0 + sf) * be)
    if wb != 0.0:
        loss += wb * s3 / M
        cE = wb / M
    if wd != 0.0:
        U = s1 + s2 + sd
        Q = (2.0 * s0 + sd) / (U * U)
        loss += wd * (1.0 - (2.0 * s0 + sd) / U)
        cA += wd * (Q - 2.0 / U)
        cB += wd * Q
    return loss, cA, cB, cE


def loss_and_grad(p, t, d, sums=None):
    """fp64 loss (float) and dL/dp (fp64 tensor, p's shape); sums: global sums if not p's own."""
    s = sums4(p, t) if sums is None else sums
    loss, cA, cB, cE = coefficients(s, d)
    pd, td = p.double(), t.double()
    g = cA * td + cB * (1.0 - td) + cE * (pd - td) / torch.clamp(pd * (1.0 - pd), min=1e-12)
    return loss, g


def loss_autograd(p, t, d):
    """The same loss as a differentiable torch expression of p (for composition with a network):
    terms with weight 0 are left out."""
    wf, al, be, ga, sf, wb, M, wd, sd = d
    pf, tf = p.reshape(-1), t.reshape(-1).to(p.dtype)
    s0, s1, s2 = (pf * tf).sum(), pf.sum(), tf.sum()
    loss = 0.0
    if wf != 0.0:
        ti = (s0 + sf) / (s0 + al * (s2 - s0) + be * (s1 - s0) + sf)
        loss = loss + wf * (1.0 - ti) ** ga
    if wb != 0.0:
        # torch's own op: the clamped logs above have a NaN autograd gradient at p = 0 or 1
        bce = torch.nn.functional.binary_cross_entropy(pf, tf, reduction="sum")
        loss = loss + wb * bce / M
    if wd != 0.0:
        loss = loss + wd * (1.0 - (2.0 * s0 + sd) / (s1 + s2 + sd))
    return loss
