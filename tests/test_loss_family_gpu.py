"""The loss family on four sums (FocalTversky / CombinedLoss / DiceLoss) on the GPU: the
stand-alone loss kernels, the out_conv launches with the fourth partial column and the BCE
gradient term, the fused TrainStep (eager, hipGraph replay, two ranks) and the fast trainer loop.

References: tests/golden/losses.npz (the REFERENCE losses.py in fp64) and the fp64 restatement
tests/_loss_family_ref.py (checked against those goldens on the CPU by test_loss_family_oracle).

Tolerances:
  * stand-alone kernels: loss 1e-6 relative; dL/dp 1e-5 of the tensor max (the op-test rule of
    tests/test_ops_gpu.py `close`), also on the unsaturated voxels alone (the saturated ones carry
    the 1e12 of torch's 1e-12 clamp and would hide everything else);
  * out_conv launches: p 1e-6 (times the logit scale in the saturating case: the fp32 logit's
    rounding error grows with its size and |dp| <= |dz| / 4); then everything downstream is teacher-forced on the kernel's own p
    (read back), so a 1-ulp sigmoid difference at p ~ 1 cannot turn into a 100-vs-16.6 BCE term:
    sums 1e-5 relative each (fp32 block sums of <= 1024 terms, then fp64), loss 1e-5 relative,
    dz 1e-5 of the tensor max, dh / weight / bias partials 1e-4 as test_outconv_ftl_fused;
  * TrainStep against the fp64 oracle: the bounds of tests/test_model_gpu.py unchanged (output
    1e-3, loss 1e-4 relative, gradient rule with e32 from the fp32 CPU oracle);
  * bit-equality wherever the design promises it (columns 0-2, partial-reducing backward, _dz
    forms, eager == replay, FocalTversky config == the old construction, run-to-run).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _loss_family_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def nat():
    from light_unet import _native
    return _native


def st():
    return torch.cuda.current_stream().cuda_stream


def close(a, b, rtol=1e-5, what=""):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    scale = max(b.abs().max().item(), 1e-30)
    err = (a - b).abs().max().item() / scale
    print(f"{what}: max err {err:.3e} (rel to {scale:.3e})")
    assert err <= rtol, f"{what}: max err {err:.3e} (rel to {scale:.3e}) > {rtol}"


def rel_each(a, b, rtol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = ((a - b).abs() / b.abs().clamp_min(1e-300)).max().item()
    print(f"{what}: max rel err {err:.3e}")
    assert err <= rtol, f"{what}: {a.tolist()} vs {b.tolist()} ({err:.3e} > {rtol})"


# ------------------------------------------------------------------ stand-alone kernels
def _standalone(cuda, p, t, d, gscale=None, through_sigmoid=0):
    n = p.numel()
    nb = nat().query("l3u_ftl_nblocks", n)
    part = torch.full((nb * 4,), float("nan"), device=cuda)
    sums = torch.empty(4, dtype=torch.float64, device=cuda)
    loss = torch.full((), float("nan"), device=cuda)
    g = torch.full_like(p, float("nan"))
    nat().call("l3u_loss4_sums", p.data_ptr(), t.data_ptr(), n, part.data_ptr(), sums.data_ptr(), st())
    nat().call("l3u_loss4_value", sums.data_ptr(), *d, loss.data_ptr(), st())
    nat().call("l3u_loss4_bwd", p.data_ptr(), t.data_ptr(), n, sums.data_ptr(), *d,
               gscale.data_ptr() if gscale is not None else None, through_sigmoid, g.data_ptr(), st())
    torch.cuda.synchronize()
    return sums, loss, g, part


@pytest.mark.parametrize("grp", ["a", "b"])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_standalone_kernels_match_reference_golden(cuda, golden, grp, name):
    z = golden("losses.npz")
    p = torch.from_numpy(z[f"{grp}/pred"]).to(cuda)
    t = torch.from_numpy(z[f"{grp}/target"]).to(cuda)
    kind, kw = R.CASES[name]
    d = R.descriptor(kind, p.numel(), **kw)
    sums, loss, g, part = _standalone(cuda, p, t, d)
    l64 = float(z[f"{grp}/{name}/loss64"])
    g64 = torch.from_numpy(z[f"{grp}/{name}/grad64"])
    print(f"loss {loss.item()!r} vs {l64!r}: rel {abs(loss.item() - l64) / abs(l64):.3e}")
    assert abs(loss.item() - l64) <= 1e-6 * abs(l64)
    close(g, g64, 1e-5, f"dL/dp {grp}/{name}")
    pc = p.cpu()
    mid = (pc > 0) & (pc < 1)
    close(g.cpu()[mid], g64[mid], 1e-5, f"dL/dp unsaturated {grp}/{name}")
    # through the sigmoid, with a gradient scale
    gs = torch.tensor([0.5], device=cuda)
    _, _, gz, _ = _standalone(cuda, p, t, d, gscale=gs, through_sigmoid=1)
    pd = pc.double()
    close(gz, 0.5 * g64 * pd * (1 - pd), 1e-5, f"dL/dz {grp}/{name}")
    _, _, gp, _ = _standalone(cuda, p, t, d, gscale=gs)
    close(gp, 0.5 * g64, 1e-5, f"gscale dL/dp {grp}/{name}")
    # bitwise reproducible
    sums2, loss2, g2, part2 = _standalone(cuda, p, t, d)
    assert torch.equal(sums, sums2) and torch.equal(loss, loss2) and torch.equal(part, part2)
    assert torch.equal(g.view(torch.int32), g2.view(torch.int32))
    # columns 0-2 are the FocalTversky stand-alone sums, bit for bit
    n = p.numel()
    part3 = torch.empty(nat().query("l3u_ftl_nblocks", n) * 3, device=cuda)
    sums3 = torch.empty(3, dtype=torch.float64, device=cuda)
    nat().call("l3u_ftl_sums", p.data_ptr(), t.data_ptr(), n, part3.data_ptr(), sums3.data_ptr(), st())
    torch.cuda.synchronize()
    assert torch.equal(sums[:3], sums3)
    rel_each(sums, R.sums4(pc, t.cpu()), 1e-6, "sums")


def test_focal_tversky_member_equals_ftl_kernels(cuda, golden):
    """(1, 0, 0) through the family kernels against l3u_ftl_loss / l3u_ftl_bwd."""
    z = golden("losses.npz")
    p = torch.from_numpy(z["a/pred"]).to(cuda)
    t = torch.from_numpy(z["a/target"]).to(cuda)
    d = R.descriptor("FocalTverskyLoss", p.numel(), alpha=0.6, beta=0.4, gamma=1.5)
    sums, loss, g, _ = _standalone(cuda, p, t, d)
    loss_f = torch.empty((), device=cuda)
    g_f = torch.empty_like(p)
    nat().call("l3u_ftl_loss", sums.data_ptr(), 0.6, 0.4, 1.5, 1e-6, loss_f.data_ptr(), st())
    nat().call("l3u_ftl_bwd", p.data_ptr(), t.data_ptr(), p.numel(), sums.data_ptr(), 0.6, 0.4, 1.5,
               1e-6, None, 0, g_f.data_ptr(), st())
    torch.cuda.synchronize()
    assert torch.equal(loss, loss_f) and torch.equal(g, g_f)


@pytest.mark.parametrize("cls,kw", [("CombinedLoss", {}), ("DiceLoss", {"smooth": 1.0})])
def test_dropin_modules_forward_backward_and_graph(cuda, golden, cls, kw):
    """The nn.Module forms: value and autograd gradient against the golden, reduce_hook contract,
    and capture into a hipGraph (no host synchronisation inside)."""
    from light_unet.models import losses
    z = golden("losses.npz")
    name = "comb_default" if cls == "CombinedLoss" else "dice_smooth1"
    p = torch.from_numpy(z["b/pred"]).to(cuda).requires_grad_(True)
    t = torch.from_numpy(z["b/target"]).to(cuda)
    crit = getattr(losses, cls)(**kw)
    loss = crit(p, t)
    loss.backward()
    l64 = float(z[f"b/{name}/loss64"])
    assert abs(loss.item() - l64) <= 1e-6 * abs(l64)
    close(p.grad, torch.from_numpy(z[f"b/{name}/grad64"]), 1e-5, "module dL/dp")
    # reduce_hook: two identical "ranks" (sums doubled, hook_world 2) give the same loss and, with
    # hook_grad_scale 2 for an averaging reduction, the same gradient
    seen = []

    def hook(s):
        seen.append(s.numel())
        s.mul_(2.0)
    hooked = getattr(losses, cls)(**kw)
    hooked.reduce_hook, hooked.hook_world, hooked.hook_grad_scale = hook, 2, 2.0
    p2 = p.detach().clone().requires_grad_(True)
    loss2 = hooked(p2, t)
    loss2.backward()
    assert seen == [4]
    ref2, gref2 = R.loss_and_grad(p2.detach().cpu(), t.cpu(),
                                  R.descriptor(cls, 2 * p.numel(), **kw),
                                  sums=2.0 * R.sums4(p2.detach().cpu(), t.cpu()))
    assert abs(loss2.item() - ref2) <= 1e-6 * abs(ref2)
    close(p2.grad, 2.0 * gref2, 1e-5, "hooked dL/dp")
    # graph capture of forward + backward
    ps = p.detach().clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        crit(ps, t).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ps.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lg = crit(ps, t)
        lg.backward()
    gbuf = ps.grad
    gbuf.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(lg.detach(), loss.detach()) and torch.equal(gbuf, p.grad)


# ------------------------------------------------------------------ out_conv launches
COMB = ("CombinedLoss", dict(ftl_weight=0.5, bce_weight=0.5, alpha=0.6, beta=0.4, gamma=1.0))
COMB_D = ("CombinedLoss", {})
DICE = ("DiceLoss", dict(smooth=1.0))
# (C, S, target offset in floats, logit scale, loss, bf16 storage)
OUTCONV = [
    (16, 252, 0, 1.0, COMB, False),      # one block, float4 path
    (32, 252, 0, 1.0, DICE, False),
    (16, 315, 0, 1.0, COMB_D, False),    # S % 4 != 0: scalar path
    (32, 315, 0, 1.0, COMB, False),
    (16, 1728, 0, 1.0, DICE, False),     # two blocks, ragged second
    (32, 1728, 0, 1.0, COMB_D, False),
    (16, 252, 1, 1.0, COMB, False),      # target one float into its storage: must go scalar
    (32, 1728, 0, 40.0, COMB_D, False),  # saturating logits: p holds exact 0.0 and 1.0
    (16, 1728, 0, 1.0, COMB, True),      # the _bf16 twins
]


@pytest.mark.parametrize("C,S,toff,scale,loss,bf16", OUTCONV)
def test_outconv_loss4(cuda, C, S, toff, scale, loss, bf16):
    N = 2
    kind, kw = loss
    sfx = "_bf16" if bf16 else ""
    gen = torch.Generator().manual_seed(12 + C + S)
    hcat = torch.randn(N, 2 * C, S, generator=gen)       # a concat buffer: h is its first half
    if bf16:
        hcat = hcat.bfloat16().float()
    w = torch.randn(1, C, generator=gen) * 0.3 * scale
    b = torch.randn(1, generator=gen) * scale
    t = (torch.rand(N, 1, S, generator=gen) > 0.8).float()
    hd = hcat.to(cuda).bfloat16() if bf16 else hcat.to(cuda)
    hns = 2 * C * S
    wd, bd = w.to(cuda), b.to(cuda)
    td = torch.empty(N * S + 4, device=cuda)[toff:toff + N * S].view(N, 1, S)
    td.copy_(t)
    assert td.data_ptr() % 16 == 4 * toff
    nb = nat().query("l3u_outconv_nblocks", S)
    assert nb == (2 if S > 1024 else 1)
    P = N * nb
    d = R.descriptor(kind, N * S, **kw)

    def fwd(name, ncol):
        part = torch.full((P * ncol,), float("nan"), device=cuda)
        p = torch.full((N, 1, S), float("nan"), device=cuda)
        nat().call(name + sfx, hd.data_ptr(), hns, wd.data_ptr(), bd.data_ptr(), p.data_ptr(),
                   td.data_ptr(), part.data_ptr(), N, C, S, st())
        return p, part

    p, part4 = fwd("l3u_outconv_fwd_loss4", 4)
    p3, part3 = fwd("l3u_outconv_fwd", 3)
    sums = torch.empty(4, dtype=torch.float64, device=cuda)
    sums3 = torch.empty(3, dtype=torch.float64, device=cuda)
    nat().call("l3u_loss4_reduce", part4.data_ptr(), P, sums.data_ptr(), st())
    nat().call("l3u_ftl_reduce", part3.data_ptr(), P, sums3.data_ptr(), st())

    def bwd(partial_reducing, dz_only):
        name = "l3u_outconv_bwd_loss4" + ("p" if partial_reducing else "") + \
            ("_dz" if dz_only else "") + sfx
        Cd = 1 if dz_only else C
        dh = torch.full((N, Cd, S), float("nan"), device=cuda)
        part = torch.full((P * (C + 1),), float("nan"), dtype=torch.float64, device=cuda)
        lo = torch.full((), float("nan"), device=cuda)
        src = (part4.data_ptr(), P) if partial_reducing else (sums.data_ptr(),)
        nat().call(name, p.data_ptr(), td.data_ptr(), *src, *d, None, hd.data_ptr(), hns,
                   wd.data_ptr(), dh.data_ptr(), Cd * S, part.data_ptr(), lo.data_ptr(), N, C, S, st())
        return dh, part, lo

    dh, part, lo = bwd(False, False)
    dh_p, part_p, lo_p = bwd(True, False)
    dz, part_z, lo_z = bwd(False, True)
    dz_p, part_zp, lo_zp = bwd(True, True)
    torch.cuda.synchronize()
    # ---- bit-equalities
    assert torch.equal(p, p3)
    assert torch.equal(part4.view(P, 4)[:, :3], part3.view(P, 3))
    assert torch.equal(sums[:3], sums3)
    for a, bb in ((dh_p, dh), (part_p, part), (lo_p, lo), (dz_p, dz), (part_zp, part_z),
                  (lo_zp, lo_z), (part_z, part), (lo_z, lo)):
        assert torch.equal(a, bb)
    assert torch.equal(dh, wd.view(1, C, 1) * dz)
    # ---- fp64, teacher-forced on the kernel's own p
    h64 = hcat[:, :C].double()
    p_ref = torch.sigmoid(torch.einsum("oc,ncs->nos", w.double(), h64) + b.double()[None, :, None])
    # |dp| <= |dz| / 4 and the fp32 logit's rounding error grows with its size: the bound of
    # test_outconv at unit scale, times the logit scale of the saturating case
    close(p, p_ref, 1e-6 * scale, "p")
    pk = p.cpu()
    if scale > 1.0:
        assert float(pk.min()) == 0.0 and float(pk.max()) == 1.0
    rel_each(sums, R.sums4(pk, t), 1e-5, "sums")
    loss_ref, g = R.loss_and_grad(pk, t, d)
    print(f"loss {lo.item()!r} vs {loss_ref!r}")
    assert abs(lo.item() - loss_ref) <= 1e-5 * abs(loss_ref)
    dz_ref = g * pk.double() * (1 - pk.double())
    close(dz, dz_ref, 1e-5, "dz")
    close(dh, w.double().view(1, C, 1) * dz_ref, 1e-4, "dh")
    ps = part.view(P, C + 1).sum(0).cpu()
    close(ps[:C], torch.einsum("nos,ncs->c", dz_ref, h64), 1e-4, "dw")
    close(ps[C:], dz_ref.sum().view(1), 1e-4, "db")


# ------------------------------------------------------------------ TrainStep
LOSS_CFGS = {
    "ftl": ({"name": "FocalTverskyLoss", "alpha": 0.7, "beta": 0.3, "gamma": 0.75},
            ("FocalTverskyLoss", {})),
    "combined": ({"name": "FocalTverskyLoss", "alpha": 0.7, "beta": 0.3, "gamma": 0.75,
                  "use_combined_loss": True,
                  "combined_loss_weights": {"focal_tversky": 0.8, "bce": 0.2}}, COMB_D),
    "dice": ({"name": "DiceLoss"}, ("DiceLoss", {})),
}
SHAPE = (2, 1, 16, 16, 16)


def _seed42_state():
    from light_unet.models.unet3d import Lightweight3DUNet
    torch.manual_seed(42)
    return {k: v.clone() for k, v in Lightweight3DUNet(dropout_p=0.0).state_dict().items()}


def _fresh(sd, cuda, dropout_p=0.0):
    from light_unet.models.unet3d import Lightweight3DUNet
    m = Lightweight3DUNet(dropout_p=dropout_p)
    m.load_state_dict(sd)
    return m.to(cuda).train()


def _inputs(cuda):
    rng = np.random.default_rng(5)
    x = rng.random(SHAPE, dtype=np.float32)
    t = (rng.random(SHAPE) > 0.95).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(t)


@pytest.fixture(scope="module")
def oracle_runs():
    """fp64 and fp32 CPU oracle forward composed with the restated loss, once per loss."""
    from oracle import unet_oracle as U
    sd = _seed42_state()
    x, t = _inputs(None)
    out = {}
    for key, (_, (kind, kw)) in LOSS_CFGS.items():
        d = R.descriptor(kind, x.numel(), **kw)
        res = []
        for dt in (torch.float64, torch.float32):
            params = {k: v.clone().to(dt).requires_grad_(True) for k, v in sd.items()}
            o = U.unet_forward(params, x.to(dt))
            loss = R.loss_autograd(o, t.to(dt), d)
            loss.backward()
            res.append((o.detach(), float(loss.detach()), {k: q.grad.numpy() for k, q in params.items()}))
        out[key] = res
    return sd, out


def _grad_errs(grads, ref):
    """per-tensor relative L2 errors and the global one (tests/test_model_gpu.py)"""
    errs, num, den = {}, 0.0, 0.0
    for k, g in grads.items():
        gr = ref[k].astype(np.float64)
        dd = np.linalg.norm(g.astype(np.float64) - gr)
        errs[k] = dd / max(np.linalg.norm(gr), 1e-30)
        num += dd * dd
        den += float(np.sum(gr * gr))
    return errs, (num / den) ** 0.5


@pytest.mark.parametrize("key", sorted(LOSS_CFGS))
def test_trainstep_matches_fp64_oracle(cuda, oracle_runs, key):
    from light_unet.train_step import TrainStep
    sd, runs = oracle_runs
    (o64, l64, g64), (_, _, g32) = runs[key]
    x, t = (v.to(cuda) for v in _inputs(cuda))
    m = _fresh(sd, cuda)
    ts = TrainStep(m, LOSS_CFGS[key][0])
    assert (ts.family is None) == (key == "ftl")
    p, sv, sums = ts._fwd(x, t)
    ts._bwd(p, sv, t, sums)
    torch.cuda.synchronize()
    grads = {k: ts.gflat[off:off + n].view(shape).cpu().numpy()
             for k, (off, n, shape) in m.param_slices().items()}
    oerr = np.abs(p.cpu().numpy() - o64.numpy()).max()
    errs, gerr = _grad_errs(grads, g64)
    e32, ge32 = _grad_errs(g32, g64)
    print(f"{key}: out err {oerr:.2e}, loss {ts.loss.item()!r} vs {l64!r}, grad L2 err {gerr:.2e} "
          f"(cpu fp32 {ge32:.2e}), worst tensor {max(errs.items(), key=lambda kv: kv[1])}")
    assert oerr <= 1e-3, oerr
    assert abs(ts.loss.item() - l64) <= 1e-4 * abs(l64), (ts.loss.item(), l64)
    assert gerr <= max(1e-3, 2 * ge32), (gerr, ge32)
    bad = {k: (errs[k], e32[k]) for k in errs if errs[k] > max(1e-2, 3 * e32[k])}
    assert not bad, f"gradient errors above tolerance: {bad}"


def test_trainstep_losses_differ(cuda, oracle_runs):
    """The config reaches the kernels: the three losses give three different first-step values."""
    from light_unet.train_step import TrainStep
    sd, runs = oracle_runs
    x, t = (v.to(cuda) for v in _inputs(cuda))
    vals = {k: TrainStep(_fresh(sd, cuda), LOSS_CFGS[k][0])(x, t).item() for k in LOSS_CFGS}
    for k, v in vals.items():
        assert abs(v - runs[k][0][1]) <= 1e-4 * abs(runs[k][0][1])
    assert len({round(v, 4) for v in vals.values()}) == 3, vals


@pytest.mark.parametrize("key", sorted(LOSS_CFGS))
def test_trainstep_eager_equals_graph_replay(cuda, oracle_runs, key):
    from light_unet.train_step import TrainStep
    sd, _ = oracle_runs
    x, t = (v.to(cuda) for v in _inputs(cuda))
    te = TrainStep(_fresh(sd, cuda, 0.1), LOSS_CFGS[key][0], lr=1e-3)
    le = [te(x, t).item() for _ in range(3)]
    tg = TrainStep(_fresh(sd, cuda, 0.1), LOSS_CFGS[key][0], lr=1e-3)
    xs, tsb = torch.full_like(x, float("nan")), torch.empty_like(t)
    tg.capture(xs, tsb)
    assert len(tg._graphs) == 1
    xs.copy_(x)
    tsb.copy_(t)
    lg = [tg.replay().item() for _ in range(3)]
    assert le == lg, (le, lg)
    assert torch.equal(te.flat, tg.flat) and torch.equal(te.gflat, tg.gflat)
    assert torch.equal(te.opt.m, tg.opt.m) and torch.equal(te.opt.v, tg.opt.v)
    assert all(np.isfinite(le)) and int(tg.opt.step_t.item()) == 3


def test_trainstep_combined_agrees_with_autograd_dropin(cuda, oracle_runs):
    """TrainStep (eager) vs the drop-in model + CombinedLoss module + torch.optim.AdamW after 2
    steps, compared as test_trainstep_eager_graph_and_autograd_agree compares."""
    from light_unet.models.losses import CombinedLoss
    from light_unet.train_step import TrainStep
    sd, _ = oracle_runs
    x, t = (v.to(cuda) for v in _inputs(cuda))
    steps = 2
    m_a = _fresh(sd, cuda)
    opt = torch.optim.AdamW(m_a.parameters(), lr=1e-4, weight_decay=1e-5)
    crit = CombinedLoss()
    la = []
    for _ in range(steps):
        loss = crit(m_a(x), t)
        opt.zero_grad()
        loss.backward()
        opt.step()
        la.append(loss.item())
    m_b = _fresh(sd, cuda)
    ts = TrainStep(m_b, crit, lr=1e-4, weight_decay=1e-5)
    lb = [ts(x, t).item() for _ in range(steps)]
    np.testing.assert_allclose(la, lb, rtol=1e-5)
    pa, pb = m_a.flat_parameters().detach(), m_b.flat_parameters().detach()
    assert (pa - pb).abs().max().item() <= 3e-4 * steps


def test_trainstep_focal_tversky_config_is_the_old_path(cuda, oracle_runs, monkeypatch):
    """A TrainStep built from a FocalTversky config (or criterion) issues the FocalTversky entry
    points only and replays bit-identically to one built the old way."""
    from light_unet import _native
    from light_unet.models.losses import FocalTverskyLoss
    from light_unet.train_step import TrainStep
    sd, _ = oracle_runs
    x, t = (v.to(cuda) for v in _inputs(cuda))
    called = []
    real = _native.call

    def spy(name, *a):
        called.append(name)
        return real(name, *a)
    monkeypatch.setattr(_native, "call", spy)
    runs = []
    for cfg in (None, {"alpha": 0.7, "beta": 0.3, "gamma": 0.75, "smooth": 1e-6},
                LOSS_CFGS["ftl"][0], FocalTverskyLoss()):
        ts = TrainStep(_fresh(sd, cuda, 0.1), cfg, lr=1e-3)
        assert ts.family is None
        xs, tsb = x.clone(), t.clone()
        ts.capture(xs, tsb)
        ls = [ts.replay().item() for _ in range(3)]
        runs.append((ls, ts.flat.clone(), ts.gflat.clone()))
    assert not [n for n in called if "loss4" in n]
    assert "l3u_outconv_bwd_ftl_dz" in called or "l3u_outconv_bwd_ftl" in called
    for r in runs[1:]:
        assert r[0] == runs[0][0] and torch.equal(r[1], runs[0][1]) and torch.equal(r[2], runs[0][2])


def test_trainstep_bf16_storage_runs_the_twins(cuda, oracle_runs, monkeypatch):
    from light_unet import _native
    from light_unet.train_step import TrainStep
    sd, runs = oracle_runs
    x, t = (v.to(cuda) for v in _inputs(cuda))
    called = []
    real = _native.call

    def spy(name, *a):
        called.append(name)
        return real(name, *a)
    monkeypatch.setattr(_native, "call", spy)
    ts = TrainStep(_fresh(sd, cuda), LOSS_CFGS["combined"][0], dtype=torch.bfloat16)
    loss = ts(x, t).item()
    assert "l3u_outconv_fwd_loss4_bf16" in called
    assert [n for n in called if n.startswith("l3u_outconv_bwd_loss4p") and n.endswith("_bf16")]
    # bf16 activation storage (8 mantissa bits) through a 9-block network: percent level
    l64 = runs["combined"][0][1]
    assert np.isfinite(loss) and abs(loss - l64) <= 2e-2 * abs(l64), (loss, l64)


# ------------------------------------------------------------------ two ranks
def test_trainstep_combined_two_ranks(cuda, tmp_path):
    """CombinedLoss on 2 ranks x bs 2 (gloo, both ranks on this GPU) against the single-process
    bs-4 step: exact mode (the four sums all-reduced in one call, M = world x local count) gives
    the bs-4 loss (1e-6 relative) and gradient (1e-4 relative L2); local mode the mean of the two
    half-batch gradients (plain DDP)."""
    import socket
    import subprocess
    from light_unet.train_step import TrainStep
    import _loss_family_dist_worker as W
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tests", "_loss_family_dist_worker.py"), str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    rk = [np.load(tmp_path / f"rank{i}.npz") for i in range(2)]
    x, t = W.batch()
    dx, dt = torch.from_numpy(x).to(cuda), torch.from_numpy(t).to(cuda)

    def rel(a, b):
        return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))

    ts = TrainStep(W.fresh_model(cuda), W.LOSS_CFG)
    l1 = ts(dx, dt).item()
    g1 = ts.gflat.cpu().numpy().astype(np.float64)
    gh = []
    for h in range(2):
        th = TrainStep(W.fresh_model(cuda), W.LOSS_CFG)
        th(dx[2 * h:2 * h + 2].contiguous(), dt[2 * h:2 * h + 2].contiguous())
        gh.append(th.gflat.cpu().numpy().astype(np.float64))
    gmean = 0.5 * (gh[0] + gh[1])
    for z in rk:
        print(f"exact loss {float(z['A_loss1'])!r} vs {l1!r}, grad rel {rel(z['A_g1'], g1):.2e}; "
              f"local grad rel {rel(z['B_g1'], gmean):.2e}")
        assert abs(float(z["A_loss1"]) - l1) <= 1e-6 * abs(l1)
        assert rel(z["A_g1"], g1) <= 1e-4
        assert rel(z["B_g1"], gmean) <= 1e-4
    assert np.array_equal(rk[0]["A_g1"], rk[1]["A_g1"]), "ranks diverged"


# ------------------------------------------------------------------ fast trainer
def test_fast_trainer_runs_combined_loss_on_the_graph_step(cuda):
    """A Trainer whose criterion is CombinedLoss trains on the graph-replayed step (the reference
    loop is not taken) and records the per-step losses of the drop-in autograd loop (1e-5)."""
    from light_unet import fast_trainer
    from light_unet.models.losses import CombinedLoss
    from test_fast_trainer_gpu import StandInTrainer, _batches, _fast_cls
    batches = _batches(3, 3, bs=2, size=16)
    ref = StandInTrainer(cuda, batches)
    ref.criterion = CombinedLoss()
    cls = _fast_cls()

    def no_fallback(self, epoch):
        raise AssertionError("the reference loop was taken")
    setattr(cls, fast_trainer._FALLBACK, {"train_epoch": no_fallback,
                                          "_train_epoch_step_based": no_fallback})
    fast = cls(cuda, batches)
    fast.criterion = CombinedLoss()
    a = ref.train_epoch(0)
    b = fast.train_epoch(0)
    step = fast._l3u_fast.step
    assert step.family is not None and step.family[5] == 0.2 and step._graphs is not None
    lr = [v for tag, v, _ in ref.writer.rec if tag == "Loss/train_step"]
    lf = [v for tag, v, _ in fast.writer.rec if tag == "Loss/train_step"]
    print("drop-in", lr, "fast", lf)
    assert len(lr) == len(lf) == 3
    np.testing.assert_allclose(lf, lr, rtol=1e-5, atol=0)
    assert abs(a - b) <= 1e-5 * abs(a)
