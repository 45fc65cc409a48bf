"""The fused block-tail backward family against ONE fp64 torch-CPU autograd graph.

The ResidualBlock tail (norm2, relu2 and the residual add, unet3d.py:62-63,87-91) with its two
producers,

    y2 = W2 . z2                 conv2.pointwise (K = J)
    r  = Wr . x                  Conv1x1 shortcut (K = cin)
    out = leaky_relu(IN(y2; g2, b2) + IN(r; gr, br), 0.01);   out.backward(dout)

is differentiated by autograd in fp64 and every entry point that forms that backward inside the two
pointwise backwards is compared with it through the C ABI: l3u_norm_act_bwd_reduce[_r1|_up] (the
tail partials: d(beta2), d(gamma2), d(gamma_r)), l3u_pw_bwd_tail[_r1|_up] (sel 1, then sel 2
accumulating) and l3u_pw_bwd_tail_pair (both in one launch, bit-identical to the two calls), with
the out_conv dz forms (l3u_outconv_bwd_dz / l3u_outconv_bwd_ftl_dz) feeding the rank-1 dout.

The kernels get y2, r and out as the fp64 values rounded to fp32 (the LeakyReLU mask is the
reference's by construction: no kink flip can enter), records built from the fp64 statistics, and
inputs that are fp32-representable, so what is measured is the kernels' own arithmetic.

Shapes (csrc/pwconv.hip pw_sch and the launchers, csrc/norm.hip elem_blocks): S = 576 (256-voxel
chunks, ragged last chunk, one tail partial), 2400 (512-voxel chunks, ragged), 4800 (two tail
partials, 256-voxel chunks, ragged), 192 (less than one chunk: every load clamped); (J, K) covers
NJ 1 / 2 and partial row / column tiles; two 32^3 cases keep the NK = 2 / 4 column splits (they
need >= 512 workgroups).  dout forms: plain, rank-1 (dscale[j] * dz) and up (dskip + the MaxPool3d
backward of dpool); the second problem's yr also as a rank-1 operand (the first block).

Bounds (test_ops_gpu.close: max error relative to the reference's max), the project's bounds for
the unfused ops these kernels replace: 1e-4 both dx (dy2 / dr in test_norm_act_fwd_bwd), 1e-4
the weight gradients, 1e-5 the three parameter-gradient sums.

The one exception is the shortcut's weight gradient at K = 1, a sum that cancels (run_case): the
same graph evaluated by torch on the CPU in fp32 is up to 7.4e-4 from the fp64 one there (<= 2e-6
in every other quantity), comparable with the kernels' 1.3e-3, so that quantity is held to 3 x the
measured fp32 CPU error, 2.2e-3 of max |dW|, and besides to 1e-4 of the uncancelled sum.

Worst errors measured on an MI355X over all cases of this module (printed by the module's
`worst_errors` fixture, pytest -s), relative to the reference's max:
    l3u_norm_act_bwd_reduce      dbeta2 6.0e-10  dgamma2 1.1e-7  dgamma_r 1.1e-7
    l3u_norm_act_bwd_reduce_r1   dbeta2 1.9e-8   dgamma2 5.6e-8  dgamma_r 8.3e-8
    l3u_norm_act_bwd_reduce_up   dbeta2 4.0e-8   dgamma2 8.9e-8  dgamma_r 1.0e-7
    l3u_pw_bwd_tail              dx 2.6e-7   dW 4.2e-7
    l3u_pw_bwd_tail_r1           dx 3.0e-7   dW 5.2e-7
    l3u_pw_bwd_tail_up           dx 2.8e-7   dW 5.0e-7
    l3u_pw_bwd_tail_pair         dx 3.0e-7   dW 5.2e-7   (bit-identical to the two calls everywhere)
    l3u_outconv_bwd_dz / _ftl_dz dz 3.1e-7   dw 1.5e-7   db 1.1e-7
    dW of sel 2 at K = 1: 6.2e-7 of the uncancelled sum; relative to max |dW| 1.3e-3 (plain),
    1.3e-4 (r1), 5.1e-4 (up), where torch's fp32 CPU evaluation of the same graph is at 7.4e-4.
With the dscale multiply removed from pw_bwd_fused_kernel every r1 case fails (31), with the sign
of the xhat * mean(g * xhat) term flipped every comparison with fp64 fails (97 cases).
"""
import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import SLOPE, nat, st

pytestmark = pytest.mark.gpu

WORST = {}
NAN = float("nan")
SENTINEL = 7.0
# the shortcut's weight gradient at K = 1, relative to max |dW|: 3 x 7.4e-4, the worst error of
# torch's fp32 CPU evaluation of the same graph over this module's K = 1 cases (run_case)
TOL_DWB_K1 = 2.2e-3


@pytest.fixture(scope="module", autouse=True)
def worst_errors():
    yield
    print()
    for k in sorted(WORST):
        print(f"worst {k}: {WORST[k]:.2e}")


def relerr(a, b, floor=0.0):
    """max error relative to the reference's max (test_ops_gpu.close), or to `floor` if larger"""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), floor, 1e-30)


def close(a, b, rtol, what, key, floor=0.0):
    """test_ops_gpu.close, keeping the worst error seen per entry point and quantity."""
    assert torch.isfinite(a).all(), f"{what}: non-finite values (an element was never written?)"
    err = relerr(a, b, floor)
    WORST[key] = max(WORST.get(key, 0.0), err)
    assert err <= rtol, f"{what}: max err {err:.3e} (rel to the reference's scale) > {rtol:.3e}"


def tail_graph(inputs, dt):
    """The block tail with its two producers in dtype dt; the caller back-propagates `out`."""
    leaves = [v.to(dt).clone().requires_grad_(True) for v in inputs]
    z2r, xr, W2r, Wrr, g2r, b2r, grr, brr = leaves
    y2 = torch.einsum("jk,nks->njs", W2r, z2r).contiguous()   # (einsum returns a permuted view)
    r = torch.einsum("jk,nks->njs", Wrr, xr).contiguous()
    r.retain_grad()
    out = F.leaky_relu(F.instance_norm(y2, weight=g2r, bias=b2r, eps=1e-5) +
                       F.instance_norm(r, weight=grr, bias=brr, eps=1e-5), SLOPE)
    return leaves, y2, r, out


def tail_grads(leaves):
    z2r, xr, W2r, Wrr, g2r, b2r, grr, brr = leaves
    return {"dxa": z2r.grad, "dxb": xr.grad, "dwa": W2r.grad, "dwb": Wrr.grad,
            "dbeta2": b2r.grad, "dgamma2": g2r.grad, "dgamma_r": grr.grad}


def f32(t):
    """fp64 tensor of fp32-representable values"""
    return t.float().double()


def rec_of(v, g, b):
    """InstanceNorm records [N][C][8] from the fp64 statistics of v [N][C][S] (no dropout)"""
    N, C = v.shape[:2]
    m = v.mean(-1)
    rs = 1 / torch.sqrt(v.var(-1, unbiased=False) + 1e-5)
    rc = torch.zeros(N, C, 8, dtype=torch.float64)
    rc[..., 0], rc[..., 1] = m, rs
    rc[..., 2] = g * rs
    rc[..., 3] = b
    rc[..., 4], rc[..., 5], rc[..., 6] = 1, g.expand(N, C), b.expand(N, C)
    return rc


class Half:
    """A [N][C][S] device tensor, contiguous or (strided) one half of a 2C-channel buffer whose
    other half holds SENTINEL and must stay untouched."""

    def __init__(self, t, cuda, strided, upper=True):
        t = t.float()
        N, C, S = t.shape
        if strided:
            self.buf = torch.full((N, 2 * C, S), SENTINEL, device=cuda)
            self.view = self.buf[:, C:] if upper else self.buf[:, :C]
            self.other = self.buf[:, :C] if upper else self.buf[:, C:]
            self.view.copy_(t.to(cuda))
            self.ns = 2 * C * S
        else:
            self.buf = t.to(cuda).contiguous()
            self.view, self.other, self.ns = self.buf, None, C * S
        self.ptr = self.view.data_ptr()

    def untouched(self):
        return self.other is None or bool((self.other == SENTINEL).all())


def nan_at(shape, off, cuda):
    """a NaN-filled fp32 device tensor whose storage starts `off` elements past a 16-byte boundary"""
    n = 1
    for d in shape:
        n *= d
    t = torch.full((n + off,), NAN, device=cuda)[off:].view(shape)
    assert t.data_ptr() % 16 == 4 * off
    return t


def outconv_dz(cuda, h, gen, check=False, off=0):
    """A small out_conv problem on h [N][C][S] (fp64, fp32-representable): dz = d(pre-sigmoid) of
    the FocalTversky loss from l3u_outconv_bwd_dz, and the out_conv weight (the rank-1 dout of the
    last block's tail is w[c] * dz).  check: also l3u_outconv_bwd_ftl_dz and l3u_outconv_bwd, the
    bit-identities between the three and dz against the fp64 closed form.  off: dz / dh start that
    many elements into their storage (off = 1: 4-byte aligned only, so the backward must not take
    its 16-byte vector stores)."""
    from oracle.unet_oracle import focal_tversky
    N, C, S = h.shape
    w = f32(torch.randn(1, C, generator=gen, dtype=torch.float64) * 0.3)
    b = f32(torch.randn(1, generator=gen, dtype=torch.float64))
    t = (torch.rand(N, 1, S, generator=gen) > 0.8).double()
    hd, wd, bd, td = (v.float().to(cuda) for v in (h, w, b, t))
    nb = nat().query("l3u_outconv_nblocks", S)
    fpart = torch.full((N * nb * 3,), NAN, device=cuda)
    pd = torch.full((N, 1, S), NAN, device=cuda)
    nat().call("l3u_outconv_fwd", hd.data_ptr(), C * S, wd.data_ptr(), bd.data_ptr(), pd.data_ptr(),
               td.data_ptr(), fpart.data_ptr(), N, C, S, st())
    sums = torch.empty(3, dtype=torch.float64, device=cuda)
    nat().call("l3u_ftl_reduce", fpart.data_ptr(), N * nb, sums.data_ptr(), st())
    abgs = (0.7, 0.3, 0.75, 1e-6)
    part = torch.full((N * nb * (C + 1),), NAN, dtype=torch.float64, device=cuda)
    dz = nan_at((N, 1, S), off, cuda)
    loss = torch.full((), NAN, device=cuda)
    nat().call("l3u_outconv_bwd_dz", None, pd.data_ptr(), td.data_ptr(), sums.data_ptr(), *abgs, None,
               hd.data_ptr(), C * S, wd.data_ptr(), dz.data_ptr(), S, part.data_ptr(),
               loss.data_ptr(), N, C, S, st())
    torch.cuda.synchronize()
    if check:
        part2, dz2, loss2 = torch.full_like(part, NAN), nan_at((N, 1, S), off, cuda), torch.full_like(loss, NAN)
        nat().call("l3u_outconv_bwd_ftl_dz", pd.data_ptr(), td.data_ptr(), fpart.data_ptr(), N * nb,
                   *abgs, None, hd.data_ptr(), C * S, wd.data_ptr(), dz2.data_ptr(), S,
                   part2.data_ptr(), loss2.data_ptr(), N, C, S, st())
        part3, loss3 = torch.full_like(part, NAN), torch.full_like(loss, NAN)
        dh = nan_at((N, C, S), off, cuda)
        nat().call("l3u_outconv_bwd", None, pd.data_ptr(), td.data_ptr(), sums.data_ptr(), *abgs, None,
                   hd.data_ptr(), C * S, wd.data_ptr(), dh.data_ptr(), C * S, part3.data_ptr(),
                   loss3.data_ptr(), N, C, S, st())
        torch.cuda.synchronize()
        assert torch.isfinite(dz).all() and torch.isfinite(part).all() and torch.isfinite(loss)
        assert torch.equal(dz2, dz) and torch.equal(part2, part) and torch.equal(loss2, loss)
        assert torch.equal(wd[0][None, :, None] * dz, dh)      # w[c] * dz == dh, bit for bit
        assert torch.equal(part3, part) and torch.equal(loss3, loss)
        # fp64 closed form: autograd of the loss with respect to the pre-sigmoid logits
        lg = (torch.einsum("oc,ncs->nos", w, h) + b[None, :, None]).requires_grad_(True)
        ref = focal_tversky(torch.sigmoid(lg), t)
        ref.backward()
        close(dz, lg.grad, 1e-4, f"outconv dz {tuple(h.shape)}", "l3u_outconv_bwd_dz dz")
        assert abs(float(loss) - float(ref.detach())) <= 1e-5 * abs(float(ref.detach())) + 1e-7
        ps = part.view(N * nb, C + 1).sum(0).cpu()
        close(ps[:C], torch.einsum("nos,ncs->c", lg.grad, h), 1e-4, "outconv dw", "l3u_outconv_bwd_dz dw")
        close(ps[C:], lg.grad.sum().reshape(1), 1e-4, "outconv db", "l3u_outconv_bwd_dz db")
    return dz, w[0]


def run_case(cuda, N, J, K, dims, form, r1yr=False, strided=False, seed=0):
    D, H, W = dims
    S = D * H * W
    gen = torch.Generator().manual_seed(1000 + seed)

    def rnd(*s):
        return f32(torch.randn(*s, generator=gen, dtype=torch.float64))

    # ---- the fp64 reference graph
    z2, x = rnd(N, J, S), rnd(N, K, S)
    W2, Wr = f32(rnd(J, J) / J ** 0.5), f32(rnd(J, K) / K ** 0.5)
    g2, b2, gr, br = f32(1 + 0.3 * rnd(J)), f32(0.3 * rnd(J)), f32(1 + 0.3 * rnd(J)), f32(0.3 * rnd(J))
    inputs = (z2, x, W2, Wr, g2, b2, gr, br)
    leaves, y2, r, out = tail_graph(inputs, torch.float64)
    y2v, rv, outv = y2.detach(), r.detach(), out.detach()

    # ---- dout, in the form under test
    dsc = dpool = idx = None
    if form == "plain":
        dout = rnd(N, J, S)
        dsrc = Half(dout, cuda, strided)
    elif form == "r1":
        dz, wo = outconv_dz(cuda, f32(outv), gen)
        dout = wo[None, :, None] * dz.double().cpu()
        dsrc = Half(dz, cuda, strided)
        dsc = wo.float().to(cuda)
    else:
        assert form == "up" and D % 2 == 0 and H % 2 == 0 and W % 4 == 0
        lev, dskip, dpl = rnd(N, J, S), rnd(N, J, S), rnd(N, J, S // 8)
        lw = lev.view(N, J, D // 2, 2, H // 2, 2, W // 2, 2)   # tie-free: one maximum per window
        assert bool(((lw == lw.amax((3, 5, 7), keepdim=True)).sum((3, 5, 7)) == 1).all())
        lr_ = lev.view(N, J, D, H, W).clone().requires_grad_(True)
        F.max_pool3d(lr_, 2).backward(dpl.view(N, J, D // 2, H // 2, W // 2))
        dout = dskip + lr_.grad.view(N, J, S)
        levd = lev.float().to(cuda)
        pooled = torch.empty(N, J, S // 8, device=cuda)
        idx = torch.empty(N, J, S // 8, dtype=torch.uint8, device=cuda)
        nat().call("l3u_maxpool2_fwd", levd.data_ptr(), J * S, pooled.data_ptr(), J * (S // 8),
                   idx.data_ptr(), N, J, D, H, W, st())
        dsrc = Half(dskip, cuda, strided)
        dpool = dpl.float().to(cuda)
    out.backward(dout)
    init = rnd(N, K, S)
    ref = tail_grads(leaves)
    ref["dxb"] = ref["dxb"] + init
    # K = 1: r = Wr[j] * x is normalised per channel, so the block does not depend on |Wr[j]| and
    # dWr is what the eps of InstanceNorm leaves of a sum that otherwise cancels (it is ~0 but for
    # the channels with Wr[j]^2 var(x) near eps): a sum that cancels to ~eps / var of its terms, in
    # which any fp32 evaluation loses digits.  The SAME graph evaluated by torch on the CPU in fp32
    # is 3e-6 .. 7.4e-4 (by case) from the fp64 one in that quantity relative to its max, the
    # kernels up to 1.3e-3, against <= 2e-6 for the CPU in every other quantity: rounding
    # residue of the same order in both (each a different draw of the roundings of the same
    # cancelling sum: the kernels form dY in fp32 from fp32 means exactly as torch's fp32
    # InstanceNorm backward does).  So at K = 1 that one quantity is held, relative to max |dW| as
    # everything else, to TOL_DWB_K1 = 3 x the worst fp32 CPU error over this module's K = 1 cases
    # (the rule of tests/test_model_gpu.py for scale-invariant tensors); each case's fp32 CPU
    # error is kept in WORST.  An extra check holds it to 1e-4 of the size the sum would have
    # without the cancellation, sqrt(sum (dr * x)^2).
    tol_dwb, floor_dwb = 1e-4, 0.0
    if K == 1:
        tol_dwb = TOL_DWB_K1
        l32, _, _, o32 = tail_graph(inputs, torch.float32)
        o32.backward(dout.float())
        e32 = relerr(tail_grads(l32)["dwb"], ref["dwb"])
        WORST["torch CPU fp32 dW (sel 2, K = 1), rel to max |dW|"] = max(
            WORST.get("torch CPU fp32 dW (sel 2, K = 1), rel to max |dW|", 0.0), e32)
        floor_dwb = (r.grad * x).square().sum((0, 2)).sqrt().max().item()

    # ---- device operands
    y2d, outd = y2v.float().contiguous().to(cuda), outv.float().contiguous().to(cuda)
    z2d, xd = Half(z2, cuda, False), Half(x, cuda, strided, upper=False)
    W2d, Wrd = W2.float().to(cuda), Wr.float().to(cuda)
    rec2 = rec_of(y2v, g2, b2).float().to(cuda)
    recr = rec_of(rv, gr, br)
    if r1yr:   # the first block's shortcut: r = wsc[c] * x, one stored channel, record slot 7
        assert K == 1 and J <= 16
        recr[..., 7] = Wr[:, 0]
        rd, rns = xd.view, -xd.ns
        assert xd.ns % 4 == 0
    else:
        rd, rns = rv.float().contiguous().to(cuda), J * S
    recr = recr.float().to(cuda)

    # ---- the tail partials from the reduce entry point of this form
    nb = nat().query("l3u_norm_act_nblocks", S)
    tp = torch.full((J * N * nb * 3,), NAN, dtype=torch.float64, device=cuda)
    tail = (outd.data_ptr(), J * S, y2d.data_ptr(), J * S, rec2.data_ptr(), rd.data_ptr(), rns,
            recr.data_ptr(), tp.data_ptr(), N, J)
    if form == "plain":
        red = "l3u_norm_act_bwd_reduce"
        nat().call(red, dsrc.ptr, dsrc.ns, *tail, S, st())
    elif form == "r1":
        red = "l3u_norm_act_bwd_reduce_r1"
        nat().call(red, dsrc.ptr, dsrc.ns, dsc.data_ptr(), *tail, S, st())
    else:
        red = "l3u_norm_act_bwd_reduce_up"
        nat().call(red, dsrc.ptr, dsrc.ns, dpool.data_ptr(), J * (S // 8), idx.data_ptr(), *tail,
                   D, H, W, st())
    torch.cuda.synchronize()
    what = f"N{N} J{J} K{K} {dims} {form}{' r1yr' if r1yr else ''}{' strided' if strided else ''}"
    ps = tp.view(J, N, nb, 3).sum((1, 2)).cpu()
    close(ps[:, 0], ref["dbeta2"], 1e-5, f"dbeta2 {what}", f"{red} dbeta2")
    close(ps[:, 1], ref["dgamma2"], 1e-5, f"dgamma2 {what}", f"{red} dgamma2")
    close(ps[:, 2], ref["dgamma_r"], 1e-5, f"dgamma_r {what}", f"{red} dgamma_r")

    # ---- the two pointwise backwards: two single calls, then the pair
    npa = nat().query("l3u_pw_bwd_nparts", N, J, J, S)
    npb = nat().query("l3u_pw_bwd_nparts", N, J, K, S)
    assert npa > 0 and npb > 0

    def outputs():
        dxa = Half(torch.full((N, J, S), NAN), cuda, strided)
        dxb = Half(init, cuda, strided, upper=False)          # the accumulating problem
        return (dxa, dxb, torch.full((npa * J * J,), NAN, device=cuda),
                torch.full((npb * J * K,), NAN, device=cuda))

    def single(sel, yr, yrns, rec, xin, w, dx, acc, part, K_):
        body = (outd.data_ptr(), J * S, yr.data_ptr(), yrns, rec.data_ptr(), tp.data_ptr(), nb, sel,
                xin.ptr, xin.ns, w.data_ptr(), dx.ptr, dx.ns, acc, part.data_ptr(), N, J, K_)
        if form == "plain":
            nat().call("l3u_pw_bwd_tail", dsrc.ptr, dsrc.ns, *body, S, st())
        elif form == "r1":
            nat().call("l3u_pw_bwd_tail_r1", dsrc.ptr, dsrc.ns, dsc.data_ptr(), *body, S, st())
        else:
            nat().call("l3u_pw_bwd_tail_up", dsrc.ptr, dsrc.ns, dpool.data_ptr(), J * (S // 8),
                       idx.data_ptr(), *body, D, H, W, st())

    sa, sb, spa, spb = outputs()
    single(1, y2d, J * S, rec2, z2d, W2d, sa, 0, spa, J)
    single(2, rd, rns, recr, xd, Wrd, sb, 1, spb, K)
    pa, pb, ppa, ppb = outputs()
    nat().call("l3u_pw_bwd_tail_pair", dsrc.ptr, dsrc.ns, dsc.data_ptr() if dsc is not None else None,
               dpool.data_ptr() if dpool is not None else None, J * (S // 8) if dpool is not None else 0,
               idx.data_ptr() if idx is not None else None, H if dpool is not None else 0,
               W if dpool is not None else 0, outd.data_ptr(), J * S, tp.data_ptr(), nb,
               y2d.data_ptr(), J * S, rec2.data_ptr(), z2d.ptr, z2d.ns, W2d.data_ptr(), pa.ptr, pa.ns, 0,
               ppa.data_ptr(), J, 1,
               rd.data_ptr(), rns, recr.data_ptr(), xd.ptr, xd.ns, Wrd.data_ptr(), pb.ptr, pb.ns, 1,
               ppb.data_ptr(), K, 2, N, J, S, st())
    torch.cuda.synchronize()
    ent = {"plain": "l3u_pw_bwd_tail", "r1": "l3u_pw_bwd_tail_r1", "up": "l3u_pw_bwd_tail_up"}[form]
    for tag, (dxa, dxb, parta, partb) in ((ent, (sa, sb, spa, spb)),
                                          ("l3u_pw_bwd_tail_pair", (pa, pb, ppa, ppb))):
        close(dxa.view, ref["dxa"], 1e-4, f"{tag} dx sel1 {what}", f"{tag} dx")
        close(dxb.view, ref["dxb"], 1e-4, f"{tag} dx sel2 {what}", f"{tag} dx")
        close(parta.view(npa, J, J).double().sum(0), ref["dwa"], 1e-4, f"{tag} dW sel1 {what}", f"{tag} dW")
        dwb = partb.view(npb, J, K).double().sum(0)
        close(dwb, ref["dwb"], tol_dwb, f"{tag} dW sel2 {what}",
              f"{tag} dW" + (" (sel 2, K = 1)" if K == 1 else ""))
        if K == 1:
            close(dwb, ref["dwb"], 1e-4, f"{tag} dW sel2 / uncancelled sum {what}",
                  f"{tag} dW (sel 2, K = 1, rel to the uncancelled sum)", floor_dwb)
        assert dxa.untouched() and dxb.untouched(), f"{tag} {what}: wrote outside its channel range"
    # the pair is the two calls, bit for bit (include/l3u.h)
    assert torch.equal(pa.view, sa.view) and torch.equal(pb.view, sb.view), what
    assert torch.equal(ppa, spa) and torch.equal(ppb, spb), what
    assert dsrc.untouched() and xd.untouched()


SHAPES = [(2, (6, 8, 12)), (3, (10, 12, 20)), (2, (10, 20, 24)), (3, (4, 4, 12))]
JK = [(16, 16), (16, 1), (32, 16), (20, 12), (8, 3)]
FORMS = ["plain", "r1", "up"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("jk", JK)
@pytest.mark.parametrize("shape", SHAPES)
def test_tail_bwd_vs_fp64(cuda, shape, jk, form):
    (N, dims), (J, K) = shape, jk
    run_case(cuda, N, J, K, dims, form, seed=SHAPES.index(shape) * 16 + JK.index(jk))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("J", [16, 12])
@pytest.mark.parametrize("shape", SHAPES)
def test_tail_bwd_rank1_yr_vs_fp64(cuda, shape, J, form):
    """The first block: the second problem's yr is r = wsc[c] * x, one stored channel (negative
    yrb_nstride, record slot 7 = wsc, Kb = 1)."""
    N, dims = shape
    run_case(cuda, N, J, 1, dims, form, r1yr=True, seed=100 + SHAPES.index(shape) * 2 + J)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", [(2, 20, 12, (6, 8, 12), False), (2, 32, 16, (10, 20, 24), False),
                                  (3, 16, 1, (10, 12, 20), True)])
def test_tail_bwd_strided_views(cuda, case, form):
    """dout (dz / dskip), x and both dx as halves of 2C-channel buffers (zero-copy concat): the
    other halves stay untouched."""
    N, J, K, dims, r1yr = case
    run_case(cuda, N, J, K, dims, form, r1yr=r1yr, strided=True, seed=200 + J)


@pytest.mark.parametrize("form", ["plain", "up"])
@pytest.mark.parametrize("K", [32, 64])
def test_tail_bwd_column_splits(cuda, K, form):
    """NK = 2 (K = 32) and NK = 4 (K = 64): the column splits survive only from 512 workgroups on
    (production takes NK = 2 in the 48^3 up-block), hence N = 4 at 32^3."""
    run_case(cuda, 4, 32, K, (32, 32, 32), form, seed=300 + K)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("case", [(2, 16, (6, 8, 12)), (3, 8, (4, 4, 12)), (1, 20, (10, 20, 24))])
def test_outconv_dz_forms(cuda, case, off):
    """l3u_outconv_bwd_dz == l3u_outconv_bwd_ftl_dz bit for bit (dz, partials, loss), w[c] * dz ==
    l3u_outconv_bwd's dh bit for bit, and dz against the fp64 closed form (test_outconv_ftl_fused's
    bound); off = 1: with dz / dh one element into their storage (the scalar stores)."""
    N, C, (D, H, W) = case
    gen = torch.Generator().manual_seed(31)
    h = f32(torch.randn(N, C, D * H * W, generator=gen, dtype=torch.float64))
    outconv_dz(cuda, h, gen, check=True, off=off)


@pytest.mark.parametrize("entry", ["l3u_pw_bwd_tail_pair", "l3u_pw_bwd_tail_pair_bf16"])
def test_tail_pair_rejects_dscale_with_dpool(cuda, entry):
    """dscale and dpool are mutually exclusive (include/l3u.h): the pool-fold kernels carry no
    dscale code, so the combination is refused with hipErrorInvalidValue before any launch and
    every output keeps its contents."""
    N, J, K, D, H, W = 2, 16, 16, 4, 4, 12
    S = D * H * W
    bf = entry.endswith("_bf16")
    gen = torch.Generator().manual_seed(5)

    def act(C):
        t = torch.randn(N, C, S, generator=gen).to(cuda)
        return t.to(torch.bfloat16) if bf else t

    dout = torch.randn(N, 1, S, generator=gen).to(cuda)
    out, y2, r, z2, x = act(J), act(J), act(J), act(J), act(K)
    dsc = torch.randn(J, generator=gen).to(cuda)
    dpool = torch.randn(N, J, S // 8, generator=gen).to(cuda)
    idx = torch.zeros(N, J, S // 8, dtype=torch.uint8, device=cuda)
    rec = rec_of(torch.randn(N, J, S, generator=gen, dtype=torch.float64), torch.ones(J, dtype=torch.float64),
                 torch.zeros(J, dtype=torch.float64)).float().to(cuda)
    tp = torch.zeros(J * N * 3, dtype=torch.float64, device=cuda)
    W2, Wr = torch.randn(J, J, generator=gen).to(cuda), torch.randn(J, K, generator=gen).to(cuda)
    npw = nat().query("l3u_pw_bwd_nparts", N, J, K, S)
    outs = [torch.full((N, J, S), SENTINEL, device=cuda), torch.full((N, K, S), SENTINEL, device=cuda),
            torch.full((npw * J * J,), SENTINEL, device=cuda), torch.full((npw * J * K,), SENTINEL, device=cuda)]

    def pair(dscale, dpl):
        return nat().query(entry, dout.data_ptr(), S, dscale, dpl, J * (S // 8) if dpl else 0,
                           idx.data_ptr() if dpl else None, H if dpl else 0, W if dpl else 0,
                           out.data_ptr(), J * S, tp.data_ptr(), 1,
                           y2.data_ptr(), J * S, rec.data_ptr(), z2.data_ptr(), J * S, W2.data_ptr(),
                           outs[0].data_ptr(), J * S, 0, outs[2].data_ptr(), J, 1,
                           r.data_ptr(), J * S, rec.data_ptr(), x.data_ptr(), K * S, Wr.data_ptr(),
                           outs[1].data_ptr(), K * S, 0, outs[3].data_ptr(), K, 2, N, J, S, st())

    invalid = 1   # hipErrorInvalidValue
    assert pair(dsc.data_ptr(), dpool.data_ptr()) == invalid
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)
    # (the same arguments with dscale alone are accepted and write every output)
    assert pair(dsc.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) and not bool((o == SENTINEL).any()) for o in outs)
