"""Which bytes each C-ABI launch may touch: a declarative table read off include/l3u.h.

`footprints(name, args)` returns one `Operand` per pointer argument (and per pointer field of an
l3u_norm_src argument) of the call `_native.call(name, *args)`: its role ("r", "w" or "rw") and the
byte intervals, relative to the pointer, that the header documents for it.  The sizes come from
the call's own scalar arguments and, for partial buffers, from the library's host queries
(`_native.query`: no device needed).  tests/fenced.py poisons everything else of the allocation
round a fenced call; tests/test_footprints.py holds the engine's launch plan against the table on
the CPU.

Conventions (include/l3u.h):
  - an [N][C][S] operand with batch stride ns is N intervals [n*ns*E, (n*ns + C*S)*E);
  - a rank-1 operand (negative batch stride -ns) stores ONE channel per sample, stride ns;
  - a NULL operand has no interval;
  - E is 4, or 2 for the saved activations of a _bf16 twin (gradients, weights, records and
    partials stay fp32 / fp64 in either form);
  - l3u_reduce_segments[_adamw] read and write what their item table says, so `items_of(ptr, n)`
    must hand over the n rows of 8 int64 at `ptr` (the CPU tensor in a trace, a device read-back
    under the fence).

Data-path kernels (l3u_ccl_*, l3u_aug_*, l3u_pp_*, l3u_rs_*, l3u_window_*, ...) have no entry:
`footprints` returns None for them and the fence gives them end guards only.
"""
import ctypes
from collections import namedtuple

from light_unet import _native as nat

# arg: index into args; field: None or the l3u_norm_src field name; ptr: the address;
# role: "r" / "w" / "rw"; ivs: [(lo, hi)] bytes relative to ptr, ascending and disjoint
Operand = namedtuple("Operand", "arg field ptr role ivs")

TICKET_INTS = 32 * 33   # L3U_ADAMW_TICKET_INTS


class _A:
    """The scalar and pointer arguments of one call by their names in include/l3u.h."""

    def __init__(self, names, args):
        names = names.split()
        if len(args) != len(names) + 1:   # + the trailing stream
            raise ValueError(f"expected {len(names) + 1} arguments, got {len(args)}")
        self.index = {n: i for i, n in enumerate(names)}
        self.__dict__.update(zip(names, args))


def _q(name, *a):
    return nat.query(name, *(int(v) for v in a))


def T(ns, N, C, S, E=4):
    """[N][C][S] of E-byte elements, batch stride ns (negative: rank-1, one stored channel)."""
    ns, C = (-ns, 1) if ns < 0 else (ns, C)
    return [(n * ns * E, (n * ns + C * S) * E) for n in range(N)]


def B(nbytes):
    return [(0, int(nbytes))]


def _src(N, C):
    """The pointer fields of an l3u_norm_src normalising [N][C] planes."""
    return lambda s: {"stat_part": ("r", B(N * C * s.nsb * 3 * 4)), "gamma": ("r", B(C * 4)),
                      "beta": ("r", B(C * 4)), "step": ("r", B(4)),
                      "rec_out": ("w", B(N * C * 8 * 4)), "rank1": ("r", B(C * 4))}


def _acc(flag):
    return "rw" if flag else "w"


# ---------------------------------------------------------------------------------- the table
# name -> (argument names as in include/l3u.h, fn(a, E) -> {argument: (role, intervals) or, for
# an l3u_norm_src argument, a function of the struct}, in-place pairs allowed to overlap)
def _dw3_fwd(a, E):
    S = a.D * a.H * a.W
    return {"x": ("r", T(a.x_ns, a.N, a.C, S, E)), "w": ("r", B(a.C * 27 * 4)),
            "rec": ("r", B(a.N * a.C * 32)), "src": _src(a.N, a.C),
            "y": ("w", T(a.y_ns, a.N, a.C, S, E))}


def _dw3_bwd(a, E):
    S = a.D * a.H * a.W
    nch = _q("l3u_dw3_nchunk", a.N, a.C, a.D, a.H, a.W)
    return {"dz": ("r", T(a.dz_ns, a.N, a.C, S)), "x": ("r", T(a.x_ns, a.N, a.C, S, E)),
            "w": ("r", B(a.C * 27 * 4)), "rec": ("r", B(a.N * a.C * 32)),
            "dx": (_acc(a.accumulate), T(a.dx_ns, a.N, a.C, S)),
            "dw_part": ("w", B(a.C * a.N * nch * 27 * 4)),
            "in_part": ("w", B(a.C * a.N * nch * 2 * 8))}


def _pw_fwd(a, E):
    nsb = _q("l3u_pw_stat_nsb", a.K, a.Nout, a.S)
    return {"x": ("r", T(a.x_ns, a.N, a.K, a.S, E)), "w": ("r", B(a.Nout * a.K * 4)),
            "bias": ("r", B(a.Nout * 4)), "y": (_acc(a.accumulate), T(a.y_ns, a.N, a.Nout, a.S, E)),
            "stat_part": ("w", B(a.N * a.Nout * nsb * 3 * 4))}


def _pw_fwd2(a, E):
    st = B(a.N * a.Nout * _q("l3u_pw_stat_nsb", a.K, a.Nout, a.S) * 3 * 4)
    out = {}
    for s in "ab":
        ns = lambda n: getattr(a, n + s + "_ns")  # noqa: E731
        out.update({"x" + s: ("r", T(ns("x"), a.N, a.K, a.S, E)), "w" + s: ("r", B(a.Nout * a.K * 4)),
                    "y" + s: ("w", T(ns("y"), a.N, a.Nout, a.S, E)), "stat_" + s: ("w", st)})
    return out


def _dwpw_fwd(a, E):
    S = a.D * a.H * a.W
    st = B(a.N * a.Nout * _q("l3u_dwpw_stat_nsb", a.K, a.Nout, a.D, a.H, a.W) * 3 * 4)
    return {"x": ("r", T(a.x_ns, a.N, a.K, S, E)), "w_dw": ("r", B(a.K * 27 * 4)),
            "rec": ("r", B(a.N * a.K * 32)), "src": _src(a.N, a.K),
            "w_pw": ("r", B(a.Nout * a.K * 4)), "y": ("w", T(a.y_ns, a.N, a.Nout, S, E)),
            "y_stat": ("w", st), "w_sc": ("r", B(a.Nout * a.K * 4)),
            "r": ("w", T(a.r_ns, a.N, a.Nout, S, E)), "r_stat": ("w", st),
            "z": ("w", T(a.z_ns, a.N, a.K, S, E))}


def _pw_bwd_weight(a, E):
    P = _q("l3u_pw_bwd_weight_nparts", a.N, a.S)
    return {"dy": ("r", T(a.dy_ns, a.N, a.J, a.S)), "x": ("r", T(a.x_ns, a.N, a.K, a.S, E)),
            "part": ("w", B(P * a.J * a.K * 4))}


def _pw_part(a, K):
    return B(_q("l3u_pw_bwd_nparts", a.N, a.J, K, a.S) * a.J * K * 4)


def _pw_bwd(a, E):
    return {"dy": ("r", T(a.dy_ns, a.N, a.J, a.S)), "y": ("r", T(a.y_ns, a.N, a.J, a.S, E)),
            "rec": ("r", B(a.N * a.J * 32)), "in_part": ("r", B(a.J * a.N * a.npart * 2 * 8)),
            "x": ("r", T(a.x_ns, a.N, a.K, a.S, E)), "w": ("r", B(a.J * a.K * 4)),
            "dx": (_acc(a.accumulate), T(a.dx_ns, a.N, a.K, a.S)), "part": ("w", _pw_part(a, a.K))}


def _pw_bwd2(a, E):
    out = {}
    for s in "ab":
        g = lambda n: getattr(a, n)  # noqa: E731
        K = g("K" + s)
        out.update({"dy" + s: ("r", T(g(f"dy{s}_ns"), a.N, a.J, a.S)),
                    "x" + s: ("r", T(g(f"x{s}_ns"), a.N, K, a.S, E)), "w" + s: ("r", B(a.J * K * 4)),
                    "dx" + s: (_acc(g("acc_" + s)), T(g(f"dx{s}_ns"), a.N, K, a.S)),
                    "part_" + s: ("w", _pw_part(a, K))})
    return out


def _dout(a, form, C, S):
    """The three forms of a block's output gradient (plain, rank-1 dz, skip + pooled)."""
    if form == "r1":
        return {"dz": ("r", T(a.dz_ns, a.N, 1, S)), "dscale": ("r", B(C * 4))}
    if form == "up":
        return {"dskip": ("r", T(a.dskip_ns, a.N, C, S)), "dpool": ("r", T(a.dpool_ns, a.N, C, S // 8)),
                "idx": ("r", B(a.N * C * (S // 8)))}
    return {"dout": ("r", T(a.dout_ns, a.N, C, S))}


def _pw_bwd_tail(form):
    def fn(a, E):
        if form == "up":
            a.S = a.D * a.H * a.W
        out = _dout(a, form, a.J, a.S)
        out.update({"out": ("r", T(a.out_ns, a.N, a.J, a.S, E)), "yr": ("r", T(a.yr_ns, a.N, a.J, a.S, E)),
                    "rec": ("r", B(a.N * a.J * 32)),
                    "tail_part": ("r", B(a.J * a.N * a.npart * 3 * 8)),
                    "x": ("r", T(a.x_ns, a.N, a.K, a.S, E)), "w": ("r", B(a.J * a.K * 4)),
                    "dx": (_acc(a.accumulate), T(a.dx_ns, a.N, a.K, a.S)),
                    "part": ("w", _pw_part(a, a.K))})
        return out
    return fn


def _pw_bwd_tail_pair(a, E):
    out = {"dout": ("r", T(a.dout_ns, a.N, 1 if a.dscale else a.J, a.S)),
           "dscale": ("r", B(a.J * 4)), "dpool": ("r", T(a.dpool_ns, a.N, a.J, a.S // 8)),
           "idx": ("r", B(a.N * a.J * (a.S // 8))), "out": ("r", T(a.out_ns, a.N, a.J, a.S, E)),
           "tail_part": ("r", B(a.J * a.N * a.npart * 3 * 8))}
    for s in "ab":
        g = lambda n: getattr(a, n)  # noqa: E731
        K = g("K" + s)
        out.update({"yr" + s: ("r", T(g(f"yr{s}_ns"), a.N, a.J, a.S, E)), "rec" + s: ("r", B(a.N * a.J * 32)),
                    "x" + s: ("r", T(g(f"x{s}_ns"), a.N, K, a.S, E)), "w" + s: ("r", B(a.J * K * 4)),
                    "dx" + s: (_acc(g("acc_" + s)), T(g(f"dx{s}_ns"), a.N, K, a.S)),
                    "part_" + s: ("w", _pw_part(a, K))})
    return out


def _in_finalize(a, E):
    return {"stat_part": ("r", B(a.N * a.C * a.nsb * 3 * 4)), "gamma": ("r", B(a.C * 4)),
            "beta": ("r", B(a.C * 4)), "step": ("r", B(4)), "rec": ("w", B(a.N * a.C * 32))}


def _tail_ops(a, E, S):
    return {"out": ("r", T(a.out_ns, a.N, a.C, S, E)), "y2": ("r", T(a.y2_ns, a.N, a.C, S, E)),
            "rec2": ("r", B(a.N * a.C * 32)), "r": ("r", T(a.r_ns, a.N, a.C, S, E)),
            "rec_r": ("r", B(a.N * a.C * 32))}


def _norm_act_fwd(pool):
    def fn(a, E):
        S = a.D * a.H * a.W if pool else a.S
        out = _tail_ops(a, E, S)
        out.update({"src2": _src(a.N, a.C), "src_r": _src(a.N, a.C),
                    "out": ("w", T(a.out_ns, a.N, a.C, S, E))})
        if pool:
            out.update({"pooled": ("w", T(a.pooled_ns, a.N, a.C, S // 8, E)),
                        "idx": ("w", B(a.N * a.C * (S // 8)))})
        return out
    return fn


def _norm_act_bwd(form, reduce, apply):
    def fn(a, E):
        S = a.D * a.H * a.W if form == "up" else a.S
        out = _dout(a, form, a.C, S)
        out.update(_tail_ops(a, E, S))
        nb = _q("l3u_norm_act_nblocks", S)
        out["part"] = ("w" if reduce else "r", B(a.C * a.N * nb * 3 * 8))
        if apply:
            out.update({"dy2": ("w", T(a.dy2_ns, a.N, a.C, S)), "dr": ("w", T(a.dr_ns, a.N, a.C, S))})
        return out
    return fn


def _in_bwd_apply(a, E):
    return {"dpre": ("r", T(a.dpre_ns, a.N, a.C, a.S)), "y": ("r", T(a.y_ns, a.N, a.C, a.S, E)),
            "rec": ("r", B(a.N * a.C * 32)), "in_part": ("r", B(a.C * a.N * a.npart * 2 * 8)),
            "dy": ("w", T(a.dy_ns, a.N, a.C, a.S))}


def _maxpool2_fwd(a, E):
    S, So = a.D * a.H * a.W, (a.D // 2) * (a.H // 2) * (a.W // 2)
    return {"x": ("r", T(a.x_ns, a.N, a.C, S, E)), "y": ("w", T(a.y_ns, a.N, a.C, So, E)),
            "idx": ("w", B(a.N * a.C * So))}


def _maxpool2_bwd(a, E):
    S, So = a.D * a.H * a.W, (a.D // 2) * (a.H // 2) * (a.W // 2)
    return {"dy": ("r", T(a.dy_ns, a.N, a.C, So)), "idx": ("r", B(a.N * a.C * So)),
            "add": ("r", T(a.add_ns, a.N, a.C, S)), "dx": ("w", T(a.dx_ns, a.N, a.C, S))}


def _convt_fwd(a, E):
    S = a.D * a.H * a.W
    return {"x": ("r", T(a.x_ns, a.N, a.Ci, S, E)), "w": ("r", B(a.Ci * a.Co * 8 * 4)),
            "bias": ("r", B(a.Co * 4)), "out": ("w", T(a.out_ns, a.N, a.Co, 8 * S, E))}


def _convt_bwd(fused):
    def fn(a, E):
        S = a.D * a.H * a.W
        P = _q("l3u_convt_bwd_fused_nparts", a.N, a.Ci, a.Co, a.D, a.H, a.W) if fused else \
            _q("l3u_pw_bwd_weight_nparts", a.N, S)
        return {"dy": ("r", T(a.dy_ns, a.N, a.Co, 8 * S)), "x": ("r", T(a.x_ns, a.N, a.Ci, S, E)),
                "w": ("r", B(a.Ci * a.Co * 8 * 4)), "dx": ("w", T(a.dx_ns, a.N, a.Ci, S)),
                "wpart": ("w", B(P * a.Ci * a.Co * 8 * 4)), "bpart": ("w", B(P * a.Co * 4))}
    return fn


def _outconv_fwd(cols):
    def fn(a, E):
        nb = _q("l3u_outconv_nblocks", a.S)
        return {"h": ("r", T(a.h_ns, a.N, a.C, a.S, E)), "w": ("r", B(a.C * 4)), "b": ("r", B(4)),
                "p": ("w", B(a.N * a.S * 4)), "t": ("r", B(a.N * a.S * 4)),
                "ftl_part": ("w", B(a.N * nb * cols * 4))}
    return fn


def _outconv_bwd(cols, dz):
    def fn(a, E):
        nb = _q("l3u_outconv_nblocks", a.S)
        return {"dp": ("r", B(a.N * a.S * 4)), "p": ("r", B(a.N * a.S * 4)),
                "t": ("r", B(a.N * a.S * 4)), "sums": ("r", B(cols * 8)),
                "loss_part": ("r", B(getattr(a, "loss_nparts", 0) * cols * 4)),
                "gscale": ("r", B(4)), "h": ("r", T(a.h_ns, a.N, a.C, a.S, E)), "w": ("r", B(a.C * 4)),
                "dh": ("w", T(a.dh_ns, a.N, 1 if dz else a.C, a.S)),
                "part": ("w", B(a.N * nb * (a.C + 1) * 8)), "loss": ("w", B(4))}
    return fn


def _loss_sums(cols):
    return lambda a, E: {"p": ("r", B(a.numel * 4)), "t": ("r", B(a.numel * 4)),
                         "part": ("w", B(_q("l3u_ftl_nblocks", a.numel) * cols * 4)),
                         "sums": ("w", B(cols * 8))}


def _loss_reduce(cols):
    return lambda a, E: {"part": ("r", B(a.nparts * cols * 4)), "sums": ("w", B(cols * 8))}


def _loss_value(cols):
    return lambda a, E: {"sums": ("r", B(cols * 8)), "loss": ("w", B(4))}


def _loss_bwd(cols):
    return lambda a, E: {"p": ("r", B(a.numel * 4)), "t": ("r", B(a.numel * 4)),
                         "sums": ("r", B(cols * 8)), "gscale": ("r", B(4)),
                         "g": ("w", B(a.numel * 4))}


def _front_fwd(a, E):
    S = a.D * a.H * a.W
    st = B(a.N * a.C * _q("l3u_front_nblocks", S) * 3 * 4)
    return {"x": ("r", T(a.x_ns, a.N, 1, S)), "w_dw": ("r", B(27 * 4)), "w1": ("r", B(a.C * 4)),
            "wr": ("r", B(a.C * 4)), "z1": ("w", B(a.N * S * E)), "y1": ("w", B(a.N * a.C * S * E)),
            "r": ("w", B(a.N * a.C * S * E)), "stat1": ("w", st), "statr": ("w", st),
            "x_copy": ("w", B(a.N * S * E))}


def _gconv3_fwd(a, E):
    S = a.D * a.H * a.W
    nb = _q("l3u_gconv3_nblocks", S)
    return {"x": ("r", T(a.x_ns, a.N, a.Cin, S)), "w": ("r", B(a.Cout * (a.Cin // a.G) * 27 * 4)),
            "rec": ("r", B(a.N * a.Cin * 32)), "y": ("w", T(a.y_ns, a.N, a.Cout, S)),
            "stat_part": ("w", B(a.N * a.Cout * nb * 3 * 4))}


def _gconv3_bwd_data(a, E):
    S = a.D * a.H * a.W
    nb = _q("l3u_gconv3_nblocks", S)
    return {"dy": ("r", T(a.dy_ns, a.N, a.Cout, S)), "w": ("r", B(a.Cout * (a.Cin // a.G) * 27 * 4)),
            "rec": ("r", B(a.N * a.Cin * 32)), "ep": ("r", T(a.ep_ns, a.N, a.Cin, S)),
            "dx": (_acc(a.accumulate), T(a.dx_ns, a.N, a.Cin, S)),
            "in_part": ("w", B(a.Cin * a.N * nb * 2 * 8))}


def _gconv3_bwd_weight(a, E):
    S = a.D * a.H * a.W
    P = _q("l3u_gconv3_wgrad_nparts", a.N, S)
    return {"dy": ("r", T(a.dy_ns, a.N, a.Cout, S)), "x": ("r", T(a.x_ns, a.N, a.Cin, S)),
            "rec": ("r", B(a.N * a.Cin * 32)),
            "part": ("w", B(P * a.Cout * (a.Cin // a.G) * 27 * 4))}


def _box_copy(a, E):
    return {"src": ("r", T(a.src_ns, a.N, a.C, a.sd * a.sh * a.sw, E)),
            "dst": ("w", T(a.dst_ns, a.N, a.C, a.dd * a.dh * a.dw, E))}


def _adamw_tick(a, E):
    n = B(a.numel * 4)
    return {"p": ("rw", n), "g": ("r", n), "m": ("rw", n), "v": ("rw", n), "lr": ("r", B(4)),
            "step": ("rw", B(4)), "ticket": ("rw", B(4)), "counter2": ("rw", B(4))}


_FAM = "w_ftl alpha beta gamma smooth_ftl w_bce global_numel w_dice smooth_dice"
_FTL = "alpha beta gamma smooth"
_OC_TAIL = "gscale h h_ns w dh dh_ns part loss N C S"
_TAIL = "out out_ns yr yr_ns rec tail_part npart sel x x_ns w dx dx_ns accumulate part N J K"
_NA = "out out_ns y2 y2_ns rec2 r r_ns rec_r part"
_NA_FWD = "y2 y2_ns rec2 src2 r r_ns rec_r src_r shortcut out out_ns"
_UP = "dskip dskip_ns dpool dpool_ns idx"

TABLE = {
    "l3u_counter_add": ("counter value", lambda a, E: {"counter": ("rw", B(4))}, ()),
    "l3u_cast_f32_bf16": ("x y n", lambda a, E: {"x": ("r", B(a.n * 4)), "y": ("w", B(a.n * 2))}, ()),
    "l3u_cast_bf16_f32": ("x y n", lambda a, E: {"x": ("r", B(a.n * 2)), "y": ("w", B(a.n * 4))}, ()),
    "l3u_dw3_fwd": ("x x_ns w rec src y y_ns N C D H W", _dw3_fwd, ()),
    "l3u_dw3_bwd": ("dz dz_ns x x_ns w rec dx dx_ns accumulate dw_part in_part N C D H W",
                    _dw3_bwd, ()),
    "l3u_pw_fwd": ("x x_ns w w_layout bias y y_ns accumulate stat_part N K Nout S", _pw_fwd, ()),
    "l3u_pw_fwd2": ("xa xa_ns wa ya ya_ns stat_a xb xb_ns wb yb yb_ns stat_b N K Nout S",
                    _pw_fwd2, ()),
    "l3u_dwpw_fwd": ("x x_ns w_dw rec src w_pw y y_ns y_stat w_sc r r_ns r_stat z z_ns N K Nout "
                     "D H W", _dwpw_fwd, ()),
    "l3u_pw_bwd_weight": ("dy dy_ns x x_ns part N J K S", _pw_bwd_weight, ()),
    "l3u_pw_bwd": ("dy dy_ns y y_ns rec in_part npart x x_ns w dx dx_ns accumulate part N J K S",
                   _pw_bwd, ()),
    "l3u_pw_bwd2": ("dya dya_ns xa xa_ns wa dxa dxa_ns acc_a part_a Ka dyb dyb_ns xb xb_ns wb dxb "
                    "dxb_ns acc_b part_b Kb N J S", _pw_bwd2, ()),
    "l3u_pw_bwd_tail": ("dout dout_ns " + _TAIL + " S", _pw_bwd_tail(""), ()),
    "l3u_pw_bwd_tail_r1": ("dz dz_ns dscale " + _TAIL + " S", _pw_bwd_tail("r1"), ()),
    "l3u_pw_bwd_tail_up": (_UP + " " + _TAIL + " D H W", _pw_bwd_tail("up"), ()),
    "l3u_pw_bwd_tail_pair": (
        "dout dout_ns dscale dpool dpool_ns idx Hf Wf out out_ns tail_part npart "
        "yra yra_ns reca xa xa_ns wa dxa dxa_ns acc_a part_a Ka sel_a "
        "yrb yrb_ns recb xb xb_ns wb dxb dxb_ns acc_b part_b Kb sel_b N J S", _pw_bwd_tail_pair, ()),
    "l3u_in_finalize": ("stat_part nsb gamma beta drop_p seed step layer rec N C", _in_finalize, ()),
    "l3u_norm_act_fwd": (_NA_FWD + " N C S", _norm_act_fwd(False), ()),
    "l3u_norm_act_pool_fwd": (_NA_FWD + " pooled pooled_ns idx N C D H W", _norm_act_fwd(True), ()),
    "l3u_norm_act_bwd_reduce": ("dout dout_ns " + _NA + " N C S",
                                _norm_act_bwd("", True, False), ()),
    "l3u_norm_act_bwd_reduce_r1": ("dz dz_ns dscale " + _NA + " N C S",
                                   _norm_act_bwd("r1", True, False), ()),
    "l3u_norm_act_bwd_reduce_up": (_UP + " " + _NA + " N C D H W",
                                   _norm_act_bwd("up", True, False), ()),
    "l3u_norm_act_bwd_apply": ("dout dout_ns " + _NA + " dy2 dy2_ns dr dr_ns N C S",
                               _norm_act_bwd("", False, True), ()),
    "l3u_norm_act_bwd": ("dout dout_ns " + _NA + " dy2 dy2_ns dr dr_ns N C S",
                         _norm_act_bwd("", True, True), ()),
    "l3u_norm_act_bwd_up": (_UP + " " + _NA + " dy2 dy2_ns dr dr_ns N C D H W",
                            _norm_act_bwd("up", True, True), ()),
    # the engine applies the inner InstanceNorm backward in place (dy == dpre): element-wise
    "l3u_in_bwd_apply": ("dpre dpre_ns y y_ns rec in_part npart dy dy_ns N C S", _in_bwd_apply,
                         (("dpre", "dy"),)),
    "l3u_maxpool2_fwd": ("x x_ns y y_ns idx N C D H W", _maxpool2_fwd, ()),
    "l3u_maxpool2_bwd": ("dy dy_ns idx add add_ns dx dx_ns N C D H W", _maxpool2_bwd, ()),
    "l3u_convt_fwd": ("x x_ns w bias out out_ns N Ci Co D H W", _convt_fwd, ()),
    "l3u_convt_bwd": ("dy dy_ns x x_ns w dx dx_ns wpart bpart N Ci Co D H W", _convt_bwd(False), ()),
    "l3u_convt_bwd_fused": ("dy dy_ns x x_ns w dx dx_ns wpart bpart N Ci Co D H W",
                            _convt_bwd(True), ()),
    "l3u_outconv_fwd": ("h h_ns w b p t ftl_part N C S", _outconv_fwd(3), ()),
    "l3u_outconv_fwd_loss4": ("h h_ns w b p t ftl_part N C S", _outconv_fwd(4), ()),
    "l3u_outconv_bwd": (f"dp p t sums {_FTL} {_OC_TAIL}", _outconv_bwd(3, False), ()),
    "l3u_outconv_bwd_dz": (f"dp p t sums {_FTL} {_OC_TAIL}", _outconv_bwd(3, True), ()),
    "l3u_outconv_bwd_ftl": (f"p t loss_part loss_nparts {_FTL} {_OC_TAIL}",
                            _outconv_bwd(3, False), ()),
    "l3u_outconv_bwd_ftl_dz": (f"p t loss_part loss_nparts {_FTL} {_OC_TAIL}",
                               _outconv_bwd(3, True), ()),
    "l3u_outconv_bwd_loss4": (f"p t sums {_FAM} {_OC_TAIL}", _outconv_bwd(4, False), ()),
    "l3u_outconv_bwd_loss4_dz": (f"p t sums {_FAM} {_OC_TAIL}", _outconv_bwd(4, True), ()),
    "l3u_outconv_bwd_loss4p": (f"p t loss_part loss_nparts {_FAM} {_OC_TAIL}",
                               _outconv_bwd(4, False), ()),
    "l3u_outconv_bwd_loss4p_dz": (f"p t loss_part loss_nparts {_FAM} {_OC_TAIL}",
                                  _outconv_bwd(4, True), ()),
    "l3u_ftl_sums": ("p t numel part sums", _loss_sums(3), ()),
    "l3u_ftl_reduce": ("part nparts sums", _loss_reduce(3), ()),
    "l3u_ftl_loss": (f"sums {_FTL} loss", _loss_value(3), ()),
    "l3u_ftl_bwd": (f"p t numel sums {_FTL} gscale through_sigmoid g", _loss_bwd(3), ()),
    "l3u_loss4_sums": ("p t numel part sums", _loss_sums(4), ()),
    "l3u_loss4_reduce": ("part nparts sums", _loss_reduce(4), ()),
    "l3u_loss4_value": (f"sums {_FAM} loss", _loss_value(4), ()),
    "l3u_loss4_bwd": (f"p t numel sums {_FAM} gscale through_sigmoid g", _loss_bwd(4), ()),
    "l3u_front_fwd": ("x x_ns w_dw w1 wr z1 y1 r stat1 statr x_copy N C D H W", _front_fwd, ()),
    "l3u_gconv3_fwd": ("x x_ns w rec y y_ns stat_part N Cin Cout G D H W", _gconv3_fwd, ()),
    "l3u_gconv3_bwd_data": ("dy dy_ns w rec ep ep_ns dx dx_ns accumulate in_part N Cin Cout G D H W",
                            _gconv3_bwd_data, ()),
    "l3u_gconv3_bwd_weight": ("dy dy_ns x x_ns rec part N Cin Cout G D H W", _gconv3_bwd_weight, ()),
    "l3u_box_copy": ("src src_ns sd sh sw dst dst_ns dd dh dw oz oy ox N C", _box_copy, ()),
    "l3u_adamw_tick": ("p g m v numel lr beta1 beta2 eps weight_decay step grad_scale ticket "
                       "counter2", _adamw_tick, ()),
}
_SEG = "src items nitems dst"
_SEG_ADAMW = ("src items nitems g p m v lr beta1 beta2 eps weight_decay step grad_scale ticket "
              "counter2")
SEGMENTS = {"l3u_reduce_segments": _SEG, "l3u_reduce_segments_adamw": _SEG_ADAMW}


def base_name(name):
    """The table's name of an entry point: a _bf16 twin is its fp32 entry."""
    return name[:-5] if name.endswith("_bf16") and name[:-5] in nat.BF16_TWINS else name


def has_entry(name):
    b = base_name(name)
    return b in TABLE or b in SEGMENTS


def _merge(lo, hi):
    """Interval bounds (arrays) -> ascending disjoint [(lo, hi)], touching ones joined."""
    import numpy as np
    if len(lo) == 0:
        return []
    order = np.argsort(lo, kind="stable")
    lo, hi = lo[order], np.maximum.accumulate(hi[order])
    first = np.concatenate(([True], lo[1:] > hi[:-1]))
    last = np.concatenate((first[1:], [True]))
    return list(zip(lo[first].tolist(), hi[last].tolist()))


def _segments(name, a, items_of):
    """l3u_reduce_segments[_adamw]: what the item table {src_off, count, istride, tstride, len,
    dst_off, accumulate, f64} addresses.  fp64 sources count doubles from the same base."""
    import numpy as np
    rows = items_of(a.items, a.nitems)
    src, dst = ([], []), {0: ([], []), 1: ([], [])}
    for so, cnt, ist, tst, ln, do, acc, f64 in rows:
        if tst == 1:     # one run of len elements per partial
            lo = so + np.arange(cnt, dtype=np.int64) * ist
            hi = lo + ln
        else:
            lo = (so + np.arange(cnt, dtype=np.int64)[:, None] * ist
                  + np.arange(ln, dtype=np.int64)[None, :] * tst).ravel()
            hi = lo + 1
        k = 8 if f64 else 4
        src[0].append(lo * k)
        src[1].append(hi * k)
        dst[1 if acc else 0][0].append(np.array([4 * do]))
        dst[1 if acc else 0][1].append(np.array([4 * (do + ln)]))
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, dtype=np.int64)  # noqa: E731
    ivs = lambda p: _merge(cat(p[0]), cat(p[1]))  # noqa: E731
    out = {"src": [("r", ivs(src))], "items": [("r", B(a.nitems * 64))]}
    gname = "dst" if name == "l3u_reduce_segments" else "g"
    out[gname] = [("w", ivs(dst[0])), ("rw", ivs(dst[1]))]
    if name == "l3u_reduce_segments_adamw":
        upd = ivs((dst[0][0] + dst[1][0], dst[0][1] + dst[1][1]))
        out.update({"p": [("rw", upd)], "m": [("rw", upd)], "v": [("rw", upd)], "lr": [("r", B(4))],
                    "step": [("rw", B(4))], "ticket": [("rw", B(TICKET_INTS * 4))],
                    "counter2": [("rw", B(4))]})
    return out


def footprints(name, args, items_of=None):
    """[Operand] of the call `name(*args)` (args with the trailing stream), or None when the
    entry point has no table entry.  A NULL pointer yields an operand without intervals."""
    b = base_name(name)
    E = 2 if b != name else 4
    ops = []
    if b in SEGMENTS:
        a = _A(SEGMENTS[b], args)
        for arg, decl in _segments(b, a, items_of).items():
            i = a.index[arg]
            for role, ivs in decl:
                if ivs:
                    ops.append(Operand(i, None, args[i], role, ivs if args[i] else []))
        return ops
    if b not in TABLE:
        return None
    names, fn, _ = TABLE[b]
    a = _A(names, args)
    for arg, decl in fn(a, E).items():
        if arg not in a.index:
            continue    # (an operand of a sibling form: loss_part of the sums forms)
        i = a.index[arg]
        v = args[i]
        if callable(decl):   # an l3u_norm_src argument: its pointer fields
            if v is None:
                continue
            if not isinstance(v, ctypes._Pointer):
                raise TypeError(f"{name} argument {i} ({arg}): expected an l3u_norm_src pointer")
            s = v.contents
            for field, (role, ivs) in decl(s).items():
                p = getattr(s, field)
                ops.append(Operand(i, field, p or None, role, ivs if p else []))
            continue
        role, ivs = decl
        ops.append(Operand(i, None, v or None, role, ivs if v else []))
    for o in ops:
        if any(lo >= hi for lo, hi in o.ivs) or any(p[1] > q[0] for p, q in zip(o.ivs, o.ivs[1:])):
            raise ValueError(f"{name} argument {o.arg}: intervals {o.ivs[:3]}... overlap or are "
                             "empty (a batch stride below one sample?)")
    return ops


def inplace_pairs(name):
    """{frozenset((arg index, arg index))}: operand pairs the table allows to overlap."""
    b = base_name(name)
    if b not in TABLE:
        return set()
    names, _, pairs = TABLE[b]
    idx = {n: i for i, n in enumerate(names.split())}
    return {frozenset((idx[x], idx[y])) for x, y in pairs}
