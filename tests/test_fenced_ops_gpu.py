"""The kernel-level tests again, every `_native.call` fenced: no access outside the operands.

An autouse fixture installs tests/fenced.py round each re-exported test: every C-ABI call then
runs on guarded, poisoned shadow copies of its allocations, laid out by the footprint table of
tests/footprints.py (include/l3u.h as data), and the test's own fp64 comparisons run on the
fenced result.  The case tables are the source modules' own (ragged S, W % 4 != 0, less than one
chunk, partial tiles, strided concat halves, rank-1 operands, 4-byte-aligned storage); nothing is
added to them.

Re-exported: every test of test_ops_gpu and test_dwpw_gpu, those of test_tail_bwd_gpu but one; the
kernel tests of test_gconv_gpu (test_gconv3_*), the twin tests and test_casts of test_bf16_gpu, the
stand-alone and out_conv kernel tests of test_loss_family_gpu, and those of test_step_tail_gpu but
two (the 3000-item launch and the 2601-item ticket cases included: 0.4 s and 0.7 s fenced).

Left out (they reach the library under graph capture, through a whole model / TrainStep whose
launches the engine-level tests below and tests/test_footprints.py cover, or in a subprocess):
  test_step_tail_gpu: test_adamw_graph_replay_equals_eager (graph),
    test_reduce_refuses_misaligned_src (it launches through _native.query to read the error code)
  test_tail_bwd_gpu: test_tail_pair_rejects_dscale_with_dpool (it launches through
    _native.query to read the error code, which the fence does not replace)
  test_gconv_gpu: test_variant_model_matches_reference_golden,
    test_grouped_model_full_channels_matches_oracle (whole model),
    test_grouped_trainstep_graph_matches_eager (graph)
  test_bf16_gpu: test_bf16_model_vs_golden_and_fp32, test_bf16_autocast_selects_the_bf16_path,
    test_bf16_model_vs_bf16_storage_oracle (whole model),
    test_bf16_trainstep_graph_equals_eager_and_tracks_fp32,
    test_bf16_trainstep_bs4_48_vs_bf16_storage_oracle (TrainStep, graph)
  test_loss_family_gpu: test_dropin_modules_forward_backward_and_graph (graph),
    test_trainstep_matches_fp64_oracle, test_trainstep_losses_differ,
    test_trainstep_eager_equals_graph_replay, test_trainstep_combined_agrees_with_autograd_dropin,
    test_trainstep_focal_tversky_config_is_the_old_path,
    test_trainstep_bf16_storage_runs_the_twins (TrainStep, graph),
    test_trainstep_combined_two_ranks (subprocess),
    test_fast_trainer_runs_combined_loss_on_the_graph_step (trainer loop, graph)

End guards only: none (every launch entry point these modules name has a footprint entry; the
data-path kernels are not reached from here).

The harness tests itself on four fake entry points written with plain torch ops on the shadow
pointers: a well-behaved one passes, a store one element past the output, a load from before the
input that reaches the result, and a store into a read-only operand are each reported with their
argument and offset.  The same on a written footprint of 600 one-element runs (the one-pass mask
of fenced.py, which tests/test_footprints.py holds equal to the run-by-run loop on the CPU): a
store into a gap between the runs and a gap's value carried into an output are reported.

The engine-level test (not fenced, eager): one forward + loss + backward, then the same step again
with both arenas and every buffer the engine allocates filled with NaN first; output, loss and the
flat gradient must be finite and bitwise the first run's.  With the read-before-write check of
tests/test_footprints.py this shows that no launch depends on memory nobody wrote in the step.

Measured on one MI355X, 2026-10-20, one pytest process each on the same box: the 468 re-exported
cases fenced 24.7 s wall (1514 fenced calls, all with a footprint entry, 12.7 GiB shadowed in all;
slowest case 1.1 s, test_dw3_bwd at 4 x 16 x 48^3), the same 468 cases unfenced in their own
modules 23.0 s.  No violation was found in any of them, nor by the engine-level test.  With the
tail bound of csrc/misc.hip cast_kernel moved by one (`t < n + 1`, a scratch build): the plain
test_bf16_gpu.test_casts passes, the fenced one fails (l3u_cast_bf16_f32 argument 1, byte +4004).
2026-10-21, with test_step_tail_gpu's 233 cases added (strided reduction items have a footprint of
up to 240 000 one-element runs; fenced.py masks more than 256 runs in one pass on the host): the
701 re-exported cases fenced 34.3 s (1990 fenced calls, 13.7 GiB shadowed), of which the 233 new
ones 12.9 s (476 calls, 1.0 GiB; slowest 0.73 s) against 5.2 s unfenced in their own module.
"""
import pytest
import torch

import fenced
import footprints as fp
from test_bf16_gpu import (test_casts, test_convt_twin, test_dw3_bwd_twin,  # noqa: F401
                           test_dw3_fwd_twin, test_front_twin, test_norm_act_pool_and_maxpool_twins,
                           test_norm_act_twins, test_outconv_dz_twins, test_outconv_twin,
                           test_pw_bwd_tail_twin, test_pw_bwd_twin, test_pw_fwd2_twin,
                           test_pw_fwd_twin, test_tail_family_twins)
from test_dwpw_gpu import test_dwpw_equals_unfused, test_dwpw_record_in_kernel  # noqa: F401
from test_gconv_gpu import (test_gconv3_bwd, test_gconv3_fwd,  # noqa: F401
                            test_gconv3_rejects_bad_groups)
from test_loss_family_gpu import (test_focal_tversky_member_equals_ftl_kernels,  # noqa: F401
                                  test_outconv_loss4,
                                  test_standalone_kernels_match_reference_golden)
from test_ops_gpu import (test_adamw_tick_matches_torch, test_box_copy_pad_and_crop,  # noqa: F401
                          test_convt_bwd_fused, test_convt_bwd_onepass, test_convt_fwd_fused,
                          test_dw3_bwd, test_dw3_bwd_rank1_input, test_dw3_fwd,
                          test_dw3_fwd_inkernel_finalize, test_dw3_fwd_rank1_input, test_front_fwd,
                          test_ftl_golden, test_in_bwd_apply, test_in_finalize_and_dropout,
                          test_maxpool, test_norm_act_bwd_one_launch_equals_pair,
                          test_norm_act_bwd_up_equals_maxpool_bwd_then_one_launch,
                          test_norm_act_fwd_bwd, test_norm_act_fwd_rank1_r, test_norm_act_pool_fwd,
                          test_outconv, test_outconv_ftl_fused, test_pw_bwd2_equals_two_calls,
                          test_pw_bwd_fused, test_pw_bwd_k1_rank1_y, test_pw_bwd_matches_unfused,
                          test_pw_bwd_tail_equals_apply_then_pw_bwd, test_pw_bwd_weight,
                          test_pw_fwd, test_pw_fwd2_equals_two_pw_fwd, test_reduce_segments)
from test_step_tail_gpu import (test_adamw_five_steps, test_adamw_lr_rewritten_on_the_device,  # noqa: F401
                                test_adamw_one_step, test_adamw_options,
                                test_adamw_scalar_path_equals_float4_path, test_counter_add,
                                test_fused_equals_two_launches, test_fused_tickets,
                                test_fused_tickets_many_items, test_reduce_3000_mixed_items, test_reduce_engine_items,
                                test_reduce_hand_lists,
                                test_reduce_near_misses_equal_the_float4_item,
                                test_reduce_order_of_additions)
from test_tail_bwd_gpu import (test_outconv_dz_forms, test_tail_bwd_column_splits,  # noqa: F401
                               test_tail_bwd_rank1_yr_vs_fp64, test_tail_bwd_strided_views,
                               test_tail_bwd_vs_fp64)

pytestmark = pytest.mark.gpu

TOTAL = {"tests": 0, "calls": 0, "tabled": 0, "mib": 0.0, "guards_only": set(), "unmapped": []}


@pytest.fixture(scope="module", autouse=True)
def fence_totals():
    yield
    print(f"\nfenced: {TOTAL['tests']} tests, {TOTAL['calls']} calls ({TOTAL['tabled']} with a "
          f"footprint entry), {TOTAL['mib']:.0f} MiB shadowed, end guards only: "
          f"{sorted(TOTAL['guards_only'])}, pointers in no allocator block: {TOTAL['unmapped']}")


@pytest.fixture(autouse=True)
def fenced_calls(request, cuda):
    """Every re-exported test runs inside the fence; this module's own tests install what they
    need themselves."""
    if request.function.__module__ == __name__:
        yield None
        return
    with fenced.fence() as f:
        yield f
    TOTAL["tests"] += 1
    TOTAL["calls"] += f.calls
    TOTAL["tabled"] += f.tabled
    TOTAL["mib"] += f.bytes_shadowed / 2 ** 20
    TOTAL["guards_only"] |= f.end_guards_only
    TOTAL["unmapped"] += f.unmapped
    # nothing in these modules hands the library memory that is not a torch allocation
    assert not f.unmapped, f"pointers in no allocator block: {f.unmapped}"


# ------------------------------------------------------------------ the harness on itself
def _f32_at(ptr, n):
    return fenced.view(ptr, 4 * n).view(torch.float32)


def _fake_good(src, dst, n, stream):
    _f32_at(dst, n).copy_(2 * _f32_at(src, n))


def _fake_past_the_end(src, dst, n, stream):
    _fake_good(src, dst, n, stream)
    _f32_at(dst + 4 * n, 1).fill_(1.0)            # one element past the output's end


def _fake_reads_before(src, dst, n, stream):
    _fake_good(src, dst, n, stream)
    _f32_at(dst + 8, 1).add_(_f32_at(src - 4, 1))  # the element before the input's start


def _fake_stores_input(src, dst, n, stream):
    _fake_good(src, dst, n, stream)
    _f32_at(src + 4, 1).fill_(0.0)                 # a store into the read-only operand


FAKES = {"l3u_fake_good": _fake_good, "l3u_fake_past_the_end": _fake_past_the_end,
         "l3u_fake_reads_before": _fake_reads_before, "l3u_fake_stores_input": _fake_stores_input}


@pytest.fixture
def fakes(monkeypatch):
    from light_unet import _native as nat
    entry = ("src dst n", lambda a, E: {"src": ("r", fp.B(4 * a.n)), "dst": ("w", fp.B(4 * a.n))}, ())
    for name in FAKES:
        monkeypatch.setitem(nat._SIGS, name, [nat.P, nat.P, nat.L, nat.P])
        monkeypatch.setitem(fp.TABLE, name, entry)
    return lambda name, *args: FAKES[name](*args)


# n = 100: the byte after the output is allocator slack; 128: it is the guard.  lead: the operands
# start that many floats into their allocation (0: what lies before them is the guard)
@pytest.mark.parametrize("n", [100, 128])
@pytest.mark.parametrize("lead", [0, 5])
def test_fence_reports_planted_violations(cuda, fakes, n, lead):
    from light_unet import _native as nat
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(lead + n, generator=gen).to(cuda)[lead:]
    ref = 2 * x.cpu()

    def run(name):
        y = torch.full((lead + n,), float("nan"), device=cuda)[lead:]
        with fenced.fence(call=fakes) as f:
            nat.call(name, x.data_ptr(), y.data_ptr(), n, 0)
        assert f.calls == 1 and f.tabled == 1 and not f.unmapped
        return y

    y = run("l3u_fake_good")
    assert torch.equal(y.cpu(), ref) and torch.equal(x.cpu() * 2, ref)
    with pytest.raises(fenced.FenceError) as e:
        run("l3u_fake_past_the_end")
    assert (e.value.entry, e.value.arg, e.value.offset) == ("l3u_fake_past_the_end", 1, 4 * n)
    assert "write outside" in e.value.kind
    with pytest.raises(fenced.FenceError) as e:
        run("l3u_fake_reads_before")
    assert (e.value.entry, e.value.arg, e.value.offset) == ("l3u_fake_reads_before", 1, 8)
    assert "poison value was read" in e.value.kind
    with pytest.raises(fenced.FenceError) as e:
        run("l3u_fake_stores_input")
    assert (e.value.entry, e.value.arg, e.value.offset) == ("l3u_fake_stores_input", 0, 4)
    assert "read-only" in e.value.kind
    # the caller's input is untouched by the refused calls (they ran on the shadow)
    assert torch.equal(x.cpu() * 2, ref)
    assert nat.call is not None and not isinstance(nat.call, fenced.Fence)


def _strided_good(src, dst, n, stream):
    _f32_at(dst, 2 * n)[0::2].copy_(2 * _f32_at(src, n))


def _strided_writes_gap(src, dst, n, stream):
    _strided_good(src, dst, n, stream)
    _f32_at(dst + 4 * (2 * 301 + 1), 1).fill_(1.0)           # the gap after output 301


def _strided_reads_gap(src, dst, n, stream):
    _strided_good(src, dst, n, stream)
    _f32_at(dst + 8 * 7, 1).add_(_f32_at(dst + 8 * 300 + 4, 1))   # a gap's value into output 7


def test_fence_reports_violations_in_a_strided_footprint(cuda, monkeypatch):
    """A written footprint of 600 one-element runs, more than fenced.MASK_LOOP_MAX, so the mask
    comes from the one-pass form that every fenced reduction item with a strided footprint gets:
    the gaps between the runs are poisoned and watched like everything else outside."""
    from light_unet import _native as nat
    n = 600
    assert n > fenced.MASK_LOOP_MAX
    strided = {"l3u_fake_strided_good": _strided_good,
               "l3u_fake_strided_writes_gap": _strided_writes_gap,
               "l3u_fake_strided_reads_gap": _strided_reads_gap}
    entry = ("src dst n", lambda a, E: {"src": ("r", fp.B(4 * a.n)),
                                        "dst": ("w", [(8 * i, 8 * i + 4) for i in range(a.n)])}, ())
    for name in strided:
        monkeypatch.setitem(nat._SIGS, name, [nat.P, nat.P, nat.L, nat.P])
        monkeypatch.setitem(fp.TABLE, name, entry)
    x = torch.randn(n, generator=torch.Generator().manual_seed(5)).to(cuda)

    def run(name):
        y = torch.full((2 * n,), -3.0, device=cuda)
        with fenced.fence(call=lambda nm, *a: strided[nm](*a)) as f:
            nat.call(name, x.data_ptr(), y.data_ptr(), n, 0)
        assert f.calls == 1 and f.tabled == 1 and not f.unmapped
        return y

    y = run("l3u_fake_strided_good")
    # the runs come back, the caller's gaps are as they were
    assert torch.equal(y[0::2], 2 * x) and bool((y[1::2] == -3.0).all())
    with pytest.raises(fenced.FenceError) as e:
        run("l3u_fake_strided_writes_gap")
    assert (e.value.entry, e.value.arg, e.value.offset) == \
        ("l3u_fake_strided_writes_gap", 1, 4 * (2 * 301 + 1))
    assert "write outside" in e.value.kind
    with pytest.raises(fenced.FenceError) as e:
        run("l3u_fake_strided_reads_gap")
    assert (e.value.entry, e.value.arg, e.value.offset) == ("l3u_fake_strided_reads_gap", 1, 8 * 7)
    assert "poison value was read" in e.value.kind


def test_fence_without_a_table_entry_guards_the_ends(cuda, fakes, monkeypatch):
    from light_unet import _native as nat
    for name in FAKES:
        monkeypatch.delitem(fp.TABLE, name)
    x = torch.randn(128, generator=torch.Generator().manual_seed(4)).to(cuda)
    y = torch.full((128,), float("nan"), device=cuda)
    with fenced.fence(call=fakes) as f:
        nat.call("l3u_fake_good", x.data_ptr(), y.data_ptr(), 128, 0)
        assert torch.equal(y, 2 * x)
        with pytest.raises(fenced.FenceError) as e:
            nat.call("l3u_fake_past_the_end", x.data_ptr(), y.data_ptr(), 128, 0)
        assert (e.value.arg, e.value.offset) == (1, 512)
    assert f.end_guards_only == {"l3u_fake_good", "l3u_fake_past_the_end"} and f.tabled == 0


def test_fence_refuses_graph_capture(cuda, fakes, monkeypatch):
    """Snapshots, copies and synchronisation cannot be captured: the fence raises before it does
    anything (the capture state is stubbed, nothing here runs under capture)."""
    from light_unet import _native as nat
    x = torch.zeros(128, device=cuda)
    y = torch.zeros(128, device=cuda)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with fenced.fence(call=fakes) as f:
        with pytest.raises(RuntimeError, match="graph capture"):
            nat.call("l3u_fake_good", x.data_ptr(), y.data_ptr(), 128, 0)
    assert f.calls == 0 and bool((y == 0).all())


# ------------------------------------------------------------------ engine-level poison
FTL = (0.7, 0.3, 0.75, 1e-6)
ENGINE_CASES = [("model_b2_32.npz", {}, torch.float32), ("model_b2_32.npz", {}, torch.bfloat16),
                ("model_g_b2_16.npz", dict(use_depthwise_separable=False, use_grouped=True, groups=8),
                 torch.float32)]


@pytest.mark.parametrize("fname,kw,adt", ENGINE_CASES,
                         ids=["dsep_fp32", "dsep_bf16", "grouped_fp32"])
def test_engine_step_depends_on_nothing_it_did_not_write(cuda, golden, monkeypatch, fname, kw, adt):
    import light_unet.engine as E
    from light_unet import _native as nat
    from light_unet.models.unet3d import Lightweight3DUNet
    z = golden(fname)
    enc = [int(c) for c in z["enc"]] if "enc" in z.files else [16, 32, 64, 128]
    m = Lightweight3DUNet(encoder_channels=enc, dropout_p=0.1, **kw)
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")})
    m = m.to(cuda).train()
    eng, flat = m.engine, m.flat_parameters().detach()
    eng.set_act_dtype(adt)
    x = torch.from_numpy(z["x"]).to(cuda)
    t = torch.from_numpy(z["target"]).to(cuda)
    N, S = x.shape[0], x[0].numel()
    nparts = N * nat.query("l3u_outconv_nblocks", S)
    counter = torch.tensor([5], dtype=torch.int32, device=cuda)
    nan = float("nan")

    def step():
        part = torch.full((nparts * 3,), nan, device=cuda)
        loss = torch.full((), nan, device=cuda)
        gflat = torch.full_like(flat, nan)
        head = E.LossHead(t, part, nparts, out=loss, ftl=FTL)
        p, sv = eng.forward(flat, x, training=True, dropout_p=0.1, counter=counter,
                            bump_counter=False, save=True, loss=head)
        eng.backward(flat, gflat, sv, None, need_dx=False, loss=head)
        torch.cuda.synchronize()
        return p.clone(), loss.clone(), gflat

    first = step()
    assert int(counter.item()) == 5
    for arena in eng._arenas.values():
        arena.fill_(nan)
    assert len(eng._arenas) == 2

    def poisoned(alloc):
        def make(*a, **k):
            out = alloc(*a, **k)
            # (the uint8 pooling indices get a valid slot, 7: they are compared, never trusted)
            return out.fill_(nan) if out.is_floating_point() else out.fill_(7)
        return make
    monkeypatch.setattr(eng, "_empty", poisoned(eng._empty), raising=False)
    monkeypatch.setattr(eng, "_f32", poisoned(eng._f32), raising=False)
    second = step()
    for what, a, b in zip(("output", "loss", "flat gradient"), first, second):
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), f"{what}: not finite"
        assert torch.equal(a, b), f"{what}: differs after poisoning by " \
                                  f"{(a - b).abs().max().item():.3e}"
