"""A fence round every `_native.call`: no access outside the operands it is given.

`fence()` is a context manager that replaces `light_unet._native.call` (the way
tools/launch_trace.Recorder.wrap and bench.StepRecorder.wrap replace it) and restores it on exit.
Every call made inside runs on shadow copies of the allocator blocks its pointers fall in:

    [ 4 KiB guard | copy of the whole block | 4 KiB guard ]

with the shadow at the block's address modulo 512 (alignment-dependent dispatch takes the same
path), one shadow per block (two pointers into one block keep their relation), and every byte that
is not payload set to a poison word, the quiet NaN 0x7fc5a5a5: the guards, the block's slack past
its requested size and, when tests/footprints.py has an entry for the call, every byte of the block
outside the declared footprints (the other half of a concat buffer, the gaps of a strided view).
After the call and a synchronise:
  - every byte outside the written footprints is bit-equal to before (the poison is intact and no
    read-only operand was stored to);
  - no poison word has appeared inside a written footprint (a poison value that was read and
    used; the callers' own fp64 comparisons catch the same through NaN);
  - the written footprints are copied back into the caller's block (the whole block without a
    table entry), so the caller's assertions run on the fenced result.
A violation raises FenceError naming the entry point, the argument index and the byte offset
relative to that operand (negative: before its start).

The shadowed call uses the same offsets inside a copy of the same block as the plain call, so it
reaches no address the plain call does not, whatever the table says: a wrong table is a failed
test, never a stray access.  No device code: raw addresses are viewed as torch tensors through
__cuda_array_interface__.  Not usable under graph capture (it raises there).

What it cannot see: a load that leaves the operand but is dropped by a select, and an access more
than 4 KiB outside the block.  4 KiB is four times the widest single-wave access of these kernels
(64 lanes x 16 B), and one 256-voxel fp32 block of the statistics partials.
"""
import bisect
import contextlib
import ctypes

import numpy as np
import torch

import footprints as fp
from light_unet import _native as nat

GUARD = 4096
POISON = 0x7FC5A5A5      # a quiet NaN with a payload; compared as an integer
MASK_LOOP_MAX = 256      # _mask: more runs than this are marked in one pass on the host


class FenceError(AssertionError):
    def __init__(self, kind, entry, arg, field, offset, detail=""):
        self.kind, self.entry, self.arg, self.field, self.offset = kind, entry, arg, field, offset
        where = f"argument {arg}" + (f".{field}" if field else "")
        super().__init__(f"fence: {entry} {where}: {kind} at byte offset {offset:+d} relative to "
                         f"the operand{detail}")


class _Raw:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1",
                                         "data": (int(ptr), False), "version": 2}


def view(ptr, nbytes):
    """The nbytes at device address ptr as a uint8 tensor (no copy)."""
    t = torch.as_tensor(_Raw(ptr, nbytes), device=torch.device("cuda", torch.cuda.current_device()))
    if t.data_ptr() != ptr or t.numel() != nbytes:
        raise RuntimeError("a raw-address view came back as a copy")
    return t


def _active_blocks():
    """[(address, size, requested size)] of the allocator's active blocks, ascending."""
    out = []
    for seg in torch.cuda.memory_snapshot():
        addr = seg["address"]
        for b in seg["blocks"]:
            if b["state"].startswith("active"):
                out.append((b.get("address", addr), b["size"], b.get("requested_size", b["size"])))
            addr += b["size"]
    out.sort()
    return out


def _mask(n, ivs, dev):
    if len(ivs) > MASK_LOOP_MAX:
        # many short runs (the strided footprint of a reduction item): one pass on the host
        # instead of one fill per run; the same mask as the loop below for any list of runs
        # (overlapping, touching, clipped at either end; an empty or inverted run covers nothing)
        b = np.clip(np.asarray(ivs, dtype=np.int64).reshape(-1, 2), 0, n)
        b = b[b[:, 0] < b[:, 1]]
        d = np.zeros(n + 1, dtype=np.int32)
        np.add.at(d, b[:, 0], 1)
        np.add.at(d, b[:, 1], -1)
        return torch.from_numpy(np.cumsum(d[:-1]) > 0).to(dev)
    m = torch.zeros(n, dtype=torch.bool, device=dev)
    for lo, hi in ivs:
        m[max(lo, 0):max(hi, 0)] = True
    return m


class _Shadow:
    """One block's shadow: `raw` = guard + block + guard, the block at raw[off : off + size]."""

    def __init__(self, addr, size, req, dev):
        self.addr, self.size, self.req = addr, size, req
        n = (GUARD + 512 + size + GUARD + 3) // 4 * 4
        self.raw = torch.empty(n, dtype=torch.uint8, device=dev)
        base = self.raw.data_ptr()
        assert base % 4 == 0
        self.off = GUARD + (addr - (base + GUARD)) % 512
        self.ptr = base + self.off
        assert self.ptr % 512 == addr % 512 and self.off + size + GUARD <= n
        self.operands = []    # (arg, field, ptr, role, [(lo, hi)] relative to ptr)

    def to_raw(self, ptr, ivs):
        d = ptr - self.addr + self.off
        return [(lo + d, hi + d) for lo, hi in ivs]


class Fence:
    def __init__(self, call=None):
        self.orig = call or nat.call
        self.calls = 0            # fenced calls
        self.tabled = 0           # ... of which with a footprint entry
        self.end_guards_only = set()
        self.unmapped = []        # (entry point, argument) pointers in no allocator block
        self.bytes_shadowed = 0
        self._blocks, self._stamp = None, None

    # ------------------------------------------------------------------ allocator blocks
    def _block_of(self, ptr, blocks):
        k = bisect.bisect_right(blocks, (ptr, float("inf"), 0)) - 1
        if k >= 0 and blocks[k][0] <= ptr < blocks[k][0] + blocks[k][1]:
            return blocks[k]
        return None

    @staticmethod
    def _allocator_stamp():
        s = torch.cuda.memory_stats()
        return tuple(s.get(k) for k in ("allocation.all.allocated", "allocation.all.freed",
                                        "segment.all.allocated", "segment.all.freed"))

    def _snapshot(self):
        # cached while the allocator has neither handed out nor taken back a block
        stamp = self._allocator_stamp()
        if self._blocks is None or stamp != self._stamp:
            self._blocks, self._stamp = _active_blocks(), stamp
        return self._blocks

    # ------------------------------------------------------------------ one call
    def __call__(self, name, *args):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the fence cannot run under graph capture")
        try:
            self._run(name, args)
        finally:
            # the shadows of _run are back with the allocator by now: the caller's blocks are as
            # the cached snapshot has them until the allocator's counters move again
            self._stamp = self._allocator_stamp()

    def _run(self, name, args):
        sig = nat._SIGS[name]
        dev = torch.device("cuda", torch.cuda.current_device())
        torch.cuda.synchronize()
        blocks = self._snapshot()

        def items_of(ptr, n):
            return view(ptr, n * 64).cpu().view(torch.int64).view(n, 8).tolist()

        ops = fp.footprints(name, args, items_of)
        self.calls += 1
        if ops is None:
            self.end_guards_only.add(name)
            # every pointer argument (and pointer field of a struct argument), whole blocks
            ops = []
            for i, a in enumerate(args[:-1]):
                if sig[i] is not nat.P or a is None:
                    continue
                if isinstance(a, ctypes._Pointer):
                    s = a.contents
                    ops += [fp.Operand(i, f, getattr(s, f) or None, None, [])
                            for f, t in s._fields_ if t is nat.P]
                elif isinstance(a, int) and a:
                    ops.append(fp.Operand(i, None, a, None, []))
            tabled = False
        else:
            self.tabled += 1
            tabled = True
        shadows, oversize = {}, None
        for o in ops:
            if o.ptr is None:
                continue
            blk = self._block_of(o.ptr, blocks)
            if blk is None:
                self.unmapped.append((name, o.arg, o.field))
                continue
            sh = shadows.get(blk[0])
            if sh is None:
                sh = shadows[blk[0]] = _Shadow(*blk, dev)
                self.bytes_shadowed += blk[1]
            ivs = o.ivs
            if tabled and ivs:
                # a footprint that leaves the requested bytes: the allocation is shorter than
                # the table (the header) says the call may touch
                end = blk[0] + blk[2]
                if o.ptr + ivs[-1][1] > end or o.ptr + ivs[0][0] < blk[0]:
                    oversize = oversize or (o, o.ptr + ivs[-1][1] - end)
                    ivs = [(max(lo, blk[0] - o.ptr), min(hi, end - o.ptr)) for lo, hi in ivs]
                    ivs = [(lo, hi) for lo, hi in ivs if lo < hi]
            sh.operands.append(fp.Operand(o.arg, o.field, o.ptr, o.role, ivs))
        # ---- fill the shadows
        state = []
        for sh in shadows.values():
            n = sh.raw.numel()
            pat = torch.full((n // 4,), POISON, dtype=torch.int32, device=dev).view(torch.uint8)
            if tabled:
                pay = [iv for o in sh.operands for iv in sh.to_raw(o.ptr, o.ivs)]
                wr = [iv for o in sh.operands if "w" in o.role for iv in sh.to_raw(o.ptr, o.ivs)]
            else:
                pay = wr = [(sh.off, sh.off + sh.req)]
            payload, wmask = _mask(n, pay, dev), _mask(n, wr, dev)
            src = view(sh.addr, sh.size)
            sh.raw.copy_(pat)
            blk = slice(sh.off, sh.off + sh.size)
            sh.raw[blk] = torch.where(payload[blk], src, pat[blk])
            state.append((sh, src, wmask, sh.raw.clone()))
        # ---- the real call on the shadow pointers
        keep = []

        def moved(p):
            blk = self._block_of(p, blocks) if p else None
            if blk is None:
                return p
            if blk[0] not in shadows:
                raise RuntimeError(f"{name}: a pointer argument has no footprint declaration")
            return shadows[blk[0]].ptr + (p - blk[0])

        new = list(args)
        for i, a in enumerate(args[:-1]):
            if sig[i] is not nat.P or a is None:
                continue
            if isinstance(a, ctypes._Pointer):
                s = type(a.contents).from_buffer_copy(a.contents)
                for f, t in s._fields_:
                    if t is nat.P and getattr(s, f):
                        setattr(s, f, moved(getattr(s, f)))
                keep.append(s)
                new[i] = ctypes.pointer(s)
            elif isinstance(a, int):
                new[i] = moved(a)
        self.orig(name, *new)
        torch.cuda.synchronize()
        if oversize is not None:
            o, by = oversize
            raise FenceError("declared footprint ends past the allocation", name, o.arg, o.field,
                             o.ivs[-1][1] - by, f" ({by} bytes short)")
        # ---- check, then hand the written bytes back
        for sh, src, wmask, before in state:
            self._check(name, sh, wmask, before)
        for sh, src, wmask, before in state:
            blk = slice(sh.off, sh.off + sh.size)
            src.copy_(torch.where(wmask[blk], sh.raw[blk], src))
        torch.cuda.synchronize()

    def _culprit(self, sh, pos, roles):
        """(operand, offset) of the operand of `sh` nearest to raw position pos."""
        best = None
        if not any(o.role in roles for o in sh.operands):
            roles = (None, "r", "w", "rw")     # (a block of read-only operands)
        for o in sh.operands:
            if o.role is not None and o.role not in roles:
                continue
            ivs = sh.to_raw(o.ptr, o.ivs) or [(o.ptr - sh.addr + sh.off,) * 2]
            d = min(0 if lo <= pos < hi else min(abs(pos - lo), abs(pos - hi + 1)) for lo, hi in ivs)
            if best is None or d < best[0]:
                best = (d, o)
        o = best[1]
        return o, pos - (o.ptr - sh.addr + sh.off)

    def _check(self, name, sh, wmask, before):
        changed = (sh.raw != before) & ~wmask
        if bool(changed.any()):
            pos = int(changed.nonzero()[0])
            inside_r = [o for o in sh.operands if o.role == "r"
                        and any(lo <= pos < hi for lo, hi in sh.to_raw(o.ptr, o.ivs))]
            if inside_r:
                o = inside_r[0]
                raise FenceError("a read-only operand was written", name, o.arg, o.field,
                                 pos - (o.ptr - sh.addr + sh.off))
            o, off = self._culprit(sh, pos, ("w", "rw"))
            raise FenceError("a write outside the operand's footprint", name, o.arg, o.field, off,
                             f" ({int(changed.sum())} bytes changed outside every written "
                             f"footprint of this block)")
        now, was = sh.raw.view(torch.int32), before.view(torch.int32)
        fresh = (now == POISON) & (was != POISON)
        if bool(fresh.any()):
            pos = 4 * int(fresh.nonzero()[0])
            o, off = self._culprit(sh, pos, ("w", "rw"))
            raise FenceError("a poison value was read and stored", name, o.arg, o.field, off,
                             " (a load outside every declared footprint reached this output)")

    def summary(self):
        return (f"{self.calls} fenced calls ({self.tabled} with a footprint entry, "
                f"{self.bytes_shadowed / 2 ** 20:.0f} MiB shadowed), end guards only: "
                f"{sorted(self.end_guards_only)}, unmapped pointers: {len(self.unmapped)}")


@contextlib.contextmanager
def fence(call=None):
    """Run `_native.call` fenced inside the block; yields the Fence (its counters)."""
    f = Fence(call)
    saved = nat.call
    nat.call = f
    try:
        yield f
    finally:
        nat.call = saved
