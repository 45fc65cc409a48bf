"""CPU: the engine's launch schedule (light_unet/engine.py) against its recorded trace.

tools/launch_trace.py runs UNetEngine.forward / backward on CPU tensors with the native calls
stubbed and writes every call, argument, allocation and reduction item as text; one sha256 per case
is kept in tests/golden/launch_trace.json.  A change of the scheduling code that is meant to
preserve behaviour leaves every hash as it is; a change that is meant to alter launches regenerates
the file (`python tools/launch_trace.py --write`) and the diff of `--dump CASE` shows what moved.
Needs the built library (its host queries), no GPU."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lt():
    spec = importlib.util.spec_from_file_location(
        "launch_trace", os.path.join(ROOT, "tools", "launch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def traced(lt):
    return lt.trace_all()


def test_hashes_equal_golden(lt, traced):
    rows, _ = traced
    gold = lt.load_golden()
    assert [r["name"] for r in rows] == [g["name"] for g in gold]
    diff = [(r["name"], r["calls"], g["calls"]) for r, g in zip(rows, gold) if r != g]
    assert not diff, f"launch trace changed (case, calls now, calls golden): {diff}"


def test_every_entry_point_is_reached(lt, traced):
    _, called = traced
    missing = lt.engine_entry_points() - called
    assert not missing, f"engine.py names entry points that no traced case calls: {sorted(missing)}"


def test_raw_address_is_refused(lt):
    import torch
    canon = lt.Canon({"buf": torch.zeros(4)})
    assert canon.arg(canon.table[0][0] + 8) == "buf+8"
    with pytest.raises(ValueError):
        canon.arg(canon.table[0][1] + (1 << 40))
