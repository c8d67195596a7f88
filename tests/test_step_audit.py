"""The audits of tests/step_audit.py bite (no GPU): a synthetic call list
over numpy buffers in which one call writes outside its declared writes, one
reads a buffer it does not declare, and one accumulates into its output; and
two traces that differ at a known call."""
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import step_audit  # noqa: E402
from step_audit import Region, SerialAudit, Trace, digest, first_difference  # noqa: E402


@dataclasses.dataclass
class FakeCall:
    fn: object
    args: tuple
    name: str
    lane: int
    reads: tuple
    writes: tuple
    idx: int = -1


ROWS, C = 6, 8


def _setup():
    rng = np.random.default_rng(5)
    bufs = {"x": rng.normal(size=16).astype(np.float32), "y": np.zeros(16, np.float32),
            "z": rng.normal(size=16).astype(np.float32), "m": np.zeros(ROWS * C, np.float32),
            "table": np.arange(4, dtype=np.int32)}
    x, y, z, m = bufs["x"], bufs["y"], bufs["z"], bufs["m"]
    mat = m.reshape(ROWS, C)

    def double():                   # honest
        y[:] = 2 * x

    def stray_write():              # declares y, also touches z[3]
        y[:] = x + 1
        z[3] = 7.0

    def stray_read():               # declares x, also reads z
        y[:] = x + z

    def accumulate():               # y += x with y declared as a write alone
        y[:] = y + x

    def slice_ok():                 # channels 2..5 of every row
        mat[:, 2:5] = x[:3]

    def slice_wide():               # declared 2..5, writes 2..6
        mat[:, 2:6] = x[:4]

    regs = {("x",): [Region("x", 0, 16)], ("y",): [Region("y", 0, 16)], ("z",): [Region("z", 0, 16)],
            ("m", 2): [Region("m", 2, 3, ROWS, C)], ("m", 5): [Region("m", 5, 3, ROWS, C)]}
    calls = [FakeCall(lambda: double(), (), "double", 0, (("x",),), (("y",),)),
             FakeCall("param_ready", 0, "hook", 0, (), ()),
             FakeCall(lambda: stray_write(), (), "stray_write", 1, (("x",),), (("y",),)),
             FakeCall(lambda: stray_read(), (), "stray_read", 0, (("x",),), (("y",),)),
             FakeCall(lambda: accumulate(), (), "accumulate", 1, (("x",),), (("y",),)),
             FakeCall(lambda: slice_ok(), (), "slice_ok", 0, (("x",),), (("m", 2),)),
             FakeCall(lambda: slice_wide(), (), "slice_wide", 0, (("x",), ("m", 5)), (("m", 2),))]
    for i, c in enumerate(calls):
        c.idx = i
    tensors = {k: torch.from_numpy(v) for k, v in bufs.items()}
    return bufs, tensors, regs, calls


def _audit(tensors, regs):
    return SerialAudit(tensors, regs.__getitem__, lambda: None)


def test_write_audit_names_the_call_that_writes_outside_its_writes():
    bufs, tensors, regs, calls = _setup()
    wfind, _ = _audit(tensors, regs).run(calls, poison=False)
    assert len(wfind) == 2, wfind
    assert wfind[0].startswith("call 2 stray_write (lane 1) wrote outside its declared writes: z[3]")
    assert "no declared resource" in wfind[0]            # no call of the list names z
    # the strided slice: channel 5 of row 0 is element 5, the next slice's first channel
    assert wfind[1].startswith("call 6 slice_wide (lane 0) wrote outside its declared writes: m[5]")
    assert "resource ('m', 5)" in wfind[1]
    assert np.isfinite(bufs["y"]).all()


def test_read_audit_names_the_call_that_reads_what_it_does_not_declare():
    bufs, tensors, regs, calls = _setup()
    x0, z0 = bufs["x"].copy(), bufs["z"].copy()
    wfind, rfind = _audit(tensors, regs).run(calls, poison=True)
    assert len(wfind) == 2
    assert len(rfind) == 1, rfind
    assert rfind[0].startswith("call 3 stray_read (lane 0) read something it does not declare; differs at y[0]")
    # the poison is gone and the run is the unpoisoned serial run
    z0[3] = 7.0
    assert np.array_equal(bufs["x"], x0) and np.array_equal(bufs["z"], z0)
    assert np.array_equal(bufs["y"], (x0 + z0) + x0)
    assert np.array_equal(bufs["table"], np.arange(4))
    assert np.array_equal(bufs["m"].reshape(ROWS, C)[:, 2:6], np.tile(x0[:4], (ROWS, 1)))


def test_a_write_implies_a_read_in_one_place(monkeypatch):
    """The accumulating call passes under the convention and is named without it."""
    _, tensors, regs, calls = _setup()
    monkeypatch.setattr(step_audit, "WRITE_IMPLIES_READ", False)
    _, rfind = _audit(tensors, regs).run(calls, poison=True)
    assert [f.split(" ")[2] for f in rfind] == ["stray_read", "accumulate"], rfind


def test_unknown_key_and_out_of_range_region_are_errors():
    _, tensors, regs, calls = _setup()
    calls[0].reads = (("nope",),)
    with pytest.raises(KeyError):
        _audit(tensors, regs).run(calls)
    calls[0].reads = (("x",),)
    regs[("x",)] = [Region("x", 8, 16)]
    with pytest.raises(IndexError):
        _audit(tensors, regs).run(calls)


def test_integer_buffers_are_never_poisoned():
    assert step_audit.never_poison("whatever", torch.zeros(2, dtype=torch.int32))
    assert step_audit.never_poison("params", torch.zeros(2))
    assert step_audit.never_poison("ws_lane[1]", torch.zeros(2))
    assert step_audit.never_poison("wprep_table", torch.zeros(2))
    assert not step_audit.never_poison("acts[3]", torch.zeros(2, dtype=torch.bfloat16))
    mem = step_audit.Memory({"a": torch.zeros(3), "b": torch.zeros(5, dtype=torch.bfloat16)})
    pois, keep = mem.poison(step_audit.never_poison)
    a, b = mem.segs(pois)
    assert a.view(torch.int32).tolist() == [0x7FC00000] * 3 and b.view(torch.int16).tolist() == [0x7FC0] * 5
    assert torch.isnan(a.view(torch.float32)).all() and torch.isnan(b.view(torch.bfloat16)).all()


def test_first_difference_returns_the_call():
    rows = [(s, i, f"op{i}", i % 2, ("r", i)) for s in range(2) for i in range(5)]
    base = np.arange(10, dtype=np.int64) * 977
    t1, t2 = Trace(rows, base.copy()), Trace(list(rows), base.copy())
    assert first_difference(t1, t2) is None
    t2.values[7] += 1
    t2.values[9] += 1
    d = first_difference(t1, t2)
    assert (d["step"], d["call"], d["name"], d["lane"], d["resource"]) == (1, 2, "op2", (0, 0), (("r", 2), ("r", 2)))
    # lanes and resource names may differ between a one- and a two-lane list; a call name may not
    t3 = Trace([(s, i, n, 0, ("q", i)) for s, i, n, _, _ in rows], base.copy())
    assert first_difference(t1, t3) is None
    t3.rows[4] = (0, 4, "other", 0, ("q", 4))
    assert first_difference(t1, t3)["call"] == 4
    assert first_difference(t1, Trace(rows[:6], base[:6].copy()))["name"] == "length"


def test_digest_sees_order_and_bits():
    ramp = 2 * torch.arange(8, dtype=torch.int64) + 1
    a = torch.tensor([1.0, 2.0, 3.0, -0.0])
    assert int(digest(a, ramp)) != int(digest(a.flip(0), ramp))
    assert int(digest(a, ramp)) != int(digest(torch.tensor([1.0, 2.0, 3.0, 0.0]), ramp))
    assert int(digest(a, ramp)) == int(digest(a.clone(), ramp))
    m = torch.arange(12, dtype=torch.float32).reshape(3, 4)[:, 1:3]          # a strided slice
    assert int(digest(m, ramp)) == int(digest(m.contiguous(), ramp))
