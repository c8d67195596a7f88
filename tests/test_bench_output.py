"""bench.py's stdout carries exactly ONE JSON line: anything else written to
fd 1 by native code (RCCL prints a version banner to C stdout when a
communicator comes up -- seen on the GPU box at world 1) goes to stderr."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_only_the_json_line_reaches_stdout():
    code = ("import os, sys, ctypes; sys.path.insert(0, %r); import bench\n"
            "fd = bench._stdout_for_json_only()\n"
            "print('python noise')\n"
            "libc = ctypes.CDLL(None); libc.puts(b'RCCL version : banner'); libc.fflush(None)\n"
            "os.write(1, b'raw fd noise\\n')\n"
            "bench.emit(fd, {'metric': 'm', 'value': 1.5})\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and json.loads(lines[0]) == {"metric": "m", "value": 1.5}, r.stdout
    assert "RCCL version" in r.stderr and "python noise" in r.stderr and "raw fd noise" in r.stderr


def test_dump_outputs_writes_float32_and_a_fixed_sample(tmp_path):
    """--dump-outputs: small arrays whole, a parameter-sized one as the same
    sorted sample of its elements on every call; float32 .npy files."""
    import numpy as np
    import bench
    big = np.arange(bench.DUMP_SAMPLE + 12345, dtype=np.float64)
    small = np.array([[0.25], [0.5]], np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,)
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0)       # the same elements, in order, none twice
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small)
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "small.npy"]


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"
