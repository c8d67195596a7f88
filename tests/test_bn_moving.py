"""Moving BN statistics, the parts that need no GPU: the C-ABI surface and its
argument validation (before any HIP call), the segment planner's refusal of a
launch without an unbiased variance, the .bnstats checkpoint side file, and
the CLI flags."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG


def test_abi_declares_binds_and_exports_both_entry_points():
    import ctypes
    from jr import _ffi
    from test_abi import header_symbols
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("jr_bn_moving_update", "jr_bn_moving_freeze"):
        assert name in header_symbols() and name in _ffi.EXPORTED and hasattr(lib, name)
    assert ctypes.sizeof(_ffi.BnMovingSeg) == 32
    # the ctypes stub of INTEGRATION.md names them too
    text = open(os.path.join(os.path.dirname(PKG), "INTEGRATION.md")).read()
    assert "jr_bn_moving_update" in text and "jr_bn_moving_freeze" in text


def test_validation_refusals_without_gpu():
    from jr import _ffi
    L = _ffi.load()
    p = 4096          # any non-null address: refused before it is looked at

    def upd(segs=p, nseg=1, max_c=16, members=1, stats=p, sms=0, moving=p, mms=0, momentum=0.99, eps=1e-3):
        return L.jr_bn_moving_update(segs, nseg, max_c, members, stats, sms, moving, mms, momentum, eps, None)

    def frz(segs=p, nseg=1, max_c=16, members=1, moving=p, mms=0, frozen=p, fms=0, eps=1e-3):
        return L.jr_bn_moving_freeze(segs, nseg, max_c, members, moving, mms, frozen, fms, eps, None)

    bad = _ffi.JR_ERR_INVALID
    for kw in (dict(segs=None), dict(stats=None), dict(moving=None), dict(nseg=0), dict(nseg=-3), dict(members=0),
               dict(members=65536), dict(momentum=-0.01), dict(momentum=1.5), dict(momentum=float("nan")),
               dict(eps=0.0), dict(eps=-1e-3), dict(sms=-1), dict(mms=-8), dict(max_c=0)):
        assert upd(**kw) == bad, kw
        assert "bn_moving_update" in _ffi.last_error()
    for kw in (dict(segs=None), dict(moving=None), dict(frozen=None), dict(nseg=0), dict(members=0),
               dict(members=65536), dict(eps=0.0), dict(mms=-1), dict(fms=-1)):
        assert frz(**kw) == bad, kw
        assert "bn_moving_freeze" in _ffi.last_error()


def test_segment_table_refuses_a_single_row():
    """rows = n * ho * wo < 2 has no unbiased variance: the planner refuses to
    build the table (at 75^2 the last blocks are 1x1, so batch 1 is refused;
    at 299^2 they are 8x8)."""
    from jr.inception import build_inception_v3
    from jr.plan import bn_moving_segments, build_plan
    units = build_plan(build_inception_v3(75, 75)).units
    segs = bn_moving_segments(units, 2)
    assert len(segs) == len(units) and min(r for _, _, r, _ in segs) == 2
    off = 0
    for (so, mo, rows, c), u in zip(segs, units):       # the statistics layout: [mean(c) | invstd(c)] per launch
        assert (so, mo, rows, c) == (off, off, 2 * u.ho * u.wo, u.cout)
        off += 2 * c
    with pytest.raises(ValueError, match="at least 2 rows"):
        bn_moving_segments(units, 1)
    assert len(bn_moving_segments(build_plan(build_inception_v3(299, 299)).units, 1)) > 0


def _stats(g, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for n in g.convs:
        out[f"batch_normalization_{n.idx + 1}/moving_mean"] = rng.standard_normal(n.cout).astype(np.float32)
        out[f"batch_normalization_{n.idx + 1}/moving_variance"] = rng.random(n.cout).astype(np.float32)
    return out


def test_checkpoint_bnstats_roundtrip_old_format_and_corruption(tmp_path):
    from jr import checkpoint
    from jr.inception import build_inception_v3
    from jr.init import init_params
    import evaluate
    g = build_inception_v3(107, 107)
    flat, st = init_params(g, 2), _stats(g, 5)
    with_stats, plain = str(tmp_path / "with" / "model"), str(tmp_path / "plain" / "model")
    checkpoint.save(with_stats, g, flat, {"epoch": 1}, bn_moving={"stats": st, "momentum": 0.99, "updates": 7})
    checkpoint.save(plain, g, flat, {"epoch": 1})
    # without statistics: the three files and the .meta of before, and none reported
    assert sorted(os.listdir(tmp_path / "plain")) == ["model" + checkpoint.DATA_SUFFIX, "model.index", "model.meta"]
    assert "bn_moving" not in json.load(open(plain + ".meta"))
    assert checkpoint.load_bn_moving(plain, g) is None
    # with: one more file; parameters, index and data as without
    assert sorted(os.listdir(tmp_path / "with")) == ["model.bnstats", "model" + checkpoint.DATA_SUFFIX, "model.index",
                                                     "model.meta"]
    for suffix in (".index", checkpoint.DATA_SUFFIX):
        assert open(with_stats + suffix, "rb").read() == open(plain + suffix, "rb").read()
    got, meta = checkpoint.load(with_stats, g)
    np.testing.assert_array_equal(got, flat)
    info = meta["bn_moving"]
    assert (info["momentum"], info["updates"]) == (0.99, 7) and sorted(info) == ["channels", "momentum", "sha256",
                                                                                "updates"]
    assert info["channels"] == [n.cout for n in g.convs]
    assert os.path.getsize(with_stats + ".bnstats") == 8 * sum(info["channels"])
    back = checkpoint.load_bn_moving(with_stats, g)
    assert sorted(back) == sorted(st)
    for k in st:
        np.testing.assert_array_equal(back[k], st[k])
    # layout: per layer in graph order, mean[c] then var[c], little-endian f32
    raw = np.frombuffer(open(with_stats + ".bnstats", "rb").read(), "<f4")
    c0 = g.convs[0].cout
    np.testing.assert_array_equal(raw[:c0], st["batch_normalization_1/moving_mean"])
    np.testing.assert_array_equal(raw[c0:2 * c0], st["batch_normalization_1/moving_variance"])
    # the ensemble glob still yields the stem once
    assert evaluate.expand_model_paths(str(tmp_path / "with" / "mod*")) == [with_stats]
    assert checkpoint.exists(with_stats) and checkpoint.read_meta(with_stats)["epoch"] == 1
    # saving over it replaces the statistics
    checkpoint.save(with_stats, g, flat, {"epoch": 2}, bn_moving={"stats": st, "momentum": 0.5, "updates": 1})
    assert checkpoint.read_meta(with_stats)["bn_moving"]["momentum"] == 0.5
    checkpoint.load_bn_moving(with_stats, g)
    # corruption and truncation raise
    p = with_stats + ".bnstats"
    blob = bytearray(open(p, "rb").read())
    blob[40] ^= 0xFF
    open(p, "wb").write(bytes(blob))
    with pytest.raises(ValueError, match="checksum"):
        checkpoint.load_bn_moving(with_stats, g)
    open(p, "wb").write(bytes(blob[:-4]))
    with pytest.raises(ValueError, match="size"):
        checkpoint.load_bn_moving(with_stats, g)
    os.remove(p)
    with pytest.raises(ValueError, match="missing"):
        checkpoint.load_bn_moving(with_stats, g)
    checkpoint.load(with_stats, g)                      # the parameters still load
    with pytest.raises(ValueError):                      # a wrong channel count
        checkpoint.save(with_stats, build_inception_v3(107, 107), flat,
                        bn_moving={"stats": {k: v[:-1] for k, v in st.items()}, "momentum": 0.9, "updates": 0})
    checkpoint.save(plain, g, flat, bn_moving={"stats": st, "momentum": 0.9, "updates": 0})
    checkpoint.save(plain, g, flat)
    assert not os.path.exists(plain + ".bnstats") and checkpoint.load_bn_moving(plain, g) is None


def test_cli_help_carries_the_flags():
    for script, flags in (("train.py", ["--bn_moving"]),
                          ("evaluate.py", ["--bn {batch,moving}", "--bn_calibrate_dir", "--bn_calibrate_batches"])):
        r = subprocess.run([sys.executable, os.path.join(PKG, script), "--help"], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        for f in flags:
            assert f in r.stdout, (script, f)
    import train
    import evaluate
    assert train.build_parser().parse_args([]).bn_moving is None
    assert train.build_parser().parse_args(["--bn_moving"]).bn_moving == 0.99
    assert train.build_parser().parse_args(["--bn_moving", "0.9"]).bn_moving == 0.9
    assert "rank 0" in train.build_parser().format_help()
    a = evaluate.build_parser().parse_args([])
    assert (a.bn, a.bn_calibrate_dir) == ("batch", None)
