"""Gradient accumulation on the GPU: jr_grad_accumulate
against its numpy restatement (tests/accum_ref.py), and Engine(accum_steps=K)
against a second engine that accumulates by hand -- forward / backward per
micro-batch, torch fp32 adds of `grads` in micro-batch order, the sum copied
into `grads`, apply_update(grad_scale=1/k).  Every comparison is bitwise: each
result is a fixed sequence of correctly rounded fp32 adds over gradients the
engine produces deterministically.

All engines at 107^2, B = 4, tiles="heuristic" (the smallest shape the suite
uses for whole steps).
"""
import os
import socket
import tempfile
import time

import numpy as np
import pytest

import accum_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RES, B = 107, 4


def _bits(t):
    return t.detach().reshape(-1).view(torch.int32)


def _same(a, b) -> bool:
    return bool(torch.equal(_bits(a), _bits(b)))


def _batch(i, nan_label=False):
    from jr import synth
    x, y = synth.fundus_batch(500 + 10 * i, B, RES), synth.labels(500 + 10 * i, B, p=0.5)
    if nan_label:
        y = y.copy()
        y.reshape(-1)[1] = np.nan
    return x, y


def _engine(**kw):
    from jr.engine import Engine
    return Engine(B, RES, RES, seed=3, tiles="heuristic", **kw)


# ------------------------------------------------ the kernel against the restatement
# update_grid caps the grid at 256 * 32 blocks of kTile = 256 quads: one pass of the aligned
# kernel covers 8,388,608 elements.  WRAP: one tile more than a pass, with a tail of 3.
PASS = 256 * 32 * 256 * 4
WRAP = PASS + 1024 + 3
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, WRAP]
ALIGN = {"both16": (0, 0), "both+4": (1, 1), "dst+4": (1, 0), "src+4": (0, 1)}    # offsets in floats
GUARD = 8       # guard words before and after dst
PATTERN = 0x5EEDBEEF


@pytest.mark.parametrize("align", sorted(ALIGN))
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_restatement(n, align):
    """first in {0, 1}; +-0, denormals, +-inf and four NaNs in the inputs (two in src, two in dst, from
    n >= 16; a prefix of the specials below); bits everywhere except at the reference's NaNs, NaN-ness there;
    the guard words around dst unchanged."""
    from jr import _ffi
    _ffi.init(0)
    L = _ffi.load()
    od, osrc = ALIGN[align]
    src_h = accum_ref.special_values(n, 11 * n + 1, nans=2)
    dst_h = accum_ref.special_values(n, 11 * n + 2, nans=2)
    if n >= 16:
        assert int(np.isnan(src_h).sum()) + int(np.isnan(dst_h).sum()) == 4
    dev = torch.device("cuda", 0)
    for first in (0, 1):
        # dst region at float offset 16 + od of a fresh buffer (torch allocations are 256-byte aligned)
        dbuf = torch.full((16 + od + n + GUARD + 4,), PATTERN, dtype=torch.int32, device=dev)
        d0 = 16 + od
        dbuf[d0:d0 + n] = torch.from_numpy(dst_h.view(np.int32)).to(dev)
        sbuf = torch.zeros(16 + osrc + n, dtype=torch.float32, device=dev)
        sbuf[16 + osrc:] = torch.from_numpy(src_h).to(dev)
        dptr, sptr = dbuf.data_ptr() + 4 * d0, sbuf.data_ptr() + 4 * (16 + osrc)
        assert (dptr % 16 == 0) == (od == 0) and (sptr % 16 == 0) == (osrc == 0)
        torch.cuda.synchronize()
        rc = L.jr_grad_accumulate(dptr, sptr, n, first, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _ffi.last_error()
        torch.cuda.synchronize()
        out = dbuf.cpu().numpy()
        got = out[d0:d0 + n].view(np.float32)
        want = accum_ref.accumulate(dst_h, src_h, bool(first))
        nan = np.isnan(want)
        if first:
            assert np.array_equal(nan, np.isnan(src_h))        # dst's NaNs are gone: a copy
        bad = np.flatnonzero(got.view(np.uint32)[~nan] != want.view(np.uint32)[~nan])
        assert bad.size == 0, (n, align, first, bad[:5])
        assert np.all(np.isnan(got[nan])), (n, align, first)
        assert np.all(out[:d0] == PATTERN) and np.all(out[d0 + n:] == PATTERN), (n, align, first, "guard words")
        assert np.array_equal(sbuf[16 + osrc:].cpu().numpy().view(np.uint32), src_h.view(np.uint32))    # src untouched
    _ffi.device_check()


# ------------------------------------------------------------------- engine, eager
CASES = {
    "f32": dict(),                                                   # the engine's default math (x8), Nesterov by value
    "x6h": dict(conv_math="x6h"),
    "bf16": dict(dtype="bf16"),
    "nesterov": dict(optimizer="nesterov", lr=0.01, momentum=0.8, lanes=1),
    "device": dict(weight_decay=4e-5, clip_norm=1.0),                # the device path: decay, clipping
    "rmsprop": dict(optimizer="rmsprop", weight_ema=0.99, bn_moving=0.99, dropout=0.2, dropout_seed=5),
}
GROUPS = (3, 3, 2)      # K = 3: two full groups, then two micro-batches and accum_flush


def _hand_update(ref, first_batch, k, micro0):
    """The reference's update over micro-batches first_batch .. first_batch + k - 1; returns their losses.
    (dropout: the mask counter counts micro-batches, set by hand; bn_moving: one update per micro-batch,
    the k-th inside apply_update.)"""
    from jr import _ffi
    losses, gsum = [], None
    for j in range(k):
        ref.set_batch(*_batch(first_batch + j))
        if ref.dropout is not None:
            ref._dropout_set(micro0 + j)
        ref.forward(training=True)
        ref.backward(training=True)
        if ref.bn_momentum is not None and j + 1 < k:
            _ffi.check("jr_bn_moving_update",
                       ref.lib.jr_bn_moving_update(*ref._bn_update_args(B, ref.bn_momentum, ref._s)))
        ref.synchronize()
        losses.append(ref.loss_value())
        g = ref.grads.clone()
        gsum = g if gsum is None else gsum + g          # torch fp32 adds, micro-batch order
    ref.grads.copy_(gsum)
    torch.cuda.synchronize()          # copy_ ran on torch's stream, the update runs on the engine's
    ref.apply_update(grad_scale=1.0 / k, training=True)
    ref.synchronize()
    return losses


@pytest.mark.parametrize("case", sorted(CASES))
def test_engine_equals_accumulating_by_hand(case):
    kw = CASES[case]
    eng, ref = _engine(accum_steps=3, **kw), _engine(**kw)
    assert eng.gacc is not None and eng.gacc.numel() == eng.nparam and ref.gacc is None
    i = micro = 0
    for u, k in enumerate(GROUPS):
        got = []
        for j in range(k):
            assert eng.accum_pending() == j
            eng.set_batch(*_batch(i + j))
            eng.train_step()
            got.append(eng.loss_value())
        if k < eng.accum_steps:
            assert eng.accum_pending() == k
            assert eng.accum_flush() is True
        assert eng.accum_pending() == 0 and eng.accum_flush() is False
        eng.synchronize()
        want = _hand_update(ref, i, k, micro)
        assert got == want, (case, u, got, want)                        # every micro-batch's loss
        assert _same(eng.params, ref.params), (case, u, int((_bits(eng.params) != _bits(ref.params)).sum()))
        assert _same(eng.accum, ref.accum), (case, u)
        if eng.opt_ex:
            assert eng.opt_step() == ref.opt_step(), (case, u)           # the accumulated mean gradient's norm
            if eng.clip_norm is not None and u == 0:
                print(f"{case}: update {u} norm, scale, skipped, total = {eng.opt_step()}")
        i, micro = i + k, micro + k
    if case == "rmsprop":
        assert _same(eng.adam_v, ref.adam_v) and _same(eng.ema, ref.ema)
        assert eng.ema_updates() == len(GROUPS) == ref.ema_updates()     # per update
        assert eng.dropout_steps() == sum(GROUPS)                        # per micro-batch
        assert eng.updates == sum(GROUPS)                                # (the BN moving averages' count)
        assert _same(eng.moving, ref.moving)
    eng.close()
    ref.close()


def test_load_params_discards_an_open_group():
    eng, ref = _engine(accum_steps=2), _engine(accum_steps=2)
    p0 = eng.params_numpy()
    eng.set_batch(*_batch(9))
    eng.train_step()
    assert eng.accum_pending() == 1
    eng.load_params(p0)
    assert eng.accum_pending() == 0
    for e in (eng, ref):
        for j in range(2):
            e.set_batch(*_batch(j))
            e.train_step()
        e.synchronize()
    assert _same(eng.params, ref.params)
    eng.close()
    ref.close()


# -------------------------------------------------------------------------- K = 1
def test_accum_steps_1_is_the_default_engine():
    """The same call lists under the same cache keys, and no buffer."""
    from jr.lanes import signature
    kw = dict(weight_decay=4e-5, weight_ema=0.99, bn_moving=0.99, dropout=0.2)
    a, b = _engine(**kw), _engine(accum_steps=1, **kw)
    assert b.accum_steps == 1 and a.gacc is None and b.gacc is None
    for build in (dict(), dict(training=True), dict(nl=1)):
        la, lb = a._build_calls(B, **build), b._build_calls(B, **build)
        for p in range(3):
            assert signature(la[p]) == signature(lb[p]), (build, p)
            assert "grad_accumulate" not in signature(lb[p])
    assert sorted(a._calls, key=repr) == sorted(b._calls, key=repr)
    with pytest.raises(ValueError):
        b._build_calls(B, accum="open")
    assert b.accum_pending() == 0 and b.accum_flush() is False
    a.close()
    b.close()


# ------------------------------------------------------------- capture and replay
@pytest.mark.parametrize("case,kw", [("nesterov", dict()),
                                     ("rmsprop_device", dict(optimizer="rmsprop", device_lr=True, clip_norm=1.0))])
def test_replayed_groups_equal_the_eager_run(case, kw):
    """K = 3 (an opening, an inside and a closing graph), two groups."""
    eager, graph = _engine(accum_steps=3, **kw), _engine(accum_steps=3, **kw)
    for m in range(6):
        for e in (eager, graph):
            e.set_batch(*_batch(m))
        eager.train_step()
        if m == 0:
            graph.capture()
            assert sorted(graph._graphs, key=repr) == [(B, "close"), (B, "inside"), (B, "open")]
        graph.replay()
        assert eager.accum_pending() == graph.accum_pending() == (m + 1) % 3
        assert eager.loss_value() == graph.loss_value(), (case, m)
        if (m + 1) % 3 == 0:
            assert _same(eager.params, graph.params) and _same(eager.accum, graph.accum), (case, m)
            if eager.opt_ex:
                assert eager.opt_step() == graph.opt_step()
    eager.close()
    graph.close()


# ------------------------------------------------------------------ a skipped group
def test_a_skipped_group_leaves_nothing_behind():
    """K = 2.  Group 2 holds a micro-batch with a NaN label: its update is skipped (parameters, optimizer
    state and the average's counter unchanged), and group 3's update equals that of a run that never saw
    group 2 -- the opening copy overwrites the NaNs the skipped group left in the accumulator."""
    kw = dict(accum_steps=2, clip_norm=5.0, weight_ema=0.99)
    eng, ref = _engine(**kw), _engine(**kw)

    def group(e, batches, bad=None):
        for i in batches:
            e.set_batch(*_batch(i, nan_label=(i == bad)))
            e.train_step()
        e.synchronize()

    group(eng, (0, 1))
    group(ref, (0, 1))
    assert _same(eng.params, ref.params) and eng.opt_step()[2:] == (0, 0)
    before = {n: getattr(eng, n).clone() for n in ("params", "accum", "ema")}
    group(eng, (2, 3), bad=2)
    norm, scale, skipped, total = eng.opt_step()
    assert not np.isfinite(norm) and (scale, skipped, total) == (0.0, 1, 1)
    for n, t in before.items():
        assert _same(getattr(eng, n), t), n
    assert eng.ema_updates() == 1
    assert bool(torch.isnan(eng.gacc).any())                # what the next group's first = 1 has to overwrite
    group(eng, (4, 5))
    group(ref, (4, 5))
    assert eng.opt_step()[2:] == (0, 1) and ref.opt_step()[2:] == (0, 0)
    assert eng.opt_step()[:2] == ref.opt_step()[:2]
    for n in before:
        assert _same(getattr(eng, n), getattr(ref, n)), n
    assert eng.ema_updates() == 2 == ref.ema_updates()
    assert bool(torch.isfinite(eng.params).all())
    eng.close()
    ref.close()


# ---------------------------------------------------------------------- step audit
def _audit(e, lists, phases=(0, 1, 2)):
    import step_audit
    return step_audit.engine_audit(e, lists, True, phases)


@pytest.mark.parametrize("phase", ["open", "inside", "close", "flush"])
def test_step_audit_of_the_accumulating_lists(phase):
    """Every keyword on (bf16: deferred filter gradients too).  Write set: what a call changes lies inside
    its declared writes; read set: everything it declares neither as a read nor as a write poisoned with
    quiet NaNs, its writes come out bit for bit; and the two-lane schedule orders every conflicting pair.
    The accumulate declares ("gacc",) and every ("g", .): reads on a step that leaves the group open,
    writes on the fold."""
    from jr import lanes
    e = _engine(dtype="bf16", lanes=2, accum_steps=3, optimizer="rmsprop", weight_decay=4e-5, clip_norm=1.0,
                weight_ema=0.99, bn_moving=0.99, dropout=0.2, label_smoothing=0.1)
    for m in range(4):                   # a whole group and an open one: every buffer holds real values
        e.set_batch(*_batch(m))
        e.train_step()
    e.set_batch(*_batch(4))
    e.synchronize()
    torch.cuda.synchronize()
    if phase == "flush":
        lists = ([], [], e._flush_calls(), [], None)
    else:
        lists = e._build_calls(B, training=True, accum=phase)
        seq = [c for p in lists[:3] for c in p if c.fn != "param_ready"]
        lanes.check_schedule(seq, precise=False)
        lanes.check_schedule(seq, precise=True)
    acc = [c for c in lists[2] if c.name == "grad_accumulate"]
    assert len(acc) == 1 and acc[0] is lists[2][0]
    g_keys = {k for k in acc[0].reads + acc[0].writes if k[0] == "g"}
    assert len(g_keys) == len(e.cunits) + 1
    if phase in ("open", "inside"):
        assert acc[0].writes == (("gacc",),) and set(acc[0].reads) == g_keys
        assert acc[0].args[3] == int(phase == "open")
        assert [c.name for c in lists[2]] == ["grad_accumulate", "bn_moving", "dropout_advance"]
    else:
        assert acc[0].reads == (("gacc",),) and set(acc[0].writes) == g_keys
        assert acc[0].args[3] == int(phase == "flush")
        tail = ["bn_moving", "dropout_advance"] if phase == "close" else []
        assert [c.name for c in lists[2]] == ["grad_accumulate", "grad_sqnorm", "opt_prepare", "rmsprop_update_ex",
                                              "ema_prepare", "ema_update"] + tail
    t0 = time.perf_counter()
    wfind, rfind = _audit(e, lists)
    print(f"step audit of the {phase} list: {sum(len(p) for p in lists[:3])} calls, {time.perf_counter() - t0:.2f} s")
    assert not wfind, "\n".join(wfind)
    assert not rfind, "\n".join(rfind)
    e.synchronize()
    e.close()


# ----------------------------------------------------------------------- two ranks
WORLD, K2, UPDATES = 2, 2, 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard(micro, rank):
    return _batch(micro * WORLD + rank)


def _rank(rank, port, outdir, payload):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from jr.dist import BucketAllReduce
    eng = _engine(accum_steps=K2)
    ar = BucketAllReduce(eng, WORLD, bucket_bytes=8 << 20, payload=payload)
    losses, issued = [], []
    for m in range(K2 * UPDATES):
        eng.set_batch(*_shard(m, rank))
        ar.begin()                      # (a reset: a step that issues nothing leaves next and fences at 0)
        eng.train_step(allreduce=ar)
        losses.append(eng.loss_value())
        issued.append((ar.next, ar.fences, eng.accum_pending()))
        if m == K2 - 1:                 # the reduced gradient of the first update
            np.save(os.path.join(outdir, f"grad{rank}.npy"), eng.grads.cpu().numpy())
    eng.synchronize()
    np.save(os.path.join(outdir, f"params{rank}.npy"), eng.params.cpu().numpy())
    np.save(os.path.join(outdir, f"losses{rank}.npy"), np.array(losses))
    np.save(os.path.join(outdir, f"issued{rank}.npy"), np.array(issued + [(len(ar.buckets), 0, 0)]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("payload", ["f32", "bf16"])
def test_two_ranks_equal_one_process(payload):
    """gloo, both ranks on cuda:0, K = 2, two updates.  The one-process reference sums each rank's two
    micro-batch gradients in order (fp32), combines the ranks as the all-reduce does -- fp32 a + b, or (bf16
    payload) each rank's sum rounded to bf16, added, rounded to bf16 -- and updates with grad_scale 1/4."""
    import torch.multiprocessing as mp
    port = _free_port()
    with tempfile.TemporaryDirectory() as d:
        ctx = mp.get_context("spawn")
        ps = [ctx.Process(target=_rank, args=(r, port, d, payload)) for r in range(WORLD)]
        for p in ps:
            p.start()
        for p in ps:
            p.join(600)
        assert all(p.exitcode == 0 for p in ps), [p.exitcode for p in ps]
        got = [np.load(os.path.join(d, f"params{r}.npy")) for r in range(WORLD)]
        got_losses = [np.load(os.path.join(d, f"losses{r}.npy")) for r in range(WORLD)]
        got_g0 = [np.load(os.path.join(d, f"grad{r}.npy")) for r in range(WORLD)]
        issued = [np.load(os.path.join(d, f"issued{r}.npy")) for r in range(WORLD)]
    for rows in issued:
        nb = rows[-1][0]
        for m, (nxt, fences, pending) in enumerate(rows[:-1]):
            if (m + 1) % K2:            # the group stays open: no bucket is issued, no lane is fenced
                assert (nxt, fences, pending) == (0, 0, (m + 1) % K2), (m, nxt, fences, pending)
            else:
                assert nxt == nb and 1 <= fences <= nb and pending == 0, (m, nxt, fences, nb)
    ref = _engine()
    ref_losses = [[] for _ in range(WORLD)]
    for u in range(UPDATES):
        total = None
        for r in range(WORLD):
            gsum = None
            for j in range(K2):
                ref.set_batch(*_shard(u * K2 + j, r))
                ref.forward()
                ref.backward()
                ref.synchronize()
                ref_losses[r].append(ref.loss_value())
                g = ref.grads.clone()
                gsum = g if gsum is None else gsum + g
            if payload == "bf16":
                gsum = gsum.to(torch.bfloat16).float()
            total = gsum if total is None else total + gsum
        if payload == "bf16":
            total = total.to(torch.bfloat16).float()
        ref.grads.copy_(total)
        torch.cuda.synchronize()
        if u == 0:
            want_g0 = total.cpu().numpy()
        ref.apply_update(grad_scale=1.0 / (K2 * WORLD))
    ref.synchronize()
    want = ref.params.cpu().numpy()
    for r in range(WORLD):
        assert np.array_equal(got_losses[r], np.array(ref_losses[r])), (r, got_losses[r], ref_losses[r])
        bad = np.flatnonzero(got_g0[r].view(np.uint32) != want_g0.view(np.uint32))
        assert bad.size == 0, (r, bad.size, bad[:5])
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))       # ranks stay bitwise identical
    assert np.array_equal(got[0].view(np.uint32), want.view(np.uint32))         # == one process, 1/4 of the sum
    ref.close()


@pytest.mark.parametrize("payload", ["f32", "bf16"])
def test_jr_comm_world1_folds_per_bucket(payload, tmp_path):
    """libjr's own communicator at world 1 (the one-GPU box cannot host two RCCL ranks): K = 2, one
    full group through the comm stream's per-bucket fold, then one micro-batch and accum_flush(allreduce) --
    against the hand-accumulated reference (bf16 payload: the group's sum rounded to bf16 once)."""
    from jr.dist import BucketAllReduce, JrComm
    comm = JrComm(0, 1, 0, uid_path=str(tmp_path / "uid"), run_id=f"accum-{os.getpid()}")
    eng, ref = _engine(accum_steps=K2), _engine()
    ar = BucketAllReduce(eng, 1, bucket_bytes=8 << 20, comm=comm, payload=payload)
    i = 0
    for k in (2, 1):
        gsum = None
        for j in range(k):
            eng.set_batch(*_batch(i + j))
            eng.train_step(allreduce=ar)
            ref.set_batch(*_batch(i + j))
            ref.forward()
            ref.backward()
            ref.synchronize()
            assert eng.loss_value() == ref.loss_value()
            g = ref.grads.clone()
            gsum = g if gsum is None else gsum + g
        if k < K2:
            assert eng.accum_flush(allreduce=ar) is True
        assert eng.accum_pending() == 0 and ar.next == len(ar.buckets)
        if payload == "bf16":
            gsum = gsum.to(torch.bfloat16).float()
        ref.grads.copy_(gsum)
        torch.cuda.synchronize()
        ref.apply_update(grad_scale=1.0 / k)
        eng.synchronize()
        ref.synchronize()
        assert _same(eng.grads, ref.grads), k
        assert _same(eng.params, ref.params), k
        i += k
    comm.close()
    eng.close()
    ref.close()
