"""The training trace without a GPU: the two structures against the header's documented layout, the tensor tables of both
networks, the decoding of a ring that wrapped, the merge of save(), argument checks, and the host-only plan / scratch entries
of cvae_tensor_stats (they need the library, not a device)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from critic_vae_amd import lib as cvlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def trace_module():
    try:
        from critic_vae_amd import trace
    except ImportError as e:
        pytest.fail(f"critic_vae_amd.trace is missing ({e}): no training trace")
    return trace


def lib_name(name):
    if not hasattr(cvlib, name):
        pytest.fail(f"the library binding has no {name}: the training trace (cvae_trace_push / cvae_tensor_stats) is missing")
    return getattr(cvlib, name)


def test_struct_layouts_are_the_documented_ones():
    Row, Stat = lib_name("TraceRow"), lib_name("TensorStat")
    assert C.sizeof(Row) == 128
    assert [(n, getattr(Row, n).offset) for n, _ in Row._fields_] == [
        ("step", 0), ("lr", 8), ("applied", 12), ("nonfinite", 16), ("grad_norm", 20), ("coef", 24), ("n_scalars", 28),
        ("reserved", 32), ("scalars", 64)]
    assert Row.scalars.size == 64 and Row.reserved.size == 32
    assert C.sizeof(Stat) == 48
    assert [(n, getattr(Stat, n).offset) for n, _ in Stat._fields_] == [
        ("g2", 0), ("p2", 8), ("u2", 16), ("gmax", 24), ("pmax", 28), ("g_nonfinite", 32), ("p_nonfinite", 36), ("step", 40)]
    tr = trace_module()
    assert tr.ROW_DTYPE.itemsize == 128 and tr.STAT_DTYPE.itemsize == 48
    assert {n: tr.ROW_DTYPE.fields[n][1] for n in tr.ROW_DTYPE.names} == {n: getattr(Row, n).offset for n, _ in Row._fields_}
    assert {n: tr.STAT_DTYPE.fields[n][1] for n in tr.STAT_DTYPE.names} == {n: getattr(Stat, n).offset for n, _ in Stat._fields_}
    header = open(os.path.join(ROOT, "include", "cvae.h")).read()
    assert "typedef struct cvae_trace_row" in header and "typedef struct cvae_tensor_stat" in header
    assert "#define CVAE_TRACE_MAX_TENSORS 32" in header and cvlib.TRACE_MAX_TENSORS == 32


def test_tensor_table_of_the_vae():
    tr = trace_module()
    h = cvlib.Handle(64, 4)
    table = tr.tensor_table(h)
    assert len(table) == 30 == len(h.layout) and table == tr.tensor_table(h.layout)
    assert {name for name, _, _ in table} == set(h.layout)
    prev = 0
    for name, b, e in table:
        assert prev <= b < e <= h.param_total and (b, e - b) == tuple(h.layout[name])
        prev = e
    assert sum(e - b for _, b, e in table) == sum(n for _, n in h.layout.values()) < h.param_total      # padding excluded


def test_tensor_table_of_the_critic():
    tr = trace_module()
    from critic_vae_amd.optim import critic_layout
    table = tr.tensor_table(critic_layout())
    assert len(table) == 14 and sum(e - b for _, b, e in table) == 11873 and table[-1][2] == 11873
    assert ("crit.4.bias", 11872, 11873) in table
    with pytest.raises(ValueError):
        tr.tensor_table({"a": (0, 5), "b": (4, 2)})


def hand_ring(tr, capacity, pushed, n_scalars=4):
    """The bytes a ring of `capacity` rows holds after steps 1..pushed were pushed, built by hand."""
    ring = np.zeros(capacity, dtype=tr.ROW_DTYPE)
    for step in range(1, pushed + 1):
        row = ring[(step - 1) % capacity]
        row["step"], row["lr"], row["applied"], row["nonfinite"] = step, 1e-4 * step, step % 2, 1 - step % 2
        row["grad_norm"], row["coef"], row["n_scalars"] = 0.5 * step, 1.0 / step, n_scalars
        row["scalars"][:n_scalars] = np.arange(n_scalars, dtype=np.float32) + 10 * step
    return ring


def test_read_decodes_a_ring_that_wrapped():
    tr = trace_module()
    t = tr.Trace(capacity=4)
    t._ring = torch.from_numpy(hand_ring(tr, 4, 6).view(np.uint8).copy())
    t._pushed, t.n_scalars = 6, 4
    got = t.read()
    assert got["step"].tolist() == [3, 4, 5, 6] and got["dropped"] == 2
    assert got["scalars"].shape == (4, 4) and got["scalars"][:, 0].tolist() == [30.0, 40.0, 50.0, 60.0]
    assert got["applied"].tolist() == [1, 0, 1, 0] and got["nonfinite"].tolist() == [0, 1, 0, 1]
    assert np.array_equal(got["lr"], (1e-4 * np.arange(3, 7)).astype(np.float32))
    assert np.array_equal(got["grad_norm"], np.array([1.5, 2.0, 2.5, 3.0], np.float32))
    assert got["tensors"]["tensor_step"].size == 0 and got["tensors"]["dropped"] == 0


def test_read_decodes_tensor_rows_in_step_order():
    tr = trace_module()
    names = ["a.w", "a.b", "c.w"]
    ring = np.zeros((2, 3), dtype=tr.STAT_DTYPE)
    for row, step in ((0, 30), (1, 20)):                  # the ring wrapped: row 0 holds the newer step
        ring[row]["step"] = step
        ring[row]["g2"], ring[row]["p2"], ring[row]["u2"] = [4.0, 9.0, 16.0], [1.0, 4.0, 0.0], [0.25, 1.0, 0.0]
        ring[row]["g_nonfinite"] = [0, step, 0]
    got = tr.decode(np.zeros(0, np.uint8), 0, ring.view(np.uint8).reshape(-1), 3, names)["tensors"]
    assert got["tensor_step"].tolist() == [20, 30] and got["dropped"] == 1 and got["names"] == names
    assert got["grad_norm"].tolist() == [[2.0, 3.0, 4.0]] * 2 and got["weight_norm"].tolist() == [[1.0, 2.0, 0.0]] * 2
    assert got["update_ratio"][0, :2].tolist() == [0.5, 0.5] and np.isnan(got["update_ratio"][0, 2])
    assert got["grad_nonfinite"][:, 1].tolist() == [20, 30]


def test_save_merges_into_an_existing_file(tmp_path):
    tr = trace_module()
    path = str(tmp_path / "trace.npz")

    def trace_of(first, last):
        t = tr.Trace(capacity=16)
        ring = np.zeros(16, dtype=tr.ROW_DTYPE)
        for k, step in enumerate(range(first, last + 1)):
            ring[k]["step"], ring[k]["n_scalars"] = step, 4
            ring[k]["scalars"][:4] = step + 0.5 * first
        t._ring, t._pushed, t.n_scalars = torch.from_numpy(ring.view(np.uint8).copy()), last - first + 1, 4
        return t

    trace_of(1, 6).save(path)
    with np.load(path) as f:
        assert f["step"].tolist() == [1, 2, 3, 4, 5, 6]
    trace_of(5, 8).save(path)                             # a run resumed from step 4: the file's rows 5, 6 are dropped
    with np.load(path) as f:
        assert f["step"].tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
        assert f["scalars"][:, 0].tolist() == [1.5, 2.5, 3.5, 4.5, 7.5, 8.5, 9.5, 10.5]
    other = trace_of(1, 2)
    other.n_scalars = 3                                   # another layout: the file is replaced, not merged
    other.save(path)
    with np.load(path) as f:
        assert f["step"].tolist() == [1, 2] and f["scalars"].shape == (2, 3)


def test_the_file_prints_as_a_table(tmp_path):
    tr = trace_module()
    names = ["enc0.w", "enc0.b"]
    ring = np.zeros((1, 2), dtype=tr.STAT_DTYPE)
    ring[0]["step"], ring[0]["g2"], ring[0]["p2"], ring[0]["u2"], ring[0]["g_nonfinite"] = 7, [4.0, 1.0], [16.0, 4.0], [1.0, 0.0], [0, 3]
    data = tr.decode(hand_ring(tr, 4, 3).view(np.uint8), 3, ring.view(np.uint8).reshape(-1), 1, names)
    path = str(tmp_path / "t.npz")
    np.savez(path, **tr.flatten(data))
    r = subprocess.run([sys.executable, "-m", "critic_vae_amd.trace", path], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in names]
    assert len(rows) == 2 and rows[1].split()[-1] == "3" and float(rows[0].split()[3]) == 0.25
    assert "3 steps held (1..3)" in r.stdout and "step 7" in r.stdout


def test_argument_checks():
    tr = trace_module()
    for kw in (dict(capacity=0), dict(capacity=-3), dict(every=-1), dict(tensors_every=-2), dict(tensors_every=5, tensor_capacity=0)):
        with pytest.raises(ValueError):
            tr.Trace(**kw)
    t = tr.Trace(capacity=8, every=2, tensors_every=100)
    assert t.tensor_capacity == 1                          # at least one row, however rare the tensor rows
    assert tr.Trace(capacity=100, every=1, tensors_every=10).tensor_capacity == 10
    assert tr.Trace().tensors_every == 0 and tr.Trace().tensor_capacity == 0
    from critic_vae_amd import fit
    for bad in ("yes", 3, object()):
        with pytest.raises(ValueError):
            fit.DeviceTrainer()._init_shared(False, None, None, bad)


def test_trace_flags_of_the_command_line():
    from critic_vae_amd import train as T
    ap = T.build_parser()
    args = ap.parse_args(["-train", "--trace-out", "x.npz", "--trace-every", "2", "--trace-tensors-every", "10", "--trace-capacity", "64"])
    t = T.trace_from_args(args)
    assert (t.capacity, t.every, t.tensors_every) == (64, 2, 10)
    assert T.trace_from_args(ap.parse_args(["-train"])) is None
    with pytest.raises(ValueError):
        T.trace_from_args(ap.parse_args(["-train", "--trace-every", "2"]))
    with pytest.raises(SystemExit):                        # the synthetic -train loop is the reference's own: no trace
        T.main(["-train", "--trace-out", "x.npz"])


def test_plan_and_scratch_bytes_are_host_only():
    plan, scratch = lib_name("tensor_stats_plan"), lib_name("tensor_stats_scratch_bytes")
    one = plan([(0, 1)])
    CH = one["chunk"]
    assert CH >= 4 and one["items"] == 1 and one["grid"] == 1
    table = [(0, CH - 1), (CH, 2 * CH), (2 * CH + 3, 3 * CH + 4), (4 * CH, 6 * CH + 7)]
    p = plan(table)
    assert p == {"chunk": CH, "items": 1 + 1 + 2 + 3, "grid": 7}
    big = plan([(5, 5 + 1000 * CH + 1)])
    assert big["items"] == 1001 and 1 <= big["grid"] <= 256
    assert scratch(table) >= 7 * 40 and scratch(table) % 16 == 0 and scratch(table) < scratch([(5, 5 + 1000 * CH + 1)])
    for bad in ([], [(0, 1)] * 33, [(3, 3)], [(4, 2)], [(0, 5), (4, 9)], [(10, 12), (0, 3)]):
        with pytest.raises(cvlib.CvaeError):
            plan(bad)
        with pytest.raises(cvlib.CvaeError):
            scratch(bad)
    assert plan([(k, k + 1) for k in range(32)])["items"] == 32


def test_reference_x_axis():
    tr = trace_module()
    assert [tr.reference_x(s, 128) for s in (1, 2, 31)] == [0, 128, 3840]
    assert [tr.reference_x(s, 4, num_samples=10) for s in (1, 2, 3, 4, 5)] == [0, 4, 8, 10, 14]      # batch_i + num_samples * ep


def test_to_tensorboard_writes_the_reference_tags(tmp_path):
    pytest.importorskip("torch.utils.tensorboard")
    tr = trace_module()
    data = tr.decode(hand_ring(tr, 4, 3, n_scalars=16).view(np.uint8), 3, np.zeros(0, np.uint8), 0, [])
    out = tr.Trace().to_tensorboard(str(tmp_path / "tb"), batch_size=4, data=data)
    assert any(name.startswith("events.out") for name in os.listdir(out))
