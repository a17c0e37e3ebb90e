"""The training trace through both trainers on the GPU: width 64, B = 4, five steps from the generator's seed-0 weights on
synthetic frames (the reference's real frames where a test says so).  The trace only reads; its rows are what step() returned;
its per-tensor sums agree with the guard's global norm and with the displacement the parameters actually took; skipped steps
name their tensors; the ring wraps; fit_device reads nothing on the host; the command line writes, prints and continues a file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from critic_vae_amd import critic_train as CT
from critic_vae_amd import episodes as E
from critic_vae_amd import lib as cvlib
from critic_vae_amd import synth
from critic_vae_amd import train as T
from critic_vae_amd.critic import Critic
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.objective import Objective
from critic_vae_amd.optim import Optim
from critic_vae_amd.train import FusedTrainer
from oracle import cvae_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
B, STEPS = 4, 5


def trace_module():
    try:
        from critic_vae_amd import trace
    except ImportError as e:
        pytest.fail(f"critic_vae_amd.trace is missing ({e}): no training trace")
    return trace


def with_trace(cls, model, trace, **kw):
    try:
        return cls(model, trace=trace, **kw)
    except TypeError as e:
        pytest.fail(f"{cls.__name__} takes no trace ({e}): fit_device keeps no training curve")


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def same(a, b):
    return torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def batches():
    return tuple(tuple(torch.from_numpy(t).to(DEV).contiguous() for t in synth.make_batch(77, s, B)) for s in range(STEPS + 1))


def vae_trainer(precision="f32", trace=None, **kw):
    vae = VariationalAutoencoder(max_batch=B, seed=0, precision=precision).to(DEV)
    vae.load_reference_params(synth.make_params(0))
    return FusedTrainer(vae, **kw) if trace is None else with_trace(FusedTrainer, vae, trace, **kw)


def vae_run(tr, steps=STEPS):
    rows = [tr.step(*batches()[s % (STEPS + 1)]).clone() for s in range(steps)]
    torch.cuda.synchronize()
    return rows


def vae_state(tr):
    return [tr.vae.theta.data, tr.m, tr.v, tr.vae.bn_state]


@functools.lru_cache(maxsize=None)
def critic_fixture():
    gen = torch.Generator().manual_seed(11)
    x = torch.rand(STEPS * B, 3, 64, 64, generator=gen).to(DEV)
    target = torch.linspace(0.1, 0.9, STEPS * B).to(DEV)
    keep = (torch.rand(STEPS * B, cvlib.CRITIC_KEEP, generator=gen) >= 0.3).to(torch.uint8).to(DEV)
    return cvlib.Handle(64, 16), x, target, keep


def critic_trainer(trace=None, **kw):
    critic = Critic(handle=critic_fixture()[0]).to(DEV)
    critic.load_state_dict(CT.initial_state_dict(0))
    return CT.CriticTrainer(critic, **kw) if trace is None else with_trace(CT.CriticTrainer, critic, trace, **kw)


def critic_run(tr, steps=STEPS):
    _, x, target, keep = critic_fixture()
    rows = [tr.step(x[s * B:(s + 1) * B], target[s * B:(s + 1) * B], keep=keep[s * B:(s + 1) * B].contiguous()).clone() for s in range(steps)]
    torch.cuda.synchronize()
    return rows


def full_trace():
    return trace_module().Trace(every=1, tensors_every=1)


OPTIM = dict(lr=2e-4, optim=Optim(schedule="cosine", warmup=2, total=STEPS, lr_min=1e-5, weight_decay=0.05, ema=0.9))
GUARD = dict(skip_nonfinite=True, max_grad_norm=1.0)


# ---- 1. the trace only reads ----
VAE_CASES = [(p, k) for p in ("f32", "bf16") for k in ("plain", "guard", "optim", "guard+optim")] + [("f32", "global")]
VAE_KW = {"plain": {}, "guard": GUARD, "optim": OPTIM, "guard+optim": dict(GUARD, **OPTIM), "global": dict(global_stats=True)}


@pytest.mark.parametrize("precision,case", VAE_CASES)
def test_vae_trainer_with_a_trace_computes_the_same_bits(precision, case):
    kw = VAE_KW[case]
    a, b = vae_trainer(precision, **kw), vae_trainer(precision, trace=full_trace(), **kw)
    ra, rb = vae_run(a), vae_run(b)
    assert torch.isfinite(a.vae.theta.data).all(), "the run itself went non-finite: equal bits would show nothing"
    assert all(same(s, t) for s, t in zip(vae_state(a), vae_state(b)))
    assert all(same(s, t) for s, t in zip(ra, rb))
    if "optim" in kw:
        assert same(a.ema, b.ema) and same(a.aux_ema, b.aux_ema)
    if "skip_nonfinite" in kw:
        assert a.guard_stats() == b.guard_stats()
    got = b.trace.read()
    assert got["step"].tolist() == [1, 2, 3, 4, 5] and got["tensors"]["tensor_step"].tolist() == [1, 2, 3, 4, 5]
    assert len(got["tensors"]["names"]) == 30 and got["dropped"] == 0
    assert "trace" not in b.state_dict() and set(a.state_dict()) == set(b.state_dict())


@pytest.mark.parametrize("kw", [{}, GUARD, OPTIM], ids=["plain", "guard", "optim"])
def test_critic_trainer_with_a_trace_computes_the_same_bits(kw):
    a, b = critic_trainer(**kw), critic_trainer(trace=full_trace(), **kw)
    ra, rb = critic_run(a), critic_run(b)
    assert torch.isfinite(a.theta).all()
    assert all(same(s, t) for s, t in zip((a.theta, a.m, a.v), (b.theta, b.m, b.v))) and all(same(s, t) for s, t in zip(ra, rb))
    got = b.trace.read()
    assert got["scalars"].shape == (5, 4) and len(got["tensors"]["names"]) == 14 and "crit.4.bias" in got["tensors"]["names"]
    assert np.array_equal(got["scalars"].view(np.int32), torch.stack(rb).cpu().numpy().view(np.int32))
    if kw is GUARD:
        assert np.array_equal(got["applied"], np.ones(5, np.int32)) and np.isfinite(got["grad_norm"]).all()
    else:
        assert np.isnan(got["grad_norm"]).all() and (got["coef"] == 1.0).all() and (got["applied"] == 1).all()


def test_wrong_trace_type_raises():
    trace_module()
    vae = VariationalAutoencoder(max_batch=B, seed=0).to(DEV)
    with pytest.raises(ValueError):
        FusedTrainer(vae, trace="curve.npz")
    t = full_trace()
    vae_run(vae_trainer(trace=t), 1)
    with pytest.raises(RuntimeError):                       # one Trace per trainer
        vae_run(vae_trainer(trace=t), 1)


# ---- 2. step rows ----
def test_step_rows_are_what_step_returned():
    tr = vae_trainer(trace=full_trace(), **OPTIM)
    rows = vae_run(tr)
    got = tr.trace.read()
    assert got["step"].tolist() == [1, 2, 3, 4, 5] and got["scalars"].shape == (5, 16)
    assert np.array_equal(got["scalars"].view(np.int32), torch.stack(rows).cpu().numpy().view(np.int32))
    want = np.array([OPTIM["optim"].lr_at(s, OPTIM["lr"]) for s in range(5)], np.float32)
    assert np.array_equal(got["lr"], want) and len(set(want.tolist())) >= 3
    assert (got["applied"] == 1).all() and (got["nonfinite"] == 0).all() and np.isnan(got["grad_norm"]).all()
    every2 = vae_trainer(trace=trace_module().Trace(capacity=2, every=2, tensors_every=3))
    rows = vae_run(every2)
    got = every2.trace.read()
    assert got["step"].tolist() == [2, 4] and got["tensors"]["tensor_step"].tolist() == [3] and got["dropped"] == 0
    assert np.array_equal(got["scalars"].view(np.int32), torch.stack([rows[1], rows[3]]).cpu().numpy().view(np.int32))


# ---- 3. the guard's norm from the per-tensor sums ----
@pytest.mark.parametrize("which", ["vae", "critic"])
def test_tensor_sums_agree_with_the_guard_record(which):
    """sqrt(sum_t g2_t) against the record's norm64: the same squares (g * gscale in fp32 against g in fp64 times the scale:
    equal when the clip leaves gscale a power of two, here 1.0 — max_grad_norm is far above the norm) in another order, the
    padding is zero; n additions of non-negative terms differ by at most n * 2^-52 relative."""
    tr = (vae_trainer if which == "vae" else critic_trainer)(trace=full_trace(), skip_nonfinite=True, max_grad_norm=1e30)
    (vae_run if which == "vae" else critic_run)(tr)
    rec, got = tr.h.guard_record(tr.guard), tr.trace.read()
    g2 = (got["tensors"]["grad_norm"][-1].astype(np.float64) ** 2).sum()
    n = tr.m.numel()
    assert rec.apply == 1 and rec.coef == 1.0 and np.isfinite(rec.norm64) and rec.norm64 > 0
    err = abs(np.sqrt(g2) - rec.norm64) / rec.norm64
    print(f"{which}: norm64 {rec.norm64!r} from the tensors {np.sqrt(g2)!r} rel err {err:.3e} (bound {n * 2.0 ** -52:.3e})")
    assert err <= n * 2.0 ** -52
    assert got["grad_norm"][-1] == np.float32(rec.norm64) and got["coef"][-1] == 1.0


# ---- 4. the displacement the parameters took ----
@pytest.mark.parametrize("which", ["vae", "critic"])
def test_update_norm_is_the_displacement(which):
    """| ||p_after - p_before|| - sqrt(u2) | <= sqrt(n_t) * 2^-24 * pmax_t + 8 * 2^-24 * sqrt(u2): p_after = fl(p_before - u) is
    off by at most half an ulp of p per element (2^-24 |p|), n_t of them give sqrt(n_t) times that in the norm through the
    triangle inequality; the second term is u's own rounding (three fp32 roundings, test_gpu_trace_ops).  No weight decay."""
    tr = (vae_trainer if which == "vae" else critic_trainer)(trace=full_trace())
    run = vae_run if which == "vae" else critic_run
    theta = tr.vae.theta.data if which == "vae" else tr.theta
    run(tr, STEPS - 1)
    before = theta.detach().cpu().numpy().astype(np.float64)
    if which == "vae":
        tr.step(*batches()[STEPS - 1])
    else:
        _, x, target, keep = critic_fixture()
        s = STEPS - 1
        tr.step(x[s * B:(s + 1) * B], target[s * B:(s + 1) * B], keep=keep[s * B:(s + 1) * B].contiguous())
    torch.cuda.synchronize()
    after = theta.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(after).all()
    t = tr.trace.read()["tensors"]
    assert t["tensor_step"][-1] == STEPS
    for k, (name, b, e) in enumerate(tr.trace.table):
        moved, u = np.sqrt(((after[b:e] - before[b:e]) ** 2).sum()), t["update_norm"][-1, k]
        bound = np.sqrt(e - b) * 2.0 ** -24 * t["weight_max"][-1, k] + 8 * 2.0 ** -24 * u
        print(f"{name}: moved {moved:.6e} update_norm {u:.6e} diff {abs(moved - u):.3e} bound {bound:.3e}")
        assert abs(moved - u) <= bound, name
        p2 = (after[b:e] ** 2).sum()                        # exact squares; the order of e - b additions, and sqrt and its square back
        assert abs(t["weight_norm"][-1, k] ** 2 - p2) <= ((e - b) + 2) * 2.0 ** -52 * p2, name
        assert t["weight_max"][-1, k] == np.abs(after[b:e]).max() and t["weight_nonfinite"][-1, k] == 0


# ---- 5. skipped steps name their tensors: the reference's real frames under its own objective ----
def test_skipped_steps_on_the_real_frames(golden_dir):
    fx = np.load(os.path.join(golden_dir, "step_real_b68.npz"))
    n, wseed = 5, int(fx["wseed"])
    x = orc.preprocess_frames(torch.from_numpy(fx["u8"][:n])).cuda()
    pred = torch.from_numpy(fx["pred"][:n]).reshape(n, 1).float().cuda().contiguous()
    eps = torch.from_numpy(synth.make_batch(int(fx["dseed"]), int(fx["step"]), 68)[2][:n]).cuda().contiguous()

    def model():
        vae = VariationalAutoencoder(max_batch=n, seed=wseed).cuda()
        vae.load_reference_params(synth.make_params(wseed))
        return vae

    tr = with_trace(FusedTrainer, model(), full_trace(), skip_nonfinite=True)
    for _ in range(3):
        tr.step(x, pred, eps)
    got = tr.trace.read()
    t = got["tensors"]
    assert got["applied"].tolist() == [0, 0, 0] and got["nonfinite"].tolist() == [1, 1, 1]
    assert (t["grad_nonfinite"] > 0).any(axis=1).all() and (t["update_norm"] == 0).all()
    step, names = trace_module().nonfinite_tensors(got)
    assert step == 3 and names and set(names) <= set(t["names"])
    print(f"non-finite gradients in {names}")
    tr = with_trace(FusedTrainer, model(), full_trace(), skip_nonfinite=True, objective=Objective(msssim_grad="used"))
    for _ in range(3):
        tr.step(x, pred, eps)
    got = tr.trace.read()
    assert got["applied"].tolist() == [1, 1, 1] and (got["tensors"]["grad_nonfinite"] == 0).all()
    assert np.isfinite(got["tensors"]["update_norm"]).all() and (got["tensors"]["update_norm"] > 0).any(axis=1).all()
    assert trace_module().nonfinite_tensors(got) is None


# ---- 6. the ring wraps ----
def test_ring_wraps_through_the_trainer():
    tr = vae_trainer(trace=trace_module().Trace(capacity=4, every=1, tensors_every=2, tensor_capacity=2))
    rows = vae_run(tr, 6)
    got = tr.trace.read()
    assert got["step"].tolist() == [3, 4, 5, 6] and got["dropped"] == 2
    assert np.array_equal(got["scalars"].view(np.int32), torch.stack(rows[2:]).cpu().numpy().view(np.int32))
    assert got["tensors"]["tensor_step"].tolist() == [4, 6] and got["tensors"]["dropped"] == 1


# ---- 7. fit_device reads nothing on the host ----
class CountingHandle:
    """Every call of a Handle method, by name, as the host fit-loop tests record their stand-in trainer's events."""

    def __init__(self, h):
        self._h, self.calls = h, []

    def __getattr__(self, name):
        attr = getattr(self._h, name)
        if not callable(attr) or name.startswith("_"):
            return attr

        def counted(*a, **kw):
            self.calls.append(name)
            return attr(*a, **kw)
        return counted


@functools.lru_cache(maxsize=None)
def small_dataset():
    gen = torch.Generator().manual_seed(3)
    n = 3 * B
    frames = torch.randint(0, 256, (n, 64, 64, 3), generator=gen, dtype=torch.uint8)
    source = np.stack([np.zeros(n, np.int64), np.arange(n, dtype=np.int64)], 1)
    return E.DeviceDataset(frames.to(DEV), torch.rand(n, 1, generator=gen).to(DEV), source)


@pytest.mark.parametrize("which", ["vae", "critic"])
def test_fit_device_with_a_trace_reads_nothing(which, monkeypatch):
    make = vae_trainer if which == "vae" else critic_trainer
    copies = []
    for name in ("cpu", "item", "tolist", "numpy"):
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _real=real, _name=name, **kw: (copies.append(_name), _real(self, *a, **kw))[1])
    logs = []
    for trace in (None, trace_module().Trace(every=1, tensors_every=2)):
        tr = make(trace=trace, **GUARD)
        tr.h = CountingHandle(tr.h)
        np.random.seed(5)
        gen = torch.Generator(device=DEV)
        gen.manual_seed(5)
        del copies[:]
        tr.fit_device(small_dataset(), B, epochs=2, generator=gen)
        logs.append((list(tr.h.calls), list(copies), tr))
    (plain_calls, plain_copies, _), (calls, fit_copies, tr) = logs
    assert fit_copies == plain_copies, "the trace added a host read to fit_device"
    assert "guard_record" not in calls
    assert [c for c in calls if c not in ("trace_push", "tensor_stats")] == plain_calls
    assert calls.count("trace_push") == 6 and calls.count("tensor_stats") == 3
    del copies[:]
    got = tr.trace.read()
    assert copies.count("cpu") == 2 and "item" not in copies and "tolist" not in copies      # one copy per ring, nothing else
    assert got["step"].tolist() == [1, 2, 3, 4, 5, 6] and got["tensors"]["tensor_step"].tolist() == [2, 4, 6]


# ---- 8. the command line ----
def test_trace_out_round_trip(tmp_path, golden_dir, capsys):
    trace_module()
    fx = np.load(os.path.join(golden_dir, "step_real_b68.npz"))
    cw = np.load(os.path.join(golden_dir, "critic_real_b8.npz"))
    d = tmp_path / "eps"
    d.mkdir()
    np.save(d / "ep_a.npy", fx["u8"][:40])
    pt, save, out = tmp_path / "critic.pt", tmp_path / "out", tmp_path / "trace.npz"
    torch.save({k[2:]: torch.from_numpy(cw[k]) for k in cw.files if k.startswith("w/")}, pt)
    common = ["-train", "--episodes", str(d), "--critic", str(pt), "--epochs", "2", "--batch", "8", "--save", str(save),
              "--skip-nonfinite", "--msssim-grad", "used", "--trace-out", str(out), "--trace-tensors-every", "2"]
    T.main(common)
    text = capsys.readouterr().out
    assert f"saved {out}" in text
    with np.load(out) as f:
        steps, tsteps = f["step"].tolist(), f["tensor_step"].tolist()
        assert steps == list(range(1, len(steps) + 1)) and len(steps) >= 2 and tsteps == list(range(2, len(steps) + 1, 2))
        assert f["scalars"].shape == (len(steps), 16) and f["grad_norm_t"].shape == (len(tsteps), 30)
    r = subprocess.run([sys.executable, "-m", "critic_vae_amd.trace", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    names = set(cvlib.Handle(64, 4).layout)
    assert len([ln for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in names]) == 30
    assert f"{len(steps)} steps held" in r.stdout
    T.main(common + ["--resume", str(save)])
    with np.load(out) as f:
        assert f["step"].tolist() == list(range(1, 2 * len(steps) + 1))
        assert f["tensor_step"].tolist() == list(range(2, 2 * len(steps) + 1, 2))
