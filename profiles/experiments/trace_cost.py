"""What the training trace costs: cvae_trace_push alone, cvae_tensor_stats at the VAE's flat buffers (30 tensors) and at the
critic's (14), a torch route to the same numbers for scale (per-tensor slices: norm of g, p and the recomputed update, abs().max(),
isfinite — all on the device, nothing read), and one fit_device epoch of each trainer with and without
Trace(every=1, tensors_every=100) — same process, same buffers, variants alternating; HIP events around 20 calls, median of 7
(the epochs: wall time around one synchronised epoch, median of 7).

    python profiles/experiments/trace_cost.py [OUT.txt]
"""
import os, sys, statistics, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from critic_vae_amd import critic_train as CT
from critic_vae_amd import episodes as E
from critic_vae_amd import lib as cvlib
from critic_vae_amd import params as P
from critic_vae_amd.critic import Critic
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.optim import critic_layout
from critic_vae_amd.trace import Trace, tensor_table
from critic_vae_amd.train import FusedTrainer
dev = torch.device("cuda:0")
N, REPS = 20, 7


def events(f):
    """ms per call: events around N calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        f()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / N


def wall(f):
    """ms of one synchronised call"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def interleaved(fs, measure=events, warm=3):
    """REPS alternating rounds of every variant after a warm-up of each -> list of sample lists"""
    for f in fs:
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    out = [[] for _ in fs]
    for _ in range(REPS):
        for k, f in enumerate(fs):
            out[k].append(measure(f))
    return out


def report(lines, variants, samples, unit=1e3, name="us"):
    base = statistics.median(samples[0])
    for (label, _), s in zip(variants, samples):
        med = statistics.median(s)
        lines.append(f"  {label:<66s} {' '.join(f'{x * unit:.1f}' for x in s)} | median {med * unit:.1f} {name} ({(med - base) * unit:+.1f}), "
                     f"spread {min(s) * unit:.1f}..{max(s) * unit:.1f}")


h = cvlib.Handle(64, 64)
lines = []

# ---- the step row ----
ring = torch.zeros(4096 * 128, dtype=torch.uint8, device=dev)
scal = torch.rand(16, device=dev)
state = h.guard_state(dev)
h.grad_stats(torch.rand(1024, device=dev), state, 1.0, 1e30, True, P.lr)
step = [0]


def push(guard):
    def f():
        step[0] += 1
        h.trace_push(ring, 4096, step[0], P.lr, scal, 16, guard=guard)
    return f


variants = [("cvae_trace_push, no guard state", push(None)), ("cvae_trace_push, with a guard state", push(state))]
lines.append("cvae_trace_push: one 128-byte row; us per call, 7 samples of 20 calls each, then the median")
report(lines, variants, interleaved([f for _, f in variants]))

# ---- the tensor pass ----
for what, n, table in (("VAE", h.param_total, tensor_table(h)), ("critic", cvlib.CRITIC_TRAIN_FLOATS, tensor_table(critic_layout()))):
    ranges = [(b, e) for _, b, e in table]
    th, gr, m, v = (torch.zeros(n, device=dev) for _ in range(4))
    th.uniform_(-1, 1); gr.uniform_(-1e-3, 1e-3); m.uniform_(-1e-3, 1e-3); v.uniform_(0, 1e-6)
    out = torch.zeros(len(ranges) * 48, dtype=torch.uint8, device=dev)
    scratch = torch.empty(cvlib.tensor_stats_scratch_bytes(ranges), dtype=torch.uint8, device=dev)
    res = torch.zeros(len(ranges), 7, device=dev)
    plan = cvlib.tensor_stats_plan(ranges)

    def torch_route():
        for k, (b, e) in enumerate(ranges):
            g, p = gr[b:e], th[b:e]
            u = 1e-4 * (m[b:e] / (v[b:e].sqrt() / 0.03 + 1e-8))
            res[k, 0], res[k, 1], res[k, 2] = g.norm(), p.norm(), u.norm()
            res[k, 3], res[k, 4] = g.abs().max(), p.abs().max()
            res[k, 5], res[k, 6] = (~torch.isfinite(g)).sum(), (~torch.isfinite(p)).sum()

    variants = [
        ("cvae_tensor_stats", lambda: h.tensor_stats(th, gr, m, v, ranges, 3, out, scratch, lr=P.lr)),
        ("cvae_tensor_stats, with a guard state", lambda: h.tensor_stats(th, gr, m, v, ranges, 3, out, scratch, lr=P.lr, guard=state)),
        ("cvae_adam_step on the same buffers, for scale", lambda: h.adam_step(th, gr, m, v, 3, P.lr)),
        (f"torch route: {len(ranges)} slices x (3 norms, 2 abs().max(), 2 isfinite counts)", torch_route),
    ]
    lines.append(f"{what}: n = {n} floats, {len(ranges)} tensors, chunk {plan['chunk']}, {plan['items']} items on {plan['grid']} workgroups; "
                 "us per call, 7 samples of 20 calls each, then the median")
    report(lines, variants, interleaved([f for _, f in variants]))

# ---- one fit_device epoch of each trainer, with and without a trace ----
B, STEPS = 64, 100
gen = torch.Generator().manual_seed(1)
frames = torch.randint(0, 256, (B * STEPS, 64, 64, 3), generator=gen, dtype=torch.uint8).to(dev)
preds = torch.rand(B * STEPS, 1, generator=gen).to(dev)
ds = E.DeviceDataset(frames, preds, np.stack([np.zeros(B * STEPS, np.int64), np.arange(B * STEPS, dtype=np.int64)], 1))


def vae_trainer(trace):
    return FusedTrainer(VariationalAutoencoder(max_batch=B, seed=0).to(dev), skip_nonfinite=True, trace=trace)


def critic_trainer(trace):
    critic = Critic(handle=h).to(dev)
    critic.load_state_dict(CT.initial_state_dict(0))
    return CT.CriticTrainer(critic, trace=trace)


for what, make in (("FusedTrainer (guarded: noise frames give non-finite gradients)", vae_trainer), ("CriticTrainer", critic_trainer)):
    plain, traced = make(None), make(Trace(every=1, tensors_every=100))
    g = torch.Generator(device=dev)
    variants = [("fit_device, no trace", lambda: plain.fit_device(ds, B, epochs=1, generator=g)),
                ("fit_device, Trace(every=1, tensors_every=100)", lambda: traced.fit_device(ds, B, epochs=1, generator=g))]
    lines.append(f"{what}: one fit_device epoch of {STEPS} steps at B = {B}; ms per epoch (wall, synchronised), 7 alternating samples, then the median")
    report(lines, variants, interleaved([f for _, f in variants], measure=wall, warm=1), unit=1.0, name="ms")
    got = traced.trace.read()
    assert len(got["step"]) == min(4096, traced.step_count) and len(got["tensors"]["tensor_step"]) >= 1
with open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w") as f:
    for line in lines:
        print(line, flush=True); f.write(line + "\n")
