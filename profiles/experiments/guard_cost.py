"""What the guarded step costs: FusedTrainer(skip_nonfinite=True, max_grad_norm=...) against the plain trainer, same process,
same inputs, alternating — HIP events around 20 steps, median of 7 — at fp32 B = 256 and bf16 B = 2048, then the optimizer
tail alone (cvae_adam_step against cvae_grad_stats + cvae_adam_step_guarded) and the statistics pass on 4 floats (its
launch floor) against the whole flat gradient (floor + the extra read).

    python profiles/experiments/guard_cost.py [OUT.txt]
"""
import os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from critic_vae_amd import params as P
from critic_vae_amd.nets import VariationalAutoencoder
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


def interleaved(fa, fb):
    """REPS alternating rounds of fa, fb after a warm-up of each -> (median a, median b, all a, all b)"""
    for f in (fa, fb):
        f(); f(); f()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(REPS):
        a.append(events(fa)); b.append(events(fb))
    return statistics.median(a), statistics.median(b), a, b


def fmt(v):
    return " ".join(f"{x * 1e3:.1f}" for x in v)


lines = []
for prec, B in (("f32", 256), ("bf16", 2048)):
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    pool = [(torch.rand(B, 3, P.w, P.w, device=dev, generator=gen), torch.rand(B, 1, device=dev, generator=gen),
             torch.randn(B, 32, device=dev, generator=gen)) for _ in range(4)]
    plain = FusedTrainer(VariationalAutoencoder(max_batch=B, seed=0, precision=prec).to(dev))
    guard = FusedTrainer(VariationalAutoencoder(max_batch=B, seed=0, precision=prec).to(dev), skip_nonfinite=True, max_grad_norm=1e30)
    k = [0, 0]

    def step(tr, slot):
        tr.step(*pool[k[slot] % 4]); k[slot] += 1

    tp, tg, ap, ag = interleaved(lambda: step(plain, 0), lambda: step(guard, 1))
    st = guard.guard_stats()
    finite = bool(torch.isfinite(plain.vae.theta.data).all()) and bool(torch.isfinite(guard.vae.theta.data).all())
    lines.append(f"{prec} B = {B}: plain step {fmt(ap)} us, median {tp * 1e3:.1f} us; guarded step {fmt(ag)} us, median {tg * 1e3:.1f} us; "
                 f"guarded / plain = {tg / tp:.4f} ({(tg - tp) * 1e3:+.1f} us); applied {st['applied']}, skipped {st['skipped']}, parameters finite: {finite}")
    if prec == "f32":
        h, n = plain.h, plain.grads.numel()
        th, gr, m, v = (torch.zeros(n, device=dev) for _ in range(4))
        gr.uniform_(-1e-3, 1e-3)
        state = h.guard_state(dev)
        small, small_state = torch.ones(4, device=dev), h.guard_state(dev)

        def tail_plain():
            h.adam_step(th, gr, m, v, 1, P.lr)

        def tail_guard():
            h.grad_stats(gr, state, 1.0, 1e30, True, P.lr)
            h.adam_step_guarded(th, gr, m, v, state)

        t0, t1, a0, a1 = interleaved(tail_plain, tail_guard)
        lines.append(f"optimizer tail alone, {n} parameters: cvae_adam_step {fmt(a0)} us, median {t0 * 1e3:.1f} us; cvae_grad_stats + "
                     f"cvae_adam_step_guarded {fmt(a1)} us, median {t1 * 1e3:.1f} us ({(t1 - t0) * 1e3:+.1f} us)")
        t0, t1, a0, a1 = interleaved(lambda: h.grad_stats(small, small_state, 1.0, 1e30, True, P.lr),
                                     lambda: h.grad_stats(gr, state, 1.0, 1e30, True, P.lr))
        lines.append(f"cvae_grad_stats alone: 4 floats (launch floor, one workgroup) {fmt(a0)} us, median {t0 * 1e3:.1f} us; {n} floats = "
                     f"{n * 4 / 1e6:.2f} MB {fmt(a1)} us, median {t1 * 1e3:.1f} us ({n * 4 / t1 / 1e9:.2f} TB/s)")
    del plain, guard, pool
with open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w") as f:
    for line in lines:
        print(line, flush=True); f.write(line + "\n")
