"""What the optimizer options cost in the Adam pass itself: cvae_adam_step against cvae_adam_step_opt with decay only (the
VAE's 11 ranges / the critic's 7), with an EMA only, with everything, the guarded forms of the same, and a torch route to the
same result for scale (masked mul_ + cvae_adam_step + lerp_ + the bn_state lerp) — same process, same buffers, variants
alternating; HIP events around 20 calls, median of 7 — at the VAE's flat n and at the critic's.

    python profiles/experiments/optim_cost.py [OUT.txt]
"""
import os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from critic_vae_amd import lib as cvlib
from critic_vae_amd import params as P
from critic_vae_amd.optim import Optim, critic_layout, decay_ranges
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


def interleaved(fs):
    """REPS alternating rounds of every variant after a warm-up of each -> list of sample lists"""
    for f in fs:
        f(); f(); f()
    torch.cuda.synchronize()
    out = [[] for _ in fs]
    for _ in range(REPS):
        for k, f in enumerate(fs):
            out[k].append(events(f))
    return out


h = cvlib.Handle(64, 4)
lines = []
for what, n, ranges, n_aux in (("VAE", h.param_total, decay_ranges(h.layout), h.bn_state_floats),
                               ("critic", cvlib.CRITIC_TRAIN_FLOATS, decay_ranges(critic_layout()), 0)):
    th, gr, m, v, ema = (torch.zeros(n, device=dev) for _ in range(5))
    th.uniform_(-1, 1); gr.uniform_(-1e-3, 1e-3); ema.copy_(th)
    aux = torch.rand(n_aux, device=dev) if n_aux else None
    aux_ema = aux.clone() if n_aux else None
    mask = torch.zeros(n, dtype=torch.bool, device=dev)
    for b, e in ranges:
        mask[b:e] = True
    views = [th[b:e] for b, e in ranges]
    o = Optim(weight_decay=0.01, ema=0.999)
    a = o.args_at(0, P.lr, ranges)
    decay = cvlib.opt_args(a["decay_mul"], 0.0, ranges)
    none = cvlib.opt_args(1.0, 0.0, [])
    ema_only = cvlib.opt_args(1.0, a["ema_omd"], [])
    full = cvlib.opt_args(a["decay_mul"], a["ema_omd"], ranges)
    state = h.guard_state(dev)

    def guarded(opt, **kw):
        def f():
            h.grad_stats(gr, state, 1.0, 1e30, True, P.lr)
            if opt is None:
                h.adam_step_guarded(th, gr, m, v, state)
            else:
                h.adam_step_guarded_opt(th, gr, m, v, state, opt=opt, **kw)
        return f

    def torch_route():
        for t in views:
            t.mul_(a["decay_mul"])
        h.adam_step(th, gr, m, v, 1, P.lr)
        ema.lerp_(th, a["ema_omd"])
        if aux is not None:
            aux_ema.lerp_(aux, a["ema_omd"])

    variants = [
        ("cvae_adam_step", lambda: h.adam_step(th, gr, m, v, 1, P.lr)),
        ("_opt, nothing on", lambda: h.adam_step_opt(th, gr, m, v, 1, P.lr, opt=none)),
        (f"_opt, decay only ({len(ranges)} ranges)", lambda: h.adam_step_opt(th, gr, m, v, 1, P.lr, opt=decay)),
        ("_opt, EMA only", lambda: h.adam_step_opt(th, gr, m, v, 1, P.lr, opt=ema_only, ema=ema, aux=aux, aux_ema=aux_ema)),
        ("_opt, decay + EMA", lambda: h.adam_step_opt(th, gr, m, v, 1, P.lr, opt=full, ema=ema, aux=aux, aux_ema=aux_ema)),
        ("grad_stats + guarded", guarded(None)),
        ("grad_stats + guarded_opt, decay only", guarded(decay)),
        ("grad_stats + guarded_opt, decay + EMA", guarded(full, ema=ema, aux=aux, aux_ema=aux_ema)),
        (f"torch route: {len(views)} mul_ + cvae_adam_step + lerp_" + (" + bn_state lerp_" if n_aux else ""), torch_route),
    ]
    samples = interleaved([f for _, f in variants])
    base = statistics.median(samples[0])
    lines.append(f"{what}: n = {n} floats, {len(ranges)} decayed ranges, n_aux = {n_aux}; us per call, 7 samples of 20 calls each, then the median")
    for (name, _), s in zip(variants, samples):
        med = statistics.median(s)
        lines.append(f"  {name:<62s} {' '.join(f'{x * 1e3:.1f}' for x in s)} | median {med * 1e3:.1f} us ({(med - base) * 1e3:+.1f} us), "
                     f"spread {min(s) * 1e3:.1f}..{max(s) * 1e3:.1f}")
    assert bool(torch.isfinite(th).all()) and bool(torch.isfinite(ema).all())
with open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w") as f:
    for line in lines:
        print(line, flush=True); f.write(line + "\n")
