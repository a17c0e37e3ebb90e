"""What cvae_loss_obj costs beside cvae_loss: the same handle, workspace and inputs, the variants alternating in one process —
HIP events around 20 calls, median of 7 rounds — at fp32 B = 256 and bf16-mode B = 2048 (the loss tensors are fp32 in both;
the mode only sizes the workspace).  Variants: cvae_loss itself a second time (its own run-to-run spread), the reference
objective through cvae_loss_obj, the used-terms gradient, the mixed objective (1, 1, 0.001) and pure MSE (0, 1, 0.001).

    python profiles/experiments/objective_cost.py [OUT.txt]
"""
import os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from critic_vae_amd import params as P
from critic_vae_amd.lib import Handle
dev = torch.device("cuda:0")
N, REPS = 20, 7
COPY_TBS = 6.29          # the measured copy rate of the chip (profiles/README.md)


def events(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        f()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / N * 1e3          # us per call


lines = []
for prec, B in (("f32", 256), ("bf16", 2048)):
    h = Handle(P.w, B, precision=prec)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    x = torch.rand(B, 3, P.w, P.w, device=dev, generator=gen)
    recon = 0.7 * x + 0.3 * torch.rand(B, 3, P.w, P.w, device=dev, generator=gen)
    mu, lv = torch.randn(B, 32, device=dev, generator=gen) * 0.5, torch.randn(B, 32, device=dev, generator=gen) * 0.3
    ws = torch.empty(h.workspace_bytes(B) // 4, device=dev)
    scal, d_r, d_mu, d_lv = torch.empty(16, device=dev), torch.empty_like(recon), torch.empty_like(mu), torch.empty_like(lv)

    def obj(o):
        return lambda: h.loss_obj(B, x, mu, lv, recon, ws, o, scal, d_r, d_mu, d_lv)

    def plain():
        h.loss(B, x, mu, lv, recon, ws, scal, d_r, d_mu, d_lv)

    variants = [("cvae_loss", plain), ("cvae_loss again", plain), ("obj reference (1, 0, 0.001)", obj((1.0, 0.0, 0.001, 0))),
                ("obj used gradient", obj((1.0, 0.0, 0.001, 1))), ("obj mixed (1, 1, 0.001)", obj((1.0, 1.0, 0.001, 0))),
                ("obj pure MSE (0, 1, 0.001)", obj((0.0, 1.0, 0.001, 0)))]
    for _, f in variants:
        f(); f(); f()
    torch.cuda.synchronize()
    t = {name: [] for name, _ in variants}
    for _ in range(REPS):
        for name, f in variants:
            t[name].append(events(f))
    base = statistics.median(t["cvae_loss"])
    lo, hi = min(t["cvae_loss"] + t["cvae_loss again"]), max(t["cvae_loss"] + t["cvae_loss again"])
    lines.append(f"{prec} mode, B = {B}: cvae_loss median {base:.1f} us; its own repeats span {lo:.1f} .. {hi:.1f} us ({hi - lo:.1f} us) over {2 * REPS} rounds of {N} calls")
    for name, _ in variants:
        m = statistics.median(t[name])
        lines.append(f"  {name}: {' '.join(f'{v:.1f}' for v in t[name])} us, median {m:.1f} us ({m - base:+.1f} us against cvae_loss; span of cvae_loss's repeats {hi - lo:.1f} us)")
    extra = 2 * x.numel() * 4
    lines.append(f"  mixed objective: x and recon read once more = {extra / 1e6:.1f} MB = {extra / COPY_TBS / 1e6:.1f} us at {COPY_TBS} TB/s; "
                 f"measured {statistics.median(t['obj mixed (1, 1, 0.001)']) - base:+.1f} us")
    lines.append(f"  pure MSE: {statistics.median(t['obj pure MSE (0, 1, 0.001)']):.1f} us against cvae_loss's {base:.1f} us "
                 f"(reads x and recon, writes d_recon = {3 * x.numel() * 4 / 1e6:.1f} MB = {3 * x.numel() * 4 / COPY_TBS / 1e6:.1f} us at {COPY_TBS} TB/s)")
    del ws, x, recon, d_r
with open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w") as f:
    for line in lines:
        print(line, flush=True); f.write(line + "\n")
