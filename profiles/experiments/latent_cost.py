"""What the latent audit costs: cvae_latent_stats at B = 256 and 2048 against a torch route to the same record (fp64 a.T @ a and the
elementwise sums, all on the device, nothing read), cvae_recon_response at 64 frames x 34 variants against the torch expression,
and FusedTrainer.latent_report over 50 000 frames against evaluate — same process, same buffers, variants alternating; HIP
events around 20 calls, median of 7 (the loops: wall time around one synchronised pass, median of 7).

    python profiles/experiments/latent_cost.py [OUT.txt]
"""
import os, sys, statistics, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from critic_vae_amd import episodes as E
from critic_vae_amd import lib as cvlib
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
        lines.append(f"  {label:<66s} {' '.join(f'{x * unit:.1f}' for x in s)} | median {med * unit:.1f} {name} ({med / base:.2f}x), "
                     f"spread {min(s) * unit:.1f}..{max(s) * unit:.1f}")


h = cvlib.Handle(64, 64)
cus = torch.cuda.get_device_properties(0).multi_processor_count
lines = []

# ---- the record ----
for B in (256, 2048):
    g = torch.Generator(device=dev); g.manual_seed(B)
    mu, lv = torch.randn(B, 32, device=dev, generator=g), torch.randn(B, 32, device=dev, generator=g) - 1
    pred = torch.rand(B, 1, device=dev, generator=g)
    state, scratch, kl = h.latent_stats_state(dev), h.latent_stats_scratch(B, dev), torch.empty(B, 32, device=dev)
    rec = torch.zeros(696, dtype=torch.float64, device=dev)
    iu = torch.triu_indices(33, 33, device=dev)

    def torch_route():
        a = torch.cat((mu, pred), 1).double()
        l = lv.double()
        e = l.exp()
        rec[2:35] += a.sum(0)
        rec[35:596] += (a.T @ a)[iu[0], iu[1]]
        rec[596:628] += (0.5 * (a[:, :32] ** 2 + e - l - 1)).sum(0)
        rec[628:660] += e.sum(0)
        rec[660:692] += l.sum(0)
        rec[0:2] += B

    p = cvlib.latent_stats_plan(B, cus)
    variants = [("cvae_latent_stats", lambda: h.latent_stats(B, mu, lv, pred, state, scratch)),
                ("cvae_latent_stats with kl_rows", lambda: h.latent_stats(B, mu, lv, pred, state, scratch, kl)),
                ("torch route: fp64 a.T @ a, elementwise sums (no finite-row filter)", torch_route)]
    lines.append(f"B = {B}: {p['chunks']} chunks of {p['rows']} rows on {p['grid']} workgroups; us per call, 7 samples of 20 calls each, then the median")
    report(lines, variants, interleaved([f for _, f in variants]))

# ---- the response reduction ----
n, K = 64, 34
base, var, out = torch.rand(n, 3, 64, 64, device=dev), torch.rand(n, K, 3, 64, 64, device=dev), torch.empty(n, K, 2, device=dev)
w = torch.tensor([0.2989, 0.5870, 0.1140], device=dev).view(1, 1, 3, 1, 1)


def torch_response():
    d = var - base[:, None]
    out[..., 0] = (d * d).double().mean(dim=(2, 3, 4)).float()
    out[..., 1] = (d.abs() * w).sum(2).flatten(2).max(2).values


variants = [("cvae_recon_response", lambda: h.recon_response(n, K, base, var, out)), ("torch expression (fp64 mean, grey max)", torch_response)]
lines.append(f"cvae_recon_response: {n} frames x {K} variants at 64 x 64 ({var.numel() * 4 / 2 ** 20:.0f} MiB streamed); us per call, 7 samples of 20 calls each, then the median")
report(lines, variants, interleaved([f for _, f in variants]))

# ---- the loop ----
NF, B = 50000, 256
vae = VariationalAutoencoder(max_batch=B, seed=0).to(dev).eval()
frames = torch.randint(0, 256, (NF, 64, 64, 3), dtype=torch.uint8, device=dev)
ds = E.DeviceDataset(frames, torch.rand(NF, 1, device=dev), torch.stack([torch.zeros(NF, dtype=torch.int64), torch.arange(NF)], 1).numpy())
tr = FusedTrainer(vae)
variants = [("FusedTrainer.evaluate", lambda: tr.evaluate(ds, B)), ("FusedTrainer.latent_report", lambda: tr.latent_report(ds, B))]
lines.append(f"the loops over {NF} frames at B = {B}, fp32: ms per pass (wall, synchronised, the host read included), 7 alternating samples, then the median")
report(lines, variants, interleaved([f for _, f in variants], measure=wall, warm=1), unit=1.0, name="ms")

print("\n".join(lines))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
