"""What a held-out evaluation costs: FusedTrainer.evaluate over 50 000 synthetic frames (HIP events around whole calls, median
of 7) at fp32 batch 256 and bf16 batch 2048, against, in the same process,
  - the nearest route without cvae_score: per batch gather + cvae_forward(train = 0) + cvae_loss with null gradients
    (batch scalars only, no per-image value, no pooled loss);
  - the only per-image route without it: cvae_loss at batch 1, once per frame, on a 2 048-frame subset;
  - one epoch of fit_device over the same frames, for the cost of an end-of-epoch evaluation as a fraction of an epoch.

    python profiles/experiments/eval_rate.py [OUT.txt]
"""
import os, sys, statistics
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from critic_vae_amd import params as P
from critic_vae_amd import synth
from critic_vae_amd.episodes import DeviceDataset
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer
dev = torch.device("cuda:0")
N, SUB, REPS = 50_000, 2_048, 7


def timed(f, reps=REPS):
    """ms per call of f: events around each whole call, after one warm-up -> (median, all)"""
    f()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), out


# Frames that train: the 68 real frames of tests/golden/step_real_b68.npz, repeated, with that fixture's weights (seed wseed, last decoder
# bias raised by last_bias_shift).  Noise frames against an untrained decoder give a NaN loss and NaN parameters after one step, and
# a NaN model need not time like a real one.
fx = np.load(os.path.join(ROOT, "tests", "golden", "step_real_b68.npz"))
gen = torch.Generator(device=dev); gen.manual_seed(1)
rep = -(-N // 68)
frames = torch.from_numpy(fx["u8"]).to(dev).repeat(rep, 1, 1, 1)[:N].contiguous()
preds = torch.from_numpy(fx["pred"]).to(dev).repeat(rep, 1)[:N].contiguous()
weights = synth.make_params(int(fx["wseed"]))
weights["decoder.model.12.bias"] = weights["decoder.model.12.bias"] + np.float32(fx["last_bias_shift"])
source = np.stack([np.arange(N) // 1000, np.arange(N) % 1000], 1)
ds = DeviceDataset(frames, preds, source)
lines = []
for prec, B in (("f32", 256), ("bf16", 2048)):
    vae = VariationalAutoencoder(max_batch=B, seed=int(fx["wseed"]), precision=prec).to(dev)
    vae.load_reference_params(weights)
    tr = FusedTrainer(vae)
    h, v = tr.h, tr.vae
    x = torch.empty(B, P.ch, P.w, P.w, device=dev); pred = torch.empty(B, 1, device=dev)
    zero = torch.zeros(B, P.latent_dim, device=dev); idx = torch.arange(N, device=dev)
    scal = torch.empty(16, device=dev)

    def batch_scalars():
        for b in range(0, N, B):
            nb = min(B, N - b)
            ds.gather(h, nb, idx[b:b + nb], x[:nb], pred[:nb])
            h.forward(nb, x[:nb], pred[:nb], zero[:nb], v.theta.data, v.bn_state, tr.mu, tr.logvar, tr.recon, tr.ws, train=False)
            h.loss(nb, x[:nb], tr.mu, tr.logvar, tr.recon, tr.ws, scal)

    def per_frame_loss():                       # the per-image route without cvae_score, given recon / mu / logvar of a batch
        for b in range(0, SUB, B):
            nb = min(B, SUB - b)
            ds.gather(h, nb, idx[b:b + nb], x[:nb], pred[:nb])
            h.forward(nb, x[:nb], pred[:nb], zero[:nb], v.theta.data, v.bn_state, tr.mu, tr.logvar, tr.recon, tr.ws, train=False)
            for i in range(nb):
                h.loss(1, x[i:i + 1], tr.mu[i:i + 1], tr.logvar[i:i + 1], tr.recon[i:i + 1], tr.ws, scal)

    def epoch():
        tr.fit_device(ds, B, 1, generator=gen)

    te, ae = timed(lambda: tr.evaluate(ds, B))
    tp, ap = timed(lambda: tr.evaluate(ds, B, per_image=True))
    tb, ab = timed(batch_scalars)
    tf, af = timed(per_frame_loss, reps=3)
    tt, at = timed(epoch, reps=3)
    f = lambda a: " ".join(f"{t:.1f}" for t in a)
    lines.append(f"{prec} B = {B}, {N} frames: evaluate {f(ae)} ms, median {te:.1f} ms = {N / te * 1e3:.0f} images/s; with per_image rows "
                 f"median {tp:.1f} ms = {N / tp * 1e3:.0f} images/s; gather + cvae_forward(train=0) + cvae_loss(no gradients), batch scalars "
                 f"only: {f(ab)} ms, median {tb:.1f} ms = {N / tb * 1e3:.0f} images/s; evaluate / that = {te / tb:.3f}")
    lines.append(f"{prec} B = {B}: cvae_loss at batch 1 per frame ({SUB} frames, forward at batch {B}): {f(af)} ms, median {tf:.1f} ms = "
                 f"{SUB / tf * 1e3:.0f} images/s; one epoch of fit_device over the {N} frames: {f(at)} ms, median {tt:.1f} ms = "
                 f"{N / tt * 1e3:.0f} images/s; one evaluation of as many frames = {te / tt:.3f} of an epoch; parameters finite after "
                 f"the epochs: {bool(torch.isfinite(v.theta.data).all())}")
text = "\n".join(lines)
print(text)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(text + "\n")
