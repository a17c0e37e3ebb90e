"""Latent audit: what the posterior of a trained Critic-VAE looks like, from ONE pooled device record (cvae_latent_stats,
include/cvae.h).

Two questions the training knobs (--kld-weight, --kld-warmup, ...) exist for and the loss scalars cannot answer:
  * did the posterior collapse?  -> the KL per latent dimension and the active units of Burda et al. (Var_x(mu_j) > 0.01);
  * does mu carry the critic value that the decoder is handed next to it (zcat = cat(z, pred))?  -> the least-squares fit
    of pred on (1, mu): its R^2, weights and the squared correlation per dimension.
Everything here is host arithmetic in float64 on the 692 sums of the record; the device work is the eval-mode encoder and one
cvae_latent_stats launch per batch (dataset_report, FusedTrainer.latent_report, VariationalAutoencoder.latent_stats).

record_host is the numpy statement of the record (the tests' reference), summarize turns a record into a dict, report_lines
prints it.  decoder_response asks the other half of the second question — does the decoder USE the injected value, and which
latent dimensions does it listen to — by decoding 34 variants of every frame's code (cvae_recon_response reduces them).
Out of scope: non-linear probes and mutual-information estimates, statistics of sampled z, and any claim about what the
numbers show on real recordings.

CLI: python -m critic_vae_amd.latent --networks DIR --critic CKPT --episodes DIR [--second] [--precision f32|bf16]
     [--batch B] [--au-threshold T] [--out FILE.npz] [--response [--delta D] [--response-frames N]]
"""
import argparse

import numpy as np

LATENT = 32
NA = LATENT + 1                       # a = (mu_0..mu_31, pred)
STATE_DOUBLES = 696                   # CVAE_LATENT_STATE_DOUBLES
RECORD = 692                          # the record without the library's scratch slots
SEEN, USED, SUM, GRAM, KL, EXP, LV = 0, 1, 2, 35, 596, 628, 660


def gram_index(i, j):
    """Slot of sum a_i a_j, i <= j, in the record (row-major upper triangle)."""
    return GRAM + i * NA - i * (i - 1) // 2 + (j - i)


_IU = np.triu_indices(NA)


def record_host(mu, logvar, pred):
    """The record cvae_latent_stats leaves after ONE call on an empty record, in numpy float64: RECORD doubles.
    mu, logvar (B,32), pred (B) or (B,1), any float dtype (float32 inputs are widened, as on the device)."""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1, LATENT)
    lv = np.asarray(logvar, dtype=np.float64).reshape(-1, LATENT)
    p = np.asarray(pred, dtype=np.float64).reshape(-1)
    assert mu.shape == lv.shape and p.shape[0] == mu.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        ev = np.exp(lv)
        use = np.isfinite(mu).all(1) & np.isfinite(lv).all(1) & np.isfinite(ev).all(1) & np.isfinite(p)
    mu, lv, ev, p = mu[use], lv[use], ev[use], p[use]
    a = np.concatenate([mu, p[:, None]], axis=1)
    rec = np.zeros(RECORD)
    rec[SEEN], rec[USED] = use.shape[0], mu.shape[0]
    rec[SUM:SUM + NA] = a.sum(0)
    rec[GRAM:KL] = (a.T @ a)[_IU]
    rec[KL:EXP] = (0.5 * (mu * mu + ev - lv - 1.0)).sum(0)
    rec[EXP:LV] = ev.sum(0)
    rec[LV:RECORD] = lv.sum(0)
    return rec


def kl_rows_host(mu, logvar):
    """kl_j of every row in float64 (what cvae_latent_stats writes to kl_rows, before its rounding to fp32)."""
    mu = np.asarray(mu, dtype=np.float64)
    lv = np.asarray(logvar, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return 0.5 * (mu * mu + np.exp(lv) - lv - 1.0)


def summarize(record, au_threshold=0.01, collapsed_below=0.01):
    """A record (>= RECORD doubles) as a dict of host values.  n = rows used.
      record (its first RECORD doubles), rows, used; kl_per_dim (32, nats, mean over the used rows), kl_total;
      mu_mean, mu_var: mean and POPULATION variance over images of mu_j; mean_posterior_var = mean exp(logvar_j); mean_logvar;
      aggregate_var = mu_var + mean_posterior_var: ~1 where the aggregate posterior matches the prior;
      active = mu_var > au_threshold (Burda et al.), n_active; collapsed = kl_per_dim < collapsed_below;
      pred_mean, pred_var;
      the leakage probe, the least-squares fit of pred on (1, mu) from the centred second moments (np.linalg.lstsq: the
      minimum-norm solution, so collapsed dimensions get weight 0 instead of breaking it): probe_weights (32), probe_bias,
      probe_r2 (NaN when pred does not vary), corr2_per_dim (squared correlation of mu_j with pred; 0 for a constant mu_j).
    An empty record gives NaNs."""
    rec = np.asarray(record, dtype=np.float64).reshape(-1)
    assert rec.shape[0] >= RECORD, f"a latent record has at least {RECORD} doubles"
    n = rec[USED]
    out = {"record": rec[:RECORD].copy(), "rows": int(rec[SEEN]), "used": int(n), "au_threshold": float(au_threshold), "collapsed_below": float(collapsed_below)}
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = 1.0 / n if n > 0 else np.nan
        S = rec[SUM:SUM + NA]
        G = np.zeros((NA, NA))
        G[_IU] = rec[GRAM:KL]
        G = G + np.triu(G, 1).T
        mean = S * inv
        C = (G - np.outer(S, S) * inv) * inv              # centred second moments: the population covariance of a
        var = np.maximum(np.diag(C), 0.0)
        kl = rec[KL:EXP] * inv
        pv = rec[EXP:LV] * inv
        out.update(kl_per_dim=kl, kl_total=float(kl.sum()), mu_mean=mean[:LATENT], mu_var=var[:LATENT], mean_posterior_var=pv,
                   mean_logvar=rec[LV:RECORD] * inv, aggregate_var=var[:LATENT] + pv,
                   pred_mean=float(mean[LATENT]), pred_var=float(var[LATENT]))
        out["active"] = out["mu_var"] > au_threshold
        out["n_active"] = int(out["active"].sum())
        out["collapsed"] = kl < collapsed_below
        Cmm, Cmp, Cpp = C[:LATENT, :LATENT], C[:LATENT, LATENT], C[LATENT, LATENT]
        if n > 0 and np.isfinite(C).all():
            w = np.linalg.lstsq(Cmm, Cmp, rcond=None)[0]
        else:
            w = np.full(LATENT, np.nan)
        out["probe_weights"] = w
        out["probe_bias"] = float(mean[LATENT] - w @ mean[:LATENT])
        out["probe_r2"] = float((w @ Cmp) / Cpp) if Cpp > 0 else float("nan")
        den = var[:LATENT] * Cpp
        out["corr2_per_dim"] = np.where(den > 0, Cmp * Cmp / np.where(den > 0, den, 1.0), 0.0 if Cpp > 0 else np.nan)
    return out


def dataset_report(vae, dataset, batch_size, theta=None, bn_state=None, au_threshold=0.01, collapsed_below=0.01):
    """The audit of `vae` on a DeviceDataset / ReconDataset: per batch one gather launch, the EVAL-mode cvae_forward with
    recon == NULL (the encoder alone: BatchNorm on its running statistics, eps = 0) and one cvae_latent_stats launch into ONE
    pooled device record; then one host read and summarize().  theta / bn_state: other weights of the same layout (a trainer's
    averaged ones), default the model's.  Needs no trainer, draws no random number and changes nothing but the workspace."""
    import torch
    from . import params as P
    h, n, dev, B = vae.handle, len(dataset), vae.theta.device, int(batch_size)
    if dataset.width != vae.width:
        raise ValueError(f"the dataset holds {dataset.width}x{dataset.width} frames, the VAE takes {vae.width}x{vae.width}")
    if not 1 <= B <= vae.max_batch:
        raise ValueError(f"batch_size {batch_size} outside 1..max_batch ({vae.max_batch}) of the handle")
    if dataset.frames.device != dev:
        raise ValueError(f"the dataset is on {dataset.frames.device}, the VAE on {dev}")
    if n < 1:
        raise ValueError("latent report: the dataset is empty")
    theta = vae.theta.data if theta is None else theta
    bn_state = vae.bn_state if bn_state is None else bn_state
    x = torch.empty(B, P.ch, vae.width, vae.width, device=dev)
    pred = torch.empty(B, 1, device=dev)
    mu = torch.empty(B, LATENT, device=dev)
    logvar = torch.empty_like(mu)
    zero = torch.zeros_like(mu)
    state, scratch = h.latent_stats_state(dev), h.latent_stats_scratch(B, dev)
    d_idx = torch.arange(n, dtype=torch.int64, device=dev)
    ws = vae._workspace(B)
    vae._stamp_workspace()
    for b in range(0, n, B):
        nb = min(B, n - b)
        dataset.gather(h, nb, d_idx[b:b + nb], x[:nb], pred[:nb])
        h.forward(nb, x[:nb], pred[:nb], zero[:nb], theta, bn_state, mu, logvar, None, ws, train=False)
        h.latent_stats(nb, mu, logvar, pred[:nb], state, scratch)
    return summarize(state.cpu().numpy(), au_threshold=au_threshold, collapsed_below=collapsed_below)      # the one host read


RESPONSE_VARIANTS = LATENT + 2        # dimension j moved by delta (0..31), pred -> 0 (32), pred -> 1 (33)


def decoder_response(vae, x, pred, delta=1.0, chunk=None):
    """What the decoder listens to, per frame: decode the frame's zcat = (mu, pred) and RESPONSE_VARIANTS = 34 variants of it —
    variants 0..31: dimension j moved by +delta (1.0 = one prior sigma); 32: pred -> 0, the contrast of the difference mask
    (diff_images); 33: pred -> 1 — and reduce every variant against the base reconstruction with cvae_recon_response.
    x (N,3,w,w), pred (N) or (N,1).  Returns the (N, 34, 2) device tensor: [..,0] the mean squared difference, [..,1] the largest
    grey difference (variant 32: diff_images' max_values, bit for bit).  The eval-mode encoder (BatchNorm on its running
    statistics; bn_state untouched) and cvae_decode run in pieces of `chunk` frames, at most max_batch // 34 (the default)."""
    import torch
    from . import params as P
    K, h = RESPONSE_VARIANTS, vae.handle
    x = vae._prep(x)
    N, dev, w = x.shape[0], x.device, vae.width
    pred = pred.to(torch.float32).reshape(N, 1).contiguous()
    per = vae.max_batch // K
    if per < 1:
        raise ValueError(f"decoder_response decodes {K} variants per frame: max_batch {vae.max_batch} < {K}")
    chunk = per if chunk is None else max(1, min(int(chunk), per))
    out = torch.empty(N, K, 2, device=dev)
    mu = torch.empty(chunk, LATENT, device=dev)
    logvar = torch.empty_like(mu)
    zero = torch.zeros_like(mu)
    base = torch.empty(chunk, P.ch, w, w, device=dev)
    var = torch.empty(chunk * K, P.ch, w, w, device=dev)
    step = torch.eye(LATENT, device=dev) * float(delta)
    with torch.no_grad():
        for s in range(0, N, chunk):
            n = min(chunk, N - s)
            h.forward(n, x[s:s + n], pred[s:s + n], zero[:n], vae.theta, vae.bn_state, mu[:n], logvar[:n], None, vae._workspace(n),
                      train=False)
            zc = torch.cat((mu[:n], pred[s:s + n]), dim=1).contiguous()
            h.decode(n, zc, vae.theta, base[:n], vae._workspace(n))
            zv = zc[:, None, :].repeat(1, K, 1)
            zv[:, :LATENT, :LATENT] += step
            zv[:, LATENT, LATENT] = 0.0
            zv[:, LATENT + 1, LATENT] = 1.0
            h.decode(n * K, zv.reshape(n * K, NA).contiguous(), vae.theta, var[:n * K], vae._workspace(n * K))
            h.recon_response(n, K, base[:n], var[:n * K], out[s:s + n])
        vae._stamp_workspace()
    return out


def summarize_response(response):
    """A (N, 34, 2) response (device tensor or array) as host values: latent_response (32) = the mean over frames of the mean
    squared change of the reconstruction when dimension j moves by delta, latent_grey_max (32) = likewise of the largest grey
    change; pred_response / pred_grey_max = the same for pred -> 0, pred_one_response for pred -> 1;
    pred_to_latent_ratio = pred_response / median(latent_response).  Read it this way: a collapsed dimension must show ~0
    response, and a decoder that ignores the critic value shows pred_response ~ 0."""
    r = response.detach().cpu().numpy() if hasattr(response, "detach") else np.asarray(response)
    r = r.astype(np.float64).reshape(-1, RESPONSE_VARIANTS, 2)
    m = r.mean(0)
    med = float(np.median(m[:LATENT, 0]))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.float64(m[LATENT, 0]) / np.float64(med))
    return {"frames": int(r.shape[0]), "latent_response": m[:LATENT, 0], "latent_grey_max": m[:LATENT, 1],
            "pred_response": float(m[LATENT, 0]), "pred_grey_max": float(m[LATENT, 1]),
            "pred_one_response": float(m[LATENT + 1, 0]), "pred_to_latent_ratio": ratio}


def report_lines(summary, response=None):
    """The table of a summary, one line per latent dimension, for printing; response: a summarize_response dict, whose
    columns are appended."""
    if response is not None:
        lines = report_lines(summary)
        lines[3] += "  response(mse)  grey max"
        for j in range(LATENT):
            lines[4 + j] += f" {response['latent_response'][j]:14.3e} {response['latent_grey_max'][j]:9.5f}"
        lines.insert(3, f"decoder response over {response['frames']} frames: pred -> 0 mse {response['pred_response']:.3e} (grey max "
                        f"{response['pred_grey_max']:.5f}), pred -> 1 mse {response['pred_one_response']:.3e}; pred / median latent "
                        f"{response['pred_to_latent_ratio']:.3f}")
        return lines
    s = summary
    lines = [f"latent audit over {s['used']} rows ({s['rows'] - s['used']} of {s['rows']} left out as non-finite)",
             f"KL total {s['kl_total']:.4f} nats; active units {s['n_active']}/{LATENT} (Var_x(mu) > {s['au_threshold']:g}); "
             f"collapsed {int(np.sum(s['collapsed']))}/{LATENT} (KL < {s['collapsed_below']:g})",
             f"critic value: mean {s['pred_mean']:.4f} var {s['pred_var']:.6f}; linear probe pred ~ (1, mu): "
             f"R^2 {s['probe_r2']:.4f}, bias {s['probe_bias']:.4f}",
             "dim       KL   Var_x(mu)  E[var_q]   agg var  active  corr^2(mu,pred)  probe w"]
    for j in range(LATENT):
        lines.append(f"{j:3d} {s['kl_per_dim'][j]:8.4f} {s['mu_var'][j]:10.5f} {s['mean_posterior_var'][j]:9.5f} "
                     f"{s['aggregate_var'][j]:9.5f}  {'yes' if s['active'][j] else ' no':>6} {s['corr2_per_dim'][j]:16.5f} "
                     f"{s['probe_weights'][j]:8.4f}")
    return lines


def save_npz(path, summary):
    """The record and every entry of the summary as one .npz."""
    np.savez(path, **{k: np.asarray(v) for k, v in summary.items()})
    return path


def build_parser():
    ap = argparse.ArgumentParser(prog="critic_vae_amd.latent", description="Latent audit of a saved Critic-VAE on curated episode frames: "
                                 "per-dimension KL, active units and the linear probe of the critic value on mu")
    ap.add_argument("--networks", required=True, help="directory with the saved encoder / decoder files")
    ap.add_argument("--critic", required=True, help="critic checkpoint, or 'synth'")
    ap.add_argument("--episodes", required=True, nargs="+", help="episode files / directories, as -train --episodes")
    ap.add_argument("--second", action="store_true", help="audit the second VAE (vae2_encoder.pt, vae2_decoder.pt)")
    ap.add_argument("--precision", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--au-threshold", type=float, default=0.01, help="active unit: Var_x(mu_j) above this (Burda et al.: 0.01)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, metavar="FILE.npz", help="write the record and the summary")
    ap.add_argument("--response", action="store_true", help="also the decoder response (decoder_response): 34 decoded variants per frame")
    ap.add_argument("--delta", type=float, default=1.0, help="--response: how far a dimension is moved (1.0 = one prior sigma)")
    ap.add_argument("--response-frames", type=int, default=256, metavar="N", help="--response: on the first N curated frames")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    from .episodes import curate, load_episodes
    from .nets import VariationalAutoencoder
    from .train import _device, _load_critic, load_networks
    episodes = load_episodes(args.episodes)
    device = _device()
    vae = VariationalAutoencoder(max_batch=args.batch, seed=args.seed, precision=args.precision).to(device)
    load_networks(vae, args.networks, second=args.second)
    critic = _load_critic(args.critic, vae.handle, args.seed, device)
    ds = curate(episodes, critic, device=device)
    if len(ds) == 0:
        raise SystemExit("the curated dataset is empty: no frame of the trajectories falls in a critic-value bin")
    summary = dataset_report(vae, ds, args.batch, au_threshold=args.au_threshold)
    response = None
    if args.response:
        if args.batch < RESPONSE_VARIANTS:
            raise SystemExit(f"--response decodes {RESPONSE_VARIANTS} variants per frame: --batch must be at least that")
        n = max(1, min(args.response_frames, len(ds)))
        x = torch.empty(n, 3, vae.width, vae.width, device=device)
        pred = torch.empty(n, 1, device=device)
        ds.gather(vae.handle, n, torch.arange(n, dtype=torch.int64, device=device), x, pred)
        response = summarize_response(decoder_response(vae, x, pred, delta=args.delta))
        summary.update({f"response_{k}": v for k, v in response.items()})
    torch.cuda.synchronize()
    print("\n".join(report_lines(summary, response)))
    if args.out:
        print(f"saved {save_npz(args.out, summary)}")
    return summary


if __name__ == "__main__":
    main()
