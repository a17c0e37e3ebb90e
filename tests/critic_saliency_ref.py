"""Torch-CPU restatement, in fp32 or fp64, of what cvae_critic_collect, cvae_critic_saliency and cvae_critic_occlusion
compute (include/cvae.h): the embeddings of Critic.forward(X, collect=True) (critic_net.py:44-59), the gradient of the
logit (the pre-sigmoid output of crit.4) with respect to the pixels, integrated gradients from the black frame with the
kernel's scaling and order, and occlusion sensitivity.  Built on tests/critic_train_ref.py's forward, whose pool / ReLU
choices can be imposed from outside, so that a run in another precision follows the device's piecewise-linear branch.
Pinned to the reference's own class by tests/golden/make_critic_saliency_golden.py."""
import numpy as np
import torch

import critic_train_ref as ref

GREY = (np.float32(0.2989), np.float32(0.5870), np.float32(0.1140))          # cvae_diff_grey's weights
EMBED_SHAPES = ((8, 32, 32), (8, 16, 16), (8, 8, 8), (16, 4, 4), (32, 1, 1))


def _params(w, dtype):
    return {k: torch.as_tensor(np.asarray(w[k])).to(dtype) for k, _ in ref.KEYS}


def embeddings(w, x, dtype=torch.float64, decisions=None):
    """-> (pred (B,1), [e1..e5]) numpy: the four pooled maps and features.14 after its ReLU (eval mode)."""
    p = _params(w, dtype)
    xt = torch.as_tensor(np.asarray(x)).to(dtype)
    B = xt.shape[0]
    with torch.no_grad():
        pred, pre, dec = ref.forward(p, xt, None, 0.0, decisions)
        d = ref.split_decisions(dec.numpy())
        out = []
        for i in range(4):
            pooled, _ = ref._relu_pool(pre[i], d[i])
            out.append(pooled.numpy())
        out.append((pre[4] * (d[4] != 0).to(dtype)).reshape(B, 32, 1, 1).numpy())
    return pred.numpy(), out


def logit_grad(w, x, dtype=torch.float64, decisions=None):
    """d z / d x with z the pre-sigmoid output of crit.4 -> dict(pred (B,1), logit (B,), grad (B,3,64,64), decisions (B,11072) —
    the run's own free choices, or the imposed ones)."""
    p = _params(w, dtype)
    xt = torch.as_tensor(np.asarray(x)).to(dtype).clone().requires_grad_()
    pred, pre, dec = ref.forward(p, xt, None, 0.0, decisions)
    pre[6].sum().backward()                       # frames are independent: the gradient of the sum is each frame's own
    return dict(pred=pred.detach().numpy(), logit=pre[6].detach().numpy().reshape(-1), grad=xt.grad.numpy(), decisions=dec.numpy())


def scaled_frames(x, k, n):
    """The frames of pass k of n: one fp32 product per pixel with the fp32 quotient (float)k / (float)n."""
    return np.asarray(x, np.float32) * (np.float32(k) / np.float32(n))


def integrated_gradients(w, x, steps, dtype=torch.float64, decisions=None):
    """The kernel's sum: passes k = 1..steps in that order on scaled_frames(x, k, steps), the gradients added in `dtype`,
    then (sum * x) * (1 / steps) with fp32(1 / steps).  decisions: None or a list of `steps` (B,11072) arrays, one per pass.
    -> dict(grad, pred, decisions (those of the last pass, x itself), pass_decisions)."""
    x = np.asarray(x, np.float32)
    acc, last, used = None, None, []
    for k in range(1, steps + 1):
        last = logit_grad(w, scaled_frames(x, k, steps), dtype, None if decisions is None else decisions[k - 1])
        used.append(last["decisions"])
        acc = last["grad"].copy() if acc is None else acc + last["grad"]
    npdt = np.float64 if dtype == torch.float64 else np.float32
    inv = (np.float32(1.0) / np.float32(steps)).astype(npdt)
    return dict(grad=(acc * x.astype(npdt)) * inv, pred=last["pred"], decisions=last["decisions"], pass_decisions=used)


def grey_map(grad):
    """(B,3,64,64) -> (B,64,64) float64: |g_r| * 0.2989f + |g_g| * 0.5870f + |g_b| * 0.1140f with the fp32 weights' values."""
    g = np.abs(np.asarray(grad, np.float64))
    return g[:, 0] * np.float64(GREY[0]) + g[:, 1] * np.float64(GREY[1]) + g[:, 2] * np.float64(GREY[2])


def occluded_frames(x, patch, fill):
    """x (3,64,64) fp32 -> ((64/patch)^2, 3, 64, 64) fp32: patch n (row-major) filled with the fp32 colour `fill`."""
    x = np.asarray(x, np.float32)
    g = 64 // patch
    out = np.repeat(x[None], g * g, axis=0)
    f = np.asarray(fill, np.float32).reshape(3, 1, 1)
    for n in range(g * g):
        py, px = divmod(n, g)
        out[n, :, py * patch:(py + 1) * patch, px * patch:(px + 1) * patch] = f
    return out


def occlusion(w, x, patch, fill, dtype=torch.float64):
    """-> dict(pred (B,), drop (B,g,g) = pred - occluded pred, map (B,64,64) = max(drop, 0) over its patch, max_values (B))."""
    x = np.asarray(x, np.float32)
    B, g = x.shape[0], 64 // patch
    pred = ref.eval_forward(w, x, dtype).reshape(-1)
    drop = np.empty((B, g, g), pred.dtype)
    for b in range(B):
        drop[b] = (pred[b] - ref.eval_forward(w, occluded_frames(x[b], patch, fill), dtype).reshape(-1)).reshape(g, g)
    m = np.maximum(drop, 0).repeat(patch, axis=1).repeat(patch, axis=2)
    return dict(pred=pred, drop=drop, map=m, max_values=m.reshape(B, -1).max(1))
