"""Torch-CPU restatement of one training step of the reference's Critic (critic_net.py:5-59, train mode) with explicit
Dropout keep masks, in fp32 or fp64: the yardstick of cvae_critic_grad (tests/test_gpu_critic_train.py) and, pinned to
the reference's own class by tests/golden/make_critic_train_golden.py, of tests/test_host_critic_train.py.

ReLU followed by MaxPool2d(2) is written as "select one element of each 2x2 window, zero it unless it is > 0": the
same function and the same gradient (torch's max-pool takes the first maximum in scan order; a window whose maximum is
<= 0 yields 0 and passes no gradient through the ReLU).  That form can take the selection from outside: with
`decisions` given (the layout of cvae_critic_grad's decisions, include/cvae.h) the pool gathers on the given index
and the two dense ReLUs use the given mask, so two runs in different precisions follow the same piecewise-linear
branch and differ by round-off only.
"""
import numpy as np
import torch
import torch.nn.functional as F

KEYS = (("features.0.weight", (8, 3, 3, 3)), ("features.0.bias", (8,)),
        ("features.3.weight", (8, 8, 3, 3)), ("features.3.bias", (8,)),
        ("features.6.weight", (8, 8, 3, 3)), ("features.6.bias", (8,)),
        ("features.10.weight", (16, 8, 3, 3)), ("features.10.bias", (16,)),
        ("features.14.weight", (32, 16, 4, 4)), ("features.14.bias", (32,)),
        ("crit.1.weight", (32, 32)), ("crit.1.bias", (32,)),
        ("crit.4.weight", (1, 32)), ("crit.4.bias", (1,)))
N_PARAMS = 11873
KEEP = 800
KEEP_SITES = ((0, (8, 8, 8)), (512, (16, 4, 4)), (768, (32,)))          # features.9, features.13, crit.3
POOL_SHAPES = ((8, 32, 32), (8, 16, 16), (8, 8, 8), (16, 4, 4))
DEC_OFFSETS = (0, 8192, 10240, 10752, 11008, 11040)
DECISIONS = 11072
LAYERS = ("features.0", "features.3", "features.6", "features.10", "features.14", "crit.1", "crit.4")


def flatten(params):
    """dict of arrays / tensors -> (11873,) float64 numpy in state_dict order."""
    return np.concatenate([np.asarray(torch.as_tensor(params[k]).detach().cpu().numpy(), dtype=np.float64).reshape(-1) for k, _ in KEYS])


def unflatten(flat, dtype=np.float32):
    out, off = {}, 0
    flat = np.asarray(flat)
    for k, shape in KEYS:
        n = int(np.prod(shape))
        out[k] = flat[off:off + n].reshape(shape).astype(dtype)
        off += n
    return out


def dropout_scale(p):
    """The one fp32 scale of kept elements (include/cvae.h)."""
    return float(np.float32(1.0 / (1.0 - float(p))))


def _windows(y):
    B, C, S, _ = y.shape
    return y.reshape(B, C, S // 2, 2, S // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, S // 2, S // 2, 4)


def _relu_pool(y, dec):
    """-> (pooled, decision): decision 0..3 = 2*dy+dx of the selected element, 4 = window maximum <= 0."""
    win = _windows(y)
    if dec is None:
        with torch.no_grad():
            best, idx = win[..., 0].clone(), torch.zeros(win.shape[:-1], dtype=torch.int64)
            for k in (1, 2, 3):                                   # first maximum in scan order: strict >
                better = win[..., k] > best
                best = torch.where(better, win[..., k], best)
                idx = torch.where(better, torch.full_like(idx, k), idx)
            dec = torch.where(best > 0, idx, torch.full_like(idx, 4))
    else:
        dec = dec.to(torch.int64)
    sel = win.gather(-1, dec.clamp(max=3).unsqueeze(-1)).squeeze(-1)
    return sel * (dec != 4).to(y.dtype), dec


def split_decisions(decisions):
    """(B, 11072) uint8 -> [4 pool decision tensors (B,C,S,S), features.14 mask (B,32), crit.1 mask (B,32)]."""
    d = torch.as_tensor(np.asarray(decisions)).to(torch.int64)
    B = d.shape[0]
    out = [d[:, DEC_OFFSETS[i]:DEC_OFFSETS[i + 1]].reshape(B, *POOL_SHAPES[i]) for i in range(4)]
    out.append(d[:, DEC_OFFSETS[4]:DEC_OFFSETS[5]])
    out.append(d[:, DEC_OFFSETS[5]:DECISIONS])
    return out


def forward(p, x, keep, dropout_p, decisions=None):
    """p: dict of tensors (the run's dtype); x (B,3,64,64); keep (B,800) or None -> (pred (B,1), pre-activations, decisions)."""
    dt, B = x.dtype, x.shape[0]
    imposed = split_decisions(decisions) if decisions is not None else [None] * 6
    scale = torch.tensor(dropout_scale(dropout_p), dtype=dt)
    if keep is None:
        ks = torch.ones(B, KEEP, dtype=dt) * scale
    else:
        ks = (torch.as_tensor(np.asarray(keep)) != 0).to(dt) * scale
    site = [ks[:, o:o + int(np.prod(s))].reshape(B, *s) for o, s in KEEP_SITES]
    pre, dec = [], []
    a = x
    for i, name in enumerate(("features.0", "features.3", "features.6", "features.10")):
        y = F.conv2d(a, p[name + ".weight"], p[name + ".bias"], padding=1)
        a, d = _relu_pool(y, imposed[i])
        pre.append(y); dec.append(d.reshape(B, -1))
        if i == 2:
            a = a * site[0]
        if i == 3:
            a = a * site[1]
    y = F.conv2d(a, p["features.14.weight"], p["features.14.bias"]).reshape(B, 32)
    m = (y > 0) if imposed[4] is None else (imposed[4] != 0)
    pre.append(y); dec.append(m.to(torch.int64))
    a = y * m.to(dt)
    y = F.linear(a, p["crit.1.weight"], p["crit.1.bias"])
    m = (y > 0) if imposed[5] is None else (imposed[5] != 0)
    pre.append(y); dec.append(m.to(torch.int64))
    a = y * m.to(dt) * site[2]
    z = F.linear(a, p["crit.4.weight"], p["crit.4.bias"])
    pre.append(z)
    return torch.sigmoid(z), pre, torch.cat(dec, dim=1).to(torch.uint8)


def losses(pred, target):
    t = target.reshape(-1).to(pred.dtype)
    return F.binary_cross_entropy(pred[:, 0], t), F.mse_loss(pred[:, 0], t)


def step(params, x, target, keep, dropout_p, loss="bce", dtype=torch.float32, decisions=None):
    """One forward + loss + backward.  params: dict of arrays; x (B,3,64,64) fp32 in [0,1]; target (B).
    -> dict(pre = per-layer pre-activations (numpy, LAYERS order), decisions (B,11072) uint8 — the run's own free
    choices, or the imposed ones —, pred (B,1), loss, bce, mse, grads = {key: numpy}, flat_grads (11873,))."""
    p = {k: torch.as_tensor(np.asarray(params[k])).to(dtype).clone().requires_grad_(True) for k, _ in KEYS}
    xt = torch.as_tensor(np.asarray(x)).to(dtype)
    tt = torch.as_tensor(np.asarray(target)).to(dtype)
    pred, pre, dec = forward(p, xt, keep, dropout_p, decisions)
    bce, mse = losses(pred, tt)
    chosen = {"bce": bce, "mse": mse}[loss]
    chosen.backward()
    grads = {k: p[k].grad.detach().numpy() for k, _ in KEYS}
    return dict(pre=[y.detach().numpy() for y in pre], decisions=dec.numpy(), pred=pred.detach().numpy(),
                loss=chosen.item(), bce=bce.item(), mse=mse.item(), grads=grads,
                flat_grads=np.concatenate([grads[k].reshape(-1) for k, _ in KEYS]))


def eval_forward(params, x, dtype=torch.float32):
    """Eval-mode prediction (Dropout = identity) -> (B,1) numpy."""
    p = {k: torch.as_tensor(np.asarray(params[k])).to(dtype) for k, _ in KEYS}
    with torch.no_grad():
        return forward(p, torch.as_tensor(np.asarray(x)).to(dtype), None, 0.0)[0].numpy()


def adam_trajectory(params, x, target, keeps, dropout_p, loss="bce", lr=1e-4, dtype=torch.float64):
    """len(keeps) steps of torch.optim.Adam (defaults, vae.py:36) on the same batch, one keep mask per step.
    -> (losses (steps,) float64, final flat parameters (11873,) float64)."""
    p = {k: torch.as_tensor(np.asarray(params[k])).to(dtype).clone().requires_grad_(True) for k, _ in KEYS}
    opt = torch.optim.Adam(list(p.values()), lr=lr)
    xt = torch.as_tensor(np.asarray(x)).to(dtype)
    tt = torch.as_tensor(np.asarray(target)).to(dtype)
    curve = []
    for keep in keeps:
        opt.zero_grad()
        pred, _, _ = forward(p, xt, keep, dropout_p)
        chosen = dict(zip(("bce", "mse"), losses(pred, tt)))[loss]
        chosen.backward()
        opt.step()
        curve.append(chosen.item())
    return np.asarray(curve, dtype=np.float64), flatten(p)


def frames_to_x(u8):
    """uint8 (B,64,64,3) -> fp32 (B,3,64,64) / 255, as cvae_preprocess_u8."""
    return (np.asarray(u8).astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2).copy()
