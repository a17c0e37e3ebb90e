"""What tests/test_gpu_critic_saliency.py and its child process share: the fixture, one call of each new entry on fresh
device buffers with guard bytes behind every output, and the tie test of a decision that differs from the fp64 restatement."""
import os

import numpy as np
import torch

import critic_saliency_ref as sref
import critic_train_ref as ref
import critic_train_tools as T
from critic_vae_amd import lib as cvlib

DEV = T.DEV
GUARD, GUARD_BYTES = 0x5A, 64
EMBED_NUMEL = tuple(int(np.prod(s)) for s in sref.EMBED_SHAPES)


def load_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "critic_saliency_real.npz"))
    ck = np.load(os.path.join(golden_dir, "critic_real_b8.npz"))
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"]
    w = {k: ck["w/" + k] for k, _ in ref.KEYS}
    return dict(z=z, w=w, flat=ref.flatten(w).astype(np.float32), u8=u8, x=ref.frames_to_x(u8))


def dev(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)


class Guarded:
    """A device buffer of `numel` elements, filled with GUARD bytes, with GUARD_BYTES more behind it."""

    def __init__(self, numel, dtype=torch.float32):
        self.nbytes = numel * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((self.nbytes + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=DEV)
        self.t = self.raw[:self.nbytes].view(dtype)

    def numpy(self, shape):
        assert bool((self.raw[self.nbytes:] == GUARD).all()), "written past the end of an output"
        return self.t.cpu().numpy().reshape(shape)


def run_collect(h, flat, x, which=(True,) * 5):
    """-> dict(pred (B,), e1..e5 (given ones), untouched = the guard buffers of the withheld ones were left alone)."""
    B = x.shape[0]
    pred = Guarded(B)
    bufs = [Guarded(B * n) for n in EMBED_NUMEL]
    h.critic_collect(B, dev(x), dev(flat), pred.t, [b.t if on else None for b, on in zip(bufs, which)])
    torch.cuda.synchronize()
    out = dict(pred=pred.numpy((B,)))
    for i, (b, on, shape) in enumerate(zip(bufs, which, sref.EMBED_SHAPES)):
        if on:
            out[f"e{i + 1}"] = b.numpy((B,) + shape)
        else:
            assert bool((b.raw == GUARD).all()), f"e{i + 1} was null, but a buffer of its size changed"
    return out


def run_saliency(h, flat, x, steps=1, grad=True, decisions=True):
    B = x.shape[0]
    pred, mp, mx = Guarded(B), Guarded(B * 4096), Guarded(B)
    g = Guarded(B * 3 * 4096) if grad else None
    d = Guarded(B * cvlib.CRITIC_DECISIONS, torch.uint8) if decisions else None
    h.critic_saliency(B, dev(x), dev(flat), steps, pred.t, mp.t, mx.t, grad=g.t if grad else None, decisions=d.t if decisions else None)
    torch.cuda.synchronize()
    return dict(pred=pred.numpy((B,)), map=mp.numpy((B, 64, 64)), max_values=mx.numpy((B,)),
                grad=g.numpy((B, 3, 64, 64)) if grad else None, decisions=d.numpy((B, cvlib.CRITIC_DECISIONS)) if decisions else None)


def run_occlusion(h, flat, x, patch, fill):
    B, g = x.shape[0], 64 // patch
    pred, drop, mp, mx = Guarded(B), Guarded(B * g * g), Guarded(B * 4096), Guarded(B)
    h.critic_occlusion(B, dev(x), dev(flat), patch, fill, pred.t, drop.t, mp.t, mx.t)
    torch.cuda.synchronize()
    return dict(pred=pred.numpy((B,)), drop=drop.numpy((B, g, g)), map=mp.numpy((B, 64, 64)), max_values=mx.numpy((B,)))


def run_forward(h, flat, x):
    """cvae_critic_forward in chunks of the handle's max_batch -> (B,)."""
    B = x.shape[0]
    xd, fd = dev(x), dev(flat)
    pred = torch.empty(B, device=DEV)
    for s in range(0, B, h.max_batch):
        n = min(h.max_batch, B - s)
        h.critic_forward(n, xd[s:s + n], fd, pred[s:s + n])
    torch.cuda.synchronize()
    return pred.cpu().numpy()


def check_ties(w, x, dec, free_dec, what, cap=11):
    """The tie test of critic_train_tools.imposed_parity for the eval-mode forward: a device decision that differs from the
    fp64 restatement's free choice must be a tie within 4 E_l, E_l = max |y32 - y64| of the layer with the device's decisions
    imposed (the restatement's own fp32 round-off); at most `cap` per frame.  Returns the number of differing decisions."""
    differ = dec != free_dec
    n = int(differ.sum())
    if n == 0:
        return 0
    B = x.shape[0]
    assert int(differ.reshape(B, -1).sum(1).max()) <= cap, f"{what}: {differ.reshape(B, -1).sum(1).max()} decisions of one frame differ"
    pre = {}
    for dt in (torch.float32, torch.float64):
        p = {k: torch.as_tensor(np.asarray(w[k])).to(dt) for k, _ in ref.KEYS}
        with torch.no_grad():
            pre[dt] = [y.numpy() for y in ref.forward(p, torch.as_tensor(x).to(dt), None, 0.0, dec)[1]]
            if dt == torch.float64:
                free = [y.numpy() for y in ref.forward(p, torch.as_tensor(x).to(dt), None, 0.0)[1]]
    E = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(pre[torch.float32], pre[torch.float64])]
    for l in range(6):
        lo, hi = ref.DEC_OFFSETS[l], (ref.DEC_OFFSETS[l + 1] if l < 5 else ref.DECISIONS)
        d = differ[:, lo:hi]
        if not d.any():
            continue
        y = free[l]
        if l < 4:
            C, S = ref.POOL_SHAPES[l][0], ref.POOL_SHAPES[l][1] * 2
            win = y.reshape(B, C, S // 2, 2, S // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, -1, 4)
            gap = T._choice_gap(win, dec[:, lo:hi].astype(np.int64))
        else:
            gap = np.abs(y.reshape(B, -1))
        worst = float(gap[d].max())
        assert worst <= 4 * E[l], f"{what}: layer {ref.LAYERS[l]}: a decision differs from the fp64 restatement by {worst:.3e} > 4 E_l = {4 * E[l]:.3e}"
    return n


def ulp32(v):
    """The spacing of float32 at |v| (float64 array in, float64 out)."""
    a = np.abs(np.asarray(v, np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)
