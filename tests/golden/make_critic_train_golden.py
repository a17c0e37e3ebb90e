"""Generate tests/golden/critic_train_real.npz: one training step of the REFERENCE's Critic class in train mode, and
a 40-step Adam curve (run only where the reference checkout exists, on the CPU).

    python tests/golden/make_critic_train_golden.py            # needs /root/reference (read-only)

The reference's Critic (critic_net.py:5-69) runs in train mode with torch.nn.functional.dropout replaced by a function
that takes its mask from the fixture's `keep` (row layout of include/cvae.h: features.9, features.13, crit.3) and
multiplies kept elements by the one fp32 scale (float)(1 / (1 - p)).  tests/critic_train_ref.py (the restatement the
GPU tests compare against) is asserted equal to it in fp32 within 1e-6 on pred, both losses and every gradient, for
both losses at B = 5 and B = 37: the reference is the authority, the restatement is what travels.

Inputs by reference, not stored again: the frames are the first 37 (and first 5) of step_real_b68.npz["u8"], the
weights are critic_real_b8.npz["w/*"].  Stored:
  dropout_p, lr                       0.3, 1e-4
  target (37,), keep (37,800) uint8   B = 5 uses the first five rows
  decisions (37,11072) uint8          the reference run's pool / ReLU choices (restatement, fp32; equal for both losses)
  b{5,37}/{bce,mse}/pred|scalars|grads   the REFERENCE class's fp32 results: pred (B,1), scalars (bce, mse), flat grads (11873,)
  traj/keep_bits (40, 3700) uint8     np.packbits of the (37,800) keep mask of each step
  traj/loss64 (40,), traj/params64    the fp64 restatement's BCE curve (loss before each update) and final parameters
  traj/gap32                          worst |loss32 - loss64| of the fp32 restatement over the same 40 steps
"""
import os
import sys
from unittest import mock

import numpy as np
import torch

sys.dont_write_bytecode = True
os.environ.setdefault("MKL_CBWR", "COMPATIBLE")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import critic_train_ref as ref          # noqa: E402

P, LR, STEPS, SEED = 0.3, 1e-4, 40, 20261018


def reference_step(weights, x, target, keep, loss):
    """The reference class itself, train mode, Dropout masks from `keep` in call order."""
    from critic_net import Critic
    net = Critic(dropout=P)
    net.load_state_dict({k: torch.from_numpy(weights[k]) for k, _ in ref.KEYS})
    net.train()
    sites = [torch.from_numpy(keep[:, o:o + int(np.prod(s))].reshape(len(keep), *s) != 0) for o, s in ref.KEEP_SITES]
    calls = []

    def fake_dropout(inp, p=0.5, training=True, inplace=False):
        assert training and p == P
        m = sites[len(calls)]
        calls.append(tuple(inp.shape))
        return inp * (m.to(inp.dtype) * torch.tensor(ref.dropout_scale(p), dtype=inp.dtype))

    with mock.patch("torch.nn.functional.dropout", fake_dropout):
        pred = net(torch.from_numpy(x))
    assert len(calls) == 3, calls
    t = torch.from_numpy(target)
    bce = torch.nn.functional.binary_cross_entropy(pred[:, 0], t)
    mse = torch.nn.functional.mse_loss(pred[:, 0], t)
    {"bce": bce, "mse": mse}[loss].backward()
    sd = dict(net.named_parameters())
    grads = np.concatenate([sd[k].grad.numpy().reshape(-1) for k, _ in ref.KEYS])
    return pred.detach().numpy(), np.array([float(bce.detach()), float(mse.detach())], dtype=np.float32), grads


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    real = np.load(os.path.join(HERE, "step_real_b68.npz"))
    ck = np.load(os.path.join(HERE, "critic_real_b8.npz"))
    weights = {k: ck["w/" + k] for k, _ in ref.KEYS}
    x37 = ref.frames_to_x(real["u8"][:37])
    rng = np.random.default_rng(SEED)
    target = rng.random(37).astype(np.float32)
    target[[0, 7]] = 0.0                     # the ends of the range are legal targets
    target[[3, 20]] = 1.0
    keep = (rng.random((37, ref.KEEP)) >= P).astype(np.uint8)
    out = dict(dropout_p=np.float64(P), lr=np.float64(LR), target=target, keep=keep)
    for B in (5, 37):
        for loss in ("bce", "mse"):
            pred, scalars, grads = reference_step(weights, x37[:B], target[:B], keep[:B], loss)
            r = ref.step(weights, x37[:B], target[:B], keep[:B], P, loss)
            worst = max(np.abs(pred - r["pred"]).max(), abs(scalars[0] - r["bce"]), abs(scalars[1] - r["mse"]),
                        np.abs(grads - r["flat_grads"]).max())
            print(f"B={B} {loss}: reference vs restatement (fp32) max diff {worst:.3e}; loss {r['loss']:.6f}")
            assert worst <= 1e-6, worst
            out[f"b{B}/{loss}/pred"], out[f"b{B}/{loss}/scalars"], out[f"b{B}/{loss}/grads"] = pred, scalars, grads
            if B == 37:
                out.setdefault("decisions", r["decisions"])
                assert np.array_equal(out["decisions"], r["decisions"])
    keeps = (rng.random((STEPS, 37, ref.KEEP)) >= P).astype(np.uint8)
    loss64, params64 = ref.adam_trajectory(weights, x37, target, keeps, P, "bce", LR, torch.float64)
    loss32, _ = ref.adam_trajectory(weights, x37, target, keeps, P, "bce", LR, torch.float32)
    gap = float(np.abs(loss32 - loss64).max())
    print(f"trajectory: loss {loss64[0]:.6f} -> {loss64[-1]:.6f}; fp32 restatement's worst gap to fp64 {gap:.3e}")
    out["traj/keep_bits"] = np.packbits(keeps.reshape(STEPS, -1), axis=1)
    out["traj/loss64"], out["traj/params64"], out["traj/gap32"] = loss64, params64, np.float64(gap)
    path = os.path.join(HERE, "critic_train_real.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
