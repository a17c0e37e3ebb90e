"""What tests/test_gpu_critic_train.py and its child process share: the fixture, one cvae_critic_grad call with
device buffers, and the parity method (decisions imposed on the restatement, ties judged by the reference's own round-off)."""
import os

import numpy as np
import torch

import critic_train_ref as ref
from critic_vae_amd import lib as cvlib

DEV = "cuda:0"
PRED_TOL, GRAD_TOL = 1e-5, 1e-4           # absolute on pred / loss scalars; of each gradient tensor's max |value|


def make_handle(max_batch=64):
    return cvlib.Handle(64, max_batch)


def load_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "critic_train_real.npz"))
    ck = np.load(os.path.join(golden_dir, "critic_real_b8.npz"))
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"][:37]
    w = {k: ck["w/" + k] for k, _ in ref.KEYS}
    return dict(z=z, w=w, flat=ref.flatten(w).astype(np.float32), u8=u8, x=ref.frames_to_x(u8))


PROBE = 0xA5


def run_kernel(h, flat, x, target, keep, dropout_p, loss, decisions=True):
    """One call on fresh buffers -> numpy dict(grads (11876,), pred (B,1), scalars (4,), decisions (B,11072) or None,
    partials_written = how many of the B partial slots of scratch (11 876 floats each, filled with PROBE bytes before the
    call) the call wrote: the number of workgroups of the persistent grid)."""
    B = x.shape[0]
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)      # noqa: E731
    grads = torch.empty(cvlib.CRITIC_TRAIN_FLOATS, device=DEV)
    pred = torch.empty(B, 1, device=DEV)
    scal = torch.empty(4, device=DEV)
    dec = torch.empty(B, cvlib.CRITIC_DECISIONS, dtype=torch.uint8, device=DEV) if decisions else None
    scratch = torch.full((h.critic_grad_scratch_bytes(B),), PROBE, dtype=torch.uint8, device=DEV)
    h.critic_grad(B, d(x, torch.float32), d(target, torch.float32), None if keep is None else d(keep, torch.uint8), dropout_p,
                  cvlib.CRITIC_LOSS[loss], d(flat, torch.float32), grads, pred, scal, scratch, decisions=dec)
    torch.cuda.synchronize()
    slots = scratch[:min(B, 256) * cvlib.CRITIC_TRAIN_FLOATS * 4].reshape(min(B, 256), -1)[:, :ref.N_PARAMS * 4]
    touched = (slots != PROBE).any(dim=1).cpu().numpy()
    untouched_whole = (slots == PROBE).all(dim=1).cpu().numpy()
    assert (touched | untouched_whole).all() and touched[:int(touched.sum())].all(), "the written partial slots are not a prefix"
    return dict(grads=grads.cpu().numpy(), pred=pred.cpu().numpy(), scalars=scal.cpu().numpy(),
                decisions=None if dec is None else dec.cpu().numpy(), partials_written=int(touched.sum()))


def split_flat(flat):
    out, off = {}, 0
    for k, shape in ref.KEYS:
        n = int(np.prod(shape))
        out[k] = np.asarray(flat[off:off + n]).reshape(shape)
        off += n
    return out


def compare(res, want_pred, want_scalars, want_grads, loss, what):
    """pred and the loss scalars within PRED_TOL, every gradient tensor within GRAD_TOL of its max |value|.
    want_scalars = (bce, mse); want_grads a flat (11873,) array.  Returns the worst (pred, scalar, relative gradient) gaps."""
    assert np.isfinite(res["grads"]).all() and np.isfinite(res["pred"]).all() and np.isfinite(res["scalars"]).all(), what
    e_pred = float(np.abs(res["pred"].astype(np.float64) - want_pred).max())
    chosen = want_scalars[0] if loss == "bce" else want_scalars[1]
    e_scal = max(abs(float(res["scalars"][0]) - chosen), abs(float(res["scalars"][1]) - want_scalars[0]),
                 abs(float(res["scalars"][2]) - want_scalars[1]))
    got, want = split_flat(res["grads"][:ref.N_PARAMS]), split_flat(want_grads)
    worst, worst_key = 0.0, None
    for k, _ in ref.KEYS:
        scale = float(np.abs(want[k]).max())
        gap = float(np.abs(got[k].astype(np.float64) - want[k]).max())
        rel = gap / scale if scale > 0 else (0.0 if gap == 0 else np.inf)
        if rel > worst:
            worst, worst_key = rel, k
    print(f"{what}: |d pred| {e_pred:.2e}  |d loss| {e_scal:.2e}  worst gradient gap {worst:.2e} of max ({worst_key})")
    assert e_pred <= PRED_TOL, f"{what}: pred off by {e_pred:.3e}"
    assert e_scal <= PRED_TOL and res["scalars"][3] == 0, f"{what}: loss scalars off by {e_scal:.3e}"
    assert worst <= GRAD_TOL, f"{what}: gradient {worst_key} off by {worst:.3e} of its max"
    assert (res["grads"][ref.N_PARAMS:] == 0).all(), f"{what}: padding floats not zero"
    return e_pred, e_scal, worst


def _choice_gap(win, dec):
    """Per window: how far the choice `dec` is from being right in the pre-activations `win` (..., 4) — 0 where it is."""
    ymax = win.max(-1)
    k = np.minimum(dec, 3)
    yk = np.take_along_axis(win, k[..., None], -1)[..., 0]
    closed = dec == 4
    # closed: claims max <= 0, wrong by max(ymax, 0).  open at k: claims y_k is the maximum and > 0
    return np.where(closed, np.maximum(ymax, 0.0), np.maximum(ymax - yk, np.maximum(-yk, 0.0)))


def imposed_parity(res, w, x, target, keep, dropout_p, loss, what):
    """The method of the parity test: restatement in fp64 and fp32 with the kernel's decisions imposed; E_l = max |y32 - y64|
    per layer (the reference's own fp32 round-off); a decision that differs from the fp64 restatement's free choice must be a
    tie within 4 E_l (two implementations, each off by E_l, times 2 for the summation order), at most 2 + 1e-4 * count per
    layer; then pred / loss / gradients against the imposed fp64 run.  Returns (flips, worst gaps)."""
    dec = res["decisions"]
    r64 = ref.step(w, x, target, keep, dropout_p, loss, torch.float64, decisions=dec)
    r32 = ref.step(w, x, target, keep, dropout_p, loss, torch.float32, decisions=dec)
    free = ref.step(w, x, target, keep, dropout_p, loss, torch.float64)
    E = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32["pre"], r64["pre"])]
    flips = []
    B = x.shape[0]
    for l in range(6):
        lo, hi = ref.DEC_OFFSETS[l], (ref.DEC_OFFSETS[l + 1] if l < 5 else ref.DECISIONS)
        mine, theirs = dec[:, lo:hi].astype(np.int64), free["decisions"][:, lo:hi].astype(np.int64)
        diff = mine != theirs
        n = int(diff.sum())
        flips.append(n)
        if n == 0:
            continue
        y = free["pre"][l]
        if l < 4:
            C, S = ref.POOL_SHAPES[l][0], ref.POOL_SHAPES[l][1] * 2
            win = y.reshape(B, C, S // 2, 2, S // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, -1, 4)
            gap = _choice_gap(win, mine)
        else:
            gap = np.abs(y.reshape(B, -1))
        worst = float(gap[diff].max())
        assert worst <= 4 * E[l], f"{what}: layer {ref.LAYERS[l]}: a decision differs from the fp64 restatement by {worst:.3e} > 4 E_l = {4 * E[l]:.3e}"
        assert n <= 2 + 1e-4 * diff.size, f"{what}: layer {ref.LAYERS[l]}: {n} tie flips in {diff.size} decisions"
    gaps = compare(res, r64["pred"], (r64["bce"], r64["mse"]), r64["flat_grads"], loss, what)
    rel_E = [e / max(float(np.abs(p).max()), 1e-30) for e, p in zip(E, r64["pre"])]
    print(f"{what}: flips per layer {flips}; E_l / max|y| {['%.1e' % e for e in rel_E]}")
    return flips, gaps
