"""Training the critic on the device: the reference ships only a trained `critic-*.pt` and points its users at "another
value network" (vae.py:50); CriticTrainer trains the reference's Critic class (critic_net.py:5-69, default arguments) from
frames and targets, with cvae_critic_grad (forward in train mode with explicit Dropout masks, loss, every gradient:
csrc/critic_train.hip) and the flat Adam kernels the VAE trainer uses.  The optimizer launches (plain or guarded), the
guard's counters, the validation fields and the loop of fit_device are DeviceTrainer's (fit.py), shared with FusedTrainer.

    critic = Critic(handle=Handle(64, 128)).to("cuda:0"); critic.load_state_dict(initial_state_dict(seed=0))
    ds = episodes.critic_dataset(load_episodes(["episodes/"]), load_rewards(["rewards/"]))      # frames + discounted targets
    CriticTrainer(critic).fit_device(ds, batch_size=128, epochs=15)
    torch.save(critic.state_dict(), "critic.pt")              # the reference's checkpoint format

critic.flat holds the trained values after every step: critic.evaluate, critic.state_dict(), curate(), segment and render
use the critic as they use a loaded checkpoint.

Held-out validation (cvae_critic_score, csrc/critic_score.hip: uint8 frame -> eval-mode forward -> one row per frame and a
pooled fp64 record, one launch per batch):

    train, val = episodes.split_by_trajectory(ds, 0.2)
    trainer.fit_device(train, 128, epochs=15, val=val)          # trainer.val_history: (step, evaluate(val)) per epoch
    trainer.evaluate(val, 2048)["bin_agreement"]                # the share of frames whose value lands in its target's bin
"""
import numpy as np
import torch

from . import params as P
from . import synth
from .fit import DeviceTrainer
from .optim import critic_layout, decay_ranges
from .lib import CRITIC_DECISIONS, CRITIC_KEEP, CRITIC_LOSS, CRITIC_SCORE_COLS, CRITIC_SCORE_STATE_DOUBLES, CRITIC_TRAIN_FLOATS

MAX_BATCH = 65536            # cvae_critic_grad's and cvae_critic_score's own cap (include/cvae.h)
RECORD_DOUBLES = 27          # the documented part of cvae_critic_score's pooled record: counts, sums, maximum, confusion


def initial_state_dict(seed=0):
    """Fresh critic weights: the reference class's shapes with PyTorch's default init bounds (synth.make_critic_params)."""
    return {k: torch.from_numpy(v) for k, v in synth.make_critic_params(seed).items()}


def score_frames(critic, frames_u8, targets, idx=None):
    """cvae_critic_score's rows, (B, 8) fp32 on the device, of frames_u8[idx] ((N,64,64,3) uint8 device tensor) against
    targets[idx] ((N) or (N,1) fp32): [0] the critic's value p, [1] the target t, [2] the BCE term, [3] (p - t)^2, [4] |p - t|,
    [5] / [6] the bin of p / of t (0 mid, 1 high, 2 low, 3 none: episodes.value_bins), [7] 0.  idx: int64 device tensor, or None =
    every frame in order; an index outside [0, N) gives a NaN row.  Batches above MAX_BATCH run in pieces."""
    h, dev = critic.handle, frames_u8.device
    B = frames_u8.shape[0] if idx is None else idx.numel()
    rows = torch.empty(B, CRITIC_SCORE_COLS, device=dev)
    for b in range(0, B, MAX_BATCH):
        nb = min(MAX_BATCH, B - b)
        if idx is None:
            h.critic_score(nb, frames_u8[b:b + nb], targets[b:b + nb], critic.flat, per_frame=rows[b:b + nb])
        else:
            h.critic_score(nb, frames_u8, targets, critic.flat, idx=idx[b:b + nb], per_frame=rows[b:b + nb])
    return rows


def summarize_record(rec, loss="bce"):
    """The pooled record of cvae_critic_score (include/cvae.h; at least its first 27 doubles, on the host) -> the dict
    CriticTrainer.evaluate returns, in float64:
      frames, finite_frames: frames seen, and those whose row is finite (a NaN target or value is counted, not hidden);
      bce, mse, mae, mean_pred, mean_target: means over the finite frames; loss: bce or mse, as `loss` names it;
      pearson: Pearson's r of value and target over the finite frames, NaN when either variance is 0 (a variance below 1e-12
        of the mean square is cancellation noise of the fp64 sums and counts as 0);
      bin_agreement: the share of finite frames whose value falls in the bin of its target (the trace of `confusion` over the
        finite frames); confusion: (4, 4) int64, row = the target's bin, column = the value's (mid, high, low, none);
      worst: the largest |p - t|.  An empty record gives NaN everywhere and a zero confusion matrix."""
    if loss not in CRITIC_LOSS:
        raise ValueError(f"loss {loss!r}: one of {sorted(CRITIC_LOSS)}")
    rec = np.asarray(rec, np.float64).reshape(-1)
    if rec.size < RECORD_DOUBLES:
        raise ValueError(f"a record of {rec.size} doubles, need at least {RECORD_DOUBLES}")
    nan = float("nan")
    fin = int(rec[1])
    conf = np.rint(rec[11:27]).astype(np.int64).reshape(4, 4)
    out = {"frames": int(rec[0]), "finite_frames": fin, "confusion": conf}
    if fin == 0:
        out.update(bce=nan, mse=nan, mae=nan, loss=nan, pearson=nan, bin_agreement=nan, mean_pred=nan, mean_target=nan, worst=nan)
        return out
    s_bce, s_se, s_ae, s_p, s_t, s_pp, s_tt, s_pt = (float(v) for v in rec[2:10])
    out.update(bce=s_bce / fin, mse=s_se / fin, mae=s_ae / fin, mean_pred=s_p / fin, mean_target=s_t / fin, worst=float(rec[10]))
    out["loss"] = out[loss]
    var_p, var_t, cov = s_pp - s_p * s_p / fin, s_tt - s_t * s_t / fin, s_pt - s_p * s_t / fin
    if var_p <= 1e-12 * s_pp or var_t <= 1e-12 * s_tt:
        out["pearson"] = nan
    else:
        out["pearson"] = float(cov / np.sqrt(var_p * var_t))
    out["bin_agreement"] = float(np.trace(conf)) / fin
    return out


class CriticTrainer(DeviceTrainer):
    """One step = cvae_critic_grad + cvae_adam_step (or the guarded pair) on the critic's flat parameter block.

    Owns the padded parameters (the critic's 11 873 floats + 3 zeros, so the Adam kernels' n % 4 == 0 holds), the gradient,
    the Adam moments and the scratch; `critic.flat` is re-pointed at the first 11 873 floats of the padded block, so the
    critic always holds the trained values.  Anything that re-allocates that buffer afterwards (critic.to(...), .float(),
    load_state_dict is fine: it copies in place) would cut the critic off from the trainer; step() checks the address and
    raises instead of training a block nobody reads.  dropout: the p of the three Dropout layers (the reference class's default is
    0.5; its shipped checkpoint does not say what it was trained with).  loss: "bce" (torch's binary_cross_entropy on the
    sigmoid output) or "mse".  skip_nonfinite / max_grad_norm: the guarded step of FusedTrainer (train.py).  augment: an
    augment.Augment or None — fit_device then builds every batch with cvae_preprocess_u8_gather_aug under
    augment.at(step_count) (still one launch per batch); the TARGET of a frame stays the stored one.  evaluate() and step()
    never augment; the augmentation is saved and restored with the trainer.  optim: an optim.Optim or None — as for
    FusedTrainer: LR schedule with `lr` as the peak, decoupled weight decay on the seven *.weight tensors (their boundaries fall
    anywhere in the flat block: the kernel's ranges are in elements), an EMA of the block in `ema` (no auxiliary buffer: the
    critic has no BatchNorm), all inside the one Adam launch; evaluate(..., ema=True) scores the averaged block.  trace: a
    trace.Trace or None — as for FusedTrainer, with the critic's 4 loss scalars and its 14 tensors."""

    def __init__(self, critic, lr=1e-4, betas=P.adam_betas, eps=P.adam_eps, dropout=0.3, loss="bce", skip_nonfinite=False,
                 max_grad_norm=None, augment=None, optim=None, trace=None):
        if loss not in CRITIC_LOSS:
            raise ValueError(f"loss {loss!r}: one of {sorted(CRITIC_LOSS)}")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"dropout {dropout!r} outside [0, 1)")
        self._init_shared(skip_nonfinite, max_grad_norm, optim, trace)      # guard fields, step_count, val_history / best_val / val_stale, optim, trace
        self.decay_ranges = decay_ranges(critic_layout())     # the seven *.weight tensors, at their element offsets
        self.critic, self.h = critic, critic.handle
        self._init_augment(augment, 64)
        self.lr, self.betas, self.eps = float(lr), tuple(betas), float(eps)
        if self.optim is not None:
            self.optim.check_lr(self.lr)
        self.dropout, self.loss = float(dropout), loss
        dev = critic.flat.device
        if dev.type != "cuda":
            raise ValueError("CriticTrainer needs the critic on the device (critic.to('cuda:0')): there is no CPU path")
        n = critic.flat.numel()
        assert self.h.lib.cvae_critic_train_floats() == CRITIC_TRAIN_FLOATS and n <= CRITIC_TRAIN_FLOATS
        self.theta = torch.zeros(CRITIC_TRAIN_FLOATS, device=dev)
        self.theta[:n].copy_(critic.flat)
        critic.flat = self.theta[:n]               # the registered buffer becomes a view of the padded block
        self.grads = torch.zeros_like(self.theta)
        self.m = torch.zeros_like(self.theta)
        self.v = torch.zeros_like(self.theta)
        self.scalars = torch.zeros(4, device=dev)
        self._scratch, self._pred = None, None

    def _buffers(self, B):
        need = self.h.critic_grad_scratch_bytes(B)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.theta.device)
        if self._pred is None or self._pred.numel() < B:
            self._pred = torch.empty(B, 1, device=self.theta.device)
        return self._scratch, self._pred[:B]

    def _trace_layout(self):
        return critic_layout()

    def draw_keep(self, B, generator=None):
        """(B, 800) uint8 keep mask on the device: torch.rand >= dropout."""
        return (torch.rand((B, CRITIC_KEEP), device=self.theta.device, generator=generator) >= self.dropout).to(torch.uint8)

    def step(self, x, target, keep=None, generator=None, decisions=None):
        """x (B,3,64,64) fp32 in [0,1], target (B) or (B,1) fp32 in [0,1], keep (B,800) uint8 or None (drawn from `generator`
        on the device): contiguous device tensors.  Returns the 4 loss scalars (chosen, BCE, MSE, 0) of the parameters BEFORE
        the update, on the device — no host sync; the tensor is overwritten by the next step.  The predictions of the step are
        in self.pred."""
        B = x.shape[0]
        if self.critic.flat.data_ptr() != self.theta.data_ptr():
            raise RuntimeError("critic.flat no longer is the trainer's parameter block (the critic was moved or converted after "
                               "CriticTrainer(critic)): construct the trainer after critic.to(device)")
        if keep is None:
            keep = self.draw_keep(B, generator)
        scratch, pred = self._buffers(B)
        self.h.critic_grad(B, x, target, keep, self.dropout, CRITIC_LOSS[self.loss], self.theta, self.grads, pred,
                           self.scalars, scratch, decisions=decisions)
        self.pred = pred
        self.step_count += 1
        self._update(self.theta, 1.0)
        return self.scalars

    def _check_dataset(self, dataset, batch_size, cap):
        dev = self.theta.device
        if dataset.width != 64:
            raise ValueError(f"the dataset holds {dataset.width}x{dataset.width} frames, the critic takes 64x64")
        if dataset.frames.dtype != torch.uint8:
            raise ValueError("the critic's dataset holds uint8 frames (episodes.critic_dataset)")
        if not 1 <= int(batch_size) <= cap:
            raise ValueError(f"batch_size {batch_size} outside 1..{cap}")
        if dataset.frames.device != dev:
            raise ValueError(f"the dataset is on {dataset.frames.device}, the critic on {dev}")
        return dev, int(batch_size)

    def evaluate(self, dataset, batch_size, per_frame=False, ema=False):
        """The critic on a held-out DeviceDataset whose `preds` slot holds the targets (episodes.critic_dataset,
        split_by_trajectory): the dataset in order, one cvae_critic_score launch per batch — uint8 frame, EVAL-mode forward
        (Dropout = identity), row, pooling — into ONE fp64 device record that the host reads once, at the end.  Returns
        summarize_record's dict (loss = this trainer's chosen loss), plus per_frame = the (N, 8) device rows when asked for.
        batch_size: 1..65 536, whatever the handle's max_batch.  Draws nothing from any random generator and leaves the
        parameters, the Adam state, the step count and the guard record untouched.  ema=True: the averaged block instead of theta."""
        dev, B = self._check_dataset(dataset, batch_size, MAX_BATCH)
        theta = self.theta
        if ema:
            if not self.has_ema():
                raise ValueError("evaluate(ema=True): this trainer keeps no averaged weights (optim=Optim(ema=...))")
            theta = self._ema_view(self.theta)[0]
        h, n = self.h, len(dataset)
        if n < 1:
            raise ValueError("evaluate(): the dataset is empty")
        rows = torch.empty(n, CRITIC_SCORE_COLS, device=dev) if per_frame else None
        scratch = None if per_frame else torch.empty(h.critic_score_scratch_bytes(min(B, n)), dtype=torch.uint8, device=dev)
        state = h.critic_score_state(dev)
        targets = dataset.preds.view(-1)
        for b in range(0, n, B):
            nb = min(B, n - b)
            h.critic_score(nb, dataset.frames[b:b + nb], targets[b:b + nb], theta, state=state, scratch=scratch,
                           per_frame=None if rows is None else rows[b:b + nb])
        out = summarize_record(state[:RECORD_DOUBLES].cpu().numpy(), self.loss)        # the one host read
        if per_frame:
            out["per_frame"] = rows
        return out

    def fit_device(self, dataset, batch_size, epochs=1, generator=None, shuffle=True, val=None, val_every=None, on_val=None):
        """The loop of FusedTrainer.fit_device over a DeviceDataset whose `preds` slot holds the targets
        (episodes.critic_dataset): per epoch np.random.shuffle of the host indices, slices of batch_size with the ragged last
        batch kept, one cvae_preprocess_u8_gather launch per batch (x = frames[idx] / 255, target = preds[idx]), keep masks from
        `generator`.  With an augmentation (the constructor's `augment`) that launch is cvae_preprocess_u8_gather_aug.
        Returns the loss scalars of every step taken, (steps, 4), on the device.
        val, val_every, on_val: held-out validation as in FusedTrainer.fit_device (the shared loop, fit.py), with this
        trainer's evaluate(val, batch_size); a fit that on_val ended returns the rows of the steps it took."""
        dev, B = self._check_dataset(dataset, batch_size, min(self.h.max_batch, MAX_BATCH))
        n = len(dataset)
        if val is not None:
            self._check_dataset(val, B, MAX_BATCH)
        x = torch.empty(B, 3, 64, 64, device=dev)
        target = torch.empty(B, 1, device=dev)
        log = torch.zeros(epochs * ((n + B - 1) // B), 4, device=dev)
        first = self.step_count

        def batch(xb, targetb):                            # the keep mask is drawn inside step()
            row = log[self.step_count - first]
            row.copy_(self.step(xb, targetb, generator=generator))

        self._fit(dataset, B, epochs, shuffle, x, target, batch, val, val_every, on_val, B)
        return log[:self.step_count - first]

    def state_dict(self):
        """Parameters (the 11 873 floats, flat), Adam moments, step count and the guard's counters, as CPU copies; the
        validation history (confusion matrices as nested lists), best_val and val_stale."""
        n = self.critic.flat.numel()
        return {"flat": self.theta[:n].detach().cpu().clone(), "m": self.m.detach().cpu().clone(), "v": self.v.detach().cpu().clone(),
                **self._shared_state()}

    def load_state_dict(self, state):
        n = self.critic.flat.numel()
        if state["flat"].numel() != n or state["m"].numel() != self.m.numel() or state["v"].numel() != self.v.numel():
            raise ValueError("trainer state of another parameter count")
        self._load_shared_state(state)
        self.theta[:n].copy_(state["flat"])
        self.m.copy_(state["m"])
        self.v.copy_(state["v"])


__all__ = ["CriticTrainer", "initial_state_dict", "score_frames", "summarize_record", "CRITIC_SCORE_COLS", "CRITIC_SCORE_STATE_DOUBLES", "CRITIC_KEEP", "CRITIC_DECISIONS", "CRITIC_TRAIN_FLOATS", "MAX_BATCH"]
