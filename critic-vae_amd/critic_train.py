"""Training the critic on the device: the reference ships only a trained `critic-*.pt` and points its users at "another
value network" (vae.py:50); CriticTrainer trains the reference's Critic class (critic_net.py:5-69, default arguments) from
frames and targets, with cvae_critic_grad (forward in train mode with explicit Dropout masks, loss, every gradient:
csrc/critic_train.hip) and the flat Adam kernels the VAE trainer uses.

    critic = Critic(handle=Handle(64, 128)).to("cuda:0"); critic.load_state_dict(initial_state_dict(seed=0))
    ds = episodes.critic_dataset(load_episodes(["episodes/"]), load_rewards(["rewards/"]))      # frames + discounted targets
    CriticTrainer(critic).fit_device(ds, batch_size=128, epochs=15)
    torch.save(critic.state_dict(), "critic.pt")              # the reference's checkpoint format

critic.flat holds the trained values after every step: critic.evaluate, critic.state_dict(), curate(), segment and render
use the critic as they use a loaded checkpoint.
"""
import numpy as np
import torch

from . import params as P
from . import synth
from .lib import CRITIC_DECISIONS, CRITIC_KEEP, CRITIC_LOSS, CRITIC_TRAIN_FLOATS

MAX_BATCH = 65536            # cvae_critic_grad's own cap (include/cvae.h)


def initial_state_dict(seed=0):
    """Fresh critic weights: the reference class's shapes with PyTorch's default init bounds (synth.make_critic_params)."""
    return {k: torch.from_numpy(v) for k, v in synth.make_critic_params(seed).items()}


class CriticTrainer:
    """One step = cvae_critic_grad + cvae_adam_step (or the guarded pair) on the critic's flat parameter block.

    Owns the padded parameters (the critic's 11 873 floats + 3 zeros, so the Adam kernels' n % 4 == 0 holds), the gradient,
    the Adam moments and the scratch; `critic.flat` is re-pointed at the first 11 873 floats of the padded block, so the
    critic always holds the trained values.  Anything that re-allocates that buffer afterwards (critic.to(...), .float(),
    load_state_dict is fine: it copies in place) would cut the critic off from the trainer; step() checks the address and
    raises instead of training a block nobody reads.  dropout: the p of the three Dropout layers (the reference class's default is
    0.5; its shipped checkpoint does not say what it was trained with).  loss: "bce" (torch's binary_cross_entropy on the
    sigmoid output) or "mse".  skip_nonfinite / max_grad_norm: the guarded step of FusedTrainer (train.py)."""

    def __init__(self, critic, lr=1e-4, betas=P.adam_betas, eps=P.adam_eps, dropout=0.3, loss="bce", skip_nonfinite=False,
                 max_grad_norm=None):
        if loss not in CRITIC_LOSS:
            raise ValueError(f"loss {loss!r}: one of {sorted(CRITIC_LOSS)}")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"dropout {dropout!r} outside [0, 1)")
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f"max_grad_norm {max_grad_norm!r}: a positive number (inf = no clipping) or None")
        self.critic, self.h = critic, critic.handle
        self.lr, self.betas, self.eps = float(lr), tuple(betas), float(eps)
        self.dropout, self.loss = float(dropout), loss
        self.skip_nonfinite = bool(skip_nonfinite)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.guarded = self.skip_nonfinite or self.max_grad_norm is not None
        self.guard, self._guard_counts = None, (0, 0)
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
        self.step_count = 0
        self._scratch, self._pred = None, None

    def _buffers(self, B):
        need = self.h.critic_grad_scratch_bytes(B)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.theta.device)
        if self._pred is None or self._pred.numel() < B:
            self._pred = torch.empty(B, 1, device=self.theta.device)
        return self._scratch, self._pred[:B]

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
        if self.guarded:
            if self.guard is None:
                self.guard = self.h.guard_state(self.theta.device, *self._guard_counts)
            self.h.grad_stats(self.grads, self.guard, 1.0, float("inf") if self.max_grad_norm is None else self.max_grad_norm,
                              self.skip_nonfinite, self.lr, self.betas[0], self.betas[1])
            self.h.adam_step_guarded(self.theta, self.grads, self.m, self.v, self.guard, self.eps)
        else:
            self.h.adam_step(self.theta, self.grads, self.m, self.v, self.step_count, self.lr, self.betas[0], self.betas[1],
                             self.eps)
        return self.scalars

    def fit_device(self, dataset, batch_size, epochs=1, generator=None, shuffle=True):
        """The loop of FusedTrainer.fit_device over a DeviceDataset whose `preds` slot holds the targets
        (episodes.critic_dataset): per epoch np.random.shuffle of the host indices, slices of batch_size with the ragged last
        batch kept, one cvae_preprocess_u8_gather launch per batch (x = frames[idx] / 255, target = preds[idx]), keep masks from
        `generator`.  Returns the loss scalars of every step, (steps, 4), on the device."""
        dev = self.theta.device
        n, B = len(dataset), int(batch_size)
        if dataset.width != 64:
            raise ValueError(f"the dataset holds {dataset.width}x{dataset.width} frames, the critic takes 64x64")
        if not 1 <= B <= min(self.h.max_batch, MAX_BATCH):
            raise ValueError(f"batch_size {batch_size} outside 1..max_batch ({self.h.max_batch}) of the critic's handle")
        if dataset.frames.device != dev:
            raise ValueError(f"the dataset is on {dataset.frames.device}, the critic on {dev}")
        x = torch.empty(B, 3, 64, 64, device=dev)
        target = torch.empty(B, 1, device=dev)
        log = torch.zeros(epochs * ((n + B - 1) // B), 4, device=dev)
        k = 0
        for _ in range(epochs):
            idx = np.arange(n)
            if shuffle:
                np.random.shuffle(idx)
            d_idx = torch.from_numpy(idx).to(dev)
            for b in range(0, n, B):
                nb = min(B, n - b)
                dataset.gather(self.h, nb, d_idx[b:b + nb], x[:nb], target[:nb])
                log[k].copy_(self.step(x[:nb], target[:nb], generator=generator))
                k += 1
        return log

    # ---- the guard's counters, as FusedTrainer ----
    def guard_stats(self):
        """dict(applied, skipped, norm, coef) of a guarded trainer (one device -> host copy)."""
        if not self.guarded:
            raise RuntimeError("guard_stats(): this trainer has no guard (skip_nonfinite / max_grad_norm)")
        if self.guard is None:
            return dict(applied=self._guard_counts[0], skipped=self._guard_counts[1], norm=0.0, coef=1.0)
        rec = self.h.guard_record(self.guard)
        return dict(applied=int(rec.t), skipped=int(rec.skipped), norm=float(rec.norm64), coef=float(rec.coef))

    def state_dict(self):
        """Parameters (the 11 873 floats, flat), Adam moments, step count and the guard's counters, as CPU copies."""
        if self.guarded:
            st = self.guard_stats()
            applied, skipped = st["applied"], st["skipped"]
        else:
            applied, skipped = self.step_count, 0
        n = self.critic.flat.numel()
        return {"flat": self.theta[:n].detach().cpu().clone(), "m": self.m.detach().cpu().clone(), "v": self.v.detach().cpu().clone(),
                "step_count": int(self.step_count), "applied": applied, "skipped": skipped}

    def load_state_dict(self, state):
        n = self.critic.flat.numel()
        if state["flat"].numel() != n or state["m"].numel() != self.m.numel() or state["v"].numel() != self.v.numel():
            raise ValueError("trainer state of another parameter count")
        applied, skipped, steps = int(state["applied"]), int(state["skipped"]), int(state["step_count"])
        if not self.guarded and applied != steps:
            raise ValueError(f"the state skipped {skipped} of {steps} steps: an unguarded trainer corrects Adam's bias by step_count "
                             "and cannot continue it; construct the trainer with skip_nonfinite=True")
        self.theta[:n].copy_(state["flat"])
        self.m.copy_(state["m"])
        self.v.copy_(state["v"])
        self.step_count = steps
        self._guard_counts = (applied, skipped)
        if self.guarded and self.guard is not None:
            self.h.guard_init(self.guard, applied, skipped)


__all__ = ["CriticTrainer", "initial_state_dict", "CRITIC_KEEP", "CRITIC_DECISIONS", "CRITIC_TRAIN_FLOATS", "MAX_BATCH"]
