"""The `-train` path of the reference (vae.py:33-66, 154-163) on synthetic data.

Two drivers over the same C-ABI kernels:

  * train(autoencoder, dset, critic_fn)  — the reference loop, line for line (torch.optim.Adam over
    autoencoder.parameters(), np.random.shuffle per epoch, short tail batch kept, log every log_n).
  * FusedTrainer                          — the same step without autograd/optimizer objects: direct
    cvae_forward -> cvae_loss -> cvae_backward -> (RCCL all-reduce of the flat gradient) ->
    cvae_adam_step, all asynchronous on one stream.  This is what bench.py times.  The optimizer launches (plain or
    guarded), the guard's counters, the validation fields and the loop of fit_device are DeviceTrainer's (fit.py), which
    CriticTrainer (critic_train.py) shares.

    python -m critic_vae_amd.train -train --synthetic 1024 --batch 32 --epochs 1
    python -m critic_vae_amd.train -train --episodes episodes/ --critic critic.pt --epochs 7 --save saved-networks

With --episodes the training set is built as the reference's load_minerl_data(critic) builds it (episodes.py), on the
device, and FusedTrainer.fit_device trains on it.

The second stage of the reference's experiment (vae.py:130-153):

    python -m critic_vae_amd.train -dataset --episodes episodes/ --critic critic.pt --networks saved-networks --out recon.npz
    python -m critic_vae_amd.train -second --dataset recon.npz --critic critic.pt --epochs 7 --save saved-networks
"""
import argparse
import os
import time

import numpy as np
import torch

from . import params as P
from . import synth
from .fit import DeviceTrainer
from .lib import N_SCALARS, SCORE_COLS, SYNC_DOUBLES, SYNC_POINTS
from .nets import VariationalAutoencoder
from .augment import Augment
from .objective import Objective, compose
from .optim import Optim, decay_ranges
from .trace import Trace, nonfinite_tensors


def _reference_batches(dset, epoch_indices, starts, batch_size, device, critic_fn):
    """vae.py:46-50 as the reference does it: gather, fp32 copy to the device, critic — all synchronous."""
    for b in starts:
        images = torch.from_numpy(dset[epoch_indices[b:b + batch_size]]).to(device=device, dtype=torch.float32)
        yield images, critic_fn(images)


def train(autoencoder, dset, critic_fn, device, epochs=P.epochs, batch_size=P.batch_size, lr=P.lr,
          log_n=None, log=print):
    """vae.py:33-66.  `dset`: list/array of (1,3,w,w) or (3,w,w) float frames in [0,1] — the reference's own
    host-side format: every batch is converted and copied synchronously, as vae.py:46-48 does — OR one uint8
    array (N,w,w,3), the frames as the environment delivers them: batches then come through FrameFeeder
    (pinned double buffer, H2D on a side stream, uint8 -> fp32 CHW/255 and the critic on the GPU, batch i+1
    in flight under step i).  `critic_fn(images) -> (B,1)` stands in for critic.evaluate (vae.py:50); with
    uint8 input it may also be a critic_vae_amd.critic.Critic."""
    u8 = isinstance(dset, np.ndarray) and dset.dtype == np.uint8
    if not u8:
        dset = np.stack(dset).squeeze()
    opt = torch.optim.Adam(autoencoder.parameters(), lr=lr)
    num_samples = dset.shape[0]
    log_n = log_n if log_n is not None else batch_size * 30
    history = []
    feeder = None
    if u8:
        from .feeder import FrameFeeder
        feeder = FrameFeeder(dset, batch_size, device, autoencoder.handle, critic=critic_fn)
    for ep in range(epochs):
        epoch_indices = np.arange(num_samples)
        np.random.shuffle(epoch_indices)
        starts = range(0, num_samples, batch_size)                              # tail batch is kept (vae.py:44-46)
        if feeder is not None:
            stream = feeder.batches([epoch_indices[b:b + batch_size] for b in starts])
        else:
            stream = _reference_batches(dset, epoch_indices, starts, batch_size, device, critic_fn)
        for batch_i, (images, preds) in zip(starts, stream):
            opt.zero_grad()
            out = autoencoder(images, preds)
            losses = autoencoder.vae_loss(out[0], out[1], out[2], out[3])
            losses["total_loss"].backward()
            opt.step()
            if batch_i % log_n == 0:
                rec = {k: float(v.item()) for k, v in losses.items()}
                history.append((num_samples * ep + batch_i + 1, rec))
                log(f"    ep:{ep}, imgs:{num_samples * ep + (batch_i + 1)} {rec}")
    return autoencoder, history


class FusedTrainer(DeviceTrainer):
    """One training step = forward + loss + backward + all-reduce + Adam on flat buffers."""

    def __init__(self, vae, lr=P.lr, betas=P.adam_betas, eps=P.adam_eps, process_group=None, world_size=1,
                 overlap=None, reduce_dtype=None, sync=True, global_stats=None, skip_nonfinite=False, max_grad_norm=None,
                 objective=None, augment=None, optim=None, trace=None):
        """Construction with world_size > 1 is a COLLECTIVE (sync_replicas: five broadcasts from rank 0) unless
        sync=False.
        overlap: all-reduce the gradient in three buckets while backward still runs (default for
        world_size > 1; CVAE_DP_OVERLAP=0 or overlap=False = one all-reduce after backward).
        reduce_dtype: "f32" (default; the contract of SURVEY 8e: reduced gradient == mean of the shard gradients
        within 1e-4) or "bf16" (CVAE_DP_REDUCE=bf16): the wire format of the all-reduce is bf16 — half the bytes,
        the summed gradient carries a relative rounding of 2^-9 per rank, optimizer state stays fp32.
        global_stats: global-batch semantics across ranks (CVAE_DP_GLOBAL_STATS=1; default off): the step runs in stages
        (include/cvae.h) and all-reduces the fp64 BatchNorm and loss sums between them (SUM on process_group; no exchange at
        world_size 1), so N ranks at B images train the model one rank trains at N*B — BatchNorm over the global batch,
        global MS-SSIM / KLD means.  The summed gradient is then the global-batch gradient: Adam's grad_scale is 1.
        skip_nonfinite / max_grad_norm: the guarded step (both off by default: the step then launches what it always did).
        The step ends in cvae_grad_stats + cvae_adam_step_guarded instead of cvae_adam_step: one pass over the REDUCED
        gradient (after the all-reduce and the bf16 unpack, with Adam's grad_scale) decides on the device — no host read —
        whether the update is applied (skip_nonfinite: not when the gradient holds an Inf or a NaN, torch's GradScaler rule;
        theta, m and v then keep their bits) and by how much it is scaled (max_grad_norm: torch's clip_grad_norm_ over the
        whole flat gradient).  Every rank reads the same reduced gradient, so every rank decides alike and the replicas
        stay bit-identical.  step_count keeps counting calls of step(); Adam's bias correction uses the device's count of
        APPLIED steps.  A skipped step still ran forward in training mode: num_batches_tracked and the BatchNorm running
        statistics are whatever forward wrote, as with a step torch's GradScaler skips.
        objective: an objective.Objective, or None = the reference's MS-SSIM + 0.001 * KLD through cvae_loss, with the launches
        and bits the step always had.  Otherwise the step calls cvae_loss_obj with objective.at(step_count): the four values
        travel by value in the launch, a schedule costs no copy and no synchronisation.  The objective is saved and restored
        with the trainer, so a run resumed in the middle of a warm-up continues exactly.  Not with global_stats: the fp64
        record of the staged step has no slot for the squared-error sum, and its finish step carries the reference weights.
        augment: an augment.Augment, or None = the plain batch gathers with the launches and bits fit_device always had.
        Otherwise fit_device (only) builds every batch with cvae_preprocess_u8_gather_aug / cvae_gather_f32_aug under
        augment.at(step_count): flip, shift and brightness happen inside the one gather launch, the key travels by value.
        The critic value of a sample stays the stored one.  evaluate() never augments, step() takes the batch it is given,
        fit_u8 (the host feeder) refuses.  A shift above width / 4 raises here; a ReconDataset with brightness > 0 raises in
        fit_device before the first launch.  Saved and restored with the trainer: the draw is step_count, so a resumed run
        applies exactly the transforms of the uninterrupted one.  With world_size > 1 every rank uses the same key on its
        own dataset indices; no collective is added.
        optim: an optim.Optim, or None = cvae_adam_step (or the guarded pair) at the constant `lr`, with the launches and bits the
        step always had.  Otherwise the step ends in cvae_adam_step_opt (cvae_grad_stats + cvae_adam_step_guarded_opt when
        guarded) — still one Adam launch — under optim.args_at(step): `lr` becomes the schedule's peak, weight decay (AdamW's
        decoupled form) touches the eleven weight tensors (optim.decay_ranges: no bias, no BatchNorm gamma / beta), and with
        optim.ema the launch also maintains `ema` (the averaged theta) and `aux_ema` (the averaged bn_state, which forward of
        the same step has already written).  Both are created by the first such step as copies of theta / bn_state, so
        load_networks after construction is safe.  evaluate(..., ema=True) runs on them, fit_device(val=...) judges them, and
        state_dict carries them with the Optim: a run resumed in the middle of a schedule continues exactly.  Works with
        global_stats and reduce_dtype="bf16" (the update is downstream of both); sync_replicas also broadcasts the averages.
        trace: a trace.Trace, or None = the step launches exactly what it always did.  Otherwise every step ends with
        cvae_trace_push (its 16 loss scalars, lr and the guard's decision into a device ring) and, every tensors_every steps,
        cvae_tensor_stats (per-tensor gradient / weight / update norms of the REDUCED gradient and the buffers Adam left); nothing
        is read on the host before trace.read().  Each rank traces its own loss scalars; no collective is added.  The trace is
        not part of state_dict()."""
        self.vae = vae
        self.h = vae.handle
        if overlap is None:
            overlap = os.environ.get("CVAE_DP_OVERLAP", "1") != "0"
        self.overlap = bool(overlap) and world_size > 1
        if reduce_dtype is None:
            reduce_dtype = os.environ.get("CVAE_DP_REDUCE", "f32")
        if reduce_dtype not in ("f32", "bf16"):
            raise ValueError(f"reduce_dtype {reduce_dtype!r}: 'f32' or 'bf16'")
        self.reduce_dtype = reduce_dtype
        if global_stats is None:
            global_stats = os.environ.get("CVAE_DP_GLOBAL_STATS") == "1"
        self.global_stats = bool(global_stats)
        if objective is not None and not isinstance(objective, Objective):
            raise ValueError(f"objective {objective!r}: an objective.Objective or None")
        if objective is not None and self.global_stats:
            raise ValueError("objective with global_stats=True: the staged cross-rank step (cvae_loss_stage) sums a fixed fp64 "
                             "record of the 11 MS-SSIM / KLD sums and finishes it with the reference weights; it has no slot for "
                             "the squared-error sum.  Use per-rank losses (global_stats=False) or objective=None")
        self.objective = objective
        self.buckets = [self.h.grad_bucket(ph) for ph in range(3)]
        self.lr, self.betas, self.eps = lr, betas, eps
        self._init_shared(skip_nonfinite, max_grad_norm, optim, trace)      # guard fields, step_count, val_history / best_val / val_stale, optim, trace
        self._init_augment(augment, vae.width)
        if self.optim is not None:
            self.optim.check_lr(self.lr)      # an lr_min above the peak raises here, not after the warm-up
        self.decay_ranges = decay_ranges(self.h.layout)
        self.world_size, self.pg = world_size, process_group
        dev = vae.theta.device
        n = vae.theta.numel()
        self.grads = torch.zeros(n, device=dev)
        self.grads16 = torch.empty(n, dtype=torch.bfloat16, device=dev) if (reduce_dtype == "bf16" and world_size > 1) else None
        self.m = torch.zeros(n, device=dev)
        self.v = torch.zeros(n, device=dev)
        B = vae.max_batch
        self.mu = torch.empty(B, P.latent_dim, device=dev)
        self.logvar = torch.empty_like(self.mu)
        self.recon = torch.empty(B, P.ch, vae.width, vae.width, device=dev)
        self.d_recon = torch.empty_like(self.recon)
        self.d_mu = torch.empty_like(self.mu)
        self.d_logvar = torch.empty_like(self.mu)
        self.scalars = torch.empty(16, device=dev)
        self.ws = vae._workspace(B)
        self.sync = torch.zeros(SYNC_DOUBLES, dtype=torch.float64, device=dev) if self.global_stats else None
        self.sync_slots = [self.h.sync_slot(p) for p in range(SYNC_POINTS)]
        self.exposed_ms = []              # measure_exposed: device time the compute stream spent waiting for the all-reduce
        self.measure_exposed = False
        self._ev = None
        if world_size > 1 and sync:
            if not torch.distributed.is_initialized():
                raise RuntimeError("FusedTrainer(world_size > 1) broadcasts rank 0's replica at construction (a COLLECTIVE: "
                                   "every rank must construct its trainer, in the same order): call "
                                   "torch.distributed.init_process_group / critic_vae_amd.dp.init() first, or pass "
                                   "sync=False and call sync_replicas() yourself")
            self.sync_replicas()

    def sync_replicas(self, src=0):
        """Every rank starts from rank `src`'s replica: parameters, BatchNorm running statistics and the Adam
        state are broadcast (torch DDP does the same at construction) — ranks built with different seeds,
        or one rank restored from a checkpoint, would otherwise train different models on the averaged
        gradient without any error."""
        dist = torch.distributed
        for t in (self.vae.theta.data, self.vae.bn_state, self.m, self.v):
            dist.broadcast(t, src=src, group=self.pg)
        counts = list(self._guard_read()) if self.guarded else []
        meta = torch.tensor([self.step_count, self.vae.num_batches_tracked] + counts, dtype=torch.int64, device=self.m.device)
        dist.broadcast(meta, src=src, group=self.pg)
        meta = meta.tolist()
        self.step_count, self.vae.num_batches_tracked = meta[0], meta[1]
        if self.guarded:
            self._guard_write(meta[2], meta[3])
        if self.has_ema():
            self._sync_ema(self.vae.theta.data, src)

    def _opt_aux(self):
        return self.vae.bn_state

    def step(self, x, pred, eps):
        """x (B,3,w,w), pred (B,1), eps (B,32): contiguous fp32 device tensors."""
        if self.global_stats:
            return self._step_global(x, pred, eps)
        v, h, B = self.vae, self.h, x.shape[0]
        theta = v.theta.data
        v._stamp_workspace()               # an autograd graph of the same VAE still pending is now stale (nets.py)
        h.forward(B, x, pred, eps, theta, v.bn_state, self.mu, self.logvar, self.recon, self.ws, train=True)
        if self.objective is None:
            h.loss(B, x, self.mu, self.logvar, self.recon, self.ws, self.scalars, self.d_recon, self.d_mu, self.d_logvar)
        else:
            h.loss_obj(B, x, self.mu, self.logvar, self.recon, self.ws, self.objective.at(self.step_count), self.scalars,
                       self.d_recon, self.d_mu, self.d_logvar)
        if self.world_size > 1 and self.overlap:
            # bucketed all-reduce overlapped with backward (torch DDP's scheme on the flat buffer): the
            # three buckets are contiguous ranges, each reduced (sum, RCCL) while the next phase computes
            works = []
            for ph in range(3):
                h.backward_phase(ph, B, x, pred, eps, theta, self.logvar, self.recon, self.d_recon, self.d_mu,
                                 self.d_logvar, self.ws, self.grads)
                works.append(self._reduce_bucket(ph))
            self._wait_buckets(works)
        else:
            h.backward(B, x, pred, eps, theta, self.logvar, self.recon, self.d_recon, self.d_mu, self.d_logvar,
                       self.ws, self.grads)
            self._reduce_all()
        self.step_count += 1
        v.num_batches_tracked += 1
        self._update(theta, 1.0 / self.world_size)
        return self.scalars

    def _reduce_bucket(self, ph):
        off, n = self.buckets[ph]
        if self.grads16 is not None:
            self.h.grads_to_bf16(self.grads[off:off + n], self.grads16[off:off + n])
            return torch.distributed.all_reduce(self.grads16[off:off + n], group=self.pg, async_op=True)
        return torch.distributed.all_reduce(self.grads[off:off + n], group=self.pg, async_op=True)

    def _wait_buckets(self, works):
        self._exposed_begin()
        for wk in works:
            wk.wait()                     # nccl: the compute stream waits for the collective's stream
        self._exposed_end()
        if self.grads16 is not None:
            self.h.grads_from_bf16(self.grads16, self.grads)

    def _reduce_all(self):
        if self.world_size > 1:
            self._exposed_begin()
            if self.grads16 is not None:
                self.h.grads_to_bf16(self.grads, self.grads16)
                torch.distributed.all_reduce(self.grads16, group=self.pg)
                self.h.grads_from_bf16(self.grads16, self.grads)
            else:
                torch.distributed.all_reduce(self.grads, group=self.pg)      # one flat RCCL all-reduce (sum)
            self._exposed_end()

    def _exchange(self, point):
        """Sum sync point `point` of the record over the ranks, in place (nothing to do on one rank)."""
        if self.world_size > 1:
            off, n = self.sync_slots[point]
            torch.distributed.all_reduce(self.sync[off:off + n], group=self.pg)

    def _step_global(self, x, pred, eps):
        """The step with global-batch statistics: forward / loss / backward in stages, the BatchNorm and loss sums
        all-reduced between them; gradient buckets as in step()."""
        v, h, B = self.vae, self.h, x.shape[0]
        theta, rec = v.theta.data, self.sync
        v._stamp_workspace()
        for k in range(5):
            h.forward_stage(k, B, x, pred, eps, theta, v.bn_state, self.mu, self.logvar, self.recon, self.ws, rec)
            if k < 4:
                self._exchange(k)
        h.loss_stage(0, B, x, self.mu, self.logvar, self.recon, self.ws, self.scalars, self.d_recon, self.d_mu,
                     self.d_logvar, rec)
        self._exchange(4)
        h.loss_stage(1, B, x, self.mu, self.logvar, self.recon, self.ws, self.scalars, self.d_recon, self.d_mu,
                     self.d_logvar, rec)
        bucketed = self.world_size > 1 and self.overlap
        works = []
        for k in range(5):
            h.backward_stage(k, B, x, pred, eps, theta, self.logvar, self.recon, self.d_recon, self.d_mu, self.d_logvar,
                             self.ws, self.grads, rec)
            if bucketed and k in (0, 1, 4):                 # the stages that complete buckets 0, 1, 2
                works.append(self._reduce_bucket(len(works)))
            if k < 4:
                self._exchange(5 + k)
        if bucketed:
            self._wait_buckets(works)
        else:
            self._reduce_all()
        self.step_count += 1
        v.num_batches_tracked += 1
        self._update(theta, 1.0)                     # the summed gradient already is the global-batch gradient
        return self.scalars

    # ---- checkpoint ----
    def state_dict(self):
        """What a restart needs beside the two network files: the Adam moments (CPU copies), step_count, the applied / skipped
        counters (an unguarded trainer applied every step) and the VAE's num_batches_tracked.  With the networks restored by
        load_networks, a resumed run is exact at the step() level — the caller supplies eps; the generators that fit_* draw
        shuffles and eps from are not saved.  "objective": the objective's state_dict (absent with objective=None);
        "augment": the augmentation's (absent with augment=None)."""
        state = {"m": self.m.detach().cpu().clone(), "v": self.v.detach().cpu().clone(),
                 "num_batches_tracked": int(self.vae.num_batches_tracked), **self._shared_state()}
        if self.objective is not None:
            state["objective"] = self.objective.state_dict()
        return state

    def load_state_dict(self, state):
        if state["m"].numel() != self.m.numel() or state["v"].numel() != self.v.numel():
            raise ValueError(f"trainer state of {state['m'].numel()} parameters, this trainer has {self.m.numel()}")
        saved = state.get("objective")
        if saved is not None and self.global_stats:
            raise ValueError("the state carries an objective, this trainer runs the staged cross-rank step (global_stats=True)")
        restored = None if saved is None else Objective().load_state_dict(saved)      # raises before anything changes
        self._load_shared_state(state)
        if restored is not None:           # a state without one keeps what the trainer was built with
            self.objective = restored
        self.m.copy_(state["m"])
        self.v.copy_(state["v"])
        self.vae.num_batches_tracked = int(state["num_batches_tracked"])

    def fit_u8(self, frames_u8, critic, batch_size, epochs=1, generator=None, shuffle=True):
        """The `-train` loop (vae.py:40-58) over a host uint8 dataset (N,w,w,3), fused step + overlapped feeder:
        batch i+1 is gathered, copied (pinned, side stream) while step i computes; uint8 -> fp32 CHW/255 and the
        critic run on the GPU.  eps ~ N(0,1) from `generator` (device).  Returns the loss scalars of the last step."""
        from .feeder import FrameFeeder
        if self.augment is not None:
            raise ValueError("fit_u8 with an augmentation: the transforms live in the device gathers (fit_device); the host "
                             "feeder path has none")
        dev = self.vae.theta.device
        feeder = FrameFeeder(frames_u8, batch_size, dev, self.h, critic=critic)
        n, scal = frames_u8.shape[0], None
        for _ in range(epochs):
            idx = np.arange(n)
            if shuffle:
                np.random.shuffle(idx)
            for images, preds in feeder.batches([idx[b:b + batch_size] for b in range(0, n, batch_size)]):
                eps = torch.randn(images.shape[0], P.latent_dim, device=dev, generator=generator)
                scal = self.step(images, preds, eps)
        return scal

    def _check_dataset(self, dataset, batch_size):
        dev = self.vae.theta.device
        if dataset.width != self.vae.width:
            raise ValueError(f"the dataset holds {dataset.width}x{dataset.width} frames, the VAE takes {self.vae.width}x{self.vae.width}")
        if not 1 <= int(batch_size) <= self.h.max_batch:
            raise ValueError(f"batch_size {batch_size} outside 1..max_batch ({self.h.max_batch}) of the handle")
        if dataset.frames.device != dev:
            raise ValueError(f"the dataset is on {dataset.frames.device}, the VAE on {dev}")
        return dev, int(batch_size)

    def evaluate(self, dataset, batch_size, per_image=False, ema=False):
        """The model on a held-out DeviceDataset / ReconDataset: per batch one gather launch, the EVAL-mode forward (BatchNorm
        on its running statistics, z = mu, i.e. eps = 0, the entries' own critic values) and cvae_score into ONE pooled device
        record; the host reads once, at the end.  Returns a dict of host values:
          total_loss, recon_loss, KLD, ssim_levels (5), cs_levels (5): POOLED — the scalars cvae_loss would give had the whole
            set been one batch (global level means over all images, KLD mean over all images); not a mean of batch losses, so
            the value does not depend on batch_size;
          images, finite_images: entries seen, and those whose per-image total is finite (a negative per-image level mean makes
            an image's MS-SSIM NaN, as in the reference; such an image is counted, not hidden);
          mean_total, mean_msssim, mean_kld, mean_mse: means of the per-image scores over the finite images; psnr = 10 log10(1 /
            mean_mse) (frames in [0, 1]); worst: the largest finite per-image total;
          per_image (only with per_image=True): the (N, 8) device tensor of cvae_score's rows, in dataset order.
          objective, kld_raw (only when the trainer has an objective): objective.compose on this result — with the FINAL weights
            (objective.final()), so that values from different steps of a warm-up compare: msssim * recon_loss (pooled; omitted,
            not multiplied, at weight 0) + mse * mean_mse + kld * kld_raw, kld_raw = -0.5 * rec[10] / rec[11], the pooled KLD mean
            without its weight.  mean_mse is the record's mean over finite_images ONLY: an image whose per-image MS-SSIM is NaN
            is left out of it, also under a pure-MSE objective.  Computed on the host from the same one read.
        Draws nothing from any random generator and leaves parameters, Adam state, bn_state, num_batches_tracked, step_count
        and the guard record untouched; it overwrites the workspace and the trainer's mu / logvar / recon buffers, which a
        step() rewrites before reading.  With world_size > 1 every rank evaluates the dataset IT is given and no collective
        runs: give every rank the same set (identical results on identical replicas) or reduce the per-rank results yourself.
        ema=True (a trainer whose Optim has an EMA): the same loop on the averaged weights and the averaged BatchNorm statistics
        (`ema`, `aux_ema`; before the first step temporaries, copies of theta and bn_state that are not kept).  Only the two pointers differ."""
        dev, B = self._check_dataset(dataset, batch_size)
        v, h, n = self.vae, self.h, len(dataset)
        if n < 1:
            raise ValueError("evaluate(): the dataset is empty")
        x = torch.empty(B, P.ch, v.width, v.width, device=dev)
        pred = torch.empty(B, 1, device=dev)
        zero = torch.zeros(B, P.latent_dim, device=dev)
        rows = torch.empty(n, SCORE_COLS, device=dev) if per_image else None
        state = h.score_state(dev)
        d_idx = torch.arange(n, dtype=torch.int64, device=dev)
        theta, bn_state = v.theta.data, v.bn_state
        if ema:
            if not self.has_ema():
                raise ValueError("evaluate(ema=True): this trainer keeps no averaged weights (optim=Optim(ema=...))")
            theta, bn_state = self._ema_view(theta)
        v._stamp_workspace()
        for b in range(0, n, B):
            nb = min(B, n - b)
            dataset.gather(h, nb, d_idx[b:b + nb], x[:nb], pred[:nb])
            h.forward(nb, x[:nb], pred[:nb], zero[:nb], theta, bn_state, self.mu, self.logvar, self.recon, self.ws, train=False)
            h.score(nb, x[:nb], self.mu, self.logvar, self.recon, self.ws, None if rows is None else rows[b:b + nb], state)
        scal = torch.empty(N_SCALARS, device=dev)
        h.score_finish(state, scal)
        host = torch.cat([state[:18], scal.to(torch.float64)]).cpu().numpy()        # the one host read
        rec, sc = host[:18], host[18:]
        fin = int(rec[12])
        mean = (lambda k: float(rec[k] / fin)) if fin else (lambda k: float("nan"))
        out = {"total_loss": float(sc[0]), "recon_loss": float(sc[1]), "KLD": float(sc[2]),
               "ssim_levels": [float(t) for t in sc[3:8]], "cs_levels": [float(t) for t in sc[8:13]],
               "images": int(rec[11]), "finite_images": fin,
               "mean_total": mean(13), "mean_msssim": mean(14), "mean_kld": mean(15), "mean_mse": mean(16),
               "worst": float(rec[17]) if fin else float("nan")}
        out["psnr"] = float(10.0 * np.log10(1.0 / out["mean_mse"])) if fin and out["mean_mse"] > 0 else float("inf" if fin else "nan")
        if self.objective is not None:
            out["kld_raw"] = float(-0.5 * rec[10] / rec[11]) if rec[11] > 0 else float("nan")
            out["objective"] = compose(self.objective, out)
        if per_image:
            out["per_image"] = rows
        return out

    def latent_report(self, dataset, batch_size, ema=False, au_threshold=0.01, collapsed_below=0.01):
        """The latent audit of the model on a DeviceDataset / ReconDataset (latent.py): the loop of evaluate() with the encoder
        alone — per batch one gather launch, the EVAL-mode cvae_forward with recon == NULL (BatchNorm on its running statistics,
        eps = 0) and one cvae_latent_stats launch into ONE pooled device record — then one host read and latent.summarize on
        it.  Returns that dict (per-dimension KL, active units, the linear probe of the critic value on mu, ..., and the
        record itself under "record").  Like evaluate() it draws nothing from any random generator and leaves parameters, Adam
        state, bn_state, num_batches_tracked, step_count and the guard record untouched; it overwrites the workspace (its
        batch buffers are its own: latent.dataset_report, which needs no trainer).  Every rank reports the set it is given; ema=True as in evaluate()."""
        from .latent import dataset_report
        _, B = self._check_dataset(dataset, batch_size)
        theta, bn_state = self.vae.theta.data, self.vae.bn_state
        if ema:
            if not self.has_ema():
                raise ValueError("latent_report(ema=True): this trainer keeps no averaged weights (optim=Optim(ema=...))")
            theta, bn_state = self._ema_view(theta)
        return dataset_report(self.vae, dataset, B, theta=theta, bn_state=bn_state, au_threshold=au_threshold,
                              collapsed_below=collapsed_below)

    def fit_device(self, dataset, batch_size, epochs=1, generator=None, shuffle=True, val=None, val_every=None, on_val=None):
        """The loop of fit_u8 over a DeviceDataset (episodes.py) that already lives on the device with its critic values:
        per epoch np.random.shuffle of the host indices (uploaded once), slices of batch_size with the ragged last batch
        kept, eps ~ N(0,1) from `generator`; each batch is one cvae_preprocess_u8_gather launch (x = frames[idx] / 255,
        pred = preds[idx]) and step() — no host gather, no PCIe copy, no critic launch.  A ReconDataset (fp32 entries, the
        second VAE's training set) runs the identical loop with cvae_gather_f32 as the batch launch.  Returns the last step's
        scalars.
        val: a held-out dataset of the same kind (episodes.split_by_trajectory).  It is evaluated (evaluate(val, batch_size))
        after every `val_every` optimizer steps — default: at the end of every epoch —, (step_count, result) is appended to
        self.val_history and on_val(trainer, result) is called; a true return value ends the fit there.  The evaluation draws
        no random number and touches no training state, so the training run is bit for bit the one without it.  val=None:
        the loop and its launches are exactly the ones above."""
        dev, B = self._check_dataset(dataset, batch_size)
        if val is not None:
            self._check_dataset(val, batch_size)
        x = torch.empty(B, P.ch, self.vae.width, self.vae.width, device=dev)
        pred = torch.empty(B, 1, device=dev)

        def batch(xb, predb):                              # eps is drawn after the gather, before the step
            return self.step(xb, predb, torch.randn(xb.shape[0], P.latent_dim, device=dev, generator=generator))

        return self._fit(dataset, B, epochs, shuffle, x, pred, batch, val, val_every, on_val, min(B, self.h.max_batch))

    # time between "backward is done" and "the reduced gradient is usable" on the compute stream = the part
    # of the all-reduce that backward did not hide (bench.py: allreduce_exposed_us)
    def _exposed_begin(self):
        if self.measure_exposed:
            self._ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self._ev[0].record()

    def _exposed_end(self):
        if self.measure_exposed:
            self._ev[1].record()
            self.exposed_ms.append(self._ev)
            if len(self.exposed_ms) > 1024:          # ring: a long run without exposed_us() keeps the newest samples only
                del self.exposed_ms[:512]

    def exposed_us(self):
        """Mean exposed all-reduce time per step (µs) over the steps taken with measure_exposed; syncs."""
        if not self.exposed_ms:
            return None
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in self.exposed_ms]
        self.exposed_ms = []
        return 1e3 * sum(ms) / len(ms)


def synthetic_dataset(n_frames, width=P.w, seed=1234):
    x, _, _ = synth.make_batch(seed, 0, n_frames, width)
    return [x[i:i + 1] for i in range(n_frames)]


ENCODER_FILE, DECODER_FILE = "vae_encoder.pt", "vae_decoder.pt"      # vae_parameters.py:25-26 (under saved-networks/)
SECOND_ENCODER_FILE, SECOND_DECODER_FILE = "vae2_encoder.pt", "vae2_decoder.pt"      # SECOND_*_PATH, vae_parameters.py


def _network_files(directory, second):
    enc, dec = (SECOND_ENCODER_FILE, SECOND_DECODER_FILE) if second else (ENCODER_FILE, DECODER_FILE)
    return os.path.join(directory, enc), os.path.join(directory, dec)


def save_networks(vae, directory, second=False):
    """End of `-train` (vae.py:162-163): torch.save(vae.encoder.state_dict(), ENCODER_PATH) and the same for the decoder —
    the reference's key names and layouts (OIHW conv weights, (C,H,W)-ordered fc columns / decoder_input rows, BatchNorm
    running statistics), so the two files load into the reference's own modules with strict=True and into
    `VariationalAutoencoder.encoder / .decoder.load_state_dict` here.  second: the second VAE's file names (vae.py:151-152).
    Returns the two paths."""
    os.makedirs(directory, exist_ok=True)
    enc, dec = _network_files(directory, second)
    torch.save({k: v.detach().cpu() for k, v in vae.encoder.state_dict().items()}, enc)
    torch.save({k: v.detach().cpu() for k, v in vae.decoder.state_dict().items()}, dec)
    return enc, dec


def load_networks(vae, directory, device=None, second=False):
    """load_vae_network (vae_utility.py:345-361) for the two files save_networks / the reference wrote."""
    enc, dec = _network_files(directory, second)
    vae.encoder.load_state_dict(torch.load(enc, map_location=device or "cpu"))
    vae.decoder.load_state_dict(torch.load(dec, map_location=device or "cpu"))
    return vae


def save_ema_networks(trainer, directory, second=False):
    """The network files of a FusedTrainer's AVERAGED weights and BatchNorm statistics (the CLI's DIR/ema/), in save_networks'
    format: load_networks / --networks DIR/ema of every mode loads them.  The live parameters are swapped out for the time of
    the save and put back; nothing of the trainer changes."""
    vae = trainer.vae
    ema, aux_ema = trainer._ema_view(vae.theta.data)
    live_theta, live_bn = vae.theta.data.clone(), vae.bn_state.clone()
    try:
        vae.theta.data.copy_(ema)
        vae.bn_state.copy_(aux_ema)
        save_networks(vae, directory, second=second)
    finally:
        vae.theta.data.copy_(live_theta)
        vae.bn_state.copy_(live_bn)
    return directory


TRAINER_FILE = "trainer.pt"


def save_trainer(trainer, path):
    """FusedTrainer.state_dict() -> `path` (torch.save; the CLI writes DIR/trainer.pt beside the two network files)."""
    torch.save(trainer.state_dict(), path)
    return path


def load_trainer(trainer, path):
    """The counterpart of save_trainer; load the networks (load_networks) as well to continue a run."""
    trainer.load_state_dict(torch.load(path, map_location="cpu"))
    return trainer


def build_parser():
    """The command line of this module (main() parses with it; host tests read it without a GPU)."""
    ap = argparse.ArgumentParser(description="Critic-VAE -train on synthetic frames (vae.py:154-163)")
    ap.add_argument("--save", metavar="DIR", default=None,
                    help="write DIR/vae_encoder.pt and DIR/vae_decoder.pt when training ends (vae.py:162-163; the reference's "
                         "DIR is saved-networks/)")
    ap.add_argument("-train", action="store_true")
    ap.add_argument("-dataset", dest="dataset_mode", action="store_true",
                    help="build the second VAE's training set (vae.py:130-140): the first VAE's eval-mode reconstructions of "
                         "the curated frames; needs --episodes, --critic, --networks, --out")
    ap.add_argument("-second", action="store_true",
                    help="train a fresh VAE on that set (vae.py:142-153); needs --dataset and --critic (the critic\'s values of "
                         "the entries are cached in the dataset; the checkpoint names the critic it was built with); --save DIR writes "
                         "DIR/vae2_encoder.pt and DIR/vae2_decoder.pt")
    ap.add_argument("-critic", dest="critic_mode", action="store_true",
                    help="train the critic itself on recorded trajectories and their rewards (critic_train.py); needs --episodes, "
                         "--rewards and --save; writes DIR/critic.pt in the reference's checkpoint format, which --critic of the "
                         "other modes loads; --critic CKPT starts from a checkpoint instead of fresh weights; takes --val-fraction, "
                         "--val-every, --keep-best (DIR/best/critic.pt) and --patience, judged by the chosen --loss on held-out trajectories")
    ap.add_argument("--eval-only", action="store_true",
                    help="-critic: train nothing; evaluate the checkpoint --critic on ALL frames of --episodes / --rewards under this "
                         "project's target recipe (--gamma, --shift) and print the result; writes nothing, needs no --save")
    ap.add_argument("--rewards", nargs="+", metavar="PATH", default=None,
                    help="-critic: .npy files (T,) or directories of them, one per trajectory, named as the trajectory's frame file")
    ap.add_argument("--lr", type=float, default=1e-4, help="-critic: Adam's learning rate")
    ap.add_argument("--dropout", type=float, default=0.3, help="-critic: p of the critic's three Dropout layers")
    ap.add_argument("--loss", choices=("bce", "mse"), default="bce", help="-critic: the loss on the sigmoid output")
    ap.add_argument("--gamma", type=float, default=0.98, help="-critic: discount of the value targets (episodes.discounted_targets)")
    ap.add_argument("--shift", type=int, default=12, help="-critic: frames by which the rewards are moved earlier")
    ap.add_argument("--datasize", type=int, default=None, metavar="N", help="-critic: frames drawn over all trajectories (default: all)")
    ap.add_argument("--networks", metavar="DIR", default="saved-networks", help="-dataset: directory with the first VAE's "
                    f"{ENCODER_FILE} and {DECODER_FILE}")
    ap.add_argument("--out", metavar="FILE", default=None, help="-dataset: where the recon dataset goes (plain arrays)")
    ap.add_argument("--pickle", metavar="FILE", default=None, help="-dataset: also write the reference's recon-dataset.pickle")
    ap.add_argument("--dataset", metavar="FILE", default=None, help="-second: the file -dataset --out wrote")
    ap.add_argument("--synthetic", type=int, default=1024, help="number of synthetic frames")
    ap.add_argument("--batch", type=int, default=P.batch_size)
    ap.add_argument("--epochs", type=int, default=None, help="default 1; -critic: 15")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--critic", default=None, help="'random' scalars (BASELINE config 1; the default without --episodes), "
                    "'synth' = the HIP critic with generator weights, or a path to a reference critic checkpoint (.pt)")
    ap.add_argument("--episodes", nargs="+", metavar="PATH", default=None,
                    help="train on recorded trajectories: .npy files (T,64,64,3) uint8 or directories of them, curated as "
                         "load_minerl_data(critic) does (vae_utility.py:393-461); needs --critic")
    ap.add_argument("--total-images", type=int, default=P.total_images, help="dataset size at which the walk over the "
                    "trajectories stops (vae_parameters.py:19)")
    ap.add_argument("--collect", type=int, default=P.collect, help="frames per critic-value bin and trajectory "
                    "(vae_utility.py:404)")
    ap.add_argument("--skip-nonfinite", action="store_true", help="fused trainer (--episodes, -second): skip the update of a step "
                    "whose gradient holds an Inf or a NaN (decided on the device)")
    ap.add_argument("--max-grad-norm", type=float, default=None, metavar="C", help="fused trainer: clip the gradient to global "
                    "norm C (torch.nn.utils.clip_grad_norm_)")
    ap.add_argument("--resume", metavar="DIR", default=None, help=f"fused trainer: continue from DIR's network files and {TRAINER_FILE} "
                    "(what --save wrote); the run continues under the objective saved there — objective flags are not needed, and "
                    "flags that describe another objective are refused")
    ap.add_argument("--val-fraction", type=float, default=None, metavar="F", help="fused trainer: hold out whole trajectories until "
                    "they make up at least F of the curated entries (episodes.split_by_trajectory, seeded by --seed) and evaluate on them")
    ap.add_argument("--val-every", type=int, default=None, metavar="N", help="with --val-fraction: evaluate after every N optimizer "
                    "steps (default: at the end of every epoch)")
    ap.add_argument("--keep-best", action="store_true", help="with --val-fraction and --save DIR: write the network files under "
                    "DIR/best/ whenever the pooled validation total_loss improves (a non-finite value never does)")
    ap.add_argument("--patience", type=int, default=None, metavar="K", help="with --val-fraction: stop after K evaluations in a row "
                    "without an improvement")
    ap.add_argument("--latent-report", action="store_true", help="-train --episodes, -second: after the fit print the latent audit "
                    "(latent.py: KL per dimension, active units, the linear probe of the critic value on mu) of the held-out set "
                    "(--val-fraction), or of the training set without one; with --save DIR also DIR/latent.npz")
    ap.add_argument("--msssim-weight", type=float, default=None, metavar="W", help="-train, -second: weight of the MS-SSIM term "
                    "(reference: 1).  Any of these six flags switches the loss to cvae_loss_obj; validation is then judged by the objective")
    ap.add_argument("--mse-weight", type=float, default=None, metavar="W", help="weight of F.mse_loss(recon, x), the reference's "
                    "commented-out reconstruction term (vae_nets.py:54; reference: 0)")
    ap.add_argument("--kld-weight", type=float, default=None, metavar="BETA", help=f"weight of the KLD (reference: {P.kld_weight})")
    ap.add_argument("--msssim-grad", choices=("reference", "used"), default=None, help="'used': differentiate only the level terms the "
                    "MS-SSIM product uses — the same loss, and no NaN gradient from a negative unused level mean (README)")
    ap.add_argument("--kld-warmup", type=int, default=None, metavar="N", help="fused trainer: KLD weight * min(1, (step + 1) / N)")
    ap.add_argument("--msssim-from", type=int, default=None, metavar="N", help="fused trainer: no MS-SSIM term (and no pyramid) before "
                    "optimizer step N; needs --mse-weight > 0")
    ap.add_argument("--augment-flip", type=float, default=None, metavar="P", help="-train --episodes, -second, -critic: flip a "
                    "gathered frame horizontally with probability P.  Any of these four flags moves the batch gather to its "
                    "augmented kernel (augment.py); critic values / targets stay the stored ones; validation never augments")
    ap.add_argument("--augment-shift", type=int, default=None, metavar="S", help="shift by dx, dy in [-S, S] whole pixels, edges "
                    "replicated; S <= width / 4")
    ap.add_argument("--augment-brightness", type=float, default=None, metavar="B", help="gain within 1 +- B on uint8 frames, "
                    "clamped at 1 (not -second: its entries are Tanh outputs)")
    ap.add_argument("--augment-seed", type=int, default=None, metavar="N", help="seed of the per-sample hash (default 0)")
    ap.add_argument("--lr-schedule", choices=("constant", "linear", "cosine"), default=None, help="-train --episodes, -second, "
                    "-critic: the learning rate after the warm-up, with the run's lr as the peak.  Any of these seven flags moves the "
                    "Adam launch to its _opt kernel (optim.py): schedule, weight decay and EMA ride in that one launch")
    ap.add_argument("--lr-warmup", type=int, default=None, metavar="N", help="lr * (step + 1) / N over the first N optimizer steps")
    ap.add_argument("--lr-min", type=float, default=None, metavar="F", help="where the linear / cosine schedule ends (default 0)")
    ap.add_argument("--lr-total", type=int, default=None, metavar="N", help="the step at which it gets there (default: epochs * "
                    "ceil(training entries / batch), the whole run)")
    ap.add_argument("--weight-decay", type=float, default=None, metavar="W", help="decoupled weight decay (torch.optim.AdamW) on the "
                    "weight tensors; biases and BatchNorm gamma / beta are left alone")
    ap.add_argument("--ema", type=float, default=None, metavar="D", help="keep an exponential moving average of the weights (and of "
                    "the BatchNorm statistics) with decay D; validation judges it, --save DIR also writes DIR/ema/")
    ap.add_argument("--ema-warmup", action="store_true", help="with --ema: decay min(D, (1 + step) / (10 + step))")
    ap.add_argument("--trace-out", metavar="FILE.npz", default=None, help="-train --episodes, -second, -critic: keep a training trace on "
                    "the device (trace.py) and write it wherever the run saves; an existing file of the same run is continued "
                    "(--resume).  python -m critic_vae_amd.trace FILE.npz prints it")
    ap.add_argument("--trace-every", type=int, default=None, metavar="N", help="with --trace-out: a step row (loss scalars, lr, the "
                    "guard's decision) every N optimizer steps (default 1; 0: none)")
    ap.add_argument("--trace-tensors-every", type=int, default=None, metavar="M", help="with --trace-out: per-tensor gradient / weight / "
                    "update norms every M optimizer steps (default 0: none)")
    ap.add_argument("--trace-capacity", type=int, default=None, metavar="C", help="with --trace-out: rows of the step ring (default 4096; "
                    "older rows are overwritten)")
    return ap


OPTIM_FLAGS = "--lr-schedule, --lr-warmup, --lr-min, --lr-total, --weight-decay, --ema and --ema-warmup"
EMA_DIR = "ema"


def optim_kwargs_from_args(args):
    """The Optim arguments the seven optimizer flags give, or None when none of them is given (the plain Adam launch).  `total`
    may be missing: optim_from_kwargs fills in the length of the run once the training set is known."""
    given = {"schedule": args.lr_schedule, "warmup": args.lr_warmup, "lr_min": args.lr_min, "total": args.lr_total,
             "weight_decay": args.weight_decay, "ema": args.ema, "ema_warmup": True if args.ema_warmup else None}
    given = {k: v for k, v in given.items() if v is not None}
    return given or None


def optim_from_kwargs(kw, default_total):
    """Optim(**kw) with --lr-total's default for a decaying schedule; None stays None.  Raises ValueError as Optim does."""
    if kw is None:
        return None
    if "total" not in kw and kw.get("schedule", "constant") != "constant":
        kw = dict(kw, total=int(default_total))
    return Optim(**kw)


def _run_steps(args, n_entries):
    return args.epochs * ((n_entries + args.batch - 1) // args.batch)


def _settle_optim(args, trainer, provisional, n_entries, directory):
    """After the training set is known: the Optim of the flags with its final `total`, installed in a fresh run; in a resumed
    one the checkpoint's Optim continues, and flags that describe another one are refused (the rule of the objective)."""
    try:
        given = optim_from_kwargs(getattr(args, "optim_kw", None), _run_steps(args, n_entries))
    except ValueError as e:
        raise SystemExit(str(e))
    saved = trainer.optim if (directory and trainer.optim is not provisional) else None
    try:                                   # an lr_min above the run's lr: an argument error now, not a ValueError after the warm-up
        for o in (given, saved):
            if o is not None:
                o.check_lr(trainer.lr)
    except ValueError as e:
        raise SystemExit(str(e))
    if not directory:
        trainer.optim = given
    elif given is None:
        if saved is not None:
            print(f"continuing with the optimizer options saved in {directory}")
    elif saved is None or saved != given:
        was = "none (the plain Adam launch at a constant lr)" if saved is None else repr(saved)
        raise SystemExit(f"--resume {directory}: the checkpoint's optimizer options are {was}, the flags give {given!r}.  A resumed "
                         "run keeps its schedule, weight decay and EMA: drop the optimizer flags, or repeat the run's own")
    if trainer.optim is not None:
        print(trainer.optim.describe())


def trace_from_args(args):
    """The Trace the four --trace-* flags describe, or None when none of them is given.  Raises ValueError as Trace does, and
    for flags without --trace-out."""
    given = {"every": args.trace_every, "tensors_every": args.trace_tensors_every, "capacity": args.trace_capacity}
    given = {k: v for k, v in given.items() if v is not None}
    if args.trace_out is None:
        if given:
            raise ValueError("--trace-every, --trace-tensors-every and --trace-capacity need --trace-out FILE.npz")
        return None
    return Trace(**given)


def _save_trace(args, trainer):
    """--trace-out: the trainer's trace -> the file (one device -> host copy of each ring); called wherever the run saves."""
    trace, path = getattr(trainer, "trace", None), getattr(args, "trace_out", None)
    if trace is not None and path:
        print(f"saved {trace.save(path)}")


def augment_from_args(args):
    """The Augment the four --augment-* flags describe, or None when none of them is given.  Raises ValueError as Augment does."""
    given = {"flip": args.augment_flip, "shift": args.augment_shift, "brightness": args.augment_brightness, "seed": args.augment_seed}
    given = {k: v for k, v in given.items() if v is not None}
    return Augment(**given) if given else None


def objective_from_args(args):
    """The Objective the six objective flags describe, or None when none of them is given (the reference loss through cvae_loss).
    Raises ValueError as Objective does."""
    given = {"msssim": args.msssim_weight, "mse": args.mse_weight, "kld": args.kld_weight, "msssim_grad": args.msssim_grad,
             "kld_warmup": args.kld_warmup, "msssim_from": args.msssim_from}
    given = {k: v for k, v in given.items() if v is not None}
    return Objective(**given) if given else None


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    try:
        args.objective = objective_from_args(args)
    except ValueError as e:
        ap.error(str(e))
    if args.objective is not None and not (args.train or args.second):
        ap.error("--msssim-weight, --mse-weight, --kld-weight, --msssim-grad, --kld-warmup and --msssim-from belong to -train and -second")
    if args.objective is not None and args.train and args.episodes is None and (args.objective.kld_warmup or args.objective.msssim_from):
        ap.error("--kld-warmup and --msssim-from belong to the fused trainer (-train --episodes, -second): the synthetic -train "
                 "loop is the reference's own and follows no schedule")
    try:
        args.augment = augment_from_args(args)
        if args.augment is not None:
            args.augment.check_width(P.w)
    except ValueError as e:
        ap.error(str(e))
    if args.augment is not None:
        if not ((args.train and args.episodes is not None) or args.second or (args.critic_mode and not args.eval_only)):
            ap.error("--augment-flip, --augment-shift, --augment-brightness and --augment-seed belong to the runs that gather their "
                     "batches on the device: -train --episodes, -second and -critic")
        if args.second and args.augment.gain_q16 != 0:
            ap.error("-second takes no --augment-brightness: its entries are Tanh outputs in (-1, 1), a gain clamped at 1 has no "
                     "meaning for them")
    if args.max_grad_norm is not None and not args.max_grad_norm > 0:
        ap.error("--max-grad-norm needs a positive number")
    try:
        args.trace = trace_from_args(args)
    except ValueError as e:
        ap.error(str(e))
    if args.trace is not None and not ((args.train and args.episodes is not None) or args.second or (args.critic_mode and not args.eval_only)):
        ap.error("--trace-out, --trace-every, --trace-tensors-every and --trace-capacity belong to the fused trainers: "
                 "-train --episodes, -second and -critic")
    args.optim_kw = optim_kwargs_from_args(args)
    if args.optim_kw is not None:
        if not ((args.train and args.episodes is not None) or args.second or (args.critic_mode and not args.eval_only)):
            ap.error(f"{OPTIM_FLAGS} belong to the fused trainers: -train --episodes, -second and -critic")
        try:
            optim_from_kwargs(args.optim_kw, args.optim_kw.get("warmup", 0) + 1)
        except ValueError as e:
            ap.error(str(e))
    if args.latent_report and not ((args.train and args.episodes is not None) or args.second):
        ap.error("--latent-report belongs to the fused VAE trainer (-train --episodes, -second); python -m critic_vae_amd.latent "
                 "audits saved networks")
    if args.val_fraction is None:
        if args.val_every is not None or args.keep_best or args.patience is not None:
            ap.error("--val-every, --keep-best and --patience need --val-fraction")
    else:
        if not 0.0 < args.val_fraction < 1.0:
            ap.error("--val-fraction needs a number in (0, 1)")
        if (args.val_every is not None and args.val_every < 1) or (args.patience is not None and args.patience < 1):
            ap.error("--val-every and --patience need positive integers")
        if args.keep_best and args.save is None:
            ap.error("--keep-best needs --save DIR (the best networks go to DIR/best/)")
        if not (args.second or (args.train and args.episodes is not None) or args.critic_mode):
            ap.error("--val-fraction belongs to the fused trainer (-train --episodes, -second)")
    if args.train + args.dataset_mode + args.second + args.critic_mode != 1:
        ap.error("exactly one of -train, -dataset, -second, -critic (segment.py has -video [-thresh] [--second]); see SURVEY.md §8 for scope")
    if args.eval_only and not args.critic_mode:
        ap.error("--eval-only belongs to -critic")
    if args.critic_mode:
        if args.eval_only:
            if args.critic in (None, "random"):
                ap.error("--eval-only needs --critic (the checkpoint to evaluate)")
            if args.episodes is None or args.rewards is None:
                ap.error("-critic --eval-only needs --episodes and --rewards")
            if args.val_fraction is not None:
                ap.error("--eval-only evaluates every frame: it takes no --val-fraction")
            return _eval_critic(args)
        if args.episodes is None or args.rewards is None or args.save is None:
            ap.error("-critic needs --episodes, --rewards and --save")
        if args.critic == "random":
            ap.error("-critic --critic takes a checkpoint or 'synth'")
        if args.epochs is None:
            args.epochs = 15
        return _train_critic(args)
    if args.epochs is None:
        args.epochs = 1
    if args.dataset_mode:
        if args.episodes is None or args.critic in (None, "random") or args.out is None:
            ap.error("-dataset needs --episodes, --critic (a checkpoint or 'synth') and --out")
        return _build_recon_dataset(args)
    if args.second:
        if args.dataset is None or args.critic in (None, "random"):
            ap.error("-second needs --dataset (written by -dataset --out) and --critic")
        return _train_second(args)
    if args.episodes is not None and args.critic in (None, "random"):
        ap.error("--episodes needs --critic (a reference critic checkpoint, or 'synth'): the dataset is chosen by its values")
    if args.critic is None:
        args.critic = "random"
    if args.episodes is not None:
        return _train_episodes(args)
    if args.skip_nonfinite or args.max_grad_norm is not None or args.resume:
        ap.error("--skip-nonfinite, --max-grad-norm and --resume belong to the fused trainer (-train --episodes, -second); "
                 "the synthetic -train loop is the reference's own, with torch.optim.Adam")
    device = _device()
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    vae = VariationalAutoencoder(max_batch=args.batch, seed=args.seed).to(device)
    if args.objective is not None:
        vae.objective = args.objective
        print(args.objective.describe())
    dset = synthetic_dataset(args.synthetic)
    if args.critic == "random":
        critic_fn = lambda im: torch.rand(im.shape[0], 1, device=im.device)      # noqa: E731
    else:                                  # critic.evaluate(images), vae.py:50 / vae_utility.py:363-370
        critic_fn = _load_critic(args.critic, vae.handle, args.seed, device).evaluate
    t0 = time.time()
    _, hist = train(vae, dset, critic_fn, device,
                    epochs=args.epochs, batch_size=args.batch, log_n=args.batch * 8)
    torch.cuda.synchronize()
    dt = time.time() - t0
    print(f"{args.epochs * args.synthetic / dt:.1f} images/s over {args.epochs} epoch(s)")
    if args.save:
        enc, dec = save_networks(vae, args.save)
        print(f"saved {enc} and {dec}")
    return hist


def _device():
    """cuda:0, or the exit every mode takes without a GPU."""
    if not torch.cuda.is_available():
        raise SystemExit("critic-vae_amd needs an MI355X: the HIP library has no CPU fallback")
    return torch.device("cuda:0")


def _fit_and_save(args, vae, ds, second):
    """What -train --episodes and -second share once the dataset is on the device: seeds, FusedTrainer.fit_device, the rate
    line, save_networks.  Nothing before it draws from the global generators (the networks are built from args.seed)."""
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    kw = getattr(args, "optim_kw", None)
    provisional = optim_from_kwargs(kw, (kw or {}).get("warmup", 0) + 1)      # --lr-total's default needs the training set: _settle_optim
    trainer = FusedTrainer(vae, skip_nonfinite=args.skip_nonfinite, max_grad_norm=args.max_grad_norm,
                           objective=getattr(args, "objective", None), augment=getattr(args, "augment", None), optim=provisional,
                           trace=getattr(args, "trace", None))
    if args.resume:
        given, given_aug = trainer.objective, trainer.augment
        load_networks(vae, args.resume, second=second)
        load_trainer(trainer, os.path.join(args.resume, TRAINER_FILE))
        print(f"resumed from {args.resume} at step {trainer.step_count}")
        _check_resumed_objective(given, trainer, args.resume)
        _check_resumed_augment(given_aug, trainer, args.resume)
    if trainer.objective is not None:
        print(trainer.objective.describe())
    if trainer.augment is not None:
        print(trainer.augment.describe())
    gen = torch.Generator(device=vae.theta.device)
    gen.manual_seed(args.seed)
    ds, val_kw = _hold_out(args, ds, _ValidationLog(args, second, by_objective=trainer.objective is not None), "entries", curated=True)
    _settle_optim(args, trainer, provisional, len(ds), args.resume)
    t0 = time.time()
    scal = trainer.fit_device(ds, args.batch, epochs=args.epochs, generator=gen, **val_kw)
    torch.cuda.synchronize()
    dt = time.time() - t0
    s = scal.cpu().numpy()
    print(f"{args.epochs * len(ds) / dt:.1f} images/s over {args.epochs} epoch(s); last loss {s[0]:.6f} "
          f"(recon {s[1]:.6f}, kld {s[2]:.6f})")
    if args.save:
        enc, dec = save_networks(vae, args.save, second=second)
        print(f"saved {enc} and {dec}")
        print(f"saved {save_trainer(trainer, os.path.join(args.save, TRAINER_FILE))}")
        if trainer.has_ema():
            print(f"saved the averaged weights under {save_ema_networks(trainer, os.path.join(args.save, EMA_DIR), second=second)}")
    _save_trace(args, trainer)
    _print_guard(trainer)
    if getattr(args, "latent_report", False):
        from .latent import report_lines, save_npz
        held = val_kw.get("val")
        summary = trainer.latent_report(ds if held is None else held, args.batch)
        print(f"latent report on the {'training' if held is None else 'held-out'} set:")
        print("\n".join(report_lines(summary)))
        if args.save:
            print(f"saved {save_npz(os.path.join(args.save, LATENT_FILE), summary)}")
    return ds


def _check_resumed_objective(given, trainer, directory):
    """--resume with objective flags: the checkpoint's objective must be the one the flags describe.  A run continues under the
    objective it was started with — its schedules count from step 0 of that run, and best_val / val_stale were judged by that
    objective's validation entry (total_loss for a run without one) — so a different one is refused, not silently replaced in
    either direction.  Without flags the checkpoint's objective (or none) continues, with a line that says so."""
    saved = trainer.objective if trainer.objective is not given else None       # load_trainer replaced it only if the state carried one
    if given is None:
        if trainer.objective is not None:
            print(f"continuing with the objective saved in {directory}")
        return
    if saved is None or saved != given:
        was = "none (the reference loss through cvae_loss, validation judged by total_loss)" if saved is None else repr(saved)
        raise SystemExit(f"--resume {directory}: the checkpoint's objective is {was}, the flags give {given!r}.  A resumed run keeps "
                         "its objective (schedules, best_val and --patience refer to it): drop the objective flags, or repeat the run's own")


def _check_resumed_augment(given, trainer, directory):
    """--resume with --augment-* flags, by the rule of the objective: the transforms of step s are a function of (seed, s), so
    a resumed run continues the augmentation it was started with.  Without flags the saved one (or none) continues; flags that
    describe another one are refused with both named."""
    saved = trainer.augment if trainer.augment is not given else None       # load_trainer replaced it only if the state carried one
    if given is None:
        if trainer.augment is not None:
            print(f"continuing with the augmentation saved in {directory}")
        return
    if saved is None or saved != given:
        was = "none (the plain batch gathers)" if saved is None else repr(saved)
        raise SystemExit(f"--resume {directory}: the checkpoint's augmentation is {was}, the flags give {given!r}.  A resumed run "
                         "keeps its augmentation: drop the --augment-* flags, or repeat the run's own")


BEST_DIR = "best"
LATENT_FILE = "latent.npz"


def _has_ema(trainer):
    """Whether --keep-best saves averaged weights; a stand-in trainer without the method has none."""
    has = getattr(trainer, "has_ema", None)
    return bool(has()) if callable(has) else False


def _hold_out(args, ds, on_val, noun, curated):
    """--val-fraction: (the training part of ds, fit_device's val / val_every / on_val); without it (ds, {}).  curated: the
    dataset's names list the trajectories that gave entries (curate, curate_recon), not every trajectory (critic_dataset)."""
    if args.val_fraction is None:
        return ds, {}
    from .episodes import split_by_trajectory
    n_all = len(ds)
    ds, val = split_by_trajectory(ds, args.val_fraction, seed=args.seed)
    whole = (len(val.names) if curated else 0) or len(np.unique(val.source[:, 0]))
    print(f"held out {len(val)} of {n_all} {noun} ({whole} whole trajectories); training on {len(ds)}")
    return ds, dict(val=val, val_every=args.val_every, on_val=on_val)


def _print_guard(trainer):
    if trainer.guarded:
        st = trainer.guard_stats()
        print(f"guard: {st['applied']} steps applied, {st['skipped']} skipped")
        trace = getattr(trainer, "trace", None)
        if st["skipped"] > 0 and trace is not None and trace.tensors_every:
            found = nonfinite_tensors(trace.read())
            if found is not None:
                print(f"guard: the skipped step {found[0]} had non-finite gradients in {', '.join(found[1]) or 'no traced tensor'}")


class _KeepBestLog:
    """on_val of the command line: one line per evaluation, --keep-best and --patience.  The best value and the count of
    evaluations since it improved live in the trainer (best_val, val_stale: saved and resumed with it); a non-finite
    value never counts as an improvement.  A subclass names the judged entry of the result (`key`), writes the line and saves."""

    def __init__(self, args):
        self.args = args

    def __call__(self, trainer, r):
        loss = r[self.key]
        better = bool(np.isfinite(loss)) and (trainer.best_val is None or loss < trainer.best_val)
        print(f"val @ step {trainer.step_count}: {self.line(trainer, r)}{' *' if better else ''}")
        if better:
            trainer.best_val, trainer.val_stale = float(loss), 0
            if self.args.keep_best:
                self.save(trainer, os.path.join(self.args.save, BEST_DIR))
                _save_trace(self.args, trainer)
        else:
            trainer.val_stale += 1
        if self.args.patience is not None and trainer.val_stale >= self.args.patience:
            print(f"no improvement in {trainer.val_stale} evaluations: stopping at step {trainer.step_count}")
            return True
        return False


class _ValidationLog(_KeepBestLog):
    """The VAE's: judged by the pooled total_loss — by the result's "objective" entry when the run has an objective;
    --keep-best writes the two network files."""
    key = "total_loss"

    def __init__(self, args, second, by_objective=False):
        self.args, self.second = args, second
        if by_objective:
            self.key = "objective"

    def line(self, trainer, r):
        head = f"objective {r['objective']:.6f} " if self.key == "objective" else ""
        return (f"{head}loss {r['total_loss']:.6f} (recon {r['recon_loss']:.6f}, kld {r['KLD']:.6f}) over {r['images']} images, "
                f"{r['images'] - r['finite_images']} non-finite; per image: mean {r['mean_total']:.6f} worst {r['worst']:.6f} "
                f"psnr {r['psnr']:.2f} dB")

    def save(self, trainer, directory):                  # the weights that were judged: the averaged ones of a trainer with an EMA
        if _has_ema(trainer):
            save_ema_networks(trainer, directory, second=self.second)
        else:
            save_networks(trainer.vae, directory, second=self.second)


def _load_critic(spec, handle, seed, device):
    from .critic import Critic
    critic = Critic(handle=handle).to(device)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_critic_params(seed).items()} \
        if spec == "synth" else torch.load(spec, map_location="cpu")
    critic.load_state_dict(sd)
    return critic


def _train_episodes(args):
    """-train on recorded trajectories: curate (episodes.py) -> FusedTrainer.fit_device -> save_networks."""
    from .episodes import curate, load_episodes
    episodes = load_episodes(args.episodes)
    device = _device()
    vae = VariationalAutoencoder(max_batch=args.batch, seed=args.seed).to(device)
    critic = _load_critic(args.critic, vae.handle, args.seed, device)
    t0 = time.time()
    ds = curate(episodes, critic, collect=args.collect, total_images=args.total_images, device=device)
    torch.cuda.synchronize()
    print(f"curated {len(ds)} frames in {time.time() - t0:.2f} s")
    if len(ds) == 0:
        raise SystemExit("the curated dataset is empty: no frame of the trajectories falls in a critic-value bin")
    return _fit_and_save(args, vae, ds, second=False)


CRITIC_FILE = "critic.pt"


class _CriticValidationLog(_KeepBestLog):
    """`-critic`'s: judged by the trainer's chosen loss on the held-out frames; --keep-best writes DIR/best/critic.pt."""
    key = "loss"

    def line(self, trainer, r):
        return (f"{trainer.loss} {r['loss']:.6f} (bce {r['bce']:.6f}, mse {r['mse']:.6f}, mae {r['mae']:.6f}) "
                f"pearson {r['pearson']:.4f} bin agreement {r['bin_agreement']:.4f} worst {r['worst']:.4f} over {r['frames']} frames, "
                f"{r['frames'] - r['finite_frames']} non-finite")

    def save(self, trainer, directory):                  # likewise
        print(f"saved {_save_critic(trainer.critic, directory, ema=trainer if _has_ema(trainer) else None)}")


def _save_critic(critic, directory, ema=None):
    """DIR/critic.pt in the reference's checkpoint format (what --critic of every mode loads).  ema: a CriticTrainer with
    averaged weights — the file then holds those, cut up by the keys and shapes of the critic's own state_dict."""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, CRITIC_FILE)
    sd = critic.state_dict()
    if ema is not None:
        flat, off = ema._ema_view(ema.theta)[0], 0
        for k, v in sd.items():
            sd[k] = flat[off:off + v.numel()].reshape(v.shape).clone()
            off += v.numel()
    torch.save({k: v.detach().cpu() for k, v in sd.items()}, path)
    return path


def _critic_and_dataset(args, size):
    """What -critic and its --eval-only share: the trajectories with their rewards, the critic (fresh from --seed, or --critic)
    on a handle of its own, and the (frame, discounted target) dataset on the device."""
    from .critic import Critic
    from .critic_train import initial_state_dict
    from .episodes import critic_dataset, load_episodes, load_rewards
    from .lib import Handle
    episodes = load_episodes(args.episodes)
    rewards = load_rewards(args.rewards, episodes)
    device = _device()
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    handle = Handle(64, max(args.batch, 1))
    if args.critic is None:
        critic = Critic(handle=handle).to(device)
        critic.load_state_dict(initial_state_dict(args.seed))
    else:
        critic = _load_critic(args.critic, handle, args.seed, device)
    ds = critic_dataset(episodes, rewards, size=size, seed=args.seed, gamma=args.gamma, shift=args.shift, device=device)
    if len(ds) == 0:
        raise SystemExit("the critic's dataset is empty")
    return critic, ds, device


def _train_critic(args):
    """-critic: load_episodes + load_rewards -> critic_dataset (discounted targets) -> CriticTrainer.fit_device -> DIR/critic.pt."""
    from .critic_train import CriticTrainer
    critic, ds, device = _critic_and_dataset(args, args.datasize)
    trainer = CriticTrainer(critic, lr=args.lr, dropout=args.dropout, loss=args.loss, skip_nonfinite=args.skip_nonfinite,
                            max_grad_norm=args.max_grad_norm, augment=getattr(args, "augment", None), trace=getattr(args, "trace", None))
    if trainer.augment is not None:
        print(trainer.augment.describe())
    gen = torch.Generator(device=device)
    gen.manual_seed(args.seed)
    ds, val_kw = _hold_out(args, ds, _CriticValidationLog(args), "frames", curated=False)
    _settle_optim(args, trainer, None, len(ds), None)
    t0 = time.time()
    log = trainer.fit_device(ds, args.batch, epochs=args.epochs, generator=gen, **val_kw)
    torch.cuda.synchronize()
    dt = time.time() - t0
    s = log.cpu().numpy()
    steps, per_epoch = s.shape[0], (len(ds) + args.batch - 1) // args.batch
    images = steps // per_epoch * len(ds) + steps % per_epoch * args.batch          # a fit that --patience ended took fewer steps
    span = f"{args.epochs} epoch(s)" if steps == args.epochs * per_epoch else f"{steps} steps"
    per_epoch = min(per_epoch, steps)
    print(f"{images / dt:.1f} images/s over {span} of {len(ds)} frames; {args.loss} loss "
          f"{s[:per_epoch, 0].mean():.6f} (first epoch) -> {s[-per_epoch:, 0].mean():.6f} (last)")
    print(f"saved {_save_critic(critic, args.save)}")
    if trainer.has_ema():
        print(f"saved {_save_critic(critic, os.path.join(args.save, EMA_DIR), ema=trainer)}")
    _save_trace(args, trainer)
    _print_guard(trainer)
    return critic


def _eval_critic(args):
    """-critic --eval-only: the checkpoint --critic on every frame of the trajectories, against discounted_targets."""
    from .critic_train import MAX_BATCH, CriticTrainer
    critic, ds, _ = _critic_and_dataset(args, None)
    result = CriticTrainer(critic, loss=args.loss).evaluate(ds, min(max(args.batch, 1), MAX_BATCH))
    print({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in result.items()})
    return result


def _build_recon_dataset(args):
    """-dataset (vae.py:130-140): load_networks -> curate_recon (episodes.py) -> ReconDataset.save."""
    from .episodes import curate_recon, load_episodes
    episodes = load_episodes(args.episodes)
    device = _device()
    vae = load_networks(VariationalAutoencoder(max_batch=max(args.batch, 256), seed=args.seed).to(device), args.networks)
    critic = _load_critic(args.critic, vae.handle, args.seed, device)
    t0 = time.time()
    ds = curate_recon(episodes, critic, vae, collect=args.collect, total_images=args.total_images, device=device)
    torch.cuda.synchronize()
    print(f"built {len(ds)} entries from {ds.stats['encoded']} of {ds.stats['walked']} walked frames in {time.time() - t0:.2f} s")
    ds.save(args.out)
    print(f"saved {args.out}")
    if args.pickle:
        import pickle
        with open(args.pickle, "wb") as f:
            pickle.dump(ds.to_reference_list(), f)
        print(f"saved {args.pickle}")
    return ds


def _train_second(args):
    """-second (vae.py:142-153): a fresh VAE, FusedTrainer.fit_device on the recon dataset, saved as vae2_*.pt."""
    from .episodes import ReconDataset
    device = _device()
    ds = ReconDataset.load(args.dataset, device)
    if len(ds) == 0:
        raise SystemExit("the recon dataset is empty")
    vae = VariationalAutoencoder(max_batch=args.batch, seed=args.seed).to(device)
    return _fit_and_save(args, vae, ds, second=True)


if __name__ == "__main__":
    main()
