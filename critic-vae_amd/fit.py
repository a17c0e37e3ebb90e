"""What FusedTrainer (train.py) and CriticTrainer (critic_train.py) share: the guard's setup and counters, the optimizer
launch pair, the validation fields with their part of the trainer state, and the loop of fit_device.  Host Python only;
every launch goes through the subclass's Handle (`h`).

A subclass owns `h`, `lr`, `betas`, `eps`, the flat `grads`, `m`, `v`, `step_count`, its `step()` and its `evaluate()`.
Everything here is a plain attribute of the trainer, so a test can build one with __new__ and set what it needs."""
import numpy as np
import torch

from .augment import Augment
from .optim import Optim
from .trace import Trace


class DeviceTrainer:
    def _init_shared(self, skip_nonfinite, max_grad_norm, optim=None, trace=None):
        if optim is not None and not isinstance(optim, Optim):
            raise ValueError(f"optim {optim!r}: an optim.Optim or None")
        if trace is not None and not isinstance(trace, Trace):
            raise ValueError(f"trace {trace!r}: a trace.Trace or None")
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f"max_grad_norm {max_grad_norm!r}: a positive number (inf = no clipping) or None")
        self.skip_nonfinite = bool(skip_nonfinite)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.guarded = self.skip_nonfinite or self.max_grad_norm is not None
        self.guard = None                 # the device guard state, created by the first guarded step ...
        self._guard_counts = (0, 0)       # ... from these (applied, skipped): what load_state_dict / sync_replicas left
        self.step_count = 0
        self.val_history = []             # (step_count, result of evaluate()) per evaluation that fit_device(val=...) ran
        self.best_val = None              # the lowest finite validation loss seen (the CLI's --keep-best / --patience)
        self.val_stale = 0                # evaluations in a row since it last improved
        self.augment = None               # an augment.Augment: fit_device gathers through the augmented kernels (_init_augment)
        self.optim = optim                # an optim.Optim: _update launches the _opt kernels under optim.args_at(step)
        self.decay_ranges = []            # the element ranges weight decay touches (optim.decay_ranges of the subclass's layout)
        self.ema = None                   # the averaged parameters and the averaged auxiliary buffer (the VAE's bn_state) of an
        self.aux_ema = None               # Optim with an EMA: created by the first such _update, or by load_state_dict
        self.trace = trace                # a trace.Trace: every step ends in its _after_update (one or two more launches, no host read)

    def _init_augment(self, augment, width):
        """The constructor's `augment` argument: None, or an Augment whose shift fits frames of `width`."""
        if augment is not None:
            if not isinstance(augment, Augment):
                raise ValueError(f"augment {augment!r}: an augment.Augment or None")
            augment.check_width(width)
        self.augment = augment

    def _check_augment(self, dataset):
        """Before the first launch of a fit_device: fp32 entries (ReconDataset) take no brightness gain."""
        augment = getattr(self, "augment", None)
        if augment is not None and augment.gain_q16 != 0 and dataset.frames.dtype != torch.uint8:
            raise ValueError(f"{augment!r} on a dataset of fp32 entries: they are Tanh outputs in (-1, 1), a brightness gain "
                             "clamped at 1 has no meaning for them; use brightness=0")

    # ---- the optimizer launches ----
    def _opt_aux(self):
        """The small buffer whose EMA rides in the Adam launch (FusedTrainer: the BatchNorm running statistics); None: none."""
        return None

    def has_ema(self):
        optim = getattr(self, "optim", None)
        return optim is not None and optim.ema is not None

    def _ema_buffers(self, theta):
        """(ema, aux_ema) of a trainer whose Optim has an EMA, created on first use as copies of `theta` and of the auxiliary
        buffer as they stand — unless load_state_dict / sync_replicas supplied them.  So a load_networks after construction is
        safe: nothing was copied at construction."""
        if self.ema is None:
            self.ema = theta.detach().clone()
        aux = self._opt_aux()
        if aux is not None and self.aux_ema is None:
            self.aux_ema = aux.detach().clone()
        return self.ema, self.aux_ema

    def _ema_view(self, theta):
        """(ema, aux_ema) for a READER (evaluate(ema=True), the save paths): the trainer's own buffers where they exist,
        else temporaries — copies of `theta` / the auxiliary buffer that are NOT kept, so that only the first update (or a loaded
        state) ever creates the averages and a load_networks after an early evaluation cannot leave them stale."""
        aux = self._opt_aux()
        ema = self.ema if self.ema is not None else theta.detach().clone()
        aux_ema = self.aux_ema if (self.aux_ema is not None or aux is None) else aux.detach().clone()
        return ema, aux_ema

    def _sync_ema(self, theta, src):
        """sync_replicas with an EMA: rank `src`'s averages reach every rank — or, where it has none yet, every rank drops
        its own, so that all of them start theirs from the (already broadcast) parameters at the next step.  Two or three
        collectives more, only for a trainer whose Optim has an EMA."""
        dist = torch.distributed
        flag = torch.tensor([0 if self.ema is None else 1], dtype=torch.int64, device=self.m.device)
        dist.broadcast(flag, src=src, group=self.pg)
        if int(flag.item()) == 0:
            self.ema, self.aux_ema = None, None
            return
        for t in self._ema_buffers(theta):
            if t is not None:
                dist.broadcast(t, src=src, group=self.pg)

    def _update_opt(self, theta, grad_scale):
        """_update under an Optim: the same launch count, the _opt kernels in place of the plain ones.  The schedule and the EMA
        warm-up count calls of step() (step_count is already this step's 1-based number); the guarded bias correction stays the
        device's count of applied steps."""
        h, optim = self.h, self.optim
        a = optim.args_at(self.step_count - 1, self.lr, self.decay_ranges)
        ema, aux, aux_ema = None, None, None
        if optim.ema is not None:
            ema, aux_ema = self._ema_buffers(theta)
            aux = self._opt_aux()
        if not self.guarded:
            h.adam_step_opt(theta, self.grads, self.m, self.v, self.step_count, a["lr"], self.betas[0], self.betas[1], self.eps,
                            grad_scale=grad_scale, opt=a, ema=ema, aux=aux, aux_ema=aux_ema)
            return a["lr"]
        if self.guard is None:
            self.guard = h.guard_state(self.m.device, *self._guard_counts)
        h.grad_stats(self.grads, self.guard, grad_scale, float("inf") if self.max_grad_norm is None else self.max_grad_norm,
                     self.skip_nonfinite, a["lr"], self.betas[0], self.betas[1])
        h.adam_step_guarded_opt(theta, self.grads, self.m, self.v, self.guard, self.eps, opt=a, ema=ema, aux=aux, aux_ema=aux_ema)
        return a["lr"]

    def _update(self, theta, grad_scale):
        """The optimizer launches of one step (_apply_update), then the trace's hook where the trainer has a trace: the one
        place both trainers and every update path (plain, guarded, _opt; per-rank or global statistics) pass through."""
        lr = self._apply_update(theta, grad_scale)
        trace = getattr(self, "trace", None)               # a trainer assembled by hand (tests) may not carry the field
        if trace is not None:
            trace._after_update(self, theta, grad_scale, lr)

    def _apply_update(self, theta, grad_scale):
        """cvae_adam_step, or the guarded pair: statistics of the reduced gradient -> decision record -> the Adam launch that
        obeys it; nothing comes back to the host.  With an Optim: _update_opt.  Returns the lr the step was given."""
        h = self.h
        if getattr(self, "optim", None) is not None:
            return self._update_opt(theta, grad_scale)
        if not self.guarded:
            h.adam_step(theta, self.grads, self.m, self.v, self.step_count, self.lr, self.betas[0], self.betas[1], self.eps,
                        grad_scale=grad_scale)
            return self.lr
        if self.guard is None:
            self.guard = h.guard_state(self.m.device, *self._guard_counts)
        h.grad_stats(self.grads, self.guard, grad_scale, float("inf") if self.max_grad_norm is None else self.max_grad_norm,
                     self.skip_nonfinite, self.lr, self.betas[0], self.betas[1])
        h.adam_step_guarded(theta, self.grads, self.m, self.v, self.guard, self.eps)
        return self.lr

    def _trace_layout(self):
        """{name: (offset, numel)} of the flat buffers, for the trace's tensor table: the handle's (the VAE); CriticTrainer
        has its own."""
        return self.h.layout

    # ---- the guard's counters ----
    def _guard_read(self):
        """(applied, skipped) of a guarded trainer; one sync once the device state exists."""
        if self.guard is None:
            return self._guard_counts
        rec = self.h.guard_record(self.guard)
        return int(rec.t), int(rec.skipped)

    def _guard_write(self, applied, skipped):
        self._guard_counts = (int(applied), int(skipped))
        if self.guard is not None:
            self.h.guard_init(self.guard, *self._guard_counts)

    def guard_stats(self):
        """dict(applied, skipped, norm, coef) of a guarded trainer: the two counters, and the global gradient norm (after
        grad_scale) and clip coefficient of the LAST step — norm 0 and coef 1, what cvae_guard_init writes, before the first step
        and right after a load_state_dict / sync_replicas.  One device -> host copy, i.e. one sync; the trainer itself never calls it."""
        if not self.guarded:
            raise RuntimeError("guard_stats(): this trainer has no guard (skip_nonfinite / max_grad_norm)")
        if self.guard is None:
            return dict(applied=self._guard_counts[0], skipped=self._guard_counts[1], norm=0.0, coef=1.0)
        rec = self.h.guard_record(self.guard)
        return dict(applied=int(rec.t), skipped=int(rec.skipped), norm=float(rec.norm64), coef=float(rec.coef))

    # ---- the shared part of state_dict / load_state_dict ----
    def _shared_state(self):
        """step_count, the applied / skipped counters (an unguarded trainer applied every step) and the validation fields; a
        result in val_history is saved with its arrays as nested lists and without its device rows (per_image / per_frame)."""
        applied, skipped = self._guard_read() if self.guarded else (self.step_count, 0)
        history = [(int(t), {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in r.items() if k not in ("per_image", "per_frame")})
                   for t, r in self.val_history]
        state = {"step_count": int(self.step_count), "applied": applied, "skipped": skipped, "val_history": history,
                 "best_val": self.best_val, "val_stale": int(self.val_stale)}
        if getattr(self, "augment", None) is not None:      # absent without one; draw = step_count: a resumed run continues exactly
            state["augment"] = self.augment.state_dict()
        if getattr(self, "optim", None) is not None:        # absent without one; the EMA tensors once they exist
            state["optim"] = self.optim.state_dict()
            for key in ("ema", "aux_ema"):
                if getattr(self, key) is not None:
                    state[key] = getattr(self, key).detach().cpu().clone()
        return state

    def _load_shared_state(self, state):
        """The counterpart; raises before it changes anything."""
        applied, skipped, steps = int(state["applied"]), int(state["skipped"]), int(state["step_count"])
        saved = state.get("augment")
        restored = None if saved is None else Augment.from_state_dict(saved).check_width(self.h.width)
        saved_optim = state.get("optim")
        optim = None if saved_optim is None else Optim.from_state_dict(saved_optim)
        ema, aux_ema = (state.get("ema"), state.get("aux_ema")) if optim is not None else (None, None)
        if ema is not None and ema.numel() != self.m.numel():
            raise ValueError(f"the state's averaged weights hold {ema.numel()} floats, this trainer has {self.m.numel()}")
        aux = self._opt_aux()
        if aux_ema is not None and (aux is None or aux_ema.numel() != aux.numel()):
            raise ValueError(f"the state's averaged auxiliary buffer holds {aux_ema.numel()} floats, this trainer's "
                             f"{0 if aux is None else aux.numel()}")
        if not self.guarded and applied != steps:
            raise ValueError(f"the state skipped {skipped} of {steps} steps: an unguarded trainer corrects Adam's bias by step_count "
                             "and cannot continue it; construct the trainer with skip_nonfinite=True")
        self.step_count = steps
        self.val_history = [(int(t), dict(r)) for t, r in state.get("val_history", [])]      # absent in states written before validation existed
        self.best_val = state.get("best_val")
        self.val_stale = int(state.get("val_stale", 0))
        if restored is not None:           # a state without one keeps what the trainer was built with
            self.augment = restored
        if optim is not None:              # likewise; averaged tensors the state does not carry are created by the next _update
            self.optim = optim
            self.ema = None if ema is None else ema.to(device=self.m.device, dtype=torch.float32).clone()
            self.aux_ema = None if aux_ema is None else aux_ema.to(device=self.m.device, dtype=torch.float32).clone()
        if self.guarded:
            self._guard_write(applied, skipped)

    # ---- the loop of fit_device ----
    def _validate(self, val, batch_size, on_val):
        """One evaluation inside fit_device: history entry, callback; True = the callback asked to stop.  A trainer with an
        Optim evaluates its averaged weights when it keeps an EMA, and its result says which weights were judged: "weights":
        "ema" or "live".  A trainer WITHOUT an Optim gets the call and the result dict it always got — no "weights" key — so
        that results and saved histories of runs without the option stay what they were."""
        if getattr(self, "optim", None) is None:
            result = self.evaluate(val, batch_size)
        else:                              # the averaged weights are what gets shipped: they are the ones judged
            result = self.evaluate(val, batch_size, ema=True) if self.has_ema() else self.evaluate(val, batch_size)
            result["weights"] = "ema" if self.has_ema() else "live"
        self.val_history.append((int(self.step_count), result))
        return bool(on_val(self, result)) if on_val is not None else False

    def _fit(self, dataset, B, epochs, shuffle, x, pred, batch, val=None, val_every=None, on_val=None, val_batch=None):
        """Per epoch np.random.shuffle of the host indices (one draw; uploaded once), slices of B with the ragged last one kept;
        per slice one dataset.gather launch into x / pred and batch(x[:nb], pred[:nb]), which takes the step.  val is evaluated
        (at val_batch) after every val_every steps, or at the end of every epoch; a true return value of on_val ends the fit.
        With self.augment the gather is the augmented one under augment.at(step_count) (the step the batch is for); without,
        gather is called with the five positional arguments it always had.  Returns what the last batch() returned, None if
        none ran."""
        self._check_augment(dataset)
        augment = getattr(self, "augment", None)           # a trainer assembled by hand (tests) may not carry the field
        if val is not None:
            if val_every is not None and int(val_every) < 1:
                raise ValueError(f"val_every {val_every!r}: a positive number of optimizer steps, or None for once per epoch")
        elif val_every is not None or on_val is not None:
            raise ValueError("val_every / on_val need val, the held-out dataset")
        n, dev, last = len(dataset), self.m.device, None
        for _ in range(epochs):
            idx = np.arange(n)
            if shuffle:
                np.random.shuffle(idx)
            d_idx = torch.from_numpy(idx).to(dev)          # indices of arange(n): in [0, n) by construction
            for b in range(0, n, B):
                nb = min(B, n - b)
                if augment is None:
                    dataset.gather(self.h, nb, d_idx[b:b + nb], x[:nb], pred[:nb])
                else:
                    dataset.gather(self.h, nb, d_idx[b:b + nb], x[:nb], pred[:nb], aug=augment.at(self.step_count))
                last = batch(x[:nb], pred[:nb])
                if val is not None and val_every is not None and self.step_count % int(val_every) == 0 \
                        and self._validate(val, val_batch, on_val):
                    return last
            if val is not None and val_every is None and self._validate(val, val_batch, on_val):
                return last
        return last
