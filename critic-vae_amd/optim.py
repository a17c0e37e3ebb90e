"""The optimizer's options as data: a learning-rate schedule, decoupled weight decay (torch.optim.AdamW) and an exponential
moving average of the weights.  The arithmetic is cvae_adam_step_opt's / cvae_adam_step_guarded_opt's (include/cvae.h), inside
the one launch of the Adam pass; this module only chooses the values of a step.

    Optim()                                                  torch.optim.Adam(lr): what the trainers do without one
    Optim(schedule="cosine", warmup=500, total=20000)        linear warm-up to lr, then a half cosine down to lr_min
    Optim(weight_decay=0.01)                                 AdamW on the weight tensors (no bias, no BatchNorm gamma / beta)
    Optim(ema=0.999, ema_warmup=True)                        averaged weights (and BatchNorm statistics) beside the live ones

Host arithmetic only: importable and testable without a GPU.
"""
import ctypes
import math

SCHEDULES = ("constant", "linear", "cosine")
MAX_RANGES = 16           # CVAE_OPT_MAX_RANGES


def _count(name, v):
    if isinstance(v, bool) or int(v) != v or int(v) < 0:
        raise ValueError(f"{name} {v!r}: a number of optimizer steps >= 0")
    return int(v)


def _f32(v):
    return ctypes.c_float(v).value


class Optim:
    """lr, weight decay and EMA rate per optimizer step (0-based, counted in calls of the trainer's step()).

    schedule / warmup / total / lr_min: the learning rate of step s under the trainer's `lr` as the peak is
      lr * (s + 1) / warmup while s < warmup; then lr ("constant"), or a straight line ("linear") or a half cosine ("cosine")
      from lr at s = warmup to lr_min at s = total; lr_min from total on.  The two decaying schedules need total > warmup.
    weight_decay W >= 0: AdamW's decoupled form, p *= 1 - lr_s * W before the Adam update, on the ranges of decay_ranges().
    ema D in [0, 1): e += (1 - D_s) * (p_new - e) after every applied update; with ema_warmup D_s = min(D, (1 + s) / (10 + s))
      (TensorFlow's num_updates rule), so the average forgets its starting point quickly."""

    def __init__(self, schedule="constant", warmup=0, total=None, lr_min=0.0, weight_decay=0.0, ema=None, ema_warmup=False):
        if schedule not in SCHEDULES:
            raise ValueError(f"schedule {schedule!r}: one of {SCHEDULES}")
        self.schedule = schedule
        self.warmup = _count("warmup", warmup)
        self.total = None if total is None else _count("total", total)
        if schedule != "constant" and (self.total is None or self.total <= self.warmup):
            raise ValueError(f"total {total!r}: the {schedule} schedule needs a number of steps above warmup = {self.warmup}")
        if self.total is not None and self.total < self.warmup:
            raise ValueError(f"total {total!r} below warmup = {self.warmup}")
        self.lr_min = float(lr_min)
        if not math.isfinite(self.lr_min) or self.lr_min < 0.0:
            raise ValueError(f"lr_min {lr_min!r}: finite and >= 0")
        self.weight_decay = float(weight_decay)
        if not math.isfinite(self.weight_decay) or self.weight_decay < 0.0:
            raise ValueError(f"weight_decay {weight_decay!r}: finite and >= 0")
        self.ema = None if ema is None else float(ema)
        if self.ema is not None and not 0.0 <= self.ema < 1.0:
            raise ValueError(f"ema {ema!r}: a decay in [0, 1), or None")
        if not isinstance(ema_warmup, (bool, int)) or ema_warmup not in (0, 1):
            raise ValueError(f"ema_warmup {ema_warmup!r}: True or False")
        self.ema_warmup = bool(ema_warmup)
        if self.ema_warmup and self.ema is None:
            raise ValueError("ema_warmup=True without ema: there is no average to warm up")

    @staticmethod
    def _step(step):
        if isinstance(step, bool) or int(step) != step or int(step) < 0:
            raise ValueError(f"step {step!r}: >= 0")
        return int(step)

    def check_lr(self, lr):
        """Raises ValueError when a decaying schedule would end above its peak `lr`; returns self."""
        if self.schedule != "constant" and self.lr_min > lr:
            raise ValueError(f"lr_min {self.lr_min!r} above the peak lr {lr!r}: the {self.schedule} schedule decays from lr to lr_min")
        return self

    def lr_at(self, step, lr):
        """The learning rate of optimizer step `step` (0-based: the trainer's step_count before the step), `lr` the peak."""
        step = self._step(step)
        if step < self.warmup:
            return lr * (step + 1) / self.warmup
        if self.schedule == "constant":
            return lr
        self.check_lr(lr)
        if step >= self.total:
            return self.lr_min
        t = (step - self.warmup) / (self.total - self.warmup)
        if self.schedule == "linear":
            return lr + (self.lr_min - lr) * t
        return self.lr_min + (lr - self.lr_min) * 0.5 * (1 + math.cos(math.pi * (step - self.warmup) / (self.total - self.warmup)))

    def ema_decay_at(self, step):
        """The EMA decay of step `step`; None without an EMA."""
        step = self._step(step)
        if self.ema is None:
            return None
        return min(self.ema, (1 + step) / (10 + step)) if self.ema_warmup else self.ema

    def args_at(self, step, lr, ranges=()):
        """What the Adam launch of step `step` takes: dict(lr, decay_mul, ema_omd, ranges) — lr_at, and the values of
        cvae_opt_args rounded to fp32 as the header defines them.  `ranges`: decay_ranges() of the trainer's layout; dropped
        when weight_decay is 0 (nothing decays, and the launch tests no range)."""
        lr_s = self.lr_at(step, lr)
        decay_mul = _f32(1.0 - float(lr_s) * self.weight_decay)
        if not 0.0 < decay_mul <= 1.0:
            raise ValueError(f"lr {lr_s!r} * weight_decay {self.weight_decay!r}: 1 - their product must lie in (0, 1]")
        d = self.ema_decay_at(step)
        ranges = [(int(b), int(e)) for b, e in ranges] if self.weight_decay > 0.0 else []
        if len(ranges) > MAX_RANGES:
            raise ValueError(f"{len(ranges)} decayed ranges: the launch carries at most {MAX_RANGES}")
        return {"lr": lr_s, "decay_mul": decay_mul, "ema_omd": 0.0 if d is None else _f32(1.0 - d), "ranges": ranges}

    _KEYS = ("schedule", "warmup", "total", "lr_min", "weight_decay", "ema", "ema_warmup")

    def state_dict(self):
        return {k: getattr(self, k) for k in self._KEYS}

    def load_state_dict(self, state):
        fresh = Optim(**{k: state[k] for k in self._KEYS})
        self.__dict__.update(fresh.__dict__)
        return self

    @classmethod
    def from_state_dict(cls, state):
        return cls().load_state_dict(state)

    def __eq__(self, other):
        return isinstance(other, Optim) and self.state_dict() == other.state_dict()

    __hash__ = None

    def __repr__(self):
        return "Optim(" + ", ".join(f"{k}={v!r}" for k, v in self.state_dict().items()) + ")"

    def describe(self):
        """One line for a log."""
        s = f"optimizer: {self.schedule} lr"
        if self.warmup:
            s += f", warmed up over {self.warmup} steps"
        if self.schedule != "constant":
            s += f", down to {self.lr_min:g} at step {self.total}"
        s += f"; weight decay {self.weight_decay:g}" + (" (decoupled, weight tensors only)" if self.weight_decay else "")
        if self.ema is None:
            return s + "; no EMA"
        return s + f"; EMA {self.ema:g}" + (" with warm-up" if self.ema_warmup else "")


def decay_ranges(layout):
    """The element ranges [begin, end) that weight decay touches, sorted, from a layout {name: (offset, numel)}: the weight
    tensors only — names ending in ".w" (the VAE's native layout: enc0..3.w, fc.w, dec0..4.w, decin.w) or ".weight" (the
    critic's state_dict order), one range per tensor.  Biases and BatchNorm gamma / beta are left out."""
    out = sorted((int(off), int(off) + int(n)) for name, (off, n) in layout.items()
                 if (name.endswith(".w") or name.endswith(".weight")) and int(n) > 0)
    for (_, e), (b, _) in zip(out, out[1:]):
        if b < e:
            raise ValueError(f"the layout's tensors overlap at element {b}")
    return out


def critic_layout():
    """{name: (offset, numel)} of the critic's flat block: the reference's state_dict order (critic.CRITIC_KEYS)."""
    from .critic import CRITIC_KEYS
    layout, off = {}, 0
    for name, shape in CRITIC_KEYS:
        n = math.prod(shape)
        layout[name] = (off, n)
        off += n
    return layout
