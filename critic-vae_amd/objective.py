"""The training objective as data: weights of the MS-SSIM, pixel (MSE) and KLD terms, the MS-SSIM gradient mode and two
step schedules.  The arithmetic is cvae_loss_obj's (include/cvae.h); this module only chooses the four values per step.

    Objective()                                      the reference: MS-SSIM + 0.001 * KLD (vae_nets.py:53-62)
    Objective(msssim_grad="used")                    same loss, gradient over the level terms the product uses: no 0 * NaN
    Objective(mse=1.0, msssim_from=2000)             F.mse_loss alone (vae_nets.py:54) for 2000 steps, then both
    Objective(kld=0.004, kld_warmup=5000)            beta-VAE with a linear warm-up of beta

Host arithmetic only: importable and testable without a GPU.
"""
import math

from . import params as P

MSGRAD = {"reference": 0, "used": 1}      # CVAE_MSGRAD_REFERENCE, CVAE_MSGRAD_USED


def _weight(name, v):
    v = float(v)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError(f"{name} weight {v!r}: every weight must be finite and >= 0")
    return v


def _count(name, v):
    if isinstance(v, bool) or int(v) != v or int(v) < 0:
        raise ValueError(f"{name} {v!r}: a number of optimizer steps >= 0")
    return int(v)


class Objective:
    """total = msssim * MS-SSIM loss + mse * F.mse_loss(recon, x) + kld * KLD, per optimizer step.

    msssim_grad: "reference" = autograd of vae_nets.py:243-247 as the reference runs it, including the 0 * w * x^(w-1) of the
      level terms the product never uses (NaN gradients as soon as ssim_0..3 or cs_4 is negative); "used" = the derivative of
      the terms the product uses (the same loss value).
    kld_warmup N > 0: the KLD weight of step s (0-based) is kld * min(1, (s + 1) / N).
    msssim_from N > 0: the MS-SSIM weight is 0 while s < N — such steps run no pyramid at all, so mse must then be > 0.
    Validation matches cvae_loss_obj: every weight finite and >= 0, and a reconstruction term at every step."""

    def __init__(self, msssim=1.0, mse=0.0, kld=P.kld_weight, msssim_grad="reference", kld_warmup=0, msssim_from=0):
        self.msssim, self.mse, self.kld = _weight("msssim", msssim), _weight("mse", mse), _weight("kld", kld)
        if msssim_grad not in MSGRAD:
            raise ValueError(f"msssim_grad {msssim_grad!r}: 'reference' or 'used'")
        self.msssim_grad = msssim_grad
        self.kld_warmup, self.msssim_from = _count("kld_warmup", kld_warmup), _count("msssim_from", msssim_from)
        if not self.msssim + self.mse > 0.0:
            raise ValueError("msssim + mse must be > 0: the objective has no reconstruction term")
        if self.msssim_from > 0 and not self.mse > 0.0:
            raise ValueError(f"msssim_from={self.msssim_from} leaves the first steps without a reconstruction term: mse must be > 0")

    def at(self, step):
        """(msssim_weight, mse_weight, kld_weight, msssim_grad) of optimizer step `step` (0-based: the trainer's step_count
        before the step) — what Handle.loss_obj takes."""
        step = int(step)
        if step < 0:
            raise ValueError(f"step {step}: >= 0")
        kld = self.kld * min(1.0, (step + 1) / self.kld_warmup) if self.kld_warmup > 0 else self.kld
        ms = 0.0 if step < self.msssim_from else self.msssim
        return ms, self.mse, kld, MSGRAD[self.msssim_grad]

    def final(self):
        """The four values once every schedule has run out."""
        return self.msssim, self.mse, self.kld, MSGRAD[self.msssim_grad]

    def state_dict(self):
        return {"msssim": self.msssim, "mse": self.mse, "kld": self.kld, "msssim_grad": self.msssim_grad,
                "kld_warmup": self.kld_warmup, "msssim_from": self.msssim_from}

    def load_state_dict(self, state):
        fresh = Objective(**{k: state[k] for k in ("msssim", "mse", "kld", "msssim_grad", "kld_warmup", "msssim_from")})
        self.__dict__.update(fresh.__dict__)
        return self

    def __eq__(self, other):
        return isinstance(other, Objective) and self.state_dict() == other.state_dict()

    def __repr__(self):
        return "Objective(" + ", ".join(f"{k}={v!r}" for k, v in self.state_dict().items()) + ")"

    def describe(self):
        """One line for a log."""
        s = f"objective: {self.msssim:g} * MS-SSIM ({self.msssim_grad} gradient) + {self.mse:g} * MSE + {self.kld:g} * KLD"
        if self.kld_warmup:
            s += f", KLD weight warmed up over {self.kld_warmup} steps"
        if self.msssim_from:
            s += f", MS-SSIM from step {self.msssim_from}"
        return s


def compose(objective, result):
    """The objective's value on an evaluate() result (train.FusedTrainer.evaluate), with objective.final() so that values
    from different steps of a warm-up compare:
        msssim * recon_loss (pooled)  +  mse * mean_mse  +  kld * raw pooled KLD mean
    A term whose weight is 0 is omitted, not multiplied: a NaN pooled MS-SSIM does not reach a pure-MSE objective.
    result["KLD"] is 0.001 * the raw mean (the record's -0.5 * rec[10] / rec[11]); result["kld_raw"] carries the raw one when
    evaluate() provides it.  mean_mse is the record's mean over the FINITE images only (result["finite_images"])."""
    ms, mse, kld, _ = objective.final()
    raw = result["kld_raw"] if "kld_raw" in result else result["KLD"] / P.kld_weight
    total = 0.0
    if ms != 0.0:
        total += ms * result["recon_loss"]
    if mse != 0.0:
        total += mse * result["mean_mse"]
    if kld != 0.0:
        total += kld * raw
    return float(total)
