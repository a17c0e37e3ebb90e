"""Augmentation of a training batch as data: a horizontal flip, a shift by whole pixels with edge replication and a
brightness gain, drawn per sample from a counter-based hash and applied INSIDE the batch gather launch
(cvae_preprocess_u8_gather_aug / cvae_gather_f32_aug, include/cvae.h).  This module chooses the five values of a
cvae_augment per step and states on the host, in numpy, what the kernels draw and write.

    Augment(flip=0.5, shift=2, brightness=0.1, seed=0)      # FusedTrainer(vae, augment=...), CriticTrainer(critic, augment=...)

The definition (one for kernel, host statement and tests), with mix64 = synth._mix64:

    key(seed, draw) = mix64((seed * 0x100000001B3 + draw) mod 2^64)             draw = the trainer's step_count at the gather
    r(s)            = mix64(key ^ mix64(uint64(s)))                             s = the sample's dataset index
    flip            = (r >> 40) < flip_below,          flip_below = round(flip * 2^24)
    k               = ((r >> 24) & 0xFFFF) - 32768,    num = 2^31 + gain_q16 * k,  gain_q16 = round(brightness * 65536)
    g               = float32(num) * 2^-31             (round to nearest, then an exact scaling): within 1 +- brightness
    dx, dy          = ((r >> 12) & 0xFFF) % (2 S + 1) - S,  (r & 0xFFF) % (2 S + 1) - S,   S = shift

Output pixel (i, j) of every channel is source pixel (clamp(i - dy), clamp(jj - dx)), jj = W-1-j if flip else j.  uint8
frames: min(v * g, 1) in fp32 with v = u8 / 255 as the plain gather writes it; fp32 entries: a bit copy, no gain.  The
critic value (or the critic's target) of a sample stays the stored one: the transforms are taken to preserve it.

Under data parallelism every rank derives the same key (same seed, same step_count) and hashes its OWN dataset indices;
no collective is involved.

Host arithmetic only: importable and testable without a GPU.
"""
import numpy as np

from . import synth

FLIP_ONE = 1 << 24           # flip_below of "always"
GAIN_ONE = 1 << 16           # gain_q16 is below this
_MASK64 = (1 << 64) - 1
_FIELDS = ("flip", "shift", "brightness", "seed")


def key(seed, draw):
    """The 64-bit key of one gather, a Python int."""
    return int(synth._mix64(np.uint64((int(seed) * 0x100000001B3 + int(draw)) & _MASK64)))


class Augment:
    """flip: probability of a horizontal flip, 0..1.  shift: S >= 0, dx and dy uniform over [-S, S] (at most width / 4; the
    width is checked where the augmentation is used).  brightness: b in [0, 1), the gain is uniform within 1 +- b (uint8
    frames only).  seed: any integer.  Augment() transforms nothing: the augmented gather then writes the plain gather's bits."""

    def __init__(self, flip=0.0, shift=0, brightness=0.0, seed=0):
        flip, brightness = float(flip), float(brightness)
        if not 0.0 <= flip <= 1.0:
            raise ValueError(f"flip {flip!r}: a probability in [0, 1]")
        if isinstance(shift, bool) or int(shift) != shift or int(shift) < 0:
            raise ValueError(f"shift {shift!r}: a whole number of pixels >= 0")
        if not 0.0 <= brightness < 1.0:
            raise ValueError(f"brightness {brightness!r}: in [0, 1)")
        if isinstance(seed, bool) or int(seed) != seed:
            raise ValueError(f"seed {seed!r}: an integer")
        self.flip, self.shift, self.brightness, self.seed = flip, int(shift), brightness, int(seed)
        self.flip_below = int(round(flip * FLIP_ONE))
        self.gain_q16 = min(int(round(brightness * GAIN_ONE)), GAIN_ONE - 1)

    def check_width(self, width):
        if self.shift > int(width) // 4:
            raise ValueError(f"augment shift {self.shift} above width / 4 = {int(width) // 4} of {width}x{width} frames")
        return self

    def at(self, draw):
        """(key, flip_below, max_shift, gain_q16) of gather number `draw` (the trainer's step_count before the step) — what
        Handle.preprocess_u8_gather_aug / gather_f32_aug take."""
        draw = int(draw)
        if draw < 0:
            raise ValueError(f"draw {draw}: >= 0")
        return key(self.seed, draw), self.flip_below, self.shift, self.gain_q16

    def draws(self, draw, idx):
        """(n, 4) int64 rows [flip, dx, dy, num - 2^31] for the dataset indices `idx`: what the kernels record in `applied`."""
        k, flip_below, S, gain = self.at(draw)
        s = np.asarray(idx, np.int64).reshape(-1).astype(np.uint64)
        r = synth._mix64(np.uint64(k) ^ synth._mix64(s))
        span = np.uint64(2 * S + 1)
        out = np.empty((s.size, 4), np.int64)
        out[:, 0] = (r >> np.uint64(40)).astype(np.int64) < flip_below
        out[:, 1] = (((r >> np.uint64(12)) & np.uint64(0xFFF)) % span).astype(np.int64) - S
        out[:, 2] = ((r & np.uint64(0xFFF)) % span).astype(np.int64) - S
        out[:, 3] = gain * (((r >> np.uint64(24)) & np.uint64(0xFFFF)).astype(np.int64) - 32768)
        return out

    @staticmethod
    def gains(draws):
        """The fp32 gain of every row of draws(): float32(num) * 2^-31."""
        num = np.asarray(draws, np.int64).reshape(-1, 4)[:, 3] + (1 << 31)
        return num.astype(np.float32) * np.float32(2.0 ** -31)

    @staticmethod
    def apply_host(frames, draws):
        """The pixel rule in numpy.  frames uint8 (n, W, W, 3) -> fp32 (n, 3, W, W) = min(frame / 255 * g, 1), transformed;
        frames fp32 (n, 3, W, W) -> the transformed copy (a row whose gain is not 1 is refused).  Row b is transformed by
        draws[b]."""
        frames = np.asarray(frames)
        draws = np.asarray(draws, np.int64).reshape(-1, 4)
        if frames.ndim != 4 or frames.shape[0] != draws.shape[0]:
            raise ValueError(f"frames {frames.shape} against {draws.shape[0]} rows of draws")
        if frames.dtype == np.uint8:
            src = (frames.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)
        elif frames.dtype == np.float32:
            if np.any(draws[:, 3] != 0):
                raise ValueError("fp32 entries take no brightness gain")
            src = frames
        else:
            raise ValueError(f"frames of dtype {frames.dtype}: uint8 (n, W, W, 3) or float32 (n, 3, W, W)")
        n, W = src.shape[0], src.shape[2]
        out = np.empty((n, 3, W, W), np.float32)
        ar = np.arange(W)
        g = Augment.gains(draws)
        for b in range(n):
            f, dx, dy = (int(t) for t in draws[b, :3])
            rows = np.clip(ar - dy, 0, W - 1)
            cols = np.clip((W - 1 - ar if f else ar) - dx, 0, W - 1)
            t = src[b][:, rows][:, :, cols]
            out[b] = np.minimum(t * g[b], np.float32(1.0)) if frames.dtype == np.uint8 else t
        return out

    def state_dict(self):
        return {k: getattr(self, k) for k in _FIELDS}

    @classmethod
    def from_state_dict(cls, state):
        return cls(**{k: state[k] for k in _FIELDS})

    def __eq__(self, other):
        return isinstance(other, Augment) and self.state_dict() == other.state_dict()

    def __repr__(self):
        return "Augment(" + ", ".join(f"{k}={v!r}" for k, v in self.state_dict().items()) + ")"

    def describe(self):
        """One line for a log."""
        return (f"augment: flip with p = {self.flip:g}, shift within +-{self.shift} px (edges replicated), "
                f"brightness gain within 1 +- {self.brightness:g}, seed {self.seed}; critic values are the stored ones")
