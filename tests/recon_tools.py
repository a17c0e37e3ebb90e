"""Shared by tests/golden/make_recon_golden.py and the recon tests: the generator-defined first VAE of recon_real.npz
(synth.make_params(wseed) plus non-trivial BatchNorm running statistics) and the fixture's fixed sample of a reconstruction."""
import numpy as np

from critic_vae_amd import layout as L
from critic_vae_amd import params as P
from critic_vae_amd import synth

SAMPLE_STRIDE = 97            # every 97th of the 12 288 values of a (3, 64, 64) reconstruction: 127 samples


def first_vae_params(wseed):
    """Reference-keyed parameters of the first VAE, with running statistics away from (0, 1): per channel a mean of
    magnitude 0.05..0.3 with a generator-drawn sign, and a variance in 0.4..0.8 or 1.3..2.5."""
    ref = synth.make_params(wseed)
    for l, ci in enumerate(L.ENC_CONV):
        c = P.dims[l]
        mag = synth.uniform(wseed, f"recon/bn_mean/{l}", (c,), 0.05, 0.3)
        sign = np.where(synth.uniform(wseed, f"recon/bn_sign/{l}", (c,)) < 0.5, -1.0, 1.0).astype(np.float32)
        lo = synth.uniform(wseed, f"recon/bn_var_lo/{l}", (c,), 0.4, 0.8)
        hi = synth.uniform(wseed, f"recon/bn_var_hi/{l}", (c,), 1.3, 2.5)
        pick = synth.uniform(wseed, f"recon/bn_var_pick/{l}", (c,)) < 0.5
        ref[f"encoder.model.{ci + 1}.running_mean"] = (mag * sign).astype(np.float32)
        ref[f"encoder.model.{ci + 1}.running_var"] = np.where(pick, lo, hi).astype(np.float32)
    return ref


def sample_of(recon):
    """(strided sample, sum (float64), min, max) of one reconstruction (any shape holding 3 * 64 * 64 values)."""
    a = np.asarray(recon, np.float32).reshape(-1)
    return a[::SAMPLE_STRIDE].copy(), float(a.astype(np.float64).sum()), float(a.min()), float(a.max())
