// msssim_finish.h — the scalar end of the MS-SSIM + KLD loss: from the 11 fp64 sums to the loss scalars and the per-level
// gradient coefficients.  One definition for every kernel that finishes a loss: the batch finalize and the cross-rank finish
// (msssim.hip) and the per-image scores (score.hip), so that an image scored alone is
// finished by the code that finishes a batch of one (each file compiles its own copy: results agree to 1e-6, contraction may differ).
#pragma once
#include "common.h"
#include <math.h>

// lanes 0-4: ssim_l, lanes 5-9: cs_l, lane 10: KLD sum — every lane finishes its own scalar from its fp64 sum t
// (same operations and order as a serial evaluation), shuffles bring them together.  cnt: this lane's level count
// B*3*S_l*S_l; Bd: the image count of the KLD mean.  Called by lanes 0..63 of one wave.
// The objective (cvae_loss_obj): kw is the KLD weight, w_ms the weight of the MS-SSIM term — scalars[1] stays the unweighted
// 1 - prod, scalars[0] = w_ms * [1] + [2] and w_ms is folded into coef, so the backward chain needs no second multiply —
// and `used` selects the gradient over the terms the product uses (no poison term below).  The reference objective is
// (MS_REF_KW, false, 1.0f): an fp32 multiply by 1.0f is exact (also inside a contracted fma), so every caller that passes it
// computes the bits it computed before these were arguments.
constexpr float MS_REF_KW = 0.001f;          // vae_parameters.py:17
__device__ __forceinline__ void ms_finish_scalars(int lane, double t, double cnt, double Bd, float* scalars, float* coef,
                                                  float kw, bool used, float w_ms) {
    const int l = lane % 5;
    const float wts[5] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};
    const float meanf = (float)(t / cnt);
    const float pw = powf(meanf, wts[l]);
    const float p2 = __shfl(pw, 4, 64);
    float out = 1.0f;
    for (int q = 0; q < 4; ++q) out *= __shfl(pw, 5 + q, 64) * p2;              // vae_nets.py:243-246
    const float recon = 1.0f - out;
    const double k = __shfl(t, 10, 64);
    const float kld = Bd > 0 ? (float)(-0.5 * k / Bd) * kw : 0.0f;
    if (lane == 0) { scalars[0] = w_ms * recon + kld; scalars[1] = recon; scalars[2] = kld; }
    if (lane < 5) scalars[3 + lane] = meanf;
    else if (lane < 10) scalars[8 + l] = meanf;
    else if (lane < 13) scalars[13 + lane - 10] = 0.f;
    // autograd of the reference also differentiates the terms `prod(pow1[:-1] * pow2[-1])` never uses — mssim ** weights and
    // mcs ** weights are evaluated for all five levels (vae_nets.py:243-244) — with an incoming gradient of exactly 0:
    // 0 * w * x^(w-1), which is 0 for x > 0 but NaN for x < 0 (fractional power) and for x == 0 (0 * inf).  A negative
    // ssim level 0..3 (dark real frames against an untrained decoder) or cs level 4 therefore turns EVERY gradient that passes
    // through recon into NaN while the loss itself stays finite (tests/golden/step_real_b68.npz, "seed0/").  Same arithmetic
    // here: the poison term is added to the level's coefficient.
    const float poison = 0.0f * (wts[l] * powf(meanf, wts[l] - 1.0f));          // lanes 0-4: ssim_l, lanes 5-9: cs_l
    const float p_ssim = __shfl(poison, l, 64), p_cs4 = __shfl(poison, 9, 64);
    // `used`: the derivative of prod(cs_0..3 ^ w) * ssim_4 ^ (4 w_4) alone — same value, and a negative UNUSED level mean no
    // longer reaches the gradient (a negative used one still gives NaN, as in the reference)
    if (lane >= 5 && lane < 9) {
        const float c = (float)((double)(-out * wts[l] / meanf) / cnt);
        coef[l] = w_ms * (used ? c : c + p_ssim);
    }
    if (lane == 4) {
        const float c = (float)((double)(-out * 4.0f * wts[4] / meanf) / cnt);
        coef[4] = w_ms * (used ? c : c + p_cs4);
    }
}
