// objective.hip — the pixel term of the configurable objective (cvae_loss_obj): F.mse_loss(recon, x), the reference's own
// commented-out reconstruction loss (vae_nets.py:54), its gradient, and the last step of the loss scalars.
//
// ONE streaming pass over recon and x with 16-byte loads, persistent over a CU-sized grid:
//   MS = true  (mixed objective, both weights non-zero): msssim_bwd_kernel's chain
//                dx = c0 F0 + 1/4 up(c1 F1 + 1/4 up(c2 F2 + ...))     (coef already carries the MS-SSIM weight: msssim_finish.h)
//              plus the pixel gradient 2 w_mse (recon - x) / N in the same store — d_recon is written once and never read;
//   MS = false (MS-SSIM weight 0): no chain, no F field is touched; the pass also does what the MS-SSIM finalize would have
//              done for the KLD: its fp64 sum, d_mu and d_logvar.
// Differences and squares are fp32, every sum fp64: one partial per workgroup in the finalize's slab (free once the
// finalize has run), merged in a fixed order by the last workgroup to arrive on the finalize's ticket (wg_arrive_last
// leaves it at 0).  No floating-point atomics: the same call gives the same bits.  The merging workgroup writes scalars[13]
// and the final scalars[0] (pure MSE: every scalar).
#include "../../include/cvae.h"
#include "common.h"
#include <math.h>

static constexpr int OBJ_NT = 1024;          // threads per workgroup: 16 waves, one workgroup per CU
static constexpr int OBJ_MAXG = 256;         // workgroups: squared-error partials slab[0, OBJ_MAXG)
static constexpr int OBJ_MAXK = 96;          // of which the first OBJ_MAXK stride over the KLD: slab[OBJ_MAXG, OBJ_MAXG + OBJ_MAXK)
static_assert(OBJ_MAXG + OBJ_MAXK <= MSSSIM_SLAB_DOUBLES, "the partials must fit the finalize's slab");

struct ObjPixArgs {
    const float* r; const float* x;          // recon (carries the gradient), frames
    const float* F[5]; const float* coef;    // MS only
    float* dx;                               // null: values only
    const float* mu; const float* logvar; float* d_mu; float* d_logvar; int B;      // !MS only (B = 0: no KLD)
    int64_t total4;                          // 3 * B * W * W / 4
    double N;                                // 3 * B * W * W
    float gscale;                            // 2 * w_mse / N
    float w_ms, w_mse, kw;
    double* slab; unsigned* ticket; float* scalars;
    int nk;                                  // workgroups that take part in the KLD
};

// the 16 wave sums of a workgroup in a fixed order; valid in thread 0
__device__ __forceinline__ double obj_block_sum(double v, double* red) {
    v = wave_sum_d(v);
    __syncthreads();                         // red may still be read from the previous use
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < OBJ_NT / 64; ++k) t += red[k];
    return t;
}

template <int W, bool MS>
__global__ __launch_bounds__(OBJ_NT) void objective_pixel_kernel(ObjPixArgs a) {
    __shared__ double red[OBJ_NT / 64];
    __shared__ unsigned last_flag;
    constexpr int W4 = W / 4;
    const int tid = threadIdx.x;
    const bool grad = a.dx != nullptr;
    float cf[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (MS && grad)
#pragma unroll
        for (int l = 0; l < 5; ++l) cf[l] = a.coef[l];
    const float gs = a.gscale;
    double s = 0.0;
    const int64_t stride = (int64_t)gridDim.x * OBJ_NT;
#pragma unroll 2
    for (int64_t idx = (int64_t)blockIdx.x * OBJ_NT + tid; idx < a.total4; idx += stride) {
        const f32x4 rv = *reinterpret_cast<const f32x4*>(a.r + idx * 4);
        const f32x4 xv = *reinterpret_cast<const f32x4*>(a.x + idx * 4);
        const f32x4 d = rv - xv;
        const f32x4 d2 = d * d;
        s += ((double)d2[0] + (double)d2[1]) + ((double)d2[2] + (double)d2[3]);
        if (!grad) continue;
        f32x4 o = d * gs;
        if constexpr (MS) {
            const int c = (int)(idx % W4) * 4, r = (int)((idx / W4) % W);
            const int64_t plane = idx / ((int64_t)W4 * W);
            // top level first, exactly the nesting of the avg_pool2d backward chain (msssim_bwd_kernel)
            const float g4 = cf[4] * a.F[4][(plane * (W / 16) + (r >> 4)) * (W / 16) + (c >> 4)];
            const float g3 = cf[3] * a.F[3][(plane * (W / 8) + (r >> 3)) * (W / 8) + (c >> 3)] + 0.25f * g4;
            const float g2 = cf[2] * a.F[2][(plane * (W / 4) + (r >> 2)) * (W / 4) + (c >> 2)] + 0.25f * g3;
            const float2 f1 = *reinterpret_cast<const float2*>(a.F[1] + (plane * (W / 2) + (r >> 1)) * (W / 2) + (c >> 1));
            const float g1a = cf[1] * f1.x + 0.25f * g2, g1b = cf[1] * f1.y + 0.25f * g2;
            const f32x4 f0 = *reinterpret_cast<const f32x4*>(a.F[0] + idx * 4);
            o[0] += cf[0] * f0[0] + 0.25f * g1a; o[1] += cf[0] * f0[1] + 0.25f * g1a;
            o[2] += cf[0] * f0[2] + 0.25f * g1b; o[3] += cf[0] * f0[3] + 0.25f * g1b;
        }
        *reinterpret_cast<f32x4*>(a.dx + idx * 4) = o;
    }
    {
        const double t = obj_block_sum(s, red);
        if (tid == 0) a.slab[blockIdx.x] = t;
    }
    if constexpr (!MS) {
        // uniform per workgroup.  nk = min(grid, OBJ_MAXK) workgroups stride over the B * 32 latent values: a second trip of this
        // loop needs B * 32 > OBJ_MAXK * OBJ_NT, i.e. B > 3072 — above what the tests reach; the pixel loop above, whose
        // stride has the same form, is tested past one trip (tests/test_gpu_objective.py)
        if ((int)blockIdx.x < a.nk) {
            const float invB = a.B > 0 ? 1.0f / (float)a.B : 0.f;
            double k = 0.0;
            for (int i = blockIdx.x * OBJ_NT + tid; i < a.B * 32; i += a.nk * OBJ_NT) {
                const float m = a.mu[i], lv = a.logvar[i], e = expf(lv);
                k += (double)(1.0f + lv - m * m - e);
                if (a.d_mu) { a.d_mu[i] = a.kw * m * invB; a.d_logvar[i] = a.kw * 0.5f * (e - 1.0f) * invB; }
            }
            const double t = obj_block_sum(k, red);
            if (tid == 0) a.slab[OBJ_MAXG + blockIdx.x] = t;
        }
    }
    if (!wg_arrive_last(a.ticket, gridDim.x, &last_flag)) return;
    if (tid >= 64) return;
    double t = 0.0, k = 0.0;
    for (int g = tid; g < (int)gridDim.x; g += 64) t += a.slab[g];
    t = wave_sum_d(t);
    if constexpr (!MS) {
        for (int g = tid; g < a.nk; g += 64) k += a.slab[OBJ_MAXG + g];
        k = wave_sum_d(k);
    }
    const float mse = (float)(t / a.N);
    if constexpr (MS) {
        if (tid == 0) {
            const float rec = a.scalars[1], kld = a.scalars[2];      // the finalize's, a launch boundary behind
            a.scalars[13] = mse;
            a.scalars[0] = (a.w_ms * rec + a.w_mse * mse) + kld;
        }
    } else {
        const float kld = a.B > 0 ? (float)(-0.5 * k / (double)a.B) * a.kw : 0.0f;
        if (tid < CVAE_N_SCALARS) {
            float v = 0.0f;                       // [1], [3..12]: the MS-SSIM term was not computed; [14], [15] reserved
            if (tid == 0) v = a.w_mse * mse + kld;
            else if (tid == 2) v = kld;
            else if (tid == 13) v = mse;
            a.scalars[tid] = v;
        }
    }
}

int launch_objective_pixels(int width, int B, const float* recon, const float* x, const float* const* F, const float* coef,
                            float* dx, const float* mu, const float* logvar, float* d_mu, float* d_logvar,
                            LossObjective obj, double* slab, unsigned* ticket, float* scalars, hipStream_t st) {
    if (width != 64 && width != 128) { cvae_set_error("objective: width %d unsupported", width); return -2; }
    ObjPixArgs a{};
    a.r = recon; a.x = x; a.dx = dx;
    if (F) { for (int l = 0; l < 5; ++l) a.F[l] = F[l]; a.coef = coef; }
    a.mu = mu; a.logvar = logvar; a.d_mu = d_mu; a.d_logvar = d_logvar; a.B = mu ? B : 0;
    a.total4 = (int64_t)B * 3 * width * width / 4;
    a.N = (double)B * 3 * width * width;
    a.gscale = (float)(2.0 * (double)obj.w_mse / a.N);
    a.w_ms = obj.w_ms; a.w_mse = obj.w_mse; a.kw = obj.kw;
    a.slab = slab; a.ticket = ticket; a.scalars = scalars;
    // one workgroup per CU, every thread strides over the frames: B = 2048 is 24 trips, not 6144 workgroups
    int64_t grid = (a.total4 + OBJ_NT - 1) / OBJ_NT;
    const int cus = cvae_num_cus();
    if (grid > cus) grid = cus;
    if (grid > OBJ_MAXG) grid = OBJ_MAXG;
    if (grid < 1) grid = 1;
    a.nk = (int)(grid < OBJ_MAXK ? grid : OBJ_MAXK);
    if (F) {
        if (width == 64) hipLaunchKernelGGL((objective_pixel_kernel<64, true>), dim3((unsigned)grid), dim3(OBJ_NT), 0, st, a);
        else hipLaunchKernelGGL((objective_pixel_kernel<128, true>), dim3((unsigned)grid), dim3(OBJ_NT), 0, st, a);
    } else {
        if (width == 64) hipLaunchKernelGGL((objective_pixel_kernel<64, false>), dim3((unsigned)grid), dim3(OBJ_NT), 0, st, a);
        else hipLaunchKernelGGL((objective_pixel_kernel<128, false>), dim3((unsigned)grid), dim3(OBJ_NT), 0, st, a);
    }
    CVAE_CHECK_LAUNCH();
    return 0;
}
