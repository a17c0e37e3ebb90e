// score.hip — per-image scores of a batch and the pooled record of a whole set (cvae_score, include/cvae.h).
//
// The values-only MS-SSIM pyramid (msssim.hip, no derivative passes) leaves one (ssim, cs) partial pair per plane and
// level; its record-mode finalize leaves the batch's 11 fp64 sums.  score_image_kernel turns the partials into one row
// per image: one workgroup per image streams the image's x and recon once (mean squared error, max |recon - x|), sums
// the image's three plane partials per level and its KLD terms in fp64, and finishes them with ms_finish_scalars as a
// batch of one — the code cvae_loss runs at batch 1 (compiled here a second time: equal to 1e-6, not promised bit for bit).  The last workgroup to arrive then adds the batch to
// the pooled record: rows in a fixed thread-strided order, no floating-point atomics, the same inputs give the same bits.
#include "common.h"
#include "msssim_finish.h"
#include "../../include/cvae.h"
#include <math.h>

// the pooled record (include/cvae.h, cvae_score_state): CVAE_SCORE_STATE_DOUBLES doubles
static constexpr int SC_SUMS = 0, SC_IMAGES = 11, SC_FINITE = 12 /* then the sums of [0..3] */, SC_MAX = 17, SC_COEF = 18, SC_TICKET = 22;
static_assert(CVAE_SCORE_STATE_DOUBLES == 24 && CVAE_SCORE_COLS == 8, "record layout of include/cvae.h");

struct ScoreArgs {
    const float* x; const float* recon;      // (B, 3, W, W)
    const float* mu; const float* logvar;    // (B, 32)
    const float* part[5];                    // level l: (ssim, cs) pairs of planes 3 i .. 3 i + 2
    float* rows;                             // (B, CVAE_SCORE_COLS)
    const double* rec;                       // the batch's 11 sums (msssim_finalize_kernel<true>)
    double* state;                           // pooled record or null
    int B;
};

__global__ __launch_bounds__(64) void score_init_kernel(double* state) {
    const int i = threadIdx.x;
    if (i < CVAE_SCORE_STATE_DOUBLES) state[i] = i == SC_MAX ? (double)-INFINITY : 0.0;      // an all-zero double is ticket 0 too
}

template <int W>
__global__ __launch_bounds__(256) void score_image_kernel(ScoreArgs a) {
    constexpr int N = 3 * W * W, N4 = N / 4;
    __shared__ double red_s[4];
    __shared__ float red_m[4];
    __shared__ float sc[CVAE_N_SCALARS], cf[8];
    __shared__ double red_b[6][4];
    __shared__ unsigned last_flag;
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // ---- one pass over the image: differences and squares in fp32, sums in fp64 ----
    const f32x4* px = reinterpret_cast<const f32x4*>(a.x + (size_t)img * N);
    const f32x4* pr = reinterpret_cast<const f32x4*>(a.recon + (size_t)img * N);
    double s = 0.0;
    float mx = 0.f;
    bool bad = false;                        // a NaN difference: fmaxf would drop it
#pragma unroll 4
    for (int q = tid; q < N4; q += 256) {
        const f32x4 d = pr[q] - px[q];
        const f32x4 d2 = d * d;
        s += ((double)d2[0] + (double)d2[1]) + ((double)d2[2] + (double)d2[3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) { mx = fmaxf(mx, fabsf(d[e])); bad |= d[e] != d[e]; }
    }
    if (bad) mx = NAN;
    s = wave_sum_d(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float v = __shfl_xor(mx, o, 64); mx = (mx != mx || v != v) ? NAN : fmaxf(mx, v); }
    if (lane == 0) { red_s[wv] = s; red_m[wv] = mx; }
    // ---- wave 0: the image's 11 sums in the finalize's order (three plane partials per level, 32 KLD terms), then the
    //      finish of a batch of one ----
    if (wv == 0) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 10; ++q) {
            double v = lane < 3 ? (double)a.part[q % 5][((size_t)img * 3 + lane) * 2 + q / 5] : 0.0;
            v = wave_sum_d(v);
            if (lane == q) t = v;
        }
        double k = 0.0;
        if (lane < 32) {
            const float m = a.mu[(size_t)img * 32 + lane], lv = a.logvar[(size_t)img * 32 + lane], e = expf(lv);
            k = (double)(1.0f + lv - m * m - e);
        }
        k = wave_sum_d(k);
        if (lane == 10) t = k;
        const int S = W >> (lane % 5);
        ms_finish_scalars(lane, t, 3.0 * S * S, 1.0, sc, cf, MS_REF_KW, false, 1.0f);
    }
    __syncthreads();
    if (tid == 0) {
        const double ss = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
        float m = red_m[0];
        for (int k = 1; k < 4; ++k) m = (m != m || red_m[k] != red_m[k]) ? NAN : fmaxf(m, red_m[k]);
        float* row = a.rows + (size_t)img * CVAE_SCORE_COLS;
        row[0] = __fadd_rn(sc[1], sc[2]); row[1] = sc[1]; row[2] = sc[2];      // exactly the fp32 sum (sc[0] may be a contracted 1 - prod + kld)
        row[3] = (float)(ss / (double)N); row[4] = m;
        row[5] = sc[3]; row[6] = sc[7]; row[7] = 0.f;
    }
    if (!a.state) return;
    // ---- the batch into the pooled record: the last workgroup to arrive, rows in thread-strided order ----
    if (!wg_arrive_last(reinterpret_cast<unsigned*>(a.state + SC_TICKET), (unsigned)a.B, &last_flag)) return;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};      // finite images, sums of [0..3] over them
    double bmax = (double)-INFINITY;
    for (int i = tid; i < a.B; i += 256) {
        const float* row = a.rows + (size_t)i * CVAE_SCORE_COLS;
        const float r0 = row[0];
        if (!(fabsf(r0) <= 3.402823466e38f)) continue;      // NaN or Inf total: counted in images only
        acc[0] += 1.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[1 + c] += (double)row[c];
        bmax = fmax(bmax, (double)r0);
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) { const double v = wave_sum_d(acc[c]); if (lane == 0) red_b[c][wv] = v; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bmax = fmax(bmax, __shfl_xor(bmax, o, 64));
    if (lane == 0) red_b[5][wv] = bmax;
    __syncthreads();
    if (tid < 11) a.state[SC_SUMS + tid] += a.rec[tid];
    else if (tid == 11) a.state[SC_IMAGES] += (double)a.B;
    else if (tid < 17) { const int c = tid - 12; a.state[SC_FINITE + c] += (red_b[c][0] + red_b[c][1]) + (red_b[c][2] + red_b[c][3]); }
    else if (tid == 17) a.state[SC_MAX] = fmax(a.state[SC_MAX], fmax(fmax(red_b[5][0], red_b[5][1]), fmax(red_b[5][2], red_b[5][3])));
}

int64_t score_state_bytes() { return CVAE_SCORE_STATE_DOUBLES * 8; }

int launch_score_init(void* state, hipStream_t st) {
    hipLaunchKernelGGL(score_init_kernel, dim3(1), dim3(64), 0, st, static_cast<double*>(state));
    CVAE_CHECK_LAUNCH();
    return 0;
}

// ms: the MS-SSIM workspace of the call (ws + the "ms" slot of the carve).  The values-only pyramid with its record-mode
// finalize, then one launch that scores every image and pools the batch.
int launch_score(int width, int B, const float* x, const float* mu, const float* logvar, const float* recon, float* ms,
                 float* per_image, void* state, hipStream_t st) {
    int64_t part[5], scratch;
    msssim_score_slots(width, B, part, &scratch);
    double* rec = reinterpret_cast<double*>(ms + scratch);                 // 11 doubles
    float* rows = per_image ? per_image : ms + scratch + 64;               // B rows of 8 floats: far inside 3 * B * width^2
    int rc = launch_msssim(width, B, recon, x, mu, logvar, ms, nullptr, nullptr, nullptr, nullptr, st, 1, rec, nullptr);
    if (rc) return rc;
    ScoreArgs a{x, recon, mu, logvar, {}, rows, rec, static_cast<double*>(state), B};
    for (int l = 0; l < 5; ++l) a.part[l] = ms + part[l];
    if (width == 64) hipLaunchKernelGGL(score_image_kernel<64>, dim3(B), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(score_image_kernel<128>, dim3(B), dim3(256), 0, st, a);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// the loss scalars of everything pooled since the init: msssim_finish_kernel on the record's sums and image count
int launch_score_finish(int width, void* state, float* scalars, hipStream_t st) {
    double* s = static_cast<double*>(state);
    return launch_msssim_finish_rec(width, s + SC_SUMS, s + SC_IMAGES, scalars, reinterpret_cast<float*>(s + SC_COEF), st);
}
