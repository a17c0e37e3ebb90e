// critic_score.hip — per-frame scores of the critic against its targets and the pooled record of a held-out set
// (cvae_critic_score, include/cvae.h).
//
// One launch, a persistent grid of at most one workgroup per compute unit (the forward holds 104 KB of LDS).  Per frame a
// workgroup stages the 12 KB uint8 HWC frame straight into the zero-bordered LDS planes as (float)u8 / 255.0f — the
// arithmetic of preprocess_u8_gather_kernel (dataset.hip), no fp32 frame in memory —, runs the eval-mode forward of
// critic_fwd.h (the device code of critic_fwd_kernel: the same bits) and writes one row of CVAE_CRITIC_SCORE_COLS floats.
// The borders are zeroed once per workgroup: every later write goes to an interior.  The last workgroup to arrive then
// adds the batch to the pooled fp64 record: rows in a fixed thread-strided order, integer LDS atomics for the confusion
// counts only, no floating-point atomics — the same calls give the same bits.
#include "common.h"
#include "critic_fwd.h"
#include "../../include/cvae.h"
#include <math.h>

// the pooled record (include/cvae.h, cvae_critic_score): CVAE_CRITIC_SCORE_STATE_DOUBLES doubles
static constexpr int CS_SEEN = 0, CS_FINITE = 1 /* then the 8 sums */, CS_MAX = 10, CS_CONF = 11 /* 4 x 4 */, CS_TICKET = 32;
static_assert(CVAE_CRITIC_SCORE_STATE_DOUBLES == 40 && CVAE_CRITIC_SCORE_COLS == 8, "record layout of include/cvae.h");

struct CriticScoreArgs {
    const uint8_t* frames;       // (n, 64, 64, 3)
    const float* targets;        // (n)
    int64_t n;
    const int64_t* idx;          // (B) or null: frame i of the batch is i
    const float* cp;             // the critic's 11 873 floats
    float* rows;                 // (B, CVAE_CRITIC_SCORE_COLS)
    double* state;               // pooled record or null
    int B;
};

// 0 mid, 1 high, 2 low, 3 none: bin_of (dataset.hip) with "none" stored as 3; float32 comparisons, NaN falls in no bin
__device__ __forceinline__ int value_bin(float v) {
    if (v >= 0.4f && v <= 0.6f) return 0;
    if (v >= 0.7f) return 1;
    if (v <= 0.25f) return 2;
    return 3;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }

__global__ __launch_bounds__(64) void critic_score_init_kernel(double* state) {
    const int i = threadIdx.x;
    if (i < CVAE_CRITIC_SCORE_STATE_DOUBLES) state[i] = i == CS_MAX ? (double)-INFINITY : 0.0;      // an all-zero double is ticket 0 too
}

__global__ __launch_bounds__(256) void critic_score_kernel(CriticScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double red_b[10][4];
    __shared__ unsigned conf_s[16];
    __shared__ unsigned last_flag;
    float* lx = smem;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int q = tid; q < critic_fwd::BORDERED_FLOATS; q += 256) smem[q] = 0.f;      // zero borders, once per workgroup
    __syncthreads();
    for (int i = blockIdx.x; i < a.B; i += gridDim.x) {
        const int64_t s = a.idx ? a.idx[i] : (int64_t)i;
        float* row = a.rows + (size_t)i * CVAE_CRITIC_SCORE_COLS;
        if (s < 0 || s >= a.n) {                 // the same in every thread: a NaN row, nothing of frame s is read
            if (tid == 0) {
                const float q = __builtin_nanf("");
                row[0] = q; row[1] = q; row[2] = q; row[3] = q; row[4] = q; row[5] = 3.f; row[6] = 3.f; row[7] = 0.f;
            }
            continue;
        }
        // 16 pixels per thread: three 16-byte loads of uint8 HWC, (float)u8 / 255.0f into the interior of plane c
        {
            const uint4* src = reinterpret_cast<const uint4*>(a.frames + s * (3 * 64 * 64) + tid * 48);
            const uint4 v0 = src[0], v1 = src[1], v2 = src[2];
            const uint32_t wd[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
            float* d = lx + ((tid >> 2) + 1) * 66 + (tid & 3) * 16 + 1;
#pragma unroll
            for (int e = 0; e < 48; ++e) {
                const float val = (float)((wd[e >> 2] >> ((e & 3) * 8)) & 0xffu) / 255.0f;
                d[(e % 3) * 66 * 66 + e / 3] = val;
            }
        }
        __syncthreads();
        const float p = critic_fwd::forward_from_lds(smem, a.cp);
        if (tid == 0) {
            const float t = a.targets[s];
            const float d = __fsub_rn(p, t);
            // torch's binary_cross_entropy, both logs clamped at -100; every operation rounded on its own (no contraction)
            const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(logf(__fsub_rn(1.f, p)), -100.f);
            row[0] = p; row[1] = t;
            row[2] = -__fadd_rn(__fmul_rn(t, lp), __fmul_rn(__fsub_rn(1.f, t), lq));
            row[3] = __fmul_rn(d, d); row[4] = fabsf(d);
            row[5] = (float)value_bin(p); row[6] = (float)value_bin(t); row[7] = 0.f;
        }
        __syncthreads();                         // the next frame's staging overwrites lx
    }
    if (!a.state) return;
    // ---- the batch into the pooled record: the last workgroup to arrive, rows in thread-strided order ----
    if (!wg_arrive_last(reinterpret_cast<unsigned*>(a.state + CS_TICKET), gridDim.x, &last_flag)) return;
    if (tid < 16) conf_s[tid] = 0u;
    __syncthreads();
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // finite frames, then the 8 sums over them
    double bmax = (double)-INFINITY;
    for (int i = tid; i < a.B; i += 256) {
        const float* row = a.rows + (size_t)i * CVAE_CRITIC_SCORE_COLS;
        const float p = row[0], t = row[1], bce = row[2], se = row[3], ae = row[4];
        if (!(finite_f(p) && finite_f(t) && finite_f(bce) && finite_f(se) && finite_f(ae))) continue;      // counted in [0] only
        const double pd = (double)p, td = (double)t;
        acc[0] += 1.0;
        acc[1] += (double)bce; acc[2] += (double)se; acc[3] += (double)ae;
        acc[4] += pd; acc[5] += td; acc[6] += pd * pd; acc[7] += td * td; acc[8] += pd * td;
        bmax = fmax(bmax, (double)ae);
        atomicAdd(&conf_s[((int)row[6] & 3) * 4 + ((int)row[5] & 3)], 1u);      // integer counts: any order gives the same
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) { const double v = wave_sum_d(acc[c]); if (lane == 0) red_b[c][wv] = v; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bmax = fmax(bmax, __shfl_xor(bmax, o, 64));
    if (lane == 0) red_b[9][wv] = bmax;
    __syncthreads();
    if (tid == 0) a.state[CS_SEEN] += (double)a.B;
    else if (tid < 10) { const int c = tid - 1; a.state[CS_FINITE + c] += (red_b[c][0] + red_b[c][1]) + (red_b[c][2] + red_b[c][3]); }
    else if (tid == 10) a.state[CS_MAX] = fmax(a.state[CS_MAX], fmax(fmax(red_b[9][0], red_b[9][1]), fmax(red_b[9][2], red_b[9][3])));
    else if (tid < 27) a.state[CS_CONF + tid - 11] += (double)conf_s[tid - 11];
}

int64_t critic_score_state_bytes() { return CVAE_CRITIC_SCORE_STATE_DOUBLES * 8; }
int64_t critic_score_scratch_bytes(int B) { return (int64_t)B * CVAE_CRITIC_SCORE_COLS * 4; }

int launch_critic_score_init(void* state, hipStream_t st) {
    hipLaunchKernelGGL(critic_score_init_kernel, dim3(1), dim3(64), 0, st, static_cast<double*>(state));
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_critic_score(int B, const uint8_t* frames, const float* targets, int64_t n, const int64_t* idx, const float* critic_params,
                        float* rows, void* state, hipStream_t st) {
    static DeviceOnce once;
    { int rc = cvae_grant_lds(once, reinterpret_cast<const void*>(critic_score_kernel), critic_fwd::SMEM_BYTES); if (rc) return rc; }
    CriticScoreArgs a{frames, targets, n, idx, critic_params, rows, static_cast<double*>(state), B};
    hipLaunchKernelGGL(critic_score_kernel, dim3(persistent_grid(1, B)), dim3(256), critic_fwd::SMEM_BYTES, st, a);
    CVAE_CHECK_LAUNCH();
    return 0;
}
