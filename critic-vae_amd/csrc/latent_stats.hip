// latent_stats.hip — pooled statistics of the latent code of a whole set (cvae_latent_stats, include/cvae.h).
//
// One launch per batch reads mu (B,32), logvar (B,32) and pred (B) and ADDS the batch to a pooled fp64 record: rows seen and
// used, the first and second moments of a = (mu_0..mu_31, pred) and the per-dimension sums of the KL term, exp(logvar) and
// logvar.  All arithmetic is fp64 on the fp32 inputs widened, exp included.  The design is grad_stats_kernel / tensor_stats /
// score.hip again: rows are cut into chunks of LS_ROWS, min(chunks, compute units) persistent workgroups stride over the
// chunks, each leaves one fp64 partial record in scratch, and the last workgroup to arrive (wg_arrive_last) sums the
// partials in workgroup order and adds them to the record.  No floating-point atomics: the same calls give the same bits.
//
// Inside a workgroup a chunk is staged in LDS as rows of b = (mu_0..mu_31, pred, 1) in fp32 — the inputs are fp32, so the
// staging loses nothing — with a row that is not used staged as zeros.  The 595 entries of the upper triangle of sum b b^T are
// then everything the record's slots [1..595] need: (33,33) counts the used rows, (i,33) is sum a_i, the rest is the Gram
// matrix.  Thread t owns entries t, t + 256, t + 512 and walks the chunk's rows in ascending order; a product of two widened
// fp32 values is exact in fp64, so a contraction to fma changes nothing.
#include "common.h"
#include "../../include/cvae.h"
#include <math.h>

static constexpr int LS_ROWS = 128;                      // rows per chunk
static constexpr int LS_NB = 34;                         // (mu_0..mu_31, pred, 1)
static constexpr int LS_TRI = LS_NB * (LS_NB + 1) / 2;   // 595
static constexpr int LS_USED = 1, LS_SUM = 2, LS_GRAM = 35, LS_KL = 596, LS_EXP = 628, LS_LV = 660, LS_TICKET = 692;
static constexpr int LS_PART = LS_TICKET;                // doubles per workgroup partial: the record without its scratch slots
static constexpr int LS_MAX_WGS = 1024;                  // grid cap; scratch is sized by it, not by the device
static constexpr int LS_MAX_BATCH = 1 << 24;
static_assert(CVAE_LATENT_STATE_DOUBLES == LS_TICKET + 4 && CVAE_LATENT == 32 && CVAE_ZCAT == 33, "record layout of include/cvae.h");
static_assert(LS_GRAM + CVAE_ZCAT * (CVAE_ZCAT + 1) / 2 == LS_KL && 1 + LS_TRI == LS_KL && LS_EXP == LS_KL + 32 && LS_LV == LS_EXP + 32 &&
              LS_TICKET == LS_LV + 32, "record layout of include/cvae.h");

struct LsArgs {
    const float* mu; const float* logvar;    // (B, 32)
    const float* pred;                       // (B)
    double* state;                           // the pooled record
    float* kl_rows;                          // (B, 32) or null
    double* part;                            // gridDim.x partial records of LS_PART doubles
    int B, chunks;
};

__device__ __forceinline__ bool ls_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN

__global__ __launch_bounds__(256) void latent_stats_kernel(LsArgs a) {
    __shared__ float s[LS_ROWS][LS_NB];
    __shared__ double red[3][8][32];
    __shared__ unsigned last_flag;
    const int tid = threadIdx.x, j = tid & 31, rg = tid >> 5;
    // the entries of the upper triangle this thread owns, and the record slot of each (-1: none)
    int ei[3], ej[3], slot[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int e = tid + 256 * q;
        int i = 0, rem = e;
        while (i < LS_NB && rem >= LS_NB - i) { rem -= LS_NB - i; ++i; }
        const bool has = e < LS_TRI;
        ei[q] = has ? i : 0; ej[q] = has ? i + rem : 0;
        slot[q] = !has ? -1 : ej[q] == 33 ? (i == 33 ? LS_USED : LS_SUM + i) : LS_GRAM + i * 33 - i * (i - 1) / 2 + (ej[q] - i);
    }
    double g[3] = {0.0, 0.0, 0.0};
    double kl = 0.0, ev = 0.0, lv = 0.0;     // of dimension j over the rows rg, rg + 8, ... of this workgroup's chunks
    for (int c = blockIdx.x; c < a.chunks; c += gridDim.x) {
        const int r0 = c * LS_ROWS, n = a.B - r0 < LS_ROWS ? a.B - r0 : LS_ROWS;
        // ---- stage: half-wave rg takes rows rg, rg + 8, ..., lane j dimension j; the loop is uniform, the loads are guarded ----
        for (int rb = 0; rb < n; rb += 8) {
            const int r = rb + rg;
            const bool in = r < n;
            const size_t idx = ((size_t)r0 + (size_t)(in ? r : 0)) * 32 + j;
            float m = 0.f, l = 0.f, p = 0.f;
            if (in) { m = a.mu[idx]; l = a.logvar[idx]; p = a.pred[(size_t)r0 + r]; }
            const double md = (double)m, ld = (double)l, e = exp(ld);
            const double k = 0.5 * (md * md + e - ld - 1.0);
            if (in && a.kl_rows) a.kl_rows[idx] = (float)k;
            int bad = (ls_finite(md) && ls_finite(ld) && ls_finite(e) && ls_finite((double)p)) ? 0 : 1;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);      // over the 32 lanes of the row
            const bool use = in && !bad;
            if (in) {
                s[r][j] = use ? m : 0.f;
                if (j == 0) { s[r][32] = use ? p : 0.f; s[r][33] = use ? 1.f : 0.f; }
            }
            if (use) { kl += k; ev += e; lv += ld; }
        }
        __syncthreads();
        // ---- the triangle of sum b b^T over the chunk's rows, ascending ----
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (slot[q] < 0) continue;
            double t = g[q];
            for (int r = 0; r < n; ++r) t += (double)s[r][ei[q]] * (double)s[r][ej[q]];
            g[q] = t;
        }
        __syncthreads();                     // s is free for the next chunk
    }
    red[0][rg][j] = kl; red[1][rg][j] = ev; red[2][rg][j] = lv;
    __syncthreads();
    double* part = a.part + (size_t)blockIdx.x * LS_PART;
#pragma unroll
    for (int q = 0; q < 3; ++q) if (slot[q] >= 0) part[slot[q]] = g[q];
    if (tid < 96) {
        const int w = tid >> 5;
        double t = red[w][0][j];
        for (int k = 1; k < 8; ++k) t += red[w][k][j];
        part[LS_KL + w * 32 + j] = t;
    }
    if (tid == 96) part[0] = 0.0;            // rows seen: the merge adds B
    // ---- the batch into the pooled record: the last workgroup to arrive, partials in workgroup order ----
    if (!wg_arrive_last(reinterpret_cast<unsigned*>(a.state + LS_TICKET), gridDim.x, &last_flag)) return;
    for (int k = tid; k < LS_PART; k += 256) {
        double t = 0.0;
        for (unsigned w = 0; w < gridDim.x; ++w) t += a.part[(size_t)w * LS_PART + k];
        a.state[k] += k == 0 ? (double)a.B : t;
    }
}

int64_t latent_stats_state_bytes() { return (int64_t)CVAE_LATENT_STATE_DOUBLES * 8; }

// (rows per chunk, chunks, workgroups) at a batch on a device of num_cus compute units; -1 for a batch outside 1..2^24 or
// num_cus < 1.  Host arithmetic only; the launcher and cvae_latent_stats_plan both read it.
int latent_stats_plan(int B, int num_cus, int plan[3]) {
    if (B < 1 || B > LS_MAX_BATCH || num_cus < 1) return -1;
    const int chunks = cdiv(B, LS_ROWS), cap = num_cus < LS_MAX_WGS ? num_cus : LS_MAX_WGS;
    plan[0] = LS_ROWS; plan[1] = chunks; plan[2] = chunks < cap ? chunks : cap;
    return 0;
}

// one partial per workgroup the launch can have at this batch on ANY device (the grid is capped by LS_MAX_WGS)
int64_t latent_stats_scratch_bytes(int B) {
    int plan[3];
    if (latent_stats_plan(B, LS_MAX_WGS, plan) != 0) return -1;
    return align_up((int64_t)plan[2] * LS_PART * 8, 16);
}

int launch_latent_stats(int B, const float* mu, const float* logvar, const float* pred, void* state, float* kl_rows, void* scratch,
                        hipStream_t st) {
    int plan[3];
    if (latent_stats_plan(B, cvae_num_cus(), plan) != 0) { cvae_set_error("cvae_latent_stats: batch %d outside 1..2^24", B); return -1; }
    LsArgs a{mu, logvar, pred, static_cast<double*>(state), kl_rows, static_cast<double*>(scratch), B, plan[1]};
    hipLaunchKernelGGL(latent_stats_kernel, dim3((unsigned)plan[2]), dim3(256), 0, st, a);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// ---- cvae_recon_response: what the decoder listens to (include/cvae.h) ----
// One workgroup per (image, variant) streams the variant's reconstruction and the image's base reconstruction once:
// [0] the mean over 3 W^2 of (var - base)^2 — differences and squares fp32, the sum fp64 in a fixed order, as cvae_score's
// column 3 — and [1] the maximum over pixels of the grey difference of cvae_diff_grey.  No scratch, no atomics.
//
// The grey value restates diff_grey_kernel (critic.hip) with every rounding spelled out, in the form that kernel compiles to:
// the red and blue products rounded on their own, the green product fused into the red one, then one addition.  The tests hold
// the two bit-equal on real frames.
__device__ __forceinline__ float grey_abs_diff(float dr, float dg, float db) {
#pragma clang fp contract(off)               // the one fusion is the fmaf written out; the intrinsics __fmul_rn / __fadd_rn do not stop contraction
    const float red = fabsf(dr) * 0.2989f, blue = fabsf(db) * 0.1140f;
    return __builtin_fmaf(fabsf(dg), 0.5870f, red) + blue;
}

template <int W>
__global__ __launch_bounds__(256) void recon_response_kernel(const float* __restrict__ base, const float* __restrict__ var,
                                                             float* __restrict__ out, int K) {
    constexpr int HW = W * W, HW4 = HW / 4;
    __shared__ double red_s[4];
    __shared__ float red_m[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t item = blockIdx.x, img = item / (size_t)K;
    const f32x4* pb = reinterpret_cast<const f32x4*>(base + img * (size_t)(3 * HW));
    const f32x4* pv = reinterpret_cast<const f32x4*>(var + item * (size_t)(3 * HW));
    double s = 0.0;
    float mx = 0.f;
    bool bad = false;                        // a NaN difference: fmaxf would drop it
#pragma unroll 2
    for (int q = tid; q < HW4; q += 256) {
        const f32x4 dr = pv[q] - pb[q], dg = pv[q + HW4] - pb[q + HW4], db = pv[q + 2 * HW4] - pb[q + 2 * HW4];
        const f32x4 r2 = dr * dr, g2 = dg * dg, b2 = db * db;
        s += ((double)r2[0] + (double)r2[1]) + ((double)r2[2] + (double)r2[3]);
        s += ((double)g2[0] + (double)g2[1]) + ((double)g2[2] + (double)g2[3]);
        s += ((double)b2[0] + (double)b2[1]) + ((double)b2[2] + (double)b2[3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gr = grey_abs_diff(dr[e], dg[e], db[e]);
            mx = fmaxf(mx, gr); bad |= gr != gr;
        }
    }
    if (bad) mx = NAN;
    s = wave_sum_d(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float v = __shfl_xor(mx, o, 64); mx = (mx != mx || v != v) ? NAN : fmaxf(mx, v); }
    if (lane == 0) { red_s[wv] = s; red_m[wv] = mx; }
    __syncthreads();
    if (tid == 0) {
        const double ss = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
        float m = red_m[0];
        for (int k = 1; k < 4; ++k) m = (m != m || red_m[k] != red_m[k]) ? NAN : fmaxf(m, red_m[k]);
        out[item * 2] = (float)(ss / (double)(3 * HW));
        out[item * 2 + 1] = m;
    }
}

int launch_recon_response(int width, int64_t items, int K, const float* base, const float* var, float* out, hipStream_t st) {
    if (width == 64) hipLaunchKernelGGL(recon_response_kernel<64>, dim3((unsigned)items), dim3(256), 0, st, base, var, out, K);
    else hipLaunchKernelGGL(recon_response_kernel<128>, dim3((unsigned)items), dim3(256), 0, st, base, var, out, K);
    CVAE_CHECK_LAUNCH();
    return 0;
}
