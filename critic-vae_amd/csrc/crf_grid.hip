// crf_grid.hip — the dense CRF of segment.hip for K variants of one frame set in one call: the grid search that crf()
// (vae_utility.py:22-54) is written as.  All variants of a call share (alpha, beta, gamma), hence the kernels k_b, k_g and
// their normalisers n_b, n_g; a variant is its unary (a threshold of the uint8 difference mask, or the fp32 prob1 plane, with
// its floor) and its weights (w1, w2).  The equations are those of segment.hip / include/cvae.h (cvae_dense_crf).
//
// The pair pass computes k_b(i,j) once per (query, neighbour) pair and applies it to the KC message values n_b v_c of the
// neighbour, which every lane reads from the same LDS address (a broadcast).  Per channel the summation order is that of
// crf_bilateral_kernel: chunks of CH neighbours in order, a per-chunk partial, partials added in order.  More than KC variants
// run as consecutive groups over the same scratch.  The file is compiled with -ffp-contract=off and spells its fused operations
// out, so that every instantiation and every slot performs the same roundings: the bits of one (frame, variant) result depend
// on that frame and that variant alone.
//
// Launches per call: init, normaliser pass; per group a start pass (Q0 = softmax(-u)) and per iteration a Gaussian row pass
// over the group's planes plus a pair pass.  After a listed iteration the pass that computed d also counts (tp, fn, fp) of
// d > 0 against gt with integer atomics (order-free).  No floating-point atomics.
#include "common.h"
#include "../../include/cvae.h"

namespace {

constexpr int TPB = 256;         // threads per workgroup
constexpr int QPT = 4;           // query pixels per thread of the pair pass
constexpr int QBLK = TPB * QPT;  // query pixels per workgroup
constexpr int CH = 1024;         // neighbours per LDS chunk: CH * (4 + KC) floats
constexpr int KMAX = 8;          // the largest KC built: variants per group
constexpr float LOG2E = 1.4426950408889634f;

struct GridVariants {            // one group, by value
    int32_t thr[KMAX];
    float pf[KMAX], w1[KMAX], w2[KMAX];
};

struct GridScratch {             // col, ng, nbn hold B*W*W elements; the planes hold S * B*W*W, S = min(K, KMAX)
    float4* col;                 // (r', g', b', 0): colours prescaled by sb
    float *ng, *nbn;             // Gaussian / bilateral normalisers
    float *m0, *m1;              // n_b * v per slot, ping-pong across passes
    float *ug, *tg;              // n_g * v per slot and its row-filtered form
};

struct GridOut {                 // what a pass leaves besides the next pass's inputs
    const uint8_t* gt;
    unsigned long long* counts;  // this snapshot's (K, B, 3) block, or null when the pass is no snapshot
    uint8_t* labels;             // (K, B, W, W), null unless this is the last pass and labels were asked for
    float* q1;
    int k0, B, last;             // first variant of the group, batch, 1 = no further pass follows
};

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

GridScratch carve_grid(void* base, int64_t npix, int S) {
    char* p = (char*)base;
    GridScratch s;
    s.col = (float4*)p; p += align256(npix * 16);
    s.ng = (float*)p; p += align256(npix * 4);
    s.nbn = (float*)p; p += align256(npix * 4);
    const int64_t plane = align256(npix * 4 * S);
    s.m0 = (float*)p; p += plane;
    s.m1 = (float*)p; p += plane;
    s.ug = (float*)p; p += plane;
    s.tg = (float*)p;
    return s;
}

__device__ __forceinline__ float gauss_tap(int d, float cg) { return __builtin_amdgcn_exp2f(-(float)(d * d) * cg); }

// u(0) - u(1), u(l) = -log(max(prob(l), p_floor)), as crf_init_kernel forms it; thr >= 0 reads the thresholded uint8 mask
__device__ __forceinline__ float unary_d0(int thr, float pfloor, const float* __restrict__ prob1, const uint8_t* __restrict__ u8,
                                          int64_t i) {
    const float p1 = thr < 0 ? prob1[i] : ((int)u8[i] > thr ? 1.0f : 0.0f), p0 = 1.0f - p1;
    return logf(fmaxf(p1, pfloor)) - logf(fmaxf(p0, pfloor));
}

// (tp, fn, fp) of one pixel in 10-bit fields: a wave of 64 lanes with QPT pixels each sums to at most 256 per field
__device__ __forceinline__ int count_bits(int m, int g) { return (g & m) | ((g & (1 - m)) << 10) | (((1 - g) & m) << 20); }

// sum of the packed fields over the wave, added by lane 0 into wc[0..2] (LDS, zeroed before, integer atomics)
__device__ __forceinline__ void wave_counts(int pk, unsigned* wc) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pk += __shfl_xor(pk, o);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&wc[0], (unsigned)(pk & 1023));
        atomicAdd(&wc[1], (unsigned)((pk >> 10) & 1023));
        atomicAdd(&wc[2], (unsigned)((pk >> 20) & 1023));
    }
}

// per pixel, shared by all variants: prescaled colours and the Gaussian normaliser
__global__ __launch_bounds__(TPB) void grid_init_kernel(const uint8_t* __restrict__ frames, GridScratch s, int W, int64_t npix,
                                                        float sb, float cg) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= npix) return;
    const int p = (int)(i % ((int64_t)W * W)), x = p % W, y = p / W;
    const uint8_t* c = frames + i * 3;
    s.col[i] = make_float4((float)c[0] * sb, (float)c[1] * sb, (float)c[2] * sb, 0.0f);
    float gx = 0.f, gy = 0.f;
    for (int k = 0; k < W; ++k) {
        gx += gauss_tap(x - k, cg);
        gy += gauss_tap(y - k, cg);
    }
    s.ng[i] = 1.0f / sqrtf(gx * gy);                                    // sum_j k_g(i,j) = Gx(x) Gy(y)
}

// Q0 = softmax(-u) of every slot of a group: the first messages, and snapshot 0.  One workgroup = TPB pixels of one frame.
__global__ __launch_bounds__(TPB) void grid_start_kernel(const float* __restrict__ prob1, const uint8_t* __restrict__ u8,
                                                         GridScratch s, GridVariants v, int nv, int N, int64_t npix, GridOut o) {
    __shared__ unsigned wc[KMAX * 3];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * TPB + tid;                   // npix is a multiple of TPB
    const int64_t f = i / N;
    if (tid < KMAX * 3) wc[tid] = 0;
    __syncthreads();
    const float ng = s.ng[i], nb = s.nbn[i];
    const int g = o.counts ? (o.gt[i] != 0) : 0;
#pragma unroll
    for (int c = 0; c < KMAX; ++c) {
        if (c < nv) {
            const float d = unary_d0(v.thr[c], v.pf[c], prob1, u8, i);
            const float q = 1.0f / (1.0f + expf(-d));
            if (o.counts) wave_counts(count_bits(d > 0.f ? 1 : 0, g), wc + c * 3);
            if (o.last) {
                const int64_t oi = ((int64_t)(o.k0 + c) * o.B) * N + i;
                if (o.labels) o.labels[oi] = d > 0.f ? 1 : 0;
                if (o.q1) o.q1[oi] = q;
            } else {
                const float vv = fmaf(2.0f, q, -1.0f);
                s.m0[(int64_t)c * npix + i] = __fmul_rn(nb, vv);
                s.ug[(int64_t)c * npix + i] = __fmul_rn(ng, vv);
            }
        }
    }
    if (o.counts) {
        __syncthreads();
        if (tid < nv * 3 && wc[tid]) atomicAdd(&o.counts[((int64_t)(o.k0 + tid / 3) * o.B + f) * 3 + tid % 3], (unsigned long long)wc[tid]);
    }
}

// tg[y][x] = sum_x' g(x - x') ug[y][x'] over every row of the group's planes (row half of the separable Gaussian filter)
__global__ __launch_bounds__(TPB) void grid_gauss_rows_kernel(const float* __restrict__ ug, float* __restrict__ tg, int W,
                                                              int64_t total, float cg) {
    __shared__ float tap[128];
    if (threadIdx.x < W) tap[threadIdx.x] = gauss_tap(threadIdx.x, cg);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W);
    const float* row = ug + (i - x);
    float acc = 0.f;
    for (int k = 0; k < W; ++k) acc = fmaf(tap[x > k ? x - k : k - x], row[k], acc);
    tg[i] = acc;
}

// One workgroup = QBLK query pixels of one frame; every neighbour of the frame streams through LDS in chunks of CH.
// NORM: the bilateral normaliser pass (every message is 1, KC = 1) -> nbn.  Else one mean-field update of the nv <= KC slots
// of a group: k_b once per pair, KC accumulators per query pixel.  Slots >= nv hold zero messages and are never written.
template <int W, int KC, bool NORM>
__global__ __launch_bounds__(TPB, 2) void grid_pair_kernel(const float* __restrict__ m_in, float* __restrict__ m_out,
                                                           const float* __restrict__ prob1, const uint8_t* __restrict__ u8,
                                                           GridScratch s, GridVariants v, int nv, int64_t npix, float sa, float cg,
                                                           GridOut o) {
    constexpr int N = W * W, BPF = N / QBLK;
    static_assert(N % QBLK == 0 && N % CH == 0 && CH % W == 0, "tile shape");
    static_assert(KC == 1 || KC % 4 == 0, "message rows are read as float4");
    static_assert(KC <= KMAX && (!NORM || KC == 1), "instantiation");
    __shared__ float4 cs[CH];
    __shared__ __attribute__((aligned(16))) float ms[NORM ? 4 : CH * KC];
    __shared__ float tap[W];
    __shared__ unsigned wc[KMAX * 3];
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x / BPF;
    const int q0 = (int)(blockIdx.x % BPF) * QBLK;
    const int64_t fo = f * N;
    const float4* src = s.col + fo;
    if (tid < W) tap[tid] = gauss_tap(tid, cg);
    if (tid < KMAX * 3) wc[tid] = 0;

    float qx[QPT], qy[QPT], qr[QPT], qg[QPT], qb[QPT], acc[QPT][KC];
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int p = q0 + k * TPB + tid;
        const float4 c = src[p];
        qx[k] = (float)(p % W) * sa; qy[k] = (float)(p / W) * sa;
        qr[k] = c.x; qg[k] = c.y; qb[k] = c.z;
#pragma unroll
        for (int c2 = 0; c2 < KC; ++c2) acc[k][c2] = 0.f;
    }
    for (int c0 = 0; c0 < N; c0 += CH) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CH / TPB; ++k) {
            const int j = k * TPB + tid;
            cs[j] = src[c0 + j];
            if (!NORM) {
#pragma unroll
                for (int c = 0; c < KC; ++c) ms[j * KC + c] = c < nv ? m_in[(int64_t)c * npix + fo + c0 + j] : 0.0f;
            }
        }
        __syncthreads();
        float part[QPT][KC];
#pragma unroll
        for (int k = 0; k < QPT; ++k)
#pragma unroll
            for (int c = 0; c < KC; ++c) part[k][c] = 0.f;
        for (int r = 0; r < CH / W; ++r) {                               // one neighbour row: its dy is fixed
            const float yj = (float)(c0 / W + r) * sa;
            float a0[QPT];
#pragma unroll
            for (int k = 0; k < QPT; ++k) { const float dy = qy[k] - yj; a0[k] = dy * dy; }
            const int jb = r * W;
#pragma unroll 4
            for (int xj = 0; xj < W; ++xj) {
                const float4 n = cs[jb + xj];
                float m[KC];
#pragma unroll
                for (int c = 0; c < KC; ++c) m[c] = NORM ? 1.0f : ms[(jb + xj) * KC + c];
                const float xs = (float)xj * sa;
#pragma unroll
                for (int k = 0; k < QPT; ++k) {
                    const float dx = qx[k] - xs, dr = qr[k] - n.x, dg = qg[k] - n.y, db = qb[k] - n.z;
                    float a = fmaf(dx, dx, a0[k]);
                    a = fmaf(dr, dr, a);
                    a = fmaf(dg, dg, a);
                    a = fmaf(db, db, a);
                    const float kb = __builtin_amdgcn_exp2f(-a);
#pragma unroll
                    for (int c = 0; c < KC; ++c) part[k][c] = fmaf(kb, m[c], part[k][c]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < QPT; ++k)
#pragma unroll
            for (int c = 0; c < KC; ++c) acc[k][c] += part[k][c];
    }
    if (NORM) {
#pragma unroll
        for (int k = 0; k < QPT; ++k) s.nbn[fo + q0 + k * TPB + tid] = 1.0f / sqrtf(acc[k][0]);
        return;
    }
    int pk[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) pk[c] = 0;
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int p = q0 + k * TPB + tid;
        const int64_t i = fo + p;
        const int x = p % W, y = p / W;
        const float nb = s.nbn[i], ng = s.ng[i];
        const int g = o.counts ? (o.gt[i] != 0) : 0;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            if (c < nv) {
                const float* col = s.tg + (int64_t)c * npix + fo + x;
                float sg = 0.f;
#pragma unroll 8
                for (int yy = 0; yy < W; ++yy) sg = fmaf(tap[y > yy ? y - yy : yy - y], col[yy * W], sg);
                float d = unary_d0(v.thr[c], v.pf[c], prob1, u8, i);
                d = fmaf(v.w2[c], __fmul_rn(ng, sg), d);
                d = fmaf(v.w1[c], __fmul_rn(nb, acc[k][c]), d);
                const float q = 1.0f / (1.0f + expf(-d));
                pk[c] += count_bits(d > 0.f ? 1 : 0, g);
                if (o.last) {
                    const int64_t oi = ((int64_t)(o.k0 + c) * o.B) * N + i;
                    if (o.labels) o.labels[oi] = d > 0.f ? 1 : 0;
                    if (o.q1) o.q1[oi] = q;
                } else {
                    const float vv = fmaf(2.0f, q, -1.0f);
                    m_out[(int64_t)c * npix + i] = __fmul_rn(nb, vv);
                    s.ug[(int64_t)c * npix + i] = __fmul_rn(ng, vv);
                }
            }
        }
    }
    if (o.counts) {                                                      // wc was zeroed before the chunk loop's barriers
#pragma unroll
        for (int c = 0; c < KC; ++c)
            if (c < nv) wave_counts(pk[c], wc + c * 3);
        __syncthreads();
        if (tid < nv * 3 && wc[tid]) atomicAdd(&o.counts[((int64_t)(o.k0 + tid / 3) * o.B + f) * 3 + tid % 3], (unsigned long long)wc[tid]);
    }
}

template <int W, int KC>
void launch_pair(unsigned blocks, hipStream_t st, const float* in, float* out, const float* prob1, const uint8_t* u8,
                 const GridScratch& s, const GridVariants& v, int nv, int64_t npix, float sa, float cg, const GridOut& o) {
    hipLaunchKernelGGL((grid_pair_kernel<W, KC, false>), dim3(blocks), dim3(TPB), 0, st, in, out, prob1, u8, s, v, nv, npix, sa, cg, o);
}

template <int W>
int run_grid(int B, const uint8_t* frames, const float* prob1, const uint8_t* u8, const uint8_t* gt, float alpha, float beta,
             float gamma, const cvae_crf_variant* var, int K, const int32_t* snaps, int n_snaps, int64_t* counts,
             uint8_t* labels, float* q1, void* scratch, hipStream_t st) {
    constexpr int N = W * W;
    const int64_t npix = (int64_t)B * N;
    const int S = K < KMAX ? K : KMAX;
    const GridScratch s = carve_grid(scratch, npix, S);
    // exp(-x^2 / (2 s^2)) = exp2(-(x * sqrt(log2 e / (2 s^2)))^2).  A tiny alpha, beta or gamma sends its scale to +inf, and
    // 0 * inf (pixel 0, colour 0, tap 0) is NaN; a large finite sa is no better, since a product with it that rounds
    // zeroes a pixel's own tap.  The scales stop where exp2 of the smallest nonzero distance is already 0 (2^-256) and
    // that of distance 0 is 1: the identity filter, as in exact arithmetic.  Powers of two, so that coordinate * scale is
    // exact.  (The clamps of run_crf in segment.hip.)
    const float sa = fminf(sqrtf(LOG2E / (2.0f * alpha * alpha)), 16.0f);
    const float sb = fminf(sqrtf(LOG2E / (2.0f * beta * beta)), 16.0f);
    const float cg = fminf(LOG2E / (2.0f * gamma * gamma), 256.0f);
    const unsigned pix_blocks = (unsigned)(npix / TPB);
    const unsigned pair_blocks = (unsigned)(npix / QBLK);
    const int last_it = snaps[n_snaps - 1];
    if (counts) {
        hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_snaps * K * B * 3 * sizeof(int64_t), st);
        if (e != hipSuccess) { cvae_set_error("cvae_crf_grid: clearing the counts failed: %s", hipGetErrorString(e)); return (int)e; }
    }
    hipLaunchKernelGGL(grid_init_kernel, dim3(pix_blocks), dim3(TPB), 0, st, frames, s, W, npix, sb, cg);
    CVAE_CHECK_LAUNCH();
    {
        GridVariants none = {};
        GridOut no = {};
        hipLaunchKernelGGL((grid_pair_kernel<W, 1, true>), dim3(pair_blocks), dim3(TPB), 0, st, (const float*)nullptr, (float*)nullptr,
                           (const float*)nullptr, (const uint8_t*)nullptr, s, none, 0, npix, sa, cg, no);
        CVAE_CHECK_LAUNCH();
    }
    for (int k0 = 0; k0 < K; k0 += KMAX) {
        const int nv = K - k0 < KMAX ? K - k0 : KMAX;
        GridVariants v = {};
        for (int c = 0; c < nv; ++c) {
            v.thr[c] = var[k0 + c].thr; v.pf[c] = var[k0 + c].p_floor; v.w1[c] = var[k0 + c].w1; v.w2[c] = var[k0 + c].w2;
        }
        int sn = 0;                                                      // next snapshot to meet
        float *in = s.m0, *out = s.m1;
        for (int it = 0; it <= last_it; ++it) {
            GridOut o;
            o.gt = gt;
            o.counts = nullptr;
            if (sn < n_snaps && snaps[sn] == it) {
                if (counts) o.counts = (unsigned long long*)counts + (int64_t)sn * K * B * 3;
                ++sn;
            }
            o.last = it == last_it ? 1 : 0;
            o.labels = o.last ? labels : nullptr;
            o.q1 = o.last ? q1 : nullptr;
            o.k0 = k0; o.B = B;
            if (it == 0) {
                hipLaunchKernelGGL(grid_start_kernel, dim3(pix_blocks), dim3(TPB), 0, st, prob1, u8, s, v, nv, N, npix, o);
                CVAE_CHECK_LAUNCH();
                continue;
            }
            const int64_t total = (int64_t)nv * npix;
            hipLaunchKernelGGL(grid_gauss_rows_kernel, dim3((unsigned)(total / TPB)), dim3(TPB), 0, st, s.ug, s.tg, W, total, cg);
            CVAE_CHECK_LAUNCH();
            if (nv == 1) launch_pair<W, 1>(pair_blocks, st, in, out, prob1, u8, s, v, nv, npix, sa, cg, o);
            else if (nv <= 4) launch_pair<W, 4>(pair_blocks, st, in, out, prob1, u8, s, v, nv, npix, sa, cg, o);
            else launch_pair<W, 8>(pair_blocks, st, in, out, prob1, u8, s, v, nv, npix, sa, cg, o);
            CVAE_CHECK_LAUNCH();
            float* t = in; in = out; out = t;
        }
    }
    return 0;
}

}  // namespace

int crf_grid_group() { return KMAX; }

int64_t crf_grid_scratch_bytes(int width, int B, int K) {
    const int64_t npix = (int64_t)B * width * width;
    const int S = K < KMAX ? K : KMAX;
    return align256(npix * 16) + 2 * align256(npix * 4) + 4 * align256(npix * 4 * S);
}

int launch_crf_grid(int width, int B, const uint8_t* frames, const float* prob1, const uint8_t* u8, const uint8_t* gt, float alpha,
                    float beta, float gamma, const cvae_crf_variant* var, int K, const int32_t* snaps, int n_snaps,
                    int64_t* counts, uint8_t* labels, float* q1, void* scratch, hipStream_t st) {
    if (width == 64)
        return run_grid<64>(B, frames, prob1, u8, gt, alpha, beta, gamma, var, K, snaps, n_snaps, counts, labels, q1, scratch, st);
    return run_grid<128>(B, frames, prob1, u8, gt, alpha, beta, gamma, var, K, snaps, n_snaps, counts, labels, q1, scratch, st);
}
