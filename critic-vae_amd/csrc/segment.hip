// segment.hip — the evaluation path after the difference mask (eval_textured_frames, vae_utility.py:162-212):
// set-wide normalisation + threshold + IoU counts + histograms of the uint8 masks, and an exact mean-field dense CRF
// (the model SimpleCRF's denseCRF.densecrf names, vae_utility.py:22-54) on two labels.
//
// Dense CRF, per frame of N = W*W pixels, two labels, Potts compatibility:
//   bilateral k_b(i,j) = exp(-|p_i - p_j|^2 / (2 alpha^2) - |c_i - c_j|^2 / (2 beta^2))   (c: raw uint8 RGB)
//   Gaussian  k_g(i,j) = exp(-|p_i - p_j|^2 / (2 gamma^2))                                 (both sums include j = i)
//   n_i = (sum_j k(i,j))^-1/2 per kernel, filtered(v)_i = n_i sum_j k(i,j) n_j v_j
//   d_i = logit_1 - logit_0 = (u_i(0) - u_i(1)) + w2 filtered_g(2Q(1) - 1)_i + w1 filtered_b(2Q(1) - 1)_i
//   Q(1) = 1 / (1 + exp(-d)); label 1 iff d > 0.
// The bilateral sum is brute force over all N^2 pairs (no permutohedral lattice); the Gaussian is separable and runs
// as a row pass (crf_gauss_rows_kernel) plus a column pass inside the bilateral kernel, both over the full width.
// Launches per call: init, normaliser pass, then per iteration a row pass and a bilateral pass.  Each frame's result
// depends on that frame alone (fixed summation order, no float atomics), whatever the batch and its position.
#include "common.h"
#include "../../include/cvae.h"

namespace {

constexpr int TPB = 256;         // threads per workgroup
constexpr int QPT = 4;           // query pixels per thread of the bilateral kernel
constexpr int QBLK = TPB * QPT;  // query pixels per workgroup (W*W is a multiple of it at W = 64 and 128)
constexpr int CH = 1024;         // neighbours per LDS chunk (float4 each: 16 KiB)
constexpr float LOG2E = 1.4426950408889634f;

struct CrfScratch {              // per-call carve: every array holds B*W*W elements
    float4 *nb0, *nb1;           // neighbour data (r', g', b', n_b * v), ping-pong across passes
    float *d0, *ng, *nbn, *ug, *tg;   // unary difference, Gaussian / bilateral normalisers, n_g * v, its row-filtered form
};

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

CrfScratch carve_crf(void* base, int64_t npix) {
    char* p = (char*)base;
    CrfScratch s;
    s.nb0 = (float4*)p; p += align256(npix * 16);
    s.nb1 = (float4*)p; p += align256(npix * 16);
    s.d0 = (float*)p; p += align256(npix * 4);
    s.ng = (float*)p; p += align256(npix * 4);
    s.nbn = (float*)p; p += align256(npix * 4);
    s.ug = (float*)p; p += align256(npix * 4);
    s.tg = (float*)p;
    return s;
}

// Gaussian taps g[d] = exp(-d^2 / (2 gamma^2)), d = 0..W-1, as exp2 of an exact integer times a constant
__device__ __forceinline__ float gauss_tap(int d, float cg) { return __builtin_amdgcn_exp2f(-(float)(d * d) * cg); }

// per pixel: prescaled colour features, unary difference, Gaussian normaliser; nb0 = (r', g', b', 1) for the normaliser pass
__global__ __launch_bounds__(TPB) void crf_init_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ prob1,
                                                       CrfScratch s, int W, int64_t npix, float sb, float cg, float pfloor) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= npix) return;
    const int p = (int)(i % ((int64_t)W * W)), x = p % W, y = p / W;
    const uint8_t* c = frames + i * 3;
    s.nb0[i] = make_float4((float)c[0] * sb, (float)c[1] * sb, (float)c[2] * sb, 1.0f);
    const float p1 = prob1[i], p0 = 1.0f - p1;
    s.d0[i] = logf(fmaxf(p1, pfloor)) - logf(fmaxf(p0, pfloor));         // u(0) - u(1), u(l) = -log(max(prob(l), p_floor))
    float gx = 0.f, gy = 0.f;
    for (int k = 0; k < W; ++k) {
        gx += gauss_tap(x - k, cg);
        gy += gauss_tap(y - k, cg);
    }
    s.ng[i] = 1.0f / sqrtf(gx * gy);                                    // sum_j k_g(i,j) = Gx(x) Gy(y)
}

// tg[f][y][x] = sum_x' g(x - x') ug[f][y][x']   (row half of the separable Gaussian filter)
__global__ __launch_bounds__(TPB) void crf_gauss_rows_kernel(const float* __restrict__ ug, float* __restrict__ tg, int W,
                                                             int64_t npix, float cg) {
    __shared__ float tap[128];
    if (threadIdx.x < W) tap[threadIdx.x] = gauss_tap(threadIdx.x, cg);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= npix) return;
    const int x = (int)(i % W);
    const float* row = ug + (i - x);
    float acc = 0.f;
    for (int k = 0; k < W; ++k) acc = fmaf(tap[x > k ? x - k : k - x], row[k], acc);
    tg[i] = acc;
}

// One workgroup = QBLK query pixels of one frame; every neighbour of the frame streams through LDS in chunks of CH.
// norm = 1: the bilateral normaliser pass (nb_in.w == 1) -> nbn; d = d0.  norm = 0: one mean-field update.
// last = 1: write labels (and q1); else the next pass's inputs nb_out (r', g', b', n_b v) and ug (n_g v), v = 2Q(1) - 1.
template <int W>
__global__ __launch_bounds__(TPB) void crf_bilateral_kernel(const float4* __restrict__ nb_in, float4* __restrict__ nb_out,
                                                            CrfScratch s, float sa, float cg, float w1, float w2, int norm,
                                                            int last, uint8_t* __restrict__ labels, float* __restrict__ q1) {
    constexpr int N = W * W, BPF = N / QBLK;
    static_assert(N % QBLK == 0 && N % CH == 0 && CH % W == 0, "tile shape");
    __shared__ float4 nbs[CH];
    __shared__ float tap[W];
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x / BPF;
    const int q0 = (int)(blockIdx.x % BPF) * QBLK;
    const int64_t fo = f * N;
    const float4* src = nb_in + fo;
    if (tid < W) tap[tid] = gauss_tap(tid, cg);

    float qx[QPT], qy[QPT], qr[QPT], qg[QPT], qb[QPT], acc[QPT];
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int p = q0 + k * TPB + tid;
        const float4 c = src[p];
        qx[k] = (float)(p % W) * sa; qy[k] = (float)(p / W) * sa;
        qr[k] = c.x; qg[k] = c.y; qb[k] = c.z;
        acc[k] = 0.f;
    }
    for (int c0 = 0; c0 < N; c0 += CH) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CH / TPB; ++k) nbs[k * TPB + tid] = src[c0 + k * TPB + tid];
        __syncthreads();
        float part[QPT];
#pragma unroll
        for (int k = 0; k < QPT; ++k) part[k] = 0.f;
        for (int r = 0; r < CH / W; ++r) {                               // one neighbour row: its dy is fixed
            const float yj = (float)(c0 / W + r) * sa;
            float a0[QPT];
#pragma unroll
            for (int k = 0; k < QPT; ++k) { const float dy = qy[k] - yj; a0[k] = dy * dy; }
            const float4* rowp = nbs + r * W;
#pragma unroll 4
            for (int xj = 0; xj < W; ++xj) {
                const float4 n = rowp[xj];
                const float xs = (float)xj * sa;
#pragma unroll
                for (int k = 0; k < QPT; ++k) {
                    const float dx = qx[k] - xs, dr = qr[k] - n.x, dg = qg[k] - n.y, db = qb[k] - n.z;
                    float a = fmaf(dx, dx, a0[k]);
                    a = fmaf(dr, dr, a);
                    a = fmaf(dg, dg, a);
                    a = fmaf(db, db, a);
                    part[k] = fmaf(__builtin_amdgcn_exp2f(-a), n.w, part[k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < QPT; ++k) acc[k] += part[k];
    }
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int p = q0 + k * TPB + tid;
        const int64_t i = fo + p;
        float d = s.d0[i], nb;
        if (norm) {
            nb = 1.0f / sqrtf(acc[k]);
            s.nbn[i] = nb;
        } else {
            nb = s.nbn[i];
            const int x = p % W, y = p / W;
            const float* col = s.tg + fo + x;
            float sg = 0.f;
            for (int yy = 0; yy < W; ++yy) sg = fmaf(tap[y > yy ? y - yy : yy - y], col[(int64_t)yy * W], sg);
            d += w2 * (s.ng[i] * sg) + w1 * (nb * acc[k]);
        }
        const float q = 1.0f / (1.0f + expf(-d));
        if (last) {
            labels[i] = d > 0.f ? 1 : 0;
            if (q1) q1[i] = q;
        } else {
            const float v = 2.0f * q - 1.0f;
            nb_out[i] = make_float4(qr[k], qg[k], qb[k], nb * v);
            s.ug[i] = s.ng[i] * v;
        }
    }
}

template <int W>
int run_crf(int B, const uint8_t* frames, const float* prob1, const cvae_crf_params& p, uint8_t* labels, float* q1,
            void* scratch, hipStream_t st) {
    const int64_t npix = (int64_t)B * W * W;
    const CrfScratch s = carve_crf(scratch, npix);
    // exp(-x^2 / (2 s^2)) = exp2(-(x * sqrt(log2 e / (2 s^2)))^2).  A tiny alpha, beta or gamma sends its scale to +inf, and
    // 0 * inf (pixel 0, colour 0, tap 0) is NaN; a large finite sa is no better, since (qy - y * sa) contracts to an fma that
    // returns the rounding error of qy, whose square then zeroes a pixel's own tap.  The scales stop where exp2 of the
    // smallest nonzero distance is already 0 (2^-256) and that of distance 0 is 1: the identity filter, as in exact
    // arithmetic.  Powers of two, so that coordinate * scale is exact.
    const float sa = fminf(sqrtf(LOG2E / (2.0f * p.alpha * p.alpha)), 16.0f);
    const float sb = fminf(sqrtf(LOG2E / (2.0f * p.beta * p.beta)), 16.0f);
    const float cg = fminf(LOG2E / (2.0f * p.gamma * p.gamma), 256.0f);
    const unsigned pix_blocks = (unsigned)((npix + TPB - 1) / TPB);
    const unsigned crf_blocks = (unsigned)(npix / QBLK);
    hipLaunchKernelGGL(crf_init_kernel, dim3(pix_blocks), dim3(TPB), 0, st, frames, prob1, s, W, npix, sb, cg, p.p_floor);
    CVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(crf_bilateral_kernel<W>, dim3(crf_blocks), dim3(TPB), 0, st, s.nb0, s.nb1, s, sa, cg, p.w1, p.w2,
                       1, p.iterations == 0 ? 1 : 0, labels, q1);
    CVAE_CHECK_LAUNCH();
    float4 *in = s.nb1, *out = s.nb0;
    for (int it = 1; it <= p.iterations; ++it) {
        hipLaunchKernelGGL(crf_gauss_rows_kernel, dim3(pix_blocks), dim3(TPB), 0, st, s.ug, s.tg, W, npix, cg);
        CVAE_CHECK_LAUNCH();
        hipLaunchKernelGGL(crf_bilateral_kernel<W>, dim3(crf_blocks), dim3(TPB), 0, st, in, out, s, sa, cg, p.w1, p.w2,
                           0, it == p.iterations ? 1 : 0, labels, q1);
        CVAE_CHECK_LAUNCH();
        float4* t = in; in = out; out = t;
    }
    return 0;
}

// One workgroup per frame.  u8 = trunc((min(d, mean_max) * diff_factor) * 255) in float64 (prepare_diff + astype(uint8),
// vae_utility.py:148-160, 279-284); mask = u8 > thr; with gt: per-frame (tp, fn, fp) of get_iou(gt, mask) and the 2 x 256
// histograms of u8 (row 0: gt set, row 1: gt clear), added into `hist` with integer atomics (order-free).
__global__ __launch_bounds__(TPB) void diff_normalize_kernel(const float* __restrict__ diff, double mean_max, double factor,
                                                             int thr, const uint8_t* __restrict__ gt, uint8_t* __restrict__ u8,
                                                             uint8_t* __restrict__ mask, int64_t* __restrict__ counts,
                                                             unsigned long long* __restrict__ hist, int N) {
    __shared__ unsigned h[512];
    __shared__ int red[3][TPB];
    const int tid = threadIdx.x;
    const int64_t fo = (int64_t)blockIdx.x * N;
    if (hist) for (int b = tid; b < 512; b += TPB) h[b] = 0;
    __syncthreads();
    int tp = 0, fn = 0, fp = 0;
    for (int p = tid; p < N; p += TPB) {
        double v = (double)diff[fo + p];
        if (v > mean_max) v = mean_max;
        v = v * factor;
        v = v * 255.0;
        int q = (int)v;
        q = q < 0 ? 0 : (q > 255 ? 255 : q);
        u8[fo + p] = (uint8_t)q;
        const int m = q > thr;
        if (mask) mask[fo + p] = (uint8_t)m;
        if (gt) {
            const int g = gt[fo + p] != 0;
            tp += g & m; fn += g & (1 - m); fp += (1 - g) & m;
            if (hist) atomicAdd(&h[(g ? 0 : 256) + q], 1u);
        }
    }
    if (counts) {
        red[0][tid] = tp; red[1][tid] = fn; red[2][tid] = fp;
        __syncthreads();
        for (int o = TPB / 2; o > 0; o >>= 1) {
            if (tid < o) for (int c = 0; c < 3; ++c) red[c][tid] += red[c][tid + o];
            __syncthreads();
        }
        if (tid < 3) counts[blockIdx.x * 3 + tid] = red[tid][0];
    }
    if (hist) {
        __syncthreads();
        for (int b = tid; b < 512; b += TPB)
            if (h[b]) atomicAdd(&hist[b], (unsigned long long)h[b]);
    }
}

// per-frame (tp, fn, fp) of get_iou(gt, mask) (vae_utility.py:56-68) for any uint8 mask (nonzero = set)
__global__ __launch_bounds__(TPB) void mask_counts_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ gt,
                                                          int64_t* __restrict__ counts, int N) {
    __shared__ int red[3][TPB];
    const int tid = threadIdx.x;
    const int64_t fo = (int64_t)blockIdx.x * N;
    int tp = 0, fn = 0, fp = 0;
    for (int p = tid; p < N; p += TPB) {
        const int g = gt[fo + p] != 0, m = mask[fo + p] != 0;
        tp += g & m; fn += g & (1 - m); fp += (1 - g) & m;
    }
    red[0][tid] = tp; red[1][tid] = fn; red[2][tid] = fp;
    __syncthreads();
    for (int o = TPB / 2; o > 0; o >>= 1) {
        if (tid < o) for (int c = 0; c < 3; ++c) red[c][tid] += red[c][tid + o];
        __syncthreads();
    }
    if (tid < 3) counts[blockIdx.x * 3 + tid] = red[tid][0];
}

}  // namespace

int64_t crf_scratch_bytes(int width, int B) {
    const int64_t npix = (int64_t)B * width * width;
    return 2 * align256(npix * 16) + 5 * align256(npix * 4);
}

int launch_dense_crf(int width, int B, const uint8_t* frames, const float* prob1, const cvae_crf_params& p,
                     uint8_t* labels, float* q1, void* scratch, hipStream_t st) {
    if (width == 64) return run_crf<64>(B, frames, prob1, p, labels, q1, scratch, st);
    return run_crf<128>(B, frames, prob1, p, labels, q1, scratch, st);
}

int launch_diff_normalize(int width, int B, const float* diff, double mean_max, double factor, int thr, const uint8_t* gt,
                          uint8_t* u8, uint8_t* mask, int64_t* counts, int64_t* hist, hipStream_t st) {
    hipLaunchKernelGGL(diff_normalize_kernel, dim3((unsigned)B), dim3(TPB), 0, st, diff, mean_max, factor, thr, gt, u8, mask,
                       counts, (unsigned long long*)hist, width * width);
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_mask_counts(int width, int B, const uint8_t* mask, const uint8_t* gt, int64_t* counts, hipStream_t st) {
    hipLaunchKernelGGL(mask_counts_kernel, dim3((unsigned)B), dim3(TPB), 0, st, mask, gt, counts, width * width);
    CVAE_CHECK_LAUNCH();
    return 0;
}
