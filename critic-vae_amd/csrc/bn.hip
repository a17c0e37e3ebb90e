// bn.hip — train-mode BatchNorm2d + MaxPool2d(2) + ReLU/Tanh, forward and backward, NHWC.
//
// Replaces the ATen chain nn.BatchNorm2d -> nn.MaxPool2d(2) -> nn.ReLU / nn.Tanh of the four
// encoder blocks (vae_nets.py:70-72, 75-77, 80-82, 85-87) and its autograd (vae.py:57).
// All of it is HBM-bound elementwise / reduction work; every reduction is two fixed-order
// stages (per-workgroup partials, then a finalize kernel) -> bitwise reproducible.
//
// forward : conv epilogue emits per-tile (sum, M2) -> bn_fwd_finalize merges them in fp64
//           (Chan) into coef[c] = {scale, shift, mean, invstd} and updates the running stats
//           (momentum 0.1, unbiased variance) -> bn_pool_act_fwd applies scale/shift, takes the
//           2x2 max (first maximum in scan order, like ATen) and the activation.
// backward: g = da * act'(a) lives only at each window's argmax (recomputed from y), so
//           sum(g) and sum(g*xhat) run over pooled pixels; dy = scale*(g - mean(g) - xhat*mean(g*xhat)).
//
// y, a, da, dy are fp32 or bf16 in HBM (precision mode 1); statistics, coefficients and partial sums stay fp32.  Each
// elementwise pass is ONE kernel template over the storage type (Act<AT>, common.h): bn_pool_act_fwd_kernel<AT, ACT>,
// bn_bwd_kernel<AT, ACT, MODE>, bn_bwd_stats_relu_kernel<AT>.  The types differ only in the channels a thread owns
// (BnWidth<AT>) and in the access that loads them; mapping, summation order, tie rule and rounding points are shared.
#include "common.h"

struct BnGeom { int C, H, act; };                       // act: 0 relu, 1 tanh
static inline BnGeom bn_geom(int layer, int width) {
    const int s = width / 64;
    return BnGeom{kLayers[layer].cout, kLayers[layer].h * s, layer == 3 ? 1 : 0};
}
// geometry of the BatchNorm partials a layer's conv kernel emits: E1 (layer 0) reports one partial per
// 16x32-pixel strip (conv_thin.hip), the others one per 128-pixel tile of Tile<H> (conv_epilogue.h; tile_geom, common.h)
static inline void part_geom(int layer, int H, int* imgs, int* pxPerImg, int* tilesPerImg) {
    if (layer == 0) { *imgs = 1; *pxPerImg = 512; *tilesPerImg = (H / 16) * (H / 32); return; }
    const TileGeom t = tile_geom(H);
    *imgs = t.IMGS; *pxPerImg = t.PX_PER_IMG; *tilesPerImg = t.TILES_PER_IMG;
}
int bn_num_tiles(int layer, int width, int B) {
    const BnGeom g = bn_geom(layer, width);
    int imgs, ppi, tpi;
    part_geom(layer, g.H, &imgs, &ppi, &tpi);
    return cdiv(B, imgs) * tpi;
}

// stage A: mid[ra][{S,Q,M}][c] (fp64) over the tiles of chunk ra; grid (C/32, RA)
__global__ __launch_bounds__(256) void bn_fwd_reduce_kernel(const float* __restrict__ part, int numTiles, int C, int B,
                                                            int imgsPerTile, int pxPerImg, int tilesPerImg,
                                                            double* __restrict__ mid, int tilesPerBlk) {
    __shared__ double red[3][8][32];
    const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    const int t0 = blockIdx.y * tilesPerBlk;
    int t1 = t0 + tilesPerBlk; if (t1 > numTiles) t1 = numTiles;
    double S = 0.0, Q = 0.0, M = 0.0;
#pragma unroll 4
    for (int t = t0 + rg; t < t1; t += 8) {
        const int img0 = (t / tilesPerImg) * imgsPerTile;
        int ni = B - img0; if (ni > imgsPerTile) ni = imgsPerTile;
        const double n = (double)(ni * pxPerImg);
        const double s = (double)part[(size_t)t * C + c];
        S += s; Q += s * s / n; M += (double)part[((size_t)numTiles + t) * C + c];
    }
    red[0][rg][cl] = S; red[1][rg][cl] = Q; red[2][rg][cl] = M;
    __syncthreads();
    if (rg == 0) {
        for (int k = 1; k < 8; ++k) { S += red[0][k][cl]; Q += red[1][k][cl]; M += red[2][k][cl]; }
        double* o = mid + (size_t)blockIdx.y * 3 * C;
        o[c] = S; o[C + c] = Q; o[2 * C + c] = M;
    }
}

// (S, Q, M) of channel c -> coef[c] = {scale, shift, mean, invstd} and the running-stat update (train), or coef from the
// running stats (eval).  Shared by the single-rank finalize and the finish step of the cross-rank path.
__device__ __forceinline__ void bn_fwd_coef(int c, double S, double Q, double M, double N, const float* __restrict__ gamma,
                                            const float* __restrict__ beta, float* __restrict__ run_mean,
                                            float* __restrict__ run_var, float* __restrict__ coef, int train) {
    float mean, var;
    if (train) {
        const double mu = S / N;
        double v = (M + Q - S * S / N) / N;          // biased variance
        if (v < 0.0) v = 0.0;
        mean = (float)mu; var = (float)v;
        const float uvar = (float)(v * N / (N - 1.0));
        {   // two roundings, never an fma: the value must not depend on how the compiler contracts it in each kernel
#pragma clang fp contract(off)
            run_mean[c] = 0.9f * run_mean[c] + 0.1f * mean;
            run_var[c] = 0.9f * run_var[c] + 0.1f * uvar;
        }
    } else {
        mean = run_mean[c]; var = run_var[c];
    }
    const float invstd = 1.0f / sqrtf(var + 1e-5f);
    const float scale = gamma[c] * invstd;
    coef[c * 4 + 0] = scale;
    coef[c * 4 + 1] = beta[c] - mean * scale;
    coef[c * 4 + 2] = mean;
    coef[c * 4 + 3] = invstd;
}

// The RA chunk sums of channel c merged in fp64: lane r of 32 loads chunk r (RA <= 32), then a fixed xor-shuffle tree;
// every lane ends with the sums.  The single-rank finalize and the cross-rank record both merge here, so that one rank
// without an exchange reproduces the single-call step bit for bit.
struct BnSums { double S, Q, M; };
__device__ __forceinline__ BnSums bn_fwd_merge(const double* __restrict__ mid, int RA, int C, int c, int r) {
    BnSums s{0.0, 0.0, 0.0};
    if (r < RA) { s.S = mid[(size_t)r * 3 * C + c]; s.Q = mid[(size_t)r * 3 * C + C + c]; s.M = mid[(size_t)r * 3 * C + 2 * C + c]; }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) { s.S += __shfl_xor(s.S, o, 64); s.Q += __shfl_xor(s.Q, o, 64); s.M += __shfl_xor(s.M, o, 64); }
    return s;
}

// stage B: merge the RA chunk sums, emit coef[c] = {scale, shift, mean, invstd}, update running stats.  32 lanes per
// channel, two channels per wave.  Eval mode (train == 0): mid is not read, coef comes from the running statistics.
__global__ __launch_bounds__(64) void bn_fwd_finalize_kernel(const double* __restrict__ mid, int RA, int C, double N,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float* __restrict__ run_mean, float* __restrict__ run_var,
                                                             float* __restrict__ coef, int train) {
    const int c = blockIdx.x * 2 + (threadIdx.x >> 5), r = threadIdx.x & 31;
    const BnSums s = bn_fwd_merge(mid, train ? RA : 0, C, c, r);
    if (r != 0) return;
    bn_fwd_coef(c, s.S, s.Q, s.M, N, gamma, beta, run_mean, run_var, coef, train);
}

// Cross-rank path, record step: the same merge, written to this layer's slot of the sync record as rec[c] = S,
// rec[C + c] = Q, rec[2C + c] = M (fp64).  Every term is a sum over tiles, so the records of several ranks add up to the
// record of their union.  count != null: also *count = this rank's image count.
__global__ __launch_bounds__(64) void bn_fwd_record_kernel(const double* __restrict__ mid, int RA, int C, double* __restrict__ rec,
                                                           double* __restrict__ count, double images) {
    const int c = blockIdx.x * 2 + (threadIdx.x >> 5), r = threadIdx.x & 31;
    const BnSums s = bn_fwd_merge(mid, RA, C, c, r);
    if (r != 0) return;
    rec[c] = s.S; rec[C + c] = s.Q; rec[2 * C + c] = s.M;
    if (count && c == 0) *count = images;
}

// Cross-rank path, finish step: coef and the running statistics from the summed record; N = (summed image count) * H * H,
// so the running variance takes the global N / (N - 1).  One thread per channel.
__global__ __launch_bounds__(64) void bn_fwd_finish_kernel(const double* __restrict__ rec, const double* __restrict__ count, int C, int H,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ run_mean, float* __restrict__ run_var,
                                                           float* __restrict__ coef) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const double N = count[0] * H * H;
    bn_fwd_coef(c, rec[c], rec[C + c], rec[2 * C + c], N, gamma, beta, run_mean, run_var, coef, 1);
}

__device__ __forceinline__ float act_fwd(float v, int act) { return act ? tanhf(v) : fmaxf(v, 0.f); }
__device__ __forceinline__ float act_bwd_from_out(float a, int act) { return act ? (1.f - a * a) : (a > 0.f ? 1.f : 0.f); }

// Channels a thread owns in the elementwise passes, per activation storage type (Act<AT>, common.h).  W: forward and
// ReLU statistics, one 16-byte access per tensor row.  WB: backward; its fp32 form stays on per-lane scalar accesses
// coalesced across the wave.  A::Vec<V> holds the stored form: elements widen to fp32 before any arithmetic ((float)v[e])
// and round once where the result is packed (v[e] = (AT)x), whatever the type.
template <typename AT> struct BnWidth;
template <> struct BnWidth<float> { static constexpr int W = 4, WB = 1; };
template <> struct BnWidth<__bf16> { static constexpr int W = 8, WB = 8; };

// element offset of channel 0 of the first pixel of pooled pixel pp's 2x2 window, and of window pixel p from there
// (frame sizes are powers of two: no 64-bit divisions in the pixel loops)
__device__ __forceinline__ size_t window_base(int64_t pp, int H, int C) {
    const int HO = H / 2, hsh = 31 - __builtin_clz(HO);
    const int px = (int)(pp & (HO - 1)), py = (int)((pp >> hsh) & (HO - 1));
    const int64_t ib = pp >> (2 * hsh);
    return (size_t)((ib * H + 2 * py) * H + 2 * px) * C;
}
__device__ __forceinline__ size_t window_px(int p, int H, int C) { return (size_t)((p >> 1) * H + (p & 1)) * C; }

// one channel of a window: position of the first maximum of the normalised values in scan order (like ATen); returns y there
__device__ __forceinline__ float window_argmax(const float (&yy)[4], float sc, float sh, int* pos) {
    float m = 0.f, ym = 0.f;
    *pos = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float n = fmaf(yy[p], sc, sh);
        if (p == 0 || n > m) { m = n; *pos = p; ym = yy[p]; }
    }
    return ym;
}

template <typename AT, int ACT>
__global__ __launch_bounds__(256) void bn_pool_act_fwd_kernel(const float* __restrict__ y, const float* __restrict__ coef,
                                                              float* __restrict__ a, int C, int H, int64_t total) {
    using A = Act<AT>;
    constexpr int V = BnWidth<AT>::W;
    // grid-stride over (pooled pixel, channel group): the stride (gridDim * 256) is a multiple of C/V, so a thread keeps its
    // channel group — scale / shift are loaded once per thread instead of once per output (fp32: 8 extra loads beside 4 + 1
    // useful accesses, 4.6 TB/s against 5.6-5.9 for the backward apply pass); channel counts are powers of two
    const int CV = C / V, csh = 31 - __builtin_clz(CV);
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const int cv = (int)(first & (CV - 1));
    float sc[V], sh[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { const float2 cf = *reinterpret_cast<const float2*>(coef + (cv * V + e) * 4); sc[e] = cf.x; sh[e] = cf.y; }
    for (int64_t idx = first; idx < total; idx += stride) {
        const int64_t pp = idx >> csh;
        const size_t base = window_base(pp, H, C) + cv * V;
        typename A::template Vec<V> yv[4], o;
#pragma unroll
        for (int p = 0; p < 4; ++p) yv[p] = A::template ldv<V>(y, base + window_px(p, H, C));
        float m[V];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float n = fmaf((float)yv[p][e], sc[e], sh[e]);
                m[e] = (p == 0 || n > m[e]) ? n : m[e];
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = (AT)act_fwd(m[e], ACT);
        A::template stv<V>(a, (size_t)pp * C + cv * V, o);
    }
}

// Backward over the pooled pixels: g = da*act'(a) at the window argmax (recomputed from y).
// MODE 0: partial sums (sum g, sum g*xhat) per channel.  MODE 1: write dy, partial sums of dy.
template <typename AT, int ACT, int MODE>
__global__ __launch_bounds__(256) void bn_bwd_kernel(const float* __restrict__ y, const float* __restrict__ a,
                                                     const float* __restrict__ da, const float* __restrict__ coef,
                                                     const float* __restrict__ bcoef, float* __restrict__ dy,
                                                     float* __restrict__ part, int C, int H, int64_t totalPx, int64_t pxPerBlk) {
    using A = Act<AT>;
    constexpr int V = BnWidth<AT>::WB;
    __shared__ float red[2][256][V];
    const int CV = C / V, cv = threadIdx.x % CV, sub = threadIdx.x / CV, NSUB = 256 / CV;     // C / V <= 256, divides 256
    float sc[V], sh[V], mean[V], invstd[V], k1[V], k2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const int c = cv * V + e;
        sc[e] = coef[c * 4]; sh[e] = coef[c * 4 + 1]; mean[e] = coef[c * 4 + 2]; invstd[e] = coef[c * 4 + 3];
        k1[e] = MODE == 1 ? bcoef[c * 2] : 0.f; k2[e] = MODE == 1 ? bcoef[c * 2 + 1] : 0.f;
    }
    const int64_t p0 = blockIdx.x * pxPerBlk;
    int64_t p1 = p0 + pxPerBlk; if (p1 > totalPx) p1 = totalPx;
    float acc0[V], acc1[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
    for (int64_t pp = p0 + sub; pp < p1; pp += NSUB) {
        const size_t base = window_base(pp, H, C) + cv * V;
        typename A::template Vec<V> yv[4], out[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) yv[p] = A::template ldv<V>(y, base + window_px(p, H, C));
        const auto av = A::template ldv<V>(a, (size_t)pp * C + cv * V), gv = A::template ldv<V>(da, (size_t)pp * C + cv * V);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float yy[4] = {(float)yv[0][e], (float)yv[1][e], (float)yv[2][e], (float)yv[3][e]};
            int pos;
            const float ym = window_argmax(yy, sc[e], sh[e], &pos);
            const float g = (float)gv[e] * act_bwd_from_out((float)av[e], ACT);
            if (MODE == 0) {
                acc0[e] += g; acc1[e] += g * ((ym - mean[e]) * invstd[e]);
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const float xhat = (yy[p] - mean[e]) * invstd[e];
                    const float d = sc[e] * ((p == pos ? g : 0.f) - k1[e] - xhat * k2[e]);
                    out[p][e] = (AT)d;
                    acc0[e] += d;
                }
            }
        }
        if (MODE == 1) {
#pragma unroll
            for (int p = 0; p < 4; ++p) A::template stv<V>(dy, base + window_px(p, H, C), out[p]);
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) { red[0][threadIdx.x][e] = acc0[e]; red[1][threadIdx.x][e] = acc1[e]; }
    __syncthreads();
    if (sub == 0) {
        for (int k = 1; k < NSUB; ++k)
#pragma unroll
            for (int e = 0; e < V; ++e) { acc0[e] += red[0][k * CV + cv][e]; acc1[e] += red[1][k * CV + cv][e]; }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int c = cv * V + e;
            if (MODE == 0) {
                part[((size_t)blockIdx.x * 2) * C + c] = acc0[e];
                part[((size_t)blockIdx.x * 2 + 1) * C + c] = acc1[e];
            } else {
                part[(size_t)blockIdx.x * C + c] = acc0[e];
            }
        }
    }
}

// ReLU blocks: the two backward sums need only the POOLED tensors.  g = da*[a>0]; at the window argmax
// the normalised value is n = a (ReLU passed it through), and xhat = (n - beta)/gamma, so
// sum(g) and sum(g*xhat) never touch the full-resolution y (3x less traffic than bn_bwd_kernel<AT, 0, 0>).
// Channels whose |gamma| is small (< 1e-2; exactly 0 and NaN included) cannot use that shortcut — the division
// amplifies the rounding of a by 1/|gamma| and is undefined at 0 — and take xhat from y at the recomputed
// argmax instead (the bn_bwd_kernel<AT, 0, 0> formula), so dgamma stays correct and such a channel can recover.
template <typename AT>
__global__ __launch_bounds__(256) void bn_bwd_stats_relu_kernel(const float* __restrict__ y, const float* __restrict__ a,
                                                                const float* __restrict__ da, const float* __restrict__ coef,
                                                                const float*, float*,           // bcoef, dy: bn_bwd_kernel's parameter list
                                                                float* __restrict__ part, int C, int H, int64_t totalPx, int64_t pxPerBlk) {
    using A = Act<AT>;
    constexpr int V = BnWidth<AT>::W;
    __shared__ float red[2][256][V];
    const int CV = C / V, cv = threadIdx.x % CV, sub = threadIdx.x / CV, NSUB = 256 / CV;
    float gam[V], bet[V];
    bool tiny[V], any_tiny = false;
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const int c = cv * V + e;
        const float scale = coef[c * 4], shift = coef[c * 4 + 1], mean = coef[c * 4 + 2], invstd = coef[c * 4 + 3];
        const float g = scale / invstd;                       // gamma
        tiny[e] = !(fabsf(g) >= 1e-2f);
        any_tiny = any_tiny || tiny[e];
        gam[e] = tiny[e] ? 0.f : 1.0f / g;
        bet[e] = shift + mean * scale;                        // beta
    }
    const int64_t p0 = blockIdx.x * pxPerBlk;
    int64_t p1 = p0 + pxPerBlk; if (p1 > totalPx) p1 = totalPx;
    float s1[V], s2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
    for (int64_t pp = p0 + sub; pp < p1; pp += NSUB) {
        const auto av = A::template ldv<V>(a, (size_t)pp * C + cv * V), gv = A::template ldv<V>(da, (size_t)pp * C + cv * V);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float aa = (float)av[e];
            const float g = aa > 0.f ? (float)gv[e] : 0.f;
            s1[e] += g;
            s2[e] += g * ((aa - bet[e]) * gam[e]);
        }
        if (any_tiny) {
            const size_t base = window_base(pp, H, C);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if (!tiny[e]) continue;
                const int c = cv * V + e;
                float yy[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) yy[p] = A::ld(y, base + window_px(p, H, C) + c);
                int pos;
                const float ym = window_argmax(yy, coef[c * 4], coef[c * 4 + 1], &pos);
                s2[e] += ((float)av[e] > 0.f ? (float)gv[e] : 0.f) * ((ym - coef[c * 4 + 2]) * coef[c * 4 + 3]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) { red[0][threadIdx.x][e] = s1[e]; red[1][threadIdx.x][e] = s2[e]; }
    __syncthreads();
    if (sub == 0) {
        for (int k = 1; k < NSUB; ++k)
#pragma unroll
            for (int e = 0; e < V; ++e) { s1[e] += red[0][k * CV + cv][e]; s2[e] += red[1][k * CV + cv][e]; }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            part[((size_t)blockIdx.x * 2) * C + cv * V + e] = s1[e];
            part[((size_t)blockIdx.x * 2 + 1) * C + cv * V + e] = s2[e];
        }
    }
}

// rows[r] = [sum g | sum g*xhat] partials (R <= 64 rows left by launch_col_reduce_partial), summed
// here in fixed order -> dgamma, dbeta, bcoef = (s1/N, s2/N).  REC (cross-rank path): rec[c] = s1, rec[C + c] = s2
// (fp64) instead of bcoef; dgamma / dbeta stay this rank's own (the gradient all-reduce sums them).
template <bool REC>
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ rows, int R, int64_t stride, int C, float invN,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ bcoef,
                                                              double* __restrict__ rec) {
    // 16 lanes per channel: lane q adds rows q, q+16, q+32, q+48, then a fixed xor-shuffle tree
    const int c = blockIdx.x * 16 + (threadIdx.x >> 4), q = threadIdx.x & 15;
    float s1 = 0.f, s2 = 0.f;
    if (c < C)
        for (int r = q; r < R; r += 16) { s1 += rows[(size_t)r * stride + c]; s2 += rows[(size_t)r * stride + C + c]; }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    if (c < C && q == 0) {
        dgamma[c] = s2; dbeta[c] = s1;
        if (REC) { rec[c] = (double)s1; rec[C + c] = (double)s2; }
        else { bcoef[c * 2] = s1 * invN; bcoef[c * 2 + 1] = s2 * invN; }
    }
}

// cross-rank path: bcoef from the summed record with the global 1/N, N = (summed image count) * H * H.  invN is the
// correctly rounded fp32 1 / (float)N, as the single-rank launcher computes it on the host (a double quotient of two
// floats rounds to the same float: 53 >= 2 * 24 + 2 bits), so that one rank reproduces it bit for bit.
__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const double* __restrict__ rec, const double* __restrict__ count, int C, int H,
                                                            float* __restrict__ bcoef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float invN = (float)(1.0 / (double)(float)(count[0] * H * H));
    bcoef[c * 2] = (float)rec[c] * invN;
    bcoef[c * 2 + 1] = (float)rec[C + c] * invN;
}

static constexpr int BN_RA = 32;
int64_t bn_fwd_ws_floats(int layer, int width) { (void)width; return (int64_t)2 * BN_RA * 3 * kLayers[layer].cout; }

// stage A of the forward statistics: the RA chunk rows of fp64 (S, Q, M) in `ws`; returns RA
static int bn_fwd_reduce(int layer, int width, int B, const float* bnpart, float* ws, hipStream_t st, int tilesPerPartial, int* RA_out) {
    const BnGeom g = bn_geom(layer, width);
    int imgs, ppi, tpi;
    part_geom(layer, g.H, &imgs, &ppi, &tpi);
    int numTiles = cdiv(B, imgs) * tpi;
    if (tilesPerPartial > 1) {           // conv_bf16_big.hip: one partial per T = 4 / 8 consecutive 128-pixel tiles (T a power of two)
        const int T = tilesPerPartial;
        numTiles = cdiv(numTiles, T);
        if (tpi >= T) { ppi *= T; tpi /= T; }                          // a part of an image
        else if (tpi > 1) { imgs = T / tpi; ppi *= tpi; tpi = 1; }      // T / tpi whole images (a tile is at most one image while tpi > 1)
        else imgs *= T;                                                 // T x imgs whole images
    }
    double* mid = reinterpret_cast<double*>(ws);
    const int tpb = cdiv(numTiles, BN_RA);
    const int RA = cdiv(numTiles, tpb);
    hipLaunchKernelGGL(bn_fwd_reduce_kernel, dim3(g.C / 32, RA), dim3(256), 0, st, bnpart, numTiles, g.C, B, imgs,
                       ppi, tpi, mid, tpb);
    CVAE_CHECK_LAUNCH();
    *RA_out = RA;
    return 0;
}

int launch_bn_fwd_finalize(int layer, int width, int B, const float* bnpart, const float* gamma, const float* beta,
                           float* run_mean, float* run_var, float* coef, float* ws, int train, hipStream_t st, int tilesPerPartial) {
    const BnGeom g = bn_geom(layer, width);
    double* mid = reinterpret_cast<double*>(ws);
    int RA = 0;
    if (train) { int rc = bn_fwd_reduce(layer, width, B, bnpart, ws, st, tilesPerPartial, &RA); if (rc) return rc; }
    hipLaunchKernelGGL(bn_fwd_finalize_kernel, dim3(g.C / 2), dim3(64), 0, st, mid, RA, g.C,
                       (double)B * g.H * g.H, gamma, beta, run_mean, run_var, coef, train);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// cross-rank path (train mode): this rank's (S, Q, M) into rec[0, 3C) (+ its image count into *count when count != null) ...
int launch_bn_fwd_record(int layer, int width, int B, const float* bnpart, float* ws, hipStream_t st, int tilesPerPartial,
                         double* rec, double* count) {
    const BnGeom g = bn_geom(layer, width);
    int RA = 0;
    { int rc = bn_fwd_reduce(layer, width, B, bnpart, ws, st, tilesPerPartial, &RA); if (rc) return rc; }
    hipLaunchKernelGGL(bn_fwd_record_kernel, dim3(g.C / 2), dim3(64), 0, st, reinterpret_cast<const double*>(ws), RA, g.C,
                       rec, count, (double)B);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// ... and, once the caller has summed rec and count over the ranks, coef + running statistics from the sums
int launch_bn_fwd_finish(int layer, int width, const double* rec, const double* count, const float* gamma, const float* beta,
                         float* run_mean, float* run_var, float* coef, hipStream_t st) {
    const BnGeom g = bn_geom(layer, width);
    hipLaunchKernelGGL(bn_fwd_finish_kernel, dim3(cdiv(g.C, 64)), dim3(64), 0, st, rec, count, g.C, g.H, gamma, beta,
                       run_mean, run_var, coef);
    CVAE_CHECK_LAUNCH();
    return 0;
}

template <typename AT, int ACT>
static int bn_pool_act_fwd(const BnGeom& g, int B, const float* y, const float* coef, float* a, hipStream_t st) {
    const int64_t total = (int64_t)B * (g.H / 2) * (g.H / 2) * (g.C / BnWidth<AT>::W);
    const int64_t want = (int64_t)cvae_num_cus() * 16;                  // grid-stride: 16 workgroups per CU
    const unsigned grid = (unsigned)((total + 255) / 256 < want ? (total + 255) / 256 : want);
    hipLaunchKernelGGL((bn_pool_act_fwd_kernel<AT, ACT>), dim3(grid), dim3(256), 0, st, y, coef, a, g.C, g.H, total);
    CVAE_CHECK_LAUNCH();
    return 0;
}
int launch_bn_pool_act_fwd(int layer, int width, int B, const float* y, const float* coef, float* a, hipStream_t st, bool bf16io) {
    const BnGeom g = bn_geom(layer, width);
    if (bf16io) return g.act ? bn_pool_act_fwd<__bf16, 1>(g, B, y, coef, a, st) : bn_pool_act_fwd<__bf16, 0>(g, B, y, coef, a, st);
    return g.act ? bn_pool_act_fwd<float, 1>(g, B, y, coef, a, st) : bn_pool_act_fwd<float, 0>(g, B, y, coef, a, st);
}

static inline int bn_bwd_blocks(int64_t totalPx, int C) {
    const int nsub = 256 / C;
    int64_t nb = totalPx / (nsub * 8);          // >= 8 pixels per thread
    if (nb > 1024) nb = 1024;
    if (nb < 1) nb = 1;
    return (int)nb;
}
int64_t bn_bwd_ws_floats(int layer, int width, int B) {
    const BnGeom g = bn_geom(layer, width);
    const int64_t totalPx = (int64_t)B * (g.H / 2) * (g.H / 2);
    return (int64_t)bn_bwd_blocks(totalPx, g.C) * 2 * g.C + 4 * g.C + col_reduce_ws_floats(2 * g.C);
}

const float* bn_bwd_bcoef(int layer, int width, int B, const float* ws) {
    const BnGeom g = bn_geom(layer, width);
    return ws + (size_t)bn_bwd_blocks((int64_t)B * (g.H / 2) * (g.H / 2), g.C) * 2 * g.C;
}

// the two elementwise kernels of a backward, for one (storage type, activation): all take bn_bwd_kernel's parameters
using BnBwdKernel = void (*)(const float*, const float*, const float*, const float*, const float*, float*, float*, int, int, int64_t, int64_t);
struct BnBwdKernels { BnBwdKernel stats, apply; };
template <typename AT, int ACT>
static BnBwdKernels bn_bwd_kernels() {
    if constexpr (ACT == 0) return {bn_bwd_stats_relu_kernel<AT>, bn_bwd_kernel<AT, 0, 1>};
    else return {bn_bwd_kernel<AT, ACT, 0>, bn_bwd_kernel<AT, ACT, 1>};
}

// dy == nullptr: statistics only (dgamma, dbeta and the (k1, k2) pair at bn_bwd_bcoef(ws)); the caller's next kernel
// applies the backward itself (block 0: launch_e1_wgrad's fused staging).
// stage (cross-rank path): 0 = everything above; 1 = the statistics only, dgamma / dbeta plus this rank's (sum g, sum g*xhat)
// into rec[0, 2C) instead of (k1, k2); 2 = (k1, k2) from the summed rec and *count (the summed image count), then the
// apply pass (dy != null) as stage 0 runs it.  Stages 1 and 2 run on the same ws, batch and tensors, in that order.
int launch_bn_pool_act_bwd(int layer, int width, int B, const float* y, const float* a, const float* da,
                           const float* coef, const float* gamma, float* dy, float* dgamma, float* dbeta,
                           float* dbias, float* ws, hipStream_t st, bool bf16io, int stage, double* rec, const double* count) {
    (void)gamma;
    const BnGeom g = bn_geom(layer, width);
    const int64_t totalPx = (int64_t)B * (g.H / 2) * (g.H / 2);
    const int nblk = bn_bwd_blocks(totalPx, g.C);
    const int64_t ppb = (totalPx + nblk - 1) / nblk;
    float* part = ws;
    float* bcoef = ws + (size_t)nblk * 2 * g.C;
    float* red = bcoef + 2 * g.C;
    float* crws = red + 2 * g.C;
    const float invN = 1.0f / (float)((double)B * g.H * g.H);
    const BnBwdKernels k = bf16io ? (g.act ? bn_bwd_kernels<__bf16, 1>() : bn_bwd_kernels<__bf16, 0>())
                                  : (g.act ? bn_bwd_kernels<float, 1>() : bn_bwd_kernels<float, 0>());
    if (stage != 2) {
        hipLaunchKernelGGL(k.stats, dim3(nblk), dim3(256), 0, st, y, a, da, coef, nullptr, nullptr, part, g.C, g.H, totalPx, ppb);
        CVAE_CHECK_LAUNCH();
        const float* rows; int R; int64_t rstride;
        { int rc = launch_col_reduce_partial(part, nblk, 2 * g.C, 2 * g.C, crws, st, &rows, &R, &rstride); if (rc) return rc; }
        if (stage == 1) hipLaunchKernelGGL(bn_bwd_finalize_kernel<true>, dim3(cdiv(g.C, 16)), dim3(256), 0, st, rows, R, rstride, g.C, invN, dgamma, dbeta, nullptr, rec);
        else hipLaunchKernelGGL(bn_bwd_finalize_kernel<false>, dim3(cdiv(g.C, 16)), dim3(256), 0, st, rows, R, rstride, g.C, invN, dgamma, dbeta, bcoef, nullptr);
        CVAE_CHECK_LAUNCH();
        if (stage == 1) return 0;
    } else {
        hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(cdiv(g.C, 256)), dim3(256), 0, st, rec, count, g.C, g.H, bcoef);
        CVAE_CHECK_LAUNCH();
    }
    if (!dy) {
        if (dbias) { cvae_set_error("bn_bwd: dbias needs the apply pass (dy)"); return -2; }
        return 0;
    }
    cvae_probe_begin(st);                       // the apply pass: reads y, a, da, writes dy — the step's largest HBM-bound kernel
    hipLaunchKernelGGL(k.apply, dim3(nblk), dim3(256), 0, st, y, a, da, coef, bcoef, dy, part, g.C, g.H, totalPx, ppb);
    cvae_probe_end(st);
    CVAE_CHECK_LAUNCH();
    if (dbias) return launch_col_reduce(part, nblk, g.C, g.C, dbias, crws, st);   // else: the wgrad kernel provides it
    return 0;
}
