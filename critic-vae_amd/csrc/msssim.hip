// msssim.hip — fused MS-SSIM pyramid loss + KLD, forward and backward, on NCHW planes.
//
// Replaces MSSIM.forward / MSSIM.ssim (vae_nets.py:181-247: per level 5 depthwise 11x11
// F.conv2d + ~12 elementwise ATen ops + 2 means + avg_pool2d, window rebuilt on every call),
// the KLD of VariationalAutoencoder.vae_loss (vae_nets.py:57-60) and their autograd.
//
// Semantics kept exactly: the window is exp(+d^2/2s^2)/sum ("anti-Gaussian",
// vae_nets.py:171), zero padding 5 at every level, C1=1e-4, C2=9e-4, GLOBAL means over
// B*3*H*W, final 1 - prod_{l<4}(cs_l^w_l * ssim_4^w_4); negative cs -> NaN, no clamping.
// The 2-D window is the outer product of the 1-D one (vae_nets.py:176-177) so the filter is run
// as 11+11 taps (summation order differs from the 121-tap ATen conv by ~1e-7 relative).
//
// Structure (round 2): the loss is L = 1 - prod(mean_l ^ w_l), so dL/dx_l = coef_l * F_l with
//   F_l = win * u_mu + 2 x (win * u_11) + y (win * u_12),   u_* = d map_l / d (mu1, E[x^2], E[xy])
// where only the scalar coef_l depends on the global means.  ONE forward kernel per level computes the five
// filtered maps on the whole plane (streamed in bands at 128 wide), the SSIM/CS partial sums, the
// three derivative maps in LDS (never in HBM), filters them again and stores the single field F_l plus the
// 2x2 average for the next level.  Levels 16/8/4 run in one launch (one workgroup per plane, everything in
// LDS).  The finalize runs on 32 workgroups; the last one to arrive (release/acquire ticket) merges their
// fp64 partials in a fixed order, evaluates the loss, the KLD (+ its gradients) and the five coefficients.
// The backward is ONE elementwise pass: dx = c0 F0 + 1/4 up(c1 F1 + 1/4 up(c2 F2 + ...)) (avg_pool2d backward).
// HBM traffic: forward reads x, y once and writes F (+ 1/4-size pyramids); backward reads the F pyramid and
// writes dx — 1.2x the algorithmic bytes (was 3.2x / 2.5x with the derivative maps stored).
#include "common.h"
#include "msssim_finish.h"
#include <math.h>

// The 11 normalised taps travel BY VALUE in every kernel's argument struct (scalar registers): no
// __constant__ symbol, no upload, no process-global device state — handles on different devices are
// independent and nothing here synchronises.  gaussian_window (vae_nets.py:169-173): fp32 exp, fp32 sum.
struct MsWin { float w[11]; };
static MsWin make_window() {
    MsWin m;
    float s = 0.f;
    for (int i = 0; i < 11; ++i) { m.w[i] = (float)exp((double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); s += m.w[i]; }
    for (int i = 0; i < 11; ++i) m.w[i] = m.w[i] / s;
    return m;
}

static constexpr int MS_NF = 32;            // finalize workgroups
static_assert(MS_NF * 11 == MSSSIM_SLAB_DOUBLES, "objective.hip reuses the slab once the finalize has run");

// ------------------------------------------------------------------------------------------------
// shared by the forward kernels: packed fp32, the argument struct, the SSIM point function, segment sums
// ------------------------------------------------------------------------------------------------
// Round 3: the four filter passes run on PACKED fp32 (v_pk_fma_f32 / v_pk_mul_f32: two lanes of arithmetic per VALU
// issue — the kernels are VALU-bound, one wave64 VALU instruction holds its SIMD for 4 cycles).  What is packed is chosen
// so that every operand pair is already adjacent in registers AND in LDS, i.e. no v_mov shuffles:
//   horizontal passes pair two PLANES of one pixel — the staged image interleaves (x, y) per pixel, so (x, y) -> (hx, hy)
//     and (x^2, y^2) -> (hxx, hyy) are one packed chain each (xy -> hxy stays scalar); the derivative maps are kept as
//     (d_mu, d_11) pairs + a d_12 plane in the same way;
//   vertical passes pair the same two planes again for the pair images and two adjacent COLUMNS for the single plane;
//   the SSIM point function runs on two adjacent columns at once.
// Every output is still the same t = 0..10 fma chain over the same products: values are unchanged.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 splat2(float v) { return f32x2{v, v}; }

struct MsFwdArgs {
    const float* x;       // img1 at this level (carries grad)
    const float* y;       // img2
    float* nx; float* ny; // next level (2x2 averages)
    float* F;             // gradient field of this level (null: forward only)
    float* part;          // [numBlocks][2] (ssim sum, cs sum)
    unsigned* ticket;     // finalize arrival counter: zeroed here, a launch boundary ahead of its use
    int P;
    MsWin win;
};

// SSIM / CS value of two adjacent points and the derivatives of the level's contributing map (cs_map; ssim_map on the
// last level) w.r.t. (mu1, E[x^2], E[xy]) — vae_nets.py:201-215 and its autograd.
// 1/x to ~0.5 ulp: v_rcp_f32 + one Newton step (3 instructions instead of the ~11 of an IEEE division; the
// denominators are >= C1 / C2 minus round-off, far from the denormal range)
__device__ __forceinline__ f32x2 ms_rcp2(f32x2 x) {
    const f32x2 r = {__builtin_amdgcn_rcpf(x.x), __builtin_amdgcn_rcpf(x.y)};
    return pk_fma(pk_fma(-x, r, splat2(1.0f)), r, r);
}
template <bool LAST = false>
__device__ __forceinline__ void ms_point2(f32x2 mu1, f32x2 mu2, f32x2 a11, f32x2 a22, f32x2 a12, f32x2* ssim, f32x2* cs,
                                          f32x2* dm, f32x2* d11, f32x2* d12) {
    const f32x2 C1 = splat2(0.0001f), C2 = splat2(0.0009f), two = splat2(2.0f);
    const f32x2 mu1sq = mu1 * mu1, mu2sq = mu2 * mu2, mu12 = mu1 * mu2;
    const f32x2 v1 = two * (a12 - mu12) + C2;
    const f32x2 v2 = (a11 - mu1sq) + (a22 - mu2sq) + C2;
    const f32x2 inv2 = ms_rcp2(v2);
    const f32x2 c = v1 * inv2;
    const f32x2 num = two * mu12 + C1, den = mu1sq + mu2sq + C1;
    const f32x2 invden = ms_rcp2(den);
    const f32x2 lum = num * invden;
    *cs = c;
    *ssim = lum * c;
    f32x2 m = (two * mu1 * c - two * mu2) * inv2, e11 = -c * inv2, e12 = two * inv2;
    if constexpr (LAST) {          // the last level contributes ssim_map = lum * cs_map (same operations as ms_point)
        const f32x2 dlum = (two * mu2 - two * mu1 * lum) * invden;
        m = dlum * c + lum * m; e11 *= lum; e12 *= lum;
    }
    *dm = m; *d11 = e11; *d12 = e12;
}

// Sum over the SEG (4, 16 or 64) lanes of a lane's aligned segment with DPP row operations (6 VALU instructions per value
// for the whole wave; the shuffle form costs ~6 per STEP); the result is valid in the LAST lane of each segment for
// SEG = 64 and in every lane of the segment otherwise
template <int SEG>
__device__ __forceinline__ float seg_sum_dpp(float v) {
#define MS_DPP(ctrl, rmask) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rmask, 0xf, false))
    v += MS_DPP(0xB1, 0xf);       // quad_perm [1,0,3,2]
    v += MS_DPP(0x4E, 0xf);       // quad_perm [2,3,0,1]: every lane holds its quad's sum
    if constexpr (SEG >= 16) {
        v += MS_DPP(0x141, 0xf);  // row_half_mirror
        v += MS_DPP(0x140, 0xf);  // row_mirror: every lane holds its row's sum
    }
    if constexpr (SEG == 64) {
        v += MS_DPP(0x142, 0xa);  // row_bcast:15 into rows 1 and 3
        v += MS_DPP(0x143, 0xc);  // row_bcast:31 into rows 2 and 3: lane 63 holds the total
    }
#undef MS_DPP
    return v;
}

// ------------------------------------------------------------------------------------------------
// whole-plane levels (S <= 64): one workgroup per plane, S*S/4 threads, every pass exactly one item per thread
// ------------------------------------------------------------------------------------------------
// With the whole plane in one workgroup nothing outside the image is ever computed: conv2d's zero padding is literally
// zero rows / columns in LDS, each of the four filter passes runs on S x S positions, no position needs an inside /
// interior test, and every pass has exactly NT = S*S/4 items — all waves busy in every phase, which is what lets a
// single 1024-thread workgroup per CU (152 KB of LDS at S = 64) work.  Every output is the same t = 0..10 fma chain over
// the same products as in the stream kernel below, so F, the pyramid and the per-element SSIM / CS values are
// bit-identical between the two forms; only the order of a plane's partial sums differs.
template <int S>
struct MsP {
    static constexpr int NTP = S * S / 4;     // threads per plane
    static constexpr int PPW = NTP >= 256 ? 1 : 256 / NTP;      // planes per workgroup: 256 threads below S = 32
    static constexpr int NT = NTP * PPW;
    static constexpr int DAS = S + 14;        // row stride (pixels) of the (x, y) input image AND of the (d_mu, d_11) image that later
                                              // overlays it: 6 zero columns left (16-byte aligned stores and window reads; the
                                              // windows are read 16 wide), 8 right — the same columns in both uses, zeroed once
                                              // per workgroup.  DAS / 2 is ODD: an item of a horizontal pass reads
                                              // 16-byte units 32 bytes apart from its neighbour's, and with an odd row
                                              // stride in 16-byte units, lanes that alternate between two rows cover all
                                              // 16 slots of the 256-byte bank row: conflict-free
    static constexpr int DCS = S + 12;        // d_12 row stride: 6 zero columns either side (behind the input image: zeroed once)
    static constexpr int TAS = S + 2;         // row stride (pixels) of the pair images in tmp: the two rows of a lane pair
                                              // land 16 bytes apart modulo 32 — their 16-byte stores interleave
    static constexpr int TR = S + 10;         // rows of the tmp images: 5 zero rows above and below
    static constexpr int LIN = S * (2 * DAS + DCS);
    static constexpr int TA = 2 * TR * TAS;   // floats of one pair image
    static constexpr int TMP = 2 * TA + TR * S;
    static constexpr int PLANE = LIN + TMP;   // floats of LDS per plane
    static constexpr int SMEM = PPW * PLANE * 4;
    static_assert((DAS / 2) % 2 == 1 && DCS % 4 == 0 && TAS % 2 == 0 && PLANE % 4 == 0, "strides");
    static_assert(SMEM <= 160 * 1024 - 256, "LDS");
};

template <int S, bool LAST>
__global__ __launch_bounds__(MsP<S>::NT) void msssim_plane_kernel(MsFwdArgs a) {
    using T = MsP<S>;
    constexpr int NT = T::NT, NTP = T::NTP, PPW = T::PPW, J = S / 4, H = S / 2;
    constexpr int WPP = NTP >= 64 ? NTP / 64 : 1;        // waves per plane
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[2 * (NT / 64)];
    const int sub = PPW > 1 ? threadIdx.x / NTP : 0, tid = PPW > 1 ? threadIdx.x % NTP : threadIdx.x;
    float* lin = smem + sub * T::PLANE;   // (x, y) pixels [S][DAS][2], later (d_mu, d_11) in the same layout | d_12 [S][DCS]
    float* tmp = lin + T::LIN;            // (hx, hy) [TR][TAS][2] | (hxx, hyy) [TR][TAS][2] | hxy [TR][S]; later (g0, g1) | - | g2
    float* tA = tmp; float* tB = tmp + T::TA; float* tC = tmp + 2 * T::TA;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.ticket) *a.ticket = 0u;
    float w[11];
#pragma unroll
    for (int t = 0; t < 11; ++t) w[t] = a.win.w[t];
    {   // the 5 zero rows above and below the tmp images: written once, no pass ever stores there
        constexpr int ZP = 5 * T::TAS * 2 / 4, ZC = 5 * S / 4;        // 16-byte units of one block of 5 zero rows
        static_assert(ZP * 4 == 5 * T::TAS * 2 && ZC * 4 == 5 * S && ((S + 5) * T::TAS * 2) % 4 == 0 && T::TA % 4 == 0, "16-byte zero fill");
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int q = tid; q < ZP; q += NTP) {
            reinterpret_cast<f32x4*>(tA)[q] = z; reinterpret_cast<f32x4*>(tA + (S + 5) * T::TAS * 2)[q] = z;
            reinterpret_cast<f32x4*>(tB)[q] = z; reinterpret_cast<f32x4*>(tB + (S + 5) * T::TAS * 2)[q] = z;
        }
        for (int q = tid; q < ZC; q += NTP) { reinterpret_cast<f32x4*>(tC)[q] = z; reinterpret_cast<f32x4*>(tC + (S + 5) * S)[q] = z; }
        // ... and the zero columns of the input / derivative images: per row 3 + 4 16-byte units of the pair image, 6 + 6 floats of d_12
        float* dA0 = lin; float* dC0 = lin + 2 * S * T::DAS;
        for (int q = tid; q < S * 16; q += NTP) {
            const int zr = q >> 4, k = q & 15;
            float* ra = dA0 + zr * T::DAS * 2; float* rc = dC0 + zr * T::DCS;
            if (k < 3) *reinterpret_cast<f32x4*>(ra + 4 * k) = z;
            else if (k < 7) *reinterpret_cast<f32x4*>(ra + (S + 6) * 2 + 4 * (k - 3)) = z;
            else if (k == 7) *reinterpret_cast<f32x4*>(rc) = z;
            else if (k == 8) *reinterpret_cast<f32x2*>(rc + 4) = splat2(0.f);
            else if (k == 9) *reinterpret_cast<f32x2*>(rc + S + 6) = splat2(0.f);
            else if (k == 10) *reinterpret_cast<f32x4*>(rc + S + 8) = z;
        }
    }
    // Persistent: the grid is one residency of the chip (LDS-limited, 1 workgroup per CU at S = 64) and every workgroup walks
    // its share of the planes; the next plane's pixels are fetched into registers while this one is filtered, so the HBM
    // latency of the staging loads (2-5 k cycles with nothing else resident on the CU) is paid once per workgroup.
    const int ngroups = (a.P + PPW - 1) / PPW;
    float2 vx[2], vy[2];                  // pixels (r, 2c), (r, 2c + 1) of rows r = tid / H and r + H
    {
        const int p0 = min((int)blockIdx.x * PPW + sub, a.P - 1);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            vx[k] = *reinterpret_cast<const float2*>(a.x + (size_t)p0 * S * S + 2 * (tid + k * NTP));
            vy[k] = *reinterpret_cast<const float2*>(a.y + (size_t)p0 * S * S + 2 * (tid + k * NTP));
        }
    }
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int pl = grp * PPW + sub;
    const bool valid = pl < a.P;                          // planes past the end: same work on the last plane, no stores
    const int plane = valid ? pl : a.P - 1;
    // ---- stage the plane, (x, y) interleaved per pixel (the zero columns either side are already there) ----
    {
        const int r = tid / H, c = (tid % H) * 2;
#pragma unroll
        for (int k = 0; k < 2; ++k)
            *reinterpret_cast<f32x4*>(lin + ((r + k * H) * T::DAS + 6 + c) * 2) = f32x4{vx[k].x, vy[k].x, vx[k].y, vy[k].y};
        if (grp + (int)gridDim.x < ngroups) {             // next plane of this workgroup: in flight during the four passes
            const int pn = min((grp + (int)gridDim.x) * PPW + sub, a.P - 1);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                vx[k] = *reinterpret_cast<const float2*>(a.x + (size_t)pn * S * S + 2 * (tid + k * NTP));
                vy[k] = *reinterpret_cast<const float2*>(a.y + (size_t)pn * S * S + 2 * (tid + k * NTP));
            }
        }
    }
    __syncthreads();
    // ---- 2x2 average for the next level (avg_pool2d, vae_nets.py:232-233): one output per thread ----
    if (a.nx) {
        const int pr = tid / H, pc = tid % H;
        const float* p = lin + ((2 * pr) * T::DAS + 6 + 2 * pc) * 2;
        const f32x4 u = *reinterpret_cast<const f32x4*>(p), d = *reinterpret_cast<const f32x4*>(p + 2 * T::DAS);      // (x0, y0, x1, y1)
        const f32x2 o = ((f32x2{u[0], u[1]} + f32x2{u[2], u[3]}) + (f32x2{d[0], d[1]} + f32x2{d[2], d[3]})) * splat2(0.25f);
        if (valid) { a.nx[(size_t)plane * NTP + tid] = o.x; a.ny[(size_t)plane * NTP + tid] = o.y; }
    }
    // ---- horizontal pass of {x, y, x^2, y^2, xy}: 4 adjacent outputs per thread from a register window (16 pixels from
    //      column c - 6, 16-byte aligned; taps at window positions o + 1 .. o + 11) ----
    const int hr = 2 * (tid / (2 * J)) + (tid & 1), hc = ((tid % (2 * J)) >> 1) * 4;      // neighbouring lanes: the two rows of a pair
    {
        const float* p = lin + (hr * T::DAS + hc) * 2;
        f32x2 xy[16];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(p + 4 * i);
            xy[2 * i] = f32x2{u[0], u[1]}; xy[2 * i + 1] = f32x2{u[2], u[3]};
        }
        f32x2 hA[4], hB[4];
        float hC[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            f32x2 sA = splat2(0.f), sB = splat2(0.f);
            float sC = 0.f;
#pragma unroll
            for (int t = 0; t < 11; ++t) {
                const f32x2 v = xy[o + t + 1];
                sA = pk_fma(splat2(w[t]), v, sA);
                sB = pk_fma(splat2(w[t]), v * v, sB);
                sC = fmaf(w[t], v.x * v.y, sC);
            }
            hA[o] = sA; hB[o] = sB; hC[o] = sC;
        }
        const int d = ((hr + 5) * T::TAS + hc) * 2;
        *reinterpret_cast<f32x4*>(tA + d) = f32x4{hA[0].x, hA[0].y, hA[1].x, hA[1].y};
        *reinterpret_cast<f32x4*>(tA + d + 4) = f32x4{hA[2].x, hA[2].y, hA[3].x, hA[3].y};
        *reinterpret_cast<f32x4*>(tB + d) = f32x4{hB[0].x, hB[0].y, hB[1].x, hB[1].y};
        *reinterpret_cast<f32x4*>(tB + d + 4) = f32x4{hB[2].x, hB[2].y, hB[3].x, hB[3].y};
        *reinterpret_cast<f32x4*>(tC + (hr + 5) * S + hc) = f32x4{hC[0], hC[1], hC[2], hC[3]};
    }
    __syncthreads();
    // ---- vertical pass (2 rows x 2 columns per thread) + SSIM / CS maps + derivative maps into the input buffer ----
    const int vr = (tid / H) * 2, vc = (tid % H) * 2;
    float* dA = lin; float* dC = lin + 2 * S * T::DAS;
    float s_ssim = 0.f, s_cs = 0.f;
    f32x4 xy_keep[2];                     // (x0, y0, x1, y1) of rows vr, vr + 1 at columns vc, vc + 1
    {
        constexpr int VR = 2;
        f32x2 mu[VR][2], aa[VR][2], a12[VR];
#pragma unroll
        for (int o = 0; o < VR; ++o) { mu[o][0] = mu[o][1] = aa[o][0] = aa[o][1] = a12[o] = splat2(0.f); }
        // one base address per image, rows at compile-time offsets (ds_read immediates, no per-row address arithmetic)
        const float* pA = tA + (vr * T::TAS + vc) * 2;
        const float* pC = tC + vr * S + vc;
#pragma unroll
        for (int i = 0; i < VR + 10; ++i) {               // tmp row vr + i = image row vr + i - 5
            const f32x4 vA = *reinterpret_cast<const f32x4*>(pA + i * (T::TAS * 2));
            const f32x4 vB = *reinterpret_cast<const f32x4*>(pA + T::TA + i * (T::TAS * 2));
            const f32x2 vC = *reinterpret_cast<const f32x2*>(pC + i * S);
#pragma unroll
            for (int o = 0; o < VR; ++o) {
                if (i - o < 0 || i - o > 10) continue;
                const f32x2 wt = splat2(w[i - o]);
                mu[o][0] = pk_fma(wt, f32x2{vA[0], vA[1]}, mu[o][0]);
                mu[o][1] = pk_fma(wt, f32x2{vA[2], vA[3]}, mu[o][1]);
                aa[o][0] = pk_fma(wt, f32x2{vB[0], vB[1]}, aa[o][0]);
                aa[o][1] = pk_fma(wt, f32x2{vB[2], vB[3]}, aa[o][1]);
                a12[o] = pk_fma(wt, vC, a12[o]);
            }
            if (i < 10) continue;
            const int o = i - 10, r = vr + o;
            f32x2 ss, cs, dmv, d11v, d12v;
            ms_point2<LAST>(f32x2{mu[o][0].x, mu[o][1].x}, f32x2{mu[o][0].y, mu[o][1].y}, f32x2{aa[o][0].x, aa[o][1].x},
                            f32x2{aa[o][0].y, aa[o][1].y}, a12[o], &ss, &cs, &dmv, &d11v, &d12v);
            s_ssim += ss.x + ss.y; s_cs += cs.x + cs.y;
            // the derivative pair overwrites exactly this thread's own (x, y) pixels of row r: keep them for the last pass (F = f0 +
            // 2 x f1 + y f2) instead of fetching them again from global memory, where — 19 k cycles and 1.8 MB of other planes per
            // XCD later — 70 % of the lines had left L2 (round 3: 490 MB of HBM traffic for 352 MB algorithmic)
            xy_keep[o] = *reinterpret_cast<const f32x4*>(dA + (r * T::DAS + 6 + vc) * 2);
            *reinterpret_cast<f32x4*>(dA + (r * T::DAS + 6 + vc) * 2) = f32x4{dmv.x, d11v.x, dmv.y, d11v.y};
            *reinterpret_cast<f32x2*>(dC + r * T::DCS + 6 + vc) = d12v;
        }
    }
    constexpr int SEG = NTP >= 64 ? 64 : NTP;
    s_ssim = seg_sum_dpp<SEG>(s_ssim); s_cs = seg_sum_dpp<SEG>(s_cs);
    if constexpr (WPP > 1) {
        if ((threadIdx.x & 63) == 63) { red[(threadIdx.x >> 6) * 2] = s_ssim; red[(threadIdx.x >> 6) * 2 + 1] = s_cs; }
    } else if (valid && (tid & (SEG - 1)) == SEG - 1) {
        a.part[(size_t)plane * 2] = s_ssim;
        a.part[(size_t)plane * 2 + 1] = s_cs;
    }
    __syncthreads();
    if constexpr (WPP > 1) {
        if (tid == 0 && valid) {
            float t0 = 0.f, t1 = 0.f;
#pragma unroll
            for (int k = 0; k < WPP; ++k) { t0 += red[2 * (sub * WPP + k)]; t1 += red[2 * (sub * WPP + k) + 1]; }
            a.part[(size_t)plane * 2] = t0;
            a.part[(size_t)plane * 2 + 1] = t1;
        }
    }
    if (!a.F) continue;         // (all waves are past the barrier above: the next plane may be staged over the derivative maps)
    // ---- the same separable filter over the three derivative maps: horizontal (16-wide windows from column c - 6) ... ----
    {
        f32x2 va[16];
        float vc4[16];
        const float* pa = dA + (hr * T::DAS + hc) * 2;
        const float* pc = dC + hr * T::DCS + hc;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(pa + 4 * i);
            va[2 * i] = f32x2{u[0], u[1]}; va[2 * i + 1] = f32x2{u[2], u[3]};
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(pc + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) vc4[4 * i + e] = u[e];
        }
        f32x2 gAo[4];
        f32x4 gCo;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            f32x2 sA = splat2(0.f);
            float sC = 0.f;
#pragma unroll
            for (int t = 0; t < 11; ++t) { sA = pk_fma(splat2(w[t]), va[o + t + 1], sA); sC = fmaf(w[t], vc4[o + t + 1], sC); }
            gAo[o] = sA; gCo[o] = sC;
        }
        const int d = ((hr + 5) * T::TAS + hc) * 2;
        *reinterpret_cast<f32x4*>(tA + d) = f32x4{gAo[0].x, gAo[0].y, gAo[1].x, gAo[1].y};
        *reinterpret_cast<f32x4*>(tA + d + 4) = f32x4{gAo[2].x, gAo[2].y, gAo[3].x, gAo[3].y};
        *reinterpret_cast<f32x4*>(tC + (hr + 5) * S + hc) = gCo;
    }
    __syncthreads();
    // ---- ... vertical (2 rows x 2 columns per thread), then F = f0 + 2 x f1 + y f2 ----
    {
        constexpr int VR = 2;
        const size_t g = (size_t)vr * S + vc;
        float2 xv[VR], yv[VR];               // kept from the staged image (see the vertical pass above)
#pragma unroll
        for (int o = 0; o < VR; ++o) {
            xv[o] = make_float2(xy_keep[o][0], xy_keep[o][2]);
            yv[o] = make_float2(xy_keep[o][1], xy_keep[o][3]);
        }
        f32x2 f01[VR][2], f2[VR];
#pragma unroll
        for (int o = 0; o < VR; ++o) { f01[o][0] = f01[o][1] = f2[o] = splat2(0.f); }
        const float* pA = tA + (vr * T::TAS + vc) * 2;
        const float* pC = tC + vr * S + vc;
#pragma unroll
        for (int i = 0; i < VR + 10; ++i) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(pA + i * (T::TAS * 2));
            const f32x2 u = *reinterpret_cast<const f32x2*>(pC + i * S);
#pragma unroll
            for (int o = 0; o < VR; ++o) {
                if (i - o < 0 || i - o > 10) continue;
                f01[o][0] = pk_fma(splat2(w[i - o]), f32x2{v[0], v[1]}, f01[o][0]);
                f01[o][1] = pk_fma(splat2(w[i - o]), f32x2{v[2], v[3]}, f01[o][1]);
                f2[o] = pk_fma(splat2(w[i - o]), u, f2[o]);
            }
        }
        float* pf = a.F + (size_t)plane * S * S;
        if (valid) {
#pragma unroll
            for (int o = 0; o < VR; ++o)
                *reinterpret_cast<float2*>(pf + g + (size_t)o * S) =
                    make_float2(f01[o][0].x + 2.0f * xv[o].x * f01[o][0].y + yv[o].x * f2[o].x,
                                f01[o][1].x + 2.0f * xv[o].y * f01[o][1].y + yv[o].y * f2[o].y);
        }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// the 128-wide level (level 0 of BASELINE config 5's frames): one workgroup per plane, the plane STREAMED through LDS in bands
// ------------------------------------------------------------------------------------------------
// A whole 128 x 128 plane needs 4x the LDS of the 64-wide plane kernel, and strips with a halo pay for the halo in every one of the four
// filter passes (a 16 x 128 strip filters 36 / 26 / 26 / 16 rows: 6.5 units of work per output row against the plane kernel's 4.0).  Streaming pays 4.5: the workgroup walks down its plane in bands of R = 16 rows and keeps, in LDS, the
// last R + 10 rows of every ROW-FILTERED field — {hx, hy, hxx, hyy, hxy} of the input (t1) and {g0, g1, g2} of the derivative maps (t2).
// Per band (image rows b0 .. b0 + R - 1 arrive; b0 = 0, R, .., S, the last band carries zero rows to flush the two 5-row lags):
//   stage the band's (x, y) rows                                    -> lin rows 0..R-1
//   h1: row-filter them                                            -> t1 rows 10..R+9        (t1 row j = image row b0 - 10 + j)
//   v1: column-filter t1 rows i..i+10, SSIM / CS point function    -> maps of image rows b0 - 5 + i; derivative maps over lin
//   h2: row-filter the derivative maps                              -> t2 rows 10..R+9        (t2 row j = map row b0 - 15 + j)
//   v2: column-filter t2 rows i..i+10, F = f0 + 2 x f1 + y f2       -> F rows b0 - 10 + i      (x, y of those rows: fetched again, L2)
//   the last 10 rows of t1 / t2 move to the top (rows outside the image are zero: conv2d's padding, never computed as maps).
// Every pass has exactly R * S / 4 = 512 items = threads, with the plane kernel's item shapes and fma chains (the same
// t = 0..10 order over the same products, so values are the plane kernel's; only the order of a plane's partial sums differs).  9 bands x 4 passes of 16
// rows = 4.5 units; 135 KB of LDS, one workgroup (8 waves) per CU, persistent over planes, the next band's pixels in flight in
// registers during the passes.
template <int S, int R>
struct MsS {
    static constexpr int NT = R * S / 4;                 // threads = items of every pass
    static constexpr int NBAND = S / R + 1;
    static constexpr int DAS = S + 14, DCS = S + 12, TAS = S + 2, TR = R + 10;       // strides as in MsP; TR = rows of the t images
    static constexpr int LIN = R * (2 * DAS + DCS);      // (x, y) [R][DAS][2], later (d_mu, d_11) | d_12 [R][DCS]
    static constexpr int TA = 2 * TR * TAS;              // one pair image
    static constexpr int T1 = 2 * TA + TR * S;           // (hx, hy) | (hxx, hyy) | hxy
    static constexpr int T2 = TA + TR * S;               // (g0, g1) | g2
    static constexpr int SMEM = (LIN + T1 + T2) * 4;
    static constexpr int HA4 = 10 * TAS * 2 / 4, HC4 = 10 * S / 4;                  // 16-byte units of 10 history rows (pair image / single plane)
    static_assert((DAS / 2) % 2 == 1 && DCS % 4 == 0 && TAS % 2 == 0 && LIN % 4 == 0 && TA % 4 == 0 && (TR * S) % 4 == 0, "strides");
    static_assert(R >= 10 && R % 2 == 0 && S % R == 0 && NT % 64 == 0 && NT <= 1024 && (R * TAS * 2) % 4 == 0, "band geometry");
    static_assert(SMEM <= 160 * 1024 - 256, "LDS");
};

template <int S, int R>
__global__ __launch_bounds__((MsS<S, R>::NT)) void msssim_stream_kernel(MsFwdArgs a) {
    using T = MsS<S, R>;
    constexpr int NT = T::NT, J = S / 4, H = S / 2, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[2 * NW];
    const int tid = threadIdx.x;
    float* lin = smem;
    float* t1A = lin + T::LIN; float* t1B = t1A + T::TA; float* t1C = t1B + T::TA;
    float* t2A = t1C + T::TR * S; float* t2C = t2A + T::TA;
    float* dA = lin; float* dC = lin + 2 * R * T::DAS;
    if (blockIdx.x == 0 && tid == 0 && a.ticket) *a.ticket = 0u;
    float w[11];
#pragma unroll
    for (int t = 0; t < 11; ++t) w[t] = a.win.w[t];
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    // the zero columns either side of the input / derivative rows: written once, no pass ever stores there (as in the plane kernel)
    for (int q = tid; q < R * 16; q += NT) {
        const int zr = q >> 4, k = q & 15;
        float* ra = dA + zr * T::DAS * 2; float* rc = dC + zr * T::DCS;
        if (k < 3) *reinterpret_cast<f32x4*>(ra + 4 * k) = z4;
        else if (k < 7) *reinterpret_cast<f32x4*>(ra + (S + 6) * 2 + 4 * (k - 3)) = z4;
        else if (k == 7) *reinterpret_cast<f32x4*>(rc) = z4;
        else if (k == 8) *reinterpret_cast<f32x2*>(rc + 4) = splat2(0.f);
        else if (k == 9) *reinterpret_cast<f32x2*>(rc + S + 6) = splat2(0.f);
        else if (k == 10) *reinterpret_cast<f32x4*>(rc + S + 8) = z4;
    }
    // item shapes of the plane kernel: horizontal = 4 adjacent outputs of one row (neighbouring lanes: the two rows of a pair), vertical = 2 x 2
    const int hr = 2 * (tid / (2 * J)) + (tid & 1), hc = ((tid % (2 * J)) >> 1) * 4;
    const int vr = (tid / H) * 2, vc = (tid % H) * 2;
    const int sr = tid / H, sc = (tid % H) * 2;              // staging: pixels (sr, sc), (sr, sc + 1) and the same of row sr + R / 2
    float2 vx[2], vy[2];                                     // the band to be staged next
    auto fetch_band = [&](int plane, int b0) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const bool in = b0 + sr + k * (R / 2) < S;       // rows past the image: the flush band
            const size_t e = (size_t)plane * S * S + (in ? (size_t)b0 * S + 2 * (tid + k * NT) : 0);
            const float2 lx = *reinterpret_cast<const float2*>(a.x + e), ly = *reinterpret_cast<const float2*>(a.y + e);
            vx[k] = in ? lx : make_float2(0.f, 0.f);
            vy[k] = in ? ly : make_float2(0.f, 0.f);
        }
    };
    if ((int)blockIdx.x < a.P) fetch_band(blockIdx.x, 0);
    for (int plane = blockIdx.x; plane < a.P; plane += gridDim.x) {
        float s_ssim = 0.f, s_cs = 0.f;
        for (int kb = 0; kb < T::NBAND; ++kb) {
            const int b0 = kb * R;
            // ---- history rows of the row-filtered images: zero at the top of a plane, else the last 10 rows of the previous band ----
            for (int q = tid; q < T::HA4; q += NT) {
                f32x4* A1 = reinterpret_cast<f32x4*>(t1A); f32x4* B1 = reinterpret_cast<f32x4*>(t1B); f32x4* A2 = reinterpret_cast<f32x4*>(t2A);
                constexpr int SRC = R * T::TAS * 2 / 4;
                A1[q] = kb ? A1[q + SRC] : z4; B1[q] = kb ? B1[q + SRC] : z4; A2[q] = kb ? A2[q + SRC] : z4;
            }
            for (int q = tid; q < T::HC4; q += NT) {
                f32x4* C1 = reinterpret_cast<f32x4*>(t1C); f32x4* C2 = reinterpret_cast<f32x4*>(t2C);
                constexpr int SRC = R * S / 4;
                C1[q] = kb ? C1[q + SRC] : z4; C2[q] = kb ? C2[q + SRC] : z4;
            }
            // ---- stage the band, (x, y) interleaved per pixel; the next band (or the next plane's first) goes in flight ----
#pragma unroll
            for (int k = 0; k < 2; ++k)
                *reinterpret_cast<f32x4*>(lin + ((sr + k * (R / 2)) * T::DAS + 6 + sc) * 2) = f32x4{vx[k].x, vy[k].x, vx[k].y, vy[k].y};
            if (kb + 1 < T::NBAND) fetch_band(plane, b0 + R);
            else if (plane + (int)gridDim.x < a.P) fetch_band(plane + gridDim.x, 0);
            // x, y of the F rows this band completes (rows b0 - 10 + vr, + 1): both inside the image or both outside
            const int f0 = b0 - 10 + vr;
            const bool fvalid = (unsigned)f0 < (unsigned)S;
            float2 fx[2], fy[2];
            if (a.F) {
#pragma unroll
                for (int o = 0; o < 2; ++o) {
                    const size_t e = (size_t)plane * S * S + (fvalid ? (size_t)(f0 + o) * S + vc : 0);
                    fx[o] = *reinterpret_cast<const float2*>(a.x + e); fy[o] = *reinterpret_cast<const float2*>(a.y + e);
                }
            }
            __syncthreads();
            // ---- 2x2 average for the next level: one output per thread (R / 2 rows of S / 2) ----
            if (a.nx && b0 < S) {
                const int pr = tid / H, pc = tid % H;
                const float* p = lin + ((2 * pr) * T::DAS + 6 + 2 * pc) * 2;
                const f32x4 u = *reinterpret_cast<const f32x4*>(p), d = *reinterpret_cast<const f32x4*>(p + 2 * T::DAS);
                const f32x2 o = ((f32x2{u[0], u[1]} + f32x2{u[2], u[3]}) + (f32x2{d[0], d[1]} + f32x2{d[2], d[3]})) * splat2(0.25f);
                const size_t e = (size_t)plane * H * H + (size_t)(b0 / 2 + pr) * H + pc;
                a.nx[e] = o.x; a.ny[e] = o.y;
            }
            // ---- horizontal pass of {x, y, x^2, y^2, xy} (the flush band's rows are zero: so are their filtered values) ----
            if (b0 >= S) {
                const int d = ((hr + 10) * T::TAS + hc) * 2;
                *reinterpret_cast<f32x4*>(t1A + d) = z4; *reinterpret_cast<f32x4*>(t1A + d + 4) = z4;
                *reinterpret_cast<f32x4*>(t1B + d) = z4; *reinterpret_cast<f32x4*>(t1B + d + 4) = z4;
                *reinterpret_cast<f32x4*>(t1C + (hr + 10) * S + hc) = z4;
            } else {
                const float* p = lin + (hr * T::DAS + hc) * 2;
                f32x2 xy[16];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const f32x4 u = *reinterpret_cast<const f32x4*>(p + 4 * i);
                    xy[2 * i] = f32x2{u[0], u[1]}; xy[2 * i + 1] = f32x2{u[2], u[3]};
                }
                f32x2 hA[4], hB[4];
                float hC[4];
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    f32x2 sA = splat2(0.f), sB = splat2(0.f);
                    float sC = 0.f;
#pragma unroll
                    for (int t = 0; t < 11; ++t) {
                        const f32x2 v = xy[o + t + 1];
                        sA = pk_fma(splat2(w[t]), v, sA);
                        sB = pk_fma(splat2(w[t]), v * v, sB);
                        sC = fmaf(w[t], v.x * v.y, sC);
                    }
                    hA[o] = sA; hB[o] = sB; hC[o] = sC;
                }
                const int d = ((hr + 10) * T::TAS + hc) * 2;
                *reinterpret_cast<f32x4*>(t1A + d) = f32x4{hA[0].x, hA[0].y, hA[1].x, hA[1].y};
                *reinterpret_cast<f32x4*>(t1A + d + 4) = f32x4{hA[2].x, hA[2].y, hA[3].x, hA[3].y};
                *reinterpret_cast<f32x4*>(t1B + d) = f32x4{hB[0].x, hB[0].y, hB[1].x, hB[1].y};
                *reinterpret_cast<f32x4*>(t1B + d + 4) = f32x4{hB[2].x, hB[2].y, hB[3].x, hB[3].y};
                *reinterpret_cast<f32x4*>(t1C + (hr + 10) * S + hc) = f32x4{hC[0], hC[1], hC[2], hC[3]};
            }
            __syncthreads();
            // ---- vertical pass + SSIM / CS maps of image rows b0 - 5 + vr (+ 1); derivative maps over the input rows ----
            if ((unsigned)(b0 - 5 + vr) >= (unsigned)S && (unsigned)(b0 - 4 + vr) >= (unsigned)S) {      // wave-uniform: vr = 2 x wave
#pragma unroll
                for (int o = 0; o < 2; ++o) {
                    *reinterpret_cast<f32x4*>(dA + ((vr + o) * T::DAS + 6 + vc) * 2) = z4;
                    *reinterpret_cast<f32x2*>(dC + (vr + o) * T::DCS + 6 + vc) = splat2(0.f);
                }
            } else {
                constexpr int VR = 2;
                f32x2 mu[VR][2], aa[VR][2], a12[VR];
#pragma unroll
                for (int o = 0; o < VR; ++o) { mu[o][0] = mu[o][1] = aa[o][0] = aa[o][1] = a12[o] = splat2(0.f); }
                const float* pA = t1A + (vr * T::TAS + vc) * 2;
                const float* pC = t1C + vr * S + vc;
#pragma unroll
                for (int i = 0; i < VR + 10; ++i) {               // t1 row vr + i = image row b0 - 10 + vr + i
                    const f32x4 vA = *reinterpret_cast<const f32x4*>(pA + i * (T::TAS * 2));
                    const f32x4 vB = *reinterpret_cast<const f32x4*>(pA + T::TA + i * (T::TAS * 2));
                    const f32x2 vC = *reinterpret_cast<const f32x2*>(pC + i * S);
#pragma unroll
                    for (int o = 0; o < VR; ++o) {
                        if (i - o < 0 || i - o > 10) continue;
                        const f32x2 wt = splat2(w[i - o]);
                        mu[o][0] = pk_fma(wt, f32x2{vA[0], vA[1]}, mu[o][0]);
                        mu[o][1] = pk_fma(wt, f32x2{vA[2], vA[3]}, mu[o][1]);
                        aa[o][0] = pk_fma(wt, f32x2{vB[0], vB[1]}, aa[o][0]);
                        aa[o][1] = pk_fma(wt, f32x2{vB[2], vB[3]}, aa[o][1]);
                        a12[o] = pk_fma(wt, vC, a12[o]);
                    }
                    if (i < 10) continue;
                    const int o = i - 10, r = vr + o;
                    const bool mvalid = (unsigned)(b0 - 5 + r) < (unsigned)S;      // map rows outside the image: zero (conv2d's padding of the derivative maps)
                    f32x2 ss, cs, dmv, d11v, d12v;
                    ms_point2<false>(f32x2{mu[o][0].x, mu[o][1].x}, f32x2{mu[o][0].y, mu[o][1].y}, f32x2{aa[o][0].x, aa[o][1].x},
                                     f32x2{aa[o][0].y, aa[o][1].y}, a12[o], &ss, &cs, &dmv, &d11v, &d12v);
                    if (mvalid) { s_ssim += ss.x + ss.y; s_cs += cs.x + cs.y; }
                    else { dmv = d11v = d12v = splat2(0.f); }
                    *reinterpret_cast<f32x4*>(dA + (r * T::DAS + 6 + vc) * 2) = f32x4{dmv.x, d11v.x, dmv.y, d11v.y};
                    *reinterpret_cast<f32x2*>(dC + r * T::DCS + 6 + vc) = d12v;
                }
            }
            __syncthreads();
            if (a.F) {
                // ---- the same separable filter over the three derivative maps: horizontal (zero map rows filter to zero) ... ----
                const int hw = hr & ~1;           // the wave's two rows
                if ((unsigned)(b0 - 5 + hw) >= (unsigned)S && (unsigned)(b0 - 4 + hw) >= (unsigned)S) {
                    const int d = ((hr + 10) * T::TAS + hc) * 2;
                    *reinterpret_cast<f32x4*>(t2A + d) = z4; *reinterpret_cast<f32x4*>(t2A + d + 4) = z4;
                    *reinterpret_cast<f32x4*>(t2C + (hr + 10) * S + hc) = z4;
                } else {
                    f32x2 va[16];
                    float vc4[16];
                    const float* pa = dA + (hr * T::DAS + hc) * 2;
                    const float* pc = dC + hr * T::DCS + hc;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const f32x4 u = *reinterpret_cast<const f32x4*>(pa + 4 * i);
                        va[2 * i] = f32x2{u[0], u[1]}; va[2 * i + 1] = f32x2{u[2], u[3]};
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const f32x4 u = *reinterpret_cast<const f32x4*>(pc + 4 * i);
#pragma unroll
                        for (int e = 0; e < 4; ++e) vc4[4 * i + e] = u[e];
                    }
                    f32x2 gAo[4];
                    f32x4 gCo;
#pragma unroll
                    for (int o = 0; o < 4; ++o) {
                        f32x2 sA = splat2(0.f);
                        float sC = 0.f;
#pragma unroll
                        for (int t = 0; t < 11; ++t) { sA = pk_fma(splat2(w[t]), va[o + t + 1], sA); sC = fmaf(w[t], vc4[o + t + 1], sC); }
                        gAo[o] = sA; gCo[o] = sC;
                    }
                    const int d = ((hr + 10) * T::TAS + hc) * 2;
                    *reinterpret_cast<f32x4*>(t2A + d) = f32x4{gAo[0].x, gAo[0].y, gAo[1].x, gAo[1].y};
                    *reinterpret_cast<f32x4*>(t2A + d + 4) = f32x4{gAo[2].x, gAo[2].y, gAo[3].x, gAo[3].y};
                    *reinterpret_cast<f32x4*>(t2C + (hr + 10) * S + hc) = gCo;
                }
                __syncthreads();
                // ---- ... vertical, then F = f0 + 2 x f1 + y f2 for image rows b0 - 10 + vr (+ 1) ----
                if (fvalid) {
                    constexpr int VR = 2;
                    f32x2 f01[VR][2], f2[VR];
#pragma unroll
                    for (int o = 0; o < VR; ++o) { f01[o][0] = f01[o][1] = f2[o] = splat2(0.f); }
                    const float* pA = t2A + (vr * T::TAS + vc) * 2;
                    const float* pC = t2C + vr * S + vc;
#pragma unroll
                    for (int i = 0; i < VR + 10; ++i) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(pA + i * (T::TAS * 2));
                        const f32x2 u = *reinterpret_cast<const f32x2*>(pC + i * S);
#pragma unroll
                        for (int o = 0; o < VR; ++o) {
                            if (i - o < 0 || i - o > 10) continue;
                            f01[o][0] = pk_fma(splat2(w[i - o]), f32x2{v[0], v[1]}, f01[o][0]);
                            f01[o][1] = pk_fma(splat2(w[i - o]), f32x2{v[2], v[3]}, f01[o][1]);
                            f2[o] = pk_fma(splat2(w[i - o]), u, f2[o]);
                        }
                    }
                    float* pf = a.F + (size_t)plane * S * S + (size_t)f0 * S + vc;
#pragma unroll
                    for (int o = 0; o < VR; ++o)
                        *reinterpret_cast<float2*>(pf + (size_t)o * S) =
                            make_float2(f01[o][0].x + 2.0f * fx[o].x * f01[o][0].y + fy[o].x * f2[o].x,
                                        f01[o][1].x + 2.0f * fx[o].y * f01[o][1].y + fy[o].y * f2[o].y);
                }
            }
            if (kb == T::NBAND - 1) {             // the plane's partial sums: per wave by DPP, then one thread in wave order
                const float t0 = seg_sum_dpp<64>(s_ssim), t1 = seg_sum_dpp<64>(s_cs);
                if ((tid & 63) == 63) { red[(tid >> 6) * 2] = t0; red[(tid >> 6) * 2 + 1] = t1; }
            }
            __syncthreads();                      // the next band's history move / staging overwrite what this band's passes read
        }
        if (tid == 0) {
            float t0 = 0.f, t1 = 0.f;
#pragma unroll
            for (int k = 0; k < NW; ++k) { t0 += red[2 * k]; t1 += red[2 * k + 1]; }
            a.part[(size_t)plane * 2] = t0;
            a.part[(size_t)plane * 2 + 1] = t1;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// finalize: MS_NF workgroups reduce the partials / the KLD in fp64, the last arriver finishes
// ------------------------------------------------------------------------------------------------
struct MsFinArgs {
    const float* part[5];    // level l: nblk[l] (ssim, cs) pairs
    int nblk[5];
    double count[5];         // B*3*S_l*S_l
    const float* mu; const float* logvar; int B;
    double* slab;            // [MS_NF][11]
    unsigned* ticket;
    float* scalars;          // CVAE_N_SCALARS
    float* coef;             // [5] per-pixel gradient coefficient of each level's map
    float* d_mu; float* d_logvar;
    double* rec;             // cross-rank path: the 11 sums (record mode writes them, the finish step reads the summed ones)
    const double* images;    // cross-rank path, finish step: the summed image count (replaces B and count[])
    float kw, w_ms;          // the objective: KLD weight, MS-SSIM weight (MS_REF_KW, 1 everywhere but under cvae_loss_obj)
    int used;                // gradient over the used terms only (msssim_finish.h)
};

// REC (cross-rank path): no d_mu / d_logvar (a.d_mu is null), and the last arriver writes its 11 sums to a.rec instead of
// finishing — msssim_finish_kernel finishes from the sums of all ranks
template <bool REC>
__global__ __launch_bounds__(256) void msssim_finalize_kernel(MsFinArgs a) {
    __shared__ double red[11][4];
    __shared__ unsigned last_flag;
    // every thread accumulates all 11 sums (5 x ssim, 5 x cs, KLD) over its strided share, one block
    // reduction, one fp64 row per workgroup — all in a fixed order
    double acc[11];
#pragma unroll
    for (int q = 0; q < 11; ++q) acc[q] = 0.0;
    const int gtid = blockIdx.x * 256 + threadIdx.x, gstride = MS_NF * 256;
#pragma unroll
    for (int l = 0; l < 5; ++l)
        for (int i = gtid; i < a.nblk[l]; i += gstride) {
            acc[l] += (double)a.part[l][(size_t)i * 2];
            acc[5 + l] += (double)a.part[l][(size_t)i * 2 + 1];
        }
    const float kw = a.kw, invB = a.B > 0 ? 1.0f / (float)a.B : 0.f;
    for (int i = gtid; i < a.B * 32; i += gstride) {
        const float m = a.mu[i], lv = a.logvar[i], e = expf(lv);
        acc[10] += (double)(1.0f + lv - m * m - e);
        if (a.d_mu) { a.d_mu[i] = kw * m * invB; a.d_logvar[i] = kw * 0.5f * (e - 1.0f) * invB; }
    }
#pragma unroll
    for (int q = 0; q < 11; ++q) {
        const double v = wave_sum_d(acc[q]);
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < 11) a.slab[blockIdx.x * 11 + threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
    if (!wg_arrive_last(a.ticket, MS_NF, &last_flag)) return;
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        double t = 0.0;
        if (lane < 11) for (int g = 0; g < MS_NF; ++g) t += a.slab[g * 11 + lane];
        if (REC) { if (lane < 11) a.rec[lane] = t; return; }
        ms_finish_scalars(lane, t, a.count[lane % 5], (double)a.B, a.scalars, a.coef, kw, a.used != 0, a.w_ms);
    }
}

// cross-rank path, finish step: scalars and coef from the summed 11 sums with the global counts 3 * B_g * S_l^2, and d_mu /
// d_logvar of this rank's a.B rows with the global 1 / B_g (B_g = *a.images).  Grid: ceil(a.B * 32 / 256) workgroups (>= 1).
__global__ __launch_bounds__(256) void msssim_finish_kernel(MsFinArgs a, int width) {
    const double Bg = a.images[0];
    const float kw = MS_REF_KW, invB = Bg > 0 ? 1.0f / (float)Bg : 0.f;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (a.d_mu && i < a.B * 32) {
        const float m = a.mu[i], lv = a.logvar[i], e = expf(lv);
        a.d_mu[i] = kw * m * invB; a.d_logvar[i] = kw * 0.5f * (e - 1.0f) * invB;
    }
    if (blockIdx.x != 0 || threadIdx.x >= 64) return;
    const int lane = threadIdx.x, S = width >> (lane % 5);
    const double t = lane < 11 ? a.rec[lane] : 0.0;
    ms_finish_scalars(lane, t, 3.0 * Bg * S * S, Bg, a.scalars, a.coef, MS_REF_KW, false, 1.0f);
}

// ------------------------------------------------------------------------------------------------
// backward: dx = c0 F0 + 1/4 up(c1 F1 + 1/4 up(c2 F2 + 1/4 up(c3 F3 + 1/4 up(c4 F4))))
// ------------------------------------------------------------------------------------------------
struct MsBwdArgs {
    const float* F[5];
    const float* coef;
    float* dx;
    int64_t total4;       // P * W * W / 4
};

template <int W>
__global__ __launch_bounds__(256) void msssim_bwd_kernel(MsBwdArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.total4) return;
    constexpr int W4 = W / 4;
    const int c = (int)(idx % W4) * 4, r = (int)((idx / W4) % W);
    const int64_t plane = idx / ((int64_t)W4 * W);
    float cf[5];
#pragma unroll
    for (int l = 0; l < 5; ++l) cf[l] = a.coef[l];
    // top level first, exactly the nesting of the avg_pool2d backward chain
    const float g4 = cf[4] * a.F[4][(plane * (W / 16) + (r >> 4)) * (W / 16) + (c >> 4)];
    const float g3 = cf[3] * a.F[3][(plane * (W / 8) + (r >> 3)) * (W / 8) + (c >> 3)] + 0.25f * g4;
    const float g2 = cf[2] * a.F[2][(plane * (W / 4) + (r >> 2)) * (W / 4) + (c >> 2)] + 0.25f * g3;
    const float2 f1 = *reinterpret_cast<const float2*>(a.F[1] + (plane * (W / 2) + (r >> 1)) * (W / 2) + (c >> 1));
    const float g1a = cf[1] * f1.x + 0.25f * g2, g1b = cf[1] * f1.y + 0.25f * g2;
    const f32x4 f0 = *reinterpret_cast<const f32x4*>(a.F[0] + (plane * W + r) * W + c);
    f32x4 o;
    o[0] = cf[0] * f0[0] + 0.25f * g1a; o[1] = cf[0] * f0[1] + 0.25f * g1a;
    o[2] = cf[0] * f0[2] + 0.25f * g1b; o[3] = cf[0] * f0[3] + 0.25f * g1b;
    *reinterpret_cast<f32x4*>(a.dx + (plane * W + r) * W + c) = o;
}

// ------------------------------------------------------------------------------------------------
// workspace carve (floats) and the launcher
// ------------------------------------------------------------------------------------------------
struct MsWs {
    int64_t pyrx[5], pyry[5], F[5], part[5], slab, coef, ticket, total;
    int nblk[5];
};
// every level writes one partial pair per plane: msssim_stream_kernel at 128 wide, msssim_plane_kernel below
static MsWs ms_carve(int width, int B) {
    MsWs w{};
    const int P = B * 3;
    int64_t off = 0;
    auto take = [&](int64_t n) { int64_t o = off; off += align_up(n, 64); return o; };
    for (int l = 0; l < 5; ++l) {
        const int S = width >> l;
        const int64_t n = (int64_t)P * S * S;
        if (l > 0) { w.pyrx[l] = take(n); w.pyry[l] = take(n); }
        w.F[l] = take(n);
        w.nblk[l] = P;
    }
    for (int l = 0; l < 5; ++l) w.part[l] = take((int64_t)w.nblk[l] * 2);
    w.slab = take(MS_NF * 11 * 2);
    w.coef = take(8);
    w.ticket = take(4);
    w.total = off;
    return w;
}
int64_t msssim_ws_floats(int width, int B) { return ms_carve(width, B).total; }

template <int S, bool LAST>
static int ms_fwd(const MsFwdArgs& a, hipStream_t st) {
    static DeviceOnce once;
    if (a.ticket) cvae_probe_begin(st);                 // level 0 only (the launch that also zeroes the ticket)
    if constexpr (S == 128) {
        using T = MsS<S, 16>;
        { int rc = cvae_grant_lds(once, reinterpret_cast<const void*>(msssim_stream_kernel<S, 16>), T::SMEM); if (rc) return rc; }
        const int resident = cvae_num_cus();                 // 135 KB of LDS: one workgroup per CU, persistent over the planes
        hipLaunchKernelGGL((msssim_stream_kernel<S, 16>), dim3(a.P < resident ? a.P : resident), dim3(T::NT), T::SMEM, st, a);
    } else {
        using T = MsP<S>;
        { int rc = cvae_grant_lds(once, reinterpret_cast<const void*>(msssim_plane_kernel<S, LAST>), T::SMEM); if (rc) return rc; }
        constexpr int byLds = (160 * 1024) / (T::SMEM + 256), byThreads = 2048 / T::NT;
        const int resident = cvae_num_cus() * (byLds < byThreads ? byLds : byThreads), ngroups = (a.P + T::PPW - 1) / T::PPW;
        hipLaunchKernelGGL((msssim_plane_kernel<S, LAST>), dim3(ngroups < resident ? ngroups : resident), dim3(T::NT), T::SMEM, st, a);
    }
    if (a.ticket) cvae_probe_end(st);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// stage (cross-rank path): 0 = the whole loss; 1 = pyramid + partial sums, the 11 fp64 sums into rec[0, 11) (no
// scalars, no gradients yet); 2 = finish from the summed rec and *images (the summed image count): scalars, coef,
// d_mu / d_logvar of this rank's rows, then the backward pass.  Stages 1 and 2 run on the same ws and tensors, in order.
int launch_msssim(int width, int B, const float* img1, const float* img2, const float* mu, const float* logvar,
                  float* ws, float* scalars, float* d_img1, float* d_mu, float* d_logvar, hipStream_t st,
                  int stage, double* rec, const double* images, const LossObjective* obj) {
    if (width != 64 && width != 128) { cvae_set_error("msssim: width %d unsupported", width); return -2; }
    int rc = 0;
    const MsWin win = make_window();
    const MsWs w = ms_carve(width, B);
    const int P = B * 3;
    const bool grad = d_img1 != nullptr;
    unsigned* ticket = reinterpret_cast<unsigned*>(ws + w.ticket);
    const LossObjective o = obj ? *obj : LossObjective{1.0f, 0.0f, MS_REF_KW, 0};
    // an MS-SSIM weight of exactly 0: no pyramid, no finalize, no F fields — the pixel pass finishes the KLD too.  Its
    // partials go to the slab and it draws from the ticket, which no earlier launch of this call has zeroed.
    if (o.w_ms == 0.0f) {
        hipError_t e = hipMemsetAsync(ticket, 0, sizeof(unsigned), st);
        if (e != hipSuccess) { cvae_set_error("msssim: ticket reset failed: %s", hipGetErrorString(e)); return (int)e; }
        return launch_objective_pixels(width, B, img1, img2, nullptr, nullptr, d_img1, mu, logvar, d_mu, d_logvar, o,
                                       reinterpret_cast<double*>(ws + w.slab), ticket, scalars, st);
    }
    const float* lx[5]; const float* ly[5];
    lx[0] = img1; ly[0] = img2;
    for (int l = 1; l < 5; ++l) { lx[l] = ws + w.pyrx[l]; ly[l] = ws + w.pyry[l]; }
    for (int l = 0; l < 5 && stage != 2; ++l) {
        const bool last = l == 4;
        MsFwdArgs a{lx[l], ly[l], last ? nullptr : ws + w.pyrx[l + 1], last ? nullptr : ws + w.pyry[l + 1],
                    grad ? ws + w.F[l] : nullptr, ws + w.part[l], l == 0 ? ticket : nullptr, P, win};
        switch (width >> l) {
            case 128: rc = ms_fwd<128, false>(a, st); break;
            case 64: rc = ms_fwd<64, false>(a, st); break;
            case 32: rc = ms_fwd<32, false>(a, st); break;
            case 16: rc = ms_fwd<16, false>(a, st); break;
            case 8: rc = last ? ms_fwd<8, true>(a, st) : ms_fwd<8, false>(a, st); break;
            default: rc = ms_fwd<4, true>(a, st); break;
        }
        if (rc) return rc;
    }
    MsFinArgs f{};
    for (int l = 0; l < 5; ++l) {
        f.part[l] = ws + w.part[l]; f.nblk[l] = w.nblk[l];
        f.count[l] = (double)P * (width >> l) * (width >> l);
    }
    f.mu = mu; f.logvar = logvar; f.B = mu ? B : 0; f.scalars = scalars; f.coef = ws + w.coef;
    f.slab = reinterpret_cast<double*>(ws + w.slab); f.ticket = ticket;
    f.d_mu = d_mu; f.d_logvar = d_logvar;
    f.rec = rec; f.images = images;
    f.kw = o.kw; f.w_ms = o.w_ms; f.used = o.used;
    if (stage == 0) hipLaunchKernelGGL(msssim_finalize_kernel<false>, dim3(MS_NF), dim3(256), 0, st, f);
    else if (stage == 1) { f.d_mu = f.d_logvar = nullptr; hipLaunchKernelGGL(msssim_finalize_kernel<true>, dim3(MS_NF), dim3(256), 0, st, f); }
    else hipLaunchKernelGGL(msssim_finish_kernel, dim3(cdiv(f.B * 32, 256) > 1 ? cdiv(f.B * 32, 256) : 1), dim3(256), 0, st, f, width);
    CVAE_CHECK_LAUNCH();
    // mixed objective: the pixel pass writes d_img1 (MS-SSIM chain + pixel gradient), the squared-error sum and the final
    // scalars [0] and [13].  The slab and the ticket are free again: the finalize's last arriver left the ticket at 0.
    if (o.w_mse != 0.0f) {
        const float* F[5];
        for (int l = 0; l < 5; ++l) F[l] = ws + w.F[l];
        return launch_objective_pixels(width, B, img1, img2, F, ws + w.coef, d_img1, nullptr, nullptr, nullptr, nullptr, o,
                                       reinterpret_cast<double*>(ws + w.slab), ticket, scalars, st);
    }
    if (!grad || stage == 1) return 0;
    MsBwdArgs b{};
    for (int l = 0; l < 5; ++l) b.F[l] = ws + w.F[l];
    b.coef = ws + w.coef; b.dx = d_img1; b.total4 = (int64_t)P * width * width / 4;
    const unsigned grid = (unsigned)((b.total4 + 255) / 256);
    if (width == 64) hipLaunchKernelGGL(msssim_bwd_kernel<64>, dim3(grid), dim3(256), 0, st, b);
    else hipLaunchKernelGGL(msssim_bwd_kernel<128>, dim3(grid), dim3(256), 0, st, b);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// what score.hip needs: where a values-only pyramid (launch_msssim, stage 1, no gradients) leaves its per-plane partial
// pairs, a scratch region it never touches, and the finish step on a caller-held record
// ------------------------------------------------------------------------------------------------
// part[l]: float offset of level l's (ssim, cs) pairs, 3 planes per image in image order; *scratch: the level-0 field F,
// which no kernel writes when d_img1 is null (3 * B * width^2 floats, 256-byte aligned like every slot)
void msssim_score_slots(int width, int B, int64_t part[5], int64_t* scratch) {
    const MsWs w = ms_carve(width, B);
    for (int l = 0; l < 5; ++l) part[l] = w.part[l];
    *scratch = w.F[0];
}
// msssim_finish_kernel on a pooled record: rec = 11 sums, *images = the image count they cover; writes CVAE_N_SCALARS
// scalars and the 5 coefficients (coef: 8 floats of the caller's)
int launch_msssim_finish_rec(int width, const double* rec, const double* images, float* scalars, float* coef, hipStream_t st) {
    if (width != 64 && width != 128) { cvae_set_error("msssim: width %d unsupported", width); return -2; }
    MsFinArgs f{};
    f.rec = const_cast<double*>(rec); f.images = images; f.scalars = scalars; f.coef = coef;
    hipLaunchKernelGGL(msssim_finish_kernel, dim3(1), dim3(256), 0, st, f, width);
    CVAE_CHECK_LAUNCH();
    return 0;
}
