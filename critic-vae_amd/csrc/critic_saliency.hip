// critic_saliency.hip — what the critic alone says about a frame (cvae_critic_collect, cvae_critic_saliency,
// cvae_critic_occlusion; include/cvae.h): its pooled feature maps, the gradient of its logit with respect to the pixels
// (plain or integrated from the black frame) and the drop of its value when a patch is covered.
//
// Three persistent kernels, one workgroup of 256 threads per image, every activation in LDS (one workgroup per compute
// unit: 104 .. 118 KB).  collect and occlusion run critic_fwd.h's forward (the device code of cvae_critic_forward: the same
// bits); saliency runs critic_bwd.h's recorded forward and input-gradient chain (the device code of cvae_critic_grad: the
// same decisions) and adds the one step that kernel stops short of, the input gradient of features.0.
//
// saliency keeps the frame's gradient in REGISTERS: element e = tid + 256 i of the dense (3,64,64) gradient belongs to
// thread tid, 48 accumulators, so a thread holds the three colours of its 16 pixels, the input planes are never written
// by the backward (their border stays zero for every pass and every image) and the integrated-gradients sum runs in
// pass order.  The backward does overwrite the planes of blocks 1..3 with dense gradients: they are zeroed before
// every pass, as critic_train_kernel does before every image.
#include "common.h"
#include "critic_fwd.h"
#include "critic_bwd.h"

namespace {
using namespace critic_layout;
using critic_bwd::X_FLOATS; using critic_bwd::A1; using critic_bwd::A2; using critic_bwd::A3; using critic_bwd::A4;
using critic_bwd::WST; using critic_bwd::DECISIONS;
using critic_bwd::D1; using critic_bwd::D2; using critic_bwd::D3; using critic_bwd::D4; using critic_bwd::D5; using critic_bwd::DF;

// the frame's fp32 CHW planes times `scale` into the interiors of the zero-bordered LDS planes (critic_fwd_kernel's staging;
// scale == 1 leaves the bits as they are)
__device__ __forceinline__ void stage_frame(float* lx, const float* __restrict__ xb, float scale) {
    for (int q = threadIdx.x; q < 3 * 64 * 16; q += 256) {
        const int c4 = q & 15, row = (q >> 4) & 63, c = q >> 10;
        const float4 v = *reinterpret_cast<const float4*>(xb + (c * 64 + row) * 64 + c4 * 4);
        float* d = lx + c * 66 * 66 + (row + 1) * 66 + c4 * 4 + 1;
        d[0] = v.x * scale; d[1] = v.y * scale; d[2] = v.z * scale; d[3] = v.w * scale;
    }
}

// the workgroup's maximum of v in every thread; red: 4 floats of LDS nobody else touches around the call
__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return v;
}

// ---------------------------------------------------------------- collect ----------------------------------------------------------------
struct CollectArgs {
    const float* x; const float* cp; float* pred; float* e[5]; int B;
};

// the interior of zero-bordered (BORDER = 1) or plain planes src[C][S + 2 BORDER][..] to dense dst[C][S][S]
template <int C, int S, int BORDER>
__device__ __forceinline__ void copy_interior(const float* src, float* __restrict__ dst) {
    constexpr int W = S + 2 * BORDER;
    for (int q = threadIdx.x; q < C * S * S; q += 256) {
        const int c = q / (S * S), y = (q / S) % S, xx = q % S;
        dst[q] = src[c * W * W + (y + BORDER) * W + xx + BORDER];
    }
}

__global__ __launch_bounds__(256) void critic_collect_kernel(const CollectArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    float* a1 = smem + critic_fwd::X_FLOATS;
    float* a2 = a1 + critic_fwd::A1;
    float* a3 = a2 + critic_fwd::A2;
    float* a4 = a3 + critic_fwd::A3;
    float* a5 = a4 + critic_fwd::A4;
    for (int q = tid; q < critic_fwd::BORDERED_FLOATS; q += 256) smem[q] = 0.f;      // zero borders, once per workgroup
    __syncthreads();
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        stage_frame(smem, a.x + (size_t)b * 3 * 64 * 64, 1.0f);
        __syncthreads();
        const float p = critic_fwd::forward_from_lds(smem, a.cp);
        if (tid == 0) a.pred[b] = p;
        if (a.e[0]) copy_interior<8, 32, 1>(a1, a.e[0] + (size_t)b * 8 * 32 * 32);
        if (a.e[1]) copy_interior<8, 16, 1>(a2, a.e[1] + (size_t)b * 8 * 16 * 16);
        if (a.e[2]) copy_interior<8, 8, 1>(a3, a.e[2] + (size_t)b * 8 * 8 * 8);
        if (a.e[3]) copy_interior<16, 4, 0>(a4, a.e[3] + (size_t)b * 16 * 4 * 4);
        if (a.e[4] && tid < 32) a.e[4][(size_t)b * 32 + tid] = a5[tid];
        __syncthreads();                         // the next frame's staging and forward overwrite the planes
    }
}

// ---------------------------------------------------------------- saliency ---------------------------------------------------------------
constexpr int SAL_FLOATS = X_FLOATS + A1 + A2 + A3 + A4 + 32 + 32 + WST + 32 + 32 + 8;
constexpr int SAL_BYTES = SAL_FLOATS * 4 + DECISIONS;

struct SaliencyArgs {
    const float* x; const float* cp; float* pred; float* grad; float* map; float* max_values; uint8_t* decisions;
    int B, steps;
};

// acc[i] += the gradient of input element e = tid + 256 i of features.0 (dense (3,64,64)): dgrad3 of critic_bwd.h for
// CI = 3, S = 64 without a previous pool or ReLU to mask with, kept in registers instead of a plane
// The three colours of a pixel meet the same windows, decisions and dp and differ in the weight alone, so a thread walks its
// 16 pixels and keeps three sums; a window that contributes nothing (outside the map, closed, or selected outside the
// footprint) is read at a safe index and dropped by a select, so the loads of a pixel do not wait for one another.
__device__ __forceinline__ void dgrad3_input(const float* w, const float* dp, const uint8_t* dec, float (&acc)[48]) {
    constexpr int CI = 3, CO = 8, S = 64, SO = 32, NWIN = SO * SO;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int pix = threadIdx.x + 256 * j, y = pix / S, x = pix % S;
        const int wy0 = (y - 1) >> 1, wx0 = (x - 1) >> 1;
        float s[CI] = {0.f, 0.f, 0.f};
#pragma unroll 4
        for (int co = 0; co < CO; ++co) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int wy = wy0 + a, wx = wx0 + c;
                    const bool inside = (unsigned)wy < (unsigned)SO && (unsigned)wx < (unsigned)SO;
                    const int wi = inside ? co * NWIN + wy * SO + wx : co * NWIN;
                    const int d = dec[wi];
                    const int kr = y + 1 - (2 * wy + (d >> 1)), kc = x + 1 - (2 * wx + (d & 1));
                    const bool hit = inside && d < 4 && (unsigned)kr < 3u && (unsigned)kc < 3u;
                    const int k = hit ? kr * 3 + kc : 0;
                    const float g = dp[wi];
#pragma unroll
                    for (int ci = 0; ci < CI; ++ci) {
                        const float v = fmaf(g, w[(co * CI + ci) * 9 + k], s[ci]);
                        s[ci] = hit ? v : s[ci];
                    }
                }
        }
#pragma unroll
        for (int ci = 0; ci < CI; ++ci) acc[16 * ci + j] += s[ci];
    }
}

__global__ __launch_bounds__(256) void critic_saliency_kernel(const SaliencyArgs a) {
    using namespace critic_bwd;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* lx = smem;
    float* a1 = lx + X_FLOATS;
    float* a2 = a1 + A1;
    float* a3 = a2 + A2;
    float* a4 = a3 + A3;
    float* a5 = a4 + A4;          // 32
    float* f1 = a5 + 32;          // 32
    float* wst = f1 + 32;         // one layer's weights
    float* d5 = wst + WST;        // 32: gradient of features.14's pre-activation
    float* df1 = d5 + 32;         // 32: gradient of crit.1's pre-activation
    float* misc = df1 + 32;       // [0..3]: block_max
    uint8_t* dec = reinterpret_cast<uint8_t*>(misc + 8);
    const int tid = threadIdx.x, N = a.steps;
    const float* __restrict__ cp = a.cp;
    const float invN = 1.0f / (float)N;

    for (int q = tid; q < X_FLOATS; q += 256) lx[q] = 0.f;       // the frame's border stays zero: only the staging writes lx
    __syncthreads();

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float* xb = a.x + (size_t)b * 3 * 64 * 64;
        float acc[48];
#pragma unroll
        for (int i = 0; i < 48; ++i) acc[i] = 0.f;
        for (int k = 1; k <= N; ++k) {
            // ---------------- forward at x * (k / N): critic_train_kernel's, every element kept and unscaled ----------------
            for (int q = tid; q < A1 + A2 + A3; q += 256) a1[q] = 0.f;       // borders (the backward overwrote the planes)
            stage_frame(lx, xb, (float)k / (float)N);                        // k == N: 1.0f, the frame itself
            stage(wst, cp + CW1, 216);
            __syncthreads();
            conv3_relu_pool_dec<3, 8, 64, 1, false>(lx, a1, wst, cp + CB1, dec + D1, nullptr);
            __syncthreads();
            stage(wst, cp + CW2, 576);
            __syncthreads();
            conv3_relu_pool_dec<8, 8, 32, 1, false>(a1, a2, wst, cp + CB2, dec + D2, nullptr);
            __syncthreads();
            stage(wst, cp + CW3, 576);
            __syncthreads();
            conv3_relu_pool_dec<8, 8, 16, 1, false>(a2, a3, wst, cp + CB3, dec + D3, nullptr);
            __syncthreads();
            stage(wst, cp + CW4, 1152);
            __syncthreads();
            conv3_relu_pool_dec<8, 16, 8, 0, false>(a3, a4, wst, cp + CB4, dec + D4, nullptr);
            __syncthreads();
            {   // Conv(16,32,4) on the 4x4 map, critic_fwd_kernel's 8 lanes per output
                const int o = tid >> 3, part = tid & 7;
                float s = 0.f;
                for (int j = part; j < 256; j += 8) s = fmaf(cp[CW5 + o * 256 + j], a4[j], s);
                s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
                if (part == 0) {
                    const float pre = s + cp[CB5 + o];
                    dec[D5 + o] = pre > 0.f;
                    a5[o] = fmaxf(pre, 0.f);
                }
            }
            __syncthreads();
            if (tid < 32) {
                float s = cp[CF1B + tid];
                for (int j = 0; j < 32; ++j) s = fmaf(cp[CF1W + tid * 32 + j], a5[j], s);
                dec[DF + tid] = s > 0.f;
                f1[tid] = fmaxf(s, 0.f);
            }
            __syncthreads();
            if (k == N) {                        // the pass on x itself: its value and its decisions are the call's
                if (tid == 0) {
                    float s = cp[CF2B];
                    for (int j = 0; j < 32; ++j) s = fmaf(cp[CF2W + j], f1[j], s);
                    a.pred[b] = 1.0f / (1.0f + expf(-s));
                }
                if (a.decisions) {
                    uint32_t* dst = reinterpret_cast<uint32_t*>(a.decisions + (size_t)b * DECISIONS);
                    const uint32_t* src = reinterpret_cast<const uint32_t*>(dec);
                    for (int q = tid; q < DECISIONS / 4; q += 256) dst[q] = src[q];
                }
            }
            // ---------------- backward of the logit: d z = 1 ----------------
            if (tid < 32) df1[tid] = dec[DF + tid] ? cp[CF2W + tid] : 0.f;
            __syncthreads();
            if (tid < 32) {
                float g = 0.f;
                for (int j = 0; j < 32; ++j) g = fmaf(df1[j], cp[CF1W + j * 32 + tid], g);
                d5[tid] = dec[D5 + tid] ? g : 0.f;
            }
            __syncthreads();
            {   // features.14: thread tid owns input element tid (weight column tid); dp4 replaces a4 in place
                float g = 0.f;
#pragma unroll 8
                for (int i = 0; i < 32; ++i) g = fmaf(d5[i], cp[CW5 + i * 256 + tid], g);
                a4[tid] = dec[D4 + tid] != 4 ? g : 0.f;
            }
            __syncthreads();
            dgrad3<8, 16, 8, false>(wst, a4, dec + D4, dec + D3, nullptr, a3);      // wst still holds features.10.weight
            __syncthreads();
            stage(wst, cp + CW3, 576);
            __syncthreads();
            dgrad3<8, 8, 16, false>(wst, a3, dec + D3, dec + D2, nullptr, a2);
            __syncthreads();
            stage(wst, cp + CW2, 576);
            __syncthreads();
            dgrad3<8, 8, 32, false>(wst, a2, dec + D2, dec + D1, nullptr, a1);
            __syncthreads();
            stage(wst, cp + CW1, 216);
            __syncthreads();
            dgrad3_input(wst, a1, dec + D1, acc);
            __syncthreads();                     // the next pass zeroes a1 and stages over lx and wst
        }
        // ---------------- the frame's gradient, its grey map and the map's maximum ----------------
        float* gb = a.grad ? a.grad + (size_t)b * 3 * 64 * 64 : nullptr;
        float* mb = a.map + (size_t)b * 64 * 64;
        float mx = 0.f;                          // the map is non-negative
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int pix = tid + 256 * j;
            float g[3] = {acc[j], acc[16 + j], acc[32 + j]};
            if (N > 1) {                         // integrated gradients: x is read again from memory, not from the scaled planes
#pragma unroll
                for (int c = 0; c < 3; ++c) g[c] = g[c] * xb[c * 4096 + pix] * invN;
            }
            if (gb) { gb[pix] = g[0]; gb[4096 + pix] = g[1]; gb[2 * 4096 + pix] = g[2]; }
            const float m = fabsf(g[0]) * 0.2989f + fabsf(g[1]) * 0.5870f + fabsf(g[2]) * 0.1140f;
            mb[pix] = m;
            mx = fmaxf(mx, m);
        }
        mx = block_max(mx, misc);
        if (tid == 0) a.max_values[b] = mx;
    }
}

// ---------------------------------------------------------------- occlusion --------------------------------------------------------------
// behind critic_fwd's carve: the patch set aside (3 x 16 x 16 at most), the drops of the frame's patches (256 at most), p
constexpr int OCC_SAVE = critic_fwd::SMEM_BYTES / 4, OCC_DROP = OCC_SAVE + 768, OCC_P = OCC_DROP + 256;
constexpr int OCC_BYTES = (OCC_P + 4) * 4;

struct OcclusionArgs {
    const float* x; const float* cp; float* pred; float* drop; float* map; float* max_values;
    float fill[3]; int B, patch;
};

__global__ __launch_bounds__(256) void critic_occlusion_kernel(const OcclusionArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* lx = smem;
    float* save = smem + OCC_SAVE;
    float* drops = smem + OCC_DROP;
    float* pbox = smem + OCC_P;
    const int tid = threadIdx.x, P = a.patch, G = 64 / P, NP = G * G, PP = P * P;
    for (int q = tid; q < critic_fwd::BORDERED_FLOATS; q += 256) smem[q] = 0.f;      // zero borders, once per workgroup
    __syncthreads();
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        stage_frame(lx, a.x + (size_t)b * 3 * 64 * 64, 1.0f);
        __syncthreads();
        const float p0 = critic_fwd::forward_from_lds(smem, a.cp);
        if (tid == 0) { a.pred[b] = p0; pbox[0] = p0; }
        for (int n = 0; n <= NP; ++n) {
            // put patch n - 1 back, set patch n aside and fill it: cell q of either patch belongs to thread q % 256, and the
            // patches do not overlap, so no thread reads what another writes here
            for (int q = tid; q < 3 * PP; q += 256) {
                const int c = q / PP, r = (q % PP) / P, cc = q % P;
                if (n > 0) {
                    const int py = (n - 1) / G, px = (n - 1) % G;
                    lx[c * 66 * 66 + (py * P + r + 1) * 66 + px * P + cc + 1] = save[q];
                }
                if (n < NP) {
                    const int py = n / G, px = n % G;
                    float* cell = lx + c * 66 * 66 + (py * P + r + 1) * 66 + px * P + cc + 1;
                    save[q] = *cell;
                    *cell = a.fill[c];
                }
            }
            __syncthreads();
            if (n == NP) break;                  // every patch is back: the planes hold the frame again
            const float p = critic_fwd::forward_from_lds(smem, a.cp);
            if (tid == 0) drops[n] = pbox[0] - p;
        }
        // thread 0 wrote pbox and drops; the break above followed a barrier, and every forward ends behind one
        __syncthreads();
        float* db = a.drop + (size_t)b * NP;
        for (int q = tid; q < NP; q += 256) db[q] = drops[q];
        float* mb = a.map + (size_t)b * 64 * 64;
        float mx = 0.f;
        for (int q = tid; q < 64 * 64; q += 256) {
            const float m = fmaxf(drops[((q >> 6) / P) * G + (q & 63) / P], 0.f);
            mb[q] = m;
            mx = fmaxf(mx, m);
        }
        mx = block_max(mx, pbox);                // pbox[0] was last read before the barrier above; ends with a barrier
        if (tid == 0) a.max_values[b] = mx;
    }
}

}  // namespace

int launch_critic_collect(int B, const float* x, const float* critic_params, float* pred, float* const e[5], hipStream_t st) {
    static DeviceOnce once;
    { int rc = cvae_grant_lds(once, reinterpret_cast<const void*>(critic_collect_kernel), critic_fwd::SMEM_BYTES); if (rc) return rc; }
    const CollectArgs a{x, critic_params, pred, {e[0], e[1], e[2], e[3], e[4]}, B};
    hipLaunchKernelGGL(critic_collect_kernel, dim3(persistent_grid(1, B)), dim3(256), critic_fwd::SMEM_BYTES, st, a);
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_critic_saliency(int B, const float* x, const float* critic_params, int steps, float* pred, float* grad, float* map,
                           float* max_values, uint8_t* decisions, hipStream_t st) {
    static_assert(SAL_BYTES <= 160 * 1024 && OCC_BYTES <= 160 * 1024, "a workgroup may declare at most 160 KiB of LDS");
    static DeviceOnce once;
    { int rc = cvae_grant_lds(once, reinterpret_cast<const void*>(critic_saliency_kernel), SAL_BYTES); if (rc) return rc; }
    const SaliencyArgs a{x, critic_params, pred, grad, map, max_values, decisions, B, steps};
    hipLaunchKernelGGL(critic_saliency_kernel, dim3(persistent_grid(1, B)), dim3(256), SAL_BYTES, st, a);
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_critic_occlusion(int B, const float* x, const float* critic_params, int patch, float fill_r, float fill_g, float fill_b,
                            float* pred, float* drop, float* map, float* max_values, hipStream_t st) {
    static DeviceOnce once;
    { int rc = cvae_grant_lds(once, reinterpret_cast<const void*>(critic_occlusion_kernel), OCC_BYTES); if (rc) return rc; }
    const OcclusionArgs a{x, critic_params, pred, drop, map, max_values, {fill_r, fill_g, fill_b}, B, patch};
    hipLaunchKernelGGL(critic_occlusion_kernel, dim3(persistent_grid(1, B)), dim3(256), OCC_BYTES, st, a);
    CVAE_CHECK_LAUNCH();
    return 0;
}
