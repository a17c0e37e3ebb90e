// critic_train.hip — one training step of the critic CNN (critic_net.py:5-59, train mode): forward with explicit
// Dropout masks, BCE / MSE loss and the gradient of every parameter, in one persistent kernel plus a finalize.
//
// A workgroup walks images b = wg, wg + G, ...  Per image every activation lives in LDS (critic_fwd_kernel's planes
// and arithmetic, so the eval-mode prediction is the eval kernel's), the forward records its discrete choices (which
// element each 2x2 max-pool window selected, which ReLUs were open), and the backward reuses each activation plane for
// the gradient of the pooled tensor it held once its consumer's weight gradient has been taken:
//     wgrad_l (reads a_{l-1}, dp_l)  ->  dgrad_l (reads dp_l, W_l; writes dp_{l-1} over a_{l-1})  ->  wgrad_{l-1} ...
// After the pool d_y of a conv has at most one nonzero per 2x2 window, at the position of its decision byte, so a
// weight gradient is a sum over S/2 x S/2 windows and an input gradient reads the 4 windows its 3x3 footprint meets.
// Weight gradients accumulate in REGISTERS across the workgroup's images (thread t owns flat parameters t + 256 i
// of each layer: 50 accumulators), are stored once per workgroup into scratch and summed over the workgroups in a
// fixed order by critic_train_finalize_kernel: no floating-point atomics, the same inputs give the same bits.
#include "common.h"
#include "critic_bwd.h"

namespace {
using namespace critic_layout;
using namespace critic_bwd;

constexpr int TRAIN_FLOATS = 11876, MAX_GRID = 256;
// LDS floats: critic_fwd_kernel's planes, then keep scales, one layer's staged weights, d5, df1, (p, dz) and the decision bytes
constexpr int LDS_FLOATS = X_FLOATS + A1 + A2 + A3 + A4 + 32 + 32 + KEEP + WST + 32 + 32 + 8;
constexpr int LDS_BYTES = LDS_FLOATS * 4 + DECISIONS;

struct TrainArgs {
    const float* x; const float* target; const uint8_t* keep; const float* cp;
    float* pred; uint8_t* decisions; float* partials; float* terms;          // terms: (2, B) per-image BCE and MSE
    int B, loss_kind; float scale;
};

__global__ __launch_bounds__(256) void critic_train_kernel(const TrainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* lx = smem;
    float* a1 = lx + X_FLOATS;
    float* a2 = a1 + A1;
    float* a3 = a2 + A2;
    float* a4 = a3 + A3;
    float* a5 = a4 + A4;          // 32
    float* f1 = a5 + 32;          // 32, after crit.3's Dropout
    float* ks = f1 + 32;          // 800: kept ? scale : 0
    float* wst = ks + KEEP;       // one layer's weights
    float* d5 = wst + WST;        // 32: gradient of features.14's pre-activation
    float* df1 = d5 + 32;         // 32: gradient of crit.1's pre-activation
    float* misc = df1 + 32;       // [0] = d_z
    uint8_t* dec = reinterpret_cast<uint8_t*>(misc + 8);
    const int tid = threadIdx.x, G = gridDim.x;
    const float* __restrict__ cp = a.cp;

    float acc1[1] = {}, acc2[3] = {}, acc3[3] = {}, acc4[5] = {}, acc5[32] = {}, accf[4] = {};
    float accb5 = 0.f, accbf = 0.f, accw2 = 0.f, accb2 = 0.f;
    float w5r[32];                // column tid of features.14.weight (32 x 256), for its input gradient
#pragma unroll
    for (int i = 0; i < 32; ++i) w5r[i] = cp[CW5 + i * 256 + tid];

    for (int q = tid; q < X_FLOATS; q += 256) lx[q] = 0.f;       // the frame's border stays zero for every image
    __syncthreads();                                             // other threads store the first frame into these cells

    for (int b = blockIdx.x; b < a.B; b += G) {
        // ---------------- forward ----------------
        for (int q = tid; q < A1 + A2 + A3; q += 256) a1[q] = 0.f;           // borders (the backward overwrote the planes)
        {
            const uint8_t* kb = a.keep ? a.keep + (size_t)b * KEEP : nullptr;
            for (int q = tid; q < KEEP; q += 256) ks[q] = (!kb || kb[q]) ? a.scale : 0.f;
        }
        const float* xb = a.x + (size_t)b * 3 * 64 * 64;
        for (int q = tid; q < 3 * 64 * 16; q += 256) {
            const int c4 = q & 15, row = (q >> 4) & 63, c = q >> 10;
            const float4 v = *reinterpret_cast<const float4*>(xb + (c * 64 + row) * 64 + c4 * 4);
            float* d = lx + c * 66 * 66 + (row + 1) * 66 + c4 * 4 + 1;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
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
        conv3_relu_pool_dec<8, 8, 16, 1, true>(a2, a3, wst, cp + CB3, dec + D3, ks + KS3);
        __syncthreads();
        stage(wst, cp + CW4, 1152);
        __syncthreads();
        conv3_relu_pool_dec<8, 16, 8, 0, true>(a3, a4, wst, cp + CB4, dec + D4, ks + KS4);
        __syncthreads();
        {   // Conv(16,32,4) on the 4x4 map, critic_fwd_kernel's 8 lanes per output
            const int o = tid >> 3, part = tid & 7;
            float acc = 0.f;
            for (int k = part; k < 256; k += 8) acc = fmaf(cp[CW5 + o * 256 + k], a4[k], acc);
            acc += __shfl_xor(acc, 1, 64); acc += __shfl_xor(acc, 2, 64); acc += __shfl_xor(acc, 4, 64);
            if (part == 0) {
                const float pre = acc + cp[CB5 + o];
                dec[D5 + o] = pre > 0.f;
                a5[o] = fmaxf(pre, 0.f);
            }
        }
        __syncthreads();
        if (tid < 32) {
            float acc = cp[CF1B + tid];
            for (int k = 0; k < 32; ++k) acc = fmaf(cp[CF1W + tid * 32 + k], a5[k], acc);
            dec[DF + tid] = acc > 0.f;
            f1[tid] = fmaxf(acc, 0.f) * ks[KSF + tid];
        }
        __syncthreads();
        if (tid == 0) {
            float acc = cp[CF2B];
            for (int k = 0; k < 32; ++k) acc = fmaf(cp[CF2W + k], f1[k], acc);
            const float p = 1.0f / (1.0f + expf(-acc)), t = a.target[b], invB = 1.0f / (float)a.B;
            a.pred[b] = p;
            // torch's binary_cross_entropy: both logs clamped at -100
            a.terms[b] = -(t * fmaxf(logf(p), -100.f) + (1.f - t) * fmaxf(log1pf(-p), -100.f));
            a.terms[(size_t)a.B + b] = (p - t) * (p - t);
            const float pq = p * (1.f - p);
            // torch's arithmetic: binary_cross_entropy_backward, then sigmoid_backward (a saturated sigmoid gives 0)
            const float dpred = a.loss_kind == 0 ? (p - t) / fmaxf(pq, 1e-12f) * invB : 2.f * (p - t) * invB;
            misc[0] = dpred * pq;
        }
        __syncthreads();
        if (a.decisions) {
            uint32_t* dst = reinterpret_cast<uint32_t*>(a.decisions + (size_t)b * DECISIONS);
            const uint32_t* src = reinterpret_cast<const uint32_t*>(dec);
            for (int q = tid; q < DECISIONS / 4; q += 256) dst[q] = src[q];
        }
        // ---------------- backward ----------------
        if (tid < 32) {
            const float dz = misc[0];
            accw2 += dz * f1[tid];
            if (tid == 0) accb2 += dz;
            const float g = dec[DF + tid] ? dz * cp[CF2W + tid] * ks[KSF + tid] : 0.f;
            df1[tid] = g;
            accbf += g;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) accf[i] = fmaf(df1[(tid >> 5) + 8 * i], a5[tid & 31], accf[i]);
        if (tid < 32) {
            float g = 0.f;
            for (int j = 0; j < 32; ++j) g = fmaf(df1[j], cp[CF1W + j * 32 + tid], g);
            g = dec[D5 + tid] ? g : 0.f;
            d5[tid] = g;
            accb5 += g;
        }
        __syncthreads();
        {   // features.14: thread tid owns input element tid (weight column tid); dp4 replaces a4 in place
            const float av = a4[tid];
            float g = 0.f;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const float d = d5[i];
                acc5[i] = fmaf(d, av, acc5[i]);
                g = fmaf(d, w5r[i], g);
            }
            a4[tid] = dec[D4 + tid] != 4 ? g * ks[KS4 + tid] : 0.f;
        }
        __syncthreads();
        wgrad3<8, 16, 8>(a3, a4, dec + D4, acc4);                      // wst still holds features.10.weight
        __syncthreads();
        dgrad3<8, 16, 8, true>(wst, a4, dec + D4, dec + D3, ks + KS3, a3);
        __syncthreads();
        stage(wst, cp + CW3, 576);
        wgrad3<8, 8, 16>(a2, a3, dec + D3, acc3);
        __syncthreads();
        dgrad3<8, 8, 16, false>(wst, a3, dec + D3, dec + D2, nullptr, a2);
        __syncthreads();
        stage(wst, cp + CW2, 576);
        wgrad3<8, 8, 32>(a1, a2, dec + D2, acc2);
        __syncthreads();
        dgrad3<8, 8, 32, false>(wst, a2, dec + D2, dec + D1, nullptr, a1);
        __syncthreads();
        wgrad3<3, 8, 64>(lx, a1, dec + D1, acc1);
        __syncthreads();
    }

    // one partial per workgroup, every slot written (a workgroup always has at least one image: G <= B)
    float* part = a.partials + (size_t)blockIdx.x * TRAIN_FLOATS;
    if (tid < 224) part[CW1 + tid] = acc1[0];
#pragma unroll
    for (int i = 0; i < 3; ++i) if (tid + 256 * i < 584) { part[CW2 + tid + 256 * i] = acc2[i]; part[CW3 + tid + 256 * i] = acc3[i]; }
#pragma unroll
    for (int i = 0; i < 5; ++i) if (tid + 256 * i < 1168) part[CW4 + tid + 256 * i] = acc4[i];
#pragma unroll
    for (int i = 0; i < 32; ++i) part[CW5 + tid + 256 * i] = acc5[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) part[CF1W + tid + 256 * i] = accf[i];
    if (tid < 32) { part[CB5 + tid] = accb5; part[CF1B + tid] = accbf; part[CF2W + tid] = accw2; }
    if (tid == 0) part[CF2B] = accb2;
}

// grads[i] = the partials of workgroups 0 .. G-1 summed in that order (fp64), padding = 0; the last workgroup
// merges the per-image loss terms: strided fp64 sums per thread, then a fixed tree
__global__ __launch_bounds__(256) void critic_train_finalize_kernel(const float* __restrict__ partials, int G, const float* __restrict__ terms,
                                                                    int B, int loss_kind, float* __restrict__ grads, float* __restrict__ scalars) {
    const int tid = threadIdx.x;
    if (blockIdx.x + 1 < gridDim.x) {
        const int i = blockIdx.x * 256 + tid;
        if (i >= TRAIN_FLOATS) return;
        if (i >= CRITIC_PARAMS) { grads[i] = 0.f; return; }      // the workgroups never write the padding slots of a partial
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += (double)partials[(size_t)g * TRAIN_FLOATS + i];
        grads[i] = (float)s;
        return;
    }
    __shared__ double red[2][256];
    double sb = 0.0, sm = 0.0;
    for (int b = tid; b < B; b += 256) { sb += (double)terms[b]; sm += (double)terms[(size_t)B + b]; }
    red[0][tid] = sb; red[1][tid] = sm;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        const float bce = (float)(red[0][0] / B), mse = (float)(red[1][0] / B);
        scalars[0] = loss_kind == 0 ? bce : mse; scalars[1] = bce; scalars[2] = mse; scalars[3] = 0.f;
    }
}

}  // namespace

int critic_train_floats() { return TRAIN_FLOATS; }

// partials of at most MAX_GRID workgroups, then the (2, B) loss terms
int64_t critic_grad_scratch_bytes(int B) {
    const int64_t slots = B < MAX_GRID ? B : MAX_GRID;
    return align_up((slots * TRAIN_FLOATS + 2 * (int64_t)B) * 4, 256);
}

int launch_critic_grad(int width, int B, const float* x, const float* target, const uint8_t* keep, float scale, int loss_kind,
                       const float* critic_params, float* grads, float* pred, float* loss_scalars, uint8_t* decisions,
                       void* scratch, hipStream_t st) {
    if (width != 64) { cvae_set_error("critic: width %d unsupported (the reference critic is 64x64 only)", width); return -2; }
    static_assert(LDS_BYTES <= 160 * 1024, "a workgroup may declare at most 160 KiB of LDS");
    static DeviceOnce once;
    { int rc = cvae_grant_lds(once, reinterpret_cast<const void*>(critic_train_kernel), LDS_BYTES); if (rc) return rc; }
    int G = persistent_grid(1, B);
    if (G > MAX_GRID) G = MAX_GRID;
    float* partials = static_cast<float*>(scratch);
    float* terms = partials + (size_t)(B < MAX_GRID ? B : MAX_GRID) * TRAIN_FLOATS;
    const TrainArgs a{x, target, keep, critic_params, pred, decisions, partials, terms, B, loss_kind, scale};
    hipLaunchKernelGGL(critic_train_kernel, dim3(G), dim3(256), LDS_BYTES, st, a);
    CVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(critic_train_finalize_kernel, dim3(cdiv(TRAIN_FLOATS, 256) + 1), dim3(256), 0, st, partials, G, terms, B,
                       loss_kind, grads, loss_scalars);
    CVAE_CHECK_LAUNCH();
    return 0;
}
