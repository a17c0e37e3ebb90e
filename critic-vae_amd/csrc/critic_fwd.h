// critic_fwd.h — the device code of the critic's eval-mode forward, shared by critic_fwd_kernel (critic.hip: fp32 CHW frames
// from memory) and critic_score_kernel (critic_score.hip: uint8 HWC frames staged straight into LDS): one copy, so both
// kernels give the same bits for the same pixels.  One workgroup of 256 threads per image, every activation in LDS.
#pragma once
#include "common.h"

namespace critic_fwd {
using namespace critic_layout;

// LDS carve of one image, in floats: the zero-bordered input planes, the zero-bordered outputs of blocks 1..3, the
// un-bordered output of block 4, then features.14 (32) and crit.1 (32)
constexpr int X_FLOATS = 3 * 66 * 66, A1 = 8 * 34 * 34, A2 = 8 * 18 * 18, A3 = 8 * 10 * 10, A4 = 16 * 4 * 4;
constexpr int BORDERED_FLOATS = X_FLOATS + A1 + A2 + A3;           // what must be zero outside the interiors
constexpr int SMEM_BYTES = (BORDERED_FLOATS + A4 + 64) * 4;

// 3x3/pad-1 conv + ReLU + 2x2 max-pool from zero-bordered LDS planes in[CI][S+2][S+2] to zero-bordered
// LDS planes out[CO][S/2+2][S/2+2] (or un-bordered when BORDER_OUT == 0)
template <int CI, int CO, int S, int BORDER_OUT>
__device__ __forceinline__ void conv3_relu_pool(const float* in, float* out, const float* __restrict__ w,
                                                const float* __restrict__ b) {
    constexpr int SO = S / 2, PI = (S + 2) * (S + 2), WO = SO + 2 * BORDER_OUT, PO = WO * WO;
    for (int q = threadIdx.x; q < CO * SO * SO; q += 256) {
        const int co = q % CO, p = q / CO, py = p / SO, px = p % SO;
        float acc[4] = {b[co], b[co], b[co], b[co]};
        for (int ci = 0; ci < CI; ++ci) {
            const float* ip = in + ci * PI + (2 * py) * (S + 2) + 2 * px;      // top-left of the 4x4 input patch
            const float* wp = w + (co * CI + ci) * 9;
            float v[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) v[r][c] = ip[r * (S + 2) + c];
#pragma unroll
            for (int kr = 0; kr < 3; ++kr)
#pragma unroll
                for (int kc = 0; kc < 3; ++kc) {
                    const float wv = wp[kr * 3 + kc];
                    acc[0] = fmaf(wv, v[kr][kc], acc[0]); acc[1] = fmaf(wv, v[kr][kc + 1], acc[1]);
                    acc[2] = fmaf(wv, v[kr + 1][kc], acc[2]); acc[3] = fmaf(wv, v[kr + 1][kc + 1], acc[3]);
                }
        }
        const float m = fmaxf(fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3])), 0.f);   // ReLU then max == max then ReLU
        out[co * PO + (py + BORDER_OUT) * WO + px + BORDER_OUT] = m;
    }
}

// Everything behind the staged input planes: smem = the carve above with lx = smem filled (interior) and every border
// zero; the caller has met (__syncthreads) after staging.  Returns the sigmoid output in thread 0 (other threads: 0).
__device__ __forceinline__ float forward_from_lds(float* smem, const float* __restrict__ cp) {
    float* lx = smem;
    float* a1 = lx + X_FLOATS;
    float* a2 = a1 + A1;
    float* a3 = a2 + A2;
    float* a4 = a3 + A3;
    float* a5 = a4 + A4;          // 32
    float* f1 = a5 + 32;          // 32
    const int tid = threadIdx.x;
    conv3_relu_pool<3, 8, 64, 1>(lx, a1, cp + CW1, cp + CB1);
    __syncthreads();
    conv3_relu_pool<8, 8, 32, 1>(a1, a2, cp + CW2, cp + CB2);
    __syncthreads();
    conv3_relu_pool<8, 8, 16, 1>(a2, a3, cp + CW3, cp + CB3);
    __syncthreads();
    conv3_relu_pool<8, 16, 8, 0>(a3, a4, cp + CW4, cp + CB4);
    __syncthreads();
    // Conv(16,32,4) on the 4x4 map = a 256-long dot product per output; 8 lanes per output
    {
        const int o = tid >> 3, part = tid & 7;
        float acc = 0.f;
        for (int k = part; k < 256; k += 8) acc = fmaf(cp[CW5 + o * 256 + k], a4[k], acc);
        acc += __shfl_xor(acc, 1, 64); acc += __shfl_xor(acc, 2, 64); acc += __shfl_xor(acc, 4, 64);
        if (part == 0) a5[o] = fmaxf(acc + cp[CB5 + o], 0.f);
    }
    __syncthreads();
    if (tid < 32) {
        float acc = cp[CF1B + tid];
        for (int k = 0; k < 32; ++k) acc = fmaf(cp[CF1W + tid * 32 + k], a5[k], acc);
        f1[tid] = fmaxf(acc, 0.f);
    }
    __syncthreads();
    float p = 0.f;
    if (tid == 0) {
        float acc = cp[CF2B];
        for (int k = 0; k < 32; ++k) acc = fmaf(cp[CF2W + k], f1[k], acc);
        p = 1.0f / (1.0f + expf(-acc));
    }
    return p;
}
}  // namespace critic_fwd
