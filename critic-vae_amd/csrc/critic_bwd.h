// critic_bwd.h — the device code of the critic's recorded forward and its backward, shared by critic_train_kernel
// (critic_train.hip: every parameter's gradient) and critic_saliency_kernel (critic_saliency.hip: the gradient of the logit
// with respect to the pixels): one copy, so both kernels take the same decisions and give the same bits for the same frame.
// One workgroup of 256 threads per image, critic_fwd.h's LDS planes.
#pragma once
#include "common.h"

namespace critic_bwd {
using namespace critic_layout;

constexpr int KEEP = 800, DECISIONS = 11072;
constexpr int KS3 = 0, KS4 = 512, KSF = 768;                                   // Dropout sites: features.9, features.13, crit.3
constexpr int D1 = 0, D2 = 8192, D3 = 10240, D4 = 10752, D5 = 11008, DF = 11040;   // decision byte offsets
// LDS floats of critic_fwd_kernel's planes, and of one layer's staged weights (features.10 is the largest)
constexpr int X_FLOATS = 3 * 66 * 66, A1 = 8 * 34 * 34, A2 = 8 * 18 * 18, A3 = 8 * 10 * 10, A4 = 16 * 4 * 4;
constexpr int WST = 1152;

__device__ __forceinline__ void stage(float* wst, const float* __restrict__ w, int n) {
    for (int q = threadIdx.x; q < n; q += 256) wst[q] = w[q];
}

// conv3_relu_pool of critic.hip (the same operation order) with weights staged in LDS; records the window's choice
// (first maximum in scan order; 4 = maximum <= 0) and applies the Dropout scale of the pooled tensor when DROP
template <int CI, int CO, int S, int BORDER_OUT, bool DROP>
__device__ __forceinline__ void conv3_relu_pool_dec(const float* in, float* out, const float* w, const float* __restrict__ b,
                                                    uint8_t* dec, const float* ks) {
    constexpr int SO = S / 2, PI = (S + 2) * (S + 2), WO = SO + 2 * BORDER_OUT, PO = WO * WO;
    for (int q = threadIdx.x; q < CO * SO * SO; q += 256) {
        const int co = q % CO, p = q / CO, py = p / SO, px = p % SO;
        float acc[4] = {b[co], b[co], b[co], b[co]};
        for (int ci = 0; ci < CI; ++ci) {
            const float* ip = in + ci * PI + (2 * py) * (S + 2) + 2 * px;
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
        float best = acc[0]; int sel = 0;
        if (acc[1] > best) { best = acc[1]; sel = 1; }
        if (acc[2] > best) { best = acc[2]; sel = 2; }
        if (acc[3] > best) { best = acc[3]; sel = 3; }
        if (!(best > 0.f)) { best = 0.f; sel = 4; }
        const int o = co * SO * SO + py * SO + px;
        dec[o] = (uint8_t)sel;
        if (DROP) best *= ks[o];
        out[co * PO + (py + BORDER_OUT) * WO + px + BORDER_OUT] = best;
    }
}

// acc[i] += the gradient of flat item q = tid + 256 i of a 3x3 conv: q < CO*CI*9 a weight (OIHW), then the CO biases.
// in: zero-bordered planes [CI][S+2][S+2]; dp: the gradient of the pooled output [CO][S/2][S/2], 0 where dec == 4.
template <int CI, int CO, int S, int NACC>
__device__ __forceinline__ void wgrad3(const float* in, const float* dp, const uint8_t* dec, float (&acc)[NACC]) {
    constexpr int SO = S / 2, NW = CO * CI * 9, NITEM = NW + CO, PI = (S + 2) * (S + 2), NWIN = SO * SO;
    static_assert(NACC * 256 >= NITEM, "accumulators must cover the layer");
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
        const int q = threadIdx.x + 256 * i;
        if (q >= NITEM) continue;
        float s = 0.f;
        if (q < NW) {
            const int co = q / (CI * 9), r = q % (CI * 9), ci = r / 9, k = r % 9;
            const float* ip = in + ci * PI + (k / 3) * (S + 2) + k % 3;
            const float* dpp = dp + co * NWIN;
            const uint8_t* dc = dec + co * NWIN;
#pragma unroll 8
            for (int w = 0; w < NWIN; ++w) {
                const int d = dc[w], py = w / SO, px = w % SO;           // d == 4: dp is 0 there, (4 >> 1) & 1 == 0 stays in the window
                s = fmaf(dpp[w], ip[(2 * py + ((d >> 1) & 1)) * (S + 2) + 2 * px + (d & 1)], s);
            }
        } else {
            const float* dpp = dp + (q - NW) * NWIN;
#pragma unroll 8
            for (int w = 0; w < NWIN; ++w) s += dpp[w];
        }
        acc[i] += s;
    }
}

// out[ci][y][x] (dense, S x S) = the gradient of the pooled tensor the conv read: the sum over the windows that the
// 3x3 footprint of (y, x) meets (two per axis) of dp * W where the window selected an output inside the footprint;
// masked by the previous block's own pool decisions (dec_prev == 4: its ReLU was closed) and scaled by its Dropout.
template <int CI, int CO, int S, bool DROP>
__device__ __forceinline__ void dgrad3(const float* w, const float* dp, const uint8_t* dec, const uint8_t* dec_prev,
                                       const float* ks, float* out) {
    constexpr int SO = S / 2, NWIN = SO * SO;
    for (int e = threadIdx.x; e < CI * S * S; e += 256) {
        const int ci = e / (S * S), y = (e / S) % S, x = e % S;
        float s = 0.f;
        if (dec_prev[e] != 4) {
            const int wy0 = (y - 1) >> 1, wx0 = (x - 1) >> 1;
            for (int co = 0; co < CO; ++co) {
                const float* wp = w + (co * CI + ci) * 9;
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const int wy = wy0 + a, wx = wx0 + c;
                        if ((unsigned)wy >= (unsigned)SO || (unsigned)wx >= (unsigned)SO) continue;
                        const int wi = co * NWIN + wy * SO + wx, d = dec[wi];
                        const int kr = y + 1 - (2 * wy + (d >> 1)), kc = x + 1 - (2 * wx + (d & 1));
                        if (d < 4 && (unsigned)kr < 3u && (unsigned)kc < 3u) s = fmaf(dp[wi], wp[kr * 3 + kc], s);
                    }
            }
            if (DROP) s *= ks[e];
        }
        out[e] = s;
    }
}
}  // namespace critic_bwd
