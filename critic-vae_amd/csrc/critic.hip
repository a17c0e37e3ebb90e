// critic.hip — the frozen critic CNN that produces `preds` in the training loop, and the uint8
// frame pre-processing, as two small fused kernels.
//
// Replaces Critic.evaluate / Critic.forward (critic_net.py:5-69, eval mode: Dropout = identity):
//   Conv(3,8,3,p1) ReLU Pool2 -> Conv(8,8,3,p1) ReLU Pool2 -> Conv(8,8,3,p1) ReLU Pool2 ->
//   Conv(8,16,3,p1) ReLU Pool2 -> Conv(16,32,4) ReLU -> Flatten -> Linear(32,32) ReLU ->
//   Linear(32,1) Sigmoid                                  (3.4 MFLOP / image, 11 873 parameters)
// called once per step at vae.py:50, and adjust_values + HWC->CHW of preprocess_observation
// (vae_utility.py:324-343).  One workgroup per image, every activation lives in LDS; weights are
// read in the reference's own state_dict order / OIHW layout (critic_train.hip trains that same block).
#include "common.h"
#include "critic_fwd.h"
using namespace critic_layout;

// the forward itself (conv3_relu_pool, forward_from_lds) lives in critic_fwd.h: critic_score.hip runs the same device code
__global__ __launch_bounds__(256) void critic_fwd_kernel(const float* __restrict__ x, const float* __restrict__ cp,
                                                         float* __restrict__ pred) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* lx = smem;
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int q = tid; q < critic_fwd::BORDERED_FLOATS; q += 256) smem[q] = 0.f;      // zero borders
    __syncthreads();
    const float* xb = x + (size_t)b * 3 * 64 * 64;
    for (int q = tid; q < 3 * 64 * 16; q += 256) {
        const int c4 = q & 15, row = (q >> 4) & 63, c = q >> 10;
        const float4 v = *reinterpret_cast<const float4*>(xb + (c * 64 + row) * 64 + c4 * 4);
        float* d = lx + c * 66 * 66 + (row + 1) * 66 + c4 * 4 + 1;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    const float p = critic_fwd::forward_from_lds(smem, cp);
    if (tid == 0) pred[b] = p;
}

// x[b][c][y][x] = u8[b][y][x][c] / 255   (adjust_values + transpose(2,0,1), vae_utility.py:324-343)
__global__ __launch_bounds__(256) void preprocess_u8_kernel(const uint8_t* __restrict__ u8, float* __restrict__ x,
                                                            int64_t npix_total, int hw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;       // pixel index over B*H*W
    if (i >= npix_total) return;
    const int64_t b = i / hw, p = i % hw;
    const uint8_t* s = u8 + i * 3;
    float* d = x + b * 3 * hw + p;
    d[0] = (float)s[0] / 255.0f; d[hw] = (float)s[1] / 255.0f; d[2 * (int64_t)hw] = (float)s[2] / 255.0f;
}

int launch_critic_fwd(int width, int B, const float* x, const float* critic_params, float* pred, hipStream_t st) {
    if (width != 64) { cvae_set_error("critic: width %d unsupported (the reference critic is 64x64 only)", width); return -2; }
    constexpr int SMEM = critic_fwd::SMEM_BYTES;
    static DeviceOnce once;
    { int rc = cvae_grant_lds(once, reinterpret_cast<const void*>(critic_fwd_kernel), SMEM); if (rc) return rc; }
    hipLaunchKernelGGL(critic_fwd_kernel, dim3(B), dim3(256), SMEM, st, x, critic_params, pred);
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_preprocess_u8(int width, int B, const uint8_t* u8, float* x, hipStream_t st) {
    const int64_t n = (int64_t)B * width * width;
    hipLaunchKernelGGL(preprocess_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, u8, x, n, width * width);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// diff[b][y][x] = grey(|a - b|) with the reference's luma weights (get_diff_image, vae_utility.py:256-277)
__global__ __launch_bounds__(256) void diff_grey_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        float* __restrict__ diff, int64_t npix_total, int hw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix_total) return;
    const int64_t img = i / hw, p = i % hw, o = img * 3 * hw + p;
    const float r = fabsf(b[o] - a[o]), g = fabsf(b[o + hw] - a[o + hw]), bl = fabsf(b[o + 2 * (int64_t)hw] - a[o + 2 * (int64_t)hw]);
    diff[i] = r * 0.2989f + g * 0.5870f + bl * 0.1140f;
}

int launch_diff_grey(int width, int B, const float* a, const float* b, float* diff, hipStream_t st) {
    const int64_t n = (int64_t)B * width * width;
    hipLaunchKernelGGL(diff_grey_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, b, diff, n, width * width);
    CVAE_CHECK_LAUNCH();
    return 0;
}

int critic_param_count() { return CRITIC_PARAMS; }
