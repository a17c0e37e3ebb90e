// fc.hip — the three Linear layers around the latent, fused with reparametrize and the concat.
//
// Replaces (vae_nets.py):  :105-109 flatten + fc_mu + fc_var,  :48-51 reparametrize (eps given),
// :143 cat((z,pred),1) + decoder_input Linear(33, bottleneck),  :144 view(-1,256,s,s), and their
// autograd.  Tiny GEMMs (0.8 MFLOP/img) -> VALU kernels, LDS-broadcast operands, fixed-order
// two-stage reductions.  Native layouts: Wfc [K][64] (cols 0..31 = fc_mu, 32..63 = fc_var, K in
// (h,w,c) order), Wd [33][K] (K in (h,w,c) order) so that `flat`/`h` are the NHWC activations.
#include "common.h"

static constexpr int FC_KS = 32;         // K splits of the fc_mu|fc_var GEMM

// slab[ks][m][64] = sum_{k in K-slice ks} A[m][k] * Bm(k, n)   on v_mfma_f32_32x32x2_f32.
// A is [M][K] row-major.  B_KMAJOR == false: Bm(k,n) = Bp[k*64 + n] (fc_mu|fc_var weights, N = 64);
// B_KMAJOR == true : Bm(k,n) = Bp[n*K + k] for n < NV, 0 otherwise (decoder_input transposed, NV = 33).
// WG = 128 rows x 64 columns x one K-slice; wave w owns rows 32w..32w+31 and both 32-column tiles.
// Block (bx, by) = row block bx, K-slice by; lds: LATENT_GEMM_LDS floats.  Chunk i+1's A and B units are requested into registers
// before the MFMAs of chunk i; rows / columns outside the matrices read element row 0 and are zeroed at the LDS write, so that
// nothing waits on the load where it is issued.
static constexpr int LATENT_GEMM_LDS = 128 * 33 + 32 * 65;
template <bool B_KMAJOR, typename AT>       // AT = storage type of A (an activation / activation gradient)
__device__ __forceinline__ void latent_gemm_body(float* lds, const float* __restrict__ A, const float* __restrict__ Bp,
                                                 float* __restrict__ slab, int M, int K, int kslice, int NV, int bx, int by) {
    constexpr bool BF = Act<AT>::BF16;
    float* lds_a = lds;
    float* lds_b = lds + 128 * 33;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int m0 = bx * 128, k0 = by * kslice, kend = k0 + kslice;
    f32x16 acc[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[nb][v] = 0.f;
    f32x4 ra32[BF ? 1 : 4], rb[2];
    bf16x4 ra16[BF ? 4 : 1];
    auto fetch = [&](int kc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + i * 256, c4 = q & 7, r = q >> 3;
            const size_t at = (m0 + r < M ? (size_t)(m0 + r) * K : 0) + kc + c4 * 4;
            if constexpr (BF) ra16[i] = Act<AT>::ld4raw(A, at);
            else ra32[i] = Act<AT>::ld4(A, at);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = tid + i * 256;
            if constexpr (!B_KMAJOR) rb[i] = *reinterpret_cast<const f32x4*>(Bp + (size_t)(kc + (q >> 4)) * 64 + (q & 15) * 4);
            else rb[i] = *reinterpret_cast<const f32x4*>(Bp + ((q >> 3) < NV ? (size_t)(q >> 3) * K : 0) + kc + (q & 7) * 4);
        }
    };
    fetch(k0);
    for (int kc = k0; kc < kend; kc += 32) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + i * 256, c4 = q & 7, r = q >> 3;
            f32x4 v;
            if constexpr (BF) v = f32x4{(float)ra16[i][0], (float)ra16[i][1], (float)ra16[i][2], (float)ra16[i][3]};
            else v = ra32[i];
            if (!(m0 + r < M)) v = f32x4{0.f, 0.f, 0.f, 0.f};
            float* d = lds_a + r * 33 + c4 * 4;
            d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = tid + i * 256;
            if constexpr (!B_KMAJOR) {
                const int c4 = q & 15, kk = q >> 4;
                float* d = lds_b + kk * 65 + c4 * 4;
                d[0] = rb[i][0]; d[1] = rb[i][1]; d[2] = rb[i][2]; d[3] = rb[i][3];
            } else {
                const int c4 = q & 7, n = q >> 3;
                const f32x4 v = n < NV ? rb[i] : f32x4{0.f, 0.f, 0.f, 0.f};
                lds_b[(c4 * 4 + 0) * 65 + n] = v[0]; lds_b[(c4 * 4 + 1) * 65 + n] = v[1];
                lds_b[(c4 * 4 + 2) * 65 + n] = v[2]; lds_b[(c4 * 4 + 3) * 65 + n] = v[3];
            }
        }
        __syncthreads();
        if (kc + 32 < kend) fetch(kc + 32);
        __builtin_amdgcn_sched_barrier(0);                    // the next chunk's loads stay in front of the MFMAs they travel under
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float av = lds_a[(wave * 32 + li) * 33 + 2 * j + lh];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, lds_b[(2 * j + lh) * 65 + nb * 32 + li], acc[nb], 0, 0, 0);
        }
    }
    float* out = slab + (size_t)by * M * 64;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int m = m0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
            if (m < M) out[(size_t)m * 64 + nb * 32 + li] = acc[nb][v];
        }
}

template <bool B_KMAJOR, typename AT>       // grid (row blocks, K-slices)
__global__ __launch_bounds__(256) void latent_gemm_kernel(const float* __restrict__ A, const float* __restrict__ Bp,
                                                          float* __restrict__ slab, int M, int K, int kslice, int NV) {
    __shared__ __attribute__((aligned(16))) float lds[LATENT_GEMM_LDS];
    latent_gemm_body<B_KMAJOR, AT>(lds, A, Bp, slab, M, K, kslice, NV, blockIdx.x, blockIdx.y);
}

// dzcat[b][i] = sum_ks slab[ks][b][i], i < 33
__global__ __launch_bounds__(256) void decin_dz_finish_kernel(const float* __restrict__ slab, float* __restrict__ dzcat, int B, int KS) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * 33) return;
    const int b = idx / 33, i = idx % 33;
    float acc = 0.f;
    if (KS == FC_KS) {                      // the split count the launchers use: all loads in flight at once
#pragma unroll
        for (int ks = 0; ks < FC_KS; ++ks) acc += slab[((size_t)ks * B + b) * 64 + i];
    } else {
        for (int ks = 0; ks < KS; ++ks) acc += slab[((size_t)ks * B + b) * 64 + i];
    }
    dzcat[idx] = acc;
}

// mu, logvar = bias + sum of partials; z = mu + eps*exp(0.5*logvar); zcat = [z | pred]
__global__ __launch_bounds__(256) void fc_finish_kernel(const float* __restrict__ part, const float* __restrict__ bfc,
                                                        const float* __restrict__ eps, const float* __restrict__ pred,
                                                        float* __restrict__ mu, float* __restrict__ logvar,
                                                        float* __restrict__ zcat, int B) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * 32) return;
    const int b = idx >> 5, d = idx & 31;
    float m = bfc[d], lv = bfc[32 + d];
    for (int ks = 0; ks < FC_KS; ++ks) {
        m += part[((size_t)ks * B + b) * 64 + d];
        lv += part[((size_t)ks * B + b) * 64 + 32 + d];
    }
    mu[idx] = m;
    logvar[idx] = lv;
    zcat[b * 33 + d] = m + eps[idx] * expf(0.5f * lv);
    if (d == 0) zcat[b * 33 + 32] = pred[b];
}

// h[b][j] = bd[j] + sum_i zcat[b][i] * Wd[i][j].  Workgroup = 1024 columns x DI_IMGS images: every 16-byte load of Wd
// serves DI_IMGS images (one image per workgroup re-read the 33 x K weights B times from L2: 1.1 GB at B = 2048,
// 44 us; now 69 MB).  Per output the sum still runs i = 0..32 from the bias.  DI_IMGS = 16 at large batches, 8 or 4 where 16 would
// leave most of the chip without a workgroup (latent_plan); an image's sums do not depend on it.
template <typename AT, int DI_IMGS>
__global__ __launch_bounds__(256) void decin_fwd_kernel(const float* __restrict__ zcat, const float* __restrict__ wd,
                                                        const float* __restrict__ bd, float* __restrict__ h, int K, int B) {
    __shared__ float z[DI_IMGS][33];
    const int b0 = blockIdx.y * DI_IMGS, j = (blockIdx.x * 256 + threadIdx.x) * 4;
    for (int q = threadIdx.x; q < DI_IMGS * 33; q += 256) z[q / 33][q % 33] = b0 + q / 33 < B ? zcat[(size_t)b0 * 33 + q] : 0.f;
    __syncthreads();
    const f32x4 bias = *reinterpret_cast<const f32x4*>(bd + j);
    f32x4 acc[DI_IMGS];
#pragma unroll
    for (int m = 0; m < DI_IMGS; ++m) acc[m] = bias;
#pragma unroll 3
    for (int i = 0; i < 33; ++i) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(wd + (size_t)i * K + j);
#pragma unroll
        for (int m = 0; m < DI_IMGS; ++m) {
            const float zv = z[m][i];                         // wave-uniform LDS broadcast
            acc[m][0] = fmaf(zv, w[0], acc[m][0]); acc[m][1] = fmaf(zv, w[1], acc[m][1]);
            acc[m][2] = fmaf(zv, w[2], acc[m][2]); acc[m][3] = fmaf(zv, w[3], acc[m][3]);
        }
    }
#pragma unroll
    for (int m = 0; m < DI_IMGS; ++m)
        if (b0 + m < B) Act<AT>::st4(h, (size_t)(b0 + m) * K + j, acc[m]);
}

// dml[b][0..31] = dz + dmu_loss ; dml[b][32..63] = dz*eps*0.5*exp(0.5*logvar) + dlv_loss
__global__ __launch_bounds__(256) void fc_bwd_prep_kernel(const float* __restrict__ dzcat, const float* __restrict__ eps,
                                                          const float* __restrict__ logvar, const float* __restrict__ dmu_loss,
                                                          const float* __restrict__ dlv_loss, float* __restrict__ dml, int B) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * 32) return;
    const int b = idx >> 5, d = idx & 31;
    const float dz = dzcat[b * 33 + d];
    dml[b * 64 + d] = dz + dmu_loss[idx];
    dml[b * 64 + 32 + d] = dz * eps[idx] * 0.5f * expf(0.5f * logvar[idx]) + dlv_loss[idx];
}

// dflat[b][k] = sum_n dml[b][n] * Wfc[k][n].  Thread = one k (its 64 weights in registers), workgroup = 256 k x DF_IMGS
// images (8 images per workgroup re-read the 1 MB of Wfc 256 times at B = 2048 and ran at 42 us); n = 0..63 in order.
// DF_IMGS = 32 at large batches, 16 or 8 where 32 would leave most of the chip without a workgroup (latent_plan); an image's sums
// do not depend on it.  Block (bx, by) = image group bx, 256-row block by of Wfc; lds: DF_IMGS * 64 floats.
template <typename AT, int DF_IMGS>
__device__ __forceinline__ void fc_bwd_dflat_body(float* lds, const float* __restrict__ dml, const float* __restrict__ wfc,
                                                  float* __restrict__ dflat, int B, int K, int bx, int by) {
    float (*g)[64] = reinterpret_cast<float (*)[64]>(lds);
    const int b0 = bx * DF_IMGS, k = by * 256 + threadIdx.x;
    for (int q = threadIdx.x; q < DF_IMGS * 16; q += 256) {
        const int r = q >> 4, c4 = q & 15;
        *reinterpret_cast<f32x4*>(&g[r][c4 * 4]) = b0 + r < B ? *reinterpret_cast<const f32x4*>(dml + (size_t)(b0 + r) * 64 + c4 * 4)
                                                              : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    float w[64];
#pragma unroll
    for (int n4 = 0; n4 < 16; ++n4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(wfc + (size_t)k * 64 + n4 * 4);
        w[n4 * 4] = v[0]; w[n4 * 4 + 1] = v[1]; w[n4 * 4 + 2] = v[2]; w[n4 * 4 + 3] = v[3];
    }
#pragma unroll 4
    for (int i = 0; i < DF_IMGS; ++i) {
        if (b0 + i >= B) break;
        float acc = 0.f;
#pragma unroll
        for (int n4 = 0; n4 < 16; ++n4) {
            const f32x4 gv = *reinterpret_cast<const f32x4*>(&g[i][n4 * 4]);      // wave-uniform 16-byte LDS broadcast
            acc = fmaf(gv[0], w[n4 * 4], acc); acc = fmaf(gv[1], w[n4 * 4 + 1], acc);
            acc = fmaf(gv[2], w[n4 * 4 + 2], acc); acc = fmaf(gv[3], w[n4 * 4 + 3], acc);
        }
        Act<AT>::st(dflat, (size_t)(b0 + i) * K + k, acc);
    }
}

// precision mode 1: the two batch-contracted weight gradients  C[m][n] = sum_b A[b][m] * Bm[b][n]  on the bf16 MFMA
// (fc_mu|fc_var: A = flat (bf16 activations), Bm = dml;  decoder_input: A = [zcat | 1] (the ones column yields the
// bias gradient), Bm = dh (bf16)).  Both inputs are row-major in b, i.e. the contraction index is the ROW: tiles of BG_BT
// images are copied to LDS as they are (fp32 inputs rounded to bf16 on the way) and both MFMA operands are transposed
// LDS reads (ds_read_b64_tr_b16).  Workgroup = (32*MBLK) x (32*NBLK) outputs over the whole batch (no split-K slabs);
// wave w contracts images [w*BG_BT/4, (w+1)*BG_BT/4) of every tile, the four partial tiles are summed through LDS.
struct BGemmArgs {
    const float* A; const float* Bm;      // opaque: bf16 or fp32 per template flags
    int lda, ldb;                         // row strides in elements
    int a_cols;                           // valid columns of A (fp32 A only); column a_cols reads as 1.0, beyond as 0
    float* out; int ldo;                  // C rows [0, out_rows) -> out[m*ldo + n0 + n]
    int out_rows;
    float* out_last;                      // row `out_rows` (the ones column) -> out_last[n0 + n], may be null
    int B;
};

// BT images per LDS tile: each tile costs two workgroup barriers, and at 64 images a wave had two MFMAs between them (41 / 35 us
// at B = 2048 for 1 GFLOP); 256 images per tile = 4 k-steps per wave and tile
static constexpr int BG_BT = 256;
static constexpr int bgemm_tr_lds(int MBLK, int NBLK) { return BG_BT * 32 * (MBLK + NBLK) / 2 + 3 * 1024; }     // floats
template <int MBLK, int NBLK, bool A_F32, bool B_F32>       // block bx of K / 32; lds: bgemm_tr_lds(MBLK, NBLK) floats, 16-byte aligned
__device__ __forceinline__ void bgemm_tr_body(float* lds, const BGemmArgs& a, int bx) {
    constexpr int MC = 32 * MBLK, NC = 32 * NBLK, BT = BG_BT;
    __bf16* lds_a = reinterpret_cast<__bf16*>(lds);
    __bf16* lds_b = lds_a + BT * MC;
    float* red = reinterpret_cast<float*>(lds_b + BT * NC);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int g = lane >> 4, h = g >> 1, qrow = (lane & 15) >> 2, cb = 16 * (g & 1) + 4 * (lane & 3);
    const int m0 = A_F32 ? 0 : bx * MC, n0 = (A_F32 ? bx : 0) * NC;   // fp32-A form tiles N, bf16-A form tiles M
    f32x16 acc[MBLK][NBLK];
#pragma unroll
    for (int i = 0; i < MBLK; ++i)
#pragma unroll
        for (int j = 0; j < NBLK; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;
    // fp32 A (decoder_input: [zcat | 1], 34 real columns of MC = 64): only the real columns travel — item q = (row q / AC, column
    // q % AC); the LDS columns past them are zeroed once and never written again (half the loads and stores of a dense tile)
    constexpr int AC = 34;
    constexpr int AU = A_F32 ? (BT * AC) / 256 : (BT * MC / 8 + 255) / 256;        // per-thread staging items
    constexpr int BU = B_F32 ? (BT * NC / 4) / 256 : (BT * NC / 8 + 255) / 256;
    float ra32[A_F32 ? AU : 1];
    bf16x8 ra16[A_F32 ? 1 : AU];
    f32x4 rb32[B_F32 ? BU : 1];
    bf16x8 rb16[B_F32 ? 1 : BU];
    bf16x8 zero8;
#pragma unroll
    for (int c = 0; c < 8; ++c) zero8[c] = (__bf16)0.f;
    auto fetch = [&](int b0) {
        if constexpr (A_F32) {
#pragma unroll
            for (int i = 0; i < AU; ++i) {
                const int q = tid + i * 256, r = q / AC, c = q % AC, b = b0 + r;
                const bool ok = b < a.B && c < a.a_cols;
                const float l = a.A[ok ? (size_t)b * a.lda + c : 0];
                ra32[i] = ok ? l : ((b < a.B && c == a.a_cols) ? 1.0f : 0.f);
            }
        } else {
#pragma unroll
            for (int i = 0; i < AU; ++i) {
                const int q = tid + i * 256, r = q / (MC / 8), c8 = q % (MC / 8), b = b0 + r;
                const bool ok = (BT * MC / 8) % 256 == 0 || q < BT * MC / 8;
                const bool inb = ok && b < a.B;
                const bf16x8 l = Act<__bf16>::ld8(a.A, inb ? (size_t)b * a.lda + m0 + c8 * 8 : 0);
                ra16[i] = inb ? l : zero8;
            }
        }
        if constexpr (B_F32) {
#pragma unroll
            for (int i = 0; i < BU; ++i) {
                const int q = tid + i * 256, r = q / (NC / 4), c4 = q % (NC / 4), b = b0 + r;
                const bool ok = b < a.B;
                const f32x4 l = *reinterpret_cast<const f32x4*>(a.Bm + (ok ? (size_t)b * a.ldb + n0 + c4 * 4 : 0));
                rb32[i] = ok ? l : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        } else {
#pragma unroll
            for (int i = 0; i < BU; ++i) {
                const int q = tid + i * 256, r = q / (NC / 8), c8 = q % (NC / 8), b = b0 + r;
                const bool ok = ((BT * NC / 8) % 256 == 0 || q < BT * NC / 8) && b < a.B;
                const bf16x8 l = Act<__bf16>::ld8(a.Bm, ok ? (size_t)b * a.ldb + n0 + c8 * 8 : 0);
                rb16[i] = ok ? l : zero8;
            }
        }
    };
    if constexpr (A_F32) {
        static_assert((BT * AC) % 256 == 0 && AC <= MC, "whole staging rounds of the real columns");
        for (int q = tid; q < BT * MC; q += 256) lds_a[q] = (__bf16)0.f;      // columns >= AC stay zero
    }
    fetch(0);
    for (int b0 = 0; b0 < a.B; b0 += BT) {
        __syncthreads();
        if constexpr (A_F32) {
#pragma unroll
            for (int i = 0; i < AU; ++i) { const int q = tid + i * 256; lds_a[(q / AC) * MC + q % AC] = (__bf16)ra32[i]; }
        } else {
#pragma unroll
            for (int i = 0; i < AU; ++i) {
                const int q = tid + i * 256;
                if ((BT * MC / 8) % 256 == 0 || q < BT * MC / 8) *reinterpret_cast<bf16x8*>(lds_a + (size_t)q * 8) = ra16[i];
            }
        }
        if constexpr (B_F32) {
#pragma unroll
            for (int i = 0; i < BU; ++i) {
                bf16x4 u;
                u[0] = (__bf16)rb32[i][0]; u[1] = (__bf16)rb32[i][1]; u[2] = (__bf16)rb32[i][2]; u[3] = (__bf16)rb32[i][3];
                *reinterpret_cast<bf16x4*>(lds_b + (size_t)(tid + i * 256) * 4) = u;
            }
        } else {
#pragma unroll
            for (int i = 0; i < BU; ++i) {
                const int q = tid + i * 256;
                if ((BT * NC / 8) % 256 == 0 || q < BT * NC / 8) *reinterpret_cast<bf16x8*>(lds_b + (size_t)q * 8) = rb16[i];
            }
        }
        __syncthreads();
        if (b0 + BT < a.B) fetch(b0 + BT);
#pragma unroll
        for (int ks = 0; ks < BT / 64; ++ks) {
            const int row = (BT / 4) * wave + 16 * ks + 8 * h + qrow;      // this wave's BT/4 images of the tile, 16 per k-step
            bf16x8 bv[NBLK];
#pragma unroll
            for (int j = 0; j < NBLK; ++j) bv[j] = tr_frag(lds_b + row * NC + j * 32 + cb, lds_b + (row + 4) * NC + j * 32 + cb);
#pragma unroll
            for (int i = 0; i < MBLK; ++i) {
                const bf16x8 av = tr_frag(lds_a + row * MC + i * 32 + cb, lds_a + (row + 4) * MC + i * 32 + cb);
#pragma unroll
                for (int j = 0; j < NBLK; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv[j], acc[i][j], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MBLK; ++i)
#pragma unroll
        for (int j = 0; j < NBLK; ++j) {
            __syncthreads();
            if (wave > 0) {
#pragma unroll
                for (int v = 0; v < 16; ++v) red[((wave - 1) * 16 + v) * 64 + lane] = acc[i][j][v];
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float x = ((acc[i][j][v] + red[v * 64 + lane]) + red[(16 + v) * 64 + lane]) + red[(32 + v) * 64 + lane];
                    const int m = m0 + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh, n = n0 + j * 32 + li;
                    if (m < a.out_rows) a.out[(size_t)m * a.ldo + n] = x;
                    else if (m == a.out_rows && a.out_last) a.out_last[n] = x;
                }
            }
        }
}

// fp32 mode: the same batch-contracted weight gradients on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: one A and one B
// value per lane and k-step, read as conflict-free LDS rows — no transposition needed).  Replaces the serial VALU loops
// over the batch and the batch-split slabs + two slab reductions they replaced.
// A_PAD: A is [b][a_cols] fp32 with an implicit ones column at a_cols (decoder_input); else A is [b][lda] and the
// workgroup takes columns m0..m0+MC.
static constexpr int bgemm_f32_lds(int MBLK, int NBLK) { return 64 * 32 * (MBLK + NBLK) + 3 * 1024; }           // floats
template <int MBLK, int NBLK, bool A_PAD>                   // block bx of K / 32; lds: bgemm_f32_lds(MBLK, NBLK) floats, 16-byte aligned
__device__ __forceinline__ void bgemm_f32_body(float* lds, const BGemmArgs& a, int bx) {
    constexpr int MC = 32 * MBLK, NC = 32 * NBLK;
    float* lds_a = lds;
    float* lds_b = lds + 64 * MC;
    float* red = lds_b + 64 * NC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int m0 = A_PAD ? 0 : bx * MC, n0 = (A_PAD ? bx : 0) * NC;
    f32x16 acc[MBLK][NBLK];
#pragma unroll
    for (int i = 0; i < MBLK; ++i)
#pragma unroll
        for (int j = 0; j < NBLK; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;
    constexpr int AU = A_PAD ? (64 * MC) / 256 : (64 * MC / 4) / 256, BU = (64 * NC / 4) / 256;
    float ra1[A_PAD ? AU : 1];
    f32x4 ra4[A_PAD ? 1 : AU], rb4[BU];
    auto fetch = [&](int b0) {
        if constexpr (A_PAD) {
#pragma unroll
            for (int i = 0; i < AU; ++i) {
                const int q = tid + i * 256, r = q / MC, c = q % MC, b = b0 + r;
                const bool ok = b < a.B && c < a.a_cols;
                const float l = a.A[ok ? (size_t)b * a.lda + c : 0];
                ra1[i] = ok ? l : ((b < a.B && c == a.a_cols) ? 1.0f : 0.f);
            }
        } else {
#pragma unroll
            for (int i = 0; i < AU; ++i) {
                const int q = tid + i * 256, r = q / (MC / 4), c4 = q % (MC / 4), b = b0 + r;
                const bool ok = b < a.B;
                const f32x4 l = *reinterpret_cast<const f32x4*>(a.A + (ok ? (size_t)b * a.lda + m0 + c4 * 4 : 0));
                ra4[i] = ok ? l : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int i = 0; i < BU; ++i) {
            const int q = tid + i * 256, r = q / (NC / 4), c4 = q % (NC / 4), b = b0 + r;
            const bool ok = b < a.B;
            const f32x4 l = *reinterpret_cast<const f32x4*>(a.Bm + (ok ? (size_t)b * a.ldb + n0 + c4 * 4 : 0));
            rb4[i] = ok ? l : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    fetch(0);
    for (int b0 = 0; b0 < a.B; b0 += 64) {
        __syncthreads();
        if constexpr (A_PAD) {
#pragma unroll
            for (int i = 0; i < AU; ++i) lds_a[tid + i * 256] = ra1[i];
        } else {
#pragma unroll
            for (int i = 0; i < AU; ++i) *reinterpret_cast<f32x4*>(lds_a + (size_t)(tid + i * 256) * 4) = ra4[i];
        }
#pragma unroll
        for (int i = 0; i < BU; ++i) *reinterpret_cast<f32x4*>(lds_b + (size_t)(tid + i * 256) * 4) = rb4[i];
        __syncthreads();
        if (b0 + 64 < a.B) fetch(b0 + 64);
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {                       // this wave's 16 images of the tile, two per MFMA
            const int row = 16 * wave + 2 * kk + lh;
            float bv[NBLK];
#pragma unroll
            for (int j = 0; j < NBLK; ++j) bv[j] = lds_b[row * NC + j * 32 + li];
#pragma unroll
            for (int i = 0; i < MBLK; ++i) {
                const float av = lds_a[row * MC + i * 32 + li];
#pragma unroll
                for (int j = 0; j < NBLK; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[j], acc[i][j], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MBLK; ++i)
#pragma unroll
        for (int j = 0; j < NBLK; ++j) {
            __syncthreads();
            if (wave > 0) {
#pragma unroll
                for (int v = 0; v < 16; ++v) red[((wave - 1) * 16 + v) * 64 + lane] = acc[i][j][v];
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float x = ((acc[i][j][v] + red[v * 64 + lane]) + red[(16 + v) * 64 + lane]) + red[(32 + v) * 64 + lane];
                    const int m = m0 + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh, n = n0 + j * 32 + li;
                    if (m < a.out_rows) a.out[(size_t)m * a.ldo + n] = x;
                    else if (m == a.out_rows && a.out_last) a.out_last[n] = x;
                }
            }
        }
}

// Work that does not depend on each other shares a launch: each job is a range of blockIdx.x (LatentPlan's order: the batch-contracted
// GEMM first, whose workgroups each walk the whole batch and so live longest at every batch; the other jobs' grids grow with the batch
// instead) and the jobs' LDS areas are carved from one buffer of the largest job's size.  Every body computes what its
// own kernel computed, in the same order.
static constexpr int imax(int a, int b) { return a > b ? a : b; }

// launch_decin_bwd: dWd | dbd = [zcat | 1]^T . dh and the d_zcat slabs (latent_gemm, B_KMAJOR) both read only dh, zcat and Wd
struct DecinBwdJobs {
    const float* dh; const float* wd; float* slab; int B, K;
    BGemmArgs g; int bgemm_blocks;        // blocks [0, K / 32)
    int row_blocks;                       // then latent_gemm: block l = (row block l % row_blocks, K-slice l / row_blocks)
};
template <typename AT>
__global__ __launch_bounds__(256) void decin_bwd_kernel(DecinBwdJobs j) {
    constexpr bool BF = Act<AT>::BF16;
    __shared__ __attribute__((aligned(16))) float lds[imax(LATENT_GEMM_LDS, BF ? bgemm_tr_lds(2, 1) : bgemm_f32_lds(2, 1))];
    const int blk = blockIdx.x, l = blk - j.bgemm_blocks;
    if (blk < j.bgemm_blocks) {
        if constexpr (BF) bgemm_tr_body<2, 1, true, false>(lds, j.g, blk);
        else bgemm_f32_body<2, 1, true>(lds, j.g, blk);
    } else latent_gemm_body<true, AT>(lds, j.dh, j.wd, j.slab, j.B, j.K, j.K / FC_KS, 33, l % j.row_blocks, l / j.row_blocks);
}

// launch_fc_bwd after fc_bwd_prep: dWfc = flat^T . dml, dflat and stage 1 of dbfc = colsum(dml) all read only dml (and flat, Wfc)
struct FcBwdJobs {
    const float* dml; const float* wfc; float* dflat; int B, K;
    BGemmArgs g; int bgemm_blocks;        // blocks [0, K / 32)
    int dflat_blocks, img_blocks;         // then dflat: block l = (image group l % img_blocks, row block l / img_blocks)
    float* cs_part; int cs_blocks;        // then the column sum's stage 1
};
template <typename AT, int DF_IMGS>
__global__ __launch_bounds__(256) void fc_bwd_kernel(FcBwdJobs j) {
    constexpr bool BF = Act<AT>::BF16;
    __shared__ __attribute__((aligned(16))) float lds[imax(DF_IMGS * 64, BF ? bgemm_tr_lds(1, 2) : bgemm_f32_lds(1, 2))];
    const int blk = blockIdx.x, l = blk - j.bgemm_blocks;
    if (blk < j.bgemm_blocks) {
        if constexpr (BF) bgemm_tr_body<1, 2, false, true>(lds, j.g, blk);
        else bgemm_f32_body<1, 2, false>(lds, j.g, blk);
    } else if (l < j.dflat_blocks) fc_bwd_dflat_body<AT, DF_IMGS>(lds, j.dml, j.wfc, j.dflat, j.B, j.K, l % j.img_blocks, l / j.img_blocks);
    else colsum_stage1_block(j.dml, j.B, 64, j.cs_part, l - j.dflat_blocks, j.cs_blocks, lds);
}

// dflat alone (grid: LatentPlan::fb_dflat blocks), for the shapes where the GEMM's workgroups fill the chip by themselves: with its own
// 2 - 8 KB of LDS and 76 registers six workgroups fit a compute unit, beside the GEMM's buffer only two to four
template <typename AT, int DF_IMGS>
__global__ __launch_bounds__(256) void fc_bwd_dflat_kernel(const float* __restrict__ dml, const float* __restrict__ wfc,
                                                           float* __restrict__ dflat, int B, int K, int img_blocks) {
    __shared__ __attribute__((aligned(16))) float lds[DF_IMGS * 64];
    fc_bwd_dflat_body<AT, DF_IMGS>(lds, dml, wfc, dflat, B, K, blockIdx.x % img_blocks, blockIdx.x / img_blocks);
}

static inline int bott(int width) { return 256 * (width / 16) * (width / 16); }
static inline int decin_splits(int B) { int s = cdiv(B, 16); return s > 16 ? 16 : s; }

// Images per workgroup of decin_fwd / fc_bwd_dflat: the large-batch value (fewest re-reads of the weights), halved while the
// halved form's grid still fits two workgroups per compute unit, down to `lo`.
static inline int imgs_per_wg(int B, int col_blocks, int hi, int lo, int num_cus) {
    int imgs = hi;
    while (imgs > lo && (int64_t)col_blocks * cdiv(B, imgs / 2) <= 2 * (int64_t)num_cus) imgs /= 2;
    return imgs;
}

LatentPlan latent_plan(int width, int B, int num_cus) {
    const int K = bott(width);
    LatentPlan p;
    p.fc_fwd_gemm = cdiv(B, 128) * FC_KS;
    p.di_imgs = imgs_per_wg(B, K / 1024, 16, 4, num_cus);
    p.di_blocks = (K / 1024) * cdiv(B, p.di_imgs);
    p.db_gemm = cdiv(B, 128) * FC_KS;
    p.db_bgemm = K / 32;
    p.df_imgs = imgs_per_wg(B, K / 256, 32, 8, num_cus);
    p.fb_dflat = (K / 256) * cdiv(B, p.df_imgs);
    p.fb_bgemm = K / 32;
    p.fb_colsum = B < CS_BLOCKS ? B : CS_BLOCKS;
    // The merged launch holds two (bf16 storage) to four workgroups per compute unit.  Where the GEMM's K / 32 workgroups take more than
    // half of the two-per-unit slots (128 x 128 frames on 256 units: 512 of 512), dflat would only queue behind them at a third of its
    // own occupancy (measured: 82.9 us against 50.4 + 22.0 + 5.0 us apart): it then keeps a launch of its own.
    p.fb_split = K / 32 > num_cus ? 1 : 0;
    return p;
}

int64_t fc_ws_floats(int width, int B) {
    const int K = bott(width);
    const int64_t a = (int64_t)FC_KS * B * 64;                 // fc forward partials
    const int64_t b = (int64_t)decin_splits(B) * 34 * K;       // decoder_input dW slabs
    const int64_t c = (int64_t)B * 64 + colsum_ws_floats(B, 64);   // dml + its column sums
    return (a > b ? a : b) + c;
}

int launch_fc_fwd(int width, int B, const float* flat, const float* wfc, const float* bfc, const float* eps,
                  const float* pred, float* mu, float* logvar, float* zcat, float* ws, hipStream_t st, bool bf16io) {
    const int K = bott(width);
    if (bf16io) hipLaunchKernelGGL((latent_gemm_kernel<false, __bf16>), dim3(cdiv(B, 128), FC_KS), dim3(256), 0, st, flat, wfc, ws, B, K, K / FC_KS, 64);
    else hipLaunchKernelGGL((latent_gemm_kernel<false, float>), dim3(cdiv(B, 128), FC_KS), dim3(256), 0, st, flat, wfc, ws, B, K, K / FC_KS, 64);
    CVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(fc_finish_kernel, dim3(cdiv(B * 32, 256)), dim3(256), 0, st, ws, bfc, eps, pred, mu, logvar, zcat, B);
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_decin_fwd(int width, int B, const float* zcat, const float* wd, const float* bd, float* h, hipStream_t st, bool bf16io) {
    const int K = bott(width);
    const LatentPlan p = latent_plan(width, B, cvae_num_cus());
    const dim3 grid(K / 1024, cdiv(B, p.di_imgs));
#define DECIN_FWD(AT, IMGS) hipLaunchKernelGGL((decin_fwd_kernel<AT, IMGS>), grid, dim3(256), 0, st, zcat, wd, bd, h, K, B)
    switch (p.di_imgs + (bf16io ? 1 : 0)) {
        case 16: DECIN_FWD(float, 16); break;
        case 17: DECIN_FWD(__bf16, 16); break;
        case 8: DECIN_FWD(float, 8); break;
        case 9: DECIN_FWD(__bf16, 8); break;
        case 4: DECIN_FWD(float, 4); break;
        case 5: DECIN_FWD(__bf16, 4); break;
        default: cvae_set_error("decin_fwd: no kernel for %d images per workgroup", p.di_imgs); return -2;
    }
#undef DECIN_FWD
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_decin_bwd(int width, int B, const float* zcat, const float* dh, const float* wd, float* dwd, float* dbd,
                     float* dzcat, float* ws, hipStream_t st, bool bf16io) {
    const int K = bott(width);
    const LatentPlan p = latent_plan(width, B, cvae_num_cus());
    // one launch: [zcat | 1]^T . dh on the MFMA of the storage type, whole batch per workgroup (dWd and dbd written directly), and the d_zcat slabs
    DecinBwdJobs j{dh, wd, ws, B, K, BGemmArgs{zcat, dh, 33, K, 33, dwd, K, 33, dbd, B}, p.db_bgemm, cdiv(B, 128)};
    if (bf16io) hipLaunchKernelGGL(decin_bwd_kernel<__bf16>, dim3(p.db_bgemm + p.db_gemm), dim3(256), 0, st, j);
    else hipLaunchKernelGGL(decin_bwd_kernel<float>, dim3(p.db_gemm + p.db_bgemm), dim3(256), 0, st, j);
    CVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(decin_dz_finish_kernel, dim3(cdiv(B * 33, 256)), dim3(256), 0, st, ws, dzcat, B, FC_KS);
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_fc_bwd(int width, int B, const float* flat, const float* wfc, const float* dzcat, const float* eps,
                  const float* logvar, const float* dmu_loss, const float* dlv_loss, float* dwfc, float* dbfc,
                  float* dflat, float* ws, hipStream_t st, bool bf16io) {
    const int K = bott(width);
    const LatentPlan p = latent_plan(width, B, cvae_num_cus());
    const int64_t a = (int64_t)FC_KS * B * 64, b = (int64_t)decin_splits(B) * 34 * K;
    float* dml = ws + (a > b ? a : b);
    float* csws = dml + (size_t)B * 64;
    hipLaunchKernelGGL(fc_bwd_prep_kernel, dim3(cdiv(B * 32, 256)), dim3(256), 0, st, dzcat, eps, logvar, dmu_loss, dlv_loss, dml, B);
    CVAE_CHECK_LAUNCH();
    // one launch: flat^T . dml on the MFMA of the storage type, dflat, and the first stage of the column sum of dml
    FcBwdJobs j{dml, wfc, dflat, B, K, BGemmArgs{flat, dml, K, 64, 0, dwfc, 64, K, nullptr, B}, p.fb_bgemm,
                p.fb_dflat, cdiv(B, p.df_imgs), csws, p.fb_colsum};
    if (p.fb_split) j.dflat_blocks = 0;                       // first launch: dWfc and the column sum; dflat follows alone
    const dim3 grid(p.fb_bgemm + j.dflat_blocks + p.fb_colsum), dgrid(p.fb_dflat);
#define FC_BWD(AT, IMGS)                                                                                                          \
    do {                                                                                                                          \
        hipLaunchKernelGGL((fc_bwd_kernel<AT, IMGS>), grid, dim3(256), 0, st, j);                                                 \
        if (p.fb_split) hipLaunchKernelGGL((fc_bwd_dflat_kernel<AT, IMGS>), dgrid, dim3(256), 0, st, dml, wfc, dflat, B, K, j.img_blocks); \
    } while (0)
    switch (p.df_imgs + (bf16io ? 1 : 0)) {
        case 32: FC_BWD(float, 32); break;
        case 33: FC_BWD(__bf16, 32); break;
        case 16: FC_BWD(float, 16); break;
        case 17: FC_BWD(__bf16, 16); break;
        case 8: FC_BWD(float, 8); break;
        case 9: FC_BWD(__bf16, 8); break;
        default: cvae_set_error("fc_bwd: no kernel for %d images per workgroup", p.df_imgs); return -2;
    }
#undef FC_BWD
    CVAE_CHECK_LAUNCH();
    return launch_col_reduce(csws, p.fb_colsum, 64, 64, dbfc, csws + (size_t)CS_BLOCKS * 64, st);      // second stage, as launch_colsum runs it
}
