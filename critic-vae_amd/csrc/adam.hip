// adam.hip — fused flat-buffer Adam: torch.optim.Adam(lr) defaults (vae.py:36,58) over the whole
// parameter buffer in one HBM-bound pass (4 reads + 3 writes per element), gradient scale fused
// (1/world_size after the summing all-reduce).  Mirrors torch's single-tensor formulas:
//   m.lerp_(g, 1-b1);  v = b2*v + (1-b2)*g*g;  p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
#include "common.h"
#include "../../include/cvae.h"
#include <math.h>

// The options of cvae_adam_step_opt / cvae_adam_step_guarded_opt as the kernels take them: by value in the launch, as PadGaps is.
struct OptRanges {
    int32_t n;
    int64_t begin[CVAE_OPT_MAX_RANGES], end[CVAE_OPT_MAX_RANGES];
};
struct OptArgs {
    float decay_mul, ema_omd;
    float* ema;                 // n floats, or nullptr
    const float* aux;           // n_aux floats, read only
    float* aux_ema;
    int32_t n_aux;
    OptRanges r;
};

// one grid-stride pass of the update, shared by the plain and the guarded kernel and by their _opt forms: the same expressions,
// the same bits.  OPT: decoupled weight decay on the elements of o.r first (one fp32 product, rounded on its own: __fmul_rn keeps
// it out of the fused multiply-add of the update); EMA: o.ema follows the p just written.
template <bool OPT, bool EMA>
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, int64_t n4, float omb1, float b2, float omb2, float step_size,
                                            float sqrt_bc2, float eps, float gscale, const OptArgs* o) {
    // OPT: lane l keeps range l % 16 of the table (an unused slot is the empty [0, 0)), so one trip tests the wave's 256-element
    // span [e0, e0 + 256) against all 16 ranges with four vector compares and two ballots.  Wholly inside one range, or outside
    // all of them: done.  Where a boundary crosses the span, the ranges that touch it (one or two) are broadcast out of their
    // lanes and every lane tests its four elements against them.  No memory access and no scalar loop per trip: the first form
    // of this lookup walked the table with scalar loads per element in the boundary waves, and those 22 waves alone
    // outlasted the rest of the pass (LABNOTES).  Every lane of a wave that still has a float4 takes the trip, so the ballots see all 16
    // slots in a ragged last wave too.
    const int64_t lane = threadIdx.x & 63;
    int64_t rb = 0, re = 0;
    bool ranged = false;
    if constexpr (OPT) {
        ranged = o->r.n > 0;
        const int k = threadIdx.x & (CVAE_OPT_MAX_RANGES - 1);
        if (k < o->r.n) { rb = o->r.begin[k]; re = o->r.end[k]; }
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; (OPT ? i - lane : i) < n4; i += (int64_t)gridDim.x * 256) {
        // the four loads go out first: the table's own loads (first trip) then return under them, not in front of them
        const bool live = !OPT || i < n4;
        float4 pv = make_float4(0.f, 0.f, 0.f, 0.f), gv = pv, mv = pv, vv = pv;
        if (live) {
            pv = reinterpret_cast<float4*>(p)[i];
            gv = reinterpret_cast<const float4*>(g)[i];
            mv = reinterpret_cast<float4*>(m)[i];
            vv = reinterpret_cast<float4*>(v)[i];
        }
        unsigned decay = 0u;                // bit e: element 4 i + e lies in a decayed range
        if constexpr (OPT) {
            if (ranged) {
                const int64_t e0 = 4 * (i - lane);
                const bool full = rb <= e0 && re >= e0 + 256, touched = rb < e0 + 256 && re > e0;
                if (__any((int)full)) {
                    decay = 0xfu;
                } else {
                    uint64_t tm = __ballot((int)touched) & 0xffffull;          // the table's slots, once each
                    while (tm) {
                        const int k = __builtin_ctzll(tm);
                        tm &= tm - 1;
                        const int64_t b = ((int64_t)__builtin_amdgcn_readlane((int)(rb >> 32), k) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)rb, k);
                        const int64_t e = ((int64_t)__builtin_amdgcn_readlane((int)(re >> 32), k) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)re, k);
#pragma unroll
                        for (int q = 0; q < 4; ++q) decay |= (4 * i + q >= b && 4 * i + q < e) ? 1u << q : 0u;
                    }
                }
            }
            if (!live) continue;
        }
        float* pp = &pv.x; const float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
        if constexpr (OPT) {
#pragma unroll
            for (int e = 0; e < 4; ++e) pp[e] = (decay >> e & 1u) ? __fmul_rn(pp[e], o->decay_mul) : pp[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gr = gp[e] * gscale;
            mp[e] = mp[e] + (gr - mp[e]) * omb1;
            vp[e] = vp[e] * b2 + omb2 * gr * gr;
            const float denom = sqrtf(vp[e]) / sqrt_bc2 + eps;
            pp[e] = pp[e] - step_size * (mp[e] / denom);
        }
        reinterpret_cast<float4*>(p)[i] = pv;
        reinterpret_cast<float4*>(m)[i] = mv;
        reinterpret_cast<float4*>(v)[i] = vv;
        if constexpr (EMA) {
            float4 ev = reinterpret_cast<float4*>(o->ema)[i];
            float* ep = &ev.x;
#pragma unroll
            for (int e = 0; e < 4; ++e) ep[e] = ep[e] + (pp[e] - ep[e]) * o->ema_omd;
            reinterpret_cast<float4*>(o->ema)[i] = ev;
        }
    }
    if constexpr (EMA) {                                            // the small second buffer: the last workgroup, element by element
        if (blockIdx.x == gridDim.x - 1)
            for (int j = threadIdx.x; j < o->n_aux; j += 256) {
                const float a = o->aux[j], e = o->aux_ema[j];
                o->aux_ema[j] = e + (a - e) * o->ema_omd;
            }
    }
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n4,
                                                   float omb1, float b2, float omb2, float step_size,
                                                   float sqrt_bc2, float eps, float gscale) {
    adam_update<false, false>(p, g, m, v, n4, omb1, b2, omb2, step_size, sqrt_bc2, eps, gscale, nullptr);
}

int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, int step, float lr, float b1, float b2,
                float eps, float gscale, hipStream_t st) {
    if (n % 4 != 0) { cvae_set_error("adam: n=%lld must be a multiple of 4", (long long)n); return -1; }
    if (n == 0) return 0;
    const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p, g, m, v, n4, 1.0f - b1, b2, 1.0f - b2,
                       (float)((double)lr / bc1), (float)sqrt(bc2), eps, gscale);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// ---- guarded step (include/cvae.h): gradient statistics -> decision record -> Adam that obeys it ----
// One pass over the flat gradient: per-thread fp64 sum of (g * gscale)^2 and an OR of "exponent bits all set", reduced per
// wave (xor shuffles), per workgroup (four LDS words, fixed order) and over the workgroups by the LAST one to arrive
// (wg_arrive_last; partial k is read by thread k % 256 in ascending k, then the same wave / LDS tree): every addition has a
// fixed place, so the record depends on the buffer alone.  No floating-point atomics.
constexpr int GUARD_MAX_WGS = 256;       // one workgroup per compute unit.  Every workgroup draws a ticket from ONE word: with 2 048 the pass took 41.1 us, with 256 10.7 us (LABNOTES, profiles/r10_a_*)
struct GuardState {
    cvae_guard_record rec;
    double part[GUARD_MAX_WGS];
    uint32_t flag[GUARD_MAX_WGS];
};
static_assert(sizeof(cvae_guard_record) == 64 && offsetof(cvae_guard_record, norm64) == 16 && offsetof(cvae_guard_record, t) == 24 &&
              offsetof(cvae_guard_record, step_size) == 40 && offsetof(cvae_guard_record, ticket) == 60, "cvae_guard_record: the documented layout");
int64_t guard_state_bytes() { return (int64_t)sizeof(GuardState); }

__global__ __launch_bounds__(256) void guard_init_kernel(GuardState* s, int64_t applied, int64_t skipped) {
    uint32_t* w = reinterpret_cast<uint32_t*>(s);
    for (int i = threadIdx.x; i < (int)(sizeof(GuardState) / 4); i += 256) w[i] = 0u;
    __syncthreads();
    if (threadIdx.x == 0) { s->rec.t = applied; s->rec.skipped = skipped; s->rec.coef = 1.0f; }
}
int launch_guard_init(void* state, int64_t applied, int64_t skipped, hipStream_t st) {
    hipLaunchKernelGGL(guard_init_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<GuardState*>(state), applied, skipped);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// sum and flag of one workgroup in thread 0 (the other threads return garbage-free but unused values)
__device__ __forceinline__ void guard_wg_reduce(double& acc, unsigned& bad, double* red, unsigned* redf) {
    acc = wave_sum_d(acc);
    bad = __any((int)bad) ? 1u : 0u;
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = acc; redf[threadIdx.x >> 6] = bad; }
    __syncthreads();
    acc = (red[0] + red[1]) + (red[2] + red[3]);
    bad = redf[0] | redf[1] | redf[2] | redf[3];
}

__global__ __launch_bounds__(256) void grad_stats_kernel(const float* __restrict__ g, int64_t n4, float gscale, float max_norm,
                                                         int skip_nonfinite, float lr, float b1, float b2, GuardState* s) {
    __shared__ double red[4];
    __shared__ unsigned redf[4];
    __shared__ unsigned last_flag;
    const double sc = (double)gscale;
    double acc = 0.0;
    unsigned bad = 0u;
#pragma unroll 4
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        const float* gp = &gv.x;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double d = (double)gp[e] * sc;
            acc += d * d;
            bad |= (__float_as_uint(gp[e]) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
        }
    }
    guard_wg_reduce(acc, bad, red, redf);
    if (threadIdx.x == 0) { s->part[blockIdx.x] = acc; s->flag[blockIdx.x] = bad; }
    if (!wg_arrive_last(&s->rec.ticket, gridDim.x, &last_flag)) return;
    acc = 0.0;
    bad = 0u;
    for (unsigned k = threadIdx.x; k < gridDim.x; k += 256) { acc += s->part[k]; bad |= s->flag[k]; }
    guard_wg_reduce(acc, bad, red, redf);
    if (threadIdx.x != 0) return;
    cvae_guard_record& r = s->rec;
    const double norm = sqrt(acc);
    const int apply = (skip_nonfinite && bad) ? 0 : 1;
    const float coef = (float)fmin(1.0, (double)max_norm / (norm + 1e-6));      // clip_grad_norm_; fmin drops a NaN quotient (inf / inf): 1
    int64_t t = r.t, skipped = r.skipped;
    if (apply) ++t; else ++skipped;
    float step_size = 0.f, sqrt_bc2 = 0.f;
    if (apply) {                                                                // launch_adam's host arithmetic, on the device's own t
        const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
        step_size = (float)((double)lr / bc1);
        sqrt_bc2 = (float)sqrt(bc2);
    }
    r.apply = apply;
    r.nonfinite = bad;
    r.coef = coef;
    r.norm = (float)norm;
    r.norm64 = norm;
    r.t = t;
    r.skipped = skipped;
    r.step_size = step_size;
    r.sqrt_bc2 = sqrt_bc2;
    r.gscale = gscale * coef;
    r.beta1 = b1;
    r.beta2 = b2;
}
int launch_grad_stats(const float* g, int64_t n, float gscale, float max_norm, int skip_nonfinite, float lr, float b1, float b2,
                      void* state, hipStream_t st) {
    if (n % 4 != 0) { cvae_set_error("grad stats: n=%lld must be a multiple of 4", (long long)n); return -1; }
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > GUARD_MAX_WGS) blocks = GUARD_MAX_WGS;
    if (blocks < 1) blocks = 1;                              // n == 0: norm 0, still one decision
    hipLaunchKernelGGL(grad_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g, n4, gscale, max_norm, skip_nonfinite, lr, b1, b2,
                       reinterpret_cast<GuardState*>(state));
    CVAE_CHECK_LAUNCH();
    return 0;
}

// adam_kernel with its scalars read from the finished record; apply == 0: no store at all
__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, int64_t n4, float eps,
                                                           const cvae_guard_record* __restrict__ r) {
    if (r->apply == 0) return;
    const float b1 = r->beta1, b2 = r->beta2;
    adam_update<false, false>(p, g, m, v, n4, 1.0f - b1, b2, 1.0f - b2, r->step_size, r->sqrt_bc2, eps, r->gscale, nullptr);
}
int launch_adam_guarded(float* p, const float* g, float* m, float* v, int64_t n, float eps, const void* state, hipStream_t st) {
    if (n % 4 != 0) { cvae_set_error("guarded adam: n=%lld must be a multiple of 4", (long long)n); return -1; }
    if (n == 0) return 0;
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(adam_guarded_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p, g, m, v, n4, eps,
                       &reinterpret_cast<const GuardState*>(state)->rec);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// ---- the optimizer options (include/cvae.h): decoupled weight decay on element ranges, an EMA of the parameters and of one
// small auxiliary buffer, inside the same single pass.  The plain and the guarded kernel above stay as they are. ----
template <bool EMA>
__global__ __launch_bounds__(256) void adam_opt_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, int64_t n4, float omb1, float b2, float omb2,
                                                       float step_size, float sqrt_bc2, float eps, float gscale, OptArgs o) {
    adam_update<true, EMA>(p, g, m, v, n4, omb1, b2, omb2, step_size, sqrt_bc2, eps, gscale, &o);
}
// apply == 0: no store at all, the EMA buffers included
template <bool EMA>
__global__ __launch_bounds__(256) void adam_guarded_opt_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                               float* __restrict__ m, float* __restrict__ v, int64_t n4, float eps,
                                                               const cvae_guard_record* __restrict__ r, OptArgs o) {
    if (r->apply == 0) return;
    const float b1 = r->beta1, b2 = r->beta2;
    adam_update<true, EMA>(p, g, m, v, n4, 1.0f - b1, b2, 1.0f - b2, r->step_size, r->sqrt_bc2, eps, r->gscale, &o);
}

// The checked cvae_opt_args -> the kernels' OptArgs.  ema_omd == 0 moves no average: such a launch is the one without an EMA.
static OptArgs opt_pack(const cvae_opt_args* opt, float* ema, const float* aux, float* aux_ema, int32_t n_aux) {
    OptArgs o{};
    o.decay_mul = opt->decay_mul;
    o.r.n = opt->n_ranges;
    for (int k = 0; k < opt->n_ranges; ++k) { o.r.begin[k] = opt->begin[k]; o.r.end[k] = opt->end[k]; }
    if (ema && opt->ema_omd != 0.f) {
        o.ema = ema; o.ema_omd = opt->ema_omd;
        if (n_aux > 0) { o.aux = aux; o.aux_ema = aux_ema; o.n_aux = n_aux; }
    }
    return o;
}
static unsigned opt_blocks(int64_t n4) {
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    return (unsigned)(blocks < 1 ? 1 : blocks);              // n == 0 with an auxiliary buffer: one workgroup for it
}
int launch_adam_opt(float* p, const float* g, float* m, float* v, int64_t n, int step, float lr, float b1, float b2, float eps,
                    float gscale, const cvae_opt_args* opt, float* ema, const float* aux, float* aux_ema, int32_t n_aux, hipStream_t st) {
    const OptArgs o = opt_pack(opt, ema, aux, aux_ema, n_aux);
    if (n == 0 && o.n_aux == 0) return 0;
    const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
    const int64_t n4 = n / 4;
    const float step_size = (float)((double)lr / bc1), sqrt_bc2 = (float)sqrt(bc2);
    if (o.ema) hipLaunchKernelGGL(adam_opt_kernel<true>, dim3(opt_blocks(n4)), dim3(256), 0, st, p, g, m, v, n4, 1.0f - b1, b2, 1.0f - b2,
                                  step_size, sqrt_bc2, eps, gscale, o);
    else hipLaunchKernelGGL(adam_opt_kernel<false>, dim3(opt_blocks(n4)), dim3(256), 0, st, p, g, m, v, n4, 1.0f - b1, b2, 1.0f - b2,
                            step_size, sqrt_bc2, eps, gscale, o);
    CVAE_CHECK_LAUNCH();
    return 0;
}
int launch_adam_guarded_opt(float* p, const float* g, float* m, float* v, int64_t n, float eps, const void* state,
                            const cvae_opt_args* opt, float* ema, const float* aux, float* aux_ema, int32_t n_aux, hipStream_t st) {
    const OptArgs o = opt_pack(opt, ema, aux, aux_ema, n_aux);
    if (n == 0 && o.n_aux == 0) return 0;
    const int64_t n4 = n / 4;
    const cvae_guard_record* rec = &reinterpret_cast<const GuardState*>(state)->rec;
    if (o.ema) hipLaunchKernelGGL(adam_guarded_opt_kernel<true>, dim3(opt_blocks(n4)), dim3(256), 0, st, p, g, m, v, n4, eps, rec, o);
    else hipLaunchKernelGGL(adam_guarded_opt_kernel<false>, dim3(opt_blocks(n4)), dim3(256), 0, st, p, g, m, v, n4, eps, rec, o);
    CVAE_CHECK_LAUNCH();
    return 0;
}

__global__ __launch_bounds__(256) void zero_kernel(float4* __restrict__ p, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
        p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
int launch_zero(float* p, int64_t n, hipStream_t st) {
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(zero_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<float4*>(p), n4);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// Alignment padding between the tensors of the flat gradient buffer (<= 63 floats each): written as 0 so a
// caller may hand cvae_backward an uninitialised buffer (phase bit 3).  One workgroup per tensor gap.
__global__ __launch_bounds__(64) void zero_gaps_kernel(float* __restrict__ g, PadGaps gaps) {
    const int64_t o = gaps.off[blockIdx.x];
    if ((int)threadIdx.x < gaps.len[blockIdx.x]) g[o + threadIdx.x] = 0.f;
}
int launch_zero_gaps(float* grads, const PadGaps& gaps, hipStream_t st) {
    if (gaps.n == 0) return 0;
    hipLaunchKernelGGL(zero_gaps_kernel, dim3(gaps.n), dim3(64), 0, st, grads, gaps);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// out_k = in_k * g[0] for the three loss gradients in ONE launch (the chain-rule factor autograd hands
// total_loss.backward(): a device scalar, so no host read)
__global__ __launch_bounds__(256) void scale3_kernel(Scale3 a) {
    const float g = a.g[0];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int64_t j = i; j < a.n[k]; j += (int64_t)gridDim.x * 256) a.dst[k][j] = a.src[k][j] * g;
}
int launch_scale3(const Scale3& a, hipStream_t st) {
    int64_t nmax = a.n[0] > a.n[1] ? a.n[0] : a.n[1];
    if (a.n[2] > nmax) nmax = a.n[2];
    int64_t blocks = (nmax + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(scale3_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// fp32 <-> bf16 copies of a gradient range for the optional bf16 all-reduce (5.17 MB instead of 10.34 MB on
// the wire); RNE on the way down, exact on the way up.  n is a multiple of 64 (bucket ranges are).
__global__ __launch_bounds__(256) void grads_pack_bf16_kernel(const float* __restrict__ src, __bf16* __restrict__ dst, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + i * 4);
    bf16x4 o;
    o[0] = (__bf16)v[0]; o[1] = (__bf16)v[1]; o[2] = (__bf16)v[2]; o[3] = (__bf16)v[3];
    *reinterpret_cast<bf16x4*>(dst + i * 4) = o;
}
__global__ __launch_bounds__(256) void grads_unpack_bf16_kernel(const __bf16* __restrict__ src, float* __restrict__ dst, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(src + i * 4);
    *reinterpret_cast<f32x4*>(dst + i * 4) = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
int launch_grads_bf16(const float* src_f32, void* bf16_buf, float* dst_f32, int64_t n, hipStream_t st) {
    if (n % 4 != 0) { cvae_set_error("grads bf16 copy: n = %lld is not a multiple of 4", (long long)n); return -2; }
    if (n == 0) return 0;                                    // an empty range is a no-op, not a zero-block launch
    const int64_t n4 = n / 4;
    const unsigned blocks = (unsigned)((n4 + 255) / 256);
    if (src_f32) hipLaunchKernelGGL(grads_pack_bf16_kernel, dim3(blocks), dim3(256), 0, st, src_f32, reinterpret_cast<__bf16*>(bf16_buf), n4);
    else hipLaunchKernelGGL(grads_unpack_bf16_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const __bf16*>(bf16_buf), dst_f32, n4);
    CVAE_CHECK_LAUNCH();
    return 0;
}
