// trace.hip — the training trace (include/cvae.h): cvae_trace_push writes one 128-byte step row into a caller-owned ring,
// cvae_tensor_stats leaves per-tensor sums of squares, maxima and non-finite counts of the flat buffers as the optimizer left
// them.  The pattern of grad_stats_kernel (adam.hip): fp64 partials, a fixed-order merge by the last workgroup to arrive, no
// floating-point atomics, nothing read on the host.
#include "common.h"
#include "../../include/cvae.h"
#include <math.h>
#include <stddef.h>

static_assert(sizeof(cvae_trace_row) == 128 && offsetof(cvae_trace_row, step) == 0 && offsetof(cvae_trace_row, lr) == 8 &&
              offsetof(cvae_trace_row, applied) == 12 && offsetof(cvae_trace_row, nonfinite) == 16 &&
              offsetof(cvae_trace_row, grad_norm) == 20 && offsetof(cvae_trace_row, coef) == 24 &&
              offsetof(cvae_trace_row, n_scalars) == 28 && offsetof(cvae_trace_row, reserved) == 32 &&
              offsetof(cvae_trace_row, scalars) == 64, "cvae_trace_row: the documented layout");
static_assert(sizeof(cvae_tensor_stat) == 48 && offsetof(cvae_tensor_stat, g2) == 0 && offsetof(cvae_tensor_stat, p2) == 8 &&
              offsetof(cvae_tensor_stat, u2) == 16 && offsetof(cvae_tensor_stat, gmax) == 24 && offsetof(cvae_tensor_stat, pmax) == 28 &&
              offsetof(cvae_tensor_stat, g_nonfinite) == 32 && offsetof(cvae_tensor_stat, p_nonfinite) == 36 &&
              offsetof(cvae_tensor_stat, step) == 40, "cvae_tensor_stat: the documented layout");
static_assert(CVAE_TRACE_MAX_SCALARS == 16, "cvae_trace_row holds 16 scalars");

// ---- the step row: 32 dwords, lane d writes dword d of the row (every byte of it, nothing else) ----
__global__ __launch_bounds__(64) void trace_push_kernel(uint32_t* __restrict__ row, int64_t step, float lr,
                                                        const uint32_t* __restrict__ scalars, int n_scalars,
                                                        const cvae_guard_record* __restrict__ rec) {
    const int d = threadIdx.x;
    if (d >= 32) return;
    uint32_t w = 0u;
    switch (d) {
        case 0: w = (uint32_t)((uint64_t)step & 0xffffffffull); break;
        case 1: w = (uint32_t)((uint64_t)step >> 32); break;
        case 2: w = __float_as_uint(lr); break;
        case 3: w = rec ? (uint32_t)rec->apply : 1u; break;
        case 4: w = rec ? rec->nonfinite : 0u; break;
        case 5: w = rec ? __float_as_uint(rec->norm) : 0x7fc00000u; break;
        case 6: w = rec ? __float_as_uint(rec->coef) : __float_as_uint(1.0f); break;
        case 7: w = (uint32_t)n_scalars; break;
        default: if (d >= 16 && d - 16 < n_scalars) w = scalars[d - 16];
    }
    row[d] = w;
}
int launch_trace_push(void* ring, int64_t capacity, int64_t step, float lr, const float* scalars, int n_scalars,
                      const void* guard_state, hipStream_t st) {
    uint32_t* row = reinterpret_cast<uint32_t*>(reinterpret_cast<cvae_trace_row*>(ring) + (step - 1) % capacity);
    hipLaunchKernelGGL(trace_push_kernel, dim3(1), dim3(64), 0, st, row, step, lr, reinterpret_cast<const uint32_t*>(scalars), n_scalars,
                       reinterpret_cast<const cvae_guard_record*>(guard_state));
    CVAE_CHECK_LAUNCH();
    return 0;
}

// ---- per-tensor statistics ----
constexpr int TS_CHUNK = 4096;           // elements per item: four trips of 256 threads x float4
constexpr int TS_MAX_WGS = 256;          // one workgroup per compute unit; every workgroup draws a ticket from one word (adam.hip)
constexpr int TS_HEADER_BYTES = 16;      // the arrival counter, in a block of its own at the start of scratch (zeroed per call)
struct TsPartial {                       // what one item leaves in scratch; 40 bytes
    double g2, p2, u2;
    float gmax, pmax;
    uint32_t gnf, pnf;
};
static_assert(sizeof(TsPartial) == 40, "TsPartial: five 8-byte words");
// The tensor table as the kernel takes it: by value in the launch, as OptRanges is.  item0[t] = index of tensor t's first item.
struct TsTable {
    int32_t n, items;
    int64_t begin[CVAE_TRACE_MAX_TENSORS], end[CVAE_TRACE_MAX_TENSORS];
    int32_t item0[CVAE_TRACE_MAX_TENSORS + 1];
};

struct TsAcc {
    double g2, p2, u2;
    float gmax, pmax;
    uint32_t gnf, pnf;
};
template <bool UPD>
__device__ __forceinline__ void ts_element(TsAcc& a, float p, float graw, float m, float v, float gscale, float step_size,
                                           float sqrt_bc2, float eps) {
    const float g = graw * gscale;
    a.g2 += (double)g * (double)g;
    a.p2 += (double)p * (double)p;
    const float ga = fabsf(g), pa = fabsf(p);
    if (ga > a.gmax) a.gmax = ga;                     // a NaN compares false: it never enters
    if (pa > a.pmax) a.pmax = pa;
    a.gnf += (__float_as_uint(graw) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
    a.pnf += (__float_as_uint(p) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
    if constexpr (UPD) {                              // adam_update's expressions on the moments it left
        const float denom = sqrtf(v) / sqrt_bc2 + eps;
        const float u = step_size * (m / denom);
        a.u2 += (double)u * (double)u;
    }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_u(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
__device__ __forceinline__ void ts_wave_reduce(TsAcc& a) {
    a.g2 = wave_sum_d(a.g2); a.p2 = wave_sum_d(a.p2); a.u2 = wave_sum_d(a.u2);
    a.gmax = wave_max(a.gmax); a.pmax = wave_max(a.pmax);          // no NaN in here: fmaxf is plain max
    a.gnf = wave_sum_u(a.gnf); a.pnf = wave_sum_u(a.pnf);
}

// One item = elements [b, e) of the flat buffers, e - b <= TS_CHUNK.  `vec`: all four buffers are 16-byte aligned, so element
// index i is 16-byte aligned in all of them exactly when i % 4 == 0.
template <bool UPD>
__device__ __forceinline__ void ts_item(TsAcc& a, const float* __restrict__ p, const float* __restrict__ g,
                                        const float* __restrict__ m, const float* __restrict__ v, int64_t b, int64_t e, bool vec,
                                        float gscale, float step_size, float sqrt_bc2, float eps) {
    const int tid = threadIdx.x;
    if (!vec) {
        for (int64_t i = b + tid; i < e; i += 256) ts_element<UPD>(a, p[i], g[i], m[i], v[i], gscale, step_size, sqrt_bc2, eps);
        return;
    }
    int64_t b4 = (b + 3) & ~(int64_t)3;               // first aligned element ...
    if (b4 > e) b4 = e;
    const int64_t e4 = b4 + ((e - b4) & ~(int64_t)3); // ... and the end of the last whole float4
    if (b + tid < b4) { const int64_t i = b + tid; ts_element<UPD>(a, p[i], g[i], m[i], v[i], gscale, step_size, sqrt_bc2, eps); }
    for (int64_t i = b4 + 4 * (int64_t)tid; i < e4; i += 1024) {
        const float4 pv = *reinterpret_cast<const float4*>(p + i), gv = *reinterpret_cast<const float4*>(g + i);
        float4 mv = make_float4(0.f, 0.f, 0.f, 0.f), vv = mv;
        if constexpr (UPD) { mv = *reinterpret_cast<const float4*>(m + i); vv = *reinterpret_cast<const float4*>(v + i); }
        const float* pp = &pv.x; const float* gp = &gv.x; const float* mp = &mv.x; const float* vp = &vv.x;
#pragma unroll
        for (int q = 0; q < 4; ++q) ts_element<UPD>(a, pp[q], gp[q], mp[q], vp[q], gscale, step_size, sqrt_bc2, eps);
    }
    if (e4 + tid < e) { const int64_t i = e4 + tid; ts_element<UPD>(a, p[i], g[i], m[i], v[i], gscale, step_size, sqrt_bc2, eps); }
}

__global__ __launch_bounds__(256) void tensor_stats_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                           const float* __restrict__ m, const float* __restrict__ v, TsTable tb,
                                                           int64_t step, float step_size, float sqrt_bc2, float eps, float gscale,
                                                           const cvae_guard_record* __restrict__ rec, cvae_tensor_stat* out,
                                                           unsigned* ticket, TsPartial* part, int vec) {
    __shared__ TsAcc red[4];
    __shared__ unsigned last_flag;
    bool upd = true;
    if (rec) {                                         // written by an earlier launch: plain loads
        upd = rec->apply != 0;
        step_size = rec->step_size; sqrt_bc2 = rec->sqrt_bc2; gscale = rec->gscale;
    }
    for (int it = blockIdx.x; it < tb.items; it += gridDim.x) {
        int t = 0;                                     // the tensor of item `it`: item0 ascends, at most 32 entries, uniform
        while (t + 1 < tb.n && tb.item0[t + 1] <= it) ++t;
        const int64_t b = tb.begin[t] + (int64_t)(it - tb.item0[t]) * TS_CHUNK;
        const int64_t e = b + TS_CHUNK < tb.end[t] ? b + TS_CHUNK : tb.end[t];
        TsAcc a{};
        if (upd) ts_item<true>(a, p, g, m, v, b, e, vec != 0, gscale, step_size, sqrt_bc2, eps);
        else ts_item<false>(a, p, g, m, v, b, e, vec != 0, gscale, step_size, sqrt_bc2, eps);
        ts_wave_reduce(a);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
        __syncthreads();
        if (threadIdx.x == 0) {
            TsPartial o;
            o.g2 = (red[0].g2 + red[1].g2) + (red[2].g2 + red[3].g2);
            o.p2 = (red[0].p2 + red[1].p2) + (red[2].p2 + red[3].p2);
            o.u2 = (red[0].u2 + red[1].u2) + (red[2].u2 + red[3].u2);
            o.gmax = fmaxf(fmaxf(red[0].gmax, red[1].gmax), fmaxf(red[2].gmax, red[3].gmax));
            o.pmax = fmaxf(fmaxf(red[0].pmax, red[1].pmax), fmaxf(red[2].pmax, red[3].pmax));
            o.gnf = red[0].gnf + red[1].gnf + red[2].gnf + red[3].gnf;
            o.pnf = red[0].pnf + red[1].pnf + red[2].pnf + red[3].pnf;
            part[it] = o;
        }
        __syncthreads();                               // red is free for the next item
    }
    if (!wg_arrive_last(ticket, gridDim.x, &last_flag)) return;
    // the merge: wave w takes tensors w, w + 4, ...; lane l sums chunks l, l + 64, ... in ascending order, then the xor tree
    const int lane = threadIdx.x & 63;
    for (int t = threadIdx.x >> 6; t < tb.n; t += 4) {
        TsAcc a{};
        for (int k = tb.item0[t] + lane; k < tb.item0[t + 1]; k += 64) {
            const TsPartial q = part[k];
            a.g2 += q.g2; a.p2 += q.p2; a.u2 += q.u2;
            a.gmax = fmaxf(a.gmax, q.gmax); a.pmax = fmaxf(a.pmax, q.pmax);
            a.gnf += q.gnf; a.pnf += q.pnf;
        }
        ts_wave_reduce(a);
        if (lane == 0) {
            cvae_tensor_stat s;
            s.g2 = a.g2; s.p2 = a.p2; s.u2 = a.u2; s.gmax = a.gmax; s.pmax = a.pmax;
            s.g_nonfinite = a.gnf; s.p_nonfinite = a.pnf; s.step = step;
            out[t] = s;
        }
    }
}

// the table of a checked range list; -1 (error set) for a list the entry refuses.  Host logic only.
static int ts_table(const char* who, int32_t n_tensors, const int64_t* begin, const int64_t* end, int64_t n, TsTable* tb) {
    if (!begin || !end) { cvae_set_error("%s: null range table", who); return -1; }
    if (n_tensors < 1 || n_tensors > CVAE_TRACE_MAX_TENSORS) {
        cvae_set_error("%s: n_tensors = %d outside 1..%d", who, (int)n_tensors, CVAE_TRACE_MAX_TENSORS); return -1;
    }
    int64_t prev = 0, items = 0;
    for (int t = 0; t < n_tensors; ++t) {
        const int64_t b = begin[t], e = end[t];
        if (b >= e || b < prev || (n >= 0 && e > n)) {
            cvae_set_error("%s: range %d = [%lld, %lld): ranges must be non-empty, ascending, disjoint and within [0, n)", who, t,
                           (long long)b, (long long)e);
            return -1;
        }
        prev = e;
        tb->begin[t] = b; tb->end[t] = e;
        tb->item0[t] = (int32_t)items;
        items += (e - b + TS_CHUNK - 1) / TS_CHUNK;
        if (items > (int64_t)1 << 30) { cvae_set_error("%s: more than 2^30 chunks of %d elements", who, TS_CHUNK); return -1; }
    }
    for (int t = n_tensors; t <= CVAE_TRACE_MAX_TENSORS; ++t) tb->item0[t] = (int32_t)items;
    for (int t = n_tensors; t < CVAE_TRACE_MAX_TENSORS; ++t) { tb->begin[t] = 0; tb->end[t] = 0; }
    tb->n = n_tensors;
    tb->items = (int32_t)items;
    return 0;
}
static int ts_grid(int items) {
    int G = cvae_num_cus();
    if (G > TS_MAX_WGS) G = TS_MAX_WGS;
    return G < items ? G : items;
}
int tensor_stats_plan(int32_t n_tensors, const int64_t* begin, const int64_t* end, int32_t* chunk, int32_t* items, int32_t* grid) {
    TsTable tb;
    if (ts_table("cvae_tensor_stats_plan", n_tensors, begin, end, -1, &tb) != 0) return -1;
    *chunk = TS_CHUNK; *items = tb.items; *grid = ts_grid(tb.items);
    return 0;
}
int64_t tensor_stats_scratch_bytes(int32_t n_tensors, const int64_t* begin, const int64_t* end) {
    TsTable tb;
    if (ts_table("cvae_tensor_stats_scratch_bytes", n_tensors, begin, end, -1, &tb) != 0) return -1;
    return align_up(TS_HEADER_BYTES + (int64_t)tb.items * (int64_t)sizeof(TsPartial), 16);
}

int launch_tensor_stats(const float* p, const float* g, const float* m, const float* v, int64_t n, int32_t n_tensors,
                        const int64_t* begin, const int64_t* end, int64_t step, float lr, float b1, float b2, float eps, float gscale,
                        const void* guard_state, cvae_tensor_stat* out, void* scratch, hipStream_t st) {
    TsTable tb;
    if (ts_table("cvae_tensor_stats", n_tensors, begin, end, n, &tb) != 0) return -1;
    const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);     // launch_adam's
    const float step_size = (float)((double)lr / bc1), sqrt_bc2 = (float)sqrt(bc2);
    const int vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15u) == 0 ? 1 : 0;
    hipError_t e = hipMemsetAsync(scratch, 0, TS_HEADER_BYTES, st);
    if (e != hipSuccess) { cvae_set_error("cvae_tensor_stats: zeroing the arrival counter failed: %s", hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(tensor_stats_kernel, dim3((unsigned)ts_grid(tb.items)), dim3(256), 0, st, p, g, m, v, tb, step, step_size, sqrt_bc2,
                       eps, gscale, reinterpret_cast<const cvae_guard_record*>(guard_state), out, reinterpret_cast<unsigned*>(scratch),
                       reinterpret_cast<TsPartial*>(reinterpret_cast<char*>(scratch) + TS_HEADER_BYTES), vec);
    CVAE_CHECK_LAUNCH();
    return 0;
}
