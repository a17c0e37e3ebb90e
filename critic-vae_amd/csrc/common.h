// common.h — shared host/device declarations for libcvae_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <atomic>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));     // one v_mfma_f32_32x32x16_bf16 operand fragment

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// Activation storage type of a run: fp32 (precision modes 0, 2, 3) or bf16 (precision mode 1: y_l, a_l, h, o_i and
// their gradients live in HBM as bf16; BatchNorm statistics, loss scalars, master weights and the flat gradient
// stay fp32).  Tensor pointers cross the launchers as opaque float*; kernels index them in ELEMENTS through Act<AT>.
template <typename AT> struct Act;
template <> struct Act<float> {
    static constexpr bool BF16 = false;
    static __device__ __forceinline__ float ld(const float* p, size_t i) { return p[i]; }
    static __device__ __forceinline__ void st(float* p, size_t i, float v) { p[i] = v; }
    static __device__ __forceinline__ f32x4 ld4(const float* p, size_t i) { return *reinterpret_cast<const f32x4*>(p + i); }
    static __device__ __forceinline__ void st4(float* p, size_t i, f32x4 v) { *reinterpret_cast<f32x4*>(p + i) = v; }
    // V consecutive elements in one access (bn.hip): a scalar or a float4.  v[e] reads / writes element e.
    template <int V> using Vec = float __attribute__((ext_vector_type(V)));
    template <int V> static __device__ __forceinline__ Vec<V> ldv(const float* p, size_t i) {
        static_assert(V == 1 || V == 4, "fp32 storage: scalar or float4 accesses");
        return *reinterpret_cast<const Vec<V>*>(p + i);
    }
    template <int V> static __device__ __forceinline__ void stv(float* p, size_t i, Vec<V> v) {
        static_assert(V == 1 || V == 4, "fp32 storage: scalar or float4 accesses");
        *reinterpret_cast<Vec<V>*>(p + i) = v;
    }
};
template <> struct Act<__bf16> {
    static constexpr bool BF16 = true;
    static __device__ __forceinline__ float ld(const float* p, size_t i) { return (float)reinterpret_cast<const __bf16*>(p)[i]; }
    static __device__ __forceinline__ void st(float* p, size_t i, float v) { reinterpret_cast<__bf16*>(p)[i] = (__bf16)v; }
    static __device__ __forceinline__ f32x4 ld4(const float* p, size_t i) {
        const bf16x4 v = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(p) + i);
        return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    }
    static __device__ __forceinline__ void st4(float* p, size_t i, f32x4 v) {
        bf16x4 o;
        o[0] = (__bf16)v[0]; o[1] = (__bf16)v[1]; o[2] = (__bf16)v[2]; o[3] = (__bf16)v[3];
        *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(p) + i) = o;
    }
    static __device__ __forceinline__ bf16x4 ld4raw(const float* p, size_t i) { return *reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(p) + i); }
    // 8 consecutive elements = one 16-byte unit
    static __device__ __forceinline__ bf16x8 ld8(const float* p, size_t i) { return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const __bf16*>(p) + i); }
    static __device__ __forceinline__ void st8(float* p, size_t i, bf16x8 v) { *reinterpret_cast<bf16x8*>(reinterpret_cast<__bf16*>(p) + i) = v; }
    // V consecutive elements in one access (bn.hip): the 16-byte unit.  (float)v[e] widens, v[e] = (__bf16)x rounds.
    template <int V> using Vec = __bf16 __attribute__((ext_vector_type(V)));
    template <int V> static __device__ __forceinline__ Vec<V> ldv(const float* p, size_t i) {
        static_assert(V == 8, "bf16 storage: 16-byte units of 8 elements");
        return ld8(p, i);
    }
    template <int V> static __device__ __forceinline__ void stv(float* p, size_t i, Vec<V> v) {
        static_assert(V == 8, "bf16 storage: 16-byte units of 8 elements");
        st8(p, i, v);
    }
};

// 8 k-values of this lane for one bf16 MFMA operand out of a row-major [k rows][channel columns] LDS image: two
// transposed 4x16 reads (ds_read_b64_tr_b16; within each group of 16 lanes, lane 4q+p supplies the address of row q,
// columns 4p..4p+3 of a 4 x 16 block and lane i receives column i of the 4 rows — profiles/experiments/tr16_probe.hip).
// EXEC must be all ones; addresses 8-byte aligned.
typedef short short4v __attribute__((ext_vector_type(4)));
typedef short short8v __attribute__((ext_vector_type(8)));
__device__ __forceinline__ bf16x8 tr_frag(const __bf16* p0, const __bf16* p1) {
    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)p0);
    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)p1);
    const short8v v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

#define CVAE_LATENT 32
#define CVAE_ZCAT 33

// Conv layers of the path.  0..3 encoder (vae_nets.py:69,74,79,84), 4..8 decoder (:117-133).
// h = output spatial size at width 64 (scaled by width/64 at run time); up = input is the
// nearest-2x upsample of the stored tensor (vae_nets.py:119,123,127,131).
struct LayerDesc { int cin, cout, h, up; };
static constexpr LayerDesc kLayers[9] = {
    {3, 32, 64, 0}, {32, 64, 32, 0}, {64, 128, 16, 0}, {128, 256, 8, 0},
    {256, 128, 4, 0}, {128, 64, 8, 1}, {64, 32, 16, 1}, {32, 32, 32, 1}, {32, 3, 64, 1}};

// ---- output-tile geometry shared by the conv kernels: 128 output pixels per workgroup ----
// One arithmetic for the kernels (Tile<H>) and for the host side that sizes and reads the per-tile BatchNorm partials (bn.hip).
struct TileGeom { int TW, TH, IMGS, PX_PER_IMG, TILES_PER_IMG; };
__host__ __device__ constexpr TileGeom tile_geom(int H) {
    const int TW = H < 32 ? H : 32;
    const int TH = (128 / TW) < H ? (128 / TW) : H;
    return TileGeom{TW, TH, 128 / (TW * TH), TW * TH, (H / TW) * (H / TH)};
}
template <int H>
struct Tile {
    static constexpr int TW = tile_geom(H).TW, TH = tile_geom(H).TH;
    static constexpr int IMGS = tile_geom(H).IMGS;       // whole images per tile when H*H < 128
    static constexpr int HTW = TW + 4, HTH = TH + 4;     // halo for the 5x5 window
    static constexpr int HPI = HTW * HTH;                // halo pixels per image
    static constexpr int HP = IMGS * HPI;
    static constexpr int PS = ((HP + 5) / 8) * 8 + 2;    // LDS plane stride, == 2 (mod 8), >= HP
    static constexpr int TILES_X = H / TW, TILES_Y = H / TH;
    static constexpr int TILES_PER_IMG = tile_geom(H).TILES_PER_IMG;
    static_assert(TW * TH * IMGS == 128, "tile must hold 128 pixels");
};

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// `s_waitcnt vmcnt(0)` the compiler can SEE (the builtin, not inline asm), placed where a register-prefetch loop ends and nothing
// is in flight any more.  The loop's staging registers are load destinations; without this the compiler protects their reuse in the
// epilogue with counted waits (vmcnt(3), (2), (1) ...) that it derives from the loop body — and since vmcnt counts stores too and
// retires in order, such a wait placed after the epilogue's first global stores waits for THOSE (profiles/experiments/vm_after_store.py).
__device__ __forceinline__ void vm_drained() { __builtin_amdgcn_s_waitcnt(0x0F70); }      // gfx9 encoding: vmcnt = 0, expcnt / lgkmcnt untouched

// Workgroups are dealt to the 8 XCDs round-robin by linear id, and every XCD has its own L2.  Map
// workgroup x of a grid of G (G % 8 == 0) to tile (x % 8) * (G / 8) + x / 8: each XCD then owns a
// contiguous range of tiles — neighbouring tiles share their halo rows in ONE L2, and the workgroups of
// the other output-channel tiles (blockIdx.y) that re-read the same input tile sit on the same XCD.
__device__ __forceinline__ int xcd_tile(int x, int G) { return (G & 7) ? x : (x & 7) * (G >> 3) + (x >> 3); }
inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// In-launch "last workgroup to arrive" (cdna guide §6 Guideline 16, counter form; placement-independent): every wave
// drains its stores, the workgroup meets, ONE lane releases at agent scope, drains again and draws a ticket; the
// workgroup that draws total-1 acquires at agent scope and may then read, with plain loads, everything the other
// workgroups stored before they arrived.  Returns the same answer in every thread.  *counter must be 0 when the
// launch starts (zeroed by an EARLIER launch on the stream); the last arriver puts it back to 0.
__device__ __forceinline__ bool wg_arrive_last(unsigned* counter, unsigned total, unsigned* lds_word) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = t == total - 1;
        if (last) {
            __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *lds_word = last ? 1u : 0u;
    }
    __syncthreads();
    return *lds_word != 0u;
}

// Optional in-step kernel probe (api.hip): the launchers bracket their MAIN kernel with a HIP event
// pair on the stream it is launched on when the orchestration armed a slot (bench.py roofline).
void cvae_probe_begin(hipStream_t st);
void cvae_probe_end(hipStream_t st);

// error plumbing (api.hip)
void cvae_set_error(const char* fmt, ...);
#define CVAE_CHECK_LAUNCH()                                                        \
    do {                                                                           \
        hipError_t e_ = hipGetLastError();                                         \
        if (e_ != hipSuccess) {                                                    \
            cvae_set_error("%s:%d launch failed: %s", __FILE__, __LINE__,          \
                           hipGetErrorString(e_));                                 \
            return (int)e_;                                                        \
        }                                                                          \
    } while (0)

// The opt-in to more than 64 KB of dynamic LDS is a PER-DEVICE function attribute: remember, per kernel,
// the set of devices it has been granted on (idempotent, thread-safe; one handle per device may live in
// the same process).  `once` is a function-local static of the launcher that owns the kernel.
struct DeviceOnce { std::atomic<uint64_t> mask{0}; };
inline int cvae_grant_lds(DeviceOnce& once, const void* kernel, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    const uint64_t bit = 1ull << (dev & 63);
    if (e == hipSuccess && (once.mask.load(std::memory_order_acquire) & bit)) return 0;
    if (e == hipSuccess) e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) { cvae_set_error("dynamic LDS opt-in (%d bytes) failed: %s", bytes, hipGetErrorString(e)); return (int)e; }
    once.mask.fetch_or(bit, std::memory_order_release);
    return 0;
}

// Compute units of the current device (256 on the MI355X), queried once per device: sizes the persistent grids.
int cvae_num_cus();
// Grid of a persistent conv kernel (api.hip): wgs_per_cu workgroups per compute unit, capped by CVAE_PERSIST_MAXWG (tests: several items
// per workgroup), rounded down to a multiple of 8 (xcd_tile), at least 8 and at most num_items.
int persistent_grid(int wgs_per_cu, int num_items);

// Kernel family of a conv forward / input-gradient pass of layers 1..4 (E2..E4, D0); the codes are those of cvae_conv_route.
// CONV_PS: conv_mfma_ps.hip in fp32 mode, conv_bf16_ps.hip in bf16 mode; CONV_BIG: conv_bf16_big.hip.
// Layer 0 (E1) forward in bf16 mode: E1_PACKED_FRAME = E1's passes stage their strips from the packed bf16 frame (workspace slot xp),
// CONV_PER_TILE (0) = from the fp32 frame x.
enum ConvFamily { CONV_PER_TILE = 0, CONV_PS = 1, CONV_BIG = 2, E1_PACKED_FRAME = 1 };
struct ConvRoute {
    ConvFamily family;
    int tilesPerPartial;      // forward passes: 128-pixel tiles per BatchNorm partial row of bnpart
};
// conv_mfma.hip: the one table the conv launchers read (host logic only, never touches the device); precision as in cvae_config
ConvRoute conv_route(int precision, int layer, int width, bool dgrad, int64_t B);

// ---- launchers implemented across the .hip files (all asynchronous on `st`) ----
// conv_mfma.hip
int launch_conv_fwd(int layer, int width, int B, const float* in, const float* w, const float* bias,
                    float* out, float* bnpart, float* ws, hipStream_t st);
int64_t conv_fwd_ws_floats(int layer, int width, int B);
int launch_conv_dgrad(int layer, int width, int B, const float* dout, const float* w,
                      const float* mask_src, float* din, float* ws, hipStream_t st);   // ws: D0's split-K slabs at 64 x 64 (conv_dgrad_ws_floats)
int64_t conv_dgrad_ws_floats(int layer, int width, int B);
// conv_bf16.hip — precision mode 1: bf16-MFMA forward / dgrad / wgrad of layers 1..7
int64_t conv_bf16_pack_floats(int ns);
int launch_pack_w_bf16(const float* const w[4], float* packed, int ns, hipStream_t st);     // ns = 1 (bf16) or 3 (fp32 emulation)
int launch_conv_fwd_bf16(int layer, int width, int ns, int B, const float* in, const float* packed, const float* bias, float* out,
                         float* bnpart, float* ws, hipStream_t st, int* tilesPerPartial = nullptr);    // out: 128-pixel tiles per BatchNorm partial row
int launch_conv_dgrad_bf16(int layer, int width, int ns, int B, const float* dout, const float* packed, float* din, float* ws, hipStream_t st);
int launch_pack_up_bf16(const float* const wc[3], float* packed, int ns, hipStream_t st);
int launch_conv_up_fwd_bf16(int layer, int width, int ns, int B, const float* in, const float* packed, const float* bias, float* out, hipStream_t st);
int launch_conv_up_dgrad_bf16(int layer, int width, int ns, int B, const float* dout, const float* packed, const float* aux, float* din, hipStream_t st);
int64_t wgrad_bf16_ws_floats(int layer, int width, int B);
int launch_conv_wgrad_bf16(int layer, int width, int B, const float* in, const float* dout, float* dw, float* dbias, float* ws, hipStream_t st);
int64_t wgrad_split_ws_floats(int layer, int width, int B);        // fp32-emulation modes: exact 3-way operand splits on the bf16 MFMA
int launch_conv_wgrad_split(int layer, int width, int products, int B, const float* in, const float* dout, float* dw, float* dbias,
                            float* ws, hipStream_t st);
int launch_splitk_bias_relu(const float* slab, const float* bias, float* out, int64_t slice, int KS, int C, hipStream_t st, bool out_bf16 = false);
// conv_wgrad.hip
int64_t wgrad_ws_floats(int layer, int width, int B);
int launch_conv_wgrad(int layer, int width, int B, const float* in, const float* dout, float* dw,
                      float* dbias, float* ws, hipStream_t st);
int launch_reduce_slabs(const float* slab, float* dst, int64_t n, int S, int64_t stride, hipStream_t st,
                        float* mid = nullptr, bool out_bf16 = false);
int launch_colsum(const float* src, int64_t rows, int C, float* dst, float* ws, hipStream_t st);
int64_t colsum_ws_floats(int64_t rows, int C);
// Stage 1 of the column sum as block `blk` of `nblk` (colsum_stage1, and the column-sum job of fc.hip's fc_bwd launch):
// part[blk][c] = sum of this block's rows.  thread -> (channel c = tid % C, row lane rl = tid / C); requires C <= 256 and
// 256 % C == 0; red: 256 floats of LDS.  launch_colsum runs min(CS_BLOCKS, rows) blocks.
static constexpr int CS_BLOCKS = 128;
__device__ __forceinline__ void colsum_stage1_block(const float* __restrict__ src, int64_t rows, int C, float* __restrict__ part,
                                                    int blk, int nblk, float* red) {
    const int c = threadIdx.x % C, rl = threadIdx.x / C, RL = 256 / C;
    const int64_t per = (rows + nblk - 1) / nblk;
    const int64_t r0 = blk * per;
    int64_t r1 = r0 + per; if (r1 > rows) r1 = rows;
    float acc = 0.f;
    for (int64_t r = r0 + rl; r < r1; r += RL) acc += src[r * C + c];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (rl == 0) {
        for (int k = 1; k < RL; ++k) acc += red[k * C + c];
        part[(size_t)blk * C + c] = acc;
    }
}
// reduce.hip
int64_t col_reduce_ws_floats(int W);
int launch_col_reduce_partial(const float* in, int R, int W, int64_t stride, float* ws, hipStream_t st,
                              const float** rows_out, int* R_out, int64_t* stride_out);
int launch_col_reduce(const float* in, int R, int W, int64_t stride, float* out, float* ws, hipStream_t st, int skip_col0 = -1);
// conv_thin.hip (E1 / D4)
int launch_e1_fwd(int width, int B, const float* x, const float* w, const float* bias, float* y,
                  float* bnpart, hipStream_t st, bool bf16 = false, int pass = 0, const float* coef = nullptr, float* a1 = nullptr,
                  float* xp = nullptr);
                  // bf16 mode: pass 1 = BatchNorm partials only (+ writes the packed bf16 frame xp, B*width*width*8 bytes of workspace),
                  // pass 2 = fused BatchNorm/pool/ReLU -> a1 (needs coef; stages its strips from xp); y is written
                  // by pass 2 only if a channel has |gamma| < 1e-2 (the backward's statistics then read it)
int launch_e1_wgrad(int width, int B, const float* x, const float* dy, float* dw, float* dbias, float* ws,
                    hipStream_t st, bool bf16 = false, const float* const* fuse = nullptr,    // fuse: {y0, a0, d_a0, coef0, bcoef0, w1, b1}, dy unused; bf16 needs it
                    const float* xp = nullptr);                                               // bf16 mode: the packed frame of launch_e1_fwd's pass 1, or null
                    // (bf16 mode recomputes y0 from x, w1, b1 and never reads fuse[0])
const float* bn_bwd_bcoef(int layer, int width, int B, const float* ws);                       // where launch_bn_pool_act_bwd left (k1, k2)
int64_t e1_wgrad_ws_floats(int width, int B);
int launch_d4_fwd(int width, int B, const float* in, const float* w, const float* bias, float* recon,
                  hipStream_t st, bool bf16io = false);
int64_t d4_bwd_ws_floats(int width, int B);
int launch_d4_bwd(int width, int B, const float* o3, const float* d_recon, const float* recon,
                  const float* w, float* dout, float* d_o3, float* dw, float* db, float* ws,
                  hipStream_t st, bool bf16io = false);
// conv_up.hip (phase-collapsed Upsample->Conv blocks D1..D3, layers 5..7)
int64_t conv_up_wc_floats(int layer);
int launch_collapse_w(int layer, const float* w, float* wc, hipStream_t st);
int launch_collapse_w3(const float* const w[3], float* const wc[3], hipStream_t st);     // D1..D3 in one launch
int64_t conv_up_ws_floats(int layer, int width, int B);
int launch_conv_up_fwd(int layer, int width, int B, const float* in, const float* wc, const float* bias,
                       float* out, float* ws, hipStream_t st);
int launch_conv_up_dgrad(int layer, int width, int B, const float* dout, const float* wc, const float* aux,
                         float* din, float* ws, hipStream_t st);
int64_t conv_up_wgrad_ws_floats(int layer, int width, int B);
int launch_conv_up_wgrad(int layer, int width, int B, const float* in, const float* dout, float* dw,
                         float* dbias, float* ws, hipStream_t st, bool bf16 = false);
int launch_up_wgrad_bf16_main(int layer, int width, int B, const float* in, const float* dout, float* slab, int Smax, int* S_out, hipStream_t st,
                              int* plan = nullptr);      // plan != null: no launch, plan = (tiles, splits, tiles per split)
// (tiles, splits, tiles per split) of the bf16 weight-gradient kernels at a batch, from the launchers' own arithmetic (no launch; layers 5..7 ask the device's CU count)
int conv_wgrad_bf16_plan(int layer, int width, int B, int plan[3]);       // layers 1..4
int conv_up_wgrad_bf16_plan(int layer, int width, int B, int plan[3]);    // layers 5..7
// the same of the fp32 kernels: layers 1..4 (conv_wgrad.hip), 5..7 on a device of `cus` compute units (conv_up.hip), 0 and 8 (conv_thin.hip).  No device access.
int conv_wgrad_plan_f32(int layer, int width, int B, int plan[3]);
int conv_up_wgrad_plan_f32(int layer, int width, int B, int cus, int plan[3]);
int thin_wgrad_plan_f32(int layer, int width, int B, int plan[3]);
int e1_wgrad_plan_bf16(int width, int B, int plan[3]);                                        // E1's bf16 weight-gradient launch (asks the device's compute-unit count)
// bn.hip
int bn_num_tiles(int layer, int width, int B);
int launch_bn_fwd_finalize(int layer, int width, int B, const float* bnpart, const float* gamma,
                           const float* beta, float* run_mean, float* run_var, float* coef,
                           float* ws, int train, hipStream_t st, int tilesPerPartial = 1);
// cross-rank BatchNorm statistics (api.hip's staged entry points): this rank's fp64 (S, Q, M) record of the layer
// (+ its image count) ...
int launch_bn_fwd_record(int layer, int width, int B, const float* bnpart, float* ws, hipStream_t st, int tilesPerPartial,
                         double* rec, double* count);
// ... and coef + running statistics from the record summed over the ranks (count = the summed image count)
int launch_bn_fwd_finish(int layer, int width, const double* rec, const double* count, const float* gamma, const float* beta,
                         float* run_mean, float* run_var, float* coef, hipStream_t st);
int64_t bn_fwd_ws_floats(int layer, int width);
int launch_bn_pool_act_fwd(int layer, int width, int B, const float* y, const float* coef, float* a,
                           hipStream_t st, bool bf16io = false);
int64_t bn_bwd_ws_floats(int layer, int width, int B);
int launch_bn_pool_act_bwd(int layer, int width, int B, const float* y, const float* a,
                           const float* da, const float* coef, const float* gamma, float* dy,
                           float* dgamma, float* dbeta, float* dbias, float* ws, hipStream_t st, bool bf16io = false,
                           int stage = 0, double* rec = nullptr, const double* count = nullptr);     // stage 1 / 2: cross-rank split (bn.hip)
// fc.hip
// Grids of the latent launches at a batch: host arithmetic only; the launchers and cvae_op_latent_plan both read it.
// A merged launch runs its jobs over consecutive blockIdx.x ranges in the order of the fields.
struct LatentPlan {
    int fc_fwd_gemm;                            // launch_fc_fwd: latent_gemm blocks, cdiv(B, 128) * 32 K-slices
    int di_imgs, di_blocks;                     // launch_decin_fwd: images per workgroup, (K / 1024) * cdiv(B, di_imgs) blocks
    int db_bgemm, db_gemm;                      // launch_decin_bwd: dWd | dbd (K / 32), then the d_zcat slabs (cdiv(B, 128) * 32)
    int df_imgs, fb_bgemm, fb_dflat, fb_colsum; // launch_fc_bwd: images per dflat workgroup; dWfc (K / 32), dflat ((K / 256) *
                                                // cdiv(B, df_imgs)), dbfc stage 1 (min(B, CS_BLOCKS))
    int fb_split;                               // 1: dflat runs in a launch of its own behind dWfc | dbfc stage 1 (K / 32 > num_cus)
};
LatentPlan latent_plan(int width, int B, int num_cus);
int64_t fc_ws_floats(int width, int B);
int launch_fc_fwd(int width, int B, const float* flat, const float* wfc, const float* bfc,
                  const float* eps, const float* pred, float* mu, float* logvar, float* zcat,
                  float* ws, hipStream_t st, bool bf16io = false);
int launch_decin_fwd(int width, int B, const float* zcat, const float* wd, const float* bd, float* h,
                     hipStream_t st, bool bf16io = false);
int launch_decin_bwd(int width, int B, const float* zcat, const float* dh, const float* wd, float* dwd,
                     float* dbd, float* dzcat, float* ws, hipStream_t st, bool bf16io = false);
int launch_fc_bwd(int width, int B, const float* flat, const float* wfc, const float* dzcat,
                  const float* eps, const float* logvar, const float* dmu_loss,
                  const float* dlv_loss, float* dwfc, float* dbfc, float* dflat, float* ws,
                  hipStream_t st, bool bf16io = false);
// the objective of cvae_loss_obj (include/cvae.h), validated by the entry point: weights of the MS-SSIM, pixel (MSE) and KLD
// terms; used != 0: MS-SSIM gradient over the terms the product uses only.  The reference objective is {1, 0, 0.001f, 0}.
struct LossObjective { float w_ms, w_mse, kw; int used; };
// objective.hip: the pixel pass.  F non-null (mixed objective): d_x = coef-weighted MS-SSIM chain + the pixel gradient, and
// the merging workgroup adds w_mse * [13] to the scalars the finalize wrote.  F null (pure MSE): no chain, and the pass
// also does the KLD (mu, logvar -> d_mu, d_logvar, scalars[2]) and writes every scalar.  slab: MSSSIM_SLAB_DOUBLES
// doubles, *ticket 0 at launch.  dx null: values only.
constexpr int MSSSIM_SLAB_DOUBLES = 32 * 11;
int launch_objective_pixels(int width, int B, const float* recon, const float* x, const float* const* F, const float* coef,
                            float* dx, const float* mu, const float* logvar, float* d_mu, float* d_logvar,
                            LossObjective obj, double* slab, unsigned* ticket, float* scalars, hipStream_t st);
// msssim.hip
int64_t msssim_ws_floats(int width, int B);
int launch_msssim(int width, int B, const float* img1, const float* img2, const float* mu,
                  const float* logvar, float* ws, float* scalars, float* d_img1, float* d_mu,
                  float* d_logvar, hipStream_t st,
                  int stage = 0, double* rec = nullptr, const double* images = nullptr,       // stage 1 / 2: cross-rank split
                  const LossObjective* obj = nullptr);                                        // null: the reference objective (stage 0 only otherwise)
void msssim_score_slots(int width, int B, int64_t part[5], int64_t* scratch);      // score.hip: partial pairs and a free region of a values-only pyramid
int launch_msssim_finish_rec(int width, const double* rec, const double* images, float* scalars, float* coef, hipStream_t st);
// score.hip: per-image scores and the pooled record (layout: include/cvae.h)
int64_t score_state_bytes();
int launch_score_init(void* state, hipStream_t st);
int launch_score(int width, int B, const float* x, const float* mu, const float* logvar, const float* recon, float* ms,
                 float* per_image, void* state, hipStream_t st);
int launch_score_finish(int width, void* state, float* scalars, hipStream_t st);
// latent_stats.hip: the pooled latent record (layout: include/cvae.h); plan = (rows per chunk, chunks, workgroups), -1 for a bad batch
int64_t latent_stats_state_bytes();
int latent_stats_plan(int B, int num_cus, int plan[3]);
int64_t latent_stats_scratch_bytes(int B);
int launch_latent_stats(int B, const float* mu, const float* logvar, const float* pred, void* state, float* kl_rows, void* scratch,
                        hipStream_t st);
int launch_recon_response(int width, int64_t items, int K, const float* base, const float* var, float* out, hipStream_t st);
// critic.hip, critic_train.hip: float offsets into the flat critic parameter block (reference state_dict order)
namespace critic_layout {
constexpr int CW1 = 0, CB1 = 216, CW2 = 224, CB2 = 800, CW3 = 808, CB3 = 1384, CW4 = 1392, CB4 = 2544,
              CW5 = 2560, CB5 = 10752, CF1W = 10784, CF1B = 11808, CF2W = 11840, CF2B = 11872;
constexpr int CRITIC_PARAMS = 11873;
}
int critic_param_count();
int launch_critic_fwd(int width, int B, const float* x, const float* critic_params, float* pred, hipStream_t st);
int launch_preprocess_u8(int width, int B, const uint8_t* u8, float* x, hipStream_t st);
// critic_train.hip
int critic_train_floats();
int64_t critic_grad_scratch_bytes(int B);
int launch_critic_grad(int width, int B, const float* x, const float* target, const uint8_t* keep, float scale, int loss_kind,
                       const float* critic_params, float* grads, float* pred, float* loss_scalars, uint8_t* decisions,
                       void* scratch, hipStream_t st);
// critic_score.hip: per-frame scores against the targets and the pooled record (layout: include/cvae.h)
int64_t critic_score_state_bytes();
int64_t critic_score_scratch_bytes(int B);
int launch_critic_score_init(void* state, hipStream_t st);
int launch_critic_score(int B, const uint8_t* frames, const float* targets, int64_t n, const int64_t* idx, const float* critic_params,
                        float* rows, void* state, hipStream_t st);
// critic_saliency.hip: embeddings, the logit's input gradient (plain / integrated) and occlusion drops (include/cvae.h)
int launch_critic_collect(int B, const float* x, const float* critic_params, float* pred, float* const e[5], hipStream_t st);
int launch_critic_saliency(int B, const float* x, const float* critic_params, int steps, float* pred, float* grad, float* map,
                           float* max_values, uint8_t* decisions, hipStream_t st);
int launch_critic_occlusion(int B, const float* x, const float* critic_params, int patch, float fill_r, float fill_g, float fill_b,
                            float* pred, float* drop, float* map, float* max_values, hipStream_t st);
// dataset.hip
int launch_curate_select(int n_traj, const int64_t* off, int64_t n_frames, const float* preds, int collect,
                         int64_t total_images, int64_t* running, int64_t* counts, int64_t* first, int64_t* span,
                         int64_t* sel, hipStream_t st);
int launch_gather_frames_u8(int width, const uint8_t* src, const float* src_pred, int64_t n_src, const int64_t* sel,
                            int64_t max_count, const int64_t* span, uint8_t* dst, float* dst_pred, int64_t capacity,
                            hipStream_t st);
int launch_preprocess_u8_gather(int width, int B, const uint8_t* frames, const float* preds, int64_t n, const int64_t* idx,
                                float* x, float* pred, hipStream_t st);
int launch_curate_select_recon(int n_traj, const int64_t* off, int64_t n_frames, const float* preds, int collect,
                               int64_t total_images, int64_t* running, int64_t* counts, int64_t* first, int64_t* sel_first,
                               int64_t* span, int64_t* ent_frame, int32_t* ent_kind, int64_t* ent_sel, int64_t* sel,
                               hipStream_t st);
int launch_recon_zcat(int n_entries, const int64_t* ent_sel, const int32_t* ent_kind, const float* mu, const float* sel_pred,
                      int64_t n_sel, float* zcat, hipStream_t st);
int launch_inject_zcat(int n_images, int n_rewards, const float* mu, const float* rewards, float* zcat, hipStream_t st);
int launch_gather_f32(int width, int B, const float* frames, const float* preds, int64_t n, const int64_t* idx, float* x,
                      float* pred, hipStream_t st);
int launch_preprocess_u8_gather_aug(int width, int B, const uint8_t* frames, const float* preds, int64_t n, const int64_t* idx,
                                    const struct cvae_augment& aug, float* x, float* pred, int32_t* applied, hipStream_t st);
int launch_gather_f32_aug(int width, int B, const float* frames, const float* preds, int64_t n, const int64_t* idx,
                          const struct cvae_augment& aug, float* x, float* pred, int32_t* applied, hipStream_t st);
int launch_diff_grey(int width, int B, const float* a, const float* b, float* diff, hipStream_t st);
// segment.hip
int64_t crf_scratch_bytes(int width, int B);
int launch_dense_crf(int width, int B, const uint8_t* frames, const float* prob1, const struct cvae_crf_params& p,
                     uint8_t* labels, float* q1, void* scratch, hipStream_t st);
int launch_diff_normalize(int width, int B, const float* diff, double mean_max, double factor, int thr, const uint8_t* gt,
                          uint8_t* u8, uint8_t* mask, int64_t* counts, int64_t* hist, hipStream_t st);
int launch_mask_counts(int width, int B, const uint8_t* mask, const uint8_t* gt, int64_t* counts, hipStream_t st);
// components.hip: objects from masks; arguments already checked by the caller
int launch_mask_objects(int width, int B, const uint8_t* mask, const uint8_t* values, int conn8, int fill, int min_area, int keep, int M,
                        uint8_t* mask_out, uint16_t* labels, int32_t* info, int32_t* table, hipStream_t st);
int launch_object_overlap(int width, int B, const uint16_t* la, const uint16_t* lb, int M, int32_t* inter, hipStream_t st);
// crf_grid.hip
int crf_grid_group();
int64_t crf_grid_scratch_bytes(int width, int B, int K);
int launch_crf_grid(int width, int B, const uint8_t* frames, const float* prob1, const uint8_t* u8, const uint8_t* gt, float alpha,
                    float beta, float gamma, const struct cvae_crf_variant* var, int K, const int32_t* snaps, int n_snaps,
                    int64_t* counts, uint8_t* labels, float* q1, void* scratch, hipStream_t st);
// render.hip
int launch_compose_frames(int width, int B, int n_panels, const struct cvae_panel* panels, int ih, int clamp, const uint8_t* overlay,
                          const uint8_t* atlas, int n_labels, int lh, int lw, const int32_t* label_idx, int lx, int ly,
                          uint8_t* out, hipStream_t st);
// adam.hip
int launch_grads_bf16(const float* src_f32, void* bf16_buf, float* dst_f32, int64_t n, hipStream_t st);   // src set: pack; else unpack
int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, int step, float lr, float b1,
                float b2, float eps, float gscale, hipStream_t st);
// guarded step: the layout of `state` is cvae_guard_record + partials (include/cvae.h)
int64_t guard_state_bytes();
int launch_guard_init(void* state, int64_t applied, int64_t skipped, hipStream_t st);
int launch_grad_stats(const float* g, int64_t n, float gscale, float max_norm, int skip_nonfinite, float lr, float b1, float b2,
                      void* state, hipStream_t st);
int launch_adam_guarded(float* p, const float* g, float* m, float* v, int64_t n, float eps, const void* state, hipStream_t st);
// the optimizer options (cvae_opt_args, include/cvae.h): arguments already checked by the caller
struct cvae_opt_args;
int launch_adam_opt(float* p, const float* g, float* m, float* v, int64_t n, int step, float lr, float b1, float b2, float eps,
                    float gscale, const cvae_opt_args* opt, float* ema, const float* aux, float* aux_ema, int32_t n_aux, hipStream_t st);
int launch_adam_guarded_opt(float* p, const float* g, float* m, float* v, int64_t n, float eps, const void* state,
                            const cvae_opt_args* opt, float* ema, const float* aux, float* aux_ema, int32_t n_aux, hipStream_t st);
// the training trace (trace.hip): arguments already checked by the caller, but for the range table (checked by the launcher,
// which returns CVAE_EINVAL = -1 with the error set)
struct cvae_tensor_stat;
int launch_trace_push(void* ring, int64_t capacity, int64_t step, float lr, const float* scalars, int n_scalars,
                      const void* guard_state, hipStream_t st);
int launch_tensor_stats(const float* p, const float* g, const float* m, const float* v, int64_t n, int32_t n_tensors,
                        const int64_t* begin, const int64_t* end, int64_t step, float lr, float b1, float b2, float eps, float gscale,
                        const void* guard_state, cvae_tensor_stat* out, void* scratch, hipStream_t st);
int64_t tensor_stats_scratch_bytes(int32_t n_tensors, const int64_t* begin, const int64_t* end);
int tensor_stats_plan(int32_t n_tensors, const int64_t* begin, const int64_t* end, int32_t* chunk, int32_t* items, int32_t* grid);
int launch_zero(float* p, int64_t n, hipStream_t st);
struct PadGaps { int64_t off[32]; int len[32]; int n; };
int launch_zero_gaps(float* grads, const PadGaps& gaps, hipStream_t st);
struct Scale3 { const float* g; const float* src[3]; float* dst[3]; int64_t n[3]; };
int launch_scale3(const Scale3& a, hipStream_t st);
