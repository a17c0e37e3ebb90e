// components.hip — objects from masks (cvae_mask_objects, cvae_object_overlap; include/cvae.h).
//
// One workgroup per frame, one launch for any batch.  A thread owns OBJ_PX = 16 consecutive pixels of one row (256 threads at
// W = 64, 1024 at W = 128): the frame's mask is read from memory once, 16 bytes per thread, and everything up to the output
// writes lives in LDS:
//   lab   W*W uint16   the label of a pixel: its component's representative as index + 1, 0xFFFF for a pixel outside the set,
//                      and 0 for "connected to the frame border" while the holes are filled
//   area  W*W/2 uint16 per component (by raster rank of its root): the area, later the final label
//   table M*8 int32    the object rows
// 32 KB + 16 KB + 2 KB at W = 128.
//
// Labelling is label equivalence (Hawick et al. 2010; Kalentev et al. 2011) on uint16 labels.  A pass is a SCAN — a pixel whose
// set neighbours hold a smaller label than its own writes that minimum to its own label's entry, the root, with an LDS atomic
// minimum (a compare-and-swap on the 32-bit word that holds the 16-bit entry) — and a FLATTEN — every pixel follows its chain
// to the root.  Labels only ever decrease and a label always names a pixel of the same component (or the border, 0), so
// chains point downward and end; a scan that changes nothing ends the loop, and then every component holds one label, its
// minimum linear index.  A budget shared by both labellings caps the scans of a frame at W*W + 1 whatever the input.
//
// Holes: the same routine on the clear pixels under the complementary connectivity, with every clear border pixel starting at
// label 0; clear pixels that do not end at 0 become set.  Roots are ranked in raster order by a prefix sum over root flags; the
// area filter, the k-th largest area (a binary search over area values, ties to the earlier rank by a second prefix sum) and the
// final labels (a third prefix sum over the survivors) work on the per-rank array.  All accumulations are integer atomics on
// LDS, which are order-free, after a per-thread aggregation of runs of equal labels: a frame's result depends on the frame alone.
#include "common.h"
#include "../../include/cvae.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
static constexpr int OBJ_PX = 16;               // pixels per thread, consecutive in one row
static constexpr unsigned OBJ_OUT = 0xFFFFu;     // a pixel outside the set being labelled
static constexpr unsigned OBJ_ROOT = 0x8000u;    // flag of a ranked root entry: OBJ_ROOT | raster rank (rank < W*W/2 <= 8192)

struct ObjArgs {
    const uint8_t* mask; const uint8_t* values;  // (B,W,W); values or null
    uint8_t* mask_out; uint16_t* labels;         // (B,W,W) or null
    int32_t* info; int32_t* table;               // (B,4); (B,M,8) or null
    int conn8, fill, min_area, keep, M;
};

// the 16-bit entry `idx` of lab <- min(entry, v), atomically on the 32-bit word that holds it
__device__ __forceinline__ void obj_min16(uint16_t* lab, int idx, unsigned v) {
    unsigned* w = reinterpret_cast<unsigned*>(lab) + (idx >> 1);
    const int sh = (idx & 1) * 16;
    unsigned old = *reinterpret_cast<volatile unsigned*>(w);
    while (((old >> sh) & 0xFFFFu) > v) {
        const unsigned want = (old & ~(0xFFFFu << sh)) | (v << sh);
        const unsigned seen = atomicCAS(w, old, want);
        if (seen == old) break;
        old = seen;
    }
}

// exclusive prefix sum of v over the workgroup's threads in thread order; total = the sum.  s_w: NT / 64 ints.
template <int NT>
__device__ __forceinline__ int obj_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) { const int t = s_w[k]; tot += t; if (k < wv) base += t; }
    __syncthreads();                             // s_w is free for the next call
    total = tot;
    return base + inc - v;
}

template <int W>
__device__ __forceinline__ unsigned obj_nb_min(const uint16_t* lab, int y, int x, bool c8) {
    const int i = y * W + x;
    unsigned m = OBJ_OUT;
    const bool l = x > 0, r = x < W - 1;
    if (l) m = min(m, (unsigned)lab[i - 1]);
    if (r) m = min(m, (unsigned)lab[i + 1]);
    if (y > 0) {
        m = min(m, (unsigned)lab[i - W]);
        if (c8 && l) m = min(m, (unsigned)lab[i - W - 1]);
        if (c8 && r) m = min(m, (unsigned)lab[i - W + 1]);
    }
    if (y < W - 1) {
        m = min(m, (unsigned)lab[i + W]);
        if (c8 && l) m = min(m, (unsigned)lab[i + W - 1]);
        if (c8 && r) m = min(m, (unsigned)lab[i + W + 1]);
    }
    return m;
}

// Labels to the fixpoint; returns the scans used.  `budget` (the frame's remaining scans) is the same in every thread.
template <int W>
__device__ int obj_label(uint16_t* lab, int* s_changed, bool c8, int budget) {
    const int p0 = threadIdx.x * OBJ_PX, y = p0 / W, x0 = p0 % W;
    int passes = 0;
    while (passes < budget) {
        if (threadIdx.x == 0) *s_changed = 0;
        __syncthreads();
        bool ch = false;
        for (int j = 0; j < OBJ_PX; ++j) {
            const unsigned l = lab[p0 + j];
            if (l == OBJ_OUT || l == 0) continue;
            const unsigned m = obj_nb_min<W>(lab, y, x0 + j, c8);
            if (m < l) { obj_min16(lab, (int)l - 1, m); ch = true; }
        }
        if (ch) *s_changed = 1;
        ++passes;
        __syncthreads();
        const int any = *s_changed;
        if (!any) break;
        for (int j = 0; j < OBJ_PX; ++j) {
            unsigned l = lab[p0 + j];
            if (l == OBJ_OUT || l == 0) continue;
            for (int hop = 0; hop < W * W; ++hop) {          // chains point downward: at most W*W hops
                const unsigned up = lab[l - 1];
                if (up == l) break;
                l = up;
                if (l == 0) break;
            }
            lab[p0 + j] = (uint16_t)l;
        }
        __syncthreads();
    }
    return passes;
}

// the rank of the component of a labelled pixel, after the roots were ranked (NC, a power of two, bounds it whatever lab holds)
template <int NC>
__device__ __forceinline__ int obj_rank(const uint16_t* lab, unsigned l) {
    const unsigned e = (l & OBJ_ROOT) ? l : (unsigned)lab[l - 1];
    return (int)(e & (OBJ_ROOT - 1) & (unsigned)(NC - 1));
}

template <int W>
__global__ __launch_bounds__(W * W / OBJ_PX) void mask_objects_kernel(ObjArgs a) {
    constexpr int N = W * W, NT = N / OBJ_PX, NC = N / 2, CP = NC / NT;      // CP = 8 ranks per thread
    static_assert(OBJ_PX == 16 && CP == 8 && W % OBJ_PX == 0 && (NC & (NC - 1)) == 0, "thread ownership");
    __shared__ __attribute__((aligned(16))) uint16_t lab[N];
    __shared__ __attribute__((aligned(16))) uint16_t area[NC];
    __shared__ int table[CVAE_OBJECTS_MAX * 8];
    __shared__ int s_w[NT / 64];
    __shared__ int s_changed;
    const int tid = threadIdx.x, p0 = tid * OBJ_PX, y = p0 / W, x0 = p0 % W, M = a.M;
    const size_t f0 = (size_t)blockIdx.x * N;

    // ---- the one read of the mask ----
    const u32x4 raw = *reinterpret_cast<const u32x4*>(a.mask + f0 + p0);
    unsigned setbits = 0;
#pragma unroll
    for (int j = 0; j < OBJ_PX; ++j) if ((raw[j >> 2] >> (8 * (j & 3))) & 0xFFu) setbits |= 1u << j;
    for (int k = tid; k < NC / 2; k += NT) reinterpret_cast<unsigned*>(area)[k] = 0u;
    for (int k = tid; k < CVAE_OBJECTS_MAX * 8; k += NT) table[k] = 0;

    int budget = N + 1, passes = 0, filled = 0;
    // ---- 1. holes: label the clear pixels under the complementary connectivity, the border at label 0 ----
    if (a.fill) {
        const bool edge_row = y == 0 || y == W - 1;
        for (int j = 0; j < OBJ_PX; ++j) {
            const int x = x0 + j;
            const bool border = edge_row || x == 0 || x == W - 1;
            lab[p0 + j] = (uint16_t)(((setbits >> j) & 1u) ? OBJ_OUT : border ? 0u : (unsigned)(p0 + j + 1));
        }
        __syncthreads();
        passes = obj_label<W>(lab, &s_changed, !a.conn8, budget);
        budget -= passes;
        int mine = 0;
        for (int j = 0; j < OBJ_PX; ++j) {
            if (!((setbits >> j) & 1u) && lab[p0 + j] != 0) { setbits |= 1u << j; ++mine; }
        }
        obj_scan<NT>(mine, s_w, filled);         // its barriers also order the reads above before the writes below
    }
    // ---- 2. label the set pixels ----
    for (int j = 0; j < OBJ_PX; ++j) lab[p0 + j] = (uint16_t)(((setbits >> j) & 1u) ? (unsigned)(p0 + j + 1) : OBJ_OUT);
    __syncthreads();
    if (budget > 0) passes += obj_label<W>(lab, &s_changed, a.conn8 != 0, budget);

    // ---- roots in raster order: entry <- OBJ_ROOT | rank ----
    int nroot = 0, ncomp;
    for (int j = 0; j < OBJ_PX; ++j) nroot += lab[p0 + j] == (unsigned)(p0 + j + 1);
    int rk = obj_scan<NT>(nroot, s_w, ncomp);
    for (int j = 0; j < OBJ_PX; ++j) if (lab[p0 + j] == (unsigned)(p0 + j + 1)) lab[p0 + j] = (uint16_t)(OBJ_ROOT | (unsigned)rk++);
    __syncthreads();

    // ---- areas by rank: runs of equal rank, one packed 16-bit atomic add per run (an area is at most W*W = 2^14) ----
    {
        int cur = -1, cnt = 0;
        for (int j = 0; j <= OBJ_PX; ++j) {
            int r = -1;
            if (j < OBJ_PX) { const unsigned l = lab[p0 + j]; if (l != OBJ_OUT) r = obj_rank<NC>(lab, l); }
            if (r != cur) {
                if (cur >= 0) atomicAdd(reinterpret_cast<unsigned*>(area) + (cur >> 1), (unsigned)cnt << (16 * (cur & 1)));
                cur = r; cnt = 0;
            }
            ++cnt;
        }
    }
    __syncthreads();

    // ---- 3. / 4. the filters on this thread's CP ranks ----
    int ar[CP];
    unsigned keepbits = 0;
    int nsurv_mine = 0, nsurv;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        const int rank = tid * CP + c;
        ar[c] = rank < ncomp ? (int)area[rank] : 0;
        if (rank < ncomp && ar[c] >= a.min_area) { keepbits |= 1u << c; ++nsurv_mine; }
    }
    obj_scan<NT>(nsurv_mine, s_w, nsurv);
    if (a.keep > 0 && nsurv > a.keep) {
        // T = the keep-th largest surviving area: the largest T with at least `keep` survivors of area >= T
        int lo = 1, hi = N;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            int c_mine = 0, c_all;
#pragma unroll
            for (int c = 0; c < CP; ++c) c_mine += ((keepbits >> c) & 1u) && ar[c] >= mid;
            obj_scan<NT>(c_mine, s_w, c_all);
            if (c_all >= a.keep) lo = mid; else hi = mid - 1;
        }
        const int T = lo;
        int gt_mine = 0, eq_mine = 0, gt_all, eq_all;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            const bool s = (keepbits >> c) & 1u;
            gt_mine += s && ar[c] > T; eq_mine += s && ar[c] == T;
        }
        obj_scan<NT>(gt_mine, s_w, gt_all);
        int eq_before = obj_scan<NT>(eq_mine, s_w, eq_all);
        const int need = a.keep - gt_all;        // ties at area T go to the earlier rank
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            if (!((keepbits >> c) & 1u)) continue;
            if (ar[c] < T) keepbits &= ~(1u << c);
            else if (ar[c] == T) { if (eq_before >= need) keepbits &= ~(1u << c); ++eq_before; }
        }
    }
    // ---- 5. final labels 1..kept in raster order of the first pixel; the table rows of labels <= M ----
    int kept;
    int nl = obj_scan<NT>(__popc(keepbits), s_w, kept);
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        const int rank = tid * CP + c;
        unsigned fin = 0;
        if ((keepbits >> c) & 1u) {
            fin = (unsigned)++nl;
            if (nl <= M) { int* row = table + (nl - 1) * 8; row[0] = ar[c]; row[1] = W; row[2] = W; }
        }
        area[rank] = (uint16_t)fin;              // this thread's own four words
    }
    __syncthreads();

    // ---- outputs; box, sums by runs of equal final label ----
    u32x4 vraw = {0u, 0u, 0u, 0u};
    if (a.values) vraw = *reinterpret_cast<const u32x4*>(a.values + f0 + p0);
    u32x4 mo = {0u, 0u, 0u, 0u};
    u32x4 lo4[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    {
        int cur = 0, xa = 0, sx = 0, sv = 0, cnt = 0;
        for (int j = 0; j <= OBJ_PX; ++j) {
            int fin = 0;
            if (j < OBJ_PX) {
                const unsigned l = lab[p0 + j];
                if (l != OBJ_OUT) fin = (int)area[obj_rank<NC>(lab, l)];
                if (fin) { mo[j >> 2] |= 1u << (8 * (j & 3)); lo4[j >> 3][(j >> 1) & 3] |= (unsigned)fin << (16 * (j & 1)); }
            }
            if (fin != cur) {
                if (cur > 0 && cur <= M) {
                    int* row = table + (cur - 1) * 8;
                    atomicMin(row + 1, xa); atomicMin(row + 2, y);
                    atomicMax(row + 3, x0 + j - 1); atomicMax(row + 4, y);
                    atomicAdd(row + 5, sx); atomicAdd(row + 6, cnt * y); atomicAdd(row + 7, sv);
                }
                cur = fin; xa = x0 + j; sx = 0; sv = 0; cnt = 0;
            }
            if (j < OBJ_PX) { sx += x0 + j; sv += (int)((vraw[j >> 2] >> (8 * (j & 3))) & 0xFFu); ++cnt; }
        }
    }
    if (a.mask_out) *reinterpret_cast<u32x4*>(a.mask_out + f0 + p0) = mo;
    if (a.labels) {
        u32x4* dst = reinterpret_cast<u32x4*>(a.labels + f0 + p0);
        dst[0] = lo4[0]; dst[1] = lo4[1];
    }
    __syncthreads();
    if (a.table) {
        int32_t* t = a.table + (size_t)blockIdx.x * (size_t)(M * 8);
        for (int k = tid; k < M * 8; k += NT) t[k] = table[k];
    }
    if (tid == 0) {
        int32_t* o = a.info + (size_t)blockIdx.x * 4;
        o[0] = ncomp; o[1] = kept; o[2] = filled; o[3] = passes;
    }
}

int launch_mask_objects(int width, int B, const uint8_t* mask, const uint8_t* values, int conn8, int fill, int min_area, int keep, int M,
                        uint8_t* mask_out, uint16_t* labels, int32_t* info, int32_t* table, hipStream_t st) {
    ObjArgs a{mask, values, mask_out, labels, info, table, conn8, fill, min_area, keep, M};
    if (width == 64) hipLaunchKernelGGL(mask_objects_kernel<64>, dim3((unsigned)B), dim3(64 * 64 / OBJ_PX), 0, st, a);
    else hipLaunchKernelGGL(mask_objects_kernel<128>, dim3((unsigned)B), dim3(128 * 128 / OBJ_PX), 0, st, a);
    CVAE_CHECK_LAUNCH();
    return 0;
}

// ---- cvae_object_overlap: inter[i][j] = pixels with a == i + 1 and b == j + 1 (labels above M ignored) ----
// One workgroup per frame, the M x M matrix in LDS, runs of equal (a, b) aggregated per thread before the integer atomic.
template <int W>
__global__ __launch_bounds__(256) void object_overlap_kernel(const uint16_t* __restrict__ la, const uint16_t* __restrict__ lb,
                                                             int32_t* __restrict__ inter, int M) {
    constexpr int N = W * W;
    __shared__ int s[CVAE_OBJECTS_MAX * CVAE_OBJECTS_MAX];
    const int tid = threadIdx.x;
    const size_t f0 = (size_t)blockIdx.x * N;
    for (int k = tid; k < M * M; k += 256) s[k] = 0;
    __syncthreads();
    for (int q = tid; q < N / 8; q += 256) {                 // 8 labels of each plane per load
        const u32x4 va = *reinterpret_cast<const u32x4*>(la + f0 + (size_t)q * 8);
        const u32x4 vb = *reinterpret_cast<const u32x4*>(lb + f0 + (size_t)q * 8);
        int cur = -1, cnt = 0;
#pragma unroll
        for (int j = 0; j <= 8; ++j) {
            int cell = -1;
            if (j < 8) {
                const int x = (int)((va[j >> 1] >> (16 * (j & 1))) & 0xFFFFu), z = (int)((vb[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
                if (x >= 1 && x <= M && z >= 1 && z <= M) cell = (x - 1) * M + (z - 1);
            }
            if (cell != cur) {
                if (cur >= 0) atomicAdd(&s[cur], cnt);
                cur = cell; cnt = 0;
            }
            ++cnt;
        }
    }
    __syncthreads();
    int32_t* o = inter + (size_t)blockIdx.x * (size_t)(M * M);
    for (int k = tid; k < M * M; k += 256) o[k] = s[k];
}

int launch_object_overlap(int width, int B, const uint16_t* la, const uint16_t* lb, int M, int32_t* inter, hipStream_t st) {
    if (width == 64) hipLaunchKernelGGL(object_overlap_kernel<64>, dim3((unsigned)B), dim3(256), 0, st, la, lb, inter, M);
    else hipLaunchKernelGGL(object_overlap_kernel<128>, dim3((unsigned)B), dim3(256), 0, st, la, lb, inter, M);
    CVAE_CHECK_LAUNCH();
    return 0;
}
