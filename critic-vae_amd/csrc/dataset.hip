// dataset.hip — the training set of `-train` built on the device (load_minerl_data, vae_utility.py:393-461, non-recon
// branch) and the per-step batch gather out of it.
//
//   curate_select         critic values of a chunk of whole trajectories -> the frames the reference keeps, in its order:
//                         per trajectory at most `collect` frames in each of the bins mid [0.4, 0.6], high >= 0.7,
//                         low <= 0.25 (tested in that order, fp32), and the global cut `len(dset) >= total_images` before
//                         each trajectory against a running count held on the device across chunks.  Three launches:
//                         per-trajectory bin counts, one fixed-order scan over the trajectories (the cut), the scatter.
//   gather_frames_u8      the selected uint8 frames (and their critic values) into the dataset buffer at their slots.
//   preprocess_u8_gather  x[b] = frames[idx[b]] / 255 as CHW fp32 and pred[b] = preds[idx[b]]: one training batch.
//
// and the recon branch of the same walk (vae_utility.py:422-443: the dataset of the second VAE holds the first VAE's
// eval-mode reconstructions, two entries for a mid frame):
//
//   curate_select_recon   the same three kernels with entry weight 2 / 1 / 1 (mid / high / low) in the cut and in the slot
//                         positions (template parameter MIDW; MIDW = 1 is curate_select), plus per entry its frame and kind
//                         and per selected frame its chunk index, so that the encoder runs once per selected frame.
//   recon_zcat            zcat rows (mu of the entry's frame, its critic value or 0) for cvae_decode into the dataset slots.
//   gather_f32            x[b] = frames[idx[b]] (fp32 CHW, bit copy) and pred[b] = preds[idx[b]]: one training batch.
//   inject_zcat           zcat rows (mu of image b, reward r) of the batched -inject: one decoder call for all of them.
//
// and the augmented forms of the two batch gathers (cvae_augment, include/cvae.h: per sample a hashed flip, a shift with edge
// replication and, for uint8 frames, a brightness gain — inside the same single launch):
//
//   preprocess_u8_gather_aug, gather_f32_aug   source rows staged in LDS between replicated edge pads, one window per thread.
//
// Integer math only, no atomics: every result is deterministic.  Frame offsets are 64-bit (a 64x64 dataset passes
// 2^31 bytes at 174 763 frames).
#include "common.h"
#include "../../include/cvae.h"

namespace {

constexpr int TPB = 256;
constexpr int NWAVE = TPB / 64;

// 0 mid, 1 high, 2 low, -1 none: vae_utility.py:450-459, float32 comparisons (NaN falls in no bin)
__device__ __forceinline__ int bin_of(float p) {
    if (p >= 0.4f && p <= 0.6f) return 0;
    if (p >= 0.7f) return 1;
    if (p <= 0.25f) return 2;
    return -1;
}

__device__ __forceinline__ uint64_t lanes_below(int lane) { return lane == 0 ? 0ull : (~0ull >> (64 - lane)); }

// frames [lo, hi) of trajectory t, clamped to the chunk
__device__ __forceinline__ void traj_range(const int64_t* off, int t, int64_t n_frames, int64_t& lo, int64_t& hi) {
    lo = off[t]; hi = off[t + 1];
    lo = lo < 0 ? 0 : (lo > n_frames ? n_frames : lo);
    hi = hi < lo ? lo : (hi > n_frames ? n_frames : hi);
}

// one workgroup per trajectory: counts[t][k] = min(#frames of bin k, collect)
__global__ __launch_bounds__(TPB) void curate_count_kernel(const float* __restrict__ preds, const int64_t* __restrict__ off,
                                                           int64_t n_frames, int collect, int64_t* __restrict__ counts) {
    __shared__ int64_t part[NWAVE][3];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t lo, hi;
    traj_range(off, t, n_frames, lo, hi);
    int64_t c[3] = {0, 0, 0};
    for (int64_t i = lo + tid; i < hi; i += TPB) {
        const int k = bin_of(preds[i]);
        c[0] += k == 0; c[1] += k == 1; c[2] += k == 2;
    }
    for (int k = 0; k < 3; ++k) {
        int64_t v = c[k];
        for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
        if (lane == 0) part[wv][k] = v;
    }
    __syncthreads();
    if (tid < 3) {
        int64_t v = 0;
        for (int w = 0; w < NWAVE; ++w) v += part[w][tid];
        counts[(int64_t)t * 3 + tid] = v < collect ? v : collect;
    }
}

// exclusive scan of v over the workgroup's threads on top of `carry`; total = the workgroup's sum.  wsum is written here and
// read after the barrier inside: the caller puts a barrier before the next call on the same wsum.
__device__ __forceinline__ int64_t block_scan_excl(int64_t v, int64_t* wsum, int64_t carry, int64_t& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int64_t incl = v;                                            // inclusive scan within the wave
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t u = __shfl_up(incl, d, 64);
        if (lane >= d) incl += u;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int64_t before = carry + incl - v;
    total = 0;
    for (int w = 0; w < NWAVE; ++w) {
        if (w < wv) before += wsum[w];
        total += wsum[w];
    }
    return before;
}

// one workgroup, trajectories in order: trajectory t is visited iff running + (frames selected by the visited ones
// before it) < total_images — the running count only grows, so that is an exclusive prefix sum compared with the cut.
// first[t] = its first dataset slot (the reference's len(dset) before it) or -1; counts of unvisited ones become 0.
// MIDW = the dataset entries of a mid frame (2 in the recon branch: vae_utility.py:434-435); the recon form also scans the
// selected FRAMES of the chunk: ffirst[t] = frames selected in this chunk before trajectory t (or -1), span[2] = their total.
template <int MIDW>
__global__ __launch_bounds__(TPB) void curate_cut_kernel(int n_traj, int64_t total_images, int64_t* __restrict__ running,
                                                         int64_t* __restrict__ counts, int64_t* __restrict__ first,
                                                         int64_t* __restrict__ span, int64_t* __restrict__ ffirst) {
    __shared__ int64_t wsum[NWAVE];
    __shared__ int64_t fsum[NWAVE];                              // MIDW > 1 only: the same scan over frames
    const int tid = threadIdx.x;
    const int64_t r0 = *running;
    int64_t carry = r0, fcarry = 0;                              // identical in every thread
    for (int t0 = 0; t0 < n_traj; t0 += TPB) {
        const int t = t0 + tid;
        const int64_t s = t < n_traj ? MIDW * counts[(int64_t)t * 3] + counts[(int64_t)t * 3 + 1] + counts[(int64_t)t * 3 + 2] : 0;
        int64_t total;
        const int64_t before = block_scan_excl(s, wsum, carry, total);      // len(dset) before trajectory t
        carry += total;
        const bool visited = t < n_traj && before < total_images;
        if (t < n_traj) {
            if (visited) {
                first[t] = before;
            } else {
                first[t] = -1;
                counts[(int64_t)t * 3] = counts[(int64_t)t * 3 + 1] = counts[(int64_t)t * 3 + 2] = 0;
            }
        }
        if constexpr (MIDW > 1) {                                // visited trajectories are a prefix: unvisited ones add 0
            const int64_t sf = visited ? counts[(int64_t)t * 3] + counts[(int64_t)t * 3 + 1] + counts[(int64_t)t * 3 + 2] : 0;
            const int64_t fbefore = block_scan_excl(sf, fsum, fcarry, total);
            fcarry += total;
            if (t < n_traj) ffirst[t] = visited ? fbefore : -1;
        }
        __syncthreads();                                         // the next round rewrites wsum / fsum; tid 0 reads first / counts below
    }
    // the visited trajectories are a prefix: the new running count is the last visited one's first + its selection
    if (tid == 0) {
        int64_t r = r0;
        for (int t = n_traj - 1; t >= 0; --t)
            if (first[t] >= 0) { r = first[t] + MIDW * counts[(int64_t)t * 3] + counts[(int64_t)t * 3 + 1] + counts[(int64_t)t * 3 + 2]; break; }
        span[0] = r0; span[1] = r - r0;
        if constexpr (MIDW > 1) span[2] = fcarry;
        *running = r;
    }
}

// one workgroup per visited trajectory: frames in order, a frame is kept iff it has a bin and fewer than `collect`
// earlier frames of the trajectory fell in that bin; sel[first[t] - span[0] + rank] = its chunk frame index.
// MIDW = 2 (recon branch): a kept mid frame owns two consecutive entries (kind 0, then kind 1), a high frame one of kind 0, a
// low frame one of kind 1; per entry e (chunk-relative) sel[e] = the chunk frame index, kind[e], esel[e] = the frame's rank
// among the chunk's selected frames, and fsel[that rank] = the chunk frame index.
template <int MIDW>
__global__ __launch_bounds__(TPB) void curate_scatter_kernel(const float* __restrict__ preds, const int64_t* __restrict__ off,
                                                             int64_t n_frames, int collect, const int64_t* __restrict__ first,
                                                             const int64_t* __restrict__ span, int64_t* __restrict__ sel,
                                                             const int64_t* __restrict__ ffirst, int32_t* __restrict__ kind,
                                                             int64_t* __restrict__ esel, int64_t* __restrict__ fsel) {
    __shared__ int wcnt[NWAVE][5];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t f = first[t];
    if (f < 0) return;
    int64_t lo, hi;
    traj_range(off, t, n_frames, lo, hi);
    const int64_t base = f - span[0];
    int64_t carry[3] = {0, 0, 0}, taken = 0;                    // identical in every thread
    [[maybe_unused]] int64_t taken_mid = 0;                      // MIDW > 1: kept mid frames so far
    const uint64_t below = lanes_below(lane);
    for (int64_t b0 = lo; b0 < hi; b0 += TPB) {
        if (carry[0] >= collect && carry[1] >= collect && carry[2] >= collect) break;
        const int64_t i = b0 + tid;
        const int k = i < hi ? bin_of(preds[i]) : -1;
        int rank = 0;                                            // earlier frames of this block in bin k
        for (int q = 0; q < 3; ++q) {
            const uint64_t m = __ballot(k == q);
            if (k == q) rank = __popcll(m & below);
            if (lane == 0) wcnt[wv][q] = __popcll(m);
        }
        __syncthreads();
        int64_t prev = 0;
        if (k >= 0) {
            prev = (k == 0 ? carry[0] : k == 1 ? carry[1] : carry[2]) + rank;
            for (int w = 0; w < wv; ++w) prev += wcnt[w][k];
        }
        const bool keep = k >= 0 && prev < collect;
        const uint64_t mk = __ballot(keep);
        if (lane == 0) wcnt[wv][3] = __popcll(mk);
        [[maybe_unused]] uint64_t mm = 0;
        if constexpr (MIDW > 1) {
            mm = __ballot(keep && k == 0);
            if (lane == 0) wcnt[wv][4] = __popcll(mm);
        }
        __syncthreads();
        if (keep) {
            int64_t pos = taken + __popcll(mk & below);
            for (int w = 0; w < wv; ++w) pos += wcnt[w][3];
            if constexpr (MIDW == 1) {
                pos += base;
                if (pos >= 0 && pos < n_frames) sel[pos] = i;
            } else {
                int64_t mids = taken_mid + __popcll(mm & below);     // kept mid frames before this one
                for (int w = 0; w < wv; ++w) mids += wcnt[w][4];
                const int64_t fr = ffirst[t] + pos;                  // rank among the chunk's selected frames
                const int64_t e = base + pos + (MIDW - 1) * mids;    // its first entry, chunk-relative
                if (fr >= 0 && fr < n_frames) fsel[fr] = i;
                const int ne = k == 0 ? MIDW : 1;
                for (int j = 0; j < ne; ++j)
                    if (fr >= 0 && fr < n_frames && e + j >= 0 && e + j < MIDW * n_frames) {
                        sel[e + j] = i;
                        kind[e + j] = k == 0 ? j : (k == 2);
                        esel[e + j] = fr;
                    }
            }
        }
        for (int q = 0; q < 4; ++q) {
            int64_t s = 0;
            for (int w = 0; w < NWAVE; ++w) s += wcnt[w][q];
            if (q < 3) carry[q] += s; else taken += s;
        }
        if constexpr (MIDW > 1)
            for (int w = 0; w < NWAVE; ++w) taken_mid += wcnt[w][4];
        __syncthreads();
    }
}

// one workgroup per candidate k < span[1]: frame sel[k] of the chunk -> dataset slot span[0] + k, 16 bytes per thread
__global__ __launch_bounds__(TPB) void gather_frames_kernel(const uint4* __restrict__ src, const float* __restrict__ src_pred,
                                                            const int64_t* __restrict__ sel, const int64_t* __restrict__ span,
                                                            int64_t n_src, uint4* __restrict__ dst, float* __restrict__ dst_pred,
                                                            int64_t capacity, int units) {
    const int64_t k = blockIdx.x;
    if (k >= span[1]) return;
    const int64_t s = sel[k], d = span[0] + k;
    if (s < 0 || s >= n_src || d < 0 || d >= capacity) return;
    const uint4* a = src + s * units;
    uint4* b = dst + d * units;
    for (int u = threadIdx.x; u < units; u += TPB) b[u] = a[u];
    if (threadIdx.x == 0 && src_pred && dst_pred) dst_pred[d] = src_pred[s];
}

// 16 pixels per thread: three 16-byte loads of uint8 HWC, four float4 stores per plane.  (float)u8 / 255.0f exactly as
// preprocess_u8_kernel (critic.hip).  An index outside [0, n) yields NaN (never read out of bounds).
__global__ __launch_bounds__(TPB) void preprocess_u8_gather_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ preds,
                                                                   int64_t n, const int64_t* __restrict__ idx, float* __restrict__ x,
                                                                   float* __restrict__ pred, int hw, int bpf) {
    const int64_t b = blockIdx.x / bpf;
    const int g = (int)(blockIdx.x % bpf) * TPB + threadIdx.x;   // 16-pixel group of the frame
    const int64_t s = idx[b];
    const bool ok = s >= 0 && s < n;
    float* d = x + b * 3 * (int64_t)hw + (int64_t)g * 16;
    if (g * 16 >= hw) return;
    if (!ok) {
        const float4 q = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
        for (int c = 0; c < 3; ++c)
            for (int j = 0; j < 4; ++j) reinterpret_cast<float4*>(d + (int64_t)c * hw)[j] = q;
        if (g == 0) pred[b] = __builtin_nanf("");
        return;
    }
    const uint4* src = reinterpret_cast<const uint4*>(frames + s * 3 * (int64_t)hw + (int64_t)g * 48);
    const uint4 v0 = src[0], v1 = src[1], v2 = src[2];
    const uint32_t wd[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
    float o[3][16];
#pragma unroll
    for (int e = 0; e < 48; ++e) {
        const float val = (float)((wd[e >> 2] >> ((e & 3) * 8)) & 0xffu) / 255.0f;
        o[e % 3][e / 3] = val;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            reinterpret_cast<float4*>(d + (int64_t)c * hw)[j] = make_float4(o[c][4 * j], o[c][4 * j + 1], o[c][4 * j + 2], o[c][4 * j + 3]);
    if (g == 0) pred[b] = preds[s];
}

// one thread per zcat element: row e = (mu of selected frame esel[e], kind[e] == 0 ? that frame's critic value : 0);
// an esel outside [0, n_sel) yields a NaN row (never read)
__global__ __launch_bounds__(TPB) void recon_zcat_kernel(const int64_t* __restrict__ esel, const int32_t* __restrict__ kind,
                                                         const float* __restrict__ mu, const float* __restrict__ spred,
                                                         int64_t n_sel, int n_entries, float* __restrict__ zcat) {
    const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (g >= (int64_t)n_entries * 33) return;
    const int e = (int)(g / 33), c = (int)(g % 33);
    const int64_t s = esel[e];
    float v = __builtin_nanf("");
    if (s >= 0 && s < n_sel) v = c < 32 ? mu[s * 32 + c] : (kind[e] == 0 ? spred[s] : 0.0f);
    zcat[g] = v;
}

// one thread per zcat element: row b * R + r = (mu of image b, rewards[r]) — the batch form of vae.py -inject (vae_nets.py:31-40)
__global__ __launch_bounds__(TPB) void inject_zcat_kernel(const float* __restrict__ mu, const float* __restrict__ rewards, int n_rewards,
                                                          int n_rows, float* __restrict__ zcat) {
    const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (g >= (int64_t)n_rows * 33) return;
    const int e = (int)(g / 33), c = (int)(g % 33);
    zcat[g] = c < 32 ? mu[(int64_t)(e / n_rewards) * 32 + c] : rewards[e % n_rewards];
}

// GF32_PER 16-byte units per thread, all loaded before the first store: a wave keeps 4 KiB of one 48 KiB row in flight, a
// workgroup 16 KiB (units / (TPB * GF32_PER) workgroups per image: 3 at 64x64, 12 at 128x128).  Every wave instruction
// covers 1 KiB of contiguous bytes.  An index outside [0, n) yields NaN (never read out of bounds).
constexpr int GF32_PER = 4;
__global__ __launch_bounds__(TPB) void gather_f32_kernel(const uint4* __restrict__ frames, const float* __restrict__ preds, int64_t n,
                                                         const int64_t* __restrict__ idx, uint4* __restrict__ x,
                                                         float* __restrict__ pred, int units, int bpf) {
    const int64_t b = blockIdx.x / bpf;
    const int piece = (int)(blockIdx.x % bpf);
    const int64_t s = idx[b];
    const bool ok = s >= 0 && s < n;
    const int u0 = piece * (TPB * GF32_PER) + threadIdx.x;
    uint4* d = x + b * units + u0;
    uint4 v[GF32_PER];
    if (ok) {
        const uint4* a = frames + s * units + u0;
#pragma unroll
        for (int j = 0; j < GF32_PER; ++j) v[j] = a[j * TPB];
    } else {
        const uint32_t q = 0x7fc00000u;
#pragma unroll
        for (int j = 0; j < GF32_PER; ++j) v[j] = make_uint4(q, q, q, q);
    }
#pragma unroll
    for (int j = 0; j < GF32_PER; ++j) d[j * TPB] = v[j];
    if (piece == 0 && threadIdx.x == 0) pred[b] = ok ? preds[s] : __builtin_nanf("");
}

// ---- the augmented gathers (include/cvae.h: cvae_augment) ----
// What the hash draws for dataset index s.  Every input is uniform over the workgroup (s comes from idx[blockIdx]), so the
// two mix64 run once per wave on the scalar unit, not per pixel.
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct AugDraw { int flip, dx, dy, dnum; };                     // dnum = num - 2^31 = gain_q16 * k

__device__ __forceinline__ AugDraw aug_draw(const cvae_augment& a, int64_t s) {
    const uint64_t r = mix64(a.key ^ mix64((uint64_t)s));
    const uint32_t span = 2u * (uint32_t)a.max_shift + 1u;
    AugDraw d;
    d.flip = (uint32_t)(r >> 40) < a.flip_below;
    d.dnum = a.gain_q16 * ((int)((r >> 24) & 0xFFFFu) - 32768);  // |.| <= 65535 * 32768 < 2^31
    d.dx = (int)((uint32_t)((r >> 12) & 0xFFFu) % span) - a.max_shift;
    d.dy = (int)((uint32_t)(r & 0xFFFu) % span) - a.max_shift;
    return d;
}

__device__ __forceinline__ void aug_record(int32_t* __restrict__ applied, int64_t b, int f, int dx, int dy, int dnum) {
    if (!applied) return;
    applied[b * 4] = f; applied[b * 4 + 1] = dx; applied[b * 4 + 2] = dy; applied[b * 4 + 3] = dnum;
}

// Both kernels keep the plain kernels' grid and stores and stage the source rows of their 4096 output pixels in LDS, each
// row between two pads of W/4 (>= max_shift) copies of its edge pixel:
//   LDS row l = source row clamp(r0 + l - dy) — the vertical shift is done by WHICH row is fetched (16-byte global loads,
//   rows are whole 16-byte units), the pads by the thread that fetched the row's first / last unit — so that the horizontal
//   shift and the flip are one unclamped window per thread: output pixels j0 .. j0+15 (j0 % 16 == 0) are the 16 consecutive
//   padded pixels from vmin + P, vmin = flip ? W-16-j0-dx : j0-dx, in reverse order if flipped.  The window starts at an
//   arbitrary byte (uint8) or float (fp32), so the thread reads the aligned dwords (13) or 16-byte units (2) that cover it
//   and shifts in registers — no byte-wide LDS reads.
// One barrier; an out-of-range index leaves the workgroup before it (the test is uniform).
template <int W> struct AugU8 {
    static constexpr int P = W / 4;                      // pad pixels per side
    static constexpr int ROWB = (W + 2 * P) * 3;         // 288 / 576 bytes: whole 16-byte units
    static constexpr int R = 4096 / W;                   // rows per workgroup: 64 / 32
    static constexpr int UPR = W * 3 / 16;               // 16-byte units per source row: 12 / 24
    static constexpr int PADU = P * 3 / 16;              // ... per pad: 3 / 6
    static constexpr int BPF = W * W / 4096;             // workgroups per frame
    static constexpr int LDSB = R * ROWB + 64;           // the last row's window may read one unit past it (never used)
};

template <int W>
__global__ __launch_bounds__(TPB) void preprocess_u8_gather_aug_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ preds,
                                                                       int64_t n, const int64_t* __restrict__ idx, cvae_augment aug,
                                                                       float* __restrict__ x, float* __restrict__ pred,
                                                                       int32_t* __restrict__ applied) {
    using K = AugU8<W>;
    __shared__ uint4 lds[K::LDSB / 16];
    constexpr int hw = W * W;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / K::BPF;
    const int piece = (int)(blockIdx.x % K::BPF);
    const int64_t s = idx[b];
    float* d = x + b * 3 * (int64_t)hw + (int64_t)piece * 4096 + tid * 16;
    if (!(s >= 0 && s < n)) {
        const float4 q = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
        for (int c = 0; c < 3; ++c)
            for (int j = 0; j < 4; ++j) reinterpret_cast<float4*>(d + (int64_t)c * hw)[j] = q;
        if (piece == 0 && tid == 0) { pred[b] = __builtin_nanf(""); aug_record(applied, b, 0, 0, 0, 0); }
        return;
    }
    const AugDraw a = aug_draw(aug, s);
    const float g = (float)((uint32_t)a.dnum + 0x80000000u) * 0x1p-31f;
    if (piece == 0 && tid == 0) { pred[b] = preds[s]; aug_record(applied, b, a.flip, a.dx, a.dy, a.dnum); }

    // stage: 768 units of 16 bytes, three per thread, all loaded before the first LDS store
    const uint4* src = reinterpret_cast<const uint4*>(frames + s * 3 * (int64_t)hw);
    const int r0 = piece * K::R;
    uint4 v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int lu = j * TPB + tid, l = lu / K::UPR, wi = lu % K::UPR;
        int si = r0 + l - a.dy;
        si = si < 0 ? 0 : (si > W - 1 ? W - 1 : si);
        v[j] = src[si * K::UPR + wi];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int lu = j * TPB + tid, l = lu / K::UPR, wi = lu % K::UPR;
        uint4* row = lds + l * (K::ROWB / 16);
        row[K::PADU + wi] = v[j];
        if (wi == 0 || wi == K::UPR - 1) {                      // the row's first pixel (bytes 0..2) or last (bytes 13..15)
            const uint32_t p = wi == 0 ? (v[j].x & 0xffffffu) : (v[j].w >> 8);
            const uint32_t d0 = p | (p << 24), d1 = (p >> 8) | (p << 16), d2 = (p >> 16) | (p << 8);      // 12-byte period
            uint4* pad = row + (wi == 0 ? 0 : K::PADU + K::UPR);
#pragma unroll
            for (int u = 0; u < K::PADU; u += 3) {
                pad[u] = make_uint4(d0, d1, d2, d0); pad[u + 1] = make_uint4(d1, d2, d0, d1); pad[u + 2] = make_uint4(d2, d0, d1, d2);
            }
        }
    }
    __syncthreads();

    // assemble: 48 bytes from byte `start` of the padded row
    const int l = tid / (W / 16), j0 = (tid % (W / 16)) * 16;
    const int vmin = a.flip ? W - 16 - j0 - a.dx : j0 - a.dx;
    const int start = (vmin + K::P) * 3, sh = (start & 3) * 8;
    const uint32_t* win = reinterpret_cast<const uint32_t*>(lds) + l * (K::ROWB / 4) + (start >> 2);
    uint32_t e[13];                                             // the 13 aligned dwords that cover the window
#pragma unroll
    for (int m = 0; m < 13; ++m) e[m] = win[m];
    uint32_t wd[12];
#pragma unroll
    for (int m = 0; m < 12; ++m) wd[m] = (uint32_t)((((uint64_t)e[m + 1] << 32) | e[m]) >> sh);
    float o[3][16];
#pragma unroll
    for (int t = 0; t < 48; ++t) {
        const float val = (float)((wd[t >> 2] >> ((t & 3) * 8)) & 0xffu) / 255.0f;      // the plain gather's value ...
        o[t % 3][t / 3] = fminf(val * g, 1.0f);                                        // ... times the gain, clamped
    }
    if (a.flip) {                                               // uniform: the window holds the pixels in reverse order
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                reinterpret_cast<float4*>(d + (int64_t)c * hw)[j] = make_float4(o[c][15 - 4 * j], o[c][14 - 4 * j], o[c][13 - 4 * j], o[c][12 - 4 * j]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                reinterpret_cast<float4*>(d + (int64_t)c * hw)[j] = make_float4(o[c][4 * j], o[c][4 * j + 1], o[c][4 * j + 2], o[c][4 * j + 3]);
    }
}

// fp32 entries: the same staging per channel plane (a workgroup's 1024 units are R whole rows of one plane), bit copies.
template <int W> struct AugF32 {
    static constexpr int P = W / 4;                      // pad floats per side
    static constexpr int ROWU = (W + 2 * P) / 4;         // 16-byte units per padded row: 24 / 48
    static constexpr int R = 4096 / W;                   // rows per workgroup
    static constexpr int UPR = W / 4, PADU = P / 4;
    static constexpr int BPF = 3 * W * W / 4096;         // workgroups per entry: 3 / 12
    static constexpr int LDSU = R * ROWU + 2;
};

template <int W>
__global__ __launch_bounds__(TPB) void gather_f32_aug_kernel(const uint4* __restrict__ frames, const float* __restrict__ preds, int64_t n,
                                                             const int64_t* __restrict__ idx, cvae_augment aug, uint4* __restrict__ x,
                                                             float* __restrict__ pred, int32_t* __restrict__ applied) {
    using K = AugF32<W>;
    __shared__ uint4 lds[K::LDSU];
    constexpr int units = 3 * W * W / 4;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / K::BPF;
    const int piece = (int)(blockIdx.x % K::BPF);
    const int64_t s = idx[b];
    uint4* d = x + b * units + piece * (TPB * GF32_PER) + tid;
    if (!(s >= 0 && s < n)) {
        const uint32_t q = 0x7fc00000u;
#pragma unroll
        for (int j = 0; j < GF32_PER; ++j) d[j * TPB] = make_uint4(q, q, q, q);
        if (piece == 0 && tid == 0) { pred[b] = __builtin_nanf(""); aug_record(applied, b, 0, 0, 0, 0); }
        return;
    }
    const AugDraw a = aug_draw(aug, s);
    if (piece == 0 && tid == 0) { pred[b] = preds[s]; aug_record(applied, b, a.flip, a.dx, a.dy, a.dnum); }

    const int c = piece * K::R / W, r0 = piece * K::R % W;       // the plane and the first row of this workgroup
    const uint4* src = frames + s * units + c * (W * K::UPR);
    uint4 v[GF32_PER];
#pragma unroll
    for (int j = 0; j < GF32_PER; ++j) {
        const int lu = j * TPB + tid, l = lu / K::UPR, wi = lu % K::UPR;
        int si = r0 + l - a.dy;
        si = si < 0 ? 0 : (si > W - 1 ? W - 1 : si);
        v[j] = src[si * K::UPR + wi];
    }
#pragma unroll
    for (int j = 0; j < GF32_PER; ++j) {
        const int lu = j * TPB + tid, l = lu / K::UPR, wi = lu % K::UPR;
        uint4* row = lds + l * K::ROWU;
        row[K::PADU + wi] = v[j];
        if (wi == 0 || wi == K::UPR - 1) {
            const uint32_t p = wi == 0 ? v[j].x : v[j].w;
            uint4* pad = row + (wi == 0 ? 0 : K::PADU + K::UPR);
#pragma unroll
            for (int u = 0; u < K::PADU; ++u) pad[u] = make_uint4(p, p, p, p);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < GF32_PER; ++j) {
        const int lu = j * TPB + tid, l = lu / K::UPR, j0 = (lu % K::UPR) * 4;
        const int vmin = a.flip ? W - 4 - j0 - a.dx : j0 - a.dx;
        const int start = vmin + K::P, q = start & 3;
        const uint4* win = lds + l * K::ROWU + (start >> 2);
        const uint4 w0 = win[0], w1 = win[1];
        uint32_t e[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
        if (q & 1) {
#pragma unroll
            for (int m = 0; m < 7; ++m) e[m] = e[m + 1];
        }
        if (q & 2) {
#pragma unroll
            for (int m = 0; m < 6; ++m) e[m] = e[m + 2];
        }
        d[j * TPB] = a.flip ? make_uint4(e[3], e[2], e[1], e[0]) : make_uint4(e[0], e[1], e[2], e[3]);
    }
}

// the three launches of one chunk's selection; the recon-only outputs are null at MIDW = 1
template <int MIDW>
int launch_curate(int n_traj, const int64_t* off, int64_t n_frames, const float* preds, int collect, int64_t total_images,
                  int64_t* running, int64_t* counts, int64_t* first, int64_t* sel_first, int64_t* span, int64_t* ent_frame,
                  int32_t* ent_kind, int64_t* ent_sel, int64_t* sel, hipStream_t st) {
    if (n_traj > 0) {
        hipLaunchKernelGGL(curate_count_kernel, dim3((unsigned)n_traj), dim3(TPB), 0, st, preds, off, n_frames, collect, counts);
        CVAE_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(curate_cut_kernel<MIDW>, dim3(1), dim3(TPB), 0, st, n_traj, total_images, running, counts, first, span, sel_first);
    CVAE_CHECK_LAUNCH();
    if (n_traj > 0) {
        hipLaunchKernelGGL(curate_scatter_kernel<MIDW>, dim3((unsigned)n_traj), dim3(TPB), 0, st, preds, off, n_frames, collect, first,
                           span, ent_frame, (const int64_t*)sel_first, ent_kind, ent_sel, sel);
        CVAE_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace

int launch_curate_select(int n_traj, const int64_t* off, int64_t n_frames, const float* preds, int collect,
                         int64_t total_images, int64_t* running, int64_t* counts, int64_t* first, int64_t* span,
                         int64_t* sel, hipStream_t st) {
    return launch_curate<1>(n_traj, off, n_frames, preds, collect, total_images, running, counts, first, nullptr, span, sel,
                            nullptr, nullptr, nullptr, st);
}

int launch_curate_select_recon(int n_traj, const int64_t* off, int64_t n_frames, const float* preds, int collect,
                               int64_t total_images, int64_t* running, int64_t* counts, int64_t* first, int64_t* sel_first,
                               int64_t* span, int64_t* ent_frame, int32_t* ent_kind, int64_t* ent_sel, int64_t* sel,
                               hipStream_t st) {
    return launch_curate<2>(n_traj, off, n_frames, preds, collect, total_images, running, counts, first, sel_first, span,
                            ent_frame, ent_kind, ent_sel, sel, st);
}

int launch_recon_zcat(int n_entries, const int64_t* ent_sel, const int32_t* ent_kind, const float* mu, const float* sel_pred,
                      int64_t n_sel, float* zcat, hipStream_t st) {
    const int64_t total = (int64_t)n_entries * 33;
    hipLaunchKernelGGL(recon_zcat_kernel, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, st, ent_sel, ent_kind, mu, sel_pred,
                       n_sel, n_entries, zcat);
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_inject_zcat(int n_images, int n_rewards, const float* mu, const float* rewards, float* zcat, hipStream_t st) {
    const int n_rows = n_images * n_rewards;
    const int64_t total = (int64_t)n_rows * 33;
    hipLaunchKernelGGL(inject_zcat_kernel, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, st, mu, rewards, n_rewards, n_rows, zcat);
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_gather_f32(int width, int B, const float* frames, const float* preds, int64_t n, const int64_t* idx, float* x,
                      float* pred, hipStream_t st) {
    const int units = width * width * 3 / 4, bpf = units / (TPB * GF32_PER);
    hipLaunchKernelGGL(gather_f32_kernel, dim3((unsigned)((int64_t)B * bpf)), dim3(TPB), 0, st, (const uint4*)frames, preds, n, idx,
                       (uint4*)x, pred, units, bpf);
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_preprocess_u8_gather_aug(int width, int B, const uint8_t* frames, const float* preds, int64_t n, const int64_t* idx,
                                    const cvae_augment& aug, float* x, float* pred, int32_t* applied, hipStream_t st) {
    if (width == 64)
        hipLaunchKernelGGL(preprocess_u8_gather_aug_kernel<64>, dim3((unsigned)((int64_t)B * AugU8<64>::BPF)), dim3(TPB), 0, st, frames,
                           preds, n, idx, aug, x, pred, applied);
    else if (width == 128)
        hipLaunchKernelGGL(preprocess_u8_gather_aug_kernel<128>, dim3((unsigned)((int64_t)B * AugU8<128>::BPF)), dim3(TPB), 0, st, frames,
                           preds, n, idx, aug, x, pred, applied);
    else { cvae_set_error("preprocess_u8_gather_aug: width %d unsupported", width); return -2; }
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_gather_f32_aug(int width, int B, const float* frames, const float* preds, int64_t n, const int64_t* idx,
                          const cvae_augment& aug, float* x, float* pred, int32_t* applied, hipStream_t st) {
    if (width == 64)
        hipLaunchKernelGGL(gather_f32_aug_kernel<64>, dim3((unsigned)((int64_t)B * AugF32<64>::BPF)), dim3(TPB), 0, st,
                           (const uint4*)frames, preds, n, idx, aug, (uint4*)x, pred, applied);
    else if (width == 128)
        hipLaunchKernelGGL(gather_f32_aug_kernel<128>, dim3((unsigned)((int64_t)B * AugF32<128>::BPF)), dim3(TPB), 0, st,
                           (const uint4*)frames, preds, n, idx, aug, (uint4*)x, pred, applied);
    else { cvae_set_error("gather_f32_aug: width %d unsupported", width); return -2; }
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_gather_frames_u8(int width, const uint8_t* src, const float* src_pred, int64_t n_src, const int64_t* sel,
                            int64_t max_count, const int64_t* span, uint8_t* dst, float* dst_pred, int64_t capacity,
                            hipStream_t st) {
    if (max_count == 0) return 0;
    const int units = width * width * 3 / 16;
    hipLaunchKernelGGL(gather_frames_kernel, dim3((unsigned)max_count), dim3(TPB), 0, st, (const uint4*)src, src_pred, sel, span,
                       n_src, (uint4*)dst, dst_pred, capacity, units);
    CVAE_CHECK_LAUNCH();
    return 0;
}

int launch_preprocess_u8_gather(int width, int B, const uint8_t* frames, const float* preds, int64_t n, const int64_t* idx,
                                float* x, float* pred, hipStream_t st) {
    const int hw = width * width, bpf = hw / 16 / TPB;          // 1 workgroup per frame at 64x64, 4 at 128x128
    hipLaunchKernelGGL(preprocess_u8_gather_kernel, dim3((unsigned)((int64_t)B * bpf)), dim3(TPB), 0, st, frames, preds, n, idx,
                       x, pred, hw, bpf);
    CVAE_CHECK_LAUNCH();
    return 0;
}
