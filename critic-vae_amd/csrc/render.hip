// render.hip — the pictures the reference's users look at, composed on the device: the PNG strips of image_evaluate
// (vae.py:68-108) and get_injected_img (vae_utility.py:240-254) and the 7-panel video frames of get_final_frame
// (vae_utility.py:286-322).
//
//   compose_frames   B pictures (B, ih + w, n_panels * w, 3) uint8 HWC out of up to 8 panels of w x w pixels side by side at
//                    row offset ih (rows above it black), plus optional white text: an overlay shared by all pictures and
//                    one label of an atlas per picture.
//
// Panel pixel rules, each what the reference's host code does:
//   F32_CHW  prepare_rgb_image: (img * 255).astype(np.uint8) = one fp32 multiply (rounded to nearest, never contracted into
//            an FMA), truncation toward zero to int32, the low 8 bits (two's-complement wrap: the decoder ends in Tanh and
//            negative pixels show wrapped in the reference's pictures); NaN, +-inf and |v * 255| >= 2^31 give 0.
//   U8_HWC   copied.   U8_GREY  Image mode L pasted into RGB: replicated.   MASK  Image mode 1 pasted into RGB: 255 or 0.
//
// One thread = 16 output bytes = one 16-byte store; a wave's store instruction covers 1 KiB of one picture.  16 bytes are
// 5 1/3 pixels, so a thread reads the 8 pixels (4-aligned) that contain them: two float4 per plane for F32_CHW, two dwords
// for the one-byte kinds, one uint4 for U8_HWC.  Three consecutive threads share a 16-pixel group (phase m = 0, 1, 2).
// Pure function of the inputs: no atomics, no scratch, picture offsets in 64 bits.
#include "common.h"
#include "../../include/cvae.h"

namespace {

constexpr int TPB = 256;

struct ComposeArgs {
    cvae_panel panel[CVAE_MAX_PANELS];
    const uint8_t* overlay;      // (Hout, Wout) or null
    const uint8_t* atlas;        // (n_labels, lh, lw) or null
    const int32_t* label_idx;    // (B)
    uint8_t* out;
    int64_t pic_bytes;
    int w, ih, n_panels, upp, upr, bpp, units;   // units per panel row / picture row, workgroups and units per picture
    int n_labels, lh, lw, lx, ly, clamp;
};

__device__ __forceinline__ uint32_t to_u8(float v, int clamp) {
    const float t = __fmul_rn(v, 255.0f);
    int q = fabsf(t) < 2147483648.0f ? (int)t : 0;           // NaN compares false
    if (clamp) q = q < 0 ? 0 : (q > 255 ? 255 : q);
    return (uint32_t)q & 0xffu;
}

// bytes 16 M .. 16 M + 15 of a 16-pixel RGB group from the 8 pixels 4 M .. 4 M + 7 (px[i] = 0x00BBGGRR); white[i] wins
template <int M>
__device__ __forceinline__ uint4 pack16(const uint32_t (&px)[8]) {
    uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int a = 16 * M + e, i = a / 3 - 4 * M, c = a % 3;
        wd[e >> 2] |= ((px[i] >> (8 * c)) & 0xffu) << (8 * (e & 3));
    }
    return make_uint4(wd[0], wd[1], wd[2], wd[3]);
}

__global__ __launch_bounds__(TPB) void compose_frames_kernel(const ComposeArgs a) {
    const int64_t b = blockIdx.x / a.bpp;
    const int u = (int)(blockIdx.x % a.bpp) * TPB + threadIdx.x;     // 16-byte unit of the picture
    if (u >= a.units) return;
    const int y = u / a.upr, ur = u - y * a.upr;
    const int p = ur / a.upp, k = ur - p * a.upp;
    const int m = k % 3, x0 = (k / 3) * 16 + 4 * m;                  // first of the 8 pixels read, in the panel row
    const int sy = y - a.ih;
    uint4 o;
    bool packed = false;
    uint32_t px[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (sy >= 0) {
        const cvae_panel pn = a.panel[p];
        const int64_t poff = b * pn.batch_stride + (int64_t)sy * a.w;   // first element of the source row (per plane / per byte)
        if (pn.kind == CVAE_PANEL_U8_HWC) {
            o = *reinterpret_cast<const uint4*>((const uint8_t*)pn.data + (b * pn.batch_stride + (int64_t)sy * a.w * 3) + 16 * k);
            packed = true;
        } else if (pn.kind == CVAE_PANEL_F32_CHW) {
            const float* s = (const float*)pn.data + poff + x0;
            const int64_t hw = (int64_t)a.w * a.w;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 v0 = reinterpret_cast<const float4*>(s + c * hw)[0];
                const float4 v1 = reinterpret_cast<const float4*>(s + c * hw)[1];
                const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
                for (int i = 0; i < 8; ++i) px[i] |= to_u8(v[i], a.clamp) << (8 * c);
            }
        } else {
            const uint32_t* s = reinterpret_cast<const uint32_t*>((const uint8_t*)pn.data + poff + x0);
            const uint32_t d[2] = {s[0], s[1]};
            const bool mask = pn.kind == CVAE_PANEL_MASK;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                uint32_t g = (d[i >> 2] >> (8 * (i & 3))) & 0xffu;
                if (mask) g = g ? 255u : 0u;
                px[i] = g * 0x010101u;
            }
        }
    }
    // white text: where set, the pixel becomes white whatever the panel holds
    const int X0 = p * a.w + x0;                                     // picture column of px[0]
    uint32_t white = 0;                                              // bit i: px[i] is white
    if (a.overlay) {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(a.overlay + (int64_t)y * (a.n_panels * a.w) + X0);
        const uint32_t d[2] = {s[0], s[1]};
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if ((d[i >> 2] >> (8 * (i & 3))) & 0xffu) white |= 1u << i;
    }
    if (a.atlas && y >= a.ly && y < a.ly + a.lh && X0 + 8 > a.lx && X0 < a.lx + a.lw) {
        const int li = a.label_idx[b];
        if (li >= 0 && li < a.n_labels) {
            const uint8_t* g = a.atlas + ((int64_t)li * a.lh + (y - a.ly)) * a.lw;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int gx = X0 + i - a.lx;
                if (gx >= 0 && gx < a.lw && g[gx]) white |= 1u << i;
            }
        }
    }
    if (packed) {
        if (white) {                                                 // rare: byte e of the unit belongs to pixel (16 m + e) / 3
            uint32_t ow[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int i = (16 * m + e) / 3 - 4 * m;
                if ((white >> i) & 1u) ow[e >> 2] |= 0xffu << (8 * (e & 3));
            }
            o = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if ((white >> i) & 1u) px[i] = 0xffffffu;
        o = m == 0 ? pack16<0>(px) : (m == 1 ? pack16<1>(px) : pack16<2>(px));
    }
    *reinterpret_cast<uint4*>(a.out + b * a.pic_bytes + (int64_t)u * 16) = o;
}

}  // namespace

int launch_compose_frames(int width, int B, int n_panels, const cvae_panel* panels, int ih, int clamp, const uint8_t* overlay,
                          const uint8_t* atlas, int n_labels, int lh, int lw, const int32_t* label_idx, int lx, int ly,
                          uint8_t* out, hipStream_t st) {
    ComposeArgs a{};
    for (int i = 0; i < n_panels; ++i) a.panel[i] = panels[i];
    a.overlay = overlay; a.atlas = atlas; a.label_idx = label_idx; a.out = out;
    a.w = width; a.ih = ih; a.n_panels = n_panels;
    a.upp = width * 3 / 16;
    a.upr = a.upp * n_panels;
    const int64_t units = (int64_t)(ih + width) * a.upr;
    a.units = (int)units;
    a.pic_bytes = units * 16;
    a.bpp = (int)((units + TPB - 1) / TPB);
    a.n_labels = n_labels; a.lh = lh; a.lw = lw; a.lx = lx; a.ly = ly; a.clamp = clamp;
    const int64_t blocks = (int64_t)B * a.bpp;
    if (blocks > 0x7fffffffLL) {
        cvae_set_error("cvae_compose_frames: %lld workgroups (batch %d x %d per picture) do not fit one launch", (long long)blocks, B, a.bpp);
        return CVAE_EINVAL;
    }
    hipLaunchKernelGGL(compose_frames_kernel, dim3((unsigned)blocks), dim3(TPB), 0, st, a);
    CVAE_CHECK_LAUNCH();
    return 0;
}
