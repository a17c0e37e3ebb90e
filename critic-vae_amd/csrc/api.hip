// api.hip — the C-ABI of include/cvae.h: handle, flat parameter layout, workspace carve and the
// forward / loss / backward / optimizer orchestration.  Host code only; every launch is
// asynchronous on the caller's stream, nothing here allocates or synchronises.
#include "common.h"
#include "../../include/cvae.h"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <cmath>
#include <string>
#include <vector>

static thread_local char g_err[512] = "";
void cvae_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- in-step kernel probe: ids = kind*9 + layer, kind 0 fwd / 1 dgrad / 2 wgrad (conv kernels; layer 0 = E1: id 0 its
//      forward — the BatchNorm/pool pass in two-pass mode —, id 18 its weight gradient; layer 8 = D4: id 8 forward,
//      id 17 the fused backward);  kind 3: ids 27..30 = the BatchNorm+pool backward apply kernel of encoder block
//      `layer` (HBM-bound), id 31 = the MS-SSIM level-0 tile kernel ----
static constexpr int PROBE_IDS = 32, PROBE_CAP = 128;
struct ProbeSlot { hipEvent_t e0[PROBE_CAP], e1[PROBE_CAP]; int n = 0; bool made = false; };
struct ProbeState { uint32_t mask = 0; ProbeSlot slot[PROBE_IDS]; };
static thread_local ProbeSlot* g_probe_cur = nullptr;
void cvae_probe_begin(hipStream_t st) {
    ProbeSlot* p = g_probe_cur;
    if (p && p->n < PROBE_CAP) (void)hipEventRecord(p->e0[p->n], st);
}
void cvae_probe_end(hipStream_t st) {
    ProbeSlot* p = g_probe_cur;
    if (p && p->n < PROBE_CAP) { (void)hipEventRecord(p->e1[p->n], st); p->n++; }
}

// Compute units of the current device.  Sizes persistent grids and split counts only (never a result), so a failed
// query falls back to the MI355X's 256 — but not silently: the error string says so (the launch that follows still
// succeeds, and cvae_last_error() then explains an unexpected grid).  Cached per device ordinal (ordinals past the
// table are queried every time rather than aliased onto another device's entry).
int cvae_num_cus() {
    constexpr int NCACHE = 64;
    static std::atomic<int> cached[NCACHE];                  // 0 = not yet queried
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) { cvae_set_error("cvae_num_cus: hipGetDevice failed (%s); assuming 256 compute units", hipGetErrorString(e)); return 256; }
    const bool cacheable = dev >= 0 && dev < NCACHE;
    int n = cacheable ? cached[dev].load(std::memory_order_relaxed) : 0;
    if (n > 0) return n;
    e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess || n <= 0) {
        cvae_set_error("cvae_num_cus: compute-unit query failed on device %d (%s); assuming 256", dev, hipGetErrorString(e));
        return 256;                                          // not cached: the next call asks again
    }
    if (cacheable) cached[dev].store(n, std::memory_order_relaxed);
    return n;
}

int persistent_grid(int wgs_per_cu, int num_items) {
    // CVAE_PERSIST_MAXWG (tests): caps the grid, so that test batches walk several items per workgroup; 0 (unset) = no cap
    static const int maxwg = [] { const char* e = getenv("CVAE_PERSIST_MAXWG"); const int n = e ? atoi(e) : 0; return n > 0 ? n : 0; }();
    int G = wgs_per_cu * cvae_num_cus();
    if (maxwg > 0 && G > maxwg) G = maxwg;
    G -= G % 8;
    if (G < 8) G = 8;
    return G < num_items ? G : num_items;
}
// include/cvae.h: which kernel family a conv pass of E2..E4 takes at a batch size (host logic only, no device access)
extern "C" int32_t cvae_conv_route(int32_t precision, int32_t width, int32_t layer, int32_t dgrad, int64_t batch) {
    if ((width != 64 && width != 128) || layer < 0 || layer > 3 || precision < 0 || precision > 3 || batch < 1 || batch > 0x7fffffffLL) return CVAE_EINVAL;
    if (layer == 0 && (precision != 1 || dgrad != 0)) return CVAE_EINVAL;        // layer 0: the packed-frame row of bf16 mode only
    return conv_route(precision, layer, width, dgrad != 0, batch).family;
}

struct ParamEntry { std::string name; int64_t offset, numel; };

struct WsLayout {
    int64_t y[4], a[4], coef[4], bnpart[4];
    int64_t zcat, h, o[4];
    int64_t dout4, d_o[4], d_h, d_zcat, d_a[4], d_y[4];
    int64_t wc[3];             // phase-collapsed weights of D1..D3 (rebuilt every forward)
    int64_t xp;                // bf16 mode: the frame as packed bf16 (r, g, b, 0) pixels, written by E1's statistics pass (B * W * W * 8 bytes)
    int64_t wpack;             // bf16 mode: packed E2..E4 / D0 weights, forward + dgrad orientation (rebuilt every forward)
    int64_t ms, scratch_w, scratch, total;     // scratch_w: wgrad slabs (side stream); scratch: everything else (last)
};

struct cvae_handle_s {
    cvae_config cfg;
    std::vector<ParamEntry> params;
    int64_t param_total;
    int K;                       // bottleneck
    // parameter indices
    int enc_w[4], enc_b[4], enc_g[4], enc_be[4], fc_w, fc_b, dec_w[5], dec_b[5], di_w, di_b;
    // weight-gradient work runs on a lower-priority side stream, off the dgrad critical path
    hipStream_t side = nullptr;
    hipEvent_t ev_ready[8] = {}, ev_side = nullptr;
    bool streams_ready = false;
    const void* xp_ws = nullptr;     // the workspace (and batch) whose packed bf16 frame the last train-mode forward wrote: the backward stages E1's strips from
    int xp_B = 0;                    // it only then (an eval-mode forward, or another workspace, leaves it stale -> the fp32 frame is staged instead)
    // staged (cross-rank) step: the stage the handle expects next — pass 0 forward (stages 0..4), 1 loss (0..1), 2 backward
    // (0..4) — and the workspace, batch and record the step runs on.  Forward stage 0 may always start a new step.
    struct { int pass = 0, next = 0, B = 0; const void* ws = nullptr; const double* rec = nullptr; } sync;
    ProbeState probe;
};

struct ProbeArm {      // RAII: arm the slot of (kind, layer) for the launches inside the scope
    ProbeArm(cvae_handle_s* h, int kind, int layer) {
        const int id = kind * 9 + layer;
        g_probe_cur = (h->probe.mask >> id) & 1u ? &h->probe.slot[id] : nullptr;
    }
    ~ProbeArm() { g_probe_cur = nullptr; }
};

static int ensure_streams(cvae_handle_s* h) {
    if (h->streams_ready) return 0;
    int lo = 0, hi = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);      // lo = least priority
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, lo);
    for (int i = 0; i < 8 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&h->ev_ready[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_side, hipEventDisableTiming);
    if (e != hipSuccess) { cvae_set_error("side stream setup failed: %s", hipGetErrorString(e)); return (int)e; }
    h->streams_ready = true;
    return 0;
}

static int layer_h(const cvae_handle_s* h, int layer) { return kLayers[layer].h * (h->cfg.width / 64); }
static int64_t pack_floats(const cvae_handle_s* h);      // with the conv table below

static WsLayout carve(const cvae_handle_s* h, int B) {
    WsLayout w{};
    const int W = h->cfg.width;
    int64_t off = 0;
    auto take = [&](int64_t n) { int64_t o = off; off += align_up(n, 64); return o; };
    // activation / activation-gradient slots hold bf16 elements in precision mode 1: half the floats
    const bool b16 = h->cfg.precision == 1;
    auto act = [&](int64_t elems) { return take(b16 ? (elems + 1) / 2 : elems); };
    for (int l = 0; l < 4; ++l) {
        const int64_t H = layer_h(h, l), C = kLayers[l].cout;
        w.y[l] = act(B * H * H * C);
        w.a[l] = act(B * (H / 2) * (H / 2) * C);
        w.coef[l] = take(C * 4);
        w.bnpart[l] = take((int64_t)2 * bn_num_tiles(l, W, B) * C);
        // block 0 has no d_y (E1's weight-gradient kernel applies the BatchNorm backward itself);
        // the slot keeps its offset entry (-1 -> "not allocated") for cvae_ws_offset
        w.d_y[l] = l == 0 ? -1 : act(B * H * H * C);
        w.d_a[l] = act(B * (H / 2) * (H / 2) * C);
    }
    w.zcat = take((int64_t)B * 33);
    w.d_zcat = take((int64_t)B * 33);
    w.h = act((int64_t)B * h->K);
    w.d_h = act((int64_t)B * h->K);
    for (int i = 0; i < 4; ++i) {
        const int64_t H = layer_h(h, 4 + i), C = kLayers[4 + i].cout;
        w.o[i] = act(B * H * H * C);
        w.d_o[i] = act(B * H * H * C);
    }
    w.dout4 = take(b16 ? 0 : (int64_t)B * 3 * W * W);          // bf16 mode applies the Tanh backward inside d4_bwd: no dOut tensor
    for (int i = 0; i < 3; ++i) w.wc[i] = take(conv_up_wc_floats(5 + i));
    w.xp = take(b16 ? (int64_t)B * W * W * 2 : 0);
    w.wpack = take(pack_floats(h));
    w.ms = take(msssim_ws_floats(W, B));
    int64_t sc = 0, scw = 0;
    auto mx = [&](int64_t v) { if (v > sc) sc = v; };
    for (int l = 1; l <= 4; ++l) { if (wgrad_ws_floats(l, W, B) > scw) scw = wgrad_ws_floats(l, W, B);
        if (h->cfg.precision == 1 && wgrad_bf16_ws_floats(l, W, B) > scw) scw = wgrad_bf16_ws_floats(l, W, B);
        if (h->cfg.precision >= 2 && wgrad_split_ws_floats(l, W, B) > scw) scw = wgrad_split_ws_floats(l, W, B);
        mx(conv_fwd_ws_floats(l, W, B)); mx(conv_dgrad_ws_floats(l, W, B)); }
    for (int l = 5; l <= 7; ++l) { if (conv_up_wgrad_ws_floats(l, W, B) > scw) scw = conv_up_wgrad_ws_floats(l, W, B); mx(conv_up_ws_floats(l, W, B)); }
    if (e1_wgrad_ws_floats(W, B) > scw) scw = e1_wgrad_ws_floats(W, B);
    w.scratch_w = take(scw);
    mx(scw + 36 * 128 * 64);                   // per-op entry points: one scratch = [collapsed W | everything else]
    mx(d4_bwd_ws_floats(W, B));
    for (int l = 0; l < 4; ++l) { mx(bn_bwd_ws_floats(l, W, B)); mx(bn_fwd_ws_floats(l, W)); }
    mx(fc_ws_floats(W, B));
    mx(colsum_ws_floats(0, 256));
    w.scratch = take(sc);
    w.total = off;
    return w;
}

static void add_param(cvae_handle_s* h, int* idx, const char* name, int64_t numel) {
    *idx = (int)h->params.size();
    h->params.push_back(ParamEntry{name, h->param_total, numel});
    h->param_total += align_up(numel, 64);
}

extern "C" {

const char* cvae_version(void) { return "critic-vae_amd 0.3 (gfx950; fp32 MFMA, bf16 MFMA with bf16 storage)"; }
const char* cvae_last_error(void) { return g_err; }

int cvae_create(const cvae_config* cfg, cvae_handle* out) {
    if (!cfg || !out) { cvae_set_error("cvae_create: null argument"); return CVAE_EINVAL; }
    if (cfg->width != 64 && cfg->width != 128) { cvae_set_error("cvae_create: width %d not supported (64 or 128)", cfg->width); return CVAE_EUNSUPPORTED; }
    if (cfg->precision < 0 || cfg->precision > 3) { cvae_set_error("cvae_create: precision %d not supported (0 = fp32, 1 = bf16 MFMA, 2 = fp32 emulated by 3-way bf16 splits)", cfg->precision); return CVAE_EUNSUPPORTED; }
    cvae_handle_s* h = new cvae_handle_s();
    h->cfg = *cfg;
    h->param_total = 0;
    h->K = 256 * (cfg->width / 16) * (cfg->width / 16);
    char nm[64];
    for (int l = 0; l < 4; ++l) {
        snprintf(nm, sizeof nm, "enc%d.w", l); add_param(h, &h->enc_w[l], nm, (int64_t)25 * kLayers[l].cin * kLayers[l].cout);
        snprintf(nm, sizeof nm, "enc%d.b", l); add_param(h, &h->enc_b[l], nm, kLayers[l].cout);
        snprintf(nm, sizeof nm, "enc%d.gamma", l); add_param(h, &h->enc_g[l], nm, kLayers[l].cout);
        snprintf(nm, sizeof nm, "enc%d.beta", l); add_param(h, &h->enc_be[l], nm, kLayers[l].cout);
    }
    add_param(h, &h->fc_w, "fc.w", (int64_t)h->K * 64);
    add_param(h, &h->fc_b, "fc.b", 64);
    for (int i = 0; i < 5; ++i) {
        snprintf(nm, sizeof nm, "dec%d.w", i); add_param(h, &h->dec_w[i], nm, (int64_t)25 * kLayers[4 + i].cin * kLayers[4 + i].cout);
        snprintf(nm, sizeof nm, "dec%d.b", i); add_param(h, &h->dec_b[i], nm, kLayers[4 + i].cout);
    }
    add_param(h, &h->di_w, "decin.w", (int64_t)33 * h->K);
    add_param(h, &h->di_b, "decin.b", h->K);
    *out = h;
    return CVAE_OK;
}

void cvae_destroy(cvae_handle h) {
    if (!h) return;
    if (h->streams_ready) {
        for (int i = 0; i < 8; ++i) (void)hipEventDestroy(h->ev_ready[i]);
        (void)hipEventDestroy(h->ev_side);
        (void)hipStreamDestroy(h->side);
    }
    delete h;
}

int64_t cvae_param_total(cvae_handle h) { return h->param_total; }
int32_t cvae_param_count(cvae_handle h) { return (int32_t)h->params.size(); }
const char* cvae_param_name(cvae_handle h, int32_t i) { return h->params[i].name.c_str(); }
int64_t cvae_param_offset(cvae_handle h, int32_t i) { return h->params[i].offset; }
int64_t cvae_param_numel(cvae_handle h, int32_t i) { return h->params[i].numel; }
int64_t cvae_workspace_bytes(cvae_handle h, int32_t batch) { return carve(h, batch).total * 4; }
int64_t cvae_bn_state_floats(cvae_handle) { return 2 * 480; }

// float offset of a named saved tensor inside the workspace (tests / debugging); -1 if unknown
int64_t cvae_ws_offset(cvae_handle h, int32_t batch, const char* name) {
    const WsLayout w = carve(h, batch);
    char nm[32];
    for (int l = 0; l < 4; ++l) {
        snprintf(nm, sizeof nm, "y%d", l); if (!strcmp(name, nm)) return w.y[l];
        snprintf(nm, sizeof nm, "a%d", l); if (!strcmp(name, nm)) return w.a[l];
        snprintf(nm, sizeof nm, "d_y%d", l); if (!strcmp(name, nm)) return w.d_y[l];
        snprintf(nm, sizeof nm, "d_a%d", l); if (!strcmp(name, nm)) return w.d_a[l];
        snprintf(nm, sizeof nm, "coef%d", l); if (!strcmp(name, nm)) return w.coef[l];
        snprintf(nm, sizeof nm, "o%d", l); if (!strcmp(name, nm)) return w.o[l];
        snprintf(nm, sizeof nm, "d_o%d", l); if (!strcmp(name, nm)) return w.d_o[l];
    }
    if (!strcmp(name, "zcat")) return w.zcat;
    if (!strcmp(name, "d_zcat")) return w.d_zcat;
    if (!strcmp(name, "h")) return w.h;
    if (!strcmp(name, "d_h")) return w.d_h;
    if (!strcmp(name, "dout4")) return w.dout4;
    if (!strcmp(name, "scratch")) return w.scratch;
    if (!strcmp(name, "ms")) return w.ms;      // the MS-SSIM region: cvae_op_msssim_ws_floats(batch) floats, level fields first, the 832 floats of slab / coef / ticket last
    if (!strcmp(name, "xp")) return h->cfg.precision == 1 ? w.xp : -1;      // packed bf16 frame (precision mode 1)
    return -1;
}

static const int kBnOff[4] = {0, 32, 96, 224};
// the fp64 sync record of the staged entry points (include/cvae.h): points 0..3 = forward blocks 0..3 (S, Q, M per channel;
// point 0 ends with this rank's image count), 4 = the 11 loss sums, 5..8 = backward blocks 3..0 (sum g, sum g*xhat per channel)
static const int64_t kSyncOff[9] = {0, 97, 289, 673, 1441, 1452, 1964, 2220, 2348};
static const int64_t kSyncCnt[9] = {97, 192, 384, 768, 11, 512, 256, 128, 64};
static const int64_t kSyncCount = 96;            // the image count inside point 0
static_assert(2348 + 64 == CVAE_SYNC_DOUBLES, "sync record size");
int cvae_decode(cvae_handle h, int32_t B, const float* zcat, const float* params, float* recon, void* wsv, void* stream);
int cvae_backward_phases(cvae_handle h, int32_t B, const float* x, const float* pred, const float* eps, const float* params,
                         const float* logvar, const float* recon, const float* d_recon, const float* d_mu,
                         const float* d_logvar, void* wsv, float* grads, int32_t phase_mask, void* stream);

#define P_(idx) (params + h->params[(idx)].offset)
#define G_(idx) (grads + h->params[(idx)].offset)
#define RC(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

// ---- the one place a conv family is chosen: layers 1..7 (E2..E4, D0, D1..D3), by cvae_config.precision ----
// The step (FwdCtx, cvae_decode, BwdCtx, hence the staged entry points) and the per-op entry points cvae_op_conv_* reach the launchers
// of these layers only through conv_fwd / conv_dgrad / conv_wgrad and prepare_conv_weights, which read this table.  Precision 2 / 3:
// 3-way split operands on the bf16 MFMA (exact fp32 products, 9 / the 6 leading MFMAs each) for E2..E4 / D0; D1..D3 stay on the fp32
// phase-collapsed kernels, which beat nine bf16 MFMAs per block.  Layers 0 and 8 (E1, D4) are outside on purpose: the step runs their
// fused forms (two-pass E1, packed frame, E1Fuse, fused D4 backward), the per-op entry points the plain ones.
enum ConvFamilyFD { FD_F32, FD_BF16, FD_UP, FD_UP_BF16 };      // forward / input gradient: launch_conv_*, _bf16, _up_*, _up_*_bf16
enum ConvFamilyWG { WG_F32, WG_BF16, WG_SPLIT, WG_UP };        // weight gradient: launch_conv_wgrad, _bf16, _split, launch_conv_up_wgrad
enum WeightForm { W_RAW, W_COLLAPSED, W_PACKED };              // fp32 [25][Cin][Cout]; D1..D3 phase-collapsed; packed bf16 (D1..D3: of the collapsed)
enum FdScratch { SCRATCH_D0_AT_64, SCRATCH_ALWAYS };           // split-K slabs of D0 at 64 x 64 only; every layer
struct ConvRow {
    int precision, first, last;      // key: layers first..last of a handle of this precision
    ConvFamilyFD fd; int mode;       // forward / input gradient; bf16 families: launcher mode 1 = bf16, 3 = x9, 6 = x6
    WeightForm wform;                // the weights that family reads (a weight gradient reads none)
    FdScratch scratch;               // where that family writes scratch (slabs; a per-op call also prepares its weights there)
    ConvFamilyWG wg; int wgArg;      // weight gradient, always with split-K slabs in scratch; WG_SPLIT: 9 / 6 products, WG_UP: the bf16 flag
    int splits() const { return mode == 1 ? 1 : 3; }      // copies of a packed weight
};
static constexpr ConvRow kConvTable[] = {
    {0, 1, 4, FD_F32,     0, W_RAW,       SCRATCH_D0_AT_64, WG_F32,   0},
    {0, 5, 7, FD_UP,      0, W_COLLAPSED, SCRATCH_ALWAYS,   WG_UP,    0},
    {1, 1, 4, FD_BF16,    1, W_PACKED,    SCRATCH_ALWAYS,   WG_BF16,  0},
    {1, 5, 7, FD_UP_BF16, 1, W_PACKED,    SCRATCH_ALWAYS,   WG_UP,    1},
    {2, 1, 4, FD_BF16,    3, W_PACKED,    SCRATCH_ALWAYS,   WG_SPLIT, 9},
    {2, 5, 7, FD_UP,      0, W_COLLAPSED, SCRATCH_ALWAYS,   WG_UP,    0},
    {3, 1, 4, FD_BF16,    6, W_PACKED,    SCRATCH_ALWAYS,   WG_SPLIT, 6},
    {3, 5, 7, FD_UP,      0, W_COLLAPSED, SCRATCH_ALWAYS,   WG_UP,    0},
};
static const ConvRow& conv_row(const cvae_handle_s* h, int layer) {      // layer 1..7: the step's constants, the range cvae_op_conv_* check
    for (const ConvRow& r : kConvTable)
        if (r.precision == h->cfg.precision && layer >= r.first && layer <= r.last) return r;
    abort();
}
static bool fd_uses_scratch(const ConvRow& r, int layer, int width) { return r.scratch == SCRATCH_ALWAYS || (layer == 4 && width == 64); }
static int64_t pack_floats(const cvae_handle_s* h) {      // the packed-weight block: workspace slot wpack, the head of a per-op scratch
    return conv_row(h, 1).wform == W_PACKED ? conv_bf16_pack_floats(conv_row(h, 1).splits()) : 0;
}
// precision 1: activations and activation gradients are bf16 IN HBM (every kernel that touches them is told so)
static bool io_bf16(cvae_handle h) { return h->cfg.precision == 1; }
// raw[l - 1] = the fp32 weights of layer l (null: not given); collapsed[l - 5] and packed (the whole pack block) = where their other forms go
struct ConvWeights { const float* raw[7]; float* collapsed[3]; float* packed; };
static int conv_fwd(cvae_handle h, int layer, int B, const float* in, const ConvWeights& wt, const float* bias, float* out, float* bnpart, float* scratch, hipStream_t st, int* tilesPerPartial) {
    const ConvRow& r = conv_row(h, layer);
    switch (r.fd) {
        case FD_F32: return launch_conv_fwd(layer, h->cfg.width, B, in, wt.raw[layer - 1], bias, out, bnpart, scratch, st);
        case FD_BF16: return launch_conv_fwd_bf16(layer, h->cfg.width, r.mode, B, in, wt.packed, bias, out, bnpart, scratch, st, tilesPerPartial);
        case FD_UP: return launch_conv_up_fwd(layer, h->cfg.width, B, in, wt.collapsed[layer - 5], bias, out, scratch, st);
        case FD_UP_BF16: return launch_conv_up_fwd_bf16(layer, h->cfg.width, r.mode, B, in, wt.packed, bias, out, st);
    }
    return CVAE_EINVAL;
}
static int conv_dgrad(cvae_handle h, int layer, int B, const float* dout, const ConvWeights& wt, const float* mask_src, float* din, float* scratch, hipStream_t st) {
    const ConvRow& r = conv_row(h, layer);
    switch (r.fd) {
        case FD_F32: return launch_conv_dgrad(layer, h->cfg.width, B, dout, wt.raw[layer - 1], mask_src, din, scratch, st);
        case FD_BF16: return launch_conv_dgrad_bf16(layer, h->cfg.width, r.mode, B, dout, wt.packed, din, scratch, st);
        case FD_UP: return launch_conv_up_dgrad(layer, h->cfg.width, B, dout, wt.collapsed[layer - 5], mask_src, din, scratch, st);
        case FD_UP_BF16: return launch_conv_up_dgrad_bf16(layer, h->cfg.width, r.mode, B, dout, wt.packed, mask_src, din, st);
    }
    return CVAE_EINVAL;
}
static int conv_wgrad(cvae_handle h, int layer, int B, const float* in, const float* dout, float* dw, float* dbias, float* scratch, hipStream_t st) {
    const ConvRow& r = conv_row(h, layer);
    switch (r.wg) {
        case WG_F32: return launch_conv_wgrad(layer, h->cfg.width, B, in, dout, dw, dbias, scratch, st);
        case WG_BF16: return launch_conv_wgrad_bf16(layer, h->cfg.width, B, in, dout, dw, dbias, scratch, st);
        case WG_SPLIT: return launch_conv_wgrad_split(layer, h->cfg.width, r.wgArg, B, in, dout, dw, dbias, scratch, st);
        case WG_UP: return launch_conv_up_wgrad(layer, h->cfg.width, B, in, dout, dw, dbias, scratch, st, r.wgArg != 0);
    }
    return CVAE_EINVAL;
}
// The forms the table asks for, of the layers given: 1..4 packed (one launch); 5..7 collapsed (one launch for all three, else one each), then packed (one launch)
static int prepare_conv_weights(cvae_handle h, const ConvWeights& f, hipStream_t st) {
    const ConvRow &enc = conv_row(h, 1), &up_row = conv_row(h, 5);
    if (enc.wform == W_PACKED && (f.raw[0] || f.raw[1] || f.raw[2] || f.raw[3])) RC(launch_pack_w_bf16(f.raw, f.packed, enc.splits(), st));
    const float* const* up = f.raw + 4;
    const int n_up = (up[0] != nullptr) + (up[1] != nullptr) + (up[2] != nullptr);
    if (n_up == 3) RC(launch_collapse_w3(up, f.collapsed, st));
    else for (int i = 0; i < 3; ++i) if (up[i]) RC(launch_collapse_w(5 + i, up[i], f.collapsed[i], st));
    if (n_up == 0 || up_row.wform != W_PACKED) return 0;
    const float* wcs[3] = {up[0] ? f.collapsed[0] : nullptr, up[1] ? f.collapsed[1] : nullptr, up[2] ? f.collapsed[2] : nullptr};      // the packer skips a null layer
    return launch_pack_up_bf16(wcs, f.packed, up_row.splits(), st);
}
// the step's: layers first..last of the parameters, the workspace slots wc[] and wpack (rebuilt every forward)
static ConvWeights step_weights(cvae_handle h, const float* params, float* ws, const WsLayout& w, int first = 1, int last = 7) {
    ConvWeights f{{}, {ws + w.wc[0], ws + w.wc[1], ws + w.wc[2]}, ws + w.wpack};
    for (int l = first; l <= last; ++l) f.raw[l - 1] = l < 4 ? P_(h->enc_w[l]) : P_(h->dec_w[l - 4]);
    return f;
}

static int check(cvae_handle h, int32_t batch, const void* ws) {
    if (!h) { cvae_set_error("null handle"); return CVAE_EINVAL; }
    if (batch < 1 || batch > h->cfg.max_batch) { cvae_set_error("batch %d outside [1, %d]", batch, h->cfg.max_batch); return CVAE_EINVAL; }
    if (!ws) { cvae_set_error("null workspace"); return CVAE_ENOWS; }
    return 0;
}

// One encoder block of the forward in steps: conv (the conv and its BatchNorm partials; bf16 mode, block 0: the
// statistics pass), stats (the statistics: finalized here, or this rank's record for the cross-rank path, whose finish
// turns the summed record into coef) and apply (BatchNorm/pool/activation -> a[l]).
struct FwdCtx {
    cvae_handle h; int B, W, train; const float* x; const float* params; float* bn_state; float* ws; void* wsv; WsLayout w; hipStream_t st;
    int tpp = 1;                 // 128-pixel tiles per BatchNorm partial row, as reported by the conv kernel that ran
    // bf16 mode, block 0: both E1 passes stage the packed bf16 frame (slot xp) that the statistics pass writes while it stays
    // below 2 GiB (conv_route); past that every E1 pass stages the fp32 frame
    float* xp() const { return train && conv_route(1, 0, W, false, B).family == E1_PACKED_FRAME ? ws + w.xp : nullptr; }
    bool two_pass(int l) const { return l == 0 && h->cfg.precision == 1; }
    int conv(int l) {
        tpp = 1;
        if (two_pass(l)) {
            // bf16 mode, block 0: conv (statistics only) -> merged statistics -> conv again with BatchNorm/pool/ReLU in its
            // epilogue (writes a0); bn_pool_act_fwd's read of y0 is replaced by a second read of x
            if (train) RC(launch_e1_fwd(W, B, x, P_(h->enc_w[0]), P_(h->enc_b[0]), nullptr, ws + w.bnpart[0], st, true, 1, nullptr, nullptr, xp()));     // also writes xp
            h->xp_ws = xp() ? wsv : nullptr; h->xp_B = B;
            return 0;
        }
        if (l == 0) { ProbeArm pa(h, 0, 0); RC(launch_e1_fwd(W, B, x, P_(h->enc_w[0]), P_(h->enc_b[0]), ws + w.y[0], ws + w.bnpart[0], st)); }
        else { ProbeArm pa(h, 0, l); RC(conv_fwd(h, l, B, ws + w.a[l - 1], step_weights(h, params, ws, w), P_(h->enc_b[l]), ws + w.y[l], ws + w.bnpart[l], ws + w.scratch, st, &tpp)); }
        return 0;
    }
    int stats(int l, double* sync) {
        if (sync) return launch_bn_fwd_record(l, W, B, ws + w.bnpart[l], ws + w.scratch, st, tpp, sync + kSyncOff[l], l == 0 ? sync + kSyncCount : nullptr);
        return launch_bn_fwd_finalize(l, W, B, ws + w.bnpart[l], P_(h->enc_g[l]), P_(h->enc_be[l]), bn_state + kBnOff[l],
                                      bn_state + 480 + kBnOff[l], ws + w.coef[l], ws + w.scratch, train, st, tpp);
    }
    int finish(int l, const double* sync) {
        return launch_bn_fwd_finish(l, W, sync + kSyncOff[l], sync + kSyncCount, P_(h->enc_g[l]), P_(h->enc_be[l]), bn_state + kBnOff[l],
                                    bn_state + 480 + kBnOff[l], ws + w.coef[l], st);
    }
    int apply(int l) {
        if (two_pass(l)) {
            ProbeArm pa(h, 0, 0);
            // y0 is written only when a channel's gamma is tiny (decided on the device): the fused weight-gradient kernel recomputes it
            return launch_e1_fwd(W, B, x, P_(h->enc_w[0]), P_(h->enc_b[0]), ws + w.y[0], nullptr, st, true, 2, ws + w.coef[0], ws + w.a[0],
                                 xp());                // eval mode (no statistics pass) or no packed frame: E1_POOL_X
        }
        return launch_bn_pool_act_fwd(l, W, B, ws + w.y[l], ws + w.coef[l], ws + w.a[l], st, io_bf16(h));
    }
};

int cvae_forward(cvae_handle h, int32_t B, const float* x, const float* pred, const float* eps, const float* params,
                 float* bn_state, float* mu, float* logvar, float* recon, void* wsv, int32_t train, void* stream) {
    RC(check(h, B, wsv));
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)wsv;
    const WsLayout w = carve(h, B);
    const int W = h->cfg.width;
    RC(prepare_conv_weights(h, step_weights(h, params, ws, w, 1, 4), st));
    FwdCtx f{h, B, W, train, x, params, bn_state, ws, wsv, w, st};
    for (int l = 0; l < 4; ++l) {
        RC(f.conv(l));
        RC(f.stats(l, nullptr));
        RC(f.apply(l));
    }
    RC(launch_fc_fwd(W, B, ws + w.a[3], P_(h->fc_w), P_(h->fc_b), eps, pred, mu, logvar, ws + w.zcat, ws + w.scratch, st, io_bf16(h)));
    if (!recon) return 0;                       // encode only (VariationalEncoder.forward)
    return cvae_decode(h, B, nullptr, params, recon, wsv, stream);
}

// Decoder.forward (vae_nets.py:139-147) from zcat = [z | pred] (B,33); zcat == NULL uses the one
// cvae_forward left in the workspace.
int cvae_decode(cvae_handle h, int32_t B, const float* zcat, const float* params, float* recon, void* wsv, void* stream) {
    RC(check(h, B, wsv));
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)wsv;
    const WsLayout w = carve(h, B);
    const int W = h->cfg.width;
    if (zcat) {
        hipError_t e = hipMemcpyAsync(ws + w.zcat, zcat, (size_t)B * 33 * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) { cvae_set_error("cvae_decode: copy failed: %s", hipGetErrorString(e)); return (int)e; }
    }
    RC(launch_decin_fwd(W, B, ws + w.zcat, P_(h->di_w), P_(h->di_b), ws + w.h, st, io_bf16(h)));
    // Upsample -> Conv of D1..D3 runs at the low resolution with phase-collapsed weights (conv_up.hip); a stand-alone decode
    // (cvae_forward did not run) prepares layers 1..4 as well
    RC(prepare_conv_weights(h, step_weights(h, params, ws, w, zcat ? 1 : 5, 7), st));
    for (int i = 0; i < 4; ++i) {
        ProbeArm pa(h, 0, 4 + i);
        RC(conv_fwd(h, 4 + i, B, i == 0 ? ws + w.h : ws + w.o[i - 1], step_weights(h, params, ws, w), P_(h->dec_b[i]), ws + w.o[i], nullptr,
                    ws + w.scratch, st, nullptr));
    }
    { ProbeArm pa(h, 0, 8); RC(launch_d4_fwd(W, B, ws + w.o[3], P_(h->dec_w[4]), P_(h->dec_b[4]), recon, st, io_bf16(h))); }
    return 0;
}

int cvae_loss(cvae_handle h, int32_t B, const float* x, const float* mu, const float* logvar, const float* recon,
              void* wsv, float* scalars, float* d_recon, float* d_mu, float* d_logvar, void* stream) {
    RC(check(h, B, wsv));
    if ((d_recon == nullptr) != (d_mu == nullptr) || (d_mu == nullptr) != (d_logvar == nullptr)) {
        cvae_set_error("cvae_loss: d_recon, d_mu, d_logvar must be all set or all null");
        return CVAE_EINVAL;
    }
    float* ws = (float*)wsv;
    const WsLayout w = carve(h, B);
    ProbeArm pa(h, 3, 4);            // id 31: the level-0 tile kernel
    return launch_msssim(h->cfg.width, B, recon, x, mu, logvar, ws + w.ms, scalars, d_recon, d_mu, d_logvar, (hipStream_t)stream);
}

// cvae_loss under a caller-chosen objective.  The reference objective {1, 0, 0.001f, 0} takes exactly cvae_loss's launches.
int cvae_loss_obj(cvae_handle h, int32_t B, const float* x, const float* mu, const float* logvar, const float* recon,
                  void* wsv, const cvae_objective* obj, float* scalars, float* d_recon, float* d_mu, float* d_logvar, void* stream) {
    RC(check(h, B, wsv));
    if (!obj) { cvae_set_error("cvae_loss_obj: null objective"); return CVAE_EINVAL; }
    if (!x || !mu || !logvar || !recon || !scalars) { cvae_set_error("cvae_loss_obj: null tensor"); return CVAE_EINVAL; }
    if ((d_recon == nullptr) != (d_mu == nullptr) || (d_mu == nullptr) != (d_logvar == nullptr)) {
        cvae_set_error("cvae_loss_obj: d_recon, d_mu, d_logvar must be all set or all null");
        return CVAE_EINVAL;
    }
    if ((((uintptr_t)x | (uintptr_t)recon | (uintptr_t)d_recon) & 15) != 0) {
        cvae_set_error("cvae_loss_obj: x, recon and d_recon must be 16-byte aligned");
        return CVAE_EINVAL;
    }
    const float wts[3] = {obj->msssim_weight, obj->mse_weight, obj->kld_weight};
    for (int i = 0; i < 3; ++i)
        if (!(wts[i] >= 0.0f) || !(wts[i] <= 3.402823466e38f)) {      // NaN fails both comparisons
            cvae_set_error("cvae_loss_obj: weight %d is %g: every weight must be finite and >= 0", i, (double)wts[i]);
            return CVAE_EINVAL;
        }
    if (!((double)obj->msssim_weight + (double)obj->mse_weight > 0.0)) {      // fp64: two large finite weights do not overflow the test
        cvae_set_error("cvae_loss_obj: msssim_weight + mse_weight must be > 0 (no reconstruction term)");
        return CVAE_EINVAL;
    }
    if (obj->msssim_grad != CVAE_MSGRAD_REFERENCE && obj->msssim_grad != CVAE_MSGRAD_USED) {
        cvae_set_error("cvae_loss_obj: msssim_grad %d is neither CVAE_MSGRAD_REFERENCE nor CVAE_MSGRAD_USED", obj->msssim_grad);
        return CVAE_EINVAL;
    }
    float* ws = (float*)wsv;
    const WsLayout w = carve(h, B);
    const LossObjective o{obj->msssim_weight, obj->mse_weight, obj->kld_weight, obj->msssim_grad == CVAE_MSGRAD_USED ? 1 : 0};
    ProbeArm pa(h, 3, 4);            // id 31: the level-0 tile kernel (not launched at msssim_weight 0)
    return launch_msssim(h->cfg.width, B, recon, x, mu, logvar, ws + w.ms, scalars, d_recon, d_mu, d_logvar, (hipStream_t)stream,
                         0, nullptr, nullptr, &o);
}

// ---- per-image scores and the pooled record of a held-out set (score.hip) ----
int32_t cvae_score_cols(void) { return CVAE_SCORE_COLS; }
int64_t cvae_score_state_bytes(void) { return score_state_bytes(); }
int cvae_score_init(cvae_handle h, void* state, void* stream) {
    if (!h || !state || ((uintptr_t)state & 7)) { cvae_set_error("cvae_score_init: bad handle, null or misaligned state"); return CVAE_EINVAL; }
    return launch_score_init(state, (hipStream_t)stream);
}
int cvae_score(cvae_handle h, int32_t B, const float* x, const float* mu, const float* logvar, const float* recon, void* wsv,
               float* per_image, void* state, void* stream) {
    RC(check(h, B, wsv));
    if (!x || !mu || !logvar || !recon) { cvae_set_error("cvae_score: null tensor"); return CVAE_EINVAL; }
    if (!per_image && !state) { cvae_set_error("cvae_score: per_image and state are both null: nothing to write"); return CVAE_EINVAL; }
    if (((uintptr_t)x & 15) || ((uintptr_t)recon & 15) || ((uintptr_t)state & 7)) {
        cvae_set_error("cvae_score: x and recon must be 16-byte aligned, state 8-byte aligned"); return CVAE_EINVAL;
    }
    float* ws = (float*)wsv;
    const WsLayout w = carve(h, B);
    return launch_score(h->cfg.width, B, x, mu, logvar, recon, ws + w.ms, per_image, state, (hipStream_t)stream);
}
int cvae_score_finish(cvae_handle h, int32_t width, void* state, float* scalars, void* stream) {
    if (!h || !state || !scalars || ((uintptr_t)state & 7)) { cvae_set_error("cvae_score_finish: bad handle, null pointer or misaligned state"); return CVAE_EINVAL; }
    if (width != 64 && width != 128) { cvae_set_error("cvae_score_finish: width %d unsupported", width); return CVAE_EINVAL; }
    return launch_score_finish(width, state, scalars, (hipStream_t)stream);
}

// ---- pooled latent statistics of a set (latent_stats.hip) ----
int64_t cvae_latent_stats_state_bytes(void) { return latent_stats_state_bytes(); }
int64_t cvae_latent_stats_scratch_bytes(cvae_handle h, int32_t B) {
    const int64_t n = h ? latent_stats_scratch_bytes(B) : -1;
    if (n < 0) cvae_set_error("cvae_latent_stats_scratch_bytes: bad handle, or batch %d outside 1..2^24", B);
    return n < 0 ? -1 : n;
}
int32_t cvae_latent_stats_plan(int32_t B, int32_t num_cus, int32_t* out) {
    int plan[3];
    if (!out || latent_stats_plan(B, num_cus, plan) != 0) {
        cvae_set_error("cvae_latent_stats_plan: batch %d outside 1..2^24, compute units %d below 1, or null pointer", B, num_cus);
        return CVAE_EINVAL;
    }
    for (int i = 0; i < 3; ++i) out[i] = plan[i];
    return 0;
}
int cvae_latent_stats(cvae_handle h, int32_t B, const float* mu, const float* logvar, const float* pred, void* state, float* kl_rows,
                      void* scratch, void* stream, uint32_t flags) {
    if (!h || !mu || !logvar || !pred || !state || !scratch) { cvae_set_error("cvae_latent_stats: bad handle or null pointer"); return CVAE_EINVAL; }
    if (flags != 0) { cvae_set_error("cvae_latent_stats: flags = %u must be 0", (unsigned)flags); return CVAE_EINVAL; }
    if (latent_stats_scratch_bytes(B) < 0) { cvae_set_error("cvae_latent_stats: batch %d outside 1..2^24", B); return CVAE_EINVAL; }
    if ((((uintptr_t)mu | (uintptr_t)logvar | (uintptr_t)pred | (uintptr_t)kl_rows) & 3) || (((uintptr_t)state | (uintptr_t)scratch) & 7)) {
        cvae_set_error("cvae_latent_stats: mu, logvar, pred and kl_rows must be 4-byte aligned, state and scratch 8-byte aligned"); return CVAE_EINVAL;
    }
    return launch_latent_stats(B, mu, logvar, pred, state, kl_rows, scratch, (hipStream_t)stream);
}
int cvae_recon_response(cvae_handle h, int32_t n_images, int32_t n_variants, const float* recon_base, const float* recon_var, float* out,
                        void* stream, uint32_t flags) {
    if (!h || !recon_base || !recon_var || !out) { cvae_set_error("cvae_recon_response: bad handle or null pointer"); return CVAE_EINVAL; }
    if (flags != 0) { cvae_set_error("cvae_recon_response: flags = %u must be 0", (unsigned)flags); return CVAE_EINVAL; }
    if (n_images < 1 || n_variants < 1 || (int64_t)n_images * n_variants >= ((int64_t)1 << 31)) {
        cvae_set_error("cvae_recon_response: %d images x %d variants: both at least 1, the product below 2^31", n_images, n_variants); return CVAE_EINVAL;
    }
    if ((((uintptr_t)recon_base | (uintptr_t)recon_var) & 15) || ((uintptr_t)out & 3)) {
        cvae_set_error("cvae_recon_response: recon_base and recon_var must be 16-byte aligned, out 4-byte aligned"); return CVAE_EINVAL;
    }
    return launch_recon_response(h->cfg.width, (int64_t)n_images * n_variants, n_variants, recon_base, recon_var, out, (hipStream_t)stream);
}

int cvae_backward(cvae_handle h, int32_t B, const float* x, const float* pred, const float* eps, const float* params,
                  const float* logvar, const float* recon, const float* d_recon, const float* d_mu,
                  const float* d_logvar, void* wsv, float* grads, void* stream) {
    return cvae_backward_phases(h, B, x, pred, eps, params, logvar, recon, d_recon, d_mu, d_logvar, wsv, grads, 7, stream);
}

// Gradient buckets in the order backward completes them (for bucketed all-reduce overlapped with the
// rest of backward): phase 0 = decoder + decoder_input, 1 = fc_mu|fc_var + encoder block 3,
// 2 = encoder blocks 2..0.  Each bucket is one contiguous range of the flat gradient buffer.
int cvae_grad_bucket(cvae_handle h, int32_t phase, int64_t* offset, int64_t* numel) {
    if (!h || !offset || !numel || phase < 0 || phase > 2) { cvae_set_error("cvae_grad_bucket: bad argument"); return CVAE_EINVAL; }
    const int64_t enc3 = h->params[h->enc_w[3]].offset, dec0 = h->params[h->dec_w[0]].offset;
    if (phase == 0) { *offset = dec0; *numel = h->param_total - dec0; }
    else if (phase == 1) { *offset = enc3; *numel = dec0 - enc3; }
    else { *offset = 0; *numel = enc3; }
    return 0;
}

#define HIPRC(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { cvae_set_error("%s: %s", #call, hipGetErrorString(e_)); return (int)e_; } } while (0)
// The backward in pieces shared by cvae_backward_phases and the staged entry points.  cfg.overlap_wgrad != 0: weight-gradient
// work on a lower-priority side stream (bit-identical results; round 3: +1.5 % in bf16 mode at B = 2048, -3 % in fp32 mode at
// B = 256); default: everything in order on the caller's stream.
struct BwdCtx {
    cvae_handle h; int B, W; const float* x; const float* eps; const float* params; const float* logvar; const float* recon;
    const float* d_recon; const float* d_mu; const float* d_logvar; float* ws; float* grads; WsLayout w; hipStream_t st;
    bool overlap = false; hipStream_t sd = nullptr; float* sc = nullptr; float* scw = nullptr;
    int init() {
        sc = ws + w.scratch; scw = ws + w.scratch_w;
        overlap = h->cfg.overlap_wgrad != 0;
        if (overlap) RC(ensure_streams(h));
        sd = overlap ? h->side : st;
        return 0;
    }
    // `ready k` = the gradient a weight-gradient kernel needs exists on the main stream; the side
    // stream picks it up from there, so dW/db never delay the dgrad chain.
    int fork(int idx) {
        if (!overlap) return 0;
        HIPRC(hipEventRecord(h->ev_ready[idx], st));
        HIPRC(hipStreamWaitEvent(sd, h->ev_ready[idx], 0));
        return 0;
    }
    int join() {                                        // side-stream work so far is complete on the caller's stream
        if (!overlap) return 0;
        HIPRC(hipEventRecord(h->ev_side, h->side));
        HIPRC(hipStreamWaitEvent(st, h->ev_side, 0));
        return 0;
    }
    int decoder() {                                     // decoder, last layer first, then the latent (phase 0)
        { ProbeArm pa(h, 1, 8);
          RC(launch_d4_bwd(W, B, ws + w.o[3], d_recon, recon, P_(h->dec_w[4]), ws + w.dout4, ws + w.d_o[3],
                           G_(h->dec_w[4]), G_(h->dec_b[4]), sc, st, io_bf16(h))); }
        for (int i = 3; i >= 0; --i) {
            const int l = 4 + i;
            const float* in = i == 0 ? ws + w.h : ws + w.o[i - 1];
            RC(fork(3 - i));
            { ProbeArm pa(h, 2, l); RC(conv_wgrad(h, l, B, in, ws + w.d_o[i], G_(h->dec_w[i]), G_(h->dec_b[i]), scw, sd)); }
            { ProbeArm pa(h, 1, l);      // D1..D3 mask with the ReLU of their input o[i - 1]
              RC(conv_dgrad(h, l, B, ws + w.d_o[i], step_weights(h, params, ws, w), i == 0 ? nullptr : in, i == 0 ? ws + w.d_h : ws + w.d_o[i - 1], sc, st)); }
        }
        RC(launch_decin_bwd(W, B, ws + w.zcat, ws + w.d_h, P_(h->di_w), G_(h->di_w), G_(h->di_b), ws + w.d_zcat, sc, st, io_bf16(h)));
        return join();
    }
    int fc() {
        return launch_fc_bwd(W, B, ws + w.a[3], P_(h->fc_w), ws + w.d_zcat, eps, logvar, d_mu, d_logvar, G_(h->fc_w),
                             G_(h->fc_b), ws + w.d_a[3], sc, st, io_bf16(h));
    }
    // BatchNorm/pool/activation backward of block l: stage 0 whole, 1 statistics -> record `rec`, 2 finish from the summed
    // record + apply.  Block 0: only the statistics run here; E1's weight-gradient kernel applies the BatchNorm/pool/ReLU
    // backward while it stages its tiles (there is no d_y[0]: nothing else would read it)
    int bn(int l, int stage, double* rec, const double* count) {
        ProbeArm pa(h, 3, l);
        return launch_bn_pool_act_bwd(l, W, B, ws + w.y[l], ws + w.a[l], ws + w.d_a[l], ws + w.coef[l], P_(h->enc_g[l]),
                                      l == 0 ? nullptr : ws + w.d_y[l], G_(h->enc_g[l]), G_(h->enc_be[l]), nullptr, sc, st, io_bf16(h),
                                      stage, rec, count);
    }
    int block_grads(int l) {                            // weight (side stream) and input gradients of block l, after bn(l)
        RC(fork(7 - l));
        if (l == 0) {
            const float* fu[7] = {ws + w.y[0], ws + w.a[0], ws + w.d_a[0], ws + w.coef[0], bn_bwd_bcoef(0, W, B, sc),
                                  P_(h->enc_w[0]), P_(h->enc_b[0])};
            ProbeArm pa(h, 2, 0);
            return launch_e1_wgrad(W, B, x, nullptr, G_(h->enc_w[0]), G_(h->enc_b[0]), scw, sd, h->cfg.precision == 1, fu,
                                   (h->cfg.precision == 1 && h->xp_ws == (const void*)ws && h->xp_B == B &&
                                    conv_route(1, 0, W, false, B).family == E1_PACKED_FRAME) ? ws + w.xp : nullptr);
        }
        { ProbeArm pa(h, 2, l); RC(conv_wgrad(h, l, B, ws + w.a[l - 1], ws + w.d_y[l], G_(h->enc_w[l]), G_(h->enc_b[l]), scw, sd)); }
        ProbeArm pa(h, 1, l);
        return conv_dgrad(h, l, B, ws + w.d_y[l], step_weights(h, params, ws, w), nullptr, ws + w.d_a[l - 1], sc, st);
    }
};

int cvae_backward_phases(cvae_handle h, int32_t B, const float* x, const float* pred, const float* eps, const float* params,
                         const float* logvar, const float* recon, const float* d_recon, const float* d_mu,
                         const float* d_logvar, void* wsv, float* grads, int32_t phase_mask, void* stream) {
    (void)pred;
    RC(check(h, B, wsv));
    if ((phase_mask & ~15) != 0 || (phase_mask & 7) == 0) { cvae_set_error("cvae_backward_phases: phase_mask %d (bits 0..2 = phases, bit 3 = zero the alignment padding)", phase_mask); return CVAE_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    if (phase_mask & 8) {                               // caller handed an uninitialised gradient buffer
        PadGaps gaps{};                                 // 32 gaps per launch; as many launches as the parameter list needs
        for (const ParamEntry& p : h->params) {
            const int64_t pad = align_up(p.numel, 64) - p.numel;
            if (pad <= 0) continue;
            gaps.off[gaps.n] = p.offset + p.numel; gaps.len[gaps.n] = (int)pad; gaps.n++;
            if (gaps.n == 32) { RC(launch_zero_gaps(grads, gaps, st)); gaps.n = 0; }
        }
        RC(launch_zero_gaps(grads, gaps, st));
    }
    BwdCtx b{h, B, h->cfg.width, x, eps, params, logvar, recon, d_recon, d_mu, d_logvar, (float*)wsv, grads, carve(h, B), st};
    RC(b.init());
    if (phase_mask & 1) RC(b.decoder());
    if (phase_mask & 2) RC(b.fc());
    // encoder
    for (int l = 3; l >= 0; --l) {
        if (!(phase_mask & (l == 3 ? 2 : 4))) continue;
        RC(b.bn(l, 0, nullptr, nullptr));
        RC(b.block_grads(l));
        if (l == 3 || l == 0) RC(b.join());             // end of phase 1 / phase 2
    }
    return 0;
}

// ---- staged step for cross-rank BatchNorm / loss statistics (include/cvae.h: cvae_sync_slot and the *_stage calls) ----
int cvae_sync_slot(int32_t point, int64_t* offset, int64_t* count) {
    if (point < 0 || point > 8 || !offset || !count) { cvae_set_error("cvae_sync_slot: point %d outside [0, 8] or null output", point); return CVAE_EINVAL; }
    *offset = kSyncOff[point]; *count = kSyncCnt[point];
    return 0;
}

static const char* kPassName[3] = {"cvae_forward_stage", "cvae_loss_stage", "cvae_backward_stage"};
static const int kPassStages[3] = {5, 2, 5};
// host-only checks of a staged call, before any device access: stage range, record, and the order of the step
static int sync_check(cvae_handle h, int pass, int32_t B, const void* ws, const double* rec, int32_t stage) {
    RC(check(h, B, ws));
    if (!rec) { cvae_set_error("%s: null sync record", kPassName[pass]); return CVAE_EINVAL; }
    if (stage < 0 || stage >= kPassStages[pass]) { cvae_set_error("%s: stage %d outside [0, %d]", kPassName[pass], stage, kPassStages[pass] - 1); return CVAE_EINVAL; }
    if (pass == 0 && stage == 0) return 0;              // a new step may always start
    const auto& s = h->sync;
    if (s.pass != pass || s.next != stage || s.ws != ws || s.B != B || s.rec != rec) {
        cvae_set_error("%s: stage %d out of order (the handle expects %s stage %d%s)", kPassName[pass], stage, kPassName[s.pass], s.next,
                       s.ws ? " on the workspace, batch and record of the step in progress" : "; a step starts with cvae_forward_stage 0");
        return CVAE_EINVAL;
    }
    return 0;
}
// after a stage: the next one the handle accepts (rc != 0: none but a new step)
static int sync_advance(cvae_handle h, int pass, int32_t B, const void* ws, const double* rec, int32_t stage, int rc) {
    auto& s = h->sync;
    if (rc) { s.pass = 0; s.next = 0; s.ws = nullptr; s.rec = nullptr; s.B = 0; return rc; }
    s.ws = ws; s.B = B; s.rec = rec;
    if (stage + 1 < kPassStages[pass]) { s.pass = pass; s.next = stage + 1; }
    else if (pass < 2) { s.pass = pass + 1; s.next = 0; }
    else { s.pass = 0; s.next = 0; s.ws = nullptr; s.rec = nullptr; s.B = 0; }
    return 0;
}

static int forward_stage(cvae_handle h, int32_t B, const float* x, const float* pred, const float* eps, const float* params,
                         float* bn_state, float* mu, float* logvar, float* recon, void* wsv, double* sync, int32_t k, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)wsv;
    const WsLayout w = carve(h, B);
    const int W = h->cfg.width;
    FwdCtx f{h, B, W, 1, x, params, bn_state, ws, wsv, w, st};
    if (k == 0) RC(prepare_conv_weights(h, step_weights(h, params, ws, w, 1, 4), st));
    if (k > 0) {                                        // block k-1 from the summed record
        RC(f.finish(k - 1, sync));
        RC(f.apply(k - 1));
    }
    if (k < 4) {
        RC(f.conv(k));
        return f.stats(k, sync);
    }
    RC(launch_fc_fwd(W, B, ws + w.a[3], P_(h->fc_w), P_(h->fc_b), eps, pred, mu, logvar, ws + w.zcat, ws + w.scratch, st, io_bf16(h)));
    if (!recon) return 0;
    return cvae_decode(h, B, nullptr, params, recon, wsv, stream);
}

int cvae_forward_stage(cvae_handle h, int32_t B, const float* x, const float* pred, const float* eps, const float* params,
                       float* bn_state, float* mu, float* logvar, float* recon, void* wsv, int32_t train, double* sync,
                       int32_t stage, void* stream) {
    RC(sync_check(h, 0, B, wsv, sync, stage));
    if (train != 1) { cvae_set_error("cvae_forward_stage: train must be 1 (eval mode uses the running statistics: cvae_forward)"); return CVAE_EINVAL; }
    const int rc = forward_stage(h, B, x, pred, eps, params, bn_state, mu, logvar, recon, wsv, sync, stage, stream);
    return sync_advance(h, 0, B, wsv, sync, stage, rc);
}

int cvae_loss_stage(cvae_handle h, int32_t B, const float* x, const float* mu, const float* logvar, const float* recon,
                    void* wsv, float* scalars, float* d_recon, float* d_mu, float* d_logvar, double* sync, int32_t stage,
                    void* stream) {
    RC(sync_check(h, 1, B, wsv, sync, stage));
    if ((d_recon == nullptr) != (d_mu == nullptr) || (d_mu == nullptr) != (d_logvar == nullptr)) {
        cvae_set_error("cvae_loss_stage: d_recon, d_mu, d_logvar must be all set or all null");
        return CVAE_EINVAL;
    }
    float* ws = (float*)wsv;
    const WsLayout w = carve(h, B);
    int rc;
    { ProbeArm pa(h, 3, 4);
      rc = launch_msssim(h->cfg.width, B, recon, x, mu, logvar, ws + w.ms, scalars, d_recon, d_mu, d_logvar, (hipStream_t)stream,
                         stage + 1, sync + kSyncOff[4], sync + kSyncCount); }
    return sync_advance(h, 1, B, wsv, sync, stage, rc);
}

static int backward_stage(cvae_handle h, int32_t B, const float* x, const float* eps, const float* params, const float* logvar,
                          const float* recon, const float* d_recon, const float* d_mu, const float* d_logvar, void* wsv,
                          float* grads, double* sync, int32_t k, void* stream) {
    BwdCtx b{h, B, h->cfg.width, x, eps, params, logvar, recon, d_recon, d_mu, d_logvar, (float*)wsv, grads, carve(h, B), (hipStream_t)stream};
    RC(b.init());
    const int l = 4 - k;                                // the block stage k applies (k >= 1); its statistics are point 8 - l
    if (k == 0) {
        RC(b.decoder());
        RC(b.fc());
    } else {
        RC(b.bn(l, 2, sync + kSyncOff[8 - l], sync + kSyncCount));
        RC(b.block_grads(l));
    }
    if (k < 4) RC(b.bn(3 - k, 1, sync + kSyncOff[5 + k], nullptr));      // the next block's statistics -> point 5 + k
    return b.join();
}

int cvae_backward_stage(cvae_handle h, int32_t B, const float* x, const float* pred, const float* eps, const float* params,
                        const float* logvar, const float* recon, const float* d_recon, const float* d_mu,
                        const float* d_logvar, void* wsv, float* grads, double* sync, int32_t stage, void* stream) {
    (void)pred;
    RC(sync_check(h, 2, B, wsv, sync, stage));
    const int rc = backward_stage(h, B, x, eps, params, logvar, recon, d_recon, d_mu, d_logvar, wsv, grads, sync, stage, stream);
    return sync_advance(h, 2, B, wsv, sync, stage, rc);
}
#undef HIPRC

int cvae_adam_step(cvae_handle h, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                   int32_t step, float lr, float beta1, float beta2, float eps, float grad_scale, void* stream) {
    if (!h || step < 1) { cvae_set_error("cvae_adam_step: bad handle/step"); return CVAE_EINVAL; }
    return launch_adam(params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, grad_scale, (hipStream_t)stream);
}

int64_t cvae_guard_state_bytes(void) { return guard_state_bytes(); }
int cvae_guard_init(cvae_handle h, void* state, int64_t applied, int64_t skipped, void* stream) {
    if (!h || !state || applied < 0 || skipped < 0) { cvae_set_error("cvae_guard_init: bad handle, null state or negative counter"); return CVAE_EINVAL; }
    return launch_guard_init(state, applied, skipped, (hipStream_t)stream);
}
int cvae_grad_stats(cvae_handle h, const float* grads, int64_t n, float grad_scale, float max_norm, int32_t skip_nonfinite,
                    float lr, float beta1, float beta2, void* state, void* stream) {
    if (!h || !grads || !state) { cvae_set_error("cvae_grad_stats: bad handle or null pointer"); return CVAE_EINVAL; }
    if (n < 0 || n % 4 != 0) { cvae_set_error("cvae_grad_stats: n = %lld must be a non-negative multiple of 4", (long long)n); return CVAE_EINVAL; }
    if (!(max_norm > 0.f)) { cvae_set_error("cvae_grad_stats: max_norm = %g must be positive (+inf = no clipping)", (double)max_norm); return CVAE_EINVAL; }
    return launch_grad_stats(grads, n, grad_scale, max_norm, skip_nonfinite != 0, lr, beta1, beta2, state, (hipStream_t)stream);
}
int cvae_adam_step_guarded(cvae_handle h, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                           float eps, const void* state, void* stream) {
    if (!h || !params || !grads || !exp_avg || !exp_avg_sq || !state) { cvae_set_error("cvae_adam_step_guarded: bad handle or null pointer"); return CVAE_EINVAL; }
    if (n < 0 || n % 4 != 0) { cvae_set_error("cvae_adam_step_guarded: n = %lld must be a non-negative multiple of 4", (long long)n); return CVAE_EINVAL; }
    return launch_adam_guarded(params, grads, exp_avg, exp_avg_sq, n, eps, state, (hipStream_t)stream);
}

// the checks the two _opt entries share (include/cvae.h); `who` names the entry in the message.  Host values only.
static int opt_check(const char* who, int64_t n, const cvae_opt_args* opt, const float* ema, const float* aux, const float* aux_ema,
                     int32_t n_aux) {
    if (!opt) { cvae_set_error("%s: opt is null", who); return CVAE_EINVAL; }
    if (n < 0 || n % 4 != 0) { cvae_set_error("%s: n = %lld must be a non-negative multiple of 4", who, (long long)n); return CVAE_EINVAL; }
    if (opt->n_ranges < 0 || opt->n_ranges > CVAE_OPT_MAX_RANGES) {
        cvae_set_error("%s: n_ranges = %d outside 0..%d", who, (int)opt->n_ranges, CVAE_OPT_MAX_RANGES); return CVAE_EINVAL;
    }
    int64_t prev = 0;
    for (int k = 0; k < opt->n_ranges; ++k) {
        const int64_t b = opt->begin[k], e = opt->end[k];
        if (b >= e || b < prev || e > n) {
            cvae_set_error("%s: range %d = [%lld, %lld): ranges must be non-empty, ascending, disjoint and within [0, n = %lld)", who, k,
                           (long long)b, (long long)e, (long long)n);
            return CVAE_EINVAL;
        }
        prev = e;
    }
    if (!(opt->decay_mul > 0.f && opt->decay_mul <= 1.f)) { cvae_set_error("%s: decay_mul = %g outside (0, 1]", who, (double)opt->decay_mul); return CVAE_EINVAL; }
    if (ema && !(opt->ema_omd >= 0.f && opt->ema_omd <= 1.f)) { cvae_set_error("%s: ema_omd = %g outside [0, 1]", who, (double)opt->ema_omd); return CVAE_EINVAL; }
    if (n_aux < 0 || n_aux > 4096) { cvae_set_error("%s: n_aux = %d outside 0..4096", who, (int)n_aux); return CVAE_EINVAL; }
    if (n_aux > 0 && (!aux || !aux_ema)) { cvae_set_error("%s: n_aux = %d with a null aux or aux_ema", who, (int)n_aux); return CVAE_EINVAL; }
    if ((n_aux > 0 || aux_ema) && !ema) { cvae_set_error("%s: aux_ema without ema", who); return CVAE_EINVAL; }
    return CVAE_OK;
}
int cvae_adam_step_opt(cvae_handle h, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                       int32_t step, float lr, float beta1, float beta2, float eps, float grad_scale, const cvae_opt_args* opt,
                       float* ema, float* aux, float* aux_ema, int32_t n_aux, void* stream) {
    if (!h || !params || !grads || !exp_avg || !exp_avg_sq || step < 1) { cvae_set_error("cvae_adam_step_opt: bad handle, null pointer or step < 1"); return CVAE_EINVAL; }
    RC(opt_check("cvae_adam_step_opt", n, opt, ema, aux, aux_ema, n_aux));
    return launch_adam_opt(params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, grad_scale, opt, ema, aux, aux_ema, n_aux,
                           (hipStream_t)stream);
}
int cvae_adam_step_guarded_opt(cvae_handle h, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                               float eps, const void* state, const cvae_opt_args* opt, float* ema, float* aux, float* aux_ema,
                               int32_t n_aux, void* stream) {
    if (!h || !params || !grads || !exp_avg || !exp_avg_sq || !state) { cvae_set_error("cvae_adam_step_guarded_opt: bad handle or null pointer"); return CVAE_EINVAL; }
    RC(opt_check("cvae_adam_step_guarded_opt", n, opt, ema, aux, aux_ema, n_aux));
    return launch_adam_guarded_opt(params, grads, exp_avg, exp_avg_sq, n, eps, state, opt, ema, aux, aux_ema, n_aux, (hipStream_t)stream);
}

// ---- the training trace (include/cvae.h; trace.hip): every check on host values, before any device access ----
int cvae_trace_push(cvae_handle h, void* ring, int64_t capacity, int64_t step, float lr, const float* loss_scalars, int32_t n_scalars,
                    const void* guard_state_or_null, void* stream) {
    if (!h || !ring || !loss_scalars) { cvae_set_error("cvae_trace_push: bad handle or null pointer"); return CVAE_EINVAL; }
    if (capacity < 1 || step < 1) { cvae_set_error("cvae_trace_push: capacity = %lld and step = %lld must be at least 1", (long long)capacity, (long long)step); return CVAE_EINVAL; }
    if (n_scalars < 0 || n_scalars > CVAE_TRACE_MAX_SCALARS) { cvae_set_error("cvae_trace_push: n_scalars = %d outside 0..%d", (int)n_scalars, CVAE_TRACE_MAX_SCALARS); return CVAE_EINVAL; }
    return launch_trace_push(ring, capacity, step, lr, loss_scalars, n_scalars, guard_state_or_null, (hipStream_t)stream);
}
int cvae_tensor_stats(cvae_handle h, const float* params, const float* grads, const float* exp_avg, const float* exp_avg_sq, int64_t n,
                      int32_t n_tensors, const int64_t* begin, const int64_t* end, int64_t step, float lr, float beta1, float beta2,
                      float eps, float grad_scale, const void* guard_state_or_null, cvae_tensor_stat* out, void* scratch, void* stream) {
    if (!h || !params || !grads || !exp_avg || !exp_avg_sq || !begin || !end || !out || !scratch) {
        cvae_set_error("cvae_tensor_stats: bad handle or null pointer"); return CVAE_EINVAL;
    }
    if (n < 0 || step < 1) { cvae_set_error("cvae_tensor_stats: n = %lld must not be negative and step = %lld at least 1", (long long)n, (long long)step); return CVAE_EINVAL; }
    return launch_tensor_stats(params, grads, exp_avg, exp_avg_sq, n, n_tensors, begin, end, step, lr, beta1, beta2, eps, grad_scale,
                               guard_state_or_null, out, scratch, (hipStream_t)stream);
}
int64_t cvae_tensor_stats_scratch_bytes(int32_t n_tensors, const int64_t* begin, const int64_t* end) {
    return tensor_stats_scratch_bytes(n_tensors, begin, end);
}
int cvae_tensor_stats_plan(int32_t n_tensors, const int64_t* begin, const int64_t* end, int32_t* chunk, int32_t* items, int32_t* grid) {
    if (!chunk || !items || !grid) { cvae_set_error("cvae_tensor_stats_plan: null output"); return CVAE_EINVAL; }
    return tensor_stats_plan(n_tensors, begin, end, chunk, items, grid);
}

int cvae_grads_to_bf16(cvae_handle h, const float* grads, void* out_bf16, int64_t n, void* stream) {
    if (h && n == 0) return 0;                       // empty range (its pointers may be null): nothing to do
    if (!h || !grads || !out_bf16 || n < 0) { cvae_set_error("cvae_grads_to_bf16: bad argument"); return CVAE_EINVAL; }
    return launch_grads_bf16(grads, out_bf16, nullptr, n, (hipStream_t)stream);
}
int cvae_grads_from_bf16(cvae_handle h, const void* in_bf16, float* grads, int64_t n, void* stream) {
    if (h && n == 0) return 0;
    if (!h || !grads || !in_bf16 || n < 0) { cvae_set_error("cvae_grads_from_bf16: bad argument"); return CVAE_EINVAL; }
    return launch_grads_bf16(nullptr, const_cast<void*>(in_bf16), grads, n, (hipStream_t)stream);
}

// d_* (out) = d_* (in) * gscale[0]: total_loss.backward()'s incoming factor applied to the three loss
// gradients cvae_loss wrote, one launch, gscale a device scalar (no host read)
int cvae_scale_loss_grads(cvae_handle h, int32_t B, const float* gscale, const float* d_recon, const float* d_mu,
                          const float* d_logvar, float* d_recon_out, float* d_mu_out, float* d_logvar_out, void* stream) {
    if (!h || B < 1 || !gscale) { cvae_set_error("cvae_scale_loss_grads: bad argument"); return CVAE_EINVAL; }
    const int W = h->cfg.width;
    Scale3 a{gscale, {d_recon, d_mu, d_logvar}, {d_recon_out, d_mu_out, d_logvar_out}, {(int64_t)B * 3 * W * W, (int64_t)B * 32, (int64_t)B * 32}};
    return launch_scale3(a, (hipStream_t)stream);
}

// ---- critic inference + uint8 frame pre-processing (vae.py:46-50) ----
int32_t cvae_critic_param_count(void) { return critic_param_count(); }

int cvae_critic_forward(cvae_handle h, int32_t B, const float* x, const float* critic_params, float* pred, void* stream) {
    if (!h || B < 1 || B > h->cfg.max_batch) { cvae_set_error("cvae_critic_forward: bad handle, or batch %d outside [1, max_batch]", B); return CVAE_EINVAL; }
    return launch_critic_fwd(h->cfg.width, B, x, critic_params, pred, (hipStream_t)stream);
}

// ---- critic training step (critic_train.hip) ----
static constexpr int32_t kCriticGradMaxBatch = 65536;
int64_t cvae_critic_train_floats(void) { return critic_train_floats(); }

int64_t cvae_critic_grad_scratch_bytes(cvae_handle h, int32_t batch) {
    if (!h || batch < 1 || batch > kCriticGradMaxBatch) { cvae_set_error("cvae_critic_grad_scratch_bytes: null handle, or batch %d outside [1, %d]", batch, kCriticGradMaxBatch); return -1; }
    return critic_grad_scratch_bytes(batch);
}

int cvae_critic_grad(cvae_handle h, int32_t B, const float* x, const float* target, const uint8_t* keep_or_null, float dropout_p,
                     int32_t loss_kind, const float* critic_params, float* grads, float* pred, float* loss_scalars,
                     uint8_t* decisions_or_null, void* scratch, void* stream) {
    if (!h) { cvae_set_error("cvae_critic_grad: null handle"); return CVAE_EINVAL; }
    if (h->cfg.width != 64) { cvae_set_error("cvae_critic_grad: width %d unsupported (the reference critic is 64x64 only)", h->cfg.width); return CVAE_EUNSUPPORTED; }
    if (B < 1 || B > kCriticGradMaxBatch) { cvae_set_error("cvae_critic_grad: batch %d outside [1, %d]", B, kCriticGradMaxBatch); return CVAE_EINVAL; }
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) { cvae_set_error("cvae_critic_grad: dropout_p %g outside [0, 1)", (double)dropout_p); return CVAE_EINVAL; }
    if (loss_kind != CVAE_CRITIC_LOSS_BCE && loss_kind != CVAE_CRITIC_LOSS_MSE) { cvae_set_error("cvae_critic_grad: loss_kind %d (0 = BCE, 1 = MSE)", loss_kind); return CVAE_EINVAL; }
    if (!x || !target || !critic_params || !grads || !pred || !loss_scalars || !scratch) { cvae_set_error("cvae_critic_grad: null pointer"); return CVAE_EINVAL; }
    if (((uintptr_t)x & 15) || ((uintptr_t)scratch & 15) || ((uintptr_t)decisions_or_null & 3)) {
        cvae_set_error("cvae_critic_grad: x and scratch must be 16-byte aligned, decisions 4-byte aligned"); return CVAE_EINVAL;
    }
    const float scale = (float)(1.0 / (1.0 - (double)dropout_p));
    return launch_critic_grad(h->cfg.width, B, x, target, keep_or_null, scale, loss_kind, critic_params, grads, pred, loss_scalars,
                              decisions_or_null, scratch, (hipStream_t)stream);
}

// ---- critic-side masks: embeddings, the logit's input gradient, occlusion (critic_saliency.hip) ----
// what the three entries share: handle, width, batch, the frames and the parameters; 0 or the error code
static int critic_mask_args(const char* fn, cvae_handle h, int32_t B, const float* x, const float* critic_params) {
    if (!h) { cvae_set_error("%s: null handle", fn); return CVAE_EINVAL; }
    if (h->cfg.width != 64) { cvae_set_error("%s: width %d unsupported (the reference critic is 64x64 only)", fn, h->cfg.width); return CVAE_EUNSUPPORTED; }
    if (B < 1 || B > kCriticGradMaxBatch) { cvae_set_error("%s: batch %d outside [1, %d]", fn, B, kCriticGradMaxBatch); return CVAE_EINVAL; }
    if (!x) { cvae_set_error("%s: x is null", fn); return CVAE_EINVAL; }
    if ((uintptr_t)x & 15) { cvae_set_error("%s: x must be 16-byte aligned", fn); return CVAE_EINVAL; }
    if (!critic_params || ((uintptr_t)critic_params & 3)) { cvae_set_error("%s: critic_params is null or not 4-byte aligned", fn); return CVAE_EINVAL; }
    return 0;
}

// a required (or, with optional, nullable) fp32 output: non-null and 4-byte aligned
static int critic_mask_out(const char* fn, const char* name, const void* p, bool optional) {
    if (!p && !optional) { cvae_set_error("%s: %s is null", fn, name); return CVAE_EINVAL; }
    if ((uintptr_t)p & 3) { cvae_set_error("%s: %s must be 4-byte aligned", fn, name); return CVAE_EINVAL; }
    return 0;
}

int cvae_critic_collect(cvae_handle h, int32_t B, const float* x, const float* critic_params, float* pred, float* e1_or_null,
                        float* e2_or_null, float* e3_or_null, float* e4_or_null, float* e5_or_null, void* stream) {
    const char* fn = "cvae_critic_collect";
    if (int rc = critic_mask_args(fn, h, B, x, critic_params)) return rc;
    if (int rc = critic_mask_out(fn, "pred", pred, false)) return rc;
    float* const e[5] = {e1_or_null, e2_or_null, e3_or_null, e4_or_null, e5_or_null};
    const char* names[5] = {"e1", "e2", "e3", "e4", "e5"};
    for (int i = 0; i < 5; ++i)
        if (int rc = critic_mask_out(fn, names[i], e[i], true)) return rc;
    return launch_critic_collect(B, x, critic_params, pred, e, (hipStream_t)stream);
}

int cvae_critic_saliency(cvae_handle h, int32_t B, const float* x, const float* critic_params, int32_t steps, float* pred,
                         float* grad_or_null, float* map, float* max_values, uint8_t* decisions_or_null, void* stream) {
    const char* fn = "cvae_critic_saliency";
    if (int rc = critic_mask_args(fn, h, B, x, critic_params)) return rc;
    if (steps < 1 || steps > CVAE_CRITIC_IG_MAX_STEPS) { cvae_set_error("%s: steps %d outside [1, %d]", fn, steps, CVAE_CRITIC_IG_MAX_STEPS); return CVAE_EINVAL; }
    if (int rc = critic_mask_out(fn, "pred", pred, false)) return rc;
    if (int rc = critic_mask_out(fn, "grad", grad_or_null, true)) return rc;
    if (int rc = critic_mask_out(fn, "map", map, false)) return rc;
    if (int rc = critic_mask_out(fn, "max_values", max_values, false)) return rc;
    if (int rc = critic_mask_out(fn, "decisions", decisions_or_null, true)) return rc;
    return launch_critic_saliency(B, x, critic_params, steps, pred, grad_or_null, map, max_values, decisions_or_null, (hipStream_t)stream);
}

int cvae_critic_occlusion(cvae_handle h, int32_t B, const float* x, const float* critic_params, int32_t patch, float fill_r,
                          float fill_g, float fill_b, float* pred, float* drop, float* map, float* max_values, void* stream) {
    const char* fn = "cvae_critic_occlusion";
    if (int rc = critic_mask_args(fn, h, B, x, critic_params)) return rc;
    if (patch != 4 && patch != 8 && patch != 16) { cvae_set_error("%s: patch %d (4, 8 or 16)", fn, patch); return CVAE_EINVAL; }
    if (int rc = critic_mask_out(fn, "pred", pred, false)) return rc;
    if (int rc = critic_mask_out(fn, "drop", drop, false)) return rc;
    if (int rc = critic_mask_out(fn, "map", map, false)) return rc;
    if (int rc = critic_mask_out(fn, "max_values", max_values, false)) return rc;
    return launch_critic_occlusion(B, x, critic_params, patch, fill_r, fill_g, fill_b, pred, drop, map, max_values, (hipStream_t)stream);
}

// ---- per-frame scores of the critic against its targets and the pooled record (critic_score.hip) ----
int64_t cvae_critic_score_state_bytes(void) { return critic_score_state_bytes(); }

int64_t cvae_critic_score_scratch_bytes(cvae_handle h, int32_t batch) {
    if (!h || batch < 1 || batch > kCriticGradMaxBatch) { cvae_set_error("cvae_critic_score_scratch_bytes: null handle, or batch %d outside [1, %d]", batch, kCriticGradMaxBatch); return -1; }
    return critic_score_scratch_bytes(batch);
}

int cvae_critic_score_init(cvae_handle h, void* state, void* stream) {
    if (!h || !state || ((uintptr_t)state & 7)) { cvae_set_error("cvae_critic_score_init: bad handle, null or misaligned state"); return CVAE_EINVAL; }
    return launch_critic_score_init(state, (hipStream_t)stream);
}

int cvae_critic_score(cvae_handle h, int32_t B, const uint8_t* frames_hwc, const float* targets, int64_t n_frames,
                      const int64_t* idx_or_null, const float* critic_params, float* per_frame_or_null, void* state_or_null,
                      void* scratch, void* stream) {
    if (!h) { cvae_set_error("cvae_critic_score: null handle"); return CVAE_EINVAL; }
    if (h->cfg.width != 64) { cvae_set_error("cvae_critic_score: width %d unsupported (the reference critic is 64x64 only)", h->cfg.width); return CVAE_EUNSUPPORTED; }
    if (B < 1 || B > kCriticGradMaxBatch) { cvae_set_error("cvae_critic_score: batch %d outside [1, %d]", B, kCriticGradMaxBatch); return CVAE_EINVAL; }
    if (n_frames < 1) { cvae_set_error("cvae_critic_score: n_frames %lld must be >= 1", (long long)n_frames); return CVAE_EINVAL; }
    if (!frames_hwc || !targets || !critic_params) { cvae_set_error("cvae_critic_score: null pointer"); return CVAE_EINVAL; }
    if (!per_frame_or_null && !state_or_null) { cvae_set_error("cvae_critic_score: per_frame and state are both null: nothing to write"); return CVAE_EINVAL; }
    if (!per_frame_or_null && !scratch) { cvae_set_error("cvae_critic_score: without per_frame the rows go to scratch, which is null"); return CVAE_EINVAL; }
    if (!idx_or_null && B > n_frames) { cvae_set_error("cvae_critic_score: batch %d of %lld frames without idx", B, (long long)n_frames); return CVAE_EINVAL; }
    float* rows = per_frame_or_null ? per_frame_or_null : static_cast<float*>(scratch);
    if (((uintptr_t)frames_hwc & 15) || ((uintptr_t)state_or_null & 7) || ((uintptr_t)idx_or_null & 7) || ((uintptr_t)rows & 3) ||
        ((uintptr_t)targets & 3) || ((uintptr_t)critic_params & 3)) {
        cvae_set_error("cvae_critic_score: frames must be 16-byte aligned, state and idx 8-byte, the float arrays 4-byte"); return CVAE_EINVAL;
    }
    return launch_critic_score(B, frames_hwc, targets, n_frames, idx_or_null, critic_params, rows, state_or_null, (hipStream_t)stream);
}

int cvae_preprocess_u8(cvae_handle h, int32_t B, const uint8_t* frames_hwc, float* x, void* stream) {
    if (!h || B < 1 || !frames_hwc || !x) { cvae_set_error("cvae_preprocess_u8: bad handle/batch/pointer"); return CVAE_EINVAL; }
    if (B > h->cfg.max_batch) { cvae_set_error("cvae_preprocess_u8: batch %d outside [1, %d]", B, h->cfg.max_batch); return CVAE_EINVAL; }
    return launch_preprocess_u8(h->cfg.width, B, frames_hwc, x, (hipStream_t)stream);
}

// ---- the training set on the device (load_minerl_data, vae_utility.py:393-461; kernels in dataset.hip) ----
// the scalar arguments both selection entry points share; `who` = the calling function
static bool curate_args_ok(cvae_handle h, int32_t n_traj, int64_t n_frames, int32_t collect, int64_t total_images, const char* who) {
    if (!h) { cvae_set_error("%s: null handle", who); return false; }
    if (n_traj < 0 || n_frames < 0 || total_images < 0) {
        cvae_set_error("%s: n_traj %d, n_frames %lld, total_images %lld must be >= 0", who, n_traj, (long long)n_frames,
                       (long long)total_images);
        return false;
    }
    if (collect < 1) { cvae_set_error("%s: collect %d must be >= 1", who, collect); return false; }
    return true;
}

int cvae_curate_select(cvae_handle h, int32_t n_traj, const int64_t* traj_offsets, int64_t n_frames, const float* preds,
                       int32_t collect, int64_t total_images, int64_t* running, int64_t* counts, int64_t* first,
                       int64_t* span, int64_t* sel, void* stream) {
    if (!curate_args_ok(h, n_traj, n_frames, collect, total_images, "cvae_curate_select")) return CVAE_EINVAL;
    if (!running || !span || (n_traj > 0 && (!traj_offsets || !counts || !first)) || (n_frames > 0 && (!preds || !sel))) {
        cvae_set_error("cvae_curate_select: null pointer"); return CVAE_EINVAL;
    }
    return launch_curate_select(n_traj, traj_offsets, n_frames, preds, collect, total_images, running, counts, first, span, sel,
                                (hipStream_t)stream);
}

int cvae_gather_frames_u8(cvae_handle h, int32_t width, const uint8_t* src_frames, const float* src_preds, int64_t n_src,
                          const int64_t* sel, int64_t max_count, const int64_t* span, uint8_t* dst_frames, float* dst_preds,
                          int64_t capacity, void* stream) {
    if (!h) { cvae_set_error("cvae_gather_frames_u8: null handle"); return CVAE_EINVAL; }
    if (width != h->cfg.width) { cvae_set_error("cvae_gather_frames_u8: width %d, the handle's is %d", width, h->cfg.width); return CVAE_EINVAL; }
    if (n_src < 0 || max_count < 0 || capacity < 0 || max_count > 0x7fffffffLL) {
        cvae_set_error("cvae_gather_frames_u8: n_src %lld, max_count %lld, capacity %lld outside range", (long long)n_src,
                       (long long)max_count, (long long)capacity);
        return CVAE_EINVAL;
    }
    if (!span || (max_count > 0 && (!src_frames || !sel || !dst_frames)) || (!src_preds != !dst_preds)) {
        cvae_set_error("cvae_gather_frames_u8: null pointer (src_preds and dst_preds go together)"); return CVAE_EINVAL;
    }
    if (((uintptr_t)src_frames & 15) || ((uintptr_t)dst_frames & 15)) {
        cvae_set_error("cvae_gather_frames_u8: frame buffers must be 16-byte aligned"); return CVAE_EINVAL;
    }
    return launch_gather_frames_u8(width, src_frames, src_preds, n_src, sel, max_count, span, dst_frames, dst_preds, capacity,
                                   (hipStream_t)stream);
}

// what the two batch gathers check alike; `who` = the calling function, frames = the dataset's frame buffer
static bool batch_gather_ok(cvae_handle h, int32_t batch, int32_t width, const void* frames, const float* preds, int64_t n_frames,
                            const int64_t* idx, const float* x, const float* pred, const char* who) {
    if (!h) { cvae_set_error("%s: null handle", who); return false; }
    if (width != h->cfg.width) { cvae_set_error("%s: width %d, the handle's is %d", who, width, h->cfg.width); return false; }
    if (batch < 1 || batch > h->cfg.max_batch) { cvae_set_error("%s: batch %d outside [1, %d]", who, batch, h->cfg.max_batch); return false; }
    if (n_frames < 1) { cvae_set_error("%s: n_frames %lld must be >= 1", who, (long long)n_frames); return false; }
    if (!frames || !preds || !idx || !x || !pred) { cvae_set_error("%s: null pointer", who); return false; }
    if (((uintptr_t)frames & 15) || ((uintptr_t)x & 15)) { cvae_set_error("%s: frames and x must be 16-byte aligned", who); return false; }
    return true;
}

int cvae_preprocess_u8_gather(cvae_handle h, int32_t batch, int32_t width, const uint8_t* frames_hwc, const float* preds,
                              int64_t n_frames, const int64_t* idx, float* x, float* pred, void* stream) {
    if (!batch_gather_ok(h, batch, width, frames_hwc, preds, n_frames, idx, x, pred, "cvae_preprocess_u8_gather")) return CVAE_EINVAL;
    return launch_preprocess_u8_gather(width, batch, frames_hwc, preds, n_frames, idx, x, pred, (hipStream_t)stream);
}

// ---- the recon branch of the same walk (vae_utility.py:422-443): the second VAE's dataset ----
int cvae_curate_select_recon(cvae_handle h, int32_t n_traj, const int64_t* traj_offsets, int64_t n_frames, const float* preds,
                             int32_t collect, int64_t total_images, int64_t* running, int64_t* counts, int64_t* first,
                             int64_t* sel_first, int64_t* span, int64_t* ent_frame, int32_t* ent_kind, int64_t* ent_sel,
                             int64_t* sel, void* stream) {
    if (!curate_args_ok(h, n_traj, n_frames, collect, total_images, "cvae_curate_select_recon")) return CVAE_EINVAL;
    if (!running || !span || (n_traj > 0 && (!traj_offsets || !counts || !first || !sel_first)) ||
        (n_frames > 0 && (!preds || !ent_frame || !ent_kind || !ent_sel || !sel))) {
        cvae_set_error("cvae_curate_select_recon: null pointer"); return CVAE_EINVAL;
    }
    return launch_curate_select_recon(n_traj, traj_offsets, n_frames, preds, collect, total_images, running, counts, first,
                                      sel_first, span, ent_frame, ent_kind, ent_sel, sel, (hipStream_t)stream);
}

int cvae_recon_zcat(cvae_handle h, int32_t n_entries, const int64_t* ent_sel, const int32_t* ent_kind, const float* mu,
                    const float* sel_preds, int64_t n_sel, float* zcat, void* stream) {
    if (!h) { cvae_set_error("cvae_recon_zcat: null handle"); return CVAE_EINVAL; }
    if (n_entries < 1 || n_entries > h->cfg.max_batch) {
        cvae_set_error("cvae_recon_zcat: n_entries %d outside [1, %d]", n_entries, h->cfg.max_batch); return CVAE_EINVAL;
    }
    if (n_sel < 1) { cvae_set_error("cvae_recon_zcat: n_sel %lld must be >= 1", (long long)n_sel); return CVAE_EINVAL; }
    if (!ent_sel || !ent_kind || !mu || !sel_preds || !zcat) { cvae_set_error("cvae_recon_zcat: null pointer"); return CVAE_EINVAL; }
    return launch_recon_zcat(n_entries, ent_sel, ent_kind, mu, sel_preds, n_sel, zcat, (hipStream_t)stream);
}

int cvae_inject_zcat(cvae_handle h, int32_t n_images, int32_t n_rewards, const float* mu, const float* rewards, float* zcat, void* stream) {
    if (!h) { cvae_set_error("cvae_inject_zcat: null handle"); return CVAE_EINVAL; }
    if (n_images < 1 || n_rewards < 1 || (int64_t)n_images * n_rewards > h->cfg.max_batch) {
        cvae_set_error("cvae_inject_zcat: %d images x %d rewards outside [1, max_batch %d]", n_images, n_rewards, h->cfg.max_batch); return CVAE_EINVAL;
    }
    if (!mu || !rewards || !zcat) { cvae_set_error("cvae_inject_zcat: null pointer"); return CVAE_EINVAL; }
    return launch_inject_zcat(n_images, n_rewards, mu, rewards, zcat, (hipStream_t)stream);
}

int cvae_gather_f32(cvae_handle h, int32_t batch, int32_t width, const float* frames, const float* preds, int64_t n_frames,
                    const int64_t* idx, float* x, float* pred, void* stream) {
    if (!batch_gather_ok(h, batch, width, frames, preds, n_frames, idx, x, pred, "cvae_gather_f32")) return CVAE_EINVAL;
    return launch_gather_f32(width, batch, frames, preds, n_frames, idx, x, pred, (hipStream_t)stream);
}

// the augmented gathers: the plain gathers' checks, then the ranges of cvae_augment (fp32: no gain), all on the host
static bool augment_ok(const cvae_augment* aug, int32_t width, bool allow_gain, const char* who) {
    if (!aug) { cvae_set_error("%s: null aug", who); return false; }
    if (aug->flip_below > (1u << 24)) { cvae_set_error("%s: flip_below %u above 2^24", who, aug->flip_below); return false; }
    if (aug->max_shift < 0 || aug->max_shift > width / 4) {
        cvae_set_error("%s: max_shift %d outside [0, %d] (width / 4)", who, aug->max_shift, width / 4); return false;
    }
    if (aug->gain_q16 < 0 || aug->gain_q16 > 65535) { cvae_set_error("%s: gain_q16 %d outside [0, 65535]", who, aug->gain_q16); return false; }
    if (!allow_gain && aug->gain_q16 != 0) {
        cvae_set_error("%s: gain_q16 %d: fp32 entries are Tanh outputs, a brightness gain clamped at 1 has no meaning for them", who, aug->gain_q16);
        return false;
    }
    if (aug->reserved != 0) { cvae_set_error("%s: reserved must be 0", who); return false; }
    return true;
}

int cvae_preprocess_u8_gather_aug(cvae_handle h, int32_t batch, int32_t width, const uint8_t* frames_hwc, const float* preds,
                                  int64_t n_frames, const int64_t* idx, const cvae_augment* aug, float* x, float* pred,
                                  int32_t* applied, void* stream) {
    const char* who = "cvae_preprocess_u8_gather_aug";
    if (!batch_gather_ok(h, batch, width, frames_hwc, preds, n_frames, idx, x, pred, who) || !augment_ok(aug, width, true, who)) return CVAE_EINVAL;
    return launch_preprocess_u8_gather_aug(width, batch, frames_hwc, preds, n_frames, idx, *aug, x, pred, applied, (hipStream_t)stream);
}

int cvae_gather_f32_aug(cvae_handle h, int32_t batch, int32_t width, const float* frames, const float* preds, int64_t n_frames,
                        const int64_t* idx, const cvae_augment* aug, float* x, float* pred, int32_t* applied, void* stream) {
    const char* who = "cvae_gather_f32_aug";
    if (!batch_gather_ok(h, batch, width, frames, preds, n_frames, idx, x, pred, who) || !augment_ok(aug, width, false, who)) return CVAE_EINVAL;
    return launch_gather_f32_aug(width, batch, frames, preds, n_frames, idx, *aug, x, pred, applied, (hipStream_t)stream);
}

// |recon_zero - recon_one| -> greyscale difference mask (get_diff_image, vae_utility.py:256-277), batched
int cvae_diff_grey(cvae_handle h, int32_t B, const float* recon_one, const float* recon_zero, float* diff, void* stream) {
    if (!h || B < 1) { cvae_set_error("cvae_diff_grey: bad handle/batch"); return CVAE_EINVAL; }
    return launch_diff_grey(h->cfg.width, B, recon_one, recon_zero, diff, (hipStream_t)stream);
}

// ---- segmentation evaluation (eval_textured_frames, vae_utility.py:162-212; kernels in segment.hip) ----
// batch is not capped by max_batch; the per-pixel launches need batch * W * W < 2^31 work-items
static bool seg_batch_ok(cvae_handle h, int32_t B, const char* who) {
    if (!h) { cvae_set_error("%s: null handle", who); return false; }
    const int W = h->cfg.width;
    if (W != 64 && W != 128) { cvae_set_error("%s: width %d not supported (64 or 128)", who, W); return false; }
    if (B < 1 || (int64_t)B * W * W > 0x7fffffffLL) { cvae_set_error("%s: batch %d outside [1, 2^31 / (%d * %d))", who, B, W, W); return false; }
    return true;
}

int64_t cvae_crf_scratch_bytes(cvae_handle h, int32_t B) {
    if (!seg_batch_ok(h, B, "cvae_crf_scratch_bytes")) return CVAE_EINVAL;
    return crf_scratch_bytes(h->cfg.width, B);
}

int cvae_dense_crf(cvae_handle h, int32_t B, const uint8_t* frames_hwc, const float* prob1, const cvae_crf_params* p,
                   uint8_t* labels, float* q1, void* scratch, void* stream) {
    if (!seg_batch_ok(h, B, "cvae_dense_crf")) return CVAE_EINVAL;
    if (!frames_hwc || !prob1 || !p || !labels || !scratch) { cvae_set_error("cvae_dense_crf: null frames, prob1, params, labels or scratch"); return CVAE_EINVAL; }
    const float fin[6] = {p->w1, p->alpha, p->beta, p->w2, p->gamma, p->p_floor};
    for (float v : fin)
        if (!std::isfinite(v)) { cvae_set_error("cvae_dense_crf: non-finite parameter"); return CVAE_EINVAL; }
    if (p->w1 < 0.f || p->w2 < 0.f) { cvae_set_error("cvae_dense_crf: weights w1 %g, w2 %g must be >= 0", p->w1, p->w2); return CVAE_EINVAL; }
    if (!(p->alpha > 0.f && p->beta > 0.f && p->gamma > 0.f)) { cvae_set_error("cvae_dense_crf: alpha %g, beta %g, gamma %g must be > 0", p->alpha, p->beta, p->gamma); return CVAE_EINVAL; }
    if (!(p->p_floor > 0.f && p->p_floor <= 1.f)) { cvae_set_error("cvae_dense_crf: p_floor %g outside (0, 1]", p->p_floor); return CVAE_EINVAL; }
    if (p->iterations < 0 || p->iterations > 10000) { cvae_set_error("cvae_dense_crf: iterations %d outside [0, 10000]", p->iterations); return CVAE_EINVAL; }
    if (((uintptr_t)scratch & 255) != 0) { cvae_set_error("cvae_dense_crf: scratch not 256-byte aligned"); return CVAE_EINVAL; }
    return launch_dense_crf(h->cfg.width, B, frames_hwc, prob1, *p, labels, q1, scratch, (hipStream_t)stream);
}

// ---- the CRF for a grid of variants (kernels in crf_grid.hip) ----
int32_t cvae_crf_grid_group(cvae_handle h) {
    if (!h) { cvae_set_error("cvae_crf_grid_group: null handle"); return CVAE_EINVAL; }
    return crf_grid_group();
}

int64_t cvae_crf_grid_scratch_bytes(cvae_handle h, int32_t B, int32_t n_variants) {
    if (!seg_batch_ok(h, B, "cvae_crf_grid_scratch_bytes")) return CVAE_EINVAL;
    if (n_variants < 1 || n_variants > CVAE_CRF_GRID_MAX_VARIANTS) {
        cvae_set_error("cvae_crf_grid_scratch_bytes: n_variants %d outside [1, %d]", n_variants, CVAE_CRF_GRID_MAX_VARIANTS); return CVAE_EINVAL;
    }
    return crf_grid_scratch_bytes(h->cfg.width, B, n_variants);
}

int cvae_crf_grid(cvae_handle h, int32_t B, const uint8_t* frames_hwc, const float* prob1, const uint8_t* diff_u8, const uint8_t* gt,
                  float alpha, float beta, float gamma, const cvae_crf_variant* variants, int32_t n_variants, const int32_t* snaps,
                  int32_t n_snaps, int64_t* counts, uint8_t* labels, float* q1, void* scratch, void* stream) {
    const char* who = "cvae_crf_grid";
    if (!seg_batch_ok(h, B, who)) return CVAE_EINVAL;
    if (!frames_hwc || !variants || !snaps || !scratch) { cvae_set_error("%s: null frames, variants, snaps or scratch", who); return CVAE_EINVAL; }
    if (n_variants < 1 || n_variants > CVAE_CRF_GRID_MAX_VARIANTS) { cvae_set_error("%s: n_variants %d outside [1, %d]", who, n_variants, CVAE_CRF_GRID_MAX_VARIANTS); return CVAE_EINVAL; }
    if (n_snaps < 1 || n_snaps > CVAE_CRF_GRID_MAX_SNAPS) { cvae_set_error("%s: n_snaps %d outside [1, %d]", who, n_snaps, CVAE_CRF_GRID_MAX_SNAPS); return CVAE_EINVAL; }
    if (!counts && !labels && !q1) { cvae_set_error("%s: no output requested (counts, labels and q1 are all null)", who); return CVAE_EINVAL; }
    if (counts && !gt) { cvae_set_error("%s: counts need the ground truth", who); return CVAE_EINVAL; }
    if (!std::isfinite(alpha) || !std::isfinite(beta) || !std::isfinite(gamma)) { cvae_set_error("%s: non-finite parameter", who); return CVAE_EINVAL; }
    if (!(alpha > 0.f && beta > 0.f && gamma > 0.f)) { cvae_set_error("%s: alpha %g, beta %g, gamma %g must be > 0", who, alpha, beta, gamma); return CVAE_EINVAL; }
    for (int k = 0; k < n_variants; ++k) {
        const cvae_crf_variant& v = variants[k];
        if (v.thr < -1 || v.thr > 255) { cvae_set_error("%s: variant %d: thr %d outside [-1, 255]", who, k, v.thr); return CVAE_EINVAL; }
        if (v.thr < 0 ? !prob1 : !diff_u8) { cvae_set_error("%s: variant %d (thr %d) needs the %s plane, which is null", who, k, v.thr, v.thr < 0 ? "prob1" : "diff_u8"); return CVAE_EINVAL; }
        if (!std::isfinite(v.p_floor) || !std::isfinite(v.w1) || !std::isfinite(v.w2)) { cvae_set_error("%s: variant %d: non-finite parameter", who, k); return CVAE_EINVAL; }
        if (v.w1 < 0.f || v.w2 < 0.f) { cvae_set_error("%s: variant %d: weights w1 %g, w2 %g must be >= 0", who, k, v.w1, v.w2); return CVAE_EINVAL; }
        if (!(v.p_floor > 0.f && v.p_floor <= 1.f)) { cvae_set_error("%s: variant %d: p_floor %g outside (0, 1]", who, k, v.p_floor); return CVAE_EINVAL; }
    }
    for (int s = 0; s < n_snaps; ++s) {
        if (snaps[s] < 0 || snaps[s] > 10000) { cvae_set_error("%s: snapshot %d outside [0, 10000]", who, snaps[s]); return CVAE_EINVAL; }
        if (s > 0 && snaps[s] <= snaps[s - 1]) { cvae_set_error("%s: snapshots must ascend strictly (%d after %d)", who, snaps[s], snaps[s - 1]); return CVAE_EINVAL; }
    }
    if (((uintptr_t)scratch & 255) != 0) { cvae_set_error("%s: scratch not 256-byte aligned", who); return CVAE_EINVAL; }
    return launch_crf_grid(h->cfg.width, B, frames_hwc, prob1, diff_u8, gt, alpha, beta, gamma, variants, n_variants, snaps, n_snaps,
                           counts, labels, q1, scratch, (hipStream_t)stream);
}

int cvae_diff_normalize(cvae_handle h, int32_t B, const float* diff, double mean_max, double diff_factor, int32_t thr,
                        const uint8_t* gt, uint8_t* diff_u8, uint8_t* mask, int64_t* counts, int64_t* hist, void* stream) {
    if (!seg_batch_ok(h, B, "cvae_diff_normalize")) return CVAE_EINVAL;
    if (!diff || !diff_u8) { cvae_set_error("cvae_diff_normalize: null diff or diff_u8"); return CVAE_EINVAL; }
    if (!std::isfinite(mean_max) || !std::isfinite(diff_factor) || mean_max < 0.0 || diff_factor < 0.0) {
        cvae_set_error("cvae_diff_normalize: mean_max %g, diff_factor %g must be finite and >= 0", mean_max, diff_factor); return CVAE_EINVAL;
    }
    if (thr < 0 || thr > 255) { cvae_set_error("cvae_diff_normalize: thr %d outside [0, 255]", thr); return CVAE_EINVAL; }
    if ((counts || hist) && !gt) { cvae_set_error("cvae_diff_normalize: frame counts and histogram need the ground truth"); return CVAE_EINVAL; }
    return launch_diff_normalize(h->cfg.width, B, diff, mean_max, diff_factor, thr, gt, diff_u8, mask, counts, hist, (hipStream_t)stream);
}

int cvae_mask_counts(cvae_handle h, int32_t B, const uint8_t* mask, const uint8_t* gt, int64_t* counts, void* stream) {
    if (!seg_batch_ok(h, B, "cvae_mask_counts")) return CVAE_EINVAL;
    if (!mask || !gt || !counts) { cvae_set_error("cvae_mask_counts: null mask, gt or frame_counts"); return CVAE_EINVAL; }
    return launch_mask_counts(h->cfg.width, B, mask, gt, counts, (hipStream_t)stream);
}

// ---- objects from masks (components.hip) ----
int cvae_mask_objects(cvae_handle h, int32_t B, const uint8_t* mask, const uint8_t* values, const cvae_object_params* p,
                      uint8_t* mask_out, uint16_t* labels, int32_t* info, int32_t* table, void* stream, uint32_t flags) {
    const char* who = "cvae_mask_objects";
    if (!seg_batch_ok(h, B, who)) return CVAE_EINVAL;
    if (!mask || !p || !info) { cvae_set_error("%s: null mask, params or info", who); return CVAE_EINVAL; }
    if (flags != 0) { cvae_set_error("%s: flags = %u must be 0", who, (unsigned)flags); return CVAE_EINVAL; }
    if (p->connectivity != 4 && p->connectivity != 8) { cvae_set_error("%s: connectivity %d must be 4 or 8", who, p->connectivity); return CVAE_EINVAL; }
    if (p->fill_holes != 0 && p->fill_holes != 1) { cvae_set_error("%s: fill_holes %d must be 0 or 1", who, p->fill_holes); return CVAE_EINVAL; }
    if (p->min_area < 1) { cvae_set_error("%s: min_area %d must be >= 1", who, p->min_area); return CVAE_EINVAL; }
    if (p->keep_largest < 0) { cvae_set_error("%s: keep_largest %d must be >= 0", who, p->keep_largest); return CVAE_EINVAL; }
    if (p->max_objects < 1 || p->max_objects > CVAE_OBJECTS_MAX) {
        cvae_set_error("%s: max_objects %d outside [1, %d]", who, p->max_objects, CVAE_OBJECTS_MAX); return CVAE_EINVAL;
    }
    if (((uintptr_t)mask | (uintptr_t)values | (uintptr_t)mask_out | (uintptr_t)labels) & 15) {
        cvae_set_error("%s: mask, values, mask_out and labels must be 16-byte aligned", who); return CVAE_EINVAL;
    }
    if (((uintptr_t)info | (uintptr_t)table) & 3) { cvae_set_error("%s: info and table must be 4-byte aligned", who); return CVAE_EINVAL; }
    return launch_mask_objects(h->cfg.width, B, mask, values, p->connectivity == 8, p->fill_holes, p->min_area, p->keep_largest,
                               p->max_objects, mask_out, labels, info, table, (hipStream_t)stream);
}

int cvae_object_overlap(cvae_handle h, int32_t B, const uint16_t* labels_a, const uint16_t* labels_b, int32_t M, int32_t* inter,
                        void* stream, uint32_t flags) {
    const char* who = "cvae_object_overlap";
    if (!seg_batch_ok(h, B, who)) return CVAE_EINVAL;
    if (!labels_a || !labels_b || !inter) { cvae_set_error("%s: null labels_a, labels_b or inter", who); return CVAE_EINVAL; }
    if (flags != 0) { cvae_set_error("%s: flags = %u must be 0", who, (unsigned)flags); return CVAE_EINVAL; }
    if (M < 1 || M > CVAE_OBJECTS_MAX) { cvae_set_error("%s: max_objects %d outside [1, %d]", who, M, CVAE_OBJECTS_MAX); return CVAE_EINVAL; }
    if (((uintptr_t)labels_a | (uintptr_t)labels_b) & 15) { cvae_set_error("%s: labels_a and labels_b must be 16-byte aligned", who); return CVAE_EINVAL; }
    if ((uintptr_t)inter & 3) { cvae_set_error("%s: inter must be 4-byte aligned", who); return CVAE_EINVAL; }
    return launch_object_overlap(h->cfg.width, B, labels_a, labels_b, M, inter, (hipStream_t)stream);
}

// ---- the reference's pictures (get_final_frame / get_injected_img, vae_utility.py:240-322; kernel in render.hip) ----
int cvae_compose_frames(cvae_handle h, int32_t B, int32_t n_panels, const cvae_panel* panels, int32_t row_offset, int32_t flags,
                        const uint8_t* overlay, const uint8_t* atlas, int32_t n_labels, int32_t label_h, int32_t label_w,
                        const int32_t* label_idx, int32_t label_x, int32_t label_y, uint8_t* out, void* stream) {
    if (!h) { cvae_set_error("cvae_compose_frames: null handle"); return CVAE_EINVAL; }
    const int W = h->cfg.width;
    if (W != 64 && W != 128) { cvae_set_error("cvae_compose_frames: width %d not supported (64 or 128)", W); return CVAE_EINVAL; }
    if (B < 1) { cvae_set_error("cvae_compose_frames: batch %d must be >= 1", B); return CVAE_EINVAL; }
    if (n_panels < 1 || n_panels > CVAE_MAX_PANELS || !panels) {
        cvae_set_error("cvae_compose_frames: n_panels %d outside [1, %d] or null panels", n_panels, CVAE_MAX_PANELS); return CVAE_EINVAL;
    }
    if (row_offset < 0 || row_offset > 2 * W) { cvae_set_error("cvae_compose_frames: row_offset %d outside [0, %d]", row_offset, 2 * W); return CVAE_EINVAL; }
    if (flags & ~CVAE_COMPOSE_CLAMP) { cvae_set_error("cvae_compose_frames: unknown flags %d", flags); return CVAE_EINVAL; }
    for (int i = 0; i < n_panels; ++i) {
        const cvae_panel& p = panels[i];
        if (p.kind < CVAE_PANEL_F32_CHW || p.kind > CVAE_PANEL_MASK) { cvae_set_error("cvae_compose_frames: panel %d has unknown kind %d", i, p.kind); return CVAE_EINVAL; }
        if (!p.data || ((uintptr_t)p.data & 15)) { cvae_set_error("cvae_compose_frames: panel %d data is null or not 16-byte aligned", i); return CVAE_EINVAL; }
        if (p.batch_stride < 0 || p.batch_stride % (p.kind == CVAE_PANEL_U8_HWC ? 16 : 4)) {
            cvae_set_error("cvae_compose_frames: panel %d batch_stride %lld must be >= 0 and a multiple of %d", i, (long long)p.batch_stride,
                           p.kind == CVAE_PANEL_U8_HWC ? 16 : 4);
            return CVAE_EINVAL;
        }
    }
    if (!out || ((uintptr_t)out & 15) || ((uintptr_t)overlay & 15)) { cvae_set_error("cvae_compose_frames: out is null, or out / overlay not 16-byte aligned"); return CVAE_EINVAL; }
    if (atlas && (!label_idx || n_labels < 1 || label_h < 1 || label_w < 1 || label_h > 4096 || label_w > 4096 ||
                  label_x < -4096 || label_x > 65536 || label_y < -4096 || label_y > 65536)) {
        cvae_set_error("cvae_compose_frames: an atlas needs label_idx, n_labels >= 1, a label size in [1, 4096]^2 and a position near the picture");
        return CVAE_EINVAL;
    }
    return launch_compose_frames(W, B, n_panels, panels, row_offset, flags & CVAE_COMPOSE_CLAMP, overlay, atlas, n_labels, label_h, label_w,
                                 label_idx, label_x, label_y, out, (hipStream_t)stream);
}

// ---- probe API: bracket chosen conv kernels of the real step with HIP events (bench.py roofline) ----
int cvae_probe_config(cvae_handle h, uint32_t mask) {
    if (!h) return CVAE_EINVAL;
    for (int id = 0; id < PROBE_IDS; ++id) {
        ProbeSlot& s = h->probe.slot[id];
        s.n = 0;
        if (((mask >> id) & 1u) && !s.made) {
            for (int i = 0; i < PROBE_CAP; ++i) {
                hipError_t e = hipEventCreate(&s.e0[i]);
                if (e == hipSuccess) e = hipEventCreate(&s.e1[i]);
                if (e != hipSuccess) { cvae_set_error("probe event create: %s", hipGetErrorString(e)); return (int)e; }
            }
            s.made = true;
        }
    }
    h->probe.mask = mask;
    return 0;
}

// elapsed ms of every recorded launch of slot `id` (synchronises on the events); returns the count
int cvae_probe_read(cvae_handle h, int32_t id, float* ms_host, int32_t cap) {
    if (!h || id < 0 || id >= PROBE_IDS) return 0;
    ProbeSlot& s = h->probe.slot[id];
    int n = 0;
    for (int i = 0; i < s.n && n < cap; ++i) {
        if (hipEventSynchronize(s.e1[i]) != hipSuccess) break;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.e0[i], s.e1[i]) != hipSuccess) break;
        ms_host[n++] = ms;
    }
    s.n = 0;
    return n;
}

// ------------------------------ per-op entry points ------------------------------
// Conv layers 1..7 go through the conv table: the kernels the step runs on this handle, on tensors in the handle's storage type
// (precision 1: bf16 activations and activation gradients; fp32 weights, biases, their gradients and recon / d_recon); layers 0 and 8
// run the plain forms of E1 / D4.  Host-only checks of a conv entry, before any device access: lo..hi = the layers it documents; a null
// scratch is refused on every weight gradient and on the forward / input-gradient passes whose table row writes scratch.
static int op_conv_check(const char* who, cvae_handle h, int layer, int lo, int hi, int B, bool wgrad, const void* scratch) {
    if (!h) { cvae_set_error("%s: null handle", who); return CVAE_EINVAL; }
    if (layer < lo || layer > hi) { cvae_set_error("%s: layer %d outside [%d, %d]", who, layer, lo, hi); return CVAE_EINVAL; }
    if (B < 1 || B > h->cfg.max_batch) { cvae_set_error("%s: batch %d outside [1, %d]", who, B, h->cfg.max_batch); return CVAE_EINVAL; }
    if (scratch || !(wgrad || (layer >= 1 && layer <= 7 && fd_uses_scratch(conv_row(h, layer), layer, h->cfg.width)))) return 0;
    cvae_set_error("%s: null scratch (layer %d on this handle prepares its weights or reduces split-K slabs there)", who, layer);
    return CVAE_EINVAL;
}
// The weight forms of a forward / input-gradient call, prepared in its scratch: [pack block (the step's wpack, only the layer's own
// slots written) | the layer's collapsed weights | *rest: everything else], each part only where the table row reads it
static int op_weights(cvae_handle h, int layer, const float* wt, float* scratch, hipStream_t st, ConvWeights* f, float** rest) {
    *f = ConvWeights{};
    f->raw[layer - 1] = wt;
    if (conv_row(h, layer).wform == W_PACKED) { f->packed = scratch; scratch += align_up(pack_floats(h), 64); }
    if (layer >= 5) { f->collapsed[layer - 5] = scratch; scratch += conv_up_wc_floats(layer); }
    *rest = scratch;
    return prepare_conv_weights(h, *f, st);
}

int cvae_op_conv_fwd(cvae_handle h, int32_t layer, int32_t B, const float* in, const float* wt, const float* bias,
                     float* out, float* bn_partials, void* scratch, void* stream) {
    RC(op_conv_check("cvae_op_conv_fwd", h, layer, 0, 8, B, false, scratch));
    hipStream_t st = (hipStream_t)stream;
    if (layer == 0) return launch_e1_fwd(h->cfg.width, B, in, wt, bias, out, bn_partials, st, io_bf16(h));   // y in the handle's storage type
    if (layer == 8) return launch_d4_fwd(h->cfg.width, B, in, wt, bias, out, st, io_bf16(h));                // o3 in the handle's storage type
    ConvWeights forms; float* rest;
    RC(op_weights(h, layer, wt, (float*)scratch, st, &forms, &rest));
    return conv_fwd(h, layer, B, in, forms, bias, out, bn_partials, rest, st, nullptr);
}

int cvae_op_conv_dgrad(cvae_handle h, int32_t layer, int32_t B, const float* dout, const float* wt,
                       const float* mask_src, float* din, void* scratch, void* stream) {
    RC(op_conv_check("cvae_op_conv_dgrad", h, layer, 1, 7, B, false, scratch));
    ConvWeights forms; float* rest;
    RC(op_weights(h, layer, wt, (float*)scratch, (hipStream_t)stream, &forms, &rest));
    return conv_dgrad(h, layer, B, dout, forms, mask_src, din, rest, (hipStream_t)stream);
}

// cvae_op_e1_wgrad_fused with flag bit 0: [E1's weight-gradient workspace | packed bf16 frame | partials of the statistics pass]
static int64_t e1_fused_xp_floats(const cvae_handle_s* h, int B) {
    const int64_t W = h->cfg.width;
    return align_up(e1_wgrad_ws_floats((int)W, B), 64) + align_up((int64_t)B * W * W * 2, 64) + (int64_t)2 * bn_num_tiles(0, (int)W, B) * 32;
}
// [pack block | the step's scratch, which starts with room for one layer's collapsed weights and covers the split-K and weight-gradient
// slabs of every precision's launchers and d4_bwd's workspace (carve)]; on a bf16 handle at least what
// cvae_op_e1_wgrad_fused lays out with flag bit 0
int64_t cvae_op_scratch_floats(cvae_handle h, int32_t B) {
    const WsLayout w = carve(h, B);
    const int64_t n = w.total - w.scratch + align_up(pack_floats(h), 64);
    return h->cfg.precision == 1 && e1_fused_xp_floats(h, B) > n ? e1_fused_xp_floats(h, B) : n;
}

int cvae_op_conv_wgrad(cvae_handle h, int32_t layer, int32_t B, const float* in, const float* dout, float* dw,
                       float* dbias, void* scratch, void* stream) {
    RC(op_conv_check("cvae_op_conv_wgrad", h, layer, 0, 7, B, true, scratch));
    if (layer == 0) return launch_e1_wgrad(h->cfg.width, B, in, dout, dw, dbias, (float*)scratch, (hipStream_t)stream);
    return conv_wgrad(h, layer, B, in, dout, dw, dbias, (float*)scratch, (hipStream_t)stream);
}

// E1's weight gradient as the step runs it (block_grads(0)): block 0's BatchNorm / pool / ReLU backward applied while the kernel stages
// its tiles.  Host-only checks first, as in op_conv_check.  flags bit 0 (bf16 handles): the statistics pass of the forward writes the
// packed bf16 frame into `scratch` and the kernel stages its strips from it, as after a train-mode forward.
int cvae_op_e1_wgrad_fused(cvae_handle h, int32_t B, const float* x, const float* y0, const float* a0, const float* d_a0,
                           const float* coef0, const float* bcoef0, const float* w1, const float* b1, float* dw, float* dbias,
                           void* scratch, int32_t flags, void* stream) {
    const char* who = "cvae_op_e1_wgrad_fused";
    if (!h) { cvae_set_error("%s: null handle", who); return CVAE_EINVAL; }
    if (B < 1 || B > h->cfg.max_batch) { cvae_set_error("%s: batch %d outside [1, %d]", who, B, h->cfg.max_batch); return CVAE_EINVAL; }
    const bool bf16 = io_bf16(h);
    const struct { const void* p; const char* name; bool needed; } args[] = {
        {x, "x", true}, {y0, "y0", !bf16}, {a0, "a0", true}, {d_a0, "d_a0", true}, {coef0, "coef0", true}, {bcoef0, "bcoef0", true},
        {w1, "w1", bf16}, {b1, "b1", bf16}, {dw, "dw", true}, {scratch, "scratch", true}};
    for (const auto& a : args)
        if (a.needed && !a.p) { cvae_set_error("%s: null %s (y0 may be null on bf16 handles only, w1 and b1 on the others)", who, a.name); return CVAE_EINVAL; }
    if (flags & ~1) { cvae_set_error("%s: unknown flag bits in flags = %d (bit 0: stage the packed bf16 frame)", who, flags); return CVAE_EINVAL; }
    const int W = h->cfg.width;
    if ((flags & 1) && !bf16) { cvae_set_error("%s: flags bit 0 (packed bf16 frame) on a handle that is not bf16", who); return CVAE_EINVAL; }
    if ((flags & 1) && conv_route(1, 0, W, false, B).family != E1_PACKED_FRAME) {
        cvae_set_error("%s: flags bit 0 at batch %d, where the step stages the fp32 frame (cvae_conv_route)", who, B); return CVAE_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    float* sc = (float*)scratch;
    const float* xp = nullptr;
    if (flags & 1) {
        float* xpf = sc + align_up(e1_wgrad_ws_floats(W, B), 64);
        RC(launch_e1_fwd(W, B, x, w1, b1, nullptr, xpf + align_up((int64_t)B * W * W * 2, 64), st, true, 1, nullptr, nullptr, xpf));
        xp = xpf;
    }
    const float* fu[7] = {y0, a0, d_a0, coef0, bcoef0, w1, b1};
    return launch_e1_wgrad(W, B, x, nullptr, dw, dbias, sc, st, bf16, fu, xp);
}

// bf16 mode: o3 / d_o3 in bf16, the Tanh backward applied while the kernel stages (`dout` is not written and may be null)
int cvae_op_d4_bwd(cvae_handle h, int32_t B, const float* o3, const float* d_recon, const float* recon, const float* wt,
                   float* dout, float* d_o3, float* dw, float* db, void* scratch, void* stream) {
    return launch_d4_bwd(h->cfg.width, B, o3, d_recon, recon, wt, dout, d_o3, dw, db, (float*)scratch, (hipStream_t)stream, io_bf16(h));
}

// 128-pixel tiles behind one BatchNorm partial row of cvae_op_conv_fwd (the route table's; 1 for the per-tile kernels and layer 0)
int32_t cvae_op_conv_tiles_per_partial(cvae_handle h, int32_t layer, int32_t B) {
    if (!h || layer < 0 || layer > 3 || B < 1) { cvae_set_error("cvae_op_conv_tiles_per_partial: null handle, layer %d outside [0, 3] or batch %d below 1", layer, B); return CVAE_EINVAL; }
    return conv_route(h->cfg.precision, layer, h->cfg.width, false, B).tilesPerPartial;
}

// (tiles, splits, tiles per split) of cvae_op_conv_wgrad's kernel on a bf16 handle (layer 0: cvae_op_e1_wgrad_fused's), from the launchers'
// own split arithmetic (no launch)
int cvae_op_conv_wgrad_plan(cvae_handle h, int32_t layer, int32_t B, int32_t* out) {
    if (!h || !out || B < 1) { cvae_set_error("cvae_op_conv_wgrad_plan: null handle or output, or batch %d below 1", B); return CVAE_EINVAL; }
    if (h->cfg.precision != 1 || layer < 0 || layer > 7) { cvae_set_error("cvae_op_conv_wgrad_plan: layer %d on this handle does not run a bf16 weight-gradient kernel (bf16 handles, layers 0..7)", layer); return CVAE_EUNSUPPORTED; }
    int plan[3] = {0, 0, 0};
    RC(layer == 0  ? e1_wgrad_plan_bf16(h->cfg.width, B, plan)
       : layer >= 5 ? conv_up_wgrad_bf16_plan(layer, h->cfg.width, B, plan) : conv_wgrad_bf16_plan(layer, h->cfg.width, B, plan));
    for (int i = 0; i < 3; ++i) out[i] = plan[i];
    return CVAE_OK;
}

// include/cvae.h: the same of the fp32 kernels, from the launchers' own split functions (host logic only, no handle, no device access)
int32_t cvae_op_conv_wgrad_plan_f32(int32_t width, int32_t layer, int32_t B, int32_t num_cus, int32_t* out) {
    if ((width != 64 && width != 128) || layer < 0 || layer > 8 || B < 1 || num_cus < 1 || !out) {
        cvae_set_error("cvae_op_conv_wgrad_plan_f32: width %d not 64 / 128, layer %d outside [0, 8], batch %d or compute units %d below 1, or null pointer",
                       width, layer, B, num_cus);
        return CVAE_EINVAL;
    }
    int plan[3] = {0, 0, 0};
    RC(layer == 0 || layer == 8 ? thin_wgrad_plan_f32(layer, width, B, plan)
       : layer >= 5             ? conv_up_wgrad_plan_f32(layer, width, B, num_cus, plan)
                                : conv_wgrad_plan_f32(layer, width, B, plan));
    for (int i = 0; i < 3; ++i) out[i] = plan[i];
    return CVAE_OK;
}

// the statistics half of cvae_op_bn_pool_act_fwd, on partial rows of `tiles_per_partial` tiles each
int cvae_op_bn_fwd_finalize(cvae_handle h, int32_t layer, int32_t B, const float* bn_partials, int32_t tiles_per_partial,
                            const float* gamma, const float* beta, float* run_mean, float* run_var, float* coef,
                            void* scratch, int32_t train, void* stream) {
    if (!h || layer < 0 || layer > 3 || B < 1 || !gamma || !beta || !run_mean || !run_var || !coef || !scratch || (train && !bn_partials)) {
        cvae_set_error("cvae_op_bn_fwd_finalize: null argument, layer %d outside [0, 3] or batch %d below 1", layer, B); return CVAE_EINVAL;
    }
    if (tiles_per_partial != 1 && tiles_per_partial != 2 && tiles_per_partial != 4 && tiles_per_partial != 8) {
        cvae_set_error("cvae_op_bn_fwd_finalize: %d tiles per partial (1, 2, 4 or 8)", tiles_per_partial); return CVAE_EINVAL;
    }
    return launch_bn_fwd_finalize(layer, h->cfg.width, B, bn_partials, gamma, beta, run_mean, run_var, coef, (float*)scratch, train,
                                  (hipStream_t)stream, tiles_per_partial);
}

int cvae_op_bn_pool_act_fwd(cvae_handle h, int32_t layer, int32_t B, const float* y, const float* bn_partials,
                            const float* gamma, const float* beta, float* run_mean, float* run_var, float* coef,
                            float* a, void* scratch, int32_t train, void* stream) {
    const int W = h->cfg.width;
    RC(launch_bn_fwd_finalize(layer, W, B, bn_partials, gamma, beta, run_mean, run_var, coef, (float*)scratch, train, (hipStream_t)stream));
    return launch_bn_pool_act_fwd(layer, W, B, y, coef, a, (hipStream_t)stream, io_bf16(h));     // y, a in the handle's storage type
}

int cvae_op_bn_pool_act_bwd(cvae_handle h, int32_t layer, int32_t B, const float* y, const float* a, const float* da,
                            const float* coef, const float* gamma, float* dy, float* dgamma, float* dbeta, float* dbias,
                            void* scratch, void* stream) {
    return launch_bn_pool_act_bwd(layer, h->cfg.width, B, y, a, da, coef, gamma, dy, dgamma, dbeta, dbias,
                                  (float*)scratch, (hipStream_t)stream, io_bf16(h));                 // y, a, da, dy in the handle's storage type
}

int64_t cvae_op_bn_partial_floats(cvae_handle h, int32_t layer, int32_t B) {
    return (int64_t)2 * bn_num_tiles(layer, h->cfg.width, B) * kLayers[layer].cout;
}

int64_t cvae_op_msssim_ws_floats(cvae_handle h, int32_t B) { return msssim_ws_floats(h->cfg.width, B); }

int cvae_op_msssim(cvae_handle h, int32_t B, const float* img1, const float* img2, void* ws, float* scalars,
                   float* d_img1, void* stream) {
    return launch_msssim(h->cfg.width, B, img1, img2, nullptr, nullptr, (float*)ws, scalars, d_img1, nullptr, nullptr,
                         (hipStream_t)stream);
}

// The latent-layer launchers of fc.hip, one per entry point.  flat / h_out / dh / dflat are in the handle's storage type.
static int latent_check(cvae_handle h, int32_t B, const char* who, bool pointers_ok) {
    if (!h) { cvae_set_error("%s: null handle", who); return CVAE_EINVAL; }
    if (B < 1 || B > h->cfg.max_batch) { cvae_set_error("%s: batch %d outside [1, %d]", who, B, h->cfg.max_batch); return CVAE_EINVAL; }
    if (!pointers_ok) { cvae_set_error("%s: null pointer", who); return CVAE_EINVAL; }
    return 0;
}

int64_t cvae_op_latent_scratch_floats(cvae_handle h, int32_t B) {
    if (!h || B < 1 || B > h->cfg.max_batch) { cvae_set_error("cvae_op_latent_scratch_floats: bad handle, or batch %d outside [1, max_batch]", B); return CVAE_EINVAL; }
    return fc_ws_floats(h->cfg.width, B);
}

// include/cvae.h: the grids of the latent launches at a batch, from the function the launchers call (host logic only, no device access)
int32_t cvae_op_latent_plan(int32_t width, int32_t B, int32_t num_cus, int32_t* out) {
    if ((width != 64 && width != 128) || B < 1 || num_cus < 1 || !out) {
        cvae_set_error("cvae_op_latent_plan: width %d not 64 / 128, batch %d or compute units %d below 1, or null pointer", width, B, num_cus);
        return CVAE_EINVAL;
    }
    const LatentPlan p = latent_plan(width, B, num_cus);
    const int dfl0 = p.fb_split ? 0 : p.fb_bgemm, cs0 = p.fb_bgemm + (p.fb_split ? 0 : p.fb_dflat);
    const int v[CVAE_LATENT_PLAN_INTS] = {p.fc_fwd_gemm, p.di_imgs, p.di_blocks,
                                          0, p.db_bgemm, p.db_bgemm, p.db_bgemm + p.db_gemm,
                                          p.df_imgs, 0, p.fb_bgemm, dfl0, dfl0 + p.fb_dflat, cs0, cs0 + p.fb_colsum, p.fb_split};
    for (int i = 0; i < CVAE_LATENT_PLAN_INTS; ++i) out[i] = v[i];
    return 0;
}

int cvae_op_fc_fwd(cvae_handle h, int32_t B, const float* flat, const float* wfc, const float* bfc, const float* eps,
                   const float* pred, float* mu, float* logvar, float* zcat, void* scratch, void* stream) {
    RC(latent_check(h, B, "cvae_op_fc_fwd", flat && wfc && bfc && eps && pred && mu && logvar && zcat && scratch));
    return launch_fc_fwd(h->cfg.width, B, flat, wfc, bfc, eps, pred, mu, logvar, zcat, (float*)scratch, (hipStream_t)stream, io_bf16(h));
}

int cvae_op_decin_fwd(cvae_handle h, int32_t B, const float* zcat, const float* wd, const float* bd, float* h_out, void* stream) {
    RC(latent_check(h, B, "cvae_op_decin_fwd", zcat && wd && bd && h_out));
    return launch_decin_fwd(h->cfg.width, B, zcat, wd, bd, h_out, (hipStream_t)stream, io_bf16(h));
}

int cvae_op_decin_bwd(cvae_handle h, int32_t B, const float* zcat, const float* dh, const float* wd, float* dwd, float* dbd,
                      float* dzcat, void* scratch, void* stream) {
    RC(latent_check(h, B, "cvae_op_decin_bwd", zcat && dh && wd && dwd && dbd && dzcat && scratch));
    return launch_decin_bwd(h->cfg.width, B, zcat, dh, wd, dwd, dbd, dzcat, (float*)scratch, (hipStream_t)stream, io_bf16(h));
}

int cvae_op_fc_bwd(cvae_handle h, int32_t B, const float* flat, const float* wfc, const float* dzcat, const float* eps,
                   const float* logvar, const float* dmu_loss, const float* dlv_loss, float* dwfc, float* dbfc, float* dflat,
                   void* scratch, void* stream) {
    RC(latent_check(h, B, "cvae_op_fc_bwd", flat && wfc && dzcat && eps && logvar && dmu_loss && dlv_loss && dwfc && dbfc && dflat && scratch));
    return launch_fc_bwd(h->cfg.width, B, flat, wfc, dzcat, eps, logvar, dmu_loss, dlv_loss, dwfc, dbfc, dflat, (float*)scratch,
                         (hipStream_t)stream, io_bf16(h));
}

}  // extern "C"
