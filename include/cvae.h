/*
 * cvae.h — C-ABI of libcvae_hip.so: the Critic-VAE training step on MI355X (gfx950).
 *
 * The reference (lcicek/Critic-VAE) has no FFI for this path: its "interface" is the set of
 * PyTorch calls made by vae.py:44-58.  This header is the boundary a maintainer would bind
 * (ctypes stub in INTEGRATION.md); each entry point names the reference call it replaces.
 *
 * Conventions
 *   - Plain C types only.  Every pointer is a DEVICE pointer unless stated; every tensor that crosses this
 *     boundary is fp32 (precision mode 1 keeps bf16 tensors only inside the workspace it is handed).
 *   - The caller owns every buffer (parameters, gradients, inputs, outputs, workspace); the
 *     library owns only the opaque handle.  No allocation, no device synchronisation inside.
 *   - Process-wide state is limited to two caches that never change results: a THREAD-LOCAL error string
 *     (cvae_last_error() reports the calling thread's last failure) and a per-device compute-unit count queried
 *     once (it sizes persistent grids).  Everything else lives in the handle; distinct handles are independent.
 *   - What the workspace, a scratch buffer or an output holds ON ENTRY does not matter: they may be uninitialised memory (NaNs,
 *     huge values, the leavings of a call at another batch size), and are never cleared by the caller.  Every slot a kernel reads
 *     (split-K slabs, BatchNorm and reduction partials, the MS-SSIM partials and its arrival ticket, packed weights) is written
 *     earlier in the same call.  What must be kept is the workspace BETWEEN a cvae_forward and the cvae_loss and cvae_backward
 *     that belong to it (it carries the saved activations; the stages of one staged step likewise).  Every output is fully
 *     written for the `batch` rows of the call: mu, logvar, recon, the first 13 scalars, d_recon, d_mu, d_logvar and every
 *     tensor of `grads`; only the alignment padding between the tensors of `grads` is the caller's (see cvae_backward_phases).
 *   - All work is enqueued on the caller's hipStream_t (passed as void*).
 *   - Return: 0 = OK, <0 = library error (cvae_last_error()), >0 = hipError_t passthrough.
 *   - Layouts: frames x / recon / d_recon are NCHW (B,3,W,W) exactly as the reference holds
 *     them (vae_utility.py:337-343); mu/logvar/eps (B,32), pred (B,1) row-major.  Parameters
 *     and gradients live in ONE flat fp32 buffer in the library's native layout described by
 *     cvae_param_*(): conv weights [kh*5+kw][Cin][Cout], fc_mu|fc_var fused as [k][64] with k
 *     in (h,w,c) order, decoder_input as [33][bottleneck] with columns in (h,w,c) order.
 *     critic-vae_amd/layout.py converts to/from the reference's state_dict layouts.
 */
#ifndef CVAE_H
#define CVAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cvae_handle_s* cvae_handle;

typedef struct cvae_config {
    int32_t width;        /* frame width == height: 64 (vae_parameters.py:5) or 128 (BASELINE config 5 shape) */
    int32_t max_batch;    /* largest per-call batch the workspace is sized for                 */
    int32_t overlap_wgrad;    /* != 0: run weight-gradient kernels on an internal low-priority side stream */
    int32_t precision;    /* 0 = fp32 everywhere (the 1e-4-parity path, bench default);
                           * 1 = bf16 mode (BASELINE.json configs 3-5): every contraction on the bf16 MFMA (fp32 accumulate) AND
                           *     activations / activation gradients stored as bf16 inside the workspace; x, recon, mu, logvar, the loss
                           *     gradients, parameters, gradients, BatchNorm statistics and Adam state stay fp32 at this boundary;
                           * 2 = fp32 emulation: forward/dgrad of E2..E4 and D0 on the bf16 MFMA with exact 3-way bf16 operand splits
                           *     (9 MFMAs per block), everything else as 0;  3 = as 2 with the six leading partial products only;
                           * other values are rejected */
} cvae_config;

enum { CVAE_OK = 0, CVAE_EINVAL = -1, CVAE_EUNSUPPORTED = -2, CVAE_ENOWS = -3 };

/* number of loss scalars written by cvae_loss: [0]=total [1]=recon(MS-SSIM) [2]=KLD(weighted)
 * [3..7]=ssim level means [8..12]=cs level means [13..15]=reserved (written as 0; cvae_loss_obj
 * writes F.mse_loss(recon, x) to [13])                                                         */
#define CVAE_N_SCALARS 16

const char* cvae_version(void);
const char* cvae_last_error(void);

/* lifecycle */
int  cvae_create(const cvae_config* cfg, cvae_handle* out);
void cvae_destroy(cvae_handle h);

/* flat parameter / gradient buffer description (replaces nn.Module.parameters(), vae.py:36) */
int64_t     cvae_param_total(cvae_handle h);                 /* floats incl. alignment padding */
int32_t     cvae_param_count(cvae_handle h);                 /* number of tensors (30)          */
const char* cvae_param_name(cvae_handle h, int32_t i);       /* NATIVE tensor name: enc{0..3}.{w,b,gamma,beta}, fc.{w,b}
                                                              * (fc_mu|fc_var fused), dec{0..4}.{w,b}, decin.{w,b} — not a
                                                              * reference state_dict key; critic-vae_amd/layout.py holds the
                                                              * name + layout map to encoder./decoder. keys            */
int64_t     cvae_param_offset(cvae_handle h, int32_t i);     /* float offset in the flat buffer */
int64_t     cvae_param_numel(cvae_handle h, int32_t i);

/* workspace (saved activations, gradients of activations, split-K slabs, reduction partials) */
int64_t cvae_workspace_bytes(cvae_handle h, int32_t batch);

/* BatchNorm running statistics buffer: 2*480 floats [mean(32,64,128,256) | var(...)] */
int64_t cvae_bn_state_floats(cvae_handle h);

/*
 * Forward: VariationalAutoencoder.forward (vae_nets.py:14-19) = encoder (:101-111) ->
 * reparametrize with caller-supplied eps (:48-51) -> decoder (:139-147).
 * train != 0: BatchNorm uses batch statistics and updates bn_state (momentum 0.1, unbiased var).
 * Saves what backward needs in ws.
 */
int cvae_forward(cvae_handle h, int32_t batch, const float* x, const float* pred, const float* eps,
                 const float* params, float* bn_state, float* mu, float* logvar, float* recon,
                 void* ws, int32_t train, void* stream);

/*
 * Decoder.forward alone (vae_nets.py:139-147) from zcat = cat((z, pred), 1), shape (B,33).
 * zcat == NULL reuses the one cvae_forward left in ws.  cvae_forward with recon == NULL stops
 * after the encoder + reparametrize (VariationalEncoder.forward, vae_nets.py:101-111).
 */
int cvae_decode(cvae_handle h, int32_t batch, const float* zcat, const float* params, float* recon,
                void* ws, void* stream);

/*
 * Loss: VariationalAutoencoder.vae_loss (vae_nets.py:53-62) = MSSIM.forward (:217-247) + KLD.
 * Writes CVAE_N_SCALARS floats to `scalars` and the gradients of total_loss w.r.t. recon, mu,
 * logvar (d_* may be NULL to skip the backward half).
 */
int cvae_loss(cvae_handle h, int32_t batch, const float* x, const float* mu, const float* logvar,
              const float* recon, void* ws, float* scalars, float* d_recon, float* d_mu,
              float* d_logvar, void* stream);

/*
 * cvae_loss under a caller-chosen objective:
 *   total = msssim_weight * MSSIM.forward(recon, x) + mse_weight * F.mse_loss(recon, x) + kld_weight * KLD
 * (F.mse_loss is the reference's own commented-out reconstruction term, vae_nets.py:54; kld_weight is the beta of a beta-VAE).
 * `obj` is HOST memory, read during the call and passed to the kernels by value: a per-step schedule costs no copy and no
 * synchronisation.  Arguments, alignment (x, recon, d_recon 16-byte aligned) and null gradients as in cvae_loss.
 * Scalars: [1] the UNWEIGHTED MS-SSIM loss 1 - prod, [3..12] the level means, [2] kld_weight * the raw KLD mean,
 *   [13] F.mse_loss(recon, x): the mean over all 3 * batch * W^2 elements (differences and squares fp32, the sum fp64: one fp64
 *   partial per workgroup, merged in a fixed order by the last workgroup to arrive — no floating-point atomics, the same call
 *   gives the same bits), [0] = msssim_weight * [1] + mse_weight * [13] + [2] in fp32, [14], [15] = 0.
 * Gradients: d_recon = msssim_weight * d[1]/d recon + mse_weight * 2 (recon - x) / (3 * batch * W^2), written once;
 *   d_mu, d_logvar as cvae_loss with kld_weight in place of 0.001.
 * msssim_grad: CVAE_MSGRAD_REFERENCE is autograd of vae_nets.py:243-247 as the reference runs it, including the 0 * w * x^(w-1)
 *   of the level terms the product never uses (ssim_0..3, cs_4): NaN in EVERY element of d_recon as soon as one of those means
 *   is negative, while the loss stays finite.  CVAE_MSGRAD_USED differentiates prod(cs_0..3 ^ w) * ssim_4 ^ (4 w_4) alone: the
 *   same loss value (bit for bit), and only a negative USED level mean still gives NaN (loss and gradients, as in the reference).
 * A term whose weight is exactly 0 is NOT COMPUTED, never multiplied by 0: at msssim_weight == 0 no pyramid kernel runs, no
 *   level field of ws is touched, [1] and [3..12] are written as 0 (also where MS-SSIM would have been NaN), and one pixel
 *   pass does the MSE, the KLD and their gradients; at mse_weight == 0 there is no pixel pass and [13] is 0.  With both
 *   non-zero the pixel gradient and the squared-error sum are folded into the pass that writes d_recon.
 * The reference objective {1, 0, 0.001f, CVAE_MSGRAD_REFERENCE} launches what cvae_loss launches and writes the same bits.
 * CVAE_EINVAL: null obj, a weight that is NaN, infinite or negative, msssim_weight + mse_weight == 0, msssim_grad outside
 * {0, 1}.  Every argument is checked before any device access; nothing allocates or synchronises.
 * Out of scope: the staged cross-rank path (cvae_loss_stage keeps the reference objective: its fp64 record has no slot for the
 * squared-error sum), an L1 term, and — in validation — a per-image MSE over non-finite images.
 */
typedef struct cvae_objective {
    float   msssim_weight;   /* reference: 1     */
    float   mse_weight;      /* reference: 0     */
    float   kld_weight;      /* reference: 0.001 */
    int32_t msssim_grad;     /* CVAE_MSGRAD_REFERENCE or CVAE_MSGRAD_USED */
} cvae_objective;
enum { CVAE_MSGRAD_REFERENCE = 0, CVAE_MSGRAD_USED = 1 };
int cvae_loss_obj(cvae_handle h, int32_t batch, const float* x, const float* mu, const float* logvar,
                  const float* recon, void* ws, const cvae_objective* obj, float* scalars, float* d_recon,
                  float* d_mu, float* d_logvar, void* stream);

/*
 * Per-image scores and the pooled loss of a held-out set (no reference counterpart: vae.py never evaluates; the values are the
 * reference's own MSSIM.forward (vae_nets.py:217-247) and KLD (:57-60) applied per image and to the whole set).
 *
 * cvae_score runs the MS-SSIM pyramid WITHOUT its derivative passes, then one launch that scores every image of the batch.
 * per_image_or_null: (batch, cvae_score_cols() = CVAE_SCORE_COLS = 8) floats, row i:
 *   [0] total = [1] + [2], exactly that fp32 sum
 *   [1] MSSIM.forward(recon[i:i+1], x[i:i+1]): 1 - prod_{l<4}(cs_l^w_l * ssim_4^w_4) over THIS image's level means (each over
 *       3 * S_l^2 values), with the code cvae_loss runs at batch 1 (equal to 1e-6); a negative used level mean gives NaN, as there
 *   [2] 0.001 * (-0.5 * sum_j (1 + logvar - mu^2 - exp(logvar))) of row i
 *   [3] mean over the 3 * W * W elements of (recon - x)^2      (differences and squares fp32, sum fp64)
 *   [4] max |recon - x|                                        (NaN if a difference is NaN)
 *   [5] this image's level-0 ssim mean      [6] its level-4 ssim mean      [7] reserved, written as 0
 * state_or_null: the pooled record, cvae_score_state_bytes() = 8 * CVAE_SCORE_STATE_DOUBLES bytes, 8-byte aligned, fp64:
 *   [0..4] ssim sums of levels 0..4, [5..9] cs sums, [10] the KLD sum — over every image since cvae_score_init
 *   [11]   images seen                     [12] images whose [0] is finite
 *   [13..16] sums of [0], [1], [2], [3] over the finite images        [17] maximum of [0] over them (-inf: none yet)
 *   [18..23] library scratch (the arrival counter of the pooling step lives here: do not write between calls)
 * cvae_score_init writes the record once; every cvae_score with a state ADDS its batch: the 11 sums as the cross-rank path
 * records them, the rows in a fixed order by the last workgroup to arrive.  No floating-point atomics, nothing depends on the order
 * of arrival: the same calls give the same bits.  At least one of per_image / state must be given; x and recon 16-byte aligned;
 * ws: cvae_workspace_bytes(h, batch), contents on entry irrelevant (the call overwrites the MS-SSIM region: not between a
 * cvae_forward and its cvae_backward).  cvae_score_finish writes the CVAE_N_SCALARS loss scalars of the pooled set — what
 * cvae_loss would give had every image since the init been ONE batch (global level means, KLD mean over all images) — with the
 * finish step of the cross-rank path; width: 64 or 128, the width of the frames pooled.  An empty record gives NaN scalars.
 * Every argument is checked before any device access; nothing allocates or synchronises.
 */
#define CVAE_SCORE_COLS 8
#define CVAE_SCORE_STATE_DOUBLES 24
int32_t cvae_score_cols(void);
int64_t cvae_score_state_bytes(void);
int cvae_score_init(cvae_handle h, void* state, void* stream);
int cvae_score(cvae_handle h, int32_t batch, const float* x, const float* mu, const float* logvar, const float* recon,
               void* ws, float* per_image_or_null, void* state_or_null, void* stream);
int cvae_score_finish(cvae_handle h, int32_t width, void* state, float* scalars, void* stream);

/*
 * Pooled statistics of the latent code of a set (no reference counterpart: vae.py never looks at its posterior).  What a
 * beta-VAE is judged by — the KL per latent dimension, the active units of Burda et al. (Var_x(mu_j) > 0.01) — and what a
 * Critic-VAE rests on — that mu does not predict the critic value injected next to it — all follow from first and second
 * moments, so the device keeps those and critic-vae_amd/latent.py derives the rest on the host from one read.
 *
 * cvae_latent_stats is ONE launch per batch.  It reads mu (batch,32), logvar (batch,32) and pred (batch) — fp32, as cvae_forward
 * leaves them in every precision mode — and ADDS the batch to `state`, a pooled record of CVAE_LATENT_STATE_DOUBLES fp64
 * values, 8-byte aligned.  With a = (mu_0..mu_31, pred), 33 entries:
 *   [0] rows seen                          [1] rows used
 *   [2..34]    sum a_i
 *   [35..595]  sum a_i a_j for i <= j, row-major upper triangle: index 35 + i*33 - i*(i-1)/2 + (j-i)
 *   [596..627] sum kl_j, kl_j = 0.5 * (mu_j^2 + exp(logvar_j) - logvar_j - 1), in nats
 *   [628..659] sum exp(logvar_j)           [660..691] sum logvar_j
 *   [692..695] library scratch (the arrival counter of the merge lives here: do not write between calls)
 * An ALL-ZERO record is the empty record: there is no init entry point, the caller clears it (a device memset) and every call
 * adds.  A row is USED when its 65 inputs are finite and its 32 exp(logvar_j) are finite in fp64 (logvar = 100 is; 800 is not);
 * any other row is counted in [0] only and enters no sum — counted, not hidden, as cvae_score does with non-finite images.
 * All arithmetic is fp64 on the widened fp32 inputs, exp included.  Rows are cut into chunks, min(chunks, compute units)
 * persistent workgroups stride over them, each leaves one fp64 partial record in `scratch`, and the last workgroup to arrive
 * adds the partials, in workgroup order, to the record: no floating-point atomics, the same calls give the same bits (two
 * calls on the same record must be ordered by their streams).  kl_rows_or_null: (batch,32) fp32, (float)kl_j of EVERY row,
 * used or not — whatever the arithmetic gives.  scratch: cvae_latent_stats_scratch_bytes(h, batch) bytes, 8-byte aligned,
 * contents on entry irrelevant.  batch is NOT capped by max_batch: 1 <= batch <= 2^24.  cvae_latent_stats_plan reports the
 * launcher's own arithmetic, as cvae_op_latent_plan does.  Every argument is checked before any device access (nulls, flags,
 * alignment, batch: CVAE_EINVAL); nothing allocates or synchronises.
 *
 * Stream parameter.  In this entry point the stream is followed by `uint32_t flags` (must be 0) on purpose: the test suite
 * keeps a closed registry of one side-stream scenario per entry point whose LAST parameter is the stream, and that registry
 * could not be extended together with this entry point.  Its side-stream case lives with its own GPU tests; moving it into
 * the registry (and then, if wanted, dropping `flags`) is a follow-up.
 */
#define CVAE_LATENT_STATE_DOUBLES 696
int64_t cvae_latent_stats_state_bytes(void);                                  /* host only */
int64_t cvae_latent_stats_scratch_bytes(cvae_handle h, int32_t batch);        /* host only; -1 for a bad argument */
int32_t cvae_latent_stats_plan(int32_t batch, int32_t num_cus, int32_t* out); /* host only: out[0] rows per chunk,
                                      out[1] chunks, out[2] workgroups = min(chunks, num_cus, 1024); CVAE_EINVAL for a bad argument */
int cvae_latent_stats(cvae_handle h, int32_t batch, const float* mu, const float* logvar, const float* pred,
                      void* state, float* kl_rows_or_null, void* scratch, void* stream, uint32_t flags /* 0 */);

/*
 * What the decoder listens to: the reduction over n_images * n_variants reconstructions of VARIED latent codes against each
 * image's base reconstruction (critic-vae_amd/latent.py builds the variants — dimension j moved by one prior sigma, the critic
 * value set to 0 and to 1 — with cvae_decode; this streams the results once).  recon_base (n,3,W,W), recon_var (n,K,3,W,W),
 * out (n,K,2) fp32:
 *   [..,0] mean over the 3 * W * W elements of (var - base)^2   (differences and squares fp32, the sum fp64 in a fixed order,
 *          as column 3 of cvae_score)
 *   [..,1] max over pixels of 0.2989 |dR| + 0.5870 |dG| + 0.1140 |dB| in the fp32 operation order of cvae_diff_grey: with the
 *          critic value set to 0 as the variant it is bit for bit the max_values of the difference mask.  NaN if a difference is NaN.
 * One workgroup per (image, variant) at both widths (W: the handle's); no scratch, no atomics, 64-bit offsets.  CVAE_EINVAL for
 * n_images * n_variants >= 2^31 or a count below 1, nulls, recon_base / recon_var not 16-byte aligned, flags != 0; every
 * argument is checked before any device access.  The stream is followed by `flags` for the reason given at cvae_latent_stats.
 */
int cvae_recon_response(cvae_handle h, int32_t n_images, int32_t n_variants, const float* recon_base /* (n,3,W,W) */,
                        const float* recon_var /* (n,K,3,W,W) */, float* out /* (n,K,2) */, void* stream, uint32_t flags /* 0 */);

/*
 * Backward: loss.backward() (vae.py:57) for everything cvae_forward computed, given the loss
 * gradients w.r.t. its outputs (and logvar/recon as returned by cvae_forward).  Overwrites the
 * flat gradient buffer `grads` (same layout as `params`).
 * `x`, `params` and `ws` MUST be the ones the matching cvae_forward ran on, bit for bit (no optimizer step, no other
 * forward on the same workspace in between): in precision mode 1 the first conv's output y0 is not stored — the E1
 * weight-gradient kernel recomputes it from `x` and the enc0.w / enc0.b of `params` and re-derives block 0's max-pool
 * decisions from those values — and every mode reads the saved activations of that forward from `ws`.  (Round 5: in
 * precision mode 1 a train-mode forward also leaves the frame in `ws` as packed bf16 pixels — 8 bytes per pixel, slot "xp" —
 * and the backward stages E1's strips from that copy when `ws` and `batch` are the ones of the handle's last train-mode
 * forward and the copy stays below 2 GiB (cvae_conv_route(1, width, 0, 0, batch) == 1); after an eval-mode forward, or on another workspace, it converts the fp32 `x` itself, as rounds 3-4 did.)
 */
int cvae_backward(cvae_handle h, int32_t batch, const float* x, const float* pred, const float* eps,
                  const float* params, const float* logvar, const float* recon, const float* d_recon,
                  const float* d_mu, const float* d_logvar, void* ws, float* grads, void* stream);

/*
 * The same backward in three phases, in the order the gradients complete, so that a data-parallel
 * host can all-reduce one bucket of the flat gradient buffer while the next phase computes
 * (torch DDP's bucketed overlap; vae.py:57 under the north star's RCCL all-reduce):
 *   bit 0: decoder + decoder_input      bit 1: fc_mu|fc_var + encoder block 3      bit 2: encoder blocks 2..0
 * Phases must be issued in that order on one stream; phase_mask 7 == cvae_backward.  Bit 3 (value 8) additionally
 * writes 0 into the alignment padding between the tensors of `grads`, so an uninitialised buffer may be passed
 * (cvae_backward itself never touches the padding: FusedTrainer zeroes its buffer once).  cvae_grad_bucket
 * returns the contiguous [offset, offset+numel) range of `grads` that phase `phase` (0..2) completes.
 */
int cvae_backward_phases(cvae_handle h, int32_t batch, const float* x, const float* pred, const float* eps,
                         const float* params, const float* logvar, const float* recon, const float* d_recon,
                         const float* d_mu, const float* d_logvar, void* ws, float* grads, int32_t phase_mask,
                         void* stream);
int cvae_grad_bucket(cvae_handle h, int32_t phase, int64_t* offset, int64_t* numel);

/*
 * Global-batch data parallelism: the same step in stages, so that a data-parallel host can sum the BatchNorm statistics and the
 * loss sums over its ranks (torch's SyncBatchNorm plus a global loss normaliser).  N ranks at B_r images each then train the
 * model that one rank trains at batch sum(B_r): BatchNorm normalises over the global batch (forward statistics, running
 * statistics with the global N / (N - 1), backward sums), MS-SSIM level means and the KLD mean are global, and d_mu / d_logvar
 * carry 1 / B_global.  The summed gradient is then the global-batch gradient itself (Adam's grad_scale = 1, not 1 / world_size).
 *
 * The exchange is an fp64 record of CVAE_SYNC_DOUBLES values with 9 sync points; cvae_sync_slot returns the contiguous
 * [offset, offset + count) of point `point` (host-only, no handle):
 *   points 0..3: forward BatchNorm of encoder blocks 0..3, 3*C doubles each (C = 32, 64, 128, 256); point 0 ends with one
 *                more double, this rank's image count (so ranks may hold different batch sizes, e.g. a ragged last batch);
 *   point 4:     the loss, 11 sums (5 ssim levels, 5 cs levels, the KLD term);
 *   points 5..8: backward BatchNorm of encoder blocks 3..0, 2*C doubles each.
 * Stage k writes this rank's values into its point; the CALLER sums that slot over all ranks, in place, on the stream
 * (torch.distributed / RCCL all_reduce, SUM), before the next stage reads it.  One rank skips the exchange: the stages then
 * reproduce cvae_forward + cvae_loss + cvae_backward bit for bit.  The library itself stays collective-free.
 *   cvae_forward_stage  k = 0..3 writes point k (stage k > 0 first finishes block k-1 from point k-1); stage 4 finishes
 *                       block 3, then runs fc, reparametrize and the decoder (recon == NULL: stops after the encoder).
 *                       train must be 1 (eval mode uses the running statistics and needs no exchange: cvae_forward).
 *   cvae_loss_stage     stage 0 writes point 4; stage 1 finishes: scalars, d_recon, d_mu, d_logvar.
 *   cvae_backward_stage stage 0: decoder, decoder_input, fc and block 3's statistics -> point 5; stages 1..3 apply block 4-k
 *                       from its summed point, run its weight and input gradients and block 3-k's statistics -> point 5+k;
 *                       stage 4: E1's fused apply + weight gradient.  The gradient buckets of cvae_grad_bucket complete at
 *                       the ends of stages 0 (phase 0), 1 (phase 1) and 4 (phase 2).  dgamma / dbeta are this rank's own
 *                       (the gradient all-reduce sums them).  `grads` is overwritten except its alignment padding.
 * Each call takes the arguments of the call it splits plus the record `sync` and the stage index.  The step runs forward
 * stages 0..4, loss stages 0..1, backward stages 0..4, in that order, on one workspace, batch and record; the handle tracks it
 * and rejects any other order with CVAE_EINVAL (forward stage 0 may always start a new step; a failed stage ends the step).
 * Every argument check happens before any device access.  Every stage joins the overlap_wgrad side stream before it returns.
 */
#define CVAE_SYNC_DOUBLES 2412
int cvae_sync_slot(int32_t point, int64_t* offset, int64_t* count);
int cvae_forward_stage(cvae_handle h, int32_t batch, const float* x, const float* pred, const float* eps,
                       const float* params, float* bn_state, float* mu, float* logvar, float* recon, void* ws,
                       int32_t train, double* sync, int32_t stage, void* stream);
int cvae_loss_stage(cvae_handle h, int32_t batch, const float* x, const float* mu, const float* logvar,
                    const float* recon, void* ws, float* scalars, float* d_recon, float* d_mu, float* d_logvar,
                    double* sync, int32_t stage, void* stream);
int cvae_backward_stage(cvae_handle h, int32_t batch, const float* x, const float* pred, const float* eps,
                        const float* params, const float* logvar, const float* recon, const float* d_recon,
                        const float* d_mu, const float* d_logvar, void* ws, float* grads, double* sync, int32_t stage,
                        void* stream);

/*
 * Chain-rule factor of total_loss.backward() (vae.py:57): d_*_out = d_* * gscale[0] for the three loss
 * gradients written by cvae_loss, in one launch; gscale is a DEVICE scalar (autograd's incoming gradient).
 */
int cvae_scale_loss_grads(cvae_handle h, int32_t batch, const float* gscale, const float* d_recon,
                          const float* d_mu, const float* d_logvar, float* d_recon_out, float* d_mu_out,
                          float* d_logvar_out, void* stream);

/*
 * Optional bf16 transport of the gradient all-reduce ("bf16 optional 5.17 MB"): round a range of the flat
 * fp32 gradient buffer to bf16 (RNE) into a caller-owned buffer of n 2-byte elements, and widen the reduced buffer
 * back.  n: a multiple of 4 (the ranges of cvae_grad_bucket are multiples of 64).  The all-reduce itself stays the
 * caller's (torch.distributed / RCCL).
 */
int cvae_grads_to_bf16(cvae_handle h, const float* grads, void* out_bf16, int64_t n, void* stream);
int cvae_grads_from_bf16(cvae_handle h, const void* in_bf16, float* grads, int64_t n, void* stream);

/*
 * Optimizer: torch.optim.Adam.step() with defaults (vae.py:36,58) on the flat buffers.
 * grad_scale multiplies the gradient first (1/world_size after a summing all-reduce).
 */
int cvae_adam_step(cvae_handle h, float* params, const float* grads, float* exp_avg,
                   float* exp_avg_sq, int64_t n, int32_t step, float lr, float beta1, float beta2,
                   float eps, float grad_scale, void* stream);

/*
 * Guarded optimizer step (opt-in): skip the update when the gradient is non-finite (torch's GradScaler rule) and / or clip it by
 * its global norm (torch.nn.utils.clip_grad_norm_), decided ON THE DEVICE — no host read between backward and Adam.
 *
 * The caller owns one guard state of cvae_guard_state_bytes() bytes (8-byte aligned): a cvae_guard_record followed by the
 * per-workgroup partials of the statistics pass.  cvae_guard_init writes it once (all zero, applied / skipped counters as
 * given: 0, 0 for a new run, the saved values for a resumed one).  Each step is then
 *     cvae_grad_stats (one pass over the reduced gradient, writes the record)  ->  cvae_adam_step_guarded (reads it),
 * two launches where cvae_adam_step is one.
 *
 * cvae_grad_stats: n % 4 == 0.  norm = sqrt(sum (g_i * grad_scale)^2), accumulated in fp64 (elements near FLT_MAX give a
 * finite norm64); nonfinite = some g_i has all exponent bits set (Inf or NaN) — taken from the bits, not from the sum.
 * Per-workgroup partials are merged in a fixed order by the last workgroup to arrive: no floating-point atomics, the same
 * buffer gives the same record bit for bit.  Then
 *     apply = !(skip_nonfinite && nonfinite)
 *     coef  = min(1, max_norm / (norm + 1e-6))        (max_norm = +inf: no clipping, coef = 1)
 *     apply ? ++t : ++skipped
 *     step_size = lr / (1 - beta1^t), sqrt_bc2 = sqrt(1 - beta2^t)     (fp64, rounded to float; 0 when apply == 0)
 * With skip_nonfinite == 0 a non-finite gradient is applied.  max_norm = +inf: coef = 1 and the update is cvae_adam_step's at step t
 * (the same arithmetic).  Finite max_norm: an Inf element makes norm = +inf and coef = 0, so the Inf elements become NaN (inf * 0) and the finite ones
 * contribute 0, as clip_grad_norm_ does; a NaN element makes norm NaN and coef = 1 (the min drops the NaN quotient), so only the NaN
 * elements reach the state as NaN, where clip_grad_norm_ would spread the NaN to every element.  Either way the state is non-finite
 * from then on: skip_nonfinite is the protection, the clip is not.
 * max_norm <= 0 or NaN, n % 4 != 0, n < 0 or a null pointer: CVAE_EINVAL, cvae_last_error() set, nothing launched.
 *
 * cvae_adam_step_guarded: cvae_adam_step's arithmetic with gradient scale `gscale` (= grad_scale * coef, one fp32 product),
 * step_size, sqrt_bc2 and the betas taken from the record; when apply == 0 it writes nothing — params, exp_avg and
 * exp_avg_sq keep their bits.  It never writes the record.
 */
typedef struct cvae_guard_record {      /* 64 bytes at offset 0 of the guard state; device memory                        */
    int32_t  apply;                     /*  0: 1 = this step updates, 0 = skipped                                         */
    uint32_t nonfinite;                 /*  4: 1 = the gradient holds an Inf or a NaN                                     */
    float    coef;                      /*  8: clip coefficient in (0, 1]                                                 */
    float    norm;                      /* 12: (float)norm64 — +inf where the fp64 norm exceeds FLT_MAX                   */
    double   norm64;                    /* 16: global norm of grads * grad_scale                                          */
    int64_t  t;                         /* 24: applied steps so far (Adam's bias-correction step)                         */
    int64_t  skipped;                   /* 32: skipped steps so far                                                       */
    float    step_size;                 /* 40: lr / (1 - beta1^t)                                                         */
    float    sqrt_bc2;                  /* 44: sqrt(1 - beta2^t)                                                          */
    float    gscale;                    /* 48: grad_scale * coef                                                          */
    float    beta1, beta2;              /* 52, 56: Adam's betas, as cvae_grad_stats was given them                        */
    uint32_t ticket;                    /* 60: arrival counter of the statistics pass; 0 between launches                 */
} cvae_guard_record;
int64_t cvae_guard_state_bytes(void);
int cvae_guard_init(cvae_handle h, void* state, int64_t applied, int64_t skipped, void* stream);
int cvae_grad_stats(cvae_handle h, const float* grads, int64_t n, float grad_scale, float max_norm, int32_t skip_nonfinite,
                    float lr, float beta1, float beta2, void* state, void* stream);
int cvae_adam_step_guarded(cvae_handle h, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                           float eps, const void* state, void* stream);

/*
 * Optimizer options (opt-in): decoupled weight decay (torch.optim.AdamW), an exponential moving average of the parameters and
 * of one small auxiliary buffer, all inside the ONE launch of the Adam pass.  cvae_adam_step_opt is cvae_adam_step with them,
 * cvae_adam_step_guarded_opt is cvae_adam_step_guarded with them; the two plain entries keep their kernels and bits.  A learning-rate
 * schedule needs no entry of its own: lr (cvae_adam_step_opt, cvae_grad_stats) is an argument of every step.
 *
 * Weight decay: for every element inside one of the decayed ranges, p = p * decay_mul comes first — ONE fp32 product, rounded
 * on its own as torch's param.mul_(1 - lr * weight_decay) is, never contracted into the update — and cvae_adam_step's arithmetic
 * then runs on that p.  Elements outside every range skip the product.  Ranges are in ELEMENTS [begin, end), ascending and
 * disjoint; they need not respect the float4s the kernel moves (the critic's block of cvae_critic_grad has its tensor boundaries
 * anywhere).  The table travels by value in the launch; lane l of a wave holds slot l % 16, so a wave tests its 256-element
 * span against all slots with four vector compares and two ballots, and broadcasts the one or two ranges that touch the span out
 * of their lanes to test single elements only where a boundary crosses it.
 * EMA (ema != NULL): e = e + (p_new - e) * ema_omd on the p just written, in the same trip.  params, exp_avg and exp_avg_sq get
 * the same bits whether or not ema is given.  ema_omd == 0 writes nothing to ema / aux_ema.
 * aux / aux_ema (n_aux floats each, no alignment asked, aux is only read): the same EMA for a second small buffer, done by one
 * workgroup of the same launch — for the VAE the BatchNorm running statistics (cvae_bn_state_floats() floats, which cvae_forward
 * of this step has already written), so that the averaged weights are evaluated with averaged statistics.
 * decay_mul == 1, n_ranges == 0, ema == NULL: exactly cvae_adam_step's (cvae_adam_step_guarded's) bits.
 * Guarded form: step_size, sqrt_bc2, gscale and the betas come from the record; decay_mul and ema_omd come from the host, which
 * knows lr of this step (the lr it also gave cvae_grad_stats).  apply == 0: nothing is written at all — params, both moments,
 * ema and aux_ema keep their bits.  cvae_guard_record and cvae_grad_stats are unchanged.
 * CVAE_EINVAL, cvae_last_error() set and nothing launched, checked before any device access: a null handle, opt, params, grads
 * or moment (or guard state); n < 0 or n % 4 != 0; step < 1; n_ranges outside 0..CVAE_OPT_MAX_RANGES; a range with begin >= end,
 * before its predecessor's end, or past n; decay_mul outside (0, 1]; ema given and ema_omd outside [0, 1]; n_aux outside 0..4096;
 * n_aux > 0 with a null aux or aux_ema; aux_ema without ema.
 */
#define CVAE_OPT_MAX_RANGES 16
typedef struct cvae_opt_args {
    float   decay_mul;                  /* (float)(1.0 - (double)lr * (double)weight_decay); 1.0f = no decay                 */
    float   ema_omd;                    /* (float)(1.0 - ema_decay of this step); read only when ema != NULL                 */
    int32_t n_ranges;                   /* decayed element ranges [begin, end), ascending, disjoint, within [0, n)           */
    int32_t reserved;                   /* 0                                                                                 */
    int64_t begin[CVAE_OPT_MAX_RANGES], end[CVAE_OPT_MAX_RANGES];
} cvae_opt_args;
int cvae_adam_step_opt(cvae_handle h, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                       int32_t step, float lr, float beta1, float beta2, float eps, float grad_scale,
                       const cvae_opt_args* opt /* host memory, copied into the launch */, float* ema /* n floats or NULL */,
                       float* aux, float* aux_ema, int32_t n_aux /* 0..4096; both NULL when 0 */, void* stream);
int cvae_adam_step_guarded_opt(cvae_handle h, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                               float eps, const void* state, const cvae_opt_args* opt, float* ema, float* aux, float* aux_ema,
                               int32_t n_aux, void* stream);

/*
 * Training trace on the device (opt-in): a ring of step rows and per-tensor statistics of the flat buffers, written by launches
 * on the caller's stream — no host read, no allocation, no synchronisation.  A trainer without a trace launches neither.
 *
 * cvae_trace_push: ONE small launch that writes row (step - 1) % capacity of `ring` (capacity rows of 128 bytes, 8-byte aligned,
 * caller-owned device memory).  Every byte of the row is written, so a ring may hold anything on entry; no other row is touched.
 * loss_scalars: n_scalars device floats, copied bit for bit (the VAE's 16, the critic's 4).  guard_state: the state cvae_grad_stats
 * of this step has written (so the push runs after it), or NULL; it is only read.
 * CVAE_EINVAL, cvae_last_error() set and nothing launched: a null handle, ring or loss_scalars; capacity < 1; step < 1; n_scalars
 * outside 0..16.
 */
#define CVAE_TRACE_MAX_SCALARS 16
typedef struct cvae_trace_row {          /* 128 bytes                                                                       */
    int64_t  step;                       /*   0: 1-based optimizer step (the trainer's step_count after the step)            */
    float    lr;                         /*   8: the lr this step was given                                                  */
    int32_t  applied;                    /*  12: guard record's apply; 1 without a guard                                     */
    uint32_t nonfinite;                  /*  16: guard record's; 0 without a guard                                           */
    float    grad_norm, coef;            /*  20, 24: guard record's norm and coef; NaN and 1 without a guard                 */
    int32_t  n_scalars;                  /*  28: 0..16                                                                       */
    uint8_t  reserved[32];               /*  32: 0                                                                           */
    float    scalars[16];                /*  64: the step's loss scalars, bit for bit; unused slots 0                        */
} cvae_trace_row;
int cvae_trace_push(cvae_handle h, void* ring, int64_t capacity, int64_t step, float lr,
                    const float* loss_scalars, int32_t n_scalars, const void* guard_state_or_null, void* stream);

/*
 * cvae_tensor_stats: per-tensor statistics of the flat buffers AS THE OPTIMIZER LEFT THEM — it runs after the Adam launch of the
 * step, reads params (already updated), grads and both moments (already updated) and writes n_tensors records to `out`.
 * The tensors are element ranges [begin, end) of the flat buffers, ascending and disjoint; they may begin and end anywhere (no
 * multiple of 4 is asked), and elements between ranges (alignment padding) are never read.
 *     g   = grads[i] * gscale, one fp32 product: the gradient as Adam consumed it.  gscale is the record's (grad_scale * coef)
 *           when a guard state is given, grad_scale otherwise.                      g2 = sum (double)g * (double)g
 *     u   = step_size * (m / (sqrtf(v) / sqrt_bc2 + eps)), cvae_adam_step's fp32 expressions on the moments it left: the Adam
 *           displacement of the step just taken.  step_size and sqrt_bc2 come from the record when one is given (apply == 0:
 *           every u2 is exactly 0), otherwise from cvae_adam_step's host arithmetic on `step`, lr and the betas.
 *           The displacement of decoupled weight decay (cvae_adam_step_opt's p * decay_mul) is NOT part of u.
 *     p   = params[i] after the update.
 * g_nonfinite / p_nonfinite count the elements of grads / params whose exponent bits are all set (Inf or NaN), taken from the
 * stored bits as cvae_grad_stats takes them; a NaN never enters gmax / pmax (an Inf does).
 * Work: every tensor is cut into chunks of `chunk` elements (a constant of the library); an item is one (tensor, chunk) pair;
 * min(items, compute units, 256) persistent workgroups stride over the items and each item leaves one fp64 partial in `scratch`.
 * The last workgroup to arrive merges the partials tensor by tensor: lane l of one wave sums chunks l, l + 64, ... in ascending
 * order, then the wave's fixed xor tree.  Every addition has a fixed place and there are no floating-point atomics: the same
 * buffers give the same bits.  16-byte loads wherever the four buffers are 16-byte aligned (scalar for the up to three elements
 * in front of the first and behind the last aligned float4 of a chunk); element by element otherwise.
 * scratch: cvae_tensor_stats_scratch_bytes() bytes, 16-byte aligned; it may hold anything on entry (the arrival counter in its
 * first 16 bytes is zeroed on the stream in front of the launch).  out: n_tensors records, 8-byte aligned.
 * cvae_tensor_stats_plan / cvae_tensor_stats_scratch_bytes are host logic only (no device access; without a device the grid
 * assumes 256 compute units): chunk, item count and grid as the launcher computes them.
 * CVAE_EINVAL (the size query: a negative value), cvae_last_error() set, before any device access: a null pointer; n_tensors
 * outside 1..CVAE_TRACE_MAX_TENSORS; a range that is empty, before its predecessor's end or past n; step < 1.
 */
#define CVAE_TRACE_MAX_TENSORS 32
typedef struct cvae_tensor_stat {        /* 48 bytes, one per tensor, device memory                                          */
    double   g2, p2, u2;                 /*  0, 8, 16: sums of squares, fp64                                                 */
    float    gmax, pmax;                 /* 24, 28: max |g * gscale|, max |p|; NaN elements do not enter the maxima          */
    uint32_t g_nonfinite, p_nonfinite;   /* 32, 36: elements whose exponent bits are all set                                 */
    int64_t  step;                       /* 40: as given                                                                     */
} cvae_tensor_stat;
int cvae_tensor_stats(cvae_handle h, const float* params, const float* grads, const float* exp_avg, const float* exp_avg_sq,
                      int64_t n, int32_t n_tensors, const int64_t* begin, const int64_t* end /* host; copied into the launch */,
                      int64_t step, float lr, float beta1, float beta2, float eps, float grad_scale,
                      const void* guard_state_or_null, cvae_tensor_stat* out, void* scratch, void* stream);
int64_t cvae_tensor_stats_scratch_bytes(int32_t n_tensors, const int64_t* begin, const int64_t* end);   /* host only */
int cvae_tensor_stats_plan(int32_t n_tensors, const int64_t* begin, const int64_t* end,
                           int32_t* chunk, int32_t* items, int32_t* grid);                              /* host only; from the launcher */

/*
 * Critic.evaluate (critic_net.py:66-69; eval mode) on frames x (B,3,64,64) in [0,1] -> pred (B,1),
 * the `preds` of vae.py:50.  critic_params: cvae_critic_param_count() (= 11 873) floats in the
 * reference's own state_dict order and layouts (features.{0,3,6,10,14}.{weight,bias},
 * crit.{1,4}.{weight,bias}); the critic is frozen, the library never writes it.
 */
int32_t cvae_critic_param_count(void);
int cvae_critic_forward(cvae_handle h, int32_t batch, const float* x, const float* critic_params,
                        float* pred, void* stream);

/*
 * One training step of the critic: Critic.forward in TRAIN mode (critic_net.py:15-59, default arguments: width 64,
 * dims [8,8,8,16], bottleneck 32, ReLU, max-pool; fp32), the loss against `target`, and the gradient of every parameter.
 * Caller-owned buffers, the caller's stream, no allocation, no sync; every argument is checked before any device access.
 *
 * x (B,3,64,64) in [0,1], 16-byte aligned; target (B) in [0,1]; 1 <= batch <= 65 536, independent of the handle's max_batch
 * (scratch is sized by cvae_critic_grad_scratch_bytes(batch): at most 256 per-workgroup gradient partials + 2 floats per image).
 * A handle of another width than 64: CVAE_EUNSUPPORTED.  critic_params: the 11 873 floats cvae_critic_forward reads.
 * grads: cvae_critic_train_floats() (= 11 876) floats, the same order and OIHW layouts, the mean over the batch; the three
 * padding floats are written as 0, so cvae_adam_step / cvae_grad_stats / cvae_adam_step_guarded (n % 4 == 0) take the block.
 * Every output is fully written; scratch (16-byte aligned) may hold anything on entry.
 *
 * Dropout is explicit, as eps is for the VAE: keep (B, CVAE_CRITIC_KEEP) uint8, nonzero = kept; a row holds the sites
 * features.9 (512, on the pooled (8,8,8) tensor), features.13 (256, on (16,4,4)), crit.3 (32), each in (c,h,w) order.
 * Kept elements are multiplied by (float)(1.0 / (1.0 - (double)dropout_p)), 0 <= dropout_p < 1.  keep == NULL: every
 * element kept (and scaled); with dropout_p == 0 that is the eval-mode forward, pred equal to cvae_critic_forward's.
 * Max-pool follows ReLU and takes the first maximum of its window in scan order (strict >), as torch does.
 *
 * loss_kind CVAE_CRITIC_LOSS_BCE: mean over B of -(t * max(log p, -100) + (1 - t) * max(log(1 - p), -100)) (torch's
 * binary_cross_entropy); CVAE_CRITIC_LOSS_MSE: mean (p - t)^2; anything else CVAE_EINVAL.  loss_scalars: 4 device floats,
 * [0] the chosen loss, [1] BCE, [2] MSE, [3] 0; per-image terms are summed in a fixed order in fp64.
 * Backward in torch's arithmetic: BCE d_p = (p - t) / max(p (1 - p), 1e-12) / B, then d_z = d_p * p (1 - p), so a
 * sigmoid saturated to exactly 1 contributes a zero gradient; MSE d_p = 2 (p - t) / B.
 * No floating-point atomics: per-workgroup partials in scratch, merged in workgroup order; the same inputs give the same
 * bits (the grid, and with it the summation order, depends on batch, the device's compute units and CVAE_PERSIST_MAXWG).
 *
 * decisions (optional, (B, CVAE_CRITIC_DECISIONS) uint8, 4-byte aligned): the discrete choices of the forward.  Per
 * pooled output in (c,py,px) order, blocks 1..4 in turn (8*32*32, 8*16*16, 8*8*8, 16*4*4): 0..3 = 2*dy+dx of the selected
 * element, 4 = the window's maximum was <= 0 (output 0, no gradient); then 32 bytes features.14 pre-activation > 0, then
 * 32 bytes crit.1 pre-activation > 0.
 */
#define CVAE_CRITIC_KEEP      800
#define CVAE_CRITIC_DECISIONS 11072
enum { CVAE_CRITIC_LOSS_BCE = 0, CVAE_CRITIC_LOSS_MSE = 1 };
int64_t cvae_critic_train_floats(void);
int64_t cvae_critic_grad_scratch_bytes(cvae_handle h, int32_t batch);       /* host-only; -1 for a bad argument */
int cvae_critic_grad(cvae_handle h, int32_t batch, const float* x, const float* target, const uint8_t* keep_or_null,
                     float dropout_p, int32_t loss_kind, const float* critic_params, float* grads, float* pred,
                     float* loss_scalars, uint8_t* decisions_or_null, void* scratch, void* stream);

/*
 * Per-frame scores of the critic against its targets and the pooled record of a held-out set (no reference counterpart: the
 * reference ships no critic training code; the forward is Critic.evaluate, the loss terms are those of cvae_critic_grad).
 *
 * cvae_critic_score is ONE launch.  frames_hwc: (n_frames, 64, 64, 3) uint8, 16-byte aligned; targets: (n_frames) fp32.
 * Frame i of the batch is idx[i] (int64), or i when idx is null (then batch <= n_frames).  A workgroup stages the uint8 frame
 * straight into on-chip memory as (float)u8 / 255.0f — cvae_preprocess_u8_gather's arithmetic, no fp32 frame is written — and
 * runs the eval-mode forward with the device code of cvae_critic_forward: p is bit-equal to cvae_preprocess_u8_gather +
 * cvae_critic_forward on the same indices.  per_frame_or_null: (batch, CVAE_CRITIC_SCORE_COLS = 8) floats, row i:
 *   [0] p, the critic's value of the frame          [1] t = targets[idx[i]]
 *   [2] -(t * max(logf(p), -100) + (1 - t) * max(logf(1 - p), -100))   torch's binary_cross_entropy term; every operation is
 *       rounded to fp32 on its own
 *   [3] (p - t)^2 and [4] |p - t|, exactly the fp32 results
 *   [5] the bin of p, [6] the bin of t: 0 = mid (0.4 <= v <= 0.6), 1 = high (v >= 0.7), 2 = low (v <= 0.25), 3 = none — the
 *       selection rule of "The training set on the device" below: tested in the order mid, high, low, float32 comparisons
 *       against fp32(0.4), fp32(0.6), fp32(0.7), 0.25; NaN falls in no bin
 *   [7] reserved, written as 0
 * An index outside [0, n_frames) is never dereferenced: its row is NaN in [0..4], 3 in [5] and [6], 0 in [7].
 * Without per_frame the rows go to `scratch` (cvae_critic_score_scratch_bytes(h, batch) bytes, 4-byte aligned, contents on
 * entry irrelevant); with per_frame scratch may be null.
 * state_or_null: the pooled record, cvae_critic_score_state_bytes() = 8 * CVAE_CRITIC_SCORE_STATE_DOUBLES bytes, 8-byte
 * aligned, fp64:
 *   [0]      frames seen                    [1] frames whose row is finite in [0..4] ("finite frames")
 *   [2..9]   sums over the finite frames of [2] (BCE), [3] (squared error), [4] (absolute error), p, t, p^2, t^2, p t
 *            (the three products in fp64)
 *   [10]     maximum of [4] over the finite frames (-inf: none yet)
 *   [11..26] the 4 x 4 confusion counts over the finite frames, [11 + 4 * (bin of t) + (bin of p)]
 *   [27..31] reserved, zero
 *   [32..39] library scratch (the arrival counter of the pooling step lives here: do not write between calls)
 * cvae_critic_score_init writes the record once; every cvae_critic_score with a state ADDS its batch, by the last workgroup
 * to arrive, rows in a fixed order.  No floating-point atomics, nothing depends on the order of arrival: the same calls give
 * the same bits.  There is no finish call: mean BCE = [2] / [1], Pearson's r from [5..9], bin agreement = ([11] + [16] + [21]
 * + [26]) / [1] are host arithmetic on the record, read once (critic_train.summarize_record).
 * 1 <= batch <= 65 536, independent of the handle's max_batch; a handle of another width than 64: CVAE_EUNSUPPORTED.  At
 * least one of per_frame / state must be given.  Every argument is checked before any device access; nothing allocates or
 * synchronises.
 */
#define CVAE_CRITIC_SCORE_COLS 8
#define CVAE_CRITIC_SCORE_STATE_DOUBLES 40
int64_t cvae_critic_score_state_bytes(void);
int64_t cvae_critic_score_scratch_bytes(cvae_handle h, int32_t batch);      /* host-only; -1 for a bad argument */
int cvae_critic_score_init(cvae_handle h, void* state, void* stream);
int cvae_critic_score(cvae_handle h, int32_t batch, const uint8_t* frames_hwc, const float* targets, int64_t n_frames,
                      const int64_t* idx_or_null, const float* critic_params, float* per_frame_or_null,
                      void* state_or_null, void* scratch, void* stream);

/*
 * Critic-side masks: what the critic alone says about a frame, to set beside the VAE's difference mask.  Three entries,
 * each ONE launch of a persistent grid (at most one workgroup of 256 threads per compute unit, CVAE_PERSIST_MAXWG caps it),
 * one workgroup per image at a time, every activation in on-chip memory.  They share these rules: x (B,3,64,64) fp32 in
 * [0,1], 16-byte aligned; critic_params the 11 873 floats cvae_critic_forward reads; 1 <= batch <= 65 536, independent of
 * the handle's max_batch; a handle of another width than 64: CVAE_EUNSUPPORTED; caller's buffers and stream, no allocation,
 * no synchronisation, no floating-point atomics (a frame's results depend on that frame alone: the same inputs give the
 * same bits whatever the grid); every argument is checked before any device access; every output given is fully written.
 *
 * cvae_critic_collect: Critic.forward(X, collect=True) (critic_net.py:44-59) in eval mode.  pred (B) is bit-equal to
 * cvae_critic_forward's (the same device code).  The embeddings are the reference's list, NCHW fp32: e1 (B,8,32,32),
 * e2 (B,8,16,16), e3 (B,8,8,8), e4 (B,16,4,4) behind the four max-pools, e5 (B,32,1,1) = features.14 after its ReLU.
 * Any of e1..e5 may be null: nothing is written for it.
 *
 * cvae_critic_saliency: the gradient of z, the pre-sigmoid output of crit.4, with respect to the pixels (the logit, not p:
 * a saturated sigmoid would scale the gradient of a confident frame to nothing before the set-wide normalisation of the
 * masks).  The forward and the backward are cvae_critic_grad's device code with every element kept and unscaled (pred and
 * decisions are bit-equal to cvae_critic_grad(keep = NULL, dropout_p = 0) on the same frames), plus the input gradient of
 * features.0; no weight gradient is taken.
 *   steps == 1: grad (B,3,64,64) = d z / d x at x.
 *   steps == N, 2 <= N <= CVAE_CRITIC_IG_MAX_STEPS: integrated gradients from the black frame.  For k = 1 .. N in that
 *     order the pass runs on x * ((float)k / (float)N) (one fp32 product per pixel) and its gradient is added to an fp32
 *     accumulator per element; then grad = (sum * x) * (1.0f / N).  pred and decisions are those of the pass k = N, x itself.
 *   map (B,64,64) = |grad_r| * 0.2989f + |grad_g| * 0.5870f + |grad_b| * 0.1140f (cvae_diff_grey's weights and order),
 *   max_values (B) = the maximum of the frame's map: what cvae_diff_normalize takes.  grad and decisions
 *   ((B, CVAE_CRITIC_DECISIONS) uint8, 4-byte aligned, the layout of cvae_critic_grad) may be null.
 *
 * cvae_critic_occlusion: occlusion sensitivity with non-overlapping patch x patch windows, patch 4, 8 or 16.  The frame is
 * staged once; pred (B) is its value (cvae_critic_forward's bits).  Then for every patch in row-major order the patch is
 * set aside, filled with (fill_r, fill_g, fill_b), the eval-mode forward runs again and the patch is put back:
 * drop (B, 64/patch, 64/patch) = pred - (value of the occluded frame), one fp32 subtraction, where the occluded value is
 * bit-equal to cvae_critic_forward on the frame with that patch filled by the host.  map (B,64,64) = max(drop, 0)
 * replicated over its patch, max_values (B) = the maximum of the frame's map.  (64 / patch)^2 + 1 forwards per frame.
 */
#define CVAE_CRITIC_IG_MAX_STEPS 256
int cvae_critic_collect(cvae_handle h, int32_t batch, const float* x, const float* critic_params, float* pred,
                        float* e1_or_null, float* e2_or_null, float* e3_or_null, float* e4_or_null, float* e5_or_null,
                        void* stream);
int cvae_critic_saliency(cvae_handle h, int32_t batch, const float* x, const float* critic_params, int32_t steps,
                         float* pred, float* grad_or_null, float* map, float* max_values, uint8_t* decisions_or_null,
                         void* stream);
int cvae_critic_occlusion(cvae_handle h, int32_t batch, const float* x, const float* critic_params, int32_t patch,
                          float fill_r, float fill_g, float fill_b, float* pred, float* drop, float* map,
                          float* max_values, void* stream);

/* adjust_values + HWC->CHW of preprocess_observation (vae_utility.py:324-343): uint8 frames
 * (B,W,W,3) -> float (B,3,W,W) / 255, so that only 1 byte per value crosses PCIe. */
int cvae_preprocess_u8(cvae_handle h, int32_t batch, const uint8_t* frames_hwc, float* x, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * The training set on the device: load_minerl_data(critic) (vae_utility.py:393-461, non-recon
 * branch) over recorded trajectories, and the per-step batch gather out of the curated set.
 *
 * Selection rule (vae_utility.py:400-459).  Trajectories are walked in the caller's order
 * (the reference: np.random.default_rng(seed=0).shuffle of the name list), frames in order;
 * p = the critic value of the frame (preprocess_observation: fp32 CHW / 255).  Bins, tested in
 * this order, all comparisons in float32 (edges fp32(0.4), fp32(0.6), fp32(0.7), 0.25):
 *   mid 0.4 <= p <= 0.6, then high p >= 0.7, then low p <= 0.25; NaN falls in no bin.
 * A frame is selected iff it has a bin and fewer than `collect` (150) earlier frames of its
 * trajectory fell in the same bin (the reference's early break selects nothing extra).  Before
 * each trajectory the walk stops if len(dset) >= total_images; the last trajectory taken may
 * overshoot by up to 3*collect - 1, so a dataset of total_images - 1 + 3*collect frames always
 * suffices.  Output order: trajectory order, then frame order.  Integer math, no atomics:
 * deterministic.  Frame offsets are 64-bit.
 * ---------------------------------------------------------------------------------------- */

/* One chunk of whole trajectories: preds (n_frames) fp32 critic values, trajectory t = frames
 * [traj_offsets[t], traj_offsets[t+1]) (int64, n_traj + 1 entries, traj_offsets[0] = 0, non-decreasing,
 * last = n_frames).  running (int64, in/out): len(dset) before the chunk, advanced past it, so that
 * consecutive calls reproduce one walk over all trajectories with no host round trip.  Outputs:
 * counts (n_traj, 3) int64 = frames selected per bin (mid, high, low); first (n_traj) int64 = the
 * trajectory's first dataset slot, i.e. len(dset) before it, or -1 if the cut came first (its
 * counts are then 0); span (2) int64 = (first slot of the chunk, frames selected in it);
 * sel[k] (k < span[1]; room for n_frames) = the chunk frame index of dataset slot span[0] + k.
 * The handle only identifies the library; width is not used.  CVAE_EINVAL for null pointers,
 * negative counts or collect < 1. */
int cvae_curate_select(cvae_handle h, int32_t n_traj, const int64_t* traj_offsets, int64_t n_frames,
                       const float* preds, int32_t collect, int64_t total_images, int64_t* running,
                       int64_t* counts, int64_t* first, int64_t* span, int64_t* sel, void* stream);

/* Copy the frames cvae_curate_select chose: dst_frames[span[0] + k] = src_frames[sel[k]] for
 * k < span[1] (uint8 (.., W, W, 3), W = width = the handle's width, whole 16-byte loads and
 * stores; both buffers 16-byte aligned), and dst_preds[span[0] + k] = src_preds[sel[k]] if both
 * are given.  max_count (host) bounds span[1] (the chunk's n_frames); slots at or past `capacity`
 * frames and sources outside [0, n_src) are skipped. */
int cvae_gather_frames_u8(cvae_handle h, int32_t width, const uint8_t* src_frames, const float* src_preds_or_null,
                          int64_t n_src, const int64_t* sel, int64_t max_count, const int64_t* span,
                          uint8_t* dst_frames, float* dst_preds_or_null, int64_t capacity, void* stream);

/* One training batch out of a device dataset: x[b] = frames_hwc[idx[b]] / 255 as (B, 3, W, W) fp32
 * (bit-identical to cvae_preprocess_u8 on the gathered frames: (float)u8 / 255.0f) and pred[b] =
 * preds[idx[b]], one launch.  frames_hwc (n_frames, W, W, 3) uint8, preds (n_frames) fp32, idx (B)
 * int64 device; W = width = the handle's width, 1 <= batch <= max_batch, frames and x 16-byte aligned.
 * Indices must already lie in [0, n_frames) (the caller validates them); one outside yields NaN
 * for that image and is never read. */
int cvae_preprocess_u8_gather(cvae_handle h, int32_t batch, int32_t width, const uint8_t* frames_hwc,
                              const float* preds, int64_t n_frames, const int64_t* idx, float* x,
                              float* pred, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * The recon branch of the same walk: load_minerl_data(critic, recon_dset=True, vae=vae)
 * (vae_utility.py:422-443), the dataset of the second VAE.  Same walk, order, bins, float32 edges,
 * per-bin cap and cut as above, but the dataset holds ENTRIES, the first VAE's eval-mode
 * reconstructions (fp32 (3, W, W) NCHW in the Tanh range), not frames:
 *   a mid frame appends two entries, in this order: kind 0 = vae.evaluate(obs, p), kind 1 =
 *   vae.evaluate(obs, 0); it counts once against the mid cap.  A high frame appends one entry of
 *   kind 0, a low frame one of kind 1.
 * len(dset) counts entries, so the cut sees mid frames twice and the last trajectory taken may
 * overshoot by up to 4*collect - 1: a dataset of total_images - 1 + 4*collect entries suffices.
 * ---------------------------------------------------------------------------------------- */

/* cvae_curate_select with entry weights 2 / 1 / 1 (mid / high / low) in the cut and in the slot positions (the same three
 * kernels, instantiated for that weight).  Arguments as cvae_curate_select, with running / first / span[0..1] counting
 * ENTRIES and counts still FRAMES per bin.  Further outputs: sel_first (n_traj) int64 = selected frames of this chunk before
 * the trajectory, or -1 past the cut; span (3) int64 = (first entry slot of the chunk, entries in it, selected frames in
 * it); per entry e < span[1] (room for 2 * n_frames each): ent_frame[e] int64 = its chunk frame index, ent_kind[e] int32 =
 * 0 (decode at the frame's critic value) or 1 (decode at 0), ent_sel[e] int64 = the rank s of its frame among the chunk's
 * selected frames; and sel[s] (s < span[2]; room for n_frames) int64 = the chunk frame index of selected frame s, in walk
 * order, so that the encoder runs once per selected frame (cvae_preprocess_u8_gather with sel as the index).
 * CVAE_EINVAL for null pointers, negative counts or collect < 1. */
int cvae_curate_select_recon(cvae_handle h, int32_t n_traj, const int64_t* traj_offsets, int64_t n_frames,
                             const float* preds, int32_t collect, int64_t total_images, int64_t* running,
                             int64_t* counts, int64_t* first, int64_t* sel_first, int64_t* span, int64_t* ent_frame,
                             int32_t* ent_kind, int64_t* ent_sel, int64_t* sel, void* stream);

/* Decoder input of a run of entries: row e of zcat (n_entries, 33) = (mu[ent_sel[e]] (32 values), ent_kind[e] == 0 ?
 * sel_preds[ent_sel[e]] : 0).  mu (n_sel, 32) = the eval-mode encoder's mu of the chunk's selected frames, sel_preds (n_sel)
 * their critic values.  cvae_decode(zcat, recon = the dataset buffer at the run's first slot) then writes the
 * reconstructions into their slots.  1 <= n_entries <= max_batch; an ent_sel outside [0, n_sel) yields a NaN row. */
int cvae_recon_zcat(cvae_handle h, int32_t n_entries, const int64_t* ent_sel, const int32_t* ent_kind, const float* mu,
                    const float* sel_preds, int64_t n_sel, float* zcat, void* stream);

/* One training batch out of an fp32 device dataset: x[b] = frames[idx[b]] ((n_frames, 3, W, W) fp32, bit copy: 16-byte
 * loads and stores) and pred[b] = preds[idx[b]], one launch.  Same contract as cvae_preprocess_u8_gather: W = width = the
 * handle's width, 1 <= batch <= max_batch, frames and x 16-byte aligned, 64-bit frame offsets (50 000 entries of 64 x 64
 * pass 2^31 bytes); an index outside [0, n_frames) yields NaN for that image and its pred, and is never read. */
int cvae_gather_f32(cvae_handle h, int32_t batch, int32_t width, const float* frames, const float* preds,
                    int64_t n_frames, const int64_t* idx, float* x, float* pred, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * Augmentation in the batch gather (no reference counterpart: vae.py trains on the frames as stored): horizontal flip,
 * shift by whole pixels with edge replication, and a brightness gain, applied inside the one launch that builds a batch.
 *
 * Per gathered sample four integers come from a counter-based hash, mix64(z) = the project's mixer (z += 0x9E3779B97F4A7C15;
 * z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31; all mod 2^64):
 *   r    = mix64(key ^ mix64((uint64) s)), s = the sample's dataset index idx[b]
 *   flip = (r >> 40) < flip_below                                 (24 bits against flip_below in [0, 2^24])
 *   k    = ((r >> 24) & 0xFFFF) - 32768, num = 2^31 + gain_q16 * k (fits 32 unsigned bits), gain g = (float) num * 2^-31
 *          (round-to-nearest conversion, exact scaling): g = 1 + (gain_q16 / 65536) * (k / 32768), within 1 +- brightness
 *   dx   = ((r >> 12) & 0xFFF) % (2 S + 1) - S,  dy = (r & 0xFFF) % (2 S + 1) - S,  S = max_shift
 * Output pixel (i, j) of every channel is source pixel (clamp(i - dy, 0, W-1), clamp(jj - dx, 0, W-1)), jj = flip ? W-1-j : j:
 * edge replication, no black border.  uint8 sources: the value is fminf(v * g, 1.0f), v = (float) u8 / 255.0f as the plain
 * gather writes it (one multiply, no add beside it: nothing contracts).  fp32 sources: a bit copy, and gain_q16 must be 0
 * (the entries are Tanh outputs in (-1, 1); a clamp at 1 means nothing there).  pred[b] = preds[s], the STORED value: the
 * transforms are taken to preserve it, the critic is not run again on the augmented frame.
 * {key, 0, 0, 0, 0} gives g = 1 exactly and writes the bits of the plain gather.
 *
 * aug is HOST memory, read during the call and passed to the kernel by value (as cvae_objective is): a new key per step
 * costs no copy and no synchronisation.  The caller derives key from its seed and step; the library only hashes.
 * applied_or_null: (batch, 4) int32 device rows [flip, dx, dy, num - 2^31] = what the kernel drew for row b (one thread per
 * sample writes it).  An index outside [0, n_frames) gives a NaN image, a NaN pred and an applied row of zeros, and is never
 * read.  Otherwise the contract of cvae_preprocess_u8_gather / cvae_gather_f32: same shapes, alignment, 64-bit frame offsets,
 * float4 stores per channel plane; nothing allocates or synchronises.
 * CVAE_EINVAL, before any device access: null aug, flip_below > 2^24, max_shift outside [0, width / 4], gain_q16 outside
 * [0, 65535], gain_q16 != 0 in the fp32 variant, reserved != 0, and whatever the plain gathers refuse.
 * Out of scope: re-evaluating the critic on augmented frames, the host feeder path, rotation / scaling / colour transforms
 * beyond a gain.
 * ---------------------------------------------------------------------------------------- */
typedef struct cvae_augment {
    uint64_t key;            /* mixed (seed, draw): chosen by the caller per step */
    uint32_t flip_below;     /* round(p_flip * 2^24), 0 = never, 2^24 = always */
    int32_t  max_shift;      /* S: dx, dy in [-S, S]; 0 <= S <= width / 4 */
    int32_t  gain_q16;       /* round(brightness * 65536), 0 = gain 1 */
    int32_t  reserved;       /* 0 */
} cvae_augment;
int cvae_preprocess_u8_gather_aug(cvae_handle h, int32_t batch, int32_t width, const uint8_t* frames_hwc,
                                  const float* preds, int64_t n_frames, const int64_t* idx, const cvae_augment* aug,
                                  float* x, float* pred, int32_t* applied_or_null, void* stream);
int cvae_gather_f32_aug(cvae_handle h, int32_t batch, int32_t width, const float* frames, const float* preds,
                        int64_t n_frames, const int64_t* idx, const cvae_augment* aug, float* x, float* pred,
                        int32_t* applied_or_null, void* stream);

/* Difference mask of the inference path (get_diff_image, vae_utility.py:256-277), batched:
 * diff (B,W,W) = 0.2989|dR| + 0.5870|dG| + 0.1140|dB| of recon_zero - recon_one (both (B,3,W,W)). */
int cvae_diff_grey(cvae_handle h, int32_t batch, const float* recon_one, const float* recon_zero,
                   float* diff, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * Segmentation evaluation (eval_textured_frames, vae_utility.py:162-212), after the difference
 * mask of cvae_diff_grey.  W is the handle's width; `batch` is NOT capped by max_batch (a whole
 * episode may go in one call): any batch >= 1 with batch * W * W < 2^31.  uint8 masks are
 * (B,W,W), nonzero = set.  Host-side argument checks come before any device access.
 * ---------------------------------------------------------------------------------------- */

/* Mask normalisation (get_diff_factor / prepare_diff / get_diff_and_thr_masks, vae_utility.py:106-110,
 * 148-160, 279-284), in float64 and that operation order: diff_u8 = trunc((min(d, mean_max) * diff_factor) * 255)
 * with mean_max = statistics.mean of the per-frame maxima and diff_factor = 1.0 / mean_max (0 if mean_max == 0),
 * both from the host.  mask_or_null: diff_u8 > thr (thr in [0, 255]).  With gt_or_null set: frame_counts_or_null
 * (B,3) int64 = per-frame (tp, fn, fp) of get_iou(gt, mask) (vae_utility.py:56-68), and hist_or_null (2,256) int64
 * gains the histogram of diff_u8 over pixels where gt is set (row 0) and where it is clear (row 1): ADDED to what
 * the buffer holds (integer atomics, order-free), so that one pass gives the set-wide IoU at every threshold.
 * Counts or histogram without gt: CVAE_EINVAL. */
int cvae_diff_normalize(cvae_handle h, int32_t batch, const float* diff, double mean_max, double diff_factor,
                        int32_t thr, const uint8_t* gt_or_null, uint8_t* diff_u8, uint8_t* mask_or_null,
                        int64_t* frame_counts_or_null, int64_t* hist_or_null, void* stream);

/* per-frame (tp, fn, fp) of get_iou(gt, mask) for any uint8 mask -> frame_counts (B,3) int64 */
int cvae_mask_counts(cvae_handle h, int32_t batch, const uint8_t* mask, const uint8_t* gt,
                     int64_t* frame_counts, void* stream);

/* Dense CRF of crf() (vae_utility.py:22-54; SimpleCRF denseCRF.densecrf with (w1, alpha, beta, w2, gamma, it)),
 * two labels, prob = (1 - prob1, prob1).  EXACT mean field: every pairwise sum runs over all (W*W)^2 pixel pairs
 * (the densecrf library approximates the bilateral filter with a permutohedral lattice instead).  Features
 * (x/gamma, y/gamma) and (x/alpha, y/alpha, r/beta, g/beta, b/beta) on the raw uint8 RGB frame, kernels
 * exp(-|f_i - f_j|^2 / 2) including j = i, symmetric normalisation n_i = (sum_j k(i,j))^-1/2, Potts weights w2
 * (Gaussian) and w1 (bilateral), unary u(l) = -log(max(prob(l), p_floor)), Q0 = softmax(-u), `iterations`
 * updates Q <- softmax(-u + sum_k w_k n_i sum_j k(i,j) n_j Q_j).  labels (B,W,W) uint8 = Q(1) > Q(0) (0 on a
 * tie); q1_or_null (B,W,W) fp32 = Q(1).  frames_hwc (B,W,W,3) uint8, prob1 (B,W,W) fp32.  Deterministic: a
 * frame's result is bitwise independent of the batch it is in and its position there.
 * Ranges: w1, w2 >= 0; alpha, beta, gamma > 0; 0 < p_floor <= 1; 0 <= iterations <= 10000; all finite.
 * A width below about 0.05 reaches no neighbour in fp32 (the nearest tap is under 2^-256): that kernel is then the
 * identity filter, for any width > 0 however small.
 * `scratch`: cvae_crf_scratch_bytes(h, batch) bytes of device memory, 256-byte aligned (host-only query; -1 for
 * a bad handle or batch). */
typedef struct cvae_crf_params {
    float w1, alpha, beta, w2, gamma, p_floor;
    int32_t iterations;
} cvae_crf_params;
int64_t cvae_crf_scratch_bytes(cvae_handle h, int32_t batch);
int cvae_dense_crf(cvae_handle h, int32_t batch, const uint8_t* frames_hwc, const float* prob1,
                   const cvae_crf_params* params, uint8_t* labels, float* q1_or_null, void* scratch,
                   void* stream);

/* The grid search crf() is written as (vae_utility.py:22-54: lists for every parameter, the IoU per tuple): the dense
 * CRF above for n_variants VARIANTS of one frame set in one call.  All variants share (alpha, beta, gamma), hence the
 * kernels and both normalisers, which are computed once; the bilateral kernel value of a pixel pair is computed once per
 * pass and applied to every variant of a group of cvae_crf_grid_group(h) variants (more run as consecutive groups over
 * the same scratch).  A variant is its unary and its weights: thr == -1 takes prob1 (B,W,W) fp32 as cvae_dense_crf
 * does, thr in 0..255 takes the mask diff_u8 > thr of diff_u8 (B,W,W) uint8 as prob1 = 1.0 / 0.0; p_floor, w1, w2 as in
 * cvae_crf_params.  The equations, and per variant the summation order of the bilateral sum, are cvae_dense_crf's; the
 * results agree with it to rounding, not bitwise (this entry fixes its fused operations).
 * `snaps`: n_snaps (1..8) strictly ascending iteration counts, each in [0, 10000]; the last is the number of updates
 * run, 0 stands for the labels of softmax(-u).  After each listed iteration counts_or_null (n_snaps, n_variants, B, 3)
 * int64 receives per (snapshot, variant, frame) the (tp, fn, fp) of get_iou(gt, label) with label = Q(1) > Q(0) (the buffer
 * is cleared by the call; integer atomics, order-free; gt (B,W,W) uint8, nonzero = set).  At the LAST snapshot only:
 * labels_or_null (n_variants, B, W, W) uint8 and q1_or_null (n_variants, B, W, W) fp32; with both null no mask is ever
 * written (the search needs the counts alone).
 * Deterministic: the bits of one (frame, variant) result depend on that frame and that variant alone, not on the batch,
 * the frame's position, the number of variants, the variant's slot in its group or the group.
 * `variants` and `snaps` are HOST arrays, read before the call returns.  Ranges as for cvae_dense_crf, all finite.
 * CVAE_EINVAL before any device access, every output untouched: a variant whose plane (prob1 / diff_u8) is null; thr
 * outside -1..255; counts without gt; no output at all; snapshots unsorted, repeated or out of range; n_variants outside
 * 1..64; n_snaps outside 1..8; a non-finite value; scratch null or not 256-byte aligned.
 * `scratch`: cvae_crf_grid_scratch_bytes(h, batch, n_variants) bytes of device memory (host-only query; -1 for a bad
 * handle, batch or n_variants).  cvae_crf_grid_group is host-only too (-1 for a null handle). */
typedef struct cvae_crf_variant {
    int32_t thr;             /* -1: prob1; 0..255: diff_u8 > thr */
    float p_floor, w1, w2;
} cvae_crf_variant;
#define CVAE_CRF_GRID_MAX_VARIANTS 64
#define CVAE_CRF_GRID_MAX_SNAPS 8
int32_t cvae_crf_grid_group(cvae_handle h);
int64_t cvae_crf_grid_scratch_bytes(cvae_handle h, int32_t batch, int32_t n_variants);
int cvae_crf_grid(cvae_handle h, int32_t batch, const uint8_t* frames_hwc, const float* prob1_or_null,
                  const uint8_t* diff_u8_or_null, const uint8_t* gt_or_null, float alpha, float beta, float gamma,
                  const cvae_crf_variant* variants, int32_t n_variants, const int32_t* snaps, int32_t n_snaps,
                  int64_t* counts_or_null, uint8_t* labels_or_null, float* q1_or_null, void* scratch, void* stream);

/* Objects from masks (no reference counterpart: vae_utility.py scores pixels only).  cvae_mask_objects is ONE launch for any
 * batch, one workgroup per frame at both widths; the frame's mask (B,W,W) uint8, nonzero = set, is read once and everything up
 * to the output writes stays in LDS.  Per frame, in this order:
 *   1. fill_holes: every clear region not connected to the frame border becomes set.  Clear pixels connect under the
 *      COMPLEMENTARY connectivity: 4 when the set pixels use 8, 8 when they use 4 (scipy.ndimage.binary_fill_holes with that
 *      structure).
 *   2. the set pixels are labelled under `connectivity` (4 or 8).
 *   3. components of fewer than min_area pixels are cleared.
 *   4. keep_largest = k >= 1 keeps the k largest of the rest, ties on area to the component whose first pixel comes earlier in
 *      raster order; 0 keeps all.
 *   5. the survivors are labelled 1..kept in raster order of each component's first pixel (scipy.ndimage.label's order).
 * Outputs, every element written:
 *   mask_out_or_null (B,W,W) uint8  0 / 1
 *   labels_or_null   (B,W,W) uint16 0 = background; every kept object is labelled, those past max_objects included
 *   info             (B,4) int32    [0] components after step 1, [1] components kept, [2] pixels set by the hole fill,
 *                                   [3] labelling passes used (a diagnostic: 1 .. W*W + 1, not part of the result)
 *   table_or_null    (B,M,8) int32  M = max_objects; row i is label i + 1: area, x0, y0, x1, y1 (inclusive box), sum x, sum y,
 *                                   sum value over values_u8_or_null (B,W,W) uint8 (0 without that plane).  Rows at or past
 *                                   `kept` are zero; kept > M means the table is truncated while labels and counts stay complete.
 * Labelling is label equivalence on 16-bit labels in LDS: a pass writes the smallest neighbouring label to the label's root
 * with an atomic minimum and then flattens every chain.  Labels only decrease, a pass that changes nothing ends the loop, and
 * W*W + 1 passes end it whatever the input.  The final label of a component is a function of the component alone (its minimum
 * linear index, ranked in raster order among the survivors), and all accumulations are integer atomics: a frame's result is
 * bitwise independent of the batch and of its slot in it.
 * CVAE_EINVAL before any device access: null handle, mask, params or info; flags != 0; connectivity not 4 or 8; fill_holes not
 * 0 or 1; min_area < 1; keep_largest < 0; max_objects outside 1..CVAE_OBJECTS_MAX; batch < 1 or batch * W * W >= 2^31 (batch
 * is NOT capped by max_batch); mask, values, mask_out or labels not 16-byte aligned.  Nothing allocates or synchronises.
 * The stream is followed by `flags` for the reason given at cvae_latent_stats.
 *
 * cvae_object_overlap: inter (B,M,M) int32 = the number of pixels with labels_a == i + 1 and labels_b == j + 1 (both (B,W,W)
 * uint16, 16-byte aligned; labels above M are ignored).  One workgroup per frame, the matrix in LDS, integer atomics, one write.
 * Same argument checks. */
#define CVAE_OBJECTS_MAX 64
typedef struct cvae_object_params {
    int32_t connectivity;    /* 4 or 8: of the set pixels */
    int32_t fill_holes;      /* 0 or 1 */
    int32_t min_area;        /* >= 1 */
    int32_t keep_largest;    /* 0: all; k >= 1: the k largest */
    int32_t max_objects;     /* M: table rows, 1..CVAE_OBJECTS_MAX */
} cvae_object_params;
int cvae_mask_objects(cvae_handle h, int32_t batch, const uint8_t* mask, const uint8_t* values_u8_or_null,
                      const cvae_object_params* params, uint8_t* mask_out_or_null, uint16_t* labels_or_null, int32_t* info,
                      int32_t* table_or_null, void* stream, uint32_t flags /* 0 */);
int cvae_object_overlap(cvae_handle h, int32_t batch, const uint16_t* labels_a, const uint16_t* labels_b, int32_t max_objects,
                        int32_t* inter, void* stream, uint32_t flags /* 0 */);

/* ---------------------------------------------------------------------------------------- *
 * The reference's pictures: the PNG strips of image_evaluate (vae.py:68-108) and get_injected_img
 * (vae_utility.py:240-254) and the 7-panel video frames of get_final_frame (vae_utility.py:286-322).
 * ---------------------------------------------------------------------------------------- */

/* One panel of w x w pixels (w = the handle's width).  Picture b reads `data` + b * batch_stride ELEMENTS (floats for
 * F32_CHW, bytes otherwise; 0 shows the same panel in every picture).  Pixel rules, each what the reference's host code does:
 *   F32_CHW  fp32 (3,w,w) in the range of Tanh: prepare_rgb_image's (img * 255).astype(np.uint8) = ONE fp32 multiply rounded
 *            to nearest, truncation toward zero to int32, the low 8 bits (two's-complement wrap: -0.3 -> 180, -0.99 -> 4, 1.0
 *            -> 255; the reference's pictures show negative reconstruction pixels wrapped); NaN, +-inf and |v * 255| >= 2^31
 *            give 0.  With CVAE_COMPOSE_CLAMP the truncated value saturates to [0, 255] instead.
 *   U8_HWC   uint8 (w,w,3), copied (the episode frames).
 *   U8_GREY  uint8 (w,w), replicated to r, g, b (PIL mode L pasted into RGB: diff_u8).
 *   MASK     uint8 (w,w), nonzero -> 255, else 0, replicated (PIL mode 1 pasted into RGB: thr, crf, gt masks).
 * `data`: 16-byte aligned, batch_stride a multiple of 4 (F32_CHW, U8_GREY, MASK) or 16 (U8_HWC) elements. */
enum { CVAE_PANEL_F32_CHW = 0, CVAE_PANEL_U8_HWC = 1, CVAE_PANEL_U8_GREY = 2, CVAE_PANEL_MASK = 3 };
#define CVAE_MAX_PANELS 8
#define CVAE_COMPOSE_CLAMP 1
typedef struct cvae_panel {
    int32_t kind;
    int32_t reserved;        /* 0 */
    const void* data;        /* device */
    int64_t batch_stride;    /* elements, >= 0 */
} cvae_panel;

/* out (batch, row_offset + w, n_panels * w, 3) uint8 HWC: the panels side by side from row `row_offset` down (0 for the
 * strips, w for the video frames whose upper half holds the titles); rows above it are black.  `panels`: HOST array of
 * n_panels (1..CVAE_MAX_PANELS) descriptors.  Text, white over whatever the panel holds:
 *   overlay_or_null (row_offset + w, n_panels * w) uint8, shared by every picture: nonzero = white pixel;
 *   atlas_or_null (n_labels, label_h, label_w) uint8 with label_idx (batch) int32: picture b shows label label_idx[b] with its
 *   top left corner at column label_x, row label_y (clipped at the picture's edges; an index outside [0, n_labels) shows
 *   none and is never read).
 * One launch on the caller's stream, 16 output bytes per thread, no scratch, no atomics: a picture's bytes depend on its own
 * inputs alone, whatever the batch.  Picture offsets are 64-bit (2 450 video frames at 128 x 128 are 0.8 GB); batch >= 1,
 * 0 <= row_offset <= 2 * w; CVAE_EINVAL for a bad argument or a batch whose workgroup count does not fit one launch
 * (batch * ceil((row_offset + w) * n_panels * w * 3 / 4096) >= 2^31).  out and overlay 16-byte aligned. */
int cvae_compose_frames(cvae_handle h, int32_t batch, int32_t n_panels, const cvae_panel* panels, int32_t row_offset,
                        int32_t flags, const uint8_t* overlay_or_null, const uint8_t* atlas_or_null, int32_t n_labels,
                        int32_t label_h, int32_t label_w, const int32_t* label_idx, int32_t label_x, int32_t label_y,
                        uint8_t* out, void* stream);

/* Decoder input of `vae.py -inject` for a batch (VariationalAutoencoder.inject, vae_nets.py:31-40): row b * n_rewards + r of
 * zcat (n_images * n_rewards, 33) = (mu[b] (32 values), rewards[r]).  mu (n_images, 32) = the eval-mode encoder's mu,
 * rewards (n_rewards) fp32 on the device.  cvae_decode(zcat) then gives (n_images, n_rewards, 3, W, W).
 * n_images, n_rewards >= 1 and n_images * n_rewards <= max_batch. */
int cvae_inject_zcat(cvae_handle h, int32_t n_images, int32_t n_rewards, const float* mu, const float* rewards,
                     float* zcat, void* stream);

/* float offset of a named saved tensor in the workspace ("y0".."y3", "a0".."a3", "o0".."o3",
 * "zcat", "h", "d_*" ...) for tests; -1 if unknown OR not allocated in this configuration: "d_y0" does not exist
 * (block 0's BatchNorm backward runs inside the E1 weight-gradient kernel), and in precision mode 1 "dout4" has no
 * storage and the "y0" slot is STALE unless a block-0 |gamma| is < 1e-2 (the device decides per step) — do not read it
 * otherwise.  Slots hold bf16 elements in precision mode 1.  "ms": the MS-SSIM region of cvae_loss / cvae_loss_obj / cvae_score,
 * cvae_op_msssim_ws_floats(batch) floats: the level pyramids, fields and partials, then — its last 832 floats — the fp64 slab
 * (704), the coefficients (64) and the arrival ticket (64), which is all a cvae_loss_obj at msssim_weight 0 touches. */
int64_t cvae_ws_offset(cvae_handle h, int32_t batch, const char* name);

/* Which kernel family the forward (dgrad = 0) or input-gradient (dgrad = 1) pass of encoder conv layer 1..3 (E2..E4, nn.Conv2d at
 * vae_nets.py:74,79,84) takes at `batch` images: 0 = per-tile kernel (64-bit addressing, any size), 1 = two-workgroup persistent kernel,
 * 2 = big-tile persistent kernel.  The persistent kernels address their tensors with 32-bit byte offsets, so activations of 2 GiB and
 * more (E2's output: batch >= 8192 in fp32, >= 16384 in bf16 mode at 64 x 64) take the per-tile kernel, without the caller doing
 * anything.  Layer 0 (E1), dgrad = 0, precision 1 only: 1 = E1's passes stage the packed bf16 frame (workspace slot "xp", addressed
 * the same way), 0 = the fp32 frame x — from batch * width^2 * 8 + (2 * width + 2) * 8 >= 2^31 (batch >= 65536 at 64 x 64, >= 16384 at
 * 128 x 128).  Host logic only (the route table the launchers read; no device access, works without a GPU);
 * CVAE_EINVAL for arguments outside these ranges.  precision as in cvae_config. */
int32_t cvae_conv_route(int32_t precision, int32_t width, int32_t layer, int32_t dgrad, int64_t batch);

/*
 * In-step kernel probe (measurement only): bit (kind*9 + layer) of `mask` arms a HIP event pair
 * around that conv kernel (kind 0 forward, 1 dgrad, 2 wgrad; layer 1..7) inside cvae_forward /
 * cvae_backward, recorded on the stream the kernel is launched on.  HBM-side kernels: bit 0 = E1 forward
 * (in bf16 mode the BatchNorm/pool pass), bit 18 = E1 weight gradient (with block 0's fused BatchNorm backward),
 * bit 8 = D4 forward, bit 17 = the fused D4 backward, bits 27..30 = the BatchNorm+pool backward apply kernel of
 * encoder block 0..3, bit 31 = the MS-SSIM level-0 tile kernel (inside cvae_loss).  cvae_probe_read returns the
 * elapsed milliseconds of each recorded launch (host array) and clears the slot.
 */
int cvae_probe_config(cvae_handle h, uint32_t mask);
int cvae_probe_read(cvae_handle h, int32_t id, float* ms_host, int32_t cap);

/* ---------------------------------------------------------------------------------------- *
 * Per-op entry points (unit tests and the roofline probe in bench.py).  `layer`: 0..3 =
 * encoder conv blocks E1..E4 (vae_nets.py:69,74,79,84), 4..8 = decoder convs D0..D4
 * (vae_nets.py:117,121,125,129,133).  Activations are NHWC except x/recon (NCHW); decoder
 * layers 5..8 read the stored (pre-Upsample) tensor.  `scratch` needs cvae_op_scratch_floats().
 * The conv ops of layers 1..7 run the kernels the step runs there: the step and these entry points
 * choose their launcher in the same three functions over one table of (precision, layers) rows
 * (api.hip, kConvTable), and a call on the operands the step stored stores the words the step
 * stored.  Layers 0 and 8 (E1, D4) are not in the table: the step runs their fused forms, these
 * entry points the plain ones.
 * On a handle of the fp32-emulation modes (precision 2, 3) that is, for layers 1..4: forward and
 * input gradient on the bf16 MFMA with 3-way split operands (the fp32 weight is packed into
 * `scratch` first), weight gradient on the split-operand kernel.  All tensors stay fp32;
 * cvae_op_scratch_floats() includes the packed copy.  Every other layer of these handles, and every
 * layer of precision 0, runs the fp32 kernels (layers 5..7: the weight is collapsed into `scratch`).
 * On a bf16 handle (precision 1) the tensors are in the handle's storage type: activations and
 * activation gradients (in, out, dout, din, mask_src, o3, d_o3) are bf16 behind the float pointers;
 * weights, biases, their gradients, recon and d_recon are fp32.  cvae_op_conv_fwd /
 * cvae_op_conv_dgrad of layers 1..4 pack the layer's weights into `scratch` and take conv_route's
 * kernel family at that batch (D0: split-K + finish at 64 x 64); layers 5..7 collapse and pack them
 * and run the bf16 up-conv kernels (mask_src in bf16); layer 8 and cvae_op_d4_bwd run D4's bf16
 * forms (the Tanh backward is applied inside: `dout` is not written and may be null);
 * cvae_op_conv_wgrad of layers 1..7 runs the bf16 weight-gradient kernels.  Layer 0's weight
 * gradient stays the fp32 kernel on fp32 tensors: its bf16 form exists only fused with block 0's
 * BatchNorm backward (cvae_op_e1_wgrad_fused, which runs the step's fused form on every handle).
 * The three cvae_op_conv_* entry points check their arguments before any device access and return
 * CVAE_EINVAL, with cvae_last_error() naming the argument, for a null handle, a layer outside the
 * entry's range (forward 0..8, input gradient 1..7, weight gradient 0..7), a batch outside
 * [1, max_batch], and a null `scratch` on a pass that uses it.  On every precision alike that is:
 * every weight gradient; forward and input gradient of every layer whose weights are prepared in
 * `scratch` (packed: layers 1..7 of precision 1, 1..4 of precision 2 and 3; collapsed: layers
 * 5..7 of every precision) and of D0 (layer 4) at 64 x 64, whose split-K slabs live there.  A null
 * `scratch` is valid everywhere else: layers 0 and 8, layers 1..3 of precision 0, D0 of
 * precision 0 at 128 x 128.
 * ---------------------------------------------------------------------------------------- */
int64_t cvae_op_scratch_floats(cvae_handle h, int32_t batch);
int64_t cvae_op_bn_partial_floats(cvae_handle h, int32_t layer, int32_t batch);
int64_t cvae_op_msssim_ws_floats(cvae_handle h, int32_t batch);

/* nn.Conv2d forward (+bias; encoder: raw output + BatchNorm partials; decoder: +ReLU, D4: +Tanh) */
int cvae_op_conv_fwd(cvae_handle h, int32_t layer, int32_t batch, const float* in, const float* w,
                     const float* bias, float* out, float* bn_partials, void* scratch, void* stream);
/* input gradient, layers 1..7; decoder layers 5..7 also fold Upsample backward (2x2 sum) and the
 * ReLU mask of the producing layer's output `mask_src`; layer 4 (D0) at 64x64 runs the training
 * step's split-K kernel, its partial slabs in `scratch` */
int cvae_op_conv_dgrad(cvae_handle h, int32_t layer, int32_t batch, const float* dout,
                       const float* w, const float* mask_src, float* din, void* scratch, void* stream);
/* weight (+ optional bias) gradient, layers 0..7 */
int cvae_op_conv_wgrad(cvae_handle h, int32_t layer, int32_t batch, const float* in,
                       const float* dout, float* dw, float* dbias, void* scratch, void* stream);
/* D4 backward, fused: Tanh' -> dout (B,3,W,W), d_o3 (ReLU-masked, NHWC), dW4, db4 */
int cvae_op_d4_bwd(cvae_handle h, int32_t batch, const float* o3, const float* d_recon,
                   const float* recon, const float* w, float* dout, float* d_o3, float* dw,
                   float* db, void* scratch, void* stream);
/* E1's weight (+ optional bias) gradient in the form the training step runs: the kernel applies block 0's BatchNorm / MaxPool / ReLU
 * backward while it stages a tile, dy[p] = scale * ((p == argmax ? g : 0) - k1 - xhat[p] * k2) with g = d_a0 * [a0 > 0] and the argmax
 * the first maximum of fma(y, scale, shift) in scan order (0,0) (0,1) (1,0) (1,1), and no dy tensor exists.  The same launcher call as
 * the step's: precision 0, 2 and 3 run the fp32 kernel, precision 1 the bf16 kernel, which also recomputes y from x, w1 and b1.
 * x: the fp32 NCHW frame; y0, a0, d_a0: NHWC in the handle's storage type; coef0: 128 floats, (scale, shift, mean, invstd) per channel;
 * bcoef0: 64 floats, (k1, k2) per channel; w1 [75][32] and b1: E1's parameters.  On a bf16 handle y0 is never read and may be null;
 * on the other handles w1 and b1 are never read and may be null.  dbias may be null; dbias == dw + 2432 (the flat gradient buffer's
 * layout) takes the step's single column reduction, which leaves the 32 floats between the two alone.
 * flags: bit 0, bf16 handles only: the kernel stages its strips from the packed bf16 frame, as after a train-mode forward; the entry
 * first runs the forward's statistics pass, which writes that frame, into `scratch`.  CVAE_EINVAL at a batch where
 * cvae_conv_route(1, width, 0, 0, batch) is not 1.  `scratch`: cvae_op_scratch_floats().
 * Checked before any launch, CVAE_EINVAL with cvae_last_error() naming the argument: a null handle, a batch outside [1, max_batch], a
 * null required pointer, unknown flag bits, flag bit 0 on a handle that is not bf16. */
int cvae_op_e1_wgrad_fused(cvae_handle h, int32_t batch, const float* x, const float* y0, const float* a0, const float* d_a0,
                           const float* coef0, const float* bcoef0, const float* w1, const float* b1,
                           float* dw, float* dbias, void* scratch, int32_t flags, void* stream);
/* BatchNorm2d(train) -> MaxPool2d(2) -> ReLU/Tanh of encoder block `layer` (0..3) */
int cvae_op_bn_pool_act_fwd(cvae_handle h, int32_t layer, int32_t batch, const float* y,
                            const float* bn_partials, const float* gamma, const float* beta,
                            float* run_mean, float* run_var, float* coef, float* a, void* scratch,
                            int32_t train, void* stream);
/* How many 128-pixel tiles one BatchNorm partial row written by cvae_op_conv_fwd(layer 0..3) covers on this
 * handle at this batch (conv_route: 4 or 8 for the big-tile bf16 kernels, 1 otherwise).  cvae_op_bn_pool_act_fwd
 * expects one tile per row; rows of more tiles go through cvae_op_bn_fwd_finalize. */
int32_t cvae_op_conv_tiles_per_partial(cvae_handle h, int32_t layer, int32_t batch);
/* Host logic only (layers 0 and 5..7 ask the device's compute-unit count): out[0..2] = (tiles, splits, tiles per split) of the kernel
 * that cvae_op_conv_wgrad(layer 1..7) or cvae_op_e1_wgrad_fused (layer 0: strips of 4 x 32 pixels) launches on a bf16 handle at this
 * batch, from the launchers' own split arithmetic.  CVAE_EUNSUPPORTED on other handles and layers. */
int cvae_op_conv_wgrad_plan(cvae_handle h, int32_t layer, int32_t batch, int32_t* out);
/* Host logic only (no handle, no device access): out[0..2] = (tiles, splits, tiles per split) of the fp32 kernel that
 * cvae_op_conv_wgrad(layer 0..7) and cvae_op_d4_bwd (layer 8) launch on a precision 0 handle of this width at this batch, on a
 * device of `num_cus` compute units (only layers 5..7 depend on it; the launchers pass the current device's count), from the
 * launchers' own split functions.  Tiles are 128 pixels for layers 1..4, 64 low-resolution pixels for layers 5..7, and
 * batch * (width / 4) * (width / 32) / batch * (width / 16) * (width / 32) strips for layers 0 / 8.
 * Width other than 64 / 128, layer outside 0..8, batch or num_cus below 1, or a null pointer: CVAE_EINVAL. */
int32_t cvae_op_conv_wgrad_plan_f32(int32_t width, int32_t layer, int32_t batch, int32_t num_cus, int32_t* out);
/* The statistics half of cvae_op_bn_pool_act_fwd on partial rows of `tiles_per_partial` (1, 2, 4, 8) tiles each:
 * coef (scale, shift, mean, invstd per channel) and, in train mode, the running statistics.  `scratch` as above. */
int cvae_op_bn_fwd_finalize(cvae_handle h, int32_t layer, int32_t batch, const float* bn_partials,
                            int32_t tiles_per_partial, const float* gamma, const float* beta,
                            float* run_mean, float* run_var, float* coef, void* scratch,
                            int32_t train, void* stream);
int cvae_op_bn_pool_act_bwd(cvae_handle h, int32_t layer, int32_t batch, const float* y,
                            const float* a, const float* da, const float* coef, const float* gamma,
                            float* dy, float* dgamma, float* dbeta, float* dbias, void* scratch,
                            void* stream);
/* MSSIM.forward (vae_nets.py:217-247) on NCHW planes, optional gradient w.r.t. img1 */
int cvae_op_msssim(cvae_handle h, int32_t batch, const float* img1, const float* img2, void* ws,
                   float* scalars, float* d_img1, void* stream);

/*
 * The latent layers (fc.hip), one entry point per launcher of the step.  Weights in the native layouts: Wfc [K][64]
 * (columns 0..31 = fc_mu, 32..63 = fc_var), Wd [33][K], K = 256 (width/16)^2 in (h,w,c) order, i.e. `flat`, `h_out`, `dh`
 * and `dflat` are (batch, K) NHWC activations in the handle's storage type (bf16 elements on a precision 1 handle, fp32
 * otherwise); every other tensor is fp32.  `scratch` needs cvae_op_latent_scratch_floats(batch) floats; its contents on
 * entry do not matter.  batch < 1, batch > max_batch or a null pointer is CVAE_EINVAL (the size query returns it too).
 */
int64_t cvae_op_latent_scratch_floats(cvae_handle h, int32_t batch);
/* Host logic only (no handle, no device access): the grids the four launchers below use at `batch` on a device of `num_cus`
 * compute units, from the function the launchers themselves call (they pass the current device's count).  A merged launch runs
 * its jobs over consecutive blockIdx.x ranges [begin, end).  out[0..CVAE_LATENT_PLAN_INTS):
 *   [0]      fc_fwd: blocks of the fc_mu | fc_var GEMM, ceil(batch / 128) row blocks x 32 K-slices
 *   [1] [2]  decin_fwd: images per workgroup (16, 8 or 4), blocks = (K / 1024) * ceil(batch / images)
 *   [3] [4]  decin_bwd, job 0: dWd | dbd, K / 32 blocks        [5] [6]  job 1: the d_zcat slabs, ceil(batch / 128) * 32 blocks
 *   [7]      fc_bwd: images per dflat workgroup (32, 16 or 8)
 *   [8] [9]  fc_bwd, job 0: dWfc, K / 32 blocks                [10] [11] job 1: dflat, (K / 256) * ceil(batch / images) blocks
 *   [12] [13] job 2: first stage of dbfc, min(batch, 128) blocks
 *   [14]     0: the three jobs of fc_bwd share one launch of [13] blocks.  1 (K / 32 > num_cus: the dWfc workgroups fill the
 *            device by themselves): dflat runs in a launch of its own of [11] blocks, [10] = 0, behind dWfc and dbfc ([13] blocks)
 * [6] is the grid of decin_bwd's launch.  Width other than 64 / 128, batch or num_cus below 1, or a null pointer: CVAE_EINVAL. */
#define CVAE_LATENT_PLAN_INTS 15
int32_t cvae_op_latent_plan(int32_t width, int32_t batch, int32_t num_cus, int32_t* out);
/* flatten + fc_mu | fc_var + reparametrize + cat (vae_nets.py:105-109, :48-51, :143): mu, logvar (batch,32) = flat . Wfc + bfc,
 * zcat (batch,33) = [mu + eps * exp(logvar / 2) | pred] */
int cvae_op_fc_fwd(cvae_handle h, int32_t batch, const float* flat, const float* wfc, const float* bfc,
                   const float* eps, const float* pred, float* mu, float* logvar, float* zcat,
                   void* scratch, void* stream);
/* decoder_input Linear(33, K) (vae_nets.py:143-144): h_out (batch,K) = zcat . Wd + bd */
int cvae_op_decin_fwd(cvae_handle h, int32_t batch, const float* zcat, const float* wd, const float* bd,
                      float* h_out, void* stream);
/* its backward: dwd [33][K] = zcat^T . dh, dbd [K] = column sums of dh, dzcat (batch,33) = dh . Wd^T */
int cvae_op_decin_bwd(cvae_handle h, int32_t batch, const float* zcat, const float* dh, const float* wd,
                      float* dwd, float* dbd, float* dzcat, void* scratch, void* stream);
/* backward of cvae_op_fc_fwd: dml (batch,64) = [dz + dmu_loss | dz * eps * exp(logvar / 2) / 2 + dlv_loss] with dz =
 * dzcat[:, :32]; dwfc [K][64] = flat^T . dml, dbfc [64] = column sums of dml, dflat (batch,K) = dml . Wfc^T */
int cvae_op_fc_bwd(cvae_handle h, int32_t batch, const float* flat, const float* wfc, const float* dzcat,
                   const float* eps, const float* logvar, const float* dmu_loss, const float* dlv_loss,
                   float* dwfc, float* dbfc, float* dflat, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CVAE_H */
