"""ctypes binding of libcvae_hip.so (C-ABI in include/cvae.h).

There is no CPU fallback: if the library is missing or a call fails, this raises.  PyTorch is
used only as the owner of device memory and streams; raw pointers cross the boundary.
"""
import ctypes as C
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CVAE_LIB") or os.path.join(_HERE, "libcvae_hip.so")     # CVAE_LIB: A/B another build of the same sources
N_SCALARS = 16
SYNC_DOUBLES = 2412      # CVAE_SYNC_DOUBLES: the fp64 record of the staged (global-statistics) step
SYNC_POINTS = 9
SCORE_COLS = 8            # CVAE_SCORE_COLS: floats per image row of cvae_score
SCORE_STATE_DOUBLES = 24  # CVAE_SCORE_STATE_DOUBLES: the pooled fp64 record of cvae_score
LATENT_STATE_DOUBLES = 696  # CVAE_LATENT_STATE_DOUBLES: the pooled fp64 record of cvae_latent_stats


class CvaeError(RuntimeError):
    pass


class _Config(C.Structure):
    _fields_ = [("width", C.c_int32), ("max_batch", C.c_int32),
                ("overlap_wgrad", C.c_int32), ("precision", C.c_int32)]


class CrfParams(C.Structure):
    """cvae_crf_params (include/cvae.h): the (w1, alpha, beta, w2, gamma, it) of crf(), vae_utility.py:22-54, plus the unary floor."""
    _fields_ = [("w1", C.c_float), ("alpha", C.c_float), ("beta", C.c_float), ("w2", C.c_float),
                ("gamma", C.c_float), ("p_floor", C.c_float), ("iterations", C.c_int32)]


class CrfVariant(C.Structure):
    """cvae_crf_variant (include/cvae.h): one variant of cvae_crf_grid: thr -1 = the prob1 plane, 0..255 = diff_u8 > thr."""
    _fields_ = [("thr", C.c_int32), ("p_floor", C.c_float), ("w1", C.c_float), ("w2", C.c_float)]


class ObjectParams(C.Structure):
    """cvae_object_params (include/cvae.h): connectivity, hole fill, area filter, keep-largest and table rows of cvae_mask_objects."""
    _fields_ = [("connectivity", C.c_int32), ("fill_holes", C.c_int32), ("min_area", C.c_int32), ("keep_largest", C.c_int32),
                ("max_objects", C.c_int32)]


OBJECTS_MAX = 64          # CVAE_OBJECTS_MAX
CRF_GRID_MAX_VARIANTS, CRF_GRID_MAX_SNAPS = 64, 8      # CVAE_CRF_GRID_MAX_VARIANTS, CVAE_CRF_GRID_MAX_SNAPS


class GuardRecord(C.Structure):
    """cvae_guard_record (include/cvae.h): the decision record at offset 0 of a guard state."""
    _fields_ = [("apply", C.c_int32), ("nonfinite", C.c_uint32), ("coef", C.c_float), ("norm", C.c_float),
                ("norm64", C.c_double), ("t", C.c_int64), ("skipped", C.c_int64), ("step_size", C.c_float),
                ("sqrt_bc2", C.c_float), ("gscale", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("ticket", C.c_uint32)]


class Objective(C.Structure):
    """cvae_objective (include/cvae.h): the weights of cvae_loss_obj and its MS-SSIM gradient mode."""
    _fields_ = [("msssim_weight", C.c_float), ("mse_weight", C.c_float), ("kld_weight", C.c_float),
                ("msssim_grad", C.c_int32)]


MSGRAD_REFERENCE, MSGRAD_USED = 0, 1
OPT_MAX_RANGES = 16       # CVAE_OPT_MAX_RANGES
OPT_MAX_AUX = 4096


class OptArgs(C.Structure):
    """cvae_opt_args (include/cvae.h): weight-decay factor, EMA rate and the decayed element ranges of one optimizer step."""
    _fields_ = [("decay_mul", C.c_float), ("ema_omd", C.c_float), ("n_ranges", C.c_int32), ("reserved", C.c_int32),
                ("begin", C.c_int64 * OPT_MAX_RANGES), ("end", C.c_int64 * OPT_MAX_RANGES)]


def opt_args(decay_mul=1.0, ema_omd=0.0, ranges=()):
    """An OptArgs from host values; more than OPT_MAX_RANGES ranges raise here (the table has no room for them), every other
    check is the library's."""
    ranges = list(ranges)
    if len(ranges) > OPT_MAX_RANGES:
        raise ValueError(f"{len(ranges)} decayed ranges: at most {OPT_MAX_RANGES}")
    a = OptArgs(float(decay_mul), float(ema_omd), len(ranges), 0)
    for k, (b, e) in enumerate(ranges):
        a.begin[k], a.end[k] = int(b), int(e)
    return a


TRACE_MAX_SCALARS = 16   # CVAE_TRACE_MAX_SCALARS
TRACE_MAX_TENSORS = 32   # CVAE_TRACE_MAX_TENSORS


class TraceRow(C.Structure):
    """cvae_trace_row (include/cvae.h): one step row of the trace ring, 128 bytes."""
    _fields_ = [("step", C.c_int64), ("lr", C.c_float), ("applied", C.c_int32), ("nonfinite", C.c_uint32),
                ("grad_norm", C.c_float), ("coef", C.c_float), ("n_scalars", C.c_int32), ("reserved", C.c_uint8 * 32),
                ("scalars", C.c_float * TRACE_MAX_SCALARS)]


class TensorStat(C.Structure):
    """cvae_tensor_stat (include/cvae.h): the statistics of one tensor, 48 bytes."""
    _fields_ = [("g2", C.c_double), ("p2", C.c_double), ("u2", C.c_double), ("gmax", C.c_float), ("pmax", C.c_float),
                ("g_nonfinite", C.c_uint32), ("p_nonfinite", C.c_uint32), ("step", C.c_int64)]


def _range_arrays(ranges):
    """(n, begin, end) as ctypes int64 arrays from [(begin, end), ...]; the library checks the table."""
    ranges = [(int(b), int(e)) for b, e in ranges]
    n = len(ranges)
    return n, (C.c_int64 * max(n, 1))(*[b for b, _ in ranges]), (C.c_int64 * max(n, 1))(*[e for _, e in ranges])


def tensor_stats_plan(ranges):
    """cvae_tensor_stats_plan (host logic only): dict(chunk, items, grid) of cvae_tensor_stats on the ranges."""
    lib = load()
    n, b, e = _range_arrays(ranges)
    chunk, items, grid = C.c_int32(), C.c_int32(), C.c_int32()
    if lib.cvae_tensor_stats_plan(n, b, e, C.byref(chunk), C.byref(items), C.byref(grid)) != 0:
        raise CvaeError(f"cvae_tensor_stats_plan: {lib.cvae_last_error().decode()}")
    return {"chunk": chunk.value, "items": items.value, "grid": grid.value}


def tensor_stats_scratch_bytes(ranges):
    """cvae_tensor_stats_scratch_bytes (host logic only)."""
    lib = load()
    n, b, e = _range_arrays(ranges)
    size = lib.cvae_tensor_stats_scratch_bytes(n, b, e)
    if size < 0:
        raise CvaeError(f"cvae_tensor_stats_scratch_bytes: {lib.cvae_last_error().decode()}")
    return size


class AugmentParams(C.Structure):
    """cvae_augment (include/cvae.h): the key and ranges of one augmented batch gather."""
    _fields_ = [("key", C.c_uint64), ("flip_below", C.c_uint32), ("max_shift", C.c_int32), ("gain_q16", C.c_int32),
                ("reserved", C.c_int32)]


class Panel(C.Structure):
    """cvae_panel (include/cvae.h): one w x w panel of cvae_compose_frames."""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("data", C.c_void_p), ("batch_stride", C.c_int64)]


PANEL_F32_CHW, PANEL_U8_HWC, PANEL_U8_GREY, PANEL_MASK = 0, 1, 2, 3
MAX_PANELS = 8
COMPOSE_CLAMP = 1
CRITIC_KEEP, CRITIC_DECISIONS, CRITIC_TRAIN_FLOATS = 800, 11072, 11876      # include/cvae.h: cvae_critic_grad
CRITIC_LOSS = {"bce": 0, "mse": 1}
CRITIC_EMBED_SHAPES = ((8, 32, 32), (8, 16, 16), (8, 8, 8), (16, 4, 4), (32, 1, 1))     # cvae_critic_collect: e1..e5
CRITIC_IG_MAX_STEPS = 256         # CVAE_CRITIC_IG_MAX_STEPS
CRITIC_OCCLUSION_PATCHES = (4, 8, 16)
CRITIC_SCORE_COLS = 8             # CVAE_CRITIC_SCORE_COLS: floats per frame row of cvae_critic_score
CRITIC_SCORE_STATE_DOUBLES = 40   # CVAE_CRITIC_SCORE_STATE_DOUBLES: the pooled fp64 record of cvae_critic_score


def build(verbose=False):
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-j8", "-C", os.path.join(_HERE, "csrc")],
                       capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise CvaeError("building libcvae_hip.so failed:\n" + (r.stdout or "") + (r.stderr or ""))
    return LIB_PATH


_lib = None
_p, _i32, _i64, _f = C.c_void_p, C.c_int32, C.c_int64, C.c_float

_SIGS = {
    "cvae_version": (C.c_char_p, []),
    "cvae_last_error": (C.c_char_p, []),
    "cvae_create": (C.c_int, [C.POINTER(_Config), C.POINTER(_p)]),
    "cvae_destroy": (None, [_p]),
    "cvae_param_total": (_i64, [_p]),
    "cvae_param_count": (_i32, [_p]),
    "cvae_param_name": (C.c_char_p, [_p, _i32]),
    "cvae_param_offset": (_i64, [_p, _i32]),
    "cvae_param_numel": (_i64, [_p, _i32]),
    "cvae_workspace_bytes": (_i64, [_p, _i32]),
    "cvae_bn_state_floats": (_i64, [_p]),
    "cvae_ws_offset": (_i64, [_p, _i32, C.c_char_p]),
    "cvae_conv_route": (_i32, [_i32, _i32, _i32, _i32, _i64]),
    "cvae_forward": (C.c_int, [_p, _i32] + [_p] * 9 + [_i32, _p]),
    "cvae_decode": (C.c_int, [_p, _i32] + [_p] * 5),
    "cvae_loss": (C.c_int, [_p, _i32] + [_p] * 10),
    "cvae_loss_obj": (C.c_int, [_p, _i32] + [_p] * 5 + [C.POINTER(Objective)] + [_p] * 5),
    "cvae_backward": (C.c_int, [_p, _i32] + [_p] * 12),
    "cvae_backward_phases": (C.c_int, [_p, _i32] + [_p] * 11 + [_i32, _p]),
    "cvae_grad_bucket": (C.c_int, [_p, _i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "cvae_sync_slot": (C.c_int, [_i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "cvae_forward_stage": (C.c_int, [_p, _i32] + [_p] * 9 + [_i32, _p, _i32, _p]),
    "cvae_loss_stage": (C.c_int, [_p, _i32] + [_p] * 10 + [_i32, _p]),
    "cvae_backward_stage": (C.c_int, [_p, _i32] + [_p] * 12 + [_i32, _p]),
    "cvae_scale_loss_grads": (C.c_int, [_p, _i32] + [_p] * 8),
    "cvae_adam_step": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i32, _f, _f, _f, _f, _f, _p]),
    "cvae_score_cols": (_i32, []),
    "cvae_score_state_bytes": (_i64, []),
    "cvae_score_init": (C.c_int, [_p, _p, _p]),
    "cvae_score": (C.c_int, [_p, _i32] + [_p] * 8),
    "cvae_score_finish": (C.c_int, [_p, _i32, _p, _p, _p]),
    "cvae_latent_stats_state_bytes": (_i64, []),
    "cvae_latent_stats_scratch_bytes": (_i64, [_p, _i32]),
    "cvae_latent_stats_plan": (_i32, [_i32, _i32, C.POINTER(C.c_int32)]),
    "cvae_latent_stats": (C.c_int, [_p, _i32] + [_p] * 7 + [C.c_uint32]),
    "cvae_recon_response": (C.c_int, [_p, _i32, _i32, _p, _p, _p, _p, C.c_uint32]),
    "cvae_guard_state_bytes": (_i64, []),
    "cvae_guard_init": (C.c_int, [_p, _p, _i64, _i64, _p]),
    "cvae_grad_stats": (C.c_int, [_p, _p, _i64, _f, _f, _i32, _f, _f, _f, _p, _p]),
    "cvae_adam_step_guarded": (C.c_int, [_p, _p, _p, _p, _p, _i64, _f, _p, _p]),
    "cvae_adam_step_opt": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i32, _f, _f, _f, _f, _f, C.POINTER(OptArgs), _p, _p, _p, _i32, _p]),
    "cvae_adam_step_guarded_opt": (C.c_int, [_p, _p, _p, _p, _p, _i64, _f, _p, C.POINTER(OptArgs), _p, _p, _p, _i32, _p]),
    "cvae_trace_push": (C.c_int, [_p, _p, _i64, _i64, _f, _p, _i32, _p, _p]),
    "cvae_tensor_stats": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _i64, _f, _f, _f, _f, _f,
                                    _p, _p, _p, _p]),
    "cvae_tensor_stats_scratch_bytes": (_i64, [_i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "cvae_tensor_stats_plan": (C.c_int, [_i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)] + [C.POINTER(C.c_int32)] * 3),
    "cvae_grads_to_bf16": (C.c_int, [_p, _p, _p, _i64, _p]),
    "cvae_grads_from_bf16": (C.c_int, [_p, _p, _p, _i64, _p]),
    "cvae_critic_param_count": (_i32, []),
    "cvae_critic_forward": (C.c_int, [_p, _i32, _p, _p, _p, _p]),
    "cvae_critic_train_floats": (_i64, []),
    "cvae_critic_grad_scratch_bytes": (_i64, [_p, _i32]),
    "cvae_critic_grad": (C.c_int, [_p, _i32, _p, _p, _p, _f, _i32] + [_p] * 7),
    "cvae_critic_collect": (C.c_int, [_p, _i32] + [_p] * 9),
    "cvae_critic_saliency": (C.c_int, [_p, _i32, _p, _p, _i32] + [_p] * 6),
    "cvae_critic_occlusion": (C.c_int, [_p, _i32, _p, _p, _i32, _f, _f, _f] + [_p] * 5),
    "cvae_critic_score_state_bytes": (_i64, []),
    "cvae_critic_score_scratch_bytes": (_i64, [_p, _i32]),
    "cvae_critic_score_init": (C.c_int, [_p, _p, _p]),
    "cvae_critic_score": (C.c_int, [_p, _i32, _p, _p, _i64] + [_p] * 6),
    "cvae_preprocess_u8": (C.c_int, [_p, _i32, _p, _p, _p]),
    "cvae_diff_grey": (C.c_int, [_p, _i32, _p, _p, _p, _p]),
    "cvae_curate_select": (C.c_int, [_p, _i32, _p, _i64, _p, _i32, _i64] + [_p] * 6),
    "cvae_gather_frames_u8": (C.c_int, [_p, _i32, _p, _p, _i64, _p, _i64, _p, _p, _p, _i64, _p]),
    "cvae_preprocess_u8_gather": (C.c_int, [_p, _i32, _i32, _p, _p, _i64, _p, _p, _p, _p]),
    "cvae_curate_select_recon": (C.c_int, [_p, _i32, _p, _i64, _p, _i32, _i64] + [_p] * 10),
    "cvae_recon_zcat": (C.c_int, [_p, _i32, _p, _p, _p, _p, _i64, _p, _p]),
    "cvae_gather_f32": (C.c_int, [_p, _i32, _i32, _p, _p, _i64, _p, _p, _p, _p]),
    "cvae_preprocess_u8_gather_aug": (C.c_int, [_p, _i32, _i32, _p, _p, _i64, _p, C.POINTER(AugmentParams), _p, _p, _p, _p]),
    "cvae_gather_f32_aug": (C.c_int, [_p, _i32, _i32, _p, _p, _i64, _p, C.POINTER(AugmentParams), _p, _p, _p, _p]),
    "cvae_diff_normalize": (C.c_int, [_p, _i32, _p, C.c_double, C.c_double, _i32] + [_p] * 6),
    "cvae_mask_counts": (C.c_int, [_p, _i32, _p, _p, _p, _p]),
    "cvae_mask_objects": (C.c_int, [_p, _i32, _p, _p, C.POINTER(ObjectParams), _p, _p, _p, _p, _p, C.c_uint32]),
    "cvae_object_overlap": (C.c_int, [_p, _i32, _p, _p, _i32, _p, _p, C.c_uint32]),
    "cvae_crf_scratch_bytes": (_i64, [_p, _i32]),
    "cvae_dense_crf": (C.c_int, [_p, _i32, _p, _p, C.POINTER(CrfParams), _p, _p, _p, _p]),
    "cvae_crf_grid_group": (_i32, [_p]),
    "cvae_crf_grid_scratch_bytes": (_i64, [_p, _i32, _i32]),
    "cvae_crf_grid": (C.c_int, [_p, _i32, _p, _p, _p, _p, C.c_float, C.c_float, C.c_float, C.POINTER(CrfVariant), _i32,
                                C.POINTER(C.c_int32), _i32, _p, _p, _p, _p, _p]),
    "cvae_compose_frames": (C.c_int, [_p, _i32, _i32, C.POINTER(Panel), _i32, _i32, _p, _p, _i32, _i32, _i32, _p, _i32, _i32, _p, _p]),
    "cvae_inject_zcat": (C.c_int, [_p, _i32, _i32, _p, _p, _p, _p]),
    "cvae_probe_config": (C.c_int, [_p, C.c_uint32]),
    "cvae_probe_read": (C.c_int, [_p, _i32, C.POINTER(C.c_float), _i32]),
    "cvae_op_scratch_floats": (_i64, [_p, _i32]),
    "cvae_op_bn_partial_floats": (_i64, [_p, _i32, _i32]),
    "cvae_op_msssim_ws_floats": (_i64, [_p, _i32]),
    "cvae_op_conv_fwd": (C.c_int, [_p, _i32, _i32] + [_p] * 7),
    "cvae_op_conv_dgrad": (C.c_int, [_p, _i32, _i32] + [_p] * 6),
    "cvae_op_conv_wgrad": (C.c_int, [_p, _i32, _i32] + [_p] * 6),
    "cvae_op_d4_bwd": (C.c_int, [_p, _i32] + [_p] * 10),
    "cvae_op_e1_wgrad_fused": (C.c_int, [_p, _i32] + [_p] * 11 + [_i32, _p]),
    "cvae_op_bn_pool_act_fwd": (C.c_int, [_p, _i32, _i32] + [_p] * 9 + [_i32, _p]),
    "cvae_op_bn_pool_act_bwd": (C.c_int, [_p, _i32, _i32] + [_p] * 11),
    "cvae_op_conv_tiles_per_partial": (_i32, [_p, _i32, _i32]),
    "cvae_op_conv_wgrad_plan": (C.c_int, [_p, _i32, _i32, C.POINTER(C.c_int32)]),
    "cvae_op_conv_wgrad_plan_f32": (_i32, [_i32, _i32, _i32, _i32, C.POINTER(C.c_int32)]),
    "cvae_op_bn_fwd_finalize": (C.c_int, [_p, _i32, _i32, _p, _i32] + [_p] * 6 + [_i32, _p]),
    "cvae_op_msssim": (C.c_int, [_p, _i32] + [_p] * 6),
    "cvae_op_latent_scratch_floats": (_i64, [_p, _i32]),
    "cvae_op_latent_plan": (_i32, [_i32, _i32, _i32, C.POINTER(C.c_int32)]),
    "cvae_op_fc_fwd": (C.c_int, [_p, _i32] + [_p] * 10),
    "cvae_op_decin_fwd": (C.c_int, [_p, _i32] + [_p] * 5),
    "cvae_op_decin_bwd": (C.c_int, [_p, _i32] + [_p] * 8),
    "cvae_op_fc_bwd": (C.c_int, [_p, _i32] + [_p] * 12),
}
EXPORTS = tuple(_SIGS)


def load():
    """dlopen the library (no GPU needed) and bind every symbol include/cvae.h declares."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CvaeError(f"{LIB_PATH} not found: run __graft_entry__.build() / make -C critic-vae_amd/csrc "
                        "(the HIP library is required; there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)          # AttributeError here = missing export
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


_DTYPE_NAMES = {torch.float32: "fp32", torch.float64: "fp64", torch.uint8: "uint8", torch.int64: "int64", torch.int32: "int32",
                torch.uint16: "uint16"}


def _dev_ptr(t, dtype, what):
    """The address of a contiguous device tensor of `dtype`; None stays None (a NULL argument), an int is an address already."""
    if t is None or isinstance(t, int):
        return t
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), \
        f"{what}: need a contiguous {_DTYPE_NAMES[dtype]} device tensor, got {t.dtype} {t.device} contiguous={t.is_contiguous()}"
    return t.data_ptr()


def _ptr(t):
    return _dev_ptr(t, torch.float32, "argument")


def _ptr64(t):
    return _dev_ptr(t, torch.float64, "argument")


def sync_slot(point):
    """(offset, count) of sync point `point` (0..8) in the fp64 record of the staged step (include/cvae.h)."""
    lib = load()
    off, n = C.c_int64(), C.c_int64()
    if lib.cvae_sync_slot(point, C.byref(off), C.byref(n)) != 0:
        raise CvaeError(f"cvae_sync_slot: {lib.cvae_last_error().decode()}")
    return off.value, n.value


LATENT_PLAN_INTS = 15     # CVAE_LATENT_PLAN_INTS


def latent_plan(width, B, num_cus):
    """cvae_op_latent_plan (host logic only): the grids of the latent launches at batch B on a device of num_cus compute
    units.  Job ranges are (begin, end) over blockIdx.x in launch order; `grid` is the launch's block count.  fc_bwd with
    `split`: dflat has a launch of its own ((0, n) there) behind the launch of `grid` blocks that holds the other two jobs."""
    lib = load()
    out = (C.c_int32 * LATENT_PLAN_INTS)()
    if lib.cvae_op_latent_plan(width, B, num_cus, out) != 0:
        raise CvaeError(f"cvae_op_latent_plan: {lib.cvae_last_error().decode()}")
    v = list(out)
    return {"fc_fwd": {"gemm": v[0]},
            "decin_fwd": {"imgs": v[1], "grid": v[2]},
            "decin_bwd": {"jobs": {"bgemm": (v[3], v[4]), "gemm": (v[5], v[6])}, "grid": v[6]},
            "fc_bwd": {"imgs": v[7], "jobs": {"bgemm": (v[8], v[9]), "dflat": (v[10], v[11]), "colsum": (v[12], v[13])},
                       "grid": v[13], "split": bool(v[14])}}


def latent_stats_plan(B, num_cus):
    """cvae_latent_stats_plan (host logic only): dict(rows, chunks, grid) of cvae_latent_stats at batch B on a device of num_cus
    compute units."""
    lib = load()
    out = (C.c_int32 * 3)()
    if lib.cvae_latent_stats_plan(B, num_cus, out) != 0:
        raise CvaeError(f"cvae_latent_stats_plan: {lib.cvae_last_error().decode()}")
    return {"rows": out[0], "chunks": out[1], "grid": out[2]}


def conv_wgrad_plan_f32(width, layer, B, num_cus):
    """cvae_op_conv_wgrad_plan_f32 (host logic only): (tiles, splits, tiles per split) of the fp32 weight-gradient kernel of conv
    layer 0..8 (8: the fused D4 backward) at batch B on a device of num_cus compute units."""
    lib = load()
    out = (C.c_int32 * 3)()
    if lib.cvae_op_conv_wgrad_plan_f32(width, layer, B, num_cus, out) != 0:
        raise CvaeError(f"cvae_op_conv_wgrad_plan_f32: {lib.cvae_last_error().decode()}")
    return tuple(out)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Handle:
    """Opaque library handle + the flat-parameter layout it reports."""

    PRECISIONS = {"f32": 0, "bf16": 1, "bf16x9": 2, "bf16x6": 3}
    _u8 = staticmethod(lambda t, what: _dev_ptr(t, torch.uint8, what))
    _i32 = staticmethod(lambda t, what: _dev_ptr(t, torch.int32, what))
    _i64 = staticmethod(lambda t, what: _dev_ptr(t, torch.int64, what))

    def __init__(self, width=64, max_batch=256, overlap_wgrad=None, precision="f32"):
        """precision "f32": every contraction on the exact-fp32 MFMA (the 1e-4 parity path).
        "bf16": forward and input-gradient convs of E2..E4 / D0 on the bf16 MFMA (fp32 accumulate,
        fp32 tensors in HBM; BASELINE.json configs 3-5).
        "bf16x9": fp32 emulation — forward / input-gradient convs on the bf16 MFMA with both operands split
        exactly into three bf16 parts (nine exact partial products per fp32 product, fp32 accumulate);
        weight gradients of E2..E4 / D0 on the bf16 MFMA with the same exact splits.  Meets the same 1e-4 parity bar as "f32".
        "bf16x6": as "bf16x9" with the six leading partial products (drops <= 3*2^-24 of each product)."""
        self.lib = load()
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(self.PRECISIONS)}")
        self.precision = precision
        if overlap_wgrad is None:      # unset: the experiment switch CVAE_OVERLAP_WGRAD=1 decides; an explicit
            overlap_wgrad = os.environ.get("CVAE_OVERLAP_WGRAD") == "1"       # argument always wins (tests compare True with False)
        self.overlap_wgrad = bool(overlap_wgrad)                               # the effective value, for bench lines and tests
        cfg = _Config(width, max_batch, int(self.overlap_wgrad), self.PRECISIONS[precision])
        h = _p()
        rc = self.lib.cvae_create(C.byref(cfg), C.byref(h))
        self._check(rc)
        self.h = h
        self.width, self.max_batch = width, max_batch
        self.param_total = self.lib.cvae_param_total(h)
        self.layout = {}
        for i in range(self.lib.cvae_param_count(h)):
            self.layout[self.lib.cvae_param_name(h, i).decode()] = (
                self.lib.cvae_param_offset(h, i), self.lib.cvae_param_numel(h, i))
        self.bn_state_floats = self.lib.cvae_bn_state_floats(h)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.cvae_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise CvaeError(f"libcvae_hip error {rc}: {self.lib.cvae_last_error().decode()}")

    def workspace_bytes(self, batch):
        return self.lib.cvae_workspace_bytes(self.h, batch)

    def ws_view(self, ws, batch, name, numel):
        off = self.lib.cvae_ws_offset(self.h, batch, name.encode())
        if off < 0:
            raise KeyError(name)
        return ws[off:off + numel]

    # ---- the hot path ----
    def forward(self, B, x, pred, eps, params, bn_state, mu, logvar, recon, ws, train=True):
        self._check(self.lib.cvae_forward(self.h, B, _ptr(x), _ptr(pred), _ptr(eps), _ptr(params), _ptr(bn_state),
                                          _ptr(mu), _ptr(logvar), _ptr(recon), _ptr(ws), int(train), _stream()))

    def decode(self, B, zcat, params, recon, ws):
        self._check(self.lib.cvae_decode(self.h, B, _ptr(zcat), _ptr(params), _ptr(recon), _ptr(ws), _stream()))

    def loss(self, B, x, mu, logvar, recon, ws, scalars, d_recon=None, d_mu=None, d_logvar=None):
        self._check(self.lib.cvae_loss(self.h, B, _ptr(x), _ptr(mu), _ptr(logvar), _ptr(recon), _ptr(ws),
                                       _ptr(scalars), _ptr(d_recon), _ptr(d_mu), _ptr(d_logvar), _stream()))

    def loss_obj(self, B, x, mu, logvar, recon, ws, obj, scalars, d_recon=None, d_mu=None, d_logvar=None):
        """cvae_loss under an objective: `obj` is an `Objective` structure, a (msssim, mse, kld, msssim_grad) tuple as
        objective.Objective.at() returns it, or None (a null pointer: CVAE_EINVAL)."""
        if obj is not None and not isinstance(obj, Objective):
            obj = Objective(*obj)
        self._check(self.lib.cvae_loss_obj(self.h, B, _ptr(x), _ptr(mu), _ptr(logvar), _ptr(recon), _ptr(ws),
                                           None if obj is None else C.byref(obj), _ptr(scalars), _ptr(d_recon),
                                           _ptr(d_mu), _ptr(d_logvar), _stream()))

    def backward(self, B, x, pred, eps, params, logvar, recon, d_recon, d_mu, d_logvar, ws, grads, zero_padding=False):
        """zero_padding: `grads` is uninitialised memory — also write 0 into the alignment gaps (phase bit 3)."""
        if zero_padding:
            self._check(self.lib.cvae_backward_phases(self.h, B, _ptr(x), _ptr(pred), _ptr(eps), _ptr(params),
                                                      _ptr(logvar), _ptr(recon), _ptr(d_recon), _ptr(d_mu),
                                                      _ptr(d_logvar), _ptr(ws), _ptr(grads), 15, _stream()))
            return
        self._check(self.lib.cvae_backward(self.h, B, _ptr(x), _ptr(pred), _ptr(eps), _ptr(params), _ptr(logvar),
                                           _ptr(recon), _ptr(d_recon), _ptr(d_mu), _ptr(d_logvar), _ptr(ws),
                                           _ptr(grads), _stream()))

    def scale_loss_grads(self, B, g, d_recon, d_mu, d_logvar, out_recon, out_mu, out_logvar):
        self._check(self.lib.cvae_scale_loss_grads(self.h, B, _ptr(g), _ptr(d_recon), _ptr(d_mu), _ptr(d_logvar),
                                                   _ptr(out_recon), _ptr(out_mu), _ptr(out_logvar), _stream()))

    def grads_to_bf16(self, grads, out_bf16):
        """fp32 gradient range -> caller's bf16 buffer of the same length (transport of the optional bf16 all-reduce)."""
        assert out_bf16.is_cuda and out_bf16.dtype == torch.bfloat16 and out_bf16.is_contiguous() and out_bf16.numel() == grads.numel()
        self._check(self.lib.cvae_grads_to_bf16(self.h, _ptr(grads), out_bf16.data_ptr(), grads.numel(), _stream()))

    def grads_from_bf16(self, in_bf16, grads):
        assert in_bf16.is_cuda and in_bf16.dtype == torch.bfloat16 and in_bf16.is_contiguous() and in_bf16.numel() == grads.numel()
        self._check(self.lib.cvae_grads_from_bf16(self.h, in_bf16.data_ptr(), _ptr(grads), grads.numel(), _stream()))

    def backward_phase(self, phase, B, x, pred, eps, params, logvar, recon, d_recon, d_mu, d_logvar, ws, grads):
        """Phase 0..2 of the backward (decoder | fc + encoder block 3 | encoder blocks 2..0), in order."""
        self._check(self.lib.cvae_backward_phases(self.h, B, _ptr(x), _ptr(pred), _ptr(eps), _ptr(params), _ptr(logvar),
                                                  _ptr(recon), _ptr(d_recon), _ptr(d_mu), _ptr(d_logvar), _ptr(ws),
                                                  _ptr(grads), 1 << phase, _stream()))

    def grad_bucket(self, phase):
        """(offset, numel) of the flat-gradient range that backward phase `phase` completes."""
        off, n = C.c_int64(), C.c_int64()
        self._check(self.lib.cvae_grad_bucket(self.h, phase, C.byref(off), C.byref(n)))
        return off.value, n.value

    # ---- the staged step (global-batch statistics across ranks; include/cvae.h) ----
    # `sync`: a contiguous fp64 device tensor of SYNC_DOUBLES values.  After forward stages 0..3, loss stage 0 and backward
    # stages 0..3, the caller sums slot sync_slot(point) over the ranks (in place) before the next stage.
    sync_slot = staticmethod(sync_slot)

    def forward_stage(self, stage, B, x, pred, eps, params, bn_state, mu, logvar, recon, ws, sync, train=True):
        self._check(self.lib.cvae_forward_stage(self.h, B, _ptr(x), _ptr(pred), _ptr(eps), _ptr(params), _ptr(bn_state),
                                                _ptr(mu), _ptr(logvar), _ptr(recon), _ptr(ws), int(train), _ptr64(sync),
                                                stage, _stream()))

    def loss_stage(self, stage, B, x, mu, logvar, recon, ws, scalars, d_recon, d_mu, d_logvar, sync):
        self._check(self.lib.cvae_loss_stage(self.h, B, _ptr(x), _ptr(mu), _ptr(logvar), _ptr(recon), _ptr(ws),
                                             _ptr(scalars), _ptr(d_recon), _ptr(d_mu), _ptr(d_logvar), _ptr64(sync),
                                             stage, _stream()))

    def backward_stage(self, stage, B, x, pred, eps, params, logvar, recon, d_recon, d_mu, d_logvar, ws, grads, sync):
        self._check(self.lib.cvae_backward_stage(self.h, B, _ptr(x), _ptr(pred), _ptr(eps), _ptr(params), _ptr(logvar),
                                                 _ptr(recon), _ptr(d_recon), _ptr(d_mu), _ptr(d_logvar), _ptr(ws),
                                                 _ptr(grads), _ptr64(sync), stage, _stream()))

    def adam_step(self, params, grads, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
        self._check(self.lib.cvae_adam_step(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), params.numel(),
                                            step, lr, b1, b2, eps, grad_scale, _stream()))

    # ---- per-image scores and the pooled record of a held-out set (include/cvae.h) ----
    def score_cols(self):
        return self.lib.cvae_score_cols()

    def score_state_bytes(self):
        return self.lib.cvae_score_state_bytes()

    def score_state(self, device):
        """A fresh pooled record on `device`: a float64 tensor of SCORE_STATE_DOUBLES values, initialised."""
        state = torch.empty(self.lib.cvae_score_state_bytes() // 8, dtype=torch.float64, device=device)
        self.score_init(state)
        return state

    def _score_ptr(self, state):
        if state is None:
            return None
        ptr = _ptr64(state)
        assert isinstance(state, int) or state.numel() * 8 >= self.lib.cvae_score_state_bytes(), "score state: too small"
        return ptr

    def score_init(self, state):
        self._check(self.lib.cvae_score_init(self.h, self._score_ptr(state), _stream()))

    def score(self, B, x, mu, logvar, recon, ws, per_image=None, state=None):
        """Rows (B, SCORE_COLS) into `per_image` and / or the batch into the pooled record `state`."""
        self._check(self.lib.cvae_score(self.h, B, _ptr(x), _ptr(mu), _ptr(logvar), _ptr(recon), _ptr(ws), _ptr(per_image),
                                        self._score_ptr(state), _stream()))

    def score_finish(self, state, scalars, width=None):
        """The 16 loss scalars of everything pooled in `state` since score_init: cvae_loss of all of it as one batch."""
        self._check(self.lib.cvae_score_finish(self.h, self.width if width is None else width, self._score_ptr(state),
                                               _ptr(scalars), _stream()))

    # ---- pooled latent statistics of a set (include/cvae.h; latent.py) ----
    def latent_stats_state(self, device):
        """A fresh (empty = all-zero) pooled latent record on `device`: a float64 tensor of LATENT_STATE_DOUBLES values."""
        return torch.zeros(self.lib.cvae_latent_stats_state_bytes() // 8, dtype=torch.float64, device=device)

    def latent_stats_scratch_bytes(self, B):
        n = self.lib.cvae_latent_stats_scratch_bytes(self.h, B)
        if n < 0:
            raise CvaeError(f"cvae_latent_stats_scratch_bytes: {self.lib.cvae_last_error().decode()}")
        return n

    def latent_stats_scratch(self, B, device):
        """Scratch for cvae_latent_stats at batches up to B (uninitialised: its contents never matter)."""
        return torch.empty(self.latent_stats_scratch_bytes(B) // 8, dtype=torch.float64, device=device)

    def latent_stats(self, B, mu, logvar, pred, state, scratch, kl_rows=None, flags=0):
        """cvae_latent_stats: ADD the B rows of mu (B,32), logvar (B,32), pred (B) to the pooled record `state`; kl_rows (B,32)
        fp32 or None."""
        need = self.lib.cvae_latent_stats_scratch_bytes(self.h, B)          # negative: a batch the entry itself refuses below
        assert isinstance(state, int) or state is None or state.numel() >= LATENT_STATE_DOUBLES, "latent state: too small"
        assert need < 0 or isinstance(scratch, int) or scratch is None or scratch.numel() * scratch.element_size() >= need, \
            f"latent scratch: need {need} bytes"
        for t, n in ((mu, 32 * B), (logvar, 32 * B), (pred, B), (kl_rows, 32 * B)):
            assert need < 0 or t is None or isinstance(t, int) or t.numel() >= n, "latent_stats: a tensor is shorter than the batch"
        self._check(self.lib.cvae_latent_stats(self.h, B, _ptr(mu), _ptr(logvar), _ptr(pred), _ptr64(state), _ptr(kl_rows),
                                               self._raw(scratch, 8, "latent scratch"), _stream(), int(flags)))

    def recon_response(self, n, K, recon_base, recon_var, out, flags=0):
        """cvae_recon_response: out (n,K,2) = per (image, variant) the mean squared difference and the largest grey difference
        of recon_var (n,K,3,W,W) against recon_base (n,3,W,W)."""
        px = 3 * self.width * self.width
        for t, m in ((recon_base, n * px), (recon_var, n * K * px), (out, n * K * 2)):
            assert t is None or isinstance(t, int) or n < 1 or K < 1 or t.numel() >= m, "recon_response: a tensor is shorter than n x K"
        self._check(self.lib.cvae_recon_response(self.h, n, K, _ptr(recon_base), _ptr(recon_var), _ptr(out), _stream(), int(flags)))

    # ---- the guarded step (include/cvae.h): statistics of the reduced gradient -> decision record -> Adam that obeys it ----
    def guard_state(self, device, applied=0, skipped=0):
        """A fresh guard state on `device` (an int64 tensor: 8-byte aligned), counters as given."""
        state = torch.empty((self.lib.cvae_guard_state_bytes() + 7) // 8, dtype=torch.int64, device=device)
        self.guard_init(state, applied, skipped)
        return state

    def guard_init(self, state, applied=0, skipped=0):
        self._check(self.lib.cvae_guard_init(self.h, self._guard_ptr(state), int(applied), int(skipped), _stream()))

    def _guard_ptr(self, state):
        ptr = self._i64(state, "guard state")
        assert isinstance(state, int) or state.numel() * 8 >= self.lib.cvae_guard_state_bytes(), "guard state: too small"
        return ptr

    def grad_stats(self, grads, state, grad_scale=1.0, max_norm=float("inf"), skip_nonfinite=True, lr=0.0, b1=0.9, b2=0.999,
                   n=None):
        self._check(self.lib.cvae_grad_stats(self.h, _ptr(grads), grads.numel() if n is None else n, grad_scale, max_norm,
                                             int(bool(skip_nonfinite)), lr, b1, b2, self._guard_ptr(state), _stream()))

    def adam_step_guarded(self, params, grads, m, v, state, eps=1e-8, n=None):
        self._check(self.lib.cvae_adam_step_guarded(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v),
                                                    params.numel() if n is None else n, eps, self._guard_ptr(state), _stream()))

    # ---- the optimizer options (include/cvae.h): weight decay on element ranges and the EMA buffers, in the Adam launch ----
    @staticmethod
    def _opt(opt):
        """An OptArgs, a dict(decay_mul, ema_omd, ranges) as optim.Optim.args_at returns it, or None (a null pointer)."""
        if opt is None or isinstance(opt, OptArgs):
            return opt
        return opt_args(opt.get("decay_mul", 1.0), opt.get("ema_omd", 0.0), opt.get("ranges", ()))

    def adam_step_opt(self, params, grads, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0, opt=None, ema=None,
                      aux=None, aux_ema=None, n_aux=None, n=None):
        """cvae_adam_step with the options `opt`; ema / aux / aux_ema: fp32 device tensors or None."""
        opt = self._opt(opt)
        n_aux = (0 if aux is None else aux.numel()) if n_aux is None else n_aux
        self._check(self.lib.cvae_adam_step_opt(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v),
                                                params.numel() if n is None else n, step, lr, b1, b2, eps, grad_scale,
                                                None if opt is None else C.byref(opt), _ptr(ema), _ptr(aux), _ptr(aux_ema),
                                                n_aux, _stream()))

    def adam_step_guarded_opt(self, params, grads, m, v, state, eps=1e-8, opt=None, ema=None, aux=None, aux_ema=None,
                              n_aux=None, n=None):
        """cvae_adam_step_guarded with the options `opt`; the record of `state` decides, as there."""
        opt = self._opt(opt)
        n_aux = (0 if aux is None else aux.numel()) if n_aux is None else n_aux
        self._check(self.lib.cvae_adam_step_guarded_opt(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v),
                                                        params.numel() if n is None else n, eps, self._guard_ptr(state),
                                                        None if opt is None else C.byref(opt), _ptr(ema), _ptr(aux),
                                                        _ptr(aux_ema), n_aux, _stream()))

    # ---- the training trace (include/cvae.h; trace.py): ring and records are caller-owned device tensors of any dtype ----
    @staticmethod
    def _raw(t, nbytes, what):
        """The address of a contiguous device tensor of at least `nbytes` bytes; None stays None, an int is an address."""
        if t is None or isinstance(t, int):
            return t
        assert t.is_cuda and t.is_contiguous() and t.numel() * t.element_size() >= nbytes, f"{what}: need {nbytes} contiguous device bytes"
        return t.data_ptr()

    def trace_push(self, ring, capacity, step, lr, loss_scalars, n_scalars=None, guard=None):
        """cvae_trace_push: row (step - 1) % capacity of `ring` (capacity rows of 128 bytes); guard: a guard state or None."""
        n_scalars = loss_scalars.numel() if n_scalars is None else n_scalars
        self._check(self.lib.cvae_trace_push(self.h, self._raw(ring, 128 * max(int(capacity), 0), "trace ring"), int(capacity), int(step),
                                             float(lr), _ptr(loss_scalars), int(n_scalars),
                                             None if guard is None else self._guard_ptr(guard), _stream()))

    def tensor_stats(self, params, grads, m, v, ranges, step, out, scratch, lr=0.0, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0,
                     guard=None, n=None):
        """cvae_tensor_stats on the element ranges [(begin, end), ...]: len(ranges) records of 48 bytes into `out`."""
        nt, b, e = _range_arrays(ranges)
        need = self.lib.cvae_tensor_stats_scratch_bytes(nt, b, e)            # negative: a table the entry itself refuses below
        assert need < 0 or isinstance(scratch, int) or scratch is None or scratch.numel() * scratch.element_size() >= need, \
            f"tensor scratch: need {need} bytes"
        self._check(self.lib.cvae_tensor_stats(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), params.numel() if n is None else n,
                                               nt, b, e, int(step), float(lr), b1, b2, eps, grad_scale,
                                               None if guard is None else self._guard_ptr(guard),
                                               self._raw(out, 48 * nt, "tensor records"), self._raw(scratch, 16, "tensor scratch"),
                                               _stream()))

    @staticmethod
    def guard_record(state):
        """The record of `state` on the host (one device -> host copy: a sync)."""
        raw = state[:C.sizeof(GuardRecord) // 8].cpu().numpy().tobytes()
        return GuardRecord.from_buffer_copy(raw)

    # ---- critic + input pipeline ----
    def critic_forward(self, B, x, critic_params, pred):
        self._check(self.lib.cvae_critic_forward(self.h, B, _ptr(x), _ptr(critic_params), _ptr(pred), _stream()))

    def critic_grad_scratch_bytes(self, B):
        n = self.lib.cvae_critic_grad_scratch_bytes(self.h, B)
        if n < 0:
            raise CvaeError(f"cvae_critic_grad_scratch_bytes: {self.lib.cvae_last_error().decode()}")
        return n

    def critic_grad(self, B, x, target, keep, dropout_p, loss_kind, critic_params, grads, pred, loss_scalars, scratch, decisions=None):
        """One critic training step without the optimizer (include/cvae.h): keep (B, 800) uint8 or None, loss_kind 0 = BCE,
        1 = MSE; grads cvae_critic_train_floats() floats, loss_scalars 4, decisions (B, 11072) uint8 or None."""
        assert grads.numel() >= CRITIC_TRAIN_FLOATS and pred.numel() >= B and loss_scalars.numel() >= 4 and target.numel() >= B
        assert keep is None or keep.numel() >= B * CRITIC_KEEP
        assert decisions is None or decisions.numel() >= B * CRITIC_DECISIONS
        assert scratch.is_cuda and scratch.is_contiguous() and scratch.numel() * scratch.element_size() >= self.critic_grad_scratch_bytes(B)
        self._check(self.lib.cvae_critic_grad(self.h, B, _ptr(x), _ptr(target), self._u8(keep, "keep"), float(dropout_p), int(loss_kind),
                                              _ptr(critic_params), _ptr(grads), _ptr(pred), _ptr(loss_scalars),
                                              self._u8(decisions, "decisions"), scratch.data_ptr(), _stream()))

    # ---- critic-side masks: embeddings, the logit's input gradient, occlusion (include/cvae.h) ----
    def critic_collect(self, B, x, critic_params, pred, embeds=(None,) * 5):
        """Eval-mode forward + the five tensors of Critic.forward(X, collect=True); any of `embeds` (e1..e5) may be None."""
        assert len(embeds) == 5 and pred.numel() >= B and x.numel() >= B * 3 * 64 * 64
        for e, shape in zip(embeds, CRITIC_EMBED_SHAPES):
            assert e is None or e.numel() >= B * shape[0] * shape[1] * shape[2]
        self._check(self.lib.cvae_critic_collect(self.h, B, _ptr(x), _ptr(critic_params), _ptr(pred), *[_ptr(e) for e in embeds], _stream()))

    def critic_saliency(self, B, x, critic_params, steps, pred, map_, max_values, grad=None, decisions=None):
        """d logit / d x (steps == 1) or integrated gradients from black (steps 2..256): pred (B), map_ (B,64,64), max_values (B),
        grad (B,3,64,64) or None, decisions (B, 11072) uint8 or None."""
        assert x.numel() >= B * 3 * 64 * 64 and pred.numel() >= B and map_.numel() >= B * 64 * 64 and max_values.numel() >= B
        assert grad is None or grad.numel() >= B * 3 * 64 * 64
        assert decisions is None or decisions.numel() >= B * CRITIC_DECISIONS
        self._check(self.lib.cvae_critic_saliency(self.h, B, _ptr(x), _ptr(critic_params), int(steps), _ptr(pred), _ptr(grad), _ptr(map_),
                                                  _ptr(max_values), self._u8(decisions, "decisions"), _stream()))

    def critic_occlusion(self, B, x, critic_params, patch, fill_rgb, pred, drop, map_, max_values):
        """Occlusion sensitivity with non-overlapping patch x patch windows (4, 8 or 16) filled with fill_rgb (three floats):
        pred (B), drop (B, 64/patch, 64/patch), map_ (B,64,64), max_values (B)."""
        g = 64 // int(patch) if int(patch) in CRITIC_OCCLUSION_PATCHES else 0
        assert x.numel() >= B * 3 * 64 * 64 and pred.numel() >= B and map_.numel() >= B * 64 * 64 and max_values.numel() >= B
        assert drop.numel() >= B * g * g
        r, gr, b = (float(v) for v in fill_rgb)
        self._check(self.lib.cvae_critic_occlusion(self.h, B, _ptr(x), _ptr(critic_params), int(patch), r, gr, b, _ptr(pred), _ptr(drop),
                                                   _ptr(map_), _ptr(max_values), _stream()))

    # ---- per-frame critic scores and the pooled record of a held-out set (include/cvae.h) ----
    def critic_score_state(self, device):
        """A fresh pooled record on `device`: a float64 tensor of CRITIC_SCORE_STATE_DOUBLES values, initialised."""
        state = torch.empty(self.lib.cvae_critic_score_state_bytes() // 8, dtype=torch.float64, device=device)
        self.critic_score_init(state)
        return state

    def _critic_score_ptr(self, state):
        if state is None:
            return None
        ptr = _ptr64(state)
        assert isinstance(state, int) or state.numel() * 8 >= self.lib.cvae_critic_score_state_bytes(), "critic score state: too small"
        return ptr

    def critic_score_init(self, state):
        self._check(self.lib.cvae_critic_score_init(self.h, self._critic_score_ptr(state), _stream()))

    def critic_score_scratch_bytes(self, B):
        n = self.lib.cvae_critic_score_scratch_bytes(self.h, B)
        if n < 0:
            raise CvaeError(f"cvae_critic_score_scratch_bytes: {self.lib.cvae_last_error().decode()}")
        return n

    def critic_score(self, B, frames_u8, targets, critic_params, idx=None, per_frame=None, state=None, scratch=None):
        """One launch (include/cvae.h): rows (B, CRITIC_SCORE_COLS) of frames_u8[idx] ((N,64,64,3) uint8) against targets[idx]
        into `per_frame` and / or the batch into the pooled record `state`; idx (>= B) int64 on the device, or None = the first
        B frames; scratch (critic_score_scratch_bytes(B) bytes) holds the rows when per_frame is None."""
        n = frames_u8.shape[0]
        assert tuple(frames_u8.shape[1:]) == (64, 64, 3) and targets.numel() >= n
        assert idx is None or idx.numel() >= B
        assert per_frame is None or per_frame.numel() >= B * CRITIC_SCORE_COLS
        assert scratch is None or (scratch.is_cuda and scratch.is_contiguous()
                                   and scratch.numel() * scratch.element_size() >= self.critic_score_scratch_bytes(B))
        self._check(self.lib.cvae_critic_score(self.h, B, self._u8(frames_u8, "frames"), _ptr(targets), n, self._i64(idx, "idx"),
                                               _ptr(critic_params), _ptr(per_frame), self._critic_score_ptr(state),
                                               None if scratch is None else scratch.data_ptr(), _stream()))

    def preprocess_u8(self, B, frames_u8, x):
        self._check(self.lib.cvae_preprocess_u8(self.h, B, self._u8(frames_u8, "frames"), _ptr(x), _stream()))

    def diff_grey(self, B, recon_one, recon_zero, diff):
        self._check(self.lib.cvae_diff_grey(self.h, B, _ptr(recon_one), _ptr(recon_zero), _ptr(diff), _stream()))

    # ---- the training set on the device (load_minerl_data, vae_utility.py:393-461; episodes.py) ----
    @staticmethod
    def _curate_sizes(offsets, preds, counts, first, sel):
        """(n_traj, n_frames) of one chunk, after the size checks both selection calls share."""
        n_traj, n_frames = offsets.numel() - 1, preds.numel()
        assert sel.numel() >= n_frames and counts.numel() >= 3 * n_traj and first.numel() >= n_traj
        return n_traj, n_frames

    def curate_select(self, offsets, preds, collect, total_images, running, counts, first, span, sel):
        """One chunk of whole trajectories: offsets (n_traj+1) int64, preds (n_frames) fp32, running (1) int64 in/out,
        counts (n_traj,3), first (n_traj), span (2), sel (>= n_frames) int64 — all device tensors (include/cvae.h)."""
        n_traj, n_frames = self._curate_sizes(offsets, preds, counts, first, sel)
        self._check(self.lib.cvae_curate_select(self.h, n_traj, self._i64(offsets, "offsets"), n_frames, _ptr(preds),
                                                int(collect), int(total_images), self._i64(running, "running"),
                                                self._i64(counts, "counts"), self._i64(first, "first"),
                                                self._i64(span, "span"), self._i64(sel, "sel"), _stream()))

    def gather_frames_u8(self, src, src_preds, sel, max_count, span, dst, dst_preds):
        """dst[span[0] + k] = src[sel[k]] (uint8 (N,W,W,3)) and dst_preds likewise, k < span[1] <= max_count."""
        assert sel.numel() >= max_count
        self._check(self.lib.cvae_gather_frames_u8(self.h, int(src.shape[1]), self._u8(src, "src"), _ptr(src_preds), src.shape[0],
                                                   self._i64(sel, "sel"), int(max_count), self._i64(span, "span"),
                                                   self._u8(dst, "dst"), _ptr(dst_preds), dst.shape[0], _stream()))

    def preprocess_u8_gather(self, B, frames_u8, preds, idx, x, pred):
        """x[b] = frames_u8[idx[b]] / 255 (CHW fp32), pred[b] = preds[idx[b]]; idx (>= B) int64 in [0, N) on the device."""
        w = frames_u8.shape[1]
        assert idx.numel() >= B and preds.numel() >= frames_u8.shape[0] and x.numel() >= B * 3 * w * w and pred.numel() >= B
        self._check(self.lib.cvae_preprocess_u8_gather(self.h, B, int(frames_u8.shape[1]), self._u8(frames_u8, "frames"), _ptr(preds),
                                                       frames_u8.shape[0], self._i64(idx, "idx"), _ptr(x), _ptr(pred), _stream()))

    # ---- the recon branch (the second VAE's dataset, vae_utility.py:422-443) ----
    def curate_select_recon(self, offsets, preds, collect, total_images, running, counts, first, sel_first, span,
                            ent_frame, ent_kind, ent_sel, sel):
        """curate_select with two entries per mid frame: running / first / span[0..1] count entries; sel_first (n_traj),
        span (3), ent_frame / ent_sel (>= 2 n_frames) int64, ent_kind (>= 2 n_frames) int32, sel (>= n_frames) int64."""
        n_traj, n_frames = self._curate_sizes(offsets, preds, counts, first, sel)
        assert span.numel() >= 3 and sel_first.numel() >= n_traj
        assert min(ent_frame.numel(), ent_kind.numel(), ent_sel.numel()) >= 2 * n_frames
        self._check(self.lib.cvae_curate_select_recon(
            self.h, n_traj, self._i64(offsets, "offsets"), n_frames, _ptr(preds), int(collect), int(total_images),
            self._i64(running, "running"), self._i64(counts, "counts"), self._i64(first, "first"),
            self._i64(sel_first, "sel_first"), self._i64(span, "span"), self._i64(ent_frame, "ent_frame"),
            self._i32(ent_kind, "ent_kind"), self._i64(ent_sel, "ent_sel"), self._i64(sel, "sel"), _stream()))

    def recon_zcat(self, n_entries, ent_sel, ent_kind, mu, sel_preds, zcat):
        """zcat[e] = (mu[ent_sel[e]], ent_kind[e] == 0 ? sel_preds[ent_sel[e]] : 0) for a run of n_entries entries."""
        assert ent_sel.numel() >= n_entries and ent_kind.numel() >= n_entries and zcat.numel() >= 33 * n_entries
        n_sel = sel_preds.numel()
        assert mu.numel() >= 32 * n_sel
        self._check(self.lib.cvae_recon_zcat(self.h, n_entries, self._i64(ent_sel, "ent_sel"), self._i32(ent_kind, "ent_kind"), _ptr(mu),
                                             _ptr(sel_preds), n_sel, _ptr(zcat), _stream()))

    def gather_f32(self, B, frames, preds, idx, x, pred):
        """x[b] = frames[idx[b]] ((N,3,W,W) fp32, bit copy), pred[b] = preds[idx[b]]; idx (>= B) int64 in [0, N) on the device."""
        w = frames.shape[2]
        assert frames.dim() == 4 and frames.shape[1] == 3 and frames.shape[3] == w
        assert idx.numel() >= B and preds.numel() >= frames.shape[0] and x.numel() >= B * 3 * w * w and pred.numel() >= B
        self._check(self.lib.cvae_gather_f32(self.h, B, int(w), _ptr(frames), _ptr(preds), frames.shape[0],
                                             self._i64(idx, "idx"), _ptr(x), _ptr(pred), _stream()))

    # ---- the augmented batch gathers (augment.py) ----
    @staticmethod
    def _aug(aug):
        """An AugmentParams structure, a (key, flip_below, max_shift, gain_q16) tuple as augment.Augment.at() returns it, or
        None (a null pointer: CVAE_EINVAL) -> the ctypes argument."""
        if aug is not None and not isinstance(aug, AugmentParams):
            aug = AugmentParams(*aug)
        return None if aug is None else C.byref(aug)

    def preprocess_u8_gather_aug(self, B, frames_u8, preds, idx, aug, x, pred, applied=None):
        """preprocess_u8_gather with the flip / shift / gain `aug` draws per sample; applied: (>= B, 4) int32 device rows
        [flip, dx, dy, num - 2^31] or None."""
        w = frames_u8.shape[1]
        assert idx.numel() >= B and preds.numel() >= frames_u8.shape[0] and x.numel() >= B * 3 * w * w and pred.numel() >= B
        assert applied is None or isinstance(applied, int) or applied.numel() >= 4 * B
        self._check(self.lib.cvae_preprocess_u8_gather_aug(self.h, B, int(w), self._u8(frames_u8, "frames"), _ptr(preds),
                                                           frames_u8.shape[0], self._i64(idx, "idx"), self._aug(aug), _ptr(x),
                                                           _ptr(pred), self._i32(applied, "applied"), _stream()))

    def gather_f32_aug(self, B, frames, preds, idx, aug, x, pred, applied=None):
        """gather_f32 with the flip / shift `aug` draws per sample (bit copies; a gain is CVAE_EINVAL); applied as above."""
        w = frames.shape[2]
        assert frames.dim() == 4 and frames.shape[1] == 3 and frames.shape[3] == w
        assert idx.numel() >= B and preds.numel() >= frames.shape[0] and x.numel() >= B * 3 * w * w and pred.numel() >= B
        assert applied is None or isinstance(applied, int) or applied.numel() >= 4 * B
        self._check(self.lib.cvae_gather_f32_aug(self.h, B, int(w), _ptr(frames), _ptr(preds), frames.shape[0],
                                                 self._i64(idx, "idx"), self._aug(aug), _ptr(x), _ptr(pred),
                                                 self._i32(applied, "applied"), _stream()))

    # ---- segmentation evaluation (eval_textured_frames, vae_utility.py:162-212) ----
    def diff_normalize(self, B, diff, mean_max, diff_factor, thr, gt, diff_u8, mask=None, counts=None, hist=None):
        """uint8 masks of the set-wide normalisation; counts (B,3) (tp, fn, fp); hist (2,256) is ADDED to."""
        self._check(self.lib.cvae_diff_normalize(self.h, B, _ptr(diff), float(mean_max), float(diff_factor), int(thr),
                                                 self._u8(gt, "gt"), self._u8(diff_u8, "diff_u8"), self._u8(mask, "mask"),
                                                 self._i64(counts, "counts"), self._i64(hist, "hist"), _stream()))

    def mask_counts(self, B, mask, gt, counts):
        self._check(self.lib.cvae_mask_counts(self.h, B, self._u8(mask, "mask"), self._u8(gt, "gt"),
                                              self._i64(counts, "counts"), _stream()))

    # ---- objects from masks (include/cvae.h; objects.py) ----
    _u16 = staticmethod(lambda t, what: _dev_ptr(t, torch.uint16, what))

    def mask_objects(self, B, mask, params, info, values=None, mask_out=None, labels=None, table=None, flags=0):
        """cvae_mask_objects: params an ObjectParams or None (a null pointer); info (B,4) int32; mask_out (B,W,W) uint8, labels
        (B,W,W) uint16 and table (B,M,8) int32 or None."""
        self._check(self.lib.cvae_mask_objects(self.h, B, self._u8(mask, "mask"), self._u8(values, "values"),
                                               None if params is None else C.byref(params), self._u8(mask_out, "mask_out"),
                                               self._u16(labels, "labels"), self._i32(info, "info"), self._i32(table, "table"),
                                               _stream(), int(flags)))

    def object_overlap(self, B, labels_a, labels_b, M, inter, flags=0):
        """cvae_object_overlap: inter (B,M,M) int32 = pixels with labels_a == i + 1 and labels_b == j + 1."""
        self._check(self.lib.cvae_object_overlap(self.h, B, self._u16(labels_a, "labels_a"), self._u16(labels_b, "labels_b"), int(M),
                                                 self._i32(inter, "inter"), _stream(), int(flags)))

    def crf_scratch_bytes(self, B):
        n = self.lib.cvae_crf_scratch_bytes(self.h, B)
        if n < 0:
            raise CvaeError(f"cvae_crf_scratch_bytes: {self.lib.cvae_last_error().decode()}")
        return n

    def dense_crf(self, B, frames_u8, prob1, params, labels, q1, scratch):
        """params: CrfParams; scratch: a device tensor of at least crf_scratch_bytes(B) bytes."""
        assert scratch.is_cuda and scratch.is_contiguous() and scratch.numel() * scratch.element_size() >= self.crf_scratch_bytes(B)
        self._check(self.lib.cvae_dense_crf(self.h, B, self._u8(frames_u8, "frames"), _ptr(prob1), C.byref(params),
                                            self._u8(labels, "labels"), _ptr(q1), scratch.data_ptr(), _stream()))

    def crf_grid_group(self):
        """variants per pair pass of cvae_crf_grid"""
        return self.lib.cvae_crf_grid_group(self.h)

    def crf_grid_scratch_bytes(self, B, n_variants):
        n = self.lib.cvae_crf_grid_scratch_bytes(self.h, B, n_variants)
        if n < 0:
            raise CvaeError(f"cvae_crf_grid_scratch_bytes: {self.lib.cvae_last_error().decode()}")
        return n

    def crf_grid(self, B, frames_u8, prob1, diff_u8, gt, kernel, variants, snaps, counts, labels, q1, scratch):
        """kernel (alpha, beta, gamma); variants [(thr, p_floor, w1, w2), ...]; snaps ascending iteration counts (host
        values, read before the call returns); counts (len(snaps), K, B, 3) int64, labels (K,B,W,W) uint8, q1 (K,B,W,W)
        fp32 or None; scratch: a device tensor of at least crf_grid_scratch_bytes(B, K) bytes.  Every check is the library's."""
        variants, snaps = list(variants), list(snaps)
        if 1 <= len(variants) <= CRF_GRID_MAX_VARIANTS:
            assert scratch.is_cuda and scratch.is_contiguous() and \
                scratch.numel() * scratch.element_size() >= self.crf_grid_scratch_bytes(B, len(variants))
        va = (CrfVariant * max(1, len(variants)))(*[CrfVariant(int(t), float(pf), float(w1), float(w2)) for t, pf, w1, w2 in variants])
        sa = (C.c_int32 * max(1, len(snaps)))(*[int(s) for s in snaps])
        alpha, beta, gamma = (float(x) for x in kernel)
        self._check(self.lib.cvae_crf_grid(self.h, B, self._u8(frames_u8, "frames"), _ptr(prob1), self._u8(diff_u8, "diff_u8"),
                                           self._u8(gt, "gt"), alpha, beta, gamma, va, len(variants), sa, len(snaps),
                                           self._i64(counts, "counts"), self._u8(labels, "labels"), _ptr(q1),
                                           scratch.data_ptr(), _stream()))

    # ---- the reference's pictures (get_final_frame / get_injected_img, vae_utility.py:240-322; render.py) ----
    def compose_frames(self, B, panels, row_offset, out, overlay=None, atlas=None, label_idx=None, label_xy=(0, 0), clamp=False):
        """panels: [(kind, device tensor, batch stride in elements), ...] of w x w panels side by side -> out
        (B, row_offset + w, len(panels) * w, 3) uint8.  overlay (row_offset + w, len(panels) * w) uint8 and atlas (L, lh, lw) uint8
        with label_idx (B) int32 draw white text (include/cvae.h)."""
        w, n = self.width, len(panels)
        if not 1 <= n <= MAX_PANELS:
            raise ValueError(f"{n} panels, need 1..{MAX_PANELS}")
        need = {PANEL_F32_CHW: (torch.float32, 3 * w * w), PANEL_U8_HWC: (torch.uint8, 3 * w * w),
                PANEL_U8_GREY: (torch.uint8, w * w), PANEL_MASK: (torch.uint8, w * w)}
        arr = (Panel * n)()
        for i, (kind, t, stride) in enumerate(panels):
            dtype, numel = need[kind]
            ptr = _dev_ptr(t, dtype, f"panel {i}")
            assert stride >= 0 and t.numel() >= (B - 1) * stride + numel, f"panel {i}: {t.numel()} elements for {B} pictures at stride {stride}"
            arr[i] = Panel(kind, 0, ptr, stride)
        assert out.numel() == B * (row_offset + w) * n * w * 3, "out: wrong size"
        if overlay is not None:
            assert overlay.numel() == (row_offset + w) * n * w, "overlay: wrong size"
        L = lh = lw = 0
        if atlas is not None:
            L, lh, lw = atlas.shape
            assert label_idx is not None and label_idx.numel() >= B, "label_idx: need a contiguous int32 device tensor of B entries"
        self._check(self.lib.cvae_compose_frames(self.h, B, n, arr, int(row_offset), COMPOSE_CLAMP if clamp else 0,
                                                 self._u8(overlay, "overlay"), self._u8(atlas, "atlas"), L, lh, lw,
                                                 None if atlas is None else self._i32(label_idx, "label_idx"), int(label_xy[0]), int(label_xy[1]),
                                                 self._u8(out, "out"), _stream()))

    def inject_zcat(self, n_images, n_rewards, mu, rewards, zcat):
        """zcat[b * n_rewards + r] = (mu[b], rewards[r]): the decoder input of the batched -inject."""
        assert mu.numel() >= 32 * n_images and rewards.numel() >= n_rewards and zcat.numel() >= 33 * n_images * n_rewards
        self._check(self.lib.cvae_inject_zcat(self.h, n_images, n_rewards, _ptr(mu), _ptr(rewards), _ptr(zcat), _stream()))

    # ---- in-step kernel probe (bench.py roofline) ----
    def probe_config(self, ids):
        mask = 0
        for i in ids:
            mask |= 1 << i
        self._check(self.lib.cvae_probe_config(self.h, mask))

    def probe_read(self, pid, cap=128):
        buf = (C.c_float * cap)()
        n = self.lib.cvae_probe_read(self.h, pid, buf, cap)
        return [buf[i] for i in range(n)]

    # ---- per-op entry points (tests, roofline probe) ----
    # "bf16x9" / "bf16x6" handles: the conv ops of layers 1..4 run the step's split-operand kernels and need `scratch`
    # "bf16" handles: the conv ops of layers 1..8 and op_d4_bwd run the step's bf16 kernels on bf16 activations (passed as the
    # fp32 tensors that hold them, two elements per float) and fp32 weights; they need `scratch`
    def op_scratch_floats(self, B):
        return self.lib.cvae_op_scratch_floats(self.h, B)

    def op_bn_partial_floats(self, layer, B):
        return self.lib.cvae_op_bn_partial_floats(self.h, layer, B)

    def op_msssim_ws_floats(self, B):
        return self.lib.cvae_op_msssim_ws_floats(self.h, B)

    def op_conv_fwd(self, layer, B, inp, w, bias, out, bn_partials=None, scratch=None):
        self._check(self.lib.cvae_op_conv_fwd(self.h, layer, B, _ptr(inp), _ptr(w), _ptr(bias), _ptr(out),
                                              _ptr(bn_partials), _ptr(scratch), _stream()))

    def op_conv_dgrad(self, layer, B, dout, w, mask_src, din, scratch=None):
        self._check(self.lib.cvae_op_conv_dgrad(self.h, layer, B, _ptr(dout), _ptr(w), _ptr(mask_src), _ptr(din),
                                                _ptr(scratch), _stream()))

    def op_conv_wgrad(self, layer, B, inp, dout, dw, dbias, scratch):
        self._check(self.lib.cvae_op_conv_wgrad(self.h, layer, B, _ptr(inp), _ptr(dout), _ptr(dw), _ptr(dbias),
                                                _ptr(scratch), _stream()))

    def op_e1_wgrad_fused(self, B, x, y0, a0, d_a0, coef0, bcoef0, w1, b1, dw, dbias, scratch, flags=0):
        """E1's weight gradient as the step runs it (block 0's BatchNorm / pool / ReLU backward applied while staging); flags bit 0
        (bf16 handles): stage the packed bf16 frame, which the entry writes into scratch first."""
        self._check(self.lib.cvae_op_e1_wgrad_fused(self.h, B, _ptr(x), _ptr(y0), _ptr(a0), _ptr(d_a0), _ptr(coef0), _ptr(bcoef0),
                                                    _ptr(w1), _ptr(b1), _ptr(dw), _ptr(dbias), _ptr(scratch), int(flags), _stream()))

    def op_d4_bwd(self, B, o3, d_recon, recon, w, dout, d_o3, dw, db, scratch):
        self._check(self.lib.cvae_op_d4_bwd(self.h, B, _ptr(o3), _ptr(d_recon), _ptr(recon), _ptr(w), _ptr(dout),
                                            _ptr(d_o3), _ptr(dw), _ptr(db), _ptr(scratch), _stream()))

    def op_bn_pool_act_fwd(self, layer, B, y, bn_partials, gamma, beta, run_mean, run_var, coef, a, scratch, train=True):
        self._check(self.lib.cvae_op_bn_pool_act_fwd(self.h, layer, B, _ptr(y), _ptr(bn_partials), _ptr(gamma),
                                                     _ptr(beta), _ptr(run_mean), _ptr(run_var), _ptr(coef), _ptr(a),
                                                     _ptr(scratch), int(train), _stream()))

    def op_bn_pool_act_bwd(self, layer, B, y, a, da, coef, gamma, dy, dgamma, dbeta, dbias, scratch):
        self._check(self.lib.cvae_op_bn_pool_act_bwd(self.h, layer, B, _ptr(y), _ptr(a), _ptr(da), _ptr(coef),
                                                     _ptr(gamma), _ptr(dy), _ptr(dgamma), _ptr(dbeta), _ptr(dbias),
                                                     _ptr(scratch), _stream()))

    def op_conv_tiles_per_partial(self, layer, B):
        n = self.lib.cvae_op_conv_tiles_per_partial(self.h, layer, B)
        if n < 1:
            raise CvaeError(f"cvae_op_conv_tiles_per_partial: {self.lib.cvae_last_error().decode()}")
        return n

    def op_conv_wgrad_plan(self, layer, B):
        """(tiles, splits, tiles per split) of op_conv_wgrad's kernel (layer 0: op_e1_wgrad_fused's) on a bf16 handle, from the launchers
        (no launch)."""
        out = (C.c_int32 * 3)()
        self._check(self.lib.cvae_op_conv_wgrad_plan(self.h, layer, B, out))
        return tuple(out)

    def op_bn_fwd_finalize(self, layer, B, bn_partials, tiles_per_partial, gamma, beta, run_mean, run_var, coef, scratch, train=True):
        self._check(self.lib.cvae_op_bn_fwd_finalize(self.h, layer, B, _ptr(bn_partials), tiles_per_partial, _ptr(gamma), _ptr(beta),
                                                     _ptr(run_mean), _ptr(run_var), _ptr(coef), _ptr(scratch), int(train), _stream()))

    def op_msssim(self, B, img1, img2, ws, scalars, d_img1=None):
        self._check(self.lib.cvae_op_msssim(self.h, B, _ptr(img1), _ptr(img2), _ptr(ws), _ptr(scalars),
                                            _ptr(d_img1), _stream()))

    # the latent layers (fc.hip): flat / h_out / dh / dflat in the handle's storage type (bf16 elements packed two per float on a
    # "bf16" handle), native weights Wfc [K][64] and Wd [33][K]; scratch: op_latent_scratch_floats(B) floats
    def op_latent_scratch_floats(self, B):
        n = self.lib.cvae_op_latent_scratch_floats(self.h, B)
        if n < 0:
            self._check(int(n))
        return n

    def op_fc_fwd(self, B, flat, wfc, bfc, eps, pred, mu, logvar, zcat, scratch):
        self._check(self.lib.cvae_op_fc_fwd(self.h, B, _ptr(flat), _ptr(wfc), _ptr(bfc), _ptr(eps), _ptr(pred), _ptr(mu),
                                            _ptr(logvar), _ptr(zcat), _ptr(scratch), _stream()))

    def op_decin_fwd(self, B, zcat, wd, bd, h_out):
        self._check(self.lib.cvae_op_decin_fwd(self.h, B, _ptr(zcat), _ptr(wd), _ptr(bd), _ptr(h_out), _stream()))

    def op_decin_bwd(self, B, zcat, dh, wd, dwd, dbd, dzcat, scratch):
        self._check(self.lib.cvae_op_decin_bwd(self.h, B, _ptr(zcat), _ptr(dh), _ptr(wd), _ptr(dwd), _ptr(dbd), _ptr(dzcat),
                                               _ptr(scratch), _stream()))

    def op_fc_bwd(self, B, flat, wfc, dzcat, eps, logvar, dmu_loss, dlv_loss, dwfc, dbfc, dflat, scratch):
        self._check(self.lib.cvae_op_fc_bwd(self.h, B, _ptr(flat), _ptr(wfc), _ptr(dzcat), _ptr(eps), _ptr(logvar),
                                            _ptr(dmu_loss), _ptr(dlv_loss), _ptr(dwfc), _ptr(dbfc), _ptr(dflat),
                                            _ptr(scratch), _stream()))
