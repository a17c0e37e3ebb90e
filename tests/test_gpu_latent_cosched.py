"""The merged latent launches of fc.hip (decin_bwd: dWd | dbd with the d_zcat slabs; fc_bwd: dWfc, dflat and the first stage of dbfc)
and the batch-dependent images per workgroup of decin_fwd / fc_bwd_dflat, through the per-op entry points.

The batches come from cvae_op_latent_plan at the device's compute-unit count: 1, 33, 129 (the first batch with two
latent_gemm row blocks: every job range behind it shifts), and every T at which the images per workgroup of decin_fwd or dflat change
between T and T + 1, with T + 1.  One 128 x 128 case (K = 16 384: 512 blocks per batch-contracted GEMM, more than the device has compute
units, so dflat takes the launch of its own there and the 64 x 64 cases the shared one) runs at B = 17.  fp32 and bf16 storage.  Everything is compared bit for bit; test_gpu_latent_ops.py holds the kernels to their round-off bounds.

(a) row consistency: h (decin_fwd) and dflat (fc_bwd) of the first T rows of a (T + 1)-row call equal the T-row call: a row's sums do
    not depend on how the rows are grouped into workgroups.
(b) independence of the jobs of a launch: with the outputs of the OTHER job pre-filled with NaN (dzcat against dWd / dbd, dflat against
    dWfc / dbfc), NaN in the scratch and NaN in the PAD rows behind every batch-indexed input, each output equals the clean call's
    (zero-filled outputs, scratch and padding).
(c) the same call twice gives the same bits."""
import functools
import zlib

import pytest
import torch

from critic_vae_amd import lib as cvlib
from ws_tools import ALL_ONES, ZERO, poison, same_bits

pytestmark = pytest.mark.gpu

PAD = 256                    # rows behind every batch-indexed buffer: the largest batch tile of fc.hip
STORAGE = ["f32", "bf16"]
PLAN_UPTO = 2100             # thresholds are looked for below this batch


def bottleneck(W):
    return 256 * (W // 16) ** 2


@functools.lru_cache(maxsize=None)
def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def thresholds(W, which=None):
    """Every T < PLAN_UPTO where the images per workgroup of decin_fwd ("di"), of dflat ("df") or of either (None) differ between T and
    T + 1 on this device, ascending."""
    plans = [None] + [cvlib.latent_plan(W, B, device_cus()) for B in range(1, PLAN_UPTO + 1)]
    key = {"di": lambda p: p["decin_fwd"]["imgs"], "df": lambda p: p["fc_bwd"]["imgs"],
           None: lambda p: (p["decin_fwd"]["imgs"], p["fc_bwd"]["imgs"])}[which]
    return [T for T in range(1, PLAN_UPTO) if key(plans[T]) != key(plans[T + 1])]


# A case names its batch; the thresholds are resolved on the device that runs the test (both kernels have three forms, so two thresholds
# each; where two coincide the case repeats a batch, which costs a few milliseconds).
NAMED = ["1", "33", "129"] + [f"{k}{n}{s}" for k in ("di", "df") for n in (0, 1) for s in ("", "+1")]


def batch_of(W, name):
    if name.isdigit():
        return int(name)
    return thresholds(W, name[:2])[int(name[2])] + (1 if name.endswith("+1") else 0)


def max_batch(W):
    return max(batch_of(W, n) for n in NAMED) + 1


CASES = [(64, n, m) for m in STORAGE for n in NAMED] + [(128, "17", m) for m in STORAGE]
cases = pytest.mark.parametrize("W,name,mode", CASES, ids=[f"w{w}-b{n}-{m}" for w, n, m in CASES])


@pytest.fixture(scope="module")
def handles():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    made = {}

    def get(W, mode):
        if (W, mode) not in made:
            made[W, mode] = cvlib.Handle(W, max_batch(W) if W == 64 else 17, precision=mode)
        return made[W, mode]
    yield get
    made.clear()


def test_the_plan_has_thresholds_on_this_device():
    """The batch list is not empty of what it is for: both kernels change their images per workgroup below PLAN_UPTO."""
    cus = device_cus()
    assert len(thresholds(64, "di")) == 2 and len(thresholds(64, "df")) == 2, (thresholds(64, "di"), thresholds(64, "df"))
    assert sorted(set(thresholds(64, "di")) | set(thresholds(64, "df"))) == thresholds(64)
    assert cvlib.latent_plan(64, 129, cus)["decin_bwd"]["jobs"]["gemm"] != cvlib.latent_plan(64, 128, cus)["decin_bwd"]["jobs"]["gemm"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs (made once per (W, rows, storage) on the device) and buffers
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def inputs(W, rows, bf):
    """Device fp32 / bf16 inputs of the three ops for `rows` images, without padding."""
    K = bottleneck(W)
    g = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr((W, rows, bf)).encode()))

    def rnd(*shape, scale=1.0, act=False):
        t = torch.randn(shape, generator=g, device="cuda") * scale
        return t.to(torch.bfloat16) if act and bf else t
    return {"zcat": rnd(rows, 33, scale=1.5), "wd": rnd(33, K, scale=33 ** -0.5), "bd": rnd(K, scale=33 ** -0.5),
            "dh": rnd(rows, K, act=True), "flat": rnd(rows, K, act=True), "wfc": rnd(K, 64, scale=K ** -0.5),
            "dzcat": rnd(rows, 33), "eps": rnd(rows, 32), "logvar": rnd(rows, 32, scale=2.0), "dmu": rnd(rows, 32, scale=0.5),
            "dlv": rnd(rows, 32, scale=0.5)}


def padded(t, B, pattern):
    """The first B rows of t followed by PAD rows of the pattern, in one allocation."""
    t = t.reshape(t.shape[0], -1)
    full = poison(torch.empty((B + PAD, t.shape[1]), dtype=t.dtype, device="cuda"), pattern)
    full[:B] = t[:B]
    return full


def arg(t):
    """The pointer argument of a buffer: bf16 storage travels as the packed fp32 view the binding expects."""
    return t if t.dtype == torch.float32 else t.reshape(-1).view(torch.float32)


def out(shape, pattern, bf=False):
    return poison(torch.empty(shape, dtype=torch.bfloat16 if bf else torch.float32, device="cuda"), pattern)


def scratch(H, B, pattern):
    return poison(torch.empty(H.op_latent_scratch_floats(B), device="cuda"), pattern)


def run_decin_fwd(H, W, B, rows, pad=ZERO):
    bf, i = H.precision == "bf16", inputs(W, rows, H.precision == "bf16")
    h = out((B, bottleneck(W)), ZERO, bf)
    H.op_decin_fwd(B, padded(i["zcat"], B, pad), i["wd"], i["bd"], arg(h))
    return {"h": h}


def run_decin_bwd(H, W, B, rows, pad=ZERO, fill=None, scr=ZERO):
    i, K, fill = inputs(W, rows, H.precision == "bf16"), bottleneck(W), fill or {}
    o = {"dwd": out(33 * K, fill.get("dwd", ZERO)), "dbd": out(K, fill.get("dbd", ZERO)), "dzcat": out((B, 33), fill.get("dzcat", ZERO))}
    H.op_decin_bwd(B, padded(i["zcat"], B, pad), arg(padded(i["dh"], B, pad)), i["wd"], o["dwd"], o["dbd"], o["dzcat"], scratch(H, B, scr))
    return o


def run_fc_bwd(H, W, B, rows, pad=ZERO, fill=None, scr=ZERO):
    bf, i, K, fill = H.precision == "bf16", inputs(W, rows, H.precision == "bf16"), bottleneck(W), fill or {}
    o = {"dwfc": out(K * 64, fill.get("dwfc", ZERO)), "dbfc": out(64, fill.get("dbfc", ZERO)), "dflat": out((B, K), fill.get("dflat", ZERO), bf)}
    p = {k: padded(i[k], B, pad) for k in ("flat", "dzcat", "eps", "logvar", "dmu", "dlv")}
    H.op_fc_bwd(B, arg(p["flat"]), i["wfc"], p["dzcat"], p["eps"], p["logvar"], p["dmu"], p["dlv"], o["dwfc"], o["dbfc"], arg(o["dflat"]),
                scratch(H, B, scr))
    return o


def assert_same(a, b, keys, what):
    torch.cuda.synchronize()
    for k in keys:
        assert not torch.isnan(a[k].float()).any(), f"{what}: {k} of the reference call holds NaN"
        assert same_bits(a[k], b[k]), f"{what}: {k} differs ({int((a[k] != b[k]).sum())} of {a[k].numel()} elements)"


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a) row consistency across every change of the images per workgroup
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", STORAGE)
def test_rows_do_not_depend_on_their_grouping(handles, mode):
    """(a): for every threshold T, h and dflat of rows 0..T-1 from a (T + 1)-row call equal the T-row call on the same rows."""
    W, H, cus = 64, handles(64, mode), device_cus()
    for T in thresholds(W):
        small, large = cvlib.latent_plan(W, T, cus), cvlib.latent_plan(W, T + 1, cus)
        assert (small["decin_fwd"]["imgs"], small["fc_bwd"]["imgs"]) != (large["decin_fwd"]["imgs"], large["fc_bwd"]["imgs"])
        a, b = run_decin_fwd(H, W, T, T + 1), run_decin_fwd(H, W, T + 1, T + 1)
        assert_same(a, {"h": b["h"][:T]}, ["h"], f"decin_fwd [{mode}] T = {T}")
        a, b = run_fc_bwd(H, W, T, T + 1), run_fc_bwd(H, W, T + 1, T + 1)
        assert_same(a, {"dflat": b["dflat"][:T]}, ["dflat"], f"fc_bwd [{mode}] T = {T}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# (b) the jobs of a launch do not read each other's outputs, the scratch or the padding; (c) the same call twice
# ---------------------------------------------------------------------------------------------------------------------------------------
@cases
def test_jobs_are_independent_and_calls_repeat(handles, W, name, mode):
    H, B = handles(W, mode), batch_of(W, name)
    what = f"[w{W} b{B} {mode}]"
    clean = run_decin_fwd(H, W, B, B)
    assert_same(clean, run_decin_fwd(H, W, B, B), ["h"], f"decin_fwd twice {what}")
    assert_same(clean, run_decin_fwd(H, W, B, B, pad=ALL_ONES), ["h"], f"decin_fwd, NaN padding {what}")

    clean = run_decin_bwd(H, W, B, B)
    assert_same(clean, run_decin_bwd(H, W, B, B), ["dwd", "dbd", "dzcat"], f"decin_bwd twice {what}")
    got = run_decin_bwd(H, W, B, B, pad=ALL_ONES, fill={"dzcat": ALL_ONES}, scr=ALL_ONES)
    assert_same(clean, got, ["dwd", "dbd", "dzcat"], f"decin_bwd, NaN in dzcat {what}")
    got = run_decin_bwd(H, W, B, B, pad=ALL_ONES, fill={"dwd": ALL_ONES, "dbd": ALL_ONES}, scr=ALL_ONES)
    assert_same(clean, got, ["dwd", "dbd", "dzcat"], f"decin_bwd, NaN in dWd / dbd {what}")

    clean = run_fc_bwd(H, W, B, B)
    assert_same(clean, run_fc_bwd(H, W, B, B), ["dwfc", "dbfc", "dflat"], f"fc_bwd twice {what}")
    got = run_fc_bwd(H, W, B, B, pad=ALL_ONES, fill={"dflat": ALL_ONES}, scr=ALL_ONES)
    assert_same(clean, got, ["dwfc", "dbfc", "dflat"], f"fc_bwd, NaN in dflat {what}")
    got = run_fc_bwd(H, W, B, B, pad=ALL_ONES, fill={"dwfc": ALL_ONES, "dbfc": ALL_ONES}, scr=ALL_ONES)
    assert_same(clean, got, ["dwfc", "dbfc", "dflat"], f"fc_bwd, NaN in dWfc / dbfc {what}")
