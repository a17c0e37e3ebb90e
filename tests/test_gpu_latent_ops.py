"""The latent-layer kernels of fc.hip, op by op, at every batch-tile edge.

The four per-op entry points (cvae_op_fc_fwd, cvae_op_decin_fwd, cvae_op_decin_bwd, cvae_op_fc_bwd) run the launchers of the step
alone: latent_gemm (128 rows per workgroup, FC_KS K slices) with fc_finish / decin_dz_finish, decin_fwd (16 images per workgroup),
fc_bwd_prep, colsum (one kernel up to 64 rows, another above), fc_bwd_dflat (32 images per workgroup) and the batch-contracted weight
gradients: bgemm_f32 (64 images per LDS tile, 16 per wave) on fp32 storage, bgemm_tr (256 images per tile, 64 per wave, the next tile
prefetched into registers) on bf16 storage.  The batches sit on both sides of each of those edges, on both storage types and frame sizes.

(a) parity: every element against plain torch in float64, inside the worst-case round-off bound of the kernel's own summation order,
    (n + c) * 2^-24 * (|A| @ |B| + |bias|).  n is the length of the serial sum (ws_tools: fc_split_terms, DECIN_TERMS, DFLAT_TERMS,
    batch_terms), c what the bound needs besides:
      mu, logvar   n = K / FC_KS + FC_KS, c = 2: the rounding of each product and the bias
      zcat         ZCAT_TERMS * 2^-24 * (|mu| + |eps exp(logvar / 2)|) from the mu / logvar the kernel returned; column 32 is pred, bitwise
      h            n = 33, c = 2: the bias that starts the fmaf chain, and one for the cross term of the output rounding
      d_zcat       n = K / FC_KS + FC_KS, c = 1: the rounding of each product
      dflat        n = 64 + 8 (the 8 are dml's own roundings, of the sum of |its terms|), c = 1: the cross term of the output rounding
      dWd, dbd     n = B + 4, c = 1: the rounding of each product
      dWfc, dbfc   n = B + 4, c = 8 + 1: dml's own roundings, the rounding of each product
    Tensors in bf16 storage (h, dflat on a "bf16" handle) add the output rounding 2^-8 |want| (ws_tools.BF16), the unit round-off of a
    round-to-nearest store of 8 significant bits: half a bf16 spacing is 2^-8 of a value just above a power of two.  (2^-9 is half
    of that and too tight for any correct kernel: the fp32 host restatement of decin_fwd and fc_bwd_dflat with a bf16 store, against
    float64 on these inputs, reaches 1.98 * 2^-9 |want|; the bound is 1.01 times that measured worst case, i.e. the provable maximum.)
    Inputs in bf16 storage are generated bf16-representable.
    Where the bf16 kernels round an fp32 operand on its way to the MFMA, the reference rounds the same operand:
    [zcat | 1] of dWd is an input, so its rounding is decided; dml of dWfc is computed by fc_bwd_prep in fp32, and a value that fp32 and
    float64 arithmetic put on different sides of a bf16 rounding boundary would move one product by 2^-8, which is no round-off of the
    sum.  The bf16 cases therefore choose the loss gradients d_mu / d_logvar (free inputs) so that every dml lands within fp32 round-off
    of a bf16-representable target of the size of its terms, about 2^-9 relative away from the nearest boundary: both roundings give the target.
(b) exact: small-integer operands (|v| <= 4; smaller where a bf16-stored result has to stay <= 256), the non-linear part switched off
    (eps = 0; logvar = 0 where it is an input, <= 0 where fc_fwd computes it, so that exp stays finite and 0 * exp is 0).  Every product
    and partial sum is an integer below 2^24: any summation order gives the integer result, and an image counted twice or not at all
    does not.
(c) one lit image: the batch-contracted outputs with every image zero but one must be that image's outer product, exactly, wherever it
    sits in the tile, wave and prefetch structure.
(d) padding: every batch-indexed input and output is allocated with PAD = 256 rows (one largest tile) past B.  The input padding holds
    NaN, the output padding and the tails behind the weight-shaped outputs and the scratch a sentinel.  Every run of (a), (b), (c) and
    (e) checks that the outputs hold no NaN (a contracted row >= B) and that the sentinel is untouched (an unguarded tail store).
(e) determinism: the same call twice, bit for bit.
(f) the KL term of cvae_loss from caller-supplied mu / logvar: the KLD scalar and d_mu / d_logvar against the float64 formula.

The measured head-room of every bound is in LABNOTES.md."""
import functools
import math
import zlib

import pytest
import torch

from critic_vae_amd import lib as cvlib
from ws_tools import (ALL_ONES, BF16, DECIN_TERMS, DFLAT_TERMS, DML_TERMS, U32, ZCAT_TERMS, batch_terms, fc_split_terms, poison, same_bits,
                      within)

pytestmark = pytest.mark.gpu

PAD = 256                    # rows past B in every batch-indexed buffer: BG_BT, the largest batch tile of fc.hip
SENTINEL = 0xDEADBEEF        # finite as fp32 (-6.3e18) and as each bf16 half: an output NaN can only come from the NaN input padding
B_64 = [1, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 255, 257, 300, 513]
B_128 = [1, 17, 65, 129, 257]
MAX_B = {64: max(B_64), 128: max(B_128)}
STORAGE = ["f32", "bf16"]
EMULATION = ["bf16x9", "bf16x6"]          # these run the fp32 latent kernels: one batch across the colsum switch is enough
OPS = ["fc_fwd", "decin_fwd", "decin_bwd", "fc_bwd"]
CASES = ([(64, B, m) for m in STORAGE for B in B_64] + [(128, B, m) for m in STORAGE for B in B_128] + [(64, 65, m) for m in EMULATION])
cases = pytest.mark.parametrize("W,B,mode", CASES, ids=[f"w{w}-b{b}-{m}" for w, b, m in CASES])
ops = pytest.mark.parametrize("op", OPS)
WORST = {}                   # (op output, mode) -> largest err / bound seen, printed per test (pytest -s) for LABNOTES


def bottleneck(W):
    return 256 * (W // 16) ** 2


@pytest.fixture(scope="module")
def handles():
    """One handle per (width, precision) for the whole module, max_batch = the largest batch the module runs at that width."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    made = {}

    def get(W, mode):
        if (W, mode) not in made:
            made[W, mode] = cvlib.Handle(W, MAX_B[W] if mode in STORAGE else 65, precision=mode)
        return made[W, mode]
    yield get
    made.clear()
    for (tag, mode), r in sorted(WORST.items()):          # pytest -s: the head-room table of LABNOTES.md
        print(f"worst err / bound  {tag:12s} {mode:7s} {r:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# buffers: PAD rows / floats of padding inside the same allocation, always
# ---------------------------------------------------------------------------------------------------------------------------------------
def _i32(pattern):
    return pattern - (1 << 32) if pattern >= 1 << 31 else pattern


def rows_in(t, bf16=False):
    """(B, cols) or (B,) host tensor -> device buffer with PAD more rows that hold NaN, in bf16 storage if asked."""
    t = t.reshape(t.shape[0], -1)
    full = torch.full((t.shape[0] + PAD, t.shape[1]), float("nan"), dtype=torch.bfloat16 if bf16 else torch.float32)
    full[:t.shape[0]] = t                 # bf16: the values are bf16-representable already
    return full.cuda()


def rows_out(B, cols, bf16=False):
    """Device buffer of B + PAD rows, every word the sentinel."""
    return poison(torch.empty((B + PAD, cols), dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda"), SENTINEL)


def flat_out(n):
    """A weight-shaped output of n floats with a sentinel tail of PAD floats."""
    return poison(torch.empty(n + PAD, device="cuda"), SENTINEL)


def scratch_for(H, B):
    """The op's scratch: NaN where the kernels work, a sentinel tail of one slab row block behind it."""
    n = H.op_latent_scratch_floats(B)
    s = torch.empty(n + PAD * 64, device="cuda")
    poison(s[:n], ALL_ONES)
    poison(s[n:], SENTINEL)
    return s, n


def arg(t):
    """The pointer argument of a buffer: bf16 storage travels as the packed fp32 view the binding expects."""
    return t if t.dtype == torch.float32 else t.reshape(-1).view(torch.float32)


def take(name, buf, n):
    """The first n rows (floats) of an output on the host, after the padding checks of (d)."""
    torch.cuda.synchronize()
    tail = buf[n:].reshape(-1)
    words = tail.view(torch.int32) if tail.dtype == torch.float32 else tail.view(torch.int16).view(torch.int32)
    bad = int((words != _i32(SENTINEL)).sum())
    assert bad == 0, f"{name}: {bad} words of the padding behind the output were overwritten (a store at a row >= B)"
    got = buf[:n].float().cpu()
    nan = int(torch.isnan(got).sum())
    assert nan == 0, f"{name}: {nan} NaN in the output: an input row >= B (NaN padding) was contracted, or scratch was read before it was written"
    return got


def check_scratch(name, s, n):
    torch.cuda.synchronize()
    bad = int((s[n:].view(torch.int32) != _i32(SENTINEL)).sum())
    assert bad == 0, f"{name}: {bad} words behind the scratch were overwritten"


# ---------------------------------------------------------------------------------------------------------------------------------------
# the four ops on host tensors (fp32 values; bf16 storage converts exactly)
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_fc_fwd(H, B, flat, wfc, bfc, eps, pred):
    bf = H.precision == "bf16"
    mu, logvar, zcat = rows_out(B, 32), rows_out(B, 32), rows_out(B, 33)
    s, n = scratch_for(H, B)
    H.op_fc_fwd(B, arg(rows_in(flat, bf)), wfc.cuda(), bfc.cuda(), rows_in(eps), rows_in(pred).reshape(-1), mu, logvar, zcat, s)
    check_scratch("fc_fwd", s, n)
    return {"mu": take("mu", mu, B), "logvar": take("logvar", logvar, B), "zcat": take("zcat", zcat, B)}


def run_decin_fwd(H, B, zcat, wd, bd):
    bf = H.precision == "bf16"
    h = rows_out(B, wd.shape[1], bf)
    H.op_decin_fwd(B, rows_in(zcat), wd.cuda(), bd.cuda(), arg(h))
    return {"h": take("h", h, B)}


def run_decin_bwd(H, B, zcat, dh, wd):
    bf = H.precision == "bf16"
    K = wd.shape[1]
    dwd, dbd, dzcat = flat_out(33 * K), flat_out(K), rows_out(B, 33)
    s, n = scratch_for(H, B)
    H.op_decin_bwd(B, rows_in(zcat), arg(rows_in(dh, bf)), wd.cuda(), dwd, dbd, dzcat, s)
    check_scratch("decin_bwd", s, n)
    return {"dwd": take("dwd", dwd, 33 * K).view(33, K), "dbd": take("dbd", dbd, K), "dzcat": take("dzcat", dzcat, B)}


def run_fc_bwd(H, B, flat, wfc, dzcat, eps, logvar, dmu, dlv):
    bf = H.precision == "bf16"
    K = wfc.shape[0]
    dwfc, dbfc, dflat = flat_out(K * 64), flat_out(64), rows_out(B, K, bf)
    s, n = scratch_for(H, B)
    H.op_fc_bwd(B, arg(rows_in(flat, bf)), wfc.cuda(), rows_in(dzcat), rows_in(eps), rows_in(logvar), rows_in(dmu), rows_in(dlv),
                dwfc, dbfc, arg(dflat), s)
    check_scratch("fc_bwd", s, n)
    return {"dwfc": take("dwfc", dwfc, K * 64).view(K, 64), "dbfc": take("dbfc", dbfc, 64), "dflat": take("dflat", dflat, B)}


RUN = {"fc_fwd": run_fc_fwd, "decin_fwd": run_decin_fwd, "decin_bwd": run_decin_bwd, "fc_bwd": run_fc_bwd}


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs (seeded generators on the host) and float64 references
# ---------------------------------------------------------------------------------------------------------------------------------------
def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def uni(g, shape, lo, hi):
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def to_bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


@functools.lru_cache(maxsize=None)
def weights(W):
    """fp32 weights in the native layouts, sized so that mu is O(1) and logvar = bias + O(0.3) with the biases spread over
    [-6.4, 6.4]: logvar stays inside [-8, 8] and reaches both tails of expf."""
    K, g = bottleneck(W), gen("weights", W)
    wfc = torch.cat((uni(g, (K, 32), -1, 1) * (3.2 / math.sqrt(K)), uni(g, (K, 32), -1, 1) * (0.9 / math.sqrt(K))), 1).contiguous()
    bfc = torch.cat((uni(g, (32,), -0.5, 0.5), torch.linspace(-6.4, 6.4, 32)))
    wd = uni(g, (33, K), -1, 1) / math.sqrt(33.0)
    bd = uni(g, (K,), -1, 1) / math.sqrt(33.0)
    return wfc, bfc, wd, bd


def parity_inputs(op, W, B, bf):
    """Host fp32 inputs of `op`, in call order.  bf: the tensors that live in bf16 storage are bf16-representable."""
    K, g = bottleneck(W), gen("parity", op, W, B)
    wfc, bfc, wd, bd = weights(W)
    act = (lambda t: to_bf16(t)) if bf else (lambda t: t)
    if op == "fc_fwd":
        return act(uni(g, (B, K), -1, 1)), wfc, bfc, torch.randn((B, 32), generator=g), uni(g, (B,), 0, 1)
    if op == "decin_fwd":
        return 1.5 * torch.randn((B, 33), generator=g), wd, bd
    if op == "decin_bwd":
        return 1.5 * torch.randn((B, 33), generator=g), act(torch.randn((B, K), generator=g)), wd
    flat, dz = act(uni(g, (B, K), -1, 1)), torch.randn((B, 33), generator=g)
    eps, lv = torch.randn((B, 32), generator=g), uni(g, (B, 32), -8, 8)
    if not bf:
        return flat, wfc, dz, eps, lv, 0.5 * torch.randn((B, 32), generator=g), 0.5 * torch.randn((B, 32), generator=g)
    # bf16 storage: dml is rounded to bf16 on its way to the MFMA.  Choose the loss gradients so that each dml is, up to fp32 round-off
    # of its terms, a bf16-representable target 1.5 .. 2.5 times its reparametrize term: fp32 and float64 round to the same bf16 value
    d, e, l = dz[:, :32].double(), eps.double(), lv.double()
    t1, t2 = d, d * e * 0.5 * torch.exp(0.5 * l)
    dmu = (to_bf16(t1 * uni(g, (B, 32), 1.5, 2.5).double()) - t1).float()
    dlv = (to_bf16(t2 * uni(g, (B, 32), 1.5, 2.5).double()) - t2).float()
    return flat, wfc, dz, eps, lv, dmu, dlv


def d64(*ts):
    return [t.double() for t in ts]


def dml_of(dz, eps, lv, dmu, dlv):
    """float64 dml (B, 64) and the sum of the absolute values of its terms."""
    dz, eps, lv, dmu, dlv = d64(dz[:, :32], eps, lv, dmu, dlv)
    t = dz * eps * 0.5 * torch.exp(0.5 * lv)
    return torch.cat((dz + dmu, t + dlv), 1), torch.cat((dz.abs() + dmu.abs(), t.abs() + dlv.abs()), 1)


def bounded(tag, mode, got, want, bound):
    r = within(tag, got, want, bound)
    WORST[tag, mode] = max(WORST.get((tag, mode), 0.0), r)
    print(f"{tag} [{mode}]: err / bound {r:.3f}")


def check_parity(op, mode, B, inputs, got):
    bf = mode == "bf16"
    out_round = BF16 if bf else 0.0
    if op == "fc_fwd":
        flat, wfc, bfc, eps, pred = d64(*inputs)
        K = wfc.shape[0]
        ml = flat @ wfc + bfc
        assert ml[:, 32:].abs().max() <= 8 and (B < 17 or (ml[:, 32:].min() < -6 and ml[:, 32:].max() > 6)), "logvar leaves [-8, 8] or misses a tail"
        mb = (fc_split_terms(K, bias=True) + 1) * U32 * (flat.abs() @ wfc.abs() + bfc.abs())        # n = K / FC_KS + FC_KS, c = 2
        bounded("mu", mode, got["mu"], ml[:, :32], mb[:, :32])
        bounded("logvar", mode, got["logvar"], ml[:, 32:], mb[:, 32:])
        mu_g, se = got["mu"].double(), eps * torch.exp(0.5 * got["logvar"].double())
        bounded("zcat", mode, got["zcat"][:, :32], mu_g + se, ZCAT_TERMS * U32 * (mu_g.abs() + se.abs()))
        assert len(set(inputs[4].tolist())) == B and same_bits(got["zcat"][:, 32], inputs[4]), "zcat: column 32 is not pred, bit for bit"
    elif op == "decin_fwd":
        zcat, wd, bd = d64(*inputs)
        want = zcat @ wd + bd
        hb = (DECIN_TERMS + 1) * U32 * (zcat.abs() @ wd.abs() + bd.abs())                           # n = 33, c = 2
        bounded("h", mode, got["h"], want, hb + out_round * want.abs())
    elif op == "decin_bwd":
        zcat, dh, wd = d64(*inputs)
        z1 = torch.cat((to_bf16(zcat) if bf else zcat, torch.ones(B, 1, dtype=torch.float64)), 1)   # the MFMA operand [zcat | 1]
        want, wb = z1.t() @ dh, (batch_terms(B) + 1) * U32 * (z1.abs().t() @ dh.abs())              # n = B + 4, c = 1
        bounded("dwd", mode, got["dwd"], want[:33], wb[:33])
        bounded("dbd", mode, got["dbd"], want[33], wb[33])
        K = wd.shape[1]
        bounded("dzcat", mode, got["dzcat"], dh @ wd.t(), fc_split_terms(K, bias=False) * U32 * (dh.abs() @ wd.abs().t()))   # c = 1
    else:
        flat, wfc = d64(*inputs[:2])
        dml, dml_abs = dml_of(*inputs[2:])
        want = dml @ wfc.t()
        bounded("dflat", mode, got["dflat"], want, (DFLAT_TERMS + 1) * U32 * (dml_abs @ wfc.abs().t()) + out_round * want.abs())
        bounded("dbfc", mode, got["dbfc"], dml.sum(0), (batch_terms(B) + DML_TERMS) * U32 * dml_abs.sum(0))
        opnd = to_bf16(dml) if bf else dml                                                          # the MFMA operand
        bounded("dwfc", mode, got["dwfc"], flat.t() @ opnd, (batch_terms(B) + DML_TERMS + 1) * U32 * (flat.abs().t() @ dml_abs))


@ops
@cases
def test_parity_against_fp64_with_nan_padding(handles, W, B, mode, op):
    """(a) and (d): every element of every output of the op inside its derived round-off bound, with NaN in the PAD input rows past B
    and the sentinel intact behind every output."""
    H = handles(W, mode)
    inputs = parity_inputs(op, W, B, mode == "bf16")
    check_parity(op, mode, B, inputs, RUN[op](H, B, *inputs))


# ---------------------------------------------------------------------------------------------------------------------------------------
# (b) exact integer cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def exact_inputs(op, W, B, bf):
    K, g = bottleneck(W), gen("exact", op, W, B)
    if op == "fc_fwd":        # flat >= 0 and the fc_var half <= 0: logvar <= 0, exp(logvar / 2) in [0, 1], eps = 0 -> z = mu exactly
        wfc = torch.cat((ints(g, (K, 32), -4, 4), ints(g, (K, 32), -4, 0)), 1).contiguous()
        bfc = torch.cat((ints(g, (32,), -4, 4), ints(g, (32,), -4, 0)))
        return ints(g, (B, K), 0, 4), wfc, bfc, torch.zeros(B, 32), ints(g, (B,), 0, 4)
    if op == "decin_fwd":     # |h| <= 33 a^2 + a: 532 in fp32 storage (a = 4), 134 in bf16 storage (a = 2)
        a = 2 if bf else 4
        return ints(g, (B, 33), -a, a), ints(g, (33, K), -a, a), ints(g, (K,), -a, a)
    if op == "decin_bwd":     # all outputs fp32: |dWd| <= 16 B, |d_zcat| <= 16 K
        return ints(g, (B, 33), -4, 4), ints(g, (B, K), -4, 4), ints(g, (33, K), -4, 4)
    # fc_bwd: eps = 0, logvar = 0 -> dml = [dz + d_mu | d_logvar].  bf16 storage: |dflat| <= 32 * 2 * 1 + 32 * 2 * 1 = 128
    a, w = (1, 1) if bf else (2, 4)
    return (ints(g, (B, K), -4, 4), ints(g, (K, 64), -w, w), ints(g, (B, 33), -a, a), torch.zeros(B, 32), torch.zeros(B, 32),
            ints(g, (B, 32), -a, a), ints(g, (B, 32), -2 * a, 2 * a))


def exact(name, got, want):
    """want: float64 holding integers below 2^24 (exact there), compared as int64."""
    assert want.abs().max() < 2 ** 24 and torch.equal(want, want.round())
    want = want.to(torch.int64)
    if not torch.equal(got.double(), want.double()):
        d = (got.double() != want.double())
        i = int(d.flatten().nonzero()[0])
        raise AssertionError(f"{name}: {int(d.sum())} of {d.numel()} elements are not the integer result, first at flat index {i}: "
                             f"{got.flatten()[i].item()!r} vs {want.flatten()[i].item()}")


def check_exact(op, B, inputs, got):
    if op == "fc_fwd":
        flat, wfc, bfc, eps, pred = d64(*inputs)
        ml = flat @ wfc + bfc
        exact("mu", got["mu"], ml[:, :32])
        exact("logvar", got["logvar"], ml[:, 32:])
        exact("zcat", got["zcat"], torch.cat((ml[:, :32], pred[:, None]), 1))
    elif op == "decin_fwd":
        zcat, wd, bd = d64(*inputs)
        exact("h", got["h"], zcat @ wd + bd)
    elif op == "decin_bwd":
        zcat, dh, wd = d64(*inputs)
        exact("dwd", got["dwd"], zcat.t() @ dh)
        exact("dbd", got["dbd"], dh.sum(0))
        exact("dzcat", got["dzcat"], dh @ wd.t())
    else:
        flat, wfc = d64(*inputs[:2])
        dml, _ = dml_of(*inputs[2:])
        exact("dwfc", got["dwfc"], flat.t() @ dml)
        exact("dbfc", got["dbfc"], dml.sum(0))
        exact("dflat", got["dflat"], dml @ wfc.t())


@ops
@cases
def test_exact_on_small_integers(handles, W, B, mode, op):
    """(b): integer operands give the integer result in any summation order: every image and every k counted exactly once."""
    H = handles(W, mode)
    inputs = exact_inputs(op, W, B, mode == "bf16")
    check_exact(op, B, inputs, RUN[op](H, B, *inputs))


# ---------------------------------------------------------------------------------------------------------------------------------------
# (c) one lit image
# ---------------------------------------------------------------------------------------------------------------------------------------
LIT_B = 300
LIT_ROWS = sorted({b for b in (0, 15, 16, 63, 64, 127, 128, 255, 256, LIT_B - 1) if 0 <= b < LIT_B})


def dyadic(g, shape):
    """Non-zero multiples of 1/64 in [-2, 2]: bf16-representable, and the product of two of them is exact in fp32."""
    v = torch.randint(1, 129, shape, generator=g).float() / 64.0
    return v * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


@pytest.mark.parametrize("mode", STORAGE)
@pytest.mark.parametrize("op", ["decin_bwd", "fc_bwd"])
def test_one_lit_image_is_counted_once_wherever_it_sits(handles, mode, op):
    """(c): B = 300, all images zero but b*: dWd / dbd (decin_bwd), dWfc / dbfc (fc_bwd) equal the one outer product exactly, and the
    per-image outputs of every other image are zero."""
    W, B = 64, LIT_B
    H, K = handles(W, mode), bottleneck(W)
    wfc, _, wd, _ = weights(W)
    for bs in LIT_ROWS:
        g = gen("lit", op, bs)
        lit = torch.zeros(B, 1)
        lit[bs] = 1.0
        others = torch.arange(B) != bs
        try:
            if op == "decin_bwd":
                zcat, dh = dyadic(g, (B, 33)) * lit, dyadic(g, (B, K)) * lit
                got = run_decin_bwd(H, B, zcat, dh, wd)
                assert torch.equal(got["dwd"].double(), torch.outer(zcat[bs].double(), dh[bs].double())), "dWd is not zcat[b*] x dh[b*]"
                assert torch.equal(got["dbd"], dh[bs]), "dbd is not dh[b*]"
                assert not got["dzcat"][others].any(), "d_zcat of a zero image is not zero"
            else:             # eps = 0, logvar = 0, d_mu = 0: dml[b*] = [dz[b*] | d_logvar[b*]]
                flat, dz, dlv = dyadic(g, (B, K)) * lit, dyadic(g, (B, 33)) * lit, dyadic(g, (B, 32)) * lit
                zero = torch.zeros(B, 32)
                got = run_fc_bwd(H, B, flat, wfc, dz, zero, zero, zero, dlv)
                dml = torch.cat((dz[bs, :32], dlv[bs]))
                assert torch.equal(got["dwfc"].double(), torch.outer(flat[bs].double(), dml.double())), "dWfc is not flat[b*] x dml[b*]"
                assert torch.equal(got["dbfc"], dml), "dbfc is not dml[b*]"
                assert not got["dflat"][others].any(), "dflat of a zero image is not zero"
        except AssertionError as e:
            raise AssertionError(f"{op} [{mode}], B = {B}, lit image b* = {bs}: {e}") from e


# ---------------------------------------------------------------------------------------------------------------------------------------
# (e) determinism
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", STORAGE)
@ops
def test_same_call_twice_is_bit_identical(handles, mode, op):
    """(e): a ragged batch past the second bgemm_tr tile, fresh buffers (and fresh NaN scratch) for each call."""
    W, B = 64, 300
    H = handles(W, mode)
    inputs = parity_inputs(op, W, B, mode == "bf16")
    first, second = RUN[op](H, B, *inputs), RUN[op](H, B, *inputs)
    for k in first:
        assert same_bits(first[k], second[k]), f"{op} [{mode}]: {k} differs between two identical calls"


# ---------------------------------------------------------------------------------------------------------------------------------------
# (f) the KL term through cvae_loss
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 17, 65, 300])
def test_kl_term_of_the_loss(handles, B):
    """(f): KLD = kw * mean_b(-0.5 * sum_d(1 + logvar - mu^2 - exp(logvar))), kw = 0.001 (vae_nets.py:57-60), and its gradients
    d_mu = kw mu / B, d_logvar = kw (exp(logvar) - 1) / (2 B), from caller-supplied mu ~ N(0, 1) and logvar in [-8, 8].
    The scalar to 2e-5 (test_msssim's bar); the gradients to 4 * 2^-24 |want| (the constant, two products and 1 / B), d_logvar plus one
    ulp of expf(logvar) times kw / B (exp - 1 cancels near logvar = 0).  scalars[0] is the fp32 sum scalars[1] + scalars[2]."""
    H, W, kw = handles(64, "f32"), 64, 0.001
    g = gen("kl", B)
    mu, lv = torch.randn((B, 32), generator=g), uni(g, (B, 32), -8, 8)
    x = torch.rand((B, 3, W, W), generator=g)
    recon = 0.7 * x + 0.3 * torch.rand((B, 3, W, W), generator=g)
    ws = torch.empty(H.workspace_bytes(B) // 4, device="cuda")
    scal = poison(torch.empty(16, device="cuda"), SENTINEL)
    d_recon = torch.empty(B * 3 * W * W, device="cuda")
    d_mu, d_lv = rows_out(B, 32), rows_out(B, 32)
    H.loss(B, x.cuda(), rows_in(mu), rows_in(lv), recon.cuda(), ws, scal, d_recon, d_mu, d_lv)
    d_mu, d_lv = take("d_mu", d_mu, B), take("d_logvar", d_lv, B)
    s = scal.cpu()
    m64, l64 = mu.double(), lv.double()
    kld = kw * (-0.5 * (1 + l64 - m64 ** 2 - l64.exp()).sum(1)).mean()
    print(f"B={B}: KLD {s[2].item():.7f} vs {kld.item():.7f}")
    assert abs(s[2].item() - kld.item()) <= 2e-5, f"KLD {s[2].item()!r} vs {kld.item()!r}"
    assert torch.isfinite(s[:3]).all() and (s[0] - (s[1] + s[2])).abs().item() < 1e-7, s[:3]
    want_mu, want_lv = kw * m64 / B, kw * 0.5 * (l64.exp() - 1) / B
    exp_ulp = 2.0 ** (torch.floor(torch.log2(l64.exp().float().double())) - 23)          # the spacing of fp32 at expf(logvar)
    bounded("kl d_mu", "f32", d_mu, want_mu, 4 * U32 * want_mu.abs())
    bounded("kl d_logvar", "f32", d_lv, want_lv, 4 * U32 * want_lv.abs() + exp_ulp * kw / B)
