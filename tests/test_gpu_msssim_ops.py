"""The loss kernels op by op: the MS-SSIM pyramid (msssim.hip), its scalar end (msssim_finish.h), the KLD of the finalize and the per-image
scores (score.hip), at every plane-group and grid edge.

msssim_plane_kernel<S> is persistent over groups of PPW planes (1 at S = 64 and 32, 4 at 16, 16 at 8, 64 at 4) on a grid of one
residency of the chip; msssim_stream_kernel walks the 128-wide level on one workgroup per compute unit.  The cases (ws_tools.MS_CASES)
sit on both sides of the batch at which a workgroup of each level first walks a second group, plus the configs' batches (2048 / 1024:
four levels loop, the deepest of them unevenly) and the ragged batches ws_tools.MS_RAGGED; the batches are derived from the launcher's
rules and this device's compute-unit count (ws_tools.ms_case_batch), and every test asserts first that its batch is on its edge.

Inputs of the large batches are replicas: image i is base pair i % 5 (ws_tools.ms_base_pairs), built on the device by indexing.  The
reference is the oracle's MS-SSIM restated in float64 on the five pairs with their counts (ws_tools.ms_replica_ref;
tests/test_host_msssim_tools.py shows it equal to the oracle on an expanded batch).  Per case:
(a) parity, the project's bars: levels and loss 2e-5, every element of d_recon of the first occurrence of each base image 1e-4 of the
    largest reference gradient, score rows to the bars of test_gpu_score.test_rows_match_the_oracle_per_image.
(b) position independence, exact: every replica's d_recon and score row is bit for bit the first occurrence's.
(c) every plane summed exactly once: the record sums of cvae_score at batch B equal sum_k n_k s_k to 1e-12 relative, s_k the sums of
    base image k scored alone, and the ten level scalars of the gradient-mode call are within one fp32 ulp of
    float32(sum_k n_k s_k,l / (3 B S_l^2)).  The host test shows that one misplaced plane moves a level mean by 11 ulps or more.
(d) hygiene on every call: two NaN images behind x and recon (NaN rows behind mu and logvar) in the same allocation, a sentinel behind
    d_recon, the rows, the scalars, the record and the MS-SSIM workspace, the workspace itself ALL_ONES on entry; no NaN comes out, no
    sentinel is touched, the same call twice gives the same bits.
(e) score pooling past 256 rows (B = 257, 683): images, finite, the four row sums and worst of the record against the returned rows;
    a flipped image at an index >= 256 is NaN in its own row only and counted in images, not in finite.
(f) the KLD and its gradients through cvae_loss at B = 1, 255, 256, 257, 683 (the finalize's loop strides from B = 257 on), against
    float64 within bounds derived from the kernel's fp32 arithmetic (U = 2^-24, ws_tools.kld_ref):
      d_mu      kw * m * (1.0f / (float)B): the reciprocal and two products, 3 U |d_mu|
      d_logvar  kw * 0.5f * (e - 1.0f) * (1.0f / (float)B), e = expf(lv) to EXPF_ULPS = 3 ulps (the OpenCL bound the device library is
                built to; an ulp is at most 2 U e): expf's error enters e - 1 in full, which matters near lv = 0 where e - 1 cancels:
                kw / (2 B) 6 U e + 4 U |d_logvar| (the difference, the reciprocal, two products; kw * 0.5f is exact)
      KLD       (float)(-0.5 k / B) * kw, k the fp64 sum of the fp32 terms 1.0f + lv - m * m - e: per term
                U (|1 + lv| + m^2 + |1 + lv - m^2| + |t|) + 6 U e, 2^-45 sum |t| for the fp64 additions, 2 U |KLD| for the cast and the
                product.  About 1e-8 of a KLD of 7e-3; leaving out one image's 32 terms moves it by 6e-6 or more (host test).
(g) NaN and negative levels at 128 wide, B = 3 (ws_tools.ms_inputs "neg", "nan" and "unused"): levels to 2e-5, the oracle's NaN / finite
    pattern in loss and gradient, and through cvae_loss_obj a finite used-terms gradient where only unused levels are negative.

Peak device memory: 15 GiB, at 128 wide: the handle's workspace for B = 1366 (13.2 GiB, torch.empty; cvae_score and cvae_loss address
their MS-SSIM region through it and touch 0.5 GiB of it), the batch with its padding and the outputs of two calls (0.27 GiB each).
5461 / 5462 run through cvae_op_msssim alone, on a workspace of op_msssim_ws_floats (0.5 GiB).

The measured head-room of every check is in LABNOTES.md."""
import functools

import numpy as np
import pytest
import torch

from critic_vae_amd import lib as cvlib
from oracle import cvae_oracle as orc
from ws_tools import (ALL_ONES, MS_BASES, MS_CASES, MS_RAGGED, bits, kld_case, kld_ref, ms_assert_edge, ms_base_pairs, ms_case_batch,
                      ms_counts, ms_inputs, ms_level_facts, ms_replica_ref, poison, same_bits, within)

pytestmark = pytest.mark.gpu

PAD = 2                      # NaN images (rows) behind every batch-indexed input
TAIL = 256                   # floats behind every output and the op's workspace
SENTINEL = 0xDEADBEEF        # a finite fp32 no kernel writes by chance
COLS = 8                     # CVAE_SCORE_COLS
STATE = 24                   # CVAE_SCORE_STATE_DOUBLES
DEV = "cuda"
OP_ONLY = {(64, 4)}          # (width, level): batches that run through cvae_op_msssim alone (no full step workspace at B = 5462)
CASES = list(MS_CASES)
cases = pytest.mark.parametrize("W,level,edge", CASES, ids=[f"w{w}-l{l}-{e}" for w, l, e in CASES])
MS_W = torch.tensor(orc.MS_WEIGHTS, dtype=torch.float32)
WORST = {}                   # (check, width) -> largest err / bar seen, printed per module (pytest -s) for LABNOTES


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _i32(pattern):
    return pattern - (1 << 32) if pattern >= 1 << 31 else pattern


def note(tag, W, r):
    WORST[tag, W] = max(WORST.get((tag, W), 0.0), float(r))


# ---------------------------------------------------------------------------------------------------------------------------------------
# one handle, one step workspace and the five base pairs per width
# ---------------------------------------------------------------------------------------------------------------------------------------
class Rig:
    def __init__(self, W):
        self.W = W
        tops = [ms_case_batch(w, l, e, cus()) for w, l, e in CASES if w == W]
        step = [ms_case_batch(w, l, e, cus()) for w, l, e in CASES if w == W and (w, l) not in OP_ONLY]
        self.H = cvlib.Handle(W, max(tops))
        self.step_top = max(step + [683])
        self.ws = torch.empty(self.H.workspace_bytes(self.step_top) // 4, device=DEV)
        self.base = [t.to(DEV).contiguous() for t in ms_base_pairs(W)]             # x, mu, logvar, recon: the only host copies
        self._sums = None

    def ms_region(self, B):
        """The MS-SSIM region of the step workspace at batch B and the TAIL floats behind it."""
        off, n = self.H.lib.cvae_ws_offset(self.H.h, B, b"ms"), self.H.op_msssim_ws_floats(B)
        assert off >= 0 and off + n + TAIL <= self.ws.numel() and B <= self.step_top
        return self.ws[off:off + n], self.ws[off + n:off + n + TAIL]

    def base_sums(self):
        """(c): s_k, the 11 fp64 sums of base image k scored alone on a fresh record, (5, 11) float64."""
        if self._sums is None:
            x, mu, lv, recon = self.base
            out = []
            for k in range(MS_BASES):
                r = run_score(self, 1, replicas(x[k:k + 1], 1), replicas(mu[k:k + 1], 1), replicas(lv[k:k + 1], 1), replicas(recon[k:k + 1], 1))
                out.append(r["state"][:11].cpu().numpy())
            self._sums = np.stack(out)
        return self._sums


@pytest.fixture(scope="module")
def rigs():
    """One Rig at a time: the step workspace of the other width is released first."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    held = {}

    def get(W):
        if W not in held:
            held.clear()
            torch.cuda.empty_cache()
            held[W] = Rig(W)
        return held[W]
    yield get
    held.clear()
    torch.cuda.empty_cache()
    for (tag, W), r in sorted(WORST.items()):
        print(f"worst err / bar  {tag:28s} w{W:<4d} {r:.4f}")


@functools.lru_cache(maxsize=None)
def replica_ref(W, B):
    x, _, _, recon = ms_base_pairs(W)
    return ms_replica_ref(recon, x, ms_counts(B))


@functools.lru_cache(maxsize=None)
def base_rows(W):
    """Per base image alone, float64: MS-SSIM loss, weighted KLD, mse, max |recon - x|, ssim levels 0 and 4."""
    x, mu, lv, recon = ms_base_pairs(W)
    out = np.zeros((MS_BASES, 6))
    for k in range(MS_BASES):
        r = ms_replica_ref(recon[k:k + 1], x[k:k + 1])
        d = recon[k].double() - x[k].double()
        out[k] = (r["loss"].item(), kld_ref(mu[k:k + 1], lv[k:k + 1])["kld"].item(), (d ** 2).mean().item(), d.abs().max().item(),
                  r["ssim"][0].item(), r["ssim"][4].item())
    return out


def replicas(base, B):
    """(B + PAD, ...): image i = base[i % len(base)], NaN behind, built on the device."""
    out = torch.full((B + PAD,) + tuple(base.shape[1:]), float("nan"), device=DEV)
    out[:B] = base[torch.arange(B, device=DEV) % base.shape[0]]
    return out


def sentinel(n):
    return poison(torch.empty(n, device=DEV), SENTINEL)


def intact(name, t):
    bad = int((t.contiguous().reshape(-1).view(torch.int32) != _i32(SENTINEL)).sum())
    assert bad == 0, f"{name}: {bad} words behind the output were overwritten"


def clean(name, t):
    nan = int(torch.isnan(t).sum())
    assert nan == 0, f"{name}: {nan} NaN: the NaN padding or workspace that was never written has been read"
    return t


def twice(call):
    """(d): the call twice on fresh buffers, bit for bit the same.  Returns the first."""
    first, second = call(), call()
    for k in first:
        assert same_bits(first[k], second[k]), f"{k} differs between two identical calls"
    return first


# ---------------------------------------------------------------------------------------------------------------------------------------
# the calls, each with (d)
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_msssim(H, W, B, rb, xb, nan_ok=False):
    """cvae_op_msssim in gradient mode on a workspace of its own.  rb, xb: (B + PAD, 3, W, W).  Returns scalars (16,), d_recon (B, 3, W, W)."""
    n, per = H.op_msssim_ws_floats(B), 3 * W * W

    def call():
        ws = torch.empty(n + TAIL, device=DEV)
        poison(ws[:n], ALL_ONES)
        poison(ws[n:], SENTINEL)
        scal, d = sentinel(16 + TAIL), sentinel((B + PAD) * per)
        H.op_msssim(B, rb, xb, ws, scal, d)
        torch.cuda.synchronize()
        intact("msssim workspace", ws[n:]), intact("scalars", scal[16:]), intact("d_recon", d[B * per:])
        out = {"scalars": scal[:16], "d_recon": d[:B * per].view(B, 3, W, W)}
        if not nan_ok:
            clean("scalars", out["scalars"]), clean("d_recon", out["d_recon"])
        return out
    return twice(call)


def run_score(rig, B, xb, mub, lvb, rb, nan_rows=()):
    """cvae_score, rows and record, through the step workspace.  Returns rows (B, 8) and the record (24 doubles)."""
    H = rig.H

    def call():
        region, behind = rig.ms_region(B)
        poison(region, ALL_ONES)
        poison(behind, SENTINEL)
        rows = sentinel((B + PAD) * COLS)
        state = poison(torch.empty(STATE + 8, dtype=torch.float64, device=DEV), SENTINEL)
        H.score_init(state)
        H.score(B, xb, mub, lvb, rb, rig.ws, rows, state)
        torch.cuda.synchronize()
        intact("workspace behind the MS-SSIM region", behind), intact("rows", rows[B * COLS:]), intact("record", state[STATE:])
        out = {"rows": rows[:B * COLS].view(B, COLS), "state": state[:STATE]}
        keep = [i for i in range(B) if i not in nan_rows] if nan_rows else slice(None)
        clean("rows", out["rows"][keep]), clean("record", out["state"][:18])
        return out
    return twice(call)


def run_loss(rig, B, xb, mub, lvb, rb, obj=None, nan_ok=False):
    """cvae_loss (obj None) or cvae_loss_obj with every gradient, through the step workspace."""
    H, W = rig.H, rig.W
    per = 3 * W * W

    def call():
        region, behind = rig.ms_region(B)
        poison(region, ALL_ONES)
        poison(behind, SENTINEL)
        scal, d = sentinel(16 + TAIL), sentinel((B + PAD) * per)
        d_mu, d_lv = sentinel((B + PAD) * 32), sentinel((B + PAD) * 32)
        if obj is None:
            H.loss(B, xb, mub, lvb, rb, rig.ws, scal, d, d_mu, d_lv)
        else:
            H.loss_obj(B, xb, mub, lvb, rb, rig.ws, obj, scal, d, d_mu, d_lv)
        torch.cuda.synchronize()
        intact("workspace behind the MS-SSIM region", behind), intact("scalars", scal[16:]), intact("d_recon", d[B * per:])
        intact("d_mu", d_mu[B * 32:]), intact("d_logvar", d_lv[B * 32:])
        out = {"scalars": scal[:16], "d_recon": d[:B * per].view(B, 3, W, W), "d_mu": d_mu[:B * 32].view(B, 32), "d_logvar": d_lv[:B * 32].view(B, 32)}
        clean("d_mu", out["d_mu"]), clean("d_logvar", out["d_logvar"])
        if not nan_ok:
            clean("scalars", out["scalars"]), clean("d_recon", out["d_recon"])
        return out
    return twice(call)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_levels(W, scal, ref, tag="levels"):
    """(a): the ten level means and the loss to 2e-5; no KLD in the op."""
    s = scal.cpu().double()
    want = torch.cat((ref["ssim"], ref["cs"]))
    note(tag, W, within(f"{tag}: ssim / cs level means", s[3:13], want, torch.full((10,), 2e-5)))
    note("loss", W, within("msssim loss", s[1:2], ref["loss"].reshape(1), torch.full((1,), 2e-5)))


def check_first_occurrences(W, B, d_recon, ref):
    """(a): every element of d_recon of the first occurrence of each base image against the reference gradient of one occurrence."""
    n = min(B, MS_BASES)
    want = ref["grad"][:n]
    got = d_recon[:n].cpu().double()
    note("d_recon", W, within("d_recon, first occurrences", got, want, torch.full_like(want, 1e-4 * want.abs().max().item())))


def check_replicas_identical(what, t, B):
    """(b): row i of t (B, ...) is bit for bit row i % 5, compared on the device."""
    v = bits(t).view(B, -1)
    same = (v == v[torch.arange(B, device=v.device) % MS_BASES]).all(dim=1)
    bad = (~same).nonzero().flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {B} replicas differ from the first occurrence of their base image, first at "
                              f"image {int(bad[0])} (base {int(bad[0]) % MS_BASES}); planes {3 * int(bad[0])}..{3 * int(bad[0]) + 2}")


def check_sums(rig, B, scal, state=None):
    """(c): the record's 11 sums against sum_k n_k s_k to 1e-12 relative; the gradient-mode level scalars within one fp32 ulp of
    float32(sum_k n_k s_k,l / (3 B S_l^2))."""
    W = rig.W
    want = (ms_counts(B).numpy()[:, None] * rig.base_sums()).sum(0)
    if state is not None:
        got = state[:11].cpu().numpy()
        rel = np.abs(got - want) / np.abs(want)
        note("record sums / 1e-12", W, rel.max() / 1e-12)
        assert rel.max() <= 1e-12, f"record sums: {got} against sum n_k s_k {want}: relative {rel}"
        means = (got[:10] / np.array([3.0 * B * (W >> (q % 5)) ** 2 for q in range(10)])).astype(np.float32)      # the same partials, the same finalize
        assert same_bits(torch.from_numpy(means), scal[3:13].cpu()), f"the record's level means {means} are not the gradient-mode call's {scal[3:13]}"
    cnt = np.array([3.0 * B * (W >> (q % 5)) ** 2 for q in range(10)])
    want32 = (want[:10] / cnt).astype(np.float32)
    got32 = scal[3:13].cpu().numpy()
    ulps = np.abs(got32.view(np.int32).astype(np.int64) - want32.view(np.int32).astype(np.int64))
    note("level scalars, ulps", W, ulps.max())
    assert ulps.max() <= 1, f"level scalars {got32} against float32(sum n_k s_k / count) {want32}: {ulps} ulps"


def check_rows(W, B, rows):
    """(a): the rows of the first occurrences to the bars of test_gpu_score.test_rows_match_the_oracle_per_image."""
    got, want = rows[:min(B, MS_BASES)].cpu().numpy().astype(np.float64), base_rows(W)
    for i in range(got.shape[0]):
        note("row msssim / 1e-4", W, abs(got[i, 1] - want[i, 0]) / 1e-4)
        note("row kld / 1e-4", W, abs(got[i, 2] - want[i, 1]) / 1e-4)
        note("row mse / 1e-6", W, abs(got[i, 3] - want[i, 2]) / (1e-6 * want[i, 2]))
        assert abs(got[i, 1] - want[i, 0]) <= 1e-4 and abs(got[i, 2] - want[i, 1]) <= 1e-4, (i, got[i], want[i])
        assert abs(got[i, 3] - want[i, 2]) <= 1e-6 * want[i, 2], (i, got[i, 3], want[i, 2])
        assert np.float32(got[i, 4]) == np.float32(want[i, 3]), (i, got[i, 4], want[i, 3])
        assert np.float32(got[i, 0]) == np.float32(got[i, 1]) + np.float32(got[i, 2]) and got[i, 7] == 0
    assert np.abs(got[:, 5:7] - want[:got.shape[0], 4:6]).max() <= 1e-4


def describe(f):
    return "; ".join(f"S {x['S']}: {x['groups']} groups / grid {x['grid']} / trips {x['min_trips']}..{x['trips']}" for x in f)


# ---------------------------------------------------------------------------------------------------------------------------------------
# residency edges: (a) - (d)
# ---------------------------------------------------------------------------------------------------------------------------------------
@cases
def test_replica_batch_at_residency_edge(rigs, W, level, edge):
    B = ms_case_batch(W, level, edge, cus())
    f = ms_assert_edge(W, level, edge, B, cus())
    print(f"w{W} level {level} {edge}: B {B}: {describe(f)}")
    rig = rigs(W)
    x, mu, lv, recon = rig.base
    xb, rb = replicas(x, B), replicas(recon, B)
    ref = replica_ref(W, B)
    g = run_msssim(rig.H, W, B, rb, xb)
    check_levels(W, g["scalars"], ref)
    assert g["scalars"][2].item() == 0.0
    check_first_occurrences(W, B, g["d_recon"], ref)
    check_replicas_identical("d_recon", g["d_recon"], B)
    if (W, level) in OP_ONLY:
        check_sums(rig, B, g["scalars"])
        return
    s = run_score(rig, B, xb, replicas(mu, B), replicas(lv, B), rb)
    check_rows(W, B, s["rows"])
    check_replicas_identical("score rows", s["rows"], B)
    check_sums(rig, B, g["scalars"], s["state"])
    rec = s["state"].cpu().numpy()
    assert rec[11] == B and rec[12] == B


# ---------------------------------------------------------------------------------------------------------------------------------------
# ragged groups: distinct images, float64 on the whole batch
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def distinct_case(W):
    """max(MS_RAGGED) distinct pairs, the way test_gpu_objective.smooth_case builds them, with a latent: CPU tensors, never modified."""
    n = max(MS_RAGGED)
    g = torch.Generator().manual_seed(4000 + W)
    x = torch.rand(n, 3, W, W, generator=g)
    recon = (0.7 * x + 0.3 * torch.rand(n, 3, W, W, generator=g)).contiguous()
    return x, torch.randn(n, 32, generator=g) * 0.5, torch.randn(n, 32, generator=g) * 0.3, recon


def padded(t):
    out = torch.full((t.shape[0] + PAD,) + tuple(t.shape[1:]), float("nan"), device=DEV)
    out[:t.shape[0]] = t.to(DEV)
    return out


@pytest.mark.parametrize("B", MS_RAGGED)
@pytest.mark.parametrize("W", [64, 128])
def test_ragged_plane_groups(rigs, W, B):
    """P = 3 B planes in groups of 4, 16 and 64: the absent planes of the last group do the last plane's work and store nothing."""
    f = ms_level_facts(W, B, cus())
    assert all(x["trips"] == 1 for x in f) and [x["last_group"] for x in f[-3:]] == [(3 * B - 1) % g + 1 for g in ((4, 16, 64) if W == 64 else (1, 4, 16))]
    rig = rigs(W)
    x, mu, lv, recon = (t[:B] for t in distinct_case(W))
    ref = ms_replica_ref(recon, x)
    xb, rb = padded(x), padded(recon)
    g = run_msssim(rig.H, W, B, rb, xb)
    check_levels(W, g["scalars"], ref, "levels (ragged)")
    want = ref["grad"]
    note("d_recon (ragged)", W, within("d_recon", g["d_recon"].cpu().double(), want, torch.full_like(want, 1e-4 * want.abs().max().item())))
    s = run_score(rig, B, xb, padded(mu), padded(lv), rb)
    # per plane partials: image i's rows come from its own three planes wherever they sit in their groups
    rows = s["rows"].cpu().numpy().astype(np.float64)
    w = MS_W.double()
    per_image = 1 - torch.prod(ref["plane_cs"].mean(1)[:, :4] ** w[:4], dim=1) * ref["plane_ssim"].mean(1)[:, 4] ** (4 * w[4])
    err = np.abs(rows[:, 1] - per_image.numpy())
    note("row msssim / 1e-4 (ragged)", W, err.max() / 1e-4)
    assert err.max() <= 1e-4, err
    assert np.abs(rows[:, 5] - ref["plane_ssim"].mean(1)[:, 0].numpy()).max() <= 1e-4
    assert np.abs(rows[:, 6] - ref["plane_ssim"].mean(1)[:, 4].numpy()).max() <= 1e-4
    # the record's level sums are the batch's: the means of the gradient-mode call, from the same partials
    rec = s["state"].cpu().numpy()
    cnt = np.array([3.0 * B * (W >> (q % 5)) ** 2 for q in range(10)])
    means = (rec[:10] / cnt).astype(np.float32)
    assert same_bits(torch.from_numpy(means), g["scalars"][3:13].cpu()), (means, g["scalars"][3:13])
    assert rec[11] == B and rec[12] == B


# ---------------------------------------------------------------------------------------------------------------------------------------
# (e) score pooling past 256 rows
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [257, 683])
@pytest.mark.parametrize("W", [64, 128])
def test_score_pooling_past_256_rows(rigs, W, B):
    rig = rigs(W)
    x, mu, lv, recon = rig.base
    xb, mub, lvb, rb = replicas(x, B), replicas(mu, B), replicas(lv, B), replicas(recon, B)

    def pooled(out, finite):
        rec = out["state"].cpu().numpy()
        rows = out["rows"].cpu().numpy().astype(np.float64)[finite]
        assert rec[11] == B and rec[12] == len(finite), (rec[11], rec[12])
        for c in range(4):
            want = rows[:, c].sum()
            note("pooled row sums / 1e-12", W, abs(rec[13 + c] - want) / (1e-12 * abs(want)))
            assert abs(rec[13 + c] - want) <= 1e-12 * abs(want), (c, rec[13 + c], want)
        assert rec[17] == rows[:, 0].max()

    whole = run_score(rig, B, xb, mub, lvb, rb)
    pooled(whole, list(range(B)))
    j = 256 + (B - 257) // 2
    assert 256 <= j < B
    rb[j] = 1 - xb[j]
    out = run_score(rig, B, xb, mub, lvb, rb, nan_rows=(j,))
    keep = [i for i in range(B) if i != j]
    r = out["rows"][j].cpu().numpy()
    assert np.isnan(r[0]) and np.isnan(r[1]) and np.isfinite(r[2:5]).all(), r
    assert same_bits(out["rows"][keep], whole["rows"][keep]), "a row of another image changed with the flipped one"
    pooled(out, keep)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (f) KLD and its gradients through cvae_loss
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 255, 256, 257, 683])
def test_kld_and_its_gradients_within_roundoff(rigs, B):
    """Bounds: the module docstring, (f).  B * 32 passes the finalize's 8192 threads from B = 257 on."""
    W = 64
    rig = rigs(W)
    assert (B * 32 > 32 * 256) == (B >= 257)
    x, _, _, recon = rig.base
    mu, lv = kld_case(B)
    r = kld_ref(mu, lv)
    assert 0.5 * 0.001 * r["terms"].abs().min().item() / B > 4 * r["kld_bound"].item(), "one dropped image would pass the KLD bound"
    out = run_loss(rig, B, replicas(x, B), padded(mu), padded(lv), replicas(recon, B))
    s = out["scalars"].cpu().double()
    note("KLD", W, within("KLD", s[2:3], r["kld"].reshape(1), r["kld_bound"].reshape(1)))
    note("d_mu", W, within("d_mu", out["d_mu"].cpu(), r["d_mu"], r["d_mu_bound"]))
    note("d_logvar", W, within("d_logvar", out["d_logvar"].cpu(), r["d_logvar"], r["d_logvar_bound"]))
    print(f"B {B}: KLD {s[2].item():.9e} (float64 {r['kld'].item():.9e}, bound {r['kld_bound'].item():.2e}); err / bound: KLD "
          f"{WORST['KLD', W]:.3f} d_mu {WORST['d_mu', W]:.3f} d_logvar {WORST['d_logvar', W]:.3f}")
    # the rest of the call: the MS-SSIM term of the replica batch and total = recon + KLD in fp32
    ref = replica_ref(W, B)
    check_levels(W, out["scalars"], ref, "levels (cvae_loss)")
    assert abs(s[0].item() - (s[1].item() + s[2].item())) <= 2 * 2.0 ** -24 * abs(s[0].item())
    check_first_occurrences(W, B, out["d_recon"], ref)
    check_replicas_identical("d_recon", out["d_recon"], B)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (g) NaN and negative levels at 128 wide
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signed_case(tag):
    """The oracle (fp32, CPU) on the pair: loss, levels, autograd's gradient, and the gradient of the used terms alone."""
    a, b = ms_inputs(tag, 128, 3)
    r = a.clone().requires_grad_(True)
    loss, sims, css = orc.msssim(r, b)
    loss.backward()
    u = a.clone().requires_grad_(True)
    _, s2, c2 = orc.msssim(u, b)
    (1 - torch.prod(c2[:4] ** MS_W[:4]) * s2[4] ** (4 * MS_W[4])).backward()
    return a, b, loss.detach(), sims.detach(), css.detach(), r.grad, u.grad


def same_pattern(what, got, want, rel=1e-4):
    """NaN exactly where the oracle has NaN; elsewhere to rel of the largest finite reference element."""
    got, want = got.cpu().double(), want.double()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: {int(torch.isnan(got).sum())} NaN, the oracle has {int(torch.isnan(want).sum())}"
    ok = ~torch.isnan(want)
    if ok.any():
        bar = rel * want[ok].abs().max().item()
        err = (got[ok] - want[ok]).abs().max().item()
        note(what, 128, err / bar)
        assert err <= bar, f"{what}: err {err:.3e} bar {bar:.3e}"


@pytest.mark.parametrize("tag", ["neg", "nan", "unused"])
def test_nan_and_negative_levels_at_128_wide(rigs, tag):
    W, B = 128, 3
    rig = rigs(W)
    a, b, loss, sims, css, grad, grad_used = signed_case(tag)
    used_negative = bool((css[:4] <= 0).any()) or bool(sims[4] <= 0)
    unused_negative = bool((sims[:4] <= 0).any()) or bool(css[4] <= 0)
    assert (tag == "nan") == used_negative and (tag != "neg") == unused_negative and torch.isnan(loss).item() == used_negative
    rb, xb = padded(a), padded(b)
    g = run_msssim(rig.H, W, B, rb, xb, nan_ok=True)
    s = g["scalars"].cpu()
    note(f"levels ({tag})", W, within("level means", s[3:13].double(), torch.cat((sims, css)).double(), torch.full((10,), 2e-5)))
    assert bool(((s[3:13] < 0) == (torch.cat((sims, css)) < 0)).all()), "a level mean has the other sign"
    assert torch.isnan(s[1]).item() == used_negative and torch.isnan(s[0]).item() == used_negative
    if not used_negative:
        assert abs(s[1].item() - loss.item()) <= 2e-5
    same_pattern(f"d_recon ({tag})", g["d_recon"], grad)
    # through cvae_loss_obj: the reference objective is the op; the used-terms gradient is finite unless a USED level is negative
    _, mu, lv, _ = rig.base
    mub, lvb = padded(mu[:B]), padded(lv[:B])
    ref_obj = run_loss(rig, B, xb, mub, lvb, rb, obj=(1.0, 0.0, 0.001, 0), nan_ok=True)
    assert same_bits(ref_obj["d_recon"], g["d_recon"]) and same_bits(ref_obj["scalars"][3:13], g["scalars"][3:13])
    used = run_loss(rig, B, xb, mub, lvb, rb, obj=(1.0, 0.0, 0.001, 1), nan_ok=True)
    assert same_bits(used["scalars"][:13], ref_obj["scalars"][:13])
    if not used_negative:
        assert bool(torch.isfinite(used["d_recon"]).all()), "the used-terms gradient is not finite though only unused levels are negative"
        assert bool(torch.isfinite(grad_used).all())
    same_pattern(f"used-terms d_recon ({tag})", used["d_recon"], grad_used)
