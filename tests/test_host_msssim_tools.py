"""Host checks of the MS-SSIM / KLD helpers of ws_tools that tests/test_gpu_msssim_ops.py stands on: the launch geometry against the
numbers worked out by hand from msssim.hip, the float64 restatement of the loss on replica batches against the oracle, and the
properties of the generated inputs that the device checks rely on, each shown with the reference alone."""
import pytest
import torch

from oracle import cvae_oracle as orc
from ws_tools import (MS_BASES, MS_CASES, MS_CONFIG_BATCH, MS_RAGGED, kld_case, kld_ref, ms_assert_edge, ms_base_pairs, ms_case_batch,
                      ms_counts, ms_inputs, ms_level_facts, ms_loss_from_means, ms_oracle64, ms_plane_geom, ms_replica_ref,
                      ms_resident_groups, ms_swap_shift)

SCORE_POOL = (257, 683)              # (e) of the device tests
KLD_BATCHES = (1, 255, 256, 257, 683)      # (f)


def case_batches(W):
    return sorted({ms_case_batch(w, l, e, 256) for w, l, e in MS_CASES if w == W} | set(MS_RAGGED) | set(SCORE_POOL))


def test_plane_geometry_restates_msp_at_256_compute_units():
    want = {64: (156480, 256, 86), 32: (45632, 768, 257), 16: (59136, 512, 683), 8: (88064, 256, 1366), 4: (153600, 256, 5462)}
    for S, (smem, resident, first) in want.items():
        g = ms_plane_geom(S)
        assert g["SMEM"] == smem and g["SMEM"] <= 160 * 1024 - 256, (S, g)
        assert ms_resident_groups(S, 256) == resident, S
        level = {64: 0, 32: 1, 16: 2, 8: 3, 4: 4}[S]
        assert ms_case_batch(64, level, "loops", 256) == first and ms_case_batch(64, level, "below", 256) == first - 1
        if S >= 8:                   # the same kernel one level further down at 128 wide
            assert ms_case_batch(128, level + 1, "loops", 256) == first
    assert [ms_plane_geom(S)["PPW"] for S in (64, 32, 16, 8, 4)] == [1, 1, 4, 16, 64]
    assert [ms_plane_geom(S)["NT"] for S in (64, 32, 16, 8, 4)] == [1024, 256, 256, 256, 256]


def test_case_batches_at_256_compute_units():
    got = {W: [ms_case_batch(w, l, e, 256) for w, l, e in MS_CASES if w == W] for W in (64, 128)}
    assert got[64] == [85, 86, 256, 257, 682, 683, 1365, 1366, 5461, 5462, 2048]
    assert got[128] == [85, 86, 256, 257, 682, 683, 1365, 1366, 1024]
    for W, level, edge in MS_CASES:
        f = ms_assert_edge(W, level, edge, ms_case_batch(W, level, edge, 256), 256)
        assert [x["S"] for x in f] == [W >> l for l in range(5)]
    # the stream kernel: one workgroup per compute unit, a second plane from P = 257 on
    f = ms_level_facts(128, 86, 256)
    assert (f[0]["kernel"], f[0]["grid"], f[0]["trips"], f[0]["min_trips"]) == ("stream", 256, 2, 1)
    assert ms_level_facts(128, 85, 256)[0]["grid"] == 255
    # the configs' batches: four levels loop; the deepest of them ends unevenly (S = 8 at 64 wide, S = 16 at 128 wide: at 128 wide
    # B = 1024 has only 192 groups of 16 planes at S = 8, one trip)
    f = ms_level_facts(64, MS_CONFIG_BATCH[64], 256)
    assert [(x["S"], x["groups"], x["grid"], x["trips"], x["min_trips"]) for x in f[3:]] == [(8, 384, 256, 2, 1), (4, 96, 96, 1, 1)]
    f = ms_level_facts(128, MS_CONFIG_BATCH[128], 256)
    assert [(x["S"], x["groups"], x["grid"], x["trips"], x["min_trips"]) for x in f[3:]] == [(16, 768, 512, 2, 1), (8, 192, 192, 1, 1)]
    with pytest.raises(AssertionError):                  # more compute units move every edge: the case must notice
        ms_assert_edge(64, 0, "loops", 86, 304)
    assert ms_case_batch(64, 0, "loops", 304) == 102


def test_ragged_batches_cover_the_last_group_shapes():
    last = {B: [x["last_group"] for x in ms_level_facts(64, B, 256)[2:]] for B in MS_RAGGED}         # S = 16, 8, 4: groups of 4, 16, 64
    assert last == {1: [3, 3, 3], 21: [3, 15, 63], 22: [2, 2, 2], 43: [1, 1, 1], 64: [4, 16, 64]}
    assert all(x["trips"] == 1 for B in MS_RAGGED for W in (64, 128) for x in ms_level_facts(W, B, 256))


def test_replica_reference_equals_the_oracle_on_the_expanded_batch():
    """(a): B = 7, counts (2, 2, 1, 1, 1)."""
    x, _, _, recon = ms_base_pairs(64)
    B = 7
    idx = torch.arange(B) % MS_BASES
    full = recon[idx].double().requires_grad_(True)
    loss, sims, css = ms_oracle64(full, x[idx])
    loss.backward()
    ref = ms_replica_ref(recon, x, ms_counts(B))
    assert ms_counts(B).tolist() == [2, 2, 1, 1, 1]
    assert abs(ref["loss"].item() - loss.item()) <= 1e-12
    assert (ref["ssim"] - sims.detach()).abs().max().item() <= 1e-12 and (ref["cs"] - css.detach()).abs().max().item() <= 1e-12
    gmax = full.grad.abs().max().item()
    assert (ref["grad"][idx] - full.grad).abs().max().item() <= 1e-12 * gmax
    # ... and the oracle's own fp32 evaluation is that to fp32 round-off
    l32, s32, c32 = orc.msssim(recon[idx], x[idx])
    assert abs(l32.item() - loss.item()) <= 2e-6 and (s32.double() - sims.detach()).abs().max().item() <= 2e-6


@pytest.mark.parametrize("W", [64, 128])
def test_every_case_batch_has_positive_levels_and_a_finite_loss(W):
    """(b): then the used-terms product and autograd's gradient are finite and the gradient bars apply."""
    x, _, _, recon = ms_base_pairs(W)
    ref = ms_replica_ref(recon, x)
    ps, pc = ref["plane_ssim"].mean(1), ref["plane_cs"].mean(1)
    batches = case_batches(W) + list(KLD_BATCHES)
    for B in batches:
        n = ms_counts(B)
        sims, css = (n[:, None] * ps).sum(0) / B, (n[:, None] * pc).sum(0) / B
        assert bool((sims > 0).all()) and bool((css > 0).all()), (W, B, sims, css)
        assert 0 < ms_loss_from_means(sims, css).item() < 1, (W, B)
        if B in (min(batches), 22, max(batches)):        # the whole reference, gradient included, where the counts are most uneven
            r = ms_replica_ref(recon, x, n)
            assert abs(r["loss"].item() - ms_loss_from_means(sims, css).item()) <= 1e-15 and torch.isfinite(r["grad"]).all(), (W, B)
            assert (r["ssim"] - sims).abs().max().item() <= 1e-15 and (r["cs"] - css).abs().max().item() <= 1e-15


@pytest.mark.parametrize("W,B", [(64, 5462), (128, 1366)])
def test_a_misplaced_plane_moves_a_level_mean_by_eight_ulps(W, B):
    """(c): at the largest batch of each width, one plane of base image k taken from image k + 1 instead, at any level: the 1-ulp check
    of the level scalars (test_gpu_msssim_ops, (c)) cannot miss it."""
    assert B == max(ms_case_batch(w, l, e, 256) for w, l, e in MS_CASES if w == W)
    x, _, _, recon = ms_base_pairs(W)
    n = ms_counts(B)
    shift = ms_swap_shift(ms_replica_ref(recon, x, n), n)
    assert shift.shape == (MS_BASES, 3, 5)
    print(f"W {W} B {B}: smallest shift per level, in ulps: {shift.amin(dim=(0, 1)).tolist()}")
    assert shift.min().item() >= 8.0, shift.amin(dim=1)


@pytest.mark.parametrize("W", [64, 128])
def test_a_flipped_image_scores_nan(W):
    """(e): recon = 1 - x of a base image: negative cs means, a NaN MS-SSIM loss for that image alone."""
    x = ms_base_pairs(W)[0]
    for k in range(MS_BASES):
        loss, _, css = orc.msssim(1 - x[k:k + 1], x[k:k + 1])
        assert torch.isnan(loss) and css[0].item() < 0


@pytest.mark.parametrize("B", KLD_BATCHES)
def test_kld_bound_notices_one_dropped_image(B):
    """(f): the bound of the KLD scalar is round-off sized, the reference is the oracle's KLD, and leaving out ANY one image's 32 terms
    moves the KLD by more than four times the bound (1e-8; the project's 2e-5 bar cannot see that at B = 257, where one image moves
    the KLD by 1.6e-5, nor at B = 683: 6e-6)."""
    mu, lv = kld_case(B)
    assert float(lv.abs().max()) <= 1 and len({tuple(r.tolist()) for r in mu}) == B
    r = kld_ref(mu, lv)
    o = orc.vae_loss(torch.zeros(1, 3, 64, 64), mu.double(), lv.double(), torch.zeros(1, 3, 64, 64))["KLD"].item()
    assert abs(r["kld"].item() - o) <= 1e-7 * abs(o)                 # 0.001f against 0.001
    moved = 0.5 * 0.001 * r["terms"].abs().min().item() / B
    print(f"B {B}: KLD {r['kld'].item():.6e} bound {r['kld_bound'].item():.3e}, one image moves it by at least {moved:.3e}")
    assert r["kld_bound"].item() <= 2e-6 * abs(r["kld"].item())
    assert moved > 4 * r["kld_bound"].item()
    assert bool((r["d_mu_bound"] <= 4e-7 * r["d_mu"].abs() + 1e-44).all())
    # d_logvar: the bound stays a few ulps of kw e / (2 B), the size of the terms that cancel
    assert bool((r["d_logvar_bound"] <= 12 * 2.0 ** -24 * 0.5 * 0.001 * lv.double().exp().clamp_min(1.0) / B).all())


def test_negative_and_nan_inputs_at_128_wide():
    """(g): which level means are negative, on the CPU: "nan" has negative used levels (cs 0..3) and a NaN loss; "neg" has none at this
    size and a finite loss and gradient; "unused" has negative ssim means at the fine levels only: a finite loss whose reference
    gradient is NaN everywhere (the 0 * x^(w - 1) terms of the unused powers), a finite used-terms gradient."""
    from test_gpu_ops import _ms_inputs
    for tag in ("pos", "neg", "nan"):                    # the restatement makes test_msssim's pairs at test_msssim's shape
        assert all(torch.equal(p, q) for p, q in zip(ms_inputs(tag, 64, 4), _ms_inputs(tag))), tag
    W, B = 128, 3
    out = {}
    for tag in ("neg", "nan", "unused"):
        a, b = ms_inputs(tag, W, B)
        a.requires_grad_(True)
        loss, sims, css = orc.msssim(a, b)
        loss.backward()
        out[tag] = (loss.item(), sims.detach(), css.detach(), a.grad)
        print(tag, loss.item(), sims.tolist(), css.tolist())
    loss, sims, css, g = out["neg"]
    assert torch.isfinite(torch.tensor(loss)) and bool((sims > 0).all()) and bool((css > 0).all()) and bool(torch.isfinite(g).all())
    loss, sims, css, g = out["nan"]
    assert loss != loss and bool((css[:4] < 0).all()) and css[4].item() > 0 and bool((sims[:2] < 0).all()) and bool((sims[2:] > 0).all())
    assert bool(torch.isnan(g).all())
    loss, sims, css, g = out["unused"]
    assert 0 < loss < 1 and bool((css > 0).all()) and bool((sims[:2] < 0).all()) and bool((sims[2:] > 0).all())
    assert bool(torch.isnan(g).all())
