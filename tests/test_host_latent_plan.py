"""cvae_op_latent_plan: the grids of the latent launches (fc.hip), from the function the launchers call.  Host logic only, no device.

For every batch 1..2100, both frame sizes and devices of 256, 64 and 304 compute units:
  * the job ranges of a merged launch tile [0, grid) in launch order, without gap or overlap; fc_bwd's dflat has a launch of its own
    (from block 0) exactly where K / 32 exceeds the compute units, and the other two jobs then tile theirs;
  * every job has the block count its body expects: K / 32 for a batch-contracted GEMM, ceil(B / 128) * FC_KS for latent_gemm,
    (K / 256) * ceil(B / images) for dflat, min(B, 128) for the column sum's first stage, (K / 1024) * ceil(B / images) for decin_fwd;
  * images per workgroup x image groups covers B, with the last group not empty;
  * the images per workgroup are the large-batch values (16 for decin_fwd, 32 for dflat), halved while the halved form's grid still
    fits two workgroups per compute unit, down to 4 / 8: restated here, so that the thresholds are the stated rule's;
  * at B >= 2048 they are 16 / 32 on all three devices."""
import ctypes as C

import pytest

from critic_vae_amd import lib as cvlib

FC_KS, CS_BLOCKS = 32, 128
CUS = [256, 64, 304]
WIDTHS = [64, 128]
BATCHES = range(1, 2101)


def cdiv(a, b):
    return -(-a // b)


def imgs_rule(B, col_blocks, hi, lo, cus):
    imgs = hi
    while imgs > lo and col_blocks * cdiv(B, imgs // 2) <= 2 * cus:
        imgs //= 2
    return imgs


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("W", WIDTHS)
def test_plan_ranges_counts_and_images(W, cus):
    K = 256 * (W // 16) ** 2
    seen_di, seen_df = set(), set()
    for B in BATCHES:
        p = cvlib.latent_plan(W, B, cus)
        what = f"W={W} B={B} cus={cus}: {p}"
        assert p["fc_fwd"]["gemm"] == cdiv(B, 128) * FC_KS, what
        assert p["fc_bwd"]["split"] == (K // 32 > cus), what
        for launch in ("decin_bwd", "fc_bwd"):
            jobs = dict(p[launch]["jobs"])                              # dict order = launch order
            if launch == "fc_bwd" and p[launch]["split"]:               # dflat alone in a second launch that starts at block 0
                lo, hi = jobs.pop("dflat")
                assert lo == 0 and hi > 0, what
            at = 0
            for name, (lo, hi) in jobs.items():
                assert lo == at and hi > lo, f"{launch}.{name} leaves a gap, overlaps or is empty; {what}"
                at = hi
            assert at == p[launch]["grid"], what
        db, fb = p["decin_bwd"]["jobs"], p["fc_bwd"]["jobs"]
        assert db["bgemm"][1] - db["bgemm"][0] == K // 32 and db["gemm"][1] - db["gemm"][0] == cdiv(B, 128) * FC_KS, what
        di, df = p["decin_fwd"]["imgs"], p["fc_bwd"]["imgs"]
        assert fb["bgemm"][1] - fb["bgemm"][0] == K // 32, what
        assert fb["dflat"][1] - fb["dflat"][0] == (K // 256) * cdiv(B, df), what
        assert fb["colsum"][1] - fb["colsum"][0] == min(B, CS_BLOCKS), what
        assert p["decin_fwd"]["grid"] == (K // 1024) * cdiv(B, di), what
        for imgs in (di, df):                                          # the groups cover B and the last one holds an image
            assert imgs * cdiv(B, imgs) >= B > imgs * (cdiv(B, imgs) - 1), what
        assert di == imgs_rule(B, K // 1024, 16, 4, cus) and df == imgs_rule(B, K // 256, 32, 8, cus), what
        if B >= 2048:
            assert (di, df) == (16, 32), what
        seen_di.add(di)
        seen_df.add(df)
    assert seen_di <= {16, 8, 4} and seen_df <= {32, 16, 8}
    if W == 64:
        assert seen_di == {16, 8, 4} and seen_df == {32, 16, 8}, "every compiled form is reached at 64 x 64"


def test_plan_rejects_bad_arguments():
    lib = cvlib.load()
    out = (C.c_int32 * cvlib.LATENT_PLAN_INTS)()
    for W, B, cus in ((32, 8, 256), (64, 0, 256), (64, 8, 0)):
        assert lib.cvae_op_latent_plan(W, B, cus, out) != 0
    assert lib.cvae_op_latent_plan(64, 8, 256, None) != 0
    with pytest.raises(cvlib.CvaeError):
        cvlib.latent_plan(96, 8, 256)
