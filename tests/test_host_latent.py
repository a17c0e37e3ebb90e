"""The latent audit without a GPU: the exports of cvae_latent_stats / cvae_recon_response are declared and bound, the plan
arithmetic and every rejection that needs no device, latent.record_host against direct numpy formulas, and latent.summarize
on planted data: collapsed dimensions, a critic value that IS a linear function of mu, and one that is independent of it —
the probe against np.linalg.lstsq on the raw rows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from critic_vae_amd import latent as LT
from critic_vae_amd import lib as cvlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NEW = ("cvae_latent_stats_state_bytes", "cvae_latent_stats_scratch_bytes", "cvae_latent_stats_plan", "cvae_latent_stats",
       "cvae_recon_response")


def header():
    with open(os.path.join(ROOT, "include", "cvae.h")) as f:
        return f.read()


def test_exports_are_declared_and_bound():
    lib, text = cvlib.load(), header()
    for name in NEW:
        assert name in cvlib.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)), f"{name} is not declared in cvae.h"
    assert "#define CVAE_LATENT_STATE_DOUBLES 696" in text
    assert cvlib.LATENT_STATE_DOUBLES == LT.STATE_DOUBLES == 696 and lib.cvae_latent_stats_state_bytes() == 696 * 8
    for m in ("latent_stats", "latent_stats_state", "latent_stats_scratch", "latent_stats_scratch_bytes", "recon_response"):
        assert callable(getattr(cvlib.Handle, m))
    # the device entries end in (stream, flags): the stream-scenario registry of tests/stream_tools.py does not see them
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in ("cvae_latent_stats", "cvae_recon_response"):
        params = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", code, flags=re.S).group(1)
        assert re.search(r"void\s*\*\s*stream\s*,\s*uint32_t\s+flags\s*$", params.strip()), params


def test_record_layout_indices():
    assert LT.gram_index(0, 0) == 35 and LT.gram_index(0, 32) == 67 and LT.gram_index(1, 1) == 68 and LT.gram_index(32, 32) == 595
    seen = [LT.gram_index(i, j) for i in range(33) for j in range(i, 33)]
    assert seen == list(range(35, 596))
    assert (LT.SEEN, LT.USED, LT.SUM, LT.GRAM, LT.KL, LT.EXP, LT.LV, LT.RECORD) == (0, 1, 2, 35, 596, 628, 660, 692)


@pytest.mark.parametrize("cus", [1, 7, 256, 304, 5000])
def test_plan_arithmetic(cus):
    R = cvlib.latent_stats_plan(1, cus)["rows"]
    assert R >= 1
    for B in (1, 2, R - 1, R, R + 1, 2 * R + 1, cus * R - 1, cus * R, cus * R + 1, 2 * cus * R + 1, 1 << 24):
        if not 1 <= B <= 1 << 24:
            continue
        p = cvlib.latent_stats_plan(B, cus)
        chunks = -(-B // R)
        assert p == {"rows": R, "chunks": chunks, "grid": min(chunks, cus, 1024)}, (B, cus, p)


def test_plan_and_scratch_rejects():
    lib = cvlib.load()
    out = (C.c_int32 * 3)()
    for B, cus in ((0, 256), (-1, 256), ((1 << 24) + 1, 256), (1, 0), (1, -3)):
        assert lib.cvae_latent_stats_plan(B, cus, out) == EINVAL
        with pytest.raises(cvlib.CvaeError):
            cvlib.latent_stats_plan(B, cus)
    assert lib.cvae_latent_stats_plan(1, 1, None) == EINVAL
    H = cvlib.Handle(64, 4)
    assert lib.cvae_latent_stats_scratch_bytes(None, 4) == -1
    for B in (0, -5, (1 << 24) + 1):
        assert lib.cvae_latent_stats_scratch_bytes(H.h, B) == -1
        with pytest.raises(cvlib.CvaeError):
            H.latent_stats_scratch_bytes(B)
    # one partial of 692 doubles per workgroup the launch can have on any device; not capped by max_batch
    R = cvlib.latent_stats_plan(1, 1)["rows"]
    assert H.latent_stats_scratch_bytes(1) == 692 * 8 and H.latent_stats_scratch_bytes(R + 1) == 2 * 692 * 8
    assert H.latent_stats_scratch_bytes(1 << 24) == min(-(-(1 << 24) // R), 1024) * 692 * 8
    assert H.latent_stats_scratch_bytes(100000) % 16 == 0


def test_einval_paths_that_need_no_device():
    """Every argument is checked before any device access: these calls return CVAE_EINVAL on a machine without a GPU."""
    lib = cvlib.load()
    H = cvlib.Handle(64, 4)
    A = 1 << 20            # an aligned address that is never dereferenced
    ok = dict(h=H.h, B=4, mu=A, lv=A, pred=A, state=A, kl=None, scratch=A, stream=None, flags=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cvae_latent_stats(a["h"], a["B"], a["mu"], a["lv"], a["pred"], a["state"], a["kl"], a["scratch"], a["stream"], a["flags"])

    for bad in (dict(h=None), dict(mu=None), dict(lv=None), dict(pred=None), dict(state=None), dict(scratch=None), dict(flags=1),
                dict(flags=0x80000000), dict(B=0), dict(B=-1), dict(B=(1 << 24) + 1), dict(state=A + 4), dict(scratch=A + 4),
                dict(mu=A + 2), dict(lv=A + 1), dict(pred=A + 3), dict(kl=A + 2)):
        assert call(**bad) == EINVAL, bad
        assert lib.cvae_last_error()

    def resp(h=H.h, n=2, K=34, base=A, var=A, out=A, flags=0):
        return lib.cvae_recon_response(h, n, K, base, var, out, None, flags)

    for bad in (dict(h=None), dict(base=None), dict(var=None), dict(out=None), dict(flags=2), dict(n=0), dict(K=0), dict(n=-1),
                dict(n=1 << 16, K=1 << 15), dict(n=(1 << 31) - 1, K=(1 << 31) - 1), dict(base=A + 4), dict(var=A + 8), dict(out=A + 2)):
        assert resp(**bad) == EINVAL, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# record_host and summarize
# ---------------------------------------------------------------------------------------------------------------------------------
def planted(seed=0, n=4096, pred="linear"):
    rng = np.random.default_rng(seed)
    mu = (rng.standard_normal((n, 32)) * rng.uniform(0.3, 2.0, 32)).astype(np.float32)
    lv = (rng.standard_normal((n, 32)) * 0.5 - 1.0).astype(np.float32)
    dead = np.array([0, 5, 9, 13, 20, 21, 30, 31])
    mu[:, dead], lv[:, dead] = 0.0, 0.0
    if pred == "linear":
        p = 0.5 + 0.1 * mu[:, 3].astype(np.float64) - 0.05 * mu[:, 7].astype(np.float64)     # float64: exactly linear in the stored mu
    else:
        p = rng.uniform(0, 1, n)
    return mu, lv, p, dead


def test_record_host_against_direct_formulas():
    mu, lv, p, _ = planted(1, 300, "random")
    p = p.astype(np.float32)
    mu[7, 3] = np.nan; lv[11, 0] = np.inf; lv[12, 1] = -np.inf; lv[13, 2] = 800.0; p[14] = np.nan; lv[15, 4] = 100.0
    rec = LT.record_host(mu, lv, p.reshape(-1, 1))
    keep = np.ones(300, bool)
    keep[[7, 11, 12, 13, 14]] = False
    m, l, q = mu[keep].astype(np.float64), lv[keep].astype(np.float64), p[keep].astype(np.float64)
    assert rec.shape == (692,) and rec[0] == 300 and rec[1] == 295
    a = np.concatenate([m, q[:, None]], 1)
    assert np.array_equal(rec[2:35], a.sum(0))
    for i, j in ((0, 0), (0, 32), (3, 17), (31, 32), (32, 32)):
        want = float(np.sum(a[:, i] * a[:, j]))
        assert abs(rec[LT.gram_index(i, j)] - want) <= 1e-12 * np.sum(np.abs(a[:, i] * a[:, j]))
    assert np.allclose(rec[596:628], (0.5 * (m * m + np.exp(l) - l - 1)).sum(0), rtol=1e-14, atol=0)
    assert np.allclose(rec[628:660], np.exp(l).sum(0), rtol=1e-14, atol=0) and np.array_equal(rec[660:692], l.sum(0))
    assert np.isfinite(rec).all() and rec[628 + 4] > 1e43          # logvar = 100 stays in


def raw_fit(mu, p):
    X = np.concatenate([np.ones((mu.shape[0], 1)), mu.astype(np.float64)], 1)
    w = np.linalg.lstsq(X, p, rcond=None)[0]
    res = p - X @ w
    return w[1:], w[0], 1.0 - float(res @ res) / float(((p - p.mean()) ** 2).sum())


def test_summarize_planted_collapse_and_linear_leak():
    mu, lv, p, dead = planted(0, 4096, "linear")
    s = LT.summarize(LT.record_host(mu, lv, p))
    assert s["rows"] == s["used"] == 4096
    alive = np.setdiff1d(np.arange(32), dead)
    assert not s["active"][dead].any() and s["collapsed"][dead].all() and s["active"][alive].all() and not s["collapsed"][alive].any()
    assert s["n_active"] == 24
    assert np.array_equal(s["kl_per_dim"][dead], np.zeros(8)) and np.array_equal(s["mean_posterior_var"][dead], np.ones(8))
    assert np.allclose(s["mu_var"], mu.astype(np.float64).var(0), rtol=1e-10, atol=1e-14)
    assert np.allclose(s["mu_mean"], mu.astype(np.float64).mean(0), rtol=0, atol=1e-12)
    assert np.allclose(s["aggregate_var"], s["mu_var"] + np.exp(lv.astype(np.float64)).mean(0), rtol=1e-12)
    assert abs(s["kl_total"] - s["kl_per_dim"].sum()) <= 1e-12 and abs(s["pred_var"] - p.var()) <= 1e-12
    w, b, r2 = raw_fit(mu, p)
    assert np.abs(s["probe_weights"] - w).max() <= 1e-9 and abs(s["probe_bias"] - b) <= 1e-9 and abs(s["probe_r2"] - r2) <= 1e-9
    assert s["probe_r2"] > 1 - 1e-9
    want = np.zeros(32); want[3], want[7] = 0.1, -0.05
    assert np.abs(s["probe_weights"] - want).max() <= 1e-9 and abs(s["probe_bias"] - 0.5) <= 1e-9
    c = np.array([0.0 if j in dead else np.corrcoef(mu[:, j].astype(np.float64), p)[0, 1] ** 2 for j in range(32)])
    assert np.abs(s["corr2_per_dim"] - c).max() <= 1e-9
    assert len(LT.report_lines(s)) == 36


def test_summarize_independent_pred_matches_the_raw_fit():
    mu, lv, p, _ = planted(3, 4096, "random")
    s = LT.summarize(LT.record_host(mu, lv, p))
    w, b, r2 = raw_fit(mu, p)
    print("independent pred: R^2", s["probe_r2"], "raw rows", r2)
    assert abs(s["probe_r2"] - r2) <= 1e-9 and np.abs(s["probe_weights"] - w).max() <= 1e-9 and abs(s["probe_bias"] - b) <= 1e-9


def test_singular_and_empty_records_do_not_raise():
    n = 64
    mu = np.zeros((n, 32), np.float32)
    mu[:, 1] = np.arange(n)
    mu[:, 2] = 2 * mu[:, 1]                    # collinear, and 30 constant dimensions
    s = LT.summarize(LT.record_host(mu, np.zeros((n, 32), np.float32), 0.25 * mu[:, 1]))
    assert s["n_active"] == 2 and abs(s["probe_r2"] - 1.0) <= 1e-9 and np.isfinite(s["probe_weights"]).all()
    s = LT.summarize(LT.record_host(mu, np.zeros((n, 32), np.float32), np.full(n, 0.5)))      # a constant critic value
    assert np.isnan(s["probe_r2"]) and s["pred_var"] == 0.0
    e = LT.summarize(np.zeros(LT.STATE_DOUBLES))
    assert e["rows"] == 0 and e["used"] == 0 and np.isnan(e["kl_total"]) and e["n_active"] == 0
    LT.report_lines(e)


def test_summarize_response():
    r = np.zeros((3, 34, 2))
    r[:, :32, 0] = np.arange(1, 33)[None, :]
    r[:, 32, 0], r[:, 33, 0], r[:, 32, 1] = 33.0, 7.0, 0.5
    s = LT.summarize_response(r)
    assert s["frames"] == 3 and np.array_equal(s["latent_response"], np.arange(1, 33.0)) and s["pred_response"] == 33.0
    assert s["pred_one_response"] == 7.0 and s["pred_grey_max"] == 0.5 and s["pred_to_latent_ratio"] == 33.0 / 16.5
    mu, lv, p, _ = planted(0, 256, "random")
    assert len(LT.report_lines(LT.summarize(LT.record_host(mu, lv, p)), s)) == 37


# ---------------------------------------------------------------------------------------------------------------------------------
# command lines and files
# ---------------------------------------------------------------------------------------------------------------------------------
def test_latent_report_flag_belongs_to_the_fused_vae_trainers(capsys):
    from critic_vae_amd import train as T
    ap = T.build_parser()
    assert ap.parse_args(["-train", "--episodes", "E", "--critic", "synth", "--latent-report"]).latent_report is True
    assert ap.parse_args(["-second", "--dataset", "D", "--critic", "synth"]).latent_report is False
    for argv in (["-train", "--latent-report"],                                                    # the synthetic -train loop
                 ["-critic", "--episodes", "E", "--rewards", "R", "--save", "S", "--latent-report"],
                 ["-dataset", "--episodes", "E", "--critic", "synth", "--out", "O", "--latent-report"]):
        with pytest.raises(SystemExit) as e:
            T.main(argv)
        assert e.value.code == 2 and "--latent-report belongs to the fused VAE trainer" in capsys.readouterr().err


def test_latent_cli_parser():
    ap = LT.build_parser()
    a = ap.parse_args(["--networks", "N", "--critic", "synth", "--episodes", "E1", "E2"])
    assert (a.second, a.precision, a.batch, a.au_threshold, a.out, a.response, a.delta, a.response_frames) == \
        (False, "f32", 256, 0.01, None, False, 1.0, 256) and a.episodes == ["E1", "E2"]
    a = ap.parse_args(["--networks", "N", "--critic", "C", "--episodes", "E", "--second", "--precision", "bf16", "--batch", "64",
                       "--au-threshold", "0.02", "--out", "o.npz", "--response", "--delta", "0.5", "--response-frames", "8"])
    assert (a.second, a.precision, a.batch, a.au_threshold, a.out, a.response, a.delta, a.response_frames) == \
        (True, "bf16", 64, 0.02, "o.npz", True, 0.5, 8)
    for bad in (["--critic", "C", "--episodes", "E"], ["--networks", "N", "--critic", "C", "--episodes", "E", "--precision", "bf16x9"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_save_npz_round_trip(tmp_path):
    mu, lv, p, _ = planted(0, 512, "linear")
    s = LT.summarize(LT.record_host(mu, lv, p))
    s.update({f"response_{k}": v for k, v in LT.summarize_response(np.ones((2, 34, 2))).items()})
    path = LT.save_npz(str(tmp_path / "latent.npz"), s)
    with np.load(path) as f:
        assert set(f.files) == set(s)
        for k, v in s.items():
            assert np.array_equal(f[k], np.asarray(v), equal_nan=True), k
        assert f["record"].shape == (692,) and f["active"].dtype == bool
        again = LT.summarize(f["record"])
    assert np.array_equal(again["probe_weights"], s["probe_weights"]) and again["n_active"] == s["n_active"]
