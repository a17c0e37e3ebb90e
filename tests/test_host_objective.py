"""The configurable objective without a GPU: Objective's validation and schedule arithmetic, its state dict (alone and inside
the trainer checkpoint), the command line, the composition evaluate() reports, and the argument checks of cvae_loss_obj (every
call here fails them, so nothing is launched)."""
import ctypes as C
import math

import pytest

from critic_vae_amd import lib as cvlib
from critic_vae_amd import params as P
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.objective import Objective, compose
from critic_vae_amd.train import FusedTrainer, build_parser, load_trainer, objective_from_args, save_trainer

FAKE = 4096                                  # a non-null, 16-byte aligned "device address": never dereferenced


def test_defaults_are_the_reference_objective():
    o = Objective()
    assert o.at(0) == o.at(10 ** 6) == o.final() == (1.0, 0.0, P.kld_weight, 0)
    assert Objective(msssim_grad="used").final() == (1.0, 0.0, P.kld_weight, 1)


@pytest.mark.parametrize("kw", [dict(msssim=-1.0), dict(mse=-0.5), dict(kld=-1e-3), dict(msssim=float("nan")), dict(mse=float("inf")),
                                dict(kld=float("nan")), dict(msssim=0.0), dict(msssim=0.0, mse=0.0), dict(msssim_grad="both"),
                                dict(msssim_grad=1), dict(kld_warmup=-1), dict(kld_warmup=2.5), dict(msssim_from=-3),
                                dict(msssim_from=2), dict(msssim_from=2, mse=0.0)])
def test_validation_raises_value_error(kw):
    with pytest.raises(ValueError):
        Objective(**kw)


def test_valid_corner_objectives():
    assert Objective(msssim=0.0, mse=1.0).final()[:2] == (0.0, 1.0)         # pure MSE
    assert Objective(kld=0.0).final()[2] == 0.0                             # an autoencoder
    assert Objective(mse=1e-6, msssim_from=5).at(0)[0] == 0.0


def test_kld_warmup_edges():
    o = Objective(kld=0.004, kld_warmup=4)
    assert o.at(0)[2] == 0.004 * (1 / 4)                # step 0: the first step already carries 1 / N
    assert o.at(2)[2] == 0.004 * (3 / 4)                # warmup - 2
    assert o.at(3)[2] == 0.004                          # warmup - 1: (step + 1) / N == 1
    assert o.at(4)[2] == 0.004 and o.at(1000)[2] == 0.004
    assert o.final()[2] == 0.004
    assert Objective(kld=0.004, kld_warmup=1).at(0)[2] == 0.004
    assert all(o.at(s)[0] == 1.0 and o.at(s)[1] == 0.0 and o.at(s)[3] == 0 for s in range(6))
    with pytest.raises(ValueError):
        o.at(-1)


def test_msssim_from_edges():
    o = Objective(msssim=0.7, mse=2.0, msssim_from=3, msssim_grad="used")
    assert [o.at(s)[0] for s in (0, 2, 3, 4)] == [0.0, 0.0, 0.7, 0.7]      # step 0, from - 1, from, from + 1
    assert all(o.at(s)[1] == 2.0 and o.at(s)[3] == 1 for s in range(5))
    assert o.final() == (0.7, 2.0, P.kld_weight, 1)


def test_state_dict_round_trip():
    o = Objective(msssim=0.25, mse=3.0, kld=0.01, msssim_grad="used", kld_warmup=7, msssim_from=2)
    sd = o.state_dict()
    assert sd == dict(msssim=0.25, mse=3.0, kld=0.01, msssim_grad="used", kld_warmup=7, msssim_from=2)
    back = Objective().load_state_dict(sd)
    assert back == o and back.state_dict() == sd and all(back.at(s) == o.at(s) for s in range(10))
    with pytest.raises(ValueError):
        Objective().load_state_dict(dict(sd, mse=-1.0))
    with pytest.raises(KeyError):
        Objective().load_state_dict({"msssim": 1.0})


def test_trainer_carries_the_objective_through_its_checkpoint(tmp_path):
    vae = VariationalAutoencoder(max_batch=2, seed=0)
    assert vae.objective is None and FusedTrainer(vae).objective is None
    assert "objective" not in FusedTrainer(vae).state_dict()
    o = Objective(mse=1.0, kld_warmup=4, msssim_from=3)
    tr = FusedTrainer(vae, objective=o)
    tr.step_count = 2
    path = save_trainer(tr, str(tmp_path / "trainer.pt"))
    tr2 = load_trainer(FusedTrainer(VariationalAutoencoder(max_batch=2, seed=1)), path)
    assert tr2.objective == o and tr2.objective is not o and tr2.step_count == 2
    assert tr2.objective.at(tr2.step_count) == o.at(2)
    # a state written without an objective leaves the trainer's own in place
    plain = save_trainer(FusedTrainer(vae), str(tmp_path / "plain.pt"))
    assert load_trainer(FusedTrainer(vae, objective=o), plain).objective == o
    with pytest.raises(ValueError, match="global_stats"):
        FusedTrainer(vae, global_stats=True, objective=o)
    with pytest.raises(ValueError, match="global_stats"):
        load_trainer(FusedTrainer(vae, global_stats=True), path)
    with pytest.raises(ValueError):
        FusedTrainer(vae, objective=(1.0, 0.0, 0.001, 0))


def test_command_line_parses_the_six_flags_and_defaults_to_none(tmp_path, monkeypatch):
    from critic_vae_amd import train
    ap = build_parser()
    assert objective_from_args(ap.parse_args(["-train"])) is None
    a = ap.parse_args(["-train", "--msssim-weight", "0.5", "--mse-weight", "2", "--kld-weight", "0.004", "--msssim-grad", "used",
                       "--kld-warmup", "100", "--msssim-from", "20"])
    assert objective_from_args(a) == Objective(0.5, 2.0, 0.004, "used", 100, 20)
    assert objective_from_args(ap.parse_args(["-second", "--msssim-grad", "used"])) == Objective(msssim_grad="used")
    with pytest.raises(SystemExit):
        ap.parse_args(["-train", "--msssim-grad", "both"])
    seen = {}
    monkeypatch.setattr(train, "_train_episodes", lambda args: seen.setdefault("args", args))
    train.main(["-train", "--episodes", str(tmp_path), "--critic", "synth"])
    assert seen.pop("args").objective is None
    train.main(["-train", "--episodes", str(tmp_path), "--critic", "synth", "--mse-weight", "1", "--msssim-from", "10"])
    assert seen.pop("args").objective == Objective(mse=1.0, msssim_from=10)
    for bad in (["--mse-weight", "-1"], ["--msssim-weight", "0"], ["--msssim-from", "10"], ["--kld-weight", "nan"]):
        with pytest.raises(SystemExit):
            train.main(["-train", "--episodes", str(tmp_path), "--critic", "synth"] + bad)
    with pytest.raises(SystemExit):                      # the flags belong to the VAE's modes
        train.main(["-critic", "--episodes", str(tmp_path), "--rewards", str(tmp_path), "--save", str(tmp_path), "--mse-weight", "1"])


def test_synthetic_train_refuses_schedules_before_it_needs_a_device(capsys):
    from critic_vae_amd import train
    for flags in (["--kld-warmup", "5"], ["--mse-weight", "1", "--msssim-from", "5"]):
        with pytest.raises(SystemExit):
            train.main(["-train"] + flags)
        assert "belong to the fused trainer" in capsys.readouterr().err        # argparse's error, not the missing-GPU exit


def test_resume_keeps_the_checkpoints_objective_and_refuses_another(tmp_path, capsys):
    from critic_vae_amd.train import _check_resumed_objective
    vae = VariationalAutoencoder(max_batch=2, seed=0)
    o = Objective(mse=1.0, kld_warmup=4)
    with_obj = save_trainer(FusedTrainer(vae, objective=o), str(tmp_path / "a.pt"))
    plain = save_trainer(FusedTrainer(vae), str(tmp_path / "b.pt"))

    def resume(given, path):
        tr = load_trainer(FusedTrainer(vae, objective=given), path)
        _check_resumed_objective(given, tr, "DIR")
        return tr

    assert resume(None, plain).objective is None and capsys.readouterr().out == ""
    assert resume(None, with_obj).objective == o and "continuing with the objective saved in DIR" in capsys.readouterr().out
    assert resume(Objective(mse=1.0, kld_warmup=4), with_obj).objective == o          # the run's own flags repeated
    with pytest.raises(SystemExit, match="the flags give"):
        resume(Objective(mse=2.0, kld_warmup=4), with_obj)
    with pytest.raises(SystemExit, match="judged by total_loss"):
        resume(o, plain)


def test_validation_log_judges_by_the_objective_only_when_one_is_given():
    from critic_vae_amd.train import _ValidationLog
    assert _ValidationLog(None, False).key == "total_loss" and _ValidationLog.key == "total_loss"
    log = _ValidationLog(None, False, by_objective=True)
    assert log.key == "objective"
    r = dict(total_loss=0.5, recon_loss=0.4, KLD=0.1, images=3, finite_images=3, mean_total=0.5, worst=0.6, psnr=12.0, objective=0.25)
    assert log.line(None, r).startswith("objective 0.250000 loss 0.500000")
    assert _ValidationLog(None, False).line(None, r).startswith("loss 0.500000")


def test_compose_on_a_hand_made_record():
    r = dict(recon_loss=0.4, mean_mse=0.05, KLD=0.001 * 12.0, kld_raw=12.0, finite_images=9)
    assert compose(Objective(), r) == pytest.approx(0.4 + 0.001 * 12.0, rel=1e-15)
    assert compose(Objective(msssim=0.5, mse=2.0, kld=0.01), r) == pytest.approx(0.5 * 0.4 + 2.0 * 0.05 + 0.01 * 12.0, rel=1e-15)
    # the final weights, not those of an early step of the schedules
    assert compose(Objective(mse=2.0, kld=0.01, kld_warmup=100, msssim_from=50), r) == pytest.approx(0.4 + 0.1 + 0.12, rel=1e-15)
    # weight 0: the term is omitted, never multiplied — a NaN pooled MS-SSIM does not reach a pure-MSE objective
    nan_ms = dict(r, recon_loss=float("nan"))
    assert compose(Objective(msssim=0.0, mse=1.0, kld=0.01), nan_ms) == pytest.approx(0.05 + 0.12, rel=1e-15)
    assert math.isnan(compose(Objective(mse=1.0), nan_ms))
    assert compose(Objective(kld=0.0), dict(r, kld_raw=float("nan"), KLD=float("nan"))) == pytest.approx(0.4)
    # without kld_raw the raw mean comes back out of the weighted entry
    assert compose(Objective(kld=0.01), {k: v for k, v in r.items() if k != "kld_raw"}) == pytest.approx(0.4 + 0.12, rel=1e-12)


def test_ctypes_structure_matches_the_header():
    assert [n for n, _ in cvlib.Objective._fields_] == ["msssim_weight", "mse_weight", "kld_weight", "msssim_grad"]
    assert C.sizeof(cvlib.Objective) == 16 and (cvlib.MSGRAD_REFERENCE, cvlib.MSGRAD_USED) == (0, 1)


def _loss_obj(h, obj, ptrs=None, batch=2, ws=FAKE):
    p = [FAKE] * 9 if ptrs is None else ptrs           # x, mu, logvar, recon, scalars, d_recon, d_mu, d_logvar
    o = None if obj is None else C.byref(cvlib.Objective(*obj))
    return h.lib.cvae_loss_obj(h.h, batch, p[0], p[1], p[2], p[3], ws, o, p[4], p[5], p[6], p[7], None)


@pytest.mark.parametrize("obj,word", [((-1.0, 1.0, 0.001, 0), "weight"), ((1.0, -2.0, 0.001, 0), "weight"), ((1.0, 0.0, -0.001, 0), "weight"),
                                      ((float("nan"), 1.0, 0.001, 0), "weight"), ((1.0, float("inf"), 0.001, 0), "weight"),
                                      ((1.0, 0.0, float("nan"), 0), "weight"), ((0.0, 0.0, 0.001, 0), "msssim_weight + mse_weight"),
                                      ((1.0, 0.0, 0.001, 2), "msssim_grad"), ((1.0, 0.0, 0.001, -1), "msssim_grad"), (None, "null objective")])
def test_loss_obj_refuses_a_bad_objective(obj, word):
    h = cvlib.Handle(64, 8)
    assert _loss_obj(h, obj) == -1
    assert word in h.lib.cvae_last_error().decode()


def test_loss_obj_refuses_bad_arguments():
    h = cvlib.Handle(64, 8)
    good = (1.0, 1.0, 0.001, 1)
    assert _loss_obj(h, good, batch=0) == -1 and _loss_obj(h, good, batch=9) == -1
    assert _loss_obj(h, good, ws=None) == -3                                        # CVAE_ENOWS, as cvae_loss
    for k in range(5):                                                              # x, mu, logvar, recon, scalars
        ptrs = [FAKE] * 9
        ptrs[k] = None
        assert _loss_obj(h, good, ptrs) == -1, k
    for k in (5, 6, 7):                                                             # the gradients: all or none
        ptrs = [FAKE] * 9
        ptrs[k] = None
        assert _loss_obj(h, good, ptrs) == -1, k
    for k in (0, 3, 5):                                                             # x, recon, d_recon: 16-byte loads and stores
        ptrs = [FAKE] * 9
        ptrs[k] = FAKE + 4
        assert _loss_obj(h, good, ptrs) == -1 and "aligned" in h.lib.cvae_last_error().decode()
