"""The guarded optimizer step without a GPU: argument checks of its C-ABI entry points (every call here fails them, so nothing is
launched), the documented record layout, and the trainer checkpoint through torch.save / torch.load on CPU tensors."""
import ctypes as C
import os
import re

import pytest
import torch

from critic_vae_amd import lib as cvlib
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer, load_trainer, save_trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096                                  # a non-null "device address": never dereferenced, every call below fails its checks first


def _refused(rc, *words):
    msg = cvlib.load().cvae_last_error().decode()
    assert rc == -1, rc                      # CVAE_EINVAL
    assert all(w in msg for w in words), msg


@pytest.mark.parametrize("max_norm", [0.0, -1.0, float("-inf"), float("nan")])
def test_grad_stats_refuses_a_bad_max_norm(max_norm):
    h = cvlib.Handle(64, 8)
    _refused(h.lib.cvae_grad_stats(h.h, FAKE, 4096, 1.0, max_norm, 1, 1e-4, 0.9, 0.999, FAKE, None), "cvae_grad_stats", "max_norm")


@pytest.mark.parametrize("n", [1, 6, 4095, -4])
def test_guard_calls_refuse_a_length_that_is_no_multiple_of_4(n):
    h = cvlib.Handle(64, 8)
    _refused(h.lib.cvae_grad_stats(h.h, FAKE, n, 1.0, float("inf"), 1, 1e-4, 0.9, 0.999, FAKE, None), "cvae_grad_stats", str(n))
    _refused(h.lib.cvae_adam_step_guarded(h.h, FAKE, FAKE, FAKE, FAKE, n, 1e-8, FAKE, None), "cvae_adam_step_guarded", str(n))


def test_guard_calls_refuse_null_arguments():
    h = cvlib.Handle(64, 8)
    lib = h.lib
    _refused(lib.cvae_grad_stats(None, FAKE, 4, 1.0, 1.0, 1, 1e-4, 0.9, 0.999, FAKE, None), "cvae_grad_stats")
    _refused(lib.cvae_grad_stats(h.h, None, 4, 1.0, 1.0, 1, 1e-4, 0.9, 0.999, FAKE, None), "cvae_grad_stats")
    _refused(lib.cvae_grad_stats(h.h, FAKE, 4, 1.0, 1.0, 1, 1e-4, 0.9, 0.999, None, None), "cvae_grad_stats")
    for k in range(5):
        ptrs = [FAKE] * 5
        ptrs[k] = None                       # params, grads, exp_avg, exp_avg_sq, state in turn
        _refused(lib.cvae_adam_step_guarded(h.h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], 4, 1e-8, ptrs[4], None), "cvae_adam_step_guarded")
    _refused(lib.cvae_guard_init(h.h, None, 0, 0, None), "cvae_guard_init")
    _refused(lib.cvae_guard_init(h.h, FAKE, -1, 0, None), "cvae_guard_init")
    _refused(lib.cvae_guard_init(h.h, FAKE, 0, -1, None), "cvae_guard_init")


def test_record_layout_is_the_documented_one():
    """lib.GuardRecord mirrors cvae_guard_record field for field at the offsets the header documents; the state holds the
    record plus one fp64 partial and one flag word per workgroup of the statistics pass."""
    hdr = open(os.path.join(ROOT, "include", "cvae.h")).read()
    body = re.search(r"typedef struct cvae_guard_record \{(.*?)\} cvae_guard_record;", hdr, re.S).group(1)
    documented = {}
    for line in body.splitlines():
        m = re.match(r"\s*\w+\s+([\w, ]+);\s*/\*\s*([\d, ]+):", line)
        if m:
            for name, off in zip(m.group(1).split(","), m.group(2).split(",")):
                documented[name.strip()] = int(off)
    got = {name: getattr(cvlib.GuardRecord, name).offset for name, _ in cvlib.GuardRecord._fields_}
    assert got == documented and len(got) == 13, (got, documented)
    assert C.sizeof(cvlib.GuardRecord) == 64
    nbytes = cvlib.load().cvae_guard_state_bytes()
    assert nbytes % 8 == 0 and nbytes == 64 + 256 * (8 + 4)


def test_trainer_arguments():
    vae = VariationalAutoencoder(max_batch=2, seed=0)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            FusedTrainer(vae, max_grad_norm=bad)
    assert not FusedTrainer(vae).guarded
    assert FusedTrainer(vae, skip_nonfinite=True).guarded and FusedTrainer(vae, max_grad_norm=float("inf")).guarded
    with pytest.raises(RuntimeError):
        FusedTrainer(vae).guard_stats()
    assert FusedTrainer(vae, max_grad_norm=2.0).guard_stats() == dict(applied=0, skipped=0, norm=0.0, coef=1.0)


@pytest.mark.parametrize("guarded", [False, True])
def test_state_dict_round_trip_through_torch_save(tmp_path, guarded):
    kw = dict(skip_nonfinite=True, max_grad_norm=3.0) if guarded else {}
    vae = VariationalAutoencoder(max_batch=2, seed=0)
    tr = FusedTrainer(vae, **kw)
    g = torch.Generator().manual_seed(5)
    tr.m.copy_(torch.randn(tr.m.numel(), generator=g))
    tr.v.copy_(torch.rand(tr.v.numel(), generator=g))
    tr.step_count, vae.num_batches_tracked = 7, 9
    if guarded:
        tr.load_state_dict(dict(tr.state_dict(), applied=5, skipped=2))
    sd = tr.state_dict()
    assert (sd["applied"], sd["skipped"]) == ((5, 2) if guarded else (7, 0))
    assert all(not t.is_cuda for t in (sd["m"], sd["v"]))
    sd["m"][0] += 1.0                                       # a copy: the trainer's own moments do not move with it
    assert sd["m"][0] != tr.m[0]
    path = save_trainer(tr, str(tmp_path / "trainer.pt"))
    vae2 = VariationalAutoencoder(max_batch=2, seed=1)
    tr2 = load_trainer(FusedTrainer(vae2, **kw), path)
    assert torch.equal(tr2.m, tr.m) and torch.equal(tr2.v, tr.v)
    assert tr2.step_count == 7 and vae2.num_batches_tracked == 9
    back = tr2.state_dict()
    assert (back["applied"], back["skipped"], back["step_count"], back["num_batches_tracked"]) == \
        (sd["applied"], sd["skipped"], 7, 9)
    if guarded:
        assert tr2.guard_stats() == dict(applied=5, skipped=2, norm=0.0, coef=1.0)
        with pytest.raises(ValueError):                     # an unguarded trainer corrects the bias by step_count: 5 != 7
            load_trainer(FusedTrainer(vae2), path)
    else:
        load_trainer(FusedTrainer(vae2, skip_nonfinite=True), path)      # the other direction is fine: every step was applied
    with pytest.raises(ValueError):
        tr2.load_state_dict(dict(sd, m=sd["m"][:-4]))


def test_cli_takes_the_guard_flags(tmp_path, monkeypatch):
    from critic_vae_amd import train
    seen = {}
    monkeypatch.setattr(train, "_train_episodes", lambda args: seen.setdefault("args", args))
    train.main(["-train", "--episodes", str(tmp_path), "--critic", "synth", "--skip-nonfinite", "--max-grad-norm", "2.5",
                "--resume", "old"])
    a = seen["args"]
    assert a.skip_nonfinite and a.max_grad_norm == 2.5 and a.resume == "old"
    seen.clear()
    train.main(["-train", "--episodes", str(tmp_path), "--critic", "synth"])
    a = seen["args"]
    assert not a.skip_nonfinite and a.max_grad_norm is None and a.resume is None
    for argv in (["-train", "--episodes", str(tmp_path), "--critic", "synth", "--max-grad-norm", "0"],
                 ["-train", "--skip-nonfinite"], ["-train", "--resume", "old"]):      # the torch-Adam loop has no guard
        with pytest.raises(SystemExit) as e:
            train.main(argv)
        assert e.value.code == 2
