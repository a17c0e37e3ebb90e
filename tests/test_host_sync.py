"""CPU: the host side of the staged step with global-batch statistics (include/cvae.h, cvae_sync_slot and the *_stage
calls) — the record layout, and every argument / order check, which must fail before any device access."""
import ctypes as C

import pytest

from critic_vae_amd import lib as cvlib

CVAE_EINVAL = -1
CHANNELS = (32, 64, 128, 256)
FAKE = 0x1000            # never dereferenced: every call below fails in its host-side checks


def test_sync_slots_are_disjoint_and_sized():
    slots = [cvlib.sync_slot(p) for p in range(cvlib.SYNC_POINTS)]
    want = [3 * c for c in CHANNELS] + [11] + [2 * c for c in reversed(CHANNELS)]
    want[0] += 1                                                     # point 0 also carries this rank's image count
    assert [n for _, n in slots] == want
    used = set()
    for off, n in slots:
        assert 0 <= off and off + n <= cvlib.SYNC_DOUBLES
        span = set(range(off, off + n))
        assert not (span & used)
        used |= span
    assert len(used) == cvlib.SYNC_DOUBLES                           # the record has no unused doubles
    lib = cvlib.load()
    off, n = C.c_int64(), C.c_int64()
    for bad in (-1, cvlib.SYNC_POINTS):
        assert lib.cvae_sync_slot(bad, C.byref(off), C.byref(n)) == CVAE_EINVAL
    assert lib.cvae_sync_slot(0, None, C.byref(n)) == CVAE_EINVAL


def test_sync_doubles_matches_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cvae.h")).read()
    assert int(re.search(r"#define CVAE_SYNC_DOUBLES (\d+)", hdr).group(1)) == cvlib.SYNC_DOUBLES


def _fwd(h, stage, B=4, train=1, sync=FAKE, ws=FAKE):
    return h.lib.cvae_forward_stage(h.h, B, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, ws, train, sync, stage, None)


def _loss(h, stage, B=4, sync=FAKE):
    return h.lib.cvae_loss_stage(h.h, B, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, sync, stage, None)


def _bwd(h, stage, B=4, sync=FAKE):
    return h.lib.cvae_backward_stage(h.h, B, *([FAKE] * 11), sync, stage, None)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_stage_arguments_and_order_are_checked_on_the_host(precision):
    h = cvlib.Handle(64, 4, precision=precision)
    # bad stage indices
    for s in (-1, 5):
        assert _fwd(h, s) == CVAE_EINVAL and b"stage" in h.lib.cvae_last_error()
        assert _bwd(h, s) == CVAE_EINVAL
    for s in (-1, 2):
        assert _loss(h, s) == CVAE_EINVAL
    # a null record
    assert _fwd(h, 0, sync=None) == CVAE_EINVAL and b"record" in h.lib.cvae_last_error()
    assert _loss(h, 0, sync=None) == CVAE_EINVAL
    assert _bwd(h, 0, sync=None) == CVAE_EINVAL
    # eval mode has no exchange: forward stages need train = 1
    assert _fwd(h, 0, train=0) == CVAE_EINVAL and b"train" in h.lib.cvae_last_error()
    # out of order: no step in progress, so only forward stage 0 is accepted
    for s in range(1, 5):
        assert _fwd(h, s) == CVAE_EINVAL and b"order" in h.lib.cvae_last_error()
    assert _loss(h, 0) == CVAE_EINVAL and b"order" in h.lib.cvae_last_error()
    assert _loss(h, 1) == CVAE_EINVAL
    for s in range(5):
        assert _bwd(h, s) == CVAE_EINVAL
    # the usual checks of the call a stage splits still apply (batch, workspace)
    assert _fwd(h, 0, B=5) == CVAE_EINVAL and b"batch" in h.lib.cvae_last_error()
    assert _fwd(h, 0, ws=None) != 0
    assert h.lib.cvae_forward_stage(None, 4, *([FAKE] * 9), 1, FAKE, 0, None) == CVAE_EINVAL
