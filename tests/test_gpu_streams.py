"""Every entry point of the C-ABI on a side stream, with the null stream held busy (tests/stream_tools.py has the method and the
scenarios; tests/test_host_streams.py holds the registry against include/cvae.h).

Each group of scenarios runs once, in a fresh child process (tests/stream_worker.py) with GPU_MAX_HW_QUEUES = 8 in its environment
and nothing else changed, under a time limit sized to the group; the child leaves a JSON record and the tests here assert on it.
A child that does not end normally starts nothing further: the groups behind it fail without having run.

What a scenario asserts (a-f) is described in stream_tools.py.  If the control finds no side stream that runs ahead of a blocked
null stream, b, c, d and f cannot be conclusive: they are recorded as "not run", printed by every test, and test_control fails.

Host-asynchronous by design, all of them: every scenario here asserts a and e.  (A wrapper that returned a Python float would be
registered with host_async=False and its reason; there is none today.)"""
import json
import os
import subprocess
import sys

import pytest

import stream_tools as ST

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_results, _stopped_by = {}, []


def group_result(group, tmp_path_factory):
    if group in _results:
        return _results[group]
    if _stopped_by:
        _results[group] = dict(not_started=f"not started: the child of group '{_stopped_by[0]}' did not end normally")
        return _results[group]
    out = str(tmp_path_factory.mktemp("streams") / f"{group}.json")
    env = dict(os.environ, GPU_MAX_HW_QUEUES=str(ST.HW_QUEUES))
    limit = ST.group_timeout(group) if group != "threads" else 240
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "stream_worker.py"), group, out], env=env, timeout=limit,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        _stopped_by.append(group)
        _results[group] = dict(failed=f"the child of group '{group}' did not end within {limit} s\n{e.stdout}\n{e.stderr}")
        return _results[group]
    print(r.stdout)
    if r.returncode != 0 or not os.path.exists(out):
        _stopped_by.append(group)
        _results[group] = dict(failed=f"the child of group '{group}' exited with {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}")
        return _results[group]
    with open(out) as f:
        _results[group] = json.load(f)
    if _results[group].get("stopped"):
        _stopped_by.append(group)
    return _results[group]


def usable(res):
    assert "not_started" not in res, res.get("not_started")
    assert "failed" not in res, res.get("failed")
    return res


def test_control_finds_an_independent_stream(tmp_path_factory):
    res = usable(group_result(ST.groups()[0], tmp_path_factory))
    print("control:", res["control"], "blocker:", res["blocker"])
    assert res["independent"], f"none of {len(res['control'])} side streams ran ahead of a blocked null stream: {res['control']}"


@pytest.mark.parametrize("name", [s.name for s in ST.SCENARIOS])
def test_scenario(name, tmp_path_factory):
    sc = next(s for s in ST.SCENARIOS if s.name == name)
    res = usable(group_result(sc.group, tmp_path_factory))
    assert name in res["scenarios"], f"{name}: not run, the group stopped at '{res['stopped']}'"
    rec = res["scenarios"][name]
    assert "error" not in rec, rec.get("error")
    print(f"{name}: duration {rec['duration_ms']:.3f} ms, blocker {rec['blocker_s']:.2f} s, asserts {rec['asserts']}")
    not_run = sorted(k for k, v in rec["asserts"].items() if v == ST.NOT_RUN)
    if not_run:
        print(f"{name}: NOT RUN: {', '.join(not_run)}" + ("" if res["independent"] else " (the control found no independent stream)"))
    for m in rec["messages"]:
        print(f"{name}: {m}")
    assert rec["called"] == rec["declared"], f"{name} declares {rec['declared']} but called {rec['called']}"
    failed = sorted(k for k, v in rec["asserts"].items() if v is False)
    assert not failed, f"{name}: failed {', '.join(failed)}:\n" + "\n".join(rec["messages"])
    if sc.host_async:
        assert rec["asserts"]["a"] is True and rec["asserts"]["e"] is True
    if res["independent"]:
        assert all(rec["asserts"][k] is True for k in "bcdf")


def test_two_threads_two_handles(tmp_path_factory):
    """An f32 handle (with a probe mask armed) and a bf16x9 handle, each with its own workspace and stream, run 20 steps from two
    threads released together: parameters, Adam state, BatchNorm statistics and every step's loss scalars equal the same steps run
    alone, word for word; the call refused in the second thread leaves the first thread's cvae_last_error() empty."""
    res = usable(group_result("threads", tmp_path_factory))
    a, b = res["threads"]
    for t in (a, b):
        assert t["raised"] is None, t["raised"]
        assert t["errors"] == [], t["errors"]
        assert t["differs"] == [], f"{t['precision']}: differs from the same {res['steps']} steps run alone: {t['differs']}"
    assert a["probe_count"] == res["steps"], f"the armed probe recorded {a['probe_count']} launches, not one per step"
    assert a["last_error"] == "", f"the refusal in the other thread shows in this one: {a['last_error']!r}"
    assert "batch" in b["last_error"], f"the refused call left no error in its own thread: {b['last_error']!r}"
