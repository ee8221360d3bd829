"""The library under concurrent host threads against the oracle (tests/threadsuite.py, which holds the jobs, the expected results and the
runner): every call surface from four caller threads with a context each, objects handed from thread to thread between calls and destroyed
on threads that did not make them, PIPE-mode streams closed while their worker is ahead so that another thread's next stream takes their
engine and pinned blocks, the caches released between two rounds, and the device-resident chain (decode, index, the first hash of a fresh
handle, gather under verify_table) on four threads beside a thread of streams. Everything expected comes from the oracle, computed before a
thread starts. The suite runs ONCE, in a fresh child process; the tests below read its report. A hang or a fault ends the session: nothing
further may start on the GPU behind one."""
import json
import os
import subprocess
import sys
import time

import pytest

import threadsuite as ts

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT_S = 600


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("threads") / "report.json")
    t0 = time.monotonic()
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "threadsuite.py"), "--report", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=LIMIT_S)
        code, tail = p.returncode, (p.stdout.decode(errors="replace")[-1500:], p.stderr.decode(errors="replace")[-3000:])
    except subprocess.TimeoutExpired as e:
        code, tail = None, ("no answer in %d s" % LIMIT_S, (e.stderr or b"").decode(errors="replace")[-3000:])
    rep = json.load(open(path)) if os.path.exists(path) else None
    if code is None or code == 3 or code < 0:
        what = "timed out" if code is None else "a thread hung: %s" % (rep or {}).get("hung") if code == 3 else "died on signal %d" % -code
        pytest.exit("tests/threadsuite.py %s; scenarios that ran: %s; %s" % (what, (rep or {}).get("ran"), tail), returncode=1)
    assert code == 0 and rep is not None, (code, tail)
    rep["test_wall_s"] = round(time.monotonic() - t0, 2)
    print("\nthreadsuite: %.1f s in all; t_serial %s; wall %s; deadlines %s" % (
        rep["test_wall_s"], rep["t_serial"], {n: s["wall_s"] for n, s in rep["scenarios"].items()}, rep["deadline_s"]))
    return rep


def _lists():
    return dict(ts.build(), serial=[ts.serial_list(ts.build())])


def check_scenario(rep, name, what):
    assert name in rep["scenarios"], "%s did not run: %s" % (name, rep["stopped"])
    res = rep["scenarios"][name]
    assert res["hung"] == []
    bad = ["thread %d, %s %s (%s, mode %s): %s: %s" % (i, r["kind"], r["id"], r["name"], ts.MODES[r["mode"]] if r["mode"] is not None else None,
                                                       r["verdict"], r["detail"]) for i, r in ts.failures(res)]
    assert not bad, "%s: %d of %d jobs: %s" % (what, len(bad), sum(len(t["records"]) for t in res["threads"]), bad[:12])
    lists = _lists()[name]
    assert len(res["threads"]) == len(lists)
    for i, (th, lst) in enumerate(zip(res["threads"], lists)):                     # every thread ran every job of its list
        assert th["done"] and [r["id"] for r in th["records"]] == [j.id for j in lst], (name, i)
    assert res["wall_s"] <= res["deadline_s"]
    return res


def test_serial(report):
    """every job of every list on one thread and one context: a disagreement here is an ordinary parity failure, not a concurrency finding"""
    res = check_scenario(report, "serial", "parity with the oracle on ONE thread (no concurrency involved)")
    assert [c["wrong"] for c in res["main_checks"] if c["wrong"]] == []
    assert set(report["t_serial"]) == set(ts.CONCURRENT) and all(v > 0 for v in report["t_serial"].values())


def test_own_contexts(report):
    check_scenario(report, "own_contexts", "four threads, a context each, made inside the thread")


def test_moved(report):
    res = check_scenario(report, "moved", "objects handed from thread to thread between calls")
    assert sorted(d["group"] for d in res["destroyed"]) == [0, 1, 2] and all(d["off_thread"] for d in res["destroyed"]), res["destroyed"]


def test_churn(report):
    res = check_scenario(report, "churn", "streams abandoned beside streams read to their end, the caches released in between")
    assert res["released"] and len(res["released"]) == 1 and res["released"][0]["on_main_thread"], res["released"]


def test_device(report):
    res = check_scenario(report, "device", "the device-resident chain on four threads beside a thread of streams")
    assert [c["wrong"] for c in res["main_checks"] if c["wrong"]] == []            # arenas, guards, gaps and sources, checked on the main thread after the join
    assert len(res["main_checks"]) == 2 * ts.T
    serial = {r["id"]: r["extra"] for r in report["scenarios"]["serial"]["threads"][0]["records"] if r["kind"] == "device"}
    mine = {r["id"]: r["extra"] for th in res["threads"] for r in th["records"] if r["kind"] == "device"}
    assert len(mine) == 2 * ts.T and mine == serial                                # per entry and per range what the serial pass got


def test_coverage(report):
    """what ran is what was meant to run: the floors are conditions on the seeded lists (tests/test_threadsuite_cpu.py pins them from the
    oracle alone); here they are held against the records of the run"""
    scen = report["scenarios"]
    ran = {sc: [[r for r in th["records"] if r["verdict"] == "ok"] for th in scen[sc]["threads"]] for sc in ts.CONCURRENT if sc in scen}
    assert list(ran) == list(ts.CONCURRENT)
    cov = ts.coverage(ran)
    assert [what for what, holds in ts.floors(cov) if not holds] == [], cov
    assert any(d["off_thread"] for d in scen["moved"]["destroyed"])                # a moved object was destroyed off its creating thread
    rel = scen["churn"]["released"]
    assert len(rel) == 1 and rel[0]["on_main_thread"]                              # the caches were released between the churn rounds ...
    for th in scen["churn"]["threads"]:                                            # ... with every stream of round one closed and none of round two open
        at = [r["kind"] for r in th["records"]].index("release_caches")
        assert th["records"][at - 1]["t1"] <= th["records"][at]["t0"] and th["records"][at]["t1"] <= th["records"][at + 1]["t0"]
    # the threads did run at once: in every concurrent scenario at least two threads' jobs overlap in time
    for sc in ts.CONCURRENT:
        spans = [(th["records"][0]["t0"], th["records"][-1]["t1"]) for th in scen[sc]["threads"]]
        assert sum(1 for a in spans for b in spans if a is not b and a[0] < b[1] and b[0] < a[1]) >= 2, (sc, spans)
    counts = report["job_counts"]
    assert all(counts.get(k, 0) >= ts.T for k in ts.KINDS), counts
