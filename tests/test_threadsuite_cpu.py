"""tests/threadsuite.py without a GPU: the job lists are deterministic and meet, from the oracle's results alone, the coverage that
tests/test_gpu_threads.py asserts of a run; the runner, driven through make_executor by a pure-Python executor that answers from the oracle's
results (computed before the threads start: the oracle is never called from two threads), reports a clean run as clean, a planted
cross-delivery on the jobs it hit, an exception on its job while the other threads finish, and a thread past the deadline as hung without
blocking — which is what shows that the GPU test can fail."""
import copy
import threading
import time

import pytest

import threadsuite as ts


@pytest.fixture(scope="module")
def lists():
    return ts.build()


@pytest.fixture(scope="module")
def small():
    """four threads with three decode_all jobs each, all of different frames with different plaintext"""
    c = ts.Corpus()
    names = [n for n in c.names if 2000 <= c.size[n] <= 40000][:12]
    assert len(names) == 12
    out = [[ts.decode_all_job("small/%d/%d" % (t, k), names[3 * t + k], c.pack[names[3 * t + k]], c.size[names[3 * t + k]]) for k in range(3)] for t in range(4)]
    plains = [j.expected[1] for lst in out for j in lst]
    assert all(j.expected[0] == "ok" for lst in out for j in lst) and len(set(plains)) == 12
    return out


class OracleExecutor:
    """answers every job with the oracle's result for it"""

    def __init__(self, jobs_per_thread, thread):
        self.answers = {j.id: j.expected for lst in jobs_per_thread for j in lst}
        self.thread, self.index, self.closed = thread, -1, False

    def run(self, job):
        assert job.expected is None, "an executor never sees what is expected of it"
        self.index += 1
        return copy.deepcopy(self.answers[job.id])

    def close(self):
        self.closed = True


def ran_all(res, jobs_per_thread, but=()):
    for i, (th, lst) in enumerate(zip(res["threads"], jobs_per_thread)):
        if i not in but:
            assert th["done"] and [r["id"] for r in th["records"]] == [j.id for j in lst], i


# ---- the lists ---------------------------------------------------------------------------------------------------------------------------
def test_the_same_seed_gives_the_same_lists(lists):
    again = ts.build(fresh=True)
    assert ts.digest(again) == ts.digest(lists)                      # names, read patterns, digests of inputs and of expected results
    assert [j.id for j in ts.serial_list(again)] == [j.id for j in ts.serial_list(lists)]
    other = ts.own_list(0, ts.random.Random(1), ts.Corpus(), ts.hand_built())
    assert ts.digest({"x": [other]})["x"][0] != ts.digest(lists)["own_contexts"][0]


def test_the_lists_meet_the_coverage_floors_from_the_oracle_alone(lists):
    cov = ts.coverage({sc: [[ts.describe(j) for j in lst] for lst in ls] for sc, ls in lists.items()})
    assert [what for what, holds in ts.floors(cov) if not holds] == [], cov
    assert list(lists) == list(ts.CONCURRENT) and [len(ls) for ls in lists.values()] == [ts.T, 3, ts.T, ts.T + 1]
    # every thread's list decodes at most about 4 MB
    for sc, ls in lists.items():
        for lst in ls:
            assert sum(ts.describe(j)["plaintext"] for j in lst) <= (4 << 20) + (256 << 10), sc
    # own_contexts: every kind but `device` on every thread, the kinds in different rotations
    firsts = [lst[0].kind for lst in lists["own_contexts"]]
    assert len(set(firsts)) == ts.T, firsts
    for lst in lists["own_contexts"]:
        assert set(j.kind for j in lst) == set(ts.KINDS[:-1])
        assert sorted(set(j.inputs["mode"] for j in lst if j.kind == "stream")) == list(range(len(ts.MODES)))
    # every stream is a slice source with one copy thread's worth of inputs; an abandoned one stops in front of the frame's end
    for sc, ls in lists.items():
        for lst in ls:
            for j in lst:
                if j.kind == "stream_abandoned":
                    assert j.inputs["mode"] == ts.PIPE and j.inputs["end"] is None and sum(j.inputs["reads"]) < j.inputs["plaintext"] // 3
                    assert sum(n for n, _ in j.expected["reads"]) == sum(j.inputs["reads"])
                if j.kind == "stream" and j.inputs["end"] == "full":
                    assert j.expected["reads"][-1] == (0, b"") and j.expected["end"][0] is True and j.expected["end"][5] == len(j.inputs["z"]) - len(ts.TAIL)


def test_moved_never_has_an_object_in_two_calls_and_destroys_off_thread(lists):
    m = lists["moved"]
    assert m[0][0].kind == "moved_create" and all(j.kind != "moved_create" for lst in m for j in lst[1:])
    steps = [[j for j in lst if j.kind == "moved_step"] for lst in m]
    assert [len(s) for s in steps] == [ts.MOVED_STEPS] * 3
    before = None
    for s in range(ts.MOVED_STEPS):
        groups = [steps[i][s].inputs["group"] for i in range(3)]
        assert sorted(groups) == [0, 1, 2], (s, groups)                # no group in two calls at once
        if before:
            assert all(a != b for a, b in zip(groups, before))         # every call from another thread than the one before
        before = groups
    closes = [[j for j in lst if j.kind == "moved_close"] for lst in m]
    assert [len(c) for c in closes] == [1, 1, 1] and closes[0][0].inputs["groups"] == []     # thread 0 made them: it destroys none
    assert sorted(closes[1][0].inputs["groups"] + closes[2][0].inputs["groups"]) == [0, 1, 2]
    # the groups are mid-frame when they are destroyed: the oracle's decoder is not finished behind the last step
    assert all(j.expected["blocks"][0] == 0 and j.expected["blocks"][2] is False for s in steps for j in s)


def test_churn_releases_the_caches_between_two_rounds_of_closed_streams(lists):
    for t, lst in enumerate(lists["churn"]):
        kinds = [j.kind for j in lst]
        at = kinds.index("release_caches")
        assert kinds.count("release_caches") == 1 and 0 < at < len(kinds) - 1
        want = "stream_abandoned" if t < 2 else "stream"
        assert set(kinds[:at]) == set(kinds[at + 1:]) == {want} and all(j.inputs["mode"] == ts.PIPE for j in lst if j.kind == want)


def test_the_serial_list_holds_every_job_once(lists):
    ids = [j.id for j in ts.serial_list(lists)]
    assert sorted(ids) == sorted(j.id for ls in lists.values() for lst in ls for j in lst) and len(set(ids)) == len(ids)


def test_diff_names_the_place():
    assert ts.diff(("ok", b"abcd"), ("ok", b"abcd")) is None and ts.diff([1, (2, 3)], (1, [2, 3])) is None
    assert ts.diff(("ok", b"abcd"), ("ok", b"abXd")) == "result[1]: bytes differ at 2 (4 bytes, expected 4)"
    assert ts.diff(("ok", b"abcd"), ("ok", b"abc")) == "result[1]: bytes differ at 3 (3 bytes, expected 4)"
    assert ts.diff({"reads": [(1, b"a")], "end": (True, 5)}, {"reads": [(1, b"a")]}) == "result: no 'end'"
    assert ts.diff({"reads": [(1, b"a")]}, {"reads": [(1, b"a")], "end": 1}) is None        # (what is expected decides what is compared)
    assert "92, expected 10" in ts.diff(("err", 10), ("err", 92)) and ts.HIP_ERROR.search(ts.diff(("err", 10), ("err", 92)))
    assert not ts.HIP_ERROR.search(ts.diff(("err", 10), ("err", 192)))
    assert ts.leaves_of({"a": [("err", 10), (5, b"x")], "b": ("init", 7)}) == [10, 7]


# ---- the runner ----------------------------------------------------------------------------------------------------------------------------
def test_a_clean_run_is_reported_clean(lists):
    jobs = lists["own_contexts"]
    made = []

    def make(i):
        made.append((i, threading.get_ident()))
        return OracleExecutor(jobs, i)
    res = ts.run("own_contexts", ts.T, jobs, 30, make)
    assert res["hung"] == [] and ts.failures(res) == [] and res["scenario"] == "own_contexts" and res["wall_s"] <= res["deadline_s"] == 30
    ran_all(res, jobs)
    assert len(set(t for _, t in made)) == ts.T and threading.get_ident() not in [t for _, t in made]   # every executor is made inside its thread
    assert all(r["t0"] <= r["t1"] for th in res["threads"] for r in th["records"])


def test_a_planted_cross_delivery_is_reported_on_the_job_it_hit(small):
    """threads 1 and 2 write job 1's bytes into ONE bytearray and read them back in a fixed order: thread 1 gets thread 2's bytes"""
    out, turn = bytearray(), threading.Barrier(2)

    class SharedOutput(OracleExecutor):
        def run(self, job):
            got = super().run(job)
            if self.index != 1 or self.thread not in (1, 2):
                return got
            if self.thread == 2:
                turn.wait(10)
            out[:] = got[1]
            if self.thread == 1:
                turn.wait(10)
            turn.wait(10)
            return ("ok", bytes(out))
    res = ts.run("planted", 4, small, 30, lambda i: SharedOutput(small, i))
    bad = ts.failures(res)
    assert [(i, r["id"], r["verdict"]) for i, r in bad] == [(1, "small/1/1", "mismatch")], bad
    assert bad[0][1]["detail"].startswith("result[1]: bytes differ at ") and bad[0][1]["name"] == small[1][1].inputs["name"]
    ran_all(res, small)
    assert res["hung"] == []


def test_an_exception_is_recorded_and_the_other_threads_finish(small):
    class Raises(OracleExecutor):
        def run(self, job):
            got = super().run(job)
            if (self.thread, self.index) == (2, 1):
                raise RuntimeError("planted")
            return got
    res = ts.run("raises", 4, small, 30, lambda i: Raises(small, i))
    assert [(i, r["id"], r["verdict"], r["detail"]) for i, r in ts.failures(res)] == [(2, "small/2/1", "exception", "RuntimeError: planted")]
    ran_all(res, small)                                               # thread 2 went on with its next job as well

    def make(i):
        if i == 3:
            raise RuntimeError("no context")
        return OracleExecutor(small, i)
    res = ts.run("no_executor", 4, small, 30, make)
    assert [(i, r["kind"], r["verdict"]) for i, r in ts.failures(res)] == [(3, "executor", "exception")] and res["hung"] == []
    ran_all(res, small, but=(3,))


def test_a_thread_past_the_deadline_is_named_and_the_call_returns(small):
    release = threading.Event()

    class Sleeps(OracleExecutor):
        def run(self, job):
            got = super().run(job)
            if (self.thread, self.index) == (3, 0):
                release.wait(60)
            return got
    t0 = time.monotonic()
    try:
        res = ts.run("sleeps", 4, small, 0.5, lambda i: Sleeps(small, i))
        took = time.monotonic() - t0
        assert res["hung"] == [3] and 0.5 <= took < 5, (res["hung"], took)
        assert not res["threads"][3]["done"] and res["threads"][3]["records"] == []
        ran_all(res, small, but=(3,))
        assert ts.failures(res) == []
    finally:
        release.set()


def test_executors_reach_the_main_thread_while_it_joins(lists):
    """what churn's release_caches job relies on: all threads wait, ONE call runs on the main thread, all threads go on"""
    jobs = lists["churn"]
    sh = ts.Shared("churn", ts.T)
    order = []

    class Churn(OracleExecutor):
        def run(self, job):
            got = super().run(job)
            if job.kind == "release_caches":
                if sh.barrier.wait(10) == 0:
                    sh.on_main(lambda: sh.released.append(threading.current_thread() is threading.main_thread()))
                sh.barrier.wait(10)
            order.append((job.kind, len(sh.released)))
            return got

    def make(i):
        return Churn(jobs, i)
    make.main_calls = sh.main_calls
    res = ts.run("churn", ts.T, jobs, 30, make)
    assert ts.failures(res) == [] and res["hung"] == [] and sh.released == [True]
    ran_all(res, jobs)
    first = order.index(("release_caches", 1))
    assert all(n == 0 for _, n in order[:first]) and all(n == 1 for _, n in order[first:])      # nothing of round 2 ran before the release
