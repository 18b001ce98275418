"""Host thread budget (robosumo_selfplay_amd/hostcfg.py): the cgroup CPU quota is what the pools must be sized by, not os.cpu_count()
(the cause of the bimodal short bench window of round 1: DESIGN.md §4, bench reproducibility)."""
import builtins
import io
import os

from robosumo_selfplay_amd import hostcfg


def _fake_open(files):
    real = builtins.open

    def f(path, *a, **k):
        if path in files:
            if files[path] is None:
                raise OSError(path)
            return io.StringIO(files[path])
        return real(path, *a, **k)
    return f


def test_cpu_quota_reads_cgroup_v2_and_v1(monkeypatch):
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(256)), raising=False)
    monkeypatch.setattr(builtins, "open", _fake_open({"/sys/fs/cgroup/cpu.max": "1600000 100000\n"}))
    assert hostcfg.cpu_quota() == 16
    monkeypatch.setattr(builtins, "open", _fake_open({"/sys/fs/cgroup/cpu.max": "max 100000\n"}))
    assert hostcfg.cpu_quota() == 256
    monkeypatch.setattr(builtins, "open", _fake_open({"/sys/fs/cgroup/cpu.max": None, "/sys/fs/cgroup/cpu/cpu.cfs_quota_us": "800000\n",
                                                       "/sys/fs/cgroup/cpu/cpu.cfs_period_us": "100000\n"}))
    assert hostcfg.cpu_quota() == 8
    monkeypatch.setattr(builtins, "open", _fake_open({"/sys/fs/cgroup/cpu.max": "50000 100000\n"}))
    assert hostcfg.cpu_quota() == 1                                      # never below one
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(4)), raising=False)
    monkeypatch.setattr(builtins, "open", _fake_open({"/sys/fs/cgroup/cpu.max": "1600000 100000\n"}))
    assert hostcfg.cpu_quota() == 4                                      # the affinity mask caps it too


def test_apply_caps_pools_and_respects_overrides(monkeypatch):
    for v in hostcfg._VARS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.delenv("SUMO_HOST_THREADS", raising=False)
    monkeypatch.delenv("LOCAL_WORLD_SIZE", raising=False)
    monkeypatch.setattr(hostcfg, "_applied", None)
    monkeypatch.setattr(hostcfg, "cpu_quota", lambda: 16)
    assert hostcfg.apply() == 8 and os.environ["OMP_NUM_THREADS"] == "8" and os.environ["OPENBLAS_NUM_THREADS"] == "8"
    assert hostcfg.apply() == 8                                           # idempotent
    monkeypatch.setattr(hostcfg, "_applied", None)
    for v in hostcfg._VARS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "4")                           # four ranks share the node's quota
    assert hostcfg.apply() == 2 and os.environ["OPENBLAS_NUM_THREADS"] == "2"
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "64")
    monkeypatch.setattr(hostcfg, "_applied", None)
    assert hostcfg.apply() == 1                                           # never below one
    monkeypatch.delenv("LOCAL_WORLD_SIZE", raising=False)
    monkeypatch.setattr(hostcfg, "_applied", None)
    monkeypatch.setenv("SUMO_HOST_THREADS", "0")
    assert hostcfg.apply() == 0                                           # opt-out
    monkeypatch.setattr(hostcfg, "_applied", None)
    monkeypatch.setenv("SUMO_HOST_THREADS", "3")
    monkeypatch.setenv("OMP_NUM_THREADS", "5")                            # a user's own setting is not overridden
    assert hostcfg.apply() == 3 and os.environ["OMP_NUM_THREADS"] == "5"


def test_throttle_stats_parses_cpu_stat(monkeypatch):
    monkeypatch.setattr(builtins, "open", _fake_open({"/sys/fs/cgroup/cpu.stat": "usage_usec 10\nnr_periods 5\nnr_throttled 3\nthrottled_usec 12345\n"}))
    assert hostcfg.throttle_stats() == (3, 12345)
    monkeypatch.setattr(builtins, "open", _fake_open({"/sys/fs/cgroup/cpu.stat": None}))
    assert hostcfg.throttle_stats() is None


def test_gc_paused_restores_collector_state():
    import gc
    from robosumo_selfplay_amd import hostcfg
    assert gc.isenabled()
    with hostcfg.gc_paused():
        assert not gc.isenabled()
        with hostcfg.gc_paused():                 # nested (a capture inside a paused region) keeps it off
            assert not gc.isenabled()
        assert not gc.isenabled()
    assert gc.isenabled()
    gc.disable()
    try:
        with hostcfg.gc_paused():
            pass
        assert not gc.isenabled()                 # was off before: stays off
    finally:
        gc.enable()


def test_drop_graphs_refuses_inside_a_capture_block():
    """A captured HIP graph destroyed while a stream is capturing aborts the process: the release path raises instead."""
    import pytest
    from robosumo_selfplay_amd import hostcfg
    graphs = {"k": object()}
    assert not hostcfg.capturing()
    with hostcfg.gc_paused():
        assert hostcfg.capturing()
        with pytest.raises(RuntimeError, match="graph capture is open"):
            hostcfg.drop_graphs(graphs)
        assert graphs                              # nothing was released
    assert not hostcfg.capturing()
    hostcfg.drop_graphs(graphs)
    assert not graphs


class _StandInCuda(object):
    """What ``GraphCache.capture`` uses of ``torch.cuda``, recording the order of the calls instead of touching a device."""

    def __init__(self):
        self.log, self.cur = [], "main"

    class _Stream(object):
        def __init__(self, owner, name):
            self.owner, self.name = owner, name

        def wait_stream(self, other):
            self.owner.log.append("%s waits for %s" % (self.name, other.name))

    class _Block(object):
        def __init__(self, owner, enter, leave, stream=None):
            self.owner, self.enter, self.leave, self.stream = owner, enter, leave, stream

        def __enter__(self):
            self.owner.log.append(self.enter)
            if self.stream:
                self.prev, self.owner.cur = self.owner.cur, self.stream

        def __exit__(self, *exc):
            self.owner.log.append(self.leave)
            if self.stream:
                self.owner.cur = self.prev
            return False

    def Stream(self, device=None):
        return self._Stream(self, "side")

    def current_stream(self, device=None):
        return self._Stream(self, self.cur)

    def stream(self, s):
        return self._Block(self, "on side", "off side", stream=s.name)

    def synchronize(self, device=None):
        self.log.append("synchronize")

    def CUDAGraph(self):
        return object()

    def graph(self, graph, **kwargs):
        return self._Block(self, "capture begins %r" % (sorted(kwargs.items()),), "capture ends")


def test_graph_cache_policy_without_a_device():
    """``hostcfg.GraphCache``: at most two records, a third key drops all of them; the step's launches run once as a warm-up on a side
    stream outside the capture and once inside it with the collector paused; a failing body drops the records, switches the caller's
    graph path off, warns once and yields None; records are never released while a capture is open."""
    import gc
    import warnings
    import pytest
    from robosumo_selfplay_amd import hostcfg
    cuda = _StandInCuda()
    cache = hostcfg.GraphCache("PPO", "dev0", cuda=cuda)
    failed, seen = [], []

    def body(rec):
        seen.append((cuda.cur, hostcfg.capturing(), gc.isenabled()))
        cuda.log.append("body of %s" % rec["name"])

    rec = cache.capture("a", lambda: dict(name="a"), body, lambda: failed.append(1), capture_error_mode="thread_local")
    assert rec is cache.get("a") and rec["name"] == "a" and rec["graph"] is not None and not failed
    assert seen == [("side", False, True), ("main", True, False)]            # warm-up outside the capture, capture with the collector off
    assert cuda.log == ["side waits for main", "on side", "body of a", "off side", "main waits for side", "synchronize",
                        "capture begins [('capture_error_mode', 'thread_local')]", "body of a", "capture ends"]
    assert gc.isenabled() and not hostcfg.capturing()
    assert cache.capture("b", lambda: dict(name="b"), body, lambda: failed.append(1)) is cache["b"]
    assert len(cache) == 2 and sorted(cache) == ["a", "b"]
    cache.capture("c", lambda: dict(name="c"), body, lambda: failed.append(1))    # a third key drops ALL records first
    assert sorted(cache) == ["c"] and cache.get("a") is None

    # records are not released while a capture is open: neither by clear() nor by a capture that would have to make room
    cache.capture("d", lambda: dict(name="d"), body, lambda: failed.append(1))
    with hostcfg.gc_paused():
        with pytest.raises(RuntimeError, match="graph capture is open"):
            cache.clear()
        with pytest.raises(RuntimeError, match="graph capture is open"):
            hostcfg.drop_graphs(cache)
        with pytest.raises(RuntimeError, match="graph capture is open"):
            cache.capture("e", lambda: dict(name="e"), body, lambda: failed.append(1))
    assert sorted(cache) == ["c", "d"] and not failed

    # a failing body (here: inside the capture block) drops the records, calls on_fail, warns once with the caller's noun, returns None
    calls = []

    def bad_body(rec):
        calls.append(hostcfg.capturing())
        if hostcfg.capturing():
            raise RuntimeError("operation not permitted when stream is capturing")

    one = hostcfg.GraphCache("recurrent PPO", "dev0", cuda=cuda)
    one.capture("k", lambda: dict(name="k"), body, lambda: failed.append(1))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert one.capture("x", lambda: dict(name="x"), bad_body, lambda: failed.append("x")) is None
    assert calls == [False, True] and failed == ["x"] and len(one) == 0
    assert len(w) == 1 and "HIP graph capture of the recurrent PPO step failed" in str(w[0].message)
    assert "not permitted" in str(w[0].message) and str(w[0].message).endswith("using eager launches")
    assert gc.isenabled() and not hostcfg.capturing()                           # the failed capture left nothing open
    one.clear()
    cache.clear()
    assert len(cache) == 0
