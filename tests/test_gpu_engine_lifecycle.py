"""Creation and destruction of engines (csrc/engine_host_api.h: sumo_create / sumo_destroy; every device buffer of an engine is owned by
it and goes with it): two engines alive on one device do not share anything, destroying one leaves the other's results bit for bit
what a fresh engine gives, destroying nothing or twice is harmless, and a creation that fails on the host (a scene whose lane roles do
not fit, -26) leaves nothing behind that changes the next engine.  16 envs, three env steps at a time; Ant-vs-Ant runs the static-layout
kernel variants, Bug-vs-Spider the runtime-layout ones.  No case provokes a device error."""
import copy
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import capi, mjcf

N, STEPS = 16, 3
HINGE = 3
ANT, MIXED = "RoboSumo-Ant-vs-Ant-v0", "RoboSumo-Bug-vs-Spider-v0"


class Drive:
    """An engine with its env-side buffers, reset with fixed seeds and stepped with fixed actions (step t takes the t-th action block)."""

    def __init__(self, model, cfrc=False):
        self.eng = capi.Engine(model, N)
        if cfrc:
            self.eng.set_cfrc_mode("rne_post")
        self.cfrc = cfrc
        dev, E = torch.device("cuda:0"), self.eng
        self.obs = torch.zeros((N, 2, E.obs_stride), dtype=torch.float32, device=dev)
        self.act = torch.zeros((N, 2, E.act_stride), dtype=torch.float32, device=dev)
        self.info = torch.zeros((N, 2, 8), dtype=torch.float64, device=dev)
        self.done = torch.zeros((N, 2), dtype=torch.uint8, device=dev)
        self.ep_r = torch.zeros(N, dtype=torch.float64, device=dev)
        self.ep_dr = torch.zeros(N, dtype=torch.float64, device=dev)
        self.ep_l = torch.zeros(N, dtype=torch.int32, device=dev)
        self.actions = np.random.default_rng(7).standard_normal((2 * STEPS, N, 2, E.act_stride)).astype(np.float32)
        self.t = 0
        E.reset(self.obs.data_ptr(), seeds=np.arange(N, dtype=np.uint64) + 100)
        torch.cuda.synchronize()

    def steps(self, n=STEPS):
        """-> per step: every array a step writes, the env states after it and (rne_post) the contact forces."""
        out = []
        for _ in range(n):
            self.act.copy_(torch.from_numpy(self.actions[self.t]))
            self.t += 1
            self.eng.step(self.act.data_ptr(), self.obs.data_ptr(), self.info.data_ptr(), self.done.data_ptr(), self.ep_r.data_ptr(),
                          self.ep_dr.data_ptr(), self.ep_l.data_ptr())
            torch.cuda.synchronize()
            rec = [x.cpu().numpy().copy() for x in (self.obs, self.info, self.done, self.ep_r, self.ep_dr, self.ep_l)]
            rec += list(self.eng.get_state())
            if self.cfrc:
                rec.append(self.eng.get_cfrc_ext())
            out.append(rec)
        return out


def _same(a, b):
    assert len(a) == len(b)
    for t, (ra, rb) in enumerate(zip(a, b)):
        assert len(ra) == len(rb)
        for k, (x, y) in enumerate(zip(ra, rb)):
            assert np.array_equal(x, y), (t, k)


@pytest.mark.parametrize("env_id,layout,cfrc_on", [(ANT, 1, "A"), (MIXED, 0, "B")], ids=["ant-static", "bug-spider-runtime"])
def test_engines_are_independent(env_id, layout, cfrc_on):
    """A and B alive together, one of them in cfrc_mode rne_post (its three buffers are allocated by the switch, not by sumo_create);
    after A is destroyed, B goes on exactly as an engine that never had a neighbour."""
    m = mjcf.load_model(env_id)
    a, b = Drive(m, cfrc=cfrc_on == "A"), Drive(m, cfrc=cfrc_on == "B")
    assert a.eng.static_layout() == layout and b.eng.static_layout() == layout
    assert a.eng.h.value != b.eng.h.value
    first = [a.steps(), b.steps()]
    a.eng.close()
    rest = b.steps()
    fresh = Drive(m, cfrc=b.cfrc)
    want = fresh.steps(2 * STEPS)
    _same(first[1] + rest, want)
    assert np.isfinite(rest[-1][0]).all() and not np.array_equal(rest[-1][6], first[1][-1][6])   # observations finite, qpos moved on
    b.eng.close()
    fresh.eng.close()


def test_destroy_null_and_close_twice():
    assert capi.lib().sumo_destroy(None) == 0
    e = capi.Engine(mjcf.load_model(ANT), N)
    e.close()
    assert e.h is None
    e.close()
    assert e.h is None


def test_failed_creation_leaves_the_next_engine_alone():
    """The over-wide role field of tests/test_lane_roles_cpu.py (2 in the one-bit jt_limited of Ant-vs-Bug's fourth hinge) through
    sumo_create: -26 with that message and no handle; the engine created next steps to what the one before the failure stepped to."""
    m = mjcf.load_model(ANT)
    d = Drive(m)
    before = d.steps()
    d.eng.close()
    bad = copy.deepcopy(mjcf.load_model("RoboSumo-Ant-vs-Bug-v0"))
    j = int(np.flatnonzero(np.asarray(bad.jnt_type) == HINGE)[3])
    bad.tables["jnt_limited"] = np.array(bad.jnt_limited, np.int32)
    bad.tables["jnt_limited"][j] = 2
    blob = bad.to_blob()
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    h = C.c_void_p()
    L = capi.lib()
    assert L.sumo_create(C.cast(buf, C.c_void_p), len(blob), N, 0, C.byref(h)) == -26
    msg = L.sumo_last_error().decode()
    assert "jt_limited = 2 does not fit" in msg and "lane %d" % j in msg, msg
    assert not h.value
    d = Drive(m)
    _same(d.steps(), before)
    d.eng.close()
