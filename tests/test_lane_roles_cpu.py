"""The two packed role words a lane keeps in registers (csrc/sumo_engine.hip: LaneRec::role0 / role1, built by build_lane_roles of
csrc/engine_host_scene.h): every field, for all 64 lanes of all nine scenes, against the same quantity recomputed here from the
compiled model; the chain elements the tree-shaped velocity pass derives from the words against the model's dof_parentid walk; and
a value that does not fit its field must fail creation instead of being truncated.  Host only: sumo_debug_lane_roles touches no
device."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from robosumo_selfplay_amd import build, mjcf

FREE, HINGE = 0, 3
NAMES = ("Ant", "Bug", "Spider")
ENV_IDS = ["RoboSumo-%s-vs-%s-v0" % (a, b) for a in NAMES for b in NAMES]
_SRC = os.path.join(ROOT, "robosumo_selfplay_amd", "csrc", "sumo_engine.hip")


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(build.build_all()[0])
    L.sumo_debug_lane_roles.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    L.sumo_debug_layout.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    L.sumo_last_error.restype = C.c_char_p
    return L


@pytest.fixture(scope="module")
def fields():
    """{name: (word, first bit, width)} from the ROLE0_* / ROLE1_* definitions of the engine source."""
    f = {m.group(2): (int(m.group(1)), int(m.group(3)), int(m.group(4)))
         for m in re.finditer(r"^#define ROLE([01])_(\w+) (\d+), (\d+)$", open(_SRC).read(), flags=re.M)}
    assert len(f) == 18
    used = [0, 0]
    for w, lo, n in f.values():          # the fields tile the two words without overlap
        mask = ((1 << n) - 1) << lo
        assert mask < (1 << 32) and not used[w] & mask
        used[w] |= mask
    return f


def _roles(lib, model):
    blob = model.to_blob()
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    out = (C.c_uint32 * 128)()
    n = lib.sumo_debug_lane_roles(C.cast(buf, C.c_void_p), len(blob), out, 128)
    return n, np.array(out, dtype=np.uint64).reshape(64, 2)


def _tree_ok(lib, model):
    src = open(_SRC).read()
    body = src[src.index("struct Layout {"):]
    body = re.sub(r"//[^\n]*", "", body[body.index("{") + 1:body.index("};")])
    names = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip()[4:].split(",")]
    blob = model.to_blob()
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    out = (C.c_int32 * 256)()
    n = lib.sumo_debug_layout(C.cast(buf, C.c_void_p), len(blob), out, 256)
    assert n == len(names)
    return bool(out[names.index("tree_ok")])


def _expected(m):
    """Per-lane integer roles from the compiled model alone (the effective tree folds jointless inner bodies into their parents)."""
    nb, nv, njnt = m.nbody, m.nv, m.njnt
    tpar = [int(x) for x in m.body_parentid]
    jntnum, jntadr = m.body_jntnum, m.body_jntadr
    par = [0] * nb
    for b in range(1, nb):
        p = tpar[b]
        while p != 0 and jntnum[p] == 0:
            p = tpar[p]
        par[b] = p
    depth = [0] * nb
    for b in range(1, nb):
        depth[b] = depth[par[b]] + 1
    stub = [b >= 1 and jntnum[b] == 0 and par[b] != 0 and not any(par[c] == b for c in range(1, nb) if c != b) for b in range(nb)]
    chains = {}
    for b in range(1, nb):
        bb = b
        while bb and m.body_dofnum[bb] == 0:
            bb = tpar[bb]
        dc = []
        if bb:
            d = int(m.body_dofadr[bb] + m.body_dofnum[bb] - 1)
            while d >= 0:
                dc.insert(0, d)
                d = int(m.dof_parentid[d])
        chains[b] = dc
    agent = [0] * nb
    for a in range(m.nagent):
        for b in range(int(m.agent_bodyadr[a]), int(m.agent_bodyadr[a] + m.agent_nbody[a])):
            agent[b] = a
    hinge_index = {}
    for j in range(njnt):
        if m.jnt_type[j] == HINGE:
            hinge_index[j] = len(hinge_index)
    rows = []
    for l in range(64):
        e = dict(level=-1, agent=0, isfree=0, hinge=0, parent=0, nchild=0, chain_len=0, bchain_len=0, qadr=0, ldof=0,
                 d_hid=-1, d_pos=0, d_body=0, jt_hinge=0, jt_limited=0, jt_agent=0, jt_body=0, jt_nfree=0)
        if l < nb:
            b = l
            e["level"] = depth[b]
            if b >= 1:
                e["agent"], e["parent"] = agent[b], par[b]
                e["nchild"] = sum(1 for c in range(b + 1, nb) if par[c] == b and not stub[c])
                k, n = b, 0
                while k != 0:
                    k, n = par[k], n + 1
                e["bchain_len"], e["chain_len"] = n, len(chains[b])
                e["ldof"] = chains[b][-1] if chains[b] else 0
            if jntnum[b] == 1:
                j = int(jntadr[b])
                e["isfree"], e["hinge"], e["qadr"] = int(m.jnt_type[j] == FREE), int(m.jnt_type[j] == HINGE), int(m.jnt_qposadr[j])
        if l < nv:
            b = int(m.dof_bodyid[l])
            e["d_body"], e["d_pos"] = b, chains[b].index(l)
            e["d_hid"] = hinge_index.get(int(m.dof_jntid[l]), -1)
        if l < njnt:
            b = int(m.jnt_bodyid[l])
            e.update(jt_hinge=int(m.jnt_type[l] == HINGE), jt_limited=int(m.jnt_limited[l]), jt_agent=agent[b], jt_body=b,
                     jt_nfree=sum(1 for j in range(l) if m.jnt_type[j] == FREE))
        rows.append(e)
    return rows, chains


def _unpack(fields, words):
    g = lambda name: int((int(words[fields[name][0]]) >> fields[name][1]) & ((1 << fields[name][2]) - 1))
    return dict(level=g("LEVEL1") - 1, agent=g("AGENT"), isfree=g("ISFREE"), hinge=g("HINGE"), parent=g("PARENT"), nchild=g("NCHILD"),
                chain_len=g("CHAIN_LEN"), bchain_len=g("BCHAIN_LEN"), qadr=g("QADR"), ldof=g("LDOF"), d_hid=g("HID1") - 1,
                d_pos=g("DPOS"), d_body=g("DBODY"), jt_hinge=g("JT_HINGE"), jt_limited=g("JT_LIMITED"), jt_agent=g("JT_AGENT"),
                jt_body=g("JT_BODY"), jt_nfree=g("JT_NFREE"))


@pytest.mark.parametrize("env_id", ENV_IDS)
def test_every_field_of_every_lane(lib, fields, env_id):
    m = mjcf.load_model(env_id)
    assert m.nbody <= 64 and m.nv <= 44
    n, words = _roles(lib, m)
    assert n == 128, lib.sumo_last_error()
    want, chains = _expected(m)
    for l in range(64):
        got = _unpack(fields, words[l])
        assert got == want[l], (env_id, l, {k: (got[k], want[l][k]) for k in got if got[k] != want[l][k]})
        if l < m.njnt:   # what the kernels derive from the number of free joints before the joint (6 dofs / 7 qpos against 1 / 1)
            f = got["jt_nfree"]
            assert l + 5 * f == m.jnt_dofadr[l] and l + 6 * f == m.jnt_qposadr[l], (env_id, l)
            if got["jt_hinge"]:
                assert l - f == sum(1 for j in range(l) if m.jnt_type[j] == HINGE), (env_id, l)
    # the tree-shaped velocity pass takes its chain from the words: root dofs B .. B + 5, then the chain's last dof (hip), or the
    # one before it and the last (hip, ankle); the body owns the root dofs if its joint is free, the last dof if it is a hinge
    assert _tree_ok(lib, m), env_id
    d1 = int(m.agent_dofadr[1])
    for b in range(1, m.nbody):
        r = _unpack(fields, words[b])
        ln, ld, B = r["chain_len"], r["ldof"], d1 if r["agent"] else 0
        derived = [B + p for p in range(6)] + ([ld] if ln == 7 else [ld - 1, ld] if ln == 8 else [])
        assert derived == chains[b], (env_id, b)
        own = [bool(r["isfree"]) if p < 6 else bool(r["hinge"]) and p == ln - 1 for p in range(ln)]
        assert own == [int(m.dof_bodyid[d]) == b for d in chains[b]], (env_id, b)


def test_a_value_past_its_field_fails_creation(lib):
    """jt_limited has one bit: a model whose table carries 2 there must be refused with a message, not packed as 0."""
    m = copy.deepcopy(mjcf.load_model("RoboSumo-Ant-vs-Bug-v0"))
    j = int(np.flatnonzero(np.asarray(m.jnt_type) == HINGE)[3])
    m.tables["jnt_limited"] = np.array(m.jnt_limited, np.int32)
    m.tables["jnt_limited"][j] = 2
    n, _ = _roles(lib, m)
    assert n == -26
    msg = lib.sumo_last_error().decode()
    assert "jt_limited = 2 does not fit" in msg and "lane %d" % j in msg, msg
