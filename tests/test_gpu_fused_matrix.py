"""Every fused-launch kernel the Python API can reach (tests/fused_matrix.py ``cases()``: 5 same-species variants x 17 policies and the
co-training launch on the six mixed scenes) against the step-by-step definition of its mode, bit for bit, at the smallest shapes at
which these kernels can still go wrong.  The per-feature tests hold each mode on the scenes its author had at
hand; here one parametrised test runs the same comparison on every ``sumo_rollout_kernel<NV, POLICY, SL>`` instantiation.

Builders and comparison helpers are those of the feature tests (test_gpu_zoo_league, test_gpu_matches_cross, test_gpu_pair_fused,
zoo_lstm_helpers.golden); where they are written for Ant, :func:`_species` points their module constants at the variant's scene.

Shapes.  Rollout modes: T = 6 in launches of 3 steps (``SUMO_ROLLOUT_CHUNK=3``: the second launch starts at s0 = 3), two consecutive
``run()`` calls (carried-over recurrent / zoo state, the second noise buffer).  Match modes: two launches of K = 6, quota 2, stochastic
actions.  N = 40 envs: two whole 16-env tiles and a partial one of 8.  N = 48 where the mode selects a table row per whole tile:

    an LSTM opponent pool      opponent_pool.py  ``if num_envs % 16: raise ValueError("an LSTM opponent pool needs num_envs to be a multiple of 16 ...")``
    a league                   policy_zoo.py     ``if nenvs < LEAGUE_TILE or nenvs % LEAGUE_TILE: raise ValueError("a league deals its %d members over tiles ...")``
    LSTM learner vs a zoo net  runner.py         ``ok = ... and (not lstm or grid())`` -- off the grid the launch does not apply; the engine:
                               ``FAIL(-11, "a %s per 16-env tile needs env_offset (%d) and the env count (%d) to be multiples of 16", ...)``

N = 64 for the co-training launch (co_train.tile_halves: "num_envs = %d is not a multiple of %d", 32).  No case had to be enlarged
beyond these.  Every episode counter starts so close to the time limit that envs end and auto-reset inside every launch window.

Asserted in every case, so that an empty comparison cannot pass: the fused path applied (``rollout_mode()`` / the pairing record's
entry / the counted ``rollout_steps_pair_group`` calls) and names the row's entry; ``engine.static_layout()`` and nv are the variant's;
``rollout_aborts == 0``; an episode ended inside the window; league: both families were dealt a tile; policy 16: both sides recorded
rows; policy 15: agent 1's done flag masks the learner's shadow state in at least one recorded row and keeps it in at least one."""
import numpy as np
import pytest

import fused_matrix as FM
from conftest import has_gpu

pytestmark = pytest.mark.gpu

T, CHUNK, POOL = 6, 3, 3
K, QUOTA, LAUNCHES = 6, 2, 2
CASES = FM.cases()


def _species(monkeypatch, L, D, A, N):
    """The Ant constants of tests/test_gpu_zoo_league.py, read by its learner builders, set to the variant's scene for this test."""
    for name, value in (("D", D), ("A", A), ("N", N)):
        monkeypatch.setattr(L, name, value)
    assert L.T == T and L.CHUNK == CHUNK


def _layout_env(monkeypatch, v):
    if v.layout_env is None:
        monkeypatch.delenv("SUMO_STATIC_LAYOUT", raising=False)
    else:
        monkeypatch.setenv("SUMO_STATIC_LAYOUT", v.layout_env)


def _check_variant(env, v):
    for E in env.engines:
        assert E.static_layout() == v.static and E.nv == v.nv, (v.key, E.static_layout(), E.nv)


def _same(L, x, y, what):
    if x is None or y is None:
        assert x is None and y is None, what
    else:
        assert L._bytes_equal(x, y), what


def _env_side(env):
    """The device buffers and the engine state every mode leaves behind."""
    import torch
    torch.cuda.synchronize()
    out = [("obs_dev", env.obs_dev.clone()), ("info_dev", env.info_dev.clone()), ("done_dev", env.done_dev.clone()), ("act_dev", env.act_dev.clone())]
    for g, E in enumerate(env.engines):
        out += [("%s[%d]" % (n, g), x) for n, x in zip(("qpos", "qvel", "warm", "counters"), E.get_state())]
    return out


# ---- rollout modes: a Runner, as tools/runner_mode_digest.py builds every mode --------------------------------------------------
def _rollout(case, fused, monkeypatch):
    import torch
    import test_gpu_zoo_league as L
    from zoo_lstm_helpers import golden
    from robosumo_selfplay_amd import opponent_pool, policy_zoo
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    v, N = case.variant, case.num_envs
    _, learner, opponent = case.builder.split(":")
    monkeypatch.setenv("SUMO_ROLLOUT_CHUNK", str(CHUNK))
    env = SumoVecEnv(v.env_id, num_envs=N, seed=11)
    _check_variant(env, v)
    D, A = env.observation_space[0].shape[0], env.action_space[0].shape[0]
    _species(monkeypatch, L, D, A, N)
    make = (lambda seed: L._lstm_learner(seed, 128)) if learner == "lstm" else L._mlp_learner
    models = [make(5), make(6)]
    for k, m in enumerate(models):
        m.act_model.seed(101 + k)
    r = Runner(env=env, models=models, nsteps=T, nagent=2, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0, anneal_bound=500)
    zoo = None
    sp = v.species[0]
    if opponent == "pool":        # LSTM learners only: an MLP pool plays in the fused launch alone ("a per-env opponent pool needs the fused rollout path")
        pool = opponent_pool.LstmOpponentPool(models[0].spec, POOL, N, env.device)
        for k in range(POOL):
            pool.set_snapshot(k, make(7 + k).act_model.params)
        pool.assign(np.arange(N // 16) % POOL)                        # every snapshot plays a tile
        pool.seed(102)
        r.models[1] = pool
    elif opponent == "reuse":
        r.reuse_opponent = True
    elif opponent != "self":
        if opponent == "league":
            nets = [policy_zoo.load_zoo_policy_from_flat(golden("%s-%s-v3" % (sp, fam)), A) for fam in ("mlp", "lstm")]
            zoo = policy_zoo.ZooLeague(nets, N, env.device)
            dealt = {zoo.kinds[m] for m in zoo.tile_member}
            assert dealt == {"mlp", "lstm"}, "a family of the league was dealt no tile"
        else:
            zoo = policy_zoo.load_zoo_policy_from_flat(golden("%s-%s-v3" % (sp, opponent[len("zoo_"):])), A)
        zoo.seed(202)
        r.models[1] = policy_zoo.FixedOpponentModel(zoo)
    r.fused_fix_opponent = True
    r.fused_rollout = fused
    assert r.rollout_chunk == CHUNK
    mode = r.rollout_mode()
    assert mode.fused == fused, (case.id, mode)
    assert "sumo_" + mode.launch.entry[:-len("_group")] == case.entry
    if fused:
        assert mode.entry == mode.launch.entry
    L._near_time_limit(env)
    calls = []
    for k in range(2):
        out = r.run(250 + k)
        torch.cuda.synchronize()
        rec = [(L.NAMES[i], x) for i, x in enumerate(out)] + _env_side(env)
        rec += [("states[0]", r.states[0].clone() if torch.is_tensor(r.states[0]) else None),
                ("shadow_state", None if r.shadow_state is None else r.shadow_state.clone()),
                ("zoo_state", (zoo.state if isinstance(zoo, policy_zoo.ZooLeague) else r.zoo_state).clone()),
                ("league_scores", r.league_scores)]
        calls.append(rec)
    aborts = env.stats()["rollout_aborts"]
    env.close()
    return calls, aborts


def _run_rollout_case(case, monkeypatch):
    import torch
    import test_gpu_zoo_league as L
    f, f_aborts = _rollout(case, True, monkeypatch)
    s, s_aborts = _rollout(case, False, monkeypatch)
    assert f_aborts == 0 and s_aborts == 0
    N = case.num_envs
    for k, (a, b) in enumerate(zip(f, s)):
        assert [n for n, _ in a] == [n for n, _ in b]
        for (name, x), (_, y) in zip(a, b):
            if name == "epinfos":
                assert x == y, (k, name)
            else:
                _same(L, x, y, (k, name))
        out = dict(a)
        masks = out["masks"]
        assert len(out["epinfos"]) > 0 and bool(masks[0].any()) and bool(masks[1].any()), "no episode ended inside the window (call %d)" % k
        for name in ("actions", "values", "neglogpacs", "opp_neglogpacs"):
            assert bool(torch.isfinite(out[name]).all()), (k, name)
    first, last = dict(f[0]), dict(f[1])
    assert not bool(first["masks"][0].reshape(N, T)[:, 1:].any(dim=1).all()), "every env reset in the first call: no state is carried over"
    learner, opponent = case.builder.split(":")[1:]
    if learner == "lstm":
        assert float(last["states[0]"].abs().max()) > 0
    if opponent in ("zoo_lstm", "league"):
        assert float(last["zoo_state"].abs().max()) > 0
    if opponent == "league":
        assert last["league_scores"] is not None and int(np.asarray(last["league_scores"])[:, 0].sum()) == len(last["epinfos"])
        assert (np.asarray(first["league_scores"])[:, 0] > 0).all(), "a member of the league finished no episode"
    if opponent == "reuse":                                           # policy 15: the shadow state is masked by agent 1's done flag
        m1 = first["masks"][1]
        assert bool(m1.any()) and not bool(m1.all()), "agent 1's rows: none masked out, or none kept"
        assert float(last["shadow_state"].abs().max()) > 0


# ---- match modes: a pairing of two tables, as tools/match_pairing_digest.py plays every pairing ---------------------------------
def _tables(env, sp):
    import test_gpu_matches_cross as X
    from zoo_lstm_helpers import golden, synthetic_lstm_flat
    from robosumo_selfplay_amd import policy_zoo
    D, A = X._dims(env)
    np.random.seed(1)                                                 # the MLP builder starts from numpy's global generator
    return dict(mt=X._mlp_table(env), lt=X._lstm_table(env),
                zoo=policy_zoo.ZooTable([golden("%s-mlp-v3" % sp), X._synthetic_zoo_flat(D - 1, A, 21)], A, env.device),
                zl=policy_zoo.ZooLstmTable([golden("%s-lstm-v3" % sp), synthetic_lstm_flat(D - 1, A, 21)], A, env.device))


PAIRINGS = {"mlp": [("mt", "mt")], "lstm": [("lt", "lt")], "zoo": [("mt", "zoo")], "zoo_lstm": [("mt", "zl")], "lstm_zoo_lstm": [("lt", "zl")],
            "cross": [("lt", "mt"), ("mt", "lt")], "lstm_zoo": [("lt", "zoo")]}          # both seatings of the cross launch


def _end_inside_every_launch(envs):
    """Env e runs out of time in its step 1 + e % 12: episodes end in both launches of K = 6, at every step of each."""
    qpos, qvel, warm, cnt = envs[0].engine.get_state()
    cnt[:, 0] = envs[0].model.timestep_limit - 1 - (np.arange(len(cnt)) % (K * LAUNCHES))
    for e in envs:
        e.engine.set_state(qpos, qvel, warm, cnt)


def _run_match_case(case, monkeypatch):
    import torch
    import test_gpu_matches_cross as X
    import test_gpu_zoo_league as L
    from robosumo_selfplay_amd import matches as M
    v, N = case.variant, case.num_envs
    ef, es = X._env(v.env_id, N), X._env(v.env_id, N)
    for e in (ef, es):
        _check_variant(e, v)
    D, A = X._dims(ef)
    tabs = _tables(ef, v.species[0])
    for names in PAIRINGS[case.builder.split(":")[1]]:
        t0, t1 = (tabs[n] for n in names)
        p = M.match_pairing(t0, t1)
        assert "sumo_" + p.entry == case.entry
        M._check_env(ef, t0)
        rng = np.random.default_rng(5)
        idx0, idx1 = (rng.integers(0, t.capacity, N).astype(np.int32) for t in (t0, t1))
        assert idx0.max() == t0.capacity - 1 and idx1.max() == t1.capacity - 1          # the last row of each table plays
        i0, i1 = torch.from_numpy(idx0).cuda(), torch.from_numpy(idx1).cuda()
        for e in (ef, es):
            e._needs_seed = True
            e.reset_device()
        _end_inside_every_launch([ef, es])
        widths = [s.width for s in p.seats]
        stf, sts = ([None if w is None else torch.zeros((N, w), dtype=torch.float32, device="cuda") for w in widths] for _ in range(2))
        cf = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
        e_ = torch.arange(N, device="cuda")
        cf[e_, e_ % 3] = (e_ % 3).to(torch.int32)                    # 0, 1 or 2 games finished before the window: the quota cuts some envs off
        cs, before = cf.clone(), int(cf.sum())
        gen = torch.Generator(device="cuda")
        gen.manual_seed(3)
        for launch in range(LAUNCHES):
            noise = tuple(torch.randn((K, N, A), generator=gen, device="cuda") for _ in range(2))
            M.pairing_steps(ef, p, tuple(stf), i0, i1, cf, QUOTA, K, noise, True)
            M.pairing_steps(es, p, tuple(sts), idx0, idx1, cs, QUOTA, K, noise, False)
            _same(L, cf, cs, (names, launch, "score"))
            for k, (x, y) in enumerate(zip(stf, sts)):
                _same(L, x, y, (names, launch, "state of agent %d" % k))
            for (name, x), (_, y) in zip(_env_side(ef), _env_side(es)):
                _same(L, x, y, (names, launch, name))
            assert ef.stats()["rollout_aborts"] == 0 and es.stats()["rollout_aborts"] == 0
            now = int(cf.sum())
            assert now > before, "no episode ended inside launch %d" % launch
            before = now
        assert int(cf.sum(1).max()) == QUOTA
        for k, x in enumerate(stf):
            assert x is None or float(x.abs().max()) > 0, (names, "state of agent %d never written" % k)
    ef.close(); es.close()


# ---- the co-training launch: a PairRunner, as tests/test_gpu_pair_fused.py compares it ------------------------------------------
def _run_pair_case(case, monkeypatch):
    import test_gpu_pair_fused as P
    import test_gpu_zoo_league as L
    from robosumo_selfplay_amd import co_train
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    v, N = case.variant, case.num_envs
    left, launches = [], []
    close, launch = SumoVecEnv.close, SumoVecEnv.rollout_steps_pair_group

    def closing(self):                                                # P._run closes its env: what it leaves behind is read first
        if not self.closed:
            left.append((self.stats()["rollout_aborts"], _env_side(self)))
        close(self)

    def counted(self, g, ro):
        launches.append((ro.s0, ro.K))
        return launch(self, g, ro)
    monkeypatch.setattr(SumoVecEnv, "close", closing)
    monkeypatch.setattr(SumoVecEnv, "rollout_steps_pair_group", counted)

    def prepare(env):
        _check_variant(env, v)
        L._near_time_limit(env)
    bf, _ = P._assert_launch_equals_steps(v.env_id, N, T, 1, 2, prepare=prepare, rollout_chunk=CHUNK)
    assert launches == [(0, CHUNK), (CHUNK, CHUNK)] * 2 and case.entry == "sumo_rollout_steps_pair"   # the fused runner alone launched
    (fa, fs), (sa, ss) = left
    assert fa == 0 and sa == 0
    for (name, x), (_, y) in zip(fs, ss):
        _same(L, x, y, name)
    assert bool(bf["ep_done"].any()), "no episode ended inside the window"
    for side in range(2):
        own = co_train.own_envs(N, side)
        for k in ("obs", "act", "val", "nlp"):
            assert float(bf["side"][side][k][:, own].abs().sum()) > 0, "side %d recorded no %s rows" % (side, k)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_fused_launch_equals_its_stepwise_path(case, monkeypatch):
    assert has_gpu()
    _layout_env(monkeypatch, case.variant)
    kind = case.builder.split(":")[0]
    {"rollout": _run_rollout_case, "match": _run_match_case, "pair": _run_pair_case}[kind](case, monkeypatch)
