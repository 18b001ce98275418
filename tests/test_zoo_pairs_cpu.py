"""CPU checks of zoo-vs-zoo play (robosumo_selfplay_amd/zoo_pairs.py, zoo_tournament.py, ``ppo_zoo_seat_act`` of include/sumo_ppo.h,
DESIGN.md section 23): the export and its struct mirror, the host refusals of the launch (they return before any device is
touched), how a seat sorts its nets, what it refuses, and the script's path rule."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from robosumo_selfplay_amd import build, mjcf, policy_zoo, ppo_capi, zoo_pairs  # noqa: E402
import zoo_tournament  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = {"ant": (120, 8), "bug": (164, 12), "spider": (208, 16)}
ENV_IDS = ["RoboSumo-%s-vs-%s-v0" % (a, b) for a in ("Ant", "Bug", "Spider") for b in ("Ant", "Bug", "Spider")]


@pytest.fixture(scope="module")
def nets():
    with np.load(os.path.join(HERE, "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
        return {k: z[k].copy() for k in z.files}


# ---- the export ---------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sumo_ppo.h")).read()
    assert re.search(r"\bint\s+ppo_zoo_seat_act\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "ppo_zoo_seat_act" in ppo_capi.EXPORTS
    build.build_all()
    L = C.CDLL(build.lib_path("libsumo_ppo.so"))
    assert hasattr(L, "ppo_zoo_seat_act")


def test_struct_mirror_matches_the_header(tmp_path):
    st, cname = ppo_capi.ZooSeat, "ppo_zoo_seat"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sumo_ppo.h"', 'int main(void) {',
             '  printf("size %%zu\\n", sizeof(%s));' % cname]
    lines += ['  printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f) for f, _ in st._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    table = dict((a, int(v)) for a, v in (ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()))
    assert C.sizeof(st) == table["size"]
    for f, _ in st._fields_:
        assert getattr(st, f).offset == table[f], f
    last = st._fields_[-1][0]
    assert getattr(st, last).offset + getattr(st, last).size == table["size"]      # every field of the header is mirrored
    # the header's own field list, in order
    body = re.search(r"typedef struct ppo_zoo_seat \{(.*?)\} ppo_zoo_seat;", open(os.path.join(ROOT, "include", "sumo_ppo.h")).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"[*\s]([a-z_0-9]+)\s*(?=[,;])", body)
    assert names == [f for f, _ in st._fields_]


# ---- host refusals: every call returns before a device is touched ----------------------------------------------------------------
def _seat(**kw):
    """A well-formed seat on fake (never dereferenced) addresses."""
    z = ppo_capi.ZooSeat()
    z.mlp_params, z.mlp_filt, z.lstm_params, z.lstm_filt, z.tile_entry, z.state = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    z.n_mlp, z.n_lstm, z.ob_dim, z.ac_dim, z.obs_clip, z.forget_bias = 1, 1, 120, 8, 5.0, 1.0
    for k, v in kw.items():
        setattr(z, k, v)
    return z


def _call(seat, obs=0x7000, n=16, obs_stride=128, act=0x8000, act_stride=16):
    L = ppo_capi.lib()
    return L.ppo_zoo_seat_act(C.byref(seat) if seat is not None else None, obs, n, obs_stride, None, 2, None, act, act_stride, None, None)


REFUSED = [
    ("null seat", lambda: _call(None)),
    ("null obs", lambda: _call(_seat(), obs=None)),
    ("null action_out", lambda: _call(_seat(), act=None)),
    ("n below a tile", lambda: _call(_seat(), n=8)),
    ("n zero", lambda: _call(_seat(), n=0)),
    ("n negative", lambda: _call(_seat(), n=-16)),
    ("n off the tile grid", lambda: _call(_seat(), n=40)),
    ("ob_dim 0", lambda: _call(_seat(ob_dim=0))),
    ("ob_dim 513", lambda: _call(_seat(ob_dim=513), obs_stride=600)),
    ("obs_stride below ob_dim", lambda: _call(_seat(), obs_stride=119)),
    ("ac_dim 0", lambda: _call(_seat(ac_dim=0))),
    ("ac_dim 17", lambda: _call(_seat(ac_dim=17), act_stride=32)),
    ("act_stride below ac_dim", lambda: _call(_seat(), act_stride=7)),
    ("no rows", lambda: _call(_seat(n_mlp=0, n_lstm=0))),
    ("negative rows", lambda: _call(_seat(n_mlp=-1, n_lstm=2))),
    ("mlp rows, no params", lambda: _call(_seat(mlp_params=None))),
    ("mlp rows, no filter", lambda: _call(_seat(mlp_filt=None))),
    ("lstm rows, no params", lambda: _call(_seat(lstm_params=None))),
    ("lstm rows, no filter", lambda: _call(_seat(lstm_filt=None))),
    ("lstm rows, no state", lambda: _call(_seat(state=None))),
    ("no tile entries", lambda: _call(_seat(tile_entry=None))),
]


@pytest.mark.parametrize("what,call", REFUSED, ids=[w for w, _ in REFUSED])
def test_bad_arguments_are_refused_on_the_host(what, call):
    rc = call()
    assert rc < 0 and rc != -100, (what, rc)          # -100 is a failed HIP call: the refusals come before any
    assert len(ppo_capi.lib().ppo_last_error()) > 0


# ---- seats ----------------------------------------------------------------------------------------------------------------------
def test_seat_sorts_its_nets_into_families(nets):
    m, l = nets["bug-mlp-v3"], nets["bug-lstm-v3"]
    seat = zoo_pairs.ZooSeat([l, m, l * np.float32(0.5), m * np.float32(0.5), l], 164, 12, device="cpu")
    assert seat.kinds == ["lstm", "mlp", "lstm", "mlp", "lstm"]
    assert (seat.n_mlp, seat.n_lstm, len(seat)) == (2, 3, 5)
    assert seat.entries.tolist() == [2, 0, 3, 1, 4] and seat.entries.dtype == np.int32
    want, n_mlp, n_lstm = policy_zoo.league_entries(seat.kinds)
    assert seat.entries.tolist() == want.tolist() and (n_mlp, n_lstm) == (2, 3)
    assert seat.labels == [None] * 5 and seat.recurrent
    assert tuple(seat.mlp_table.params.shape) == (2, ppo_capi.lib().ppo_param_count(164, 12)) and tuple(seat.mlp_table.filt.shape) == (2, 2, 164)
    assert tuple(seat.lstm_table.params.shape) == (3, 164 * 64 + 64 + 128 * 256 + 256 + 64 * 12 + 12 + 12) and seat.lstm_table.capacity == 3
    # rows keep the order of their family
    assert np.array_equal(seat.mlp_table.params[1].numpy(), policy_zoo.zoo_table_rows([m * np.float32(0.5)], 12)[0][0])
    assert np.array_equal(seat.lstm_table.params[2].numpy(), policy_zoo.zoo_lstm_table_rows([l], 12)[0][0])
    z = seat.struct(seat.mlp_table.params, seat.new_state(16))       # (any tensor stands in for the tile entries here)
    assert (z.n_mlp, z.n_lstm, z.ob_dim, z.ac_dim, z.obs_clip, z.forget_bias) == (2, 3, 164, 12, 5.0, 1.0)
    assert z.mlp_params == seat.mlp_table.params.data_ptr() and z.lstm_filt == seat.lstm_table.filt.data_ptr()
    assert tuple(seat.new_state(32).shape) == (32, 128)


def test_seat_of_one_family_has_one_table(nets, tmp_path):
    path = str(tmp_path / "agent-params-v3.npy")
    np.save(path, nets["ant-mlp-v3"])
    seat = zoo_pairs.ZooSeat([path], 120, 8, device="cpu")
    assert seat.kinds == ["mlp"] and seat.lstm_table is None and not seat.recurrent and seat.new_state(16) is None
    assert seat.labels == [path] and seat.entries.tolist() == [0]
    z = seat.struct(seat.mlp_table.params, None)
    assert not z.lstm_params and not z.lstm_filt and not z.state and (z.n_mlp, z.n_lstm) == (1, 0)
    seat = zoo_pairs.ZooSeat([nets["ant-lstm-v3"]], 120, 8, device="cpu")
    assert seat.kinds == ["lstm"] and seat.mlp_table is None and seat.entries.tolist() == [0] and (seat.n_mlp, seat.n_lstm) == (0, 1)


@pytest.mark.parametrize("species", sorted(DIMS))
def test_every_fixture_net_fits_its_species_seat_in_every_scene(nets, species):
    D, A = DIMS[species]
    for env_id in ENV_IDS:
        model = mjcf.load_model(env_id)
        for side, sp in enumerate(zoo_tournament.species_of(env_id)):
            if sp == species:
                assert (model.obs_dims[side] - 1, model.act_dims[side]) == (D, A), env_id
    seat = zoo_pairs.ZooSeat([nets[species + "-mlp-v3"], nets[species + "-lstm-v3"]], D, A, device="cpu")
    assert seat.kinds == ["mlp", "lstm"]


def test_species_mismatch_is_refused(nets):
    for other in ("bug-mlp-v3", "bug-lstm-v3", "spider-mlp-v3", "spider-lstm-v3"):
        with pytest.raises(ValueError, match="another species"):
            zoo_pairs.ZooSeat([nets["ant-mlp-v3"], nets[other]], 120, 8, device="cpu")
    with pytest.raises(ValueError, match="another species"):
        zoo_pairs.ZooSeat([nets["ant-mlp-v3"]], 164, 12, device="cpu")
    with pytest.raises(ValueError, match="reads 120 observation columns, the seat has 121"):
        zoo_pairs.ZooSeat([nets["ant-lstm-v3"]], 121, 8, device="cpu")
    with pytest.raises(ValueError, match="at least one"):
        zoo_pairs.ZooSeat([], 120, 8, device="cpu")


def test_tile_entries_of_a_batch(nets):
    seat = zoo_pairs.ZooSeat([nets["ant-lstm-v3"], nets["ant-mlp-v3"]], 120, 8, device="cpu")
    te = seat.tile_entries(np.repeat([0, 1, 1, 0], 16))
    assert te.tolist() == [1, 0, 0, 1] and te.dtype == np.int32
    for bad, msg in ((np.zeros(24, int), "whole tiles"), (np.arange(32) // 8, "play one net"), (np.full(16, 2), "outside"), (np.full(16, -1), "outside")):
        with pytest.raises(ValueError, match=msg):
            seat.tile_entries(bad)
    assert zoo_pairs.seat_runs(np.array([1, 1, 0, 1], np.int32)) == [(0, 2, 1), (2, 3, 0), (3, 4, 1)]


class _Env:
    """What play_zoo_pairs reads of an env before it refuses."""
    num_envs = 64


@pytest.mark.parametrize("epp", [1, 8, 17, 24, 0])
def test_envs_per_pair_off_the_tile_grid_is_refused(epp):
    with pytest.raises(ValueError, match="whole tiles of 16"):
        zoo_pairs.play_zoo_pairs(_Env(), None, None, [(0, 0)], 1, epp)


def test_trials_split_on_whole_tiles():
    assert zoo_pairs.split_trials16(16, 16) == (16, 1)
    assert zoo_pairs.split_trials16(64, 256) == (64, 1)
    assert zoo_pairs.split_trials16(96, 64) == (48, 2)
    assert zoo_pairs.split_trials16(512, 256) == (256, 2)
    for trials, num_env in ((20, 256), (8, 16), (32, 24)):
        with pytest.raises(ValueError):
            zoo_pairs.split_trials16(trials, num_env)


# ---- the script -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", ENV_IDS)
def test_path_rule_is_the_demos(env_id):
    a, b = env_id.split("-")[1].lower(), env_id.split("-")[3].lower()
    got = zoo_tournament.zoo_paths(env_id, ("mlp", "lstm"), (1, 2), "zoo/assets")
    assert got == [os.path.join("zoo/assets", a, "mlp", "agent-params-v1.npy"), os.path.join("zoo/assets", b, "lstm", "agent-params-v2.npy")]
    assert zoo_tournament.species_of(env_id) == (a, b) and a in DIMS and b in DIMS


def test_all_finds_every_net_of_both_species(tmp_path):
    for sp, fam, vs in (("ant", "mlp", (1, 2, 10)), ("ant", "lstm", (3,)), ("bug", "lstm", (2, 1))):
        os.makedirs(str(tmp_path / sp / fam))
        for v in vs:
            (tmp_path / sp / fam / ("agent-params-v%d.npy" % v)).write_bytes(b"")
    f0, f1 = zoo_tournament.all_paths("RoboSumo-Ant-vs-Bug-v0", str(tmp_path))
    rel = lambda fs: [os.path.relpath(f, str(tmp_path)) for f in fs]
    assert rel(f0) == ["ant/mlp/agent-params-v1.npy", "ant/mlp/agent-params-v2.npy", "ant/mlp/agent-params-v10.npy", "ant/lstm/agent-params-v3.npy"]
    assert rel(f1) == ["bug/lstm/agent-params-v1.npy", "bug/lstm/agent-params-v2.npy"]
    with pytest.raises(ValueError, match="no agent-params"):
        zoo_tournament.all_paths("RoboSumo-Ant-vs-Spider-v0", str(tmp_path))


def test_names_and_versions_take_two_values_each():
    base = ["--zoo", "z", "--env", "RoboSumo-Ant-vs-Bug-v0"]
    a = zoo_tournament.parse_args(base + ["--policy-names", "lstm", "mlp", "--param-versions", "3", "2", "--max_episodes", "16"])
    assert a.policy_names == ["lstm", "mlp"] and a.param_versions == [3, 2] and a.max_episodes == 16 and not a.stepwise and not a.all
    d = zoo_tournament.parse_args(base)
    assert d.policy_names == ["mlp", "mlp"] and d.param_versions == [1, 1] and d.max_episodes == 20 and d.num_env == 256
    for bad in (["--policy-names", "mlp"], ["--policy-names", "mlp", "lstm", "mlp"], ["--param-versions", "1"], ["--param-versions", "1", "2", "3"],
                ["--policy-names", "mlp", "gru"], ["--num_env", "24"]):
        with pytest.raises(SystemExit):
            zoo_tournament.parse_args(base + bad)
    for names, versions in ((("mlp",), (1, 1)), (("mlp", "mlp"), (1,)), (("mlp", "cnn"), (1, 1))):
        with pytest.raises(ValueError):
            zoo_tournament.zoo_paths("RoboSumo-Ant-vs-Bug-v0", names, versions, "z")


def test_module_does_not_shadow_the_test_helper():
    import zoo_play                                    # tests/zoo_play.py keeps its name
    assert os.path.dirname(os.path.abspath(zoo_play.__file__)) == HERE
    assert os.path.dirname(os.path.abspath(zoo_tournament.__file__)) == ROOT
