"""The matrix of fused-launch kernels a user can reach: which ``sumo_rollout_kernel<NV, POLICY, SL>`` instantiations the Python API
can launch, one row per (scene variant, policy).  Pure: no GPU, no torch, nothing imported at module level but the bindings' tables.
tests/test_fused_matrix_cpu.py holds the matrix against ``capi``, ``runner.rollout_launch``, ``matches.match_pairing``, ``co_train``
and the engine's source; tests/test_gpu_fused_matrix.py runs every row against its step-by-step path.

The library holds 7 kernel variants x ``SUMO_N_POLICY`` = 17 policy phases = 119 instantiations (csrc/sumo_engine.hip ``SUMO_RK_ALL``,
csrc/engine_host_fused.h ``rollout_kernel``): dynamic layout ``<nv, *, 0>`` at nv 28, 32, 36, 40, 44 and static layout ``<28, *, 1>``
(Ant-vs-Ant), ``<44, *, 2>`` (Spider-vs-Spider).

Reachable (87 instantiations, the 91 rows of :func:`cases`; the mirrored mixed scenes share a kernel):

    <28, 0..16, 1>   Ant-vs-Ant                            <28, 0..16, 0>   Ant-vs-Ant with SUMO_STATIC_LAYOUT=0
    <36, 0..16, 0>   Bug-vs-Bug (0..16), Ant-vs-Spider / Spider-vs-Ant (16)
    <44, 0..16, 2>   Spider-vs-Spider                      <44, 0..16, 0>   Spider-vs-Spider with SUMO_STATIC_LAYOUT=0
    <32, 16, 0>      Ant-vs-Bug / Bug-vs-Ant               <40, 16, 0>      Bug-vs-Spider / Spider-vs-Bug

Policy 16 (``sumo_rollout_steps_pair``) on a same-species scene: ``co_train.learn`` refuses a homogeneous env (``check_learn``), but
``co_train.PairRunner(engine_fused=True)`` and ``SumoVecEnv.rollout_steps_pair_group`` are public and accept one -- the entry's own
scene check says "a homogeneous scene is simply a valid one" -- so these five rows are in the matrix.

UNREACHABLE (32 instantiations): policies 0 .. 15 at nv 32 and nv 40, ``<32, 0..15, 0>`` and ``<40, 0..15, 0>``.  Only mixed scenes
have these nv, and every entry point but ``sumo_rollout_steps_pair`` refuses a mixed scene (``rollout_scene``: "fused rollout needs
a homogeneous match-up").  They are compiled, linked and never launched; the next change to how the library is built can drop them.
"""
from collections import namedtuple

ENV_ID = "RoboSumo-%s-vs-%s-v0"
SPECIES = ("ant", "bug", "spider")

# key, env id, the species of agent 0 / agent 1, nv, engine.static_layout(), SUMO_STATIC_LAYOUT to set before the envs exist (or None)
Variant = namedtuple("Variant", "key env_id species nv static layout_env")


def _same(species, nv, static, layout_env=None):
    key = species + ("-static" if static else "-dynamic" if layout_env is not None else "")
    return Variant(key, ENV_ID % (species.title(), species.title()), (species, species), nv, static, layout_env)


def _mixed(a, b, nv):
    return Variant("%s-%s" % (a, b), ENV_ID % (a.title(), b.title()), (a, b), nv, False, None)


VARIANTS = (
    _same("ant", 28, True), _same("ant", 28, False, "0"), _same("bug", 36, False), _same("spider", 44, True), _same("spider", 44, False, "0"),
    _mixed("ant", "bug", 32), _mixed("bug", "ant", 32), _mixed("ant", "spider", 36), _mixed("spider", "ant", 36),
    _mixed("bug", "spider", 40), _mixed("spider", "bug", 40),
)

# policy -> (C entry, builder key, envs).  The policy is the third argument of the entry's ``rollout_launch(E, r, POLICY, b, stream)``
# (csrc/engine_host_fused.h).  Builder keys: 'rollout:<learner>:<opponent>' a ``Runner``, 'match:<pairing>' a ``matches`` pairing,
# 'pair' a ``co_train.PairRunner``.  Envs: 40 = two whole 16-env tiles and a partial one of 8; 48 where the mode deals one table row
# per whole tile and refuses or leaves a partial one (see tests/test_gpu_fused_matrix.py for the lines); 64 for the co-training launch,
# which splits the tiles in two halves of whole pairs (co_train.tile_halves: "num_envs = %d is not a multiple of 32").
POLICIES = {
    0: ("sumo_rollout_steps", "rollout:mlp:self", 40),            # (an MLP snapshot pool has no step-by-step path to compare with)
    1: ("sumo_rollout_steps_lstm", "rollout:lstm:pool", 48),
    2: ("sumo_match_steps", "match:mlp", 40),
    3: ("sumo_match_steps_lstm", "match:lstm", 40),
    4: ("sumo_rollout_steps_zoo", "rollout:mlp:zoo_mlp", 40),
    5: ("sumo_match_steps_zoo", "match:zoo", 40),
    6: ("sumo_match_steps_zoo_lstm", "match:zoo_lstm", 40),
    7: ("sumo_match_steps_lstm_zoo_lstm", "match:lstm_zoo_lstm", 40),
    8: ("sumo_rollout_steps_zoo_lstm", "rollout:mlp:zoo_lstm", 40),
    9: ("sumo_rollout_steps_lstm_zoo", "rollout:lstm:zoo_mlp", 48),
    10: ("sumo_rollout_steps_lstm_zoo_lstm", "rollout:lstm:zoo_lstm", 48),
    11: ("sumo_rollout_steps_zoo_league", "rollout:mlp:league", 48),
    12: ("sumo_rollout_steps_lstm_zoo_league", "rollout:lstm:league", 48),
    13: ("sumo_match_steps_cross", "match:cross", 40),
    14: ("sumo_match_steps_lstm_zoo", "match:lstm_zoo", 40),
    15: ("sumo_rollout_steps_lstm_reuse", "rollout:lstm:reuse", 40),
    16: ("sumo_rollout_steps_pair", "pair", 64),
}
PAIR_POLICY = 16

Case = namedtuple("Case", "id variant policy entry builder num_envs")


def is_mixed(variant):
    return variant.species[0] != variant.species[1]


def reachable(variant):
    """The policies the Python API can launch on ``variant``: all of them on a same-species scene, the co-training launch alone on
    a mixed one."""
    return (PAIR_POLICY,) if is_mixed(variant) else tuple(sorted(POLICIES))


def cases():
    """One :class:`Case` per (variant, policy) the Python API can reach, in variant and policy order."""
    out = []
    for v in VARIANTS:
        for p in reachable(v):
            entry, builder, n = POLICIES[p]
            out.append(Case("%s-p%02d-%s" % (v.key, p, entry[len("sumo_"):]), v, p, entry, builder, n))
    return out


def kernel_of(case):
    """(NV, POLICY, SL) of the ``sumo_rollout_kernel`` instantiation the case launches (SL: 1 Ant's static layout, 2 Spider's, 0 dynamic)."""
    v = case.variant
    return v.nv, case.policy, (0 if not v.static else {28: 1, 44: 2}[v.nv])
