"""CPU checks of the one piece of pure logic in ``alg_ppo.learn``: which checkpoints agent 1 gets and which draws from numpy's
global stream that consumes (``alg_ppo.choose_opponents``).  The expected values are the draw expressions of the loop the function
was cut from, written out here."""
import numpy as np
import pytest

from robosumo_selfplay_amd.alg_ppo import choose_opponents

SEED = 1234


def _uniform(sub):
    return np.full(len(sub), 1.0 / len(sub))


def _expected(mode, update, npaths, K):
    if mode == "random":
        return [int(x) for x in np.random.choice(update, K)]
    if mode == "latest":
        return list(range(npaths - 1, max(-1, npaths - 1 - K), -1))
    sub = np.sort(np.random.choice(npaths, 30, replace=False)) if npaths > 30 else np.arange(npaths)
    rd = _uniform(sub)
    return [int(sub[j]) for j in np.random.choice(len(rd), K, p=rd)]


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("npaths", [1, 2, 31, 40])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("mode", ["random", "latest", "ours"])
def test_choices_and_draws_are_the_loops(mode, K, npaths):
    update = npaths + 1        # a checkpoint per update: 00000 .. update - 1 exist when ``update`` selects
    np.random.seed(SEED)
    want = _expected(mode, update, npaths, K)
    state = np.random.get_state()
    np.random.seed(SEED)
    got = choose_opponents(mode, update, npaths, K, _uniform)
    assert got == want and all(type(c) is int for c in got)
    assert _same_state(np.random.get_state(), state)      # 'latest': the state of a fresh seed, no draw at all


def test_latest_with_fewer_paths_than_slots():
    assert choose_opponents("latest", 3, 2, 3, None) == [1, 0]
    assert choose_opponents("latest", 2, 1, 3, None) == [0]
    assert choose_opponents("latest", 9, 8, 3, None) == [7, 6, 5]


@pytest.mark.parametrize("npaths", [5, 40])
def test_ours_scores_the_sorted_subset_once_and_samples_with_its_probabilities(npaths):
    calls = []

    def one_hot(sub):
        calls.append(np.array(sub))
        p = np.zeros(len(sub))
        p[3] = 1.0
        return p
    np.random.seed(SEED)
    got = choose_opponents("ours", npaths + 1, npaths, 4, one_hot)
    assert len(calls) == 1
    sub = calls[0]
    assert len(sub) == min(npaths, 30) and np.array_equal(sub, np.sort(sub)) and len(set(sub.tolist())) == len(sub)
    assert 0 <= sub.min() and sub.max() < npaths
    if npaths <= 30:
        assert np.array_equal(sub, np.arange(npaths))
    assert got == [int(sub[3])] * 4


def test_unknown_mode():
    with pytest.raises(ValueError, match="opponent_mode 'sideways'"):
        choose_opponents("sideways", 2, 1, 1, None)
