"""CPU checks of tests/exact_mlp_ref.py, the exact-arithmetic reference of tests/test_gpu_grad_partition.py: it is the same gradient as
the float64 restatements (tests/a2c_ref.py, oracle/ppo_oracle.py), and every case of the GPU test satisfies the exactness condition
(largest absolute-sum bound < 2**24) and exercises the nets (active relus, nonzero gradient entries)."""
import numpy as np
import pytest

import exact_mlp_ref as E
from a2c_ref import a2c_loss_and_grads
from oracle import ppo_oracle as po

ALL = E.CASES + E.REUSE


@pytest.mark.parametrize("ob,ac,n,ent_coef", [(121, 8, 117, 1), (5, 1, 37, 0), (209, 16, 64, 1)])
def test_exact_reference_is_the_a2c_and_ppo_value_gradient(ob, ac, n, ent_coef):
    """exact_grads = n * (gradient of the mean loss) of the float64 restatements with vf_coef = 1: integers, so the float64 results
    differ from them by rounding only (1e-9 relative to the tensor's largest entry)."""
    pr = E.make_problem(ob, ac, n, seed=3)
    g, dv, bound, _ = E.exact_grads(pr["params"], pr["obs"], pr["act"], pr["adv"], pr["ret"], pr["w"], ent_coef)
    _, _, sums, ga = a2c_loss_and_grads(pr["params"], pr["obs"], pr["act"], pr["adv"], pr["ret"], pr["w"], float(ent_coef), 1.0)
    for k in range(13):
        ref = n * np.asarray(ga[k]).reshape(g[k].shape)
        assert np.array_equal(np.rint(g[k]), g[k])
        assert np.abs(g[k] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), k
    assert 0.5 * np.sum(pr["w"].astype(np.float64) * dv * dv) == pytest.approx(sums[1], rel=1e-12) and pr["w"].sum() == sums[2]
    gv, dv2, _, _ = E.exact_grads(pr["params"], pr["obs"], pr["act"], pr["adv"], pr["ret"], pr["w"], ent_coef, weighted_value=False)
    old = np.zeros(n, np.float32)
    _, stats, _, gp = po.ppo_loss_and_grads(pr["params"], pr["obs"], pr["act"], pr["adv"], pr["ret"], old, pr["w"], 0.2, 0.0, 1.0)
    for k in (4, 5, 6, 7, 11, 12):
        ref = n * np.asarray(gp[k]).reshape(gv[k].shape)
        assert np.abs(gv[k] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), k
    assert np.array_equal(dv, dv2) and 0.5 * np.sum(dv * dv) / n == pytest.approx(stats[1], rel=1e-12)
    assert E.flat(g).dtype == np.float32 and np.array_equal(E.flat(g).astype(np.float64), np.concatenate([t.ravel() for t in g]))


@pytest.mark.parametrize("case", ALL, ids=[c[0] for c in ALL])
def test_gpu_cases_are_exact_and_exercise_the_nets(case):
    """Conditions on the rows the GPU test uses, for both entropy coefficients and both value-term forms:
      * bound < 2**24: every partial sum of every summation order is an exactly representable float32;
      * at least a third of the hidden units of each of the four hidden layers are active;
      * n >= 15: at least a third of the entries of each weight-gradient tensor are nonzero.  A gradient over n rows is a sum of n outer
        products of vectors that are about half zeros, so a single row fills at most about a quarter of a tensor: for n = 1 the condition
        is instead that the row has a nonzero weight, advantage and value residual and that every weight gradient has nonzero entries."""
    d = E.build_case(case)
    r, n = d["rows"], d["n"]
    pr = E.problem(d["ob"], d["ac"])
    for ent_coef in (0, 1):
        for weighted in (True, False):
            g, dv, bound, frac = E.exact_grads(pr["params"], r["obs"], r["act"], r["adv"], r["ret"], r["w"], ent_coef, weighted)
            assert bound < E.EXACT_LIMIT
            assert min(frac.values()) >= 1.0 / 3.0, frac
            for k in (0, 2, 4, 6, 8, 11):
                nz = float((g[k] != 0).mean())
                assert nz >= 1.0 / 3.0 if n >= 15 else nz > 0, (k, nz)
    if n == 1:
        assert r["w"][0] != 0 and r["adv"][0] != 0 and dv[0] != 0
    assert np.isnan(d["obs"]).any() and np.isnan(d["adv_mb"][n:]).all()
    if d["idx"] is not None:
        assert np.isnan(d["obs"][d["idx"][n:], 0]).all() and not np.isnan(d["obs"][d["idx"][:n], :d["ob"]]).any()
