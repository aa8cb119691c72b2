"""The block certificate's numpy model (tests/_lobpcg.py) against dense eigenvalues, no GPU: the method itself, with
the library's start stream, locked block, drop and refresh rules and defaults, on every case the GPU tests run
(tests/_cholcert.py).  The GPU tests take their iteration bars from this model, so what is asserted here is what
those bars stand on:

* it converges within max_iters (2000) at tol 1e-8;
* its value is the dense one to 1e-6 |lambda|_max (it stops at a residual of 1e-8 |lambda|_max-estimate, and a Ritz
  value lies within its residual of an eigenvalue): lambda_min(S) without U, the lowest eigenvalue of S on U's
  complement with U;
* lower_bound <= lambda_min(S) <= the returned lambda, up to 1e-9 |lambda|_max (the bars of
  tests/test_gpu_certify.py's sandwich);
* at both golden optima a block of r rows needs fewer iterations than a block of one row: each iteration costs the
  same one operator pass over all r rows of the lifted layout, so this is the feature's premise."""
import pytest

from tests import _cholcert as CC
from tests import _lobpcg as LB

CASES = CC.DECISION_CASES + [CC.WEIGHTED]
_ids = lambda k: "-".join(map(str, k))  # noqa: E731


@pytest.mark.parametrize("seed_x", [False, True], ids=["plain", "seed_x"])
@pytest.mark.parametrize("key", CASES, ids=_ids)
def test_model_against_dense(key, seed_x):
    c = CC.case(key)
    out = LB.model(key, seed_x)
    print(key, seed_x, {k: v for k, v in out.items() if k not in ("vec", "ritz")})
    assert out["converged"] and out["iterations"] <= 2000
    dense = LB.complement(key)["lambda_complement"] if seed_x else c.lam
    assert abs(out["lambda_complement"] - dense) <= 1e-6 * c.lam_max, (out["lambda_complement"], dense)
    assert out["lower_bound"] <= c.lam + 1e-9 * c.lam_max <= out["lambda_min"] + 2e-9 * c.lam_max, (out, c.lam)
    if seed_x:
        ref = LB.complement(key)
        assert out["seeds"] == ref["seeds"]
        assert abs(out["lambda_seed"] - ref["lambda_seed"]) <= 1e-9 * c.lam_max
        assert abs(out["coupling"] - ref["coupling"]) <= 1e-9 * c.lam_max + 1e-6 * ref["coupling"]
        assert out["lambda_min"] == min(out["lambda_seed"], out["lambda_complement"])


@pytest.mark.parametrize("seed_x", [False, True], ids=["plain", "seed_x"])
@pytest.mark.parametrize("key", [CC.OPT_SMALL, CC.OPT_TINY], ids=_ids)
def test_block_needs_fewer_iterations_than_one_row(key, seed_x):
    """The premise: at an optimum (a cluster of small eigenvalues above the locked near-null block) r rows converge
    in fewer iterations than one."""
    blk, one = LB.model(key, seed_x), LB.model(key, seed_x, block=1)
    print(key, seed_x, "iterations: block r", blk["iterations"], "one row", one["iterations"])
    assert blk["converged"] and one["converged"]
    assert blk["iterations"] < one["iterations"]


@pytest.mark.parametrize("key", [CC.OPT_SMALL, CC.OPT_TINY], ids=_ids)
def test_preconditioned_model(key):
    """precon = 1 (the block-Jacobi inverse of Q + 0.1 I per pose) at both optima: the same value and bound."""
    c = CC.case(key)
    out = LB.model(key, True, precon=True)
    print(key, "iterations", out["iterations"], "plain", LB.model(key, True)["iterations"])
    assert out["converged"]
    assert abs(out["lambda_complement"] - LB.complement(key)["lambda_complement"]) <= 1e-6 * c.lam_max
    assert out["lower_bound"] <= c.lam + 1e-9 * c.lam_max <= out["lambda_min"] + 2e-9 * c.lam_max


def test_start_block_is_the_certificates_stream():
    """The first values of the SplitMix64 stream (seed 0x5EED), in the lifted layout's memory order."""
    b = LB.start_block(3, 4)
    st, vals = 0x5EED, []
    for _ in range(12):
        st = (st + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        z = st
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        z ^= z >> 31
        vals.append(2.0 * ((z >> 11) / 9007199254740992.0) - 1.0)
    assert [b[i, x] for x in range(4) for i in range(3)] == vals
