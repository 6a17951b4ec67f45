"""Generate tests/golden/solver_B2_C7_9x13_k3.npz: the reference's own Cython solver on fresh data.

Run where the reference tree is readable (the solver is rebuilt from it into oracle/_ref, see oracle/build_ref.py):

    python oracle/build_ref.py && python tests/golden/make_golden_solver.py

Stores the inputs of tests/test_oracle.py::test_against_live_reference_solver_if_built (z, the canonical bank wc) and
`solve_parallel`'s fp64 answer, so that the test holds the oracle to the reference's solver on every machine, not only
where oracle/_ref can be built.  Only inputs and outputs are saved.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
from oracle import build_ref, oracle  # noqa: E402


def solver_inputs():
    """The test's inputs; the same calls, so the stored arrays and the test's fresh ones must agree bit for bit."""
    rng = np.random.default_rng(5)
    wc = oracle.make_stored_weights(1, 7, 3, 3, orient=0, seed=77)
    z = rng.standard_normal((2, 7, 9, 13)).astype(np.float32)
    return z, wc


if __name__ == "__main__":
    assert build_ref.build(), "oracle/_ref could not be built (the reference tree is not readable here)"
    solve_parallel = build_ref.load()
    z, wc = solver_inputs()
    ref = solve_parallel(np.array(z, dtype=np.float64), np.array(wc, dtype=np.float64), (3, 3))
    path = os.path.join(OUT, "solver_B2_C7_9x13_k3.npz")
    np.savez_compressed(path, z=z, wc=wc, ref=ref)
    print("wrote", path, ref.shape, ref.dtype)
