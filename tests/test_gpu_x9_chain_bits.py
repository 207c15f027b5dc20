"""GPU: the bf16x9 chain kernels (PC step, seeded PC step, Heun step, RK45 stage; csrc/trunk_bf16x9.h) give the BITS recorded in
tests/golden/x9_chain_bits.npz, which was taken from the k-major heads before they went chunk-major: every accumulator still receives
its k-blocks in ascending order and every head output its chunks in ascending order, so nothing may differ.  The cases, their shapes and
the replay itself are tests/golden/make_x9_chain_bits.py's (129 rows: clamped duplicate rows, a workgroup's rows over several clouds, a
head epilogue crossing a ring barrier, the last head's exposed tail; two batches per launch; seeded noise; Heun; one RK45 solve)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("pc_a", "pc_b", "pc_s", "heun", "ode")


def _generator():
    spec = importlib.util.spec_from_file_location("make_x9_chain_bits", os.path.join(HERE, "golden", "make_x9_chain_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def replay(golden):
    rec = golden("x9_chain_bits.npz")
    inputs = {k: v for k, v in rec.items() if ".out." not in k}
    return rec, _generator().compute(inputs)


@pytest.mark.parametrize("case", CASES)
def test_recorded_bits(replay, case):
    rec, new = replay
    names = sorted(k for k in rec if k.startswith(case + ".out."))
    assert names and names == sorted(k for k in new if k.startswith(case + ".out."))
    for k in names:
        assert rec[k].dtype == new[k].dtype and rec[k].shape == new[k].shape, k
        differ = int(np.count_nonzero(rec[k] != new[k]))
        print(f"{k} {rec[k].shape}: {differ} of {rec[k].size} elements differ")
        assert np.array_equal(rec[k], new[k]), k
