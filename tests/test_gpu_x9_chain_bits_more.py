"""GPU: the bf16x9 chain kernels (PC step, seeded PC step, Heun step; csrc/trunk_bf16x9.h) give the BITS recorded in
tests/golden/x9_chain_bits_more.npz on the shapes tests/golden/x9_chain_bits.npz does not have.  The fixture was taken before the staged
fp32 operands (w_out, the hidden biases, cvec[cloud] + tvec for NCL clouds) were requested ahead of the sampler update and before the
k-major layers' splits and tails went between the MFMAs: summation orders and expressions are unchanged, so nothing may differ.  The
cases, their shapes and the replay itself are tests/golden/make_x9_chain_bits_more.py's: 6 x 43 = 258 rows (workgroup 1 spans clouds
2-5, all four staged rows; workgroup 2 has two live rows and a clamped last cloud), 1 x 50 = 50 rows (78 clamped duplicate rows, two
waves without a live row), the seeded kernel and the Heun step on 6 x 43."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("pc_w", "pc_one", "pc_s", "heun")


def _generator():
    spec = importlib.util.spec_from_file_location("make_x9_chain_bits_more", os.path.join(HERE, "golden", "make_x9_chain_bits_more.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def replay(golden):
    rec = golden("x9_chain_bits_more.npz")
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
