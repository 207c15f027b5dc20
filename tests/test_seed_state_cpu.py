"""_lib.seed_words, the one writer of the Philox seed state (csrc/philox.h: 8 uint32 words - seed lo, seed hi, run, 0, row base lo, row base
hi, 0, 0), against the two spellings its callers used to write by hand, restated here literally: the uint32 [8] array of the front ends and
the tracker, and the int64 [4] tensor of the samplers with the seed folded into two's complement.  No device."""
import itertools

import numpy as np
import pytest

from genpose_amd._lib import seed_words

SEEDS = (0, 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, (1 << 64) + 5, -1)
RUNS = (0, 7, (1 << 32) - 1)
BASES = (0, (1 << 32) - 1, 1 << 32, (1 << 63) - 1)


def _as_uint32(seed, run, base):
    seed = int(seed) % (1 << 64)
    return np.array([seed & 0xFFFFFFFF, seed >> 32, run & 0xFFFFFFFF, 0, base & 0xFFFFFFFF, base >> 32, 0, 0], dtype=np.uint32)


def _as_int64(seed, run, base):
    seed = int(seed) % (1 << 64)
    return np.array([seed - (1 << 64) if seed >= (1 << 63) else seed, int(run), int(base), 0], dtype=np.int64)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_words_are_both_hand_written_spellings(seed):
    for run, base in itertools.product(RUNS, BASES):
        w = seed_words(seed, run, base)
        assert w.dtype == np.uint32 and w.shape == (8,) and w.flags.c_contiguous
        assert np.array_equal(w, _as_uint32(seed, run, base)), (seed, run, base)
        assert np.array_equal(w.view(np.int64), _as_int64(seed, run, base)), (seed, run, base)
        assert np.array_equal(w.view(np.int32).view(np.uint32), w)  # (the int32 [8] view the front ends upload: the same bytes)


def test_run_and_base_default_to_zero():
    assert np.array_equal(seed_words(0xFEED5EED12345678), _as_uint32(0xFEED5EED12345678, 0, 0))


@pytest.mark.parametrize("run,base", [(1 << 32, 0), (-1, 0), (0, 1 << 63), (0, -1)])
def test_a_run_outside_32_bits_or_a_base_outside_63_is_refused(run, base):
    with pytest.raises(ValueError):
        seed_words(3, run, base)
