"""CPU (no GPU): the seeded draw of the depth front end (genpose_amd.preprocess.seeded_ranks, the host-side definition of what
gp_roi_sample_seeded draws on the device; csrc/philox.h, "the depth front end's draw").  The draw is restated here, independently, on
tests/philox_reference.py's Philox and counter layout; then its rules, its keying, its place in the counter layout and its statistics."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_reference as pr  # noqa: E402
import track_prior_reference as tpr  # noqa: E402

from genpose_amd.preprocess import seeded_ranks  # noqa: E402

ROUNDS = 8
PRIOR_STEP = (1 << 29) - 1
STREAM = 1


def F_counters(u, r, seed, run, slot):
    """(ctr [n, 4], key [n, 2]) of the round function's blocks, through philox_reference.pack: ctr[0] = u and ctr[1] = slot | r << 24 are
    the low and high words of pack's `row`; step = the reserved one, stream 1, block 0."""
    u = np.asarray(u, np.uint64)
    row = u | np.uint64(((slot & 0xFFFFFF) | r << 24) << 32)
    return pr.pack(seed, run, PRIOR_STEP, STREAM, 0, row)


def F(u, r, seed, run, slot):
    ctr, key = F_counters(u, r, seed, run, slot)
    return pr.philox4x32_10(ctr, key)[..., 0].astype(np.uint64)


def restated_ranks(c, n, seed, run, slot):
    """The issue's definition, row by row in the walk (one vector over the output rows, no sharing with the package's code)."""
    k = np.arange(n, dtype=np.uint64)
    if c < n:
        return (k % np.uint64(c)).astype(np.int64)
    if c == n:
        return k.astype(np.int64)
    b = max(2, (c - 1).bit_length())
    ha = b // 2
    hb = b - ha
    out = np.zeros(n, dtype=np.int64)
    x, rows = k.copy(), np.arange(n)
    while rows.size:
        a, v = x >> np.uint64(hb), x & np.uint64((1 << hb) - 1)
        for r in range(ROUNDS):
            if r % 2 == 0:
                a = a ^ (F(v, r, seed, run, slot) & np.uint64((1 << ha) - 1))
            else:
                v = v ^ (F(a, r, seed, run, slot) & np.uint64((1 << hb) - 1))
        x = a << np.uint64(hb) | v
        done = x < np.uint64(c)
        out[rows[done]] = x[done].astype(np.int64)
        x, rows = x[~done], rows[~done]
    return out


COUNTS = (1, 2, 63, 64, 65, 1100, 65536)
N_PTS = (64, 1024)


@pytest.mark.parametrize("n", N_PTS)
@pytest.mark.parametrize("c", COUNTS)
def test_seeded_ranks_is_the_restated_draw_and_keeps_its_rules(c, n):
    seed, run, slot = 0x1234_5678_9ABC_DEF1, 41, 19
    got = seeded_ranks(c, n, seed, run, slot)
    assert got.dtype == np.int64 and got.shape == (n,)
    np.testing.assert_array_equal(got, restated_ranks(c, n, seed, run, slot))
    k = np.arange(n)
    if c < n:
        np.testing.assert_array_equal(got, k % c)  # sample_points' tiling
    elif c == n:
        np.testing.assert_array_equal(got, k)
    else:
        assert got.min() >= 0 and got.max() < c and len(np.unique(got)) == n
        assert not np.array_equal(got, k)  # (a draw, not the first n pixels)


def test_every_branch_is_among_the_cases():
    for n in N_PTS:
        assert any(c < n for c in COUNTS) and sum(c > n for c in COUNTS) >= 2
    assert 64 in COUNTS and 63 in COUNTS and 65 in COUNTS  # c == n at n = 64, and either side of it


def test_batched_seeds_are_the_single_draws():
    seeds, runs, slots = np.array([0, 5, 1 << 40]), np.array([0, 7, 2]), np.array([3, 3, 1 << 20])
    R = seeded_ranks(1100, 64, seeds, runs, slots)
    assert R.shape == (3, 64)
    for s in range(3):
        np.testing.assert_array_equal(R[s], seeded_ranks(1100, 64, int(seeds[s]), int(runs[s]), int(slots[s])))


@pytest.mark.parametrize("c,n", [(65, 64), (1100, 1024), (5000, 64)])
def test_seed_run_and_slot_each_move_the_draw(c, n):
    base = dict(seed=11, run=4, slot=9)
    ref = seeded_ranks(c, n, **base)
    np.testing.assert_array_equal(ref, seeded_ranks(c, n, **base))
    for name, other in (("seed", 12), ("seed", 11 + (1 << 32)), ("run", 5), ("slot", 10)):
        moved = seeded_ranks(c, n, **{**base, name: other})
        assert not np.array_equal(ref, moved), (name, other)


def test_counter_words_lie_on_the_reserved_step_with_the_stream_bit_set():
    """Every (counter, key) of the round function unpacks to (step = PRIOR_STEP, stream 1, block 0); the tracker's prior has stream 0 at
    that step and a PC sampler's steps end at PRIOR_STEP - 1: the stream bit alone tells the front end's tuples from both."""
    u = np.arange(0, 1 << 10, dtype=np.uint64)
    for r in range(ROUNDS):
        for slot in (0, 1, 77, (1 << 24) - 1):
            ctr, key = F_counters(u, r, seed=99, run=12, slot=slot)
            seed, run, step, stream, block, row = pr.unpack(ctr, key)
            assert (step == PRIOR_STEP).all() and (stream == 1).all() and (block == 0).all() and (seed == 99).all() and (run == 12).all()
            assert ((ctr[..., 3] >> np.uint32(2)) & np.uint32(1) == 1).all()
            assert (ctr[..., 0] == u.astype(np.uint32)).all() and (ctr[..., 1] == np.uint32(slot | r << 24)).all()
    # the prior: the same step, stream bit clear, for any rows
    pc, _ = tpr.counters(99, 12, tpr.global_rows(3, 8, 50))
    assert ((pc[..., 3] >> np.uint32(3)) == PRIOR_STEP).all() and (((pc[..., 3] >> np.uint32(2)) & np.uint32(1)) == 0).all()
    # a PC draw: pack() refuses nothing below 2^29, the samplers take nsteps < 2^29, so their last step is PRIOR_STEP - 1
    cpc, _ = pr.pack(99, 12, PRIOR_STEP - 1, pr.STREAM_PREDICTOR, 2, np.uint64(5))
    assert int(cpc[3]) >> 3 < PRIOR_STEP
    from genpose_amd import preprocess
    assert preprocess.PRIOR_STEP == tpr.PRIOR_STEP == PRIOR_STEP and preprocess.FRONT_END_STREAM == 1 != tpr.PRIOR_STREAM
    assert preprocess.FEISTEL_ROUNDS == ROUNDS


def chi_square_z(R, c):
    """R [S, n]: S draws of n distinct ranks out of c -> (z of the inclusion counts, z of the element in output row 0), each a chi-square
    with c - 1 degrees of freedom as a z-score (X - (c - 1)) / sqrt(2 (c - 1)).
    Row 0: the S values are multinomial over c equal cells, X = sum (o - S/c)^2 / (S/c), the textbook statistic.
    Inclusion: under a uniform n-subset the indicator of pixel j has p = n/c, variance p (1 - p) and covariance -p (1 - p) / (c - 1) with
    every other pixel's, so o_j (over S draws) has variance S p (1 - p) and sum_j (o_j - S p)^2 has mean c S p (1 - p); the statistic
    X = (c - 1) / c * sum_j (o_j - S p)^2 / (S p (1 - p)) then has mean c - 1 and, the counts being asymptotically normal on the
    hyperplane sum_j o_j = S n with exchangeable covariance, the chi-square law with c - 1 degrees of freedom."""
    S, n = R.shape
    inc = np.bincount(R.ravel(), minlength=c).astype(np.float64)
    p = n / c
    x_inc = (c - 1) / c * ((inc - S * p) ** 2).sum() / (S * p * (1 - p))
    first = np.bincount(R[:, 0], minlength=c).astype(np.float64)
    x_first = ((first - S / c) ** 2).sum() / (S / c)
    z = lambda x: (x - (c - 1)) / math.sqrt(2.0 * (c - 1))
    return z(x_inc), z(x_first)


@pytest.mark.parametrize("c,n,seeds", [(1100, 1024, 3000), (1500, 1024, 3000), (5000, 1024, 3000), (37, 16, 20000), (300, 64, 20000),
                                       (37, 64, 20000), (300, 16, 20000)])
def test_draw_statistics(c, n, seeds):
    """Over `seeds` seeds: every draw distinct and inside [0, c) where c > n, and the two chi-square z-scores within the project's 5-sigma
    convention (philox_reference.statistics).  (37, 64) is the tiling branch: only its rule is checked there."""
    R = seeded_ranks(c, n, np.arange(seeds, dtype=np.uint64) + np.uint64(1000), 3, 5)
    assert R.shape == (seeds, n)
    if c <= n:
        np.testing.assert_array_equal(R, np.broadcast_to(np.arange(n) % c, (seeds, n)))
        return
    assert R.min() >= 0 and R.max() < c
    srt = np.sort(R, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "a draw repeats a pixel"
    z_inc, z_first = chi_square_z(R, c)
    print(f"c = {c}, n = {n}, {seeds} seeds: z(inclusion) = {z_inc:+.2f}, z(row 0) = {z_first:+.2f}")
    assert abs(z_inc) <= 5.0 and abs(z_first) <= 5.0
