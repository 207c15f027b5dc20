"""numpy restatement of the fixed-step tracker's prior (genpose_amd/csrc/philox.h, "the tracker's prior"; gp_track_warm_start,
gp_track_prior_fill), on top of tests/philox_reference.py: the generator, the Box-Muller map and the counter layout are the seeded PC
sampler's, with the STEP field reserved:
    key[0], key[1] = seed bits 0..31, 32..63
    ctr[0], ctr[1] = GLOBAL row = (sequence * max_objects_per_frame + object) * K + candidate, bits 0..31, 32..63
    ctr[2]         = FRAME index (the seed state's run word)
    ctr[3]         = PRIOR_STEP << 3 | 0 << 2 | block,  PRIOR_STEP = 2^29 - 1, block 0..2
A seeded PC sampler takes nsteps < 2^29, so its step fields end at 2^29 - 2: every field has its own bits, hence no PC draw shares a
(counter, key) with the prior.  A helper for tests/test_fixed_step_tracker_host.py and tests/test_gpu_fixed_step_tracker.py, not a test."""
import numpy as np

import philox_reference as pr

PRIOR_STEP = (1 << 29) - 1
PRIOR_STREAM = 0


def global_rows(sequence, n_objects, K, max_objects_per_frame=8):
    """Global rows of a sequence's frame with n_objects objects x K candidates, in launch order -> uint64 [n_objects * K]."""
    assert n_objects <= max_objects_per_frame
    base = np.uint64(sequence) * np.uint64(max_objects_per_frame) * np.uint64(K)
    return base + np.arange(n_objects * K, dtype=np.uint64)


def counters(seed, frame, rows):
    """(ctr [n, 3, 4], key [n, 3, 2]) uint32: the three blocks of every row."""
    rows = np.asarray(rows, np.uint64)
    cs, ks = zip(*[pr.pack(seed, frame, PRIOR_STEP, PRIOR_STREAM, b, rows) for b in range(3)])
    return np.stack(cs, axis=-2), np.stack(ks, axis=-2)


def normals(seed, frame, rows):
    """The nine float32 standard normals of every row -> [n, 9]."""
    return pr.normals(seed, frame, PRIOR_STEP, PRIOR_STREAM, np.asarray(rows, np.uint64))
