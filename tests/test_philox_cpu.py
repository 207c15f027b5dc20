"""CPU: the numpy restatement of the seeded PC sampler's generator (tests/philox_reference.py) - the published known-answer vectors of
Philox4x32-10, the statistics of its normals with derived bounds, and the counter layout's injectivity.  The device generator
(genpose_amd/csrc/philox.h) is held to this restatement bit for bit in tests/test_gpu_seeded_noise.py."""
import numpy as np
import pytest

import philox_reference as pr

# (counter, key, output): the known-answer vectors distributed with Random123 for philox4x32-10
KAT = [
    ([0x00000000] * 4, [0x00000000] * 2, [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
]

STAT_SEED, STAT_RUN, STAT_STEPS, STAT_ROWS = 20240229, 3, 4, 65536  # 2 streams x 4 steps x 65 536 rows x 9 = 4.7e6 normals


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_known_answer_vectors(ctr, key, out):
    got = pr.philox4x32_10(np.array([ctr], dtype=np.uint32), np.array([key], dtype=np.uint32))[0]
    assert [hex(int(v)) for v in got] == [hex(v) for v in out]


def test_uniforms_and_truncation():
    """Uniforms are in (0, 1] on the 2^-24 grid, so every normal is finite and |z| <= sqrt(48 log 2) = 5.768."""
    w = np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint32)
    u = pr.uniform24(w)
    assert u.dtype == np.float32 and u.tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0]
    z1, z2 = pr.noise(7, 0, 2, 4096)
    assert np.isfinite(z1).all() and np.isfinite(z2).all() and max(np.abs(z1).max(), np.abs(z2).max()) <= pr.Z_MAX * (1 + 1e-6)


def test_statistics_of_the_normals():
    z1, z2 = pr.noise(STAT_SEED, STAT_RUN, STAT_STEPS, STAT_ROWS)
    z1n, _ = pr.noise(STAT_SEED + 1, STAT_RUN, STAT_STEPS, STAT_ROWS)
    assert z1.size + z2.size >= 4_000_000
    res = pr.statistics(z1, z2, z1n)
    for name, val, bound in res:
        print(f"{name}: {val:.3e} (bound {bound:.3e})")
    bad = [(n, v, b) for n, v, b in res if not v < b]
    assert not bad, bad


def test_layout_invariance_of_the_restatement():
    """A row's draws depend on its global index only: a window of a larger fill, and a base shifted into the rows."""
    a1, a2 = pr.noise(5, 2, 3, 64, row_base=1000)
    b1, b2 = pr.noise(5, 2, 3, 16, row_base=1000, row0=20)
    c1, _ = pr.noise(5, 2, 3, 16, row_base=1020)
    d1, _ = pr.noise(5, 2, 1, 64, row_base=1000, step0=2)
    assert np.array_equal(a1[:, 20:36], b1) and np.array_equal(a2[:, 20:36], b2) and np.array_equal(b1, c1) and np.array_equal(a1[2:], d1)
    assert not np.array_equal(a1, a2) and not np.array_equal(a1, pr.noise(5, 3, 3, 64, row_base=1000)[0])


def test_counter_layout_is_injective():
    """(counter, key) maps back to the field tuple: 10^6 random tuples and every combination of the fields' edge values."""
    rng = np.random.default_rng(1)
    n = 1_000_000
    r64 = lambda: rng.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, n, dtype=np.uint64)
    fields = [r64(), rng.integers(0, 1 << 32, n, dtype=np.uint64), rng.integers(0, 1 << 29, n, dtype=np.uint64), rng.integers(0, 2, n, dtype=np.uint64),
              rng.integers(0, 3, n, dtype=np.uint64), r64()]
    axes = ([0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1], [0, 1, (1 << 32) - 1], [0, 1, 499, (1 << 29) - 1], [0, 1], [0, 1, 2],
            [0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1])
    edges = np.stack(np.meshgrid(*[np.array(v, dtype=np.uint64) for v in axes], indexing="ij")).reshape(6, -1)
    assert edges.dtype == np.uint64
    fields = [np.concatenate([f, e]) for f, e in zip(fields, edges)]
    ctr, key = pr.pack(*fields)
    assert ctr.dtype == np.uint32 and key.dtype == np.uint32
    back = pr.unpack(ctr, key)
    for f, b in zip(fields, back):
        assert np.array_equal(f, b)
    # and distinct tuples give distinct 192-bit words
    e_ctr, e_key = pr.pack(*edges)
    packed = np.concatenate([e_ctr, e_key], axis=-1)
    assert len(np.unique(packed, axis=0)) == edges.shape[1]
