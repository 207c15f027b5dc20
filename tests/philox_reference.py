"""numpy restatement of the seeded PC sampler's noise (genpose_amd/csrc/philox.h; DESIGN.md "seeded noise"): Philox4x32-10 as published
(Salmon, Moraes, Dror, Shaw, SC'11) on uint32 / uint64 arrays, the counter layout, and Box-Muller in float32 with numpy's
log / sqrt / sin / cos.  A helper for tests/test_philox_cpu.py and tests/test_gpu_seeded_noise.py, not a test."""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)
STREAM_LANGEVIN, STREAM_PREDICTOR = 0, 1
TWO_PI = np.float32(6.2831854820251465)
Z_MAX = math.sqrt(48.0 * math.log(2.0))  # u1 >= 2^-24: |z| <= 5.768


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] uint32 -> [..., 4] uint32."""
    c = [np.asarray(ctr[..., j], dtype=np.uint32).copy() for j in range(4)]
    k0, k1 = np.asarray(key[..., 0], dtype=np.uint32).copy(), np.asarray(key[..., 1], dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0, p1 = M0 * c[0].astype(np.uint64), M1 * c[2].astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & MASK32).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & MASK32).astype(np.uint32)
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
            k0, k1 = k0 + W0, k1 + W1
    return np.stack(c, axis=-1)


def pack(seed, run, step, stream, block, row):
    """Field tuple (arrays broadcast together; seed, row: uint64) -> (ctr [..., 4], key [..., 2]) uint32.
    key = seed lo, hi; ctr = row lo, row hi, run, step << 3 | stream << 2 | block  (step < 2^29)."""
    seed, run, step, stream, block, row = np.broadcast_arrays(np.asarray(seed, np.uint64), np.asarray(run, np.uint64), np.asarray(step, np.uint64),
                                                               np.asarray(stream, np.uint64), np.asarray(block, np.uint64), np.asarray(row, np.uint64))
    assert (step < (1 << 29)).all() and (run < (1 << 32)).all() and (stream < 2).all() and (block < 3).all()
    u32 = lambda v: (v & MASK32).astype(np.uint32)
    ctr = np.stack([u32(row), u32(row >> np.uint64(32)), u32(run), u32(step << np.uint64(3) | stream << np.uint64(2) | block)], axis=-1)
    key = np.stack([u32(seed), u32(seed >> np.uint64(32))], axis=-1)
    return ctr, key


def unpack(ctr, key):
    """(ctr, key) -> (seed, run, step, stream, block, row), uint64 arrays: the layout's inverse."""
    c, k = ctr.astype(np.uint64), key.astype(np.uint64)
    return (k[..., 0] | k[..., 1] << np.uint64(32), c[..., 2], c[..., 3] >> np.uint64(3), (c[..., 3] >> np.uint64(2)) & np.uint64(1),
            c[..., 3] & np.uint64(3), c[..., 0] | c[..., 1] << np.uint64(32))


def uniform24(w):
    """uint32 words -> float32 uniforms on the 2^-24 grid in (0, 1] (exact in float32)."""
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(1.0)) * np.float32(2.0 ** -24)


def words(seed, run, step, stream, rows):
    """The 12 raw words of every row in `rows` (uint64 array [...]) -> [..., 12] uint32."""
    out = []
    for b in range(3):
        ctr, key = pack(seed, run, step, stream, b, rows)
        out.append(philox4x32_10(ctr, key))
    return np.concatenate(out, axis=-1)


def normals(seed, run, step, stream, rows):
    """The nine float32 normals of every row in `rows` for one stream at one step -> [..., 9]."""
    w = words(seed, run, step, stream, np.asarray(rows, np.uint64))
    u1, u2 = uniform24(w[..., 0:10:2]), uniform24(w[..., 1:10:2])  # pairs 0..4 (of the sixth pair nothing is used)
    r = np.sqrt(np.float32(-2.0) * np.log(u1))
    th = TWO_PI * u2
    z = np.stack([r * np.cos(th), r * np.sin(th)], axis=-1).reshape(w.shape[:-1] + (10,))
    assert z.dtype == np.float32
    return z[..., :9]


def noise(seed, run, num_steps, nrows, row_base=0, step0=0, row0=0):
    """What gp_pc_noise_fill writes: (z_langevin, z_predictor), [num_steps, nrows, 9] float32 each."""
    rows = np.uint64(row_base) + np.uint64(row0) + np.arange(nrows, dtype=np.uint64)
    z = [np.stack([normals(seed, run, step0 + s, stream, rows) for s in range(num_steps)]) for stream in (STREAM_LANGEVIN, STREAM_PREDICTOR)]
    return z[0], z[1]


def _ndtr(x):
    from scipy.special import ndtr
    return ndtr(x)


def _corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / math.sqrt((a * a).mean() * (b * b).mean()))


def statistics(z1, z2, z1_next_seed):
    """Checks on draws z1, z2 [n, R, 9] (the two streams of one seed) and z1_next_seed (stream 0 of seed + 1, same steps and rows).
    Returns [(name, |statistic|, bound)]: every bound is FACTOR = 5 times the statistic's own sampling error under N(0, 1) i.i.d. at the
    sample size used (mean: 1/sqrt N; variance: sqrt(2/N); skewness: sqrt(6/N); excess kurtosis: sqrt(24/N); a correlation over M pairs:
    1/sqrt M), and the Kolmogorov-Smirnov distance is held to its 1 % critical value 1.63/sqrt N.  (The truncation at 5.77 sigma moves
    none of these by more than 1e-6.)"""
    F = 5.0
    z = np.concatenate([z1.ravel(), z2.ravel()]).astype(np.float64)
    N = z.size
    m, v = z.mean(), z.var()
    c = z - m
    out = [("mean", abs(m), F / math.sqrt(N)), ("variance", abs(v - 1.0), F * math.sqrt(2.0 / N)),
           ("skewness", abs((c ** 3).mean() / v ** 1.5), F * math.sqrt(6.0 / N)),
           ("excess kurtosis", abs((c ** 4).mean() / v ** 2 - 3.0), F * math.sqrt(24.0 / N))]
    zs = np.sort(z)
    cdf = _ndtr(zs)
    i = np.arange(1, N + 1, dtype=np.float64)
    out.append(("Kolmogorov-Smirnov", float(max((i / N - cdf).max(), (cdf - (i - 1) / N).max())), 1.63 / math.sqrt(N)))
    M = z1[..., 0].size
    worst = max(abs(_corr(z1[..., a], z1[..., b])) for a in range(9) for b in range(a + 1, 9))
    out.append(("components of a row (worst of 36 pairs)", worst, F / math.sqrt(M)))
    out.append(("consecutive rows", abs(_corr(z1[:, :-1], z1[:, 1:])), F / math.sqrt(z1[:, 1:].size)))
    out.append(("consecutive steps", abs(_corr(z1[:-1], z1[1:])), F / math.sqrt(z1[1:].size)))
    out.append(("the two streams", abs(_corr(z1, z2)), F / math.sqrt(z1.size)))
    out.append(("seeds s and s + 1", abs(_corr(z1, z1_next_seed)), F / math.sqrt(z1.size)))
    return out
