"""GPU: the six-product PC chain kernels (csrc/trunk_bf16x9.hip: pc_step_chain_kernel_bf16x6 and its seeded twin) after their fp32 side
work was cut down (csrc/trunk_bf16x9.h, the NPROD == 6 forms: the ReLU as one integer maximum on the bits, the heads' Linear(256, 3)
epilogue as one fma chain per output, the second ring slot and the staged fp32 operands read through pinned base registers + immediates).
The arithmetic moved (one rounding fewer per product of the epilogue), the LDS addresses are formed differently: held here, on a shape
that reaches every one of them, to the rules the kernel was admitted under - nothing here is a new tolerance:

  MARGIN x the fp32 oracle's own error against float64 (tests/f64_reference.py, tests/test_gpu_f64_score.py), each head on its own;
  GATE_VS_F32 x the fp32 chain kernel's error on the same rows (tests/test_gpu_bf16x9.py);
  bit equality of a batch alone and inside a two-batch launch, and of the seeded kernel and the injected-noise kernel;
  the PC-100 limits against the nine-product kernel (tests/test_gpu_fullsize.py).

Shape: 6 clouds x 43 candidates = 258 rows = three workgroups of 128.  The second one's rows 128..255 lie in clouds 2, 3, 4 and 5 -
four clouds, so the fourth staged cvec + tvec row (the highest LDS address the kernel reads) is read - and the third has two live rows.
(The two-batch case cannot have it: a batch of a group must be whole workgroups.  It takes the smallest batch of K = 43 that is.)

Measured (MI355X): float64 rule, worst head 0.39 x (seed0) and 0.90 x (trained) of the yardstick; against the fp32 chain kernel 1.10 and
1.14 (rule 1.5); PC-100 six against nine: rotation p99.9 1.4e-5, max 3.2e-5, translation 3.9e-7."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import f64_reference as fr
from oracle import genpose_oracle as go

from test_gpu_bf16x9 import GATE_VS_F32, _inputs, _net
from test_gpu_f64_score import _net as _net_of
from test_gpu_fullsize import PC100_ROT_MAX, PC100_ROT_P999, PC100_TRANS_RTOL, _pose_errors
from test_gpu_x6_trunk import _sampler

B, K = 6, 43
_host = {}


def _case(which, scale):
    """inputs of the 258-row shape drawn as f64_reference.inputs draws its own (its seed table names only its four shapes), the float64
    score at t = 1 and the fp32 oracle's: computed once, read-only"""
    if (which, scale) not in _host:
        g = torch.Generator().manual_seed(1000 * B + 10 * K + int(scale))
        feat = torch.randn(B, 1024, generator=g).abs()
        pose = torch.randn(B * K, 9, generator=g) * scale
        centre = torch.randn(B, 3, generator=g) * 0.3
        ref = fr.evaluate(fr.state_dict64(which, "score"), "score", feat, K, pose, 1.0)
        f32 = fr.evaluate(fr.state_dict(which, "score"), "score", feat, K, pose, 1.0)
        _host[which, scale] = dict(feat=feat, pose=pose, centre=centre, ref=ref, f32=f32)
    return _host[which, scale]


def _first(which, scale, arith):
    """the first score evaluation (t = 1) of a PC sampler on the case's rows: 6 | 'f32mfma'"""
    c = _case(which, scale)
    net = _net_of(which, "score")
    smp = _sampler(net, B, K, 2, 1, arith, use_graph=False)
    smp.cvec.copy_(net.cloud_embed(c["feat"].cuda())), smp.centre.copy_(c["centre"].cuda()), smp.x.copy_(c["pose"].cuda())
    smp.z1.zero_(), smp.z2.zero_()
    smp.score.fill_(float("nan"))
    smp.launch_step(0)
    torch.cuda.synchronize()
    return smp.score.clone()


@pytest.mark.parametrize("which", ["seed0", "trained"])
def test_first_evaluation_against_float64_and_the_fp32_chain(which):
    """Cases 1 and 2: per head, at most MARGIN x the fp32 oracle's own error (f64_reference.e_oracle_cell, the yardstick of the cell) on both
    pose scales; and the worst head error over the two scales at most GATE_VS_F32 x the fp32 chain kernel's on the same rows."""
    E = fr.e_oracle_cell("score", 1.0)["score"]
    worst = {6: [0.0] * 3, "f32mfma": [0.0] * 3}
    for scale in fr.POSE_SCALES:
        c = _case(which, scale)
        own = fr.block_error(c["f32"], c["ref"])
        for arith in worst:
            e = fr.block_error(_first(which, scale, arith), c["ref"])
            worst[arith] = [max(a, b) for a, b in zip(worst[arith], e)]
            print(f"x6 diet | {which:7s} | x{scale:<4g} | {str(arith):7s} | " + " | ".join(
                f"head {j} {e[j]:.2e} ({e[j] / E[j]:.3f} x E, oracle here {own[j]:.2e})" for j in range(3)))
    for j in range(3):
        print(f"x6 diet | {which:7s} | head {j} | yardstick {E[j]:.2e} | six {worst[6][j]:.2e} ({worst[6][j] / E[j]:.3f} x) | fp32 chain "
              f"{worst['f32mfma'][j]:.2e} | six / fp32 chain {worst[6][j] / worst['f32mfma'][j]:.3f}")
    assert all(e6 <= fr.MARGIN * eo for e6, eo in zip(worst[6], E)), (worst[6], E)
    assert all(e6 <= GATE_VS_F32 * e32 for e6, e32 in zip(worst[6], worst["f32mfma"])), worst


def test_a_batch_alone_equals_the_batch_in_a_group():
    """Case 3: two batches in one launch (groups = 2), six steps with the trajectory - each batch computes alone, to the bit, what it
    computes inside the group.  The chain plan admits several batches per launch only when a batch is whole workgroups (gp_pc_layout: a
    workgroup must not straddle two batches), which 258 rows are not: with K = 43 the smallest batch it admits is 128 clouds = 5 504 rows
    = 43 workgroups, whose cloud boundaries fall on every position of a workgroup (three- and four-cloud spans among them)."""
    net = _net()
    n, G, B = 6, 2, 128
    feat, centre, x0, z1, z2 = (t.cuda() for t in _inputs(G * B, K, n, 643))
    cvec = net.cloud_embed(feat)
    with pytest.raises(ValueError):  # the 258-row batch of the other cases, two to a launch: refused before anything runs
        _sampler(net, 2 * 6, K, n, 2, 6, use_graph=False)
    xs, mx = _sampler(net, G * B, K, n, G, 6, record_traj=True, use_graph=False).run(cvec, centre, x0, z1, z2)
    torch.cuda.synchronize()
    assert torch.isfinite(mx).all()
    R1 = B * K
    for b in range(G):
        one = _sampler(net, B, K, n, 1, 6, record_traj=True, use_graph=False)
        x1, m1 = one.run(cvec[b * B:(b + 1) * B], centre[b * B:(b + 1) * B], x0[b * R1:(b + 1) * R1], z1[:, b * R1:(b + 1) * R1].contiguous(),
                         z2[:, b * R1:(b + 1) * R1].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(m1, mx[b * R1:(b + 1) * R1]), b
        assert torch.equal(x1, xs[b * R1:(b + 1) * R1]), b


def test_seeded_kernel_equals_the_injected_noise_kernel():
    """Case 4: pc_step_chain_seeded_kernel_bf16x6 against the unseeded kernel on gp_pc_noise_fill's buffers for the same seed state - poses,
    trajectory and partial sums bit for bit."""
    from genpose_amd.samplers import pc_noise_fill
    net = _net()
    n, seed = 6, 0xD1E7
    feat, centre, x0, _, _ = (t.cuda() for t in _inputs(B, K, 1, 644))
    cvec = net.cloud_embed(feat)
    seeded = _sampler(net, B, K, n, 1, 6, record_traj=True, seed=seed)
    plain = _sampler(net, B, K, n, 1, 6, record_traj=True)
    assert seeded.z1 is None
    xs, m = seeded.run(cvec, centre, x0, run_index=3)
    z1, z2 = pc_noise_fill(seed, 3, n, B * K, "cuda")
    xs_p, m_p = plain.run(cvec, centre, x0, z1, z2)
    torch.cuda.synchronize()
    assert torch.isfinite(m).all() and torch.equal(m, m_p) and torch.equal(xs, xs_p) and torch.equal(seeded.partials, plain.partials)


def test_pc100_against_nine_products():
    """Case 5: PC-100 on 3 x 50 rows, the same draws: six products against nine within the PC-100 limits."""
    net = _net()
    B5, K5, n = 3, 50, 100
    feat, centre, x0, z1, z2 = (t.cuda() for t in _inputs(B5, K5, n, 645))
    x0 = x0 * (float(go.ve_sigma(1.0)) / 50.0)  # the prior's scale at t = 1
    cvec = net.cloud_embed(feat)
    out = {arith: _sampler(net, B5, K5, n, 1, arith).run(cvec, centre, x0, z1, z2)[1].cpu().numpy().copy() for arith in (9, 6)}
    p999, mx, trans = _pose_errors(out[6], out[9])
    print(f"x6 diet | PC-100, 3 clouds x 50, six vs nine products: rotation p99.9 {p999:.2e} max {mx:.2e}, translation (rel) {trans:.2e} "
          f"(limits {PC100_ROT_P999:.0e} / {PC100_ROT_MAX:.0e} / {PC100_TRANS_RTOL:.0e})")
    assert np.isfinite(out[6]).all() and not np.array_equal(out[6], out[9])
    assert p999 < PC100_ROT_P999 and mx < PC100_ROT_MAX and trans < PC100_TRANS_RTOL
