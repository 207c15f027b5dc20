"""GPU: the bf16x9 chain launchers (gp_pc_step_bf16x9, its seeded twin, gp_heun_step_bf16x9) stage cvec, tvec_all and the fp32 biases /
output layer with 16-byte loads and refuse a pointer that is not 16-byte aligned with GP_EINVAL before anything is launched
(include/genpose_hip.h).  The aligned launch of the same sampler is accepted."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, K = 3, 43


def _net():
    from genpose_amd.scorenet import ScoreNetHIP
    from genpose_amd.weights_synth import make_state_dict
    return ScoreNetHIP(make_state_dict(0, "score"), "cuda")


def _off_by_one_float(t):
    buf = torch.zeros(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("which", ["cvec", "tvec_all"])
@pytest.mark.parametrize("kind", ["pc", "pc_seeded", "heun"])
def test_misaligned_staged_operand_is_refused(kind, which):
    from genpose_amd._lib import GenposeHipError
    from genpose_amd.samplers import HeunSampler, PCSampler
    net = _net()
    if kind == "heun":
        smp = HeunSampler(net, B, K, 2, "cuda", tile=128, use_graph=False)
        smp._write_schedule(1.0, 1e-5)
    else:
        smp = PCSampler(net, B, K, 2, "cuda", tile=128, trunk="bf16x9", use_graph=False, **({"seed": 1} if kind == "pc_seeded" else {}))
        if kind == "pc":
            smp.z1.zero_(), smp.z2.zero_()
        else:
            smp._write_seed_state(0, None)
    assert "bf16x9" in smp.kernel_name
    smp.cvec.zero_(), smp.centre.zero_(), smp.x.zero_()
    smp.launch_step(0)  # aligned: accepted
    torch.cuda.synchronize()
    setattr(smp, which, _off_by_one_float(getattr(smp, which)))
    with pytest.raises(GenposeHipError, match="GP_EINVAL"):
        smp.launch_step(0)
    torch.cuda.synchronize()
