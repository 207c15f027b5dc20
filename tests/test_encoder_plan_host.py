"""CPU (no GPU): the encoder's launch plan (genpose_amd/encoder.py) - which kernel the constructor assigns to every (level, scale) under
every combination of its options, and the entry points a set-abstraction pass issues on either side of the two minimum batches.  Pure
host logic: the encoders are built on the CPU.  tests/test_gpu_encoder_plan.py holds the launches themselves to launch_plan()."""
import itertools

import pytest

from oracle import genpose_oracle as go

CODE = {"f": "f32mfma", "9": "bf16x9", "3": "bf16x3"}
# (precision, level1, level3) -> sa_kernels level by level (one letter per scale) | level3_kernel
KERNELS = {
    "light": {
        ("f32", None, None): "ff ff ff | f",
        ("f32", None, "bf16x9"): "ff ff ff | 9",
        ("f32", "bf16x9", None): "ff 99 ff | f",
        ("f32", "bf16x9", "bf16x9"): "ff 99 ff | 9",
        ("bf16x9", None, None): "ff ff 99 | f",
        ("bf16x9", None, "bf16x9"): "ff ff 99 | 9",
        ("bf16x9", "bf16x9", None): "ff 99 99 | f",
        ("bf16x9", "bf16x9", "bf16x9"): "ff 99 99 | 9",
        ("bf16x3", None, None): "ff 33 33 | f",
        ("bf16x3", None, "bf16x9"): "ff 33 33 | 9",
        ("bf16x3", "bf16x9", None): "ff 33 33 | f",
        ("bf16x3", "bf16x9", "bf16x9"): "ff 33 33 | 9",
    },
    "dense": {  # level 2 has 8 | 16 samples: no split kernel is instantiated for 8
        ("f32", None, None): "ff ff ff | f",
        ("f32", None, "bf16x9"): "ff ff ff | 9",
        ("f32", "bf16x9", None): "ff 99 ff | f",
        ("f32", "bf16x9", "bf16x9"): "ff 99 ff | 9",
        ("bf16x9", None, None): "ff ff f9 | f",
        ("bf16x9", None, "bf16x9"): "ff ff f9 | 9",
        ("bf16x9", "bf16x9", None): "ff 99 f9 | f",
        ("bf16x9", "bf16x9", "bf16x9"): "ff 99 f9 | 9",
        ("bf16x3", None, None): "ff 33 f3 | f",
        ("bf16x3", None, "bf16x9"): "ff 33 f3 | 9",
        ("bf16x3", "bf16x9", None): "ff 33 f3 | f",
        ("bf16x3", "bf16x9", "bf16x9"): "ff 33 f3 | 9",
    },
    "lighter": {  # one scale per level; level 1 is 64-64-128 at 32 samples (bf16x3 only), the GroupAll level is not the light encoder's
        ("f32", None, None): "f f f f | f",
        ("f32", None, "bf16x9"): "f f f f | f",
        ("f32", "bf16x9", None): "f f f f | f",
        ("f32", "bf16x9", "bf16x9"): "f f f f | f",
        ("bf16x9", None, None): "f f 9 f | f",
        ("bf16x9", None, "bf16x9"): "f f 9 f | f",
        ("bf16x9", "bf16x9", None): "f f 9 f | f",
        ("bf16x9", "bf16x9", "bf16x9"): "f f 9 f | f",
        ("bf16x3", None, None): "f 3 3 f | f",
        ("bf16x3", None, "bf16x9"): "f 3 3 f | f",
        ("bf16x3", "bf16x9", None): "f 3 3 f | f",
        ("bf16x3", "bf16x9", "bf16x9"): "f 3 3 f | f",
    },
}
F32, X3, X9, LDS, GA, PL = ("gp_sa_pre_mlp_max_layout", "gp_sa_pre_mlp_max_bf16x3", "gp_sa_pre_mlp_max_bf16x9", "gp_sa_lds_bf16x9", "gp_sa_groupall_bf16x9",
                            "gp_point_linear")


@pytest.fixture(scope="module")
def state_dicts():
    return {p: go.make_state_dict(0, "score", p) for p in KERNELS}


def _encoder(sd, params="light", **kw):
    from genpose_amd.encoder import Pointnet2EncoderHIP
    return Pointnet2EncoderHIP(sd, "cpu", params, **kw)


@pytest.mark.parametrize("params", list(KERNELS))
def test_kernel_of_every_scale_under_every_option(state_dicts, params):
    assert set(KERNELS[params]) == set(itertools.product(("f32", "bf16x9", "bf16x3"), (None, "bf16x9"), (None, "bf16x9")))
    for (precision, level1, level3), row in KERNELS[params].items():
        enc = _encoder(state_dicts[params], params, precision=precision, level1=level1, level3=level3)
        levels, l3 = row.split(" | ")
        want = {(k, i): CODE[c] for k, scales in enumerate(levels.split()) for i, c in enumerate(scales)}
        assert enc.sa_kernels == want, (params, precision, level1, level3)
        assert enc.level3_kernel == CODE[l3], (params, precision, level1, level3)
        assert (enc.precision, enc.level1, enc.level3) == (precision, level1 or "f32mfma", level3 or "f32mfma")


def test_launch_plan_on_either_side_of_both_minimum_batches(state_dicts):
    enc = _encoder(state_dicts["light"], precision="bf16x9", level1="bf16x9", level3="bf16x9")
    assert (enc.LEVEL1_BF16X9_MIN_CLOUDS, enc.LEVEL3_BF16X9_MIN_CLOUDS) == (64, 128)
    small = [F32, F32, PL, F32, F32, PL, X9, X9, PL, F32, F32]
    middle = [F32, F32, PL, LDS, LDS, PL, X9, X9, PL, F32, F32]
    large = [F32, F32, PL, LDS, LDS, PL, X9, X9, GA]
    assert enc.launch_plan(1) == enc.launch_plan(63) == small
    assert enc.launch_plan(64) == enc.launch_plan(127) == middle
    assert enc.launch_plan(128) == enc.launch_plan(640) == large
    # the thresholds are read through the instance at call time
    enc.LEVEL1_BF16X9_MIN_CLOUDS = enc.LEVEL3_BF16X9_MIN_CLOUDS = 1
    assert [enc.launch_plan(B) for B in (1, 63, 64, 127, 128)] == [large] * 5
    enc.LEVEL1_BF16X9_MIN_CLOUDS, enc.LEVEL3_BF16X9_MIN_CLOUDS = 128, 64  # each level by its own threshold
    assert enc.launch_plan(63) == small and enc.launch_plan(128) == large
    assert enc.launch_plan(64) == enc.launch_plan(127) == [F32, F32, PL, F32, F32, PL, X9, X9, GA]
    assert type(enc).LEVEL1_BF16X9_MIN_CLOUDS == 64 and type(enc).LEVEL3_BF16X9_MIN_CLOUDS == 128  # (the class is untouched)


def test_launch_plan_of_the_other_options_and_configurations(state_dicts):
    fp32 = [F32, F32, PL, F32, F32, PL, F32, F32, PL, F32, F32]
    for B in (1, 63, 64, 127, 128):  # no kernel with a minimum batch: the plan does not depend on B
        assert _encoder(state_dicts["light"]).launch_plan(B) == fp32
        assert _encoder(state_dicts["light"], precision="bf16x3").launch_plan(B) == [F32, F32, PL, X3, X3, PL, X3, X3, PL, F32, F32]
        assert _encoder(state_dicts["dense"], "dense", precision="bf16x3").launch_plan(B) == [F32, F32, PL, X3, X3, PL, F32, X3, PL, F32, F32]
        assert _encoder(state_dicts["lighter"], "lighter", precision="bf16x3").launch_plan(B) == [F32, PL, X3, PL, X3, PL, F32, PL, F32]
    # bf16x3 wins over both bf16x9 kernels of the grouping levels; the GroupAll level is independent of it
    enc = _encoder(state_dicts["light"], precision="bf16x3", level1="bf16x9", level3="bf16x9")
    assert enc.launch_plan(127) == [F32, F32, PL, X3, X3, PL, X3, X3, PL, F32, F32]
    assert enc.launch_plan(128) == [F32, F32, PL, X3, X3, PL, X3, X3, GA]
    enc = _encoder(state_dicts["dense"], "dense", precision="bf16x9", level1="bf16x9", level3="bf16x9")
    assert enc.launch_plan(63) == [F32, F32, PL, F32, F32, PL, F32, X9, PL, F32, F32]
    assert enc.launch_plan(128) == [F32, F32, PL, LDS, LDS, PL, F32, X9, GA]
    enc = _encoder(state_dicts["lighter"], "lighter", precision="bf16x9", level1="bf16x9", level3="bf16x9")
    assert enc.launch_plan(63) == enc.launch_plan(128) == [F32, PL, F32, PL, X9, PL, F32, PL, F32]


def test_a_subnormal_level1_weight_takes_only_its_scale_back(state_dicts):
    bad = dict(state_dicts["light"])
    key = "pts_encoder.SA_modules.1.mlps.0.layer1.conv.weight"
    W = bad[key].clone()
    W[3, 5] = 1e-40
    bad[key] = W
    enc = _encoder(bad, precision="bf16x9", level1="bf16x9", level3="bf16x9")
    assert enc.sa_kernels == {(0, 0): "f32mfma", (0, 1): "f32mfma", (1, 0): "f32mfma", (1, 1): "bf16x9", (2, 0): "bf16x9", (2, 1): "bf16x9"}
    assert enc.level3_kernel == "bf16x9"
    assert enc.launch_plan(63) == [F32, F32, PL, F32, F32, PL, X9, X9, PL, F32, F32]
    assert enc.launch_plan(64) == [F32, F32, PL, F32, LDS, PL, X9, X9, PL, F32, F32]
    assert enc.launch_plan(128) == [F32, F32, PL, F32, LDS, PL, X9, X9, GA]
