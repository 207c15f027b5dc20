"""CPU (no GPU): gp_rk45_phase_bf16x9 - declared in include/genpose_hip.h, exported, bound in _lib.SIGNATURES with the header's arity and
argument kinds (tests/test_abi_and_host.py checks names only), and the host-side option values."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prototype(name):
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/genpose_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _kind(decl):
    if "*" in decl or decl.startswith("gp_stream_t"):
        return "pointer"
    return "double" if decl.startswith("double") else "int"


@pytest.mark.parametrize("name", ["gp_rk45_phase_bf16x9", "gp_rk45_phase_model", "gp_pc_step_bf16x9"])
def test_signature_matches_header(name):
    from genpose_amd import _lib
    args = _prototype(name)
    sig = _lib.SIGNATURES[name]
    assert len(sig) == len(args), (name, len(sig), len(args))
    for decl, ct in zip(args, sig):
        want = _kind(decl)
        got = "double" if ct is ctypes.c_double else ("int" if ct is ctypes.c_int else "pointer")
        assert want == got, (name, decl, ct)


def test_phase_bf16x9_is_phase_model_without_model_plan_probe_plus_the_packs():
    a, b = _prototype("gp_rk45_phase_bf16x9"), _prototype("gp_rk45_phase_model")
    drop = {"int model", "int plan", "const float *probe"}
    packs = ["const void *w_pose0_x9", "const void *w_pose2_x9", "const void *w_headx_x9"]
    assert a == [x for x in b[:-1] if x not in drop] + packs + [b[-1]]


def test_library_exports_it():
    from genpose_amd import _lib, build
    build.build()
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), "gp_rk45_phase_bf16x9")


def test_config_default():
    from genpose_amd.config import get_config
    assert get_config().ode_trunk is None and get_config(ode_trunk="bf16x9").ode_trunk == "bf16x9"
