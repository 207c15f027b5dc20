"""GPU: every step entry point's FIRST launch in a fresh process.  The suite runs in one long process in which an earlier test has usually
set a kernel's dynamic-LDS attribute already, so a launch path that forgets to set it (csrc/gp_common.h: gp_prepare_lds / gp_launch) would
pass everywhere else - and come back as GP_ELAUNCH in a user's process.  One child process (tests/cold_launch_child.py) makes the calls;
this test reads its one line."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HS = 0x100  # GP_PLAN_HEADSPLIT
EXPECTED = ([f"gp_score_eval_plan[{p}]" for p in (128, 64, 32, 16)]
            + [f"gp_pc_step_plan[score, {p}]" for p in (128, 64, 32, 16, 16 | HS)]
            + [f"gp_pc_step_plan[energy, {p}]" for p in (128, 16)]
            + [f"gp_pc_step_plan_seeded[{p}]" for p in (128, 64, 32, 16, 16 | HS)]
            + [f"gp_{s}_{form}[{p}]" for s in ("heun", "dpm2m") for form, plans in (("step_plan", (128, 64, 32, 16)), ("solve_tile", (64, 32, 16)))
               for p in plans]
            + ["gp_pc_step_bf16x9", "gp_pc_step_bf16x9_seeded", "gp_heun_step_bf16x9", "gp_dpm2m_step_bf16x9", "gp_heun_likelihood_step",
               "gp_score_div", "gp_energy_score", "gp_score_div_exact"])


def test_first_launch_of_every_step_entry_point_in_a_fresh_process():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cold_launch_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    line = json.loads(lines[0])
    assert line["ok"] and p.returncode == 0, (line.get("failed"), p.stderr[-3000:])
    # GP_OK, a clean synchronise, finite buffers and the same bits from a second identical call - for every one of these, in this order
    assert line["calls"] == EXPECTED
