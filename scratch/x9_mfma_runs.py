"""Static count for profiles/x9_kmajor_under_mfma.txt: in one kernel's gfx950 assembly (hipcc -save-temps, the device .s file), the
non-MFMA instructions - s_nop excluded - that sit in runs of more than 6 between two MFMAs, listed by the index of the MFMA the run
precedes.  Nothing is run; both arms of a branch are counted.

    python scratch/x9_mfma_runs.py FILE.s [kernel-name-substring] [--min 6]
"""
import re
import sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
path, kern = args[0], (args[1] if len(args) > 1 else "pc_step_chain_kernel_bf16x9")
thresh = int(sys.argv[sys.argv.index("--min") + 1]) if "--min" in sys.argv else 6
inside, runs, run, nmfma = False, [], 0, 0
for line in open(path):
    t = line.strip()
    if not inside:
        inside = bool(re.match(r"^\S*%s\S*:" % re.escape(kern), t)) and not t.startswith(".")
        continue
    if t.startswith(".Lfunc_end"):
        break
    if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
        continue
    op = t.split()[0]
    if op.startswith("v_mfma"):
        runs.append((nmfma, run))
        nmfma, run = nmfma + 1, 0
    elif op != "s_nop":
        run += 1
runs.append((nmfma, run))
long_runs = [(i, r) for i, r in runs if r > thresh]
print(f"{kern}: {nmfma} MFMAs (static), {sum(r for _, r in runs)} other instructions, {sum(r for _, r in long_runs)} of them in "
      f"{len(long_runs)} runs of more than {thresh}")
for i, r in long_runs:
    print(f"  before MFMA {i:5d}{' (after the last)' if i == nmfma else ''}: {r}")
