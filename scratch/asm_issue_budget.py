"""Instruction classes per kernel of ONE csrc/*.hip file, from the device assembly the build's flags give (CPU only: hipcc cross-compiles
for gfx950 without a GPU).  For profiles/x6_issue_budget.txt: a kernel with one wave per SIMD pays the vector issue of everything it
places beside its MFMAs, so the table is what the kernel ISSUES, class by class - nothing here is checked against anything.

  static    every instruction of the kernel's text once (both arms of a branch)
  dynamic   the same with the body of each loop (a label that a later branch jumps back to) counted `trips` times; loops are listed
            per kernel as L0, L1, ... in text order with their label, size and MFMA count, and named on the command line by that
            ordinal or by the label:  --trips 'pc_step_chain.*bf16x6:L0=3'
  loop region   a third column: the part of the static text from the kernel's first MFMA on (what can sit beside MFMAs at all)

Classes: MFMA; the accumulator moves (v_accvgpr_read / _write); VALU by mnemonic group (packed fp32, fp32 add / sub, mul, fma / fmac,
max / min with the canonicalising `v_max_f32 v, v, v` form on a line of its own, conversions, 32-bit integer adds, the carry pairs of
64-bit address arithmetic, shifts / logic / permutes, moves, cross-lane, the rest); s_nop (instructions and the wait states they
carry); s_waitcnt; LDS reads and writes by width; global / scratch loads and stores; barriers; branches; the other scalar instructions.

    python scratch/asm_issue_budget.py genpose_amd/csrc/trunk_bf16x9.hip [--kernel REGEX] [--trips 'REGEX:L0=3' ...] [--asm FILE.s]
                                       [--keep-asm FILE.s] [--flags '...']

--asm reads an assembly file made earlier (of another commit, say) instead of compiling.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLASSES = ["MFMA", "v_accvgpr_read", "v_accvgpr_write", "VALU packed fp32 (v_pk_*_f32)", "VALU fp32 add/sub", "VALU fp32 mul", "VALU fp32 fma/fmac",
           "VALU fp32 max/min", "  of them v_max_f32 v, v, v", "VALU max/min/med3, other types", "VALU convert (v_cvt_*)", "VALU int add/sub 32 (v_add_u32 ...)",
           "VALU 64-bit address carry (v_add_co / v_addc_co)", "VALU shift/logic/perm", "VALU move (v_mov / v_cndmask)", "VALU cross-lane (dpp, readlane, permlane, bpermute)",
           "VALU other", "s_nop", "  wait states in them", "s_waitcnt", "ds_read_b128", "ds_read, narrower", "ds_write_b128", "ds_write, narrower", "DS other",
           "global_load_dwordx4", "global_load, narrower", "global_store", "scratch load/store", "VMEM other", "s_barrier", "branch", "SALU / SMEM other"]


def classify(mn, ops):
    """-> list of (class, count) for one instruction"""
    if mn.startswith("v_mfma") or mn.startswith("v_smfmac"):
        return [("MFMA", 1)]
    if mn.startswith("v_accvgpr_read"):
        return [("v_accvgpr_read", 1)]
    if mn.startswith("v_accvgpr_write") or mn.startswith("v_accvgpr_mov"):
        return [("v_accvgpr_write", 1)]
    if mn.startswith("v_"):
        base = re.sub(r"_(e32|e64|dpp|sdwa|e64_dpp)$", "", mn)
        if "dpp" in mn or "dpp" in ops or re.match(r"v_(readlane|readfirstlane|writelane|permlane|swap|mov_b32_dpp)", base):
            return [("VALU cross-lane (dpp, readlane, permlane, bpermute)", 1)]
        if re.match(r"v_pk_\w+_f32$", base):
            return [("VALU packed fp32 (v_pk_*_f32)", 1)]
        if re.match(r"v_(add|sub|subrev)_f32$", base):
            return [("VALU fp32 add/sub", 1)]
        if base == "v_mul_f32":
            return [("VALU fp32 mul", 1)]
        if re.match(r"v_(fma|fmac|mad|mac|fmaak|fmamk)_f32$", base):
            return [("VALU fp32 fma/fmac", 1)]
        if re.match(r"v_(max|min|med3|max3|min3)_f32$", base):
            r = [("VALU fp32 max/min", 1)]
            o = [x.strip() for x in ops.split(",")]
            if base == "v_max_f32" and len(o) == 3 and o[1] == o[2]:
                r.append(("  of them v_max_f32 v, v, v", 1))
            return r
        if re.match(r"v_(max|min|med3|max3|min3)_", base):
            return [("VALU max/min/med3, other types", 1)]
        if base.startswith("v_cvt_"):
            return [("VALU convert (v_cvt_*)", 1)]
        if re.match(r"v_(add_co|addc_co|sub_co|subb_co|subrev_co|subbrev_co)_u32$", base):
            return [("VALU 64-bit address carry (v_add_co / v_addc_co)", 1)]
        if re.match(r"v_(add|sub|subrev|add3|lshl_add|add_lshl|mad_u|mad_i|mul_lo|mul_hi|mul_u32_u24|mul_i32_i24|mad_u32_u24|mad_i32_i24)", base):
            return [("VALU int add/sub 32 (v_add_u32 ...)", 1)]
        if re.match(r"v_(lshl|lshr|ashr|and|or|xor|not|bfe|bfi|perm|alignbit|alignbyte|and_or|or3|lshl_or|xad)", base):
            return [("VALU shift/logic/perm", 1)]
        if re.match(r"v_(mov|cndmask)", base):
            return [("VALU move (v_mov / v_cndmask)", 1)]
        return [("VALU other", 1)]
    if mn == "s_nop":
        return [("s_nop", 1), ("  wait states in them", int(ops.strip() or 0) + 1)]
    if mn.startswith("s_waitcnt"):
        return [("s_waitcnt", 1)]
    if mn == "s_barrier":
        return [("s_barrier", 1)]
    if mn.startswith("s_cbranch") or mn in ("s_branch", "s_endpgm", "s_setpc_b64", "s_swappc_b64"):
        return [("branch", 1)]
    if mn.startswith("ds_"):
        if mn.startswith("ds_read_b128") or mn.startswith("ds_load_b128"):
            return [("ds_read_b128", 1)]
        if mn.startswith("ds_read") or mn.startswith("ds_load"):
            return [("ds_read, narrower", 1)]
        if mn.startswith("ds_write_b128") or mn.startswith("ds_store_b128"):
            return [("ds_write_b128", 1)]
        if mn.startswith("ds_write") or mn.startswith("ds_store"):
            return [("ds_write, narrower", 1)]
        if mn.startswith("ds_bpermute") or mn.startswith("ds_permute") or mn.startswith("ds_swizzle"):
            return [("VALU cross-lane (dpp, readlane, permlane, bpermute)", 1)]
        return [("DS other", 1)]
    if mn.startswith("global_load_dwordx4"):
        return [("global_load_dwordx4", 1)]
    if mn.startswith("global_load") or mn.startswith("flat_load") or mn.startswith("buffer_load"):
        return [("global_load, narrower", 1)]
    if mn.startswith("global_store") or mn.startswith("flat_store") or mn.startswith("buffer_store"):
        return [("global_store", 1)]
    if mn.startswith("scratch_"):
        return [("scratch load/store", 1)]
    if mn.startswith(("global_", "flat_", "buffer_")):
        return [("VMEM other", 1)]
    if mn.startswith("s_"):
        return [("SALU / SMEM other", 1)]
    return [("VALU other", 1)]


def kernels_of(text):
    """-> {kernel name: [(label or None, mnemonic, operands)]} for the .amdhsa kernels of an assembly file"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur = collections.OrderedDict(), None
    for line in text.splitlines():
        s = line.split(";")[0].rstrip()
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m:
            lab = m.group(1)
            if lab in names:
                cur = out.setdefault(lab, [])
            elif cur is not None and lab.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None:
                cur.append((lab, None, None))
            continue
        if cur is None:
            continue
        s = s.strip()
        if not s or s.startswith("."):
            continue
        parts = s.split(None, 1)
        cur.append((None, parts[0], parts[1] if len(parts) > 1 else ""))
    return out


def loops_of(body):
    """[(header label, sorted entry indices of the loop's body)] in text order.  A loop is a label that a later branch jumps back to AND
    that reaches that branch (a cold block laid out behind the kernel's end jumps back too, and is no loop); its body is the natural
    loop: the entries that reach the back branch without passing the header."""
    at = {lab: i for i, (lab, _, _) in enumerate(body) if lab}
    n = len(body)
    succ = [[] for _ in range(n)]
    for i, (lab, mn, ops) in enumerate(body):
        if mn and (mn.startswith("s_cbranch") or mn == "s_branch") and ops.strip() in at:
            succ[i].append(at[ops.strip()])
        if mn not in ("s_branch", "s_endpgm", "s_setpc_b64") and i + 1 < n:
            succ[i].append(i + 1)
    pred = [[] for _ in range(n)]
    for i, ss in enumerate(succ):
        for s in ss:
            pred[s].append(i)
    members = {}
    for i, (lab, mn, ops) in enumerate(body):
        if mn and (mn.startswith("s_cbranch") or mn == "s_branch"):
            h = at.get(ops.strip(), n)
            if h < i:
                seen, todo = {h, i}, [i]
                while todo:  # backwards from the latch, stopping at the header
                    for p in pred[todo.pop()]:
                        if p not in seen:
                            seen.add(p)
                            todo.append(p)
                if all(x >= h for x in seen):  # the header dominates what reaches the latch: a loop, not a jump back from a cold block
                    members.setdefault(ops.strip(), set()).update(seen)
    return sorted(((lab, sorted(m)) for lab, m in members.items()), key=lambda x: at[x[0]])


def count(body, weight=None, start=0):
    c = collections.Counter()
    for i, (lab, mn, ops) in enumerate(body):
        if mn is None or i < start:
            continue
        for k, n in classify(mn, ops):
            c[k] += n * (weight[i] if weight else 1)
    return c


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool] + list(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source")
    ap.add_argument("--kernel", default=".", help="regex on the (demangled) kernel name")
    ap.add_argument("--trips", action="append", default=[], help="KERNEL_REGEX:L<ordinal>|<label>=N")
    ap.add_argument("--asm", help="read this assembly instead of compiling")
    ap.add_argument("--keep-asm", help="write the assembly here")
    ap.add_argument("--flags", help="replace the build's flags")
    args = ap.parse_args()
    if args.asm:
        text = open(args.asm).read()
    else:
        from genpose_amd import build as gb
        flags = args.flags.split() if args.flags else [f for f in gb.FLAGS if f != "-fPIC"]
        dst = args.keep_asm or os.path.join(tempfile.mkdtemp(), "out.s")
        cmd = [gb._hipcc()] + flags + ["--cuda-device-only", "-S", args.source, "-o", dst]
        print("# " + " ".join(cmd))
        subprocess.check_call(cmd)
        text = open(dst).read()
    ks = kernels_of(text)
    pretty = demangle(list(ks))
    for name, body in ks.items():
        if not re.search(args.kernel, pretty[name]):
            continue
        loops = loops_of(body)
        weight = [1] * len(body)
        given = []
        for spec in args.trips:
            rx, rest = spec.rsplit(":", 1)
            which, n = rest.split("=")
            if not re.search(rx, pretty[name]):
                continue
            for j, (lab, idx) in enumerate(loops):
                if which in (f"L{j}", lab):
                    for i in idx:
                        weight[i] *= int(n)
                    given.append(f"L{j} x {n}")
        first_mfma = next((i for i, (_, mn, _) in enumerate(body) if mn and mn.startswith("v_mfma")), len(body))
        st, dy, lr = count(body), count(body, weight), count(body, None, first_mfma)
        print(f"\n== {pretty[name]}")
        for j, (lab, idx) in enumerate(loops):
            inner = count([body[i] for i in idx])
            print(f"   loop L{j} {lab}: {sum(1 for i in idx if body[i][1])} instructions, {inner['MFMA']} MFMAs")
        print(f"   trips: {', '.join(given) if given else 'none given (dynamic = static)'}")
        print(f"   {'class':66s} {'static':>8s} {'dynamic':>8s} {'from first MFMA':>16s}")
        for k in CLASSES:
            if st[k] or dy[k]:
                print(f"   {k:66s} {st[k]:8d} {dy[k]:8d} {lr[k]:16d}")
        sub = lambda c: sum(v for k, v in c.items() if not k.startswith("  "))
        valu = lambda c: sum(v for k, v in c.items() if k.startswith("VALU"))
        print(f"   {'all VALU classes':66s} {valu(st):8d} {valu(dy):8d} {valu(lr):16d}")
        print(f"   {'everything but MFMA':66s} {sub(st) - st['MFMA']:8d} {sub(dy) - dy['MFMA']:8d} {sub(lr) - lr['MFMA']:16d}")


if __name__ == "__main__":
    main()
