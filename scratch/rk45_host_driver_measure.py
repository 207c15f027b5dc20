"""Measurements behind profiles/rk45_host_driver.txt: a host-only change of the RK45 driver against its parent commit.

    python scratch/rk45_host_driver_measure.py devcode <parent.s> <this.s> <parent remarks> <this remarks>
        compares two device-only compiles of csrc/rk45.hip (build.py's FLAGS + --cuda-device-only -S -Rpass-analysis=kernel-resource-usage,
        stderr kept as the remarks file): per symbol the instruction stream (assembler comments stripped; the ordinals inside local labels
        follow the order of emission and are normalised), per kernel the .amdhsa_kernel descriptor, the amdhsa.kernels metadata entry and
        the resource-usage table.  No GPU.
    python scratch/rk45_host_driver_measure.py enqueue <tree root> <label> [calls]
        host time of one un-captured ODESampler._phase(3, None) call, 5 clouds x 50 candidates, use_graph=False, median over `calls` (400) calls
        (the call only; the synchronise is outside the timed region).  One tree per process: run the two trees in turn.
    python scratch/rk45_host_driver_measure.py paired <parent tree> <this tree>
        the same call of both trees in ONE process, call by call in turn (the parent's package is loaded under another name with its own
        library), and the C entry point alone - takes the placement of the process out of the comparison.
Both trees must be built (python -m genpose_amd.build)."""
import sys


def devcode(argv):
    import re
    import sys
    import hashlib


    def norm(l):
        l = l.split(";")[0].rstrip()
        return re.sub(r"\.L(BB|func_end|func_begin|tmp|post_getpc)\d+", r".L\1N", l)


    def parse(path):
        code, desc, meta = {}, {}, {}
        cur = kd = None
        lines = open(path).read().split("\n")
        i = 0
        while i < len(lines) and not lines[i].strip().startswith(".amdgpu_metadata"):
            l = norm(lines[i])
            i += 1
            if not l.strip():
                continue
            m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l)
            if m:
                kd = m.group(1)
                desc[kd] = []
                continue
            if l.strip() == ".end_amdhsa_kernel":
                kd = None
                continue
            if kd:
                desc[kd].append(l.strip())
                continue
            m = re.match(r"^([A-Za-z_][\w.$]*):", l)
            if m:
                cur = m.group(1)
                code[cur] = []
                continue
            if cur is None:
                continue
            if l.startswith(".L"):
                code[cur].append(l)
            elif l.startswith("\t") and not l.strip().startswith("."):
                code[cur].append(l.strip())
        entry = None
        for l in lines[i:]:
            if l.startswith("  - "):
                entry = []
                meta[len(meta)] = entry
            if entry is not None and l.startswith("  "):
                entry.append(l.rstrip())
            elif not l.startswith(" "):
                entry = None
        bykey = {}
        for e in meta.values():
            name = [x.split(":", 1)[1].strip() for x in e if x.strip().startswith(".name:") and x.startswith("    .name")]
            bykey[name[0] if name else "\n".join(e[:1])] = e
        return code, desc, bykey


    def remarks(path):
        out, fn = {}, None
        for l in open(path):
            m = re.search(r"remark: (.*)$", l)
            if not m:
                continue
            t = m.group(1).strip()
            m2 = re.match(r"Function Name: (\S+)", t)
            if m2:
                fn = m2.group(1)
                out[fn] = []
            elif fn:
                out[fn].append(t)
        return out


    def cmp(what, a, b, hide=lambda k: False):
        ka, kb = {k for k in a if not hide(k)}, {k for k in b if not hide(k)}
        print(f"{what}: parent {len(ka)}, head {len(kb)}, same names: {ka == kb}")
        for k in sorted(ka ^ kb):
            print("   only in", "parent" if k in ka else "head", k)
        bad = [k for k in sorted(ka & kb) if a[k] != b[k]]
        print(f"   entries that differ: {len(bad)}")
        for k in bad:
            d = [(x, y) for x, y in zip(a[k], b[k]) if x != y]
            print("   DIFF", k, len(a[k]), len(b[k]), d[:4])
        return sum(len(a[k]) for k in ka)


    ca, da, ma = parse(argv[0])
    cb, db, mb = parse(argv[1])
    cuid = lambda k: k.startswith("__hip_cuid_")
    print("compilation-unit identifiers:", [k for k in ca if cuid(k)], [k for k in cb if cuid(k)])
    n = cmp("symbols (instruction stream)", ca, cb, cuid)
    print("   instruction and label lines compared:", n)
    cmp("kernel descriptors (.amdhsa_kernel)", da, db)
    cmp("metadata entries (amdhsa.kernels)", ma, mb)
    ra, rb = remarks(argv[2]), remarks(argv[3])
    cmp("kernel-resource-usage remarks", ra, rb)
    order_a = [k for k in ca if k in da]
    order_b = [k for k in cb if k in db]
    print("kernels emitted in the same order:", order_a == order_b)
    for p in argv[0:2]:
        print("sha256", p.split("/")[-1], hashlib.sha256(open(p, "rb").read()).hexdigest())


def enqueue(argv):
    import json
    import os
    import sys
    import time

    root, label = os.path.abspath(argv[0]), argv[1]
    sys.path.insert(0, root)
    os.chdir(root)
    import numpy as np
    import torch

    import genpose_amd
    from genpose_amd.samplers import ODESampler
    from genpose_amd.scorenet import ScoreNetHIP
    from genpose_amd.weights_synth import make_state_dict

    assert os.path.abspath(genpose_amd.__file__).startswith(root), genpose_amd.__file__
    torch.cuda.set_device(0)
    B, K, T0, N = 5, 50, 0.55, int(argv[2]) if len(argv) > 2 else 400
    net = ScoreNetHIP(make_state_dict(0, "score"), "cuda")
    g = torch.Generator().manual_seed(3)
    feat = torch.randn(B, 1024, generator=g).abs().cuda()
    centre = (torch.randn(B, 3, generator=g) * 0.3).cuda()
    x0 = (torch.randn(B * K, 9, generator=g) * (0.01 * 5000.0 ** T0)).cuda()
    cvec = net.cloud_embed(feat)
    smp = ODESampler(net, B, K, "cuda", use_graph=False)
    out = smp.run(cvec, centre, x0, T0)[1]  # warm-up: every kernel of the plan loaded; the solve is finished, attempts exit at once
    torch.cuda.synchronize()
    for _ in range(max(50, N // 4)):
        smp._phase(3, None)
    torch.cuda.synchronize()
    ts = np.empty(N)
    for i in range(N):
        t = time.perf_counter_ns()
        smp._phase(3, None)
        ts[i] = time.perf_counter_ns() - t
        torch.cuda.synchronize()
    print(json.dumps({"label": label, "plan": hex(smp.plan), "kernel": smp.kernel_name, "calls": N, "median_us": round(float(np.median(ts)) / 1e3, 2),
                      "p10_us": round(float(np.percentile(ts, 10)) / 1e3, 2), "p90_us": round(float(np.percentile(ts, 90)) / 1e3, 2),
                      "attempts": int(smp.group_stats[0]["n_attempts"]), "out_sha": __import__("hashlib").sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]}), flush=True)


def paired(argv):
    import ctypes
    import importlib
    import importlib.util
    import json
    import os
    import sys
    import time

    import numpy as np
    import torch


    def load_pkg(name, tree):
        d = os.path.join(os.path.abspath(tree), "genpose_amd")
        spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return name


    torch.cuda.set_device(0)
    B, K, T0, N = 5, 50, 0.55, 3000
    g = torch.Generator().manual_seed(3)
    feat = torch.randn(B, 1024, generator=g).abs().cuda()
    centre = (torch.randn(B, 3, generator=g) * 0.3).cuda()
    x0 = (torch.randn(B * K, 9, generator=g) * (0.01 * 5000.0 ** T0)).cuda()
    S = {}
    for label, tree in (("parent", argv[0]), ("head", argv[1])):
        pkg = load_pkg("genpose_" + label, tree)
        samplers = importlib.import_module(pkg + ".samplers")
        scorenet = importlib.import_module(pkg + ".scorenet")
        synth = importlib.import_module(pkg + ".weights_synth")
        lib = importlib.import_module(pkg + "._lib")
        assert lib.SO_PATH.startswith(os.path.abspath(tree)), lib.SO_PATH
        net = scorenet.ScoreNetHIP(synth.make_state_dict(0, "score"), "cuda")
        smp = samplers.ODESampler(net, B, K, "cuda", use_graph=False)
        out = smp.run(net.cloud_embed(feat), centre, x0, T0)[1].clone()
        torch.cuda.synchronize()
        S[label] = (smp, lib, out)
    assert torch.equal(S["parent"][2], S["head"][2])
    labels = ("parent", "head")


    def series(fns, n):
        ts = {l: np.empty(n) for l in labels}
        for i in range(n):
            for l in (labels if i % 2 == 0 else labels[::-1]):  # who goes first alternates
                t = time.perf_counter_ns()
                fns[l]()
                ts[l][i] = time.perf_counter_ns() - t
                torch.cuda.synchronize()
        return {l: round(float(np.median(v)) / 1e3, 2) for l, v in ts.items()}


    phase = {l: (lambda s=S[l][0]: s._phase(3, None)) for l in labels}
    series(phase, 200)
    for block in range(5):
        print(json.dumps({"what": "_phase(3, None), median us over %d calls in turn" % N, **series(phase, N)}), flush=True)

    cd = ctypes.c_double


    def c_call(l):
        s, lib, _ = S[l]
        p = lib.ptr
        fn = lib.lib().gp_rk45_phase_model
        args = (s.model, s.plan, p(s.probe), 3, s.groups, s.B // s.groups, s.K, s.net.w.ref(), p(s.cvec), p(s.tvec), p(s.centre), p(s.state), p(s.y), p(s.ynew),
                p(s.Kbuf), p(s.partials), None, 0, cd(0.0), cd(0.0), cd(1e-5), cd(1e-5), cd(0.0), 1, 0, p(s.x_out), None, 0, lib.stream_ptr())
        return lambda: fn(*args)


    cc = {l: c_call(l) for l in labels}
    series(cc, 200)
    for block in range(5):
        print(json.dumps({"what": "gp_rk45_phase_model(phase 3) alone, median us over %d calls in turn" % N, **series(cc, N)}), flush=True)


if __name__ == "__main__":
    {"devcode": devcode, "enqueue": enqueue, "paired": paired}[sys.argv[1]](sys.argv[2:])
