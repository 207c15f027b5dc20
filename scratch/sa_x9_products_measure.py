"""Stand-alone timing and accuracy of the three bf16x9 encoder kernels (levels 1, 2, 3) of ONE build of the library, from the fp32
encoder's intermediates - for the eight-against-nine-products comparison (profiles/sa_x9_products.txt): run it once per build,

    python scratch/sa_x9_products_measure.py --tag eight
    GENPOSE_HIP_LIB=genpose_amd/lib/libgenpose_hip_p9.so python scratch/sa_x9_products_measure.py --tag nine
        (GP_BUILD_TAG=p9 GP_EXTRA_FLAGS=-DGP_SA_X9_PRODUCTS=9 python -m genpose_amd.build)

alternating the two.  Timing: HIP events around each launch, 2 warm-ups + 11 repeats, us, median [min, max]; the fp32 kernels of the same
level ride along as a control that must not move between the builds.  --accuracy: max error over the feature scale against float64
(computed on the device) for the split kernel and for the fp32 kernels, on the tests' five clouds (synth.make_batch(5, start=4321), the
last one tiled duplicates) and on a 640-cloud pass (64 distinct clouds x 10: the reference covers the 64, the split kernels' copies must
repeat their bits)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fp64_level(xyz, centres, z, idxs, folded, width, paren):
    """Levels 1 / 2 in float64 on the device: relu(z_j + Wxyz d + b1) -> relu(W2 . + b2) -> relu(max_j (W3 .) + b3), cloud chunks of 8.
    paren: layer 1 as z + (dot + b1) (level 1's test reference) or (z + dot) + b1 (level 2's)."""
    outs = []
    for c0 in range(0, xyz.shape[0], 8):
        s = slice(c0, c0 + 8)
        X, C, Z = xyz[s].double(), centres[s].double(), z[s].double()
        bi = torch.arange(X.shape[0], device=X.device)[:, None, None]
        cols = []
        for i, ((W1, b1), (W2, b2), (W3, b3)) in enumerate(folded):
            W1, b1, W2, b2, W3, b3 = (t.double().to(X.device) for t in (W1, b1, W2, b2, W3, b3))
            idx = idxs[i][s].long()
            d = X[bi, idx] - C[:, :, None, :]
            zz = Z[bi, idx][..., width * i:width * i + width]
            h1 = torch.relu(zz + (d @ W1[:, -3:].t() + b1) if paren else zz + d @ W1[:, -3:].t() + b1)
            h2 = torch.relu(h1 @ W2.t() + b2)
            cols.append(torch.relu((h2 @ W3.t()).max(dim=2)[0] + b3))
        outs.append(torch.cat(cols, dim=-1))
    return torch.cat(outs)


def fp64_groupall(xyz, feat, folded):
    x = torch.cat([feat.double(), xyz.double()], dim=-1)
    outs = []
    for (W1, b1), (W2, b2), (W3, b3) in folded:
        W1, b1, W2, b2, W3, b3 = (t.double().to(x.device) for t in (W1, b1, W2, b2, W3, b3))
        h2 = torch.relu(torch.relu(x @ W1.t() + b1) @ W2.t() + b2)
        outs.append(torch.relu(h2 @ W3.t() + b3).max(dim=1)[0])
    return torch.cat(outs, dim=-1)


class Levels:
    """The three levels' launches on the intermediates of one fp32 encoder pass over `pts`."""

    def __init__(self, e32, e9, pts):
        from genpose_amd._lib import ptr
        self.e32, self.e9, self.B = e32, e9, pts.shape[0]
        _, ws = e32.forward(pts, return_intermediates=True)
        self.ws = {k: ([t.clone() if torch.is_tensor(t) else ([u.clone() for u in t] if t is not None else None) for t in v] if isinstance(v, list) else v)
                   for k, v in ws.items() if k in ("new_xyz", "z", "bq", "feat")}
        self.out = {k: torch.empty_like(self.ws["feat"][k]) for k in (1, 2, 3)}

    def launch(self, level, kind, i=None):
        """kind 'x9' | 'f32'; i: the scale (levels 1, 2), None = both (level 3: one launch under 'x9')."""
        from genpose_amd import _lib
        from genpose_amd._lib import ptr, stream_ptr
        ws, B, out = self.ws, self.B, self.out[level]
        if level == 3:
            xyz, feat = ws["new_xyz"][2], ws["feat"][2]
            if kind == "x9":
                wx9, offs = self.e32.w.groupall_bf16x9_packs()
                sargs = []
                for j, sc in enumerate(self.e32.w.levels[3]):
                    (_, b1), (_, b2), (_, b3) = sc.layers
                    sargs += [sc.couts[1], ptr(wx9[offs[j]:]), ptr(sc.wxyz), ptr(b1), ptr(b2), ptr(b3), 512 * j]
                _lib.call("gp_sa_groupall_bf16x9", B, 128, 512, 256, 512, ptr(xyz), ptr(feat), *sargs, ptr(out), 1024, stream_ptr())
            else:
                out.zero_()
                z = ws["z"][3]
                _lib.call("gp_point_linear", B * 128, 512, 512, ptr(feat), ptr(self.e32.w.z_weights[3]), ptr(z), stream_ptr())
                for j, sc in enumerate(self.e32.w.levels[3]):
                    (_, b1), (w2, b2), (w3, b3) = sc.layers
                    _lib.call("gp_sa_pre_mlp_max_layout", sc.hidden_layout, B, 128, 1, 128, 256, sc.couts[1], 512, ptr(xyz), None, None, ptr(z), 512, 256 * j,
                              ptr(sc.wxyz), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(out), 1024, 512 * j, stream_ptr())
            return
        n, npnt, c1, c3 = (512, 256, 64, 128) if level == 1 else (256, 128, 128, 256)
        for j in ((0, 1) if i is None else (i,)):
            sc = (self.e9 if kind == "x9" else self.e32).w.levels[level][j]
            ns = self.e32.cfg["nsamples"][level][j]
            head = (B, n, npnt, ns, *sc.couts, ptr(ws["new_xyz"][level - 1]), ptr(ws["new_xyz"][level]), ptr(ws["bq"][level][j]), ptr(ws["z"][level]), 2 * c1,
                    c1 * j, ptr(sc.wxyz), ptr(sc.layers[0][1]))
            if kind == "f32":
                (_, _), (w2, b2), (w3, b3) = sc.layers
                _lib.call("gp_sa_pre_mlp_max_layout", sc.hidden_layout, *head, ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(out), 2 * c3, c3 * j, stream_ptr())
            elif level == 1:
                _lib.call("gp_sa_lds_bf16x9", *head, *map(ptr, sc.bf16x9_lds_packs()), ptr(out), 2 * c3, c3 * j, stream_ptr())
            else:
                _lib.call("gp_sa_pre_mlp_max_bf16x9", *head, *map(ptr, sc.bf16x9_packs()), ptr(out), 2 * c3, c3 * j, stream_ptr())

    def result(self, level, kind):
        self.out[level].fill_(float("nan"))
        self.launch(level, kind)
        torch.cuda.synchronize()
        return self.out[level].reshape(self.ws["feat"][level].shape).clone()

    def reference(self, level, nb):
        ws, e = self.ws, self.e32
        if level == 3:
            return fp64_groupall(ws["new_xyz"][2][:nb], ws["feat"][2][:nb], [sc._folded_plain for sc in e.w.levels[3]]).reshape(nb, 1, 1024)
        return fp64_level(ws["new_xyz"][level - 1][:nb], ws["new_xyz"][level][:nb], ws["z"][level][:nb], [t[:nb] for t in ws["bq"][level]],
                          [sc._folded_plain for sc in e.w.levels[level]], 64 if level == 1 else 128, level == 1)


def timed(fn, repeats):
    ts = []
    for rep in range(2 + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if rep >= 2:
            ts.append(e0.elapsed_time(e1) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", required=True)
    ap.add_argument("--clouds", type=int, nargs="*", default=[640, 320, 128, 64])
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from genpose_amd import _lib, synth
    from genpose_amd.encoder import Pointnet2EncoderHIP
    from oracle import genpose_oracle as go
    sd = go.make_state_dict(0, "score")
    e32 = Pointnet2EncoderHIP(sd, "cuda")
    e9 = Pointnet2EncoderHIP(sd, "cuda", precision="bf16x9")
    rec = {"tag": a.tag, "lib": _lib.SO_PATH, "timing_us": {}, "accuracy": {}}
    print(f"# build {a.tag}: {_lib.SO_PATH}", flush=True)
    base = torch.from_numpy(synth.make_batch(64, start=100)).cuda().float()
    for B in a.clouds:
        lv = Levels(e32, e9, base[torch.arange(B, device="cuda") % 64].contiguous())
        arms = [(f"level{k}.{kind}" + ("" if i is None else f".scale{i}"), (lambda k=k, kind=kind, i=i: lv.launch(k, kind, i)))
                for kind in ("x9", "f32") for k, scales in ((1, (0, 1)), (2, (0, 1)), (3, (None,))) for i in scales]
        for name, fn in arms:
            ts = timed(fn, a.repeats)
            rec["timing_us"][f"{B}.{name}"] = ts
            print(f"{a.tag:6s} clouds {B:4d}  {name:18s} {statistics.median(ts):8.1f} [{min(ts):8.1f}, {max(ts):8.1f}]", flush=True)
    if a.accuracy:
        five = torch.from_numpy(synth.make_batch(5, start=4321)).cuda().float()
        five[4] = five[4, :64].repeat(five.shape[1] // 64, 1)
        for what, pts, nref in (("tests' 5 clouds", five, 5), ("640 clouds (64 distinct x 10)", base[torch.arange(640, device="cuda") % 64].contiguous(), 64)):
            lv = Levels(e32, e9, pts)
            for k in (1, 2, 3):
                ref = lv.reference(k, nref)
                scale = float(ref.abs().max())
                row = {}
                for kind in ("x9", "f32"):
                    o = lv.result(k, kind)
                    assert bool(torch.isfinite(o).all())
                    if kind == "f32":
                        assert torch.equal(o, lv.ws["feat"][k])  # the direct calls are what the fp32 encoder ran
                    copies = [o[c:c + nref] for c in range(0, pts.shape[0], nref)]
                    if kind == "x9":  # the copies repeat the bits (the fp32 GroupAll path's hoisted GEMM tiles by row position: not asked of it)
                        assert all(torch.equal(t, copies[0]) for t in copies), k
                    row[kind] = max(float((t.double().reshape(ref.shape) - ref).abs().max()) for t in copies) / scale
                rec["accuracy"][f"{what}.level{k}"] = row
                print(f"{a.tag:6s} {what}: level {k}: max error / feature scale vs float64: bf16x9 kernel {row['x9']:.4e}, fp32 kernels {row['f32']:.4e}", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rec, f)


if __name__ == "__main__":
    main()
