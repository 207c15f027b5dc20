"""What the CPU tests of the split-bf16 set-abstraction kernels' host side share: the declared prototype of an entry point, the three bf16
terms of a weight matrix and pack_bf16x9's k order.  A plain helper module (imported by the tests, not collected by pytest)."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prototype(name):
    """The argument declarations of `int name(...)` in include/genpose_hip.h, whitespace normalised."""
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/genpose_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def terms(W):
    hi = W.to(torch.bfloat16)
    r = W - hi.float()
    mid = r.to(torch.bfloat16)
    lo = (r - mid.float()).to(torch.bfloat16)
    return hi, mid, lo


def k_of(kb, g, e):
    """Input channel of element e of lane group g in k-block kb: two consecutive D fragments of the previous layer (pack_bf16x9, chain order)."""
    return 32 * kb + (4 * g + e if e < 4 else 16 + 4 * g + e - 4)
