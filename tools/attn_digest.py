#!/usr/bin/env python
"""One SHA-256 of the attention output bytes, and the status word, per case of tests/test_attention_variants_gpu.CASES x math
mode (fp32, F16X3, F16X3 with operand scales (8, 32, 4), F16) x route (natural, attn_nw8, no_attn_img): what a change that
claims "the same bits" has to reproduce line for line.

    python tools/attn_digest.py                      the listing of the library in use (CS_LIB_PATH, else the product)
    python tools/attn_digest.py --against ALT.so     both listings, each from a child process of its own; exit 1 if they differ
"""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def listing():
    import torch
    import test_attention_variants_gpu as T
    from commonscenes_amd import lib as L, ops
    maths = (("fp32", L.MATH_FP32, None), ("f16x3", L.MATH_F16X3, None), ("f16x3-scaled", L.MATH_F16X3, (8.0, 32.0, 4.0)),
             ("f16", L.MATH_F16, None))
    routes = (("natural", {}), ("attn_nw8", dict(attn_nw8=1)), ("no_attn_img", dict(no_attn_img=1)))
    for case in T.CASES:
        q, k, v = T._inputs(case)
        for mname, math, scales in maths:
            for rname, switches in routes:
                qd, kd, vd, out = T._operands(case, q, k, v)
                ops.read_status()
                o = T._run(case, qd, kd, vd, math, out=out, scales=scales, route="", **switches)
                torch.cuda.synchronize()
                sha = hashlib.sha256(o.contiguous().cpu().numpy().tobytes()).hexdigest()
                print(f"{T._id(case):24s} {mname:12s} {rname:11s} status {ops.read_status()} {sha}", flush=True)


def child(libpath):
    env = dict(os.environ)
    env.pop("CS_LIB_PATH", None)
    if libpath:
        env["CS_LIB_PATH"] = os.path.abspath(libpath)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"listing under {libpath or 'the product library'} failed ({r.returncode}):\n{r.stdout}{r.stderr}")
    return r.stdout


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", help="an alternative build of the library (tools/build_alt.sh) to compare the product with")
    a = ap.parse_args()
    if not a.against:
        listing()
        sys.exit(0)
    alt = child(a.against)      # one after the other: a failure in the first starts nothing more on the GPU
    own = child(None)
    print(f"# CS_LIB_PATH={a.against}\n{alt}# product library\n{own}", end="")
    same = alt == own and alt.count("\n") > 0
    print(f"# {alt.count(chr(10))} lines each: {'identical' if same else 'DIFFERENT'}")
    sys.exit(0 if same else 1)
