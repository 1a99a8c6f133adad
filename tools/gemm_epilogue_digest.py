#!/usr/bin/env python
"""One SHA-256 of the output view's bytes, and the status word, per case of tests/test_line_store_epilogue_gpu.CASES and of
tests/test_pw_reg_epilogue_gpu.CASES (every TR tile x every epilogue form of the one-tap GEMMs), and one SHA-256 of the
workspace view per position case x slice count of test_line_store_epilogue_gpu.py (the Winograd-W position GEMMs have no
untransposed twin in the product build): what a change to the register-direct epilogue of cs_gemm_f16x3.hip that claims
"the same bits" has to reproduce line for line.

    python tools/gemm_epilogue_digest.py                      the listing of the library in use (CS_LIB_PATH, else the product)
    python tools/gemm_epilogue_digest.py --against ALT.so     both listings, each from a child process of its own; exit 1 if they differ
"""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def listing():
    import torch
    import test_line_store_epilogue_gpu as T
    import test_pw_reg_epilogue_gpu as P
    import _wino_cases as W
    from commonscenes_amd import ops
    for c in T.CASES:
        dev = T._device(c)
        ops.read_status()
        out = T._launch(c, dev)
        torch.cuda.synchronize()
        print(f"line {T._id(c):40s} status {ops.read_status()} {_sha(out)}", flush=True)
    for c in P.CASES:
        dev = P._device(c)
        ops.read_status()
        out, part = P._launch(c, dev)
        torch.cuda.synchronize()
        tail = "" if part is None else f" partials {_sha(part)}"
        print(f"pw   {P._id(c):40s} status {ops.read_status()} {_sha(out)}{tail}", flush=True)
    for c in T.POS:
        for slices in T.SLICES:
            p, keep, mt = T._pos_setup(c)
            ws = T._run_positions(p, slices, mt, c.cout, keep[-1])      # (asserts status 0 and the sentinel bands)
            print(f"pos  {W.conv_id(c) + f' k{slices}':40s} status {ops.read_status()} {_sha(ws)}", flush=True)


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
