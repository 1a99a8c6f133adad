#!/usr/bin/env python
"""profiles/gemm_variants_kernel_trace.txt from the rocpd database of ONE kernel-trace run of tests/test_gemm_variants_gpu.py:

    rocprofv3 --kernel-trace -d prof -o gemm_variants -- python -m pytest -m gpu tests/test_gemm_variants_gpu.py
    python tools/gemm_variants_trace.py prof/gemm_variants_results.db > profiles/gemm_variants_kernel_trace.txt

How dispatches are mapped to cases: the tests run in file order and every conv_gemm_f16x3_kernel dispatch of the run comes from
them in a known order -- per case of test_variant_matrix its own launch, the second run, then one launch per identity twin
(_twins); per case of test_k_slices_at_ragged_chunk_counts the sliced launch, the unsliced one, the sliced one again.  The
dispatches are sorted by start time and dealt out by those counts; the total must match, and a case whose own launch is not
the instantiation its table row names (_key) is marked."""
import re
import sqlite3
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import test_gemm_variants_gpu as T  # noqa: E402


def _args(name):
    """template arguments of a (demangled or mangled) conv_gemm_f16x3_kernel name as <a,b,...>"""
    m = re.search(r"conv_gemm_f16x3_kernel<([^>]*)>", name)
    if m:
        return "<" + ",".join(a.strip() for a in m.group(1).split(",")) + ">"
    m = re.search(r"conv_gemm_f16x3_kernelI((?:L[ib]\d+E)+)E", name)
    return "<" + ",".join(v if k == "i" else ("true" if v == "1" else "false")
                          for k, v in re.findall(r"L([ib])(\d+)E", m.group(1))) + ">"


def _fmt(key):
    return "<" + ",".join(str(v).lower() if isinstance(v, bool) else str(v) for v in key) + ">"


def main(path):
    cur = sqlite3.connect(path).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    rows = sorted((s, n) for n, s in cur.execute(f"select {name_col}, start from kernels"))
    names = [_args(n) for _, n in rows if "conv_gemm_f16x3_kernel" in n]
    reduces = sum("splitk_reduce_kernel" in n for _, n in rows)
    want = sum(2 + len(T._twins(c)) for c in T.CASES) + 3 * len(T.SLICED)
    print("# rocprofv3 --kernel-trace -- python -m pytest -m gpu tests/test_gemm_variants_gpu.py, dealt out to the cases by "
          "tools/gemm_variants_trace.py")
    print(f"# conv_gemm_f16x3_kernel<WMB,WNB,WAVES_M,WAVES_N,PRE,SLAB,PAIR,TPK,PW> dispatches: {len(names)} (the tests issue {want}); "
          f"splitk_reduce_kernel dispatches: {reduces} (the sliced cases issue {2 * len(T.SLICED)})")
    if len(names) != want:
        sys.exit(f"dispatch count {len(names)} != {want}: the trace is not one run of the whole file")
    i, bad, reached = 0, 0, set()
    for c in T.CASES:
        tw = T._twins(c)
        blk = names[i:i + 2 + len(tw)]
        i += len(blk)
        ok = blk[0] == _fmt(T._key(c)) and blk[1] == blk[0]
        bad += not ok
        reached.add(blk[0])
        print(f"{T._id(c):58s} {blk[0]}{'' if ok else '   NOT the instantiation the table names: ' + _fmt(T._key(c))}")
        for (claim, _, _), k in zip(tw, blk[2:]):
            print(f"{'':8s}{claim:50s} {k}")
    print(f"# instantiations reached by a case's own launch: {len(reached)}; mismatches: {bad}")
    print("# K-sliced cases: the sliced launch (+ splitk_reduce_kernel), the unsliced one, the sliced one again")
    for c, s in zip(T.SLICED, T.SLICES):
        blk = names[i:i + 3]
        i += 3
        print(f"{T._id(c) + f' x{s}':58s} {blk[0]}{'' if blk[2] == blk[0] else '   rerun: ' + blk[2]}")
        print(f"{'':8s}{'unsliced':50s} {blk[1]}")


if __name__ == "__main__":
    main(sys.argv[1])
