"""The proof that the gates of test_ops_variants_gpu.py (tests/_ops_cases.py) are neither vacuous nor tighter than fp32, on the
CPU: for every case of the table the fp32 emulation of the kernel's expression stays at or under 0.5 of its gate at every element
(bit-exact ops: equals the oracle; ddim / plms: under E itself -- their k is the exact count of roundings on a path of three to
eleven, and over the 10^6 elements of the wrap cases three roundings come close to 2^-24 of a term of S at once: the numpy fp32
evaluation measures 0.83 E, 0.67 E at n = 257, so half of E is no bound for IEEE arithmetic there.  E itself is one: every
operation rounds its result by at most 2^-24 of that result's magnitude, each intermediate result is in magnitude at most the sum
of the magnitudes of the terms it was built from, and every later operation scales an earlier error and that sum alike, so each
of the k roundings on a path adds at most 2^-24 S to the error of the output, to first order in 2^-24 -- k 2^-24 S in all, with
the roundings of parallel branches (dc * e beside sp * p0) already inside the S of the sum that joins them.  The GPU test
asserts the kernels equal this evaluation bit for bit), and every applicable mutant of it -- the last partial workgroup / lane chunk dropped, c in
place of ld, the elements beyond one sweep of the capped grid left untouched or (in place) visited twice, row % rows for
row / rows, the unconditional eps for both CFG terms, a border mask of tapsum27 missing, log_softmax without the max, the row
norm rounded to nearest, or bumped although it was exact, a rowstats call that overwrites the slot, a node's CSR entries out of edge order, the VQ tie to the last index, a NaN dropped by absmax -- leaves
the gate somewhere.  A mutant that a case's shape turns into a no-op is printed and counted, at most one per case.  Also here:
the recount of cs_ops.hip's extern "C" entries against the table, the oracles against oracle/ref_ops.py, and the k constants."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _ops_cases as N

SRC = Path(__file__).resolve().parent.parent / "commonscenes_amd" / "csrc" / "cs_ops.hip"


@pytest.mark.parametrize("c", N.CASES, ids=N.case_id)
def test_emulation_is_inside_half_the_gate_and_every_mutant_outside_it(c):
    for _, kind, ref, E in N.reference(c):
        if kind == "E":
            fin = torch.isfinite(ref)
            assert not torch.isnan(ref).any() and not torch.isnan(E).any() and bool((E[fin] >= 0).all())
    emu = N.worst_ratio(N.emulate(c), c)
    line = f"ops_variants_cpu {N.case_id(c)}: emulation {emu:.3f}"
    noop, worst = [], {}
    for m in N.mutants_of(c):
        v = N.emulate(c, m)
        if v is None:
            noop.append(m)
            continue
        worst[m] = N.worst_ratio(v, c)
        line += f"  {m} {worst[m]:.3g}"
    if c.op == "vq":
        idx, zq = N.emulate(c)
        flips = N.vq_report(c, idx, zq)[0]
        line += f"  (fp32 emulation: {flips} flips against fp64)"
        assert flips == 0, (N.case_id(c), flips)
    print(line + (f"  (no-op at this shape: {', '.join(noop)})" if noop else ""))
    # ddim / plms: k is the exact count of roundings on a path of three to eleven, each of which can come close to 2^-24 of a
    # term of S at once -- over 10^6 elements the fp32 evaluation reaches 0.83 E, so half of E is not a bound there; E is
    assert emu <= (1.0 if c.op in ("ddim", "plms") else 0.5), (N.case_id(c), emu)
    assert len(noop) <= 1, (N.case_id(c), noop)
    for m, v in worst.items():
        assert v > 1.0, (N.case_id(c), m, v)


def test_every_mutant_is_applied_in_three_cases():
    applied = {m: 0 for m in N.MUTANTS}
    for c in N.CASES:
        if max(c.get(k, 0) for k in ("m", "rows", "per", "n")) > 100000:     # the wrap cases are counted from their shape alone
            for m in N.mutants_of(c):
                applied[m] += 1
            continue
        for m in N.mutants_of(c):
            applied[m] += N.emulate(c, m) is not None
    print("ops_variants_cpu mutants applied:", applied)
    assert all(n >= 3 for n in applied.values()), applied


def test_table_names_every_extern_c_entry_of_cs_ops():
    """the extern "C" entries of cs_ops.hip, recounted from the source, are exactly the entries the table's cases name: an entry
    added to (or dropped from) the file must get (lose) its case"""
    src = SRC.read_text()
    found = re.findall(r'extern "C"\s+[A-Za-z_0-9]+\s+(cs_[a-z_0-9]+)\s*\(', src)
    named = {e for c in N.CASES for e in c.entries}
    assert len(found) == len(set(found)) == 24, sorted(found)
    assert named == set(found), (sorted(named - set(found)), sorted(set(found) - named))
    # the grid caps the sweep sizes of the table stand for
    assert len(re.findall(r"cs_grid_for\([^;]*256 \* 32\)", src)) == 7
    assert "cs_grid_for(m, 256, 1024)" in src and "cs_grid_for((n + 7) / 8, 256, 256)" in src
    assert "int cap = 256 * 16" in (SRC.parent / "cs_common.h").read_text()


def test_k_constants_keep_the_cpu_fp32_evaluation_under_half_the_gate():
    for op, k in (("geglu", N.K_GEGLU), ("ts_embedding", N.K_TSEMB), ("log_softmax", N.K_LSM)):
        r = N.measured_k(op)
        print(f"ops_variants_cpu {op}: torch CPU fp32 worst ratio {r:.2f} x 2^-24 S, k = {k}")
        assert 2.0 * r <= k, (op, r, k)          # <= 0.5 E; the constant was set as 4 r rounded up to a power of two
        assert k & (k - 1) == 0


def test_oracles_agree_with_the_project_oracle():
    from oracle import ref_ops as R
    for c in N.BY_OP["gcn"]:
        d = N.data(c)
        h = c["h"]
        nt = torch.nan_to_num(d["nt"], nan=0.0)
        ref = R.gcn_pool(nt, d["edges"], c["n_obj"], h, h + 1)
        assert torch.equal(ref, N.reference(c)[1][2]), N.case_id(c)
        pooled = np.zeros((c["n_obj"], h), np.float32)                         # two sequential scatter_adds, written out
        np.add.at(pooled, d["edges"][:, 0].numpy(), nt[:, :h].numpy())
        np.add.at(pooled, d["edges"][:, 1].numpy(), nt[:, h + 1:2 * h + 1].numpy())
        cnt = np.maximum(np.bincount(d["edges"].reshape(-1).numpy(), minlength=c["n_obj"]), 1).astype(np.float32)
        assert np.array_equal(pooled / cnt[:, None], ref.numpy()), N.case_id(c)
    for c in N.BY_OP["chamfer"]:
        d = N.data(c)
        dist, idx = R.chamfer_nm(d["a"], d["b"])
        ref = N.reference(c)
        assert np.array_equal(np.asarray(dist), ref[0][2].numpy()) and np.array_equal(np.asarray(idx), ref[1][2].numpy())
    for c in N.BY_OP["log_softmax"]:
        x = N.data(c)["x"].double()
        want, got = torch.log_softmax(x, dim=1), N.reference(c)[0][2]
        fin = torch.isfinite(want)
        assert torch.equal(fin, torch.isfinite(got)) and float((want[fin] - got[fin]).abs().max()) <= 1e-12
    for c in N.BY_OP["tapsum27"]:
        if not c["ints"]:
            continue
        # integers: the sum is exact in any order -- conv3d of Y's tap planes with one-hot kernels
        nb, (D, H, W), co = c["nb"], c["vol"], c["cout"]
        d = N.data(c)
        y = torch.nan_to_num(d["y"], nan=0.0).reshape(nb, D, H, W, co, 27).double()
        out = torch.zeros(nb, D, H, W, co, dtype=torch.float64)
        yp = torch.nn.functional.pad(y, (0, 0, 0, 0, 1, 1, 1, 1, 1, 1))
        for t in range(27):
            kd, kh, kw = t // 9, (t // 3) % 3, t % 3
            out += yp[:, kd:kd + D, kh:kh + H, kw:kw + W, :, t]
        if d["bias"] is not None:
            out += d["bias"].double()
        assert torch.equal(out.reshape(-1, co).float(), N.reference(c)[0][2]), N.case_id(c)


def test_table_reaches_the_edges_it_claims():
    by = N.BY_OP
    assert {(c["m"], c["h"]) for c in by["geglu"]} == {(1, 4), (3, 12), (77, 448), (N.SWEEP32 + 5, 4)}
    assert any(c["ldx"] > 2 * c["h"] and c["ldo"] > c["h"] for c in by["geglu"])
    assert any(c["m"] % c["rows"] and (256 // (c["c"] // 4)) % c["rows"] for c in by["add_rowvec"])
    assert any(c["share"] == 2 for c in by["concat"])
    for op, key in (("to_ndhwc", "cpad"), ("to_nchw", "c")):
        assert max(c["nb"] * N._s_of(c) * c[key] for c in by[op]) == N.SWEEP32 + 3
    assert {c["dim"] for c in by["ts_embedding"]} == {2, 3, 33, 224} and all((3 * c["dim"]) % 256 for c in by["ts_embedding"])
    ns = {c["nb"] * c["per"] for c in by["ddim"]}
    assert {1, 255, 257, N.SWEEP16 + 77} <= ns and any(c["nb"] == 7 and c["per"] % 2 and c["nb"] * c["per"] > N.SWEEP16 for c in by["ddim"])
    assert {c["mode"] for c in by["plms"]} == set(range(5)) and {c["cfg"] for c in by["plms"]} == {0, 1}
    assert {c["ncode"] for c in by["vq"]} == {1, 7, 4097, 8192} and 4097 * 16 > 64 * 1024 >= 4096 * 16
    assert {(c["edim"], c["ldz"]) for c in by["vq"]} == {(1, 1), (1, 4), (2, 2), (2, 4), (3, 3), (3, 4)}
    assert max(c["m"] for c in by["vq"]) == N.SWEEP_VQ + 3
    assert {c["n_tri"] for c in by["gcn"]} == {1, 63, 64, 65, 128, 129} and {c["h"] for c in by["gcn"]} == {1, 33}
    for c in by["gcn"]:
        e = N.data(c)["edges"]
        if c["kind"] != "self":
            assert c["n_obj"] - 1 not in e
        if c["kind"] == "hub":
            assert bool(((e[:, 0] == 0) | (e[:, 1] == 0)).all())
    assert max(c["n"] * c["dim"] for c in by["embedding"]) > N.SWEEP16
    assert {c["c"] for c in by["log_softmax"]} == {1, 24, 63, 64, 65, 130} and {c["m"] for c in by["log_softmax"]} == {1, 4, 5}
    assert {r for c in by["rowstats"] for r, _ in c["mats"]} >= {1, 3, 4, 5}
    assert {cl for c in by["rowstats"] for _, cl in c["mats"]} >= {1, 63, 64, 65, 200}
    assert {len(c["mats"]) for c in by["rowstats"]} == {1, 2, 3}
    assert {c["vol"] for c in by["tapsum27"]} == {(1, 1, 1), (1, 1, 5), (3, 1, 1), (2, 3, 4)}
    for k, vals in (("nb", {1, 2}), ("cout", {1, 4}), ("ypad", {0, 5}), ("bias", {0, 1}), ("ints", {0, 1})):
        assert {c[k] for c in by["tapsum27"]} == vals, k
    assert {(c["cout"], c["ncolp"]) for c in by["pack_tapcol"]} == {(1, 28), (1, 84), (3, 84)}
    assert {c["cin"] for c in by["pack_tapcol"]} == {3, 16, 20} and {c["scale"] for c in by["pack_tapcol"]} == {1.0, 0.125}
