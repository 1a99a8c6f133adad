"""The proof that the gate of test_norm_variants_gpu.py (err <= E elementwise, tests/_norm_cases.py) is neither vacuous nor
tighter than fp32 itself, on the CPU: for every case of the table the fp32 emulation of the kernel's expression stays at or
under 0.5 E at every element, and every applicable mutant of it -- a row left out of the statistics, the neighbour group's
statistics at the first channel of group 1, a channel left out of the LayerNorm mean, the partials' channel index off by one,
the wrapped voxel in place of the zero pad after a Winograd line -- exceeds E at some element.  A mutant that a case's shape
turns into a no-op is reported (printed and counted), at most one per case.  Also here: the written-out fp64 GroupNorm against
oracle/ref_ops.py::groupnorm_ndhwc on fp64, and the recount of cs_norm.hip's launch sites against the table."""
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import _norm_cases as N

SRC = Path(__file__).resolve().parent.parent / "commonscenes_amd" / "csrc" / "cs_norm.hip"


@pytest.mark.parametrize("c", N.CASES, ids=N.case_id)
def test_emulation_is_inside_half_the_bound_and_every_mutant_outside_it(c):
    r = N.reference(c)
    assert torch.isfinite(r["ref"]).all() and torch.isfinite(r["E"]).all() and float(r["E"].min()) > 0.0
    emu = N.worst_ratio(N.emulate(c), c)
    line = f"norm_variants_cpu {N.case_id(c)}: emulation {emu:.3f} E"
    noop, worst = [], {}
    for m in N.mutants_of(c):
        v = N.emulate(c, m)
        if v is None:
            noop.append(m)
            continue
        worst[m] = N.worst_ratio(v, c)
        line += f"  {m} {worst[m]:.3g} E"
    print(line + (f"  (no-op at this shape: {', '.join(noop)})" if noop else ""))
    assert emu <= 0.5, (N.case_id(c), emu)
    assert len(noop) <= 1, (N.case_id(c), noop)
    for m, v in worst.items():
        assert v > 1.0, (N.case_id(c), m, v)


def test_every_mutant_is_applied_somewhere_and_noops_are_the_expected_ones():
    applied = {m: 0 for m in N.MUTANTS}
    for c in N.CASES:
        nb, rows, ch = N.dims(c)
        for m in N.mutants_of(c):
            if c.kind in ("ln32", "pair16"):
                noop = False
            else:
                noop = {"drop_row": rows == 1, "neighbour": c.groups == 1, "chan_off1": ch == c.groups, "wrap_pad": False}[m]
            applied[m] += not noop
    assert all(n >= 5 for n in applied.values()), applied


def test_written_out_groupnorm_equals_the_oracle_on_fp64():
    from oracle import ref_ops as R
    for c in (N.BY_GROUP["small"][0], N.BY_GROUP["apply"][1], N.BY_GROUP["apply"][3]):
        t = N.data(c)
        nb, rows, ch = c.shape
        ref = N.reference(c)["ref"]
        act = {N.ACT_NONE: None, N.ACT_SILU: "silu", N.ACT_GELU: "gelu"}[c.act]
        o = R.groupnorm_ndhwc(t["x"].double().reshape(nb, rows, 1, 1, ch), t["g"].double(), t["b"].double(), c.groups, N.EPS, act)
        assert float((o.reshape(nb * rows, ch) - ref).abs().max()) <= 1e-12
    c = N.BY_GROUP["layernorm"][10]
    t = N.data(c)
    o = F.layer_norm(t["x"][0].double(), (c.shape[1],), t["g"].double(), t["b"].double(), N.EPS)
    assert float((o - N.reference(c)["ref"]).abs().max()) <= 1e-12


def test_winograd_reference_is_the_transform_of_the_kernel_comments():
    """B^T d against a plain loop over lines, tiles and taps, for both variants"""
    for grp in ("wino23", "wino43"):
        c = N.BY_GROUP[grp][1]
        nb, d, h, w, ch = c.shape
        var = c.o["variant"]
        y = torch.randn(nb, d * h * w, ch, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
        img = N.wino_images(c, y)
        yl = y.reshape(nb * d * h, w, ch)
        for q, row in enumerate(N.BT[var]):
            for line in (0, nb * d * h - 1):
                for t in range(w // var):
                    want = sum(cf * yl[line, var * t - 1 + j] for j, cf in enumerate(row) if cf and 0 <= var * t - 1 + j < w)
                    assert float((img[q, line * (w // var) + t] - want).abs().max()) <= 1e-12


def test_pair_split_terms():
    """|lo| <= half an fp16 ulp of hi and (hi + lo) within 2^-22 |o| + 2^-25 of o, on values across the fp16 range"""
    o = torch.randn(20000, generator=torch.Generator().manual_seed(3)) * torch.logspace(-9, 4, 20000)
    hi, lo, v = N.pair_value(o, 1.0)
    assert bool(((v - o.double()).abs() <= 2.0 ** -22 * o.double().abs() + 2.0 ** -25).all())
    h = hi.double().abs()
    ulp = torch.ldexp(torch.ones_like(h), torch.frexp(h.clamp_min(2.0 ** -14))[1] - 11)
    assert bool((lo.double().abs() <= 0.5 * ulp).all())


def test_table_names_every_launch_site_of_cs_norm():
    """the CS_LAUNCH( sites of cs_norm.hip (10, and 2 CS_LN_LAUNCH( sites of three instantiations each), recounted from the
    source, are exactly the kernels the table's cases name: a kernel or instantiation added to (or dropped from) the file must
    get (lose) its case"""
    src = SRC.read_text()
    wv = re.search(r"#else\s*\n\s*constexpr int WV = (\d+);", src).group(1)
    sites = re.findall(r"CS_LAUNCH\(\s*\(?([A-Za-z_0-9]+(?:<[^>]*>)?)", src)
    # a CS_LN_LAUNCH site launches the MAXV instantiations that cs_ln_pair.h's macro spells out
    maxv = re.findall(r"CS_LAUNCH\(kernel<(\d+)>", (SRC.parent / "cs_ln_pair.h").read_text())
    ln_sites = re.findall(r"CS_LN_LAUNCH\(\s*([A-Za-z_0-9]+)", src)
    sites += [f"{k}<{v}>" for k in ln_sites for v in maxv]
    found = {s.replace("WV>", f"{wv}>").replace(" ", "") for s in sites}
    named = {k for c in N.CASES for k in c.kernels}
    assert maxv == ["2", "4", "8"] and len(ln_sites) == 2
    assert len(sites) == len(found) == 16, sorted(found)
    assert named == found, (sorted(named - found), sorted(found - named))
    kernels = set(re.findall(r"__global__\s+__launch_bounds__\([^)]*\)\s+void\s+(\w+)", src))
    assert len(kernels) == 10 and kernels == {k.split("<")[0] for k in found}, sorted(kernels)


def test_table_reaches_the_branches_it_claims():
    """the host geometry each case is in the table for, recomputed here from the rules of cs_norm.hip"""
    by = N.BY_GROUP
    for c in by["parts"]:
        nb, rows, ch = c.shape
        assert rows * (ch // c.groups) <= 11264 and N.rsplit_rule(nb, rows, ch, c.groups) == c.o["rsplit"], N.case_id(c)
    assert {c.o["rsplit"] for c in by["parts"]} == {1, 2, 4}
    nsplit = lambda nb, rows: min(256, max(1, min((2048 + nb - 1) // nb, (rows + 15) // 16)))
    assert [nsplit(c.shape[0], c.shape[1]) for c in by["stats"]] == [3, 3, 1, 66, 256]
    for grp in ("stats", "finalize_parts", "parts", "small", "apply", "split16", "wino23", "wino43", "layernorm", "pair16"):
        views = [c.view for c in by[grp]]
        assert views == [i % 2 == 1 for i in range(len(views))]
    for c in by["finalize_parts"] + by["parts"] + by["parts_split"]:
        cpg = c.shape[2] // c.groups
        pairs = max(ncls * tps * min(nch, cpg) for nch, tps, ncls, _, _, _ in c.o["segs"])
        assert (pairs >= 512) == ("gn_finalize_parts_kernel<4>" in c.kernels), N.case_id(c)
        assert sum(s[0] for s in c.o["segs"]) == c.shape[2]
    assert max(N.dims(c)[0] * N.dims(c)[1] * N.dims(c)[2] * 4 for c in N.CASES) <= 3 << 20
