"""The part of tests/test_kwave_variants_gpu.py that needs no device: the table of tests/_kwave_cases.py keeps the properties it was
built for, the restated XCD tile map is a bijection for every grid the table launches (and every small one), and for every row a
descriptor built from the geometry alone -- aligned dummy pointers, nothing launched or dereferenced -- is reported on tile 10
by cs_conv_gemm_launch_info; with CsDebug.no_kwave the automatic choice never is.  (The automatic choice itself is not asserted
here: it admits 4 x CUs tiles, which is none without a device.)"""
import pytest

import _kwave_cases as K
from test_gemm_variants_cpu import _desc, _info
from test_gemm_variants_gpu import CASES, FOREIGN_SEEDS, SLICED, _rows


def test_table_keeps_what_it_is_for():
    K.check_table(K.KW_CASES)
    assert len(K.KW_CASES) == len(set(K.KW_CASES)) == len(K.NAMES) == 17
    # the rows as the issue states them: chunks per wave and tiles
    assert K.per_wave(K.BY_NAME["A4"]) == [2, 2, 1, 0] and K.per_wave(K.BY_NAME["A7"]) == [4, 4, 4, 1]
    assert K.per_wave(K.BY_NAME["A10"]) == [7, 7, 7, 5] and K.per_wave(K.BY_NAME["P5"]) == [5, 5, 5, 2]
    assert K.tiles(K.BY_NAME["A6"]) == (5, 4) and K.tiles(K.BY_NAME["A11"]) == (8, 1) and _rows(K.BY_NAME["A1"]) == 1
    # the cases that lose one directional gate are the four with M <= 2 or cout = 4
    one = [n for n, c in K.BY_NAME.items() if not (K.row_gated(c) and K.col_gated(c))]
    assert one == ["A1", "A2", "A5", "P6"]


def test_a_thinned_table_fails_the_check():
    """the check is not vacuous: dropping the rows that carry a property fails it"""
    for drop in (["A7"], ["A8", "A9", "P5"], ["A11"], ["A5"], ["A4"], ["A1"], ["A8"], ["P1", "P2", "P3", "P4"]):
        with pytest.raises(AssertionError):
            K.check_table([c for n, c in K.BY_NAME.items() if n not in drop])


def test_foreign_seeds_do_not_touch_the_existing_tables():
    assert not any(c in FOREIGN_SEEDS for c in CASES + SLICED)
    seeds = [FOREIGN_SEEDS[c] for c in K.KW_CASES + K.R_CASES]
    assert len(set(seeds)) == len(seeds)
    own = {1000 + 16 * i for i in range(len(CASES))} | {1000 + 16 * (100 + i) for i in range(len(SLICED))}
    assert not own & set(seeds)


def test_bound_scale_rule_at_its_clamps():
    """the expectation test_operand_scale_from_a_bound holds the kernel to, at values worked out by hand: 65000 / 2 = 32500 in
    [2^14, 2^15); 65000 / 5000 = 13 in [8, 16); 65000 / 65000 = 1 exactly; 65000 / 1e-30 beyond 2^40; 65000 / 3e7 below 2^-8"""
    inf = float("inf")
    got = [K.bound_scale(v) for v in (2.0, 5000.0, 65000.0, 1e-30, 3.0e7, 0.0, -1.0, inf, float("nan"), 3.1e38)]
    assert got == [2.0 ** 14, 8.0, 1.0, 2.0 ** 40, 2.0 ** -8, 2.0 ** 40, 2.0 ** 40, 2.0 ** 40, 2.0 ** 40, 2.0 ** 40]


@pytest.mark.parametrize("n", sorted({K.nblk(c) for c in K.KW_CASES} | set(range(1, 34))))
def test_restated_tile_map_is_a_bijection(n):
    assert sorted(K.tile_map(n)) == list(range(n))


@pytest.mark.parametrize("c", K.KW_CASES, ids=K.case_id)
def test_launch_info_reports_the_kwave_tile(c):
    from commonscenes_amd import lib as L
    assert _info(_desc(c))[0] == 10
    assert _info(_desc(c, fmt=0))[0] == 10                    # the pair rows' fp32 twin
    with L.debug_override(no_kwave=1):
        assert _info(_desc(c, tile=0))[0] != 10


def test_launch_info_of_the_refusal_base_without_the_kernel():
    from commonscenes_amd import lib as L
    assert _info(_desc(K.R_BASE))[0] == 10
    with L.debug_override(no_kwave=1):
        assert _info(_desc(K.R_BASE, tile=0))[0] != 10
