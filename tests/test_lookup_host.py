"""CPU: the host-only side of the lookup argument (include/stark_mi.h, "Lookup argument") -- smi_air_plan_lookup and its
refusals, mirror.Air.lookup, the declarations in the header, the loader and the Rust binding, and the restatement
(tests/lookup_compose.py) against plain definitions."""
import os
import re

import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import ext_compose as xc
import lookup_compose as lc
import perm_compose as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["smi_air_plan_lookup", "smi_dev_lookup_multiplicities", "smi_dev_lookup_column", "smi_dev_air_compose_lookup",
                "smi_dev_air_prove_lookup", "smi_air_verify_lookup"]


@pytest.fixture(scope="module")
def s():
    import stark_rs_amd
    stark_rs_amd.build()
    return stark_rs_amd


def plan(s, p, air, n_cols, log_n, lb, tau=1, h=3):
    from stark_rs_amd import _lib, engine
    a = air.flatten(p)
    return engine.air_plan_lookup(p, a, a.lookup, _lib.StarkCfg(log_n, lb, n_cols, 1, tau, h, 0, 1))


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_plan_counts_the_auxiliary_transition_of_degree_three(s, p, g):
    from stark_rs_amd.mirror import Air
    air = Air(3).lookup([0], [1], 2)                                     # no transition: d_air = 1
    assert plan(s, p, air, 3, 6, 3) == (3, 4)                            # d = 3, D = 2, E = 8 / 2
    assert plan(s, p, air, 3, 6, 4) == (3, 8)
    air, _cols = ac.make("fib", 64, p)                                   # linear transitions
    air.n_cols = 5
    air.lookup([2], [3], 4)
    assert plan(s, p, air, 5, 6, 3) == (3, 4)
    air, cols = ap.make("mimc", 64, p)                                   # the AIR's own degree decides above 3
    W = len(cols)
    air.n_cols = W + 1
    air.lookup([0], [0], W)
    d, D = max(air.degree, 3), 1
    while D < d - 1:
        D *= 2
    assert plan(s, p, air, W + 1, 6, 4) == (d, 16 // D)
    with pytest.raises(s.StarkMiError) as ei:                            # B / D < 4: log_blowup = 2 never serves
        plan(s, p, Air(3).lookup([0], [1], 2), 3, 6, 2)
    assert ei.value.status == -10 and "2^log_blowup / D < 4" in str(ei.value)


@pytest.mark.parametrize("cols,table,mult,text", [
    ([], [], 11, "width must be in 1 .. SMI_LOOKUP_MAX_WIDTH (8)"),
    (list(range(9)), list(range(9)), 11, "width must be in 1 .. SMI_LOOKUP_MAX_WIDTH (8)"),
    ([0, 12], [1, 2], 11, "lookup_col must be < n_cols"),
    ([0, 1], [1, 12], 11, "table_col must be < n_cols"),
    ([0, 1], [2, 3], 12, "mult_col must be < n_cols"),
    ([0, 1], [2, 3], 1, "mult_col must be none of the tuple columns"),
    ([0, 1], [2, 3], 2, "mult_col must be none of the tuple columns"),
])
def test_plan_refusals_name_the_limit(s, cols, table, mult, text):
    from stark_rs_amd.mirror import Air
    p = xc.PRIMES[0][0]
    air = Air(12).lookup(cols, table, mult)
    with pytest.raises(s.StarkMiError) as ei:
        plan(s, p, air, 12, 5, 3)
    assert ei.value.status == -50 and text in str(ei.value)


def test_plan_keeps_the_refusals_of_the_air(s):
    from stark_rs_amd.mirror import Air
    p = xc.PRIMES[0][0]
    air = Air(3).lookup([0], [1], 2)
    with pytest.raises(s.StarkMiError, match="log_n must be in 1 .. 27"):
        plan(s, p, air, 3, 0, 3)
    with pytest.raises(s.StarkMiError, match="1..64 columns"):
        plan(s, p, Air(65).lookup([0], [1], 2), 65, 5, 3)
    with pytest.raises(s.StarkMiError, match="offsets must be in 1 .. p-1"):
        plan(s, p, air, 3, 5, 3, tau=0)


def test_mirror_lookup(s):
    from stark_rs_amd.mirror import Air
    p, _g = xc.PRIMES[1]
    air = Air(5)
    assert air.lookup_arg is None and air.flatten(p).lookup is None
    air.lookup([0, 1], [2, 3], 4)
    flat = air.flatten(p)
    assert flat.perm is None and flat.lookup.width == 2 and flat.lookup.mult_col == 4
    assert [flat.lookup.lookup_col[j] for j in range(2)] == [0, 1] and [flat.lookup.table_col[j] for j in range(2)] == [2, 3]
    with pytest.raises(ValueError, match="one lookup per AIR"):
        air.lookup([0], [1], 2)
    with pytest.raises(ValueError, match="one width"):
        Air(3).lookup([0, 1], [2], 0)
    with pytest.raises(ValueError, match="a permutation or a lookup, not both"):
        air.permutation([0], [1])
    with pytest.raises(ValueError, match="a permutation or a lookup, not both"):
        Air(3).permutation([0], [1]).lookup([0], [1], 2)
    both = Air(3).permutation([0], [1])
    both.lookup_arg = ([0], [1], 2)                                      # set behind the methods' backs: flatten refuses
    with pytest.raises(ValueError, match="a permutation or a lookup, not both"):
        both.flatten(p)


def test_declarations(s):
    import ctypes as C
    from stark_rs_amd import _lib
    declared = s.declared_symbols()
    header = open(os.path.join(ROOT, "include", "stark_mi.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "stark_mi.rs")).read()
    lib = C.CDLL(_lib.LIB_PATH) if os.path.exists(_lib.LIB_PATH) else None
    for name in ENTRY_POINTS:
        assert name in declared
        assert re.search(r"pub fn " + name + r"\(", rust), name
        assert re.search(r"\b" + name + r"\(", rust[rust.index("// END GENERATED"):]), name
        if lib is not None:
            assert hasattr(lib, name), name
    assert "#define SMI_LOOKUP_MAX_WIDTH 8" in header and "pub const SMI_LOOKUP_MAX_WIDTH: u32 = 8;" in rust
    assert re.search(r"SMI_ERR_LOOKUP_MISSING = -56\b", header) and "pub const SMI_ERR_LOOKUP_MISSING: c_int = -56;" in rust
    assert re.search(r"pub struct smi_air_lookup \{\s*pub width: u32,\s*pub mult_col: u32,\s*pub lookup_col: \*const u32,\s*pub table_col: \*const u32,\s*\}", rust)
    assert C.sizeof(_lib.AirLookup) == 24
    assert header.index("---- Permutation argument") < header.index("---- Lookup argument") < header.index("---- multi-GPU")
    assert "LogUp / lookup arguments;" not in header and "One lookup per\n *   proof, and not together with a permutation" in header


def test_restated_multiplicities():
    cols = [[5, 7, 5, 9], [7, 5, 7, 5], [0] * 4]                        # table (column 1): 7 in rows 0 and 2, 5 in rows 1 and 3
    assert lc.multiplicities(cols, [0], [1]) == ([1, 2, 0, 0], 3)       # 9 is missing; the lowest rows are credited
    cols, lookup, table, mult_col = lc.shaped("dups", 64, xc.PRIMES[0][0], 3)
    M = cols[mult_col]
    assert sum(M) == 64
    seen = set()
    for t in range(64):                                                  # only the first row of a tuple may be credited
        key = tuple(cols[c][t] for c in table)
        assert key not in seen or M[t] == 0
        seen.add(key)
    cols, lookup, table, mult_col = lc.shaped("one", 32, xc.PRIMES[0][0], 3)
    assert cols[mult_col][32 // 3] == 32 and sum(cols[mult_col]) == 32


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_restated_column_is_the_definition_row_by_row(p, g):
    """s[r+1] = s[r] + 1 / f_L(r) - M[r] / f_T(r) with two separate inversions per row, against the restatement's one
    walked-back inversion and against the vectorised recurrence"""
    n = 32
    cols, lookup, table, mult_col = lc.shaped("dups", n, p, 3)
    ch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, (1 << 64) - 1, 8, dtype=np.uint64)]
    s_, closes, zero = lc.column(cols, lookup, table, mult_col, ch, p, g)
    assert zero is None and closes
    alpha, gamma = pm.alpha_gamma(ch, p)
    apow = pm.alpha_powers(alpha, 2, p, g)
    cur = [0, 0, 0, 0]
    for r in range(n):
        assert [int(v) for v in s_[:, r]] == cur
        row = [c[r] for c in cols]
        il = xc.inv(pm.tuple_value(row, lookup, apow, gamma, p), p, g)
        it = xc.inv(pm.tuple_value(row, table, apow, gamma, p), p, g)
        cur = xc.sub(xc.add(cur, il, p), xc.scale(it, cols[mult_col][r], p), p)
    assert cur == [0, 0, 0, 0]
    assert lc.recurrence_holds(s_, cols, lookup, table, mult_col, ch, p, g) == (True, True)
    bad = s_.copy()
    bad[1, 9] = (bad[1, 9] + np.uint64(1)) % np.uint64(p)
    assert lc.recurrence_holds(bad, cols, lookup, table, mult_col, ch, p, g)[0] is False
    for kind in ("multiplicity", "absent"):
        cols, lookup, table, mult_col = lc.non_closing(kind, n, p)
        s_, closes, zero = lc.column(cols, lookup, table, mult_col, ch, p, g)
        assert zero is None and not closes
        assert lc.recurrence_holds(s_, cols, lookup, table, mult_col, ch, p, g) == (True, False)


def test_the_verifiers_sentences_have_a_restated_class():
    """every sentence of the lookup verifier's opening checks (csrc/lookup_core.h) is one the restatement classifies, and
    every class has its sentence"""
    src = open(os.path.join(ROOT, "stark_rs_amd", "csrc", "lookup_core.h")).read()
    sentences = re.findall(r'"(lookup openings: [^"]*)"', src)
    assert len(sentences) == 6
    assert sorted(lc.reason_class(t) for t in sentences) == sorted(["length", "record", "record", "path", "canonical", "composition"])
