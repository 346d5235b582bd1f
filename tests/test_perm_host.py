"""CPU: the host-only side of the permutation argument (include/stark_mi.h, "Permutation argument") -- smi_air_plan_perm and
its refusals, mirror.Air.permutation, the declarations in the header, the loader and the Rust binding, and the restatement
(tests/perm_compose.py) against plain definitions."""
import os
import re

import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import ext_compose as xc
import perm_compose as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["smi_air_plan_perm", "smi_dev_perm_column", "smi_dev_air_compose_perm", "smi_dev_air_prove_perm", "smi_air_verify_perm"]


@pytest.fixture(scope="module")
def s():
    import stark_rs_amd
    stark_rs_amd.build()
    return stark_rs_amd


def plan(s, p, air, n_cols, log_n, lb, tau=1, h=3):
    from stark_rs_amd import _lib, engine
    a = air.flatten(p)
    return engine.air_plan_perm(p, a, a.perm, _lib.StarkCfg(log_n, lb, n_cols, 1, tau, h, 0, 1))


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_plan_counts_the_auxiliary_constraints_of_degree_two(s, p, g):
    from stark_rs_amd.mirror import Air
    air = Air(3).permutation([0], [1])                                   # no transition: d_air = 1
    assert plan(s, p, air, 3, 6, 3) == (2, 8)
    air, _cols = ac.make("fib", 64, p)                                   # linear transitions
    air.permutation([0], [1])
    assert plan(s, p, air, 2, 6, 3) == (2, 8)
    air, cols = ap.make("mimc", 64, p)                                   # degree 3: D = 2
    air.permutation([0], [0])
    d, E = plan(s, p, air, len(cols), 6, 3)
    assert (d, E) == (max(air.degree, 2), 8 // 2 if air.degree == 3 else E)
    with pytest.raises(s.StarkMiError) as ei:                            # B / D < 4
        plan(s, p, air, len(cols), 6, 2)
    assert ei.value.status == -10


@pytest.mark.parametrize("left,right,text", [
    ([], [], "width must be in 1 .. SMI_PERM_MAX_WIDTH (8)"),
    (list(range(9)), list(range(9)), "width must be in 1 .. SMI_PERM_MAX_WIDTH (8)"),
    ([0, 12], [1, 2], "left_col must be < n_cols"),
    ([0, 1], [1, 12], "right_col must be < n_cols"),
])
def test_plan_refusals_name_the_limit(s, left, right, text):
    from stark_rs_amd.mirror import Air
    p = xc.PRIMES[0][0]
    air = Air(12).permutation(left, right)
    with pytest.raises(s.StarkMiError) as ei:
        plan(s, p, air, 12, 5, 3)
    assert ei.value.status == -50 and text in str(ei.value)


def test_plan_keeps_the_refusals_of_the_air(s):
    from stark_rs_amd.mirror import Air
    p = xc.PRIMES[0][0]
    air = Air(2).permutation([0], [1])
    with pytest.raises(s.StarkMiError, match="log_n must be in 1 .. 27"):
        plan(s, p, air, 2, 0, 3)
    with pytest.raises(s.StarkMiError, match="1..64 columns"):
        plan(s, p, Air(65).permutation([0], [1]), 65, 5, 3)
    with pytest.raises(s.StarkMiError, match="offsets must be in 1 .. p-1"):
        plan(s, p, air, 2, 5, 3, tau=0)


def test_mirror_permutation(s):
    from stark_rs_amd.mirror import Air
    p, g = xc.PRIMES[1]
    air = Air(5)
    assert air.perm is None and air.flatten(p).perm is None
    air.permutation([0, 1], [2, 3])
    flat = air.flatten(p)
    assert flat.perm.width == 2 and [flat.perm.left_col[j] for j in range(2)] == [0, 1] and [flat.perm.right_col[j] for j in range(2)] == [2, 3]
    with pytest.raises(ValueError, match="one permutation per AIR"):
        air.permutation([0], [1])
    with pytest.raises(ValueError, match="one width"):
        Air(3).permutation([0, 1], [2])
    ch = [int(x) for x in np.random.default_rng(1).integers(1, 1 << 63, 8)]
    alpha, gamma = pm.alpha_gamma(ch, p)
    cols, left, right = pm.shuffled_copy(16, 2, p)
    assert Air(5).permutation(left, right).closes(p, g, cols, alpha, gamma)
    assert pm.column(cols, left, right, ch, p, g)[1]
    for kind in ("cell", "multiplicity", "columnwise"):
        cols, left, right = pm.non_closing(kind, 16, p)
        assert not Air(len(cols)).permutation(left, right).closes(p, g, cols, alpha, gamma), kind
        assert not pm.column(cols, left, right, ch, p, g)[1], kind


def test_declarations(s):
    from stark_rs_amd import _lib
    declared = s.declared_symbols()
    header = open(os.path.join(ROOT, "include", "stark_mi.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "stark_mi.rs")).read()
    import ctypes as C
    lib = C.CDLL(_lib.LIB_PATH) if os.path.exists(_lib.LIB_PATH) else None
    for name in ENTRY_POINTS:
        assert name in declared
        assert re.search(r"pub fn " + name + r"\(", rust), name
        assert re.search(r"\b" + name + r"\(", rust[rust.index("// END GENERATED"):]) or name == "smi_dev_air_compose_perm", name
        if lib is not None:
            assert hasattr(lib, name), name
    assert "#define SMI_PERM_MAX_WIDTH 8" in header and "pub const SMI_PERM_MAX_WIDTH: u32 = 8;" in rust
    assert re.search(r"pub struct smi_air_perm \{\s*pub width: u32,\s*pub reserved0: u32,\s*pub left_col: \*const u32,\s*pub right_col: \*const u32,\s*\}", rust)
    assert C.sizeof(_lib.AirPerm) == 24
    assert "one permutation per proof" in header and "committed extension-field columns (an\n *   auxiliary trace); out-of-domain" not in header


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_restated_column_is_the_definition_row_by_row(p, g):
    """z[r+1] = z[r] f_L(r) / f_R(r) with a separate inversion per row, against the restatement's one walked-back inversion
    and against the vectorised recurrence"""
    n = 32
    cols, left, right = pm.shuffled_copy(n, 2, p, 3)
    ch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, (1 << 64) - 1, 8, dtype=np.uint64)]
    z, closes, zero = pm.column(cols, left, right, ch, p, g)
    assert zero is None and closes
    alpha, gamma = pm.alpha_gamma(ch, p)
    apow = pm.alpha_powers(alpha, 2, p, g)
    cur = [1, 0, 0, 0]
    for r in range(n):
        assert [int(v) for v in z[:, r]] == cur
        row = [c[r] for c in cols]
        cur = xc.mul(cur, xc.mul(pm.tuple_value(row, left, apow, gamma, p), xc.inv(pm.tuple_value(row, right, apow, gamma, p), p, g), p, g), p, g)
    assert cur == [1, 0, 0, 0]
    assert pm.recurrence_holds(z, cols, left, right, ch, p, g)
    a, b = np.random.default_rng(5).integers(0, p, (2, 4, 9), dtype=np.uint64)
    got = pm.mul_vec(a, b, p, g)
    for i in range(9):
        assert [int(v) for v in got[:, i]] == xc.mul([int(v) for v in a[:, i]], [int(v) for v in b[:, i]], p, g)
