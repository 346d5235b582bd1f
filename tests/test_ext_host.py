"""CPU: the quartic extension's host side -- smi_ext_mul / smi_ext_inv through libstarkmi.so (no context, no GPU) against
the Python restatement (tests/ext_compose.py), the mirror's Ext4, and the declarations in the header, the ctypes table
and the Rust binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ext_compose as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["smi_ext_mul", "smi_ext_inv", "smi_dev_fri_fold_ext", "smi_dev_air_compose_ext", "smi_dev_fri_prove_ext", "smi_fri_verify_ext",
       "smi_dev_air_prove_ext", "smi_air_verify_ext"]


@pytest.fixture(scope="module")
def L():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    return _lib.lib()


def _call(fn, p, g, *elems):
    arrs = [(C.c_uint64 * 4)(*e) for e in elems]
    out = (C.c_uint64 * 4)()
    return fn(p, g, *arrs, out), [int(v) for v in out]


def _operands(p, seed):
    rng = np.random.default_rng(seed)
    ops = [[int(v) for v in rng.integers(0, p, 4)] for _ in range(24)]
    ops += [[p - 1] * 4, [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0, p - 1], [p - 1, 0, 0, 0], [0, p - 1, 0, 1], [2, 0, p - 2, 0]]
    return ops


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_ext_mul_equals_the_restatement(L, p, g):
    ops = _operands(p, 1)
    for a in ops:
        for b in ops[::3]:
            st, got = _call(L.smi_ext_mul, p, g, a, b)
            assert st == 0 and got == xc.mul(a, b, p, g), (a, b)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_ext_inv_is_the_inverse_and_equals_the_restatement(L, p, g):
    one = xc.embed(1, p)
    for k, a in enumerate(_operands(p, 2)):
        st, ai = _call(L.smi_ext_inv, p, g, a)
        assert st == 0, a
        st, prod = _call(L.smi_ext_mul, p, g, a, ai)
        assert st == 0 and prod == one, a
        assert xc.mul(a, ai, p, g) == one
        if k % 4 == 0:   # a^(q-2): 120 squarings in Python, on a sample
            assert ai == xc.inv(a, p, g)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_frobenius_has_order_four(L, p, g):
    """X^(p^2) != X and X^(p^4) = X: the field has p^4 elements and no subfield of p^2 holds X (so X^4 - g is irreducible)"""
    X = [0, 1, 0, 0]

    def lib_pow(a, e):
        r, b = xc.embed(1, p), list(a)
        while e:
            if e & 1:
                st, r = _call(L.smi_ext_mul, p, g, r, b)
                assert st == 0
            st, b = _call(L.smi_ext_mul, p, g, b, b)
            assert st == 0
            e >>= 1
        return r
    assert lib_pow(X, p * p) != X
    assert lib_pow(X, p ** 4) == X
    assert lib_pow(X, p * p) == xc.power(X, p * p, p, g)


def test_refusals(L):
    a = [1, 2, 3, 4]
    p, g = xc.PRIMES[0]
    assert L.smi_status_string(-1) == b"no inverse"
    assert _call(L.smi_ext_inv, p, g, [0, 0, 0, 0])[0] == -1                 # the reference's "no inverse"
    assert _call(L.smi_ext_mul, p, 4, a, a)[0] == -50                        # 4 = 2^2 is a square
    assert _call(L.smi_ext_inv, p, 9, a)[0] == -50
    assert _call(L.smi_ext_mul, p, 0, a, a)[0] == -50
    assert _call(L.smi_ext_mul, p, p, a, a)[0] == -50
    for p3 in (7, 1000003):   # primes that are 3 mod 4
        assert p3 % 4 == 3
        for gg in range(1, 7):
            assert _call(L.smi_ext_mul, p3, gg, a, a)[0] == -50
    assert _call(L.smi_ext_mul, 21, 2, a, a)[0] == -50                       # 21 = 1 mod 4, not a prime
    assert _call(L.smi_ext_mul, 1 << 32 | 5, 2, a, a)[0] == -50
    assert _call(L.smi_ext_mul, p, g, [p, 0, 0, 0], a)[0] == -51             # non-canonical
    assert _call(L.smi_ext_mul, p, g, a, [0, 0, 0, p])[0] == -51
    assert _call(L.smi_ext_inv, p, g, [0, 1 << 63, 0, 0])[0] == -51
    assert not xc.field_ok(p, 4) and not xc.field_ok(7, 3) and all(xc.field_ok(*pg) for pg in xc.PRIMES)


def test_small_field_exhaustively(L):
    """p = 13 (1 mod 4), g = 2 (a non-square): every non-zero element of a sample line has its inverse"""
    p, g = 13, 2
    assert xc.field_ok(p, g)
    for v in range(1, p ** 4, 7):
        a = [v % p, v // p % p, v // p ** 2 % p, v // p ** 3 % p]
        st, ai = _call(L.smi_ext_inv, p, g, a)
        assert st == 0 and xc.mul(a, ai, p, g) == [1, 0, 0, 0], a


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_mirror_ext4(L, p, g):
    from stark_rs_amd import StarkMiError
    from stark_rs_amd.mirror import Ext4
    a, b = Ext4([5, p - 1, 7, 123456], p, g), Ext4([p - 2, 0, 3, 1], p, g)
    assert list((a * b).c) == xc.mul(a.c, b.c, p, g)
    assert (a / b) * b == a and a * a.inv() == Ext4.embed(1, p, g)
    assert list((a + b).c) == xc.add(a.c, b.c, p) and list((a - b).c) == xc.sub(a.c, b.c, p) and (-a) + a == Ext4.embed(0, p, g)
    assert list(a.pow(p + 3).c) == xc.power(a.c, p + 3, p, g)
    assert a * 3 == a + a + a
    with pytest.raises(StarkMiError, match="no inverse"):
        Ext4.embed(0, p, g).inv()


def test_declared_in_the_header_the_ctypes_table_and_the_rust_binding(L):
    import stark_rs_amd as s
    declared = s.declared_symbols()
    rust = open(os.path.join(ROOT, "bindings", "stark_mi.rs")).read()
    header = open(os.path.join(ROOT, "include", "stark_mi.h")).read()
    assert re.search(r"#define SMI_EXT_DEGREE 4\b", header)
    for name in NEW:
        assert name in declared, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert re.search(r"pub fn smi_dev_fri_fold_ext\(ctx: \*mut smi_ctx, d_in: \*const u32, len: usize, stride: usize, d_alpha: \*const u64, "
                     r"offset: u64, omega: u64, d_out: \*mut u32, out_stride: usize\) -> c_int;", rust)
    assert re.search(r"pub fn smi_ext_inv\(p: u64, g: u64, a: \*const u64, out: \*mut u64\) -> c_int;", rust)
