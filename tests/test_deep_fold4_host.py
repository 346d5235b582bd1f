"""CPU: out-of-domain sampling over coset leaves (include/stark_mi.h, "Out-of-domain sampling over coset leaves") without a
GPU -- the two layout entry points against the header's byte formula and against the lengths of restated proofs
(tests/deep_fold4_compose.py), the engine keyword's refusals, the sentences of the two verifiers against the restatement's,
and the declarations."""
import os
import re

import pytest

import air_compose as ac
import deep_args_compose as da
import deep_compose as dc
import deep_fold4_compose as d4
import ext_compose as xc
import fold4_compose as f4
import xargs_compose as xa
from test_deep_host import quartic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["smi_dev_merkle_build_cosets", "smi_air_deep_fold4_layout", "smi_dev_air_prove_deep_fold4", "smi_air_verify_deep_fold4",
                "smi_air_deep_xargs_fold4_layout", "smi_dev_air_prove_deep_xargs_fold4", "smi_air_verify_deep_xargs_fold4"]


def lib_layout(p, g, air, W, log_n, lb, t, listed=False):
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    s.build()
    cfg = _lib.StarkCfg(log_n, lb, W, 1, 1, g, t, 1)
    flat = air.flatten(p)
    if listed:
        return s.engine.air_deep_args_fold4_layout(p, flat, s.engine.xargs_of(flat), cfg)
    return s.engine.air_deep_fold4_layout(p, flat, cfg)


def formula(p, g, W, A, D, log_n, lb, t):
    """the header's byte formula, with len_FRI4 from the library's smi_fri_fold4_layout"""
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    s.build()
    N, log_N = 1 << (log_n + lb), log_n + lb
    folds, _last, fri = s.engine.fri_fold4_layout(_lib.FriCfg(1, g, N, 1 << lb, t))
    groups = [W, 4 * D] if A == 0 else [W, 4 * A, 4 * D]
    return folds, 9 + 32 * (2 * W + 2 * A + D) + fri + sum(t * (9 + 32 * V) + t * (9 + 32 * (log_N - 2)) for V in groups)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_layouts_equal_the_byte_formula(p, g):
    for log_n, lb, t in ((3, 3, 4), (4, 3, 4), (5, 3, 4), (6, 3, 4), (7, 3, 4), (5, 2, 4), (8, 2, 6), (20, 3, 32), (21, 2, 32)):
        n = 1 << min(log_n, 6)                                                # the statement's shape, not its trace, decides the layout
        for air, W in ((ac.make("fib", n, p)[0], 2), (ac.make("mixer", n, p)[0], len(ac.make("mixer", n, p)[1])), (quartic(n, p)[0], 1)):
            D = dc.plan(air)[1]
            if D > 1 << lb:
                continue
            got = lib_layout(p, g, air, W, log_n, lb, t)
            assert got == formula(p, g, W, 0, D, log_n, lb, t) == d4.layout(W, 0, D, log_n, lb, t), (log_n, lb, W, D)
        for name, (air, cols, args) in da.small_lists(16, p).items():
            import copy
            D = da.plan(air, args)[1]
            if D > 1 << lb:
                continue
            got = lib_layout(p, g, xa.mirror_air(copy.deepcopy(air), args), len(cols), log_n, lb, t, listed=True)
            assert got == formula(p, g, len(cols), len(args), D, log_n, lb, t) == d4.layout(len(cols), len(args), D, log_n, lb, t), (name, log_n, lb)
    # the two opening sections at N = 2^23, t = 32, W = 4, D = 2: 56 448 bytes against 102 656 with two rows and two full paths
    assert sum(d4.section_len(V, 32, 23) for V in (4, 8)) == 56448
    assert 2 * 32 * (9 + 8 * 4) + 2 * 32 * (9 + 32 * 23) + 2 * 32 * (9 + 32 * 2) + 2 * 32 * (9 + 32 * 23) == 102656


def test_the_fold_counts_the_gpu_tests_rely_on():
    """N = 64 at B = 8 and t = 4 has no fold; 128 and 256 one, 512 and 1024 two; R2 - 1 takes both parities"""
    got = {log_N: f4.layout(1 << log_N, 8, 4)[:2] for log_N in range(6, 11)}
    assert {k: v[1] for k, v in got.items()} == {6: 0, 7: 1, 8: 1, 9: 2, 10: 2}
    assert {(v[0] - 1) % 2 for k, v in got.items() if v[1]} == {0, 1}
    assert f4.layout(128, 4, 4)[1] == 1 and f4.layout(64, 4, 4)[1] == 0


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_restated_proofs_have_the_layouts_length_and_verify(oracle, p, g):
    t = 4
    for name, log_n, lb in (("fib", 4, 3), ("mixer", 6, 3), ("fib", 5, 2)):
        air, cols = ac.make(name, 1 << log_n, p)
        W, D = len(cols), dc.plan(air)[1]
        res = d4.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g, bits=3)
        F, length = lib_layout(p, g, air, W, log_n, lb, t)
        assert len(res["proof"]) == length and F == d4.folds(log_n, lb, t) >= 1
        assert d4.verify(oracle, air, None, res["proof"], res["roots"], p, g, W, log_n, lb, t, 1, g, 3) == (True, "")
    import copy
    for name in ("perm", "lookup_per"):
        air, cols, args = da.small_lists(16, p)[name]
        W, A, D = len(cols), len(args), da.plan(air, args)[1]
        res = d4.prove_args(oracle, air, args, cols, p, g, 4, 3, t, 1, g)
        assert len(res["proof"]) == lib_layout(p, g, xa.mirror_air(copy.deepcopy(air), args), W, 4, 3, t, listed=True)[1]
        assert d4.verify(oracle, air, args, res["proof"], res["roots"], p, g, W, 4, 3, t, 1, g) == (True, "")


def test_engine_keyword_refusals():
    """host-side checks of the Engine's dispatch that need no device: a stand-in object carries the methods' self"""
    from stark_rs_amd.engine import Engine
    from stark_rs_amd.mirror import Air
    eng = Engine.__new__(Engine)
    eng.p = xc.PRIMES[0][0]
    plain, listed = Air(2), Air(2).add_permutation([0], [1])
    roots = [bytes(32)] * 3
    for air, kw, word in ((plain, dict(deep=True), "row_leaves=True, ext=True"), (plain, dict(deep=True, row_leaves=True), "row_leaves=True, ext=True"),
                          (plain, dict(deep=True, ext=True), "row_leaves=True, ext=True"), (plain, dict(row_leaves=True, ext=True), "deep=True"),
                          (listed, dict(row_leaves=True, ext=True), "deep_args=True"),
                          (listed, dict(row_leaves=True, ext=True, deep=True, deep_args=True), "exactly one")):
        with pytest.raises(ValueError, match=word):
            eng.dev_air_prove(air, 0, 2, 4, 3, 4, coset_leaves=True, **kw)
        with pytest.raises(ValueError, match=word):
            eng.air_verify(air, b"", roots, 2, 4, 3, 4, coset_leaves=True, **kw)
    # the variants keep their own refusals: folding stays 2, a plain AIR has no list, a list is not a plain AIR
    for air, kw in ((plain, dict(deep=True, folding=4)), (listed, dict(deep_args=True, folding=4)), (plain, dict(deep_args=True)), (listed, dict(deep=True))):
        with pytest.raises(ValueError):
            eng.dev_air_prove(air, 0, 2, 4, 3, 4, coset_leaves=True, row_leaves=True, ext=True, **kw)
        with pytest.raises(ValueError):
            eng.air_verify(air, b"", roots, 2, 4, 3, 4, coset_leaves=True, row_leaves=True, ext=True, **kw)


def _body(src, head):
    at = src.index(head)
    return src[at:src.index("\n}\n", at)]


def test_the_sentences_of_the_two_verifiers_are_the_restatement_s():
    """Reads the source: every verdict air_verify_deep_fold4_impl (verify.hip) can give -- a sentence defined in deep_core.h, a
    member of its two OpeningWords tables, or a verdict of the fold-by-4 FRI walk it calls (pinned to tests/fold4_compose.py by
    tests/test_fold4_host.py) -- is a sentence of tests/deep_fold4_compose.py, and the other way round.  The function holds no
    literal of its own: tests/test_air_transcript_host.py pins verify.hip's literals to the recorded fixture."""
    csrc = os.path.join(ROOT, "stark_rs_amd", "csrc")
    src = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, "verify.hip")).read().splitlines())
    core = open(os.path.join(csrc, "deep_core.h")).read()
    lit = r'"((?:[^"\\]|\\.)*)"'
    body = re.sub(r"smi_fail\([^;]*;", "", _body(src, "static int air_verify_deep_fold4_impl("))
    assert not re.findall(lit, body)

    def macro(name):
        m = re.search(r"#define " + name + r"\s*(?:\\\n)?\s*" + lit, core)
        assert m, name
        return m.group(1)
    found = set()
    for arg in re.findall(r"reject\(ctx, accept, ([^)]*)\)", body):
        if re.fullmatch(r"DEEP_[A-Z0-9_]+", arg):
            found.add(macro(arg))
        else:
            assert re.fullmatch(r"say\.(length|row|path|auth|canonical|composition)", arg), arg
    assert "const OpeningWords &say = xargs ? DEEP_ARGS_FOLD4_WORDS : DEEP_FOLD4_WORDS;" in body
    for table in ("DEEP_FOLD4_SENTENCES", "DEEP_ARGS_FOLD4_SENTENCES"):
        words = re.search(r"static const char \*const " + table + r"\[6\] = \{([^}]*)\}", core).group(1)
        got = re.findall(lit, words)
        assert len(got) == 6
        found |= set(got)
        assert re.search(r"const OpeningWords DEEP_(ARGS_)?FOLD4_WORDS = \{" + ",\\s*".join(table + r"\[%d\]" % i for i in range(6)) + r"\}", src), table
    for name in ("fri_walk_fold4(", "deep_coset_parse(", "auth_section(", "deep_coset_q_matches("):
        assert name in body, name
    assert found | f4.FRI_SENTENCES == d4.SENTENCES
    assert found == set(d4.FRONT.values()) | set(d4.WORDS.values()) | set(d4.ARGS_WORDS.values())


def test_the_entry_points_are_declared_everywhere():
    import stark_rs_amd
    from stark_rs_amd import _lib
    header = open(os.path.join(ROOT, "include", "stark_mi.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "stark_mi.rs")).read()
    assert "Out-of-domain sampling over coset leaves" in header
    stark_rs_amd.build()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert "pub fn %s(" % name in rust, name
        assert getattr(_lib.lib(), name).argtypes is not None, name
    assert set(ENTRY_POINTS) <= set(stark_rs_amd.declared_symbols())
