"""GPU: every DEEP kernel and prover under a caller's trace_offset tau and lde_offset h (include/stark_mi.h, "Out-of-domain
sampling" and the sections after it).  The other GPU tests pass tau = 1 and h = g, which is what lde_offset=None already means:
a launcher, a kernel instantiation, a prover step or a verifier branch that took g for h or 1 for tau would pass all of them.
Here the three codeword kernels run at h in {11, p - 2}, and one proof per prover at four offset pairs -- two of which move one
offset only, so that a failure names the offset -- equals the restatement byte for byte, verifies under its offsets and is
rejected under the default ones, by the library and by the restatement for the same class of sentence.  At the reference modulus
and, for the plain and the window provers and the kernels, at the boundary moduli of tests/test_gpu_boundary_primes.py.  Every
comparison is exact; every case asserts that its reference under the default offsets differs.  `pytest -m gpu`."""
import numpy as np
import pytest

import deep_args_compose as da
import deep_compose as dc
import deep_fold4_compose as d4
import ext_compose as xc
import fold4_compose as f4
import window_compose as wc
import zk_args_compose as za
from test_gpu_air import Dev
from test_gpu_air_window import check_codeword
from test_gpu_boundary_primes import GEN as BOUNDARY_GEN, THREE
from test_gpu_deep import check_compose, make_air
from test_gpu_deep_args import SHAPES, check_compose as check_compose_args, mirror
from test_gpu_zk import engines  # noqa: F401  (a fixture: one context per modulus, the reference modulus among them)

pytestmark = pytest.mark.gpu
P_REF, G_REF = xc.PRIMES[0]
GEN = dict(BOUNDARY_GEN)
GEN[P_REF] = G_REF
FIELDS = [P_REF] + THREE
SEED = bytes(range(32))
PLAIN = dict(row_leaves=True, ext=True, deep=True)
LIST = dict(row_leaves=True, ext=True, deep_args=True)
# prover -> (statements, (log_n, log_blowup, t), the engine's keywords, coset leaves, also at the boundary moduli)
FAMILIES = {"deep": (("mimc", "mixer"), (6, 3, 4), PLAIN, False, True),                                    # mimc: a periodic column
            "deep cosets": (("mixer",), (5, 2, 4), dict(PLAIN, coset_leaves=True), True, False),
            "window": (("tap4", "wide"), (5, 3, 4), PLAIN, False, True),                                   # a periodic read at shift 3, D = 4; boundary rows 0, 1
            "window cosets": (("tap4", "sq"), (5, 3, 4), dict(PLAIN, coset_leaves=True), True, False),
            "list": (("nine", "selectors"), (5, 2, 4), LIST, False, False),
            "list cosets": (("nine",), (5, 2, 4), dict(LIST, coset_leaves=True), True, False),
            "zk list": (("vm",), (6, 2, 1), dict(LIST, coset_leaves=True), True, False)}                  # the smallest shape of tests/test_gpu_zk_args.py


def offsets(p):
    """(tau, h): both moved; h alone; tau alone (h = g, the default, written out); both at the top of the field"""
    return [(5, 11), (1, 11), (5, GEN[p]), (p - 1, p - 2)]


def assert_accepted(p, tau, h, log_N):
    """the library's two rules for an offset pair (air_core.h): a pair it would refuse is an error of this file, not a case"""
    assert 0 < tau < p and 0 < h < p
    assert pow(h, 1 << log_N, p) != 1, (p, tau, h)
    assert pow(h * pow(tau, p - 2, p) % p, 1 << log_N, p) != 1, (p, tau, h)


def test_the_offset_pairs_are_what_the_cases_need():
    for p in FIELDS:
        g = GEN[p]
        assert 11 != g and p - 2 != g and [tau != 1 for tau, _h in offsets(p)] == [True, False, True, True]
        assert [h != g for _tau, h in offsets(p)] == [True, True, False, True]
        for tau, h in offsets(p):
            for log_N in (7, 8, 9, 10):
                assert_accepted(p, tau, h, log_N)
    for _names, (log_n, lb, t), _kw, _cosets, _three in FAMILIES.values():
        assert d4.folds(log_n, lb, t) >= 1, (log_n, lb, t)


# ---------------------------------------------------------------------------------------------- the codeword kernels alone
@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("top", [False, True], ids=["h11", "hp-2"])
def test_dev_deep_compose_under_an_offset(engines, oracle, p, top):
    h = p - 2 if top else 11
    assert_accepted(p, 1, h, 10)
    check_compose(engines[p], oracle, p, GEN[p], 10, dc.compose_combos(10), h=h)


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("top", [False, True], ids=["h11", "hp-2"])
def test_dev_deep_compose_window_under_an_offset(engines, oracle, p, top):
    """S in {2, 3, 4}: every instantiation of deep_compose_window_kernel, and the two-row kernel beside S = 2"""
    h = p - 2 if top else 11
    assert_accepted(p, 1, h, 10)
    check_codeword(engines[p], oracle, p, GEN[p], 10, h=h)


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("top", [False, True], ids=["h11", "hp-2"])
def test_dev_deep_compose_args_under_an_offset(engines, oracle, p, top):
    h = p - 2 if top else 11
    assert_accepted(p, 1, h, 10)
    check_compose_args(engines[p], oracle, p, GEN[p], 10, SHAPES, h=h)


# ---------------------------------------------------------------------------------------------- the proofs
def statement(family, name, log_n, t, p):
    """-> (the AIR the engine takes, the trace, (air, list) of the restatement or None, fill the multiplicities on the device)"""
    n = 1 << log_n
    if family in ("deep", "deep cosets"):
        air, cols = make_air(name, n, p)
        return air, cols, None, False
    if family in ("window", "window cosets"):
        air, cols = wc.make(name, n, p)
        return air, cols, None, False
    air, cols, lst = za.vm(log_n, t, p) if family == "zk list" else da.readme_lists(n, p)[name]
    return mirror(air, lst), cols, (air, lst), name == "nine"


def restated_proof(o, family, air, cols, listed, p, g, log_n, lb, t, tau, h):
    if family == "deep":
        return dc.prove(o, air, cols, p, g, log_n, lb, t, tau, h)
    if family == "deep cosets":
        return d4.prove(o, air, cols, p, g, log_n, lb, t, tau, h)
    if family in ("window", "window cosets"):
        return wc.prove(o, air, cols, p, g, log_n, lb, t, tau, h, 0, family == "window cosets")
    if family == "list":
        return da.prove(o, listed[0], listed[1], cols, p, g, log_n, lb, t, tau, h)
    if family == "list cosets":
        return d4.prove_args(o, listed[0], listed[1], cols, p, g, log_n, lb, t, tau, h)
    return za.prove(o, listed[0], listed[1], cols, SEED, p, g, log_n, lb, t, tau, h)


def restated_verdict(o, family, air, listed, proof, roots, p, g, W, log_n, lb, t, tau, h):
    """-> (accept, reason): a reason class over row leaves, the library's sentence over coset leaves"""
    roots = [bytes(r) for r in roots]
    if family == "deep":
        return dc.verify(o, air, proof, roots, p, g, W, log_n, lb, t, tau, h)
    if family == "deep cosets":
        return d4.verify(o, air, None, proof, roots, p, g, W, log_n, lb, t, tau, h)
    if family in ("window", "window cosets"):
        return wc.verify(o, air, proof, roots, p, g, W, log_n, lb, t, tau, h, 0, family == "window cosets")
    if family == "list":
        return da.verify(o, listed[0], listed[1], proof, roots, p, g, W, log_n, lb, t, tau, h)
    if family == "list cosets":
        return d4.verify(o, listed[0], listed[1], proof, roots, p, g, W, log_n, lb, t, tau, h)
    return za.verify(o, listed[0], listed[1], proof, roots, p, g, W, log_n, lb, t, tau, h)


def expected_under_the_defaults(family, tau):
    """what the restated verifier says to a proof made under (tau, h) when it is handed (1, g): with another tau the record is
    not consistent at z -- the exemption roots, the boundary points and the periodic columns sit elsewhere --, and that check
    comes first; with h alone the record is consistent and FRI's first fold, over other points, is not"""
    if tau != 1:
        return {"deep": "consistency", "window": "consistency", "list": "consistency", "deep cosets": d4.FRONT["consistency"],
                "window cosets": d4.FRONT["consistency"], "list cosets": d4.FRONT["consistency args"], "zk list": za.FRONT["consistency"]}[family]
    return "fri: colinearity" if family in ("deep", "window", "list") else f4.FOLD4_MISMATCH


def sentence_matches(family, reason, sentence):
    if family == "list":
        return da.keyword(reason) in sentence
    if family in ("deep", "window"):
        return dc.keyword(reason) in sentence
    return reason == sentence


def check_family(eng, o, family, p, pairs):
    names, (log_n, lb, t), kw, cosets, _three = FAMILIES[family]
    g = GEN[p]
    assert d4.folds(log_n, lb, t) >= 1                                       # a shape without a fold has no layer-0 query to bind Q to
    more = dict(zk=SEED) if family == "zk list" else {}
    for name in names:
        air, cols, listed, fill = statement(family, name, log_n, t, p)
        W = len(cols)
        default = restated_proof(o, family, air, cols, listed, p, g, log_n, lb, t, 1, g)
        for tau, h in pairs:
            assert_accepted(p, tau, h, log_n + lb)
            where = (family, name, p, tau, h)
            want = restated_proof(o, family, air, cols, listed, p, g, log_n, lb, t, tau, h)
            assert want["proof"] != default["proof"] and want["roots"][0] != default["roots"][0], where   # the reference sees the offsets
            trace = [list(c) for c in cols]
            if fill:
                for arg in listed[1]:
                    if arg[0] == "lookup":
                        trace[arg[3]] = [0] * len(trace[0])
            with Dev(eng) as dev:
                res = eng.dev_air_prove(air, dev.upload(np.array(trace, dtype=np.uint64)), W, log_n, lb, t, trace_offset=tau, lde_offset=h, grind_bits=0,
                                        fill_multiplicities=fill, **kw, **more)
            assert [bytes(r) for r in res["column_roots"]] == want["roots"], where
            assert [c for el in res["ood"] for c in el] == want["ood"], where
            assert res["top_indices"] == [int(v) for v in want["top"]], where
            assert res["proof"] == want["proof"], where
            zk = family == "zk list"
            ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, trace_offset=tau, lde_offset=h, grind_bits=0, zk=zk, **kw)
            assert ok, (where, why)
            assert restated_verdict(o, family, air, listed, res["proof"], res["column_roots"], p, g, W, log_n, lb, t, tau, h) == (True, ""), where
            # the same proof under the default offsets
            ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=0, zk=zk, **kw)
            ok_o, why_o = restated_verdict(o, family, air, listed, res["proof"], res["column_roots"], p, g, W, log_n, lb, t, 1, g)
            assert not ok and why and not ok_o, (where, why, why_o)
            assert why_o == expected_under_the_defaults(family, tau), (where, why, why_o)
            assert sentence_matches(family, why_o, why), (where, why, why_o)


@pytest.mark.parametrize("pair", range(4), ids=["tau5-h11", "tau1-h11", "tau5-hg", "taup-1-hp-2"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_proofs_under_offsets_equal_the_restatement_and_bind_them(engines, oracle, family, pair):
    check_family(engines[P_REF], oracle, family, P_REF, [offsets(P_REF)[pair]])


@pytest.mark.parametrize("p", THREE)
@pytest.mark.parametrize("family", [f for f, row in FAMILIES.items() if row[4]])
def test_proofs_under_offsets_at_boundary_moduli(engines, oracle, family, p):
    check_family(engines[p], oracle, family, p, [offsets(p)[0], offsets(p)[3]])
