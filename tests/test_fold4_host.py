"""CPU: the restated fold by 4 (tests/fold4_compose.py, Lagrange through a coset) against the fold by 2 applied twice, and
smi_fri_fold4_layout (host only) against the restated layout."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ext_compose as xc
import fold4_compose as f4

U64_MAX = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _alphas(p):
    return [[U64_MAX] * 4, [p, p + 1, U64_MAX - 1, 2 * p - 1], [0, 0, 0, 0], [5, 0, 0, 0], [0, 0, 0, 1], [1 << 63, 12345, p - 1, 1 << 32]]


def _codewords(p, L, seed):
    rng = np.random.default_rng(seed)
    cw = rng.integers(0, p, (4, L), dtype=np.uint64)
    cw[:, 0] = p - 1
    cw[:, L // 4] = [0, p - 1, 0, p - 1]
    yield cw
    yield np.full((4, L), p - 1, dtype=np.uint64)
    yield np.zeros((4, L), dtype=np.uint64)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_len", range(2, 9))
def test_restated_fold4_is_the_fold_by_2_under_alpha_then_alpha_squared(oracle, p, g, log_len):
    L = 1 << log_len
    omega, offset = oracle.ff_prim_nth_root_g(L, p, g), [g, 7, 1][log_len % 3]
    for cw in _codewords(p, L, log_len):
        for al in _alphas(p):
            assert np.array_equal(f4.fold4(cw, al, offset, omega, p, g), f4.two_folds(cw, al, offset, omega, p, g)), al


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_a_cubic_folds_to_its_value_at_alpha(oracle, p, g):
    """the definition itself: a codeword that IS a polynomial of degree < 4 over F_q folds to P(alpha) in every element"""
    L = 16
    omega, offset = oracle.ff_prim_nth_root_g(L, p, g), g
    rng = np.random.default_rng(1)
    coef = [[int(v) for v in rng.integers(0, p, 4)] for _ in range(4)]   # four F_q coefficients

    def at(x):   # Horner over F_q, x: four residues
        acc = [0, 0, 0, 0]
        for c in reversed(coef):
            acc = xc.add(xc.mul(acc, x, p, g), c, p)
        return acc
    cw = np.array([at(xc.embed(offset * pow(omega, i, p) % p, p)) for i in range(L)], dtype=np.uint64).T
    al = [U64_MAX, 3, p + 9, 1 << 40]
    got = f4.fold4(cw, al, offset, omega, p, g)
    assert all([int(v) for v in got[:, i]] == at([a % p for a in al]) for i in range(L // 4))


def _status(name):
    text = open(os.path.join(ROOT, "include", "stark_mi.h")).read()
    return int(re.search(r"\b%s = (-?\d+)," % name, text).group(1))


def _layout(cfg):
    from stark_rs_amd import _lib
    folds, last, plen = C.c_uint64(), C.c_uint64(), C.c_size_t()
    st = _lib.lib().smi_fri_fold4_layout(C.byref(cfg), C.byref(folds), C.byref(last), C.byref(plen))
    return st, folds.value, last.value, plen.value


def test_fold4_layout_equals_the_restatement():
    from stark_rs_amd import _lib
    no_rounds = _status("SMI_ERR_NO_ROUNDS")
    cases = [(32, 4, 2), (64, 4, 3), (128, 4, 4), (256, 8, 5), (1 << 23, 8, 32), (1 << 25, 8, 32), (8, 8, 1)]   # test_num_rounds_host_logic's
    cases += [(1 << ln, E, t) for ln in range(2, 15) for E in (4, 8, 16) for t in (1, 2, 5, 32)]
    seen_f, seen_parity = set(), set()
    for N, E, t in cases:
        R2, F, last, n = f4.layout(N, E, t)
        st, folds, last_len, plen = _layout(_lib.FriCfg(1, 1, N, E, t))
        if R2 == 0:                                     # the reference rule admits no round: refused as today
            assert st == no_rounds, (N, E, t)
            continue
        assert (st, folds, last_len, plen) == (0, F, last, n), (N, E, t)
        assert last == N // 4 ** F and last > E and last >= N >> (R2 - 1)
        seen_f.add(F)
        seen_parity.add((R2 - 1) % 2)
    assert {0, 1, 2, 3} <= seen_f and seen_parity == {0, 1}
    assert f4.layout(1 << 25, 8, 32)[:3] == (18, 8, 1 << 9)


def test_fold4_layout_refusals():
    from stark_rs_amd import _lib
    L = _lib.lib()
    cfg = _lib.FriCfg(1, 1, 64, 4, 2)
    x, s = C.c_uint64(), C.c_size_t()
    assert L.smi_fri_fold4_layout(None, C.byref(x), C.byref(x), C.byref(s)) == _status("SMI_ERR_BAD_ARG")
    assert L.smi_fri_fold4_layout(C.byref(cfg), None, C.byref(x), C.byref(s)) == _status("SMI_ERR_BAD_ARG")
    assert _layout(_lib.FriCfg(1, 1, 96, 4, 2))[0] == _status("SMI_ERR_DOMAIN_NOT_POW2")
    assert _layout(_lib.FriCfg(1, 1, 64, 6, 2))[0] == _status("SMI_ERR_EXPANSION_NOT_POW2")
    assert _layout(_lib.FriCfg(1, 1, 64, 2, 2))[0] == _status("SMI_ERR_EXPANSION_TOO_SMALL")


def test_the_python_wrapper_of_the_layout():
    from stark_rs_amd import _lib
    from stark_rs_amd.engine import fri_fold4_layout
    import stark_rs_amd as s
    assert fri_fold4_layout(_lib.FriCfg(1, 1, 1 << 25, 8, 32)) == f4.layout(1 << 25, 8, 32)[1:]
    with pytest.raises(s.StarkMiError):
        fri_fold4_layout(_lib.FriCfg(1, 1, 8, 8, 1))


HOST_SHAPES = [(6, 4, 1, 0), (6, 8, 5, 8), (8, 8, 5, 0), (9, 4, 5, 8), (9, 8, 3, 0)]   # (log N, E, t, bits): R2 - 1 odd and even, F = 0 .. 3


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n,E,t,bits", HOST_SHAPES)
def test_restated_prove_then_restated_verify_accepts(oracle, p, g, log_n, E, t, bits):
    N = 1 << log_n
    for prior in (b"", b"\x07" * 37):
        cfg, cw, proof, top, nonce = f4.shared_proof(oracle, p, g, log_n, E, t, bits, prior)
        R2, F, last, n = f4.layout(N, E, t)
        assert len(proof) == n and len(top) == t and len({s % last for s in top}) == t
        ok, pv, used, top_v, why = f4.verify(oracle, cfg, proof, g, prior, bits)
        assert ok and why == "" and used == n and top_v == top
        assert len(pv) == (4 * t if F else 0)
        for idx, val in pv:                                   # the layer-0 cosets are the codeword's own elements
            assert val == [int(v) for v in cw[:, idx]]
        assert not f4.verify(oracle, cfg, proof, g, prior + b"x", bits)[0]
        if bits:
            assert f4.verify(oracle, cfg, proof, g, prior, bits - 3)[0]                      # a lower demand is met
            assert f4.verify(oracle, cfg, proof, g, prior, 24)[4] == "proof of work"


def test_the_shapes_cover_both_parities_and_every_fold_count():
    got = [f4.layout(1 << ln, E, t)[:2] for ln, E, t, _b in HOST_SHAPES]
    assert {(R2 - 1) % 2 for R2, _F in got} == {0, 1} and {F for _R2, F in got} >= {0, 1, 2}


@pytest.mark.parametrize("p,g", xc.PRIMES[1:])
@pytest.mark.parametrize("log_n,E,t,bits", [(8, 8, 5, 0), (9, 4, 5, 8)])
def test_every_mutation_class_is_rejected_with_its_sentence(oracle, p, g, log_n, E, t, bits):
    N = 1 << log_n
    cfg, _cw, proof, _top, nonce = f4.shared_proof(oracle, p, g, log_n, E, t, bits)
    muts = f4.mutations(proof, N, E, t, p)
    kinds = {name.split(" at ")[0].split(" 0")[0] for name, _m, _w in muts}
    assert len(muts) > 2 * t and any("coordinate + p in coset" in k for k in kinds)
    for name, m, want in muts:
        ok, _pv, _used, _top, why = f4.verify(oracle, cfg, m, g, b"", bits)
        assert not ok and why, name
        assert want is None or why == want, (name, why)
    at = [a for kind, _r, a in f4.objects(N, E, t)[0] if kind == "nonce"][0]
    wrong = bytearray(proof)
    wrong[at + 9:at + 17] = (nonce + 1).to_bytes(8, "little")
    ok, _pv, _used, _top, why = f4.verify(oracle, cfg, bytes(wrong), g, b"", bits)
    assert not ok and why in ("proof of work", "merkle authentication path verification fails for aa", f4.FOLD4_MISMATCH), why


@pytest.mark.parametrize("p,g", xc.PRIMES[:1])
def test_a_coset_that_does_not_fold_to_the_next_layer_is_rejected(oracle, p, g):
    """an honest tree over a codeword that is NOT the fold of the previous one: every path verifies, the fold does not"""
    log_n, E, t = 8, 4, 3
    N = 1 << log_n
    cw, omega = f4.low_degree_codeword(oracle, p, g, N, E, g, 5)
    cfg = oracle.fri_cfg(omega, g, N, E, t, p)
    real = f4.fold4
    try:
        def crooked(c, alpha, offset, om, pp, gg):
            out = real(c, alpha, offset, om, pp, gg)
            out[2] = (out[2] + np.uint64(1)) % np.uint64(pp)      # every element of every later layer is off by X^2
            return out
        f4.fold4 = crooked
        proof, _top, _nonce = f4.prove(oracle, cfg, cw, g)
    finally:
        f4.fold4 = real
    ok, _pv, _used, _top, why = f4.verify(oracle, cfg, proof, g)
    assert not ok and why == f4.FOLD4_MISMATCH


def _body(src, head):
    """the text of the function whose definition starts with `head`, up to the first closing brace in column 0"""
    at = src.index(head)
    return src[at:src.index("\n}\n", at)]


def test_the_sentences_of_the_factor_4_verifiers_are_the_restatement_s():
    """Reads the source: every verdict fri_walk_fold4 and air_verify_fold4_impl (verify.hip) can give -- a literal, the one
    sentence defined in fri_core.h, a member of AIR_WORDS, or a sentence of the ExtFri rules they call -- is a sentence of
    tests/fold4_compose.py, and the other way round.  A sentence added to either verifier fails here until the restatement
    (and with it the GPU comparisons of tests/test_gpu_fold4.py) knows it."""
    csrc = os.path.join(ROOT, "stark_rs_amd", "csrc")
    src = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, "verify.hip")).read().splitlines())
    core = open(os.path.join(csrc, "fri_core.h")).read()
    lit = r'"((?:[^"\\]|\\.)*)"'
    walk, air = _body(src, "int fri_walk_fold4("), _body(src, "static int air_verify_fold4_impl(")
    found = set()
    nonce = _body(src, "int nonce_record(")                      # the step the walk shares with fri_walk
    for body in (walk, air, nonce):
        body = re.sub(r"smi_fail\([^;]*;", "", body)             # the message of a status is not a verdict
        found |= set(re.findall(lit, body))
        for arg in re.findall(r"reject\(ctx, accept, ([^)]*)\)", body):
            arg = arg.strip()
            if arg.startswith('"'):
                continue
            if arg == "FOLD4_MISMATCH":
                assert re.search(r"const char \*const FOLD4_MISMATCH = FRI_FOLD4_MISMATCH_SENTENCE;", src)
                found.add(re.search(r"#define FRI_FOLD4_MISMATCH_SENTENCE " + lit, core).group(1))
            else:
                assert re.fullmatch(r"say\.(length|row|path|auth|canonical|composition)", arg), arg
    assert "const OpeningWords &say = AIR_WORDS;" in air
    words = re.search(r"const OpeningWords AIR_WORDS = \{([^}]*)\}", src).group(1)
    found |= set(re.findall(lit, words))                          # parse_section and auth_section speak through `say`
    ext = _body(src, "struct ExtFri {")                           # the rules the walk calls: draw, last_shape, low_degree
    for rule in ("int last_shape(", "int low_degree("):
        found |= set(re.findall(lit, ext[ext.index(rule):ext.index("\n    }\n", ext.index(rule))]))
    assert "return reject(ctx, accept, LOW_DEGREE)" in ext
    found.add(re.search(r"const char \*const LOW_DEGREE = " + lit, src).group(1))
    assert found == f4.FRI_SENTENCES | set(f4.AIR_WORDS.values())
    for name in ("K.last_shape(", "K.low_degree(", "nonce_record(", "last_domain(", "parse_section(", "auth_section("):
        assert name in walk + air, name


def test_the_entry_points_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "stark_mi.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "stark_mi.rs")).read()
    from stark_rs_amd import _lib
    for name in ("smi_fri_fold4_layout", "smi_dev_fri_fold4_ext", "smi_dev_fri_prove_ext_fold4", "smi_fri_verify_ext_fold4"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert "pub fn %s(" % name in rust, name
        assert hasattr(_lib.lib(), name)
    assert re.search(r"pub fn smi_dev_fri_fold4_ext\(ctx: \*mut smi_ctx, d_in: \*const u32, len: usize, stride: usize, d_alpha: \*const u64, "
                     r"offset: u64, omega: u64, d_out: \*mut u32, out_stride: usize\) -> c_int;", rust)
