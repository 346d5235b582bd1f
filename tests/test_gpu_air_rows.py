"""GPU: AIR proofs over one row-committed tree (smi_dev_air_prove_rows / smi_air_verify_rows) against the oracle's
composition -- the root of the oracle's tree over the row leaves, the weights of the documented transcript, the codeword
of the polynomial route, Fri::prove continued from that transcript and the opening section restated record by record --
the verifier's verdicts with their reasons, and the wide-row leaf kernel through smi_dev_merkle_build_rows.
Every comparison is exact.  `pytest -m gpu`."""
import ctypes as C
import signal

import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import air_rows as ar
import transcript_compose as tc

pytestmark = pytest.mark.gpu

PATH = "air openings: authentication path does not verify"
LENGTH = "air openings: wrong length"
ROW = "air openings: malformed row"
PATH_RECORD = "air openings: malformed path"
COMPOSITION = "air openings: the composition of the opened rows is not the codeword value"
LOW_DEGREE = "last codeword does not correspond to polynomial of low enough degree"
COLINEARITY = "colinearity check failure"


@pytest.fixture(scope="module")
def engines():
    import stark_rs_amd as s
    es = {p: s.Engine(p, g, 0) for p, g in ac.PRIMES}
    yield es
    for e in es.values():
        e.close()


class Dev:
    """device buffers of one test, freed on exit"""

    def __init__(self, eng):
        self.eng, self.ptrs = eng, []

    def alloc(self, nbytes):
        self.ptrs.append(self.eng.dev_alloc(nbytes))
        return self.ptrs[-1]

    def upload(self, values):
        v = np.ascontiguousarray(np.asarray(values, dtype=np.uint64)).reshape(-1)
        d = self.alloc(4 * v.size)
        self.eng.dev_upload(v, d)
        return d

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.sync()
        for d in self.ptrs:
            self.eng.dev_free(d)


def prove(eng, air, cols, log_n, lb, t, rows=True, check=True):
    with Dev(eng) as dev:
        d_trace = dev.upload(np.array(cols, dtype=np.uint64))
        return eng.dev_air_prove(air, d_trace, len(cols), log_n, lb, t, check=check, timed=True, row_leaves=rows)


def verify(eng, air, proof, roots, W, log_n, lb, t, rows=True):
    return eng.air_verify(air, proof, roots, W, log_n, lb, t, row_leaves=rows)


def expected(o, air, cols, codeword, p, g, log_n, lb, t, E):
    """-> (root, transcript, FRI bytes, top indices, opening section) of the proof the definition prescribes"""
    N, B = 1 << (log_n + lb), 1 << lb
    W, K = air.n_cols, len(air.constraints)
    lde = ac.lde(o, cols, p, g, log_n, lb, 1, g)
    leaves = ar.row_leaves(o, lde)
    root = o.merkle_commit(leaves)
    prior, wts = ar.transcript(o, W, K, root)
    assert len(prior) == 32 + 8 * (W + K)
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    fri, top = tc.prove(o, o.fri_cfg(wN, g, N, E, t, p), codeword(wts), prior)
    return root, prior, fri, [int(x) for x in top], ar.openings_bytes(o, lde, top, N, B, K > 0, o.merkle_new(leaves))


def assert_proof(o, eng, air, cols, codeword, p, g, log_n, lb, t, want_accept=True):
    W, K = air.n_cols, len(air.constraints)
    _d, E = eng.air_plan(air, W, log_n, lb)
    res = prove(eng, air, cols, log_n, lb, t, check=want_accept)
    root, prior, fri, top, opened = expected(o, air, cols, codeword, p, g, log_n, lb, t, E)
    assert res["column_roots"].shape == (1, 32) and bytes(res["column_roots"][0]) == root
    assert res["top_indices"] == top
    got_fri, got_opened = ar.split(res["proof"], W, K, log_n + lb, t)
    assert got_fri == fri
    assert got_opened == opened
    assert res["proof"] == fri + opened
    assert len(res["proof"]) == len(fri) + ar.opening_len(W, K, log_n + lb, t)
    assert set(res["stage_ms"]) == {"lde", "commit", "compose", "fri", "open"}
    got = verify(eng, air, res["proof"], res["column_roots"], W, log_n, lb, t)
    if want_accept:
        assert got == (True, ""), got
        # the FRI part alone is Fri::prove's continuation of the transcript
        _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
        ok, _pv, why, used = eng.fri_verify(eng.fri_cfg(wN, g, 1 << (log_n + lb), E, t), res["proof"], transcript=prior, want_consumed=True)
        assert ok and used == len(fri), why
    return res, got


@pytest.mark.parametrize("name", ["empty", "fib", "mixer", "switch"])
@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_proof_bytes_equal_the_oracle_composition(engines, oracle, name, p, g):
    o, eng, log_n, lb, t = oracle, engines[p], 10, 3, 8
    if name == "switch":     # one periodic column (a selector of period 2), read at this row and the next
        air, cols = ap.make(name, 1 << log_n, p)
        codeword = lambda wts: ap.route(o, air, cols, wts, p, g, log_n, lb, 1, g)[0]
    else:
        air, cols = ac.make(name, 1 << log_n, p)
        codeword = lambda wts: ac.codeword_poly_route(o, air, cols, wts, p, g, log_n, lb, 1, g)[0]
    res, _ = assert_proof(o, eng, air, cols, codeword, p, g, log_n, lb, t)
    # against the column-tree proof of the same statement: shorter by exactly the W - 1 paths per opened position
    W, K, R = air.n_cols, len(air.constraints), 4 if air.constraints else 2
    col = prove(eng, air, cols, log_n, lb, t, rows=False)
    assert len(col["proof"]) - len(res["proof"]) == t * R * (W - 1) * (9 + 32 * (log_n + lb))
    assert len(col["proof"]) - len(res["proof"]) == ar.column_opening_len(W, K, log_n + lb, t) - ar.opening_len(W, K, log_n + lb, t)
    assert verify(eng, air, col["proof"], col["column_roots"], W, log_n, lb, t, rows=False) == (True, "")


# (W + K) mod 4 = 0, 1, 2, 3, 1: the transcript's 8 (W + K) bytes after the root leave every phase FRI can be seeded with;
# W = 5, 9, 64 go through the wide-row leaf kernel, W = 6 with a ragged last chunk of two
PHASES = [(5, 3), (9, 0), (64, 2), (5, 2), (6, 3)]


@pytest.mark.parametrize("W,K", PHASES)
@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_every_transcript_phase_with_a_satisfied_wide_air(engines, oracle, W, K, p, g):
    o, eng, log_n, lb, t = oracle, engines[p], 6, 3, 4
    air, cols = ar.wide(W, K, p, 1 << log_n)
    codeword = lambda wts: ac.codeword_poly_route(o, air, cols, wts, p, g, log_n, lb, 1, g)[0]
    assert_proof(o, eng, air, cols, codeword, p, g, log_n, lb, t)


@pytest.mark.parametrize("W,K", PHASES)
def test_every_transcript_phase_with_a_synthetic_air(engines, oracle, W, K):
    """air_compose.synthetic: K degree-2 constraints the random columns do not satisfy.  The codeword is still defined point
    by point (the Python mirror's compose_at over the oracle's extension), the proof bytes are still the definition's, and
    the verifier refuses them -- the folding does not end in a polynomial of low degree -- unless K = 0"""
    o = oracle
    p, g = ac.PRIMES[1]
    eng, log_n, lb, t = engines[p], 6, 3, 4
    N, B = 1 << (log_n + lb), 1 << lb
    air, cols = ac.synthetic(W, K, p, 1 << log_n)
    lde = ac.lde(o, cols, p, g, log_n, lb, 1, g)
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)

    def codeword(wts):
        return [air.compose_at(p, log_n, lb, 1, g, wN, i, [int(c[i]) for c in lde], [int(c[(i + B) % N]) for c in lde], wts) for i in range(N)]
    _, got = assert_proof(o, eng, air, cols, codeword, p, g, log_n, lb, t, want_accept=(K == 0))
    print("synthetic", W, K, got)
    assert got == ((True, "") if K == 0 else (False, LOW_DEGREE))


def test_rejections(engines, oracle):
    p, g = ac.PRIMES[0]
    eng, log_n, lb, t = engines[p], 10, 3, 8
    n, logN = 1 << log_n, log_n + lb
    mixer, cols = ac.make("mixer", n, p)
    wide4, _ = ac.make("wide4", n, p)
    W, K, R = 4, 3, 4
    res = prove(eng, mixer, cols, log_n, lb, t)
    proof, root = res["proof"], res["column_roots"]
    check = lambda air, pr, rt: verify(eng, air, pr, rt, W, log_n, lb, t)
    assert check(mixer, proof, root) == (True, "")
    fri, opened = ar.split(proof, W, K, logN, t)
    rec, prec = 9 + 8 * W, 9 + 32 * logN
    paths_at = len(fri) + t * R * rec

    def changed(at, to=None):
        b = bytearray(proof)
        b[at] = (b[at] ^ 1) if to is None else to
        return bytes(b)
    # one opened value: this row (record 0 of test 0), then a next row (record 2); the leaf is the hash of the row as it stands
    assert check(mixer, changed(len(fri) + 9), root) == (False, PATH)
    assert check(mixer, changed(len(fri) + 2 * rec + 9 + 8), root) == (False, PATH)
    # one path digest: the first byte of the first path, the last byte of the last
    assert check(mixer, changed(paths_at + 9), root) == (False, PATH)
    assert check(mixer, changed(len(proof) - 1), root) == (False, PATH)
    # a wrong root is another transcript: other challenges and other sampled indices than the prover's
    wrong = np.array(root).copy()
    wrong[0, 5] ^= 1
    assert check(mixer, proof, wrong) == (False, COLINEARITY)
    # truncated, extended, and cut inside the rows
    assert check(mixer, proof[:-1], root) == (False, LENGTH)
    assert check(mixer, proof + b"\x00", root) == (False, LENGTH)
    assert check(mixer, proof[:len(fri) + 2 * rec], root) == (False, LENGTH)
    # tags and widths
    assert check(mixer, changed(len(fri), 3), root) == (False, ROW)
    assert check(mixer, changed(len(fri) + 5 * rec, 0), root) == (False, ROW)
    assert check(mixer, changed(len(fri) + 1, W + 1), root) == (False, ROW)            # a row that claims five values
    assert check(mixer, changed(paths_at, 2), root) == (False, PATH_RECORD)
    assert check(mixer, changed(paths_at + 3 * prec + 1, logN - 1), root) == (False, PATH_RECORD)   # a path that claims one digest fewer
    # a non-canonical opened value: v + p in the 8 bytes of column 1 of the first row.  The leaf is hashed from the bytes as
    # they stand, so it is not the committed leaf and the path is what refuses it
    at = len(fri) + 9 + 8
    v = int.from_bytes(proof[at:at + 8], "little")
    b = bytearray(proof)
    b[at:at + 8] = (v + p).to_bytes(8, "little")
    assert check(mixer, bytes(b), root) == (False, PATH)
    # K = 4: a transcript 8 bytes longer than the prover's
    assert check(wide4, proof, root) == (False, COLINEARITY)
    # a trace with one cell changed: refused before proving, and the proof made without the check is refused by the verifier
    import stark_rs_amd as s
    bad = [list(c) for c in cols]
    bad[1][500] = (bad[1][500] + 1) % p
    want = mixer.first_violation(p, bad)
    with pytest.raises(s.StarkMiError, match=f"rows {want[1]} and {want[1] + 1}"):
        prove(eng, mixer, bad, log_n, lb, t)
    res_bad = prove(eng, mixer, bad, log_n, lb, t, check=False)
    got = check(mixer, res_bad["proof"], res_bad["column_roots"])
    print("proof from a violating trace:", got)
    assert got == (False, LOW_DEGREE)


def _mixer_like(n, p, a0=5, b_coef=3, last_c_col=2, c_next=2, a_last=None):
    """the mixer AIR of tests/air_compose.py with one thing changed: same W, same K, same transcript"""
    from stark_rs_amd.mirror import Air
    air = Air(4)
    air.transition({("next", 0): 1, (("cur", 0), ("cur", 1)): -1, ("cur", 2): -1})
    air.transition({("next", 1): 1, (("cur", 0, 2), ("cur", 2)): -1, ("cur", 1): -b_coef})
    air.transition({("next", c_next): 1, ("cur", 2): -1, (): -1})
    air.boundary(0, 0, a0).boundary(1, 0, 11).boundary(2, 0, 0).boundary(last_c_col, n - 1, (n - 1) % p).boundary(0, n - 1, a_last)
    return air


@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_verifier_recomputes_the_composition(engines, p, g):
    """An honest proof under another statement with the same W and K: transcript, FRI and every path are the prover's, so
    only the recomputation of the codeword from the opened rows can refuse it"""
    eng, log_n, lb, t = engines[p], 10, 3, 8
    n = 1 << log_n
    mixer, cols = ac.make("mixer", n, p)
    a_last = cols[0][-1]
    res = prove(eng, mixer, cols, log_n, lb, t)
    check = lambda air: verify(eng, air, res["proof"], res["column_roots"], 4, log_n, lb, t)
    assert check(mixer) == (True, "")
    assert check(_mixer_like(n, p, a_last=a_last)) == (True, "")                      # the same statement, rebuilt
    assert check(_mixer_like(n, p, a0=6, a_last=a_last)) == (False, COMPOSITION)      # one boundary value
    assert check(_mixer_like(n, p, b_coef=4, a_last=a_last)) == (False, COMPOSITION)  # one coefficient
    assert check(_mixer_like(n, p, c_next=3, a_last=a_last)) == (False, COMPOSITION)  # one next-row operand
    # one periodic value: the selector of the switch AIR
    switch, scols = ap.make("switch", n, p)
    sres = prove(eng, switch, scols, log_n, lb, t)
    scheck = lambda air: verify(eng, air, sres["proof"], sres["column_roots"], 2, log_n, lb, t)
    assert scheck(switch) == (True, "")
    other, _ = ap.make("switch", n, p)
    other.periodics[0] = [1, 2]
    assert scheck(other) == (False, COMPOSITION)


@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_the_two_variants_do_not_verify_as_each_other_at_width_one(engines, oracle, p, g):
    """W = 1: the leaf of a row is the leaf of its one element, so the column root and the row root are the same 32 bytes
    and the opening sections have the same layout; the transcripts (root | k ... against root | 0 | 1 + k ...) differ"""
    eng, log_n, lb, t = engines[p], 10, 3, 8
    air, cols = ap.make("mimc", 1 << log_n, p)
    rows, col = prove(eng, air, cols, log_n, lb, t), prove(eng, air, cols, log_n, lb, t, rows=False)
    assert bytes(rows["column_roots"][0]) == bytes(col["column_roots"][0])
    assert len(rows["proof"]) == len(col["proof"]) and rows["proof"] != col["proof"]
    assert verify(eng, air, rows["proof"], rows["column_roots"], 1, log_n, lb, t) == (True, "")
    assert verify(eng, air, col["proof"], col["column_roots"], 1, log_n, lb, t, rows=False) == (True, "")
    got = verify(eng, air, col["proof"], col["column_roots"], 1, log_n, lb, t)
    print("column proof under the row verifier:", got)
    assert got == (False, COLINEARITY)
    got = verify(eng, air, rows["proof"], rows["column_roots"], 1, log_n, lb, t, rows=False)
    print("row proof under the column verifier:", got)
    assert got == (False, COLINEARITY)


def test_the_column_tree_entry_points_still_refuse_row_leaves(engines):
    from stark_rs_amd import _lib
    import stark_rs_amd as s
    p, g = ac.PRIMES[0]
    eng, log_n, lb, t = engines[p], 10, 3, 8
    mixer, cols = ac.make("mixer", 1 << log_n, p)
    res = prove(eng, mixer, cols, log_n, lb, t)
    cfg, a = _lib.StarkCfg(log_n, lb, 4, 1, 1, g, t, 1), mixer.flatten(p)
    roots = np.zeros((4, 32), dtype=np.uint8)
    with pytest.raises(s.StarkMiError, match="row_leaves"):
        eng._ck(eng.L.smi_air_verify(eng.h, C.byref(cfg), C.byref(a), roots.ctypes.data, res["proof"], len(res["proof"]), C.byref(C.c_int())))
    with Dev(eng) as dev:
        d_trace = dev.upload(np.array(cols, dtype=np.uint64))
        proof, plen = C.c_void_p(), C.c_size_t()
        with pytest.raises(s.StarkMiError, match="row_leaves"):
            eng._ck(eng.L.smi_dev_air_prove(eng.h, C.byref(cfg), C.byref(a), C.c_void_p(d_trace), roots.ctypes.data, C.byref(proof), C.byref(plen),
                                            None, None))
    with pytest.raises(s.StarkMiError, match="column trees"):
        eng._ck(eng.L.smi_stark_verify(eng.h, C.byref(cfg), roots.ctypes.data, res["proof"], len(res["proof"]), C.byref(C.c_int())))


@pytest.mark.parametrize("W", [5, 6, 7, 8, 33, 64])
@pytest.mark.parametrize("logn", [0, 1, 7, 13])
@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_row_leaf_tree_of_wide_rows_equals_the_oracle(engines, oracle, W, logn, p, g):
    """smi_dev_merkle_build_rows over more than four columns: the wide-row leaf kernel, then the tree over its digests;
    every level against MerkleTree::new over the oracle's row hashes.  Row 0 is all p-1, row 1 all 0; the columns are a
    few words further apart than they are long"""
    o, eng = oracle, engines[p]
    n, stride = 1 << logn, (1 << logn) + 4
    rng = np.random.default_rng(100 * W + logn)
    cols = np.zeros((W, stride), dtype=np.uint64)
    cols[:, :n] = rng.integers(0, p, (W, n))
    cols[:, 0] = p - 1
    if n > 1:
        cols[:, 1] = 0
    with Dev(eng) as dev:
        d_cols, d_nodes = dev.upload(cols), dev.alloc((2 * n - 1) * 32)
        eng.dev_merkle_build_rows(d_cols, W, stride, n, d_nodes)
        got = eng.dev_download(d_nodes, (2 * n - 1) * 8).astype(np.uint32).view(np.uint8).reshape(-1, 32)
    want = o.merkle_new(o.row_hashes(np.ascontiguousarray(cols[:, :n])))
    assert np.array_equal(got, want)
    assert bytes(got[0]) == o.hash_from_field_elements([p - 1] * W)


class _TimeLimit:
    """a wall-clock limit of this one test's own (SIGALRM): generous, so that it only ends a hang"""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        def fire(*_):
            raise TimeoutError(f"the headline-shape case ran longer than {self.seconds} s")
        self.old = signal.signal(signal.SIGALRM, fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        signal.signal(signal.SIGALRM, self.old)


def test_headline_shape_once(engines, oracle):
    """W = 4, n = 2^22, blowup 8, t = 32 on 469762049: prove over the row tree, verify, the length formula, and 64 sampled
    leaves of the row tree (recomputed with smi_dev_merkle_build_rows over the device extension, whose root must be the
    proof's) against the oracle's row hash of the device extension's rows"""
    import torch
    o = oracle
    p, g = ac.PRIMES[1]
    eng, log_n, lb, W, t = engines[p], 22, 3, 4, 32
    n, N, logN = 1 << log_n, 1 << (log_n + lb), log_n + lb
    with _TimeLimit(900):
        air, cols = ac.make("mixer", n, p)
        dev = torch.device("cuda:0")
        trace = torch.from_numpy(np.array(cols, dtype=np.int64).astype(np.int32)).to(dev)
        torch.cuda.synchronize()
        res = eng.dev_air_prove(air, trace.data_ptr(), W, log_n, lb, t, timed=True, row_leaves=True)
        print("stage_ms", res["stage_ms"], "proof bytes", len(res["proof"]))
        assert verify(eng, air, res["proof"], res["column_roots"], W, log_n, lb, t) == (True, "")
        fri, opened = ar.split(res["proof"], W, 3, logN, t)
        assert len(opened) == t * 4 * (9 + 8 * W) + t * 4 * (9 + 32 * logN) == ar.opening_len(W, 3, logN, t)
        _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
        ok, _pv, why, used = eng.fri_verify(eng.fri_cfg(wN, g, N, 4, t), res["proof"],
                                            transcript=ar.transcript(o, W, 3, bytes(res["column_roots"][0]))[0], want_consumed=True)
        assert ok and used == len(fri), why
        lde = torch.empty((W, N), dtype=torch.int32, device=dev)
        nodes = torch.empty((2 * N, 32), dtype=torch.uint8, device=dev)
        eng.dev_lde(trace.data_ptr(), W, log_n, lb, lde.data_ptr())
        eng.dev_merkle_build_rows(lde.data_ptr(), W, N, N, nodes.data_ptr())
        eng.sync()
        assert bytes(nodes[2 * N - 2].cpu().numpy()) == bytes(res["column_roots"][0])
        rng = np.random.default_rng(4)
        idx = sorted({0, 1, N // 2 - 1, N // 2, N - 1} | {int(x) for x in rng.integers(0, N, 59)})
        ti = torch.tensor(idx, dtype=torch.int64, device=dev)
        rows, leaves = lde[:, ti].cpu().numpy().astype(np.uint32), nodes[ti].cpu().numpy()
        for k, i in enumerate(idx):
            assert bytes(leaves[k]) == o.hash_from_field_elements([int(v) for v in rows[:, k]]), i
        # the opened rows of the proof are rows of that extension
        a = res["top_indices"][0] % (N // 2)
        first = [int.from_bytes(opened[9 + 8 * c:17 + 8 * c], "little") for c in range(W)]
        assert first == [int(v) for v in lde[:, a].cpu().numpy().astype(np.uint32)]
