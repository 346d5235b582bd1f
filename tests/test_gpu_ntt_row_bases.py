"""GPU: the address forms of the NTT passes (csrc/ntt_core.h: uniform row / run base + one thread offset per tile), each at
the smallest shape where it is live, bit for bit against the oracle on both primes.  Every call's profile must name the
kernel the case is there for.  Inputs are the columns of tests/ntt_matrix.py (pseudo-random, alternating p - 1 / 0, all p - 1)."""
import os
import re

import numpy as np
import pytest

import ntt_matrix as nm

pytestmark = pytest.mark.gpu

GAP_IN, GAP_OUT, SENTINEL = 32, 64, nm.SENTINEL
_want = {}


def _leg(batch, inverse, offset, post=1, nin=(0, 0)):
    return {"batch": batch, "inverse": inverse, "offset": offset, "post": post, "nin": nin, "strided": False, "inplace": False}


def _expected(o, prime, L, leg, c):
    """one oracle run per (prime, size, transform, column), shared by the cases and never written to"""
    k = nm.key(prime, L, leg, c)
    if k not in _want:
        v = nm.oracle_column(o, prime, L, leg, c)
        v.setflags(write=False)
        _want[k] = v
    return _want[k]


@pytest.fixture(scope="module")
def engines():
    """one context per prime, and one per prime created with the launch-size threshold of the column-sharing rule lifted
    (SMI_NTT_SHARE_COLS=2 is read when a context is created, as in tests/ntt_matrix.py)"""
    import stark_rs_amd as s
    made = {}

    def get(prime, share2=False):
        if (prime, share2) not in made:
            old = os.environ.get("SMI_NTT_SHARE_COLS")
            if share2:
                os.environ["SMI_NTT_SHARE_COLS"] = "2"
            try:
                made[(prime, share2)] = s.Engine(nm.PRIMES[prime][0], nm.PRIMES[prime][1], 0)
            finally:
                if share2:
                    if old is None:
                        del os.environ["SMI_NTT_SHARE_COLS"]
                    else:
                        os.environ["SMI_NTT_SHARE_COLS"] = old
        return made[(prime, share2)]

    yield get
    for e in made.values():
        e.close()


def _run(eng, prime, L, leg, in_gap=0, out_gap=0):
    """-> (outputs (batch, n), output gaps, {ntt kernel name: launches})"""
    p = nm.PRIMES[prime][0]
    n, batch = 1 << L, leg["batch"]
    n_in = nm.n_in_of(leg, n)
    si, so = n + in_gap, n + out_gap
    host = np.full(batch * si, SENTINEL, dtype=np.uint64)
    for c in range(batch):
        host[c * si:c * si + n] = nm.column(p, L, c)
    d_in, d_out = eng.dev_alloc(batch * si * 4), eng.dev_alloc(batch * so * 4)
    try:
        eng.dev_upload(host, d_in)
        eng.dev_upload(np.full(batch * so, SENTINEL, dtype=np.uint64), d_out)
        eng.profile(True)
        try:
            eng.dev_ntt(d_in, d_out, L, n_in=n_in, batch=batch, in_stride=si, out_stride=so, inverse=leg["inverse"],
                        offset=leg["offset"], post_scale=leg["post"])
            kernels = {k: v["launches"] for k, v in eng.profile_read().items() if k.startswith("ntt_")}
        finally:
            eng.profile(False)
        got = eng.dev_download(d_out, batch * so).reshape(batch, so)
    finally:
        eng.dev_free(d_in)
        eng.dev_free(d_out)
    return got[:, :n], got[:, n:], kernels


def _check(o, eng, prime, L, leg, names, **gaps):
    got, gap, kernels = _run(eng, prime, L, leg, **gaps)
    for pat in names:
        assert any(re.fullmatch(pat, k) for k in kernels), (pat, kernels)
    assert (gap == SENTINEL).all(), "a store left its column"
    for c in range(leg["batch"]):
        assert np.array_equal(got[c], _expected(o, prime, L, leg, c)), (prime, L, c, kernels)


@pytest.mark.parametrize("prime", ["ref", "p2"])
def test_two_pass_plan_with_column_strides_that_are_not_the_size(oracle, engines, prime):
    first, last = r"ntt_pass_kernel<7,\d,first>", r"ntt_pass_kernel<6,\d,last>"
    _check(oracle, engines(prime), prime, 13, _leg(3, False, 5), [first, last], in_gap=GAP_IN, out_gap=GAP_OUT)
    _check(oracle, engines(prime), prime, 13, _leg(3, True, 3, 5), [first, r"ntt_pass(_cols)?_kernel<6,\d,last>"], in_gap=GAP_IN, out_gap=GAP_OUT)


@pytest.mark.parametrize("prime", ["ref", "p2"])
def test_three_pass_plan_deferred_twiddles_and_a_short_last_column_group(oracle, engines, prime):
    # 2^21 x 5: column groups of 4 + 1; the first pass leaves its twiddles (NTT_TW_SKIP) to the column-sharing middle pass
    _check(oracle, engines(prime, share2=True), prime, 21, _leg(5, False, 5),
           [r"ntt_pass_kernel<7,\d,first>", r"ntt_pass_cols_kernel<7,5,mid>", r"ntt_pass_kernel<7,\d,last>"])


@pytest.mark.parametrize("prime,L", [("ref", 23), ("p2", 23), ("p2", 25)])   # 2^25 is beyond the first modulus' two-adicity
@pytest.mark.parametrize("ragged", [0, -3])
def test_zero_padded_first_pass_and_512_point_last_pass(oracle, engines, prime, L, ragged):
    mid = "ntt_pass_kernel<%d,%d,mid>" % (L - 17, 6 if L - 17 <= 7 else 5)
    _check(oracle, engines(prime), prime, L, _leg(1, False, 5, nin=(3, ragged)),
           [r"ntt_pass_kernel<8,6,first>", re.escape(mid), r"ntt_pass_kernel<9,5,last>"])


@pytest.mark.parametrize("prime", ["ref", "p2"])
def test_inverse_with_output_scale_in_the_column_sharing_last_pass(oracle, engines, prime):
    _check(oracle, engines(prime), prime, 22, _leg(4, True, 3, 5),
           [r"ntt_pass_kernel<8,\d,first>", r"ntt_pass_cols_kernel<7,\d,mid>", r"ntt_pass_cols_kernel<7,\d,last>"])


@pytest.mark.parametrize("prime", ["ref", "p2"])
def test_extension_end_to_end(oracle, engines, prime):
    o, eng = oracle, engines(prime)
    p, g, _ = nm.PRIMES[prime]
    logn, lb, W = 13, 3, 3
    n, N = 1 << logn, 1 << (logn + lb)
    cols = np.stack([nm.column(p, logn, c) for c in (0, 2, 5)])   # pseudo-random, alternating, all p - 1
    d_cols, d_out = eng.dev_alloc(W * n * 4), eng.dev_alloc(W * N * 4)
    try:
        eng.dev_upload(cols.reshape(-1), d_cols)
        eng.profile(True)
        try:
            eng.dev_lde(d_cols, W, logn, lb, d_out, 1, g)
            kernels = {k for k in eng.profile_read() if k.startswith("ntt_")}
        finally:
            eng.profile(False)
        got = eng.dev_download(d_out, W * N).reshape(W, N)
    finally:
        eng.dev_free(d_cols)
        eng.dev_free(d_out)
    for role in ("first", "last"):
        assert any(re.fullmatch(r"ntt_pass(_cols)?_kernel<\d+,\d,%s>" % role, k) for k in kernels), kernels
    w, Wn = o.ff_prim_nth_root_g(n, p, g), o.ff_prim_nth_root_g(N, p, g)
    for c in range(W):
        assert np.array_equal(got[c], o.fast_coset_ntt(o.fast_intt(cols[c], w, 1, p), N, Wn, g, p)), (prime, c)
