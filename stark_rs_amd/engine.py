"""Engine: one smi_ctx (one GPU, one prime field) with numpy- and pointer-level calls.

Host-buffer methods take/return numpy uint64 arrays (the reference's wire width); dev_*
methods take raw device pointers (ints, e.g. torch.Tensor.data_ptr()) of u32 residues and
only enqueue work on the context's stream.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FriCfg, StarkMiError, check, vp

P_REF, G_REF = 998244353, 3          # reference field (src/ff.rs:191-197)
P2, G2 = 469762049, 3              # 7*2^26+1: domains above 2^23; p < 2^30 keeps 4p < 2^32

_default = {}


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


class Engine:
    def __init__(self, p=P_REF, g=G_REF, device=0):
        self.L = _lib.lib()
        h = vp()
        st = self.L.smi_ctx_create(p, g, device, C.byref(h))
        if st != 0:
            raise StarkMiError(st, f"smi_ctx_create(p={p}, g={g}, device={device}): {_lib.status_string(st)} "
                                   "(the HIP path is the only path: no CPU fallback)")
        self.h = h
        self.p, self.g, self.device = p, g, device

    def close(self):
        if getattr(self, "h", None):
            self.L.smi_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st):
        check(st, self.h)

    # ---- context
    def set_stream(self, stream_ptr):
        self._ck(self.L.smi_ctx_set_stream(self.h, vp(stream_ptr)))

    def sync(self):
        self._ck(self.L.smi_ctx_sync(self.h))

    def profile(self, enable=True):
        """Bracket every hot-path kernel launch with HIP events on the context's stream."""
        self._ck(self.L.smi_ctx_profile(self.h, 1 if enable else 0))

    def profile_only(self, name_part=None):
        """Bracket only launches whose kernel name contains name_part (None: all): one kernel timed inside an otherwise
        undisturbed loop."""
        self._ck(self.L.smi_ctx_profile_only(self.h, name_part.encode() if name_part else None))

    def lde_two_pass(self, enable=True):
        """extensions of 2^20..2^22 rows in two passes over the outputs (csrc/lde_core.h) instead of three"""
        self._ck(self.L.smi_ctx_lde_two_pass(self.h, 1 if enable else 0))

    def copy_probe(self, enable=True):
        """Measurement aid: NTT passes launch their copy-only twins (same access pattern, no
        arithmetic); results are meaningless while it is on."""
        self._ck(self.L.smi_ctx_copy_probe(self.h, 1 if enable else 0))

    def mix_probe(self, mixes=512):
        """mix_state evaluations per second of the bare permutation (two hashes per lane, no memory traffic): the
        integer-VALU ceiling the Merkle kernels are reported against."""
        out = C.c_double()
        self._ck(self.L.smi_ctx_mix_probe(self.h, mixes, C.byref(out)))
        return float(out.value)

    def profile_read(self):
        """-> {kernel name: {"launches", "total_ms", "alg_bytes", "alg_mixes"}} since the last read (synchronises)."""
        arr = (_lib.KernelTime * 64)()
        n = C.c_size_t()
        self._ck(self.L.smi_ctx_profile_read(self.h, arr, 64, C.byref(n)))
        return {arr[i].name.decode(): {"launches": int(arr[i].launches), "total_ms": float(arr[i].total_ms),
                                       "alg_bytes": float(arr[i].alg_bytes), "alg_mixes": float(arr[i].alg_mixes)}
                for i in range(n.value)}

    @property
    def two_adicity(self):
        return int(self.L.smi_ctx_two_adicity(self.h))

    # ---- scalars
    def prim_nth_root(self, n):
        out = C.c_uint64()
        self._ck(self.L.smi_prim_nth_root(self.h, n, C.byref(out)))
        return out.value

    def inv(self, x):
        out = C.c_uint64()
        self._ck(self.L.smi_ff_inv(self.h, x, C.byref(out)))
        return out.value

    def exp(self, b, e):
        out = C.c_uint64()
        self._ck(self.L.smi_ff_exp(self.h, b, e, C.byref(out)))
        return out.value

    def mul(self, a, b):
        out = C.c_uint64()
        self._ck(self.L.smi_ff_mul(self.h, a, b, C.byref(out)))
        return out.value

    # ---- univariate (host buffers)
    def intt(self, values, offset=1):
        v = _u64(values)
        n = len(v)
        if n == 0 or n & (n - 1):
            raise StarkMiError(-3, "n must be a power of two")
        out = np.empty(n, dtype=np.uint64)
        self._ck(self.L.smi_intt(self.h, v.ctypes.data, out.ctypes.data, n.bit_length() - 1, offset))
        return out

    def coset_ntt(self, coeffs, log_N, offset=1):
        c = _u64(coeffs)
        out = np.empty(1 << log_N, dtype=np.uint64)
        self._ck(self.L.smi_coset_ntt(self.h, c.ctypes.data, len(c), out.ctypes.data, log_N, offset))
        return out

    def poly_scale(self, coeffs, factor):
        c = _u64(coeffs)
        out = np.empty(len(c), dtype=np.uint64)
        self._ck(self.L.smi_poly_scale(self.h, c.ctypes.data, len(c), factor, out.ctypes.data))
        return out

    def poly_mul(self, a, b):
        """Polynomial::mul (mul.rs:6-29) by NTT."""
        a, b = _u64(a), _u64(b)
        out = np.empty(max(len(a) + len(b), 1), dtype=np.uint64)
        n = C.c_size_t()
        self._ck(self.L.smi_poly_mul(self.h, a.ctypes.data, len(a), b.ctypes.data, len(b), out.ctypes.data, C.byref(n)))
        return out[:n.value].copy()

    def poly_div(self, a, b):
        """Polynomial::div (div.rs:6-42) -> (quotient, remainder) by NTT products (power-series inverse)."""
        a, b = _u64(a), _u64(b)
        q = np.empty(max(len(a), 1), dtype=np.uint64)
        r = np.empty(max(len(a), len(b), 1), dtype=np.uint64)
        nq, nr = C.c_size_t(), C.c_size_t()
        self._ck(self.L.smi_poly_div(self.h, a.ctypes.data, len(a), b.ctypes.data, len(b), q.ctypes.data, C.byref(nq),
                                     r.ctypes.data, C.byref(nr)))
        return q[:nq.value].copy(), r[:nr.value].copy()

    def poly_zerofier(self, domain):
        """Polynomial::zerofier (mod.rs:77-96): prod (x - d) over any points, n + 1 coefficients (subproduct tree)."""
        d = _u64(domain)
        out = np.empty(len(d) + 1, dtype=np.uint64)
        self._ck(self.L.smi_poly_zerofier(self.h, d.ctypes.data, len(d), out.ctypes.data))
        return out

    def poly_eval_points(self, coeffs, points):
        """Polynomial::eval_domain (eval.rs:16-21) at any points, in order (subproduct tree)."""
        c, x = _u64(coeffs), _u64(points)
        out = np.empty(len(x), dtype=np.uint64)
        self._ck(self.L.smi_poly_eval_points(self.h, c.ctypes.data, len(c), x.ctypes.data, len(x), out.ctypes.data))
        return out

    def poly_interpolate_points(self, domain, values):
        """Polynomial::interpolate_domain (interpolate.rs:6-44) on any distinct points: n coefficients."""
        d, v = _u64(domain), _u64(values)
        if len(d) != len(v):
            raise StarkMiError(-14, "assertion failed: domain.len() == values.len()")
        out = np.empty(len(d), dtype=np.uint64)
        self._ck(self.L.smi_poly_interpolate_points(self.h, d.ctypes.data, v.ctypes.data, len(d), out.ctypes.data))
        return out

    def domain_is_geometric(self, domain):
        d = _u64(domain)
        off = C.c_uint64()
        st = self.L.smi_domain_is_geometric(self.h, d.ctypes.data, len(d), C.byref(off))
        return (st == 0), off.value

    def lde(self, cols, log_blowup, trace_offset=1, lde_offset=None, out=None):
        cols = _u64(cols)
        n_cols, n = cols.shape
        if out is None:
            out = np.empty((n_cols, n << log_blowup), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.shape == (n_cols, n << log_blowup) and out.flags.c_contiguous
        lde_offset = self.g if lde_offset is None else lde_offset
        self._ck(self.L.smi_lde(self.h, cols.ctypes.data, n_cols, n.bit_length() - 1, log_blowup, trace_offset, lde_offset,
                                out.ctypes.data))
        return out

    def trace_pack(self, rows_i128_bytes, n_rows, n_cols):
        out = np.empty((n_cols, n_rows), dtype=np.uint64)
        buf = np.frombuffer(rows_i128_bytes, dtype=np.uint8)
        self._ck(self.L.smi_trace_pack(self.h, buf.ctypes.data, n_rows, n_cols, out.ctypes.data))
        return out

    # ---- hash / merkle (host buffers)
    def hash_leaves(self, elems):
        e = _u64(elems)
        out = np.empty((len(e), 32), dtype=np.uint8)
        self._ck(self.L.smi_hash_leaves(self.h, e.ctypes.data, len(e), out.ctypes.data))
        return out

    def hash_combine_pairs(self, digests):
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 64)
        out = np.empty((len(d), 32), dtype=np.uint8)
        self._ck(self.L.smi_hash_combine_pairs(self.h, d.ctypes.data, len(d), out.ctypes.data))
        return out

    def hash_bytes(self, msg: bytes) -> bytes:
        out = (C.c_uint8 * 32)()
        self._ck(self.L.smi_hash_bytes(self.h, msg, len(msg), out))
        return bytes(out)

    def hash_bytes_batch(self, msgs):
        """Hash::from_bytes of equally long messages -> list of 32-byte digests (one device call)."""
        msgs = list(msgs)
        if not msgs:
            return []
        ln = len(msgs[0])
        assert all(len(m) == ln for m in msgs)
        out = np.empty((len(msgs), 32), dtype=np.uint8)
        self._ck(self.L.smi_hash_bytes_batch(self.h, b"".join(msgs), len(msgs), ln, out.ctypes.data))
        return [bytes(r) for r in out]

    def merkle_commit(self, leaves) -> bytes:
        l = np.ascontiguousarray(leaves, dtype=np.uint8).reshape(-1, 32)
        out = (C.c_uint8 * 32)()
        self._ck(self.L.smi_merkle_commit(self.h, l.ctypes.data, len(l), out))
        return bytes(out)

    def merkle_verify_batch(self, leaves, indices, paths, root):
        """MerkleTree::verify for k triples sharing one depth and root -> bool array."""
        l = np.ascontiguousarray(leaves, dtype=np.uint8).reshape(-1, 32)
        k = len(l)
        pth = np.ascontiguousarray(paths, dtype=np.uint8).reshape(k, -1, 32) if k else np.zeros((0, 0, 32), np.uint8)
        idx = _u64(indices)
        ok = np.zeros(max(k, 1), dtype=np.uint8)
        rt = np.frombuffer(bytes(root), dtype=np.uint8).copy()
        self._ck(self.L.smi_merkle_verify_batch(self.h, l.ctypes.data, idx.ctypes.data, pth.ctypes.data, k, pth.shape[1],
                                                rt.ctypes.data, ok.ctypes.data))
        return ok[:k].astype(bool)

    def merkle_new(self, leaves):
        l = np.ascontiguousarray(leaves, dtype=np.uint8).reshape(-1, 32)
        t = vp()
        self._ck(self.L.smi_merkle_new(self.h, l.ctypes.data, len(l), C.byref(t)))
        return DeviceTree(self, t)

    def merkle_from_codeword(self, codeword):
        c = _u64(codeword)
        t = vp()
        self._ck(self.L.smi_merkle_from_codeword(self.h, c.ctypes.data, len(c), C.byref(t)))
        return DeviceTree(self, t)

    # ---- fri (host buffers)
    def fri_cfg(self, omega, offset, domain_length, expansion_factor, num_colinearity_tests):
        cfg = FriCfg(omega, offset, domain_length, expansion_factor, num_colinearity_tests)
        self._ck(self.L.smi_fri_check(self.h, C.byref(cfg)))
        return cfg

    def fri_num_rounds(self, cfg):
        r = C.c_uint64()
        self._ck(self.L.smi_fri_num_rounds(C.byref(cfg), C.byref(r)))
        return r.value

    def fri_fold(self, codeword, alpha, offset, omega):
        c = _u64(codeword)
        out = np.empty(len(c) // 2, dtype=np.uint64)
        self._ck(self.L.smi_fri_fold(self.h, c.ctypes.data, len(c), alpha, offset, omega, out.ctypes.data))
        return out

    # `transcript`: the bytes the caller's FiatShamir holds before the call (src/fri.rs:105-110, 250-255, 313-318); the
    # empty default is a fresh FiatShamir and calls the entry points without a transcript.  The roots are not absorbed
    # here: the caller appends them to its transcript, as the reference leaves it.
    def _commit(self, cfg, codeword, transcript, run):
        c = _u64(codeword)
        R = max(self.fri_num_rounds(cfg), 1)
        roots = np.zeros((R, 32), dtype=np.uint8)
        alphas = np.zeros(R, dtype=np.uint64)
        last = np.zeros(len(c), dtype=np.uint64)
        ll = C.c_size_t()
        tail = (roots.ctypes.data, alphas.ctypes.data, last.ctypes.data, C.byref(ll), run)
        if transcript:
            t = bytes(transcript)
            self._ck(self.L.smi_fri_commit_fs(self.h, C.byref(cfg), t, len(t), c.ctypes.data, len(c), *tail))
        else:
            self._ck(self.L.smi_fri_commit(self.h, C.byref(cfg), c.ctypes.data, len(c), *tail))
        return roots, [int(a) for a in alphas[:R - 1]], last[:ll.value].copy()

    def fri_commit(self, cfg, codeword, transcript=b""):
        return self._commit(cfg, codeword, transcript, None)

    def fri_commit_run(self, cfg, codeword, transcript=b""):
        """Fri::commit keeping every round's codeword and tree on the device -> (roots, alphas, FriRun)."""
        run = vp()
        roots, alphas, _ = self._commit(cfg, codeword, transcript, C.byref(run))
        return roots, alphas, FriRun(self, run)

    def fri_prove(self, cfg, codeword, transcript=b""):
        """-> (ProofStream::serialize bytes, top-level indices) -- Fri::prove, src/fri.rs:250-311; with a transcript,
        the objects it pushes after the caller's."""
        c = _u64(codeword)
        proof, plen = vp(), C.c_size_t()
        top = np.zeros(max(cfg.num_colinearity_tests, 1), dtype=np.uint64)
        if transcript:
            t = bytes(transcript)
            self._ck(self.L.smi_fri_prove_fs(self.h, C.byref(cfg), t, len(t), c.ctypes.data, len(c), C.byref(proof), C.byref(plen),
                                             top.ctypes.data))
        else:
            self._ck(self.L.smi_fri_prove(self.h, C.byref(cfg), c.ctypes.data, len(c), C.byref(proof), C.byref(plen),
                                          top.ctypes.data))
        b = C.string_at(proof, plen.value)
        self.L.smi_free(proof)
        return b, [int(v) for v in top[:cfg.num_colinearity_tests]]

    # ---- device-resident calls (pointers are ints)
    def fri_verify(self, cfg, proof: bytes, transcript=b"", want_consumed=False):
        """Fri::verify (src/fri.rs:313-504) -> (accept, [(index, value)], reason); a reference panic raises.
        want_consumed: a fourth item, the bytes of the objects it popped (0 on rejection)."""
        t = int(cfg.num_colinearity_tests)
        pi, pv = np.zeros(2 * t + 2, dtype=np.uint64), np.zeros(2 * t + 2, dtype=np.uint64)
        acc, n, used = C.c_int(), C.c_size_t(), C.c_size_t()
        if transcript or want_consumed:
            tr = bytes(transcript)
            self._ck(self.L.smi_fri_verify_fs(self.h, C.byref(cfg), tr, len(tr), proof, len(proof), C.byref(acc), pi.ctypes.data,
                                              pv.ctypes.data, C.byref(n), C.byref(used)))
        else:
            self._ck(self.L.smi_fri_verify(self.h, C.byref(cfg), proof, len(proof), C.byref(acc), pi.ctypes.data, pv.ctypes.data,
                                           C.byref(n)))
        why = "" if acc.value else self.L.smi_last_error(self.h).decode()
        out = (bool(acc.value), [(int(pi[i]), int(pv[i])) for i in range(n.value)], why)
        return out + (used.value,) if want_consumed else out

    def stark_verify(self, proof: bytes, column_roots, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset=1,
                     lde_offset=None, open_columns=False):
        """verifier of dev_stark_prove / MultiGpu.stark_prove -> (accept, reason)"""
        cfg = _lib.StarkCfg(log_n, log_blowup, n_cols, 0, trace_offset, self.g if lde_offset is None else lde_offset,
                            num_colinearity_tests, 1 if open_columns else 0)
        roots = np.ascontiguousarray(np.frombuffer(b"".join(bytes(r) for r in column_roots), dtype=np.uint8))
        acc = C.c_int()
        self._ck(self.L.smi_stark_verify(self.h, C.byref(cfg), roots.ctypes.data, proof, len(proof), C.byref(acc)))
        return bool(acc.value), ("" if acc.value else self.L.smi_last_error(self.h).decode())

    def dev_alloc(self, nbytes):
        d = vp()
        self._ck(self.L.smi_dev_alloc(self.h, nbytes, C.byref(d)))
        return d.value

    def dev_free(self, ptr):
        self._ck(self.L.smi_dev_free(self.h, vp(ptr)))

    def dev_upload(self, values, d_ptr, reduce=False):
        v = _u64(values)
        self._ck(self.L.smi_dev_upload_u64(self.h, v.ctypes.data, v.size, vp(d_ptr), 1 if reduce else 0))

    def dev_download(self, d_ptr, n):
        out = np.empty(n, dtype=np.uint64)
        self._ck(self.L.smi_dev_download_u64(self.h, vp(d_ptr), n, out.ctypes.data))
        return out

    def dev_ntt(self, d_in, d_out, log_n, n_in=None, batch=1, in_stride=None, out_stride=None, inverse=False, offset=1,
                post_scale=1):
        n = 1 << log_n
        n_in = n if n_in is None else n_in
        self._ck(self.L.smi_dev_ntt(self.h, vp(d_in), vp(d_out), log_n, n_in, batch, n_in if in_stride is None else in_stride,
                                    n if out_stride is None else out_stride, 1 if inverse else 0, offset, post_scale))

    def dev_lde(self, d_cols, n_cols, log_n, log_blowup, d_out, trace_offset=1, lde_offset=None):
        lde_offset = self.g if lde_offset is None else lde_offset
        self._ck(self.L.smi_dev_lde(self.h, vp(d_cols), n_cols, log_n, log_blowup, trace_offset, lde_offset, vp(d_out)))

    def dev_hash_leaves(self, d_elems, n, d_digests):
        self._ck(self.L.smi_dev_hash_leaves(self.h, vp(d_elems), n, vp(d_digests)))

    def dev_merkle_build(self, d_elems, n, d_nodes):
        self._ck(self.L.smi_dev_merkle_build(self.h, vp(d_elems), n, vp(d_nodes)))

    def dev_merkle_build_rows(self, d_cols, n_cols, col_stride, n, d_nodes):
        """One tree whose leaf i is Hash::from_field_elements(row i) over n_cols columns."""
        self._ck(self.L.smi_dev_merkle_build_rows(self.h, vp(d_cols), n_cols, col_stride, n, vp(d_nodes)))

    def dev_merkle_build_cosets(self, d_cols, n_cols, col_stride, n, d_nodes):
        """One tree of n / 4 leaves: leaf i is Hash::from_field_elements of the 4 * n_cols values (column c at index
        i + j * n / 4 is value 4 c + j) of the coset {i, i + n/4, i + n/2, i + 3n/4}; n_cols is 1 .. 64."""
        self._ck(self.L.smi_dev_merkle_build_cosets(self.h, vp(d_cols), n_cols, col_stride, n, vp(d_nodes)))

    def dev_hash_bytes(self, d_msg, length, d_out32):
        self._ck(self.L.smi_dev_hash_bytes(self.h, vp(d_msg), length, vp(d_out32)))

    def dev_merkle_from_digests(self, n, d_nodes):
        self._ck(self.L.smi_dev_merkle_from_digests(self.h, n, vp(d_nodes)))

    def dev_fri_fold(self, d_in, length, d_alpha, offset, omega, d_out):
        self._ck(self.L.smi_dev_fri_fold(self.h, vp(d_in), length, vp(d_alpha), offset, omega, vp(d_out)))

    def dev_fri_fold_ext(self, d_in, length, stride, d_alpha, offset, omega, d_out, out_stride=None):
        """smi_dev_fri_fold_ext: the fold of a codeword over the quartic extension -- four coordinate columns `stride`
        apart in, four columns out_stride (default length / 2) apart out; d_alpha = four unreduced u64 on the device"""
        out_stride = length // 2 if out_stride is None else out_stride
        self._ck(self.L.smi_dev_fri_fold_ext(self.h, vp(d_in), length, stride, vp(d_alpha), offset, omega, vp(d_out), out_stride))

    def dev_fri_fold4_ext(self, d_in, length, stride, d_alpha, offset, omega, d_out, out_stride=None):
        """smi_dev_fri_fold4_ext: the fold by 4 of a codeword over the quartic extension in one launch -- what
        dev_fri_fold_ext gives under alpha over (offset, omega, length) and then under alpha^2 over (offset^2, omega^2,
        length / 2); four columns out_stride (default length / 4) apart out"""
        out_stride = length // 4 if out_stride is None else out_stride
        self._ck(self.L.smi_dev_fri_fold4_ext(self.h, vp(d_in), length, stride, vp(d_alpha), offset, omega, vp(d_out), out_stride))

    @staticmethod
    def fri_fold4_layout(cfg):
        """smi_fri_fold4_layout (host only) -> (folds, last codeword length, proof bytes) of extension FRI at folding factor 4"""
        return fri_fold4_layout(cfg)

    def dev_fri_fold_shard(self, d_lo, d_hi, count, index0, full_len, d_alpha, offset, omega, d_out):
        self._ck(self.L.smi_dev_fri_fold_shard(self.h, vp(d_lo), vp(d_hi), count, index0, full_len, vp(d_alpha), offset, omega,
                                               vp(d_out)))

    def dev_fri_prove(self, cfg, d_codeword, length, transcript=b""):
        proof, plen = vp(), C.c_size_t()
        top = np.zeros(max(cfg.num_colinearity_tests, 1), dtype=np.uint64)
        if transcript:   # host bytes (the transcript is never on the device)
            t = bytes(transcript)
            self._ck(self.L.smi_dev_fri_prove_fs(self.h, C.byref(cfg), t, len(t), vp(d_codeword), length, C.byref(proof),
                                                 C.byref(plen), top.ctypes.data, None))
        else:
            self._ck(self.L.smi_dev_fri_prove(self.h, C.byref(cfg), vp(d_codeword), length, C.byref(proof), C.byref(plen),
                                              top.ctypes.data, None))
        b = C.string_at(proof, plen.value)
        self.L.smi_free(proof)
        return b, [int(v) for v in top[:cfg.num_colinearity_tests]]

    # ---- proof-of-work grinding (include/stark_mi.h, "Grinding")
    def grind(self, transcript, bits, max_tries=0):
        """smi_dev_grind -> the smallest nonce whose hash with the transcript (host bytes) has `bits` low zero bits in its
        check word; max_tries = 0: the default cap 2^(bits+6).  StarkMiError -55 when no nonce below the cap is valid."""
        t = bytes(transcript)
        out = C.c_uint64()
        self._ck(self.L.smi_dev_grind(self.h, t if t else None, len(t), bits, max_tries, C.byref(out)))
        return int(out.value)

    @staticmethod
    def grind_check(transcript, nonce, bits):
        """smi_grind_check (host only) -> pow_ok(transcript, nonce, bits)"""
        return grind_check(transcript, nonce, bits)

    def dev_fri_prove_ext(self, cfg, d_codeword, length, stride=None, transcript=b"", grind_bits=None, folding=2):
        """smi_dev_fri_prove_ext: Fri::prove over the quartic extension on four device coordinate columns `stride`
        (default length) apart, continuing the caller's transcript (host bytes) -> (proof bytes, top-level indices).
        grind_bits (None: no grinding, today's stream): smi_dev_fri_prove_ext_pow -> (proof bytes, top-level indices, nonce).
        folding=4: smi_dev_fri_prove_ext_fold4 -> (proof bytes, top-level indices, nonce); grind_bits None means 0 there"""
        _check_folding(folding)
        proof, plen = vp(), C.c_size_t()
        top = np.zeros(max(cfg.num_colinearity_tests, 1), dtype=np.uint64)
        t = bytes(transcript)
        args = (self.h, C.byref(cfg), t if t else None, len(t), vp(d_codeword), length, length if stride is None else stride, C.byref(proof),
                C.byref(plen), top.ctypes.data)
        nonce = C.c_uint64()
        if folding == 4:
            self._ck(self.L.smi_dev_fri_prove_ext_fold4(*args, grind_bits or 0, C.byref(nonce)))
        elif grind_bits is None:
            self._ck(self.L.smi_dev_fri_prove_ext(*args))
        else:
            self._ck(self.L.smi_dev_fri_prove_ext_pow(*args, grind_bits, C.byref(nonce)))
        b = C.string_at(proof, plen.value)
        self.L.smi_free(proof)
        top = [int(v) for v in top[:cfg.num_colinearity_tests]]
        return (b, top) if grind_bits is None and folding == 2 else (b, top, int(nonce.value))

    def fri_verify_ext(self, cfg, proof: bytes, transcript=b"", grind_bits=None, folding=2):
        """smi_fri_verify_ext -> (accept, polynomial_values [(index, [c0, c1, c2, c3])], bytes consumed, reason).
        grind_bits (None: a proof without grinding): smi_fri_verify_ext_pow, the least difficulty demanded.
        folding=4: smi_fri_verify_ext_fold4 (grind_bits None means 0); polynomial_values holds the layer-0 cosets, four
        entries per test"""
        _check_folding(folding)
        t = bytes(transcript)
        n = (4 if folding == 4 else 2) * max(cfg.num_colinearity_tests, 1)
        idx, val = np.zeros(n, dtype=np.uint64), np.zeros(4 * n, dtype=np.uint64)
        acc, npv, used = C.c_int(), C.c_size_t(), C.c_size_t()
        args = (self.h, C.byref(cfg), t if t else None, len(t), proof, len(proof), C.byref(acc), idx.ctypes.data, val.ctypes.data, C.byref(npv),
                C.byref(used))
        if folding == 4:
            self._ck(self.L.smi_fri_verify_ext_fold4(*args, grind_bits or 0))
        elif grind_bits is None:
            self._ck(self.L.smi_fri_verify_ext(*args))
        else:
            self._ck(self.L.smi_fri_verify_ext_pow(*args, grind_bits))
        pv = [(int(idx[i]), [int(v) for v in val[4 * i:4 * i + 4]]) for i in range(npv.value)]
        return bool(acc.value), pv, used.value, ("" if acc.value else self.L.smi_last_error(self.h).decode())

    def dev_combine_columns(self, d_cols, n_cols, length, stride, d_weights, d_out):
        self._ck(self.L.smi_dev_combine_columns(self.h, vp(d_cols), n_cols, length, stride, vp(d_weights), vp(d_out)))

    def dev_stark_prove(self, d_trace_cols, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset=1,
                        lde_offset=None, timed=False, row_leaves=False, open_columns=False):
        """Build-defined prove.  -> dict(column_roots, proof, top_indices[, stage_ms]).
        row_leaves: commit to the extended trace with one tree over its rows instead of one per column."""
        cfg = _lib.StarkCfg(log_n, log_blowup, n_cols, 1 if row_leaves else 0, trace_offset,
                            self.g if lde_offset is None else lde_offset, num_colinearity_tests, 1 if open_columns else 0)
        roots = np.zeros((1 if row_leaves else n_cols, 32), dtype=np.uint8)
        proof, plen = vp(), C.c_size_t()
        top = np.zeros(max(num_colinearity_tests, 1), dtype=np.uint64)
        stage = (C.c_double * 4)()
        self._ck(self.L.smi_dev_stark_prove(self.h, C.byref(cfg), vp(d_trace_cols), roots.ctypes.data, C.byref(proof),
                                            C.byref(plen), top.ctypes.data, stage if timed else None))
        b = C.string_at(proof, plen.value)
        self.L.smi_free(proof)
        out = {"column_roots": roots, "proof": b, "top_indices": [int(v) for v in top[:num_colinearity_tests]]}
        if timed:
            out["stage_ms"] = dict(zip(("lde", "commit", "combine", "fri"), [float(x) for x in stage]))
        return out

    # ---- AIR constraints (include/stark_mi.h, "AIR"); `air` is a mirror.Air or a flattened _lib.Air
    def _air(self, air):
        return air if isinstance(air, _lib.Air) else air.flatten(self.p)

    @staticmethod
    def _window(a):
        """the transition window S of a flattened AIR (include/stark_mi.h, "AIR: transition windows"); 0 reads as 2"""
        return a.window or 2

    def _check_window(self, a, who, deep, deep_args, zk):
        """an AIR with a window above two rows is proven and verified by the plain DEEP variants only"""
        if self._window(a) > 2 and (not deep or deep_args or (zk is not None and zk is not False)):
            raise ValueError(f"{who}: an AIR with a transition window of {self._window(a)} rows takes deep=True (row or coset leaves) only: "
                             "no argument list, no zero knowledge, none of the provers that open next rows")

    def _stark_cfg(self, n_cols, log_n, log_blowup, num_colinearity_tests=0, trace_offset=1, lde_offset=None, row_leaves=False):
        return _lib.StarkCfg(log_n, log_blowup, n_cols, 1 if row_leaves else 0, trace_offset, self.g if lde_offset is None else lde_offset,
                             num_colinearity_tests, 1)

    def air_plan(self, air, n_cols, log_n, log_blowup, trace_offset=1, lde_offset=None):
        """smi_air_plan -> (degree d, FRI expansion factor E); raises with the limit that was broken"""
        a = self._air(air)
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, 0, trace_offset, lde_offset)
        if self._xargs(a) is not None:   # smi_air_plan_xargs: a permutation with a selector counts 3
            return air_plan_xargs(self.p, a, a.xargs, cfg)
        if self._args(a) is not None:   # smi_air_plan_args: d = max(d_air, 2 with a permutation, 3 with a lookup)
            return air_plan_args(self.p, a, a.args, cfg)
        if self._perm(a) is not None:   # smi_air_plan_perm: d = max(d_air, 2)
            return air_plan_perm(self.p, a, a.perm, cfg)
        if self._lookup(a) is not None:   # smi_air_plan_lookup: d = max(d_air, 3)
            return air_plan_lookup(self.p, a, a.lookup, cfg)
        return air_plan(self.p, a, cfg)

    @staticmethod
    def _perm(air):
        """the _lib.AirPerm a flattened AIR carries (mirror.Air.permutation), or None"""
        return getattr(air, "perm", None)

    @staticmethod
    def _lookup(air):
        """the _lib.AirLookup a flattened AIR carries (mirror.Air.lookup), or None"""
        return getattr(air, "lookup", None)

    @staticmethod
    def _args(air):
        """the _lib.AirArgs a flattened AIR carries (mirror.Air.add_permutation / add_lookup), or None"""
        return getattr(air, "args", None)

    @staticmethod
    def _xargs(air):
        """the _lib.AirXArgs a flattened AIR carries (a list with a selector or a periodic member), or None"""
        return getattr(air, "xargs", None)

    def dev_args_multiplicities(self, air, a, d_trace_cols, n_cols, log_n, d_mult):
        """the multiplicities of lookup argument a of air's list into d_mult (n device words): smi_dev_xargs_multiplicities for
        a list with selectors or periodic members -- only selected rows are inserted and counted --, smi_dev_lookup_multiplicities
        otherwise.  StarkMiError naming the smallest (selected) row whose tuple is in no (selected) table row."""
        f = self._air(air)
        if self._xargs(f) is not None:
            self._ck_perm(self.L.smi_dev_xargs_multiplicities(self.h, C.byref(f), C.byref(f.xargs), a, vp(d_trace_cols), n_cols, log_n, vp(d_mult)))
            return
        if self._args(f) is None:
            raise ValueError("dev_args_multiplicities: the AIR has no argument list (mirror.Air.add_permutation / add_lookup)")
        if not 0 <= a < f.args.count or f.args.arg[a].kind != 1:
            raise ValueError(f"dev_args_multiplicities: argument {a} is not a lookup of the list")
        g = f.args.arg[a]
        one = _lib.AirLookup(g.width, g.mult_col, g.a_col, g.b_col)
        self._ck_perm(self.L.smi_dev_lookup_multiplicities(self.h, C.byref(one), vp(d_trace_cols), n_cols, log_n, vp(d_mult)))

    def _args_of(self, air, who):
        a = self._air(air)
        if self._args(a) is None and self._xargs(a) is None:
            raise ValueError(f"{who}: the AIR has no argument list (mirror.Air.add_permutation / add_lookup)")
        return a

    def dev_args_columns(self, air, d_trace_cols, n_cols, log_n, challenges, d_c, c_stride=None):
        """smi_dev_args_columns: the A columns of air's argument list under the 8 unreduced challenges (alpha, gamma) into 4 A
        coordinate columns c_stride (default n) apart -> closes, a list of A bools.  StarkMiError "no inverse: ... argument a:
        ... row r" when a denominator is zero."""
        a = self._args_of(air, "dev_args_columns")
        ch = (C.c_uint64 * 8)(*[int(c) for c in challenges])
        closes = C.c_uint32()
        if self._xargs(a) is not None:   # selectors or periodic members: smi_dev_xargs_columns
            self._ck_perm(self.L.smi_dev_xargs_columns(self.h, C.byref(a), C.byref(a.xargs), vp(d_trace_cols), n_cols, log_n, ch, vp(d_c),
                                                       (1 << log_n) if c_stride is None else c_stride, C.byref(closes)))
            return [bool(closes.value >> i & 1) for i in range(a.xargs.count)]
        self._ck_perm(self.L.smi_dev_args_columns(self.h, C.byref(a.args), vp(d_trace_cols), n_cols, log_n, ch, vp(d_c),
                                                  (1 << log_n) if c_stride is None else c_stride, C.byref(closes)))
        return [bool(closes.value >> i & 1) for i in range(a.args.count)]

    def dev_air_compose_args(self, air, d_lde, d_c_lde, n_cols, log_n, log_blowup, challenges, d_weights, d_out, stride=None, c_stride=None,
                             out_stride=None, trace_offset=1, lde_offset=None):
        """smi_dev_air_compose_args: smi_dev_air_compose_ext under the first 4 (W + K) of the 4 (W + K + 2 A) device weights plus
        the 2 A auxiliary quotients of the 4 A extended coordinate columns d_c_lde, in one streaming launch"""
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, 0, trace_offset, lde_offset)
        a = self._args_of(air, "dev_air_compose_args")
        N = 1 << (log_n + log_blowup)
        ch = (C.c_uint64 * 8)(*[int(c) for c in challenges])
        if self._xargs(a) is not None:   # selectors or periodic members: smi_dev_air_compose_xargs
            self._ck(self.L.smi_dev_air_compose_xargs(self.h, C.byref(cfg), C.byref(a), C.byref(a.xargs), vp(d_lde), N if stride is None else stride,
                                                      vp(d_c_lde), N if c_stride is None else c_stride, ch, vp(d_weights), vp(d_out),
                                                      N if out_stride is None else out_stride))
            return
        self._ck(self.L.smi_dev_air_compose_args(self.h, C.byref(cfg), C.byref(a), C.byref(a.args), vp(d_lde), N if stride is None else stride,
                                                 vp(d_c_lde), N if c_stride is None else c_stride, ch, vp(d_weights), vp(d_out),
                                                 N if out_stride is None else out_stride))

    def _ck_perm(self, st):
        if st in (-1, -56):   # SMI_ERR_NO_INVERSE, SMI_ERR_LOOKUP_MISSING: the sentence names the row
            raise StarkMiError(st, f"{_lib.status_string(st)}: {self.L.smi_last_error(self.h).decode()}")
        self._ck(st)

    def dev_perm_column(self, air, d_trace_cols, n_cols, log_n, challenges, d_z, z_stride=None):
        """smi_dev_perm_column: the column z of air's permutation under the 8 unreduced challenges (alpha, gamma) into four
        coordinate columns z_stride (default n) apart -> closes (bool).  StarkMiError "no inverse: ... row r" when some
        f_R(r) is zero."""
        a = self._air(air)
        if self._perm(a) is None:
            raise ValueError("dev_perm_column: the AIR has no permutation (mirror.Air.permutation)")
        ch = (C.c_uint64 * 8)(*[int(c) for c in challenges])
        closes = C.c_int()
        self._ck_perm(self.L.smi_dev_perm_column(self.h, C.byref(a.perm), vp(d_trace_cols), n_cols, log_n, ch, vp(d_z),
                                                 (1 << log_n) if z_stride is None else z_stride, C.byref(closes)))
        return bool(closes.value)

    def dev_air_compose_perm(self, air, d_lde, d_z_lde, n_cols, log_n, log_blowup, challenges, d_weights, d_out, stride=None, z_stride=None,
                             out_stride=None, trace_offset=1, lde_offset=None):
        """smi_dev_air_compose_perm: smi_dev_air_compose_ext under the first 4 (W + K) of the 4 (W + K + 2) device weights plus
        the two auxiliary quotients of the extended column d_z_lde"""
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, 0, trace_offset, lde_offset)
        a = self._air(air)
        if self._perm(a) is None:
            raise ValueError("dev_air_compose_perm: the AIR has no permutation (mirror.Air.permutation)")
        N = 1 << (log_n + log_blowup)
        ch = (C.c_uint64 * 8)(*[int(c) for c in challenges])
        self._ck(self.L.smi_dev_air_compose_perm(self.h, C.byref(cfg), C.byref(a), C.byref(a.perm), vp(d_lde), N if stride is None else stride,
                                                 vp(d_z_lde), N if z_stride is None else z_stride, ch, vp(d_weights), vp(d_out),
                                                 N if out_stride is None else out_stride))

    def _lookup_of(self, air, who):
        a = self._air(air)
        if self._lookup(a) is None:
            raise ValueError(f"{who}: the AIR has no lookup (mirror.Air.lookup)")
        return a

    def dev_lookup_multiplicities(self, air, d_trace_cols, n_cols, log_n, d_mult):
        """smi_dev_lookup_multiplicities: the multiplicities of air's lookup over the device trace into d_mult (n u32, zeroed by
        the call; pass the address of the trace's mult_col to fill the trace in place).  StarkMiError -56 naming the smallest
        row whose tuple is in no table row."""
        a = self._lookup_of(air, "dev_lookup_multiplicities")
        self._ck_perm(self.L.smi_dev_lookup_multiplicities(self.h, C.byref(a.lookup), vp(d_trace_cols), n_cols, log_n, vp(d_mult)))

    def dev_lookup_column(self, air, d_trace_cols, n_cols, log_n, challenges, d_s, s_stride=None):
        """smi_dev_lookup_column: the column s of air's lookup under the 8 unreduced challenges (alpha, gamma) into four
        coordinate columns s_stride (default n) apart -> closes (bool).  StarkMiError "no inverse: ... row r" when some f_L(r)
        or f_T(r) is zero."""
        a = self._lookup_of(air, "dev_lookup_column")
        ch = (C.c_uint64 * 8)(*[int(c) for c in challenges])
        closes = C.c_int()
        self._ck_perm(self.L.smi_dev_lookup_column(self.h, C.byref(a.lookup), vp(d_trace_cols), n_cols, log_n, ch, vp(d_s),
                                                   (1 << log_n) if s_stride is None else s_stride, C.byref(closes)))
        return bool(closes.value)

    def dev_air_compose_lookup(self, air, d_lde, d_s_lde, n_cols, log_n, log_blowup, challenges, d_weights, d_out, stride=None, s_stride=None,
                               out_stride=None, trace_offset=1, lde_offset=None):
        """smi_dev_air_compose_lookup: smi_dev_air_compose_ext under the first 4 (W + K) of the 4 (W + K + 2) device weights plus
        the two auxiliary quotients of the extended column d_s_lde"""
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, 0, trace_offset, lde_offset)
        a = self._lookup_of(air, "dev_air_compose_lookup")
        N = 1 << (log_n + log_blowup)
        ch = (C.c_uint64 * 8)(*[int(c) for c in challenges])
        self._ck(self.L.smi_dev_air_compose_lookup(self.h, C.byref(cfg), C.byref(a), C.byref(a.lookup), vp(d_lde), N if stride is None else stride,
                                                   vp(d_s_lde), N if s_stride is None else s_stride, ch, vp(d_weights), vp(d_out),
                                                   N if out_stride is None else out_stride))

    def dev_air_compose(self, air, d_lde, n_cols, log_n, log_blowup, d_weights, d_out, stride=None, trace_offset=1, lde_offset=None):
        """the composition codeword of n_cols extended device columns under n_cols + K unreduced device weights"""
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, 0, trace_offset, lde_offset)
        a = self._air(air)
        stride = (1 << (log_n + log_blowup)) if stride is None else stride
        self._ck(self.L.smi_dev_air_compose(self.h, C.byref(cfg), C.byref(a), vp(d_lde), stride, vp(d_weights), vp(d_out)))

    def dev_air_compose_ext(self, air, d_lde, n_cols, log_n, log_blowup, d_weights, d_out, stride=None, out_stride=None, trace_offset=1,
                            lde_offset=None):
        """smi_dev_air_compose_ext: the composition under 4 (n_cols + K) unreduced device weights (coordinate e of weight
        j at 4 j + e) into four coordinate columns out_stride (default N) apart"""
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, 0, trace_offset, lde_offset)
        a = self._air(air)
        N = 1 << (log_n + log_blowup)
        self._ck(self.L.smi_dev_air_compose_ext(self.h, C.byref(cfg), C.byref(a), vp(d_lde), N if stride is None else stride, vp(d_weights),
                                                vp(d_out), N if out_stride is None else out_stride))

    def dev_air_check(self, air, d_trace_cols, n_cols, log_n):
        """-> (ok, constraint, row, sentence): the first violation of the AIR on the trace itself; constraint is the
        boundary point's position, or n_boundary + k for transition constraint k"""
        a = self._air(air)
        ok, con, row = C.c_int(), C.c_uint32(), C.c_uint64()
        self._ck(self.L.smi_dev_air_check(self.h, C.byref(a), n_cols, log_n, vp(d_trace_cols), C.byref(ok), C.byref(con), C.byref(row)))
        if ok.value:
            return True, None, None, ""
        return False, con.value, row.value, self.L.smi_last_error(self.h).decode()

    # ---- out-of-domain sampling (include/stark_mi.h, "Out-of-domain sampling")
    def _check_deep(self, a, row_leaves, ext, folding, fill_multiplicities):
        if any(f(a) is not None for f in (self._xargs, self._args, self._lookup, self._perm)) or fill_multiplicities:
            raise ValueError("deep=True takes a plain AIR: no permutation, lookup or argument list")
        if folding != 2:
            raise ValueError("deep=True folds by 2 only (folding=4 is not supported)")
        if not (row_leaves and ext):
            raise ValueError("deep=True runs over the row-committed extension proof: pass row_leaves=True, ext=True")

    def air_plan_deep(self, air, n_cols, log_n, log_blowup, trace_offset=1, lde_offset=None, num_colinearity_tests=None):
        """smi_air_plan_deep -> (degree d, segments D); with num_colinearity_tests also the proof length of
        smi_air_deep_layout: (d, D, bytes).  Host only; raises with the limit that was broken."""
        a = self._air(air)
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests or 0, trace_offset, lde_offset, True)
        return air_plan_deep(self.p, a, cfg, num_colinearity_tests is not None)

    def dev_poly_eval_ext(self, d_coeffs, n_cols, n_coeffs, points, stride=None):
        """smi_dev_poly_eval_ext: n_cols device columns of n_coeffs base-field coefficients, stride (default n_coeffs) apart,
        at one or two points of F_q (four canonical coordinates each) -> [[[c0..c3] per point] per column]"""
        pts = [int(v) for pt in points for v in pt]
        if len(pts) not in (4, 8):
            raise ValueError("dev_poly_eval_ext: one or two points of four coordinates")
        P = len(pts) // 4
        arr = (C.c_uint64 * len(pts))(*pts)
        out = (C.c_uint64 * (4 * n_cols * P))()
        self._ck(self.L.smi_dev_poly_eval_ext(self.h, vp(d_coeffs), n_cols, n_coeffs, n_coeffs if stride is None else stride, arr, P, out))
        return [[[int(out[4 * (c * P + k) + e]) for e in range(4)] for k in range(P)] for c in range(n_cols)]

    def dev_poly_eval_ext_shifts(self, d_coeffs, n_cols, n_coeffs, z, w, n_shifts, stride=None):
        """smi_dev_poly_eval_ext_shifts: the columns of dev_poly_eval_ext at z, z w, .. z w^(n_shifts - 1) (z: four canonical
        coordinates, w: a canonical base-field element, n_shifts in 1 .. 4) -> [[[c0..c3] per shift] per column]"""
        if len(z) != 4:
            raise ValueError("dev_poly_eval_ext_shifts: z has four coordinates")
        za = (C.c_uint64 * 4)(*[int(v) for v in z])
        out = (C.c_uint64 * (4 * n_cols * max(int(n_shifts), 1)))()
        self._ck(self.L.smi_dev_poly_eval_ext_shifts(self.h, vp(d_coeffs), n_cols, n_coeffs, n_coeffs if stride is None else stride, za, int(w), n_shifts, out))
        S = n_shifts
        return [[[int(out[4 * (c * S + k) + e]) for e in range(4)] for k in range(S)] for c in range(n_cols)]

    def dev_deep_compose(self, d_lde, d_seg, n_cols, n_segments, log_n, log_blowup, z, ood, challenges, d_out, stride=None, seg_stride=None,
                         out_stride=None, lde_offset=None):
        """smi_dev_deep_compose: the DEEP codeword of n_cols extended columns and 4 n_segments segment columns under z (four
        canonical coordinates), the record's 4 (2 W + D) values and as many unreduced challenges, into four coordinate columns"""
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, 0, 1, lde_offset, True)
        N, cnt = 1 << (log_n + log_blowup), 4 * (2 * n_cols + n_segments)
        if len(z) != 4 or len(ood) != cnt or len(challenges) != cnt:
            raise ValueError("dev_deep_compose: z has 4 coordinates, ood and challenges 4 (2 W + D) values")
        za, oa, ca = (C.c_uint64 * 4)(*[int(v) for v in z]), (C.c_uint64 * cnt)(*[int(v) for v in ood]), (C.c_uint64 * cnt)(*[int(v) for v in challenges])
        self._ck(self.L.smi_dev_deep_compose(self.h, C.byref(cfg), n_segments, vp(d_lde), N if stride is None else stride, vp(d_seg),
                                             N if seg_stride is None else seg_stride, za, oa, ca, vp(d_out), N if out_stride is None else out_stride))

    def dev_deep_compose_window(self, window, d_lde, d_seg, n_cols, n_segments, log_n, log_blowup, z, ood, challenges, d_out, stride=None,
                                seg_stride=None, out_stride=None, lde_offset=None):
        """smi_dev_deep_compose_window: dev_deep_compose under a window of S = window rows; ood and challenges hold 4 (S W + D)
        values, u_{s,c} s-major, then s_j"""
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, 0, 1, lde_offset, True)
        N, cnt = 1 << (log_n + log_blowup), 4 * (int(window) * n_cols + n_segments)
        if len(z) != 4 or len(ood) != cnt or len(challenges) != cnt:
            raise ValueError("dev_deep_compose_window: z has 4 coordinates, ood and challenges 4 (S W + D) values")
        za, oa, ca = (C.c_uint64 * 4)(*[int(v) for v in z]), (C.c_uint64 * cnt)(*[int(v) for v in ood]), (C.c_uint64 * cnt)(*[int(v) for v in challenges])
        self._ck(self.L.smi_dev_deep_compose_window(self.h, C.byref(cfg), window, n_segments, vp(d_lde), N if stride is None else stride, vp(d_seg),
                                                    N if seg_stride is None else seg_stride, za, oa, ca, vp(d_out), N if out_stride is None else out_stride))

    def _dev_air_prove_deep(self, a, d_trace_cols, n_cols, log_n, log_blowup, t, trace_offset, lde_offset, timed, check, row_leaves, ext, grind_bits,
                            fill_multiplicities, folding, coset_leaves=False):
        self._check_deep(a, row_leaves, ext, folding, fill_multiplicities)
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, t, trace_offset, lde_offset, True)
        _d, D = air_plan_deep(self.p, a, cfg)
        if check:
            ok, _con, _row, why = self.dev_air_check(a, d_trace_cols, n_cols, log_n)
            if not ok:
                raise StarkMiError(-50, why)
        roots = np.zeros((2, 32), dtype=np.uint8)
        S = self._window(a)
        ood = np.zeros(4 * (S * n_cols + D), dtype=np.uint64)
        proof, plen = vp(), C.c_size_t()
        top = np.zeros(max(t, 1), dtype=np.uint64)
        stage = (C.c_double * 7)()
        prove = self.L.smi_dev_air_prove_deep_fold4 if coset_leaves else self.L.smi_dev_air_prove_deep
        self._ck(prove(self.h, C.byref(cfg), C.byref(a), vp(d_trace_cols), roots.ctypes.data, ood.ctypes.data, C.byref(proof),
                       C.byref(plen), top.ctypes.data, stage if timed else None, 0 if grind_bits is None else grind_bits))
        b = C.string_at(proof, plen.value)
        self.L.smi_free(proof)
        out = {"column_roots": roots, "proof": b, "top_indices": [int(v) for v in top[:t]],
               "ood": [[int(v) for v in ood[4 * i:4 * i + 4]] for i in range(S * n_cols + D)]}
        if timed:
            out["stage_ms"] = dict(zip(("lde", "commit", "compose", "segments", "ood", "fri", "open"), [float(x) for x in stage]))
        return out

    # ---- out-of-domain sampling with an argument list (include/stark_mi.h, "Out-of-domain sampling with an argument list")
    def _check_deep_args(self, a, row_leaves, ext, folding, deep):
        if deep:
            raise ValueError("deep_args=True and deep=True exclude each other: deep=True takes a plain AIR")
        if self._xargs(a) is None and self._args(a) is None:
            raise ValueError("deep_args=True takes an AIR with an argument list (mirror.Air.add_permutation / add_lookup)")
        if folding != 2:
            raise ValueError("deep_args=True folds by 2 only (folding=4 is not supported)")
        if not (row_leaves and ext):
            raise ValueError("deep_args=True runs over the row-committed extension proof: pass row_leaves=True, ext=True")
        return xargs_of(a)

    def air_plan_deep_args(self, air, n_cols, log_n, log_blowup, trace_offset=1, lde_offset=None, num_colinearity_tests=None):
        """smi_air_plan_deep_xargs for air's argument list -> (degree d, segments D); with num_colinearity_tests also the proof
        length of smi_air_deep_xargs_layout: (d, D, bytes).  Host only; raises with the limit that was broken."""
        a = self._args_of(air, "air_plan_deep_args")
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests or 0, trace_offset, lde_offset, True)
        return air_plan_deep_args(self.p, a, xargs_of(a), cfg, num_colinearity_tests is not None)

    def dev_deep_compose_args(self, d_lde, d_c_lde, d_seg, n_cols, n_args, n_segments, log_n, log_blowup, z, ood, challenges, d_out, stride=None,
                              c_stride=None, seg_stride=None, out_stride=None, lde_offset=None):
        """smi_dev_deep_compose_args: the DEEP codeword of n_cols extended columns, the 4 n_args extended coordinate columns of
        the auxiliary columns and 4 n_segments segment columns under z, the record's 4 (2 W + 2 A + D) values and as many
        unreduced challenges, into four coordinate columns"""
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, 0, 1, lde_offset, True)
        N, cnt = 1 << (log_n + log_blowup), 4 * (2 * n_cols + 2 * n_args + n_segments)
        if len(z) != 4 or len(ood) != cnt or len(challenges) != cnt:
            raise ValueError("dev_deep_compose_args: z has 4 coordinates, ood and challenges 4 (2 W + 2 A + D) values")
        za, oa, ca = (C.c_uint64 * 4)(*[int(v) for v in z]), (C.c_uint64 * cnt)(*[int(v) for v in ood]), (C.c_uint64 * cnt)(*[int(v) for v in challenges])
        self._ck(self.L.smi_dev_deep_compose_args(self.h, C.byref(cfg), n_args, n_segments, vp(d_lde), N if stride is None else stride, vp(d_c_lde),
                                                  N if c_stride is None else c_stride, vp(d_seg), N if seg_stride is None else seg_stride, za, oa, ca,
                                                  vp(d_out), N if out_stride is None else out_stride))

    def _dev_air_prove_deep_args(self, a, d_trace_cols, n_cols, log_n, log_blowup, t, trace_offset, lde_offset, timed, check, row_leaves, ext, grind_bits,
                                 fill_multiplicities, folding, deep, coset_leaves=False):
        xa = self._check_deep_args(a, row_leaves, ext, folding, deep)
        A = xa.count
        lookups = [i for i in range(A) if xa.arg[i].kind & 0xff == 1]
        if fill_multiplicities and not lookups:
            raise ValueError("dev_air_prove(fill_multiplicities=True): the argument list has no lookup")
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, t, trace_offset, lde_offset, True)
        _d, D = air_plan_deep_args(self.p, a, xa, cfg)
        if fill_multiplicities:
            for i in lookups:
                self._ck_perm(self.L.smi_dev_xargs_multiplicities(self.h, C.byref(a), C.byref(xa), i, vp(d_trace_cols), n_cols, log_n,
                                                                  vp(vp(d_trace_cols).value + 4 * (xa.arg[i].mult_col << log_n))))
        if check:
            ok, _con, _row, why = self.dev_air_check(a, d_trace_cols, n_cols, log_n)
            if not ok:
                raise StarkMiError(-50, why)
        roots = np.zeros((3, 32), dtype=np.uint8)
        cnt = 2 * n_cols + 2 * A + D
        ood = np.zeros(4 * cnt, dtype=np.uint64)
        proof, plen, mask = vp(), C.c_size_t(), C.c_uint32()
        top = np.zeros(max(t, 1), dtype=np.uint64)
        stage = (C.c_double * 8)()
        prove = self.L.smi_dev_air_prove_deep_xargs_fold4 if coset_leaves else self.L.smi_dev_air_prove_deep_xargs
        self._ck_perm(prove(self.h, C.byref(cfg), C.byref(a), C.byref(xa), vp(d_trace_cols), roots.ctypes.data, ood.ctypes.data, C.byref(proof),
                            C.byref(plen), top.ctypes.data, stage if timed else None, 0 if grind_bits is None else grind_bits, C.byref(mask)))
        b = C.string_at(proof, plen.value)
        self.L.smi_free(proof)
        closes = [bool(mask.value >> i & 1) for i in range(A)]
        if check and not all(closes):
            raise StarkMiError(-50, f"air_prove_deep_xargs: the arguments {[i for i, c in enumerate(closes) if not c]} do not close")
        out = {"column_roots": roots, "proof": b, "top_indices": [int(v) for v in top[:t]], "closes": closes,
               "ood": [[int(v) for v in ood[4 * i:4 * i + 4]] for i in range(cnt)]}
        if timed:
            out["stage_ms"] = dict(zip(("lde", "commit", "args", "compose", "segments", "ood", "fri", "open"), [float(x) for x in stage]))
        return out

    # ---- out-of-domain sampling over coset leaves (include/stark_mi.h, "Out-of-domain sampling over coset leaves")
    @staticmethod
    def _check_coset_leaves(row_leaves, ext, deep, deep_args):
        if not (row_leaves and ext):
            raise ValueError("coset_leaves=True runs over the row-committed extension proof: pass row_leaves=True, ext=True")
        if deep and deep_args:
            raise ValueError("coset_leaves=True takes exactly one of deep=True and deep_args=True, not both")
        if not (deep or deep_args):
            raise ValueError("coset_leaves=True commits the groups of a DEEP proof: pass deep=True (a plain AIR) or deep_args=True (an argument list)")

    def air_deep_fold4_layout(self, air, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset=1, lde_offset=None):
        """smi_air_deep_fold4_layout -> (folds, proof bytes) of dev_air_prove(deep=True, coset_leaves=True).  Host only."""
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
        return air_deep_fold4_layout(self.p, self._air(air), cfg)

    def air_deep_args_fold4_layout(self, air, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset=1, lde_offset=None):
        """smi_air_deep_xargs_fold4_layout for air's argument list -> (folds, proof bytes) of dev_air_prove(deep_args=True,
        coset_leaves=True).  Host only."""
        a = self._args_of(air, "air_deep_args_fold4_layout")
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
        return air_deep_args_fold4_layout(self.p, a, xargs_of(a), cfg)

    # ---- zero-knowledge building blocks (include/stark_mi.h, "Zero-knowledge DEEP proofs")
    def air_plan_deep_zk(self, air, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset=1, lde_offset=None):
        """smi_air_plan_deep_zk -> (degree d of the derived AIR, segments D', k_t, k_s).  Host only; raises with the limit that
        was broken."""
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
        return air_plan_deep_zk(self.p, self._air(air), cfg)

    def dev_random_fill(self, seed, stream_id, d_out, count):
        """smi_dev_random_fill: count residues of stream stream_id under the 32-byte seed into device memory at d_out"""
        seed = bytes(seed)
        if len(seed) != 32:
            raise ValueError("dev_random_fill: the seed is 32 bytes")
        self._ck(self.L.smi_dev_random_fill(self.h, seed, int(stream_id), vp(d_out), count))

    def dev_zk_segments(self, d_h, h_len, log_n, k_s, n_segments, d_rho, d_out, h_stride=None, out_stride=None):
        """smi_dev_zk_segments: the 4 n_segments masked segment columns (n = 2^log_n coefficients each, out_stride apart, default
        n) of the four coefficient columns of H at d_h (h_len coefficients each, h_stride apart, default h_len) under the
        4 (n_segments - 1) k_s random words at d_rho"""
        self._ck(self.L.smi_dev_zk_segments(self.h, vp(d_h), h_len if h_stride is None else h_stride, h_len, log_n, k_s, n_segments, vp(d_rho),
                                            vp(d_out), (1 << log_n) if out_stride is None else out_stride))

    def air_deep_zk_layout(self, air, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset=1, lde_offset=None):
        """smi_air_deep_zk_layout -> (folds, proof bytes) of dev_air_prove(deep=True, coset_leaves=True, zk=seed).  Host only."""
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
        return air_deep_zk_layout(self.p, self._air(air), cfg)

    def _dev_air_prove_deep_zk(self, air, a, d_trace_cols, n_cols, log_n, log_blowup, t, trace_offset, lde_offset, timed, check, row_leaves, ext, grind_bits,
                               fill_multiplicities, folding, zk):
        import os
        self._check_deep(a, row_leaves, ext, folding, fill_multiplicities)
        seed = os.urandom(32) if zk is True else bytes(zk)
        if len(seed) != 32:
            raise ValueError("zk: the seed is 32 bytes (or True for os.urandom(32))")
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, t, trace_offset, lde_offset, True)
        _d, Dp, _kt, _ks = air_plan_deep_zk(self.p, a, cfg)
        if check:
            if isinstance(air, _lib.Air):
                raise ValueError("zk with check=True derives the AIR to check from a mirror.Air; pass one, or check=False")
            derived = air.zk_derived(self.p, log_n, t, trace_offset, self.prim_nth_root(1 << log_n))
            ok, _con, _row, why = self.dev_air_check(derived.flatten(self.p), d_trace_cols, n_cols, log_n)
            if not ok:
                raise StarkMiError(-50, why)
        roots = np.zeros((2, 32), dtype=np.uint8)
        ood = np.zeros(4 * (2 * n_cols + Dp), dtype=np.uint64)
        proof, plen = vp(), C.c_size_t()
        top = np.zeros(max(t, 1), dtype=np.uint64)
        stage = (C.c_double * 9)()
        self._ck(self.L.smi_dev_air_prove_deep_zk(self.h, C.byref(cfg), C.byref(a), vp(d_trace_cols), seed, roots.ctypes.data, ood.ctypes.data,
                                                  C.byref(proof), C.byref(plen), top.ctypes.data, stage if timed else None,
                                                  0 if grind_bits is None else grind_bits))
        b = C.string_at(proof, plen.value)
        self.L.smi_free(proof)
        out = {"column_roots": roots, "proof": b, "top_indices": [int(v) for v in top[:t]], "seed": seed,
               "ood": [[int(v) for v in ood[4 * i:4 * i + 4]] for i in range(2 * n_cols + Dp)]}
        if timed:
            out["stage_ms"] = dict(zip(("random", "lde", "commit", "compose", "segments", "ood", "mask", "fri", "open"), [float(x) for x in stage]))
        return out

    # ---- zero-knowledge DEEP proofs with an argument list (include/stark_mi.h, "Zero-knowledge DEEP proofs with an argument list")
    def air_plan_deep_zk_args(self, air, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset=1, lde_offset=None):
        """smi_air_plan_deep_zk_xargs for air's argument list -> (d, D', k_t = 8 t + 16, k_s).  Host only."""
        a = self._args_of(air, "air_plan_deep_zk_args")
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
        return air_plan_deep_zk_args(self.p, a, xargs_of(a), cfg)

    def air_deep_zk_args_layout(self, air, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset=1, lde_offset=None):
        """smi_air_deep_zk_xargs_layout -> (folds, proof bytes) of dev_air_prove(deep_args=True, coset_leaves=True, zk=seed).  Host only."""
        a = self._args_of(air, "air_deep_zk_args_layout")
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
        return air_deep_zk_args_layout(self.p, a, xargs_of(a), cfg)

    def dev_xargs_multiplicities_rows(self, air, a, d_trace_cols, n_cols, log_n, rows, d_mult):
        """smi_dev_xargs_multiplicities_rows: the multiplicities of lookup argument a over the rows < rows into d_mult (n words)"""
        f = self._args_of(air, "dev_xargs_multiplicities_rows")
        self._ck_perm(self.L.smi_dev_xargs_multiplicities_rows(self.h, C.byref(f), C.byref(xargs_of(f)), a, vp(d_trace_cols), n_cols, log_n, rows,
                                                               vp(d_mult)))

    def dev_zk_args_tail(self, d_c, log_n, k_t, n_args, d_rnd, c_stride=None):
        """smi_dev_zk_args_tail: rows n - k_t + 1 .. n - 1 of the 4 n_args coordinate columns at d_c take the random words at
        d_rnd -> the closing values c_a[n - k_t], n_args elements of four coordinates"""
        closing = np.zeros(4 * n_args, dtype=np.uint64)
        self._ck(self.L.smi_dev_zk_args_tail(self.h, vp(d_c), (1 << log_n) if c_stride is None else c_stride, log_n, k_t, n_args, vp(d_rnd),
                                             closing.ctypes.data_as(C.POINTER(C.c_uint64))))
        return [[int(v) for v in closing[4 * a:4 * a + 4]] for a in range(n_args)]

    def dev_air_compose_zk_args(self, air, d_lde, d_c_lde, n_cols, log_n, log_blowup, num_colinearity_tests, challenges, d_weights, d_out, trace_offset=1,
                                lde_offset=None, stride=None, c_stride=None, out_stride=None):
        """smi_dev_air_compose_zk_xargs: the composition of the derived AIR plus the 3 A auxiliary quotients into four coordinate
        columns; challenges: alpha, gamma (8 unreduced values); d_weights: 4 (W + K + 3 A) u64 on the device"""
        a = self._args_of(air, "dev_air_compose_zk_args")
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
        N = 1 << (log_n + log_blowup)
        ch = (C.c_uint64 * 8)(*[int(v) for v in challenges])
        self._ck(self.L.smi_dev_air_compose_zk_xargs(self.h, C.byref(cfg), C.byref(a), C.byref(xargs_of(a)), vp(d_lde), N if stride is None else stride,
                                                     vp(d_c_lde), N if c_stride is None else c_stride, ch, vp(d_weights), vp(d_out),
                                                     N if out_stride is None else out_stride))

    def _dev_air_prove_deep_zk_args(self, air, a, d_trace_cols, n_cols, log_n, log_blowup, t, trace_offset, lde_offset, timed, check, grind_bits,
                                    fill_multiplicities, zk):
        import os
        xa = xargs_of(a)
        A = xa.count
        seed = os.urandom(32) if zk is True else bytes(zk)
        if len(seed) != 32:
            raise ValueError("zk: the seed is 32 bytes (or True for os.urandom(32))")
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, t, trace_offset, lde_offset, True)
        _d, Dp, kt, _ks = air_plan_deep_zk_args(self.p, a, xa, cfg)
        lookups = [i for i in range(A) if xa.arg[i].kind & 0xff == 1]
        if fill_multiplicities and not lookups:
            raise ValueError("dev_air_prove(fill_multiplicities=True): the argument list has no lookup")
        if fill_multiplicities:   # over the active rows, before the prover writes the randomiser rows
            for i in lookups:
                self._ck_perm(self.L.smi_dev_xargs_multiplicities_rows(self.h, C.byref(a), C.byref(xa), i, vp(d_trace_cols), n_cols, log_n, (1 << log_n) - kt,
                                                                       vp(vp(d_trace_cols).value + 4 * (xa.arg[i].mult_col << log_n))))
        if check:
            if isinstance(air, _lib.Air):
                raise ValueError("zk with check=True derives the AIR to check from a mirror.Air; pass one, or check=False")
            derived = air.zk_derived(self.p, log_n, t, trace_offset, self.prim_nth_root(1 << log_n), with_args=True)
            ok, _con, _row, why = self.dev_air_check(derived.flatten(self.p), d_trace_cols, n_cols, log_n)
            if not ok:
                raise StarkMiError(-50, why)
        roots = np.zeros((3, 32), dtype=np.uint8)
        cnt = 2 * n_cols + 2 * A + Dp
        ood = np.zeros(4 * cnt, dtype=np.uint64)
        proof, plen, mask = vp(), C.c_size_t(), C.c_uint32()
        top = np.zeros(max(t, 1), dtype=np.uint64)
        stage = (C.c_double * 10)()
        self._ck_perm(self.L.smi_dev_air_prove_deep_zk_xargs(self.h, C.byref(cfg), C.byref(a), C.byref(xa), vp(d_trace_cols), seed, roots.ctypes.data,
                                                             ood.ctypes.data, C.byref(proof), C.byref(plen), top.ctypes.data, stage if timed else None,
                                                             0 if grind_bits is None else grind_bits, C.byref(mask)))
        b = C.string_at(proof, plen.value)
        self.L.smi_free(proof)
        closes = [bool(mask.value >> i & 1) for i in range(A)]
        if check and not all(closes):
            raise StarkMiError(-50, f"air_prove_deep_zk_xargs: the arguments {[i for i, c in enumerate(closes) if not c]} do not close")
        out = {"column_roots": roots, "proof": b, "top_indices": [int(v) for v in top[:t]], "closes": closes, "seed": seed,
               "ood": [[int(v) for v in ood[4 * i:4 * i + 4]] for i in range(cnt)]}
        if timed:
            out["stage_ms"] = dict(zip(("random", "lde", "commit", "args", "compose", "segments", "ood", "mask", "fri", "open"), [float(x) for x in stage]))
        return out

    def _zk_takes_a_list(self, a, deep, deep_args, coset_leaves):
        """zk with deep_args=True, coset_leaves=True and an AIR that carries a list: the list variant"""
        return bool(deep_args and coset_leaves and not deep and (self._xargs(a) is not None or self._args(a) is not None))

    def _check_air_folding(self, a, folding, row_leaves, ext):
        _check_folding(folding)
        if folding == 4 and not (row_leaves and ext):
            raise StarkMiError(-50, "folding=4 runs over the row-committed extension proof: pass row_leaves=True, ext=True")
        if folding == 4 and any(f(a) is not None for f in (self._xargs, self._args, self._lookup, self._perm)):
            raise StarkMiError(-50, "folding=4: the permutation, lookup and argument-list provers fold by 2 only")

    def dev_air_prove(self, air, d_trace_cols, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset=1, lde_offset=None,
                      timed=False, check=True, row_leaves=False, ext=False, grind_bits=None, fill_multiplicities=False, folding=2, deep=False,
                      deep_args=False, coset_leaves=False, zk=None):
        """smi_dev_air_prove -> dict(column_roots, proof, top_indices[, stage_ms]).  check (default on) runs
        dev_air_check first and raises StarkMiError naming the first violated constraint and row.
        row_leaves: smi_dev_air_prove_rows -- one tree over the rows of the extended trace; column_roots is then its
        one root, shape (1, 32), and the proof opens every queried position once (verify with row_leaves=True).
        ext (needs row_leaves): smi_dev_air_prove_ext -- weights and FRI over the quartic extension.
        grind_bits (needs ext; None: no grinding): smi_dev_air_prove_ext_pow -- proof-of-work bits before the query indices.
        An AIR with a permutation (mirror.Air.permutation) takes smi_dev_air_prove_perm: row_leaves=True and ext=True are
        required (ValueError otherwise), grind_bits None counts as 0, column_roots is (2, 32) -- root_1, root_2 --, stage_ms has
        a sixth stage "perm", the result has "closes", and check=True raises when the product does not close.
        An AIR with a lookup (mirror.Air.lookup) takes smi_dev_air_prove_lookup in the same way (the sixth stage is "lookup",
        check=True raises when the sum does not close); fill_multiplicities=True first runs dev_lookup_multiplicities into the
        trace's mult_col, which is otherwise taken as filled.
        An AIR with an argument list (mirror.Air.add_permutation / add_lookup) takes smi_dev_air_prove_args in the same way: the
        sixth stage is "args", "closes" is a list of A bools, check=True raises naming the arguments that do not close, and
        fill_multiplicities=True runs dev_lookup_multiplicities once per lookup argument.  A list with selectors or periodic
        members (mirror.Air.extended_args) takes smi_dev_air_prove_xargs and smi_dev_xargs_multiplicities instead.
        folding=4 (needs row_leaves=True, ext=True and an AIR without permutation, lookup or argument list; StarkMiError
        otherwise, and for any value but 2 and 4): smi_dev_air_prove_ext_fold4 -- FRI at folding factor 4, the rows opened at
        the four points of every layer-0 coset; grind_bits None counts as 0.
        deep=True (needs row_leaves=True, ext=True; ValueError together with a permutation, a lookup, an argument list or
        folding=4): smi_dev_air_prove_deep -- out-of-domain sampling, FRI at the full blowup (include/stark_mi.h, "Out-of-domain
        sampling").  column_roots is (2, 32) -- root_1, root_2 --, the result gains "ood" (the record's 2 W + D elements of
        four coordinates each), stage_ms has seven stages, grind_bits None counts as 0.
        deep_args=True (needs row_leaves=True, ext=True, folding=2 and an add_permutation / add_lookup list; ValueError otherwise
        and together with deep=True): smi_dev_air_prove_deep_xargs -- out-of-domain sampling for an argument list (include/
        stark_mi.h, "Out-of-domain sampling with an argument list").  column_roots is (3, 32), the result has "ood" (2 W + 2 A + D
        elements) and "closes", stage_ms has eight stages, fill_multiplicities works as for the list prover.
        coset_leaves=True (needs row_leaves=True, ext=True and exactly one of deep=True and deep_args=True; ValueError naming
        what is missing otherwise): smi_dev_air_prove_deep_fold4 / smi_dev_air_prove_deep_xargs_fold4 -- the same DEEP proof
        with every group of columns committed as a tree of coset leaves and FRI at folding factor 4 (include/stark_mi.h,
        "Out-of-domain sampling over coset leaves").  The result has the keys of the variant it stands beside.  folding stays 2
        on these calls: deep=True, folding=4 and deep_args=True, folding=4 keep raising ValueError.
        zk=seed (32 bytes) or zk=True (os.urandom(32)); needs deep=True, coset_leaves=True, ValueError otherwise:
        smi_dev_air_prove_deep_zk -- the zero-knowledge variant (include/stark_mi.h, "Zero-knowledge DEEP proofs").  The last
        k_t = 8 t + 8 rows of the device trace are OVERWRITTEN with random residues; the statement covers the rows before them.
        check=True checks the derived AIR (air must then be a mirror.Air).  The result gains "seed", which is in no proof and
        must stay with the prover; "ood" has 2 W + D' elements; stage_ms has nine stages.
        zk with deep_args=True, coset_leaves=True and an AIR that carries a list: smi_dev_air_prove_deep_zk_xargs (include/
        stark_mi.h, "Zero-knowledge DEEP proofs with an argument list").  k_t = 8 t + 16 rows are overwritten and every argument
        is over the rows before them; column_roots is (3, 32); the result has "closes" and "seed"; "ood" has 2 W + 2 A + D'
        elements; stage_ms has ten stages; fill_multiplicities=True counts over the active rows only
        (smi_dev_xargs_multiplicities_rows)."""
        a = self._air(air)
        self._check_window(a, "dev_air_prove", deep, deep_args, zk)
        if zk is not None and zk is not False:
            if self._zk_takes_a_list(a, deep, deep_args, coset_leaves):
                self._check_coset_leaves(row_leaves, ext, deep, deep_args)
                self._check_deep_args(a, row_leaves, ext, folding, deep)
                return self._dev_air_prove_deep_zk_args(air, a, d_trace_cols, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset,
                                                        timed, check, grind_bits, fill_multiplicities, zk)
            if not (deep and coset_leaves) or deep_args:
                raise ValueError("zk runs over the coset-leaf DEEP proof of a plain AIR (deep=True, coset_leaves=True) or of an AIR with an argument "
                                 "list (deep_args=True, coset_leaves=True)")
            self._check_coset_leaves(row_leaves, ext, deep, deep_args)
            return self._dev_air_prove_deep_zk(air, a, d_trace_cols, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, timed,
                                               check, row_leaves, ext, grind_bits, fill_multiplicities, folding, zk)
        if coset_leaves:
            self._check_coset_leaves(row_leaves, ext, deep, deep_args)
        if deep_args:
            return self._dev_air_prove_deep_args(a, d_trace_cols, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, timed,
                                                 check, row_leaves, ext, grind_bits, fill_multiplicities, folding, deep, coset_leaves)
        if deep:
            return self._dev_air_prove_deep(a, d_trace_cols, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, timed, check,
                                            row_leaves, ext, grind_bits, fill_multiplicities, folding, coset_leaves)
        self._check_air_folding(a, folding, row_leaves, ext)
        if self._xargs(a) is not None:
            if not (row_leaves and ext):
                raise ValueError("dev_air_prove: an AIR with an argument list needs row_leaves=True, ext=True")
            A = a.xargs.count
            lookups = [i for i in range(A) if a.xargs.arg[i].kind & 0xff == 1]
            if fill_multiplicities and not lookups:
                raise ValueError("dev_air_prove(fill_multiplicities=True): the argument list has no lookup")
            if fill_multiplicities:
                for i in lookups:
                    self.dev_args_multiplicities(a, i, d_trace_cols, n_cols, log_n, vp(d_trace_cols).value + 4 * (a.xargs.arg[i].mult_col << log_n))
            if check:
                ok, _con, _row, why = self.dev_air_check(a, d_trace_cols, n_cols, log_n)
                if not ok:
                    raise StarkMiError(-50, why)
            cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
            roots = np.zeros((2, 32), dtype=np.uint8)
            proof, plen, mask = vp(), C.c_size_t(), C.c_uint32()
            top = np.zeros(max(num_colinearity_tests, 1), dtype=np.uint64)
            stage = (C.c_double * 6)()
            self._ck_perm(self.L.smi_dev_air_prove_xargs(self.h, C.byref(cfg), C.byref(a), C.byref(a.xargs), vp(d_trace_cols), roots.ctypes.data,
                                                         C.byref(proof), C.byref(plen), top.ctypes.data, stage if timed else None,
                                                         0 if grind_bits is None else grind_bits, C.byref(mask)))
            b = C.string_at(proof, plen.value)
            self.L.smi_free(proof)
            closes = [bool(mask.value >> i & 1) for i in range(A)]
            if check and not all(closes):
                raise StarkMiError(-50, f"air_prove_xargs: the arguments {[i for i, c in enumerate(closes) if not c]} do not close")
            out = {"column_roots": roots, "proof": b, "top_indices": [int(v) for v in top[:num_colinearity_tests]], "closes": closes}
            if timed:
                out["stage_ms"] = dict(zip(("lde", "commit", "args", "compose", "fri", "open"), [float(x) for x in stage]))
            return out
        if self._args(a) is not None:
            if not (row_leaves and ext):
                raise ValueError("dev_air_prove: an AIR with an argument list needs row_leaves=True, ext=True")
            lookups = [a.args.arg[i] for i in range(a.args.count) if a.args.arg[i].kind == 1]
            if fill_multiplicities and not lookups:
                raise ValueError("dev_air_prove(fill_multiplicities=True): the argument list has no lookup")
            if fill_multiplicities:
                for g in lookups:
                    one = _lib.AirLookup(g.width, g.mult_col, g.a_col, g.b_col)
                    self._ck_perm(self.L.smi_dev_lookup_multiplicities(self.h, C.byref(one), vp(d_trace_cols), n_cols, log_n,
                                                                       vp(vp(d_trace_cols).value + 4 * (g.mult_col << log_n))))
            if check:
                ok, _con, _row, why = self.dev_air_check(a, d_trace_cols, n_cols, log_n)
                if not ok:
                    raise StarkMiError(-50, why)
            cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
            roots = np.zeros((2, 32), dtype=np.uint8)
            proof, plen, mask = vp(), C.c_size_t(), C.c_uint32()
            top = np.zeros(max(num_colinearity_tests, 1), dtype=np.uint64)
            stage = (C.c_double * 6)()
            self._ck_perm(self.L.smi_dev_air_prove_args(self.h, C.byref(cfg), C.byref(a), C.byref(a.args), vp(d_trace_cols), roots.ctypes.data,
                                                        C.byref(proof), C.byref(plen), top.ctypes.data, stage if timed else None,
                                                        0 if grind_bits is None else grind_bits, C.byref(mask)))
            b = C.string_at(proof, plen.value)
            self.L.smi_free(proof)
            closes = [bool(mask.value >> i & 1) for i in range(a.args.count)]
            if check and not all(closes):
                raise StarkMiError(-50, f"air_prove_args: the arguments {[i for i, c in enumerate(closes) if not c]} do not close")
            out = {"column_roots": roots, "proof": b, "top_indices": [int(v) for v in top[:num_colinearity_tests]], "closes": closes}
            if timed:
                out["stage_ms"] = dict(zip(("lde", "commit", "args", "compose", "fri", "open"), [float(x) for x in stage]))
            return out
        if fill_multiplicities and self._lookup(a) is None:
            raise ValueError("dev_air_prove(fill_multiplicities=True): the AIR has no lookup (mirror.Air.lookup)")
        if self._lookup(a) is not None:
            if not (row_leaves and ext):
                raise ValueError("dev_air_prove: an AIR with a lookup needs row_leaves=True, ext=True")
            if fill_multiplicities:
                self.dev_lookup_multiplicities(a, d_trace_cols, n_cols, log_n, vp(d_trace_cols).value + 4 * (a.lookup.mult_col << log_n))
            if check:
                ok, _con, _row, why = self.dev_air_check(a, d_trace_cols, n_cols, log_n)
                if not ok:
                    raise StarkMiError(-50, why)
            cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
            roots = np.zeros((2, 32), dtype=np.uint8)
            proof, plen, closes = vp(), C.c_size_t(), C.c_int()
            top = np.zeros(max(num_colinearity_tests, 1), dtype=np.uint64)
            stage = (C.c_double * 6)()
            self._ck_perm(self.L.smi_dev_air_prove_lookup(self.h, C.byref(cfg), C.byref(a), C.byref(a.lookup), vp(d_trace_cols), roots.ctypes.data,
                                                          C.byref(proof), C.byref(plen), top.ctypes.data, stage if timed else None,
                                                          0 if grind_bits is None else grind_bits, C.byref(closes)))
            b = C.string_at(proof, plen.value)
            self.L.smi_free(proof)
            if check and not closes.value:
                raise StarkMiError(-50, "air_prove_lookup: the lookup sum does not close (a missing lookup or a wrong multiplicity)")
            out = {"column_roots": roots, "proof": b, "top_indices": [int(v) for v in top[:num_colinearity_tests]], "closes": bool(closes.value)}
            if timed:
                out["stage_ms"] = dict(zip(("lde", "commit", "lookup", "compose", "fri", "open"), [float(x) for x in stage]))
            return out
        if self._perm(a) is not None:
            if not (row_leaves and ext):
                raise ValueError("dev_air_prove: an AIR with a permutation needs row_leaves=True, ext=True")
            if check:
                ok, _con, _row, why = self.dev_air_check(a, d_trace_cols, n_cols, log_n)
                if not ok:
                    raise StarkMiError(-50, why)
            cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
            roots = np.zeros((2, 32), dtype=np.uint8)
            proof, plen, closes = vp(), C.c_size_t(), C.c_int()
            top = np.zeros(max(num_colinearity_tests, 1), dtype=np.uint64)
            stage = (C.c_double * 6)()
            self._ck_perm(self.L.smi_dev_air_prove_perm(self.h, C.byref(cfg), C.byref(a), C.byref(a.perm), vp(d_trace_cols), roots.ctypes.data,
                                                        C.byref(proof), C.byref(plen), top.ctypes.data, stage if timed else None,
                                                        0 if grind_bits is None else grind_bits, C.byref(closes)))
            b = C.string_at(proof, plen.value)
            self.L.smi_free(proof)
            if check and not closes.value:
                raise StarkMiError(-50, "air_prove_perm: the permutation product does not close (the two multisets differ)")
            out = {"column_roots": roots, "proof": b, "top_indices": [int(v) for v in top[:num_colinearity_tests]], "closes": bool(closes.value)}
            if timed:
                out["stage_ms"] = dict(zip(("lde", "commit", "perm", "compose", "fri", "open"), [float(x) for x in stage]))
            return out
        if ext and not row_leaves:
            raise StarkMiError(-50, "dev_air_prove(ext=True) commits to one tree over the rows: pass row_leaves=True")
        if grind_bits is not None and not ext:
            raise StarkMiError(-50, "dev_air_prove(grind_bits=...) grinds the extension proof: pass ext=True")
        if check:
            ok, _con, _row, why = self.dev_air_check(a, d_trace_cols, n_cols, log_n)
            if not ok:
                raise StarkMiError(-50, why)   # SMI_ERR_BAD_ARG: the trace handed in does not satisfy the AIR
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, row_leaves)
        roots = np.zeros((1 if row_leaves else n_cols, 32), dtype=np.uint8)
        proof, plen = vp(), C.c_size_t()
        top = np.zeros(max(num_colinearity_tests, 1), dtype=np.uint64)
        stage = (C.c_double * 5)()
        prove = self.L.smi_dev_air_prove_ext if ext else (self.L.smi_dev_air_prove_rows if row_leaves else self.L.smi_dev_air_prove)
        args = (self.h, C.byref(cfg), C.byref(a), vp(d_trace_cols), roots.ctypes.data, C.byref(proof), C.byref(plen), top.ctypes.data,
                stage if timed else None)
        if folding == 4:
            self._ck(self.L.smi_dev_air_prove_ext_fold4(*args, grind_bits or 0))
        elif grind_bits is None:
            self._ck(prove(*args))
        else:
            self._ck(self.L.smi_dev_air_prove_ext_pow(*args, grind_bits))
        b = C.string_at(proof, plen.value)
        self.L.smi_free(proof)
        out = {"column_roots": roots, "proof": b, "top_indices": [int(v) for v in top[:num_colinearity_tests]]}
        if timed:
            out["stage_ms"] = dict(zip(("lde", "commit", "compose", "fri", "open"), [float(x) for x in stage]))
        return out

    def air_verify(self, air, proof: bytes, column_roots, n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset=1,
                   lde_offset=None, row_leaves=False, ext=False, grind_bits=None, folding=2, deep=False, deep_args=False,
                   coset_leaves=False, zk=False):
        """verifier of dev_air_prove -> (accept, reason).  zk=True (needs deep=True, coset_leaves=True; ValueError otherwise):
        smi_air_verify_deep_zk; with deep_args=True, coset_leaves=True and an AIR that carries a list: smi_air_verify_deep_zk_xargs.  row_leaves: smi_air_verify_rows, column_roots is the one root of
        the tree over the rows.  ext (needs row_leaves): smi_air_verify_ext.  grind_bits (needs ext; None: a proof without
        grinding): smi_air_verify_ext_pow, the least proof-of-work difficulty demanded.
        An AIR with a permutation takes smi_air_verify_perm: row_leaves=True and ext=True are required (ValueError otherwise),
        column_roots is root_1 then root_2, grind_bits None counts as 0.  An AIR with a lookup takes smi_air_verify_lookup in
        the same way, and an AIR with an argument list smi_air_verify_args (smi_air_verify_xargs when the list has selectors
        or periodic members).
        folding=4: smi_air_verify_ext_fold4, under the conditions of dev_air_prove(folding=4).
        deep=True: smi_air_verify_deep, under the conditions of dev_air_prove(deep=True); column_roots is root_1 then root_2.
        deep_args=True: smi_air_verify_deep_xargs, under the conditions of dev_air_prove(deep_args=True); three roots.
        coset_leaves=True: smi_air_verify_deep_fold4 / smi_air_verify_deep_xargs_fold4, under the conditions of
        dev_air_prove(coset_leaves=True); folding stays 2."""
        self._check_window(self._air(air), "air_verify", deep, deep_args, zk)
        zk_list = bool(zk) and self._zk_takes_a_list(self._air(air), deep, deep_args, coset_leaves)
        if zk and not zk_list and (not (deep and coset_leaves) or deep_args):
            raise ValueError("zk runs over the coset-leaf DEEP proof of a plain AIR (deep=True, coset_leaves=True) or of an AIR with an argument "
                             "list (deep_args=True, coset_leaves=True)")
        if coset_leaves:
            self._check_coset_leaves(row_leaves, ext, deep, deep_args)
        if deep_args:
            a = self._air(air)
            xa = self._check_deep_args(a, row_leaves, ext, folding, deep)
            cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
            roots = np.ascontiguousarray(np.frombuffer(b"".join(bytes(r) for r in column_roots), dtype=np.uint8))
            if roots.size != 96:
                raise StarkMiError(-50, "air_verify(deep_args=True) takes three 32-byte roots")
            acc = C.c_int()
            verify = self.L.smi_air_verify_deep_zk_xargs if zk_list else self.L.smi_air_verify_deep_xargs_fold4 if coset_leaves else self.L.smi_air_verify_deep_xargs
            self._ck(verify(self.h, C.byref(cfg), C.byref(a), C.byref(xa), roots.ctypes.data, proof, len(proof), C.byref(acc),
                            0 if grind_bits is None else grind_bits))
            return bool(acc.value), ("" if acc.value else self.L.smi_last_error(self.h).decode())
        if deep:
            a = self._air(air)
            self._check_deep(a, row_leaves, ext, folding, False)
            cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
            roots = np.ascontiguousarray(np.frombuffer(b"".join(bytes(r) for r in column_roots), dtype=np.uint8))
            if roots.size != 64:
                raise StarkMiError(-50, "air_verify(deep=True) takes two 32-byte roots")
            acc = C.c_int()
            verify = self.L.smi_air_verify_deep_zk if zk else self.L.smi_air_verify_deep_fold4 if coset_leaves else self.L.smi_air_verify_deep
            self._ck(verify(self.h, C.byref(cfg), C.byref(a), roots.ctypes.data, proof, len(proof), C.byref(acc), 0 if grind_bits is None else grind_bits))
            return bool(acc.value), ("" if acc.value else self.L.smi_last_error(self.h).decode())
        self._check_air_folding(self._air(air), folding, row_leaves, ext)
        if self._xargs(self._air(air)) is not None:
            if not (row_leaves and ext):
                raise ValueError("air_verify: an AIR with an argument list needs row_leaves=True, ext=True")
            a = self._air(air)
            cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
            roots = np.ascontiguousarray(np.frombuffer(b"".join(bytes(r) for r in column_roots), dtype=np.uint8))
            if roots.size != 64:
                raise StarkMiError(-50, "air_verify: an AIR with an argument list takes two 32-byte roots")
            acc = C.c_int()
            self._ck(self.L.smi_air_verify_xargs(self.h, C.byref(cfg), C.byref(a), C.byref(a.xargs), roots.ctypes.data, proof, len(proof), C.byref(acc),
                                                 0 if grind_bits is None else grind_bits))
            return bool(acc.value), ("" if acc.value else self.L.smi_last_error(self.h).decode())
        if self._args(self._air(air)) is not None:
            if not (row_leaves and ext):
                raise ValueError("air_verify: an AIR with an argument list needs row_leaves=True, ext=True")
            a = self._air(air)
            cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
            roots = np.ascontiguousarray(np.frombuffer(b"".join(bytes(r) for r in column_roots), dtype=np.uint8))
            if roots.size != 64:
                raise StarkMiError(-50, "air_verify: an AIR with an argument list takes two 32-byte roots")
            acc = C.c_int()
            self._ck(self.L.smi_air_verify_args(self.h, C.byref(cfg), C.byref(a), C.byref(a.args), roots.ctypes.data, proof, len(proof), C.byref(acc),
                                                0 if grind_bits is None else grind_bits))
            return bool(acc.value), ("" if acc.value else self.L.smi_last_error(self.h).decode())
        if self._lookup(self._air(air)) is not None:
            if not (row_leaves and ext):
                raise ValueError("air_verify: an AIR with a lookup needs row_leaves=True, ext=True")
            a = self._air(air)
            cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
            roots = np.ascontiguousarray(np.frombuffer(b"".join(bytes(r) for r in column_roots), dtype=np.uint8))
            if roots.size != 64:
                raise StarkMiError(-50, "air_verify: an AIR with a lookup takes two 32-byte roots")
            acc = C.c_int()
            self._ck(self.L.smi_air_verify_lookup(self.h, C.byref(cfg), C.byref(a), C.byref(a.lookup), roots.ctypes.data, proof, len(proof), C.byref(acc),
                                                  0 if grind_bits is None else grind_bits))
            return bool(acc.value), ("" if acc.value else self.L.smi_last_error(self.h).decode())
        if self._perm(self._air(air)) is not None:
            if not (row_leaves and ext):
                raise ValueError("air_verify: an AIR with a permutation needs row_leaves=True, ext=True")
            a = self._air(air)
            cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, True)
            roots = np.ascontiguousarray(np.frombuffer(b"".join(bytes(r) for r in column_roots), dtype=np.uint8))
            if roots.size != 64:
                raise StarkMiError(-50, "air_verify: an AIR with a permutation takes two 32-byte roots")
            acc = C.c_int()
            self._ck(self.L.smi_air_verify_perm(self.h, C.byref(cfg), C.byref(a), C.byref(a.perm), roots.ctypes.data, proof, len(proof), C.byref(acc),
                                                0 if grind_bits is None else grind_bits))
            return bool(acc.value), ("" if acc.value else self.L.smi_last_error(self.h).decode())
        if ext and not row_leaves:
            raise StarkMiError(-50, "air_verify(ext=True) checks a proof over one row tree: pass row_leaves=True")
        if grind_bits is not None and not ext:
            raise StarkMiError(-50, "air_verify(grind_bits=...) checks a ground extension proof: pass ext=True")
        cfg = self._stark_cfg(n_cols, log_n, log_blowup, num_colinearity_tests, trace_offset, lde_offset, row_leaves)
        a = self._air(air)
        roots = np.ascontiguousarray(np.frombuffer(b"".join(bytes(r) for r in column_roots), dtype=np.uint8))
        acc = C.c_int()
        verify = self.L.smi_air_verify_ext if ext else (self.L.smi_air_verify_rows if row_leaves else self.L.smi_air_verify)
        if row_leaves and roots.size != 32:
            raise StarkMiError(-50, "air_verify(row_leaves=True) takes the one 32-byte root of the row tree")
        args = (self.h, C.byref(cfg), C.byref(a), roots.ctypes.data, proof, len(proof), C.byref(acc))
        if folding == 4:
            self._ck(self.L.smi_air_verify_ext_fold4(*args, grind_bits or 0))
        elif grind_bits is None:
            self._ck(verify(*args))
        else:
            self._ck(self.L.smi_air_verify_ext_pow(*args, grind_bits))
        return bool(acc.value), ("" if acc.value else self.L.smi_last_error(self.h).decode())


class DeviceTree:
    """MerkleTree kept on the device (all levels, src/merkle.rs:4-8)."""

    def __init__(self, eng, handle):
        self.eng, self.h = eng, handle
        self.n = int(eng.L.smi_merkle_num_leaves(handle))

    def root(self) -> bytes:
        out = (C.c_uint8 * 32)()
        self.eng._ck(self.eng.L.smi_merkle_root(self.eng.h, self.h, out))
        return bytes(out)

    def open(self, index):
        path = np.zeros((64, 32), dtype=np.uint8)
        depth = C.c_size_t()
        self.eng._ck(self.eng.L.smi_merkle_open(self.eng.h, self.h, index, path.ctypes.data, C.byref(depth)))
        return [bytes(path[i]) for i in range(depth.value)]

    def level(self, lvl):
        out = np.zeros((max(self.n >> lvl, 1), 32), dtype=np.uint8)
        cnt = C.c_size_t()
        self.eng._ck(self.eng.L.smi_merkle_level(self.eng.h, self.h, lvl, out.ctypes.data, C.byref(cnt)))
        return out[:cnt.value]

    def free(self):
        if self.h:
            self.eng.L.smi_merkle_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class FriRun:
    """Device-resident result of Fri::commit: the codewords it returns and the per-round trees."""

    def __init__(self, eng, handle):
        self.eng, self.h = eng, handle

    def __len__(self):
        n = C.c_size_t()
        self.eng._ck(self.eng.L.smi_fri_run_num_codewords(self.h, C.byref(n)))
        return n.value

    def codeword(self, rnd):
        ln = C.c_size_t()
        self.eng._ck(self.eng.L.smi_fri_run_codeword(self.h, rnd, None, C.byref(ln)))
        out = np.empty(ln.value, dtype=np.uint64)
        self.eng._ck(self.eng.L.smi_fri_run_codeword(self.h, rnd, out.ctypes.data, C.byref(ln)))
        return out

    def open(self, rnd, index):
        path = np.zeros((64, 32), dtype=np.uint8)
        depth = C.c_size_t()
        self.eng._ck(self.eng.L.smi_fri_run_open(self.h, rnd, index, path.ctypes.data, C.byref(depth)))
        return [bytes(path[i]) for i in range(depth.value)]

    def free(self):
        if self.h:
            self.eng.L.smi_fri_run_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def air_plan(p, air, cfg):
    """smi_air_plan (host only: no context, no GPU) -> (d, E).  air: a flattened _lib.Air; cfg: a _lib.StarkCfg."""
    d, e = C.c_uint32(), C.c_uint64()
    L = _lib.lib()
    st = L.smi_air_plan(p, C.byref(cfg), C.byref(air), C.byref(d), C.byref(e))
    if st:
        raise StarkMiError(st, f"{_lib.status_string(st)}: {L.smi_air_last_error().decode()}")
    return d.value, e.value


def air_plan_deep(p, air, cfg, with_length=False):
    """smi_air_plan_deep (host only) -> (d, D), or with_length (d, D, proof bytes of smi_air_deep_layout for cfg's number of
    colinearity tests).  air: a flattened _lib.Air"""
    d, D, n = C.c_uint32(), C.c_uint32(), C.c_size_t()
    L = _lib.lib()
    st = L.smi_air_plan_deep(p, C.byref(cfg), C.byref(air), C.byref(d), C.byref(D))
    if not st and with_length:
        st = L.smi_air_deep_layout(p, C.byref(cfg), C.byref(air), C.byref(n))
    if st:
        raise StarkMiError(st, f"{_lib.status_string(st)}: {L.smi_air_last_error().decode()}")
    return (d.value, D.value, n.value) if with_length else (d.value, D.value)


def air_plan_deep_zk(p, air, cfg):
    """smi_air_plan_deep_zk (host only) -> (d, D', k_t, k_s) for cfg's number of colinearity tests.  air: a flattened _lib.Air"""
    d, D, kt, ks = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    L = _lib.lib()
    st = L.smi_air_plan_deep_zk(p, C.byref(cfg), C.byref(air), C.byref(d), C.byref(D), C.byref(kt), C.byref(ks))
    if st:
        raise StarkMiError(st, f"{_lib.status_string(st)}: {L.smi_air_last_error().decode()}")
    return d.value, D.value, kt.value, ks.value


def air_deep_zk_layout(p, air, cfg):
    """smi_air_deep_zk_layout (host only) -> (folds, proof bytes).  air: a flattened _lib.Air"""
    f, n = C.c_uint64(), C.c_size_t()
    L = _lib.lib()
    st = L.smi_air_deep_zk_layout(p, C.byref(cfg), C.byref(air), C.byref(f), C.byref(n))
    if st:
        raise StarkMiError(st, f"{_lib.status_string(st)}: {L.smi_air_last_error().decode()}")
    return f.value, n.value


def air_plan_deep_zk_args(p, air, xargs, cfg):
    """smi_air_plan_deep_zk_xargs (host only) -> (d, D', k_t, k_s).  air: a flattened _lib.Air; xargs: xargs_of(air)"""
    d, D, kt, ks = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    L = _lib.lib()
    st = L.smi_air_plan_deep_zk_xargs(p, C.byref(cfg), C.byref(air), C.byref(xargs), C.byref(d), C.byref(D), C.byref(kt), C.byref(ks))
    if st:
        raise StarkMiError(st, f"{_lib.status_string(st)}: {L.smi_air_last_error().decode()}")
    return d.value, D.value, kt.value, ks.value


def air_deep_zk_args_layout(p, air, xargs, cfg):
    """smi_air_deep_zk_xargs_layout (host only) -> (folds, proof bytes)"""
    f, n = C.c_uint64(), C.c_size_t()
    L = _lib.lib()
    st = L.smi_air_deep_zk_xargs_layout(p, C.byref(cfg), C.byref(air), C.byref(xargs), C.byref(f), C.byref(n))
    if st:
        raise StarkMiError(st, f"{_lib.status_string(st)}: {L.smi_air_last_error().decode()}")
    return f.value, n.value


def xargs_of(air):
    """the _lib.AirXArgs of a flattened AIR's argument list: its own when the list has selectors or periodic members (or was
    flattened with xargs_always), else its smi_air_args written in the superset form -- every column an operand of this row,
    no selector.  None without a list."""
    if getattr(air, "xargs", None) is not None:
        return air.xargs
    args = getattr(air, "args", None)
    if args is None:
        return None
    raw = (_lib.AirXArg * args.count)()
    for i in range(args.count):
        g = args.arg[i]
        raw[i] = _lib.AirXArg(g.kind, g.width, g.mult_col, 0, g.a_col, g.b_col, _lib.NO_SELECTOR, _lib.NO_SELECTOR)
    out = _lib.AirXArgs(args.count, 0, raw)
    out._keep = (raw, args)
    return out


def air_plan_deep_args(p, air, xargs, cfg, with_length=False):
    """smi_air_plan_deep_xargs (host only) -> (d, D), or with_length (d, D, proof bytes of smi_air_deep_xargs_layout for cfg's
    number of colinearity tests).  air: a flattened _lib.Air; xargs: a _lib.AirXArgs"""
    d, D, n = C.c_uint32(), C.c_uint32(), C.c_size_t()
    L = _lib.lib()
    st = L.smi_air_plan_deep_xargs(p, C.byref(cfg), C.byref(air), C.byref(xargs), C.byref(d), C.byref(D))
    if not st and with_length:
        st = L.smi_air_deep_xargs_layout(p, C.byref(cfg), C.byref(air), C.byref(xargs), C.byref(n))
    if st:
        raise StarkMiError(st, f"{_lib.status_string(st)}: {L.smi_air_last_error().decode()}")
    return (d.value, D.value, n.value) if with_length else (d.value, D.value)


def air_deep_fold4_layout(p, air, cfg):
    """smi_air_deep_fold4_layout (host only) -> (folds, proof bytes) for cfg's number of colinearity tests.  air: a flattened
    _lib.Air"""
    folds, n = C.c_uint64(), C.c_size_t()
    L = _lib.lib()
    st = L.smi_air_deep_fold4_layout(p, C.byref(cfg), C.byref(air), C.byref(folds), C.byref(n))
    if st:
        raise StarkMiError(st, f"{_lib.status_string(st)}: {L.smi_air_last_error().decode()}")
    return int(folds.value), int(n.value)


def air_deep_args_fold4_layout(p, air, xargs, cfg):
    """smi_air_deep_xargs_fold4_layout (host only) -> (folds, proof bytes).  air: a flattened _lib.Air; xargs: a _lib.AirXArgs"""
    folds, n = C.c_uint64(), C.c_size_t()
    L = _lib.lib()
    st = L.smi_air_deep_xargs_fold4_layout(p, C.byref(cfg), C.byref(air), C.byref(xargs), C.byref(folds), C.byref(n))
    if st:
        raise StarkMiError(st, f"{_lib.status_string(st)}: {L.smi_air_last_error().decode()}")
    return int(folds.value), int(n.value)


def air_plan_perm(p, air, perm, cfg):
    """smi_air_plan_perm (host only) -> (d = max(d_air, 2), E).  air: a flattened _lib.Air; perm: a _lib.AirPerm"""
    d, e = C.c_uint32(), C.c_uint64()
    L = _lib.lib()
    st = L.smi_air_plan_perm(p, C.byref(cfg), C.byref(air), C.byref(perm), C.byref(d), C.byref(e))
    if st:
        raise StarkMiError(st, f"{_lib.status_string(st)}: {L.smi_air_last_error().decode()}")
    return d.value, e.value


def air_plan_args(p, air, args, cfg):
    """smi_air_plan_args (host only) -> (d, E).  air: a flattened _lib.Air; args: a _lib.AirArgs"""
    L = _lib.lib()
    d, e = C.c_uint32(), C.c_uint64()
    st = L.smi_air_plan_args(p, C.byref(cfg), C.byref(air), C.byref(args), C.byref(d), C.byref(e))
    if st != 0:
        raise StarkMiError(st, f"{_lib.status_string(st)}: {L.smi_air_last_error().decode()}")
    return d.value, e.value


def air_plan_xargs(p, air, xargs, cfg):
    """smi_air_plan_xargs (host only) -> (d, E).  air: a flattened _lib.Air; xargs: a _lib.AirXArgs"""
    L = _lib.lib()
    d, e = C.c_uint32(), C.c_uint64()
    st = L.smi_air_plan_xargs(p, C.byref(cfg), C.byref(air), C.byref(xargs), C.byref(d), C.byref(e))
    if st != 0:
        raise StarkMiError(st, f"{_lib.status_string(st)}: {L.smi_air_last_error().decode()}")
    return d.value, e.value


def air_plan_lookup(p, air, lookup, cfg):
    """smi_air_plan_lookup (host only) -> (d = max(d_air, 3), E).  air: a flattened _lib.Air; lookup: a _lib.AirLookup"""
    d, e = C.c_uint32(), C.c_uint64()
    L = _lib.lib()
    st = L.smi_air_plan_lookup(p, C.byref(cfg), C.byref(air), C.byref(lookup), C.byref(d), C.byref(e))
    if st:
        raise StarkMiError(st, f"{_lib.status_string(st)}: {L.smi_air_last_error().decode()}")
    return d.value, e.value


def _ext_call(fn, p, g, *elems):
    arrs = [(C.c_uint64 * 4)(*[int(v) for v in e]) for e in elems]
    out = (C.c_uint64 * 4)()
    st = fn(p, g, *arrs, out)
    if st:
        raise StarkMiError(st, _lib.status_string(st))
    return [int(v) for v in out]


def ext_mul(p, g, a, b):
    """smi_ext_mul (host only, no GPU): a * b in F_p[X] / (X^4 - g), four canonical coordinates each, low degree first"""
    return _ext_call(_lib.lib().smi_ext_mul, p, g, a, b)


def ext_inv(p, g, a):
    """smi_ext_inv (host only, no GPU); StarkMiError "no inverse" for zero"""
    return _ext_call(_lib.lib().smi_ext_inv, p, g, a)


def grind_check(transcript, nonce, bits):
    """smi_grind_check (host only, no GPU): pow_ok(transcript, nonce, bits) -- the hash of transcript || nonce (8 little-endian
    bytes) has `bits` low zero bits in the u64 read from its bytes 24..31"""
    t = bytes(transcript)
    ok = C.c_int()
    st = _lib.lib().smi_grind_check(t if t else None, len(t), nonce, bits, C.byref(ok))
    if st:
        raise StarkMiError(st, _lib.status_string(st))
    return bool(ok.value)


def _check_folding(folding):
    if folding not in (2, 4):
        raise StarkMiError(-50, f"folding must be 2 or 4, not {folding!r}")


def fri_fold4_layout(cfg):
    """smi_fri_fold4_layout (host only, no GPU) -> (folds, last codeword length, proof bytes) of extension FRI at folding
    factor 4 for this FriCfg"""
    folds, last, plen = C.c_uint64(), C.c_uint64(), C.c_size_t()
    st = _lib.lib().smi_fri_fold4_layout(C.byref(cfg), C.byref(folds), C.byref(last), C.byref(plen))
    if st:
        raise StarkMiError(st, _lib.status_string(st))
    return int(folds.value), int(last.value), int(plen.value)


def default_engine(p=P_REF, g=G_REF, device=0):
    """Process-wide engine per (p, device); created on first use."""
    key = (p, device)
    if key not in _default:
        _default[key] = Engine(p, g, device)
    return _default[key]
