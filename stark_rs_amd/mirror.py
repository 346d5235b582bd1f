"""Host-side mirror of the reference's types for the hot path -- same names, argument meaning
and error behaviour as 0xSooki/stark-rs, with the heavy methods routed through the C ABI
(include/stark_mi.h) onto the GPU.  The Rust binding a maintainer would add is shown in
INTEGRATION.md; this mirror exists so the parity tests read like the reference's own tests
(tests/test_gpu_mirror.py transliterates them).

Scalar field operations (FiniteField::add/sub/mul/...) are plain host integer arithmetic, as in
the reference (src/ff.rs:138-233) -- they are the glue between kernel calls, not the hot path.
Anything that touches a whole codeword, polynomial or tree goes to the device:

    Polynomial.interpolate_domain / eval_domain / scale   -> smi_intt / smi_coset_ntt / smi_poly_scale
    Polynomial.zerofier                                    -> smi_poly_zerofier (subproduct tree, any points)
    Hash.from_field_elements / combine / from_bytes       -> smi_hash_* (device kernels, even for one digest)
    MerkleTree.new / commit / open                        -> smi_merkle_*
    FiatShamir.challenge                                   -> smi_hash_bytes
    Fri.fold_codeword / commit / prove                     -> smi_fri_fold / smi_fri_commit / smi_fri_prove

Polynomial.interpolate_domain / eval_domain keep the fast-path contract: on a domain that is not
geometric (offset * omega^k) the mirror raises StarkMiError("domain is not offset*omega^k").  Such
domains have a general GPU path of their own, which the Rust shim takes there:
smi_poly_interpolate_points / smi_poly_eval_points, i.e. Engine.poly_interpolate_points /
Engine.poly_eval_points (subproduct trees on the device).  This package has no CPU compute path by
design.
"""
import numpy as np

from ._lib import StarkMiError
from .engine import P_REF, default_engine

PANIC = StarkMiError  # a reference panic surfaces as this exception with the identical message


class FiniteField:
    """src/ff.rs:9-12,108-233"""

    def __init__(self, p):
        self.p = p

    def __eq__(self, o):
        return isinstance(o, FiniteField) and self.p == o.p

    def __hash__(self):
        return hash(self.p)

    def modulus(self):
        return self.p

    def new_element(self, value):
        return FieldElement(value, self)      # unreduced, like src/ff.rs:113-118

    def zero(self):
        return FieldElement(0, self)

    def one(self):
        return FieldElement(1, self)

    def add(self, l, r):
        return FieldElement((l.value + r.value) % self.p, self)

    def sub(self, l, r):
        return FieldElement((self.p + l.value - r.value) % self.p, self)

    def mul(self, l, r):
        return FieldElement((l.value * r.value) % self.p, self)

    def neg(self, x):
        return FieldElement((self.p - x.value) % self.p, self)

    def inv(self, x):
        if x.value % self.p == 0:
            raise StarkMiError(-1, "no inverse")                  # src/ff.rs:171
        return FieldElement(pow(x.value, -1, self.p), self)

    def div(self, l, r):
        if r.value == 0:
            raise StarkMiError(-2, "no division by zero")         # src/ff.rs:182
        return self.mul(l, self.inv(r))

    def exp(self, base, e):
        return FieldElement(pow(base.value, e, self.p), self)

    def g(self):
        if self.p != P_REF:
            raise StarkMiError(-16, "assertion failed: self.p == 998244353")   # src/ff.rs:192
        return FieldElement(3, self)

    def prim_nth_root(self, n):
        if self.p != P_REF:
            raise StarkMiError(-16, "assertion failed: self.p == 998244353")   # src/ff.rs:216
        if n == 0 or n & (n - 1):
            raise StarkMiError(-3, "n must be a power of two")                 # src/ff.rs:217
        if n > (1 << 23):
            raise StarkMiError(-4, "n > 2^23 not supported by this modulus")   # src/ff.rs:218
        return self.exp(self.g(), (self.p - 1) // n)

    def sample(self, salt: bytes):
        acc = 0
        for b in salt:                                             # src/ff.rs:225-232
            acc = (acc << 8) % self.p
            acc = (acc ^ b) % self.p
        return FieldElement(acc, self)

    def engine(self):
        """The GPU context for this modulus (one per process)."""
        if self.p == P_REF:
            return default_engine()
        from .engine import G2, P2
        if self.p == P2:
            return default_engine(P2, G2)
        raise StarkMiError(-52, f"unsupported modulus for this size: no generator registered for p={self.p}")


class FieldElement:
    """src/ff.rs:24-28 plus the operator impls (:30-106, :235-281)"""
    __slots__ = ("value", "field")

    def __init__(self, value, field):
        self.value, self.field = value, field

    def __eq__(self, o):
        return isinstance(o, FieldElement) and self.value == o.value and self.field == o.field

    def __hash__(self):
        return hash((self.value, self.field.p))

    def __lt__(self, o):
        return self.value < o.value

    def __add__(self, o):
        return self.field.add(self, o)

    def __sub__(self, o):
        return self.field.sub(self, o)

    def __mul__(self, o):
        return self.field.mul(self, o)

    def __truediv__(self, o):
        return self.field.div(self, o)

    def __neg__(self):
        return self.field.neg(self)

    def __xor__(self, e):
        return self.field.exp(self, e)

    def pow(self, e):
        return self.field.exp(self, e)

    def __repr__(self):
        return f"FieldElement({self.value})"


class Ext4:
    """An element of F_p[X] / (X^4 - g) (include/stark_mi.h, "Quartic extension"): four canonical coordinates, low degree
    first.  Products and inverses go through the library's host helpers (smi_ext_mul / smi_ext_inv: no GPU needed)."""
    __slots__ = ("c", "p", "g")

    def __init__(self, coords, p, g):
        coords = [int(v) % p for v in coords]
        if len(coords) != 4:
            raise ValueError("Ext4 takes four coordinates")
        self.c, self.p, self.g = tuple(coords), p, g

    @classmethod
    def embed(cls, value, p, g):
        return cls((value, 0, 0, 0), p, g)

    def _same(self, o):
        if isinstance(o, FieldElement):
            o = Ext4.embed(o.value, self.p, self.g)
        elif isinstance(o, int):
            o = Ext4.embed(o, self.p, self.g)
        if (o.p, o.g) != (self.p, self.g):
            raise ValueError("Ext4 operands of different fields")
        return o

    def __eq__(self, o):
        return isinstance(o, Ext4) and (self.c, self.p, self.g) == (o.c, o.p, o.g)

    def __hash__(self):
        return hash((self.c, self.p, self.g))

    def __add__(self, o):
        o = self._same(o)
        return Ext4([a + b for a, b in zip(self.c, o.c)], self.p, self.g)

    def __sub__(self, o):
        o = self._same(o)
        return Ext4([a - b for a, b in zip(self.c, o.c)], self.p, self.g)

    def __neg__(self):
        return Ext4([-a for a in self.c], self.p, self.g)

    def __mul__(self, o):
        from .engine import ext_mul
        return Ext4(ext_mul(self.p, self.g, self.c, self._same(o).c), self.p, self.g)

    def inv(self):
        from .engine import ext_inv
        return Ext4(ext_inv(self.p, self.g, self.c), self.p, self.g)     # "no inverse" for zero, like src/ff.rs:171

    def __truediv__(self, o):
        return self * self._same(o).inv()

    def pow(self, e):
        r, b = Ext4.embed(1, self.p, self.g), self
        while e:
            if e & 1:
                r = r * b
            b = b * b
            e >>= 1
        return r

    def __repr__(self):
        return f"Ext4{self.c}"


def _vals(elems):
    return np.fromiter((e.value for e in elems), dtype=np.uint64, count=len(elems))


class Polynomial:
    """src/univariate/mod.rs:8-153 (+ interpolate.rs, eval.rs); ascending coefficients."""

    def __init__(self, coeffs, field):
        self.coeffs, self.field = list(coeffs), field

    new = classmethod(lambda cls, coeffs, field: cls(coeffs, field))

    @staticmethod
    def zero_poly(field):
        return Polynomial([], field)

    @staticmethod
    def constant_poly(field, value):
        return Polynomial([field.new_element(value)], field)

    @staticmethod
    def linear_poly(field, a, b):
        return Polynomial([field.new_element(a), field.new_element(b)], field)

    def deg(self):
        d = -1
        for i, c in enumerate(self.coeffs):
            if c.value != 0:
                d = i
        return d

    def is_zero(self):
        return self.deg() == -1

    def __eq__(self, o):                                            # mod.rs:13-39: trailing zeros ignored
        if self.deg() != o.deg():
            return False
        return all(self.coeffs[i] == o.coeffs[i] for i in range(self.deg() + 1))

    def scale(self, factor):
        """f(cX) -- mod.rs:99-113, on the device."""
        if not self.coeffs:
            return Polynomial([], self.field)
        out = self.field.engine().poly_scale(_vals(self.coeffs), factor.value % self.field.p)
        return Polynomial([FieldElement(int(v), self.field) for v in out], self.field)

    def __mul__(self, o):
        """Polynomial::mul (mul.rs:6-29), NTT-based on the device."""
        out = self.field.engine().poly_mul(_vals(self.coeffs), _vals(o.coeffs))
        return Polynomial([FieldElement(int(v), self.field) for v in out], self.field)

    mul = staticmethod(lambda lhs, rhs: lhs * rhs)

    @staticmethod
    def div(numer, denom):
        """Polynomial::div (div.rs:6-42) -> (quotient, remainder), NTT products on the device."""
        q, r = numer.field.engine().poly_div(_vals(numer.coeffs), _vals(denom.coeffs))
        f = numer.field
        return Polynomial([FieldElement(int(v), f) for v in q], f), Polynomial([FieldElement(int(v), f) for v in r], f)

    def __truediv__(self, o):
        return Polynomial.div(self, o)

    @staticmethod
    def intdiv(numer, denom):                                       # div.rs:44-48
        q, r = Polynomial.div(numer, denom)
        assert r.is_zero()
        return q

    @staticmethod
    def modulo(numer, denom):                                       # div.rs:50-53
        return Polynomial.div(numer, denom)[1]

    @staticmethod
    def zerofier(domain):
        """mod.rs:77-96: prod (x - d).  The reference multiplies the factors in one by one; here one
        subproduct tree on the device (smi_poly_zerofier) gives the same polynomial."""
        field = domain[0].field
        d = np.fromiter((e.value % field.p for e in domain), dtype=np.uint64, count=len(domain))
        z = field.engine().poly_zerofier(d)
        return Polynomial([FieldElement(int(c), field) for c in z], field)

    @staticmethod
    def interpolate_domain(domain, values):
        """interpolate.rs:6-44 for a geometric domain offset*omega_n^k (the fast-path contract)."""
        if len(domain) != len(values):
            raise StarkMiError(-14, "assertion failed: domain.len() == values.len()")
        if len(domain) == 0:
            raise StarkMiError(-15, "assertion failed: domain.len() > 0")
        field = domain[0].field
        eng = field.engine()
        d = _vals(domain)
        if len(set(int(x) for x in d)) != len(d):
            raise StarkMiError(-1, "no inverse")                    # duplicate points: ff.rs:171 via interpolate.rs:34
        ok, offset = eng.domain_is_geometric(d)
        if not ok:
            raise StarkMiError(-53, "domain is not offset*omega^k")
        v = _vals(values)
        out = eng.intt(v, offset)
        if len(v) > 1 and not v.any():
            return Polynomial([], field)                            # H8: all-zero values give the empty polynomial
        return Polynomial([FieldElement(int(c), field) for c in out], field)

    def eval(self, x):
        """eval.rs:6-14 -- one point: host Horner-equivalent (not the hot path)."""
        p = self.field.p
        acc = 0
        for c in reversed(self.coeffs):
            acc = (acc * x.value + c.value) % p
        return FieldElement(acc, self.field)

    def eval_domain(self, domain):
        """eval.rs:16-21 on a geometric domain, in domain order, on the device."""
        if not domain:
            return []
        field = domain[0].field
        eng = field.engine()
        d = _vals(domain)
        ok, offset = eng.domain_is_geometric(d)
        n_c = self.deg() + 1
        if not ok or n_c > len(d):
            raise StarkMiError(-53, "domain is not offset*omega^k")
        out = eng.coset_ntt(_vals(self.coeffs[:n_c]), len(d).bit_length() - 1, offset)
        return [FieldElement(int(v), field) for v in out]


class Hash:
    """src/hash.rs:1-46; digests are computed by the device kernels."""
    __slots__ = ("bytes",)

    def __init__(self, b):
        self.bytes = bytes(b)

    @property
    def _0(self):
        return self.bytes

    def __eq__(self, o):
        return isinstance(o, Hash) and self.bytes == o.bytes

    def __hash__(self):
        return hash(self.bytes)

    @staticmethod
    def from_bytes(data: bytes):
        return Hash(default_engine().hash_bytes(bytes(data)))

    @staticmethod
    def from_field_elements(elements):
        b = b"".join(int(e).to_bytes(8, "little") for e in elements)    # hash.rs:32-35
        return Hash.from_bytes(b)

    @staticmethod
    def from_u64(value):
        return Hash.from_bytes(int(value).to_bytes(8, "little"))

    @staticmethod
    def combine(left, right):
        return Hash(bytes(default_engine().hash_combine_pairs(np.frombuffer(left.bytes + right.bytes, dtype=np.uint8))[0]))

    def to_hex(self):
        return self.bytes.hex()


class MerkleTree:
    """src/merkle.rs:4-97; the tree lives on the device."""

    def __init__(self, leaves):
        arr = np.frombuffer(b"".join(h.bytes for h in leaves), dtype=np.uint8).reshape(-1, 32) if leaves else np.zeros((0, 32), np.uint8)
        self._t = default_engine().merkle_new(arr)
        self.leaves = list(leaves)
        self.root = Hash(self._t.root())

    new = classmethod(lambda cls, leaves: cls(leaves))

    @property
    def nodes(self):
        """`nodes` of merkle.rs:6: every level, leaves first."""
        lv, n, out = 0, len(self.leaves), []
        while n >= 1:
            out.append([Hash(bytes(r)) for r in self._t.level(lv)])
            lv, n = lv + 1, n // 2
        return out

    def get_root(self):
        return self.root

    @staticmethod
    def commit(leaves):
        arr = np.frombuffer(b"".join(h.bytes for h in leaves), dtype=np.uint8).reshape(-1, 32) if leaves else np.zeros((0, 32), np.uint8)
        return Hash(default_engine().merkle_commit(arr))

    def open(self, index):
        return [Hash(p) for p in self._t.open(index)]

    @staticmethod
    def verify(leaf, index, proof, root):
        cur, idx = leaf, index                                          # merkle.rs:82-96
        for sib in proof:
            cur = Hash.combine(cur, sib) if idx % 2 == 0 else Hash.combine(sib, cur)
            idx //= 2
        return cur == root


class FiatShamir:
    """src/fiat_shamir.rs:4-26"""

    def __init__(self):
        self.transcript = bytearray()

    new = classmethod(lambda cls: cls())

    def absorb(self, data: bytes):
        self.transcript += bytes(data)

    def challenge(self, field):
        h = default_engine().hash_bytes(bytes(self.transcript))
        return field.new_element(int.from_bytes(h[:8], "little"))      # unreduced (H6)

    # proof-of-work grinding (include/stark_mi.h, "Grinding"; no reference counterpart)
    def grind(self, bits, max_tries=0):
        """the smallest nonce whose hash with the transcript has `bits` low zero bits in its check word: found on the GPU
        (smi_dev_grind), absorbed as 8 little-endian bytes, returned"""
        nonce = default_engine().grind(bytes(self.transcript), bits, max_tries)
        self.absorb(nonce.to_bytes(8, "little"))
        return nonce

    def check_grind(self, nonce, bits):
        """pow_ok of `nonce` on the transcript as it stands (smi_grind_check, host only); absorbs nothing"""
        from .engine import grind_check
        return grind_check(bytes(self.transcript), nonce, bits)


class ProofObject:
    """src/stream.rs:8-14"""
    MERKLE_ROOT, FIELD_ELEMENT, FIELD_ELEMENTS, MERKLE_PATH = 0, 1, 2, 3

    def __init__(self, tag, payload):
        self.tag, self.payload = tag, payload

    def __repr__(self):
        return f"ProofObject({self.tag}, ...)"


class ProofStream:
    """src/stream.rs:4-168 (wire format: tags 0-3, LE u64 lengths/values, raw 32-byte digests)."""

    def __init__(self):
        self.objects = []

    new = classmethod(lambda cls: cls())

    def push(self, obj):
        self.objects.append(obj)

    def pop(self):
        return self.objects.pop(0) if self.objects else None

    def serialize(self) -> bytes:
        out = bytearray()
        for o in self.objects:
            out.append(o.tag)
            if o.tag == 0:
                out += o.payload.bytes
            elif o.tag == 1:
                out += int(o.payload.value).to_bytes(8, "little")
            elif o.tag == 2:
                out += len(o.payload).to_bytes(8, "little")
                for fe in o.payload:
                    out += int(fe.value).to_bytes(8, "little")
            else:
                out += len(o.payload).to_bytes(8, "little")
                for h in o.payload:
                    out += h.bytes
        return bytes(out)

    @staticmethod
    def deserialize(data: bytes, field):
        s, i, n = ProofStream(), 0, len(data)
        while i < n:
            tag = data[i]
            i += 1
            if tag == 0:
                if i + 32 <= n:
                    s.push(ProofObject(0, Hash(data[i:i + 32])))
                    i += 32
            elif tag == 1:
                if i + 8 <= n:
                    s.push(ProofObject(1, field.new_element(int.from_bytes(data[i:i + 8], "little"))))
                    i += 8
            elif tag == 2:
                if i + 8 <= n:
                    cnt = int.from_bytes(data[i:i + 8], "little")
                    i += 8
                    fes = []
                    for _ in range(min(cnt, (n - i) // 8)):
                        fes.append(field.new_element(int.from_bytes(data[i:i + 8], "little")))
                        i += 8
                    s.push(ProofObject(2, fes))
            elif tag == 3:
                if i + 8 <= n:
                    cnt = int.from_bytes(data[i:i + 8], "little")
                    i += 8
                    path = []
                    for _ in range(min(cnt, (n - i) // 32)):
                        path.append(Hash(data[i:i + 32]))
                        i += 32
                    s.push(ProofObject(3, path))
            else:
                break
        return s


class Fri:
    """src/fri.rs:8-311 (prover side).  Verification stays with the reference's CPU code (it is
    tiny and host-side); the tests use the oracle's restatement of Fri::verify."""

    def __init__(self, omega, offset, domain_length, expansion_factor, num_colinearity_tests):
        self.field = omega.field
        self._eng = self.field.engine()
        self._cfg = self._eng.fri_cfg(omega.value, offset.value, domain_length, expansion_factor, num_colinearity_tests)
        self.omega, self.offset = omega, offset
        self.domain_length, self.expansion_factor, self.num_colinearity_tests = domain_length, expansion_factor, num_colinearity_tests

    new = classmethod(lambda cls, *a: cls(*a))

    def num_rounds(self):
        return self._eng.fri_num_rounds(self._cfg)

    def fold_codeword(self, codeword, alpha, offset, omega):
        out = self._eng.fri_fold(_vals(codeword), alpha.value, offset.value, omega.value)
        return [FieldElement(int(v), self.field) for v in out]

    def eval_domain(self, rnd=0):
        p = self.field.p                                               # fri.rs:158-166
        return [FieldElement(self.offset.value * pow(self.omega.value, (1 << rnd) * i, p) % p, self.field)
                for i in range(self.domain_length >> rnd)]

    def commit(self, initial_codeword, proof_stream, fiat_shamir):
        """fri.rs:105-156: pushes the roots and the last codeword, absorbs the roots, and returns
        the codewords of every round (`Vec<Vec<FieldElement>>`), read back from the device.  The device continues
        whatever fiat_shamir already holds."""
        roots, alphas, run = self._eng.fri_commit_run(self._cfg, _vals(initial_codeword), bytes(fiat_shamir.transcript))
        for r in roots:
            proof_stream.push(ProofObject(0, Hash(bytes(r))))
            fiat_shamir.absorb(bytes(r))
        codewords = [[FieldElement(int(v), self.field) for v in run.codeword(i)] for i in range(len(run))]
        run.free()
        proof_stream.push(ProofObject(2, list(codewords[-1])))
        return codewords

    def prove(self, initial_codeword, fiat_shamir, proof_stream):
        """fri.rs:250-311: fills proof_stream, absorbs the roots into fiat_shamir, returns the
        top-level indices.  The device continues whatever fiat_shamir already holds."""
        proof, top = self._eng.fri_prove(self._cfg, _vals(initial_codeword), bytes(fiat_shamir.transcript))
        for obj in ProofStream.deserialize(proof, self.field).objects:
            proof_stream.push(obj)
            if obj.tag == 0:
                fiat_shamir.absorb(obj.payload.bytes)
        return top


def _fri_verify(self, proof_stream, fiat_shamir, polynomial_values):
    """Fri::verify (src/fri.rs:313-504): host control flow as in the reference; the heavy parts run
    on the device -- leaf hashes and Merkle paths in batches (smi_hash_leaves,
    smi_merkle_verify_batch) and the last-layer interpolation as an inverse NTT instead of the
    reference's O(L^3) Lagrange.  Returns False where the reference prints + returns false."""
    field, p, t = self.field, self.field.p, self.num_colinearity_tests
    eng = self._eng
    omega, offset = self.omega.value, self.offset.value
    R = self.num_rounds()
    roots, alphas = [], []
    for _ in range(R):                                                      # :325-334
        o = proof_stream.pop()
        if o is None or o.tag != ProofObject.MERKLE_ROOT:
            return False
        roots.append(o.payload)
        fiat_shamir.absorb(o.payload.bytes)
        alphas.append(fiat_shamir.challenge(field).value)
    o = proof_stream.pop()                                                   # :337-342
    if o is None or o.tag != ProofObject.FIELD_ELEMENTS:
        return False
    last = [fe.value for fe in o.payload]
    if not roots:
        return False                                                         # "No FRI roots extracted"
    n_last = len(last)
    if n_last == 0 or n_last & (n_last - 1):
        raise StarkMiError(-6, "Number of leaves must be power of 2")       # MerkleTree::new at :353
    if eng.merkle_commit(eng.hash_leaves(last)) != roots[-1].bytes:          # :349-357
        return False
    degree_bound = n_last // self.expansion_factor                            # :360-365
    if degree_bound == 0:
        return False
    last_omega, last_offset = omega, offset
    for _ in range(R - 1):
        last_omega, last_offset = last_omega * last_omega % p, last_offset * last_offset % p
    coeffs = eng.intt(np.array(last, dtype=np.uint64), last_offset) if n_last > 1 else np.array(last, dtype=np.uint64)
    # the iNTT needs last_omega to be the canonical n_last-th root; the round trip below is the
    # reference's own re-evaluation check (:384-390) and fails otherwise
    re_eval = eng.coset_ntt(coeffs, n_last.bit_length() - 1, last_offset)
    if last_omega != eng.prim_nth_root(n_last) or [int(v) for v in re_eval] != last:
        return False
    nz = np.nonzero(coeffs)[0]
    if len(nz) and int(nz[-1]) > degree_bound - 1:                            # :392-397
        return False
    seed = Hash.from_u64(fiat_shamir.challenge(field).value).bytes            # :400-405
    top = self.sample_indices(seed, self.domain_length >> 1, self.domain_length >> (R - 1), t)
    for r in range(R - 1):                                                    # :408-502
        half = self.domain_length >> (r + 1)
        c_idx = [i % half for i in top]
        aa, bb, cc = [], [], []
        for s_ in range(t):
            o = proof_stream.pop()
            if o is None or o.tag != ProofObject.FIELD_ELEMENTS or len(o.payload) != 3:
                return False
            ay, by, cy = (fe.value for fe in o.payload)
            aa.append(ay); bb.append(by); cc.append(cy)
            if r == 0:
                polynomial_values.append((c_idx[s_], field.new_element(ay)))
                polynomial_values.append((c_idx[s_] + half, field.new_element(by)))
            ax = offset * pow(omega, c_idx[s_], p) % p
            bx = offset * pow(omega, c_idx[s_] + half, p) % p
            cx = alphas[r]                                                    # unreduced, like :452
            # test_colinearity (:507-525): (y1-y0)(x2-x0) == (y2-y0)(x1-x0)
            if ((p + by - ay) % p) * ((p + cx - ax) % p) % p != ((p + cy - ay) % p) * ((p + bx - ax) % p) % p:
                return False
        paths = []
        for _ in range(3 * t):
            o = proof_stream.pop()
            if o is None or o.tag != ProofObject.MERKLE_PATH:
                return False
            paths.append(b"".join(h.bytes for h in o.payload))
        for vals, idxs, sel, root in ((aa, c_idx, 0, roots[r]), (bb, [i + half for i in c_idx], 1, roots[r]),
                                      (cc, c_idx, 2, roots[r + 1])):
            mine = [paths[3 * i + sel] for i in range(t)]
            depth = len(mine[0]) // 32 if mine else 0
            if any(len(m_) != depth * 32 for m_ in mine):
                return False
            ok = eng.merkle_verify_batch(eng.hash_leaves(vals), idxs, np.frombuffer(b"".join(mine), dtype=np.uint8), root.bytes)
            if not ok.all():
                return False
        omega, offset = omega * omega % p, offset * offset % p
    return True


def _fri_sample_indices(self, seed, size, reduced_size, number):
    """Fri::sample_indices (src/fri.rs:176-213); digests come from the device hash kernel."""
    if number > 2 * reduced_size:
        raise StarkMiError(-12, "not enough entropy in indices wrt last codeword")
    if number > reduced_size:
        raise StarkMiError(-13, "cannot sample more indices than available in last codeword")
    indices, reduced, counter = [], [], 0
    while len(indices) < number:
        h = Hash.from_bytes(bytes(seed) + counter.to_bytes(4, "little")).bytes
        index = int.from_bytes(h[24:], "big") % size                          # sample_index, :168-174
        counter += 1
        if index % reduced_size not in reduced:
            indices.append(index)
            reduced.append(index % reduced_size)
    return indices


Fri.verify = _fri_verify
Fri.sample_indices = _fri_sample_indices


class Trace:
    """src/trace.rs:3-50"""

    def __init__(self, trace):
        self.trace = [list(r) for r in trace]
        self.num_columns = len(self.trace[0])

    new = classmethod(lambda cls, t: cls(t))

    def get_row(self, i):
        return self.trace[i] if 0 <= i < len(self.trace) else None

    def get_col(self, j):
        return [r[j] for r in self.trace]

    def get(self, i, j):
        try:
            return self.trace[i][j]
        except IndexError:
            return None

    def to_field_elements(self, field):
        return [[field.new_element(e & 0xFFFFFFFFFFFFFFFF) for e in r] for r in self.trace]   # `e as u64`, unreduced

    @staticmethod
    def fibonacci(length):
        a, b, rows = 1, 1, []
        for _ in range(length):
            rows.append([a])
            a, b = b, a + b
        return Trace(rows)

    def lde(self, field, log_blowup, lde_offset=None):
        """Build-defined: column-major low-degree extension of the whole trace on
        the device -- per column interpolate on the trace subgroup, evaluate on the coset."""
        eng = field.engine()
        rows = b"".join(int(v & ((1 << 128) - 1)).to_bytes(16, "little") for r in self.trace for v in r)
        cols = eng.trace_pack(rows, len(self.trace), self.num_columns)
        return eng.lde(cols, log_blowup, 1, lde_offset)


def verify_column_openings(eng, proof: bytes, n_cols, log_n, log_blowup, num_colinearity_tests, column_roots, top_indices):
    """Verifier side of smi_stark_cfg.open_columns (build-defined composition, include/stark_mi.h): the bytes
    after the FRI objects must (1) open every committed column at the layer-0 positions a, b of every
    colinearity test with authentication paths that verify against that column's root (MerkleTree::verify,
    reference src/merkle.rs:82-96, in one device batch per column), and (2) combine, with the Fiat-Shamir
    weights drawn from the column roots (fresh transcript: absorb root c, challenge -- src/fiat_shamir.rs:15-25),
    to the values a and b of the FRI proof's layer-0 triples (src/fri.rs:229-236).  -> bool"""
    p, W, t = eng.p, n_cols, num_colinearity_tests
    N = 1 << (log_n + log_blowup)
    depth, half = log_n + log_blowup, N // 2
    rec, prec = 9 + 8 * W, 9 + 32 * depth
    tail = t * 2 * rec + t * W * 2 * prec
    if len(proof) < tail:
        return False
    fri, ext = proof[:len(proof) - tail], proof[len(proof) - tail:]
    objs = ProofStream.deserialize(fri, FiniteField(p)).objects
    rounds = sum(1 for o in objs if o.tag == 0)
    triples = [o for o in objs if o.tag == 2][1:1 + t]            # after the last codeword: layer 0's t triples
    if len(triples) != t:
        return False
    fs, weights = FiatShamir(), []
    for root in column_roots:
        fs.absorb(bytes(root))
        weights.append(fs.challenge(FiniteField(p)).value % p)
    rows = np.zeros((t, 2, W), dtype=np.uint64)
    for s in range(t):
        for k in range(2):
            r = ext[(2 * s + k) * rec:(2 * s + k + 1) * rec]
            if r[0] != 2 or int.from_bytes(r[1:9], "little") != W:
                return False
            rows[s, k] = np.frombuffer(r[9:], dtype="<u8")
    base = t * 2 * rec
    for c in range(W):
        leaves, idx, paths = [], [], []
        for s in range(t):
            a = top_indices[s] % half
            for k, i in enumerate((a, a + half)):
                rp = ext[base + ((s * W + c) * 2 + k) * prec:base + ((s * W + c) * 2 + k + 1) * prec]
                if rp[0] != 3 or int.from_bytes(rp[1:9], "little") != depth:
                    return False
                leaves.append(int(rows[s, k, c]))
                idx.append(i)
                paths.append(rp[9:])
        digests = eng.hash_leaves(np.array(leaves, dtype=np.uint64))
        if not eng.merkle_verify_batch(digests, idx, np.frombuffer(b"".join(paths), dtype=np.uint8), column_roots[c]).all():
            return False
    for s in range(t):
        for k in range(2):
            acc = sum(weights[c] * int(rows[s, k, c]) for c in range(W)) % p
            if acc != triples[s].payload[k].value % p:
                return False
    return rounds > 0


class Air:
    """An AIR over n_cols trace columns (include/stark_mi.h, "AIR"): boundary points and transition constraints
    written readably, flattened to the C ABI's smi_air, with a pure-Python pointwise evaluator of the composition
    codeword (what a verifier recomputes from opened rows; plain integer arithmetic, the glue side of this mirror).
    The reference has no counterpart: its Trace has no consumer (src/trace.rs).

        air = Air(2)
        air.boundary(0, 0, 1)                                   # column 0 holds 1 in row 0
        air.transition({("next", 0): 1, ("cur", 1): -1})        # a' = b
        air.transition({("next", 1): 1, ("cur", 0): -1, ("cur", 1): -1})

    A monomial is () (a constant), one factor, or a tuple of factors; a factor is ("cur" | "next", column) or
    ("cur" | "next", column, exponent).  Coefficients are integers, reduced mod p when flattened.

    Periodic columns (round constants, selectors, public columns) are part of the statement, not of the trace:

        k = air.periodic([3, 1, 4, 1])                          # row r holds values[r mod 4]; the period is a power of two
        air.transition({("next", 0): 1, ("cur", 0): -1, ("per", k): -1})          # a' = a + k
        air.transition({("next", 1): 1, (("per_next", k), ("cur", 1, 2)): -1})    # b' = k' b^2

    ("per", j[, exponent]) is periodic column j at this row, ("per_next", j[, exponent]) at the next row.  Factors are
    kept symbolic until they are used, so periodic columns may be declared before or after the constraints.

    A constraint may read up to four consecutive rows (include/stark_mi.h, "AIR: transition windows"):

        air = Air(1)
        air.transition({("row", 2, 0): 1, ("row", 1, 0): -1, ("row", 0, 0): -1})  # a[r+2] = a[r+1] + a[r] in one column

    ("row", s, column[, exponent]) is the column at row r + s and ("per_row", s, j[, exponent]) periodic column j there, s = 0 .. 3;
    "cur" / "next" / "per" / "per_next" are s = 0 and 1.  Air.window is 2, or 1 + the largest s used; such an AIR holds on
    the windows that start at rows 0 .. n - window and is proven by the plain DEEP provers (Engine.dev_air_prove(deep=True)).

    A permutation argument (include/stark_mi.h, "Permutation argument"; one per AIR) claims that two lists of row tuples
    are equal as multisets over all rows:

        air.permutation([0, 1], [2, 3])                         # {(c0[r], c1[r])} = {(c2[r], c3[r])}

    With it set, Engine.air_plan / dev_air_prove / air_verify take the smi_*_perm entry points.

    A lookup argument (include/stark_mi.h, "Lookup argument"; one per AIR, and not together with a permutation) claims that
    every row's tuple of some columns occurs among the rows' tuples of other columns, with a trace column of multiplicities:

        air.lookup([0], [1], 2)                                 # every c0[r] is some c1[t]; c2[t] counts them

    With it set the same three take the smi_*_lookup entry points.

    An argument list (include/stark_mi.h, "Argument list") holds up to 8 permutations and lookups, in any mix and order, that
    one proof shows over one committed trace:

        air.add_permutation([0, 1], [2, 3]).add_lookup([4], [5], 6).add_lookup([7], [5], 8)

    With a non-empty air.args the same three take the smi_*_args entry points.  A list does not mix with permutation() /
    lookup(): a single argument is either the one of its own section or a list of one, which give the same proof.

    In a list a tuple member may be a periodic column, ("per", j), and each side may have a selector (include/stark_mi.h,
    "Argument list with selectors and periodic members"):
        flag, rng = 3, air.periodic(range(256))
        air.add_lookup([0], [("per", rng)], 2, sel=flag)         # on the rows with c3 = 1, c0[r] is in 0 .. 255; c2 counts
    A member or selector may also be read one row later, cyclically (include/stark_mi.h, "Argument list: next-row operands"):
    ("next", c) for trace column c, ("next", ("per", j)) for periodic column j:
        air.add_lookup([0, 1, ("next", 0)], [("per", s), ("per", i), ("per", nx)], 2, sel=("per", live))   # a table-driven transition
    A list with such an argument takes the smi_*_xargs entry points; any other list the smi_*_args ones, as before."""

    def __init__(self, n_cols):
        self.n_cols = n_cols
        self._symbolic = []     # [[(coeff, [(kind, index, exp), ...]), ...], ...]
        self.boundaries = []    # [(col, row, value), ...]
        self.periodics = []     # [[value, ...], ...]: a power-of-two number of integers each
        self.perm = None        # ([left columns], [right columns]) once permutation() was called
        self.lookup_arg = None  # ([lookup columns], [table columns], multiplicity column) once lookup() was called
        self.xargs_always = False   # flatten a list without selectors or periodic members to smi_air_xargs all the same (the
                                    # two paths give the same bytes; for comparisons)
        self.args = []          # [("perm", left, right) | ("lookup", columns, table columns, multiplicity column), ...]; with
                                # selectors two more entries (a_sel, b_sel); a member is an int or ("per", j).  A shared
                                # lookup is ("lookups", [columns_0, ..], table columns, multiplicity column, [sel_0, ..], table_sel)

    MAX_WINDOW = 4          # SMI_AIR_MAX_WINDOW

    @staticmethod
    def _shift(kind):
        """the row shift s of a stored factor kind: "cur" / "per" 0, "next" / "per_next" 1, ("row", s) / ("per_row", s) s"""
        return kind[1] if isinstance(kind, tuple) else (1 if kind in ("next", "per_next") else 0)

    @property
    def window(self):
        """S: the rows a constraint may read, max(2, 1 + the largest shift used)"""
        return max([2] + [1 + self._shift(kind) for con in self._symbolic for _, factors in con for kind, _, _ in factors])

    @property
    def constraints(self):
        """[[(coeff, [(var, exp), ...]), ...], ...] with the variable numbering of smi_air under the window S: s W + col, then
        S W + s Q + j; for S = 2 that is col, W + col, 2W + j, 2W + Q + j"""
        W, Q, S = self.n_cols, len(self.periodics), self.window

        def var(kind, idx):
            periodic = (kind[0] if isinstance(kind, tuple) else kind) in ("per", "per_next", "per_row")
            return S * W + self._shift(kind) * Q + idx if periodic else self._shift(kind) * W + idx
        return [[(cf, [(var(kind, idx), e) for kind, idx, e in factors]) for cf, factors in con] for con in self._symbolic]

    def _factor(self, f):
        if f[0] in ("row", "per_row"):
            s = int(f[1])
            if not 0 <= s < self.MAX_WINDOW:
                raise ValueError(f"row shift {s} is outside 0 .. {self.MAX_WINDOW - 1}")
            return (f[0], s), int(f[2]), (f[3] if len(f) > 3 else 1)
        if f[0] not in ("cur", "next", "per", "per_next"):
            raise ValueError(f"unknown factor kind {f[0]!r}")
        return f[0], int(f[1]), (f[2] if len(f) > 2 else 1)

    def periodic(self, values):
        """a periodic column: row r holds values[r mod len(values)]; -> its index j for ("per", j) / ("per_next", j)"""
        values = [int(v) for v in values]
        if not values or len(values) & (len(values) - 1):
            raise ValueError("the period must be a power of two")
        self.periodics.append(values)
        return len(self.periodics) - 1

    def permutation(self, left, right):
        """the multiset of the tuples (T[left[0]][r], ..) over all rows equals that of (T[right[0]][r], ..); 1 .. 8 columns a
        side, the two lists may overlap"""
        left, right = [int(c) for c in left], [int(c) for c in right]
        if len(left) != len(right):
            raise ValueError("a permutation relates tuples of one width")
        if self.perm is not None:
            raise ValueError("one permutation per AIR")
        if self.args:
            raise ValueError("permutation() does not mix with an argument list (add_permutation / add_lookup)")
        if self.lookup_arg is not None:
            raise ValueError("an AIR takes a permutation or a lookup, not both")
        self.perm = (left, right)
        return self

    def lookup(self, cols, table_cols, mult_col):
        """every tuple (T[cols[0]][r], ..) occurs among the tuples (T[table_cols[0]][t], ..); column mult_col holds the
        multiplicities (a duplicated table tuple is credited to its lowest row); 1 .. 8 columns a side, the two lists may
        overlap, mult_col is none of them"""
        cols, table_cols = [int(c) for c in cols], [int(c) for c in table_cols]
        if len(cols) != len(table_cols):
            raise ValueError("a lookup relates tuples of one width")
        if self.lookup_arg is not None:
            raise ValueError("one lookup per AIR")
        if self.args:
            raise ValueError("lookup() does not mix with an argument list (add_permutation / add_lookup)")
        if self.perm is not None:
            raise ValueError("an AIR takes a permutation or a lookup, not both")
        self.lookup_arg = (cols, table_cols, int(mult_col))
        return self

    ARGS_MAX = 8            # SMI_ARGS_MAX

    def _add_arg(self, arg):
        a = len(self.args)
        if self.perm is not None or self.lookup_arg is not None:
            raise ValueError(f"argument {a}: an argument list does not mix with permutation() / lookup()")
        if a >= self.ARGS_MAX:
            raise ValueError(f"argument {a}: an argument list holds at most {self.ARGS_MAX} arguments")
        if len(arg[1]) != len(arg[2]):
            raise ValueError(f"argument {a}: a {'permutation' if arg[0] == 'perm' else 'lookup'} relates tuples of one width")
        if not 1 <= len(arg[1]) <= 8:
            raise ValueError(f"argument {a}: 1 .. 8 columns a side")
        self.args.append(arg)
        return self

    @staticmethod
    def _operand(x, what, none_ok=False):
        """a member or selector of an argument: an int (trace column), ("per", j) (periodic column j), or either of them one
        row later, cyclically: ("next", c) / ("next", ("per", j)) (include/stark_mi.h, "Argument list: next-row operands")"""
        if x is None and none_ok:
            return None
        if isinstance(x, tuple):
            if len(x) == 2 and x[0] == "next" and not (isinstance(x[1], tuple) and x[1][:1] == ("next",)):
                return ("next", Air._operand(x[1], what))
            if len(x) != 2 or x[0] != "per":
                raise ValueError(f"{what}: an operand is a trace column, (\"per\", j), or (\"next\", either), not {x!r} "
                                 "(a next-row operand is spelt (\"next\", c) or (\"next\", (\"per\", j)))")
            return ("per", int(x[1]))
        return int(x)

    def add_permutation(self, left, right, left_sel=None, right_sel=None):
        """appends a permutation argument (see permutation()) to the argument list.  A member is a trace column or ("per", j),
        periodic column j; left_sel / right_sel (a member each, or None) select the rows of a side: with 0 / 1 selectors the
        selected left tuples are a permutation of the selected right tuples (include/stark_mi.h, "Argument list with selectors
        and periodic members")"""
        arg = ("perm", [self._operand(c, "add_permutation") for c in left], [self._operand(c, "add_permutation") for c in right])
        ls, rs = self._operand(left_sel, "left_sel", True), self._operand(right_sel, "right_sel", True)
        return self._add_arg(arg if ls is None and rs is None else arg + (ls, rs))

    def add_lookup(self, cols, table_cols, mult_col, sel=None, table_sel=None):
        """appends a lookup argument (see lookup()) to the argument list.  A member is a trace column or ("per", j); sel selects
        the rows that look up, table_sel the rows of the table; mult_col is a trace column"""
        arg = ("lookup", [self._operand(c, "add_lookup") for c in cols], [self._operand(c, "add_lookup") for c in table_cols], int(mult_col))
        s, ts = self._operand(sel, "sel", True), self._operand(table_sel, "table_sel", True)
        return self._add_arg(arg if s is None and ts is None else arg + (s, ts))

    ARG_MAX_TUPLES = 4      # SMI_ARG_MAX_TUPLES

    def add_lookups(self, tuples, table_cols, mult_col, sels=None, table_sel=None):
        """appends ONE lookup argument whose J = len(tuples) looked-up tuples share the table, the multiplicity column and the
        running sum (include/stark_mi.h, "Shared-table lookups"): on every row each tuples[j] whose selector sels[j] holds
        occurs among the selected table tuples, and mult_col counts the (row, tuple) pairs that hit a table row.  1 .. 4 tuples
        of one width; sels: None, or one member or None per tuple.  One tuple is add_lookup."""
        a = len(self.args)
        tuples = [[self._operand(c, "add_lookups") for c in t] for t in tuples]
        table = [self._operand(c, "add_lookups") for c in table_cols]
        sels = [None] * len(tuples) if sels is None else [self._operand(x, "sels", True) for x in sels]
        if not 1 <= len(tuples) <= self.ARG_MAX_TUPLES:
            raise ValueError(f"argument {a}: a shared lookup has 1 .. {self.ARG_MAX_TUPLES} tuples")
        if len(sels) != len(tuples):
            raise ValueError(f"argument {a}: one selector (or None) per tuple")
        if any(len(t) != len(table) for t in tuples):
            raise ValueError(f"argument {a}: a lookup relates tuples of one width")
        if len(tuples) == 1:
            return self.add_lookup(tuples[0], table, mult_col, sels[0], table_sel)
        if not 1 <= len(table) <= 8:
            raise ValueError(f"argument {a}: 1 .. 8 columns a side")
        if self.perm is not None or self.lookup_arg is not None:
            raise ValueError(f"argument {a}: an argument list does not mix with permutation() / lookup()")
        if a >= self.ARGS_MAX:
            raise ValueError(f"argument {a}: an argument list holds at most {self.ARGS_MAX} arguments")
        self.args.append(("lookups", tuples, table, int(mult_col), sels, self._operand(table_sel, "table_sel", True)))
        return self

    @staticmethod
    def arg_selectors(arg):
        """(a_sel, b_sel) of an entry of Air.args; None: the constant 1.  A shared lookup keeps its selectors per tuple
        (arg[4]): its a_sel is None"""
        if arg[0] == "lookups":
            return (None, arg[5])
        k = 3 if arg[0] == "perm" else 4
        return (arg[k], arg[k + 1]) if len(arg) > k else (None, None)

    @property
    def extended_args(self):
        """does some argument of the list use a selector or a periodic member?  Then the list flattens to smi_air_xargs;
        otherwise to smi_air_args, and callers take the entry points of "Argument list" as before"""
        return any(g[0] == "lookups" or self.arg_selectors(g) != (None, None) or any(isinstance(c, tuple) for c in g[1] + g[2]) for g in self.args)

    def closes(self, p, g, cols, alpha, gamma):
        """z[n-1] * rho[n-1] == 1 for the trace cols under alpha, gamma (four canonical coordinates each); plain Python"""
        left, right = self.perm
        num = den = Ext4([1, 0, 0, 0], p, g)
        a, c = Ext4(alpha, p, g), Ext4(gamma, p, g)
        for r in range(len(cols[0])):
            fl = fr = c
            pw = Ext4([1, 0, 0, 0], p, g)
            for lj, rj in zip(left, right):
                fl, fr = fl + pw * Ext4.embed(int(cols[lj][r]), p, g), fr + pw * Ext4.embed(int(cols[rj][r]), p, g)
                pw = pw * a
            num, den = num * fl, den * fr
        return num == den

    def with_periodic_as_trace(self):
        """-> the AIR over n_cols + Q trace columns that states the same transitions with the periodic columns read as
        trace columns n_cols .. n_cols + Q - 1 (what one had to write before periodic columns, and what they are as
        polynomials).  The boundary points carry over; the extra columns get none."""
        out = Air(self.n_cols + len(self.periodics))
        kind = {"cur": ("cur", 0), "next": ("next", 0), "per": ("cur", self.n_cols), "per_next": ("next", self.n_cols)}
        for s in range(self.MAX_WINDOW):
            kind[("row", s)], kind[("per_row", s)] = (("row", s), 0), (("row", s), self.n_cols)
        out._symbolic = [[(cf, [(kind[k][0], kind[k][1] + i, e) for k, i, e in factors]) for cf, factors in con] for con in self._symbolic]
        out.boundaries = list(self.boundaries)
        return out

    def zk_derived(self, p, log_n, t, trace_offset, omega_n, with_args=False):
        """-> the AIR that a zero-knowledge DEEP proof of this one proves (include/stark_mi.h, "Zero-knowledge DEEP proofs"): one
        more periodic column of period n = 2^log_n holding E(tau w^r), E(x) = prod over the exempt rows q = n - k_t - 1 .. n - 2
        of (x - tau w^q), k_t = 8 t + 8, as one more factor of every transition term.  n k_t products in Python ints.
        with_args: the list form ("... with an argument list") -- k_t = 8 t + 16 and a second column, E_A(tau w^r) with the roots
        q = n - k_t .. n - 1, that no constraint reads; the result carries no argument list (the arguments cover the rows below
        n - k_t and are the prover's to check: "closes")."""
        import copy
        n, kt = 1 << log_n, 8 * t + (16 if with_args else 8)
        pts = [trace_offset * pow(omega_n, r, p) % p for r in range(n)]
        col = []
        for r in range(n):
            v = 1
            for q in range(n - kt - 1, n - 1):
                v = v * (pts[r] - pts[q]) % p
            col.append(v)
        out = copy.deepcopy(self)
        j = out.periodic(col)
        out._symbolic = [[(cf, list(factors) + [("per", j, 1)]) for cf, factors in con] for con in out._symbolic]
        if with_args:
            wk = pow(omega_n, kt, p)
            out.periodic([col[(r - 1) % n] * wk % p for r in range(n)])   # E_A(x w) = w^k_t E(x)
            out.args = []
        return out

    def transition(self, poly):
        terms = []
        for mono, coeff in poly.items():
            if mono == ():
                factors = []
            elif isinstance(mono[0], str):
                factors = [self._factor(mono)]
            else:
                factors = [self._factor(f) for f in mono]
            terms.append((int(coeff), factors))
        self._symbolic.append(terms)
        return self

    def boundary(self, col, row, value):
        self.boundaries.append((int(col), int(row), int(value)))
        return self

    @property
    def degree(self):
        return max([1] + [sum(e for _, e in f) for con in self.constraints for _, f in con])

    def flatten(self, p):
        """-> _lib.Air (smi_air); the arrays it points to stay alive as long as the returned object"""
        import ctypes as C
        from . import _lib
        cft, coeff, tff, var, exp = [0], [], [0], [], []
        for con in self.constraints:
            for cf, factors in con:
                coeff.append(cf % p)
                var += [v for v, _ in factors]
                exp += [e for _, e in factors]
                tff.append(len(var))
            cft.append(len(coeff))
        arrs = [np.array(cft, dtype=np.uint32), np.array(coeff, dtype=np.uint64), np.array(tff, dtype=np.uint32),
                np.array(var, dtype=np.uint32), np.array(exp, dtype=np.uint32),
                np.array([b[0] for b in self.boundaries], dtype=np.uint32), np.array([b[1] for b in self.boundaries], dtype=np.uint64),
                np.array([b[2] for b in self.boundaries], dtype=np.uint64),
                np.array([len(v).bit_length() - 1 for v in self.periodics], dtype=np.uint32),
                np.array([x % p for v in self.periodics for x in v], dtype=np.uint64)]
        ptr = lambda a, t: a.ctypes.data_as(t)
        out = _lib.Air(len(self.constraints), len(coeff), len(var), len(self.boundaries), ptr(arrs[0], _lib.u32p), ptr(arrs[1], _lib.u64p),
                       ptr(arrs[2], _lib.u32p), ptr(arrs[3], _lib.u32p), ptr(arrs[4], _lib.u32p), ptr(arrs[5], _lib.u32p),
                       ptr(arrs[6], _lib.u64p), ptr(arrs[7], _lib.u64p), len(self.periodics), 0 if self.window == 2 else self.window,
                       ptr(arrs[8], _lib.u32p), ptr(arrs[9], _lib.u64p))
        out._keep = arrs
        if self.perm is not None and self.lookup_arg is not None:
            raise ValueError("an AIR takes a permutation or a lookup, not both")
        out.lookup = None
        if self.lookup_arg is not None:
            la, ta = np.array(self.lookup_arg[0], dtype=np.uint32), np.array(self.lookup_arg[1], dtype=np.uint32)
            out.lookup = _lib.AirLookup(len(la), self.lookup_arg[2] % (1 << 32), ptr(la, _lib.u32p), ptr(ta, _lib.u32p))
            out.lookup._keep = (la, ta)
        out.args = out.xargs = None
        if self.extended_args or (self.args and self.xargs_always):
            W = self.n_cols

            def var(c):
                if c is None:
                    return _lib.NO_SELECTOR
                if isinstance(c, tuple) and c[0] == "next":   # SMI_ARG_NEXT_ROW on a this-row variable
                    return _lib.ARG_NEXT_ROW | var(c[1])
                return (2 * W + c[1]) % (1 << 32) if isinstance(c, tuple) else c % (1 << 32)

            keep, raw = [], (_lib.AirXArg * len(self.args))()
            for a, arg in enumerate(self.args):
                if arg[0] == "lookups":   # J m operands, tuple-major, then the J selectors; J - 1 in the second byte of kind
                    J = len(arg[1])
                    la = np.array([var(c) for t in arg[1] for c in t] + [var(x) for x in arg[4]], dtype=np.uint32)
                    ra = np.array([var(c) for c in arg[2]], dtype=np.uint32)
                    keep += [la, ra]
                    raw[a] = _lib.AirXArg(1 | (J - 1) << _lib.ARG_TUPLES_SHIFT, len(ra), arg[3] % (1 << 32), 0, ptr(la, _lib.u32p), ptr(ra, _lib.u32p),
                                          _lib.NO_SELECTOR, var(arg[5]))
                    continue
                la, ra = np.array([var(c) for c in arg[1]], dtype=np.uint32), np.array([var(c) for c in arg[2]], dtype=np.uint32)
                keep += [la, ra]
                sa, sb = self.arg_selectors(arg)
                raw[a] = _lib.AirXArg(0 if arg[0] == "perm" else 1, len(la), (arg[3] % (1 << 32)) if arg[0] == "lookup" else 0, 0, ptr(la, _lib.u32p),
                                      ptr(ra, _lib.u32p), var(sa), var(sb))
            out.xargs = _lib.AirXArgs(len(self.args), 0, raw)
            out.xargs._keep = (keep, raw)
        elif self.args:
            keep, raw = [], (_lib.AirArg * len(self.args))()
            for a, arg in enumerate(self.args):
                la, ra = np.array(arg[1], dtype=np.uint32), np.array(arg[2], dtype=np.uint32)
                keep += [la, ra]
                raw[a] = _lib.AirArg(0 if arg[0] == "perm" else 1, len(la), (arg[3] % (1 << 32)) if arg[0] == "lookup" else 0, 0, ptr(la, _lib.u32p),
                                     ptr(ra, _lib.u32p))
            out.args = _lib.AirArgs(len(self.args), 0, raw)
            out.args._keep = (keep, raw)
        out.perm = None
        if self.perm is not None:
            la, ra = np.array(self.perm[0], dtype=np.uint32), np.array(self.perm[1], dtype=np.uint32)
            out.perm = _lib.AirPerm(len(la), 0, ptr(la, _lib.u32p), ptr(ra, _lib.u32p))
            out.perm._keep = (la, ra)
        return out

    def periodic_row(self, p, r):
        """the periodic columns' values in trace row r"""
        return [v[r % len(v)] % p for v in self.periodics]

    def periodic_at(self, p, log_n, trace_offset, omega_n, x):
        """pi_j(x) for every periodic column, from the definition: pi_j(x) = q_j((x / tau)^(n / P_j)) with q_j the Lagrange
        interpolant of the P_j values on the powers of omega_n^(n / P_j) (P_j inversions per column and point: for
        small periods or small n)"""
        inv = lambda v: pow(v, p - 2, p)
        n, out = 1 << log_n, []
        for v in self.periodics:
            P = len(v)
            y = pow(x * inv(trace_offset) % p, n // P, p)
            w = pow(omega_n, n // P, p)
            # q(y) = (y^P - 1) / P * sum_r v_r w^r / (y - w^r); y is never a P-th root of unity off the trace domain
            zp, acc, wr = (pow(y, P, p) - 1) % p, 0, 1
            if zp == 0:
                r = next(r for r in range(P) if pow(w, r, p) == y)
                out.append(v[r] % p)
                continue
            for r in range(P):
                acc += v[r] % p * wr % p * inv((y - wr) % p)
                wr = wr * w % p
            out.append(acc % p * zp % p * inv(P % p) % p)
        return out

    def constraint_value(self, k, p, cur, nxt, per_cur=(), per_nxt=()):
        """C_k on one row pair; per_cur / per_nxt: the periodic columns' values at this row and the next"""
        vals = [int(v) for v in cur] + [int(v) for v in nxt] + [int(v) for v in per_cur] + [int(v) for v in per_nxt]
        acc = 0
        for cf, factors in self.constraints[k]:
            m = cf % p
            for v, e in factors:
                m = m * pow(vals[v], e, p) % p
            acc += m
        return acc % p

    def constraint_value_window(self, k, p, rows, per_rows=()):
        """C_k on one window: rows[s] the trace columns' values at row r + s, per_rows[s] the periodic columns' there, s < window"""
        S = self.window
        vals = [int(v) for s in range(S) for v in rows[s]] + [int(v) for s in range(S) for v in (per_rows[s] if per_rows else ())]
        acc = 0
        for cf, factors in self.constraints[k]:
            m = cf % p
            for v, e in factors:
                m = m * pow(vals[v], e, p) % p
            acc += m
        return acc % p

    def first_violation(self, p, cols):
        """(constraint, row) of the first violation on a trace in smi_dev_air_check's order, or None; a constraint holds on
        the windows that start at rows 0 .. n - window"""
        n, S = len(cols[0]), self.window
        for j, (c, r, v) in enumerate(self.boundaries):
            if int(cols[c][r]) != v % p:
                return j, r
        for k in range(len(self.constraints)):
            for r in range(n - S + 1):
                if self.constraint_value_window(k, p, [[col[r + s] for col in cols] for s in range(S)],
                                                [self.periodic_row(p, r + s) for s in range(S)]):
                    return len(self.boundaries) + k, r
        return None

    def compose_at(self, p, log_n, log_blowup, trace_offset, lde_offset, omega_N, i, cur, nxt, weights, per_cur=None, per_nxt=None):
        """cw[i] from the extended columns' values at index i (cur) and (i + B) mod N (nxt; unused when there is no
        transition constraint) under the W + K unreduced weights -- the definition of include/stark_mi.h, term by term.
        per_cur / per_nxt: pi_j(x_i) and pi_j(w x_i) of the periodic columns; left out, they are evaluated here from the
        definition (periodic_at), which is for small periods or small n"""
        n, B = 1 << log_n, 1 << log_blowup
        inv = lambda v: pow(v, p - 2, p)
        w = pow(omega_N, B, p)
        x = lde_offset * pow(omega_N, i, p) % p
        acc = 0
        for c in range(self.n_cols):
            pts = [(trace_offset * pow(w, r, p) % p, v % p) for (cc, r, v) in self.boundaries if cc == c]
            term = int(cur[c])
            if pts:
                ix, z = 0, 1
                for j, (rj, vj) in enumerate(pts):     # Lagrange form of the interpolant at x
                    num, den = 1, 1
                    for k, (rk, _) in enumerate(pts):
                        if k != j:
                            num, den = num * (x - rk) % p, den * (rj - rk) % p
                    ix += vj * num * inv(den)
                    z = z * (x - rj) % p
                term = (term - ix) * inv(z) % p
            acc += weights[c] % p * term
        if self.constraints:
            last = trace_offset * pow(w, n - 1, p) % p
            zt_inv = (x - last) * inv(pow(x, n, p) - pow(trace_offset, n, p)) % p
            if self.periodics and per_cur is None:
                per_cur = self.periodic_at(p, log_n, trace_offset, w, x)
            if self.periodics and per_nxt is None:
                per_nxt = self.periodic_at(p, log_n, trace_offset, w, x * w % p)
            for k in range(len(self.constraints)):
                acc += weights[self.n_cols + k] % p * (self.constraint_value(k, p, cur, nxt, per_cur or (), per_nxt or ()) * zt_inv % p)
        return acc % p
