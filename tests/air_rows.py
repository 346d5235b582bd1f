"""The checker of the row-committed AIR proofs (smi_dev_air_prove_rows / smi_air_verify_rows), from the CPU oracle's
primitives only: the row leaves and their tree, the transcript of include/stark_mi.h ("AIR over one row-committed
tree"), the opening section restated record by record and the lengths of both proof variants.
Not a test module: imported by tests/test_air_rows_emu.py and tests/test_gpu_air_rows.py."""
import numpy as np


def _u64(v):
    return int(v).to_bytes(8, "little")


def row_leaves(o, lde_cols):
    """leaf i = Hash::from_field_elements([col_0[i] .. col_{W-1}[i]]) -> (N, 32) uint8"""
    return o.row_hashes(np.ascontiguousarray(np.array(lde_cols, dtype=np.uint64)))


def transcript(o, n_cols, n_constraints, root):
    """-> (the 32 + 8 (W + K) transcript bytes FRI continues, the W + K weights): the root, then every j < W + K as 8
    little-endian bytes with a challenge after each; every challenge is Hash::from_bytes of the whole transcript so far"""
    tr, wts = bytearray(bytes(root)), []
    for j in range(n_cols + n_constraints):
        tr += _u64(j)
        wts.append(int.from_bytes(o.hash_from_bytes(bytes(tr))[:8], "little"))
    return bytes(tr), wts


def positions(s, N, B, with_next):
    a = int(s) % (N // 2)
    return [a, a + N // 2] + ([(a + B) % N, (a + N // 2 + B) % N] if with_next else [])


def openings_bytes(o, lde_cols, top, N, B, with_next, nodes=None):
    """per test the rows at a, b (and (a+B) mod N, (b+B) mod N when there are transition constraints), then per test one
    MerklePath of the single tree per opened position in the same order"""
    W = len(lde_cols)
    nodes = o.merkle_new(row_leaves(o, lde_cols)) if nodes is None else nodes
    out = bytearray()
    for s in top:
        for i in positions(s, N, B, with_next):
            out += b"\x02" + _u64(W) + b"".join(_u64(col[i]) for col in lde_cols)
    for s in top:
        for i in positions(s, N, B, with_next):
            path = o.merkle_open(nodes, N, i)
            out += b"\x03" + _u64(len(path)) + b"".join(bytes(d) for d in path)
    return bytes(out)


def opening_len(W, K, log_N, t):
    R = 4 if K else 2
    return t * R * (9 + 8 * W) + t * R * (9 + 32 * log_N)


def column_opening_len(W, K, log_N, t):
    R = 4 if K else 2
    return t * R * (9 + 8 * W) + t * W * R * (9 + 32 * log_N)


def split(proof, W, K, log_N, t):
    """-> (the FRI objects, the opening section) of a row-committed proof"""
    ob = opening_len(W, K, log_N, t)
    return proof[:len(proof) - ob], proof[len(proof) - ob:]


def wide(W, K, p, n, seed=13):
    """a satisfiable AIR of any width: columns c < K follow x' = x * y + (c + 1) with y the column after c (degree 2, so FRI
    runs at the full blowup), the others are random; boundary points on column 0 and on the last column"""
    from stark_rs_amd.mirror import Air
    assert K <= W - 1 or W == 1
    rng = np.random.default_rng(seed)
    cols = [[int(x) for x in rng.integers(0, p, n)] for _ in range(W)]
    air = Air(W)
    for c in range(K - 1, -1, -1):           # column c reads column c + 1, so build from the last constrained one down
        y = cols[c + 1] if W > 1 else cols[0]
        x = [cols[c][0]]
        for r in range(n - 1):
            x.append((x[-1] * y[r] + c + 1) % p)
        cols[c] = x
    for c in range(K):
        air.transition({("next", c): 1, (("cur", c), ("cur", (c + 1) % W)): -1, (): -(c + 1)})
    air.boundary(0, 0, cols[0][0]).boundary(W - 1, n - 1, cols[W - 1][n - 1])
    return air, cols
