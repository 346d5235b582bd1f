// mgpu_core.h -- device-side pieces of the multi-GPU prover that the HIP kernels (mgpu.hip) and
// the CPU emulator of the non-GPU tests (emu_mgpu.cpp) share: how an opening of a sharded
// codeword is served and written into the serialized proof.
//
// One codeword of length `len` is split in contiguous blocks of `blk` elements, rank g holding
// [g*blk, (g+1)*blk) and the complete Merkle subtree over it (a power-of-two aligned leaf block is
// a subtree of MerkleTree::new, reference src/merkle.rs:21-31); the G sub-roots are all-gathered
// and every rank holds the log2 G levels above them (`top`).  An opening (value + authentication
// path, Fri::query src/fri.rs:215-248, MerkleTree::open src/merkle.rs:67-80) is written by the
// rank that owns the leaf; everything replicated (tags, lengths, roots, the last codeword) by
// rank 0; the proof buffer starts zeroed on every rank, so a byte-wise sum over the ranks
// (all-reduce) assembles the reference's serialization (src/stream.rs:35-64) on all of them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "field.h"

struct MgSide {            // one round's codeword and tree as THIS rank holds them
    const uint32_t *cw;    // the local block (the whole codeword when the round is replicated)
    const uint8_t *nodes;  // all levels of the tree over the local block, level 0 first
    const uint8_t *top;    // all levels of the tree over the G sub-roots (sharded rounds), else unused
    uint64_t len;          // length of the round's whole codeword
    uint64_t blk;          // length of the local block (== len when replicated)
    uint32_t depth_local;  // log2 blk
    uint32_t depth_top;    // log2 G for a sharded round, 0 otherwise
};
struct MgLayer {           // one FRI layer of the query phase (src/fri.rs:280-308)
    MgSide cur, next;
    uint64_t off_triples;  // byte offset of this layer's first FieldElements triple
    uint64_t off_paths;    // byte offset of this layer's first MerklePath
};

SMI_HD void mg_put_u64(uint8_t *p, uint64_t v) {
    for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}

// Value slot (8 bytes LE) and path (tag 3, u64 count, 32-byte digests) of leaf `index` of `side`.
// lane / n_lanes: the caller's cooperative threads (n_lanes >= 32 on the device, 1 in the emulator).
SMI_HD void mg_open_write(const MgSide &side, uint64_t index, int rank, uint8_t *value_slot, uint8_t *path_slot, uint32_t lane,
                          uint32_t n_lanes) {
    const uint32_t depth = side.depth_local + side.depth_top;
    if (rank == 0 && lane == 0) {            // replicated bytes: rank 0
        path_slot[0] = 3;
        mg_put_u64(path_slot + 1, depth);
    }
    const uint64_t owner = side.depth_top ? index / side.blk : 0;
    if ((uint64_t)rank != owner) return;
    const uint64_t local = index - owner * side.blk;
    if (lane == 0) mg_put_u64(value_slot, side.cw[local]);
    uint64_t idx = local, lvl_off = 0, n = side.blk;
    for (uint32_t l = 0; l < side.depth_local; l++) {          // inside the resident subtree
        const uint64_t sib = idx ^ 1;
        for (uint32_t b = lane; b < 32; b += n_lanes) path_slot[9 + 32 * l + b] = side.nodes[(lvl_off + sib) * 32 + b];
        idx >>= 1;
        lvl_off += n;
        n >>= 1;
    }
    idx = owner;
    lvl_off = 0;
    n = (uint64_t)1 << side.depth_top;
    for (uint32_t l = 0; l < side.depth_top; l++) {            // above the sub-roots (replicated levels)
        const uint64_t sib = idx ^ 1;
        for (uint32_t b = lane; b < 32; b += n_lanes)
            path_slot[9 + 32 * (side.depth_local + l) + b] = side.top[(lvl_off + sib) * 32 + b];
        idx >>= 1;
        lvl_off += n;
        n >>= 1;
    }
}

// Test s of layer L: the triple (a, b, c) and the three paths, src/fri.rs:229-243.
SMI_HD void mg_query_write(const MgLayer &L, uint64_t top_index, uint32_t s, int rank, uint8_t *proof, uint32_t lane, uint32_t n_lanes) {
    const uint64_t half = L.cur.len / 2;
    const uint64_t c = top_index % half;     // indices folded layer by layer: (x % a) % b == x % b for b | a
    uint8_t *tr = proof + L.off_triples + (uint64_t)s * 33;
    if (rank == 0 && lane == 0) {
        tr[0] = 2;
        mg_put_u64(tr + 1, 3);
    }
    const uint64_t pa = 9 + 32ull * (L.cur.depth_local + L.cur.depth_top), pc = 9 + 32ull * (L.next.depth_local + L.next.depth_top);
    uint8_t *pp = proof + L.off_paths + (uint64_t)s * (2 * pa + pc);
    mg_open_write(L.cur, c, rank, tr + 9, pp, lane, n_lanes);
    mg_open_write(L.cur, c + half, rank, tr + 17, pp + pa, lane, n_lanes);
    mg_open_write(L.next, c, rank, tr + 25, pp + 2 * pa, lane, n_lanes);
}

// Column openings of the build-defined composition (smi_stark_cfg.open_columns): what ties the codeword FRI
// proves low-degree to the W committed columns.  For test s: a = top mod N/2, b = a + N/2;
//   rows : t x 2 records  tag 2 | u64 W | W x u64            (row a, then row b)
//   paths: t x W x 2 records  tag 3 | u64 depth | depth x 32  (column c at a, then at b)
// written like the FRI openings: values and digests by the rank that owns the leaf, tags by rank 0.
SMI_HD uint64_t mg_column_open_bytes(uint32_t W, uint32_t t, uint32_t depth, uint32_t R = 2) {
    return (uint64_t)t * R * (9 + 8ull * W) + (uint64_t)t * W * R * (9 + 32ull * depth);
}
// The same records at R positions per test.  R == 2: a, b (open_columns).  R == 4: a, b, (a + shift) mod N, (b + shift) mod N
// -- the AIR prover's next-row openings (smi_dev_air_prove, shift = the blowup): rows t x R, paths t x W x R, same order.
SMI_HD void mg_column_open_write_n(const MgSide *cols, uint32_t W, uint32_t c, uint64_t top_index, uint32_t s, uint32_t t, int rank,
                                   uint8_t *out, uint32_t lane, uint32_t n_lanes, uint32_t R, uint64_t shift) {
    const MgSide &side = cols[c];
    const uint32_t depth = side.depth_local + side.depth_top;
    const uint64_t half = side.len / 2, a = top_index % half, rec = 9 + 8ull * W, prec = 9 + 32ull * depth;
    const uint64_t pos[4] = {a, a + half, (a + shift) & (side.len - 1), (a + half + shift) & (side.len - 1)};
    uint8_t *rows = out + (uint64_t)s * R * rec;
    uint8_t *paths = out + (uint64_t)t * R * rec + ((uint64_t)s * W + c) * R * prec;
    if (rank == 0 && c == 0 && lane == 0)
        for (uint32_t k = 0; k < R; k++) {
            rows[k * rec] = 2;
            mg_put_u64(rows + k * rec + 1, W);
        }
    for (uint32_t k = 0; k < R; k++) mg_open_write(side, pos[k], rank, rows + k * rec + 9 + 8ull * c, paths + k * prec, lane, n_lanes);
}
SMI_HD void mg_column_open_write(const MgSide *cols, uint32_t W, uint32_t c, uint64_t top_index, uint32_t s, uint32_t t, int rank,
                                 uint8_t *out, uint32_t lane, uint32_t n_lanes) {
    mg_column_open_write_n(cols, W, c, top_index, s, t, rank, out, lane, n_lanes, 2, 0);
}

// Row openings of ONE tree over the rows of W columns (smi_dev_air_prove_rows): the rows as above, then one path per
// opened position instead of one per (position, column):
//   rows : t x R records  tag 2 | u64 W | W x u64
//   paths: t x R records  tag 3 | u64 depth | depth x 32       (test s, inside it the positions in the rows' order)
// Single device: the tree (`nodes`, every level back to back, N = 2^depth leaves) and the columns (`stride` apart) are whole.
SMI_HD uint64_t mg_row_open_bytes(uint32_t W, uint32_t t, uint32_t depth, uint32_t R) {
    return (uint64_t)t * R * (9 + 8ull * W) + (uint64_t)t * R * (9 + 32ull * depth);
}
// record k (position k of a, b, (a + shift) mod N, (b + shift) mod N) of test s, by n_lanes cooperating lanes
SMI_HD void mg_row_open_write(const uint32_t *cols, uint64_t stride, uint32_t W, const uint8_t *nodes, uint32_t depth, uint64_t top_index,
                              uint32_t s, uint32_t k, uint32_t t, uint8_t *out, uint32_t lane, uint32_t n_lanes, uint32_t R, uint64_t shift) {
    const uint64_t N = 1ull << depth, half = N / 2, a = top_index % half, rec = 9 + 8ull * W, prec = 9 + 32ull * depth;
    const uint64_t pos = ((k & 1 ? a + half : a) + (k & 2 ? shift : 0)) & (N - 1);
    uint8_t *row = out + ((uint64_t)s * R + k) * rec;
    uint8_t *path = out + (uint64_t)t * R * rec + ((uint64_t)s * R + k) * prec;
    if (lane == 0) {
        row[0] = 2;
        mg_put_u64(row + 1, W);
        path[0] = 3;
        mg_put_u64(path + 1, depth);
    }
    for (uint32_t c = lane; c < W; c += n_lanes) mg_put_u64(row + 9 + 8ull * c, cols[c * stride + pos]);
    for (uint32_t q = lane; q < 32 * depth; q += n_lanes) {   // byte q & 31 of the sibling on level q >> 5 (level l starts at 2N - (2N >> l))
        const uint32_t l = q >> 5;
        const uint64_t sib = (pos >> l) ^ 1;
        path[9 + q] = nodes[(2 * N - ((2 * N) >> l) + sib) * 32 + (q & 31)];
    }
}

// The same section for the AIR proof over FRI at folding factor 4 (include/stark_mi.h, "Extension FRI, folding factor 4"):
// record k of test s is the row at a + (k & 3) N / 4, a = top mod N / 4 -- the four points of the layer-0 coset --, and for
// k >= 4 (R == 8) the row `shift` further, mod N.  Layout and lengths as above (mg_row_open_bytes with R = 4 or 8).
SMI_HD void mg_row_open4_write(const uint32_t *cols, uint64_t stride, uint32_t W, const uint8_t *nodes, uint32_t depth, uint64_t top_index,
                               uint32_t s, uint32_t k, uint32_t t, uint8_t *out, uint32_t lane, uint32_t n_lanes, uint32_t R, uint64_t shift) {
    const uint64_t N = 1ull << depth, q = N / 4, a = top_index % q, rec = 9 + 8ull * W, prec = 9 + 32ull * depth;
    const uint64_t pos = (a + (k & 3) * q + (k & 4 ? shift : 0)) & (N - 1);
    uint8_t *row = out + ((uint64_t)s * R + k) * rec;
    uint8_t *path = out + (uint64_t)t * R * rec + ((uint64_t)s * R + k) * prec;
    if (lane == 0) {
        row[0] = 2;
        mg_put_u64(row + 1, W);
        path[0] = 3;
        mg_put_u64(path + 1, depth);
    }
    for (uint32_t c = lane; c < W; c += n_lanes) mg_put_u64(row + 9 + 8ull * c, cols[c * stride + pos]);
    for (uint32_t b = lane; b < 32 * depth; b += n_lanes) {
        const uint32_t l = b >> 5;
        const uint64_t sib = (pos >> l) ^ 1;
        path[9 + b] = nodes[(2 * N - ((2 * N) >> l) + sib) * 32 + (b & 31)];
    }
}

// Openings of a tree of coset leaves (include/stark_mi.h, "Out-of-domain sampling over coset leaves"): the section of one
// group of V columns follows a fold-by-4 FRI layer --
//   records: t x  tag 2 | u64 4 V | 4 V x u64      (test s: leaf a = top_s mod N / 4, value 4 c + j = column c at a + j N / 4)
//   paths  : t x  tag 3 | u64 depth | depth x 32   (depth = log2 N - 2, the siblings of leaf a from the leaves up)
// The groups of one proof travel as a table (coset_open_kernel's argument, deep.hip): where the columns and the tree of
// N / 4 leaves are, and where the group's section starts in the output.
struct MgCosetGroup {
    const uint32_t *cols;
    uint64_t stride;
    const uint8_t *nodes;
    uint64_t out_at;
    uint32_t V, reserved0;
};
struct MgCosetTable {
    MgCosetGroup g[3];
};
SMI_HD uint64_t mg_coset_open_bytes(uint32_t V, uint32_t t, uint32_t log_N) {
    return (uint64_t)t * (9 + 32ull * V) + (uint64_t)t * (9 + 32ull * (log_N - 2));
}
// the record and the path of test s of one group, by n_lanes cooperating lanes; out: the start of the group's section
SMI_HD void mg_coset_open_write(const MgCosetGroup &G, uint32_t log_N, uint64_t top_index, uint32_t s, uint32_t t, uint8_t *out, uint32_t lane,
                                uint32_t n_lanes) {
    const uint32_t depth = log_N - 2, cnt = 4 * G.V;
    const uint64_t q = 1ull << depth, a = top_index % q, rec = 9 + 8ull * cnt, prec = 9 + 32ull * depth;
    uint8_t *row = out + (uint64_t)s * rec;
    uint8_t *path = out + (uint64_t)t * rec + (uint64_t)s * prec;
    if (lane == 0) {
        row[0] = 2;
        mg_put_u64(row + 1, cnt);
        path[0] = 3;
        mg_put_u64(path + 1, depth);
    }
    for (uint32_t i = lane; i < cnt; i += n_lanes) mg_put_u64(row + 9 + 8ull * i, G.cols[(uint64_t)(i >> 2) * G.stride + a + (uint64_t)(i & 3) * q]);
    for (uint32_t b = lane; b < 32 * depth; b += n_lanes) {   // byte b & 31 of the sibling on level b >> 5 (level l starts at 2 q - (2 q >> l))
        const uint32_t l = b >> 5;
        const uint64_t sib = (a >> l) ^ 1;
        path[9 + b] = G.nodes[(2 * q - ((2 * q) >> l) + sib) * 32 + (b & 31)];
    }
}

// column_open_kernel on the context's stream (stark.hip; mgpu.hip and air.hip call it too)
struct smi_ctx;
int launch_column_open(smi_ctx *ctx, const MgSide *d_cols, uint32_t W, const uint64_t *d_top, uint32_t t, int rank, uint8_t *d_out);
