// merkle_plan.h -- host-side planning of the Merkle launches, shared by the HIP launcher (hash.hip), the FRI round
// plan (fri_plan.h) and the CPU emulator of the non-GPU tests (emu.cpp).  No HIP in here: what a tree costs in
// launches, and what its first launch can do with leaves that are computed instead of read, is decided by
// merkle_plan() alone and executed step by step by launch_merkle_impl.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#ifndef SMI_HASH_THREADS
#define SMI_HASH_THREADS 256   // tuning builds: -DSMI_HASH_THREADS=128 | 512
#endif
#define SMI_TOP_MAX 2048       // digests one chunk workgroup finishes (11 levels)

inline bool is_pow2(uint64_t n) { return n && !(n & (n - 1)); }
inline uint32_t ilog2(uint64_t n) {   // floor
    uint32_t l = 0;
    while ((n >> l) > 1) l++;
    return l;
}

// The SMI_MERKLE_* tuning knobs (tools/*.sh)
struct MerkleKnobs {
    uint32_t k;          // K: levels per subtree launch, 1..3 (LDS stash = 8 KB << K); default 2
    size_t top_blocks;   // TOP_BLOCKS: chunk workgroups per launch below which the chunk kernel takes over (one per CU); 256
    uint32_t elems_log;  // ELEMS_LOG: a tree of elements goes to the chunk kernel only with at most 2^ELEMS_LOG leaves; 19
    size_t single;       // SINGLE: up to this many digests stay one chunk; 512
    size_t minchunk;     // MINCHUNK: smallest chunk otherwise; 64
    bool fuse;           // FUSE: leaves computed by the launch that hashes them, fold at the head of the FRI tail; 1
    bool generic;        // GENERIC: no straight-line K == 2 instantiations; 0
    // A chunk's first level over elements is leaf hashing by single lanes, nine mixes per leaf, which the
    // four-leaves-per-lane kernel does at twice the rate even when it fills a quarter of the chip.
    size_t elems_max() const {
        const size_t v = (size_t)1 << elems_log, by_blocks = SMI_TOP_MAX * top_blocks;
        return v < by_blocks ? v : by_blocks;
    }
};
inline MerkleKnobs merkle_knobs_make(long k, long top_blocks, long elems_log, long single, long minchunk, long fuse, long generic) {
    return MerkleKnobs{(uint32_t)(k < 1 ? 1 : (k > 3 ? 3 : k)), (size_t)top_blocks, (uint32_t)elems_log, (size_t)single, (size_t)minchunk,
                       fuse != 0, generic != 0};
}
inline const MerkleKnobs &merkle_knobs_env() {   // read once per process
    static const MerkleKnobs knobs = [] {
        auto num = [](const char *name, long dflt) { return getenv(name) ? (long)atoi(getenv(name)) : dflt; };
        return merkle_knobs_make(num("SMI_MERKLE_K", 2), num("SMI_MERKLE_TOP_BLOCKS", 256), num("SMI_MERKLE_ELEMS_LOG", 19),
                                 num("SMI_MERKLE_SINGLE", 512), num("SMI_MERKLE_MINCHUNK", 64), num("SMI_MERKLE_FUSE", 1),
                                 num("SMI_MERKLE_GENERIC", 0));
    }();
    return knobs;
}

enum { MK_DIGESTS = 0, MK_ELEMENTS = 1, MK_ROWS = 2 };           // what level 0 is made from (rows: of row_cols <= 4 columns)
struct MerkleShape {
    size_t n;            // leaves per tree, a power of two
    uint32_t n_trees;
    int leaves;
    uint32_t row_cols;   // MK_ROWS only
};
enum { MK_LEAF_HASH = 0, MK_CHUNK = 1, MK_SUB = 2 };            // kernel family (a lone leaf hash: the tree is its leaf)
enum { MK_INST_ROWS = 0, MK_INST_K2 = 1, MK_INST_GENERIC = 2 };   // instantiation of the subtree kernel
// What the first step can do with computed leaves (LeafSrc, internal.h):
//   CHUNK: the chunk kernel folds as it reads, element by element -- LEAF_FOLD only, no alignment demand;
//   QUAD : the four-leaves-per-lane kernel folds or combines, four elements per access -- 16-byte aligned buffers only.
enum { MK_SRC_NONE = 0, MK_SRC_CHUNK = 1, MK_SRC_QUAD = 2 };
struct MerkleStep {
    uint8_t family, inst;
    bool from_leaves;    // level 0 is hashed from elements / rows by this step
    bool ends_root;      // one workgroup of one tree ends with the root: the Fiat-Shamir hook may fire here
    uint8_t src_cap;     // first step only
    uint32_t level;      // input level (0 with from_leaves)
    uint32_t arg;        // chunk size (MK_CHUNK) or levels per lane K (MK_SUB)
    size_t count, out;   // inputs and outputs per tree
    uint32_t grid;       // grid.x (grid.y = n_trees)
    size_t lds;          // dynamic LDS: the subtree kernel's stash of child digests
};
#define MK_MAX_STEPS 64   // K >= 1 level per step, n < 2^64
struct MerklePlan {
    uint32_t n_steps;
    MerkleStep s[MK_MAX_STEPS];
};

// Once what is left fits the chip as one wave of chunk workgroups, the per-level latency of the chunk kernel beats
// two-level launches: up to SMI_TOP_MAX digests per launch.  Chunks are as small as one workgroup per CU allows
// (not below MINCHUNK): the widest levels of a chunk are throughput on a single CU, so 256 chunks of 256 digests
// and then their 256 roots finish a 2^16-leaf tree in 42 us where 32 chunks of 2048 took 65.  Up to SINGLE digests
// stay one chunk.  (tools/sweep_merkle_chunks.sh: flat within 3 % from 8 to 64.)
inline MerklePlan merkle_plan(const MerkleShape &sh, const MerkleKnobs &kn) {
    MerklePlan pl;
    pl.n_steps = 0;
    if (!sh.n_trees) return pl;
    const uint32_t depth = ilog2(sh.n);
    const bool rows = sh.leaves == MK_ROWS;
    bool from_leaves = sh.leaves != MK_DIGESTS;
    uint32_t lvl = 0;
    size_t count = sh.n;
    auto push = [&](uint8_t family, uint8_t inst, uint32_t arg, size_t out, bool ends_root, size_t grid, size_t lds) {
        pl.s[pl.n_steps++] = MerkleStep{family, inst, from_leaves, ends_root, MK_SRC_NONE, lvl, arg, count, out, (uint32_t)grid, lds};
        from_leaves = false;
        count = out;
    };
    if (from_leaves && depth == 0 && !rows) {
        push(MK_LEAF_HASH, MK_INST_GENERIC, 0, 1, false, 1, 0);
        return pl;
    }
    while ((lvl < depth || from_leaves) && pl.n_steps < MK_MAX_STEPS) {
        size_t chunk = count;
        if (count > kn.single) {
            chunk = kn.minchunk;
            while (chunk < SMI_TOP_MAX && (count / chunk) * sh.n_trees > kn.top_blocks) chunk <<= 1;
        }
        const size_t n_chunks = count / chunk;
        if (chunk <= SMI_TOP_MAX && n_chunks * sh.n_trees <= kn.top_blocks && (!from_leaves || rows || count <= kn.elems_max())) {
            push(MK_CHUNK, MK_INST_GENERIC, (uint32_t)chunk, n_chunks, n_chunks == 1 && sh.n_trees == 1, n_chunks, 0);
            lvl += ilog2(chunk) + !is_pow2(chunk);   // ceil
            continue;
        }
        // the hot shapes (element leaves or digests, two levels per lane) have instantiations of their own: with leaves the
        // stash holds two digests per lane, with digests there is none
        const uint32_t K = depth - lvl < kn.k ? depth - lvl : kn.k;
        const uint8_t inst = from_leaves && rows ? MK_INST_ROWS : (K == 2 && !kn.generic ? MK_INST_K2 : MK_INST_GENERIC);
        const size_t stash = inst == MK_INST_K2 ? (from_leaves ? 16 : 0) : 8u << K;
        const size_t threads = count >> K;
        push(MK_SUB, inst, K, threads, false, (threads + SMI_HASH_THREADS - 1) / SMI_HASH_THREADS,
             stash * SMI_HASH_THREADS * sizeof(uint32_t));
        lvl += K;
    }
    MerkleStep &first = pl.s[0];
    if (kn.fuse && sh.leaves == MK_ELEMENTS && sh.n_trees == 1 && pl.n_steps) {
        if (first.family == MK_CHUNK) first.src_cap = MK_SRC_CHUNK;
        else if (first.family == MK_SUB && first.inst == MK_INST_K2 && sh.n >= 8) first.src_cap = MK_SRC_QUAD;
    }
    return pl;
}
// what the first launch of one tree of n single-element leaves can do with computed leaves
inline int merkle_src_cap(size_t n, const MerkleKnobs &kn) {
    const MerklePlan pl = merkle_plan(MerkleShape{n, 1, MK_ELEMENTS, 0}, kn);
    return is_pow2(n) && pl.n_steps ? (int)pl.s[0].src_cap : (int)MK_SRC_NONE;
}

// Profile accounting of one step.  bytes: inputs read once (4 B elements or 32 B digests), every produced digest written
// once; mixes: mix_state evaluations, 9 per single-element leaf (one more per extra 32-byte chunk of a row), 10 per node.
struct MerkleCost {
    double bytes, mixes;
};
inline MerkleCost merkle_step_cost(const MerkleStep &s, const MerkleShape &sh) {
    const double count = (double)s.count, out = (double)s.out, cols = sh.leaves == MK_ROWS ? sh.row_cols : 1;
    const double produced = (s.from_leaves ? 2.0 * count : count) - out;
    const double leaf_mixes = s.from_leaves ? (8.0 + (double)(((uint32_t)cols + 3) / 4)) * count : 0.0;
    return MerkleCost{((s.from_leaves ? 4.0 * cols : 32.0) * count + 32.0 * produced) * sh.n_trees,
                      (leaf_mixes + 10.0 * (count - out)) * sh.n_trees};
}
