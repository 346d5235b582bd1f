// fri_plan.h -- host-side planning of Fri::commit / Fri::prove, shared by the single-GPU driver (fri.hip), the multi-GPU
// round loop (mgpu_loop.h) and the CPU emulator of the non-GPU tests (emu.cpp).  No HIP in here.
//   fri_layout     : the number of rounds and the byte layout of the serialized proof;
//   fri_round_plan : per round, who produces the codeword and who builds its tree and runs its Fiat-Shamir round.
#pragma once
#include "../../include/stark_mi.h"
#include "merkle_plan.h"

#define SMI_FRI_MAX_ROUNDS 64
#define SMI_FRI_TAIL_MAX_ROUNDS 12
#define SMI_FRI_TAIL_MAX_LEN 2048   // = SMI_TOP_MAX: what one workgroup finishes

// proof layout (src/fri.rs:129,151,229-243; tags src/stream.rs:39-60): R root records, the last codeword, then per
// layer t triples and t x 3 Merkle paths
struct FriLayout {
    uint64_t R, last_n;   // src/fri.rs:93-103; the last codeword's length (the domain's when R == 0)
    size_t off_last, off_layers, proof_len;
    size_t off_triples[SMI_FRI_MAX_ROUNDS], off_paths[SMI_FRI_MAX_ROUNDS];   // layers 0 .. R - 2
};
inline FriLayout fri_layout(const smi_fri_cfg &cfg, bool do_query) {
    FriLayout l = {};
    const uint64_t N = cfg.domain_length, t = cfg.num_colinearity_tests;
    l.R = 0;
    for (uint64_t len = N; len > cfg.expansion_factor && 4 * t < len; len /= 2) l.R++;
    l.last_n = l.R ? N >> (l.R - 1) : N;
    l.off_last = 33 * l.R;
    l.off_layers = l.off_last + 9 + 8 * l.last_n;
    size_t off = l.off_layers;
    for (uint64_t i = 0; i + 1 < l.R; i++) {
        const uint32_t d = ilog2(N >> i);
        l.off_triples[i] = off;
        off += 33 * t;
        l.off_paths[i] = off;
        off += t * (2 * (9 + 32ull * d) + (9 + 32ull * (d - 1)));
    }
    l.proof_len = do_query ? off : l.off_layers;
    return l;
}

// The same layout for FRI over the quartic extension (include/stark_mi.h, "Extension FRI"): an element is four u64, so the
// last codeword is one record of 4 last_n values and a triple one record of 12; rounds, paths and their order are unchanged.
// pow: the proof-of-work nonce record (include/stark_mi.h, "Grinding": tag 2, count 1, one u64) sits between the last
// codeword and the layers, at off_layers - SMI_GRIND_RECORD_BYTES.
#define SMI_GRIND_RECORD_BYTES 17
inline FriLayout fri_layout_ext(const smi_fri_cfg &cfg, bool pow = false) {
    FriLayout l = fri_layout(cfg, true);
    const uint64_t N = cfg.domain_length, t = cfg.num_colinearity_tests;
    l.off_layers = l.off_last + 9 + 32 * l.last_n + (pow ? SMI_GRIND_RECORD_BYTES : 0);
    size_t off = l.off_layers;
    for (uint64_t i = 0; i + 1 < l.R; i++) {
        const uint32_t d = ilog2(N >> i);
        l.off_triples[i] = off;
        off += (9 + 96) * t;
        l.off_paths[i] = off;
        off += t * (2 * (9 + 32ull * d) + (9 + 32ull * (d - 1)));
    }
    l.proof_len = off;
    return l;
}

// Extension FRI at folding factor 4 (include/stark_mi.h, "Extension FRI, folding factor 4"): with R2 the reference's round
// count, F = (R2 - 1) / 2 folds and F + 1 committed codewords, layer r of length N / 4^r; the last one, of length
// N / 4^F, in the clear; the nonce record always present; per layer t coset records of 16 values and t paths of
// log2(n_r / 4) digests.
struct FriFold4Layout {
    uint64_t R2, F, last_n;
    size_t off_last, off_nonce, off_layers, proof_len;
    size_t off_cosets[SMI_FRI_MAX_ROUNDS / 2], off_paths[SMI_FRI_MAX_ROUNDS / 2];   // layers 0 .. F - 1
};
inline FriFold4Layout fri_layout_fold4(const smi_fri_cfg &cfg) {
    FriFold4Layout l = {};
    const uint64_t N = cfg.domain_length, t = cfg.num_colinearity_tests;
    l.R2 = fri_layout(cfg, false).R;
    l.F = l.R2 ? (l.R2 - 1) / 2 : 0;
    l.last_n = N >> (2 * l.F);
    l.off_last = 33 * (l.F + 1);
    l.off_nonce = l.off_last + 9 + 32 * l.last_n;
    l.off_layers = l.off_nonce + SMI_GRIND_RECORD_BYTES;
    size_t off = l.off_layers;
    for (uint64_t r = 0; r < l.F; r++) {
        const uint32_t d = ilog2(N >> (2 * r)) - 2;   // log2 q_r
        l.off_cosets[r] = off;
        off += (9 + 128) * t;
        l.off_paths[r] = off;
        off += t * (9 + 32ull * d);
    }
    l.proof_len = off;
    return l;
}

// The fused tail (hash.hip, fri_tail_kernel) finishes every remaining round in one workgroup launch.  It runs the
// sixteen-lane Fiat-Shamir round, which knows phase 0 only, and holds at most max_rounds rounds.
inline bool fri_tail_starts(uint32_t phase, uint64_t len, uint64_t tail_len, uint64_t rounds_left, uint64_t max_rounds) {
    return phase == 0 && len <= tail_len && rounds_left <= max_rounds;
}

// the initial codeword: the caller's buffer (only that one can be misaligned), or computed by the first tree's launch as
// the caller's weighted column sum (LEAF_COMBINE)
enum { FRI_R0_ALIGNED16 = 0, FRI_R0_UNALIGNED = 1, FRI_R0_COMBINE = 2 };
// who produces a round's codeword ...
enum {
    FRI_BY_CALLER = 0,
    FRI_BY_FOLD = 1,         // a fold launch
    FRI_BY_LEAF_CHUNK = 2,   // the first step of the round's own tree (merkle_plan.h MK_SRC_CHUNK / MK_SRC_QUAD): one launch and one
    FRI_BY_LEAF_QUAD = 3,    //   pass over the codeword less -- the hash kernels are bound by integer issue and leave HBM idle
    FRI_BY_TAIL_HEAD = 4,    // the head of the tail launch
    FRI_IN_TAIL = 5,
};
// ... and who builds its tree and runs its Fiat-Shamir round
enum {
    FRI_TREE_HOOK = 0,    // the Merkle launches, the one that ends with the root running the round (a kernel of its own otherwise)
    FRI_TREE_PHASE = 1,   // the Merkle launches, then the phase-aware single-lane kernel
    FRI_TREE_TAIL = 2,
};
struct FriRoundPlan {
    bool ok;            // false: round 0 cannot be FRI_R0_COMBINE for this length
    uint32_t R, tail_at;   // the tail takes rounds [tail_at, R); tail_at == R: no tail
    uint8_t producer[SMI_FRI_MAX_ROUNDS], tree[SMI_FRI_MAX_ROUNDS];
};
// A leaf-computed codeword is planned only where merkle_plan's first step for that length really takes it, and
// FRI_BY_LEAF_QUAD only between 16-byte aligned buffers: the library's own are, so only round 1 can lose it.
inline FriRoundPlan fri_round_plan(uint64_t len, uint64_t R, uint32_t phase, uint64_t tail_len, int round0, const MerkleKnobs &kn) {
    FriRoundPlan pl;
    pl.R = (uint32_t)R;
    pl.tail_at = pl.R;
    // The combination is taken exactly where it was before the planners existed: outside the tail, and by a tree too large
    // for the chunk kernel.  `len > elems_max()` is kept for that parity alone (under SINGLE > 2048 a smaller tree can start
    // with a QUAD step too, and is still refused); tests/test_launch_plans.py pins it against the old rule.
    pl.ok = round0 != FRI_R0_COMBINE || (merkle_src_cap(len, kn) == MK_SRC_QUAD && len > kn.elems_max() && len > tail_len);
    for (uint32_t r = 0; r < pl.R; r++) {
        const uint64_t n = len >> r;
        if (pl.tail_at == pl.R && fri_tail_starts(phase, n, tail_len, R - r, SMI_FRI_TAIL_MAX_ROUNDS)) pl.tail_at = r;
        pl.tree[r] = r >= pl.tail_at ? FRI_TREE_TAIL : (phase ? FRI_TREE_PHASE : FRI_TREE_HOOK);
        const int cap = r > 0 && r < pl.tail_at ? merkle_src_cap(n, kn) : MK_SRC_NONE;
        if (r == 0) pl.producer[r] = round0 == FRI_R0_COMBINE ? FRI_BY_LEAF_QUAD : FRI_BY_CALLER;
        else if (r > pl.tail_at) pl.producer[r] = FRI_IN_TAIL;
        else if (r == pl.tail_at) pl.producer[r] = kn.fuse ? FRI_BY_TAIL_HEAD : FRI_BY_FOLD;
        else if (cap == MK_SRC_QUAD && (r > 1 || round0 != FRI_R0_UNALIGNED)) pl.producer[r] = FRI_BY_LEAF_QUAD;
        else if (cap == MK_SRC_CHUNK) pl.producer[r] = FRI_BY_LEAF_CHUNK;
        else pl.producer[r] = FRI_BY_FOLD;
    }
    return pl;
}
