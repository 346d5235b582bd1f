// verify.hip -- Fri::verify (reference src/fri.rs:313-504) behind the C ABI, and the verifier of the
// build-defined composition's column openings (smi_stark_cfg.open_columns).
//
// The reference's control flow runs on the host over the serialized ProofStream (src/stream.rs:66-168,
// with its leniency for truncated objects); the work that scales with the proof goes to the device
// in batches: every leaf hash (Hash::from_field_elements(&[v]) = the hash of v's 8 LE bytes,
// src/hash.rs:32-35 -- taken from the raw u64, so an unreduced value hashes as the reference hashes
// it), every authentication path (MerkleTree::verify, src/merkle.rs:82-96), the Merkle root of the
// last codeword, and the last layer's low-degree test as an inverse + forward NTT instead of the
// reference's O(L^3) Lagrange interpolation.  *accept is 1 where the reference returns
// true and 0 where it prints a reason and returns false (smi_last_error carries the reason); where
// the reference panics the status is that panic's code.
#include <string.h>

#include <vector>

#include "air_core.h"
#include "fri_core.h"
#include "hash_core.h"
#include "internal.h"
#include "perm_core.h"
#include "proof_parse.h"

namespace {
using proofp::Obj;
using proofp::get_u64;
using proofp::parse;
uint64_t mulm(uint64_t a, uint64_t b, uint64_t p) { return (uint64_t)((unsigned __int128)a * b % p); }
// FiniteField::sub (src/ff.rs:154-160): `p + l - r` in u128, then `% p`; for an unreduced r > p + l a release build wraps
// mod 2^128 before the reduction (a debug build panics) -- the oracle restates the release behaviour and so does this
uint64_t subm(uint64_t a, uint64_t b, uint64_t p) { return (uint64_t)((((unsigned __int128)p + a) - b) % p); }
uint64_t powm(uint64_t b, uint64_t e, uint64_t p) {
    uint64_t r = 1 % p;
    b %= p;
    while (e) {
        if (e & 1) r = mulm(r, b, p);
        b = mulm(b, b, p);
        e >>= 1;
    }
    return r;
}
int reject(smi_ctx *ctx, int *accept, const char *why) {
    *accept = 0;
    ctx->err = why;
    return SMI_OK;
}
// leaf digests of raw u64 values: Hash::from_bytes(v.to_le_bytes())
int leaf_digests(smi_ctx *ctx, const uint64_t *v, size_t n, std::vector<uint8_t> &out) {
    std::vector<uint8_t> msgs(8 * n);
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 8; k++) msgs[8 * i + k] = (uint8_t)(v[i] >> (8 * k));
    out.resize(32 * n);
    return n ? smi_hash_bytes_batch(ctx, msgs.data(), n, 8, out.data()) : SMI_OK;
}
// FiatShamir::challenge over the transcript of the first k roots
int challenge_of(smi_ctx *ctx, const std::vector<uint8_t> &transcript, uint64_t *out) {
    uint8_t d[32];
    SMI_TRY(smi_hash_bytes(ctx, transcript.data(), transcript.size(), d));
    *out = get_u64(d);
    return SMI_OK;
}

// Fri::sample_indices (src/fri.rs:168-213) from the index-seed challenge, counters hashed a batch at a time
int sample_top(smi_ctx *ctx, uint64_t seed_ch, uint64_t size, uint64_t reduced_size, uint64_t t, std::vector<uint64_t> *top_out) {
    if (t > 2 * reduced_size) return smi_fail(ctx, SMI_ERR_SAMPLE_ENTROPY, nullptr);
    if (t > reduced_size) return smi_fail(ctx, SMI_ERR_SAMPLE_TOO_MANY, nullptr);
    uint8_t seed[32], seed_msg[8];
    for (int k = 0; k < 8; k++) seed_msg[k] = (uint8_t)(seed_ch >> (8 * k));
    SMI_TRY(smi_hash_bytes(ctx, seed_msg, 8, seed));                                // Hash::from_u64
    std::vector<uint64_t> &top = *top_out, reduced;
    top.clear();
    for (uint32_t counter = 0; top.size() < t;) {
        const size_t run = 2 * (size_t)(t - top.size()) + 8;
        std::vector<uint8_t> msgs(36 * run), dig(32 * run);
        for (size_t k = 0; k < run; k++) {
            memcpy(&msgs[36 * k], seed, 32);
            for (int b = 0; b < 4; b++) msgs[36 * k + 32 + b] = (uint8_t)((counter + k) >> (8 * b));
        }
        SMI_TRY(smi_hash_bytes_batch(ctx, msgs.data(), run, 36, dig.data()));
        for (size_t k = 0; k < run && top.size() < t; k++, counter++) {
            uint64_t acc = 0;                                                       // sample_index: the last eight digest bytes, big-endian
            for (int b = 24; b < 32; b++) acc = (acc << 8) | dig[32 * k + b];
            const uint64_t index = acc % size, ri = index % reduced_size;
            bool seen = false;
            for (uint64_t q : reduced) seen |= q == ri;
            if (!seen) {
                top.push_back(index);
                reduced.push_back(ri);
            }
        }
    }
    return SMI_OK;
}

// Fri::verify on objs[0..] with the transcript the caller's FiatShamir holds (seed, hash_core.h fs_seed); *used = objects
// consumed on acceptance.  The challenges continue the seed one root at a time instead of re-hashing the transcript.
int fri_verify_objs(smi_ctx *ctx, const smi_fri_cfg &cfg, const FsSeed &fs0, const std::vector<Obj> &objs, int *accept,
                    std::vector<uint64_t> *top_out, std::vector<uint64_t> *pv_idx, std::vector<uint64_t> *pv_val,
                    std::vector<uint64_t> *layer0_ab, size_t *used) {
    const uint64_t p = ctx->fs.F.p, t = cfg.num_colinearity_tests, N = cfg.domain_length;
    uint64_t R = 0;
    smi_fri_num_rounds(&cfg, &R);
    size_t at = 0;
    auto pop = [&]() -> const Obj * { return at < objs.size() ? &objs[at++] : nullptr; };
    uint32_t fs[16];
    memcpy(fs, fs0.s, sizeof fs);
    std::vector<const uint8_t *> roots;
    std::vector<uint64_t> alphas;
    for (uint64_t r = 0; r < R; r++) {                                             // src/fri.rs:325-334
        const Obj *o = pop();
        if (!o || o->tag != 0) return reject(ctx, accept, "Failed to extract Merkle root");
        roots.push_back(o->p);
        uint32_t m[8];
        memcpy(m, o->p, 32);   // little-endian words (proof bytes in order)
        uint64_t a = 0;
        hashc::fs_absorb_root_phase(fs, m, fs0.phase, nullptr, &a);
        alphas.push_back(a);
    }
    const Obj *lo = pop();                                                          // :337-342
    if (!lo || lo->tag != 2) return reject(ctx, accept, "Failed to extract last codeword");
    if (R == 0) return reject(ctx, accept, "No FRI roots extracted");               // :345-348
    const size_t n_last = lo->count;
    std::vector<uint64_t> last(n_last);
    for (size_t i = 0; i < n_last; i++) last[i] = get_u64(lo->p + 8 * i);
    if (n_last == 0) return smi_fail(ctx, SMI_ERR_EMPTY_LEAVES, nullptr);          // MerkleTree::new panics, :353
    if (!is_pow2(n_last)) return smi_fail(ctx, SMI_ERR_LEAVES_NOT_POW2, nullptr);
    std::vector<uint8_t> digests;
    SMI_TRY(leaf_digests(ctx, last.data(), n_last, digests));
    uint8_t last_root[32];
    SMI_TRY(smi_merkle_commit(ctx, digests.data(), n_last, last_root));
    if (memcmp(last_root, roots.back(), 32) != 0) return reject(ctx, accept, "last codeword is not well formed");
    const size_t degree_bound = n_last / cfg.expansion_factor;                      // :360-365
    if (degree_bound == 0) return reject(ctx, accept, "last codeword too small");
    uint64_t last_omega = cfg.omega % p, last_offset = cfg.offset % p;
    for (uint64_t i = 0; i + 1 < R; i++) {
        last_omega = mulm(last_omega, last_omega, p);
        last_offset = mulm(last_offset, last_offset, p);
    }
    // The reference interpolates over the point list offset_L * omega_L^i; the transform needs that list
    // to be the coset of the 2^k-th roots (any prover that folded a codeword over a proper domain has it).
    if (n_last > ((uint64_t)1 << ctx->fs.K) || last_omega != h_root(ctx, ilog2(n_last)) || last_offset == 0)
        return smi_fail(ctx, SMI_ERR_NOT_GEOMETRIC, "Fri::verify: the last layer's domain is not offset * <primitive root>");
    for (size_t i = 0; i < n_last; i++)
        if (last[i] >= p) return reject(ctx, accept, "re-evaluated codeword does not match original!");   // :384-390 on an unreduced value
    std::vector<uint64_t> coeffs(n_last), re_eval(n_last);
    if (n_last > 1) {
        SMI_TRY(smi_intt(ctx, last.data(), coeffs.data(), ilog2(n_last), last_offset));
        SMI_TRY(smi_coset_ntt(ctx, coeffs.data(), n_last, re_eval.data(), ilog2(n_last), last_offset));
        if (re_eval != last) return reject(ctx, accept, "re-evaluated codeword does not match original!");
    } else {
        coeffs = last;
    }
    for (size_t i = degree_bound; i < n_last; i++)                                  // :392-397: degree <= degree_bound - 1
        if (coeffs[i] != 0) return reject(ctx, accept, "last codeword does not correspond to polynomial of low enough degree");

    // index sampling (:400-405, :168-213)
    std::vector<uint64_t> top;
    SMI_TRY(sample_top(ctx, hashc::fs_challenge_phase(fs, fs0.phase), N >> 1, N >> (R - 1), t, &top));
    if (top_out) *top_out = top;

    uint64_t om = cfg.omega % p, off = cfg.offset % p;
    for (uint64_t r = 0; r + 1 < R; r++) {                                          // :408-502
        const uint64_t half = N >> (r + 1);
        std::vector<uint64_t> ci(t), bi(t), aa(t), bb(t), cc(t);
        for (uint64_t s = 0; s < t; s++) {
            ci[s] = top[s] % half;
            bi[s] = ci[s] + half;
            const Obj *o = pop();
            if (!o || o->tag != 2) return reject(ctx, accept, "Failed to extract triple values");
            if (o->count != 3) return reject(ctx, accept, "Expected triple of values");
            aa[s] = get_u64(o->p);
            bb[s] = get_u64(o->p + 8);
            cc[s] = get_u64(o->p + 16);
            if (r == 0) {
                if (pv_idx && pv_val) {
                    pv_idx->push_back(ci[s]); pv_val->push_back(aa[s]);
                    pv_idx->push_back(bi[s]); pv_val->push_back(bb[s]);
                }
                if (layer0_ab) {
                    layer0_ab->push_back(aa[s]);
                    layer0_ab->push_back(bb[s]);
                }
            }
            // test_colinearity (:507-525): (y1 - y0)(x2 - x0) == (y2 - y0)(x1 - x0)
            const uint64_t ax = mulm(off, powm(om, ci[s], p), p), bx = mulm(off, powm(om, bi[s], p), p), cx = alphas[r] % p;
            if (mulm(subm(bb[s], aa[s], p), subm(cx, ax, p), p) != mulm(subm(cc[s], aa[s], p), subm(bx, ax, p), p))
                return reject(ctx, accept, "colinearity check failure");
        }
        // The 3t authentication paths.  The reference pops and verifies them one at a time in the order
        // (test 0: a, b, c), (test 1: a, b, c), ... and stops at the first failure of either kind; here the paths
        // are verified in one device batch per (a, b, c), so the pops run first, up to the first one that fails,
        // and the verdict is the earliest failure in the reference's order.
        static const char *const miss[3] = {"Failed to extract path for aa", "Failed to extract path for bb", "Failed to extract path for cc"};
        static const char *const bad[3] = {"merkle authentication path verification fails for aa", "merkle authentication path verification fails for bb",
                                           "merkle authentication path verification fails for cc"};
        const uint32_t want_depth[3] = {ilog2(2 * half), ilog2(2 * half), ilog2(half)};
        std::vector<std::vector<uint8_t>> paths(3);
        std::vector<uint64_t> have(3, 0);        // how many paths of each kind were popped
        uint64_t stop_at = 3 * t;                // position (3 s + w) of the first pop that failed
        const char *stop_why = nullptr;
        for (uint64_t s = 0; s < t && !stop_why; s++)
            for (int w = 0; w < 3; w++) {
                const Obj *o = pop();
                if (!o || o->tag != 3) { stop_at = 3 * s + w; stop_why = miss[w]; break; }
                if (o->count != want_depth[w]) { stop_at = 3 * s + w; stop_why = bad[w]; break; }   // wrong length: the recomputed root cannot match
                paths[w].insert(paths[w].end(), o->p, o->p + 32 * o->count);
                have[w]++;
            }
        const std::vector<uint64_t> *vals[3] = {&aa, &bb, &cc}, *idxs[3] = {&ci, &bi, &ci};
        const uint8_t *rt[3] = {roots[r], roots[r], roots[r + 1]};
        uint64_t first_bad = stop_at;
        const char *why = stop_why;
        for (int w = 0; w < 3; w++) {
            const uint64_t k = have[w];
            if (!k) continue;
            std::vector<uint8_t> leaf, ok(k);
            SMI_TRY(leaf_digests(ctx, vals[w]->data(), k, leaf));
            if (want_depth[w])
                SMI_TRY(smi_merkle_verify_batch(ctx, leaf.data(), idxs[w]->data(), paths[w].data(), k, want_depth[w], rt[w], ok.data()));
            else
                for (uint64_t s = 0; s < k; s++) ok[s] = memcmp(&leaf[32 * s], rt[w], 32) == 0;   // a one-leaf tree: the leaf is the root
            for (uint64_t s = 0; s < k; s++)
                if (!ok[s] && 3 * s + w < first_bad) {
                    first_bad = 3 * s + w;
                    why = bad[w];
                }
        }
        if (why) return reject(ctx, accept, why);
        om = mulm(om, om, p);
        off = mulm(off, off, p);
    }
    *accept = 1;
    if (used) *used = at;
    return SMI_OK;
}
// The verifier of FRI over the quartic extension (include/stark_mi.h, "Extension FRI") on objs[0..]; the structure of
// fri_verify_objs with four-coordinate elements.  pv_val gets four values per entry, layer0_ab eight per test (a, then b).
// grind: the least proof-of-work difficulty demanded (include/stark_mi.h, "Grinding"), or SMI_GRIND_NONE: no nonce record.
int fri_verify_ext_objs(smi_ctx *ctx, const smi_fri_cfg &cfg, const FsSeed &fs0, const std::vector<Obj> &objs, int *accept,
                        std::vector<uint64_t> *top_out, std::vector<uint64_t> *pv_idx, std::vector<uint64_t> *pv_val,
                        std::vector<uint64_t> *layer0_ab, size_t *used, int grind = SMI_GRIND_NONE) {
    const uint32_t p = ctx->fs.F.p, g = ctx->fs.g;
    const uint64_t t = cfg.num_colinearity_tests, N = cfg.domain_length;
    uint64_t R = 0;
    smi_fri_num_rounds(&cfg, &R);
    if (R == 0) return reject(ctx, accept, "No FRI roots extracted");
    size_t at = 0;
    auto pop = [&]() -> const Obj * { return at < objs.size() ? &objs[at++] : nullptr; };
    uint32_t fs[16];
    memcpy(fs, fs0.s, sizeof fs);
    std::vector<const uint8_t *> roots;
    std::vector<uint64_t> alphas;   // four unreduced coordinates per round but the last
    for (uint64_t r = 0; r < R; r++) {
        const Obj *o = pop();
        if (!o || o->tag != 0) return reject(ctx, accept, "Failed to extract Merkle root");
        roots.push_back(o->p);
        uint32_t m[8];
        memcpy(m, o->p, 32);
        if (r + 1 == R) {
            hashc::fs_absorb_root_phase(fs, m, fs0.phase, nullptr, nullptr);
            break;
        }
        uint32_t out[16];
        for (int e = 0; e < 4; e++) {
            uint64_t a = 0;
            hashc::fs_round_ext_lane(fs, m, fs0.phase, e, out, &a);
            alphas.push_back(a);
        }
        memcpy(fs, out, sizeof fs);
    }
    const size_t n_last = (size_t)(N >> (R - 1));
    const Obj *lo = pop();
    if (!lo || lo->tag != 2) return reject(ctx, accept, "Failed to extract last codeword");
    if (lo->count != 4 * n_last) return reject(ctx, accept, "last codeword: expected four values per element of the last domain");
    std::vector<uint64_t> last(4 * n_last);
    for (size_t i = 0; i < 4 * n_last; i++)
        if ((last[i] = get_u64(lo->p + 8 * i)) >= p) return reject(ctx, accept, "last codeword: a coordinate is not canonical");
    // row-leaf root: leaf i = Hash::from_field_elements of element i's four u64s as they stand in the proof
    std::vector<uint8_t> digests(32 * n_last);
    for (size_t i = 0; i < n_last; i++) {
        uint32_t d[8];
        hashc::hash_bytes(lo->p + 32 * i, 32, d);
        memcpy(&digests[32 * i], d, 32);
    }
    uint8_t last_root[32];
    SMI_TRY(smi_merkle_commit(ctx, digests.data(), n_last, last_root));
    if (memcmp(last_root, roots.back(), 32) != 0) return reject(ctx, accept, "last codeword is not well formed");
    const size_t degree_bound = n_last / cfg.expansion_factor;
    if (degree_bound == 0) return reject(ctx, accept, "last codeword too small");
    uint64_t last_omega = cfg.omega % p, last_offset = cfg.offset % p;
    for (uint64_t i = 0; i + 1 < R; i++) {
        last_omega = mulm(last_omega, last_omega, p);
        last_offset = mulm(last_offset, last_offset, p);
    }
    if (n_last > ((uint64_t)1 << ctx->fs.K) || last_omega != h_root(ctx, ilog2(n_last)) || last_offset == 0)
        return smi_fail(ctx, SMI_ERR_NOT_GEOMETRIC, "Fri::verify: the last layer's domain is not offset * <primitive root>");
    // EVERY coordinate is a base-field codeword on the last domain and must be of low degree
    for (int e = 0; e < 4; e++) {
        std::vector<uint64_t> col(n_last), coeffs(n_last);
        for (size_t i = 0; i < n_last; i++) col[i] = last[4 * i + e];
        if (n_last > 1) SMI_TRY(smi_intt(ctx, col.data(), coeffs.data(), ilog2(n_last), last_offset));
        else coeffs = col;
        for (size_t i = degree_bound; i < n_last; i++)
            if (coeffs[i] != 0) return reject(ctx, accept, "last codeword does not correspond to polynomial of low enough degree");
    }
    uint32_t seed_phase = fs0.phase;
    if (grind != SMI_GRIND_NONE) {   // the nonce record: one u64 (not a field element), checked with one hash, then absorbed
        const Obj *no = pop();
        if (!no || no->tag != 2) return reject(ctx, accept, "proof of work: failed to extract the nonce");
        if (no->count != 1) return reject(ctx, accept, "proof of work: the nonce record must hold exactly one value");
        const uint64_t word = hashc::grind_word(fs, fs0.phase, get_u64(no->p), fs, &seed_phase);
        if (word & ((1ull << grind) - 1)) return reject(ctx, accept, "proof of work");
    }
    std::vector<uint64_t> top;
    SMI_TRY(sample_top(ctx, hashc::fs_challenge_phase(fs, seed_phase), N >> 1, n_last, t, &top));
    if (top_out) *top_out = top;

    uint64_t om = cfg.omega % p, off = cfg.offset % p;
    for (uint64_t r = 0; r + 1 < R; r++) {
        const uint64_t half = N >> (r + 1);
        std::vector<uint64_t> ci(t), bi(t);
        std::vector<const uint8_t *> rec(t);
        const uint32_t al[4] = {(uint32_t)(alphas[4 * r] % p), (uint32_t)(alphas[4 * r + 1] % p), (uint32_t)(alphas[4 * r + 2] % p), (uint32_t)(alphas[4 * r + 3] % p)};
        for (uint64_t s = 0; s < t; s++) {
            ci[s] = top[s] % half;
            bi[s] = ci[s] + half;
            const Obj *o = pop();
            if (!o || o->tag != 2) return reject(ctx, accept, "Failed to extract triple values");
            if (o->count != 12) return reject(ctx, accept, "Expected triple of values");
            rec[s] = o->p;
            uint32_t v[12];
            for (int k = 0; k < 12; k++) {
                const uint64_t x = get_u64(o->p + 8 * k);
                if (x >= p) return reject(ctx, accept, "triple: a coordinate is not canonical");
                v[k] = (uint32_t)x;
            }
            if (r == 0) {
                if (pv_idx && pv_val) {
                    pv_idx->push_back(ci[s]); pv_val->insert(pv_val->end(), v, v + 4);
                    pv_idx->push_back(bi[s]); pv_val->insert(pv_val->end(), v + 4, v + 8);
                }
                if (layer0_ab) layer0_ab->insert(layer0_ab->end(), v, v + 8);
            }
            // (x_a, a), (-x_a, b), (alpha, c) colinear over F_q: (b - a)(alpha - x_a) == (c - a)(x_b - x_a), x_a and x_b in F_p
            const uint32_t ax = (uint32_t)mulm(off, powm(om, ci[s], p), p), bx = (uint32_t)mulm(off, powm(om, bi[s], p), p);
            uint32_t ba[4], ca[4], lhs[4];
            for (int e = 0; e < 4; e++) {
                ba[e] = fp_sub(v[4 + e], v[e], p);
                ca[e] = fp_sub(v[8 + e], v[e], p);
            }
            const uint32_t ax4[4] = {fp_sub(al[0], ax, p), al[1], al[2], al[3]};
            ext_mul_host(p, g, ba, ax4, lhs);
            const uint32_t dx = fp_sub(bx, ax, p);
            for (int e = 0; e < 4; e++)
                if (lhs[e] != host_mulmod(ca[e], dx, p)) return reject(ctx, accept, "colinearity check failure");
        }
        static const char *const miss[3] = {"Failed to extract path for aa", "Failed to extract path for bb", "Failed to extract path for cc"};
        static const char *const bad[3] = {"merkle authentication path verification fails for aa", "merkle authentication path verification fails for bb",
                                           "merkle authentication path verification fails for cc"};
        const uint32_t want_depth[3] = {ilog2(2 * half), ilog2(2 * half), ilog2(half)};
        std::vector<std::vector<uint8_t>> paths(3), leaves(3);
        for (uint64_t s = 0; s < t; s++)
            for (int w = 0; w < 3; w++) {
                const Obj *o = pop();
                if (!o || o->tag != 3) return reject(ctx, accept, miss[w]);
                if (o->count != want_depth[w]) return reject(ctx, accept, bad[w]);
                paths[w].insert(paths[w].end(), o->p, o->p + 32 * o->count);
                uint32_t d[8];   // the leaf: the four u64s of a / b / c as they stand in the proof
                hashc::hash_bytes(rec[s] + 32 * w, 32, d);
                leaves[w].insert(leaves[w].end(), (const uint8_t *)d, (const uint8_t *)d + 32);
            }
        const std::vector<uint64_t> *idxs[3] = {&ci, &bi, &ci};
        const uint8_t *rt[3] = {roots[r], roots[r], roots[r + 1]};
        uint64_t first_bad = 3 * t;
        const char *why = nullptr;
        for (int w = 0; w < 3 && t; w++) {
            std::vector<uint8_t> ok(t);
            if (want_depth[w])
                SMI_TRY(smi_merkle_verify_batch(ctx, leaves[w].data(), idxs[w]->data(), paths[w].data(), t, want_depth[w], rt[w], ok.data()));
            else
                for (uint64_t s = 0; s < t; s++) ok[s] = memcmp(&leaves[w][32 * s], rt[w], 32) == 0;
            for (uint64_t s = 0; s < t; s++)
                if (!ok[s] && 3 * s + w < first_bad) {
                    first_bad = 3 * s + w;
                    why = bad[w];
                }
        }
        if (why) return reject(ctx, accept, why);
        om = mulm(om, om, p);
        off = mulm(off, off, p);
    }
    *accept = 1;
    if (used) *used = at;
    return SMI_OK;
}
size_t fri_object_count(const smi_fri_cfg &cfg) {
    uint64_t R = 0;
    smi_fri_num_rounds(&cfg, &R);
    return (size_t)(R + 1 + (R ? R - 1 : 0) * 4 * cfg.num_colinearity_tests);
}
FsSeed fresh_seed() {
    FsSeed z;
    hashc::fs_seed(nullptr, 0, z.s, &z.phase);
    return z;
}
}  // namespace

int smi_fri_verify_fs(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint8_t *proof,
                      size_t proof_len, int *accept, uint64_t *pv_indices, uint64_t *pv_values, size_t *n_pv, size_t *consumed) {
    if (!ctx || !cfg || (!proof && proof_len) || !accept || (!transcript && transcript_len)) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    if (n_pv) *n_pv = 0;
    if (consumed) *consumed = 0;
    SMI_TRY(smi_fri_check(ctx, cfg));
    FsSeed seed;
    hashc::fs_seed(transcript, transcript_len, seed.s, &seed.phase);
    size_t end = 0;
    const std::vector<Obj> objs = parse(proof, proof_len, (size_t)-1, &end);
    std::vector<uint64_t> pi, pv;
    size_t used = 0;
    const int rc = fri_verify_objs(ctx, *cfg, seed, objs, accept, nullptr, &pi, &pv, nullptr, &used);
    if (n_pv) *n_pv = pi.size();       // like the reference's &mut Vec: what was pushed before a rejection stays
    if (pv_indices && !pi.empty()) memcpy(pv_indices, pi.data(), 8 * pi.size());
    if (pv_values && !pv.empty()) memcpy(pv_values, pv.data(), 8 * pv.size());
    if (rc == SMI_OK && *accept && consumed) (void)parse(proof, proof_len, used, consumed);   // the bytes of the popped objects
    return rc;
}
int smi_fri_verify(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *proof, size_t proof_len, int *accept, uint64_t *pv_indices,
                   uint64_t *pv_values, size_t *n_pv) {
    return smi_fri_verify_fs(ctx, cfg, nullptr, 0, proof, proof_len, accept, pv_indices, pv_values, n_pv, nullptr);
}

static int fri_verify_ext_impl(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint8_t *proof,
                               size_t proof_len, int *accept, uint64_t *pv_indices, uint64_t *pv_values, size_t *n_pv, size_t *consumed, int grind) {
    if (!ctx || !cfg || (!proof && proof_len) || !accept || (!transcript && transcript_len)) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    if (n_pv) *n_pv = 0;
    if (consumed) *consumed = 0;
    SMI_TRY(ext_field_check(ctx));
    SMI_TRY(smi_fri_check(ctx, cfg));
    FsSeed seed;
    hashc::fs_seed(transcript, transcript_len, seed.s, &seed.phase);
    size_t end = 0;
    const std::vector<Obj> objs = parse(proof, proof_len, (size_t)-1, &end);
    std::vector<uint64_t> pi, pv;
    size_t used = 0;
    const int rc = fri_verify_ext_objs(ctx, *cfg, seed, objs, accept, nullptr, &pi, &pv, nullptr, &used, grind);
    if (n_pv) *n_pv = pi.size();
    if (pv_indices && !pi.empty()) memcpy(pv_indices, pi.data(), 8 * pi.size());
    if (pv_values && !pv.empty()) memcpy(pv_values, pv.data(), 8 * pv.size());
    if (rc == SMI_OK && *accept && consumed) (void)parse(proof, proof_len, used, consumed);
    return rc;
}

int smi_fri_verify_ext(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint8_t *proof,
                       size_t proof_len, int *accept, uint64_t *pv_indices, uint64_t *pv_values, size_t *n_pv, size_t *consumed) {
    return fri_verify_ext_impl(ctx, cfg, transcript, transcript_len, proof, proof_len, accept, pv_indices, pv_values, n_pv, consumed, SMI_GRIND_NONE);
}
int smi_fri_verify_ext_pow(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint8_t *proof,
                           size_t proof_len, int *accept, uint64_t *pv_indices, uint64_t *pv_values, size_t *n_pv, size_t *consumed,
                           uint32_t grind_bits) {
    if (!ctx) return SMI_ERR_BAD_ARG;
    if (accept) *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    return fri_verify_ext_impl(ctx, cfg, transcript, transcript_len, proof, proof_len, accept, pv_indices, pv_values, n_pv, consumed, (int)grind_bits);
}

int smi_stark_verify(smi_ctx *ctx, const smi_stark_cfg *cfg, const uint8_t *column_roots, const uint8_t *proof, size_t proof_len,
                     int *accept) {
    if (!ctx || !cfg || !column_roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    const uint32_t W = cfg->n_cols, logN = cfg->log_n + cfg->log_blowup;
    if (!W || W > 64 || cfg->row_leaves) return smi_fail(ctx, SMI_ERR_BAD_ARG, "stark_verify: 1..64 column trees");
    // Without the column openings the proof is Fri::prove's bytes and nothing else: no relation to column_roots
    // could be checked, so nothing is "verified" here (include/stark_mi.h).
    if (!cfg->open_columns)
        return smi_fail(ctx, SMI_ERR_COLUMNS_NOT_BOUND, "stark_verify: proof made without open_columns; use smi_fri_verify for the FRI part");
    if (cfg->log_blowup < 2) return smi_fail(ctx, SMI_ERR_EXPANSION_TOO_SMALL, nullptr);
    if (logN > ctx->fs.K) return smi_fail(ctx, ctx->fs.F.p == 998244353u ? SMI_ERR_ROOT_TOO_LARGE : SMI_ERR_UNSUPPORTED_PRIME, "LDE domain too large");
    const uint64_t p = ctx->fs.F.p, N = 1ull << logN, t = cfg->num_colinearity_tests;
    smi_fri_cfg fc;
    fc.omega = h_root(ctx, logN);
    fc.offset = cfg->lde_offset;
    fc.domain_length = N;
    fc.expansion_factor = 1ull << cfg->log_blowup;
    fc.num_colinearity_tests = t;
    size_t end = 0;
    const std::vector<Obj> objs = parse(proof, proof_len, fri_object_count(fc), &end);
    std::vector<uint64_t> top, ab;
    size_t used = 0;
    SMI_TRY(fri_verify_objs(ctx, fc, fresh_seed(), objs, accept, &top, nullptr, nullptr, &ab, &used));
    if (!*accept) return SMI_OK;
    // ---- the column openings (mgpu_core.h layout): rows, then paths
    *accept = 0;
    const size_t rec = 9 + 8 * (size_t)W, prec = 9 + 32 * (size_t)logN, need = t * 2 * rec + t * W * 2 * prec;
    if (proof_len - end != need) return reject(ctx, accept, "column openings: wrong length");
    const uint8_t *ext = proof + end, *pathsb = ext + t * 2 * rec;
    // weight c = FiatShamir::challenge after absorbing roots[0..c] (fresh transcript)
    std::vector<uint64_t> weights(W);
    std::vector<uint8_t> transcript;
    for (uint32_t c = 0; c < W; c++) {
        transcript.insert(transcript.end(), column_roots + 32 * c, column_roots + 32 * c + 32);
        SMI_TRY(challenge_of(ctx, transcript, &weights[c]));
    }
    std::vector<uint64_t> rows(t * 2 * W);
    for (uint64_t s = 0; s < t; s++)
        for (int k = 0; k < 2; k++) {
            const uint8_t *r = ext + (2 * s + k) * rec;
            if (r[0] != 2 || get_u64(r + 1) != W) return reject(ctx, accept, "column openings: malformed row");
            uint64_t acc = 0;
            for (uint32_t c = 0; c < W; c++) {
                const uint64_t v = get_u64(r + 9 + 8 * c);
                rows[(2 * s + k) * W + c] = v;
                acc = (acc + mulm(weights[c] % p, v % p, p)) % p;
            }
            if (acc != ab[2 * s + k] % p) return reject(ctx, accept, "column openings: the weighted sum is not the codeword value");
        }
    const uint64_t half = N / 2;
    for (uint32_t c = 0; c < W; c++) {
        std::vector<uint64_t> vals(2 * t), idx(2 * t);
        std::vector<uint8_t> paths(2 * t * 32 * (size_t)logN), leaf, ok(2 * t ? 2 * t : 1);
        for (uint64_t s = 0; s < t; s++)
            for (int k = 0; k < 2; k++) {
                const uint8_t *pr = pathsb + ((s * W + c) * 2 + k) * prec;
                if (pr[0] != 3 || get_u64(pr + 1) != logN) return reject(ctx, accept, "column openings: malformed path");
                vals[2 * s + k] = rows[(2 * s + k) * W + c];
                idx[2 * s + k] = top[s] % half + (k ? half : 0);
                memcpy(&paths[(2 * s + k) * 32 * (size_t)logN], pr + 9, 32 * (size_t)logN);
            }
        SMI_TRY(leaf_digests(ctx, vals.data(), 2 * t, leaf));
        if (t) SMI_TRY(smi_merkle_verify_batch(ctx, leaf.data(), idx.data(), paths.data(), 2 * t, logN, column_roots + 32 * c, ok.data()));
        for (uint64_t s = 0; s < 2 * t; s++)
            if (!ok[s]) return reject(ctx, accept, "column openings: authentication path does not verify");
    }
    *accept = 1;
    return SMI_OK;
}

// Verifier of smi_dev_air_prove and smi_dev_air_prove_rows (include/stark_mi.h, "AIR"): the weights and FRI's seed from
// the variant's transcript, Fri::verify at expansion factor E, then the openings -- length, rows, every path against its
// root (W column roots, or the one root of the tree over the rows), and the composition codeword recomputed at x_a and
// x_b with the evaluator the prover's kernel runs (air_core.h) over the opened rows.  Only the transcript and the
// authentication of the opened rows differ between the two commitments; everything else is this one function.
// over_ext (with by_rows): weights from the quartic extension -- four counters and four challenges per weight, FRI over F_q, the
// four coordinates of the composition against the layer-0 triple's a and b (smi_air_verify_ext).
// grind (with over_ext): the proof-of-work difficulty demanded of the FRI part, or SMI_GRIND_NONE (smi_air_verify_ext_pow).
static int air_verify_impl(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air, const uint8_t *column_roots, const uint8_t *proof,
                           size_t proof_len, int *accept, bool by_rows, bool over_ext = false, int grind = SMI_GRIND_NONE) {
    std::string why;
    uint64_t E = 0;
    const int vrc = air_validate(ctx->fs.F.p, cfg, air, nullptr, &E, &why);
    if (vrc != SMI_OK) return smi_fail(ctx, vrc, why.c_str());
    const uint32_t W = cfg->n_cols, K = air->n_constraints, logN = cfg->log_n + cfg->log_blowup;
    if (logN > ctx->fs.K) return smi_fail(ctx, ctx->fs.F.p == 998244353u ? SMI_ERR_ROOT_TOO_LARGE : SMI_ERR_UNSUPPORTED_PRIME, "LDE domain too large");
    const uint64_t p = ctx->fs.F.p, N = 1ull << logN, B = 1ull << cfg->log_blowup, t = cfg->num_colinearity_tests;
    smi_fri_cfg fc;
    fc.omega = h_root(ctx, logN);
    fc.offset = cfg->lde_offset;
    fc.domain_length = N;
    fc.expansion_factor = E;
    fc.num_colinearity_tests = t;
    // transcript.  Column trees: root c, weight c; then k as 8 LE bytes, weight W + k.  Row tree: the root; then j = 0 ..
    // W + K - 1 as 8 LE bytes, weight j.
    const uint32_t NE = over_ext ? 4 : 1;   // coordinates per weight and per codeword value
    std::vector<uint64_t> weights((size_t)NE * (W + K));
    std::vector<uint8_t> transcript;
    auto absorb_index = [&](uint64_t j) {
        for (int i = 0; i < 8; i++) transcript.push_back((uint8_t)(j >> (8 * i)));
    };
    if (over_ext) {   // the root; then m = 0 .. 4 (W + K) - 1 as 8 LE bytes, challenge m = coordinate m mod 4 of weight m / 4
        transcript.assign(column_roots, column_roots + 32);
        for (uint32_t m = 0; m < 4 * (W + K); m++) {
            absorb_index(m);
            SMI_TRY(challenge_of(ctx, transcript, &weights[m]));
        }
    } else if (by_rows) {
        transcript.assign(column_roots, column_roots + 32);
        for (uint32_t j = 0; j < W + K; j++) {
            absorb_index(j);
            SMI_TRY(challenge_of(ctx, transcript, &weights[j]));
        }
    } else {
        for (uint32_t c = 0; c < W; c++) {
            transcript.insert(transcript.end(), column_roots + 32 * c, column_roots + 32 * c + 32);
            SMI_TRY(challenge_of(ctx, transcript, &weights[c]));
        }
        for (uint32_t k = 0; k < K; k++) {
            absorb_index(k);
            SMI_TRY(challenge_of(ctx, transcript, &weights[W + k]));
        }
    }
    FsSeed seed;
    hashc::fs_seed(transcript.data(), transcript.size(), seed.s, &seed.phase);
    size_t end = 0;
    const std::vector<Obj> objs = parse(proof, proof_len, fri_object_count(fc) + (grind != SMI_GRIND_NONE ? 1 : 0), &end);
    std::vector<uint64_t> top, ab;
    size_t used = 0;
    if (over_ext) SMI_TRY(fri_verify_ext_objs(ctx, fc, seed, objs, accept, &top, nullptr, nullptr, &ab, &used, grind));
    else SMI_TRY(fri_verify_objs(ctx, fc, seed, objs, accept, &top, nullptr, nullptr, &ab, &used));
    if (!*accept) return SMI_OK;
    *accept = 0;
    const size_t R = K ? 4 : 2, rec = 9 + 8 * (size_t)W, prec = 9 + 32 * (size_t)logN, need = t * R * rec + t * (by_rows ? 1 : W) * R * prec;
    if (proof_len - end != need) return reject(ctx, accept, "air openings: wrong length");
    const uint8_t *ext = proof + end, *pathsb = ext + t * R * rec;
    const uint64_t half = N / 2;
    std::vector<uint64_t> rows(t * R * W), pos(t * R);
    for (uint64_t s = 0; s < t; s++) {
        const uint64_t a = top[s] % half;
        const uint64_t ps[4] = {a, a + half, (a + B) & (N - 1), (a + half + B) & (N - 1)};
        for (size_t k = 0; k < R; k++) {
            const uint8_t *r = ext + (R * s + k) * rec;
            if (r[0] != 2 || get_u64(r + 1) != W) return reject(ctx, accept, "air openings: malformed row");
            pos[R * s + k] = ps[k];
            for (uint32_t c = 0; c < W; c++) rows[(R * s + k) * W + c] = get_u64(r + 9 + 8 * c);
        }
    }
    if (by_rows) {
        // one path per opened row; its leaf is the hash of the row's 8 W bytes as they stand in the proof
        const size_t m = R * t;
        std::vector<uint8_t> paths(m * 32 * (size_t)logN), leaf(32 * (m ? m : 1)), ok(m ? m : 1);
        for (size_t q = 0; q < m; q++) {
            const uint8_t *pr = pathsb + q * prec;
            if (pr[0] != 3 || get_u64(pr + 1) != logN) return reject(ctx, accept, "air openings: malformed path");
            memcpy(&paths[q * 32 * (size_t)logN], pr + 9, 32 * (size_t)logN);
            uint32_t d[8];
            hashc::hash_bytes(ext + q * rec + 9, 8 * (size_t)W, d);
            memcpy(&leaf[32 * q], d, 32);
        }
        if (m) SMI_TRY(smi_merkle_verify_batch(ctx, leaf.data(), pos.data(), paths.data(), m, logN, column_roots, ok.data()));
        for (size_t q = 0; q < m; q++)
            if (!ok[q]) return reject(ctx, accept, "air openings: authentication path does not verify");
    }
    for (uint32_t c = 0; c < W && !by_rows; c++) {
        const size_t m = R * t;
        std::vector<uint64_t> vals(m);
        std::vector<uint8_t> paths(m * 32 * (size_t)logN), leaf, ok(m ? m : 1);
        for (size_t q = 0; q < m; q++) {
            const uint8_t *pr = pathsb + (((q / R) * W + c) * R + q % R) * prec;
            if (pr[0] != 3 || get_u64(pr + 1) != logN) return reject(ctx, accept, "air openings: malformed path");
            vals[q] = rows[q * W + c];
            memcpy(&paths[q * 32 * (size_t)logN], pr + 9, 32 * (size_t)logN);
        }
        SMI_TRY(leaf_digests(ctx, vals.data(), m, leaf));
        if (m) SMI_TRY(smi_merkle_verify_batch(ctx, leaf.data(), pos.data(), paths.data(), m, logN, column_roots + 32 * c, ok.data()));
        for (size_t q = 0; q < m; q++)
            if (!ok[q]) return reject(ctx, accept, "air openings: authentication path does not verify");
    }
    // the composition codeword at x_a and x_b from the opened rows
    AirHost H;
    air_build(ctx->fs.F, (uint32_t)fc.omega, cfg, air, &H);
    const Fp F = ctx->fs.F;
    // the periodic operands at the 2 t positions and B further, from the statement alone: the tables the prover's
    // builder makes of it, gathered on the device (per[(2 s + k) * 2Q + ..]: Q at this row, Q at the next)
    const uint32_t Q = air->n_periodic;
    std::vector<uint32_t> per;
    if (Q) {
        std::vector<uint64_t> at(2 * t);
        for (uint64_t s = 0; s < t; s++)
            for (size_t k = 0; k < 2; k++) at[2 * s + k] = pos[R * s + k];
        SMI_TRY(air_periodic_at(ctx, cfg, H, at, &per));
    }
    std::vector<uint32_t> w_m(over_ext ? 4 * AIR_MAX_WEIGHTS : W + K, 0);   // over_ext: coordinate e of weight j at e * AIR_MAX_WEIGHTS + j
    for (uint32_t i = 0; i < NE * (W + K); i++) w_m[over_ext ? (i & 3) * AIR_MAX_WEIGHTS + (i >> 2) : i] = to_mont_u64(weights[i], F);
    for (uint64_t s = 0; s < t; s++)
        for (size_t k = 0; k < 2; k++) {
            const uint64_t i = pos[R * s + k];
            for (size_t r = k; r < R; r += 2)
                for (uint32_t c = 0; c < W; c++)
                    if (rows[(R * s + r) * W + c] >= p) return reject(ctx, accept, "air openings: an opened value is not canonical");
            const uint64_t *cur = &rows[(R * s + k) * W], *nxt = K ? &rows[(R * s + k + 2) * W] : nullptr;
            const uint32_t x_m = air_to_m((uint32_t)mulm(cfg->lde_offset, powm(fc.omega, i, p), p), (uint32_t)p), ib = (uint32_t)(i & (B - 1));
            auto operand = [&](int, uint32_t var) {   // AirDev::fac's numbering: W + Q operands at this row, then at the next
                const bool next = var >= W + Q;
                const uint32_t c = next ? var - (W + Q) : var;
                if (c >= W) return per[(2 * s + k) * 2 * Q + (next ? Q : 0) + (c - W)];
                return (uint32_t)(next ? nxt[c] : cur[c]);
            };
            uint32_t got[4] = {0, 0, 0, 0};
            if (over_ext) air_compose_points_ext<1>(H.dev, F, w_m.data(), &x_m, &ib, operand, got);
            else air_compose_points<1>(H.dev, F, w_m.data(), &x_m, &ib, operand, got);
            for (uint32_t e = 0; e < NE; e++)
                if (got[e] != ab[(2 * s + k) * NE + e] % p) return reject(ctx, accept, "air openings: the composition of the opened rows is not the codeword value");
        }
    *accept = 1;
    return SMI_OK;
}

int smi_air_verify(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t *column_roots, const uint8_t *proof,
                   size_t proof_len, int *accept) {
    if (!ctx || !cfg || !air || !column_roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    if (cfg->row_leaves) return smi_fail(ctx, SMI_ERR_BAD_ARG, "air_verify: column trees only (row_leaves must be 0; smi_air_verify_rows checks a proof over one row tree)");
    return air_verify_impl(ctx, cfg, (const smi_air *)air, column_roots, proof, proof_len, accept, false);
}

int smi_air_verify_rows(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t row_root[32], const uint8_t *proof,
                        size_t proof_len, int *accept) {
    if (!ctx || !cfg || !air || !row_root || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    return air_verify_impl(ctx, cfg, (const smi_air *)air, row_root, proof, proof_len, accept, true);
}

int smi_air_verify_ext(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t row_root[32], const uint8_t *proof,
                       size_t proof_len, int *accept) {
    if (!ctx || !cfg || !air || !row_root || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(ext_field_check(ctx));
    return air_verify_impl(ctx, cfg, (const smi_air *)air, row_root, proof, proof_len, accept, true, true);
}

int smi_air_verify_ext_pow(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t row_root[32], const uint8_t *proof,
                           size_t proof_len, int *accept, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !row_root || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    return air_verify_impl(ctx, cfg, (const smi_air *)air, row_root, proof, proof_len, accept, true, true, (int)grind_bits);
}

// Verifier of smi_dev_air_prove_perm (include/stark_mi.h, "Permutation argument"), in the order the header gives: the
// transcript of both roots; extension FRI with proof of work at E; the exact lengths, tags and widths of the two opening
// sections; the leaves from the bytes as they stand and every path against root_1 / root_2; the canonical check, z
// coordinates included; the composition at x_a and x_b -- the main part by air_compose_points_ext as smi_air_verify_ext runs
// it, the two auxiliary quotients in host F_q arithmetic (ext_mul_host) -- against the layer-0 triple.
int smi_air_verify_perm(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air_, const void *perm_, const uint8_t *roots, const uint8_t *proof,
                        size_t proof_len, int *accept, uint32_t grind_bits) {
    const smi_air *air = (const smi_air *)air_;
    const smi_air_perm *perm = (const smi_air_perm *)perm_;
    if (!ctx || !cfg || !air || !perm || !roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    std::string why;
    uint64_t E = 0;
    const int vrc = perm_plan(ctx->fs.F.p, cfg, air, perm, nullptr, &E, &why);
    if (vrc != SMI_OK) return smi_fail(ctx, vrc, why.c_str());
    const uint32_t W = cfg->n_cols, K = air->n_constraints, logN = cfg->log_n + cfg->log_blowup, NW = W + K + 2;
    if (logN > ctx->fs.K) return smi_fail(ctx, ctx->fs.F.p == 998244353u ? SMI_ERR_ROOT_TOO_LARGE : SMI_ERR_UNSUPPORTED_PRIME, "LDE domain too large");
    const uint64_t p = ctx->fs.F.p, N = 1ull << logN, B = 1ull << cfg->log_blowup, n = 1ull << cfg->log_n, t = cfg->num_colinearity_tests;
    const uint32_t p32 = (uint32_t)p, g = ctx->fs.g;
    smi_fri_cfg fc;
    fc.omega = h_root(ctx, logN);
    fc.offset = cfg->lde_offset;
    fc.domain_length = N;
    fc.expansion_factor = E;
    fc.num_colinearity_tests = t;
    // transcript: root_1; m = 0 .. 7; root_2; 8 + m for m = 0 .. 4 (W + K + 2) - 1
    std::vector<uint8_t> transcript(roots, roots + 32);
    auto absorb_index = [&](uint64_t j) {
        for (int i = 0; i < 8; i++) transcript.push_back((uint8_t)(j >> (8 * i)));
    };
    uint64_t ch[8];
    for (uint32_t m = 0; m < 8; m++) {
        absorb_index(m);
        SMI_TRY(challenge_of(ctx, transcript, &ch[m]));
    }
    transcript.insert(transcript.end(), roots + 32, roots + 64);
    std::vector<uint64_t> weights(4 * (size_t)NW);
    for (uint32_t m = 0; m < 4 * NW; m++) {
        absorb_index(8 + m);
        SMI_TRY(challenge_of(ctx, transcript, &weights[m]));
    }
    FsSeed seed;
    hashc::fs_seed(transcript.data(), transcript.size(), seed.s, &seed.phase);
    size_t end = 0;
    const std::vector<Obj> objs = parse(proof, proof_len, fri_object_count(fc) + 1, &end);
    std::vector<uint64_t> top, ab;
    size_t used = 0;
    SMI_TRY(fri_verify_ext_objs(ctx, fc, seed, objs, accept, &top, nullptr, nullptr, &ab, &used, (int)grind_bits));
    if (!*accept) return SMI_OK;
    *accept = 0;
    // ---- the two opening sections: rows of W values under root_1, rows of 4 values under root_2; R = 4 positions per test
    const size_t R = 4, prec = 9 + 32 * (size_t)logN, m_pos = R * t;
    const uint32_t widths[2] = {W, 4};
    const size_t sec_len[2] = {m_pos * (9 + 8 * (size_t)W) + m_pos * prec, m_pos * (9 + 8 * (size_t)4) + m_pos * prec};
    if (proof_len - end != sec_len[0] + sec_len[1]) return reject(ctx, accept, "perm openings: wrong length");
    const uint64_t half = N / 2;
    std::vector<uint64_t> pos(m_pos);
    for (uint64_t s = 0; s < t; s++) {
        const uint64_t a = top[s] % half;
        const uint64_t ps[4] = {a, a + half, (a + B) & (N - 1), (a + half + B) & (N - 1)};
        for (size_t k = 0; k < R; k++) pos[R * s + k] = ps[k];
    }
    std::vector<uint64_t> rows[2];
    const uint8_t *sec = proof + end;
    for (int v = 0; v < 2; v++) {   // tags and widths of every record of both sections first
        const size_t rec = 9 + 8 * (size_t)widths[v];
        const uint8_t *pathsb = sec + m_pos * rec;
        rows[v].resize(m_pos * widths[v]);
        for (size_t q = 0; q < m_pos; q++) {
            const uint8_t *r = sec + q * rec, *pr = pathsb + q * prec;
            if (r[0] != 2 || get_u64(r + 1) != widths[v]) return reject(ctx, accept, "perm openings: malformed row");
            if (pr[0] != 3 || get_u64(pr + 1) != logN) return reject(ctx, accept, "perm openings: malformed path");
            for (uint32_t c = 0; c < widths[v]; c++) rows[v][q * widths[v] + c] = get_u64(r + 9 + 8 * c);
        }
        sec += sec_len[v];
    }
    sec = proof + end;
    for (int v = 0; v < 2; v++) {   // leaves from the bytes as they stand, every path against its root
        const size_t rec = 9 + 8 * (size_t)widths[v];
        const uint8_t *pathsb = sec + m_pos * rec;
        std::vector<uint8_t> paths(m_pos * 32 * (size_t)logN), leaf(32 * (m_pos ? m_pos : 1)), ok(m_pos ? m_pos : 1);
        for (size_t q = 0; q < m_pos; q++) {
            memcpy(&paths[q * 32 * (size_t)logN], pathsb + q * prec + 9, 32 * (size_t)logN);
            uint32_t d[8];
            hashc::hash_bytes(sec + q * rec + 9, 8 * (size_t)widths[v], d);
            memcpy(&leaf[32 * q], d, 32);
        }
        if (m_pos) SMI_TRY(smi_merkle_verify_batch(ctx, leaf.data(), pos.data(), paths.data(), m_pos, logN, roots + 32 * v, ok.data()));
        for (size_t q = 0; q < m_pos; q++)
            if (!ok[q]) return reject(ctx, accept, "perm openings: authentication path does not verify");
        sec += sec_len[v];
    }
    for (int v = 0; v < 2; v++)
        for (uint64_t x : rows[v])
            if (x >= p) return reject(ctx, accept, "perm openings: an opened value is not canonical");
    // ---- the composition at x_a and x_b
    AirHost H;
    air_build(ctx->fs.F, (uint32_t)fc.omega, cfg, air, &H);
    const Fp F = ctx->fs.F;
    const uint32_t Q = air->n_periodic;
    std::vector<uint32_t> per;
    if (Q) {
        std::vector<uint64_t> at(2 * t);
        for (uint64_t s = 0; s < t; s++)
            for (size_t k = 0; k < 2; k++) at[2 * s + k] = pos[R * s + k];
        SMI_TRY(air_periodic_at(ctx, cfg, H, at, &per));
    }
    std::vector<uint32_t> w_m(4 * AIR_MAX_WEIGHTS, 0);
    for (uint32_t i = 0; i < 4 * (W + K); i++) w_m[(i & 3) * AIR_MAX_WEIGHTS + (i >> 2)] = to_mont_u64(weights[i], F);
    uint32_t alpha[4], gamma[4], wb[4], wt[4];
    perm_challenges(p32, ch, alpha, gamma);
    for (int e = 0; e < 4; e++) wb[e] = (uint32_t)(weights[4 * (W + K) + e] % p), wt[e] = (uint32_t)(weights[4 * (W + K + 1) + e] % p);
    std::vector<std::vector<uint32_t>> apow(perm->width, std::vector<uint32_t>(4, 0));
    {
        uint32_t pw[4] = {1, 0, 0, 0};
        for (uint32_t j = 0; j < perm->width; j++) {
            apow[j].assign(pw, pw + 4);
            ext_mul_host(p32, g, pw, alpha, pw);
        }
    }
    const uint64_t tau = cfg->trace_offset, tau_n = powm(tau, n, p);
    for (uint64_t s = 0; s < t; s++)
        for (size_t k = 0; k < 2; k++) {
            const uint64_t i = pos[R * s + k];
            const uint64_t *cur = &rows[0][(R * s + k) * W], *nxt = &rows[0][(R * s + k + 2) * W];
            const uint64_t *zc = &rows[1][(R * s + k) * 4], *zn = &rows[1][(R * s + k + 2) * 4];
            const uint64_t x = mulm(cfg->lde_offset, powm(fc.omega, i, p), p);
            const uint32_t x_m = air_to_m((uint32_t)x, p32), ib = (uint32_t)(i & (B - 1));
            auto operand = [&](int, uint32_t var) {
                const bool next = var >= W + Q;
                const uint32_t c = next ? var - (W + Q) : var;
                if (c >= W) return per[(2 * s + k) * 2 * Q + (next ? Q : 0) + (c - W)];
                return (uint32_t)(next ? nxt[c] : cur[c]);
            };
            uint32_t got[4] = {0, 0, 0, 0};
            air_compose_points_ext<1>(H.dev, F, w_m.data(), &x_m, &ib, operand, got);
            // the auxiliary quotients
            uint32_t fl[4], fr[4], z0[4], z1[4], a[4], b[4], bq[4], tq[4], u[4], v[4];
            for (int e = 0; e < 4; e++) fl[e] = fr[e] = gamma[e], z0[e] = (uint32_t)zc[e], z1[e] = (uint32_t)zn[e];
            for (uint32_t j = 0; j < perm->width; j++)
                for (int e = 0; e < 4; e++) {
                    fl[e] = (uint32_t)((fl[e] + mulm(apow[j][e], cur[perm->left_col[j]], p)) % p);
                    fr[e] = (uint32_t)((fr[e] + mulm(apow[j][e], cur[perm->right_col[j]], p)) % p);
                }
            ext_mul_host(p32, g, z1, fr, a);
            ext_mul_host(p32, g, z0, fl, b);
            const uint64_t izt = powm((powm(x, n, p) + p - tau_n) % p, p - 2, p), ixt = powm((x + p - tau) % p, p - 2, p);
            for (int e = 0; e < 4; e++) {
                tq[e] = (uint32_t)mulm((a[e] + p - b[e]) % p, izt, p);
                bq[e] = (uint32_t)mulm(e ? z0[e] : (z0[0] + p - 1) % p, ixt, p);
            }
            ext_mul_host(p32, g, bq, wb, u);
            ext_mul_host(p32, g, tq, wt, v);
            for (uint32_t e = 0; e < 4; e++) {
                const uint64_t want = ((uint64_t)got[e] + u[e] + v[e]) % p;
                if (want != ab[(2 * s + k) * 4 + e] % p) return reject(ctx, accept, "perm openings: the composition of the opened rows is not the codeword value");
            }
        }
    *accept = 1;
    return SMI_OK;
}
