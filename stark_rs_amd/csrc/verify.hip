// verify.hip -- Fri::verify (reference src/fri.rs:313-504) behind the C ABI, the verifier of the build-defined
// composition's column openings (smi_stark_cfg.open_columns), and the verifiers of the AIR proofs.
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
//
// Where a new proof variant plugs in.  There is one of each of these, and a variant states its differences instead of
// copying the walk:
//   * the transcript: a layout function in transcript_core.h, shared with the variant's prover;
//   * FRI: fri_walk, over an element kind (BaseFri / ExtFri) that supplies the record widths, the canonical rules and
//     their sentences, the leaf digests, the alpha draw, the last layer's degree test, the colinearity test, the rule of
//     the path stage and the optional nonce.  The two kinds differ ON PURPOSE (base follows the reference, unreduced
//     values included; the extension is stricter): a new rule is a new member of the kind, never an edit of the other;
//   * the openings: air_verify_impl over an AirVariant -- sections of row and path records (parse_section, in the
//     RecordOrder the variant names), their authentication (auth_section from the bytes as they stand, auth_column_trees
//     from the raw u64 on the device), the canonical check where the variant places it, and the composition at x_a and
//     x_b with the evaluator the prover's kernel runs.  The sentences come from the variant's OpeningWords.
// The order of the checks is part of the behaviour (it decides which sentence a proof with two defects gets);
// tests/golden/verify_verdicts.json records it for every verifier here.
#include <string.h>

#include <optional>
#include <vector>

#include "air_core.h"
#include "args_core.h"
#include "deep_core.h"
#include "xargs_core.h"
#include "zk_core.h"
#include "zkargs_core.h"
#include "fri_core.h"
#include "hash_core.h"
#include "internal.h"
#include "lookup_core.h"
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
// A verdict: *accept = 0 and the sentence.  Inside this file it travels up through SMI_TRY like a status; the entry
// points of the C ABI hand it out as SMI_OK (settle).
enum { REJECTED = 1 };
int reject(smi_ctx *ctx, int *accept, const char *why) {
    *accept = 0;
    ctx->err = why;
    return REJECTED;
}
int settle(int rc) { return rc == REJECTED ? SMI_OK : rc; }
// leaf digests of n elements of `width` bytes each as they stand in the proof, hashed in one device batch
int leaf_digests_dev(smi_ctx *ctx, const std::vector<const uint8_t *> &at, size_t width, std::vector<uint8_t> &out) {
    const size_t n = at.size();
    std::vector<uint8_t> msgs(width * n);
    for (size_t i = 0; i < n; i++) memcpy(&msgs[width * i], at[i], width);
    out.resize(32 * n);
    return n ? smi_hash_bytes_batch(ctx, msgs.data(), n, width, out.data()) : SMI_OK;
}
// ... hashed on the host
void leaf_digests_host(const std::vector<const uint8_t *> &at, size_t width, std::vector<uint8_t> &out) {
    out.resize(32 * at.size());
    for (size_t i = 0; i < at.size(); i++) {
        uint32_t d[8];
        hashc::hash_bytes(at[i], width, d);
        memcpy(&out[32 * i], d, 32);
    }
}
bool high_coefficients_zero(const std::vector<uint64_t> &coeffs, size_t degree_bound) {   // src/fri.rs:392-397: degree <= degree_bound - 1
    for (size_t i = degree_bound; i < coeffs.size(); i++)
        if (coeffs[i] != 0) return false;
    return true;
}
const char *const LOW_DEGREE = "last codeword does not correspond to polynomial of low enough degree";

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

// ---------------------------------------------------------------------------------------------- FRI
// The two element kinds of fri_walk.  A kind supplies: NE, the u64 values per element (a last codeword of NE n values,
// triples of 3 NE, NE alphas per round); where "No FRI roots extracted" is reported; the alpha draw; the shape rule of the
// last codeword; the leaf digests; the degree test of the last layer; the rule for the values of a triple; the colinearity
// test; whether the path stage stops at the first failing pop; the proof-of-work difficulty (or SMI_GRIND_NONE).

// FRI over F_p, to the letter of the reference -- unreduced values included
struct BaseFri {
    static constexpr uint32_t NE = 1;
    static constexpr bool no_rounds_before_pops = false;   // reported after the last-codeword pop (src/fri.rs:345-348)
    static constexpr bool stop_at_first_bad_pop = false;   // pops run up to the first one that fails; what was popped is verified
    static constexpr int grind = SMI_GRIND_NONE;
    // an alpha after every root, the last included (src/fri.rs:325-334)
    void draw(uint32_t fs[16], const uint32_t m[8], uint32_t phase, bool, std::vector<uint64_t> *alphas) const {
        uint64_t a = 0;
        hashc::fs_absorb_root_phase(fs, m, phase, nullptr, &a);
        alphas->push_back(a);
    }
    // the length is the record's; MerkleTree::new panics on these two (:353)
    int last_shape(smi_ctx *ctx, const Obj &lo, int *, size_t *n_last) const {
        *n_last = lo.count;
        if (lo.count == 0) return smi_fail(ctx, SMI_ERR_EMPTY_LEAVES, nullptr);
        if (!is_pow2(lo.count)) return smi_fail(ctx, SMI_ERR_LEAVES_NOT_POW2, nullptr);
        return SMI_OK;
    }
    // Hash::from_field_elements(&[v]) of the raw u64, on the device
    int leaves(smi_ctx *ctx, const std::vector<const uint8_t *> &at, std::vector<uint8_t> &out) const { return leaf_digests_dev(ctx, at, 8, out); }
    // inverse transform, forward re-evaluation (:384-390; an unreduced value cannot match it), high coefficients
    int low_degree(smi_ctx *ctx, int *accept, const uint8_t *vals, size_t n_last, uint64_t last_offset, size_t degree_bound) const {
        const uint64_t p = ctx->fs.F.p;
        std::vector<uint64_t> last(n_last);
        for (size_t i = 0; i < n_last; i++)
            if ((last[i] = get_u64(vals + 8 * i)) >= p) return reject(ctx, accept, "re-evaluated codeword does not match original!");
        std::vector<uint64_t> coeffs(n_last), re_eval(n_last);
        if (n_last > 1) {
            SMI_TRY(smi_intt(ctx, last.data(), coeffs.data(), ilog2(n_last), last_offset));
            SMI_TRY(smi_coset_ntt(ctx, coeffs.data(), n_last, re_eval.data(), ilog2(n_last), last_offset));
            if (re_eval != last) return reject(ctx, accept, "re-evaluated codeword does not match original!");
        } else {
            coeffs = last;
        }
        return high_coefficients_zero(coeffs, degree_bound) ? SMI_OK : reject(ctx, accept, LOW_DEGREE);
    }
    const char *triple_rule(const uint64_t *, uint64_t) const { return nullptr; }   // unreduced values are tolerated
    // test_colinearity (:507-525): (y1 - y0)(x2 - x0) == (y2 - y0)(x1 - x0); subm keeps the reference's wrap
    bool colinear(const smi_ctx *ctx, const uint64_t v[3], uint64_t ax, uint64_t bx, const uint64_t *alpha) const {
        const uint64_t p = ctx->fs.F.p, cx = alpha[0] % p;
        return mulm(subm(v[1], v[0], p), subm(cx, ax, p), p) == mulm(subm(v[2], v[0], p), subm(bx, ax, p), p);
    }
};

// FRI over the quartic extension (include/stark_mi.h, "Extension FRI"): this library's own format, and stricter
struct ExtFri {
    static constexpr uint32_t NE = 4;
    static constexpr bool no_rounds_before_pops = true;
    static constexpr bool stop_at_first_bad_pop = true;    // no earlier path is verified once a pop fails
    int grind;   // the least proof-of-work difficulty demanded (include/stark_mi.h, "Grinding"), or SMI_GRIND_NONE: no nonce record
    // four coordinates per round by fs_round_ext_lane; the last root is absorbed without drawing
    void draw(uint32_t fs[16], const uint32_t m[8], uint32_t phase, bool last, std::vector<uint64_t> *alphas) const {
        if (last) {
            hashc::fs_absorb_root_phase(fs, m, phase, nullptr, nullptr);
            return;
        }
        uint32_t out[16];
        for (int e = 0; e < 4; e++) {
            uint64_t a = 0;
            hashc::fs_round_ext_lane(fs, m, phase, e, out, &a);
            alphas->push_back(a);
        }
        memcpy(fs, out, sizeof out);
    }
    // four canonical values per element of the last domain (*n_last comes in as its length)
    int last_shape(smi_ctx *ctx, const Obj &lo, int *accept, size_t *n_last) const {
        if (lo.count != 4 * *n_last) return reject(ctx, accept, "last codeword: expected four values per element of the last domain");
        for (size_t i = 0; i < 4 * *n_last; i++)
            if (get_u64(lo.p + 8 * i) >= ctx->fs.F.p) return reject(ctx, accept, "last codeword: a coordinate is not canonical");
        return SMI_OK;
    }
    // Hash::from_field_elements of an element's four u64s as they stand in the proof, on the host
    int leaves(smi_ctx *, const std::vector<const uint8_t *> &at, std::vector<uint8_t> &out) const {
        leaf_digests_host(at, 32, out);
        return SMI_OK;
    }
    // EVERY coordinate is a base-field codeword on the last domain and must be of low degree; no re-evaluation
    int low_degree(smi_ctx *ctx, int *accept, const uint8_t *vals, size_t n_last, uint64_t last_offset, size_t degree_bound) const {
        for (int e = 0; e < 4; e++) {
            std::vector<uint64_t> col(n_last), coeffs(n_last);
            for (size_t i = 0; i < n_last; i++) col[i] = get_u64(vals + 8 * (4 * i + e));
            if (n_last > 1) SMI_TRY(smi_intt(ctx, col.data(), coeffs.data(), ilog2(n_last), last_offset));
            else coeffs = col;
            if (!high_coefficients_zero(coeffs, degree_bound)) return reject(ctx, accept, LOW_DEGREE);
        }
        return SMI_OK;
    }
    const char *triple_rule(const uint64_t *v, uint64_t p) const {
        for (int k = 0; k < 12; k++)
            if (v[k] >= p) return "triple: a coordinate is not canonical";
        return nullptr;
    }
    // (x_a, a), (-x_a, b), (alpha, c) colinear over F_q: (b - a)(alpha - x_a) == (c - a)(x_b - x_a), x_a and x_b in F_p
    bool colinear(const smi_ctx *ctx, const uint64_t w[12], uint64_t ax, uint64_t bx, const uint64_t *alpha) const {
        const uint32_t p = ctx->fs.F.p;
        uint32_t v[12], ba[4], ca[4], lhs[4];
        for (int k = 0; k < 12; k++) v[k] = (uint32_t)w[k];
        for (int e = 0; e < 4; e++) {
            ba[e] = fp_sub(v[4 + e], v[e], p);
            ca[e] = fp_sub(v[8 + e], v[e], p);
        }
        const uint32_t ax4[4] = {fp_sub((uint32_t)(alpha[0] % p), (uint32_t)ax, p), (uint32_t)(alpha[1] % p), (uint32_t)(alpha[2] % p), (uint32_t)(alpha[3] % p)};
        ext_mul_host(p, ctx->fs.g, ba, ax4, lhs);
        const uint32_t dx = fp_sub((uint32_t)bx, (uint32_t)ax, p);
        for (int e = 0; e < 4; e++)
            if (lhs[e] != host_mulmod(ca[e], dx, p)) return false;
        return true;
    }
};

// Two steps every walk below takes the same way (fri_walk, fri_walk_fold4).
// The last layer's domain after `squarings` squarings of (omega, offset) -> *last_offset.  The reference interpolates over
// the point list offset_L * omega_L^i; the transform needs that list to be the coset of the 2^k-th roots (any prover that
// folded a codeword over a proper domain has it).
int last_domain(smi_ctx *ctx, const smi_fri_cfg &cfg, uint64_t squarings, size_t n_last, uint64_t *last_offset) {
    const uint64_t p = ctx->fs.F.p;
    uint64_t last_omega = cfg.omega % p;
    *last_offset = cfg.offset % p;
    for (uint64_t i = 0; i < squarings; i++) {
        last_omega = mulm(last_omega, last_omega, p);
        *last_offset = mulm(*last_offset, *last_offset, p);
    }
    if (n_last > ((uint64_t)1 << ctx->fs.K) || last_omega != h_root(ctx, ilog2(n_last)) || *last_offset == 0)
        return smi_fail(ctx, SMI_ERR_NOT_GEOMETRIC, "Fri::verify: the last layer's domain is not offset * <primitive root>");
    return SMI_OK;
}
// The nonce record (`no`: the popped object, or nullptr): one u64 (not a field element), checked with one hash at the
// difficulty `grind`, then absorbed into fs; *seed_phase: the transcript's phase behind it.
int nonce_record(smi_ctx *ctx, int *accept, const Obj *no, uint32_t fs[16], uint32_t phase, int grind, uint32_t *seed_phase) {
    if (!no || no->tag != 2) return reject(ctx, accept, "proof of work: failed to extract the nonce");
    if (no->count != 1) return reject(ctx, accept, "proof of work: the nonce record must hold exactly one value");
    const uint64_t word = hashc::grind_word(fs, phase, get_u64(no->p), fs, seed_phase);
    if (word & ((1ull << (grind & 63)) - 1)) return reject(ctx, accept, "proof of work");
    return SMI_OK;
}

// Fri::verify on objs[0..] with the transcript the caller's FiatShamir holds (fs0, hash_core.h fs_seed); *used = objects
// consumed on acceptance.  The challenges continue the seed one root at a time instead of re-hashing the transcript.
// pv_val gets Kind::NE values per entry, layer0_ab 2 Kind::NE per test (a, then b).
template <class Kind>
int fri_walk(smi_ctx *ctx, const Kind &K, const smi_fri_cfg &cfg, const FsSeed &fs0, const std::vector<Obj> &objs, int *accept,
             std::vector<uint64_t> *top_out, std::vector<uint64_t> *pv_idx, std::vector<uint64_t> *pv_val, std::vector<uint64_t> *layer0_ab, size_t *used) {
    constexpr uint32_t NE = Kind::NE;
    const uint64_t p = ctx->fs.F.p, t = cfg.num_colinearity_tests, N = cfg.domain_length;
    uint64_t R = 0;
    smi_fri_num_rounds(&cfg, &R);
    if (Kind::no_rounds_before_pops && R == 0) return reject(ctx, accept, "No FRI roots extracted");
    size_t at = 0;
    auto pop = [&]() -> const Obj * { return at < objs.size() ? &objs[at++] : nullptr; };
    uint32_t fs[16];
    memcpy(fs, fs0.s, sizeof fs);
    std::vector<const uint8_t *> roots;
    std::vector<uint64_t> alphas;   // NE unreduced values per round
    for (uint64_t r = 0; r < R; r++) {                                             // src/fri.rs:325-334
        const Obj *o = pop();
        if (!o || o->tag != 0) return reject(ctx, accept, "Failed to extract Merkle root");
        roots.push_back(o->p);
        uint32_t m[8];
        memcpy(m, o->p, 32);   // little-endian words (proof bytes in order)
        K.draw(fs, m, fs0.phase, r + 1 == R, &alphas);
    }
    const Obj *lo = pop();                                                          // :337-342
    if (!lo || lo->tag != 2) return reject(ctx, accept, "Failed to extract last codeword");
    if (R == 0) return reject(ctx, accept, "No FRI roots extracted");               // :345-348
    size_t n_last = (size_t)(N >> (R - 1));
    SMI_TRY(K.last_shape(ctx, *lo, accept, &n_last));
    std::vector<const uint8_t *> elems(n_last);
    for (size_t i = 0; i < n_last; i++) elems[i] = lo->p + 8 * NE * i;
    std::vector<uint8_t> digests;
    SMI_TRY(K.leaves(ctx, elems, digests));
    uint8_t last_root[32];
    SMI_TRY(smi_merkle_commit(ctx, digests.data(), n_last, last_root));
    if (memcmp(last_root, roots.back(), 32) != 0) return reject(ctx, accept, "last codeword is not well formed");
    const size_t degree_bound = n_last / cfg.expansion_factor;                      // :360-365
    if (degree_bound == 0) return reject(ctx, accept, "last codeword too small");
    uint64_t last_offset = 0;
    SMI_TRY(last_domain(ctx, cfg, R - 1, n_last, &last_offset));
    SMI_TRY(K.low_degree(ctx, accept, lo->p, n_last, last_offset, degree_bound));
    uint32_t seed_phase = fs0.phase;
    if (K.grind != SMI_GRIND_NONE) SMI_TRY(nonce_record(ctx, accept, pop(), fs, fs0.phase, K.grind, &seed_phase));
    // index sampling (:400-405, :168-213)
    std::vector<uint64_t> top;
    SMI_TRY(sample_top(ctx, hashc::fs_challenge_phase(fs, seed_phase), N >> 1, N >> (R - 1), t, &top));
    if (top_out) *top_out = top;

    uint64_t om = cfg.omega % p, off = cfg.offset % p;
    for (uint64_t r = 0; r + 1 < R; r++) {                                          // :408-502
        const uint64_t half = N >> (r + 1);
        std::vector<uint64_t> ci(t), bi(t);
        std::vector<const uint8_t *> rec(t);   // the triples' payloads: a, b, c of NE u64 each
        for (uint64_t s = 0; s < t; s++) {
            ci[s] = top[s] % half;
            bi[s] = ci[s] + half;
            const Obj *o = pop();
            if (!o || o->tag != 2) return reject(ctx, accept, "Failed to extract triple values");
            if (o->count != 3 * NE) return reject(ctx, accept, "Expected triple of values");
            rec[s] = o->p;
            uint64_t v[3 * NE];
            for (uint32_t k = 0; k < 3 * NE; k++) v[k] = get_u64(o->p + 8 * k);
            if (const char *why = K.triple_rule(v, p)) return reject(ctx, accept, why);
            if (r == 0) {
                if (pv_idx && pv_val) {
                    pv_idx->push_back(ci[s]); pv_val->insert(pv_val->end(), v, v + NE);
                    pv_idx->push_back(bi[s]); pv_val->insert(pv_val->end(), v + NE, v + 2 * NE);
                }
                if (layer0_ab) layer0_ab->insert(layer0_ab->end(), v, v + 2 * NE);
            }
            const uint64_t ax = mulm(off, powm(om, ci[s], p), p), bx = mulm(off, powm(om, bi[s], p), p);
            if (!K.colinear(ctx, v, ax, bx, &alphas[NE * r])) return reject(ctx, accept, "colinearity check failure");
        }
        // The 3t authentication paths.  The reference pops and verifies them one at a time in the order
        // (test 0: a, b, c), (test 1: a, b, c), ... and stops at the first failure of either kind; here the paths
        // are verified in one device batch per (a, b, c), so the pops run first, up to the first one that fails,
        // and the verdict is the earliest failure in the reference's order -- unless the kind stops at that pop.
        static const char *const miss[3] = {"Failed to extract path for aa", "Failed to extract path for bb", "Failed to extract path for cc"};
        static const char *const bad[3] = {"merkle authentication path verification fails for aa", "merkle authentication path verification fails for bb",
                                           "merkle authentication path verification fails for cc"};
        const uint32_t want_depth[3] = {ilog2(2 * half), ilog2(2 * half), ilog2(half)};
        std::vector<std::vector<uint8_t>> paths(3);
        std::vector<std::vector<const uint8_t *>> elem(3);   // the a / b / c whose path was popped
        uint64_t first_bad = 3 * t;                           // position (3 s + w) of the first pop that failed
        const char *why = nullptr;
        for (uint64_t s = 0; s < t && !why; s++)
            for (int w = 0; w < 3; w++) {
                const Obj *o = pop();
                if (!o || o->tag != 3) { first_bad = 3 * s + w; why = miss[w]; break; }
                if (o->count != want_depth[w]) { first_bad = 3 * s + w; why = bad[w]; break; }   // wrong length: the recomputed root cannot match
                paths[w].insert(paths[w].end(), o->p, o->p + 32 * o->count);
                elem[w].push_back(rec[s] + 8 * NE * w);
            }
        if (why && Kind::stop_at_first_bad_pop) return reject(ctx, accept, why);
        const std::vector<uint64_t> *idxs[3] = {&ci, &bi, &ci};
        const uint8_t *rt[3] = {roots[r], roots[r], roots[r + 1]};
        for (int w = 0; w < 3; w++) {
            const uint64_t k = elem[w].size();
            if (!k) continue;
            std::vector<uint8_t> leaf, ok(k);
            SMI_TRY(K.leaves(ctx, elem[w], leaf));
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
// the walk under its two names: FRI over F_p, and over the quartic extension at a demanded difficulty
int fri_verify_objs(smi_ctx *ctx, const smi_fri_cfg &cfg, const FsSeed &fs0, const std::vector<Obj> &objs, int *accept, std::vector<uint64_t> *top_out,
                    std::vector<uint64_t> *pv_idx, std::vector<uint64_t> *pv_val, std::vector<uint64_t> *layer0_ab, size_t *used) {
    return fri_walk(ctx, BaseFri{}, cfg, fs0, objs, accept, top_out, pv_idx, pv_val, layer0_ab, used);
}
int fri_verify_ext_objs(smi_ctx *ctx, const smi_fri_cfg &cfg, const FsSeed &fs0, const std::vector<Obj> &objs, int *accept, std::vector<uint64_t> *top_out,
                        std::vector<uint64_t> *pv_idx, std::vector<uint64_t> *pv_val, std::vector<uint64_t> *layer0_ab, size_t *used, int grind) {
    return fri_walk(ctx, ExtFri{grind}, cfg, fs0, objs, accept, top_out, pv_idx, pv_val, layer0_ab, used);
}
// ---- extension FRI at folding factor 4 (include/stark_mi.h, "Extension FRI, folding factor 4")
// The walk differs from fri_walk in its shape -- F + 1 roots, one coset record and one path per (test, layer), no c -- so it
// is a walk of its own over ExtFri's rules: the draw, the last codeword's shape and degree, the nonce.  Where a check is
// fri_walk's, the sentence is fri_walk's (a coset record plays the triple's part); the one new sentence is FOLD4_MISMATCH.
const char *const FOLD4_MISMATCH = FRI_FOLD4_MISMATCH_SENTENCE;   // fri_core.h

// 2^-1 (lo + hi) + alpha ((lo - hi) 2^-1 x^-1) on plain residues; alpha reduced
void fold_pair_host(uint32_t p, uint32_t g, const uint32_t lo[4], const uint32_t hi[4], uint32_t x_inv, const uint32_t alpha[4], uint32_t out[4]) {
    const uint32_t inv2 = (p + 1) / 2, t = host_mulmod(inv2, x_inv, p);
    uint32_t d[4], ad[4];
    for (int e = 0; e < 4; e++) d[e] = host_mulmod(fp_sub(lo[e], hi[e], p), t, p);
    ext_mul_host(p, g, d, alpha, ad);
    for (int e = 0; e < 4; e++) out[e] = fp_add(host_mulmod(fp_add(lo[e], hi[e], p), inv2, p), ad[e], p);
}
// the fold by 4 of one coset record (16 values, 4 e + j = coordinate e of slot j) at x = the point of slot 0, iota = omega^q
void fold4_host(uint32_t p, uint32_t g, const uint64_t rec[16], uint32_t x, uint32_t iota, const uint64_t *alpha_raw, uint32_t out[4]) {
    uint32_t c[4][4], a1[4], a2[4], y0[4], y1[4];
    for (int j = 0; j < 4; j++)
        for (int e = 0; e < 4; e++) c[j][e] = (uint32_t)rec[4 * e + j];
    for (int e = 0; e < 4; e++) a1[e] = (uint32_t)(alpha_raw[e] % p);
    ext_mul_host(p, g, a1, a1, a2);
    const uint32_t x_inv = host_powmod(x, p - 2, p), iota_inv = host_powmod(iota, p - 2, p);
    fold_pair_host(p, g, c[0], c[2], x_inv, a1, y0);
    fold_pair_host(p, g, c[1], c[3], host_mulmod(x_inv, iota_inv, p), a1, y1);
    fold_pair_host(p, g, y0, y1, host_mulmod(x_inv, x_inv, p), a2, out);
}

// pv_idx / pv_val: the layer-0 cosets, four entries per test (element i + j q_0, j = 0 .. 3) of four values each;
// layer0: the 16 values of each layer-0 record as they stand
int fri_walk_fold4(smi_ctx *ctx, const smi_fri_cfg &cfg, const FsSeed &fs0, const std::vector<Obj> &objs, int *accept, std::vector<uint64_t> *top_out,
                   std::vector<uint64_t> *pv_idx, std::vector<uint64_t> *pv_val, std::vector<uint64_t> *layer0, size_t *used, uint32_t grind) {
    const ExtFri K{(int)grind};
    const uint32_t p = ctx->fs.F.p, g = ctx->fs.g;
    const uint64_t t = cfg.num_colinearity_tests, N = cfg.domain_length;
    const FriFold4Layout lay = fri_layout_fold4(cfg);
    const uint64_t F = lay.F;
    if (lay.R2 == 0) return reject(ctx, accept, "No FRI roots extracted");
    if (N < 4) return reject(ctx, accept, "last codeword too small");
    size_t at = 0;
    auto pop = [&]() -> const Obj * { return at < objs.size() ? &objs[at++] : nullptr; };
    uint32_t fs[16];
    memcpy(fs, fs0.s, sizeof fs);
    std::vector<const uint8_t *> roots;
    std::vector<uint64_t> alphas;   // four unreduced values per fold
    for (uint64_t r = 0; r <= F; r++) {
        const Obj *o = pop();
        if (!o || o->tag != 0) return reject(ctx, accept, "Failed to extract Merkle root");
        roots.push_back(o->p);
        uint32_t m[8];
        memcpy(m, o->p, 32);
        K.draw(fs, m, fs0.phase, r == F, &alphas);
    }
    const Obj *lo = pop();
    if (!lo || lo->tag != 2) return reject(ctx, accept, "Failed to extract last codeword");
    size_t n_last = (size_t)lay.last_n;
    SMI_TRY(K.last_shape(ctx, *lo, accept, &n_last));
    // the last tree: n_last / 4 coset leaves, leaf i = the 16 values (coordinate outer, slot inner) of elements i + j q
    const size_t q_last = n_last / 4;
    std::vector<uint8_t> leaf_msgs(128 * q_last), digests(32 * q_last);
    for (size_t i = 0; i < q_last; i++)
        for (int e = 0; e < 4; e++)
            for (int j = 0; j < 4; j++) memcpy(&leaf_msgs[128 * i + 8 * (4 * e + j)], lo->p + 8 * (4 * (i + j * q_last) + e), 8);
    for (size_t i = 0; i < q_last; i++) {
        uint32_t d[8];
        hashc::hash_bytes(&leaf_msgs[128 * i], 128, d);
        memcpy(&digests[32 * i], d, 32);
    }
    uint8_t last_root[32];
    SMI_TRY(smi_merkle_commit(ctx, digests.data(), q_last, last_root));
    if (memcmp(last_root, roots.back(), 32) != 0) return reject(ctx, accept, "last codeword is not well formed");
    const size_t degree_bound = n_last / cfg.expansion_factor;
    if (degree_bound == 0) return reject(ctx, accept, "last codeword too small");
    uint64_t last_offset = 0;
    SMI_TRY(last_domain(ctx, cfg, 2 * F, n_last, &last_offset));   // a fold by 4 squares the domain twice
    SMI_TRY(K.low_degree(ctx, accept, lo->p, n_last, last_offset, degree_bound));
    uint32_t seed_phase = fs0.phase;
    SMI_TRY(nonce_record(ctx, accept, pop(), fs, fs0.phase, (int)grind, &seed_phase));   // always present
    std::vector<uint64_t> top;
    SMI_TRY(sample_top(ctx, hashc::fs_challenge_phase(fs, seed_phase), F ? N >> 2 : N, n_last, t, &top));
    if (top_out) *top_out = top;

    uint64_t om = cfg.omega % p, off = cfg.offset % p;
    std::vector<uint32_t> folded(4 * t);   // the fold of the previous layer's coset, per test
    for (uint64_t r = 0; r < F; r++) {
        const uint64_t q = N >> (2 * r + 2);
        std::vector<uint64_t> idx(t);
        std::vector<const uint8_t *> rec(t);
        std::vector<uint64_t> vals(16 * t);
        for (uint64_t s = 0; s < t; s++) {
            idx[s] = top[s] % q;
            const Obj *o = pop();
            if (!o || o->tag != 2) return reject(ctx, accept, "Failed to extract triple values");
            if (o->count != 16) return reject(ctx, accept, "Expected triple of values");
            rec[s] = o->p;
            uint64_t *v = &vals[16 * s];
            for (int k = 0; k < 16; k++)
                if ((v[k] = get_u64(o->p + 8 * k)) >= p) return reject(ctx, accept, "triple: a coordinate is not canonical");
            if (r == 0) {
                if (pv_idx && pv_val)
                    for (int j = 0; j < 4; j++) {
                        pv_idx->push_back(idx[s] + j * q);
                        for (int e = 0; e < 4; e++) pv_val->push_back(v[4 * e + j]);
                    }
                if (layer0) layer0->insert(layer0->end(), v, v + 16);
            }
        }
        if (r > 0)   // the previous layer's fold is slot j = i_{r-1} div q of this layer's coset
            for (uint64_t s = 0; s < t; s++) {
                const uint64_t j = (top[s] % (4 * q)) / q;
                for (int e = 0; e < 4; e++)
                    if (vals[16 * s + 4 * e + j] != folded[4 * s + e]) return reject(ctx, accept, FOLD4_MISMATCH);
            }
        const uint32_t depth = ilog2(q);
        std::vector<uint8_t> paths, leaf, ok(t);
        for (uint64_t s = 0; s < t; s++) {
            const Obj *o = pop();
            if (!o || o->tag != 3) return reject(ctx, accept, "Failed to extract path for aa");
            if (o->count != depth) return reject(ctx, accept, "merkle authentication path verification fails for aa");
            paths.insert(paths.end(), o->p, o->p + 32 * o->count);
        }
        leaf_digests_host(rec, 128, leaf);   // the record as it stands is the leaf
        if (t) {
            if (depth) SMI_TRY(smi_merkle_verify_batch(ctx, leaf.data(), idx.data(), paths.data(), t, depth, roots[r], ok.data()));
            else
                for (uint64_t s = 0; s < t; s++) ok[s] = memcmp(&leaf[32 * s], roots[r], 32) == 0;
        }
        for (uint64_t s = 0; s < t; s++)
            if (!ok[s]) return reject(ctx, accept, "merkle authentication path verification fails for aa");
        const uint32_t iota = (uint32_t)powm(om, q, p);
        for (uint64_t s = 0; s < t; s++)
            fold4_host(p, g, &vals[16 * s], (uint32_t)mulm(off, powm(om, idx[s], p), p), iota, &alphas[4 * r], &folded[4 * s]);
        for (int k = 0; k < 2; k++) {
            om = mulm(om, om, p);
            off = mulm(off, off, p);
        }
    }
    if (F)   // the last fold is entry i_{F-1} of the last codeword
        for (uint64_t s = 0; s < t; s++) {
            const uint64_t i = top[s] % n_last;
            for (int e = 0; e < 4; e++)
                if (get_u64(lo->p + 8 * (4 * i + e)) != folded[4 * s + e]) return reject(ctx, accept, FOLD4_MISMATCH);
        }
    *accept = 1;
    if (used) *used = at;
    return SMI_OK;
}
size_t fri_object_count_fold4(const smi_fri_cfg &cfg) {
    const FriFold4Layout lay = fri_layout_fold4(cfg);
    return (size_t)(lay.F + 1 + 2 + lay.F * 2 * cfg.num_colinearity_tests);
}

size_t fri_object_count(const smi_fri_cfg &cfg) {
    uint64_t R = 0;
    smi_fri_num_rounds(&cfg, &R);
    return (size_t)(R + 1 + (R ? R - 1 : 0) * 4 * cfg.num_colinearity_tests);
}

// the entry points of FRI verification: the caller's transcript, the walk of the element kind, what the C ABI hands out
int fri_verify_abi(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint8_t *proof, size_t proof_len,
                   int *accept, uint64_t *pv_indices, uint64_t *pv_values, size_t *n_pv, size_t *consumed, bool ext, int grind) {
    if (!ctx || !cfg || (!proof && proof_len) || !accept || (!transcript && transcript_len)) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    if (n_pv) *n_pv = 0;
    if (consumed) *consumed = 0;
    if (ext) SMI_TRY(ext_field_check(ctx));
    SMI_TRY(smi_fri_check(ctx, cfg));
    const FsSeed seed = fs_seed_of(transcript, transcript_len);
    size_t end = 0;
    const std::vector<Obj> objs = parse(proof, proof_len, (size_t)-1, &end);
    std::vector<uint64_t> pi, pv;
    size_t used = 0;
    const int rc = ext ? fri_verify_ext_objs(ctx, *cfg, seed, objs, accept, nullptr, &pi, &pv, nullptr, &used, grind)
                       : fri_verify_objs(ctx, *cfg, seed, objs, accept, nullptr, &pi, &pv, nullptr, &used);
    if (n_pv) *n_pv = pi.size();       // like the reference's &mut Vec: what was pushed before a rejection stays
    if (pv_indices && !pi.empty()) memcpy(pv_indices, pi.data(), 8 * pi.size());
    if (pv_values && !pv.empty()) memcpy(pv_values, pv.data(), 8 * pv.size());
    if (rc == SMI_OK && *accept && consumed) (void)parse(proof, proof_len, used, consumed);   // the bytes of the popped objects
    return settle(rc);
}

// ---------------------------------------------------------------------------------------------- openings
// the sentences of one family of opening sections; `composition` is the family's own last check
struct OpeningWords {
    const char *length, *row, *path, *auth, *canonical, *composition;
};
const OpeningWords COLUMN_WORDS = {"column openings: wrong length", "column openings: malformed row", "column openings: malformed path",
                                   "column openings: authentication path does not verify", nullptr,
                                   "column openings: the weighted sum is not the codeword value"};
const OpeningWords AIR_WORDS = {"air openings: wrong length", "air openings: malformed row", "air openings: malformed path",
                                "air openings: authentication path does not verify", "air openings: an opened value is not canonical",
                                "air openings: the composition of the opened rows is not the codeword value"};
const OpeningWords LOOKUP_WORDS = {LOOKUP_SENTENCES[0], LOOKUP_SENTENCES[1], LOOKUP_SENTENCES[2], LOOKUP_SENTENCES[3], LOOKUP_SENTENCES[4], LOOKUP_SENTENCES[5]};   // lookup_core.h
const OpeningWords ARGS_WORDS = {ARGS_SENTENCES[0], ARGS_SENTENCES[1], ARGS_SENTENCES[2], ARGS_SENTENCES[3], ARGS_SENTENCES[4], ARGS_SENTENCES[5]};   // args_core.h
const OpeningWords PERM_WORDS = {"perm openings: wrong length", "perm openings: malformed row", "perm openings: malformed path",
                                 "perm openings: authentication path does not verify", "perm openings: an opened value is not canonical",
                                 "perm openings: the composition of the opened rows is not the codeword value"};

int domain_check(smi_ctx *ctx, uint32_t logN) {
    if (logN > ctx->fs.K) return smi_fail(ctx, ctx->fs.F.p == 998244353u ? SMI_ERR_ROOT_TOO_LARGE : SMI_ERR_UNSUPPORTED_PRIME, "LDE domain too large");
    return SMI_OK;
}
// the R positions a test opens: a, b = a + N/2, and with R = 4 the rows B further (the next trace row), mod N
std::vector<uint64_t> opened_positions(const std::vector<uint64_t> &top, uint64_t N, uint64_t B, size_t R) {
    std::vector<uint64_t> pos(R * top.size());
    for (size_t s = 0; s < top.size(); s++) {
        const uint64_t a = top[s] % (N / 2);
        const uint64_t ps[4] = {a, a + N / 2, (a + B) & (N - 1), (a + N / 2 + B) & (N - 1)};
        for (size_t k = 0; k < R; k++) pos[R * s + k] = ps[k];
    }
    return pos;
}
// One section: m row records (tag 2) of w values, then its path records (tag 3) of logN digests.  The order in which the
// tags and widths are checked is the caller's: the rows alone (the paths of column trees are checked tree by tree,
// auth_column_trees), every row and then every path, or record by record (row q, then path q).
enum RecordOrder { ROWS_ONLY, ROWS_THEN_PATHS, RECORD_BY_RECORD };
int parse_section(smi_ctx *ctx, int *accept, const OpeningWords &say, const uint8_t *sec, size_t m, uint32_t w, uint32_t logN, RecordOrder order,
                  std::vector<uint64_t> *vals) {
    const size_t rec = 9 + 8 * (size_t)w, prec = 9 + 32 * (size_t)logN;
    const uint8_t *paths = sec + m * rec;
    auto path_ok = [&](size_t q) { return paths[q * prec] == 3 && get_u64(paths + q * prec + 1) == logN; };
    vals->resize(m * w);
    for (size_t q = 0; q < m; q++) {
        const uint8_t *r = sec + q * rec;
        if (r[0] != 2 || get_u64(r + 1) != w) return reject(ctx, accept, say.row);
        if (order == RECORD_BY_RECORD && !path_ok(q)) return reject(ctx, accept, say.path);
        for (uint32_t c = 0; c < w; c++) (*vals)[q * w + c] = get_u64(r + 9 + 8 * c);
    }
    for (size_t q = 0; q < m && order == ROWS_THEN_PATHS; q++)
        if (!path_ok(q)) return reject(ctx, accept, say.path);
    return SMI_OK;
}
// a parsed section against the one root of a tree over rows: leaf q is the hash of row q's 8 w bytes as they stand in
// the proof, one path per opened row
int auth_section(smi_ctx *ctx, int *accept, const OpeningWords &say, const uint8_t *sec, size_t m, uint32_t w, uint32_t logN,
                 const std::vector<uint64_t> &pos, const uint8_t *root) {
    const size_t rec = 9 + 8 * (size_t)w, prec = 9 + 32 * (size_t)logN;
    std::vector<const uint8_t *> at(m);
    std::vector<uint8_t> paths(m * 32 * (size_t)logN), leaf, ok(m ? m : 1);
    for (size_t q = 0; q < m; q++) {
        at[q] = sec + q * rec + 9;
        memcpy(&paths[q * 32 * (size_t)logN], sec + m * rec + q * prec + 9, 32 * (size_t)logN);
    }
    leaf_digests_host(at, 8 * (size_t)w, leaf);
    if (m) SMI_TRY(smi_merkle_verify_batch(ctx, leaf.data(), pos.data(), paths.data(), m, logN, root, ok.data()));
    for (size_t q = 0; q < m; q++)
        if (!ok[q]) return reject(ctx, accept, say.auth);
    return SMI_OK;
}
// the rows of a section against W column trees, tree by tree: the path records of tree c at ((s W + c) R + k), their tags,
// then the leaves from the raw u64 on the device (an unreduced value hashes as the reference hashes it) and one batch
int auth_column_trees(smi_ctx *ctx, int *accept, const OpeningWords &say, const uint8_t *pathsb, const std::vector<uint64_t> &vals, size_t m, size_t R,
                      uint32_t W, uint32_t logN, const std::vector<uint64_t> &pos, const uint8_t *roots) {
    const size_t prec = 9 + 32 * (size_t)logN;
    for (uint32_t c = 0; c < W; c++) {
        std::vector<uint8_t> raw(8 * m), paths(m * 32 * (size_t)logN), leaf(32 * (m ? m : 1)), ok(m ? m : 1);
        for (size_t q = 0; q < m; q++) {
            const uint8_t *pr = pathsb + (((q / R) * W + c) * R + q % R) * prec;
            if (pr[0] != 3 || get_u64(pr + 1) != logN) return reject(ctx, accept, say.path);
            for (int k = 0; k < 8; k++) raw[8 * q + k] = (uint8_t)(vals[q * W + c] >> (8 * k));
            memcpy(&paths[q * 32 * (size_t)logN], pr + 9, 32 * (size_t)logN);
        }
        if (m) SMI_TRY(smi_hash_bytes_batch(ctx, raw.data(), m, 8, leaf.data()));
        if (m) SMI_TRY(smi_merkle_verify_batch(ctx, leaf.data(), pos.data(), paths.data(), m, logN, roots + 32 * c, ok.data()));
        for (size_t q = 0; q < m; q++)
            if (!ok[q]) return reject(ctx, accept, say.auth);
    }
    return SMI_OK;
}
}  // namespace

int smi_fri_verify_fs(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint8_t *proof,
                      size_t proof_len, int *accept, uint64_t *pv_indices, uint64_t *pv_values, size_t *n_pv, size_t *consumed) {
    return fri_verify_abi(ctx, cfg, transcript, transcript_len, proof, proof_len, accept, pv_indices, pv_values, n_pv, consumed, false, SMI_GRIND_NONE);
}
int smi_fri_verify(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *proof, size_t proof_len, int *accept, uint64_t *pv_indices,
                   uint64_t *pv_values, size_t *n_pv) {
    return smi_fri_verify_fs(ctx, cfg, nullptr, 0, proof, proof_len, accept, pv_indices, pv_values, n_pv, nullptr);
}
int smi_fri_verify_ext(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint8_t *proof,
                       size_t proof_len, int *accept, uint64_t *pv_indices, uint64_t *pv_values, size_t *n_pv, size_t *consumed) {
    return fri_verify_abi(ctx, cfg, transcript, transcript_len, proof, proof_len, accept, pv_indices, pv_values, n_pv, consumed, true, SMI_GRIND_NONE);
}
int smi_fri_verify_ext_pow(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint8_t *proof,
                           size_t proof_len, int *accept, uint64_t *pv_indices, uint64_t *pv_values, size_t *n_pv, size_t *consumed,
                           uint32_t grind_bits) {
    if (!ctx) return SMI_ERR_BAD_ARG;
    if (accept) *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    return fri_verify_abi(ctx, cfg, transcript, transcript_len, proof, proof_len, accept, pv_indices, pv_values, n_pv, consumed, true, (int)grind_bits);
}
int smi_fri_verify_ext_fold4(smi_ctx *ctx, const smi_fri_cfg *cfg, const uint8_t *transcript, size_t transcript_len, const uint8_t *proof,
                             size_t proof_len, int *accept, uint64_t *pv_indices, uint64_t *pv_values, size_t *n_pv, size_t *consumed,
                             uint32_t grind_bits) {
    if (!ctx) return SMI_ERR_BAD_ARG;
    if (accept) *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    if (!cfg || (!proof && proof_len) || !accept || (!transcript && transcript_len)) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (n_pv) *n_pv = 0;
    if (consumed) *consumed = 0;
    SMI_TRY(ext_field_check(ctx));
    SMI_TRY(smi_fri_check(ctx, cfg));
    const FsSeed seed = fs_seed_of(transcript, transcript_len);
    size_t end = 0;
    const std::vector<Obj> objs = parse(proof, proof_len, (size_t)-1, &end);
    std::vector<uint64_t> pi, pv;
    size_t used = 0;
    const int rc = fri_walk_fold4(ctx, *cfg, seed, objs, accept, nullptr, &pi, &pv, nullptr, &used, grind_bits);
    if (n_pv) *n_pv = pi.size();
    if (pv_indices && !pi.empty()) memcpy(pv_indices, pi.data(), 8 * pi.size());
    if (pv_values && !pv.empty()) memcpy(pv_values, pv.data(), 8 * pv.size());
    if (rc == SMI_OK && *accept && consumed) (void)parse(proof, proof_len, used, consumed);
    return settle(rc);
}

static int stark_verify_impl(smi_ctx *ctx, const smi_stark_cfg *cfg, const uint8_t *column_roots, const uint8_t *proof, size_t proof_len, int *accept) {
    const uint32_t W = cfg->n_cols, logN = cfg->log_n + cfg->log_blowup;
    if (!W || W > 64 || cfg->row_leaves) return smi_fail(ctx, SMI_ERR_BAD_ARG, "stark_verify: 1..64 column trees");
    // Without the column openings the proof is Fri::prove's bytes and nothing else: no relation to column_roots
    // could be checked, so nothing is "verified" here (include/stark_mi.h).
    if (!cfg->open_columns)
        return smi_fail(ctx, SMI_ERR_COLUMNS_NOT_BOUND, "stark_verify: proof made without open_columns; use smi_fri_verify for the FRI part");
    if (cfg->log_blowup < 2) return smi_fail(ctx, SMI_ERR_EXPANSION_TOO_SMALL, nullptr);
    SMI_TRY(domain_check(ctx, logN));
    const uint64_t p = ctx->fs.F.p, N = 1ull << logN, t = cfg->num_colinearity_tests;
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, 1ull << cfg->log_blowup);
    size_t end = 0;
    const std::vector<Obj> objs = parse(proof, proof_len, fri_object_count(fc), &end);
    std::vector<uint64_t> top, ab;
    size_t used = 0;
    SMI_TRY(fri_verify_objs(ctx, fc, fresh_seed(), objs, accept, &top, nullptr, nullptr, &ab, &used));
    // ---- the column openings (mgpu_core.h layout): rows, then paths
    *accept = 0;
    const OpeningWords &say = COLUMN_WORDS;
    const size_t rec = 9 + 8 * (size_t)W, prec = 9 + 32 * (size_t)logN, m = 2 * t;
    if (proof_len - end != m * rec + m * W * prec) return reject(ctx, accept, say.length);
    const uint8_t *ext = proof + end;
    // weight c = FiatShamir::challenge after absorbing roots[0..c] (fresh transcript)
    Transcript tr;
    std::vector<uint64_t> weights, rows(m * W);
    transcript_columns(tr, column_roots, W, 0, &weights);
    for (size_t q = 0; q < m; q++) {
        const uint8_t *r = ext + q * rec;
        if (r[0] != 2 || get_u64(r + 1) != W) return reject(ctx, accept, say.row);
        uint64_t acc = 0;
        for (uint32_t c = 0; c < W; c++) {
            const uint64_t v = get_u64(r + 9 + 8 * c);
            rows[q * W + c] = v;
            acc = (acc + mulm(weights[c] % p, v % p, p)) % p;
        }
        if (acc != ab[q] % p) return reject(ctx, accept, say.composition);
    }
    SMI_TRY(auth_column_trees(ctx, accept, say, ext + m * rec, rows, m, 2, W, logN, opened_positions(top, N, 0, 2), column_roots));
    *accept = 1;
    return SMI_OK;
}
int smi_stark_verify(smi_ctx *ctx, const smi_stark_cfg *cfg, const uint8_t *column_roots, const uint8_t *proof, size_t proof_len,
                     int *accept) {
    if (!ctx || !cfg || !column_roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    return settle(stark_verify_impl(ctx, cfg, column_roots, proof, proof_len, accept));
}

// the two auxiliary quotients of the permutation argument (include/stark_mi.h, "Permutation argument") at one point, in
// host F_q arithmetic (ext_mul_host): what smi_dev_air_compose_perm adds to the main part of the composition
struct PermAux {
    uint32_t p, g, width;
    const smi_air_perm *perm;
    uint32_t gamma[4], wb[4], wt[4];
    std::vector<std::vector<uint32_t>> apow;   // alpha^j, j < width
    uint64_t n, tau, tau_n;
    PermAux(const smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air_perm *perm_, const uint64_t ch[8], const uint64_t *w_bound, const uint64_t *w_trans)
        : p(ctx->fs.F.p), g(ctx->fs.g), width(perm_->width), perm(perm_), apow(perm_->width, std::vector<uint32_t>(4, 0)), n(1ull << cfg->log_n),
          tau(cfg->trace_offset), tau_n(powm(cfg->trace_offset, 1ull << cfg->log_n, ctx->fs.F.p)) {
        uint32_t alpha[4], pw[4] = {1, 0, 0, 0};
        perm_challenges(p, ch, alpha, gamma);
        for (int e = 0; e < 4; e++) wb[e] = (uint32_t)(w_bound[e] % p), wt[e] = (uint32_t)(w_trans[e] % p);
        for (uint32_t j = 0; j < width; j++) {
            apow[j].assign(pw, pw + 4);
            ext_mul_host(p, g, pw, alpha, pw);
        }
    }
    // got += w_b (z - 1) / (x - tau) + w_t (z' f_R - z f_L) / (x^n - tau^n) over the row cur and the z coordinates zc, zn
    void add(uint64_t x, const uint64_t *cur, const uint64_t *zc, const uint64_t *zn, uint32_t got[4]) const {
        uint32_t fl[4], fr[4], z0[4], z1[4], a[4], b[4], bq[4], tq[4], u[4], v[4];
        for (int e = 0; e < 4; e++) fl[e] = fr[e] = gamma[e], z0[e] = (uint32_t)zc[e], z1[e] = (uint32_t)zn[e];
        for (uint32_t j = 0; j < width; j++)
            for (int e = 0; e < 4; e++) {
                fl[e] = (uint32_t)((fl[e] + mulm(apow[j][e], cur[perm->left_col[j]], p)) % p);
                fr[e] = (uint32_t)((fr[e] + mulm(apow[j][e], cur[perm->right_col[j]], p)) % p);
            }
        ext_mul_host(p, g, z1, fr, a);
        ext_mul_host(p, g, z0, fl, b);
        const uint64_t izt = powm((powm(x, n, p) + p - tau_n) % p, p - 2, p), ixt = powm((x + p - tau) % p, p - 2, p);
        for (int e = 0; e < 4; e++) {
            tq[e] = (uint32_t)mulm((a[e] + (uint64_t)p - b[e]) % p, izt, p);
            bq[e] = (uint32_t)mulm(e ? z0[e] : (z0[0] + (uint64_t)p - 1) % p, ixt, p);
        }
        ext_mul_host(p, g, bq, wb, u);
        ext_mul_host(p, g, tq, wt, v);
        for (int e = 0; e < 4; e++) got[e] = (uint32_t)(((uint64_t)got[e] + u[e] + v[e]) % p);
    }
};

// the two auxiliary quotients of the lookup argument (include/stark_mi.h, "Lookup argument") at one point, in host F_q
// arithmetic: what smi_dev_air_compose_lookup adds to the main part of the composition
struct LookupAux {
    uint32_t p, g, width;
    const smi_air_lookup *lk;
    uint32_t gamma[4], wb[4], wt[4];
    std::vector<std::vector<uint32_t>> apow;   // alpha^j, j < width
    uint64_t n, tau, tau_n;
    LookupAux(const smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air_lookup *lk_, const uint64_t ch[8], const uint64_t *w_bound, const uint64_t *w_trans)
        : p(ctx->fs.F.p), g(ctx->fs.g), width(lk_->width), lk(lk_), apow(lk_->width, std::vector<uint32_t>(4, 0)), n(1ull << cfg->log_n),
          tau(cfg->trace_offset), tau_n(powm(cfg->trace_offset, 1ull << cfg->log_n, ctx->fs.F.p)) {
        uint32_t alpha[4], pw[4] = {1, 0, 0, 0};
        perm_challenges(p, ch, alpha, gamma);
        for (int e = 0; e < 4; e++) wb[e] = (uint32_t)(w_bound[e] % p), wt[e] = (uint32_t)(w_trans[e] % p);
        for (uint32_t j = 0; j < width; j++) {
            apow[j].assign(pw, pw + 4);
            ext_mul_host(p, g, pw, alpha, pw);
        }
    }
    // got += w_b s / (x - tau) + w_t ((s' - s) f_L f_T - f_T + M f_L) / (x^n - tau^n) over the row cur and the s coordinates sc, sn
    void add(uint64_t x, const uint64_t *cur, const uint64_t *sc, const uint64_t *sn, uint32_t got[4]) const {
        uint32_t fl[4], ft[4], ds[4], lt[4], a[4], bq[4], tq[4], u[4], v[4];
        for (int e = 0; e < 4; e++) fl[e] = ft[e] = gamma[e], ds[e] = (uint32_t)((sn[e] + p - sc[e]) % p);
        for (uint32_t j = 0; j < width; j++)
            for (int e = 0; e < 4; e++) {
                fl[e] = (uint32_t)((fl[e] + mulm(apow[j][e], cur[lk->lookup_col[j]], p)) % p);
                ft[e] = (uint32_t)((ft[e] + mulm(apow[j][e], cur[lk->table_col[j]], p)) % p);
            }
        ext_mul_host(p, g, fl, ft, lt);
        ext_mul_host(p, g, ds, lt, a);
        const uint64_t izt = powm((powm(x, n, p) + p - tau_n) % p, p - 2, p), ixt = powm((x + p - tau) % p, p - 2, p), M = cur[lk->mult_col];
        for (int e = 0; e < 4; e++) {
            tq[e] = (uint32_t)mulm((a[e] + (uint64_t)p - ft[e] + mulm(M, fl[e], p)) % p, izt, p);
            bq[e] = (uint32_t)mulm(sc[e], ixt, p);
        }
        ext_mul_host(p, g, bq, wb, u);
        ext_mul_host(p, g, tq, wt, v);
        for (int e = 0; e < 4; e++) got[e] = (uint32_t)(((uint64_t)got[e] + u[e] + v[e]) % p);
    }
};

// the two auxiliary quotients of one argument of a list with selectors and periodic members (include/stark_mi.h, "Argument
// list with selectors and periodic members") at one point, in host F_q arithmetic: what smi_dev_air_compose_xargs adds for it
struct XArgAux {
    uint32_t p, g, W;
    const smi_air_xarg *arg;
    uint32_t gamma[4], wb[4], wt[4];
    std::vector<std::vector<uint32_t>> apow;   // alpha^j, j < width
    uint64_t n, tau, tau_n;
    XArgAux(const smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air_xarg *arg_, const uint64_t ch[8], const uint64_t *w_bound, const uint64_t *w_trans)
        : p(ctx->fs.F.p), g(ctx->fs.g), W(cfg->n_cols), arg(arg_), apow(arg_->width, std::vector<uint32_t>(4, 0)), n(1ull << cfg->log_n),
          tau(cfg->trace_offset), tau_n(powm(cfg->trace_offset, 1ull << cfg->log_n, ctx->fs.F.p)) {
        uint32_t alpha[4], pw[4] = {1, 0, 0, 0};
        perm_challenges(p, ch, alpha, gamma);
        for (int e = 0; e < 4; e++) wb[e] = (uint32_t)(w_bound[e] % p), wt[e] = (uint32_t)(w_trans[e] % p);
        for (uint32_t j = 0; j < arg->width; j++) {
            apow[j].assign(pw, pw + 4);
            ext_mul_host(p, g, pw, alpha, pw);
        }
    }
    // operand v at the point: the opened row cur, or the periodic values per[0 .. Q) of this row; a next-row operand
    // ("Argument list: next-row operands") reads the opened row B further (nxt) or pi_j(w x), per[Q .. 2 Q)
    struct Rows {
        const uint64_t *cur, *nxt;
        const uint32_t *per;
        uint32_t Q;
    };
    uint64_t val(uint32_t v, const Rows &cur) const {
        if (v == SMI_ARG_NO_SELECTOR) return 1;
        const bool next = (v & SMI_ARG_NEXT_ROW) != 0;
        v &= ~SMI_ARG_NEXT_ROW;
        return v < W ? (next ? cur.nxt : cur.cur)[v] : cur.per[(next ? cur.Q : 0) + v - 2 * W];
    }
    // got += w_b bq + w_t tq over the rows, the periodic values and the column's coordinates cc (this row), cn (next)
    void add(uint64_t x, const Rows &cur, const uint64_t *cc, const uint64_t *cn, uint32_t got[4]) const {
        uint32_t fl[4], fr[4], c0[4], c1[4], a[4], b[4], bq[4], tq[4], u[4], v[4];
        for (int e = 0; e < 4; e++) fl[e] = fr[e] = gamma[e], c0[e] = (uint32_t)cc[e], c1[e] = (uint32_t)cn[e];
        const uint32_t J = xarg_tuples(*arg), m = arg->width;
        if (J > 1) {   // "Shared-table lookups": (s' - s) P f_T - Nn f_T + M S_b P with (Nn, P) folded over the tuples
            uint32_t P[4] = {1 % p, 0, 0, 0}, Nn[4] = {0, 0, 0, 0}, ds[4], lt[4], nf[4], t[4];
            for (uint32_t i = 0; i < m; i++)
                for (int e = 0; e < 4; e++) fr[e] = (uint32_t)((fr[e] + mulm(apow[i][e], val(arg->b_var[i], cur), p)) % p);
            for (uint32_t j = 0; j < J; j++) {
                uint32_t f[4] = {gamma[0], gamma[1], gamma[2], gamma[3]};
                for (uint32_t i = 0; i < m; i++)
                    for (int e = 0; e < 4; e++) f[e] = (uint32_t)((f[e] + mulm(apow[i][e], val(arg->a_var[j * m + i], cur), p)) % p);
                const uint64_t sj = val(arg->a_var[J * m + j], cur);
                ext_mul_host(p, g, Nn, f, t);
                for (int e = 0; e < 4; e++) Nn[e] = (uint32_t)((t[e] + mulm(sj, P[e], p)) % p);
                ext_mul_host(p, g, P, f, t);
                for (int e = 0; e < 4; e++) P[e] = t[e];
            }
            for (int e = 0; e < 4; e++) ds[e] = (uint32_t)((c1[e] + (uint64_t)p - c0[e]) % p);
            ext_mul_host(p, g, P, fr, lt);
            ext_mul_host(p, g, ds, lt, a);
            ext_mul_host(p, g, Nn, fr, nf);
            const uint64_t izt = powm((powm(x, n, p) + p - tau_n) % p, p - 2, p), ixt = powm((x + p - tau) % p, p - 2, p);
            const uint64_t M = mulm(cur.cur[arg->mult_col], val(arg->b_sel, cur), p);
            for (int e = 0; e < 4; e++) {
                tq[e] = (uint32_t)mulm((a[e] + (uint64_t)p - nf[e] + mulm(M, P[e], p)) % p, izt, p);
                bq[e] = (uint32_t)mulm(c0[e], ixt, p);
            }
            ext_mul_host(p, g, bq, wb, u);
            ext_mul_host(p, g, tq, wt, v);
            for (int e = 0; e < 4; e++) got[e] = (uint32_t)(((uint64_t)got[e] + u[e] + v[e]) % p);
            return;
        }
        for (uint32_t j = 0; j < arg->width; j++)
            for (int e = 0; e < 4; e++) {
                fl[e] = (uint32_t)((fl[e] + mulm(apow[j][e], val(arg->a_var[j], cur), p)) % p);
                fr[e] = (uint32_t)((fr[e] + mulm(apow[j][e], val(arg->b_var[j], cur), p)) % p);
            }
        const uint64_t sa = val(arg->a_sel, cur), sb = val(arg->b_sel, cur);
        const uint64_t izt = powm((powm(x, n, p) + p - tau_n) % p, p - 2, p), ixt = powm((x + p - tau) % p, p - 2, p);
        if ((arg->kind & 0xffu) == SMI_ARG_PERM) {   // g = 1 + S (f - 1)
            for (int e = 0; e < 4; e++) {
                fl[e] = (uint32_t)(((e ? 0 : 1) + mulm(sa, (fl[e] + (uint64_t)p - (e ? 0 : 1)) % p, p)) % p);
                fr[e] = (uint32_t)(((e ? 0 : 1) + mulm(sb, (fr[e] + (uint64_t)p - (e ? 0 : 1)) % p, p)) % p);
            }
            ext_mul_host(p, g, c1, fr, a);
            ext_mul_host(p, g, c0, fl, b);
            for (int e = 0; e < 4; e++) {
                tq[e] = (uint32_t)mulm((a[e] + (uint64_t)p - b[e]) % p, izt, p);
                bq[e] = (uint32_t)mulm(e ? c0[e] : (c0[0] + (uint64_t)p - 1) % p, ixt, p);
            }
        } else {   // (s' - s) f_L f_T - S_a f_T + M S_b f_L
            uint32_t ds[4], lt[4];
            for (int e = 0; e < 4; e++) ds[e] = (uint32_t)((c1[e] + (uint64_t)p - c0[e]) % p);
            ext_mul_host(p, g, fl, fr, lt);
            ext_mul_host(p, g, ds, lt, a);
            const uint64_t M = mulm(cur.cur[arg->mult_col], sb, p);
            for (int e = 0; e < 4; e++) {
                tq[e] = (uint32_t)mulm((a[e] + (uint64_t)p - mulm(sa, fr[e], p) + mulm(M, fl[e], p)) % p, izt, p);
                bq[e] = (uint32_t)mulm(c0[e], ixt, p);
            }
        }
        ext_mul_host(p, g, bq, wb, u);
        ext_mul_host(p, g, tq, wt, v);
        for (int e = 0; e < 4; e++) got[e] = (uint32_t)(((uint64_t)got[e] + u[e] + v[e]) % p);
    }
};

// What the AIR verifiers differ in (include/stark_mi.h: "AIR", "AIR over one row-committed tree", "Extension FRI",
// "Grinding", "Permutation argument").
//   by_rows : one tree over the rows (one path per position, leaves from the bytes) instead of W column trees
//   over_ext: weights from the quartic extension -- four challenges per weight --, FRI over F_q, the four coordinates of the
//             composition against the layer-0 triple's a and b
//   grind   : the proof-of-work difficulty demanded of the FRI part, or SMI_GRIND_NONE
//   perm    : the permutation argument: a second root and a second section (the rows of z, four values wide), the two
//             auxiliary quotients added to the composition; the tags of both sections are checked record by record before
//             either is authenticated, and every opened value is checked canonical before the composition
//   lookup  : the lookup argument: the same second root and second section (the rows of s) with its own two quotients and
//             its own sentences
//   args    : the argument list ("Argument list"): the second section's rows are 4 A values wide, argument a at the
//             coordinates 4 a .. 4 a + 3 with the weights W + K + 2 a and W + K + 2 a + 1, PermAux or LookupAux once per
//             argument, its own sentences
//   xargs   : the argument list with selectors and periodic members: the layout, transcript and sentences of args, XArgAux once
//             per argument over the opened row and the periodic operands at the point; at most one of the four is set
struct AirVariant {
    bool by_rows, over_ext;
    int grind;
    const smi_air_perm *perm;
    const smi_air_lookup *lookup;
    const smi_air_args *args = nullptr;
    const smi_air_xargs *xargs = nullptr;
};
// One verifier for them all: the weights and FRI's seed from the variant's transcript, Fri::verify at expansion factor E,
// then the openings -- length, records, every path against its root, and the composition codeword recomputed at x_a and
// x_b with the evaluator the prover's kernel runs (air_core.h) over the opened rows.
static int air_verify_impl(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air, const uint8_t *roots, const uint8_t *proof, size_t proof_len,
                           int *accept, const AirVariant &var) {
    std::string why;
    uint64_t E = 0;
    const bool has_aux = var.perm || var.lookup || var.args || var.xargs;   // auxiliary columns: a second root, a second section, two more quotients each
    const int vrc = var.perm     ? perm_plan(ctx->fs.F.p, cfg, air, var.perm, nullptr, &E, &why)
                    : var.lookup ? lookup_plan(ctx->fs.F.p, cfg, air, var.lookup, nullptr, &E, &why)
                    : var.args   ? args_plan(ctx->fs.F.p, cfg, air, var.args, nullptr, &E, &why)
                    : var.xargs  ? xargs_plan(ctx->fs.F.p, cfg, air, var.xargs, nullptr, &E, &why)
                                 : air_validate(ctx->fs.F.p, cfg, air, nullptr, &E, &why);
    if (vrc != SMI_OK) return smi_fail(ctx, vrc, why.c_str());
    const uint32_t W = cfg->n_cols, K = air->n_constraints, logN = cfg->log_n + cfg->log_blowup;
    SMI_TRY(domain_check(ctx, logN));
    const uint64_t p = ctx->fs.F.p, N = 1ull << logN, B = 1ull << cfg->log_blowup, t = cfg->num_colinearity_tests;
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, E);
    Transcript tr;
    std::vector<uint64_t> ch, weights;   // ch: alpha and gamma of the auxiliary column
    if (has_aux) {
        transcript_perm_challenges(tr, roots, &ch);
        if (var.args || var.xargs) transcript_args_weights(tr, roots + 32, W, K, var.args ? var.args->count : var.xargs->count, &weights);
        else transcript_perm_weights(tr, roots + 32, W, K, &weights);
    } else if (var.over_ext) {
        transcript_ext(tr, roots, W, K, &weights);
    } else if (var.by_rows) {
        transcript_rows(tr, roots, W, K, &weights);
    } else {
        transcript_columns(tr, roots, W, K, &weights);
    }
    size_t end = 0;
    const std::vector<Obj> objs = parse(proof, proof_len, fri_object_count(fc) + (var.grind != SMI_GRIND_NONE ? 1 : 0), &end);
    std::vector<uint64_t> top, ab;
    size_t used = 0;
    if (var.over_ext) SMI_TRY(fri_verify_ext_objs(ctx, fc, tr.seed(), objs, accept, &top, nullptr, nullptr, &ab, &used, var.grind));
    else SMI_TRY(fri_verify_objs(ctx, fc, tr.seed(), objs, accept, &top, nullptr, nullptr, &ab, &used));
    *accept = 0;
    // ---- the opening sections: rows of W values under root_1 (or the column roots); with an auxiliary column, rows of 4
    // values under root_2
    const OpeningWords &say = var.perm ? PERM_WORDS : var.lookup ? LOOKUP_WORDS : (var.args || var.xargs) ? ARGS_WORDS : AIR_WORDS;
    const size_t R = (K || has_aux) ? 4 : 2, m = R * t, prec = 9 + 32 * (size_t)logN, n_sec = has_aux ? 2 : 1;
    const uint32_t AW = var.args ? 4 * var.args->count : var.xargs ? 4 * var.xargs->count : 4;   // values in a row of the second section
    const uint32_t widths[2] = {W, AW}, NE = var.over_ext ? 4 : 1;
    const size_t sec_len[2] = {m * (9 + 8 * (size_t)W) + (var.by_rows ? 1 : W) * m * prec, has_aux ? m * (9 + 8 * (size_t)AW) + m * prec : 0};
    if (proof_len - end != sec_len[0] + sec_len[1]) return reject(ctx, accept, say.length);
    const uint8_t *sec[2] = {proof + end, proof + end + sec_len[0]};
    const std::vector<uint64_t> pos = opened_positions(top, N, B, R);
    std::vector<uint64_t> rows[2];
    const RecordOrder order = has_aux ? RECORD_BY_RECORD : var.by_rows ? ROWS_THEN_PATHS : ROWS_ONLY;
    for (size_t v = 0; v < n_sec; v++) SMI_TRY(parse_section(ctx, accept, say, sec[v], m, widths[v], logN, order, &rows[v]));
    for (size_t v = 0; v < n_sec; v++) {
        if (var.by_rows) SMI_TRY(auth_section(ctx, accept, say, sec[v], m, widths[v], logN, pos, roots + 32 * v));
        else SMI_TRY(auth_column_trees(ctx, accept, say, sec[v] + m * (9 + 8 * (size_t)W), rows[v], m, R, W, logN, pos, roots));
    }
    if (has_aux)
        for (size_t v = 0; v < n_sec; v++)
            for (uint64_t x : rows[v])
                if (x >= p) return reject(ctx, accept, say.canonical);
    // ---- the composition codeword at x_a and x_b from the opened rows
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
    // the W + K weights of the main part in Montgomery form; over_ext: coordinate e of weight j at e * AIR_MAX_WEIGHTS + j
    std::vector<uint32_t> w_m(var.over_ext ? 4 * AIR_MAX_WEIGHTS : W + K, 0);
    for (uint32_t i = 0; i < NE * (W + K); i++) w_m[var.over_ext ? (i & 3) * AIR_MAX_WEIGHTS + (i >> 2) : i] = to_mont_u64(weights[i], F);
    std::optional<PermAux> aux;
    std::optional<LookupAux> laux;
    if (var.perm) aux.emplace(ctx, cfg, var.perm, ch.data(), &weights[4 * (W + K)], &weights[4 * (W + K + 1)]);
    if (var.lookup) laux.emplace(ctx, cfg, var.lookup, ch.data(), &weights[4 * (W + K)], &weights[4 * (W + K + 1)]);
    // the argument list: argument a as a PermAux or a LookupAux over its own statement (kept here: the Aux hold pointers)
    const uint32_t NA = var.args ? var.args->count : 0;
    std::vector<smi_air_perm> a_perm(NA);
    std::vector<smi_air_lookup> a_lookup(NA);
    std::vector<std::optional<PermAux>> a_paux(NA);
    std::vector<std::optional<LookupAux>> a_laux(NA);
    for (uint32_t a = 0; a < NA; a++) {
        const uint64_t *wb = &weights[4 * (W + K + 2 * a)], *wt = &weights[4 * (W + K + 2 * a + 1)];
        if (var.args->arg[a].kind == SMI_ARG_PERM) {
            a_perm[a] = args_as_perm(var.args->arg[a]);
            a_paux[a].emplace(ctx, cfg, &a_perm[a], ch.data(), wb, wt);
        } else {
            a_lookup[a] = args_as_lookup(var.args->arg[a]);
            a_laux[a].emplace(ctx, cfg, &a_lookup[a], ch.data(), wb, wt);
        }
    }
    std::vector<XArgAux> x_aux;
    for (uint32_t a = 0; var.xargs && a < var.xargs->count; a++)
        x_aux.emplace_back(ctx, cfg, &var.xargs->arg[a], ch.data(), &weights[4 * (W + K + 2 * a)], &weights[4 * (W + K + 2 * a + 1)]);
    for (uint64_t s = 0; s < t; s++)
        for (size_t k = 0; k < 2; k++) {
            const uint64_t i = pos[R * s + k];
            for (size_t r = k; r < R && !has_aux; r += 2)   // this side's rows, in front of this side's composition
                for (uint32_t c = 0; c < W; c++)
                    if (rows[0][(R * s + r) * W + c] >= p) return reject(ctx, accept, say.canonical);
            const uint64_t *cur = &rows[0][(R * s + k) * W], *nxt = R == 4 ? &rows[0][(R * s + k + 2) * W] : nullptr;
            const uint64_t x = mulm(cfg->lde_offset, powm(fc.omega, i, p), p);
            const uint32_t x_m = air_to_m((uint32_t)x, (uint32_t)p), ib = (uint32_t)(i & (B - 1));
            auto operand = [&](int, uint32_t v) {   // AirDev::fac's numbering: W + Q operands at this row, then at the next
                const bool next = v >= W + Q;
                const uint32_t c = next ? v - (W + Q) : v;
                if (c >= W) return per[(2 * s + k) * 2 * Q + (next ? Q : 0) + (c - W)];
                return (uint32_t)(next ? nxt[c] : cur[c]);
            };
            uint32_t got[4] = {0, 0, 0, 0};
            if (var.over_ext) air_compose_points_ext<1>(H.dev, F, w_m.data(), &x_m, &ib, operand, got);
            else air_compose_points<1>(H.dev, F, w_m.data(), &x_m, &ib, operand, got);
            if (var.perm) aux->add(x, cur, &rows[1][(R * s + k) * 4], &rows[1][(R * s + k + 2) * 4], got);
            if (var.lookup) laux->add(x, cur, &rows[1][(R * s + k) * 4], &rows[1][(R * s + k + 2) * 4], got);
            for (uint32_t a = 0; a < NA; a++) {
                const uint64_t *cc = &rows[1][(R * s + k) * AW + 4 * a], *cn = &rows[1][(R * s + k + 2) * AW + 4 * a];
                if (a_paux[a]) a_paux[a]->add(x, cur, cc, cn, got);
                else a_laux[a]->add(x, cur, cc, cn, got);
            }
            for (size_t a = 0; a < x_aux.size(); a++)
                x_aux[a].add(x, XArgAux::Rows{cur, nxt, Q ? &per[(2 * s + k) * 2 * Q] : nullptr, Q}, &rows[1][(R * s + k) * AW + 4 * a], &rows[1][(R * s + k + 2) * AW + 4 * a], got);
            for (uint32_t e = 0; e < NE; e++)
                if (got[e] != ab[(2 * s + k) * NE + e] % p) return reject(ctx, accept, say.composition);
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
    return settle(air_verify_impl(ctx, cfg, (const smi_air *)air, column_roots, proof, proof_len, accept, AirVariant{false, false, SMI_GRIND_NONE, nullptr, nullptr}));
}

int smi_air_verify_rows(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t row_root[32], const uint8_t *proof,
                        size_t proof_len, int *accept) {
    if (!ctx || !cfg || !air || !row_root || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    return settle(air_verify_impl(ctx, cfg, (const smi_air *)air, row_root, proof, proof_len, accept, AirVariant{true, false, SMI_GRIND_NONE, nullptr, nullptr}));
}

int smi_air_verify_ext(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t row_root[32], const uint8_t *proof,
                       size_t proof_len, int *accept) {
    if (!ctx || !cfg || !air || !row_root || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(ext_field_check(ctx));
    return settle(air_verify_impl(ctx, cfg, (const smi_air *)air, row_root, proof, proof_len, accept, AirVariant{true, true, SMI_GRIND_NONE, nullptr, nullptr}));
}

int smi_air_verify_ext_pow(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t row_root[32], const uint8_t *proof,
                           size_t proof_len, int *accept, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !row_root || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    return settle(air_verify_impl(ctx, cfg, (const smi_air *)air, row_root, proof, proof_len, accept, AirVariant{true, true, (int)grind_bits, nullptr, nullptr}));
}

// Verifier of smi_dev_air_prove_ext_fold4 (include/stark_mi.h, "Extension FRI, folding factor 4"): air_verify_impl's row /
// extension / proof-of-work variant with four points per test instead of two.  The transcript, the section checks
// (parse_section, auth_section, AIR_WORDS), the periodic operands and the evaluator are the ones air_verify_impl uses; what
// differs is the FRI walk, the opened positions (the layer-0 coset) and the record the composition is compared with.
static int air_verify_fold4_impl(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air, const uint8_t *root, const uint8_t *proof, size_t proof_len,
                                 int *accept, uint32_t grind) {
    std::string why;
    uint64_t E = 0;
    const int vrc = air_validate(ctx->fs.F.p, cfg, air, nullptr, &E, &why);
    if (vrc != SMI_OK) return smi_fail(ctx, vrc, why.c_str());
    const uint32_t W = cfg->n_cols, K = air->n_constraints, logN = cfg->log_n + cfg->log_blowup;
    SMI_TRY(domain_check(ctx, logN));
    const uint64_t p = ctx->fs.F.p, N = 1ull << logN, B = 1ull << cfg->log_blowup, t = cfg->num_colinearity_tests;
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, E);
    {
        const FriFold4Layout lay = fri_layout_fold4(fc);
        if (lay.R2 && lay.F == 0) return smi_fail(ctx, SMI_ERR_BAD_ARG, AIR_FOLD4_NO_LAYER);
    }
    Transcript tr;
    std::vector<uint64_t> weights;
    transcript_ext(tr, root, W, K, &weights);
    size_t end = 0;
    const std::vector<Obj> objs = parse(proof, proof_len, fri_object_count_fold4(fc), &end);
    std::vector<uint64_t> top, coset;   // coset: the 16 values of every layer-0 record
    size_t used = 0;
    SMI_TRY(fri_walk_fold4(ctx, fc, tr.seed(), objs, accept, &top, nullptr, nullptr, &coset, &used, grind));
    *accept = 0;
    const OpeningWords &say = AIR_WORDS;
    const size_t R = K ? 8 : 4, m = R * t, prec = 9 + 32 * (size_t)logN;
    if (proof_len - end != m * (9 + 8 * (size_t)W) + m * prec) return reject(ctx, accept, say.length);
    const uint8_t *sec = proof + end;
    std::vector<uint64_t> pos(m);
    for (uint64_t s = 0; s < t; s++)
        for (size_t k = 0; k < R; k++) pos[R * s + k] = (top[s] % (N / 4) + (k & 3) * (N / 4) + (k & 4 ? B : 0)) & (N - 1);
    std::vector<uint64_t> rows;
    SMI_TRY(parse_section(ctx, accept, say, sec, m, W, logN, ROWS_THEN_PATHS, &rows));
    SMI_TRY(auth_section(ctx, accept, say, sec, m, W, logN, pos, root));
    AirHost H;
    air_build(ctx->fs.F, (uint32_t)fc.omega, cfg, air, &H);
    const Fp F = ctx->fs.F;
    const uint32_t Q = air->n_periodic;
    std::vector<uint32_t> per;   // per[(4 s + k) * 2Q + ..]: Q at this row, Q at the next
    if (Q) {
        std::vector<uint64_t> at(4 * t);
        for (uint64_t s = 0; s < t; s++)
            for (size_t k = 0; k < 4; k++) at[4 * s + k] = pos[R * s + k];
        SMI_TRY(air_periodic_at(ctx, cfg, H, at, &per));
    }
    std::vector<uint32_t> w_m(4 * AIR_MAX_WEIGHTS, 0);
    for (uint32_t i = 0; i < 4 * (W + K); i++) w_m[(i & 3) * AIR_MAX_WEIGHTS + (i >> 2)] = to_mont_u64(weights[i], F);
    for (uint64_t s = 0; s < t; s++)
        for (size_t k = 0; k < 4; k++) {
            const uint64_t i = pos[R * s + k];
            for (size_t r = k; r < R; r += 4)   // this point's rows, in front of this point's composition
                for (uint32_t c = 0; c < W; c++)
                    if (rows[(R * s + r) * W + c] >= p) return reject(ctx, accept, say.canonical);
            const uint64_t *cur = &rows[(R * s + k) * W], *nxt = R == 8 ? &rows[(R * s + k + 4) * W] : nullptr;
            const uint64_t x = mulm(cfg->lde_offset, powm(fc.omega, i, p), p);
            const uint32_t x_m = air_to_m((uint32_t)x, (uint32_t)p), ib = (uint32_t)(i & (B - 1));
            auto operand = [&](int, uint32_t v) {
                const bool next = v >= W + Q;
                const uint32_t c = next ? v - (W + Q) : v;
                if (c >= W) return per[(4 * s + k) * 2 * Q + (next ? Q : 0) + (c - W)];
                return (uint32_t)(next ? nxt[c] : cur[c]);
            };
            uint32_t got[4] = {0, 0, 0, 0};
            air_compose_points_ext<1>(H.dev, F, w_m.data(), &x_m, &ib, operand, got);
            for (uint32_t e = 0; e < 4; e++)
                if (got[e] != coset[16 * s + 4 * e + k]) return reject(ctx, accept, say.composition);
        }
    *accept = 1;
    return SMI_OK;
}
int smi_air_verify_ext_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t row_root[32], const uint8_t *proof,
                             size_t proof_len, int *accept, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !row_root || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    return settle(air_verify_fold4_impl(ctx, cfg, (const smi_air *)air, row_root, proof, proof_len, accept, grind_bits));
}

// Verifier of smi_dev_air_prove_perm (include/stark_mi.h, "Permutation argument"): the extension verifier with proof of
// work, a second root and a second section, and the two auxiliary quotients added to the composition (AirVariant::perm).
int smi_air_verify_perm(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *perm, const uint8_t *roots, const uint8_t *proof,
                        size_t proof_len, int *accept, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !perm || !roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    return settle(air_verify_impl(ctx, cfg, (const smi_air *)air, roots, proof, proof_len, accept,
                                  AirVariant{true, true, (int)grind_bits, (const smi_air_perm *)perm, nullptr}));
}

// Verifier of smi_dev_air_prove_lookup (include/stark_mi.h, "Lookup argument"): smi_air_verify_perm's checks with the lookup
// argument's two auxiliary quotients (AirVariant::lookup).
int smi_air_verify_lookup(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *lookup, const uint8_t *roots, const uint8_t *proof,
                          size_t proof_len, int *accept, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !lookup || !roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    return settle(air_verify_impl(ctx, cfg, (const smi_air *)air, roots, proof, proof_len, accept,
                                  AirVariant{true, true, (int)grind_bits, nullptr, (const smi_air_lookup *)lookup}));
}

// Verifier of smi_dev_air_prove_args (include/stark_mi.h, "Argument list"): smi_air_verify_perm's checks over a second section
// of 4 A values a row, with every argument's two auxiliary quotients (AirVariant::args).
int smi_air_verify_args(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *args, const uint8_t *roots, const uint8_t *proof,
                        size_t proof_len, int *accept, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !args || !roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    return settle(air_verify_impl(ctx, cfg, (const smi_air *)air, roots, proof, proof_len, accept,
                                  AirVariant{true, true, (int)grind_bits, nullptr, nullptr, (const smi_air_args *)args}));
}

// Verifier of smi_dev_air_prove_xargs (include/stark_mi.h, "Argument list with selectors and periodic members"):
// smi_air_verify_args's checks with the quotients of that section (AirVariant::xargs).
int smi_air_verify_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint8_t *roots, const uint8_t *proof,
                         size_t proof_len, int *accept, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !xargs || !roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    return settle(air_verify_impl(ctx, cfg, (const smi_air *)air, roots, proof, proof_len, accept,
                                  AirVariant{true, true, (int)grind_bits, nullptr, nullptr, nullptr, (const smi_air_xargs *)xargs}));
}

// Verifier of smi_dev_air_prove_deep (include/stark_mi.h, "Out-of-domain sampling").  In this order: the out-of-domain
// record (count, canonical coordinates); the transcript -- root_1 and the weights, root_2 and z, the record and the gammas;
// the consistency of the record with the constraints at z (deep_core.h deep_ood_sides, host F_q arithmetic); Fri::verify
// over F_q at E = B with the proof of work; the two opening sections with air_verify_impl's parsing and authentication
// (parse_section, auth_section), two rows per test and no next row; the canonical check; Q recomputed at x_a and x_b from
// the opened rows (deep_q_at) against the layer-0 triple.
const OpeningWords DEEP_WORDS = {DEEP_SENTENCES[0], DEEP_SENTENCES[1], DEEP_SENTENCES[2], DEEP_SENTENCES[3], DEEP_SENTENCES[4], DEEP_SENTENCES[5]};   // deep_core.h
static int air_verify_deep_impl(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air, const uint8_t *roots, const uint8_t *proof, size_t proof_len,
                                int *accept, uint32_t grind) {
    std::string why;
    uint32_t D = 0;
    const int vrc = deep_plan(ctx->fs.F.p, cfg, air, nullptr, &D, &why, SMI_AIR_MAX_WINDOW);
    if (vrc != SMI_OK) return smi_fail(ctx, vrc, why.c_str());
    const uint32_t W = cfg->n_cols, K = air->n_constraints, logN = cfg->log_n + cfg->log_blowup, S = air_window(air);
    SMI_TRY(domain_check(ctx, logN));
    const uint32_t p = ctx->fs.F.p, g = ctx->fs.g, w_n = h_root(ctx, cfg->log_n);
    const uint64_t N = 1ull << logN, t = cfg->num_colinearity_tests;
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, 1ull << cfg->log_blowup);
    const size_t n_ood = 4 * ((size_t)S * W + D);
    size_t end = 0;
    std::vector<Obj> objs = parse(proof, proof_len, 1 + fri_object_count(fc) + 1, &end);
    if (objs.empty() || objs[0].tag != 2 || objs[0].count != n_ood) return reject(ctx, accept, DEEP_BAD_RECORD);
    std::vector<uint64_t> ood(n_ood);
    for (size_t i = 0; i < n_ood; i++)
        if ((ood[i] = get_u64(objs[0].p + 8 * i)) >= p) return reject(ctx, accept, DEEP_RECORD_CANONICAL);
    Transcript tr;
    std::vector<uint64_t> weights, gammas;
    uint64_t zr[4];
    deep_transcript_weights(tr, roots, W, K, &weights);
    deep_transcript_z(tr, roots + 32, W, K, zr);
    const FqH z = fqh_of(zr, p);
    if (fqh_in_base(z)) return reject(ctx, accept, DEEP_Z_IN_BASE_FIELD);
    deep_transcript_gammas(tr, ood.data(), W, K, D, &gammas, S);
    FqH lhs, rhs;
    deep_ood_sides(p, g, cfg, air, D, w_n, weights.data(), z, ood.data(), &lhs, &rhs);
    if (!fqh_eq(lhs, rhs)) return reject(ctx, accept, DEEP_INCONSISTENT);
    objs.erase(objs.begin());
    std::vector<uint64_t> top, ab;
    size_t used = 0;
    SMI_TRY(fri_verify_ext_objs(ctx, fc, tr.seed(), objs, accept, &top, nullptr, nullptr, &ab, &used, (int)grind));
    *accept = 0;
    if (ab.size() != 8 * t) return reject(ctx, accept, DEEP_NO_LAYER);
    const OpeningWords &say = DEEP_WORDS;
    const size_t R = 2, m = R * t, prec = 9 + 32 * (size_t)logN;
    const uint32_t widths[2] = {W, 4 * D};
    const size_t sec_len[2] = {m * (9 + 8 * (size_t)widths[0]) + m * prec, m * (9 + 8 * (size_t)widths[1]) + m * prec};
    if (proof_len - end != sec_len[0] + sec_len[1]) return reject(ctx, accept, say.length);
    const uint8_t *sec[2] = {proof + end, proof + end + sec_len[0]};
    const std::vector<uint64_t> pos = opened_positions(top, N, 0, R);
    std::vector<uint64_t> rows[2];
    for (size_t v = 0; v < 2; v++) SMI_TRY(parse_section(ctx, accept, say, sec[v], m, widths[v], logN, ROWS_THEN_PATHS, &rows[v]));
    for (size_t v = 0; v < 2; v++) SMI_TRY(auth_section(ctx, accept, say, sec[v], m, widths[v], logN, pos, roots + 32 * v));
    for (size_t v = 0; v < 2; v++)
        for (uint64_t x : rows[v])
            if (x >= p) return reject(ctx, accept, say.canonical);
    for (uint64_t s = 0; s < t; s++)
        for (size_t k = 0; k < 2; k++) {
            const uint32_t x = (uint32_t)mulm(cfg->lde_offset, powm(fc.omega, pos[R * s + k], p), p);
            const FqH q = deep_q_at(p, g, W, D, w_n, x, z, ood.data(), gammas.data(), &rows[0][(R * s + k) * W], &rows[1][(R * s + k) * 4 * D], S);
            for (uint32_t e = 0; e < 4; e++)
                if (q.c[e] != ab[(2 * s + k) * 4 + e]) return reject(ctx, accept, say.composition);
        }
    *accept = 1;
    return SMI_OK;
}
int smi_air_verify_deep(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t *roots, const uint8_t *proof, size_t proof_len, int *accept,
                        uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    if (ctx->fs.F.p >= (1u << 30)) return smi_fail(ctx, SMI_ERR_UNSUPPORTED_PRIME, "deep: modulus must be < 2^30");   // the prover's bound (deep.hip)
    return settle(air_verify_deep_impl(ctx, cfg, (const smi_air *)air, roots, proof, proof_len, accept, grind_bits));
}

// Verifier of smi_dev_air_prove_deep_xargs (include/stark_mi.h, "Out-of-domain sampling with an argument list"):
// air_verify_deep_impl's checks in its order with the record of 4 (2 W + 2 A + D) values, the transcript of that section
// (alpha and gamma, the weights of the list, z, the gammas), the consistency check with the 2 A auxiliary quotients at z
// (xargs_core.h deep_xargs_ood_sides), three opening sections, and Q from three rows (deep_args_q_at).
const OpeningWords DEEP_ARGS_WORDS = {DEEP_ARGS_SENTENCES[0], DEEP_ARGS_SENTENCES[1], DEEP_ARGS_SENTENCES[2],
                                      DEEP_ARGS_SENTENCES[3], DEEP_ARGS_SENTENCES[4], DEEP_ARGS_SENTENCES[5]};   // deep_core.h
static int air_verify_deep_xargs_impl(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_xargs *xargs, const uint8_t *roots,
                                      const uint8_t *proof, size_t proof_len, int *accept, uint32_t grind) {
    std::string why;
    uint32_t D = 0;
    const int vrc = deep_xargs_plan(ctx->fs.F.p, cfg, air, xargs, nullptr, &D, &why);
    if (vrc != SMI_OK) return smi_fail(ctx, vrc, why.c_str());
    const int prc = xargs_periodic_check(ctx->fs.F.p, air, cfg->log_n, &why);
    if (prc != SMI_OK) return smi_fail(ctx, prc, why.c_str());
    const uint32_t W = cfg->n_cols, K = air->n_constraints, A = xargs->count, logN = cfg->log_n + cfg->log_blowup;
    const uint64_t NW = (uint64_t)W + K + 2 * (uint64_t)A;
    SMI_TRY(domain_check(ctx, logN));
    const uint32_t p = ctx->fs.F.p, g = ctx->fs.g, w_n = h_root(ctx, cfg->log_n);
    const uint64_t N = 1ull << logN, t = cfg->num_colinearity_tests;
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, 1ull << cfg->log_blowup);
    const size_t n_ood = deep_args_record(W, A, D);
    size_t end = 0;
    std::vector<Obj> objs = parse(proof, proof_len, 1 + fri_object_count(fc) + 1, &end);
    if (objs.empty() || objs[0].tag != 2 || objs[0].count != n_ood) return reject(ctx, accept, DEEP_BAD_RECORD);
    std::vector<uint64_t> ood(n_ood);
    for (size_t i = 0; i < n_ood; i++)
        if ((ood[i] = get_u64(objs[0].p + 8 * i)) >= p) return reject(ctx, accept, DEEP_RECORD_CANONICAL);
    Transcript tr;
    std::vector<uint64_t> ch, weights, gammas;
    uint64_t zr[4];
    transcript_perm_challenges(tr, roots, &ch);
    transcript_args_weights(tr, roots + 32, W, K, A, &weights);
    deep_args_transcript_z(tr, roots + 64, NW, zr);
    const FqH z = fqh_of(zr, p);
    if (fqh_in_base(z)) return reject(ctx, accept, DEEP_Z_IN_BASE_FIELD);
    deep_args_transcript_gammas(tr, ood.data(), NW, n_ood, &gammas);
    FqH lhs, rhs;
    deep_xargs_ood_sides(p, g, cfg, air, xargs, D, w_n, ch.data(), weights.data(), z, ood.data(), &lhs, &rhs);
    if (!fqh_eq(lhs, rhs)) return reject(ctx, accept, DEEP_ARGS_INCONSISTENT);
    objs.erase(objs.begin());
    std::vector<uint64_t> top, ab;
    size_t used = 0;
    SMI_TRY(fri_verify_ext_objs(ctx, fc, tr.seed(), objs, accept, &top, nullptr, nullptr, &ab, &used, (int)grind));
    *accept = 0;
    if (ab.size() != 8 * t) return reject(ctx, accept, DEEP_NO_LAYER);
    const OpeningWords &say = DEEP_ARGS_WORDS;
    const size_t R = 2, m = R * t, prec = 9 + 32 * (size_t)logN;
    const uint32_t widths[3] = {W, 4 * A, 4 * D};
    size_t sec_len[3], total = 0;
    const uint8_t *sec[3];
    for (size_t v = 0; v < 3; v++) {
        sec[v] = proof + end + total;
        sec_len[v] = m * (9 + 8 * (size_t)widths[v]) + m * prec;
        total += sec_len[v];
    }
    if (proof_len - end != total) return reject(ctx, accept, say.length);
    const std::vector<uint64_t> pos = opened_positions(top, N, 0, R);
    std::vector<uint64_t> rows[3];
    for (size_t v = 0; v < 3; v++) SMI_TRY(parse_section(ctx, accept, say, sec[v], m, widths[v], logN, ROWS_THEN_PATHS, &rows[v]));
    for (size_t v = 0; v < 3; v++) SMI_TRY(auth_section(ctx, accept, say, sec[v], m, widths[v], logN, pos, roots + 32 * v));
    for (size_t v = 0; v < 3; v++)
        for (uint64_t x : rows[v])
            if (x >= p) return reject(ctx, accept, say.canonical);
    for (uint64_t s = 0; s < t; s++)
        for (size_t k = 0; k < 2; k++) {
            const size_t r = R * s + k;
            const uint32_t x = (uint32_t)mulm(cfg->lde_offset, powm(fc.omega, pos[r], p), p);
            const FqH q = deep_args_q_at(p, g, W, A, D, w_n, x, z, ood.data(), gammas.data(), &rows[0][r * W], &rows[1][r * 4 * A], &rows[2][r * 4 * D]);
            for (uint32_t e = 0; e < 4; e++)
                if (q.c[e] != ab[(2 * s + k) * 4 + e]) return reject(ctx, accept, say.composition);
        }
    *accept = 1;
    return SMI_OK;
}
int smi_air_verify_deep_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint8_t *roots, const uint8_t *proof,
                              size_t proof_len, int *accept, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !xargs || !roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    if (ctx->fs.F.p >= (1u << 30)) return smi_fail(ctx, SMI_ERR_UNSUPPORTED_PRIME, "deep: modulus must be < 2^30");   // the prover's bound (deep.hip)
    return settle(air_verify_deep_xargs_impl(ctx, cfg, (const smi_air *)air, (const smi_air_xargs *)xargs, roots, proof, proof_len, accept, grind_bits));
}

// Verifiers of smi_dev_air_prove_deep_fold4 and smi_dev_air_prove_deep_xargs_fold4 (include/stark_mi.h, "Out-of-domain
// sampling over coset leaves"), one function over the list (xargs == nullptr: a plain AIR).  The checks of
// air_verify_deep_impl / air_verify_deep_xargs_impl in their order with their sentences up to and including the consistency
// check at z; the refusal of a shape without a fold; the fold-by-4 FRI walk with the proof of work, which hands out the
// layer-0 coset records; then the opening sections group by group (deep_core.h deep_coset_parse: the exact length, every
// record's and every path's tag and count), every record hashed as it stands to its leaf and authenticated at a = top mod
// N / 4 (auth_section over a tree of N / 4 leaves), the canonical check, and Q at the coset's four points against the
// layer-0 record (deep_coset_q_matches).
const OpeningWords DEEP_FOLD4_WORDS = {DEEP_FOLD4_SENTENCES[0], DEEP_FOLD4_SENTENCES[1], DEEP_FOLD4_SENTENCES[2],
                                       DEEP_FOLD4_SENTENCES[3], DEEP_FOLD4_SENTENCES[4], DEEP_FOLD4_SENTENCES[5]};   // deep_core.h
const OpeningWords DEEP_ARGS_FOLD4_WORDS = {DEEP_ARGS_FOLD4_SENTENCES[0], DEEP_ARGS_FOLD4_SENTENCES[1], DEEP_ARGS_FOLD4_SENTENCES[2],
                                            DEEP_ARGS_FOLD4_SENTENCES[3], DEEP_ARGS_FOLD4_SENTENCES[4], DEEP_ARGS_FOLD4_SENTENCES[5]};
static int air_verify_deep_fold4_impl(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_xargs *xargs, const uint8_t *roots,
                                      const uint8_t *proof, size_t proof_len, int *accept, uint32_t grind) {
    std::string why;
    uint32_t D = 0;
    const int vrc = xargs ? deep_xargs_plan(ctx->fs.F.p, cfg, air, xargs, nullptr, &D, &why)
                          : deep_plan(ctx->fs.F.p, cfg, air, nullptr, &D, &why, SMI_AIR_MAX_WINDOW);
    if (vrc != SMI_OK) return smi_fail(ctx, vrc, why.c_str());
    if (xargs) {
        const int prc = xargs_periodic_check(ctx->fs.F.p, air, cfg->log_n, &why);
        if (prc != SMI_OK) return smi_fail(ctx, prc, why.c_str());
    }
    const uint32_t W = cfg->n_cols, K = air->n_constraints, A = xargs ? xargs->count : 0, logN = cfg->log_n + cfg->log_blowup;
    const uint32_t S = xargs ? 2 : air_window(air);   // a list is refused above when its AIR has a wider window
    const uint64_t NW = (uint64_t)W + K + 2 * (uint64_t)A;
    SMI_TRY(domain_check(ctx, logN));
    const uint32_t p = ctx->fs.F.p, g = ctx->fs.g, w_n = h_root(ctx, cfg->log_n);
    const uint64_t N = 1ull << logN, t = cfg->num_colinearity_tests;
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, 1ull << cfg->log_blowup);
    const size_t n_ood = deep_args_record(W, A, D) + 4 * (size_t)(S - 2) * W;
    size_t end = 0;
    std::vector<Obj> objs = parse(proof, proof_len, 1 + fri_object_count_fold4(fc), &end);
    if (objs.empty() || objs[0].tag != 2 || objs[0].count != n_ood) return reject(ctx, accept, DEEP_BAD_RECORD);
    std::vector<uint64_t> ood(n_ood);
    for (size_t i = 0; i < n_ood; i++)
        if ((ood[i] = get_u64(objs[0].p + 8 * i)) >= p) return reject(ctx, accept, DEEP_RECORD_CANONICAL);
    Transcript tr;
    std::vector<uint64_t> ch, weights, gammas;
    uint64_t zr[4];
    if (xargs) {
        transcript_perm_challenges(tr, roots, &ch);
        transcript_args_weights(tr, roots + 32, W, K, A, &weights);
        deep_args_transcript_z(tr, roots + 64, NW, zr);
    } else {
        deep_transcript_weights(tr, roots, W, K, &weights);
        deep_transcript_z(tr, roots + 32, W, K, zr);
    }
    const FqH z = fqh_of(zr, p);
    if (fqh_in_base(z)) return reject(ctx, accept, DEEP_Z_IN_BASE_FIELD);
    FqH lhs, rhs;
    if (xargs) {
        deep_args_transcript_gammas(tr, ood.data(), NW, n_ood, &gammas);
        deep_xargs_ood_sides(p, g, cfg, air, xargs, D, w_n, ch.data(), weights.data(), z, ood.data(), &lhs, &rhs);
        if (!fqh_eq(lhs, rhs)) return reject(ctx, accept, DEEP_ARGS_INCONSISTENT);
    } else {
        deep_transcript_gammas(tr, ood.data(), W, K, D, &gammas, S);
        deep_ood_sides(p, g, cfg, air, D, w_n, weights.data(), z, ood.data(), &lhs, &rhs);
        if (!fqh_eq(lhs, rhs)) return reject(ctx, accept, DEEP_INCONSISTENT);
    }
    if (fri_layout_fold4(fc).F == 0) return reject(ctx, accept, DEEP_FOLD4_NO_LAYER);
    objs.erase(objs.begin());
    std::vector<uint64_t> top, coset;   // coset: the 16 values of every layer-0 record
    size_t used = 0;
    SMI_TRY(fri_walk_fold4(ctx, fc, tr.seed(), objs, accept, &top, nullptr, nullptr, &coset, &used, grind));
    *accept = 0;
    const OpeningWords &say = xargs ? DEEP_ARGS_FOLD4_WORDS : DEEP_FOLD4_WORDS;
    const DeepGroups gr = deep_groups(W, A, D);
    const uint8_t *sec = proof + end;
    std::vector<uint64_t> vals[3];
    size_t at[3] = {0, 0, 0};
    switch (deep_coset_parse(sec, proof_len - end, gr, t, logN, vals, at)) {
        case DEEP_COSET_LENGTH: return reject(ctx, accept, say.length);
        case DEEP_COSET_RECORD: return reject(ctx, accept, say.row);
        case DEEP_COSET_PATH: return reject(ctx, accept, say.path);
        default: break;
    }
    const uint64_t q = N / 4;
    std::vector<uint64_t> pos(t);
    for (uint64_t s = 0; s < t; s++) pos[s] = top[s] % q;
    for (uint32_t k = 0; k < gr.G; k++) SMI_TRY(auth_section(ctx, accept, say, sec + at[k], t, 4 * gr.V[k], logN - 2, pos, roots + 32 * k));
    for (uint32_t k = 0; k < gr.G; k++)
        for (uint64_t x : vals[k])
            if (x >= p) return reject(ctx, accept, say.canonical);
    const uint32_t iota = (uint32_t)powm(fc.omega, q, p);
    for (uint64_t s = 0; s < t; s++) {
        const uint64_t *rec[3] = {nullptr, nullptr, nullptr};
        for (uint32_t k = 0; k < gr.G; k++) rec[k] = &vals[k][s * 4 * (size_t)gr.V[k]];
        const uint32_t x_a = (uint32_t)mulm(cfg->lde_offset, powm(fc.omega, pos[s], p), p);
        if (!deep_coset_q_matches(p, g, W, A, D, w_n, x_a, iota, z, ood.data(), gammas.data(), rec, &coset[16 * s], S)) return reject(ctx, accept, say.composition);
    }
    *accept = 1;
    return SMI_OK;
}
int smi_air_verify_deep_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t *roots, const uint8_t *proof, size_t proof_len,
                              int *accept, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    if (ctx->fs.F.p >= (1u << 30)) return smi_fail(ctx, SMI_ERR_UNSUPPORTED_PRIME, "deep: modulus must be < 2^30");   // the prover's bound (deep.hip)
    return settle(air_verify_deep_fold4_impl(ctx, cfg, (const smi_air *)air, nullptr, roots, proof, proof_len, accept, grind_bits));
}
int smi_air_verify_deep_xargs_fold4(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint8_t *roots, const uint8_t *proof,
                                    size_t proof_len, int *accept, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !xargs || !roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    if (ctx->fs.F.p >= (1u << 30)) return smi_fail(ctx, SMI_ERR_UNSUPPORTED_PRIME, "deep: modulus must be < 2^30");   // the prover's bound (deep.hip)
    return settle(air_verify_deep_fold4_impl(ctx, cfg, (const smi_air *)air, (const smi_air_xargs *)xargs, roots, proof, proof_len, accept, grind_bits));
}

// What the two zero-knowledge verifiers share behind the consistency check: the refusal of a shape without a fold, the fold-by-4
// FRI walk, the opening sections of the groups gr (every group's last column is its salt; the last group holds the 4 D'
// segment columns, the 4 columns of R and the salt; A > 0: the middle group holds the 4 A auxiliary coordinates), every record
// hashed as it stands, the canonical check that leaves the salts out, and Q + R at the four coset points.  objs: the record
// first, then FRI's objects; end: where the sections start.
static int zk_walk_and_open(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_fri_cfg &fc, const char *no_layer, const OpeningWords &say,
                            const DeepGroups &gr, uint32_t A, uint32_t Dp, const uint8_t *roots, const uint8_t *proof, size_t proof_len, size_t end,
                            std::vector<Obj> &objs, const Transcript &tr, const FqH &z, const std::vector<uint64_t> &ood, const std::vector<uint64_t> &gammas,
                            int *accept, uint32_t grind) {
    const uint32_t W = cfg->n_cols, logN = cfg->log_n + cfg->log_blowup, p = ctx->fs.F.p, g = ctx->fs.g, w_n = h_root(ctx, cfg->log_n);
    const uint64_t N = 1ull << logN, t = cfg->num_colinearity_tests;
    if (fri_layout_fold4(fc).F == 0) return reject(ctx, accept, no_layer);
    objs.erase(objs.begin());
    std::vector<uint64_t> top, coset;   // coset: the 16 values of every layer-0 record
    size_t used = 0;
    SMI_TRY(fri_walk_fold4(ctx, fc, tr.seed(), objs, accept, &top, nullptr, nullptr, &coset, &used, grind));
    *accept = 0;
    const uint8_t *sec = proof + end;
    std::vector<uint64_t> vals[3];
    size_t at[3] = {0, 0, 0};
    switch (deep_coset_parse(sec, proof_len - end, gr, t, logN, vals, at)) {
        case DEEP_COSET_LENGTH: return reject(ctx, accept, say.length);
        case DEEP_COSET_RECORD: return reject(ctx, accept, say.row);
        case DEEP_COSET_PATH: return reject(ctx, accept, say.path);
        default: break;
    }
    const uint64_t q = N / 4;
    std::vector<uint64_t> pos(t);
    for (uint64_t s = 0; s < t; s++) pos[s] = top[s] % q;
    for (uint32_t k = 0; k < gr.G; k++) SMI_TRY(auth_section(ctx, accept, say, sec + at[k], t, 4 * gr.V[k], logN - 2, pos, roots + 32 * k));
    for (uint32_t k = 0; k < gr.G; k++)   // every value but the salts, which are the last four of a record
        for (uint64_t s = 0; s < t; s++)
            for (size_t i = 0; i + 4 < 4 * (size_t)gr.V[k]; i++)
                if (vals[k][s * 4 * (size_t)gr.V[k] + i] >= p) return reject(ctx, accept, say.canonical);
    const uint32_t iota = (uint32_t)powm(fc.omega, q, p), last = gr.G - 1;
    std::vector<uint64_t> trow(W), crow(4 * (size_t)A), srow(4 * (size_t)Dp);
    for (uint64_t s = 0; s < t; s++) {
        const uint64_t *r1 = &vals[0][s * 4 * (size_t)gr.V[0]], *r2 = &vals[1][s * 4 * (size_t)gr.V[1]], *r3 = &vals[last][s * 4 * (size_t)gr.V[last]];
        uint32_t x = (uint32_t)mulm(cfg->lde_offset, powm(fc.omega, pos[s], p), p);
        for (uint32_t j = 0; j < 4; j++) {   // column c at point j = value 4 c + j
            for (uint32_t c = 0; c < W; c++) trow[c] = r1[4 * (size_t)c + j];
            for (uint32_t c = 0; c < 4 * A; c++) crow[c] = r2[4 * (size_t)c + j];
            for (uint32_t c = 0; c < 4 * Dp; c++) srow[c] = r3[4 * (size_t)c + j];
            const FqH qv = A ? deep_args_q_at(p, g, W, A, Dp, w_n, x, z, ood.data(), gammas.data(), trow.data(), crow.data(), srow.data())
                             : deep_q_at(p, g, W, Dp, w_n, x, z, ood.data(), gammas.data(), trow.data(), srow.data());
            for (uint32_t e = 0; e < 4; e++)
                if (fp_add(qv.c[e], (uint32_t)r3[4 * (size_t)(4 * Dp + e) + j], p) != coset[16 * s + 4 * e + j]) return reject(ctx, accept, say.composition);
            x = host_mulmod(x, iota, p);
        }
    }
    *accept = 1;
    return SMI_OK;
}

// Verifier of smi_dev_air_prove_deep_zk (include/stark_mi.h, "Zero-knowledge DEEP proofs"): air_verify_deep_fold4_impl for a
// plain AIR with the derived AIR on the left of the consistency check and sum_j z^(j L) s_j on its right, groups of W + 1 and
// 4 D' + 5 columns, the salts hashed as they stand and otherwise ignored, and Q + R at the four coset points.
const OpeningWords ZK_WORDS = {ZK_SENTENCES[0], ZK_SENTENCES[1], ZK_SENTENCES[2], ZK_SENTENCES[3], ZK_SENTENCES[4], ZK_SENTENCES[5]};   // zk_core.h
static int air_verify_deep_zk_impl(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air0, const uint8_t *roots, const uint8_t *proof, size_t proof_len,
                                   int *accept, uint32_t grind) {
    std::string why;
    uint32_t Dp = 0, ks = 0;
    const int vrc = zk_plan(ctx->fs.F.p, cfg, air0, nullptr, &Dp, nullptr, &ks, &why);
    if (vrc != SMI_OK) return smi_fail(ctx, vrc, why.c_str());
    const uint32_t W = cfg->n_cols, K = air0->n_constraints, logN = cfg->log_n + cfg->log_blowup;
    SMI_TRY(domain_check(ctx, logN));
    const uint32_t p = ctx->fs.F.p, g = ctx->fs.g, w_n = h_root(ctx, cfg->log_n);
    ZkAir Z;
    const int drc = zk_derive_air(p, w_n, cfg, air0, &Z, &why);
    if (drc != SMI_OK) return smi_fail(ctx, drc, why.c_str());
    const uint64_t n = 1ull << cfg->log_n;
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, 1ull << cfg->log_blowup);
    const size_t n_ood = 4 * (2 * (size_t)W + Dp);
    size_t end = 0;
    std::vector<Obj> objs = parse(proof, proof_len, 1 + fri_object_count_fold4(fc), &end);
    if (objs.empty() || objs[0].tag != 2 || objs[0].count != n_ood) return reject(ctx, accept, ZK_BAD_RECORD);
    std::vector<uint64_t> ood(n_ood);
    for (size_t i = 0; i < n_ood; i++)
        if ((ood[i] = get_u64(objs[0].p + 8 * i)) >= p) return reject(ctx, accept, ZK_RECORD_CANONICAL);
    Transcript tr;
    std::vector<uint64_t> weights, gammas;
    uint64_t zr[4];
    deep_transcript_weights(tr, roots, W, K, &weights);
    deep_transcript_z(tr, roots + 32, W, K, zr);
    const FqH z = fqh_of(zr, p);
    if (fqh_in_base(z)) return reject(ctx, accept, ZK_Z_IN_BASE_FIELD);
    deep_transcript_gammas(tr, ood.data(), W, K, Dp, &gammas);
    FqH lhs, unused, rhs = fqh(0), pw = fqh(1 % p);
    deep_ood_sides(p, g, cfg, &Z.air, 0, w_n, weights.data(), z, ood.data(), &lhs, &unused);
    const FqH zl = fqh_pow(z, n - ks, p, g);
    for (uint32_t j = 0; j < Dp; j++) {
        rhs = fqh_add(rhs, fqh_mul(pw, fqh_of(ood.data() + 4 * (2 * (size_t)W + j), p), p, g), p);
        pw = fqh_mul(pw, zl, p, g);
    }
    if (!fqh_eq(lhs, rhs)) return reject(ctx, accept, ZK_INCONSISTENT);
    return zk_walk_and_open(ctx, cfg, fc, ZK_NO_LAYER, ZK_WORDS, zk_groups(W, Dp), 0, Dp, roots, proof, proof_len, end, objs, tr, z, ood, gammas, accept, grind);
}
int smi_air_verify_deep_zk(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const uint8_t *roots, const uint8_t *proof, size_t proof_len, int *accept,
                           uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    if (ctx->fs.F.p >= (1u << 30)) return smi_fail(ctx, SMI_ERR_UNSUPPORTED_PRIME, "deep: modulus must be < 2^30");   // the prover's bound (deep.hip)
    return settle(air_verify_deep_zk_impl(ctx, cfg, (const smi_air *)air, roots, proof, proof_len, accept, grind_bits));
}


// Verifier of smi_dev_air_prove_deep_zk_xargs (include/stark_mi.h, "Zero-knowledge DEEP proofs with an argument list"):
// air_verify_deep_zk_impl over three sections.  The transcript is the list variant's with NW = W + K + 3 A; the left side of the
// consistency check is zkargs_core.h's zkx_ood_lhs over the derived AIR with both exemption columns; Q + R at the four coset
// points goes through deep_args_q_at with D' segments.
const OpeningWords ZKX_WORDS = {ZKX_SENTENCES[0], ZKX_SENTENCES[1], ZKX_SENTENCES[2], ZKX_SENTENCES[3], ZKX_SENTENCES[4], ZKX_SENTENCES[5]};   // zkargs_core.h
static int air_verify_deep_zk_xargs_impl(smi_ctx *ctx, const smi_stark_cfg *cfg, const smi_air *air0, const smi_air_xargs *xargs, const uint8_t *roots,
                                         const uint8_t *proof, size_t proof_len, int *accept, uint32_t grind) {
    std::string why;
    uint32_t Dp = 0, ks = 0;
    const int vrc = zkx_plan(ctx->fs.F.p, cfg, air0, xargs, nullptr, &Dp, nullptr, &ks, &why);
    if (vrc != SMI_OK) return smi_fail(ctx, vrc, why.c_str());
    const int prc = xargs_periodic_check(ctx->fs.F.p, air0, cfg->log_n, &why);
    if (prc != SMI_OK) return smi_fail(ctx, prc, why.c_str());
    const uint32_t W = cfg->n_cols, K = air0->n_constraints, A = xargs->count, logN = cfg->log_n + cfg->log_blowup;
    const uint64_t NW = (uint64_t)W + K + 3 * (uint64_t)A;
    SMI_TRY(domain_check(ctx, logN));
    const uint32_t p = ctx->fs.F.p, g = ctx->fs.g, w_n = h_root(ctx, cfg->log_n);
    ZkAir Z;
    const int drc = zk_derive_air(p, w_n, cfg, air0, &Z, &why, true);
    if (drc != SMI_OK) return smi_fail(ctx, drc, why.c_str());
    const uint64_t n = 1ull << cfg->log_n;
    const smi_fri_cfg fc = trace_fri_cfg(ctx, cfg, 1ull << cfg->log_blowup);
    const size_t n_ood = deep_args_record(W, A, Dp);
    size_t end = 0;
    std::vector<Obj> objs = parse(proof, proof_len, 1 + fri_object_count_fold4(fc), &end);
    if (objs.empty() || objs[0].tag != 2 || objs[0].count != n_ood) return reject(ctx, accept, ZKX_BAD_RECORD);
    std::vector<uint64_t> ood(n_ood);
    for (size_t i = 0; i < n_ood; i++)
        if ((ood[i] = get_u64(objs[0].p + 8 * i)) >= p) return reject(ctx, accept, ZKX_RECORD_CANONICAL);
    Transcript tr;
    std::vector<uint64_t> ch, weights, gammas;
    uint64_t zr[4];
    transcript_perm_challenges(tr, roots, &ch);
    transcript_indexed(tr, roots + 32, 8, 4 * NW, &weights);
    deep_args_transcript_z(tr, roots + 64, NW, zr);
    const FqH z = fqh_of(zr, p);
    if (fqh_in_base(z)) return reject(ctx, accept, ZKX_Z_IN_BASE_FIELD);
    deep_args_transcript_gammas(tr, ood.data(), NW, n_ood, &gammas);
    const FqH lhs = zkx_ood_lhs(p, g, cfg, &Z.air, xargs, w_n, ch.data(), weights.data(), z, ood.data());
    FqH rhs = fqh(0), pw = fqh(1 % p);
    const FqH zl = fqh_pow(z, n - ks, p, g);
    for (uint32_t j = 0; j < Dp; j++) {
        rhs = fqh_add(rhs, fqh_mul(pw, fqh_of(ood.data() + 4 * (2 * (size_t)W + 2 * (size_t)A + j), p), p, g), p);
        pw = fqh_mul(pw, zl, p, g);
    }
    if (!fqh_eq(lhs, rhs)) return reject(ctx, accept, ZKX_INCONSISTENT);
    return zk_walk_and_open(ctx, cfg, fc, ZKX_NO_LAYER, ZKX_WORDS, zkx_groups(W, A, Dp), A, Dp, roots, proof, proof_len, end, objs, tr, z, ood, gammas, accept,
                            grind);
}
int smi_air_verify_deep_zk_xargs(smi_ctx *ctx, const smi_stark_cfg *cfg, const void *air, const void *xargs, const uint8_t *roots, const uint8_t *proof,
                                 size_t proof_len, int *accept, uint32_t grind_bits) {
    if (!ctx || !cfg || !air || !xargs || !roots || (!proof && proof_len) || !accept) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    *accept = 0;
    SMI_TRY(grind_bits_check(ctx, grind_bits));
    SMI_TRY(ext_field_check(ctx));
    if (ctx->fs.F.p >= (1u << 30)) return smi_fail(ctx, SMI_ERR_UNSUPPORTED_PRIME, "deep: modulus must be < 2^30");   // the prover's bound (deep.hip)
    return settle(air_verify_deep_zk_xargs_impl(ctx, cfg, (const smi_air *)air, (const smi_air_xargs *)xargs, roots, proof, proof_len, accept, grind_bits));
}
