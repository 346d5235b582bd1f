// zk_core.h -- what zero-knowledge DEEP proofs add (include/stark_mi.h, "Zero-knowledge DEEP proofs"), shared
// by the kernels of zk.hip and the CPU emulator (emu_zk.cpp): the lane body of the device random generator, the lane body of
// the masked split of the composition, and on the host the derived AIR with its exemption column and the plan.
#pragma once
#include <mutex>
#include <string>
#include <vector>

#include "deep_core.h"
#include "hash_core.h"

#define ZK_BLOCK 256
#define ZK_RAND_PER_LANE 8   // two digests of four u64 words
#define ZK_MAX_RECORD 64     // the widest coset leaf the tree builder takes

// ------------------------------------------------------------------------------------------------ random residues
// Output element i is word (i mod 4) of Hash::from_bytes(seed || stream_id as 8 LE bytes || floor(i / 4) as 8 LE bytes), read
// as a little-endian u64 and reduced mod p.  The 40 leading bytes are the same for every block, so they travel as the
// transcript midstate that the grinding search uses (hash_core.h fs_seed: the state after the whole chunk `seed` and its
// mix, with the 8 stream bytes absorbed at positions 0..7, phase 8); a lane absorbs the counter at positions 8..15, runs the
// short chunk's mix and the 8 closing ones on two hashes at once (hashc::grind_pair's state) and keeps all 32 digest bytes.
struct ZkRandSeed {
    uint32_t mid[16];
};
inline ZkRandSeed zk_rand_seed(const uint8_t seed[32], uint64_t stream_id) {
    uint8_t msg[40];
    for (int i = 0; i < 32; i++) msg[i] = seed[i];
    for (int i = 0; i < 8; i++) msg[32 + i] = (uint8_t)(stream_id >> (8 * i));
    ZkRandSeed s;
    uint32_t phase = 0;
    hashc::fs_seed(msg, 40, s.mid, &phase);   // phase == 8
    return s;
}
// the digests of the block counters c0 and c1 in natural layout
SMI_HD void zk_rand_pair(const uint32_t mid[16], uint64_t c0, uint64_t c1, uint32_t d0[8], uint32_t d1[8]) {
    hashc::State2 st;
#pragma unroll
    for (int w = 0; w < 32; w++) st.s[w] = ((mid[w & 15] >> ((w & 16) ? 16 : 0)) & 0xFFu) * 0x00010001u;
    const hashc::MixK K = hashc::mix_consts();
#pragma unroll
    for (int i = 0; i < 8; i++) hashc::grind_absorb_at(st, 8 + i, hashc::grind_byte2(c0, c1, (uint32_t)i));
    hashc::mix2_t<false>(st, K);
#pragma unroll 1
    for (int k = 0; k < 8; k++) hashc::mix2_t<true>(st, K);
    hashc::flush2(st);
    hashc::to_words2(st, d0, d1);
}
// a little-endian u64 (lo, hi) mod p without a 64-bit division
SMI_HD uint32_t zk_reduce(uint32_t lo, uint32_t hi, const Fp &F) { return from_mont(to_mont_u64(((uint64_t)hi << 32) | lo, F), F); }
// the eight residues of lane `lane`: elements 8 lane .. 8 lane + 7
SMI_HD void zk_rand_lane(const uint32_t mid[16], uint64_t lane, const Fp &F, uint32_t v[ZK_RAND_PER_LANE]) {
    uint32_t d0[8], d1[8];
    zk_rand_pair(mid, 2 * lane, 2 * lane + 1, d0, d1);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[k] = zk_reduce(d0[2 * k], d0[2 * k + 1], F);
        v[4 + k] = zk_reduce(d1[2 * k], d1[2 * k + 1], F);
    }
}

// ------------------------------------------------------------------------------------------------ masked segments
// Column 4 j + e of the output holds the n coefficients of coordinate e of H~_j.  With L = n - k_s:
//   m <  L:  H_e[j L + m] (0 at and above h_len), minus rho_{j-1,e}[m] when j >= 1 and m < k_s
//   m >= L:  rho_{j,e}[m - L] when j < D' - 1, else 0
// rho_{j,e} sits at rho + (4 j + e) k_s.  A lane makes four consecutive coefficients m0 .. m0 + 3 (m0 a multiple of 4) of
// one column.  j L + m0 is no multiple of 4 in general (k_s is odd), so the lane reads the two aligned groups of four that
// cover its window and picks by the offset s = (j L + m0) mod 4, a value that is uniform over a column.
struct ZkSegShape {
    uint64_t n, L, h_len;
    uint32_t ks, Dp;
};
// the window's first word `at` -> its aligned base and the offset into the eight words loaded from there
SMI_HD uint64_t zk_seg_window(uint64_t at, uint32_t *s) {
    *s = (uint32_t)(at & 3);
    return at & ~(uint64_t)3;
}
// words s .. s + 3 of the eight words lo | hi, without indexing registers by a run-time value
SMI_HD void zk_seg_pick(const uint32_t lo[4], const uint32_t hi[4], uint32_t s, uint32_t h[4]) {
    switch (s) {
    case 0: h[0] = lo[0], h[1] = lo[1], h[2] = lo[2], h[3] = lo[3]; break;
    case 1: h[0] = lo[1], h[1] = lo[2], h[2] = lo[3], h[3] = hi[0]; break;
    case 2: h[0] = lo[2], h[1] = lo[3], h[2] = hi[0], h[3] = hi[1]; break;
    default: h[0] = lo[3], h[1] = hi[0], h[2] = hi[1], h[3] = hi[2]; break;
    }
}
// h[q] = H_e[j L + m0 + q] as loaded (0 past h_len; ignored where m0 + q >= L) -> out[q] = coefficient m0 + q
SMI_HD void zk_seg_words(const ZkSegShape &S, uint32_t j, uint32_t e, uint64_t m0, const uint32_t h[4], const uint32_t *__restrict__ rho, uint32_t p,
                         uint32_t out[4]) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint64_t m = m0 + q;
        uint32_t v;
        if (m < S.L) {
            v = h[q];
            if (j && m < S.ks) v = fp_sub(v, rho[(size_t)(4 * (j - 1) + e) * S.ks + m], p);
        } else {
            v = j + 1 < S.Dp ? rho[(size_t)(4 * j + e) * S.ks + (m - S.L)] : 0u;
        }
        out[q] = v;
    }
}

// The whole group: what a lane of zk_segments_kernel runs and what the emulator runs.  load4(src, at, len, v) fetches four
// words from `at` (a multiple of 4), 0 at and above len; store4(dst, at, len, v) writes four words.
template <class Load4, class Store4>
SMI_HD void zk_seg_group(const ZkSegShape &S, uint32_t col, uint64_t m0, const uint32_t *__restrict__ hc, size_t h_stride, const uint32_t *__restrict__ rho,
                         uint32_t *__restrict__ out, size_t out_stride, uint32_t p, Load4 &&load4, Store4 &&store4) {
    const uint32_t j = col >> 2, e = col & 3;
    const uint32_t *src = hc + (size_t)e * h_stride;
    uint32_t s, lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0}, h[4], o[4];
    const uint64_t a0 = zk_seg_window((uint64_t)j * S.L + m0, &s);
    if (m0 < S.L) {   // a group wholly behind L reads rho only
        load4(src, a0, S.h_len, lo);
        if (s) load4(src, a0 + 4, S.h_len, hi);
    }
    zk_seg_pick(lo, hi, s, h);
    zk_seg_words(S, j, e, m0, h, rho, p, o);
    store4(out + (size_t)col * out_stride, m0, S.n, o);
}

// ------------------------------------------------------------------------------------------------ the derived AIR and the plan
// Stream identifiers of smi_dev_random_fill inside one proof (include/stark_mi.h): every random value comes from one of these.
enum : uint64_t { ZK_STREAM_ROWS = 1, ZK_STREAM_SALT1 = 2, ZK_STREAM_RHO = 3, ZK_STREAM_MASK = 4, ZK_STREAM_SALT2 = 5 };

#define ZK_BAD_RECORD "zk deep: the out-of-domain record is missing or has the wrong count"
#define ZK_RECORD_CANONICAL "zk deep: an out-of-domain coordinate is not canonical"
#define ZK_Z_IN_BASE_FIELD "zk deep: the out-of-domain point z lies in the base field"
#define ZK_INCONSISTENT "zk deep: out-of-domain consistency check fails: the derived AIR's constraints at z do not give the masked segments' value"
#define ZK_NO_LAYER "zk deep: FRI has no fold at this shape (F = 0), so there is no layer-0 coset to compare the masked DEEP quotient with"
static const char *const ZK_SENTENCES[6] = {"zk deep coset openings: wrong length",
                                            "zk deep coset openings: malformed record",
                                            "zk deep coset openings: malformed path",
                                            "zk deep coset openings: authentication path does not verify",
                                            "zk deep coset openings: an opened value is not canonical",
                                            "zk deep coset openings: the masked DEEP quotient of the opened cosets is not the codeword value"};

inline uint32_t zk_kt(uint64_t t) { return (uint32_t)(8 * t + 8); }
inline uint32_t zk_ks(uint64_t t) { return (uint32_t)(4 * t + 1); }

// The caller's AIR with one more periodic column of period n, index Q, that every transition term is multiplied by.  The
// column holds E(tau w^r), E(x) = prod_{r = n - k_t - 1}^{n - 2} (x - tau w^r): zero exactly on the exempt rows.  w_n == 0:
// the column is left zero (the plan needs the shape only).  Variables 2 W + Q + j (periodic j at the next row) move up by one.
struct ZkAir {
    std::vector<uint32_t> cft, tff, var, exp, bcol, plog;
    std::vector<uint64_t> coeff, brow, bval, pval;
    smi_air air;
};
// E(tau w^r) for r < n in about 8 n products.  With x_r = tau w^r, a = n - k_t - 1 and b = n - 2 the value is
// F(r) = prod_{q = a}^{b} (x_r - x_q), and F(r + 1) = w^k_t F(r) (x_r - x_{a-1}) / (x_r - x_b): the window of roots slides by
// one.  F(0) and F(n - 1) are taken from the definition, rows a .. b are zero, and the denominators of rows 0 .. a - 2
// share one inversion (Montgomery's trick).
inline void zk_exemption_column(uint32_t p, uint32_t tau, uint32_t w_n, uint32_t log_n, uint32_t kt, uint64_t *out) {
    const uint64_t n = 1ull << log_n, a = n - kt - 1, b = n - 2;
    std::vector<uint32_t> pt(n);
    uint32_t x = tau % p;
    for (uint64_t r = 0; r < n; r++) pt[r] = x, x = host_mulmod(x, w_n, p);
    auto direct = [&](uint64_t r) {
        uint32_t v = 1 % p;
        for (uint64_t q = a; q <= b; q++) v = host_mulmod(v, fp_sub(pt[r], pt[q], p), p);
        return v;
    };
    for (uint64_t r = 0; r < n; r++) out[r] = 0;
    out[0] = direct(0);
    out[n - 1] = direct(n - 1);
    if (a >= 2) {   // rows 1 .. a - 1 by the recurrence
        std::vector<uint32_t> pre(a - 1);   // prefix products of den_r = x_r - x_b, r = 0 .. a - 2 (never zero: r < b)
        uint32_t acc = 1 % p;
        for (uint64_t r = 0; r + 1 < a; r++) pre[r] = acc = host_mulmod(acc, fp_sub(pt[r], pt[b], p), p);
        uint32_t inv = host_powmod(acc, p - 2, p);
        std::vector<uint32_t> dinv(a - 1);
        for (uint64_t r = a - 1; r-- > 0;) {
            dinv[r] = r ? host_mulmod(inv, pre[r - 1], p) : inv;
            inv = host_mulmod(inv, fp_sub(pt[r], pt[b], p), p);
        }
        const uint32_t wk = host_powmod(w_n, kt, p);
        for (uint64_t r = 0; r + 1 < a; r++) {
            const uint32_t step = host_mulmod(host_mulmod(wk, fp_sub(pt[r], pt[a - 1], p), p), dinv[r], p);
            out[r + 1] = host_mulmod((uint32_t)out[r], step, p);
        }
    }
}
// list: the derived AIR of "Zero-knowledge DEEP proofs with an argument list" (zkargs_core.h) -- k_t = 8 t + 16, the sentences
// start "zk deep argument:", and a second column of period n, index Q + 1, holds E_A(tau w^r), E_A(x) = prod_{r = n - k_t}^{n - 1}
// (x - tau w^r) = w^k_t E(x / w): row r + 1 is w^k_t times row r of the first column.  No constraint reads it.
inline int zk_derive_air(uint64_t p64, uint32_t w_n, const smi_stark_cfg *cfg, const smi_air *air, ZkAir *Z, std::string *why, bool list = false) {
    auto fail = [&](int code, const std::string &s) {
        if (why) *why = s;
        return code;
    };
    // the caller's own AIR first: everything below indexes its tables
    const int rc = air_validate(p64, cfg, air, nullptr, nullptr, why, true);
    if (rc != SMI_OK) return rc;
    const uint32_t W = cfg->n_cols, Q = air->n_periodic, K = air->n_constraints, nt = air->n_terms, nb = air->n_boundary;
    const uint64_t n = 1ull << cfg->log_n, kt = zk_kt(cfg->num_colinearity_tests) + (list ? 8 : 0);
    const std::string who = list ? "zk deep argument: " : "zk deep: ";
    const uint32_t extra = list ? 2 : 1;   // the periodic columns the derivation adds
    if (cfg->num_colinearity_tests > (1u << 20) || kt >= n / 2)
        return fail(SMI_ERR_BAD_ARG, who + "k_t = 8 t + " + (list ? "16" : "8") + " = " + std::to_string(kt) +
                                         " >= n / 2: the randomiser rows would outnumber the statement's");
    if (list && Q + 2 > SMI_AIR_MAX_PERIODIC)
        return fail(SMI_ERR_BAD_ARG, who + "Q + 2 = " + std::to_string(Q + 2) + " > SMI_AIR_MAX_PERIODIC (" + std::to_string(SMI_AIR_MAX_PERIODIC) +
                                         "): no room for the two exemption columns");
    for (uint32_t j = 0; j < nb; j++)
        if (air->boundary_row[j] >= n - kt)
            return fail(SMI_ERR_BAD_ARG, who + "boundary point " + std::to_string(j) + " lies on row " + std::to_string(air->boundary_row[j]) +
                                             " >= n - k_t = " + std::to_string(n - kt) + ", a randomiser row");
    Z->cft.assign(air->constraint_first_term, air->constraint_first_term + K + 1);
    Z->coeff.assign(air->term_coeff, air->term_coeff + nt);
    Z->tff.assign(nt + 1, 0);
    Z->var.clear();
    Z->exp.clear();
    for (uint32_t t = 0; t < nt; t++) {
        for (uint32_t f = air->term_first_factor[t]; f < air->term_first_factor[t + 1]; f++) {
            const uint32_t v = air->factor_var[f];
            Z->var.push_back(v >= 2 * W + Q ? v + extra : v);
            Z->exp.push_back(air->factor_exp[f]);
        }
        Z->var.push_back(2 * W + Q);
        Z->exp.push_back(1);
        Z->tff[t + 1] = (uint32_t)Z->var.size();
    }
    Z->bcol.assign(air->boundary_col, air->boundary_col + nb);
    Z->brow.assign(air->boundary_row, air->boundary_row + nb);
    Z->bval.assign(air->boundary_value, air->boundary_value + nb);
    uint64_t at = 0;
    for (uint32_t j = 0; j < Q; j++) at += 1ull << air->periodic_log_period[j];
    Z->plog.assign(air->periodic_log_period, air->periodic_log_period + Q);
    for (uint32_t k = 0; k < extra; k++) Z->plog.push_back(cfg->log_n);
    Z->pval.assign(air->periodic_value, air->periodic_value + at);
    Z->pval.resize(at + extra * n, 0);
    if (w_n) {   // the column depends on (p, tau, w_n, n, k_t) alone: the last one made is kept for the next proof of that shape
        static std::mutex mu;
        static uint64_t key[5] = {0, 0, 0, 0, 0};
        static std::vector<uint64_t> kept;
        const uint64_t want[5] = {p64, cfg->trace_offset, w_n, cfg->log_n, kt};
        std::lock_guard<std::mutex> lock(mu);
        if (memcmp(key, want, sizeof key) != 0 || kept.size() != extra * n) {   // k_t tells the two forms apart
            kept.assign(extra * n, 0);
            zk_exemption_column((uint32_t)p64, (uint32_t)cfg->trace_offset, w_n, cfg->log_n, (uint32_t)kt, kept.data());
            if (list) {
                const uint32_t wk = host_powmod(w_n, kt, (uint32_t)p64);
                uint64_t *ea = kept.data() + n;
                for (uint64_t r = 0; r < n; r++) ea[(r + 1) & (n - 1)] = host_mulmod((uint32_t)kept[r], wk, (uint32_t)p64);
            }
            memcpy(key, want, sizeof key);
        }
        memcpy(Z->pval.data() + at, kept.data(), extra * n * 8);
    }
    smi_air &a = Z->air;
    a.n_constraints = K, a.n_terms = nt, a.n_factors = (uint32_t)Z->var.size(), a.n_boundary = nb;
    a.constraint_first_term = Z->cft.data(), a.term_coeff = Z->coeff.data(), a.term_first_factor = Z->tff.data();
    a.factor_var = Z->var.data(), a.factor_exp = Z->exp.data();
    a.boundary_col = Z->bcol.data(), a.boundary_row = Z->brow.data(), a.boundary_value = Z->bval.data();
    a.n_periodic = Q + extra, a.window = 0;
    a.periodic_log_period = Z->plog.data(), a.periodic_value = Z->pval.data();
    return SMI_OK;
}

// smi_air_plan_deep_zk: the two refusals of the derived AIR, the DEEP plan of the derived AIR (d, D), then
// D' = ceil(D n / (n - k_s)) with 4 D' + 5 <= 64 and W + 1 <= 64
inline int zk_plan(uint64_t p, const smi_stark_cfg *cfg, const smi_air *air, uint32_t *degree, uint32_t *segments, uint32_t *kt_out, uint32_t *ks_out,
                   std::string *why, uint32_t *D_out = nullptr) {
    auto fail = [&](int code, const std::string &s) {
        if (why) *why = s;
        return code;
    };
    if (!cfg || !air) return fail(SMI_ERR_BAD_ARG, "air: null argument");
    ZkAir Z;
    int rc = zk_derive_air(p, 0, cfg, air, &Z, why);
    if (rc != SMI_OK) return rc;
    uint32_t d = 0, D = 0;
    rc = deep_plan(p, cfg, &Z.air, &d, &D, why);
    if (rc != SMI_OK) return rc;
    const uint64_t n = 1ull << cfg->log_n, ks = zk_ks(cfg->num_colinearity_tests), L = n - ks;   // k_s < k_t < n / 2
    const uint64_t Dp = ((uint64_t)D * n + L - 1) / L;
    if (4 * Dp + 5 > ZK_MAX_RECORD)
        return fail(SMI_ERR_BAD_ARG, "zk deep: 4 D' + 5 = " + std::to_string(4 * Dp + 5) + " > 64: a leaf of the segment tree is wider than the leaf hash takes");
    if (cfg->n_cols + 1 > ZK_MAX_RECORD) return fail(SMI_ERR_BAD_ARG, "zk deep: W + 1 > 64: the trace tree has no room for the salt column");
    if (degree) *degree = d;
    if (segments) *segments = (uint32_t)Dp;
    if (D_out) *D_out = D;
    if (kt_out) *kt_out = zk_kt(cfg->num_colinearity_tests);
    if (ks_out) *ks_out = (uint32_t)ks;
    return SMI_OK;
}

// the groups of a proof: the trace with its salt column; the segments, R and their salt column
inline DeepGroups zk_groups(uint32_t W, uint32_t Dp) {
    DeepGroups gr;
    gr.G = 2;
    gr.V[0] = W + 1;
    gr.V[1] = 4 * Dp + 5;
    gr.V[2] = 0;
    return gr;
}
// 9 + 32 (2 W + D') + len_FRI4(N, B, t) + the two sections
inline size_t zk_proof_len(const smi_stark_cfg *cfg, uint32_t Dp, uint64_t *folds) {
    const uint32_t W = cfg->n_cols, log_N = cfg->log_n + cfg->log_blowup;
    const FriFold4Layout lay = fri_layout_fold4(deep_fri_cfg(cfg, 1));
    if (folds) *folds = lay.F;
    return 9 + 32 * (2 * (size_t)W + Dp) + lay.proof_len + deep_coset_sections_len(zk_groups(W, Dp), cfg->num_colinearity_tests, log_N);
}
