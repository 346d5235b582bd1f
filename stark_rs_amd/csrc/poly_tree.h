// poly_tree.h -- subproduct trees over arbitrary points: the zerofier, multipoint evaluation and interpolation
// (Polynomial::zerofier / eval_domain / interpolate_domain, src/univariate/{mod,eval,interpolate}.rs) as a sequence of
// batched NTTs and small kernels.  Templated on a launcher so that the HIP path (poly.hip) and the CPU emulator of the
// non-GPU tests (emu_poly.cpp) share every decision about levels, sizes and buffers, as ntt_driver.h does for the NTT.
//
// Launcher concept (every call is a no-op once rc != SMI_OK):
//   int rc;
//   void ntt(const uint32_t *in, uint32_t *out, uint32_t L, uint64_t n_in, uint32_t batch, uint64_t in_stride,
//            uint64_t out_stride, int inverse);     // dev_ntt with offset 1 (batch <= SMI_POLY_NTT_BATCH)
//   void ew(int op, const PolyEw &a);              // poly_ew<op> for every i < a.n
//   void block(const PolyBlockArgs &a, uint64_t blocks);
//   void horner(const PolyHornerArgs &a, uint64_t blocks);
//   uint32_t read_word(const uint32_t *p);         // waits for the work queued so far
//
// Levels (poly_core.h): the n points sit at the leaves of a tree of N = 2^k leaves, padded with the constant 1; level j
// holds N >> j nodes of 2^j + 1 coefficients.  Levels up to b come from the LDS block kernel; above, node c of level
// j is the product of nodes 2c and 2c+1 of level j - 1, taken by size-2^j transforms: the product of two monic degree-2^(j-1)
// nodes has degree 2^j, and its one wrapped term (the leading 1) is put back by PEW_TREE_FIX.  Only the node holding
// the last point can be partial; its degree is below 2^j and nothing wraps.
//
// Evaluation (scaled remainder tree, Bernstein; Bostan-Lecerf-Schost): a node v of degree d_v carries the first d_v
// coefficients g_v of (f mod M_v) / M_v as a series in 1/x.  At the root they come from one power-series inverse of
// rev(Z); a child u with sibling w takes g_u[t] = sum_k M_w[k] g_v[t + k], a middle product.  Stored reversed in a slot
// of the parent's transform size (H_v[i] = g_v[2^j - 1 - i]) it is the upper half of the cyclic product M_w * H_v of
// size 2^j, so a level costs one transform of the parents' H, one of the children's M (the product tree's own
// operands), one pointwise kernel and one batched inverse.  At the blocks PolyHorner takes over.
//
// Interpolation: Z = the root; Z' evaluated by the descent; c_i = v_i / Z'(d_i) (a zero means a repeated point);
// numerators N_v = N_l M_r + N_r M_l upward (degree < 2^j, no wrap), the bottom levels in the block kernel.
#pragma once
#include <string.h>

#include "../../include/stark_mi.h"
#include "poly_core.h"

#define SMI_POLY_NTT_BATCH 32768u   // columns per dev_ntt call (dev_ntt takes at most 65535)

struct PolyShape {
    uint64_t n;      // points
    uint64_t nf;     // coefficients of the evaluated polynomial (evaluation), n (interpolation), 0 (zerofier only)
    uint64_t m;      // length of the root's series: max(nf, n), or 0 without evaluation
    uint32_t k, b;   // N = 2^k leaves, blocks of 2^b leaves
    uint32_t Lm;     // root products: 2^Lm >= 2m - 1
    bool interp;
};

// Sizes of a call on n points (nf coefficients to evaluate); SMI_ERR_ROOT_TOO_LARGE when a transform would exceed 2^K.
// The entry points answer n == 0 before they get here.
inline int poly_shape(uint64_t n, uint64_t nf, bool eval, bool interp, uint32_t K, PolyShape *s) {
    memset(s, 0, sizeof *s);
    s->n = n;
    s->interp = interp;
    while ((1ull << s->k) < n) s->k++;
    s->b = s->k < SMI_POLY_BLOCK_LOG ? s->k : SMI_POLY_BLOCK_LOG;
    if (s->k > K) return SMI_ERR_ROOT_TOO_LARGE;
    if (eval || interp) {
        s->nf = interp ? n : nf;
        s->m = s->nf > n ? s->nf : n;
        while ((1ull << s->Lm) < 2 * s->m - 1) s->Lm++;
        if (s->Lm > K) return SMI_ERR_ROOT_TOO_LARGE;
    }
    return SMI_OK;
}

struct PolyWs {
    uint32_t *lev[33];
    uint32_t *pts, *coef, *vals, *flag;                   // inputs (n points, nf coefficients or n values), results
    uint32_t *fa, *fh;                                    // 2N, N: transforms of a level
    uint32_t *rz, *g, *e, *rf, *prod, *f1, *f2, *hroot;   // the root's series (m each, 2^Lm, 2^Lm, N)
    uint32_t *zp, *zv, *cw, *fb, *num;                    // interpolation: Z', Z'(d_i), c_i (n each), 2N, N
    // Assigns the buffers from base (nullptr: sizes only) and returns the words used.
    uint64_t carve(uint32_t *base, const PolyShape &s) {
        uint64_t off = 0;
        auto take = [&](uint64_t words) -> uint32_t * {
            uint32_t *q = base ? base + off : nullptr;
            off += (words + 63) & ~(uint64_t)63;   // 256-byte alignment
            return q;
        };
        const uint64_t N = 1ull << s.k, m = s.m, cap = 1ull << s.Lm;
        memset(lev, 0, sizeof lev);
        for (uint32_t j = s.b; j <= s.k; j++) lev[j] = take(N + (N >> j));
        pts = take(s.n);
        flag = take(1);
        fa = take(2 * N);
        fh = take(N);
        coef = vals = rz = g = e = rf = prod = f1 = f2 = hroot = zp = zv = cw = fb = num = nullptr;
        if (m) {
            coef = take(s.interp ? s.n : s.nf);
            vals = take(s.n);
            rz = take(m); g = take(m); e = take(m); rf = take(m); prod = take(m);
            f1 = take(cap); f2 = take(cap);
            hroot = take(N);
        }
        if (s.interp) {
            zp = take(s.n); zv = take(s.n); cw = take(s.n);
            fb = take(2 * N);
            num = take(N);
        }
        return off;
    }
};

template <class Ln> inline void poly_ew_run(Ln &ln, int op, uint32_t *out, const uint32_t *a, const uint32_t *b, uint64_t n, const Fp &F,
                                            uint64_t s0 = 0, uint64_t s1 = 0, uint64_t s2 = 0, uint32_t v = 0, uint32_t *flag = nullptr) {
    PolyEw w;
    w.out = out; w.a = a; w.b = b; w.flag = flag; w.n = n; w.s0 = s0; w.s1 = s1; w.s2 = s2; w.v = v; w.F = F;
    if (n) ln.ew(op, w);
}

// batched transform of any batch size (dev_ntt's limit is 65535 columns)
template <class Ln> inline void poly_ntt(Ln &ln, const uint32_t *in, uint32_t *out, uint32_t L, uint64_t n_in, uint64_t batch, uint64_t is,
                                         uint64_t os, int inverse) {
    for (uint64_t c0 = 0; c0 < batch; c0 += SMI_POLY_NTT_BATCH) {
        const uint64_t nb = batch - c0 < SMI_POLY_NTT_BATCH ? batch - c0 : SMI_POLY_NTT_BATCH;
        ln.ntt(in + c0 * is, out + c0 * os, L, n_in, (uint32_t)nb, is, os, inverse);
    }
}

// first `keep` coefficients of x * y into out (f1, f2: 2^L words each, 2^L >= nx + ny - 1; out may alias x or y)
template <class Ln> inline void poly_mul_trunc(Ln &ln, const uint32_t *x, uint64_t nx, const uint32_t *y, uint64_t ny, uint32_t *out, uint64_t keep,
                                               uint32_t *f1, uint32_t *f2, const Fp &F) {
    const uint64_t n = nx + ny - 1;
    uint32_t L = 0;
    while ((1ull << L) < n) L++;
    const uint64_t N = 1ull << L;
    ln.ntt(x, f1, L, nx, 1, nx, N, 0);
    ln.ntt(y, f2, L, ny, 1, ny, N, 0);
    poly_ew_run(ln, PEW_MUL, f1, f2, nullptr, N, F);
    ln.ntt(f1, f1, L, N, 1, N, N, 1);
    poly_ew_run(ln, PEW_COPY_TRUNC, out, f1, nullptr, keep, F, n);
}

// g = rb^-1 mod x^k by Newton iteration (rb[0] = 1 / g0, rb has k coefficients): g_1 = g0,
// g_2t = g_t * (2 - rb * g_t) mod x^2t.  e: k words; f1, f2: 2^L words each, 2^L >= 2k - 1.
template <class Ln> inline void poly_series_inv(Ln &ln, const uint32_t *rb, uint64_t k, uint32_t g0, uint32_t *g, uint32_t *e, uint32_t *f1,
                                                uint32_t *f2, const Fp &F) {
    poly_ew_run(ln, PEW_SET_FIRST, g, nullptr, nullptr, k, F, 0, 0, 0, g0);
    for (uint64_t t = 1; t < k; t <<= 1) {
        const uint64_t t2 = 2 * t < k ? 2 * t : k;
        poly_mul_trunc(ln, rb, t2, g, t, e, t2, f1, f2, F);
        poly_ew_run(ln, PEW_TWO_MINUS, e, nullptr, nullptr, t2, F);
        poly_mul_trunc(ln, g, t, e, t2, g, t2, f1, f2, F);
    }
}

// the product tree of w.pts: the root Z (n + 1 coefficients) ends at w.lev[k]
template <class Ln> inline void poly_tree_build(Ln &ln, const PolyShape &s, const PolyWs &w, const Fp &F) {
    const uint64_t N = 1ull << s.k;
    PolyBlockArgs ba;
    memset(&ba, 0, sizeof ba);
    ba.pts = w.pts; ba.m_out = w.lev[s.b]; ba.n = s.n; ba.b = s.b; ba.F = F;
    ln.block(ba, N >> s.b);
    for (uint32_t j = s.b + 1; j <= s.k; j++) {
        const uint64_t P = N >> j, cw = (1ull << (j - 1)) + 1, h = 1ull << j;
        poly_ntt(ln, w.lev[j - 1], w.fa, j, cw, 2 * P, cw, h, 0);
        poly_ew_run(ln, PEW_PAIR_MUL, w.fa, nullptr, nullptr, P * h, F, j);
        poly_ntt(ln, w.fa, w.lev[j], j, h, P, 2 * h, h + 1, 1);
        poly_ew_run(ln, PEW_TREE_FIX, w.lev[j], w.lev[j - 1], nullptr, P, F, j - 1);
    }
}

// values[i] = f(pts[i]) for the nf coefficients in f, on the tree built by poly_tree_build
template <class Ln> inline void poly_tree_eval(Ln &ln, const PolyShape &s, const PolyWs &w, const uint32_t *f, uint64_t nf, uint32_t *values,
                                               const Fp &F) {
    const uint64_t N = 1ull << s.k, n = s.n, m = s.m;
    // root: g = (rev(f) * rev(Z)^-1 mod x^m)[m - n, m); H_root[i] = g[N - 1 - i] (zero beyond the root's degree n)
    poly_ew_run(ln, PEW_REV, w.rz, w.lev[s.k], nullptr, m, F, n, n + 1);
    poly_series_inv(ln, w.rz, m, 1u, w.g, w.e, w.f1, w.f2, F);
    poly_ew_run(ln, PEW_REV, w.rf, f, nullptr, m, F, m - 1, nf);
    poly_mul_trunc(ln, w.rf, m, w.g, m, w.prod, m, w.f1, w.f2, F);
    poly_ew_run(ln, PEW_ROOT_H, w.hroot, w.prod, nullptr, N, F, N, n, m);
    const uint32_t *h = w.hroot;
    uint64_t hs = N;
    for (uint32_t j = s.k; j > s.b; j--) {   // parents at level j, children at j - 1, transforms of 2^j
        const uint64_t P = N >> j, cw = (1ull << (j - 1)) + 1, sz = 1ull << j;
        poly_ntt(ln, h, w.fh, j, sz, P, hs, sz, 0);
        poly_ntt(ln, w.lev[j - 1], w.fa, j, cw, 2 * P, cw, sz, 0);
        poly_ew_run(ln, PEW_CROSS, w.fa, nullptr, w.fh, P * sz, F, j);
        poly_ntt(ln, w.fa, w.fa, j, sz, 2 * P, sz, sz, 1);
        h = w.fa + sz / 2;   // H of child u: the upper half of its product
        hs = sz;
    }
    PolyHornerArgs ha;
    memset(&ha, 0, sizeof ha);
    ha.m = w.lev[s.b]; ha.h = h; ha.h_stride = hs; ha.pts = w.pts; ha.out = values; ha.n = n; ha.b = s.b; ha.F = F;
    ln.horner(ha, N >> s.b);
}

// Z' at the points, c_i = v_i / Z'(d_i), numerators up the tree: the interpolant ends in w.num (n coefficients).
// Returns SMI_ERR_NO_INVERSE for a repeated point.
template <class Ln> inline int poly_tree_interp(Ln &ln, const PolyShape &s, const PolyWs &w, const Fp &F) {
    const uint64_t N = 1ull << s.k, n = s.n;
    poly_ew_run(ln, PEW_SET_FIRST, w.flag, nullptr, nullptr, 1, F);
    poly_ew_run(ln, PEW_DERIV, w.zp, w.lev[s.k], nullptr, n, F);
    poly_tree_eval(ln, s, w, w.zp, n, w.zv, F);
    poly_ew_run(ln, PEW_DIV, w.cw, w.zv, w.coef, n, F, 0, 0, 0, 0, w.flag);
    PolyBlockArgs ba;
    memset(&ba, 0, sizeof ba);
    ba.pts = w.pts; ba.c = w.cw; ba.n_out = w.num; ba.n = n; ba.b = s.b; ba.F = F;
    ln.block(ba, N >> s.b);
    for (uint32_t j = s.b + 1; j <= s.k; j++) {
        const uint64_t P = N >> j, cw = (1ull << (j - 1)) + 1, h = 1ull << j;
        poly_ntt(ln, w.lev[j - 1], w.fa, j, cw, 2 * P, cw, h, 0);
        poly_ntt(ln, w.num, w.fb, j, h / 2, 2 * P, h / 2, h, 0);
        poly_ew_run(ln, PEW_CROSS_SUM, w.fb, w.fa, nullptr, P * h, F, j);
        poly_ntt(ln, w.fb, w.num, j, h, P, 2 * h, h, 1);
    }
    if (ln.rc != SMI_OK) return ln.rc;
    return ln.read_word(w.flag) ? SMI_ERR_NO_INVERSE : ln.rc;
}
