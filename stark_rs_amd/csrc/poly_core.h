// poly_core.h -- per-thread bodies of the subproduct-tree kernels (poly.hip) and of their CPU emulation (emu_poly.cpp).
//
// The tree over n points (leaves padded to N = 2^k with the constant 1) stores level j as N >> j nodes of 2^j + 1
// coefficients each (a node's degree is at most 2^j; full nodes are monic of degree exactly 2^j).  The bottom levels,
// up to blocks of 2^b <= SMI_POLY_BLOCK leaves, are built in LDS by schoolbook doubling (PolyBlock); the levels above
// by batched NTT products (poly_tree.h).  At the blocks, PolyHorner turns a block's scaled remainder into its
// residue and evaluates it at the block's points.
#pragma once
#include "field.h"

#define SMI_POLY_BLOCK_LOG 8
#define SMI_POLY_BLOCK (1u << SMI_POLY_BLOCK_LOG)   // leaves per LDS block
#define SMI_POLY_THREADS 256                        // threads of the block kernels
#define SMI_POLY_MSLOT (2 * SMI_POLY_BLOCK + 2)     // words of one level of products in LDS: B + (B >> s) <= 2B

// ---- elementwise ops (poly_ew_kernel<OP>): one output element per index i < n
enum {
    PEW_PAIR_MUL = 0,   // a[2c][e] *= a[2c+1][e]               (rows of 2^s0; i = c * 2^s0 + e)
    PEW_TREE_FIX,       // node c of the level above: t = a[2c][2^s0] * a[2c+1][2^s0]; out[c][0] -= t; out[c][2^(s0+1)] = t
    PEW_CROSS,          // (a[2c][e], a[2c+1][e]) <- (a[2c+1][e] * b[c][e], a[2c][e] * b[c][e])
    PEW_CROSS_SUM,      // out[2c][e] <- out[2c][e] * a[2c+1][e] + out[2c+1][e] * a[2c][e]
    PEW_DERIV,          // out[i] = (i + 1) * a[i + 1]
    PEW_DIV,            // out[i] = b[i] / a[i]; a[i] == 0 sets *flag
    PEW_REV,            // out[i] = a[s0 - i] when i <= s0 and s0 - i < s1, else 0
    PEW_ROOT_H,         // out[i] = a[s0 - 1 - i + s2 - s1] when s0 - 1 - i < s1, else 0
    PEW_TWO_MINUS,      // out[i] = (i == 0 ? 2 : 0) - out[i]
    PEW_SET_FIRST,      // out[i] = i == 0 ? v : 0
    PEW_MUL,            // out[i] *= a[i]
    PEW_COPY_TRUNC,     // out[i] = i < s0 ? a[i] : 0
    PEW_COUNT
};

struct PolyEw {
    uint32_t *out;
    const uint32_t *a, *b;
    uint32_t *flag;
    uint64_t n;          // indices
    uint64_t s0, s1, s2;
    uint32_t v;
    Fp F;
};

SMI_HD uint32_t pmul(uint32_t x, uint32_t y, const Fp &F) { return mont_mul(to_mont(x, F), y, F); }   // plain * plain

template <int OP> SMI_HD void poly_ew(const PolyEw &a, uint64_t i) {
    const Fp &F = a.F;
    if (OP == PEW_PAIR_MUL || OP == PEW_CROSS || OP == PEW_CROSS_SUM) {
        const uint64_t w = 1ull << a.s0, c = i >> a.s0, e = i & (w - 1), l = (2 * c) * w + e, r = l + w;
        if (OP == PEW_PAIR_MUL) a.out[l] = pmul(a.out[l], a.out[r], F);
        if (OP == PEW_CROSS) {
            const uint32_t x = to_mont(a.b[c * w + e], F), vl = a.out[l], vr = a.out[r];
            a.out[l] = mont_mul(vr, x, F);
            a.out[r] = mont_mul(vl, x, F);
        }
        if (OP == PEW_CROSS_SUM) a.out[l] = fp_add(pmul(a.out[l], a.a[r], F), pmul(a.out[r], a.a[l], F), F.p);
    } else if (OP == PEW_TREE_FIX) {
        const uint64_t cw = (1ull << a.s0) + 1, pw = (2ull << a.s0) + 1;
        const uint32_t t = pmul(a.a[(2 * i) * cw + cw - 1], a.a[(2 * i + 1) * cw + cw - 1], F);
        a.out[i * pw] = fp_sub(a.out[i * pw], t, F.p);
        a.out[i * pw + pw - 1] = t;
    } else if (OP == PEW_DERIV) {
        a.out[i] = pmul((uint32_t)(i + 1), a.a[i + 1], F);   // i + 1 <= 2^27 < p
    } else if (OP == PEW_DIV) {
        const uint32_t z = a.a[i];
        if (z == 0) {
            *a.flag = 1u;
            a.out[i] = 0;
        } else {
            const uint32_t zi = mont_pow(to_mont(z, F), F.p - 2, F);   // z^-1 (Montgomery form)
            a.out[i] = mont_mul(a.b[i], zi, F);
        }
    } else if (OP == PEW_REV) {
        a.out[i] = (i <= a.s0 && a.s0 - i < a.s1) ? a.a[a.s0 - i] : 0u;
    } else if (OP == PEW_ROOT_H) {
        const uint64_t t = a.s0 - 1 - i;
        a.out[i] = t < a.s1 ? a.a[t + a.s2 - a.s1] : 0u;
    } else if (OP == PEW_TWO_MINUS) {
        a.out[i] = fp_sub(i == 0 ? 2u % F.p : 0u, a.out[i], F.p);
    } else if (OP == PEW_SET_FIRST) {
        a.out[i] = i == 0 ? a.v : 0u;
    } else if (OP == PEW_MUL) {
        a.out[i] = pmul(a.out[i], a.a[i], F);
    } else if (OP == PEW_COPY_TRUNC) {
        a.out[i] = i < a.s0 ? a.a[i] : 0u;
    }
}

// ---- the bottom of the product tree, one block of 2^b leaves per workgroup.  Level s of the block is held in LDS as
// 2^(b-s) nodes of 2^s + 1 coefficients (Montgomery form), numerators (interpolation) as 2^(b-s) nodes of 2^s.
// Leaf l of block blk is point blk * 2^b + l: (x - d) for a point, the constant 1 for padding (numerator c_l, or 0).
struct PolyBlockArgs {
    const uint32_t *pts;   // n points
    const uint32_t *c;     // interpolation weights (n), or nullptr: products only
    uint32_t *m_out;       // level b: nodes of 2^b + 1 coefficients, or nullptr
    uint32_t *n_out;       // level b numerators: nodes of 2^b coefficients (c != nullptr)
    uint64_t n;
    uint32_t b;
    Fp F;
};
struct PolyBlock {
    static SMI_HD void load(const PolyBlockArgs &a, uint32_t blk, uint32_t *m, uint32_t *nm, uint32_t tid) {
        const uint32_t B = 1u << a.b;
        for (uint32_t l = tid; l < B; l += SMI_POLY_THREADS) {
            const uint64_t idx = (uint64_t)blk * B + l;
            const bool real = idx < a.n;
            m[2 * l] = real ? to_mont(fp_neg(a.pts[idx], a.F.p), a.F) : a.F.r1;
            m[2 * l + 1] = real ? a.F.r1 : 0u;
            if (nm) nm[l] = real ? to_mont(a.c[idx], a.F) : 0u;
        }
    }
    // level s (m0, n0) -> level s + 1 (m1, n1): each output coefficient is one thread's schoolbook sum
    static SMI_HD void step(const PolyBlockArgs &a, uint32_t s, const uint32_t *m0, uint32_t *m1, const uint32_t *n0, uint32_t *n1,
                            uint32_t tid) {
        const Fp &F = a.F;
        const uint32_t h = 1u << s, cw = h + 1, pw = 2 * h + 1, nodes = (1u << a.b) >> (s + 1);
        for (uint32_t o = tid; o < nodes * pw; o += SMI_POLY_THREADS) {
            const uint32_t q = o / pw, e = o - q * pw;
            const uint32_t *L = m0 + (2 * q) * cw, *R = L + cw;
            const uint32_t lo = e > h ? e - h : 0u, hi = e < h ? e : h;
            uint32_t acc = 0;
            for (uint32_t i = lo; i <= hi; i++) acc = fp_add(acc, mont_mul(L[i], R[e - i], F), F.p);
            m1[q * pw + e] = acc;
            if (n0 && e < 2 * h) {   // N_l * M_r + N_r * M_l: numerator i of degree < h, products of degree <= h
                const uint32_t *NL = n0 + (2 * q) * h, *NR = NL + h;
                const uint32_t nhi = e < h - 1 ? e : h - 1;
                uint32_t acn = 0;
                for (uint32_t i = lo; i <= nhi; i++) {
                    acn = fp_add(acn, mont_mul(NL[i], R[e - i], F), F.p);
                    acn = fp_add(acn, mont_mul(NR[i], L[e - i], F), F.p);
                }
                n1[q * 2 * h + e] = acn;
            }
        }
    }
    static SMI_HD void store(const PolyBlockArgs &a, uint32_t blk, const uint32_t *m, const uint32_t *nm, uint32_t tid) {
        const uint32_t B = 1u << a.b;
        if (a.m_out)
            for (uint32_t e = tid; e <= B; e += SMI_POLY_THREADS) a.m_out[(uint64_t)blk * (B + 1) + e] = from_mont(m[e], a.F);
        if (nm)
            for (uint32_t e = tid; e < B; e += SMI_POLY_THREADS) a.n_out[(uint64_t)blk * B + e] = from_mont(nm[e], a.F);
    }
};

// ---- evaluation at the blocks.  The descent (poly_tree.h) leaves, per block u, H_u[t] = g_{B-1-t} where
// (f mod M_u) / M_u = sum_{i>=1} g_{i-1} x^-i; the residue is the polynomial part of M_u * that series,
// r[e] = sum_{i=1}^{B-e} M_u[e+i] H_u[B-i], and each lane evaluates r at its point by Horner.
struct PolyHornerArgs {
    const uint32_t *m;     // level b: nodes of 2^b + 1 coefficients
    const uint32_t *h;     // block u's H at h + u * h_stride (2^b values)
    uint64_t h_stride;
    const uint32_t *pts;
    uint32_t *out;
    uint64_t n;
    uint32_t b;
    Fp F;
};
struct PolyHorner {
    static SMI_HD void load(const PolyHornerArgs &a, uint32_t blk, uint32_t *m, uint32_t *h, uint32_t tid) {
        const uint32_t B = 1u << a.b;
        for (uint32_t e = tid; e <= B; e += SMI_POLY_THREADS) m[e] = to_mont(a.m[(uint64_t)blk * (B + 1) + e], a.F);
        for (uint32_t e = tid; e < B; e += SMI_POLY_THREADS) h[e] = a.h[(uint64_t)blk * a.h_stride + e];
    }
    static SMI_HD void residue(const PolyHornerArgs &a, const uint32_t *m, const uint32_t *h, uint32_t *r, uint32_t tid) {
        const uint32_t B = 1u << a.b;
        for (uint32_t e = tid; e < B; e += SMI_POLY_THREADS) {
            uint32_t acc = 0;
            for (uint32_t i = 1; i <= B - e; i++) acc = fp_add(acc, mont_mul(m[e + i], h[B - i], a.F), a.F.p);
            r[e] = acc;
        }
    }
    static SMI_HD void eval(const PolyHornerArgs &a, uint32_t blk, const uint32_t *r, uint32_t tid) {
        const uint32_t B = 1u << a.b;
        for (uint32_t l = tid; l < B; l += SMI_POLY_THREADS) {
            const uint64_t idx = (uint64_t)blk * B + l;
            if (idx >= a.n) continue;
            const uint32_t x = to_mont(a.pts[idx], a.F);
            uint32_t acc = 0;
            for (uint32_t e = B; e-- > 0;) acc = fp_add(mont_mul(acc, x, a.F), r[e], a.F.p);
            a.out[idx] = acc;
        }
    }
};
