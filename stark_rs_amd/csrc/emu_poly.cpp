// emu_poly.cpp -- CPU emulator of the subproduct-tree entry points (TEST INFRASTRUCTURE).
//
// emu_poly_* run the driver of poly_tree.h -- the very sequence of transforms and launches smi_poly_zerofier,
// smi_poly_eval_points and smi_poly_interpolate_points enqueue -- with emu_ntt for the transforms and the kernels'
// per-thread bodies (poly_core.h) one "thread" at a time, phase by phase, in host memory.  Same arguments and statuses
// as the C ABI, with (p, g) in place of a context.
#include <vector>

#include "poly_tree.h"
#include "tables.h"

extern "C" int emu_ntt(uint64_t p, uint64_t g, const uint32_t *in, uint32_t *out, uint32_t L, uint32_t n_in, uint32_t batch,
                       uint64_t in_stride, uint64_t out_stride, int inverse, uint64_t offset, uint64_t post_scale);

namespace {

struct EmuPolyLauncher {
    uint64_t p, g;
    int rc = SMI_OK;
    void ntt(const uint32_t *in, uint32_t *out, uint32_t L, uint64_t n_in, uint32_t batch, uint64_t in_stride, uint64_t out_stride,
             int inverse) {
        if (rc != SMI_OK) return;
        if (emu_ntt(p, g, in, out, L, (uint32_t)n_in, batch, in_stride, out_stride, inverse, 1, 1) != 0) rc = SMI_ERR_BAD_ARG;
    }
    template <int OP> static void ew_all(const PolyEw &a) {
        for (uint64_t i = 0; i < a.n; i++) poly_ew<OP>(a, i);
    }
    void ew(int op, const PolyEw &a) {
        if (rc != SMI_OK) return;
        switch (op) {
#define C(OP) case OP: ew_all<OP>(a); break;
            C(PEW_PAIR_MUL) C(PEW_TREE_FIX) C(PEW_CROSS) C(PEW_CROSS_SUM) C(PEW_DERIV) C(PEW_DIV) C(PEW_REV) C(PEW_ROOT_H)
            C(PEW_TWO_MINUS) C(PEW_SET_FIRST) C(PEW_MUL) C(PEW_COPY_TRUNC)
#undef C
        default: rc = SMI_ERR_BAD_ARG;
        }
    }
    // poly_block_kernel: LDS ping-pong between the levels, a barrier after every phase
    void block(const PolyBlockArgs &a, uint64_t blocks) {
        if (rc != SMI_OK) return;
        std::vector<uint32_t> m[2] = {std::vector<uint32_t>(SMI_POLY_MSLOT), std::vector<uint32_t>(SMI_POLY_MSLOT)};
        std::vector<uint32_t> nm[2] = {std::vector<uint32_t>(SMI_POLY_BLOCK), std::vector<uint32_t>(SMI_POLY_BLOCK)};
        const bool num = a.c != nullptr;
        for (uint64_t blk = 0; blk < blocks; blk++) {
            for (uint32_t tid = 0; tid < SMI_POLY_THREADS; tid++) PolyBlock::load(a, (uint32_t)blk, m[0].data(), num ? nm[0].data() : nullptr, tid);
            for (uint32_t s = 0; s < a.b; s++)
                for (uint32_t tid = 0; tid < SMI_POLY_THREADS; tid++)
                    PolyBlock::step(a, s, m[s & 1].data(), m[(s + 1) & 1].data(), num ? nm[s & 1].data() : nullptr, nm[(s + 1) & 1].data(), tid);
            for (uint32_t tid = 0; tid < SMI_POLY_THREADS; tid++)
                PolyBlock::store(a, (uint32_t)blk, m[a.b & 1].data(), num ? nm[a.b & 1].data() : nullptr, tid);
        }
    }
    void horner(const PolyHornerArgs &a, uint64_t blocks) {
        if (rc != SMI_OK) return;
        std::vector<uint32_t> m(SMI_POLY_BLOCK + 1), h(SMI_POLY_BLOCK), r(SMI_POLY_BLOCK);
        for (uint64_t blk = 0; blk < blocks; blk++) {
            for (uint32_t tid = 0; tid < SMI_POLY_THREADS; tid++) PolyHorner::load(a, (uint32_t)blk, m.data(), h.data(), tid);
            for (uint32_t tid = 0; tid < SMI_POLY_THREADS; tid++) PolyHorner::residue(a, m.data(), h.data(), r.data(), tid);
            for (uint32_t tid = 0; tid < SMI_POLY_THREADS; tid++) PolyHorner::eval(a, (uint32_t)blk, r.data(), tid);
        }
    }
    uint32_t read_word(const uint32_t *q) { return *q; }
};

// host_to_dev_u32 with reduce = 0: canonical values only
bool narrow(const uint64_t *in, size_t n, uint32_t p, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        if (in[i] >= p) return false;
        out[i] = (uint32_t)in[i];
    }
    return true;
}

}  // namespace

extern "C" int emu_poly_zerofier(uint64_t p, uint64_t g, const uint64_t *domain, size_t n, uint64_t *coeffs) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (n == 0) return SMI_ERR_EMPTY_DOMAIN;
    PolyShape s;
    const int st = poly_shape(n, 0, false, false, fs.K, &s);
    if (st != SMI_OK) return st;
    PolyWs w;
    std::vector<uint32_t> ws(w.carve(nullptr, s));
    w.carve(ws.data(), s);
    if (!narrow(domain, n, fs.F.p, w.pts)) return SMI_ERR_NON_CANONICAL;
    EmuPolyLauncher ln{p, g};
    poly_tree_build(ln, s, w, fs.F);
    if (ln.rc != SMI_OK) return ln.rc;
    for (size_t i = 0; i <= n; i++) coeffs[i] = w.lev[s.k][i];
    return SMI_OK;
}

extern "C" int emu_poly_eval_points(uint64_t p, uint64_t g, const uint64_t *coeffs, size_t n_coeffs, const uint64_t *points, size_t n_points,
                                    uint64_t *values) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    std::vector<uint32_t> chk(n_coeffs > n_points ? n_coeffs : n_points);
    if (!narrow(coeffs, n_coeffs, fs.F.p, chk.data()) || !narrow(points, n_points, fs.F.p, chk.data())) return SMI_ERR_NON_CANONICAL;
    if (n_points == 0) return SMI_OK;
    if (n_coeffs == 0) {   // the empty polynomial is 0 everywhere (src/univariate/eval.rs:6-14)
        for (size_t i = 0; i < n_points; i++) values[i] = 0;
        return SMI_OK;
    }
    PolyShape s;
    const int st = poly_shape(n_points, n_coeffs, true, false, fs.K, &s);
    if (st != SMI_OK) return st;
    PolyWs w;
    std::vector<uint32_t> ws(w.carve(nullptr, s));
    w.carve(ws.data(), s);
    narrow(points, n_points, fs.F.p, w.pts);
    narrow(coeffs, n_coeffs, fs.F.p, w.coef);
    EmuPolyLauncher ln{p, g};
    poly_tree_build(ln, s, w, fs.F);
    poly_tree_eval(ln, s, w, w.coef, n_coeffs, w.vals, fs.F);
    if (ln.rc != SMI_OK) return ln.rc;
    for (size_t i = 0; i < n_points; i++) values[i] = w.vals[i];
    return SMI_OK;
}

extern "C" int emu_poly_interpolate_points(uint64_t p, uint64_t g, const uint64_t *domain, const uint64_t *values, size_t n, uint64_t *coeffs) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (n == 0) return SMI_ERR_EMPTY_DOMAIN;
    PolyShape s;
    const int st = poly_shape(n, n, false, true, fs.K, &s);
    if (st != SMI_OK) return st;
    PolyWs w;
    std::vector<uint32_t> ws(w.carve(nullptr, s));
    w.carve(ws.data(), s);
    if (!narrow(domain, n, fs.F.p, w.pts) || !narrow(values, n, fs.F.p, w.coef)) return SMI_ERR_NON_CANONICAL;
    EmuPolyLauncher ln{p, g};
    poly_tree_build(ln, s, w, fs.F);
    const int rc = poly_tree_interp(ln, s, w, fs.F);
    if (rc != SMI_OK) return rc;
    for (size_t i = 0; i < n; i++) coeffs[i] = w.num[i];
    return SMI_OK;
}
