// poly.hip -- subproduct trees on the device: Polynomial::zerofier, eval_domain and interpolate_domain on arbitrary
// points (smi_poly_zerofier / smi_poly_eval_points / smi_poly_interpolate_points), and the Newton power-series inverse
// smi_poly_div shares with them.  The sequence of launches is poly_tree.h's; the kernels' bodies are poly_core.h's.
#include "internal.h"
#include "poly_tree.h"

template <int OP> __global__ void __launch_bounds__(256) poly_ew_kernel(PolyEw a) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (; i < a.n; i += step) poly_ew<OP>(a, i);
}

// one block of 2^b leaves per workgroup: the products (and with NUM the interpolation numerators) level by level in LDS
template <bool NUM> __global__ void __launch_bounds__(SMI_POLY_THREADS) poly_block_kernel(PolyBlockArgs a) {
    __shared__ uint32_t m[2][SMI_POLY_MSLOT];
    __shared__ uint32_t nm[2][NUM ? SMI_POLY_BLOCK : 1];
    const uint32_t tid = threadIdx.x, blk = blockIdx.x;
    PolyBlock::load(a, blk, m[0], NUM ? nm[0] : nullptr, tid);
    __syncthreads();
    for (uint32_t s = 0; s < a.b; s++) {
        PolyBlock::step(a, s, m[s & 1], m[(s + 1) & 1], NUM ? nm[s & 1] : nullptr, nm[(s + 1) & 1], tid);
        __syncthreads();
    }
    PolyBlock::store(a, blk, m[a.b & 1], NUM ? nm[a.b & 1] : nullptr, tid);
}

// one block of 2^b points per workgroup: its residue from the scaled remainder, then Horner per lane
__global__ void __launch_bounds__(SMI_POLY_THREADS) poly_horner_kernel(PolyHornerArgs a) {
    __shared__ uint32_t m[SMI_POLY_BLOCK + 1], h[SMI_POLY_BLOCK], r[SMI_POLY_BLOCK];
    const uint32_t tid = threadIdx.x, blk = blockIdx.x;
    PolyHorner::load(a, blk, m, h, tid);
    __syncthreads();
    PolyHorner::residue(a, m, h, r, tid);
    __syncthreads();
    PolyHorner::eval(a, blk, r, tid);
}

namespace {
struct HipPolyLauncher {
    smi_ctx *ctx;
    int rc = SMI_OK;
    void note(const char *what) {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess && rc == SMI_OK) rc = smi_hip_fail(ctx, e, what);
    }
    void ntt(const uint32_t *in, uint32_t *out, uint32_t L, uint64_t n_in, uint32_t batch, uint64_t in_stride, uint64_t out_stride,
             int inverse) {
        if (rc == SMI_OK) rc = dev_ntt(ctx, in, out, L, n_in, batch, in_stride, out_stride, inverse, 1, 1);
    }
    void ew(int op, const PolyEw &a) {
        if (rc != SMI_OK) return;
        uint64_t grid = (a.n + 255) / 256;
        if (grid > 4096) grid = 4096;
        const double bytes = 8.0 * (double)a.n;
        switch (op) {
#define C(OP, NAME)                                                                      \
    case OP: {                                                                           \
        ProfScope ps(ctx, "poly_ew_kernel<" NAME ">", bytes);                            \
        poly_ew_kernel<OP><<<(uint32_t)grid, 256, 0, ctx->stream>>>(a);                  \
        break;                                                                           \
    }
            C(PEW_PAIR_MUL, "pair_mul") C(PEW_TREE_FIX, "tree_fix") C(PEW_CROSS, "cross") C(PEW_CROSS_SUM, "cross_sum")
            C(PEW_DERIV, "deriv") C(PEW_DIV, "div") C(PEW_REV, "rev") C(PEW_ROOT_H, "root_h") C(PEW_TWO_MINUS, "two_minus")
            C(PEW_SET_FIRST, "set_first") C(PEW_MUL, "mul") C(PEW_COPY_TRUNC, "copy_trunc")
#undef C
        default: rc = smi_fail(ctx, SMI_ERR_BAD_ARG, "poly: unknown elementwise op"); return;
        }
        note("poly_ew_kernel launch");
    }
    void block(const PolyBlockArgs &a, uint64_t blocks) {
        if (rc != SMI_OK) return;
        const double bytes = 4.0 * (double)blocks * ((1u << a.b) * (a.c ? 3 : 2) + 1);
        if (a.c) {
            ProfScope ps(ctx, "poly_block_kernel<num>", bytes);
            poly_block_kernel<true><<<(uint32_t)blocks, SMI_POLY_THREADS, 0, ctx->stream>>>(a);
        } else {
            ProfScope ps(ctx, "poly_block_kernel<prod>", bytes);
            poly_block_kernel<false><<<(uint32_t)blocks, SMI_POLY_THREADS, 0, ctx->stream>>>(a);
        }
        note("poly_block_kernel launch");
    }
    void horner(const PolyHornerArgs &a, uint64_t blocks) {
        if (rc != SMI_OK) return;
        ProfScope ps(ctx, "poly_horner_kernel", 4.0 * (double)blocks * ((4u << a.b) + 1));
        poly_horner_kernel<<<(uint32_t)blocks, SMI_POLY_THREADS, 0, ctx->stream>>>(a);
        note("poly_horner_kernel launch");
    }
    uint32_t read_word(const uint32_t *q) {
        uint32_t v = 0;
        if (rc != SMI_OK) return 0;
        hipError_t e = hipMemcpyAsync(&v, q, 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = smi_hip_fail(ctx, e, "poly: flag read-back");
        return v;
    }
};

// the call's buffers, carved from one context staging buffer (grows, never shrinks)
int poly_ws(smi_ctx *ctx, const PolyShape &s, PolyWs *w) {
    void *base;
    SMI_TRY(ctx_tmp(ctx, 3, w->carve(nullptr, s) * 4, &base));
    w->carve((uint32_t *)base, s);
    return SMI_OK;
}
int poly_size_fail(smi_ctx *ctx, int st) {
    return smi_fail(ctx, st, st == SMI_ERR_ROOT_TOO_LARGE ? "too many points for the transforms of this modulus (include/stark_mi.h)" : nullptr);
}
}  // namespace

// g = rb^-1 mod x^k (rb[0] = 1 / g0): smi_poly_div's quotient and the evaluation tree's root run the same iteration
int dev_series_inv(smi_ctx *ctx, const uint32_t *rb, size_t k, uint32_t g0, uint32_t *g, uint32_t *e, uint32_t *f1, uint32_t *f2) {
    HipPolyLauncher ln{ctx};
    poly_series_inv(ln, rb, k, g0, g, e, f1, f2, ctx->fs.F);
    return ln.rc;
}

int smi_poly_zerofier(smi_ctx *ctx, const uint64_t *domain, size_t n, uint64_t *coeffs) {
    if (!ctx || (n && (!domain || !coeffs))) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (n == 0) return smi_fail(ctx, SMI_ERR_EMPTY_DOMAIN, nullptr);   // the reference indexes domain[0] (mod.rs:78)
    PolyShape s;
    const int st = poly_shape(n, 0, false, false, ctx->fs.K, &s);
    if (st != SMI_OK) return poly_size_fail(ctx, st);
    PolyWs w;
    SMI_TRY(poly_ws(ctx, s, &w));
    SMI_TRY(host_to_dev_u32(ctx, domain, n, w.pts, 0));
    HipPolyLauncher ln{ctx};
    poly_tree_build(ln, s, w, ctx->fs.F);
    SMI_TRY(ln.rc);
    return dev_u32_to_host(ctx, w.lev[s.k], n + 1, coeffs);
}

int smi_poly_eval_points(smi_ctx *ctx, const uint64_t *coeffs, size_t n_coeffs, const uint64_t *points, size_t n_points, uint64_t *values) {
    if (!ctx || (n_coeffs && !coeffs) || (n_points && (!points || !values))) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (!n_points || !n_coeffs) {   // no tree: check the inputs; the empty polynomial is 0 everywhere (eval.rs:6-14)
        void *chk;
        SMI_TRY(ctx_tmp(ctx, 3, (n_coeffs > n_points ? n_coeffs : n_points) * 4 + 4, &chk));
        SMI_TRY(host_to_dev_u32(ctx, coeffs, n_coeffs, (uint32_t *)chk, 0));
        SMI_TRY(host_to_dev_u32(ctx, points, n_points, (uint32_t *)chk, 0));
        for (size_t i = 0; i < n_points; i++) values[i] = 0;
        return SMI_OK;
    }
    PolyShape s;
    const int st = poly_shape(n_points, n_coeffs, true, false, ctx->fs.K, &s);
    if (st != SMI_OK) return poly_size_fail(ctx, st);
    PolyWs w;
    SMI_TRY(poly_ws(ctx, s, &w));
    SMI_TRY(host_to_dev_u32(ctx, points, n_points, w.pts, 0));
    SMI_TRY(host_to_dev_u32(ctx, coeffs, n_coeffs, w.coef, 0));
    HipPolyLauncher ln{ctx};
    poly_tree_build(ln, s, w, ctx->fs.F);
    poly_tree_eval(ln, s, w, w.coef, n_coeffs, w.vals, ctx->fs.F);
    SMI_TRY(ln.rc);
    return dev_u32_to_host(ctx, w.vals, n_points, values);
}

int smi_poly_interpolate_points(smi_ctx *ctx, const uint64_t *domain, const uint64_t *values, size_t n, uint64_t *coeffs) {
    if (!ctx || (n && (!domain || !values || !coeffs))) return SMI_ERR_BAD_ARG;
    DeviceGuard dg__(ctx);
    if (n == 0) return smi_fail(ctx, SMI_ERR_EMPTY_DOMAIN, nullptr);   // interpolate.rs:11
    PolyShape s;
    const int st = poly_shape(n, n, false, true, ctx->fs.K, &s);
    if (st != SMI_OK) return poly_size_fail(ctx, st);
    PolyWs w;
    SMI_TRY(poly_ws(ctx, s, &w));
    SMI_TRY(host_to_dev_u32(ctx, domain, n, w.pts, 0));
    SMI_TRY(host_to_dev_u32(ctx, values, n, w.coef, 0));
    HipPolyLauncher ln{ctx};
    poly_tree_build(ln, s, w, ctx->fs.F);
    const int rc = poly_tree_interp(ln, s, w, ctx->fs.F);
    if (rc == SMI_ERR_NO_INVERSE) return smi_fail(ctx, rc, "no inverse");   // a repeated point: field.inv(0), interpolate.rs:34
    SMI_TRY(rc);
    return dev_u32_to_host(ctx, w.num, n, coeffs);
}
