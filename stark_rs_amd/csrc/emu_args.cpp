// emu_args.cpp -- CPU emulator of the argument list's kernels (TEST INFRASTRUCTURE).
//
// emu_args_columns runs the three launches of smi_dev_args_columns over args_core.h's lane code for every lane, workgroup
// and argument, with the kernels' own lane batching and block split; emu_air_compose_args runs emu_air_compose_ext and then
// air_args_compose_kernel's grid-stride loop over args_compose_points; emu_args_transcript runs the transcript layout of
// the proof.  Same arguments and statuses as the C ABI, with (p, g) in place of a context.
#include <string.h>

#include <string>
#include <vector>

#include "args_core.h"
#include "tables.h"
#include "transcript_core.h"

extern "C" int emu_air_compose_ext(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const uint32_t *lde, uint64_t stride,
                                   const uint64_t *weights, uint32_t *out, uint64_t out_stride, int force_direct);

namespace {
void load4(const uint32_t *src, uint64_t at, uint64_t len, uint32_t v[4]) {
    for (int q = 0; q < 4; q++) v[q] = at + q < len ? src[at + q] : 0u;
}
void store4(uint32_t *dst, uint64_t at, uint64_t len, const uint32_t v[4]) {
    for (int q = 0; q < 4; q++)
        if (at + q < len) dst[at + q] = v[q];
}
// args_wg_scan of args.hip: v[tid] -> excl[tid] and the aggregate
Fq wg_scan(bool perm, const Fq *v, Fq *excl, uint32_t g_m, const Fp &F) {
    static thread_local uint32_t sc[2][4][PERM_BLOCK];
    for (uint32_t tid = 0; tid < PERM_BLOCK; tid++)
        for (int e = 0; e < 4; e++) sc[0][e][tid] = v[tid].c[e];
    int cur = 0;
    for (uint32_t off = 1; off < PERM_BLOCK; off <<= 1) {
        for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) args_scan_step(perm, sc[cur], sc[cur ^ 1], tid, off, g_m, F);
        cur ^= 1;
    }
    for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) excl[tid] = tid ? perm_scan_at(sc[cur], tid - 1) : args_identity(perm, F);
    return perm_scan_at(sc[cur], PERM_BLOCK - 1);
}
}  // namespace

// c: 4 A coordinate columns c_stride apart.  *closes: the mask; *key: the smallest 16 row + 2 a + side with a zero
// denominator, or ~0
extern "C" int emu_args_columns(uint64_t p, uint64_t g, const smi_air_args *args, const uint32_t *trace, uint32_t n_cols, uint32_t log_n,
                                const uint64_t *challenges, uint32_t *c, uint64_t c_stride, uint32_t *closes, uint64_t *key) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (!ext_field_ok(p, g, nullptr) || p >= (1ull << 30)) return SMI_ERR_BAD_ARG;
    if (!n_cols || n_cols > 64 || log_n < 1 || log_n > 27) return SMI_ERR_BAD_ARG;
    const int rc = args_validate(args, n_cols, nullptr);
    if (rc != SMI_OK) return rc;
    const Fp F = fs.F;
    const uint64_t n = 1ull << log_n, nb = (n + PERM_TILE - 1) / PERM_TILE;
    if (c_stride < n) return SMI_ERR_BAD_ARG;
    ArgsDev AD;
    args_build(F, (uint32_t)g, args, challenges, &AD);
    const uint32_t A = AD.A;
    std::vector<Fq> agg_all((size_t)A * nb), total(A);
    uint64_t first = ~0ull;
    std::vector<Fq> agg(PERM_BLOCK), pre(PERM_BLOCK), pls((size_t)PERM_BLOCK * PERM_ROWS);
    // args_block_kernel: grid (nb, A)
    for (uint32_t a = 0; a < A; a++) {
        const bool perm = AD.kind[a] == SMI_ARG_PERM;
        uint32_t *ca = c + 4 * (uint64_t)a * c_stride;
        for (uint64_t b = 0; b < nb; b++) {
            for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) {
                const uint64_t row0 = (b * PERM_BLOCK + tid) * PERM_ROWS;
                uint64_t k;
                args_lane_column(
                    AD, a, F, row0, n,
                    [&](uint32_t col, uint32_t v[4]) {
                        if (row0 < n) load4(trace + (uint64_t)col * n, row0, n, v);
                        else v[0] = v[1] = v[2] = v[3] = 0u;
                    },
                    &pls[(size_t)tid * PERM_ROWS], &agg[tid], &k);
                if (k < first) first = k;
            }
            agg_all[(size_t)a * nb + b] = wg_scan(perm, agg.data(), pre.data(), AD.g_m, F);
            for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) {
                const uint64_t row0 = (b * PERM_BLOCK + tid) * PERM_ROWS;
                if (row0 >= n) break;
                uint32_t o[4][PERM_ROWS];
                for (int q = 0; q < PERM_ROWS; q++) {
                    const Fq w = args_combine(perm, pls[(size_t)tid * PERM_ROWS + q], pre[tid], AD.g_m, F);
                    for (int e = 0; e < 4; e++) o[e][q] = w.c[e];
                }
                for (int e = 0; e < 4; e++) store4(ca + e * c_stride, row0, n, o[e]);
            }
        }
    }
    // args_scan_kernel: workgroup a, PERM_BLOCK aggregates at a time
    for (uint32_t a = 0; a < A; a++) {
        const bool perm = AD.kind[a] == SMI_ARG_PERM;
        Fq *bs = &agg_all[(size_t)a * nb];
        Fq carry = args_identity(perm, F);
        for (uint64_t base = 0; base < nb; base += PERM_BLOCK) {
            for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) agg[tid] = base + tid < nb ? bs[base + tid] : args_identity(perm, F);
            const Fq tile = wg_scan(perm, agg.data(), pre.data(), AD.g_m, F);
            for (uint32_t tid = 0; tid < PERM_BLOCK && base + tid < nb; tid++)
                bs[base + tid] = args_scan_out(perm, args_combine(perm, carry, pre[tid], AD.g_m, F), F);
            carry = args_combine(perm, carry, tile, AD.g_m, F);
        }
        total[a] = args_scan_out(perm, carry, F);
    }
    // args_propagate_kernel: grid (nb, A)
    for (uint32_t a = 0; a < A; a++) {
        uint32_t *ca = c + 4 * (uint64_t)a * c_stride;
        for (uint64_t b = 0; b < nb; b++)
            for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) {
                const uint64_t row0 = (b * PERM_BLOCK + tid) * PERM_ROWS;
                if (row0 >= n) break;
                uint32_t v[4][PERM_ROWS];
                for (int e = 0; e < 4; e++) load4(ca + e * c_stride, row0, n, v[e]);
                args_propagate_rows(AD.kind[a] == SMI_ARG_PERM, agg_all[(size_t)a * nb + b].c, v, AD.g_m, F);
                for (int e = 0; e < 4; e++) store4(ca + e * c_stride, row0, n, v[e]);
            }
    }
    if (key) *key = first;
    if (first != ~0ull) return SMI_ERR_NO_INVERSE;
    uint32_t mask = 0;
    for (uint32_t a = 0; a < A; a++) {
        const uint32_t *t = total[a].c;
        if (t[0] == (AD.kind[a] == SMI_ARG_PERM ? 1u : 0u) && !(t[1] | t[2] | t[3])) mask |= 1u << a;
    }
    if (closes) *closes = mask;
    return SMI_OK;
}

// grid: workgroups of the streaming launch (0: as the library sizes it for 256 compute units)
extern "C" int emu_air_compose_args(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_args *args, const uint32_t *lde,
                                    uint64_t stride, const uint32_t *cl, uint64_t c_stride, const uint64_t *challenges, const uint64_t *weights,
                                    uint32_t *out, uint64_t out_stride, int force_direct, uint32_t grid) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (!ext_field_ok(p, g, nullptr)) return SMI_ERR_BAD_ARG;
    std::string why;
    const int prc = args_plan(p, cfg, air, args, nullptr, nullptr, &why);
    if (prc != SMI_OK) return prc;
    const int rc = emu_air_compose_ext(p, g, cfg, air, lde, stride, weights, out, out_stride, force_direct);
    if (rc != SMI_OK) return rc;
    const uint32_t log_N = cfg->log_n + cfg->log_blowup;
    const Fp F = fs.F;
    AirHost H;
    air_build(F, host_powmod(fs.wmax[0], 1ull << (fs.K - log_N), F.p), cfg, air, &H);
    const AirDev &A = H.dev;
    if (c_stride < A.N) return SMI_ERR_BAD_ARG;
    ArgsDev AD;
    args_build(F, (uint32_t)g, args, challenges, &AD);
    const uint64_t *w = weights + 4 * (uint64_t)(A.W + A.K);
    const uint64_t groups = A.N / PERM_ROWS, want = (groups + PERM_BLOCK - 1) / PERM_BLOCK;
    if (!grid) grid = (uint32_t)(want < 2048 ? want : 2048);
    const uint64_t gstep = (uint64_t)grid * PERM_BLOCK;
    const uint32_t B = 1u << A.log_B, tau_m = air_to_m((uint32_t)cfg->trace_offset, F.p);
    const uint32_t xstep_m = mont_pow(A.omega_m, gstep * PERM_ROWS, F);
    for (uint64_t gid = 0; gid < gstep && gid < groups; gid++) {
        uint32_t x_m = mont_mul(A.h_m, mont_pow(A.omega_m, gid * PERM_ROWS, F), F);
        for (uint64_t gq = gid; gq < groups; gq += gstep) {
            const uint64_t i0 = gq * PERM_ROWS, i1 = (i0 + B) & (A.N - 1);
            uint32_t acc[4][PERM_ROWS];
            for (int e = 0; e < 4; e++) load4(out + e * out_stride, i0, A.N, acc[e]);
            args_compose_points(
                AD, F, w, tau_m, A.izt_m, B, i0, x_m, A.omega_m, [&](uint32_t col, uint32_t v[4]) { load4(lde + (uint64_t)col * stride, i0, A.N, v); },
                [&](uint32_t col, bool next, uint32_t v[4]) { load4(cl + (uint64_t)col * c_stride, next ? i1 : i0, A.N, v); }, acc);
            for (int e = 0; e < 4; e++) store4(out + e * out_stride, i0, A.N, acc[e]);
            x_m = mont_mul(x_m, xstep_m, F);
        }
    }
    return SMI_OK;
}

// the proof's transcript: the 8 challenges of root_1, the 4 (W + K + 2 A) weights of root_2 -> their count; seed: 16 words
// and the phase; *len: the transcript's length in bytes
extern "C" uint64_t emu_args_transcript(const uint8_t *roots, uint32_t W, uint32_t K, uint32_t A, uint64_t *challenges, uint32_t *seed, uint64_t *len) {
    Transcript T;
    std::vector<uint64_t> out;
    transcript_perm_challenges(T, roots, &out);
    transcript_args_weights(T, roots + 32, W, K, A, &out);
    memcpy(challenges, out.data(), 8 * out.size());
    const FsSeed z = T.seed();
    memcpy(seed, z.s, sizeof z.s);
    seed[16] = z.phase;
    if (len) *len = T.bytes.size();
    return out.size();
}
