// emu_air.cpp -- CPU emulator of the AIR entry points (TEST INFRASTRUCTURE).
//
// emu_air_compose runs air_compose_kernel's own structure in host memory: the tile choice of air_tile, the staging of
// T + B elements per column with the wrap at N, and the per-thread body air_tile_thread (air_core.h) one "thread" at a
// time; where the kernel takes air_direct_kernel the emulator runs air_direct_point.  emu_air_check evaluates the
// boundary points and the constraints with the kernels' air_constraint and keeps the first violation in the order the
// device's atomic minimum does.  Same arguments and statuses as the C ABI, with (p, g) in place of a context.
// The periodic tables are laid out by air_periodic_plan (air_core.h) and filled with the emulator's own transforms
// (emu_ntt: an inverse transform per group, then a forward one on the group's coset), not with anything of the GPU path.
// emu_air_row_open runs air_row_open_kernel's grid -- one workgroup of 64 lanes per (test, position) -- over the record
// writer both share (mgpu_core.h mg_row_open_write).
// emu_air_transcript runs the transcript layouts of transcript_core.h, the code provers and verifiers derive the weights and
// FRI's seed with.
// There is no emu_air_prove / emu_air_verify: the emulator has no single-device Fri::prove loop to continue a
// transcript with (emu_mgpu.cpp emulates the multi-GPU round loop only), and the verifier is host code already.
#include <string.h>

#include <string>
#include <vector>

#include "air_core.h"
#include "mgpu_core.h"
#include "tables.h"
#include "transcript_core.h"

extern "C" int emu_ntt(uint64_t p, uint64_t g, const uint32_t *in, uint32_t *out, uint32_t L, uint32_t n_in, uint32_t batch, uint64_t in_stride,
                       uint64_t out_stride, int inverse, uint64_t offset, uint64_t post_scale);

namespace {
// tbl_j[i] = pi_j(x_i), i < L_j, for every periodic column, at the places AirHost::per names
bool emu_periodic_tables(uint64_t p, uint64_t g, const AirPeriodic &P, std::vector<uint32_t> *tab) {
    tab->assign(P.table_words, 0);
    for (const AirPeriodGroup &gr : P.groups) {
        const uint64_t per = 1ull << gr.log_period, len = 1ull << gr.log_len;
        std::vector<uint32_t> coef(gr.count * per);
        if (emu_ntt(p, g, P.vals.data() + gr.in_off, coef.data(), gr.log_period, (uint32_t)per, gr.count, per, per, 1, 1, gr.lde_offset)) return false;
        if (emu_ntt(p, g, coef.data(), tab->data() + gr.out_off, gr.log_len, (uint32_t)per, gr.count, per, len, 0, 1, 1)) return false;
    }
    return true;
}

template <int P, bool WIN = false>
void emu_tiles(const AirDev &A, const Fp &F, const uint32_t *w_m, const uint32_t *cols, uint64_t stride, const AirTile &tl, uint32_t *out) {
    const uint32_t B = 1u << A.log_B, pitch = tl.T + (A.S - 1) * B;
    std::vector<uint32_t> tile((size_t)(A.W + A.Q) * pitch);
    const uint32_t step_m = mont_pow(A.omega_m, tl.threads, F);
    for (uint64_t base = 0; base < A.N; base += tl.T) {
        for (uint32_t c = 0; c < A.W; c++)
            for (uint32_t e = 0; e < pitch; e++) tile[(size_t)c * pitch + e] = cols[c * stride + ((base + e) & (A.N - 1))];
        for (uint32_t j = 0; j < A.Q; j++)
            for (uint32_t e = 0; e < pitch; e++) tile[(size_t)(A.W + j) * pitch + e] = A.ptab[A.pofs[j] + ((uint32_t)(base + e) & ((1u << A.plog[j]) - 1u))];
        const uint32_t xbase_m = mont_mul(A.h_m, mont_pow(A.omega_m, base, F), F);
        for (uint32_t tid = 0; tid < tl.threads; tid++) air_tile_thread<P, WIN>(A, F, w_m, tile.data(), tl.T, tl.threads, base, xbase_m, step_m, tid, out);
    }
}

template <int P, bool WIN = false>
void emu_tiles_ext(const AirDev &A, const Fp &F, const uint32_t *w_m, const uint32_t *cols, uint64_t stride, const AirTile &tl, uint32_t *out,
                   uint64_t out_stride) {
    const uint32_t B = 1u << A.log_B, pitch = tl.T + (A.S - 1) * B;
    std::vector<uint32_t> tile((size_t)(A.W + A.Q) * pitch);
    const uint32_t step_m = mont_pow(A.omega_m, tl.threads, F);
    for (uint64_t base = 0; base < A.N; base += tl.T) {
        for (uint32_t c = 0; c < A.W; c++)
            for (uint32_t e = 0; e < pitch; e++) tile[(size_t)c * pitch + e] = cols[c * stride + ((base + e) & (A.N - 1))];
        for (uint32_t j = 0; j < A.Q; j++)
            for (uint32_t e = 0; e < pitch; e++) tile[(size_t)(A.W + j) * pitch + e] = A.ptab[A.pofs[j] + ((uint32_t)(base + e) & ((1u << A.plog[j]) - 1u))];
        const uint32_t xbase_m = mont_mul(A.h_m, mont_pow(A.omega_m, base, F), F);
        for (uint32_t tid = 0; tid < tl.threads; tid++)
            air_tile_thread_ext<P, WIN>(A, F, w_m, tile.data(), tl.T, tl.threads, base, xbase_m, step_m, tid, out, out_stride);
    }
}
}  // namespace

extern "C" int emu_air_compose(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const uint32_t *lde, uint64_t stride,
                               const uint64_t *weights, uint32_t *out, int force_direct) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    std::string why;
    const int rc = air_validate(p, cfg, air, nullptr, nullptr, &why, false, false, SMI_AIR_MAX_WINDOW);
    if (rc != SMI_OK) return rc;
    const uint32_t log_N = cfg->log_n + cfg->log_blowup;
    if (log_N > fs.K) return SMI_ERR_UNSUPPORTED_PRIME;
    AirHost H;
    air_build(fs.F, host_powmod(fs.wmax[0], 1ull << (fs.K - log_N), fs.F.p), cfg, air, &H);
    std::vector<uint32_t> tab;
    if (!emu_periodic_tables(p, g, H.per, &tab)) return SMI_ERR_BAD_ARG;
    H.dev.ptab = tab.data();
    const AirDev &A = H.dev;
    if (stride < A.N) return SMI_ERR_BAD_ARG;
    std::vector<uint32_t> w_m(A.W + A.K);
    for (uint32_t i = 0; i < A.W + A.K; i++) w_m[i] = to_mont_u64(weights[i], fs.F);
    AirTile tl = air_tile(A.W + A.Q, 1ull << A.log_B, A.N, 1, A.S);
    if (force_direct || (stride & 3)) tl.T = 0;
    if (A.S > 2) {   // the WIN = true instantiations the launcher picks for a window
        if (!tl.T)
            for (uint64_t i = 0; i < A.N; i++) air_direct_point<true>(A, fs.F, w_m.data(), lde, stride, i, out);
        else if (tl.P == 4) emu_tiles<4, true>(A, fs.F, w_m.data(), lde, stride, tl, out);
        else if (tl.P == 2) emu_tiles<2, true>(A, fs.F, w_m.data(), lde, stride, tl, out);
        else emu_tiles<1, true>(A, fs.F, w_m.data(), lde, stride, tl, out);
        return SMI_OK;
    }
    if (!tl.T)
        for (uint64_t i = 0; i < A.N; i++) air_direct_point(A, fs.F, w_m.data(), lde, stride, i, out);
    else if (tl.P == 4) emu_tiles<4>(A, fs.F, w_m.data(), lde, stride, tl, out);
    else if (tl.P == 2) emu_tiles<2>(A, fs.F, w_m.data(), lde, stride, tl, out);
    else emu_tiles<1>(A, fs.F, w_m.data(), lde, stride, tl, out);
    return SMI_OK;
}

// air_compose_ext_kernel the same way: weights = 4 (W + K) unreduced u64 (coordinate e of weight j at 4 j + e), out =
// four coordinate columns out_stride apart
extern "C" int emu_air_compose_ext(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const uint32_t *lde, uint64_t stride,
                                   const uint64_t *weights, uint32_t *out, uint64_t out_stride, int force_direct) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    std::string why;
    const int rc = air_validate(p, cfg, air, nullptr, nullptr, &why, false, false, SMI_AIR_MAX_WINDOW);
    if (rc != SMI_OK) return rc;
    const uint32_t log_N = cfg->log_n + cfg->log_blowup;
    if (log_N > fs.K) return SMI_ERR_UNSUPPORTED_PRIME;
    AirHost H;
    air_build(fs.F, host_powmod(fs.wmax[0], 1ull << (fs.K - log_N), fs.F.p), cfg, air, &H);
    std::vector<uint32_t> tab;
    if (!emu_periodic_tables(p, g, H.per, &tab)) return SMI_ERR_BAD_ARG;
    H.dev.ptab = tab.data();
    const AirDev &A = H.dev;
    if (stride < A.N || out_stride < A.N) return SMI_ERR_BAD_ARG;
    std::vector<uint32_t> w_m(4 * AIR_MAX_WEIGHTS, 0);
    for (uint32_t i = 0; i < 4 * (A.W + A.K); i++) w_m[(i & 3) * AIR_MAX_WEIGHTS + (i >> 2)] = to_mont_u64(weights[i], fs.F);
    AirTile tl = air_tile(A.W + A.Q, 1ull << A.log_B, A.N, 4, A.S);
    if (force_direct || (stride & 3)) tl.T = 0;
    if (A.S > 2) {
        if (!tl.T)
            for (uint64_t i = 0; i < A.N; i++) air_direct_point_ext<true>(A, fs.F, w_m.data(), lde, stride, i, out, out_stride);
        else if (tl.P == 4) emu_tiles_ext<4, true>(A, fs.F, w_m.data(), lde, stride, tl, out, out_stride);
        else if (tl.P == 2) emu_tiles_ext<2, true>(A, fs.F, w_m.data(), lde, stride, tl, out, out_stride);
        else emu_tiles_ext<1, true>(A, fs.F, w_m.data(), lde, stride, tl, out, out_stride);
        return SMI_OK;
    }
    if (!tl.T)
        for (uint64_t i = 0; i < A.N; i++) air_direct_point_ext(A, fs.F, w_m.data(), lde, stride, i, out, out_stride);
    else if (tl.P == 4) emu_tiles_ext<4>(A, fs.F, w_m.data(), lde, stride, tl, out, out_stride);
    else if (tl.P == 2) emu_tiles_ext<2>(A, fs.F, w_m.data(), lde, stride, tl, out, out_stride);
    else emu_tiles_ext<1>(A, fs.F, w_m.data(), lde, stride, tl, out, out_stride);
    return SMI_OK;
}

extern "C" int emu_air_check(uint64_t p, const smi_air *air, uint32_t n_cols, uint32_t log_n, const uint32_t *trace, int *ok,
                             uint32_t *constraint, uint64_t *row) {
    smi_stark_cfg cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.n_cols = n_cols;
    cfg.log_n = log_n;
    std::string why;
    const int rc = air_validate(p, &cfg, air, nullptr, nullptr, &why, true, false, SMI_AIR_MAX_WINDOW);
    if (rc != SMI_OK) return rc;
    const Fp F = fp_make((uint32_t)p);
    AirHost H;
    air_build(F, 1, &cfg, air, &H, true);
    H.dev.ptab = H.per.vals.data();   // on the trace itself the tables are the values
    const uint64_t n = 1ull << log_n;
    uint64_t first = ~0ull;
    auto take = [&](uint64_t key) { if (key < first) first = key; };
    for (uint64_t i = 0; i < n || i < air->n_boundary; i++) {
        if (i < air->n_boundary && trace[air->boundary_col[i] * n + air->boundary_row[i]] != air->boundary_value[i])
            take((i << 32) | air->boundary_row[i]);
        if (i + H.dev.S <= n)
            for (uint32_t k = 0; k < H.dev.K; k++)
                if (air_constraint(H.dev, F, k, [&](uint32_t var) {
                        return air_mem_operand_win(H.dev, var, i, [&](uint32_t c, uint32_t s) { return trace[c * n + i + s]; });
                    })) {
                    take((1ull << 63) | ((uint64_t)k << 32) | i);
                    break;
                }
    }
    *ok = first == ~0ull;
    if (!*ok) {
        const uint32_t idx = (uint32_t)((first >> 32) & 0x7fffffffu);
        if (constraint) *constraint = (first >> 63) ? air->n_boundary + idx : idx;
        if (row) *row = first & 0xffffffffull;
    }
    return SMI_OK;
}

// air_row_open_kernel (air.hip): grid (t, R), 64 lanes; -> the bytes of the opening section
extern "C" uint64_t emu_air_row_open(const uint32_t *cols, uint64_t stride, uint32_t W, const uint8_t *nodes, uint64_t N, const uint64_t *top,
                                     uint32_t t, uint32_t R, uint64_t B, uint8_t *out) {
    uint32_t depth = 0;
    while ((1ull << depth) < N) depth++;
    for (uint32_t s = 0; s < t; s++)
        for (uint32_t k = 0; k < R; k++)
            for (uint32_t lane = 0; lane < 64; lane++) mg_row_open_write(cols, stride, W, nodes, depth, top[s], s, k, t, out, lane, 64, R, B);
    return mg_row_open_bytes(W, t, depth, R);
}

// coset_open_kernel (deep.hip): its grid -- one workgroup of 64 lanes per (test, group) -- over the writer both share
// (mgpu_core.h mg_coset_open_write).  Group k: V[k] columns at cols[k], stride[k] apart, under the tree nodes[k] of N / 4
// coset leaves; the sections follow each other in group order -> the bytes written
extern "C" uint64_t emu_coset_open(uint32_t G, const uint32_t *const *cols, const uint64_t *stride, const uint32_t *V, const uint8_t *const *nodes, uint64_t N,
                                   const uint64_t *top, uint32_t t, uint8_t *out) {
    uint32_t log_N = 0;
    while ((1ull << log_N) < N) log_N++;
    MgCosetTable tab;
    memset(&tab, 0, sizeof tab);
    uint64_t total = 0;
    for (uint32_t k = 0; k < G && k < 3; k++) {
        tab.g[k] = MgCosetGroup{cols[k], stride[k], nodes[k], total, V[k], 0};
        total += mg_coset_open_bytes(V[k], t, log_N);
    }
    for (uint32_t s = 0; s < t; s++)
        for (uint32_t k = 0; k < G && k < 3; k++)
            for (uint32_t lane = 0; lane < 64; lane++) mg_coset_open_write(tab.g[k], log_N, top[s], s, t, out + tab.g[k].out_at, lane, 64);
    return total;
}

// transcript_core.h: layout 0 column trees (roots = W roots), 1 one row tree, 2 the extension, 3 the permutation proof (roots =
// root_1, root_2; the 8 challenges, then the 4 (W + K + 2) weights) -> the number of challenges written; seed = the 16 words
// and the phase FRI continues
extern "C" uint64_t emu_air_transcript(int layout, const uint8_t *roots, uint32_t W, uint32_t K, uint64_t *challenges, uint32_t *seed) {
    Transcript T;
    std::vector<uint64_t> out;
    if (layout == 0) transcript_columns(T, roots, W, K, &out);
    else if (layout == 1) transcript_rows(T, roots, W, K, &out);
    else if (layout == 2) transcript_ext(T, roots, W, K, &out);
    else {
        transcript_perm_challenges(T, roots, &out);
        transcript_perm_weights(T, roots + 32, W, K, &out);
    }
    memcpy(challenges, out.data(), 8 * out.size());
    const FsSeed z = T.seed();
    memcpy(seed, z.s, sizeof z.s);
    seed[16] = z.phase;
    return out.size();
}
