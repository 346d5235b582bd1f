// emu_zk.cpp -- CPU emulator of the zero-knowledge kernels (TEST INFRASTRUCTURE).
//
// emu_random_fill runs random_fill_kernel's lanes over zk_rand_lane, emu_zk_segments runs zk_segments_kernel's grid over
// zk_seg_group, the body the kernel's lanes run, with bounded word loads (zk_core.h).  emu_zk_derived_air hands out
// the tables of the derived AIR that the plan and a prover build (zk_derive_air).  Same arguments and statuses as the C ABI,
// with (p, g) in place of a context.
#include <string.h>

#include <string>
#include <vector>

#include "tables.h"
#include "zk_core.h"

namespace {
void load4(const uint32_t *src, uint64_t at, uint64_t len, uint32_t v[4]) {
    for (int q = 0; q < 4; q++) v[q] = at + q < len ? src[at + q] : 0u;
}
void store4(uint32_t *dst, uint64_t at, uint64_t len, const uint32_t v[4]) {
    for (int q = 0; q < 4; q++)
        if (at + q < len) dst[at + q] = v[q];
}
}  // namespace

extern "C" int emu_random_fill(uint64_t p, const uint8_t *seed, uint64_t stream_id, uint32_t *out, uint64_t count) {
    if (p < 3 || p >= (1ull << 30) || !(p & 1)) return SMI_ERR_UNSUPPORTED_PRIME;
    const Fp F = fp_make((uint32_t)p);
    const ZkRandSeed S = zk_rand_seed(seed, stream_id);
    const uint64_t lanes = (count + ZK_RAND_PER_LANE - 1) / ZK_RAND_PER_LANE;
    for (uint64_t lane = 0; lane < lanes; lane++) {
        uint32_t v[ZK_RAND_PER_LANE];
        zk_rand_lane(S.mid, lane, F, v);
        for (int q = 0; q < ZK_RAND_PER_LANE; q++)
            if (lane * ZK_RAND_PER_LANE + q < count) out[lane * ZK_RAND_PER_LANE + q] = v[q];
    }
    return SMI_OK;
}

extern "C" int emu_zk_segments(uint64_t p, const uint32_t *hc, uint64_t h_stride, uint64_t h_len, uint32_t log_n, uint32_t k_s, uint32_t n_segments,
                               const uint32_t *rho, uint32_t *out, uint64_t out_stride) {
    if (p < 3 || p >= (1ull << 30) || !(p & 1)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (log_n < 2 || log_n > 27) return SMI_ERR_BAD_ARG;
    const uint64_t n = 1ull << log_n;
    if (!k_s || k_s >= n / 2 || !n_segments || 4 * n_segments + 5 > ZK_MAX_RECORD || (n_segments > 1 && !rho)) return SMI_ERR_BAD_ARG;
    const uint64_t L = n - k_s;
    if (h_stride < h_len || out_stride < n || h_len > (uint64_t)n_segments * L) return SMI_ERR_BAD_ARG;
    const ZkSegShape S{n, L, h_len, k_s, n_segments};
    for (uint32_t col = 0; col < 4 * n_segments; col++)
        for (uint64_t m0 = 0; m0 < n; m0 += 4)
            zk_seg_group(S, col, m0, hc, h_stride, rho, out, out_stride, (uint32_t)p, load4, store4);
    return SMI_OK;
}

// head: n_constraints, n_terms, n_factors, n_boundary, n_periodic, the periodic values' count; the arrays take what head says
// (call once with the arrays null for the sizes).  The exemption column is filled: w_n comes from (p, g).
extern "C" int emu_zk_derived_air(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, uint64_t *head, uint32_t *cft, uint64_t *coeff,
                                  uint32_t *tff, uint32_t *var, uint32_t *exp, uint32_t *plog, uint64_t *pval) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs) || !cfg || cfg->log_n > fs.K) return SMI_ERR_UNSUPPORTED_PRIME;
    ZkAir Z;
    std::string why;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - cfg->log_n), fs.F.p);
    const int rc = zk_derive_air(p, w_n, cfg, air, &Z, &why);
    if (rc != SMI_OK) return rc;
    const uint64_t h[6] = {Z.air.n_constraints, Z.air.n_terms, Z.air.n_factors, Z.air.n_boundary, Z.air.n_periodic, Z.pval.size()};
    memcpy(head, h, sizeof h);
    if (!cft) return SMI_OK;
    memcpy(cft, Z.cft.data(), Z.cft.size() * 4);
    memcpy(coeff, Z.coeff.data(), Z.coeff.size() * 8);
    memcpy(tff, Z.tff.data(), Z.tff.size() * 4);
    memcpy(var, Z.var.data(), Z.var.size() * 4);
    memcpy(exp, Z.exp.data(), Z.exp.size() * 4);
    memcpy(plog, Z.plog.data(), Z.plog.size() * 4);
    memcpy(pval, Z.pval.data(), Z.pval.size() * 8);
    return SMI_OK;
}
