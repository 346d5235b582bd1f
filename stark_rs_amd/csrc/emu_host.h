// emu_host.h -- what the emulator's translation units share on the host side (TEST INFRASTRUCTURE): bounded four-word loads
// and stores in place of the kernels' 16-byte accesses, the extended periodic tables as the device builds them, and the
// helper's atomics on one thread.
#pragma once
#include <stdint.h>

#include <vector>

#include "air_core.h"

extern "C" int emu_ntt(uint64_t p, uint64_t g, const uint32_t *in, uint32_t *out, uint32_t L, uint32_t n_in, uint32_t batch, uint64_t in_stride,
                       uint64_t out_stride, int inverse, uint64_t offset, uint64_t post_scale);

namespace emu_host {
inline void load4(const uint32_t *src, uint64_t at, uint64_t len, uint32_t v[4]) {
    for (int q = 0; q < 4; q++) v[q] = at + q < len ? src[at + q] : 0u;
}
inline void store4(uint32_t *dst, uint64_t at, uint64_t len, const uint32_t v[4]) {
    for (int q = 0; q < 4; q++)
        if (at + q < len) dst[at + q] = v[q];
}
// the extended periodic tables at the places AirPeriodic names (emu_air.cpp builds them the same way)
inline bool periodic_tables(uint64_t p, uint64_t g, const AirPeriodic &P, std::vector<uint32_t> *tab) {
    tab->assign(P.table_words, 0);
    for (const AirPeriodGroup &gr : P.groups) {
        const uint64_t per = 1ull << gr.log_period, len = 1ull << gr.log_len;
        std::vector<uint32_t> coef(gr.count * per);
        if (emu_ntt(p, g, P.vals.data() + gr.in_off, coef.data(), gr.log_period, (uint32_t)per, gr.count, per, per, 1, 1, gr.lde_offset)) return false;
        if (emu_ntt(p, g, coef.data(), tab->data() + gr.out_off, gr.log_len, (uint32_t)per, gr.count, per, len, 0, 1, 1)) return false;
    }
    return true;
}
struct HostAtomics {
    uint32_t cas(uint32_t *a, uint32_t expect, uint32_t v) const {
        const uint32_t old = *a;
        if (old == expect) *a = v;
        return old;
    }
    void min(uint32_t *a, uint32_t v) const {
        if (v < *a) *a = v;
    }
    void add(uint32_t *a, uint32_t v) const { *a += v; }
};
}  // namespace emu_host
