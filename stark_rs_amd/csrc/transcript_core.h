// transcript_core.h -- the Fiat-Shamir transcript of the AIR proofs (include/stark_mi.h: "AIR", "AIR over one row-committed
// tree", "Extension FRI", "Permutation argument"), host code: the one derivation of roots -> weights -> FRI's seed that
// provers (air.hip, perm.hip) and verifiers (verify.hip) must agree on bit for bit, written once.  Every challenge is
// Hash::from_bytes of the whole transcript so far (src/fiat_shamir.rs:15-25) -- re-hashed per challenge, no sponge is
// kept -- and its first eight digest bytes, little-endian, are the challenge.  Kept free of HIP so that the CPU build
// (csrc/emu_air.cpp, emu_air_transcript) compiles the same code for tests/test_air_transcript_host.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "hash_core.h"

// A caller's Fiat-Shamir transcript as the prover continues it (hash_core.h fs_seed): the sponge state after its whole
// 32-byte chunks and its trailing bytes, and the count of those trailing bytes.  Computed on the host: the reference's
// transcript is a host Vec<u8>.  The same 17 words are the transcript's state on the device.  phase == 0 (every transcript
// of whole roots, the empty one included) runs the fused Fiat-Shamir sites; phase != 0 takes the single-lane phase-aware
// kernels after each tree and no fused tail.
struct FsSeed {
    uint32_t s[16];
    uint32_t phase;
};
inline FsSeed fs_seed_of(const uint8_t *transcript, size_t len) {
    FsSeed z;
    hashc::fs_seed(transcript, len, z.s, &z.phase);
    return z;
}

struct Transcript {
    std::vector<uint8_t> bytes;
    void absorb(const uint8_t *b, size_t n) { bytes.insert(bytes.end(), b, b + n); }
    void absorb_index(uint64_t j) {   // 8 little-endian bytes
        for (int i = 0; i < 8; i++) bytes.push_back((uint8_t)(j >> (8 * i)));
    }
    uint64_t challenge() const {
        uint32_t d[8];
        hashc::hash_bytes(bytes.data(), bytes.size(), d);
        return (uint64_t)d[0] | ((uint64_t)d[1] << 32);
    }
    FsSeed seed() const { return fs_seed_of(bytes.data(), bytes.size()); }   // what FRI continues
};

// The layouts.  Each appends its challenges to *out and leaves T ready for seed() (or for the next step).
// a root, then the indices first .. first + count - 1 with a challenge after each
inline void transcript_indexed(Transcript &T, const uint8_t root[32], uint64_t first, uint64_t count, std::vector<uint64_t> *out) {
    T.absorb(root, 32);
    for (uint64_t m = 0; m < count; m++) {
        T.absorb_index(first + m);
        out->push_back(T.challenge());
    }
}
// column trees: root c, weight c; then k, weight W + k (K = 0: the build-defined composition of smi_dev_stark_prove)
inline void transcript_columns(Transcript &T, const uint8_t *roots, uint32_t W, uint32_t K, std::vector<uint64_t> *out) {
    for (uint32_t c = 0; c < W; c++) {
        T.absorb(roots + 32 * (size_t)c, 32);
        out->push_back(T.challenge());
    }
    for (uint32_t k = 0; k < K; k++) {
        T.absorb_index(k);
        out->push_back(T.challenge());
    }
}
// one row tree: the root, then j < W + K, weight j
inline void transcript_rows(Transcript &T, const uint8_t root[32], uint32_t W, uint32_t K, std::vector<uint64_t> *out) {
    transcript_indexed(T, root, 0, (uint64_t)W + K, out);
}
// ... over the extension: the root, then m < 4 (W + K), challenge m = coordinate m mod 4 of weight m / 4
inline void transcript_ext(Transcript &T, const uint8_t root[32], uint32_t W, uint32_t K, std::vector<uint64_t> *out) {
    transcript_indexed(T, root, 0, 4 * ((uint64_t)W + K), out);
}
// the permutation proof, in two steps: root_1 and m < 8 (alpha, gamma) -- the column z is built from these --, then
// root_2 and 8 + m for m < 4 (W + K + 2)
inline void transcript_perm_challenges(Transcript &T, const uint8_t root1[32], std::vector<uint64_t> *out) { transcript_indexed(T, root1, 0, 8, out); }
inline void transcript_perm_weights(Transcript &T, const uint8_t root2[32], uint32_t W, uint32_t K, std::vector<uint64_t> *out) {
    transcript_indexed(T, root2, 8, 4 * ((uint64_t)W + K + 2), out);
}
// the argument list (include/stark_mi.h, "Argument list"): transcript_perm_challenges, then root_2 and 8 + m for m < 4 (W + K +
// 2 A); with A = 1 these are transcript_perm_weights' bytes
inline void transcript_args_weights(Transcript &T, const uint8_t root2[32], uint32_t W, uint32_t K, uint32_t A, std::vector<uint64_t> *out) {
    transcript_indexed(T, root2, 8, 4 * ((uint64_t)W + K + 2 * (uint64_t)A), out);
}
