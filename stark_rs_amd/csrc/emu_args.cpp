// emu_args.cpp -- CPU emulator of the plain argument list (TEST INFRASTRUCTURE): emu_args_transcript runs the transcript
// layout of the proof.  The list's kernels are the operand list's: emu_args_columns and emu_air_compose_args are in
// emu_xargs.cpp, in front of the code they share with emu_xargs_columns and emu_air_compose_xargs.
#include <string.h>

#include <vector>

#include "transcript_core.h"

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
