// philox_normals.h -- the seeded generator of the sampler (sampler.hip) and of the forecast paths (paths.hip): Philox4x32-10 words, Box-Muller in
// fp32, and THE counter layout (include/moihgp.h).  Nothing of it touches memory.
#pragma once
#include "common.h"
#include <cstdint>

namespace moihgp {
namespace {

// Philox4x32-10 (Salmon et al., Random123): counter c[4], key k[2] -> four words
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* w) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
// two normals of a pair of words (Box-Muller in fp32, the accurate library functions)
__device__ __forceinline__ void word_pair_normals(uint32_t a, uint32_t b, float& n0, float& n1) {
    const float u1 = ((float)(a >> 8) + 0.5f) * 0x1p-24f, u2 = ((float)(b >> 8) + 0.5f) * 0x1p-24f;
    const float rho = sqrtf(-2.0f * logf(u1)), ang = 6.283185307179586f * u2;
    n0 = rho * cosf(ang);
    n1 = rho * sinf(ang);
}
// THE counter layout: key = the seed's two words, counter = (q, latent, sample, tag).  tag 0: the normals of ticks 4q .. 4q+3 of a sample inside
// the stream; tag 1 (q = 0): its start normals g_0 .. g_3; tag 2: the normals of steps 4q .. 4q+3 of a forecast path.  Words (0, 1) give the
// first two, words (2, 3) the other two.
__device__ __forceinline__ void sample_normals4(unsigned long long seed, uint32_t q, uint32_t latent, uint32_t sample, uint32_t tag, float* n) {
    uint32_t w[4];
    philox4x32_10(q, latent, sample, tag, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    word_pair_normals(w[0], w[1], n[0], n[1]);
    word_pair_normals(w[2], w[3], n[2], n[3]);
}

}  // namespace
}  // namespace moihgp
