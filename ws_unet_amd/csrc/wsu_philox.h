// Philox4x32-10 (Salmon et al., SC'11) as the stego simulators (the rules of embed.hip: K23, K28, K30, and K34; of ternary.hip: K38, K39;
// stc.hip: K40, K41) and the stego-key search (ws_keysearch.hip: K35) use it: counter (c0, 0, 0, 0), key (k0, k1), ten rounds of two
// 32 x 32 -> 64 bit products, the key bumped between rounds.  One definition, so a key scanned by K35 selects exactly the pixels K30
// embeds in.  philox_quad / philox_byte: the word(s) of a quad of pixels / of one pixel, as the rules of wsu_embed.h's loop ask for them.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

struct Words4 { uint32_t v[4]; };
__device__ __forceinline__ Words4 philox4x32_10(uint32_t c0, uint32_t k0, uint32_t k1) {
    uint32_t c[4] = {c0, 0u, 0u, 0u};
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Words4{{c[0], c[1], c[2], c[3]}};
}

// byte e = (word e < thr), compared in thr's type: uint32_t, or uint64_t for a threshold that may be 2^32
template <typename T> __device__ __forceinline__ uint32_t below_bytes(const Words4& wd, T thr) {
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) m |= ((T)wd.v[e] < thr ? 1u : 0u) << (8 * e);
    return m;
}
__device__ __forceinline__ uint32_t word_of(const Words4& wd, int e) {                   // (selects: a dynamic index would put the words in LDS)
    return e == 0 ? wd.v[0] : e == 1 ? wd.v[1] : e == 2 ? wd.v[2] : wd.v[3];
}
// a 64-bit seed (an image's, or a stego key) as the generator's key words
struct SeedKey {
    uint32_t k0, k1;
    __device__ __forceinline__ explicit SeedKey(uint64_t seed) : k0((uint32_t)seed), k1((uint32_t)(seed >> 32)) {}
};
// pixel i of an image draws word i % 4 of counter i / 4 (the entries keep i below 2^32, WSU_COUNTER_PIXELS); i0: a multiple of 4
__device__ __forceinline__ Words4 philox_quad(long long i0, const SeedKey& k) { return philox4x32_10((uint32_t)i0 >> 2, k.k0, k.k1); }
__device__ __forceinline__ uint32_t philox_byte(long long i, const SeedKey& k) {
    return word_of(philox4x32_10((uint32_t)i >> 2, k.k0, k.k1), (int)(i & 3));
}
