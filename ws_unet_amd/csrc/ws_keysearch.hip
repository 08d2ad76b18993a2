// K35: the stego-key search over WS residual sums (Fridrich, Goljan, Soukal, "Searching for the stego-key", Proc. SPIE 5306, 2004, with
// the per-pixel WS terms of A. D. Ker, MM&Sec 2008, as the evidence).  Not part of the reference.
//
//   K29 leaves two int64 planes: num (the weighted residual terms) and den (the weights).  A candidate key selects pixels exactly as K30
//   does (word i % 4 of Philox4x32-10 on counter (i / 4, 0, 0, 0) under the key, below thr); the pixels a wrong key selects are a random
//   sample of the image, whose mean term is about half the change rate, the pixels the right key selects (at a threshold at or below the
//   embedder's: the selections nest) all carry payload and their mean term is about 1/2.  Per key the kernel returns the two masked sums
//       snum[j] = sum of num[i] over the selected i < count,   sden[j] likewise,
//   two's-complement int64, wrapping: exact integers, so the result depends on neither the grid, `parts` nor the order of the adds.
//
// Thread = key, 256 keys per workgroup, grid.y = `parts` contiguous slices of the quad range (a quad = four pixels = one generator call).
// All lanes of a wave walk the same quads, so num and den are read through wave-uniform (scalar) loads, 64 bytes per quad and wave; the
// work is the generator: twenty 32 x 32 -> 64 bit products and about as many xors per quad and key, then eight conditional 64-bit adds.
// Both sums stay in the thread's registers: no cross-lane reduction, no LDS, no barrier.  With one part a key has one owner, which writes
// its sums with a plain vector store; with more the parts add theirs with 64-bit vector atomics (two per key and part).  parts = 0
// brings the grid to about WKS_FILL workgroups when there are few keys (the second stage of a search: a short list over a whole frame),
// but leaves a part at least WKS_MIN_QUADS quads.
#include "wsu_device.h"
#include "wsu_philox.h"

namespace {

constexpr int WKS_FILL = 1024;                           // automatic parts: bring the grid to about this many workgroups (256 CUs x 4)
constexpr long long WKS_MIN_QUADS = 64;                  // ... of at least this many quads each

// the quad's four pixels under one key; GUARD: the frame's last, partial quad (i < count is uniform over the grid)
template <bool GUARD>
__device__ __forceinline__ void add_quad(const unsigned long long* __restrict__ num, const unsigned long long* __restrict__ den,
                                         unsigned long long q, long long count, uint32_t k0, uint32_t k1, uint32_t tmax,
                                         unsigned long long& a, unsigned long long& b) {
    unsigned long long n[4], d[4];                       // read before the generator call and whatever it selects: uniform loads, merged
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned long long i = 4 * q + e;
        const bool in = !GUARD || (long long)i < count;
        n[e] = in ? num[i] : 0ull;
        d[e] = in ? den[i] : 0ull;
    }
    const Words4 wd = philox4x32_10((uint32_t)q, k0, k1);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned long long on = wd.v[e] <= tmax ? ~0ull : 0ull;    // word < thr for thr = tmax + 1 in 1..2^32
        a += n[e] & on;
        b += d[e] & on;
    }
}

__global__ __launch_bounds__(256) void ws_key_search_kernel(const unsigned long long* __restrict__ num, const unsigned long long* __restrict__ den,
                                                            long long count, const uint64_t* __restrict__ keys, uint64_t key_first, int k,
                                                            uint32_t tmax, unsigned long long* __restrict__ snum,
                                                            unsigned long long* __restrict__ sden) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;                                  // (no barrier below)
    const uint64_t key = keys ? keys[j] : key_first + (uint64_t)j;       // (wraps mod 2^64)
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    const long long quads = (count + 3) / 4, full = count / 4;
    const long long per = (quads + gridDim.y - 1) / gridDim.y;
    const long long q0 = (long long)blockIdx.y * per;
    const long long q1 = q0 + per < quads ? q0 + per : quads;            // (q0 >= quads: an empty slice)
    const long long qf = q1 < full ? q1 : full;
    unsigned long long a = 0, b = 0;
    for (long long q = q0; q < qf; ++q) add_quad<false>(num, den, (unsigned long long)q, count, k0, k1, tmax, a, b);
    if (q0 <= full && full < q1) add_quad<true>(num, den, (unsigned long long)full, count, k0, k1, tmax, a, b);
    if (gridDim.y == 1) {                                // (uniform over the grid) the key's only owner
        snum[j] = a;
        sden[j] = b;
    } else {
        if (a) atomicAdd(snum + j, a);
        if (b) atomicAdd(sden + j, b);
    }
}

}  // namespace

extern "C" {

int wsu_ws_key_search(const long long* num, const long long* den, long long count, const uint64_t* keys, uint64_t key_first, int key_range,
                      int k, uint64_t thr, int parts, long long* snum, long long* sden, void* stream) {
    WSU_REQUIRE(num && den && snum && sden, "ws_key_search: null pointer");
    WSU_REQUIRE((keys != nullptr) != (key_range != 0), "ws_key_search: give exactly one of the keys array and the key range");
    WSU_REQUIRE(key_range == 0 || key_range == 1, "ws_key_search: key_range=%d outside {0,1}", key_range);
    WSU_REQUIRE(count >= 1 && count <= (1LL << 34), "ws_key_search: count=%lld pixels outside 1..2^34 (Philox's 32-bit counter word, 4 pixels each)",
                count);
    WSU_REQUIRE(k >= 1, "ws_key_search: k=%d keys outside 1..2^31-1", k);
    WSU_REQUIRE(thr <= (1ull << 32), "ws_key_search: thr=%llu above 2^32", (unsigned long long)thr);
    WSU_REQUIRE(parts >= 0 && parts <= 65535, "ws_key_search: parts=%d outside 0 (automatic) .. 65535", parts);
    WSU_REQUIRE((uintptr_t)num % 8 == 0 && (uintptr_t)den % 8 == 0 && (uintptr_t)keys % 8 == 0 && (uintptr_t)snum % 8 == 0 &&
                (uintptr_t)sden % 8 == 0, "ws_key_search: arrays must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(snum, 0, (size_t)k * sizeof(long long), s) != hipSuccess) return wsu_check_launch("ws_key_search memset");
    if (hipMemsetAsync(sden, 0, (size_t)k * sizeof(long long), s) != hipSuccess) return wsu_check_launch("ws_key_search memset");
    if (thr == 0) return 0;                              // no word is below 0: the sums are the zeros just written
    const long long blocks = ((long long)k + 255) / 256, quads = (count + 3) / 4;
    if (parts == 0) {
        const long long room = quads / WKS_MIN_QUADS;
        parts = (int)(blocks >= WKS_FILL ? 1 : WKS_FILL / blocks);
        if (parts > room) parts = (int)(room < 1 ? 1 : room);
    }
    if (parts > quads) parts = (int)quads;
    hipLaunchKernelGGL(ws_key_search_kernel, dim3((unsigned)blocks, parts), dim3(256), 0, s, reinterpret_cast<const unsigned long long*>(num),
                       reinterpret_cast<const unsigned long long*>(den), count, keys, key_first, k, (uint32_t)(thr - 1),
                       reinterpret_cast<unsigned long long*>(snum), reinterpret_cast<unsigned long long*>(sden));
    return wsu_check_launch("ws_key_search_kernel");
}

}  // extern "C"
