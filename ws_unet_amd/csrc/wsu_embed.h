// The pixel loop of the stego simulators and its launch: one definition each of an image's span, the loop over it, the change count and the
// host's launch set-up (embed.hip: K23 through the loop, K22, K28, K30 and K34 beside it; ternary.hip: K38, K39).
#pragma once
#include "wsu_device.h"

// ---- an image as aligned 16-byte groups -------------------------------------------------------------------------------------------------
// An image's pixels as `head` leading bytes, `groups` 16-byte groups whose loads and stores are aligned, and trailing bytes; `bytes` =
// head + tail.  Input and output must share their alignment, else every pixel is a byte; quad: a group must start at a multiple of 4
// pixels (one generator call serves pixels 4g .. 4g+3), else every pixel is a byte as well.
struct Span { long long head, groups, bytes; };
__device__ __forceinline__ Span image_span(const uint8_t* in, const uint8_t* out, long long hw, bool quad) {
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    long long head = hw;
    if (((a ^ b) & 15) == 0) {
        const long long hd = (long long)((16 - (a & 15)) & 15);
        if (hd <= hw && (!quad || hd % 4 == 0)) head = hd;
    }
    const long long groups = (hw - head) / 16;
    return Span{head, groups, hw - 16 * groups};
}
__device__ __forceinline__ long long span_byte_index(const Span& sp, long long j) { return j < sp.head ? j : j + 16 * sp.groups; }

// this thread's count -> one integer atomic per workgroup (wave reduction, then the four wave sums)
__device__ __forceinline__ void add_changes(int cnt, long long* __restrict__ dst, int tid) {
    __shared__ int wsum[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (total) atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)total);
    }
}

// ---- the loop ------------------------------------------------------------------------------------------------------------------------------
// One image of `hw` pixels, `cin` -> `cout`, by the workgroups blockIdx.x of gridDim.x (256 threads each); the changed pixels are added to
// *changes.  A thread takes whole 16-byte groups (one load, four quads, one store), then the bytes before and behind the groups.  What a
// pixel becomes is the rule's business, and so is every saving (a generator call skipped, a cost not read); the loop never asks which
// rule it serves.  A rule holds its image's state (seed halves, threshold, runs, lambda and the cost row) and has
//   uint32_t quad(long long i0, uint32_t x, int& cnt)    pixels i0 .. i0 + 3 (i0 a multiple of 4), byte e of x = pixel i0 + e -> the new word
//   uint8_t  byte(long long i, uint8_t x, int& cnt)      pixel i -> the new byte
// both of which add the pixels they changed to cnt.  A rule's float64 arithmetic lives in the including file, under its contract(off).
//
// Not every simulator kernel is this loop, and the others are not to be folded in: K22 (embed_threshold_kernel) hands 64-bit keys round a
// wave by ballot, 1024 pixels per wave and step, and needs no quad alignment; K34 (embed_threshold_lsbr_kernel) reads and writes bytes on
// purpose, so that any alignment and in-place use are fine; K28 (embed_lsbr_seq_kernel) and K30 (embed_lsbr_keyed_kernel, with the mask
// that has no cover and no count) were rules once, compiled to nearly the same instructions and still measured slower (profiles/r33), so
// their loops are written out in embed.hip.  They share the span and the change count only.  The radix selects and the trellis kernels are no
// pixel loops at all.
template <class Rule>
__device__ __forceinline__ void embed_span(const Rule& rule, const uint8_t* __restrict__ cin, uint8_t* __restrict__ cout, long long hw,
                                           long long* __restrict__ changes) {
    const int tid = threadIdx.x;
    const Span sp = image_span(cin, cout, hw, true);
    int cnt = 0;
    for (long long g = (long long)blockIdx.x * 256 + tid; g < sp.groups; g += (long long)gridDim.x * 256) {
        const long long p = sp.head + 16 * g;                               // a multiple of 4
        u32x4 v = *reinterpret_cast<const u32x4*>(cin + p);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = rule.quad(p + 4 * q, v[q], cnt);
        *reinterpret_cast<u32x4*>(cout + p) = v;
    }
    for (long long j = (long long)blockIdx.x * 256 + tid; j < sp.bytes; j += (long long)gridDim.x * 256) {
        const long long i = span_byte_index(sp, j);
        cout[i] = rule.byte(i, cin[i], cnt);
    }
    add_changes(cnt, changes, tid);
}

// ---- the launch ----------------------------------------------------------------------------------------------------------------------------
constexpr int EMB_MAX_BLOCKS = 64;     // workgroups per image, at most
inline int embed_blocks(long long hw) {
    const long long b = (hw / 16 + 255) / 256;
    return (int)(b < 1 ? 1 : b > EMB_MAX_BLOCKS ? EMB_MAX_BLOCKS : b);
}
// zeroes the n change counters on the stream, then launches `kernel(args...)` over (embed_blocks, n) workgroups of 256 threads
template <class... P, class... A>
inline int embed_launch(const char* memset_name, const char* kernel_name, void (*kernel)(P...), long long* changes, int n, int h, int w,
                        void* stream, A... args) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(changes, 0, (size_t)n * sizeof(long long), s) != hipSuccess) return wsu_check_launch(memset_name);
    hipLaunchKernelGGL(kernel, dim3(embed_blocks((long long)h * w), n), dim3(256), 0, s, args...);
    return wsu_check_launch(kernel_name);
}
