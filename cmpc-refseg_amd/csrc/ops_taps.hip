// cmpc_taps_copy: whole per-frame backbone tap blocks between two sets of buffers, up to three levels and eight frames in ONE launch
// (segment.ClipSegmenter: the backbone's output slot -> the ring of cached taps, and the ring -> the head's contiguous [5, h, w, C]
// inputs).  Pure data movement: every address comes from kernel arguments (indices, pointers and block sizes are passed by value, nothing
// is read from device memory to decide one), every access is a 16-byte vector load or store, consecutive lanes take consecutive chunks.
#include "cmpc_common.h"
#include "../../include/cmpc.h"
#include <algorithm>

#define ST ((hipStream_t)stream)

namespace {

constexpr int NTHR = 256;
constexpr int UNROLL = 4;                    // 16-byte chunks in flight per lane: 4 loads issued before the first store
constexpr int MAX_BLOCKS = 4096;             // 256 CUs x 16: past this a workgroup strides over its block instead

struct TapsArgs {
    const uint4* src[CMPC_TAPS_MAX_LEVELS];
    uint4* dst[CMPC_TAPS_MAX_LEVELS];
    uint32_t chunks[CMPC_TAPS_MAX_LEVELS];   // 16-byte chunks of one frame's block
    uint32_t wgs[CMPC_TAPS_MAX_LEVELS];      // workgroups per (level, frame)
    uint32_t first[CMPC_TAPS_MAX_LEVELS];    // first workgroup of the level: levels are laid out one after the other in the grid
    int src_idx[CMPC_TAPS_MAX_FRAMES], dst_idx[CMPC_TAPS_MAX_FRAMES];
    int levels, n;
};

__global__ __launch_bounds__(NTHR) void taps_copy_kernel(const TapsArgs a) {
    const uint32_t wg = blockIdx.x;
    int l = 0;
    if (a.levels > 1 && wg >= a.first[1]) l = 1;
    if (a.levels > 2 && wg >= a.first[2]) l = 2;
    // the arrays are indexed with wave-uniform values only: they stay in scalar registers, no scratch
    const uint32_t chunks = l == 0 ? a.chunks[0] : l == 1 ? a.chunks[1] : a.chunks[2];
    const uint32_t wgs = l == 0 ? a.wgs[0] : l == 1 ? a.wgs[1] : a.wgs[2];
    const uint32_t r = wg - (l == 0 ? a.first[0] : l == 1 ? a.first[1] : a.first[2]);
    const uint32_t j = r / wgs, part = r - j * wgs;
    int si = 0, di = 0;
#pragma unroll
    for (int k = 0; k < CMPC_TAPS_MAX_FRAMES; ++k)
        if ((uint32_t)k == j) { si = a.src_idx[k]; di = a.dst_idx[k]; }
    const uint4* __restrict__ s = (l == 0 ? a.src[0] : l == 1 ? a.src[1] : a.src[2]) + (size_t)si * chunks;
    uint4* __restrict__ d = (l == 0 ? a.dst[0] : l == 1 ? a.dst[1] : a.dst[2]) + (size_t)di * chunks;
    const uint32_t step = wgs * NTHR * UNROLL;
    for (uint32_t base = part * (NTHR * UNROLL); base < chunks; base += step) {      // base is workgroup-uniform
        const uint32_t c0 = base + threadIdx.x;
        uint4 v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
            if (c0 + u * NTHR < chunks) v[u] = s[c0 + u * NTHR];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
            if (c0 + u * NTHR < chunks) d[c0 + u * NTHR] = v[u];
    }
}

}  // namespace

extern "C" int cmpc_taps_copy(int levels, void* const* dst_host, const void* const* src_host, const int64_t* bytes_host, int n,
                              const int* dst_idx_host, const int* src_idx_host, int dst_frames, int src_frames, void* stream) {
    if (!dst_host || !src_host || !bytes_host || !dst_idx_host || !src_idx_host) { cmpc_set_error("taps_copy: NULL argument array"); return CMPC_EINVAL; }
    if (levels < 1 || levels > CMPC_TAPS_MAX_LEVELS) { cmpc_set_error("taps_copy: %d levels outside 1..%d", levels, CMPC_TAPS_MAX_LEVELS); return CMPC_EINVAL; }
    if (n < 1 || n > CMPC_TAPS_MAX_FRAMES) { cmpc_set_error("taps_copy: n = %d frames outside 1..%d", n, CMPC_TAPS_MAX_FRAMES); return CMPC_EINVAL; }
    if (dst_frames < 1 || src_frames < 1) { cmpc_set_error("taps_copy: capacity of %d / %d frames (dst / src)", dst_frames, src_frames); return CMPC_EINVAL; }
    TapsArgs a = {};
    a.levels = levels; a.n = n;
    for (int l = 0; l < levels; ++l) {
        if (!dst_host[l] || !src_host[l]) { cmpc_set_error("taps_copy: level %d: NULL pointer", l); return CMPC_EINVAL; }
        const int64_t b = bytes_host[l];
        if (b <= 0 || (b & 15) != 0) { cmpc_set_error("taps_copy: level %d: bytes = %lld is not a positive multiple of 16", l, (long long)b); return CMPC_EINVAL; }
        if (b / 16 > (int64_t)0x7fffffff) { cmpc_set_error("taps_copy: level %d: bytes = %lld is too large (2^35 per frame at most)", l, (long long)b); return CMPC_EINVAL; }
        a.chunks[l] = (uint32_t)(b / 16);
    }
    for (int j = 0; j < n; ++j) {
        if (dst_idx_host[j] < 0 || dst_idx_host[j] >= dst_frames) {
            cmpc_set_error("taps_copy: dst index %d (entry %d) outside the capacity of %d frames", dst_idx_host[j], j, dst_frames); return CMPC_EINVAL; }
        if (src_idx_host[j] < 0 || src_idx_host[j] >= src_frames) {
            cmpc_set_error("taps_copy: src index %d (entry %d) outside the capacity of %d frames", src_idx_host[j], j, src_frames); return CMPC_EINVAL; }
        for (int k = 0; k < j; ++k)
            if (dst_idx_host[k] == dst_idx_host[j]) {
                cmpc_set_error("taps_copy: duplicate dst index %d (entries %d and %d): two blocks would race for one destination", dst_idx_host[j], k, j);
                return CMPC_EINVAL; }
        a.dst_idx[j] = dst_idx_host[j]; a.src_idx[j] = src_idx_host[j];
    }
    for (int l = 0; l < levels; ++l) {
        if (((uintptr_t)dst_host[l] & 15) != 0 || ((uintptr_t)src_host[l] & 15) != 0) { cmpc_set_error("taps_copy: level %d: pointers must be 16-byte aligned", l); return CMPC_EINVAL; }
        a.dst[l] = (uint4*)dst_host[l]; a.src[l] = (const uint4*)src_host[l];
    }
    // one workgroup per NTHR * UNROLL * iters chunks of a block; iters grows until the whole grid fits MAX_BLOCKS
    uint64_t total = 0;
    for (uint32_t iters = 1;; iters *= 2) {
        total = 0;
        for (int l = 0; l < levels; ++l) {
            const uint64_t per = (uint64_t)NTHR * UNROLL * iters;
            a.wgs[l] = (uint32_t)((a.chunks[l] + per - 1) / per);
            a.first[l] = (uint32_t)total;
            total += (uint64_t)a.wgs[l] * n;
        }
        if (total <= MAX_BLOCKS) break;
    }
    hipLaunchKernelGGL(taps_copy_kernel, dim3((uint32_t)total), dim3(NTHR), 0, ST, a);
    return cmpc_check_launch("taps_copy");
}
