// What the reference's pivot-frame step needs from the device (test.py:150-181, 289-307): per result a descriptor of the frame,
// "global feature of each frame = (mask * visual_feature)", and the agreement of two levels' score maps (util/loss.py:51-68).
//
//   mask_pool     desc[i, c] = sum_{y, x} wgt_i[y, x] * feat_i[y, x, c],  area[i] = sum wgt_i, with
//                 wgt_i[y, x] = score_i[y * (sH / h), x * (sW / w)] (soft) or that value >= thresh ? 1 : 0 (hard, the float32 itself)
//   level_agree   counts[i] = (|a_i > t  and  b_i > t|, |a_i > t  or  b_i > t|), exact integers
//
// mask_pool is one read of the tap: N = h * w positions of C channels.  A workgroup is 4 waves; a wave takes every fourth position of
// a chunk of CMPC_POOL_CHUNK positions and each lane 8 consecutive channels of it (one 16-byte load for the 16-bit types, two for
// float32), so a wave reads 64 * 8 consecutive channels and the grid is (ceil(C / 512), ceil(N / CMPC_POOL_CHUNK), n): 400 workgroups
// for 8 results of a 40 x 40 x 1024 tap.  A wave first reads its 16 weights, one per lane, and broadcasts them position by position, so
// that its 16 tap loads depend on nothing but their addresses.  Sums are float32 in a fixed order:
// a lane adds its positions in order, the four waves are added 0 + 1 + 2 + 3 through LDS and stored as the chunk's partial row
// [C + 8] in the workspace (element C holds the partial area), and fold_kernel adds the chunks in order.  No floating-point atomics:
// two calls give the same bits, and a result does not depend on the results beside it.  Nothing but desc, area and ws is written.
//
// level_agree follows ops_jf.hip: the counters are cleared on the stream, every workgroup adds its two sums with one integer atomic each.
#include "cmpc_common.h"
#include "../../include/cmpc.h"

namespace {

constexpr int NTHR = 256;
constexpr int NWAVE = NTHR / 64;
constexpr int CG_T = 64;                         // groups of 8 channels per workgroup: one per lane
constexpr int ROW_PAD = 8;                       // a partial row is [C + ROW_PAD] floats: element C is the area, rows stay 32-byte aligned
typedef unsigned long long u64;

struct PoolArgs {
    const void* feat; int64_t stride;            // elements between results
    const float* score; int sH, sW;
    int h, w, C, mode;
    float thresh;
    float* part;                                 // [n][nchunk][C + ROW_PAD]
    float* desc; float* area;
    int nchunk;
};

template <typename T>
__global__ __launch_bounds__(NTHR) void pool_kernel(PoolArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.z, k = blockIdx.y;
    const int cg = blockIdx.x * CG_T + lane;
    const bool on = cg < a.C / 8;
    const int N = a.h * a.w;
    const int p0 = k * CMPC_POOL_CHUNK, p1 = min(p0 + CMPC_POOL_CHUNK, N);
    const T* f = (const T*)a.feat + (int64_t)i * a.stride + (int64_t)(on ? cg : 0) * 8;
    const float* sc = a.score + (int64_t)i * a.sH * a.sW;
    const int fy = a.sH / a.h, fx = a.sW / a.w;
    // the wave's weights first, one position per lane: the divisions and the score reads run side by side, and the tap loads below
    // depend on nothing but their addresses
    constexpr int PER_WAVE = CMPC_POOL_CHUNK / NWAVE;
    float wl = 0.f;
    {
        const int p = p0 + wave + NWAVE * lane;
        if (lane < PER_WAVE && p < p1) {
            const int y = p / a.w, x = p - y * a.w;
            wl = sc[(int64_t)(y * fy) * a.sW + x * fx];
            if (a.mode == CMPC_POOL_HARD) wl = wl >= a.thresh ? 1.f : 0.f;
        }
    }
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float asum = 0.f;
#pragma unroll
    for (int j = 0; j < PER_WAVE; ++j) {                           // positions in order; past the chunk's end: weight 0, value 0
        const int p = p0 + wave + NWAVE * j;
        const bool in = p < p1;                                    // wave-uniform
        const float wt = __shfl(wl, j, 64);
        asum += wt;
        float v[8];
        ld8<T>(f + (int64_t)(in ? p : p1 - 1) * a.C, v);           // lanes past C / 8 read channel group 0: their sums are not stored
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += wt * (in ? v[e] : 0.f);
    }
    __shared__ float red[NWAVE][CG_T * 8];
    __shared__ float red_a[NWAVE];
#pragma unroll
    for (int e = 0; e < 8; ++e) red[wave][lane * 8 + e] = acc[e];
    if (lane == 0) red_a[wave] = asum;
    __syncthreads();
    float* row = a.part + ((int64_t)i * a.nchunk + k) * (a.C + ROW_PAD);
    for (int t = threadIdx.x; t < CG_T * 8; t += NTHR) {
        const int c = blockIdx.x * CG_T * 8 + t;
        if (c < a.C) row[c] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) row[a.C] = ((red_a[0] + red_a[1]) + red_a[2]) + red_a[3];
}

// desc[i, c] (c < C) and area[i] (c == C): the chunks' partial rows added in order
__global__ __launch_bounds__(NTHR) void fold_kernel(PoolArgs a) {
    const int i = blockIdx.y;
    const int c = blockIdx.x * NTHR + threadIdx.x;
    if (c > a.C) return;
    const int ld = a.C + ROW_PAD;
    const float* p = a.part + (int64_t)i * a.nchunk * ld + c;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < a.nchunk; ++k) s += p[(int64_t)k * ld];
    if (c < a.C) a.desc[(int64_t)i * a.C + c] = s;
    else a.area[i] = s;
}

__global__ __launch_bounds__(NTHR) void agree_kernel(const float* a, const float* b, int64_t hw, float t, u64* counts) {
    const int i = blockIdx.y;
    const float* pa = a + (int64_t)i * hw;
    const float* pb = b + (int64_t)i * hw;
    u64 cI = 0, cU = 0;
    for (int64_t j = (int64_t)blockIdx.x * NTHR + threadIdx.x; j < hw; j += (int64_t)gridDim.x * NTHR) {
        const bool x = pa[j] > t, y = pb[j] > t;
        cI += x && y;
        cU += x || y;
    }
    for (int off = 32; off > 0; off >>= 1) { cI += __shfl_down(cI, off, 64); cU += __shfl_down(cU, off, 64); }
    __shared__ u64 s[NWAVE][2];
    if ((threadIdx.x & 63) == 0) { s[threadIdx.x >> 6][0] = cI; s[threadIdx.x >> 6][1] = cU; }
    __syncthreads();
    if (threadIdx.x < 2) {
        u64 v = 0;
        for (int k = 0; k < NWAVE; ++k) v += s[k][threadIdx.x];
        if (v) atomicAdd(&counts[2 * i + threadIdx.x], v);
    }
}

// the sizes of one mask_pool call -> chunks per result and workspace bytes
int plan(const char* who, int n, int h, int w, int C, int* nchunk, int64_t* bytes) {
    if (n < 1 || n > CMPC_EVAL_MAX_BATCH) { cmpc_set_error("%s: n = %d outside 1..%d", who, n, CMPC_EVAL_MAX_BATCH); return CMPC_EINVAL; }
    if (h < 1 || w < 1 || C < 1) { cmpc_set_error("%s: empty tap (%d x %d x %d)", who, h, w, C); return CMPC_EINVAL; }
    if ((int64_t)h * w > CMPC_POOL_MAX_POSITIONS) {
        cmpc_set_error("%s: %d x %d positions, at most %d", who, h, w, CMPC_POOL_MAX_POSITIONS);
        return CMPC_EINVAL;
    }
    if (C % 8 || C > (1 << 20)) { cmpc_set_error("%s: C = %d must be a multiple of 8, at most %d", who, C, 1 << 20); return CMPC_EINVAL; }
    const int nc = (h * w + CMPC_POOL_CHUNK - 1) / CMPC_POOL_CHUNK;
    if (nchunk) *nchunk = nc;
    *bytes = (int64_t)n * nc * (C + ROW_PAD) * (int64_t)sizeof(float);
    return CMPC_OK;
}

}  // namespace

extern "C" int cmpc_mask_pool_workspace(int n, int h, int w, int C, int64_t* bytes) {
    if (!bytes) { cmpc_set_error("mask_pool_workspace: NULL pointer"); return CMPC_EINVAL; }
    return plan("mask_pool_workspace", n, h, w, C, nullptr, bytes);
}

extern "C" int cmpc_mask_pool(int dt, const void* feat, int64_t feat_stride, const float* score, int sH, int sW, int n, int h, int w, int C,
                              int mode, float thresh, float* desc, float* area, void* ws, int64_t ws_bytes, void* stream) {
    if (!feat || !score || !desc || !area || !ws) { cmpc_set_error("mask_pool: NULL pointer"); return CMPC_EINVAL; }
    PoolArgs a;
    int64_t need = 0;
    const int rc = plan("mask_pool", n, h, w, C, &a.nchunk, &need);
    if (rc) return rc;
    if (dt != DT_F32 && dt != DT_BF16 && dt != DT_F16) { cmpc_set_error("mask_pool: bad dtype %d", dt); return CMPC_EINVAL; }
    if (mode != CMPC_POOL_SOFT && mode != CMPC_POOL_HARD) { cmpc_set_error("mask_pool: unknown mode %d", mode); return CMPC_EINVAL; }
    if (sH < h || sW < w || sH % h || sW % w) {
        cmpc_set_error("mask_pool: a score grid of %d x %d is not a multiple of the tap grid %d x %d", sH, sW, h, w);
        return CMPC_EINVAL;
    }
    const int64_t tap = (int64_t)h * w * C;
    if (feat_stride % 8 || feat_stride < tap) {
        cmpc_set_error("mask_pool: a stride of %lld elements between results: a multiple of 8 >= %lld (one tap) is needed",
                       (long long)feat_stride, (long long)tap);
        return CMPC_EINVAL;
    }
    if (ws_bytes < need) {
        cmpc_set_error("mask_pool: workspace of %lld bytes, %lld needed (cmpc_mask_pool_workspace)", (long long)ws_bytes, (long long)need);
        return CMPC_EINVAL;
    }
    if (((uintptr_t)feat & 15) || ((uintptr_t)ws & 15) || ((uintptr_t)score & 3) || ((uintptr_t)desc & 3) || ((uintptr_t)area & 3)) {
        cmpc_set_error("mask_pool: feat and the workspace must be 16-byte aligned, score, desc and area 4-byte aligned");
        return CMPC_EINVAL;
    }
    a.feat = feat; a.stride = feat_stride; a.score = score; a.sH = sH; a.sW = sW; a.h = h; a.w = w; a.C = C; a.mode = mode;
    a.thresh = thresh; a.part = (float*)ws; a.desc = desc; a.area = area;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((C / 8 + CG_T - 1) / CG_T, a.nchunk, n);
    CMPC_DISPATCH_DT(dt, hipLaunchKernelGGL(pool_kernel<T>, grid, dim3(NTHR), 0, st, a));
    const int e = cmpc_check_launch("mask_pool");
    if (e) return e;
    hipLaunchKernelGGL(fold_kernel, dim3((C + 1 + NTHR - 1) / NTHR, n), dim3(NTHR), 0, st, a);
    return cmpc_check_launch("mask_pool");
}

extern "C" int cmpc_level_agree(const float* a, const float* b, int n, int h, int w, float thresh, uint64_t* counts, void* stream) {
    if (!a || !b || !counts) { cmpc_set_error("level_agree: NULL pointer"); return CMPC_EINVAL; }
    if (n < 1 || n > CMPC_EVAL_MAX_BATCH) { cmpc_set_error("level_agree: n = %d outside 1..%d", n, CMPC_EVAL_MAX_BATCH); return CMPC_EINVAL; }
    if (h < 1 || w < 1) { cmpc_set_error("level_agree: empty map (%d x %d)", h, w); return CMPC_EINVAL; }
    if (thresh != thresh) { cmpc_set_error("level_agree: the threshold is NaN"); return CMPC_EINVAL; }
    if (((uintptr_t)a & 3) || ((uintptr_t)b & 3) || ((uintptr_t)counts & 7)) {
        cmpc_set_error("level_agree: the maps must be 4-byte aligned, counts 8-byte aligned");
        return CMPC_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, sizeof(uint64_t) * 2 * n, st) != hipSuccess) { cmpc_set_error("level_agree: hipMemsetAsync"); return CMPC_EHIP; }
    const int64_t hw = (int64_t)h * w;
    const int g = (int)std::max<int64_t>(1, std::min<int64_t>((hw + 4 * NTHR - 1) / (4 * NTHR), std::max(1, 2048 / n)));
    hipLaunchKernelGGL(agree_kernel, dim3(g, n), dim3(NTHR), 0, st, a, b, hw, thresh, (u64*)counts);
    return cmpc_check_launch("level_agree");
}
