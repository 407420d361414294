// Region similarity J and boundary accuracy F of video object segmentation (the DAVIS-2017 measures db_eval_iou and f_measure, by
// which Refer-YouTube-VOS and Refer-DAVIS are ranked) as six exact integers per (prediction, ground truth) pair:
//
//   mask_jf   I = |pred & gt|, U = |pred | gt|, n_pred = |bmap(pred)|, n_gt = |bmap(gt)|,
//             pred_match = |bmap(pred) & dilate(bmap(gt), disc(r))|, gt_match = |bmap(gt) & dilate(bmap(pred), disc(r))|
//
// bmap(seg) is the measure's boundary map: with e, s, se the mask read one pixel to the east, south and south-east (zero outside),
// b = (seg ^ e) | (seg ^ s) | (seg ^ se); then the last row becomes seg ^ e, the last column seg ^ s, the bottom-right pixel 0, in that
// order.  The disc holds the offsets dx^2 + dy^2 <= r^2: on row y + dy a pixel of the other map lies in [x - hw, x + hw] with
// hw = isqrt(r^2 - dy^2); pixels outside the image contribute nothing.  These restate the DAVIS evaluation code, which is not
// available to this project: parity against it is unpinned (tests/jf_ref.py states the same rules in NumPy).
//
// Two launches.  bmap_kernel: one thread per pixel, a wave per 64 pixels of a row; __ballot packs bmap(pred) and bmap(gt) into one
// 64-bit word each (bits past w stay zero) and __popcll counts I, U, n_pred, n_gt.  match_kernel: one thread per word and direction;
// a zero word (the common case) is done at once; otherwise the other map's rows y - r .. y + r are dilated horizontally by hw(dy),
// ORed, ANDed with the thread's own word and counted.  hw <= 128, so a 64-bit target word sees five words of the other row: its own
// (shift-ORs by doubling), and two to either side, of which only the nearest set bit matters (a run of target bits from one end).
// Integer atomics on the six counters: the result does not depend on the order.  The kernels write nothing but counts and ws.
#include "cmpc_common.h"
#include "../../include/cmpc.h"

namespace {

constexpr int NTHR = 256;
constexpr int NWAVE = NTHR / 64;
typedef unsigned long long u64;

struct JfArgs {
    const unsigned char* pred; const unsigned char* gt;
    u64* counts; u64* ws;
    cmpc_jf_desc d[CMPC_EVAL_MAX_BATCH];
    int64_t ws_off[CMPC_EVAL_MAX_BATCH];         // first word of the sample in ws: [2][h][ceil(w / 64)], bmap(pred) then bmap(gt)
};

__host__ __device__ inline int words_per_row(int w) { return (w + 63) >> 6; }

__device__ __forceinline__ bool bmap_at(const unsigned char* m, int h, int w, int y, int x) {
    const int64_t i = (int64_t)y * w + x;
    const bool in_e = x + 1 < w, in_s = y + 1 < h;
    const bool seg = m[i] != 0;
    const bool e = in_e && m[i + 1] != 0;
    const bool s = in_s && m[i + w] != 0;
    const bool se = in_e && in_s && m[i + w + 1] != 0;
    bool b = (seg != e) || (seg != s) || (seg != se);
    if (!in_s) b = seg != e;                     // the last row
    if (!in_e) b = seg != s;                     // then the last column
    if (!in_s && !in_e) b = false;               // then the bottom-right pixel
    return b;
}

__global__ __launch_bounds__(NTHR) void bmap_kernel(JfArgs a) {
    const int b = blockIdx.y;
    const cmpc_jf_desc d = a.d[b];
    const unsigned char* pm = a.pred + d.pred_off;
    const unsigned char* gm = a.gt + d.gt_off;
    const int wpr = words_per_row(d.w);
    const int64_t nw = (int64_t)d.h * wpr;
    u64* bp = a.ws + a.ws_off[b];
    u64* bg = bp + nw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 cI = 0, cU = 0, cP = 0, cG = 0;          // wave-uniform
    for (int64_t k = (int64_t)blockIdx.x * NWAVE + wave; k < nw; k += (int64_t)gridDim.x * NWAVE) {      // wave-uniform trip count
        const int y = (int)(k / wpr), x = (int)(k - (int64_t)y * wpr) * 64 + lane;
        bool p = false, g = false, p_b = false, g_b = false;
        if (x < d.w) {
            const int64_t i = (int64_t)y * d.w + x;
            p = pm[i] != 0; g = gm[i] != 0;
            p_b = bmap_at(pm, d.h, d.w, y, x);
            g_b = bmap_at(gm, d.h, d.w, y, x);
        }
        const u64 wp = __ballot(p_b), wg = __ballot(g_b);
        cI += __popcll(__ballot(p && g));
        cU += __popcll(__ballot(p || g));
        cP += __popcll(wp);
        cG += __popcll(wg);
        if (lane == 0) { bp[k] = wp; bg[k] = wg; }
    }
    __shared__ u64 s[NWAVE][4];
    if (lane == 0) { s[wave][0] = cI; s[wave][1] = cU; s[wave][2] = cP; s[wave][3] = cG; }
    __syncthreads();
    if (threadIdx.x < 4) {
        u64 t = 0;
        for (int i = 0; i < NWAVE; ++i) t += s[i][threadIdx.x];
        if (t) atomicAdd(&a.counts[6 * b + threadIdx.x], t);
    }
}

// OR of v shifted towards the high / low bits by 0 .. n (n <= 63), by doubling
__device__ __forceinline__ u64 smear_up(u64 v, int n) {
    int c = 1;                                   // v holds the shifts 0 .. c - 1
    while (2 * c <= n + 1) { v |= v << c; c *= 2; }
    if (n + 1 > c) v |= v << (n + 1 - c);
    return v;
}
__device__ __forceinline__ u64 smear_down(u64 v, int n) {
    int c = 1;
    while (2 * c <= n + 1) { v |= v >> c; c *= 2; }
    if (n + 1 > c) v |= v >> (n + 1 - c);
    return v;
}
// target bits i >= t (t <= 0: all, t >= 64: none) and i <= u (u < 0: none, u >= 63: all)
__device__ __forceinline__ u64 bits_from(int t) { return t <= 0 ? ~0ull : t >= 64 ? 0ull : ~0ull << t; }
__device__ __forceinline__ u64 bits_upto(int u) { return u < 0 ? 0ull : u >= 63 ? ~0ull : ~0ull >> (63 - u); }

__global__ __launch_bounds__(NTHR) void match_kernel(JfArgs a) {
    const int b = blockIdx.y;
    const cmpc_jf_desc d = a.d[b];
    const int wpr = words_per_row(d.w), r = d.r;
    const int64_t nw = (int64_t)d.h * wpr;
    const u64* maps = a.ws + a.ws_off[b];
    __shared__ int hw[CMPC_JF_MAX_RADIUS + 1];   // hw[|dy|] = isqrt(r^2 - dy^2)
    for (int dy = threadIdx.x; dy <= r; dy += NTHR) {
        const int v = r * r - dy * dy;
        int q = (int)sqrtf((float)v);
        while (q * q > v) --q;
        while ((q + 1) * (q + 1) <= v) ++q;
        hw[dy] = q;
    }
    __syncthreads();
    u64 cnt[2] = {0, 0};                         // pred_match, gt_match
    for (int64_t t = (int64_t)blockIdx.x * NTHR + threadIdx.x; t < 2 * nw; t += (int64_t)gridDim.x * NTHR) {
        const int dir = t >= nw;                 // 0: bmap(pred) against dilated bmap(gt); 1: the roles swapped
        const int64_t k = t - dir * nw;
        const u64 own = maps[dir * nw + k];
        if (!own) continue;
        const u64* other = maps + (1 - dir) * nw;
        const int y = (int)(k / wpr), c = (int)(k - (int64_t)y * wpr);
        const int y0 = max(y - r, 0), y1 = min(y + r, d.h - 1);
        u64 acc = 0;
        for (int yy = y0; yy <= y1 && (own & ~acc); ++yy) {
            const int n = hw[abs(yy - y)];
            const u64* row = other + (int64_t)yy * wpr;
            const u64 m = row[c];
            if (m) acc |= smear_up(m, min(n, 63)) | smear_down(m, min(n, 63));
            // word c + j (j = 1, 2), lowest set bit at q: target bits i with 64 j + q - i <= n
            // word c - j, highest set bit at q: target bits i with i + 64 j - q <= n
            if (c + 1 < wpr) { const u64 v = row[c + 1]; if (v) acc |= bits_from(64 + __ffsll(v) - 1 - n); }
            if (c >= 1) { const u64 v = row[c - 1]; if (v) acc |= bits_upto(n - 64 + (63 - __clzll(v))); }
            if (n > 64) {
                if (c + 2 < wpr) { const u64 v = row[c + 2]; if (v) acc |= bits_from(128 + __ffsll(v) - 1 - n); }
                if (c >= 2) { const u64 v = row[c - 2]; if (v) acc |= bits_upto(n - 128 + (63 - __clzll(v))); }
            }
        }
        cnt[dir] += __popcll(own & acc);
    }
    // wave sums, then one integer atomic per counter and workgroup
    for (int off = 32; off > 0; off >>= 1) { cnt[0] += __shfl_down(cnt[0], off, 64); cnt[1] += __shfl_down(cnt[1], off, 64); }
    __shared__ u64 s[NWAVE][2];
    if ((threadIdx.x & 63) == 0) { s[threadIdx.x >> 6][0] = cnt[0]; s[threadIdx.x >> 6][1] = cnt[1]; }
    __syncthreads();
    if (threadIdx.x < 2) {
        u64 t = 0;
        for (int i = 0; i < NWAVE; ++i) t += s[i][threadIdx.x];
        if (t) atomicAdd(&a.counts[6 * b + 4 + threadIdx.x], t);
    }
}

// descriptors -> the workspace offsets (in words) and the total; everything but the buffers is checked here
int plan(const char* who, const cmpc_jf_desc* ds, int B, int64_t* ws_off, int64_t* words) {
    if (!ds) { cmpc_set_error("%s: NULL pointer", who); return CMPC_EINVAL; }
    if (B <= 0 || B > CMPC_EVAL_MAX_BATCH) { cmpc_set_error("%s: B = %d outside 1..%d", who, B, CMPC_EVAL_MAX_BATCH); return CMPC_EINVAL; }
    int64_t n = 0;
    for (int b = 0; b < B; ++b) {
        const cmpc_jf_desc& d = ds[b];
        if (d.h < 1 || d.w < 1) { cmpc_set_error("%s: sample %d: empty mask (%d x %d)", who, b, d.h, d.w); return CMPC_EINVAL; }
        if (d.r < 1 || d.r > CMPC_JF_MAX_RADIUS) { cmpc_set_error("%s: sample %d: radius %d outside 1..%d", who, b, d.r, CMPC_JF_MAX_RADIUS); return CMPC_EINVAL; }
        if (ws_off) ws_off[b] = n;
        n += 2 * (int64_t)d.h * words_per_row(d.w);
    }
    *words = n;
    return CMPC_OK;
}

}  // namespace

extern "C" int cmpc_mask_jf_workspace(const cmpc_jf_desc* descs_host, int B, int64_t* bytes) {
    if (!bytes) { cmpc_set_error("mask_jf_workspace: NULL pointer"); return CMPC_EINVAL; }
    int64_t words = 0;
    const int rc = plan("mask_jf_workspace", descs_host, B, nullptr, &words);
    if (rc) return rc;
    *bytes = words * (int64_t)sizeof(uint64_t);
    return CMPC_OK;
}

extern "C" int cmpc_mask_jf(const unsigned char* pred, int64_t pred_bytes, const unsigned char* gt, int64_t gt_bytes,
                            const cmpc_jf_desc* descs_host, int B, uint64_t* counts, void* ws, int64_t ws_bytes, void* stream) {
    if (!pred || !gt || !descs_host || !counts || !ws) { cmpc_set_error("mask_jf: NULL pointer"); return CMPC_EINVAL; }
    JfArgs a;
    int64_t words = 0;
    const int rc = plan("mask_jf", descs_host, B, a.ws_off, &words);
    if (rc) return rc;
    int64_t most = 0;
    for (int b = 0; b < B; ++b) {
        const cmpc_jf_desc& d = descs_host[b];
        const int64_t n = (int64_t)d.h * d.w;
        if (d.pred_off < 0 || d.pred_off > pred_bytes || n > pred_bytes - d.pred_off) {
            cmpc_set_error("mask_jf: sample %d: prediction at offset %lld + %lld bytes beyond the buffer (%lld)", b, (long long)d.pred_off,
                           (long long)n, (long long)pred_bytes);
            return CMPC_EINVAL;
        }
        if (d.gt_off < 0 || d.gt_off > gt_bytes || n > gt_bytes - d.gt_off) {
            cmpc_set_error("mask_jf: sample %d: ground truth at offset %lld + %lld bytes beyond the buffer (%lld)", b, (long long)d.gt_off,
                           (long long)n, (long long)gt_bytes);
            return CMPC_EINVAL;
        }
        a.d[b] = d;
        most = std::max(most, (int64_t)d.h * words_per_row(d.w));
    }
    if (ws_bytes < words * (int64_t)sizeof(uint64_t)) {
        cmpc_set_error("mask_jf: workspace of %lld bytes, %lld needed (cmpc_mask_jf_workspace)", (long long)ws_bytes,
                       (long long)(words * (int64_t)sizeof(uint64_t)));
        return CMPC_EINVAL;
    }
    if (((uintptr_t)ws & 7) || ((uintptr_t)counts & 7)) { cmpc_set_error("mask_jf: counts and the workspace must be 8-byte aligned"); return CMPC_EINVAL; }
    a.pred = pred; a.gt = gt; a.counts = (u64*)counts; a.ws = (u64*)ws;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, sizeof(uint64_t) * 6 * B, st) != hipSuccess) { cmpc_set_error("mask_jf: hipMemsetAsync"); return CMPC_EHIP; }
    const int64_t cap = std::max(1, 2048 / B);   // memory-bound cap, as in ops_eval.hip: ~2048 workgroups per launch
    const int g1 = (int)std::max<int64_t>(1, std::min<int64_t>((most + NWAVE - 1) / NWAVE, cap));
    hipLaunchKernelGGL(bmap_kernel, dim3(g1, B), dim3(NTHR), 0, st, a);
    int e = cmpc_check_launch("mask_jf");
    if (e) return e;
    const int g2 = (int)std::max<int64_t>(1, std::min<int64_t>((2 * most + NTHR - 1) / NTHR, cap));
    hipLaunchKernelGGL(match_kernel, dim3(g2, B), dim3(NTHR), 0, st, a);
    return cmpc_check_launch("mask_jf");
}
