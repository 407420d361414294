// Connected components of uint8 masks, and the usual clean-up on top of them (keep the largest components, drop the small ones).
//
//   Input     a [h, w] uint8 mask, non-zero = foreground; connectivity c = 4 or 8.  A component is a maximal c-connected set of
//             foreground pixels.
//   Label     background 0; foreground 1 + min{ y * w + x over the pixels of the component }: the raster index of the component's
//             first pixel, plus one.  Canonical: it does not depend on the order of the work and needs no prefix scan (a NumPy / SciPy
//             labelling is brought to the same form with one ndimage.minimum).
//   Ranking   components by area descending, ties to the smaller first-pixel index: the 64-bit key (area << 32) | (0xFFFFFFFF - first)
//             orders them, larger first.
//   clean     (keep, min_area) keeps a component iff (keep == 0 or its rank < keep) and its area >= min_area.  Kept pixels keep their
//             byte, every other foreground pixel becomes 0, background is never written.  keep in 0..CMPC_CC_MAX_KEEP;
//             keep == 0 && min_area <= 1 is label-only: the masks are not written at all.
//   stats     {n_components, area, area_largest, area_kept}, exact integers; {0, 0, 0, 0} for an empty mask.
//
// Every sample's state is two int32 arrays of h * w in ws: P (parent links: -1 background, else the index of a pixel of the same
// component that is <= the pixel's own; a root has P[i] == i) and A (A[root] = area).  A link is only ever lowered (atomicMin), so a
// chain of links strictly decreases and ends at a root after fewer than h * w steps, whatever the interleaving.
//
// Launches, each over all B samples (grid.y = sample), separated by kernel boundaries only -- no workgroup waits for another:
//   local    one workgroup per CMPC_CC_TILE_H x CMPC_CC_TILE_W tile, a wave per 64-pixel tile row.  __ballot gives the row's
//            foreground bits; a pixel starts linked to the first pixel of its run in the row, runs of adjacent rows are united by a
//            min-index union-find in LDS (unions that a neighbour in the tile is sure to make are left to it), the tile's links are
//            flattened and written as global indices; A is cleared.
//   merge    the pixels of a tile's first row and first / last column unite with their neighbours in the tiles before (west,
//            north-west, north, north-east), by the same rule, on P with device-scope atomicMin.
//   flatten  every pixel follows its chain to the root and stores it (the final label); the first pixel of each run in a 64-pixel
//            row segment adds the run's length to A[root] (a run shares one root): one atomicAdd per run, not per pixel.  Counts
//            n_components (roots) and area per wave, one atomicAdd per workgroup.
//   rank     max(keep, 1) rounds: round k takes the 64-bit atomicMax of the keys below round k - 1's winner (the rounds exclude the
//            winners before them; keys are distinct), reduced per wave and workgroup first.
//   filter   drops what clean() does not keep, counts area_kept, stores area_largest.
// Integer atomics only: results are exact and bit-identical from run to run.  Loop bounds: find() follows at most h * w links; a
// union's finds and retries together take fewer than 2 h w steps (each step strictly lowers one of the two indices it holds), 2 * tile
// pixels in LDS.  A loop that reaches its bound sets the status word (the first uint32 of ws, cleared by every call) and leaves: a
// bug ends as a wrong answer and a non-zero status, not as a hang.
#include "cmpc_common.h"
#include "../../include/cmpc.h"

namespace {

constexpr int NTHR = 256;
constexpr int NWAVE = NTHR / 64;
constexpr int TH = CMPC_CC_TILE_H, TW = CMPC_CC_TILE_W;
static_assert(TW == 64, "a wave handles one tile row: the tile is 64 pixels wide");
static_assert(TH % NWAVE == 0, "whole rows per wave");
constexpr int HEADER = 64;                       // bytes: status word, padding
typedef unsigned long long u64;

struct CcArgs {
    unsigned char* masks; int32_t* labels; u64* stats;
    unsigned int* status;                        // ws
    u64* win;                                    // ws + HEADER: [B][CMPC_CC_MAX_KEEP] winners' keys, 0 = none
    int32_t* pa;                                 // ws + HEADER + 64 B: per sample P [n4] then A [n4], n4 = h * w rounded up to 4
    int conn, keep, write;
    int64_t min_area;
    cmpc_cc_desc d[CMPC_EVAL_MAX_BATCH];
    int64_t pa_off[CMPC_EVAL_MAX_BATCH];         // first element of the sample's P in pa
    int64_t lab_off[CMPC_EVAL_MAX_BATCH];        // first element of the sample's labels
};

__host__ __device__ inline int64_t round4(int64_t n) { return (n + 3) & ~(int64_t)3; }
__host__ __device__ inline int words_per_row(int w) { return (w + 63) >> 6; }

__device__ __forceinline__ u64 make_key(unsigned int area, int first) { return ((u64)area << 32) | (u64)(0xFFFFFFFFu - (unsigned int)first); }

// the first pixel of lane x's run in a 64-pixel row with foreground bits `bits` (bit x set)
__device__ __forceinline__ int run_start(u64 bits, int x) {
    const u64 zeros_below = ~bits & ((1ull << x) - 1);
    return zeros_below ? 64 - __clzll(zeros_below) : 0;
}
// one past the last pixel of lane x's run
__device__ __forceinline__ int run_end(u64 bits, int x) {
    const u64 zeros_above = x == 63 ? 0ull : ~bits & (~0ull << (x + 1));
    return zeros_above ? __ffsll(zeros_above) - 1 : 64;
}

// ---- union-find on links that only decrease.  `budget` is shared by the finds and the retries of one union ----------------------------
__device__ __forceinline__ int lds_find(int* s, int p, int& budget) {
    while (budget > 0) {
        const int q = __hip_atomic_load(&s[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (q == p) return p;
        p = q; --budget;
    }
    return p;
}
__device__ __forceinline__ bool lds_unite(int* s, int a, int b, int budget) {
    while (budget > 0) {
        a = lds_find(s, a, budget);
        b = lds_find(s, b, budget);
        if (budget <= 0) break;
        if (a == b) return true;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&s[a], b);
        if (old == a) return true;
        a = old; --budget;                       // somebody lowered the link first: go on from where it points
    }
    return false;
}
__device__ __forceinline__ int glb_find(int32_t* P, int p, int& budget) {
    while (budget > 0) {
        const int q = __hip_atomic_load(&P[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (q == p) return p;
        p = q; --budget;
    }
    return p;
}
__device__ __forceinline__ bool glb_unite(int32_t* P, int a, int b, int budget) {
    while (budget > 0) {
        a = glb_find(P, a, budget);
        b = glb_find(P, b, budget);
        if (budget <= 0) break;
        if (a == b) return true;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&P[a], b);
        if (old == a) return true;
        a = old; --budget;
    }
    return false;
}

// Which of the neighbours before it a foreground pixel must unite with.  w_, nw, n, ne, e: the neighbour is foreground (false
// outside the image; the local kernel also passes false outside the tile, which only adds unions).  The run in the row links the pixel
// to its west neighbour already.  North: not needed when west and north-west are both set (west unites with north-west, its own north,
// or leaves that to its west in turn).  8-connectivity, north clear: north-west unless west is set (west's north), north-east unless
// east is set (east's north; east cannot leave it to its west, because that pixel's north is clear).
__device__ __forceinline__ void needed(int conn, bool w_, bool nw, bool n, bool ne, bool e, bool& do_n, bool& do_nw, bool& do_ne) {
    do_n = n && !(w_ && nw);
    do_nw = conn == 8 && !n && nw && !w_;
    do_ne = conn == 8 && !n && ne && !e;
}

__global__ __launch_bounds__(NTHR) void cc_local_kernel(CcArgs a) {
    const int b = blockIdx.y;
    const cmpc_cc_desc d = a.d[b];
    const unsigned char* m = a.masks + d.off;
    const int64_t n4 = round4((int64_t)d.h * d.w);
    int32_t* P = a.pa + a.pa_off[b];
    int32_t* A = P + n4;
    const int tiles_x = (d.w + TW - 1) / TW, tiles_y = (d.h + TH - 1) / TH;
    const int ntiles = tiles_x * tiles_y;        // <= CMPC_CC_MAX_PIXELS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ int s[TH * TW];
    __shared__ u64 bits[TH];
    bool fail = false;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {               // workgroup-uniform trip count
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int x = tx * TW + lane;
        __syncthreads();                         // the previous tile's s and bits are no longer read
        for (int ly = wave; ly < TH; ly += NWAVE) {
            const int y = ty * TH + ly;
            const bool fg = y < d.h && x < d.w && m[(int64_t)y * d.w + x] != 0;
            const u64 rb = __ballot(fg);
            if (lane == 0) bits[ly] = rb;
            s[ly * TW + lane] = fg ? ly * TW + run_start(rb, lane) : ly * TW + lane;
        }
        __syncthreads();
        for (int ly = wave; ly < TH; ly += NWAVE) {
            if (ly == 0) continue;
            const u64 cur = bits[ly], up = bits[ly - 1];
            if (!((cur >> lane) & 1)) continue;
            const bool w_ = lane > 0 && ((cur >> (lane - 1)) & 1), e = lane < 63 && ((cur >> (lane + 1)) & 1);
            const bool nw = lane > 0 && ((up >> (lane - 1)) & 1), n = (up >> lane) & 1, ne = lane < 63 && ((up >> (lane + 1)) & 1);
            bool do_n, do_nw, do_ne;
            needed(a.conn, w_, nw, n, ne, e, do_n, do_nw, do_ne);
            const int p = ly * TW + lane, q = p - TW;
            if (do_n && !lds_unite(s, p, q, 2 * TH * TW)) fail = true;
            if (do_nw && !lds_unite(s, p, q - 1, 2 * TH * TW)) fail = true;
            if (do_ne && !lds_unite(s, p, q + 1, 2 * TH * TW)) fail = true;
        }
        __syncthreads();
        for (int ly = wave; ly < TH; ly += NWAVE) {
            const int y = ty * TH + ly;
            if (y >= d.h || x >= d.w) continue;
            const int g = y * d.w + x;
            int root = -1;
            if ((bits[ly] >> lane) & 1) {
                int budget = TH * TW;
                const int r = lds_find(s, ly * TW + lane, budget);
                if (budget <= 0) fail = true;
                root = (ty * TH + r / TW) * d.w + tx * TW + (r % TW);
            }
            P[g] = root;
            A[g] = 0;
        }
    }
    if (fail) atomicOr(a.status, 1u);
}

// one wave per 64-pixel row segment (= one tile row), as in every kernel below
__global__ __launch_bounds__(NTHR) void cc_merge_kernel(CcArgs a) {
    const int b = blockIdx.y;
    const cmpc_cc_desc d = a.d[b];
    const int n = d.h * d.w;
    int32_t* P = a.pa + a.pa_off[b];
    const int wpr = words_per_row(d.w);
    const int nw_ = d.h * wpr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool fail = false;
    for (int k = blockIdx.x * NWAVE + wave; k < nw_; k += gridDim.x * NWAVE) {
        const int y = k / wpr, x = (k - y * wpr) * 64 + lane;
        const bool top = y % TH == 0;            // north, north-west and north-east lie in the tiles above
        if (y == 0 && lane != 0) continue;       // nothing before the first row but the west neighbour across a seam
        if (!top && lane != 0 && lane != 63) continue;
        if (x >= d.w) continue;
        const int g = y * d.w + x;
        if (P[g] < 0) continue;                  // background: P's sign does not change after the local kernel
        const bool has_w = x > 0, has_e = x + 1 < d.w, has_n = y > 0;
        const bool w_ = has_w && P[g - 1] >= 0, e = has_e && P[g + 1] >= 0;
        const bool nw = has_n && has_w && P[g - d.w - 1] >= 0, nn = has_n && P[g - d.w] >= 0, ne = has_n && has_e && P[g - d.w + 1] >= 0;
        bool do_n, do_nw, do_ne;
        needed(a.conn, w_, nw, nn, ne, e, do_n, do_nw, do_ne);
        // only what crosses a seam: the rest was united in the tile
        if (lane == 0 && w_ && !glb_unite(P, g, g - 1, 2 * n)) fail = true;
        if (do_n && top && !glb_unite(P, g, g - d.w, 2 * n)) fail = true;
        if (do_nw && (top || lane == 0) && !glb_unite(P, g, g - d.w - 1, 2 * n)) fail = true;
        if (do_ne && (top || lane == 63) && !glb_unite(P, g, g - d.w + 1, 2 * n)) fail = true;
    }
    if (fail) atomicOr(a.status, 1u);
}

// sums of two per-thread counters over the workgroup, one atomicAdd each
__device__ __forceinline__ void block_add2(u64 c0, u64 c1, u64* dst0, u64* dst1) {
    __shared__ u64 sc[NWAVE][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sc[wave][0] = c0; sc[wave][1] = c1; }       // wave-uniform counters
    __syncthreads();
    if (threadIdx.x < 2) {
        u64 t = 0;
        for (int i = 0; i < NWAVE; ++i) t += sc[i][threadIdx.x];
        if (t) atomicAdd(threadIdx.x == 0 ? dst0 : dst1, t);
    }
}

__global__ __launch_bounds__(NTHR) void cc_flatten_kernel(CcArgs a) {
    const int b = blockIdx.y;
    const cmpc_cc_desc d = a.d[b];
    const int n = d.h * d.w;
    int32_t* P = a.pa + a.pa_off[b];
    unsigned int* A = (unsigned int*)(P + round4(n));
    int32_t* lab = a.labels ? a.labels + a.lab_off[b] : nullptr;
    const int wpr = words_per_row(d.w);
    const int nw_ = d.h * wpr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 c_comp = 0, c_area = 0;                  // wave-uniform
    bool fail = false;
    for (int k = blockIdx.x * NWAVE + wave; k < nw_; k += gridDim.x * NWAVE) {          // wave-uniform trip count
        const int y = k / wpr, x = (k - y * wpr) * 64 + lane;
        const int g = y * d.w + x;
        int root = -1;
        if (x < d.w && P[g] >= 0) {
            int budget = n;
            root = glb_find(P, g, budget);
            if (budget <= 0) fail = true;
            P[g] = root;                         // a racing reader sees the old link or the root: both lie on its chain
        }
        const u64 fgb = __ballot(root >= 0);
        if (root >= 0 && run_start(fgb, lane) == lane) atomicAdd(&A[root], (unsigned int)(run_end(fgb, lane) - lane));
        c_comp += __popcll(__ballot(root == g && root >= 0));
        c_area += __popcll(fgb);
        if (lab && x < d.w) lab[g] = root + 1;
    }
    if (fail) atomicOr(a.status, 1u);
    block_add2(c_comp, c_area, &a.stats[4 * b + 0], &a.stats[4 * b + 1]);
}

__global__ __launch_bounds__(NTHR) void cc_rank_kernel(CcArgs a, int round) {
    const int b = blockIdx.y;
    const cmpc_cc_desc d = a.d[b];
    const int n = d.h * d.w;
    const int32_t* P = a.pa + a.pa_off[b];
    const unsigned int* A = (const unsigned int*)(P + round4(n));
    u64* win = a.win + (int64_t)b * CMPC_CC_MAX_KEEP;
    const u64 below = round == 0 ? ~0ull : win[round - 1];       // written by the launch before
    if (below == 0) return;                      // fewer components than rounds
    u64 best = 0;
    for (int g = blockIdx.x * NTHR + threadIdx.x; g < n; g += gridDim.x * NTHR) {
        if (P[g] != g) continue;
        const u64 key = make_key(A[g], g);
        if (key < below && key > best) best = key;
    }
    for (int o = 32; o > 0; o >>= 1) { const u64 v = __shfl_xor(best, o, 64); best = v > best ? v : best; }
    __shared__ u64 sb[NWAVE];
    if ((threadIdx.x & 63) == 0) sb[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < NWAVE; ++i) best = sb[i] > best ? sb[i] : best;
        if (best) atomicMax(&win[round], best);
    }
}

__global__ __launch_bounds__(NTHR) void cc_filter_kernel(CcArgs a) {
    const int b = blockIdx.y;
    const cmpc_cc_desc d = a.d[b];
    const int n = d.h * d.w;
    unsigned char* m = a.masks + d.off;
    const int32_t* P = a.pa + a.pa_off[b];
    const unsigned int* A = (const unsigned int*)(P + round4(n));
    const u64* win = a.win + (int64_t)b * CMPC_CC_MAX_KEEP;
    const u64 least = a.keep > 0 ? win[a.keep - 1] : 0;          // the last ranked key that is kept; 0: fewer components than keep
    const int wpr = words_per_row(d.w);
    const int nw_ = d.h * wpr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 c_kept = 0;                              // wave-uniform
    for (int k = blockIdx.x * NWAVE + wave; k < nw_; k += gridDim.x * NWAVE) {
        const int y = k / wpr, x = (k - y * wpr) * 64 + lane;
        const int g = y * d.w + x;
        bool kept = false;
        if (x < d.w) {
            const int root = P[g];
            if (root >= 0) {
                const unsigned int area = A[root];
                kept = make_key(area, root) >= least && (int64_t)area >= a.min_area;
                if (!kept && a.write) m[g] = 0;
            }
        }
        c_kept += __popcll(__ballot(kept));
    }
    block_add2(c_kept, 0, &a.stats[4 * b + 3], &a.stats[4 * b + 3]);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.stats[4 * b + 2] = win[0] >> 32;
}

// descriptors -> the samples' offsets in the P / A part of the workspace and its size in bytes; everything but the buffers is checked
int plan(const char* who, const cmpc_cc_desc* ds, int B, int64_t* pa_off, int64_t* lab_off, int64_t* bytes) {
    if (!ds) { cmpc_set_error("%s: NULL pointer", who); return CMPC_EINVAL; }
    if (B <= 0 || B > CMPC_EVAL_MAX_BATCH) { cmpc_set_error("%s: B = %d outside 1..%d", who, B, CMPC_EVAL_MAX_BATCH); return CMPC_EINVAL; }
    int64_t el = 0, lab = 0;
    for (int b = 0; b < B; ++b) {
        const cmpc_cc_desc& d = ds[b];
        if (d.h < 1 || d.w < 1) { cmpc_set_error("%s: sample %d: empty mask (%d x %d)", who, b, d.h, d.w); return CMPC_EINVAL; }
        const int64_t n = (int64_t)d.h * d.w;
        if (n > CMPC_CC_MAX_PIXELS) {
            cmpc_set_error("%s: sample %d: %d x %d = %lld pixels, at most %d", who, b, d.h, d.w, (long long)n, CMPC_CC_MAX_PIXELS);
            return CMPC_EINVAL;
        }
        if (pa_off) { pa_off[b] = el; lab_off[b] = lab; }
        el += 2 * round4(n);
        lab += n;
    }
    *bytes = HEADER + (int64_t)sizeof(uint64_t) * CMPC_CC_MAX_KEEP * B + (int64_t)sizeof(int32_t) * el;
    return CMPC_OK;
}

}  // namespace

extern "C" int cmpc_mask_components_workspace(const cmpc_cc_desc* descs_host, int B, int64_t* bytes) {
    if (!bytes) { cmpc_set_error("mask_components_workspace: NULL pointer"); return CMPC_EINVAL; }
    return plan("mask_components_workspace", descs_host, B, nullptr, nullptr, bytes);
}

extern "C" int cmpc_mask_components(unsigned char* masks, int64_t mask_bytes, const cmpc_cc_desc* descs_host, int B, int connectivity,
                                    int keep, int64_t min_area, int32_t* labels, uint64_t* stats, void* ws, int64_t ws_bytes, void* stream) {
    if (!masks || !descs_host || !stats || !ws) { cmpc_set_error("mask_components: NULL pointer"); return CMPC_EINVAL; }
    if (connectivity != 4 && connectivity != 8) { cmpc_set_error("mask_components: connectivity %d, expected 4 or 8", connectivity); return CMPC_EINVAL; }
    if (keep < 0 || keep > CMPC_CC_MAX_KEEP) { cmpc_set_error("mask_components: keep = %d outside 0..%d", keep, CMPC_CC_MAX_KEEP); return CMPC_EINVAL; }
    if (min_area < 0) { cmpc_set_error("mask_components: min_area = %lld is negative", (long long)min_area); return CMPC_EINVAL; }
    CcArgs a;
    int64_t need = 0;
    const int rc = plan("mask_components", descs_host, B, a.pa_off, a.lab_off, &need);
    if (rc) return rc;
    int64_t most_px = 0, most_words = 0, most_tiles = 0;
    for (int b = 0; b < B; ++b) {
        const cmpc_cc_desc& d = descs_host[b];
        const int64_t n = (int64_t)d.h * d.w;
        if (d.off < 0 || d.off > mask_bytes || n > mask_bytes - d.off) {
            cmpc_set_error("mask_components: sample %d: mask at offset %lld + %lld bytes beyond the buffer (%lld)", b, (long long)d.off,
                           (long long)n, (long long)mask_bytes);
            return CMPC_EINVAL;
        }
        a.d[b] = d;
        most_px = std::max(most_px, n);
        most_words = std::max(most_words, (int64_t)d.h * words_per_row(d.w));
        most_tiles = std::max(most_tiles, (int64_t)((d.h + TH - 1) / TH) * ((d.w + TW - 1) / TW));
    }
    if (ws_bytes < need) {
        cmpc_set_error("mask_components: workspace of %lld bytes, %lld needed (cmpc_mask_components_workspace)", (long long)ws_bytes, (long long)need);
        return CMPC_EINVAL;
    }
    if (((uintptr_t)ws & 15) || ((uintptr_t)stats & 7) || ((uintptr_t)labels & 3)) {
        cmpc_set_error("mask_components: the workspace must be 16-byte, stats 8-byte and labels 4-byte aligned");
        return CMPC_EINVAL;
    }
    const int64_t head = HEADER + (int64_t)sizeof(uint64_t) * CMPC_CC_MAX_KEEP * B;
    a.masks = masks; a.labels = labels; a.stats = (u64*)stats;
    a.status = (unsigned int*)ws;
    a.win = (u64*)((char*)ws + HEADER);
    a.pa = (int32_t*)((char*)ws + head);
    a.conn = connectivity; a.keep = keep; a.min_area = min_area;
    a.write = !(keep == 0 && min_area <= 1);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, head, st) != hipSuccess || hipMemsetAsync(stats, 0, sizeof(uint64_t) * 4 * B, st) != hipSuccess) {
        cmpc_set_error("mask_components: hipMemsetAsync");
        return CMPC_EHIP;
    }
    const int64_t cap = std::max(1, 2048 / B);   // memory-bound cap, as in ops_jf.hip: ~2048 workgroups per launch
    const int g_tiles = (int)std::max<int64_t>(1, std::min(most_tiles, cap));
    const int g_words = (int)std::max<int64_t>(1, std::min((most_words + NWAVE - 1) / NWAVE, cap));
    const int g_px = (int)std::max<int64_t>(1, std::min((most_px + NTHR - 1) / NTHR, cap));
    int e;
    hipLaunchKernelGGL(cc_local_kernel, dim3(g_tiles, B), dim3(NTHR), 0, st, a);
    if ((e = cmpc_check_launch("mask_components"))) return e;
    hipLaunchKernelGGL(cc_merge_kernel, dim3(g_words, B), dim3(NTHR), 0, st, a);
    if ((e = cmpc_check_launch("mask_components"))) return e;
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(g_words, B), dim3(NTHR), 0, st, a);
    if ((e = cmpc_check_launch("mask_components"))) return e;
    for (int k = 0; k < std::max(keep, 1); ++k) {
        hipLaunchKernelGGL(cc_rank_kernel, dim3(g_px, B), dim3(NTHR), 0, st, a, k);
        if ((e = cmpc_check_launch("mask_components"))) return e;
    }
    hipLaunchKernelGGL(cc_filter_kernel, dim3(g_words, B), dim3(NTHR), 0, st, a);
    return cmpc_check_launch("mask_components");
}
