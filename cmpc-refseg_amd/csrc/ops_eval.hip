// Evaluation-side image and mask resampling of the reference's `-m test` loop (trainval_model.py:227-303):
//
//   eval_prep     proc_im = img_as_ubyte(resize_and_pad(im, H, W)); feed = proc_im[..., ::-1].astype(float32) - mu
//   eval_mask_iu  I, U of resize_and_crop(up >= thresh, mh, mw) against the ground truth at its original size
//   train_target  target_fine = resize_and_pad(mask_obj, H, W) > 0 of the training reader, and its foreground count (cmpc_train_prep)
//
// The resampler is skimage.transform.resize as cmpc-refseg_amd/hostutil.py restates it on scipy.ndimage: a mirror-mode Gaussian
// (sigma = (f - 1) / 2, radius int(4 sigma + 0.5)) on every shrinking axis, then ndimage.zoom(order=1, mode="mirror", grid_mode=True).
// eval_prep repeats SciPy's float64 arithmetic operation for operation (file-wide contract(off): no fused multiply-adds):
//   - correlate1d's symmetric form  out = x[0] w[0] + sum_{d=r..1} (x[-d] + x[+d]) w[d]   (axis 0, then axis 1)
//   - the zoom's source coordinate  cc = (o + 0.5) (in / out) - 0.5, reflected about 0 when negative; taps floor(cc), floor(cc) + 1
//     (mirrored indices) with weights 1 - t and 1 - (1 - t); the four products ((v wy) wx) summed in row-major tap order
// so proc_im equals the host's bytes except where the device's exp() rounds a Gaussian weight differently from NumPy's.
// eval_mask_iu needs no arithmetic at all: every Gaussian weight inside the radius is positive and the bilinear weight 1 - (1 - t) is
// zero exactly when SciPy's is, so "resampled value > 0" is the OR of the binarised map over the taps with non-zero weight.
#include "cmpc_common.h"
#include "../../include/cmpc.h"
#include "eval_resample.h"          // MAXR, SampleGeo, mirror_idx, zoom_taps, gauss_weights, geometry, sample_geo (shared with ops_vis.hip)

#pragma clang fp contract(off)

namespace {

constexpr int NTHR = 256;

struct PrepArgs {
    const unsigned char* src; int64_t src_bytes;
    unsigned char* proc; float* feed;
    int H, W, B, ty, tx, tiles_x, tiles;
    cmpc_eval_desc d[CMPC_EVAL_MAX_BATCH];
    SampleGeo g[CMPC_EVAL_MAX_BATCH];
};

struct MaskArgs {
    const void* map; int map_dt; int H, W, B; float thresh;
    const unsigned char* gt; unsigned char* mask_out;
    unsigned long long* iu;
    cmpc_eval_desc d[CMPC_EVAL_MAX_BATCH];
    SampleGeo g[CMPC_EVAL_MAX_BATCH];
};

// LDS footprint (bytes) of one tile: raw uint8 rows [ny + 2 ry][nx + 2 rx][c] + vertical pass [ny][nx + 2 rx][c] float64
__host__ __device__ inline void tile_extent(double z, int t, int r, int n, int& span, int& span_r) {
    span = (int)ceil((double)(t - 1) * z) + 6;
    if (span > n + 2) span = n + 2;
    span_r = span + 2 * r;
}

__global__ __launch_bounds__(NTHR) void eval_prep_kernel(PrepArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ double wy[MAXR + 1], wx[MAXR + 1];
    const int b = blockIdx.y;
    const cmpc_eval_desc d = a.d[b];
    const SampleGeo g = a.g[b];
    const int C = d.c, h = d.h, w = d.w;
    if (threadIdx.x == 0) {
        if (g.sy > 0.0) gauss_weights(g.sy, g.ry, wy);
        if (g.sx > 0.0) gauss_weights(g.sx, g.rx, wx);
    }
    int NYb, NYr, NXb, NXr;
    tile_extent(g.zy, a.ty, g.ry, h, NYb, NYr);
    tile_extent(g.zx, a.tx, g.rx, w, NXb, NXr);
    unsigned char* raw = lds;                                                       // [NYr][NXr][C]
    double* vy = (double*)(lds + (((size_t)NYr * NXr * C + 15) & ~(size_t)15));      // [NYb][NXr][C]
    const unsigned char* src = a.src + d.offset;
    const double mu[3] = {104.00698793, 116.66876762, 122.67891434};               // trainval_model.py:371 (B, G, R)
    __syncthreads();

    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int oy0 = (tile / a.tiles_x) * a.ty, ox0 = (tile % a.tiles_x) * a.tx;
        // the tile's part of the resized rectangle, in resized coordinates
        const int ya = max(oy0 - d.top, 0), yb = min(oy0 + a.ty - d.top, d.rh);
        const int xa = max(ox0 - d.left, 0), xb = min(ox0 + a.tx - d.left, d.rw);
        const bool any = ya < yb && xa < xb;
        int lo_y = 0, lo_x = 0, ny = 0, nx = 0;
        if (any) {
            // source rows / columns the bilinear taps can reach (one extra on each side covers the reflections at the edges)
            lo_y = max(0, (int)floor(((double)ya + 0.5) * g.zy - 0.5) - 1);
            lo_x = max(0, (int)floor(((double)xa + 0.5) * g.zx - 0.5) - 1);
            ny = min(h - 1, (int)floor(((double)(yb - 1) + 0.5) * g.zy - 0.5) + 2) - lo_y + 1;
            nx = min(w - 1, (int)floor(((double)(xb - 1) + 0.5) * g.zx - 0.5) + 2) - lo_x + 1;
            ny = min(ny, NYb); nx = min(nx, NXb);           // never binding (tile_extent has slack): keeps LDS indexing in range
            const int nyr = ny + 2 * g.ry, nxr = nx + 2 * g.rx;
            const int rowb = nxr * C;
            // stage the mirrored footprint: consecutive threads take consecutive bytes of a source row
            for (int i = threadIdx.x; i < nyr * rowb; i += NTHR) {
                const int r = i / rowb, k = i - r * rowb;
                const int col = k / C, ch = k - col * C;
                const int sy = mirror_idx(lo_y - g.ry + r, h), sx = mirror_idx(lo_x - g.rx + col, w);
                raw[r * NXr * C + k] = src[((int64_t)sy * w + sx) * C + ch];
            }
            __syncthreads();
            // axis 0: correlate1d (or the plain img_as_float value when the axis is not blurred)
            for (int i = threadIdx.x; i < ny * rowb; i += NTHR) {
                const int r = i / rowb, k = i - r * rowb;
                const unsigned char* col = raw + (r + g.ry) * NXr * C + k;
                double acc;
                if (g.sy > 0.0) {
                    acc = ((double)col[0] / 255.0) * wy[0];
                    for (int dd = g.ry; dd >= 1; --dd)
                        acc = acc + (((double)col[-dd * NXr * C] / 255.0) + ((double)col[dd * NXr * C] / 255.0)) * wy[dd];
                } else {
                    acc = (double)col[0] / 255.0;
                }
                vy[r * NXr * C + k] = acc;
            }
            __syncthreads();
        }
        const int ly = threadIdx.x / a.tx, lx = threadIdx.x - ly * a.tx;
        const int oy = oy0 + ly, ox = ox0 + lx;
        if (ly < a.ty && oy < a.H && ox < a.W) {
            const int y = oy - d.top, x = ox - d.left;
            unsigned char q[3] = {0, 0, 0};
            if (any && y >= 0 && y < d.rh && x >= 0 && x < d.rw) {
                int y0, y1, x0, x1; double wy0, wy1, wx0, wx1;
                zoom_taps(y, g.zy, h, y0, y1, wy0, wy1);
                zoom_taps(x, g.zx, w, x0, x1, wx0, wx1);
                const int ys[2] = {y0 - lo_y, y1 - lo_y}, xs[2] = {x0 - lo_x + g.rx, x1 - lo_x + g.rx};
                const double wys[2] = {wy0, wy1}, wxs[2] = {wx0, wx1};
                for (int c = 0; c < C; ++c) {
                    double t = 0.0;
                    for (int iy = 0; iy < 2; ++iy)
                        for (int ix = 0; ix < 2; ++ix) {
                            const double* row = vy + ys[iy] * NXr * C + c;
                            const int cx = xs[ix];
                            double v;
                            if (g.sx > 0.0) {           // axis 1: correlate1d on the vertical pass
                                v = row[cx * C] * wx[0];
                                for (int dd = g.rx; dd >= 1; --dd) v = v + (row[(cx - dd) * C] + row[(cx + dd) * C]) * wx[dd];
                            } else {
                                v = row[cx * C];
                            }
                            t = t + (v * wys[iy]) * wxs[ix];
                        }
                    const double s = rint(t * 255.0);                        // img_as_ubyte
                    q[c] = (unsigned char)fmin(fmax(s, 0.0), 255.0);
                }
                if (C == 1) q[1] = q[2] = q[0];                              // build_batches.py:67-68
            }
            const int64_t o = (((int64_t)b * a.H + oy) * a.W + ox) * 3;
            if (a.proc) { a.proc[o] = q[0]; a.proc[o + 1] = q[1]; a.proc[o + 2] = q[2]; }
            // proc_im[..., ::-1].astype(float32) -= mu: a float64 subtract rounded once to float32
            a.feed[o] = (float)((double)q[2] - mu[0]);
            a.feed[o + 1] = (float)((double)q[1] - mu[1]);
            a.feed[o + 2] = (float)((double)q[0] - mu[2]);
        }
        __syncthreads();                                    // the next tile overwrites raw / vy
    }
}

template <typename T>
__device__ __forceinline__ bool fg(const T* m, int W, int y, int x, float th) { return (float)m[(int64_t)y * W + x] >= th; }

// foreground of the resampled binarised map at resized position (oy, ox): OR over the non-zero-weight taps of the blurred window
template <typename T>
__device__ bool pred_at(const T* m, int H, int W, float th, const SampleGeo& g, int oy, int ox) {
    int y0, y1, x0, x1; double wy0, wy1, wx0, wx1;
    zoom_taps(oy, g.zy, H, y0, y1, wy0, wy1);
    zoom_taps(ox, g.zx, W, x0, x1, wx0, wx1);
    const int ty[2] = {y0, y1}, tx[2] = {x0, x1};
    const int ny = wy1 != 0.0 ? 2 : 1, nx = wx1 != 0.0 ? 2 : 1;        // w0 = 1 - t is never 0
    const int ry = g.sy > 0.0 ? g.ry : 0, rx = g.sx > 0.0 ? g.rx : 0;
    for (int iy = 0; iy < ny; ++iy)
        for (int ix = 0; ix < nx; ++ix)
            for (int dy = -ry; dy <= ry; ++dy) {
                const int yy = mirror_idx(ty[iy] + dy, H);
                for (int dx = -rx; dx <= rx; ++dx)
                    if (fg(m, W, yy, mirror_idx(tx[ix] + dx, W), th)) return true;
            }
    return false;
}

template <typename T>
__global__ __launch_bounds__(NTHR) void eval_mask_iu_kernel(MaskArgs a) {
    const int b = blockIdx.y;
    const cmpc_eval_desc d = a.d[b];
    const SampleGeo g = a.g[b];
    const T* m = (const T*)a.map + (int64_t)b * a.H * a.W;
    const unsigned char* gt = a.gt + d.offset;
    unsigned char* mo = a.mask_out ? a.mask_out + d.offset : nullptr;
    const int64_t n = (int64_t)d.h * d.w;
    const bool al_gt = (d.offset & 3) == 0;
    unsigned long long I = 0, U = 0;
    for (int64_t i4 = ((int64_t)blockIdx.x * NTHR + threadIdx.x) * 4; i4 < n; i4 += (int64_t)gridDim.x * NTHR * 4) {
        const int k = (int)min((int64_t)4, n - i4);
        uint32_t gv = 0;
        if (k == 4 && al_gt) gv = *(const uint32_t*)(gt + i4);                // 4 ground-truth bytes per load
        else for (int j = 0; j < k; ++j) gv |= (uint32_t)gt[i4 + j] << (8 * j);
        uint32_t pv = 0;
        for (int j = 0; j < k; ++j) {
            const int64_t i = i4 + j;
            const int y = (int)(i / d.w), x = (int)(i - (int64_t)y * d.w);
            const bool p = pred_at(m, a.H, a.W, a.thresh, g, y + d.top, x + d.left);
            const bool t = ((gv >> (8 * j)) & 255u) != 0;
            I += p && t; U += p || t;
            pv |= (uint32_t)p << (8 * j);
        }
        if (mo) {
            if (k == 4 && al_gt) *(uint32_t*)(mo + i4) = pv;
            else for (int j = 0; j < k; ++j) mo[i4 + j] = (unsigned char)(pv >> (8 * j));
        }
    }
    // wave sums, then one integer atomic per wave-partial per block
    for (int off = 32; off > 0; off >>= 1) { I += __shfl_down(I, off, 64); U += __shfl_down(U, off, 64); }
    __shared__ unsigned long long sI[NTHR / 64], sU[NTHR / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sI[wave] = I; sU[wave] = U; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tI = 0, tU = 0;
        for (int i = 0; i < NTHR / 64; ++i) { tI += sI[i]; tU += sU[i]; }
        if (tI) atomicAdd(&a.iu[2 * b], tI);
        if (tU) atomicAdd(&a.iu[2 * b + 1], tU);
    }
}

struct OutArgs {
    const void* map; int H, W; float thresh;
    unsigned char* out; uint32_t value;
    cmpc_eval_desc d[CMPC_EVAL_MAX_BATCH];
    SampleGeo g[CMPC_EVAL_MAX_BATCH];
};

// eval_mask_iu's decision without a ground truth: value * (resampled binarised map > 0) at the descriptor's size, four pixels per thread
template <typename T>
__global__ __launch_bounds__(NTHR) void eval_mask_out_kernel(OutArgs a) {
    const int b = blockIdx.y;
    const cmpc_eval_desc d = a.d[b];
    const SampleGeo g = a.g[b];
    const T* m = (const T*)a.map + (int64_t)b * a.H * a.W;
    unsigned char* mo = a.out + d.offset;
    const int64_t n = (int64_t)d.h * d.w;
    const bool al = ((uintptr_t)mo & 3) == 0;
    for (int64_t i4 = ((int64_t)blockIdx.x * NTHR + threadIdx.x) * 4; i4 < n; i4 += (int64_t)gridDim.x * NTHR * 4) {
        const int k = (int)min((int64_t)4, n - i4);
        uint32_t pv = 0;
        for (int j = 0; j < k; ++j) {
            const int64_t i = i4 + j;
            const int y = (int)(i / d.w), x = (int)(i - (int64_t)y * d.w);
            if (pred_at(m, a.H, a.W, a.thresh, g, y + d.top, x + d.left)) pv |= a.value << (8 * j);
        }
        if (k == 4 && al) *(uint32_t*)(mo + i4) = pv;
        else for (int j = 0; j < k; ++j) mo[i4 + j] = (unsigned char)(pv >> (8 * j));
    }
}

int check_descs(const char* who, const cmpc_eval_desc* ds, int B, int64_t bytes, int H, int W, bool pad, SampleGeo* geo) {
    for (int b = 0; b < B; ++b) {
        const cmpc_eval_desc& d = ds[b];
        if (d.h <= 0 || d.w <= 0) { cmpc_set_error("%s: sample %d: empty or 1-D image (%d x %d)", who, b, d.h, d.w); return CMPC_EINVAL; }
        if (pad ? (d.c != 1 && d.c != 3) : d.c != 1) { cmpc_set_error("%s: sample %d: %d channels", who, b, d.c); return CMPC_EINVAL; }
        if (d.offset < 0 || d.offset > bytes || (int64_t)d.h * d.w * d.c > bytes - d.offset) {
            cmpc_set_error("%s: sample %d: offset %lld + %lld bytes beyond the buffer (%lld)", who, b, (long long)d.offset,
                           (long long)d.h * d.w * d.c, (long long)bytes);
            return CMPC_EINVAL;
        }
        int gm[4];
        if (pad) geometry(d.h, d.w, H, W, true, gm); else geometry(H, W, d.h, d.w, false, gm);
        if (gm[0] != d.rh || gm[1] != d.rw || gm[2] != d.top || gm[3] != d.left || d.rh <= 0 || d.rw <= 0) {
            cmpc_set_error("%s: sample %d: geometry (%d, %d, %d, %d) differs from resize_and_%s_geometry (%d, %d, %d, %d)", who, b, d.rh, d.rw,
                           d.top, d.left, pad ? "pad" : "crop", gm[0], gm[1], gm[2], gm[3]);
            return CMPC_EINVAL;
        }
        const bool ok = pad ? sample_geo(d.h, d.w, d.rh, d.rw, geo[b]) : sample_geo(H, W, d.rh, d.rw, geo[b]);
        if (!ok) { cmpc_set_error("%s: sample %d: shrink factor too large (Gaussian radius > %d)", who, b, MAXR); return CMPC_EINVAL; }
    }
    return CMPC_OK;
}

constexpr size_t LDS_CAP = 64 * 1024 - 2 * (MAXR + 1) * sizeof(double);

size_t prep_lds(const cmpc_eval_desc* ds, const SampleGeo* geo, int B, int ty, int tx) {
    size_t m = 0;
    for (int b = 0; b < B; ++b) {
        int nyb, nyr, nxb, nxr;
        tile_extent(geo[b].zy, ty, geo[b].ry, ds[b].h, nyb, nyr);
        tile_extent(geo[b].zx, tx, geo[b].rx, ds[b].w, nxb, nxr);
        const size_t c = ds[b].c;
        m = std::max(m, (((size_t)nyr * nxr * c + 15) & ~(size_t)15) + (size_t)nyb * nxr * c * sizeof(double));
    }
    return m;
}

// ---- train_target: target_fine = resize_and_pad(mask_obj, H, W) > 0 of the training reader (data_reader_refvos.py:30,33,42) ----------
// As in eval_mask_iu the resampled value is positive exactly when the object bit is set under a tap with non-zero weight, each tap
// widened by the Gaussian window.  Mirrored window indices land inside the clipped window [c - r, c + r] ∩ [0, n), so the window OR is
// the OR over the clipped rectangle, and that is separable: a workgroup stages the object bits of its tile's source footprint plus
// halo (0 outside the image) as bytes, four pixels per 32-bit word, ORs rows (word-wide, funnel shifts), then columns, and every
// thread reads its <= 4 taps from the dilated map.
struct TrainArgs {
    const unsigned char* ann; int64_t ann_bytes;
    float* target; unsigned long long* pos;
    int H, W, B, order, ty, tx;
    cmpc_train_desc d[CMPC_EVAL_MAX_BATCH];
    SampleGeo g[CMPC_EVAL_MAX_BATCH];
};

// LDS words of one tile: bits [NYr][wr] (staged, halo included), hb [NYr][wn] (row OR), dil [NYb][wn] (row and column OR)
struct TileLds { int NYb, NYr, wn, wr; };
__host__ __device__ inline TileLds tile_lds(const SampleGeo& g, int ty, int tx, int h, int w) {
    TileLds t; int NXb, NXr;
    tile_extent(g.zy, ty, g.ry, h, t.NYb, t.NYr);
    tile_extent(g.zx, tx, g.rx, w, NXb, NXr);
    t.wn = (NXb + 3) / 4;
    t.wr = t.wn + (2 * g.rx) / 4 + 2;            // the row pass reads words g .. g + 2 rx / 4 + 1
    return t;
}
__host__ __device__ inline size_t tile_lds_bytes(const TileLds& t) { return sizeof(uint32_t) * ((size_t)t.NYr * t.wr + (size_t)t.NYr * t.wn + (size_t)t.NYb * t.wn); }

__device__ __forceinline__ uint32_t ld_word(const unsigned char* base, int64_t k, int64_t nbytes) {
    if ((k + 1) * 4 <= nbytes) return ((const uint32_t*)base)[k];
    uint32_t v = 0;
    for (int j = 0; j < 4; ++j) if (k * 4 + j < nbytes) v |= (uint32_t)base[k * 4 + j] << (8 * j);
    return v;
}

__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, int bytes) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * bytes)); }

// object bits (one byte each, 0 / 1) of the 4 pixels whose first byte is at A: C + 1 aligned 32-bit loads, then compile-time byte picks
template <int C>
__device__ __forceinline__ uint32_t object_bits4(const unsigned char* ann, int64_t nbytes, int64_t A, int kind, int match, uint32_t key) {
    const int64_t k0 = A >> 2;
    const int sh = (int)(A & 3);
    uint32_t wd[C + 1], al[C];
    for (int i = 0; i <= C; ++i) wd[i] = (i < C || sh) ? ld_word(ann, k0 + i, nbytes) : 0u;
    for (int i = 0; i < C; ++i) al[i] = funnel(wd[i + 1], wd[i], sh);
    uint32_t out = 0;
    for (int j = 0; j < 4; ++j) {
        bool f;
        if (C == 1) {
            const uint32_t v = (al[0] >> (8 * j)) & 255u;
            f = kind == CMPC_ANN_PLAIN ? v != 0 : v == (key & 255u);
        } else {
            f = true;
            for (int ch = 0; ch < 3; ++ch) {
                const int p = j * C + ch;
                const uint32_t v = (al[p >> 2] >> (8 * (p & 3))) & 255u;
                f = f && (ch >= match || v == ((key >> (8 * ch)) & 255u));
            }
        }
        out |= (uint32_t)f << (8 * j);
    }
    return out;
}

__device__ __forceinline__ bool object_bit(const unsigned char* p, int C, int kind, int match, uint32_t key) {
    if (kind == CMPC_ANN_PLAIN) return p[0] != 0;
    bool f = true;
    for (int ch = 0; ch < 3 && ch < C; ++ch) f = f && (ch >= match || p[ch] == ((key >> (8 * ch)) & 255u));
    return f;
}

__global__ __launch_bounds__(NTHR) void train_target_kernel(TrainArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int b = blockIdx.z;
    const cmpc_train_desc d = a.d[b];
    const SampleGeo g = a.g[b];
    const int C = d.c, h = d.h, w = d.w;
    const uint32_t key = (uint32_t)d.key[0] | (uint32_t)d.key[1] << 8 | (uint32_t)d.key[2] << 16;
    const TileLds L = tile_lds(g, a.ty, a.tx, h, w);
    uint32_t* bits = (uint32_t*)lds;                    // [NYr][wr]
    uint32_t* hb = bits + L.NYr * L.wr;                  // [NYr][wn]
    uint32_t* dil = hb + L.NYr * L.wn;                   // [NYb][wn]
    const unsigned char* dilb = (const unsigned char*)dil;
    const unsigned char* src = a.ann + d.offset;
    unsigned long long cnt = 0;

    {                                                   // one output tile per workgroup
        const int oy0 = blockIdx.y * a.ty, ox0 = blockIdx.x * a.tx;
        const int ya = max(oy0 - d.top, 0), yb = min(oy0 + a.ty - d.top, d.rh);
        const int xa = max(ox0 - d.left, 0), xb = min(ox0 + a.tx - d.left, d.rw);
        const bool any = ya < yb && xa < xb;
        int lo_y = 0, lo_x = 0, ny = 0, nx = 0;
        if (any) {
            // source rows / columns the taps can reach (eval_prep's footprint; the order-0 tap floor(cc + 0.5) lies inside it)
            lo_y = max(0, (int)floor(((double)ya + 0.5) * g.zy - 0.5) - 1);
            lo_x = max(0, (int)floor(((double)xa + 0.5) * g.zx - 0.5) - 1);
            ny = min(h - 1, (int)floor(((double)(yb - 1) + 0.5) * g.zy - 0.5) + 2) - lo_y + 1;
            nx = min(w - 1, (int)floor(((double)(xb - 1) + 0.5) * g.zx - 0.5) + 2) - lo_x + 1;
            ny = min(ny, L.NYb); nx = min(nx, 4 * L.wn);    // never binding (tile_extent has slack): keeps LDS indexing in range
            const int nyr = ny + 2 * g.ry, wn = (nx + 3) / 4;
            const int Y0 = lo_y - g.ry, X0 = lo_x - g.rx;
            // stage: one compare per source pixel, four pixels per thread and store
            for (int i = threadIdx.x; i < nyr * L.wr; i += NTHR) {
                const int r = i / L.wr, q = i - r * L.wr;
                const int sy = Y0 + r, sx = X0 + 4 * q;
                uint32_t v = 0;
                if (sy >= 0 && sy < h && sx + 3 >= 0 && sx < w) {
                    if (sx >= 0 && sx + 3 < w) {
                        const int64_t A = d.offset + ((int64_t)sy * w + sx) * C;
                        v = C == 1 ? object_bits4<1>(a.ann, a.ann_bytes, A, d.kind, d.match, key)
                          : C == 3 ? object_bits4<3>(a.ann, a.ann_bytes, A, d.kind, d.match, key)
                                   : object_bits4<4>(a.ann, a.ann_bytes, A, d.kind, d.match, key);
                    } else {
                        for (int j = 0; j < 4; ++j)
                            if (sx + j >= 0 && sx + j < w)
                                v |= (uint32_t)object_bit(src + ((int64_t)sy * w + sx + j) * C, C, d.kind, d.match, key) << (8 * j);
                    }
                }
                bits[i] = v;
            }
            __syncthreads();
            // rows: hb[r][x] = OR bits[r][x .. x + 2 rx]
            for (int i = threadIdx.x; i < nyr * wn; i += NTHR) {
                const int r = i / wn, q = i - r * wn;
                const uint32_t* row = bits + r * L.wr + q;
                uint32_t lo = row[0], acc = lo;
                for (int k = 0; 4 * k < 2 * g.rx; ++k) {
                    const uint32_t hi = row[k + 1];
                    for (int s = 1; s <= 4; ++s)
                        if (4 * k + s <= 2 * g.rx) acc |= funnel(hi, lo, s);
                    lo = hi;
                }
                hb[r * L.wn + q] = acc;
            }
            __syncthreads();
            // columns: dil[y][x] = OR hb[y .. y + 2 ry][x]
            for (int i = threadIdx.x; i < ny * wn; i += NTHR) {
                const int y = i / wn, q = i - y * wn;
                uint32_t acc = 0;
                for (int s = 0; s <= 2 * g.ry; ++s) acc |= hb[(y + s) * L.wn + q];
                dil[y * L.wn + q] = acc;
            }
            __syncthreads();
        }
        const int ly = threadIdx.x / a.tx, lx = threadIdx.x - ly * a.tx;
        const int oy = oy0 + ly, ox = ox0 + lx;
        if (ly < a.ty && oy < a.H && ox < a.W) {
            const int y = oy - d.top, x = ox - d.left;
            bool f = false;
            if (any && y >= 0 && y < d.rh && x >= 0 && x < d.rw) {
                int ys[2], xs[2], nty = 1, ntx = 1;
                if (a.order == 0) {
                    // ndimage.zoom order 0: the sample nearest the grid-mode coordinate
                    ys[0] = min(max((int)floor((((double)y + 0.5) * g.zy - 0.5) + 0.5), 0), h - 1);
                    xs[0] = min(max((int)floor((((double)x + 0.5) * g.zx - 0.5) + 0.5), 0), w - 1);
                } else {
                    double wy0, wy1, wx0, wx1;
                    zoom_taps(y, g.zy, h, ys[0], ys[1], wy0, wy1);
                    zoom_taps(x, g.zx, w, xs[0], xs[1], wx0, wx1);
                    nty = wy1 != 0.0 ? 2 : 1; ntx = wx1 != 0.0 ? 2 : 1;            // w0 = 1 - t is never 0
                }
                for (int iy = 0; iy < nty; ++iy)
                    for (int ix = 0; ix < ntx; ++ix) {
                        const int ry_ = ys[iy] - lo_y, rx_ = xs[ix] - lo_x;
                        if (ry_ >= 0 && ry_ < ny && rx_ >= 0 && rx_ < nx) f = f || dilb[(ry_ * L.wn) * 4 + rx_] != 0;
                    }
            }
            a.target[((int64_t)b * a.H + oy) * a.W + ox] = f ? 1.0f : 0.0f;
            cnt += f;
        }
    }
    // wave sums, then one integer atomic per workgroup
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    __shared__ unsigned long long sC[NTHR / 64];
    if ((threadIdx.x & 63) == 0) sC[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int i = 0; i < NTHR / 64; ++i) t += sC[i];
        if (t) atomicAdd(&a.pos[b], t);
    }
}

// validated descriptors -> one eval_prep_kernel launch (proc_im may be NULL: cmpc_train_prep)
int launch_prep(const char* who, const unsigned char* src, int64_t src_bytes, const cmpc_eval_desc* descs_host, int B, int H, int W,
                unsigned char* proc_im, float* feed, hipStream_t stream) {
    PrepArgs a;
    const int rc = check_descs(who, descs_host, B, src_bytes, H, W, true, a.g);
    if (rc) return rc;
    // tile: 256 threads as ty x tx output pixels; shrink the tile until the staged footprint fits in 64 KB of LDS
    static const int shapes[][2] = {{8, 32}, {4, 32}, {2, 32}, {1, 32}, {1, 16}, {1, 8}, {1, 4}, {1, 1}};
    size_t lds = 0; int ty = 0, tx = 0;
    for (auto& s : shapes) {
        lds = prep_lds(descs_host, a.g, B, s[0], s[1]);
        if (lds <= LDS_CAP) { ty = s[0]; tx = s[1]; break; }
    }
    if (!ty) { cmpc_set_error("%s: source footprint does not fit in LDS", who); return CMPC_EINVAL; }
    a.src = src; a.src_bytes = src_bytes; a.proc = proc_im; a.feed = feed;
    a.H = H; a.W = W; a.B = B; a.ty = ty; a.tx = tx;
    a.tiles_x = (W + tx - 1) / tx;
    a.tiles = a.tiles_x * ((H + ty - 1) / ty);
    for (int b = 0; b < B; ++b) a.d[b] = descs_host[b];
    const int per_sample = std::max(1, std::min(a.tiles, 2048 / B));        // memory-bound cap: ~2048 workgroups per launch
    hipLaunchKernelGGL(eval_prep_kernel, dim3(per_sample, B), dim3(NTHR), lds, stream, a);
    return cmpc_check_launch(who);
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int cmpc_eval_prep(const unsigned char* src, int64_t src_bytes, const cmpc_eval_desc* descs_host, int B, int H, int W,
                              unsigned char* proc_im, float* feed, void* stream) {
    if (!src || !descs_host || !proc_im || !feed) { cmpc_set_error("eval_prep: NULL pointer"); return CMPC_EINVAL; }
    if (B <= 0 || B > CMPC_EVAL_MAX_BATCH) { cmpc_set_error("eval_prep: B = %d outside 1..%d", B, CMPC_EVAL_MAX_BATCH); return CMPC_EINVAL; }
    if (H <= 0 || W <= 0 || src_bytes <= 0) { cmpc_set_error("eval_prep: bad output size %d x %d or buffer length", H, W); return CMPC_EINVAL; }
    return launch_prep("eval_prep", src, src_bytes, descs_host, B, H, W, proc_im, feed, ST);
}

extern "C" int cmpc_eval_mask_iu(const void* map, int map_dt, int B, int H, int W, float thresh, const unsigned char* gt, int64_t gt_bytes,
                                 const cmpc_eval_desc* descs_host, uint64_t* iu, unsigned char* mask_out, void* stream) {
    if (!map || !gt || !descs_host || !iu) { cmpc_set_error("eval_mask_iu: NULL pointer"); return CMPC_EINVAL; }
    if (map_dt != CMPC_EVAL_F32 && map_dt != CMPC_EVAL_U8) { cmpc_set_error("eval_mask_iu: map dtype %d is neither f32 nor u8", map_dt); return CMPC_EINVAL; }
    if (B <= 0 || B > CMPC_EVAL_MAX_BATCH) { cmpc_set_error("eval_mask_iu: B = %d outside 1..%d", B, CMPC_EVAL_MAX_BATCH); return CMPC_EINVAL; }
    if (H <= 0 || W <= 0 || gt_bytes <= 0) { cmpc_set_error("eval_mask_iu: bad map size %d x %d or buffer length", H, W); return CMPC_EINVAL; }
    MaskArgs a;
    const int rc = check_descs("eval_mask_iu", descs_host, B, gt_bytes, H, W, false, a.g);
    if (rc) return rc;
    a.map = map; a.map_dt = map_dt; a.H = H; a.W = W; a.B = B; a.thresh = thresh; a.gt = gt; a.mask_out = mask_out;
    a.iu = (unsigned long long*)iu;
    int64_t most = 0;
    for (int b = 0; b < B; ++b) { a.d[b] = descs_host[b]; most = std::max(most, (int64_t)descs_host[b].h * descs_host[b].w); }
    if (hipMemsetAsync(iu, 0, sizeof(uint64_t) * 2 * B, ST) != hipSuccess) { cmpc_set_error("eval_mask_iu: hipMemsetAsync"); return CMPC_EHIP; }
    const int per_sample = (int)std::max<int64_t>(1, std::min<int64_t>((most + 4 * NTHR - 1) / (4 * NTHR), 2048 / B));
    if (map_dt == CMPC_EVAL_F32) hipLaunchKernelGGL(eval_mask_iu_kernel<float>, dim3(per_sample, B), dim3(NTHR), 0, ST, a);
    else hipLaunchKernelGGL(eval_mask_iu_kernel<unsigned char>, dim3(per_sample, B), dim3(NTHR), 0, ST, a);
    return cmpc_check_launch("eval_mask_iu");
}

namespace {

// cmpc_train_prep's annotation half, validation: descriptors -> kernel arguments and the tile / LDS size.  Nothing is launched.
int plan_target(const char* who, const unsigned char* ann, int64_t ann_bytes, const cmpc_train_desc* ann_descs_host, int B, int H, int W,
                int order, TrainArgs& a, size_t& lds) {
    if (order != 0 && order != 1) { cmpc_set_error("%s: order %d is neither 0 nor 1", who, order); return CMPC_EINVAL; }
    if ((uintptr_t)ann & 3) { cmpc_set_error("%s: the annotation buffer is not 4-byte aligned", who); return CMPC_EINVAL; }
    cmpc_eval_desc e[CMPC_EVAL_MAX_BATCH];
    for (int b = 0; b < B; ++b) {
        const cmpc_train_desc& d = ann_descs_host[b];
        if (d.kind != CMPC_ANN_COLOR && d.kind != CMPC_ANN_PLAIN) { cmpc_set_error("%s: sample %d: unknown annotation kind %d", who, b, d.kind); return CMPC_EINVAL; }
        if (d.kind == CMPC_ANN_COLOR ? (d.c != 3 && d.c != 4) : d.c != 1) {
            cmpc_set_error("%s: sample %d: %d channels for a %s annotation", who, b, d.c, d.kind == CMPC_ANN_COLOR ? "colour-coded" : "plain");
            return CMPC_EINVAL;
        }
        if (d.kind == CMPC_ANN_COLOR ? (d.match < 1 || d.match > 3) : d.match != 0) {
            cmpc_set_error("%s: sample %d: %d channels to match (1..3 for a colour-coded annotation, 0 for a plain mask)", who, b, d.match);
            return CMPC_EINVAL;
        }
        e[b] = cmpc_eval_desc{d.offset, d.h, d.w, 1, d.rh, d.rw, d.top, d.left, 0};
        if (d.h > 0 && d.w > 0 && d.offset >= 0 && d.offset <= ann_bytes && (int64_t)d.h * d.w * d.c > ann_bytes - d.offset) {
            cmpc_set_error("%s: sample %d: offset %lld + %lld bytes beyond the buffer (%lld)", who, b, (long long)d.offset,
                           (long long)d.h * d.w * d.c, (long long)ann_bytes);
            return CMPC_EINVAL;
        }
    }
    const int rc = check_descs(who, e, B, ann_bytes, H, W, true, a.g);
    if (rc) return rc;
    if (order == 0)
        for (int b = 0; b < B; ++b) { a.g[b].sy = a.g[b].sx = 0.0; a.g[b].ry = a.g[b].rx = 0; }       // nearest sample: no Gaussian
    static const int shapes[][2] = {{8, 32}, {4, 32}, {2, 32}, {1, 32}, {1, 16}, {1, 8}, {1, 4}, {1, 1}};
    int ty = 0, tx = 0;
    lds = 0;
    for (auto& s : shapes) {
        lds = 0;
        for (int b = 0; b < B; ++b) lds = std::max(lds, tile_lds_bytes(tile_lds(a.g[b], s[0], s[1], ann_descs_host[b].h, ann_descs_host[b].w)));
        if (lds <= LDS_CAP) { ty = s[0]; tx = s[1]; break; }
    }
    if (!ty) { cmpc_set_error("%s: source footprint does not fit in LDS", who); return CMPC_EINVAL; }
    a.ann = ann; a.ann_bytes = ann_bytes;
    a.H = H; a.W = W; a.B = B; a.order = order; a.ty = ty; a.tx = tx;
    for (int b = 0; b < B; ++b) a.d[b] = ann_descs_host[b];
    return CMPC_OK;
}

// the planned annotations -> target_fine and pos: one memset and one train_target_kernel launch
int launch_target(const char* who, TrainArgs& a, size_t lds, float* target_fine, uint64_t* pos, hipStream_t stream) {
    a.target = target_fine; a.pos = (unsigned long long*)pos;
    if (hipMemsetAsync(pos, 0, sizeof(uint64_t) * a.B, stream) != hipSuccess) { cmpc_set_error("%s: hipMemsetAsync", who); return CMPC_EHIP; }
    hipLaunchKernelGGL(train_target_kernel, dim3((a.W + a.tx - 1) / a.tx, (a.H + a.ty - 1) / a.ty, a.B), dim3(NTHR), lds, stream, a);
    return cmpc_check_launch(who);
}

}  // namespace

extern "C" int cmpc_train_prep(const unsigned char* img, int64_t img_bytes, const cmpc_eval_desc* img_descs_host, const unsigned char* ann,
                               int64_t ann_bytes, const cmpc_train_desc* ann_descs_host, int B, int H, int W, int order,
                               unsigned char* proc_im, float* feed, float* target_fine, uint64_t* pos, void* stream) {
    if (!ann || !ann_descs_host || !target_fine || !pos) { cmpc_set_error("train_prep: NULL pointer"); return CMPC_EINVAL; }
    const bool images = img || img_descs_host || feed || proc_im;
    if (images && (!img || !img_descs_host || !feed)) { cmpc_set_error("train_prep: NULL pointer (img, img_descs and feed go together)"); return CMPC_EINVAL; }
    if (B <= 0 || B > CMPC_EVAL_MAX_BATCH) { cmpc_set_error("train_prep: B = %d outside 1..%d", B, CMPC_EVAL_MAX_BATCH); return CMPC_EINVAL; }
    if (H <= 0 || W <= 0 || ann_bytes <= 0 || (images && img_bytes <= 0)) { cmpc_set_error("train_prep: bad output size %d x %d or buffer length", H, W); return CMPC_EINVAL; }
    TrainArgs a;
    size_t lds = 0;
    int rc = plan_target("train_prep", ann, ann_bytes, ann_descs_host, B, H, W, order, a, lds);
    if (rc) return rc;
    if (images) {
        rc = launch_prep("train_prep", img, img_bytes, img_descs_host, B, H, W, proc_im, feed, ST);
        if (rc) return rc;
    }
    return launch_target("train_prep", a, lds, target_fine, pos, ST);
}

// One clip of the video model: n_img frames through cmpc_eval_prep's kernel and the key frame's annotation through cmpc_train_prep's
extern "C" int cmpc_clip_prep(const unsigned char* img, int64_t img_bytes, const cmpc_eval_desc* img_descs_host, int n_img,
                              const unsigned char* ann, int64_t ann_bytes, const cmpc_train_desc* ann_desc_host, int H, int W, int order,
                              float* feed, float* target_fine, uint64_t* pos, void* stream) {
    if (!img || !img_descs_host || !ann || !ann_desc_host || !feed || !target_fine || !pos) { cmpc_set_error("clip_prep: NULL pointer"); return CMPC_EINVAL; }
    if (n_img <= 0 || n_img > CMPC_TAPS_MAX_FRAMES) { cmpc_set_error("clip_prep: n_img = %d outside 1..%d", n_img, CMPC_TAPS_MAX_FRAMES); return CMPC_EINVAL; }
    if (H <= 0 || W <= 0 || ann_bytes <= 0 || img_bytes <= 0) { cmpc_set_error("clip_prep: bad output size %d x %d or buffer length", H, W); return CMPC_EINVAL; }
    TrainArgs a;
    size_t lds = 0;
    int rc = plan_target("clip_prep", ann, ann_bytes, ann_desc_host, 1, H, W, order, a, lds);
    if (rc) return rc;
    rc = launch_prep("clip_prep", img, img_bytes, img_descs_host, n_img, H, W, nullptr, feed, ST);
    if (rc) return rc;
    return launch_target("clip_prep", a, lds, target_fine, pos, ST);
}

extern "C" int cmpc_eval_mask_out(const void* map, int map_dt, int B, int H, int W, float thresh, const cmpc_eval_desc* descs_host,
                                  unsigned char* mask_out, int64_t out_bytes, int value, void* stream) {
    if (!map || !descs_host || !mask_out) { cmpc_set_error("eval_mask_out: NULL pointer"); return CMPC_EINVAL; }
    if (map_dt != CMPC_EVAL_F32 && map_dt != CMPC_EVAL_U8) { cmpc_set_error("eval_mask_out: map dtype %d is neither f32 nor u8", map_dt); return CMPC_EINVAL; }
    if (B <= 0 || B > CMPC_EVAL_MAX_BATCH) { cmpc_set_error("eval_mask_out: B = %d outside 1..%d", B, CMPC_EVAL_MAX_BATCH); return CMPC_EINVAL; }
    if (H <= 0 || W <= 0 || out_bytes <= 0) { cmpc_set_error("eval_mask_out: bad map size %d x %d or buffer length", H, W); return CMPC_EINVAL; }
    if (value != 1 && value != 255) { cmpc_set_error("eval_mask_out: value %d is neither 1 nor 255", value); return CMPC_EINVAL; }
    OutArgs a;
    const int rc = check_descs("eval_mask_out", descs_host, B, out_bytes, H, W, false, a.g);
    if (rc) return rc;
    a.map = map; a.H = H; a.W = W; a.thresh = thresh; a.out = mask_out; a.value = (uint32_t)value;
    int64_t most = 0;
    for (int b = 0; b < B; ++b) { a.d[b] = descs_host[b]; most = std::max(most, (int64_t)descs_host[b].h * descs_host[b].w); }
    const int per_sample = (int)std::max<int64_t>(1, std::min<int64_t>((most + 4 * NTHR - 1) / (4 * NTHR), 2048 / B));
    if (map_dt == CMPC_EVAL_F32) hipLaunchKernelGGL(eval_mask_out_kernel<float>, dim3(per_sample, B), dim3(NTHR), 0, ST, a);
    else hipLaunchKernelGGL(eval_mask_out_kernel<unsigned char>, dim3(per_sample, B), dim3(NTHR), 0, ST, a);
    return cmpc_check_launch("eval_mask_out");
}
