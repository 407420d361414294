// The pictures the reference's drivers draw from what the model computes, rendered where the tensors already are:
//
//   vis_overlay  the `-v` switch's pred.png / gt.png (trainval_model.py:306-330, CMPC_video/trainval_video.py):
//                  pred  (im / 2; [:, :, 0] += predicts.astype('uint8') * 100).astype('uint8')  ->  (im0 >> 1) + 100 m, im1 >> 1, im2 >> 1
//                  gt    (170 m, 0, 170 (1 - m))
//                with m = mask != 0: the package's "resampled value > 0" mask (evaluate.masks_out's docstring), not the driver's
//                .astype('uint8') of a fractional map.  A grey frame is tiled to three channels (build_batches.py:67-68).
//   vis_heat     one panel of test_visualize_fusion*.py (:283-304): resize_and_crop(sigmoid(map), h, w) through a colour map
//   vis_words    test_visualize_graph.py (:267-274): gw_v reshaped to (gh, gw, T), one panel per word
//
// vis_heat's value v is the float64 value of hostutil.resize_and_crop(s, h, w) for the float32 map s (or, with CMPC_VIS_SIGMOID,
// s = 1 / (1 + exp(-x)) evaluated in float32 in that order): eval_resample.h's restatement of SciPy, operation for operation (file-wide
// contract(off)), so v equals the host's bits except where the device's exp() rounds differently from NumPy's (the Gaussian weights of
// a shrinking axis, the sigmoid).  The colour index is
//     idx = clip(floor((v - lo) / (hi - lo) * 256), 0, 255)  in float64,  0 when hi == lo
// with (lo, hi) the caller's (vmin, vmax) or, with CMPC_VIS_AUTO, the min and max of v over the sample's h x w outputs (imshow's
// autoscale, per sample).  The min and max are integer atomics on an order-preserving encoding of the float64 bits: they do not depend on
// the order of the work, so reruns are bit-identical.  vis_words has no resampling arithmetic at all: its results are exact.
//
// Parity with matplotlib's own image pipeline is UNPINNED: imshow resamples the array to screen pixels and draws a figure around it;
// these kernels index the array's own pixels (tests/vis_ref.py repeats the rules in NumPy).
#include "cmpc_common.h"
#include "../../include/cmpc.h"
#include "eval_resample.h"

#pragma clang fp contract(off)

namespace {

constexpr int NTHR = 256;
constexpr int MB = CMPC_EVAL_MAX_BATCH;

// ---- overlay ------------------------------------------------------------------------------------------------------------------------
struct OverlaySample { int64_t fo, mo, oo; int h, w, c, pad_; };
struct OverlayArgs {
    const unsigned char* frames; const unsigned char* masks; unsigned char* out; int kind;
    OverlaySample s[MB];
};

// A sample is a flat stream of 3 h w output bytes, four per thread: byte k belongs to pixel k / 3, channel k % 3, so the four bytes touch
// two pixels.  One 32-bit frame load (three-channel frames: the same flat index) and one 32-bit store where the addresses are aligned.
__global__ __launch_bounds__(NTHR) void vis_overlay_kernel(OverlayArgs a) {
    const OverlaySample s = a.s[blockIdx.y];
    const int64_t npx = (int64_t)s.h * s.w, n = 3 * npx;
    const unsigned char* mk = a.masks + s.mo;
    const unsigned char* fr = a.kind == CMPC_VIS_PRED ? a.frames + s.fo : nullptr;
    unsigned char* out = a.out + s.oo;
    const bool al_o = ((uintptr_t)out & 3) == 0, al_f = fr && s.c == 3 && ((uintptr_t)fr & 3) == 0;
    for (int64_t i4 = ((int64_t)blockIdx.x * NTHR + threadIdx.x) * 4; i4 < n; i4 += (int64_t)gridDim.x * NTHR * 4) {
        const int k = (int)min((int64_t)4, n - i4);
        const int64_t px0 = i4 / 3;
        const int r0 = (int)(i4 - 3 * px0);
        const bool two = px0 + 1 < npx;
        const bool m0 = mk[px0] != 0, m1 = two && mk[px0 + 1] != 0;
        uint32_t fw = 0;
        if (fr) {
            if (s.c == 3) {
                if (k == 4 && al_f) fw = *(const uint32_t*)(fr + i4);
                else for (int j = 0; j < k; ++j) fw |= (uint32_t)fr[i4 + j] << (8 * j);
            } else {
                const uint32_t f0 = fr[px0], f1 = two ? fr[px0 + 1] : 0u;
                for (int j = 0; j < k; ++j) fw |= (r0 + j >= 3 ? f1 : f0) << (8 * j);
            }
        }
        uint32_t ov = 0;
        for (int j = 0; j < k; ++j) {
            const int t = r0 + j, p = t >= 3 ? 1 : 0, ch = t - 3 * p;
            const bool m = p ? m1 : m0;
            uint32_t v;
            if (a.kind == CMPC_VIS_PRED) v = (((fw >> (8 * j)) & 255u) >> 1) + (ch == 0 && m ? 100u : 0u);
            else v = ch == 0 ? (m ? 170u : 0u) : ch == 2 ? (m ? 0u : 170u) : 0u;
            ov |= v << (8 * j);
        }
        if (k == 4 && al_o) *(uint32_t*)(out + i4) = ov;
        else for (int j = 0; j < k; ++j) out[i4 + j] = (unsigned char)(ov >> (8 * j));
    }
}

// ---- heat ---------------------------------------------------------------------------------------------------------------------------
struct HeatArgs {
    const float* map; int H, W, flags; double vmin, vmax;
    const unsigned char* lut; unsigned char* idx; unsigned char* rgb; double* range; unsigned long long* mm;      // mm [B][2]: ~encoded min, encoded max (both grow from 0)
    cmpc_eval_desc d[MB];
    int64_t rgb_off[MB];
    SampleGeo g[MB];
};

// float64 bits <-> an unsigned integer with the same order (finite values)
__device__ __forceinline__ unsigned long long enc_f64(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double dec_f64(unsigned long long e) {
    const unsigned long long u = (e >> 63) ? (e & 0x7fffffffffffffffull) : ~e;
    return __longlong_as_double((long long)u);
}

__device__ __forceinline__ double heat_src(const float* m, int W, int y, int x, bool sig) {
    float v = m[(int64_t)y * W + x];
    if (sig) v = 1.0f / (1.0f + expf(-v));
    return (double)v;
}

// gaussian_filter's axis-0 pass at (y, x): correlate1d's symmetric form, mirrored rows
__device__ __forceinline__ double heat_vy(const float* m, int H, int W, const SampleGeo& g, const double* wy, int y, int x, bool sig) {
    if (!(g.sy > 0.0)) return heat_src(m, W, y, x, sig);
    double acc = heat_src(m, W, y, x, sig) * wy[0];
    for (int dd = g.ry; dd >= 1; --dd)
        acc = acc + (heat_src(m, W, mirror_idx(y - dd, H), x, sig) + heat_src(m, W, mirror_idx(y + dd, H), x, sig)) * wy[dd];
    return acc;
}

// the axis-1 pass on the axis-0 pass: the blurred map at (y, x), a plain window loop (shrinking is the rare direction)
__device__ __forceinline__ double heat_blur(const float* m, int H, int W, const SampleGeo& g, const double* wy, const double* wx, int y, int x, bool sig) {
    if (!(g.sx > 0.0)) return heat_vy(m, H, W, g, wy, y, x, sig);
    double v = heat_vy(m, H, W, g, wy, y, x, sig) * wx[0];
    for (int dd = g.rx; dd >= 1; --dd)
        v = v + (heat_vy(m, H, W, g, wy, y, mirror_idx(x - dd, W), sig) + heat_vy(m, H, W, g, wy, y, mirror_idx(x + dd, W), sig)) * wx[dd];
    return v;
}

// resize_and_crop's value at resized position (oy, ox): ndimage.zoom's four products ((v wy) wx) summed in row-major tap order
__device__ __forceinline__ double heat_value(const float* m, int H, int W, const SampleGeo& g, const double* wy, const double* wx, int oy, int ox, bool sig) {
    int y0, y1, x0, x1; double wy0, wy1, wx0, wx1;
    zoom_taps(oy, g.zy, H, y0, y1, wy0, wy1);
    zoom_taps(ox, g.zx, W, x0, x1, wx0, wx1);
    const int ys[2] = {y0, y1}, xs[2] = {x0, x1};
    const double wys[2] = {wy0, wy1}, wxs[2] = {wx0, wx1};
    double t = 0.0;
    for (int iy = 0; iy < 2; ++iy)
        for (int ix = 0; ix < 2; ++ix)
            t = t + (heat_blur(m, H, W, g, wy, wx, ys[iy], xs[ix], sig) * wys[iy]) * wxs[ix];
    return t;
}

__device__ __forceinline__ uint32_t heat_index(double v, double lo, double hi) {
    if (!(hi > lo)) return 0u;
    const double f = floor((v - lo) / (hi - lo) * 256.0);
    return (uint32_t)fmin(fmax(f, 0.0), 255.0);
}

// REDUCE: the sample's min and max of v into a.mm (CMPC_VIS_AUTO's first pass, nothing else written); else the index / RGB planes, four
// pixels per thread.  Both passes evaluate v by the same code, so the second pass meets exactly the values the first one ranked.
template <bool REDUCE>
__global__ __launch_bounds__(NTHR) void vis_heat_kernel(HeatArgs a) {
    __shared__ double wy[MAXR + 1], wx[MAXR + 1];
    __shared__ unsigned char slut[768];
    __shared__ unsigned long long smin[NTHR / 64], smax[NTHR / 64];
    const int b = blockIdx.y;
    const cmpc_eval_desc d = a.d[b];
    const SampleGeo g = a.g[b];
    const float* m = a.map + (int64_t)b * a.H * a.W;
    const bool sig = (a.flags & CMPC_VIS_SIGMOID) != 0;
    if (threadIdx.x == 0) {
        if (g.sy > 0.0) gauss_weights(g.sy, g.ry, wy);
        if (g.sx > 0.0) gauss_weights(g.sx, g.rx, wx);
    }
    if (!REDUCE && a.rgb)
        for (int i = threadIdx.x; i < 768; i += NTHR) slut[i] = a.lut[i];
    __syncthreads();
    const int64_t n = (int64_t)d.h * d.w;
    if (REDUCE) {
        unsigned long long lo = ~0ull, hi = 0ull;
        for (int64_t i = (int64_t)blockIdx.x * NTHR + threadIdx.x; i < n; i += (int64_t)gridDim.x * NTHR) {
            const int y = (int)(i / d.w), x = (int)(i - (int64_t)y * d.w);
            const unsigned long long e = enc_f64(heat_value(m, a.H, a.W, g, wy, wx, y + d.top, x + d.left, sig));
            lo = min(lo, e); hi = max(hi, e);
        }
        for (int off = 32; off > 0; off >>= 1) { lo = min(lo, __shfl_down(lo, off, 64)); hi = max(hi, __shfl_down(hi, off, 64)); }
        if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 1; i < NTHR / 64; ++i) { lo = min(lo, smin[i]); hi = max(hi, smax[i]); }
            if (lo <= hi) { atomicMax(&a.mm[2 * b], ~lo); atomicMax(&a.mm[2 * b + 1], hi); }      // a block without pixels has lo > hi
        }
        return;
    }
    double lo = a.vmin, hi = a.vmax;
    if (a.flags & CMPC_VIS_AUTO) { lo = dec_f64(~a.mm[2 * b]); hi = dec_f64(a.mm[2 * b + 1]); }
    if (a.range && blockIdx.x == 0 && threadIdx.x == 0) { a.range[2 * b] = lo; a.range[2 * b + 1] = hi; }
    unsigned char* io = a.idx ? a.idx + d.offset : nullptr;
    unsigned char* ro = a.rgb ? a.rgb + a.rgb_off[b] : nullptr;
    const bool al_i = ((uintptr_t)io & 3) == 0, al_r = ((uintptr_t)ro & 3) == 0;
    for (int64_t i4 = ((int64_t)blockIdx.x * NTHR + threadIdx.x) * 4; i4 < n; i4 += (int64_t)gridDim.x * NTHR * 4) {
        const int k = (int)min((int64_t)4, n - i4);
        uint32_t q[4] = {0, 0, 0, 0};
        for (int j = 0; j < k; ++j) {
            const int64_t i = i4 + j;
            const int y = (int)(i / d.w), x = (int)(i - (int64_t)y * d.w);
            q[j] = heat_index(heat_value(m, a.H, a.W, g, wy, wx, y + d.top, x + d.left, sig), lo, hi);
        }
        if (io) {
            if (k == 4 && al_i) *(uint32_t*)(io + i4) = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
            else for (int j = 0; j < k; ++j) io[i4 + j] = (unsigned char)q[j];
        }
        if (ro) {
            unsigned char px[12];
            for (int j = 0; j < 4; ++j)
                for (int c = 0; c < 3; ++c) px[3 * j + c] = slut[3 * q[j] + c];
            unsigned char* o = ro + 3 * i4;
            if (k == 4 && al_r) {
                for (int wd = 0; wd < 3; ++wd)
                    ((uint32_t*)o)[wd] = (uint32_t)px[4 * wd] | (uint32_t)px[4 * wd + 1] << 8 | (uint32_t)px[4 * wd + 2] << 16 | (uint32_t)px[4 * wd + 3] << 24;
            } else {
                for (int j = 0; j < 3 * k; ++j) o[j] = px[j];
            }
        }
    }
}

// ---- words --------------------------------------------------------------------------------------------------------------------------
struct WordsArgs {
    const float* gw; int gh, gwd, ld, zoom, cols, gap, rows, sh, sw;
    const unsigned char* lut; unsigned char* out;
    int nw[MB];
};

// One workgroup per cell of the sheet: panel t = row * cols + col with the gap to its right and below it.  The panel's own min and max
// (float32, widened to float64 for the index rule), then one thread per sheet pixel of the cell.
__global__ __launch_bounds__(NTHR) void vis_words_kernel(WordsArgs a) {
    __shared__ float rmin[NTHR / 64], rmax[NTHR / 64];
    const int b = blockIdx.y, t = blockIdx.x;
    const int r = t / a.cols, c = t - r * a.cols;
    const int N = a.gh * a.gwd, ph = a.gh * a.zoom, pw = a.gwd * a.zoom;
    const int y0 = r * (ph + a.gap), x0 = c * (pw + a.gap);
    const int ch = ph + (r < a.rows - 1 ? a.gap : 0), cw = pw + (c < a.cols - 1 ? a.gap : 0);
    const bool active = t < a.nw[b];                                     // uniform over the workgroup
    const float* col = a.gw + (int64_t)b * N * a.ld + t;
    double lo = 0.0, hi = 0.0;
    if (active) {
        float mn = col[0], mx = col[0];
        for (int i = threadIdx.x; i < N; i += NTHR) { const float v = col[(int64_t)i * a.ld]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
        for (int off = 32; off > 0; off >>= 1) { mn = fminf(mn, __shfl_xor(mn, off, 64)); mx = fmaxf(mx, __shfl_xor(mx, off, 64)); }
        if ((threadIdx.x & 63) == 0) { rmin[threadIdx.x >> 6] = mn; rmax[threadIdx.x >> 6] = mx; }
        __syncthreads();
        lo = (double)fminf(fminf(rmin[0], rmin[1]), fminf(rmin[2], rmin[3]));
        hi = (double)fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3]));
    }
    unsigned char* out = a.out + (int64_t)b * a.sh * a.sw * 3;
    for (int p = threadIdx.x; p < ch * cw; p += NTHR) {
        const int yy = p / cw, xx = p - yy * cw;
        uint32_t c0 = 255, c1 = 255, c2 = 255;
        if (active && yy < ph && xx < pw) {
            const int i = (yy / a.zoom) * a.gwd + xx / a.zoom;
            const uint32_t q = heat_index((double)col[(int64_t)i * a.ld], lo, hi);
            c0 = a.lut[3 * q]; c1 = a.lut[3 * q + 1]; c2 = a.lut[3 * q + 2];
        }
        unsigned char* o = out + ((int64_t)(y0 + yy) * a.sw + x0 + xx) * 3;
        o[0] = (unsigned char)c0; o[1] = (unsigned char)c1; o[2] = (unsigned char)c2;
    }
}

// a packed [h, w, c] sample inside its buffer
bool inside(const cmpc_eval_desc& d, int c, int64_t bytes) {
    return d.offset >= 0 && d.offset <= bytes && (int64_t)d.h * d.w * c <= bytes - d.offset;
}

int grid_x(int64_t most_items, int B) {       // four items per thread, ~2048 workgroups per launch
    return (int)std::max<int64_t>(1, std::min<int64_t>((most_items + 4 * NTHR - 1) / (4 * NTHR), 2048 / B));
}

}  // namespace

#define ST ((hipStream_t)stream)
#define VIS_B(who)                                                                                                                   \
    if (B <= 0 || B > CMPC_EVAL_MAX_BATCH) { cmpc_set_error(who ": B = %d outside 1..%d", B, CMPC_EVAL_MAX_BATCH); return CMPC_EINVAL; }

extern "C" int cmpc_vis_overlay(int kind, const unsigned char* frames, int64_t frame_bytes, const cmpc_eval_desc* frame_descs_host,
                                const unsigned char* masks, int64_t mask_bytes, const cmpc_eval_desc* mask_descs_host, int B,
                                unsigned char* out, int64_t out_bytes, const cmpc_eval_desc* out_descs_host, void* stream) {
    if (kind != CMPC_VIS_PRED && kind != CMPC_VIS_GT) { cmpc_set_error("vis_overlay: kind %d is neither CMPC_VIS_PRED nor CMPC_VIS_GT", kind); return CMPC_EINVAL; }
    if (!masks || !mask_descs_host || !out || !out_descs_host || (kind == CMPC_VIS_PRED && (!frames || !frame_descs_host))) {
        cmpc_set_error("vis_overlay: NULL pointer");
        return CMPC_EINVAL;
    }
    VIS_B("vis_overlay")
    OverlayArgs a;
    a.frames = frames; a.masks = masks; a.out = out; a.kind = kind;
    int64_t most = 0;
    for (int b = 0; b < B; ++b) {
        const cmpc_eval_desc& dm = mask_descs_host[b];
        const cmpc_eval_desc& dout = out_descs_host[b];
        if (dm.h <= 0 || dm.w <= 0) { cmpc_set_error("vis_overlay: sample %d: empty mask (%d x %d)", b, dm.h, dm.w); return CMPC_EINVAL; }
        if (dout.h != dm.h || dout.w != dm.w) {
            cmpc_set_error("vis_overlay: sample %d: output %d x %d, mask %d x %d: the sizes differ", b, dout.h, dout.w, dm.h, dm.w);
            return CMPC_EINVAL;
        }
        OverlaySample s{0, dm.offset, dout.offset, dm.h, dm.w, 3, 0};
        if (kind == CMPC_VIS_PRED) {
            const cmpc_eval_desc& df = frame_descs_host[b];
            if (df.h != dm.h || df.w != dm.w) {
                cmpc_set_error("vis_overlay: sample %d: frame %d x %d, mask %d x %d: the sizes differ", b, df.h, df.w, dm.h, dm.w);
                return CMPC_EINVAL;
            }
            if (df.c != 1 && df.c != 3) { cmpc_set_error("vis_overlay: sample %d: %d channels (1 or 3)", b, df.c); return CMPC_EINVAL; }
            if (!inside(df, df.c, frame_bytes)) {
                cmpc_set_error("vis_overlay: sample %d: frame at offset %lld + %lld bytes beyond the buffer (%lld)", b, (long long)df.offset,
                               (long long)df.h * df.w * df.c, (long long)frame_bytes);
                return CMPC_EINVAL;
            }
            s.fo = df.offset; s.c = df.c;
        }
        if (!inside(dm, 1, mask_bytes)) {
            cmpc_set_error("vis_overlay: sample %d: mask at offset %lld + %lld bytes beyond the buffer (%lld)", b, (long long)dm.offset,
                           (long long)dm.h * dm.w, (long long)mask_bytes);
            return CMPC_EINVAL;
        }
        if (!inside(dout, 3, out_bytes)) {
            cmpc_set_error("vis_overlay: sample %d: output at offset %lld + %lld bytes beyond the buffer (%lld)", b, (long long)dout.offset,
                           (long long)dout.h * dout.w * 3, (long long)out_bytes);
            return CMPC_EINVAL;
        }
        a.s[b] = s;
        most = std::max(most, (int64_t)3 * dm.h * dm.w);
    }
    hipLaunchKernelGGL(vis_overlay_kernel, dim3(grid_x(most, B), B), dim3(NTHR), 0, ST, a);
    return cmpc_check_launch("vis_overlay");
}

extern "C" int cmpc_vis_heat_workspace(int B, int flags, int64_t* bytes) {
    if (!bytes) { cmpc_set_error("vis_heat_workspace: NULL pointer"); return CMPC_EINVAL; }
    VIS_B("vis_heat_workspace")
    if (flags & ~(CMPC_VIS_SIGMOID | CMPC_VIS_AUTO)) { cmpc_set_error("vis_heat_workspace: unknown flags %d", flags); return CMPC_EINVAL; }
    *bytes = (flags & CMPC_VIS_AUTO) ? (int64_t)sizeof(uint64_t) * 2 * B : 0;
    return CMPC_OK;
}

extern "C" int cmpc_vis_heat(const float* map, int B, int H, int W, const cmpc_eval_desc* descs_host, int flags, double vmin, double vmax,
                             const unsigned char* lut, unsigned char* idx_out, int64_t idx_bytes, unsigned char* rgb_out, int64_t rgb_bytes,
                             const cmpc_eval_desc* rgb_descs_host, double* range_out, void* ws, int64_t ws_bytes, void* stream) {
    if (!map || !descs_host) { cmpc_set_error("vis_heat: NULL pointer"); return CMPC_EINVAL; }
    if (!idx_out && !rgb_out) { cmpc_set_error("vis_heat: NULL pointer (neither an index plane nor an RGB plane to write)"); return CMPC_EINVAL; }
    VIS_B("vis_heat")
    if (H <= 0 || W <= 0) { cmpc_set_error("vis_heat: bad map size %d x %d", H, W); return CMPC_EINVAL; }
    if (flags & ~(CMPC_VIS_SIGMOID | CMPC_VIS_AUTO)) { cmpc_set_error("vis_heat: unknown flags %d", flags); return CMPC_EINVAL; }
    const bool autor = (flags & CMPC_VIS_AUTO) != 0;
    if (!autor && !(vmin < vmax)) { cmpc_set_error("vis_heat: vmin %g is not below vmax %g", vmin, vmax); return CMPC_EINVAL; }
    if (rgb_out && !lut) { cmpc_set_error("vis_heat: an RGB plane needs a LUT (lut is NULL)"); return CMPC_EINVAL; }
    if (rgb_out && !rgb_descs_host) { cmpc_set_error("vis_heat: NULL pointer (an RGB plane needs its descriptors)"); return CMPC_EINVAL; }
    if ((uintptr_t)range_out & 7) { cmpc_set_error("vis_heat: range_out is not 8-byte aligned"); return CMPC_EINVAL; }
    HeatArgs a;
    int64_t most = 0;
    for (int b = 0; b < B; ++b) {
        const cmpc_eval_desc& d = descs_host[b];
        if (d.h <= 0 || d.w <= 0) { cmpc_set_error("vis_heat: sample %d: empty output (%d x %d)", b, d.h, d.w); return CMPC_EINVAL; }
        int gm[4];
        geometry(H, W, d.h, d.w, false, gm);
        if (gm[0] != d.rh || gm[1] != d.rw || gm[2] != d.top || gm[3] != d.left || d.rh <= 0 || d.rw <= 0) {
            cmpc_set_error("vis_heat: sample %d: geometry (%d, %d, %d, %d) differs from resize_and_crop_geometry (%d, %d, %d, %d)", b, d.rh, d.rw,
                           d.top, d.left, gm[0], gm[1], gm[2], gm[3]);
            return CMPC_EINVAL;
        }
        if (!sample_geo(H, W, d.rh, d.rw, a.g[b])) {
            cmpc_set_error("vis_heat: sample %d: shrink factor too large (Gaussian radius > %d)", b, MAXR);
            return CMPC_EINVAL;
        }
        if (idx_out && !inside(d, 1, idx_bytes)) {
            cmpc_set_error("vis_heat: sample %d: index plane at offset %lld + %lld bytes beyond the buffer (%lld)", b, (long long)d.offset,
                           (long long)d.h * d.w, (long long)idx_bytes);
            return CMPC_EINVAL;
        }
        a.rgb_off[b] = 0;
        if (rgb_out) {
            const cmpc_eval_desc& r = rgb_descs_host[b];
            if (r.h != d.h || r.w != d.w) {
                cmpc_set_error("vis_heat: sample %d: RGB plane %d x %d, output %d x %d: the sizes differ", b, r.h, r.w, d.h, d.w);
                return CMPC_EINVAL;
            }
            if (!inside(r, 3, rgb_bytes)) {
                cmpc_set_error("vis_heat: sample %d: RGB plane at offset %lld + %lld bytes beyond the buffer (%lld)", b, (long long)r.offset,
                               (long long)r.h * r.w * 3, (long long)rgb_bytes);
                return CMPC_EINVAL;
            }
            a.rgb_off[b] = r.offset;
        }
        a.d[b] = d;
        most = std::max(most, (int64_t)d.h * d.w);
    }
    if (autor) {
        const int64_t need = (int64_t)sizeof(uint64_t) * 2 * B;
        if (!ws || ws_bytes < need) { cmpc_set_error("vis_heat: workspace of %lld bytes, CMPC_VIS_AUTO needs %lld", (long long)(ws ? ws_bytes : 0), (long long)need); return CMPC_EINVAL; }
        if ((uintptr_t)ws & 7) { cmpc_set_error("vis_heat: the workspace is not 8-byte aligned"); return CMPC_EINVAL; }
    }
    a.map = map; a.H = H; a.W = W; a.flags = flags; a.vmin = vmin; a.vmax = vmax;
    a.lut = lut; a.idx = idx_out; a.rgb = rgb_out; a.range = range_out; a.mm = (unsigned long long*)ws;
    if (autor) {
        if (hipMemsetAsync(ws, 0, sizeof(uint64_t) * 2 * B, ST) != hipSuccess) { cmpc_set_error("vis_heat: hipMemsetAsync"); return CMPC_EHIP; }
        const int gx = (int)std::max<int64_t>(1, std::min<int64_t>((most + NTHR - 1) / NTHR, 2048 / B));
        hipLaunchKernelGGL(vis_heat_kernel<true>, dim3(gx, B), dim3(NTHR), 0, ST, a);
        const int rc = cmpc_check_launch("vis_heat");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(vis_heat_kernel<false>, dim3(grid_x(most, B), B), dim3(NTHR), 0, ST, a);
    return cmpc_check_launch("vis_heat");
}

extern "C" int cmpc_vis_words(const float* gw, int B, int gh, int gwd, int ld, const int* n_words_host, int max_words, int zoom, int cols,
                              int gap, const unsigned char* lut, unsigned char* out, int64_t out_bytes, void* stream) {
    if (!gw || !n_words_host || !lut || !out) { cmpc_set_error("vis_words: NULL pointer"); return CMPC_EINVAL; }
    VIS_B("vis_words")
    if (gh <= 0 || gwd <= 0 || ld <= 0) { cmpc_set_error("vis_words: bad grid %d x %d or leading dimension %d", gh, gwd, ld); return CMPC_EINVAL; }
    if (max_words < 1 || max_words > 32) { cmpc_set_error("vis_words: max_words = %d outside 1..32", max_words); return CMPC_EINVAL; }
    if (zoom < 1 || cols < 1 || gap < 0) { cmpc_set_error("vis_words: zoom %d < 1, cols %d < 1 or gap %d < 0", zoom, cols, gap); return CMPC_EINVAL; }
    WordsArgs a;
    for (int b = 0; b < B; ++b) {
        const int n = n_words_host[b];
        if (n < 0 || n > ld || n > max_words) {
            cmpc_set_error("vis_words: sample %d: n_words = %d outside 0..min(ld = %d, max_words = %d)", b, n, ld, max_words);
            return CMPC_EINVAL;
        }
        a.nw[b] = n;
    }
    const int rows = (max_words + cols - 1) / cols;
    const int64_t sh = (int64_t)rows * gh * zoom + (int64_t)(rows - 1) * gap, sw = (int64_t)cols * gwd * zoom + (int64_t)(cols - 1) * gap;
    if (sh > (1 << 15) || sw > (1 << 15) || (int64_t)gh * gwd > (1 << 24)) { cmpc_set_error("vis_words: a sheet of %lld x %lld pixels is too large", (long long)sh, (long long)sw); return CMPC_EINVAL; }
    if (out_bytes < (int64_t)B * sh * sw * 3) {
        cmpc_set_error("vis_words: %d sheets of %lld x %lld x 3 bytes beyond the buffer (%lld)", B, (long long)sh, (long long)sw, (long long)out_bytes);
        return CMPC_EINVAL;
    }
    a.gw = gw; a.gh = gh; a.gwd = gwd; a.ld = ld; a.zoom = zoom; a.cols = cols; a.gap = gap; a.rows = rows; a.sh = (int)sh; a.sw = (int)sw;
    a.lut = lut; a.out = out;
    hipLaunchKernelGGL(vis_words_kernel, dim3(rows * cols, B), dim3(NTHR), 0, ST, a);
    return cmpc_check_launch("vis_words");
}
