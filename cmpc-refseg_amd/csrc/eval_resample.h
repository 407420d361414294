// The resampler's arithmetic shared by ops_eval.hip and ops_vis.hip: skimage.transform.resize as cmpc-refseg_amd/hostutil.py restates it on
// scipy.ndimage (a mirror-mode Gaussian on every shrinking axis, then ndimage.zoom(order=1, mode="mirror", grid_mode=True)).  Every
// including file is compiled with `#pragma clang fp contract(off)` from here on: these functions repeat SciPy's float64 operations one for
// one, and a fused multiply-add would round differently.
#pragma once
#include "cmpc_common.h"
#include "../../include/cmpc.h"

#pragma clang fp contract(off)

namespace {

// Gaussian radius limit: int(4 sigma + 0.5) <= 63, i.e. shrink factors below 32.75 per axis.  Grey images and masks go that far; a colour
// source is refused earlier, by eval_prep's LDS footprint (at radii 63 / 63 even the 1 x 1 tile needs ~70 KB): 720 x 1280 x 3 into 23 x 41
// (radii 61 / 60) is refused, the same source in grey is not, and a square colour source fits up to radius 59 there
// (tests/test_gpu_resample_edges.py).
constexpr int MAXR = 63;

struct SampleGeo {                       // host-derived per-sample constants (passed by value)
    double zy, zx;                       // source / resized, float64 (ndimage.zoom's factors)
    double sy, sx;                       // Gaussian sigmas (0: axis not blurred)
    int ry, rx;                          // radii
};

__device__ __forceinline__ int mirror_idx(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i = abs(i) % p;
    return i >= n ? p - i : i;
}

// SciPy's zoom source coordinate for output index o (grid_mode, mirror): taps i0, i1 and weights w0 = 1 - t, w1 = 1 - (1 - t)
__device__ __forceinline__ void zoom_taps(int o, double z, int n, int& i0, int& i1, double& w0, double& w1) {
    double cc = ((double)o + 0.5) * z - 0.5;
    if (n == 1) cc = 0.0;
    else if (cc < 0.0) cc = -cc;
    const double f = floor(cc);
    const double t = cc - f;
    w0 = 1.0 - t;
    w1 = 1.0 - w0;
    i0 = mirror_idx((int)f, n);
    i1 = mirror_idx((int)f + 1, n);
}

// _gaussian_kernel1d(sigma, 0, r) normalised by NumPy's pairwise sum; w[d] for d = 0..r (symmetric)
__device__ void gauss_weights(double sigma, int r, double* w) {
    double phi[2 * MAXR + 1];
    const int n = 2 * r + 1;
    const double a = -0.5 / (sigma * sigma);
    for (int i = 0; i < n; ++i) { const double x = (double)((i - r) * (i - r)); phi[i] = exp(a * x); }
    double s;
    if (n < 8) {
        s = 0.0;
        for (int i = 0; i < n; ++i) s += phi[i];
    } else {
        double p[8];
        for (int j = 0; j < 8; ++j) p[j] = phi[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) p[j] += phi[i + j];
        s = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
        for (; i < n; ++i) s += phi[i];
    }
    for (int d = 0; d <= r; ++d) w[d] = phi[r + d] / s;
}

// resize_and_pad_geometry / resize_and_crop_geometry (hostutil.py): Python's true division, np.round (half to even), int(floor(.) / 2)
void geometry(int ih, int iw, int oh, int ow, bool pad, int out[4]) {
    const double s = pad ? fmin((double)oh / ih, (double)ow / iw) : fmax((double)oh / ih, (double)ow / iw);
    const int rh = (int)nearbyint(ih * s), rw = (int)nearbyint(iw * s);
    out[0] = rh; out[1] = rw;
    out[2] = (int)((double)(pad ? oh - rh : rh - oh) / 2.0);
    out[3] = (int)((double)(pad ? ow - rw : rw - ow) / 2.0);
}

// skimage_like_resize's Gaussian and zoom constants for src -> dst
bool sample_geo(int sh, int sw, int dh, int dw, SampleGeo& g) {
    g.zy = (double)sh / dh; g.zx = (double)sw / dw;
    g.sy = g.sx = 0.0; g.ry = g.rx = 0;
    if (fmax(g.zy, g.zx) > 1.0) {
        const double sy = fmax(0.0, (g.zy - 1.0) / 2.0), sx = fmax(0.0, (g.zx - 1.0) / 2.0);
        if (sy > 1e-15) { g.sy = sy; g.ry = (int)(4.0 * sy + 0.5); }         // gaussian_filter skips sigma <= 1e-15
        if (sx > 1e-15) { g.sx = sx; g.rx = (int)(4.0 * sx + 0.5); }
    }
    return g.ry <= MAXR && g.rx <= MAXR;
}

}  // namespace
