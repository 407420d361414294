// Training accuracy of the reference's train loops (test.py:94-127, CMPC_video/trainval_video.py:93-123) on the device:
//
//   train_accuracy   per sample {n_pos, n_neg, correct_pos, correct_neg} of compute_accuracy(pred, target)
//                    (util/processing_tools.py:24-35) with target = tf.image.resize_bilinear(target_fine, [h, w])
//                    (model.target: CMPC_model.py:439, CMPC_video_mm_tgraph_allvec.py:567)
//
// The resize is the legacy one (align_corners=False, no half-pixel centres) as oracle/cmpc_torch.py:resize_bilinear states it:
// src = dst * (in / out) in float32, lo = floor(src), hi = min(lo + 1, in - 1), weight src - floor(src); lerp a + (b - a) * t along x,
// then along y, every operation rounded to float32 (file-wide contract(off): no fused multiply-adds).  lo is taken from the float32
// product, as TensorFlow's kernel takes it; the oracle floors the float64 product, which is the same index unless dst * (in / out)
// rounds to just below an integer in float32 (e.g. 26 -> 22; never for an integer or dyadic scale such as 320 -> 40).  Only `target != 0` is used,
// but a lerp of {0, 1} taps can cancel to exactly 0 only through that arithmetic, so it is repeated rather than replaced by an OR.
// The counts are integers: reruns are bit-identical and a sample's counts do not depend on the batch around it.
#include "cmpc_common.h"
#include "../../include/cmpc.h"

#pragma clang fp contract(off)

namespace {

constexpr int NTHR = 256;
constexpr int NWAVE = NTHR / 64;

// one workgroup per sample: every thread walks a strided set of the h * w coarse pixels, reading its (at most 4) taps of target_fine
__global__ __launch_bounds__(NTHR) void train_accuracy_kernel(const float* __restrict__ pred, const float* __restrict__ fine, int h, int w,
                                                              int H, int W, float sy, float sx, unsigned long long* __restrict__ counts) {
    const int b = blockIdx.x;
    const float* p = pred + (int64_t)b * h * w;
    const float* f = fine + (int64_t)b * H * W;
    const int n = h * w;
    const bool same = h == H && w == W;              // the identity resize: target = target_fine
    unsigned int npos = 0, cpos = 0, cneg = 0;       // per thread at most n / NTHR + 1 each
    for (int i = threadIdx.x; i < n; i += NTHR) {
        float t;
        if (same) {
            t = f[i];
        } else {
            const int y = i / w, x = i - y * w;
            const float fy = (float)y * sy, fx = (float)x * sx;
            const float y0f = floorf(fy), x0f = floorf(fx);
            const int y0 = min((int)y0f, H - 1), x0 = min((int)x0f, W - 1);        // in range already: h <= H, w <= W
            const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
            const float ty = fy - y0f, tx = fx - x0f;
            const float* r0 = f + (int64_t)y0 * W;
            const float* r1 = f + (int64_t)y1 * W;
            const float a = r0[x0], c = r1[x0];
            const float top = a + (r0[x1] - a) * tx;
            const float bot = c + (r1[x1] - c) * tx;
            t = top + (bot - top) * ty;
        }
        const bool pos = t != 0.0f;
        const bool correct = (p[i] < 0.0f) != pos;   // 0.0, -0.0 and NaN are not < 0: predicted positive
        npos += pos;
        cpos += correct && pos;
        cneg += correct && !pos;
    }
    // integer wave sums (each at most n < 2^31), then LDS across the waves
    for (int off = 32; off > 0; off >>= 1) {
        npos += __shfl_down(npos, off, 64);
        cpos += __shfl_down(cpos, off, 64);
        cneg += __shfl_down(cneg, off, 64);
    }
    __shared__ unsigned int s[NWAVE][3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s[wave][0] = npos; s[wave][1] = cpos; s[wave][2] = cneg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tp = 0, cp = 0, cn = 0;
        for (int k = 0; k < NWAVE; ++k) { tp += s[k][0]; cp += s[k][1]; cn += s[k][2]; }
        unsigned long long* o = counts + 4 * (int64_t)b;
        o[0] = tp; o[1] = (unsigned long long)n - tp; o[2] = cp; o[3] = cn;
    }
}

}  // namespace

extern "C" int cmpc_train_accuracy(const float* pred, const float* target_fine, int B, int h, int w, int H, int W, uint64_t* counts,
                                   void* stream) {
    if (!pred || !target_fine || !counts) { cmpc_set_error("train_accuracy: NULL pointer"); return CMPC_EINVAL; }
    if (B <= 0 || B > CMPC_EVAL_MAX_BATCH) { cmpc_set_error("train_accuracy: B = %d outside 1..%d", B, CMPC_EVAL_MAX_BATCH); return CMPC_EINVAL; }
    if (h <= 0 || w <= 0 || H <= 0 || W <= 0) { cmpc_set_error("train_accuracy: bad size %d x %d from %d x %d", h, w, H, W); return CMPC_EINVAL; }
    if (h > H || w > W) { cmpc_set_error("train_accuracy: pred %d x %d is larger than target_fine %d x %d", h, w, H, W); return CMPC_EINVAL; }
    if ((int64_t)H * W > 0x7fffffffLL) { cmpc_set_error("train_accuracy: %d x %d pixels exceed 2^31 - 1", H, W); return CMPC_EINVAL; }
    // the scale in / out, rounded to float32 as the oracle rounds it (np.float32 of the float64 quotient)
    const float sy = (float)((double)H / (double)h), sx = (float)((double)W / (double)w);
    hipLaunchKernelGGL(train_accuracy_kernel, dim3(B), dim3(NTHR), 0, (hipStream_t)stream, pred, target_fine, h, w, H, W, sy, sx,
                       (unsigned long long*)counts);
    return cmpc_check_launch("train_accuracy");
}
