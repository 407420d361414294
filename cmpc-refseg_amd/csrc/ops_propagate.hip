// Mask propagation from pivot frames (the step the reference's find_pivot_frames was written for, test.py:150-181, and never got):
// a non-pivot frame receives the labels of its pivot frame(s) along dense correspondences between backbone taps.
//
//   label_propagate   a_q = f_q * rsqrt(max(sum f_q^2, 1e-12)), b_p likewise, c = <a_q, b_p> over the candidates (s, p) of the item's
//                     sources with |y' - y| <= radius and |x' - x| <= radius, w = softmax(c / temperature) over all of them,
//                     out[q] = sum w * label_s[p], peak[q] = max c
//   prop_fuse         fused = (1 - alpha) * own + alpha * U(prop), U the legacy bilinear rule that makes `up` from `pred` (ops_score.hip)
//
// label_propagate is two kernels.  norm_kernel writes the inverse norms of the target tap and of every source tap of every item into
// the workspace, [n][1 + CMPC_PROP_MAX_SOURCES][h * w] floats: a wave per position, lanes over groups of 8 channels, one butterfly.
// prop_kernel gives a workgroup of 4 waves the 16 target positions (y, x0 .. x0 + 15) of one item.  Its work is a list of units
// (source s, candidate row y', tile of 16 candidate columns) in that order, rows y - r .. y + r and columns x0 - r .. x0 + 15 + r
// clipped to the grid; wave k takes units k, k + 4, ...  A unit is one 16 x 16 x C product on the MFMA unit: A = the 16 candidates
// (rows), B = the 16 targets (columns), so that lane (g, q) = (lane >> 4, lane & 15) ends with the four scores of target q against
// candidates 4 g .. 4 g + 3 and runs its own online softmax over them -- no cross-lane traffic inside the loop.  The candidates'
// rows stream through a wave-private LDS stage in chunks of 256 bytes per row (the next chunk's global loads are in flight while the
// current one is multiplied); the target tile stays resident in LDS when it fits 32 KB (C <= 1024 for the 16-bit types) and streams
// beside the candidates otherwise.  Both images are swizzled (16-byte slot ^ row) so that the fragment reads of 16 rows hit 16
// distinct slots.  The byte image serves v_mfma_f32_16x16x32_{bf16,f16} and, four steps per 16 bytes, v_mfma_f32_16x16x4_f32, as in
// gemm.hip.  Columns outside a target's own window (and the tails of the tiles) are masked before the softmax.  At the end the 16
// partial states of a target (4 waves x 4 lane groups) are merged in a fixed order by one thread.  No floating-point atomics, nothing
// depends on which workgroup runs first: reruns are bit-identical, and an item's result does not depend on the items beside it
// (its inverse norms are its own rows of the workspace).  Every loop is bounded by the shapes.
#include "cmpc_common.h"
#include "../../include/cmpc.h"
#include <math.h>

namespace {

constexpr int NTHR = 256;
constexpr int NWAVE = NTHR / 64;
constexpr int TQ = 16;                           // target positions per workgroup = candidates per unit: one MFMA tile
constexpr int CHB = 256;                         // bytes of a row per LDS chunk: 16 slots of 16 bytes, 4 MFMA steps
constexpr int STAGE = TQ * CHB;                  // bytes of one wave-private stage
constexpr int RES_MAX = 32 * 1024;               // the target tile stays in LDS up to this many bytes
constexpr int NSLOT = 1 + CMPC_PROP_MAX_SOURCES; // rows of inverse norms per item: the target, then the sources

template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
    static __device__ __forceinline__ f4 run(const uint4& a, const uint4& b, f4 acc) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8v, a), __builtin_bit_cast(bf8v, b), acc, 0, 0, 0);
    }
};
template <> struct Mma<f16_t> {
    static __device__ __forceinline__ f4 run(const uint4& a, const uint4& b, f4 acc) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8v, a), __builtin_bit_cast(h8v, b), acc, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    static __device__ __forceinline__ f4 run(const uint4& a, const uint4& b, f4 acc) {
        // a lane's 16 bytes are four k-values: step e pairs element e of both operands (gemm.hip)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
        return acc;
    }
};

struct PropArgs {
    const void* feat; int64_t stride;            // elements between frames
    const float* labels;
    float* out; float* peak; float* inv;         // inv: [n][NSLOT][h * w]
    int h, w, C, r;                              // r: 0 .. max(h, w)
    float temperature;
    int pitch;                                   // bytes of a row rounded up to CHB
    cmpc_prop_item it[CMPC_EVAL_MAX_BATCH];
};

// slot ^ row inside each 256-byte chunk: 16 rows reading one logical slot touch 16 distinct 16-byte slots
__device__ __forceinline__ int swz(int row, int slot) { return (slot ^ (row & 15)) << 4; }

// The stages are wave-private, so no workgroup barrier is needed between a wave's stores and its own lanes' reads of them; this
// states the order the code relies on: LDS accesses before it complete (workgroup-scope fence) and the compiler moves none across it.
__device__ __forceinline__ void stage_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <typename T>
__global__ __launch_bounds__(NTHR) void norm_kernel(PropArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.z, slot = blockIdx.y;
    const int hw = a.h * a.w;
    const int pos = blockIdx.x * NWAVE + wave;
    if (slot > a.it[i].nsrc || pos >= hw) return;
    const int frame = slot == 0 ? a.it[i].tgt : a.it[i].src[slot - 1];
    const T* f = (const T*)a.feat + (int64_t)frame * a.stride + (int64_t)pos * a.C;
    float s = 0.f;
    for (int g = lane; g < a.C / 8; g += 64) {
        float v[8];
        ld8<T>(f + (int64_t)g * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[e] * v[e];
    }
    s = wave_sum(s);
    if (lane == 0) a.inv[((int64_t)i * NSLOT + slot) * hw + pos] = 1.0f / sqrtf(fmaxf(s, 1e-12f));
}

template <typename T, bool RES>
__global__ __launch_bounds__(NTHR) void prop_kernel(PropArgs a) {
    extern __shared__ uint4 lds_[];
    __shared__ float4 part[NWAVE][4][TQ];
    char* smem = (char*)lds_;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane & 15, g = lane >> 4;
    const int x0 = blockIdx.x * TQ, y = blockIdx.y, i = blockIdx.z;
    const int hw = a.h * a.w, r = a.r;
    const int rowbytes = a.C * (int)sizeof(T);
    const int nchunk = a.pitch / CHB;
    const int nq = min(TQ, a.w - x0);
    const char* fb = (const char*)a.feat;
    const char* tgt_base = fb + ((int64_t)a.it[i].tgt * a.stride + ((int64_t)y * a.w + x0) * a.C) * (int64_t)sizeof(T);
    char* tgt_img = smem;
    char* stage = smem + (RES ? TQ * a.pitch : 0) + wave * (RES ? 1 : 2) * STAGE;
    char* stage_t = stage + STAGE;               // !RES only

    if (RES) {                                   // the 16 targets' rows, zero beyond the grid's edge and beyond C
        const int per_row = a.pitch / 16;
        for (int id = threadIdx.x; id < TQ * per_row; id += NTHR) {
            const int row = id / per_row, s = id - row * per_row;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (row < nq && s * 16 < rowbytes) v = *reinterpret_cast<const uint4*>(tgt_base + (int64_t)row * rowbytes + s * 16);
            *reinterpret_cast<uint4*>(tgt_img + row * a.pitch + (s >> 4) * CHB + swz(row, s & 15)) = v;
        }
        __syncthreads();
    }

    const int ylo = max(0, y - r), yhi = min(a.h - 1, y + r);
    const int xl = max(0, x0 - r), xr = min(a.w - 1, x0 + nq - 1 + r);
    const int nt = (xr - xl) / TQ + 1, nrow = yhi - ylo + 1;
    const int nsrc = a.it[i].nsrc;
    const int nunit = nsrc * nrow * nt;
    const int xq = x0 + q;
    const bool qon = q < nq;
    const float invq = qon ? a.inv[(int64_t)i * NSLOT * hw + y * a.w + xq] : 0.f;
    const float ninf = -INFINITY;
    float m = ninf, l = 0.f, ac = 0.f, pk = ninf;

    for (int u = wave; u < nunit; u += NWAVE) {
        const int s = u / (nrow * nt), rem = u - s * (nrow * nt);
        const int yy = ylo + rem / nt, cx = xl + (rem % nt) * TQ;
        const int ncol = min(TQ, xr - cx + 1);
        const char* cand_base = fb + ((int64_t)a.it[i].src[s] * a.stride + ((int64_t)yy * a.w + cx) * a.C) * (int64_t)sizeof(T);
        const float* invp = a.inv + ((int64_t)i * NSLOT + 1 + s) * hw + yy * a.w + cx;
        const float* labp = a.labels + (int64_t)a.it[i].label[s] * hw + yy * a.w + cx;
        float ip[4], lb[4];
        bool ok[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int pc = g * 4 + e;
            const bool on = pc < ncol;
            ok[e] = on && qon && abs(cx + pc - xq) <= r;
            ip[e] = on ? invp[pc] : 0.f;
            lb[e] = on ? labp[pc] : 0.f;
        }
        uint4 cv[4], tv[4];
        auto load = [&](int c) {
            const int byte = c * CHB + q * 16;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = j * 4 + g;
                cv[j] = make_uint4(0, 0, 0, 0);
                if (row < ncol && byte < rowbytes) cv[j] = *reinterpret_cast<const uint4*>(cand_base + (int64_t)row * rowbytes + byte);
                if (!RES) {
                    tv[j] = make_uint4(0, 0, 0, 0);
                    if (row < nq && byte < rowbytes) tv[j] = *reinterpret_cast<const uint4*>(tgt_base + (int64_t)row * rowbytes + byte);
                }
            }
        };
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        load(0);
        for (int c = 0; c < nchunk; ++c) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = j * 4 + g;
                *reinterpret_cast<uint4*>(stage + row * CHB + swz(row, q)) = cv[j];
                if (!RES) *reinterpret_cast<uint4*>(stage_t + row * CHB + swz(row, q)) = tv[j];
            }
            if (c + 1 < nchunk) load(c + 1);
            stage_sync();                        // the rows other lanes of this wave stored are read below
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int o = swz(q, st * 4 + g);
                const uint4 fa = *reinterpret_cast<const uint4*>(stage + q * CHB + o);
                const uint4 fb_ = RES ? *reinterpret_cast<const uint4*>(tgt_img + q * a.pitch + c * CHB + o)
                                      : *reinterpret_cast<const uint4*>(stage_t + q * CHB + o);
                acc = Mma<T>::run(fa, fb_, acc);
            }
            stage_sync();                        // and the next chunk's stores come behind these reads
        }
        // acc[e] = <candidate 4 g + e, target q>: the lane's own online softmax
        float lg[4], mx = m;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float c = (acc[e] * invq) * ip[e];
            lg[e] = c / a.temperature;
            if (ok[e]) { pk = fmaxf(pk, c); mx = fmaxf(mx, lg[e]); }
        }
        if (mx > ninf) {
            if (mx > m) {
                const float sc = m == ninf ? 0.f : expf(m - mx);
                l *= sc; ac *= sc; m = mx;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (ok[e]) {
                    const float wgt = expf(lg[e] - m);
                    l += wgt;
                    ac += wgt * lb[e];
                }
        }
    }
    part[wave][g][q] = make_float4(m, l, ac, pk);
    __syncthreads();
    if (threadIdx.x < nq) {                      // the target's 16 partial states in a fixed order
        float M = ninf, P = ninf;
        for (int k = 0; k < NWAVE * 4; ++k) { const float4 p = part[k >> 2][k & 3][threadIdx.x]; M = fmaxf(M, p.x); P = fmaxf(P, p.w); }
        float L = 0.f, A = 0.f;
        for (int k = 0; k < NWAVE * 4; ++k) {
            const float4 p = part[k >> 2][k & 3][threadIdx.x];
            if (p.x > ninf) { const float e = expf(p.x - M); L += p.y * e; A += p.z * e; }
        }
        const int64_t o = ((int64_t)i * a.h + y) * a.w + x0 + threadIdx.x;
        a.out[o] = A / L;                        // L >= 1: p = q of every source is a candidate, and the largest weight is exp(0)
        if (a.peak) a.peak[o] = P;
    }
}

// legacy bilinear coefficients (ops_score.hip interp_coef): the product is rounded on its own
__device__ __forceinline__ void fuse_coef(int o, float scale, int n_in, int& lo, int& hi, float& lerp) {
#pragma clang fp contract(off)
    const float in = (float)o * scale;
    lo = min((int)floorf(in), n_in - 1);           // never past the map, whatever the rounding of the product (it is not, below 2^22 rows)
    hi = min(lo + 1, n_in - 1);
    lerp = in - (float)lo;
}

__global__ __launch_bounds__(NTHR) void fuse_kernel(const float* own, const float* prop, float* fused,
                                                    int h, int w, int H, int W, float alpha) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int px = blockIdx.x * NTHR + threadIdx.x;
    if (px >= H * W) return;
    const int64_t o = (int64_t)b * H * W + px;
    const float ov = own[o];
    if (alpha == 0.f) { fused[o] = ov; return; }                     // own, bit for bit: no multiply
    const int Y = px / W, X = px - Y * W;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    int y0, y1, x0, x1; float fy, fx;
    fuse_coef(Y, sy, h, y0, y1, fy);
    fuse_coef(X, sx, w, x0, x1, fx);
    const float* s = prop + (int64_t)b * h * w;
    const float tl = s[y0 * w + x0], tr = s[y0 * w + x1], bl = s[y1 * w + x0], br = s[y1 * w + x1];
    const float top = tl + (tr - tl) * fx;
    const float bot = bl + (br - bl) * fx;
    const float u = top + (bot - top) * fy;
    fused[o] = (1.0f - alpha) * ov + alpha * u;
}

int plan(const char* who, int n, int h, int w, int64_t* bytes) {
    if (n < 1 || n > CMPC_EVAL_MAX_BATCH) { cmpc_set_error("%s: n = %d outside 1..%d", who, n, CMPC_EVAL_MAX_BATCH); return CMPC_EINVAL; }
    if (h < 1 || w < 1) { cmpc_set_error("%s: empty grid (%d x %d)", who, h, w); return CMPC_EINVAL; }
    if ((int64_t)h * w > CMPC_POOL_MAX_POSITIONS) {
        cmpc_set_error("%s: %d x %d positions, at most %d", who, h, w, CMPC_POOL_MAX_POSITIONS);
        return CMPC_EINVAL;
    }
    if (h > CMPC_PROP_MAX_ROWS) {               // a grid row is a workgroup row of the launch
        cmpc_set_error("%s: %d rows, at most %d", who, h, CMPC_PROP_MAX_ROWS);
        return CMPC_EINVAL;
    }
    *bytes = (int64_t)n * NSLOT * h * w * (int64_t)sizeof(float);
    return CMPC_OK;
}

}  // namespace

extern "C" int cmpc_label_propagate_workspace(int n, int h, int w, int64_t* bytes) {
    if (!bytes) { cmpc_set_error("label_propagate_workspace: NULL pointer"); return CMPC_EINVAL; }
    return plan("label_propagate_workspace", n, h, w, bytes);
}

extern "C" int cmpc_label_propagate(int dt, const void* feat, int64_t frame_stride, int frames, const float* labels, int n_labels,
                                    const cmpc_prop_item* items_host, int n, int h, int w, int C, int radius, float temperature,
                                    float* out, float* peak, void* ws, int64_t ws_bytes, void* stream) {
    if (!feat || !labels || !items_host || !out || !ws) { cmpc_set_error("label_propagate: NULL pointer"); return CMPC_EINVAL; }
    int64_t need = 0;
    const int rc = plan("label_propagate", n, h, w, &need);
    if (rc) return rc;
    if (dt != DT_F32 && dt != DT_BF16 && dt != DT_F16) { cmpc_set_error("label_propagate: bad dtype %d", dt); return CMPC_EINVAL; }
    if (C < 8 || C % 8 || C > (1 << 20)) { cmpc_set_error("label_propagate: C = %d must be a multiple of 8, at most %d", C, 1 << 20); return CMPC_EINVAL; }
    if (frames < 1 || n_labels < 1) { cmpc_set_error("label_propagate: empty bank (%d frames, %d labels)", frames, n_labels); return CMPC_EINVAL; }
    const int64_t tap = (int64_t)h * w * C;
    if (frame_stride % 8 || frame_stride < tap) {
        cmpc_set_error("label_propagate: a stride of %lld elements between frames: a multiple of 8 >= %lld (one tap) is needed",
                       (long long)frame_stride, (long long)tap);
        return CMPC_EINVAL;
    }
    if (!(temperature >= CMPC_PROP_MIN_TEMPERATURE) || !isfinite(temperature)) {    // below it c / temperature could leave float32
        cmpc_set_error("label_propagate: the temperature must be finite and >= %g, got %g", (double)CMPC_PROP_MIN_TEMPERATURE, (double)temperature);
        return CMPC_EINVAL;
    }
    for (int i = 0; i < n; ++i) {
        const cmpc_prop_item& it = items_host[i];
        if (it.nsrc < 1 || it.nsrc > CMPC_PROP_MAX_SOURCES) {
            cmpc_set_error("label_propagate: item %d has %d sources, 1..%d are allowed", i, it.nsrc, CMPC_PROP_MAX_SOURCES);
            return CMPC_EINVAL;
        }
        if (it.tgt < 0 || it.tgt >= frames) {
            cmpc_set_error("label_propagate: item %d: target frame %d outside a bank of %d", i, it.tgt, frames);
            return CMPC_EINVAL;
        }
        for (int s = 0; s < it.nsrc; ++s) {
            if (it.src[s] < 0 || it.src[s] >= frames) {
                cmpc_set_error("label_propagate: item %d: source frame %d outside a bank of %d", i, it.src[s], frames);
                return CMPC_EINVAL;
            }
            if (it.label[s] < 0 || it.label[s] >= n_labels) {
                cmpc_set_error("label_propagate: item %d: label %d outside a bank of %d", i, it.label[s], n_labels);
                return CMPC_EINVAL;
            }
        }
    }
    if (ws_bytes < need) {
        cmpc_set_error("label_propagate: workspace of %lld bytes, %lld needed (cmpc_label_propagate_workspace)", (long long)ws_bytes, (long long)need);
        return CMPC_EINVAL;
    }
    if (((uintptr_t)feat & 15) || ((uintptr_t)ws & 15) || ((uintptr_t)labels & 3) || ((uintptr_t)out & 3) || ((uintptr_t)peak & 3)) {
        cmpc_set_error("label_propagate: feat and the workspace must be 16-byte aligned, labels, out and peak 4-byte aligned");
        return CMPC_EINVAL;
    }
    PropArgs a;
    a.feat = feat; a.stride = frame_stride; a.labels = labels; a.out = out; a.peak = peak; a.inv = (float*)ws;
    a.h = h; a.w = w; a.C = C; a.temperature = temperature;
    const int whole = std::max(h, w);
    a.r = radius < 0 || radius > whole ? whole : radius;
    const int esz = dt == DT_F32 ? 4 : 2;
    a.pitch = (C * esz + CHB - 1) / CHB * CHB;
    for (int i = 0; i < n; ++i) a.it[i] = items_host[i];
    for (int i = n; i < CMPC_EVAL_MAX_BATCH; ++i) a.it[i] = items_host[0];
    hipStream_t st = (hipStream_t)stream;
    const int hw = h * w;
    CMPC_DISPATCH_DT(dt, hipLaunchKernelGGL(norm_kernel<T>, dim3((hw + NWAVE - 1) / NWAVE, NSLOT, n), dim3(NTHR), 0, st, a));
    const int e = cmpc_check_launch("label_propagate");
    if (e) return e;
    const dim3 grid((w + TQ - 1) / TQ, h, n);
    if (TQ * a.pitch <= RES_MAX) {
        const size_t lds = (size_t)TQ * a.pitch + NWAVE * STAGE;
        CMPC_DISPATCH_DT(dt, hipLaunchKernelGGL((prop_kernel<T, true>), grid, dim3(NTHR), lds, st, a));
    } else {
        const size_t lds = (size_t)NWAVE * 2 * STAGE;
        CMPC_DISPATCH_DT(dt, hipLaunchKernelGGL((prop_kernel<T, false>), grid, dim3(NTHR), lds, st, a));
    }
    return cmpc_check_launch("label_propagate");
}

extern "C" int cmpc_prop_fuse(const float* own, const float* prop, int n, int h, int w, int H, int W, float alpha, float* fused, void* stream) {
    if (!own || !prop || !fused) { cmpc_set_error("prop_fuse: NULL pointer"); return CMPC_EINVAL; }
    if (n < 1 || n > CMPC_EVAL_MAX_BATCH) { cmpc_set_error("prop_fuse: n = %d outside 1..%d", n, CMPC_EVAL_MAX_BATCH); return CMPC_EINVAL; }
    if (h < 1 || w < 1 || H < 1 || W < 1) { cmpc_set_error("prop_fuse: empty map (%d x %d -> %d x %d)", h, w, H, W); return CMPC_EINVAL; }
    if ((int64_t)h * w > CMPC_POOL_MAX_POSITIONS || (int64_t)H * W > (1 << 28)) {
        cmpc_set_error("prop_fuse: %d x %d -> %d x %d is too large (at most %d and %d positions)", h, w, H, W, CMPC_POOL_MAX_POSITIONS, 1 << 28);
        return CMPC_EINVAL;
    }
    if (!(alpha >= 0.f && alpha <= 1.f)) { cmpc_set_error("prop_fuse: alpha = %g outside [0, 1]", (double)alpha); return CMPC_EINVAL; }
    if (((uintptr_t)own & 3) || ((uintptr_t)prop & 3) || ((uintptr_t)fused & 3)) {
        cmpc_set_error("prop_fuse: own, prop and fused must be 4-byte aligned");
        return CMPC_EINVAL;
    }
    hipLaunchKernelGGL(fuse_kernel, dim3((H * W + NTHR - 1) / NTHR, n), dim3(NTHR), 0, (hipStream_t)stream, own, prop, fused, h, w, H, W, alpha);
    return cmpc_check_launch("prop_fuse");
}
