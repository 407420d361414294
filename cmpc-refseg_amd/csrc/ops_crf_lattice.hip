// DenseCRF post-processing (test.py:309-322) with both pairwise terms filtered through a permutohedral lattice, as pydensecrf does it,
// batched: one call refines B samples of the same H x W, every launch covers all B, nothing synchronises with the host.
//
//   A. Adams, J. Baek, M. A. Davis, "Fast High-Dimensional Filtering Using the Permutohedral Lattice", Eurographics 2010 (lattice).
//   P. Kraehenbuehl, V. Koltun, "Efficient Inference in Fully Connected CRFs with Gaussian Edge Potentials", NIPS 2011 (mean field).
//
// Features (oracle/dense_crf_numpy.py):  Gaussian  d = 2, f = (x, y) / sxy_g;   bilateral  d = 5, f = (x / sxy_b, y / sxy_b, r / srgb,
// g / srgb, b / srgb),  every quotient evaluated as f = c * float(1 / s).
// Lattice (Adams et al. 2010, sections 3-4), per pixel, in float32 without contraction (tests/crf_lattice_ref.py repeats the same
// operations, so both sides take the same discrete decisions):
//   elevate    cf_i = f_i * s_i,  s_i = sqrt(2/3) (d+1) / sqrt((i+1)(i+2));   e_j = sum_{i>=j} cf_i - j cf_{j-1} (j >= 1),  e_0 = sum_i cf_i
//   simplex    rem0_i = (d+1) rint(e_i / (d+1));  rank_i = #{k : e_k - rem0_k beats e_i - rem0_i} (ties go to the later index), shifted by
//              sum_i rint(e_i / (d+1)) and wrapped into [0, d] with rem0_i -/+ (d+1)
//   weights    b[d - rank_i] += (e_i - rem0_i) / (d+1),  b[d - rank_i + 1] -= (e_i - rem0_i) / (d+1),  b[0] += 1 + b[d+1]
//   vertices   key_r = rem0 + c_r(rank),  c_r(k) = r if k <= d - r else r - (d+1),   r = 0..d   (the first d coordinates are stored)
// A filter L v = alpha * S^T B_d ... B_0 S v:  splat S (vertex += w * v), blur B_j (v' = v + (v_n1 + v_n2) / 2 with n1 / n2 the vertices at
// key -/+ (-1, ..., -1, +d at axis j, -1, ...), absent = 0), slice S^T scaled by alpha = 1 / (1 + 2^-d) (Adams et al. 2010, p. 6).
// Each B_j is symmetric; their product is not exactly (a vertex a path passes through may be absent), so L^T applies them in reverse.
// Mean field (Kraehenbuehl & Koltun 2011), unchanged from ops_crf.hip: unary clamp 1e-30, Q_0 = softmax(-U), nrm = 1 / sqrt(L 1 + 1e-20),
// Q <- softmax(-U + sum_m w_m nrm_m L_m (nrm_m Q)), argmax with label 0 winning a tie, iters = 0 gives softmax(-U).
// PARITY UNPINNED against pydensecrf itself: the library is not installed and not in the reference tree.
//
// Per sample and lattice the work is built once and reused by both normalisers and every iteration:
//   lat_embed      one thread per pixel: the d+1 keys, inserted into the sample's open-addressing table (linear probing, at most T probes,
//                  T = pow2 >= 2 N (d+1)), atomicMin of the entry id e = pixel (d+1) + r on the slot: its smallest producer ("leader")
//   lat_count / lat_scan_parts / lat_number   dense vertex numbers = prefix sum of the leader flags in entry order: independent of timing
//   lat_links      slice table (vertex of every entry) and blur-neighbour table (d+1 directions x 2 per vertex, -1 = absent)
// Determinism (README "reproducibility"): integer atomics only.  Splat accumulates EXACT fixed-point int64 (2^-32 units): integer sums are
// order-independent, so no sort, one pass, and a sample gives the same bits alone or anywhere in a batch.  Range: a contribution w * v is
// at most nrm <= 1 / sqrt(alpha / (d+1)) < 2 (L 1 >= alpha sum_r w_r^2), so a vertex total stays below 2 N << 2^31 units of 1.
// Keys: d coordinates of 63 / d bits (31 for d = 2, 12 for d = 5), so |key_i| <= 2^(bits-1) - 1; the entry point bounds |key_i| from the
// parameters before launching (CMPC_EINVAL naming the limit).  At the reference's parameters (sxy_b 20, srgb 3) the bound on bilateral
// keys is +-396 at 320 x 320 and stays within +-2047 up to 6379 x 6379; Gaussian keys (sxy_g 3) reach +-298 at 320 x 320 against +-2^30.  A probe loop that runs out, or a key outside the range, sets an error word:
// that call's outputs are poisoned (Q NaN, mask 255) and the next call on any stream returns CMPC_EHIP.
#include "cmpc_common.h"
#include "../../include/cmpc.h"

#include <cmath>
#include <mutex>

namespace {

constexpr unsigned long long kEmpty = ~0ull;           // no valid packed key has all 64 bits set (the top bit is always 0)
constexpr int kChunk = 1024;                           // entries per block of the leader scan (256 threads x 4)

__host__ __device__ constexpr int key_bits(int d) { return 63 / d; }
__host__ __device__ constexpr int key_max(int d) { return (1 << (key_bits(d) - 1)) - 1; }

struct LatArgs {
    float inv[5];                                      // 1 / sigma per feature (float)
    float sc[5];                                       // elevation scale s_i (float)
    int N, H, W;
    long E, T;                                         // entries N (d+1) and table slots per sample
    int nblk;                                          // leader-scan chunks per sample
    unsigned long long* keys; int* lead;               // [B][T]
    int* slot; float* w; int* off; int* vid;           // [B][E]
    unsigned long long* vkey;                          // [B][E]: key of vertex m (m < M[b])
    int2* nb;                                          // [B][d+1][E]
    unsigned long long* acc;                           // [B][E][2] fixed-point splat accumulator
    float2* buf0; float2* buf1;                        // [B][E] blur ping-pong
    int* part; int* M;                                 // [B][nblk], [B]
};

__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}

template <int D>
__device__ __forceinline__ bool pack_key(const int* k, unsigned long long* out) {
    unsigned long long p = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        if (k[i] < -key_max(D) || k[i] > key_max(D)) return false;
        p |= (unsigned long long)(k[i] + key_max(D) + 1) << (i * key_bits(D));
    }
    *out = p;
    return true;
}

template <int D>
__device__ __forceinline__ void unpack_key(unsigned long long p, int* k) {
#pragma unroll
    for (int i = 0; i < D; ++i) k[i] = (int)((p >> (i * key_bits(D))) & ((1ull << key_bits(D)) - 1)) - key_max(D) - 1;
}

// vertex number of `key` in the sample's table, -1 when absent; at most T probes
__device__ __forceinline__ int lookup(const unsigned long long* keys, const int* lead, const int* vid, long T, unsigned long long key, unsigned int* err) {
    long t = (long)(mix64(key) & (unsigned long long)(T - 1));
    for (long p = 0; p < T; ++p, t = (t + 1) & (T - 1)) {
        const unsigned long long k = keys[t];
        if (k == key) return vid[lead[t]];
        if (k == kEmpty) return -1;
    }
    atomicOr(err, 1u);
    return -1;
}

__global__ __launch_bounds__(256) void lat_init_kernel(const float* __restrict__ sigm, float2* __restrict__ U, float2* __restrict__ Q, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float p = sigm[i];
    const float u0 = -logf(fmaxf(1.0f - p, 1e-30f)), u1 = -logf(fmaxf(p, 1e-30f));      // test.py:312-315
    U[i] = make_float2(u0, u1);
    const float m = fminf(u0, u1), e0 = expf(m - u0), e1 = expf(m - u1), r = 1.0f / (e0 + e1);
    Q[i] = make_float2(e0 * r, e1 * r);
}

// grid (ceil(N / 256), B): the d+1 vertices of each pixel, inserted; slot and weight of every entry
template <int D>
__global__ __launch_bounds__(256) void lat_embed_kernel(const unsigned char* __restrict__ rgb, LatArgs a, unsigned int* err) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= a.N) return;
    float f[D];
    f[0] = (float)(i % a.W) * a.inv[0];
    f[1] = (float)(i / a.W) * a.inv[1];
    if constexpr (D == 5) {
        const unsigned char* px = rgb + ((long)b * a.N + i) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) f[2 + c] = (float)px[c] * a.inv[2 + c];
    }
    float el[D + 1], sm = 0.f;
#pragma unroll
    for (int j = D; j > 0; --j) {
        const float cf = f[j - 1] * a.sc[j - 1];
        el[j] = sm - (float)j * cf;
        sm = sm + cf;
    }
    el[0] = sm;
    const float down = 1.0f / (D + 1);
    int rem0[D + 1], rank[D + 1], tot = 0;
#pragma unroll
    for (int k = 0; k <= D; ++k) {
        const int rd = (int)rintf(el[k] * down);
        rem0[k] = rd * (D + 1); tot += rd; rank[k] = 0;
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const float dk = el[k] - (float)rem0[k];
#pragma unroll
        for (int j = k + 1; j <= D; ++j) {
            if (dk < el[j] - (float)rem0[j]) ++rank[k]; else ++rank[j];
        }
    }
#pragma unroll
    for (int k = 0; k <= D; ++k) {
        rank[k] += tot;
        if (rank[k] < 0) { rank[k] += D + 1; rem0[k] += D + 1; }
        else if (rank[k] > D) { rank[k] -= D + 1; rem0[k] -= D + 1; }
    }
    float bary[D + 2];
#pragma unroll
    for (int k = 0; k < D + 2; ++k) bary[k] = 0.f;
#pragma unroll
    for (int k = 0; k <= D; ++k) {                     // + / - 0 elsewhere: register-resident, same values as indexed updates
        const float v = (el[k] - (float)rem0[k]) * down;
#pragma unroll
        for (int m = 0; m < D + 2; ++m) {
            if (m == D - rank[k]) bary[m] += v;
            if (m == D - rank[k] + 1) bary[m] -= v;
        }
    }
    bary[0] += 1.0f + bary[D + 1];
    unsigned long long* keys = a.keys + (long)b * a.T;
    int* lead = a.lead + (long)b * a.T;
#pragma unroll
    for (int r = 0; r <= D; ++r) {
        int key[D];
#pragma unroll
        for (int k = 0; k < D; ++k) key[k] = rem0[k] + (rank[k] <= D - r ? r : r - (D + 1));
        const int e = i * (D + 1) + r;
        const long ge = (long)b * a.E + e;
        a.w[ge] = bary[r];
        unsigned long long pk;
        int s = -1;
        if (!pack_key<D>(key, &pk)) {
            atomicOr(err, 2u);
        } else {
            long t = (long)(mix64(pk) & (unsigned long long)(a.T - 1));
            for (long p = 0; p < a.T; ++p, t = (t + 1) & (a.T - 1)) {
                unsigned long long cur = __hip_atomic_load(&keys[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur == kEmpty) cur = atomicCAS(&keys[t], kEmpty, pk);
                if (cur == kEmpty || cur == pk) { s = (int)t; break; }
            }
            if (s < 0) atomicOr(err, 1u);
            else atomicMin(&lead[s], e);
        }
        a.slot[ge] = s;
    }
}

__device__ __forceinline__ bool is_leader(const LatArgs& a, int b, long e) {
    if (e >= a.E) return false;
    const int s = a.slot[(long)b * a.E + e];
    return s >= 0 && a.lead[(long)b * a.T + s] == (int)e;
}

// exclusive prefix over the block's 256 thread counts (LDS); returns the thread's offset, *total = the block's sum
__device__ __forceinline__ int block_exclusive_scan(int v, int* total) {
    __shared__ int s[256];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int t = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    const int incl = s[threadIdx.x];
    *total = s[255];
    __syncthreads();
    return incl - v;
}

// grid (nblk, B): leaders per chunk of kChunk entries
__global__ __launch_bounds__(256) void lat_count_kernel(LatArgs a) {
    const int b = blockIdx.y;
    const long e0 = (long)blockIdx.x * kChunk + threadIdx.x * 4;
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += is_leader(a, b, e0 + k) ? 1 : 0;
    int total;
    block_exclusive_scan(c, &total);
    if (threadIdx.x == 0) a.part[(long)b * a.nblk + blockIdx.x] = total;
}

// grid (1, B): exclusive scan of the chunk counts, M[b] = the sample's vertex count
__global__ __launch_bounds__(256) void lat_scan_parts_kernel(LatArgs a) {
    const int b = blockIdx.y;
    int* part = a.part + (long)b * a.nblk;
    int carry = 0;
    for (int base = 0; base < a.nblk; base += 256) {
        const int k = base + threadIdx.x;
        const int v = k < a.nblk ? part[k] : 0;
        int total;
        const int ex = block_exclusive_scan(v, &total);
        if (k < a.nblk) part[k] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) a.M[b] = carry;
}

// grid (nblk, B): vertex number of every leader entry (vid[e]) and the key of every vertex (vkey[m])
__global__ __launch_bounds__(256) void lat_number_kernel(LatArgs a) {
    const int b = blockIdx.y;
    const long e0 = (long)blockIdx.x * kChunk + threadIdx.x * 4;
    bool f[4];
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { f[k] = is_leader(a, b, e0 + k); c += f[k] ? 1 : 0; }
    int total;
    int m = a.part[(long)b * a.nblk + blockIdx.x] + block_exclusive_scan(c, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!f[k]) continue;
        const long ge = (long)b * a.E + e0 + k;
        a.vid[ge] = m;
        a.vkey[(long)b * a.E + m] = a.keys[(long)b * a.T + a.slot[ge]];
        ++m;
    }
}

// grid (ceil(E / 256), B): thread t writes the slice entry off[t] and, for t < M[b], the blur neighbours of vertex t
template <int D>
__global__ __launch_bounds__(256) void lat_links_kernel(LatArgs a, unsigned int* err) {
    const int b = blockIdx.y;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.E) return;
    const unsigned long long* keys = a.keys + (long)b * a.T;
    const int* lead = a.lead + (long)b * a.T;
    const int* vid = a.vid + (long)b * a.E;
    const int s = a.slot[(long)b * a.E + t];
    a.off[(long)b * a.E + t] = s >= 0 ? vid[lead[s]] : 0;
    if (t >= a.M[b]) return;
    int key[D], n1[D], n2[D];
    unpack_key<D>(a.vkey[(long)b * a.E + t], key);
#pragma unroll
    for (int j = 0; j <= D; ++j) {
#pragma unroll
        for (int k = 0; k < D; ++k) { n1[k] = key[k] - 1; n2[k] = key[k] + 1; }
        if (j < D) { n1[j] = key[j] + D; n2[j] = key[j] - D; }
        unsigned long long p1, p2;
        const int v1 = pack_key<D>(n1, &p1) ? lookup(keys, lead, vid, a.T, p1, err) : -1;     // out of range: no such vertex
        const int v2 = pack_key<D>(n2, &p2) ? lookup(keys, lead, vid, a.T, p2, err) : -1;
        a.nb[((long)b * (D + 1) + j) * a.E + t] = make_int2(v1, v2);
    }
}

// grid (ceil(E / 256), B): acc[vertex] += w * v in 2^-32 fixed point;  v = (1, 0) for the normaliser, else Q * nrm of the pixel
template <int D, bool ONES>
__global__ __launch_bounds__(256) void lat_splat_kernel(LatArgs a, const float2* __restrict__ Q, const float* __restrict__ nrm) {
    const int b = blockIdx.y;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.E) return;
    const long ge = (long)b * a.E + e;
    if (a.slot[ge] < 0) return;                        // error already flagged
    const float w = a.w[ge];
    unsigned long long* dst = a.acc + 2 * ((long)b * a.E + a.off[ge]);
    if (ONES) {
        atomicAdd(dst, (unsigned long long)__float2ll_rn(w * 4294967296.0f));
    } else {
        const long p = (long)b * a.N + e / (D + 1);
        const float2 q = Q[p];
        const float n = nrm[p];
        atomicAdd(dst, (unsigned long long)__float2ll_rn(w * (q.x * n) * 4294967296.0f));
        atomicAdd(dst + 1, (unsigned long long)__float2ll_rn(w * (q.y * n) * 4294967296.0f));
    }
}

__device__ __forceinline__ float2 from_fixed(const unsigned long long* acc, long v) {
    return make_float2((float)((double)(long long)acc[2 * v] * 0x1p-32), (float)((double)(long long)acc[2 * v + 1] * 0x1p-32));
}

// grid (ceil(E / 256), B): one blur pass along direction j over the sample's M[b] vertices.  Pass 0 reads the fixed-point accumulator;
// pass 1 clears it (nothing reads it any more) for the next splat.
template <int D>
__global__ __launch_bounds__(256) void lat_blur_kernel(LatArgs a, int j, const float2* __restrict__ src, float2* __restrict__ dst) {
    const int b = blockIdx.y;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.M[b]) return;
    const long base = (long)b * a.E;
    const int2 n = a.nb[((long)b * (D + 1) + j) * a.E + t];
    float2 v, v1 = make_float2(0.f, 0.f), v2 = make_float2(0.f, 0.f);
    if (j == 0) {
        v = from_fixed(a.acc, base + t);
        if (n.x >= 0) v1 = from_fixed(a.acc, base + n.x);
        if (n.y >= 0) v2 = from_fixed(a.acc, base + n.y);
    } else {
        v = src[base + t];
        if (n.x >= 0) v1 = src[base + n.x];
        if (n.y >= 0) v2 = src[base + n.y];
        if (j == 1) { a.acc[2 * (base + t)] = 0ull; a.acc[2 * (base + t) + 1] = 0ull; }
    }
    dst[base + t] = make_float2(v.x + 0.5f * (v1.x + v2.x), v.y + 0.5f * (v1.y + v2.y));
}

template <int D>
__device__ __forceinline__ float2 slice(const LatArgs& a, const float2* vals, int b, long i) {
    float2 s = make_float2(0.f, 0.f);
    const long e0 = (long)b * a.E + i * (D + 1);
#pragma unroll
    for (int r = 0; r <= D; ++r) {
        const float w = a.w[e0 + r];
        const float2 v = vals[(long)b * a.E + a.off[e0 + r]];
        s.x += w * v.x; s.y += w * v.y;
    }
    return s;
}

// grid (ceil(N / 256), B): nrm = 1 / sqrt(alpha * slice(blurred ones) + 1e-20)
template <int D>
__global__ __launch_bounds__(256) void lat_norm_kernel(LatArgs a, const float2* __restrict__ vals, float alpha, float* __restrict__ nrm) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    nrm[(long)b * a.N + i] = rsqrtf(alpha * slice<D>(a, vals, b, i).x + 1e-20f);
}

// grid (ceil(N / 256), B): Q <- softmax(-U + w_g nrm_g alpha_g slice_g + w_b nrm_b alpha_b slice_b)  (PAIR = false: softmax(-U))
template <bool PAIR>
__global__ __launch_bounds__(256) void lat_update_kernel(LatArgs g, LatArgs bl, const float2* __restrict__ U, const float2* __restrict__ vg,
                                                         const float2* __restrict__ vb, const float* __restrict__ ng, const float* __restrict__ nb,
                                                         float ag, float ab, float wg, float wb, float2* __restrict__ Q, float* __restrict__ q_out,
                                                         unsigned char* __restrict__ mask, const unsigned int* __restrict__ err,
                                                         unsigned int* err_host) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int N = g.N;
    if (i >= N) return;
    const long p = (long)b * N + i;
    const float2 u = U[p];
    float e0 = -u.x, e1 = -u.y;
    if (PAIR) {
        const float2 fg = slice<2>(g, vg, b, i), fb = slice<5>(bl, vb, b, i);
        const float cg = wg * ng[p] * ag, cb = wb * nb[p] * ab;
        e0 = -u.x + cg * fg.x + cb * fb.x;
        e1 = -u.y + cg * fg.y + cb * fb.y;
    }
    const float m = fmaxf(e0, e1), x0 = expf(e0 - m), x1 = expf(e1 - m), r = 1.0f / (x0 + x1);
    float q0 = x0 * r, q1 = x1 * r;
    Q[p] = make_float2(q0, q1);
    unsigned char lab = x1 > x0 ? 1 : 0;               // np.argmax(Q, axis=0): the first maximum wins a tie
    if (err && *err) {                                 // a failed lattice build: never a plausible answer
        q0 = q1 = __builtin_nanf(""); lab = 255;
        if (i == 0 && b == 0) *(volatile unsigned int*)err_host = *err;
    }
    if (q_out) { q_out[(long)b * 2 * N + i] = q0; q_out[(long)b * 2 * N + N + i] = q1; }
    if (mask) mask[p] = lab;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

long pow2_at_least(long x) { long t = 1; while (t < x) t <<= 1; return t; }

// bytes of one lattice's region for B samples (carve(nullptr) sizes it)
template <int D>
size_t carve(char* base, int B, int N, LatArgs* a) {
    const long E = (long)N * (D + 1), T = pow2_at_least(2 * E);
    const int nblk = (int)((E + kChunk - 1) / kChunk);
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    a->E = E; a->T = T; a->nblk = nblk; a->N = N;
    a->keys = (unsigned long long*)take((size_t)B * T * 8);
    a->lead = (int*)take((size_t)B * T * 4);
    a->slot = (int*)take((size_t)B * E * 4);
    a->w = (float*)take((size_t)B * E * 4);
    a->off = (int*)take((size_t)B * E * 4);
    a->vid = (int*)take((size_t)B * E * 4);
    a->vkey = (unsigned long long*)take((size_t)B * E * 8);
    a->nb = (int2*)take((size_t)B * (D + 1) * E * 8);
    a->acc = (unsigned long long*)take((size_t)B * E * 16);
    a->buf0 = (float2*)take((size_t)B * E * 8);
    a->buf1 = (float2*)take((size_t)B * E * 8);
    a->part = (int*)take((size_t)B * nblk * 4);
    a->M = (int*)take((size_t)B * 4);
    return o;
}

// largest |key coordinate| the embedding can produce for features in [0, fmax_i] (see the header), rounding slack included
template <int D>
double key_bound(const float* fmax, const float* sc) {
    double cf[D], worst = 0.0;
    for (int i = 0; i < D; ++i) cf[i] = (double)fmax[i] * sc[i];
    for (int j = 0; j <= D; ++j) {
        double sm = 0.0;
        for (int i = j; i < D; ++i) sm += cf[i];
        worst = std::max(worst, std::max(sm, j > 0 ? j * cf[j - 1] : 0.0));
    }
    return worst * (1.0 + 1e-5) + 1.5 * (D + 1) + D + 1;
}

// build the lattice of one feature set for all B samples and splat ones into it (the normaliser's input)
template <int D>
void build(const unsigned char* rgb, LatArgs& a, int B, unsigned int* err, hipStream_t st) {
    (void)hipMemsetAsync(a.keys, 0xFF, (size_t)B * a.T * 8, st);
    (void)hipMemsetAsync(a.lead, 0x7F, (size_t)B * a.T * 4, st);
    (void)hipMemsetAsync(a.acc, 0, (size_t)B * a.E * 16, st);
    const dim3 gp((a.N + 255) / 256, B), ge((unsigned)((a.E + 255) / 256), B), gc(a.nblk, B);
    hipLaunchKernelGGL(lat_embed_kernel<D>, gp, dim3(256), 0, st, rgb, a, err);
    hipLaunchKernelGGL(lat_count_kernel, gc, dim3(256), 0, st, a);
    hipLaunchKernelGGL(lat_scan_parts_kernel, dim3(1, B), dim3(256), 0, st, a);
    hipLaunchKernelGGL(lat_number_kernel, gc, dim3(256), 0, st, a);
    hipLaunchKernelGGL(lat_links_kernel<D>, ge, dim3(256), 0, st, a, err);
    hipLaunchKernelGGL((lat_splat_kernel<D, true>), ge, dim3(256), 0, st, a, (const float2*)nullptr, (const float*)nullptr);
}

// the d+1 blur passes over the splatted accumulator; returns the buffer holding the result
template <int D>
const float2* blur(LatArgs& a, int B, hipStream_t st) {
    const dim3 ge((unsigned)((a.E + 255) / 256), B);
    float2* src = a.buf1; float2* dst = a.buf0;
    for (int j = 0; j <= D; ++j) {
        hipLaunchKernelGGL(lat_blur_kernel<D>, ge, dim3(256), 0, st, a, j, (const float2*)src, dst);
        std::swap(src, dst);
    }
    return src;
}

unsigned int* g_err_host = nullptr;                    // sticky device-found error, pinned and mapped (allocated once)
unsigned int* g_err_host_dev = nullptr;
std::mutex g_err_mu;

}  // namespace

extern "C" int cmpc_dense_crf_lattice(const float* sigm, const unsigned char* rgb, int B, int H, int W, float sxy_g, float compat_g, float sxy_b,
                                      float srgb, float compat_b, int iters, float* q_out, unsigned char* mask_out, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    if (!sigm || !rgb || B <= 0 || B > 65535 || H <= 0 || W <= 0 || iters < 0 || !(sxy_g > 0.f) || !(sxy_b > 0.f) || !(srgb > 0.f) ||
        !std::isfinite(compat_g) || !std::isfinite(compat_b) || (!q_out && !mask_out)) {
        cmpc_set_error("dense_crf_lattice: bad args"); return CMPC_EINVAL;
    }
    if ((long)H * W * 6 * 2 > (1l << 30)) { cmpc_set_error("dense_crf_lattice: H * W = %ld > %ld pixels", (long)H * W, (1l << 30) / 12); return CMPC_EINVAL; }
    const int N = H * W;
    LatArgs g{}, bl{};
    g.H = bl.H = H; g.W = bl.W = W;
    g.inv[0] = g.inv[1] = (float)(1.0 / sxy_g);
    bl.inv[0] = bl.inv[1] = (float)(1.0 / sxy_b);
    bl.inv[2] = bl.inv[3] = bl.inv[4] = (float)(1.0 / srgb);
    for (int i = 0; i < 2; ++i) g.sc[i] = (float)(std::sqrt(2.0 / 3.0) * 3 / std::sqrt((double)((i + 1) * (i + 2))));
    for (int i = 0; i < 5; ++i) bl.sc[i] = (float)(std::sqrt(2.0 / 3.0) * 6 / std::sqrt((double)((i + 1) * (i + 2))));
    {
        const float fg[2] = {(float)(W - 1) * g.inv[0], (float)(H - 1) * g.inv[1]};
        const float fb[5] = {(float)(W - 1) * bl.inv[0], (float)(H - 1) * bl.inv[1], 255.f * bl.inv[2], 255.f * bl.inv[3], 255.f * bl.inv[4]};
        const double kg = key_bound<2>(fg, g.sc), kb = key_bound<5>(fb, bl.sc);
        if (kg > key_max(2)) { cmpc_set_error("dense_crf_lattice: Gaussian lattice keys reach +-%.0f, beyond the 31-bit packing range +-%d (sxy_g too small for %d x %d)", kg, key_max(2), H, W); return CMPC_EINVAL; }
        if (kb > key_max(5)) { cmpc_set_error("dense_crf_lattice: bilateral lattice keys reach +-%.0f, beyond the 12-bit packing range +-%d (sxy_b / srgb too small for %d x %d)", kb, key_max(5), H, W); return CMPC_EINVAL; }
    }
    {
        std::lock_guard<std::mutex> lk(g_err_mu);
        if (!g_err_host) {
            void* p = nullptr;
            if (hipHostMalloc(&p, sizeof(unsigned int), hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable) != hipSuccess) {
                cmpc_set_error("dense_crf_lattice: hipHostMalloc of the error word failed"); return CMPC_EHIP;
            }
            void* d = nullptr;
            if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) { cmpc_set_error("dense_crf_lattice: hipHostGetDevicePointer failed"); return CMPC_EHIP; }
            g_err_host = (unsigned int*)p; g_err_host_dev = (unsigned int*)d;
            *(volatile unsigned int*)g_err_host = 0;
        }
        const unsigned int prev = *(volatile unsigned int*)g_err_host;
        if (prev) {
            *(volatile unsigned int*)g_err_host = 0;
            cmpc_set_error("dense_crf_lattice: an earlier call failed on the device (%s); its outputs were poisoned",
                           (prev & 1u) ? "hash probe loop exhausted" : "lattice key outside the packing range");
            return CMPC_EHIP;
        }
    }
    const size_t common = align256((size_t)B * N * 8) * 2 + align256((size_t)B * N * 4) * 2 + 256;
    const size_t sg = carve<2>(nullptr, B, N, &g), sb = carve<5>(nullptr, B, N, &bl);
    char* ws = (char*)cmpc_ws(common + (iters > 0 ? sg + sb : 0), st);
    if (!ws) return CMPC_EHIP;
    float2* U = (float2*)ws; float2* Q = (float2*)(ws + align256((size_t)B * N * 8));
    float* ng = (float*)(ws + 2 * align256((size_t)B * N * 8));
    float* nb = (float*)((char*)ng + align256((size_t)B * N * 4));
    unsigned int* err = (unsigned int*)((char*)nb + align256((size_t)B * N * 4));
    (void)hipMemsetAsync(err, 0, sizeof(unsigned int), st);
    const long n = (long)B * N;
    hipLaunchKernelGGL(lat_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, sigm, U, Q, n);
    const dim3 gp((N + 255) / 256, B);
    if (iters == 0) {
        hipLaunchKernelGGL(lat_update_kernel<false>, gp, dim3(256), 0, st, g, bl, (const float2*)U, (const float2*)nullptr, (const float2*)nullptr,
                           (const float*)ng, (const float*)nb, 0.f, 0.f, 0.f, 0.f, Q, q_out, mask_out, (const unsigned int*)err, g_err_host_dev);
        return cmpc_check_launch("dense_crf_lattice");
    }
    carve<2>(ws + common, B, N, &g);
    carve<5>(ws + common + sg, B, N, &bl);
    const float ag = (float)(1.0 / (1.0 + std::ldexp(1.0, -2))), ab = (float)(1.0 / (1.0 + std::ldexp(1.0, -5)));
    build<2>(rgb, g, B, err, st);
    const float2* vg = blur<2>(g, B, st);
    hipLaunchKernelGGL(lat_norm_kernel<2>, gp, dim3(256), 0, st, g, vg, ag, ng);
    build<5>(rgb, bl, B, err, st);
    const float2* vb = blur<5>(bl, B, st);
    hipLaunchKernelGGL(lat_norm_kernel<5>, gp, dim3(256), 0, st, bl, vb, ab, nb);
    const dim3 geg((unsigned)((g.E + 255) / 256), B), geb((unsigned)((bl.E + 255) / 256), B);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL((lat_splat_kernel<2, false>), geg, dim3(256), 0, st, g, (const float2*)Q, (const float*)ng);
        hipLaunchKernelGGL((lat_splat_kernel<5, false>), geb, dim3(256), 0, st, bl, (const float2*)Q, (const float*)nb);
        vg = blur<2>(g, B, st);
        vb = blur<5>(bl, B, st);
        const bool last = it + 1 == iters;
        hipLaunchKernelGGL(lat_update_kernel<true>, gp, dim3(256), 0, st, g, bl, (const float2*)U, vg, vb, (const float*)ng, (const float*)nb, ag, ab,
                           compat_g, compat_b, Q, last ? q_out : nullptr, last ? mask_out : nullptr, (const unsigned int*)err, g_err_host_dev);
    }
    return cmpc_check_launch("dense_crf_lattice");
}
