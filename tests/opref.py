"""TEST SCAFFOLDING (not product code): shared pieces of the op-level kernel tests (tests/test_gpu_ops_*.py).

Every stage kernel of include/cmpc.h is called through the C ABI on seeded inputs and each output is compared, element by element, with
a float64 reference computed on the CPU from the SAME inputs (16-bit tensors are upcast, not regenerated).  This module holds what the
test files share: the tolerance check, padded / guarded buffer builders, stat blocks pre-filled with NaN, a "run twice, compare bits"
helper and a ctypes launcher.
"""
from __future__ import annotations

import importlib
import math

import torch

_lib = importlib.import_module("cmpc-refseg_amd")._lib
F32, BF16, F16 = _lib.DT_F32, _lib.DT_BF16, _lib.DT_F16
DTS = (F32, BF16, F16)
DT_IDS = ("f32", "bf16", "f16")
TDT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
ULP = {F32: 0.0, BF16: 2.0 ** -7, F16: 2.0 ** -10}      # 1 ulp (relative) of each storage type
# below the smallest normal f16 (2^-14) the ulp stops shrinking: f16 stores keep 2^-24 absolute spacing there
SUBNORMAL = {F16: 2.0 ** -24}
STAT_PARTS = 128                                         # CMPC_STAT_PARTS
GUARD = 3                                                # sentinel rows after every output
# sentinel bit patterns of the guard rows (NaN payloads no kernel produces) and of pad columns the header says are ignored
_SENT_BITS = {torch.float32: 0x7FC0DEAD, torch.bfloat16: 0x7FAD, torch.float16: 0x7E5D, torch.float64: 0x7FF8DEADBEEFDEAD,
              torch.int32: 0x5A5A5A5A}
_INT_VIEW = {4: torch.int32, 2: torch.int16, 8: torch.int64}
DEV = "cuda"


def call(name, *args):
    """One entry point; tensors are passed as their device addresses, None as NULL."""
    conv = [a.data_ptr() if torch.is_tensor(a) else a for a in args]
    _lib.call(name, *conv, stream())


def stream():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(x, dt):
    """the value an f32 / 16-bit store of x reads back as, in float64"""
    return x.to(TDT[dt] if not isinstance(dt, torch.dtype) else dt).double()


def _bits(t):
    return t.view(_INT_VIEW[t.element_size()])


def sentinel_fill(t):
    b = _SENT_BITS[t.dtype]
    if t.element_size() == 2 and b >= 0x8000:
        b -= 0x10000
    _bits(t).fill_(b)
    return t


def guarded(rows, cols, dtype, fill=None, guard=GUARD):
    """[rows + guard, cols] device buffer: the guard rows hold the sentinel; the first `rows` rows hold `fill` (a CPU tensor), or
    the sentinel when fill is None.  Returns the whole buffer; the kernel sees buf (row 0 first)."""
    if isinstance(dtype, int):
        dtype = TDT[dtype]
    buf = sentinel_fill(torch.empty(rows + guard, cols, dtype=dtype, device=DEV))
    if fill is not None:
        buf[:rows] = fill.reshape(rows, cols).to(dtype).to(DEV)
    return buf


def assert_guard(buf, rows, what=""):
    """the guard rows after `rows` come back bit-identical"""
    g = buf[rows:]
    ref = sentinel_fill(torch.empty_like(g))
    assert torch.equal(_bits(g), _bits(ref)), f"{what}: guard rows after row {rows} were written"


def assert_sentinel(t, what=""):
    ref = sentinel_fill(torch.empty_like(t))
    assert torch.equal(_bits(t), _bits(ref)), f"{what}: elements that must stay untouched were written"


def stat_block(n_stats):
    """double [n][CMPC_STAT_PARTS][2] pre-filled with NaN: the producer must clear the slots it does not use"""
    return torch.full((n_stats, STAT_PARTS, 2), float("nan"), dtype=torch.float64, device=DEV)


def map_input(B, N, C, ld, dt, g, pad="zero", scale=1.0, offset=0.0):
    """a seeded [B*N, ld] map (CPU, storage dtype) with C valid columns; pad columns [C, ld) hold 0 ("zero", what every producer
    writes), NaN ("nan") or a large sentinel ("big") for kernels whose header says they are ignored"""
    x = (torch.randn(B * N, ld, generator=g, dtype=torch.float64) * scale + offset)
    if ld > C:
        x[:, C:] = {"zero": 0.0, "nan": float("nan"), "big": 3.0e4}[pad]
    return x.to(TDT[dt])


def rtol_of(dt, K=1):
    return 2e-6 * math.sqrt(K) + ULP[dt]


def assert_close(got, ref, dt=F32, K=1, what="", rtol=None, atol=None):
    """|got - ref| <= atol + rtol |ref| on every element; rtol = 2e-6 sqrt(K) (+ 1 ulp of a 16-bit storage dt), atol = 1e-7 max|ref|.
    got: device or CPU tensor of any float dtype; ref: float64.  Reports the worst elements' indices."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if ref.numel() == 0:
        return
    rt = rtol_of(dt, K) if rtol is None else rtol
    at = 1e-7 * float(ref.abs().max()) + 1e-30 + SUBNORMAL.get(dt, 0.0)
    if atol is not None:             # a per-element term a test states the reason for (a documented 16-bit intermediate)
        at = at + (atol.double().cpu() if torch.is_tensor(atol) else atol)
    err = (got - ref).abs()
    bound = at + rt * ref.abs()
    bad = ~(err <= bound)            # NaN in got counts as bad
    if bool(bad.any()):
        idx = bad.nonzero()[:6].tolist()
        worst = [(i, float(got[tuple(i)]), float(ref[tuple(i)])) for i in idx]
        at = float(at.max()) if torch.is_tensor(at) else at
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements outside {at:.3g} + {rt:.3g}|ref| "
                             f"(dt {DT_IDS[dt] if isinstance(dt, int) else dt}, K {K}); first (index, got, ref): {worst}")


def sum_atol(terms, dim):
    """extra absolute term for a float32 sum of signed terms: its rounding scales with sum |terms| (2^-23 per term in the worst order
    is far above what a tree or blocked sum reaches; 1e-7 sum |terms| is one ulp of the magnitude the accumulator passed through)"""
    return 1e-7 * terms.abs().sum(dim)


# ---------------------------------------------------------------------------------------------------------------------------
# products (gemm_nt / gemm_tn / conv_nhwc / lowrank_nn)
# ---------------------------------------------------------------------------------------------------------------------------
U24 = 2.0 ** -24
# fp32 accumulation of a K-term product: one rounding of at most 2^-24 |partial sum| per accumulator update (K/32 .. K/4 MFMA steps, K/1024
# per lane in the skinny kernel, plus the fp32 products' own rounding in fp32 mode).  The partial sums of a random-signed reduction stay near
# ||(a_k b_k)||_2 and the roundings are independent, so their sum grows as sqrt(updates) <= sqrt(K); C_ACC = 8 covers the partial sums'
# excursions above the 2-norm.  A one-sided reduction (all terms of one sign) is not bounded by this and is not used.
C_ACC = 8.0
# cmpc_tanh (cmpc_common.h): the bound documented there, which test_gpu_ops_gemm's tanh sweep checks over every float32 with |x| in [2^-12, 16)
TANH_ABS, TANH_REL = 1.2e-7, 1e-6


def prod_norm(A, B):
    """||(a_mk b_nk)_k||_2 for every (m, n): sqrt((A o A) (B o B)^T) in float64; A [..., M, K], B [..., N, K]"""
    A, B = A.double(), B.double()
    return torch.sqrt((A * A) @ (B * B).transpose(-1, -2))


def acc_atol(norm, K, alpha=1.0):
    """the fp32-accumulation term of a product element: C_ACC 2^-24 sqrt(K) |alpha| ||(a_k b_k)||_2"""
    return C_ACC * U24 * math.sqrt(max(K, 1)) * abs(alpha) * norm


def epi_atol(pre_mag, act=0, y=None, c0=None):
    """epilogue term: the fp32 evaluation of alpha acc + bias + sbias + pbias (a rounding per operation over the magnitude pre_mag = |alpha
    acc| + |bias| + |sbias| + |pbias| it passes through; every activation is 1-Lipschitz, so that error carries through), the activation's
    own error at its float64 output y (relu exact, tanh as documented for cmpc_tanh, sigmoid: expf and a division) and the accumulate add
    of c0"""
    e = 4 * U24 * pre_mag
    if act == 2:
        e = e + TANH_ABS + TANH_REL * y.abs()
    elif act == 3:
        e = e + 4 * U24
    if c0 is not None:
        e = e + U24 * ((y.abs() if y is not None else 0) + c0.abs())
    return e


def assert_prod(got, ref, dt_out, K, norm, alpha=1.0, epi=0.0, what="", old_tol=None):
    """|got - ref| <= u_out |ref| + C_ACC 2^-24 sqrt(K) |alpha| ||(a_k b_k)||_2 + epi on every element (u_out: one ulp of a 16-bit output, 0
    for fp32).  old_tol: the whole-tensor bound an older test (U.rel_err: max |err| / max |ref|) puts on the same product -- this bound
    must be at least as strict there, which is asserted on the reference itself."""
    ref = ref.detach().double().cpu()
    atol = acc_atol(norm.detach().double().cpu(), K, alpha) + (epi.detach().double().cpu() if torch.is_tensor(epi) else epi)
    if old_tol is not None and ref.numel():
        mx = float(ref.abs().max())
        worst = float((1e-7 * mx + SUBNORMAL.get(dt_out, 0.0) + atol + ULP[dt_out] * ref.abs()).max())
        assert worst <= old_tol * mx, f"{what}: per-element bound {worst / mx:.3g} of max|ref| is looser than the old {old_tol:g}"
    assert_close(got, ref, dt_out, K=K, what=what, rtol=ULP[dt_out], atol=atol)


def assert_zero(t, what=""):
    t = t.detach().cpu()
    assert bool((t == 0).all()), f"{what}: pad elements not written as 0 ({int((t != 0).sum())} non-zero)"


def run_twice(fn):
    """fn() launches on fresh buffers and returns a dict of output tensors; it runs twice and every output must match bit for bit
    (DESIGN: fixed-order reductions, no atomics on floats).  Returns the first run's outputs."""
    a = fn()
    b = fn()
    torch.cuda.synchronize()
    for k in a:
        x, y = a[k], b[k]
        assert torch.equal(_bits(x) if x.is_floating_point() else x, _bits(y) if y.is_floating_point() else y), \
            f"{k}: two runs on the same inputs differ"
    return a


def bilinear_axis(n_in, n_out):
    """legacy resize_bilinear coefficients as the TF kernel computes them (interp_coef of ops_score.hip / ops_decoder.hip): in = out_idx *
    (in / out) in float32, lo = floor(in), hi = min(lo + 1, in - 1), lerp = in - lo (float32, returned as float64)"""
    src = torch.arange(n_out, dtype=torch.float32) * torch.tensor(n_in / n_out, dtype=torch.float32)
    lo = torch.floor(src)
    return lo.long(), torch.clamp(lo.long() + 1, max=n_in - 1), (src - lo).double()


# ----------------------------------------------------------------------------------------------------------------------------
# shapes
# ----------------------------------------------------------------------------------------------------------------------------
# (B, N, C, ld): rows per sample N in {1, 3, 49, 1600, 4096} (4096 > 4 x the largest rows_grid cap: the grid strides), the C/ld
# pairs (24, 64), (1000, 1024), (513, 520), (1025, 1032), (2047, 2048), and B in {1, 3, 8}
MAP_SHAPES = [
    (1, 1, 24, 64),
    (3, 49, 1000, 1024),
    (8, 3, 513, 520),
    (2, 4096, 24, 64),
    (1, 1600, 1025, 1032),
    (3, 7, 2047, 2048),
    (8, 49, 72, 136),
]


def shape_id(s):
    return "B%d-N%d-C%d-ld%d" % s


def clip_shapes(max_ld):
    """MAP_SHAPES clipped to an entry point's own ld limit (C clipped with it, keeping a pad tail)"""
    out = []
    for B, N, C, ld in MAP_SHAPES:
        if ld > max_ld:
            ld2 = max_ld
            C = min(C, ld2 - 1) if C < ld else ld2
            ld = ld2
        if (B, N, C, ld) not in out:
            out.append((B, N, C, ld))
    return out
