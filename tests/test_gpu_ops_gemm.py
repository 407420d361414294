"""Op-level tests of the contraction kernels of csrc/gemm.hip and csrc/ops_fusion.hip against float64 references: every cmpc_gemm_nt pipeline
in each storage type it serves (the dispatch mirrored below and confirmed by the launch trace), cmpc_gemm_nt_pair, cmpc_gemm_tn with plain
and convolution addressing, cmpc_gemm_tn_grouped under both plans, cmpc_lowrank_nn and cmpc_adam_step.

Inputs are seeded on the CPU; 16-bit operands are upcast for the reference, never regenerated.  Each output element is held to
opref.assert_prod: one ulp of a 16-bit output + the fp32-accumulation term C_ACC 2^-24 sqrt(K) |alpha| ||(a_k b_k)||_2 + the epilogue's
rounding.  Outputs carry sentinel guard rows and sentinel pad columns [N, ldc); operand pad columns [K, lda) hold NaN, so a read past K
shows.  Products above ~0.1 GMAC take their float64 reference on the GPU (torch float64 matmul) to keep the suite short."""
import ctypes
import math
import zlib

import pytest
import torch

from tests import opref as R
from tests import opwrap as W

pytestmark = pytest.mark.gpu

F32, BF16, F16 = R.F32, R.BF16, R.F16
_lib = R._lib
TRACE = {"skinny8": "gemm_nt(skinny)", "skinny16": "gemm_nt(skinny)", "64x64": "gemm_nt(64x64)", "128x128": "gemm_nt",
         "128x64": "gemm_nt", "v4-128": "gemm_nt(v4/v3)", "v4-256": "gemm_nt(v4/v3)", "v3-128": "gemm_nt(v4/v3)",
         "v3-256": "gemm_nt(v4/v3)", "v5": "gemm_nt(v5)"}
PIPES = {F32: {"skinny8", "skinny16", "64x64", "128x128", "128x64"},
         BF16: {"128x128", "128x64", "v4-128", "v4-256", "v3-128", "v3-256", "v5"},
         F16: {"128x128", "128x64", "v4-128", "v4-256", "v3-128", "v3-256", "v5"}}


def nt_pipeline(dt, M, N, Ks, batch, ldas, ldbs):
    """which kernel cmpc_gemm_nt launches (mirror of cmpc_gemm_nt / launch_nt_small / launch_nt16, csrc/gemm.hip)"""
    if dt == F32 and M <= 16 and batch == 1:
        return "skinny8" if M <= 8 else "skinny16"
    if dt == F32 or not (N >= 128 and M >= 512):
        bn = 128 if (N % 128 == 0 or N > 64) else 64
        tiles128 = -(-N // bn) * -(-M // 128) * batch
        if dt == F32 and tiles128 < 192:
            return "64x64"
        return "128x128" if bn == 128 else "128x64"
    off32 = all(M * la * 2 < 2 ** 32 and N * lb * 2 < 2 ** 32 for la, lb in zip(ldas, ldbs))
    if N >= 1024 and M >= 2048 and off32:
        return "v5"
    big = -(-M // 256) * -(-N // 128) * batch >= 192
    ktot = sum(Ks)
    v4 = ktot < 2048 or (ktot < 4096 and N >= 1024)
    return ("v4" if v4 else "v3") + ("-256" if big else "-128")


PAD = 8                              # operand pad columns past K: 16 B (16-bit) / 32 B (fp32)


# (pipeline, dtypes, M, N, Ks, batch, ldc, n_valid, rows_per_sample, shared_B): every case uses bias + sbias + pbias; lda / ldb = K + 8
# with NaN in the pad; in the batched cases rows_per_sample does not divide M, so sbias and pbias rows run on across the batch; the act parameter also picks the output type and accumulate (see _variant)
NT_CASES = [
    ("skinny8", (F32,), 7, 300, (64, 32), 1, 308, 290, 3, True),
    ("skinny16", (F32,), 13, 1028, (1024,), 1, 1028, 1028, 13, True),
    ("64x64", (F32,), 300, 132, (64, 96), 3, 140, 130, 120, False),
    ("128x128", (F32,), 3000, 1024, (64,), 1, 1032, 1000, 1000, True),
    ("128x64", (F32,), 6100, 60, (32,), 4, 64, 60, 64, False),
    ("128x128", (BF16, F16), 300, 256, (128, 64), 2, 260, 250, 200, False),
    ("128x64", (BF16, F16), 1000, 44, (64,), 1, 52, 40, 100, True),
    ("v4-128", (BF16, F16), 700, 264, (128, 64), 1, 268, 260, 70, True),
    ("v3-128", (BF16, F16), 900, 388, (4160,), 1, 396, 388, 300, True),
    ("v4-256", (BF16, F16), 6001, 1004, (192, 64), 1, 1012, 1000, 6001, True),
    ("v3-256", (BF16, F16), 1000, 640, (2048,), 10, 644, 636, 300, False),
    ("v5", (BF16, F16), 2100, 1028, (128, 64, 64), 1, 1036, 1020, 700, True),     # gx = 5: the strip order's remainder
    ("v5", (BF16, F16), 2048, 2048, (256,), 2, 2048, 2040, 1000, False),         # gx = 8, batched
]
NT_PARAMS = [pytest.param(c, dt, act, id="%s-%s-%s-act%d" % (c[0], R.DT_IDS[dt], "x".join(map(str, c[4])), act))
             for c in NT_CASES for dt in c[1] for act in (0, 1, 2, 3)]


def _variant(dt, act):
    """(c_f32, accumulate, alpha) of a case run: every pipeline sees both output types (act 0 and 3 with c_f32, 1 and 2 in the storage type),
    accumulate on and off into each, alpha 1 and not"""
    c_f32 = dt != F32 and act in (0, 3)
    return c_f32, act in (0, 1), (1.0 if act in (0, 3) else 0.75)


# the whole-tensor bounds (U.rel_err) the older tests (test_gpu_parity.py) put on the same kind of product, by (operand dtype, output dtype):
# act none and relu, 16-bit outputs 1e-2 (bf16) / 2e-3 (f16), fp32 outputs of 16-bit operands 1e-5, fp32 5e-6
OLD_TOL = {(BF16, BF16): 1e-2, (F16, F16): 2e-3, (BF16, F32): 1e-5, (F16, F32): 1e-5, (F32, F32): 5e-6}


def _mat(shape, dt, g, scale=1.0, ld=None):
    """seeded storage-dtype matrix with NaN pad columns [shape[-1], ld)"""
    x = torch.randn(*shape, generator=g, dtype=torch.float64) * scale
    if ld is not None and ld > shape[-1]:
        x = torch.cat([x, torch.full(shape[:-1] + (ld - shape[-1],), float("nan"), dtype=torch.float64)], -1)
    return x.to(R.TDT[dt])


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % 100003


def _ref_dev(macs):
    return R.DEV if macs > 1e8 else "cpu"


def nt_args(dt, segs, C, ldc, M, N, n_valid, batch=1, sC=0, c_f32=False, bias=None, sbias=None, ld_sbias=0, pbias=None, ld_pbias=0,
            rps=0, act=0, alpha=1.0, accumulate=False):
    a = _lib.GemmNtArgs()
    a.dtype, a.nseg = dt, len(segs)
    for i, (A, lda, Bt, ldb, K, sA, sB) in enumerate(segs):
        a.A[i], a.lda[i], a.Bt[i], a.ldb[i], a.K[i], a.sA[i], a.sB[i] = W._p(A), lda, W._p(Bt), ldb, K, sA, sB
    a.C, a.ldc, a.sC, a.c_f32 = W._p(C), ldc, sC, int(c_f32)
    a.M, a.N, a.n_valid, a.batch = M, N, n_valid, batch
    a.bias, a.sbias, a.ld_sbias, a.pbias, a.ld_pbias = W._p(bias), W._p(sbias), ld_sbias, W._p(pbias), ld_pbias
    a.rows_per_sample, a.act, a.alpha, a.accumulate = rps, act, alpha, int(accumulate)
    return a


def _act64(x, act):
    return {0: lambda v: v, 1: torch.relu, 2: torch.tanh, 3: torch.sigmoid}[act](x)


class NtProblem:
    """one gemm_nt problem: CPU inputs, device buffers, the float64 reference and its tolerance terms"""

    def __init__(self, dt, M, N, Ks, batch, ldc, nv, rps, shared_B, act, c_f32, acc, alpha, seed, onehot=False, A_big=None):
        g = R.gen(seed)
        self.dt, self.M, self.N, self.Ks, self.batch, self.ldc, self.nv, self.rps = dt, M, N, Ks, batch, ldc, nv, rps
        self.act, self.c_f32, self.acc, self.alpha = act, c_f32, acc, alpha
        self.out_dt = F32 if (c_f32 or dt == F32) else dt
        self.ldas = [k + PAD for k in Ks]
        self.ldbs = [k + PAD for k in Ks]
        nB = 1 if shared_B else batch
        if onehot:                   # A rows one-hot: every product term is exact, acc[m, n] = Bt[n, k(m)]
            self.A = []
            for K, la in zip(Ks, self.ldas):
                a = torch.zeros(batch, M, la, dtype=torch.float64)
                a[..., K:] = float("nan")
                self.A.append(a.to(R.TDT[dt]))
            k = torch.randint(0, Ks[0], (batch, M), generator=g)
            self.A[0].view(batch * M, -1)[torch.arange(batch * M), k.view(-1)] = 1
        else:
            self.A = [_mat((batch, M, K), dt, g, 1.0, la) for K, la in zip(Ks, self.ldas)]
        sc = 1.0 / math.sqrt(sum(Ks))
        self.B = [_mat((nB, N, K), dt, g, sc, lb) for K, lb in zip(Ks, self.ldbs)]
        ns = -(-batch * M // rps)
        self.ld_sb, self.ld_pb = N + 4, N + 8
        self.bias = (torch.randn(N, generator=g, dtype=torch.float64) * 0.5).float()
        self.sbias = (torch.randn(ns, self.ld_sb, generator=g, dtype=torch.float64) * 0.5).float()
        self.pbias = (torch.randn(rps, self.ld_pb, generator=g, dtype=torch.float64) * 0.5).float()
        self.C0 = _mat((batch * M, N), self.out_dt, g, 1.0) if acc else None
        self.sA = [M * la for la in self.ldas]
        self.sB = [0 if shared_B else N * lb for lb in self.ldbs]
        self.d_A = [a.to(R.DEV) for a in self.A] if A_big is None else A_big
        self.d_B = [b.to(R.DEV) for b in self.B]
        self.d_bias, self.d_sb, self.d_pb = self.bias.to(R.DEV), self.sbias.to(R.DEV), self.pbias.to(R.DEV)

    def pipeline(self):
        return nt_pipeline(self.dt, self.M, self.N, self.Ks, self.batch, self.ldas, self.ldbs)

    def fresh_C(self):
        C = R.guarded(self.batch * self.M, self.ldc, self.out_dt)
        if self.C0 is not None:
            C[:self.batch * self.M, :self.N] = self.C0.to(R.DEV)
        return C

    def args(self, C):
        segs = [(A, la, Bt, lb, K, sa, sb) for A, la, Bt, lb, K, sa, sb in zip(self.d_A, self.ldas, self.d_B, self.ldbs, self.Ks, self.sA, self.sB)]
        return nt_args(self.dt, segs, C, self.ldc, self.M, self.N, self.nv, self.batch, self.M * self.ldc, self.c_f32, self.d_bias, self.d_sb,
                       self.ld_sb, self.d_pb, self.ld_pb, self.rps, self.act, self.alpha, self.acc)

    def reference(self):
        """(ref [batch*M, N] float64, norm, pre_mag, y) on the CPU"""
        M, N, b = self.M, self.N, self.batch
        dev = _ref_dev(b * M * N * sum(self.Ks))
        acc = torch.zeros(b, M, N, dtype=torch.float64, device=dev)
        nrm = torch.zeros_like(acc)
        for A, B, K in zip(self.A, self.B, self.Ks):
            a = A[..., :K].to(dev).double()
            bb = B[..., :K].to(dev).double()
            acc += a @ bb.transpose(-1, -2)
            nrm += (a * a) @ (bb * bb).transpose(-1, -2)
        acc = acc.reshape(b * M, N).cpu()
        nrm = nrm.reshape(b * M, N).sqrt().cpu()
        idx = torch.arange(b * M)
        sb = self.sbias.double()[idx // self.rps, :N]
        pb = self.pbias.double()[idx % self.rps, :N]
        bias = self.bias.double()[:N]
        pre = self.alpha * acc + bias + sb + pb
        pre_mag = abs(self.alpha) * acc.abs() + bias.abs() + sb.abs() + pb.abs()
        y = _act64(pre, self.act)
        y[:, self.nv:] = 0
        ref = y + self.C0.double() if self.C0 is not None else y
        return ref, nrm, pre_mag, y

    def check(self, C, what, onehot=False):
        rows = self.batch * self.M
        R.assert_guard(C, rows, what)
        R.assert_sentinel(C[:rows, self.N:], what + " pad columns [N, ldc)")
        got = C[:rows, :self.N].cpu()
        ref, nrm, pre_mag, y = self.reference()
        nv = self.nv
        # pad columns: exactly zero, or exactly C0 when accumulating
        pad_ref = self.C0[:, nv:] if self.C0 is not None else torch.zeros(rows, self.N - nv, dtype=got.dtype)
        assert torch.equal(R._bits(got[:, nv:].contiguous()), R._bits(pad_ref.to(got.dtype).contiguous())), f"{what}: pad columns >= n_valid"
        epi = R.epi_atol(pre_mag, self.act, y, self.C0.double() if self.C0 is not None else None)[:, :nv]
        if onehot:
            R.assert_close(got[:, :nv], ref[:, :nv], self.out_dt, what=what + " (one-hot: exact products)", rtol=R.ULP[self.out_dt], atol=epi)
        else:
            old = OLD_TOL[(self.dt, self.out_dt)] if self.act in (0, 1) else None
            R.assert_prod(got[:, :nv], ref[:, :nv], self.out_dt, sum(self.Ks), nrm[:, :nv], self.alpha, epi, what, old_tol=old)


def _run_nt(p, expect_trace=True):
    def run():
        C = p.fresh_C()
        with W.LaunchTrace() as t:
            _lib.call("cmpc_gemm_nt", ctypes.byref(p.args(C)), W._st())
        torch.cuda.synchronize()
        run.trace = t
        return {"C": C}
    C = R.run_twice(run)["C"]
    if expect_trace:
        name = TRACE[p.pipeline()]
        assert run.trace.names == [name] and run.trace.counts[name] == 1, (p.pipeline(), run.trace.counts)
    return C


# ---------------------------------------------------------------------------------------------------------------------------
def test_nt_pipeline_table():
    """every gemm_nt pipeline is reached, in each storage type that serves it, by at least one case of test_gemm_nt (whose launch trace
    confirms the mirror's answer), and the one-hot epilogue cases reach skinny, small, v4 and v5"""
    seen = {dt: set() for dt in R.DTS}
    for name, dts, M, N, Ks, batch, *_ in NT_CASES:
        for dt in dts:
            p = nt_pipeline(dt, M, N, Ks, batch, [k + 8 for k in Ks], [k + 8 for k in Ks])
            assert p == name, (name, R.DT_IDS[dt], p)
            seen[dt].add(p)
    for dt in R.DTS:
        assert seen[dt] == PIPES[dt], (R.DT_IDS[dt], PIPES[dt] - seen[dt])
    assert {c[0] for c in ONEHOT} >= {"skinny8", "128x128", "v4-256", "v5"}
    # the off32 fallback: v5's shape with an operand view past 2^32 bytes goes to v4
    assert nt_pipeline(F16, 2048, 1024, (64,), 1, [OFF32_LDA], [72]) == "v4-128"
    assert nt_pipeline(F16, 2048, 1024, (64,), 1, [72], [72]) == "v5"


@pytest.mark.parametrize("case,dt,act", NT_PARAMS)
def test_gemm_nt(case, dt, act):
    """cmpc_gemm_nt (cmpc.h:37-57) per pipeline: 1-3 K-segments with lda > K, ragged M / N, ldc > N (16-bit: ldc % 8 == 4 on some),
    batch with sA / sB / sC and sbias running on across the batch, bias + sbias + pbias, alpha, accumulate into 16-bit and fp32 C, c_f32,
    n_valid < N, acts 0-3"""
    name, _, M, N, Ks, batch, ldc, nv, rps, shared = case
    c_f32, acc, alpha = _variant(dt, act)
    p = NtProblem(dt, M, N, Ks, batch, ldc, nv, rps, shared, act, c_f32, acc, alpha, seed=_seed(name, M, dt, act))
    assert p.pipeline() == name
    C = _run_nt(p)
    p.check(C, f"gemm_nt {name} {R.DT_IDS[dt]} act {act}")


OFF32_LDA = (1 << 20) + 64


def test_gemm_nt_off32_fallback():
    """v5's shape (N >= 1024, M >= 2048) with an A view whose rows span more than 2^32 bytes (M lda 2 >= 2^32): v5's 32-bit byte offsets
    would overflow, so cmpc_gemm_nt takes the v4 pipeline (launch_nt16 off32).  One ~4 GiB f16 allocation of which only K columns of each
    row are written and read."""
    dt, M, N, K = F16, 2048, 1024, 64
    lda = OFF32_LDA
    big = torch.empty(M * lda, dtype=torch.float16, device=R.DEV)
    view = big.as_strided((M, K + 8), (lda, 1))
    p = NtProblem(dt, M, N, (K,), 1, N + 4, N - 8, 512, True, 2, False, True, 0.5, seed=77, A_big=[big])
    view.copy_(p.A[0][0].to(R.DEV))
    p.ldas = [lda]
    p.sA = [0]
    assert p.pipeline() == "v4-128"
    C = _run_nt(p)
    p.check(C, "gemm_nt off32 fallback")
    del big, view


# (pipeline, dt, M, N, K, batch, rps): one-hot A -- exact products, so alpha acc + biases is known exactly and the epilogue is checked at
# a few fp32 ulps
ONEHOT = [("skinny8", F32, 8, 520, 32, 1, 4), ("64x64", F32, 130, 96, 32, 2, 60), ("128x128", BF16, 300, 256, 64, 1, 100),
          ("v4-256", BF16, 6001, 1004, 64, 1, 6001), ("v4-256", F16, 6001, 1004, 64, 1, 3000), ("v5", F16, 2100, 1028, 64, 1, 700),
          ("v5", BF16, 2048, 1280, 64, 2, 1500)]


@pytest.mark.parametrize("case", ONEHOT, ids=lambda c: "%s-%s" % (c[0], R.DT_IDS[c[1]]))
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_gemm_nt_epilogue_onehot(case, act):
    name, dt, M, N, K, batch, rps = case
    for c_f32 in ((False, True) if dt != F32 else (False,)):
        p = NtProblem(dt, M, N, (K,), batch, N + 4, N - 4, rps, batch == 1, act, c_f32, act == 1, 1.25, seed=31 + act, onehot=True)
        assert p.pipeline() == name
        C = _run_nt(p)
        p.check(C, f"gemm_nt epilogue {name} act {act} c_f32 {c_f32}", onehot=True)


# (dt, M, N, trace name) of the tanh sweeps: one launch covers M N preactivations
TANH_PIPES = {"64x64-f32": (F32, 256, 1024, "gemm_nt(64x64)"), "v5-bf16-c_f32": (BF16, 2048, 4096, "gemm_nt(v5)"),
              "v4-f16-c_f32": (F16, 8192, 1016, "gemm_nt(v4/v3)"), "128x64-bf16-c_f32": (BF16, 131072, 64, "gemm_nt")}


def _tanh_chunks(n):
    """device float32 chunks of at most n points: EVERY float32 x with |x| in [2^-12, 16) (16 binades, signs alternating: cmpc_tanh works on
    |x| and copies the sign), then a sample below 2^-12 (the polynomial, exact to a rounding there) and above 16 (where it returns 1)"""
    lo = int(R._bits(torch.tensor([2.0 ** -12], dtype=torch.float32))[0])
    hi = int(R._bits(torch.tensor([16.0], dtype=torch.float32))[0])
    for b in range(lo, hi, n):
        x = torch.arange(b, min(b + n, hi), dtype=torch.int32, device=R.DEV).view(torch.float32)
        yield torch.where(torch.arange(x.numel(), device=R.DEV) % 2 == 1, -x, x)
    tail = torch.cat([torch.logspace(-30, -12, 4096, dtype=torch.float64), torch.logspace(math.log10(16), 30, 4096, dtype=torch.float64)])
    yield torch.cat([tail, -tail]).float().to(R.DEV)


@pytest.mark.parametrize("pipe", list(TANH_PIPES))
def test_gemm_nt_tanh_epilogue(pipe):
    """ACT_TANH in the MFMA epilogues is cmpc_tanh (cmpc_common.h).  The preactivation is pbias exactly (A = 0, so acc = 0) and runs over
    every float32 with |x| in [2^-12, 16), the 1/8 branch point and the binade above it (where 1 - 2/(e+1) cancels) included; the error
    against float64 tanh must stay within the bound documented there: |error| <= TANH_ABS and <= TANH_REL |tanh x|"""
    dt, M, N, trace = TANH_PIPES[pipe]
    K = 64 if dt != F32 else 32
    A = torch.zeros(M, K, dtype=R.TDT[dt], device=R.DEV)
    Bt = torch.zeros(N, K, dtype=R.TDT[dt], device=R.DEV)
    pb = torch.empty(M, N, dtype=torch.float32, device=R.DEV)
    C = R.guarded(M, N, F32)
    a = nt_args(dt, [(A, K, Bt, K, K, 0, 0)], C, N, M, N, N, c_f32=dt != F32, pbias=pb, ld_pbias=N, rps=M, act=2)
    max_abs = max_rel = 0.0
    n_bad, bad_x, launches = 0, [], 0
    with W.LaunchTrace() as t:
        for x in _tanh_chunks(M * N):
            n = x.numel()
            pb.view(-1)[:n] = x
            pb.view(-1)[n:] = 0.5
            _lib.call("cmpc_gemm_nt", ctypes.byref(a), W._st())
            launches += 1
            ref = torch.tanh(x.double())
            err = (C[:M].reshape(-1)[:n].double() - ref).abs()
            max_abs = max(max_abs, float(err.max()))
            max_rel = max(max_rel, float((err / ref.abs()).max()))
            bad = (err > R.TANH_ABS) | (err > R.TANH_REL * ref.abs())
            if bool(bad.any()):
                n_bad += int(bad.sum())
                bad_x += x[bad][:4].tolist()
    assert t.names == [trace] and t.counts[trace] == launches, (t.names, t.counts)
    R.assert_guard(C, M, "tanh")
    print(f"cmpc_tanh {pipe}: max abs err {max_abs:.4g}, max rel err {max_rel:.4g} over {launches} launches")
    assert n_bad == 0, f"cmpc_tanh outside its documented bound at {n_bad} points, e.g. x = {bad_x[:8]} (max abs {max_abs:.3g}, rel {max_rel:.3g})"


def test_gemm_nt_pair():
    """cmpc_gemm_nt_pair (cmpc.h:58-60): two products of different shapes on the 256 x 128 v4 pipeline in one launch; a first product
    whose tile count is not a multiple of 8 falls back to two launches.  Both against float64."""
    for (M1, N1), (M2, N2), trace in (((6144, 1000), (12288, 512), {"gemm_nt(pair)": 1}),
                                      ((7100, 840), (6144, 1000), {"gemm_nt(v4/v3)": 2})):
        for dt in (BF16, F16):
            ps = [NtProblem(dt, M, N, (128,), 1, N + 4, N - 4, M, True, act, False, False, 1.0, seed=M + act)
                  for (M, N), act in (((M1, N1), 1), ((M2, N2), 2))]

            def run():
                Cs = [p.fresh_C() for p in ps]
                with W.LaunchTrace() as t:
                    _lib.call("cmpc_gemm_nt_pair", ctypes.byref(ps[0].args(Cs[0])), ctypes.byref(ps[1].args(Cs[1])), W._st())
                torch.cuda.synchronize()
                run.counts = t.counts
                return {"C1": Cs[0], "C2": Cs[1]}
            o = R.run_twice(run)
            assert run.counts == trace, run.counts
            ps[0].check(o["C1"], "gemm_nt_pair first")
            ps[1].check(o["C2"], "gemm_nt_pair second")


# ---------------------------------------------------------------------------------------------------------------------------
# gemm_tn
# ---------------------------------------------------------------------------------------------------------------------------
class TnProblem:
    """out[k, n] (+)= alpha sum_r A[r, k] D[r, n] with inner batch offsets and an outer batch; out is pre-filled (random) and every
    element outside the written regions must come back unchanged"""

    def __init__(self, dt, R_, Kv, Nv, seed, Ka=None, nb=1, nb2=1, shared_out=False, alpha=1.0, rsplit=None, conv=None, out=None):
        g = R.gen(seed)
        self.dt, self.R, self.Kv, self.Nv, self.nb, self.nb2, self.alpha, self.rsplit, self.conv = dt, R_, Kv, Nv, nb, nb2, alpha, rsplit, conv
        self.Ka = Kv if Ka is None else Ka
        e = 8
        self.kp, self.np_ = -(-max(Kv, self.Ka) // e) * e, -(-Nv // e) * e
        # inner entries side by side in the columns of A / D / out (a_off / d_off / o_off), outer entries stacked (a_bs / d_bs / o_bs)
        self.lda, self.ldd = nb * self.kp + 8, nb * self.np_ + 8
        self.ldo = nb * self.np_ + 4
        self.A = _mat((nb2, max(R_, 1), nb * self.kp), dt, g, 1.0, self.lda)
        self.D = _mat((nb2, max(R_, 1), nb * self.np_), dt, g, 1.0, self.ldd)
        self.a_bs, self.d_bs = max(R_, 1) * self.lda, max(R_, 1) * self.ldd
        self.orows = self.kp if shared_out else nb2 * self.kp
        self.o_bs = 0 if shared_out else self.kp * self.ldo
        self.out0 = torch.randn(self.orows, self.ldo, generator=g, dtype=torch.float64).float()
        self.offs = [(i * self.kp, i * self.np_, i * self.np_) for i in range(nb)]
        self.d_A, self.d_D = self.A.to(R.DEV), self.D.to(R.DEV)
        self.out = out

    def fresh_out(self):
        return R.guarded(self.orows, self.ldo, F32, self.out0)

    def launch(self, out, wg=None):
        W.gemm_tn(self.dt, self.d_A, self.lda, self.Ka, self.d_D, self.ldd, self.np_, out, self.ldo, self.R, self.Kv, self.Nv, offs=self.offs,
                  nb2=self.nb2, a_bs=self.a_bs, d_bs=self.d_bs, o_bs=self.o_bs, alpha=self.alpha, rsplit=self.rsplit, wg=wg, conv=self.conv)

    def shifted_A(self, b2, i):
        """float64 [R, Kv] rows of A entry (b2, i) as the kernel reads them: columns >= Ka zero; conv: the input pixel (y + dy, x + dx)"""
        a = self.A[b2, :self.R, i * self.kp:i * self.kp + self.Kv].double().clone()
        a[:, self.Ka:] = 0
        if self.conv is None:
            return a
        H, Wd, dy, dx = self.conv
        x = a.reshape(-1, H, Wd, self.Kv)
        s = torch.zeros_like(x)
        ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(Wd, Wd - dx))
        yt, xt = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(Wd, Wd + dx))
        if ys.start < ys.stop and xs.start < xs.stop:
            s[:, ys, xs] = x[:, yt, xt]
        return s.reshape(self.R, self.Kv)

    def reference(self):
        """(ref [orows, ldo] float64 of the whole out buffer, norm of the same shape)"""
        ref = self.out0.double().clone()
        nrm = torch.zeros_like(ref)
        self.touched = torch.zeros(ref.shape, dtype=torch.bool)
        for b2 in range(self.nb2):
            ob = 0 if self.o_bs == 0 else b2 * self.kp
            for i, (_, _, oo) in enumerate(self.offs):
                if self.R == 0:
                    continue
                a = self.shifted_A(b2, i)
                d = self.D[b2, :self.R, i * self.np_:i * self.np_ + self.Nv].double()
                self.touched[ob:ob + self.Kv, oo:oo + self.Nv] = True
                ref[ob:ob + self.Kv, oo:oo + self.Nv] += self.alpha * (a.t() @ d)
                nrm[ob:ob + self.Kv, oo:oo + self.Nv] += (a * a).t() @ (d * d)
        return ref, nrm.sqrt()

    def check(self, out, what):
        R.assert_guard(out, self.orows, what)
        ref, nrm = self.reference()
        got = out[:self.orows].cpu()
        assert torch.equal(R._bits(got[~self.touched]), R._bits(self.out0[~self.touched])), f"{what}: out written outside [Kv, Nv] regions"
        nred = self.R * (1 if self.o_bs else self.nb2)
        # out0 is added in fp32: one more rounding of |out0| + |product|
        epi = R.U24 * (self.out0.double().abs() + (ref - self.out0.double()).abs())
        R.assert_prod(got, ref, F32, max(nred, 1), nrm, self.alpha, epi, what)


TN_DT = pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)


@TN_DT
@pytest.mark.parametrize("shape", [
    dict(R_=1000, Kv=200, Nv=136, alpha=0.5),                 # Kv / Nv ragged against 128
    dict(R_=700, Kv=100, Nv=72, Ka=64),                       # Ka < Kv: rows [Ka, Kv) of out get zeros
    dict(R_=0, Kv=64, Nv=64),                                 # empty reduction: out unchanged
    dict(R_=517, Kv=64, Nv=40, rsplit=1),
    dict(R_=517, Kv=136, Nv=200, rsplit=2, alpha=-1.5),
    dict(R_=517, Kv=64, Nv=64, rsplit=7),
    dict(R_=100, Kv=64, Nv=64, rsplit=64),                    # more splits than row blocks: some splits are empty
    dict(R_=300, Kv=40, Nv=24, nb=8, rsplit=3),               # inner batch of 8 with distinct o_off
    dict(R_=257, Kv=72, Nv=136, nb=3),
    dict(R_=250, Kv=64, Nv=48, nb2=3, alpha=2.0),             # outer batch, o_bs != 0
    dict(R_=250, Kv=64, Nv=48, nb2=4, shared_out=True),       # outer batch into one output (o_bs == 0): slabs
    dict(R_=250, Kv=64, Nv=48, nb2=2, shared_out=True, rsplit=3),
], ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()))
def test_gemm_tn(dt, shape):
    """cmpc_gemm_tn (cmpc.h:61-79) against float64, fp32 out accumulated in place"""
    p = TnProblem(dt, seed=_seed(sorted(shape.items()), dt), **shape)

    def run():
        out = p.fresh_out()
        p.launch(out)
        torch.cuda.synchronize()
        return {"out": out}
    p.check(R.run_twice(run)["out"], f"gemm_tn {shape}")


CONV_TN = [(2, 7, 9, 1), (2, 7, 9, 2), (1, 6, 8, 8), (3, 5, 5, 4)]     # (B, H, W, dilation): dilation 8 >= H: only the centre tap sees pixels


@TN_DT
@pytest.mark.parametrize("geo", CONV_TN, ids=lambda g: "B%d-H%d-W%d-d%d" % g)
def test_gemm_tn_conv_taps(dt, geo):
    """conv addressing (conv_H / conv_W / conv_dy / conv_dx): all nine taps of a 3x3 TF-SAME weight gradient, each its own cmpc_gemm_tn,
    against the input shifted and zero-padded explicitly; B > 1 so the row -> (b, y, x) wrap is exercised"""
    B, H, Wd, dil = geo
    for t in range(9):
        conv = (H, Wd, (t // 3 - 1) * dil, (t % 3 - 1) * dil)
        p = TnProblem(dt, B * H * Wd, 64 if dt != F32 else 40, 72, seed=100 + t, conv=conv, alpha=1.0 if t % 2 else 0.5,
                      rsplit=1 + t % 3)

        def run():
            out = p.fresh_out()
            p.launch(out)
            torch.cuda.synchronize()
            return {"out": out}
        p.check(R.run_twice(run)["out"], f"gemm_tn conv tap {t} {geo}")


def _grouped_mix():
    """short chains (<= 64 steps), a long chain (> 64 steps, through slabs), split products, conv taps, fp32 items, an empty reduction"""
    items = []
    items.append(TnProblem(BF16, 20000, 136, 128, seed=1))               # long: split
    items.append(TnProblem(F16, 3000, 64, 200, seed=2, nb=2))
    items.append(TnProblem(F32, 700, 72, 40, seed=3, alpha=0.5))
    items.append(TnProblem(F32, 0, 8, 8, seed=4))                        # empty
    items.append(TnProblem(BF16, 250, 64, 48, seed=5, nb2=3, shared_out=True))
    for t in range(9):                                                   # conv taps, 2 x 7 x 9 pixels, dilation 2
        items.append(TnProblem(BF16, 126, 64, 72, seed=10 + t, conv=(7, 9, (t // 3 - 1) * 2, (t % 3 - 1) * 2)))
    return items


@pytest.mark.parametrize("plan", ["balanced", "no_balance"])
def test_gemm_tn_grouped(plan, monkeypatch):
    """cmpc_gemm_tn_grouped (cmpc.h:80-84): a mix of products with independent outputs, a short chain (three products into one output,
    <= 64 steps: one workgroup walks it) and a long chain (four products into one output, > 64 steps: slabs and a fold), under the default
    plan and under CMPC_TN_NO_BALANCE (read per call); each within tolerance and bit-identical across two runs (the dynamic deal included)"""
    if plan == "no_balance":
        monkeypatch.setenv("CMPC_TN_NO_BALANCE", "1")
    solo = _grouped_mix()
    g = R.gen(9)
    # chains: products into one shared output of the same shape and alpha
    short = [TnProblem(BF16, r, 64, 64, seed=40 + i, alpha=0.5) for i, r in enumerate((200, 300, 500))]        # 4 + 5 + 8 = 17 steps
    long_ = [TnProblem(F16, r, 128, 136, seed=50 + i) for i, r in enumerate((3000, 2000, 1500, 900))]          # 47 + 32 + 24 + 15 > 64
    chains = []
    for ch in (short, long_):
        ldo = ch[0].ldo
        init = torch.randn(ch[0].orows, ldo, generator=g, dtype=torch.float64).float()
        chains.append((ch, init))

    def run():
        cx = type("Cx", (), {})()
        cx.deferred = []
        outs = {}
        for i, p in enumerate(solo):
            outs[f"solo{i}"] = p.fresh_out()
            p.launch(outs[f"solo{i}"], wg=cx)
        for c, (ch, init) in enumerate(chains):
            o = R.guarded(ch[0].orows, ch[0].ldo, F32, init)
            outs[f"chain{c}"] = o
            for p in ch:
                p.launch(o, wg=cx)
        W.gemm_tn_grouped(cx.deferred)
        torch.cuda.synchronize()
        return outs
    o = R.run_twice(run)
    for i, p in enumerate(solo):
        p.check(o[f"solo{i}"], f"grouped {plan} item {i}")
    for c, (ch, init) in enumerate(chains):
        out = o[f"chain{c}"]
        rows = ch[0].orows
        R.assert_guard(out, rows, f"grouped chain {c}")
        ref, n2, Rt = init.double().clone(), torch.zeros(rows, ch[0].ldo, dtype=torch.float64), 0
        for p in ch:
            p.out0 = torch.zeros_like(p.out0)
            r, n = p.reference()
            ref += r
            n2 += n * n
            Rt += p.R
        epi = R.U24 * len(ch) * (init.double().abs() + (ref - init.double()).abs())
        R.assert_prod(out[:rows].cpu(), ref, F32, Rt, n2.sqrt(), ch[0].alpha, epi, f"grouped {plan} chain {c}")


# ---------------------------------------------------------------------------------------------------------------------------
# lowrank_nn
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("N", [4, 8, 16, 64, 1024])
@pytest.mark.parametrize("Kv", [1, 7, 8, 9, 24])
def test_lowrank_nn(dt, N, Kv):
    """cmpc_lowrank_nn (cmpc.h:137-142): C[b][m, n] (+)= alpha sum_{k < Kv} A[b][m, k] Bk[b][k, n]; lda > 8 ceil(Kv / 8) with NaN beyond Kv
    in A and NaN rows beyond Kv in Bk, batch 3, alpha, accumulate on and off, n_valid < N (pad columns exactly 0 / C0), ldc > N"""
    g = R.gen(N * 31 + Kv)
    B, M = 3, 333
    kc = -(-Kv // 8)
    lda, ldb, ldc = 8 * kc + 8, N + 4, N + 4
    nv = N - 4 if N >= 8 else N
    A = _mat((B, M, Kv), dt, g, 1.0, lda)
    Bk = torch.cat([torch.randn(B, Kv, ldb, generator=g, dtype=torch.float64),
                    torch.full((B, 32 - Kv, ldb), float("nan"), dtype=torch.float64)], 1).to(R.TDT[dt])
    Bk[:, :Kv, N:] = float("nan")
    for acc, alpha in ((False, 1.0), (True, 0.375)):
        C0 = _mat((B * M, N), dt, g)
        dA, dB = A.to(R.DEV), Bk.to(R.DEV)

        def run():
            C = R.guarded(B * M, ldc, dt)
            if acc:
                C[:B * M, :N] = C0.to(R.DEV)
            with W.LaunchTrace() as t:
                W.lowrank_nn(dt, dA, lda, M * lda, dB, ldb, 32 * ldb, C, ldc, M * ldc, M, N, Kv, n_valid=nv, batch=B, alpha=alpha,
                             accumulate=acc)
            torch.cuda.synchronize()
            assert t.names == ["lowrank_nn"]
            return {"C": C}
        C = R.run_twice(run)["C"]
        R.assert_guard(C, B * M, "lowrank_nn")
        R.assert_sentinel(C[:B * M, N:], "lowrank_nn pad columns [N, ldc)")
        got = C[:B * M, :N].cpu()
        a = A[..., :Kv].double()
        w = Bk[:, :Kv, :N].double()
        prod = (a @ w).reshape(B * M, N)
        nrm = ((a * a) @ (w * w)).reshape(B * M, N).sqrt()
        ref = alpha * prod + (C0.double() if acc else 0)
        pad = C0[:, nv:] if acc else torch.zeros(B * M, N - nv, dtype=got.dtype)
        assert torch.equal(R._bits(got[:, nv:].contiguous()), R._bits(pad.contiguous())), "lowrank_nn: pad columns >= n_valid"
        epi = 2 * R.U24 * (abs(alpha) * prod.abs() + (C0.double().abs() if acc else 0))
        R.assert_prod(got[:, :nv], ref[:, :nv], dt, Kv, nrm[:, :nv], alpha, epi[:, :nv], f"lowrank_nn N {N} Kv {Kv} acc {acc}")


# ---------------------------------------------------------------------------------------------------------------------------
# adam_step
# ---------------------------------------------------------------------------------------------------------------------------
def test_adam_step():
    """cmpc_adam_step (cmpc.h:326-332): segments with their own wd / gmult (one longer than 256 k + r), gscale; inf / NaN gradients leave
    p / m / v untouched and are counted exactly in *nonfinite (which may be NULL); elements between segments are never touched.  Against a
    float64 TF-Adam step from the same float32 state, with the rounding of a float32 evaluation"""
    g = R.gen(21)
    n = 6000
    segs = [(0, 1000, 0.0, 1.0), (1024, 256 * 3 + 17, 5e-4, 2.0), (2000, 1, 1e-3, 1.0), (2048, 3000, 1e-2, 0.5)]
    p0 = torch.randn(n, generator=g, dtype=torch.float64).float()
    gr = (torch.randn(n, generator=g, dtype=torch.float64) * 10).float()
    m0 = (torch.randn(n, generator=g, dtype=torch.float64) * 0.1).float()
    v0 = (torch.rand(n, generator=g, dtype=torch.float64) * 0.01).float()
    bad_idx = torch.tensor([3, 999, 1010, 1024, 1500, 2000, 2048, 4000, 5047, 5500])     # 1010, 5500: between / after the segments
    gr[bad_idx[::2]] = float("inf")
    gr[bad_idx[1::2]] = float("nan")
    gr[5] = -float("inf")
    lr, b1, b2, eps, gs = 1e-3, 0.9, 0.999, 1e-8, 0.5
    arr = (_lib.AdamSeg * len(segs))()
    for i, (off, cnt, wd, gm) in enumerate(segs):
        arr[i].off, arr[i].count, arr[i].wd, arr[i].gmult = off, cnt, wd, gm
    segs_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(R.DEV)
    live = torch.zeros(n, dtype=torch.bool)
    wd_e, gm_e = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for off, cnt, wd, gm in segs:
        live[off:off + cnt] = True
        wd_e[off:off + cnt] = float(torch.tensor(wd, dtype=torch.float32))
        gm_e[off:off + cnt] = gm
    fin = torch.isfinite(gr)
    assert not live[1010] and not live[5500] and not fin[1010] and not fin[5500]    # non-finite gradients outside every segment: not counted
    n_bad = int((live & ~fin).sum())
    for with_count in (True, False):
        def run():
            P, G, Mm, V = (t.clone().to(R.DEV) for t in (p0, gr, m0, v0))
            cnt = torch.tensor([3], dtype=torch.int32, device=R.DEV)
            _lib.call("cmpc_adam_step", P.data_ptr(), G.data_ptr(), Mm.data_ptr(), V.data_ptr(), segs_dev.data_ptr(), len(segs),
                      lr, b1, b2, eps, gs, cnt.data_ptr() if with_count else None, W._st())
            torch.cuda.synchronize()
            return {"p": P, "m": Mm, "v": V, "cnt": cnt}
        o = R.run_twice(run)
        assert int(o["cnt"][0]) == (3 + n_bad if with_count else 3)
        upd = live & fin
        for k, t0 in (("p", p0), ("m", m0), ("v", v0)):
            got = o[k].cpu()
            assert torch.equal(R._bits(got[~upd]), R._bits(t0[~upd])), f"adam: {k} changed where it must stay untouched"
        f = lambda x: torch.tensor(x, dtype=torch.float32).double()    # the float32 constants the kernel sees
        pp, mm, vv, gg = p0.double(), m0.double(), v0.double(), torch.where(fin, gr.double(), torch.zeros(n, dtype=torch.float64))
        geff = gg * f(gs) * gm_e + wd_e * pp
        mn = f(b1) * mm + (1 - f(b1)) * geff
        vn = f(b2) * vv + (1 - f(b2)) * geff * geff
        den = vn.sqrt() + f(eps)
        step = f(lr) * mn / den
        pn = pp - step
        u = R.U24
        gmag = (gg * f(gs) * gm_e).abs() + (wd_e * pp).abs()
        tol_m = 4 * u * (f(b1) * mm.abs() + gmag)
        tol_v = 4 * u * (f(b2) * vv + 3 * gmag * gmag)
        tol_p = u * (pp.abs() + step.abs()) + f(lr) * (tol_m + 8 * u * mn.abs()) / den + step.abs() * (tol_v / (2 * vn.sqrt().clamp_min(1e-30) * den) + 4 * u)
        for k, ref, tol in (("m", mn, tol_m), ("v", vn, tol_v), ("p", pn, tol_p)):
            R.assert_close(o[k].cpu()[upd], ref[upd], F32, what=f"adam {k}", rtol=0.0, atol=tol[upd])
