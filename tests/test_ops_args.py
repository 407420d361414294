"""CPU test: every documented limit of the op-level stage entry points (include/cmpc.h) returns CMPC_EINVAL (-1) with a message
before anything is launched -- the library loads and these calls run without a GPU.  Only the checks an entry point makes before its
first HIP call are listed here (read off each entry point: map_ok / ok / the explicit range checks sit at the top); the pointers are
dummies that are never dereferenced."""
import importlib

import pytest

L = importlib.import_module("cmpc-refseg_amd._lib")
P = 1          # a non-NULL dummy device pointer: never read, the call returns first
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _rejects(lib, name, *args, msg=None):
    rc = getattr(lib, name)(*args)
    assert rc == EINVAL, f"{name}{args} returned {rc}"
    err = lib.cmpc_last_error()
    assert err, f"{name}: no message"
    if msg is not None:
        assert msg.encode() in err, (name, err)
    return err


# (C, ld, dt) rejected by map_ok (ops_norm.hip: ld <= 2048) / the 1024-column kernels (ops_fusion.hip, ops_convlstm.hip)
def _bad_maps(max_ld):
    return [(65, 64, 0), (24, 60, 1), (8, max_ld + 8, 2), (0, 64, 0), (24, 64, 3), (24, 64, -1)]


def test_map_limits_ops_norm(lib):
    for C, ld, dt in _bad_maps(2048):
        _rejects(lib, "cmpc_act_bwd", dt, P, P, P, 0, 16, ld, ld, C, P, None, 0, 0, None)
        _rejects(lib, "cmpc_wcolsum", dt, P, P, P, ld, 2, 8, ld, C, 1.0, None)
        _rejects(lib, "cmpc_rowdot1", dt, P, P, ld, P, 2, 8, ld, C, 1.0, None)
        _rejects(lib, "cmpc_rank1_update", dt, P, P, P, None, None, ld, 1.0, 1.0, 2, 8, ld, C, None)
        _rejects(lib, "cmpc_l2norm_rows_fwd", dt, P, P, P, None, 16, ld, C, None)
        _rejects(lib, "cmpc_l2norm_rows_bwd", dt, P, P, P, P, 16, ld, C, 0, None)
        _rejects(lib, "cmpc_gconv_pre_fwd", dt, P, P, P, P, P, P, 2, 8, ld, C, None)
        _rejects(lib, "cmpc_gconv_pre_bwd", dt, P, P, P, P, P, P, 0, P, P, P, P, 2, 8, ld, C, None)
        _rejects(lib, "cmpc_gconv_post_fwd", dt, P, P, P, P, P, P, 2, 8, ld, C, None)
        _rejects(lib, "cmpc_gconv_post_bwd", dt, P, P, P, P, P, P, P, P, P, P, 2, 8, ld, C, None)
    assert b"C=65 ld=64" in _rejects(lib, "cmpc_l2norm_rows_fwd", 0, P, P, P, None, 16, 64, 65, None)
    assert b"dtype" in _rejects(lib, "cmpc_l2norm_rows_fwd", 3, P, P, P, None, 16, 64, 24, None)
    # ld itself is fine at the 2048 limit; 2056 is one column block too many
    _rejects(lib, "cmpc_l2norm_rows_fwd", 0, P, P, P, None, 16, 2056, 2048, None, msg="2048")


def test_act_bwd_stride_and_rows_per_sample(lib):
    _rejects(lib, "cmpc_act_bwd", 0, P, P, P, 0, 16, 56, 64, 24, P, None, 0, 0, None, msg="stride")     # stride < ld
    _rejects(lib, "cmpc_act_bwd", 1, P, P, P, 0, 16, 68, 64, 24, P, None, 0, 0, None, msg="stride")     # stride % 8
    _rejects(lib, "cmpc_act_bwd", 2, P, P, P, 0, 16, 64, 64, 24, None, P, 64, 0, None, msg="rows_per_sample")
    _rejects(lib, "cmpc_act_bwd", 0, P, P, P, 0, 16, 64, 64, 24, None, P, 64, 5, None, msg="rows_per_sample")   # 16 % 5
    _rejects(lib, "cmpc_act_bwd", 0, P, P, P, 0, 16, 64, 64, 24, None, P, 64, -4, None, msg="rows_per_sample")


def test_map_limits_ops_fusion_and_convlstm(lib):
    ln = L.ConvLstmLn()
    dln = L.ConvLstmDln()
    for C, ld, dt in _bad_maps(1024):
        _rejects(lib, "cmpc_mutan_fwd", dt, P, P, P, P, 2, 8, ld, C, 0, None)
        _rejects(lib, "cmpc_mutan_bwd", dt, P, P, P, P, P, P, 2, 8, ld, C, None)
        _rejects(lib, "cmpc_exchange_combine_fwd", dt, P, P, P, P, P, ld, P, P, 2, 8, ld, C, None)
        _rejects(lib, "cmpc_exchange_combine_bwd", dt, P, P, P, P, P, P, P, ld, P, 0, P, P, P, P, None, None, 2, 8, ld, C, None)
        _rejects(lib, "cmpc_convlstm_a", dt, P, None, P, P, P, 2, 8, ld, C, None)
        _rejects(lib, "cmpc_convlstm_b", dt, P, None, P, ln, P, P, 2, 8, ld, C, None)
        _rejects(lib, "cmpc_convlstm_c", dt, P, P, ln, P, P, P, 2, 8, ld, C, None)
        _rejects(lib, "cmpc_convlstm_bwd", dt, P, P, P, None, P, P, P, P, ln, P, P, None, P, P, P, dln, P, P, 2, 8, ld, C, None)
    _rejects(lib, "cmpc_mutan_fwd", 0, P, P, P, P, 2, 8, 1032, 1025, 0, None, msg="1024")
    _rejects(lib, "cmpc_convlstm_a", 0, P, None, P, P, P, 2, 8, 1032, 1025, None, msg="1024")


def test_graph_softmax_limits(lib):
    for T, Tp in ((65, 65), (0, 8), (8, 4), (33, 72)):
        _rejects(lib, "cmpc_graph_softmax_fwd", 0, 0, P, P, P, P, P, P, P, P, 2, 64, T, Tp, None, msg="Tp <= 64")
        _rejects(lib, "cmpc_graph_softmax_bwd", 1, P, P, P, P, P, P, P, P, P, P, P, 2, 64, T, Tp, None, msg="Tp <= 64")
    _rejects(lib, "cmpc_graph_softmax_fwd", 2, 1, P, P, P, P, P, P, P, None, 2, 64, 20, 24, None, msg="scratch")
    _rejects(lib, "cmpc_graph_softmax_bwd", 2, P, P, P, P, P, P, P, P, P, P, None, 2, 64, 20, 24, None, msg="scratch")


def test_lstm_bwd_step_limits(lib):
    # lstm_bwd_step: B <= 8, 16-B aligned rows
    for B, ld, ldw in ((9, 64, 256), (0, 64, 256), (2, 66, 264), (2, 64, 258)):
        _rejects(lib, "cmpc_lstm_bwd_step", P, P, ldw, P, P, P, P, 0, P, ld, P, P, P, B, ld, ld, None, msg="lstm_bwd_step")


def test_parse_and_pool_limits(lib):
    for ncls, ld in ((1, 8), (9, 16), (5, 4)):
        _rejects(lib, "cmpc_parse_softmax_fwd", P, ld, P, P, 10, ncls, None, msg="ncls")
        _rejects(lib, "cmpc_parse_softmax_bwd", P, P, P, P, ld, 10, ncls, None, msg="ncls")
    for ncls, lo, ps in ((0, 0, 4), (2, -1, 4), (3, 2, 4), (1, 5, 5), (2, 0, 9)):
        _rejects(lib, "cmpc_lang_pool_fwd", P, P, P, P, 2, 20, 64, 64, ncls, lo, ps, None, msg="cls_lo")
        _rejects(lib, "cmpc_lang_pool_bwd", P, P, P, P, P, P, P, 2, 20, 64, 64, ncls, lo, ps, None, msg="cls_lo")
    _rejects(lib, "cmpc_lang_pool_fwd", P, P, P, P, 2, 65, 64, 64, 2, 0, 4, None, msg="T <= 64")
    _rejects(lib, "cmpc_lang_pool_fwd", P, P, P, P, 2, 20, 2056, 2048, 2, 0, 4, None, msg="ld <= 2048")


def test_upsample_target_needs_outputs(lib):
    for loss, inter, uni in ((None, P, P), (P, None, P), (P, P, None)):
        _rejects(lib, "cmpc_upsample_fwd", P, P, None, P, loss, inter, uni, 2, 40, 40, 320, 320, None, msg="required with target")


def test_convlstm_needs_m_multiple_of_4(lib):
    # the peephole rows (W_c* [N, M]) are read as float4: M % 4 == 0 (M = 500, the product's, passes the check)
    ln, dln = L.ConvLstmLn(), L.ConvLstmDln()
    for M in (37, 22, 510):
        _rejects(lib, "cmpc_convlstm_a", 0, P, None, P, P, P, 2, 8, 512, M, None, msg="M % 4")
        _rejects(lib, "cmpc_convlstm_b", 1, P, None, P, ln, P, P, 2, 8, 512, M, None, msg="M % 4")
        _rejects(lib, "cmpc_convlstm_c", 2, P, P, ln, P, P, P, 2, 8, 512, M, None, msg="M % 4")
        _rejects(lib, "cmpc_convlstm_bwd", 0, P, P, P, None, P, P, P, P, ln, P, P, None, P, P, P, dln, P, P, 2, 8, 512, M, None, msg="M % 4")


def test_decoder_limits(lib):
    # batch norm: 1 <= C <= Cpad <= 2048, Cpad % 8 == 0, the x row stride a multiple of 8 and >= roundup(C, 8), R >= 1
    for C, Cpad, ld, R in ((0, 8, 8, 4), (9, 8, 16, 4), (8, 12, 8, 4), (2049, 2056, 2056, 4), (8, 8, 12, 4), (9, 16, 8, 4), (8, 8, 8, 0)):
        _rejects(lib, "cmpc_bn_stats", 0, P, ld, R, C, Cpad, 1e-5, P, P, None)
        _rejects(lib, "cmpc_bn_apply_fwd", 1, P, ld, P, Cpad, P, P, P, 16, 16, R, C, 1, None)
        _rejects(lib, "cmpc_bn_bwd", 2, P, 16, P, 16, P, ld, P, Cpad, P, P, 16, P, P, P, R, C, 1, None, msg="bn_bwd")
    _rejects(lib, "cmpc_bn_stats", 0, P, 64, 10, 24, 2056, 1e-5, P, P, None, msg="2048")
    # bn_apply_fwd: Cy % 8 == 0, Cy >= C, Cy <= 2048, ldy % 8 == 0
    for Cy, ldy in ((20, 24), (16, 24), (24, 28), (2056, 2056)):
        _rejects(lib, "cmpc_bn_apply_fwd", 0, P, 24, P, 24, P, P, P, ldy, Cy, 10, 20 if Cy != 16 else 24, 0, None)
    # bn_bwd: relu needs y; 16-B aligned row strides
    _rejects(lib, "cmpc_bn_bwd", 0, P, 24, None, 24, P, 24, P, 24, P, P, 24, P, P, P, 10, 20, 1, None, msg="bn_bwd")
    _rejects(lib, "cmpc_bn_bwd", 0, P, 20, None, 24, P, 24, P, 24, P, P, 24, P, P, P, 10, 20, 0, None, msg="bn_bwd")
    _rejects(lib, "cmpc_bn_bwd", 0, P, 24, None, 24, P, 24, P, 24, P, P, 28, P, P, P, 10, 20, 0, None, msg="bn_bwd")
    _rejects(lib, "cmpc_bn_from_moving", P, P, 10, 8, 1e-5, P, None, msg="bn_from_moving")
    _rejects(lib, "cmpc_bn_update_moving", P, 0, 0.9, P, P, 8, 8, None, msg="bn_update_moving")
    _rejects(lib, "cmpc_bn_update_moving", P, 4, 0.9, P, P, 10, 8, None, msg="bn_update_moving")
    # resize: C % 8 == 0 and >= 8, 16-B rows, sizes >= 1
    for C, ldx, ldy, h in ((12, 16, 16, 4), (0, 16, 16, 4), (16, 20, 16, 4), (16, 16, 20, 4), (16, 16, 16, 0)):
        _rejects(lib, "cmpc_resize_bilinear_fwd", 0, P, ldx, P, ldy, 2, h, 4, 8, 8, C, None, msg="resize_bilinear_fwd")
        _rejects(lib, "cmpc_resize_bilinear_bwd", 1, P, ldy, P, ldx, 2, h, 4, 8, 8, C, None, msg="resize_bilinear_bwd")
    # hsv: ld % 8 == 0 and >= 8; grid1 != grid
    for ld in (4, 12):
        _rejects(lib, "cmpc_hsv_map", 0, P, P, ld, 1, 8, 8, 4, 4, None, msg="hsv_map")
    _rejects(lib, "cmpc_hsv_grid", 0, P, P, P, 1, 8, 8, 4, 4, None, msg="hsv_grid")
    # reverse_sequence: not in place, T >= 1
    _rejects(lib, "cmpc_reverse_sequence", P, P, P, 2, 5, 16, None, msg="not in place")
    _rejects(lib, "cmpc_reverse_sequence", P, 2, P, 2, 0, 16, None, msg="reverse_sequence")
    # conv_to1: ld % 8 == 0, C <= ld, R >= 1; the backward's column registers end at 2048
    for R, C, ld in ((10, 8, 12), (10, 24, 16), (0, 8, 8)):
        _rejects(lib, "cmpc_conv_to1_fwd", 0, P, ld, P, P, P, R, C, None, msg="conv_to1_fwd")
        _rejects(lib, "cmpc_conv_to1_bwd", 0, P, P, ld, P, P, P, P, R, C, None, msg="conv_to1_bwd")
    _rejects(lib, "cmpc_conv_to1_bwd", 1, P, P, 2056, P, P, P, P, 10, 2050, None, msg="conv_to1_bwd")


# ---- the contraction entry points (csrc/gemm.hip, csrc/ops_fusion.hip lowrank_nn, csrc/ops_lang.hip adam_step) ----------------------
def _nt(dt=1, M=64, N=64, Ks=(64,), lda=None, ldb=None, ldc=64, batch=1, C=P):
    a = L.GemmNtArgs()
    a.dtype, a.nseg = dt, len(Ks)
    for i, K in enumerate(Ks[:3]):
        a.A[i], a.Bt[i], a.K[i] = P, P, K
        a.lda[i], a.ldb[i] = lda if lda is not None else K, ldb if ldb is not None else K
    a.C, a.ldc, a.M, a.N, a.n_valid, a.batch, a.alpha = C, ldc, M, N, N, batch, 1.0
    return a


def test_gemm_nt_limits(lib):
    import ctypes
    good = _nt()
    bad = [_nt(Ks=()), _nt(M=0), _nt(N=0), _nt(batch=0), _nt(dt=3), _nt(dt=-1),
           _nt(Ks=(40,)), _nt(dt=0, Ks=(48,)),                      # K a multiple of 64 (16-bit) / 32 (fp32)
           _nt(lda=68), _nt(ldb=66), _nt(dt=0, Ks=(32,), lda=34),   # 16-B aligned rows
           _nt(N=66, ldc=72), _nt(ldc=66), _nt(C=None)]
    four = _nt(Ks=(64, 64, 64))
    four.nseg = 4
    bad.append(four)
    nullA = _nt()
    nullA.A[0] = None
    bad.append(nullA)
    for a in bad:
        _rejects(lib, "cmpc_gemm_nt", ctypes.byref(a), None, msg="gemm_nt")
        _rejects(lib, "cmpc_gemm_nt_pair", ctypes.byref(good), ctypes.byref(a), None, msg="gemm_nt")
        _rejects(lib, "cmpc_gemm_nt_pair", ctypes.byref(a), ctypes.byref(good), None, msg="gemm_nt")
    _rejects(lib, "cmpc_gemm_nt", ctypes.byref(_nt(Ks=(40,))), None, msg="multiple of 64")


def _tn(dt=1, R=100, Kv=64, Nv=64, lda=64, ldd=64, Ka=64, Nd=64, nb=1, nb2=1, o_bs=64 * 64, rsplit=1):
    a = L.GemmTnArgs()
    a.dtype, a.A, a.lda, a.Ka, a.D, a.ldd, a.Nd, a.out, a.ldo = dt, P, lda, Ka, P, ldd, Nd, P, 64
    a.R, a.Kv, a.Nv, a.nb, a.nb2, a.a_bs, a.d_bs, a.o_bs, a.rsplit, a.alpha = R, Kv, Nv, nb, nb2, 64 * R, 64 * R, o_bs, rsplit, 1.0
    return a


def test_gemm_tn_limits(lib):
    import ctypes
    bad = [_tn(R=-1), _tn(Kv=0), _tn(Nv=0), _tn(nb=0), _tn(nb=9), _tn(nb2=0), _tn(dt=3),
           _tn(lda=66), _tn(ldd=60 + 2), _tn(Ka=60 + 2), _tn(Nd=66), _tn(dt=0, lda=66)]
    null = _tn()
    null.out = None
    bad.append(null)
    off = _tn(nb=2)
    off.a_off[1] = 4                                             # 8 B: not 16-B aligned in bf16
    bad.append(off)
    bs = _tn(nb2=2)
    bs.a_bs = 68 * 100 + 4
    bad.append(bs)
    for a in bad:
        _rejects(lib, "cmpc_gemm_tn", ctypes.byref(a), None, msg="gemm_tn")
        arr = (L.GemmTnArgs * 2)(_tn(), a)
        _rejects(lib, "cmpc_gemm_tn_grouped", arr, 2, None, msg="gemm_tn")
    _rejects(lib, "cmpc_gemm_tn", ctypes.byref(_tn(rsplit=0)), None, msg="rsplit")
    # an outer batch into one shared output (o_bs == 0) folds every slab into ONE region: cmpc_gemm_tn needs nb == 1 and says so
    # before launching anything; the grouped form expands such a batch into single products and takes it
    _rejects(lib, "cmpc_gemm_tn", ctypes.byref(_tn(nb=2, nb2=3, o_bs=0)), None, msg="o_bs == 0 needs nb == 1")
    _rejects(lib, "cmpc_gemm_tn", ctypes.byref(_tn(nb=2, nb2=3, o_bs=0, R=0)), None, msg="o_bs == 0 needs nb == 1")


def _conv(dt=1, k=3, s=1, dil=1, Cin=64, Cout=64, ldx=64, ldw=576, ldy=64, res=None, B=2, H=8, W=8):
    a = L.ConvArgs()
    a.dtype, a.X, a.ldx, a.Wt, a.ldw, a.bias, a.res, a.Y, a.ldy = dt, P, ldx, P, ldw, P, res, P, ldy
    a.B, a.H, a.W, a.Cin, a.Cout, a.ksize, a.stride, a.dil, a.relu, a.zeros = B, H, W, Cin, Cout, k, s, dil, 1, P
    return a


def test_conv_nhwc_limits(lib):
    import ctypes
    bad = [_conv(k=2), _conv(k=5), _conv(s=3), _conv(s=0), _conv(dil=0), _conv(Cin=32), _conv(dt=0, Cin=48), _conv(Cout=12),
           _conv(ldx=68), _conv(ldw=580), _conv(ldy=68), _conv(res=P, ldy=68), _conv(B=0), _conv(H=0), _conv(W=0)]
    for field in ("X", "Wt", "Y", "bias", "zeros"):
        a = _conv()
        setattr(a, field, None)
        bad.append(a)
    for a in bad:
        _rejects(lib, "cmpc_conv_nhwc", ctypes.byref(a), None, msg="conv_nhwc")
    _rejects(lib, "cmpc_conv_nhwc", ctypes.byref(_conv(dt=3)), None, msg="dtype")


def test_lowrank_nn_limits(lib):
    # (dt, lda, sA, ldb, sB, ldc, sC, M, N, n_valid, Kv, batch)
    ok = (1, 24, 24 * 10, 64, 24 * 64, 64, 640, 10, 64, 64, 20, 2)
    for i, v in ((0, 0), (0, 3), (8, 60), (8, 2048), (8, 0), (7, 0), (10, 25), (10, 0), (11, 0),     # dtype; N = 4 * 2^j <= 1024; Kv; M; batch
                 (1, 16), (1, 28), (3, 60), (3, 66), (5, 66), (2, 244), (4, 66), (6, 642)):         # lda >= 8 ceil(Kv / 8), % 8; ldb >= N; strides
        a = list(ok)
        a[i] = v
        dt, lda, sA, ldb, sB, ldc, sC, M, N, nv, Kv, B = a
        _rejects(lib, "cmpc_lowrank_nn", dt, P, lda, sA, P, ldb, sB, P, ldc, sC, M, N, nv, Kv, B, 1.0, 0, None, msg="lowrank_nn")
    dt, lda, sA, ldb, sB, ldc, sC, M, N, nv, Kv, B = ok
    for A, Bk, C in ((None, 16, 16), (16, None, 16), (16, 16, None), (8, 16, 16), (16, 12, 16), (16, 16, 4)):    # NULL / misaligned
        _rejects(lib, "cmpc_lowrank_nn", dt, A, lda, sA, Bk, ldb, sB, C, ldc, sC, M, N, nv, Kv, B, 1.0, 0, None, msg="lowrank_nn")


def test_adam_limits(lib):
    for i in range(5):
        bufs = [16, 16, 16, 16, 16]
        bufs[i] = None
        p, g, m, v, segs = bufs
        _rejects(lib, "cmpc_adam_step", p, g, m, v, segs, 3, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, None, msg="adam_step")
    assert lib.cmpc_adam_step(None, None, None, None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, None) == 0     # nothing to do


def test_pack_weights_limits(lib):
    # args: master, arena, descs, tile_prefix, tile_desc, ndesc, tile_begin, tile_end, stream
    _rejects(lib, "cmpc_pack_weights_range", P, P, P, P, None, 1, -1, 4, None, msg="tile range")
    _rejects(lib, "cmpc_pack_weights_range", P, P, P, P, P, 3, -5, 1, None, msg="tile range")
    for i in range(4):
        bufs = [P, P, P, P]
        bufs[i] = None
        _rejects(lib, "cmpc_pack_weights_range", *bufs, None, 2, 0, 3, None, msg="pack_weights")
        _rejects(lib, "cmpc_pack_weights", *bufs, 2, 3, None, msg="pack_weights")
    # nothing to do: no descriptors, or an empty range (returns before any launch, whatever the pointers)
    for nd in (0, -3):
        assert lib.cmpc_pack_weights_range(None, None, None, None, None, nd, 0, 8, None) == 0
        assert lib.cmpc_pack_weights(None, None, None, None, nd, 8, None) == 0
    assert lib.cmpc_pack_weights_range(P, P, P, P, None, 2, 5, 5, None) == 0
    assert lib.cmpc_pack_weights_range(P, P, P, P, None, 2, 6, 5, None) == 0
    assert lib.cmpc_pack_weights(P, P, P, P, 2, 0, None) == 0
