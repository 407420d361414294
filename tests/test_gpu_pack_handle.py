"""GPU tests of the packed operands of a cmpc_create handle, bit for bit against tests/packref.py: the whole arena (tap
"packed_operands") after cmpc_pack from stress-valued masters, for each of the six graphs; and the optimizer's per-bucket split
(cmpc_optimizer_bucket): each bucket updates exactly its own parameters (float64 TF-Adam) and repacks exactly the operands read from them."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests import packref as PR
from tests import util as U
from tests.test_pack_plan import plan_cfg
from tests.util import O

pytestmark = pytest.mark.gpu
E = importlib.import_module("cmpc-refseg_amd.engine")
SENTINEL = np.array([0xA5, 0xA5, 0xA5, 0x7F], dtype=np.uint8)


def _arena(lib, h, dev):
    ptr, dt, rank, shape = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int(), (ctypes.c_int64 * 4)()
    assert lib.cmpc_tap(h, b"packed_operands", ctypes.byref(ptr), ctypes.byref(dt), ctypes.byref(rank), ctypes.byref(shape)) == 0
    assert dt.value == 3 and rank.value == 1
    return E.dev_tensor(ptr.value, (int(shape[0]),), 3, dev)


@pytest.mark.parametrize("dt", [0, 1, 2], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("model", list(PR.MODELS))
def test_handle_pack_matches_restatement(pkg, model, dt, size="tiny"):
    lib, c = plan_cfg(pkg, model, size, dt)
    c.device = 0
    h = ctypes.c_void_p()
    assert lib.cmpc_create(ctypes.byref(c), ctypes.byref(h)) == 0, lib.cmpc_last_error()
    dev = torch.device("cuda:0")
    try:
        descs, nbytes, params, _ = PR.handle_plan(lib, pkg._lib.PackDesc, h)
        arena = _arena(lib, h, dev)
        assert arena.numel() * 4 == nbytes
        fill = np.resize(SENTINEL, nbytes)
        arena.view(torch.uint8).copy_(torch.from_numpy(fill))
        total = max(o + n for _, o, n in params)
        master = np.zeros(total, dtype=np.float32)
        for i, (name, off, n) in enumerate(params):
            x = PR.stress_master(n, i)
            master[off:off + n] = x
            assert lib.cmpc_set_weights(h, name.encode(), x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n) == 0, lib.cmpc_last_error()
        assert lib.cmpc_pack(h, None) == 0, lib.cmpc_last_error()
        torch.cuda.synchronize()
        got = arena.view(torch.uint8).cpu().numpy()
        exp, written = PR.expected_arena(descs, master, nbytes, fill=fill)
        ops = PR.handle_operands(lib, h, PR.operand_keys(PR.MODELS[model][0], bool(c.conv5)))
        assert int(written.sum()) == sum(r * ld * PR.esz(t) for _, t, r, ld in ops.values())
        PR.assert_arena_equal(got, exp, descs, f"{model} dt {dt}")
    finally:
        assert lib.cmpc_destroy(h) == 0


def test_handle_pack_full_size_f16(pkg):
    """CMPC_model at its full default size (v_emb_dim 1000, mlp_dim 500, vf_dim 2048 ...) in f16"""
    test_handle_pack_matches_restatement(pkg, "CMPC_model", 2, size="full")


def _adam_ref(p, g, wd, gm, lr, gscale):
    """first TF-Adam step (m = v = 0) in float64 from the float32 state, and the bound of the Adam op test (test_gpu_ops_gemm.py)"""
    f = lambda x: float(np.float32(x))
    b1, b2, eps, u = f(0.9), f(0.999), f(1e-8), 2.0 ** -24
    lr = f(lr)
    geff = g * f(gscale) * gm + wd * p
    mn, vn = (1 - b1) * geff, (1 - b2) * geff * geff
    den = np.sqrt(vn) + eps
    step = lr * mn / den
    gmag = np.abs(g * f(gscale) * gm) + np.abs(wd * p)
    tol_m, tol_v = 4 * u * gmag, 4 * u * 3 * gmag * gmag
    tol = u * (np.abs(p) + np.abs(step)) + lr * (tol_m + 8 * u * np.abs(mn)) / den + np.abs(step) * (tol_v / (2 * np.maximum(np.sqrt(vn), 1e-30) * den) + 4 * u)
    return p - step, tol


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_optimizer_buckets_update_and_repack_their_own_parameters(pkg, dtype):
    cfg = U.tiny_cfg()
    hp, bp = O.init_head_params(cfg), O.init_backbone_params(cfg)
    words, im, sl, tgt = O.synth_batch(cfg)
    feats = O.backbone_forward(bp, im, cfg)
    m = pkg.LSTM_model(head_params=hp, backbone_params=bp, **U.model_kwargs(cfg, dtype))
    eng = m.eng
    lib, h = eng.lib, eng.h
    descs, nbytes, params, _ = PR.handle_plan(lib, pkg._lib.PackDesc, h)
    arena = _arena(lib, h, eng.device)
    m.loss_and_grads([f.to(m.device) for f in feats], words, tgt, sl)
    torch.cuda.synchronize()
    p0 = eng.params.cpu().numpy().copy()
    g = eng.grads.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all() and np.count_nonzero(g) > g.size // 4
    PR.assert_arena_equal(arena.view(torch.uint8).cpu().numpy(), PR.expected_arena(descs, p0, nbytes)[0], descs, "before")
    wd = np.zeros(p0.size)
    gm = np.ones(p0.size)
    for name, off, n in params:
        wd[off:off + n] = np.float32(cfg.weight_decay) if "DW" in name else 0.0
        gm[off:off + n] = 2.0 if "biases" in name else 1.0
    lr = cfg.start_lr
    pn, tol = _adam_ref(p0.astype(np.float64), g, wd, gm, lr * np.sqrt(1 - 0.999) / (1 - 0.9), 1.0 / eng.loss_scale)
    owner = np.full(p0.size, -1)
    for b, ranges in enumerate(eng.grad_buckets()):
        for off, cnt in ranges:
            assert (owner[off:off + cnt] == -1).all(), ("buckets overlap", b)
            owner[off:off + cnt] = b
    live = np.zeros(p0.size, dtype=bool)
    for _, off, n in params:
        live[off:off + n] = True
    assert (owner[live] >= 0).all(), "a parameter in no bucket"
    prev = p0
    for b in range(eng.n_buckets):
        eng.optimizer_bucket(b)
        torch.cuda.synchronize()
        cur = eng.params.cpu().numpy().copy()
        mine = (owner == b) & live
        assert np.array_equal(cur[~mine].view(np.uint32), prev[~mine].view(np.uint32)), f"bucket {b} changed another bucket's parameters"
        if mine.any():
            err = np.abs(cur[mine] - pn[mine])
            assert (err <= tol[mine]).all(), (b, float((err - tol[mine]).max()))
            assert (cur[mine] != prev[mine]).any(), b
        # the packed operands: those read from bucket b hold its new masters, the rest still the old ones
        PR.assert_arena_equal(arena.view(torch.uint8).cpu().numpy(), PR.expected_arena(descs, cur, nbytes)[0], descs, f"after bucket {b}")
        prev = cur
    assert eng.step == 1
