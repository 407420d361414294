"""CPU tests of CMPC_MODEL_V5 (CMPCv5_model / CMPCv5_HSV_model) at the C ABI: planning-only handles (device = -1) carry the oracle's
manifest (tests/v5uni_oracle.py) in name, order and shape, the model's defaults, and reject bad configurations with CMPC_EINVAL."""
import ctypes

import pytest

from tests import v5uni_oracle as U5

MODEL_V5 = 3


def _cfg(pkg, cfg, hsv):
    lib = pkg._lib.load()
    c = pkg._lib.EngineCfg()
    assert lib.cmpc_default_cfg(ctypes.byref(c)) == 0
    for k in ("batch_size", "num_steps", "vf_h", "vf_w", "H", "W", "vf_dim", "c4_dim", "c3_dim", "vocab_size", "v_emb_dim", "mlp_dim",
              "rnn_size", "glove_dim", "parse_dim"):
        setattr(c, k, getattr(cfg, k))
    assert lib.cmpc_default_cfg_model(ctypes.byref(c), MODEL_V5, hsv) == 0
    c.c2_dim, c.c2_h, c.c2_w, c.aspp_depth, c.low_dim = cfg.c2_dim, cfg.H // 4, cfg.W // 4, cfg.aspp_depth, cfg.low_dim
    for i, r in enumerate(cfg.aspp_rates):
        c.aspp_rates[i] = r
    c.device = -1
    return lib, c


def _manifest(lib, h):
    name, off, rank, shape = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int(), (ctypes.c_int64 * 4)()
    out = []
    for i in range(lib.cmpc_param_count(h)):
        assert lib.cmpc_param_info(h, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(rank), ctypes.byref(shape)) == 0
        out.append((name.value.decode(), tuple(int(shape[k]) for k in range(rank.value))))
    return out


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("hsv", [0, 1])
def test_planning_handle_manifest_equals_oracle(pkg, hsv, full):
    cfg = U5.Cfg(batch_size=8, num_steps=25, vf_h=64, vf_w=64, H=512, W=512, hsv=bool(hsv)) if full else U5.tiny_cfg(hsv=bool(hsv))
    lib, c = _cfg(pkg, cfg, hsv)
    assert c.model == MODEL_V5 and c.hsv == hsv and c.bn_train == 1
    assert [round(x, 6) for x in c.loss_w] == [0.8, 0.1, 0.1, 0.0]                  # CMPCv5_model.py:531-532
    h = ctypes.c_void_p()
    assert lib.cmpc_create(ctypes.byref(c), ctypes.byref(h)) == 0, lib.cmpc_last_error()
    try:
        assert _manifest(lib, h) == [(n, tuple(s)) for n, s, _, _ in U5.head_param_specs(cfg)]
        name, cnt = ctypes.c_char_p(), ctypes.c_int64()
        st = []
        for i in range(lib.cmpc_state_count(h)):
            assert lib.cmpc_state_info(h, i, ctypes.byref(name), ctypes.byref(cnt)) == 0
            st.append((name.value.decode(), (cnt.value,)))
        assert st == [(n, tuple(s)) for n, s, _ in U5.bn_state_specs(cfg)]
        # the spatial grid: 8 channels, or 11 with the HSV map in channels 8..10 -- the Mutan and fusion operands pack that many grid rows
        descs, nd = ctypes.POINTER(pkg._lib.PackDesc)(), ctypes.c_int()
        ab, wb, s0 = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        assert lib.cmpc_plan_info(h, ctypes.byref(descs), ctypes.byref(nd), ctypes.byref(ab), ctypes.byref(wb), ctypes.byref(s0)) == 0
        offs = {}
        off = ctypes.c_int64()
        for i in range(lib.cmpc_param_count(h)):
            assert lib.cmpc_param_info(h, i, ctypes.byref(name), ctypes.byref(off), None, None) == 0
            offs[off.value] = name.value.decode()
        grid = {}
        for i in range(nd.value):
            d = descs[i]
            n = offs.get(d.src_off, "")
            if d.transpose and ("/vis_trans_" in n or "/fusion_" in n) and n.endswith("/DW") and d.nks >= 2:
                grid.setdefault(n, set()).add(d.ks_len[d.nks - 1])
        assert len(grid) == 12 and all(v == {11 if hsv else 8} for v in grid.values()), grid
    finally:
        lib.cmpc_destroy(h)


def test_bad_configurations_are_rejected(pkg):
    cfg = U5.tiny_cfg(hsv=True)
    lib, c = _cfg(pkg, cfg, 1)
    h = ctypes.c_void_p()
    for field, bad in (("hsv", 2), ("model", 4), ("c2_dim", 100), ("aspp_depth", 6), ("low_dim", 65), ("mlp_dim", 26), ("vf_dim", 2000)):
        old = getattr(c, field)
        setattr(c, field, bad)
        assert lib.cmpc_create(ctypes.byref(c), ctypes.byref(h)) == -1, field
        assert lib.cmpc_last_error()
        setattr(c, field, old)
    assert lib.cmpc_create(ctypes.byref(c), ctypes.byref(h)) == 0
    lib.cmpc_destroy(h)
    assert lib.cmpc_default_cfg_model(ctypes.byref(c), 4, 0) == -1
    # the grid kernel validates before it launches
    assert lib.cmpc_hsv_grid(2, None, None, None, 1, 8, 8, 1, 1, None) == -1
