"""CPU tests of the pack plans of every model: a planning-only handle (device = -1) of each of the six graphs, in every storage type, at
the tiny config, at the model's full config and with v_emb_dim = 30 (segment ends that are not multiples of 4), passes check_plan
(tests/packref.py), and its descriptors cover the bytes of exactly the operands plan_operands creates."""
import ctypes

import pytest

from tests import packref as PR

TINY = dict(batch_size=2, num_steps=6, vf_h=8, vf_w=8, H=64, W=64, vf_dim=256, c4_dim=128, c3_dim=64, vocab_size=50, v_emb_dim=40,
            mlp_dim=24, rnn_size=40, glove_dim=12, parse_dim=20)


def plan_cfg(pkg, model, size, dt):
    lib = pkg._lib.load()
    c = pkg._lib.EngineCfg()
    assert lib.cmpc_default_cfg(ctypes.byref(c)) == 0
    if size != "full":
        for k, v in TINY.items():
            setattr(c, k, v)
    if size == "c30":
        c.v_emb_dim = c.rnn_size = 30
    code, hsv = PR.MODELS[model]
    assert lib.cmpc_default_cfg_model(ctypes.byref(c), code, hsv) == 0
    if code == 2:
        c.batch_size = 1                        # the video graph is batch 1
    c.dtype, c.device = dt, -1
    return lib, c


@pytest.mark.parametrize("size", ["tiny", "full", "c30"])
@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("model", list(PR.MODELS))
def test_model_plan_passes_check_plan(pkg, model, dt, size):
    lib, c = plan_cfg(pkg, model, size, dt)
    h = ctypes.c_void_p()
    assert lib.cmpc_create(ctypes.byref(c), ctypes.byref(h)) == 0, lib.cmpc_last_error()
    try:
        descs, arena_bytes, params, s0 = PR.handle_plan(lib, pkg._lib.PackDesc, h)
        assert 0 < s0 < len(descs)
        PR.check_plan(descs, arena_bytes, params)
        ops = PR.handle_operands(lib, h, PR.operand_keys(PR.MODELS[model][0], bool(c.conv5)))
        PR.check_operands(descs, ops)
        # the visual operands are stored in cfg.dtype, the language side and the text encoder in float32
        assert {d.dst_dt for d in descs} == ({0} if dt == 0 else {0, dt})
    finally:
        assert lib.cmpc_destroy(h) == 0


def test_check_plan_catches_bad_tables(pkg):
    """check_plan and check_operands are not vacuous: each broken table below is refused"""
    lib, c = plan_cfg(pkg, "CMPC_model", "tiny", 1)
    h = ctypes.c_void_p()
    assert lib.cmpc_create(ctypes.byref(c), ctypes.byref(h)) == 0, lib.cmpc_last_error()
    try:
        descs, arena_bytes, params, _ = PR.handle_plan(lib, pkg._lib.PackDesc, h)
        keys = PR.operand_keys(0)
        ops = PR.handle_operands(lib, h, keys)
    finally:
        lib.cmpc_destroy(h)

    def copy():
        return [pkg._lib.PackDesc.from_buffer_copy(bytes(d)) for d in descs]
    PR.check_plan(copy(), arena_bytes, params)
    breakers = [
        lambda ds: setattr(ds[3], "dst_off", ds[2].dst_off),                      # two descriptors on the same bytes
        lambda ds: setattr(ds[-1], "rows", ds[-1].rows + 64),                     # past the end of the arena
        lambda ds: ds[0].ns_len.__setitem__(0, ds[0].ns_len[0] + 64),             # an N segment into the next gate block
        lambda ds: ds[5].ks_len.__setitem__(0, ds[5].ks_len[0] + 1),              # a source row of the next parameter
        lambda ds: setattr(ds[1], "cols", ds[1].cols - 2),                        # cols not a multiple of 4
        lambda ds: setattr(ds[0], "dst_off", ds[0].dst_off + 8),                  # not 16-B aligned
    ]
    for i, brk in enumerate(breakers):
        ds = copy()
        brk(ds)
        with pytest.raises(AssertionError):
            PR.check_plan(ds, arena_bytes, params)
            pytest.fail(f"breaker {i} passed")
    with pytest.raises(AssertionError):
        PR.check_operands(descs, {k: v for k, v in ops.items() if k != "fus_c4.n"})     # an operand the key list misses
    ds = copy()
    ds[7].rows -= 8
    with pytest.raises(AssertionError):
        PR.check_operands(ds, ops)                                                # an operand row left unwritten
