"""The train step's serial chains keep only what the next stage on the chain reads (engine.hip: the exchange rounds' products and text side
on the caller's stream, the ConvLSTM's peephole gradients behind the recurrence, the text bucket's weight-gradient launch beside the
embedding gradient).  None of this changes a kernel, a grid or the order of a sum, so every comparison here is `torch.equal`: the handle
with one lane (every launch on the caller's stream, in host issue order -- the race-free reference) against three lanes, and three lanes
against themselves.  A difference is a missing dependency between streams, never rounding."""
import numpy as np
import pytest
import torch

from tests import util as U
from tests.util import O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
    torch.set_num_threads(8)
    cfg = U.tiny_cfg()
    hp, bp = O.init_head_params(cfg), O.init_backbone_params(cfg)
    words, im, sl, tgt = O.synth_batch(cfg)
    return dict(cfg=cfg, hp=hp, bp=bp, words=words, im=im, sl=sl, tgt=tgt)


def _tiny(case, dtype, lanes):
    return U.pkg().LSTM_model(head_params=case["hp"], backbone_params=case["bp"], n_lanes=lanes, **U.model_kwargs(case["cfg"], dtype))


def _tiny_steps(case, m, steps):
    """train steps with changing feeds (words rolled over the batch, images flipped / scaled); returns what the last step left behind"""
    w0, im0 = torch.as_tensor(case["words"]), torch.as_tensor(case["im"])
    scal = None
    for step in range(steps):
        w = torch.roll(w0, step % 2, 0)
        im = (im0, torch.flip(im0, dims=[0]).contiguous(), im0 * 0.5)[step % 3]
        _, scal = m.train_step(w, im, case["tgt"], case["sl"])
    torch.cuda.synchronize()
    return ({k: float(v) for k, v in scal.items()}, m.state_dict(), m.eng.params.clone(), m.eng.grads.clone())


def _assert_same(a, b):
    assert a[0] == b[0]
    assert set(a[1]) == set(b[1])
    for n in a[1]:
        assert torch.equal(torch.as_tensor(a[1][n]), torch.as_tensor(b[1][n])), n
    assert torch.equal(a[2], b[2]), "flat parameter buffer"
    assert torch.equal(a[3], b[3]), "final gradient buffer"


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_one_and_three_lanes_tiny(case, dtype):
    """4 steps with changing feeds: scalars, every parameter and the final gradient buffer, bit for bit"""
    outs = [_tiny_steps(case, _tiny(case, dtype, lanes), 4) for lanes in (3, 1)]
    _assert_same(outs[0], outs[1])


def test_one_and_three_lanes_full_size():
    """B=8, 320x320, f16, 2 steps: pred, up, sigm and the parameter / gradient sample of bench.py --dump-outputs"""
    from bench import DUMP_SAMPLE, synth_batch
    dev = torch.device("cuda:0")
    outs = []
    for lanes in (3, 1):
        m = U.pkg().LSTM_model(batch_size=8, mode="train", dtype="f16", n_lanes=lanes)
        scal = None
        for step in range(2):
            w, im, sl, tg = [torch.from_numpy(x).to(dev) for x in synth_batch(8, 20, 320, 320, m.cfg.vocab_size, step)]
            _, scal = m.train_step(w, im, tg, sl)
        torch.cuda.synchronize()
        eng = m.eng
        idx = np.sort(np.random.default_rng(0).choice(eng.total, size=min(DUMP_SAMPLE, eng.total), replace=False))
        ix = torch.from_numpy(idx).to(eng.params.device)
        outs.append(({k: float(v) for k, v in scal.items()}, {k: eng.tap(k).clone() for k in ("pred", "up", "sigm")},
                     eng.params[ix].clone(), eng.grads[ix].clone()))
        del m, eng
        torch.cuda.empty_cache()
    a, b = outs
    assert a[0] == b[0]
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert torch.equal(a[2], b[2]), "params_sample"
    assert torch.equal(a[3], b[3]), "grads_sample"


def test_two_three_lane_runs_of_ten_steps(case):
    """the race detector: two independent 3-lane models, 10 steps each (two steps in flight throughout)"""
    outs = [_tiny_steps(case, _tiny(case, "f16", 3), 10) for _ in range(2)]
    _assert_same(outs[0], outs[1])


def test_v5_bilstm_one_and_three_lanes():
    """CMPCv5_BiLSTM: one gated branch per module, two levels, both LSTM directions behind the text bucket's early launch"""
    import tests.test_gpu_v5 as T5
    c = T5.make_case(hsv=False)
    outs = []
    for lanes in (3, 1):
        m = T5.build(c, "f32")
        m.set_lanes(lanes)
        scal = None
        for step in range(2):
            w = torch.roll(torch.as_tensor(c["words"]), step, 0)
            _, scal = m.train_step(w, c["im"], c["tgt"], c["sl"])
        torch.cuda.synchronize()
        outs.append(({k: float(v) for k, v in scal.items()}, m.state_dict(), m.eng.params.clone(), m.eng.grads.clone()))
    _assert_same(outs[0], outs[1])


def test_video_one_and_three_lanes():
    import tests.test_gpu_video as TV
    c = TV.make_case(seed=2)
    outs = []
    for lanes in (3, 1):
        m = TV.build(c, "f32")
        m.set_lanes(lanes)
        scal = None
        for step in range(2):
            _, scal = m.train_step_video(c["words"], None, c["tgt"], c["vi"], c["clip"])
        torch.cuda.synchronize()
        outs.append(({k: float(v) for k, v in scal.items()}, m.state_dict(), m.eng.params.clone(), m.eng.grads.clone()))
    _assert_same(outs[0], outs[1])


@pytest.mark.parametrize("with_c", [True, False], ids=["c_prev", "first_step"])
@pytest.mark.parametrize("dt", [0, 2], ids=["f32", "f16"])
def test_convlstm_bwd_split_is_the_whole(dt, with_c):
    """cmpc_convlstm_bwd against cmpc_convlstm_bwd_gates + cmpc_convlstm_peephole_grad on the same inputs and the same pre-filled
    accumulators: dYg, dc_prev, the three peephole gradients and the ten LayerNorm gradients, bit for bit"""
    import tests.test_gpu_ops_convlstm as TC
    R = TC.R
    shape = (2, 1600, 500, 512)
    B, N, M, ld = shape
    case = TC.make_case(shape, dt, 11, with_c=with_c)
    dev = TC._dev(case)
    fw = TC.run_fwd(case, dev)
    pre = TC._prefill(N, M, case["g"])
    whole = TC.run_bwd(case, dev, fw, pre=pre)
    Rr = B * N
    c = case["c"].to(R.DEV) if with_c else None
    dY, dcp = R.guarded(Rr, 4 * ld, dt), R.guarded(Rr, ld, dt)
    dW = [R.guarded(N, M, torch.float32, p) for p in pre["dW"]]
    dW0 = [d.clone() for d in dW]
    dg = [R.guarded(1, M, torch.float32, p) for p in pre["dg"]]
    db = [R.guarded(1, M, torch.float32, p) for p in pre["db"]]
    scr = torch.zeros(Rr, ld, dtype=R.TDT[dt], device=R.DEV)
    bs = R.stat_block(5 * B)
    R.call("cmpc_convlstm_bwd_gates", dt, case["dh"].to(R.DEV), case["dcn"].to(R.DEV), fw["Y"], c, fw["cp"], dev["W"][0], dev["W"][1],
           dev["W"][2], dev["ln"], fw["sums"], dY, dcp if with_c else None, TC._dln_struct(dg, db), scr, bs, B, N, ld, M)
    torch.cuda.synchronize()
    for k in range(3):          # the peephole rows are untouched until the second call
        assert torch.equal(R._bits(dW[k]), R._bits(dW0[k])), k
    R.call("cmpc_convlstm_peephole_grad", dt, dY, c, fw["cp"], dW[0], dW[1], dW[2], B, N, ld, M)
    torch.cuda.synchronize()
    split = {"dY": dY, "dcp": dcp, "dW0": dW[0], "dW1": dW[1], "dW2": dW[2], **{f"dg{k}": dg[k] for k in range(5)},
             **{f"db{k}": db[k] for k in range(5)}}
    for k in whole:             # as bit patterns, guard rows and never-written sentinels included (dc_prev without a previous state)
        assert torch.equal(R._bits(whole[k]), R._bits(split[k])), k
