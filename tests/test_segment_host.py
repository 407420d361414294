"""CPU tests of the per-sample gv_lang norm switch, cmpc_eval_mask_out's argument validation (before anything is launched: the library
loads without a GPU) and the host half of segment.FrameSegmenter driven through a fake device stage."""
import ctypes
import importlib

import numpy as np
import pytest

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
SG = importlib.import_module("cmpc-refseg_amd.segment")
L = importlib.import_module("cmpc-refseg_amd._lib")


def test_library_exports_the_new_symbols():
    lib = L.load()
    assert hasattr(lib, "cmpc_set_gv_norm") and hasattr(lib, "cmpc_eval_mask_out")
    assert "cmpc_set_gv_norm" in L.SIGNATURES and "cmpc_eval_mask_out" in L.SIGNATURES
    assert lib.cmpc_abi_version() == L.ABI_VERSION == 4            # additive: two new symbols, no layout change
    assert (L.GV_NORM_BATCH, L.GV_NORM_SAMPLE) == (0, 1) and L.GV_NORMS == {"batch": 0, "sample": 1}


@pytest.mark.parametrize("model", [L.MODEL_CMPC, L.MODEL_V5_BILSTM, L.MODEL_V5, L.MODEL_VIDEO])
def test_set_gv_norm_on_a_planning_only_handle(model):
    lib = L.load()
    c, h = L.EngineCfg(), ctypes.c_void_p()
    assert lib.cmpc_default_cfg(ctypes.byref(c)) == 0
    c.device, c.model = -1, model
    if model == L.MODEL_VIDEO:
        c.batch_size = 1
    assert lib.cmpc_create(ctypes.byref(c), ctypes.byref(h)) == 0, lib.cmpc_last_error()
    try:
        assert lib.cmpc_set_gv_norm(h, L.GV_NORM_SAMPLE) == 0 and lib.cmpc_set_gv_norm(h, L.GV_NORM_BATCH) == 0
        for bad in (2, -1, 255):
            assert lib.cmpc_set_gv_norm(h, bad) == -1
            msg = lib.cmpc_last_error()
            assert b"set_gv_norm" in msg and str(bad).encode() in msg
        assert lib.cmpc_set_gv_norm(h, L.GV_NORM_SAMPLE) == 0      # a rejected value leaves the handle usable
    finally:
        assert lib.cmpc_destroy(h) == 0
    assert lib.cmpc_set_gv_norm(None, 0) == -1 and b"null handle" in lib.cmpc_last_error()


def _out(lib, d, nbytes, B=None, dt=0, H=32, m=1, out=1, value=255):
    return lib.cmpc_eval_mask_out(m, dt, len(d) if B is None else B, H, H, 0.5, d, out, nbytes, value, None)


def test_eval_mask_out_rejects_invalid_arguments_before_launch():
    """Every call below passes the fake pointer 1: had a kernel been launched (or a pointer been followed) the process would fault."""
    lib = L.load()
    m, mn = EV.plan_masks([(40, 30), (16, 50)], 32, 32)
    # NULL pointers
    assert _out(lib, m, mn, m=None) == -1 and b"eval_mask_out" in lib.cmpc_last_error()
    assert _out(lib, m, mn, out=None) == -1 and b"NULL" in lib.cmpc_last_error()
    assert lib.cmpc_eval_mask_out(1, 0, 2, 32, 32, 0.5, None, 1, mn, 255, None) == -1
    # B outside 1..CMPC_EVAL_MAX_BATCH
    assert _out(lib, m, mn, B=0) == -1 and _out(lib, m, mn, B=-2) == -1
    assert _out(lib, m, mn, B=L.EVAL_MAX_BATCH + 1) == -1 and b"outside" in lib.cmpc_last_error()
    # map dtype, value
    assert _out(lib, m, mn, dt=2) == -1 and b"dtype" in lib.cmpc_last_error()
    for v in (0, 2, 254, 256, -1):
        assert _out(lib, m, mn, value=v) == -1 and b"value" in lib.cmpc_last_error(), v
    # map size, buffer length
    assert lib.cmpc_eval_mask_out(1, 0, 2, 0, 32, 0.5, m, 1, mn, 255, None) == -1
    assert _out(lib, m, 0) == -1
    # offset + size beyond out_bytes, naming the sample
    assert _out(lib, m, mn - 1) == -1 and b"beyond" in lib.cmpc_last_error() and b"sample 1" in lib.cmpc_last_error()
    e = (L.EvalDesc * 2)(m[0], m[1])
    e[0].offset = mn - 10
    assert _out(lib, e, mn) == -1 and b"sample 0" in lib.cmpc_last_error()
    e[0].offset = -16
    assert _out(lib, e, mn) == -1
    # empty output, channels, a geometry that differs from resize_and_crop_geometry
    for field, val in (("h", 0), ("w", 0), ("c", 3), ("rh", m[1].rh + 1), ("rw", m[1].rw - 1), ("top", m[1].top + 1), ("left", m[1].left + 1)):
        e = (L.EvalDesc * 2)(m[0], m[1])
        setattr(e[1], field, val)
        assert _out(lib, e, mn) == -1 and b"sample 1" in lib.cmpc_last_error(), field
    e = (L.EvalDesc * 2)(m[0], m[1])
    e[1].rh += 1
    assert _out(lib, e, mn) == -1 and b"geometry" in lib.cmpc_last_error()
    # a shrink factor whose Gaussian radius exceeds the limit (63): a 1024 x 1024 map onto a 16 x 16 mask (factor 64, radius 126);
    # sample 0's factor of 25.6 (radius 49) is within it
    big, bn = EV.plan_masks([(40, 30), (16, 16)], 1024, 1024)
    assert _out(lib, big, bn, H=1024) == -1
    msg = lib.cmpc_last_error()
    assert b"shrink factor" in msg and b"sample 1" in msg


def test_option_values_are_checked():
    assert EV.check_gv_norm(None) is None and EV.check_gv_norm("sample") == "sample" and EV.check_gv_norm("batch") == "batch"
    for bad in ("row", 1, ""):
        with pytest.raises(ValueError):
            EV.check_gv_norm(bad)
    with pytest.raises(ValueError):
        EV.check_gv_norm(None, allow_none=False)
    with pytest.raises(ValueError):
        EV.masks_out(np.zeros((1, 4, 4), np.float32), [(4, 4)])        # not a device tensor


# ---- FrameSegmenter's host half ------------------------------------------------------------------------------------------------------
class FakeModel:
    video = False

    def __init__(self, B=4, T=6, H=64, W=64):
        self.batch_size, self.num_steps, self.H, self.W = B, T, H, W
        self.gv_norm = "batch"
        self.modes = []

    def set_gv_norm(self, mode):
        self.gv_norm = mode
        self.modes.append(mode)


class FakeStage:
    """Stands for _DeviceStage: frames carry their index in pixel [0, 0, 0]; the 'mask' of (e, f) is filled with 10 * e + f + 1.
    segment() refuses a ring slot whose previous masks the consumer has not all received."""

    def __init__(self, nslots, ready=True, check_reuse=True):
        self.check_reuse = check_reuse
        self.bufs = [np.zeros(1 << 20, np.uint8) for _ in range(nslots)]
        self.holds = [None] * nslots            # (e, frame ids) last written to the slot
        self.consumed = set()
        self.ready = ready
        self.log = []
        self.reserved = 0

    def reserve(self, nbytes):
        self.reserved = max(self.reserved, nbytes)

    def set_expressions(self, exprs):
        self.exprs = exprs

    def begin(self, images):
        ids = [int(a.reshape(-1)[0]) for a in images]
        self.log.append(("begin", ids))
        return ids

    def segment(self, token, e, descs, nbytes, slot):
        assert nbytes <= self.reserved
        if self.check_reuse and self.holds[slot] is not None:
            pe, pf = self.holds[slot]
            missing = [(pe, f) for f in pf if (pe, f) not in self.consumed]
            assert not missing, "slot %d rewritten before %s were handed out" % (slot, missing)
        frames = token[: len(descs)]
        self.holds[slot] = (e, frames)
        self.log.append(("segment", e, frames, slot))
        for f, d in zip(frames, descs):
            self.bufs[slot][d.offset: d.offset + d.h * d.w] = 10 * e + f + 1

    def done(self, slot):
        return self.ready

    def wait(self, slot):
        self.log.append(("wait", slot))

    def view(self, slot):
        return self.bufs[slot]


SIZES = [(48, 64), (36, 64), (33, 50), (43, 64)]


def _frames(n):
    out = []
    for f in range(n):
        h, w = SIZES[f % len(SIZES)]
        a = np.zeros((h, w, 3), np.uint8)
        a[0, 0, 0] = f
        out.append(a)
    return out


def _exprs(T=6):
    return [(np.array([3, 4, 0, 0, 0, 0][:T]), 2), (np.array([5, 6, 7, 8, 9, 1][:T]), 6), (np.array([2, 0, 0, 0, 0, 0][:T]), 1)]


def test_plan_batches():
    assert SG.plan_batches(1, 4) == [[0, 0, 0, 0]]
    assert SG.plan_batches(4, 4) == [[0, 1, 2, 3]]
    assert SG.plan_batches(7, 4) == [[0, 1, 2, 3], [4, 5, 6, 4]]
    with pytest.raises(ValueError):
        SG.plan_batches(0, 4)


@pytest.mark.parametrize("n", [1, 4, 7])
@pytest.mark.parametrize("depth,ready,copy", [(1, True, True), (2, False, True), (3, True, False), (2, False, False)])
def test_segmenter_order_batches_and_slot_reuse(n, depth, ready, copy):
    B = 4
    model = FakeModel(B=B)
    st = FakeStage(depth + 1, ready=ready)
    seg = SG.FrameSegmenter(model, depth=depth, copy=copy, _stage=st)
    frames, exprs = _frames(n), _exprs()
    got = []
    for e, f, mk in seg.run(iter(frames), exprs):          # any iterable: read lazily
        h, w = frames[f].shape[:2]
        assert mk.dtype == np.uint8 and mk.shape == (h // 2, w // 2)
        assert np.all(mk == 10 * e + f + 1)                # the right slot, offset and extent, still intact when handed out
        got.append((e, f))
        st.consumed.add((e, f))
    # yield order: frame batches in order, within a batch expressions in order, within those frames in order
    want = [(e, f) for b in SG.plan_batches(n, B) for e in range(len(exprs)) for f in sorted(set(b))]
    assert got == want
    # the device stage saw every frame batch once, padded by repeating its first frame, and one segment() per (batch, expression)
    begins = [x[1] for x in st.log if x[0] == "begin"]
    assert begins == SG.plan_batches(n, B)
    segs = [(x[1], x[2]) for x in st.log if x[0] == "segment"]
    assert segs == [(e, sorted(set(b))) for b in SG.plan_batches(n, B) for e in range(len(exprs))]
    # the next batch's backbone pass is enqueued ahead of this batch's heads
    if n > B:
        order = [x[0] for x in st.log if x[0] != "wait"]
        assert order[:3] == ["begin", "begin", "segment"]
    # at most depth + 1 slots, and the model's own mode is back
    assert {x[3] for x in st.log if x[0] == "segment"} <= set(range(depth + 1))
    assert model.modes == ["sample", "batch"] and model.gv_norm == "batch"
    assert [(i.tolist(), k) for i, k in st.exprs] == [(i.tolist(), k) for i, k in exprs]


def test_segmenter_geometry_of_odd_sizes_and_out_size():
    model = FakeModel(B=2, H=320, W=320)
    st = FakeStage(3, check_reuse=False)
    seen = []
    orig = st.segment

    def spy(token, e, descs, nbytes, slot):
        seen.append([(d.offset, d.h, d.w, d.c, d.rh, d.rw, d.top, d.left) for d in descs])
        orig(token, e, descs, nbytes, slot)
    st.segment = spy
    frames = [np.zeros((333, 500, 3), np.uint8), np.zeros((427, 640), np.uint8)]
    list(SG.FrameSegmenter(model, _stage=st).run(frames, _exprs()[:1]))
    (d0, d1), = seen
    assert d0[:4] == (0, 166, 250, 1) and d0[4:] == HU.resize_and_crop_geometry(320, 320, 166, 250)
    assert d1[1:4] == (213, 320, 1) and d1[4:] == HU.resize_and_crop_geometry(320, 320, 213, 320)
    assert d1[0] == -(-166 * 250 // 16) * 16
    # a caller's out_size: the frame's own size
    seen.clear()
    out = list(SG.FrameSegmenter(model, out_size=lambda h, w: (h, w), value=1, _stage=st).run(frames, _exprs()[:1]))
    assert [m.shape for _, _, m in out] == [(333, 500), (427, 640)]
    assert seen[0][0][4:] == HU.resize_and_crop_geometry(320, 320, 333, 500)
    with pytest.raises(ValueError, match="frame 1"):
        list(SG.FrameSegmenter(model, out_size=lambda h, w: (h if h < 400 else 0, w), _stage=st).run(frames, _exprs()[:1]))


def test_segmenter_rejects_bad_inputs():
    model = FakeModel()
    st = FakeStage(3, check_reuse=False)
    seg = SG.FrameSegmenter(model, _stage=st)
    good = _frames(2)
    with pytest.raises(ValueError, match="frame 1"):
        list(seg.run([good[0], np.zeros((8, 8, 3), np.float32)], _exprs()))
    with pytest.raises(ValueError, match="frame 0"):
        list(seg.run([np.zeros((8, 8, 2), np.uint8)], _exprs()))
    with pytest.raises(ValueError, match="no frames"):
        list(seg.run([], _exprs()))
    with pytest.raises(ValueError, match="no expressions"):
        list(seg.run(good, []))
    vocab = {"<pad>": 0, "<unk>": 1, "a": 2, "dog": 3}
    with pytest.raises(ValueError, match="vocabulary"):
        list(seg.run(good, ["a dog"]))
    segv = SG.FrameSegmenter(model, vocab=vocab, _stage=st)
    with pytest.raises(ValueError, match="expression 1: empty sentence"):
        list(segv.run(good, ["a dog", ""]))
    list(segv.run(good, ["a dog"]))
    assert (st.exprs[0][0].tolist(), st.exprs[0][1]) == HU.preprocess_sentence_lstm("a dog", vocab, model.num_steps)
    for bad in ((np.zeros(5, np.int64), 2), (np.zeros(6, np.float32), 2), (np.zeros(6, np.int64), 0), (np.zeros(6, np.int64), 7), 5):
        with pytest.raises(ValueError, match="expression 0"):
            list(seg.run(good, [bad]))
    assert model.gv_norm == "batch"                       # restored after every failed run as well
    video = FakeModel()
    video.video = True
    with pytest.raises(ValueError, match="video model"):
        SG.FrameSegmenter(video, _stage=st)
    with pytest.raises(ValueError, match="batch_size"):
        SG.FrameSegmenter(FakeModel(B=L.EVAL_MAX_BATCH + 1), _stage=st)
    for kw in (dict(value=2), dict(depth=0), dict(gv_norm=None), dict(gv_norm="rows"), dict(dcrf_method="fast")):
        with pytest.raises(ValueError):
            SG.FrameSegmenter(model, _stage=st, **kw)
