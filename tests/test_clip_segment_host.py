"""CPU tests of the video model's prediction path over whole videos: the window rule (segment.clip_window / sampled_frames against a literal
restatement of build_A2D_batches.py's frame_range), the host half of segment.ClipSegmenter driven through a fake device stage that models
the ring of cached taps, the rejections, and cmpc_taps_copy's argument validation (before anything is launched: the library loads without
a GPU, and the fake pointers would fault if anything ran)."""
import ctypes
import importlib

import numpy as np
import pytest

SG = importlib.import_module("cmpc-refseg_amd.segment")
MD = importlib.import_module("cmpc-refseg_amd.model")
L = importlib.import_module("cmpc-refseg_amd._lib")

B = len(MD.FRAME_IDX)


# ---- the window rule -----------------------------------------------------------------------------------------------------------------
def _frame_range_1based(fid, n_frames, frames=16):
    """build_A2D_batches.py:150-167 restated: frame ids are 1-based, the clip holds ids fid - 8 .. fid + 7, each clamped to 1..n_frames."""
    out = []
    for k in range(frames):
        i = fid - frames // 2 + k
        if i < 1:
            i = 1
        if i > n_frames:
            i = n_frames
        out.append(i)
    return out


def test_window_rule_every_frame_of_short_and_long_videos():
    for n in range(1, 41):
        for f in range(n):
            want = [i - 1 for i in _frame_range_1based(f + 1, n)]
            assert SG.clip_window(f, n) == want, (n, f)
            assert want[8] == f and len(want) == 16
            assert SG.sampled_frames(f, n) == [want[k] for k in (0, 4, 8, 12, 15)], (n, f)
            assert SG.sampled_frames(f, n) == [min(max(f + d, 0), n - 1) for d in (-8, -4, 0, 4, 7)]
    assert MD.FRAME_IDX == (0, 4, 8, 12, 15)
    for bad in (-1, 5):
        with pytest.raises(ValueError):
            SG.clip_window(bad, 5)


def test_min_ring():
    assert [SG.min_ring(16, k) for k in (0, 1, 2)] == [20, 25, 30]          # frames - 1 + 5 * (lookahead + 1)
    assert SG.min_ring() == SG.min_ring(16, SG.CLIP_LOOKAHEAD) and SG.CLIP_LOOKAHEAD in (0, 1, 2)
    with pytest.raises(ValueError):
        SG.min_ring(15, 1)
    with pytest.raises(ValueError):
        SG.min_ring(16, -1)


# ---- ClipSegmenter's host half -------------------------------------------------------------------------------------------------------
class FakeModel:
    video = True

    def __init__(self, T=6, H=64, W=64, frames=16):
        self.batch_size, self.num_steps, self.H, self.W, self.frames = 1, T, H, W, frames


class FakeStage:
    """Stands for _ClipStage and models its buffers: ring[slot] = the frame whose taps the slot holds, gathered = the frames in the
    head's inputs.  Frames carry their index in pixel [0, 0, 0]; the 'mask' of (e, f) is filled with a value made of e, f and the clip
    the head saw.  Every call checks what the real stage relies on."""

    def __init__(self, ring, nslots, n_frames, ready=True):
        self.ring, self.nslots, self.n, self.ready = ring, nslots, n_frames, ready
        self.slots = [None] * ring
        self.gathered = None
        self.heads_done = {}                    # frame -> expressions enqueued
        self.bufs = [np.zeros(1 << 20, np.uint8) for _ in range(nslots)]
        self.dev = np.zeros(1 << 20, np.uint8)
        self.holds = [None] * nslots            # (frame, number of masks) last written to the slot
        self.consumed = set()
        self.log = []
        self.reserved = 0
        self.E = 0

    def reserve(self, nbytes):
        self.reserved = max(self.reserved, nbytes)

    def set_expressions(self, exprs):
        self.exprs = exprs
        self.E = len(exprs)

    def _oldest(self):
        """The oldest frame whose heads are not all enqueued."""
        f = 0
        while self.heads_done.get(f, 0) == self.E:
            f += 1
        return f

    def backbone(self, first, images, n):
        ids = [int(a.reshape(-1)[0]) for a in images]
        assert len(images) == B and 1 <= n <= B
        assert ids == list(range(first, first + n)) + [first] * (B - n), "consecutive frames, padded with the first"
        assert first % B == 0
        oldest = self._oldest()
        for j in range(n):
            s = (first + j) % self.ring
            ev = self.slots[s]
            # no slot is rewritten while a head not yet enqueued needs it: those heads read frames >= oldest - 8
            assert ev is None or ev < oldest - 8, "batch %d evicts frame %d, frame %d's heads still read from %d" % (first, ev, oldest, oldest - 8)
            self.slots[s] = first + j
        self.log.append(("backbone", first, n))

    def gather(self, f, idx):
        assert list(idx) == SG.sampled_frames(f, self.n)
        for g in idx:
            # written by an earlier backbone batch and not evicted since
            assert self.slots[g % self.ring] == g, "frame %d: frame %d is not in the ring (slot holds %r)" % (f, g, self.slots[g % self.ring])
        self.gathered = (f, list(idx))
        self.log.append(("gather", f))

    def head(self, f, e, descs, slot):
        assert self.gathered is not None and self.gathered[0] == f
        assert self.heads_done.get(f, 0) == e
        d = descs[e]
        assert d.offset + d.h * d.w <= self.reserved
        if e == 0 and self.holds[slot] is not None:
            pf, pe = self.holds[slot]
            missing = [(x, pf) for x in range(pe) if (x, pf) not in self.consumed]
            assert not missing, "slot %d rewritten before %s were handed out" % (slot, missing)
            self.holds[slot] = None
        self.dev[d.offset: d.offset + d.h * d.w] = (7 * e + f + 1) % 251
        self.heads_done[f] = e + 1
        self.log.append(("head", f, e, slot))

    def finish(self, f, slot, nbytes):
        assert nbytes <= self.reserved and self.heads_done[f] == self.E
        self.bufs[slot][:nbytes] = self.dev[:nbytes]
        self.holds[slot] = (f, self.E)
        self.log.append(("finish", f, slot))

    def done(self, slot):
        return self.ready

    def wait(self, slot):
        self.log.append(("wait", slot))

    def view(self, slot):
        return self.bufs[slot]


SIZES = [(48, 64), (36, 64), (33, 50), (43, 64)]


def _frames(n):
    for f in range(n):
        h, w = SIZES[f % len(SIZES)]
        a = np.zeros((h, w, 3), np.uint8)
        a[0, 0, 0] = f
        yield a


def _exprs(E, T=6):
    return [(np.array([3, 4, 0, 0, 0, 0][:T]), 2), (np.array([5, 6, 7, 8, 9, 1][:T]), 6), (np.array([2, 0, 0, 0, 0, 0][:T]), 1)][:E]


@pytest.mark.parametrize("n", [1, 4, 5, 6, 16, 23, 41])
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("big_ring", [False, True])
@pytest.mark.parametrize("depth,lookahead,ready", [(1, 1, True), (2, 2, False), (3, 0, True), (2, 1, False), (1, 2, True)])
def test_clip_segmenter_schedule(n, E, big_ring, depth, lookahead, ready):
    ring = 32 if big_ring else SG.min_ring(16, lookahead)
    st = FakeStage(ring, depth + 1, n, ready=ready)
    seg = SG.ClipSegmenter(FakeModel(), ring=ring, depth=depth, lookahead=lookahead, copy=(depth != 3), _stage=st)
    got = []
    for e, f, mk in seg.run(_frames(n), _exprs(E)):        # a generator: read lazily, its length unknown until it ends
        assert mk.dtype == np.uint8 and mk.shape == SIZES[f % len(SIZES)]          # the frame's own size by default
        assert np.all(mk == (7 * e + f + 1) % 251)          # the right slot, offset and extent, still intact when handed out
        got.append((e, f))
        st.consumed.add((e, f))
    assert got == [(e, f) for f in range(n) for e in range(E)]
    nb = -(-n // B)
    assert seg.stats == {"frames": n, "backbone_passes": nb, "gathers": n, "heads": n * E}
    assert [x[1:] for x in st.log if x[0] == "backbone"] == [(B * b, min(B, n - B * b)) for b in range(nb)]      # every frame once
    assert [x[1] for x in st.log if x[0] == "gather"] == list(range(n))
    assert [x[1:3] for x in st.log if x[0] == "head"] == [(f, e) for f in range(n) for e in range(E)]
    assert {x[2] for x in st.log if x[0] == "finish"} <= set(range(depth + 1))
    # the backbone runs `lookahead` batches ahead: when frame f's gather goes in, the batch of frame f + 7 and that many more are in
    seen = 0
    for x in st.log:
        if x[0] == "backbone":
            seen += 1
        elif x[0] == "gather":
            need = min(x[1] + 7, n - 1) // B + 1
            assert min(need + lookahead, nb) <= seen <= need + lookahead, (x, seen)


def test_clip_segmenter_second_run_and_stats_reset():
    st = FakeStage(32, 3, 7)
    seg = SG.ClipSegmenter(FakeModel(), _stage=st)
    assert seg.lookahead == SG.CLIP_LOOKAHEAD and seg.ring == 32
    a = [(e, f, mk.copy()) for e, f, mk in seg.run(_frames(7), _exprs(2)) if not st.consumed.add((e, f))]
    st.__init__(32, 3, 12)
    b = [(e, f) for e, f, mk in seg.run(list(_frames(12)), _exprs(1)) if not st.consumed.add((e, f))]
    assert len(a) == 14 and b == [(0, f) for f in range(12)]
    assert seg.stats == {"frames": 12, "backbone_passes": 3, "gathers": 12, "heads": 12}


def test_clip_segmenter_rejections():
    class Image:
        video = False
    with pytest.raises(ValueError, match="FrameSegmenter"):
        SG.ClipSegmenter(Image())
    with pytest.raises(ValueError, match="video"):           # and the other way round, as before
        SG.FrameSegmenter(FakeModel())
    m = FakeModel()
    for la in (0, 1, 2):
        with pytest.raises(ValueError, match="min_ring"):
            SG.ClipSegmenter(m, ring=SG.min_ring(16, la) - 1, lookahead=la, _stage=object())
        SG.ClipSegmenter(m, ring=SG.min_ring(16, la), lookahead=la, _stage=object())
    for kw in (dict(value=2), dict(value=0), dict(depth=0), dict(score="pred"), dict(lookahead=-1), dict(dcrf_method="nope")):
        with pytest.raises(ValueError):
            SG.ClipSegmenter(m, _stage=object(), **kw)

    def run(frames, exprs, **kw):
        st = FakeStage(32, 3, len(frames))
        return list(SG.ClipSegmenter(m, _stage=st, **kw).run(iter(frames), exprs))

    ok = list(_frames(3))
    assert len(run(ok, _exprs(1))) == 3
    with pytest.raises(ValueError, match="no frames"):
        run([], _exprs(1))
    with pytest.raises(ValueError, match="no expressions"):
        run(ok, [])
    with pytest.raises(ValueError, match="frame 1"):
        run([ok[0], ok[1].astype(np.float32), ok[2]], _exprs(1))
    with pytest.raises(ValueError, match="frame 2"):
        run([ok[0], ok[1], np.zeros((0, 5, 3), np.uint8)], _exprs(1))
    with pytest.raises(ValueError, match="frame 0.*empty"):
        run(ok, _exprs(1), out_size=lambda h, w: (0, w))
    with pytest.raises(ValueError, match="expression 1"):
        run(ok, [_exprs(1)[0], (np.zeros(6, np.int64), 0)])
    with pytest.raises(ValueError, match="expression 0.*vocabulary"):
        run(ok, ["a dog"])
    vocab = {"<pad>": 0, "<unk>": 1, "dog": 2}
    with pytest.raises(ValueError, match="expression 1: empty sentence"):
        run(ok, ["dog", ""], vocab=vocab)
    assert len(run(ok, ["dog", (np.array([2, 0, 0, 0, 0, 0]), 1)], vocab=vocab)) == 6


# ---- cmpc_taps_copy: exported, bound, and validated before anything is launched ---------------------------------------------------------
def _copy(lib, levels=3, dst=(16, 16, 16), src=(32, 32, 32), nbytes=(16, 9216, 65536), n=5, di=(0, 1, 2, 3, 4), si=(7, 7, 0, 31, 2),
          dcap=5, scap=32):
    vp = ctypes.c_void_p * 3
    arr = lambda t, v: None if v is None else t(*v)
    return lib.cmpc_taps_copy(levels, arr(vp, dst), arr(vp, src), arr(ctypes.c_int64 * 3, nbytes), n, arr(ctypes.c_int * 8, di),
                              arr(ctypes.c_int * 8, si), dcap, scap, None)


def test_taps_copy_is_exported_and_rejects_bad_arguments():
    lib = L.load()
    assert hasattr(lib, "cmpc_taps_copy") and "cmpc_taps_copy" in L.SIGNATURES
    assert lib.cmpc_abi_version() == L.ABI_VERSION == 4            # additive: one new symbol
    assert (L.TAPS_MAX_LEVELS, L.TAPS_MAX_FRAMES) == (3, 8)

    def bad(word, **kw):
        assert _copy(lib, **kw) == -1, kw
        msg = lib.cmpc_last_error()
        assert b"taps_copy" in msg and word in msg, (kw, msg)

    # the pointers are fake (1 is not even aligned): had anything been launched, the process would fault
    for k in ("dst", "src", "nbytes", "di", "si"):
        bad(b"NULL", **{k: None})
    bad(b"NULL pointer", dst=(16, 0, 16))
    bad(b"NULL pointer", src=(0, 32, 32))
    bad(b"level 2", src=(32, 32, 0))
    assert _copy(lib, levels=2, dst=(1, 1, 0), src=(1, 1, 0), n=0) == -1      # the third level is not looked at with two
    for lv in (0, 4, -1):
        bad(b"levels", levels=lv, dst=(1, 1, 1), src=(1, 1, 1))
    for n in (0, 9, -3):
        bad(b"outside 1..8", n=n, dst=(1, 1, 1), src=(1, 1, 1))
    for nb in ((0, 16, 16), (16, 24, 16), (16, 16, -16), (16, 16, 8)):
        bad(b"multiple of 16", nbytes=nb, dst=(1, 1, 1), src=(1, 1, 1))
    bad(b"too large", nbytes=(16, 16, 1 << 36), dst=(1, 1, 1), src=(1, 1, 1))
    bad(b"dst index 5", di=(0, 1, 2, 3, 5), dst=(1, 1, 1), src=(1, 1, 1))
    bad(b"dst index -1", di=(0, -1, 2, 3, 4), dst=(1, 1, 1), src=(1, 1, 1))
    bad(b"src index 32", si=(0, 1, 2, 3, 32), dst=(1, 1, 1), src=(1, 1, 1))
    bad(b"src index -2", si=(-2, 1, 2, 3, 4), dst=(1, 1, 1), src=(1, 1, 1))
    bad(b"capacity", dcap=0, dst=(1, 1, 1), src=(1, 1, 1))
    bad(b"capacity", scap=-1, dst=(1, 1, 1), src=(1, 1, 1))
    bad(b"duplicate dst index 3", di=(0, 3, 2, 3, 4), dst=(1, 1, 1), src=(1, 1, 1))
    bad(b"duplicate", n=8, di=(0, 1, 2, 3, 4, 5, 6, 0), si=(0,) * 8, dcap=8, dst=(1, 1, 1), src=(1, 1, 1))
    # repeated SOURCE indices are fine; with everything else in order only the fake pointers' alignment is left to object to
    bad(b"16-byte aligned", dst=(1, 1, 1), src=(1, 1, 1))
    bad(b"16-byte aligned", dst=(16, 16, 16), src=(32, 40, 32))
    with pytest.raises(L.CmpcError, match="taps_copy"):
        L.call("cmpc_taps_copy", 3, (ctypes.c_void_p * 3)(1, 1, 1), (ctypes.c_void_p * 3)(1, 1, 1), (ctypes.c_int64 * 3)(16, 16, 16), 9,
               (ctypes.c_int * 8)(), (ctypes.c_int * 8)(), 8, 8, None)
