"""CPU tests of the mask-cleaning feature: tests/cc_ref.py against scipy.ndimage.label, hostutil.clean_mask against cc_ref.clean,
hostutil.CleanLog, segment.CleanPlan's offsets behind every combination of tails, the two segmenters' host halves with clean= through
fake stages, and cmpc_mask_components' argument validation (before anything is launched: the library loads without a GPU)."""
import ctypes
import importlib
import json

import numpy as np
import pytest
from scipy import ndimage

from tests import cc_ref as R
from tests import test_clip_segment_host as TC
from tests import test_segment_host as TS

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
SG = importlib.import_module("cmpc-refseg_amd.segment")
L = importlib.import_module("cmpc-refseg_amd._lib")

TH, TW = L.CC_TILE_H, L.CC_TILE_W
INPUTS = R.all_inputs(TH, TW)
STRUCTURE = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}


def test_the_exported_constants_match_the_header():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmpc.h")).read()
    c = {k: int(eval(v)) for k, v in re.findall(r"#define (CMPC_CC_\w+) (\(?[\d <]+\)?)", text)}
    assert c == {"CMPC_CC_MAX_KEEP": L.CC_MAX_KEEP, "CMPC_CC_MAX_PIXELS": L.CC_MAX_PIXELS, "CMPC_CC_TILE_H": TH, "CMPC_CC_TILE_W": TW}
    assert L.CC_MAX_KEEP == HU.CLEAN_MAX_KEEP == 8 and L.CC_MAX_PIXELS == 1 << 24
    assert ctypes.sizeof(L.CcDesc) == 16
    lib = L.load()
    assert hasattr(lib, "cmpc_mask_components") and hasattr(lib, "cmpc_mask_components_workspace") and lib.cmpc_abi_version() == 4


@pytest.mark.parametrize("conn", [4, 8])
def test_cc_ref_against_scipy_label(conn):
    counts, largest = [], []
    for name, m in INPUTS:
        lab, n = ndimage.label(m, structure=STRUCTURE[conn])
        got = R.labels(m, conn)
        assert got.dtype == np.int32 and np.array_equal(got != 0, m), name
        if n == 0:
            assert not got.any(), name
            continue
        idx = np.arange(m.size).reshape(m.shape)
        first = ndimage.minimum(idx, lab, index=np.arange(1, n + 1)).astype(np.int64)
        assert np.all(np.diff(first) > 0), name            # SciPy numbers components by their first pixel in raster order
        assert np.array_equal(got, np.where(lab > 0, np.concatenate([[0], first + 1])[lab], 0)), name
        if name.startswith("noise"):
            counts.append(n)
            largest.append(int(np.bincount(lab.reshape(-1))[1:].max()))
    # both "many tiny" and "one tortuous giant" are among the noise masks
    if conn == 4:
        assert counts == [1744, 1406, 936, 405, 114] and largest == [22, 53, 169, 1527, 8655]
    else:
        assert counts == [640, 216, 66, 21, 3] and largest == [169, 3061, 6147, 7454, 8876]


@pytest.mark.parametrize("conn", [4, 8])
def test_clean_mask_against_cc_ref(conn):
    for name, m in INPUTS:
        a = m.astype(np.uint8) * 255
        lab = R.labels(m, conn)
        for keep in R.KEEPS:
            for min_area in R.MIN_AREAS:
                want, want_stats, _ = R.clean(a, keep, min_area, conn, lab=lab)
                got, stats = HU.clean_mask(a, keep, min_area, conn)
                assert got.dtype == np.uint8 and got is not a and np.array_equal(got, want), (name, keep, min_area)
                assert stats.dtype == np.int64 and np.array_equal(stats, want_stats), (name, keep, min_area, stats, want_stats)
    # kept pixels keep their value, whatever the dtype; the defaults keep the largest 8-connected component
    m = np.zeros((6, 9), np.float32)
    m[0, :3], m[2:5, 4:8], m[5, 0] = 0.5, 7.0, -1.0
    got, stats = HU.clean_mask(m)
    assert got.dtype == np.float32 and np.array_equal(got, np.where(m == 7.0, m, 0)) and stats.tolist() == [3, 16, 12, 12]
    for bad in (dict(keep=9), dict(keep=-1), dict(min_area=-1), dict(connectivity=6), dict(keep=1.0), dict(keep=True)):
        with pytest.raises(ValueError):
            HU.clean_mask(m, **bad)
    with pytest.raises(ValueError):
        HU.clean_mask(np.zeros((2, 2, 2)))


def test_the_closed_form_frame_at_24_x_40():
    m, count, area, largest, second = R.closed_form_frame(24, 40)
    assert (count, area, largest, second) == (31, 240 + 4 * 29 + 9, 240, 9)
    for conn in (4, 8):
        _, stats, lab = R.clean(m, 2, 0, conn)
        assert stats.tolist() == [count, area, largest, largest + second] and int(m.sum()) == area
        assert np.all(lab[:, :19][m[:, :19]] == 1)
        assert R.clean(m, 0, 5, conn)[1][3] == largest + second


def test_clean_log():
    log = HU.CleanLog()
    log.add(("v", 0), 2, np.array([3, 100, 80, 80]))
    log.add(("v", 0), 0, [1, 50, 50, 50])
    log.add(("v", 1), 0, (0, 0, 0, 0))
    log.add("w", 5, (4, 100, 90, 90))
    assert len(log) == 4
    with pytest.raises(ValueError, match="already holds"):
        log.add(("v", 0), 2, (1, 1, 1, 1))
    for bad in ((1, 10, 11, 5), (1, 10, 5, 11), (0, 5, 5, 5), (2, 0, 0, 0), (1, -1, 0, 0)):
        with pytest.raises(ValueError, match="impossible"):
            log.add("x", 0, bad)
    st, ids = log.stats(("v", 0))
    assert ids == [0, 2] and st.dtype == np.int64 and st.tolist() == [[1, 50, 50, 50], [3, 100, 80, 80]]
    with pytest.raises(KeyError):
        log.stats("nope")
    assert log.fragmented() == [(("v", 0), 2)]             # 0.8 < 0.9; exactly 0.9 is not below; the empty frame never
    assert log.fragmented(0.95) == [(("v", 0), 2), ("w", 5)] and log.fragmented(0.5) == []
    d = log.dump()
    assert json.loads(json.dumps(d)) == d and len(d) == 4
    assert d[0] == {"seq": ["v", 0], "frame": 0, "n_components": 1, "area": 50, "area_largest": 50, "area_kept": 50}


def test_clean_plan_offsets_behind_every_combination_of_tails():
    descs, nbytes = EV.plan_masks([(33, 50), (7, 9), (20, 31)], 64, 64)
    assert nbytes % 16 == 0
    n, C = 3, 24
    for scored in (None, 0, 2, 3):
        for described in (None, (n, C)):
            tail = SG._slot_tail(nbytes, scored, described)
            if described is not None:
                assert tail == SG.plan_describe(nbytes, scored or 0, n, C).end
            elif scored is not None:
                assert tail == SG.scored_bytes(nbytes, scored)
            else:
                assert tail == nbytes
            for extra in (0, 1, 4, 7):                       # a tail that does not end on an 8-byte boundary
                p = SG.CleanPlan(descs, (2, 5, 4), tail + extra)
                assert p.off % 8 == 0 and tail + extra <= p.off < tail + extra + 8 and p.end == p.off + 32 * n
                assert p.end == SG.cleaned_bytes(tail + extra, n)
                assert (p.n, p.keep, p.min_area, p.connectivity) == (n, 2, 5, 4)
                assert [(d.off, d.h, d.w) for d in p.descs] == [(e.offset, e.h, e.w) for e in descs]
                assert p.ws_bytes == 64 + 64 * n + 8 * sum(-(-d.h * d.w // 4) * 4 for d in descs)
                host = np.zeros(p.end + 3, np.uint8)
                host[p.off: p.end] = np.arange(4 * n, dtype=np.int64).view(np.uint8)
                assert SG.slot_clean(host, p).tolist() == np.arange(4 * n).reshape(n, 4).tolist()


def test_check_clean_option():
    assert SG.check_clean(None) is None
    assert SG.check_clean({}) == (1, 0, 8) and SG.check_clean({"keep": 0, "min_area": 30, "connectivity": 4}) == (0, 30, 4)

    class Opt:
        keep, min_area = 2, 9
    assert SG.check_clean(Opt()) == (2, 9, 8)
    for bad in ({"keeps": 1}, {"keep": 9}, {"min_area": -1}, {"connectivity": 5}, {"keep": "1"}, 1, "largest", True):
        with pytest.raises(ValueError):
            SG.check_clean(bad)
    with pytest.raises(ValueError):
        SG.FrameSegmenter(TS.FakeModel(), _stage=object(), clean={"keep": 9})
    with pytest.raises(ValueError):
        SG.ClipSegmenter(TC.FakeModel(), _stage=object(), clean={"connectivity": 6})


def _fake_stats(e, f):
    return [1 + e, 100 + f, 90 + f, 90 + f]


class CleanFrameStage(TS.FakeStage):
    """The older fake stage, taught the new keyword: the statistics of (e, f) go where the plan says."""

    def segment(self, token, e, descs, nbytes, slot, clean=None):
        self.kw = getattr(self, "kw", []) + [clean]
        super().segment(token, e, descs, nbytes, slot)
        assert clean.end <= self.reserved and clean.off >= nbytes and clean.n == len(descs)
        st = np.array([_fake_stats(e, f) for f in token[: len(descs)]], np.int64)
        self.bufs[slot][clean.off: clean.end] = st.reshape(-1).view(np.uint8)


def test_frame_segmenter_host_half_with_and_without_clean():
    frames, exprs = TS._frames(7), TS._exprs()
    # off: the stage that knows nothing of the keyword gets the old call shape
    old = TS.FakeStage(3, check_reuse=False)
    seg = SG.FrameSegmenter(TS.FakeModel(), _stage=old)
    plain = [(e, f, m) for e, f, m in seg.run(frames, exprs)]
    assert seg.clean is None and seg.cleaned is None
    reserved_plain = old.reserved
    # on: the keyword arrives, the statistics come out per (seq, e), frame
    st = CleanFrameStage(3, check_reuse=False)
    seg = SG.FrameSegmenter(TS.FakeModel(), _stage=st, clean={"keep": 2, "min_area": 4})
    log = HU.CleanLog()
    got = [(e, f, m) for e, f, m in seg.run(frames, exprs, seq="vid", cleaned=log)]
    assert [(e, f) for e, f, _ in got] == [(e, f) for e, f, _ in plain]
    assert all(np.array_equal(a[2], b[2]) for a, b in zip(got, plain))
    assert all(isinstance(c, SG.CleanPlan) and (c.keep, c.min_area, c.connectivity) == (2, 4, 8) for c in st.kw) and len(st.kw) == 2 * len(exprs)
    assert seg.cleaned is log and len(log) == len(exprs) * 7
    for e in range(len(exprs)):
        stats, ids = log.stats(("vid", e))
        assert ids == list(range(7)) and stats.tolist() == [_fake_stats(e, f) for f in range(7)]
    assert st.reserved == SG.cleaned_bytes(reserved_plain, 4) > reserved_plain       # reserve() accounts for the new tail
    # a fresh log when none is passed
    seg = SG.FrameSegmenter(TS.FakeModel(), _stage=CleanFrameStage(3, check_reuse=False), clean={})
    list(seg.run(frames[:2], exprs[:1]))
    assert isinstance(seg.cleaned, HU.CleanLog) and len(seg.cleaned) == 2


class CleanClipStage(TC.FakeStage):
    def finish(self, f, slot, nbytes, clean=None):
        self.kw = getattr(self, "kw", []) + [clean]
        assert clean.off >= nbytes and clean.n == self.E and clean.end <= self.reserved
        self.dev[clean.off: clean.end] = np.array([_fake_stats(e, f) for e in range(self.E)], np.int64).reshape(-1).view(np.uint8)
        super().finish(f, slot, clean.end)


def test_clip_segmenter_host_half_with_and_without_clean():
    n, E = 11, 3
    old = TC.FakeStage(32, 3, n)
    seg = SG.ClipSegmenter(TC.FakeModel(), _stage=old)
    plain = [(e, f, m) for e, f, m in seg.run(TC._frames(n), TC._exprs(E)) if not old.consumed.add((e, f))]
    assert seg.clean is None and seg.cleaned is None
    st = CleanClipStage(32, 3, n)
    seg = SG.ClipSegmenter(TC.FakeModel(), _stage=st, clean={"keep": 1})
    got = [(e, f, m) for e, f, m in seg.run(TC._frames(n), TC._exprs(E), seq=7) if not st.consumed.add((e, f))]
    assert [(e, f) for e, f, _ in got] == [(e, f) for e, f, _ in plain] and all(np.array_equal(a[2], b[2]) for a, b in zip(got, plain))
    assert len(st.kw) == n and all(isinstance(c, SG.CleanPlan) and (c.keep, c.min_area, c.connectivity) == (1, 0, 8) for c in st.kw)
    assert len(seg.cleaned) == n * E
    for e in range(E):
        stats, ids = seg.cleaned.stats((7, e))
        assert ids == list(range(n)) and stats.tolist() == [_fake_stats(e, f) for f in range(n)]
    assert st.reserved > old.reserved


# ---- cmpc_mask_components' argument validation -------------------------------------------------------------------------------------
def _descs(*shapes_offs):
    return (L.CcDesc * len(shapes_offs))(*[L.CcDesc(o, h, w) for h, w, o in shapes_offs])


def _call(lib, d, B=None, masks=1, mask_bytes=1 << 20, conn=8, keep=1, min_area=0, labels=None, stats=8, ws=16, ws_bytes=1 << 30):
    return lib.cmpc_mask_components(masks, mask_bytes, d, len(d) if B is None else B, conn, keep, min_area, labels, stats, ws, ws_bytes, None)


def test_mask_components_rejects_invalid_arguments_before_launch():
    """Every call below passes small fake pointers: had a kernel been launched (or a pointer been followed) the process would fault."""
    lib = L.load()
    d = _descs((40, 30, 1), (16, 50, 1301))
    need = ctypes.c_int64()
    assert lib.cmpc_mask_components_workspace(d, 2, ctypes.byref(need)) == 0
    assert need.value == 64 + 64 * 2 + 8 * (1200 + 800) == EV.cc_workspace(d, 2)
    one = _descs((1, 1, 0))
    assert lib.cmpc_mask_components_workspace(one, 1, ctypes.byref(need)) == 0 and need.value == 64 + 64 + 32
    big = _descs((4096, 4096, 0))
    assert lib.cmpc_mask_components_workspace(big, 1, ctypes.byref(need)) == 0 and need.value == 128 + 8 * (1 << 24)
    err = lib.cmpc_last_error
    # the workspace query validates what it is given
    assert lib.cmpc_mask_components_workspace(d, 2, None) == -1 and lib.cmpc_mask_components_workspace(None, 2, ctypes.byref(need)) == -1
    assert lib.cmpc_mask_components_workspace(d, 0, ctypes.byref(need)) == -1 and b"outside" in err()
    assert lib.cmpc_mask_components_workspace(d, L.EVAL_MAX_BATCH + 1, ctypes.byref(need)) == -1
    assert lib.cmpc_mask_components_workspace(_descs((4097, 4096, 0)), 1, ctypes.byref(need)) == -1 and b"pixels" in err()
    # NULL pointers, B
    for kw in (dict(masks=None), dict(stats=None), dict(ws=None)):
        assert _call(lib, d, **kw) == -1 and b"NULL" in err()
    assert lib.cmpc_mask_components(1, 1 << 20, None, 2, 8, 1, 0, None, 8, 16, 1 << 30, None) == -1
    assert _call(lib, d, B=0) == -1 and _call(lib, d, B=-1) == -1 and _call(lib, d, B=L.EVAL_MAX_BATCH + 1) == -1 and b"outside" in err()
    # connectivity, keep, min_area
    for c in (0, 1, 6, 9, -8):
        assert _call(lib, d, conn=c) == -1 and b"connectivity" in err(), c
    for k in (-1, L.CC_MAX_KEEP + 1):
        assert _call(lib, d, keep=k) == -1 and b"keep" in err(), k
    assert _call(lib, d, min_area=-1) == -1 and b"min_area" in err()
    # h or w < 1, too many pixels
    for h, w in ((0, 5), (5, 0), (-1, 5)):
        assert _call(lib, _descs((40, 30, 1), (h, w, 1301))) == -1 and b"sample 1" in err(), (h, w)
    assert _call(lib, _descs((4096, 4097, 0)), mask_bytes=1 << 30) == -1 and b"pixels" in err()
    # a mask outside mask_bytes, naming the sample
    assert _call(lib, d, mask_bytes=1301 + 799) == -1 and b"beyond" in err() and b"sample 1" in err()
    assert _call(lib, d, mask_bytes=1200) == -1 and b"sample 0" in err()
    assert _call(lib, _descs((40, 30, -1))) == -1 and b"sample 0" in err()
    # a short or misaligned workspace; misaligned stats and labels
    assert _call(lib, d, ws_bytes=EV.cc_workspace(d, 2) - 1) == -1 and b"workspace" in err() and b"needed" in err()
    assert _call(lib, d, ws=24) == -1 and b"aligned" in err()
    assert _call(lib, d, stats=12) == -1 and b"aligned" in err()
    assert _call(lib, d, labels=6) == -1 and b"aligned" in err()


def test_the_wrappers_validate_on_the_host():
    m = np.ones((4, 4), np.uint8)
    for fn, kw in ((EV.mask_clean, dict(keep=9)), (EV.mask_clean, dict(keep=-1)), (EV.mask_clean, dict(min_area=-2)),
                   (EV.mask_clean, dict(connectivity=5)), (EV.mask_components, dict(connectivity=0))):
        with pytest.raises(ValueError):
            fn([m], device="cuda:0", **kw)
    with pytest.raises(ValueError, match="no masks"):
        EV.mask_components([], device="cuda:0")
    with pytest.raises(ValueError, match="mask 1"):
        EV.mask_clean([m, np.zeros((2, 0))], device="cuda:0")
    with pytest.raises(ValueError):
        EV.cc_descs([(4097, 4096)], [0])
