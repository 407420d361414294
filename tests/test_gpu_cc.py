"""GPU tests of cmpc_mask_components through the C ABI: labels, cleaned masks and statistics equal tests/cc_ref.py's exactly -- at edge
shapes placed by the exported tile size, for patterns whose components cross every tile seam, for a full batch of mixed shapes at odd
offsets -- with guard bytes around `stats`, `labels`, the packed masks and past the stated workspace; the status word is read back
and must be 0 after every call.  Then evaluate.mask_components / mask_clean on host arrays and device tensors."""
import functools
import importlib

import numpy as np
import pytest
import torch

from tests import cc_ref as R

pytestmark = pytest.mark.gpu

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
L = importlib.import_module("cmpc-refseg_amd._lib")

TH, TW = L.CC_TILE_H, L.CC_TILE_W
SHAPES = R.shapes(TH, TW)
GUARD = 0xA5
GUARD_WORD = -0x5A5A5A5A5A5A5A5B                  # 0xA5 in every byte, as int64
GUARD_I32 = -0x5A5A5A5B
PAD = 5                                            # guard elements on either side of labels


def _pack(masks, aligned, value):
    """The masks (bool) as one uint8 buffer in {0, value}, between guard bytes: 16-byte aligned offsets, or odd ones from byte 1."""
    offs, off = [], 0 if aligned else 1
    for m in masks:
        offs.append(off)
        off += -(-m.size // 16) * 16 if aligned else m.size + m.size % 2 + 2             # keeps the following offsets odd, a gap between
    buf = np.full(off + 3, GUARD, np.uint8)
    for m, o in zip(masks, offs):
        buf[o: o + m.size] = m.reshape(-1).astype(np.uint8) * value
    return buf, offs


def _run(masks, conn, keep=0, min_area=0, aligned=True, value=255, want_labels=True, slack=64):
    """One cmpc_mask_components call with the minimal workspace; checks every guard and the status word; returns (the cleaned masks
    as uint8 arrays, the labels or None, int64 stats [B, 4])."""
    B = len(masks)
    buf, offs = _pack(masks, aligned, value)
    d = (L.CcDesc * B)(*[L.CcDesc(offs[i], masks[i].shape[0], masks[i].shape[1]) for i in range(B)])
    need = EV.cc_workspace(d, B)
    assert need == 64 + 64 * B + 8 * sum(-(-m.size // 4) * 4 for m in masks)
    md = torch.from_numpy(buf).cuda()
    stats = torch.full((B + 2, 4), GUARD_WORD, dtype=torch.int64, device="cuda")
    ws = torch.full((need // 8 + slack,), GUARD_WORD, dtype=torch.int64, device="cuda")
    total = sum(m.size for m in masks)
    lab = torch.full((total + 2 * PAD,), GUARD_I32, dtype=torch.int32, device="cuda") if want_labels else None
    L.call("cmpc_mask_components", md.data_ptr(), buf.size, d, B, conn, keep, min_area, lab[PAD:].data_ptr() if want_labels else None,
           stats[1].data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(ws.view(torch.int32)[0].item()) == 0, "the status word is set: a bounded loop reached its bound"
    st = stats.cpu().numpy()
    assert np.all(st[0] == GUARD_WORD) and np.all(st[-1] == GUARD_WORD), "words around stats were written"
    assert torch.all(ws[need // 8:] == GUARD_WORD).item(), "words past ws_bytes were written"
    got = md.cpu().numpy()
    inside = np.zeros(buf.size, bool)
    for m, o in zip(masks, offs):
        inside[o: o + m.size] = True
    assert np.array_equal(got[~inside], buf[~inside]), "bytes between or around the packed masks were written"
    labels = None
    if want_labels:
        lh = lab.cpu().numpy()
        assert np.all(lh[:PAD] == GUARD_I32) and np.all(lh[-PAD:] == GUARD_I32), "elements around labels were written"
        labels, first = [], PAD
        for m in masks:
            labels.append(lh[first: first + m.size].reshape(m.shape))
            first += m.size
    return [got[o: o + m.size].reshape(m.shape) for m, o in zip(masks, offs)], labels, st[1:-1]


@functools.lru_cache(maxsize=None)
def _inputs():
    return R.all_inputs(TH, TW)


@functools.lru_cache(maxsize=None)
def _ref_labels(i, conn):
    return R.labels(_inputs()[i][1], conn)


def _ref(i, conn, keep, min_area, value):
    """(cleaned uint8, stats, labels) of input i, computed once per (input, connectivity) and filtered per call."""
    m = _inputs()[i][1].astype(np.uint8) * value
    return R.clean(m, keep, min_area, conn, lab=_ref_labels(i, conn))


def _check(idx, conn, keep, min_area, got, value):
    masks, labels, stats = got
    for j, i in enumerate(idx):
        want_mask, want_stats, want_lab = _ref(i, conn, keep, min_area, value)
        name = (_inputs()[i][0], conn, keep, min_area)
        assert np.array_equal(stats[j], want_stats), (name, stats[j].tolist(), want_stats.tolist())
        if labels is not None:
            assert np.array_equal(labels[j], want_lab), (name, np.argwhere(labels[j] != want_lab)[:5].tolist())
        assert np.array_equal(masks[j], want_mask), (name, np.argwhere(masks[j] != want_mask)[:5].tolist())


def _of_kind(kind):
    return [i for i, (name, _) in enumerate(_inputs()) if name.startswith(kind + " ")]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("kind", R.PATTERNS + ("noise",))
def test_labels_stats_and_cleaning_exact(kind, conn):
    """Every shape of the pattern (or the five noise densities) in one call: label-only leaves the masks as they are, then every
    (keep, min_area) of the reference's grid."""
    idx = _of_kind(kind)
    assert len(idx) == (5 if kind == "noise" else len(SHAPES))
    masks = [_inputs()[i][1] for i in idx]
    got = _run(masks, conn)
    _check(idx, conn, 0, 0, got, 255)
    for m, out in zip(masks, got[0]):
        assert np.array_equal(out, m.astype(np.uint8) * 255)
    stats = got[2]
    if kind == "empty":
        assert not stats.any()
    if kind == "full":
        assert np.array_equal(stats, [[1, m.size, m.size, m.size] for m in masks])
    if kind == "checkerboard":                     # every foreground pixel its own component, or (with two rows and columns at least) one component
        n_fg = [int(m.sum()) for m in masks]
        assert stats[:, 0].tolist() == [n if conn == 4 or min(m.shape) == 1 else 1 for n, m in zip(n_fg, masks)]
    if kind in ("serpentine", "comb", "comb_tm"):
        assert stats[:, 0].tolist() == [1] * len(masks)
    if kind == "corner_touch":
        assert stats[-1, 0] == (2 if conn == 4 else 1) and stats[-1, 1] == 4 * 5 + 3 * 6
    if kind == "noise":
        print("noise, connectivity %d: components %s, largest %s" % (conn, stats[:, 0].tolist(), stats[:, 2].tolist()))
    for keep in (1, 2, 8):
        for min_area in R.MIN_AREAS:
            _check(idx, conn, keep, min_area, _run(masks, conn, keep, min_area), 255)
    _check(idx, conn, 0, 50, _run(masks, conn, 0, 50, want_labels=False), 255)


def _mixed_batch():
    n = len(_inputs())
    return [(7 * i) % n for i in range(L.EVAL_MAX_BATCH)]


@pytest.mark.parametrize("aligned,value", [(False, 255), (True, 1)])
def test_full_batch_mixed_shapes_and_each_sample_alone(aligned, value):
    idx = _mixed_batch()
    masks = [_inputs()[i][1] for i in idx]
    assert len({m.shape for m in masks}) >= 5
    got = _run(masks, 8, 2, 2, aligned=aligned, value=value)
    _check(idx, 8, 2, 2, got, value)
    for j, i in enumerate(idx):                    # the batch around a sample does not change its result
        one = _run([masks[j]], 8, 2, 2, aligned=aligned, value=value)
        assert np.array_equal(one[0][0], got[0][j]) and np.array_equal(one[1][0], got[1][j]) and np.array_equal(one[2][0], got[2][j])


def test_label_only_without_labels_and_reruns_bit_identical():
    idx = _of_kind("noise")
    masks = [_inputs()[i][1] for i in idx]
    out, labels, stats = _run(masks, 4, want_labels=False)
    assert labels is None
    for m, o in zip(masks, out):
        assert np.array_equal(o, m.astype(np.uint8) * 255)
    _check(idx, 4, 0, 0, (out, None, stats), 255)
    _check(idx, 4, 0, 1, _run(masks, 4, 0, 1, want_labels=False), 255)               # min_area 1 is label-only too
    a, b = _run(masks, 8, 3, 5), _run(masks, 8, 3, 5)
    for x, y in zip(a[0] + a[1] + [a[2]], b[0] + b[1] + [b[2]]):
        assert np.array_equal(x, y)


def test_filtering_edges():
    h, w = SHAPES[-1]
    two = R.pattern("two_rectangles", h, w, TH, TW)
    full = R.pattern("full", 7, 65, TH, TW)
    area = (h // 3) * (w // 3)
    first = np.zeros_like(two)
    first[: h // 3] = two[: h // 3]                # the upper-right rectangle comes first in raster order
    for conn in (4, 8):
        for keep in (1, 2, 8):                     # fewer components than keep (except keep = 1 on the two rectangles)
            out, _, st = _run([two, full], conn, keep, 0)
            assert st.tolist() == [[2, 2 * area, area, area if keep == 1 else 2 * area], [1, 455, 455, 455]]
            assert np.array_equal(out[0] != 0, first if keep == 1 else two) and out[1].all()
        # min_area above every area: nothing is left
        out, _, st = _run([two, full], conn, 0, 10 ** 9)
        assert st.tolist() == [[2, 2 * area, area, 0], [1, 455, 455, 0]] and not out[0].any() and not out[1].any()
        out, _, st = _run([two], conn, 8, 2 ** 40)
        assert st.tolist() == [[2, 2 * area, area, 0]] and not out[0].any()
        # min_area equal to the largest area: exactly the tied winners that keep allows
        for keep, want in ((1, first), (2, two), (0, two)):
            out, _, st = _run([two], conn, keep, area)
            assert np.array_equal(out[0] != 0, want) and st[0, 3] == want.sum()


@pytest.mark.parametrize("conn", [4, 8])
def test_one_frame_720_x_1280_in_closed_form(conn):
    m, count, area, largest, second = R.closed_form_frame(720, 1280)
    out, labels, st = _run([m], conn)
    assert st.tolist() == [[count, area, largest, area]]
    assert np.array_equal(out[0] != 0, m)
    lab = labels[0]
    assert np.array_equal(lab != 0, m) and np.all(lab[:, :639][m[:, :639]] == 1)        # the serpentine starts at pixel 0
    assert len(np.unique(lab)) == count + 1
    ys, xs = np.nonzero(m[:, 640:])
    block = 1 + (ys // 4 * 4) * 1280 + 640 + xs // 4 * 4                             # a block's first pixel is its lattice corner
    assert np.array_equal(lab[:, 640:][m[:, 640:]], block)
    out, _, st = _run([m], conn, 1, 0, want_labels=False)
    assert st.tolist() == [[count, area, largest, largest]] and out[0][:, 640:].sum() == 0 and np.array_equal(out[0][:, :640] != 0, m[:, :640])
    out, _, st = _run([m], conn, 2, 0, want_labels=False)
    assert st.tolist() == [[count, area, largest, largest + second]] and (out[0][:, 640:] != 0).sum() == 9
    out, _, st = _run([m], conn, 0, 5, want_labels=False)
    assert st.tolist() == [[count, area, largest, largest + second]]


def test_wrappers_host_arrays_device_tensors_and_their_checks():
    n = L.EVAL_MAX_BATCH + 5
    idx = [(5 * i + 3) % len(_inputs()) for i in range(n)]
    masks = [_inputs()[i][1] for i in idx]
    as_dev = lambda m: torch.from_numpy(m.astype(np.uint8) * 255).cuda()
    mixed = [as_dev(m) if j % 2 == 0 else m.astype(np.float32) * 3 for j, m in enumerate(masks)]
    labels, stats = EV.mask_components(mixed, connectivity=4)
    assert stats.dtype == np.int64 and stats.shape == (n, 4)
    for j, i in enumerate(idx):
        _, want_stats, want_lab = _ref(i, 4, 0, 0, 1)
        assert torch.is_tensor(labels[j]) == (j % 2 == 0)
        got = labels[j].cpu().numpy() if j % 2 == 0 else labels[j]
        assert got.dtype == np.int32 and np.array_equal(got, want_lab) and np.array_equal(stats[j], want_stats)
        if j % 2 == 0:
            assert torch.equal(mixed[j], as_dev(masks[j]))                             # label-only reads a device mask in place
    cleaned, stats = EV.mask_clean(mixed, keep=2, min_area=3)
    for j, i in enumerate(idx):
        want_mask, want_stats, _ = _ref(i, 8, 2, 3, 1)
        assert np.array_equal(stats[j], want_stats)
        if j % 2 == 0:
            assert cleaned[j] is mixed[j] and np.array_equal(cleaned[j].cpu().numpy(), want_mask * 255)    # cleaned in place
        else:
            assert cleaned[j].dtype == np.float32 and np.array_equal(cleaned[j], want_mask.astype(np.float32) * 3)
            assert cleaned[j] is not mixed[j] and np.array_equal(mixed[j] != 0, masks[j])                 # a new array
        host_mask, host_stats = HU.clean_mask(masks[j], 2, 3, 8)
        assert np.array_equal(host_mask, want_mask != 0) and np.array_equal(host_stats, want_stats)
    with pytest.raises(ValueError, match="keep"):
        EV.mask_clean([masks[0]], keep=9)
    with pytest.raises(ValueError, match="min_area"):
        EV.mask_clean([masks[0]], min_area=-1)
    with pytest.raises(ValueError, match="connectivity"):
        EV.mask_components([masks[0]], connectivity=6)
    with pytest.raises(ValueError, match="mask 1"):
        EV.mask_components([masks[0], torch.zeros(4, 4, device="cuda")])
    with pytest.raises(ValueError, match="no masks"):
        EV.mask_clean([])
