"""GPU tests of cmpc_mask_jf: the six integers equal tests/jf_ref.py's exactly -- at edge shapes, for every mask kind, for radii whose
windows span two and three words or exceed the image, for a full batch of mixed sizes at unaligned offsets -- with guard bytes around
`counts` and past the stated workspace, and of evaluate.mask_jf on host arrays and device tensors."""
import importlib

import numpy as np
import pytest
import torch

from tests import jf_ref as R

pytestmark = pytest.mark.gpu

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
L = importlib.import_module("cmpc-refseg_amd._lib")

SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (7, 65), (33, 129), (64, 64), (63, 127), (90, 200)]
KINDS = ["noise", "rectangles", "empty_pred", "both_empty", "both_full", "gt_sparse"]
GUARD = 0xA5
GUARD_WORD = -0x5A5A5A5A5A5A5A5B                  # 0xA5 in every byte, as int64


def _pair(kind, h, w, rng):
    if kind == "noise":
        return rng.random((h, w)) < 0.5, rng.random((h, w)) < 0.5
    if kind == "rectangles":                       # two rectangles offset against each other (clipped by small images)
        p, g = np.zeros((h, w), bool), np.zeros((h, w), bool)
        p[h // 5: h // 5 + max(h // 2, 1), w // 6: w // 6 + max(w // 2, 1)] = True
        g[h // 5 + h // 8: h // 5 + h // 8 + max(h // 2, 1), w // 6 + 3: w // 6 + 3 + max(w // 2, 1)] = True
        return p, g
    if kind == "empty_pred":
        return np.zeros((h, w), bool), rng.random((h, w)) < 0.5
    if kind == "both_empty":
        return np.zeros((h, w), bool), np.zeros((h, w), bool)
    if kind == "both_full":
        return np.ones((h, w), bool), np.ones((h, w), bool)
    if kind == "gt_sparse":
        return rng.random((h, w)) < 0.5, rng.random((h, w)) < 0.1
    raise ValueError(kind)


def _pack(masks, aligned, value):
    """The masks (bool) as one uint8 buffer in {0, value}, between guard bytes: 16-byte aligned offsets, or odd ones from byte 1."""
    offs, off = [], 0 if aligned else 1
    for m in masks:
        offs.append(off)
        off += -(-m.size // 16) * 16 if aligned else m.size + m.size % 2                  # keeps the following offsets odd
    buf = np.full(off + 3, GUARD, np.uint8)
    for m, o in zip(masks, offs):
        buf[o: o + m.size] = m.reshape(-1).astype(np.uint8) * value
    return buf, offs


def _run(preds, gts, radii, aligned=True, value=(255, 1), slack=64):
    """cmpc_mask_jf through the C ABI with the minimal workspace; checks the guards; returns int64 [B, 6]."""
    B = len(preds)
    pb, po = _pack(preds, aligned, value[0])
    gb, go = _pack(gts, aligned, value[1])
    d = (L.JfDesc * B)(*[L.JfDesc(po[i], go[i], preds[i].shape[0], preds[i].shape[1], radii[i], 0) for i in range(B)])
    need = EV.jf_workspace(d, B)
    assert need == sum(16 * m.shape[0] * -(-m.shape[1] // 64) for m in preds)
    pd, gd = torch.from_numpy(pb).cuda(), torch.from_numpy(gb).cuda()
    counts = torch.full((B + 2, 6), GUARD_WORD, dtype=torch.int64, device="cuda")
    ws = torch.full((need // 8 + slack,), GUARD_WORD, dtype=torch.int64, device="cuda")
    L.call("cmpc_mask_jf", pd.data_ptr(), pb.size, gd.data_ptr(), gb.size, d, B, counts[1].data_ptr(), ws.data_ptr(), need,
           torch.cuda.current_stream().cuda_stream)
    c = counts.cpu().numpy()
    assert np.all(c[0] == GUARD_WORD) and np.all(c[-1] == GUARD_WORD), "words around counts were written"
    assert torch.all(ws[need // 8:] == GUARD_WORD).item(), "words past ws_bytes were written"
    assert torch.equal(pd.cpu(), torch.from_numpy(pb)) and torch.equal(gd.cpu(), torch.from_numpy(gb)), "the masks were written"
    return c[1:-1]


def _ref(preds, gts, radii):
    return np.stack([R.counts(p, g, r) for p, g, r in zip(preds, gts, radii)])


@pytest.mark.parametrize("kind", KINDS)
def test_counts_exact_every_shape(kind):
    rng = np.random.default_rng(KINDS.index(kind))
    pairs = [_pair(kind, h, w, rng) for h, w in SHAPES]
    preds, gts = [p for p, _ in pairs], [g for _, g in pairs]
    radii = [HU.jf_radius(h, w) for h, w in SHAPES]
    assert radii == [1, 1, 1, 1, 1, 2, 1, 2, 2]
    got, want = _run(preds, gts, radii), _ref(preds, gts, radii)
    assert np.array_equal(got, want), (kind, np.argwhere(got != want).tolist())
    if kind == "both_empty":
        assert not got.any()
    if kind == "both_full":
        assert np.array_equal(got[:, :2], [[h * w, h * w] for h, w in SHAPES]) and not got[:, 2:].any()


RADII = [1, 2, 5, 31, 32, 33, 64, 70, 128]


@pytest.mark.parametrize("density", [0.5, 0.004])
def test_counts_exact_every_radius(density):
    """(40, 200): four words per row, one of them partial.  Dense noise, and a few isolated pixels whose discs reach the neighbouring
    words (radius >= 32), the ones after (>= 65) and past the image."""
    rng = np.random.default_rng(5)
    p, g = rng.random((40, 200)) < density, rng.random((40, 200)) < density
    preds, gts = [p] * len(RADII), [g] * len(RADII)
    got, want = _run(preds, gts, RADII), _ref(preds, gts, RADII)
    assert np.array_equal(got, want), np.argwhere(got != want).tolist()
    assert np.all(np.diff(got[:, 4]) >= 0) and np.all(np.diff(got[:, 5]) >= 0)          # a larger disc matches no fewer pixels
    if density < 0.1:
        assert got[0, 4] < got[-1, 4] == got[-1, 2]                                      # at radius 128 every boundary pixel here has a partner


def test_full_batch_mixed_sizes_unaligned_values_and_reruns():
    rng = np.random.default_rng(9)
    shapes = [SHAPES[(3 * i) % len(SHAPES)] for i in range(L.EVAL_MAX_BATCH)]
    pairs = [_pair(KINDS[i % len(KINDS)], h, w, rng) for i, (h, w) in enumerate(shapes)]
    preds, gts = [p for p, _ in pairs], [g for _, g in pairs]
    radii = [1 + i % 4 for i in range(len(shapes))]
    want = _ref(preds, gts, radii)
    got = _run(preds, gts, radii, aligned=False)
    assert np.array_equal(got, want), np.argwhere(got != want).tolist()
    # any non-zero byte is foreground; a second call gives the same integers (the counters are cleared, not accumulated)
    for value in ((1, 255), (7, 7), (255, 1)):
        assert np.array_equal(_run(preds, gts, radii, aligned=False, value=value), want), value


def test_default_radius_at_360_x_640_and_the_wrapper():
    rng = np.random.default_rng(13)
    p, g = rng.random((360, 640)) < 0.5, rng.random((360, 640)) < 0.5
    assert HU.jf_radius(360, 640) == 6
    want = R.counts(p, g, 6)
    assert np.array_equal(_run([p], [g], [6])[0], want)
    # evaluate.mask_jf: host arrays of any dtype and device uint8 tensors, mixed sizes, more pairs than one call takes
    small = [_pair(KINDS[i % len(KINDS)], *SHAPES[i % len(SHAPES)], rng) for i in range(L.EVAL_MAX_BATCH + 5)]
    preds = [p] + [a for a, _ in small]
    gts = [g] + [b for _, b in small]
    ref = np.stack([R.counts(a, b, HU.jf_radius(*a.shape)) for a, b in zip(preds, gts)])
    as_dev = lambda m, v: torch.from_numpy(m.astype(np.uint8) * v).cuda()
    mixed_p = [as_dev(m, 255) if i % 2 == 0 else m.astype(np.float32) for i, m in enumerate(preds)]
    mixed_g = [as_dev(m, 3) if i % 3 == 0 else m for i, m in enumerate(gts)]
    got = EV.mask_jf(mixed_p, mixed_g)
    assert got.dtype == np.int64 and got.shape == (len(preds), 6) and np.array_equal(got, ref)
    assert np.array_equal(EV.mask_jf(preds, gts, bound_th=3), np.stack([R.counts(a, b, 3) for a, b in zip(preds, gts)]))
    J, F = HU.jf_from_counts(got[0])
    print("360 x 640 noise pair: counts %s, J %.4f, F %.4f" % (got[0].tolist(), J, F))
    with pytest.raises(ValueError, match="pair 1"):
        EV.mask_jf([p, p], [g, g[:10]])
    with pytest.raises(ValueError, match="mask 0"):
        EV.mask_jf([torch.zeros(4, 4, device="cuda")], [np.zeros((4, 4))])
