"""GPU tests of the resampling kernels of csrc/ops_eval.hip (cmpc_eval_prep, cmpc_train_prep, cmpc_clip_prep, cmpc_eval_mask_iu,
cmpc_eval_mask_out) against the dense float64 reference of tests/resample_ref.py, at odd non-square outputs -- (23, 41), (41, 23) and
(32, 32): every tile is partial -- and at the sources that walk eval_prep_kernel through all eight LDS tile shapes and
train_target_kernel through all seven it can reach (tests/test_resample_ref_host.py checks that they do, and that the reference agrees
with hostutil on every case used here).

  prep bytes      |byte - 255 * dense| <= 0.5 + 1e-9 on EVERY pixel of the resized rectangle: img_as_ubyte's rounding and the reference's
                  float64 error bound, no share of pixels left out; padding 0; feed bit-equal to float32(float64(byte) - mu)
  tile invariance a sample's bytes do not depend on the tile its neighbours force on the launch (no reference needed)
  targets, masks  binary decisions, exactly equal
  refusals        decided on the host, outputs untouched, the next call unharmed
"""
import functools
import importlib

import numpy as np
import pytest
import torch

from tests import resample_ref as R

pytestmark = pytest.mark.gpu

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
FD = importlib.import_module("cmpc-refseg_amd.feed")
L = importlib.import_module("cmpc-refseg_amd._lib")

MARGIN = 1e-9              # the reference's float64 error bound in grey levels (tests/test_resample_ref_host.py)
GUARD = 0xA5
KEY = FD.REFVOS_OBJECT_COLOR["3"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(feed):
    return feed.contiguous().view(torch.int32)


# ---- cmpc_eval_prep -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _prep_images(out):
    return [R.image(h, w, c) for h, w, c in R.prep_cases(out)]


@functools.lru_cache(maxsize=None)
def _prep_alone(out):
    """[(proc uint8 [H, W, 3], feed float32 [H, W, 3])] of every image of `out` prepared alone: each launch picks the sample's own tile."""
    res = [EV.prepare_images([im], out[0], out[1]) for im in _prep_images(out)]
    return [(proc[0].cpu().numpy(), feed[0].cpu().numpy()) for feed, proc in res]


@pytest.mark.parametrize("out", R.OUTS)
def test_prep_bytes_against_dense(out):
    H, W = out
    n_id = 0
    for (h, w, c), im, (proc, feed) in zip(R.prep_cases(out), _prep_images(out), _prep_alone(out)):
        rh, rw, top, left = HU.resize_and_pad_geometry(h, w, H, W)
        dense = 255.0 * R.dense_pad(im.reshape(h, w) if c != 3 else im, H, W)
        if c != 3:
            assert np.array_equal(proc[..., 0], proc[..., 1]) and np.array_equal(proc[..., 0], proc[..., 2]), (out, (h, w, c))
            dense = np.repeat(dense[..., None], 3, 2)
        inside = np.zeros((H, W), bool)
        inside[top: top + rh, left: left + rw] = True
        err = np.abs(proc.astype(np.float64) - dense)
        print("out %s source %s tile %s: worst |byte - 255 dense| %.6f" % (out, (h, w, c), R.tile_choice("prep", [(h, w, c or 1)], H, W), err[inside].max()))
        assert err[inside].max() <= 0.5 + MARGIN, (out, (h, w, c), float(err[inside].max()), int((err[inside] > 0.5 + MARGIN).sum()))
        assert not proc[~inside].any(), (out, (h, w, c), "padding")
        want = (proc[..., ::-1].astype(np.float64) - HU.MU).astype(np.float32)
        assert np.array_equal(feed.view(np.int32), want.view(np.int32)), (out, (h, w, c), "feed")
        if (h, w) == (H, W):
            assert np.array_equal(proc, np.repeat(im.reshape(h, w, -1), 3 // im.reshape(h, w, -1).shape[2], 2)), (out, (h, w, c), "identity")
            n_id += 1
    assert n_id == (2 if out != (32, 32) else 0)


def _beside(n, group, pos_shift):
    """Index groups of `group` samples out of n, rotated by pos_shift, and where in each the neighbour goes."""
    idx = list(range(n))
    idx = idx[pos_shift * 3:] + idx[:pos_shift * 3]
    for g, s in enumerate(range(0, n, group)):
        part = idx[s: s + group]
        yield part, (g + 3 * pos_shift) % (len(part) + 1)


@pytest.mark.parametrize("out", R.OUTS)
def test_prep_tile_invariance(out):
    """Each sample alone, and at three batch positions beside a colour neighbour that forces the smallest tile on the whole launch
    ((50, 900): {1, 1} at (23, 41)), and beside a (96, 96) one ({4, 32}): proc_im and feed are bit-identical every time."""
    H, W = out
    ims, alone = _prep_images(out), _prep_alone(out)
    flip = out == (41, 23)
    for nb in ((900, 50) if flip else (50, 900), (96, 96)):
        nim = R.image(nb[0], nb[1], 3, seed=1)
        for shift in range(3):
            for part, at in _beside(len(ims), 7, shift):
                batch = [ims[i] for i in part]
                batch.insert(at, nim)
                feed, proc = EV.prepare_images(batch, H, W)
                proc, feed = proc.cpu().numpy(), feed.cpu().numpy()
                for j, i in enumerate(part):
                    k = j + (j >= at)
                    assert np.array_equal(proc[k], alone[i][0]), (out, nb, R.prep_cases(out)[i], "proc_im at position %d of %d" % (k, len(batch)))
                    assert np.array_equal(feed[k].view(np.int32), alone[i][1].view(np.int32)), (out, nb, R.prep_cases(out)[i], "feed")


def test_prep_full_batch_loops_over_tiles():
    """32 samples, one of them the (50, 900) colour source: tile {1, 1}, 943 tiles over 64 workgroups per sample, so the grid-stride
    tile loop runs 15 times with its barriers.  Every sample equals its result alone."""
    out = (23, 41)
    ims, alone = _prep_images(out), _prep_alone(out)
    idx = [i for i, (h, w, c) in enumerate(R.prep_cases(out)) if (h, w, c) != (50, 900, 3)][:31]
    idx.insert(17, R.prep_cases(out).index((50, 900, 3)))
    assert len(idx) == EV.MAX_BATCH == 32
    assert R.tile_choice("prep", [(h, w, c or 1) for h, w, c in (R.prep_cases(out)[i] for i in idx)], *out) == (1, 1)
    feed, proc = EV.prepare_images([ims[i] for i in idx], *out)
    proc, feed = proc.cpu().numpy(), feed.cpu().numpy()
    for k, i in enumerate(idx):
        assert np.array_equal(proc[k], alone[i][0]) and np.array_equal(feed[k].view(np.int32), alone[i][1].view(np.int32)), R.prep_cases(out)[i]


# ---- cmpc_train_prep: targets ---------------------------------------------------------------------------------------------------------
def _target_ref(out, order):
    return [ref if order == 1 else R.nearest_pad(m, *out) for m, _, ref in R.target_cases(out)]


@functools.lru_cache(maxsize=None)
def _targets_alone(out, order):
    res = [FD.prepare_targets([m], None, out[0], out[1], order=order) for m, _, _ in R.target_cases(out)]
    return [(t[0, :, :, 0].cpu().numpy(), int(p[0])) for t, p in res]


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("out", R.OUTS)
def test_targets_against_dense(out, order):
    """target_fine and pos of every mask prepared alone (its own tile) equal dense_pad(mask) > 0 (order 1) and the order-0 rule."""
    cases, refs = R.target_cases(out), _target_ref(out, order)
    assert sum(0 < int(r.sum()) < r.size for r in refs) > len(refs) // 3
    for (m, name, _), ref, (tgt, pos) in zip(cases, refs, _targets_alone(out, order)):
        assert tgt.dtype == np.float32 and set(np.unique(tgt)) <= {0.0, 1.0}
        diff = int((tgt != ref).sum())
        print("out %s order %d %s tile %s: %d differing pixels, pos %d (reference %d)"
              % (out, order, name, R.tile_choice("target", [m.shape + (1,)], out[0], out[1], order), diff, pos, int(ref.sum())))
        assert diff == 0, (out, order, name, diff)
        assert pos == int(ref.sum()), (out, order, name)


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("out", R.OUTS)
def test_targets_tile_invariance(out, order):
    """The targets beside a plain-mask neighbour that forces a narrow tile -- (720, 1280): {1, 4}; (50, 900): {1, 8} at (23, 41) -- at
    three batch positions each: bit-identical to the targets prepared alone."""
    H, W = out
    cases, alone = R.target_cases(out), _targets_alone(out, order)
    flip = out == (41, 23)
    nbs = [(900, 50) if flip else (50, 900)] + ([] if out == (32, 32) else [R.BIG[::-1] if flip else R.BIG])
    for nb in nbs:
        nm = R.mask(nb[0], nb[1], "interior")
        for shift in range(3):
            for part, at in _beside(len(cases), 15, shift):
                batch = [cases[i][0] for i in part]
                batch.insert(at, nm)
                tgt, pos = FD.prepare_targets(batch, None, H, W, order=order)
                tgt, pos = tgt.cpu().numpy()[..., 0], pos.cpu().numpy()
                for j, i in enumerate(part):
                    k = j + (j >= at)
                    assert np.array_equal(tgt[k], alone[i][0]) and int(pos[k]) == alone[i][1], (out, order, nb, cases[i][1], k)


def _colour(rng, m, channels):
    """A colour-coded annotation [h, w, channels] whose object under match = 3 is exactly m and under match = 1 is m | red: `red`
    pixels carry the key's R alone, other pixels the key's G and B but never its R."""
    h, w = m.shape
    a = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    a[..., 0][a[..., 0] == KEY[0]] = KEY[0] ^ 1
    gb = rng.random((h, w)) < 0.3
    a[gb, 1], a[gb, 2] = KEY[1], KEY[2]
    red = (rng.random((h, w)) < 0.03) & ~m
    a[red, 0] = KEY[0]
    a[red, 1] = KEY[1] ^ 0x40
    a[m, :3] = KEY
    return a, red


@pytest.mark.parametrize("order", [1, 0])
def test_colour_coded_annotations(order):
    """3 and 4 channels, match 1 and 3, odd widths: with 3 channels a row starts at every byte phase of object_bits4's 32-bit loads.
    The object is cut out here with plain NumPy comparisons, then resampled by the dense reference."""
    out = (23, 41)
    rng = np.random.default_rng(11)
    sizes = [(5, 3), (7, 1), (1, 7), (23, 41), (37, 61), (12, 21), (46, 83), (9, 5), (40, 701), (160, 161)]
    phases = set()
    for match in (1, 3):
        anns, refs = [], []
        for i, (h, w) in enumerate(sizes):
            m = R.mask(h, w, ("interior", "c11", "c00", "col")[i % 4])
            if h * w > 60:
                m |= R.mask(h, w, "noise") & (rng.random((h, w)) < 0.2)
            a, red = _colour(rng, m, 3 + i % 2)
            obj = np.all(a[..., :match] == np.array(KEY[:match], np.uint8), axis=2)
            assert np.array_equal(obj, m | red if match == 1 else m)
            anns.append(a)
            refs.append(R.dense_pad(obj, *out) > 0 if order == 1 else R.nearest_pad(obj, *out))
            if a.shape[2] == 3:
                phases |= {(y * w * 3) % 4 for y in range(h)}
        assert any(0 < int(r.sum()) < r.size for r in refs)
        tgt, pos = FD.prepare_targets(anns, [KEY] * len(anns), out[0], out[1], order=order, match=match)
        tgt, pos = tgt.cpu().numpy()[..., 0], pos.cpu().numpy()
        for (h, w), a, ref, t, p in zip(sizes, anns, refs, tgt, pos):
            assert np.array_equal(t, ref), (order, match, a.shape, int((t != ref).sum()))
            assert int(p) == int(ref.sum())
            t1, p1 = FD.prepare_targets([a], [KEY], out[0], out[1], order=order, match=match)
            assert np.array_equal(t1.cpu().numpy()[0, :, :, 0], t) and int(p1[0]) == int(p), (order, match, a.shape, "alone")
    assert phases == {0, 1, 2, 3}


@pytest.mark.parametrize("kind", ["plain", "colour"])
def test_annotation_tail_word(kind):
    """cmpc_train_prep alone (no image half) on an annotation whose packed length is no multiple of 4, inside a larger allocation whose
    bytes just past the end would read as object.  The width is a multiple of 4 and the annotation starts at byte 1, so the four-pixel
    group that ends the last row spills into the final, partial 32-bit word, which ld_word must assemble from the bytes that belong
    to the annotation.  Once the last pixels are background (the target must not see what lies behind them), once the very last
    pixel is the object (its last byte comes out of that word)."""
    H, W = 23, 41
    h, w, c = (3, 8, 1) if kind == "plain" else (3, 4, 3)
    n = 1 + h * w * c
    assert n % 4 == 1 and w % 4 == 0
    for last in (False, True):
        m = np.zeros((h, w), bool)
        m[0, 1] = True
        m[h - 1, w - 1] = last
        if kind == "plain":
            a, fill, k, ck, match = m.astype(np.uint8), [255], (0, 0, 0), L.ANN_PLAIN, 1
        else:
            a = np.full((h, w, 3), 7, np.uint8)
            a[m] = KEY
            fill, k, ck, match = list(KEY), KEY, L.ANN_COLOR, 3
        host = np.resize(np.array(fill, np.uint8), n + 63)        # byte 0 and everything behind the annotation would be the object
        host[1:n] = a.reshape(-1)
        buf = torch.from_numpy(host).cuda()
        assert buf.data_ptr() % 4 == 0
        d, _ = FD.plan_targets([a.shape], [ck], [k], H, W, match=match)
        d[0].offset = 1
        for order in (1, 0):
            tgt = torch.full((1, H, W, 1), -1.0, device="cuda")
            pos = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            L.call("cmpc_train_prep", None, 0, None, buf.data_ptr(), n, d, 1, H, W, order, None, None, tgt.data_ptr(), pos.data_ptr(), _stream())
            ref = R.dense_pad(m, H, W) > 0 if order == 1 else R.nearest_pad(m, H, W)
            assert 0 < int(ref.sum()) < ref.size
            assert np.array_equal(tgt.cpu().numpy()[0, :, :, 0], ref), (kind, last, order)
            assert int(pos[0]) == int(ref.sum())


# ---- cmpc_clip_prep -------------------------------------------------------------------------------------------------------------------
def test_clip_prep_narrow_tile():
    """(40, 700) frames and annotation at (23, 41): eval_prep_kernel runs at {1, 4}.  Bit-equal to cmpc_eval_prep plus cmpc_train_prep."""
    H, W = 23, 41
    frames = [R.image(40, 700, 3, seed=s) for s in range(5)]
    ann = np.zeros((40, 700), bool)
    ann[8:30, 150:420] = True
    assert R.tile_choice("prep", [(40, 700, 3)] * 5, H, W) == (1, 4)
    for order in (1, 0):
        f, t, p = FD.prepare_clip(frames, ann, None, H, W, order=order)
        f2, _ = EV.prepare_images(frames, H, W)
        t2, p2 = FD.prepare_targets([ann], None, H, W, order=order)
        assert torch.equal(_bits(f), _bits(f2)) and torch.equal(t, t2) and torch.equal(p, p2)
        assert 0 < int(p[0]) < H * W


# ---- cmpc_eval_mask_iu / cmpc_eval_mask_out -------------------------------------------------------------------------------------------
def _score_map(rng, m, dtype):
    """(map, threshold) whose binarisation is exactly m: float32 scores either side of 1e-9, or uint8 {0, 1} against 0.5."""
    if dtype == "u8":
        return m.astype(np.uint8), 0.5
    th = np.float32(1e-9)
    s = np.where(m, rng.uniform(1e-9, 1.0, m.shape), rng.uniform(-1.0, 1e-9, m.shape)).astype(np.float32)
    s[m & (s < th)] = th
    s[~m & (s >= th)] = -th
    assert np.array_equal(s >= th, m)
    return s, 1e-9


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("shape", R.MAPS)
def test_masks_and_iu_against_dense(shape, dtype):
    """I, U and the masks of mask_iu(want_masks=True), and masks_out with both values, equal dense_crop(binarised) > 0 against random
    ground truth; 72 samples per map shape in batches of 32, 32 and 8, kinds and sizes mixed."""
    rng = np.random.default_rng(5)
    cases = R.crop_cases(shape)
    cases = [cases[i] for i in rng.permutation(len(cases))]
    for s0 in range(0, len(cases), EV.MAX_BATCH):
        part = cases[s0: s0 + EV.MAX_BATCH]
        maps, th = zip(*[_score_map(rng, R.binary_map(shape[0], shape[1], kind), dtype) for kind, _, _ in part])
        md = torch.from_numpy(np.stack(maps)).cuda()
        sizes = [size for _, size, _ in part]
        gts = [rng.random(size) < 0.4 for size in sizes]
        iu, masks = EV.mask_iu(md, gts, th[0], want_masks=True)
        iu = iu.cpu().numpy()
        b1, d1 = EV.masks_out(md, sizes, th[0], value=1)
        b255, d255 = EV.masks_out(md, sizes, th[0], value=255)
        for b, ((kind, size, ref), gt) in enumerate(zip(part, gts)):
            got = masks[b].cpu().numpy()
            assert got.shape == size and np.array_equal(got, ref.astype(np.uint8)), (shape, dtype, kind, size, int((got != ref).sum()))
            assert (int(iu[b, 0]), int(iu[b, 1])) == (int((ref & gt).sum()), int((ref | gt).sum())), (shape, dtype, kind, size)
            assert np.array_equal(EV.unpack_masks(b1, d1)[b].cpu().numpy(), ref.astype(np.uint8)), (shape, dtype, kind, size, "mask_out 1")
            assert np.array_equal(EV.unpack_masks(b255, d255)[b].cpu().numpy(), ref.astype(np.uint8) * 255), (shape, dtype, kind, size, "mask_out 255")


def test_mask_threshold_special_values():
    """score >= threshold on the float32 itself: the threshold is foreground, the float below it background, NaN and -inf background,
    +inf foreground, and -0.0 is foreground at threshold 0 while the smallest negative number is not.  The pixels sit in the
    middle columns, which every target size keeps."""
    h, w = 24, 40
    th = np.float32(0.5)
    a = np.full((h, w), -1.0, np.float32)
    want_a = np.zeros((h, w), bool)
    for (y, x), v, f in (((2, 13), th, True), ((2, 22), np.nextafter(th, np.float32(0)), False), ((10, 15), np.float32("nan"), False),
                         ((10, 26), np.float32("inf"), True), ((20, 14), np.float32("-inf"), False), ((20, 24), np.nextafter(th, np.float32(1)), True)):
        a[y, x], want_a[y, x] = v, f
    z = np.full((h, w), -1.0, np.float32)
    want_z = np.zeros((h, w), bool)
    for (y, x), v, f in (((3, 13), np.float32(-0.0), True), ((3, 26), np.float32(0.0), True), ((15, 20), -np.float32(1e-45), False),
                         ((21, 21), np.float32("nan"), False)):
        z[y, x], want_z[y, x] = v, f
    sizes = [(24, 40), (37, 61), (5, 7), (200, 150)]
    for m, t, want in ((a, 0.5, want_a), (z, 0.0, want_z)):
        with np.errstate(invalid="ignore"):
            assert np.array_equal(m >= np.float32(t), want)
        md = torch.from_numpy(np.stack([m] * len(sizes))).cuda()
        gts = [np.ones(s, bool) for s in sizes]
        iu, masks = EV.mask_iu(md, gts, t, want_masks=True)
        buf, d = EV.masks_out(md, sizes, t, value=255)
        for b, s in enumerate(sizes):
            ref = R.dense_crop(want, *s) > 0
            assert 0 < int(ref.sum()) < ref.size
            assert np.array_equal(masks[b].cpu().numpy(), ref.astype(np.uint8)), (t, s)
            assert np.array_equal(EV.unpack_masks(buf, d)[b].cpu().numpy(), ref.astype(np.uint8) * 255), (t, s)
            assert (int(iu[b, 0]), int(iu[b, 1])) == (int(ref.sum()), ref.size)


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_mask_iu_unaligned_descriptors(dtype):
    """cmpc_eval_mask_iu called directly with hand-made descriptors: offsets at every byte phase and sizes with h * w % 4 in {0, 1, 2, 3}
    (the byte-wise path and the tail of the four-pixel loop).  Ground-truth bytes between the masks are all foreground, so a read past
    a mask shows in I and U; predicted-mask bytes between and behind the masks keep the guard pattern."""
    shape = (24, 40)
    rng = np.random.default_rng(9)
    sizes = [(5, 7), (1, 9), (3, 250), (37, 61), (2, 90), (1, 1), (7, 5), (9, 1), (24, 40), (61, 37), (2, 2), (200, 150)]
    assert {s[0] * s[1] % 4 for s in sizes} == {0, 1, 2, 3}
    d, _ = EV.plan_masks(sizes, *shape)
    off = 0
    for b, di in enumerate(d):
        off += 5 + (b + 1 - off - 5) % 4                              # at least 5 guard bytes, then phase (b + 1) % 4
        di.offset = off
        off += di.h * di.w
    assert {di.offset % 4 for di in d} == {0, 1, 2, 3}
    nbytes = off + 7
    kinds = [R.MAP_KINDS[b % 5] for b in range(len(sizes))]
    maps, th = zip(*[_score_map(rng, R.binary_map(shape[0], shape[1], k), dtype) for k in kinds])
    md = torch.from_numpy(np.stack(maps)).cuda()
    gt_host = np.full(nbytes, 255, np.uint8)
    gts = [rng.random(s) < 0.4 for s in sizes]
    for di, g in zip(d, gts):
        gt_host[di.offset: di.offset + g.size] = g.reshape(-1)
    gt = torch.from_numpy(gt_host).cuda()
    mo = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    iu = torch.full((len(sizes), 2), -1, dtype=torch.int64, device="cuda")
    assert gt.data_ptr() % 4 == 0 and mo.data_ptr() % 4 == 0
    L.call("cmpc_eval_mask_iu", md.data_ptr(), L.EVAL_F32 if dtype == "f32" else L.EVAL_U8, len(sizes), shape[0], shape[1], float(th[0]),
           gt.data_ptr(), nbytes, d, iu.data_ptr(), mo.data_ptr(), _stream())
    host, iu = mo.cpu().numpy(), iu.cpu().numpy()
    inside = np.zeros(host.shape, bool)
    for b, (di, s, k, g) in enumerate(zip(d, sizes, kinds, gts)):
        ref = R.dense_crop(R.binary_map(shape[0], shape[1], k), *s) > 0
        got = host[di.offset: di.offset + g.size].reshape(s)
        assert np.array_equal(got, ref.astype(np.uint8)), (dtype, s, k, di.offset % 4)
        assert (int(iu[b, 0]), int(iu[b, 1])) == (int((ref & g).sum()), int((ref | g).sum())), (dtype, s, k, di.offset % 4)
        inside[di.offset: di.offset + g.size] = True
    assert np.all(host[~inside] == GUARD)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src, why, message", [(s, w, {"radius": "Gaussian radius > 63", "lds": "source footprint does not fit in LDS",
                                                        "empty": r"geometry \(0, 41, "}[w]) for s, w in R.REFUSALS],
                         ids=[w for _, w in R.REFUSALS])
def test_refusals_leave_the_outputs_alone(src, why, message):
    """Radius above MAXR, a colour source whose footprint fits no tile (radii 61 / 60, inside MAXR), a resized side of 0: each is
    refused by cmpc_eval_prep with its message before anything is launched -- the outputs keep their fill -- whether the sample is
    alone or rides behind a valid one, and a valid call directly afterwards is correct."""
    H, W = 23, 41
    bad = R.image(*src)
    good = R.image(5, 3, 3)
    with pytest.raises(L.CmpcError, match=message):          # the Python wrapper has no check of its own: the library refuses
        EV.prepare_images([bad], H, W)
    for batch in ([bad], [good, bad]):
        d, nbytes = EV.plan_prep([a.shape for a in batch], H, W)
        host = np.zeros(nbytes, np.uint8)
        for di, a in zip(d, batch):
            host[di.offset: di.offset + a.size] = a.reshape(-1)
        srcd = torch.from_numpy(host).cuda()
        proc = torch.full((len(batch), H, W, 3), GUARD, dtype=torch.uint8, device="cuda")
        feed = torch.full((len(batch), H, W, 3), -7.0, device="cuda")
        with pytest.raises(L.CmpcError, match=message):
            L.call("cmpc_eval_prep", srcd.data_ptr(), nbytes, d, len(batch), H, W, proc.data_ptr(), feed.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert bool((proc == GUARD).all()) and bool((feed == -7.0).all())
    if why == "radius":                                        # the target half refuses the same geometry, before its memset
        with pytest.raises(L.CmpcError, match=message):
            FD.prepare_targets([R.mask(src[0], src[1], "interior")], None, H, W)
    feed, proc = EV.prepare_images([good], H, W)
    i = R.prep_cases((23, 41)).index((5, 3, 3))
    assert np.array_equal(proc[0].cpu().numpy(), _prep_alone((23, 41))[i][0])
    assert np.abs(proc[0].cpu().numpy().astype(np.float64) - 255.0 * R.dense_pad(good, H, W)).max() <= 0.5 + MARGIN


def test_grey_source_fits_where_colour_is_refused():
    """The (720, 1280) source the colour refusal is tested with goes through as a grey image (tile {1, 8}), radii 61 / 60."""
    assert R.tile_choice("prep", [R.BIG + (1,)], 23, 41) == (1, 8)
    im = R.image(720, 1280, 0)
    _, proc = EV.prepare_images([im], 23, 41)
    assert np.abs(proc[0, :, :, 0].cpu().numpy().astype(np.float64) - 255.0 * R.dense_pad(im, 23, 41)).max() <= 0.5 + MARGIN
