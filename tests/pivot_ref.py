"""NumPy float64 restatements of what the pivot-frame step computes: cmpc_mask_pool's weighted sums (the stored values read and
upcast), cmpc_level_agree's counts and hostutil.find_pivot_frames' selection.  Written apart from the package's code; the tests compare
the two."""
import numpy as np


def weights(score, h, w, mode, thresh):
    """wgt[i, y, x]: the point sample score[i, y * (sH / h), x * (sW / w)] (soft), or that float32 >= float32(thresh) ? 1 : 0 (hard)."""
    score = np.asarray(score)
    assert score.dtype == np.float32 and score.ndim == 3
    sH, sW = score.shape[1:]
    assert sH % h == 0 and sW % w == 0
    s = score[:, ::sH // h, ::sW // w]
    assert s.shape[1:] == (h, w)
    if mode == "hard":
        return (s >= np.float32(thresh)).astype(np.float64)
    assert mode == "soft"
    return s.astype(np.float64)


def pool(feat, score, mode="soft", thresh=0.5):
    """feat [n, h, w, C] (any float type: its stored values), score float32 [n, sH, sW] ->
    (desc [n, C], area [n], sum |wgt * feat| [n, C], sum |wgt| [n]) in float64."""
    x = np.asarray(feat).astype(np.float64)
    n, h, w, C = x.shape
    wg = weights(score, h, w, mode, thresh)
    desc = np.einsum("nyx,nyxc->nc", wg, x)
    mag = np.einsum("nyx,nyxc->nc", np.abs(wg), np.abs(x))
    return desc, wg.sum((1, 2)), mag, np.abs(wg).sum((1, 2))


def bound(h, w, mag):
    """|float32 result - exact| <= (N + 1) 2^-24 sum |wgt * x| for N = h * w products and their sum in any order: a term passes through
    at most N roundings (its product and at most N - 1 additions, whatever the summation tree), each relative u = 2^-24, so the error is
    at most ((1 + u)^N - 1) sum |wgt * x| <= (N u + N^2 u^2) sum |wgt * x|, and N^2 u <= 1 up to N = 4096."""
    return (h * w + 1) * 2.0 ** -24 * mag


def agree(a, b, logit):
    """int64 [n, 2]: the sizes of (a > t) & (b > t) and (a > t) | (b > t) with t = float32(logit)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
    t = np.float32(logit)
    x, y = (a > t).reshape(a.shape[0], -1), (b > t).reshape(a.shape[0], -1)
    return np.stack([(x & y).sum(1), (x | y).sum(1)], 1).astype(np.int64)


def find_pivot_frames(descriptors, num_propagate=2, nearest_first=False):
    """The selection, loop by loop: cosine similarities of the float64 rows (a zero row is similar to nothing), the frame with the
    largest column sum, the frames ordered by their similarity to it (ties by index), each taken unless a taken frame lies within
    num_propagate of it."""
    d = np.asarray(descriptors, dtype=np.float64)
    F = d.shape[0]
    unit = np.zeros_like(d)
    for i in range(F):
        # The norm is formed as numpy.linalg.norm(axis=1) forms it, i.e. as the code under test does: a last-bit difference in a norm
        # decides exact ties (with F = 2 both column sums are 1 + s).  So how TIES fall is not checked independently by this
        # restatement; the hand-worked cases and the two properties in tests/test_pivot_host.py are independent of it.
        nrm = np.sqrt(np.sum(d[i] * d[i]))
        if nrm > 0:
            unit[i] = d[i] / nrm
    S = np.dot(unit, unit.T)
    total = np.sum(S, axis=0)
    first = 0
    for i in range(F):
        if total[i] > total[first]:
            first = i
    sim = [S[first][i] for i in range(F)]
    order = sorted(range(F), key=(lambda i: (-sim[i], i)) if nearest_first else (lambda i: (sim[i], i)))
    taken = []
    for f in order:
        if all(abs(f - t) > num_propagate for t in taken):
            taken.append(f)
    return taken
