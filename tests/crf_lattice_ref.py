"""Float64 restatement of DenseCRF with both pairwise terms filtered through a permutohedral lattice -- what
`cmpc_dense_crf_lattice` (cmpc-refseg_amd/csrc/ops_crf_lattice.hip) computes, small and readable, for the tests to compare with.

    A. Adams, J. Baek, M. A. Davis, "Fast High-Dimensional Filtering Using the Permutohedral Lattice", Eurographics 2010.
    P. Kraehenbuehl, V. Koltun, "Efficient Inference in Fully Connected CRFs with Gaussian Edge Potentials", NIPS 2011.

The embedding (elevation, remainder-0 point, ranks, barycentric weights) is evaluated in float32 with the kernel's operation order, so
that the discrete decisions -- which simplex a feature lies in, how rank ties break -- are the kernel's own; the vertices form a dict keyed
by the key tuple and are numbered in order of first appearance (pixel * (d+1) + r), as on the GPU.  Splat, blur, slice and the
mean-field recursion are float64.  Parity against pydensecrf itself is UNPINNED (the library is not installed)."""
import numpy as np

from oracle.dense_crf_numpy import _softmax0, unary_from_sigmoid


def scale_factors(d):
    """Per-axis scale of the elevation, sqrt(2/3) (d+1) / sqrt((i+1)(i+2)) (Adams et al. 2010, p. 5-6), rounded to float32."""
    i = np.arange(d, dtype=np.float64)
    return (np.sqrt(2.0 / 3.0) * (d + 1) / np.sqrt((i + 1) * (i + 2))).astype(np.float32)


def features(H, W, rgb, sxy, srgb=None):
    """float32 features [N, d]: (x, y) / sxy, and (r, g, b) / srgb for the bilateral term; x / s is x * float32(1 / s)."""
    ys, xs = np.mgrid[0:H, 0:W]
    inv = np.float32(1.0 / sxy)
    f = [xs.reshape(-1).astype(np.float32) * inv, ys.reshape(-1).astype(np.float32) * inv]
    if srgb is not None:
        ic = np.float32(1.0 / srgb)
        col = np.asarray(rgb).reshape(-1, 3).astype(np.float32)
        f += [col[:, c] * ic for c in range(3)]
    return np.stack(f, 1)


def embed(f):
    """f [N, d] float32 -> keys [N, d+1, d] int64 (the d+1 enclosing vertices, first d coordinates) and weights [N, d+1] float32."""
    N, d = f.shape
    one = np.float32(1)
    down = np.float32(1.0 / (d + 1))
    cf = f * scale_factors(d)
    el = np.empty((N, d + 1), np.float32)                       # elevate onto the hyperplane sum(x) = 0
    sm = np.zeros(N, np.float32)
    for j in range(d, 0, -1):
        el[:, j] = sm - np.float32(j) * cf[:, j - 1]
        sm = sm + cf[:, j - 1]
    el[:, 0] = sm
    rd = np.rint(el * down)                                     # nearest remainder-0 point (coordinates multiple of d+1)
    rem0 = rd.astype(np.int64) * (d + 1)
    tot = rd.astype(np.int64).sum(1)
    di = el - rem0.astype(np.float32)
    rank = np.zeros((N, d + 1), np.int64)                       # position of each coordinate of el - rem0 in descending order
    for i in range(d):
        for j in range(i + 1, d + 1):
            lt = di[:, i] < di[:, j]
            rank[:, i] += lt
            rank[:, j] += ~lt
    rank += tot[:, None]                                        # back onto the hyperplane when sum(rem0) != 0
    lo, hi = rank < 0, rank > d
    rank[lo] += d + 1; rem0[lo] += d + 1
    rank[hi] -= d + 1; rem0[hi] -= d + 1
    bary = np.zeros((N, d + 2), np.float32)                     # barycentric weights (Adams et al. 2010, p. 10)
    rows = np.arange(N)
    for i in range(d + 1):
        v = (el[:, i] - rem0[:, i].astype(np.float32)) * down
        bary[rows, d - rank[:, i]] += v
        bary[rows, d - rank[:, i] + 1] -= v
    bary[:, 0] += one + bary[:, d + 1]
    r = np.arange(d + 1)
    canon = np.where(rank[:, None, :d] <= d - r[None, :, None], r[None, :, None], r[None, :, None] - (d + 1))   # [N, r, i]
    keys = rem0[:, None, :d] + canon
    return keys, bary[:, : d + 1]


class Lattice:
    """The lattice of one feature set: slice table (off, w), blur neighbours nb [d+1, M, 2] (M = absent -> a zero row)."""

    def __init__(self, f, fast=False):
        N, d = f.shape
        keys, w = embed(f)
        self.d, self.N = d, N
        self.w = w.astype(np.float64)
        self.alpha = 1.0 / (1.0 + 2.0 ** -d)
        if fast:
            self._number_sorted(keys)
            return
        index = {}
        off = np.empty((N, d + 1), np.int64)
        for p in range(N):
            for r in range(d + 1):
                off[p, r] = index.setdefault(tuple(keys[p, r]), len(index))
        self.M, self.off = len(index), off
        vk = np.array(list(index.keys()), np.int64).reshape(self.M, d)
        nb = np.full((d + 1, self.M, 2), self.M, np.int64)
        for j in range(d + 1):
            step = np.full(d, -1, np.int64)                     # the direction j offset: +d on axis j, -1 on the others
            if j < d:
                step[j] = d
            for m in range(self.M):
                nb[j, m, 0] = index.get(tuple(vk[m] + step), self.M)
                nb[j, m, 1] = index.get(tuple(vk[m] - step), self.M)
        self.nb = nb

    def _number_sorted(self, keys):
        """The same M, off and nb without the Python loops, for images of 10^4 pixels and more: np.unique on the keys packed into one
        int64, renumbered by first appearance.  tests/test_crf_refs_host.py pins it to the dict version."""
        N, d = self.N, self.d
        flat = keys.reshape(-1, d)
        lo = flat.min(0)
        span = flat.max(0) - lo + 1
        assert np.prod(span.astype(np.float64)) < 2.0 ** 62, "keys do not pack into an int64"
        stride = np.concatenate([[1], np.cumprod(span[:-1])]).astype(np.int64)

        def pack(k):
            return ((k - lo) * stride).sum(1)

        uniq, first, inv = np.unique(pack(flat), return_index=True, return_inverse=True)
        self.M = M = len(uniq)
        number = np.empty(M, np.int64)
        number[np.argsort(first, kind="stable")] = np.arange(M)     # sorted position -> number in order of first appearance
        self.off = number[inv.reshape(-1)].reshape(N, d + 1)
        vk = np.empty((M, d), np.int64)
        vk[number] = flat[first]
        nb = np.full((d + 1, M, 2), M, np.int64)
        for j in range(d + 1):
            step = np.full(d, -1, np.int64)
            if j < d:
                step[j] = d
            for side, k in enumerate((vk + step, vk - step)):
                inside = ((k >= lo) & (k < lo + span)).all(1)       # outside the box of the keys: no such vertex (and no valid packing)
                pk = pack(np.where(inside[:, None], k, lo))
                pos = np.minimum(np.searchsorted(uniq, pk), M - 1)
                nb[j, :, side] = np.where(inside & (uniq[pos] == pk), number[pos], M)
        self.nb = nb

    def splat(self, v):
        """v [N, C] -> vertex values [M + 1, C] (row M stays zero)."""
        out = np.zeros((self.M + 1, v.shape[1]))
        np.add.at(out, self.off.reshape(-1), (self.w[:, :, None] * v[:, None, :]).reshape(-1, v.shape[1]))
        return out

    def blur(self, val, order=None):
        for j in (range(self.d + 1) if order is None else order):
            new = val.copy()                                    # v' = v + (v_n1 + v_n2) / 2 along direction j; row M stays zero
            new[: self.M] = val[: self.M] + 0.5 * (val[self.nb[j, :, 0]] + val[self.nb[j, :, 1]])
            val = new
        return val

    def slice(self, val):
        return self.alpha * (self.w[:, :, None] * val[self.off]).sum(1)

    def apply(self, v, order=None):
        """L v for v [N, C]: splat, blur along each of the d+1 directions, slice scaled by alpha = 1 / (1 + 2^-d)."""
        return self.slice(self.blur(self.splat(v), order))


def lattices(sigm_shape, rgb, sxy_g=3.0, sxy_b=20.0, srgb=3.0, fast=False):
    H, W = sigm_shape
    return Lattice(features(H, W, None, sxy_g), fast), Lattice(features(H, W, rgb, sxy_b, srgb), fast)


def dense_crf(sigm, rgb, sxy_g=3.0, compat_g=3.0, sxy_b=20.0, srgb=3.0, compat_b=10.0, iters=5, lats=None):
    """oracle.dense_crf_numpy.dense_crf with K Q replaced by the lattice filter L Q: Q [2, H, W] float64.  `lats`: the pair that
    `lattices` returns for these parameters, when the caller has built it already."""
    sigm = np.asarray(sigm, dtype=np.float64)
    H, W = sigm.shape
    U = unary_from_sigmoid(sigm)
    Q = _softmax0(-U)
    if iters == 0:
        return Q.reshape(2, H, W)
    terms = []
    for w, lat in zip((compat_g, compat_b), lats if lats is not None else lattices((H, W), rgb, sxy_g, sxy_b, srgb)):
        nrm = 1.0 / np.sqrt(lat.apply(np.ones((H * W, 1)))[:, 0] + 1e-20)      # symmetric normalisation, K 1 through the same lattice
        terms.append((w, lat, nrm))
    for _ in range(iters):
        e = -U
        for w, lat, nrm in terms:
            e = e + w * (nrm[None, :] * lat.apply((Q * nrm[None, :]).T).T)
        Q = _softmax0(e)
    return Q.reshape(2, H, W)
