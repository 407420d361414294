"""Float64 reference of what `cmpc_dense_crf` (cmpc-refseg_amd/csrc/ops_crf.hip) documents: oracle/dense_crf_numpy.py's mean-field
recursion with each Gaussian kernel truncated to the square window the launcher chooses,

    K_ij <- K_ij * [|x_i - x_j| <= r and |y_i - y_j| <= r],   r = min(max(H, W) - 1, ceil(float32(4) * float32(sxy)))

per term: the Gaussian radius from sxy_g, the bilateral radius from sxy_b.  The oracle sums all N^2 pairs; the difference is the kernel
mass beyond 4 sigma (below e^-8 per pair), small but not zero, and it is a modelling difference, not kernel error -- so the edge tests
of the exact path compare with this file.  `window=False` gives the oracle back.  Dense N^2: small images only."""
import numpy as np

from oracle.dense_crf_numpy import _kernel, _softmax0, unary_from_sigmoid

MAX_RADIUS = 511                                                # the launcher's window table holds radii 0..511


def window_radius(H, W, sxy):
    """The launcher's `min(max(H, W) - 1, (int)ceilf(4.0f * sxy))`, in float32 as there."""
    return min(max(H, W) - 1, int(np.ceil(np.float32(4) * np.float32(sxy))))


def window_mask(H, W, r):
    """[N, N] bool: pixel j lies in the (2r+1)^2 window of pixel i."""
    ys, xs = np.mgrid[0:H, 0:W]
    x, y = xs.reshape(-1), ys.reshape(-1)
    return (np.abs(x[:, None] - x[None, :]) <= r) & (np.abs(y[:, None] - y[None, :]) <= r)


def dense_crf(sigm, rgb, sxy_g=3.0, compat_g=3.0, sxy_b=20.0, srgb=3.0, compat_b=10.0, iters=5, window=True):
    """sigm [H, W], rgb [H, W, 3] uint8 -> Q [2, H, W] float64; the same statements as the oracle's dense_crf, K masked by the window."""
    sigm = np.asarray(sigm, dtype=np.float64)
    H, W = sigm.shape
    ys, xs = np.mgrid[0:H, 0:W]
    pos = np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.float64)
    col = np.asarray(rgb, dtype=np.float64).reshape(-1, 3)
    kernels = []
    for w, feat, sxy in ((compat_g, pos / sxy_g, sxy_g), (compat_b, np.concatenate([pos / sxy_b, col / srgb], 1), sxy_b)):
        K = _kernel(feat)
        if window:
            K = K * window_mask(H, W, window_radius(H, W, sxy))
        nrm = 1.0 / np.sqrt(K.sum(1) + 1e-20)
        kernels.append((w, K, nrm))
    U = unary_from_sigmoid(sigm)
    Q = _softmax0(-U)
    for _ in range(iters):
        e = -U
        for w, K, nrm in kernels:
            e = e + w * (nrm[None, :] * ((Q * nrm[None, :]) @ K.T))
        Q = _softmax0(e)
    return Q.reshape(2, H, W)
