"""Dense CRF post-processing of the reference's evaluation script (test.py:309-322, the `-c` / dcrf option): pydensecrf's
`DenseCRF2D(W, H, 2)` with the unary energies of the sigmoid map, a Gaussian and a bilateral Potts term and 5 mean-field iterations.

    Q = dense_crf(sigm, proc_im)                     # [2, H, W]; np.argmax(Q, 0) is the refined mask
    mask = dense_crf_mask(sigm, proc_im)             # [H, W] uint8 in {0, 1}

Runs on the GPU through `cmpc_dense_crf` (csrc/ops_crf.hip): the Gaussian kernels are evaluated exactly in a 4-sigma window where the
library filters through a permutohedral lattice, so masks can differ from pydensecrf's at object borders (parity-unpinned: pydensecrf
is a third-party dependency outside the reference tree and is not installed here).  `oracle/dense_crf_numpy.py` is the brute-force
CPU restatement the tests compare with.

method="lattice" filters both pairwise terms through a permutohedral lattice instead, as pydensecrf does (`cmpc_dense_crf_lattice`,
csrc/ops_crf_lattice.hip; tests/crf_lattice_ref.py restates it in float64): O(N (d+1)) per filter against O(N window), and batched --
`dense_crf_batch` refines B samples of one size in one call.  "exact" stays the default.

    masks = dense_crf_batch(sigm, proc_ims, method="lattice")     # sigm [B, H, W], proc_ims [B, H, W, 3] uint8 -> [B, H, W] uint8
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

DEFAULTS = dict(sxy_g=3.0, compat_g=3.0, sxy_b=20.0, srgb=3.0, compat_b=10.0, iters=5)        # test.py:317-319


METHODS = ("exact", "lattice")


def _as(x, dev, dtype=None):
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
    return t.to(dev, dtype) if dtype is not None else t


def _run(sigm, rgb, want_q, want_mask, device, method="exact", batched=False, **kw):
    if method not in METHODS:
        raise ValueError("method must be one of %s, got %r" % (METHODS, method))
    p = dict(DEFAULTS); p.update(kw)
    dev = torch.device(device)
    s = _as(sigm, dev, torch.float32).contiguous()
    if s.dim() != (3 if batched else 2):
        raise ValueError("sigm must be %s, got %s" % ("[B, H, W]" if batched else "[H, W]", tuple(s.shape)))
    lead = tuple(s.shape[:-2])
    H, W = s.shape[-2:]
    im = _as(rgb, dev)
    if tuple(im.shape) != lead + (H, W, 3):
        raise ValueError("rgb must be %s matching sigm, got %s" % ("[B, H, W, 3]" if batched else "[H, W, 3]", tuple(im.shape)))
    if im.dtype != torch.uint8:
        raise ValueError("rgb must be uint8 (the resized / padded image the reference passes as rgbim)")
    im = im.to(dev).contiguous()
    q = torch.empty(lead + (2, H, W), device=dev, dtype=torch.float32) if want_q else None
    m = torch.empty(lead + (H, W), device=dev, dtype=torch.uint8) if want_mask else None
    pair = (float(p["sxy_g"]), float(p["compat_g"]), float(p["sxy_b"]), float(p["srgb"]), float(p["compat_b"]), int(p["iters"]),
            q.data_ptr() if q is not None else None, m.data_ptr() if m is not None else None)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        if method == "lattice":
            _lib.call("cmpc_dense_crf_lattice", s.data_ptr(), im.data_ptr(), lead[0] if batched else 1, H, W, *pair, st)
        elif batched:                                              # the exact kernel takes one sample per call
            for b in range(lead[0]):
                qb = q[b].data_ptr() if q is not None else None
                mb = m[b].data_ptr() if m is not None else None
                _lib.call("cmpc_dense_crf", s[b].data_ptr(), im[b].data_ptr(), H, W, *pair[:6], qb, mb, st)
        else:
            _lib.call("cmpc_dense_crf", s.data_ptr(), im.data_ptr(), H, W, *pair, st)
    return q, m


def dense_crf(sigm, rgb, device="cuda:0", method="exact", **params) -> torch.Tensor:
    """d.inference(iters) of test.py:309-320: the label marginals Q [2, H, W] (fp32, on `device`)."""
    return _run(sigm, rgb, True, False, device, method, **params)[0]


def dense_crf_mask(sigm, rgb, device="cuda:0", method="exact", **params) -> torch.Tensor:
    """np.argmax(Q, axis=0) of test.py:321: [H, W] uint8 in {0, 1}."""
    return _run(sigm, rgb, False, True, device, method, **params)[1]


def dense_crf_batch(sigm, rgb, device="cuda:0", method="exact", want_q=False, **params):
    """B samples of one size: sigm [B, H, W], rgb [B, H, W, 3] uint8 -> masks [B, H, W] uint8, or (Q [B, 2, H, W], masks) with want_q.
    method="lattice" is one call for the whole batch; "exact" runs the exact kernel once per sample."""
    q, m = _run(sigm, rgb, want_q, True, device, method, batched=True, **params)
    return (q, m) if want_q else m
