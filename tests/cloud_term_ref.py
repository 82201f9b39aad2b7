"""NumPy restatement of the pointwise conv with a per-cloud term (include/amc3d.h, amc3d_pointwise_conv_cloud_term_forward and
amc3d_cloud_term_grad), in fp64:

    y[b,co,p]  = sum_ci w[co,ci] x[b,ci,p] + c[b,co]
    dc[b,co]   = sum_p dy[b,co,p]
    dx[b,ci,p] = sum_co w[co,ci] dy[b,co,p]
    dw[co,ci]  = sum_{b,p} dy[b,co,p] x[b,ci,p]

and the magnitudes the error bounds of tests/test_gpu_cloud_term.py are stated in."""
import numpy as np


def forward(x, w, c):
    x, w, c = (np.asarray(a, dtype=np.float64) for a in (x, w, c))
    return np.einsum("oi,bip->bop", w, x) + c[:, :, None]


def forward_magnitude(x, w, c):
    """sum_ci |w||x| + |c| per output element"""
    x, w, c = (np.abs(np.asarray(a, dtype=np.float64)) for a in (x, w, c))
    return np.einsum("oi,bip->bop", w, x) + c[:, :, None]


def backward(x, w, dy):
    """-> dc (B,Cout), dx (B,Cin,P), dw (Cout,Cin)"""
    x, w, dy = (np.asarray(a, dtype=np.float64) for a in (x, w, dy))
    return dy.sum(-1), np.einsum("oi,bop->bip", w, dy), np.einsum("bop,bip->oi", dy, x)


def backward_magnitudes(x, w, dy):
    """the same three sums over absolute values"""
    return backward(np.abs(x), np.abs(w), np.abs(dy))
