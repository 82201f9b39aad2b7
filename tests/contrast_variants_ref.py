"""Plain-torch restatement of every form of ContrastHead.contrast_softnn_margin (MarginContrast.py:117-174) and of the stage
around it (:250-257), shared by tests/test_contrast_variants_host.py (which pins it to the head's own code at fp64) and
tests/test_gpu_contrast_variants.py (which uses it as the arbiter at fp64 and the yardstick at fp32).  Nothing of the
package's kernels or operators is used here."""
import itertools

import torch

EPS = 1e-8
MARGINS = ("constant", "adaptive", "learned")
DBS = ("-m", "+m", "NONE")
METHODS = ("Method1", "Method2")
TEMPERATURES = (None, 0.3, 0.07)
FORMS = tuple(itertools.product(MARGINS, DBS, METHODS, TEMPERATURES))      # 54
DEFAULT_FORM = ("adaptive", "-m", "Method1", 0.3)                          # the shipped configuration
MU, NU = -1.0, 0.5


def form_id(form):
    return "{}/{}/{}/{}".format(*form)


def form_loss(sim, posmask, a, form, mu=MU, nu=NU):
    """per-anchor loss (n) of one form from the cosines sim (n,k), the mask (n,k) bool and the ambiguities a (n), at sim's
    dtype: the margin, the shift of the positives (-m) or the negatives (+m), the optional temperature, then Method1
    -log(P / (P + N) + 1e-12) or Method2 -log(sum_j (e_j pos_j / (e_j pos_j + N) + 1e-12) / (npos + 1e-12)), j over all k slots"""
    margin, db, method, T = form
    k = sim.shape[1]
    a = a.to(sim.dtype)
    zero = torch.zeros_like(sim)
    if margin == "constant":
        m = torch.full_like(sim[:, :1], nu)
    elif margin == "adaptive":
        m = (mu * a + nu)[:, None]
    else:
        u = torch.where(posmask, zero, sim).sum(1) / k
        v = torch.where(posmask, sim, zero).sum(1) / k
        m = ((u - 1) * a + v)[:, None]
    z = sim
    if db == "-m":
        z = torch.where(posmask, sim - m, sim)
    elif db == "+m":
        z = torch.where(posmask, sim, sim + m)
    if T is not None:
        z = z / T
    e = torch.exp(z)
    ep = torch.where(posmask, e, zero)
    P, N = ep.sum(1), torch.where(posmask, zero, e).sum(1)
    if method == "Method1":
        ratio = P / (P + N) + 1e-12
    else:
        # (the count is an integer tensor there, so `+ _eps` makes it float32 at any dtype of the cosines: 1e-12 vanishes next to a
        #  count >= 1 and stays, rounded to fp32, next to 0)
        ratio = (ep / (ep + N[:, None]) + 1e-12).sum(1) / (posmask.sum(1).to(torch.float32) + 1e-12)
    return -torch.log(ratio)


def keep_rows(a):
    return torch.nonzero((a > 0) & (a <= 1)).flatten()


class StageRef:
    """One stage at `dtype`: x = f as a leaf, sim = cosines of the selected anchors from x / clamp_min(||x||, 1e-8) (retained, so
    that g = dL/dsim comes from autograd whatever the form), per-anchor losses, their mean, and d(grad_out * mean)/df."""

    def __init__(self, f, nidx, posmask, a, form, dtype, grad_out, mu=MU, nu=NU):
        x = f.detach().to(dtype).requires_grad_(True)
        self.rows = rows = keep_rows(a)
        h = x / torch.linalg.vector_norm(x, dim=1).clamp_min(EPS)[:, None]
        sim = (h[rows][:, None, :] * h[nidx[rows].long()]).sum(-1)
        sim.retain_grad()
        self.loss_pt = form_loss(sim, posmask[rows], a[rows], form, mu, nu)
        self.loss = self.loss_pt.mean()
        if rows.numel():
            (self.loss * grad_out).backward()
        self.grad = x.grad.detach() if x.grad is not None else torch.zeros_like(x).detach()
        self.g = sim.grad.detach() if sim.grad is not None else torch.zeros_like(sim).detach()
        self.sim = sim.detach()
        self.loss_pt, self.loss = self.loss_pt.detach(), self.loss.detach()


def edge_decomposition(f, nidx, rows, sim, g):
    """fp64: dL/df_n = sum over the edges (n, x) touching n, own and incoming, of g / max(||f_n||, eps) * (fhat_x - s fhat_n),
    without the projection s fhat_n where the clamp is active (fhat_n = f_n / eps is linear in f_n there).
    -> (A (m): the sum of the terms' magnitudes, max over the channels; df (m, C): their signed sum)"""
    x = f.detach().double()
    m, C = x.shape
    A = torch.zeros(m, dtype=torch.float64, device=x.device)
    df = torch.zeros(m, C, dtype=torch.float64, device=x.device)
    if rows.numel() == 0:
        return A, df
    raw = torch.linalg.vector_norm(x, dim=1)
    n = raw.clamp_min(EPS)
    h = x / n[:, None]
    live = (raw >= EPS).double()
    nb = nidx[rows].long()
    hi, hx = h[rows][:, None, :], h[nb]
    s, g = sim.double(), g.double()
    own = (g / n[rows][:, None])[..., None] * (hx - (live[rows][:, None] * s)[..., None] * hi)
    inc = (g / n[nb])[..., None] * (hi - (live[nb] * s)[..., None] * hx)
    df.index_add_(0, rows, own.sum(1))
    df.index_add_(0, nb.flatten(), inc.reshape(-1, C))
    A.index_add_(0, rows, own.abs().amax(-1).sum(1))
    A.index_add_(0, nb.flatten(), inc.abs().amax(-1).flatten())
    return A, df
