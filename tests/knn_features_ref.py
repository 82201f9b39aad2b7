"""fp64 restatement of ops.knn_features for the tests: exact squared distances and the list of the k smallest pairs
(d2, index) -- farthest: (-d2, index) -- by a stable sort.  Also the fp32 rounding band of the kernel's expression."""
import torch


def exact_d2(query, support):
    """query (B,M,C), support (B,N,C), any float dtype -> (B,M,N) fp64 sum_c (q - s)^2"""
    q, s = query.double(), support.double()
    return ((q[:, :, None, :] - s[:, None, :, :]) ** 2).sum(-1)


def exact_lists(query, support, k, farthest=False):
    """-> (idx (B,M,k) int64, d2 (B,M,k) fp64, d2 of all pairs (B,M,N)): ascending (d2, index), or ascending (-d2, index)"""
    d2 = exact_d2(query, support)
    order = torch.sort(-d2 if farthest else d2, dim=-1, stable=True).indices[..., :k]
    return order, torch.gather(d2, -1, order), d2


def band(query, support):
    """tol (B,M,N) = 2 (C + 3) 2^-24 (|q_i|^2 + |s_j|^2): the rounding bound of d2 = (qq + ss) - 2 dot in fp32.  Each of the
    three chains over C channels is within C 2^-24 of its sum of absolute products (|q|^2, |s|^2, and |q.s| <= (|q|^2 +
    |s|^2) / 2, doubled), the sum qq + ss and the final subtraction round once more each on values no larger than
    2 (|q|^2 + |s|^2): in all below (2 C + 6) 2^-24 (|q|^2 + |s|^2)."""
    C = query.shape[-1]
    qq = (query.double() ** 2).sum(-1)
    ss = (support.double() ** 2).sum(-1)
    return 2.0 * (C + 3) * 2.0 ** -24 * (qq[:, :, None] + ss[:, None, :])
