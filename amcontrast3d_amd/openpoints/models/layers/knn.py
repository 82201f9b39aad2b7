"""k nearest neighbours of (B,N,C) clouds.

API mirror of models/layers/knn.py: ``knn_point`` (:6-20), ``KNN`` (:23-61), ``DenseDilated`` (:65-88),
``DilatedKNN`` (:91-108).  CUDA fp32 coordinates of width 3 with ``farthest=False`` and at most 100 columns go through
the gfx950 search (ops.knn_batch: amc3d_knnquery's distances and order of equal distances); every other input -- CPU
tensors, feature-space k-NN, ``farthest=True``, more columns, other dtypes -- runs the composition the reference
writes, cdist + topk.
"""
import torch
import torch.nn as nn

from amcontrast3d_amd import ops


def kernel_route(query, support, columns, farthest=False):
    """True when the neighbour search of these clouds runs on the HIP kernels"""
    return (not farthest and query.is_cuda and support.is_cuda and query.dtype == torch.float32
            and support.dtype == torch.float32 and query.dim() == 3 and support.dim() == 3 and query.shape[-1] == 3
            and support.shape[-1] == 3 and query.shape[0] == support.shape[0] and 1 <= columns <= ops.KNN_BATCH_MAX)


def kernel_search(k, query, support, dilation=1, dist=None):
    """ops.knn_batch on the tensors as the modules get them: one tensor for both clouds stays one tensor (self-search)"""
    if support is query:
        support = query = query.detach().contiguous()
    else:
        support, query = support.detach().contiguous(), query.detach().contiguous()
    return ops.knn_batch(k, support, query, dilation=dilation, dist=dist)


@torch.no_grad()
def knn_point(k, query, support=None):
    """query (B,M,C), support (B,N,C) -> distances (B,M,k), indices (B,M,k) int64"""
    if support is None:
        support = query
    if kernel_route(query, support, k):
        dist, idx = kernel_search(k, query, support, dist="bmk")
        return dist, idx.long()
    dist = torch.cdist(query, support)
    k_dist = dist.topk(k=k, dim=-1, largest=False, sorted=True)
    return k_dist.values, k_dist.indices


class KNN(nn.Module):
    """distances and indices of a fixed number of neighbours, both (B,M,neighbors); indices int32"""

    def __init__(self, neighbors, farthest=False, sorted=True, **kwargs):
        super(KNN, self).__init__()
        self.neighbors = neighbors
        self.farthest = farthest
        self.sorted = sorted

    @torch.no_grad()
    def forward(self, query, support=None):
        if support is None:
            support = query
        if kernel_route(query, support, self.neighbors, self.farthest):  # always sorted, which `sorted=False` allows
            return kernel_search(self.neighbors, query, support, dist="bmk")
        dist = torch.cdist(query, support)
        k_dist = dist.topk(k=self.neighbors, dim=-1, largest=self.farthest, sorted=self.sorted)
        return k_dist.values, k_dist.indices.int()


class DenseDilated(nn.Module):
    """every dilation-th of the (B,npoint,k*dilation) neighbours; in training, with probability epsilon, a random k"""

    def __init__(self, k=9, dilation=1, stochastic=False, epsilon=0.0):
        super(DenseDilated, self).__init__()
        self.dilation = dilation
        self.stochastic = stochastic
        self.epsilon = epsilon
        self.k = k

    def draw(self):
        """the columns of a stochastic pick, or None for the strided one.  Draws from torch's global CPU generator
        exactly as the reference's forward does: rand(1) whenever stochastic, randperm only when that falls below epsilon
        in training"""
        if self.stochastic and torch.rand(1) < self.epsilon and self.training:
            return torch.randperm(self.k * self.dilation)[:self.k]
        return None

    def pick(self, edge_index, randnum):
        if randnum is not None:
            return edge_index[:, :, randnum.to(edge_index.device)].contiguous()
        return edge_index[:, :, ::self.dilation].contiguous()

    def forward(self, edge_index):
        return self.pick(edge_index, self.draw())


class DilatedKNN(nn.Module):
    """indices (B,N,k) int32 of the dilated k-NN of a cloud among itself"""

    def __init__(self, k=9, dilation=1, stochastic=False, epsilon=0.0):
        super(DilatedKNN, self).__init__()
        self.dilation = dilation
        self.stochastic = stochastic
        self.epsilon = epsilon
        self.k = k
        self._dilated = DenseDilated(k, dilation, stochastic, epsilon)
        self.knn = KNN(k * self.dilation, transpose_mode=True)

    def forward(self, query):
        if not kernel_route(query, query, self.k * self.dilation):
            _, idx = self.knn(query, query)
            return self._dilated(idx)
        # the strided pick happens in the search's epilogue; a stochastic pick needs all k * dilation columns
        randnum = self._dilated.draw()
        if randnum is None:
            return kernel_search(self.k, query, query, dilation=self.dilation)[1]
        return self._dilated.pick(kernel_search(self.k * self.dilation, query, query)[1], randnum)
