"""CPU restatements for the k-NN grouper's tests (a helper, not a test module).

  cdist_topk_bmk / cdist_topk_bkm   the composition the reference's two KNN modules write (cdist + topk)
  exact_knn                         the exact neighbour lists from fp64 squared differences, with a per-query `untied` flag
  oracle_knn                        oracle.pointops_ref.knnquery_cuda over uniform offsets, indices made cloud-local
  knn_group_forward                 KNNGroup.forward in fp32, the norm written (x*x + y*y) + z*z
  query_and_group                   a k-NN stand-in for oracle.model_ref's ball-query `query_and_group`
"""
import numpy as np
import torch


def cdist_topk_bmk(k, query, support, farthest=False):
    """layers/knn.py: values (B,M,k), indices (B,M,k) int64"""
    kd = torch.cdist(query, support).topk(k=k, dim=-1, largest=farthest, sorted=True)
    return kd.values, kd.indices


def cdist_topk_bkm(k, support, query):
    """layers/group.py's KNN: values (B,k,M) untransposed, indices (B,M,k) int32"""
    kd = torch.cdist(support, query).topk(k=k, dim=1, largest=False)
    return kd.values, kd.indices.transpose(1, 2).contiguous().int()


def exact_knn(k, query, support):
    """-> idx (B,M,k) int64 ordered by (fp64 squared distance, index), untied (B,M) bool: the first k+1 fp64 distances
    of the query are pairwise distinct, so its list is unique.  The differences of fp32 coordinates are exact in fp64."""
    q, s = query.double(), support.double()
    idx, untied = [], []
    for b in range(q.shape[0]):
        d2 = ((q[b, :, None, :] - s[b, None, :, :]) ** 2).sum(-1)
        order = torch.sort(d2, dim=1, stable=True)
        take = min(k + 1, s.shape[1])
        v = order.values[:, :take]
        idx.append(order.indices[:, :k])
        untied.append((v[:, 1:] > v[:, :-1]).all(dim=1))
    return torch.stack(idx), torch.stack(untied)


def oracle_knn(k, query, support):
    """-> idx (B,M,k) int32 cloud-local, dist2 (B,M,k) fp32 squared, as the reference's pointops kernel computes them"""
    from oracle import pointops_ref as K
    B, N, _ = support.shape
    M = query.shape[1]
    off = torch.arange(1, B + 1, dtype=torch.int32) * N
    noff = torch.arange(1, B + 1, dtype=torch.int32) * M
    idx = torch.zeros(B * M, k, dtype=torch.int32)
    d2 = torch.zeros(B * M, k, dtype=torch.float32)
    K.knnquery_cuda(B * M, k, support.reshape(-1, 3).contiguous(), query.reshape(-1, 3).contiguous(), off, noff, idx, d2)
    idx = idx.view(B, M, k) - (torch.arange(B, dtype=torch.int32) * N).view(B, 1, 1)
    return idx, d2.view(B, M, k)


def oracle_untied(k, query, support):
    """(B,M) bool on the oracle's own k+1 fp32 distances: strictly increasing, so no order of equal distances is in
    play (k == N: the k distances)"""
    _, d2 = oracle_knn(min(k + 1, support.shape[1]), query, support)
    return (d2[..., 1:] > d2[..., :-1]).all(dim=-1)


def gather(features, idx):
    """(B,C,N), (B,M,K) -> (B,C,M,K)"""
    B, C = features.shape[:2]
    flat = idx.reshape(B, 1, -1).expand(-1, C, -1).long()
    return features.gather(2, flat).reshape(B, C, idx.shape[1], idx.shape[2])


def knn_group_forward(idx, query, support, features=None, relative=True, normalize=False):
    """group.py:309-320 in fp32 on the CPU -> dp (B,3,M,K), grouped features or None"""
    dp = gather(support.transpose(1, 2).contiguous(), idx)
    if relative:
        dp = dp - query.transpose(1, 2).unsqueeze(-1)
    if normalize:
        x, y, z = dp[:, 0], dp[:, 1], dp[:, 2]
        norm = torch.sqrt((x * x + y * y) + z * z)
        dp = dp / torch.amax(norm, dim=(1, 2)).view(-1, 1, 1, 1)
    return dp, (gather(features, idx) if features is not None else None)


def query_and_group(radius, nsample, query_xyz, support_xyz, features, normalize_dp=True):
    """oracle.model_ref.query_and_group's signature and returns (dp, grouped features, idx) with the k-NN grouper behind
    it: the radius is unused, normalize_dp divides by the cloud's largest offset.  Coordinates stay fp32 as there."""
    idx, _ = oracle_knn(nsample, query_xyz.float().contiguous(), support_xyz.float().contiguous())
    dp, _ = knn_group_forward(idx, query_xyz.float(), support_xyz.float(), None, True, normalize_dp)
    return dp.to(features.dtype), gather(features, idx), idx


def ulp_diff(a, b):
    """largest distance in units of the last place between two fp32 arrays of non-negative or same-signed values"""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return int(np.abs(a - b).max()) if a.size else 0
