"""ops.posmask_and_ambiguity (csrc/loss.hip amc3d_loss_rows): the positive mask and the neighbourhood statistics of a loss
stage in one pass over its neighbour rows.  Every output -- mask, n+, d+, d-, the grid-wide max n+ and the ambiguity -- must
carry the bits of amc3d_posmask followed by amc3d_ambiguity: d+ and d- are sums of cancelling terms in a fixed order and the
ambiguity is steep in them, so nothing here is compared with a tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = {1: "Method1", 2: "Method2", 3: "Method3"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from amcontrast3d_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def two_kernels(labels, p, nbr, mode, beta):
    """amc3d_posmask + amc3d_ambiguity with the workspace kept: (posmask, a, (max n+, n+, d+, d-))"""
    from amcontrast3d_amd import _lib, ops
    lib = _lib.load()
    posmask = ops.posmask_from_labels(labels, nbr)
    m, k = nbr.shape
    wbytes = int(lib.amc3d_ambiguity_workspace_bytes(m))
    work = torch.empty(wbytes, dtype=torch.uint8, device=p.device)
    a = torch.empty(m, dtype=torch.float32, device=p.device)
    _lib.check(lib.amc3d_ambiguity(m, k, nbr.stride(0), mode, beta, p.data_ptr(), posmask.data_ptr(), nbr.data_ptr(),
                                   a.data_ptr(), work.data_ptr(), wbytes, torch.cuda.current_stream().cuda_stream), "ambiguity")
    return posmask, a, (work[:4].view(torch.int32), work[64:64 + 4 * m].view(torch.int32),
                        work[64 + 4 * m:64 + 8 * m].view(torch.float32), work[64 + 8 * m:64 + 12 * m].view(torch.float32))


def label_sets(m, g):
    return {"equal": torch.full((m,), 3, dtype=torch.int32), "different": torch.arange(m, dtype=torch.int32),
            "random13": torch.randint(0, 13, (m,), generator=g, dtype=torch.int32)}


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("m,k,stride", [(1, 23, 24), (63, 23, 24), (1000, 23, 24), (257, 7, 8), (130, 63, 64)])
def test_one_pass_equals_the_two_kernels(dev, m, k, stride, mode):
    from amcontrast3d_amd import ops
    g = torch.Generator().manual_seed(m * 100 + k)
    # points of a few tight clusters far from the origin: the expanded squared distance cancels, and comes out negative too
    p = (torch.randint(0, 4, (m, 1), generator=g).float() * 3 + 7 + 0.01 * torch.randn(m, 3, generator=g)).to(dev)
    full = torch.randint(0, m, (m, stride), generator=g, dtype=torch.int32)
    full[:, stride - 1] = full[:, stride - k]  # every list names a point twice (m == 1: all the same point anyway)
    if k > 2:
        full[::3, stride - k + 2] = full[::3, stride - k + 1]
    nbr = full.to(dev)[:, stride - k:]  # the first stride - k columns are skipped by the pointer offset
    assert nbr.stride(0) == stride and nbr.shape[1] == k
    beta = 0.5
    for name, labels in label_sets(m, g).items():
        labels = labels.to(dev)
        assert ops.loss_rows_supported(p, labels, nbr)
        want_mask, want_a, want_stats = two_kernels(labels, p, nbr, mode, beta)
        mask, a, stats = ops.posmask_and_ambiguity(labels, p, nbr, MODES[mode], beta, stats=True)
        assert mask.dtype == torch.bool and torch.equal(mask, want_mask), name
        for got, want, what in zip(stats, want_stats, ("max n+", "n+", "d+", "d-")):
            assert got.dtype == want.dtype and torch.equal(got, want), (name, what)
        # (a may hold NaN where d+ or d- is 0 or the lists are all-negative: the same NaN in both)
        assert torch.equal(a.view(torch.int32), want_a.view(torch.int32)), name
        if mode != 1 and name == "random13" and m > 1:
            assert bool((want_stats[2] != 0).any()) and bool((want_stats[3] != 0).any())  # the sums are exercised


def test_more_than_64_neighbours_keep_the_two_kernels(dev):
    from amcontrast3d_amd import ops
    p = torch.randn(100, 3, device=dev)
    labels = torch.zeros(100, dtype=torch.int32, device=dev)
    assert not ops.loss_rows_supported(p, labels, torch.zeros(100, 65, dtype=torch.int32, device=dev))
    assert not ops.loss_rows_supported(p.double(), labels, torch.zeros(100, 23, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError):
        ops.posmask_and_ambiguity(labels, p, torch.zeros(100, 65, dtype=torch.int32, device=dev), "Method2", 0.5)
