"""The id-to-batch arithmetic of input_pipeline.ScanNetTrainFeed (input_pipeline.feed_picks) against torch's own BatchSampler
and ScanNet.__getitem__'s `idx % len(data_list)` rule.  No GPU."""
import pytest
import torch
from torch.utils.data import BatchSampler


@pytest.mark.parametrize("drop_last", [True, False])
@pytest.mark.parametrize("items,batch_size", [(1, 1), (5, 2), (6, 2), (7, 3), (2, 4), (12, 12), (13, 5)])
def test_feed_picks_groups_ids_as_batch_sampler_does(items, batch_size, drop_last):
    from amcontrast3d_amd.input_pipeline import feed_picks
    ids = torch.randperm(items, generator=torch.Generator().manual_seed(items * 31 + batch_size)).tolist()
    want = list(BatchSampler(ids, batch_size, drop_last))
    got = feed_picks(ids, items, batch_size, drop_last)  # one item per room: the picks are the ids
    assert got == want
    assert len(got) == (items // batch_size if drop_last else -(-items // batch_size))


@pytest.mark.parametrize("drop_last", [True, False])
@pytest.mark.parametrize("n_rooms,loop,batch_size", [(3, 2, 2), (3, 6, 4), (1, 5, 2), (7, 3, 8), (4, 1, 3)])
def test_feed_picks_maps_item_ids_to_rooms_modulo(n_rooms, loop, batch_size, drop_last):
    from amcontrast3d_amd.input_pipeline import feed_picks
    items = n_rooms * loop
    ids = torch.randperm(items, generator=torch.Generator().manual_seed(items)).tolist()
    want = [[i % n_rooms for i in batch] for batch in BatchSampler(ids, batch_size, drop_last)]
    assert feed_picks(ids, n_rooms, batch_size, drop_last) == want
    assert feed_picks(torch.tensor(ids), n_rooms, batch_size, drop_last) == want  # a tensor of ids as well as a list
    if not drop_last:  # a whole epoch: every room exactly `loop` times
        flat = sorted(r for batch in want for r in batch)
        assert flat == sorted(list(range(n_rooms)) * loop)
    # in order, the ids visit the rooms round-robin
    assert feed_picks(range(items), n_rooms, items, False) == [[i % n_rooms for i in range(items)]]


def test_feed_picks_rejects_empty_sizes():
    from amcontrast3d_amd.input_pipeline import feed_picks
    assert feed_picks([], 3, 2, True) == [] and feed_picks([], 3, 2, False) == []
    with pytest.raises(ValueError):
        feed_picks([0, 1], 0, 2, True)
    with pytest.raises(ValueError):
        feed_picks([0, 1], 2, 0, True)
