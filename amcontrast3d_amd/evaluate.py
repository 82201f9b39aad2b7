"""Evaluation loops around the hot path: validation batches and whole-room testing with boundary / inner mIoU
(the reference's `validate_boundary_inner` and `test_boundary_inner`, examples/segmentation/main_AA.py:431-802;
SURVEY.md section 8(f) rank 2).

The reference's loops are welded to its dataset readers, transform registry, tqdm / wandb logging and result
files; what they compute is restated here on arrays the caller already holds:

    voxel_parts                 main_AA.py:91-116 (`load_data`, multi_voxel mode) + dataset/data_util.py:92-143
    voxel_representatives       main_AA.py:99-107, 666 (`load_data`, nearest_neighbor mode)
    boundary_mask               main_AA.py:470-476, 628-633 (posmask_searching + the 0 < n+ < nsample test)
    scatter_mean                torch_scatter.scatter(..., reduce='mean') of main_AA.py:662 (package absent here)
    validate_boundary_inner     main_AA.py:431-513
    test_cloud_boundary_inner   one iteration of the cloud loop of main_AA.py:556-684
    test_room_scannet           the same iteration for a raw ScanNet room, split / gathered / voted on the device
    scannet_benchmark_ids       main.py:652-659 (the label ids of the benchmark's submission files)
    test_room_s3dis             the same iteration for a raw S3DIS room with the config's evaluation transforms, on the device
    summarize                   main_AA.py:484-506 / 746-770 (get_mious over the accumulated matrices)
    validate_sphere             main.py:436-483 (S3DISSphere batches: logits of overlapping spheres averaged per sub-point)

The model runs with model.eval(): BatchNorm uses its running statistics on the fused inference kernels
(ops.bn_eval), FPS / ball query / grouped convolutions / 3-NN are the same HIP kernels as in training.
"""
import numpy as np
import torch

from . import activate


def _fnv64(cells):
    """FNV-1a over the integer voxel coordinates, as dataset/data_util.py:92-105 (uint64 wrap-around)."""
    h = np.full(cells.shape[0], 14695981039346656037, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for j in range(cells.shape[1]):
            h *= np.uint64(1099511628211)
            h ^= cells[:, j]
    return h


def voxel_parts(coord, voxel_size, rng=None):
    """Split a cloud into sub-clouds holding one point per occupied voxel each (test_mode 'multi_voxel'):
    part i takes the (i mod count)-th point of every voxel, so count.max() parts cover every point and sparse voxels
    repeat theirs.  Returns the list of index arrays (each shuffled with `rng`, as the reference shuffles them)."""
    cells = np.floor(np.asarray(coord) / np.asarray(voxel_size)).astype(np.uint64)
    key = _fnv64(cells)
    order = np.argsort(key)
    _, count = np.unique(key[order], return_counts=True)
    first = np.cumsum(np.insert(count, 0, 0)[:-1])
    rng = np.random.default_rng(0) if rng is None else rng
    parts = []
    for i in range(int(count.max())):
        part = order[first + i % count]
        rng.shuffle(part)
        parts.append(part)
    return parts


def voxel_representatives(coord, voxel_size, rng=None):
    """test_mode 'nearest_neighbor' (main_AA.py:99-107): ONE sub-cloud holding a random point of every occupied voxel;
    afterwards every point takes the logits of its voxel's representative (main_AA.py:666).
    Returns (part, expand): the representatives' indices (shuffled) and, for every point of the cloud, the position in
    `part` of its voxel's representative -- test_cloud_boundary_inner(..., parts=[part], expand=expand)."""
    cells = np.floor(np.asarray(coord) / np.asarray(voxel_size)).astype(np.uint64)
    key = _fnv64(cells)
    order = np.argsort(key)
    _, voxel_of_sorted, count = np.unique(key[order], return_inverse=True, return_counts=True)
    first = np.cumsum(np.insert(count, 0, 0)[:-1])
    rng = np.random.default_rng(0) if rng is None else rng
    pick = order[first + rng.integers(0, count.max(), count.size) % count]  # one point per voxel, voxel order
    perm = rng.permutation(count.size)
    part = pick[perm]
    where = np.argsort(perm)                       # voxel -> position of its representative in `part`
    expand = np.empty(len(key), dtype=np.int64)
    expand[order] = where[voxel_of_sorted]         # undo the sort by hash
    return part, expand


@torch.no_grad()
def boundary_mask(xyz, target, nsample, num_classes, ignore_index):
    """(m) bool: points whose nsample-1 nearest neighbours contain between 1 and nsample-1 points of their own class.
    (The upper bound is `< nsample`, not `< nsample - 1`, exactly as main_AA.py:475 writes it: a point all of whose
    neighbours agree with it therefore counts as boundary too, and "inner" means no neighbour agrees.)"""
    activate()
    from openpoints.AMContrast3D.metrics import posmask_searching
    posmask, _ = posmask_searching(xyz, target, nsample, num_classes, ignore_index)
    same = posmask.sum(-1)
    return torch.logical_and(0 < same, same < nsample)


def scatter_mean(src, index, size=None):
    """out[j] = mean of src[i] over index[i] == j (0 where no i): torch_scatter.scatter(src, index, dim=0,
    reduce='mean') for 2-d src, which is how overlapping sub-cloud logits are voted (main_AA.py:662)."""
    n = int(index.max().item()) + 1 if size is None else size
    out = torch.zeros(n, src.shape[1], dtype=src.dtype, device=src.device)
    out.index_add_(0, index, src)
    cnt = torch.zeros(n, dtype=src.dtype, device=src.device)
    cnt.index_add_(0, index, torch.ones_like(index, dtype=src.dtype))
    return out / cnt.clamp(min=1).unsqueeze(1)


def _logits(out):
    """the AMContrast3D models return (logits, stageACE_list); the plain PointNeXt baseline (BaseSeg) the logits alone"""
    if torch.is_tensor(out):
        return out
    logits, _ = out
    return logits


def _matrices(num_classes, ignore_index):
    activate()
    from openpoints.utils import ConfusionMatrix
    return [ConfusionMatrix(num_classes=num_classes, ignore_index=ignore_index) for _ in range(3)]


def summarize(cm, cm_b=None, cm_i=None, distributed=False):
    """(miou, macc, oa, ious, accs) for the whole set [+ the same five for boundary and inner points], with the
    cross-rank sum of (tp, union, count) first when `distributed` (main_AA.py:459-462, 484-500)."""
    activate()
    from openpoints.utils import get_mious
    out = ()
    for m in (cm, cm_b, cm_i):
        if m is None:
            continue
        tp, union, count = m.tp, m.union, m.count
        if distributed:
            import torch.distributed as dist
            from .graphs import on_side_stream
            on_side_stream(lambda: (dist.all_reduce(tp), dist.all_reduce(union), dist.all_reduce(count)))
        out += tuple(get_mious(tp, union, count))
    return out


@torch.no_grad()
def validate_boundary_inner(model, batches, num_classes, ignore_index, nsample, miou_B_I=True, distributed=False):
    """Validation pass over batches of ONE cloud each (the reference's val loader uses batch size 1;
    `data['pos'].squeeze()` at main_AA.py:469 assumes it): dicts with pos (1,N,3), x (1,C,N), y (1,N) on the GPU.
    Returns summarize(...) of the whole / boundary / inner confusion matrices.  miou_B_I=False is the plain trainer's
    `validate` (examples/segmentation/main.py:392-433): one matrix over all points, any batch size, five values."""
    model.eval()
    cm, cm_b, cm_i = _matrices(num_classes, ignore_index)
    for data in batches:
        target = data["y"].reshape(data["y"].shape[0], -1)
        logits = _logits(model(data))
        pred = logits.argmax(dim=1)
        cm.update(pred, target)
        if miou_B_I:
            assert data["pos"].shape[0] == 1, "boundary / inner split is defined per cloud (batch size 1)"
            b = boundary_mask(data["pos"][0], target[0], nsample, num_classes, ignore_index).unsqueeze(0)
            cm_b.update(pred[b], target[b])
            cm_i.update(pred[~b], target[~b])
    return summarize(cm, cm_b, cm_i, distributed) if miou_B_I else summarize(cm, distributed=distributed)


@torch.no_grad()
def boundary_masks_stacked(pos, labels, nsample, num_classes, ignore_index):
    """boundary_mask for P equally sized clouds in one k-NN call: pos (P,n,3), labels (P,n) -> (P,n) bool.  The clouds
    are the segments of one knnquery (offsets n, 2n, ...), which searches every segment on its own -- the same lists
    as P separate calls (main_AA.py:628 calls posmask_searching per sub-cloud)."""
    activate()
    from openpoints.cpp.pointops.functions import pointops
    from . import ops
    P, n = labels.shape
    xyz = pos.reshape(P * n, 3).contiguous()
    target = labels.reshape(-1)
    if ignore_index is not None:
        target = torch.where(target == ignore_index, num_classes, target)
    o = torch.arange(1, P + 1, dtype=torch.int32, device=xyz.device) * n
    idx, _ = pointops.knnquery(nsample, xyz, xyz, o, o)
    same = ops.posmask_from_labels(target.to(torch.int32).contiguous(), idx[..., 1:].contiguous()).sum(-1)
    return torch.logical_and(0 < same, same < nsample).view(P, n)


@torch.no_grad()
def test_cloud_boundary_inner(model, coord, feat, label, parts, num_classes, ignore_index, nsample,
                              make_input=None, miou_B_I=True, batch=64, expand=None):
    """One whole cloud (room): every sub-cloud of `parts` goes through the model, overlapping logits are averaged per
    point, and three confusion matrices are filled -- all points (voted prediction), boundary and inner points (per
    sub-cloud predictions, as the reference keeps them: main_AA.py:634-641, 651-657, 671-676).

    coord (n,3) float array, feat (n,c) float array or None, label (n) int tensor on the GPU, parts: index arrays.
    make_input(coord_part, feat_part) -> model input dict; default: pos shifted to its minimum corner, x = feat and
    the height channel (the S3DIS feature_keys 'x,heights', cfgs/s3dis/default.yaml).
    batch: sub-clouds stacked per model call.  The reference feeds them one at a time (main_AA.py:575-611); in eval
    mode nothing couples the clouds of a batch (BatchNorm uses running statistics, FPS / ball query / 3-NN work per
    cloud), so the logits are the same -- but the FPS chain is latency-bound, 8 ms for 24 k points on ONE workgroup
    per cloud, and 5/6 of the model time at 8 clouds per call (scratch/eval_phases.py): stacking a whole room runs all
    its chains side by side.  Sub-clouds of a voxel partition have one point per voxel, hence equal size; with the
    default make_input they are also gathered and shifted on the GPU (one upload of the room instead of one per
    sub-cloud) and their boundary masks come from one segmented k-NN call.  Ragged parts fall back to single calls.
    expand: with the single sub-cloud of voxel_representatives, the per-point index into it ('nearest_neighbor' mode).
    Returns dict(pred, logits, cm, cm_b, cm_i)."""
    model.eval()
    dev = label.device
    cm, cm_b, cm_i = _matrices(num_classes, ignore_index)
    same_size = len({len(p) for p in parts}) == 1
    step = max(1, int(batch)) if same_size else 1
    index = torch.from_numpy(np.hstack(parts)).to(dev)
    all_logits, pb, pi, tb, ti = [], [], [], [], []

    def split_by_boundary(pred_stack, label_stack, b):
        pb.append(pred_stack[b]); pi.append(pred_stack[~b]); tb.append(label_stack[b]); ti.append(label_stack[~b])

    if make_input is None and same_size:
        # the room goes to the GPU once; sub-clouds are gathered, shifted to their minimum corner (in the array's own
        # precision, as numpy does it at main_AA.py:578-579) and stacked there
        idx = index.view(len(parts), -1)
        room = torch.from_numpy(np.ascontiguousarray(coord)).to(dev)
        room_f = None if feat is None else torch.from_numpy(np.ascontiguousarray(feat, dtype=np.float32)).to(dev)
        for j0 in range(0, len(parts), step):
            sel = idx[j0:j0 + step]
            pos = room[sel]
            pos = (pos - pos.amin(dim=1, keepdim=True)).float()
            cols = ([room_f[sel]] if room_f is not None else []) + [pos[..., 2:3]]
            data = {"pos": pos.contiguous(), "x": torch.cat(cols, dim=2).transpose(1, 2).contiguous()}
            logits = _logits(model(data))
            all_logits.append(logits)
            if miou_B_I:
                split_by_boundary(logits.argmax(dim=1), label[sel],
                                  boundary_masks_stacked(data["pos"], label[sel], nsample, num_classes, ignore_index))
    else:
        if make_input is None:
            def make_input(coord_part, feat_part):
                pos = torch.from_numpy(np.ascontiguousarray(coord_part, dtype=np.float32)).to(dev).unsqueeze(0)
                cols = [torch.from_numpy(np.ascontiguousarray(feat_part, dtype=np.float32)).to(dev)] if feat_part is not None else []
                return {"pos": pos, "x": torch.cat(cols + [pos[0, :, 2:3]], dim=1).t().contiguous().unsqueeze(0)}
        inputs = []
        for part in parts:
            coord_part = np.asarray(coord)[part]
            inputs.append(make_input(coord_part - coord_part.min(0), None if feat is None else np.asarray(feat)[part]))
        for j0 in range(0, len(parts), step):
            chunk = inputs[j0:j0 + step]
            data = chunk[0] if len(chunk) == 1 else {k: torch.cat([d[k] for d in chunk], dim=0) for k in chunk[0]}
            logits = _logits(model(data))
            all_logits.append(logits)
            if miou_B_I:
                for j, d in enumerate(chunk):
                    label_part = label[torch.from_numpy(parts[j0 + j]).to(dev)]
                    b = boundary_mask(d["pos"][0], label_part, nsample, num_classes, ignore_index)
                    split_by_boundary(logits[j].argmax(dim=0), label_part, b)
    flat = torch.cat([lg.transpose(1, 2).reshape(-1, num_classes) for lg in all_logits], dim=0)
    if expand is not None:
        assert len(parts) == 1, "expand belongs to the single sub-cloud of voxel_representatives"
        voted = flat[torch.from_numpy(np.asarray(expand)).to(dev)]
    else:
        voted = scatter_mean(flat, index, size=label.shape[0]) if len(parts) > 1 else flat[torch.argsort(index)]
    pred = voted.argmax(dim=1)
    cm.update(pred, label)
    if miou_B_I:
        cm_b.update(torch.cat(pb), torch.cat(tb))
        cm_i.update(torch.cat(pi), torch.cat(ti))
    return {"pred": pred, "logits": voted, "cm": cm, "cm_b": cm_b, "cm_i": cm_i}


# the benchmark's label id of each of the 20 training classes (dataset/scannetv2/scannet.py VALID_CLASS_IDS)
SCANNET_VALID_CLASS_IDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)


def scannet_benchmark_ids(pred):
    """class indices 0..19 -> the ScanNet benchmark's label ids, as the `save_pred` text files hold them
    (examples/segmentation/main.py:652-659).  pred: integer tensor or array; the result has its type."""
    if torch.is_tensor(pred):
        if pred.numel() and (int(pred.min()) < 0 or int(pred.max()) >= len(SCANNET_VALID_CLASS_IDS)):
            raise ValueError("scannet_benchmark_ids: predictions must be class indices 0..19")
        return torch.tensor(SCANNET_VALID_CLASS_IDS, dtype=pred.dtype, device=pred.device)[pred.long()]
    pred = np.asarray(pred)
    if pred.size and (pred.min() < 0 or pred.max() >= len(SCANNET_VALID_CLASS_IDS)):
        raise ValueError("scannet_benchmark_ids: predictions must be class indices 0..19")
    return np.asarray(SCANNET_VALID_CLASS_IDS, dtype=pred.dtype)[pred]


def _test_room(model, rp, make_batch, vote, label, num_classes, ignore_index, nsample, miou_B_I, batch):
    """the sub-cloud loop of test_room_scannet / test_room_s3dis: make_batch(rows of rp["parts"]) -> the model -> the
    boundary split per sub-cloud, then vote(logits (P,C,nvox), rp) -> (voted, pred) and the three matrices"""
    P, nvox = rp["parts"].shape
    cm = cm_b = cm_i = None
    if label is not None:
        cm, cm_b, cm_i = _matrices(num_classes, ignore_index)
    step = max(1, int(batch))
    logits_all = torch.empty(P, num_classes, nvox, dtype=torch.float32, device=rp["parts"].device)
    pb, pi, tb, ti = [], [], [], []
    for j0 in range(0, P, step):
        data = make_batch(rp["parts"][j0:j0 + step])
        logits = _logits(model(data))
        logits_all[j0:j0 + step] = logits
        if miou_B_I:
            b = boundary_masks_stacked(data["pos"], data["y"], nsample, num_classes, ignore_index)
            pred_stack = logits.argmax(dim=1)
            pb.append(pred_stack[b]); pi.append(pred_stack[~b]); tb.append(data["y"][b]); ti.append(data["y"][~b])
    voted, pred = vote(logits_all, rp)
    if label is not None:
        cm.update(pred, label)
    if miou_B_I:
        cm_b.update(torch.cat(pb), torch.cat(tb))
        cm_i.update(torch.cat(pi), torch.cat(ti))
    return {"pred": pred, "logits": voted, "cm": cm, "cm_b": cm_b, "cm_i": cm_i}


def _batch_options(gravity_dim, feature_keys, color_mean, color_std):
    """the keyword arguments of part_batch / s3dis_part_batch; None keeps the dataset's own colour constants"""
    kw = {"gravity_dim": gravity_dim, "feature_keys": feature_keys}
    if color_mean is not None:
        kw["color_mean"] = color_mean
    if color_std is not None:
        kw["color_std"] = color_std
    return kw


@torch.no_grad()
def test_room_scannet(model, coord, feat, label, voxel_size, num_classes, ignore_index, nsample,
                      feature_keys="pos,x,heights", color_mean=None, color_std=None, gravity_dim=2, miou_B_I=False,
                      batch=8, perm=None, generator=None, variable=False):
    """One whole ScanNet room through the test loop (main.py:512-660 / main_AA.py:517-684 with `load_data`'s scannet
    branch, `feature_keys: pos,x,heights`, `test: [PointsToTensor, NumpyChromaticNormalize]`), everything after the upload
    on the device: coord - min, input_pipeline.room_parts, part_batch over `batch` sub-clouds at a time, the model,
    ops.vote_parts.

    coord (n,3) fp32, feat (n,3) fp32 in [-1, 1], label (n[,1]) or None (the `test` split): the raw .pth arrays (numpy or
    tensors).  perm / generator: the shuffles of the sub-clouds (room_parts).  Confusion matrices as
    test_cloud_boundary_inner fills them: all points from the voted prediction, boundary / inner from the per-sub-cloud
    predictions.  The one deviation from the reference: the vote adds a point's logits in ascending sub-cloud order where
    torch_scatter's atomics add them in any order.  Returns dict(pred, logits, cm, cm_b, cm_i); the matrices are None
    without labels."""
    from . import input_pipeline as ip
    from . import ops
    if variable:
        raise ValueError("test_room_scannet: `variable: True` batches are not built (the ScanNet configs stack sub-clouds)")
    model.eval()
    dev = next(model.parameters()).device
    up = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev)  # noqa: E731
    coord, feat = up(coord), up(feat)
    label = None if label is None else up(label).reshape(-1).long()
    if miou_B_I and label is None:
        raise ValueError("test_room_scannet: the boundary / inner split needs labels")
    coord = coord - coord.min(0).values  # load_data: coord -= coord.min(0), in the array's own precision
    rp = ip.room_parts(coord, voxel_size, perm=perm, generator=generator)
    kw = _batch_options(gravity_dim, feature_keys, color_mean, color_std)
    return _test_room(model, rp, lambda rows: ip.part_batch(rows, coord, feat, label, "test", **kw), ops.vote_parts, label,
                      num_classes, ignore_index, nsample, miou_B_I, batch)


@torch.no_grad()
def test_room_s3dis(model, cdata, voxel_size, num_classes, ignore_index, nsample, feature_keys="x,heights", color_mean=None,
                    color_std=None, gravity_dim=2, miou_B_I=False, batch=8, test_mode="multi_voxel", perm=None, rnd=None,
                    generator=None, variable=False):
    """One whole S3DIS room through the test loop (main.py:512-612 / main_AA.py:517-684 with `load_data`'s s3dis branch and
    the transforms of cfgs/s3dis/default.yaml, `val: [PointsToTensor, PointCloudXYZAlign, ChromaticNormalize]`, which test()
    uses for want of a `test` list), everything after the upload on the device: coord - min, input_pipeline.room_parts or
    room_representatives, s3dis_part_batch over `batch` sub-clouds at a time, the model, ops.vote_parts or expand_parts.

    cdata (n,7) or (n,6): the raw .npy array, float64 or float32 (numpy or tensor): xyz, rgb 0..255 [, label]; the arithmetic
    before the cast to float32 is in its dtype, as numpy's is.  test_mode 'multi_voxel' (perm / generator: the shuffles, as in
    room_parts) or 'nearest_neighbor' (rnd, perm, generator: room_representatives).  Confusion matrices as
    test_cloud_boundary_inner fills them.  Deviations from the reference: the xy-centre of a sub-cloud is the fixed-order fp64
    mean rounded once (torch.mean's last bit depends on the host), the vote adds in ascending sub-cloud order, and a room
    whose voxels all hold one point is voted over its one part (the reference then takes its nearest-neighbour branch with
    tables it never built).  6-fold testing is `all_cm.value += r["cm"].value` over the rooms of every area.
    Returns dict(pred, logits, cm, cm_b, cm_i); the matrices are None without labels."""
    from . import input_pipeline as ip
    from . import ops
    if variable:
        raise ValueError("test_room_s3dis: `variable: True` batches are not built (sub-clouds of one room are stacked)")
    if test_mode not in ("multi_voxel", "nearest_neighbor"):
        raise ValueError(f"test_room_s3dis: test_mode {test_mode!r} (multi_voxel or nearest_neighbor)")
    model.eval()
    dev = next(model.parameters()).device
    cdata = (cdata if torch.is_tensor(cdata) else torch.from_numpy(np.ascontiguousarray(cdata))).to(dev)
    if cdata.dim() != 2 or cdata.shape[1] not in (6, 7) or cdata.dtype not in (torch.float32, torch.float64):
        raise ValueError("test_room_s3dis: cdata (n,7) or (n,6), float32 or float64: xyz, rgb [, label]")
    label = cdata[:, 6].long() if cdata.shape[1] == 7 else None
    if miou_B_I and label is None:
        raise ValueError("test_room_s3dis: the boundary / inner split needs labels")
    coord = cdata[:, :3] - cdata[:, :3].min(0).values  # load_data: coord -= coord.min(0), in the file's own precision
    colour = cdata[:, 3:6].contiguous()
    if test_mode == "nearest_neighbor":
        rp, vote = ip.room_representatives(coord, voxel_size, rnd=rnd, perm=perm, generator=generator), ops.expand_parts
    else:
        rp, vote = ip.room_parts(coord, voxel_size, perm=perm, generator=generator), ops.vote_parts
    kw = _batch_options(gravity_dim, feature_keys, color_mean, color_std)
    return _test_room(model, rp, lambda rows: ip.s3dis_part_batch(rows, coord, colour, label, "test", **kw), vote, label,
                      num_classes, ignore_index, nsample, miou_B_I, batch)


@torch.no_grad()
def vote_spheres(logits, input_inds, n_sub):
    """validate_sphere's `scatter(all_logits, idx_points, dim=0, reduce='mean')` (main.py:461-468) without atomics: logits
    (M,C) float32 rows in (batch, slot) order, input_inds (M) -> (voted (n_sub,C), visits (n_sub) int32).  A gather over the
    reverse lists of input_inds (amc3d_group_csr with b = 1, then amc3d_pointops_scatter_csr's summation-order contract): per
    sub-point the float32 sum of its rows in ascending (batch, slot) order from +0, divided by their number -- the same bits on
    every run.  A sub-point no sphere visited gets zero logits."""
    from . import ops
    from .offset_ops import _scatter_csr_lists
    flat = logits.contiguous()
    idx = input_inds.reshape(1, -1, 1).to(torch.int32).contiguous()
    rev_start, rev_edge = ops.group_csr(idx, int(n_sub))
    total = _scatter_csr_lists(0, rev_start, rev_edge, int(n_sub), flat.shape[1], 1, 1, flat, None)
    visits = rev_start[1:] - rev_start[:-1]
    # the float32 quotient through float64: 53 bits round once more to the correctly rounded float32 division (53 >= 2 * 24 + 2)
    return (total.double() / visits.clamp(min=1).double().unsqueeze(1)).float(), visits


@torch.no_grad()
def validate_sphere(model, batches, n_sub, projections, labels, num_classes, ignore_index=None, feature_keys="x,heights",
                    distributed=False, details=False):
    """The reference's validate_sphere (examples/segmentation/main.py:436-483) on S3DISSphere batches of ONE cloud (the
    reference validates cloud 0 only): every batch {pos, x, heights, input_inds, ...} goes through the model in eval mode, the
    logits of all slots of all batches -- padding duplicates included, the reference applies no mask here -- are averaged per
    sub-point (vote_spheres), then argmax, then pred[projections] against the raw points' labels into one confusion matrix.
    n_sub: the cloud's number of sub-points; projections (n_raw): input_pipeline.sphere_projections or the reference's own;
    labels (n_raw).  Differences from the reference: the vote adds in ascending (batch, slot) order instead of atomics, and a
    sub-point no sphere visited has zero logits (class 0) where the reference's shorter scatter output would raise on
    projection.  distributed=True all-reduces the confusion vectors only (the reference's all_reduce of logits and indices
    is not built).  Returns summarize(cm): (miou, macc, oa, ious, accs); details=True: dict(logits (n_sub,C) voted, pred (n_sub),
    cm) instead, before any cross-rank sum."""
    from .train import get_features_by_keys
    model.eval()
    cm = _matrices(num_classes, ignore_index)[0]
    dev = next(model.parameters()).device
    all_logits, inds = [], []
    for data in batches:
        data = dict(data)
        data["x"] = get_features_by_keys(data, feature_keys)
        logits = _logits(model(data))
        all_logits.append(logits.transpose(1, 2).reshape(-1, num_classes))
        inds.append(data["input_inds"].reshape(-1))
    if not all_logits:
        raise ValueError("validate_sphere: no batches")
    voted, _ = vote_spheres(torch.cat(all_logits, dim=0), torch.cat(inds), n_sub)
    pred = voted.argmax(dim=1)
    projections = torch.as_tensor(projections).to(dev).long().reshape(-1)
    labels = torch.as_tensor(labels).to(dev).long().reshape(-1)
    cm.update(pred[projections], labels)
    if details:
        return {"logits": voted, "pred": pred, "cm": cm}
    return summarize(cm, distributed=distributed)
