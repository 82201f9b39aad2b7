"""The loader's per-cloud preprocessing on the MI355X.

Same names, arguments and results as the reference's numpy functions
    voxelize(coord, voxel_size, hash_type, mode)      openpoints/dataset/data_util.py:127-141
    crop_pc(coord, feat, label, split, voxel_size, voxel_max, downsample, variable, shuffle)   :146-174
on torch GPU tensors, running csrc/voxel.hip: FNV-1a cell hash, stable radix sort, run-length voxel ids / counts, nearest-
`voxel_max` crop, min-corner shift.  The reference runs them in 6 numpy loader workers per GPU
(cfgs/s3dis/default.yaml:30-31), which cannot feed a step of ~10 ms; S3DIS.__getitem__ (dataset/s3dis/s3dis.py:122-144)
calls crop_pc once per cloud, and that call is what these replace.

Randomness: the reference draws from numpy's global RandomState (np.random.randint / choice / permutation).  Here the
draws come from a torch.Generator on the device, or are passed in (`rnd`, `init_idx`, `perm`) -- the tests pass the very
numbers the reference drew.  numpy's argsort is not stable, so WHICH point of a voxel the reference's mode-0 pick lands on
(and the order of equidistant points in the crop) is unspecified by the reference itself; the stable order is used here.

Batch-level calls: scannet_train_batch (ScanNet's training item, room by room after the transform), scannet_train_rooms /
ScanNetTrainFeed (the same item for the whole batch at once on csrc/room_input.hip, one read-back per batch),
s3dis_train_batch / S3DISTrainFeed (S3DIS's training item for a whole batch of raw rooms on csrc/room_input.hip, one read-back
per batch), the validation / whole-room testing items, and S3DISSphere's potential-picked spheres (SpherePotentials,
s3dis_sphere_batch, S3DISSphereFeed, sphere_projections on csrc/sphere.hip: no read-back per batch).
"""
import ctypes

import torch

from . import _lib
from .ops import _need_dtype, _need_gpu, _ptr, _stream


def _coord_f32_or_f64(coord):
    _need_gpu(coord)
    if coord.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"expected coord to be torch.float32 or torch.float64, got {coord.dtype}")
    return coord.contiguous()


def _voxel_tables_raw(coord, voxel_size):
    """the voxel tables at their allocated size (n) and the voxel count still on the device: no read-back"""
    coord = _coord_f32_or_f64(coord)
    n = coord.shape[0]
    dev = coord.device
    lib = _lib.load()
    key = torch.empty(n, dtype=torch.int64, device=dev)  # uint64 bit patterns
    idx_sort = torch.empty(n, dtype=torch.int32, device=dev)
    voxel_idx = torch.empty(n, dtype=torch.int32, device=dev)
    start = torch.empty(n + 1, dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    nvox = torch.empty(1, dtype=torch.int32, device=dev)
    wb = int(lib.amc3d_voxelize_workspace_bytes(n))
    work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        fn = lib.amc3d_voxelize_f64 if coord.dtype == torch.float64 else lib.amc3d_voxelize
        _lib.check(fn(n, _ptr(coord), ctypes.c_double(float(voxel_size)), _ptr(key), _ptr(idx_sort),
                                      _ptr(voxel_idx), _ptr(start), _ptr(count), _ptr(nvox), _ptr(work), wb, _stream(coord)),
                   "voxelize")
    return key, idx_sort, voxel_idx, start, count, nvox


def _voxel_tables(coord, voxel_size):
    key, idx_sort, voxel_idx, start, count, nvox = _voxel_tables_raw(coord, voxel_size)
    nv = int(nvox.item())  # the number of voxels sizes what follows: one read-back per cloud
    return key, idx_sort, voxel_idx, start[:nv + 1], count[:nv]


def voxelize(coord, voxel_size=0.05, hash_type='fnv', mode=0, rnd=None, generator=None):
    """coord (n,3) fp32 or fp64 on the GPU, already shifted to its min corner.
    mode 0 (train): idx_unique (nvox) int64 -- one point per voxel, the rnd[v] % count[v]-th of the voxel, rnd =
    randint(0, count.max(), nvox) drawn on the device (or given);  mode 1 (val): (idx_sort, voxel_idx, count) int64."""
    if hash_type != 'fnv':
        raise NotImplementedError("hash_type 'ravel': the loaders of the AMContrast3D configs use the default 'fnv'")
    key, idx_sort, voxel_idx, start, count = _voxel_tables(coord, voxel_size)
    if mode != 0:
        return idx_sort.long(), voxel_idx.long(), count.long()
    nv = count.shape[0]
    if rnd is None:
        rnd = torch.randint(0, int(count.max().item()), (nv,), device=coord.device, generator=generator, dtype=torch.int32)
    rnd = rnd.to(device=coord.device, dtype=torch.int32).contiguous()
    out = torch.empty(nv, dtype=torch.int32, device=coord.device)
    with torch.cuda.device(coord.device):
        _lib.check(_lib.load().amc3d_voxel_select(nv, _ptr(start), _ptr(count), _ptr(idx_sort), _ptr(rnd), _ptr(out),
                                                  _stream(coord)), "voxel_select")
    return out.long()


def crop_nearest(coord, init_idx, keep):
    """the `keep` points nearest to coord[init_idx], ascending distance -> (d2 (n), crop_idx (keep) int64); d2 has the
    coordinates' dtype (fp32 or fp64)"""
    d2, idx = _crop_nearest_i32(coord, init_idx, keep)
    return d2, idx.long()


def _crop_nearest_i32(coord, init_idx, keep):
    coord = _coord_f32_or_f64(coord)
    n = coord.shape[0]
    dev = coord.device
    lib = _lib.load()
    f64 = coord.dtype == torch.float64
    d2 = torch.empty(n, dtype=coord.dtype, device=dev)
    idx = torch.empty(int(keep), dtype=torch.int32, device=dev)
    wb = int(lib.amc3d_crop_nearest_f64_workspace_bytes(n) if f64 else lib.amc3d_crop_nearest_workspace_bytes(n))
    work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
    fn = lib.amc3d_crop_nearest_f64 if f64 else lib.amc3d_crop_nearest
    with torch.cuda.device(dev):
        _lib.check(fn(n, _ptr(coord), int(init_idx), int(keep), _ptr(d2), _ptr(idx), _ptr(work), wb, _stream(coord)),
                   "crop_nearest")
    return d2, idx


def crop_pc(coord, feat, label, split='train', voxel_size=0.04, voxel_max=None, downsample=True, variable=True,
            shuffle=True, generator=None, rnd=None, init_idx=None, perm=None, pad=None):
    """data_util.py:146-174 on GPU tensors: coord (n,3) fp32 or fp64 (the arithmetic is then float64 throughout, as numpy's on
    a float64 room), feat (n,c) or None, label (n[,1]) or None -> (coord fp32 shifted to its min corner, feat fp32, label
    int64), all on the GPU.  Draws that can be passed in: rnd (voxelize), init_idx (crop centre), pad (the
    np.random.choice(N, voxel_max - N) of the variable=False repetition), perm (the shuffle)."""
    if voxel_size and downsample:
        coord = coord - coord.min(0).values
        uniq = voxelize(coord, voxel_size, rnd=rnd, generator=generator)
        coord = coord[uniq]
        feat = feat[uniq] if feat is not None else None
        label = label[uniq] if label is not None else None
    if voxel_max is not None:
        crop_idx = None
        N = len(label)
        dev = coord.device
        if N >= voxel_max:
            if init_idx is None:
                init_idx = int(torch.randint(N, (1,), generator=generator, device=dev).item()) if 'train' in split else N // 2
            crop_idx = crop_nearest(coord.contiguous(), init_idx, voxel_max)[1]
        elif not variable:  # fill up by repetition (batched data of a fixed size)
            if pad is None:
                pad = torch.randint(N, (voxel_max - N,), generator=generator, device=dev)
            pad = pad.to(device=dev, dtype=torch.int64)
            crop_idx = torch.cat([torch.arange(N, device=dev), pad])
        if crop_idx is None:
            crop_idx = torch.arange(coord.shape[0], device=dev)
        if shuffle:
            if perm is None:
                perm = torch.randperm(len(crop_idx), generator=generator, device=dev)
            crop_idx = crop_idx[perm]
        coord = coord[crop_idx]
        feat = feat[crop_idx] if feat is not None else None
        label = label[crop_idx] if label is not None else None
    coord = coord - coord.min(0).values
    return coord.float(), feat.float() if feat is not None else None, label.long() if label is not None else None


def _voxel_select_i32(start, count, idx_sort, rnd):
    nv = count.shape[0]
    out = torch.empty(nv, dtype=torch.int32, device=count.device)
    rnd = rnd.to(device=count.device, dtype=torch.int32).contiguous()
    with torch.cuda.device(count.device):
        _lib.check(_lib.load().amc3d_voxel_select(nv, _ptr(start), _ptr(count), _ptr(idx_sort), _ptr(rnd), _ptr(out),
                                                  _stream(count)), "voxel_select")
    return out


def _is_chain(t):
    from .transforms import TransformChain
    return isinstance(t, TransformChain)


def _chain_draws(t, d, sizes, dev, generator):
    """the keys of a transforms.TransformChain out of the draws d; what is missing is drawn on the device"""
    own = {k: v for k, v in d.items() if k in t.spec() or k.endswith(".R")}
    given_R = {k.split(".", 1)[0] for k, v in own.items() if k.endswith(".R") and v is not None}
    if any(k not in own and not (k.split(".", 1)[0] in given_R and k.split(".", 1)[1] in ("angle", "theta", "order"))
           for k in t.spec()):
        for k, v in t.draw(sizes, dev, generator).items():
            own.setdefault(k, v)
    return own


def _chain_rooms(t, coord, feat, off_t, sizes, d):
    """a TransformChain on whole raw ScanNet rooms: colours (feat + 1) * 127.5 first; the positions float64 for crop_pc (a chain
    that leaves them float32 is cast, exactly)"""
    out = t({"pos": coord, "x": feat, "offsets": off_t, "sizes": sizes}, draws=d, scannet_colour=True, want_heights=False)
    return (out["pos"] if out["pos"].dtype == torch.float64 else out["pos"].double()), out["x"]


def scannet_train_batch(rooms, transform, voxel_size=0.02, voxel_max=64000, variable=False, generator=None, draws=None,
                        gravity_dim=2):
    """ScanNet.__getitem__ for training (dataset/scannetv2/scannet.py:140-176) plus the default collate, for a batch of raw
    rooms on the GPU: colours (feat + 1) * 127.5, `transform` (augment.ScanNetTrainAugment) on the whole room, crop_pc in
    float64 (min-corner shift, voxelize mode 0, nearest-voxel_max crop or, with variable=False, padding by repetition,
    shuffle, min-corner shift, cast) and heights.

    rooms: list of (coord (n,3) fp32, feat (n,3) fp32 in [-1, 1], label (n,) or (n,1)) GPU tensors, as torch.load of a
    ScanNet .pth gives them (labels pass through unchanged, -100 included).  Returns {pos (B,N,3) fp32, x (B,N,3) fp32,
    heights (B,N,1) fp32, y (B,N) int64}, what DataLoader(ScanNet(split='train')) yields; every room must come out with the
    same N (always so with variable=False).

    Random numbers come from `generator` (a torch.Generator on the rooms' device, or the default one) or from `draws`: a
    dict with the transform's keys (see ScanNetTrainAugment.draw; "R" for given rotation matrices) and per-room lists
    "rnd" (voxelize's randint(0, count.max(), nvox)), "init_idx", "pad", "perm" (entries may be None).
    Host synchronisation: one read-back per room (its voxel count, which sizes everything after it) and up to two per
    batch (the room-level draws -- the rotation matrix is formed on the host -- and the crop centres' uniforms)."""
    B = len(rooms)
    if B == 0:
        raise ValueError("scannet_train_batch: no rooms")
    dev = rooms[0][0].device
    for c, f, l in rooms:
        _need_gpu(c, f, l)
        _need_dtype(torch.float32, coord=c, feat=f)
        if c.dim() != 2 or c.shape[1] != 3 or f.shape != c.shape or l.numel() != c.shape[0] or c.shape[0] == 0:
            raise ValueError("scannet_train_batch: every room needs coord (n,3), feat (n,3), label (n,) with n > 0")
    d = dict(draws or {})
    sizes = [int(c.shape[0]) for c, _, _ in rooms]
    keys = ("scale", "mirror_u", "contrast_u", "blend", "drop_u")
    if not _is_chain(transform) and (any(k not in d for k in keys) or ("angle" not in d and "R" not in d)):
        for k, v in transform.draw(B, generator, dev).items():
            d.setdefault(k, v)
    per_room = {k: list(d.get(k) or [None] * B) for k in ("rnd", "init_idx", "pad", "perm")}
    if any(len(v) != B for v in per_room.values()):
        raise ValueError("scannet_train_batch: per-room draws need one entry per room")
    offsets = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0).to(dev)
    if _is_chain(transform):  # a transforms.TransformChain: any configured list, its draws under its own keys
        pos64, x = _chain_rooms(transform, torch.cat([c for c, _, _ in rooms]), torch.cat([f for _, f, _ in rooms]), offsets, sizes,
                                _chain_draws(transform, d, sizes, dev, generator))
    else:
        pos64, x, _ = transform(torch.cat([c for c, _, _ in rooms]), torch.cat([f for _, f, _ in rooms]), offsets, draws=d,
                                generator=generator)
    u_init = None
    plans = []
    beg = 0
    for b in range(B):
        p = pos64[beg:beg + sizes[b]]
        p = p - p.min(0).values  # crop_pc's `coord -= coord.min(0)`, float64
        key, idx_sort, voxel_idx, start, count = _voxel_tables(p, voxel_size)
        N = count.shape[0]  # the read-back of this room
        rnd = per_room["rnd"][b]
        if rnd is None:  # randint(0, count.max(), nvox) without reading count.max() back
            rnd = (torch.rand(N, dtype=torch.float64, device=dev, generator=generator) * count.max().double()).int()
        else:
            rnd = torch.as_tensor(rnd).to(dev)
            if rnd.shape != (N,) or bool((rnd < 0).any()):
                raise ValueError(f"scannet_train_batch: room {b}: rnd must hold {N} non-negative draws")
        sel = _voxel_select_i32(start, count, idx_sort, rnd)
        crop = None
        if N >= voxel_max:
            init = per_room["init_idx"][b]
            if init is None:
                if u_init is None:
                    u_init = torch.rand(B, dtype=torch.float64, device=dev, generator=generator).cpu()
                init = min(int(float(u_init[b]) * N), N - 1)
            init = int(init)
            if not 0 <= init < N:
                raise ValueError(f"scannet_train_batch: room {b}: init_idx {init} out of range")
            crop = _crop_nearest_i32(p[sel.long()], init, voxel_max)[1]
        elif not variable:
            pad = per_room["pad"][b]
            pad = (torch.randint(N, (voxel_max - N,), generator=generator, device=dev) if pad is None
                   else torch.as_tensor(pad).to(dev))
            if pad.shape != (voxel_max - N,) or (pad.numel() and bool(((pad < 0) | (pad >= N)).any())):
                raise ValueError(f"scannet_train_batch: room {b}: pad must hold {voxel_max - N} indices below {N}")
            crop = torch.cat([torch.arange(N, device=dev), pad.long()]).int()
        n_out = int(crop.shape[0]) if crop is not None else N
        perm = per_room["perm"][b]
        perm = torch.randperm(n_out, generator=generator, device=dev) if perm is None else torch.as_tensor(perm).to(dev)
        if perm.shape != (n_out,) or bool(((perm < 0) | (perm >= n_out)).any()):
            raise ValueError(f"scannet_train_batch: room {b}: perm must be a permutation of {n_out}")
        plans.append((p, sel, crop, perm.int().contiguous(), n_out, beg))
        beg += sizes[b]
    n_out = plans[0][4]
    if any(pl[4] != n_out for pl in plans):
        raise ValueError("scannet_train_batch: the rooms came out with different sizes %s (variable=True); the collate "
                         "stacks them" % [pl[4] for pl in plans])
    out = {"pos": torch.empty(B, n_out, 3, dtype=torch.float32, device=dev),
           "x": torch.empty(B, n_out, 3, dtype=torch.float32, device=dev),
           "heights": torch.empty(B, n_out, 1, dtype=torch.float32, device=dev),
           "y": torch.empty(B, n_out, dtype=torch.int64, device=dev)}
    lib = _lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    with torch.cuda.device(dev):
        for b, (p, sel, crop, perm, _, beg) in enumerate(plans):
            y = rooms[b][2].reshape(-1).to(torch.int64).contiguous()
            xr = x[beg:beg + sizes[b]]
            _lib.check(lib.amc3d_scannet_crop_tail(n_out, int(gravity_dim), P(p), P(xr), P(y), P(sel), P(crop), P(perm),
                                                   P(out["pos"][b]), P(out["x"][b]), P(out["heights"][b]), P(out["y"][b]),
                                                   _stream(p)), "scannet_crop_tail")
    return out


_SEG_KINDS = {"pos": 0, "x": 1, "heights": 2}
SCANNET_COLOR_MEAN = (0.46259782, 0.46253258, 0.46253258)  # dataset/scannetv2/scannet.py:73-74
SCANNET_COLOR_STD = (0.693565, 0.6852543, 0.68061745)


_colour_cache = {}


def _colour_constants(mean, std, dev, who="part_batch"):
    """color_mean / color_std on the device, uploaded once per value and device (part_batch runs once per model call)"""
    key = (mean, std, str(dev))
    if key not in _colour_cache:
        if len(mean) != 3 or len(std) != 3:
            raise ValueError(f"{who}: color_mean and color_std hold three values")
        _colour_cache[key] = (torch.tensor(mean, dtype=torch.float32).to(dev), torch.tensor(std, dtype=torch.float32).to(dev))
    return _colour_cache[key]


def _room_tables(coord, voxel_size, tables, who):
    """the voxel tables of a room, from the device's voxelisation or from `tables`, with nvox and count.max() (one read-back)"""
    _need_gpu(coord)
    dev = coord.device
    n = coord.shape[0]
    if tables is None:
        _, idx_sort, voxel_idx, start, count, nvox = _voxel_tables_raw(coord, voxel_size)
        live = torch.arange(n, device=dev, dtype=torch.int32) < nvox
        nv, P = torch.cat([nvox, torch.where(live, count, 0).max().reshape(1)]).tolist()
        start, count = start[:nv + 1], count[:nv]
    else:
        as_i32 = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.int32).contiguous()  # noqa: E731
        idx_sort, count = as_i32(tables["idx_sort"]), as_i32(tables["count"])
        nv = count.shape[0]
        ends = count.cumsum(0, dtype=torch.int32)
        start = as_i32(tables["start"]) if tables.get("start") is not None else torch.cat([ends.new_zeros(1), ends])
        voxel_idx = (as_i32(tables["voxel_idx"]) if tables.get("voxel_idx") is not None else
                     torch.repeat_interleave(torch.arange(nv, device=dev, dtype=torch.int32), count.long()))
        P = int(count.max().item())
        if idx_sort.shape != (n,) or voxel_idx.shape != (n,) or start.shape != (nv + 1,):
            raise ValueError(f"{who}: tables need idx_sort (n), voxel_idx (n), start (nvox+1), count (nvox)")
    return idx_sort, voxel_idx, start, count, nv, P


def room_parts(coord, voxel_size, perm=None, generator=None, tables=None):
    """The split of a whole room into sub-clouds of one point per voxel (`load_data`, main_AA.py:95-113, test_mode
    'multi_voxel') on the device.  coord (n,3) fp32 or fp64 on the GPU, already shifted to its min corner.

    Returns a dict: idx_sort (n), voxel_idx (n), start (nvox+1), count (nvox) int32 (the voxel tables), parts (P,nvox) int32
    with P = count.max() -- part i holds the (i mod count)-th point of every voxel -- and where (P,nvox) int32, the position
    of voxel v's point in part i.  perm (P,nvox): row i is the order of part i's voxels, the stand-in for the reference's
    np.random.shuffle(idx_part); None draws the rows on the device from `generator`.  tables: given idx_sort / count
    [/ start / voxel_idx] instead of a voxelisation (numpy's argsort is unstable, so the order inside a voxel is the
    reference's to choose; the tests pass its own).  One read-back: nvox and count.max() together."""
    idx_sort, voxel_idx, start, count, nv, P = _room_tables(coord, voxel_size, tables, "room_parts")
    dev = coord.device
    n = coord.shape[0]
    if perm is None:
        perm = torch.rand(P, nv, device=dev, generator=generator).argsort(dim=1).int()
    else:
        perm = torch.as_tensor(perm).to(device=dev, dtype=torch.int32).contiguous()
        if perm.shape != (P, nv) or not bool((perm.sort(dim=1).values == torch.arange(nv, device=dev, dtype=torch.int32)).all()):
            raise ValueError(f"room_parts: perm must hold {P} permutations of the {nv} voxel ids")
    parts = torch.empty(P, nv, dtype=torch.int32, device=dev)
    where = torch.empty(P, nv, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().amc3d_room_parts(P, nv, n, _ptr(start), _ptr(count), _ptr(idx_sort), _ptr(perm), _ptr(parts),
                                                _ptr(where), _stream(coord)), "room_parts")
    return {"idx_sort": idx_sort, "voxel_idx": voxel_idx, "start": start, "count": count, "parts": parts, "where": where}


def _part_batch(who, idx, coord, colour, label, mode, color_mean, color_std, gravity_dim, feature_keys, centre=None, s3dis=False):
    """the body of part_batch and s3dis_part_batch after their dtype checks: the refusals, the outputs, the workspace and the
    call of amc3d_<who>; `s3dis` adds what only that entry point takes: coord's dtype, a given centre, the centre output"""
    if mode not in ("test", "val"):
        raise ValueError(f"{who}: mode {mode!r} (test or val)")
    f64 = coord.dtype == torch.float64
    if mode == "val" and f64:
        raise ValueError(f"{who}: the val item is float32 (S3DIS casts the room when it loads it)")
    keys = [k.strip() for k in feature_keys.split(",")]
    if not 1 <= len(keys) <= 3 or any(k not in _SEG_KINDS for k in keys):
        raise ValueError(f"{who}: feature_keys {feature_keys!r}: up to three of pos, x, heights")
    if idx.dim() != 2 or coord.dim() != 2 or coord.shape[1] != 3 or colour.shape != coord.shape:
        raise ValueError(f"{who}: idx (R,n), coord (N,3), {'colour' if s3dis else 'feat'} (N,3)")
    if s3dis and gravity_dim not in (0, 1, 2):
        raise ValueError(f"{who}: gravity_dim is 0, 1 or 2")
    dev = coord.device
    idx, coord, colour = idx.contiguous(), coord.contiguous(), colour.contiguous()
    R, n = idx.shape
    N = coord.shape[0]
    cx = sum(1 if k == "heights" else 3 for k in keys)
    out = {"pos": torch.empty(R, n, 3, dtype=torch.float32, device=dev),
           "x": torch.empty(R, cx, n, dtype=torch.float32, device=dev),
           "heights": torch.empty(R, n, 1, dtype=torch.float32, device=dev)}
    y = None
    if label is not None:
        _need_gpu(label)
        label = label.reshape(-1).to(torch.int64).contiguous()
        if label.shape[0] != N:
            raise ValueError(f"{who}: one label per room point")
        y = out["y"] = torch.empty(R, n, dtype=torch.int64, device=dev)
    if centre is not None:
        _need_gpu(centre)
        _need_dtype(torch.float32, centre=centre)
        if centre.shape != (R, 3):
            raise ValueError(f"{who}: centre (R,3)")
        centre = centre.contiguous()
    lib = _lib.load()
    wb = int(getattr(lib, f"amc3d_{who}_workspace_bytes")(R))
    work = torch.empty(max(wb, 8) // 8, dtype=torch.float64, device=dev)
    kinds = (ctypes.c_int * 3)(*([_SEG_KINDS[k] for k in keys] + [0] * (3 - len(keys))))
    mean, std = _colour_constants(tuple(float(v) for v in color_mean), tuple(float(v) for v in color_std), dev, who)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    ins = [int(gravity_dim), len(keys), ctypes.cast(kinds, ctypes.c_void_p), P(idx), P(coord), P(colour), P(label), P(mean), P(std)]
    outs = [P(out["pos"]), P(out["x"]), P(out["heights"]), P(y)]
    if s3dis:
        out["centre"] = torch.empty(R, 3, dtype=torch.float32, device=dev)
        ins = [int(f64)] + ins + [P(centre)]
        outs.append(P(out["centre"]))
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, f"amc3d_{who}")(R, n, N, 1 if mode == "val" else 0, *ins, *outs, P(work), wb, _stream(coord)), who)
    return out


def part_batch(idx, coord, feat, label=None, mode="test", color_mean=SCANNET_COLOR_MEAN, color_std=SCANNET_COLOR_STD,
               gravity_dim=2, feature_keys="pos,x,heights"):
    """Sub-clouds of a room as a model batch (csrc/room_eval.hip).  idx (R,n) int32 rows of point indices into coord (N,3)
    fp32, feat (N,3) fp32 in [-1, 1] (the .pth colours), label (N) int64 or None.  Per row: pos = coordinate minus the
    row's minimum corner; colours `mode` 'test' clip((f + 1) / 2, 0, 1) (`load_data`) or 'val' (f + 1) * 127.5
    (ScanNet.__getitem__), then NumpyChromaticNormalize per row; heights = pos[..., gravity_dim]; x assembled channel-major
    from `feature_keys` (get_features_by_keys).  Returns {pos (R,n,3), x (R,Cx,n), heights (R,n,1)[, y (R,n) int64]}."""
    _need_gpu(idx, coord, feat)
    _need_dtype(torch.int32, idx=idx)
    _need_dtype(torch.float32, coord=coord, feat=feat)
    return _part_batch("part_batch", idx, coord, feat, label, mode, color_mean, color_std, gravity_dim, feature_keys)


def scannet_val_cloud(room, voxel_size=0.02, rnd=None, generator=None, color_mean=SCANNET_COLOR_MEAN,
                      color_std=SCANNET_COLOR_STD, gravity_dim=2, feature_keys="pos,x,heights"):
    """The val item of ScanNet.__getitem__ with `presample: True`, `voxel_max: null`, `val: [NumpyChromaticNormalize]`
    (dataset/scannetv2/scannet.py:114-176): crop_pc at load time (min-corner shift, voxelize mode 0, min-corner shift; no
    crop and no shuffle without voxel_max), then colours (f + 1) * 127.5, the normalisation and heights.
    room: (coord (n,3) fp32, feat (n,3) fp32 in [-1, 1], label (n[,1])) GPU tensors.  rnd: voxelize's randint(0, count.max(),
    nvox), drawn from `generator` when None.  Returns {pos (1,n,3), x (1,Cx,n), heights (1,n,1), y (1,n)}: one batch of
    evaluate.validate_boundary_inner."""
    coord, feat, label = room
    _need_gpu(coord, feat, label)
    _need_dtype(torch.float32, coord=coord, feat=feat)
    coord = coord - coord.min(0).values
    sel = voxelize(coord, voxel_size, rnd=rnd, generator=generator).int()
    return part_batch(sel.view(1, -1), coord, feat, label, "val", color_mean, color_std, gravity_dim, feature_keys)


S3DIS_COLOR_MEAN = (0.5136457, 0.49523646, 0.44921124)  # transforms/point_transformer_gpu.py:398-399 (ChromaticNormalize)
S3DIS_COLOR_STD = (0.18308958, 0.18415008, 0.19252081)


def s3dis_part_batch(idx, coord, colour, label=None, mode="test", color_mean=S3DIS_COLOR_MEAN, color_std=S3DIS_COLOR_STD,
                     gravity_dim=2, feature_keys="x,heights", centre=None):
    """Sub-clouds of an S3DIS room as a model batch with the config's evaluation transforms `[PointsToTensor,
    PointCloudXYZAlign, ChromaticNormalize]` (csrc/room_eval.hip).  idx (R,n) int32 rows of point indices into coord (N,3),
    fp32 or fp64 and already at the room's minimum corner, colour (N,3) raw 0..255 in coord's dtype, label (N) or None.
    mode 'test' (`load_data` + the sub-cloud loop, main.py:73, 563-576): colour clip(f / 255, 0, 1) and coordinates minus the
    row's minimum corner, both in coord's dtype, then float32; 'val' (S3DIS.__getitem__, fp32 only): both as they are.
    heights = that coordinate's gravity column, before the alignment; pos = it minus the row's centre, then the gravity column
    minus its minimum; colours / 255 if the row's maximum exceeds 1, then (x - color_mean) / color_std; x assembled
    channel-major from `feature_keys` (get_features_by_keys).
    centre: the reference's torch.mean sums in an order that depends on the host's vector width and thread count, so its last
    bit is not specified; here it is the fp64 column sum in a fixed order, divided by n and rounded once to float32 (the same
    bits on every run, within 2 ulp of torch.mean on the fixture's sub-clouds).  A given centre (R,3) fp32 replaces it.
    Returns {pos (R,n,3), x (R,Cx,n), heights (R,n,1)[, y (R,n) int64], centre (R,3)}."""
    _need_gpu(idx, coord, colour)
    _need_dtype(torch.int32, idx=idx)
    if coord.dtype not in (torch.float32, torch.float64) or colour.dtype != coord.dtype:
        raise RuntimeError(f"s3dis_part_batch: coord and colour are both float32 or both float64, got {coord.dtype} and {colour.dtype}")
    return _part_batch("s3dis_part_batch", idx, coord, colour, label, mode, color_mean, color_std, gravity_dim, feature_keys,
                       centre, s3dis=True)


def room_representatives(coord, voxel_size, rnd=None, perm=None, generator=None, tables=None):
    """The single sub-cloud of `test_mode: nearest_neighbor` (`load_data`, main.py:96-104) on the device: one point of every
    voxel, the (rnd[v] % count[v])-th, in the order of `perm`.  coord (n,3) fp32 or fp64 on the GPU, already shifted to its
    min corner.  rnd (nvox): the reference's np.random.randint(0, count.max(), count.size); perm (nvox): its
    np.random.permutation; both drawn on the device from `generator` when None.  tables: as in room_parts.
    Returns the voxel tables idx_sort (n), voxel_idx (n), start (nvox+1), count (nvox) plus parts (1,nvox) and where (1,nvox),
    the inverse of perm (the reference's reverse_idx_part), all int32: what s3dis_part_batch and ops.expand_parts take."""
    idx_sort, voxel_idx, start, count, nv, P = _room_tables(coord, voxel_size, tables, "room_representatives")
    dev = coord.device
    n = coord.shape[0]
    if rnd is None:
        rnd = torch.randint(0, max(P, 1), (nv,), device=dev, generator=generator, dtype=torch.int32)
    else:
        rnd = torch.as_tensor(rnd).to(device=dev, dtype=torch.int32).contiguous()
        if rnd.shape != (nv,) or (nv and int(rnd.min()) < 0):
            raise ValueError(f"room_representatives: rnd holds one draw >= 0 for each of the {nv} voxels")
    if perm is None:
        perm = torch.rand(nv, device=dev, generator=generator).argsort().int()
    else:
        perm = torch.as_tensor(perm).to(device=dev, dtype=torch.int32).contiguous()
        if perm.shape != (nv,) or not bool((perm.sort().values == torch.arange(nv, device=dev, dtype=torch.int32)).all()):
            raise ValueError(f"room_representatives: perm must be a permutation of the {nv} voxel ids")
    parts = torch.empty(1, nv, dtype=torch.int32, device=dev)
    where = torch.empty(1, nv, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().amc3d_room_representatives(nv, n, _ptr(start), _ptr(count), _ptr(idx_sort), _ptr(rnd), _ptr(perm),
                                                          _ptr(parts), _ptr(where), _stream(coord)), "room_representatives")
    return {"idx_sort": idx_sort, "voxel_idx": voxel_idx, "start": start, "count": count, "parts": parts, "where": where}


def s3dis_val_cloud(cdata, voxel_size=0.04, rnd=None, generator=None, color_mean=S3DIS_COLOR_MEAN, color_std=S3DIS_COLOR_STD,
                    gravity_dim=2, feature_keys="x,heights", centre=None, tables=None):
    """The val item of S3DIS.__getitem__ with `presample: True`, `voxel_max: null`, `val: [PointsToTensor, PointCloudXYZAlign,
    ChromaticNormalize]` (dataset/s3dis/s3dis.py:94-144): the raw room cast to float32, shifted to its minimum corner,
    voxelize mode 0 (one random point per voxel), then the three transforms on the selected points and heights = the
    gravity column before the alignment.  There is no second min-corner shift, and the colours are still 0..255, so
    ChromaticNormalize's / 255 is the live branch.
    cdata (n,7) GPU tensor, fp32 or fp64: xyz, rgb 0..255, label.  rnd: voxelize's randint(0, count.max(), nvox), drawn from
    `generator` when None.  centre (1,3): see s3dis_part_batch.  tables: idx_sort / count [/ start] of the reference's own
    voxelisation (its unstable sort chooses the order inside a voxel; the tests pass it).
    Returns {pos (1,n,3), x (1,Cx,n), heights (1,n,1), y (1,n), centre (1,3)}: one batch of evaluate.validate_boundary_inner."""
    _need_gpu(cdata)
    if cdata.dim() != 2 or cdata.shape[1] != 7:
        raise ValueError("s3dis_val_cloud: cdata (n,7): xyz, rgb, label")
    cdata = cdata.float()
    coord = cdata[:, :3] - cdata[:, :3].min(0).values
    colour, label = cdata[:, 3:6].contiguous(), cdata[:, 6].long()
    if tables is None:
        sel = voxelize(coord, voxel_size, rnd=rnd, generator=generator).int()
    else:
        idx_sort, _, start, count, nv, P = _room_tables(coord, voxel_size, tables, "s3dis_val_cloud")
        if rnd is None:
            rnd = torch.randint(0, max(P, 1), (nv,), device=coord.device, generator=generator, dtype=torch.int32)
        rnd = torch.as_tensor(rnd).to(device=coord.device, dtype=torch.int32).contiguous()
        sel = torch.empty(nv, dtype=torch.int32, device=coord.device)
        with torch.cuda.device(coord.device):
            _lib.check(_lib.load().amc3d_voxel_select(nv, _ptr(start), _ptr(count), _ptr(idx_sort), _ptr(rnd), _ptr(sel),
                                                      _stream(coord)), "voxel_select")
    return s3dis_part_batch(sel.view(1, -1), coord, colour, label, "val", color_mean, color_std, gravity_dim, feature_keys,
                            centre)


def _upload(values, dtype, dev):
    """a small host table on the device without a blocking copy: pinned staging, asynchronous on the current stream"""
    return torch.tensor(values, dtype=dtype).pin_memory().to(dev, non_blocking=True)


_S3DIS_TRANSFORM_KEYS = {"contrast": (), "blend": (), "scale_u": (3,), "theta": (3,), "drop": ()}


def _s3dis_transform_draws(t, B, N, dev, generator):
    """S3DISTrainAugment.draw -- the same draws in the same order -- without its blocking upload of the angle bounds (a
    pageable host-to-device copy waits for everything queued on the stream: here, the whole voxelisation)"""
    import math
    r = lambda *s: torch.rand(*s, device=dev, generator=generator)  # noqa: E731
    d = {"contrast": r(B) < t.contrast_p,
         "blend": r(B) if t.blend_factor is None else torch.full((B,), float(t.blend_factor), device=dev),
         "scale_u": r(B, 3)}
    u = r(B, 3).double() * 2 - 1
    d["theta"] = torch.stack([u[:, j] * (t.angle[j] * math.pi) for j in range(3)], 1)
    d["noise"] = torch.randn(B, N, 3, device=dev, generator=generator)
    d["drop"] = r(B) < t.color_drop
    return d


def _s3dis_augment(t, pos, colour, d):
    """S3DISTrainAugment.__call__ on given draws -- the same records for the same amc3d_augment_clouds, bit for bit -- with the
    scale bounds as host scalars instead of uploaded tensors: no blocking copy"""
    B, N, dev = pos.shape[0], pos.shape[1], pos.device
    lo, hi = torch.tensor(t.scale[0], dtype=torch.float32), torch.tensor(t.scale[1], dtype=torch.float32)
    scale = d["scale_u"].float() * float(hi - lo) + float(lo)  # point_transformer_gpu.py:151-152, in float32
    th = d["theta"].double()
    c, s = torch.cos(th), torch.sin(th)
    one, zero = torch.ones(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)
    rx = torch.stack([one, zero, zero, zero, c[:, 0], -s[:, 0], zero, s[:, 0], c[:, 0]], 1).view(B, 3, 3)
    ry = torch.stack([c[:, 1], zero, s[:, 1], zero, one, zero, -s[:, 1], zero, c[:, 1]], 1).view(B, 3, 3)
    rz = torch.stack([c[:, 2], -s[:, 2], zero, s[:, 2], c[:, 2], zero, zero, zero, one], 1).view(B, 3, 3)
    par = torch.zeros(B, 24, dtype=torch.float32, device=dev)
    par[:, 0] = d["contrast"].float()
    par[:, 1] = d["blend"].float()
    par[:, 2:5] = scale
    par[:, 5:14] = (rx @ ry @ rz).float().reshape(B, 9)
    par[:, 14] = d["drop"].float()
    noise = d["noise"].to(torch.float32).contiguous()
    mean, std = _colour_constants(tuple(float(v) for v in t.color_mean), tuple(float(v) for v in t.color_std), dev,
                                  "s3dis_train_batch")
    pos_out, x_out = torch.empty_like(pos), torch.empty_like(colour)
    heights = torch.empty(B, N, 1, dtype=torch.float32, device=dev)
    lib = _lib.load()
    wb = int(lib.amc3d_augment_workspace_bytes(B))
    work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.amc3d_augment_clouds(B, N, t.g, t.sigma, t.clip, _ptr(pos), _ptr(colour), _ptr(noise), _ptr(par), _ptr(mean),
                                            _ptr(std), _ptr(pos_out), _ptr(x_out), _ptr(heights), _ptr(work), wb, _stream(pos)),
                   "augment_clouds")
    return pos_out, x_out, heights


def _opt(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _check_rooms_args(who, voxel_size, voxel_max, gravity_dim, total, hint=""):
    if voxel_max is None or int(voxel_max) <= 0:
        raise ValueError(f"{who}: voxel_max is the size of a training cloud{hint}")
    if gravity_dim not in (0, 1, 2) or not float(voxel_size) > 0:
        raise ValueError(f"{who}: gravity_dim is 0, 1 or 2 and voxel_size is positive")
    if total >= 2 ** 31:
        raise ValueError(f"{who}: {total} points in one batch (at most 2^31 - 1)")


def _pop_per_room(d, B, who):
    """the per-room lists "rnd", "init_idx", "pad", "perm" taken out of the draws d (an entry or a whole list may be None)"""
    per_room = {}
    for k in ("rnd", "init_idx", "pad", "perm"):
        v = d.pop(k, None)
        per_room[k] = list(v) if v is not None else [None] * B
        if len(per_room[k]) != B:
            raise ValueError(f"{who}: per-room draws need one entry per room")
    return per_room


class _RoomVoxels:
    """the voxel tables of a ragged batch of B rooms (csrc/room_input.hip), coordinates of `dtype`: allocated here and filled by
    amc3d_<which>_voxelize_rooms, whose arguments between the sizes and voxel_size are `source`"""

    def __init__(self, which, dtype, B, total, voxel_size, dev, source):
        self.which, self.dtype, self.B, self.dev = which, dtype, B, dev
        self.lib = lib = _lib.load()
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.coord = torch.empty(total, 3, dtype=dtype, device=dev)
        key = torch.empty(total, dtype=torch.int64, device=dev)  # uint64 bit patterns
        self.idx_sort = torch.empty(total, dtype=torch.int32, device=dev)
        self.start = torch.empty(total + 1, dtype=torch.int32, device=dev)
        self.count = torch.empty(total, dtype=torch.int32, device=dev)
        small = torch.empty(2 * B + 1, dtype=torch.int32, device=dev)
        self.vbase, self.cmax = small[:B + 1], small[B + 1:]
        corner = torch.empty(B, 3, dtype=dtype, device=dev)
        wb = int(getattr(lib, f"amc3d_{which}_voxelize_workspace_bytes")(B, total))
        work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(getattr(lib, f"amc3d_{which}_voxelize_rooms")(
                B, total, *source, ctypes.c_double(float(voxel_size)), _opt(self.coord), _opt(key), _opt(self.idx_sort),
                _opt(self.start), _opt(self.count), _opt(self.vbase), _opt(self.cmax), _opt(corner), _opt(work), wb, self.stream),
                f"{which}_voxelize_rooms")

    def read_back(self, voxel_max, variable, who):
        """the batch's one read-back: the voxel counts size everything after the voxelisation"""
        B = self.B
        self.vb = vb = self.vbase.tolist()
        self.nv = nv = [vb[b + 1] - vb[b] for b in range(B)]
        self.nvt = vb[B]
        outs = [voxel_max if (n >= voxel_max or not variable) else n for n in nv]
        self.n_out = outs[0]
        if any(n != self.n_out for n in outs):
            raise ValueError(f"{who}: the rooms came out with different sizes {outs} (variable=True); the collate stacks them")
        self.cropped = [n >= voxel_max for n in nv]
        self.padded = [n < self.n_out for n in nv]

    def nv_column(self):
        return (self.vbase[1:] - self.vbase[:-1]).view(self.B, 1)

    def given(self, per_room, pad_t, perm_t, shuffle, who):
        """validates the per-room draws that were passed in and scatters them into the batch's tables -> rnd_t (-1 where the
        device draws), init_t, pad_t, perm_t.  pad_t / perm_t: what the caller drew for the rooms without given ones, or None"""
        B, dev, vb, nv, n_out = self.B, self.dev, self.vb, self.nv, self.n_out
        given = lambda v: torch.as_tensor(v).to(dev)  # noqa: E731
        rnd_t = init_t = None
        if any(r is not None for r in per_room["rnd"]):  # voxelize's randint(0, count.max(), nvox)
            rnd_t = torch.full((self.nvt,), -1, dtype=torch.int32, device=dev)
            for b, r in enumerate(per_room["rnd"]):
                if r is not None:
                    r = given(r)
                    if r.shape != (nv[b],) or r.is_floating_point() or bool((r < 0).any()):
                        raise ValueError(f"{who}: room {b}: rnd must hold {nv[b]} non-negative draws")
                    rnd_t[vb[b]:vb[b + 1]] = r
        if any(self.cropped):  # crop_pc's randint(N)
            inits = []
            for b, v in enumerate(per_room["init_idx"]):
                v = -1 if (v is None or not self.cropped[b]) else int(v)
                if per_room["init_idx"][b] is not None and self.cropped[b] and not 0 <= v < nv[b]:
                    raise ValueError(f"{who}: room {b}: init_idx {v} out of range")
                inits.append(v)
            if any(v >= 0 for v in inits):
                init_t = _upload(inits, torch.int32, dev)
        if any(self.padded):  # its np.random.choice(N, voxel_max - N)
            if pad_t is None:
                pad_t = torch.zeros(B, n_out, dtype=torch.int32, device=dev)
            for b, v in enumerate(per_room["pad"]):
                if v is not None and self.padded[b]:
                    v = given(v)
                    if v.shape != (n_out - nv[b],) or v.is_floating_point() or bool(((v < 0) | (v >= nv[b])).any()):
                        raise ValueError(f"{who}: room {b}: pad must hold {n_out - nv[b]} indices below {nv[b]}")
                    pad_t[b, nv[b]:] = v
        if shuffle:  # its permutation
            if perm_t is None:
                perm_t = torch.empty(B, n_out, dtype=torch.int32, device=dev)
            for b, v in enumerate(per_room["perm"]):
                if v is not None:
                    v = given(v)
                    if (v.shape != (n_out,) or v.is_floating_point()
                            or not bool((v.sort().values == torch.arange(n_out, device=dev)).all())):
                        raise ValueError(f"{who}: room {b}: perm must be a permutation of {n_out}")
                    perm_t[b] = v
        return rnd_t, init_t, pad_t, perm_t

    def select_crop(self, voxel_max, rnd_t, rnd_u, init_t, init_u):
        """one point per voxel and, where a room has voxel_max voxels or more, its crop order -> sel, order (or None)"""
        dev, nvt, any_crop = self.dev, self.nvt, any(self.cropped)
        sel = torch.empty(max(nvt, 1), dtype=torch.int32, device=dev)
        d2 = order = work = None
        wb = 0
        if any_crop:
            d2 = torch.empty(nvt, dtype=self.dtype, device=dev)
            order = torch.empty(nvt, dtype=torch.int32, device=dev)
            wb = int(getattr(self.lib, f"amc3d_{self.which}_crop_workspace_bytes")(nvt))
            work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(getattr(self.lib, f"amc3d_{self.which}_select_crop")(
                self.B, nvt, voxel_max, int(any_crop), _opt(self.coord), _opt(self.idx_sort), _opt(self.start), _opt(self.count),
                _opt(self.vbase), _opt(self.cmax), _opt(rnd_t), _opt(rnd_u), _opt(init_t), _opt(init_u), _opt(sel), _opt(d2),
                _opt(order), _opt(work), wb, self.stream), f"{self.which}_select_crop")
        return sel, order


def _s3dis_batch(raw, src, sizes, transform, voxel_size, voxel_max, variable, shuffle, generator, draws, gravity_dim):
    """s3dis_train_batch on rooms that are row ranges [src[b], src[b] + sizes[b]) of one (rows,7) GPU array"""
    who = "s3dis_train_batch"
    B, dev, total = len(sizes), raw.device, sum(sizes)
    _check_rooms_args(who, voxel_size, voxel_max, gravity_dim, total, " (validation goes through s3dis_val_cloud)")
    voxel_max = int(voxel_max)
    f64 = int(raw.dtype == torch.float64)
    offsets = [0]
    for n in sizes:
        offsets.append(offsets[-1] + n)
    table = _upload(list(src) + offsets, torch.int64, dev)
    src_t, off_t = table[:B], table[B:]
    v = _RoomVoxels("s3dis", torch.float32, B, total, voxel_size, dev, (f64, _opt(raw), _opt(src_t), _opt(off_t)))
    v.read_back(voxel_max, variable, who)
    n_out = v.n_out

    d = dict(draws or {})
    per_room = _pop_per_room(d, B, who)
    # the device's own draws, at the sizes the voxel counts give: voxelize's randint, crop_pc's randint(N), its
    # np.random.choice(N, voxel_max - N) and its permutation, in this order
    rnd_u = init_u = pad_t = perm_t = None
    if any(r is None for r in per_room["rnd"]):
        rnd_u = torch.rand(v.nvt, dtype=torch.float64, device=dev, generator=generator)
    if any(c and i is None for c, i in zip(v.cropped, per_room["init_idx"])):
        init_u = torch.rand(B, dtype=torch.float64, device=dev, generator=generator)
    if any(p and per_room["pad"][b] is None for b, p in enumerate(v.padded)):
        pad_t = (torch.rand(B, n_out, dtype=torch.float64, device=dev, generator=generator) * v.nv_column()).int()
    if shuffle and any(p is None for p in per_room["perm"]):
        perm_t = torch.rand(B, n_out, device=dev, generator=generator).argsort(dim=1).int()
    rnd_t, init_t, pad_t, perm_t = v.given(per_room, pad_t, perm_t, shuffle, who)
    chain = _is_chain(transform)
    if chain:  # a transforms.TransformChain: any configured list, its draws under its own keys
        cd = _chain_draws(transform, d, [n_out] * B, dev, generator)
    # the transform's draws (S3DISTrainAugment.draw's keys)
    if not chain and any(k not in d for k in list(_S3DIS_TRANSFORM_KEYS) + ["noise"]):
        for k, t in _s3dis_transform_draws(transform, B, n_out, dev, generator).items():
            d.setdefault(k, t)
    for k, shape in [] if chain else list(_S3DIS_TRANSFORM_KEYS.items()) + [("noise", (n_out, 3))]:
        d[k] = torch.as_tensor(d[k]).to(dev)
        if d[k].shape != (B,) + shape:
            raise ValueError(f"{who}: draws[{k!r}] has shape {tuple(d[k].shape)}, not {(B,) + shape}")

    sel, order = v.select_crop(voxel_max, rnd_t, rnd_u, init_t, init_u)
    pos0 = torch.empty(B, n_out, 3, dtype=torch.float32, device=dev)
    colour = torch.empty(B, n_out, 3, dtype=torch.float32, device=dev)
    y = torch.empty(B, n_out, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(v.lib.amc3d_s3dis_crop_tail(B, n_out, voxel_max, f64, _opt(raw), _opt(src_t), _opt(off_t), _opt(v.coord),
                                               _opt(v.vbase), _opt(sel), _opt(order), _opt(pad_t), _opt(perm_t), _opt(pos0),
                                               _opt(colour), _opt(y), v.stream), "s3dis_crop_tail")
    if chain:
        out = transform({"pos": pos0, "x": colour}, draws=cd)
        pos, x, heights = out["pos"], out["x"], out["heights"]
        if gravity_dim != transform.gravity_dim:
            heights = pos0[:, :, gravity_dim:gravity_dim + 1].contiguous()
        return {"pos": pos, "x": x, "heights": heights, "y": y}
    pos, x, heights = _s3dis_augment(transform, pos0, colour, d)
    if gravity_dim != transform.g:
        heights = pos0[:, :, gravity_dim:gravity_dim + 1].contiguous()
    return {"pos": pos, "x": x, "heights": heights, "y": y}


def _s3dis_rooms(rooms, who):
    rooms = list(rooms)
    if len(rooms) == 0:
        raise ValueError(f"{who}: no rooms")
    for r in rooms:
        if not (torch.is_tensor(r) and r.is_cuda and r.dim() == 2 and r.shape[1] == 7 and r.shape[0] > 0
                and r.dtype in (torch.float32, torch.float64) and r.device == rooms[0].device):
            raise ValueError(f"{who}: every room is an (n,7) float32 or float64 tensor on one GPU with n > 0: xyz, rgb, label")
    return rooms


def s3dis_train_batch(rooms, transform, voxel_size=0.04, voxel_max=24000, variable=False, shuffle=True, generator=None,
                      draws=None, gravity_dim=2):
    """S3DIS.__getitem__ for training with presample=False (dataset/s3dis/s3dis.py:122-144) plus the default collate, for a
    batch of raw rooms on the GPU (csrc/room_input.hip): every room cast to float32, xyz -= min, crop_pc (min-corner shift,
    voxelize mode 0, the voxel_max representatives nearest to representative init_idx or, with variable=False, padding by
    repetition, shuffle, min-corner shift), then `transform` (augment.S3DISTrainAugment) on the cropped clouds; heights is the
    gravity coordinate of the cropped cloud before the transforms.  Bit for bit what crop_pc per room, torch.stack and
    `transform` give from the same draws, in a handful of launches for the whole batch instead of about twenty per room.

    rooms: list of (n_b,7) GPU tensors, float32 or float64, as np.load of an Area_*.npy gives them: xyz, rgb 0..255, label
    (rooms of both dtypes in one batch are promoted to float64, which changes nothing: the first step is the float32 cast).
    Returns {pos (B,N,3) fp32, x (B,N,3) fp32, heights (B,N,1) fp32, y (B,N) int64}, what DataLoader(S3DIS(split='train'))
    yields; every room must come out with the same N (always so with variable=False).

    Random numbers come from `generator` (a torch.Generator on the rooms' device, or the default one) or from `draws`: a
    dict with the transform's keys (S3DISTrainAugment.draw) and per-room lists "rnd" (voxelize's randint(0, count.max(),
    nvox)), "init_idx", "pad", "perm" (entries may be None).  Device draws are floor(u * range) of a float64 uniform, as in
    scannet_train_batch; the shuffle is the argsort of uniforms.
    Host synchronisation: one read-back per batch (the B voxel counts, after all the voxelise work is enqueued), none per
    room; draws that are passed in are validated, which reads their verdicts back."""
    rooms = _s3dis_rooms(rooms, "s3dis_train_batch")
    sizes = [int(r.shape[0]) for r in rooms]
    src = [0]
    for n in sizes[:-1]:
        src.append(src[-1] + n)
    raw = rooms[0].contiguous() if len(rooms) == 1 else torch.cat(rooms)
    return _s3dis_batch(raw, src, sizes, transform, voxel_size, voxel_max, variable, shuffle, generator, draws, gravity_dim)


class S3DISTrainFeed:
    """An epoch of S3DIS training batches from rooms resident on the device: what DataLoader(S3DIS(split='train', loop=loop,
    presample=False), batch_size, shuffle=shuffle, drop_last=drop_last) yields.  Every epoch (every `iter`) draws a
    permutation of the len(rooms) * loop item ids from `generator` (one read-back per epoch); item id -> room id % len(rooms)
    (s3dis.py:123,146-147).  Every batch is one s3dis_train_batch call (variable=False) on the current stream, at the moment
    the consumer asks for it: no side stream, no prefetch.  The rooms are kept as one concatenated array, so a batch copies
    nothing.  train.train_one_epoch takes it as `train_loader`."""

    def __init__(self, rooms, transform, batch_size, loop=1, voxel_size=0.04, voxel_max=24000, shuffle=True, drop_last=True,
                 generator=None):
        rooms = _s3dis_rooms(rooms, "S3DISTrainFeed")
        if int(batch_size) <= 0 or int(loop) <= 0:
            raise ValueError("S3DISTrainFeed: batch_size and loop are positive")
        if voxel_max is None:
            raise ValueError("S3DISTrainFeed: voxel_max is the size of a training cloud")
        self.sizes = [int(r.shape[0]) for r in rooms]
        self.starts = [0]
        for n in self.sizes[:-1]:
            self.starts.append(self.starts[-1] + n)
        self.raw = rooms[0].contiguous() if len(rooms) == 1 else torch.cat(rooms)
        self.transform, self.batch_size, self.loop = transform, int(batch_size), int(loop)
        self.voxel_size, self.voxel_max, self.shuffle, self.drop_last = voxel_size, voxel_max, bool(shuffle), bool(drop_last)
        self.generator = generator

    def __len__(self):
        items = len(self.sizes) * self.loop
        return items // self.batch_size if self.drop_last else -(-items // self.batch_size)

    def __iter__(self):
        items = len(self.sizes) * self.loop
        ids = (torch.randperm(items, device=self.raw.device, generator=self.generator).tolist() if self.shuffle
               else list(range(items)))
        for i in range(len(self)):
            pick = [j % len(self.sizes) for j in ids[i * self.batch_size:(i + 1) * self.batch_size]]
            yield _s3dis_batch(self.raw, [self.starts[j] for j in pick], [self.sizes[j] for j in pick], self.transform,
                               self.voxel_size, self.voxel_max, False, True, self.generator, None, 2)


_SCANNET_TRANSFORM_KEYS = ("scale", "mirror_u", "contrast_u", "blend", "drop_u")


def _scannet_rooms(rooms, who):
    """the rooms of a ScanNet batch or feed, checked -> (coord (T,3), feat (T,3), label (T) int64, sizes)"""
    rooms = list(rooms)
    if len(rooms) == 0:
        raise ValueError(f"{who}: no rooms")
    for c, f, l in rooms:
        _need_gpu(c, f, l)
        _need_dtype(torch.float32, coord=c, feat=f)
        if (c.dim() != 2 or c.shape[1] != 3 or f.shape != c.shape or l.numel() != c.shape[0] or c.shape[0] == 0
                or c.device != rooms[0][0].device):
            raise ValueError(f"{who}: every room needs coord (n,3), feat (n,3), label (n,) with n > 0, on one GPU")
    one = len(rooms) == 1
    coord = rooms[0][0].contiguous() if one else torch.cat([c for c, _, _ in rooms])
    feat = rooms[0][1].contiguous() if one else torch.cat([f for _, f, _ in rooms])
    label = torch.cat([l.reshape(-1).to(torch.int64) for _, _, l in rooms])
    return coord, feat, label, [int(c.shape[0]) for c, _, _ in rooms]


def _scannet_transform(t, coord, feat, off_t, d):
    """ScanNetTrainAugment.__call__ on given draws -- the same records for the same two entry points, bit for bit -- with the
    records going up through pinned staging instead of a blocking copy"""
    B, T, dev = off_t.shape[0] - 1, coord.shape[0], coord.device
    par = t.params(d).pin_memory().to(dev, non_blocking=True)
    mean, std = _colour_constants(t.color_mean if t.color_mean is not None else (0.0, 0.0, 0.0),  # (x - 0) / 1 == x exactly
                                  t.color_std if t.color_std is not None else (1.0, 1.0, 1.0), dev, "scannet_train_rooms")
    pos = torch.empty(T, 3, dtype=torch.float64, device=dev)
    x = torch.empty(T, 3, dtype=torch.float32, device=dev)
    stats = torch.empty(B, 8, dtype=torch.float32, device=dev)
    lib = _lib.load()
    wb = int(lib.amc3d_scannet_stats_workspace_bytes(B))
    work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.amc3d_scannet_room_stats(B, _ptr(off_t), _ptr(feat), _ptr(par), _ptr(stats), _ptr(work), wb, _stream(coord)),
                   "scannet_room_stats")
        _lib.check(lib.amc3d_scannet_transform_rooms(B, T, _ptr(off_t), _ptr(coord), _ptr(feat), _ptr(par), _ptr(stats), _ptr(mean),
                                                     _ptr(std), _ptr(pos), _ptr(x), _stream(coord)), "scannet_transform_rooms")
    return pos, x


def _scannet_batch(coord, feat, label, sizes, transform, voxel_size, voxel_max, variable, generator, draws, gravity_dim,
                   who="scannet_train_rooms"):
    """scannet_train_rooms on rooms that are already concatenated: coord (T,3) fp32, feat (T,3) fp32, label (T) int64"""
    B, dev, total = len(sizes), coord.device, sum(sizes)
    _check_rooms_args(who, voxel_size, voxel_max, gravity_dim, total)
    voxel_max = int(voxel_max)
    d = dict(draws or {})
    per_room = _pop_per_room(d, B, who)
    chain = _is_chain(transform)
    if not chain and (any(k not in d for k in _SCANNET_TRANSFORM_KEYS) or ("angle" not in d and "R" not in d)):
        for k, t in transform.draw(B, generator, dev).items():  # a read-back when the generator lives on the device
            d.setdefault(k, t)
    offsets = [0]
    for n in sizes:
        offsets.append(offsets[-1] + n)
    off_t = _upload(offsets, torch.int64, dev)
    if chain:  # a transforms.TransformChain: its draws are made on the device, nothing is read back for them
        pos64, x = _chain_rooms(transform, coord, feat, off_t, sizes, _chain_draws(transform, d, sizes, dev, generator))
    else:
        pos64, x = _scannet_transform(transform, coord, feat, off_t, d)
    v = _RoomVoxels("scannet", torch.float64, B, total, voxel_size, dev, (_opt(pos64), _opt(off_t)))
    # the device's own draws, enqueued before the read-back in tables sized by the point count (a room has at most as many
    # voxels as points), so the stream does not depend on the voxel counts: voxelize's randint, crop_pc's randint(N), its
    # np.random.choice(N, voxel_max - N) and its permutation, in this order
    rnd_u = init_u = pad_t = perm_t = None
    if any(r is None for r in per_room["rnd"]):
        rnd_u = torch.rand(total, dtype=torch.float64, device=dev, generator=generator)
    if any(i is None for i in per_room["init_idx"]):
        init_u = torch.rand(B, dtype=torch.float64, device=dev, generator=generator)
    if not variable:
        if any(p is None for p in per_room["pad"]):
            pad_t = (torch.rand(B, voxel_max, dtype=torch.float64, device=dev, generator=generator) * v.nv_column()).int()
        if any(p is None for p in per_room["perm"]):
            perm_t = torch.rand(B, voxel_max, device=dev, generator=generator).argsort(dim=1).int()
    v.read_back(voxel_max, variable, who)
    n_out = v.n_out
    if perm_t is None and any(p is None for p in per_room["perm"]):  # variable=True: the size of the shuffle is the voxel count
        perm_t = torch.rand(B, n_out, device=dev, generator=generator).argsort(dim=1).int()
    rnd_t, init_t, pad_t, perm_t = v.given(per_room, pad_t, perm_t, True, who)
    sel, order = v.select_crop(voxel_max, rnd_t, rnd_u, init_t, init_u)
    wb = int(v.lib.amc3d_scannet_crop_tail_workspace_bytes(B))
    work = torch.empty(max(wb, 8) // 8, dtype=torch.float64, device=dev)
    out = {"pos": torch.empty(B, n_out, 3, dtype=torch.float32, device=dev),
           "x": torch.empty(B, n_out, 3, dtype=torch.float32, device=dev),
           "heights": torch.empty(B, n_out, 1, dtype=torch.float32, device=dev),
           "y": torch.empty(B, n_out, dtype=torch.int64, device=dev)}
    with torch.cuda.device(dev):
        _lib.check(v.lib.amc3d_scannet_crop_tail_rooms(B, n_out, voxel_max, int(gravity_dim), _opt(v.coord), _opt(x), _opt(label),
                                                       _opt(v.vbase), _opt(sel), _opt(order), _opt(pad_t), _opt(perm_t),
                                                       _opt(out["pos"]), _opt(out["x"]), _opt(out["heights"]), _opt(out["y"]),
                                                       _opt(work), wb, v.stream), "scannet_crop_tail_rooms")
    return out


def scannet_train_rooms(rooms, transform, voxel_size=0.02, voxel_max=64000, variable=False, generator=None, draws=None,
                        gravity_dim=2):
    """scannet_train_batch with everything after the transform chain done for the whole batch at once (csrc/room_input.hip):
    the same arguments, the same `draws` dictionary -- the transform's keys, "R" included, and the per-room lists "rnd",
    "init_idx", "pad", "perm" (entries may be None) -- and the same return value.  For the same draws every output equals
    scannet_train_batch's bit for bit, in about twenty launches for the batch instead of about twenty per room.

    With a generator the draws are made on the device, the way s3dis_train_batch makes them: floor(u * range) of float64
    uniforms (voxelize's randint, the crop centre, the padding) and the shuffle as the argsort of uniforms.  They are enqueued
    before the read-back, in tables sized by the point count (voxels <= points) and by voxel_max, so the random stream does not
    depend on the voxel counts -- and therefore differs from scannet_train_batch's, which draws room by room at the voxel
    count's size.  (variable=True: the shuffle has the voxel count's size and is drawn after the read-back.)
    Host synchronisation: one read-back per batch (the B voxel counts, after the voxelisation is enqueued), none per room; one
    more only when the room-level draws have to come from a device generator (the rotation is formed on the host from cos /
    sin); draws that are passed in are validated, which reads their verdicts back.  Small host tables (offsets, the transform's
    records, the crop centres) go up through pinned staging.
    variable=True: a room below voxel_max keeps its own size; rooms that come out with different sizes raise ValueError."""
    coord, feat, label, sizes = _scannet_rooms(rooms, "scannet_train_rooms")
    return _scannet_batch(coord, feat, label, sizes, transform, voxel_size, voxel_max, variable, generator, draws, gravity_dim)


def feed_picks(ids, n_rooms, batch_size, drop_last):
    """the rooms of every batch of an epoch: item ids (in the epoch's order) -> [[room, ...], ...], what
    BatchSampler(ids, batch_size, drop_last) groups and ScanNet.__getitem__'s `idx % len(data_list)` maps to rooms"""
    ids = [int(i) for i in ids]
    if int(n_rooms) <= 0 or int(batch_size) <= 0:
        raise ValueError("feed_picks: n_rooms and batch_size are positive")
    end = len(ids) - len(ids) % batch_size if drop_last else len(ids)
    return [[j % n_rooms for j in ids[i:i + batch_size]] for i in range(0, end, batch_size)]


class ScanNetTrainFeed:
    """An epoch of ScanNet training batches from rooms resident on the device: what DataLoader(ScanNet(split='train',
    loop=loop), batch_size, shuffle=shuffle, drop_last=drop_last) yields.  rooms: list of (coord (n,3) fp32, feat (n,3) fp32,
    label (n[,1])) GPU tensors, kept as three concatenated arrays.  Every epoch (every `iter`) draws a permutation of the
    len(rooms) * loop item ids and the room-level transform uniforms of all its items from `generator` (at most two read-backs
    per epoch); item id -> room id % len(rooms) (scannet.py:137-138).  Every batch is one scannet_train_rooms call
    (variable=False) with those room-level draws passed in, on the current stream, at the moment the consumer asks for it: one
    read-back per batch, no side stream, no prefetch.  The transform kernels take contiguous rooms, so a batch first
    concatenates the picked slices (one torch.cat per array).  train.train_one_epoch takes it as `train_loader`."""

    def __init__(self, rooms, transform, batch_size, loop=1, voxel_size=0.02, voxel_max=64000, shuffle=True, drop_last=True,
                 generator=None):
        self.coord, self.feat, self.label, self.sizes = _scannet_rooms(rooms, "ScanNetTrainFeed")
        if int(batch_size) <= 0 or int(loop) <= 0:
            raise ValueError("ScanNetTrainFeed: batch_size and loop are positive")
        if voxel_max is None:
            raise ValueError("ScanNetTrainFeed: voxel_max is the size of a training cloud")
        self.starts = [0]
        for n in self.sizes[:-1]:
            self.starts.append(self.starts[-1] + n)
        self.transform, self.batch_size, self.loop = transform, int(batch_size), int(loop)
        self.voxel_size, self.voxel_max, self.shuffle, self.drop_last = voxel_size, voxel_max, bool(shuffle), bool(drop_last)
        self.generator = generator

    def __len__(self):
        items = len(self.sizes) * self.loop
        return items // self.batch_size if self.drop_last else -(-items // self.batch_size)

    def __iter__(self):
        items, dev = len(self.sizes) * self.loop, self.coord.device
        ids = torch.randperm(items, device=dev, generator=self.generator).tolist() if self.shuffle else list(range(items))
        # host tensors, one row per item in the epoch's order; a TransformChain draws per batch, on the device
        room_draws = {} if _is_chain(self.transform) else self.transform.draw(items, self.generator, dev)
        for i, pick in enumerate(feed_picks(ids, len(self.sizes), self.batch_size, self.drop_last)):
            lo = i * self.batch_size
            d = {k: v[lo:lo + len(pick)] for k, v in room_draws.items()}
            cut = lambda t: (t[self.starts[pick[0]]:self.starts[pick[0]] + self.sizes[pick[0]]] if len(pick) == 1 else  # noqa: E731
                             torch.cat([t[self.starts[j]:self.starts[j] + self.sizes[j]] for j in pick]))
            yield _scannet_batch(cut(self.coord), cut(self.feat), cut(self.label), [self.sizes[j] for j in pick], self.transform,
                                 self.voxel_size, self.voxel_max, False, self.generator, d, 2, "ScanNetTrainFeed")


# ---- S3DISSphere: potential-picked spheres out of whole sub-sampled Areas (dataset/s3dis/s3dis_sphere.py, csrc/sphere.hip) ----
_POT_BLOCK = 1024  # kPotBlock of csrc/sphere.hip: potentials per entry of the minima table


class SpherePotentials:
    """The resident state of S3DISSphere's schedule (s3dis_sphere.py:214-247): the sub-clouds of a split, concatenated, the
    float64 potentials of their points and the table of block minima the centre pick runs over.

    clouds: list of (sub_points (n,3) float32, sub_colors (n,3), sub_labels (n)) GPU tensors -- an Area after
    crop_pc(points, colors, labels, voxel_size=voxel_size); colours are kept as float32, labels as int64.
    potentials: list of (n) float64 tensors or arrays, one per cloud (the tests pass the reference's own); None draws the
    reference's rand(n) * 1e-3 per cloud on the device from `generator`.
    advance(steps) runs the next `steps` schedule steps on the device -- five launches each, counting the library sort as one,
    nothing read back -- and returns (cloud_ind (steps) int64, point_ind (steps) int64, noise (steps,3) float64): because step s
    depends only on the steps before it, the concatenation over calls is the table the reference precomputes for
    num_epochs * num_steps steps from the same draws.
    Arithmetic: the reference's with numpy >= 2 (the Tukey weights and their comparison are float64 there; numpy 1.x keeps them
    float32).  Equal distances inside a sphere are listed in ascending point order and a tied potential minimum is the first
    one (the reference: sklearn's unspecified order, numpy's first minimum).  A sphere without any point (a noise draw of about
    ten sigma; the reference raises inside np.random.choice) updates nothing."""

    def __init__(self, clouds, in_radius, num_points, potentials=None, generator=None):
        clouds = list(clouds)
        if len(clouds) == 0:
            raise ValueError("SpherePotentials: no clouds")
        for p, c, l in clouds:
            _need_gpu(p, c, l)
            _need_dtype(torch.float32, sub_points=p)
            if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] == 0 or c.shape != p.shape or l.numel() != p.shape[0] \
                    or p.device != clouds[0][0].device:
                raise ValueError("SpherePotentials: every cloud needs sub_points (n,3), sub_colors (n,3), sub_labels (n) with n > 0, "
                                 "on one GPU")
        if not float(in_radius) > 0 or int(num_points) <= 0:
            raise ValueError("SpherePotentials: in_radius and num_points are positive")
        self.in_radius, self.num_points, self.generator = float(in_radius), int(num_points), generator
        self.dev = dev = clouds[0][0].device
        self.sizes = [int(p.shape[0]) for p, _, _ in clouds]
        self.offsets = [0]
        for n in self.sizes:
            self.offsets.append(self.offsets[-1] + n)
        self.total = self.offsets[-1]
        if self.total >= 2 ** 31:
            raise ValueError(f"SpherePotentials: {self.total} points (at most 2^31 - 1)")
        one = len(clouds) == 1
        self.points = clouds[0][0].contiguous() if one else torch.cat([p for p, _, _ in clouds])
        self.colors = torch.cat([c.to(torch.float32) for _, c, _ in clouds]).contiguous()
        self.labels = torch.cat([l.reshape(-1).to(torch.int64) for _, _, l in clouds]).contiguous()
        self.cloud_off = torch.tensor(self.offsets, dtype=torch.int32).to(dev)
        self.n_max = max(self.sizes)
        self.nb_max = max((self.offsets[c + 1] - 1) // _POT_BLOCK - self.offsets[c] // _POT_BLOCK + 1 for c in range(len(clouds)))
        if potentials is None:
            self.potentials = torch.cat([torch.rand(n, dtype=torch.float64, device=dev, generator=generator) for n in self.sizes]) * 1e-3
        else:
            potentials = [torch.as_tensor(p).to(device=dev, dtype=torch.float64).reshape(-1) for p in potentials]
            if [int(p.shape[0]) for p in potentials] != self.sizes:
                raise ValueError("SpherePotentials: one potential per point of every cloud")
            self.potentials = torch.cat(potentials).contiguous()
        nblk = -(-self.total // _POT_BLOCK)
        self.blk_val = torch.empty(nblk, dtype=torch.float64, device=dev)
        self.blk_idx = torch.empty(nblk, dtype=torch.int32, device=dev)
        self.touched = torch.empty(nblk, dtype=torch.int32, device=dev)
        self.lib = lib = _lib.load()
        self.wb = int(lib.amc3d_sphere_workspace_bytes(self.n_max))
        self.work = torch.empty(max(self.wb, 8), dtype=torch.uint8, device=dev)
        self.steps_done = 0
        with torch.cuda.device(dev):
            _lib.check(lib.amc3d_sphere_minima(self.total, _opt(self.potentials), _opt(self.blk_val), _opt(self.blk_idx),
                                               _opt(self.touched), _stream(self.points)), "sphere_minima")

    def cloud_potentials(self):
        """the potentials per cloud (views)"""
        return [self.potentials[self.offsets[c]:self.offsets[c + 1]] for c in range(len(self.sizes))]

    def _noise(self, steps, noise):
        if noise is None:  # np.random.normal(scale=in_radius / 10, size=(1, 3)) per step
            return torch.randn(steps, 3, dtype=torch.float64, device=self.dev, generator=self.generator) * (self.in_radius / 10)
        noise = torch.as_tensor(noise).to(device=self.dev, dtype=torch.float64).reshape(-1, 3).contiguous()
        if noise.shape[0] != steps:
            raise ValueError(f"SpherePotentials: noise holds {noise.shape[0]} rows for {steps} spheres")
        return noise

    def _lists(self, n):
        dev = self.dev
        return (torch.empty(n, 3, dtype=torch.float64, device=dev), torch.empty(n, self.num_points, dtype=torch.int32, device=dev),
                torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))

    def advance(self, steps, noise=None, lists=False):
        """the next `steps` schedule steps -> (cloud_ind, point_ind, noise) on the device; lists=True adds the dictionary of
        every step's query (centre (steps,3) float64, order (steps,num_points) int32, cur, count (steps) int32), which is the
        query its item repeats in the reference"""
        steps = int(steps)
        if steps < 0:
            raise ValueError("SpherePotentials.advance: steps is not negative")
        noise = self._noise(steps, noise)
        cloud = torch.empty(steps, dtype=torch.int32, device=self.dev)
        point = torch.empty(steps, dtype=torch.int32, device=self.dev)
        centre, order, cur, count = self._lists(steps)
        if steps:
            with torch.cuda.device(self.dev):
                _lib.check(self.lib.amc3d_sphere_schedule(
                    len(self.sizes), self.total, self.n_max, self.nb_max, steps, self.num_points, ctypes.c_double(self.in_radius),
                    _opt(self.points), _opt(self.cloud_off), _opt(self.potentials), _opt(self.blk_val), _opt(self.blk_idx),
                    _opt(self.touched), _opt(noise), _opt(cloud), _opt(point), _opt(centre), _opt(order) if lists else None,
                    _opt(cur), _opt(count), _opt(self.work), self.wb, _stream(self.points)), "sphere_schedule")
        self.steps_done += steps
        out = (cloud.long(), point.long(), noise)
        if lists:
            return out + ({"cloud": cloud, "point": point, "centre": centre, "order": order, "cur": cur, "count": count},)
        return out

    def query(self, cloud_ind, point_ind, noise):
        """the radius query of given centres (three launches each, counting the sort as one; the potentials are not touched) ->
        {cloud, point (B) int32, centre (B,3) float64, order (B,num_points) int32 (-1 beyond count), cur, count (B) int32}"""
        cloud = torch.as_tensor(cloud_ind).to(device=self.dev, dtype=torch.int32).reshape(-1).contiguous()
        point = torch.as_tensor(point_ind).to(device=self.dev, dtype=torch.int32).reshape(-1).contiguous()
        B = int(cloud.shape[0])
        if point.shape[0] != B:
            raise ValueError("SpherePotentials.query: one point per cloud index")
        noise = self._noise(B, noise)
        centre, order, cur, count = self._lists(B)
        if B:
            with torch.cuda.device(self.dev):
                _lib.check(self.lib.amc3d_sphere_query(
                    len(self.sizes), self.total, self.n_max, B, self.num_points, ctypes.c_double(self.in_radius), _opt(self.points),
                    _opt(self.cloud_off), _opt(cloud), _opt(point), _opt(noise), _opt(centre), _opt(order), _opt(cur), _opt(count),
                    _opt(self.work), self.wb, _stream(self.points)), "sphere_query")
        return {"cloud": cloud, "point": point, "centre": centre, "order": order, "cur": cur, "count": count}


def _sphere_draw_table(given, B, N, count, pad, who):
    """per-sphere draws that were passed in -> ((B,N) int32 table, -1 where the device draws; one read-back: the counts size
    them).  perm[b]: a permutation of count[b]; pad[b]: N - count[b] indices below count[b], stored in slots count[b].."""
    dev = count.device
    given = list(given)
    if len(given) != B:
        raise ValueError(f"{who}: per-sphere draws need one entry per sphere")
    cnt = count.tolist()
    table = torch.full((B, N), -1, dtype=torch.int32, device=dev)
    for b, v in enumerate(given):
        if v is None:
            continue
        v = torch.as_tensor(v).to(dev)
        c = cnt[b]
        if pad:
            if v.shape != (N - c,) or v.is_floating_point() or (v.numel() and bool(((v < 0) | (v >= c)).any())):
                raise ValueError(f"{who}: sphere {b}: pad must hold {N - c} indices below {c}")
            table[b, c:] = v
        else:
            if v.shape != (c,) or v.is_floating_point() or not bool((v.sort().values == torch.arange(c, device=dev)).all()):
                raise ValueError(f"{who}: sphere {b}: perm must be a permutation of {c}")
            table[b, :c] = v
    return table


def _sphere_tail(state, q, perm_t, pad_t, pad_u, gravity_dim):
    B, N, dev = int(q["cloud"].shape[0]), state.num_points, state.dev
    out = {"pos": torch.empty(B, N, 3, dtype=torch.float32, device=dev), "x": torch.empty(B, N, 3, dtype=torch.float32, device=dev),
           "heights": torch.empty(B, N, 1, dtype=torch.float32, device=dev), "y": torch.empty(B, N, dtype=torch.int64, device=dev),
           "mask": torch.empty(B, N, dtype=torch.int32, device=dev), "cloud_index": q["cloud"].long(),
           "input_inds": torch.empty(B, N, dtype=torch.int64, device=dev)}
    with torch.cuda.device(dev):
        _lib.check(state.lib.amc3d_sphere_tail(
            len(state.sizes), B, N, int(gravity_dim), _opt(state.points), _opt(state.colors), _opt(state.labels), _opt(state.cloud_off),
            _opt(q["cloud"]), _opt(q["point"]), _opt(q["centre"]), _opt(q["order"]), _opt(q["count"]), _opt(perm_t), _opt(pad_t),
            _opt(pad_u), _opt(out["input_inds"]), _opt(out["mask"]), _opt(out["pos"]), _opt(out["x"]), _opt(out["y"]),
            _opt(out["heights"]), _stream(state.points)), "sphere_tail")
    return out


def s3dis_sphere_batch(state, steps_or_B, transform=None, draws=None, generator=None, gravity_dim=2):
    """S3DISSphere.__getitem__ (s3dis_sphere.py:288-347) plus the default collate for B spheres of `state` (a SpherePotentials).
    steps_or_B: an int B -- the next B schedule steps, whose potentials are updated (state.advance) -- or the (cloud_ind,
    point_ind, noise) of B steps already advanced, which are queried again as the reference's item does.
    transform: an augment.S3DISTrainAugment, a transforms.TransformChain or None, applied to pos = point - pick and the colours.
    Returns {pos (B,N,3) fp32, x (B,N,3) fp32, heights (B,N,1) fp32, y (B,N) int64, mask (B,N) int32, cloud_index (B) int64,
    input_inds (B,N) int64, cloud-local}, N = num_points.  heights follows the reference's `if 'heights' not in data` rule: the
    chain's value where its list holds a PointCloudCenterAndNormalize (the only reference transform that writes one), otherwise
    the point's own gravity coordinate, before the centring.
    Per sphere, count = min(cur, N): slots below count are the query's first count points shuffled, the others repeat draws
    among them; mask is 1 below count.  cur == 0: every slot is the centre's own point and mask is 0.
    draws: "perm" / "pad" as per-sphere lists (entries may be None) of the reference's np.random.permutation (count entries)
    and np.random.choice(cur, N - cur), "centre_noise" (B,3) for the B steps an int advances (the schedule's
    np.random.normal), plus the transform's keys.  Device draws: the shuffle is the argsort of uniforms
    restricted to the first count slots, the padding floor(u * count) of float64 uniforms -- both enqueued without knowing
    count.  Host synchronisation: none with generator draws; passed-in perm / pad are validated against the counts, which
    reads them back."""
    who = "s3dis_sphere_batch"
    if not isinstance(state, SpherePotentials):
        raise TypeError(f"{who}: state is a SpherePotentials")
    if gravity_dim not in (0, 1, 2):
        raise ValueError(f"{who}: gravity_dim is 0, 1 or 2")
    generator = generator if generator is not None else state.generator
    d = dict(draws or {})
    centre_noise = d.pop("centre_noise", None)
    if isinstance(steps_or_B, int):
        q = state.advance(steps_or_B, noise=centre_noise, lists=True)[3]
    else:
        q = state.query(*steps_or_B)
    B, N, dev = int(q["cloud"].shape[0]), state.num_points, state.dev
    if B == 0:
        raise ValueError(f"{who}: no spheres")
    perm_g, pad_g = d.pop("perm", None), d.pop("pad", None)
    count = q["count"]
    perm_t = pad_t = pad_u = None
    if perm_g is not None:
        perm_t = _sphere_draw_table(perm_g, B, N, count, False, who)
    if perm_g is None or any(v is None for v in perm_g):
        u = torch.rand(B, N, device=dev, generator=generator)
        slot = torch.arange(N, device=dev, dtype=torch.int32).view(1, N)
        drawn = torch.where(slot < count.view(B, 1), u, 2.0).argsort(dim=1, stable=True).int()
        given = torch.tensor([v is not None for v in perm_g], device=dev).view(B, 1) if perm_g is not None else None
        perm_t = drawn if given is None else torch.where(given, perm_t, drawn)
    if pad_g is not None:
        pad_t = _sphere_draw_table(pad_g, B, N, count, True, who)
    if pad_g is None or any(v is None for v in pad_g):
        pad_u = torch.rand(B, N, dtype=torch.float64, device=dev, generator=generator)
    out = _sphere_tail(state, q, perm_t.contiguous(), pad_t, pad_u, gravity_dim)
    if transform is None:
        return out
    if _is_chain(transform):
        t = transform({"pos": out["pos"], "x": out["x"]}, draws=_chain_draws(transform, d, [N] * B, dev, generator))
        out["pos"], out["x"] = t["pos"], t["x"]
        if "PointCloudCenterAndNormalize" in transform.names:
            out["heights"] = t["heights"]
        return out
    if any(k not in d for k in list(_S3DIS_TRANSFORM_KEYS) + ["noise"]):
        for k, t in _s3dis_transform_draws(transform, B, N, dev, generator).items():
            d.setdefault(k, t)
    for k, shape in list(_S3DIS_TRANSFORM_KEYS.items()) + [("noise", (N, 3))]:
        d[k] = torch.as_tensor(d[k]).to(dev)
        if d[k].shape != (B,) + shape:
            raise ValueError(f"{who}: draws[{k!r}] has shape {tuple(d[k].shape)}, not {(B,) + shape}")
    out["pos"], out["x"], _ = _s3dis_augment(transform, out["pos"], out["x"], d)
    return out


class S3DISSphereFeed:
    """An epoch of S3DISSphere batches from sub-clouds resident on the device: what DataLoader(S3DISSphere(...), batch_size,
    shuffle=shuffle, drop_last=True) yields, `mask` and `input_inds` included.  len = num_steps // batch_size.  Every `iter` is
    the next epoch of the schedule (the reference's `epoch * num_steps` offset into its precomputed table): with shuffle=False
    batch i advances the schedule by its own batch_size steps at the moment the consumer asks for it, and the steps a last,
    incomplete batch would hold are advanced at the end; shuffle=True advances the epoch's whole schedule first, permutes its
    items on the device and queries every batch's centres again.  Nothing is read back.  train.train_one_epoch takes it as
    `train_loader` (with a criterion whose name contains 'mask' the loop passes data['mask'] on)."""

    def __init__(self, clouds, transform, batch_size, in_radius, num_points, num_steps, shuffle=False, potentials=None,
                 generator=None, gravity_dim=2):
        if int(batch_size) <= 0 or int(num_steps) < 0:
            raise ValueError("S3DISSphereFeed: batch_size is positive and num_steps is not negative")
        self.state = SpherePotentials(clouds, in_radius, num_points, potentials=potentials, generator=generator)
        self.transform, self.batch_size, self.num_steps = transform, int(batch_size), int(num_steps)
        self.shuffle, self.generator, self.gravity_dim = bool(shuffle), generator, gravity_dim
        self.epoch = 0

    def __len__(self):
        return self.num_steps // self.batch_size

    def __iter__(self):
        B, n = self.batch_size, len(self)
        self.epoch += 1
        if self.shuffle:
            cloud, point, noise = self.state.advance(self.num_steps)
            ids = torch.randperm(self.num_steps, device=self.state.dev, generator=self.generator)
            for i in range(n):
                pick = ids[i * B:(i + 1) * B]
                yield s3dis_sphere_batch(self.state, (cloud[pick], point[pick], noise[pick]), self.transform,
                                         generator=self.generator, gravity_dim=self.gravity_dim)
        else:
            for i in range(n):
                yield s3dis_sphere_batch(self.state, B, self.transform, generator=self.generator, gravity_dim=self.gravity_dim)
            self.state.advance(self.num_steps - n * B)


def sphere_projections(points, sub_points):
    """S3DISSphere's validation projections (s3dis_sphere.py:255-266): per raw point the index of its nearest sub-point, (n)
    int64, on the k-NN search with k = 1.  The reference asks sklearn's KD-tree, float64; here the distance is the search's
    float32 ((dx*dx + dy*dy) + dz*dz) of the direct differences with its own order of equal distances, so a raw point with two
    sub-points at one float32 distance may take the other one."""
    _need_gpu(points, sub_points)
    _need_dtype(torch.float32, points=points, sub_points=sub_points)
    if points.dim() != 2 or points.shape[1] != 3 or sub_points.dim() != 2 or sub_points.shape[1] != 3 or sub_points.shape[0] == 0:
        raise ValueError("sphere_projections: points (n,3) and sub_points (m,3) with m > 0")
    from . import ops
    _, idx = ops.knn_batch(1, sub_points.contiguous().unsqueeze(0), points.contiguous().unsqueeze(0))
    return idx.reshape(-1).long()
