"""S3DIS validation and whole-room testing on the device (csrc/room_eval.hip; input_pipeline.s3dis_part_batch /
room_representatives / s3dis_val_cloud, ops.expand_parts, evaluate.test_room_s3dis) against what the reference's own code
returned for the same rooms (tests/golden/s3dis_eval.npz, recorded by tests/tools/gen_golden_s3dis_eval.py) and against the
numpy restatements of tests/s3dis_eval_ref.py, which tests/test_s3dis_eval_host.py pins to that fixture.

The reference leaves one bit open: PointCloudXYZAlign's torch.mean sums in an order that depends on the host.  Given the
reference's own centre every output is compared bit for bit; without it the centre must be the exactly rounded mean
(math.fsum / n, rounded once) and everything else must follow from that centre bit for bit.  numpy's argsort is unstable, so
where a test needs the reference's very picks it hands its tables to the same kernels (tables=...)."""
import numpy as np
import pytest
import torch

import s3dis_eval_ref as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BATCH = 3


@pytest.fixture(scope="module")
def g():
    return load_golden("s3dis_eval")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    """the bit patterns of a float32 array, every NaN as one pattern (which NaN it is, numpy / torch do not specify either)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.int32(0x7fc00000), a.view(np.int32))


def _same(got, want, msg=""):
    """bit-equal float32 arrays (a NaN equals a NaN)"""
    got = _np(got) if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, msg
    np.testing.assert_array_equal(got, want, err_msg=msg)  # NaN == NaN here, -0.0 == 0.0
    assert not (np.signbit(got) != np.signbit(want))[~np.isnan(want)].any(), msg


def _room(g, tag):
    room = ref.fixture_room(g, tag)
    cdata = ref.fixture_cdata(room)
    return room, cdata, cdata[:, :3] - cdata[:, :3].min(0), np.ascontiguousarray(cdata[:, 3:6])


def _check_against_rows(out, j, rec, cols, rows, msg):
    pos, x, heights, inp = ref.fixture_rows(rec, rows)
    _same(out["pos"][j][cols], pos, msg + " pos")
    _same(out["heights"][j][cols], heights, msg + " heights")
    _same(out["x"][j][:, cols], inp, msg + " input")
    _same(out["x"][j, :3].t().contiguous()[cols], x, msg + " x")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_part_batch_test_mode_equals_the_reference_run(g, tag):
    """a: float64 file, b: float32; every sub-cloud of both test modes with the centre the reference's torch.mean returned.
    P (14 / 20) is no multiple of the batch, n (1555 / 995) no multiple of 64 or 256 and more than one workgroup per row"""
    from amcontrast3d_amd import input_pipeline as ip
    room, cdata, shifted, colour = _room(g, tag)
    rows, pick = g["meta"]["rows"], room["pick"].astype(np.int64)
    parts = _dev(room["parts"], torch.int32)
    coord_d, colour_d, label_d = _dev(shifted), _dev(colour), _dev(room["label_u8"], torch.int64)
    assert coord_d.dtype == (torch.float64 if tag == "a" else torch.float32)
    P, n = parts.shape
    assert n % 64 != 0 and n % 256 != 0 and n > 256 and P % BATCH != 0
    full = 0
    for R in (1, BATCH):
        for j0 in range(0, P, R):
            centre = _dev(room["centre"][j0:j0 + R])
            out = ip.s3dis_part_batch(parts[j0:j0 + R], coord_d, colour_d, label_d, "test", centre=centre)
            k = out["pos"].shape[0]
            assert out["x"].shape == (k, 4, n) and out["heights"].shape == (k, n, 1) and out["y"].dtype == torch.int64
            assert torch.equal(out["centre"], centre)
            for j in range(k):
                i = j0 + j
                _check_against_rows(out, j, room[f"rows/{i}"], pick, rows, f"{tag} part {i} R={R}")
                if f"full/{i}" in room:
                    _check_against_rows(out, j, room[f"full/{i}"], slice(None), rows, f"{tag} full part {i} R={R}")
                    full += 1
                np.testing.assert_array_equal(_np(out["y"][j]), room["label_u8"][room["parts"][i]])
    assert full == 2 * len(g["meta"]["full"][tag])
    nn = ip.s3dis_part_batch(_dev(room["nn/part"], torch.int32).view(1, -1), coord_d, colour_d, None, "test",
                             centre=_dev(room["nn/centre"]).view(1, 3))
    assert "y" not in nn
    _check_against_rows(nn, 0, room["nn/rows"], pick, rows, f"{tag} nearest-neighbour part")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_part_batch_val_mode_equals_the_reference_run(g, tag):
    """the val item's arithmetic on the reference's own picks: a takes the / 255 branch, b (dark) does not"""
    from amcontrast3d_amd import input_pipeline as ip
    room, cdata, _, _ = _room(g, tag)
    c32 = cdata.astype(np.float32)
    shifted = c32[:, :3] - c32[:, :3].min(0)
    out = ip.s3dis_part_batch(_dev(room["val/idx_unique"], torch.int32).view(1, -1), _dev(shifted), _dev(c32[:, 3:6]),
                              _dev(room["label_u8"], torch.int64), "val", centre=_dev(room["val/centre"]).view(1, 3))
    _check_against_rows(out, 0, room["val/full"], slice(None), g["meta"]["rows"], f"{tag} val")
    np.testing.assert_array_equal(_np(out["y"][0]), room["val/y"])
    if tag == "a":
        with pytest.raises(ValueError):  # the val item is float32
            ip.s3dis_part_batch(_dev(room["val/idx_unique"], torch.int32).view(1, -1), _dev(shifted).double(),
                                _dev(c32[:, 3:6]).double(), None, "val")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_part_batch_own_centre(g, tag):
    """without `centre`: the exactly rounded mean, within the fixture's recorded distance of torch.mean's; every other output
    is the restatement's with that centre; two runs give the same bits"""
    from amcontrast3d_amd import input_pipeline as ip
    room, cdata, shifted, colour = _room(g, tag)
    parts = room["parts"].astype(np.int64)
    coord_d, colour_d = _dev(shifted), _dev(colour)
    out = ip.s3dis_part_batch(_dev(parts, torch.int32), coord_d, colour_d, None, "test")
    again = ip.s3dis_part_batch(_dev(parts, torch.int32), coord_d, colour_d, None, "test")
    worst = 0
    for i in range(len(parts)):
        pos, x, heights, centre = ref.sub_cloud(shifted, colour, parts[i], "test")
        got_centre = _np(out["centre"][i])
        assert np.array_equal(_bits(got_centre), _bits(centre)), (i, got_centre, centre)
        d = ref.ulp_distance(got_centre, room["centre"][i])
        worst = max(worst, d)
        _same(out["pos"][i], pos, f"pos {i}")
        _same(out["heights"][i], heights, f"heights {i}")
        _same(out["x"][i], ref.assemble(pos, x, heights), f"input {i}")
    print(f"{tag}: own centre within {worst} ulp of torch.mean's (recorded: {g['meta']['centre_ulp']})")
    assert worst <= g["meta"]["centre_ulp"]
    for k in ("pos", "x", "heights", "centre"):
        assert torch.equal(out[k].view(torch.int32), again[k].view(torch.int32)), k
    # the val item
    c32 = cdata.astype(np.float32)
    sh32, col32 = c32[:, :3] - c32[:, :3].min(0), np.ascontiguousarray(c32[:, 3:6])
    pick = room["val/idx_unique"].astype(np.int64)
    val = ip.s3dis_part_batch(_dev(pick, torch.int32).view(1, -1), _dev(sh32), _dev(col32), None, "val")
    pos, x, heights, centre = ref.sub_cloud(sh32, col32, pick, "val")
    assert np.array_equal(_bits(_np(val["centre"][0])), _bits(centre))
    assert ref.ulp_distance(centre, room["val/centre"]) <= g["meta"]["centre_ulp"]
    _same(val["pos"][0], pos)
    _same(val["x"][0], ref.assemble(pos, x, heights))


def _synthetic(n, R, dtype, seed):
    """a room of 9000 points and R rows of n indices into it (with repeats); float64 coordinates are no float32 numbers"""
    rng = np.random.default_rng(seed)
    N = 9000
    coord = (rng.uniform(0, 6, (N, 3)) + np.array([0.0, 0.0, 0.5])).astype(dtype)
    coord[rng.integers(0, N, 40)] *= 0.01  # some points near the corner: small next to the centre
    colour = np.rint(rng.uniform(0, 255, (N, 3))).astype(dtype)
    label = rng.integers(0, 13, N).astype(np.int64)
    idx = rng.integers(0, N - 2, (R, n))  # the last two points are kept for the NaN rows
    return coord, colour, label, idx


_CASES = [(1, 2, "x,heights", "test"), (3, 0, "pos,x,heights", "test"), (3, 2, "x", "test")]
_VAL_CASES = [(1, 0, "heights,pos", "val"), (3, 2, "x,heights", "val")]  # the val item is float32 by definition


@pytest.mark.parametrize("n", [37, 257, 8200])
@pytest.mark.parametrize("dtype,R,g_dim,keys,mode", [(np.float32,) + c for c in _CASES + _VAL_CASES] +
                         [(np.float64,) + c for c in _CASES])
def test_part_batch_shapes_against_the_restatement(n, dtype, R, g_dim, keys, mode):
    """n = 37: less than a wave; 257: one thread into the second workgroup; 8200: more than one trip of the 32 x 256 strided
    statistics passes.  With R = 3, row 0 holds a NaN coordinate and row 1 a NaN colour: NaN where numpy / torch make it
    NaN, and row 2 does not notice."""
    from amcontrast3d_amd import input_pipeline as ip
    coord, colour, label, idx = _synthetic(n, R, dtype, 1000 * n + R)
    N = len(coord)
    if R == 3:
        coord[N - 1, g_dim] = np.nan
        colour[N - 2, 1] = np.nan
        idx[0, n // 2] = N - 1
        idx[1, n // 3] = N - 2
    out = ip.s3dis_part_batch(_dev(idx, torch.int32), _dev(coord), _dev(colour), _dev(label), mode, gravity_dim=g_dim,
                              feature_keys=keys)
    cx = sum(1 if k == "heights" else 3 for k in keys.split(","))
    assert out["pos"].shape == (R, n, 3) and out["x"].shape == (R, cx, n) and out["heights"].shape == (R, n, 1)
    for r in range(R):
        pos, x, heights, centre = ref.sub_cloud(coord, colour, idx[r], mode, gravity_dim=g_dim)
        assert np.array_equal(_bits(_np(out["centre"][r])), _bits(centre)), (r, _np(out["centre"][r]), centre)
        _same(out["pos"][r], pos, f"pos row {r}")
        _same(out["heights"][r], heights, f"heights row {r}")
        _same(out["x"][r], ref.assemble(pos, x, heights, keys), f"input row {r}")
        np.testing.assert_array_equal(_np(out["y"][r]), label[idx[r]])
    if R == 3:
        pos0, x1 = _np(out["pos"][0]), _np(out["x"][1])
        assert np.isnan(pos0[:, g_dim]).all() and np.isnan(_np(out["centre"][0])[g_dim])
        others = [c for c in range(3) if c != g_dim]
        assert np.isfinite(pos0[:, others]).all() and np.isfinite(_np(out["pos"][1:])).all()
        assert np.isfinite(_np(out["x"][2])).all() and np.isfinite(_np(out["centre"][1:])).all()
        if "x" in keys.split(","):
            assert np.isnan(x1).sum() == 1  # NaN > 1 is false: the row does not divide, and only the element stays NaN


def test_part_batch_never_reads_outside_the_room():
    """an index outside [0, N) is skipped as part_batch skips it: nothing is read, the row's other points are what they are
    without it"""
    from amcontrast3d_amd import input_pipeline as ip
    coord, colour, label, idx = _synthetic(300, 2, np.float32, 5)
    N = len(coord)
    bad = idx.copy()
    holes = np.array([0, 17, 255, 256, 299])
    bad[0, holes] = [N, -1, 2 ** 31 - 1, -2 ** 31, N + 1]
    out = ip.s3dis_part_batch(_dev(bad, torch.int32), _dev(coord), _dev(colour), _dev(label), "test")
    torch.cuda.synchronize()
    keep = np.setdiff1d(np.arange(300), holes)
    pos, x, heights, centre = ref.sub_cloud(coord, colour, idx[0][keep], "test")
    assert np.array_equal(_bits(_np(out["centre"][0])), _bits(centre))
    _same(out["pos"][0][keep], pos)
    _same(out["x"][0][:, keep], ref.assemble(pos, x, heights))
    pos, x, heights, centre = ref.sub_cloud(coord, colour, idx[1], "test")
    _same(out["pos"][1], pos)
    with pytest.raises(ValueError):
        ip.s3dis_part_batch(_dev(idx, torch.int32), _dev(coord), _dev(colour), None, "test", feature_keys="x,normals")
    with pytest.raises(RuntimeError):
        ip.s3dis_part_batch(_dev(idx, torch.int32).cpu(), _dev(coord), _dev(colour), None, "test")
    with pytest.raises(RuntimeError):
        ip.s3dis_part_batch(_dev(idx, torch.int32), _dev(coord), _dev(colour).double(), None, "test")
    with pytest.raises(ValueError):
        ip.s3dis_part_batch(_dev(idx, torch.int32), _dev(coord), _dev(colour), None, "test", centre=torch.zeros(1, 3, device=DEV))


def _nn_tables(room):
    return {"idx_sort": room["idx_sort"], "count": room["count"], "voxel_idx": room["voxel_idx"]}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_room_representatives_and_expand_parts_equal_the_reference_run(g, tag):
    from amcontrast3d_amd import input_pipeline as ip, ops
    room, cdata, shifted, _ = _room(g, tag)
    rp = ip.room_representatives(_dev(shifted), ref.VOXEL, rnd=room["nn/rnd"], perm=room["nn/perm"], tables=_nn_tables(room))
    nvox = len(room["count"])
    assert rp["parts"].shape == rp["where"].shape == (1, nvox) and rp["parts"].dtype == rp["where"].dtype == torch.int32
    np.testing.assert_array_equal(_np(rp["parts"][0]), room["nn/part"])
    np.testing.assert_array_equal(_np(rp["where"][0]), room["nn/where"])
    C = 13
    logits = (np.random.default_rng(2).standard_normal((1, C, nvox)) * 4).astype(np.float32)
    logits[0, :, 11] = 1.25       # a tie: the first maximum
    logits[0, 5, 23] = np.nan     # a NaN counts as the maximum
    voted, pred = ops.expand_parts(_dev(logits), rp)
    N = len(cdata)
    assert voted.shape == (N, C) and voted.dtype == torch.float32 and pred.shape == (N,) and pred.dtype == torch.int64
    expand = room["nn/expand"].astype(np.int64)  # main.py:605 on the sub-cloud's positions
    want = np.ascontiguousarray(logits[0].T[expand])
    _same(voted, want)
    np.testing.assert_array_equal(_np(pred), torch.from_numpy(want).argmax(dim=1).numpy())
    assert (_np(pred)[expand == 11] == 0).all() and (_np(pred)[expand == 23] == 5).all() and (expand == 23).any()
    with pytest.raises(ValueError):
        ops.expand_parts(_dev(logits)[:, :, :-1], rp)
    with pytest.raises(ValueError):
        ip.room_representatives(_dev(shifted), ref.VOXEL, rnd=room["nn/rnd"], perm=room["nn/where"] * 0, tables=_nn_tables(room))
    # on the device's own tables and draws: one point of every voxel, `where` the inverse of the order
    own = ip.room_representatives(_dev(shifted), ref.VOXEL, generator=torch.Generator(device=DEV).manual_seed(4))
    idx_sort, voxel_idx, start, count = ref.stable_tables(shifted)
    voxel_of = np.empty(N, np.int64)
    voxel_of[idx_sort] = voxel_idx
    v = voxel_of[_np(own["parts"][0])]
    assert np.array_equal(np.sort(v), np.arange(nvox)) and np.array_equal(_np(own["where"][0])[v], np.arange(nvox))
    assert len(np.unique(np.diff(v))) > 2  # shuffled


@pytest.mark.parametrize("tag", ["a", "b"])
def test_s3dis_val_cloud(g, tag):
    """the val item from the raw array, with the logged randint draw, the reference's tables and torch.mean's centre: a is a
    float64 file (cast on loading) and takes the / 255 branch, b does not"""
    from amcontrast3d_amd import input_pipeline as ip
    room, cdata, _, _ = _room(g, tag)
    tables = {"idx_sort": room["val/idx_sort"], "count": room["val/count"]}
    out = ip.s3dis_val_cloud(_dev(cdata), ref.VOXEL, rnd=room["val/rnd"], centre=_dev(room["val/centre"]).view(1, 3), tables=tables)
    n = len(room["val/idx_unique"])
    assert out["pos"].shape == (1, n, 3) and out["x"].shape == (1, 4, n) and out["heights"].shape == (1, n, 1)
    assert out["y"].shape == (1, n) and out["y"].dtype == torch.int64
    _check_against_rows(out, 0, room["val/full"], slice(None), g["meta"]["rows"], f"{tag} val cloud")
    np.testing.assert_array_equal(_np(out["y"][0]), room["val/y"])
    # on the device's own voxelisation and draw: one point of every voxel, its own centre
    own = ip.s3dis_val_cloud(_dev(cdata), ref.VOXEL, generator=torch.Generator(device=DEV).manual_seed(1))
    assert own["pos"].shape == (1, n, 3) and float(own["pos"][0, :, 2].min()) == 0.0
    assert float(own["pos"][0, :, :2].mean().abs()) < 1e-4


@torch.no_grad()
def _calibrate_head(model, data):
    """An untrained head gives every point of a room the same class, and equal predictions would then say little.  The last
    layer is rescaled so that every class's logit has mean 0 and deviation 1 over the points of `data`."""
    from amcontrast3d_amd import evaluate
    lg = evaluate._logits(model(data))
    mean, std = lg.mean(dim=(0, 2)), lg.std(dim=(0, 2)).clamp_min(1e-6)
    last = model.head.head[-1][0]
    last.bias.copy_((last.bias - mean) / std)
    last.weight.div_(std.view(-1, 1, 1))


def _model(name):
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from test_baseline_host import as_amcontrast3d, build, pointnext_xl
    cfg = pointnext_xl("s3dis", width=8, blocks=(1, 1, 1, 1, 1))
    torch.manual_seed(11)
    model = build(cfg if name == "BaseSeg" else as_amcontrast3d(cfg)).to(DEV)
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():  # running statistics away from their initial values, as a trained model has them
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
    return model.eval()


@pytest.mark.parametrize("name,test_mode", [("AMContrast3D", "multi_voxel"), ("AMContrast3D", "nearest_neighbor"),
                                            ("BaseSeg", "multi_voxel")])
def test_room_s3dis_end_to_end(g, name, test_mode):
    """against the existing test_cloud_boundary_inner on the same sub-clouds, the same `batch` and a host make_input that
    applies the restatement (pinned to the reference run); room a of the fixture as a float64 file"""
    from amcontrast3d_amd import evaluate, input_pipeline as ip, ops
    model = _model(name)
    room, cdata, shifted, colour = _room(g, "a")
    N = len(cdata)
    coord_d, colour_d = _dev(shifted), _dev(colour)
    label_d = _dev(room["label_u8"], torch.int64)
    ncls, ignore, nsample = 13, None, 16
    nn = test_mode == "nearest_neighbor"
    gen = torch.Generator(device=DEV).manual_seed(5)
    if nn:
        rp = ip.room_representatives(coord_d, ref.VOXEL, generator=gen)
        split = {"rnd": None, "perm": None}
        # the draws as arguments, so that test_room_s3dis splits the room the same way
        v = torch.empty(N, dtype=torch.int64, device=DEV)
        v[rp["idx_sort"].long()] = rp["voxel_idx"].long()
        rank = torch.empty(N, dtype=torch.int64, device=DEV)
        rank[rp["idx_sort"].long()] = torch.arange(N, device=DEV) - rp["start"].long()[rp["voxel_idx"].long()]
        perm = v[rp["parts"][0].long()]
        rnd = torch.empty(len(perm), dtype=torch.int64, device=DEV)
        rnd[perm] = rank[rp["parts"][0].long()]
        split = {"rnd": rnd, "perm": perm}
    else:
        rp = ip.room_parts(coord_d, ref.VOXEL, generator=gen)
        v = torch.empty(N, dtype=torch.int64, device=DEV)
        v[rp["idx_sort"].long()] = rp["voxel_idx"].long()
        split = {"perm": v[rp["parts"].long()]}
    P, nvox = rp["parts"].shape
    assert (P == 1 if nn else (P >= 5 and P % BATCH != 0)) and nvox > 1024
    _calibrate_head(model, ip.s3dis_part_batch(rp["parts"][:1], coord_d, colour_d, None, "test"))
    new = evaluate.test_room_s3dis(model, cdata, ref.VOXEL, ncls, ignore, nsample, miou_B_I=True, batch=BATCH, test_mode=test_mode,
                                   **split)

    def make_input(coord_part, feat_part):
        x = np.clip(feat_part / 255., 0, 1).astype(np.float32)  # load_data, in the file's dtype
        pos, x, heights, _ = ref.align_normalize(coord_part, x)
        data = {"pos": torch.from_numpy(pos).unsqueeze(0),
                "x": torch.from_numpy(ref.assemble(pos, x, heights)).unsqueeze(0)}
        return {k: v.to(DEV) for k, v in data.items()}
    parts = [p for p in _np(rp["parts"]).astype(np.int64)]
    expand = None
    if nn:
        expand = _np(rp["where"][0].long()[v])
    old = evaluate.test_cloud_boundary_inner(model, shifted, colour, label_d, parts, ncls, ignore, nsample,
                                             make_input=make_input, miou_B_I=True, batch=BATCH, expand=expand)
    # per-sub-cloud inputs identical, logits within 1e-5 of their range
    logits, worst = [], 0.0
    with torch.no_grad():
        for j0 in range(0, P, BATCH):
            data = ip.s3dis_part_batch(rp["parts"][j0:j0 + BATCH], coord_d, colour_d, label_d, "test")
            host = [make_input(shifted[p] - shifted[p].min(0), colour[p]) for p in parts[j0:j0 + BATCH]]
            host = {k: torch.cat([h[k] for h in host]) for k in ("pos", "x")}
            assert torch.equal(data["pos"], host["pos"]) and torch.equal(data["x"], host["x"])
            lg, lg_host = evaluate._logits(model(data)), evaluate._logits(model(host))
            worst = max(worst, float((lg - lg_host).abs().max() / (lg_host.max() - lg_host.min())))
            logits.append(lg)
    logits = torch.cat(logits)
    print(f"{name} {test_mode}: P={P} nvox={nvox} per-sub-cloud logits differ by {worst:.2e} of their range")
    assert worst <= 1e-5
    t = {k: _np(t_).astype(np.int64) for k, t_ in rp.items()}
    if nn:
        want = _np(logits[0].t()[rp["where"][0].long()[v]])
        _same(new["logits"], np.ascontiguousarray(want))
        assert torch.equal(new["logits"], old["logits"]) and torch.equal(new["pred"], old["pred"])
        assert torch.equal(new["logits"], ops.expand_parts(logits, rp)[0])
        assert torch.equal(new["cm"].value, old["cm"].value)
    else:
        # the voted logits are the fixed-order vote of the per-sub-cloud logits, bit for bit, within the documented bound of
        # the exact mean ...
        want, mag, k = ref.vote(_np(logits), t["where"], t["start"], t["count"], t["idx_sort"], t["voxel_idx"])
        exact = ref.vote(_np(logits), t["where"], t["start"], t["count"], t["idx_sort"], t["voxel_idx"], np.float64)[0]
        _same(new["logits"], want)
        bound = ref.vote_bound(mag, k)
        err = np.abs(want.astype(np.float64) - exact)
        assert (err <= bound).all()
        # ... and so within twice the bound of the old path's, which sums in an unspecified order
        diff = np.abs(want.astype(np.float64) - _np(old["logits"]).astype(np.float64))
        print(f"largest |new - exact| / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}, "
              f"|new - old| / (2 bound) {float((diff / np.maximum(2 * bound, 1e-300)).max()):.3f}")
        assert (diff <= 2 * bound).all()
        top2 = np.sort(want.astype(np.float64), axis=1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 2 * bound.max(axis=1)
        assert clear.mean() > 0.9
        assert np.array_equal(_np(new["pred"])[clear], _np(old["pred"])[clear])
        assert np.abs(_np(new["cm"].value) - _np(old["cm"].value)).sum() <= 2 * int((~clear).sum())
    assert torch.equal(new["pred"], new["logits"].argmax(dim=1))
    # boundary / inner: per-sub-cloud predictions, no vote involved
    for tag in ("cm_b", "cm_i"):
        assert torch.equal(new[tag].value, old[tag].value), tag
    assert int(new["cm_b"].value.sum()) > 0 and int(new["cm_b"].value.sum() + new["cm_i"].value.sum()) == P * nvox
    assert int(new["cm"].value.sum()) == N and len(torch.unique(new["pred"])) > 1
    # a room without labels: predictions and no matrices; two runs give the same bits
    bare = evaluate.test_room_s3dis(model, cdata[:, :6], ref.VOXEL, ncls, ignore, nsample, batch=BATCH, test_mode=test_mode, **split)
    assert bare["cm"] is None and bare["cm_b"] is None and bare["cm_i"] is None
    assert torch.equal(bare["pred"], new["pred"]) and torch.equal(bare["logits"].view(torch.int32), new["logits"].view(torch.int32))
    with pytest.raises(ValueError):
        evaluate.test_room_s3dis(model, cdata, ref.VOXEL, ncls, ignore, nsample, variable=True)
    with pytest.raises(ValueError):
        evaluate.test_room_s3dis(model, cdata[:, :6], ref.VOXEL, ncls, ignore, nsample, miou_B_I=True)
