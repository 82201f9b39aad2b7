"""ScanNet validation and whole-room testing on the device (csrc/room_eval.hip; input_pipeline.room_parts / part_batch /
scannet_val_cloud, ops.vote_parts, evaluate.test_room_scannet) against what the reference's own code returned for the same
rooms (tests/golden/scannet_eval.npz, recorded by tests/tools/gen_golden_scannet_eval.py) and against the numpy restatements
of tests/scannet_eval_ref.py, which tests/test_scannet_eval_host.py pins to that fixture.

Everything the reference specifies is compared bit for bit.  numpy's argsort is unstable, so the order of the points inside
one voxel is the reference's to choose: where a test needs the reference's very picks it hands its tables / picks to the same
kernels (room_parts(tables=...), part_batch on val/idx_unique); where the device voxelises on its own, the restatement on the
device's (stable) picks stands in.  The vote's bound follows from its arithmetic (scannet_eval_ref.vote_bound)."""
import numpy as np
import pytest
import torch

import scannet_eval_ref as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KEYS = ["pos,x,heights", "x,heights", "x", "pos,x"]


@pytest.fixture(scope="module")
def g():
    return load_golden("scannet_eval")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _fixture_parts(room):
    """room_parts on the reference's own tables and shuffles"""
    from amcontrast3d_amd import input_pipeline as ip
    shifted = _dev(room["coord"] - room["coord"].min(0))
    perm, _ = ref.fixture_perm(room)
    tables = {"idx_sort": room["idx_sort"], "count": room["count"], "voxel_idx": room["voxel_idx"]}
    return shifted, perm, ip.room_parts(shifted, ref.VOXEL, perm=perm, tables=tables)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_room_parts_equal_the_reference_run(g, tag):
    room = ref.fixture_room(g, tag)
    shifted, perm, rp = _fixture_parts(room)
    assert rp["parts"].dtype == rp["where"].dtype == torch.int32
    np.testing.assert_array_equal(rp["parts"].cpu().numpy(), room["parts"])
    where = rp["where"].cpu().numpy()
    P, nvox = perm.shape
    rows = np.arange(P)[:, None]
    np.testing.assert_array_equal(perm[rows, where], np.broadcast_to(np.arange(nvox), (P, nvox)))  # the inverse permutation
    np.testing.assert_array_equal(where, np.argsort(perm, axis=1))


def test_room_parts_on_its_own_tables(g):
    """what the reference specifies, on the device's own (stable) voxelisation and its own shuffles: every part holds exactly
    one point of every voxel, and the point of voxel v in part i is the (i mod c)-th of that voxel"""
    from amcontrast3d_amd import input_pipeline as ip
    room = ref.fixture_room(g, "a")
    shifted_np = room["coord"] - room["coord"].min(0)
    gen = torch.Generator(device=DEV).manual_seed(3)
    rp = ip.room_parts(_dev(shifted_np), ref.VOXEL, generator=gen)
    idx_sort, voxel_idx, start, count = ref.stable_tables(shifted_np)
    for k, want in (("idx_sort", idx_sort), ("voxel_idx", voxel_idx), ("start", start), ("count", count)):
        assert rp[k].dtype == torch.int32
        np.testing.assert_array_equal(rp[k].cpu().numpy(), want, err_msg=k)
    parts, where = rp["parts"].cpu().numpy(), rp["where"].cpu().numpy()
    P, nvox = int(count.max()), len(count)
    assert parts.shape == where.shape == (P, nvox)
    voxel_of = np.empty(len(shifted_np), np.int64)
    voxel_of[idx_sort] = voxel_idx
    rank_of = np.empty(len(shifted_np), np.int64)
    rank_of[idx_sort] = np.arange(len(shifted_np)) - start[voxel_idx]
    for i in range(P):
        v = voxel_of[parts[i]]
        assert np.array_equal(np.sort(v), np.arange(nvox)), i                 # one point of every voxel
        assert np.array_equal(rank_of[parts[i]], i % count[v]), i             # the (i mod c)-th of it
        assert np.array_equal(where[i, v], np.arange(nvox)), i                # where: voxel -> slot
    assert len({tuple(voxel_of[p].tolist()) for p in parts}) == P             # the parts are shuffled independently
    assert np.array_equal(np.unique(parts), np.arange(len(shifted_np)))       # every room point occurs
    # the same generator state gives the same parts; a given perm that is no permutation is refused
    again = ip.room_parts(_dev(shifted_np), ref.VOXEL, generator=torch.Generator(device=DEV).manual_seed(3))
    assert torch.equal(again["parts"], rp["parts"]) and torch.equal(again["where"], rp["where"])
    bad = voxel_of[parts].copy()
    bad[1, 0] = bad[1, 1]
    with pytest.raises(ValueError):
        ip.room_parts(_dev(shifted_np), ref.VOXEL, perm=bad)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_part_batch_test_mode_equals_the_reference_run(g, tag):
    """R = 1, 3 and P rows per call; n (1295 / 372) is no multiple of 64 or of the workgroup size, a: more than one workgroup
    per row"""
    from amcontrast3d_amd import input_pipeline as ip
    room = ref.fixture_room(g, tag)
    shifted, _, rp = _fixture_parts(room)
    feat, label = _dev(room["feat"]), _dev(room["label"])
    P, n = rp["parts"].shape
    assert n % 64 != 0 and n % 256 != 0 and P >= 3
    for R in (1, 3, P):
        for j0 in range(0, P, R):
            out = ip.part_batch(rp["parts"][j0:j0 + R], shifted, feat, label, "test")
            rows = out["pos"].shape[0]
            assert out["x"].shape == (rows, 7, n) and out["heights"].shape == (rows, n, 1) and out["y"].dtype == torch.int64
            for j in range(rows):
                pos, x, heights, inp = ref.fixture_part(room, g["meta"]["rows"], j0 + j)
                np.testing.assert_array_equal(out["pos"][j].cpu().numpy(), pos)
                np.testing.assert_array_equal(out["heights"][j].cpu().numpy(), heights)
                np.testing.assert_array_equal(out["x"][j].cpu().numpy(), inp)
                np.testing.assert_array_equal(out["x"][j, 3:6].t().cpu().numpy(), x)
                np.testing.assert_array_equal(out["y"][j].cpu().numpy(), room["label"][room["parts"][j0 + j]])
    assert "y" not in ip.part_batch(rp["parts"][:1], shifted, feat, None, "test")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_part_batch_val_mode_equals_the_reference_run(g, tag):
    """the val item's arithmetic on the reference's own picks: a takes the / 255 branch, b (dark) does not"""
    from amcontrast3d_amd import input_pipeline as ip
    room = ref.fixture_room(g, tag)
    shifted = _dev(room["coord"] - room["coord"].min(0))
    out = ip.part_batch(_dev(room["val/idx_unique"], torch.int32).view(1, -1), shifted, _dev(room["feat"]), _dev(room["label"]),
                        "val")
    np.testing.assert_array_equal(out["pos"][0].cpu().numpy(), room["val/pos"])
    np.testing.assert_array_equal(out["heights"][0].cpu().numpy(), room["val/heights"])
    np.testing.assert_array_equal(out["x"][0].cpu().numpy(), room["val/input"])
    np.testing.assert_array_equal(out["x"][0, 3:6].t().cpu().numpy(), room["val/x"])
    np.testing.assert_array_equal(out["y"][0].cpu().numpy(), room["val/y"])


@pytest.mark.parametrize("mode", ["test", "val"])
@pytest.mark.parametrize("keys", KEYS)
def test_part_batch_feature_keys_against_torch(g, keys, mode):
    """get_features_by_keys restated with torch.cat on the kernel's own pos / x / heights (pinned above), every order; the
    dark room's sub-clouds in val mode decide `/ 255` row by row, and a NaN colour propagates as numpy's max() has it"""
    from amcontrast3d_amd import input_pipeline as ip
    room = ref.fixture_room(g, "b")
    shifted, _, rp = _fixture_parts(room)
    feat_np = room["feat"].copy()
    bright = room["parts"][1][5]
    feat_np[bright] = 0.5                      # one bright point: only the rows that hold it divide by 255
    feat_np[room["parts"][2][7], 1] = np.nan   # NaN > 1 is false: the rows that hold it do not divide, and stay NaN there
    feat = _dev(feat_np)
    full = ip.part_batch(rp["parts"], shifted, feat, None, mode)
    out = ip.part_batch(rp["parts"], shifted, feat, None, mode, feature_keys=keys)
    named = {"pos": full["pos"], "x": full["x"][:, 3:6].transpose(1, 2), "heights": full["heights"]}
    want = torch.cat([named[k] for k in keys.split(",")], -1).transpose(1, 2).contiguous()
    assert out["x"].shape == want.shape and torch.equal(out["x"].view(torch.int32), want.view(torch.int32))
    assert torch.equal(out["pos"], full["pos"]) and torch.equal(out["heights"], full["heights"])
    shifted_np = room["coord"] - room["coord"].min(0)
    took = set()
    for i, part in enumerate(room["parts"]):
        pos, x, heights = ref.sub_cloud(shifted_np, feat_np, part, mode)
        np.testing.assert_array_equal(full["x"][i].cpu().numpy(), ref.assemble(pos, x, heights), err_msg=str(i))
        raw = (feat_np[part] + 1) * 127.5
        took.add(bool(raw.max() > 1))
    assert mode == "test" or took == {True, False}
    with pytest.raises(ValueError):
        ip.part_batch(rp["parts"], shifted, feat, None, mode, feature_keys="x,normals")
    with pytest.raises(RuntimeError):
        ip.part_batch(rp["parts"].cpu(), shifted, feat, None, mode)


def _same(got, want, msg=""):
    """bit-equal float32 arrays (a NaN equals a NaN)"""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, msg
    np.testing.assert_array_equal(got, want, err_msg=msg)  # NaN == NaN here, -0.0 == 0.0
    assert not (np.signbit(got) != np.signbit(want))[~np.isnan(want)].any(), msg


N_DARK = 500  # the first points of the synthetic room: (f + 1) * 127.5 <= 1 for every colour


def _synthetic(n, R, seed, dark_last_row=False):
    """a room of 9000 fp32 points, colours in [-1, 1], and R rows of n indices into it (with repeats); the last row draws from
    the dark points alone when asked to"""
    rng = np.random.default_rng(seed)
    N = 9000
    coord = (rng.uniform(0, 6, (N, 3)) + np.array([0.0, 0.0, 0.5])).astype(np.float32)
    feat = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    feat[:N_DARK] = (-1 + rng.uniform(0, 0.9 / 127.5, (N_DARK, 3))).astype(np.float32)
    label = rng.integers(0, 20, N).astype(np.int64)
    idx = rng.integers(N_DARK, N - 2, (R, n))  # the last two points are kept for the NaN rows
    if dark_last_row:
        idx[R - 1] = rng.integers(0, N_DARK, n)
    return coord, feat, label, idx


def _shape_case(n, R, g_dim, mode):
    """the inputs of test_part_batch_shapes_against_the_restatement: with R = 3, row 0 holds a NaN coordinate in the gravity
    column, row 1 a NaN colour, and in val mode row 2 only dark points"""
    coord, feat, label, idx = _synthetic(n, R, 1000 * n + R, dark_last_row=R == 3 and mode == "val")
    N = len(coord)
    if R == 3:
        coord[N - 1, g_dim] = np.nan
        feat[N - 2, 1] = np.nan
        idx[0, n // 2] = N - 1
        idx[1, n // 3] = N - 2
    return coord, feat, label, idx


def _divides(feat, row, mode):
    """whether NumpyChromaticNormalize divides the row by 255 (a NaN maximum: not)"""
    x = np.clip((feat[row] + 1) / 2., 0, 1) if mode == "test" else (feat[row] + 1) * 127.5
    return bool(x.max() > 1)


_SHAPE_CASES = [(1, 0, "heights,pos", "val"), (3, 2, "pos,x,heights", "test"), (3, 1, "x", "val")]


@pytest.mark.parametrize("n", [37, 257, 8200])
@pytest.mark.parametrize("R,g_dim,keys,mode", _SHAPE_CASES)
def test_part_batch_shapes_against_the_restatement(n, R, g_dim, keys, mode):
    """n = 37: less than a wave; 257: one thread into the second workgroup; 8200: more than one trip of the 32 x 256 strided
    statistics pass.  With R = 3, row 0 holds a NaN coordinate and row 1 a NaN colour: NaN where numpy makes it NaN, and row 2
    does not notice.  In val mode both arms of the `/ 255` test run: bright rows divide, the NaN row and the dark row do not."""
    from amcontrast3d_amd import input_pipeline as ip
    coord, feat, label, idx = _shape_case(n, R, g_dim, mode)
    out = ip.part_batch(_dev(idx, torch.int32), _dev(coord), _dev(feat), _dev(label), mode, gravity_dim=g_dim, feature_keys=keys)
    cx = sum(1 if k == "heights" else 3 for k in keys.split(","))
    assert out["pos"].shape == (R, n, 3) and out["x"].shape == (R, cx, n) and out["heights"].shape == (R, n, 1)
    for r in range(R):
        pos, x, heights = ref.sub_cloud(coord, feat, idx[r], mode, gravity_dim=g_dim)
        _same(out["pos"][r], pos, f"pos row {r}")
        _same(out["heights"][r], heights, f"heights row {r}")
        _same(out["x"][r], ref.assemble(pos, x, heights, keys), f"input row {r}")
        np.testing.assert_array_equal(out["y"][r].cpu().numpy(), label[idx[r]])
    divides = [_divides(feat, idx[r], mode) for r in range(R)]
    assert divides == {(1, "val"): [True], (3, "test"): [False] * 3, (3, "val"): [True, False, False]}[R, mode]
    if R == 3:
        pos0, x1 = out["pos"][0].cpu().numpy(), out["x"][1].cpu().numpy()
        assert np.isnan(pos0[:, g_dim]).all()
        others = [c for c in range(3) if c != g_dim]
        assert np.isfinite(pos0[:, others]).all() and np.isfinite(out["pos"][1:].cpu().numpy()).all()
        assert np.isfinite(out["x"][2].cpu().numpy()).all() and np.isfinite(out["heights"][1:].cpu().numpy()).all()
        if "x" in keys.split(","):
            assert np.isnan(x1).sum() == 1  # NaN > 1 is false: the row does not divide, and only the element stays NaN


def test_part_batch_never_reads_outside_the_room():
    """an index outside [0, N) is skipped: nothing is read, and the row's other points are what they are without it"""
    from amcontrast3d_amd import input_pipeline as ip
    coord, feat, label, idx = _synthetic(300, 2, 5)
    N = len(coord)
    bad = idx.copy()
    holes = np.array([0, 17, 255, 256, 299])
    bad[0, holes] = [N, -1, 2 ** 31 - 1, -2 ** 31, N + 1]
    out = ip.part_batch(_dev(bad, torch.int32), _dev(coord), _dev(feat), _dev(label), "test")
    torch.cuda.synchronize()
    keep = np.setdiff1d(np.arange(300), holes)
    pos, x, heights = ref.sub_cloud(coord, feat, idx[0][keep], "test")
    _same(out["pos"][0][keep], pos)
    _same(out["heights"][0][keep], heights)
    _same(out["x"][0][:, keep], ref.assemble(pos, x, heights))
    np.testing.assert_array_equal(out["y"][0][keep].cpu().numpy(), label[idx[0][keep]])
    pos, x, heights = ref.sub_cloud(coord, feat, idx[1], "test")
    _same(out["pos"][1], pos)
    _same(out["heights"][1], heights)
    _same(out["x"][1], ref.assemble(pos, x, heights))
    np.testing.assert_array_equal(out["y"][1].cpu().numpy(), label[idx[1]])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_scannet_val_cloud(g, tag):
    """the val item with the logged randint draw.  Which point of a voxel the draw lands on follows the order inside the voxel,
    which the reference's unstable sort leaves open: the voxels, and every value wherever the picks agree, are held against
    the fixture itself; the whole item against the restatement (pinned to the fixture on the reference's picks) on the
    device's stable picks.  Labels keep their -100."""
    from amcontrast3d_amd import input_pipeline as ip
    room = ref.fixture_room(g, tag)
    rnd = room["val/rnd"]
    out = ip.scannet_val_cloud((_dev(room["coord"]), _dev(room["feat"]), _dev(room["label"])), ref.VOXEL, rnd=_dev(rnd))
    shifted = room["coord"] - room["coord"].min(0)
    idx_sort, voxel_idx, start, count = ref.stable_tables(shifted)
    pick = idx_sort[start[:-1] + rnd % count]
    voxel_of = np.empty(len(shifted), np.int64)
    voxel_of[idx_sort] = voxel_idx
    assert np.array_equal(voxel_of[pick], voxel_of[room["val/idx_unique"]])
    pos, x, heights = ref.sub_cloud(shifted, room["feat"], pick, "val")
    n = len(pick)
    assert out["pos"].shape == (1, n, 3) and out["x"].shape == (1, 7, n) and out["heights"].shape == (1, n, 1)
    assert out["y"].shape == (1, n) and out["y"].dtype == torch.int64
    np.testing.assert_array_equal(out["pos"][0].cpu().numpy(), pos)
    np.testing.assert_array_equal(out["x"][0].cpu().numpy(), ref.assemble(pos, x, heights))
    np.testing.assert_array_equal(out["heights"][0].cpu().numpy(), heights)
    np.testing.assert_array_equal(out["y"][0].cpu().numpy(), room["label"][pick])
    assert (out["y"] == -100).any()
    same = pick == room["val/idx_unique"]
    assert same.mean() > 0.3
    np.testing.assert_array_equal(out["x"][0, 3:6].t().cpu().numpy()[same], room["val/x"][same])  # colours do not depend on the corner
    if np.array_equal(shifted[pick].min(0), shifted[room["val/idx_unique"]].min(0)):  # the same corner: the same positions
        np.testing.assert_array_equal(out["pos"][0].cpu().numpy()[same], room["val/pos"][same])
    # drawn on the device: one point of every voxel
    own = ip.scannet_val_cloud((_dev(room["coord"]), _dev(room["feat"]), _dev(room["label"])), ref.VOXEL,
                               generator=torch.Generator(device=DEV).manual_seed(1))
    assert own["pos"].shape == (1, n, 3) and float(own["pos"].min()) == 0.0


def _vote_case(C, seed=0):
    from amcontrast3d_amd import input_pipeline as ip
    room = ref.make_room(930, 1500, 3, 41)
    shifted = room[0] - room[0].min(0)
    rp = ip.room_parts(_dev(shifted), ref.VOXEL, generator=torch.Generator(device=DEV).manual_seed(seed))
    P, nvox = rp["parts"].shape
    rng = np.random.default_rng(C)
    logits = (rng.standard_normal((P, C, nvox)) * 4).astype(np.float32)
    return room, rp, logits


@pytest.mark.parametrize("C", [13, 20])
def test_vote_parts(C):
    from amcontrast3d_amd import ops
    room, rp, logits = _vote_case(C)
    P, _, nvox = logits.shape
    N = len(room[0])
    t = {k: v.cpu().numpy().astype(np.int64) for k, v in rp.items()}
    r, c, k_sorted = ref.votes_of(P, t["start"], t["count"], t["voxel_idx"])
    assert P >= 3 and nvox > 256 and N > 256 and len(set(k_sorted.tolist())) >= 3 and (P % t["count"] != 0).any()
    # a row of tied logits and a row with a NaN, each on a point with several votes
    many = np.flatnonzero(k_sorted >= 2)
    s_tie, s_nan = many[0], many[1]
    v_tie, v_nan = t["voxel_idx"][s_tie], t["voxel_idx"][s_nan]
    for i in range(int(r[s_tie]), P, int(c[s_tie])):
        logits[i, :, t["where"][i, v_tie]] = 1.25
    logits[int(r[s_nan]), 5, t["where"][int(r[s_nan]), v_nan]] = np.nan
    want, mag, k = ref.vote(logits, t["where"], t["start"], t["count"], t["idx_sort"], t["voxel_idx"])
    exact = ref.vote(logits, t["where"], t["start"], t["count"], t["idx_sort"], t["voxel_idx"], np.float64)[0]
    lg = _dev(logits)
    voted, pred = ops.vote_parts(lg, rp)
    assert voted.shape == (N, C) and voted.dtype == torch.float32 and pred.shape == (N,) and pred.dtype == torch.int64
    got = voted.cpu().numpy()
    np.testing.assert_array_equal(got, want)                                  # the same fp32 operations in the same order
    p_tie, p_nan = t["idx_sort"][s_tie], t["idx_sort"][s_nan]
    finite = np.ones(N, bool)
    finite[p_nan] = False
    err = np.abs(got[finite].astype(np.float64) - exact[finite])
    bound = ref.vote_bound(mag, k)[finite]
    print(f"C={C} P={P} nvox={nvox}: largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}, votes {sorted(set(k.tolist()))}")
    assert (err <= bound).all()
    assert (err[k[finite] == 1] == 0).all()                                   # a single vote is the logit itself
    want_pred = torch.from_numpy(want).argmax(dim=1).numpy()                  # first maximum; NaN counts as the maximum
    np.testing.assert_array_equal(pred.cpu().numpy(), want_pred)
    assert pred[p_tie].item() == 0 and (got[p_tie] == 1.25).all()
    assert pred[p_nan].item() == 5 and np.isnan(got[p_nan, 5]) and np.isfinite(np.delete(got[p_nan], 5)).all()
    voted2, pred2 = ops.vote_parts(lg, rp)
    assert torch.equal(voted.view(torch.int32), voted2.view(torch.int32)) and torch.equal(pred, pred2)
    with pytest.raises(RuntimeError):
        ops.vote_parts(lg.cpu(), rp)
    with pytest.raises(ValueError):
        ops.vote_parts(lg[:-1], rp)


@torch.no_grad()
def _calibrate_head(model, data):
    """An untrained head gives every point of a room the same class, and equal predictions would then say little.  The last
    layer is rescaled so that every class's logit has mean 0 and deviation 1 over the points of `data`: the classes then
    differ from point to point, as a trained model's do."""
    from amcontrast3d_amd import evaluate
    lg = evaluate._logits(model(data))
    mean, std = lg.mean(dim=(0, 2)), lg.std(dim=(0, 2)).clamp_min(1e-6)
    last = model.head.head[-1][0]
    last.bias.copy_((last.bias - mean) / std)
    last.weight.div_(std.view(-1, 1, 1))


def _models():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from test_baseline_host import as_amcontrast3d, build, pointnext_xl
    cfg = pointnext_xl("scannet", width=8, blocks=(1, 1, 1, 1, 1))
    out = {}
    for name, c in (("BaseSeg", cfg), ("AMContrast3D", as_amcontrast3d(cfg))):
        torch.manual_seed(11)
        model = build(c).to(DEV)
        gen = torch.Generator().manual_seed(12)
        with torch.no_grad():  # running statistics away from their initial values, as a trained model has them
            for m in model.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
                    m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
        out[name] = model.eval()
    return out


@pytest.fixture(scope="module")
def e2e_room():
    room = ref.make_room(940, 2250, 2, 51)
    from amcontrast3d_amd import input_pipeline as ip
    shifted = _dev(room[0]) - _dev(room[0]).min(0).values
    rp = ip.room_parts(shifted, ref.VOXEL, generator=torch.Generator(device=DEV).manual_seed(5))
    # the shuffles as a `perm`, so that test_room_scannet splits the room the same way
    voxel_of = torch.empty(len(room[0]), dtype=torch.int64, device=DEV)
    voxel_of[rp["idx_sort"].long()] = rp["voxel_idx"].long()
    return room, shifted, rp, voxel_of[rp["parts"].long()]


@pytest.mark.parametrize("name", ["BaseSeg", "AMContrast3D"])
def test_room_scannet_end_to_end(e2e_room, name):
    """against the existing test_cloud_boundary_inner on the same sub-clouds, the same `batch` and a host make_input that
    applies the reference's per-sub-cloud steps (the restatement pinned to the reference run)"""
    from amcontrast3d_amd import evaluate, input_pipeline as ip, ops
    model = _models()[name]
    (coord, feat, label), shifted, rp, perm = e2e_room
    P, nvox = rp["parts"].shape
    assert len(coord) == 4500 and P >= 3 and nvox > 1024
    ncls, ignore, nsample, batch = 20, -100, 16, 3
    _calibrate_head(model, ip.part_batch(rp["parts"][:1], shifted, _dev(feat), None, "test"))
    new = evaluate.test_room_scannet(model, coord, feat, label, ref.VOXEL, ncls, ignore, nsample, miou_B_I=True, batch=batch,
                                     perm=perm)
    shifted_np = coord - coord.min(0)
    np.testing.assert_array_equal(shifted.cpu().numpy(), shifted_np)
    test_feat = np.clip((feat + 1) / 2., 0, 1).astype(np.float32)  # load_data

    def make_input(coord_part, feat_part):
        x = torch.from_numpy(feat_part.copy())
        if x.max() > 1:
            x /= 255.
        x = (x - torch.from_numpy(ref.COLOR_MEAN)) / torch.from_numpy(ref.COLOR_STD)
        pos = torch.from_numpy(np.ascontiguousarray(coord_part, dtype=np.float32))
        data = {"pos": pos.unsqueeze(0), "x": torch.cat([pos, x, pos[:, 2:3]], -1).t().contiguous().unsqueeze(0)}
        return {k: v.to(DEV) for k, v in data.items()}
    parts = [p for p in rp["parts"].cpu().numpy().astype(np.int64)]
    label_dev = _dev(label)
    old = evaluate.test_cloud_boundary_inner(model, shifted_np, test_feat, label_dev, parts, ncls, ignore, nsample,
                                             make_input=make_input, miou_B_I=True, batch=batch)
    # per-sub-cloud inputs identical
    logits = []
    with torch.no_grad():
        for j0 in range(0, P, batch):
            data = ip.part_batch(rp["parts"][j0:j0 + batch], shifted, _dev(feat), label_dev, "test")
            for j in range(data["pos"].shape[0]):
                host = make_input(shifted_np[parts[j0 + j]] - shifted_np[parts[j0 + j]].min(0), test_feat[parts[j0 + j]])
                assert torch.equal(data["pos"][j], host["pos"][0]) and torch.equal(data["x"][j], host["x"][0])
            logits.append(evaluate._logits(model(data)))
    logits = torch.cat(logits)
    # the voted logits are the fixed-order vote of the per-sub-cloud logits, bit for bit ...
    t = {k: v.cpu().numpy().astype(np.int64) for k, v in rp.items()}
    want, mag, k = ref.vote(logits.cpu().numpy(), t["where"], t["start"], t["count"], t["idx_sort"], t["voxel_idx"])
    np.testing.assert_array_equal(new["logits"].cpu().numpy(), want)
    assert torch.equal(new["pred"], new["logits"].argmax(dim=1)) and torch.equal(new["logits"], ops.vote_parts(logits, rp)[0])
    # ... and within twice the bound of the old path's, which sums in an unspecified order
    bound = 2 * ref.vote_bound(mag, k)
    diff = np.abs(new["logits"].cpu().numpy().astype(np.float64) - old["logits"].cpu().numpy().astype(np.float64))
    print(f"{name}: P={P} nvox={nvox} largest |new - old| / (2 bound) {float((diff / np.maximum(bound, 1e-300)).max()):.3f}, "
          f"differing entries {int((diff > 0).sum())} of {diff.size}")
    assert (diff <= bound).all()
    # predictions equal wherever the two top voted logits are further apart than that
    top2 = np.sort(want.astype(np.float64), axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * bound.max(axis=1)
    assert clear.mean() > 0.9
    assert np.array_equal(new["pred"].cpu().numpy()[clear], old["pred"].cpu().numpy()[clear])
    assert np.abs(new["cm"].value.cpu().numpy() - old["cm"].value.cpu().numpy()).sum() <= 2 * int((~clear).sum())
    # boundary / inner: per-sub-cloud predictions, no vote involved
    for tag in ("cm_b", "cm_i"):
        assert torch.equal(new[tag].value, old[tag].value), tag
    assert int(new["cm_b"].value.sum()) > 0 and int((new["cm_b"].value.sum() + new["cm_i"].value.sum())) == int((label_dev[rp["parts"].long()] != ignore).sum())
    assert len(torch.unique(new["pred"])) > 1
    # the `test` split: predictions and no matrices; two runs give the same bits
    bare = evaluate.test_room_scannet(model, coord, feat, None, ref.VOXEL, ncls, ignore, nsample, batch=batch, perm=perm)
    assert bare["cm"] is None and bare["cm_b"] is None and bare["cm_i"] is None
    assert torch.equal(bare["pred"], new["pred"]) and torch.equal(bare["logits"].view(torch.int32), new["logits"].view(torch.int32))
    with pytest.raises(ValueError):
        evaluate.test_room_scannet(model, coord, feat, label, ref.VOXEL, ncls, ignore, nsample, variable=True)
