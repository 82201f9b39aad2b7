"""S3DISSphere on the device (csrc/sphere.hip, input_pipeline.SpherePotentials / s3dis_sphere_batch / S3DISSphereFeed /
sphere_projections, evaluate.validate_sphere) against the plain-numpy restatement tests/sphere_ref.py, which
tests/test_sphere_oracle.py ties to the reference's own S3DISSphere.  Every comparison is exact: integer tables with
assert_array_equal, float32 outputs bit for bit, the float64 potentials through their int64 patterns.

  (a) the recorded schedule (24 steps over two clouds) and the recorded items as two batches of B = 4 at num_points = 1024
  (b) constructed edges: cur == num_points, cur == 1, cur == 0 (a noise larger than in_radius), exact duplicate points with
      equal potentials (the ascending-index rule for equal distances and the first of a tied minimum), and a cloud 100 m from
      the origin, where float32 distances order the sphere differently (asserted on the case itself)
  (c) generator draws: masks, counts, the query's set, the pads; nothing is read back (torch's sync debug mode, where honoured);
      a transform (S3DISTrainAugment, a TransformChain without and with a `heights` writer) on the centred spheres
  (d) one epoch of S3DISSphereFeed is the s3dis_sphere_batch sequence; one train_one_epoch with MaskedCrossEntropy on the feed
  (e) validate_sphere with a fixed 1x1-conv stand-in: voted logits, predictions, confusion matrix; two runs, the same bits
  (f) sphere_projections: the chosen sub-point's float32 d2 is the row minimum"""
import numpy as np
import pytest
import torch

import sphere_ref as sr
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == "f":
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)
    else:
        np.testing.assert_array_equal(got, want, err_msg=what)


@pytest.fixture(scope="module")
def fx():
    g = load_golden("s3dis_sphere")
    g["clouds"] = [{k: g[f"cloud{c}/{k}"] for k in ("sub_points", "sub_colors", "sub_labels", "points", "labels", "potentials",
                                                     "projections")} for c in range(2)]
    m = g["meta"]
    pots = [c["potentials"].copy() for c in g["clouds"]]
    g["want_schedule"] = sr.schedule(pots, [c["sub_points"] for c in g["clouds"]], g["noise"], m["in_radius"], m["num_points"])
    g["want_potentials"] = pots
    return g


def _device_clouds(clouds):
    return [(_t(c["sub_points"]), _t(c["sub_colors"]), _t(c["sub_labels"])) for c in clouds]


def _state(fx, **kw):
    from amcontrast3d_amd import input_pipeline as ip
    m = fx["meta"]
    return ip.SpherePotentials(_device_clouds(fx["clouds"]), m["in_radius"], m["num_points"],
                               potentials=[c["potentials"] for c in fx["clouds"]], **kw)


# ---- (a) the fixture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", [(24,), (5, 1, 18)])
def test_the_recorded_schedule_and_the_potentials_bit_for_bit(fx, chunks):
    st = _state(fx)
    cloud, point, lo = [], [], 0
    for n in chunks:
        c, p, nz = st.advance(n, noise=fx["noise"][lo:lo + n])
        assert c.dtype == p.dtype == torch.int64 and nz.dtype == torch.float64
        cloud.append(c.cpu().numpy()); point.append(p.cpu().numpy()); lo += n
    _same(np.concatenate(cloud), fx["cloud_inds"], "cloud_inds")
    _same(np.concatenate(point), fx["point_inds"], "point_inds")
    for c, (got, want) in enumerate(zip(st.cloud_potentials(), fx["want_potentials"])):
        _same(got, want, f"potentials of cloud {c}")
        assert not np.array_equal(want, fx["clouds"][c]["potentials"]), "the schedule updated this cloud"


def _check_items(fx, out, first):
    for b in range(4):
        for k in ("pos", "x", "y", "mask", "input_inds", "heights", "cloud_index"):
            _same(out[k][b], fx[f"item{first + b}/{k}"], f"item {first + b}: {k}")


@pytest.mark.parametrize("first", [0, 4])
def test_the_recorded_items_as_batches_of_four(fx, first):
    from amcontrast3d_amd import input_pipeline as ip
    st = _state(fx)
    sel = slice(first, first + 4)
    draws = {"perm": [fx[f"item{i}/perm"] for i in range(first, first + 4)], "pad": [fx[f"item{i}/pad"] for i in range(first, first + 4)]}
    before = st.potentials.clone()
    out = ip.s3dis_sphere_batch(st, (_t(fx["cloud_inds"][sel]), _t(fx["point_inds"][sel]), _t(fx["noise"][sel])), None, draws=draws)
    assert torch.equal(st.potentials, before), "a query of given centres leaves the potentials alone"
    assert out["pos"].shape == (4, 1024, 3) and out["heights"].shape == (4, 1024, 1) and out["mask"].dtype == torch.int32
    _check_items(fx, out, first)


def test_an_int_advances_the_schedule_and_gives_the_same_items(fx):
    from amcontrast3d_amd import input_pipeline as ip
    st = _state(fx)
    for first in (0, 4):
        draws = {"perm": [fx[f"item{i}/perm"] for i in range(first, first + 4)],
                 "pad": [fx[f"item{i}/pad"] for i in range(first, first + 4)], "centre_noise": fx["noise"][first:first + 4]}
        _check_items(fx, ip.s3dis_sphere_batch(st, 4, None, draws=draws), first)
    assert st.steps_done == 8
    c, p, _ = st.advance(16, noise=fx["noise"][8:])
    _same(c, fx["cloud_inds"][8:], "the schedule goes on where the batches left it")
    _same(p, fx["point_inds"][8:], "point_inds")


# ---- (b) constructed edges ------------------------------------------------------------------------------------------------------
def _edge_cases():
    rng = np.random.default_rng(5)
    cases = {}
    # 40 points within 0.05 of one another, 500 far away: the sphere of radius 0.3 around any of the 40 holds exactly them
    near = rng.uniform(0, 0.05, (40, 3)) + 3.0
    far = rng.uniform(10, 12, (500, 3))
    pts = np.concatenate([far[:200], near, far[200:]]).astype(np.float32)
    pot = rng.uniform(1, 2, len(pts)); pot[200:240] = rng.uniform(0, 1e-3, 40)
    cases["cur == num_points"] = dict(clouds=[pts], pots=[pot], noise=rng.normal(0, 0.003, (3, 3)), r=0.3, N=40, curs={40})
    # one isolated point holds the minimum; the next steps pick among the 40
    pts2 = np.concatenate([pts, np.array([[50.0, 50.0, 50.0]], np.float32)])
    pot2 = np.concatenate([pot, [0.0]])
    cases["cur == 1"] = dict(clouds=[pts2], pots=[pot2], noise=rng.normal(0, 0.003, (3, 3)), r=0.3, N=64, curs={1, 40})
    nz = rng.normal(0, 0.003, (3, 3)); nz[0] = [0.0, 0.45, 0.0]
    cases["cur == 0"] = dict(clouds=[pts2], pots=[pot2], noise=nz, r=0.3, N=64, curs={0, 1})
    # every point twice, in two clouds, with equal potentials everywhere: ties in the distances and in both arg-mins
    base = rng.uniform(0, 1, (700, 3)).astype(np.float32)
    dup = np.concatenate([base, base[::-1]])
    cases["duplicates"] = dict(clouds=[dup, dup[:900].copy()], pots=[np.full(1400, 0.5), np.full(900, 0.5)],
                               noise=rng.normal(0, 0.03, (4, 3)), r=0.3, N=128, curs=None)
    shifted = (rng.uniform(0, 0.6, (4000, 3)) + 100.0).astype(np.float32)
    cases["100 m from the origin"] = dict(clouds=[shifted, (rng.uniform(0, 0.6, (1500, 3)) + 100.0).astype(np.float32)],
                                          pots=[rng.uniform(0, 1e-3, 4000), rng.uniform(0, 1e-3, 1500)],
                                          noise=rng.normal(0, 0.045, (4, 3)), r=0.45, N=1200, curs=None)
    return cases


EDGES = _edge_cases()


@pytest.mark.parametrize("name", list(EDGES))
def test_constructed_edges(name):
    from amcontrast3d_amd import input_pipeline as ip
    case = EDGES[name]
    N, r, steps = case["N"], case["r"], len(case["noise"])
    rng = np.random.default_rng(17)
    colours = [rng.integers(0, 256, c.shape).astype(np.float32) for c in case["clouds"]]
    labels = [rng.integers(0, 13, len(c)).astype(np.int64) for c in case["clouds"]]
    st = ip.SpherePotentials([(_t(p), _t(c), _t(l)) for p, c, l in zip(case["clouds"], colours, labels)], r, N, potentials=case["pots"])
    cloud, point, noise, q = st.advance(steps, noise=case["noise"], lists=True)
    pots = [p.astype(np.float64).copy() for p in case["pots"]]
    want, curs = [], []
    for s in range(steps):
        before = [p.copy() for p in pots]
        c, p, ql, cur = sr.schedule_step(pots, case["clouds"], case["noise"][s], r, N)
        want.append((c, p, ql, cur)); curs.append(cur)
        if cur == 0:
            assert all(np.array_equal(a, b) for a, b in zip(before, pots)), "an empty sphere updates nothing"
    if case["curs"] is not None:
        assert case["curs"] <= set(curs), curs
    _same(cloud, np.array([w[0] for w in want]), "cloud_inds")
    _same(point, np.array([w[1] for w in want]), "point_inds")
    _same(q["cur"], np.array(curs, dtype=np.int32), "cur")
    _same(q["count"], np.minimum(curs, N).astype(np.int32), "count")
    order = q["order"].cpu().numpy()
    for s, (_, _, ql, cur) in enumerate(want):
        np.testing.assert_array_equal(order[s, :len(ql)], ql, err_msg=f"step {s}: the list")
        assert (order[s, len(ql):] == -1).all()
    for c, (got, w) in enumerate(zip(st.cloud_potentials(), pots)):
        _same(got, w, f"potentials of cloud {c}")
    if name == "duplicates":
        assert any(len(np.unique(sr.radius_query(case["clouds"][w[0]], sr.pick_point(case["clouds"][w[0]], w[1], case["noise"][s]), r)[1]
                                 [w[2]])) < len(w[2]) for s, w in enumerate(want)), "equal distances inside a sphere"
        assert want[0][:2] == (0, 0), "the first of a tied minimum, in the first of two tied clouds"
    if name == "100 m from the origin":
        differs = []
        for s, (c, p, ql, cur) in enumerate(want):
            pts = case["clouds"][c]
            d = pts - (pts[p] + case["noise"][s].astype(np.float32)).astype(np.float32)
            d32 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            inside = np.flatnonzero(d32 <= np.float32(r * r))
            differs.append(not np.array_equal(inside[np.argsort(d32[inside], kind="stable")][:N], ql))
        assert all(differs), "float32 distances list every one of these spheres differently"
    # the items of the same centres, with numpy's draws
    perms = [rng.permutation(min(cur, N)) for cur in curs]
    pads = [rng.integers(0, cur, max(N - cur, 0)) if cur else None for cur in curs]  # (an empty sphere takes no draws)
    out = ip.s3dis_sphere_batch(st, (cloud, point, noise), None, draws={"perm": perms, "pad": pads})
    for s, (c, p, _, cur) in enumerate(want):
        w = sr.item(case["clouds"][c], colours[c], labels[c], c, p, case["noise"][s], r, N, perms[s], pads[s])
        assert w["cur"] == cur
        for k in ("pos", "x", "y", "mask", "input_inds", "heights", "cloud_index"):
            _same(out[k][s], w[k], f"{name}, item {s}: {k}")
        if cur == 0:
            assert not w["mask"].any() and (w["input_inds"] == p).all()


# ---- (c) generator draws ---------------------------------------------------------------------------------------------------------
def _sync_mode_is_honoured():
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


def test_generator_draws_and_no_read_back(fx):
    from amcontrast3d_amd import input_pipeline as ip
    m = fx["meta"]
    N, r = m["num_points"], m["in_radius"]
    g = torch.Generator(device=DEV).manual_seed(7)
    st = _state(fx, generator=g)
    ip.s3dis_sphere_batch(st, 2, None)  # (first use: the library is loaded, the allocator is warm)
    honoured = _sync_mode_is_honoured()
    if honoured:
        torch.cuda.set_sync_debug_mode("error")
    try:
        cloud, point, noise = st.advance(4)
        out = ip.s3dis_sphere_batch(st, (cloud, point, noise), None)
        out2 = ip.s3dis_sphere_batch(st, 4, None)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("torch.cuda.set_sync_debug_mode honoured:", honoured)
    assert out2["pos"].shape == (4, N, 3) and st.steps_done == 10
    cloud, point, noise = cloud.cpu().numpy(), point.cpu().numpy(), noise.cpu().numpy()
    assert np.abs(noise).max() < r and noise.std() > 0
    inds, mask = out["input_inds"].cpu().numpy(), out["mask"].cpu().numpy()
    counts = []
    for b in range(4):
        pts = fx["clouds"][cloud[b]]["sub_points"]
        centre = sr.pick_point(pts, point[b], noise[b])
        q, _ = sr.radius_query(pts, centre, r)
        cnt = min(len(q), N)
        counts.append(cnt)
        np.testing.assert_array_equal(mask[b], (np.arange(N) < cnt).astype(np.int32))
        np.testing.assert_array_equal(np.sort(inds[b, :cnt]), np.sort(q[:N]))
        assert not np.array_equal(inds[b, :cnt], q[:N]), "shuffled"
        assert np.isin(inds[b, cnt:], inds[b, :cnt]).all(), "the pads repeat listed points"
        if cnt < N:
            assert len(np.unique(inds[b, cnt:])) > 1
        _same(out["pos"][b], (pts[inds[b]].astype(np.float64) - centre).astype(np.float32), "pos")
        _same(out["heights"][b], pts[inds[b]][:, 2:3], "heights")
        _same(out["y"][b], fx["clouds"][cloud[b]]["sub_labels"][inds[b]], "y")
    assert len(counts) == 4


@pytest.mark.parametrize("kind", ["augment", "chain", "chain with heights"])
def test_a_transform_is_applied_to_the_centred_spheres(fx, kind):
    """the batch with a transform is that transform on the untransformed batch's pos / x from the same draws, bit for bit;
    heights stays the absolute gravity coordinate unless the list holds the one reference transform that writes `heights`"""
    from amcontrast3d_amd import input_pipeline as ip
    from amcontrast3d_amd.augment import S3DISTrainAugment
    from amcontrast3d_amd.transforms import TransformChain
    kw = {"color_drop": 0.2, "gravity_dim": 2, "scale": [0.9, 1.1], "angle": [0, 0, 1], "jitter_sigma": 0.005, "jitter_clip": 0.02}
    names = ["ChromaticAutoContrast", "PointsToTensor", "PointCloudScaling", "PointCloudXYZAlign", "PointCloudRotation",
             "PointCloudJitter", "ChromaticDropGPU", "ChromaticNormalize"]  # cfgs/s3dis/default.yaml
    if kind == "augment":
        t = S3DISTrainAugment(**kw)
    else:
        t = TransformChain(names[:2] + (["PointCloudCenterAndNormalize"] if kind == "chain with heights" else []) + names[2:], kw)
    st = _state(fx)
    B, N = 4, fx["meta"]["num_points"]
    sel = slice(4, 8)
    centres = (_t(fx["cloud_inds"][sel]), _t(fx["point_inds"][sel]), _t(fx["noise"][sel]))
    own = {"perm": [fx[f"item{i}/perm"] for i in range(4, 8)], "pad": [fx[f"item{i}/pad"] for i in range(4, 8)]}
    plain = ip.s3dis_sphere_batch(st, centres, None, draws=own)
    g = torch.Generator(device=DEV).manual_seed(9)
    d = t.draw(B, N, torch.device(DEV), g) if kind == "augment" else t.draw([N] * B, torch.device(DEV), g)
    got = ip.s3dis_sphere_batch(st, centres, t, draws=dict(own, **d))
    if kind == "augment":
        pos, x, _ = t(plain["pos"], plain["x"], draws=d)
        heights = plain["heights"]
    else:
        out = t({"pos": plain["pos"], "x": plain["x"]}, draws=d)
        pos, x, heights = out["pos"], out["x"], out["heights"] if kind == "chain with heights" else plain["heights"]
    assert torch.equal(got["pos"], pos) and torch.equal(got["x"], x) and torch.equal(got["heights"], heights)
    assert not torch.equal(got["pos"], plain["pos"]) and not torch.equal(got["x"], plain["x"])
    assert torch.equal(got["heights"], plain["heights"]) == (kind != "chain with heights")
    for k in ("y", "mask", "cloud_index", "input_inds"):
        assert torch.equal(got[k], plain[k]), k


# ---- (d) the feed -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffle", [False, True])
def test_one_epoch_of_the_feed_is_the_batch_sequence(fx, shuffle):
    from amcontrast3d_amd import input_pipeline as ip
    m = fx["meta"]
    B, steps = 4, 10
    g1, g2 = torch.Generator(device=DEV).manual_seed(3), torch.Generator(device=DEV).manual_seed(3)
    feed = ip.S3DISSphereFeed(_device_clouds(fx["clouds"]), None, B, m["in_radius"], m["num_points"], steps, shuffle=shuffle,
                              potentials=[c["potentials"] for c in fx["clouds"]], generator=g1)
    assert len(feed) == 2
    got = list(feed)
    st = _state(fx, generator=g2)
    want = []
    if shuffle:
        cloud, point, noise = st.advance(steps)
        ids = torch.randperm(steps, device=DEV, generator=g2)
        for i in range(2):
            pick = ids[i * B:(i + 1) * B]
            want.append(ip.s3dis_sphere_batch(st, (cloud[pick], point[pick], noise[pick]), None))
    else:
        want = [ip.s3dis_sphere_batch(st, B, None) for _ in range(2)]
        st.advance(steps - 2 * B)
    assert len(got) == 2
    for a, b in zip(got, want):
        assert set(a) == {"pos", "x", "heights", "y", "mask", "cloud_index", "input_inds"}
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(feed.state.potentials, st.potentials) and feed.state.steps_done == steps
    assert not torch.equal(got[0]["pos"], got[1]["pos"])


@pytest.fixture
def _fresh_pipelines():
    from amcontrast3d_amd import train
    train.release_pipelines()
    yield
    train.release_pipelines()


def test_train_one_epoch_with_the_masked_criterion_on_the_feed(fx, _fresh_pipelines):
    """the tiny baseline model of tests/test_gpu_loss_family.py at (2, 1024), lr = 0: the captured pipeline and the eager loop see
    the same batches (two feeds from one seed) and return the same averages"""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import input_pipeline as ip, train
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.optim import build_optimizer_from_cfg
    from openpoints.utils import EasyConfig
    from test_baseline_host import build, pointnext_xl
    from test_gpu_train_edges import _Probe, _same_results
    m = fx["meta"]
    results = []
    for graph_pipeline in (True, False):
        cfg = pointnext_xl("s3dis", width=8, blocks=(1, 1, 1, 1, 1))
        cfg["cls_args"]["dropout"] = 0
        torch.manual_seed(0)
        model = build(cfg).to(DEV)
        cc = EasyConfig(); cc.update({"NAME": "MaskedCrossEntropy"})
        crit = build_criterion_from_cfg(cc).to(DEV)
        c = EasyConfig()
        c.update({"num_classes": 13, "ignore_index": None, "feature_keys": "x,heights", "use_amp": False, "step_per_update": 1,
                  "grad_norm_clip": 10, "sched_on_epoch": False, "fps_lanes": 2, "criterion_args": {"NAME": "MaskedCrossEntropy"},
                  "graph_pipeline": graph_pipeline})
        opt = build_optimizer_from_cfg(model, NAME="adamw", lr=0.0, weight_decay=1e-4)
        feed = ip.S3DISSphereFeed(_device_clouds(fx["clouds"]), None, 2, m["in_radius"], m["num_points"], 4,
                                  potentials=[cl["potentials"] for cl in fx["clouds"]],
                                  generator=torch.Generator(device=DEV).manual_seed(11))
        results.append(train.train_one_epoch(model, feed, crit, opt, _Probe(), None, 1, c))
        torch.cuda.synchronize()
        assert feed.state.steps_done == 4
    assert len(train._PIPELINES) == 1
    pipe = next(iter(train._PIPELINES.values()))[0]
    assert "mask" in pipe.keys and "input_inds" in pipe.keys
    assert np.isfinite(results[0][0])
    _same_results(results[0], results[1])


# ---- (e) validate_sphere --------------------------------------------------------------------------------------------------------
class _StandIn(torch.nn.Module):
    """a fixed 1x1 convolution over the model's 'x' (B,4,N) -> logits (B,C,N), written element-wise: the same bits on every run"""

    def __init__(self, classes):
        super().__init__()
        g = torch.Generator().manual_seed(2)
        self.w = torch.nn.Parameter(torch.randn(classes, 4, generator=g) * torch.tensor([0.01, 0.01, 0.01, 1.0]))
        self.b = torch.nn.Parameter(torch.randn(classes, generator=g))

    def forward(self, data):
        x = data["x"]
        out = self.b.view(1, -1, 1).expand(x.shape[0], -1, x.shape[2]).clone()
        for k in range(4):
            out = out + self.w[:, k].view(1, -1, 1) * x[:, k:k + 1, :]
        return out


def test_validate_sphere_votes_in_position_order(fx):
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import evaluate, input_pipeline as ip
    m = fx["meta"]
    cl = fx["clouds"][0]
    n_sub, C = len(cl["sub_points"]), 13
    st = ip.SpherePotentials(_device_clouds([cl]), m["in_radius"], m["num_points"], potentials=[cl["potentials"]],
                             generator=torch.Generator(device=DEV).manual_seed(5))
    batches = [ip.s3dis_sphere_batch(st, 4, None) for _ in range(2)]
    model = _StandIn(C).to(DEV)
    proj, labels = cl["projections"].astype(np.int64), cl["labels"].reshape(-1).astype(np.int64)
    runs = [evaluate.validate_sphere(model, batches, n_sub, _t(proj), _t(labels), C, None, "x,heights", details=True) for _ in range(2)]
    for k in ("logits", "pred"):
        assert torch.equal(runs[0][k], runs[1][k]), f"{k}: two runs, the same bits"
    assert torch.equal(runs[0]["cm"].value, runs[1]["cm"].value)
    with torch.no_grad():
        flat = torch.cat([model({"x": torch.cat([b["x"], b["heights"]], -1).transpose(1, 2).contiguous()}).transpose(1, 2).reshape(-1, C)
                          for b in batches]).cpu().numpy()
    inds = torch.cat([b["input_inds"].reshape(-1) for b in batches]).cpu().numpy()
    voted, pred, _, cm = sr.vote(flat, inds, n_sub, proj, labels, C)
    visits = np.bincount(inds, minlength=n_sub)
    assert (visits == 0).any() and (visits > 1).any(), "unvisited sub-points and overlapping spheres are both in the case"
    _same(runs[0]["logits"], voted, "voted logits")
    _same(runs[0]["pred"], pred.astype(np.int64), "predictions")
    _same(runs[0]["cm"].value, cm.astype(np.int64), "confusion matrix")
    assert not runs[0]["logits"][torch.as_tensor(visits == 0).to(DEV)].any(), "zero logits where no sphere came"
    metrics = evaluate.validate_sphere(model, batches, n_sub, _t(proj), _t(labels), C, None, "x,heights")
    assert len(metrics) == 5 and 0.0 <= float(metrics[2]) <= 100.0


# ---- (f) the projections ---------------------------------------------------------------------------------------------------------
def test_sphere_projections_reach_the_row_minimum(fx):
    from amcontrast3d_amd import input_pipeline as ip
    cl = fx["clouds"][0]
    raw, sub = cl["points"][:3001], cl["sub_points"]
    got = ip.sphere_projections(_t(raw), _t(sub))
    assert got.dtype == torch.int64 and got.shape == (3001,)
    got = got.cpu().numpy()
    assert got.min() >= 0 and got.max() < len(sub)
    for lo in range(0, len(raw), 500):
        d2 = sr.projections(raw[lo:lo + 500], sub)
        rows = np.arange(d2.shape[0])
        np.testing.assert_array_equal(_bits(d2[rows, got[lo:lo + 500]]), _bits(d2.min(1)))
