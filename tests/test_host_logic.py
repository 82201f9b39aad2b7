"""Host-side contract of the drop-in (no GPU needed): registries, config objects, module / state-dict
naming identical to the reference (key lists recorded from the reference's own classes in
tests/golden/state_keys.json), and the C-ABI library exporting every symbol include/amc3d.h declares."""
import ctypes
import json
import os
import re

import pytest
import torch

import amcontrast3d_amd
from amcontrast3d_amd import configs
from conftest import GOLDEN, ROOT

amcontrast3d_amd.activate()

from openpoints.loss import LOSS, build_criterion_from_cfg  # noqa: E402
from openpoints.models import MODELS, build_model_from_cfg  # noqa: E402
from openpoints.utils import EasyConfig, registry  # noqa: E402


def easy(d):
    c = EasyConfig()
    c.update(d)
    return c


def test_openpoints_resolves_to_this_build():
    import openpoints
    assert openpoints.__file__.startswith(os.path.join(ROOT, "amcontrast3d_amd"))


def test_registry_contract():
    assert {"BaseSeg_AMContrast3D", "PointNextEncoder_AMContrast3D", "PointNextDecoder_AMContrast3D", "SegHead"} <= set(MODELS.module_dict)
    assert {"CrossEntropyAce", "CrossEntropy", "CrossEntropyLoss", "BCEWithLogitsLoss"} <= set(LOSS.module_dict)
    R = registry.Registry("things")

    @R.register_module()
    class A:
        def __init__(self, x, y=2):
            self.x, self.y = x, y

    R.register_module(name="alias", module=A)
    assert R.get("A") is A and R.get("alias") is A and "A" in R and len(R) == 2
    with pytest.raises(KeyError, match="already registered"):
        R.register_module(module=A)
    cfg = {"NAME": "A", "x": 1}
    obj = R.build(cfg)
    assert (obj.x, obj.y) == (1, 2) and cfg == {"NAME": "A", "x": 1}  # cfg is deep-copied, not consumed
    with pytest.raises(KeyError, match="not in the things registry"):
        R.build({"NAME": "B"})
    with pytest.raises(KeyError, match='must contain the key "NAME"'):
        R.build({"x": 1})
    with pytest.raises(TypeError, match="cfg must be a dict"):
        R.build([1])
    with pytest.raises(TypeError, match="^A: "):  # ctor errors carry the class name (registry.py:292-294)
        R.build({"NAME": "A"})


def test_easyconfig_behaviour(tmp_path):
    c = easy({"a": {"b": 1, "c": {"d": 2}}, "e": [1, 2]})
    assert c.a.c.d == 2 and isinstance(c.a, EasyConfig)
    c.update(["a.b=5", "--a.c.d", "7", "new.key=[1,2]", "s=hello"])
    assert c.a.b == 5 and c.a.c.d == 7 and c.new.key == [1, 2] and c.s == "hello"
    with pytest.raises(AttributeError):
        c.missing
    # recursive default.yaml layering (utils/config.py:30-49)
    (tmp_path / "default.yaml").write_text("x: 1\ny: {z: 1}\n")
    sub = tmp_path / "ds"
    sub.mkdir()
    (sub / "default.yaml").write_text("y: {z: 2, w: 3}\n")
    (sub / "m.yaml").write_text("x: 9\n")
    d = EasyConfig()
    d.load(str(sub / "m.yaml"), recursive=True)
    assert d.x == 9 and d.y.z == 2 and d.y.w == 3
    assert d.dict() == {"x": 9, "y": {"z": 2, "w": 3}} and len(d.hash()) == 64


@pytest.mark.parametrize("variant", ["S", "B", "L", "XL"])
def test_state_dict_keys_match_reference(variant):
    keys = json.load(open(os.path.join(GOLDEN, "state_keys.json")))
    model = build_model_from_cfg(easy(configs.model_cfg(variant)))
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == keys[variant]
    assert sum(p.numel() for p in model.parameters()) == keys[variant + "_nparams"]


def test_scannet_head_and_bn_module_types():
    keys = json.load(open(os.path.join(GOLDEN, "state_keys.json")))
    model = build_model_from_cfg(easy(configs.model_cfg("S", num_classes=20, in_channels=7, global_feat="max")))
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == keys["S_scannet"]
    # BN layers must stay real torch modules so SyncBatchNorm conversion / DDP see them (main_AA.py:146-151)
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    assert len(bns) == 17
    conv = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
    assert sum(isinstance(m, torch.nn.SyncBatchNorm) for m in conv.modules()) == 17


def test_builder_side_effects_on_cfg():
    """Built through the registry the constructors work on a deep copy (registry.py:287), so the caller's
    cfg is untouched; built directly they write into the caller's objects like the reference does."""
    cfg = easy(configs.model_cfg("S"))
    model = build_model_from_cfg(cfg)
    assert cfg.cls_args.in_channels is None and model.decoder.out_channels == 32
    assert "radius" not in cfg.encoder_args.group_args
    assert model.encoder.channel_list == [32, 64, 128, 256, 512] and model.encoder.out_channels == 512
    assert model.encoder.radii == [[0.1], [0.1], [0.2], [0.4], [0.8]]
    assert [s[0].grouper.radius for s in list(model.encoder.encoder)[1:]] == [0.1, 0.2, 0.4, 0.8]
    enc = easy(configs.model_cfg("S")["encoder_args"])
    from openpoints.models.backbone import PointNextEncoder_AMContrast3D
    ga = enc.group_args
    kw = dict(enc); kw.pop("NAME")
    PointNextEncoder_AMContrast3D(**kw)
    assert ga.radius == 0.8 and ga.nsample == 32  # pointnext_AA.py:362-363, 405-406 leave the last stage's values


def test_criterion_ctor_swallows_kwargs():
    crit = build_criterion_from_cfg(easy({"NAME": "CrossEntropyAce", "label_smoothing": 0.2, "weight": None, "ignore_index": -100}))
    assert isinstance(crit.creterion, torch.nn.CrossEntropyLoss) and crit.creterion.label_smoothing == 0.0
    assert type(crit.contrast_head).__name__ == "ContrastHead"
    assert crit.contrast_head.nstride.tolist() == [4, 4, 4, 4]


def test_product_ops_have_no_cpu_path():
    from amcontrast3d_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ball_query(0.1, 4, torch.rand(1, 8, 3), torch.rand(1, 2, 3))
    model = build_model_from_cfg(easy(configs.model_cfg("S")))
    with pytest.raises(RuntimeError, match="GPU only"):
        model({"pos": torch.rand(1, 64, 3), "x": torch.rand(1, 4, 64)})


def test_c_abi_exports_every_declared_symbol():
    from amcontrast3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "amc3d.h")).read()
    declared = set(re.findall(r"\b(amc3d_\w+)\s*\(", header))
    assert declared and declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    so = _lib.build()
    lib = ctypes.CDLL(so)
    for name in declared:
        assert hasattr(lib, name), name
    lib.amc3d_version.restype = ctypes.c_char_p
    assert lib.amc3d_version() == b"amc3d-hip gfx950 1"
    # no torch / libc10 dependency in the boundary library
    import subprocess
    deps = subprocess.run(["ldd", so], capture_output=True, text=True).stdout
    names = [line.split()[0] for line in deps.splitlines() if line.split()]  # library names only: a load address may
    assert not any("torch" in n or "c10" in n for n in names), names               # well contain the digits "c10"


def test_c_abi_argtypes_match_the_header():
    """A miscounted `[_vp] * n` row of _lib.SIGNATURES loads without complaint and corrupts an argument at the call: every
    row must have the header's parameter count, a pointer type where the prototype has a `*` and the matching scalar elsewhere."""
    from amcontrast3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "amc3d.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    header = re.sub(r"//[^\n]*", " ", header)
    protos = dict(re.findall(r"\b(amc3d_\w+)\s*\(([^()]*)\)\s*;", header))
    assert set(protos) == set(_lib.SIGNATURES), set(protos) ^ set(_lib.SIGNATURES)
    scalars = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long": ctypes.c_long,
               "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong}

    def is_pointer(t):
        return t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer)

    for name, params in sorted(protos.items()):
        params = [] if params.strip() in ("", "void") else [" ".join(p.split()) for p in params.split(",")]
        argtypes = _lib.SIGNATURES[name][1]
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (p, t) in enumerate(zip(params, argtypes)):
            if "*" in p:
                assert is_pointer(t), (name, k, p, t)
            else:
                ctype = " ".join(w for w in p.split()[:-1] if w != "const")  # the declaration without its parameter name
                assert t is scalars[ctype], (name, k, p, t)


def test_compat_modules_have_the_reference_entry_points():
    from amcontrast3d_amd import compat
    names = ["ball_query_wrapper", "group_points_wrapper", "group_points_grad_wrapper", "gather_points_wrapper",
             "gather_points_grad_wrapper", "furthest_point_sampling_wrapper", "three_nn_wrapper",
             "three_interpolate_wrapper", "three_interpolate_grad_wrapper"]  # pointnet2_api.cpp:10-24
    for n in names:
        assert callable(getattr(compat.pointnet2_batch_cuda, n))
    assert callable(compat.pointops_cuda.knnquery_cuda)  # pointops_api.cpp:14


def test_synthetic_scenes_are_reproducible_and_shaped():
    from amcontrast3d_amd import synthetic
    a = synthetic.make_batch(2, 1500, first_id=3)
    b = synthetic.make_batch(2, 1500, first_id=3)
    for k in a:
        assert (a[k] == b[k]).all()
    assert a["pos"].shape == (2, 1500, 3) and a["x"].shape == (2, 4, 1500) and a["y"].shape == (2, 1500)
    assert a["pos"].dtype == "float32" and a["y"].dtype == "int64" and a["pos"].min() == 0
    assert (a["x"][:, 3] == a["pos"][..., 2]).all()  # heights channel
    d = synthetic.make_scene(5, 4000, duplicates=True)
    import numpy as np
    assert len(np.unique(d["pos"], axis=0)) < 4000  # padded by repetition like data_util.py:161-167


def test_mm_registry_and_state_keys():
    """AMContrast3D++ classes are registered under the reference's names and the model's state-dict keys are the
    reference's (recorded in the golden fixture's meta by oracle/gen_golden.py)."""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import configs
    from conftest import load_golden
    from openpoints.loss import LOSS
    from openpoints.models import MODELS, build_model_from_cfg
    from openpoints.utils import EasyConfig
    for name in ("BaseSeg_M_AMContrast3D", "PointNextEncoder_M_AMContrast3D", "PointNextDecoder_M_AMContrast3D",
                 "APM_pf_ConCate"):
        assert MODELS.get(name) is not None, name
    assert LOSS.get("CrossEntropyAcePre") is not None
    m = load_golden("model_mm_w8_b2_n2048")["meta"]
    c = EasyConfig()
    c.update(configs.model_cfg_mm(m["variant"], dropout=0, **m["model_kw"]))
    model = build_model_from_cfg(c)
    assert list(model.state_dict().keys()) == m["state_keys"]
    xl = EasyConfig()
    xl.update(configs.model_cfg_mm("XL"))  # cfgs/s3dis/AMContrast3D-MM.yaml shape
    apm = build_model_from_cfg(xl.APM_args)
    assert [apm.layer_0[0].in_features, apm.layer_3[0].in_features] == [3 + 64, 3 + 512]


def test_trainer_import_surface_of_the_metrics_modules():
    """examples/segmentation/main_AA.py:16,31 / main_MM.py:16,27 import these names; this package's modules shadow the
    reference's under the path overlay, so they must all exist"""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.AMContrast3D.metrics import ambiguity_metrics, ambiguity_summary, posmask_searching, vis_tsne  # noqa: F401
    from openpoints.utils import AverageMeter, ConfusionMatrix, get_mious  # noqa: F401
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        out = ambiguity_summary(2, [{}], [[10, 20, 30, 20, 20], [20, 20, 20, 20, 20]], [[1.0] * 5] * 2,
                                [{0: [1, 2, 3, 4, 5]}, {0: [3, 2, 3, 4, 5]}], [[1, 2, 3, 4, 5]] * 2, [[1, 2, 3, 4, 5]] * 2,
                                [[1, 2, 3, 4, 5]] * 2, [[[1, 2]] * 5] * 2)
    assert list(out["count"]) == [15, 20, 25, 20, 20] and list(out["cls"][0]) == [2, 2, 3, 4, 5] and out["cls"][1] is None


# ---- trainer-side helpers under the reference's names ---------------------------------------
def _tiny_model():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import configs
    from openpoints.models import build_model_from_cfg
    from openpoints.utils import EasyConfig
    import torch
    torch.manual_seed(0)
    c = EasyConfig()
    c.update(configs.model_cfg("S", dropout=0, width=8))
    return build_model_from_cfg(c)


def test_param_groups_and_optimizer_factory():
    """optim_factory.py:66-120: 1-d parameters and biases -> weight decay 0, everything else decays; AdamW as the configs ask"""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.optim import build_optimizer_from_cfg, get_parameter_groups
    model = _tiny_model()
    groups = get_parameter_groups(model, weight_decay=1e-4)
    assert [g["weight_decay"] for g in groups] in ([1e-4, 0.0], [0.0, 1e-4]) and all(g["lr_scale"] == 1.0 for g in groups)
    by_id = {id(p): g["weight_decay"] for g in groups for p in g["params"]}
    for name, p in model.named_parameters():
        assert by_id[id(p)] == (0.0 if (p.ndim == 1 or name.endswith(".bias")) else 1e-4), name
    opt = build_optimizer_from_cfg(model, NAME="adamw", lr=0.01, weight_decay=1e-4)
    assert type(opt).__name__ == "AdamW" and sorted(g["weight_decay"] for g in opt.param_groups) == [0.0, 1e-4]
    assert sum(len(g["params"]) for g in opt.param_groups) == len(list(model.parameters()))
    import pytest
    with pytest.raises(NotImplementedError):
        build_optimizer_from_cfg(model, NAME="lamb", lr=0.01)


def test_checkpoint_round_trip(tmp_path):
    """utils/ckpt_util.py:61-183: save -> resume (model, optimizer, scheduler, epoch) -> load (non-strict) round trip, the
    reference's file layout and names, 'module.' prefixes handled both ways"""
    import torch
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.optim import build_optimizer_from_cfg
    from openpoints.scheduler import build_scheduler_from_cfg
    from openpoints.utils import EasyConfig, load_checkpoint, resume_checkpoint, resume_model, resume_optimizer, save_checkpoint
    cfg = EasyConfig()
    cfg.update({"ckpt_dir": str(tmp_path), "run_name": "run", "save_freq": 2, "epochs": 10, "lr": 0.01, "min_lr": 1e-5,
                "sched": "cosine"})
    model = _tiny_model()
    opt = build_optimizer_from_cfg(model, NAME="adamw", lr=0.01, weight_decay=1e-4)
    sched = build_scheduler_from_cfg(cfg, opt)
    for p in model.parameters():  # one optimizer step so that the state is not empty
        p.grad = torch.full_like(p, 0.01)
    opt.step()
    sched.step(3)
    lr3 = opt.param_groups[0]["lr"]
    assert abs(lr3 - (1e-5 + 0.5 * (0.01 - 1e-5) * (1 + __import__("math").cos(__import__("math").pi * 3 / 10)))) < 1e-12
    save_checkpoint(cfg, model, 4, opt, sched, additioanl_dict={"best_val": 0.5}, is_best=True)
    files = sorted(p.name for p in tmp_path.iterdir())
    assert files == ["run_E4.pth", "run_ckpt_best.pth", "run_ckpt_latest.pth"]
    raw = torch.load(tmp_path / "run_ckpt_latest.pth", weights_only=True)
    assert set(raw) == {"model", "optimizer", "scheduler", "epoch", "best_val"} and raw["epoch"] == 4
    want = {k: v.clone() for k, v in model.state_dict().items()}

    model2 = _tiny_model()
    with torch.no_grad():
        for p in model2.parameters():
            p.add_(1.0)
    opt2 = build_optimizer_from_cfg(model2, NAME="adamw", lr=0.01, weight_decay=1e-4)
    sched2 = build_scheduler_from_cfg(cfg, opt2)
    resume_checkpoint(cfg, model2, opt2, sched2, pretrained_path=str(tmp_path / "run_ckpt_latest.pth"))
    assert cfg.start_epoch == 5 and cfg.epoch == 5
    assert all(torch.equal(v, want[k]) for k, v in model2.state_dict().items())
    s1, s2 = opt.state_dict()["state"], opt2.state_dict()["state"]
    assert s1.keys() == s2.keys() and all(torch.equal(s1[k]["exp_avg"], s2[k]["exp_avg"]) for k in s1)
    sched2.step(3)
    assert opt2.param_groups[0]["lr"] == lr3

    wrapped = torch.nn.DataParallel(_tiny_model()) if False else None  # (no GPU here; the prefix logic is tested directly)
    model3 = _tiny_model()
    epoch, metrics = load_checkpoint(model3, str(tmp_path / "run_ckpt_best.pth"))
    assert epoch == 4 and metrics == {"best_val": 0.5}
    assert all(torch.equal(v, want[k]) for k, v in model3.state_dict().items())
    # a checkpoint saved from a wrapped model ('module.' keys) into a bare model and back
    torch.save({"model": {"module." + k: v for k, v in want.items()}, "epoch": 7}, tmp_path / "wrapped.pth")
    model4 = _tiny_model()
    resume_checkpoint(cfg, model4, pretrained_path=str(tmp_path / "wrapped.pth"))
    assert cfg.start_epoch == 8 and all(torch.equal(v, want[k]) for k, v in model4.state_dict().items())
    cfg2 = EasyConfig()
    cfg2.update({"ckpt_dir": str(tmp_path), "run_name": "absent"})
    assert resume_model(_tiny_model(), cfg2) == (0, 0) and resume_optimizer(cfg2, opt) == (0, 0, 0)
    assert resume_model(_tiny_model(), cfg, pretrained_path=str(tmp_path / "wrapped.pth")) == (8, None)


def _stand_in_reference(root):
    """A stand-in for a reference checkout under `root`, built from tests/golden/trainer_imports.json (names recorded from
    the reference): every module the overlay is to supply exists at the reference's path and defines the recorded names
    as placeholders; a package re-exports what the trainer imports from it.  Returns `root` as a string."""
    spec = json.load(open(os.path.join(GOLDEN, "trainer_imports.json")))
    files = {}  # path relative to root -> source lines

    def source(module, package=False):
        parts = module.split(".")
        for k in range(1, len(parts)):  # every enclosing package
            files.setdefault(os.path.join(*parts[:k], "__init__.py"), [])
        return files.setdefault(os.path.join(*parts, "__init__.py") if package else os.path.join(*parts) + ".py", [])

    for mod, names in spec["reference_defines"].items():
        source(mod).extend(f"def {n}(*args, **kwargs):\n    raise NotImplementedError('stand-in for the reference')\n"
                           for n in names)
    for mod, name in spec["trainer_imports"]:
        if mod == "openpoints.utils":  # this build's package: the overlay only adds modules to it
            continue
        owner = [d for d, names in spec["reference_defines"].items() if name in names and d.startswith(mod + ".")]
        if owner:
            source(mod, package=True).append(f"from {owner[0]} import {name}\n")
    for rel, lines in files.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("".join(lines))
    return str(root)


def test_reference_overlay_and_native_module_registration(tmp_path):
    """INTEGRATION.md mode B: with AMC3D_REFERENCE_ROOT the sub-packages this build does not provide resolve from the
    reference tree under the same `openpoints` name, and compat.register_native_modules() makes the reference's own
    wrappers import this library.  The reference tree is a stand-in with the reference's module layout
    (_stand_in_reference)."""
    import subprocess
    import sys
    ref = _stand_in_reference(tmp_path / "reference")
    code = (
        "import sys, types\n"
        "for m in ('easydict', 'multimethod', 'termcolor', 'shortuuid'):\n"
        "    sys.modules.setdefault(m, types.ModuleType(m))\n"
        "import amcontrast3d_amd; amcontrast3d_amd.activate()\n"
        "import openpoints, openpoints.utils\n"
        f"assert len(openpoints.__path__) == 2 and openpoints.__path__[1].startswith({ref!r})\n"
        "from openpoints.models import build_model_from_cfg\n"
        "import openpoints.models as om\n"
        "assert om.__file__.startswith(amcontrast3d_amd._HERE)  # the model side is this build's\n"
        "import importlib.util\n"
        f"assert importlib.util.find_spec('openpoints.transforms').origin.startswith({ref!r})\n"
        f"assert importlib.util.find_spec('openpoints.dataset').origin.startswith({ref!r})\n"
        "from openpoints.utils import save_checkpoint\n"
        "assert save_checkpoint.__module__ == 'openpoints.utils.ckpt_util' and "
        "sys.modules['openpoints.utils.ckpt_util'].__file__.startswith(amcontrast3d_amd._HERE)\n"
        "print('overlay ok')\n")
    env = dict(os.environ, AMC3D_REFERENCE_ROOT=ref)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0 and "overlay ok" in out.stdout, out.stderr[-2000:]
    # the native module names resolve to this library's compat views (no GPU needed to register / inspect them)
    from amcontrast3d_amd import compat
    compat.register_native_modules()
    import pointnet2_batch_cuda
    import pointops_cuda
    assert pointnet2_batch_cuda is compat.pointnet2_batch_cuda and hasattr(pointops_cuda, "knnquery_cuda")
    for name in ("ball_query_wrapper", "group_points_wrapper", "group_points_grad_wrapper", "gather_points_wrapper",
                 "gather_points_grad_wrapper", "furthest_point_sampling_wrapper", "three_nn_wrapper",
                 "three_interpolate_wrapper", "three_interpolate_grad_wrapper"):
        assert callable(getattr(pointnet2_batch_cuda, name))
    sys.modules.pop("pointnet2_batch_cuda"); sys.modules.pop("pointops_cuda")


@pytest.mark.parametrize("lanes", [2, 3, 4, 7, 12])
@pytest.mark.parametrize("nbatches", [1, 5, 24, 31])
def test_pipeline_hand_down_keeps_every_batch_with_its_own_geometry(lanes, nbatches):
    """pipeline.GraphPipeline's tick loop replayed with batch ids instead of tensors (amcontrast3d_amd/schedule.py holds its index
    arithmetic): every batch trains exactly once, in the order it entered, on ONE consistent set -- its points, its own FPS
    result and the neighbourhood / loss geometry computed from both -- a joint FPS launch has `lanes` ticks before its first
    lane is consumed, no lane is overwritten between its launch and its consumption, and a result set is never refilled
    before the feature variant that reads it has run."""
    from amcontrast3d_amd import schedule
    J = lanes
    src = iter(range(nbatches))
    joint_in = [[None] * J, [None] * J]     # batch id per lane
    joint_fps = [[None] * J, [None] * J]    # ("fps", id) once launched
    launched_at = [None, None]
    lane_valid = [[False] * J, [False] * J]
    sets = [None] * schedule.SETS
    set_valid = [False] * schedule.SETS
    read_pending = [False] * schedule.SETS  # set filled but not yet trained on
    last_read = [-10] * schedule.SETS       # tick at which a set was last trained on
    trained = []
    t, busy = 0, True
    while busy:
        plan = schedule.tick_plan(t, J)
        v0, v1 = plan["train"], plan["fill"]
        assert v0 != v1
        if set_valid[v0]:
            st = sets[v0]
            assert st["fps"] == ("fps", st["batch"]) and st["geo"] == ("geo", st["batch"], st["fps"])
            trained.append(st["batch"])
            read_pending[v0] = False
            last_read[v0] = t
        jc, l = plan["consume"]
        assert not read_pending[v1], "a result set is refilled before its feature variant ran"
        assert t - last_read[v1] >= 2, "a set is refilled less than two ticks after it was read (the host only checks tick t - 2)"
        if lane_valid[jc][l]:
            assert t - launched_at[jc] >= J, "a lane is consumed before its joint FPS launch can have finished"
            assert joint_fps[jc][l] == ("fps", joint_in[jc][l]), "a lane was overwritten between launch and consumption"
            sets[v1] = {"batch": joint_in[jc][l], "fps": joint_fps[jc][l]}
        set_valid[v1], lane_valid[jc][l] = lane_valid[jc][l], False
        if plan["launch"] is not None:
            jl = plan["launch"]
            assert jl != jc and not any(lane_valid[jl]), "a joint buffer is reloaded while lanes of it are still to be consumed"
            got = 0
            for k in range(J):
                b = next(src, None)
                if b is None:
                    break
                joint_in[jl][k] = b
                got += 1
            lane_valid[jl] = [k < got for k in range(J)]
            if got:
                joint_fps[jl] = [("fps", b) for b in joint_in[jl]]
                launched_at[jl] = t
        if set_valid[v1]:
            sets[v1]["geo"] = ("geo", sets[v1]["batch"], sets[v1]["fps"])
            read_pending[v1] = True
        busy = set_valid[v1] or any(lane_valid[0]) or any(lane_valid[1])
        t += 1
        assert t < 4 * (nbatches + 4 * J), "the pipeline does not drain"
    assert trained == list(range(nbatches))
    P = schedule.period(J)
    assert P % (2 * J) == 0 and P % schedule.SETS == 0 and all(schedule.tick_plan(k, J) == schedule.tick_plan(k + P, J) for k in range(P))



def test_confusion_matrix_counts_and_rejects_out_of_range_labels():
    """openpoints/utils/metrics.py:50-170 (CPU tensors here): the matrix, ignore_index, and labels outside the class range --
    left out of the histogram, reported by the first summary that reads the matrix back"""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    import torch
    from openpoints.utils import ConfusionMatrix
    true = torch.tensor([0, 1, 2, 2, 255, 1])
    pred = torch.tensor([0, 2, 2, 1, 0, 1])
    cm = ConfusionMatrix(3, ignore_index=255)
    cm.update(pred, true)
    assert cm.value.tolist() == [[1, 0, 0], [0, 1, 1], [0, 1, 1]]
    assert int(true[4]) == 255 and int(pred[4]) == 0  # the caller's tensors are left alone
    miou, macc, oa, ious, accs = cm.all_metrics()
    assert abs(oa - 60.0) < 1e-4
    cm.update(torch.tensor([0, 7, -1]), torch.tensor([0, 1, 2]))  # prediction 7 and -1: not classes, not ignore_index
    assert cm.value.tolist() == [[2, 0, 0], [0, 1, 1], [0, 1, 1]]
    with pytest.raises(ValueError, match="2 entries"):
        cm.all_metrics()
    cm.reset()
    cm.update(pred[:4], true[:4])
    cm.all_acc()
    with pytest.raises(ValueError):
        bad = ConfusionMatrix(3)  # no ignore_index: 255 is out of range
        bad.update(pred, true)
        bad.check()


def test_fused_adamw_has_no_cpu_path():
    import torch
    from amcontrast3d_amd.fused_optim import FusedAdamW
    with pytest.raises(RuntimeError, match="no CPU path"):
        FusedAdamW([torch.zeros(3, requires_grad=True)], lr=1e-3)


def test_main_AA_imports_and_call_sites_resolve_against_this_package(tmp_path):
    """north_star: "drops into examples/segmentation/main_AA.py unchanged".  The trainer's own import list (main_AA.py:14-31,
    recorded from the reference checkout in tests/golden/trainer_imports.json) is resolved name by name in a fresh interpreter
    with this package active as `openpoints` and AMC3D_REFERENCE_ROOT as overlay (mode B of INTEGRATION.md; the overlay is
    a stand-in with the reference's module layout, _stand_in_reference); third-party modules the image lacks (wandb,
    torch_scatter, tensorboard, easydict, ...) are empty stand-ins.  Every name must exist; the names on the hot path
    (build_model_from_cfg, build_criterion_from_cfg, build_optimizer_from_cfg, build_scheduler_from_cfg, the checkpoint
    helpers, ConfusionMatrix / get_mious / AverageMeter, posmask_searching / ambiguity_metrics) must come from THIS build;
    the call sites main_AA.py:142 (build_model_from_cfg(cfg.model)), :251-257 (build_criterion_from_cfg(cfg.criterion_args_Ace))
    and :390-394 (model(data) -> (logits, stageACE_list); criterion(logits, target, stageACE_list, num_classes, ignore_index,
    ambiguity_args)) are checked by signature."""
    import subprocess
    import sys
    ref = _stand_in_reference(tmp_path / "reference")
    # (module, name) of every `from openpoints... import ...` at module level of the trainer
    wanted = [tuple(w) for w in json.load(open(os.path.join(GOLDEN, "trainer_imports.json")))["trainer_imports"]]
    assert ("openpoints.models", "build_model_from_cfg") in wanted and ("openpoints.loss", "build_criterion_from_cfg") in wanted
    assert len(wanted) >= 30, wanted
    code = (
        "import sys, types, json, importlib, inspect\n"
        "class _Any(types.ModuleType):\n"
        "    def __getattr__(self, k):\n"
        "        if k.startswith('__'): raise AttributeError(k)\n"
        "        return type(k, (), {})\n"
        "for m in ('easydict', 'multimethod', 'termcolor', 'shortuuid', 'wandb', 'torch_scatter', 'h5py', 'pyvista', 'tensorboard',\n"
        "          'torch.utils.tensorboard', 'sklearn.manifold', 'matplotlib', 'matplotlib.pyplot', 'plyfile', 'pickle5'):\n"
        "    sys.modules.setdefault(m, _Any(m))\n"
        "sys.modules['easydict'].EasyDict = dict\n"
        "import amcontrast3d_amd; amcontrast3d_amd.activate()\n"
        "here = amcontrast3d_amd._HERE\n"
        "wanted = json.loads(sys.argv[1])\n"
        "out = {}\n"
        "for mod, name in wanted:\n"
        "    try:\n"
        "        obj = getattr(importlib.import_module(mod), name)\n"
        "        src = getattr(sys.modules.get(getattr(obj, '__module__', None) or mod), '__file__', '') or ''\n"
        "        out[mod + ':' + name] = 'ours' if src.startswith(here) else 'reference'\n"
        "    except Exception as e:\n"
        "        out[mod + ':' + name] = 'MISSING ' + type(e).__name__ + ': ' + str(e)[:200]\n"
        "from openpoints.models import build_model_from_cfg\n"
        "from openpoints.loss import build_criterion_from_cfg, LOSS\n"
        "from openpoints.models import MODELS\n"
        "out['sig:build_model_from_cfg'] = list(inspect.signature(build_model_from_cfg).parameters)\n"
        "out['sig:build_criterion_from_cfg'] = list(inspect.signature(build_criterion_from_cfg).parameters)\n"
        "out['sig:criterion'] = list(inspect.signature(LOSS.get('CrossEntropyAce').forward).parameters)\n"
        "out['sig:model'] = list(inspect.signature(MODELS.get('BaseSeg_AMContrast3D').forward).parameters)\n"
        "out['registered'] = [n for n in ('BaseSeg_AMContrast3D', 'PointNextEncoder_AMContrast3D', 'PointNextDecoder_AMContrast3D', 'SegHead',\n"
        "                                 'BaseSeg_M_AMContrast3D') if MODELS.get(n) is not None]\n"
        "print('RESULT ' + json.dumps(out))\n")
    env = dict(os.environ, AMC3D_REFERENCE_ROOT=ref)
    run = subprocess.run([sys.executable, "-c", code, json.dumps(wanted)], env=env, capture_output=True, text=True, timeout=600,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert run.returncode == 0, run.stderr[-3000:]
    res = json.loads([l for l in run.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    missing = {k: v for k, v in res.items() if isinstance(v, str) and v.startswith("MISSING")}
    assert not missing, missing
    ours = ["openpoints.models:build_model_from_cfg", "openpoints.loss:build_criterion_from_cfg", "openpoints.optim:build_optimizer_from_cfg",
            "openpoints.scheduler:build_scheduler_from_cfg", "openpoints.utils:save_checkpoint", "openpoints.utils:load_checkpoint",
            "openpoints.utils:resume_checkpoint", "openpoints.utils:EasyConfig", "openpoints.utils:ConfusionMatrix",
            "openpoints.utils:get_mious", "openpoints.utils:AverageMeter", "openpoints.AMContrast3D.metrics:posmask_searching",
            "openpoints.AMContrast3D.metrics:ambiguity_metrics"]
    for k in ours:
        assert res.get(k) == "ours", (k, res.get(k))
    for k in ("openpoints.dataset:build_dataloader_from_cfg", "openpoints.transforms:build_transforms_from_cfg",
              "openpoints.dataset.data_util:voxelize"):
        assert res.get(k) == "reference", (k, res.get(k))  # out of scope: resolved from the overlay
    assert res["sig:build_model_from_cfg"][0] == "cfg" and res["sig:build_criterion_from_cfg"][0] == "cfg"
    assert res["sig:criterion"][:7] == ["self", "logit", "target", "stageACE_list", "num_classes", "ignore_index", "ambiguity_args"], res["sig:criterion"]
    assert res["sig:model"][:2] == ["self", "data"], res["sig:model"]
    assert len(res["registered"]) == 5


def test_environment_switches_are_exactly_the_documented_ones():
    """every AMC3D_* name in the package's .py / .hip / .h sources has its row in INTEGRATION.md's table, and nothing else has:
    a new lever needs a documented reason to exist"""
    found = set()
    for base in (os.path.join(ROOT, "amcontrast3d_amd"), os.path.join(ROOT, "include")):
        for d, _, files in os.walk(base):
            for name in files:
                if name.endswith((".py", ".hip", ".h")):
                    found |= set(re.findall(r"AMC3D_[A-Z0-9_]+", open(os.path.join(d, name), errors="replace").read()))
    found.discard("AMC3D_H")  # the header's include guard
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text.split("## Environment variables", 1)[1].split("\n## ", 1)[0]
    table = set(re.findall(r"^\| `(AMC3D_[A-Z0-9_]+)` \|", section, flags=re.M))
    assert table and found == table, sorted(found ^ table)


def _conv_bn_block_cases():
    from openpoints.models.layers import create_convblock1d, create_convblock2d
    bn, relu = {"norm": "bn"}, {"act": "relu"}
    return [  # (block, matches, has relu, conv has a bias)
        (create_convblock2d(7, 16, norm_args=bn, act_args=relu), True, True, False),
        (create_convblock1d(7, 16, norm_args=bn, act_args=relu), True, True, False),
        (create_convblock2d(7, 16, norm_args=bn, act_args=None), True, False, False),
        (create_convblock1d(7, 16, norm_args=bn, act_args=None, bias=True), True, False, False),  # a norm drops the bias
        (torch.nn.Sequential(torch.nn.Conv1d(7, 16, 1, bias=False), torch.nn.SyncBatchNorm(16), torch.nn.ReLU()), True, True, False),
        (create_convblock1d(7, 16, norm_args=None, act_args=relu), False, None, None),            # conv (+ bias) -> ReLU
        (create_convblock1d(7, 16, norm_args=None, act_args=None), False, None, None),            # bare conv: the skip convs
        (create_convblock2d(7, 16, norm_args=bn, act_args={"act": "gelu"}), False, None, None),
        (create_convblock2d(7, 16, norm_args={"norm": "in"}, act_args=relu), False, None, None),
        (create_convblock2d(7, 16, 3, norm_args=bn, act_args=relu), False, None, None),           # 3-wide kernel
        (create_convblock1d(7, 16, 3, norm_args=bn, act_args=relu, padding=1), False, None, None),
        (create_convblock1d(7, 16, norm_args=bn, act_args=relu, stride=2), False, None, None),
        (create_convblock1d(8, 16, norm_args=bn, act_args=relu, groups=2), False, None, None),
        (create_convblock2d(7, 16, norm_args=bn, act_args=relu, order="norm-act-conv"), False, None, None),
        (create_convblock2d(7, 16, norm_args=bn, act_args=relu, order="conv-act-norm"), False, None, None),
        (torch.nn.Linear(7, 16), False, None, None),
    ]


@pytest.mark.parametrize("case", range(16))
def test_conv_bn_block_matches_only_pointwise_conv_batchnorm_relu(case):
    from openpoints.models.layers import blocks
    blk, matches, has_relu, has_bias = _conv_bn_block_cases()[case]
    m = blocks.conv_bn_block(blk)
    if not matches:
        assert m is None
        return
    conv, bn, relu = m
    assert conv is blk[0] and bn is blk[1] and (relu is blk[2] if has_relu else relu is None)
    assert isinstance(bn, torch.nn.modules.batchnorm._BatchNorm) and (conv.bias is not None) == has_bias
    assert all(k == 1 for k in conv.kernel_size)
