"""The training transforms of a config's `datatransforms` list, compiled into one program for csrc/transforms.hip.

`build_transforms_from_cfg(split, cfg)` takes what the reference's openpoints/transforms/transforms_factory.py:44-60 takes and
returns a `TransformChain` (or None for a missing / empty list).  Every class keeps the reference's constructor arguments,
defaults and meaning (transforms/point_transform_cpu.py, point_transformer_gpu.py); `kwargs` are the default arguments of every
class, as `DataTransforms.build(..., default_args=kwargs)` passes them.

The chain is compiled into micro-ops.  The compiler tracks, per tensor along the chain,
  * the dtype: numpy computes float32_array (op) float64_array in double and rounds when it assigns into the float32 array;
    np.dot(pos, R) and `pos * scale + jitter` leave `pos` float64 for every later op; PointsToTensor rounds it to float32;
    the torch classes work in float32.  The colours stay float32 throughout;
  * the domain: the torch classes need tensors (a PointsToTensor before them), the numpy classes need arrays;
  * the reduction phases: an op that reads a per-cloud statistic of the CURRENT state takes the earliest phase in which every
    earlier op of its stream (positions or colours) can be evaluated.  Statistics of the two streams that fall into the same
    phase share its launch.  The kernels run 1 + phases launches and store no intermediate of the batch's size.

Random numbers: `chain.draw(sizes, device, generator)` makes them per cloud on the device, in the order the reference's classes
draw them, keyed "<position in the chain>.<name>"; `chain(data, draws=...)` takes given ones (a recorded reference run).
Rotation matrices may be given ("<i>.R"); the reference forms RandomRotateZ's and PointCloudRotation's with
scipy.linalg.expm, the default here is cos / sin in double.  Means are double sums rounded once (the reference: float32 sums).

Caps (csrc/transforms.hip): 32 micro-ops, 4 reduction phases, 4 per-point draw tensors per chain."""
import ctypes
import math
import struct

import numpy as np
import torch

from . import _lib

MAX_OPS, MAX_PHASES, MAX_NOISE = 32, 4, 4

CODES = ["ROT_DOT", "SCALE_NP", "SCALE_JITTER_NP", "FLIP_NP", "JITTER_NP", "TO_F32", "SCALE_T", "TRANSLATE_T", "SCALE_TRANSLATE_T",
         "JITTER_T", "SCALE_JITTER_T", "ROT_T", "HEIGHTS_MIN", "CENTER", "SUB_MIN_G", "NORM_DIV", "HFLIP", "AUTOCONTRAST",
         "TRANSLATE_C", "JITTER_C", "HUESAT", "DROP", "PERDROP", "NORMALIZE"]  # csrc/transforms.hip: enum TfCode
CODE = {n: i for i, n in enumerate(CODES)}
_FIRST_COLOUR = CODE["AUTOCONTRAST"]
F32, F64 = "float32", "float64"


class _State:
    """what the compiler knows at one point of the chain"""

    def __init__(self, pos_dtype):
        self.pos, self.x, self.tensor = pos_dtype, F32, False


def _micro(code, slot=0, needs=None, share=False, iarg=0, f=(), d=(), noise=None):
    return {"code": code, "slot": slot, "needs": needs, "share": share, "iarg": iarg, "f": tuple(f), "d": tuple(d), "noise": noise}


def _rand(gen, dev, *shape, dtype=torch.float64):
    return torch.rand(*shape, dtype=dtype, device=dev, generator=gen)


def _randn(gen, dev, *shape, dtype=torch.float64):
    return torch.randn(*shape, dtype=dtype, device=dev, generator=gen)


_consts = {}


def _const(values, dtype, dev):
    """a small constant on the device, uploaded once (pinned staging, asynchronous) and kept"""
    key = (tuple(float(v) for v in values), dtype, str(dev))
    if key not in _consts:
        _consts[key] = torch.tensor(key[0], dtype=dtype).pin_memory().to(dev, non_blocking=True)
    return _consts[key]


def _f64(t, dev):
    return torch.as_tensor(t, device=dev).to(torch.float64)


class _Transform:
    """one class of the reference: `domain` (numpy / torch / any), `width` (doubles in the cloud's table row), `spec()` (the
    draws: name -> (kind, columns, dtype); kind "cloud": (B, columns), "point": (T, columns)), `emit(state)` (micro-ops, with the
    dtype bookkeeping), `row(d, B, dev)` ((B, width) float64 from the draws)"""
    domain, width = "numpy", 0

    def spec(self):
        return {}

    def draw(self, B, T, dev, gen):
        out = {}
        for name, (kind, cols, dtype) in self.spec().items():
            n = B if kind == "cloud" else T
            shape = (n,) if cols == 0 else (n, cols)
            out[name] = (_randn if name == "noise" else _rand)(gen, dev, *shape, dtype=dtype)
        return out

    def row(self, d, B, dev):
        return None


def _need(state, who, tensor):
    if tensor and not state.tensor:
        raise ValueError(f"{who} is one of the torch classes: it needs a PointsToTensor before it in the chain")
    if not tensor and state.tensor:
        raise ValueError(f"{who} is one of the numpy classes: it cannot follow PointsToTensor")


class PointsToTensor(_Transform):
    domain = "any"

    def __init__(self, **kwargs):
        pass

    def emit(self, st):
        st.tensor = True
        if st.pos == F64:
            st.pos = F32
            return [_micro("TO_F32")]
        return []


def _rot_xyz(theta):
    """(B,3) angles -> Rx, Ry, Rz (B,3,3) float64, cos / sin in double"""
    c, s = torch.cos(theta), torch.sin(theta)
    one, zero = torch.ones_like(c[:, 0]), torch.zeros_like(c[:, 0])
    B = theta.shape[0]
    rx = torch.stack([one, zero, zero, zero, c[:, 0], -s[:, 0], zero, s[:, 0], c[:, 0]], 1).view(B, 3, 3)
    ry = torch.stack([c[:, 1], zero, s[:, 1], zero, one, zero, -s[:, 1], zero, c[:, 1]], 1).view(B, 3, 3)
    rz = torch.stack([c[:, 2], -s[:, 2], zero, s[:, 2], c[:, 2], zero, zero, zero, one], 1).view(B, 3, 3)
    return rx, ry, rz


def _axis_rot(t, dim):
    """(B,) angles -> (B,9) row-major rotation about axis `dim` (cos / sin in double): six launches, whatever B"""
    c, s = torch.cos(t), torch.sin(t)
    i, j = (dim + 1) % 3, (dim + 2) % 3
    cols = [torch.zeros_like(c)] * 9
    cols[dim * 4] = torch.ones_like(c)
    cols[i * 4], cols[i * 3 + j], cols[j * 3 + i], cols[j * 4] = c, -s, s, c
    return torch.stack(cols, 1)


def _single_axis(angle):
    """the only axis with a non-zero bound, or None: the other two matrices are then exactly the identity"""
    on = [k for k, a in enumerate(angle) if a != 0]
    return on[0] if len(on) == 1 else None


class RandomRotate(_Transform):
    width = 9

    def __init__(self, angle=[0, 0, 1], **kwargs):
        self.angle = [float(a) for a in angle]

    def spec(self):
        return {"angle": ("cloud", 3, torch.float64)}  # np.random.uniform(-a, a) per axis, before * pi

    def draw(self, B, T, dev, gen):
        a = _const(self.angle, torch.float64, dev)
        return {"angle": -a + (a - -a) * _rand(gen, dev, B, 3)}

    def emit(self, st):
        _need(st, "RandomRotate", False)
        st.pos = F64
        return [_micro("ROT_DOT", iarg=2)]  # np.dot(pos, R.T): a one-point cloud goes through dgemv's order

    def row(self, d, B, dev):
        if d.get("R") is not None:
            R = _f64(d["R"], dev).reshape(B, 3, 3)
        elif _single_axis(self.angle) is not None:
            ax = _single_axis(self.angle)
            R = _axis_rot(_f64(d["angle"], dev).reshape(B, 3)[:, ax] * math.pi, ax).view(B, 3, 3)
        else:
            rx, ry, rz = _rot_xyz(_f64(d["angle"], dev) * math.pi)
            R = rz @ (ry @ rx)
        return R.transpose(1, 2).reshape(B, 9)  # np.dot(pos, R.T)


class RandomRotateZ(_Transform):
    width = 9

    def __init__(self, angle=1.0, rotate_dim=2, random_rotate=True, **kwargs):
        self.angle, self.rotate_dim, self.random_rotate = float(angle) * math.pi, int(rotate_dim), bool(random_rotate)

    def spec(self):
        return {"angle": ("cloud", 0, torch.float64)}

    def draw(self, B, T, dev, gen):
        if not self.random_rotate:
            return {"angle": torch.full((B,), self.angle, dtype=torch.float64, device=dev)}
        return {"angle": -self.angle + (self.angle - -self.angle) * _rand(gen, dev, B)}

    def emit(self, st):
        _need(st, "RandomRotateZ", False)
        st.pos = F64
        return [_micro("ROT_DOT")]

    def row(self, d, B, dev):
        if d.get("R") is not None:
            return _f64(d["R"], dev).reshape(B, 9)
        return _axis_rot(_f64(d["angle"], dev).reshape(B), self.rotate_dim)


class _NumpyScale(_Transform):
    """the scale draw RandomScale and RandomScaleAndJitter share (point_transform_cpu.py:82-91,116-125)"""

    def _init_scale(self, scale, scale_anisotropic, scale_xyz, mirror):
        self.scale, self.anisotropic = (float(scale[0]), float(scale[1])), bool(scale_anisotropic)
        self.scale_xyz, self.mirror = [bool(s) for s in scale_xyz], [float(m) for m in mirror]
        self.use_mirroring = any(m > 0 for m in self.mirror)

    def _scale_spec(self):
        s = {"scale": ("cloud", 3 if self.anisotropic else 1, torch.float64)}
        if self.use_mirroring:
            s["mirror_u"] = ("cloud", 3, torch.float64)
        return s

    def _draw_scale(self, B, dev, gen):
        lo, hi = self.scale
        d = {"scale": lo + (hi - lo) * _rand(gen, dev, B, 3 if self.anisotropic else 1)}
        if self.use_mirroring:
            d["mirror_u"] = _rand(gen, dev, B, 3)
        return d

    def _scale_row(self, d, B, dev):
        s = _f64(d["scale"], dev).reshape(B, -1).expand(B, 3).clone()
        if self.use_mirroring:
            thr = _const(self.mirror, torch.float64, dev)
            s = s * ((_f64(d["mirror_u"], dev) > thr).to(torch.float64) * 2 - 1)
        for k, on in enumerate(self.scale_xyz):
            if not on:
                s[:, k] = 1.0
        return s


class RandomScale(_NumpyScale):
    width = 3

    def __init__(self, scale=[0.8, 1.2], scale_anisotropic=False, scale_xyz=[True, True, True], mirror=[-1, -1, -1], **kwargs):
        self._init_scale(scale, scale_anisotropic, scale_xyz, mirror)

    def spec(self):
        return self._scale_spec()

    def draw(self, B, T, dev, gen):
        return self._draw_scale(B, dev, gen)

    def emit(self, st):
        _need(st, "RandomScale", False)
        return [_micro("SCALE_NP", iarg=int(st.pos == F64))]  # `pos *= scale`: in double, stored in pos's own dtype

    def row(self, d, B, dev):
        return self._scale_row(d, B, dev)


class RandomScaleAndJitter(_NumpyScale):
    width = 3

    def __init__(self, scale=[0.8, 1.2], scale_xyz=[True, True, True], scale_anisotropic=False, jitter_sigma=0.01, jitter_clip=0.05,
                 mirror=[-1, -1, -1], **kwargs):
        self._init_scale(scale, scale_anisotropic, scale_xyz, mirror)
        self.sigma, self.clip = float(jitter_sigma), float(jitter_clip)

    def spec(self):
        return dict(self._scale_spec(), noise=("point", 3, torch.float64))

    def draw(self, B, T, dev, gen):
        return dict(self._draw_scale(B, dev, gen), noise=_randn(gen, dev, T, 3))

    def emit(self, st):
        _need(st, "RandomScaleAndJitter", False)
        st.pos = F64  # pos * scale + jitter is a new float64 array
        return [_micro("SCALE_JITTER_NP", d=(self.sigma, self.clip), noise="noise")]

    def row(self, d, B, dev):
        return self._scale_row(d, B, dev)


class RandomFlip(_Transform):
    width = 2

    def __init__(self, p=0.5, **kwargs):
        self.p = float(p)

    def spec(self):
        return {"u": ("cloud", 2, torch.float64)}

    def emit(self, st):
        _need(st, "RandomFlip", False)
        return [_micro("FLIP_NP")]

    def row(self, d, B, dev):
        return (_f64(d["u"], dev) < self.p).to(torch.float64)


class RandomJitter(_Transform):
    def __init__(self, jitter_sigma=0.01, jitter_clip=0.05, **kwargs):
        self.sigma, self.clip = float(jitter_sigma), float(jitter_clip)

    def spec(self):
        return {"noise": ("point", 3, torch.float64)}

    def emit(self, st):
        _need(st, "RandomJitter", False)
        return [_micro("JITTER_NP", iarg=int(st.pos == F64), d=(self.sigma, self.clip), noise="noise")]


class ChromaticAutoContrast(_Transform):
    width = 3

    def __init__(self, p=0.2, blend_factor=None, **kwargs):
        self.p, self.blend_factor = float(p), blend_factor

    def spec(self):
        s = {"u": ("cloud", 0, torch.float64)}
        if self.blend_factor is None:
            s["blend"] = ("cloud", 0, torch.float64)  # drawn only when taken; unused otherwise
        return s

    def emit(self, st):
        _need(st, "ChromaticAutoContrast", False)
        return [_micro("AUTOCONTRAST", needs="x")]

    def row(self, d, B, dev):
        blend = (_f64(d["blend"], dev) if self.blend_factor is None
                 else torch.full((B,), float(self.blend_factor), dtype=torch.float64, device=dev))
        # (1 - blend) is formed in double and rounded once: numpy takes the Python double as a float32 operand
        w = torch.stack([1 - blend, blend], 1).float()
        return torch.cat([(_f64(d["u"], dev) < self.p).reshape(B, 1).float(), w], 1).to(torch.float64)


class ChromaticTranslation(_Transform):
    width = 4

    def __init__(self, p=0.95, ratio=0.05, **kwargs):
        self.p, self.ratio = float(p), float(ratio)

    def spec(self):
        return {"u": ("cloud", 0, torch.float64), "tr_u": ("cloud", 3, torch.float64)}

    def emit(self, st):
        _need(st, "ChromaticTranslation", False)
        return [_micro("TRANSLATE_C")]

    def row(self, d, B, dev):
        tr = (_f64(d["tr_u"], dev).reshape(B, 3) - 0.5) * 255 * 2 * self.ratio
        return torch.cat([(_f64(d["u"], dev) < self.p).to(torch.float64).reshape(B, 1), tr], 1)


class ChromaticJitter(_Transform):
    width = 1

    def __init__(self, p=0.95, std=0.005, **kwargs):
        self.p, self.std = float(p), float(std)

    def spec(self):
        return {"u": ("cloud", 0, torch.float64), "noise": ("point", 3, torch.float64)}

    def emit(self, st):
        _need(st, "ChromaticJitter", False)
        return [_micro("JITTER_C", d=(self.std * 255, 0.0), noise="noise")]

    def row(self, d, B, dev):
        return (_f64(d["u"], dev) < self.p).to(torch.float64).reshape(B, 1)


class HueSaturationTranslation(_Transform):
    width = 2

    def __init__(self, hue_max=0.5, saturation_max=0.2, **kwargs):
        self.hue_max, self.saturation_max = float(hue_max), float(saturation_max)

    def spec(self):
        return {"hue_u": ("cloud", 0, torch.float64), "sat_u": ("cloud", 0, torch.float64)}

    def emit(self, st):
        _need(st, "HueSaturationTranslation", False)
        return [_micro("HUESAT")]

    def row(self, d, B, dev):
        return torch.stack([(_f64(d["hue_u"], dev) - 0.5) * 2 * self.hue_max,
                            1 + (_f64(d["sat_u"], dev) - 0.5) * 2 * self.saturation_max], 1)


class RandomDropFeature(_Transform):
    width = 1

    def __init__(self, feature_drop=0.2, drop_dim=[0, 3], **kwargs):
        self.p, self.dim = float(feature_drop), [int(v) for v in drop_dim]

    def spec(self):
        return {"u": ("cloud", 0, torch.float64)}

    def emit(self, st):
        _need(st, "RandomDropFeature", False)
        cols = list(range(3))[self.dim[0]:self.dim[-1]]  # x[:, dim[0]:dim[-1]] of the three colour columns
        return [_micro("DROP", iarg=sum(1 << (8 + c) for c in cols))]

    def row(self, d, B, dev):
        return (_f64(d["u"], dev) < self.p).to(torch.float64).reshape(B, 1)


def _mean_std(color_mean, color_std):
    if color_mean is None:
        return 0, ()
    m, s = np.array(color_mean).astype(np.float32), np.array(color_std).astype(np.float32)
    return 1, tuple(float(v) for v in m) + tuple(float(v) for v in s)


class NumpyChromaticNormalize(_Transform):
    def __init__(self, color_mean=None, color_std=None, **kwargs):
        self.has, self.f = _mean_std(color_mean, color_std)

    def emit(self, st):
        _need(st, "NumpyChromaticNormalize", False)
        return [_micro("NORMALIZE", needs="x", iarg=self.has, f=self.f)]


# ---- the torch classes (point_transformer_gpu.py): float32 throughout


class PointCloudCenterAndNormalize(_Transform):
    domain = "torch"

    def __init__(self, centering=True, normalize=True, gravity_dim=2, append_xyz=False, **kwargs):
        if append_xyz:
            raise ValueError("PointCloudCenterAndNormalize(append_xyz=True) makes `heights` three columns wide; the batches here "
                             "carry heights (B,N,1)")
        self.centering, self.normalize, self.g = bool(centering), bool(normalize), int(gravity_dim)

    def emit(self, st):
        _need(st, "PointCloudCenterAndNormalize", True)
        ops = [_micro("HEIGHTS_MIN", needs="pos", iarg=self.g << 8)]
        if self.centering:
            ops.append(_micro("CENTER", needs="pos", share=True))
        if self.normalize:
            ops.append(_micro("NORM_DIV", needs="pos", share=not self.centering))
        return ops


class PointCloudXYZAlign(_Transform):
    domain = "torch"

    def __init__(self, gravity_dim=2, **kwargs):
        self.g = int(gravity_dim)

    def emit(self, st):
        _need(st, "PointCloudXYZAlign", True)
        # the minimum of the centred gravity column follows from the uncentred one (monotone): one phase
        return [_micro("CENTER", needs="pos"), _micro("SUB_MIN_G", needs="pos", share=True, iarg=self.g << 8)]


class RandomHorizontalFlip(_Transform):
    domain, width = "torch", 2

    def __init__(self, upright_axis, aug_prob=0.95, **kwargs):
        self.up, self.aug_prob = {"x": 0, "y": 1, "z": 2}[upright_axis.lower()], float(aug_prob)

    def spec(self):
        return {"u": ("cloud", 3, torch.float64)}  # random.random(): the gate, then one per horizontal axis (when the gate is taken)

    def emit(self, st):
        _need(st, "RandomHorizontalFlip", True)
        return [_micro("HFLIP", needs="pos", iarg=self.up << 8)]

    def row(self, d, B, dev):
        u = _f64(d["u"], dev).reshape(B, 3)
        return ((u[:, :1] < self.aug_prob) & (u[:, 1:] < 0.5)).to(torch.float64)


class _TorchScale(_Transform):
    """the scale draw of PointCloudScaling, PointCloudScaleAndTranslate and PointCloudScaleAndJitter (:149-159,196-207,248-257)"""
    domain = "torch"
    round_mirror = False

    def _init_scale(self, scale, anisotropic, scale_xyz, mirror):
        self.smin, self.smax = np.array(scale).astype(np.float32)
        self.anisotropic, self.scale_xyz = bool(anisotropic), [bool(s) for s in scale_xyz]
        self.mirror = [float(m) for m in mirror]
        self.use_mirroring = self.round_mirror or any(m > 0 for m in self.mirror)
        if self.use_mirroring and not self.anisotropic and not self.round_mirror:
            raise ValueError("mirroring needs anisotropic=True (the reference asserts it)")

    def _scale_spec(self):
        s = {"scale_u": ("cloud", 3 if self.anisotropic else 1, torch.float32)}
        if self.use_mirroring:
            s["mirror_u"] = ("cloud", 3, torch.float32)
        return s

    def _scale_row(self, d, B, dev):
        u = torch.as_tensor(d["scale_u"], device=dev).to(torch.float32).reshape(B, -1)
        s = (u * float(self.smax - self.smin) + float(self.smin)).expand(B, 3).clone()
        if self.use_mirroring:
            mu = torch.as_tensor(d["mirror_u"], device=dev).to(torch.float32).reshape(B, 3)
            thr = _const(self.mirror, torch.float32, dev)
            if self.round_mirror:  # PointCloudScaleAndJitter: round(rand) * 2 - 1, blended with the 0/1 `mirror` list
                m = torch.round(mu) * 2 - 1
                m = m * thr + (1 - thr)
            else:
                m = (mu > thr).to(torch.float32) * 2 - 1
            s = s * m
        for k, on in enumerate(self.scale_xyz):
            if not on:
                s[:, k] = 1.0
        return s.double()


class PointCloudScaling(_TorchScale):
    width = 3

    def __init__(self, scale=[2. / 3, 3. / 2], anisotropic=True, scale_xyz=[True, True, True], mirror=[0, 0, 0], **kwargs):
        self._init_scale(scale, anisotropic, scale_xyz, mirror)

    def spec(self):
        return self._scale_spec()

    def emit(self, st):
        _need(st, "PointCloudScaling", True)
        return [_micro("SCALE_T")]

    def row(self, d, B, dev):
        return self._scale_row(d, B, dev)


class PointCloudTranslation(_Transform):
    domain, width = "torch", 3

    def __init__(self, shift=[0.2, 0.2, 0.], **kwargs):
        self.shift = [float(np.float32(v)) for v in shift]

    def spec(self):
        return {"u": ("cloud", 3, torch.float32)}

    def emit(self, st):
        _need(st, "PointCloudTranslation", True)
        return [_micro("TRANSLATE_T")]

    def row(self, d, B, dev):
        u = torch.as_tensor(d["u"], device=dev).to(torch.float32).reshape(B, 3)
        return (u * _const(self.shift, torch.float32, dev)).double()


class PointCloudScaleAndTranslate(_TorchScale):
    width = 6

    def __init__(self, scale=[2. / 3, 3. / 2], scale_xyz=[True, True, True], anisotropic=True, shift=[0.2, 0.2, 0.2], mirror=[0, 0, 0],
                 **kwargs):
        self._init_scale(scale, anisotropic, scale_xyz, mirror)
        self.shift = [float(np.float32(v)) for v in shift]

    def spec(self):
        return dict(self._scale_spec(), shift_u=("cloud", 3, torch.float32))

    def emit(self, st):
        _need(st, "PointCloudScaleAndTranslate", True)
        return [_micro("SCALE_TRANSLATE_T")]

    def row(self, d, B, dev):
        u = torch.as_tensor(d["shift_u"], device=dev).to(torch.float32).reshape(B, 3)
        t = (u - 0.5) * 2 * _const(self.shift, torch.float32, dev)
        return torch.cat([self._scale_row(d, B, dev), t.double()], 1)


class PointCloudJitter(_Transform):
    domain = "torch"

    def __init__(self, jitter_sigma=0.01, jitter_clip=0.05, **kwargs):
        self.std, self.clip = float(jitter_sigma), float(jitter_clip)

    def spec(self):
        return {"noise": ("point", 3, torch.float32)}

    def emit(self, st):
        _need(st, "PointCloudJitter", True)
        return [_micro("JITTER_T", f=(self.std, self.clip), noise="noise")]


class PointCloudScaleAndJitter(_TorchScale):
    width, round_mirror = 3, True

    def __init__(self, scale=[2. / 3, 3. / 2], scale_xyz=[True, True, True], anisotropic=True, jitter_sigma=0.01, jitter_clip=0.05,
                 mirror=[0, 0, 0], **kwargs):
        self._init_scale(scale, anisotropic, scale_xyz, mirror)
        self.std, self.clip = float(jitter_sigma), float(jitter_clip)

    def spec(self):
        return dict(self._scale_spec(), noise=("point", 3, torch.float32))

    def emit(self, st):
        _need(st, "PointCloudScaleAndJitter", True)
        return [_micro("SCALE_JITTER_T", f=(self.std, self.clip), noise="noise")]

    def row(self, d, B, dev):
        return self._scale_row(d, B, dev)


class PointCloudRotation(_Transform):
    domain, width = "torch", 9

    def __init__(self, angle=[0, 0, 0], **kwargs):
        self.angle = [float(a) * math.pi for a in angle]

    def spec(self):
        return {"theta": ("cloud", 3, torch.float64), "order": ("cloud", 3, torch.int64)}

    def draw(self, B, T, dev, gen):
        a = _const(self.angle, torch.float64, dev)
        theta = -a + (a - -a) * _rand(gen, dev, B, 3)
        return {"theta": theta, "order": torch.argsort(_rand(gen, dev, B, 3), 1)}  # np.random.shuffle of the three matrices

    def emit(self, st):
        _need(st, "PointCloudRotation", True)
        return [_micro("ROT_T")]

    def row(self, d, B, dev):
        if d.get("R") is not None:
            R = _f64(d["R"], dev).reshape(B, 3, 3)
        elif _single_axis(self.angle) is not None:  # the shuffled product of one rotation and two identities
            ax = _single_axis(self.angle)
            R = _axis_rot(_f64(d["theta"], dev).reshape(B, 3)[:, ax], ax)
        else:
            m = torch.stack(_rot_xyz(_f64(d["theta"], dev).reshape(B, 3)), 1)  # (B, 3 axes, 3, 3)
            o = torch.as_tensor(d["order"], device=dev).to(torch.int64).reshape(B, 3)
            pick = lambda k: m[torch.arange(B, device=dev), o[:, k]]  # noqa: E731
            R = pick(0) @ pick(1) @ pick(2)
        return R.float().double().reshape(B, 9)


class ChromaticDropGPU(_Transform):
    domain, width = "any", 1  # torch.rand(1) and a slice assignment: works on arrays and tensors alike

    def __init__(self, color_drop=0.2, **kwargs):
        self.color_drop = float(color_drop)

    def spec(self):
        return {"u": ("cloud", 0, torch.float32)}

    def emit(self, st):
        return [_micro("DROP", iarg=7 << 8)]

    def row(self, d, B, dev):
        return (torch.as_tensor(d["u"], device=dev).to(torch.float32).reshape(B) < self.color_drop).to(torch.float64).reshape(B, 1)


class ChromaticPerDropGPU(_Transform):
    domain = "torch"

    def __init__(self, color_drop=0.2, **kwargs):
        self.color_drop = float(color_drop)

    def spec(self):
        return {"noise": ("point", 0, torch.float32)}  # torch.rand((N, 1)): the mask is u > color_drop

    def draw(self, B, T, dev, gen):
        return {"noise": _rand(gen, dev, T, dtype=torch.float32)}

    def emit(self, st):
        _need(st, "ChromaticPerDropGPU", True)
        return [_micro("PERDROP", f=(float(np.float32(self.color_drop)),), noise="noise")]


class ChromaticNormalize(_Transform):
    domain = "torch"

    def __init__(self, color_mean=[0.5136457, 0.49523646, 0.44921124], color_std=[0.18308958, 0.18415008, 0.19252081], **kwargs):
        self.has, self.f = _mean_std(color_mean, color_std)

    def emit(self, st):
        _need(st, "ChromaticNormalize", True)
        return [_micro("NORMALIZE", needs="x", iarg=self.has, f=self.f)]


REGISTRY = {c.__name__: c for c in (
    PointsToTensor, RandomRotate, RandomRotateZ, RandomScale, RandomScaleAndJitter, RandomFlip, RandomJitter, ChromaticAutoContrast,
    ChromaticTranslation, ChromaticJitter, HueSaturationTranslation, RandomDropFeature, NumpyChromaticNormalize,
    PointCloudCenterAndNormalize, PointCloudXYZAlign, RandomHorizontalFlip, PointCloudScaling, PointCloudTranslation,
    PointCloudScaleAndTranslate, PointCloudJitter, PointCloudScaleAndJitter, PointCloudRotation, ChromaticDropGPU, ChromaticPerDropGPU,
    ChromaticNormalize)}

UNSUPPORTED = {
    "RandomDropout": "it changes the number of points, and the collate stacks clouds of one size",
    "PointCloudToTensor": "it works on a different data dict (colors / normals, channel-first)",
    "RandomShift": "the reference's own __call__ reads self.shift_range, which its __init__ never sets: it cannot run there either",
    "RandomScaleAndTranslate": "the reference's own __call__ reads self.anisotropic and self.shift_range, which its __init__ never "
                               "sets: it cannot run there either",
}


class TransformChain:
    """a compiled chain.  `names`: the list as configured; `ops`: the transform objects; `gravity_dim`: kwargs' gravity_dim (2)"""

    def __init__(self, names, kwargs=None):
        kwargs = dict(kwargs or {})
        self.names, self.ops = list(names), []
        for name in self.names:
            if name in UNSUPPORTED:
                raise ValueError(f"{name} is not supported: {UNSUPPORTED[name]}")
            if name not in REGISTRY:
                raise KeyError(f"{name} is not in the datatransforms registry")
            self.ops.append(REGISTRY[name](**kwargs))
        self.gravity_dim = int(kwargs.get("gravity_dim", 2))
        if not 0 <= self.gravity_dim <= 2:
            raise ValueError("gravity_dim must be 0, 1 or 2")
        self._plans, self._device = {}, {}
        self.plan(F32)  # compile now: a chain that cannot run raises where it is built

    # ---- the compiler
    def plan(self, pos_dtype=F32):
        """the compiled program as data, for positions that come in as `pos_dtype`"""
        pos_dtype = str(pos_dtype).replace("torch.", "")
        if pos_dtype not in (F32, F64):
            raise ValueError("positions are float32 or float64")
        if pos_dtype in self._plans:
            return self._plans[pos_dtype]
        st = _State(pos_dtype)
        ready, last, masks = {"pos": 0, "x": 0}, {"pos": None, "x": None}, []
        micro, dtypes, noise, slot = [], [], [], 0
        for i, op in enumerate(self.ops):
            for m in op.emit(st):
                m = dict(m, op=i, slot=slot + m["slot"], phase=-1)
                if m["needs"] is not None:
                    s = m["needs"]
                    if m["share"] and last[s] is not None:
                        m["phase"] = last[s]  # a statistic of the same state as the transform's previous micro-op
                    else:
                        m["phase"] = last[s] = ready[s]
                        ready[s] += 1
                        while len(masks) <= m["phase"]:
                            masks.append(0)
                    masks[m["phase"]] |= 1 if s == "pos" else 2
                if m["noise"] is not None:
                    noise.append(f"{i}.{m['noise']}")
                    m["iarg"] |= (len(noise) - 1) << 8
                micro.append(m)
            slot += op.width
            dtypes.append((st.pos, st.x))
        if len(micro) > MAX_OPS:
            raise ValueError(f"the chain compiles to {len(micro)} micro-ops; the program table holds {MAX_OPS}")
        if len(masks) > MAX_PHASES:
            raise ValueError(f"the chain needs {len(masks)} reduction phases; the kernels hold {MAX_PHASES}")
        if len(noise) > MAX_NOISE:
            raise ValueError(f"the chain uses {len(noise)} per-point draw tensors; the kernels take {MAX_NOISE}")
        plan = {"ops": list(self.names), "dtypes": dtypes, "in_dtype": pos_dtype, "out_dtype": st.pos,
                "micro": [(m["code"], m["op"], m["phase"]) for m in micro], "phases": len(masks), "phase_masks": list(masks),
                "launches": 1 + len(masks), "noise": noise, "stride": max(slot, 1), "_micro": micro}
        self._plans[pos_dtype] = plan
        return plan

    def _program(self, plan):
        buf = struct.pack("8i", len(plan["_micro"]), plan["phases"], plan["stride"], self.gravity_dim,
                          *(plan["phase_masks"] + [0] * MAX_PHASES)[:MAX_PHASES])
        for m in plan["_micro"]:
            f, d = (list(m["f"]) + [0.0] * 8)[:8], (list(m["d"]) + [0.0] * 2)[:2]
            buf += struct.pack("4i8f2d", CODE[m["code"]], m["phase"], m["slot"], m["iarg"], *f, *d)
        buf += b"\0" * (32 + 64 * MAX_OPS - len(buf))
        return buf

    # ---- the draws
    def spec(self):
        """name -> (kind, columns, dtype) of every draw of the chain"""
        return {f"{i}.{k}": v for i, op in enumerate(self.ops) for k, v in op.spec().items()}

    def draw(self, sizes, device, generator=None):
        """the random numbers of one batch, on `device`, in the order the reference's classes draw theirs.  sizes: the point
        count of every cloud (host integers)"""
        B, T = len(sizes), int(sum(sizes))
        out = {}
        for i, op in enumerate(self.ops):
            for k, v in op.draw(B, T, torch.device(device), generator).items():
                out[f"{i}.{k}"] = v
        return out

    def _check_draws(self, d, B, T):
        for key, (kind, cols, _) in self.spec().items():
            i, name = key.split(".", 1)
            if name in ("angle", "theta", "order") and d.get(f"{i}.R") is not None:
                continue
            if key not in d:
                raise ValueError(f"draws: {key} is missing")
            n = B if kind == "cloud" else T
            if int(torch.as_tensor(d[key]).numel()) != n * max(cols, 1) or int(torch.as_tensor(d[key]).shape[0]) != n:
                raise ValueError(f"draws: {key} has shape {tuple(torch.as_tensor(d[key]).shape)}, expected {(n, cols) if cols else (n,)}")
        for key, v in d.items():
            if key.endswith(".R") and v is not None and int(torch.as_tensor(v).numel()) != B * 9:
                raise ValueError(f"draws: {key} has shape {tuple(torch.as_tensor(v).shape)}, expected {(B, 3, 3)}")

    # ---- the call
    def __call__(self, data, draws=None, generator=None, scannet_colour=False, want_heights=True):
        """data: {"pos": (B,N,3), "x": (B,N,3)} or {"pos": (T,3), "x": (T,3), "offsets": (B+1) int64 [, "sizes": host list]} on
        the GPU; pos float32 or float64, x float32.  Returns a new dict: pos (float32 or float64, as the reference's chain ends),
        x float32, heights (.., 1) float32, in the input's layout.  Ragged offsets are validated from `sizes` when it is given
        (no read-back) and by reading them back otherwise.  scannet_colour: x is ScanNet's [-1, 1] feature and becomes
        (x + 1) * 127.5 first, as ScanNet.__getitem__ does before its transform."""
        pos, x = data["pos"], data["x"]
        if not (pos.is_cuda and x.is_cuda):
            raise RuntimeError("TransformChain runs on the GPU only (there is no CPU path)")
        if pos.dtype not in (torch.float32, torch.float64) or x.dtype != torch.float32:
            raise ValueError("pos must be float32 or float64 and x float32")
        if pos.shape != x.shape or pos.shape[-1] != 3 or pos.dim() not in (2, 3):
            raise ValueError("pos and x must both be (B,N,3) or (T,3)")
        dev, dense = pos.device, pos.dim() == 3
        if dense:
            if "offsets" in data and data["offsets"] is not None:
                raise ValueError("a dense (B,N,3) batch takes no offsets")
            B, N = int(pos.shape[0]), int(pos.shape[1])
            if B == 0 or N == 0:
                raise ValueError("empty clouds")
            sizes = [N] * B
            key = ("off", B, N)
            if key not in self._dev(dev):
                self._dev(dev)[key] = torch.arange(B + 1, dtype=torch.int64, device=dev) * N
            offsets = self._dev(dev)[key]
        else:
            offsets = data.get("offsets")
            if offsets is None or offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 2 or not offsets.is_cuda:
                raise ValueError("ragged clouds need offsets (B+1) int64 on the GPU")
            sizes = data.get("sizes")
            if sizes is None:
                o = offsets.cpu()
                if int(o[0]) != 0:
                    raise ValueError("offsets must start at 0")
                sizes = [int(v) for v in (o[1:] - o[:-1])]
            sizes = [int(s) for s in sizes]
            if len(sizes) != offsets.numel() - 1:
                raise ValueError("sizes and offsets disagree")
            if any(s < 0 for s in sizes):
                raise ValueError("offsets must not decrease")
            if any(s == 0 for s in sizes):
                raise ValueError("empty rooms are not supported")
            if sum(sizes) != pos.shape[0]:
                raise ValueError("offsets[-1] must be the number of points")
            B = len(sizes)
        T = int(sum(sizes))
        plan = self.plan(pos.dtype)
        d = draws if draws is not None else self.draw(sizes, dev, generator)
        self._check_draws(d, B, T)
        pos, x, offsets = pos.contiguous(), x.contiguous(), offsets.contiguous()
        rows = []
        for i, op in enumerate(self.ops):
            if op.width:
                own = {k.split(".", 1)[1]: v for k, v in d.items() if k.split(".", 1)[0] == str(i)}
                rows.append(op.row(own, B, dev).reshape(B, op.width))
        table = torch.cat(rows, 1).contiguous() if rows else torch.zeros(B, 1, dtype=torch.float64, device=dev)
        noise = []
        for key in plan["noise"]:
            _, cols, dtype = self.spec()[key]
            noise.append(torch.as_tensor(d[key], device=dev).to(dtype).contiguous())
        pkey = ("prog", plan["in_dtype"])
        if pkey not in self._dev(dev):
            self._dev(dev)[pkey] = torch.frombuffer(bytearray(self._program(plan)), dtype=torch.uint8).to(dev)
        prog = self._dev(dev)[pkey]
        out64 = plan["out_dtype"] == F64
        pos_out = torch.empty(pos.shape, dtype=torch.float64 if out64 else torch.float32, device=dev)
        x_out = torch.empty_like(x)
        heights = torch.empty(pos.shape[:-1] + (1,), dtype=torch.float32, device=dev) if want_heights else None
        lib = _lib.load()
        wb = int(lib.amc3d_transform_workspace_bytes(B, T, plan["phases"]))
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        nz = (ctypes.c_void_p * MAX_NOISE)(*[t.data_ptr() for t in noise])
        P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        flags = int(pos.dtype == torch.float64) | (2 if scannet_colour else 0) | (4 if out64 else 0)
        with torch.cuda.device(dev):
            _lib.check(lib.amc3d_transform_chain(B, T, plan["phases"], P(offsets), P(prog), P(table), nz, flags, P(pos), P(x),
                                                 P(pos_out), P(x_out), P(heights), P(work), wb,
                                                 ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "transform_chain")
        out = {"pos": pos_out, "x": x_out}
        if want_heights:
            out["heights"] = heights
        return out

    def _dev(self, dev):
        return self._device.setdefault(str(dev), {})


def build_transforms_from_cfg(split, datatransforms_cfg):
    """the reference's transforms_factory.build_transforms_from_cfg for the device: the `split` list of `datatransforms_cfg`
    with its `kwargs` as every class's default arguments -> TransformChain, or None for a missing or empty list"""
    names = datatransforms_cfg.get(split, None)
    kwargs = datatransforms_cfg.get("kwargs", None)
    compose = datatransforms_cfg.get("compose_fn", "Compose")
    if compose != "Compose":
        raise ValueError(f"compose_fn {compose!r}: only Compose is supported")
    if names is None or len(names) == 0:
        return None
    return TransformChain(list(names), kwargs)
