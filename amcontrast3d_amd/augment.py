"""The loader's training transforms on the device, for a whole batch of cropped clouds at once.

The reference applies `cfgs/s3dis/default.yaml:33-43`'s chain -- ChromaticAutoContrast, PointsToTensor, PointCloudScaling,
PointCloudXYZAlign, PointCloudRotation, PointCloudJitter, ChromaticDropGPU, ChromaticNormalize (openpoints/transforms/
point_transform_cpu.py:8-19,192-209, point_transformer_gpu.py:70-89,135-164,216-229,267-311,373-409) -- per cloud inside
`S3DIS.__getitem__` (dataset/s3dis/s3dis.py:136-143), in loader worker processes.  With the step at 7 ms the six workers of
the reference's loader cannot keep up; `S3DISTrainAugment` does the same arithmetic for the (B,N,3) batch in two launches
(csrc/augment.hip), after `input_pipeline.crop_pc`.  Same parameters (the config's `kwargs`), same order of operations, the
random numbers drawn per cloud from a device generator (or passed in: `draws`); `heights` is, as in the reference, the gravity
coordinate of the cloud BEFORE the transforms.  Oracle: oracle/augment_ref.py, pinned by tests/golden/augment_s3dis.npz
(recorded from the reference's own classes); tests/test_gpu_augment.py."""
import ctypes

import torch

from . import _lib


class S3DISTrainAugment:
    def __init__(self, scale=(0.9, 1.1), angle=(0, 0, 1), jitter_sigma=0.005, jitter_clip=0.02, color_drop=0.2, contrast_p=0.2,
                 blend_factor=None, gravity_dim=2, color_mean=(0.5136457, 0.49523646, 0.44921124),
                 color_std=(0.18308958, 0.18415008, 0.19252081), **kwargs):
        self.scale, self.angle = (float(scale[0]), float(scale[1])), tuple(float(a) for a in angle)
        self.sigma, self.clip, self.color_drop, self.contrast_p = float(jitter_sigma), float(jitter_clip), float(color_drop), float(contrast_p)
        self.blend_factor, self.g = blend_factor, int(gravity_dim)
        self.color_mean, self.color_std = tuple(color_mean), tuple(color_std)
        self._const = {}

    def draw(self, B, N, device, generator=None):
        """the random numbers of one batch, per cloud, in the order the reference's classes draw them"""
        r = lambda *s: torch.rand(*s, device=device, generator=generator)  # noqa: E731
        import math
        bound = torch.tensor([a * math.pi for a in self.angle], device=device, dtype=torch.float64)
        return {"contrast": r(B) < self.contrast_p,
                "blend": r(B) if self.blend_factor is None else torch.full((B,), float(self.blend_factor), device=device),
                "scale_u": r(B, 3), "theta": (r(B, 3).double() * 2 - 1) * bound,
                "noise": torch.randn(B, N, 3, device=device, generator=generator), "drop": r(B) < self.color_drop}

    def params(self, d):
        """(B,24) per-cloud records of amc3d_augment_clouds from a set of draws"""
        B, dev = d["scale_u"].shape[0], d["scale_u"].device
        lo, hi = torch.tensor(self.scale[0], dtype=torch.float32), torch.tensor(self.scale[1], dtype=torch.float32)
        scale = d["scale_u"].float() * (hi - lo).to(dev) + lo.to(dev)  # point_transformer_gpu.py:151-152
        t = d["theta"].double()
        c, s, one, zero = torch.cos(t), torch.sin(t), torch.ones(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)
        rx = torch.stack([one, zero, zero, zero, c[:, 0], -s[:, 0], zero, s[:, 0], c[:, 0]], 1).view(B, 3, 3)
        ry = torch.stack([c[:, 1], zero, s[:, 1], zero, one, zero, -s[:, 1], zero, c[:, 1]], 1).view(B, 3, 3)
        rz = torch.stack([c[:, 2], -s[:, 2], zero, s[:, 2], c[:, 2], zero, zero, zero, one], 1).view(B, 3, 3)
        rot = (rx @ ry @ rz).float()  # expm of the axis generators (:272-274); the reference shuffles the order of the three
        p = torch.zeros(B, 24, dtype=torch.float32, device=dev)
        p[:, 0] = d["contrast"].float()
        p[:, 1] = d["blend"].float()
        p[:, 2:5] = scale
        p[:, 5:14] = rot.reshape(B, 9)
        p[:, 14] = d["drop"].float()
        return p

    def __call__(self, pos, color, draws=None, generator=None):
        """pos (B,N,3) fp32 cropped clouds, color (B,N,3) fp32 -> (pos', x (B,N,3) normalised colours, heights (B,N,1))"""
        if not (pos.is_cuda and color.is_cuda):
            raise RuntimeError("S3DISTrainAugment runs on the GPU only (there is no CPU path)")
        assert pos.dtype == color.dtype == torch.float32 and pos.shape == color.shape and pos.dim() == 3 and pos.shape[2] == 3
        pos, color = pos.contiguous(), color.contiguous()
        B, N, dev = pos.shape[0], pos.shape[1], pos.device
        d = draws if draws is not None else self.draw(B, N, dev, generator)
        par = self.params(d).contiguous()
        noise = d["noise"].to(torch.float32).contiguous()
        key = str(dev)
        if key not in self._const:
            self._const[key] = (torch.tensor(self.color_mean, dtype=torch.float32, device=dev),
                                torch.tensor(self.color_std, dtype=torch.float32, device=dev))
        mean, std = self._const[key]
        pos_out, x_out = torch.empty_like(pos), torch.empty_like(color)
        heights = torch.empty(B, N, 1, dtype=torch.float32, device=dev)
        lib = _lib.load()
        wb = int(lib.amc3d_augment_workspace_bytes(B))
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        with torch.cuda.device(dev):
            _lib.check(lib.amc3d_augment_clouds(B, N, self.g, self.sigma, self.clip, P(pos), P(color), P(noise), P(par), P(mean), P(std),
                                                P(pos_out), P(x_out), P(heights), P(work), wb,
                                                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "augment_clouds")
        return pos_out, x_out, heights


class ScanNetTrainAugment:
    """ScanNet's training chain, `cfgs/scannet/default.yaml` datatransforms.train: RandomRotateZ, RandomScale,
    ChromaticAutoContrast, RandomDropFeature, NumpyChromaticNormalize (transforms/point_transform_cpu.py:43-92,192-209,
    304-332), applied as ScanNet.__getitem__ applies it (dataset/scannetv2/scannet.py:140-166): to the WHOLE raw room, before
    crop_pc, after the colours went from [-1, 1] to (feat + 1) * 127.5.  For a batch of ragged rooms in four launches
    (csrc/scannet_input.hip: three for the per-room colour statistics, one elementwise pass).  The positions come out
    float64, as np.dot(pos_f32, R_f64) leaves them, and input_pipeline.crop_pc / scannet_train_batch keep them float64.

    Same parameters as the reference's classes read from the config's `kwargs`, with the defaults those classes fall back
    on (RandomDropFeature reads `feature_drop`, not the config's `color_drop`; ChromaticAutoContrast's `p` is 0.2).
    Random numbers: `draw` makes them per room, in the order the classes draw theirs -- angle, scale, mirror rand(3),
    contrast rand [, blend], drop rand -- or they are passed in (`draws`).  The rotation matrix itself may be passed as
    draws["R"]: the reference forms it with scipy.linalg.expm, which differs from cos / sin by up to a dozen ulp; the
    default is cos / sin in double on the host."""

    def __init__(self, angle=1.0, rotate_dim=2, random_rotate=True, scale=(0.8, 1.2), scale_anisotropic=False,
                 scale_xyz=(True, True, True), mirror=(-1, -1, -1), p=0.2, blend_factor=None, feature_drop=0.2, drop_dim=(0, 3),
                 color_mean=None, color_std=None, **kwargs):
        import math
        if list(drop_dim) != [0, 3]:
            raise NotImplementedError("RandomDropFeature: only drop_dim [0, 3] (the colours) is supported")
        self.angle, self.rotate_dim, self.random_rotate = float(angle) * math.pi, int(rotate_dim), bool(random_rotate)
        self.scale, self.anisotropic = (float(scale[0]), float(scale[1])), bool(scale_anisotropic)
        self.scale_xyz, self.mirror = tuple(bool(s) for s in scale_xyz), tuple(float(m) for m in mirror)
        self.use_mirroring = any(m > 0 for m in self.mirror)
        self.p, self.blend_factor, self.feature_drop = float(p), blend_factor, float(feature_drop)
        self.color_mean = tuple(float(v) for v in color_mean) if color_mean is not None else None
        self.color_std = tuple(float(v) for v in color_std) if color_std is not None else None
        self._const = {}

    def draw(self, B, generator=None, device=None):
        """the random numbers of B rooms, as float64 host tensors; one read-back when `generator` lives on the GPU"""
        dev = generator.device if generator is not None else (device or "cpu")
        u = torch.rand(B, 10, dtype=torch.float64, device=dev, generator=generator).cpu()
        lo, hi = self.scale
        return {"angle": -self.angle + 2 * self.angle * u[:, 0] if self.random_rotate else torch.full((B,), self.angle, dtype=torch.float64),
                "scale": lo + (hi - lo) * (u[:, 1:4] if self.anisotropic else u[:, 1]),
                "mirror_u": u[:, 4:7], "contrast_u": u[:, 7], "blend": u[:, 8], "drop_u": u[:, 9]}

    def rotation(self, angle):
        """(3,3) float64 R of RandomRotateZ.M(axis, angle) (pos' = pos @ R), from cos / sin"""
        import math
        c, s = math.cos(float(angle)), math.sin(float(angle))
        i, j = (self.rotate_dim + 1) % 3, (self.rotate_dim + 2) % 3
        R = torch.eye(3, dtype=torch.float64)
        R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
        return R

    def params(self, d):
        """(B,16) float64 per-room records of amc3d_scannet_room_stats / amc3d_scannet_transform_rooms, on the host"""
        import numpy as np
        scale = torch.as_tensor(d["scale"], dtype=torch.float64).cpu()
        B = scale.shape[0]
        p = torch.zeros(B, 16, dtype=torch.float64)
        for b in range(B):
            R = torch.as_tensor(d["R"][b], dtype=torch.float64) if d.get("R") is not None else self.rotation(float(d["angle"][b]))
            p[b, 0:9] = R.reshape(9)
            s = [float(v) for v in scale[b]] if scale.dim() == 2 else [float(scale[b])] * 3
            if self.use_mirroring:  # (np.random.rand(3) > mirror).astype(np.float32) * 2 - 1
                s = [v if float(d["mirror_u"][b][k]) > self.mirror[k] else -v for k, v in enumerate(s)]
            p[b, 9:12] = torch.tensor([v if self.scale_xyz[k] else 1.0 for k, v in enumerate(s)], dtype=torch.float64)
            contrast = float(d["contrast_u"][b]) < self.p
            blend = float(self.blend_factor) if self.blend_factor is not None else float(d["blend"][b])
            p[b, 12] = float(contrast)
            p[b, 13] = float(np.float32(1 - blend))  # NEP 50: the Python-double weights become float32 before the product
            p[b, 14] = float(np.float32(blend))
            p[b, 15] = float(float(d["drop_u"][b]) < self.feature_drop)
        return p

    def __call__(self, coord, feat, offsets, draws=None, generator=None):
        """coord (T,3) fp32, feat (T,3) fp32 in [-1, 1] (the rooms' .pth arrays, concatenated), offsets (B+1) int64 on the GPU
        -> (pos (T,3) float64, x (T,3) fp32 normalised colours, stats (B,8) fp32 {colour lo[3], hi[3], max after contrast and
        drop, unused})"""
        if not (coord.is_cuda and feat.is_cuda and offsets.is_cuda):
            raise RuntimeError("ScanNetTrainAugment runs on the GPU only (there is no CPU path)")
        assert coord.dtype == feat.dtype == torch.float32 and coord.shape == feat.shape and coord.dim() == 2 and coord.shape[1] == 3
        assert offsets.dtype == torch.int64 and offsets.dim() == 1
        coord, feat, offsets = coord.contiguous(), feat.contiguous(), offsets.contiguous()
        B, T, dev = offsets.shape[0] - 1, coord.shape[0], coord.device
        d = draws if draws is not None else self.draw(B, generator, dev)
        par = self.params(d).to(dev)
        key = str(dev)
        if key not in self._const:
            mean = self.color_mean if self.color_mean is not None else (0.0, 0.0, 0.0)  # (x - 0) / 1 == x exactly
            std = self.color_std if self.color_std is not None else (1.0, 1.0, 1.0)
            self._const[key] = (torch.tensor(mean, dtype=torch.float32, device=dev), torch.tensor(std, dtype=torch.float32, device=dev))
        mean, std = self._const[key]
        pos = torch.empty(T, 3, dtype=torch.float64, device=dev)
        x = torch.empty(T, 3, dtype=torch.float32, device=dev)
        stats = torch.empty(B, 8, dtype=torch.float32, device=dev)
        lib = _lib.load()
        wb = int(lib.amc3d_scannet_stats_workspace_bytes(B))
        work = torch.empty(max(wb, 8), dtype=torch.uint8, device=dev)
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        with torch.cuda.device(dev):
            _lib.check(lib.amc3d_scannet_room_stats(B, P(offsets), P(feat), P(par), P(stats), P(work), wb, stream), "scannet_room_stats")
            _lib.check(lib.amc3d_scannet_transform_rooms(B, T, P(offsets), P(coord), P(feat), P(par), P(stats), P(mean), P(std),
                                                         P(pos), P(x), stream), "scannet_transform_rooms")
        return pos, x, stats
