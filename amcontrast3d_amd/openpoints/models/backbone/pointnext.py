"""The plain PointNeXt encoder / decoder: the baseline AMContrast3D is compared against.

Drop-in for openpoints/models/backbone/pointnext.py: same registered class names, constructor keywords, attribute
names and module nesting (hence state-dict keys -- which are also those of the _AMContrast3D classes):

    PointNextEncoder    pointnext.py:310-458
    PointNextDecoder    :461-498

The modules are those of pointnext_AA.py (the reference's two files define the same blocks twice); what differs is the
forward: (p, f) lists only, no stageACE_list and no per-stage rows for a contrastive loss.  The coordinate-only half
(``'_geometry'`` in the batch dict, amcontrast3d_amd/geometry.py) is consumed as there and built in line when absent.
"""
from ..build import MODELS
from .pointnext_AA import PointNextDecoder_AMContrast3D, PointNextEncoder_AMContrast3D


@MODELS.register_module()
class PointNextEncoder(PointNextEncoder_AMContrast3D):
    def forward_seg_feat(self, p0, f0=None, geometry=None):
        """-> p[6], f[6] (pointnext.py:443-455).  `geometry`: the plan's 'encoder' entry, when p0 is not a batch dict
        that carries one."""
        if hasattr(p0, 'keys'):
            if geometry is None and p0.get('_geometry', None) is not None:
                geometry = p0['_geometry']['encoder']
            p0, f0 = p0['pos'], p0.get('x', None)
        if f0 is None:
            f0 = p0.clone().transpose(1, 2).contiguous()
        if geometry is None:
            geometry = self.plan_geometry(p0)
        p, f = [p0], [f0]
        for stage, plans in zip(self.encoder, geometry):
            pf = [p[-1], f[-1]]
            for blk, g in zip(stage, plans):
                pf = blk(pf, geom=g)
            p.append(pf[0])
            f.append(pf[1])
        return p, f

    def forward(self, p0, f0=None):
        return self.forward_seg_feat(p0, f0)


@MODELS.register_module()
class PointNextDecoder(PointNextDecoder_AMContrast3D):
    def forward(self, p, f, geometry=None):
        """-> the finest level's features (pointnext.py:494-498).  `geometry`: the plan's 'decoder' entry."""
        if geometry is None:
            geometry = self.plan_geometry(p)
        for i in range(-1, -len(self.decoder) - 1, -1):
            f[i - 1] = self.decoder[i][1:](
                [p[i], self.decoder[i][0]([p[i - 1], f[i - 1]], [p[i], f[i]], geom=geometry[i])])[1]
        return f[-len(self.decoder) - 1]
