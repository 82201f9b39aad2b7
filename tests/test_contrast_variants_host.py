"""The 54 forms of the contrast loss (margin constant / adaptive / learned x db -m / +m / none x Method1 / Method2 x temperature
None / 0.3 / 0.07): the fp64 restatement in tests/contrast_variants_ref.py -- the arbiter of tests/test_gpu_contrast_variants.py --
equals ContrastHead.contrast_softnn_margin, the code the CPU path runs, on CPU tensors to 1e-12.  No GPU, no kernel: this pins
the yardstick, it does not test the feature."""
import types

import pytest
import torch

from contrast_variants_ref import DEFAULT_FORM, FORMS, MU, NU, form_id, form_loss


def _head():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.AMContrast3D.MarginContrast import ContrastHead
    return ContrastHead()


def _inputs():
    g = torch.Generator().manual_seed(3)
    n, k = 331, 24
    sim = torch.rand(n, k, generator=g, dtype=torch.float64) * 2 - 1
    sim[0], sim[1, :5] = 1.0, -1.0
    posmask = torch.rand(n, k, generator=g) < 0.5
    posmask[:7], posmask[7:13] = True, False       # anchors whose neighbours are all positive / that have no positive neighbour
    a = torch.rand(n, generator=g, dtype=torch.float64).clamp_min(1e-30)
    a[2], a[8] = 1.0, 1e-30
    return sim, posmask, a


def test_the_form_list():
    assert len(FORMS) == len(set(FORMS)) == 54 and DEFAULT_FORM in FORMS


@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_restatement_equals_the_heads_loss_at_fp64(form):
    sim, posmask, a = _inputs()
    margin, db, method, T = form
    args = types.SimpleNamespace(margin=margin, db=db, supervisedCL=method, temperature=T, mu=MU, nu=NU)
    want = _head().contrast_softnn_margin(sim, posmask, a, args)
    got = form_loss(sim, posmask, a, form)
    assert want.dtype == torch.float64 and want.shape == got.shape == (331,)
    assert bool(torch.isfinite(want).all()), "finite also without a positive neighbour and with positives only"
    assert float((got - want).abs().max()) <= 1e-12
