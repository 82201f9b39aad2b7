"""The three contrast entry points (ops.contrast_stage, contrast_stage_variant, contrast_stage_cm) apply one set of input
checks and one choice of backward route.

Inputs: a non-contiguous `a`, a posmask of shape (m, k + 1) and anchors of the wrong dtype raise before any launch.
Route: features whose rows are not 16-byte aligned cannot feed the reverse-list gather; with a contrast_csr plan default mode
takes the float atomics (gradient within the bound tests/test_gpu_contrast_fp64.py applies to the atomic route: per row
4 * rho32 * A_n against fp64), deterministic mode raises."""
import pytest
import torch

import test_gpu_contrast_fp64 as tf
from amcontrast3d_amd.timing import count_calls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, K, C = 64, 5, 16
PRM = tf.PARAMS[0]
FORM = ("adaptive", "-m", "Method1", PRM[2])  # the default form, so that one fp64 reference serves both entries


@pytest.fixture(scope="module")
def case():
    G = tf._small_graph(M, K, 5, B=2)
    f = torch.randn(M, C, generator=torch.Generator().manual_seed(3)).to(DEV)
    return G, f, G.plan()


def _call(ops, entry, f, G, posmask, a, anchors, rev_csr, mutual, rev_m):
    if entry == "stage":
        return ops.contrast_stage(f, G.nidx, posmask, a, *PRM, anchors, rev_csr)
    if entry == "variant":
        return ops.contrast_stage_variant(f, G.nidx, posmask, a, *FORM[:3], PRM[0], PRM[1], FORM[3], anchors, rev_csr)
    f_cm = f.view(G.B, M // G.B, C).transpose(1, 2).contiguous()
    return ops.contrast_stage_cm(f_cm, G.nidx, posmask, a, *PRM, anchors, rev_m, mutual)


@pytest.mark.parametrize("entry", ["stage", "variant", "cm"])
def test_bad_inputs_raise_before_any_launch(case, entry):
    from amcontrast3d_amd import ops
    G, f, (anchors, rev_csr, mutual, rev_m) = case
    strided_a = torch.stack([G.a, G.a], 1)[:, 0]
    assert not strided_a.is_contiguous() and torch.equal(strided_a, G.a)
    wide_mask = torch.cat([G.posmask, G.posmask[:, :1]], 1).contiguous()
    bad = {"a": dict(a=strided_a), "posmask": dict(posmask=wide_mask), "anchors": dict(anchors=anchors.long())}
    for what, change in bad.items():
        args = dict(posmask=G.posmask, a=G.a, anchors=anchors)
        args.update(change)
        with count_calls() as c, pytest.raises((AssertionError, RuntimeError)):
            _call(ops, entry, f, G, args["posmask"], args["a"], args["anchors"], rev_csr, mutual, rev_m)
        assert not dict(c), (entry, what, dict(c))
    _call(ops, entry, f, G, G.posmask, G.a, anchors, rev_csr, mutual, rev_m)  # (the unchanged inputs pass)


def _misaligned(f):
    flat = torch.randn(M * C + 1, device=DEV)
    flat[1:] = f.flatten()
    g = flat[1:].view(M, C)
    assert g.is_contiguous() and g.data_ptr() % 16 == 4 and torch.equal(g, f)
    return g


def test_misaligned_rows_take_the_atomics_in_default_mode_and_raise_in_deterministic_mode(case):
    from amcontrast3d_amd import ops
    G, f, plan = case
    ref = tf.Ref(f, G, G.a, G.posmask, PRM)
    for entry, gather, atomic in (("stage", "contrast_backward_csr", "contrast_backward"),
                                  ("variant", "contrast_variant_backward_csr", "contrast_variant_backward")):
        grads = {}
        for name, rows in (("aligned", f.clone()), ("misaligned", _misaligned(f))):
            rows.requires_grad_(True)
            with count_calls() as c:
                loss = _call(ops, entry, rows, G, G.posmask, G.a, *plan)
                (loss * tf.GRAD_OUT).backward()
            c = dict(c)
            want, other = (gather, atomic) if name == "aligned" else (atomic, gather)
            assert c.get(want, 0) == 1 and c.get(other, 0) == 0, (entry, name, c)
            grads[name] = (loss.detach(), rows.grad)
        for name, (loss, grad) in grads.items():
            ref.check(f"inputs entry={entry} {name} rows", loss, grad)
        with ops.deterministic_mode():
            rows = _misaligned(f).requires_grad_(True)
            loss = _call(ops, entry, rows, G, G.posmask, G.a, *plan)
            with pytest.raises(RuntimeError, match=r"no deterministic route .*16-byte aligned rows"):
                loss.backward()
