"""Deterministic mode on the host: the flag's set / restore / nesting semantics, and the rule that a Function honours in
backward the mode it was built under (autograd runs backward outside the `with` block of forward)."""
import pytest
import torch


def _ops():
    from amcontrast3d_amd import ops
    return ops


def test_flag_set_restore_and_nesting():
    ops = _ops()
    ops.set_deterministic(False)
    assert ops.deterministic() is False
    ops.set_deterministic(1)
    assert ops.deterministic() is True
    ops.set_deterministic(False)
    with ops.deterministic_mode():
        assert ops.deterministic()
        with ops.deterministic_mode(False):
            assert not ops.deterministic()
            with ops.deterministic_mode(True):
                assert ops.deterministic()
            assert not ops.deterministic()
        assert ops.deterministic()
        ops.set_deterministic(False)  # set inside a block: the block still restores what it found
    assert ops.deterministic() is False
    ops.set_deterministic(True)
    with ops.deterministic_mode(False):
        assert not ops.deterministic()
    assert ops.deterministic() is True
    ops.set_deterministic(False)
    with pytest.raises(ValueError):
        with ops.deterministic_mode():
            raise ValueError("leaves through an exception")
    assert ops.deterministic() is False


def test_a_function_honours_in_backward_the_mode_of_its_forward():
    ops = _ops()
    ops.set_deterministic(False)
    seen = []

    class Stub(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.det = ops.deterministic()
            return x * 2

        @staticmethod
        def backward(ctx, g):
            seen.append((ctx.det, ops.deterministic()))
            return g * 2

    x = torch.ones(3, requires_grad=True)
    with ops.deterministic_mode():
        y = Stub.apply(x)
    y.sum().backward()                 # outside the block
    z = Stub.apply(x)
    with ops.deterministic_mode():
        z.sum().backward()             # inside a block, built outside
    assert seen == [(True, False), (False, True)]


def test_no_route_errors_name_the_operator_and_need_no_gpu():
    ops = _ops()
    ops.set_deterministic(False)
    err = ops._no_route("group_points_grad", "why")
    assert isinstance(err, RuntimeError) and str(err).startswith("group_points_grad: no deterministic route")
    # the product's Functions read the record, not the current mode: GroupedConv refuses in backward what was built under it
    class Ctx:
        det = True
        saved_tensors = (None, None, None, None)
    with pytest.raises(RuntimeError, match="grouped_conv_backward: no deterministic route"):
        ops.GroupedConv.backward(Ctx(), torch.zeros(1, 1, 1, 1))


def test_train_loops_key_their_pipeline_cache_by_the_mode():
    ops = _ops()
    ops.set_deterministic(False)
    import inspect
    from amcontrast3d_amd import train
    src = inspect.getsource(train._graph_pipeline)
    assert "ops.deterministic()" in src.split("hit = _PIPELINES.get(key)")[0]
    assert "deterministic_mode" in inspect.getsource(train._run_epoch)
