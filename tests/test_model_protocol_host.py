"""The public surface the four models share (gcnx/models.py, _GraphRunner) and the layout of their flat parameter buffers,
pinned without a device: signatures as the callers of train_step / loss_and_grads use them positionally, the edge-feature
attribute gcnx.fit / gcnx.evaluate read, and every offset of GCN2's packed and GCN's 4-float-aligned buffer."""
import inspect

import pytest

from gcnx.models import ECCNet, GCN, GCN2, GeneralGNN

_CALL = "(self, inputs, training=False)"
_EVAL = "(self, inputs, target)"
_STEP = "(self, inputs, target=None, lr=0.02, fetch=True, global_batch=None)"
_GRADS = "(self, inputs, target=None, global_batch=None, _lr=None)"
SIGNATURES = {
    GCN2: {"__call__": _CALL, "loss_and_grads": "(self, inputs, target, global_batch=None, _lr=None)",
           "train_step": "(self, inputs, target=None, lr=0.02, global_batch=None, fetch=True)", "fetch_metrics": "(self, n_graphs)",
           "evaluate_batch": _EVAL, "get_weights": "(self)", "set_weights": "(self, weights)", "build": "(self, f_in)"},
    GeneralGNN: {"__call__": _CALL, "loss_and_grads": "(self, inputs, target=None, _lr=None, global_batch=None)",
                 "train_step": _STEP, "fetch_metrics": "(self, n_graphs)", "evaluate_batch": _EVAL,
                 "get_weights": "(self, order='keras')", "set_weights": "(self, weights, order='keras')", "build": "(self, f_in)"},
    GCN: {"__call__": _CALL, "loss_and_grads": _GRADS, "train_step": _STEP, "fetch_metrics": "(self, n_graphs)",
          "evaluate_batch": _EVAL, "get_weights": "(self)", "set_weights": "(self, weights)", "build": "(self, f_in)"},
    ECCNet: {"__call__": _CALL, "loss_and_grads": _GRADS, "train_step": _STEP, "fetch_metrics": "(self, n_graphs)",
             "evaluate_batch": _EVAL, "get_weights": "(self, as_dict=False)", "set_weights": "(self, weights)",
             "build": "(self, f_in, edge_dim)"},
}


@pytest.mark.parametrize("cls", list(SIGNATURES), ids=lambda c: c.__name__)
def test_public_signatures_are_the_ones_callers_use_positionally(cls):
    for name, want in SIGNATURES[cls].items():
        assert str(inspect.signature(getattr(cls, name))) == want, (cls.__name__, name)


def test_only_eccnet_reads_edge_features():
    assert [getattr(c, "uses_edge_features", False) for c in (GCN2, GeneralGNN, GCN, ECCNet)] == [False, False, False, True]


class _View:
    def __init__(self, shape):
        self.shape = shape

    def copy_from_host(self, host, wait=True):
        assert host.shape == tuple(self.shape)


class _Buffer:
    def __init__(self, size):
        self.size, self.views = size, []

    def flat(self, off, n, shape=None):
        assert off + n <= self.size
        self.views.append((off, n, shape or (n,)))
        return _View(shape or (n,))


class _RecordingContext:
    """Stands in for gcnx.Context in build(): records zeros(n) and every flat(off, n, shape) of what it hands back."""

    def __init__(self):
        self.buffers = []

    def zeros(self, n):
        self.buffers.append(_Buffer(n))
        return self.buffers[-1]


def _check_layout(m, ctx, order, shapes, offsets, n_params):
    assert [b.size for b in ctx.buffers] == [n_params, n_params + 2]
    assert m.flat_p is ctx.buffers[0] and m.flat_g is ctx.buffers[1] and m.n_params == n_params
    want = [(offsets[k], shapes[k][0] * (shapes[k][1] if len(shapes[k]) > 1 else 1), shapes[k]) for k in order]
    assert sorted(m.flat_p.views) == want                             # every parameter, nothing else
    assert sorted(m.flat_g.views) == want + [(n_params, 2, (2,))]     # the same places, then (loss sum, correct count)
    assert set(m.p) == set(m.g) == set(order) and all(m.p[k].shape == shapes[k] == m.g[k].shape for k in order)
    assert m.loss_acc.shape == (2,)


def test_gcn2_flat_buffer_is_packed_in_param_order():
    ctx = _RecordingContext()
    m = GCN2(ctx=ctx, n_labels=2, hidden=3)
    m.build(5)
    shapes = {"w1": (5, 3), "b1": (3,), "w2": (3, 3), "b2": (3,), "w3": (3, 2), "b3": (2,)}
    offsets = {"w1": 0, "b1": 15, "w2": 18, "b2": 27, "w3": 30, "b3": 36}
    _check_layout(m, ctx, GCN2.PARAM_ORDER, shapes, offsets, 38)


def test_gcn_flat_buffer_starts_every_tensor_on_four_floats():
    ctx = _RecordingContext()
    m = GCN(ctx=ctx, hidden_channels=3)
    m.build(5)
    shapes = {"w1": (5, 3), "w2": (3, 3), "w3": (3, 3), "w4": (1, 3)}
    shapes.update({k: (3,) for k in ("b1", "g1", "be1", "b2", "g2", "be2", "b3", "g3", "be3")})
    shapes.update({k: (1,) for k in ("a1", "a2", "a3", "b4", "g4", "be4", "a4")})
    # 15 -> 16, 3 -> 4, 1 -> 4, 9 -> 12 floats per tensor
    offsets = {"w1": 0, "b1": 16, "g1": 20, "be1": 24, "a1": 28, "w2": 32, "b2": 44, "g2": 48, "be2": 52, "a2": 56,
               "w3": 60, "b3": 72, "g3": 76, "be3": 80, "a3": 84, "w4": 88, "b4": 92, "g4": 96, "be4": 100, "a4": 104}
    _check_layout(m, ctx, GCN.PARAM_ORDER, shapes, offsets, 108)
