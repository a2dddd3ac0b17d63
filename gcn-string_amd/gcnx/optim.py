"""Optimizers with state on the device: ``Adam`` (torch's Adam / AdamW form) and ``SGD`` (Keras form: momentum, Nesterov), both
with clipping by global norm (torch.nn.utils.clip_grad_norm_).  ``model.set_optimizer(opt)`` -- or ``gcnx.fit(..., optimizer=opt)``
-- puts one behind every model's update; the kernels are csrc/optim.hip.

An optimizer holds no learning rate: the step's ``lr`` argument stays the rate, so ``fit(schedule=...)``,
``PiecewiseConstantDecay`` and the device-scalar rate of a captured step work unchanged.  Its state -- m, v or vel over the
model's flat parameter buffer, the step count t, the norm's partial sums and the norm -- lives on the device and is allocated
when the optimizer meets a built model.  A step is: t += 1 (gcnx_counter_add), the norm's partials if ``clipnorm`` is set
(gcnx_grad_sqnorm), the update (gcnx_adam / gcnx_sgd_momentum / gcnx_sgd): nothing of it is read by the host.

Importing this module does not load libgcnx (host-only use of the package needs no .so)."""
from __future__ import annotations

import numpy as np


class _Optimizer:
    STATE = ()                            # names of the per-parameter state buffers

    def __init__(self, clipnorm=None):
        if clipnorm is not None and not float(clipnorm) > 0.0:
            raise ValueError(f"clipnorm={clipnorm!r}: a positive norm, or None")
        self.clipnorm = None if clipnorm is None else float(clipnorm)
        self._model = None                # the model whose flat buffers the state parallels
        self._pending = None              # a state_dict loaded before the state exists
        self._flat = {}

    # ---- state ---------------------------------------------------------------------------------------------------------
    def bind(self, model):
        """Allocate the state for ``model`` (built): zeros of n_params floats per buffer, t = 0 -- or what load_state_dict left."""
        if self._model is model and self._n == model.n_params and self._p_ptr == model.flat_p.ptr:
            return
        ctx, n = model.ctx, int(model.n_params)
        self._model, self._n, self._p_ptr = model, n, model.flat_p.ptr
        self._flat = {s: ctx.zeros(n) for s in self.STATE}
        self.t = ctx.zeros(1, np.int32)                      # (the bits of a uint32: gcnx_counter_add)
        self._partials = ctx.zeros(256) if self.clipnorm is not None else None
        self._norm = ctx.zeros(1) if self.clipnorm is not None else None
        views = {}
        if isinstance(getattr(model, "p", None), dict):
            views.update(model.p)
        for i, layer in enumerate(getattr(model, "layers", ()) if not views else ()):     # GeneralGNN: "<layer>.<name>"
            views.update({f"{i}.{k[2:]}": layer[k[2:]] for k in layer if k.startswith("g_")})
        for s in self.STATE:
            setattr(self, s, {k: self._flat[s].flat((a.ptr - model.flat_p.ptr) // 4, a.size, a.shape) for k, a in views.items()})
        if self._pending is not None:
            d, self._pending = self._pending, None
            self.load_state_dict(d)

    def _bound(self):
        return self._model is not None

    def flat(self, name):
        """The whole state buffer ``name`` ("m", "v" / "vel"): n_params floats parallel to model.flat_p."""
        return self._flat[name]

    def state_dict(self):
        """{"t": steps taken, state name: the flat buffer as a NumPy array}.  Before the optimizer has met a built model: what
        load_state_dict was given, or t = 0 and empty arrays."""
        if not self._bound():
            if self._pending is not None:
                return {"t": int(self._pending["t"]), **{s: np.array(self._pending[s], np.float32) for s in self.STATE}}
            return {"t": 0, **{s: np.zeros(0, np.float32) for s in self.STATE}}
        return {"t": int(self.t.numpy().view(np.uint32)[0]), **{s: self._flat[s].numpy() for s in self.STATE}}

    def load_state_dict(self, d):
        """Restore a run: the state buffers and a 4-byte upload of t.  Before the state exists the dict is kept and applied when it does."""
        missing = [k for k in ("t",) + tuple(self.STATE) if k not in d]
        if missing:
            raise KeyError(f"{type(self).__name__}.load_state_dict: missing {missing}")
        if not self._bound():
            self._pending = {"t": int(d["t"]), **{s: np.array(d[s], np.float32).ravel() for s in self.STATE}}
            return
        for s in self.STATE:
            a = np.asarray(d[s], np.float32).ravel()
            if a.size != self._n:
                raise ValueError(f"{type(self).__name__}.load_state_dict: {s} has {a.size} elements, the model {self._n} parameters")
            self._flat[s].copy_from_host(a)
        self.t.copy_from_host(np.asarray([int(d["t"])], np.uint32).view(np.int32))

    def last_grad_norm(self):
        """The global gradient norm the last step clipped by (None without clipnorm): one device -> host copy, for logging --
        no step calls it."""
        if not self._bound() or self._norm is None:
            return None
        return float(self._norm.numpy()[0])

    # ---- the step ------------------------------------------------------------------------------------------------------
    def step(self, model, lr):
        """The update launches of one step on model.flat_p / model.flat_g (model._apply_sgd calls this)."""
        from . import device as D
        self.bind(model)
        ctx = model.ctx
        grads = model.flat_g.flat(0, model.n_params)
        D.counter_add(ctx, self.t, 1)
        k = D.grad_sqnorm(ctx, grads, self._partials) if self.clipnorm is not None else 0
        self._update(D, ctx, model.flat_p, grads, lr, k)


class Adam(_Optimizer):
    """torch.optim.Adam; with ``weight_decay`` torch.optim.AdamW (decoupled: p *= 1 - lr * weight_decay).  ``opt.m[key]`` /
    ``opt.v[key]`` are views parallel to ``model.p[key]`` (GeneralGNN: "<layer index>.<name>"), ``opt.flat("m")`` the whole buffer."""

    STATE = ("m", "v")

    def __init__(self, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, clipnorm=None):
        super().__init__(clipnorm)
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError(f"Adam: betas ({beta1}, {beta2}) outside [0, 1)")
        self.beta1, self.beta2, self.eps, self.weight_decay = float(beta1), float(beta2), float(eps), float(weight_decay)
        self.m, self.v = {}, {}

    def _update(self, D, ctx, params, grads, lr, k):
        D.adam(ctx, params, grads, self._flat["m"], self._flat["v"], self.t, lr, self.beta1, self.beta2, self.eps, self.weight_decay,
               partials=self._partials, n_partials=k, clipnorm=self.clipnorm, norm_out=self._norm)


class SGD(_Optimizer):
    """tf.keras.optimizers.SGD(momentum, nesterov) (the reference's optimizer class, gcn.py:325): vel = momentum vel - lr g,
    p += vel (Nesterov: p += momentum vel - lr g).  momentum = 0 without clipnorm is the plain gcnx_sgd launch and keeps no
    velocity; ``opt.vel[key]`` parallels ``model.p[key]`` otherwise."""

    def __init__(self, momentum=0.0, nesterov=False, clipnorm=None):
        super().__init__(clipnorm)
        if not 0.0 <= momentum < 1.0:
            raise ValueError(f"SGD: momentum {momentum} outside [0, 1)")
        self.momentum, self.nesterov = float(momentum), bool(nesterov)
        self.STATE = ("vel",) if (self.momentum > 0.0 or self.clipnorm is not None) else ()
        self.vel = {}

    def _update(self, D, ctx, params, grads, lr, k):
        if not self.STATE:
            D.sgd(ctx, params, grads, lr)
            return
        D.sgd_momentum(ctx, params, grads, self._flat["vel"], lr, self.momentum, self.nesterov, partials=self._partials, n_partials=k,
                       clipnorm=self.clipnorm, norm_out=self._norm)
