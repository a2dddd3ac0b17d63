"""NumPy fp64 restatements of the optimizer formulas of include/gcnx.h (gcnx_adam, gcnx_sgd_momentum, gcnx_grad_sqnorm).

Inputs are the fp32 arrays the device holds; beta1, beta2, eps, lr, weight_decay, momentum and clipnorm are rounded to fp32
first, as the C ABI receives them; everything after that is fp64.  Besides the new state each function returns the
magnitudes the derived error bounds of tests/test_gpu_optim.py are written in."""
import numpy as np

U = 2.0 ** -24                      # unit roundoff of fp32 (round to nearest)


def f32(x):
    return float(np.float32(x))


def grad_norm(g):
    """sqrt of the fp64 sum of the fp32 squares g[i] * g[i] (each square rounded to fp32, as the device forms them)."""
    g = np.asarray(g, np.float32).ravel()
    return float(np.sqrt(np.sum((g * g).astype(np.float64))))


def clip_factor(norm, clipnorm):
    """torch.nn.utils.clip_grad_norm_: min(1, clipnorm / (norm + 1e-6)); 1 without clipnorm."""
    if clipnorm is None or not clipnorm > 0:
        return 1.0
    return min(1.0, f32(clipnorm) / (float(norm) + 1e-6))


def adam(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, clipnorm=None, norm=None):
    """One step of torch's Adam / AdamW form.  norm: the gradient norm the clip factor is taken from (default: grad_norm(g)).
    Returns (p, m, v, info); info: s, g' = s g, the Adam term "update", what the step subtracts as "decay" + "update",
    and the two summands of m and v in absolute value ("m_terms", "v_terms")."""
    p, g, m, v = (np.asarray(a, np.float32).astype(np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(weight_decay)
    s = clip_factor(grad_norm(g) if norm is None else norm, clipnorm)
    gs = s * g
    decay = lr * wd * p
    m1 = b1 * m + (1.0 - b1) * gs
    v1 = b2 * v + (1.0 - b2) * gs * gs
    bc1, bc2 = 1.0 - b1 ** int(t), 1.0 - b2 ** int(t)
    update = (lr / bc1) * m1 / (np.sqrt(v1) / np.sqrt(bc2) + eps)
    info = {"s": s, "gs": gs, "decay": decay, "update": update,
            "m_terms": np.abs(b1 * m) + np.abs((1.0 - b1) * gs), "v_terms": np.abs(b2 * v) + np.abs((1.0 - b2) * gs * gs)}
    return p - decay - update, m1, v1, info


def sgd_momentum(p, g, vel, lr, momentum=0.0, nesterov=False, clipnorm=None, norm=None):
    """One step of tf.keras.optimizers.SGD(momentum, nesterov).  Returns (p, vel, info)."""
    p, g, vel = (np.asarray(a, np.float32).astype(np.float64) for a in (p, g, vel))
    lr, mom = f32(lr), f32(momentum)
    s = clip_factor(grad_norm(g) if norm is None else norm, clipnorm)
    gs = s * g
    vel1 = mom * vel - lr * gs
    p1 = p + (mom * vel1 - lr * gs if nesterov else vel1)
    return p1, vel1, {"s": s, "gs": gs, "lr_g": lr * gs}


def norm_chain(n, n_partials):
    """Longest addition chain of the device norm: a thread's ceil(n / (256 n_partials)) squares, six lane steps
    and three wave sums in gcnx_grad_sqnorm, six lane steps and three wave sums over the partials in the update launch."""
    return -(-int(n) // (256 * int(n_partials))) + 9 + 9
