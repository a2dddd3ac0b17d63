"""Host tests of the optimizers: the fp64 restatement tests/optim_ref.py against closed forms and against torch.optim (in a
child process, as test_dist_cpu.py runs torch), the optimizers' host-side state_dict, and the lazy import of libgcnx."""
import subprocess
import sys
import textwrap

import numpy as np

from conftest import ROOT
import optim_ref as OR


def _state(n=257, seed=0):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-4, 2, n)).astype(np.float32)
    return rng, p, g


def test_adam_first_step_moves_by_lr_sign_g():
    _, p, g = _state()
    z = np.zeros_like(p)
    lr = 1e-3
    p1, m1, v1, _ = OR.adam(p, g, z, z, 1, lr)
    # m / (1 - b1) = g and v / (1 - b2) = g^2 at t = 1: the step is lr g / (|g| + eps), eps / |g| <= 1e-4 here
    step = p.astype(np.float64) - p1
    assert np.allclose(step, OR.f32(lr) * np.sign(g), rtol=2e-4, atol=0)
    assert np.allclose(m1, (1 - OR.f32(0.9)) * g.astype(np.float64), rtol=1e-15)
    assert np.allclose(v1, (1 - OR.f32(0.999)) * g.astype(np.float64) ** 2, rtol=1e-15)


def test_weight_decay_alone_shrinks_p():
    _, p, _ = _state(seed=1)
    z = np.zeros_like(p)
    lr, wd = 1e-2, 0.1
    p1, m1, v1, info = OR.adam(p, z, z, z, 3, lr, weight_decay=wd)
    assert np.array_equal(m1, z) and np.array_equal(v1, z) and not info["update"].any()
    assert np.allclose(p1, p.astype(np.float64) * (1 - OR.f32(lr) * OR.f32(wd)), rtol=1e-15, atol=0)


def test_momentum_zero_is_plain_sgd():
    rng, p, g = _state(seed=2)
    vel = rng.standard_normal(p.size).astype(np.float32)
    for nesterov in (False, True):
        p1, vel1, _ = OR.sgd_momentum(p, g, vel, 0.02, momentum=0.0, nesterov=nesterov)
        want = p.astype(np.float64) - OR.f32(0.02) * g.astype(np.float64)
        assert np.array_equal(p1, want) and np.array_equal(vel1, -OR.f32(0.02) * g.astype(np.float64))


def test_momentum_accumulates_a_constant_gradient():
    p, g, vel = np.zeros(3, np.float32), np.ones(3, np.float32), np.zeros(3, np.float32)
    mom, lr = OR.f32(0.5), OR.f32(0.25)
    p1, v1, _ = OR.sgd_momentum(p, g, vel, lr, momentum=mom)
    p2, v2, _ = OR.sgd_momentum(p1.astype(np.float32), g, v1.astype(np.float32), lr, momentum=mom)
    assert np.array_equal(v2, np.full(3, -lr * (1 + mom))) and np.array_equal(p2, np.full(3, -lr * (2 + mom)))
    pn, _, _ = OR.sgd_momentum(p, g, vel, lr, momentum=mom, nesterov=True)
    assert np.array_equal(pn, np.full(3, -lr * (1 + mom)))


def test_clipping_leaves_small_gradients_and_scales_large_ones():
    _, _, g = _state(seed=3)
    norm = OR.grad_norm(g)
    assert abs(norm - np.linalg.norm(g.astype(np.float64))) < 1e-6 * norm      # (fp32 squares: 2^-24 each)
    assert OR.clip_factor(norm, 2 * norm) == 1.0 and OR.clip_factor(norm, None) == 1.0
    c = OR.f32(0.25 * norm)
    s = OR.clip_factor(norm, c)
    # the clipped gradient has norm c * norm / (norm + 1e-6): c within 1e-6 / norm and fp64 rounding
    assert abs(s * norm - c) <= c * (1e-6 / norm + 4e-16)
    _, m1, _, info = OR.adam(g, g, np.zeros_like(g), np.zeros_like(g), 1, 1e-3, clipnorm=c)
    assert info["s"] == s and np.allclose(m1, (1 - OR.f32(0.9)) * s * g.astype(np.float64), rtol=1e-15)


def test_norm_chain_counts_the_documented_order():
    assert OR.norm_chain(1, 1) == 1 + 18 and OR.norm_chain(257, 2) == 1 + 18
    assert OR.norm_chain(2048 * 256 + 37, 256) == 9 + 18


TORCH_CHECK = textwrap.dedent("""
    import os, sys
    import numpy as np
    sys.path.insert(0, os.path.join({root!r}, "tests"))
    try:
        import torch
    except Exception as e:                       # no torch on this machine: the closed forms stand alone
        print("NO_TORCH", e); sys.exit(0)
    import optim_ref as OR
    rng = np.random.default_rng(5)
    n, lr = 64, 1e-2
    p0 = rng.standard_normal(n).astype(np.float32)
    gs = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32) for _ in range(3)]
    for wd, clip in ((0.0, None), (0.01, None), (0.0, 0.5), (0.01, 0.5)):
        tp = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
        kw = dict(lr=OR.f32(lr), betas=(OR.f32(0.9), OR.f32(0.999)), eps=OR.f32(1e-8))
        opt = torch.optim.AdamW([tp], weight_decay=OR.f32(wd), **kw) if wd else torch.optim.Adam([tp], **kw)
        p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
        for t, g in enumerate(gs, 1):
            tp.grad = torch.tensor(g, dtype=torch.float64)
            if clip:
                torch.nn.utils.clip_grad_norm_([tp], OR.f32(clip))
            opt.step()
            # (the restatement takes fp32 arrays; p, m, v are carried in fp64 here so that three steps compare at 1e-12)
            g32, g = g, g.astype(np.float64)
            s = OR.clip_factor(float(np.sqrt(np.sum(g ** 2))), clip)
            b1, b2 = OR.f32(0.9), OR.f32(0.999)
            p = p * (1 - OR.f32(lr) * OR.f32(wd))
            m = b1 * m + (1 - b1) * s * g
            v = b2 * v + (1 - b2) * (s * g) ** 2
            p = p - (OR.f32(lr) / (1 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + OR.f32(1e-8))
            assert np.max(np.abs(tp.detach().numpy() - p)) < 1e-12, (wd, clip, t)
            if t == 1:                            # one step from fp32 state: optim_ref.adam itself
                p1, m1, v1, _ = OR.adam(p0, g32, np.zeros(n, np.float32), np.zeros(n, np.float32), 1, lr, weight_decay=wd, clipnorm=clip,
                                        norm=float(np.sqrt(np.sum(g ** 2))))
                assert np.max(np.abs(p1 - p)) < 1e-12 and np.max(np.abs(m1 - m)) < 1e-12 and np.max(np.abs(v1 - v)) < 1e-12
    print("TORCH_OK")
""")


def test_restatement_matches_torch_adam_adamw_and_clip(tmp_path):
    script = tmp_path / "torch_check.py"
    script.write_text(TORCH_CHECK.format(root=ROOT))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TORCH_OK" in r.stdout or "NO_TORCH" in r.stdout, r.stdout + r.stderr


def test_state_dict_round_trip_on_the_host():
    import gcnx
    opt = gcnx.Adam(weight_decay=0.01, clipnorm=1.0)
    d = opt.state_dict()
    assert d["t"] == 0 and d["m"].shape == (0,) and d["v"].shape == (0,)
    rng = np.random.default_rng(0)
    saved = {"t": 7, "m": rng.standard_normal((5, 4)).astype(np.float32), "v": rng.random(20).astype(np.float32)}
    opt.load_state_dict(saved)
    back = opt.state_dict()
    assert back["t"] == 7 and back["m"].shape == (20,) and back["v"].shape == (20,) and back["m"].dtype == np.float32
    assert np.array_equal(back["m"], saved["m"].ravel()) and np.array_equal(back["v"], saved["v"])
    sgd = gcnx.SGD(momentum=0.9)
    sgd.load_state_dict({"t": 2, "vel": np.ones(3)})
    assert sgd.state_dict()["vel"].shape == (3,) and set(gcnx.SGD().state_dict()) == {"t"}
    for bad in (lambda: gcnx.Adam(beta1=1.0), lambda: gcnx.SGD(momentum=-0.1), lambda: gcnx.Adam(clipnorm=0.0)):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("a bad hyper-parameter was accepted")
    try:
        opt.load_state_dict({"t": 1, "m": saved["m"]})
    except KeyError:
        pass
    else:
        raise AssertionError("a state_dict without v was accepted")


def test_host_import_of_the_optimizers_does_not_load_the_library():
    code = ("import sys; sys.path.insert(0, %r); import gcnx; gcnx.Adam(); gcnx.SGD(momentum=0.9, nesterov=True, clipnorm=1.0); "
            "from gcnx import _lib; assert _lib._lib is None and 'gcnx.device' not in sys.modules; print('LAZY_OK')"
            % (ROOT + "/gcn-string_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "LAZY_OK" in r.stdout, r.stdout + r.stderr
