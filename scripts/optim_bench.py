#!/usr/bin/env python3
"""What a device optimizer costs, with HIP events after warm-up, the candidates alternated window by window in one process.

  python scripts/optim_bench.py --launches   # the update launches alone on flat buffers of two sizes -- the n_params of
                                             # gcnx.GCN(hidden 64) and of the default GeneralGNN (F_in 16): gcnx_sgd,
                                             # gcnx_counter_add + gcnx_adam, + gcnx_grad_sqnorm in front, gcnx_sgd_momentum
  python scripts/optim_bench.py --shape ref  # the gcnx.GCN train_step with plain SGD, gcnx.Adam() and gcnx.Adam(clipnorm=1)
  python scripts/optim_bench.py --shape ecoli

Prints one JSON line.  Every figure is the median over --rounds windows with the windows' min and max beside it (the
run-to-run spread inside this process).  The step lines also carry ``expected_ms`` = the SGD step + the stand-alone time of
the launches the optimizer adds (with --launches figures measured in the same process) and ``excess_ms`` beside it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gcn-string_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import gcnx  # noqa: E402
from gcnx import device as D  # noqa: E402
from gcn_bn_bench import host_batch  # noqa: E402
from sage_bench import alternate, device_batch, stats  # noqa: E402


def model_sizes(ctx):
    gcn = gcnx.GCN(ctx, hidden_channels=64, seed=0)
    gcn.build(16)
    gnn = gcnx.GeneralGNN(ctx, 2, activation="softmax")
    gnn.build(16)
    return {"gcnx.GCN(hidden 64)": int(gcn.n_params), "GeneralGNN (default)": int(gnn.n_params)}


def launch_candidates(ctx, n):
    rng = np.random.default_rng(0)
    dev = lambda scale=1.0: ctx.to_device((scale * rng.standard_normal(n)).astype(np.float32))
    p, g, m, v, vel = dev(), dev(1e-3), ctx.zeros(n), ctx.zeros(n), ctx.zeros(n)
    t, part, norm = ctx.zeros(1, np.int32), ctx.zeros(256), ctx.zeros(1)
    lr = 1e-6                                                    # (thousands of calls on one gradient: the values stay finite)

    def adam():
        D.counter_add(ctx, t, 1)
        D.adam(ctx, p, g, m, v, t, lr)

    def adam_clip():
        D.counter_add(ctx, t, 1)
        k = D.grad_sqnorm(ctx, g, part)
        D.adam(ctx, p, g, m, v, t, lr, partials=part, n_partials=k, clipnorm=1.0, norm_out=norm)

    return {"sgd": lambda: D.sgd(ctx, p, g, lr), "counter_add": lambda: D.counter_add(ctx, t, 1), "counter+adam": adam,
            "counter+sqnorm+adam": adam_clip,
            "counter+sgd_momentum": lambda: (D.counter_add(ctx, t, 1), D.sgd_momentum(ctx, p, g, vel, lr, momentum=0.9))}


def bench_launches(ctx, args):
    cases = []
    for name, n in model_sizes(ctx).items():
        ms = alternate(ctx, launch_candidates(ctx, n), args.steps, args.rounds, args.warmup)
        cases.append({"size_of": name, "n_params": n, **{k: stats(v) for k, v in ms.items()}})
    return {"bench": "optimizer launches", "calls_per_window": args.steps, "rounds": args.rounds, "cases": cases}


def bench_step(ctx, args):
    hb = host_batch(args.shape)
    batch = device_batch(ctx, hb)
    models = {"sgd": gcnx.GCN(ctx, hidden_channels=64, seed=0), "adam": gcnx.GCN(ctx, hidden_channels=64, seed=0),
              "adam_clipnorm": gcnx.GCN(ctx, hidden_channels=64, seed=0)}
    models["adam"].set_optimizer(gcnx.Adam())
    models["adam_clipnorm"].set_optimizer(gcnx.Adam(clipnorm=1.0))
    fns = {k: (lambda m=m: m.train_step(batch, lr=1e-3, fetch=False)) for k, m in models.items()}
    ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
    n = int(models["sgd"].n_params)
    alone = alternate(ctx, launch_candidates(ctx, n), args.steps, args.rounds, args.warmup)
    med = lambda x: float(np.median(x))
    sgd_step, sgd_alone = med(ms["sgd"]), med(alone["sgd"])
    out = {"model": "gcnx.GCN", "shape": args.shape, "n_nodes": int(hb.n), "n_graphs": int(hb.n_graphs), "n_params": n,
           "steps_per_window": args.steps, "rounds": args.rounds, "train_step": {k: stats(v) for k, v in ms.items()},
           "launches_alone": {k: stats(v) for k, v in alone.items()}}
    for k, added in (("adam", "counter+adam"), ("adam_clipnorm", "counter+sqnorm+adam")):
        expected = sgd_step - sgd_alone + med(alone[added])
        out["train_step"][k]["expected_ms"] = round(expected, 5)
        out["train_step"][k]["excess_ms"] = round(med(ms[k]) - expected, 5)
    out["window_spread_ms"] = round(max(max(v) - min(v) for v in ms.values()), 5)
    out["finite"] = bool(all(np.isfinite(m.fetch_metrics(hb.n_graphs)[0]) for m in models.values()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("ref", "ecoli"), default="ref")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--steps", type=int, default=200, help="steps (calls) per timed window")
    ap.add_argument("--rounds", type=int, default=7, help="windows per candidate")
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    ctx = gcnx.Context(0)
    print(json.dumps(bench_launches(ctx, args) if args.launches else bench_step(ctx, args)))
    ctx.close()


if __name__ == "__main__":
    main()
