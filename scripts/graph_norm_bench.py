#!/usr/bin/env python3
"""gcnx.GCN(norm="graph") train_step and GraphNorm's launches (csrc/graph_norm.hip) timed with HIP events after warm-up.

  python scripts/graph_norm_bench.py --shape ref     # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/graph_norm_bench.py --shape ecoli   # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/graph_norm_bench.py --kernel        # gcnx_graph_norm_act on its whole and sliced routes and the library's choice, and
                                                     # gcnx_graph_norm_act_bwd likewise, at width 64 on both batch shapes, next to
                                                     # gcnx_bn_moments + gcnx_bn_act and gcnx_bn_act_bwd on the same rows

The step is alternated window by window with a gcnx.GCN() step (the fused max-pool) and with a gcnx.GCN() step under
GCNX_BN_POOL=0 (the same unfused pool as norm="graph") in the SAME process.  Prints one JSON line.  Every figure is the median
over --rounds windows with the windows' min and max beside it."""
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
from gcnx.device import Segments  # noqa: E402
from gcn_bn_bench import host_batch  # noqa: E402
from sage_bench import alternate, device_batch, stats  # noqa: E402


def _unfused_gcn(ctx):
    """gcnx.GCN() with GCNX_BN_POOL=0 (the knob is read at construction)."""
    old = os.environ.get("GCNX_BN_POOL")
    os.environ["GCNX_BN_POOL"] = "0"
    try:
        return gcnx.GCN(ctx, hidden_channels=64, seed=0)
    finally:
        if old is None:
            del os.environ["GCNX_BN_POOL"]
        else:
            os.environ["GCNX_BN_POOL"] = old


def bench_step(ctx, args):
    hb = host_batch(args.shape)
    batch = device_batch(ctx, hb)
    models = {"gcn_graph_norm": gcnx.GCN(ctx, hidden_channels=64, seed=0, norm="graph"), "gcn": gcnx.GCN(ctx, hidden_channels=64, seed=0),
              "gcn_unfused_pool": _unfused_gcn(ctx)}
    ms = alternate(ctx, {k: (lambda m=m: m.train_step(batch, lr=1e-3, fetch=False)) for k, m in models.items()},
                   args.steps, args.rounds, args.warmup)
    loss = {k: m.fetch_metrics(hb.n_graphs)[0] for k, m in models.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"model": "gcnx.GCN(norm='graph')", "shape": args.shape, "n_nodes": int(hb.n), "nnz": int(hb.nnz),
            "n_graphs": int(hb.n_graphs), "f_in": 16, "hidden": 64, "steps_per_window": args.steps, "rounds": args.rounds,
            "train_step": {k: stats(v) for k, v in ms.items()}, "graph_over_batch": round(med["gcn_graph_norm"] / med["gcn"], 3),
            "graph_over_unfused_batch": round(med["gcn_graph_norm"] / med["gcn_unfused_pool"], 3),
            "finite": bool(all(np.isfinite(v) for v in loss.values()))}


def bench_kernel(ctx, args):
    res = []
    f = 64
    for shape in ("ref", "ecoli"):
        hb = host_batch(shape)
        n, b = hb.n, hb.n_graphs
        seg = Segments(ctx, hb.graph_ptr)
        rng = np.random.default_rng(0)
        dev = lambda *s: ctx.to_device(rng.standard_normal(s).astype(np.float32))
        z, dy = dev(n, f), dev(n, f)
        ms_, gamma, beta = (ctx.to_device(rng.uniform(0.5, 1.5, f).astype(np.float32)) for _ in range(3))
        slope = ctx.to_device(np.array([0.25], np.float32))
        y, dz, mean, inv = ctx.empty((n, f)), ctx.empty((n, f)), ctx.empty((b, f)), ctx.empty((b, f))
        g = [ctx.empty(f) for _ in range(3)] + [ctx.empty(1)]
        bn_mean, bn_inv, bn_y, bn_dz, bn_sums = ctx.empty(f), ctx.empty(f), ctx.empty((n, f)), ctx.empty((n, f)), ctx.empty(3 * f)
        slice_rows = 64
        scratch = ctx.empty(max(D.graph_norm_scratch_floats(ctx, n, b, f, slice_rows), D.graph_norm_scratch_floats(ctx, n, b, f), 4))
        fwd = lambda sc, s: D.graph_norm_act(ctx, seg, z, ms_, gamma, beta, y, mean, inv, act="prelu_shared", alpha=slope, scratch=sc,
                                            slice_rows=s)
        bwd = lambda sc, s: D.graph_norm_act_bwd(ctx, seg, dy, z, mean, inv, ms_, gamma, beta, dz, act="prelu_shared", alpha=slope,
                                                dgamma=g[0], dbeta=g[1], dmean_scale=g[2], dalpha=g[3], scratch=sc, slice_rows=s)

        def bn_fwd():
            D.bn_moments(ctx, z, None, bn_mean, bn_inv, eps=D.TORCH_BN_EPS)
            D.bn_act(ctx, z, bn_mean, bn_inv, gamma, beta, bn_y, act="prelu_shared", alpha=slope)

        fns = {"graph_norm_whole": lambda: fwd(None, 0), "graph_norm_sliced": lambda: fwd(scratch, slice_rows),
               "graph_norm_auto": lambda: fwd(scratch, 0),
               "graph_norm_bwd_whole": lambda: bwd(None, 0), "graph_norm_bwd_sliced": lambda: bwd(scratch, slice_rows),
               "graph_norm_bwd_auto": lambda: bwd(scratch, 0),
               "bn_moments_bn_act": bn_fwd,
               "bn_act_bwd": lambda: D.bn_act_bwd(ctx, dy, z, bn_mean, bn_inv, gamma, beta, bn_dz, bn_sums, act="prelu_shared",
                                                  alpha=slope, dgamma=g[0], dbeta=g[1], dalpha=g[3])}
        fns["graph_norm_whole"]()                               # the backwards read what a forward wrote
        bn_fwd()
        ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res.append({"shape": shape, "n_nodes": int(n), "n_graphs": int(b), "width": f, "slice_rows": slice_rows,
                    **{k: stats(v) for k, v in ms.items()},
                    "whole_over_bn": round(med["graph_norm_whole"] / med["bn_moments_bn_act"], 3),
                    "sliced_over_bn": round(med["graph_norm_sliced"] / med["bn_moments_bn_act"], 3),
                    "bwd_whole_over_bn": round(med["graph_norm_bwd_whole"] / med["bn_act_bwd"], 3),
                    "bwd_sliced_over_bn": round(med["graph_norm_bwd_sliced"] / med["bn_act_bwd"], 3)})
    return {"kernel": "gcnx_graph_norm_act*", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("ref", "ecoli"), default="ref")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--steps", type=int, default=200, help="steps (calls) per timed window")
    ap.add_argument("--rounds", type=int, default=7, help="windows per candidate")
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    ctx = gcnx.Context(0)
    print(json.dumps(bench_kernel(ctx, args) if args.kernel else bench_step(ctx, args)))
    ctx.close()


if __name__ == "__main__":
    main()
