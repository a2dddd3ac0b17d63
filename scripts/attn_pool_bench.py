#!/usr/bin/env python3
"""gcnx.GCN(readout="attention") train_step and the readout's launches (csrc/attn_pool.hip) timed with HIP events after warm-up.

  python scripts/attn_pool_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/attn_pool_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/attn_pool_bench.py --kernel         # gcnx_attn_pool on its whole and sliced routes and gcnx_attn_pool_bwd alone at
                                                     # width 64 on both batch shapes, next to gcnx_segment_pool(SUM) and
                                                     # gcnx_segment_pool_bwd on the same rows: the same pass without the
                                                     # softmax, i.e. the floor

The step is alternated window by window with a gcnx.GCN() step (the fused max-pool) in the SAME process.  Prints one JSON line.
Every figure is the median over --rounds windows with the windows' min and max beside it."""
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


def bench_step(ctx, args):
    hb = host_batch(args.shape)
    batch = device_batch(ctx, hb)
    models = {"gcn_attention": gcnx.GCN(ctx, hidden_channels=64, seed=0, readout="attention"), "gcn": gcnx.GCN(ctx, hidden_channels=64, seed=0)}
    ms = alternate(ctx, {k: (lambda m=m: m.train_step(batch, lr=1e-3, fetch=False)) for k, m in models.items()},
                   args.steps, args.rounds, args.warmup)
    loss = {k: m.fetch_metrics(hb.n_graphs)[0] for k, m in models.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"model": "gcnx.GCN(readout='attention')", "shape": args.shape, "n_nodes": int(hb.n), "nnz": int(hb.nnz),
            "n_graphs": int(hb.n_graphs), "f_in": 16, "hidden": 64, "steps_per_window": args.steps, "rounds": args.rounds,
            "train_step": {k: stats(v) for k, v in ms.items()}, "attention_over_max": round(med["gcn_attention"] / med["gcn"], 3),
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
        x, dp, a = dev(n, f), dev(b, f), ctx.to_device((rng.standard_normal(f) / np.sqrt(f)).astype(np.float32))
        pooled, alpha, dx, da = ctx.empty((b, f)), ctx.empty(n), ctx.empty((n, f)), ctx.empty(f)
        floor_p, floor_dx = ctx.empty((b, f)), ctx.empty((n, f))
        slice_rows = 64
        scratch = ctx.empty(max(D.attn_pool_scratch_floats(ctx, n, b, f, slice_rows), 4))
        fns = {"attn_pool_whole": lambda: D.attn_pool(ctx, seg, x, a, pooled, alpha),
               "attn_pool_sliced": lambda: D.attn_pool(ctx, seg, x, a, pooled, alpha, scratch, slice_rows),
               "attn_pool_auto": lambda: D.attn_pool(ctx, seg, x, a, pooled, alpha, scratch),
               "attn_pool_bwd": lambda: D.attn_pool_bwd(ctx, seg, x, a, alpha, pooled, dp, dx, da, scratch),
               "segment_pool_sum_floor": lambda: D.segment_pool(ctx, seg, x, floor_p, "sum"),
               "segment_pool_bwd_floor": lambda: D.segment_pool_bwd(ctx, seg, dp, floor_dx, "sum")}
        fns["attn_pool_whole"]()                                # the backward reads what a forward wrote
        ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res.append({"shape": shape, "n_nodes": int(n), "n_graphs": int(b), "width": f, "slice_rows": slice_rows,
                    **{k: stats(v) for k, v in ms.items()},
                    "whole_over_floor": round(med["attn_pool_whole"] / med["segment_pool_sum_floor"], 3),
                    "sliced_over_floor": round(med["attn_pool_sliced"] / med["segment_pool_sum_floor"], 3),
                    "bwd_over_floor": round(med["attn_pool_bwd"] / med["segment_pool_bwd_floor"], 3)})
    return {"kernel": "gcnx_attn_pool*", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


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
