#!/usr/bin/env python3
"""gcnx.GAT train_step and the GATConv launches (csrc/gat.hip) timed with HIP events after warm-up.

  python scripts/gat_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/gat_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/gat_bench.py --kernel         # every new launch alone at width 64 on both batch shapes, heads 1 and 4, next to
                                               # gcnx_spmm_csr on the same pattern and width: the same gather without the
                                               # softmax, i.e. the floor of gcnx_gat_aggregate and gcnx_gat_bwd_nodes

The step is timed for heads 1 and 4, alternated window by window with a gcnx.GCN step in the SAME process.  Prints one JSON
line.  Every figure is the median over --rounds windows with the windows' min and max beside it (the run-to-run spread inside
this process)."""
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
from gcnx.device import DeviceCSR  # noqa: E402
from gcn_bn_bench import host_batch  # noqa: E402
from sage_bench import alternate, device_batch, stats  # noqa: E402


def bench_step(ctx, args):
    hb = host_batch(args.shape)
    batch = device_batch(ctx, hb)
    models = {"gat_heads1": gcnx.GAT(ctx, hidden_channels=64, heads=1, seed=0), "gat_heads4": gcnx.GAT(ctx, hidden_channels=64, heads=4, seed=0),
              "gcn": gcnx.GCN(ctx, hidden_channels=64, seed=0)}
    ms = alternate(ctx, {k: (lambda m=m: m.train_step(batch, lr=1e-3, fetch=False)) for k, m in models.items()},
                   args.steps, args.rounds, args.warmup)
    loss = {k: m.fetch_metrics(hb.n_graphs)[0] for k, m in models.items()}
    return {"model": "gcnx.GAT", "shape": args.shape, "n_nodes": int(hb.n), "nnz": int(hb.nnz), "n_graphs": int(hb.n_graphs), "f_in": 16,
            "hidden": 64, "steps_per_window": args.steps, "rounds": args.rounds, "train_step": {k: stats(v) for k, v in ms.items()},
            "graphs_per_s": {k: round(hb.n_graphs / float(np.median(v)) * 1e3, 1) for k, v in ms.items()},
            "finite": bool(all(np.isfinite(v) for v in loss.values()))}


def bench_kernel(ctx, args):
    res = []
    hc = 64
    for shape in ("ref", "ecoli"):
        hb = host_batch(shape)
        a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr).unweighted()
        a.transpose_perm()
        n, nnz = hb.n, hb.nnz
        rng = np.random.default_rng(0)
        dev = lambda *s: ctx.to_device(rng.standard_normal(s).astype(np.float32))
        hf, dout, bias, floor_out = dev(n, hc), dev(n, hc), dev(hc), ctx.empty((n, hc))
        for heads in (1, 4):
            c = hc // heads
            att_src, att_dst = (ctx.to_device((rng.standard_normal((heads, c)) / np.sqrt(c)).astype(np.float32)) for _ in range(2))
            asrc, adst, dadst, dasrc = (ctx.empty((n, heads)) for _ in range(4))
            alpha, dz = ctx.empty((nnz, heads)), ctx.empty((nnz, heads))
            out, o, dhf = ctx.empty((n, hc)), ctx.empty((n, hc)), ctx.empty((n, hc))
            das, dad = ctx.empty((heads, c)), ctx.empty((heads, c))
            scratch = ctx.empty(max(D.gat_bwd_scratch_floats(ctx, n, heads, c), 1))
            fns = {"gat_scores": lambda: D.gat_scores(ctx, hf, att_src, att_dst, asrc, adst),
                   "gat_aggregate": lambda: D.gat_aggregate(ctx, a, hf, asrc, adst, bias, out, alpha=alpha, o_pre=o),
                   "gat_aggregate_out_only": lambda: D.gat_aggregate(ctx, a, hf, asrc, adst, bias, out),
                   "gat_bwd_edges": lambda: D.gat_bwd_edges(ctx, a, hf, asrc, adst, alpha, dout, o, dz, dadst),
                   "gat_bwd_nodes": lambda: D.gat_bwd_nodes(ctx, a, alpha, dz, dout, hf, dadst, att_src, att_dst, dhf, dasrc, das, dad, scratch),
                   "spmm_csr_floor": lambda: D.spmm(ctx, a, hf, None, floor_out)}
            for fn in list(fns.values())[:4]:               # every launch reads what the one before it wrote
                fn()
            ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            res.append({"shape": shape, "n_nodes": int(n), "nnz": int(nnz), "width": hc, "heads": heads,
                        **{k: stats(v) for k, v in ms.items()},
                        "aggregate_over_floor": round(med["gat_aggregate"] / med["spmm_csr_floor"], 3),
                        "bwd_nodes_over_floor": round(med["gat_bwd_nodes"] / med["spmm_csr_floor"], 3)})
    return {"kernel": "gcnx_gat_*", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


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
