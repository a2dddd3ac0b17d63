#!/usr/bin/env python3
"""gcnx.GINE train_step and the GINEConv launches (csrc/gine.hip) timed with HIP events after warm-up.

  python scripts/gine_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/gine_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/gine_bench.py --kernel         # every new launch alone at 16 -> 64 -> 64 and 64 -> 64 -> 64, edge_dim 2, on both batch
                                                # shapes, next to gcnx_gin_conv and gcnx_gin_aggregate on the same pattern and widths:
                                                # the same launches without the edge term, i.e. the floor

The step is timed on both routes (GCNX_GINE_FUSED) with and without train_eps, streamed: every step a fresh batch of the same
graphs from DeviceDisjointLoader(DeviceDataset(edge_features=True)), collate included -- alternated window by window with a
gcnx.GIN, a gcnx.ResGated(edge_dim=2) and a gcnx.GATv2(heads=4, edge_dim=2) step fed by the same loader in the SAME process.
Prints one JSON line.  Every figure is the median over --rounds windows with the windows' min and max beside it (the run-to-run
spread inside this process)."""
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
from ecc_bench import edge_features  # noqa: E402
from gatv2_bench import graphs_of  # noqa: E402
from gcn_bn_bench import host_batch  # noqa: E402
from sage_bench import alternate, stats  # noqa: E402


def bench_step(ctx, args):
    hb = host_batch(args.shape)
    e = edge_features(hb)
    loader = gcnx.DeviceDisjointLoader(gcnx.DeviceDataset(ctx, gcnx.ListDataset(graphs_of(hb, e)), edge_features=True),
                                       batch_size=hb.n_graphs, shuffle=True, seed=0)
    models = {}
    for name, knob, te in (("gine_one_launch", "1", False), ("gine_composed", "0", False), ("gine_one_launch_train_eps", "1", True),
                           ("gine_composed_train_eps", "0", True)):
        os.environ["GCNX_GINE_FUSED"] = knob                # read once, at construction
        models[name] = gcnx.GINE(ctx, hidden_channels=64, edge_dim=2, train_eps=te, seed=0)
    os.environ.pop("GCNX_GINE_FUSED")
    models["gin"] = gcnx.GIN(ctx, hidden_channels=64, seed=0)
    models["resgated_edge2"] = gcnx.ResGated(ctx, hidden_channels=64, edge_dim=2, seed=0)
    models["gatv2_heads4_edge2"] = gcnx.GATv2(ctx, hidden_channels=64, heads=4, edge_dim=2, seed=0)
    fns = {k: (lambda m=m: m.train_step(loader.__next__()[0], lr=1e-3, fetch=False)) for k, m in models.items()}
    ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
    loss = {k: m.fetch_metrics(hb.n_graphs)[0] for k, m in models.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    best = min(("gine_one_launch", "gine_composed"), key=lambda k: med[k])
    return {"model": "gcnx.GINE", "shape": args.shape, "n_nodes": int(hb.n), "nnz": int(hb.nnz), "n_graphs": int(hb.n_graphs), "f_in": 16,
            "hidden": 64, "edge_dim": 2, "streamed": True, "steps_per_window": args.steps, "rounds": args.rounds,
            "train_step": {k: stats(v) for k, v in ms.items()},
            "graphs_per_s": {k: round(hb.n_graphs / med[k] * 1e3, 1) for k in ms},
            "one_launch_over_composed": round(med["gine_one_launch"] / med["gine_composed"], 3),
            "one_launch_over_composed_train_eps": round(med["gine_one_launch_train_eps"] / med["gine_composed_train_eps"], 3),
            "faster_route": best,
            "gine_over_gin": round(med[best] / med["gin"], 3),
            "gine_over_resgated_edge2": round(med[best] / med["resgated_edge2"], 3),
            "gine_over_gatv2_heads4_edge2": round(med[best] / med["gatv2_heads4_edge2"], 3),
            "finite": bool(all(np.isfinite(v) for v in loss.values()))}


def bench_kernel(ctx, args):
    res = []
    ed = 2
    for shape in ("ref", "ecoli"):
        hb = host_batch(shape)
        a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr).unweighted()
        a.transpose_perm()
        n, nnz = hb.n, hb.nnz
        rng = np.random.default_rng(0)
        e = ctx.to_device(edge_features(hb, ed))
        for k0, h in ((16, 64), (64, 64)):
            dev = lambda *s: ctx.to_device(rng.standard_normal(s).astype(np.float32))
            x, dtv, wa, ba, wb, bb, eps = dev(n, k0), dev(n, k0), dev(k0, h), dev(h), dev(h, h), dev(h), ctx.to_device(np.full(1, 0.1, np.float32))
            w_e, b_e = dev(ed, k0), dev(k0)
            out, t, u, dx = ctx.empty((n, h)), ctx.empty((n, k0)), ctx.empty((n, h)), ctx.empty((n, k0))
            g_w, g_b = ctx.empty((ed, k0)), ctx.empty(k0)
            scratch = ctx.empty(max(D.gine_bwd_scratch_floats(ctx, n, k0, ed), 4))

            def gine_composed():
                D.gine_aggregate(ctx, a, x, eps, e, w_e, b_e, t)
                D.gemm(ctx, t, wa, ba, u, act="relu")
                D.gemm(ctx, u, wb, bb, out)

            fns = {"gine_conv": lambda: D.gine_conv(ctx, a, x, eps, e, w_e, b_e, wa, ba, wb, bb, out, t=t, u=u),
                   "gine_aggregate_2gemm": gine_composed,
                   "gine_aggregate": lambda: D.gine_aggregate(ctx, a, x, eps, e, w_e, b_e, t),
                   "gine_bwd_edges": lambda: D.gine_bwd_edges(ctx, a, x, e, w_e, b_e, dtv, g_w, g_b, scratch),
                   "gine_bwd_nodes": lambda: D.gine_bwd_nodes(ctx, a, x, eps, e, w_e, b_e, dtv, dx),
                   "gin_conv_floor": lambda: D.gin_conv(ctx, a, x, eps, wa, ba, wb, bb, out, t=t, u=u),
                   "gin_aggregate_floor": lambda: D.gin_aggregate(ctx, a, x, eps, t)}
            ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            res.append({"shape": shape, "n_nodes": int(n), "nnz": int(nnz), "k0": k0, "k1": h, "k2": h, "edge_dim": ed,
                        **{k: stats(v) for k, v in ms.items()},
                        "conv_over_gin_conv": round(med["gine_conv"] / med["gin_conv_floor"], 3),
                        "conv_over_composed": round(med["gine_conv"] / med["gine_aggregate_2gemm"], 3),
                        "aggregate_over_gin_aggregate": round(med["gine_aggregate"] / med["gin_aggregate_floor"], 3),
                        "bwd_edges_over_gin_aggregate": round(med["gine_bwd_edges"] / med["gin_aggregate_floor"], 3),
                        "bwd_nodes_over_gin_aggregate": round(med["gine_bwd_nodes"] / med["gin_aggregate_floor"], 3)})
    return {"kernel": "gcnx_gine_*", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


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
