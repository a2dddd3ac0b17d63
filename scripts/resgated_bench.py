#!/usr/bin/env python3
"""gcnx.ResGated train_step and the ResGatedGraphConv launches (csrc/resgated.hip) timed with HIP events after warm-up.

  python scripts/resgated_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/resgated_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/resgated_bench.py --kernel         # the three new launches alone at H = 64 on both batch shapes, edge_dim 0 / 2, next to
                                                    # gcnx_gatv2_aggregate and gcnx_spmm_csr at width 128 on the same pattern: an entry of
                                                    # the aggregate gathers the 2 H = 128 floats Q[j] | V[j], so a width-128 gather without
                                                    # the gate is this kernel's floor

The step is timed eagerly for edge_dim None and 2 on one resident batch, alternated window by window with a
gcnx.GATv2(heads=4, same edge_dim) and a gcnx.GCN step in the SAME process.  Prints one JSON line.  Every figure is the median
over --rounds windows with the windows' min and max beside it (the run-to-run spread inside this process)."""
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
from gcnx.device import DeviceCSR, Segments  # noqa: E402
from gcnx.models import DeviceBatch  # noqa: E402
from ecc_bench import edge_features  # noqa: E402
from gcn_bn_bench import host_batch  # noqa: E402
from sage_bench import alternate, device_batch, stats  # noqa: E402


def bench_step(ctx, args):
    hb = host_batch(args.shape)
    e = edge_features(hb)
    batch = device_batch(ctx, hb)
    batch_e = DeviceBatch(ctx, batch.x, DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr), Segments(ctx, hb.graph_ptr),
                          batch.y, e=ctx.to_device(e))
    models = {"resgated": gcnx.ResGated(ctx, hidden_channels=64, seed=0),
              "resgated_edge2": gcnx.ResGated(ctx, hidden_channels=64, edge_dim=2, seed=0),
              "gatv2_heads4": gcnx.GATv2(ctx, hidden_channels=64, heads=4, seed=0),
              "gatv2_heads4_edge2": gcnx.GATv2(ctx, hidden_channels=64, heads=4, edge_dim=2, seed=0),
              "gcn": gcnx.GCN(ctx, hidden_channels=64, seed=0)}
    fns = {k: (lambda m=m, b=(batch_e if "edge2" in k else batch): m.train_step(b, lr=1e-3, fetch=False)) for k, m in models.items()}
    ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
    loss = {k: m.fetch_metrics(hb.n_graphs)[0] for k, m in models.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"model": "gcnx.ResGated", "shape": args.shape, "n_nodes": int(hb.n), "nnz": int(hb.nnz), "n_graphs": int(hb.n_graphs), "f_in": 16,
            "hidden": 64, "steps_per_window": args.steps, "rounds": args.rounds, "train_step": {k: stats(v) for k, v in ms.items()},
            "graphs_per_s": {k: round(hb.n_graphs / med[k] * 1e3, 1) for k in ms},
            "resgated_over_gatv2": round(med["resgated"] / med["gatv2_heads4"], 3),
            "resgated_edge2_over_gatv2_edge2": round(med["resgated_edge2"] / med["gatv2_heads4_edge2"], 3),
            "resgated_over_gcn": round(med["resgated"] / med["gcn"], 3),
            "finite": bool(all(np.isfinite(v) for v in loss.values()))}


def bench_kernel(ctx, args):
    res = []
    h = 64
    for shape in ("ref", "ecoli"):
        hb = host_batch(shape)
        a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr).unweighted()
        a.transpose_perm()
        n, nnz = hb.n, hb.nnz
        rng = np.random.default_rng(0)
        dev = lambda *s: ctx.to_device(rng.standard_normal(s).astype(np.float32))
        p, dout, bias, out, dp = dev(n, 4 * h), dev(n, h), dev(h), ctx.empty((n, h)), ctx.empty((n, 4 * h))
        # the yardsticks at width 2 H = 128: GATv2 (heads 4) on Xl | Xr [n, 256], the plain gather on 128 columns of the same rows
        xlr, att, bias2, out2, floor_out = dev(n, 4 * h), ctx.to_device((rng.standard_normal((4, 32)) / np.sqrt(32)).astype(np.float32)), dev(2 * h), \
            ctx.empty((n, 2 * h)), ctx.empty((n, 2 * h))
        for ed in (0, 2):
            e = ctx.to_device(edge_features(hb, ed)) if ed else None
            w_e, w_e2 = (dev(ed, 3 * h), dev(ed, 2 * h)) if ed else (None, None)
            dwe = ctx.empty((ed, 3 * h)) if ed else None
            scratch = ctx.empty(max(D.resgated_bwd_scratch_floats(ctx, n, h, ed), 1))
            fns = {"resgated_aggregate": lambda: D.resgated_aggregate(ctx, a, p, out, e=e, w_e=w_e, skip=p.cols(3 * h, 4 * h), bias=bias),
                   "resgated_bwd_targets": lambda: D.resgated_bwd_targets(ctx, a, p, dout, dp.cols(0, h), scratch, ds=dp.cols(3 * h, 4 * h), e=e,
                                                                          w_e=w_e, dw_e=dwe),
                   "resgated_bwd_sources": lambda: D.resgated_bwd_sources(ctx, a, p, dout, dp.cols(h, 3 * h), e=e, w_e=w_e),
                   "gatv2_aggregate_w128": lambda: D.gatv2_aggregate(ctx, a, xlr, att, bias2, out2, e=e, w_e=w_e2),
                   "spmm_csr_w128_floor": lambda: D.spmm(ctx, a, xlr.cols(0, 2 * h), None, floor_out)}
            ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            res.append({"shape": shape, "n_nodes": int(n), "nnz": int(nnz), "h": h, "edge_dim": ed, **{k: stats(v) for k, v in ms.items()},
                        "aggregate_over_floor": round(med["resgated_aggregate"] / med["spmm_csr_w128_floor"], 3),
                        "aggregate_over_gatv2_aggregate": round(med["resgated_aggregate"] / med["gatv2_aggregate_w128"], 3),
                        "gatv2_aggregate_over_floor": round(med["gatv2_aggregate_w128"] / med["spmm_csr_w128_floor"], 3),
                        "bwd_targets_over_floor": round(med["resgated_bwd_targets"] / med["spmm_csr_w128_floor"], 3),
                        "bwd_sources_over_floor": round(med["resgated_bwd_sources"] / med["spmm_csr_w128_floor"], 3)})
    return {"kernel": "gcnx_resgated_*", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


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
