#!/usr/bin/env python3
"""gcnx.Transformer train_step and the TransformerConv launches (csrc/transformer.hip) timed with HIP events after warm-up.

  python scripts/transformer_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/transformer_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/transformer_bench.py --kernel         # the four new launches alone at HC = 64 on both batch shapes, heads 1 / 4,
                                                       # edge_dim 0 / 2, next to gcnx_gatv2_aggregate, gcnx_resgated_aggregate and
                                                       # gcnx_spmm_csr at width 128 on the same pattern: an entry of the aggregate
                                                       # gathers the 2 HC = 128 floats K[j] | V[j], so a width-128 gather without the
                                                       # softmax is this kernel's floor

The step is timed eagerly for heads 4 with edge_dim None and 2 (and with the beta gate) on one resident batch, alternated window
by window with a gcnx.GATv2(heads=4, same edge_dim), a gcnx.ResGated(same edge_dim) and a gcnx.GCN step in the SAME process.
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
    models = {"transformer_heads1": gcnx.Transformer(ctx, hidden_channels=64, heads=1, seed=0),
              "transformer_heads4": gcnx.Transformer(ctx, hidden_channels=64, heads=4, seed=0),
              "transformer_heads4_edge2": gcnx.Transformer(ctx, hidden_channels=64, heads=4, edge_dim=2, seed=0),
              "transformer_heads4_beta_edge2": gcnx.Transformer(ctx, hidden_channels=64, heads=4, edge_dim=2, beta=True, seed=0),
              "gatv2_heads4": gcnx.GATv2(ctx, hidden_channels=64, heads=4, seed=0),
              "gatv2_heads4_edge2": gcnx.GATv2(ctx, hidden_channels=64, heads=4, edge_dim=2, seed=0),
              "resgated": gcnx.ResGated(ctx, hidden_channels=64, seed=0),
              "resgated_edge2": gcnx.ResGated(ctx, hidden_channels=64, edge_dim=2, seed=0),
              "gcn": gcnx.GCN(ctx, hidden_channels=64, seed=0)}
    fns = {k: (lambda m=m, b=(batch_e if "edge2" in k else batch): m.train_step(b, lr=1e-3, fetch=False)) for k, m in models.items()}
    ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
    loss = {k: m.fetch_metrics(hb.n_graphs)[0] for k, m in models.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"model": "gcnx.Transformer", "shape": args.shape, "n_nodes": int(hb.n), "nnz": int(hb.nnz), "n_graphs": int(hb.n_graphs), "f_in": 16,
            "hidden": 64, "steps_per_window": args.steps, "rounds": args.rounds, "train_step": {k: stats(v) for k, v in ms.items()},
            "graphs_per_s": {k: round(hb.n_graphs / med[k] * 1e3, 1) for k in ms},
            "transformer_over_gatv2": round(med["transformer_heads4"] / med["gatv2_heads4"], 3),
            "transformer_edge2_over_gatv2_edge2": round(med["transformer_heads4_edge2"] / med["gatv2_heads4_edge2"], 3),
            "transformer_over_resgated": round(med["transformer_heads4"] / med["resgated"], 3),
            "transformer_edge2_over_resgated_edge2": round(med["transformer_heads4_edge2"] / med["resgated_edge2"], 3),
            "transformer_over_gcn": round(med["transformer_heads4"] / med["gcn"], 3),
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
        p, dout, out, o, d_o, dp = dev(n, 4 * hc), dev(n, hc), ctx.empty((n, hc)), ctx.empty((n, hc)), ctx.empty((n, hc)), ctx.empty((n, 4 * hc))
        w_beta, dwb = ctx.to_device((rng.standard_normal(3 * hc) / 8).astype(np.float32)), ctx.empty(3 * hc)
        # the yardsticks at width 2 HC = 128: GATv2 (heads 4) on Xl | Xr [n, 256], ResGated at H = 64 on K | Q | V | S (the same
        # 2 H gather), the plain gather on 128 columns of the same rows
        xlr, att, bias2, out2, floor_out = dev(n, 4 * hc), ctx.to_device((rng.standard_normal((4, 32)) / np.sqrt(32)).astype(np.float32)), \
            dev(2 * hc), ctx.empty((n, 2 * hc)), ctx.empty((n, 2 * hc))
        bias = dev(hc)
        for heads in (1, 4):
            alpha, dscore = ctx.empty((nnz, heads)), ctx.empty((nnz, heads))
            for ed in (0, 2):
                e = ctx.to_device(edge_features(hb, ed)) if ed else None
                w_e, w_e2, w_e3 = (dev(ed, hc), dev(ed, 2 * hc), dev(ed, 3 * hc)) if ed else (None, None, None)
                dwe = ctx.empty((ed, hc)) if ed else None
                scratch = ctx.empty(max(D.transformer_bwd_scratch_floats(ctx, n, heads, hc // heads, ed, True), 1))
                skip = p.cols(3 * hc, 4 * hc)
                agg = lambda wb=None: D.transformer_aggregate(ctx, a, p, out, heads, e=e, w_e=w_e, skip=skip, w_beta=wb, alpha=alpha, o_pre=o)
                agg()                                                    # alpha and O of the backward calls
                fns = {"transformer_aggregate": agg,
                       "transformer_aggregate_beta": lambda: agg(w_beta),
                       "transformer_aggregate_inference": lambda: D.transformer_aggregate(ctx, a, p, out, heads, e=e, w_e=w_e, skip=skip),
                       "transformer_beta_bwd": lambda: D.transformer_beta_bwd(ctx, dout, o, skip, w_beta, d_o, dp.cols(3 * hc, 4 * hc), dwb, scratch),
                       "transformer_bwd_targets": lambda: D.transformer_bwd_targets(ctx, a, p, alpha, dout, o, dscore, dp.cols(0, hc), heads, scratch,
                                                                                    ds=dp.cols(3 * hc, 4 * hc), e=e, w_e=w_e, dw_e=dwe),
                       "transformer_bwd_sources": lambda: D.transformer_bwd_sources(ctx, a, p, alpha, dscore, dout, dp.cols(hc, 3 * hc), heads),
                       "gatv2_aggregate_w128": lambda: D.gatv2_aggregate(ctx, a, xlr, att, bias2, out2, e=e, w_e=w_e2),
                       "resgated_aggregate": lambda: D.resgated_aggregate(ctx, a, p, out, e=e, w_e=w_e3, skip=skip, bias=bias),
                       "spmm_csr_w128_floor": lambda: D.spmm(ctx, a, xlr.cols(0, 2 * hc), None, floor_out)}
                ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
                med = {k: float(np.median(v)) for k, v in ms.items()}
                floor = med["spmm_csr_w128_floor"]
                res.append({"shape": shape, "n_nodes": int(n), "nnz": int(nnz), "hc": hc, "heads": heads, "edge_dim": ed,
                            **{k: stats(v) for k, v in ms.items()},
                            "aggregate_over_floor": round(med["transformer_aggregate"] / floor, 3),
                            "aggregate_over_gatv2_aggregate": round(med["transformer_aggregate"] / med["gatv2_aggregate_w128"], 3),
                            "aggregate_over_resgated_aggregate": round(med["transformer_aggregate"] / med["resgated_aggregate"], 3),
                            "bwd_targets_over_floor": round(med["transformer_bwd_targets"] / floor, 3),
                            "bwd_sources_over_floor": round(med["transformer_bwd_sources"] / floor, 3)})
    return {"kernel": "gcnx_transformer_*", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


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
