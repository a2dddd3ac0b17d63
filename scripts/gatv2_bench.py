#!/usr/bin/env python3
"""gcnx.GATv2 train_step and the GATv2Conv launches (csrc/gatv2.hip) timed with HIP events after warm-up.

  python scripts/gatv2_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/gatv2_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/gatv2_bench.py --kernel         # every new launch alone at width 64 on both batch shapes, heads 1 / 4, edge_dim 0 / 2,
                                                 # next to gcnx_gat_aggregate and gcnx_spmm_csr on the same pattern and width: the
                                                 # same gather with scores from two scalars per entry, and without scores (the floor)

The step is timed for heads 1 and 4 without edge features and for heads 4 with edge_dim 2 -- on one resident batch, and streamed:
every step a fresh batch of the same graphs from DeviceDisjointLoader(DeviceDataset(edge_features=True)), collate included --
alternated window by window with a gcnx.GAT and a gcnx.GCN step in the SAME process.  Prints one JSON line.  Every figure is the
median over --rounds windows with the windows' min and max beside it (the run-to-run spread inside this process)."""
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


def graphs_of(hb, e):
    """The batch split back into gcnx.Graph objects (x, scipy CSR a, e, one-hot y)."""
    import scipy.sparse as sp
    a = sp.csr_matrix((np.ones(hb.nnz), hb.colidx, hb.rowptr), shape=(hb.n, hb.n))
    out = []
    for g in range(hb.n_graphs):
        lo, hi = int(hb.graph_ptr[g]), int(hb.graph_ptr[g + 1])
        out.append(gcnx.Graph(x=hb.x[lo:hi], a=a[lo:hi, lo:hi], e=e[hb.rowptr[lo]:hb.rowptr[hi]], y=hb.y[g]))
    return out


def bench_step(ctx, args):
    hb = host_batch(args.shape)
    e = edge_features(hb)
    batch = device_batch(ctx, hb)
    batch_e = DeviceBatch(ctx, batch.x, DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr), Segments(ctx, hb.graph_ptr),
                          batch.y, e=ctx.to_device(e))
    loader = gcnx.DeviceDisjointLoader(gcnx.DeviceDataset(ctx, gcnx.ListDataset(graphs_of(hb, e)), edge_features=True),
                                       batch_size=hb.n_graphs, shuffle=True, seed=0)
    v2 = lambda **kw: gcnx.GATv2(ctx, hidden_channels=64, seed=0, **kw)
    models = {"gatv2_heads1": v2(heads=1), "gatv2_heads4": v2(heads=4), "gatv2_heads4_edge2": v2(heads=4, edge_dim=2),
              "gatv2_heads4_edge2_streamed": v2(heads=4, edge_dim=2), "gat_heads4": gcnx.GAT(ctx, hidden_channels=64, heads=4, seed=0),
              "gcn": gcnx.GCN(ctx, hidden_channels=64, seed=0)}
    fns = {k: (lambda m=m, b=(batch_e if "edge2" in k else batch): m.train_step(b, lr=1e-3, fetch=False)) for k, m in models.items()}
    fns["gatv2_heads4_edge2_streamed"] = lambda m=models["gatv2_heads4_edge2_streamed"]: m.train_step(loader.__next__()[0], lr=1e-3, fetch=False)
    ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
    loss = {k: m.fetch_metrics(hb.n_graphs)[0] for k, m in models.items()}
    return {"model": "gcnx.GATv2", "shape": args.shape, "n_nodes": int(hb.n), "nnz": int(hb.nnz), "n_graphs": int(hb.n_graphs), "f_in": 16,
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
        xlr, dout, bias, floor_out = dev(n, 2 * hc), dev(n, hc), dev(hc), ctx.empty((n, hc))
        hf = xlr.cols(0, hc)                                # the operand of the two yardsticks: the same rows at the same stride
        for heads in (1, 4):
            c = hc // heads
            att, att2 = (ctx.to_device((rng.standard_normal((heads, c)) / np.sqrt(c)).astype(np.float32)) for _ in range(2))
            asrc, adst = ctx.empty((n, heads)), ctx.empty((n, heads))
            D.gat_scores(ctx, hf, att, att2, asrc, adst)
            alpha, dscore, alpha_gat = ctx.empty((nnz, heads)), ctx.empty((nnz, heads)), ctx.empty((nnz, heads))
            out, o, o_gat, dxlr, datt = ctx.empty((n, hc)), ctx.empty((n, hc)), ctx.empty((n, hc)), ctx.empty((n, 2 * hc)), ctx.empty((heads, c))
            for ed in (0, 2):
                e = ctx.to_device(edge_features(hb, ed)) if ed else None
                w_e = dev(ed, hc) if ed else None
                dwe = ctx.empty((ed, hc)) if ed else None
                scratch = ctx.empty(max(D.gatv2_bwd_scratch_floats(ctx, n, heads, c, ed), 1))
                fns = {"gatv2_aggregate": lambda: D.gatv2_aggregate(ctx, a, xlr, att, bias, out, e=e, w_e=w_e, alpha=alpha, o_pre=o),
                       "gatv2_aggregate_out_only": lambda: D.gatv2_aggregate(ctx, a, xlr, att, bias, out, e=e, w_e=w_e),
                       "gatv2_bwd_edges": lambda: D.gatv2_bwd_edges(ctx, a, xlr, att, alpha, dout, o, dscore, dxlr.cols(hc, 2 * hc), datt, scratch,
                                                                    e=e, w_e=w_e, dw_e=dwe),
                       "gatv2_bwd_nodes": lambda: D.gatv2_bwd_nodes(ctx, a, xlr, att, alpha, dscore, dout, dxlr.cols(0, hc), e=e, w_e=w_e),
                       "gat_aggregate": lambda: D.gat_aggregate(ctx, a, hf, asrc, adst, bias, out, alpha=alpha_gat, o_pre=o_gat),
                       "spmm_csr_floor": lambda: D.spmm(ctx, a, hf, None, floor_out)}
                fns["gatv2_aggregate"]()                    # every launch reads what the ones before it wrote
                fns["gatv2_bwd_edges"]()
                ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
                med = {k: float(np.median(v)) for k, v in ms.items()}
                res.append({"shape": shape, "n_nodes": int(n), "nnz": int(nnz), "width": hc, "heads": heads, "edge_dim": ed,
                            **{k: stats(v) for k, v in ms.items()},
                            "aggregate_over_floor": round(med["gatv2_aggregate"] / med["spmm_csr_floor"], 3),
                            "aggregate_over_gat_aggregate": round(med["gatv2_aggregate"] / med["gat_aggregate"], 3),
                            "bwd_edges_over_floor": round(med["gatv2_bwd_edges"] / med["spmm_csr_floor"], 3),
                            "bwd_nodes_over_floor": round(med["gatv2_bwd_nodes"] / med["spmm_csr_floor"], 3)})
    return {"kernel": "gcnx_gatv2_*", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


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
