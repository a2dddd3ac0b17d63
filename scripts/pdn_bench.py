#!/usr/bin/env python3
"""gcnx.PDN train_step and the PDNConv operator launches (csrc/pdn.hip) timed with HIP events after warm-up.

  python scripts/pdn_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/pdn_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/pdn_bench.py --kernel         # gcnx_pdn_operator and gcnx_pdn_operator_bwd alone (edge_dim 2, edge_hidden 16) on both
                                               # batch shapes, next to gcnx_edge_mask_fwd / gcnx_edge_mask_bwd on the same pattern -- the
                                               # same per-entry pass without the MLP and the degree walk: the floor -- and to
                                               # gcnx_sddmm_csr at f = 16 and 64, the other per-entry launch of a PDN step

The step is timed streamed: every step a fresh batch of the same graphs from DeviceDisjointLoader(DeviceDataset(
edge_features=True)), collate included -- alternated window by window with a gcnx.GCN and a gcnx.GINE(edge_dim=2) step fed by the
same loader in the SAME process.  Prints one JSON line.  Every figure is the median over --rounds windows with the windows' min
and max beside it (the run-to-run spread inside this process)."""
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
    models = {"pdn": gcnx.PDN(ctx, hidden_channels=64, edge_dim=2, edge_hidden=16, seed=0),
              "gcn": gcnx.GCN(ctx, hidden_channels=64, seed=0),
              "gine_edge2": gcnx.GINE(ctx, hidden_channels=64, edge_dim=2, seed=0)}
    fns = {k: (lambda m=m: m.train_step(loader.__next__()[0], lr=1e-3, fetch=False)) for k, m in models.items()}
    ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
    loss = {k: m.fetch_metrics(hb.n_graphs)[0] for k, m in models.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"model": "gcnx.PDN", "shape": args.shape, "n_nodes": int(hb.n), "nnz": int(hb.nnz), "n_graphs": int(hb.n_graphs), "f_in": 16,
            "hidden": 64, "edge_dim": 2, "edge_hidden": 16, "streamed": True, "steps_per_window": args.steps, "rounds": args.rounds,
            "train_step": {k: stats(v) for k, v in ms.items()},
            "graphs_per_s": {k: round(hb.n_graphs / med[k] * 1e3, 1) for k in ms},
            "pdn_over_gcn": round(med["pdn"] / med["gcn"], 3), "pdn_over_gine_edge2": round(med["pdn"] / med["gine_edge2"], 3),
            "finite": bool(all(np.isfinite(v) for v in loss.values()))}


def bench_kernel(ctx, args):
    res = []
    d, he = 2, 16
    for shape in ("ref", "ecoli"):
        hb = host_batch(shape)
        a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr).unweighted()
        rp_t, ci_t, pm = a.transpose_perm()
        a_hat = a.gcn_norm("pyg")                           # the mask kernels' operator: the same pattern with values
        n, nnz = hb.n, hb.nnz
        rng = np.random.default_rng(0)
        dev = lambda *s: ctx.to_device(rng.standard_normal(s).astype(np.float32))
        e = ctx.to_device(edge_features(hb, d))
        w1, b1, w2, b2 = dev(d, he), dev(he), dev(he), dev(1)
        gate, r, v, vt, g, logits, dm = ctx.empty(nnz), ctx.empty(n), ctx.empty(nnz), ctx.empty(nnz), dev(nnz), dev(nnz), ctx.empty(nnz)
        dw1, db1, dw2, db2, terms = ctx.empty((d, he)), ctx.empty(he), ctx.empty(he), ctx.empty(1), ctx.empty(2)
        scratch = ctx.empty(D.pdn_bwd_scratch_floats(ctx, n, nnz, d, he))
        mscratch = ctx.empty(D.mask_scratch_floats(ctx))
        l16, r16, l64, r64 = dev(n, 16), dev(n, 16), dev(n, 64), dev(n, 64)
        D.pdn_operator(ctx, a, e, w1, b1, w2, b2, gate, r, v, perm_t=pm, vals_t_out=vt)
        fns = {"pdn_operator": lambda: D.pdn_operator(ctx, a, e, w1, b1, w2, b2, gate, r, v, perm_t=pm, vals_t_out=vt),
               "pdn_operator_bwd": lambda: D.pdn_operator_bwd(ctx, a, e, w1, b1, w2, b2, gate, r, g, dw1, db1, dw2, db2, scratch),
               "edge_mask_fwd_floor": lambda: D.edge_mask_fwd(ctx, a_hat, logits, v, pm, vt),
               "edge_mask_bwd_floor": lambda: D.edge_mask_bwd(ctx, a_hat, logits, g, dm, terms, mscratch),
               "sddmm_16": lambda: D.sddmm(ctx, a, l16, r16, dm),
               "sddmm_64": lambda: D.sddmm(ctx, a, l64, r64, dm)}
        ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
        med = {k: float(np.median(v_)) for k, v_ in ms.items()}
        res.append({"shape": shape, "n_nodes": int(n), "nnz": int(nnz), "edge_dim": d, "edge_hidden": he,
                    **{k: stats(v_) for k, v_ in ms.items()},
                    "operator_over_edge_mask_fwd": round(med["pdn_operator"] / med["edge_mask_fwd_floor"], 3),
                    "operator_bwd_over_edge_mask_bwd": round(med["pdn_operator_bwd"] / med["edge_mask_bwd_floor"], 3),
                    "operator_over_sddmm_64": round(med["pdn_operator"] / med["sddmm_64"], 3),
                    "operator_bwd_over_sddmm_64": round(med["pdn_operator_bwd"] / med["sddmm_64"], 3)})
    return {"kernel": "gcnx_pdn_operator(_bwd)", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


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
