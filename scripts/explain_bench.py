#!/usr/bin/env python3
"""gcnx.Explainer.step and gcnx_sddmm_csr (csrc/explain.hip) timed with HIP events after warm-up.

  python scripts/explain_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/explain_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/explain_bench.py --kernel         # gcnx_sddmm_csr alone at f = 16 and 64 on both batch shapes (the tile kernel, and
                                                   # the any-width kernel on the same operands one float off alignment), next to
                                                   # gcnx_spmm_csr on the same pattern and width -- the same gather with row stores
                                                   # where the SDDMM has per-entry stores: the floor -- and to gcnx_gat_bwd_edges
                                                   # (heads = 1), the nearest existing per-entry kernel

The step is one Explainer.step() (edge mask; edge + both node-mask forms) alternated window by window with one gcnx.GCN
train_step on the same batch in the SAME process: the step adds two SDDMMs, one SpMM (node masks), two gemm_dx, the mask launches
and Adam to the model's forward and backward.  Synthetic batches from gcnx.synth; nothing outside the repository is read.
Prints one JSON line.  Every figure is the median over --rounds windows with the windows' min and max beside it."""
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
from gcnx.device import DeviceArray, DeviceCSR  # noqa: E402
from gcn_bn_bench import host_batch  # noqa: E402
from sage_bench import alternate, device_batch, stats  # noqa: E402


def bench_step(ctx, args):
    hb = host_batch(args.shape)
    batch = device_batch(ctx, hb)
    model = gcnx.GCN(ctx, hidden_channels=64, seed=0)
    model.build(16)
    trained = gcnx.GCN(ctx, hidden_channels=64, seed=0)
    runs = {"edge": dict(), "edge_node_common": dict(node_mask="common_attributes"), "edge_node_attributes": dict(node_mask="attributes")}
    ex = {k: gcnx.Explainer(model, epochs=args.steps, **kw) for k, kw in runs.items()}
    fns = {"gcn_train_step": lambda: trained.train_step(batch, lr=1e-3, fetch=False)}
    for k, e in ex.items():
        def one(e=e):
            if e._s is None:                                # (the explainers share the model: each run re-primes its cache per step)
                e.begin(batch)
            e.step()
        fns["explainer_step_" + k] = one
    ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
    finite = all(np.all(np.isfinite(e.history())) for e in ex.values())
    for e in ex.values():
        e.end()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"model": "gcnx.GCN + gcnx.Explainer", "shape": args.shape, "n_nodes": int(hb.n), "nnz": int(hb.nnz), "n_graphs": int(hb.n_graphs),
            "f_in": 16, "hidden": 64, "steps_per_window": args.steps, "rounds": args.rounds,
            "step": {k: stats(v) for k, v in ms.items()},
            **{f"{k}_over_train_step": round(med[k] / med["gcn_train_step"], 3) for k in med if k != "gcn_train_step"},
            "finite": bool(finite)}


def bench_kernel(ctx, args):
    res = []
    for shape in ("ref", "ecoli"):
        hb = host_batch(shape)
        a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr).unweighted().gcn_norm("pyg")
        n, nnz = hb.n, hb.nnz
        rng = np.random.default_rng(0)
        dev = lambda *s: ctx.to_device(rng.standard_normal(s).astype(np.float32))
        for f in (16, 64):
            l, r, out, rows = dev(n, f), dev(n, f), ctx.empty(nnz), ctx.empty((n, f))
            # the same operands one float off 16-byte alignment: the any-width kernel
            lo, ro = dev(n * f + 1), dev(n * f + 1)
            l1, r1 = (DeviceArray(ctx, b.ptr + 4, (n, f), np.float32, base=b) for b in (lo, ro))
            asrc, adst, alpha, o, dz, dad = dev(n, 1), dev(n, 1), dev(nnz, 1), dev(n, f), ctx.empty((nnz, 1)), ctx.empty((n, 1))
            fns = {"sddmm": lambda: D.sddmm(ctx, a, l, r, out),
                   "sddmm_scale_accumulate": lambda: D.sddmm(ctx, a, l, r, out, scale=a.vals, accumulate=True),
                   "sddmm_any_width": lambda: D.sddmm(ctx, a, l1, r1, out),
                   "spmm_floor": lambda: D.spmm(ctx, a, r, None, rows),
                   "gat_bwd_edges": lambda: D.gat_bwd_edges(ctx, a, r, asrc, adst, alpha, l, o, dz, dad)}
            ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            res.append({"shape": shape, "n_nodes": int(n), "nnz": int(nnz), "f": f, **{k: stats(v) for k, v in ms.items()},
                        "sddmm_over_spmm": round(med["sddmm"] / med["spmm_floor"], 3),
                        "sddmm_over_gat_bwd_edges": round(med["sddmm"] / med["gat_bwd_edges"], 3),
                        "any_width_over_tile": round(med["sddmm_any_width"] / med["sddmm"], 3)})
    return {"kernel": "gcnx_sddmm_csr", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


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
