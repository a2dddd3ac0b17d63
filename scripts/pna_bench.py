#!/usr/bin/env python3
"""gcnx.PNA train_step and gcnx_pna_aggregate / gcnx_pna_bwd timing with HIP events after warm-up; the PNA step against
gcnx.GIN and gcnx.GCN in the SAME process, alternated window by window, and the two kernels against gcnx_spmm_csr + 2 x
gcnx_spmm_csr_minmax on the same pattern: the three-gather floor for three of the four statistics.

  python scripts/pna_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/pna_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/pna_bench.py --kernel         # gcnx_pna_aggregate (with and without the statistics) and gcnx_pna_bwd alone at
                                               # F = 64 on both batch shapes, next to the three gathers (and their three
                                               # backward gathers); + the algorithmic bytes of the one-gather forms

Prints one JSON line.  Every figure is the median over --rounds windows with the windows' min and max beside it (the
run-to-run spread inside this process)."""
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
    hist = np.bincount(np.diff(hb.rowptr))
    models = {"pna": gcnx.PNA(ctx, hidden_channels=64, deg=hist, seed=0), "gin": gcnx.GIN(ctx, hidden_channels=64, seed=0),
              "gcn": gcnx.GCN(ctx, hidden_channels=64, seed=0)}
    ms = alternate(ctx, {k: (lambda m=m: m.train_step(batch, lr=1e-3, fetch=False)) for k, m in models.items()},
                   args.steps, args.rounds, args.warmup)
    loss = {k: m.fetch_metrics(hb.n_graphs)[0] for k, m in models.items()}
    return {"model": "gcnx.PNA", "shape": args.shape, "n_nodes": int(hb.n), "n_graphs": int(hb.n_graphs), "f_in": 16, "hidden": 64,
            "avg_deg_log": round(models["pna"].avg_deg_log[0], 6), "steps_per_window": args.steps, "rounds": args.rounds,
            "train_step": {k: stats(v) for k, v in ms.items()},
            "graphs_per_s_pna": round(hb.n_graphs / float(np.median(ms["pna"])) * 1e3, 1),
            "finite": bool(all(np.isfinite(v) for v in loss.values()))}


def fwd_bytes(n, nnz, f, keep):
    """Bytes gcnx_pna_aggregate has to move once: CSR, x, P | Q (the gathered Q rows count once: the same array), C, and the
    statistics when kept."""
    return 4 * (n + 1 + nnz) + 4 * n * f * (1 + 2 + 13 + (6 if keep else 0))


def bwd_bytes(n, nnz, f):
    """gcnx_pna_bwd: both patterns' row pointers and the transposed columns, Q, the statistics, 12 blocks of dC, dP | dQ and
    the coefficient rows written and read once."""
    return 4 * (2 * (n + 1) + nnz) + 4 * n * f * (1 + 6 + 12 + 2 + 2 * 4)


def bench_kernel(ctx, args):
    res = []
    f = 64
    for shape in ("ref", "ecoli"):
        hb = host_batch(shape)
        a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr).unweighted()
        a_t = a.transpose()
        a_mean, n = a.row_mean(), hb.n
        a_mean_t = a_mean.transpose()
        hist = np.bincount(np.diff(hb.rowptr))
        delta = float((hist * np.log(np.arange(hist.size) + 1.0)).sum() / hist.sum())
        rng = np.random.default_rng(0)
        dev = lambda *s: ctx.to_device(rng.standard_normal(s).astype(np.float32))
        x, pq, dc = dev(n, f), dev(n, 2 * f), dev(n, 13 * f)
        c, st, dpq = ctx.empty((n, 13 * f)), ctx.empty((n, 6 * f)), ctx.empty((n, 2 * f))
        coef = ctx.empty(D.pna_bwd_scratch_floats(ctx, n, f))
        q = dev(n, f)                                          # the floor gathers a packed array
        o_mean, o_min, o_max, c_min, c_max = (ctx.empty((n, f)) for _ in range(5))
        g, d_mean, d_min, d_max = dev(n, f), ctx.empty((n, f)), ctx.empty((n, f)), ctx.empty((n, f))

        def three_gathers():
            D.spmm(ctx, a_mean, q, None, o_mean)
            D.spmm_minmax(ctx, a, q, o_min, cnt=c_min, mode="min")
            D.spmm_minmax(ctx, a, q, o_max, cnt=c_max, mode="max")

        def three_gathers_bwd():
            D.spmm(ctx, a_mean_t, g, None, d_mean)
            D.spmm_minmax_bwd(ctx, a_t, q, o_min, c_min, g, d_min, mode="min")
            D.spmm_minmax_bwd(ctx, a_t, q, o_max, c_max, g, d_max, mode="max")

        D.pna_aggregate(ctx, a, x, pq, delta, c, st)
        three_gathers()
        fns = {"pna_aggregate": lambda: D.pna_aggregate(ctx, a, x, pq, delta, c, st),
               "pna_aggregate_no_stats": lambda: D.pna_aggregate(ctx, a, x, pq, delta, c, None),
               "three_gathers": three_gathers,
               "pna_bwd": lambda: D.pna_bwd(ctx, a, a_t, pq, st, dc, delta, dpq, coef),
               "three_gathers_bwd": three_gathers_bwd}
        ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
        res.append({"shape": shape, "n_nodes": int(n), "nnz": int(hb.nnz), "f": f, "fwd_bytes": fwd_bytes(n, hb.nnz, f, True),
                    "fwd_bytes_no_stats": fwd_bytes(n, hb.nnz, f, False), "bwd_bytes": bwd_bytes(n, hb.nnz, f),
                    **{k: stats(v) for k, v in ms.items()}})
    return {"kernel": "gcnx_pna_aggregate / gcnx_pna_bwd", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


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
