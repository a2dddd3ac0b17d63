#!/usr/bin/env python3
"""gcnx.RGCN train_step, gcnx_rgcn_conv and gcnx_rgcn_operator timing with HIP events after warm-up; the one-launch route against
the composed route (GCNX_RGCN_FUSED=0: gcnx_rgcn_aggregate + gcnx_gemm x 2 + gcnx_add, gcnx_rgcn_aggregate + R + 1 gcnx_gemm_dx)
and against gcnx.SAGE and gcnx.GCN on the same batch, in the SAME process, alternated window by window.

  python scripts/rgcn_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/rgcn_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/rgcn_bench.py --kernel         # gcnx_rgcn_conv alone (forward with the panel, transposed backward) at 16 -> 64 and
                                                # 64 -> 64 on both batch shapes, against the panel route and against gcnx_sage_conv
                                                # on the same pattern (the floor: the same gather into one accumulator), and
                                                # gcnx_rgcn_operator alone

The edge features are reference-style (dca on ~8 % of the entries, proximity on most, neither on every stored loop and some
contacts): R = 3 under relations="nonzero".  Prints one JSON line.  Every figure is the median over --rounds windows with the
windows' min and max beside it (the run-to-run spread inside this process)."""
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
from gcn_bn_bench import host_batch  # noqa: E402
from sage_bench import alternate, stats  # noqa: E402

R = 3


def edge_features(hb, seed=5):
    rows = np.repeat(np.arange(hb.n), np.diff(hb.rowptr))
    rng = np.random.default_rng(seed)
    u = rng.random(hb.nnz)
    kind = np.where(rows == hb.colidx, 2, np.where(u < 0.08, 0, np.where(u < 0.85, 1, 2)))
    e = np.zeros((hb.nnz, 2), np.float32)
    e[kind == 0, 0] = rng.uniform(0.2, 1.5, int((kind == 0).sum()))
    e[kind == 1, 1] = rng.uniform(0.2, 1.5, int((kind == 1).sum()))
    return e


def device_batch(ctx, hb, e):
    return DeviceBatch(ctx, ctx.to_device(hb.x), DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr),
                       Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y), e=ctx.to_device(e))


def bench_step(ctx, args):
    hb = host_batch(args.shape)
    batch = device_batch(ctx, hb, edge_features(hb))
    models = {}
    for name, knob in (("one_launch", "1"), ("composed", "0")):
        os.environ["GCNX_RGCN_FUSED"] = knob                # read once, at construction
        models[name] = gcnx.RGCN(ctx, hidden_channels=64, seed=0)
    models["sage"], models["gcn"] = gcnx.SAGE(ctx, hidden_channels=64, seed=0), gcnx.GCN(ctx, hidden_channels=64, seed=0)
    ms = alternate(ctx, {k: (lambda m=m: m.train_step(batch, lr=1e-3, fetch=False)) for k, m in models.items()},
                   args.steps, args.rounds, args.warmup)
    loss = {k: m.fetch_metrics(hb.n_graphs)[0] for k, m in models.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"model": "gcnx.RGCN", "shape": args.shape, "n_nodes": int(hb.n), "n_graphs": int(hb.n_graphs), "nnz": int(hb.nnz), "f_in": 16,
            "hidden": 64, "num_relations": R, "steps_per_window": args.steps, "rounds": args.rounds,
            "train_step": {k: stats(v) for k, v in ms.items()},
            "one_launch_over_composed": round(med["one_launch"] / med["composed"], 3),
            "one_launch_over_sage": round(med["one_launch"] / med["sage"], 3), "one_launch_over_gcn": round(med["one_launch"] / med["gcn"], 3),
            "graphs_per_s_one_launch": round(hb.n_graphs / med["one_launch"] * 1e3, 1),
            "finite": bool(all(np.isfinite(v) for v in loss.values()))}


def bench_kernel(ctx, args):
    res, ops_ms = [], []
    for shape in ("ref", "ecoli"):
        hb = host_batch(shape)
        a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr).unweighted()
        e = ctx.to_device(edge_features(hb))
        rel, val, rel_t, val_t = a.rgcn_operator(e, "nonzero", R)
        rp_t, ci_t, perm = a.transpose_perm()
        a_mean = a.row_mean()
        a_mean_t = a_mean.transpose()
        n = hb.n
        rng = np.random.default_rng(0)
        op = alternate(ctx, {"operator": lambda: ctx._ck(ctx.lib.gcnx_rgcn_operator(
            ctx.h, a.rowptr.ptr, e.ptr, 2, 2, 0, R, perm.ptr, a.n, a.nnz, rel.ptr, val.ptr, rel_t.ptr, val_t.ptr))},
            args.steps, args.rounds, args.warmup)
        ops_ms.append({"shape": shape, "n_nodes": int(n), "nnz": int(hb.nnz), **stats(op["operator"])})
        for fi, fo in ((16, 64), (64, 64)):
            dev = lambda *s: ctx.to_device(rng.standard_normal(s).astype(np.float32))
            x, dz, w, b = dev(n, fi), dev(n, fo), dev((R + 1) * fi, fo), dev(fo)
            wl, wr = w.flat(0, fi * fo, (fi, fo)), w.flat(R * fi * fo, fi * fo, (fi, fo))
            out, m, h, dx, mt, s = (ctx.empty((n, fo)), ctx.empty((n, R * fi)), ctx.empty((n, fo)), ctx.empty((n, fi)),
                                    ctx.empty((n, R * fo)), ctx.empty((n, fi)))

            def fwd_composed():
                D.rgcn_aggregate(ctx, a.rowptr, a.colidx, rel, val, x, m, R)
                D.gemm(ctx, m, w.flat(0, R * fi * fo, (R * fi, fo)), b, out)
                D.gemm(ctx, x, wr, None, h)
                D.add(ctx, out, h, out)

            def bwd_composed():
                D.rgcn_aggregate(ctx, rp_t, ci_t, rel_t, val_t, dz, mt, R)
                D.gemm_dx(ctx, dz, wr, dx)
                for q in range(R):
                    D.gemm_dx(ctx, mt.cols(q * fo, (q + 1) * fo), w.flat(q * fi * fo, fi * fo, (fi, fo)), dx, accumulate=True)

            fns = {"fwd_one_launch": lambda: D.rgcn_conv(ctx, a.rowptr, a.colidx, rel, val, x, w, b, out, R, True, m=m),
                   "fwd_composed": fwd_composed,
                   "fwd_sage_conv": lambda: D.sage_conv(ctx, a_mean, x, wl, wr, b, out, s=s)}
            if fi == fo:      # the backward with respect to x of the hidden layer
                fns.update({"bwd_one_launch": lambda: D.rgcn_conv(ctx, rp_t, ci_t, rel_t, val_t, dz, w, None, dx, R, True, w_transposed=True),
                            "bwd_composed": bwd_composed,
                            "bwd_sage_conv": lambda: D.sage_conv(ctx, a_mean_t, dz, wl, wr, None, dx, w_transposed=True)})
            ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
            res.append({"shape": shape, "n_nodes": int(n), "nnz": int(hb.nnz), "fi": fi, "fo": fo, **{k: stats(v) for k, v in ms.items()}})
    return {"kernel": "gcnx_rgcn_conv", "num_relations": R, "calls_per_window": args.steps, "rounds": args.rounds, "cases": res,
            "gcnx_rgcn_operator": ops_ms}


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
