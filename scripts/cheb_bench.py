#!/usr/bin/env python3
"""gcnx.Cheb train_step and gcnx_cheb_sum / gcnx_cheb_basis timing with HIP events after warm-up; the one-launch (resident) route
against the one-launch-per-gather (streamed) route (GCNX_CHEB_RESIDENT=0) and against gcnx.GCN and gcnx.APPNP in the SAME
process, alternated window by window.

  python scripts/cheb_bench.py --shape ref       # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/cheb_bench.py --shape ecoli     # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/cheb_bench.py --kernel          # gcnx_cheb_sum and gcnx_cheb_basis alone at f = 64, K in {2, 3, 4, 5}, on both
                                                 # batch shapes and on 8 ecoli graphs (the under-filled case): the library's
                                                 # choice, the resident route forced at every column block that fits, the
                                                 # streamed route forced, and K - 1 calls of gcnx_spmm_csr on the same operator
                                                 # and width (the floor: the same gathers without the recurrence)

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
from gcnx import _lib, device as D, synth  # noqa: E402
from gcnx.device import DeviceCSR  # noqa: E402
from gcn_bn_bench import host_batch  # noqa: E402
from sage_bench import alternate, device_batch, stats  # noqa: E402


def bench_step(ctx, args):
    hb = host_batch(args.shape)
    batch = device_batch(ctx, hb)
    models = {}
    for name, knob in (("cheb_resident", "1"), ("cheb_streamed", "0")):
        os.environ["GCNX_CHEB_RESIDENT"] = knob             # read once, at construction
        models[name] = gcnx.Cheb(ctx, hidden_channels=64, K=args.k, seed=0)
    models["gcn"] = gcnx.GCN(ctx, hidden_channels=64, seed=0)
    models["appnp"] = gcnx.APPNP(ctx, hidden_channels=64, K=10, alpha=0.1, seed=0)
    ms = alternate(ctx, {k: (lambda m=m: m.train_step(batch, lr=1e-3, fetch=False)) for k, m in models.items()},
                   args.steps, args.rounds, args.warmup)
    loss = {k: m.fetch_metrics(hb.n_graphs)[0] for k, m in models.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"model": "gcnx.Cheb", "K": args.k, "lambda_max": 2.0, "shape": args.shape, "n_nodes": int(hb.n), "n_graphs": int(hb.n_graphs),
            "max_graph_rows": int(np.diff(hb.graph_ptr).max()), "f_in": 16, "hidden": 64, "steps_per_window": args.steps,
            "rounds": args.rounds, "train_step": {k: stats(v) for k, v in ms.items()},
            "resident_over_gcn": round(med["cheb_resident"] / med["gcn"], 3),
            "streamed_over_gcn": round(med["cheb_streamed"] / med["gcn"], 3),
            "resident_over_appnp": round(med["cheb_resident"] / med["appnp"], 3),
            "graphs_per_s_resident": round(hb.n_graphs / med["cheb_resident"] * 1e3, 1),
            "finite": bool(all(np.isfinite(v) for v in loss.values()))}


def bench_kernel(ctx, args):
    res = []
    f = 64
    for shape, hb in (("ref", host_batch("ref")), ("ecoli", host_batch("ecoli")), ("ecoli8", synth.ecoli_batch(8, 16))):
        a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr).cheb_norm()
        n = hb.n
        rng = np.random.default_rng(0)
        x = ctx.to_device(rng.standard_normal((n, f)).astype(np.float32))
        bias = ctx.to_device(rng.standard_normal(f).astype(np.float32))
        out, scratch, tmp = ctx.empty((n, f)), ctx.empty((n * f,)), ctx.empty((n, f))
        for k in (2, 3, 4, 5):
            h, panel = ctx.to_device(rng.standard_normal((n, k * f)).astype(np.float32)), ctx.empty((n, k * f))

            def spmm_k(k=k):
                src, dst = x, out
                for _ in range(k - 1):
                    D.spmm(ctx, a, src, None, dst)
                    src, dst = dst, (tmp if dst is out else out)

            calls = {"sum": lambda cb, k=k, h=h: D.cheb_sum(ctx, a, h, bias, out, k, 2.0, scratch=scratch, col_block=cb),
                     "basis": lambda cb, k=k, panel=panel: D.cheb_basis(ctx, a, x, panel, k, 2.0, col_block=cb)}
            fns = {f"spmm_x{k - 1}": spmm_k}
            for what, call in calls.items():
                fns[f"{what}_library"] = lambda call=call: call(0)
                fns[f"{what}_streamed"] = lambda call=call: call(-1)
                for cb in (64, 32, 16, 8, 4):
                    try:
                        call(cb)
                    except _lib.GcnxError as e:
                        if e.code != _lib.ERR_UNSUPPORTED:
                            raise
                        continue
                    fns[f"{what}_resident_cb{cb}"] = lambda call=call, cb=cb: call(cb)
            ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
            res.append({"shape": shape, "n_nodes": int(n), "n_graphs": int(hb.n_graphs), "nnz": int(hb.nnz),
                        "max_graph_rows": int(np.diff(hb.graph_ptr).max()), "f": f, "K": k, **{key: stats(v) for key, v in ms.items()}})
    return {"kernel": "gcnx_cheb_sum / gcnx_cheb_basis", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("ref", "ecoli"), default="ref")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--k", type=int, default=3, help="terms of the model's two convolutions")
    ap.add_argument("--steps", type=int, default=200, help="steps (calls) per timed window")
    ap.add_argument("--rounds", type=int, default=7, help="windows per candidate")
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    ctx = gcnx.Context(0)
    print(json.dumps(bench_kernel(ctx, args) if args.kernel else bench_step(ctx, args)))
    ctx.close()


if __name__ == "__main__":
    main()
