#!/usr/bin/env python3
"""gcnx.GIN train_step and gcnx_gin_conv timing with HIP events after warm-up; the one-launch route against the composed route
(GCNX_GIN_FUSED=0: gcnx_gin_aggregate + gcnx_gemm(relu) + gcnx_gemm, gcnx_gemm_dx + gcnx_gin_aggregate) and against gcnx.SAGE
in the SAME process, alternated window by window.

  python scripts/gin_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/gin_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/gin_bench.py --kernel         # gcnx_gin_conv alone (both stages with t and u; single stage, transposed) at
                                               # 16 -> 64 -> 64 and 64 -> 64 -> 64 on both batch shapes, against the calls that
                                               # produce the same arrays; + the algorithmic bytes of the one-launch forms

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
    models = {}
    for name, knob, te in (("one_launch", "1", False), ("composed", "0", False), ("one_launch_train_eps", "1", True),
                           ("composed_train_eps", "0", True)):
        os.environ["GCNX_GIN_FUSED"] = knob                 # read once, at construction
        models[name] = gcnx.GIN(ctx, hidden_channels=64, train_eps=te, seed=0)
    models["sage"] = gcnx.SAGE(ctx, hidden_channels=64, seed=0)
    ms = alternate(ctx, {k: (lambda m=m: m.train_step(batch, lr=1e-3, fetch=False)) for k, m in models.items()},
                   args.steps, args.rounds, args.warmup)
    loss = {k: m.fetch_metrics(hb.n_graphs)[0] for k, m in models.items()}
    return {"model": "gcnx.GIN", "shape": args.shape, "n_nodes": int(hb.n), "n_graphs": int(hb.n_graphs), "f_in": 16, "hidden": 64,
            "steps_per_window": args.steps, "rounds": args.rounds, "train_step": {k: stats(v) for k, v in ms.items()},
            "graphs_per_s_one_launch": round(hb.n_graphs / float(np.median(ms["one_launch"])) * 1e3, 1),
            "graphs_per_s_composed": round(hb.n_graphs / float(np.median(ms["composed"])) * 1e3, 1),
            "finite": bool(all(np.isfinite(v) for v in loss.values()))}


def conv_bytes(n, nnz, k0, k1, k2, keep):
    """Bytes the one-launch call has to move once: CSR, x (own rows; the gathered rows count once: they are the same array),
    the weights and biases, out, and t / u when kept."""
    b = 4 * (n + 1 + nnz) + 4 * n * k0 + 4 * (k0 * k1 + k1 + k1 * k2 + k2) + 4 * n * (k2 or k1)
    return b + (4 * n * (k0 + (k1 if k2 else 0)) if keep else 0)


def bench_kernel(ctx, args):
    res = []
    for shape in ("ref", "ecoli"):
        hb = host_batch(shape)
        a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr).unweighted()
        a_t = a.transpose()
        n = hb.n
        rng = np.random.default_rng(0)
        for k0, h in ((16, 64), (64, 64)):
            dev = lambda *s: ctx.to_device(rng.standard_normal(s).astype(np.float32))
            x, du, wa, ba, wb, bb, eps = dev(n, k0), dev(n, h), dev(k0, h), dev(h), dev(h, h), dev(h), ctx.to_device(np.full(1, 0.1, np.float32))
            out, t, u, dx, dt = ctx.empty((n, h)), ctx.empty((n, k0)), ctx.empty((n, h)), ctx.empty((n, k0)), ctx.empty((n, k0))

            def fwd_composed():
                D.gin_aggregate(ctx, a, x, eps, t)
                D.gemm(ctx, t, wa, ba, u, act="relu")
                D.gemm(ctx, u, wb, bb, out)

            def bwd_composed():
                D.gemm_dx(ctx, du, wa, dt)
                D.gin_aggregate(ctx, a_t, dt, eps, dx)

            fns = {"fwd_one_launch": lambda: D.gin_conv(ctx, a, x, eps, wa, ba, wb, bb, out, t=t, u=u), "fwd_composed": fwd_composed,
                   "bwd_composed": bwd_composed}
            if D.gin_conv_ok(ctx, n, h, k0, 0):
                fns["bwd_one_launch"] = lambda: D.gin_conv(ctx, a_t, du, eps, wa, None, None, None, dx, w_transposed=True)
            ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
            res.append({"shape": shape, "n_nodes": int(n), "nnz": int(hb.nnz), "k0": k0, "k1": h, "k2": h,
                        "fwd_bytes": conv_bytes(n, hb.nnz, k0, h, h, True), "bwd_bytes": conv_bytes(n, hb.nnz, h, k0, 0, False),
                        **{k: stats(v) for k, v in ms.items()}})
    return {"kernel": "gcnx_gin_conv", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


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
