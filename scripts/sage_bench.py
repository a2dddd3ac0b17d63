#!/usr/bin/env python3
"""gcnx.SAGE train_step and gcnx_sage_conv timing with HIP events after warm-up; the one-launch route against the composed
route (GCNX_SAGE_FUSED=0: gcnx_spmm_csr + gcnx_gemm x 2 + gcnx_add, gcnx_gemm_dx + gcnx_spmm_csr + gcnx_gemm_dx) in the SAME
process, alternated window by window.

  python scripts/sage_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/sage_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/sage_bench.py --kernel         # gcnx_sage_conv alone (forward with s, transposed backward) at 16 -> 64 and
                                                # 64 -> 64 on both batch shapes, against the calls that produce the same arrays

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
from gcnx.device import DeviceCSR, Segments  # noqa: E402
from gcnx.models import DeviceBatch  # noqa: E402
from gcn_bn_bench import host_batch  # noqa: E402


def window(ctx, fn, iters):
    """ms per call of fn over one window of `iters` calls (HIP events; elapsed_ms_since waits for the second)."""
    e0 = ctx.event().record()
    for _ in range(iters):
        fn()
    e1 = ctx.event().record()
    return e1.elapsed_ms_since(e0) / iters


def alternate(ctx, fns, iters, rounds, warmup):
    """{name: [ms per call of every window]}: the candidates take turns, window by window."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ctx.sync()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(window(ctx, fn, iters))
    return out


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 5), "min_ms": round(float(np.min(ms)), 5), "max_ms": round(float(np.max(ms)), 5)}


def device_batch(ctx, hb):
    return DeviceBatch(ctx, ctx.to_device(hb.x), DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr),
                       Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y))


def bench_step(ctx, args):
    hb = host_batch(args.shape)
    batch = device_batch(ctx, hb)
    models = {}
    for name, knob in (("one_launch", "1"), ("composed", "0")):
        os.environ["GCNX_SAGE_FUSED"] = knob                # read once, at construction
        models[name] = gcnx.SAGE(ctx, hidden_channels=64, seed=0)
    ms = alternate(ctx, {k: (lambda m=m: m.train_step(batch, lr=1e-3, fetch=False)) for k, m in models.items()},
                   args.steps, args.rounds, args.warmup)
    loss = {k: m.fetch_metrics(hb.n_graphs)[0] for k, m in models.items()}
    return {"model": "gcnx.SAGE", "shape": args.shape, "n_nodes": int(hb.n), "n_graphs": int(hb.n_graphs), "f_in": 16, "hidden": 64,
            "steps_per_window": args.steps, "rounds": args.rounds, "train_step": {k: stats(v) for k, v in ms.items()},
            "graphs_per_s_one_launch": round(hb.n_graphs / float(np.median(ms["one_launch"])) * 1e3, 1),
            "finite": bool(all(np.isfinite(v) for v in loss.values()))}


def bench_kernel(ctx, args):
    res = []
    for shape in ("ref", "ecoli"):
        hb = host_batch(shape)
        a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr)
        a_mean = a.unweighted().row_mean()
        a_t = a_mean.transpose()
        n = hb.n
        rng = np.random.default_rng(0)
        for fi, fo in ((16, 64), (64, 64)):
            dev = lambda *s: ctx.to_device(rng.standard_normal(s).astype(np.float32))
            x, dz, wl, wr, b = dev(n, fi), dev(n, fo), dev(fi, fo), dev(fi, fo), dev(fo)
            out, s, h, dx, t = ctx.empty((n, fo)), ctx.empty((n, fi)), ctx.empty((n, fo)), ctx.empty((n, fi)), ctx.empty((n, fi))

            def fwd_composed():
                D.spmm(ctx, a_mean, x, None, s)
                D.gemm(ctx, s, wl, b, out)
                D.gemm(ctx, x, wr, None, h)
                D.add(ctx, out, h, out)

            def bwd_composed():
                D.gemm_dx(ctx, dz, wl, t)
                D.spmm(ctx, a_t, t, None, dx)
                D.gemm_dx(ctx, dz, wr, dx, accumulate=True)

            ms = alternate(ctx, {"fwd_one_launch": lambda: D.sage_conv(ctx, a_mean, x, wl, wr, b, out, s=s),
                                 "fwd_composed": fwd_composed,
                                 "bwd_one_launch": lambda: D.sage_conv(ctx, a_t, dz, wl, wr, None, dx, w_transposed=True),
                                 "bwd_composed": bwd_composed}, args.steps, args.rounds, args.warmup)
            res.append({"shape": shape, "n_nodes": int(n), "nnz": int(hb.nnz), "fi": fi, "fo": fo, **{k: stats(v) for k, v in ms.items()}})
    return {"kernel": "gcnx_sage_conv", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


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
