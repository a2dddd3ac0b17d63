#!/usr/bin/env python3
"""gcnx.TopKNet train_step and the launches of gcnx.TopKPool, timed with HIP events after warm-up; the device-side pool against
the same step with selection and slicing on the HOST -- what a user had to do before csrc/topk.hip: scores by gcnx_gemm, D2H of
y (and of p), NumPy selection, SciPy A[idx][:, idx], DeviceCSR.from_host_csr, upload of y / idx / pos -- in the SAME process,
alternated window by window.  The host route still uses gcnx_topk_gather and gcnx_topk_bwd: only the selection and the
slicing move, so the difference is the cost of those two alone.

  python scripts/topk_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/topk_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes
  python scripts/topk_bench.py --kernel         # every new launch alone, and the 4-byte read-back, on both batch shapes

Prints one JSON line.  Every figure is the median over --rounds windows with the windows' min and max beside it.  The step
lines carry a gcnx.GCN2-shaped flat step (same batch, hidden 64, eager and captured) from the same process for scale."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gcn-string_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

import gcnx  # noqa: E402
from gcnx import device as D, synth  # noqa: E402
from gcnx.device import DeviceCSR, Segments  # noqa: E402
from gcnx.layers import TopKPool  # noqa: E402
from gcnx.models import DeviceBatch  # noqa: E402
from gcn_bn_bench import host_batch  # noqa: E402
from sage_bench import alternate, stats  # noqa: E402


class HostTopKPool(TopKPool):
    """TopKPool with the selection and the induced adjacency computed on the host (NumPy / SciPy)."""

    def bind(self, layer, a_host):
        self.ctx, self.in_dim, self.built, self.params, self.grads, self.a_host = layer.ctx, layer.in_dim, True, layer.params, layer.grads, a_host
        return self

    def call(self, inputs, out=None):
        x, a, seg = inputs
        ctx, (n, f) = self.ctx, x.shape
        kp, seg2 = self._segments(seg)
        nk = int(kp[-1])
        raw = self._cap("raw", (n, 1))
        D.gemm(ctx, x, self.params["kernel"], None, raw)
        p = self.params["kernel"].numpy().ravel()                           # D2H (waits for the stream)
        y = (raw.numpy().ravel() / np.sqrt(np.sum(p * p, dtype=np.float32))).astype(np.float32)
        gp = seg.host
        idx = np.concatenate([gp[g] + np.sort(np.argsort(-y[gp[g]:gp[g + 1]], kind="stable")[:kp[g + 1] - kp[g]])
                              for g in range(seg.n_graphs)]).astype(np.int32)
        pos = np.full(n, -1, np.int32)
        pos[idx] = np.arange(nk, dtype=np.int32)
        a2h = self.a_host[idx][:, idx].tocsr()
        a2h.sort_indices()
        a2 = DeviceCSR.from_host_csr(ctx, a2h.indptr, a2h.indices, a2h.data if a.vals is not None else None, kp, symmetric=a.symmetric)
        dy, didx, dpos = self._cap("y", (n,)), self._cap("idx", (nk,), np.int32), self._cap("pos", (n,), np.int32)
        dy.copy_from_host(y); didx.copy_from_host(idx); dpos.copy_from_host(pos)
        x2 = out if out is not None else self._cap("x2", (nk, f))
        D.topk_gather(ctx, x, dy, didx, nk, x2, self.sigmoid_gating)
        self._saved = (x, dy, dpos, nk, didx)
        return x2, a2, Segments.from_device(ctx, a2.block_ptr, kp)


def device_batch(ctx, hb):
    vals = synth.gcn_norm_host(hb.rowptr, hb.colidx)
    a_host = sp.csr_matrix((vals, hb.colidx, hb.rowptr), shape=(hb.n, hb.n))
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, vals, hb.graph_ptr)
    return DeviceBatch(ctx, ctx.to_device(hb.x), a, Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y)), a_host


def bench_step(ctx, args):
    hb = host_batch(args.shape)
    batch, a_host = device_batch(ctx, hb)
    dev = gcnx.TopKNet(ctx, hidden=64, ratio=args.ratio, seed=0)
    host = gcnx.TopKNet(ctx, hidden=64, ratio=args.ratio, seed=0)
    for m in (dev, host):
        m.build(hb.f)
    host.topk = HostTopKPool(args.ratio).bind(host.topk, a_host)
    flat_eager, flat_graph = gcnx.GCN2(ctx, 2, hidden=64, use_graph=False), gcnx.GCN2(ctx, 2, hidden=64, use_graph=True)
    fns = {"device_pool": lambda: dev.train_step(batch, lr=1e-4, fetch=False),
           "host_pool": lambda: host.train_step(batch, lr=1e-4, fetch=False),
           "gcn2_flat_eager": lambda: flat_eager.train_step(batch, lr=1e-4, fetch=False),
           "gcn2_flat_captured": lambda: flat_graph.train_step(batch, lr=1e-4, fetch=False)}
    ms = alternate(ctx, fns, args.steps, args.rounds, args.warmup)
    loss = {"device_pool": dev.fetch_metrics(hb.n_graphs)[0], "host_pool": host.fetch_metrics(hb.n_graphs)[0]}
    return {"model": "gcnx.TopKNet", "shape": args.shape, "n_nodes": int(hb.n), "n_graphs": int(hb.n_graphs), "nnz": int(hb.nnz),
            "f_in": 16, "hidden": 64, "ratio": args.ratio, "n_kept": int(D.topk_kept_ptr(hb.graph_ptr, args.ratio)[-1]),
            "nnz_kept": int(dev.conv2._saved[1].nnz), "steps_per_window": args.steps, "rounds": args.rounds,
            "train_step": {k: stats(v) for k, v in ms.items()},
            "graphs_per_s_device_pool": round(hb.n_graphs / float(np.median(ms["device_pool"])) * 1e3, 1),
            "loss": {k: round(v, 6) for k, v in loss.items()}, "finite": bool(all(np.isfinite(v) for v in loss.values()))}


def bench_kernel(ctx, args):
    res = []
    for shape in ("ref", "ecoli"):
        hb = host_batch(shape)
        batch, _ = device_batch(ctx, hb)
        a, seg, n, f = batch.a, batch.seg, hb.n, 64
        rng = np.random.default_rng(0)
        x = ctx.to_device(rng.standard_normal((n, f)).astype(np.float32))
        p = ctx.to_device(rng.standard_normal(f).astype(np.float32))
        kp = D.topk_kept_ptr(hb.graph_ptr, args.ratio)
        nk = int(kp[-1])
        dkp = ctx.to_device(kp, np.int32)
        y, idx, pos = ctx.empty(n), ctx.empty(nk, np.int32), ctx.empty(n, np.int32)
        rp, ci, v = ctx.empty(nk + 1, np.int32), ctx.empty(a.nnz, np.int32), ctx.empty(a.nnz)
        x2, dxo, dx, dp = ctx.empty((nk, f)), ctx.to_device(rng.standard_normal((nk, f)).astype(np.float32)), ctx.empty((n, f)), ctx.empty(f)
        D.topk_select(ctx, seg, dkp, nk, x, p, y, idx, pos)
        ms = alternate(ctx, {"topk_select": lambda: D.topk_select(ctx, seg, dkp, nk, x, p, y, idx, pos),
                             "csr_induce": lambda: D.csr_induce(ctx, a, idx, pos, nk, rp, ci, v),
                             "topk_gather": lambda: D.topk_gather(ctx, x, y, idx, nk, x2),
                             "topk_bwd": lambda: D.topk_bwd(ctx, x, y, pos, p, dxo, dx, dp),
                             "read_nnz_4_bytes": lambda: D.read_int32(ctx, rp, nk)}, args.steps, args.rounds, args.warmup)
        res.append({"shape": shape, "n_nodes": int(n), "n_graphs": int(hb.n_graphs), "nnz": int(hb.nnz), "f": f, "ratio": args.ratio,
                    "n_kept": nk, "nnz_kept": D.read_int32(ctx, rp, nk), **{k: stats(v) for k, v in ms.items()}})
    return {"kernel": "csrc/topk.hip", "calls_per_window": args.steps, "rounds": args.rounds, "cases": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("ref", "ecoli"), default="ref")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--ratio", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=100, help="steps (calls) per timed window")
    ap.add_argument("--rounds", type=int, default=7, help="windows per candidate")
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    ctx = gcnx.Context(0)
    print(json.dumps(bench_kernel(ctx, args) if args.kernel else bench_step(ctx, args)))
    ctx.close()


if __name__ == "__main__":
    main()
