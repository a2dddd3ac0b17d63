#!/usr/bin/env python3
"""gcnx.ECCNet (ECCConv on the DCA / proximity edge features) train_step timing, and the two gathers of csrc/ecc.hip next to the
same results composed from gcnx_spmm_csr -- how the layer could be built without a new kernel, so that is the bar.

  python scripts/ecc_bench.py --shape ref                        # 50 tiny graphs, F_in 16 (gcn.py:297)
  python scripts/ecc_bench.py --shape ecoli --channels 64        # config-2 batch shape: synth.ecoli_batch(f=16)
  python scripts/ecc_bench.py --shape ecoli --kernel-network 8   # one hidden Dense(8, relu) in the kernel network

Edge features: two synthetic channels per stored entry, equal in both directions of an edge (as dca / proximity are).
HIP events after warm-up.  The kernel comparison alternates the two forms in one process, round after round, and reports the
median of the rounds with their spread (min .. max); C = S' + 1 channels (S' = 2, or the kernel network's width):

  expand    gcnx_ecc_expand                 vs   C x gcnx_spmm_csr on the destination-side CSR, one value array per channel,
                                                 each writing its F columns of Scat
  bwd (dx)  gcnx_ecc_bwd, dx (+ du with a   vs   C x gcnx_spmm_csr on the batch CSR into a scratch + (C - 1) x gcnx_add
            kernel network)                      (no existing kernel composes du: that side is dx only)

for the two layer widths of the model (F = 16 and F = channels).  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gcn-string_amd"))

import numpy as np  # noqa: E402

import gcnx  # noqa: E402
from gcnx import device as D  # noqa: E402
from gcnx import synth  # noqa: E402
from gcnx.device import DeviceCSR, Segments  # noqa: E402
from gcnx.models import DeviceBatch  # noqa: E402


def host_batch(shape):
    if shape == "ecoli":
        return synth.ecoli_batch(f=16)
    import scipy.sparse as sp
    raw = synth.tiny_graphs(50, 16, seed=0)
    a = sp.block_diag([g[1] for g in raw], format="csr")
    a.sort_indices()
    gp = np.concatenate([[0], np.cumsum([g[0].shape[0] for g in raw])]).astype(np.int32)
    return synth.HostBatch(np.concatenate([g[0] for g in raw]).astype(np.float32), a.indptr.astype(np.int32),
                           a.indices.astype(np.int32), None, gp, np.stack([g[2] for g in raw]).astype(np.float32))


def edge_features(hb, channels=2, seed=0):
    """[nnz, channels] in (0, 1), one row per stored entry, the same row for (r, c) and (c, r)."""
    rows = np.repeat(np.arange(hb.n, dtype=np.int64), np.diff(hb.rowptr))
    cols = hb.colidx.astype(np.int64)
    _, inv = np.unique(np.minimum(rows, cols) * hb.n + np.maximum(rows, cols), return_inverse=True)
    return np.random.default_rng(seed).random((int(inv.max()) + 1, channels), dtype=np.float32)[inv]


def timed(ctx, fn, reps):
    e0 = ctx.event().record()
    for _ in range(reps):
        fn()
    e1 = ctx.event().record()
    return e1.elapsed_ms_since(e0) / reps * 1e3          # microseconds per call


def ab(ctx, new, old, rounds, reps):
    for fn in (new, old):
        for _ in range(10):
            fn()
    ctx.sync()
    t = {"new": [], "spmm": []}
    for _ in range(rounds):
        t["new"].append(timed(ctx, new, reps))
        t["spmm"].append(timed(ctx, old, reps))
    return {k: {"us": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in t.items()}


def kernel_ab(ctx, a, f, u, with_du, rounds, reps, seed=0):
    n, nnz, sp = a.n, a.nnz, u.shape[1]
    c = sp + 1
    rng = np.random.default_rng(seed)
    x = ctx.to_device(rng.standard_normal((n, f), dtype=np.float32))
    dscat = ctx.to_device(rng.standard_normal((n, c * f), dtype=np.float32))
    scat, scat2, dx, dx2, tmp = ctx.empty((n, c * f)), ctx.empty((n, c * f)), ctx.empty((n, f)), ctx.empty((n, f)), ctx.empty((n, f))
    du = ctx.empty((nnz, sp)) if with_du else None
    rp_t, ci_t, pm = a.transpose_perm()
    uh, perm = u.numpy(), pm.numpy()[:nnz]
    fwd_ops = [DeviceCSR(ctx, n, nnz, rp_t, ci_t, ctx.to_device(np.ascontiguousarray(uh[perm, k])) if k < sp else None,
                         a.block_ptr, a.n_blocks, False, a.max_block_rows) for k in range(c)]
    bwd_ops = [DeviceCSR(ctx, n, nnz, a.rowptr, a.colidx, ctx.to_device(np.ascontiguousarray(uh[:, k])) if k < sp else None,
                         a.block_ptr, a.n_blocks, False, a.max_block_rows) for k in range(c)]

    def fwd_spmm():
        for k, op in enumerate(fwd_ops):
            D.spmm(ctx, op, x, None, scat2.cols(k * f, (k + 1) * f))

    def bwd_spmm():
        D.spmm(ctx, bwd_ops[0], dscat.cols(0, f), None, dx2)
        for k in range(1, c):
            D.spmm(ctx, bwd_ops[k], dscat.cols(k * f, (k + 1) * f), None, tmp)
            D.add(ctx, dx2, tmp, dx2)
    out = {"F": f, "C": c,
           "expand": ab(ctx, lambda: D.ecc_expand(ctx, a, u, x, scat), fwd_spmm, rounds, reps),
           "bwd": ab(ctx, lambda: D.ecc_bwd(ctx, a, u, x, dscat, None, dx, du), bwd_spmm, rounds, reps)}
    out["bwd"]["new_writes_du"] = bool(with_du)
    ref, got = scat2.numpy(), scat.numpy()                 # the two forms computed the same thing
    out["expand"]["max_abs_diff"] = float(np.abs(ref - got).max())
    out["bwd"]["max_abs_diff"] = float(np.abs(dx2.numpy() - dx.numpy()).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("ref", "ecoli"), default="ref")
    ap.add_argument("--channels", type=int, choices=(32, 64), default=32)
    ap.add_argument("--kernel-network", choices=("none", "8"), default="none")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    kn = None if args.kernel_network == "none" else [int(args.kernel_network)]
    hb = host_batch(args.shape)
    e = edge_features(hb)
    ctx = gcnx.Context(0)
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr)
    batch = DeviceBatch(ctx, ctx.to_device(hb.x), a, Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y), ctx.to_device(e))
    m = gcnx.ECCNet(ctx, 2, channels=args.channels, kernel_network=kn, seed=0)
    for _ in range(args.warmup):
        m.train_step(batch, lr=1e-3, fetch=False)
    ctx.sync()
    e0 = ctx.event().record()
    for _ in range(args.steps):
        m.train_step(batch, lr=1e-3, fetch=False)
    e1 = ctx.event().record()
    ms = e1.elapsed_ms_since(e0) / args.steps
    loss, acc = m.fetch_metrics(hb.n_graphs)
    # the kernels on the operands of the two layers: u = e, or the kernel network's output on e
    u = batch.e if kn is None else m.conv1._saved[2][-1]
    kernels = [kernel_ab(ctx, a, f, u, kn is not None, args.rounds, args.reps) for f in (16, args.channels)]
    print(json.dumps({"model": "gcnx.ECCNet", "shape": args.shape, "n_nodes": int(hb.n), "n_graphs": int(hb.n_graphs),
                      "nnz": int(a.nnz), "f_in": 16, "channels": args.channels, "kernel_network": kn,
                      "ms_per_step": round(ms, 5), "graphs_per_s": round(hb.n_graphs / ms * 1e3, 1), "steps": args.steps,
                      "loss": round(loss, 6), "finite": bool(np.isfinite(loss)), "kernels": kernels}))
    ctx.close()


if __name__ == "__main__":
    main()
