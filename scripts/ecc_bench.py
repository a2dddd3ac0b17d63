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

for the two layer widths of the model (F = 16 and F = channels).  Prints one JSON line.

  python scripts/ecc_bench.py --stream --shape ref               # a NEW batch every step: 400 tiny graphs, batches of 50
  python scripts/ecc_bench.py --stream --shape ecoli             # 256 E. coli-shaped graphs, batches of 32

--stream: ms per batch of ECCNet.train_step INCLUDING the batch's assembly, fed (a) by DisjointLoader + DeviceBatch.from_host
(host vstack / block_diag, upload, and gcnx_csr_transpose_perm's download + host sort + upload per batch) and (b) by
DeviceDisjointLoader over DeviceDataset(edge_features=True) (gcnx_collate2 + gcnx_collate_edges per batch).  Both in this
process, one epoch of each per round, alternating; wall time between two synchronisations, median with min .. max of the rounds
(and the GPU's own time between two stream events).  The two models see the same batches and must end with the same weights.
Also the two collate launches alone, HIP events around --reps back-to-back calls, alternated the same way.  One JSON line."""
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


def stream_dataset(shape, n_graphs, f=16):
    """(ListDataset of Graph(x, a, e, y), batch size): the graphs of host_batch's shapes one by one, every graph with the
    edge_features of its own entries."""
    import scipy.sparse as sp
    from types import SimpleNamespace
    rng = np.random.default_rng(0)
    if shape == "ecoli":
        raw = []
        for _ in range(n_graphs):
            n, u, v = synth.ecoli_graph_pairs(rng)
            a = sp.coo_matrix((np.ones(u.size), (u, v)), shape=(n, n)).tocsr()
            y = np.zeros(2, np.float32)
            y[int(rng.integers(0, 2))] = 1
            raw.append((rng.standard_normal((n, f), dtype=np.float32), ((a + a.T + sp.identity(n)) > 0).astype(np.float32).tocsr(), y))
    else:
        raw = synth.tiny_graphs(n_graphs, f, seed=0)
    graphs = []
    for k, (x, a, y) in enumerate(raw):
        a = sp.csr_matrix(a)
        a.sort_indices()
        e = edge_features(SimpleNamespace(n=a.shape[0], rowptr=a.indptr, colidx=a.indices), seed=k)
        graphs.append(gcnx.Graph(x=np.asarray(x, np.float32), a=a, e=e, y=np.asarray(y, np.float32)))
    return gcnx.ListDataset(graphs), (32 if shape == "ecoli" else 50)


def spread(v, digits=4):
    return {"median": round(float(np.median(v)), digits), "min": round(float(min(v)), digits), "max": round(float(max(v)), digits)}


def stream(args, kn):
    import time
    from gcnx.device_loader import DeviceDataset, DeviceDisjointLoader, collate_on_device
    ds, bs = stream_dataset(args.shape, args.graphs or (256 if args.shape == "ecoli" else 400))
    ctx = gcnx.Context(0)
    dsd = DeviceDataset(ctx, ds, edge_features=True)
    epochs = args.rounds + 1                                            # the first epoch of either route is warm-up
    routes = {"host_loader": gcnx.DisjointLoader(ds, batch_size=bs, epochs=epochs, shuffle=True, seed=1),
              "device_loader": DeviceDisjointLoader(dsd, batch_size=bs, epochs=epochs, shuffle=True, seed=1)}
    models = {k: gcnx.ECCNet(ctx, 2, channels=args.channels, kernel_network=kn, seed=0) for k in routes}
    spe = routes["host_loader"].steps_per_epoch
    wall, gpu = {k: [] for k in routes}, {k: [] for k in routes}
    n_nodes = nnz = 0
    for r in range(epochs):
        for k, loader in routes.items():
            ctx.sync()
            t0, e0 = time.perf_counter(), ctx.event().record()
            for _ in range(spe):
                inputs, target = next(loader)
                batch = inputs if k == "device_loader" else DeviceBatch.from_host(ctx, inputs, target, weighted=False)
                models[k].train_step(batch, None, lr=1e-3, fetch=False)
                n_nodes, nnz = max(n_nodes, batch.n), max(nnz, batch.a.nnz)
            e1 = ctx.event().record()
            ctx.sync()
            if r:
                wall[k].append((time.perf_counter() - t0) / spe * 1e3)
                gpu[k].append(e1.elapsed_ms_since(e0) / spe)
    w = {k: m.get_weights() for k, m in models.items()}
    same = all(np.array_equal(p, q) for p, q in zip(w["host_loader"], w["device_loader"]))
    # the collate launches alone, on one full batch of the device route (its descriptor stays in the buffers)
    sel = np.arange(min(bs, len(ds)))
    batch = collate_on_device(dsd, sel)
    bufs, csr, b = batch._bufs, dsd.csr, len(sel)
    rp_t, ci_t, pm_t = dsd.tperm
    lib, vals = ctx.lib, (dsd.csr.vals.ptr if dsd.csr.vals is not None else None)

    def collate2():
        ctx._ck(lib.gcnx_collate2(ctx.h, bufs.desc.ptr, b, dsd.node_ptr.ptr, csr.rowptr.ptr, csr.colidx.ptr, vals, dsd.x.ptr, dsd.x.ld,
                                  dsd.n_features, dsd.y.ptr, dsd.n_labels, bufs.rowptr.ptr, bufs.colidx.ptr,
                                  bufs.vals.ptr if vals else None, bufs.x.ptr, bufs.x.ld, bufs.y.ptr, bufs.gp.ptr, bufs.ids.ptr,
                                  None, 0, None, 0))

    def both():
        collate2()
        ctx._ck(lib.gcnx_collate_edges(ctx.h, bufs.desc.ptr, b, dsd.node_ptr.ptr, csr.rowptr.ptr, rp_t.ptr, ci_t.ptr, pm_t.ptr,
                                       dsd.e.ptr, dsd.e.ld, dsd.n_edge_features, bufs.rowptr_t.ptr, bufs.colidx_t.ptr,
                                       bufs.perm_t.ptr, bufs.e.ptr, bufs.e.ld))
    for fn in (collate2, both):
        for _ in range(10):
            fn()
    ctx.sync()
    us = {"collate2": [], "collate2+collate_edges": []}
    for _ in range(args.rounds):
        us["collate2"].append(timed(ctx, collate2, args.reps))
        us["collate2+collate_edges"].append(timed(ctx, both, args.reps))
    med = {k: float(np.median(v)) for k, v in wall.items()}
    print(json.dumps({"model": "gcnx.ECCNet", "mode": "stream", "shape": args.shape, "graphs": len(ds), "batch_size": bs,
                      "batches_per_epoch": spe, "rounds": args.rounds, "largest_batch": {"n_nodes": int(n_nodes), "nnz": int(nnz)},
                      "f_in": 16, "edge_dim": dsd.n_edge_features, "channels": args.channels, "kernel_network": kn,
                      "ms_per_batch_wall": {k: spread(v) for k, v in wall.items()},
                      "ms_per_batch_between_stream_events": {k: spread(v) for k, v in gpu.items()},
                      "host_over_device": round(med["host_loader"] / med["device_loader"], 2),
                      "collate_us": {k: spread(v, 2) for k, v in us.items()},
                      "collate_batch": {"n_nodes": batch.n, "nnz": batch.a.nnz}, "final_weights_equal": bool(same)}))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("ref", "ecoli"), default="ref")
    ap.add_argument("--channels", type=int, choices=(32, 64), default=32)
    ap.add_argument("--kernel-network", choices=("none", "8"), default="none")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--stream", action="store_true", help="a new batch every step, host loader against device loader")
    ap.add_argument("--graphs", type=int, default=0, help="--stream: graphs in the dataset (default 400 ref / 256 ecoli)")
    args = ap.parse_args()
    kn = None if args.kernel_network == "none" else [int(args.kernel_network)]
    if args.stream:
        return stream(args, kn)
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
