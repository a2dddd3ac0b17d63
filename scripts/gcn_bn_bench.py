#!/usr/bin/env python3
"""gcnx.GCN (the reference's torch GCN, gcn_utills.py:795-853) train_step timing with HIP events after warm-up.

  python scripts/gcn_bn_bench.py --shape ref      # synth.tiny_graphs-style batch: B = 50, F_in 16, hidden 64 (gcn.py:297)
  python scripts/gcn_bn_bench.py --shape ecoli    # config-2 batch shape: synth.ecoli_batch(f=16), 32 graphs of ~600 nodes

Prints one JSON line: ms per step, graphs/s and the GCNX_BN_POOL state (set it in the environment: 1 = fused
BN·PReLU·max-pool pair, the default; 0 = gcnx_bn_act + gcnx_segment_pool and their backward)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gcn-string_amd"))

import numpy as np  # noqa: E402

import gcnx  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("ref", "ecoli"), default="ref")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    hb = host_batch(args.shape)
    ctx = gcnx.Context(0)
    batch = DeviceBatch(ctx, ctx.to_device(hb.x), DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr),
                        Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y))
    m = gcnx.GCN(ctx, hidden_channels=64, seed=0)
    for _ in range(args.warmup):
        m.train_step(batch, lr=1e-3, fetch=False)
    ctx.sync()
    e0 = ctx.event().record()
    for _ in range(args.steps):
        m.train_step(batch, lr=1e-3, fetch=False)
    e1 = ctx.event().record()
    ms = e1.elapsed_ms_since(e0) / args.steps
    loss, acc = m.fetch_metrics(hb.n_graphs)
    print(json.dumps({"model": "gcnx.GCN", "shape": args.shape, "n_nodes": int(hb.n), "n_graphs": int(hb.n_graphs), "f_in": 16,
                      "hidden": 64, "ms_per_step": round(ms, 5), "graphs_per_s": round(hb.n_graphs / ms * 1e3, 1),
                      "GCNX_BN_POOL": int(m._bn_pool), "steps": args.steps, "loss": round(loss, 6), "finite": bool(np.isfinite(loss))}))
    ctx.close()


if __name__ == "__main__":
    main()
