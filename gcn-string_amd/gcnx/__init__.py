"""gcnx -- MI355X-native GCN forward/backward for DisjointLoader batches.

Host mirror of the Spektral call surface used by Sum02dean/GCN-STRING's src/scripts/gcn.py
(DisjointLoader, GCNConv, GlobalSumPool, model(inputs, training=), train_step) over
hand-written HIP kernels in libgcnx.so (C ABI: include/gcnx.h), bound with ctypes.
No PyTorch, no TensorFlow, no CPU fallback.
"""
from . import _lib
from .optim import SGD, Adam
from .io import best_epoch, load_weights_npz, save_to_npz
from .loader import Dataset, DisjointLoader, Graph, ListDataset, NetworkxDataset, SparseTensor, entry_edge_features, format_graph, from_networkx
from .train import PiecewiseConstantDecay, auc, binary_acc, fit, roc_curve

__all__ = ["Dataset", "DisjointLoader", "Graph", "ListDataset", "NetworkxDataset", "from_networkx", "entry_edge_features", "format_graph", "SparseTensor", "Context", "default_context", "GCNConv", "GeneralConv",
           "ECCConv", "SAGEConv", "GINConv", "GINEConv", "PDNConv", "APPNPConv", "ChebConv", "RGCNConv", "PNAConv", "GATConv", "GATv2Conv", "ResGatedGraphConv", "TransformerConv", "TopKPool", "GlobalSumPool", "GlobalAvgPool", "GlobalMaxPool", "GlobalAttnSumPool", "Dense", "BatchNorm1d", "GraphNorm", "PReLU", "GCN2", "GCN", "SAGE", "GIN", "GINE", "PDN", "APPNP", "Cheb", "RGCN", "PNA", "GAT", "GATv2", "ResGated", "Transformer", "GeneralGNN", "ECCNet", "TopKNet", "DeviceBatch", "Explainer", "Explanation",
           "save_to_npz", "load_weights_npz", "best_epoch", "DeviceDataset", "DeviceDisjointLoader",
           "PiecewiseConstantDecay", "Adam", "SGD", "fit", "roc_curve", "auc", "binary_acc"]


def __getattr__(name):  # device-side names load libgcnx lazily, host-only use needs no .so
    if name in ("Context", "default_context", "DeviceArray", "DeviceCSR", "Segments"):
        from . import device
        return getattr(device, name)
    if name in ("GCNConv", "GeneralConv", "ECCConv", "SAGEConv", "GINConv", "GINEConv", "PDNConv", "APPNPConv", "ChebConv", "RGCNConv", "PNAConv", "GATConv", "GATv2Conv", "ResGatedGraphConv", "TransformerConv", "TopKPool", "GlobalSumPool", "GlobalAvgPool", "GlobalMaxPool", "GlobalAttnSumPool", "Dense", "BatchNorm1d", "GraphNorm", "PReLU"):
        from . import layers
        return getattr(layers, name)
    if name in ("DeviceDataset", "DeviceDisjointLoader", "collate_on_device"):
        from . import device_loader
        return getattr(device_loader, name)
    if name in ("GCN2", "GCN", "SAGE", "GIN", "GINE", "PDN", "APPNP", "Cheb", "RGCN", "PNA", "GAT", "GATv2", "ResGated", "Transformer", "GeneralGNN", "ECCNet", "TopKNet", "DeviceBatch", "evaluate"):
        from . import models
        return getattr(models, name)
    if name in ("Explainer", "Explanation"):
        from . import explain
        return getattr(explain, name)
    raise AttributeError(name)
