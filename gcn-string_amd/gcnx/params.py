"""How stacked weights are stored and named, once for the layers and the models (host arithmetic only).

A *stacked* tensor is one stored tensor whose column blocks (for a bias: slices) carry names: ``block_views`` hands the blocks
out as views, ``join_blocks`` concatenates named host arrays back into the stacked one.  ``to_pyg`` / ``from_pyg`` convert
between the stored layouts and PyG's: a ``.weight`` is stored [in, out] and is [out, in] in PyG, some keys carry a leading axis
of 1 there, and ResGatedGraphConv's key / query / value weights are [node block ‖ edge block] there."""
import numpy as np


def block_views(stacked, blocks):
    """{name: view} of the blocks of ``stacked`` ([rows, columns]: column blocks; [n]: slices), for a parameter and its gradient
    alike.  ``blocks``: (name, width) in storage order; a name of None is a block nobody reads by name."""
    views, c = {}, 0
    for name, w in blocks:
        if name is not None:
            views[name] = stacked.cols(c, c + w) if len(stacked.shape) == 2 else stacked.flat(c, w)
        c += w
    return views


def join_blocks(host, names):
    """The inverse: the host arrays ``names`` taken out of ``host`` and concatenated into the stacked one.  An int among the
    names is an unnamed block of that many zeros (a bias)."""
    return np.concatenate([np.zeros(n, np.float32) if isinstance(n, int) else host.pop(n) for n in names], axis=-1)


def to_pyg(t, keys, leading=(), edge=None):
    """{PyG name: array in PyG's layout} of the stored tensors ``t`` (parameters or gradients).  ``keys``: (PyG name, key in t,
    transposed); ``leading``: the PyG names that get a leading axis of 1; ``edge``: {PyG name: key of its edge block}, joined
    behind the node block."""
    d = {tk: (t[k].numpy().T.copy() if tr else t[k].numpy()) for tk, k, tr in keys}
    d.update({tk: d[tk][None] for tk in leading})
    for tk, ke in (edge or {}).items():
        d[tk] = np.concatenate([d[tk], t[ke].numpy().T], axis=1)
    return d


def from_pyg(d, keys, shapes, who, leading=(), edge=None, edge_dim=0, misfit=None):
    """The inverse, checked: {key: array in the stored layout} of a PyG-layout dict.  A missing key raises KeyError naming all
    that are missing; an array that does not give the stored shape ``shapes[key]`` raises ValueError with the text of
    ``misfit(PyG name, array in the stored layout, stored shape)`` (default: the model's, which names the shape as given).  With
    ``edge`` the last ``edge_dim`` stored rows of those weights go to the edge block's key."""
    missing = [tk for tk, _, _ in keys if tk not in d]
    if missing:
        raise KeyError(f"{who}.load_state_dict: missing {missing}")
    misfit = misfit or (lambda tk, v, want: f"{tk}: shape {np.asarray(d[tk]).shape} does not fit this model")
    host, edge = {}, edge or {}
    for tk, k, tr in keys:
        v = np.asarray(d[tk], np.float32)
        if tk in leading and v.ndim == len(shapes[k]) + 1 and v.shape[0] == 1:
            v = v[0]
        v, want = v.T if tr else v, tuple(shapes[k])
        if tk in edge and v.ndim == 2 and v.shape[0] > edge_dim:
            host[edge[tk]], v = v[-edge_dim:], v[:-edge_dim]
        elif tk in edge:
            want = None                                   # no edge block to split off: nothing fits
        if v.shape != want:
            raise ValueError(misfit(tk, v, tuple(shapes[k])))
        host[k] = v
    return host
