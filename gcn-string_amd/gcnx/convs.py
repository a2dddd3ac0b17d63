"""The launch sequences of the convolutions that a layer (gcnx.layers) and a model (gcnx.models) both run: PNAConv, GATConv,
GATv2Conv, ResGatedGraphConv, TransformerConv, GINEConv, PDNConv (with the GCNConv sequence it is built on), APPNPConv,
ChebConv and RGCNConv.  This is the one place they are written down.

One forward and one backward function per convolution, plain functions over operands: ``ctx``, the pattern, the operands, the
parameter views, the gradient views, every scratch and output buffer, then the scalars.  The caller owns the storage, the
shape checks (``*_conv_ok``) and the scratch sizes (``*_scratch_floats``); nothing here allocates, looks a name up or
validates.  An optional operand is ``None`` and drops exactly its launch or argument: no ``bias``, no ``e`` / ``w_e`` /
``g_w_e``, ``alpha`` / ``o_pre`` not kept (a forward no backward follows), no ``w_beta``, ``dx`` not wanted.  Weights are
stored [in, out].  ``h`` below is the convolution's output width (heads * channels); whether a stacked P = ... | S carries the
root block S is read off its width (4 h, or 3 h without root_weight).

SAGEConv and GINConv are not here: layer and model choose their one-launch route by different predicates.  GINEConv's and
RGCNConv's two routes are here; the caller decides between them (``one_launch``) by its own predicate."""
from __future__ import annotations

from . import device as D


# ---- PNAConv -----------------------------------------------------------------------------------------------------------------
def pna_forward(ctx, a, x, w_pre, b_pre, w_post, b_post, w_lin, b_lin, delta, pq, c, stats, t, out):
    """pq = P | Q, c = the 13 blocks, t = C W_post + b_post, out = t W_lin + b_lin.  stats None: no backward follows."""
    f = x.shape[1]
    D.gemm(ctx, x, w_pre.flat(0, f * f, (f, f)), b_pre, pq.cols(0, f))                      # P = x W_pre[:F] + b_pre
    D.gemm(ctx, x, w_pre.flat(f * f, f * f, (f, f)), None, pq.cols(f, 2 * f))               # Q = x W_pre[F:]
    D.pna_aggregate(ctx, a, x, pq, delta, c, stats)
    D.gemm(ctx, c, w_post, b_post, t)
    D.gemm(ctx, t, w_lin, b_lin, out)


def pna_backward(ctx, a, a_t, x, pq, c, stats, t, dz, w_pre, w_post, w_lin, g_w_pre, g_b_pre, g_w_post, g_b_post, g_w_lin, g_b_lin,
                 delta, dt, dc, dpq, coef, dx):
    """From dz = dLoss / dout: every parameter gradient, and into dx (None: not needed) the gradient of the layer's input.
    dt [n, H], dc [n, 13F], dpq [n, 2F] and coef (pna_bwd_scratch_floats) are scratch."""
    f = x.shape[1]
    if g_b_lin is not None:
        D.act_bias_grad(ctx, dz, None, dz, None, db=g_b_lin)                               # db_lin: column sums of dZ
    D.gemm_dx(ctx, dz, w_lin, dt, db=g_b_post)                                             # dT = dZ W_lin^T, db_post
    D.gemm_dw2(ctx, t, dz, g_w_lin, c, dt, g_w_post)                                       # dW_lin = T^T dZ, dW_post = C^T dT
    D.gemm_dx(ctx, dt, w_post, dc)                                                         # dC = dT W_post^T
    D.pna_bwd(ctx, a, a_t, pq, stats, dc, delta, dpq, coef)                                # dP | dQ (block 0 of dC untouched)
    dp, dq = dpq.cols(0, f), dpq.cols(f, 2 * f)
    if g_b_pre is not None:
        D.act_bias_grad(ctx, dp, None, dp, None, db=g_b_pre)                               # db_pre: column sums of dP
    g_top, g_bot = g_w_pre.flat(0, f * f, (f, f)), g_w_pre.flat(f * f, f * f, (f, f))
    if f % 4 == 0:
        D.gemm_dw2(ctx, x, dp, g_top, x, dq, g_bot)                                        # dW_pre = x^T [dP | dQ]
    else:                                       # (the lower half starts off a 16-byte boundary: one launch each)
        D.gemm_dw(ctx, x, dp, g_top)
        D.gemm_dw(ctx, x, dq, g_bot)
    if dx is not None:                          # dx = dC[:, :F] + dP W_pre[:F]^T + dQ W_pre[F:]^T
        D.gemm_dx(ctx, dp, w_pre.flat(0, f * f, (f, f)), dx)
        D.gemm_dx(ctx, dq, w_pre.flat(f * f, f * f, (f, f)), dx, accumulate=True)
        D.add(ctx, dx, dc.cols(0, f), dx)


# ---- GATConv -----------------------------------------------------------------------------------------------------------------
def gat_forward(ctx, a, x, w, att_src, att_dst, bias, hf, asrc, adst, alpha, o_pre, out, slope):
    """hf = x W, the score halves asrc / adst [n, heads], then the softmax-weighted gather into out (+ bias).  alpha
    [nnz, heads] and o_pre (out before the bias) are what the backward reads."""
    D.gemm(ctx, x, w, None, hf)
    D.gat_scores(ctx, hf, att_src, att_dst, asrc, adst)
    D.gat_aggregate(ctx, a, hf, asrc, adst, bias, out, alpha=alpha, o_pre=o_pre, slope=slope)


def gat_backward(ctx, a, x, hf, asrc, adst, alpha, o_pre, dz, w, att_src, att_dst, g_w, g_att_src, g_att_dst, g_bias, dscore, dadst,
                 dasrc, dhf, scratch, dx, slope):
    """From dz: the four gradients and, with dx, the gradient of the input.  a carries its transposed pattern
    (DeviceCSR.transpose_perm); dscore [nnz, heads], dadst / dasrc [n, heads], dhf [n, h], scratch (gat_bwd_scratch_floats)."""
    if g_bias is not None:
        D.act_bias_grad(ctx, dz, None, dz, None, db=g_bias)                                # column sums of dZ
    D.gat_bwd_edges(ctx, a, hf, asrc, adst, alpha, dz, o_pre, dscore, dadst, slope=slope)
    D.gat_bwd_nodes(ctx, a, alpha, dscore, dz, hf, dadst, att_src, att_dst, dhf, dasrc, g_att_src, g_att_dst, scratch)
    D.gemm_dw(ctx, x, dhf, g_w)                                                            # dW = x^T dHf
    if dx is not None:
        D.gemm_dx(ctx, dhf, w, dx)                                                         # dx = dHf W^T


# ---- GATv2Conv ---------------------------------------------------------------------------------------------------------------
def gatv2_forward(ctx, a, x, e, w, lin_bias, att, bias, w_e, xlr, alpha, o_pre, out, slope):
    """xlr = Xl | Xr = x [W_l | W_r] + [b_l | b_r] in one product, then scores, softmax and weighted sum in one launch."""
    D.gemm(ctx, x, w, lin_bias, xlr)
    D.gatv2_aggregate(ctx, a, xlr, att, bias, out, e=e, w_e=w_e, alpha=alpha, o_pre=o_pre, slope=slope)


def gatv2_backward(ctx, a, x, e, xlr, alpha, o_pre, dz, w, att, w_e, g_w, g_lin_bias, g_att, g_bias, g_w_e, dscore, dxlr, scratch,
                   dx, slope):
    """From dz: the gradients of the stacked weight and bias, att, the conv bias and W_e, and with dx the gradient of the input.
    dxlr [n, 2 h] = dXl | dXr: the forward CSR writes dXr, the transposed pattern dXl."""
    h = dz.shape[1]
    if g_bias is not None:
        D.act_bias_grad(ctx, dz, None, dz, None, db=g_bias)                                # column sums of dZ
    D.gatv2_bwd_edges(ctx, a, xlr, att, alpha, dz, o_pre, dscore, dxlr.cols(h, 2 * h), g_att, scratch, e=e, w_e=w_e, dw_e=g_w_e,
                      slope=slope)
    D.gatv2_bwd_nodes(ctx, a, xlr, att, alpha, dscore, dz, dxlr.cols(0, h), e=e, w_e=w_e, slope=slope)
    D.gemm_dw(ctx, x, dxlr, g_w)                                                           # dW_l | dW_r = x^T (dXl | dXr)
    D.act_bias_grad(ctx, dxlr, None, dxlr, None, db=g_lin_bias)                            # db_l | db_r: column sums
    if dx is not None:
        D.gemm_dx(ctx, dxlr, w, dx)                                                        # dx = dXl W_l^T + dXr W_r^T


# ---- ResGatedGraphConv -------------------------------------------------------------------------------------------------------
def resgated_forward(ctx, a, x, e, w, gemm_bias, bias, w_e, pk, out):
    """pk = K | Q | V | S = x [W_k | W_q | W_v | W_s] + gemm_bias in one product (gemm_bias: b_k | b_q | b_v and zeros under S),
    then gates, messages and their sum in one launch."""
    h, wd = out.shape[1], pk.shape[1]
    D.gemm(ctx, x, w, gemm_bias, pk)
    D.resgated_aggregate(ctx, a, pk, out, e=e, w_e=w_e, skip=pk.cols(3 * h, wd) if wd > 3 * h else None, bias=bias)


def resgated_backward(ctx, a, x, e, pk, dz, w, w_e, g_w, g_lin_bias, g_bias, g_w_e, dp, scratch, dx):
    """From dz: the gradients of the stacked weight, of b_k | b_q | b_v, of the conv bias and of the edge weight, and with dx the
    gradient of the input.  dp = dK | dQ | dV | dS as pk; scratch: resgated_bwd_scratch_floats."""
    h, wd = dz.shape[1], dp.shape[1]
    if g_bias is not None:
        D.act_bias_grad(ctx, dz, None, dz, None, db=g_bias)                                # column sums of dZ
    D.resgated_bwd_targets(ctx, a, pk, dz, dp.cols(0, h), scratch, ds=dp.cols(3 * h, wd) if wd > 3 * h else None, e=e, w_e=w_e,
                           dw_e=g_w_e)
    D.resgated_bwd_sources(ctx, a, pk, dz, dp.cols(h, 3 * h), e=e, w_e=w_e)
    D.gemm_dw(ctx, x, dp, g_w)                                                             # dW_k | dW_q | dW_v | dW_s = x^T dP
    dkqv = dp.cols(0, 3 * h)
    D.act_bias_grad(ctx, dkqv, None, dkqv, None, db=g_lin_bias)                            # db_k | db_q | db_v: column sums
    if dx is not None:
        D.gemm_dx(ctx, dp, w, dx)                                                          # dx = dP [W_k | W_q | W_v | W_s]^T


# ---- TransformerConv ---------------------------------------------------------------------------------------------------------
def transformer_forward(ctx, a, x, e, w, lin_bias, w_e, w_beta, pk, alpha, o_pre, out, heads):
    """pk = Q | K | V | S in one product, then scores, softmax, weighted sum and the root connection (with its beta gate) in one
    launch."""
    h, wd = out.shape[1], pk.shape[1]
    D.gemm(ctx, x, w, lin_bias, pk)
    D.transformer_aggregate(ctx, a, pk, out, heads, e=e, w_e=w_e, skip=pk.cols(3 * h, wd) if wd > 3 * h else None, w_beta=w_beta,
                            alpha=alpha, o_pre=o_pre)


def transformer_backward(ctx, a, x, e, pk, alpha, o_pre, dz, w, w_e, w_beta, g_w, g_lin_bias, g_w_e, g_w_beta, dp, dscore, d_o,
                         scratch, dx, heads):
    """From dz: the gradients of the stacked weight and bias, W_e and w_beta, and with dx the gradient of the input.
    dp = dQ | dK | dV | dS as pk; d_o [n, h] is needed with w_beta only: the gate's backward writes dO there and dS itself, so
    the targets' launch then reads d_o in the place of dz and is handed no ds."""
    h, wd = dz.shape[1], dp.shape[1]
    ds = dp.cols(3 * h, wd) if wd > 3 * h else None
    if w_beta is not None:
        D.transformer_beta_bwd(ctx, dz, o_pre, pk.cols(3 * h, wd), w_beta, d_o, ds, g_w_beta, scratch)
        dz, ds = d_o, None
    D.transformer_bwd_targets(ctx, a, pk, alpha, dz, o_pre, dscore, dp.cols(0, h), heads, scratch, ds=ds, e=e, w_e=w_e, dw_e=g_w_e)
    D.transformer_bwd_sources(ctx, a, pk, alpha, dscore, dz, dp.cols(h, 3 * h), heads)
    D.gemm_dw(ctx, x, dp, g_w)                                                             # dW_q | dW_k | dW_v | dW_s = x^T dP
    if g_lin_bias is not None:
        D.act_bias_grad(ctx, dp, None, dp, None, db=g_lin_bias)                            # the stacked bias: column sums
    if dx is not None:
        D.gemm_dx(ctx, dp, w, dx)                                                          # dx = dP [W_q | W_k | W_v | W_s]^T


# ---- GINEConv ----------------------------------------------------------------------------------------------------------------
def gine_forward(ctx, a, x, e, eps, w_e, b_e, w_a, b_a, w_b, b_b, t, u, out, one_launch, keep=True):
    """out = relu(T W_a + b_a) W_b + b_b, T = (1 + eps) x + sum_j relu(x_j + e_ij W_e + b_e).  one_launch: gcnx_gine_conv, which
    stores T and U = relu(T W_a + b_a) into t and u only with ``keep`` (a backward follows); otherwise the composed route, which
    passes through t and u either way."""
    if one_launch:
        D.gine_conv(ctx, a, x, eps, e, w_e, b_e, w_a, b_a, w_b, b_b, out, t=t if keep else None, u=u if keep else None)
        return
    D.gine_aggregate(ctx, a, x, eps, e, w_e, b_e, t)
    D.gemm(ctx, t, w_a, b_a, u, act="relu")
    D.gemm(ctx, u, w_b, b_b, out)


def gine_backward(ctx, a, x, e, eps, t, u, dz, w_e, b_e, w_a, w_b, g_eps, g_w_e, g_b_e, g_w_a, g_b_a, g_w_b, g_b_b, du, dt, scratch,
                  eps_parts, dx):
    """From dz: the gradients of both MLP layers, of W_e and b_e, of eps (g_eps None: eps is not trained) and, with dx, the
    gradient of the input.  a carries its transposed pattern (DeviceCSR.transpose_perm); du [n, k1] and dt [n, k0] are scratch,
    scratch: gine_bwd_scratch_floats, eps_parts: gin_eps_grad_parts (needed with g_eps only)."""
    if g_b_b is not None:
        D.act_bias_grad(ctx, dz, None, dz, None, db=g_b_b)                                 # db_b: column sums of dZ
    D.gemm_dx(ctx, dz, w_b, du, y_mask=u, db=g_b_a)                                        # dU = (dZ W_b^T) * [U > 0], db_a
    D.gemm_dw2(ctx, u, dz, g_w_b, t, du, g_w_a)                                            # dW_b = U^T dZ, dW_a = T^T dU
    D.gemm_dx(ctx, du, w_a, dt)                                                            # dT = dU W_a^T
    D.gine_bwd_edges(ctx, a, x, e, w_e, b_e, dt, g_w_e, g_b_e, scratch)                    # dW_e, db_e (forward CSR)
    if g_eps is not None:
        D.gin_eps_grad(ctx, x, dt, eps_parts, g_eps)                                       # d eps = sum <x, dT>
    if dx is not None:
        D.gine_bwd_nodes(ctx, a, x, eps, e, w_e, b_e, dt, dx)                              # dx (transposed pattern + permutation)


# ---- GCNConv (the model's sequence; PDNConv runs it on its own operator) ------------------------------------------------------
def gcn_forward(ctx, a_hat, x, w, bias, out, h_tmp, s=None):
    """out = A^ (x W) + bias.  Returns True if it ran as the one-launch (A^ x) W (then ``s``, if given, receives S = A^ x, the
    operand of dW = S^T dZ, as GCNConv.backward uses it); otherwise gcnx_gemm into h_tmp, then gcnx_spmm_csr."""
    if a_hat.plan is None and x.contiguous and D.gcn_conv_fused_ok(ctx, x.shape[0], x.shape[1], w.shape[1], x.ld):
        D.gcn_conv_fwd(ctx, a_hat, x, w, bias, out, act=None, s=s)                         # (A^ x) W + b in one launch
        return True
    D.gemm(ctx, x, w, None, h_tmp)
    D.spmm(ctx, a_hat, h_tmp, bias, out)
    return False


def gcn_backward(ctx, a_t, x, dz, w, g_w, g_bias, t, dx, s=None):
    """From dz: the bias and weight gradients and, with dx, the gradient of the input.  a_t: the transposed operator.  s: S = A^ x
    kept by a one-launch forward (with dx only): the association of GCNConv.backward, which leaves dZ W^T in t; otherwise t
    receives A^T dZ."""
    D.act_bias_grad(ctx, dz, None, dz, None, db=g_bias)                                    # column sums of dZ
    if dx is not None and s is not None:
        D.gemm_dw(ctx, s, dz, g_w)                                                         # dW = S^T dZ
        D.gemm_dx(ctx, dz, w, t)                                                           # dZ W^T
        D.spmm(ctx, a_t, t, None, dx)                                                      # dx = A^T (dZ W^T)
        return
    D.spmm(ctx, a_t, dz, None, t)                                                          # A^T dZ
    D.gemm_dw(ctx, x, t, g_w)                                                              # dW = x^T (A^T dZ)
    if dx is not None:
        D.gemm_dx(ctx, t, w, dx)                                                           # dx = (A^T dZ) W^T


# ---- PDNConv -----------------------------------------------------------------------------------------------------------------
def pdn_forward(ctx, a, a_v, a_vt, x, e, unit, w_1, b_1, w_2, b_2, w, bias, gate, r, out, h_tmp, s=None):
    """The layer's operator pair, then GCNConv on it.  a: the pattern with its transposed pattern (DeviceCSR.transpose_perm);
    a_v / a_vt: CSRs of the pattern / the transposed pattern whose value arrays receive v_e = r_i w_e r_j and v[perm_t]; gate
    [nnz] and r [n] receive the gates and deg^-1/2 (what the backward reads).  Returns gcn_forward's route flag."""
    D.pdn_operator(ctx, a, e, w_1, b_1, w_2, b_2, gate, r, a_v.vals, unit=unit, perm_t=a.transpose_perm()[2], vals_t_out=a_vt.vals)
    return gcn_forward(ctx, a_v, x, w, bias, out, h_tmp, s)


def pdn_backward(ctx, a, a_vt, x, e, unit, w_1, b_1, w_2, b_2, gate, r, dz, w, g_w, g_bias, g_w_1, g_b_1, g_w_2, g_b_2, t, tl, gv,
                 scratch, dx, s=None):
    """GCNConv's backward on the transposed operator a_vt, then G_e = <(dZ W^T)[i], x[j]> (gcnx_sddmm_csr) and the gate MLP's
    gradients.  t [n, h] as gcn_backward's; tl [n, f_in]: room for dZ W^T where gcn_backward does not leave it in t; gv [nnz];
    scratch: pdn_bwd_scratch_floats."""
    gcn_backward(ctx, a_vt, x, dz, w, g_w, g_bias, t, dx, s)
    if dx is not None and s is not None:
        tl = t                                                                             # (the one-launch association left it)
    else:
        D.gemm_dx(ctx, dz, w, tl)                                                          # dZ W^T
    D.sddmm(ctx, a, tl, x, gv)                                                             # G = dLoss/dv on the forward pattern
    D.pdn_operator_bwd(ctx, a, e, w_1, b_1, w_2, b_2, gate, r, gv, g_w_1, g_b_1, g_w_2, g_b_2, scratch, unit=unit)


# ---- APPNPConv ---------------------------------------------------------------------------------------------------------------
def appnp_forward(ctx, a, x, w, bias, h, out, k, alpha, scratch, col_block=0):
    """h = x W + bias, then out = the k hops z <- (1 - alpha) A z + alpha h from z = h.  scratch: appnp_scratch_floats (read
    by the streamed route only).  col_block: appnp_propagate's (0: the library's route, -1: streamed)."""
    D.gemm(ctx, x, w, bias, h)
    D.appnp_propagate(ctx, a, h, out, k, alpha, scratch=scratch, col_block=col_block)


def appnp_backward(ctx, a_t, x, dz, w, g_w, g_bias, dh, k, alpha, scratch, dx, col_block=0):
    """From dz: dh = P^T dz (the same hops on the transposed operator a_t), the bias gradient (its column sums), dW = x^T dh
    and, with dx, dx = dh W^T."""
    D.appnp_propagate(ctx, a_t, dz, dh, k, alpha, scratch=scratch, col_block=col_block)
    if g_bias is not None:
        D.act_bias_grad(ctx, dh, None, dh, None, db=g_bias)                                # column sums of dH
    D.gemm_dw(ctx, x, dh, g_w)                                                             # dW = x^T dH
    if dx is not None:
        D.gemm_dx(ctx, dh, w, dx)                                                          # dx = dH W^T


# ---- ChebConv ----------------------------------------------------------------------------------------------------------------
def cheb_forward(ctx, a, x, w, bias, h, out, k, lambda_max, scratch, col_block=0):
    """h = x W, W = [lins.0.weight^T | .. | lins.{k-1}.weight^T] ([in, k c]), then out = sum_j T_j(L^) H_j + bias by Clenshaw
    summation on a = S (k - 1 gathers).  scratch: cheb_scratch_floats (read by the streamed route only).  col_block:
    cheb_sum's (0: the library's route, -1: streamed)."""
    D.gemm(ctx, x, w, None, h)
    D.cheb_sum(ctx, a, h, bias, out, k, lambda_max, scratch=scratch, col_block=col_block)


def cheb_backward(ctx, a_t, x, dz, w, g_w, g_bias, g, k, lambda_max, scratch, dx, col_block=0):
    """From dz: the bias gradient (its column sums), g [n, k c] = T_j(L^^T) dz in block j (the basis on the transposed operator
    a_t, k - 1 gathers), dW = x^T g and, with dx, dx = g W^T."""
    if g_bias is not None:
        D.act_bias_grad(ctx, dz, None, dz, None, db=g_bias)                                # column sums of dZ
    D.cheb_basis(ctx, a_t, dz, g, k, lambda_max, scratch=scratch, col_block=col_block)
    D.gemm_dw(ctx, x, g, g_w)                                                              # dW = x^T G
    if dx is not None:
        D.gemm_dx(ctx, g, w, dx)                                                           # dx = G W^T


# ---- RGCNConv ----------------------------------------------------------------------------------------------------------------
def _rgcn_blocks(w, r, fi, fo, root_weight):
    """(W_rel [r fi, fo], W_root [fi, fo] or None): the two parts of the row-stacked weight, as views."""
    return w.flat(0, r * fi * fo, (r * fi, fo)), w.flat(r * fi * fo, fi * fo, (fi, fo)) if root_weight else None


def rgcn_forward(ctx, a, ops, x, w, bias, m, out, h_tmp, r, root_weight, one_launch, keep=True):
    """out = [A_0 x | .. | A_{r-1} x | x] w + bias.  a: the pattern; ops = (rel, val, rel_t, val_t) of DeviceCSR.rgcn_operator;
    w: the row-stacked [W_0; ..; W_{r-1}; W_root] (r blocks without root_weight).  one_launch: gcnx_rgcn_conv, which stores the
    panel M = [A_0 x | .. | A_{r-1} x] into m only with ``keep`` (a backward follows); otherwise the composed route:
    gcnx_rgcn_aggregate into m, gcnx_gemm over M and, with root_weight, gcnx_gemm over x into h_tmp and gcnx_add."""
    rel, val = ops[0], ops[1]
    if one_launch:
        D.rgcn_conv(ctx, a.rowptr, a.colidx, rel, val, x, w, bias, out, r, root_weight, m=m if keep else None)
        return
    fi, fo = x.shape[1], out.shape[1]
    w_rel, w_root = _rgcn_blocks(w, r, fi, fo, root_weight)
    D.rgcn_aggregate(ctx, a.rowptr, a.colidx, rel, val, x, m, r)
    D.gemm(ctx, m, w_rel, bias, out)
    if root_weight:
        D.gemm(ctx, x, w_root, None, h_tmp)
        D.add(ctx, out, h_tmp, out)


def rgcn_backward(ctx, a, ops, x, m, dz, w, g_w, g_bias, mt, r, root_weight, one_launch, dx):
    """From dz: the bias gradient (its column sums), dW_rel = M^T dz and dW_root = x^T dz (one gcnx_gemm_dw2 where the root block
    starts on a 16-byte boundary) and, with dx, dx = dz W_root^T + sum_q A_q^T (dz W_q^T): gcnx_rgcn_conv on the transposed
    pattern (a.transpose_perm()) with rel_t / val_t and the weights as stored (one_launch), or gcnx_rgcn_aggregate of dz into mt
    [n, r fo] and one gcnx_gemm_dx per block."""
    fi, fo = x.shape[1], dz.shape[1]
    w_rel, w_root = _rgcn_blocks(w, r, fi, fo, root_weight)
    g_rel, g_root = _rgcn_blocks(g_w, r, fi, fo, root_weight)
    if g_bias is not None:
        D.act_bias_grad(ctx, dz, None, dz, None, db=g_bias)                                # column sums of dZ
    if root_weight and (r * fi * fo) % 4 == 0:
        D.gemm_dw2(ctx, m, dz, g_rel, x, dz, g_root)                                       # dW_rel = M^T dZ, dW_root = x^T dZ
    else:
        D.gemm_dw(ctx, m, dz, g_rel)
        if root_weight:
            D.gemm_dw(ctx, x, dz, g_root)
    if dx is None:
        return
    rp_t, ci_t, _ = a.transpose_perm()
    rel_t, val_t = ops[2], ops[3]
    if one_launch:
        D.rgcn_conv(ctx, rp_t, ci_t, rel_t, val_t, dz, w, None, dx, r, root_weight, w_transposed=True)
        return
    D.rgcn_aggregate(ctx, rp_t, ci_t, rel_t, val_t, dz, mt, r)
    if root_weight:
        D.gemm_dx(ctx, dz, w_root, dx)                                                     # dZ W_root^T
    for q in range(r):                                                                     # + (A_q^T dZ) W_q^T
        D.gemm_dx(ctx, mt.cols(q * fo, (q + 1) * fo), w.flat(q * fi * fo, fi * fo, (fi, fo)), dx, accumulate=root_weight or q > 0)
