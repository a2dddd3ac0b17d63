/*
 * gcnx.h -- C ABI of libgcnx.so: MI355X (gfx950) kernels for the GCN forward/backward
 * hot path of Sum02dean/GCN-STRING.
 *
 * The reference has no FFI or plugin interface for this path: its arithmetic runs inside
 * un-vendored Spektral/TensorFlow ops reached from src/scripts/gcn.py (call sites cited per
 * entry point below).  Each function here replaces one TensorFlow CPU op (SURVEY.md 2.3
 * "implicit kernel inventory" K1..K9 and their gradients) behind plain C types, so that the
 * Python host mirror of the Spektral call surface (gcn-string_amd/gcnx) binds it via ctypes.
 *
 * Conventions
 *   - every function returns int: 0 = GCNX_OK, otherwise a gcnx_status; the message is
 *     available from gcnx_last_error().  No C++ exception crosses this boundary.
 *   - all matrix operands are DEVICE pointers obtained from gcnx_malloc(), row-major fp32
 *     with an explicit leading dimension (elements) so that column slices of a wider buffer
 *     can be read/written in place (Spektral's connectivity="cat" skip, K7).
 *   - CSR: rowptr int32[N+1], colidx int32[nnz], vals fp32[nnz] or NULL (= all ones, the
 *     GeneralConv "sum" aggregation which ignores adjacency values).
 *   - a ctx is bound to one device and one HIP stream; calls are stream-ordered and return
 *     before the device finishes unless documented as synchronising.  A ctx is not
 *     thread-safe; distinct ctxs are independent.
 *   - the caller owns every buffer it allocates; the library keeps no user pointer after a
 *     call returns (captured graphs excepted: buffers used inside a capture must outlive it).
 */
#ifndef GCNX_H
#define GCNX_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define GCNX_API __attribute__((visibility("default")))
#else
#define GCNX_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gcnx_ctx gcnx_ctx;
typedef struct gcnx_comm gcnx_comm;
typedef struct gcnx_graph gcnx_graph;
typedef struct gcnx_event gcnx_event;
typedef struct gcnx_spmm_plan gcnx_spmm_plan;

typedef enum {
  GCNX_OK = 0,
  GCNX_ERR_INVALID = 1,     /* bad argument / shape / alignment */
  GCNX_ERR_HIP = 2,         /* HIP runtime error */
  GCNX_ERR_RCCL = 3,        /* RCCL error or librccl missing */
  GCNX_ERR_NOMEM = 4,
  GCNX_ERR_UNSUPPORTED = 5, /* valid request this build has no kernel for */
  GCNX_ERR_DATA = 6         /* device-side validation of input data failed */
} gcnx_status;

/* PRELU: one slope per feature, alpha[f] (Keras PReLU).  PRELU_SHARED: ONE slope alpha[0] for every feature
 * (torch.nn.PReLU(), num_parameters = 1); its gradient dalpha[0] is the sum over all features.  PRELU_SHARED is served
 * by gcnx_bn_act, gcnx_bn_act_bwd (+ _stats / _apply), gcnx_bn_act_pool(_bwd, + _stats / _apply) and gcnx_bn_prelu_bce_head
 * (+ gcnx_bce_head_phase); every other entry point that takes an activation refuses it (GCNX_ERR_INVALID). */
typedef enum { GCNX_ACT_NONE = 0, GCNX_ACT_RELU = 1, GCNX_ACT_PRELU = 2, GCNX_ACT_PRELU_SHARED = 3 } gcnx_act;
typedef enum { GCNX_POOL_SUM = 0, GCNX_POOL_AVG = 1, GCNX_POOL_MAX = 2 } gcnx_pool;
/* GEMM arithmetic: F32 = exact fp32 MFMA (v_mfma_f32_*_f32); BF16 = inputs rounded to bf16,
 * fp32 accumulate; BF16X3 = hi/lo bf16 split (16 significand bits per operand, 2^-18 relative), three MFMA passes. */
typedef enum { GCNX_PREC_F32 = 0, GCNX_PREC_BF16 = 1, GCNX_PREC_BF16X3 = 2 } gcnx_prec;
typedef enum { GCNX_NORM_SPEKTRAL = 0, GCNX_NORM_PYG = 1 } gcnx_norm_mode;
typedef enum { GCNX_RED_SUM = 0, GCNX_RED_MAX = 1 } gcnx_redop;
/* Which of Keras' two categorical_crossentropy code paths a loss entry point follows (keras.backend.
 * categorical_crossentropy, from_logits=False, as constructed at gcn.py:326):
 *   PROBS  -- the output is an EagerTensor (evaluate(), gcn.py:351-354, on TF < 2.6): p <- p / sum p, clip to
 *             [1e-7, 1 - 1e-7], -sum_c y_c log p_c; the clip passes no gradient outside its range.
 *   LOGITS -- the output is a graph tensor produced by a Softmax op (train_step runs under tf.function, gcn.py:328-335;
 *             on TF >= 2.6 also eagerly, through the output's _keras_logits): Keras takes the op's INPUT and calls
 *             softmax_cross_entropy_with_logits: loss = logsumexp(z) * sum_c y_c - sum_c y_c z_c, no renormalisation,
 *             no clip, dlogits = (p * sum_c y_c - y) / denom everywhere.
 * The two differ only where a probability saturates beyond 1e-7 (|z_i - z_j| > ~16). */
typedef enum { GCNX_CCE_PROBS = 0, GCNX_CCE_LOGITS = 1 } gcnx_cce_mode;

#define GCNX_UNIQUE_ID_BYTES 128

/* ---- lifecycle ------------------------------------------------------------------------ */
GCNX_API int gcnx_version(void);
GCNX_API int gcnx_device_count(int* n);
GCNX_API int gcnx_ctx_create(int device, gcnx_ctx** out);
GCNX_API int gcnx_ctx_destroy(gcnx_ctx* ctx);
/* Message of the last failing call on ctx (ctx may be NULL: last error of this thread). */
GCNX_API const char* gcnx_last_error(gcnx_ctx* ctx);
/* Fills name[len] with the device's gcnArchName and *cus with its compute-unit count. */
GCNX_API int gcnx_device_info(gcnx_ctx* ctx, char* name, int len, int* cus, size_t* hbm_bytes);

/* Diagnostics, not part of the drop-in contract: kernel-selection knobs of this ctx (the GCNX_* environment variables
 * set their initial values at gcnx_ctx_create; results never depend on them, only which kernel computes them).
 * Keys: "spmm_kernel" (0 auto, 1 rows, 2 tile = the round-1 tier kernels, 3 pipe = force the pipelined tile kernel),
 * "spmm_slab", "spmm_sg", "gemm_stream" (0 = bf16 GEMMs stay on the tiled kernel). */
GCNX_API int gcnx_set_tuning(gcnx_ctx* ctx, const char* key, int value);

/* ---- memory / sync (h2d, d2h synchronise the ctx stream) ------------------------------- */
GCNX_API int gcnx_malloc(gcnx_ctx* ctx, size_t bytes, void** dptr);
GCNX_API int gcnx_free(gcnx_ctx* ctx, void* dptr);
GCNX_API int gcnx_memset(gcnx_ctx* ctx, void* dptr, int value, size_t bytes);
GCNX_API int gcnx_h2d(gcnx_ctx* ctx, void* dst, const void* src, size_t bytes);
/* gcnx_h2d without the wait: the bytes are staged in pinned memory before the call returns and copied in stream order
 * (up to 16 KiB and outside capture; otherwise it is gcnx_h2d).  For per-batch descriptors: a synchronous copy makes every
 * streamed step wait for the previous one. */
GCNX_API int gcnx_h2d_async(gcnx_ctx* ctx, void* dst, const void* src, size_t bytes);
GCNX_API int gcnx_d2h(gcnx_ctx* ctx, void* dst, const void* src, size_t bytes);
GCNX_API int gcnx_d2d(gcnx_ctx* ctx, void* dst, const void* src, size_t bytes);
GCNX_API int gcnx_sync(gcnx_ctx* ctx);
/* Side sections: work launched between gcnx_side_begin and gcnx_side_end runs on a second HIP stream, after
 * everything submitted so far and concurrently with what follows on the main stream; gcnx_side_join makes the
 * main stream wait for the side sections ended so far (gcnx_sync and gcnx_capture_end join too).  Meant for the
 * gradient leaves of tape.gradient (gcn.py:337) -- dW, db -- which nothing later in the backward pass reads;
 * TensorFlow's executor runs such independent ops concurrently as well.  The caller keeps the buffers a side
 * section reads unmodified until the join.  Inside a capture the graph gets two branches. */
GCNX_API int gcnx_side_begin(gcnx_ctx* ctx);
GCNX_API int gcnx_side_end(gcnx_ctx* ctx);
GCNX_API int gcnx_side_join(gcnx_ctx* ctx);

/* ---- timing: HIP events on the ctx stream ---------------------------------------------- */
GCNX_API int gcnx_event_create(gcnx_ctx* ctx, gcnx_event** out);
GCNX_API int gcnx_event_record(gcnx_ctx* ctx, gcnx_event* ev);
/* Synchronises on `stop`, then returns stop - start in milliseconds. */
GCNX_API int gcnx_event_elapsed_ms(gcnx_ctx* ctx, gcnx_event* start, gcnx_event* stop, float* ms);
GCNX_API int gcnx_event_destroy(gcnx_ctx* ctx, gcnx_event* ev);

/* ---- HIP-graph capture of a call sequence (replaces tf.function, gcn.py:328) ----------- */
GCNX_API int gcnx_capture_begin(gcnx_ctx* ctx);
GCNX_API int gcnx_capture_end(gcnx_ctx* ctx, gcnx_graph** out);
GCNX_API int gcnx_graph_launch(gcnx_ctx* ctx, gcnx_graph* g);
GCNX_API int gcnx_graph_destroy(gcnx_ctx* ctx, gcnx_graph* g);

/* ---- graph preparation ------------------------------------------------------------------ */
/* DisjointLoader's SparseTensor (gcn.py:316-317 -> sp_matrix_to_sp_tensor + tf.sparse.reorder):
 * row-major sorted COO int64 (rows[nnz], cols[nnz]) on the DEVICE -> CSR int32.  Synchronises.
 * Fails with GCNX_ERR_DATA if rows are not non-decreasing or an index is outside [0,N); rowptr[0..N] and colidx[0..nnz)
 * are then unspecified, and nothing outside them is written in either case.  Duplicate (row, col) pairs are kept as stored.
 * N and nnz must be below 2^31 - 1 (GCNX_ERR_INVALID before anything is launched); N == 0 writes rowptr[0] = 0. */
GCNX_API int gcnx_coo_to_csr(gcnx_ctx* ctx, const int64_t* rows, const int64_t* cols, int64_t nnz,
                    int64_t n, int32_t* rowptr, int32_t* colidx);
/* Device-side collate (what DisjointLoader's collate -- vstack / block_diag / find, gcn.py:316-317,367 -- does on
 * the host).  The dataset is resident as one disjoint union: node_ptr int32[G+1], CSR (rowptr int32[Ntot+1],
 * colidx int32, optional vals), features x[Ntot, f], labels y[G, c].  desc int32[3(b+1)] = the b selected graph
 * ids (one pad), then the batch's node offsets [b+1], then its entry offsets [b+1] (host prefix sums over the
 * selected sizes).  Writes the batch: o_x[N, f], o_rowptr[N+1], o_colidx / o_vals[nnz], o_y[b, c],
 * o_graph_ptr[b+1], and (o_node_graph may be NULL) DisjointLoader's id vector i[N] = the batch position of every row's
 * graph.  Integer outputs are exact; floats are copies.  vals / o_vals are given together or both NULL; y == NULL writes no
 * labels; f == 0 needs no x / o_x.  Nothing else is written: padding columns (ldo > f) and whatever lies past N + 1 / nnz / b
 * rows stay as they were.  b == 0 writes nothing.  Does not synchronise.
 * Contract, NOT validated (the arrays live on the device): desc holds graph ids in [0, G) and the prefix sums of exactly
 * those graphs' sizes, node_ptr / rowptr are well-formed, and the outputs hold N + 1 / nnz / N x ldo / b x c elements. */
GCNX_API int gcnx_collate(gcnx_ctx* ctx, const int32_t* desc, int32_t b, const int32_t* node_ptr, const int32_t* rowptr,
                 const int32_t* colidx, const float* vals, const float* x, int64_t ldx, int32_t f, const float* y,
                 int32_t c, int32_t* o_rowptr, int32_t* o_colidx, float* o_vals, float* o_x, int64_t ldo, float* o_y,
                 int32_t* o_graph_ptr, int32_t* o_node_graph);
/* gcnx_collate that also gathers the selected graphs' rows of a second per-node matrix s [Ntot, f] (lds) into o_s [N, f]
 * (ldos) in the same launch: the aggregated features A x of the resident union, a per-graph constant because the filter of
 * a disjoint union is block-diagonal.  s == NULL (then o_s is ignored): exactly gcnx_collate. */
GCNX_API int gcnx_collate2(gcnx_ctx* ctx, const int32_t* desc, int32_t b, const int32_t* node_ptr, const int32_t* rowptr,
                 const int32_t* colidx, const float* vals, const float* x, int64_t ldx, int32_t f, const float* y,
                 int32_t c, int32_t* o_rowptr, int32_t* o_colidx, float* o_vals, float* o_x, int64_t ldo, float* o_y,
                 int32_t* o_graph_ptr, int32_t* o_node_graph, const float* s, int64_t lds, float* o_s, int64_t ldos);
/* The per-entry side of the same batch, a second launch on the same stream (Spektral's collate vstacks the graphs' edge
 * features e, gcn.py:173-180; spektral.layers.ECCConv reads them): desc, b, node_ptr and rowptr (the union's CSR row pointer,
 * read for every graph's entry offset and count) as in gcnx_collate; rowptr_t / colidx_t / perm_t = gcnx_csr_transpose_perm of
 * the UNION, e [nnz_all, s] (lde) its edge features, row k belonging to stored entry k.  The union being block-diagonal, a
 * graph's block of the transpose lies in the entry range of its own CSR block (rowptr_t[node_ptr[g]] == rowptr[node_ptr[g]]
 * for every g: the caller's guarantee), so the batch's transpose is gathered, not sorted.  Writes o_rowptr_t[N+1],
 * o_colidx_t[nnz], o_perm_t[nnz] -- exactly what gcnx_csr_transpose_perm returns on the batch's own CSR -- and o_e[nnz, s]
 * (ldoe), the rows of e in the batch CSR's entry order; nothing else (columns >= s of o_e and whatever lies past N + 1 / nnz
 * stay as they were).  Integer outputs are exact; floats are copies.  s >= 1; b == 0 writes nothing.  Does not synchronise. */
GCNX_API int gcnx_collate_edges(gcnx_ctx* ctx, const int32_t* desc, int32_t b, const int32_t* node_ptr, const int32_t* rowptr,
                       const int32_t* rowptr_t, const int32_t* colidx_t, const int32_t* perm_t, const float* e, int64_t lde,
                       int32_t s, int32_t* o_rowptr_t, int32_t* o_colidx_t, int32_t* o_perm_t, float* o_e, int64_t ldoe);
/* Spektral GCNConv.preprocess = gcn_filter on a CSR whose every row stores its
 * diagonal entry (true for the reference's data: gcn_utills.py:224-227 keeps the 0-Angstrom
 * diagonal).  vals_in NULL = ones.  SPEKTRAL: diag += 1; PYG: existing loops kept.
 * vals_out[e] = a~[e] * d^-1/2[row] * d^-1/2[col], d^-1/2 := 0 where the degree is <= 0.  vals_out may be vals_in
 * (in place: every entry is read and written by the same thread).  Synchronises; GCNX_ERR_DATA if a row has
 * no stored diagonal (vals_out is then unspecified).  n == 0 returns GCNX_OK and touches nothing.
 * Contract, NOT validated: rowptr is a well-formed CSR row pointer (rowptr[0] == 0, non-decreasing) and every column
 * index lies in [0, n) -- what gcnx_coo_to_csr produces; anything else reads out of bounds. */
GCNX_API int gcnx_gcn_norm(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx,
                  const float* vals_in, int32_t n, int mode, float* vals_out);
/* What the scheduling shortcuts may assume about a batch adjacency, checked once per batch on the device (the
 * reference's loader accepts any scipy matrix, gcn.py:104-116; nothing in Spektral requires symmetry).  *props
 * (host int) receives a bit set:
 *   GCNX_CSR_SYMMETRIC       A == A^T (pattern; values to 4 ulp): the backward aggregation may reuse this CSR for A^T
 *                            (otherwise build gcnx_csr_transpose);
 *   GCNX_CSR_GRAPH_PTR_OK    graph_ptr[0] == 0, graph_ptr[b] == n, non-decreasing;
 *   GCNX_CSR_BLOCK_DIAGONAL  every entry of a row of graph g has its column in [graph_ptr[g], graph_ptr[g+1]): the
 *                            premise of gcnx_spmm_plan_create and gcnx_spmm_csr_pool_bwd (sp.block_diag).
 * graph_ptr may be NULL (only symmetry is checked).  A graph_ptr that fails GRAPH_PTR_OK also clears BLOCK_DIAGONAL and is not
 * read any further; SYMMETRIC is still reported as the matrix has it.  A column index outside [0, n) is not followed: it
 * clears SYMMETRIC and BLOCK_DIAGONAL.  n == 0: every requested bit is reported.  Synchronises.
 * Contract, NOT validated: rowptr is a well-formed CSR row pointer (rowptr[0] == 0, non-decreasing, rowptr[n] entries
 * readable in colidx / vals). */
#define GCNX_CSR_SYMMETRIC 1
#define GCNX_CSR_BLOCK_DIAGONAL 2
#define GCNX_CSR_GRAPH_PTR_OK 4
GCNX_API int gcnx_csr_inspect(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals, int32_t n,
                     const int32_t* graph_ptr, int32_t b, int* props);
/* CSR of the transpose (for the backward SpMM when A^ is not symmetric).  Stable counting sort on the host: a column's
 * entries keep their stored order, vals_t follows them bit for bit.  vals and vals_t are given together or both NULL.
 * Validated on the host before the sort, each GCNX_ERR_DATA with nothing written: rowptr[0] == 0, rowptr non-decreasing,
 * rowptr[n] == nnz, every column index in [0, n) -- the same checks as gcnx_csr_transpose_perm.  Synchronises. */
GCNX_API int gcnx_csr_transpose(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx,
                       const float* vals, int32_t n, int32_t nnz, int32_t* rowptr_t,
                       int32_t* colidx_t, float* vals_t);
/* gcnx_csr_transpose of the pattern that also returns where every transposed entry came from: perm_t[p] = index of the
 * entry of the original CSR that became entry p of the transpose -- the row of per-entry data (edge features) that
 * belongs to it.  Integers throughout (entry numbers carried as float values stop being exact at 2^24).  Stable
 * counting sort; validates rowptr and colidx as gcnx_csr_transpose does (GCNX_ERR_DATA, nothing written); synchronises. */
GCNX_API int gcnx_csr_transpose_perm(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, int32_t n, int32_t nnz,
                            int32_t* rowptr_t, int32_t* colidx_t, int32_t* perm_t);

/* ---- edge-conditioned convolution (csrc/ecc.hip) ------------------------------------------- */
/* Replaces spektral.layers.ECCConv in single / disjoint mode (the layer Spektral offers for DisjointLoader batches with
 * edge features e -- the DCA / proximity pair the reference computes at gcn_utills.py:379-443 and its training script
 * drops, gcn.py:71): the gather of x by a.indices[:, 0], the per-entry [F, F_out] kernels of the "FGN_out" Dense, the
 * einsum and the scatter-add by a.indices[:, 1], in the factorised form of DESIGN.md ("ECCConv") that never forms the
 * per-entry kernels.  u [nnz, ldu] holds sp = S' channels per stored entry (the constant channel u^ = [u, 1] is
 * implicit; C = sp + 1 <= 17, more is refused with GCNX_ERR_UNSUPPORTED before anything is launched).  fp32, no
 * atomics: every row sums its entries in stored order, so results are bit-reproducible.  Any f >= 1 (float4 lanes when
 * f % 4 == 0 and leading dimensions / pointers are 16-byte aligned), any row length; leading dimensions honoured.
 *
 * gcnx_ecc_expand (forward): rowptr_t / colidx_t = CSR of the DESTINATIONS (row t lists the sources of the messages
 * into t: the transpose of the batch adjacency), eperm[nnz] = row of u of every entry of that CSR (perm_t of
 * gcnx_csr_transpose_perm; NULL = identity).  Writes
 *     scat[t, c*f + i] = sum over entries k of row t of  u^_k[c] * x[colidx_t[k], i]        (c < C; every row written)
 * and, with root != 0, the row's own x[t] into columns [C*f, (C+1)*f): [Scat | x], the operand of the layer's one
 * weight GEMM (gcnx_gemm with Wstack = [W_0; ..; W_{S'-1}; B; W_root]). */
GCNX_API int gcnx_ecc_expand(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const int32_t* eperm, const float* u,
                    int64_t ldu, int32_t sp, const float* x, int64_t ldx, int32_t f, float* scat, int64_t ld, int32_t n,
                    int32_t nnz, int root);
/* gcnx_ecc_bwd: the gradient of that aggregation wrt x and u in ONE launch (what tape.gradient derives from the gather /
 * einsum / scatter): rowptr / colidx = the batch adjacency itself (row s lists the destinations of s's messages, entry k
 * owns u[k]); dscat [n, ldd] = gradient wrt scat (C*f columns), dx_root [n, lddr] = gradient reaching x directly (the
 * root term; NULL = none).
 *     dx[s, i] = dx_root[s, i] + sum over entries k of row s, over c, of  u^_k[c] * dscat[colidx[k], c*f + i]
 *     du[k, c] = sum_i x[s, i] * dscat[colidx[k], c*f + i]                                        (c < sp)
 * dx (may alias dx_root) and du may each be NULL (the first layer needs no dx; u that is an input needs no du). */
GCNX_API int gcnx_ecc_bwd(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* u, int64_t ldu, int32_t sp,
                 const float* x, int64_t ldx, const float* dscat, int64_t ldd, const float* dx_root, int64_t lddr, int32_t f,
                 float* dx, int64_t lddx, float* du, int64_t lddu, int32_t n, int32_t nnz);

/* ---- forward ----------------------------------------------------------------------------- */
/* K1 MatMul+BiasAdd (+activation): out[N,Fo] = act(X[N,Fi] * W[Fi,Fo] + bias).
 * Replaces Dense / GCNConv.kernel / GeneralConv.kernel matmuls under gcn.py:334.
 * bias may be NULL.  alpha[Fo] is the PReLU slope (NULL unless act == PRELU). */
GCNX_API int gcnx_gemm(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* w, const float* bias,
              float* out, int64_t ldo, int64_t n, int32_t fi, int32_t fo, int prec, int act,
              const float* alpha);
/* Split-bf16 weight GEMMs for mid-size batches (r3; csrc/gemm_panel.hip): the Dense products of the reference's live
 * model GeneralGNN (gcn.py:320; MatMul + BiasAdd and the MatMul grad wrt the input, gcn.py:334/337) with the weight
 * operand read from a bf16 IMAGE in MFMA-fragment order.  gcnx_wimage_elems: bf16 elements of the image of W [fi, fo]
 * (transpose = 0: the operand of X W) or of W^T (transpose = 1: the operand of dH W^T); 0 for GCNX_PREC_F32.
 * gcnx_wimage_prepare: ONE launch writes the images of up to 16 matrices (per step: the weights change with every
 * update).  gcnx_gemm_wimage: out[n, fo] = x[n, fi] W + bias (transpose = 0) or out[n, fi] (+)= x[n, fo] W^T
 * (transpose = 1; accumulate: skip-connection gradients); GCNX_ERR_UNSUPPORTED without a message when the shape is
 * not the kernel's (widths in multiples of 16 / 4 floats, 16-byte aligned operands): call gcnx_gemm / gcnx_gemm_dx.
 * bn_parts (transpose = 0, fo <= 256): the batch-norm statistics of what is written, as (rows, mean, M2) per column
 * and workgroup -- [*n_parts][3][fo] floats, room for gcnx_gemm_wimage_parts(n) parts -- which gcnx_bn_finalize_parts
 * combines (Chan's formula, part order) into mean / inv and the Keras moving-statistics update: tf.nn.moments of the
 * Dense output without a pass over it. */
typedef struct gcnx_wimage_job {
  const float* w;
  void* img;
  int32_t fi, fo;
  int32_t transpose, prec;
} gcnx_wimage_job;
GCNX_API int64_t gcnx_wimage_elems(int32_t fi, int32_t fo, int transpose, int prec);
GCNX_API int gcnx_wimage_prepare(gcnx_ctx* ctx, int32_t njobs, const gcnx_wimage_job* jobs);
GCNX_API int gcnx_gemm_wimage(gcnx_ctx* ctx, const float* x, int64_t ldx, const void* img, int32_t fi, int32_t fo, int transpose,
                     const float* bias, float* out, int64_t ldo, int64_t n, int prec, int accumulate, float* bn_parts,
                     int32_t* n_parts);
GCNX_API int64_t gcnx_gemm_wimage_parts(gcnx_ctx* ctx, int64_t n);
GCNX_API int gcnx_bn_finalize_parts(gcnx_ctx* ctx, const float* parts, int32_t nparts, int32_t f, float momentum, float eps,
                           float* mean, float* inv, float* moving_mean, float* moving_var);
/* The block-diagonal structure of a DisjointLoader batch (sp.block_diag) as a
 * scheduling plan: block_ptr int32[nblocks+1] on the device (= graph_ptr) says that rows
 * [block_ptr[g], block_ptr[g+1]) reference only columns of that same range.  Built once per
 * batch (synchronises), owned by the caller, read-only afterwards; it must describe the CSR it
 * is later used with.  It only changes how gcnx_spmm_csr schedules work, never its result. */
GCNX_API int gcnx_spmm_plan_create(gcnx_ctx* ctx, const int32_t* block_ptr, int32_t nblocks,
                                   gcnx_spmm_plan** out);
GCNX_API int gcnx_spmm_plan_destroy(gcnx_ctx* ctx, gcnx_spmm_plan* plan);
/* The tile kernels deal a graph's output rows to their lanes in degree order (longest rows first), which they read from
 * a per-rowptr record list the plan builds from a host copy of rowptr (synchronises; kept per rowptr POINTER, up to four
 * per plan: the normalised, unweighted and transposed views of one batch share the plan).  gcnx_spmm_csr and
 * gcnx_spmm_csr_pool_bwd build it on first use with a rowptr; call this (a) before capturing such a call into a HIP graph
 * unless it has run once already, (b) again whenever the row pointers behind an already bound pointer change.  Like the
 * plan itself it only changes scheduling -- and the order in which a row's output is WRITTEN, never its value. */
GCNX_API int gcnx_spmm_plan_bind(gcnx_ctx* ctx, gcnx_spmm_plan* plan, const int32_t* rowptr, int32_t n);
/* K2/K3 SparseTensorDenseMatMul / gather+unsorted_segment_sum:
 * out[t,:] = act( sum_e vals[e] * h[colidx[e],:] + bias ), e over row t.
 * GCNConv.call (bias AFTER aggregation) and GeneralConv.propagate (vals NULL).
 * plan (may be NULL) enables the LDS-resident tile kernel for graphs that fit one. */
GCNX_API int gcnx_spmm_csr(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx,
                  const float* vals, const float* h, int64_t ldh, const float* bias, float* out,
                  int64_t ldo, int32_t n, int32_t f, int act, const gcnx_spmm_plan* plan);
/* K4 SegmentSum / mean / max over sorted graph ids (GlobalSumPool, gcn.py:320 pool="sum";
 * max variant: gcn_utills.py:842).  graph_ptr int32[B+1].  argmax int32[B*F] (row index of
 * the maximum; required for MAX, else NULL). */
GCNX_API int gcnx_segment_pool(gcnx_ctx* ctx, const int32_t* graph_ptr, const float* x, int64_t ldx,
                      float* pooled, int32_t b, int32_t f, int mode, int32_t* argmax);
/* K8 Softmax + CategoricalCrossentropy + categorical_accuracy (gcn.py:326,335,339):
 * probs = softmax(logits); loss_acc[0] += sum_g loss_g / denom; loss_acc[1] += #(argmax p == argmax y).
 * cce_mode GCNX_CCE_LOGITS (the training step, gcn.py:328-335): loss_g = sum_c y_c (logsumexp(z) - z_c),
 *   dlogits = (p * sum_c y_c - y) / denom.
 * cce_mode GCNX_CCE_PROBS (eager evaluate, gcn.py:351-354): loss_g = -sum_c y_c log clip(p_c, 1e-7, 1 - 1e-7),
 *   dlogits = (p * sum(y*m) - y*m) / denom with m = [1e-7 < p < 1 - 1e-7], the gradient of the clipped loss.
 * dlogits NULL to skip.  denom = global batch size (so that shard gradients add up to the full-batch gradient).
 * loss_acc is a device float[2] that the caller zeroes. */
GCNX_API int gcnx_softmax_cce(gcnx_ctx* ctx, const float* logits, const float* y, int32_t b, int32_t c,
                     float denom, float* probs, float* loss_acc, float* dlogits, int cce_mode);

/* The classifier head in ONE launch: probs = softmax(pooled * W + b)  (the model's last Dense,
 * gcn.py:320 activation="softmax"), loss_acc[0] = CCE(y, probs) summed over the b graphs / denom and
 * loss_acc[1] = #(argmax probs == argmax y)  (gcn.py:326,335,339; loss_acc is OVERWRITTEN, not accumulated),
 * and, when dw != NULL, the head gradients tape.gradient (gcn.py:337) produces:
 * dlogits as gcnx_softmax_cce (same cce_mode), dw[h,c] = pooled^T dlogits, db[c] = sum_g dlogits, dpooled[b,h] = dlogits W^T.
 * y == NULL: probabilities only.  c <= 32.  Same results as gcnx_gemm + gcnx_softmax_cce + gcnx_gemm_dw +
 * gcnx_act_bias_grad + gcnx_gemm_dx up to fp32 summation order; deterministic (fixed reduction order). */
GCNX_API int gcnx_dense_softmax_cce(gcnx_ctx* ctx, const float* pooled, int64_t ldp, const float* w, const float* bias,
                           const float* y, int32_t b, int32_t h, int32_t c, float denom, float* probs,
                           float* loss_acc, float* dw, float* db, float* dpooled, int64_t lddp, int cce_mode);

/* GlobalSumPool / GlobalAvgPool / GlobalMaxPool (gcn.py:319) + the head above as one call: pooled[b,h] =
 * gcnx_segment_pool(x[n,h]) is still written (the caller's saved activation), but where the pool is split into
 * row slices (few graphs: SUM / AVG) the head combines the partial sums itself while staging its operand, so the
 * pair runs as 2 launches instead of 3 (with half as many row slices: the head's workgroup reads them all).
 * Otherwise exactly gcnx_segment_pool + gcnx_dense_softmax_cce.  Results equal those of the two calls up to the
 * fp32 summation order of the pool; deterministic.  argmax: as gcnx_segment_pool (MAX only).
 * ldp >= h is the row stride of pooled on every route (the separate calls included); columns h .. ldp-1 are not written.
 * db_relu (may be NULL; needs dw and SUM / AVG): float[h] = what gcnx_pool_bwd_colsum(dpooled, y = x) returns, the
 * bias gradient of the layer that produced x through a ReLU (GCNConv, gcn.py:317) -- on the combined path the pool
 * counts the positive entries per (graph, column) in the pass it makes anyway and the head finishes
 * sum_g s_g * dPooled[g] * count[g], so that gradient costs no launch of its own. */
GCNX_API int gcnx_pool_dense_softmax_cce(gcnx_ctx* ctx, const int32_t* graph_ptr, const float* x, int64_t ldx, int pool_mode,
                                int32_t* argmax, float* pooled, int64_t ldp, const float* w, const float* bias,
                                const float* y, int32_t b, int32_t h, int32_t c, float denom, float* probs,
                                float* loss_acc, float* dw, float* db, float* dpooled, int64_t lddp,
                                float* db_relu, int cce_mode);

/* ---- backward (what tape.gradient, gcn.py:337, generates) -------------------------------- */
/* dZ = dY * act'(Y) (mask taken from the saved output Y; PReLU uses the saved pre-activation
 * passed as y and alpha); db[f] = sum_rows dZ (BiasAddGrad).  dz may alias dy.  db/dalpha may
 * be NULL.  For PRELU dalpha[f] = sum_rows dY*min(y,0). */
GCNX_API int gcnx_act_bias_grad(gcnx_ctx* ctx, const float* dy, int64_t lddy, const float* y, int64_t ldy,
                       float* dz, int64_t lddz, int64_t n, int32_t f, int act,
                       const float* alpha, float* db, float* dalpha);
/* dW[Fi,Fo] = X^T[Fi,N] * dH[N,Fo]: deterministic two-stage split-K (no atomics). */
GCNX_API int gcnx_gemm_dw(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* dh, int64_t lddh,
                 float* dw, int64_t n, int32_t fi, int32_t fo, int prec);
/* ---- bf16 STORAGE of activations that only bf16-operand weight GEMMs read (r3; large batches, GCNX_PREC_BF16) ----------
 * GCNX_PREC_BF16 rounds both operands of a product to bfloat16 (nearest even) as it loads them (tf.cast(x, tf.bfloat16)
 * in front of every MatMul / MatMul grad of the Dense and GCNConv kernels, gcn.py:334, :337).  A tensor that only such
 * products read -- S1 = A X, Y1, dH2 = A^T dZ2, dZ1 of the two-layer model -- can be STORED rounded: every result stays
 * bit-identical and the producer and the consumers move half its bytes.  `x16` / `dh16` / `out16` are uint16 rows
 * (bfloat16 bit patterns), leading dimensions in ELEMENTS.
 *   gcnx_spmm_csr_bf16out           = gcnx_spmm_csr with the result stored as bf16 (tile kernels + 8-row chunks only).
 *   gcnx_spmm_csr_pool_bwd_bf16out  = gcnx_spmm_csr_pool_bwd(plan, y_bits) with the result stored as bf16.
 *   gcnx_gemm_fwd_bf16              = gcnx_gemm / gcnx_gemm_relu_bits on a bf16 input; out as bf16 (out_bf16) or fp32.
 *   gcnx_gemm_dx_bf16               = gcnx_gemm_dx / gcnx_gemm_dx_bits on a bf16 dH (mask_bits and db may be NULL).
 *   gcnx_gemm_dw_bf16               = gcnx_gemm_dw with both operands stored as bf16.
 * All five return GCNX_ERR_UNSUPPORTED -- nothing launched, gcnx_last_error untouched -- for shapes outside the streaming /
 * tile kernels (GEMMs: fi = fo = 256, n >= 32768; SpMM: weighted operator, a plan whose tile graphs all take the
 * 1024-thread shape, f a multiple of 32 above 128, no hub rows): keep fp32 storage then. */
GCNX_API int gcnx_spmm_csr_bf16out(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals, const float* h,
                          int64_t ldh, const float* bias, void* out16, int64_t ldo, int32_t n, int32_t f, int act,
                          const gcnx_spmm_plan* plan);
GCNX_API int gcnx_spmm_csr_pool_bwd_bf16out(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals,
                          const float* y, int64_t ldy, const int32_t* graph_ptr, int32_t b, const float* dpooled, int64_t lddp,
                          void* out16, int64_t ldo, int32_t n, int32_t f, int mode, const gcnx_spmm_plan* plan, const void* y_bits);
GCNX_API int gcnx_gemm_fwd_bf16(gcnx_ctx* ctx, const void* x16, int64_t ldx, const float* w, const float* bias, void* out, int64_t ldo,
                          int out_bf16, int64_t n, int32_t fi, int32_t fo, int act, void* relu_bits, const void* wimg);
GCNX_API int gcnx_gemm_dx_bf16(gcnx_ctx* ctx, const void* dh16, int64_t lddh, const float* w, void* dx, int64_t lddx, int dx_bf16,
                          int64_t n, int32_t fi, int32_t fo, const void* mask_bits, float* db, const void* wimg);
/* `wimg` (may be NULL: the call builds it, one small launch): the bf16 image of the weight operand in MFMA-fragment order,
 * GCNX_STREAM_IMAGE_BYTES bytes, written by gcnx_gemm_stream_images -- the images of up to four operands in ONE launch, once
 * per step after the optimizer update (transpose = 1: the operand of gcnx_gemm_fwd_bf16, X W; 0: of gcnx_gemm_dx_bf16,
 * dH W^T).  A 1/8 shard of config 3 is a 0.5 ms step: three 5-us preparation launches are 3 % of it. */
#define GCNX_STREAM_IMAGE_BYTES 131072
typedef struct gcnx_stream_image_job {
  const float* w; int32_t fi, fo;   /* W [fi, fo], 256 x 256 */
  int32_t transpose;
  void* img;                        /* GCNX_STREAM_IMAGE_BYTES bytes, 16-byte aligned */
} gcnx_stream_image_job;
GCNX_API int gcnx_gemm_stream_images(gcnx_ctx* ctx, int32_t njobs, const gcnx_stream_image_job* jobs);
GCNX_API int gcnx_gemm_dw_bf16(gcnx_ctx* ctx, const void* x16, int64_t ldx, const void* dh16, int64_t lddh, float* dw, int64_t n,
                          int32_t fi, int32_t fo);
/* The ReLU mask of a Dense / GCNConv kernel product as a bit image between the forward and the backward product of
 * large batches: gcnx_gemm_relu_bits = gcnx_gemm(act = GCNX_ACT_RELU) that also writes [out > 0] to `bits` (n * 64
 * bytes reserved, 8-byte aligned; layout private to the pair, which must use the same precision), gcnx_gemm_dx_bits = gcnx_gemm_dx masked by that image instead of
 * the saved activation (ReluGrad after MatMul grad, gcn.py:337) -- 32 bytes per row read where the activation is 1 KiB.
 * Served by the streaming bf16 kernels only (GCNX_PREC_BF16 / BF16X3, fi = fo = 256, n >= 32768): GCNX_ERR_UNSUPPORTED
 * otherwise, nothing is launched and -- UNSUPPORTED being an answer, not a failure -- gcnx_last_error is left as it was. */
GCNX_API int gcnx_gemm_relu_bits(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* w, const float* bias, float* out,
                        int64_t ldo, int64_t n, int32_t fi, int32_t fo, int prec, void* bits);
GCNX_API int gcnx_gemm_dx_bits(gcnx_ctx* ctx, const float* dh, int64_t lddh, const float* w, float* dx, int64_t lddx,
                      int64_t n, int32_t fi, int32_t fo, int prec, const void* mask_bits, float* db);
/* dX[N,Fi] (+)= dH[N,Fo] * W^T.  accumulate != 0 adds into dx (skip-connection gradients).
 * y_mask (may be NULL): saved ReLU output of the layer that produced this GEMM's input; the
 * epilogue then writes dZ = dX * (y_mask > 0), i.e. the activation gradient of that layer is
 * fused.  db (may be NULL): column sums of what was written (BiasAddGrad of that layer). */
GCNX_API int gcnx_gemm_dx(gcnx_ctx* ctx, const float* dh, int64_t lddh, const float* w, float* dx,
                 int64_t lddx, int64_t n, int32_t fi, int32_t fo, int prec, int accumulate,
                 const float* y_mask, int64_t ldy, float* db);
/* The backward of one Dense / GCNConv kernel product H = X W given dH, as one call:
 *   dW[fi,fo] = X^T dH   (gcnx_gemm_dw)   and   dX[n,fi] = dH W^T (* [y_mask > 0]), db_prev = colsum(dX)   (gcnx_gemm_dx)
 * -- the two matmul gradients tape.gradient (gcn.py:337) emits for every `x @ kernel` (Spektral GCNConv.call).
 * Both read dH; fp32 with 64-column-aligned fi runs them as ONE launch (the dX tiles, and the dW split-K tiles in
 * the otherwise idle workgroup slots) plus ONE reduction launch (db_prev partials and dW slabs together): dW is a
 * gradient leaf, so on small batches it disappears behind dX instead of costing a launch pair or a second stream.
 * Other precisions / shapes: exactly the two calls.  Deterministic; y_mask / db_prev may be NULL. */
GCNX_API int gcnx_dense_bwd(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* dh, int64_t lddh, const float* w,
                   int64_t n, int32_t fi, int32_t fo, int prec, float* dx, int64_t lddx, const float* y_mask,
                   int64_t ldy, float* db_prev, float* dw);
/* Gradient of the global pool: SUM dX[r] = dP[g(r)]; AVG /n_g; MAX routed to argmax rows.
 * If y (saved ReLU output of the last conv layer) is given its mask is fused:
 * dX[r] *= (y[r] > 0).  db (may be NULL): column sums of dX (BiasAddGrad of that layer). */
GCNX_API int gcnx_segment_pool_bwd(gcnx_ctx* ctx, const int32_t* graph_ptr, const float* dpooled,
                          float* dx, int64_t lddx, int32_t n, int32_t b, int32_t f, int mode,
                          const int32_t* argmax, const float* y, int64_t ldy, float* db);

/* The two calls above the last conv layer's backward aggregation as ONE gather (small batches: each launch there is
 * latency): for SUM / AVG pooling and a block-diagonal operator,
 *   (A^T dZ)[i] = scale_g * dPooled[g(i)] * sum_j A^T[i,j] * [y[j] > 0],   dZ[j] = scale_g * dPooled[g(j)] * [y[j] > 0]
 * -- replaces gcnx_segment_pool_bwd(y=...) + gcnx_spmm_csr for the gradient of GlobalSumPool (gcn.py:319) through
 * the ReLU of the last GCNConv (gcn.py:317) and its aggregation; tf.GradientTape materialises dZ there (gcn.py:337).
 * (rowptr, colidx, vals) is the TRANSPOSED operator, as for the unfused backward call.  Needs f, ldy, ldo, lddp in
 * multiples of 4 floats and 16-byte aligned y / out / dpooled; MAX pooling has no such form (GCNX_ERR_INVALID).
 * plan (may be NULL): the operator's gcnx_spmm_plan built over the same graph_ptr -- large batches then run on the tile
 * kernels (the landed tile of y is masked in place, the graph's dPooled row scales the sums). */
GCNX_API int gcnx_spmm_csr_pool_bwd(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals,
                           const float* y, int64_t ldy, const int32_t* graph_ptr, int32_t b,
                           const float* dpooled, int64_t lddp, float* out, int64_t ldo, int32_t n, int32_t f,
                           int mode, const gcnx_spmm_plan* plan, const void* y_bits);
/* gcnx_spmm_csr with act = ReLU on the tile kernels, which also write [out > 0] as a bit image: one 32-bit word per (row,
 * 32-column slab), slab-major -- relu_bits[slab * n + row], (f / 32) * n words -- for the rows of every graph the plan
 * serves with a tile (graphs taller than a tile get no bits; gcnx_spmm_csr_pool_bwd folds their rows from `out`).
 * gcnx_spmm_csr_pool_bwd(..., y_bits = relu_bits) then expands the words into its 0 / 1 tile instead of reading y:
 * 4 bytes per row and slab instead of 128.  GCNX_ERR_UNSUPPORTED when gcnx_spmm_csr would not take the tile kernels
 * (no plan, too few tile units, f % 32 != 0, an operand that is not 16-byte aligned or a leading dimension that is no multiple
 * of 4 floats): nothing is launched; call gcnx_spmm_csr then and pass y_bits = NULL. */
GCNX_API int gcnx_spmm_csr_relu_bits(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals,
                           const float* h, int64_t ldh, const float* bias, float* out, int64_t ldo, int32_t n, int32_t f,
                           const gcnx_spmm_plan* plan, void* relu_bits);
/* The pooled GCNConv's forward of a TRAINING step on a tile plan without its output (r3): what the step needs of
 * Y = relu(A h + b) is [Y > 0] as the bit image (the folded backward aggregation, gcnx_spmm_csr_pool_bwd(y_bits)), the
 * graphs' pooled rows -- GlobalSumPool / GlobalAvgPool([Y, i]), gcn.py:334 -- and the positive counts per (graph, column)
 * (the layer's bias gradient).  On graphs that fit an LDS tile all three leave the aggregation's epilogue: their rows of
 * `out` are NOT written and no pool launch reads them back (2 GB of the config-3 step).  Graphs taller than a tile keep
 * the two-launch form: their rows of `out` ARE written (the folded backward gathers them) and pooled from there.
 * pooled [b, ldp], cnt [b, f]: EVERY row is written -- a graph without rows (graph_ptr[g] == graph_ptr[g + 1]) gets zeros in
 * both, what gcnx_segment_pool gives for an empty segment in SUM and AVG mode.
 * GCNX_ERR_UNSUPPORTED (nothing launched) when the tile kernels do not serve the batch:
 * gcnx_spmm_csr_relu_bits / gcnx_spmm_csr + gcnx_pool_dense_softmax_cce then. */
GCNX_API int gcnx_spmm_csr_relu_bits_pool(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals, const float* h,
                        int64_t ldh, const float* bias, float* out, int64_t ldo, int32_t n, int32_t f, const gcnx_spmm_plan* plan,
                        void* relu_bits, const int32_t* graph_ptr, int32_t b, int pool_mode, float* pooled, int64_t ldp, float* cnt);
/* ... and the classifier head on those pooled rows: gcnx_dense_softmax_cce + db_relu[c] = sum_g pool'(dPooled)[g][c] *
 * cnt[g][c] (the pooled layer's bias gradient; NULL to skip). */
GCNX_API int gcnx_pooled_dense_softmax_cce(gcnx_ctx* ctx, const int32_t* graph_ptr, int pool_mode, const float* pooled, int64_t ldp,
                        const float* cnt, const float* w, const float* bias, const float* y, int32_t b, int32_t h, int32_t c,
                        float denom, float* probs, float* loss_acc, float* dw, float* db, float* dpooled, int64_t lddp,
                        float* db_relu, int cce_mode);
/* db[f] = column sums of the same never-materialised dZ (BiasAddGrad of that layer):
 * sum_g scale_g * dPooled[g] * #{j in g : y[j] > 0}; deterministic (fixed summation order). */
GCNX_API int gcnx_pool_bwd_colsum(gcnx_ctx* ctx, const int32_t* graph_ptr, int32_t b, const float* dpooled,
                         int64_t lddp, const float* y, int64_t ldy, int32_t f, int mode, float* db);

/* ---- Keras BatchNormalization + PReLU around Dense (MLP / GeneralConv of GeneralGNN, gcn.py:320;
 *      axis -1, momentum 0.99, eps 1e-3, biased batch variance) ------------------- */
/* sums[0:f] = column sums of (z - shift), sums[f:2f] = column sums of (z - shift)^2 (device float[2f]);
 * shift (device float[f], may be NULL = 0).  tf.nn.moments takes the variance of the CENTRED data; to match it
 * in fp32 call twice: shift = NULL gives the mean, shift = mean gives a cancellation-free variance.  A sharded
 * caller all-reduces `sums` (and the row count) between gcnx_bn_stats and gcnx_bn_finalize for sync-BN. */
GCNX_API int gcnx_bn_stats(gcnx_ctx* ctx, const float* z, int64_t ldz, int64_t n, int32_t f, const float* shift,
                           float* sums);
/* Training (sums != NULL): d = sums/count, mean = shift + d, var = sums2/count - d^2 (biased),
 * inv = 1/sqrt(var+eps); the moving statistics (may be NULL) are updated: m <- momentum*m + (1-momentum)*batch.
 * mean may alias shift.  Inference (sums == NULL): mean/inv come from the moving statistics. */
GCNX_API int gcnx_bn_finalize(gcnx_ctx* ctx, const float* sums, float count, int32_t f, float momentum,
                              float eps, const float* shift, float* mean, float* inv, float* moving_mean,
                              float* moving_var);
/* Single-device shortcut for the training-mode moments: gcnx_bn_stats + gcnx_bn_finalize for the mean, then again
 * centred on it for the variance (the two-pass tf.nn.moments form), with each reduce + finalise pair fused: four
 * launches instead of six, bit-identical results.  moving_* (both or none) get the momentum update. */
GCNX_API int gcnx_bn_moments(gcnx_ctx* ctx, const float* z, int64_t ldz, int64_t n, int32_t f, float momentum, float eps,
                    float* mean, float* inv, float* moving_mean, float* moving_var);
/* y = act(gamma * (z - mean) * inv + beta); act NONE / RELU / PRELU(alpha[f]). */
GCNX_API int gcnx_bn_act(gcnx_ctx* ctx, const float* z, int64_t ldz, int64_t n, int32_t f, const float* mean,
                         const float* inv, const float* gamma, const float* beta, int act, const float* alpha,
                         float* y, int64_t ldy);
/* Backward of gcnx_bn_act given dY and the saved z, mean, inv: dzb = dY*act'(zb);
 * training: dZ = gamma*inv*(dzb - mean_rows(dzb) - xhat*mean_rows(dzb*xhat)); inference: gamma*inv*dzb.
 * dgamma = sum dzb*xhat, dbeta = sum dzb, dalpha = sum dY*min(zb,0) (each may be NULL).
 * sums_scratch: device float[3f].  dz may alias dy. */
GCNX_API int gcnx_bn_act_bwd(gcnx_ctx* ctx, const float* dy, int64_t lddy, const float* z, int64_t ldz, int64_t n,
                             int32_t f, const float* mean, const float* inv, const float* gamma, const float* beta,
                             int act, const float* alpha, int training, float* dz, int64_t lddz, float* dgamma,
                             float* dbeta, float* dalpha, float* sums_scratch);
/* The two halves of gcnx_bn_act_bwd for sync-BN: _stats writes the three LOCAL column sums to sums_scratch[3f]
 * (and, if given, to dbeta / dgamma / dalpha -- local parts, to be summed with the other parameter gradients);
 * the caller all-reduces sums_scratch; _apply forms dz with the reduced sums and the GLOBAL row count. */
GCNX_API int gcnx_bn_act_bwd_stats(gcnx_ctx* ctx, const float* dy, int64_t lddy, const float* z, int64_t ldz, int64_t n,
                          int32_t f, const float* mean, const float* inv, const float* gamma, const float* beta, int act,
                          const float* alpha, float* sums_scratch, float* dgamma, float* dbeta, float* dalpha);
GCNX_API int gcnx_bn_act_bwd_apply(gcnx_ctx* ctx, const float* dy, int64_t lddy, const float* z, int64_t ldz, int64_t n,
                          int32_t f, const float* mean, const float* inv, const float* gamma, const float* beta, int act,
                          const float* alpha, const float* sums, float count, int training, float* dz, int64_t lddz);

/* ---- the reference's torch GCN (gcn_utills.py:795-853): BatchNorm1d(track_running_stats=False) + PReLU() -------------
 * gcnx_bn_act + gcnx_segment_pool(MAX) in one pass over z: pooled[g, c] = max over graph g's rows of
 * act(gamma * (z - mean) * inv + beta) and argmax[g, c] its row (int32[b * f]), the [n, f] activation never written.
 * Every element is evaluated as gcnx_bn_act evaluates it and ties go to the first maximal row, so pooled and argmax are
 * BIT-IDENTICAL to the two calls; an empty graph pools to 0.  pool_mode: GCNX_POOL_MAX only (GCNX_ERR_UNSUPPORTED
 * otherwise). */
GCNX_API int gcnx_bn_act_pool(gcnx_ctx* ctx, const int32_t* graph_ptr, int32_t b, const float* z, int64_t ldz, int32_t f,
                     const float* mean, const float* inv, const float* gamma, const float* beta, int act, const float* alpha,
                     int pool_mode, float* pooled, int64_t ldp, int32_t* argmax);
/* Its backward (training-mode BatchNorm, batch statistics over the n rows): from dpooled [b, f], argmax and the saved z,
 * mean, inv: dZ [n, f] = gamma * inv * (dzb - sum(dzb) / n - xhat * sum(dzb * xhat) / n) with dzb nonzero only at the
 * argmax rows, and dgamma / dbeta [f], dalpha ([f] for PRELU, [1] for PRELU_SHARED) -- each may be NULL.  Two launches (the
 * three column sums come from the b * f argmax entries alone, then one dense write of dZ).  graph_ptr must cover the rows:
 * graph_ptr[0] = 0, graph_ptr[b] = n (rows outside every graph are not written).  pool_mode: GCNX_POOL_MAX only.
 * n == 0 (an empty shard) with f > 0: nothing is launched and no other pointer is read; dgamma / dbeta and, under
 * PRELU / PRELU_SHARED, dalpha ([f] / [1]) are set to zero where given, as gcnx_bn_act_bwd_stats does for n == 0 and
 * gcnx_bn_act_pool_bwd_stats for graphs that are all empty. */
GCNX_API int gcnx_bn_act_pool_bwd(gcnx_ctx* ctx, const int32_t* graph_ptr, int32_t b, const float* dpooled, int64_t lddp,
                         const int32_t* argmax, const float* z, int64_t ldz, int64_t n, int32_t f, const float* mean,
                         const float* inv, const float* gamma, const float* beta, int act, const float* alpha, int pool_mode,
                         float* dz, int64_t lddz, float* dgamma, float* dbeta, float* dalpha);
/* The two launches of gcnx_bn_act_pool_bwd with caller-held sums, for sync-BN over graph shards: _stats writes the three
 * LOCAL column sums (sum dzb, sum dzb * xhat, sum dy * min(zb, 0)), formed from the b * f argmax entries alone, to
 * sums[3f] (device memory) and the local parts of dgamma / dbeta / dalpha ([1] for PRELU_SHARED; each may be NULL);
 * the caller all-reduces sums; _apply writes dZ over every local row with the reduced sums and the GLOBAL row count
 * `count`.  _stats + _apply with count = n make the same launches as gcnx_bn_act_pool_bwd, with the same bits. */
GCNX_API int gcnx_bn_act_pool_bwd_stats(gcnx_ctx* ctx, const int32_t* graph_ptr, int32_t b, const float* dpooled, int64_t lddp,
                         const int32_t* argmax, const float* z, int64_t ldz, int32_t f, const float* mean, const float* inv,
                         const float* gamma, const float* beta, int act, const float* alpha, int pool_mode, float* sums,
                         float* dgamma, float* dbeta, float* dalpha);
GCNX_API int gcnx_bn_act_pool_bwd_apply(gcnx_ctx* ctx, const int32_t* graph_ptr, int32_t b, const float* dpooled, int64_t lddp,
                         const int32_t* argmax, const float* z, int64_t ldz, int32_t f, const float* mean, const float* inv,
                         const float* gamma, const float* beta, int act, const float* alpha, int pool_mode, const float* sums,
                         float count, float* dz, int64_t lddz);
/* The post-pool half of the torch GCN -- Linear(h->h) . BatchNorm1d . PReLU() -> Linear(h->1) . BatchNorm1d . PReLU() --
 * with BCEWithLogitsLoss and its backward in ONE launch (one workgroup: every BatchNorm needs all b rows).  Torch layouts:
 * w3 [h, h] and w4 [1, h] are [out, in]; y = x W^T + b.  BatchNorm: batch mean, biased variance, eps; gamma / beta [h] and
 * [1]; PReLU: one slope each (alpha3[0], alpha4[0]).  Forward: out[b] (the logits: torch's forward output), probs = sigmoid(out),
 * and, with y != NULL, loss_acc[0] = sum_g bce(out_g, t_g) / denom, loss_acc[1] = #(out_g > 0 == t_g > 0.5) (OVERWRITTEN,
 * the layout of gcnx_dense_softmax_cce) where t_g = y[g * y_stride + y_col]; bce(z, t) = max(z, 0) - z t + log1p(exp(-|z|)).
 * grads != 0 (needs y): dout = (sigmoid(out) - t) / denom through the whole head: dpooled [b, h] and the gradients of
 * every parameter (dw3 [h, h], db3, dgamma3, dbeta3 [h], dalpha3 [1], dw4 [1, h], db4, dgamma4, dbeta4, dalpha4 [1]).
 * Limits: b >= 2 (a BatchNorm over one row is undefined; GCNX_ERR_INVALID), 1 <= h <= 256 (GCNX_ERR_UNSUPPORTED above);
 * scratch: >= gcnx_bce_head_scratch_floats(b, h) floats of device memory, not kept between calls.  Deterministic. */
typedef struct gcnx_bce_head_args {
  const float* pooled; int64_t ldp; int32_t b; int32_t h;
  const float* w3; const float* b3; const float* gamma3; const float* beta3; const float* alpha3;
  const float* w4; const float* b4; const float* gamma4; const float* beta4; const float* alpha4;
  float eps; float denom;
  const float* y; int32_t y_stride; int32_t y_col; int32_t grads;
  float* out; float* probs; float* loss_acc;
  float* dpooled; int64_t lddp;
  float* dw3; float* db3; float* dgamma3; float* dbeta3; float* dalpha3;
  float* dw4; float* db4; float* dgamma4; float* dbeta4; float* dalpha4;
  float* scratch; int64_t scratch_floats;
} gcnx_bce_head_args;
GCNX_API int64_t gcnx_bce_head_scratch_floats(int32_t b, int32_t h);
GCNX_API int gcnx_bn_prelu_bce_head(gcnx_ctx* ctx, const gcnx_bce_head_args* args);
/* The same head in seven phases, for a batch sharded by graph over ranks (sync-BN: every BatchNorm uses the statistics
 * of the whole batch).  args is as above with args->b the LOCAL row count (>= 1); count is the GLOBAL row count (>= 2,
 * else GCNX_ERR_INVALID).  Phase k writes local partial sums to its slice of red (device float[gcnx_bce_head_phase_red_floats(h)]);
 * the caller all-reduces that slice and phase k + 1 reads it.  red's slices (offsets in floats):
 *   phase 0  z3 = P W3^T + b3; sum z3                                   -> red[0, h)
 *   phase 1  mean3; sum (z3 - mean3)^2                                   -> red[h, 2h)
 *   phase 2  inv3, y3 = PReLU3(BN3(z3)), z4 = y3 W4^T + b4; sum z4       -> red[2h]
 *   phase 3  mean4; sum (z4 - mean4)^2                                   -> red[2h + 1]
 *   phase 4  inv4, out, probs; with y: loss_acc (local part); with grads:
 *            sum dzb4, sum dzb4 xhat4 and the local dbeta4 / dgamma4 / dalpha4   -> red[2h + 2, 2h + 4)
 *   phase 5  dz4, db4, dw4; sum dzb3, sum dzb3 xhat3 and the local dbeta3 / dgamma3 / dalpha3 -> red[2h + 4, 4h + 4)
 *   phase 6  dZ3, db3, dpooled = dZ3 W3, dw3                              (nothing to reduce)
 * Phases 0-3 are the forward, 4 the loss; 5 and 6 need grads.  Every gradient and both loss_acc floats are the LOCAL
 * parts, OVERWRITTEN: summed over the ranks they give the whole batch's (loss_acc[0] is sum bce / denom).  scratch: >=
 * gcnx_bce_head_phase_scratch_floats(b, h) floats, kept between the phases; red too.  Each reduction has a fixed order.
 * One workgroup per phase.  With one shard and count = b the phases give the one-launch head's numbers. */
GCNX_API int64_t gcnx_bce_head_phase_scratch_floats(int32_t b, int32_t h);
GCNX_API int64_t gcnx_bce_head_phase_red_floats(int32_t h);
GCNX_API int gcnx_bce_head_phase(gcnx_ctx* ctx, const gcnx_bce_head_args* args, int32_t phase, float count, float* red);

/* ---- GeneralGNN options beside gcn.py:320's defaults (csrc/elementwise.hip) ------------------ */
/* Keras Dropout(rate) in training mode (the Dropout layer of Spektral's MLP and GeneralConv):
 * out = x * keep / (1 - rate), keep ~ Bernoulli(1 - rate) per element.  The keep decision of element (row, col) is a
 * stateless hash of (seed, stream_id, *step, row * f + col) -- step may be NULL (0) -- so calling it again with the same
 * arguments on the incoming gradient IS the layer's backward pass (no stored mask), and a captured step that reads `step`
 * from device memory draws a fresh mask on every replay (gcnx_counter_add advances it).  TensorFlow's random generator
 * is not reproduced.  out may alias x. */
GCNX_API int gcnx_dropout(gcnx_ctx* ctx, const float* x, int64_t ldx, int64_t n, int32_t f, float rate, uint32_t seed,
                          uint32_t stream_id, const uint32_t* step, float* out, int64_t ldo);
/* *counter += inc on the stream (the optimizer's step count: optimizer.iterations, gcn.py:338). */
GCNX_API int gcnx_counter_add(gcnx_ctx* ctx, uint32_t* counter, uint32_t inc);
/* out = a + b, row by row (GeneralGNN(connectivity="sum"): out = z + out).  out may alias a or b. */
GCNX_API int gcnx_add(gcnx_ctx* ctx, const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldo,
                      int64_t n, int32_t f);

/* GeneralConv(aggregate = "max" | "min") (tf.math.unsorted_segment_max / _min over the messages gather(h, a.indices[:,1]) of
 * every target row; adjacency values ignored): out[t, c] = max (min) over the entries (t, s) of h[s, c]; a row
 * without entries gets the lowest (largest) float, as TensorFlow does.  cnt (may be NULL; needed for the gradient) receives
 * the number of entries attaining the extremum. */
GCNX_API int gcnx_spmm_csr_minmax(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* h, int64_t ldh,
                                  float* out, int64_t ldo, float* cnt, int64_t ldc, int32_t n, int32_t f, int is_min);
/* Its gradient wrt h (TensorFlow's _UnsortedSegmentMinOrMaxGrad: the messages equal to the extremum share dy equally), from
 * the source side: rowptr_t / colidx_t is the TRANSPOSED operator (rows = sources, entries = their targets);
 * dh[s, c] = sum over targets t of [h[s, c] == out[t, c]] * dy[t, c] / cnt[t, c].  Deterministic (CSR order). */
GCNX_API int gcnx_spmm_csr_minmax_bwd(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const float* h, int64_t ldh,
                                      const float* out, int64_t ldo, const float* cnt, int64_t ldc, const float* dy, int64_t lddy,
                                      float* dh, int64_t lddh, int32_t n, int32_t f);

/* GeneralConv(aggregate = "prod") (tf.math.unsorted_segment_prod over the messages gather(h, a.indices[:,1]) of every target row,
 * SURVEY 8.A.4; adjacency values ignored): out[t, c] = product over the entries (t, s) of h[s, c], 1 for a row without entries
 * (TensorFlow's value for an empty segment).  aux (may be NULL; needed for the gradient): out where no message of the row is zero,
 * the product of the non-zero messages where exactly one is, 0 where two or more are. */
GCNX_API int gcnx_spmm_csr_prod(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* h, int64_t ldh, float* out,
                                int64_t ldo, float* aux, int64_t lda, int32_t n, int32_t f);
/* Its gradient wrt h (TensorFlow's _UnsortedSegmentProdGrad: out / h for a non-zero message, the product of the others for the only
 * zero message of a row, 0 where a row holds two or more zeros), from the source side: rowptr_t / colidx_t is the TRANSPOSED
 * operator; dh[s, c] = sum over targets t of dy[t, c] * (h[s, c] == 0 ? aux[t, c] : out[t, c] / h[s, c]).  Deterministic. */
GCNX_API int gcnx_spmm_csr_prod_bwd(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const float* h, int64_t ldh,
                                    const float* out, int64_t ldo, const float* aux, int64_t lda, const float* dy, int64_t lddy,
                                    float* dh, int64_t lddh, int32_t n, int32_t f);

/* ---- optimiser --------------------------------------------------------------------------- */
/* K9 Keras SGD without momentum (gcn.py:325,338): params -= lr * grads over a flat buffer. */
GCNX_API int gcnx_sgd(gcnx_ctx* ctx, float* params, const float* grads, int64_t n, float lr);
/* The learning rate of every update launch (gcnx_sgd, gcnx_gemm_dw_sgd, gcnx_gemm_dw2) read from a device scalar instead
 * of the `lr` argument (NULL: the argument again).  A learning rate passed by value is part of a captured launch; with a
 * source the same captured step serves every value of a schedule -- keras.optimizers.schedules.*, gcn.py:321-325 -- and
 * the host only rewrites 4 bytes (gcnx_h2d_async) when the value changes.  Not callable inside a capture. */
GCNX_API int gcnx_set_lr_source(gcnx_ctx* ctx, const float* lr_dev);

/* ---- optimisers with state (csrc/optim.hip) ---------------------------------- */
/* A step on one stream: gcnx_counter_add(t, 1) -> [gcnx_grad_sqnorm] -> gcnx_adam | gcnx_sgd_momentum.  The step count and
 * the clip factor stay on the device, so a captured step replays unchanged.  Both updates read the learning rate as
 * gcnx_sgd does (gcnx_set_lr_source) and never write g.  n == 0: nothing is launched. */
#define GCNX_OPTIM_MAX_PARTIALS 256
/* partials[b], b < n_partials (1 .. GCNX_OPTIM_MAX_PARTIALS): workgroup b's share of sum g[i]^2, fp32, in a fixed order without
 * atomics (an eager call and a graph replay give the same bits): thread j of workgroup b adds the rounded squares of
 * i = 256 b + j, + 256 n_partials, ... ascending from +0; a wave folds lane += lane + off for off = 32 .. 1; the four wave
 * sums are added as ((s0 + s1) + s2) + s3.  Not followed by a host read: the update launch finishes the sum. */
GCNX_API int gcnx_grad_sqnorm(gcnx_ctx* ctx, const float* g, int64_t n, float* partials, int32_t n_partials);
/* torch.optim.Adam / AdamW (decoupled weight_decay; 0: none) in one launch, t = *t_dev >= 1 already advanced for this step:
 *   s = clipnorm > 0 ? min(1, clipnorm / (sqrt(sum partials) + 1e-6)) : 1        (torch.nn.utils.clip_grad_norm_)
 *   g' = s g;  p = p (1 - lr weight_decay);  m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g' g'
 *   p = p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * Every workgroup folds the partials itself, in gcnx_grad_sqnorm's lane and wave order; workgroup 0 stores sqrt(sum) to
 * norm_out (may be NULL).  partials may be NULL when clipnorm <= 0 (then no norm is formed).  The bias corrections are formed
 * in fp64 from the fp32 betas, everything per element in fp32.  float4 accesses where p, g, m, v are 16-byte aligned.
 * GCNX_ERR_INVALID: NULL p / g / m / v / t_dev, n < 0, a beta outside [0, 1), n_partials > GCNX_OPTIM_MAX_PARTIALS. */
GCNX_API int gcnx_adam(gcnx_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t n, const uint32_t* t_dev, float lr,
                       float beta1, float beta2, float eps, float weight_decay, const float* partials, int32_t n_partials,
                       float clipnorm, float* norm_out);
/* tf.keras.optimizers.SGD(momentum, nesterov) (gcn.py:325): vel = momentum vel - lr g'; p += vel, with nesterov
 * p += momentum vel - lr g'.  Clipping, norm_out and the learning rate as in gcnx_adam; momentum in [0, 1). */
GCNX_API int gcnx_sgd_momentum(gcnx_ctx* ctx, float* p, const float* g, float* vel, int64_t n, float lr, float momentum,
                               int nesterov, const float* partials, int32_t n_partials, float clipnorm, float* norm_out);
/* A reduction that gcnx_dense_bwd_deferred left undone: column-sum partial rows -> cout[cf] and split-K slabs ->
 * out[total], both still in the caller's scratch buffer.  All zeros = nothing pending.  Plain data, no ownership. */
typedef struct gcnx_pending_reduce {
  const float* colpart; int64_t crows; int32_t cf; float* cout;
  const float* slabs; int64_t total; int32_t nsplit; float* out;
} gcnx_pending_reduce;

/* gcnx_dense_bwd with its second launch (the reductions that finish db_prev and dw) left to the caller: both are
 * gradient LEAVES that only the optimizer reads, so the step's last launch (gcnx_gemm_dw_sgd, `pending`) can fold
 * them in -- one launch fewer on the critical path of a small batch.  The partial results stay in `scratch`
 * (>= gcnx_dense_bwd_scratch_floats(ctx, n, fi, fo) floats, 16-byte aligned, untouched until then); db_prev / dw
 * are NOT valid until that call.  If the fused form does not apply (precision, shapes, scratch too small) this is
 * exactly gcnx_dense_bwd and *pending comes back all zeros. */
GCNX_API int64_t gcnx_dense_bwd_scratch_floats(gcnx_ctx* ctx, int64_t n, int32_t fi, int32_t fo);
GCNX_API int gcnx_dense_bwd_deferred(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* dh, int64_t lddh,
                            const float* w, int64_t n, int32_t fi, int32_t fo, int prec, float* dx, int64_t lddx,
                            const float* y_mask, int64_t ldy, float* db_prev, float* dw, float* scratch,
                            int64_t scratch_floats, gcnx_pending_reduce* pending);

/* The last gradient of a step and the optimizer apply as one call: gcnx_gemm_dw (dw = X^T dH, written into the flat
 * gradient buffer: grads <= dw, dw + fi*fo <= grads + n_params) followed by gcnx_sgd over all n_params parameters
 * (gcn.py:337-338: tape.gradient, then optimizer.apply_gradients).  Where dW is a split-K product its reduction
 * launch also applies the update (one launch instead of two); same dW and parameter bits as the two calls.
 * pending (may be NULL): a reduction left by gcnx_dense_bwd_deferred whose results lie in the same flat gradient
 * buffer; it is finished -- and its parameters updated -- by the same launch. */
GCNX_API int gcnx_gemm_dw_sgd(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* dh, int64_t lddh, float* dw,
                     int64_t n, int32_t fi, int32_t fo, int prec, float* params, float* grads, int64_t n_params,
                     float lr, const gcnx_pending_reduce* pending);

/* ---- GCNConv as one launch, small-feature regime (F <= 128; BASELINE config 2) --------------------------------
 * GCNConv.call (Spektral, the layer gcn.py:334 runs) is A (X W) + b; these entry points evaluate the same product
 * as (A X) W so that one workgroup owns 32 rows from the neighbour gather to the activation -- one launch per layer
 * instead of gcnx_gemm + gcnx_spmm_csr and no [N, F] intermediate between them.  Same results up to fp32 rounding
 * of the re-associated sum (tests: 1e-5 relative against the float64 oracle).
 * gcnx_gcn_conv_fused_ok: 1 if the shapes are served (fi in {32, 64, 128}, fo a multiple of 16 up to 128, ldx % 4 == 0,
 * n * ldx * 4 < 2^32); the entry points return GCNX_ERR_UNSUPPORTED otherwise -- use the two-launch form then. */
GCNX_API int gcnx_gcn_conv_fused_ok(int64_t n, int32_t fi, int32_t fo, int64_t ldx);
/* out[n, fo] = act((A x) w + bias), A in CSR (vals NULL: all ones); s (may be NULL) receives S = A x [n, fi], the
 * operand of the weight gradient dW = S^T dZ (gcnx_gemm_dw2).  wt_out (may be NULL) receives w^T [fo, fi], the layout
 * gcnx_gcn_conv_bwd_pool reads its weight operand fastest in.  act: GCNX_ACT_NONE / GCNX_ACT_RELU.  prec: GCNX_PREC_F32
 * (exact fp32 products on the fp32 MFMA) or GCNX_PREC_BF16X3 (split-bf16 on the bf16 MFMA); the gather is fp32 either way. */
GCNX_API int gcnx_gcn_conv_fwd(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals,
                      const float* x, int64_t ldx, int32_t n, int32_t fi, const float* w, int32_t fo,
                      const float* bias, int act, float* s, int64_t lds, float* out, int64_t ldo, float* wt_out,
                      int prec);
/* The same layer on a stored aggregate: out[n, fo] = act(s w + bias) with s = A x [n, fi] as gcnx_gcn_conv_fwd wrote it
 * (or as the loader gathered it: A x of a layer's INPUT is a constant of the batch).  No CSR, no gather, no S store; the
 * product and the epilogue are those of gcnx_gcn_conv_fwd operation for operation, so `out` is bit-identical to that
 * call's on the (A, x) that produced s.  Same shape and alignment rules (lds in the place of ldx): GCNX_ERR_UNSUPPORTED
 * otherwise. */
GCNX_API int gcnx_gcn_conv_fwd_pre(gcnx_ctx* ctx, const float* s, int64_t lds, int32_t n, int32_t fi, const float* w,
                      int32_t fo, const float* bias, int act, float* out, int64_t ldo, int prec);
/* gcnx_gcn_conv_fwd with the global pool's partial sums out of the same launch (GlobalSumPool / GlobalAvgPool over the
 * layer's output, gcn.py:334): node_graph [n] is the DisjointLoader id vector `i` (non-decreasing, values in [0, b)), b the
 * number of graphs.  Row t + g of tile_part / tile_cnt ((ceil(n / 32) + b) rows of fo floats each, 16-byte aligned) receives the
 * column sums / the number of positive entries of the rows of graph g inside the 32-row tile t; the other rows are not
 * written.  A graph's pooled sum is the sum of the rows t + g over its tiles t = first_row / 32 .. last_row / 32 --
 * gcnx_gcn_conv_bwd_pool(head) consumes them in that form. */
GCNX_API int gcnx_gcn_conv_fwd_pool(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals,
                      const float* x, int64_t ldx, int32_t n, int32_t fi, const float* w, int32_t fo,
                      const float* bias, int act, float* s, int64_t lds, float* out, int64_t ldo, float* wt_out,
                      int prec, const int32_t* node_graph, int32_t b, float* tile_part, float* tile_cnt);
/* gcnx_gcn_conv_fwd_pool that also writes the byte image of the ReLU output: mask8 [n, fo] uint8 (16-byte aligned,
 * ldmask8 >= fo a multiple of 16 bytes), mask8[r, c] = out[r, c] > 0 ? 1 : 0 -- what gcnx_gcn_conv_bwd_pool_mask8 gathers
 * in place of the fp32 rows.  act must be GCNX_ACT_RELU when mask8 is given; `out` may then be NULL: the fp32 activation
 * is not stored (s, wt_out and the pool's partial sums as usual).  mask8 == NULL: gcnx_gcn_conv_fwd_pool exactly. */
GCNX_API int gcnx_gcn_conv_fwd_mask8(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals,
                      const float* x, int64_t ldx, int32_t n, int32_t fi, const float* w, int32_t fo,
                      const float* bias, int act, float* s, int64_t lds, float* out, int64_t ldo, float* wt_out,
                      int prec, const int32_t* node_graph, int32_t b, float* tile_part, float* tile_cnt,
                      uint8_t* mask8, int64_t ldmask8);
/* The classifier head of a small-batch step whose pool is still in per-tile partial sums (plain data, no ownership).  In
 * a latency-bound step the pool and the head -- Dense(softmax) + CCE + their gradients on a [B, H] operand: 7 + 10 us of
 * little parallel work -- sit between the forward and the backward aggregation only because that needs dPooled.  With
 * this struct gcnx_gcn_conv_bwd_pool adds up the tile partials of its tile's graphs and evaluates dPooled itself (a few
 * hundred flops per graph), writing each graph's totals to pool_sum / pool_cnt on the way (the workgroup that holds the
 * graph's first row does; rows of graphs without nodes are NOT written: zero them beforehand if there can be any), and
 * gcnx_gemm_dw2 computes everything else the head produces (probabilities, loss, accuracy, dW, db, db_relu: leaves
 * nobody in the step waits for) from those totals in the FIRST workgroup of the weight-gradient launch.
 *   tile_part / tile_cnt: gcnx_gcn_conv_fwd_pool output, tile_rows = ceil(n / 32) + b rows of h floats
 *   pool_sum / pool_cnt [b, h]: written by gcnx_gcn_conv_bwd_pool, read by gcnx_gemm_dw2 (16-byte aligned)
 *   w [h, c], bias [c], y [b, c] one-hot; c <= 2 for the in-kernel form (gcnx_gcn_conv_bwd_pool returns
 *   GCNX_ERR_UNSUPPORTED beyond that; gcnx_gemm_dw2 takes any c the head kernel does)
 *   outputs (written by gcnx_gemm_dw2): probs [b, c], loss_acc [2] (mean loss, hit count), dw [h, c], db [c],
 *   db_relu [h] (may be NULL), pooled [b, h], dpooled [b, h]. */
typedef struct gcnx_head_args {
  const float* tile_part; const float* tile_cnt; int64_t tile_rows;
  float* pool_sum; float* pool_cnt;
  const int32_t* graph_ptr; int32_t b; int32_t h; int pool_mode;
  const float* w; const float* bias; const float* y; int32_t c; float denom; int cce_mode;
  float* probs; float* loss_acc; float* dw; float* db; float* db_relu; float* pooled; float* dpooled;
} gcnx_head_args;

/* Backward from the global pool down to the pre-activation gradient of the layer below, one launch:
 *   dZ2[j] = pool'(dpooled)[graph(j)] * [y2[j] > 0]                      (GlobalSumPool / GlobalAvgPool', ReLU')
 *   dz1    = ((A^T dZ2) w2^T) * [y1 > 0]                                 (aggregation', MatMul', ReLU' of layer 1)
 *   db1    = column sums of dz1                                          (BiasAddGrad)
 * rowptr_t / colidx_t / vals_t: A^T in CSR; node_graph: the DisjointLoader id vector i[n] (graph of every row);
 * w2 [f1, f2], or with w2_transposed != 0 its transpose [f2, f1] (the forward's wt_out: coalesced operand loads);
 * y2 [n, f2], y1 [n, f1]: the saved ReLU outputs.  dz2 (may be NULL) receives dZ2 [n, f2] (the operand
 * of dW2 = S2^T dZ2).  db1 (may be NULL): with `pending` and a scratch of >= gcnx_gcn_conv_bwd_scratch_floats(n, f1)
 * floats the per-tile partial sums stay in scratch and *pending describes the reduction (gcnx_gemm_dw2 finishes it);
 * otherwise db1 is complete on return.  mode: GCNX_POOL_SUM / GCNX_POOL_AVG.  head (may be NULL): see gcnx_head_args --
 * dpooled is then not read (may be NULL). */
GCNX_API int64_t gcnx_gcn_conv_bwd_scratch_floats(int64_t n, int32_t f1);
GCNX_API int gcnx_gcn_conv_bwd_pool(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const float* vals_t,
                      const float* y2, int64_t ldy2, const int32_t* node_graph, const int32_t* graph_ptr, int32_t b,
                      const float* dpooled, int64_t lddp, int mode, int32_t n, int32_t f2, const float* w2, int32_t f1,
                      int w2_transposed, const float* y1, int64_t ldy1, float* dz2, int64_t lddz2, float* dz1, int64_t lddz1, float* db1,
                      float* scratch, int64_t scratch_floats, gcnx_pending_reduce* pending, int prec,
                      const gcnx_head_args* head);
/* gcnx_gcn_conv_bwd_pool with y2 given as its byte image (gcnx_gcn_conv_fwd_mask8: 1 where y2 > 0; ldmask8 >= f2 a
 * multiple of 16 bytes, n * ldmask8 < 2^32): the launch only ever tests y2 for > 0, so it gathers a quarter of the bytes with
 * a quarter of the load instructions.  Every row is accumulated in the same order with the same operations: all outputs
 * equal those of the fp32-row form bit for bit. */
GCNX_API int gcnx_gcn_conv_bwd_pool_mask8(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const float* vals_t,
                      const uint8_t* y2_mask8, int64_t ldmask8, const int32_t* node_graph, const int32_t* graph_ptr, int32_t b,
                      const float* dpooled, int64_t lddp, int mode, int32_t n, int32_t f2, const float* w2, int32_t f1,
                      int w2_transposed, const float* y1, int64_t ldy1, float* dz2, int64_t lddz2, float* dz1, int64_t lddz1, float* db1,
                      float* scratch, int64_t scratch_floats, gcnx_pending_reduce* pending, int prec,
                      const gcnx_head_args* head);
/* Two weight gradients in one launch, dwa = xa^T dha [fia, foa] and dwb = xb^T dhb [fib, fob] over the same n rows
 * (MatMul grads wrt the kernels, gcn.py:337), both inside the flat gradient buffer `grads`; with params != NULL the
 * reduction launch also applies p -= lr * g to all n_params parameters and finishes `pending` (column sums left by
 * gcnx_gcn_conv_bwd_pool), as gcnx_gemm_dw_sgd does.  params == NULL: gradients only.  leaf (may be NULL): the classifier
 * head's outputs (gcnx_head_args) are computed by the first workgroups of the same launch; its gradients must lie in
 * `grads` too when params != NULL (they are updated with the rest). */
GCNX_API int gcnx_gemm_dw2(gcnx_ctx* ctx, const float* xa, int64_t ldxa, const float* dha, int64_t lddha, float* dwa,
                      int32_t fia, int32_t foa, const float* xb, int64_t ldxb, const float* dhb, int64_t lddhb,
                      float* dwb, int32_t fib, int32_t fob, int64_t n, int prec, float* params, float* grads,
                      int64_t n_params, float lr, const gcnx_pending_reduce* pending, const gcnx_head_args* leaf);

/* gcnx_gemm_dw2 for a layer under a SUM / AVG global pool, without dZ2.  There dZ2[r, j] = mask8[r, j] * dP[g(r), j]
 * (mask8 = [Y2 > 0] as bytes, gcnx_gcn_conv_fwd_mask8; dP[g] = dpooled[g], times 1 / rows of g for AVG), so
 *   dwb[k, j] = sum_g dP[g, j] * C_g[k, j],   C_g = xb[rows of g, :]^T mask8[rows of g, :].
 * C_g is formed on the bf16 MFMA from the exact split xb = hi + mid + lo (three bf16 numbers; every product with a 0 / 1
 * mask entry is exact, fp32 accumulation; entries of xb below 2^-110 in magnitude may lose their lo piece), per row slice
 * of a plan that never crosses a graph, and the reduction launch folds the slices' slabs with dP as a per-column scale
 * (one fmaf per slab).  dwa = xa^T dha exactly as gcnx_gemm_dw2 computes it; params / grads / lr / pending / leaf as
 * there (dpooled may be the array `leaf` writes: it is read by the reduction launch only).
 *   gcnx_dw2_slice_plan   host code, no device: cuts graph_ptr [b + 1] (host memory) into slices of at most kchunk rows
 *                         (kchunk a multiple of 32), cuts at multiples of kchunk from each graph's first row; writes
 *                         {row_begin, row_end, graph, bits of the float 1.0f / rows of the graph} (4 x int32) per slice into plan (cap slices; NULL:
 *                         count only) and returns the slice count, -1 on bad arguments.  The caller copies the table to
 *                         the device once per batch.
 *   gcnx_dw2_slices_ok    1 when nslices <= max(2 * ceil(n / kchunk), 64): many tiny graphs are refused
 *   gcnx_gemm_dw2_graph_kchunk   the rows per slice gcnx_gemm_dw2 would cut these shapes by
 *   gcnx_gemm_dw2_graph_ok       1 when gcnx_gemm_dw2_graph serves the call: fp32, SUM / AVG, foa % 4 == 0, fib in {64, 128},
 *                         fob % 64 == 0, the slice bound, and the tuning knob dw2_graph (GCNX_DW2_GRAPH=0: never)
 *   gcnx_gemm_dw2_graph   plan: the table on the device (16-byte aligned); mask8 rows ldmask8 bytes apart.  Returns
 *                         GCNX_ERR_UNSUPPORTED -- nothing launched, gcnx_last_error untouched -- for what _ok refuses,
 *                         unaligned xb, or a pending split-K record. */
GCNX_API int gcnx_dw2_slice_plan(const int32_t* graph_ptr, int32_t b, int64_t kchunk, int32_t* plan, int32_t cap);
GCNX_API int gcnx_dw2_slices_ok(int64_t n, int64_t kchunk, int32_t nslices);
GCNX_API int64_t gcnx_gemm_dw2_graph_kchunk(gcnx_ctx* ctx, int64_t n, int32_t fia, int32_t foa, int32_t fib, int32_t fob);
GCNX_API int gcnx_gemm_dw2_graph_ok(gcnx_ctx* ctx, int64_t n, int32_t fia, int32_t foa, int32_t fib, int32_t fob, int64_t kchunk,
                      int32_t nslices, int pool_mode, int prec);
GCNX_API int gcnx_gemm_dw2_graph(gcnx_ctx* ctx, const float* xa, int64_t ldxa, const float* dha, int64_t lddha, float* dwa,
                      int32_t fia, int32_t foa, const float* xb, int64_t ldxb, const uint8_t* mask8, int64_t ldmask8,
                      float* dwb, int32_t fib, int32_t fob, int64_t n, const int32_t* plan, int32_t nslices, int64_t kchunk,
                      const float* dpooled, int64_t lddp, int pool_mode, float* params, float* grads, int64_t n_params,
                      float lr, const gcnx_pending_reduce* pending, const gcnx_head_args* leaf);

/* ---- SAGEConv as one launch, small-feature regime (F <= 128) ---------------------------------------------------
 * The GraphSAGE layer the reference's torch model names as its next step ("consider using class SAGEConv instead",
 * gcn_utills.py:804-806): out = mean_{j in N(i)} x_j W_nb + x_i W_root + b, evaluated as [A x | x] [W_nb ; W_root] so that one
 * workgroup owns 32 rows from the neighbour gather to the bias -- one launch instead of gcnx_spmm_csr + two gcnx_gemm +
 * gcnx_add and no [N, F] intermediate between them.  fp32, exact fp32 products on the fp32 MFMA, no atomics: the same
 * bits on every call.  Nothing is allocated: the call can be captured.
 * gcnx_sage_conv_ok: 1 if the shapes are served (fi in {16, 32, 64, 128}, fo a multiple of 16 up to 128, ldx >= fi,
 * ldx % 4 == 0, n * ldx * 4 < 2^32); gcnx_sage_conv returns GCNX_ERR_UNSUPPORTED otherwise, and for x, w_nb, w_root, s or out
 * off a 16-byte boundary (lds >= fi, ldo >= fo, both multiples of 4 floats), with nothing launched -- use the four calls then. */
GCNX_API int gcnx_sage_conv_ok(int64_t n, int32_t fi, int32_t fo, int64_t ldx);
/* out[n, fo] = (A x) w_nb + x w_root + bias, A in CSR with per-entry vals (NULL: all ones) -- the row-mean operator and its
 * transpose are passed as values, like every other aggregation here.  bias may be NULL.  s (may be NULL) receives
 * S = A x [n, fi], the operand of dW_nb = S^T dZ (dW_root = x^T dZ: both are one gcnx_gemm_dw2).  A row without entries
 * gets an S row of exact zeros and out = x w_root + bias.  w_transposed == 0: both weights [fi, fo], row-major and
 * contiguous; w_transposed == 1: both [fo, fi] -- the layer's backward then passes its weights as stored:
 * dX = (A^T dZ) W_nb^T + dZ W_root^T is this call with x = dZ, A = the transposed operator, fi = the layer's output width
 * and fo = its input width.  n == 0 succeeds and writes nothing. */
GCNX_API int gcnx_sage_conv(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals,
                      const float* x, int64_t ldx, int32_t n, int32_t fi, const float* w_nb, const float* w_root,
                      int32_t fo, int w_transposed, const float* bias, float* s, int64_t lds, float* out, int64_t ldo);

/* ---- GINConv: sum aggregation + two-layer MLP as one launch, small-feature regime (widths <= 128) ----------------------
 * The Graph Isomorphism Network convolution (PyG GINConv(Sequential(Linear, ReLU, Linear)), Spektral GINConv(mlp_hidden)) for
 * the slot the reference's author left open (gcn_utills.py:804-806):
 *     T = (1 + *eps) x + A x                 A = the stored pattern as all ones: values are not an operand
 *     U = relu(T w_a + b_a)                  [n, k1]
 *     out = U w_b + b_b                      [n, k2]
 * One workgroup owns 32 rows from the neighbour gather to the second bias: two chained fp32 MFMA products behind the gather,
 * the first one's accumulators handed over through an LDS tile -- one launch instead of gcnx_gin_aggregate + two gcnx_gemm
 * and no [N, F] intermediate between them.  Exact fp32 products, no atomics, every row summed in CSR order from +0: the same
 * bits on every call.  Nothing is allocated: the call can be captured.
 * gcnx_gin_conv_ok: 1 if the shapes are served (k0 in {16, 32, 64, 128}, k1 a multiple of 16 up to 128, k2 = 0 (single
 * stage) or a multiple of 16 up to 128, ldx >= k0, ldx % 4 == 0, n * ldx * 4 < 2^32). */
GCNX_API int gcnx_gin_conv_ok(int64_t n, int32_t k0, int32_t k1, int32_t k2, int64_t ldx);
/* eps: DEVICE pointer to one float (NULL: 0) -- it lives in the model's flat parameter buffer, so optimizers and captured
 * steps see its updates without a host round trip.  b_a, b_b may be NULL.  t [n, k0] and u [n, k1] (may be NULL) receive
 * T and U: the operands of dW_a = T^T dU and dW_b = U^T dZ; U is also the ReLU mask.  A row without entries has
 * T = (1 + eps) x exactly.  Rows of the last tile at or past n are never stored.
 * Single stage: w_b == NULL and k2 == 0 gives out [n, k1] = T w_a (+ b_a) with no ReLU; u and b_b must then be NULL.
 * w_transposed == 0: w_a [k0, k1], w_b [k1, k2], row-major and contiguous; w_transposed == 1: w_a [k1, k0], w_b [k2, k1] --
 * the layer's backward then passes its weights as stored: dX = ((1 + eps) dU + A^T dU) W_a^T is the single-stage call on the
 * transposed pattern with x = dU, k0 = the layer's hidden width and k1 = its input width.
 * GCNX_ERR_UNSUPPORTED, with nothing launched or written: shapes gcnx_gin_conv_ok refuses; x, w_a, w_b, t, u or out off a
 * 16-byte boundary; ldt < k0, ldu < k1, ldo < the width of out, or one of them not a multiple of 4 floats -- use
 * gcnx_gin_aggregate + gcnx_gemm then.  GCNX_ERR_INVALID: a negative size, w_b / k2 not given together, u or b_b given without
 * a second stage, a NULL mandatory pointer (rowptr, colidx, x, w_a, out), outputs that alias x or each other.
 * n == 0 succeeds and writes nothing. */
GCNX_API int gcnx_gin_conv(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* x, int64_t ldx, int32_t n,
                      int32_t k0, const float* eps, const float* w_a, const float* b_a, int32_t k1, const float* w_b,
                      const float* b_b, int32_t k2, int w_transposed, float* t, int64_t ldt, float* u, int64_t ldu, float* out,
                      int64_t ldo);
/* out[n, f] = (1 + *eps) x + A x for ANY f >= 1 and any leading dimensions >= f (eps: device pointer, NULL = 0): the first step
 * of the composed route, the route for widths gcnx_gin_conv refuses and, on the transposed pattern, the last step of the
 * composed backward.  float4 lanes when f % 4 == 0 and x, out, ldx, ldo allow 16-byte accesses (then the bits of
 * gcnx_gin_conv's t), scalar lanes otherwise.  Every row is written; a row's entries are added in CSR order from +0:
 * deterministic.  out must not alias x (GCNX_ERR_INVALID, as for f < 1, ld < f, negative n or NULL pointers).  n == 0
 * succeeds and writes nothing. */
GCNX_API int gcnx_gin_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* x, int64_t ldx,
                      const float* eps, float* out, int64_t ldo, int32_t n, int32_t f);
/* *deps = sum_i <x_i, dt_i> over the n rows of x, dt [n, f]: the gradient with respect to eps from dT = dU W_a^T.  Written,
 * never accumulated; n == 0 writes 0.  Two launches, no atomics, a fixed summation order: workgroup g sums rows
 * [64 g, 64 g + 64) into parts[g], then one workgroup sums the parts.  parts: caller-provided room for (n + 63) / 64 floats
 * (may be NULL when n == 0); deps: device pointer to one float. */
GCNX_API int gcnx_gin_eps_grad(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* dt, int64_t lddt, int64_t n, int32_t f,
                      float* parts, float* deps);

/* ---- GINEConv: GINConv whose neighbour sum reads the edge features, small-feature regime (widths <= 128) ----------------
 * PyG's GINEConv(nn = Sequential(Linear, ReLU, Linear), eps, train_eps, edge_dim): the cheapest way to put the dca /
 * proximity features the reference computes on every contact and bridge and its model drops (gcn_utills.py:319-443;
 * gcn.py:71) into a message -- one add and one ReLU per gathered element, no softmax, no gate, no weight matrix per edge.
 * CSR row i is the target, its stored entries j are the sources.  Values are ignored; the pattern and e are used as stored: no
 * loop is added or removed, a stored self-loop is one more neighbour with its own features.  e [nnz, edge_dim] (lde) holds the
 * entries' features in the CSR's entry order, w_e [edge_dim, k0] and b_e [k0] (may be NULL) are PyG's lin, 1 <= edge_dim <= 8.
 * Per entry and channel c, in fp32, EXACTLY as written (contract; every product and every sum rounded on its own, no FMA):
 *     t = rn(e[0] w_e[0,c]);  t = rn(t + rn(e[d] w_e[d,c]))  for d = 1 .. edge_dim - 1, in that order
 *     v = rn(t + b_e[c])          (b_e NULL: v = t)
 *     m = rn(x_j[c] + v)          msg = m > 0 ? m : 0     (the positive side is m > 0; m == 0 is the zero side, gradient 0)
 * m is stored nowhere: gcnx_gine_conv, gcnx_gine_aggregate, gcnx_gine_bwd_edges and gcnx_gine_bwd_nodes recompute it and
 * therefore agree on the side of every kink, and float32 arithmetic on the stored operands reproduces it.  Forward:
 *     S_i = sum_j msg_ij          in CSR order from +0
 *     T_i = fma(1 + *eps, x_i, S_i)       (a row without entries has T = (1 + eps) x exactly)
 *     U = relu(T w_a + b_a)  [n, k1]      out = U w_b + b_b  [n, k2]
 * Backward, with dT = dU w_a^T (gcnx_gemm_dx) and g_ij = dT_i * [m_ij > 0]:
 *     db_e = sum_ij g_ij     dw_e[d,:] = sum_ij e_ij[d] g_ij     dx_j = (1 + eps) dT_j + sum_{i : j in N(i)} g_ij
 *     d eps = sum_i <x_i, dT_i>   (gcnx_gin_eps_grad)
 * fp32, no float atomics, fixed summation order: the same bits on every call.  Nothing is allocated: every call can be
 * captured.  n == 0 succeeds and writes nothing (gcnx_gine_bwd_edges then writes zeros to its two gradients); negative sizes,
 * NULL mandatory pointers and aliasing are GCNX_ERR_INVALID, as are edge_dim outside 1 .. 8 and lde < edge_dim on the
 * any-width calls.
 * gcnx_gine_conv_ok (gcn.py:71): 1 if gcnx_gine_conv serves the shapes: k0 in {16, 32, 64, 128}, k1 and k2 multiples of 16 up
 * to 128 (k2 >= 16: there is no single-stage form), ldx >= k0, ldx % 4 == 0, n * ldx * 4 < 2^32, 1 <= edge_dim <= 8. */
GCNX_API int gcnx_gine_conv_ok(int64_t n, int32_t k0, int32_t k1, int32_t k2, int64_t ldx, int32_t edge_dim);
/* gcn.py:71 -- the convolution as ONE launch: gcnx_gin_conv's workgroup (32 rows from the gather to the second bias, two
 * chained fp32 MFMA products through LDS tiles) whose gather forms relu(x_j + e_ij w_e + b_e) per entry before the add.
 * eps: DEVICE pointer to one float (NULL: 0).  b_e, b_a, b_b may be NULL.  t [n, k0] and u [n, k1] (may be NULL) receive T and
 * U: the operands of dW_a = T^T dU and dW_b = U^T dZ; U is also the inner ReLU mask.  Rows of the last tile at or past n are
 * never stored.  A tile of 32 rows must hold fewer than 2^32 / (4 lde) entries.
 * GCNX_ERR_UNSUPPORTED, with nothing launched or written: shapes gcnx_gine_conv_ok refuses; x, w_e, b_e, w_a, w_b, t, u or out
 * off a 16-byte boundary; ldt < k0, ldu < k1, ldo < k2, or one of them not a multiple of 4 floats -- use gcnx_gine_aggregate +
 * gcnx_gemm then.  GCNX_ERR_INVALID: a negative size, lde < edge_dim, a NULL mandatory pointer (rowptr, colidx, x, e, w_e,
 * w_a, w_b, out), outputs that alias x or each other. */
GCNX_API int gcnx_gine_conv(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* x, int64_t ldx, int32_t n,
                      int32_t k0, const float* eps, const float* e, int64_t lde, int32_t edge_dim, const float* w_e,
                      const float* b_e, const float* w_a, const float* b_a, int32_t k1, const float* w_b, const float* b_b,
                      int32_t k2, float* t, int64_t ldt, float* u, int64_t ldu, float* out, int64_t ldo);
/* gcn.py:71 -- out [n, f] = T alone for ANY f >= 1 and any leading dimensions >= f (w_e [edge_dim, f], b_e [f] or NULL): the
 * first step of the composed route (then gcnx_gemm(relu), gcnx_gemm) and the route for every shape gcnx_gine_conv refuses.
 * float4 lanes when f % 4 == 0 and x, out, w_e, b_e, ldx, ldo allow 16-byte accesses (then the bits of gcnx_gine_conv's t),
 * scalar lanes otherwise.  Every row is written.  out must not alias x. */
GCNX_API int gcnx_gine_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* x, int64_t ldx,
                      const float* eps, const float* e, int64_t lde, int32_t edge_dim, const float* w_e, const float* b_e,
                      float* out, int64_t ldo, int32_t n, int32_t f);
/* gcn.py:71 -- floats of caller scratch gcnx_gine_bwd_edges needs (per-workgroup parts of db_e | dw_e; 0 for sizes it refuses). */
GCNX_API int64_t gcnx_gine_bwd_scratch_floats(int64_t n, int32_t k0, int32_t edge_dim);
/* gcn.py:71 -- backward, the pass over the forward CSR: dw_e [edge_dim, f] and db_e [f] (may be NULL) from x, e, w_e, b_e and
 * dt = dT [n, f] (lddt), any f >= 1 (float4 lanes where the operands allow them, scalar lanes otherwise).  The sums go through
 * per-workgroup parts in scratch (32 rows each, row-then-entry order inside a workgroup) and a second small launch inside this
 * call that adds the parts in a fixed order: no atomics, the same bits on every call.  Written, never accumulated. */
GCNX_API int gcnx_gine_bwd_edges(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* x, int64_t ldx,
                      const float* e, int64_t lde, int32_t edge_dim, const float* w_e, const float* b_e, const float* dt,
                      int64_t lddt, int32_t n, int32_t f, float* dw_e, float* db_e, float* scratch);
/* gcn.py:71 -- backward, the pass over the transposed pattern (rowptr_t, colidx_t, perm_t of gcnx_csr_transpose_perm:
 * perm_t[p] = the forward entry behind entry p; needed for a symmetric pattern too, since e is read in the forward entry order
 * through perm_t).  For source row j, with m recomputed from x_j and e[perm_t[p]]:
 *     dx_j = fma(1 + *eps, dT_j, sum_p [m > 0] dT_{colidx_t[p]})            the sum in the transposed pattern's order from +0
 * Any f >= 1.  dx (lddx) must not alias dt or x. */
GCNX_API int gcnx_gine_bwd_nodes(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const int32_t* perm_t,
                      const float* x, int64_t ldx, const float* eps, const float* e, int64_t lde, int32_t edge_dim,
                      const float* w_e, const float* b_e, const float* dt, int64_t lddt, float* dx, int64_t lddx, int32_t n,
                      int32_t f);

/* ---- PNAConv: mean, min, max and std of the neighbours' messages from one gather ------------------------------------------
 * PyG's PNAConv(aggregators = [mean, min, max, std], scalers = [identity, amplification, attenuation], deg, towers = 1,
 * pre_layers = post_layers = 1, divide_input = False, edge_dim = None, train_norm = False).  CSR row i is the target, its
 * stored entries j are the sources; values are not an operand, no self-loop is added or removed.  The message
 * M_ij = [x_i | x_j] W_pre + b_pre is linear, so the caller forms it per node: pq [n, 2f] = P | Q with
 * P = x W_pre[:f] + b_pre and Q = x W_pre[f:] (column views of one array), M_ij = P_i + Q_j.  With d_i the number of stored
 * entries of row i and delta = avg_deg_log (the mean of log(d + 1) over the training set's nodes; > 0):
 *     A_i = [ P_i + mean_j Q_j | P_i + min_j Q_j | P_i + max_j Q_j | sqrt(relu(var_j Q_j) + 1e-5) ]   (biased variance)
 *     d_i = 0:  A_i = [ 0 | 0 | 0 | sqrt(1e-5) ]                                                      (PyG's scatter)
 *     c_i = [ x_i | A_i | s_amp,i A_i | s_att,i A_i ]        s_amp,i = log(max(d_i, 1) + 1) / delta,  s_att,i = 1 / s_amp,i
 * c is [n, 13f]: scaler-major, aggregator-minor, x in front, as PyG concatenates.  All 13 blocks are written, the copy of x
 * included.  stats (may be NULL: evaluation) receives [n, 6f] = meanQ | minQ | maxQ | std | cmin | cmax for the backward;
 * cmin / cmax count the entries of the row that attain the extremum, per column (as floats); a row without entries stores
 * 0 | 0 | 0 | sqrt(1e-5) | 0 | 0.  c holds the same bits with and without stats.
 * One pass gathers each Q row once.  The variance is formed on values shifted by the row's first gathered entry K:
 * s1 = sum (Q_j - K), s2 = sum (Q_j - K)^2, meanQ = K + s1 / d, var = s2 / d - (s1 / d)^2, and is 0 exactly where the
 * row's minimum equals its maximum (so a d = 1 row has std = sqrt(1e-5f) to the bit).  fp32, no atomics, every sum in CSR
 * order: the same bits on every call.  Any f >= 1 and any leading dimensions (ldx >= f, ldpq >= 2f, ldc >= 13f, lds >= 6f):
 * float4 lanes when f % 4 == 0 and x, pq, c, stats and their leading dimensions allow 16-byte accesses, scalar lanes
 * otherwise.  Rows of any length.  GCNX_ERR_INVALID: f < 1, a negative n, a small leading dimension, avg_deg_log <= 0, a NULL
 * mandatory pointer, outputs that alias an input or each other.  n == 0 succeeds and writes nothing. */
GCNX_API int gcnx_pna_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* x, int64_t ldx,
                      const float* pq, int64_t ldpq, float avg_deg_log, float* c, int64_t ldc, float* stats, int64_t lds,
                      int32_t n, int32_t f);
/* *out = the floats of scratch gcnx_pna_bwd needs for n rows of width f (4 n f: four coefficient rows per target). */
GCNX_API int gcnx_pna_bwd_scratch_floats(int64_t n, int32_t f, int64_t* out);
/* The backward of gcnx_pna_aggregate with respect to P and Q: dpq [n, 2f] = dP | dQ from dc [n, 13f] = dLoss / dc.  Block 0
 * of dc (the gradient that reaches x directly) is neither read nor written: it stays the caller's.  rowptr / colidx: the
 * forward pattern (only its degrees are read); rowptr_t / colidx_t: its transpose (rows = sources, entries = their targets);
 * pq and stats: what the forward read and wrote.  Two launches, no atomics:
 *   per target i   (g_mean, g_min, g_max, g_std) = dc_id + s_amp,i dc_amp + s_att,i dc_att;
 *                  dP_i = g_mean + g_min + g_max (0 for d_i = 0); four coefficient rows into scratch
 *   per source j   dQ_j = sum over the targets i of row j of the transposed pattern, in its stored order, of
 *                  g_mean,i / d_i + g_min,i [Q_j = minQ_i] / cmin_i + g_max,i [Q_j = maxQ_i] / cmax_i
 *                  + g_std,i [var_i > 0] (Q_j - meanQ_i) / (d_i std_i)
 * Ties share the gradient evenly, as torch.scatter_reduce("amin" / "amax") does; [var_i > 0] is [maxQ_i > minQ_i].
 * scratch: gcnx_pna_bwd_scratch_floats(n, f) floats, 16-byte aligned for the float4 lanes.  Same widths, leading dimensions
 * and errors as the forward (lddc >= 13f, lddpq >= 2f); dpq and scratch must not alias an input or each other. */
GCNX_API int gcnx_pna_bwd(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const int32_t* rowptr_t,
                      const int32_t* colidx_t, const float* pq, int64_t ldpq, const float* stats, int64_t lds, const float* dc,
                      int64_t lddc, float avg_deg_log, float* dpq, int64_t lddpq, float* scratch, int32_t n, int32_t f);

/* ---- GATConv: edge-softmax attention, small-feature regime (heads * c <= 128) -------------------------------------
 * PyG's GATConv(in, c, heads, concat=True, negative_slope, dropout=0, bias=True), the attention layer for the slot the
 * reference's author marked as open ("consider using class SAGEConv instead", gcn_utills.py:804-806).  CSR row i is the
 * target, its stored entries j the sources, values are ignored.  With Hf = x W [n, heads * c] from gcnx_gemm (head h owns
 * columns [h c, h c + c)):
 *     a_src[j,h] = <Hf[j,h,:], att_src[h,:]>   a_dst[i,h] = <Hf[i,h,:], att_dst[h,:]>
 *     z = a_src[j,h] + a_dst[i,h] (one fp32 add)   e = z > 0 ? z : slope z   alpha = exp(e - m_i) / l_i (m: row max, l: row sum)
 *     O[i,h,:] = sum_j alpha Hf[j,h,:]   out = O + bias   (a row without entries: O = 0, out = bias)
 * fp32, no float atomics, fixed summation order: the same bits on every call, eager or replayed from a captured graph.
 * Nothing is allocated.  32 rows per workgroup, heads * c / 4 lanes per row; 1024 CSR entries of a tile are staged in LDS,
 * longer tiles read the rest from global memory.
 * gcnx_gat_conv_ok (gcn_utills.py:804-806): 1 if the shapes are served: heads in {1, 2, 4, 8}, heads * c in {16, 32, 64, 128},
 * c >= 4, ldh >= heads * c, ldh % 4 == 0, n * ldh * 4 < 2^32.  Every call below returns GCNX_ERR_UNSUPPORTED otherwise (ldh: the
 * leading dimension of the operand it gathers), and for float4 operands off a 16-byte boundary or leading dimensions that
 * are not multiples of 4 floats >= heads * c, with nothing launched and nothing written.  n == 0 succeeds and writes
 * nothing; negative sizes and NULL mandatory pointers are GCNX_ERR_INVALID. */
GCNX_API int gcnx_gat_conv_ok(int64_t n, int32_t heads, int32_t c, int64_t ldh);
/* gcn_utills.py:804-806 -- a_src, a_dst [n, heads] from hf [n, heads * c] (ldh) and att_src, att_dst [heads, c]: one pass over hf. */
GCNX_API int gcnx_gat_scores(gcnx_ctx* ctx, const float* hf, int64_t ldh, int32_t n, int32_t heads, int32_t c,
                       const float* att_src, const float* att_dst, float* a_src, float* a_dst);
/* gcn_utills.py:804-806 -- out [n, heads * c] (ldo) = softmax-weighted gather + bias (bias may be NULL).  alpha [nnz, heads]
 * (may be NULL: not stored) receives the attention coefficients in the CSR's entry order; o_pre (ldp; may be NULL) receives
 * O, the result before the bias -- without it the backward takes out and bias.  The row maximum is subtracted before the
 * exponential: no score overflows, no row divides 0 by 0. */
GCNX_API int gcnx_gat_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* hf, int64_t ldh,
                       int32_t n, int32_t heads, int32_t c, const float* a_src, const float* a_dst, const float* bias,
                       float slope, float* out, int64_t ldo, float* alpha, float* o_pre, int64_t ldp);
/* gcn_utills.py:804-806 -- backward, the pass over the forward CSR.  d_out = dLoss/dout [n, heads * c] (ldd); o (ldo) is O, or
 * out with o_bias = the bias that was added (O = o - o_bias).  With r[i,h] = <d_out[i,h,:], O[i,h,:]>:
 *     dz[e,h] = alpha[e,h] (<d_out[i,h,:], hf[j,h,:]> - r[i,h]) (z > 0 ? 1 : slope)      da_dst[i,h] = sum over the row of dz
 * dz [nnz, heads] in the CSR's entry order, da_dst [n, heads].  a_src / a_dst decide the side of z only. */
GCNX_API int gcnx_gat_bwd_edges(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* hf, int64_t ldh,
                       int32_t n, int32_t heads, int32_t c, const float* a_src, const float* a_dst, float slope,
                       const float* alpha, const float* d_out, int64_t ldd, const float* o, int64_t ldo, const float* o_bias,
                       float* dz, float* da_dst);
/* gcn_utills.py:804-806 -- floats of caller scratch gcnx_gat_bwd_nodes needs (per-workgroup parts of datt_src / datt_dst). */
GCNX_API int64_t gcnx_gat_bwd_scratch_floats(int64_t n, int32_t heads, int32_t c);
/* gcn_utills.py:804-806 -- backward, the pass over the transposed pattern (rowptr_t, colidx_t, perm_t of
 * gcnx_csr_transpose_perm: perm_t[p] = the forward entry behind entry p; needed for a symmetric pattern too):
 *     dhf[j,h,:] = sum_i alpha[ij,h] d_out[i,h,:] + da_src[j,h] att_src[h,:] + da_dst[j,h] att_dst[h,:]     da_src[j,h] = sum_i dz[ij,h]
 *     datt_src[h,:] = sum_j da_src[j,h] hf[j,h,:]      datt_dst[h,:] = sum_j da_dst[j,h] hf[j,h,:]
 * dhf [n, heads * c] (ldg), da_src [n, heads], datt_src / datt_dst [heads, c].  The datt sums go through per-workgroup parts in
 * scratch and a second small launch inside this call (fixed order, no atomics).  dbias, dW and dx of the layer are
 * gcnx_act_bias_grad, gcnx_gemm_dw and gcnx_gemm_dx. */
GCNX_API int gcnx_gat_bwd_nodes(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const int32_t* perm_t,
                       int32_t n, int32_t heads, int32_t c, const float* alpha, const float* dz, const float* d_out, int64_t ldd,
                       const float* hf, int64_t ldh, const float* da_dst, const float* att_src, const float* att_dst,
                       float* dhf, int64_t ldg, float* da_src, float* datt_src, float* datt_dst, float* scratch);

/* ---- GATv2Conv: attention whose scores read the edge features, small-feature regime (heads * c <= 128) ---------------
 * PyG's GATv2Conv(in, c, heads, concat=True, negative_slope, dropout=0, add_self_loops=False, edge_dim, bias=True,
 * share_weights=False) (Brody et al.): the LeakyReLU comes before the dot with att, so the score depends jointly on target,
 * source and edge -- the layer that can weigh an entry by the dca / proximity features the reference computes and its model
 * drops (gcn_utills.py:319-443; gcn.py:71).  CSR row i is the target, its stored entries j the sources, values are ignored,
 * the pattern and e are used as stored.  xlr = Xl | Xr [n, 2 heads c] (ldx) is ONE array from one gcnx_gemm with the stacked
 * weight and bias (head h owns columns [h c, h c + c) of each half); e [nnz, edge_dim] (lde) holds the entries' features in
 * the CSR's entry order, w_e [edge_dim, heads c], att [heads, c]:
 *     t_ij[h,c] = sum_d e_ij[d] w_e[d, h c + c]     s_ij = (Xl[j] + Xr[i]) + t_ij     g = s > 0 ? s : slope s
 *     score_ij,h = <att[h,:], g_ij[h,:]>   alpha = softmax over the stored entries of row i   O[i,h,:] = sum_j alpha Xl[j,h,:]
 *     out = O + bias      (a row without entries: O = 0, out = bias)
 * s is stored nowhere; every kernel recomputes it in fp32 EXACTLY as written (contract): t starts from the rounded product
 * of d = 0 and adds the separately rounded products of d = 1 .. edge_dim - 1 in that order (no FMA; edge_dim = 0: t = 0), one
 * add forms Xl + Xr, one more adds t; the positive side is s > 0.  All kernels therefore agree on the side of every kink,
 * and float32 arithmetic on the stored operands reproduces it.
 * fp32, no float atomics, fixed summation order: the same bits on every call.  Nothing is allocated.
 * gcnx_gatv2_conv_ok (gcn.py:71): 1 if the shapes are served: heads in {1, 2, 4, 8}, heads * c in {16, 32, 64, 128}, c >= 4,
 * ldx >= 2 heads c, ldx % 4 == 0, n * ldx * 4 < 2^32, 0 <= edge_dim <= 8.  Every call below returns GCNX_ERR_UNSUPPORTED
 * otherwise, and for float4 operands (everything but e, alpha, dscore and the index arrays) off a 16-byte boundary or leading
 * dimensions that are not multiples of 4 floats >= heads * c, with nothing launched and nothing written.  n == 0 succeeds and
 * writes nothing; negative sizes and NULL mandatory pointers are GCNX_ERR_INVALID; e, w_e (and dw_e) may be NULL only with
 * edge_dim == 0. */
GCNX_API int gcnx_gatv2_conv_ok(int64_t n, int32_t heads, int32_t c, int64_t ldx, int32_t edge_dim);
/* gcn.py:71 -- out [n, heads * c] (ldo) = softmax-weighted sum of Xl over the row's entries + bias (bias may be NULL), from ONE
 * gather of Xl[j] per entry: a running row maximum with a rescaled accumulator (one rescale per four entries, CSR order);
 * the maximum is subtracted before every exponential and the row sum is >= 1: no overflow, no 0 / 0.  alpha [nnz, heads]
 * (may be NULL) receives the attention coefficients in the CSR's entry order, o_pre (ldp; may be NULL) O before the bias
 * (the backward needs both). */
GCNX_API int gcnx_gatv2_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* xlr, int64_t ldx,
                       int32_t n, int32_t heads, int32_t c, const float* e, int64_t lde, int32_t edge_dim, const float* w_e,
                       const float* att, const float* bias, float slope, float* out, int64_t ldo, float* alpha, float* o_pre,
                       int64_t ldp);
/* gcn.py:71 -- floats of caller scratch gcnx_gatv2_bwd_edges needs (per-workgroup parts of datt | dw_e). */
GCNX_API int64_t gcnx_gatv2_bwd_scratch_floats(int64_t n, int32_t heads, int32_t c, int32_t edge_dim);
/* gcn.py:71 -- backward, the pass over the forward CSR.  d_out = dLoss/dout [n, heads * c] (ldd), o (ldo) = O as o_pre
 * received it.  With r[i,h] = <d_out[i,h,:], O[i,h,:]>:
 *     dscore[ij,h] = alpha[ij,h] (<d_out[i,h,:], Xl[j,h,:]> - r[i,h])       ds_ij = dscore att (s > 0 ? 1 : slope)
 *     dxr[i] = sum_j ds_ij     datt[h,:] = sum_ij dscore g_ij[h,:]     dw_e[d,:] = sum_ij e_ij[d] ds_ij
 * dscore [nnz, heads] in the CSR's entry order, dxr [n, heads * c] (ldg: e.g. the right half of a dXl | dXr array), datt
 * [heads, c], dw_e [edge_dim, heads * c].  The datt / dw_e sums go through per-workgroup parts in scratch (row-then-entry
 * order inside a workgroup) and a second small launch inside this call (fixed order, no atomics). */
GCNX_API int gcnx_gatv2_bwd_edges(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* xlr, int64_t ldx,
                       int32_t n, int32_t heads, int32_t c, const float* e, int64_t lde, int32_t edge_dim, const float* w_e,
                       const float* att, float slope, const float* alpha, const float* d_out, int64_t ldd, const float* o,
                       int64_t ldo, float* dscore, float* dxr, int64_t ldg, float* datt, float* dw_e, float* scratch);
/* gcn.py:71 -- backward, the pass over the transposed pattern (rowptr_t, colidx_t, perm_t of gcnx_csr_transpose_perm:
 * perm_t[p] = the forward entry behind entry p; needed for a symmetric pattern too).  alpha, dscore and e are read in the
 * forward entry order through perm_t:
 *     dxl[j] = sum_i (alpha[ij] d_out[i] + ds_ij)                 [n, heads * c] (ldg: e.g. the left half of dXl | dXr)
 * dW, db and dx of the layer are gcnx_gemm_dw, gcnx_act_bias_grad and gcnx_gemm_dx on dXl | dXr. */
GCNX_API int gcnx_gatv2_bwd_nodes(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const int32_t* perm_t,
                       const float* xlr, int64_t ldx, int32_t n, int32_t heads, int32_t c, const float* e, int64_t lde,
                       int32_t edge_dim, const float* w_e, const float* att, float slope, const float* alpha,
                       const float* dscore, const float* d_out, int64_t ldd, float* dxl, int64_t ldg);

/* ---- ResGatedGraphConv: per-channel sigmoid edge gates, small-feature regime (h <= 128) --------------------------------
 * PyG's ResGatedGraphConv(in, h, act=Sigmoid(), edge_dim, root_weight, bias) (Bresson & Laurent's GatedGCN), aggr = add: each
 * message is multiplied channel by channel by a gate that reads target, source and edge together -- the gated, per-channel
 * way to use the dca / proximity features the reference computes and its model drops (gcn_utills.py:319-443; gcn.py:71).
 * No softmax: a row's messages do not compete.  CSR row i is the target, its stored entries j the sources, values are
 * ignored, no self-loops are added, the pattern and e are used as stored.  p = K | Q | V [n, >= 3 h] (ldp) is ONE array from one
 * gcnx_gemm with the stacked weight and bias (x [W_k | W_q | W_v | W_s] + [b_k | b_q | b_v | 0]: the node halves of PyG's
 * lin_key / lin_query / lin_value, and lin_skip behind them); e [nnz, edge_dim] (lde) holds the entries' features in the
 * CSR's entry order, w_e [edge_dim, 3 h] = W_ke | W_qe | W_ve the edge halves of the three Linears:
 *     a_ij = K[i] + Q[j] + sum_d e_ij[d] (W_ke[d] + W_qe[d])    g_ij = sigmoid(a_ij)    m_ij = V[j] + sum_d e_ij[d] W_ve[d]
 *     out[i] = S[i] + bias + sum_j g_ij * m_ij                  (a row without entries: out = S[i] + bias)
 * and with dO = dLoss/dout:
 *     da_ij = dO[i] * m_ij * g_ij (1 - g_ij)        dm_ij = dO[i] * g_ij
 *     dK[i] = sum_j da_ij      dS = dO      dbias = column sums of dO
 *     dQ[j] = sum_i da_ij      dV[j] = sum_i dm_ij                          (over the transposed pattern)
 *     dW_ke[d] = dW_qe[d] = sum_ij e_ij[d] da_ij      dW_ve[d] = sum_ij e_ij[d] dm_ij
 * g and m are stored nowhere: the backward recomputes them.  sigmoid(a) = 1 / (1 + exp(-a)) with the overflow to inf
 * resolving to 0: every finite a gives a finite g in [0, 1] and a finite g (1 - g), no 0 * inf, no NaN.
 * fp32, no float atomics, fixed summation order: the same bits on every call.  Nothing is allocated.
 * gcnx_resgated_conv_ok (gcn.py:71): 1 if the shapes are served: h in {16, 32, 64, 128}, 0 <= edge_dim <= 8, ldp % 4 == 0,
 * ldp >= 3 h, n * ldp * 4 < 2^32.  Every call below returns GCNX_ERR_UNSUPPORTED otherwise, and for float4 operands
 * (everything but e and the index arrays) off a 16-byte boundary or leading dimensions that are not multiples of 4 floats
 * >= their width, with nothing launched and nothing written.  n == 0 succeeds and writes nothing; negative sizes and NULL
 * mandatory pointers are GCNX_ERR_INVALID; e, w_e (and dw_e, scratch) may be NULL only with edge_dim == 0. */
GCNX_API int gcnx_resgated_conv_ok(int64_t n, int32_t h, int64_t ldp, int32_t edge_dim);
/* gcn.py:71 -- out [n, h] (ldo) from ONE gather of the contiguous Q[j] | V[j] per entry, summed in CSR order.  skip (lds; may be
 * NULL: root_weight=False) is S, typically p + 3 h; bias [h] may be NULL.  Nothing is saved for the backward. */
GCNX_API int gcnx_resgated_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* p, int64_t ldp,
                       int32_t n, int32_t h, const float* e, int64_t lde, int32_t edge_dim, const float* w_e,
                       const float* skip, int64_t lds, const float* bias, float* out, int64_t ldo);
/* gcn.py:71 -- *out = floats of caller scratch gcnx_resgated_bwd_targets needs (per-workgroup parts of dw_e; 0 with
 * edge_dim == 0).  Answers without a context; h <= 0, n < 0, edge_dim < 0 and out == NULL are GCNX_ERR_INVALID. */
GCNX_API int gcnx_resgated_bwd_scratch_floats(int64_t n, int32_t h, int32_t edge_dim, int64_t* out);
/* gcn.py:71 -- backward, the pass over the forward CSR.  d_out = dLoss/dout [n, h] (ldd).  Writes dk [n, h] (ldg) = dK; with ds
 * non-NULL copies d_out into ds [n, h] (ldgs) = dS, so that ONE gcnx_gemm_dw / gcnx_gemm_dx serves a dK | dQ | dV | dS array;
 * dw_e [edge_dim, 3 h] = dW_ke | dW_qe | dW_ve with its first two blocks equal.  The dw_e sums go through per-workgroup
 * parts in scratch (row-then-entry order inside a workgroup) and a second small launch inside this call (fixed order, no
 * atomics). */
GCNX_API int gcnx_resgated_bwd_targets(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* p, int64_t ldp,
                       int32_t n, int32_t h, const float* e, int64_t lde, int32_t edge_dim, const float* w_e,
                       const float* d_out, int64_t ldd, float* dk, int64_t ldg, float* ds, int64_t ldgs, float* dw_e,
                       float* scratch);
/* gcn.py:71 -- backward, the pass over the transposed pattern (rowptr_t, colidx_t, perm_t of gcnx_csr_transpose_perm:
 * perm_t[p] = the forward entry behind entry p; needed for a symmetric pattern too).  e is read in the forward entry order
 * through perm_t; for source j and each of its targets i the kernel gathers K[i] and d_out[i] (n * ldd * 4 < 2^32).  Writes
 * dqv [n, 2 h] (ldg) = dQ | dV, e.g. columns [h, 3 h) of dK | dQ | dV | dS.  dW, db and dx of the layer are gcnx_gemm_dw,
 * gcnx_act_bias_grad (over the 3 h biased columns) and gcnx_gemm_dx on that array. */
GCNX_API int gcnx_resgated_bwd_sources(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const int32_t* perm_t,
                       const float* p, int64_t ldp, int32_t n, int32_t h, const float* e, int64_t lde, int32_t edge_dim,
                       const float* w_e, const float* d_out, int64_t ldd, float* dqv, int64_t ldg);

/* ---- TransformerConv: scaled dot-product edge attention, small-feature regime (heads * c <= 128) ------------------------
 * PyG's TransformerConv(in, c, heads, concat=True, beta, dropout=0, edge_dim, bias, root_weight) (Shi et al., UniMP): the
 * dot-product way to use the dca / proximity features the reference computes and its model drops (gcn_utills.py:319-443;
 * gcn.py:71).  CSR row i is the target, its stored entries j the sources, values are ignored, no self-loops are added or
 * removed, the pattern and e are used as stored.  Head h owns columns [h c, h c + c) of every heads * c = HC wide block.
 * p = Q | K | V (| S) [n, >= 3 HC] (ldp) is ONE array from one gcnx_gemm with the stacked weight and bias
 * (x [W_q | W_k | W_v | W_s] + [b_q | b_k | b_v | b_s]: lin_query, lin_key, lin_value and lin_skip); e [nnz, edge_dim] (lde)
 * holds the entries' features in the CSR's entry order, w_e [edge_dim, HC] is lin_edge (no bias):
 *     T_ij = sum_d e_ij[d] W_e[d, :]        k_ij = K[j] + T_ij        v_ij = V[j] + T_ij     (T = 0 with edge_dim = 0)
 *     score_ij,h = <Q[i,h,:], k_ij[h,:]> * s          s = fp32(1 / sqrt(c))
 *     alpha = softmax over the stored entries of row i       O[i,h,:] = sum_j alpha_ij,h v_ij[h,:]   (no entries: O = 0)
 *     no root_weight:          out = O
 *     root_weight, beta=False: out = O + S
 *     root_weight, beta=True:  b_i = sigmoid(<w1, O_i> + <w2, S_i> + <w3, O_i - S_i>)    out_i = b_i S_i + (1 - b_i) O_i
 *                              (w_beta = lin_beta.weight = w1 | w2 | w3 [3 HC], no bias)
 * and with d_out = dLoss/dout:
 *     beta=False: dO = d_out,  dS = d_out
 *     beta=True:  g_i = <d_out_i, S_i - O_i> b_i (1 - b_i)
 *                 dO_i = (1 - b_i) d_out_i + g_i (w1 + w3)      dS_i = b_i d_out_i + g_i (w2 - w3)
 *                 dw1 = sum_i g_i O_i     dw2 = sum_i g_i S_i     dw3 = sum_i g_i (O_i - S_i)
 *     r[i,h] = <dO[i,h,:], O[i,h,:]>       dscore_ij,h = alpha_ij,h (<dO[i,h,:], v_ij[h,:]> - r[i,h])
 *     dQ[i] = s sum_j dscore_ij k_ij                                            (forward CSR)
 *     dK[j] = s sum_i dscore_ij Q[i]        dV[j] = sum_i alpha_ij dO[i]        (transposed pattern; needs no e and no W_e)
 *     dW_e[d,h,:] = sum_i ( s Q[i,h,:] A_i[d,h] + dO[i,h,:] B_i[d,h] )
 *                   A_i[d,h] = sum_j e_ij[d] dscore_ij,h     B_i[d,h] = sum_j e_ij[d] alpha_ij,h
 * d b_k is analytically zero: a common shift of all keys moves every score of a row by the same amount.  The row maximum
 * is subtracted before every exponential and the softmax denominator is >= 1: no overflow, no 0 / 0.  sigmoid(a) =
 * 1 / (1 + exp(-a)) with the overflow to inf resolving to 0: every finite a gives a finite b and a finite b (1 - b).
 * fp32, no float atomics, fixed summation order: the same bits on every call.  Nothing is allocated.
 * gcnx_transformer_conv_ok (gcn.py:71): 1 if the shapes are served: heads in {1, 2, 4, 8}, heads * c in {16, 32, 64, 128},
 * c >= 4, 0 <= edge_dim <= 8, ldp % 4 == 0, ldp >= 3 * heads * c, n * ldp * 4 < 2^32.  Every call below returns
 * GCNX_ERR_UNSUPPORTED otherwise, and for float4 operands (everything but e, alpha, dscore and the index arrays) off a
 * 16-byte boundary or leading dimensions that are not multiples of 4 floats >= their width, with nothing launched and
 * nothing written.  n == 0 succeeds and writes nothing; negative sizes and NULL mandatory pointers are GCNX_ERR_INVALID;
 * e, w_e (and dw_e) may be NULL only with edge_dim == 0. */
GCNX_API int gcnx_transformer_conv_ok(int64_t n, int32_t heads, int32_t c, int64_t ldp, int32_t edge_dim);
/* gcn.py:71 -- out [n, HC] (ldo) from ONE gather of the contiguous K[j] | V[j] per entry, with a running row maximum and a
 * rescaled accumulator, summed in CSR order.  skip (lds; may be NULL: root_weight=False) is S, typically p + 3 HC; w_beta
 * [3 HC] (may be NULL: beta=False) applies the gate in the epilogue, the row's dot a butterfly over the lane group; w_beta
 * without skip is GCNX_ERR_INVALID.  A row without entries: O = 0 exactly, and out = S bit for bit without beta.  alpha
 * [nnz, heads] and o_pre [n, HC] (ldpre) = O save what the backward needs; both may be NULL (inference). */
GCNX_API int gcnx_transformer_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* p,
                       int64_t ldp, int32_t n, int32_t heads, int32_t c, const float* e, int64_t lde, int32_t edge_dim,
                       const float* w_e, const float* skip, int64_t lds, const float* w_beta, float* out, int64_t ldo,
                       float* alpha, float* o_pre, int64_t ldpre);
/* gcn.py:71 -- *out = floats of caller scratch the backward needs: per-workgroup parts of dw_e (gcnx_transformer_bwd_targets)
 * and, with beta != 0, of dw_beta (gcnx_transformer_beta_bwd); the two calls run one after the other and may share it
 * (the larger of the two; 0 with edge_dim == 0 and beta == 0).  Answers without a context; heads <= 0, c <= 0, n < 0,
 * edge_dim < 0 and out == NULL are GCNX_ERR_INVALID. */
GCNX_API int gcnx_transformer_bwd_scratch_floats(int64_t n, int32_t heads, int32_t c, int32_t edge_dim, int32_t beta,
                       int64_t* out);
/* gcn.py:71 -- backward of the beta gate (called only with beta=True), row by row: b is recomputed from o = O (ldo) and skip =
 * S (lds).  d_out [n, hc] (ldd) -> d_o [n, hc] (ldgo) = dO, d_s [n, hc] (ldgs) = dS, dw_beta [3 hc] = dw1 | dw2 | dw3.
 * hc in {16, 32, 64, 128}.  dw_beta goes through per-workgroup parts in scratch and a second small launch inside this
 * call (fixed order, no atomics). */
GCNX_API int gcnx_transformer_beta_bwd(gcnx_ctx* ctx, const float* d_out, int64_t ldd, const float* o, int64_t ldo,
                       const float* skip, int64_t lds, const float* w_beta, int32_t n, int32_t hc, float* d_o, int64_t ldgo,
                       float* d_s, int64_t ldgs, float* dw_beta, float* scratch);
/* gcn.py:71 -- backward, the pass over the forward CSR.  d_o = dO [n, HC] (ldd), o = O (ldo), alpha from the forward.
 * Writes dscore [nnz, heads] in entry order, dq [n, HC] (ldg) = dQ and dw_e [edge_dim, HC]; with ds non-NULL copies d_o
 * into ds [n, HC] (ldgs) = dS, the beta=False root path, so that ONE gcnx_gemm_dw / gcnx_gemm_dx serves a dQ | dK | dV | dS
 * array.  The dw_e sums go through per-workgroup parts in scratch (2 edge_dim scalars per row and head, the outer products
 * formed once per row) and a second small launch inside this call (fixed order, no atomics). */
GCNX_API int gcnx_transformer_bwd_targets(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* p,
                       int64_t ldp, int32_t n, int32_t heads, int32_t c, const float* e, int64_t lde, int32_t edge_dim,
                       const float* w_e, const float* alpha, const float* d_o, int64_t ldd, const float* o, int64_t ldo,
                       float* dscore, float* dq, int64_t ldg, float* ds, int64_t ldgs, float* dw_e, float* scratch);
/* gcn.py:71 -- backward, the pass over the transposed pattern (rowptr_t, colidx_t, perm_t of gcnx_csr_transpose_perm:
 * perm_t[p] = the forward entry behind entry p; needed for a symmetric pattern too).  alpha and dscore are read in the
 * forward entry order through perm_t; for source j and each of its targets i the kernel gathers Q[i] and d_o[i]
 * (n * ldd * 4 < 2^32); it reads neither e nor w_e.  Writes dkv [n, 2 HC] (ldg) = dK | dV, e.g. columns [HC, 3 HC) of
 * dQ | dK | dV | dS.  dW, db and dx of the layer are gcnx_gemm_dw, gcnx_act_bias_grad (over the biased columns) and
 * gcnx_gemm_dx on that array. */
GCNX_API int gcnx_transformer_bwd_sources(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t,
                       const int32_t* perm_t, const float* p, int64_t ldp, int32_t n, int32_t heads, int32_t c,
                       const float* alpha, const float* dscore, const float* d_o, int64_t ldd, float* dkv, int64_t ldg);

/* ---- TopKPool: per-graph top-k selection, gated gather, induced sub-CSR ------------------------------------------
 * spektral.layers.pooling.TopKPool, the one layer the reference's training script imports (gcn.py:10) that had no kernels
 * here, in disjoint mode: y = X p / ||p||, the k_g rows of every graph with the largest y are kept, X' = (X * gate(y))[idx],
 * A' = A[idx][:, idx] with the values copied (not renormalised).  Kept rows stay in their original relative order (Spektral
 * orders them by score; every layer downstream is permutation-equivariant), so A' keeps sorted columns and its diagonal
 * blocks.  Scores compare as IEEE numbers (-0.0 == +0.0), among equal scores the lower row wins; with a NaN score the only
 * promise is k_g distinct rows of graph g.  fp32, no atomics: the same bits on every call.
 * gcnx_topk_select_ok (gcn.py:10): 1 if a batch whose largest graph has max_graph_rows rows and f features is served (one
 * workgroup ranks a graph's 8-byte keys in LDS: up to 16384 rows; f > 0); answers without a context. */
GCNX_API int gcnx_topk_select_ok(int64_t max_graph_rows, int32_t f);
/* gcn.py:10 -- scores and selection.  graph_ptr int32[b+1]; kept_ptr int32[b+1] = graph_ptr', the prefix sums of the k_g the
 * CALLER chose (0 <= k_g <= n_g; TopKPool: ceil(ratio n_g)), so that N' = kept_ptr[b] is known without a read-back;
 * max_graph_rows >= every n_g (sizes the LDS; a larger graph is left untouched).  x [N, f] (row stride ldx), p [f].
 * Writes y [N], idx [N'] (kept rows, global row numbers, ascending) and pos [N] (new row number, or -1).
 * GCNX_ERR_UNSUPPORTED, with nothing launched, where gcnx_topk_select_ok says 0. */
GCNX_API int gcnx_topk_select(gcnx_ctx* ctx, const int32_t* graph_ptr, const int32_t* kept_ptr, int32_t b,
                     int32_t max_graph_rows, const float* x, int64_t ldx, int32_t f, const float* p, float* y,
                     int32_t* idx, int32_t* pos);
/* gcn.py:10 -- out[r, :] = x[idx[r], :] * gate(y[idx[r]]), r < n_kept; gate = tanh, or the logistic function with
 * sigmoid_gating != 0.  out must not alias x. */
GCNX_API int gcnx_topk_gather(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* y, const int32_t* idx,
                     int32_t n_kept, int32_t f, int sigmoid_gating, float* out, int64_t ldo);
/* gcn.py:10 -- the adjoint of gcnx_topk_gather and of the score.  dxo [N', f] = dLoss/dX'.  For a kept row i (r = pos[i]):
 * dy_i = gate'(y_i) <dxo_r, x_i>, dx_i = gate(y_i) dxo_r + dy_i p / ||p||; a dropped row gets dx_i = 0 -- every row of
 * dx [n, f] is written.  dp [f] = (I - p^ p^T)(X^T dy) / ||p||, p^ = p / ||p||, summed in a fixed order (per-tile parts in
 * the ctx workspace, then one workgroup).  Nothing flows through the selection.  dx must not alias x or dxo. */
GCNX_API int gcnx_topk_bwd(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* y, const int32_t* pos, const float* p,
                  int32_t n, int32_t f, int sigmoid_gating, const float* dxo, int64_t lddxo, float* dx, int64_t lddx,
                  float* dp);
/* gcn.py:10 -- A' = A[idx][:, idx] for idx / pos as gcnx_topk_select writes them (any ascending idx with its inverse pos
 * does): rowptr_out int32[n_kept + 1], colidx_out = pos[col] of the surviving entries in their stored order (sorted rows stay
 * sorted), vals_out their values; vals == NULL <=> vals_out == NULL.  colidx_out / vals_out need room for the parent's nnz
 * at most; nnz' = rowptr_out[n_kept] is the caller's to read back.  Three launches, the block totals in the ctx workspace. */
GCNX_API int gcnx_csr_induce(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals,
                    const int32_t* idx, const int32_t* pos, int32_t n_kept, int32_t* rowptr_out, int32_t* colidx_out,
                    float* vals_out);

/* ---- GlobalAttnSumPool: the learned readout, a softmax over the rows of every graph ---------------------------------
 * spektral.layers.pooling.GlobalAttnSumPool, from the module the reference's training script imports (gcn.py:10); PyG's
 * AttentionalAggregation(gate_nn=Linear(f, 1, bias=False)) -- a bias would cancel in the softmax.  For every graph g of a
 * disjoint batch (graph_ptr int32[b+1], graph_ptr[0] = 0, graph_ptr[b] = n), x [n, f] (ldx), a [f]:
 *     s_i = <x_i, a>   alpha_i = exp(s_i - m_g) / l_g (m: the graph's largest score, l: its sum)   P[g] = sum_i alpha_i x_i
 * One pass over x with a running maximum and sum; the maximum is subtracted before any exponential: no score overflows.
 * fp32, no float atomics, fixed summation order: the same bits on every call, eager or replayed from a captured graph.
 * Nothing is allocated, nothing synchronises with the host.  1 <= f <= 256 (GCNX_ERR_INVALID above), any ld >= f: float4 lanes
 * when f and the leading dimensions are multiples of 4 and x, a, pooled (dpooled, dx) are 16-byte aligned, scalar lanes
 * otherwise.  An empty graph pools to a zero row (as gcnx_segment_pool); a one-row graph has alpha = 1 and P = its row.
 * n == 0 or b == 0 succeeds and writes nothing; negative sizes and NULL mandatory pointers are GCNX_ERR_INVALID.
 * gcnx_attn_pool_scratch_floats (gcn.py:10): floats of caller scratch (16-byte aligned) that serve gcnx_attn_pool with this
 * slice_rows AND gcnx_attn_pool_bwd; answers without a context. */
GCNX_API int64_t gcnx_attn_pool_scratch_floats(int64_t n, int32_t b, int32_t f, int32_t slice_rows);
/* gcn.py:10 -- pooled [b, f] (ldp) and alpha [n] (may be NULL: not stored).  Two routes.  whole: one workgroup per graph, its
 * waves each walk a share of the rows and combine their (m, l, acc[f]) through LDS.  sliced: graphs taller than slice_rows are
 * cut into row slices across workgroups, each slice writes (m, l, acc[f]) to scratch, and a second launch rescales and adds
 * the parts in slice order, writes pooled and turns the stored scores into alpha.  slice_rows == 0: the library chooses --
 * sliced (slices of at least 64 rows, about two per CU) when b < 2 CUs and the graphs average more than 384 rows, whole
 * otherwise and whenever scratch is NULL; slice_rows > 0 forces that slice height (any positive value; scratch required). */
GCNX_API int gcnx_attn_pool(gcnx_ctx* ctx, const int32_t* graph_ptr, const float* x, int64_t ldx, const float* a, int32_t n,
                   int32_t b, int32_t f, int32_t slice_rows, float* pooled, int64_t ldp, float* alpha, float* scratch);
/* gcn.py:10 -- backward from alpha and pooled as the forward wrote them and dpooled [b, f] (lddp).  With
 * t_i = <dP[g], x_i - P[g]>:
 *     dx_i = alpha_i dP[g] + (alpha_i t_i) a          da = sum_i (alpha_i t_i) x_i
 * dx [n, f] (lddx; may be NULL) is written, not accumulated, and must not alias x; da [f] (may be NULL; needs scratch) goes
 * through per-workgroup partial rows in scratch and a second small launch inside this call (fixed order, no atomics).  The
 * grid goes over row blocks regardless of graph boundaries. */
GCNX_API int gcnx_attn_pool_bwd(gcnx_ctx* ctx, const int32_t* graph_ptr, const float* x, int64_t ldx, const float* a,
                       const float* alpha, const float* pooled, int64_t ldp, const float* dpooled, int64_t lddp, int32_t n,
                       int32_t b, int32_t f, float* dx, int64_t lddx, float* da, float* scratch);

/* ---- GraphNorm: per-graph normalisation in the slot of the node-level BatchNorms (gcn_utills.py:816-826) ----
 * torch_geometric.nn.GraphNorm(f, eps) (Cai et al. 2021) in place of the reference's batch_norm_1 / batch_norm_2
 * (gcn_utills.py:816-817, applied at 832-838), fused with the PReLU behind them (gcn_utills.py:820-821).  For every graph g of a
 * disjoint batch (graph_ptr int32[b+1], graph_ptr[0] = 0, graph_ptr[b] = n) with m rows, per channel, with mean_scale a [f],
 * gamma [f], beta [f]:
 *     mu = mean_i z_i   o_i = z_i - a mu   v = mean_i o_i^2   r = 1 / sqrt(v + eps)   xh_i = o_i r   y_i = act(gamma xh_i + beta)
 * Training and evaluation are the same (no running statistics).  v is the mean of the centred squares, from a second walk
 * over the graph's rows; it is never formed as a difference of moments.  A one-row graph is legal (y = beta exactly at a = 1);
 * an empty graph has no rows, contributes nothing, and its mean / inv rows are written as zero.
 * fp32, no float atomics, fixed summation order: the same bits on every call.  Nothing synchronises with the host.
 * 1 <= f <= 256 (GCNX_ERR_INVALID above), any ld >= f: float4 lanes when f and the leading dimensions are multiples of 4 and
 * every operand is 16-byte aligned, scalar lanes otherwise.  act: GCNX_ACT_NONE, or GCNX_ACT_PRELU_SHARED with its slope
 * alpha[1]; any other act is GCNX_ERR_UNSUPPORTED with nothing launched.  n == 0, b == 0 or f == 0 succeeds and writes
 * nothing; negative sizes and NULL mandatory pointers are GCNX_ERR_INVALID.
 * Two routes per direction.  whole: one workgroup per graph walks its rows three times forward (sum, centred squares, y) and
 * twice backward (sums, dz); no scratch.  sliced: slices of slice_rows rows are spread across workgroups, per-slice partial
 * rows go to scratch and every workgroup of a graph adds them in slice order; three launches forward, two backward.
 * slice_rows == 0: the library chooses by gcnx_attn_pool's rule -- sliced (slices of at least 64 rows, about two per CU) when
 * b < 2 CUs and the graphs average more than 384 rows, whole otherwise and whenever scratch is NULL; slice_rows > 0 forces that
 * slice height (any positive value; scratch required).
 * gcnx_graph_norm_scratch_floats (gcn_utills.py:816-826): floats of caller scratch (16-byte aligned) that serve both launches
 * below with this slice_rows; answers without a context. */
GCNX_API int64_t gcnx_graph_norm_scratch_floats(int64_t n, int32_t b, int32_t f, int32_t slice_rows);
/* gcn_utills.py:816-826 -- z [n, f] (ldz) -> y [n, f] (ldy; may alias z exactly) and the per-graph mean [b, f], inv [b, f]
 * (contiguous rows) that the backward reads. */
GCNX_API int gcnx_graph_norm_act(gcnx_ctx* ctx, const int32_t* graph_ptr, const float* z, int64_t ldz, const float* mean_scale,
                        const float* gamma, const float* beta, float eps, int act, const float* alpha, int32_t n, int32_t b,
                        int32_t f, int32_t slice_rows, float* y, int64_t ldy, float* mean, float* inv, float* scratch);
/* gcn_utills.py:816-826 -- backward from dy [n, f] (lddy) and the saved z, mean, inv; t is recomputed from them as
 * gcnx_bn_act_bwd does.  With dt_i = dy_i act'(t_i), S1 = sum_i dt_i, S2 = sum_i dt_i xh_i over the graph's m rows:
 *     D = r gamma (S1 - S2 r mu (1 - a))        dz_i = r gamma (dt_i - xh_i S2 / m) - a D / m
 *     dgamma = sum_g S2   dbeta = sum_g S1   dmean_scale = - sum_g mu D   dalpha[0] = sum_i dy_i min(t_i, 0)
 * dz [n, f] (lddz) is written, not accumulated, and may alias dy exactly.  dgamma, dbeta, dmean_scale [f] and dalpha [1] may
 * each be NULL; they are summed over the graphs from per-graph rows in the ctx workspace by one small launch inside this call
 * (fixed order, no atomics; dalpha is written as zero for GCNX_ACT_NONE). */
GCNX_API int gcnx_graph_norm_act_bwd(gcnx_ctx* ctx, const int32_t* graph_ptr, const float* dy, int64_t lddy, const float* z,
                            int64_t ldz, const float* mean, const float* inv, const float* mean_scale, const float* gamma,
                            const float* beta, int act, const float* alpha, int32_t n, int32_t b, int32_t f, int32_t slice_rows,
                            float* dz, int64_t lddz, float* dgamma, float* dbeta, float* dmean_scale, float* dalpha,
                            float* scratch);

/* ---- explaining a frozen model: gradients with respect to the operator's values, soft masks (csrc/explain.hip) ----
 * Sampled dense-dense product on the CSR pattern: out[e] (+)= scale[e] * <L[row(e), :f], R[colidx[e], :f]> for every stored entry
 * e (row(e): the row whose range of rowptr holds e).  L, R [n, f] with leading dimensions ldl, ldr >= f; scale [nnz] or NULL
 * (ones); out [nnz], written (accumulate = 0) or added to (1).  With Z = A H this is dLoss/d(value of e) for L = dZ, R = H: the
 * gradient of learnable edge weights.  f = 16, 32, 64, 128 with 16-byte aligned L and R and leading dimensions in multiples of 4
 * floats run on the tile kernel; every other width (0 included), alignment and leading dimension on the any-width kernel: no
 * shape is refused.  Every out[e] has one writer and one order of summation (no atomics): two calls leave the same bits.
 * n == 0 or nnz == 0: GCNX_OK, nothing launched, nothing read.  GCNX_ERR_INVALID: NULL rowptr / colidx / out, NULL L or R with
 * f > 0, ldl or ldr < f, out aliasing an operand. */
GCNX_API int gcnx_sddmm_csr(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, int32_t n, int32_t nnz, const float* l,
                            int64_t ldl, const float* r, int64_t ldr, int32_t f, const float* scale, float* out, int accumulate);
/* The masked operator of GNNExplainer: vals_out[e] = a_vals[e] * sigmoid(logits[e]) for an off-diagonal entry, a_vals[e] (bit for
 * bit; its logit is not read) for a diagonal one, and vals_t_out[p] = vals_out[perm_t[p]] (the values of the transposed pattern,
 * perm_t from gcnx_csr_transpose_perm; both NULL: not written), in one launch.  sigmoid(a) = 1 / (1 + exp(-a)) for every finite a
 * (exactly 1 from a = 17 on).  All arrays [nnz]. */
GCNX_API int gcnx_edge_mask_fwd(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, int32_t n, int32_t nnz, const float* a_vals,
                                const float* logits, const int32_t* perm_t, float* vals_out, float* vals_t_out);
/* Floats of `scratch` for gcnx_edge_mask_bwd (f = 0) and gcnx_feat_mask_bwd (n rows of f features, per_row as there). */
GCNX_API int64_t gcnx_mask_scratch_floats(int64_t n, int32_t f, int per_row);
/* Its backward with the mask regularisers: with s = sigmoid(logits[e]), ent(p) = -p log(p + 1e-15) - (1 - p) log(1 - p + 1e-15),
 *     dlogits[e] = (dv[e] a_vals[e] + c_size + c_ent ent'(s)) s (1 - s)    off the diagonal;  0 on it
 *     terms[0] = sum s, terms[1] = sum ent(s)                              over the off-diagonal entries
 * dv [nnz]: dLoss/d(vals_out) (two gcnx_sddmm_csr).  c_size, c_ent: the coefficients as they multiply the two sums in the
 * objective (a mean's 1 / count included).  The sums are folded in a fixed order -- per-workgroup partials in scratch, then one
 * workgroup -- without atomics.  n == 0 or nnz == 0: terms = 0, 0. */
GCNX_API int gcnx_edge_mask_bwd(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, int32_t n, int32_t nnz, const float* a_vals,
                                const float* logits, const float* dv, float c_size, float c_ent, float* dlogits, float* terms,
                                float* scratch);
/* The feature mask: out[i, k] = x[i, k] * sigmoid(logits[k]) (per_row = 0: one logit per feature, [f]) or
 * x[i, k] * sigmoid(logits[i f + k]) (per_row = 1: [n, f] contiguous).  x, out [n, f] with ldx, ldo >= f, any alignment. */
GCNX_API int gcnx_feat_mask_fwd(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* logits, int per_row, int64_t n, int32_t f,
                                float* out, int64_t ldo);
/* Its backward from dxm = dLoss/d(out) [n, f] (ldd): dlogits = (dxm x (per_row = 0: summed over the rows in a fixed order -- parts
 * of 64 or more rows, each dealt to the row lanes of its column, then over the parts -- in fp64 accumulators with one fp32
 * rounding per part) + c_size + c_ent ent'(s))
 * s (1 - s), terms[0 .. 1] = sum s, sum ent(s) over the logits, as gcnx_edge_mask_bwd.  scratch:
 * gcnx_mask_scratch_floats(n, f, per_row) floats. */
GCNX_API int gcnx_feat_mask_bwd(gcnx_ctx* ctx, const float* dxm, int64_t ldd, const float* x, int64_t ldx, const float* logits,
                                int per_row, int64_t n, int32_t f, float c_size, float c_ent, float* dlogits, float* terms,
                                float* scratch);

/* ---- GCNConv on edge weights learned from the edge features: PyG's PDNConv (csrc/pdn.hip) ----
 * The reference computes dca / proximity values on every contact and bridge and its model drops them (gcn.py:71); here a
 * two-layer MLP with a sigmoid turns them into the edge weights of GCNConv's operator.  CSR rows are targets; entry e = (i <- j)
 * has the features x_e = e[e * lde .. + d).  With W1 [d, he] (row-major), b1 [he], w2 [he], b2 [1], all DEVICE pointers:
 *     z_e = x_e W1 + b1     h_e = relu(z_e)     s_e = <w2, h_e> + b2
 *     w_e = 1 (exactly; x_e is not read) where unit[e] != 0, else sigmoid(s_e)   (gcnx_edge_mask_fwd's sigmoid: 1 from s = 17 on)
 *     deg_i = sum of w_e over row i     r_i = deg_i^-1/2, 0 for a row without entries     v_e = r_i w_e r_j
 * gcn.py:71 -- 1 if d in 1 .. 8 and he in 1 .. 64 (what the two entry points below serve), else 0. */
GCNX_API int gcnx_pdn_ok(int32_t d, int32_t he);
/* gcn.py:71 -- writes w_out [nnz], r_out [n], vals_out [nnz] = v and vals_t_out[p] = v[perm_t[p]] (the values on the transposed
 * pattern, perm_t from gcnx_csr_transpose_perm; evaluated from the same expression: the same bits; both NULL or both given).
 * unit [nnz] bytes or NULL (no unit entries).  e may have any leading dimension lde >= d and any alignment.  Two launches (a group
 * of 16 lanes per row: gates and degree; a thread per entry: values), no synchronisation, no atomics: a row's degree is added in one fixed
 * order (fp64 lane sums, then the lanes), two calls leave the same bits.  Finite inputs give finite outputs (logits of +-40
 * included).  n == 0 or nnz == 0: GCNX_OK, nothing launched.  GCNX_ERR_INVALID: gcnx_pdn_ok fails, a NULL operand, lde < d. */
GCNX_API int gcnx_pdn_operator(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, int32_t n, int32_t nnz, const float* e,
                               int64_t lde, int32_t d, const float* w1, const float* b1, const float* w2, const float* b2, int32_t he,
                               const uint8_t* unit, const int32_t* perm_t, float* w_out, float* r_out, float* vals_out,
                               float* vals_t_out);
/* gcn.py:71 -- floats of `scratch` for gcnx_pdn_operator_bwd: one per entry (rounded up to 4) and at most 256 parts of
 * d he + 2 he + 1 floats (one part per 64 entries below that).  0 where gcnx_pdn_ok fails.  Answers without a context. */
GCNX_API int64_t gcnx_pdn_bwd_scratch_floats(int64_t n, int64_t nnz, int32_t d, int32_t he);
/* gcn.py:71 -- the gradient of the four MLP tensors from g[e] = dLoss/dv_e in forward entry order (gcnx_sddmm_csr), w and r as
 * gcnx_pdn_operator left them, (rowptr_t, colidx_t, perm_t) the transposed pattern of gcnx_csr_transpose_perm:
 *     c_e = g_e w_e     q_i = sum_{e in row i} c_e r_col(e) + sum_{p in row i of the transposed pattern} c_{perm_t[p]} r_{colidx_t[p]}
 *     dw_e = g_e r_i r_j - 1/2 r_i^3 q_i     ds_e = dw_e w_e (1 - w_e), 0 where unit[e]   (1 - w as exp(-s) w for s >= 0)
 *     dw2 = sum ds_e h_e    db2 = sum ds_e    dz_e = ds_e w2 * [z_e > 0]    dW1 = sum x_e (x) dz_e    db1 = sum dz_e
 * z_e, h_e and s_e are recomputed from e by the forward's own expression (the same bits: the same side of every ReLU).  dw1
 * [d, he], db1 [he], dw2 [he], db2 [1] are written, not accumulated.  Three launches: a group of 16 lanes per row (q_i, ds into scratch), at
 * most 256 workgroups of per-workgroup parts, one workgroup that folds them; fp64 accumulators, a fixed order, no atomics: two
 * calls leave the same bits.  No gradient flows to e.  n == 0 or nnz == 0: the four gradients are zeroed. */
GCNX_API int gcnx_pdn_operator_bwd(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const int32_t* rowptr_t,
                                   const int32_t* colidx_t, const int32_t* perm_t, int32_t n, int32_t nnz, const float* e, int64_t lde,
                                   int32_t d, const float* w1, const float* b1, const float* w2, const float* b2, int32_t he,
                                   const uint8_t* unit, const float* w, const float* r, const float* g, float* dw1, float* db1,
                                   float* dw2, float* db2, float* scratch);

/* ---- APPNP: K hops of personalised-PageRank propagation (csrc/appnp.hip) ----
 * Spektral's APPNPConv and PyG's APPNP(K, alpha), the long-range layer for the slot the reference's author left open
 * (gcn_utills.py:804-806): a Linear (gcnx_gemm) followed by k parameter-free hops on the GCN operator (gcn.py:8's gcn_filter),
 *     z^0 = x      z^{j+1}[i, :] = (1 - alpha) * sum_{e in row i, CSR order} vals[e] * z^j[colidx[e], :] + alpha * x[i, :]      out = z^k
 * Per element: one fmaf chain over the row's entries in CSR order from +0, then fmaf(alpha, x, (1 - alpha) * acc) with
 * 1 - alpha rounded once.  Both routes below and every column block evaluate exactly that, so they leave the same bits.
 * The backward is the same call: P = M^k + alpha sum_{j<k} M^j with M = (1 - alpha) A, so P^T is the same recursion on A^T:
 * pass the transposed operator and x = dz, and out receives dLoss/dx.  Nothing is kept for it.
 *
 * gcn_utills.py:804-806 -- 1 if the one-launch (resident) route serves a batch whose tallest graph has max_graph_rows rows:
 * max_graph_rows > 0, f and ldx multiples of 4 with ldx >= f, and two buffers of max_graph_rows x 4 floats plus the graph's
 * row pointers within 128 KiB of LDS (graphs of up to 3640 rows).  Operands off a 16-byte boundary take the streamed route. */
GCNX_API int gcnx_appnp_resident_ok(int64_t max_graph_rows, int32_t f, int64_t ldx);
/* gcn_utills.py:804-806 -- floats of `scratch` for the streamed route with k >= 2: n * f.  Answers without a context. */
GCNX_API int64_t gcnx_appnp_scratch_floats(int64_t n, int32_t f);
/* gcn.py:8 -- out [n, f] (ldo) = z^k from x [n, f] (ldx); vals NULL: ones.  graph_ptr [b + 1] (may be NULL) marks the diagonal
 * blocks of a block-diagonal operator (a disjoint batch), max_graph_rows the rows of its tallest graph (0: unknown).
 * Resident route (one launch): a workgroup per (graph, block of col_block columns) keeps the graph's slice in LDS across all k
 * hops, one workgroup barrier per hop; an entry whose column lies outside its graph's rows contributes nothing (no access is
 * out of range; the result for such input is unspecified); a graph with more than max_graph_rows rows is left untouched
 * (the rule of gcnx_topk_select).  Streamed route (k launches of a one-hop gather): any n, f, leading dimension and
 * alignment; it alternates between out and scratch (gcnx_appnp_scratch_floats; may be NULL for k <= 1) so that hop k lands in
 * out.  col_block 0: the library's choice -- resident where graph_ptr is given, gcnx_appnp_resident_ok holds, x and out are
 * 16-byte aligned with ldo % 4 == 0 and k >= 3 (k >= 2 where max_graph_rows <= 256: fewer hops do not earn the prologue back),
 * in the widest block of {f, 64, 32, 16, 8, 4} columns that fits, narrowed while the narrower block's workgroups still fit one
 * round of the CUs and then while fewer than 16 CSR entries per row can be staged in LDS; otherwise streamed.  col_block > 0: the resident route with that block, GCNX_ERR_UNSUPPORTED with
 * nothing launched where it is not served (not a multiple of 4, wider than f or 256, too tall for LDS, or any condition above).
 * col_block -1: streamed.  k == 0 copies x.  n == 0, f == 0 or b == 0 (with graph_ptr): GCNX_OK, nothing launched.
 * GCNX_ERR_INVALID: k outside 0 .. 64, alpha outside [0, 1], ldx or ldo < f, out overlapping x or scratch (or scratch
 * overlapping x), the streamed route with k >= 2 and scratch NULL.  No atomics, no read-back: capture-safe, and two calls
 * leave the same bits. */
GCNX_API int gcnx_appnp_propagate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals,
                                  const int32_t* graph_ptr, int32_t b, int32_t max_graph_rows, const float* x, int64_t ldx, int32_t n,
                                  int32_t f, int32_t k, float alpha, int32_t col_block, float* out, int64_t ldo, float* scratch);

/* ---- ChebConv: k Chebyshev filter terms of the scaled Laplacian (csrc/cheb.hip) ----
 * PyG's ChebConv(in, out, K, normalization="sym", lambda_max) -- Spektral's ChebConv(channels, K) with K one less --, the K-hop
 * layer with one weight matrix per hop distance for the slot the reference's author left open (gcn_utills.py:804-806).  On the
 * operator S of gcnx_cheb_norm, with c_s = -2 / lambda_max and c_d = 2 / lambda_max - 1, each rounded once to fp32 on the host:
 *     L^ z = c_s (S z) + c_d z        T_0 z = z      T_1 z = L^ z      T_j z = 2 L^ T_{j-1} z - T_{j-2} z
 * Per element and step: acc = +0, acc = fmaf(vals[e], cur[colidx[e]], acc) over the row's entries in CSR order, then
 * fmaf(a, acc, fmaf(b, cur[i], d)) with
 *     basis step j = 1 .. k-1:  (a, b) = (c_s, c_d) at j = 1, else (2 c_s, 2 c_d);  cur = T_{j-1} x,  d = -T_{j-2} x [i]  (-0 at j = 1)
 *     sum step j = k-2 .. 0:    (a, b) = (c_s, c_d) at j = 0, else (2 c_s, 2 c_d);  cur = b_{j+1},  d = H_j[i] - b_{j+2}[i]
 *                               (b_{k-1} = H_{k-1}, b_k = +0);  step 0 then adds bias[column] (bias NULL: nothing is added)
 * Both routes below and every column block evaluate exactly that, so they leave the same bits.  The layer is H = x W (one
 * gcnx_gemm, W = [lins.0.weight^T | .. | lins.{k-1}.weight^T]) and gcnx_cheb_sum; its backward gcnx_cheb_basis on the
 * transposed operator applied to dZ (G_j = T_j(L^^T) dZ, one panel [n, k f]), then dW = x^T G and dx = G W^T.  Nothing is kept
 * for it.  A lambda_max below the operator's largest eigenvalue makes the terms grow with j.
 *
 * gcn_utills.py:804-806 -- vals_out [nnz] = the values of S on the stored pattern (row = target, column = source; vals NULL: ones):
 *     S[i, j] = r_i w_ij r_j  for a stored i != j,  exactly +0 for a stored diagonal entry;   r_j = deg_j^-1/2,
 *     deg_j = sum_{i != j} w_ij over column j,  r_j = 0 where deg_j <= 0        (PyG's get_laplacian: loops removed, the degree
 * scattered on the source index).  rowptr_t / colidx_t / vals_t: the transposed CSR, which gives the column sums without atomics
 * (the same three pointers for a symmetric operator; vals_t NULL exactly when vals is).  Degrees are summed in fp64 in CSR
 * order: two calls leave the same bits.  vals_out may be vals.  Uses the context's workspace (n floats): not capturable.
 * S^T is the transpose of S's values (gcnx_csr_transpose), not this call on the transposed pattern. */
GCNX_API int gcnx_cheb_norm(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals, const int32_t* rowptr_t,
                            const int32_t* colidx_t, const float* vals_t, int32_t n, float* vals_out);
/* gcn_utills.py:804-806 -- 1 if the one-launch (resident) route serves a batch whose tallest graph has max_graph_rows rows:
 * max_graph_rows > 0, f and ld (the leading dimension of the call's input: x or h) multiples of 4 with ld >= f, and two buffers
 * of max_graph_rows x 4 floats plus the graph's row pointers within 128 KiB of LDS (graphs of up to 3640 rows).  Operands off a
 * 16-byte boundary take the streamed route. */
GCNX_API int gcnx_cheb_resident_ok(int64_t max_graph_rows, int32_t f, int64_t ld);
/* gcn_utills.py:804-806 -- floats of `scratch` for the streamed route of gcnx_cheb_sum with k >= 3: n * f.  Answers without a
 * context. */
GCNX_API int64_t gcnx_cheb_scratch_floats(int64_t n, int32_t f);
/* gcn_utills.py:804-806 -- gcnx_cheb_basis: block j (columns j f .. (j + 1) f) of out [n, k f] (ldo) = T_j(L^) x for j = 0 .. k-1,
 * from x [n, f] (ldx).  gcnx_cheb_sum: out [n, f] (ldo) = sum_j T_j(L^) H_j + bias from h [n, k f] (ldh; H_j its block j) by the
 * Clenshaw steps above; bias [f] may be NULL.  Both run k - 1 gathers; k == 1 runs none (out = x; out = h + bias).
 * rowptr / colidx / vals (NULL: ones), graph_ptr [b + 1] (may be NULL), b and max_graph_rows (0: unknown) as in
 * gcnx_appnp_propagate.  Resident route (one launch): a workgroup per (graph, block of col_block columns) keeps two terms of the
 * graph's slice in LDS across all steps -- the new term overwrites the term two steps back --, one workgroup barrier per step;
 * an entry whose column lies outside its graph's rows contributes nothing (no access is out of range; the result for such
 * input is unspecified); a graph with more than max_graph_rows rows is left untouched.  Streamed route (k - 1 launches of a
 * one-hop gather): any n, f, leading dimension and alignment; gcnx_cheb_basis keeps its terms in the blocks of out and does not
 * read scratch (may be NULL); gcnx_cheb_sum alternates between out and scratch (gcnx_cheb_scratch_floats; may be NULL for
 * k <= 2) so that step 0 lands in out.  col_block 0: the library's choice -- resident where graph_ptr is given,
 * gcnx_cheb_resident_ok holds, input and out are 16-byte aligned with ldo % 4 == 0 and k - 1 >= 3 (k - 1 >= 2 where
 * max_graph_rows <= 256), in the column block gcnx_appnp_propagate would choose; otherwise streamed.  col_block > 0: the
 * resident route with that block, GCNX_ERR_UNSUPPORTED with nothing launched where it is not served (not a multiple of 4, wider
 * than f or 256, too tall for LDS, or any condition above; k == 1 gathers nothing on any route).  col_block -1: streamed.
 * n == 0, f == 0 or b == 0 (with graph_ptr): GCNX_OK, nothing launched.  GCNX_ERR_INVALID: k outside 1 .. 16, lambda_max not a
 * finite number > 0, col_block < -1, a leading dimension below its operand's width, out overlapping the input, bias or scratch
 * (or scratch overlapping the input), the streamed route of gcnx_cheb_sum with k >= 3 and scratch NULL.  No atomics, no
 * read-back, nothing allocated: capture-safe, and two calls leave the same bits. */
GCNX_API int gcnx_cheb_basis(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals, const int32_t* graph_ptr,
                             int32_t b, int32_t max_graph_rows, const float* x, int64_t ldx, int32_t n, int32_t f, int32_t k,
                             float lambda_max, int32_t col_block, float* out, int64_t ldo, float* scratch);
GCNX_API int gcnx_cheb_sum(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals, const int32_t* graph_ptr,
                           int32_t b, int32_t max_graph_rows, const float* h, int64_t ldh, const float* bias, int32_t n, int32_t f,
                           int32_t k, float lambda_max, int32_t col_block, float* out, int64_t ldo, float* scratch);

/* ---- RGCNConv: typed edges, every relation from one gather (csrc/rgcn.hip) -------------------------------------------------
 * PyG's RGCNConv(in, out, num_relations, aggr = "mean", root_weight, bias) without a decomposition (Schlichtkrull et al. 2018):
 *     out_i = x_i W_root + b + sum_{r < R} mean_{k in N_r(i)} x_col(k) W_r      N_r(i): the stored entries of row i of relation r
 * on the pattern as stored (row = target, column = source): no loop is added or removed, the mean over no entry is 0.  R =
 * num_relations is 1 .. 4.  In the reference's graphs the relation is in the edge features: gcn_utills.py:379-443 sets dca on the
 * inter-chain bridges only and proximity on the intra-chain contacts only.
 *
 * gcnx_rgcn_operator: rel [nnz] (one byte per stored entry, 0 .. R-1) and val [nnz] = 1 / (entries of the entry's row with the
 * entry's relation) from the edge features e [nnz, edge_dim] (lde).  rule GCNX_RGCN_NONZERO: the relation is the first column d
 * with e[k, d] != 0, edge_dim where there is none; num_relations must be edge_dim + 1.  rule GCNX_RGCN_INDEX: column 0 holds the
 * relation as an integer-valued float; a value outside 0 .. R-1 is clamped into it (a NaN reads 0).  One thread walks a row:
 * no atomics.  perm_t (gcnx_csr_transpose_perm; may be NULL together with rel_t and val_t): rel_t[p] = rel[perm_t[p]] and
 * val_t[p] = val[perm_t[p]], the operands of the backward on the transposed pattern (a second launch).  Capture-safe.
 * GCNX_ERR_INVALID: a rule or num_relations outside its range, edge_dim < 1, lde < edge_dim, the rule NONZERO with
 * num_relations != edge_dim + 1, perm_t / rel_t / val_t not all given or all NULL. */
typedef enum { GCNX_RGCN_NONZERO = 0, GCNX_RGCN_INDEX = 1 } gcnx_rgcn_rule;
GCNX_API int gcnx_rgcn_operator(gcnx_ctx* ctx, const int32_t* rowptr, const float* e, int64_t lde, int32_t edge_dim, int32_t rule,
                                int32_t num_relations, const int32_t* perm_t, int32_t n, int64_t nnz, uint8_t* rel, float* val,
                                uint8_t* rel_t, float* val_t);
/* gcnx_rgcn_conv_ok: 1 if the one launch serves the shapes (fi and fo in {16, 32, 64, 128}, num_relations in 1 .. 4, ldx >= fi,
 * ldx % 4 == 0, n * ldx * 4 < 2^32); gcnx_rgcn_conv returns GCNX_ERR_UNSUPPORTED otherwise, and for x, w, m or out off a 16-byte
 * boundary, ldm < num_relations * fi, ldo < fo or either not a multiple of 4.
 * gcnx_rgcn_conv: out [n, fo] (ldo) = [A_0 x | .. | A_{R-1} x | x] w + bias in one launch; A_r = the entries of relation r with
 * their val.  w: the row-stacked blocks W_0 .. W_{R-1} and, with root_weight != 0, W_root behind them -- [(R + 1) fi, fo]
 * contiguous; bias [fo] may be NULL.  m (may be NULL): receives the panel M = [A_0 x | .. | A_{R-1} x], [n, R fi] (ldm), the
 * operand of the weight gradient dW = M^T dZ.  w_transposed != 0: every block is [fo, fi] -- the backward with respect to x,
 * dX = dZ W_root^T + sum_r A_r^T (dZ W_r^T), as this call on (rowptr_t, colidx_t, rel_t, val_t) with x = dZ and the layer's
 * weights as stored.  Every element of M is the chain acc = fma(val_k, x[col(k)], acc) over the row's entries of its relation in
 * CSR order from +0 (no atomics: the same bits on every call, and the bits of gcnx_rgcn_aggregate); an entry whose column lies
 * outside [0, n) adds nothing.  The outputs must not alias x or each other (GCNX_ERR_INVALID). */
GCNX_API int gcnx_rgcn_conv_ok(int64_t n, int32_t fi, int32_t fo, int32_t num_relations, int64_t ldx);
GCNX_API int gcnx_rgcn_conv(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const uint8_t* rel, const float* val,
                            const float* x, int64_t ldx, int32_t n, int32_t fi, const float* w, int root_weight, int32_t fo,
                            int32_t num_relations, int w_transposed, const float* bias, float* m, int64_t ldm, float* out, int64_t ldo);
/* The panel alone: m [n, R f] (ldm) = [A_0 x | .. | A_{R-1} x] for any f >= 1, stride and alignment (16-byte loads where f, ldx,
 * ldm and the pointers allow them), with the chain of gcnx_rgcn_conv.  The composed route of the layer is this, then gcnx_gemm
 * over M and over x.  GCNX_ERR_INVALID: num_relations outside 1 .. 4, f < 1, ldx < f, ldm < R f, m aliasing x. */
GCNX_API int gcnx_rgcn_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const uint8_t* rel, const float* val,
                                 const float* x, int64_t ldx, int32_t n, int32_t f, int32_t num_relations, float* m, int64_t ldm);

/* ---- aggregation with bf16 features ("fp32 and bf16 both reported") ----
 * out[t, :] = bf16(act(sum_e vals[e] * h[colidx[e], :] + bias)): GCNConv.call's / GeneralConv's aggregation (gcn.py:334) on
 * activations stored as bf16 (uint16_t bit patterns), fp32 accumulation, round-to-nearest-even on the way out; bias fp32
 * (may be NULL), vals may be NULL (ones).  f in {64, 128, 256}, n * ldh * 2 < 2^32 (GCNX_ERR_UNSUPPORTED otherwise);
 * act: GCNX_ACT_NONE / GCNX_ACT_RELU.  A measured variant: the models keep fp32 activations.
 * gcnx_f32_to_bf16 (round to nearest even) / gcnx_bf16_to_f32: contiguous arrays of `count` elements. */
GCNX_API int gcnx_spmm_csr_bf16(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals,
                      const uint16_t* h, int64_t ldh, const float* bias, uint16_t* out, int64_t ldo, int32_t n, int32_t f,
                      int act);
GCNX_API int gcnx_f32_to_bf16(gcnx_ctx* ctx, const float* x, uint16_t* y, int64_t count);
GCNX_API int gcnx_bf16_to_f32(gcnx_ctx* ctx, const uint16_t* x, float* y, int64_t count);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI (new capability) ---- */
GCNX_API int gcnx_comm_unique_id(char id[GCNX_UNIQUE_ID_BYTES]);
GCNX_API int gcnx_comm_init_rank(gcnx_ctx* ctx, const char id[GCNX_UNIQUE_ID_BYTES], int nranks,
                        int rank, gcnx_comm** out);
GCNX_API int gcnx_comm_destroy(gcnx_comm* comm);
/* In-place all-reduce of a device fp32 buffer on the ctx stream. */
GCNX_API int gcnx_allreduce_f32(gcnx_ctx* ctx, gcnx_comm* comm, float* buf, int64_t n, int op);

#ifdef __cplusplus
}
#endif
#endif /* GCNX_H */
