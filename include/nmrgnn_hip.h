/* nmrgnn_hip.h — C ABI of libnmrgnn_hip.so: the MI355X (gfx950) engine for nmrgnn's
 * message-passing hot path.
 *
 * The reference (ur-whitelab/nmrgnn v0.7) is pure Python/TensorFlow and has NO plugin /
 * FFI / custom-op interface; this ABI is therefore defined here, one entry point per stage
 * of GNNModel.call (nmrgnn/model.py:245-274), and each declaration cites the reference
 * lines it replaces.  INTEGRATION.md shows the reference-side (ctypes) binding.
 *
 * Conventions
 *   - every pointer named *_dev (and every float* / int32_t* tensor argument) is a DEVICE pointer owned
 *     by the caller (torch allocations in the Python host); the library allocates only the
 *     opaque ng_ctx (scratch workspace, profiling events).
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on that stream
 *     and never synchronises the device.
 *   - return 0 = NG_OK, negative = error; message via ng_last_error(ctx).  Nothing throws.
 *   - all tensors are fp32 row-major; index tensors are int32.
 *   - a ctx is not thread-safe: one per host thread / GPU.
 */
#ifndef NMRGNN_HIP_H
#define NMRGNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NG_ABI_VERSION 9

enum {
  NG_OK = 0,
  NG_ERR_INVALID = -1, /* bad shape / argument */
  NG_ERR_HIP = -2,     /* HIP runtime error */
  NG_ERR_NOMEM = -3,
  NG_ERR_UNSUPPORTED = -4
};

/* keras activation names of hypers mp_activation / fc_activation (nmrgnn/model.py:33-36) */
enum { NG_ACT_NONE = 0, NG_ACT_SOFTPLUS = 1, NG_ACT_RELU = 2, NG_ACT_TANH = 3 };

typedef struct ng_ctx ng_ctx;

int ng_abi_version(void);
int ng_ctx_create(int device, ng_ctx** out);
void ng_ctx_destroy(ng_ctx* ctx);
const char* ng_last_error(ng_ctx* ctx);
/* The NG_* path switches (NG_EDGE_MATH, NG_GEMM_MATH, NG_MP_PATH, ... — listed in csrc/ng_common.h) are parsed from
 * the environment once per process; ng_reload_env() parses them again (tests / A-B tools that flip one in-process). */
int ng_reload_env(void);
/* Inference with constant weights: between ng_weights_frozen(ctx, owner != 0) and ng_weights_frozen(ctx, 0) the library
 * keeps its packed weight images (MFMA fragment orders, fp16-piece images) across calls instead of re-packing them on
 * every call.  The images are keyed by the weight tensors' addresses, so `owner` names the model they belong to: a
 * call with a different non-zero owner discards what the cache holds (another model's freed weights may have had the
 * same addresses).  A change of a weight tensor of the current owner must be announced with ng_weights_changed(ctx)
 * (ng_adam_step does so itself).  Off (owner 0) is the default; calls made while it is off never touch the cache.
 * Contract while frozen: every weight pointer handed to an entry point keeps its contents until ng_weights_changed /
 * the end of the window (a temporary tensor whose address is later reused for other weights must be announced the
 * same way).  Weights the library repacks into its own scratch inside a call (the MPLayer backward's Wp) are never
 * cached, so backward entry points may run inside a frozen window. */
int ng_weights_frozen(ng_ctx* ctx, int owner);
int ng_weights_changed(ng_ctx* ctx);
/* Deferred weight-gradient sums (ABI 5).  The backward entry points end in a second-stage reduction of per-workgroup
 * partials into the gradient tensor (deterministic, fixed order): seven launches of 5-12 us in a training step's
 * backward (head, FC block, four MPLayers, embedding; nmrgnn/model.py:262-273 differentiated).  Between
 * ng_defer_reductions(ctx, stream, 1) and the matching ng_defer_reductions(ctx, stream, 0) the entry points keep their
 * partials in a context-owned arena and only QUEUE the reduction; ng_flush_reductions(ctx, stream) runs everything
 * queued so far in one launch on `stream` (switching deferral off flushes too).  A gradient tensor is defined only
 * after the flush that follows its entry point; the bits are those of the eager form.  Off by default.
 * ABI 9: inside such a window ng_embed_bwd of a molecule-sized call (N <= 2048) launches nothing of its own — its sum
 * is a job of the flush launch that reads `atoms` and `dh0` THEN: both must stay valid and unchanged until the flush
 * (the same holds for the caller-owned `partial` of ng_head_loss_reduce). */
int ng_defer_reductions(ng_ctx* ctx, void* stream, int on);
int ng_flush_reductions(ng_ctx* ctx, void* stream);
/* Hint about the batch the following calls work on: the largest number of atoms of one member graph (the reference
 * concatenates molecules with offset neighbour indices, nmrgnn/library.py:106-117, so a neighbour index lies within its
 * own graph).  0 = unknown (default).  With 0 < span <= 272 the default-width neighbour aggregation (F % 128 == 0) keeps
 * slab windows of the gathered rows in LDS; larger or unknown spans (whole proteins) take the L2-gather kernel.  With
 * 0 < span <= 256, F = 256, E = 3 and no aggregate kept (a_save == NULL: inference) ng_mp_layer_fwd(_csr) runs the window
 * gather-GEMM (csrc/mp_gg.hip: the aggregate never reaches HBM); the backward's scatter-sum takes its LDS row-block form for
 * span <= 288.  Every kernel checks per tile that its window really holds the tile's sources and reads the others from
 * memory: results do not depend on the hint, a wrong hint only costs time. */
int ng_ctx_set_graph_span(ng_ctx* ctx, int64_t max_graph_atoms);
/* Pre-size the MAIN scratch workspace to at least `bytes` and allocate the fixed-size small scratch (range-guard word, gradient
 * scales, replay block).  What it guarantees: a later call whose main-workspace need is <= `bytes` neither grows nor moves that
 * block.  What it does not cover: the second ("aux") workspace of leaf kernels, the deferred-reduction arena and the cached
 * weight images and their job tables — those are sized only by a warm-up call of the same shape, in the same state (deferral,
 * frozen weights, armed), as the calls that follow. */
int ng_ctx_reserve(ng_ctx* ctx, uint64_t bytes);
/* Read-only view of the context's scratch (additive: NG_ABI_VERSION stays 9); launches nothing, synchronises nothing.  Writes
 * min(cap, 10) 64-bit words and returns how many:
 *   0 main workspace bytes   1 aux workspace bytes   2 small scratch bytes (0 until allocated)   3 chunks of the deferred-
 *   reduction arena   4 arena bytes   5 bytes of cached weight images and their job tables   6 device allocations made by the
 *   context's scratch management since ng_ctx_create   7 host synchronisations made by it (device / stream synchronise before a
 *   block is freed, the synchronous upload of a private job table)   8 deferred reductions queued since ng_ctx_create
 *   9 times a full queue (24 jobs) was run ahead of its flush. */
int ng_ctx_scratch_info(ng_ctx* ctx, uint64_t* out, int cap);

/* ---- graph replay of small calls (ABI 7; ng_replay_token / ng_replay_commit: ABI 8) -----------------------------------------------------------------------------
 * The reference trains on ONE graph per step (nmrgnn/library.py:88-89, nmrgnn/main.py:74-80) and predicts one structure per
 * call (main.py:236-245): ~33 / ~8 launches of a few microseconds each, bound by the host's launch rate.  Every entry point of
 * this library is asynchronous on the stream it is given and allocates nothing once its scratch is sized: ALL of it by a warm-up
 * call of the same shape and state, the main workspace and the small scratch alone by ng_ctx_reserve (which leaves the aux
 * workspace, the reduction arena and the cached images to a warm-up call).  So a chain of calls can be CAPTURED on that
 * stream (hipStreamBeginCapture, torch.cuda.CUDAGraph) and replayed as one graph launch per shape.  Three launch arguments of a training step change from step to step and would be
 * frozen into the captured nodes: the seed of ng_add_noise(_live) and ng_head_fwd_dropout, and ng_adam_step's bias-corrected
 * rate.  While a context is ARMED those launches ignore these arguments and read the values ng_replay_stage last wrote to
 * a device block of the context:
 *   ng_replay_arm    on: arm before capturing (and leave armed while replaying: the captured nodes hold the block's address);
 *                    off: eager calls take their arguments again.
 *   ng_replay_stage  ONE eager launch per replayed step, before the graph launch: stores `seed` and Adam's rate for `step`
 *                    (the expression of ng_adam_step: same bits) and a version of its own for the images the step's armed
 *                    ng_adam_step rebuilds (a recorded launch would stamp every replay with the one version frozen into it,
 *                    and an image once flagged "weights out of the fp16 piece range" could never lose the flag: the flag
 *                    is lowered by a rebuild with ANOTHER version), clears the operand-range guard word, and copies up to 8
 *                    buffers (whole 32-bit words, device to device) — the step's inputs into the static buffers the captured
 *                    chain reads.  Inference replays need it only for the copies (seed / step are then ignored: pass step 1).
 *                    EVERY armed ng_adam_step, eager (a warm-up step) or replayed, needs a staging of its own in front of
 *                    it: it reads the staged rate, and two armed steps behind one staging would rebuild their images under
 *                    one version.
 * A replayed TRAINING step changes the weights on the device while none of the library's host code runs: ng_adam_step's
 * bookkeeping of the packed-weight-image cache (the weight version, which images its launch rebuilt) happened once, at capture.
 *   ng_replay_token   after the capture: identifies the set of cached images the captured ng_adam_step rebuilds (0: none).
 *   ng_replay_commit  after EVERY replay of a captured training step: advances the context's weight version as one
 *                     ng_adam_step does and marks exactly the images of `token` as current; every other cached image —
 *                     built by an eager call of another shape, by a big validation batch, by another captured step — is
 *                     rebuilt at its next use instead of being served with the weights of N steps ago.  An unknown token
 *                     marks nothing.  Inference replays (no weight change) do not call it.
 * nmrgnn_amd/replay.py holds the Python side (TrainStepReplay, ForwardReplay). */
int ng_replay_arm(ng_ctx* ctx, int on);
int ng_replay_stage(ng_ctx* ctx, void* stream, uint64_t seed, float lr, float beta1, float beta2, int64_t step, int n_copies,
                    const void* const* src, void* const* dst, const uint64_t* bytes);
int ng_replay_token(ng_ctx* ctx, uint64_t* token);
int ng_replay_commit(ng_ctx* ctx, uint64_t token);

/* per-kernel hipEvent bracketing for bench.py's roofline leg */
int ng_prof_enable(ng_ctx* ctx, int on);
int ng_prof_reset(ng_ctx* ctx);
/* synchronises the recorded events; returns number of distinct kernel names (<= cap).
 * names[i] points to a static string; total_ms[i] / count[i] aggregate launches. */
int ng_prof_read(ng_ctx* ctx, int cap, const char** names, double* total_ms, int64_t* count);

/* ---- RNG (explicit draws so that tests can feed the same numbers to the oracle) ------------ */
/* xi ~ N(0,1): the draw inside keras GaussianNoise, nmrgnn/model.py:213,253 */
int ng_randn(ng_ctx*, void* stream, uint64_t seed, uint64_t offset, float* out, int64_t n);
/* keras Dropout keep-mask, nmrgnn/model.py:216-219,266-267: out = 1/keep with prob keep, else 0 */
int ng_dropout_mask(ng_ctx*, void* stream, uint64_t seed, uint64_t offset, float keep, float* out,
                    int64_t n);

/* out = x + alpha*xi with the xi of ng_randn(seed, offset): GaussianNoise (nmrgnn/model.py:213,253) in one launch
 * instead of ng_randn + ng_add_scaled; the bits are those of the two-call form */
int ng_add_noise(ng_ctx*, void* stream, uint64_t seed, uint64_t offset, int64_t n, const float* x, float alpha,
                 float* out);
/* out = x + alpha*y : applies the GaussianNoise draw, d_eff = d + sigma*xi (nmrgnn/model.py:253) */
int ng_add_scaled(ng_ctx*, void* stream, int64_t n, const float* x, const float* y, float alpha,
                  float* out);

/* RBFExpansion alone, nmrgnn/layers.py:137-140: out[n,H] = (d_src>0) * exp(-(d_eff-centers)^2/gap)
 * (pass d_src = d_eff for the unmasked layer on positive distances) */
int ng_rbf_expand(ng_ctx*, void* stream, int64_t n, int H, const float* d_src, const float* d_eff,
                  const float* centers, float gap, float* out);

/* ---- edge path: mask + RBFExpansion + EdgeFCBlock ------------------------------------------
 * replaces nmrgnn/model.py:251-261, nmrgnn/layers.py:137-140, nmrgnn/model.py:132-138.
 *   d_src  [n_edges]  raw distances (mask = d_src > 0)
 *   d_eff  [n_edges]  distances fed to the RBF (= d_src, or d_src + sigma*xi when training)
 *   centers[H], gap   RBF grid (layers.py:126-129)
 *   W[t] [in,out], b[t] [out]  host arrays (length Le) of device pointers, Keras Dense layout
 *   act    activation of the hidden layers = hypers fc_activation (model.py:35-36,123): NG_ACT_SOFTPLUS runs the fused
 *          kernels (H = 128, Le = 4, E <= 8); other codes, other shapes and E up to 256 (E % 4 == 0) the layered path
 *   e_out  [n_edges,E]
 *   z_save [Le-1, n_edges, H] softplus outputs of the hidden layers (NULL for inference): the tape handed to
 *          ng_edge_mlp_bwd; its element order inside a layer is given by ng_edge_tape_layout()
 */
int ng_edge_mlp_fwd(ng_ctx*, void* stream, int64_t n_edges, int H, int E, int Le, int act,
                    const float* d_src, const float* d_eff, const float* centers, float gap,
                    const float* const* W, const float* const* b, float* e_out, float* z_save);
/* Element order of a z_save layer for this shape (same footprint either way; depends on NG_EDGE_* switches, so ask
 * in the process that runs the kernels):
 *   0: row-major [n_edges][H]
 *   1: inside every FULL group of 32 consecutive edges the 32 x 128 block is stored in the kernels' register layout:
 *      edge r (0..31), feature 32*bo + 8*q + 4*hf + j  ->  float ((bo*4 + q)*64 + hf*32 + r)*4 + j of the group's
 *      4096; a last partial group is row-major.  (Both kernels then move whole contiguous KBs per wave.) */
int ng_edge_tape_layout(int H, int E, int Le, int act, int64_t n_edges);
/* de [n_edges,E] upstream gradient; writes dW[t], db[t] (overwrites).
 * ng_edge_mlp_bwd_tape: tape_layout = the value ng_edge_tape_layout() returned when the forward wrote z_save (the
 * layout then no longer depends on the switches in force at backward time); ng_edge_mlp_bwd == tape_layout -1 (ask again). */
int ng_edge_mlp_bwd(ng_ctx*, void* stream, int64_t n_edges, int H, int E, int Le, int act,
                    const float* d_src, const float* d_eff, const float* centers, float gap,
                    const float* const* W, const float* z_save, const float* de,
                    float* const* dW, float* const* db);
int ng_edge_mlp_bwd_tape(ng_ctx*, void* stream, int64_t n_edges, int H, int E, int Le, int act,
                         const float* d_src, const float* d_eff, const float* centers, float gap,
                         const float* const* W, const float* z_save, const float* de,
                         float* const* dW, float* const* db, int tape_layout);

/* ---- the edge path over the LIVE slots of a padded list (ABI 6) -----------------------------------------------
 * A padded slot (edges == 0) yields e == 0 and contributes to no gradient: the mask multiplies the RBF and the MLP
 * output (nmrgnn/model.py:251,257,261).  The fused edge kernels can therefore skip such slots entirely: results are the
 * ones of ng_edge_mlp_fwd / _bwd (e bit for bit; weight gradients up to the summation order over edges).
 *   ng_build_live_edges: a stable partition of the n_slots = N*K slots, once per batch, no host synchronisation:
 *     perm  [n_slots]  the live slots (edges > 0) in ascending order, then the dead ones
 *     pos   [n_slots]  row of slot g in the compacted order, -1 for a dead slot
 *     d_c   [n_slots]  d_c[r] = edges[perm[r]] for r < n_live: the compacted distances
 *     n_live[1]        device scalar
 *   ng_add_noise_live: GaussianNoise into the compacted order, out_c[pos[g]] = x[g] + alpha * xi_g with the xi_g of
 *     ng_add_noise(seed, offset) (y == NULL) or xi_g = y[g] (explicit draws); dead slots are skipped.
 *   ng_edge_mlp_fwd_live / _bwd_live: d_src_c / d_eff_c are the COMPACTED distances (n_live rows; d_eff_c = d_src_c
 *     for inference); e_out and de keep the caller's [n_slots, E] layout (dead slots of e_out are written 0);
 *     z_save [Le-1, n_slots, H]: layer stride as for n_slots rows, the first n_live rows of every layer used.
 *   ng_edge_live_supported: 1 when this shape runs the fused edge path (the only one with a live view).
 *   *n_live < 0 (ABI 8): the launch has nothing to do and returns at once — _fwd_live leaves e_out (dead slots included) and
 *     z_save untouched, _bwd_live writes dW = db = 0.  What the edge-function table's guard hands the per-edge launches when it
 *     is down (ng_edge_table_check: gate[1]). */
int ng_build_live_edges(ng_ctx*, void* stream, int64_t n_slots, const float* edges, int32_t* perm, int32_t* pos,
                        float* d_c, int32_t* n_live);
/* ng_build_incoming_lists (padded form) and ng_build_live_edges as ONE call (ABI 9): the same outputs; one launch when
 * ng_graph_lists_one_launch(N, K) != 0 (molecule-sized calls, the reference's own granularity: nmrgnn/library.py:88-89) */
int ng_build_graph_lists(ng_ctx*, void* stream, int64_t N, int K, const int32_t* nlist, const float* edges, int32_t* nlist_c,
                         int32_t* csc_ptr, int32_t* csc_edge, int32_t* perm, int32_t* pos, float* d_c, int32_t* n_live);
int ng_graph_lists_one_launch(int64_t N, int K);
int ng_add_noise_live(ng_ctx*, void* stream, uint64_t seed, uint64_t offset, int64_t n, const float* x, const float* y,
                      float alpha, const int32_t* pos, float* out_c);
int ng_edge_live_supported(int H, int E, int Le, int act);
int ng_edge_mlp_fwd_live(ng_ctx*, void* stream, int64_t n_slots, int H, int E, int Le, int act,
                         const float* d_src_c, const float* d_eff_c, const int32_t* perm, const int32_t* n_live,
                         const float* centers, float gap, const float* const* W, const float* const* b,
                         float* e_out, float* z_save);
int ng_edge_mlp_bwd_live(ng_ctx*, void* stream, int64_t n_slots, int H, int E, int Le, int act,
                         const float* d_src_c, const float* d_eff_c, const int32_t* perm, const int32_t* n_live,
                         const float* centers, float gap, const float* const* W, const float* z_save,
                         const float* de, float* const* dW, float* const* db, int tape_layout);

/* Gradients with respect to the inputs (csrc/input_grad.hip).
 * ng_edge_mlp_dinput: dd_out[slot] = sum_c de[slot][c] * J[slot][c], J = d e / d d_eff, the derivative of the edge function of
 *   ng_edge_mlp_fwd with respect to its input distance, in forward mode (value and tangent through the hidden layers, f32 MFMA,
 *   recomputed from d_eff: no tape).  perm == n_live == NULL: every slot in slot order, d_src / d_eff [n_slots]; otherwise the
 *   live view of ng_edge_mlp_fwd_live (d_src / d_eff compacted, slot of row r = perm[r], rows >= *n_live dead).  de, J_out
 *   [n_slots][E] and dd_out [n_slots] in slot layout; dead slots (d_src <= 0) get exactly 0.  J_out may be NULL.  No atomics:
 *   bitwise deterministic.  H % 16 == 0, H <= 512, 1 <= E <= 256, 2 <= Le <= 6, any activation code.  *n_live < 0 (the
 *   convention of _fwd_live / _bwd_live): the launch has nothing to do and returns at once, J_out and dd_out untouched.
 * ng_positions_grad / _csr: dpos [N][3] (N = G*n, batch-global rows) = sum over the live slots (i -> j) of
 *   dd * scale * (r_i - r_j) / |r_i - r_j| on atom i and its negative on atom j, the gradient of a function of the edges
 *   (edges = |r_i - r_j| * scale, ng_knn_graph / ng_cutoff_fill) with respect to the positions pos [N][3] at fixed lists.
 *   Padded form: nlist / edges / dd [N][K] (a slot is live when edges > 0); CSR form: row_ptr [N+1], col / row_of / dd [nnz].
 *   csc_ptr / csc_edge: the incoming-edge lists (ng_build_incoming_lists).  A gather, no atomics: bitwise deterministic.
 *   Entries that contribute nothing, here and in every ng_positions_grad* / ng_box_grad* below: dd == 0 (skipped on both
 *   ends, whatever the geometry), and an entry whose two ends coincide after the displacement policy, |u| == 0 (the cutoff
 *   builders list coincident atoms in the CSR form): the gradient of |r| at 0 is taken as 0, as the padded live rule
 *   (edges > 0) already has it.  dpos, strain and dvec stay finite for any finite dd. */
int ng_edge_mlp_dinput(ng_ctx*, void* stream, int64_t n_slots, int H, int E, int Le, int act, const float* d_src,
                       const float* d_eff, const int32_t* perm, const int32_t* n_live, const float* centers, float gap,
                       const float* const* W, const float* const* b, const float* de, float* J_out, float* dd_out);
int ng_positions_grad(ng_ctx*, void* stream, int64_t N, int K, const float* pos, const int32_t* nlist, const float* edges,
                      const float* dd, float scale, const int32_t* csc_ptr, const int32_t* csc_edge, float* dpos);
int ng_positions_grad_csr(ng_ctx*, void* stream, int64_t N, int64_t nnz, const float* pos, const int32_t* row_ptr,
                          const int32_t* col, const int32_t* row_of, const float* dd, float scale, const int32_t* csc_ptr,
                          const int32_t* csc_edge, float* dpos);
/* ng_positions_grad_pbc / _csr_pbc: the same gradient for lists built in periodic boxes (ng_knn_graph_pbc,
 *   ng_cutoff_fill_rows_pbc): along each edge the minimum-image vector, recomputed from the raw positions by the function
 *   that built the edge.  n = atoms per frame (frame of row i = i / n, N % n == 0), box / triclinic as ng_knn_graph_pbc.
 *   The gradient with respect to the box is ng_box_grad. */
int ng_positions_grad_pbc(ng_ctx*, void* stream, int64_t N, int K, const float* pos, const int32_t* nlist,
                          const float* edges, const float* dd, float scale, const int32_t* csc_ptr, const int32_t* csc_edge,
                          int n, const float* box, int triclinic, float* dpos);
int ng_positions_grad_csr_pbc(ng_ctx*, void* stream, int64_t N, int64_t nnz, const float* pos, const int32_t* row_ptr,
                              const int32_t* col, const int32_t* row_of, const float* dd, float scale,
                              const int32_t* csc_ptr, const int32_t* csc_edge, int n, const float* box, int triclinic,
                              float* dpos);
/* ng_box_grad / _csr: the box side of the same chain rule, per frame g in float64.  For a live slot e = (i -> j) with
 *   u_e the displacement that built it (csrc/pbc.cuh; r_j - r_i when open), p_e = dd_e * scale * u_e / |u_e| and n_e the
 *   integer image triple with u_e = (r_j - r_i) + n_e h_g (h_g the frame's rows a, b, c, box [G][9]):
 *     strain [G][9] = sum_e u_e (x) p_e   (symmetric: d/d(eps) of r -> r (I + eps), h -> h (I + eps); the virial is -strain)
 *     dvec   [G][9] = sum_e n_e (x) p_e   (dE/dh at fixed positions; zeros when triclinic = -1, open; may be NULL)
 *   at fixed lists and images.  G frames, graph_ptr [G+1] on the device (uniform frames: arange * n; a ragged batch its own).
 *   Padded form: nlist / edges / dd [N][K] (live when edges > 0 and dd != 0); CSR form: row_ptr [N+1], col / dd [nnz].
 *   triclinic: -1 open, 0 / 1 with box as ng_knn_graph_pbc.  Two launches on workspace scratch, no atomics: bitwise
 *   deterministic. */
int ng_box_grad(ng_ctx*, void* stream, int64_t N, int K, const float* pos, const int32_t* nlist, const float* edges,
                const float* dd, float scale, int G, const int32_t* graph_ptr, const float* box, int triclinic, double* strain,
                double* dvec);
int ng_box_grad_csr(ng_ctx*, void* stream, int64_t N, int64_t nnz, const float* pos, const int32_t* row_ptr,
                    const int32_t* col, const float* dd, float scale, int G, const int32_t* graph_ptr, const float* box,
                    int triclinic, double* strain, double* dvec);
/* The gradients of a ragged batch whose structures have boundary kinds of their own (ng_knn_graph_ragged_pbc below): graph_ptr
 *   [G+1], box [G][9] and kind [G] on the device, kind_host as there (checked when given, may be NULL).  A row's structure is
 *   found by a search of graph_ptr, and its edges use that structure's own policy.  ng_box_grad(_csr)_ragged: strain and dvec
 *   per structure, dvec = 0 for an open one.  Otherwise as ng_positions_grad_pbc / ng_box_grad. */
int ng_positions_grad_ragged_pbc(ng_ctx*, void* stream, int64_t N, int K, const float* pos, const int32_t* nlist,
                                 const float* edges, const float* dd, float scale, const int32_t* csc_ptr,
                                 const int32_t* csc_edge, int G, const int32_t* graph_ptr, const float* box,
                                 const int32_t* kind, const int32_t* kind_host, float* dpos);
int ng_positions_grad_csr_ragged_pbc(ng_ctx*, void* stream, int64_t N, int64_t nnz, const float* pos, const int32_t* row_ptr,
                                     const int32_t* col, const int32_t* row_of, const float* dd, float scale,
                                     const int32_t* csc_ptr, const int32_t* csc_edge, int G, const int32_t* graph_ptr,
                                     const float* box, const int32_t* kind, const int32_t* kind_host, float* dpos);
int ng_box_grad_ragged(ng_ctx*, void* stream, int64_t N, int K, const float* pos, const int32_t* nlist, const float* edges,
                       const float* dd, float scale, int G, const int32_t* graph_ptr, const float* box, const int32_t* kind,
                       const int32_t* kind_host, double* strain, double* dvec);
int ng_box_grad_csr_ragged(ng_ctx*, void* stream, int64_t N, int64_t nnz, const float* pos, const int32_t* row_ptr,
                           const int32_t* col, const float* dd, float scale, int G, const int32_t* graph_ptr,
                           const float* box, const int32_t* kind, const int32_t* kind_host, double* strain, double* dvec);

/* ---- node path ----------------------------------------------------------------------------- */
/* embed_layer, nmrgnn/model.py:241,262: h0 = atoms[N,C] @ Wemb[C,F] */
int ng_embed_fwd(ng_ctx*, void* stream, int64_t N, int C, int F, const float* atoms,
                 const float* Wemb, float* h0);
int ng_embed_bwd(ng_ctx*, void* stream, int64_t N, int C, int F, const float* atoms,
                 const float* dh0, float* dWemb);

/* MPLayer aggregation, nmrgnn/layers.py:33 + the (i,j)-contraction of layers.py:39-40:
 *   A[i,n,l] = sum_j e[i,j,n] * h[nlist[i,j], l]        A is [N,E,F]
 *   F a multiple of 4 in [16, 1024] for E <= 8; F in {16,32,64,128,256} for 8 < E <= 64 */
int ng_mp_aggregate(ng_ctx*, void* stream, int64_t N, int K, int F, int E, const float* h,
                    const int32_t* nlist, const float* e, float* A);

/* MPLayer + residual, nmrgnn/layers.py:26-46 and nmrgnn/model.py:165-167:
 *   P = inv_degree * einsum('ijn,ijl,lmn->im', e, h[nlist], w);  h_out = act(P) (+ h if residual:
 *   MPBlock, model.py:167; residual = 0 gives the bare MPLayer of layers.py:26-46)
 *   w is the reference layout [F,F,E].  A_save [N,E,F] and s_save [N,F] (= act(P)) are written
 *   when non-NULL (training). */
int ng_mp_layer_fwd(ng_ctx*, void* stream, int64_t N, int K, int F, int E, int act, int residual,
                    const float* h, const int32_t* nlist, const float* e, const float* inv_degree,
                    const float* w, float* h_out, float* A_save, float* s_save);
/* 1 when the backward pass of the kernel path selected for (F, E, K) reads the forward aggregate
 * (pass a [N,E,F] buffer as A_save to ng_mp_layer_fwd and hand it to ng_mp_layer_bwd), 0 when it does
 * not (pass NULL to both: the weight gradient is formed from h and the incoming-edge aggregate of dP).
 * A_save == NULL is always accepted by ng_mp_layer_bwd; paths that need the aggregate rebuild it. */
int ng_mp_layer_wants_aggregate(int F, int E, int K);

/* backward of the above.  csc_ptr[N+1], csc_edge[nnz]: incoming-edge lists (edge id = i*K+j
 * grouped by target nlist[i,j]); dh_out [N,F] upstream; writes dh_in (overwrite),
 * de (accumulate if de_accum else overwrite), dw [F,F,E] (overwrite).
 * dw == NULL: input gradients only.  No path forms the weight gradient then: no dw products, no per-workgroup partials, no
 * queued second-stage sums, no rebuilt aggregate (the F = 64 node kernel runs its dh-only form, the generic / layered / CSR
 * paths skip the dw GEMM).  dh_in and de are bit for bit those of the same call with dw given.  The same holds for
 * ng_mp_layer_bwd_rec and ng_mp_layer_bwd_csr. */
int ng_mp_layer_bwd(ng_ctx*, void* stream, int64_t N, int K, int F, int E, int act,
                    const float* h, const int32_t* nlist, const float* e, const float* inv_degree,
                    const float* w, const float* A_save, const float* s_save,
                    const int32_t* csc_ptr, const int32_t* csc_edge, const float* dh_out,
                    float* dh_in, float* de, int de_accum, float* dw);

/* Incoming-edge records for ng_mp_layer_bwd_rec: rec[p] = { source atom of CSC entry p (int bits),
 * e[edge p][0..2] }, 16 bytes per entry, nnz = csc_ptr[N] entries (buffer: 4*N*K floats).  The edge
 * features are the same for every MPLayer of a backward pass, so the records are built once and shared. */
int ng_mp_edge_records(ng_ctx*, void* stream, int64_t N, int K, int E, const int32_t* csc_ptr,
                       const int32_t* csc_edge, const float* e, float* rec);
/* ng_mp_layer_bwd with the records supplied (csc_rec may be NULL: they are then rebuilt per call).  The lists of
 * ng_build_incoming_lists hold every target's entries in ascending order of the SOURCE atom; the default-width scatter-sum
 * stages source rows block by block in that order.  Caller-built lists in another order give the same sums — entries behind
 * the staged block are read from memory — at a lower rate. */
int ng_mp_layer_bwd_rec(ng_ctx*, void* stream, int64_t N, int K, int F, int E, int act,
                    const float* h, const int32_t* nlist, const float* e, const float* inv_degree,
                    const float* w, const float* A_save, const float* s_save,
                    const int32_t* csc_ptr, const int32_t* csc_edge, const float* dh_out,
                    float* dh_in, float* de, int de_accum, float* dw, const float* csc_rec);

/* ---- CSR (variable-degree) form of the neighbour lists, SURVEY 8(b) ------------------------------------------
 * The reference's padded [N,K] tuple (nmrgnn/library.py:106-117) with the edges == 0 slots dropped — they contribute
 * exactly 0 through the edge mask (nmrgnn/model.py:251,261):
 *   row_ptr [N+1]  row i owns the entries p in [row_ptr[i], row_ptr[i+1])
 *   col     [nnz]  neighbour atom (batch-global index)          dist [nnz] distance
 * The edge path runs on the flat list: ng_edge_mlp_fwd(n_edges = nnz, d_src = dist, ...) -> e [nnz,E].
 * Same contract as ng_mp_aggregate / ng_mp_layer_fwd / ng_mp_layer_bwd (layers.py:26-46, model.py:165-167); on lists
 * that differ only by dropped zero-weight slots the results equal the padded generic path (NG_MP_PATH=layered) bit for
 * bit.  row_of [nnz] = row of entry p;  csc_ptr [N+1] / csc_edge [nnz] = entries grouped by col (ascending p inside a
 * group), the incoming-edge lists of the deterministic backward scatter. */
int ng_mp_aggregate_csr(ng_ctx*, void* stream, int64_t N, int F, int E, const float* h,
                        const int32_t* row_ptr, const int32_t* col, const float* e, float* A);
int ng_mp_layer_fwd_csr(ng_ctx*, void* stream, int64_t N, int64_t nnz, int F, int E, int act, int residual,
                        const float* h, const int32_t* row_ptr, const int32_t* col, const float* e,
                        const float* inv_degree, const float* w, float* h_out, float* A_save, float* s_save);
int ng_mp_layer_bwd_csr(ng_ctx*, void* stream, int64_t N, int64_t nnz, int F, int E, int act, const float* h,
                        const int32_t* row_ptr, const int32_t* col, const int32_t* row_of, const float* e,
                        const float* inv_degree, const float* w, const float* A_save, const float* s_save,
                        const int32_t* csc_ptr, const int32_t* csc_edge, const float* dh_out, float* dh_in,
                        float* de, int de_accum, float* dw);

/* ---- molecule-sized inference: FC block + head in one launch ------------------------------------------------------
 * nmrgnn/model.py:191-196 (FCBlock: L-1 residual softplus Dense F -> F, one softplus Dense F -> F/2) followed by
 * model.py:268-273 (out Dense F/2 -> C, full * std + avg, one-hot select) for one protein-sized graph (the reference's
 * eval-struct loop, main.py:236-245): peaks[N] from the MP block's output x[N][F], activations never leave the CU.
 * Inference only (no dropout, no tape).  Supported: F == 256, L == 4, act softplus, C <= 16, N <= 16384; anything else
 * returns NG_ERR_UNSUPPORTED and the caller uses ng_fc_block_fwd + ng_head_fwd.  Rows with a feature beyond the fp16
 * range of the split-operand products are recomputed in plain fp32 inside the kernel. */
/* One MPLayer forward (nmrgnn/layers.py:26-46; the call of ng_mp_layer_fwd without saved tensors) for a molecule-sized
 * graph in one launch: the neighbour aggregate of a workgroup's 32 atoms is formed in LDS and multiplied at once.
 * Supported: F == 256, E <= 3, K <= 32, N <= 16384, h != h_out; otherwise NG_ERR_UNSUPPORTED (use ng_mp_layer_fwd). */
int ng_mp_layer_fwd_short(ng_ctx*, void* stream, int64_t N, int K, int F, int E, int act, int residual, const float* h,
                          const int32_t* nlist, const float* e, const float* inv_degree, const float* w, float* h_out);
int ng_mp_layer_fwd_short_csr(ng_ctx*, void* stream, int64_t N, int F, int E, int act, int residual, const float* h,
                              const int32_t* row_ptr, const int32_t* col, const float* e, const float* inv_degree,
                              const float* w, float* h_out);      /* the same over CSR lists, any degree */
int ng_mp_layer_short_ok(int64_t N, int K, int F, int E);        /* 1: ng_mp_layer_fwd_short takes this shape now */
int ng_fc_head_ok(int64_t N, int F, int L, int C, int act);      /* 1: ng_fc_head_fwd takes this shape now */
int ng_fc_head_fwd(ng_ctx*, void* stream, int64_t N, int F, int L, int C, int act, const float* x,
                   const float* const* W, const float* const* b, const float* Wout, const float* bout,
                   const float* atoms, const float* pstd, const float* pavg, float* peaks);

/* ---- per-batch graph preprocessing: the incoming-edge lists of the deterministic backward scatter --------------
 * The reference hands the model a NEW graph tuple every step (nmrgnn/library.py:88-89, main.py:79); its backward is
 * TensorFlow's unsorted scatter-add behind tf.gather (layers.py:33).  The engine's backward pulls over incoming edges
 * instead, which needs, per batch, the transposed lists
 *   csc_ptr [N+1], csc_edge [<= n_entries]: the LIVE entries (eid = i*K + j for padded lists with K > 0; eid = CSR entry
 *   index when K == 0) whose neighbour is atom t, for t = 0..N-1, ascending eid inside a target (= a stable sort by
 *   target), csc_ptr[N] = number of live entries; and, for padded lists, nlist_c [N*K] (may be NULL): nlist with every
 *   entry that is not live replaced by the atom's own index eid / K (its weight is exactly 0), the list the MP kernels
 *   gather through.
 *   An entry is live when edges[eid] > 0 AND 0 <= nlist[eid] < N.  Everything else is dropped like a padded slot: a
 *   distance of 0, -0, a negative one, NaN (the same rule as ng_build_live_edges and every consumer's mask d_src > 0:
 *   "not > 0", so +inf is live), and a target outside [0, N) whatever its distance.  edges may be NULL: every entry with
 *   a target inside [0, N) is live.  csc_edge is written up to csc_ptr[N] and not beyond.
 * A deterministic counting sort in HIP; scratch comes from the context.  All pointers are device pointers; nlist may be
 * NULL only when n_entries == 0. */
int ng_build_incoming_lists(ng_ctx*, void* stream, int64_t N, int K, int64_t n_entries, const int32_t* nlist,
                            const float* edges, int32_t* nlist_c, int32_t* csc_ptr, int32_t* csc_edge);
size_t ng_incoming_lists_scratch_bytes(int64_t N, int64_t n_entries);

/* Distance-cutoff graph builder (BASELINE configs[4], "variable degree"; the counterpart of ng_knn_graph for the CSR
 * form, in front of nmrgnn/library.py:106-117): every OTHER atom of the same frame closer than `cutoff` (Angstrom).
 *   ng_cutoff_count: deg [G*n] neighbours per atom  ->  the caller's exclusive prefix sum is row_ptr [G*n+1]
 *   ng_cutoff_fill : col [nnz] batch-global (frame*n + j), ascending j inside a row; dist [nnz] = distance*scale;
 *                    inv_degree [G*n] = 1/#(local neighbour index > 0), 0 when none (library.py:115-116) */
int ng_cutoff_count(ng_ctx*, void* stream, int G, int n, float cutoff, const float* pos, int32_t* deg);
int ng_cutoff_fill(ng_ctx*, void* stream, int G, int n, float cutoff, float scale, const float* pos,
                   const int32_t* row_ptr, int32_t* col, float* dist, float* inv_degree);
/* ng_cutoff_fill that also writes row_of[nnz], the row of every entry (NULL: not written) */
int ng_cutoff_fill_rows(ng_ctx*, void* stream, int G, int n, float cutoff, float scale, const float* pos,
                        const int32_t* row_ptr, int32_t* col, float* dist, float* inv_degree, int32_t* row_of);
/* ng_cutoff_count_pbc / ng_cutoff_fill_rows_pbc: the same lists in periodic boxes, by minimum-image distance (box /
 *   triclinic as ng_knn_graph_pbc).  The caller keeps cutoff below half the smallest perpendicular width of every box. */
int ng_cutoff_count_pbc(ng_ctx*, void* stream, int G, int n, float cutoff, const float* pos, const float* box, int triclinic,
                        int32_t* deg);
int ng_cutoff_fill_rows_pbc(ng_ctx*, void* stream, int G, int n, float cutoff, float scale, const float* pos,
                            const float* box, int triclinic, const int32_t* row_ptr, int32_t* col, float* dist,
                            float* inv_degree, int32_t* row_of);
/* out[0..n] = exclusive prefix sums of in[0..n-1], out[n] = total (row_ptr from ng_cutoff_count's degrees) */
int ng_exclusive_scan_i32(ng_ctx*, void* stream, int64_t n, const int32_t* in, int32_t* out);

/* ---- receptive-field pruning (csrc/prune.hip; additive in ABI 9) -------------------------------------------------
 * The model is strictly local: the shift of an atom depends on the atoms within mp_layers list steps of it.  These
 * calls restrict a batch to what can reach the SELECTED atoms and expand results back to the parent's shape.  Lists
 * are padded (K > 0: nlist / edges [N*K]) or CSR (K == 0: row_ptr [N+1], row_of [n_entries], nlist = col, edges =
 * dist); an entry is live by ng_build_incoming_lists' rule (edges > 0 AND 0 <= target < N; edges == NULL: the target
 * alone), so a padded slot (0, 0.0) never pulls atom 0 in.  Integer work and copies, no atomics on values: the same
 * inputs give the same bits.  No host synchronisation; every refusal (NG_ERR_INVALID: NULL context, hops outside
 * [0, 64], K > 64, N * K >= 2^31, NULL lists with n_entries > 0) comes before any write.
 *
 * ng_receptive_hops: seed [N] (nonzero = selected) -> hop [N]: the smallest d <= hops such that the atom is reached
 *   from a selected atom in d steps i -> nlist[i, k] along live entries (row i names the atoms whose features i
 *   reads), -1 when there is none.  One frontier round per hop, one thread per entry.  N == 0 or no seed is legal.
 * ng_prune_keep_flags: flag [N] = hop >= 0.  The caller's ng_exclusive_scan_i32 of it is idx [N+1]: the new index of
 *   every kept atom, idx[N] = M atoms kept, idx[graph_ptr[g]] = kept atoms in front of graph g.
 * ng_prune_lists (padded): for every kept atom i, r = idx[i]: keep[r] = i, hop_p[r] = hop[i], atoms_p[r, :C] and
 *   inv_degree_p[r] copied from the parent (inv_degree is NOT recomputed from the pruned row); nlist_p[r, k] =
 *   idx[nlist[i, k]], edges_p[r, k] = edges[i, k] where the slot is live and hop[i] < hops — its target is then kept by
 *   construction — and otherwise a dead slot (idx[graph_ptr[g]], 0.0), g the row's graph: the builders' (0, 0.0)
 *   shifted to the batch.  Rows at hop == hops contribute their embedding only.  Outputs are [M]-shaped.
 * ng_prune_degrees_csr: deg [N] = the parent degree of a kept row with hop < hops, else 0.  Its exclusive scan
 *   rp_full [N+1] places the kept entries; rp_full[N] = nnz_p, read in the same synchronisation as M.
 * ng_prune_lists_csr: the row outputs as above, row_ptr_p [M+1] (row_ptr_p[r] = rp_full[keep[r]], [M] = nnz_p) and
 *   col_p / dist_p / row_of_p [nnz_p]: the entries of the rows with hop < hops at the same position inside the row
 *   (NULL when nnz_p == 0).  An entry that is not live becomes (the row itself, 0.0).
 * ng_prune_expand_edge_grad: writes EVERY entry of the parent-shaped de [n_entries]: de_p of the pruned batch where the
 *   entry was kept (live, row with 0 <= hop < hops; same slot, or same position in the row through row_ptr_p), +0.0
 *   everywhere else.
 * ng_prune_expand_rows: out [N] = fill, then out[keep[r]] = v[r] for r < M (peaks, per-atom uncertainties). */
int ng_receptive_hops(ng_ctx*, void* stream, int64_t N, int K, int64_t n_entries, const int32_t* row_ptr,
                      const int32_t* row_of, const int32_t* nlist, const float* edges, const int32_t* seed, int hops,
                      int32_t* hop);
int ng_prune_keep_flags(ng_ctx*, void* stream, int64_t N, const int32_t* hop, int32_t* flag);
int ng_prune_degrees_csr(ng_ctx*, void* stream, int64_t N, int hops, const int32_t* row_ptr, const int32_t* hop,
                         int32_t* deg);
int ng_prune_lists(ng_ctx*, void* stream, int64_t N, int K, int C, int G, int hops, const int32_t* graph_ptr,
                   const int32_t* nlist, const float* edges, const float* atoms, const float* inv_degree,
                   const int32_t* hop, const int32_t* idx, int32_t* keep, int32_t* hop_p, float* atoms_p,
                   float* inv_degree_p, int32_t* nlist_p, float* edges_p);
int ng_prune_lists_csr(ng_ctx*, void* stream, int64_t N, int64_t n_entries, int C, int hops, const int32_t* row_ptr,
                       const int32_t* row_of, const int32_t* col, const float* dist, const float* atoms,
                       const float* inv_degree, const int32_t* hop, const int32_t* idx, const int32_t* rp_full,
                       int32_t* keep, int32_t* hop_p, float* atoms_p, float* inv_degree_p, int32_t* row_ptr_p,
                       int32_t* col_p, float* dist_p, int32_t* row_of_p);
int ng_prune_expand_edge_grad(ng_ctx*, void* stream, int64_t N, int K, int64_t n_entries, int hops,
                              const int32_t* row_ptr, const int32_t* row_of, const int32_t* nlist, const float* edges,
                              const int32_t* hop, const int32_t* idx, const int32_t* row_ptr_p, const float* de_p,
                              float* de);
int ng_prune_expand_rows(ng_ctx*, void* stream, int64_t N, int64_t M, const int32_t* keep, const float* v, float fill,
                         float* out);

/* ---- graph front end: K nearest neighbours per atom, per frame --------------------------------
 * Replaces the neighbour search behind nmrgnn.universe2graph (nmrgnn/library.py:106-117, external
 * nmrdata.parse_universe) and the per-frame graph construction of eval-struct (main.py:236-243).
 *   pos [G][n][3] (Angstrom) -> nlist [G*n][K] batch-global indices (frame*n + j), self excluded,
 *   ascending distance, ties -> lower index; edges [G*n][K] = distance*scale; unused slots (0, 0.0);
 *   inv_degree [G*n] = 1/#(local neighbour index > 0), 0 when none (library.py:115-116).  K <= 64. */
int ng_knn_graph(ng_ctx*, void* stream, int G, int n, int K, float scale, const float* pos,
                 int32_t* nlist, float* edges, float* inv_degree);
/* ng_knn_graph in periodic boxes (minimum-image convention): box [G][9] on the device, one box per frame as lower-triangular
 *   lattice vectors, row-major a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz) (GROMACS / MDAnalysis triclinic_vectors).
 *   triclinic = 0: orthorhombic (bx = cx = cy = 0); 1: reduced triclinic, |bx| <= ax/2, |cx| <= ax/2, |cy| <= by/2 (the
 *   host validates; other boxes are not supported).  Distances are min over lattice vectors L of |r_j - r_i + L|, from the
 *   raw positions (anywhere, not wrapped); an atom's own images are never neighbours, each atom appears at most once in a
 *   list.  Conventions, path choice (brute force / cell grid) and NG_KNN as ng_knn_graph. */
int ng_knn_graph_pbc(ng_ctx*, void* stream, int G, int n, int K, float scale, const float* pos, const float* box,
                     int triclinic, int32_t* nlist, float* edges, float* inv_degree);
/* Ragged batches: G structures of different sizes, rows concatenated, graph_ptr [G+1] on the device (gp[0] = 0, non-decreasing,
 *   gp[G] = N); max_n = the largest structure.  Only atoms of the same structure are neighbours.  Each structure's rows are
 *   bit for bit what ng_knn_graph / ng_cutoff_count / ng_cutoff_fill_rows give for that structure alone (G = 1), with the
 *   indices shifted by gp[g]: batch-global nlist / col, inv_degree = 1/#(structure-local neighbour index > 0).  One launch
 *   per pass, no host synchronisation, G bounded only by N < 2^31.
 *   ng_knn_graph_ragged: structures of >= 16384 atoms take the cell grid (as ng_knn_graph does) one call each, found from
 *   graph_ptr_host, the same [G+1] array in host memory (required when max_n >= 16384, else may be NULL).  NG_KNN as ng_knn_graph.
 *   ng_cutoff_count_ragged / ng_cutoff_fill_rows_ragged: brute force at every size; the caller's exclusive scan of deg [N]
 *   is row_ptr [N+1]; row_of may be NULL.  Open boundaries; the _pbc forms below take boxes. */
int ng_knn_graph_ragged(ng_ctx*, void* stream, int G, int64_t N, int K, float scale, const float* pos, const int32_t* graph_ptr,
                        const int32_t* graph_ptr_host, int max_n, int32_t* nlist, float* edges, float* inv_degree);
int ng_cutoff_count_ragged(ng_ctx*, void* stream, int G, int64_t N, float cutoff, const float* pos, const int32_t* graph_ptr,
                           int max_n, int32_t* deg);
int ng_cutoff_fill_rows_ragged(ng_ctx*, void* stream, int G, int64_t N, float cutoff, float scale, const float* pos,
                               const int32_t* graph_ptr, int max_n, const int32_t* row_ptr, int32_t* col, float* dist,
                               float* inv_degree, int32_t* row_of);
/* The ragged builders with one boundary kind PER STRUCTURE: kind [G] int32 on the device, -1 open, 0 orthorhombic, 1 reduced
 *   triclinic, next to box [G][9] on the device (lattice vectors as ng_knn_graph_pbc; an open structure's are not read).
 *   Each structure's rows are bit for bit what ng_knn_graph_pbc / ng_cutoff_count_pbc / ng_cutoff_fill_rows_pbc give for that
 *   structure alone with its own box and triclinic flag (the open builders for kind -1), indices shifted by gp[g]: an
 *   orthorhombic structure beside a triclinic one keeps the orthorhombic arithmetic.  kind_host: the same [G] kinds in host
 *   memory; when given, a kind outside {-1, 0, 1} is refused; ng_knn_graph_ragged_pbc requires it when max_n >= 16384 (the
 *   cell grid runs once per such structure with that structure's box and kind), otherwise it may be NULL.  Asynchronous like
 *   the open forms.  The caller keeps cutoff below half the smallest perpendicular width of every periodic structure. */
int ng_knn_graph_ragged_pbc(ng_ctx*, void* stream, int G, int64_t N, int K, float scale, const float* pos,
                            const int32_t* graph_ptr, const int32_t* graph_ptr_host, int max_n, const float* box,
                            const int32_t* kind, const int32_t* kind_host, int32_t* nlist, float* edges, float* inv_degree);
int ng_cutoff_count_ragged_pbc(ng_ctx*, void* stream, int G, int64_t N, float cutoff, const float* pos,
                               const int32_t* graph_ptr, int max_n, const float* box, const int32_t* kind,
                               const int32_t* kind_host, int32_t* deg);
int ng_cutoff_fill_rows_ragged_pbc(ng_ctx*, void* stream, int G, int64_t N, float cutoff, float scale, const float* pos,
                                   const int32_t* graph_ptr, int max_n, const float* box, const int32_t* kind,
                                   const int32_t* kind_host, const int32_t* row_ptr, int32_t* col, float* dist,
                                   float* inv_degree, int32_t* row_of);

/* AMPLayer attention aggregation, nmrgnn/layers.py:89-96 (the layer is exported by the reference package but not
 * used by its model):
 *   b[i,:] = softmax_j( inv[i] * <e[i,j,:] @ wk, h[i,:] @ wq> ),  agg[i,:] = sum_j b[i,j] * h[nlist[i,j],:]
 * The layer output is act(agg @ wv) = ng_dense_fwd(agg, wv, bias 0).  K <= 64, E <= 64. */
int ng_amp_attend(ng_ctx*, void* stream, int64_t N, int K, int F, int E, const float* h,
                  const int32_t* nlist, const float* e, const float* inv_degree, const float* wq,
                  const float* wk, float* agg);
/* Backward of ng_amp_attend (the gradient TensorFlow derives for nmrgnn/layers.py:89-96): from dagg = d loss/d agg
 * it writes dh [N,F] (both uses of the node features: the gathered values and the query), de [N,K,E], dwq [F,E] and
 * dwk [E,E].  in_ptr [N+1] / in_slot [N*K] list, for every atom t, the slots i*K+j of nlist that hold t (ALL slots:
 * the reference's softmax runs over padded slots too, layers.py:94); the sums follow the list order, no atomics.
 * The wv product in front is ng_dense_bwd. */
int ng_amp_attend_bwd(ng_ctx*, void* stream, int64_t N, int K, int F, int E, const float* h,
                      const int32_t* nlist, const float* e, const float* inv_degree, const float* wq,
                      const float* wk, const int32_t* in_ptr, const int32_t* in_slot, const float* dagg,
                      float* dh, float* de, float* dwq, float* dwk);

/* FCBlock, nmrgnn/model.py:179-196, all layers in one call:
 *   x_{l+1} = act(x_l @ W[l] + b[l]) + x_l   for l < L-1  (F -> F),   g = act(x_{L-1} @ W[L-1] + b[L-1])  (F -> F/2)
 * y[l] receives x_{l+1} (l = 0 .. L-2; the tape of the backward pass), g the block output [N,F/2].
 * W / b / y are host arrays of device pointers.  F == 64 runs one fused kernel; other sizes loop over the
 * per-layer kernels. */
int ng_fc_block_fwd(ng_ctx*, void* stream, int64_t N, int F, int L, int act, const float* x,
                    const float* const* W, const float* const* b, float* const* y, float* g);

/* backward of ng_fc_block_fwd.  x[l] = layer inputs (x[0] = block input, x[l+1] = y[l] of the forward call),
 * g = block output, dg its gradient; writes dx (gradient w.r.t. x[0]) and dW[l], db[l] (overwrites).  The
 * activation outputs are rebuilt as x[l+1] - x[l].  scratch: ng_fc_block_scratch_floats(N, F, L) floats.
 * dW == db == NULL (the pointer arrays themselves): dx only — the fused kernel (both bodies) runs its form without bias
 * sums, dW products and partials, the layered path skips the column sums, the dW GEMMs and the reductions; dx is bit for
 * bit that of the same call with dW / db given.  One of the two NULL is refused. */
/* floats of scratch ng_fc_block_bwd needs for this shape (0 when the fused kernel handles it) */
int64_t ng_fc_block_scratch_floats(int64_t N, int F, int L);
int ng_fc_block_bwd(ng_ctx*, void* stream, int64_t N, int F, int L, int act, const float* const* x,
                    const float* g, const float* const* W, const float* dg, float* dx, float* const* dW,
                    float* const* db, float* scratch);

/* keras Dense (+ residual), nmrgnn/model.py:191-196:  Y = act(X@W + b) (+ X if residual)
 *   X [M,Kin], W [Kin,Nout], b [Nout] (may be NULL: no bias), Y [M,Nout]
 *   s_save [M,Nout] = act(X@W+b) written when non-NULL
 * Shape contract of ng_dense_fwd / ng_dense_bwd: Kin and Nout multiples of 4 (any M >= 0); residual needs Kin == Nout;
 * the bias gradient (db != NULL) needs Nout <= 1024.  Anything else returns NG_ERR_INVALID before an output is written.
 * M = 0: the forward writes nothing; the backward leaves dX untouched and sets dW (and db) to 0. */
int ng_dense_fwd(ng_ctx*, void* stream, int64_t M, int Kin, int Nout, int act, int residual,
                 const float* X, const float* W, const float* b, float* Y, float* s_save);
/* dX = (residual ? dY : 0) + dP @ W^T,  dW = X^T dP,  db = colsum dP,
 * dP = dY * act'(.) recovered from s_save (softplus: 1-exp(-s); s_save may be NULL only for NG_ACT_NONE).
 * dX or db may be NULL: that output is skipped, and the others keep the bits of the call that has it. */
int ng_dense_bwd(ng_ctx*, void* stream, int64_t M, int Kin, int Nout, int act, int residual,
                 const float* X, const float* W, const float* s_save, const float* dY, float* dX,
                 float* dW, float* db);

/* dropout + out_layer + de-standardisation, nmrgnn/model.py:266-273:
 *   peaks[i] = sum_c atoms[i,c]*((g*mask)[i,:]@Wout[:,c] + bout[c])*std[c] + atoms[i,c]*avg[c] */
int ng_head_fwd(ng_ctx*, void* stream, int64_t N, int Fh, int C, const float* g,
                const float* drop_mask, const float* Wout, const float* bout, const float* atoms,
                const float* peak_std, const float* peak_avg, float* peaks);
/* the same with the keras Dropout mask (model.py:216-219,266-267) drawn inside the launch: mask_out[N,Fh] receives the
 * values of ng_dropout_mask(seed, offset, keep) over the N*Fh elements (the backward reads them) */
int ng_head_fwd_dropout(ng_ctx*, void* stream, int64_t N, int Fh, int C, const float* g, uint64_t seed, uint64_t offset,
                        float keep, float* mask_out, const float* Wout, const float* bout, const float* atoms,
                        const float* peak_std, const float* peak_avg, float* peaks);
/* Head forward with the closed-form variance of the keras Dropout in front of out_layer (nmrgnn/model.py:216-219,266-273).
 * The reference reaches that layer's randomness only by sampling model(x, training=True); dropout sits in front of the LAST
 * linear layer only, so with independent masks m_f = Bernoulli(keep)/keep
 *   delta_i = sum_f m_f g_if u_if + v_i,   u_if = sum_c atoms[i,c] std[c] Wout[f][c],   v_i = sum_c atoms[i,c] (std[c] b[c] + avg[c])
 * has mean peaks[i] (the inference value) and variance exactly
 *   var[i] = (1 - keep) / keep * sum_f (g_if u_if)^2          [ppm^2, float32]
 * peaks [N] carries the bits of ng_head_fwd(drop_mask = NULL) on the same inputs (fast form for Fh in {32,64,128}, one thread
 * per row otherwise and under NG_HEAD_PATH=generic); g is read once, one launch, no atomics, asynchronous and capturable, the
 * same bits on every call.  keep == 1 gives var exactly 0.  No range handling: (g u)^2 overflows to inf where a float32
 * square does.  C outside 1..32, keep outside (0,1], NULL peaks or var are refused before any launch; N = 0 returns NG_OK. */
int ng_head_fwd_var(ng_ctx*, void* stream, int64_t N, int Fh, int C, const float* g, float keep,
                    const float* Wout, const float* bout, const float* atoms,
                    const float* peak_std, const float* peak_avg, float* peaks, float* var);
/* Moments over S replicas of one structure (S noisy forwards of nmrgnn/model.py:253 GaussianNoise, or S perturbed coordinate
 * sets): mu [S][N] predicted shifts, v [S][N] their dropout variances from ng_head_fwd_var (or NULL).  With d_s = mu_s - mu_0
 *   mean[i] = mu_0 + sum d / S,   var_input[i] = max(0, (sum d^2 - (sum d)^2 / S) / (S - 1))  (unbiased; 0 for S = 1),
 *   var_model[i] = sum_s v_s / S          (law of total variance: Var(delta_i) = var_model + var_input)
 * One thread per atom, replicas in their order, float64 sums, each result rounded to float32 once; a column of equal values
 * gives var_input exactly 0.  No atomics, deterministic, capturable.  Refused: S < 1; NULL mu, mean or var_input; one of
 * v / var_model NULL without the other. */
int ng_ensemble_moments(ng_ctx*, void* stream, int S, int64_t N, const float* mu, const float* v,
                        float* mean, float* var_input, float* var_model);
/* backward of ng_head_fwd: dg [N,Fh] (overwrite), dWout [Fh,C] and dbout [C] (overwrite).  dWout == dbout == NULL: dg only,
 * bit for bit that of the same call with them given; no weight-gradient sums, partials or reductions are formed (fast and
 * generic forms).  One of the two NULL is refused. */
int ng_head_bwd(ng_ctx*, void* stream, int64_t N, int Fh, int C, const float* g,
                const float* drop_mask, const float* Wout, const float* atoms,
                const float* peak_std, const float* dpeaks, float* dg, float* dWout, float* dbout);

/* Head forward + NameLoss with s = 1 (ng_loss_l2) + head backward in ONE launch (ABI 9).  Replaces, for a training step whose
 * loss is the L2 NameLoss, the chain ng_head_fwd_dropout -> ng_loss_l2 -> ng_head_bwd (nmrgnn/model.py:266-273,
 * nmrgnn/losses.py:30-39): a workgroup owns whole graphs, so the graph's loss and dloss/dpeaks never leave the chip.
 * peaks and dg carry the bits of the three-call chain; dWout / dbout and the mean over graphs are summed in a different order
 * (last bits).  The loss is COMPLETE ONLY AFTER ng_head_loss_reduce (its first stage is a column of `partial`).
 *   ng_head_loss_blocks  number of workgroups = rows of `partial` the call writes (0: shape not supported — a graph longer
 *                        than 256 atoms, more than 16 elements, more graphs than the chip takes in one round of workgroups,
 *                        or a head shape ng_head_bwd's fast form does not take; use the three-call chain)
 *   keep < 1: the keras Dropout mask of ng_dropout_mask(seed, offset, keep) is applied (mask_out[N,Fh] optional: may be NULL);
 *   keep == 1: no dropout.  grad_weight multiplies dloss/dpeaks (uneven data-parallel shards), 1 = none.
 *   partial [blocks][Fh*C + C + 1]: first-stage sums of [dWout ; dbout ; loss]; ng_head_loss_reduce finishes them (queued behind
 *   ng_defer_reductions like every other second stage: the caller keeps `partial` alive until the flush). */
int ng_head_loss_blocks(ng_ctx*, int G, int Fh, int C, int64_t max_graph_atoms);
int ng_head_loss_bwd(ng_ctx*, void* stream, int64_t N, int G, int Fh, int C, int64_t max_graph_atoms, const float* g,
                     uint64_t seed, uint64_t offset, float keep, float* mask_out, const float* Wout, const float* bout,
                     const float* atoms, const float* peak_std, const float* peak_avg, const int32_t* graph_ptr,
                     const float* y, const float* w, float grad_weight, float* peaks, float* dg, float* partial);
int ng_head_loss_reduce(ng_ctx*, void* stream, const float* partial, int blocks, int Fh, int C, float* dWout, float* dbout,
                        float* loss_out);

/* ---- edge path through a table of the edge function (round 5; the Engine's default since round 6: csrc/edge_table.hip) ----
 * mask + RBFExpansion + EdgeFCBlock (nmrgnn/model.py:251-261) maps ONE scalar per edge to e[E]: e_ij = m_ij f_W(d_ij).  The
 * caller evaluates f_W with ng_edge_mlp_fwd(_live) on T equidistant points that cover the step's distances and interpolates
 * every edge (four-point cubic Lagrange, error ~ (h / 0.028)^4 < 1e-9 relative at T = 4096); the backward scatters de onto the
 * table (the exact adjoint, 64-bit fixed-point sums: order-free) and runs ng_edge_mlp_bwd on the table's rows.
 * GUARD (ABI 8).  The same launch also evaluates f_W at the T midpoints (rows T .. 2T-1); ng_edge_table_check compares the
 * interpolant with it there and decides ON THE DEVICE: gate[0] != 0 means "answer this call per edge".  The caller launches
 * ng_edge_mlp_fwd_live / _bwd_live with n_live = &gate[1] (the live row count when the guard is up, -1 = "skip" otherwise) and the
 * table's backward with n_live = &gate[2] (0 when the guard is up), so exactly one of the two paths does work; interp skips
 * itself on gate[0].  No host synchronisation.
 *   d_src  [n]     raw distances in SLOT order (mask = d_src > 0)
 *   d_eff, pos     the distances fed to the RBF: slot order (pos == NULL) or compacted, slot i at d_eff[pos[i]]
 *                  (ng_build_live_edges / ng_add_noise_live)
 *   ng_edge_table_range    range[0..1] = min / max of d_eff over the live slots, widened by pad * (max - min) on both sides
 *                          (pad > 0: a table kept over calls; equal distances: width max(1e-6, |lo| 2^-20)), when d_eff != NULL;
 *                          range[2] = max |de| over the live slots (inf if one is not finite) when de != NULL.  range: 3 device floats.
 *   ng_edge_table_points   d_tab[t] = lo + (t - 1) h, h = (hi - lo) / (T - 3), t < T;  midpoints != 0: d_tab[T + t] =
 *                          lo + (t - 1/2) h too;  ones[.] = 1 (the table's d_src: all live);  perm[.] = identity (or NULL)
 *   ng_edge_table_check    e_all [2T,E] (or NULL: only the range is checked): err = max |interpolant - f_W| over the interior
 *                          midpoints, scale = max |f_W| over the table; bad = err > tol * scale, or a value not finite, or
 *                          cover != NULL and [cover[0], cover[1]] not inside [range[0], range[1]], or prev != NULL and
 *                          prev[0] != 0.  gate (8 device int32): {bad, bad ? *n_live : -1, bad ? 0 : rows, 0, err, scale (float
 *                          bits; e_all == NULL: prev's, or 0), -, -}.
 *   ng_edge_table_interp   e_out[i][c] = m_i sum_k w_k(d_i) e_tab[i0 + k][c]   (E <= 8, T * E <= 16384: T = 2048 for E > 4); skipped on gate[0]
 *   ng_edge_table_scatter  de_tab[t][c] = sum_i m_i w_k(d_i) de[i][c] over the stencils that contain t, rows T .. rows_out-1
 *                          of de_tab zeroed (the midpoint rows of the table's backward); writes range[2].  Terms rounded to
 *                          q = 2^(ex - sh), max|de| < 2^ex, sh = 38 - max(0, ceil(log2 n) - 24); a non-finite live de: NaN rows
 * INPUT GRADIENT of the table path.  J = d f_W / d d is a function of the same scalar: the caller tabulates it with
 * ng_edge_mlp_dinput (J_out) on the table's 2T rows, guards it with ng_edge_table_check (e_all = the J rows, prev = the value
 * gate of the call: one gate word says "per edge" for either reason) and launches ng_edge_mlp_dinput with n_live = &gate[1] and
 * ng_edge_table_dinput with the gate: exactly one of the two writes dd.
 *   ng_edge_table_dinput   dd_out[i] = m_i sum_c de[i][c] sum_k w_k(d_i) j_tab[i0 + k][c]   (limits of ng_edge_table_interp, the same
 *                          stencil); de [n][E] read as whole rows (even E: de 16-byte aligned); dead slots get +0 whatever their de
 *                          holds; gate != NULL and gate[0] != 0: returns at once, dd_out untouched.  No atomics: deterministic. */
int ng_edge_table_range(ng_ctx*, void* stream, int64_t n, int E, const float* d_src, const float* d_eff, const int32_t* pos,
                        const float* de, float pad, float* range);
int ng_edge_table_points(ng_ctx*, void* stream, int T, int midpoints, const float* range, float* d_tab, float* ones, int32_t* perm);
int ng_edge_table_check(ng_ctx*, void* stream, int T, int E, const float* e_all, float tol, const float* range, const float* cover,
                        const int32_t* n_live, int rows, const int32_t* prev, int32_t* gate);
int ng_edge_table_interp(ng_ctx*, void* stream, int64_t n, int E, int T, const float* d_src, const float* d_eff,
                         const int32_t* pos, const float* range, const float* e_tab, const int32_t* gate, float* e_out);
int ng_edge_table_scatter(ng_ctx*, void* stream, int64_t n, int E, int T, int rows_out, const float* d_src, const float* d_eff,
                          const int32_t* pos, float* range, const float* de, float* de_tab);
int ng_edge_table_dinput(ng_ctx*, void* stream, int64_t n, int E, int T, const float* d_src, const float* d_eff,
                         const int32_t* pos, const float* range, const float* j_tab, const int32_t* gate, const float* de,
                         float* dd_out);

/* ---- training: NameLoss (s = 1), nmrgnn/losses.py:30-39, batched over graphs -----------------
 *   loss = mean_g  sum_{i in g} w_i (y_i - pred_i)^2 / sum_{i in g} w_i   (divide_no_nan)
 *   dpred written for backward; loss_out is one device float. */
int ng_loss_l2(ng_ctx*, void* stream, int64_t N, int G, const int32_t* graph_ptr, const float* y,
               const float* w, const float* pred, float* loss_out, float* dpred);

/* Replica-averaged chemical-shift restraint (library.ShiftRestraint).  peaks [R*n] replica-major (replica r's atom i at
 * r*n + i, the row order of R frames of one topology in one batch), targets / weights [n]:
 *   mean_i = (sum_r peaks[r*n+i]) / R        float32, summed in replica order (R = 1: exactly peaks[i])
 *   energy[0] = sum_i w_i (mean_i - y_i)^2   ONE double: float32 terms (d*d)*w summed in float64 in a fixed order
 *   dpeaks[r*n+i] = w_i * (2 * (mean_i - y_i)) / R   (R = 1: the bits of w * (2 * diff))
 * Two launches, no atomics (bitwise deterministic), asynchronous, capturable in a graph once the context's scratch holds
 * n / 256 doubles.  R * n below 2^31; n = 0 writes energy 0. */
int ng_restraint_loss(ng_ctx*, void* stream, int R, int64_t n, const float* peaks, const float* targets, const float* weights,
                      double* energy, float* dpeaks);

/* Restraint forms (library.ShiftRestraint's tolerance / replica_weights / independent / tau): the restraint of
 * ng_restraint_loss with replica weights, one energy per replica, a flat-bottom tolerance and a running average over calls.
 * peaks [R*n] replica-major, targets / weights [n] as there.  mode NG_RESTRAINT_ENSEMBLE: G = 1 group (all replicas);
 * NG_RESTRAINT_INDEPENDENT: G = R groups, group g = replica g.  Every step in float32, each product and sum rounded on its
 * own (no fused multiply-add), in this order, per group g and atom i:
 *   1. m   ensemble, c == NULL:  (sum_r peaks[r*n+i]) / R, summed in replica order — the bits of ng_restraint_loss's mean
 *          ensemble, c [R]:      (..((c_0 p_0) + c_1 p_1) + ..) + c_{R-1} p_{R-1},  p_r = peaks[r*n+i]  (c as given: the
 *                                caller normalises it)
 *          independent:          peaks[g*n+i]                                      (c must be NULL)
 *   2. a   lambda == 0, or primed[0] == 0:  a = m
 *          otherwise:                       a = (lambda * avg[g*n+i]) + ((1 - lambda) * m)
 *          lambda > 0: avg[g*n+i] = a is written back, and stage 2 sets primed[0] = 1 after every stage-1 read of it.
 *          lambda == 0: avg and primed are not touched (may be NULL).
 *   3. d = a - y_i,  e = |d| - tol_i clamped below at 0 (tol == NULL: e = |d|; a NaN stays a NaN),
 *      energy[g] = sum_i (e * e) * w_i   (float32 terms summed in float64 in a fixed order, as ng_restraint_loss),
 *      q = w_i * (2 * copysign(e, d))    (tol NULL or 0: the bits of w * (2 * d); inside the band |d| < tol: +-0)
 *      q = q * (1 - lambda)              on a call with lambda > 0 and primed[0] != 0 (da/dm; 1 on the first call)
 *   4. dpeaks[r*n+i] = q / R (ensemble, c NULL), q * c_r (ensemble, c), q for the replica's own atom (independent):
 *      the exact derivative of this call's energy with respect to this call's shifts, the running average of earlier calls
 *      held fixed.  Long memories (lambda near 1) thus give small forces, (1 - lambda) of the harmonic ones; the weights w
 *      set the force constant.
 * With c = NULL, tol = NULL (or all 0), lambda = 0 and NG_RESTRAINT_ENSEMBLE, energy[0] and dpeaks are the bits of
 * ng_restraint_loss.  Two launches, no atomics, no host synchronisation: bitwise deterministic, capturable in a graph once the
 * context's scratch holds G * n / 256 doubles; a replay reads whatever c, tol, avg and primed hold.  Refused: R * n >= 2^31,
 * lambda outside [0, 1), c in independent mode, avg or primed NULL with lambda > 0.  n = 0 writes energies of 0. */
#define NG_RESTRAINT_ENSEMBLE 0
#define NG_RESTRAINT_INDEPENDENT 1
int ng_restraint_loss_ex(ng_ctx*, void* stream, int R, int64_t n, int mode, const float* peaks, const float* targets,
                         const float* weights, const float* c, const float* tol, float lambda, float* avg, int32_t* primed,
                         double* energy, float* dpeaks);

/* NameLoss with balance s in [0,1], nmrgnn/losses.py:4-15,30-39, batched over graphs:
 *   loss = mean_g [ s*l2_g + (1-s)*(1 - r_g) ],  r = cov/(m*sqrt(clip(var_x*var_y,0,1e32))) with the
 *   weighted moments of corr_coeff (divide_no_nan); s = 1 equals ng_loss_l2.  dpred as above. */
int ng_loss_name(ng_ctx*, void* stream, int64_t N, int G, const int32_t* graph_ptr, const float* y,
                 const float* w, const float* pred, float s, float* loss_out, float* dpred);

/* Ensemble-averaged NameLoss (Engine.loss_groups; csrc/group_loss.hip): the loss of the MEAN prediction over
 * the frames of a structure.  A batch of G graphs with graph_ptr [G+1] is partitioned into Q groups by group_ptr [Q+1] (int32
 * graph indices, group_ptr[0] = 0, group_ptr[Q] = G, strictly increasing).  Group q has R_q = group_ptr[q+1] - group_ptr[q]
 * members of the same atom count n_q; member r's atom i sits at row graph_ptr[group_ptr[q]] + r * n_q + i.  mean_ptr [Q+1] is the
 * prefix sum of n_q, M = mean_ptr[Q]; flat mean index j = mean_ptr[q] + i.  All three on the device.
 *   ng_group_mean:   c == NULL:  mean_out[j] = (sum_r pred_r) / R_q, float32, summed in member order (R_q = 1: the bits of pred)
 *                    c [G]:      (..((c_0 p_0) + c_1 p_1) + ..), c_r = c[group_ptr[q] + r] as given (the caller normalises it per
 *                                group); each product and sum rounded on its own, no fused multiply-add: the order of
 *                                ng_restraint_loss_ex
 *                    y_out[j], w_out[j], names_out[j] = the rows of the group's FIRST member (names and names_out may be NULL
 *                    together)
 *   ng_group_spread: dpred[row of (r, i)] = (dmean[j] / R_q) * scale   (c == NULL)
 *                                         = (dmean[j] * c_r) * scale   (c given);  every row of dpred is written, scale = 1
 *                    multiplies by one exactly.
 * The loss between the two is ng_loss_l2 / ng_loss_name called with N := M, G := Q, graph_ptr := mean_ptr.
 * One launch each of one thread per flat mean index (M is known to the device only: the grid covers N >= M indices), no
 * atomics, no scratch, no host synchronisation: bitwise deterministic, asynchronous, capturable.  The device does not verify
 * that the members of a group have equal sizes (the caller does); a group whose members would reach outside the batch is
 * skipped, never read or written out of bounds.
 * Refused (NG_ERR_INVALID, before any launch): NULL context; Q < 1; Q > G; N >= 2^31; N < G; a NULL graph_ptr, group_ptr,
 * mean_ptr, pred, y, w, dmean or output; names NULL without names_out NULL or the reverse. */
int ng_group_mean(ng_ctx*, void* stream, int64_t N, int G, int Q, const int32_t* graph_ptr, const int32_t* group_ptr,
                  const int32_t* mean_ptr, const float* pred, const float* c, const float* y, const float* w,
                  const int32_t* names, float* mean_out, float* y_out, float* w_out, int32_t* names_out);
int ng_group_spread(ng_ctx*, void* stream, int64_t N, int G, int Q, const int32_t* graph_ptr, const int32_t* group_ptr,
                    const int32_t* mean_ptr, const float* dmean, const float* c, float scale, float* dpred);

/* Per-name shift metrics, nmrgnn/metrics.py:22-116 (NameRMSD 36-43, NameCount 64-70, NameCorr 91-116), for K <= 32 classes
 * in one pass over the atoms.  Per class k the seven float64 sums
 *   moments[K][7] = {S0 = sum m, Sd2 = sum m (y - p)^2, Sy = sum m y, Sp = sum m p, Syy = sum m y^2, Spp = sum m p^2,
 *                    Syp = sum m y p},   m_i = w_i * [bit k of member[names_i]]
 * (0 <= names_i < n_names, else the atom is in no class; w is used as given), from which the caller forms
 *   RMSD = sqrt(divide_no_nan(Sd2, S0)),  count = S0,  r = cov / (S0 sqrt(var_y var_p))  (the host's few flops).
 * accumulate = 0: moments are overwritten (the reference's assign); 1: the sums are added to them.  N = 0 writes zeros /
 * adds nothing.  Two launches (per-workgroup partials in the context's scratch, then a fixed-order sum): asynchronous,
 * bitwise deterministic, capturable in a graph. */
int ng_name_metrics(ng_ctx*, void* stream, int64_t N, const float* y, const float* w, const int32_t* names, const float* pred,
                    int n_names, const uint32_t* member, int K, int accumulate, double* moments);

/* Dense per-class moments for an evaluation report (nmrgnn/main.py:93-189, eval-tfrecords; csrc/class_moments.hip): the seven
 * sums of ng_name_metrics, in its order, for 1 <= K <= 1024 classes and 1 <= M <= 4 groupings of the name ids in one pass over
 * the atoms.  class_of [M][n_ids] int32 on the device: class_of[m][id] is the class of name id `id` under grouping m, a ROW
 * index in [0, K) or -1 for "in no class"; the caller lays the groupings out in one row space (name classes in rows [0, Kn),
 * element classes in [Kn, Kn + Ke), ...).  A value outside [-1, K) counts as -1 and is never used as an index.
 *   An atom i counts iff w[i] > 0 (false for 0, -0.0, negative values and NaN) and 0 <= names[i] < n_ids; it then counts with
 *   weight 1, not w[i] (the reference selects rows by `wi > 0` and is unweighted afterwards).  For every grouping m with
 *   c = class_of[m][names[i]] in [0, K) it adds to
 *   moments[c][7] = {S0 = count, Sd2 = sum (y - p)^2, Sy, Sp, Syy, Spp, Syp},  float64, y and p converted before any product
 *   (an id that two groupings map to the same row adds twice).
 * accumulate = 0: moments are overwritten; 1: the sums are added to them.  N = 0 writes zeros / adds nothing.  Two launches on
 * `stream` (per-workgroup partials in the context's scratch, min(ceil(N / 256), 512) workgroups whatever the device, then a
 * fixed-order sum): asynchronous, never reads the device on the host, no atomics; the same call on the same inputs writes the
 * same bits.  Capturable once the scratch holds min(ceil(N / 256), 512) * K * 7 doubles.
 * Refused (NG_ERR_INVALID, before any launch): NULL context; moments NULL; with N > 0 a NULL y, w, names or pred; class_of NULL
 * with n_ids > 0; M outside [1, 4]; K outside [1, 1024]; n_ids outside [0, 2^24]; N < 0 or N >= 2^31 - 256; accumulate other
 * than 0 or 1. */
int ng_class_moments(ng_ctx*, void* stream, int64_t N, const float* y, const float* w, const int32_t* names, const float* pred,
                     int n_ids, int M, const int32_t* class_of, int K, int accumulate, double* moments);

/* Maximum-entropy reweighting of a trajectory against measured shifts (nmrgnn_amd/reweight.py; csrc/reweight.hip; DESIGN.md
 * §7.22).  S [T][M] float32 row-major (frame t, observable m), y [M] float32 targets, lambda [M] double multipliers, logw0 [T]
 * double log prior weights (NULL: uniform, -log T; -inf: a frame of weight zero), all on the device.  In float64, S and y
 * converted before their first use:
 *   d_tm = S_tm - y_m,   a_t = logw0_t - sum_m lambda_m d_tm,   logZ = log sum_t exp(a_t),   p_t = exp(a_t - logZ),
 *   out [1 + M] = {logZ, mean_0 .. mean_{M-1}},   mean_m = sum_t p_t d_tm.
 * One pass over S for M <= 2048 (a wave owns a contiguous span of frames and keeps a running maximum, rescaling its sums only
 * when the maximum rises); two passes for 2048 < M <= 16384 (the logits go to scratch, then the sums by blocks of 256 columns).
 * Per-workgroup partials (max, sum, acc[M]) in the context's scratch are merged by a last launch in workgroup order by the
 * log-sum-exp rule.  The grid is a function of (T, M) alone — min(ceil(T / 32), 1024) workgroups of four waves (256 in the
 * two-pass form), frames [g s, (g + 1) s) for wave g with s = ceil(T / waves) — so the same call writes the same bits on any
 * device; no atomics.  Asynchronous on `stream`, never reads the device on the host; capturable once the scratch holds
 * workgroups * (2 + M) (+ T + workgroups in the two-pass form) doubles.  A span, a workgroup or a call whose frames all have
 * a_t = -inf gives (-inf, 0, 0): the call then writes logZ = -inf and mean = 0.  NaN in S, y, lambda or logw0 propagates into
 * logZ and the means: it is not handled.  S aligned to 16 bytes with M % 4 == 0 is read by 16-byte loads.
 * Refused (NG_ERR_INVALID, before any launch): NULL context; T < 1 or T >= 2^31; M < 1 or M > 16384; NULL S, y, lambda or out. */
int ng_reweight_eval(ng_ctx*, void* stream, int64_t T, int M, const float* S, const float* y, const double* logw0,
                     const double* lambda, double* out);
/* The weights of ng_reweight_eval's formulas at a given logZ (a device double, as out[0] of that call): p [T] double,
 * p_t = exp(a_t - logZ), 0 where a_t = -inf; stats [2] = {sum_t p_t log(p_t / w0_t), sum_t p_t^2} with log(p_t / w0_t) =
 * -sum_m lambda_m d_tm - logZ and a frame with p_t = 0 adding 0 to the first.  One read of S (any M <= 16384: the columns are
 * strided over the lanes, lambda and y come from the cache); the sums run over the frames of a wave in order, the four waves
 * of a workgroup in order, then a fixed tree over the workgroups in a second launch: no atomics, the same bits on every call.
 * Grid and refusals as ng_reweight_eval, plus NULL logZ, p or stats. */
int ng_reweight_weights(ng_ctx*, void* stream, int64_t T, int M, const float* S, const float* y, const double* logw0,
                        const double* lambda, const double* logZ, double* p, double* stats);
/* Weighted moments over the T frames of one structure, the weighted counterpart of ng_ensemble_moments: mu [T][N] float32
 * shifts, p [T] double weights (assumed to sum to 1; zeros allowed).  With e_t = mu_t - mu_0 (exact in float64)
 *   mean[i] = mu_0 + sum_t p_t e_t,   var[i] = max(0, sum_t p_t e_t^2 - (sum_t p_t e_t)^2)        (the population form)
 * A workgroup owns 64 atoms, its sixteen waves the frame chunks [w c, (w + 1) c), c = ceil(T / 16): frames in order inside a
 * chunk, chunks added in wave order — the order depends on (T, N) alone.  Float64 sums, each result rounded to float32 once; a
 * column of equal values gives var exactly 0.  One launch, no atomics, no scratch, capturable.  N = 0 returns NG_OK.
 * Refused: NULL context; T < 1 or T >= 2^31; N < 0 or N >= 2^31; NULL mu, p, mean or var. */
int ng_weighted_moments(ng_ctx*, void* stream, int64_t T, int64_t N, const float* mu, const double* p, float* mean, float* var);

/* Frames of a binary trajectory (DCD, Amber NetCDF-3; nmrgnn_amd/trajectory.py, csrc/traj.hip): raw [raw_bytes] is a chunk of
 * file bytes on the device holding G frames frame_stride bytes apart; out [G][n_out][3] float32 receives the positions.
 * Component c of source atom a of frame g is the 32-bit word at  g * frame_stride + off_c + a * elem_stride  (planar DCD:
 * elem_stride 4, offsets one record apart; interleaved NetCDF: elem_stride 12, offsets 4 apart).  swap = 1 reverses the bytes
 * of every word.  sel: int32 [n_out] source atoms in [0, n_src) (any order, repeats allowed), or NULL for the identity with
 * n_out == n_src; the caller validates sel (an entry outside the range reads nothing, gives a NaN and is counted).  Words move
 * as bits: NaN payloads, -0.0 and subnormals are kept.  *bad (a device int32 the caller zeroes) is increased by the number of
 * output values that are not finite, by integer atomics: an exact count.  One launch of G * ceil(n_out / 256) workgroups, output
 * rows staged through LDS and stored as consecutive words; 64-bit addressing, no scratch, capturable.  G == 0 or n_out == 0
 * returns NG_OK without a launch.  Refused (NG_ERR_INVALID, before any launch): NULL context, raw, out or bad; a negative G,
 * n_src or n_out; raw_bytes outside [0, 2^31); an offset or stride that is negative or no multiple of 4, or raw not aligned to
 * 4 bytes; swap outside {0, 1}; sel == NULL with n_out != n_src; a layout whose last word ends beyond raw_bytes:
 * (G - 1) * frame_stride + max(off) + (n_src - 1) * elem_stride + 4 > raw_bytes. */
int ng_frames_decode(ng_ctx*, void* stream, const void* raw, int64_t raw_bytes, int64_t G, int64_t frame_stride, int64_t off_x,
                     int64_t off_y, int64_t off_z, int64_t elem_stride, int swap, int64_t n_src, const int32_t* sel,
                     int64_t n_out, float* out, int* bad);

/* Mini-batch collation from a device-resident record store (nmrgnn_amd/dataset.py: ShiftDataset.batch; csrc/collate.hip).
 * The store holds R records back to back, record r in the rows [rec_ptr[r], rec_ptr[r+1]) of
 *   s_atoms [Ntot,C] f32, s_nlist [Ntot,K] i32 (record-LOCAL indices), s_edges [Ntot,K] f32, s_inv_degree [Ntot] f32,
 *   s_y [Ntot,3] f32 (shift, name id, mask), s_w [Ntot] f32;  rec_ptr [R+1] int64 on the device.
 * The batch is the records ids[0..G) (int32, any order, repeats allowed) in that order; graph_ptr [G+1] int32 holds their
 * batch offsets (graph_ptr[0] = 0, graph_ptr[G] = N, graph_ptr[g+1] - graph_ptr[g] = the size of record ids[g]; the caller
 * knows the sizes on the host).  Outputs, for batch row i of graph g with source row s = rec_ptr[ids[g]] + i - graph_ptr[g]:
 *   atoms[i,:] = s_atoms[s,:], nlist[i,:] = s_nlist[s,:] + graph_ptr[g] (EVERY slot, padded ones included),
 *   edges[i,:] = s_edges[s,:], inv_degree[i], w[i], y0[i] = s_y[s,0], names[i] = (int32) s_y[s,1] (truncation),
 *   y_true[i,:] = s_y[s,:] (y_true may be NULL).
 * These are the arrays of a host concatenation with offset neighbour indices, bit for bit.  One launch on `stream`,
 * asynchronous, no allocation, no atomics: a second call writes the same bits.  Source offsets are 64-bit (Ntot * K may
 * pass 2^31).  ids and graph_ptr live on the device and are not read by the host: a row whose id lies outside [0, R) or
 * whose source row lies outside its record is skipped (its outputs keep what they held), never read out of bounds.
 * Refused (NG_ERR_INVALID, before any launch): NULL context; K or C outside [1, 4096]; N < 0 or N >= 2^31 - 256; G < 1 with
 * N > 0, or G > N; R < 1 with N > 0, or Ntot < R; with N > 0 a NULL store array, ids, graph_ptr or output other than y_true.
 * N == 0 returns NG_OK and launches nothing. */
int ng_collate_batch(ng_ctx*, void* stream, int64_t R, int64_t Ntot, const float* s_atoms, const int32_t* s_nlist,
                     const float* s_edges, const float* s_inv_degree, const float* s_y, const float* s_w,
                     const int64_t* rec_ptr, const int32_t* ids, const int32_t* graph_ptr, int64_t N, int K, int C, int G,
                     float* atoms, int32_t* nlist, float* edges, float* inv_degree, float* y0, float* w, int32_t* names,
                     float* y_true);

/* A ragged kNN batch written into a record store: the inverse of ng_collate_batch (nmrgnn_amd/dataset.py:
 * ShiftDataset.from_structures; csrc/records.hip).  The batch is what structures_to_batch builds: G structures back to back,
 * graph_ptr [G+1] int32 on the device (graph_ptr[0] = 0, graph_ptr[G] = N), b_atoms [N,C] f32, b_nlist [N,K] i32 with
 * BATCH-GLOBAL indices, b_edges [N,K] f32; per atom a label shift [N] f32 (a non-finite value: no label) and name_id [N] i32.
 * Batch row i of structure g (n_g atoms) becomes row s = row0 + i of the six store arrays (layout as ng_collate_batch, Ncap rows):
 *   slot k is live iff b_edges[i,k] > 0 (false for -0.0 and NaN): s_nlist[s,k] = b_nlist[i,k] - graph_ptr[g],
 *   s_edges[s,k] = b_edges[i,k]; every other slot holds (0, +0.0f).  A live slot whose local index lies outside [0, n_g) is
 *   written as (0, +0.0f) and counters[0] is incremented; no neighbour row is ever read.
 *   s_inv_degree[s] = 1.0f / (float)#(s_nlist[s,:] > 0), 0 when that count is 0: from the local list just written, so local
 *   index 0 never counts (nmrgnn/library.py:115-116).
 *   s_atoms[s,:] = b_atoms[i,:];  s_y[s,:] = (finite(shift[i]) ? shift[i] : 0, (float)name_id[i], mask), s_w[s] = mask,
 *   mask = finite(shift[i]) ? 1 : 0;  counters[1] gains the number of rows with mask 1.
 * counters [2] int32 on the device are added to and never reset by the call (integer adds: the totals do not depend on the
 * order).  One launch on `stream`, asynchronous, no allocation, no scratch; everything but the counters is a function of the
 * inputs alone, so a second call writes the same bits.  graph_ptr is not read by the host: whatever it holds, nothing is read or
 * written outside the N batch rows and the N store rows.
 * Refused (NG_ERR_INVALID, before any launch): NULL context; K or C outside [1, 4096]; N < 0 or N >= 2^31 - 256; G < 1 with
 * N > 0, or G > N; row0 < 0 or row0 + N > Ncap; with N > 0 any NULL pointer.  N == 0 returns NG_OK and launches nothing. */
int ng_store_from_batch(ng_ctx*, void* stream, int64_t N, int K, int C, int G, const int32_t* graph_ptr, const float* b_atoms,
                        const int32_t* b_nlist, const float* b_edges, const float* shift, const int32_t* name_id, int64_t row0,
                        int64_t Ncap, float* s_atoms, int32_t* s_nlist, float* s_edges, float* s_inv_degree, float* s_y,
                        float* s_w, int32_t* counters);

/* Per-element label statistics of a record store, or of a view of it (ShiftDataset.standards; csrc/records.hip).  Over the
 * rows of the records ids[0..Rv) (int32 on the device; an id outside [0, R) and a record whose rows do not lie in [0, Ntot]
 * are skipped) with y[row,2] > 0, the element of a row being the index of its first non-zero column of atoms [Ntot,C] (a row
 * without one is skipped):
 *   out[c][3] = (count, sum y0, sum y0^2) in float64, y0 = (double) y[row,0] converted BEFORE it is squared.
 * Two launches as ng_name_metrics (per-workgroup partials in the context's scratch, then a fixed-order sum): asynchronous,
 * no atomics, bitwise deterministic.  rec_ptr [R+1] int64 on the device.  Rv == 0 writes zeros.
 * Refused (NG_ERR_INVALID, before any launch): NULL context; C outside [1, 4096]; R < 0, Ntot < R; Rv < 0 or Rv >= 2^31; out
 * NULL; with Rv > 0 a NULL atoms, y, rec_ptr or ids. */
int ng_label_moments(ng_ctx*, void* stream, int64_t R, int64_t Ntot, int C, const float* atoms, const float* y,
                     const int64_t* rec_ptr, const int32_t* ids, int64_t Rv, double* out);

/* Keras Adam (nmrgnn/model.py:44-45): one fused pass over the flat parameter buffer.
 *   g is first multiplied by grad_scale (1/world_size after a summing all-reduce). */
int ng_adam_step(ng_ctx*, void* stream, int64_t n, float* p, const float* g, float* m, float* v,
                 float lr, float beta1, float beta2, float eps, int64_t step, float grad_scale);

/* Fine-tuning (csrc/optim.hip): Adam over parameter GROUPS of the flat buffer, and the clip factor of their gradient.
 * The groups are n_seg <= NG_ADAM_MAX_SEGMENTS half-open element ranges [seg_begin[s], seg_end[s]) of [0, n) with a rate
 * scale each — HOST arrays, sorted by begin, not overlapping (empty ranges are allowed), every scale finite and >= 0.
 * The table travels in the kernel arguments by value: no device table, no copy, the launch can be captured.
 *
 * ng_adam_step_groups: lr_t is computed exactly as ng_adam_step does; segment s is updated with the rate
 *   lr_t * seg_scale[s] (one float32 product) by the expressions of ng_adam_step.  An element of a segment of scale 0, or
 *   of no segment, keeps the bits of p, m and v, and its g is NOT READ (it may be stale, NaN or never written).  All scales 1
 *   over [0, n): the bits of ng_adam_step; a power-of-two scale: the bits of ng_adam_step called with lr * scale.
 *   clip (device pointer or NULL): every gradient is multiplied by (float)clip[0] after grad_scale; clip[0] == 1 gives the
 *   bits of clip == NULL.  The weight version is bumped and every registered image in [p, p + n) rebuilt as ng_adam_step
 *   does (also those fed by frozen segments only).  n_seg == 0 and n == 0 launch no update.
 *   Refused: an armed replay context (NG_ERR_UNSUPPORTED: a replayed step trains everything); step < 1, n_seg outside
 *   [0, 64], a range outside [0, n) or with end < begin, ranges unsorted or overlapping, a negative or non-finite scale
 *   (NG_ERR_INVALID) — before anything is launched or bumped.
 * ng_grad_clip_factor: norm = sqrt(sum over the elements of segments with scale > 0 of ((double)(g[i] * grad_scale))^2),
 *   the product rounded to float32 as Adam forms it, the squares and the sum in float64; two launches (per-workgroup partials
 *   in the context's scratch, then a fixed-order sum), no atomics: the same bits on every run.
 *   out2[0] = min(1, clipnorm / norm), and 1 where norm is 0 or not finite (a NaN gradient then reaches the weights as it
 *   would unclipped, through its own element only); out2[1] = norm.  out2 (device, 2 doubles) is what `clip` points to.
 *   Refused (NG_ERR_INVALID): the segment rules above; clipnorm not > 0 or not finite; out2 NULL; g NULL with n > 0. */
#define NG_ADAM_MAX_SEGMENTS 64
int ng_adam_step_groups(ng_ctx*, void* stream, int64_t n, float* p, const float* g, float* m, float* v, float lr, float beta1,
                        float beta2, float eps, int64_t step, float grad_scale, int n_seg, const int64_t* seg_begin,
                        const int64_t* seg_end, const float* seg_scale, const double* clip);
int ng_grad_clip_factor(ng_ctx*, void* stream, int64_t n, const float* g, float grad_scale, int n_seg, const int64_t* seg_begin,
                        const int64_t* seg_end, const float* seg_scale, double clipnorm, double* out2);

/* Gradient exchange for a caller without torch.distributed (SURVEY §8(b) suggested export, §8(e): graph-parallel data
 * parallelism needs ONE all-reduce(sum, fp32) over the flat gradient bucket per step; the reference, nmrgnn/main.py:74-80,
 * is single-device).  RCCL is bound at first use (dlopen of librccl.so): NG_ERR_UNSUPPORTED where it is absent.
 *   ng_comm_unique_id   rank 0 only: 128 opaque bytes the caller hands to every rank (MPI, a file, a socket)
 *   ng_comm_init        every rank, collectively: binds the context's GPU to a communicator of `world` ranks; world == 1
 *                       needs no id and no RCCL.  One communicator per context.
 *   ng_allreduce_grads  in-place sum of flat_grad[n] over the ranks on `stream`, asynchronous; identity in a world of one.
 *                       Divide by the world size in ng_adam_step (grad_scale).
 *   ng_comm_world       the world size of the context (1 without a communicator) */
#define NG_COMM_ID_BYTES 128
int ng_comm_unique_id(void* id_out);
int ng_comm_init(ng_ctx*, int rank, int world, const void* id);
int ng_comm_destroy(ng_ctx*);
int ng_comm_world(ng_ctx*);
int ng_allreduce_grads(ng_ctx*, void* stream, float* flat_grad, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* NMRGNN_HIP_H */
