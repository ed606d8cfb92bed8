/*
 * dexbotic_amd.h — C ABI of libdexbotic_amd.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * DB-CogACT VLA forward / training hot path (SURVEY.md §8a rows A1–A14).
 *
 * The reference (dexmal/dexbotic v0.2.0) is 100 % Python and has NO FFI boundary of its own
 * (SURVEY.md §0, §8b): every FLOP on the path is executed by torch / transformers / timm underneath
 * the reference's nn.Module classes.  This header therefore declares the boundary a reference
 * maintainer would bind *underneath* those classes; each entry point cites the reference call site
 * (file:line, relative to the reference root; "HF:" = site-packages/transformers/models) whose
 * third-party arithmetic it replaces.  INTEGRATION.md shows the ctypes binding + module swap.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless stated otherwise;
 *   - every call is asynchronous on the caller's HIP stream (`stream` = hipStream_t) and never
 *     synchronises, allocates or frees; scratch is passed in by the caller;
 *   - return 0 on success, <0 on error (dxa_status); dxa_last_error() gives a thread-local message;
 *   - dtype codes: DXA_F32 (float) / DXA_BF16 (bfloat16 bits, round-to-nearest-even);
 *   - re-entrant from several host threads / streams; no global mutable state.
 */
#ifndef DEXBOTIC_AMD_H_
#define DEXBOTIC_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dxa_stream_t; /* hipStream_t */

enum dxa_status { DXA_OK = 0, DXA_ERR_BAD_ARG = -1, DXA_ERR_UNSUPPORTED = -2, DXA_ERR_HIP = -3 };
enum dxa_dtype { DXA_F32 = 0, DXA_BF16 = 1 };
enum dxa_act {
  DXA_ACT_NONE = 0,
  DXA_ACT_GELU_ERF = 1,   /* nn.GELU()            — mm_projector/builder.py:71-79          */
  DXA_ACT_GELU_TANH = 2,  /* nn.GELU("tanh")      — cogact/action_model/dit.py:151         */
  DXA_ACT_QUICK_GELU = 3, /* x*sigmoid(1.702x)    — HF:clip/modeling_clip.py (CLIPMLP)     */
  DXA_ACT_SILU = 4,       /* x*sigmoid(x)         — HF:qwen2/modeling_qwen2.py:35-48, dit.py:30 */
  DXA_ACT_RELU = 5,       /* nn.ReLU              — memvla_arch.py:139-155 (BottleneckSE)            */
  DXA_ACT_SIGMOID = 6     /* torch.sigmoid        — memvla_arch.py:143,178 (SE gate, GateFusion)     */
};
/* operand layouts of dxa_gemm: which operand has the contraction index contiguous in memory */
enum dxa_layout {
  DXA_NT = 0, /* C[m,n] = sum_k A[m,k] B[n,k]   y = x W^T      (forward of every nn.Linear)        */
  DXA_NN = 1, /* C[m,n] = sum_k A[m,k] B[k,n]   dx = dy W      (input gradient)                     */
  DXA_TN = 2  /* C[m,n] = sum_k A[k,m] B[k,n]   dW = dy^T x    (weight gradient)                    */
};

const char* dxa_last_error(void);
int dxa_version(void);

/* ------------------------------------------------------------------------------------------------
 * GEMM with fused epilogue (MFMA: v_mfma_f32_16x16x32_bf16 for bf16, v_mfma_f32_16x16x4_f32 for
 * exact-fp32).  Replaces torch F.linear / matmul + the adjacent elementwise ops at:
 *   HF:qwen2/modeling_qwen2.py:35-48,105-235 (q/k/v/o, gate/up/down), HF:clip/modeling_clip.py:259-384,
 *   mm_projector/builder.py:71-79, cogact/action_model/dit.py:22-64,137-178 (timm Attention/Mlp),
 *   HF:clip/modeling_clip.py:149-155 (patch-embed conv as a GEMM over im2col rows),
 *   and the autograd-generated dX / dW matmuls of all of them.
 *   v = alpha * sum_k(...) ; v += bias[n] ; if aux_out: aux_out[m,n] = v ; v = act(v) ;
 *   if mulgrad: v *= act'(mulgrad[m,n]) (act given by `act`, v NOT activated in that case) ;
 *   v += residual[m,n] ; if accumulate: v += C[m,n] ; C[m,n] = v.
 * Batched over (nb0, nb1, nb2) with element strides per operand (0 = broadcast).
 * Any M/N/K and any leading dimension are accepted; 16-byte aligned rows take the vector path.
 * ---------------------------------------------------------------------------------------------- */
enum dxa_fuse { DXA_FUSE_NONE = 0, DXA_FUSE_SWIGLU = 1 };
typedef struct dxa_gemm_desc {
  int32_t layout;    /* dxa_layout */
  int32_t in_dtype;  /* dtype of A, B, bias, residual, mulgrad */
  int32_t out_dtype; /* dtype of C and aux_out */
  int32_t act;       /* dxa_act */
  int64_t M, N, K;
  const void* A;
  int64_t lda;
  const void* B;
  int64_t ldb;
  void* C;
  int64_t ldc;
  const void* bias;     /* [N] or NULL */
  const void* residual; /* [M,N] (ld = ldr, batch strides = sR*) or NULL */
  int64_t ldr;
  void* aux_out; /* pre-activation copy [M,N] (ld = ldc, batch strides as C) or NULL */
  const void* mulgrad; /* [M,N] pre-activation saved by the forward (ld = ldg) or NULL */
  int64_t ldg;
  float alpha;
  int32_t accumulate; /* C += result */
  int32_t nb[3];      /* batch extents (>=1) */
  int64_t sA[3], sB[3], sC[3], sR[3], sG[3]; /* batch strides in elements */
  int32_t epi_f32;    /* 1: bias / residual / mulgrad are fp32 although A, B are bf16 (needs out_dtype fp32 and the
                         shapes of the bf16 NT fast path) — the epilogue of a split-bf16 fp32 product, see dxa_split3 */
  void* mirror;       /* fp32 output only, or NULL: a bf16 copy of the final C (after accumulate), same ldc — the
                         communication copy of a weight gradient that the data-parallel reducer exchanges instead of the
                         fp32 values (the reference's DeepSpeed bf16 run reduces bf16 gradients, script/deepspeed/zero2.json);
                         written by the dW product's own epilogue, so no cast pass over the gradient arena exists */
  float* sumsq;       /* unbatched output, or NULL: dxa_gemm_sumsq_slots(M, N) floats, ALL of them written: partial sums of
                         squares of the final C as stored (after accumulate; bf16 output: of the rounded values) whose total,
                         added in index order, is sum(C^2) — the
                         weight gradient's share of the global-norm clip (torch.nn.utils.clip_grad_norm_ in the reference's
                         Trainer, dexbotic/exp/base_exp.py:250 max_grad_norm), produced by the dW product's own epilogue
                         instead of a pass that reads the gradient back; deterministic (fixed fold order per slot) */
  const void* A2;     /* TN only, or NULL: a SECOND pair of operands A2 [K2, M] (ld = lda), B2 [K2, N] (ld = ldb) contracted into */
  const void* B2;     /* the same product: C = A^T B + A2^T B2 in ONE pass over C.  The weight gradient of a linear layer under  */
  int64_t K2;         /* gradient accumulation (the reference recipe: 8 episodes x 2 steps, dexbotic/exp/cogact_exp.py:41-46)    */
                      /* is dY1^T X1 + dY2^T X2: HF accumulates it with a read-modify-write of the fp32 gradient per micro-      */
                      /* batch; here the first micro-batch's (dY, X) are kept and the last one writes dW once                     */
  int32_t fuse;       /* dxa_fuse (0 = none).  DXA_FUSE_SWIGLU: B is the [gate ; up] matrix of a gated MLP, [N = 2 F, K] with the F gate
                         rows first (HF Qwen2MLP gate_proj / up_proj, qwen2/modeling_qwen2.py:35-48 under cogact_arch.py:97-106);
                         C [M, F] (ld = ldc) = silu(gate) * up computed in the product's own epilogue from the rounded
                         pre-activations — bit-identical to dxa_gemm + dxa_swiglu_fwd — and aux_out, if given, the pre-activations
                         [M, 2 F] (ld = ld_aux) the backward needs.  A tile takes its 128 gate and its 128 up columns of the SAME
                         128 outputs (the weight rows are picked by the operand loads: nothing is permuted in memory).
                         bf16 NT products of the MFMA fast path only (M >= 129, K % 64 == 0, F % 8 == 0, no bias / residual /
                         activation / accumulate): anything else is DXA_ERR_BAD_ARG */
  int64_t ld_aux;     /* leading dimension of aux_out when fuse != 0 */
} dxa_gemm_desc;
int dxa_gemm(const dxa_gemm_desc* d, dxa_stream_t stream);
int64_t dxa_gemm_sumsq_slots(int64_t M, int64_t N);
/* What dxa_gemm would do with a descriptor, without doing it: its argument checks (same status, same dxa_last_error text) and
 * the launches it would make.  Host arithmetic only: no pointer is dereferenced (operand pointers count by their alignment
 * alone), nothing is allocated and no GPU is needed.  A product is one step; two where it is cut in two (a K tail after the
 * MFMA-deep part, a second (A2, B2) segment the kernel cannot contract itself, the two stages of the few-row NN route);
 * none when M or N is 0. */
typedef struct dxa_gemm_step_info {
  const char* kernel;        /* the kernel instantiation, e.g. "pp<bf16,bf16,lean,nn>" (static storage) */
  int32_t grid[3], block, lds; /* workgroups, threads per workgroup, dynamic LDS bytes */
  int64_t K, K2;             /* contraction lengths of this step (K2: the second segment, contracted by the same kernel) */
  int64_t a_off, b_off;      /* byte offsets of this step's operands into A and B (seg2: into A2 and B2) */
  int32_t seg2;
  int32_t accumulate, bias, residual; /* the step adds to C / applies the bias / the residual */
  int32_t tm, tn, full, tail_r, split_s, group_m; /* tile counts; whole tiles, tail tiles cut along K, pieces per cut tile */
  int32_t vecA, vecB, vecC, vecR, vecG, vecBias;  /* 16-byte (vector) access per operand */
  int32_t ksplit, kper;      /* few-row NN route: K slices, k per slice */
  int32_t split_ws;          /* the step takes the per-stream split-K scratch */
  int32_t mirror, sumsq;     /* the kernel's own epilogue writes dxa_gemm_desc.mirror / .sumsq */
} dxa_gemm_step_info;
typedef struct dxa_gemm_plan_info {
  int32_t nsteps;
  int32_t mirror_pass, sumsq_pass; /* dxa_gemm runs the separate mirror copy / sum-of-squares pass after the steps */
  dxa_gemm_step_info step[2];
} dxa_gemm_plan_info;
int dxa_gemm_plan(const dxa_gemm_desc* d, dxa_gemm_plan_info* out);
/* name of row i of the launcher table dxa_gemm_step_info.kernel points into, NULL past its end */
const char* dxa_gemm_kernel_name(int i);

/* fp32 product on the bf16 MFMA path ("bf16x3", the counterpart of the TF32 matmuls the reference's trainer enables
 * with tf32=True, dexbotic/exp/base_exp.py:254, for the fp32 action head under autocast(float32),
 * dexbotic/model/cogact/cogact_arch.py:133): x = hi + lo with hi = bf16(x), lo = bf16(x - hi) (16 mantissa bits), and
 *   A B^T ~= A_hi B_hi^T + A_hi B_lo^T + A_lo B_hi^T = [A_hi | A_hi | A_lo] [B_hi | B_lo | B_hi]^T,
 * i.e. ONE bf16 NT product with K' = 3K accumulated in fp32 inside the MFMA.  dxa_split3 writes that operand:
 * dst[r, 0:K | K:2K | 2K:3K] = (hi, hi, lo) for side 0 (A) and (hi, lo, hi) for side 1 (B); dst is bf16 [rows, 3*cols].
 * (dxa_split3_pair with this one operand; cols and ld multiples of 4, ld >= cols, src 16-byte and dst 8-byte aligned.) */
int dxa_split3(const float* src, int64_t ld, void* dst, int64_t rows, int64_t cols, int side, dxa_stream_t stream);
/* the same operand of the TRANSPOSE in one pass: src [R, C] fp32 -> dst [C, 3 Rp] bf16 (columns R..Rp-1 of every part zero):
 * the dX = dY W and dW = dY^T X products of the fp32 heads run as NT products of transposed operands (the backward of the
 * reference's autocast(float32) head, cogact_arch.py:133 / dit.py).  dxa_split3_pair with this one transposed operand (its size
 * limit: fewer than 2^30 tiles of 32 x 32). */
int dxa_split3_t(const float* src, int64_t ld, void* dst, int64_t R, int64_t C, int64_t Rp, int side, dxa_stream_t stream);
/* BOTH operands of one such product in ONE launch (dxa_split3 and dxa_split3_t are this call with an empty second operand): a product of the fp32 heads is
 * two operand splits + the MFMA launch, and at 1088 rows a split is a few microseconds of work behind a launch's fixed cost — 1,014 of
 * MemVLA's and 288 of DB-CogACT's launches per step were operand splits.  transposed == 0: rows x cols of src -> dst [rows, 3 cols]
 * (pad unused); transposed != 0: src [rows, cols] -> dst [cols, 3 pad], pad >= rows (dxa_split3_t's R, C, Rp). */
typedef struct dxa_split3_op {
  const float* src;
  int64_t ld;
  void* dst;
  int64_t rows, cols, pad;
  int32_t side;       /* 0: (hi, hi, lo) — the A operand; 1: (hi, lo, hi) — the B operand */
  int32_t transposed;
} dxa_split3_op;
int dxa_split3_pair(const dxa_split3_op* a, const dxa_split3_op* b, dxa_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Normalisation.  w/b are [cols] in w_dtype (NULL = no affine).
 * RMSNorm follows HF:qwen2/modeling_qwen2.py:238-253: y = w * round_to_dtype(x * rsqrt(mean(x^2)+eps)).
 * LayerNorm follows torch.nn.LayerNorm as used by HF:clip/modeling_clip.py (eps 1e-5, affine) and
 * cogact/action_model/dit.py:143-147,170 (eps 1e-6, no affine).  Statistics in fp32, saved for bwd.
 * Backward writes dx (+ `residual` when given: the gradient that bypassed the normalised sub-block, same shape and
 * dtype as dx) and per-block partial dw/db into `partial` ([nblk, 2*cols] fp32; nblk returned by
 * dxa_norm_bwd_blocks(rows)); reduce them with dxa_colsum.
 * ---------------------------------------------------------------------------------------------- */
int dxa_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int64_t rows, int64_t cols,
                    float eps, int dtype, int w_dtype, dxa_stream_t stream);
int dxa_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, void* dx,
                    const void* residual, float* partial_dw, int64_t rows, int64_t cols, int dtype, int w_dtype,
                    dxa_stream_t stream);
int dxa_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd,
                      int64_t rows, int64_t cols, float eps, int dtype, int w_dtype, dxa_stream_t stream);
int dxa_layernorm_bwd(const void* dy, const void* x, const void* w, const float* mean, const float* rstd,
                      void* dx, const void* residual, float* partial_dwdb, int64_t rows, int64_t cols, int dtype,
                      int w_dtype, dxa_stream_t stream);
int dxa_norm_bwd_blocks(int64_t rows);
/* y = LayerNorm(x + res) in one launch per direction (the fuser of dexbotic/model/muvla/muvla_arch.py:44-48: ln(attn + obs)).
 * x and res are [rows, cols] of `dtype`; the sum is formed in fp32 wherever the row is read, never rounded to `dtype` and never
 * written.  mean / rstd [rows] as dxa_layernorm_fwd writes them; with res == 0 every output equals dxa_layernorm_fwd's bit for bit.
 * bwd re-forms x + res from its two inputs and writes ONE dx [rows, cols]: the same tensor is the gradient of both addends.
 * partial dw/db as dxa_layernorm_bwd ([dxa_norm_bwd_blocks(rows), 2*cols] fp32, folded by dxa_colsum; required when w is given). */
int dxa_add_layernorm_fwd(const void* x, const void* res, const void* w, const void* b, void* y, float* mean, float* rstd,
                          int64_t rows, int64_t cols, float eps, int dtype, int w_dtype, dxa_stream_t stream);
int dxa_add_layernorm_bwd(const void* dy, const void* x, const void* res, const void* w, const float* mean, const float* rstd,
                          void* dx, float* partial_dwdb, int64_t rows, int64_t cols, int dtype, int w_dtype,
                          dxa_stream_t stream);
/* 2x2 token merge + LayerNorm(4C) in one launch per direction: the `mlp_downsample` projector's DownSampleBlock followed by
 * nn.LayerNorm (dexbotic/model/modules/mm_projector/builder.py:9-33,62-69).  x [N, G*G, C], token t = r*G + c; an odd grid is
 * zero padded to Gp = G + 1 on the bottom and right; h = Gp / 2.  y [N, h*h, 4C], output token o = j*h + i (j: column pair,
 * i: row pair) = [x(2i,2j) | x(2i,2j+1) | x(2i+1,2j) | x(2i+1,2j+1)] normalised over its 4C columns (padded positions count as
 * zeros); mean / rstd [N*h*h] as dxa_layernorm_fwd writes them.  The merged, un-normalised tensor is never written.
 * bwd reads dy [N*h*h, 4C] and the UN-merged x, writes dx in the un-merged layout (every real token lies in exactly one quarter of
 * one output row: each is written once, padded positions are not written) and partial dw/db as dxa_layernorm_bwd does
 * ([dxa_norm_bwd_blocks(N*h*h), 2*4C] fp32, folded by dxa_colsum). */
int dxa_downsample_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd,
                                 int64_t N, int64_t G, int64_t C, float eps, int dtype, int w_dtype, dxa_stream_t stream);
int dxa_downsample_layernorm_bwd(const void* dy, const void* x, const void* w, const float* mean, const float* rstd,
                                 void* dx, float* partial_dwdb, int64_t N, int64_t G, int64_t C, int dtype, int w_dtype,
                                 dxa_stream_t stream);
/* OFT policy (dexbotic/model/oft/oft_arch.py).  `off` [B] int64 on the device: the un-padded length of each sample's spliced rows,
 * i.e. the first row of its block of skip + n_query rows in a [B, Sq, d] tensor.  A sample whose block does not lie inside [0, Sq)
 * is left alone by every kernel below (no access outside the tensor).
 *
 * dxa_action_put_fwd: insert_action_embedding (oft_arch.py:169-201) into rows the splice kernel reserved (zero filled):
 * x[b, off[b] + skip + j, :] = query[j, :] for j < n_query (action_query.expand over the batch, :105; `query` in `q_dtype`: the
 * dtype of x or fp32); with `state` [B, d] (the proprio projector's row, :118-121) skip = 1 and x[b, off[b], :] = state[b, :],
 * else skip = 0.  Nothing else is written.
 * dxa_action_put_bwd: dquery[j, :] (+)= sum_b dx[b, off[b] + skip + j, :] (fp32, the samples in ascending order; `accumulate`: added
 * to what dquery holds, else replaced); dstate[b, :] = dx[b, off[b], :] (dtype of dx; NULL: not wanted). */
int dxa_action_put_fwd(void* x, const void* query, const void* state, const int64_t* off, int64_t B, int64_t Sq, int64_t d,
                       int64_t n_query, int dtype, int q_dtype, dxa_stream_t stream);
int dxa_action_put_bwd(const void* dx, const int64_t* off, float* dquery, void* dstate, int64_t B, int64_t Sq, int64_t d,
                       int64_t n_query, int skip, int accumulate, int dtype, dxa_stream_t stream);
/* extract_action_hidden_states (oft_arch.py:203-210, [:, 1:] with proprio :139-140) + reshape(B, T, A*d)
 * (oft/action_model/model.py:158) + MLPResNet.layer_norm1 (:108,119) in one launch per direction.  Row (b, t) is the A*d contiguous
 * elements from h[b, off[b] + skip + t*A, 0] of the decoder output h [B, Sq, d]; y [B*T, A*d]; mean / rstd [B*T] as
 * dxa_layernorm_fwd writes them (rows of up to 4096 columns: its summation order, hence its bits).
 * bwd writes dh [B, Sq, d] COMPLETELY (dx on the action rows, zero on every other row) and partial dw | db
 * [dxa_action_layernorm_bwd_blocks(B*T), 2*A*d] fp32, folded by dxa_colsum. */
int dxa_action_layernorm_fwd(const void* h, const int64_t* off, const void* w, const void* b, void* y, float* mean, float* rstd,
                             int64_t B, int64_t Sq, int64_t d, int64_t T, int64_t A, int skip, float eps, int dtype, int w_dtype,
                             dxa_stream_t stream);
int dxa_action_layernorm_bwd(const void* dy, const void* h, const int64_t* off, const void* w, const float* mean, const float* rstd,
                             void* dh, float* partial_dwdb, int64_t B, int64_t Sq, int64_t d, int64_t T, int64_t A, int skip,
                             int dtype, int w_dtype, dxa_stream_t stream);
int dxa_action_layernorm_bwd_blocks(int64_t rows);
/* loss = mean(|pred - target|) (torch.nn.L1Loss(), oft_arch.py:152); dpred = sign(pred - target) / n * gscale with sign(0) = 0
 * (NULL: not wanted).  One workgroup, fixed reduction tree. */
int dxa_l1_loss(const float* pred, const float* target, float* loss, float* dpred, int64_t n, float gscale, dxa_stream_t stream);
/* OFT-discrete policy (dexbotic/model/oft/oft_discrete_arch.py).  `off`, `skip` and the out-of-range rule as above; a sample's block
 * is skip + n_rows rows (n_rows = chunk_size * action_dim), its action rows are h[b, off[b] + skip + j, :], j < n_rows.
 *
 * dxa_action_rows_fwd: extract_action_hidden_states (+ [:, 1:] with proprio) as the dense operand of the lm_head product:
 * y[b * n_rows + j, :] = h[b, off[b] + skip + j, :] for h [B, Sq, d], y [B * n_rows, d]; the rows of an out-of-range sample are zero.
 * dxa_action_rows_bwd writes dh [B, Sq, d] COMPLETELY: dy[b * n_rows + j, :] on the action rows, zero on every other row (as
 * dxa_action_layernorm_bwd does).  fp32 and bf16, any d (scalar accesses when a row is not a multiple of 16 bytes). */
int dxa_action_rows_fwd(const void* h, const int64_t* off, void* y, int64_t B, int64_t Sq, int64_t d, int64_t n_rows, int skip,
                        int dtype, dxa_stream_t stream);
int dxa_action_rows_bwd(const void* dy, const int64_t* off, void* dh, int64_t B, int64_t Sq, int64_t d, int64_t n_rows, int skip,
                        int dtype, dxa_stream_t stream);
/* dxa_action_fill_fwd: the discrete head's action_query is torch.ones(1, T*A) used as token ids (oft_discrete_arch.py:125-130): every
 * query row is the embedding row of token 1.  x[b, off[b] + skip + j, :] = row[:] for j < n_rows, into rows the splice kernel
 * reserved (`row` [d] in `row_dtype`: the dtype of x or fp32); with `state` [B, d] skip = 1 and x[b, off[b], :] = state[b, :].
 * dxa_action_fill_bwd: drow[:] (+)= sum_b sum_j dx[b, off[b] + skip + j, :] in fp32, in a fixed order and without atomics (the same
 * bits on every run): the action rows, numbered b * n_rows + j, are summed ascending in chunks of 16 into `partial`
 * [dxa_action_fill_bwd_blocks(B * n_rows), d] fp32, and the chunks are then added ascending (`accumulate`: onto what drow holds).
 * dstate [B, d] as dxa_action_put_bwd writes it (NULL: not wanted). */
int dxa_action_fill_fwd(void* x, const void* row, const void* state, const int64_t* off, int64_t B, int64_t Sq, int64_t d,
                        int64_t n_rows, int dtype, int row_dtype, dxa_stream_t stream);
int dxa_action_fill_bwd(const void* dx, const int64_t* off, float* drow, void* dstate, float* partial, int64_t B, int64_t Sq,
                        int64_t d, int64_t n_rows, int skip, int accumulate, int dtype, dxa_stream_t stream);
int dxa_action_fill_bwd_blocks(int64_t rows);
/* The inference head of the discrete policy in one launch (oft_discrete_arch.py:213-230): for every action row, read in place, the
 * n_bins = num_bins - 1 logits against w_bins [n_bins, d] (the last n_bins rows of lm_head.weight, which are contiguous), without a
 * gathered copy of the rows and without any [rows, vocab] tensor.
 *   bin_logits [B * n_rows, n_bins] in `dtype`: fp32 accumulation in a fixed order (MFMA over k in four interleaved strands, added
 *       in order), rounded once;
 *   bin [B * n_rows] int64: the FIRST index of the maximum of the rounded row (torch.argmax; a NaN counts as the maximum);
 *   action [B * n_rows] fp32: ((float)bin / n_bins) * 2 - 1, each operation rounded to fp32 (IEEE division, as torch's CPU kernels).
 * The rows of an out-of-range sample are computed as zero rows: logits 0, bin 0, action -1.
 * `counters`: dxa_action_bins_counters(B * n_rows) int32 words of scratch, 16-byte aligned, zeroed by the call on the stream.
 * DXA_ERR_UNSUPPORTED when d is not a multiple of 8 (bf16) / 4 (fp32) or h / w_bins / counters are not 16-byte aligned;
 * DXA_ERR_BAD_ARG for a null pointer, n_bins outside [1, 65536] or B * n_rows above 2^24. */
int dxa_action_bins_fwd(const void* h, const int64_t* off, const void* w_bins, void* bin_logits, int64_t* bin, float* action,
                        int32_t* counters, int64_t B, int64_t Sq, int64_t d, int64_t n_rows, int skip, int64_t n_bins, int dtype,
                        dxa_stream_t stream);
int dxa_action_bins_counters(int64_t rows);
/* GRPO policy update of the discrete policy (dexbotic/exp/rl/rl_trainer.py: _forward_micro_batch_update, _compute_policy_loss), on the
 * n_bins = num_bins - 1 bin logits alone: the bin rows of lm_head.weight are their own [NB, d] operand, so no [rows, vocab] tensor
 * and none of its gradient exists.  No atomics, fixed reduction order: two runs give the same bits.
 *
 * dxa_bin_logprob_fwd: logits [rows, NB] in `dtype` (fp32 or bf16), row stride ld >= NB elements, any alignment; bins [rows] int64
 * are BIN indices (token id minus the offset of the first bin token).  With z = (float)logit * inv_temperature, all in fp32 with
 * the row maximum subtracted:
 *   lse[r] = logsumexp(z),  logp[r] = z[bins[r]] - lse[r],  entropy[r] = lse[r] - sum_j softmax(z)_j z_j
 * (logprobs_from_logits_naive / entropy_from_logits, rl_trainer.py:46-55).  A bin outside [0, NB) reads nothing and gives
 * logp = NaN (the reference's gather raises); the other rows are unaffected.  One wave per row, four rows per workgroup, a loop over
 * the row for NB > 64; NB in [1, 65536].
 *
 * dxa_bin_logprob_bwd: dlogits[r, j] = coef[r] * gscale[0] * inv_temperature * ([j == bins[r]] - exp(z_j - lse[r])) in `dtype`, row
 * stride ld; dlogits may be logits itself.  gscale: DEVICE scalar, NULL = 1.  A row with coef[r] == 0 is written as zeros whatever
 * its logits hold.  The entropy has no gradient: the reference's update never puts it into the loss.
 *
 * dxa_ppo_clip_fwd: all of logp, old_logp, adv, coef fp32 [n]; mask [n] fp32 (mask_u8 = 0) or uint8 (mask_u8 = 1), non-zero = valid.
 *   ratio = exp(logp - old_logp),  pg1 = -adv * ratio,  pg2 = -adv * clamp(ratio, 1 - clip_low, 1 + clip_high)
 *   sums[4] = (sum max(pg1, pg2), sum [pg2 > pg1], sum (old_logp - logp), count) over the valid tokens
 *   inv = inv_denom when inv_denom > 0, else 1 / count (masked_mean; 0 for an empty mask);  loss[0] = inv * sums[0] (NULL: not wanted)
 *   coef[i] = d loss / d logp[i] = inv * (pg1 >= pg2 ? pg1 : 0) on a valid token, 0 on a masked one
 * The coefficient is what torch.maximum / torch.clamp autograd give, ties included: inside the clip range and on its bounds pg1 and
 * pg2 are the same number and both halves of the split gradient are -adv * ratio; outside it a tie needs adv = 0, where both are 0.
 * A masked token contributes exactly 0 also where its values are not finite.  One workgroup, fixed reduction tree (n is a trajectory
 * chunk x chunk_size x action_dim: hundreds to a few thousand).
 * All three: DXA_ERR_BAD_ARG with a message, before any launch, for a null pointer, NB outside [1, 65536], ld < NB, rows < 0, n <= 0,
 * a non-positive or non-finite inv_temperature, a clip range outside [0, 1) x [0, inf), a dtype other than DXA_F32 / DXA_BF16. */
int dxa_bin_logprob_fwd(const void* logits, int64_t ld, const int64_t* bins, float inv_temperature, float* logp, float* entropy,
                        float* lse, int64_t rows, int64_t NB, int dtype, dxa_stream_t stream);
int dxa_bin_logprob_bwd(const void* logits, int64_t ld, const int64_t* bins, const float* lse, const float* coef, const float* gscale,
                        float inv_temperature, void* dlogits, int64_t rows, int64_t NB, int dtype, dxa_stream_t stream);
int dxa_ppo_clip_fwd(const float* logp, const float* old_logp, const float* adv, const void* mask, int mask_u8, int64_t n,
                     float clip_low, float clip_high, float inv_denom, float* sums, float* loss, float* coef, dxa_stream_t stream);
/* OFT diffusion head (dexbotic/model/oft/oft_arch.py:106-116,224-250, oft/action_model/model.py:33-55,197-271).  A sample's
 * reserved block is skip + 1 + n_rows rows: [state row, with proprio: skip = 1] [time row] [n_rows = chunk_size * action_dim
 * noisy-action rows]; `off` and the out-of-range rule as for the OFT kernels above.  Every row of d elements is accessed 16 bytes at
 * a time: d must be a multiple of 8 and every row operand 16-byte aligned (DXA_ERR_BAD_ARG otherwise, as for a null pointer; a bad
 * dtype pair is DXA_ERR_UNSUPPORTED), checked before any launch.  fp32 arithmetic, fixed summation orders, no atomics.
 *
 * dxa_noisy_embed_fwd: fc1 (a Linear(1, d)) and the GELU of NoisyActionProjector in one pass, the operand of its fc2 product:
 *   h[r, c] = gelu_erf(rnd(rnd(a[r]) * w1[c] + b1[c])) for a [R] fp32, w1 / b1 [d] in `w_dtype`, h [R, d] in `dtype`; rnd rounds to
 *   `dtype` (the noisy action and the pre-activation as the reference's projector sees them in the compute dtype).
 * dxa_noisy_embed_bwd: dpre = dh * gelu_erf'(pre), pre recomputed; dw1[c] (+)= sum_r dpre[r, c] * rnd(a[r]), db1[c] (+)= sum_r
 *   dpre[r, c], both fp32: the rows are summed ascending in chunks of 16 into `partial` [dxa_noisy_embed_bwd_blocks(R), 2 d] fp32 and
 *   the chunks are then added ascending (`accumulate`: onto what dw1 / db1 hold).  Two runs give the same bits.  a has no gradient.
 * dxa_diffusion_put_fwd: into rows the splice kernel reserved, x [B, Sq, d]: x[b, off[b]] = state[b] (state [B, d] or NULL),
 *   x[b, off[b] + skip] = time[b] (time [B, d]), x[b, off[b] + skip + 1 + j] = proj[b * n_rows + j] (proj [B * n_rows, d]).
 * dxa_diffusion_put_bwd: dproj[b * n_rows + j] = dx[b, off[b] + skip + 1 + j], dstate[b] = dx[b, off[b]] (NULL: not wanted); the
 *   rows of an out-of-range sample are written as zeros.  The time row has no gradient.
 * dxa_ddim_step_embed: the two ends of one DDIM step of the sampler, one launch.  With eps [n] (`dtype`; NULL: the first step):
 *   x0 = clamp(c0 * x - c1 * eps, -clip, clip) (clip <= 0: no clamp), x <- c2 * x0 + c3 * eps, x [n] fp32 in place.  Then
 *   suffix[0, :] = time_row[:] (the next step's time row) and h[j, :] = gelu_erf(rnd(rnd(x[j]) * w1 + b1)) as dxa_noisy_embed_fwd. */
int dxa_noisy_embed_fwd(const float* a, const void* w1, const void* b1, void* h, int64_t R, int64_t d, int dtype, int w_dtype,
                        dxa_stream_t stream);
int dxa_noisy_embed_bwd(const void* dh, const float* a, const void* w1, const void* b1, float* dw1, float* db1, float* partial,
                        int64_t R, int64_t d, int accumulate, int dtype, int w_dtype, dxa_stream_t stream);
int dxa_noisy_embed_bwd_blocks(int64_t R);
int dxa_diffusion_put_fwd(void* x, const void* proj, const void* time, const void* state, const int64_t* off, int64_t B, int64_t Sq,
                          int64_t d, int64_t n_rows, int dtype, dxa_stream_t stream);
int dxa_diffusion_put_bwd(const void* dx, const int64_t* off, void* dproj, void* dstate, int64_t B, int64_t Sq, int64_t d,
                          int64_t n_rows, int skip, int dtype, dxa_stream_t stream);
int dxa_ddim_step_embed(const void* eps, float* x, float c0, float c1, float c2, float c3, float clip, const void* time_row,
                        const void* w1, const void* b1, void* suffix, void* h, int64_t n, int64_t d, int dtype, int w_dtype,
                        dxa_stream_t stream);
/* The two ends of one Euler step of the DM0-prog sampler (dexbotic/model/dm0/dm0_prog_arch.py:360-400, 567-576), one launch each.
 * A sample's suffix is p + n rows: p in {0, 1} progress rows in front of the n = chunk_size action rows; A = action_dim, da = the
 * action expert's width.  Weights, te, h and out are in `dtype` (fp32 or bf16), x / progress / prog_min fp32 with explicit sample
 * strides in elements (ldx >= n * A; the sampler keeps x and the running minimum in ONE [B, n * A + 1] tensor).  All arithmetic
 * fp32, fixed summation orders, no atomics.
 *   dxa_flow_suffix_in -> out [B * (p + n), 2 * da], the input of action_time_mlp_in:
 *       progress row:  out[:da] = progress[b] * w_p + b_p          (progress_in_proj, w_p [da, 1], b_p [da])
 *       action row i:  out[:da] = W_in . x[b, i, :] + b_in         (action_in_proj, W_in [da, A]; x rounded to `dtype` first, the
 *                                                                   sum rounded once on store)
 *       every row:     out[da:] = te[b, :]                         (te [B, da]: the step's row of the time-embedding table)
 *   dxa_flow_euler_tail, h [B * (p + n), da] the expert's rows before its final norm, g [da] the norm's gain:
 *       y = h * rsqrt(mean(h^2) + eps) * g
 *       action row i:  x[b, i, :] += dt * (W_out . y + b_out)      in place (W_out [A, da], b_out [A])
 *       progress row:  prog_min[b] = min(prog_min[b], w_q . y + b_q), a NaN prediction wins (w_q [1, da], b_q [1]); the caller
 *                      starts prog_min at +inf.  p = 0 leaves prog_min alone.
 *       y and the velocity stay fp32 in between (the composed path rounds both to `dtype`).
 * DXA_ERR_BAD_ARG before any launch: a null pointer, p outside {0, 1}, p = 1 without progress / prog_min / w_p, b_p / w_q, b_q or
 * with a stride < 1, a non-positive size, ldx < n * A, da > 8192 (a row is staged in LDS), A > 1024, B * (p + n) > 2^24. */
int dxa_flow_suffix_in(const float* x, int64_t ldx, const float* progress, int64_t ldp, const void* te, const void* w_in,
                       const void* b_in, const void* w_p, const void* b_p, void* out, int64_t B, int64_t n, int64_t A, int64_t da,
                       int p, int dtype, dxa_stream_t stream);
int dxa_flow_euler_tail(const void* h, const void* g, const void* w_out, const void* b_out, const void* w_q, const void* b_q, float* x,
                        int64_t ldx, float* prog_min, int64_t ldm, int64_t B, int64_t n, int64_t A, int64_t da, int p, float eps,
                        float dt, int dtype, dxa_stream_t stream);
/* Adaptive RMSNorm and gated residual of the pi0.5 action expert (dexbotic/model/pi05/transformers_pi05/gemma/modeling_gemma.py:
 * 38-120): no gain, a per-SAMPLE modulation mod [B, 3*cols] = [scale | shift | gate] in `dtype` (fp32 or bf16, like every row
 * tensor here).  Row `i` of the [rows, cols] tensors belongs to sample i / rows_per_sample (rows % rows_per_sample == 0).  All
 * arithmetic fp32, every output rounded once.
 *   fwd:  r = x + branch * gate_prev[s] when `branch` is given (r_out receives r; gate_prev points at the gate third of ANOTHER
 *         modulation tensor, rows gate_ld apart), r = x otherwise;  y = r * rsqrt(mean(r^2) + eps) * (1 + scale[s]) + shift[s];
 *         rstd [rows] (may be NULL).  One launch: o_proj -> gated add -> post-attention norm reads x and branch once.
 *   gated_residual_fwd:  y = x + branch * gate[s].
 *   bwd (`r`: what the norm normalised, i.e. x or r_out):  g = dy * (1 + scale[s]);  dr = rstd * (g - xh * mean(g * xh)) (+ residual);
 *         dmod [B, 3*cols]: dscale[s] = sum_rows dy * xh and dshift[s] = sum_rows dy are WRITTEN to its first two thirds (the gate
 *         third is not touched: its gradient comes from the add the gate multiplies); with `branch`: dbranch = dr * gate_prev[s] and
 *         dgate_prev[s] = sum_rows dr * branch (rows dgate_ld apart).
 *   gated_residual_bwd:  dbranch = dy * gate[s], dgate[s] = sum_rows dy * branch (the gradient of x is dy itself).
 * The per-sample sums are fp32 and deterministic (a partial row per wave, folded in a fixed order; no atomics): `partial` holds
 * B * 4 * dxa_adarms_bwd_groups(rows_per_sample) * n * cols floats, n = 3 with a branch, 2 without, 1 for gated_residual_bwd.
 * Refused with DXA_ERR_BAD_ARG: a null pointer, rows % rows_per_sample != 0, cols <= 0, a stride < cols, a partial too small. */
int dxa_adarms_fwd(const void* x, const void* branch, const void* gate_prev, int64_t gate_ld, const void* mod, void* r_out, void* y,
                   float* rstd, int64_t rows, int64_t rows_per_sample, int64_t cols, float eps, int dtype, dxa_stream_t stream);
int dxa_gated_residual_fwd(const void* x, const void* branch, const void* gate, int64_t gate_ld, void* y, int64_t rows,
                           int64_t rows_per_sample, int64_t cols, int dtype, dxa_stream_t stream);
int dxa_adarms_bwd(const void* dy, const void* r, const void* mod, const float* rstd, const void* residual, void* dr, void* dmod,
                   const void* branch, const void* gate_prev, int64_t gate_ld, void* dbranch, void* dgate_prev, int64_t dgate_ld,
                   float* partial, size_t partial_bytes, int64_t rows, int64_t rows_per_sample, int64_t cols, int dtype,
                   dxa_stream_t stream);
int dxa_gated_residual_bwd(const void* dy, const void* branch, const void* gate, int64_t gate_ld, void* dbranch, void* dgate,
                           int64_t dgate_ld, float* partial, size_t partial_bytes, int64_t rows, int64_t rows_per_sample,
                           int64_t cols, int dtype, dxa_stream_t stream);
int dxa_adarms_bwd_groups(int64_t rows_per_sample);
/* out[c] (+)= sum_r x[r*ld + c]  (bias gradients, norm-weight gradients, pos-emb gradients).
 * Deterministic two-stage reduction; scratch >= min(64, ceil(rows/32)) * cols floats. */
int dxa_colsum(const void* x, int64_t ld, float* out, int64_t rows, int64_t cols, int dtype,
               int accumulate, float* scratch, size_t scratch_bytes, dxa_stream_t stream);
/* What a norm entry point would launch, without launching it: its argument checks (same status, same dxa_last_error text) and
 * the kernel instantiation the launcher takes.  Host arithmetic only: no pointer is dereferenced (they count by their alignment
 * alone), nothing is allocated and no GPU is needed.  The entry points launch from this plan.  The descriptor holds the entry
 * point's arguments by role; a role an entry point does not have is ignored. */
enum dxa_norm_entry {
  DXA_NORM_RMSNORM_FWD = 0, DXA_NORM_RMSNORM_BWD, DXA_NORM_LAYERNORM_FWD, DXA_NORM_LAYERNORM_BWD, DXA_NORM_ADD_LAYERNORM_FWD,
  DXA_NORM_ADD_LAYERNORM_BWD, DXA_NORM_COLSUM, DXA_NORM_DOWNSAMPLE_FWD, DXA_NORM_DOWNSAMPLE_BWD, DXA_NORM_ADARMS_FWD,
  DXA_NORM_ADARMS_BWD, DXA_NORM_GATED_RESIDUAL_FWD, DXA_NORM_GATED_RESIDUAL_BWD
};
typedef struct dxa_norm_desc {
  int32_t entry;            /* dxa_norm_entry */
  int32_t dtype, w_dtype;   /* w_dtype: the norms with a gain only */
  int32_t accumulate;       /* dxa_colsum */
  int64_t rows, cols;       /* downsample: N and C */
  int64_t G;                /* downsample: the token grid */
  int64_t rows_per_sample;  /* adarms / gated residual */
  int64_t ld, gate_ld, dgate_ld; /* dxa_colsum's row stride; the gate strides of adarms / gated residual */
  size_t partial_bytes;     /* dxa_colsum's scratch_bytes; adarms / gated residual backward */
  const void* x;            /* adarms backward: r */
  const void* x2;           /* add_layernorm: res; adarms / gated residual: branch */
  const void* w;
  const void* b;
  const void* y;            /* dxa_colsum: out */
  const void* dy;
  const void* dx;           /* adarms backward: dr; gated residual backward: dbranch */
  const void* residual;
  const void* partial;      /* dxa_colsum: scratch */
  const void* mean;
  const void* rstd;
  const void* gate;         /* adarms: gate_prev */
  const void* mod;
  const void* aux;          /* adarms forward: r_out; adarms backward: dbranch */
  const void* dgate;        /* adarms backward: dgate_prev */
  const void* dmod;
  int32_t have_counters;    /* dxa_colsum: the stream's arrival counters of the fused kernel exist */
  int32_t capturing;        /* dxa_colsum: the stream is capturing (the counters cannot be allocated) */
} dxa_norm_desc;
typedef struct dxa_norm_plan_info {
  const char* kernel;       /* the instantiation, e.g. "rmsnorm_bwd_split_k<float,8,4>" (static storage); NULL: no launch */
  const char* kernel2;      /* the second launch (colsum_stage2_k, adarms_fold_k<T>), else NULL */
  const char* mode;         /* dxa_colsum: "direct", "fused" or "two_launch"; else NULL */
  int32_t vec;              /* elements per access of the row operands */
  int32_t grid[3], block, lds; /* of the first launch; lds: dynamic LDS bytes */
  int32_t nsplit;           /* dxa_colsum: row splits */
  int64_t trips;            /* trips of the row loop per wave (row slot); 1 where a wave owns one row */
} dxa_norm_plan_info;
int dxa_norm_plan(const dxa_norm_desc* d, dxa_norm_plan_info* out);
/* name of entry i of the table dxa_norm_plan_info.kernel points into, NULL past its end */
const char* dxa_norm_kernel_name(int i);

/* ------------------------------------------------------------------------------------------------
 * RoPE (rotate-half, HF:qwen2/modeling_qwen2.py:107-140) fused with the QKV split into head-major
 * [B,H,S,D] tensors.  cos/sin: [n_pos, D/2] fp32 tables built on the host exactly like
 * Qwen2RotaryEmbedding (:52-104); pos: [B*S] int32 row index into the tables (NULL -> s).
 * dxa_rope_split : qkv [B*S, (Hq+2Hkv)*D] token-major  ->  q [B,Hq,S,D], k [B,Hkv,S,D], v [B,Hkv,S,D]
 * dxa_rope_merge : inverse rotation (backward): dq,dk,dv head-major -> dqkv token-major
 * The rotation rounds each product to the dtype, then adds once (no contraction): the arithmetic of HF's
 * q * cos + rotate_half(q) * sin in that dtype, and of its autograd backward.
 * Alignment (NOT checked by the host; a misaligned operand is undefined behaviour): qkv / dqkv, q, k, v
 * (and dq, dk, dv) 16-byte aligned for fp32 and at least 8-byte aligned for bf16 (16-byte aligned bf16
 * operands with D % 16 == 0 take the 16-byte path); cos_t / sin_t 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
int dxa_rope_split(const void* qkv, void* q, void* k, void* v, const float* cos_t, const float* sin_t,
                   const int32_t* pos, int B, int S, int Hq, int Hkv, int D, int dtype,
                   dxa_stream_t stream);
int dxa_rope_merge(const void* dq, const void* dk, const void* dv, void* dqkv, const float* cos_t,
                   const float* sin_t, const int32_t* pos, int B, int S, int Hq, int Hkv, int D,
                   int dtype, dxa_stream_t stream);
/* The same with head-major tensors that hold S_cap >= S positions per (batch, head): this call's S tokens are positions
 * s0 .. s0 + S - 1 of them (several calls fill / read ONE q, k, v — the two experts of pi0's mixture layer, pi0_arch.py:130-216,
 * whose tokens share one attention call: no concatenation / slicing copies around it). */
int dxa_rope_split_at(const void* qkv, void* q, void* k, void* v, const float* cos_t, const float* sin_t, const int32_t* pos, int B,
                      int S, int Hq, int Hkv, int D, int S_cap, int s0, int dtype, dxa_stream_t stream);
int dxa_rope_merge_at(const void* dq, const void* dk, const void* dv, void* dqkv, const float* cos_t, const float* sin_t,
                      const int32_t* pos, int B, int S, int Hq, int Hkv, int D, int S_cap, int s0, int dtype, dxa_stream_t stream);
/* Qwen3's per-head RMSNorm of q and k (HF:qwen3/modeling_qwen3.py: q = rope(q_norm(q_proj(h).view(.., H, D))), likewise k; the
 * weights q_norm_w / k_norm_w [D], in the tensors' dtype, are shared by all heads; v is not normalised) inside the same pass:
 * y = w * round_to_dtype(x * rsqrt(mean_D(x^2) + eps)) per (token, head), statistics in fp32, then the rotation of dxa_rope_split.
 * D in {32, 64, 128, 256}; every tensor 16-byte aligned; fp32 and bf16.
 * dxa_qknorm_rope_split : qkv token-major -> q, k, v head-major as dxa_rope_split; rstd [B*S, Hq+Hkv] fp32 (q heads, then k heads)
 *                         is written for the backward (NULL: not written).
 * dxa_qknorm_rope_merge : dq, dk, dv head-major + the saved pre-norm qkv and rstd -> dqkv token-major in one launch: inverse
 *                         rotation, then dx = rstd * (w*dy - x_hat * mean_D(w*dy*x_hat)) per head; dv is passed through.
 *                         partial_dw (NULL: weight gradients not wanted): [dxa_qknorm_rope_merge_blocks(B*S, ..), 2*D] fp32 rows
 *                         of (dw_q | dw_k) partial sums over tokens and heads, every row written; reduce them with dxa_colsum.
 *                         No atomics: the same inputs give the same bits. */
int dxa_qknorm_rope_split(const void* qkv, void* q, void* k, void* v, const void* q_norm_w, const void* k_norm_w, float eps,
                          float* rstd, const float* cos_t, const float* sin_t, const int32_t* pos, int B, int S, int Hq, int Hkv,
                          int D, int dtype, dxa_stream_t stream);
int dxa_qknorm_rope_merge(const void* dq, const void* dk, const void* dv, const void* qkv, const float* rstd,
                          const void* q_norm_w, const void* k_norm_w, void* dqkv, float* partial_dw, const float* cos_t,
                          const float* sin_t, const int32_t* pos, int B, int S, int Hq, int Hkv, int D, int dtype,
                          dxa_stream_t stream);
int dxa_qknorm_rope_merge_blocks(int64_t tokens, int Hq, int Hkv, int D, int dtype);
/* The same into / from head-major tensors several calls share, as dxa_rope_split_at / dxa_rope_merge_at (the two Qwen3 experts of
 * DM0's mixture layer, dm0_arch.py; a key / value cache).  The split takes q and k / v APART: the S tokens go to positions
 * q0 .. q0 + S - 1 of q [B, Hq, Sq_cap, D] and to kv0 .. kv0 + S - 1 of k, v [B, Hkv, Skv_cap, D] (a sampler's queries are the
 * suffix alone while its keys land behind the cached prefix: no concatenation, no copy).  The merge reads positions
 * s0 .. s0 + S - 1 of dq, dk, dv that all hold S_cap; qkv, rstd, dqkv and partial_dw are this call's S tokens alone, as above.
 * A window outside the capacity is refused before any launch. */
int dxa_qknorm_rope_split_at(const void* qkv, void* q, void* k, void* v, const void* q_norm_w, const void* k_norm_w, float eps,
                             float* rstd, const float* cos_t, const float* sin_t, const int32_t* pos, int B, int S, int Hq, int Hkv,
                             int D, int Sq_cap, int q0, int Skv_cap, int kv0, int dtype, dxa_stream_t stream);
int dxa_qknorm_rope_merge_from(const void* dq, const void* dk, const void* dv, const void* qkv, const float* rstd,
                               const void* q_norm_w, const void* k_norm_w, void* dqkv, float* partial_dw, const float* cos_t,
                               const float* sin_t, const int32_t* pos, int B, int S, int Hq, int Hkv, int D, int S_cap, int s0,
                               int dtype, dxa_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Attention.  Replaces torch SDPA at HF:qwen2/modeling_qwen2.py:143-235 (causal + key padding, GQA),
 * HF:clip/modeling_clip.py:259-330 (full), timm Attention in dit.py:145-149 (full, 17 tokens).
 * Element (b,h,s,d) of q/k/v/o lives at base + b*sb + h*sh + s*ss + d (element strides).
 * softmax in fp32; key j is visible to query i iff kv_start[b] <= j < min(kv_end[b], q_limit[b,i]), key_valid[b,j], and
 * (!causal || j <= i + (Sk - Sq)): the last query sees the last key.  A query that sees no key gets o = 0, lse = 0 and dq = 0;
 * a key no query sees gets dk = dv = 0 (tests/attn_ref.py restates the rule; tests/test_attention_masks_gpu.py runs its edges).
 * Forward: fused flash kernel (bf16, D in {64,72,128,256} — 72 = SigLIP-So400m's head width, run on the 128-wide tiles with
 * its 72 real columns only: K/V tiles staged in LDS, MFMA QK^T and PV,
 * wavefront-shuffle softmax reductions) or a generic fp32-accumulate kernel (any dtype / D).
 * Saves lse[b,h,i] = log sum_j exp(scale*s_ij) for the backward.
 * Backward: dq/dk/dv from (q,k,v,o,do,lse); `workspace` must hold dxa_attn_bwd_workspace(desc) bytes.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dxa_attn_desc {
  int32_t dtype;
  int32_t B, Hq, Hkv, Sq, Sk, D;
  int32_t causal;
  float scale;
  const void* q; int64_t q_sb, q_sh, q_ss;
  const void* k; int64_t k_sb, k_sh, k_ss;
  const void* v; int64_t v_sb, v_sh, v_ss;
  void* o;       int64_t o_sb, o_sh, o_ss;
  float* lse;               /* [B,Hq,Sq] */
  const int32_t* kv_start;  /* [B] or NULL (=0)  */
  const int32_t* kv_end;    /* [B] or NULL (=Sk) */
  /* backward only */
  const void* d_o; int64_t do_sb, do_sh, do_ss;
  void* dq; int64_t dq_sb, dq_sh, dq_ss;
  void* dk; int64_t dk_sb, dk_sh, dk_ss;
  void* dv; int64_t dv_sb, dv_sh, dv_ss;
  int32_t force_generic;    /* testing: 1 = bypass the MFMA kernel (one wave per query row); 2 = bypass it and take the
                               materialised path of dxa_attn_fwd_ws at any size */
  /* block-prefix masks of the pi0 mixture-of-transformers attention (dexbotic/model/pi0/pi0_arch.py:22-33):
   * cumsum(ar_mask) is non-decreasing, so "cumsum[j] <= cumsum[i]" is a per-query key count; input_mask is a
   * per-key validity.  Either may be NULL.  With one of them set the generic kernels run. */
  const int32_t* q_limit;   /* [B,Sq]: query i attends keys j < q_limit[b,i] */
  const uint8_t* key_valid; /* [B,Sk]: 0 = key j is padding / a missing camera */
  /* attention dropout as torch SDPA applies it (dropout_p on the weights after the softmax): the retrieval blocks of
   * MemVLA, dexbotic/model/memvla/memvla_arch.py:120-123.  [B,Hq,Sq,Sk] contiguous in the attention dtype, entries 0 or
   * 1/(1-p), drawn by the caller; NULL = no dropout.  Runs the generic kernels. */
  const void* drop_mask;
} dxa_attn_desc;
int dxa_attn_fwd(const dxa_attn_desc* d, dxa_stream_t stream);
/* Forward with caller-provided scratch.  Problems the fused bf16 flash kernel does not take (fp32 — how the reference serves
 * pi0: pi0_exp.py:347-353, eager_attention_forward of pi0_arch.py:185-191 — or attention dropout, memvla_arch.py:120-123) and
 * that are large (Sq >= 32, Sk >= 128) are computed like the reference's eager path: S = Q K^T (batched MFMA GEMM, fp32 scores),
 * one masked row softmax (+ dropout mask), O = P V (batched GEMM).  dxa_attn_fwd_workspace() = bytes of scratch that path
 * needs (0: dxa_attn_fwd_ws behaves exactly like dxa_attn_fwd). */
size_t dxa_attn_fwd_workspace(const dxa_attn_desc* d);
int dxa_attn_fwd_ws(const dxa_attn_desc* d, void* workspace, size_t workspace_bytes, dxa_stream_t stream);
size_t dxa_attn_bwd_workspace(const dxa_attn_desc* d);
int dxa_attn_bwd(const dxa_attn_desc* d, void* workspace, size_t workspace_bytes, dxa_stream_t stream);
/* Which kernels a descriptor gets, without running them: the route of dxa_attn_fwd_ws given dxa_attn_fwd_workspace() bytes
 * (backward = 0; dxa_attn_fwd alone takes the same route minus the key-range split and the materialised path) or of
 * dxa_attn_bwd (backward != 0).  The launchers launch from the same plan.  Same argument checks, status and dxa_last_error
 * text as the entry point itself.  Host arithmetic only: no pointer is dereferenced (tensor pointers count by their
 * alignment, the mask pointers by being NULL or not), nothing is allocated and no GPU is needed. */
typedef struct dxa_attn_plan_info {
  const char* family;   /* static storage.  Forward: "tr" (attn_fwd_tr_k), "flash" (attn_fwd_flash_k), "small_f32"
                           (attn_fwd_small_f32_k), "materialised" (GEMM, attn_softmax_rows_k, GEMM), "generic" (attn_fwd_generic_k).
                           Backward: "flash" (attn_bwd_dq_k + attn_bwd_dkv_k), "small_f32" (attn_bwd_small_f32_k), "small2_f32"
                           (attn_bwd_small2_f32_k), "composed" (batched GEMMs + elementwise kernels) */
  int32_t D, DV;        /* tr / flash: width of the staged tiles and the real columns (72 on 128); otherwise both = head_dim */
  int32_t nw, nw_dkv;   /* waves per workgroup of the forward / dQ kernel and of the dK / dV kernel (0: no such kernel) */
  int32_t pf;           /* flash backward: the dK / dV kernel prefetches the next tile into registers */
  int32_t nsplit;       /* key ranges of the split forward + attn_split_combine_k (1: not split) */
  int32_t vec;          /* generic forward: elements per K load (4 or 1); 0 elsewhere */
  uint64_t workspace;   /* bytes: dxa_attn_fwd_workspace() / dxa_attn_bwd_workspace() */
} dxa_attn_plan_info;
int dxa_attn_plan(const dxa_attn_desc* d, int backward, dxa_attn_plan_info* out);

/* ------------------------------------------------------------------------------------------------
 * Elementwise / data-movement kernels (HBM-bound; 16-byte vector access).
 * ---------------------------------------------------------------------------------------------- */
/* SwiGLU, HF:qwen2/modeling_qwen2.py:46-48.  gu = [rows, 2F]: gate = cols [0,F), up = cols [F,2F). */
int dxa_swiglu_fwd(const void* gu, void* out, int64_t rows, int64_t F, int dtype, dxa_stream_t stream);
int dxa_swiglu_bwd(const void* gu, const void* dout, void* dgu, int64_t rows, int64_t F, int dtype,
                   dxa_stream_t stream);
/* gated MLP with any gate activation: out = act(gate) * up — Gemma's GeGLU (act = DXA_ACT_GELU_TANH), HF gemma/
 * modeling_gemma.py GemmaMLP as called from dexbotic/model/pi0/pi0_arch.py:205-208.  Same packing as SwiGLU. */
int dxa_glu_fwd(const void* gu, void* out, int64_t rows, int64_t F, int act, int dtype, dxa_stream_t stream);
int dxa_glu_bwd(const void* gu, const void* dout, void* dgu, int64_t rows, int64_t F, int act, int dtype,
                dxa_stream_t stream);
/* out = alpha*a + beta*b, out = a*b, out[r, n, :] = x[r, n, :] * g[r, :] — the residual / gating arithmetic of the
 * MemVLA memory modules (memvla_arch.py:160-187: SE channel gate, GateFusion lerp) */
int dxa_axpby(const void* a, const void* b, void* out, int64_t n, float alpha, float beta, int dtype, dxa_stream_t stream);
int dxa_mul(const void* a, const void* b, void* out, int64_t n, int dtype, dxa_stream_t stream);
int dxa_mul_rows(const void* x, const void* g, void* out, int64_t R, int64_t Nn, int64_t C, int dtype, dxa_stream_t stream);
int dxa_act_fwd(const void* x, void* y, int64_t n, int act, int dtype, dxa_stream_t stream);
int dxa_act_bwd(const void* x, const void* dy, void* dx, int64_t n, int act, int dtype, dxa_stream_t stream);
/* out = a + b (same dtype) */
int dxa_add(const void* a, const void* b, void* out, int64_t n, int dtype, dxa_stream_t stream);
int dxa_cast(const void* src, void* dst, int64_t n, int src_dtype, int dst_dtype, dxa_stream_t stream);
/* dst[r, 0:cols] = src[r, 0:cols] with independent leading dimensions (padding columns zeroed) */
int dxa_copy2d(const void* src, int64_t lds, void* dst, int64_t ldd, int64_t rows, int64_t cols,
               int64_t cols_padded, int src_dtype, int dst_dtype, dxa_stream_t stream);

/* dst[c, r] = src[r, c] (r < R, c < C); dst columns R..R_padded-1 are zero.  Feeds the weight-gradient GEMMs
 * (dW = dY^T X) and the transposed bf16 weight shadows (dX = dY W) as NT products into the fast MFMA path. */
int dxa_transpose(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t R, int64_t C,
                  int64_t R_padded, int dtype, dxa_stream_t stream);
/* [B,S,H,D] <-> [B,H,S,D] (to_head = 1: token-major -> head-major) */
int dxa_permute_bshd(const void* src, void* dst, int B, int S, int H, int D, int to_head, int dtype,
                     dxa_stream_t stream);

/* Token splice (dexbotic_arch.py:182-373).  plan[b*S+s] >= 0: token id; <= -1: image row -1-plan;
 * INT64_MIN: zero padding.  Forward gathers embed_tokens rows / image-feature rows into
 * inputs_embeds [B*S, d].  Backward scatters: image rows plain-stored (each used once, untouched rows
 * must be pre-zeroed), token rows added into the fp32 embedding gradient — without atomics: duplicates of a token id
 * are summed in ascending row order by the workgroup of the first occurrence, so the result is bitwise reproducible.
 * dxa_zero_rows zeroes the gradient rows of the token entries of a (previous) plan: the sparse re-zero of the dense
 * nn.Embedding gradient (dexbotic_arch.py:224-228 embeds through nn.Embedding; its .grad is dense). */
int dxa_splice_fwd(const int64_t* plan, const void* embed, const void* img, void* out, int64_t n_rows,
                   int64_t d, int dtype, dxa_stream_t stream);
int dxa_splice_bwd(const int64_t* plan, const void* dout, float* d_embed, void* d_img, int64_t n_rows,
                   int64_t d, int dtype, dxa_stream_t stream);
int dxa_zero_rows(const int64_t* plan, float* g, int64_t n_rows, int64_t d, dxa_stream_t stream);
/* out[i,:] = x[idx[i],:]   (cognition token, cogact_arch.py:110-120) and its scatter-add backward */
int dxa_gather_rows(const void* x, const int64_t* idx, void* out, int64_t n, int64_t d, int src_dtype,
                    int dst_dtype, dxa_stream_t stream);
/* dx [R,d] is written completely: row r = sum_{i: idx[i]==r} dout[i], every other row = 0 */
int dxa_scatter_rows(const void* dout, const int64_t* idx, void* dx, int64_t n, int64_t R, int64_t d,
                     int src_dtype, int dst_dtype, dxa_stream_t stream);

/* Patch embedding front-end (HF:clip/modeling_clip.py:138-218).
 * im2col: images [N,3,H,W] (img_dtype) -> rows [N*g*g, ld] (dtype), column order (c, py, px) = the
 * flattened Conv2d weight [C, 3*P*P]; columns >= 3*P*P are zero.
 * vit_embed: x[n,0,:] = cls + pos[0]; x[n,1+p,:] = patch[n,p,:] + pos[1+p]. */
int dxa_im2col(const void* images, void* rows, int N, int H, int W, int P, int64_t ld, int img_dtype,
               int dtype, dxa_stream_t stream);
int dxa_vit_embed_fwd(const void* patch, const void* cls, const void* pos, void* x, int N, int np, int C,
                      int dtype, int w_dtype, dxa_stream_t stream);
int dxa_vit_embed_bwd(const void* dx, void* dpatch, int N, int np, int C, int dtype, dxa_stream_t stream);

/* Perception Encoder vision tower (dexbotic/model/modules/mm_vision/pe/pe_model.py), the pieces between its GEMMs.
 *
 * 2-D RoPE (Rope2D.forward + apply_rotary_emb + rotate_half, pe_model.py:17-47,114-128): rotates, in place, the q and k thirds of
 * the packed projection qkv [N, T, 3, H, D]; v is not touched.  cos / sin: fp32 tables [T, D] of the token's angles, built on the
 * host for the grid in use (the first D/2 columns turn with the token's column index, the last D/2 with its row index, each
 * frequency twice; the rows picked out of the native grid's table for another grid).  Per interleaved pair
 *   fwd:  y[2i] = x[2i] cos[2i] - x[2i+1] sin[2i],      y[2i+1] = x[2i+1] cos[2i+1] + x[2i] sin[2i+1]
 *   bwd:  dx[2i] = dy[2i] cos[2i] + dy[2i+1] sin[2i+1],  dx[2i+1] = dy[2i+1] cos[2i+1] - dy[2i] sin[2i]   (the transposed rotation)
 * each product rounded to fp32, added, rounded once to `dtype`.  A chunk whose angles are all zero (the CLS row) is not written:
 * it stays bit-identical.  Nothing is saved for the backward.  Refused with DXA_ERR_BAD_ARG: a null pointer, D % 4 != 0, sizes <= 0. */
int dxa_rope2d_fwd(void* qkv, const float* cos_t, const float* sin_t, int64_t N, int T, int H, int D, int dtype, dxa_stream_t stream);
int dxa_rope2d_bwd(void* dqkv, const float* cos_t, const float* sin_t, int64_t N, int T, int H, int D, int dtype, dxa_stream_t stream);
/* LayerScale + residual (ResidualAttentionBlock.forward, pe_model.py:311-312 with LayerScale.forward :138-139):
 *   fwd:  y = x + gamma[c] * h          x, h, y [rows, cols]; gamma [cols], all of `dtype`
 *   bwd:  dh = gamma * dy, and partial [dxa_layerscale_bwd_rows(rows)][cols] fp32: per-column sums of dy * h over disjoint row sets,
 *         each in row order (no atomics; `partial` 16-byte aligned).  Their column sum (dxa_colsum) is dgamma; the gradient of x is
 *         dy itself. */
int dxa_layerscale_residual_fwd(const void* x, const void* h, const void* gamma, void* y, int64_t rows, int64_t cols, int dtype,
                                dxa_stream_t stream);
int dxa_layerscale_residual_bwd(const void* dy, const void* h, const void* gamma, void* dh, float* partial, size_t partial_bytes,
                                int64_t rows, int64_t cols, int dtype, dxa_stream_t stream);
int dxa_layerscale_bwd_rows(int64_t rows);
/* Rows of the 3x3 / stride 2 / pad 1 convolutions vit_downsampler1 / 2 (pe_model.py:445-458,554-565) over a token-major T x T grid:
 *   im2col:  x [B, T*T, C] -> rows [B*To*To, 9*C], To = (T - 1) / 2 + 1, column c*9 + ky*3 + kx = x[b, 2 oy + ky - 1, 2 ox + kx - 1, c]
 *            (zero outside the grid): the flattening of the Conv2d weight [C', C, 3, 3], so the convolution is dxa_gemm (NT) with
 *            the weight as it lies, its bias epilogue, and a token-major result [B, To*To, C'].
 *   col2im:  the adjoint as a gather per input element: dx [B, T*T, C] from drows [B*To*To, 9*C]; every dx element is written. */
int dxa_conv3x3s2_im2col(const void* x, void* rows, int64_t B, int T, int C, int dtype, dxa_stream_t stream);
int dxa_conv3x3s2_col2im(const void* drows, void* dx, int64_t B, int T, int C, int dtype, dxa_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Diffusion action expert glue (fp32).  cogact/action_model/{action_models,dit,diffusion}.py.
 * ---------------------------------------------------------------------------------------------- */
/* x_t = a[n]*x0 + s[n]*noise   (diffusion.py:308-326; a,s gathered from the float64 tables on host) */
int dxa_qsample(const float* x0, const float* noise, const float* a, const float* s, float* xt,
                int64_t N, int64_t per, dxa_stream_t stream);
/* sinusoidal timestep embedding out[n] = [cos(t_n f) | sin(t_n f)], f = freqs[half] built on the host
 * exactly as dit.py:45-49 does (exp(-ln(10000) k/half) in fp32) */
int dxa_timestep_embedding(const float* t, const float* freqs, float* out, int64_t N, int half,
                           dxa_stream_t stream);
/* h[n,0,:] = te[n]+ze[n]+pos[0]; h[n,1+t,:] = xe[n,t]+pos[1+t]  (dit.py:281-286) and its backward */
int dxa_dit_assemble_fwd(const float* xe, const float* te, const float* ze, const float* pos, float* h,
                         int N, int T, int hd, dxa_stream_t stream);
int dxa_dit_assemble_bwd(const float* dh, float* dxe, float* dc, int N, int T, int hd, dxa_stream_t stream);
/* z_out[n] = drop[n] ? uncond : z[n]   (LabelEmbedder.token_drop, dit.py:80-96); bwd masks dz */
int dxa_token_drop(const float* z, const float* uncond, const uint8_t* drop, float* out, int64_t N,
                   int64_t d, dxa_stream_t stream);
/* dz[n] = drop[n] ? 0 : dout[n] (dz may be NULL); duncond[c] (+)= sum over dropped n of dout[n,c] */
int dxa_token_drop_bwd(const float* dout, const uint8_t* drop, float* dz, float* duncond, int64_t N,
                       int64_t d, int accumulate, dxa_stream_t stream);
/* ---- MemVLA memory path, device side (dexbotic/model/memvla/memvla_arch.py) ----------------------------------------
 * out[i] = u_i >= p ? 1/(1-p) : 0, u_i uniform in [0,1) from Philox4x32-10 keyed by `seed`, counter (i / 4, offset): one
 * launch per dropout mask of the retrieval blocks (SDPA's dropout_p on the attention weights, memvla_arch.py:120-123, and
 * the two nn.Dropout of the FFN, :99-105).  Statistically the reference's draw, not bit-for-bit torch's generator. */
int dxa_dropout_mask(void* out, int64_t n, float p, uint64_t seed, uint64_t offset, int dtype, dxa_stream_t stream);
/* token-merge consolidation of ONE memory bank on the device (_consolidate_with_token_merge, memvla_arch.py:263-287):
 * feat [len, N, D] (dtype), ts [len] fp32, len >= 2 entries oldest first.  sims[i] = mean_n cos(feat[i,n,:], feat[i+1,n,:])
 * (eps 1e-8 per norm), j = first arg-max; feat[j] <- 0.5 (feat[j] + feat[j+1]), ts[j] likewise, the later entries move down:
 * afterwards the first len - 1 entries are the bank.  `sims`: len - 1 floats of scratch.  No host read-back. */
int dxa_bank_consolidate(void* feat, float* ts, int len, int64_t N, int64_t D, int dtype, int fifo, float* sims,
                         dxa_stream_t stream);      /* fifo = 1: drop the oldest entry instead (memvla_arch.py:300-303) */
/* 'parallel_stream' (memvla_arch.py:340-361): batch slot b is its own running episode, so the B banks of a role live side by
 * side — feat [B, cap, N, D] (dtype), ts [B, cap] fp32, cap = mem_length + 1 — and every step of the bank is ONE launch over
 * the B slots.  counts [B] int32 (device): the entries each slot held when the step began; a count is clamped to [0, cap]
 * before it indexes anything.  All four refuse null pointers, B / N / D / cap <= 0, cap < 2 and a dtype other than fp32 / bf16.
 *
 * stage_fwd: what the step's retrieval reads, written afresh (the append below overwrites the bank while the backward still
 * needs it): mem [B, cap, N, D], ts_eff [B, cap], kv_len [B].  Slot with history: its counts[b] entries and their timesteps,
 * kv_len = counts[b] N.  Slot without: entry 0 = tokens[b], timestep timesteps[b], kv_len = N (the frame retrieves from itself,
 * :378-387).  Everything behind kv_len is written as zeros.
 * stage_bwd: dtokens[b] = dmem[b, 0] for a slot without history, 0 for the others (history entries are detached copies). */
int dxa_bank_stage_fwd(const void* feat, const float* ts, const int32_t* counts, const void* tokens, const float* timesteps,
                       void* mem, float* ts_eff, int32_t* kv_len, int64_t B, int64_t cap, int64_t N, int64_t D, int dtype,
                       dxa_stream_t stream);
int dxa_bank_stage_bwd(const void* dmem, const int32_t* counts, void* dtokens, int64_t B, int64_t cap, int64_t N, int64_t D,
                       int dtype, dxa_stream_t stream);
/* feat[b, counts[b]] = src[b] ([B, N, D]), ts[b, counts[b]] = timesteps[b]; a slot whose count is already cap is left alone */
int dxa_bank_append(void* feat, float* ts, const int32_t* counts, const void* src, const float* timesteps, int64_t B,
                    int64_t cap, int64_t N, int64_t D, int dtype, dxa_stream_t stream);
/* dxa_bank_consolidate on every slot whose length counts[b] + count_add exceeds mem_length (count_add: entries appended since
 * `counts` was uploaded — 1 after dxa_bank_append), bit-identical per slot; the other slots are not touched.  Two launches:
 * similarities over (pair, slot), merge over (element, slot).  sims: B (cap - 1) floats of scratch (may be NULL with fifo).
 * Also refuses mem_length outside [1, cap). */
int dxa_bank_consolidate_batched(void* feat, float* ts, const int32_t* counts, int count_add, int mem_length, int fifo,
                                 float* sims, int64_t B, int64_t cap, int64_t N, int64_t D, int dtype, dxa_stream_t stream);
/* The same three steps on a chosen subset of the slots, in any order (served episodes tick at different rates, join and
 * leave): feat [S, cap, N, D], ts [S, cap] are the banks of S slots; slot_ids [R] int32 (device), R <= S, DISTINCT (the host
 * that owns the list checks).  Row r of the call reads / writes slot slot_ids[r]; counts [R], tokens / src [R, N, D],
 * timesteps [R], mem [R, cap, N, D], ts_eff [R, cap], kv_len [R] and the scratch sims [R (cap - 1)] are indexed by the row.
 * The device code is the code above (the slot lookup is the only difference): per row bit-identical to the call above on the
 * gathered slots.  Slots not named are not touched.  An id outside [0, S) makes its row a no-op: nothing is appended or
 * merged, and stage_fwd writes the row's outputs as for a slot without history.  Refusals as above, plus R > S and S <= 0. */
int dxa_bank_stage_fwd_at(const void* feat, const float* ts, const int32_t* slot_ids, const int32_t* counts, const void* tokens,
                          const float* timesteps, void* mem, float* ts_eff, int32_t* kv_len, int64_t R, int64_t S, int64_t cap,
                          int64_t N, int64_t D, int dtype, dxa_stream_t stream);
int dxa_bank_append_at(void* feat, float* ts, const int32_t* slot_ids, const int32_t* counts, const void* src,
                       const float* timesteps, int64_t R, int64_t S, int64_t cap, int64_t N, int64_t D, int dtype,
                       dxa_stream_t stream);
int dxa_bank_consolidate_batched_at(void* feat, float* ts, const int32_t* slot_ids, const int32_t* counts, int count_add,
                                    int mem_length, int fifo, float* sims, int64_t R, int64_t S, int64_t cap, int64_t N,
                                    int64_t D, int dtype, dxa_stream_t stream);
/* out[r,n,:] = (x ? x[r,n,:] : 0) + alpha g[r,:]: the timestep embedding added to every token of a bank entry
 * (memvla_arch.py:352-360); x = NULL: broadcast of a row over the tokens (backward of the token mean, :139-141) */
int dxa_add_rows(const void* x, const void* g, void* out, int64_t R, int64_t Nn, int64_t C, float alpha, int dtype,
                 dxa_stream_t stream);
/* out[r,:] = scale * sum_n x[r,n,:] (fp32 accumulation, token order): AdaptiveAvgPool2d(1) of BottleneckSE
 * (memvla_arch.py:139-141) and the gradient of a row broadcast over the tokens */
int dxa_token_sum(const void* x, void* out, int64_t R, int64_t Nn, int64_t C, float scale, int dtype, dxa_stream_t stream);
/* loss = mean((pred-target)^2) (action_models.py:119-121); dpred = 2 (pred-target) / n * gscale */
int dxa_mse_loss(const float* pred, const float* target, float* loss, float* dpred, int64_t n,
                 float gscale, dxa_stream_t stream);
/* sample-weighted variant (HybridCogACT co-training, dexbotic/model/cogact/hybrid_cogact_arch.py:168-173):
 * loss = sum_r w[r] * mean_c((pred-target)[r,c]^2) / (sum_r w[r] + 1e-6); dpred = d loss / d pred * gscale */
int dxa_mse_loss_rows(const float* pred, const float* target, const float* row_w, float* loss, float* dpred,
                      int64_t rows, int64_t cols, float gscale, dxa_stream_t stream);
/* expectile regression of the MuVLA reward head (dexbotic/model/muvla/muvla_arch.py:584-587), one launch:
 * diff = pred - target; w = diff < 0 ? tau : 1 - tau (diff == 0 takes 1 - tau; its gradient is 0);
 * loss = mean(w * diff^2); dpred = 2 * w * diff / n * gscale (NULL to skip).  0 < tau < 1, n > 0. */
int dxa_expectile_loss(const float* pred, const float* target, float* loss, float* dpred, int64_t n, float tau,
                       float gscale, dxa_stream_t stream);
/* One DDIM(eta=0) update with classifier-free guidance (dit.py:294-311, diffusion.py:626-673):
 * eps = eu + s (ec - eu) with ec = model_out[0:B], eu = model_out[B:2B] (cfg) or eps = model_out;
 * x0 = c_recip x - c_recipm1 eps ; eps' = (c_recip x - x0)/c_recipm1 ; x <- sqrt(ab_prev) x0 +
 * sqrt(1-ab_prev) eps'.  x is [B or 2B, per]; with cfg both halves receive the same result. */
int dxa_ddim_step(float* x, const float* model_out, int64_t B, int64_t per, int use_cfg, float cfg_scale,
                  float c_recip, float c_recipm1, float ab_prev, dxa_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizer (trainer.py:25-36,88-124 -> torch.optim.AdamW + clip_grad_norm_(1.0)) over a flat arena.
 * chunk table (device): chunk c covers elements [start[c], start[c]+len[c]) and uses group grp[c].
 * Per group: lr, weight_decay.  clip_coef: device float multiplied into every gradient.
 * shadow (optional): bf16 copy of the updated parameters written in the same pass.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dxa_adamw_desc {
  float* p; const void* g; float* m; float* v;
  uint16_t* shadow;            /* or NULL */
  const int64_t* chunk_start; const int32_t* chunk_len; const int32_t* chunk_grp; int32_t n_chunks;
  float lr[8]; float wd[8];
  float beta1, beta2, eps;
  float bc1, bc2;              /* 1-beta1^t, 1-beta2^t */
  const float* clip_coef;      /* device scalar or NULL (=1) */
  int32_t g_dtype;             /* DXA_F32: g is the fp32 gradient arena; DXA_BF16: g is its bf16 communication copy (the
                                  data-parallel run averages bf16 gradients like the reference's DeepSpeed bf16 config,
                                  script/deepspeed/zero2.json, and the optimizer reads the averaged copy directly) */
  uint8_t* chunk_state;        /* or NULL.  One byte per chunk, device memory, kept by the caller across steps: 0 = ordinary chunk;
                                  1 = chunk of a sparsely touched table (nn.Embedding weight: dexbotic_arch.py:182-373 scatters
                                  gradients into <= B * S_text rows per step) that has never seen a non-zero gradient: its m and v
                                  are exactly 0, so while its gradient is all-zero and its group's weight decay is 0 torch's AdamW
                                  leaves p, m, v bit-for-bit unchanged — the kernel reads g only and returns; the first non-zero
                                  gradient turns the byte into 2 = ordinary from then on */
  const int64_t* chunk_mv_start; /* or NULL (m, v laid out like p: element chunk_start[c] + i).  Sharded optimizer state — the
                                  reference's default DeepSpeed ZeRO config partitions the optimizer state over the data-parallel
                                  ranks (dexbotic/exp/base_exp.py:229, script/deepspeed/zero3.json:17-25): a rank keeps m / v only for
                                  the arena ranges it owns, packed back to back; chunk c's moments then start at element
                                  chunk_mv_start[c] of m and v while p, g and shadow keep the arena offset chunk_start[c] */
} dxa_adamw_desc;
int dxa_adamw(const dxa_adamw_desc* d, dxa_stream_t stream);
/* out[0] = sum x^2 over n fp32 / bf16 elements (deterministic two-stage; scratch >= 4096 doubles) */
int dxa_sumsq(const void* x, int64_t n, int dtype, double* scratch, float* out, int accumulate, dxa_stream_t stream);
/* the same over n_ranges <= 4096 short slices base[starts[i] .. starts[i] + lens[i]) (device arrays, element units): the
 * slots of a gradient bucket that no dW epilogue accounts for (dxa_gemm_desc.sumsq), in one launch */
int dxa_sumsq_ranges(const void* base, int dtype, const int64_t* starts, const int64_t* lens, int n_ranges, double* scratch,
                     float* out, int accumulate, dxa_stream_t stream);
/* out[0] (+)= sum of n floats: one workgroup, fixed order, double accumulation (folds dxa_gemm_desc.sumsq partials) */
int dxa_sum_f32(const float* x, int64_t n, float* out, int accumulate, dxa_stream_t stream);
/* norm = sqrt(sumsq); coef = min(1, max_norm/(norm+1e-6))  (torch.nn.utils.clip_grad_norm_) */
int dxa_clip_coef(const float* sumsq, float max_norm, float* norm_out, float* coef_out, dxa_stream_t stream);
/* the same for an arena that holds gradient / grad_scale (data parallelism with SUM collectives leaves world x the mean,
 * grad_scale = 1 / world; replaces DDP's gradient mean + clip_grad_norm_, dexbotic/exp/trainer.py:110,121-122):
 * norm = grad_scale * sqrt(sumsq); coef = grad_scale * min(1, max_norm/(norm+1e-6)) — dxa_adamw multiplies every
 * gradient by coef, so the update is the mean gradient's */
int dxa_clip_coef_scaled(const float* sumsq, float max_norm, float grad_scale, float* norm_out, float* coef_out,
                         dxa_stream_t stream);
int dxa_scale(float* x, int64_t n, float s, dxa_stream_t stream);
/* x *= s[0] with s a DEVICE scalar (upstream loss gradient; no host sync) */
int dxa_scale_dev(float* x, int64_t n, const float* s, dxa_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * LM head: causal-LM cross-entropy and greedy token choice.
 * dxa_cross_entropy_fwd/bwd: HF ForCausalLMLoss (transformers/loss/loss_utils.py) as called from
 *   dexbotic/model/dexbotic_arch.py:483-488 on logits = lm_head(hidden_states[-1]).  `labels[r]` is the label of
 *   row r AFTER the one-position shift; rows with labels == ignore_index contribute nothing.
 *   fwd: row_loss[r] = logsumexp(logits[r]) - logits[r, label] (fp32 math on fp32 or bf16 logits), lse[r] saved.
 *        loss = sum(row_loss) / #non-ignored rows is taken by the caller (dxa_colsum).
 *        Non-finite logits are torch's (F.cross_entropy, torch.logsumexp): a -inf entry has probability 0 and gradient 0 and
 *        lse runs over the rest; a label on a -inf entry gives row_loss = +inf; a row of nothing but -inf has lse = -inf
 *        (row_loss 0 and dlogits 0 when its label is ignored); a NaN anywhere in a row gives lse = NaN, and row_loss = NaN
 *        unless the label is ignored, for that row only.
 *   bwd: dlogits[r, v] = (exp(logits[r, v] - lse[r]) - [v == label]) * gscale[0] * scale  (gscale: device scalar
 *        = upstream gradient or NULL for 1; scale = 1 / #non-ignored rows).  dlogits may alias logits.
 * dxa_argmax_rows: out[r] = first index of the row maximum — torch.argmax, the greedy choice inside
 *   GenerationMixin.generate(do_sample=False) that DiscreteVLAForCausalLM decodes with
 *   (dexbotic/model/discrete_vla/discrete_vla_arch.py:33-41).  Integer result, must equal the reference's: a NaN counts as the
 *   maximum (the first NaN's index when a row holds one, as torch.argmax and the bin argmax of oft.hip), -0 equals +0, and a row
 *   of nothing but -inf gives 0.
 * ---------------------------------------------------------------------------------------------- */
int dxa_cross_entropy_fwd(const void* logits, int64_t ld, const int64_t* labels, float* row_loss, float* lse,
                          int64_t rows, int64_t V, int64_t ignore_index, int dtype, dxa_stream_t stream);
int dxa_cross_entropy_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* lse,
                          const float* gscale, float scale, void* dlogits, int64_t ldd, int64_t rows, int64_t V,
                          int64_t ignore_index, int dtype, dxa_stream_t stream);
/* dxa_cross_entropy_bwd with one more factor per row (the same kernel):
 *   dlogits[r, v] = (exp(logits[r, v] - lse[r]) - [v == label]) * row_w[r] * gscale[0] * scale
 * row_w: [rows] fp32, device.  Ignored rows are written as zeros; dlogits may alias logits.  With row_w == NULL the result is
 * bit-identical to dxa_cross_entropy_bwd at the same scale. */
int dxa_cross_entropy_rows_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* lse,
                               const float* gscale, float scale, const float* row_w, void* dlogits, int64_t ldd,
                               int64_t rows, int64_t V, int64_t ignore_index, int dtype, dxa_stream_t stream);
/* Per-sample normalised, reward-weighted language loss of MuVLA (dexbotic/model/muvla/muvla_arch.py:566-576) from the row losses
 * of dxa_cross_entropy_fwd over [B, L] rows: n_b = number of non-ignored labels of sample b (ignore_index, or outside [0, V):
 * the forward's own rule), w_b = 1 + sigmoid(reward[b]) (reward: [B] fp32 on the DEVICE, NULL for w_b = 1),
 *   loss      = sum_b w_b * (sum_t row_loss[b, t]) / max(n_b, 1) / B
 *   row_w[b,t] = w_b / (max(n_b, 1) * B)        for every t: the row weights dxa_cross_entropy_rows_bwd takes
 * One launch of one workgroup, samples in order, double accumulation through a fixed tree: the same bits on every run. */
int dxa_ce_sample_reduce(const float* row_loss, const int64_t* labels, const float* reward, float* row_w, float* loss,
                         int64_t B, int64_t L, int64_t V, int64_t ignore_index, dxa_stream_t stream);
int dxa_argmax_rows(const void* x, int64_t ld, int64_t* out, int64_t rows, int64_t cols, int dtype,
                    dxa_stream_t stream);
/* dxa_sample_rows: token[r] = one draw from row r of logits [rows, V] (fp32 or bf16, row stride ld elements, any alignment,
 *   V < 2^31) — the token choice of GenerationMixin.generate(do_sample=True) as DiscreteVLAForCausalLM calls it
 *   (dexbotic/model/discrete_vla/discrete_vla_arch.py:35-41), in HF's order of logits warpers.  x = the row read as fp32:
 *     temperature  z_i = x_i * (1 / temperature)                                       (TemperatureLogitsWarper)
 *     top-k        active when 0 < top_k < V: tau = the top_k-th largest x counted with multiplicity, keep x_i >= tau — ties at
 *                  the threshold are all kept, as TopKLogitsWarper keeps them
 *     top-p        active when top_p < 1: softmax over the entries still kept; entry i stays iff the probability of the kept
 *                  entries with x_j > x_i is < top_p.  Without ties this is TopPLogitsWarper (ascending cumulative sum
 *                  <= 1 - top_p removed, at least one kept).  DEVIATION: entries equal to the boundary entry are all kept; HF
 *                  cuts through a run of equal values wherever its sort put them.
 *     draw         e_i = exp(z_i - max z) over the kept entries, Z = sum e_i; the first index j in ascending order whose running
 *                  sum exceeds u[r] * Z (the last kept index with e > 0 if rounding leaves none); prob[r] = e_j / Z
 *   The largest entry is always kept.  NaN and -inf have probability 0; a row without a finite entry gives token 0 like
 *   dxa_argmax_rows (kept 0, thresh +inf, prob 0).  u: device, [rows], each in [0, 1).  Optional outputs (NULL to skip):
 *   kept[r] = number of kept entries, thresh[r] = the smallest kept logit in input units ({i : x_i >= thresh} is the kept set),
 *   prob[r].  Sums are taken in 2^-40 fixed point (e < 2^-40 counts as 0), so equal inputs and equal u give equal outputs bit for
 *   bit on every run.  No device allocation, no sort.  Refused with DXA_ERR_BAD_ARG: null logits / u / token, ld < V, V <= 0,
 *   rows < 0, temperature <= 0, top_p outside (0, 1], a dtype other than DXA_F32 / DXA_BF16. */
int dxa_sample_rows(const void* logits, int64_t ld, int64_t rows, int64_t V, int dtype, float temperature, int64_t top_k,
                    float top_p, const float* u, int64_t* token, int32_t* kept, float* thresh, float* prob,
                    dxa_stream_t stream);
/* Soft-target cross-entropy (dexbotic/model/navila/loss.py soft_cross_entropy): dxa_cross_entropy_fwd/bwd with Gaussian soft
 * targets for the rows whose label is one of the K `soft_ids` (DEVICE array, int64, distinct, any order, each in [0, V)):
 *   p_k = exp(-(label - soft_ids[k])^2 * inv2s2) / sum_k exp(...)   (inv2s2 = 1 / (2 std^2); fp32 from the integer difference)
 *   fwd: row_loss = lse - sum_k p_k logits[soft_ids[k]];  bwd: dlogits = (softmax - p) * g at the soft ids, softmax * g elsewhere.
 * Every other row, ignored rows included, is treated exactly as by dxa_cross_entropy_fwd/bwd; with K = 0 (soft_ids may be NULL)
 * the results are bit-identical to them.  K <= 64.  soft_ids_host: the same K ids in HOST memory (required when K > 0): the call
 * checks them against V and for duplicates without a device round trip. */
int dxa_soft_cross_entropy_fwd(const void* logits, int64_t ld, const int64_t* labels, float* row_loss, float* lse,
                               int64_t rows, int64_t V, int64_t ignore_index, const int64_t* soft_ids,
                               const int64_t* soft_ids_host, int K, float inv2s2, int dtype, dxa_stream_t stream);
int dxa_soft_cross_entropy_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* lse,
                               const float* gscale, float scale, void* dlogits, int64_t ldd, int64_t rows, int64_t V,
                               int64_t ignore_index, const int64_t* soft_ids, const int64_t* soft_ids_host, int K,
                               float inv2s2, int dtype, dxa_stream_t stream);

/* ---- device-side image preprocessing ------------------------------------------------
 * Replaces, for uint8 RGB frames already on the device, what the reference does per frame on the host with
 * Pillow + the CLIP image processor:
 *   dexbotic/data/dataset/rgb_preprocess.py:13-28   PreprocessRGB.__call__   (training data path)
 *   dexbotic/data/dataset/rgb_preprocess.py:30-44   expand2square
 *   dexbotic/model/dexbotic_arch.py:498-529         process_images           (inference server path)
 * i.e. [expand to square with a constant colour] -> Image.resize(BICUBIC) -> center crop -> x * rescale ->
 * (x - mean) / std -> CHW.  The resize is Pillow's 8-bit two-pass resampler (Pillow 12.2.0
 * src/libImaging/Resample.c; 22-bit fixed-point taps, uint8 image between the passes); the uint8 result
 * (out_u8) is bit-exact with Pillow's, the float result equals the processor's float32 arithmetic.
 *
 * dxa_resample_ksize / dxa_resample_coeffs: HOST functions, the tap tables of one axis (precompute_coeffs +
 *   normalize_coeffs_8bpc): bounds[out_size][2] = (first source index, tap count), kk[out_size][ksize].
 *   The caller copies them to the device once per (in_size, out_size) and passes the device copies below.
 * dxa_image_preprocess: n frames of identical h x w.  `pad` != 0 centres the frame in a max(h,w) square of colour
 *   bg.  res_h x res_w is the size after the resize of that (padded) frame; a pass that does not change the size
 *   has NULL tables (Pillow skips it too).  The crop window [crop_top, +out_h) x [crop_left, +out_w) of the
 *   resized frame is what is produced.  tmp is a uint8 scratch of n * rows * out_w * 3 bytes, where
 *   [row0, row0 + rows) are the (padded) source rows the vertical taps of the cropped output rows touch
 *   (row0 = 0, rows = padded height is always valid).
 * ---------------------------------------------------------------------------------------------- */
#define DXA_FILTER_BICUBIC 3 /* PIL.Image.BICUBIC */
typedef struct dxa_image_desc {
  const void* src;        /* uint8 [n, h, w, 3] RGB */
  int n, h, w;
  int pad;                /* expand2square */
  unsigned char bg[4];    /* r, g, b, unused */
  int res_h, res_w;
  int crop_top, crop_left, out_h, out_w;
  int row0, rows;
  const int32_t *hb, *hk; /* horizontal bounds / taps (device) or NULL */
  int hks;
  const int32_t *vb, *vk; /* vertical */
  int vks;
  void* tmp;              /* uint8 scratch */
  void* out;              /* [n, 3, out_h, out_w] of out_dtype (DXA_F32 or DXA_BF16) */
  int out_dtype;
  void* out_u8;           /* optional uint8 [n, out_h, out_w, 3]: the resized + cropped frame */
  double rescale;         /* 1/255 */
  float mean[3], std[3];
} dxa_image_desc;
int dxa_resample_ksize(int in_size, int out_size);
int dxa_resample_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk);
int dxa_image_preprocess(const dxa_image_desc* d, dxa_stream_t stream);

/* ---- device-side training augmentations ---------------------------------------------------------------------------
 * The reference augments every training frame on the host (dexbotic/data/dataset/augmentations.py, albumentations over
 * cv2); the policies 'v3', 'color', 'color_dm0' and 'identity' are RandomResizedCrop / PadToSquare / Resize / ColorJitter
 * only, and run here on uint8 frames already on the device, before dxa_image_preprocess.  The arithmetic is Pillow's
 * (12.2.0), the package the resampler above is pinned to: crop + Image.resize(BILINEAR) (antialiased when it shrinks,
 * which cv2's INTER_LINEAR is not) and the ImageEnhance / HSV sequence torchvision's PIL backend runs for ColorJitter.
 * The random draws stay on the host; every frame brings its own parameters.
 *
 * dxa_resample_ksize_filter: dxa_resample_ksize for a given filter (DXA_FILTER_BILINEAR has support 1, bicubic 2).
 * dxa_image_crop_resize: n frames of identical h x w; `pad` / bg_rgb (r | g << 8 | b << 16) as dxa_image_preprocess.
 *   boxes[n][4] = (x0, y0, c, table): frame i's square box [x0, x0 + c) x [y0, y0 + c) of the (padded) frame is resized
 *   to S x S with the taps of table `table`: bounds[n_tables][S][2] and taps[n_tables][S][ks] hold dxa_resample_coeffs(c, S,
 *   DXA_FILTER_BILINEAR) of each distinct side, rows padded to the common stride ks; table_sides_host[n_tables] names the
 *   side each table was built for.  boxes is a device array, boxes_host the same values on the host (checked before any
 *   launch).  tmp is a uint8 scratch of n * tmp_rows * S * 3 bytes, tmp_rows >= the largest c.  out: uint8 [n, S, S, 3].
 * dxa_color_jitter: in place on uint8 [n, h, w, 3].  params[n] (device, params_host the same on the host): frames with
 *   apply == 0 are not touched; the others get brightness, contrast, saturation and hue in `order`.  Contrast blends with
 *   int(mean L + 0.5) of the frame as the ops before it left it: pass 1 recomputes those per pixel and adds L up per frame in
 *   sums[n] (uint64 scratch, zeroed here; integer sums do not depend on order), pass 2 applies all four in registers.
 * dxa_color_jitter_pixels_host: HOST function, the same per-pixel code on k loose RGB pixels with a given contrast mean m.
 * dxa_image_affine: bilinear affine warp (the Rotate of 'pi0' and 'dm0'), out of place: uint8 [n, h, w, 3] -> the same shape.
 *   mats[n][6] (device, mats_host the same on the host, checked to be finite before the launch) is frame i's INVERSE
 *   matrix: output pixel (x, y) reads the source at xin = m0 (x + 0.5) + m1 (y + 0.5) + m2, yin = m3 (x + 0.5) + m4 (y + 0.5)
 *   + m5.  The pixel is fill_rgb (r | g << 8 | b << 16) unless 0 <= xin < w and 0 <= yin < h; otherwise the four
 *   neighbours of (xin - 0.5, yin - 0.5), clamped to the frame, are blended in double and the result is truncated: Pillow's
 *   Image.transform(size, AFFINE, m, BILINEAR, fillcolor) bit for bit, and so Image.rotate(angle, BILINEAR).  src and dst
 *   must not overlap; n <= 65535.
 * dxa_image_affine_host: HOST function, the same per-pixel code on host buffers.
 * ---------------------------------------------------------------------------------------------- */
#define DXA_FILTER_BILINEAR 2 /* PIL.Image.BILINEAR */
#define DXA_JITTER_BRIGHTNESS 0
#define DXA_JITTER_CONTRAST 1
#define DXA_JITTER_SATURATION 2
#define DXA_JITTER_HUE 3
typedef struct dxa_jitter_params {
  int32_t apply;
  int32_t order[4];       /* a permutation of DXA_JITTER_* */
  float brightness, contrast, saturation; /* blend factors, >= 0 */
  float hue;              /* shift in turns, |hue| <= 0.5; trunc(hue * 255) levels of the 8-bit H plane */
} dxa_jitter_params;
int dxa_resample_ksize_filter(int in_size, int out_size, int filter);
int dxa_image_crop_resize(const void* src, int n, int h, int w, int pad, uint32_t bg_rgb, const int32_t* boxes,
                          const int32_t* boxes_host, int S, const int32_t* bounds, const int32_t* taps,
                          const int32_t* table_sides_host, int n_tables, int ks, void* tmp, int tmp_rows, void* out,
                          dxa_stream_t stream);
int dxa_color_jitter(void* pixels, int n, int h, int w, const dxa_jitter_params* params,
                     const dxa_jitter_params* params_host, uint64_t* sums, dxa_stream_t stream);
int dxa_color_jitter_pixels_host(void* pixels, int64_t k, const dxa_jitter_params* params, int m);
int dxa_image_affine(const void* src, void* dst, int n, int h, int w, const double* mats, const double* mats_host,
                     uint32_t fill_rgb, dxa_stream_t stream);
int dxa_image_affine_host(const void* src, void* dst, int n, int h, int w, const double* mats, uint32_t fill_rgb);

/* ---- persistent DiT blocks for the action sampler ---------------------------------------------------------------
 * All `depth` DiTBlocks of one denoising call (dexbotic/model/cogact/action_model/dit.py:137-162, walked by DiT.forward
 * :281-293 inside every DDIM step of cogact_arch.py:186-197) in ONE launch: h [N*T1, H] (fp32, in place) goes through
 *   h += proj(attn(qkv(LN(h)))) ; h += fc2(gelu_tanh(fc1(LN(h))))      (LayerNorm without affine, eps; head width 64)
 * `weights` is a DEVICE array of depth*8 fp32 pointers: qkv_w [3H,H], qkv_b, proj_w [H,H], proj_b, fc1_w [I,H], fc1_b,
 * fc2_w [H,I], fc2_b per block.  Limits: N*T1 <= 47 rows, T1 <= 32, H = heads*64 <= 1024, I a multiple of 64 (the CFG
 * batch of one request: 2 x 17 rows); anything else runs block by block on the ordinary kernels.  The workspace holds
 * the qkv / attention / MLP activations and the K-slice partials; the barrier counters live in a library-owned block per
 * (device, stream) that every launch leaves zeroed (first use on a stream allocates it: not under stream capture). */
size_t dxa_dit_blocks_workspace(int M, int H, int I);
int dxa_dit_blocks_fwd(float* h, const float* const* weights, int depth, int N, int T1, int H, int heads, int I, float eps,
                       void* workspace, size_t workspace_bytes, dxa_stream_t stream);
/* The fused launch spins on device-wide barriers and therefore needs all its workgroups resident at once; the spin is
 * bounded (~2 s).  *timed_out = 1 if a launch on this stream gave up since the last call (its output is garbage: re-run
 * the request unfused); the barrier state is re-armed.  Synchronises the stream. */
/* The WHOLE DDIM sampler of a single request in one persistent launch (the loop of GaussianDiffusion.ddim_sample_loop,
 * diffusion.py:714-794, over DiT.forward_with_cfg, dit.py:273-311; eta = 0, epsilon prediction, clip_denoised = False): per step
 * x_embedder + conditioning token + positions, the `depth` DiTBlocks, FinalLayer on the action tokens, classifier-free guidance
 * eps = u + s (c - u) and the DDIM update, `steps` times, device-wide barriers in between (same co-residency contract and
 * watchdog as dxa_dit_blocks_fwd).  x [nb, T1-1, A] fp32 in/out; z_emb [N, H] = z_embedder output (N = 2 nb with guidance:
 * [cond; uncond]); t_emb [steps, H] = t_embedder output per step in execution order; coef [steps][4] = sqrt_recip_alphas_cumprod,
 * sqrt_recipm1_alphas_cumprod, alphas_cumprod_prev, 0 per step in execution order; weights as for dxa_dit_blocks_fwd. */
size_t dxa_dit_sample_workspace(int M, int H, int I);
int dxa_dit_sample_fwd(float* x, const float* z_emb, const float* t_emb, const float* pos, const float* x_w, const float* x_b,
                       const float* final_w, const float* final_b, const float* coef, int steps, int A, int nb, int use_cfg,
                       float cfg_scale, const float* const* weights, int depth, int N, int T1, int H, int heads, int I, float eps,
                       void* workspace, size_t workspace_bytes, dxa_stream_t stream);
int dxa_dit_blocks_status(dxa_stream_t stream, int* timed_out);

/* The same sampler with bf16 MFMA operands, for a model SERVED in bfloat16 — how the reference serves action inference
 * (dexbotic/exp/cogact_exp.py:134-138 loads the whole model, DiT head included, with torch_dtype=torch.bfloat16 and
 * inference_action, cogact_arch.py:149-204, runs it without the training forward's autocast(float32) of :133).  Residual stream,
 * LayerNorm statistics, attention, GELU and accumulation stay fp32; the products read bf16 weights and bf16 copies of their
 * input activations (what every nn.Linear of the reference's bf16 head reads).
 *   dxa_dit_bf16_pack: `weights` as for dxa_dit_blocks_fwd (device array of depth*8 fp32 pointers) -> `packed`, an arena of
 *   dxa_dit_bf16_pack_bytes(depth, H, I) bytes (256-byte aligned) holding, per block, the four matrices rounded to bf16 in the
 *   MFMA operand order ([16 output columns][32 k] tiles of 1 KiB) and sum_k W[n, k] of the two LayerNorm-fed matrices; and `table`,
 *   a DEVICE array of depth*10 pointers (packed qkv_w, qkv_b, packed proj_w, proj_b, packed fc1_w, fc1_b, packed fc2_w, fc2_b,
 *   qkv_wsum, fc1_wsum) that dxa_dit_sample_bf16_fwd takes as `packed_table`.  Re-pack when the fp32 weights change.
 *   dxa_dit_sample_bf16_fwd: arguments, limits (N*T1 <= 48 rows), co-residency contract and watchdog (dxa_dit_blocks_status) as
 *   dxa_dit_sample_fwd; the workspace (dxa_dit_sample_bf16_workspace bytes) must be 256-byte aligned. */
size_t dxa_dit_bf16_pack_bytes(int depth, int H, int I);
int dxa_dit_bf16_pack(const float* const* weights, int depth, int H, int I, void* packed, size_t packed_bytes, const void** table,
                      dxa_stream_t stream);
size_t dxa_dit_sample_bf16_workspace(int M, int H, int I);
int dxa_dit_sample_bf16_fwd(float* x, const float* z_emb, const float* t_emb, const float* pos, const float* x_w, const float* x_b,
                            const float* final_w, const float* final_b, const float* coef, int steps, int A, int nb, int use_cfg,
                            float cfg_scale, const void* const* packed_table, int depth, int N, int T1, int H, int heads, int I,
                            float eps, void* workspace, size_t workspace_bytes, dxa_stream_t stream);

/* The bf16 sampler for MemVLA's DiT with perceptual attention (dexbotic/model/memvla/action_model/dit.py:136-185: every block is
 * x + attn(norm1 x); x + MHA(norm3 x, per, per); x + mlp(norm2 x), and MemVLAForCausalLM.inference_action, memvla_arch.py:666-746,
 * samples with it): three more phases per block in the same persistent launch — the query projection (the q rows of
 * nn.MultiheadAttention's packed in_proj, norm3's affine folded into the packed copy), attention of each (row, head) over the
 * request's P perceptual keys / values, out_proj + residual.
 *   dxa_dit_bf16_pack_per: `weights` = device array of depth*14 fp32 pointers (the 8 of dxa_dit_bf16_pack, then per_attn.in_proj_weight
 *   [3H, H], per_attn.in_proj_bias, per_attn.out_proj.weight, per_attn.out_proj.bias, norm3.weight, norm3.bias); `table` = device array
 *   of depth*16 pointers; arena of dxa_dit_bf16_pack_per_bytes bytes.
 *   dxa_dit_sample_bf16_per_fwd: + `per_kv` [depth][N][P][2][H] fp32, the keys / values of every block projected from the request's
 *   perceptual tokens by rows [H:3H] of in_proj (they do not depend on the DDIM step; the caller computes them once per request),
 *   64 <= P <= 256, P % 64 == 0.  Everything else as dxa_dit_sample_bf16_fwd. */
size_t dxa_dit_bf16_pack_per_bytes(int depth, int H, int I);
int dxa_dit_bf16_pack_per(const float* const* weights, int depth, int H, int I, void* packed, size_t packed_bytes, const void** table,
                          dxa_stream_t stream);
int dxa_dit_sample_bf16_per_fwd(float* x, const float* z_emb, const float* t_emb, const float* pos, const float* x_w, const float* x_b,
                                const float* final_w, const float* final_b, const float* coef, int steps, int A, int nb, int use_cfg,
                                float cfg_scale, const void* const* packed_table, const float* per_kv, int P, int depth, int N, int T1,
                                int H, int heads, int I, float eps, void* workspace, size_t workspace_bytes, dxa_stream_t stream);

/* G requests in ONE launch of the bf16 sampler.  A request GROUP is the rows of one request exactly as dxa_dit_sample_bf16_fwd lays
 * them out (N = nb, or 2 nb with guidance: conditional rows, then unconditional; N*T1 <= 48 PER GROUP); the launch walks the groups
 * inside every phase, between the same device-wide barriers, so G requests cost the barriers and the weight stream of one.  Group g
 * of the result has the bits dxa_dit_sample_bf16_fwd / _per_fwd produces on that group's inputs alone.
 *   x [G][nb, T1-1, A] in/out, z_emb [G][N, H], per_kv [depth][G][N][P][2][H]; t_emb, pos, coef and all weights are shared.
 *   1 <= G <= 16 (DXA_ERR_INVALID_ARG outside; the workspace query then returns 0); the workspace is
 *   dxa_dit_sample_bf16_batched_workspace(G, N*T1, H, I) = G * dxa_dit_sample_bf16_workspace(N*T1, H, I) bytes, 256-byte aligned.
 *   Everything else — limits, co-residency contract, watchdog (dxa_dit_blocks_status) — as dxa_dit_sample_bf16_fwd. */
size_t dxa_dit_sample_bf16_batched_workspace(int G, int M, int H, int I);
int dxa_dit_sample_bf16_batched_fwd(float* x, const float* z_emb, const float* t_emb, const float* pos, const float* x_w,
                                    const float* x_b, const float* final_w, const float* final_b, const float* coef, int steps, int A,
                                    int G, int nb, int use_cfg, float cfg_scale, const void* const* packed_table, int depth, int N,
                                    int T1, int H, int heads, int I, float eps, void* workspace, size_t workspace_bytes,
                                    dxa_stream_t stream);
int dxa_dit_sample_bf16_per_batched_fwd(float* x, const float* z_emb, const float* t_emb, const float* pos, const float* x_w,
                                        const float* x_b, const float* final_w, const float* final_b, const float* coef, int steps,
                                        int A, int G, int nb, int use_cfg, float cfg_scale, const void* const* packed_table,
                                        const float* per_kv, int P, int depth, int N, int T1, int H, int heads, int I, float eps,
                                        void* workspace, size_t workspace_bytes, dxa_stream_t stream);

/* ---- KV-cached decode step in one persistent launch (csrc/decode_fused.hip) -------------------------------------------------
 * ONE new token of ONE sequence through every decoder layer and the final RMSNorm — the use_cache=True single-token pass of HF
 * Qwen2Model that GenerationMixin.generate drives for the discrete-action policies (dexbotic/model/discrete_vla/
 * discrete_vla_arch.py:24-50, dexbotic/model/dexbotic_arch.py:429-496): a grid of co-resident workgroups walks
 * [RMSNorm] qkv + bias | RoPE + cache append + attention | o + residual | [RMSNorm] gate / up + SiLU * up | down + residual
 * per layer with device-wide barriers in between (co-residency contract and watchdog of dxa_dit_blocks_fwd; dxa_decode_status
 * reports a launch that gave up).  bf16 weights, bf16 rounding points of the unfused kernels, fp32 accumulation.  D is 64, 128 or
 * 256; Hq D need not equal d (Qwen3).
 *   layers: DEVICE array of n_layers * 9 pointers — input_layernorm.weight [d], q|k|v weight [(Hq + 2 Hkv) D, d], q|k|v bias
 *           [(Hq + 2 Hkv) D] or NULL for projections without a bias (Qwen3), o_proj.weight [d, Hq D],
 *           post_attention_layernorm.weight [d], gate|up weight [2 F, d], down_proj.weight [d, F] (all bf16, 16-byte aligned),
 *           key cache and value cache of the layer [Hkv, max_len, D] bf16 (post-RoPE keys).
 *   qk_norm: NULL (a zero-initialised descriptor: no q / k norm, Qwen2), or a DEVICE array of n_layers * 2 pointers —
 *           self_attn.q_norm.weight [D] and self_attn.k_norm.weight [D], bf16, 16-byte aligned: HF Qwen3RMSNorm(head_dim) of every q
 *           head and of the new key between the projection and RoPE (eps as the layer norms); the cached key is the normalised,
 *           rotated one.
 *   x_in [d] bf16: embedding of the new token; out [d] bf16: hidden state after the final norm (final_norm_w [d] bf16).
 *   cos_row / sin_row [D / 2] fp32: the rotary table row of the token's position.  slot: cache position the new key / value are
 *   written to; the token attends to the cached positions [kv_lo, slot) and itself.  workspace: dxa_decode_step_workspace bytes,
 *   256-byte aligned. */
typedef struct dxa_decode_desc {
  const void* const* layers;
  const void* x_in; void* out; const void* final_norm_w;
  const float* cos_row; const float* sin_row;
  void* workspace; size_t workspace_bytes;
  int32_t n_layers, d, Hq, Hkv, D, F, slot, kv_lo, max_len;
  float eps;
  const void* const* qk_norm;
} dxa_decode_desc;
size_t dxa_decode_step_workspace(int d, int Hq, int Hkv, int D, int F);
int dxa_decode_step(const dxa_decode_desc* desc, dxa_stream_t stream);
int dxa_decode_status(dxa_stream_t stream, int* timed_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXBOTIC_AMD_H_ */
