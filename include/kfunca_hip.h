/*
 * kfunca_hip.h — the C ABI of the MI355X (gfx950) device layer.
 *
 * This header is the drop-in boundary: everything the reference's host core
 * (src/core) reaches in its device layer (src/device/include/*.h) is reachable here as an
 * `extern "C"` function taking plain pointers, sizes and POD descriptors — no C++ types, no
 * torch types, nothing thrown. Each entry cites the reference interface it replaces.
 *
 * Conventions
 *   - every function returns `int` status: 0 = KF_OK, anything else is an error whose text is
 *     available from kf_last_error() (thread-local). The host core turns a non-zero status into
 *     the reference's `utils::Error` (reference: src/core/utils/exception.h:123-131).
 *   - the device layer owns NO memory: outputs, workspaces and semaphores are allocated by the
 *     caller (the host core's caching allocator) and handed in. This breaks the reference's
 *     L1→L2 link cycle (last paragraph).
 *   - `stream` is a hipStream_t passed as void*; NULL means the device's null stream.
 *   - dtype codes follow the reference's ScalarType order (src/core/include/scalar_type.h:9-27).
 */
#ifndef KFUNCA_HIP_H_
#define KFUNCA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KF_ABI_VERSION 7 /* 7 (no signature changed; later additive: kf_cross_entropy_*, KF_CE_*, kf_adamw_workspace_bytes, kf_adamw_step, kf_adamw_tensor, kf_rope, kf_rope_table, kf_attn_fwd_gqa, kf_attn_bwd_gqa_workspace_bytes, kf_attn_bwd_gqa, kf_glu_fwd, kf_glu_bwd, KF_ACT_*, kf_attn_full_fwd, kf_attn_full_bwd_workspace_bytes, kf_attn_full_bwd, kf_softmax_fwd, kf_softmax_bwd, KF_SOFTMAX, KF_LOG_SOFTMAX, kf_qk_norm_rope_fwd, kf_qk_norm_rope_bwd_workspace_bytes, kf_qk_norm_rope_bwd):kf_attn_* run the matrix-core kernels on ANY sequence lengths with Skv >= Sq (no multiple-of-128 rule), the backward workspace's row-constant arrays pad Sq to 32 and its dS part has a second, half-size layout (the causal half: taken when the workspace does not hold full rows for every pair, or under KF_ATTN_DS_TRI) - a caller must size the workspace with THIS library's query, kf_index_add drops indices outside [-nrows, nrows); 6: + KF_ERR_OOM from kf_malloc, kf_gemm_epilogue.c_f32 / kf_gemm_problem.c_f32 (float output behind 16-bit operands); 2: + kf_reduce_moments*, KF_EW_*_SCALAR, kf_graph_*, kf_attn_*_scaled; 3: + kf_sort*; 4: + kf_knobs_reload, kf_norm_*, kf_index_get, kf_gemm_ex, KF_EPI_*; 5: + kf_gemm_grouped_single_grid, kf_allreduce_sum_multi, kf_profile_samples, kf_attn_bwd accepts any workspace >= the statistics (all additive) */

/* ---- status ------------------------------------------------------------------------------ */
enum {
    KF_OK = 0,
    KF_ERR_HIP = 1,         /* a HIP runtime call or a kernel launch failed                  */
    KF_ERR_INVALID = 2,     /* bad argument (shape/dtype/alignment/null pointer)             */
    KF_ERR_UNSUPPORTED = 3, /* valid request the device layer has no kernel for              */
    KF_ERR_INDEX_RANGE = 4, /* descriptor not 32-bit indexable; caller must split (a6)       */
    KF_ERR_WORKSPACE = 5,   /* workspace missing or too small                                */
    KF_ERR_COMM = 6,        /* RCCL failure                                                  */
    KF_ERR_OOM = 7          /* kf_malloc: the device has no room for this allocation; nothing else is affected (HIP's sticky last-error is cleared), the caller may free and retry */
};

/* ---- dtypes: reference ScalarType order (scalar_type.h:9-27) ------------------------------ */
enum {
    KF_BOOL = 0,
    KF_U8 = 1,
    KF_I8 = 2,
    KF_I16 = 3,
    KF_I32 = 4,
    KF_I64 = 5,
    KF_F16 = 6,
    KF_BF16 = 7,
    KF_F32 = 8,
    KF_F64 = 9,
    KF_DTYPE_COUNT = 10
};

#define KF_MAX_DIMS 12   /* reference MAX_TENSOR_DIMS, tensor.h:7 */
#define KF_MAX_TENSORS 8 /* reference TensorIterator::MAX_TENSORS, tensor_iterator.h:22-24 */

/*
 * The post-build() state of the reference's TensorIterator (tensor_iterator.h:27-47), as a POD.
 * Operands are ordered outputs first, then inputs. Dimension 0 is the fastest-moving one
 * (the iterator reorders dims fastest-first, tensor_iterator.cpp:181-244). Strides are BYTES;
 * a stride of 0 marks a broadcast (input) or reduced (output) dimension.
 */
typedef struct kf_iter_desc {
    int32_t ndim;      /* 1..KF_MAX_DIMS after coalescing                     */
    int32_t ntensors;  /* noutputs + ninputs, <= KF_MAX_TENSORS              */
    int32_t noutputs;
    int32_t reserved;
    int32_t dtype[KF_MAX_TENSORS];
    int64_t shape[KF_MAX_DIMS];
    int64_t stride_bytes[KF_MAX_TENSORS][KF_MAX_DIMS];
    void *data[KF_MAX_TENSORS];
} kf_iter_desc;

/* ---- runtime: replaces memory_engine.h:5-10 and Launcher (launcher_cuda.h:105-354) -------- */
const char *kf_last_error(void);
int kf_abi_version(void);
/* content hash (16 hex digits) of the device sources this library was linked from: kfunca_amd/_build.py stamps it in at link time
 * (no reference counterpart: launcher_cuda.h has no build identity). bench.py prints it as device_lib_sha and refuses to quote
 * profile-derived figures when it differs from the source tree it runs in. */
const char *kf_build_source_sha(void);
int kf_device_count(int *count);
int kf_set_device(int device);              /* dset_device, memory_engine.h:5           */
int kf_get_device(int *device);
int kf_malloc(void **ptr, size_t bytes);    /* dmalloc, memory_engine.h:6               */
int kf_free(void *ptr);                     /* dfree, memory_engine.h:7                 */
int kf_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream); /* :8  (synchronous on return) */
int kf_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream); /* :9  (synchronous on return) */
int kf_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream); /* async on stream           */
int kf_memset_zero(void *ptr, size_t bytes, void *stream);                 /* dmemset_zeros, :10 (async) */
int kf_stream_create(void **stream);        /* Launcher::stream_begin, launcher_cuda.h:113-118 */
int kf_stream_destroy(void *stream);
int kf_stream_sync(void *stream);           /* Launcher::stream_sync, launcher_cuda.h:125-127  */
int kf_stream_wait_event(void *stream, void *event); /* cross-stream ordering without a host sync */
int kf_device_sync(void);
int kf_event_create(void **event);          /* per-launch timing mode, launcher_cuda.h:336-345 */
int kf_event_destroy(void *event);
int kf_event_record(void *event, void *stream);
int kf_event_sync(void *event);
int kf_event_elapsed_ms(void *start, void *stop, float *ms);

/* HIP graphs for launch-bound sequences (no reference counterpart: its Launcher submits kernel by kernel,
 * launcher_cuda.h:330-354). Every compute entry of this library only enqueues work on the stream it is given and owns
 * no memory, so a sequence of calls between begin and end is recorded instead of executed; kf_graph_launch replays it
 * with one submission. `stream` must be a stream from kf_stream_create (not NULL). */
int kf_graph_begin_capture(void *stream);
int kf_graph_end_capture(void *stream, void **graph_exec);
int kf_graph_launch(void *graph_exec, void *stream);
int kf_graph_destroy(void *graph_exec);

/* per-launch timing mode: replaces Launcher::set_profiling_mode + the cudaEvent pair around each
 * submit (launcher_cuda.h:253-255,336-345). While enabled, every kernel launch made through this
 * library is bracketed by a HIP event pair on its own stream (no host sync); kf_profile_get()
 * synchronises and reports, per kernel name, the number of launches and their summed duration. */
int kf_profile_enable(int on);
int kf_profile_reset(void);
int kf_profile_count(int *n);
int kf_profile_get(int i, char name[64], double *total_ms, int64_t *launches);
/* the durations of entry i's individual launches, in launch order (at most the first 65536 are kept): percentiles, run-to-run spread */
int kf_profile_samples(int i, float *ms, int capacity, int *written);

/* A/B switches (KF_* environment variables: kernel-selection knobs for benchmarks and parity tests, the counterpart of
 * the reference's compile-time constants, SURVEY.md section 5 "Config / flags") are read once per process; this re-reads them. */
int kf_knobs_reload(void);

typedef struct kf_device_props {
    char name[256];
    char arch[64];
    int32_t compute_units;
    int32_t wavefront_size;
    int32_t max_threads_per_block;
    int32_t clock_khz;
    int32_t memory_clock_khz;
    int32_t memory_bus_bits;
    int64_t lds_per_block;
    int64_t l2_bytes;
    uint64_t total_mem;
    uint64_t free_mem;
} kf_device_props;
int kf_device_props_get(int device, kf_device_props *out); /* device_info.h:5 (query half) */

/* ---- elementwise loops: replaces binary/unary/nullary_ops_kernel.h ------------------------ */
enum {
    KF_EW_ADD = 0,  /* add_kernel,  binary_ops_kernel.h:5 */
    KF_EW_SUB = 1,  /* sub_kernel,  :6 */
    KF_EW_MUL = 2,  /* mul_kernel,  :7 */
    KF_EW_DIV = 3,  /* div_kernel,  :8 */
    KF_EW_COPY = 4, /* copy_kernel, unary_ops_kernel.h:5 (also dtype convert) */
    KF_EW_FILL = 5, /* fill_kernel, nullary_ops_kernel.h:5 */
    /* out = in (op) scalar: what `tensor + 2.0` computes in the reference through a filled temporary
     * (register.cpp:172-206: empty_like(self).fill_(s), then the binary kernel) without the temporary */
    KF_EW_ADD_SCALAR = 6,
    KF_EW_SUB_SCALAR = 7,
    KF_EW_MUL_SCALAR = 8,
    KF_EW_DIV_SCALAR = 9
};
/*
 * out = f(in...) over the iteration space of `desc` (1 output; 2 inputs for ADD..DIV, 1 for
 * COPY and the *_SCALAR ops, 0 for FILL). *_SCALAR: input and output share one dtype (f32, f64, bf16,
 * f16, i32, i64); `scalar` is first rounded to that dtype exactly as FILL would, then the op runs in
 * its accumulate type — bit-identical to the reference's fill-then-op sequence. `compute_dtype` is the reference's iter.common_dtype() for ADD..DIV
 * (binary_ops_kernel.cu:34-60; arithmetic runs in its accumulate type: float for half/bf16,
 * int64 for ints, accumulate_type.h:17-27), ignored for COPY (value is cast to the output dtype,
 * unary_ops_kernel.cu:13-17) and FILL (`scalar` cast to the output's accumulate type then to the
 * output dtype, nullary_ops_kernel.cu:20-25).
 * Contiguous descriptors of any size are accepted; strided ones must be 32-bit indexable
 * (KF_ERR_INDEX_RANGE otherwise — the host splits, tensor_iterator.cpp:415-480).
 */
int kf_elementwise(int op, const kf_iter_desc *desc, int compute_dtype, double scalar, void *stream);

/* ---- reductions: replaces reduce_ops_kernel.h:5-6 ------------------------------------------ */
enum {
    KF_RED_SUM = 0, /* sum_kernel  */
    KF_RED_MEAN = 1 /* mean_kernel */
};
/*
 * desc: 1 output, 1 input, built by the reference's build_for_reduce (tensor_iterator.cpp:523-528):
 * reduced dims are the ones where the OUTPUT stride is 0 and shape > 1.
 * The caller supplies scratch of at least kf_reduce_workspace_bytes(desc) bytes (may be 0);
 * it needs no initialisation.
 * A descriptor with a dim of extent 0 writes nothing, even where the output has elements (a reduced
 * dim of extent 0): the caller owns the identity (the operator API writes sum 0, floating mean NaN).
 * The same holds for kf_reduce_moments (the operator API writes NaN to both outputs).
 */
int kf_reduce_workspace_bytes(const kf_iter_desc *desc, size_t *bytes);
int kf_reduce(int op, const kf_iter_desc *desc, void *workspace, size_t workspace_bytes, void *stream);

/* ---- moments: replaces mean_var_kernel (reduce_ops_kernel.h:7, reduce_ops_kernel.cu:61-153) and
 *      norm_stat_kernel (norm_ops_kernel.h, norm_ops_kernel.cu:6-61) ------------------------------------ */
enum {
    KF_MOM_VAR = 0,   /* out0 = M2 / max(n - correction, 0)            (mean_var, take_sqrt = false) */
    KF_MOM_STD = 1,   /* out0 = sqrt(M2 / max(n - correction, 0))      (mean_var, take_sqrt = true)  */
    KF_MOM_INVSTD = 2 /* out0 = 1 / sqrt(M2 / n + eps)                 (norm_stat, welford_norm.h:183) */
};
/*
 * desc: 2 outputs + 1 input in the reference iterator's order (reduce_ops.cpp:24-25): [0] = the variance-like
 * output, [1] = the mean, [2] = the input; both outputs reduce the same dims (stride 0 there).
 * Floating dtypes only; the outputs have the input's dtype, or f32 for f16 / bf16 inputs.
 * Scratch as for kf_reduce (query kf_reduce_moments_workspace_bytes).
 */
int kf_reduce_moments_workspace_bytes(const kf_iter_desc *desc, size_t *bytes);
int kf_reduce_moments(int mode, const kf_iter_desc *desc, double correction, double eps, void *workspace,
                      size_t workspace_bytes, void *stream);

/* ---- row normalisations: finishes the reference's roadmap item rms_norm (README.md:28) on its building block norm_stat
 *      (norm_ops_kernel.h:5, norm_ops_kernel.cu:6-61; invstd = 1 / sqrt(M2 / n + eps), welford_norm.h:170-187) -------------- */
enum {
    KF_NORM_RMS = 0,  /* y = x * rstd * w,                 rstd = 1 / sqrt(mean(x^2) + eps)            */
    KF_NORM_LAYER = 1 /* y = (x - mean) * rstd * w + b,    rstd = 1 / sqrt(mean((x - mean)^2) + eps)   */
};
/*
 * x, y, dy, dx: [rows, cols] with row stride `ld` elements (ld >= cols); weight, bias, dweight, dbias: [cols] (any may be
 * NULL: w = 1, b = 0; RMS takes no bias); dtype in {KF_F32, KF_BF16, KF_F16} for all of them; statistics in f32:
 * mean[rows] (LAYER only), rstd[rows] - the forward writes them (NULL: not kept), the backward reads them.
 * Backward: dx = rstd * (g - mean(g) - xhat * mean(g * xhat)) with g = dy * w, xhat = (x - mean) * rstd (RMS: no mean(g)
 * term, mean = 0); dweight = sum_rows dy * xhat, dbias = sum_rows dy - summed in a fixed order through caller scratch of
 * kf_norm_bwd_workspace_bytes() bytes (no atomics: bitwise reproducible; the scratch needs no initialisation).
 */
int kf_norm_fwd(int kind, int dtype, int64_t rows, int64_t cols, int64_t ld, const void *x, const void *weight, const void *bias,
                double eps, void *y, float *mean, float *rstd, void *stream);
int kf_norm_bwd_workspace_bytes(int kind, int dtype, int64_t rows, int64_t cols, int64_t ld, size_t *bytes);
int kf_norm_bwd(int kind, int dtype, int64_t rows, int64_t cols, int64_t ld, const void *x, const void *weight, const float *mean,
                const float *rstd, const void *dy, void *dx, void *dweight, void *dbias, void *workspace, size_t workspace_bytes,
                void *stream);

/* ---- softmax cross-entropy over the last dimension (no reference counterpart: the loss that ends a language model's chain) --- */
enum {
    KF_CE_NONE = 0, /* loss[r] per row                                   */
    KF_CE_SUM = 1,  /* loss[0] = sum of the rows' losses                 */
    KF_CE_MEAN = 2  /* loss[0] = that sum / the number of rows not ignored */
};
/*
 * logits: [rows, V] with row stride `ld` elements (ld >= V), dtype in {KF_F32, KF_BF16, KF_F16}, aligned to its element size; target:
 * int64 [rows] on the device. torch's F.cross_entropy, with the class axis LAST (torch takes dim 1 of an N-d input):
 *     lse_r  = log(sum_v exp(x_rv))
 *     loss_r = (1 - eps) (lse_r - x_r,t) + eps (lse_r - mean_v x_rv)             eps = label_smoothing in [0, 1], t = target[r]
 *     dx_rv  = g_r (exp(x_rv - lse_r) - (1 - eps) [v == t] - eps / V)
 * A row whose target is ignore_index has loss 0 and a zero gradient row and does not count toward the mean (every row ignored: the
 * mean is NaN, as torch's). A target outside [0, V) that is not ignore_index gives that row a NaN loss and a NaN gradient row and
 * disturbs no other row - unlike torch, which asserts on the device; nothing here reads out of bounds or synchronises to check.
 * -inf logits (a masked vocabulary padding) are fine.
 * Forward: loss is f32 [rows] for KF_CE_NONE, [1] otherwise; lse [rows] f32 (NULL: not kept; the backward needs it) is written for
 * every row; count [1] f32 (NULL: not kept; the mean's backward needs it) receives the number of rows not ignored. The sums run in a
 * fixed order through caller scratch of kf_cross_entropy_workspace_bytes() bytes (no initialisation, no atomics: bitwise
 * reproducible). How a row is cut depends on (rows, V) only: V <= 4096 one wave per row; else rows >= 1024 one block per row; else
 * each row splits into chunks whose partial (max, sum of exponentials, sum x) go to the scratch and are merged in chunk order.
 * Backward: dlogits [rows, V] in the logits' dtype with row stride ldd; grad is f32 [rows] for KF_CE_NONE, a device scalar [1]
 * otherwise; the mean's divisor is read from count on the device. Neither entry synchronises or allocates: both can be captured
 * with kf_graph_*. Every argument is checked before any device call: KF_ERR_INVALID (null pointers, V < 1, ld < V, dtype, reduction,
 * label_smoothing, a workspace that is too small).
 */
int kf_cross_entropy_workspace_bytes(int dtype, int64_t rows, int64_t V, int reduction, size_t *bytes);
int kf_cross_entropy_fwd(int dtype, int64_t rows, int64_t V, int64_t ld, const void *logits, const int64_t *target, int64_t ignore_index,
                         float label_smoothing, int reduction, float *loss, float *lse, float *count, void *workspace,
                         size_t workspace_bytes, void *stream);
int kf_cross_entropy_bwd(int dtype, int64_t rows, int64_t V, int64_t ld, const void *logits, const int64_t *target, int64_t ignore_index,
                         float label_smoothing, int reduction, const float *lse, const float *count, const float *grad, void *dlogits,
                         int64_t ldd, void *stream);

/* ---- cross-entropy of a block of logits WITH its gradient (no reference counterpart: the row kernel of a chunked linear + loss) --- */
/*
 * kf_ce_fused_rows: one call turns a block of logits into its per-row loss and its gradient, so that a caller walking the tokens in
 * chunks (kfunca.linear_cross_entropy) never holds more than one chunk of logits.
 * logits: [rows, V] with row stride `ld` elements (ld >= V), in_dtype in {KF_F32, KF_BF16, KF_F16}; dlogits: [rows, V] with row stride
 * ldd in out_dtype. Pairs: KF_F32 -> KF_BF16 / KF_F16 / KF_F32 (the f32 accumulators of a c_f32 GEMM -> the operands' dtype is the hot
 * one) and a 16-bit type to itself. dlogits == logits (in place) is allowed when the dtypes and the strides are equal; any other overlap
 * is refused. dlogits NULL: the loss only, in one pass over the logits. target: int64 [rows] on the device. Per row, with
 * p = softmax(x), t = target[r], eps = label_smoothing in [0, 1], z = z_loss >= 0:
 *     lse_r      = log(sum_v exp(x_rv))
 *     rowloss_r  = (1 - eps) (lse_r - x_r,t) + eps (lse_r - mean_v x_rv) + z lse_r^2
 *     dlogits_rv = p_rv (1 + 2 z lse_r) - (1 - eps) [v == t] - eps / V
 * The gradient is UNSCALED (values in about [-1, 1]): no 1 / count and no upstream gradient is folded in, so f16 never sees a subnormal
 * gradient and the kernel needs no count beforehand; kf_scale_cast applies both later, to the far smaller dX and dW.
 * rowloss [rows] f32 is required; lse [rows] f32 may be NULL. A row whose target is ignore_index has loss 0 and a zero gradient row
 * whatever its logits hold; a target outside [0, V) that is not ignore_index gives that row a NaN loss and a NaN gradient row and
 * disturbs no other row. -inf logits are fine. The logits are read twice (state, then write), dlogits is written once, in 16-byte packs
 * where the two rows' alignment allows (element by element otherwise); bytes past V in a strided row stay untouched.
 * Regimes from (rows, V) only: V <= 4096 one wave per row; else rows >= 1024 one block per row (both ONE launch); else each row splits
 * into chunks whose partial states go to the workspace of kf_ce_fused_rows_workspace_bytes() bytes (0 in the first two regimes; no
 * initialisation needed) and are merged in chunk order. No atomics: the same call gives the same bits.
 *
 * kf_ce_fused_reduce: loss[0] = the f32 sum of rowloss[0..rows) in a fixed order (mean != 0: divided by the number of rows whose target
 * is not ignore_index - NaN when every row is ignored, as torch's mean); count [1] f32 (may be NULL) receives that number. One launch
 * over ALL rows of a chunked loss, after its last chunk.
 *
 * kf_scale_cast: out[i] = (out_dtype)(in[i] * s), s = g[0] / count[0] (count NULL: s = g[0]) formed once in f32; g and count are device
 * f32 scalars, so an upstream gradient and a mean's divisor are applied without a host read. The same dtype pairs; in place (out == in)
 * when the dtypes are equal, any other overlap is refused. n up to 2^38.
 *
 * None of the three synchronises or allocates: all can be captured with kf_graph_*. rows == 0 / n == 0 is KF_OK without a launch.
 * Every argument is checked before any device call: KF_ERR_INVALID (null pointers, V < 1, ld < V, ldd < V, a dtype pair outside the
 * list, label_smoothing outside [0, 1], a negative or non-finite z_loss, misaligned pointers, an overlap that is not in place, a
 * workspace that is too small).
 */
int kf_ce_fused_rows_workspace_bytes(int64_t rows, int64_t V, size_t *bytes);
int kf_ce_fused_rows(int in_dtype, int out_dtype, int64_t rows, int64_t V, int64_t ld, const void *logits, const int64_t *target,
                     int64_t ignore_index, float label_smoothing, float z_loss, float *rowloss, float *lse, void *dlogits, int64_t ldd,
                     void *workspace, size_t workspace_bytes, void *stream);
int kf_ce_fused_reduce(const float *rowloss, const int64_t *target, int64_t rows, int64_t ignore_index, int mean, float *loss, float *count,
                       void *stream);
int kf_scale_cast(int in_dtype, int out_dtype, int64_t n, const void *in, void *out, const float *g, const float *count, void *stream);

/* ---- fused AdamW step over a list of tensors (no reference counterpart: the optimizer that applies a gradient to a weight) --- */
typedef struct kf_adamw_tensor {
    int64_t numel;         /* elements of param, grad, master, exp_avg and exp_avg_sq (all contiguous, any size, 0 included) */
    int param_dtype;       /* KF_F32, KF_BF16 or KF_F16 */
    int grad_dtype;        /* KF_F32 or param_dtype */
    void *param;
    const void *grad;
    float *master;         /* NULL, or the f32 copy of a 16-bit param: the update runs on it and param is rewritten from it (RNE) */
    float *exp_avg;        /* f32 state */
    float *exp_avg_sq;     /* f32 state */
    float *step;           /* f32 [1] on the device: this tensor's step count, advanced by one per call on the device */
    float weight_decay;    /* >= 0, decoupled (AdamW) */
} kf_adamw_tensor;
/*
 * torch.optim.AdamW (no amsgrad, no maximize) over n tensors in one call, with torch.nn.utils.clip_grad_norm_ when max_grad_norm > 0.
 * Per element, in f32, with g = grad * grad_scale * clip_coef and s = the tensor's step count after it advances:
 *     p = p (1 - lr wd);  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p = p - (lr / (1 - b1^s)) m / (sqrt(v) / sqrt(1 - b2^s) + eps)
 * lr is a device f32 [1] (a schedule may rewrite it between graph replays). Every step count advances by exactly one, on the device.
 * Clipping: norm = sqrt(sum of (grad * grad_scale)^2 over every tensor), clip_coef = min(1, max_grad_norm / (norm + 1e-6)); per-block
 * partial sums go to the caller's workspace and are folded in a fixed order (no atomics), so the call is bitwise reproducible.
 * The grads are NOT rewritten (torch's clip_grad_norm_ scales them in place). A NaN norm makes every param NaN and an infinite one
 * makes clip_coef 0, as torch with error_if_nonfinite=False. grad_norm (f32 [1], optional, clipping only) receives the norm before
 * clipping; max_grad_norm = INFINITY computes it without clipping.
 * Launches: 2 ceil(n / 48) without clipping, 2 ceil(n / 48) + 1 with (48 tensors' pointers travel in each launch's arguments).
 * Pointers need only be aligned to their element size. The workspace (clipping only) is
 *     kf_adamw_workspace_bytes = max_grad_norm > 0 ? 256 + 8192 ceil(n / 48) : 0 bytes.
 * Neither entry synchronises or allocates: the step can be captured with kf_graph_*. Every argument is checked before any device
 * call: KF_ERR_INVALID (null pointers, dtypes, negative numel, beta outside [0, 1), eps or weight_decay < 0, a master for an f32
 * param, a workspace that is too small).
 */
int kf_adamw_workspace_bytes(int64_t n, float max_grad_norm, size_t *bytes);
int kf_adamw_step(const kf_adamw_tensor *tensors, int64_t n, double beta1, double beta2, double eps, const float *lr, float grad_scale,
                  float max_grad_norm, float *grad_norm, void *workspace, size_t workspace_bytes, void *stream);

/* ---- index_put_: replaces index_ops_kernel.h:5 --------------------------------------------- */
/*
 * desc operands: [0] = self viewed with stride 0 (index_ops.cpp:23-25), [1] = values,
 * [2..2+nidx) = int64 index tensors. For each element n of the iteration space:
 *   self_bytes[ sum_i wrap(idx_i[n], sizes[i]) * strides_bytes[i] ] = values[n]
 * Negative indices wrap once; no bounds check; duplicates: last writer wins, unspecified order
 * (tensor_index.h:56-75).
 */
int kf_index_put(const kf_iter_desc *desc, int nidx, const int64_t *sizes, const int64_t *strides_bytes,
                 void *stream);

/* ---- row gather: the reference's roadmap item "embedding" (README.md:30), on the index arithmetic of tensor_index.h:56-104 ---- */
/*
 * out[n, :] = table[wrap(idx[n]), :] for n < n: rows of row_bytes bytes, moved as bytes (bit-exact for every dtype); negative
 * indices wrap once, no bounds check (as the reference's index kernels, tensor_index.h:56-75). idx is int64, on the device.
 */
int kf_index_get(const void *table, int64_t nrows, int64_t row_bytes, const int64_t *idx, int64_t n, void *out, void *stream);
/*
 * The gather's backward without atomics: dst[r, :] = sum over {n : wrap(idx[n]) == r} of src[n, :], added in input order in f32
 * (the indices are wrapped, stably sorted with kf_sort, and each run of equal rows is summed by one wave: bitwise
 * reproducible). Rows no index names are left untouched (zero dst first). An index outside [-nrows, nrows) names no row and its
 * src row is DROPPED (no out-of-bounds write, no error: the call never synchronises). dtype in {KF_F32, KF_BF16, KF_F16}; src [n, cols],
 * dst [nrows, cols] contiguous; caller scratch of kf_index_add_workspace_bytes(n) bytes, no initialisation needed.
 */
size_t kf_index_add_workspace_bytes(int64_t n);
int kf_index_add(int dtype, const int64_t *idx, int64_t n, const void *src, int64_t cols, int64_t nrows, void *dst, void *workspace,
                 size_t workspace_bytes, void *stream);

/* ---- sort: replaces sort_ops_kernel.h (segmented_sort_pairs, sort_ops_kernel.cu:402-505) ----- */
/*
 * Stable sort of nseg contiguous segments of n keys each (what sort_stable_kernel, sort_ops_kernel.cu:556-618, hands to
 * segmented_sort_pairs<scalar_t, int64_t>(keys_in, keys_out, nullptr, values_out, nsegments, nsort, descending)):
 * keys_out[s][j] = the j-th key of segment s in ascending (descending != 0: descending) order, pos_out[s][j] = its
 * int64 position inside the input segment; equal keys keep their input order in both directions. Order is that of the
 * reference's key transforms (sorting_common.h:23-260): integers by value; floats by value with -0.0 before +0.0 and
 * NaNs by bit pattern (positive NaNs last, negative NaNs first, ascending). Every dtype except KF_BOOL; n <= INT_MAX.
 * keys_in and keys_out must be different buffers. Segments of at most 8192 keys are sorted in LDS and need no
 * workspace; longer ones take kf_sort_workspace_bytes() of caller scratch (16-byte aligned, need not be zeroed).
 */
size_t kf_sort_workspace_bytes(int dtype, int64_t nseg, int64_t n);
int kf_sort(int dtype, const void *keys_in, void *keys_out, int64_t *pos_out, int64_t nseg, int64_t n, int descending,
            void *workspace, size_t workspace_bytes, void *stream);

/* ---- GEMM: replaces gemm_kernel.h:5 (+ NT/TN forms the backward needs) --------------------- */
enum {
    KF_EPI_NONE = 0,
    KF_EPI_BIAS_ROW = 1 /* C[m,n] += bias[n] after alpha/beta (fused broadcast add, config C4) */
};
/*
 * C[M,N] = alpha * op(A)[M,K] * op(B)[K,N] + beta * C, row-major, leading dims in ELEMENTS.
 *   trans_a == 0: A is stored [M,K] (lda >= K);  trans_a == 1: A is stored [K,M] (lda >= M)
 *   trans_b == 0: B is stored [K,N] (ldb >= N);  trans_b == 1: B is stored [N,K] (ldb >= K)
 * dtype in {KF_F32, KF_F64, KF_F16, KF_BF16}; A, B, C share it; accumulation is f32 (f64 for f64).
 * beta == 0 never reads C (the reference reads uninitialised memory there, gemm_ops.cpp:10-16).
 * Every kernel reads every operand layout in place, so no GEMM NEEDS scratch. kf_gemm_workspace_bytes() is non-zero only for
 * skinny 16-bit products (at most 128 output tiles of 128 x 128, at least 16 K tiles of 64): given that much 16-byte aligned
 * scratch, kf_gemm splits the contraction into 2..16 slices whose f32 partial tiles a second kernel adds in slice order
 * (deterministic; M 256, N 4096, K 16384: 169 -> 49 us); with NULL / 0 the same call runs unsplit. KF_GEMM_NO_SPLITK disables it.
 * Ragged extents (round 5): a 16-bit or f32 product of at least 2^24 multiply-adds whose M / N / K are not whole tiles (128 x 128 x 64,
 * f32 64 x 64 x 16) also reports scratch: given it, kf_gemm copies the ragged operands into zero-padded images of whole tiles, runs the
 * tile kernels on those and copies the valid part of C back (bf16 4000^3: 5.0 -> 0.11 ms; 16 x 8192 x 8192: 0.70 -> 0.05 ms); without it
 * (or with KF_GEMM_NO_PAD, which also makes the query return 0) the scalar kernel runs as before. Bytes of C outside [M, N] stay untouched.
 * The scratch is three padded images (+ split-K partials): ~2 (Mp Kp + Kp Np + Mp Np) bytes in 16 bits - gigabytes for vocabulary-sized
 * products; a workspace that is too small or not 16-byte aligned is not an error: the scalar kernel runs and the library says so once on stderr.
 */
int kf_gemm_workspace_bytes(int dtype, int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, size_t *bytes);
int kf_gemm(int dtype, int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, float alpha, const void *A,
            int64_t lda, const void *B, int64_t ldb, float beta, void *C, int64_t ldc, int epilogue,
            const void *bias, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same product with an element-wise tail fused into the store (the reference's roadmap: fused projections, README.md:32; its
 * own API can only express these as separate add / mul kernels over the GEMM's output, binary_ops.cpp:6-91):
 *     t = alpha * op(A) op(B) + beta * C + bias[n]        (bias NULL: none)
 *     aux[m,n] = t                                        (aux NULL: not kept; the backward of a gating product needs it)
 *     C[m,n]  = t * mul[m,n] + add[m,n]                   (mul NULL: 1; add NULL: 0)
 * mul, add, aux: [M,N] row-major of the GEMM's dtype with their own leading dimensions. A residual connection is add = the
 * residual stream; a gated MLP's h = (x Wg) o (x Wu) is mul = x Wu with aux = x Wg. Every kernel applies the tail.
 */
typedef struct kf_gemm_epilogue {
    const void *bias; /* [N] or NULL */
    const void *mul;  /* [M,N] or NULL */
    int64_t ldmul;
    const void *add;  /* [M,N] or NULL */
    int64_t ldadd;
    void *aux;        /* [M,N] or NULL */
    int64_t ldaux;
    int32_t c_f32;    /* ABI 6, 16-bit dtypes only: C (and beta C) is FLOAT [M, ldc floats per row]; the f32 accumulators leave unrounded -
                         a weight gradient summed over ranks or micro-batches (beta = 1) loses nothing to the 16-bit format. bias / mul / add /
                         aux stay 16-bit. 0: C has the operands' dtype. */
} kf_gemm_epilogue;
int kf_gemm_ex(int dtype, int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, float alpha, const void *A, int64_t lda,
               const void *B, int64_t ldb, float beta, void *C, int64_t ldc, const kf_gemm_epilogue *epi, void *stream);

/*
 * Several independent products in one call (no element-wise tail). The backward pair of a linear layer - p[0] = dA = dC B^T
 * (trans_a 0, trans_b 1), p[1] = dB = A^T dC (trans_a 1, trans_b 0) - in 16 bits on shapes of the 4-wave 256-tile kernel
 * (M, N multiples of 256, K of 64, at most 512 tiles each, tile counts multiples of 8) runs as ONE grid: the second product's
 * first tiles start under the first one's last tiles instead of behind a kernel boundary. Anything else is the same as calling
 * kf_gemm once per problem, in order. KF_GEMM_NO_GROUP disables the single-grid form.
 */
typedef struct kf_gemm_problem {
    int32_t trans_a, trans_b;
    int64_t M, N, K;
    float alpha, beta;
    const void *A;
    int64_t lda;
    const void *B;
    int64_t ldb;
    void *C;
    int64_t ldc;
    int32_t c_f32;    /* ABI 6: this product's C is float (see kf_gemm_epilogue.c_f32) */
} kf_gemm_problem;
int kf_gemm_grouped(int dtype, int count, const kf_gemm_problem *problems, void *stream);
/* 1 when kf_gemm_grouped would run these problems as ONE grid (the backward pair of a 16-bit linear layer on 256-tile shapes with
 * few enough tiles), 0 when it would fall back to one kf_gemm per problem WITHOUT a workspace - a caller that owns split-K scratch
 * (kf_gemm_workspace_bytes) should then issue the kf_gemm calls itself so that skinny products are still split. */
int kf_gemm_grouped_single_grid(int dtype, int count, const kf_gemm_problem *p);

/* ---- causal attention: replaces causal_attention_kernel.h:5 (+ backward) ------------------- */
/*
 * q:[B,H,Sq,D], k,v:[B,H,Skv,D], o:[B,H,Sq,D] contiguous; lse:[B,H,Sq] float32 (may be NULL for
 * inference): lse = m + log(l), the natural-log-sum-exp of the scaled, masked scores.
 * O = softmax(mask(Q K^T / sqrt(D))) V, mask keeps key n for query m iff m >= n (absolute
 * indices, top-left aligned: causal_attention_ref.h:36-41).
 * dtype in {KF_F32, KF_BF16, KF_F16}, D <= 256, any Sq / Skv. Which kernels run, and what that costs (bf16, B 8 H 32 D 128 on MI355X; profiles/r06_attn_ragged.txt):
 *   tier 1  16-bit tensors, D = 64 or 128, Skv >= Sq, ANY lengths (round 6): the generated one-wave-per-SIMD streams (forward 256 queries per
 *           block, dK/dV 256 keys per block) + the stored-dS dQ kernel. Rows beyond a tensor's end are zero-filled / dropped by the kernels'
 *           buffer descriptors: no padded copies, no alignment of S to anything. S = 4096: fwd 1.06, dK/dV 1.83, dQ 0.88 ms;
 *           S = 4000: the same per token (1.004 x); S = 4095 / 3969: 1.007 x. The backward needs workspace for at least one pair's dS here.
 *   tier 2  16-bit, D = 64 or 128, Sq and Skv multiples of 128, Skv < Sq (or KF_ATTN_FWD_V3 / KF_ATTN_DKV_V4): the 8-wave forward
 *           and the 32-key-per-wave dK/dV hand kernels: 1.25 x / 1.22 x tier 1's time at the same shape.
 *   tier 3  f32 tensors (the reference's dtype), D = 64 or 128, Sq and Skv multiples of 32: exact-f32 MFMA (C3 in f32: forward 8.8 ms).
 *   tier 4  everything else (D <= 256 off 64 / 128, 16-bit Skv < Sq off the 128-row tiles, f32 off 32 rows): generic vector-ALU kernels,
 *           correct, 20-100x slower. kfunca_amd's causal_attention zero-pads the head size (and f32 row counts) on its side to stay above this tier.
 * The *_scaled forms take the softmax scale explicitly instead of 1 / sqrt(D): a host that zero-pads a smaller head
 * size up to 64 or 128 columns (zero columns change neither Q K^T nor P V) passes 1 / sqrt(its own D) and lands on the MFMA
 * kernels - kfunca_amd's causal_attention does exactly that.
 */
int kf_attn_fwd(int dtype, int64_t B, int64_t H, int64_t Sq, int64_t Skv, int64_t D, const void *q,
                const void *k, const void *v, void *o, float *lse, void *stream);
int kf_attn_fwd_scaled(int dtype, int64_t B, int64_t H, int64_t Sq, int64_t Skv, int64_t D, float scale, const void *q,
                       const void *k, const void *v, void *o, float *lse, void *stream);
/*
 * dq,dk,dv from d_o. Needs o and lse from the forward. The workspace holds three f32 rows of statistics (delta[B,H,Sq] and the two
 * row-constant arrays the dK/dV kernel reads, the latter two with Sq rounded up to 32 rows per pair: B*H*(Sq + 2 ceil32(Sq))*4 bytes, each
 * array rounded up to 256 - the MINIMUM, O(B H S)) and, on the
 * matrix-core path for 16-bit tensors, whatever lies beyond them holds dS = P o (dP - delta) in 16 bits, one 128-KiB square per (256-query
 * block, 256-key block): the dK/dV kernel writes it, the dQ kernel computes dQ = scale dS K from it, so the backward executes the 5
 * matrix products of the algorithm instead of 7. Two layouts, picked by what the workspace holds (round 6): FULL ROWS - nq x nk squares per
 * (batch, head) pair, nq = ceil(Sq / 256), nk = ceil(Skv / 256): 32 MiB at S = 4096 - when there is room for every pair (the dQ kernel
 * streams 3-12 % faster from rows on 2 MiB boundaries), else THE CAUSAL HALF - only the squares at or below a row's diagonal, nq (nq + 1) / 2
 * when Sq = Skv: 17 MiB at S = 4096 - for as many pairs at a time as fit. The pairs are processed in GROUPS of as many as the workspace holds
 * dS for, so ANY workspace_bytes >= the minimum is accepted, for both head sizes and every S: with room for less than one pair's dS
 * (or with KF_ATTN_SPLIT_BWD set) the dQ kernel recomputes S and dP instead (minimum workspace, 7 products).
 * kf_attn_bwd_workspace_bytes() RECOMMENDS minimum + full rows for all pairs while that is within KF_ATTN_DS_CAP_MB MiB (default 16384), else
 * minimum + the causal half of as many pairs as the cap holds; with KF_ATTN_DS_TRI=1 always the causal half (config C3: 4.25 GiB instead of 8):
 * bounded whatever the problem size. No initialisation needed. Results depend neither on the group size nor on the layout (bit-identical).
 * No atomics in either form: dq, dk, dv are bitwise reproducible run to run.
 */
int kf_attn_bwd_workspace_bytes(int dtype, int64_t B, int64_t H, int64_t Sq, int64_t Skv, int64_t D,
                                size_t *bytes);
int kf_attn_bwd(int dtype, int64_t B, int64_t H, int64_t Sq, int64_t Skv, int64_t D, const void *q,
                const void *k, const void *v, const void *o, const float *lse, const void *d_o, void *dq,
                void *dk, void *dv, void *workspace, size_t workspace_bytes, void *stream);
int kf_attn_bwd_scaled(int dtype, int64_t B, int64_t H, int64_t Sq, int64_t Skv, int64_t D, float scale, const void *q,
                       const void *k, const void *v, const void *o, const float *lse, const void *d_o, void *dq,
                       void *dk, void *dv, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same two entries for tensors that are NOT contiguous [B,H,S,D]: each operand comes with the ELEMENT strides of its batch,
 * head and row dims (the head dim D itself is contiguous). This is what removes the layout copies around attention in a
 * transformer block (the reference's roadmap item qkv_linear, README.md:32): q, k, v are read in place from the packed
 * [B*S, 3*H*D] output of the QKV projection (batch = S*3*H*D, head = D, row = 3*H*D, bases offset by H*D), o is written
 * as [B*S, H*D] - the layout the output projection consumes - and the backward writes dq, dk, dv straight into a packed
 * [B*S, 3*H*D] gradient. Contiguous [B,H,S,D] is {H*S*D, S*D, D}. lse stays [B,H,Sq] contiguous f32.
 * 16-bit matrix-core path only (dtype KF_BF16 / KF_F16, D = 64 or 128; Skv >= Sq with any lengths, or Sq and Skv multiples of 128;
 * KF_ERR_UNSUPPORTED otherwise: make contiguous copies and call the plain entries). Strides are multiples of 8 elements, operands 16-byte aligned.
 * Workspace as kf_attn_bwd_workspace_bytes(). Grouped-query attention (fewer K/V heads than query heads, read in place from the packed
 * [B*S, (Hq + 2 Hkv) D] projection that kf_rope rotates) is kf_attn_*_gqa below.
 */
typedef struct kf_attn_layout {
    int64_t batch, head, row; /* element strides of dims B, H, S */
} kf_attn_layout;
int kf_attn_fwd_strided(int dtype, int64_t B, int64_t H, int64_t Sq, int64_t Skv, int64_t D, float scale, const void *q,
                        const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv,
                        void *o, const kf_attn_layout *lo, float *lse, void *stream);
int kf_attn_bwd_strided(int dtype, int64_t B, int64_t H, int64_t Sq, int64_t Skv, int64_t D, float scale, const void *q,
                        const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv,
                        const void *o, const kf_attn_layout *lo, const float *lse, const void *d_o, const kf_attn_layout *ldo, void *dq,
                        const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv, const kf_attn_layout *ldv,
                        void *workspace, size_t workspace_bytes, void *stream);

/*
 * Grouped-query attention (GQA; Hkv = 1 is multi-query attention): query head h of batch b attends to K/V head h / G, G = Hq / Hkv.
 * q, o, d_o, dq are [B, Hq, S, D]; k, v, dk, dv are [B, Hkv, Skv, D]; lse is [B, Hq, Sq] contiguous f32. Every other rule is that of the
 * entries above: causal mask, scale, dtypes, D <= 256, any Sq / Skv, the four tiers. The layouts are ALL NULL - contiguous tensors, every
 * tier - or ALL given - the _strided rules (16-bit matrix-core path only, else KF_ERR_UNSUPPORTED); a mix is KF_ERR_INVALID, and so are
 * Hkv < 1, Hkv > Hq, Hq % Hkv != 0, null operands, bad strides and a workspace below the minimum, all before any device call.
 * Hkv == Hq is exactly kf_attn_*_scaled (no layouts) / kf_attn_*_strided (layouts): the same launches, workspace and results.
 * The forward and dQ read K/V head h / G where the multi-head kernels read head h: o, lse and dq equal the multi-head call on K and V
 * repeated G times along the head dim, bit for bit. With G > 1 the dK/dV kernels run over the B Hq query heads into two partial arrays
 * in the workspace, and one more kernel (profile label attn_bwd_dkv_group_sum) forms
 *     dk[b, j] = dtype( ((f32 t_0 + t_1) + t_2) + ... + t_{G-1} ),   t_g = the dK of query head j G + g, rounded to the dtype
 * - the multi-head call's per-head dK on repeated K/V, summed once over each group in ascending g - and dv likewise. No atomics:
 * bitwise reproducible. Workspace (kf_attn_bwd_gqa_workspace_bytes): MINIMUM = the statistics of B Hq pairs (kf_attn_bwd's minimum) + two
 * 256-aligned arrays of B Hq Skv D elements of the dtype (G > 1 only; 512 MiB at bf16 B 8, Hq 32, S 4096, D 128); RECOMMENDED = minimum +
 * the dS part kf_attn_bwd_workspace_bytes gives for B Hq pairs. What lies beyond the minimum holds dS, as in kf_attn_bwd; any
 * workspace_bytes >= the minimum is accepted. minimum may be NULL.
 */
int kf_attn_fwd_gqa(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale,
                    const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk,
                    const void *v, const kf_attn_layout *lv, void *o, const kf_attn_layout *lo, float *lse, void *stream);
int kf_attn_bwd_gqa_workspace_bytes(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D,
                                    size_t *recommended, size_t *minimum);
int kf_attn_bwd_gqa(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale,
                    const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv,
                    const void *o, const kf_attn_layout *lo, const float *lse, const void *d_o, const kf_attn_layout *ldo,
                    void *dq, const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv, const kf_attn_layout *ldv,
                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * Full (non-causal) softmax attention with an optional per-batch key length: the attention of an encoder, of a cross-attention layer
 * (Sq and Skv in either size order) and of a padded batch. Operands, grouped K/V heads (g = h / (Hq / Hkv)) and the layout rule are
 * those of kf_attn_*_gqa above. kv_len: int64 [B] on the device, or NULL; len_b = clamp(kv_len[b], 0, Skv), NULL: Skv.
 *     s[m, n] = scale <q[b,h,m,:], k[b,g,n,:]>   for n < len_b (keys n >= len_b do not exist)
 *     o[b,h,m,:] = sum_n softmax_n(s[m,:])[n] v[b,g,n,:],   lse[b,h,m] = log sum_n exp s[m,n]   (natural log, f32, contiguous [B,Hq,Sq])
 * A batch with len_b == 0 has o = 0 and lse = -inf and contributes zero to every gradient. K and V rows at n >= len_b are never
 * read: padding may hold NaN or Inf. Backward: delta = rowsum(dO o O), dS = P o (dP - delta), dq = scale dS K, dk = scale dS^T Q and
 * dv = P^T dO summed over the G query heads of a K/V head in ascending order inside one kernel (f32 accumulators, no partial arrays);
 * rows n >= len_b of dk and dv are written as zeros. No atomics: bitwise reproducible run to run.
 * Kernels: bf16 / f16 with D = 64 or 128 and 16-byte aligned bases run the matrix-core kernels (any Sq, Skv >= 1; profile labels
 * attn_full_fwd_mfma_d64 / _d128, attn_full_bwd_delta, attn_full_bwd_dq_mfma_*, attn_full_bwd_dkv_mfma_*); f32 and every other head
 * size <= 256 run plain vector-ALU kernels (attn_full_*_generic: correct, not fast). Layouts: ALL NULL - contiguous [B,H,S,D], every
 * path - or ALL given - element strides, multiples of 8, 16-byte aligned bases, matrix-core path only (else KF_ERR_UNSUPPORTED); a mix
 * is KF_ERR_INVALID. lse may be NULL in the forward. The workspace (kf_attn_full_bwd_workspace_bytes: delta, O(B Hq Sq)) needs no
 * initialisation. Every argument is checked before any device call: KF_ERR_INVALID for a dtype outside {KF_F32, KF_BF16, KF_F16},
 * D < 1 or D > 256, Hkv < 1, Hkv > Hq, Hq % Hkv != 0, Skv < 1, negative extents, a scale that is not positive and finite, null
 * operands, bad strides or alignment and a workspace that is too small. B, Hq or Sq equal to 0 is KF_OK without a launch. No entry
 * synchronises or allocates: the calls can be captured with kf_graph_*.
 */
int kf_attn_full_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale,
                     const int64_t *kv_len, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk,
                     const void *v, const kf_attn_layout *lv, void *o, const kf_attn_layout *lo, float *lse, void *stream);
int kf_attn_full_bwd_workspace_bytes(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, size_t *bytes);
int kf_attn_full_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale,
                     const int64_t *kv_len, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk,
                     const void *v, const kf_attn_layout *lv, const void *o, const kf_attn_layout *lo, const float *lse,
                     const void *d_o, const kf_attn_layout *ldo, void *dq, const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk,
                     void *dv, const kf_attn_layout *ldv, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Prefix-LM softmax attention: full attention inside a per-batch prefix, causal after it, with the optional per-batch key length of
 * kf_attn_full_*. With prefix_len == NULL it is causal attention over a padded batch. Everything not said here - operands, grouped
 * K/V heads, the layout rule, lse, the argument checks and their statuses (with this entry's name in kf_last_error()), zero B, Hq or
 * Sq, capturability - is kf_attn_full_*'s contract. kv_len, prefix_len: int64 [B] on the device, or NULL.
 *     len_b = clamp(kv_len[b], 0, Skv)       (kv_len == NULL: Skv)
 *     pre_b = clamp(prefix_len[b], 0, Skv)   (prefix_len == NULL: 0)
 *     query m sees key n   <=>   n < len_b  and  (n < pre_b  or  n <= m)
 * The alignment is top-left with absolute indices, as in kf_attn_fwd; Sq and Skv may be in either size order. A batch with len_b == 0
 * has o = 0 and lse = -inf and contributes zero to every gradient; with len_b >= 1 every query sees key 0. Rows n >= len_b of dk and
 * dv are written as zeros, and so is a row n < len_b that no query sees (n >= pre_b and n >= Sq). K and V rows at n >= len_b are never
 * read. No atomics: bitwise reproducible; with pre_b >= len_b for every batch the results have the bits of kf_attn_full_*'s.
 * Kernels: the kernels of kf_attn_full_* compiled with the mask (it bounds the key tiles of a query block - min(len_b, max(pre_b,
 * last query + 1)) -, starts the query tiles of a key block beyond the prefix at the block, skips tiles no lane of a wave sees and
 * selects on the scores of the tiles the mask edge crosses). Profile labels attn_prefix_fwd_mfma_d64 / _d128,
 * attn_prefix_bwd_dq_mfma_*, attn_prefix_bwd_dkv_mfma_*, attn_prefix_*_generic; the delta pre-pass is shared and keeps
 * attn_full_bwd_delta (attn_full_bwd_delta_generic). The workspace is kf_attn_full_bwd_workspace_bytes' (delta), uninitialised.
 */
int kf_attn_prefix_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale,
                       const int64_t *kv_len, const int64_t *prefix_len, const void *q, const kf_attn_layout *lq, const void *k,
                       const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, void *o, const kf_attn_layout *lo, float *lse,
                       void *stream);
int kf_attn_prefix_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale,
                       const int64_t *kv_len, const int64_t *prefix_len, const void *q, const kf_attn_layout *lq, const void *k,
                       const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, const void *o, const kf_attn_layout *lo,
                       const float *lse, const void *d_o, const kf_attn_layout *ldo, void *dq, const kf_attn_layout *ldq, void *dk,
                       const kf_attn_layout *ldk, void *dv, const kf_attn_layout *ldv, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Sliding-window softmax attention: a band of keys around each query, either side optionally unbounded, with the optional per-batch
 * key length of kf_attn_full_*. Everything not said here - operands, grouped K/V heads, the layout rule, lse, the argument checks and
 * their statuses (with this entry's name in kf_last_error()), zero B, Hq or Sq, capturability - is kf_attn_full_*'s contract.
 * kv_len: int64 [B] on the device, or NULL. window_left, window_right: host scalars, a key count >= 0 or -1 for "unbounded on that
 * side"; anything below -1 is KF_ERR_INVALID (checked first, before any pointer is looked at).
 *     len_b = clamp(kv_len[b], 0, Skv)   (kv_len == NULL: Skv)
 *     query m sees key n   <=>   n < len_b  and  (wl < 0 or n >= m - wl)  and  (wr < 0 or n <= m + wr)
 * The alignment is top-left with absolute indices, as in kf_attn_fwd; Sq and Skv may be in either size order. (wl, 0) is a causal
 * sliding window (the query's own key and wl earlier ones), (w, w) a symmetric local window, (-1, 0) padded-causal attention and
 * (-1, -1) full attention; the last two are served by the kernels of kf_attn_prefix_* (prefix_len NULL) and kf_attn_full_*, have their
 * bits and their profile labels.
 * A query row that sees no key - possible inside a live batch: m - wl >= len_b - has o = 0 (zero bits), lse = -inf and dq = 0 and adds
 * nothing to dk or dv. Rows n >= len_b of dk and dv are written as zeros, and so is a row n < len_b that no query sees (n > Sq - 1 + wr,
 * the last key of the last query).
 * K and V rows at n >= len_b are never read. No atomics: bitwise reproducible.
 * Kernels: the kernels of kf_attn_full_* compiled with the window (a query block walks the key tiles max(0, q0 - wl) / 64 ..
 * ceil(min(len_b, qe + wr) / 64) - 1 only, a key block the query tiles max(0, k0 - wr) / 64 .. min(Sq - 1, k0 + 127 + wl) / 64; a wave
 * skips tiles outside the band of its 32 rows; the tiles an edge crosses select on their scores). Profile labels
 * attn_window_fwd_mfma_d64 / _d128, attn_window_bwd_dq_mfma_*, attn_window_bwd_dkv_mfma_*, attn_window_*_generic; the delta pre-pass
 * keeps attn_full_bwd_delta (attn_full_bwd_delta_generic). The workspace is kf_attn_full_bwd_workspace_bytes' (delta), uninitialised.
 */
int kf_attn_window_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale,
                       const int64_t *kv_len, int64_t window_left, int64_t window_right, const void *q, const kf_attn_layout *lq,
                       const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, void *o,
                       const kf_attn_layout *lo, float *lse, void *stream);
int kf_attn_window_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale,
                       const int64_t *kv_len, int64_t window_left, int64_t window_right, const void *q, const kf_attn_layout *lq,
                       const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, const void *o,
                       const kf_attn_layout *lo, const float *lse, const void *d_o, const kf_attn_layout *ldo, void *dq,
                       const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv, const kf_attn_layout *ldv,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * Document-masked softmax attention: one row of [B, H, S, D] holds several independent sequences packed end to end (packed documents
 * in LM pre-training, packed images of a vision encoder); a token attends inside its own document only. Self-attention: Sq = Skv = S.
 *
 * kf_attn_doc_table turns the documents' cumulative lengths into the per-token tables the kernels read. cu_doclens: int64
 * [B, n_docs + 1] on the device. With c_j = clamp(cu[b, j], 0, S) and c_0 taken as 0 whatever it holds, document j of row b holds the
 * tokens c_j <= m < c_{j+1} (a zero-length document owns no token: a ragged list is padded by repeating its last value) and
 * len_b = c_n. Written: kv_len[b] = len_b (int64 [B]); for a token of document j doc_start[b, m] = c_j and doc_end[b, m] = c_{j+1}
 * (int32 [B, S]); for m >= len_b doc_start = doc_end = len_b. cu[b, :] must be nondecreasing; if it is not the mask is unspecified, but
 * every value written lies in [0, S] with start <= end. One launch, one thread per token (a binary search over its row), no atomics,
 * capturable; profile label attn_doc_table. KF_ERR_INVALID: n_docs < 1, a negative extent, a null pointer; B or S equal to 0 is KF_OK
 * without a launch. The tables are built once per batch and serve every layer, forward and backward.
 *
 * kf_attn_doc_fwd / kf_attn_doc_bwd:
 *     len_b = clamp(kv_len[b], 0, S)   (kv_len == NULL: S)
 *     query m sees key n   <=>   n < len_b  and  doc_start[b, m] <= n < doc_end[b, m]  and  (causal == 0 or n <= m)
 * causal: 0 or 1, anything else is KF_ERR_INVALID (checked first). doc_start and doc_end are required: NULL is KF_ERR_INVALID wherever
 * a NULL operand is. The tables must describe a partition of the tokens into consecutive intervals - what kf_attn_doc_table writes;
 * then the relation is symmetric, and the dK/dV kernel reads the same two arrays at the key index to learn which queries see a key.
 * Every entry is clamped when it is read, so no table content moves an access outside an operand.
 * Everything not said here is kf_attn_full_*'s contract with this entry's name in kf_last_error(): operands, grouped K/V heads, the
 * layout rule, lse (lse = -inf and o = 0 as zero bits for a token in no document; dq = 0 there; rows of dk and dv that no query sees
 * are written as zeros), K and V rows at n >= len_b never read, no atomics and bitwise reproducible, the argument checks and their
 * statuses, zero extents, capturability. S >= 2^31 is KF_ERR_UNSUPPORTED (the tables are 32-bit). The workspace is
 * kf_attn_full_bwd_workspace_bytes(dtype, B, Hq, Hkv, S, S, D)'s; there is no second size query.
 * Kernels: the kernels of kf_attn_full_* compiled with the document mask - the window variant's interval per lane, read from the
 * tables: a query block walks the key tiles from that of its first row's start to that of its last row's end, a key block the query
 * tiles likewise; a wave skips tiles outside the interval of its 32 rows; tiles an edge crosses select on their scores. Profile labels
 * attn_doc_fwd_mfma_d64 / _d128, attn_doc_bwd_dq_mfma_*, attn_doc_bwd_dkv_mfma_*, attn_doc_*_generic; the delta pre-pass keeps
 * attn_full_bwd_delta (attn_full_bwd_delta_generic).
 */
int kf_attn_doc_table(int64_t B, int64_t S, int64_t n_docs, const int64_t *cu_doclens, int64_t *kv_len, int32_t *doc_start,
                      int32_t *doc_end, void *stream);
int kf_attn_doc_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, float scale, int causal,
                    const int64_t *kv_len, const int32_t *doc_start, const int32_t *doc_end, const void *q, const kf_attn_layout *lq,
                    const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, void *o,
                    const kf_attn_layout *lo, float *lse, void *stream);
int kf_attn_doc_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, float scale, int causal,
                    const int64_t *kv_len, const int32_t *doc_start, const int32_t *doc_end, const void *q, const kf_attn_layout *lq,
                    const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, const void *o,
                    const kf_attn_layout *lo, const float *lse, const void *d_o, const kf_attn_layout *ldo, void *dq,
                    const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv, const kf_attn_layout *ldv,
                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * The four masks above with two modifiers of the SCORES: logit soft-capping (Gemma-2, Grok) and attention sinks (gpt-oss, after
 * StreamingLLM). One descriptor-based trio; the mask is a kf_attn_mask, its visibility vis[b, m, n] that of the chosen kind, unchanged.
 *     x[m, n] = scale <q[b,h,m,:], k[b,h/G,n,:]>
 *     s[m, n] = softcap > 0 ? softcap tanh(x / softcap) : x                      for visible n
 *     Z[m]    = sum_n exp s[m, n]  +  (sink ? exp sink[h] : 0)
 *     o[m]    = sum_n exp(s[m, n]) v[n] / Z[m],      lse[m] = log Z[m]           (natural log, f32)
 * softcap: a host float, 0 = off; negative or not finite is KF_ERR_INVALID. sink: f32 [Hq] on the device, or NULL; the sink logit is
 * raw, neither scaled nor capped, joins the denominator and owns no value row. Backward, with P = exp(s - lse), delta = rowsum(dO o O)
 * and t = tanh(x / softcap):
 *     dS = P o (dP - delta) o (1 - t^2)   (the last factor only with softcap);  dq = scale dS K, dk = scale dS^T Q, dv = P^T dO
 *     dsink[h] = - sum_{b, m < Sq} exp(sink[h] - lse[b,h,m]) delta[b,h,m]       (f32 [Hq]; required exactly when sink is given)
 * kf_attn_mask: kind is one of KF_ATTN_MASK_*; kv_len serves every kind; prefix_len belongs to PREFIX, window_left / window_right to
 * WINDOW, doc_start / doc_end / causal to DOC (Sq must equal Skv), each with the meaning and the checks of its family's entries. A
 * field of another kind must hold its neutral value - NULL, (-1, -1), 0 - or the call is KF_ERR_INVALID, as is an unknown kind or a
 * NULL mask. Everything not said here is kf_attn_full_*'s contract with this entry's name in kf_last_error(): operands, grouped K/V
 * heads, the all-or-none layout rule, the argument checks before any device call, zero B, Hq or Sq (KF_OK without a launch; dsink is
 * not written then), K and V rows at n >= len_b never read, capturability. The workspace is delta, as kf_attn_full_bwd's.
 * A row that sees no key: without a sink o = 0 (zero bits), lse = -inf; with one o = 0 (zero bits), lse = sink[h] (the stored value),
 * dq = 0 and a zero term in dsink. The sink is folded into the forward epilogue against max(running maximum, sink), so no sink
 * overflows: sink = +100 gives o ~ 0 and lse ~ 100, a sink too small to move the denominator gives the bits of the call without one,
 * and sink = -inf is "no sink" exactly. No atomics anywhere, dsink included (attn_sink_grad: one workgroup per head, a fixed-order
 * sum over (b, m)): every result is bitwise reproducible.
 * Kernels: with softcap = 0 and sink = NULL the entries of the chosen family run - their kernels, their profile labels, their bits.
 * With softcap > 0 the same kernels compiled with the cap (tanh from v_exp_f32 and v_rcp_f32 after the score MFMAs, the factor
 * 1 - t^2 in the backward tile bodies): labels attn_<mask>_cap_fwd_mfma_d64 / _d128, attn_<mask>_cap_bwd_dq_mfma_*,
 * attn_<mask>_cap_bwd_dkv_mfma_*, attn_<mask>_cap_*_generic, <mask> in full / prefix / window / doc (the windows (-1, -1) and (-1, 0)
 * are full and prefix, as in kf_attn_window_*). A sink alone keeps the family's labels (its forward is the family's kernel compiled
 * with the sink epilogue, its backward the family's own); attn_sink_grad follows every backward with a sink.
 */
enum { KF_ATTN_MASK_FULL = 0, KF_ATTN_MASK_PREFIX = 1, KF_ATTN_MASK_WINDOW = 2, KF_ATTN_MASK_DOC = 3 };
typedef struct kf_attn_mask {
    int kind;                           /* KF_ATTN_MASK_* */
    const int64_t *kv_len;              /* every kind: int64 [B] on the device, or NULL */
    const int64_t *prefix_len;          /* PREFIX: int64 [B] on the device, or NULL */
    int64_t window_left, window_right;  /* WINDOW: key counts >= 0 or -1 (unbounded); every other kind: -1, -1 */
    const int32_t *doc_start, *doc_end; /* DOC: int32 [B, S] on the device (kf_attn_doc_table) */
    int causal;                         /* DOC: 0 or 1 */
} kf_attn_mask;
int kf_attn_ext_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale,
                    const kf_attn_mask *mask, float softcap, const float *sink, const void *q, const kf_attn_layout *lq,
                    const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, void *o,
                    const kf_attn_layout *lo, float *lse, void *stream);
int kf_attn_ext_bwd_workspace_bytes(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, size_t *bytes);
int kf_attn_ext_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale,
                    const kf_attn_mask *mask, float softcap, const float *sink, const void *q, const kf_attn_layout *lq,
                    const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, const void *o,
                    const kf_attn_layout *lo, const float *lse, const void *d_o, const kf_attn_layout *ldo, void *dq,
                    const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv, const kf_attn_layout *ldv,
                    float *dsink, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The document mask with a causal rule, a bidirectional prefix per document and a sliding window (packed rows in the local layers of
 * Mistral, Gemma-2/3 and gpt-oss; packed prefix-LM samples). Self-attention, Sq = Skv = S. Its own trio: kf_attn_mask and its kinds are
 * unchanged. c_j, len_b and document membership are kf_attn_doc_table's. For document j of row b,
 * P_j = c_j + clamp(doc_prefix[b, j], 0, c_{j+1} - c_j), or c_j when doc_prefix is NULL.
 *     query m sees key n   <=>   m and n lie in the same document j
 *                                and (causal == 0 or n <= m or n < P_j)
 *                                and (window_left < 0 or n >= m - window_left) and (window_right < 0 or n <= m + window_right)
 * Such a mask is one interval of keys per query and one interval of queries per key, and kf_attn_span_table writes both (int32 [B, S]):
 *     token m of document j as a query:  key_lo   = max(c_j, wl < 0 ? c_j : m - wl)
 *                                        key_hi   = min(c_{j+1}, causal ? max(m + 1, P_j) : c_{j+1}, wr < 0 ? c_{j+1} : m + wr + 1)
 *     token n of document j as a key:    query_lo = max(c_j, (causal and n >= P_j) ? n : c_j, wr < 0 ? c_j : n - wr)
 *                                        query_hi = min(c_{j+1}, wl < 0 ? c_{j+1} : n + wl + 1)
 * with hi = lo where hi < lo, all four equal to len_b for m >= len_b, every value in [0, S], and kv_len[b] = len_b (int64 [B]). All
 * four columns are nondecreasing along a row. With causal = 1 a window_right of 0 lets no query see a later key, so it cancels every
 * prefix: a prefix-LM window is (window_left, -1). doc_prefix: int64 [B, n_docs] on the device, or NULL. One launch, one thread per
 * token, no atomics, capturable; profile label attn_span_table. KF_ERR_INVALID: n_docs < 1, a negative extent, a null pointer
 * (doc_prefix may be NULL), causal not 0 or 1, a window side below -1, doc_prefix given with causal = 0. B or S equal to 0 is KF_OK
 * without a launch; S >= 2^31 is KF_ERR_UNSUPPORTED. The tables are built once per batch and serve every layer that shares the mask,
 * forward and backward.
 *
 * kf_attn_span_fwd / kf_attn_span_bwd: the forward and dQ read (key_lo, key_hi) at the query, dK/dV read (query_lo, query_hi) at the
 * key. If the two pairs do not describe one relation the mask is unspecified; every entry is clamped when it is read, so no table
 * content moves an access outside an operand. All tables are required wherever an operand is. softcap, sink and dsink follow
 * kf_attn_ext_*'s contract (softcap is checked first, then dsink against sink). Everything else is kf_attn_doc_*'s contract with this
 * entry's name in kf_last_error(): operands, layouts, grouped K/V heads, zero extents, the checks and their order, lse = -inf and zero
 * bits for a token that sees nothing, zeros for rows of dk and dv that no query sees, S >= 2^31 unsupported. The workspace is
 * kf_attn_full_bwd_workspace_bytes(dtype, B, Hq, Hkv, S, S, D)'s; there is no second size query.
 * Kernels: none of its own. The document kernels run without their causal rule (the tables hold it) - with softcap > 0 or a sink the
 * instantiations of kf_attn_ext_* with KF_ATTN_MASK_DOC - under the labels attn_doc_* / attn_doc_cap_*, attn_sink_grad after a backward
 * with a sink. Called without a window and a prefix the results have the bits of kf_attn_doc_* with the same causal flag.
 */
int kf_attn_span_table(int64_t B, int64_t S, int64_t n_docs, const int64_t *cu_doclens, const int64_t *doc_prefix, int causal,
                       int64_t window_left, int64_t window_right, int64_t *kv_len, int32_t *key_lo, int32_t *key_hi,
                       int32_t *query_lo, int32_t *query_hi, void *stream);
int kf_attn_span_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, float scale, const int64_t *kv_len,
                     const int32_t *key_lo, const int32_t *key_hi, float softcap, const float *sink, const void *q,
                     const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, void *o,
                     const kf_attn_layout *lo, float *lse, void *stream);
int kf_attn_span_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, float scale, const int64_t *kv_len,
                     const int32_t *key_lo, const int32_t *key_hi, const int32_t *query_lo, const int32_t *query_hi, float softcap,
                     const float *sink, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v,
                     const kf_attn_layout *lv, const void *o, const kf_attn_layout *lo, const float *lse, const void *d_o,
                     const kf_attn_layout *ldo, void *dq, const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv,
                     const kf_attn_layout *ldv, float *dsink, void *workspace, size_t workspace_bytes, void *stream);

/* ---- rotary position embeddings (no reference counterpart: the position signal between the QKV projection and attention) ---- */
/*
 * x, y: [B, H, S, D] addressed by kf_attn_layout element strides of B, H, S; D is contiguous; dtype in {KF_F32, KF_BF16, KF_F16};
 * any element-aligned base and strides (16-byte aligned heads, tables and R/2 a multiple of 16 / sizeof(T) take the packed path).
 * rotary_dim R: even, 2 <= R <= D. cos, sin: f32 [table_rows, R/2], contiguous. The position of token (b, s) is p = positions[b*S + s]
 * (int64 on the device, B*S of them) or p = s when positions is NULL. With c = cos[p, i], s = sin[p, i], i < R/2, each pair (a, b)
 *     interleaved = 0 (rotate-half: Llama, NeoX, HF rotate_half)   (a, b) = (i, i + R/2)
 *     interleaved = 1 (GPT-J)                                      (a, b) = (2i, 2i + 1)
 * becomes y_a = x_a c - x_b s, y_b = x_b c + x_a s, in f32 on the stored values with one rounding per output element. inverse = 1
 * uses -s: the exact transpose, i.e. the backward. Dims d >= R and heads h >= h_rot are copied, so ONE call over the packed QKV
 * projection [B*S, W], W = (Hq + 2 Hkv) D, with layout {S*W, D, W}, H = Hq + 2 Hkv and h_rot = Hq + Hkv rotates q and k and passes v
 * through. In place (y == x, same layout) the copied parts are not written; y must not otherwise overlap x. A position outside
 * [0, table_rows) makes that token's rotated elements NaN (no device assert, no read outside the table). One launch, no atomics,
 * no allocation, no synchronisation: calls can be captured with kf_graph_*. Every argument is checked before any device call:
 * KF_ERR_INVALID (dtype, R odd / < 2 / > D, h_rot outside [0, H], null pointers, table_rows < 1, no positions with S > table_rows,
 * y == x with another layout).
 * kf_rope_table writes cos[p, i] = cos(p base^(-2i/R)) and sin likewise for p < rows: the angle and both functions in f64, rounded
 * once to f32 (torch's f32 angle is off by about p 2^-24 rad at large p). A caller who wants torch's exact table or a scaled variant
 * (linear, NTK, Llama-3 frequency scaling) builds its own [rows, R/2] tables and passes them to kf_rope.
 */
int kf_rope(int dtype, int64_t B, int64_t H, int64_t S, int64_t D, int64_t h_rot, int64_t rotary_dim, int interleaved, int inverse,
            const float *cos, const float *sin, int64_t table_rows, const int64_t *positions, const void *x, const kf_attn_layout *lx,
            void *y, const kf_attn_layout *ly, void *stream);
int kf_rope_table(double base, int64_t rotary_dim, int64_t rows, float *cos, float *sin, void *stream);

/* ---- gated activations (no reference counterpart: the non-linearity of a SwiGLU / GeGLU MLP between its two projections) ---- */
enum {
    KF_ACT_SILU = 0,      /* g / (1 + exp(-g))                                                              */
    KF_ACT_GELU_TANH = 1, /* 0.5 g (1 + tanh(sqrt(2/pi) (g + 0.044715 g^3))): torch's approximate = 'tanh'  */
    KF_ACT_GELU_ERF = 2   /* g 0.5 (1 + erf(g / sqrt 2))                                                    */
};
/*
 * gate, up, h, dh, dgate, dup: [rows, F] row-major with leading dimensions in elements, each >= F; one dtype in {KF_F32, KF_BF16,
 * KF_F16} for all of them. The packed projection [rows, 2F] (columns gate | up: what ONE GEMM against the concatenated weights
 * writes) is gate = x, up = x + F, ldg = ldu = 2F, and the backward writes one packed gradient the same way: no split, no concat, no
 * copy on either side.
 *     forward    h = act(g) u                                   (up == NULL: the ungated h = act(g); ldu is ignored)
 *     backward   dup = dh act(g),  dgate = dh u act'(g)         (up == NULL needs dup == NULL: dgate = dh act'(g))
 * evaluated in f32 on the stored values with one rounding per output element; the backward recomputes act from gate and up, the
 * forward keeps nothing. Every finite input gives a finite result unless the product itself leaves the dtype's range: where exp
 * would overflow the result is the limit (0, or g u). NaN in gives NaN out; g = +inf gives inf * u; g = -inf gives NaN (-inf * 0,
 * as torch's x * sigmoid(x) and its GELU do).
 * Allowed aliases, bitwise equal to the out-of-place call: h == gate or h == up; dgate == gate and / or dup == up; each with the same
 * leading dimension (the backward then overwrites the projection with its gradient). Anything else must not overlap. Columns F .. ld
 * of an output row are never written. Any element-aligned base, F and leading dimensions work; 16-byte aligned bases with F and all
 * leading dimensions multiples of 16 / sizeof(T) take the path with 16-byte loads and stores, and both paths give the same bits.
 * Row offsets are 64-bit (rows * ld may exceed 2^31). One launch, no workspace, no atomics, no allocation, no synchronisation:
 * calls can be captured with kf_graph_*; rows == 0 or F == 0 is KF_OK without a launch. Every argument is checked before any device
 * call: KF_ERR_INVALID (act, dtype, negative extents, a leading dimension < F, null gate / h / dh / dgate, dup without up or up
 * without dup, a base not aligned to its element, an alias with another leading dimension).
 */
int kf_glu_fwd(int act, int dtype, int64_t rows, int64_t F, const void *gate, int64_t ldg, const void *up, int64_t ldu,
               void *h, int64_t ldh, void *stream);
int kf_glu_bwd(int act, int dtype, int64_t rows, int64_t F, const void *gate, int64_t ldg, const void *up, int64_t ldu,
               const void *dh, int64_t lddh, void *dgate, int64_t lddg, void *dup, int64_t lddu, void *stream);

/* ---- row softmax and log_softmax (no reference counterpart: MoE routers, sampling, distillation, contrastive heads) ---- */
enum { KF_SOFTMAX = 0, KF_LOG_SOFTMAX = 1 };
/*
 * x, y, dy, dx: [rows, V] row-major with leading dimensions in elements, each >= V; one dtype in {KF_F32, KF_BF16, KF_F16} for all of
 * them; the arithmetic is f32 with one rounding per output element. Over the last dimension, with s = scale * x (scale finite, > 0:
 * 1 / temperature) and lse = log sum_v exp(s_v):
 *     KF_SOFTMAX       y_v = exp(s_v - lse)        dx_v = scale * y_v * (dy_v - sum_u dy_u y_u)
 *     KF_LOG_SOFTMAX   y_v = s_v - lse             dx_v = scale * (dy_v - exp(y_v) * sum_u dy_u)
 * The backward works from the forward's OUTPUT y: a caller keeps y, not x.
 * Special values, as torch: a -inf element gives 0 (softmax) or -inf (log_softmax), and the formulas above for its gradient (0 for
 * softmax, scale * dy_v for log_softmax); a row that holds a NaN or +inf, or only -inf, is NaN throughout; no other row is affected.
 * Large logits (|s| ~ 1e4) keep f32 accuracy: the max is taken out inside one FMA and its rounding residual is folded back.
 * Allowed aliases, bitwise equal to the out-of-place call: y == x with ldy == ldx (an in-place forward); dx == dy with lddx == lddy.
 * Every other overlap of an output with an input is refused (column blocks of one wider buffer, whose rows interleave, do not overlap).
 * Columns V .. ld of an output row are never written. Bases need the alignment of an element only: a row is read as a scalar head up to
 * the first 16-byte boundary, 16-byte packs, and a scalar tail, so odd V and odd leading dimensions keep the vector access; where the
 * rows of two operands sit differently against the 16-byte boundaries the call takes the element path, with the same bits. The order in
 * which a row is summed depends on V and on the 16-byte phase of the row of x (y in the backward) only.
 * Regimes, from (rows, V) alone: V <= 2048 one wave per row, 2048 < V <= 16384 one 256-thread block per row (the row - in the backward y
 * and dy - in registers: read once, written once); longer rows one block per row in two passes (the online max and sum, or the row sum;
 * then a re-read and the write). Row offsets are 64-bit (rows * ld may exceed 2^31); rows < 2^31. One launch, no workspace, no atomics, a
 * fixed combination order: bitwise reproducible; no allocation, no synchronisation: calls can be captured with kf_graph_*. rows == 0 or
 * V == 0 is KF_OK without a launch. Every argument is checked before any device call: KF_ERR_INVALID (kind, dtype, negative extents, a
 * scale that is not finite and > 0, a null pointer, a leading dimension < V, a base not aligned to its element, an alias not listed).
 */
int kf_softmax_fwd(int kind, int dtype, int64_t rows, int64_t V, float scale, const void *x, int64_t ldx, void *y, int64_t ldy,
                   void *stream);
int kf_softmax_bwd(int kind, int dtype, int64_t rows, int64_t V, float scale, const void *y, int64_t ldy, const void *dy, int64_t lddy,
                   void *dx, int64_t lddx, void *stream);

/* ---- per-head QK-norm fused with the rotary embedding (no reference counterpart: the RMS norm over every q and k head that
 *      Chameleon, Qwen3, Gemma-3 and OLMo-2 put between the QKV projection and attention) ---- */
/*
 * x, y, dy, dx: [B*S, W], W = (Hq + Hk + Hv) D, each with a row stride ld* >= W in elements; the heads of a token in the order
 * q | k | v; wq, wk, dwq, dwk: [D]; one dtype in {KF_F32, KF_BF16, KF_F16} for all of them. A NULL weight means 1, a NULL dw* is not
 * computed. Hq, Hk, Hv >= 0 with Hq + Hk >= 1 (Hq = H, Hk = Hv = 0: the separate q of a cross-attention layer).
 * rotary_dim R: even, 0 <= R <= D. R = 0 is the norm alone (a ViT): cos, sin and positions are then ignored and may be NULL. Tables
 * (f32 [table_rows, R/2]), positions (int64 [B*S] or NULL: p = t % S) and the pairs (interleaved) are exactly kf_rope's.
 *     forward    for every q head (weight wq) and every k head (weight wk) of every token
 *                rstd = 1 / sqrt(mean_d x_d^2 + eps),  n_d = x_d rstd w_d,  y = kf_rope's rotation of n over its leading R dims
 *     backward   rstd and xhat = x rstd recomputed from x; g = the inverse rotation of dy (identity beyond R), gw = g w,
 *                m = mean_d(gw_d xhat_d):  dx_d = rstd (gw_d - xhat_d m),  dwq_d = sum over tokens and q heads of g_d xhat_d, dwk likewise
 * all in f32 on the stored values with ONE rounding, at the store. The composition of kf_norm_fwd (KF_NORM_RMS) and kf_rope rounds n
 * to the storage type in between, so its bits differ from this entry's in f16 and bf16. The sum of squares is a plain f32 sum: where
 * it overflows (|x| ~ 1e18 and above, depending on D) the result is what the formula gives in f32, rstd = 0 and y = 0. eps scales
 * tiny inputs as the formula says (x = 1e-20, eps = 1e-6: y = 1e-17 w). An all-zero head gives zeros (eps > 0). A NaN or Inf stays
 * inside its head in y and dx (and reaches dw*). A position outside [0, table_rows) makes that token's rotated elements of y NaN,
 * and in the backward all of dx of that token's q and k heads and the rotated dims of dw*; nothing is read outside the table.
 * v heads are copied bit for bit out of place (dx = dy in the backward) and not written in place. Allowed aliases, bitwise equal to
 * the out-of-place call: y == x with ldy == ldx; dx == dy with lddx == lddy. Every other overlap of an output with an input is
 * refused; dx must not overlap x. Columns W .. ld of an output row are never written.
 * The weight sums leave each block as one f32 row [2][D] of the workspace (kf_qk_norm_rope_bwd_workspace_bytes; needed only when dwq
 * or dwk is given) and a second small kernel adds the rows in a fixed order: no atomics, bitwise reproducible, and the workspace
 * needs no initialisation. The backward keeps nothing but x.
 * With every head start, both tables and the weights 16-byte aligned, D a multiple of two 16-byte packs (D / pack <= 128) and R = 0
 * or R/2 a multiple of the pack, the call moves 16-byte packs; an odd leading dimension or base keeps the same lanes on the same
 * elements (the same bits); any other geometry (R = 2, an odd D) takes an element kernel. Offsets are 64-bit. Neither entry
 * synchronises or allocates: calls can be captured with kf_graph_*. B, S or D of 0 is KF_OK without a launch. Every argument is
 * checked before any device call: KF_ERR_INVALID (dtype, negative extents, Hq + Hk < 1, R odd or > D, interleaved not 0 / 1, eps
 * negative or not finite, a leading dimension < W, a null operand, R > 0 without tables, table_rows < 1, no positions with
 * S > table_rows, a base not aligned to its element, a forbidden overlap, a workspace that is too small).
 */
int kf_qk_norm_rope_fwd(int dtype, int64_t B, int64_t S, int64_t Hq, int64_t Hk, int64_t Hv, int64_t D, int64_t rotary_dim,
                        int interleaved, double eps, const void *wq, const void *wk, const float *cos, const float *sin,
                        int64_t table_rows, const int64_t *positions, const void *x, int64_t ldx, void *y, int64_t ldy, void *stream);
int kf_qk_norm_rope_bwd_workspace_bytes(int dtype, int64_t B, int64_t S, int64_t Hq, int64_t Hk, int64_t Hv, int64_t D, size_t *bytes);
int kf_qk_norm_rope_bwd(int dtype, int64_t B, int64_t S, int64_t Hq, int64_t Hk, int64_t Hv, int64_t D, int64_t rotary_dim,
                        int interleaved, double eps, const void *wq, const void *wk, const float *cos, const float *sin,
                        int64_t table_rows, const int64_t *positions, const void *x, int64_t ldx, const void *dy, int64_t lddy,
                        void *dx, int64_t lddx, void *dwq, void *dwk, void *workspace, size_t workspace_bytes, void *stream);

/* ---- segmented (expert) GEMM with device-side offsets (no reference counterpart: the expert product of a mixture-of-experts layer -
 *      Mixtral, Qwen3-MoE, DeepSeek-V3 - and both of its backward products; the routing is softmax, topk, sort and embedding) ---- */
/*
 * offsets: int64 [E + 1] in DEVICE memory, E >= 1: expert e owns the rows offsets[e] <= r < offsets[e + 1] of operands whose rows are
 * sorted by expert. No entry reads them back: nothing synchronises, allocates or uses atomics, every output element is written by exactly
 * one workgroup and every sum runs in an order that depends on the arguments only, so results are bitwise reproducible and calls can be
 * captured with kf_graph_*. The kernels sanitise the offsets themselves: o'_0 = clamp(o_0, 0, T), o'_e = clamp(max(o_e, o'_(e-1)), 0, T);
 * malformed offsets change which rows belong to whom, never what memory is touched.
 *     segment_offsets   offsets[e] = the number of ids < e for e = 0 .. E: a lower bound over ASCENDING ids (one binary search per
 *                       entry), so ids below 0 or at least E fall outside [offsets[0], offsets[E]). n == 0 gives zeros.
 *     gemm_segmented    C[r, :] = alpha A[r, :] op(W_e) + beta C[r, :] for the rows of segment e. A is [T, K] with pitch lda, C is [T, N];
 *                       W_e = W + e w_stride (elements) is stored [K, N] when trans_b == 0 and [N, K] when trans_b == 1 (the dX form),
 *                       pitch ldw. A row that no segment covers gets beta C: +0 bit for bit when beta == 0 (a dropped token has a zero
 *                       output and a zero gradient). beta == 0 never reads C.
 *     wgrad             dW_e[M, N] = alpha A[seg_e, :]^T B[seg_e, :] + beta dW_e, A [T, M], B [T, N], dW_e = dW + e dw_stride with
 *                       pitch lddw; an empty segment gives beta dW_e. Rows outside segment e never enter dW_e, not even as a factor of
 *                       zero: a neighbour's Inf or NaN stays out.
 * dtype is KF_BF16, KF_F16 or KF_F32 for every operand; the arithmetic is f32 with one rounding per output element. 16-bit operands
 * with N % 128 == 0, the fixed contraction a multiple of 64 (wgrad: M % 128 == 0 and N % 128 == 0), pitches and strides multiples of 8
 * and 16-byte aligned bases run on the matrix cores (128 x 128 x 64 tiles that never straddle a segment, LDS-DMA staging, a four-stage
 * ring); anything else takes a plain kernel with the same semantics. Row offsets are 64-bit. The workspace
 * (workspace_bytes(dtype, T, E): the sanitised offsets and a table of T / 128 + E + 2 row tiles, 16-byte aligned) needs no
 * initialisation and is rewritten by every call. Every argument is checked before any device call: KF_ERR_INVALID for null pointers,
 * negative extents, E < 1, a pitch below its extent, an expert stride below one expert's extent, a dtype outside the three, trans_b
 * outside {0, 1}, a base not aligned to its element, a workspace that is missing, too small or misaligned. A zero T, N, K or M is
 * KF_OK without a launch.
 */
int kf_segment_offsets(const int64_t *sorted_ids, int64_t n, int64_t E, int64_t *offsets /* [E+1] */, void *stream);
int kf_gemm_segmented_workspace_bytes(int dtype, int64_t T, int64_t E, size_t *bytes);
int kf_gemm_segmented(int dtype, int trans_b, int64_t T, int64_t N, int64_t K, int64_t E, const int64_t *offsets,
                      float alpha, const void *A, int64_t lda, const void *W, int64_t ldw, int64_t w_stride,
                      float beta, void *C, int64_t ldc, void *workspace, size_t workspace_bytes, void *stream);
int kf_gemm_segmented_wgrad(int dtype, int64_t T, int64_t M, int64_t N, int64_t E, const int64_t *offsets,
                            float alpha, const void *A, int64_t lda, const void *B, int64_t ldb,
                            float beta, void *dW, int64_t lddw, int64_t dw_stride,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ---- mixture-of-experts token routing on the device (no reference counterpart: what surrounds the expert product above - the plan,
 *      the gate, the dispatch and the weighted combine of Mixtral, Qwen3-MoE, DeepSeek-V3 - with both directions of each) ---- */
/*
 * T tokens choose k experts out of E each; n = T k, and pair p = t k + j is token t's j-th choice. ids: int64 [n] in DEVICE memory (the
 * indices of a top-k). The plan sorts the pairs by expert once; everything else moves rows by its two 32-bit tables, so no backward
 * sorts and no entry reads an extent back: nothing synchronises, allocates or uses atomics, every sum runs in a fixed order (bitwise
 * reproducible), and calls can be captured with kf_graph_*. n >= 2^31 is KF_ERR_UNSUPPORTED (the tables are 32-bit).
 *     plan          key_p = ids[p] if 0 <= ids[p] < E, else E: such a pair is DROPPED (kf_segment_offsets' rule for ids outside [0, E)).
 *                   A stable ascending sort of the pairs by key (kf_sort): row_pair[r] (int32 [n]) = the pair in sorted row r,
 *                   pair_row[p] (int32 [n]) = its inverse, offsets[e] (int64 [E + 1]) = the number of pairs with key < e, so
 *                   offsets[0] = 0, offsets[E] = n_valid, and the dropped pairs fill the rows [n_valid, n) in pair order. offsets feeds
 *                   kf_gemm_segmented unchanged. n == 0 still writes zero offsets. The workspace (kf_moe_plan_workspace_bytes: the keys,
 *                   the sorted keys and positions and kf_sort's scratch; 16-byte aligned) needs no initialisation.
 *     gate_fwd      s_j = p[t, ids[t, j]] (p: [T, E], pitch ldp), 0 for a dropped pair. gate[t, j] = s_j (normalize == 0) or s_j / S
 *                   (normalize == 1), S = s_0 + ... + s_(k-1) summed in that order in f32; S = 0 gives what the formula gives.
 *     gate_bwd      writes EVERY element of dp [T, E]: zeros, then dp[t, ids[t, j]] += ds_j in the order j (f32, rounded once), with
 *                   ds_j = dgate_j (normalize == 0) or (dgate_j - sum_i dgate_i gate_i) / S (normalize == 1: S recomputed from p, gate the
 *                   forward's stored result, the sum in the order i over the pairs that are not dropped). Dropped pairs contribute nothing.
 *     dispatch      xs[r, :] = x[row_pair[r] / k, :] for r < n, bit for bit. A row_pair[r] outside [0, n) writes the row as +0 and reads
 *                   nothing.
 *     combine       y[t, :] = sum_j gate[t, j] ys[pair_row[t, j], :], accumulated in f32 from +0 in the order j = 0 .. k-1 (a product,
 *                   then a sum), rounded once. gate == NULL means 1: the backward of dispatch, dx[t] = sum_j dxs[pair_row[t, j]]. n_valid
 *                   is a DEVICE pointer to one int64 (pass offsets + E), read by the kernel and clamped to [0, n]; NULL means n. A pair
 *                   whose pair_row lies outside [0, n_valid) is skipped: neither its row nor its gate is read (a NaN gate of a dropped
 *                   pair stays out). A token with no live pair gets +0. The first 8 rows of a token are loaded together; pairs beyond 8
 *                   are added one at a time.
 *     combine_bwd   for every pair p = (t, j) with r = pair_row[p] in [0, n): dys[r, :] = gate[t, j] dy[t, :] for a live pair (one
 *                   product, one rounding), dy[t, :] bit for bit when gate == NULL, +0 when r >= n_valid. dgate[t, j] = sum_c dy[t, c]
 *                   ys[r, c] for a live pair, else +0: f32, in an order that depends on cols only, one rounding. dgate == NULL is
 *                   allowed (the gate needs no gradient; ys may then be NULL too); gate == NULL requires dgate == NULL. One pass: dy[t] is
 *                   read once per token for k <= 8 (once per 8 pairs beyond). With tables that are a permutation every row of dys is
 *                   written exactly once. An entry outside [0, n) names no row.
 * Every index a kernel reads is range-checked where it is read: malformed ids or tables change what is computed, never what memory is
 * touched.
 * No operand may alias another: an output must not overlap an input or another output (there is no in-place form; a combine writes
 * y[t] while other workgroups still read ys). This is not checked.
 * dtype is KF_F32, KF_BF16 or KF_F16 for every floating operand; the arithmetic is f32 with one rounding per output element. Rows have
 * leading dimensions in elements (ld* >= the row's extent) and 64-bit row offsets; columns beyond the extent are never written. Bases
 * need the alignment of an element only: with the row operands 16-byte aligned and cols and their leading dimensions multiples of
 * 16 / sizeof(element) a call moves 16-byte packs, anything else takes the element path, where the same lanes own the same elements:
 * the same bits. Regimes, from cols alone: cols <= 1024 one wave per row, longer rows one 256-thread block per row. Profile labels
 * moe_plan, moe_gate_fwd, moe_gate_bwd, moe_dispatch, moe_combine, moe_combine_bwd.
 * Every argument is checked before any device call, with the entry's name in kf_last_error(): KF_ERR_INVALID for null required pointers
 * (with T == 0 the plan's ids and tables may be NULL), negative extents, k < 1, E < 1, a leading dimension below its extent, a dtype
 * outside the three, normalize outside {0, 1}, a base not aligned to its element (ids, offsets and n_valid to 8 bytes, the tables to 4),
 * a workspace that is missing, too small or not 16-byte aligned. T == 0, and cols == 0 where nothing is left to write, is KF_OK without
 * a launch.
 */
int kf_moe_plan_workspace_bytes(int64_t T, int64_t k, int64_t E, size_t *bytes);
int kf_moe_plan(const int64_t *ids, int64_t T, int64_t k, int64_t E, int64_t *offsets /* [E+1] */, int32_t *row_pair /* [T k] */,
                int32_t *pair_row /* [T k] */, void *workspace, size_t workspace_bytes, void *stream);
int kf_moe_gate_fwd(int dtype, int64_t T, int64_t k, int64_t E, const int64_t *ids, const void *p, int64_t ldp, int normalize,
                    void *gate, int64_t ldg, void *stream);
int kf_moe_gate_bwd(int dtype, int64_t T, int64_t k, int64_t E, const int64_t *ids, const void *p, int64_t ldp, int normalize,
                    const void *gate, int64_t ldg, const void *dgate, int64_t lddg, void *dp, int64_t lddp, void *stream);
int kf_moe_dispatch(int dtype, int64_t T, int64_t k, int64_t cols, const int32_t *row_pair, const void *x, int64_t ldx,
                    void *xs, int64_t ldxs, void *stream);
int kf_moe_combine(int dtype, int64_t T, int64_t k, int64_t cols, const int32_t *pair_row, const int64_t *n_valid,
                   const void *gate, int64_t ldg, const void *ys, int64_t ldys, void *y, int64_t ldy, void *stream);
int kf_moe_combine_bwd(int dtype, int64_t T, int64_t k, int64_t cols, const int32_t *pair_row, const int64_t *n_valid,
                       const void *gate, int64_t ldg, const void *ys, int64_t ldys, const void *dy, int64_t lddy,
                       void *dys, int64_t lddys, void *dgate, int64_t lddg, void *stream);

/* ---- the mixture-of-experts router in front of that routing (no reference counterpart: the top-k choice and gates of Mixtral,
 *      Qwen3-MoE and DeepSeek-V3 and the auxiliary losses of Switch / Megatron and ST-MoE, fused, with both directions of each) ---- */
/*
 * logits: [T, E] (pitch ldl), one row per token. One wave owns a token's E logits in registers, so 1 <= k <= min(E, 64) and E <= 1024;
 * anything larger is KF_ERR_UNSUPPORTED. score is KF_MOE_SCORE_SOFTMAX or KF_MOE_SCORE_SIGMOID, normalize 0 or 1.
 *     router_fwd    SELECTION: ids[t, 0 .. k) (int64 [T, k], dense) are the first k positions of the stable descending order of row t in
 *                   kf_sort's key order for the dtype: by value, -0.0 below +0.0, NaNs by bit pattern (a NaN with the sign bit clear
 *                   above +inf, one with it set below -inf), equal keys by lower index first. The comparison is on the stored bits and
 *                   involves no arithmetic: ids equal the indices of this library's descending kf_sort of the row bit for bit, for both
 *                   scores (softmax and sigmoid are monotone).
 *                   GATE (f32, one rounding per stored element): softmax: m = the row maximum, e_v = exp(l_v - m), Z = sum_v e_v,
 *                   s_j = e_(ids_j) / Z; sigmoid: s_j = 1 / (1 + exp(-l_(ids_j))). gate[t, j] = s_j (normalize == 0) or s_j / S
 *                   (normalize == 1), S = s_0 + ... + s_(k-1) summed in the order j as kf_moe_gate_fwd does. A row with a NaN, a +inf or
 *                   only -inf gives what the formula gives (NaN gates for softmax); ids stay defined by the key order in every case.
 *     router_bwd    recomputes the row from logits and ids (the stored gate is not read) and writes EVERY element of dlogits [T, E]: the
 *                   exact derivative of the gate formula contracted with dgate [T, k], zero where the derivative is zero (with sigmoid,
 *                   and with softmax + normalize, off the chosen columns). An id outside [0, E) contributes nothing and reads nothing.
 *     aux_loss_fwd  p = softmax(logits) in f32; c_e = offsets[e + 1] - offsets[e], the live pairs of expert e (offsets: int64 [E + 1] on
 *                   the DEVICE, the plan's, read by the kernel and treated as a constant);
 *                   L_bal = E / (T k) sum_e c_e (1 / T) sum_t p[t, e]   (the Switch / Megatron normalisation: 1 for uniform routing;
 *                   HF-Mixtral's load_balancing_loss_func gives k times this); L_z = (1 / T) sum_t lse_t^2, lse_t = m + log Z (ST-MoE);
 *                   loss[0] = balance_coef L_bal + z_coef L_z, parts = {L_bal, L_z} when not NULL (f32, device). No atomics: a block
 *                   keeps the column sums and the sum of lse^2 of the rows it walks in registers, its four waves are added in wave order
 *                   and one f32 partial row of E + 1 sums goes to the workspace (kf_moe_aux_loss_workspace_bytes, 16-byte aligned, no
 *                   initialisation); a second kernel (one block) adds the partial rows in block order inside 16 contiguous slices, the
 *                   slices in order, and writes the scalars: bitwise reproducible.
 *     aux_loss_bwd  one pass over logits, EVERY element of dlogits written:
 *                   dlogits[t, e] = dloss p_e (a_e - sum_u a_u p_u + z_t), a_e = balance_coef E c_e / (T^2 k), z_t = z_coef 2 lse_t / T;
 *                   dloss is one f32 read from the DEVICE.
 * dtype is KF_F32, KF_BF16 or KF_F16 for logits, gate, dgate and dlogits. Rows have leading dimensions in elements (>= their extent) and
 * 64-bit row offsets; columns beyond the extent are never read into a result or written. Bases need the alignment of an element only
 * (ids and offsets 8 bytes, loss / parts / dloss 4): with logits (and dlogits) 16-byte aligned and their leading dimensions multiples of
 * 16 / sizeof(element) a row moves in 16-byte packs, otherwise the same lanes move the same elements one by one with the same arithmetic:
 * the same bits. Nothing synchronises, allocates or reads an extent back: every entry can be captured with kf_graph_*. No operand may
 * alias another. Profile labels moe_router_fwd, moe_router_bwd, moe_aux_fwd, moe_aux_fold, moe_aux_bwd.
 * Every argument is checked before any device call, with the entry's name in kf_last_error(): KF_ERR_INVALID for a dtype outside the
 * three, T < 0, E < 1, k < 1, T E or T k beyond int64, score or normalize outside {0, 1}, null or misaligned pointers, a leading
 * dimension below its extent, a workspace that is missing, too small or not 16-byte aligned; KF_ERR_UNSUPPORTED for E > 1024 or
 * k > min(E, 64). T == 0 is KF_OK without a launch (nothing is written).
 */
enum { KF_MOE_SCORE_SOFTMAX = 0, KF_MOE_SCORE_SIGMOID = 1 };
int kf_moe_router_fwd(int dtype, int64_t T, int64_t E, int64_t k, int score, int normalize, const void *logits, int64_t ldl,
                      int64_t *ids /* [T, k] */, void *gate, int64_t ldg, void *stream);
int kf_moe_router_bwd(int dtype, int64_t T, int64_t E, int64_t k, int score, int normalize, const void *logits, int64_t ldl,
                      const int64_t *ids, const void *dgate, int64_t lddg, void *dlogits, int64_t lddl, void *stream);
int kf_moe_aux_loss_workspace_bytes(int64_t T, int64_t E, size_t *bytes);
int kf_moe_aux_loss_fwd(int dtype, int64_t T, int64_t E, int64_t k, const void *logits, int64_t ldl,
                        const int64_t *offsets /* [E + 1], the plan's */, float balance_coef, float z_coef, float *loss /* [1] */,
                        float *parts /* [2] = {L_bal, L_z}, or NULL */, void *workspace, size_t workspace_bytes, void *stream);
int kf_moe_aux_loss_bwd(int dtype, int64_t T, int64_t E, int64_t k, const void *logits, int64_t ldl, const int64_t *offsets,
                        float balance_coef, float z_coef, const float *dloss /* device, [1] */, void *dlogits, int64_t lddl,
                        void *stream);

/* ---- per-tensor scaled FP8 on the block-scaled matrix pipe (no reference counterpart: the Transformer-Engine recipe with current
 *      scaling). FP8 data are bytes in the OCP encodings gfx950 uses: e4m3fn (largest value 448, no infinity, NaN =
 *      0x7f / 0xff) and e5m2 (largest finite value 57344). ---- */
/*
 *     fp8_amax      *amax = max |x| over the row-pitched [rows, cols] matrix x (KF_F32, KF_F16 or KF_BF16; ld in elements, >= cols). The
 *                   entry zeroes *amax on the stream (a one-lane launch) and the kernel combines per-wave partials with an integer atomic max
 *                   on the bits of |float(x)|: the result does not depend on block order. Any NaN in x gives the quiet NaN 0x7fc00000
 *                   (its bits lie above every number's). rows * cols == 0 gives 0.
 *     fp8_quantize  scale = 2^e, e the largest integer with amax * 2^e <= fmt_max (448 = 0.875 * 2^9, 57344 = 0.875 * 2^16: e follows
 *                   from frexp(amax) and one compare of its mantissa with 0.875), clamped to [-126, 126]; e = 0 when *amax is 0,
 *                   infinite or NaN. *scale_inv = 2^-e, exactly. q[r, c] = cvt_rne(clamp(float(x[r, c]) * scale, -fmt_max, fmt_max)):
 *                   the product by a power of two is exact, the clamp is explicit (no mode register decides saturation), and a NaN
 *                   becomes 0x7f with x's sign bit. q is [rows, cols] bytes with pitch ldq >= cols. qt (may be NULL) is the transposed
 *                   image [cols, rows] of the same bytes with pitch ldqt >= ceil16(rows); columns rows .. ceil16(rows) - 1 of each of
 *                   its rows are written as zero bytes, so a product may contract over ceil16(rows). q and qt come from ONE read of x.
 *                   No other byte of q or qt is written. amax is read on the device (kf_fp8_amax's result, or any caller's bound).
 *     gemm_fp8      C[M, N] = (*scale_inv_a * *scale_inv_b) A[M, K] B[N, K]^T: both operands K-contiguous bytes (the only layout; the
 *                   transposed copies of fp8_quantize supply the other products), f32 accumulation on
 *                   v_mfma_scale_f32_16x16x128_f8f6f4 with every block scale 1.0, one rounding to out_dtype (KF_F32, KF_BF16, KF_F16).
 *                   The two scales are read on the device. All four format pairs. M, N >= 0 (0: KF_OK without a launch); K a positive
 *                   multiple of 16; lda, ldb multiples of 16, >= K and at most 2^24; A and B 16-byte aligned, C aligned to its element;
 *                   ldc >= N. A K tail short of 128 and ragged M / N edges are handled in the kernel by range-checked loads (bytes
 *                   outside [rows, K] are never read into a result) and guarded stores. No workspace, no padded copies, no split-K:
 *                   two runs give the same bits. Special codes go through the instruction as IEEE values: a NaN code (e4m3 0x7f / 0xff,
 *                   e5m2 0x7d .. 0x7f with either sign) in A makes every output of its row of C NaN (in B: of its column), against
 *                   zero codes too; an e5m2 +infinity in A against a strictly positive column of B makes its row of C +infinity. Every
 *                   other output keeps the bits it has without that byte, wherever the byte sits (first K block, K tail, last row of a
 *                   ragged edge tile): tests/test_gpu_fp8_edges.py.
 * Nothing synchronises, allocates or reads a value back: every entry can be captured with kf_graph_*. Profile labels fp8_amax,
 * fp8_quantize, gemm_fp8. Every argument is checked before any device call, with the entry's name in kf_last_error(): KF_ERR_INVALID for
 * a dtype, format or out_dtype outside the lists, negative extents, a leading dimension below its extent (ldqt < ceil16(rows)) or not a
 * multiple of 16 where that is required, K not a positive multiple of 16, null or misaligned pointers.
 */
enum { KF_FP8_E4M3 = 0, KF_FP8_E5M2 = 1 };
int kf_fp8_amax(int dtype, int64_t rows, int64_t cols, int64_t ld, const void *x, float *amax /* device, [1] */, void *stream);
int kf_fp8_quantize(int dtype, int fmt, int64_t rows, int64_t cols, int64_t ld, const void *x, const float *amax /* device, [1] */,
                    void *q, int64_t ldq, void *qt /* or NULL */, int64_t ldqt, float *scale_inv /* device, [1] */, void *stream);
int kf_gemm_fp8(int fmt_a, int fmt_b, int out_dtype, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda, const void *B,
                int64_t ldb, const float *scale_inv_a /* device, [1] */, const float *scale_inv_b /* device, [1] */, void *C,
                int64_t ldc, void *stream);

/* ---- collectives (RCCL over xGMI): the one exchange step of the batch-sharded path (§8e) ---- */
#define KF_COMM_ID_BYTES 128
int kf_comm_unique_id(char id[KF_COMM_ID_BYTES]);
int kf_comm_init(void **comm, const char id[KF_COMM_ID_BYTES], int rank, int world_size);
int kf_comm_destroy(void *comm);
/* in-place sum all-reduce of `count` elements of dtype (KF_F32, KF_BF16, KF_F16, KF_F64, ints) */
int kf_allreduce_sum(void *comm, void *buf, size_t count, int dtype, void *stream);
/* the same over n buffers as ONE collective launch (an RCCL group): the tensors of all_reduce_(list) that are not one flat range */
int kf_allreduce_sum_multi(void *comm, int n, void *const *bufs, const size_t *counts, int dtype, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KFUNCA_HIP_H_ */
