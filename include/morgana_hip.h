/*
 * morgana_hip.h - C ABI of libmorgana_hip.so: the MI355X (gfx950) kernels behind morgana's acoustic-model
 * training hot path (ExperimentBuilder.train_epoch -> BaseSPSS.forward -> backward -> Adam).
 *
 * The reference (ZackHodari/morgana) is pure Python and has no FFI; every entry point below replaces the
 * PyTorch-eager op sequence of the cited reference lines.  The reference-side binding a maintainer would add is
 * the ctypes stub shown in INTEGRATION.md (morgana_amd/_lib.py is that stub, used by this repo's own host layer).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types.  All pointers are DEVICE pointers unless a
 *     parameter is documented as host.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - Every function is asynchronous on `stream`, never allocates or frees memory and never synchronises the
 *     device: the caller owns outputs and workspaces (sizes from the *_workspace_bytes helpers).
 *   - Return value: 0 on success, negative MG_E* on error; mg_last_error() gives a thread-local message.
 *   - Row-major everywhere.  "bf16" buffers hold raw 16-bit bfloat16 values (uint16_t).
 *   - Gather convention ("rows"): an int32 array, one entry per output row, holding the source-table row or -1
 *     for the all-zero pad row (reference: the zero `padder` frame appended at utils.py:206-207).
 */
#ifndef MORGANA_HIP_H
#define MORGANA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_OK 0
#define MG_EINVAL (-1)   /* bad argument (shape, alignment, null pointer) */
#define MG_ELAUNCH (-2)  /* HIP reported a launch error */
#define MG_EWORKSPACE (-3) /* workspace too small */

#define MG_ACT_NONE 0
#define MG_ACT_SIGMOID 1
/* torch.nn.Tanh / torch.nn.ReLU behind an nn.Linear (reference: the modules SequentialWithRecurrent.forward runs one by one,
 * morgana/utils.py:401-418).  Accepted by mg_linear_fwd_f32, mg_linear_fwd_bf16, mg_phone_front_linear_fwd_bf16,
 * mg_phone_concat_layer_bf16, mg_linear_dgrad_act_* and mg_act_*; the shape-specialised fused kernels stay Sigmoid only. */
#define MG_ACT_TANH 2
#define MG_ACT_RELU 3
/* OR-ed into `act` of mg_linear_fwd_bf16: `rows` is made of RUNS of equal consecutive indices (the frame map of
 * upsample_to_repetitions: every phone row repeated `dur` times).  A performance hint only - results do not depend on it: the
 * gathered operand is then staged once per distinct row (csrc/gemm_nt_runs.hip); rows without runs cost up to 4 passes there. */
#define MG_ACT_ROWS_RUNS 0x100

/* ------------------------------------------------------------------------------------------------------------------
 * Library
 * ---------------------------------------------------------------------------------------------------------------- */
const char* mg_last_error(void);
/* Scheduling choices: which of several kernels / split plans that compute THE SAME RESULTS an entry point launches.  For A/B runs
 * inside one process and for the equality tests that hold the forms against each other.  PROCESS-GLOBAL state (not per call, not
 * thread-local): set it between launches, not concurrently with them; everything else in this ABI is stateless apart from the
 * thread-local error text.  Unknown keys and values are refused (MG_EINVAL).  Measured-slower experiments and timing probes are
 * not in this library at all: they are compiled into the lab builds (make -C morgana_amd/csrc lab / diag) only. */
#define MG_TUNING_KEYS 8
#define MG_TUNE_FORM 0          /* large bf16 GEMM kernels: 0 = default; 3 = 32-deep instead of 64-deep stages of the 128-wide NT tile;
                                 * 6 = per-tile instead of persistent NT kernel; 14 = frame-staged instead of run-staged layer-1 forward,
                                 * 16 = its fragments read one k-step ahead;
                                 * fused backward: 12 = tiles two steps ahead (larger ring), 13 = 32-frame steps, 7 = single-buffered */
#define MG_TUNE_GRU_HANDOFF 2   /* persistent GRU / LSTM kernels: 0 = groups found on one XCD hand the state over through that XCD's L2,
                                 * bit 0 (1) = always write-through (sc1) stores, the placement-independent form;
                                 * bit 2 (4) = the bf16 GRU backward with 8 groups x 16-unit slots (default: 16 groups x 32-unit slots, B <= 128);
                                 * values with any other bit are refused */
#define MG_TUNE_PERSISTENT 3    /* recurrences: 0 = persistent kernels where the shape has them, 1 = one launch per time step,
                                 * 2 = H = 64 on the 16-row tile instead of the 4x4x1 blocks */
#define MG_TUNE_WGRAD_SPLITS 4  /* wide weight-gradient kernel: != 0 overrides the planned number of split-M slabs (a multiple of 8);
                                 * 1000 + S / 2000 + S override the one-n-tile / the 4+-n-tile plans only */
#define MG_TUNE_WGRAD_ORDER 5   /* wide weight-gradient kernel, block order: 0 = planned, 1 = n tile fastest, 2 = the n tiles of a split
                                 * on one XCD, 3 = the 128 x 128 kernel instead of the wide one */
#define MG_TUNE_LSTM_BWD_STACK 6 /* LSTM stack wavefronts, hidden units per slot: 0 = backward 32 where they fit (one workgroup per CU),
                                 * forward 16 (two per CU); bit 0 (1) = backward 16; bit 1 (2) = forward 32 (same bits, measured slower) */
#define MG_TUNE_AB 7            /* shared-grid launches as their separate launches, half-width tiles off: 65 = mg_linear_wgrad_dgrad_bf16 as
                                 * two launches, 66 = mg_phone_front_linear_fwd_bf16 as two,
                                 * 85 = plain write-back stores everywhere (default: H1 in the phone-rate step's first launch and dZ1 / the slabs
                                 * of mg_linear_wgrad_dgrad_bf16's shared grid - one tile or split per workgroup - leave as write-through stores,
                                 * so that the kernel boundary behind the launch finds no dirty lines to write back; the same bytes either way), 86 = mg_f0_l2tail_x3 with four waves per workgroup (default: eight), 87 / 88 = 64-deep LDS stages in the phone-rate forward GEMM (pair planes,
                                 * three passes / bf16; measured equal to slower, round 5), 89 = the pair-plane forward GEMM (mg_phone_front_linear_fwd_x3) as three passes
                                 * over the plane (default: all four planes' k-tile per stage), 90 = the pair-plane weight gradients
                                 * (mg_linear_wgrad_slabs_x3) as three walks over their rows (default: one walk, all four planes per
                                 * stage - the same products in another order), 91 = 128 x 512 tiles for the 512-wide weight
                                 * gradient where the square 256 x 256 tile is the default (N a multiple of 256), 92 = 128 x 640 tiles for the 640-wide weight
                                 * gradient at phone-rate rows, 93 = 128 x 512 tiles for the 512-wide one, 94 = mg_phone_front_linear_fwd_bf16 with the
                                 * front's jobs as block jobs and 256-row tiles (round 2's form), 95 = wave jobs but 256-row tiles,
                                 * 96 = mg_f0_l2tail_*_bf16 walks H1 from its first tile at every size (default: from the last one when
                                 * H1 is larger than the L2s hold; per-workgroup sums then add in another order);
                                 * the wide NT GEMM's tile for few-tile shapes: 97 = 256-wide whenever N allows, 99 = 128-wide always,
                                 * 98 = under 32,768 rows the 128 x 128 kernel (default: 128-wide when 256-wide tiles would be < 128) */
int mg_set_tuning(int key, int value);
int mg_version(void);           /* ABI version, bumped on incompatible change */
const char* mg_build_arch(void); /* "gfx950" */

/* ------------------------------------------------------------------------------------------------------------------
 * K1  upsample_to_repetitions            reference: morgana/utils.py:175-228
 * ---------------------------------------------------------------------------------------------------------------- */
/* n_frames[b] = sum_p max(dur[b,p], 0); *tmax = max_b n_frames[b]  (utils.py:198-199).  dur int64 [B,P]; a negative duration
 * counts as 0, as in the index maps below (the reference's np.repeat raises on one). */
int mg_upsample_lengths(const int64_t* dur, int B, int P, int64_t* n_frames, int64_t* tmax, void* stream);

/* Frame->phone map (utils.py:214-220, the per-utterance np.repeat loop).  Any of the outputs may be NULL.
 *   idx64 [B,t_cap]  phone index or -1   (the reference's `repeated_idxs`, bit exact)
 *   rows32[B,t_cap]  b*P + phone or -1   (flat source row, the gather convention of this library)
 * Frames t >= n_frames[b] get -1.  Requires t_cap >= 0 and P <= 16384.  If t_cap < n_frames[b] the row is cropped. */
int mg_upsample_index(const int64_t* dur, int B, int P, int t_cap, int64_t* idx64, int32_t* rows32, void* stream);
/* The same launch also writing the phone-rate maps (csrc/phone_rate.hip): rows_mapped = rows32 with -1 replaced by pad_row, and
 * seg_start / seg_end int32 [B*P] = the run of frame ids (b * t_cap + t) of every phone row, (0, 0) for a phone without frames. */
int mg_upsample_index_maps(const int64_t* dur, int B, int P, int t_cap, int32_t* rows32, int32_t* rows_mapped, int pad_row,
                           int32_t* seg_start, int32_t* seg_end, void* stream);

/* out[m,:] = rows[m] < 0 ? 0 : src[rows[m],:]   (utils.py:226).  src [R,F] f32, out [M,F] f32. */
int mg_gather_rows_f32(const float* src, const int32_t* rows, float* out, int64_t M, int F, void* stream);
/* Same gather, output converted to bf16 with leading dimension ldo >= F; columns F..ldo-1 are zero filled. */
int mg_gather_rows_bf16(const float* src, const int32_t* rows, uint16_t* out, int64_t M, int F, int ldo, void* stream);

/* Segment index maps (reference: split_to_segments / get_segment_ends, morgana/utils.py:231-330; the same scan-and-index
 * pattern as mg_upsample_index).  seg_lens int64 [B,S]; T = length of the sequence feature; L = longest segment.
 *   split [B,S,L] : flat source row b*T + start_s + j of position j of segment s, -1 where j >= len_s (the zero padder)
 *   ends  [B,S]   : flat source row b*T + cumsum_s - 1 of the last frame of segment s, -1 for empty segments
 * Either output may be NULL.  Feed them to mg_gather_rows_f32; rows that would fall beyond T come out as -1.
 * mg_scatter_rows_f32 is the adjoint of such a gather (distinct targets): dst[rows[m],:] = src[m,:] for rows[m] >= 0;
 * dst must be zero-filled by the caller. */
int mg_segment_index(const int64_t* seg_lens, int B, int S, int T, int L, int32_t* split, int32_t* ends, void* stream);
int mg_scatter_rows_f32(const float* src, const int32_t* rows, float* dst, int64_t M, int F, void* stream);

/* Packed frames for ragged batches.  The reference pads a batch to its longest utterance (collate_fn, morgana/data.py:183-193), runs
 * every nn.Linear on all B*T rows (morgana/utils.py:401-418) and masks the loss (losses.py:37-39); behind a recurrent wrapper the
 * padded frames are zero rows (utils.py:383).  mg_frame_layout builds the maps that let the row-wise layers run on the
 * total = sum_b min(seq_len[b], T) valid rows plus ONE representative zero row:
 *   offsets int32 [B+1]     first packed row of utterance b (offsets[B] = total)
 *   rows    int32 [total+1] dense row b*T + t of packed row i, utterance by utterance; rows[total] = -1
 *   inverse int32 [B*T]     packed row of dense row (b, t); `total` for padded frames
 * `total` is supplied by the caller (the host knows the lengths it collated); frames beyond it count as padding.
 * pack = mg_gather_rows_*(x, rows), unpack = mg_gather_rows_f32(packed, inverse); the adjoint of the unpack is a gather by `rows` for
 * the valid rows and, for the representative row, the sum over all padded dense rows: mg_pad_rows_colsum_f32 (g [B,T,D] -> out [D],
 * fixed summation order; workspace mg_pad_rows_colsum_workspace_bytes(B,T,D)). */
int mg_frame_layout(const int64_t* seq_len, int B, int T, int64_t total, int32_t* offsets, int32_t* rows, int32_t* inverse,
                    void* stream);
size_t mg_pad_rows_colsum_workspace_bytes(int B, int T, int D);
int mg_pad_rows_colsum_f32(const float* g, const int64_t* seq_len, int B, int T, int D, float* out, void* workspace, size_t workspace_bytes,
                           void* stream);

/* Ragged pack of padded sequence features (reference: utils.detach_batched_seqs / batched_masked_select, morgana/utils.py:66-102,
 * :147-166; csrc/unpad.hip).  ONE launch compacts up to MG_UNPAD_MAX features of any element type into one byte buffer: item b of
 * feature f contributes len = min(max(seq_len[b], 0), T_f) frames, whose bytes land at
 *   dst + dst_offset_f + row_bytes_f * sum_{b' < b} len_b'      and come from      src_f + b * T_f * row_bytes_f.
 * The launch moves bytes (bit-identical for every dtype).  seq_len int64 [B] is read ON THE DEVICE and scanned there; `descs` is a
 * HOST array.  Nothing is written outside [dst_offset_f, dst_offset_f + block_bytes_f), whatever seq_len holds: rows that do not
 * fit the block are dropped.  Refused (MG_EINVAL): count outside 1..MG_UNPAD_MAX, B outside 0..MG_UNPAD_MAX_ITEMS, row_bytes <= 0,
 * T < 0, dst_offset not a non-negative multiple of 16, a block outside [0, dst_bytes) or overlapping another, NULL pointers where
 * bytes would move.  B == 0 or no block that holds a row: MG_OK without a launch. */
#define MG_UNPAD_MAX 16
#define MG_UNPAD_MAX_ITEMS 4096
typedef struct {
    const void* src;        /* [B, T, row_bytes] contiguous                           */
    int64_t T;              /* padded axis of THIS feature (features may differ)      */
    int64_t row_bytes;      /* bytes of one frame: trailing elements x element size   */
    int64_t dst_offset;     /* start of this feature's block in dst, multiple of 16   */
    int64_t block_bytes;    /* capacity of the block; nothing is written beyond it    */
} mg_unpad_desc;
int mg_unpad_rows(const mg_unpad_desc* descs, int count, const int64_t* seq_len, int B, void* dst, int64_t dst_bytes, void* stream);

/* out[i] = all_k (xs[k][i] != 0) for 1..MG_ALL_NONZERO_MAX float32 inputs of n elements each (reference: utils.both_voiced_mask,
 * morgana/utils.py:169-172 = prod_k ~torch.eq(x_k, 0.): NaN counts as non-zero, -0.0 as zero).  `xs` is a HOST array of device
 * pointers; the output element is encoded as in mg_sequence_mask (elem_size 1 / 4 / 8 bytes, as_float). */
#define MG_ALL_NONZERO_MAX 8
int mg_all_nonzero_f32(const float* const* xs, int count, int64_t n, void* out, int elem_size, int as_float, void* stream);

/* Gather fused with the frame-level concat the shipped models do right after it (models/RNN_SPSS.py:76-81,
 * models/f0_test_model.py:78-79: upsample_to_repetitions, then torch.cat with `normalised_counters`):
 *   out[m, 0:F] = src[rows[m], :] (0 where rows[m] < 0), out[m, F:F+C] = extra[m, 0:C], out[m, F+C:ldo] = 0.
 * extra [M,C] f32.  The bf16 form needs ldo % 8 == 0 and produces the padded layer-1 operand directly. */
int mg_gather_concat_f32(const float* src, const int32_t* rows, const float* extra, float* out, int64_t M, int F, int C,
                         int ldo, void* stream);
int mg_gather_concat_bf16(const float* src, const int32_t* rows, const float* extra, uint16_t* out, int64_t M, int F, int C,
                          int ldo, void* stream);

/* Adjoint of the gather (autograd of utils.py:226): grad_src[b,p,:] = sum of grad_out[b,t,:] over the frames of
 * phone p (frames of a phone are contiguous).  grad_out [B,T,F], dur int64 [B,P], grad_src [B,P,F]. Deterministic. */
int mg_upsample_backward_f32(const float* grad_out, const int64_t* dur, float* grad_src, int B, int P, int T, int F,
                             void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * sequence_mask                           reference: morgana/utils.py:115-144
 * ---------------------------------------------------------------------------------------------------------------- */
/* mask[b,t] = t < seq_len[b].  elem_size selects the output type: 1 = uint8, 4 = float32, 8 = int64. */
int mg_sequence_mask(const int64_t* seq_len, int B, int max_len, void* mask, int elem_size, int as_float,
                     void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K4  seq_len-masked MSE, forward + backward   reference: morgana/losses.py:29-51
 * ---------------------------------------------------------------------------------------------------------------- */
/* loss = mean_{b,d}( sum_t m[b,t] (p-y)^2 / n_b ), n_b = min(seq_len[b], T) (T when seq_len == NULL);
 * grad = 2 (p-y) m / (n_b B D) * grad_scale, written for every element (zeros on padding).  n_b == 0 gives NaN,
 * as the reference does.  pred/target [B,T,D] f32; loss: one float; grad may be NULL.
 * workspace: mg_masked_mse_workspace_bytes(B,T,D) bytes.  Deterministic two-stage reduction (no atomics). */
size_t mg_masked_mse_workspace_bytes(int B, int T, int D);
int mg_masked_mse_f32(const float* pred, const float* target, const int64_t* seq_len, int B, int T, int D,
                      float grad_scale, float* loss, float* grad, void* workspace, size_t workspace_bytes,
                      void* stream);

/* Same contract with binary cross entropy as the per-element loss (reference: losses.bce, morgana/losses.py:54-56, used for
 * the voicing stream at models/RNN_SPSS.py:137): -(y log p + (1-y) log(1-p)), logs clamped at -100 as torch does. */
int mg_masked_bce_f32(const float* pred, const float* target, const int64_t* seq_len, int B, int T, int D,
                      float grad_scale, float* loss, float* grad, void* workspace, size_t workspace_bytes,
                      void* stream);

/* Multi-stream loss (reference: LSTMAcousticModel.loss, models/RNN_SPSS.py:120-139, with the torch.sigmoid of :93):
 * pred [B,T,D] f32 holds the streams side by side (torch.split at :87-88); stream k covers columns col0..col0+width-1
 * and is scored against its own target [B,T,width] (row stride ldt) with losses.mse (MG_LOSS_MSE) or with
 * losses.bce(sigmoid(pred)) (MG_LOSS_SIGMOID_BCE).  loss = mean over streams of the per-stream sequence loss
 * (the `loss / 4.` of :139).  grad [B,T,D] (may be NULL) = grad_scale * d loss / d pred, zero in columns no stream
 * covers; prob [B,T,width] (may be NULL) receives sigmoid(pred) of the one BCE stream (`pred_vuv`, :93).
 * `streams` is a HOST array, n_streams <= MG_STREAMS_MAX. */
#define MG_STREAMS_MAX 8
#define MG_LOSS_MSE 0
#define MG_LOSS_SIGMOID_BCE 1
typedef struct {
    const float* target;
    int ldt;
    int col0;
    int width;
    int kind;
} mg_stream_desc;
size_t mg_stream_loss_workspace_bytes(int B, int T, int D);
int mg_stream_loss_f32(const float* pred, const mg_stream_desc* streams, int n_streams, const int64_t* seq_len, int B, int T,
                       int D, float grad_scale, float* loss, float* grad, float* prob, void* workspace,
                       size_t workspace_bytes, void* stream);

/* seq_len-masked categorical cross entropy, forward + backward (reference: losses.ce, morgana/losses.py:59-61 -
 * F.cross_entropy(predictions.transpose(1, 2), targets, reduction='none') - under the sequence_loss wrapper of :29-46).
 *   l[b,t] = logsumexp_c x[b,t,:] - x[b,t,y[b,t]],  L = mean_b( sum_{t < n_b} l[b,t] / n_b ),  n_b = seq_len[b] clamped to [0, T]
 *   (T when seq_len == NULL; n_b == 0 gives NaN, as the reference's 0 / 0),
 *   loss[0] = loss_weight * L + loss_keep * loss[0]   (loss_keep == 0: loss[0] is not read; how a multi-stream loss is summed on the
 *   device), grad[b,t,c] = grad_scale * (softmax(x[b,t,:])[c] - [c == y[b,t]]) / (n_b B) for t < n_b and exactly 0 for pad frames
 *   (written, not skipped), argmax[b,t] = the lowest index among the largest logits (0 for pad frames).
 * pred: f32, frame (b,t) at pred + (b T + t) ldp + col0, C classes - a column slice of a wider prediction is read in place;
 * grad (may be NULL) likewise with ldg / gcol0: only those C columns of each row are written.  target [B,T] int64; seq_len [B] int64
 * or NULL; argmax [B,T] int64 or NULL.  A target of -100 in a valid frame (F.cross_entropy's default ignore_index): loss and
 * gradient of that frame are 0, the frame still counts in n_b.  Any other target outside [0, C) in a valid frame: NaN loss, zero
 * gradient row, nothing is read or written out of bounds (the reference asserts on the device).  Targets of pad frames are never
 * looked at and their logits are not read.  The maximum is subtracted before expf; a -inf logit of a non-target class is legal
 * (probability and gradient 0).  1 <= C <= MG_CE_MAX_CLASSES, B <= 65535.  Per-workgroup partials in a fixed layout and a
 * one-workgroup finishing pass: no atomics, the same bits on every call.  workspace: mg_masked_ce_workspace_bytes(B,T,C) bytes. */
#define MG_CE_MAX_CLASSES 65536
size_t mg_masked_ce_workspace_bytes(int B, int T, int C);
int mg_masked_ce_f32(const float* pred, int ldp, int col0, const int64_t* target, const int64_t* seq_len, int B, int T, int C,
                     float grad_scale, float loss_weight, float loss_keep, float* loss, float* grad, int ldg, int gcol0,
                     int64_t* argmax, void* workspace, size_t workspace_bytes, void* stream);

/* seq_len-masked mixture-density negative log likelihood, forward + backward (no counterpart in the reference: a K-component
 * diagonal-Gaussian output layer over a stream's static + delta + delta-delta vector; Zen & Senior, ICASSP 2014).
 * A frame's row holds W = K (1 + 2 D) columns: [ a_0 .. a_{K-1} | mu_{0,0} .. mu_{0,D-1}, mu_{1,0} .. mu_{K-1,D-1} | s_{0,0} ..
 * s_{K-1,D-1} ] = logits, means (component-major), log standard deviations; target [B,T,D] f32 with row stride ldt.
 *   z_kd = (y_d - mu_kd) exp(-s_kd),   q_k = log_softmax(a)_k - sum_d (0.5 z_kd^2 + s_kd) - D * 0.9189385332046727,
 *   l[b,t] = -logsumexp_k(q_k) / D  (nats per dimension),   L = mean_b( sum_{t < n_b} l[b,t] / n_b ),  n_b = seq_len[b] clamped to
 *   [0, T] (T when seq_len == NULL; n_b == 0 gives NaN),   loss[0] = loss_weight * L + loss_keep * loss[0]  (loss_keep == 0: loss[0]
 *   is not read).  With r_k = exp(q_k - logsumexp q) and c = grad_scale / (D n_b B):
 *   grad a_k = c (softmax(a)_k - r_k),   grad mu_kd = -c r_k z_kd exp(-s_kd),   grad s_kd = c r_k (1 - z_kd^2)
 * for t < n_b and exactly 0 for pad frames (written, not skipped); pad frames of pred and target are never read.  has_floor != 0:
 * s is replaced by max(s, min_log_std) and an s below the floor gets gradient 0 (torch.clamp's rule).  A -inf logit removes its
 * component exactly; all logits -inf give NaN.  pred: frame (b,t) at pred + (b T + t) ldp + col0 - a column slice of a wider
 * prediction is read in place; grad (may be NULL) likewise with ldg / gcol0: only those W columns of each row are written.
 * 1 <= K <= MG_MDN_MAX_COMPONENTS, K * D <= MG_MDN_MAX_ROW, B <= 65535 (MG_EINVAL otherwise, before any launch).  Per-workgroup
 * partials in a fixed layout and a one-workgroup finishing pass: no atomics, the same bits on every call.
 * workspace: mg_masked_mdn_workspace_bytes(B,T,K,D) bytes.
 * mg_mdn_select_f32 (generation, forward only, one launch): component[b,t] = the lowest index among the largest logits,
 * mean[b,t,:] = mu of that component (exact copies), variance[b,t,:] = exp(2 max(s, floor)) of that component; pad frames are
 * written as 0, 0 and 1.  component [B,T] int64, mean / variance [B,T,D] f32, contiguous.
 * mg_mdn_sample_f32 (generation by sampling, forward only, one launch, no workspace, no atomics, no host read; layout, caps and pad
 * rule of mg_mdn_select_f32): per valid frame, row index r = b T + t, in fp32, one wave per frame:
 *   w_k = expf((a_k - max_j a_j) * inv_temperature)  (a -inf logit gives exactly 0),  c_k = w_0 + .. + w_k as a wave scan in one
 *   fixed order,  S = c_{K-1};  u = u(word r % 4 of Philox block r / 4) under component_site - counter words, key and u(w) as
 *   documented for mg_vae_sample_f32 below;  component[b,t] = the lowest k with u * S < c_k;  if there is none (the product rounded
 *   up to S) the highest k with w_k > 0;  if S is NaN (every logit -inf) what mg_mdn_select_f32 returns.  A component whose logit is
 *   -inf is never drawn otherwise.  variance[b,t,d] = exp(2 max(s_kd, floor)) of that component.  noise_scale == 0: mean[b,t,d] =
 *   mu_kd, an exact copy, no noise word is drawn;  otherwise mean[b,t,d] = mu_kd + noise_scale exp(max(s_kd, floor)) g, g the
 *   N(0, 1) value of flat element r * D + d under noise_site by the Box-Muller mapping of mg_vae_sample_f32, word for word (blocks
 *   straddle rows when D % 4 != 0).  The counters of pad frames are not used: a frame's draw is a function of (seed, site, *counter,
 *   b, t, d) alone, not of seq_len or ldp.  inv_temperature finite and > 0, noise_scale finite and >= 0, component_site !=
 *   noise_site (MG_EINVAL otherwise, before any launch); seed, the sites and counter (DEVICE uint64, NULL = 0) as mg_vae_sample_f32. */
#define MG_MDN_MAX_COMPONENTS 64
#define MG_MDN_MAX_ROW 16384
size_t mg_masked_mdn_workspace_bytes(int B, int T, int K, int D);
int mg_masked_mdn_f32(const float* pred, int ldp, int col0, const float* target, int ldt, const int64_t* seq_len, int B, int T, int K,
                      int D, float min_log_std, int has_floor, float grad_scale, float loss_weight, float loss_keep, float* loss,
                      float* grad, int ldg, int gcol0, void* workspace, size_t workspace_bytes, void* stream);
int mg_mdn_select_f32(const float* pred, int ldp, int col0, const int64_t* seq_len, int B, int T, int K, int D, float min_log_std,
                      int has_floor, int64_t* component, float* mean, float* variance, void* stream);
int mg_mdn_sample_f32(const float* pred, int ldp, int col0, const int64_t* seq_len, int B, int T, int K, int D, float min_log_std,
                      int has_floor, float inv_temperature, float noise_scale, uint64_t seed, uint32_t component_site, uint32_t noise_site,
                      const uint64_t* counter, int64_t* component, float* mean, float* variance, void* stream);

/* Streaming metrics (reference: morgana/metrics.py:359-695; accumulated inside the shipped model's loss() every step,
 * models/RNN_SPSS.py:120-129): accum[0] += sum, accum[1] += count on the device - no host read-back (the reference calls .item()
 * per accumulate).  kind: MG_METRIC_MEAN (target only), _SQDIFF (RMSE / MelCepDistortion), _ABSDIFF (MAE), _ROOT_SQ (Distortion:
 * per-frame root of the summed squares), _SQDIFF_VOICED (F0Distortion), _SQDIFF_VOICED_EXP (LF0Distortion: on exp of both).
 * target / pred [B,T,D] f32, columns [col0, col0 + width) take part; voiced [B,T] f32 0/1 (voiced kinds); seq_len may be NULL.
 * The masked count is in frames, the unmasked one in elements, as in the reference (metrics.py:383-394). */
#define MG_METRIC_MEAN 0
#define MG_METRIC_SQDIFF 1
#define MG_METRIC_ABSDIFF 2
#define MG_METRIC_ROOT_SQ 3
#define MG_METRIC_SQDIFF_VOICED 4
#define MG_METRIC_SQDIFF_VOICED_EXP 5
size_t mg_metric_workspace_bytes(void);
int mg_metric_accumulate_f32(int kind, const float* target, const float* pred, const float* voiced, const int64_t* seq_len, int B,
                             int T, int D, int col0, int width, double* accum, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K8  maximum-likelihood parameter generation    reference: morgana/viz/synthesis.py:79-178 (MLPG), :8-36 (_build_win_mats),
 *     :39-77 (_build_poe); called per training step from predict() - models/f0_test_model.py:86-89, models/RNN_SPSS.py:107-118
 * ----------------------------------------------------------------------------------------------------------------
 * means f32 [B,T,W*D] (stream column w*D + d = window w of dimension d), variances f32 [W*D] (var_per_frame = 0, the global
 * variance both call sites pass) or [B,T,W*D] (var_per_frame = 1); seq_len int64 [B] or NULL; windows as parallel arrays:
 * win_l / win_u [W] ints (left / right extent, l + u <= 4), win_coeff [W][5] doubles (first l + u + 1 used).  Each utterance is
 * cut to its length and its first / last frame repeated `padding` times (:113-120, :156-157).  Per (b, d) the banded SPD system
 * sum_w W_w^T diag(1/var_w) W_w x = sum_w W_w^T (mean_w/var_w) is solved in float64 (LDL^T on the band); out [B,T,D] (f32, or
 * f64 if out_f64) holds the trajectory, zero past seq_len.  workspace: mg_mlpg_workspace_bytes(...) bytes. */
/* var_per_frame selects the layout of `variances`: 0 = global [W*D], MG_MLPG_VAR_ITEM = one row per utterance [B, W*D] (speaker-dependent
 * variances: the same values as the per-frame form fed that row T times, bit for bit), any other value = per frame [B,T,W*D]. */
#define MG_MLPG_VAR_ITEM 2
#define MG_MLPG_MAX_WINDOWS 4 /* n_windows <= this */
#define MG_MLPG_MAX_COEFF 5   /* the row length of win_coeff: l + u + 1 <= this */
size_t mg_mlpg_workspace_bytes(int B, int T, int D, int padding, int n_windows, const int* win_l, const int* win_u);
int mg_mlpg_f32(const float* means, const float* variances, int var_per_frame, const int64_t* seq_len, int B, int T, int D,
                int n_windows, const int* win_l, const int* win_u, const double* win_coeff, int padding, void* out, int out_f64,
                void* workspace, size_t workspace_bytes, void* stream);
/* The gradient of mg_mlpg_f32's trajectory with respect to `means` (trajectory training; the reference's host MLPG has none).
 * grad_out f32 [B,T,D] (frames past seq_len are never read); variances, var_per_frame, seq_len, windows and padding as in the
 * forward, with the same checks.  Per (b, d): P lambda = g~ (grad_out on the output rows, zero on the 2 x padding rows; the forward's
 * band and LDL^T, lambda float64 for all rows), then grad_means[b, f, w*D + d] = sum over the padded rows s that read frame f of
 * (1/var_w) (W_w lambda)[s], float64 in increasing s, rounded once: f32 [B,T,W*D], or f64 if out_f64; zero past seq_len.  The
 * variances get no gradient.  No atomics, deterministic.  workspace: mg_mlpg_workspace_bytes(...) bytes, as the forward. */
int mg_mlpg_grad_f32(const float* grad_out, const float* variances, int var_per_frame, const int64_t* seq_len, int B, int T, int D,
                     int n_windows, const int* win_l, const int* win_u, const double* win_coeff, int padding, void* grad_means,
                     int out_f64, void* workspace, size_t workspace_bytes, void* stream);
/* Both gradients of mg_mlpg_f32's trajectory, for PER-FRAME variances a model predicts: means and variances f32 [B,T,W*D] as given
 * to the forward (var_per_frame = 1; the other layouts are expanded by the caller), grad_out, seq_len, windows and padding as in
 * mg_mlpg_grad_f32, with the same checks.  Per (b, d) the forward's system P x~ = rhs and the adjoint P lambda = g~ are built and
 * solved side by side (one launch each of the band and the solve kernels over two sets of planes), then for every frame f, over
 * the padded rows s that read it in increasing s:
 *   grad_means[b,f,w*D+d]     = sum_s  (1/var_w) (W_w lambda)[s]                                  (bit-equal to mg_mlpg_grad_f32's)
 *   grad_variances[b,f,w*D+d] = sum_s -(1/var_w)^2 (W_w lambda)[s] (mean_w - (W_w x~)[s])
 * with 1/var and mean/var formed in float32 as in the forward and everything after that in float64, rounded once: f32 [B,T,W*D]
 * each, or f64 if out_f64; zero past seq_len, whose frames are read in no input.  No atomics, deterministic.
 * workspace: mg_mlpg_grad_mv_workspace_bytes(...) bytes = twice mg_mlpg_workspace_bytes(...). */
size_t mg_mlpg_grad_mv_workspace_bytes(int B, int T, int D, int padding, int n_windows, const int* win_l, const int* win_u);
int mg_mlpg_grad_mv_f32(const float* grad_out, const float* means, const float* variances, const int64_t* seq_len, int B, int T, int D,
                        int n_windows, const int* win_l, const int* win_u, const double* win_coeff, int padding, void* grad_means,
                        void* grad_variances, int out_f64, void* workspace, size_t workspace_bytes, void* stream);
/* Parameter generation under a global-variance prior (csrc/mlpg_gv.hip; Toda & Tokuda 2007 - the reference generates with plain MLPG
 * only).  means, variances, var_per_frame, seq_len, windows and padding as in mg_mlpg_f32, with the same checks; gv_mean and
 * gv_variance f32 [D], or [B,D] if gv_per_item (per-speaker statistics): mean and variance of the per-utterance variance of the static
 * feature.  Per (b, d), with P, rhs and the output rows O of mg_mlpg_f32, n = len, omega = 1/(W n) and v(x) the biased variance over O:
 *   minimise  omega (x^T P x / 2 - x^T rhs) + (gv_weight / 2) (v(x) - gv_mean)^2 / gv_variance
 * through its stationarity system (P + gamma E - (gamma/n) e e^T) x = rhs, gamma = 2 W kappa, kappa = gv_weight (v(x) - gv_mean) /
 * gv_variance: a bracketed scalar root search on kappa inside ONE launch, one thread per system, every evaluation an unpivoted banded
 * LDL^T of the shifted band with two right-hand sides and a rank-one correction, feasibility by inertia; at most max_iter (>= 3)
 * evaluations.  float32 1/var and mean/var as in mg_mlpg_f32, float64 after that.  out [B,T,D] f32, or f64 if out_f64, zero past
 * seq_len (whose input frames are never read).  info: NULL or f64 [B,D,4] = (kappa, final |h|, evaluations used, flag); flag 1 =
 * fallback, the output is the plain MLPG solution: len < 2, gv_weight = 0, gv_variance <= 0, or a search that ended with
 * |h| > 1e-6 (1 + |kappa|).  gv_weight = 0 runs mg_mlpg_f32 itself: the same bits.  No atomics, no host read, deterministic,
 * graph-capturable.  workspace: mg_mlpg_gv_workspace_bytes(...) bytes = twice mg_mlpg_workspace_bytes(...). */
size_t mg_mlpg_gv_workspace_bytes(int B, int T, int D, int padding, int n_windows, const int* win_l, const int* win_u);
int mg_mlpg_gv_f32(const float* means, const float* variances, int var_per_frame, const float* gv_mean, const float* gv_variance,
                   int gv_per_item, const int64_t* seq_len, int B, int T, int D, int n_windows, const int* win_l, const int* win_u,
                   const double* win_coeff, int padding, double gv_weight, int max_iter, void* out, int out_f64, double* info,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K5 mvn / minmax normalisers           reference: morgana/data.py:533-538, 579-590
 * ---------------------------------------------------------------------------------------------------------------- */
#define MG_NORM_MVN 0         /* (x - mean) / (std_dev + 1e-8)       p0 = mean, p1 = std_dev */
#define MG_DENORM_MVN 1       /* x * std_dev + mean                                             */
#define MG_NORM_MINMAX 2      /* (x - mmin) / scale,  scale = mmax - mmin, |scale| <= 1e-8 -> 1  p0 = mmin, p1 = mmax */
#define MG_DENORM_MINMAX 3    /* x * scale + mmin                                               */
/* x, out: n_rows x D f32 (any leading batch dims flattened); p0, p1: D f32.  In place (out == x) is allowed. */
/* Device-side collate of one sequence feature (reference: normalise on load, data.py:119-127; zero-padding collate_fn,
 * data.py:159-224; ToDeviceWrapper, :648-663).  packed f32 [sum_b len_b, D]: the batch's utterances back to back;
 * offsets int64 [B+1]: their first rows (offsets[B] = total).  raw_out / norm_out [B,T,D] (either may be NULL): the feature
 * zero padded to T frames and its normalised twin (kind MG_NORM_MVN or MG_NORM_MINMAX), zero in the pad frames. */
int mg_pad_normalise_f32(const float* packed, const int64_t* offsets, int B, int T, int D, const float* p0, const float* p1,
                         int kind, float* raw_out, float* norm_out, void* stream);
/* The same pass with the loader-side half of bf16 mode (reference: the float32 cast on load, data.py:127 - here the bf16 operand of
 * the first Linear is data preparation too): besides raw_out / norm_out (either may be NULL) it writes table_bf16
 * [B*T + extra_rows, ldb] bf16 = the normalised feature's rows (zero in pad frames), columns D .. ldb-1 zero, extra_rows zero rows
 * behind - what mg_cast_pad_bf16 would make of norm_out, without a second pass.  ldb >= D; kind MG_NORM_MVN or MG_NORM_MINMAX. */
int mg_pad_normalise_bf16_f32(const float* packed, const int64_t* offsets, int B, int T, int D, const float* p0, const float* p1, int kind,
                              float* raw_out, float* norm_out, uint16_t* table_bf16, int ldb, int extra_rows, void* stream);
int mg_normalise_f32(const float* x, float* out, const float* p0, const float* p1, int64_t n_rows, int D, int kind,
                     void* stream);
/* Per-item (speaker-dependent) normalisers    reference: morgana/data.py:388-530, :567-576, :619-628        csrc/items_norm.hip
 * p0, p1 are TABLES [S, D] f32 (one row per speaker) and item_row [B] int32 names the row of every batch item; the arithmetic per
 * element is that of mg_normalise_f32 with that row (bit for bit).  x, out [B, rows_per_item, D] f32, in place allowed; D <= 8192.
 * grad_mode != 0: x is a gradient and out = x * d out / d x of `kind` (the per-item, per-column scale; the offsets are not applied).
 * An item_row entry outside [0, S) is never used as an index: that item's output is NaN. */
int mg_normalise_items_f32(const float* x, float* out, const float* p0, const float* p1, const int32_t* item_row, int B,
                           int64_t rows_per_item, int D, int S, int kind, int grad_mode, void* stream);
/* mg_pad_normalise_f32 with tables [S, D] and one row per utterance: packed [sum_b len_b, D] + offsets [B+1] -> raw_out (may be
 * NULL) and norm_out [B,T,D], zero in the pad frames; kind MG_NORM_MVN or MG_NORM_MINMAX.  Bad item_row entry: NaN in that
 * utterance's valid frames of norm_out. */
int mg_pad_normalise_items_f32(const float* packed, const int64_t* offsets, int B, int T, int D, const float* p0, const float* p1,
                               const int32_t* item_row, int S, int kind, float* raw_out, float* norm_out, void* stream);
/* out[b, :] = table[item_row[b], :] (table [S, D], out [B, D] f32); NaN where item_row[b] is outside [0, S). */
int mg_item_rows_f32(const float* table, int S, int D, const int32_t* item_row, int B, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K2  Linear (+Sigmoid) stack             reference: nn.Linear / nn.Sigmoid in README.rst:65-73 run by
 *                                         SequentialWithRecurrent.forward, morgana/utils.py:401-418
 * f32 = exact fp32 (v_mfma_f32_32x32x2_f32), the 1e-4 parity mode.
 * bf16 = bf16 operands, fp32 accumulate (v_mfma_f32_32x32x16_bf16), the throughput mode.
 * ---------------------------------------------------------------------------------------------------------------- */
/* Y[m,:] = act( A[row(m),:] W^T + bias ).  A [*,K] (lda), rows NULL = identity else gather; W [N,K]; Y [M,N] (ldy). */
int mg_linear_fwd_f32(const float* A, int lda, const int32_t* rows, int64_t M, int K, const float* W,
                      const float* bias, int N, float* Y, int ldy, int act, void* stream);
/* dX = (dY W) [* H (1-H)].  dY [M,N]; W [N,K]; H NULL or [M,K] = the sigmoid OUTPUT feeding this layer; dX [M,K]. */
int mg_linear_dgrad_f32(const float* dY, int64_t M, int N, const float* W, int K, const float* H, float* dX,
                        void* stream);
/* dX = (dY W) * f'(H), H [M,K] the OUTPUT of activation `act` feeding this layer: f' = H (1-H) (MG_ACT_SIGMOID), 1 - H^2
 * (MG_ACT_TANH), H > 0 (MG_ACT_RELU); MG_ACT_NONE (H may be NULL): dX = dY W.  mg_linear_dgrad_f32 is this with MG_ACT_SIGMOID.
 * What it replaces: autograd's backward of torch.nn.Tanh / ReLU + nn.Linear inside morgana/utils.py:401-418. */
int mg_linear_dgrad_act_f32(const float* dY, int64_t M, int N, const float* W, int K, const float* H, int act, float* dX,
                            void* stream);
/* dW[n,k] (+)= sum_m dY[m,n] A[row(m),k];  db[n] (+)= sum_m dY[m,n].  accumulate != 0 adds into dW/db.
 * workspace: mg_linear_wgrad_workspace_bytes(M,N,K).  Deterministic (split-M slabs + ordered reduce). */
size_t mg_linear_wgrad_workspace_bytes(int64_t M, int N, int K);
int mg_linear_wgrad_f32(const float* dY, const float* A, int lda, const int32_t* rows, int64_t M, int N, int K,
                        float* dW, float* db, int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* Phone-rate first layer (csrc/phone_rate.hip): Linear commutes with upsample_to_repetitions' row repetition (reference:
 * morgana/utils.py:175-228 feeding README.rst:65-73 / morgana/utils.py:401-418), so the first layer's product runs once per
 * phone and these kernels move between phone rate and frame rate.
 *  mg_segment_bounds  seg_start / seg_end int32 [R]: the run of frames f with rows[f] == r (0, 0 if none).  rows int32 [M] as
 *                     mg_upsample_index writes them (b*P + phone, -1 = padding); the frames of a row must be consecutive.
 *                     rows_mapped (optional, int32 [M]): rows with -1 replaced by pad_row (the table row of a zero input).
 *  mg_segment_sum     out[r, :] = sum of G[f, :] over the frames of row r (fp32 accumulation, frame order), r < R; rows
 *                     R..R+extra-1 of out take the frames with rows[f] < 0 (those of the j-th of `extra` equal shares of the frame axis go to row R + j).  G, out bf16
 *                     (g_bf16) or f32. */
/*  mg_phone_target_stats  what the masked MSE (morgana/losses.py:29-51) needs per table row when every frame of a row shares one
 *                     prediction: weight[r] = sum of the frame weights [t < n_b] / (n_b B) of the row's frames, ybar[r] = their weighted
 *                     mean target, loss_const = sum_r sum_f w_f (y_f - ybar[r])^2.  Then
 *                     loss = sum_r weight[r] (pred[r] - ybar[r])^2 + loss_const  exactly, with the same gradient (mg_f0_tail_rows_bf16).
 *                     target f32 [B*T]; ybar, weight f32 [R + extra]; rows R.. take the padding frames. */
/*  mg_f0_tail_rows_f32  the README F0Model's tail (Linear(128, 32) -> Sigmoid -> Linear(32, 1), /root/reference/README.rst:65-73) with the
 *                     masked MSE in its per-phone form, forward AND backward, exact fp32 (v_mfma_f32_16x16x4_f32), ONE launch + the ordered
 *                     slab reduce - the fp32 / bf16x3 modes' counterpart of mg_f0_tail_rows_bf16 (csrc/tail_f32.hip).  Z2 f32 [M, ldz]: the
 *                     128-wide layer's PRE-activations (h2 = sigmoid(Z2) is taken here); ybar, weight f32 [M] as mg_phone_front leaves them -
 *                     or weight == NULL: the rows are the B x T frames, ybar = the targets [B * T], and the kernel forms the masked MSE's own
 *                     weights [t < n_b] / (n_b B) from seq_len (NULL = all T; an utterance without frames gives NaN, as the reference's mean).
 *                     pred f32 [M]; dZ2 f32 [M, lddz] = d loss / d Z2; grads_out f32 [4164] = dW3 [32 x 128] | db3 [32] | dW4 [32] | db4 |
 *                     loss (= sum_m weight (pred - ybar)^2, the constant term excluded) | 2 unused. */
size_t mg_f0_tail_rows_f32_workspace_bytes(int64_t M);
int mg_f0_tail_rows_f32(const float* Z2, int ldz, const float* W3, const float* b3, const float* W4, const float* b4, const float* ybar,
                        const float* weight, const int64_t* seq_len, int B, int T, int64_t M, float* pred, float* dZ2, int lddz,
                        float* grads_out, void* workspace, size_t workspace_bytes, void* stream);
/*  mg_phone_mse_rows_f32  the masked MSE of a ONE-column prediction that is constant over each table row's frames, exact-fp32 modes:
 *                     loss[0] = sum_r weight[r] (pred[r * ldp] - ybar[r])^2 over the R + extra rows of mg_phone_target_stats (its constant
 *                     term is added by mg_phone_loss_const_add / mg_expand_column_loss_f32), dpred[r] = 2 weight[r] (pred[r * ldp] - ybar[r]).
 *                     One workgroup, fixed summation order (double partial sums). */
int mg_phone_mse_rows_f32(const float* pred, int ldp, const float* ybar, const float* weight, int n_rows, float* loss, float* dpred,
                          void* stream);
/*  mg_expand_column_f32  out[f] = table[rows[f]] for a one-column f32 table (the per-phone prediction repeated to frames); rows >= 0. */
int mg_expand_column_f32(const float* table, const int32_t* rows, int64_t M, float* out, void* stream);
/* ... and mg_phone_loss_const_add in the same launch (stats_workspace as left by mg_phone_target_stats). */
int mg_expand_column_loss_f32(const float* table, const int32_t* rows, int64_t M, float* out, const void* stats_workspace, int R,
                              int extra, float* loss, void* stream);
/* ... and the ordered reduce of the fused tail's slabs in the same launch: dst[0 .. n) = sum of the S slabs (stride floats apart; the
 * arithmetic of the library's slab reduce), dst[n - 1] - the loss, stored behind the gradients - additionally receives the loss's
 * constant term.  Pairs with mg_f0_l2tail_rows_slabs_bf16. */
int mg_expand_column_reduce_f32(const float* table, const int32_t* rows, int64_t M, float* out, const void* stats_workspace, int R,
                                int extra, const float* slab, int64_t n, int64_t stride, int S, float* dst, void* stream);
size_t mg_phone_target_stats_workspace_bytes(int R, int extra);
/* loss_const may be NULL: then mg_phone_loss_const_add(workspace, R, extra, loss) adds the constant to a loss in place later on
 * (the workspace must be left untouched in between).  mg_phone_target_stats and mg_phone_front refuse extra = 0 (MG_EINVAL): the
 * padding frames' loss terms live in the extra rows, and without one they would be lost silently. */
int mg_phone_loss_const_add(const void* workspace, int R, int extra, float* loss, void* stream);
int mg_phone_target_stats(const float* target, const int32_t* rows, int64_t M, const int32_t* seg_start, const int32_t* seg_end,
                          const int64_t* seq_len, int B, int T, int R, int extra, float* ybar, float* weight, float* loss_const,
                          void* workspace, size_t workspace_bytes, void* stream);
/* The front of the phone-rate step in ONE launch: mg_upsample_index_maps (upsample_to_repetitions' frame map, morgana/utils.py:175-228)
 * and mg_phone_target_stats (morgana/losses.py:29-51 per phone row) - a phone's statistics read only the frame run its own utterance's
 * duration scan gives, so one workgroup per utterance does both (csrc/phone_front.h).  dur int64 [B, P]; target f32 [B*T] (T = the
 * frame axis the map is cut to); R = B*P phone rows + `extra` rows for the padding frames.  rows32 / rows_mapped int32 [B*T],
 * seg_start / seg_end int32 [R], ybar / weight f32 [R + extra]: bit for bit what the two launches write.  workspace
 * (mg_phone_target_stats_workspace_bytes(R, extra)): partial sums of the loss's constant term for mg_phone_loss_const_add and the
 * mg_expand_column_* launches, grouped per utterance (so the constant may differ from the two-launch one in its last bits).
 * MG_EINVAL where the form does not apply (fewer than ~16 phones per utterance; extra rows that each span many utterances). */
int mg_phone_front(const int64_t* dur, int B, int P, int T, const float* target, const int64_t* seq_len, int extra, int32_t* rows32,
                   int32_t* rows_mapped, int pad_row, int32_t* seg_start, int32_t* seg_end, float* ybar, float* weight, void* workspace,
                   size_t workspace_bytes, void* stream);
/* mg_phone_front and mg_linear_fwd_bf16(A, rows = NULL, ... bf16 output) of the phone table's first layer (README.rst:66-67), which
 * reads nothing the front writes: ONE grid where the GEMM is the persistent 256-wide form and leaves at least 32 CUs without a tile
 * (C2: 168 tiles) - the front's jobs run on those CUs - otherwise the two launches.  Same results either way. */
int mg_phone_front_linear_fwd_bf16(const int64_t* dur, int B, int P, int T, const float* target, const int64_t* seq_len, int extra,
                                   int32_t* rows32, int32_t* rows_mapped, int pad_row, int32_t* seg_start, int32_t* seg_end, float* ybar,
                                   float* weight, void* workspace, size_t workspace_bytes, const uint16_t* A, int lda, int64_t M, int K,
                                   const uint16_t* W, int ldw, const float* bias, int N, uint16_t* Y, int ldy, int act, void* stream);
int mg_segment_bounds(const int32_t* rows, int64_t M, int R, int32_t* seg_start, int32_t* seg_end, int32_t* rows_mapped,
                      int pad_row, void* stream);
int mg_segment_sum(const void* G, int ldg, int g_bf16, const int32_t* rows, int64_t M, const int32_t* seg_start,
                   const int32_t* seg_end, int R, int extra, int N, void* out, int ldo, void* stream);
/* mg_segment_sum (bf16) and, in the same pass over G, the weight gradient of C <= 16 per-frame input features (the frame counters behind
 * the repeated phone rows, /root/reference/models/RNN_SPSS.py:76-81): partial sums  slab[b][c][n] = sum over workgroup b's frames of
 * G[f, n] feat[f, c]  into `slabs` (mg_segment_sum_feat_workspace_bytes(C, ldo) bytes; must stay untouched until the reduce);
 * mg_feat_wgrad_reduce then writes dW[n, col0 + c] (+)= sum_b slab[b][c][n].  feat f32 [M, C].  Deterministic. */
size_t mg_segment_sum_feat_workspace_bytes(int C, int ldo);
int mg_segment_sum_feat_bf16(const uint16_t* G, int ldg, const int32_t* rows, int64_t M, const int32_t* seg_start, const int32_t* seg_end,
                             int R, int extra, int N, uint16_t* out, int ldo, const float* feat, int C, void* slabs, size_t slabs_bytes,
                             void* stream);
int mg_feat_wgrad_reduce(const void* slabs, int C, int ldo, int N, float* dW, int ldw, int col0, int accumulate, void* stream);
/* The first Linear of a model whose input is cat(upsample_to_repetitions(lab, durations), frame counters)
 * (/root/reference/models/RNN_SPSS.py:76-81, models/f0_test_model.py:78-79), with W = [W_lab | W_cnt]: the lab part runs once per phone
 * (P = table W_lab^T through mg_linear_fwd_bf16, f32 output, no bias) and this kernel finishes the layer per frame,
 *   Y[f, n] = act(P[rows[f], n] + sum_c feat[f, c] W[n, col0 + c] + bias[n]),   n < N; Y's padding columns [N, ldy) zero.
 * P f32 [table rows, ldp] (ldp >= N rounded up to 8); rows int32 [M], every entry a row of P (-1 already mapped to a zero-input
 * row); feat f32 [M, C], 1 <= C <= 16; W f32 [N, ldw] with the counters' weights in columns col0 .. col0 + C; Y [M, ldy] bf16, or
 * f32 with y_f32 != 0 (the layer's output leaves the fused run). */
int mg_phone_concat_layer_bf16(const float* P, int ldp, const int32_t* rows, int64_t M, const float* feat, int C, const float* W, int ldw,
                               int col0, const float* bias, int N, int act, void* Y, int ldy, int y_f32, void* stream);

/* bf16 variants: A, W, H, Y are bf16; K and N of the bf16 buffers are padded: lda/ldw/ldy multiples of 8 elements,
 * padding columns must be zero (mg_cast_pad_bf16 / mg_gather_rows_bf16 produce such buffers).  bias, dW, db f32. */
/* Y is bf16 [M,ldy] (y_f32 == 0) or f32 [M,ldy] (y_f32 != 0); ldy a multiple of 8; columns N..ldy-1 are written as 0. */
int mg_linear_fwd_bf16(const uint16_t* A, int lda, const int32_t* rows, int64_t M, int K, const uint16_t* W, int ldw,
                       const float* bias, int N, void* Y, int ldy, int y_f32, int act, void* stream);
/* WT = W^T as bf16 [K,N] (ldwt). */
int mg_linear_dgrad_bf16(const uint16_t* dY, int lddy, int64_t M, int N, const uint16_t* WT, int ldwt, int K,
                         const uint16_t* H, int ldh, void* dX, int lddx, int dx_f32, void* stream);
/* The same for H the output of `act` (see mg_linear_dgrad_act_f32); mg_linear_dgrad_bf16 is this with MG_ACT_SIGMOID. */
int mg_linear_dgrad_act_bf16(const uint16_t* dY, int lddy, int64_t M, int N, const uint16_t* WT, int ldwt, int K,
                             const uint16_t* H, int ldh, int act, void* dX, int lddx, int dx_f32, void* stream);
/* The same with H read from a table: frame m's sigmoid output is H[h_rows[m]] (phone-rate first layer; h_rows >= 0).  Needs the
 * wide-tile shape (M >= 2048, K % 128 == 0, lddy and ldwt multiples of 64); MG_EINVAL otherwise. */
int mg_linear_dgrad_gathered_bf16(const uint16_t* dY, int lddy, int64_t M, int N, const uint16_t* WT, int ldwt, int K,
                                  const uint16_t* H, int ldh, const int32_t* h_rows, void* dX, int lddx, int dx_f32, void* stream);
int mg_linear_wgrad_bf16(const uint16_t* dY, int lddy, const uint16_t* A, int lda, const int32_t* rows, int64_t M,
                         int N, int K, float* dW, float* db, int accumulate, void* workspace, size_t workspace_bytes,
                         void* stream);

/* mg_linear_wgrad_bf16 with both operands gathered: dW = sum_{m < M} dY[dy_rows[m]]^T A[rows[m]] (rows NULL: A[dy_rows[m]]); M counts the
 * index pairs.  What it replaces: the weight gradients autograd forms for nn.GRU / nn.LSTM on a PackedSequence
 * (morgana/utils.py:366-385: pack_padded_sequence in front of the layer, pad_packed_sequence behind it) - here the recurrences keep
 * padded (B, T) arrays and this product visits the sum_b T_b valid frames only.  Wide-tile shapes with lda == 512 (384 < K <= 512,
 * N % 128 == 0, M >= 4096, not the half-width plan): MG_EINVAL otherwise, the caller then multiplies the padded rows.  workspace:
 * mg_linear_wgrad_workspace_bytes(M, N, K). */
int mg_linear_wgrad_rows_bf16(const uint16_t* dY, int lddy, const int32_t* dy_rows, const uint16_t* A, int lda, const int32_t* rows, int64_t M,
                              int N, int K, float* dW, float* db, int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* mg_linear_wgrad_bf16 without its reduce launch: the split-M partial results stay in `workspace` as *n_slabs slabs of *stride floats,
 * slab s = [N*K weight partials | N bias partials], for a consumer that sums them itself (mg_adam_step_plan_f32).  Only the wide-tile
 * plan has this form: returns MG_EINVAL for shapes mg_linear_wgrad_bf16 would run on its 128 x 128 kernels (call that instead). */
int mg_linear_wgrad_slabs_bf16(const uint16_t* dY, int lddy, const uint16_t* A, int lda, const int32_t* rows, int64_t M, int N, int K,
                               void* workspace, size_t workspace_bytes, int* n_slabs, int64_t* stride, void* stream);
/* mg_linear_wgrad_slabs_bf16 (no gather) and mg_linear_dgrad_bf16 of ONE layer whose input A bf16 [M, lda] is the output of the Sigmoid
 * below it (reference: the autograd backward of nn.Linear + nn.Sigmoid inside F0Model, README.rst (the nn.Sequential of Linear + Sigmoid layers)): the slabs of
 * dW = dY^T A, db, and dX bf16 [M, lddx] = (dY W) * A (1 - A), WT = W^T bf16 [K, ldwt].  The two products are independent; for the
 * phone-rate shape of the README model (N = 128, K = lda = lddx = 512, the tiles of both within one wave of workgroups) they run as
 * ONE grid, with the split count cut to what the dgrad tiles leave free per XCD (*n_slabs says how many); other shapes run the two
 * launches.  Needs a wide-tile weight-gradient shape (as mg_linear_wgrad_slabs_bf16: MG_EINVAL otherwise); workspace as there. */
int mg_linear_wgrad_dgrad_bf16(const uint16_t* dY, int lddy, const uint16_t* A, int lda, int64_t M, int N, int K, const uint16_t* WT, int ldwt,
                               uint16_t* dX, int lddx, void* workspace, size_t workspace_bytes, int* n_slabs, int64_t* stride, void* stream);
/* mg_linear_wgrad_dgrad_bf16 with mg_expand_column_reduce_f32 (K1 section) riding at the end of the same grid: the phone-rate step's
 * repeated prediction (out[f] = table[rows[f]], `frames` of them) and the ordered sum of the fused tail's slabs into tail_dst (+ the
 * loss's constant term from stats_workspace / R / extra) are read by nothing before the update, so a step captured as a HIP graph
 * lets them start on the CUs the dgrad tiles free first instead of paying a launch of their own.  Arguments as the two entry points;
 * the same results bit for bit; shapes the one-grid form does not take run the separate launches.  loss_only != 0: of the slab sum
 * only the last 16-element chunk - the one that holds the loss at tail_dst[tail_n - 1] - is formed (the caller's update kernel sums
 * the slabs of the gradients itself: mg_adam_step_plan_f32 with the tail's slabs as a source). */
int mg_linear_wgrad_dgrad_expand_bf16(const uint16_t* dY, int lddy, const uint16_t* A, int lda, int64_t M, int N, int K, const uint16_t* WT,
                                      int ldwt, uint16_t* dX, int lddx, void* workspace, size_t workspace_bytes, int* n_slabs, int64_t* stride,
                                      const float* table, const int32_t* rows, int64_t frames, float* out, const void* stats_workspace, int R,
                                      int extra, const float* tail_slab, int64_t tail_n, int64_t tail_stride, int tail_S, float* tail_dst,
                                      int loss_only, void* stream);
/* dst[0 .. count) (+)= the ordered sum of n_slabs slabs, `stride` floats apart (the reduce launch of mg_linear_wgrad_bf16, bit for bit),
 * for a caller that took slabs from mg_linear_wgrad_slabs_bf16 / mg_linear_wgrad_dgrad_bf16 and needs the finished gradient before the
 * update (a data-parallel rank: its all-reduce comes first).  With db stored right behind dW (count = N*K + N) one launch does both. */
int mg_slab_reduce_f32(const float* slab, int n_slabs, int64_t stride, int64_t count, float* dst, int accumulate, void* stream);
/* Fused backward of Linear(K -> N) + Sigmoid feeding Linear(N -> N2): dW, db of the FIRST layer straight from dZ2, the
 * pre-activation gradient of the second one, without materialising dZ1 = (dZ2 W2) * H1 (1 - H1):
 *   dZ2 bf16 [M, lddz] (N2 = 128 columns); W2T = W2^T bf16 [N, ldwt]; H1 bf16 [M, ldh] (sigmoid outputs, N % 128 == 0);
 *   A bf16 [*, lda = 640] with `rows` (the layer-1 input, gathered), 512 < K <= 608.
 * dW f32 [N, K], db f32 [N] (accumulate != 0 adds).  workspace: mg_linear_bwd_fused_workspace_bytes(M, N, K). */
size_t mg_linear_bwd_fused_workspace_bytes(int64_t M, int N, int K);
int mg_linear_bwd_fused_bf16(const uint16_t* dZ2, int lddz, int N2, const uint16_t* W2T, int ldwt, const uint16_t* H1, int ldh,
                             const uint16_t* A, int lda, const int32_t* rows, int64_t M, int N, int K, float* dW, float* db,
                             int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* The same without its reduce launch: the split-M partial results stay in `workspace` as *n_slabs slabs of *stride floats, slab s =
 * [N*K weight partials | N bias partials] (the layout of mg_linear_wgrad_slabs_bf16), for mg_adam_step_plan_f32 to sum. */
int mg_linear_bwd_fused_slabs_bf16(const uint16_t* dZ2, int lddz, int N2, const uint16_t* W2T, int ldwt, const uint16_t* H1, int ldh,
                                   const uint16_t* A, int lda, const int32_t* rows, int64_t M, int N, int K, void* workspace,
                                   size_t workspace_bytes, int* n_slabs, int64_t* stride, void* stream);
/* The fused backward WITH the second layer's weight gradient: one launch leaves the split-M slabs of dW1 | db1 (as
 * mg_linear_bwd_fused_slabs_bf16) AND of dW2 = dZ2^T H1 | db2 = column sums of dZ2 - the stand-alone weight-gradient launch of the
 * N -> 128 layer, which re-read H1 and dZ2 from HBM, goes (reference: autograd of README.rst:65-73, the mm + sum of layer 2's
 * backward).  Needs the row map (rows != NULL).  workspace (floats): [*n_slabs x *stride1] first-layer slabs as above, then from
 * float *offset2 on [*n_slabs x *stride2] second-layer slabs, each [128 x N weight partials | 128 bias partials]; the caller sums
 * them in order (mg_slab_reduce_f32 or the update kernel's plan). */
size_t mg_linear_bwd_fused2_workspace_bytes(int64_t M, int N, int K);
int mg_linear_bwd_fused2_slabs_bf16(const uint16_t* dZ2, int lddz, int N2, const uint16_t* W2T, int ldwt, const uint16_t* H1, int ldh,
                                    const uint16_t* A, int lda, const int32_t* rows, int64_t M, int N, int K, void* workspace,
                                    size_t workspace_bytes, int* n_slabs, int64_t* stride1, int64_t* offset2, int64_t* stride2, void* stream);

/* dst[r, 0:cols] = bf16(src[r, 0:cols]), dst[r, cols:ldd] = 0.  src f32 [rows, cols] (lds). */
int mg_cast_pad_bf16(const float* src, int lds, uint16_t* dst, int ldd, int64_t rows, int cols, void* stream);
/* dst[c, 0:rows] = bf16(src[r, c]) transposed, dst [cols, ldd], zero padded. */
int mg_cast_transpose_bf16(const float* src, int lds, uint16_t* dst, int ldd, int rows, int cols, void* stream);
/* Batched weight refresh (one launch for a whole layer stack): for each descriptor, dst = bf16(src) [rows, ldd] and / or
 * dst_t = bf16(src^T) [cols, ldt], zero padded; either output may be NULL.  `descs` is a HOST array, count <= MG_CAST_MAX. */
#define MG_CAST_MAX 16
typedef struct {
    const float* src; /* device, fp32 [rows, cols], contiguous */
    int rows, cols;
    uint16_t* dst;    /* device bf16 [rows, ldd] or NULL */
    int ldd;
    uint16_t* dst_t;  /* device bf16 [cols, ldt] or NULL */
    int ldt;
} mg_cast_desc;
int mg_cast_params_bf16(const mg_cast_desc* descs, int count, void* stream);
/* Up to MG_COPY_MAX device-to-device copies as ONE launch (dst[i][0 .. bytes[i]) = src[i][...], buffers 16-byte aligned or any size
 * handled bytewise at the ends): a captured training step replayed on a NEW batch takes the batch's tensors into its static buffers
 * this way - the feature dict of /root/reference/morgana/data.py:648-663 is five tensors at BASELINE config C2, five copy launches of
 * 3-15 us each where one does (graphs.GraphedTrainStep.load).  `descs` is a HOST array. */
#define MG_COPY_MAX 16
typedef struct {
    const void* src;
    void* dst;
    int64_t bytes;
} mg_copy_desc;
int mg_copy_many(const mg_copy_desc* descs, int count, void* stream);
/* HOST half of the loader (no device work): `count` utterance arrays (srcs[i], bytes[i]) laid back to back at dst - the pinned staging
 * buffer one H2D copy then takes across PCIe - by `threads` host threads (1..64).  Replaces the np / torch concatenation in front of
 * /root/reference/morgana/data.py:159-224 (collate_fn's per-utterance pad copies; there the padding happens on the host, here on the
 * device: mg_pad_normalise_f32).  dst_bytes = capacity of dst; MG_EINVAL when the pieces do not fit. */
int mg_host_pack(const void* const* srcs, const int64_t* bytes, int count, void* dst, int64_t dst_bytes, int threads);
/* Operand splits of precision mode 'bf16x3' (split-bf16: hi = bf16(x), lo = bf16(x - hi); x w ~= hi hi + hi lo + lo hi as ONE bf16
 * GEMM over a contraction index three times as long; csrc/split3.hip).  The reference computes these products in fp32
 * (morgana/experiment_builder.py:262-263: no autocast, morgana/data.py:127: float32 features); this mode reproduces them to ~1e-5
 * at three bf16 MFMA products each.  For each descriptor: dst bf16 [rows, 3 ldp] = three planes of ldp columns (zero padded):
 * order 0 -> [hi | hi | lo] (the activation side of a product), order 1 -> [hi | lo | hi] (the weight side); transpose != 0 -> the
 * planes hold the split of src^T: dst [cols, 3 ldp] with ldp >= rows.  order 2 (not transposed) -> dst bf16 [2, rows, ldp]: the hi
 * plane, then the lo plane, each a matrix of its own (the operands of a weight gradient, which contracts over the rows: three
 * accumulating launches of mg_linear_wgrad_bf16 on plane pairs).  order 3 / 4 (not transposed) -> dst bf16 [3, rows, ldp]: three
 * row-stacked planes [hi ; hi ; lo] / [hi ; lo ; hi] - the same three products as ONE mg_linear_wgrad_bf16 launch over 3 rows rows
 * (dY = the order-3 planes, A = the order-4 planes); its bias gradient comes from `colsum`.  `descs` is a HOST array, count <= MG_SPLIT3_MAX. */
#define MG_SPLIT3_MAX 16
typedef struct {
    const float* src; /* device, fp32 [rows, cols], row stride lds */
    int64_t rows;
    int cols, lds;
    uint16_t* dst;    /* device, bf16, 16-byte aligned: [rows, 3 ldp], or [cols, 3 ldp] when transposed */
    int ldp;          /* columns per plane: multiple of 8, >= cols (>= rows when transposed) */
    int order;        /* 0: hi | hi | lo;  1: hi | lo | hi;  2: two planes [hi ; lo] of [plane_rows, ldp];  3: [hi ; hi ; lo];  4: [hi ; lo ; hi];
                       * 5: PAIR PLANES hi | lo, dst bf16 [rows, 2 ldp] ([cols, 2 ldp] with transpose): the operands of the mg_*_x3 entry points */
    int transpose;
    int64_t plane_rows; /* orders 2-4: rows of one plane in dst (>= rows; the caller owns the rows behind the split, e.g. zeros); 0 = rows */
    const float* sig; /* optional (not transposed): fp32 [rows, cols] (ldsig) sigmoid outputs s - the split is taken of src * s * (1 - s):
                       * the sigmoid gradient of autograd (README.rst:65-73's nn.Sigmoid) fused into the split of the gradient */
    int ldsig;
    float* colsum;    /* optional (not transposed): f32 [colsum_blocks, ldp] - workgroup b's partial column sums of the (sigmoid-gradient-fused)
                       * source values over its share of the rows; summed in slab order they are the bias gradient of the layer, exact */
    int colsum_blocks;
} mg_split3_desc;
int mg_split3_bf16(const mg_split3_desc* descs, int count, void* stream);

/* ---- The FUSED step of precision mode 'bf16x3' on PAIR PLANES -------------------------------------------------------------------
 * Reference arithmetic is fp32 end to end (/root/reference/morgana/experiment_builder.py:262-263, /root/reference/morgana/data.py:127);
 * x = hi + lo with hi = bf16(x), lo = bf16(x - hi), x w ~= hi hi + hi lo + lo hi, every product exact in the fp32 accumulator of a bf16
 * MFMA.  A pair-plane operand is bf16 [rows, ld] with ld = 2 ldp: columns [0, ldp) = hi, [ldp, 2 ldp) = lo (ldp a multiple of 64,
 * padding columns zero) - mg_split3_bf16 order 5 writes one, the update kernel keeps the weights' pairs current (mg_adam_shadow.pair),
 * and the entry points below write their outputs split in their epilogues, so a training step of the README F0Model at phone rate
 * (/root/reference/README.rst:65-73 behind /root/reference/morgana/utils.py:175-228) launches no split pass and no cast.  The tile programs
 * are those of bf16 mode with the contraction run three times over the plane pairs (csrc/gemm_bf16_big.hip, "pair planes").
 *
 *  mg_phone_front_linear_fwd_x3   mg_phone_front + Y = split(act(A W^T + b)): A [M, lda = 2 pa] the phone table's pair, W [N, ldw = 2 pw]
 *                     (pa, pw >= K rounded up to 64; N a multiple of 256), Y bf16 [M, ldy = 2 N] the activation's pair.  One grid where
 *                     the GEMM leaves CUs idle (as mg_phone_front_linear_fwd_bf16), else two launches.  dur == NULL: the GEMM alone.
 *  mg_linear_fwd_x3_f32  Y f32 [M, N] = act(A W^T + b) from pair-plane operands (N a multiple of 128, ldy == N).  parts == 3 (act none):
 *                     Y is [3, M, N] - the partial sums of the three products hi hi (+ b), hi lo, lo hi from three sets of workgroups
 *                     (a few-tile GEMM fills the chip with chains a third as long); the consumer adds them (mg_f0_tail_rows_x3 z_parts).
 *  mg_f0_tail_rows_x3  mg_f0_tail_rows_f32 with Z2 f32 [z_parts, M, ldz] given as z_parts (1 or 3) partial sums to add, dZ2 as a pair
 *                     [M, lddz >= 256] and the 128-wide layer's bias gradient (the column sums of
 *                     the fp32 dZ2) in front of the tail's gradients: slabs of MG_F0_TAIL_X3_SLAB floats = db2 [128] | dW3 [32 x 128] |
 *                     db3 [32] | dW4 [32] | db4 | loss | 2 unused, *n_slabs of them *stride floats apart in `workspace`
 *                     (mg_f0_tail_rows_x3_workspace_bytes(M)), reduced into grads_out [MG_F0_TAIL_X3_SLAB] when that is not NULL.
 *  mg_f0_l2tail_x3    mg_linear_fwd_x3_f32 of the 512 -> 128 layer AND mg_f0_tail_rows_x3 as ONE launch (csrc/l2tail_x3.hip): a workgroup
 *                     owns <= 96 consecutive rows, streams its rows of H1 (pair [M, 1024], whole lines, once) and W2's pair [128, 1024]
 *                     through LDS, keeps Z2 = H1 W2^T + b2 on chip and runs the exact-fp32 tail on it.  Outputs and slab layout as
 *                     mg_f0_tail_rows_x3 (workspace mg_f0_l2tail_x3_workspace_bytes(M)).
 *  mg_linear_wgrad_dgrad_x3  the 512 -> 128 layer's backward as ONE grid: dW slabs (N K floats used of each `*stride`, no bias sums) from
 *                     dY pair [M, lddy = 2 * 128] and A = H pair [M, lda = 2 * 512], and dX pair [M, lddx = 2 K] = split((dY W) * H (1 - H)),
 *                     H = hi + lo; `colsum` f32 receives *n_colsum slabs of K floats whose ordered sum is the column sum of the fp32 dX
 *                     (the bias gradient of the layer below; 2 ceil(M / 256) slabs: mg_linear_wgrad_dgrad_x3_colsum_floats(M, K) floats).
 *                     WT [K, ldwt = 2 * 128] = the pair of W^T.  N == 128, K == 512 only (MG_EINVAL otherwise).
 *  mg_linear_wgrad_slabs_x3  mg_linear_wgrad_slabs_bf16 on pairs: dY [M, lddy = 2 pn], A [M, lda = 2 pk], slabs of N K floats (+ N unused,
 *                     the bf16 layout's stride), no bias sums; the wide-tile shapes only (pk 640 or 512). */
#define MG_F0_TAIL_X3_SLAB 4292
int mg_phone_front_linear_fwd_x3(const int64_t* dur, int B, int P, int T, const float* target, const int64_t* seq_len, int extra,
                                 int32_t* rows32, int32_t* rows_mapped, int pad_row, int32_t* seg_start, int32_t* seg_end, float* ybar,
                                 float* weight, void* workspace, size_t workspace_bytes, const uint16_t* A, int lda, int64_t M, int K,
                                 const uint16_t* W, int ldw, const float* bias, int N, uint16_t* Y, int ldy, int act, void* stream);
int mg_linear_fwd_x3_f32(const uint16_t* A, int lda, int64_t M, int K, const uint16_t* W, int ldw, const float* bias, int N, float* Y,
                         int ldy, int act, int parts, void* stream);
size_t mg_f0_tail_rows_x3_workspace_bytes(int64_t M);
int mg_f0_tail_rows_x3(const float* Z2, int ldz, int z_parts, const float* W3, const float* b3, const float* W4, const float* b4,
                       const float* ybar, const float* weight, int64_t M, float* pred, uint16_t* dZ2, int lddz, float* grads_out,
                       void* workspace, size_t workspace_bytes, int* n_slabs, int64_t* stride, void* stream);
size_t mg_f0_l2tail_x3_workspace_bytes(int64_t M);
int mg_f0_l2tail_x3(const uint16_t* H1, int ldh, const uint16_t* W2, int ldw, const float* b2, const float* W3, const float* b3,
                    const float* W4, const float* b4, const float* ybar, const float* weight, int64_t M, float* pred, uint16_t* dZ2,
                    int lddz, float* grads_out, void* workspace, size_t workspace_bytes, int* n_slabs, int64_t* stride, void* stream);
size_t mg_linear_wgrad_dgrad_x3_colsum_floats(int64_t M, int K);
int mg_linear_wgrad_dgrad_x3(const uint16_t* dY, int lddy, const uint16_t* A, int lda, int64_t M, int N, int K, const uint16_t* WT, int ldwt,
                             uint16_t* dX, int lddx, void* workspace, size_t workspace_bytes, int* n_slabs, int64_t* stride, float* colsum,
                             size_t colsum_floats, int* n_colsum, void* stream);
int mg_linear_wgrad_slabs_x3(const uint16_t* dY, int lddy, const uint16_t* A, int lda, int64_t M, int N, int K, void* workspace,
                             size_t workspace_bytes, int* n_slabs, int64_t* stride, void* stream);
/* Active dropout (nn.Dropout(p) of the shipped models in training mode: /root/reference/models/RNN_SPSS.py:19,34,40,
 * /root/reference/models/f0_test_model.py:22,31-43; torch.nn.functional.dropout semantics: y = x * keep / (1 - p), keep ~ Bernoulli(1 - p)
 * per element).  The mask is a function of (seed, site, *counter, element index) through Philox4x32-10 and is never stored: the
 * backward pass calls the same entry on the gradient with the same four numbers.  x, y: n elements, fp32 (bf16 = 0) or bf16 (bf16 = 1),
 * y may be x.  counter: DEVICE uint64 (NULL = 0) - the step counter this call draws from; mg_dropout_advance(state, used) copies
 * *state to *used (the word a call's backward keeps) and increments *state, in stream order, so that a replayed HIP graph draws a new
 * mask every replay.  Bit parity with torch's mask stream is not attempted (its Philox offsets depend on its launch geometry). */
int mg_dropout(const void* x, void* y, int64_t n, int bf16, float p, uint64_t seed, uint32_t site, const uint64_t* counter, void* stream);
int mg_dropout_advance(uint64_t* state, uint64_t* used, void* stream);
/* Host-only: one Philox4x32-10 block (the generator mg_dropout draws from), for known-answer tests. */
void mg_philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);
/* Latent-conditioned models (BaseVAE, reference base_models.py:288-381; csrc/vae.hip).  Leading dims are flattened to `rows`; mean and
 * logvar are [rows, Z] with row strides ldm / ldv (column views of one [rows, 2Z] encoder output are fine); z, eps, dz, dmean, dlogvar
 * are contiguous [rows, Z] f32.
 * mg_vae_sample_f32: z = mean + exp(0.5 logvar) * eps and eps written out, eps ~ N(0, 1).  Noise mapping (restatable on the host with
 *   mg_philox4x32_10): flat element i = r * Z + c belongs to Philox block q = i / 4, counter words (q low, q high, ctr low,
 *   site ^ ctr high), key (seed low, seed high), ctr = *counter (DEVICE uint64, NULL = 0; the dropout step counter: mg_dropout_advance).
 *   A word w becomes u(w) = ((w >> 8) | 1) * 2^-24, exact in fp32 and inside (0, 1) (no log(0)).  The block's words (x, y, z, w) give
 *   elements 4q..4q+3 = Box-Muller pairs  R(x) cos(2 pi u(y)), R(x) sin(2 pi u(y)), R(z) cos(2 pi u(w)), R(z) sin(2 pi u(w)),
 *   R(a) = sqrt(-2 ln u(a)).
 * mg_vae_sample_bwd_f32: dmean = dz (dmean may be NULL), dlogvar = 0.5 dz eps exp(0.5 logvar).
 * mg_kld_standard_normal_f32: out[0] (DEVICE f32) = mean over rows of -0.5 sum_z (1 + lv - m^2 - exp(lv)) (reference losses.py:64-67); one
 *   workgroup, fixed summation order (fp64 partials): the same bits on every call.
 * mg_kld_standard_normal_bwd_f32: with g = grad[0] (DEVICE f32, the upstream gradient; no host read): dmean = g m / rows,
 *   dlogvar = g 0.5 (exp(lv) - 1) / rows.
 * mg_gather_concat_latent_*: mg_gather_concat_* with the latent behind the frame features:
 *   out[m] = [src[rows[m]] (0 for rows[m] < 0; rows NULL = src row m) | extra[m, 0:C] | z[m / rows_per_item, 0:Z] | 0 up to ldo].
 *   C may be 0 (extra NULL).  The bf16 form needs ldo % 8 == 0 and 16-byte aligned src / out.
 * mg_rows_add_per_item_f32: P[r, 0:N] += U[r / rows_per_item, 0:N] for r < rows (the rows behind, e.g. a table's extra rows, untouched).
 * mg_rows_sum_per_item: s[b, 0:N] = sum_{r = b rows_per_item}^{(b + 1) rows_per_item - 1} G[r, 0:N] (times H (1 - H) elementwise when H
 *   [rows, ldh] f32 is given: a sigmoid's gradient factor) for b < B <= 65535; G f32 (bf16 = 0) or bf16 (bf16 = 1) with row stride ldg;
 *   s f32 with row stride lds.  Fixed summation order. */
int mg_vae_sample_f32(const float* mean, int ldm, const float* logvar, int ldv, int64_t rows, int Z, uint64_t seed, uint32_t site,
                      const uint64_t* counter, float* z, float* eps, void* stream);
int mg_vae_sample_bwd_f32(const float* dz, const float* eps, const float* logvar, int ldv, int64_t rows, int Z, float* dmean, float* dlogvar,
                          void* stream);
int mg_kld_standard_normal_f32(const float* mean, int ldm, const float* logvar, int ldv, int64_t rows, int Z, float* out, void* stream);
int mg_kld_standard_normal_bwd_f32(const float* grad, const float* mean, int ldm, const float* logvar, int ldv, int64_t rows, int Z,
                                   float* dmean, float* dlogvar, void* stream);
int mg_gather_concat_latent_f32(const float* src, const int32_t* rows, const float* extra, const float* z, float* out, int64_t M, int F, int C,
                                int Z, int64_t rows_per_item, int ldo, void* stream);
int mg_gather_concat_latent_bf16(const float* src, const int32_t* rows, const float* extra, const float* z, uint16_t* out, int64_t M, int F,
                                 int C, int Z, int64_t rows_per_item, int ldo, void* stream);
int mg_rows_add_per_item_f32(float* P, int ldp, int64_t rows, int N, const float* U, int ldu, int64_t rows_per_item, void* stream);
int mg_rows_sum_per_item(const void* G, int ldg, int bf16, const float* H, int ldh, int64_t B, int64_t rows_per_item, int N, float* s, int lds,
                         void* stream);
/* Latent surface samplers (morgana.sampling, reference sampling.py; csrc/sampling.hip): points at a fixed distance from the prior's
 * centre, fed to a latent-conditioned model's predict().  out, unit, factor, dout are contiguous [rows, D] f32; rows >= 0 (0: nothing
 * is drawn); seed, site and counter as mg_vae_sample_f32 (counter: DEVICE uint64, NULL = 0; the dropout step counter).  One wave per
 * row; every reduction and the scan have one fixed order and use no atomics: the same bits on every call.
 * mg_sphere_sample_f32 (D >= 1): out = centre + radius g / |g|_2 and unit = g / |g|_2 written out; centre [D], radius a DEVICE f32
 *   scalar.  g ~ N(0, 1) by the noise mapping of mg_vae_sample_f32, word for word: flat element i = r * D + c belongs to Philox block
 *   q = i / 4 (blocks straddle rows when D % 4 != 0), counter words (q low, q high, ctr low, site ^ ctr high), key (seed low,
 *   seed high), ctr = *counter; u(w) = ((w >> 8) | 1) * 2^-24; the block's words (x, y, z, w) give elements 4q..4q+3 =
 *   R(x) cos(2 pi u(y)), R(x) sin(2 pi u(y)), R(z) cos(2 pi u(w)), R(z) sin(2 pi u(w)), R(a) = sqrt(-2 ln u(a)).  Rows of up to 256
 *   values stay in registers; longer rows loop over chunks of 64 with a carried partial sum.  D = 1 gives exactly centre +- radius.
 * mg_sphere_sample_bwd_f32: dcentre[c] = sum_r dout[r, c], dradius[0] = sum_{r, c} dout[r, c] unit[r, c]; fp64 partials.
 * mg_ellipsoid_sample_f32 (D >= 2; the reference's output is ill-formed below): D - 1 uniform angles per row.  Angle element
 *   i = r * (D - 1) + c draws u = u(word i % 4 of Philox block i / 4), same counter and key words as above; column 0 is
 *   phi = 2 pi u, columns 1..D-2 are theta = pi u.  factor[r, n] = (prod_{j < n} sin(angle_j)) * cos(angle_n) with an empty product
 *   = 1 and cos(angle_{D-1}) := 1; out = radii * factor, radii [D].  The reference's `centre` only fixes D and is NOT added
 *   (sampling.py:113); neither is it here.  The product is a wave scan with a carried prefix between chunks of 64 columns.
 * mg_ellipsoid_angles_f32: angles [rows, D - 1] of that mapping alone (the reference's sample_angles), as fp32 multiples of pi.
 * mg_ellipsoid_sample_bwd_f32: dradii[n] = sum_r dout[r, n] factor[r, n]; fp64 partials. */
int mg_sphere_sample_f32(const float* centre, const float* radius, int64_t rows, int D, uint64_t seed, uint32_t site, const uint64_t* counter,
                         float* out, float* unit, void* stream);
int mg_sphere_sample_bwd_f32(const float* dout, const float* unit, int64_t rows, int D, float* dcentre, float* dradius, void* stream);
int mg_ellipsoid_sample_f32(const float* radii, int64_t rows, int D, uint64_t seed, uint32_t site, const uint64_t* counter, float* out,
                            float* factor, void* stream);
int mg_ellipsoid_angles_f32(int64_t rows, int D, uint64_t seed, uint32_t site, const uint64_t* counter, float* angles, void* stream);
int mg_ellipsoid_sample_bwd_f32(const float* dout, const float* factor, int64_t rows, int D, float* dradii, void* stream);
/* CALIBRATION (a measurement entry; no training step calls it): one launch of a register-operand bf16 MFMA loop - n_workgroups x 512
 * threads (two waves per SIMD), every wave issues 16 x trips v_mfma_f32_16x16x32_bf16 on operands read once from `operands`
 * (bf16, at least 4096 x 64 values: the caller chooses the data, e.g. random) and writes one float per thread to `sink`
 * (n_workgroups x 512 floats).  *flop (host, optional) receives the launch's FLOP count; the caller times it with events.
 * Used by bench.py for `frac_of_sustained`: what the matrix pipe of THIS chip holds under its power limit. */
int mg_calib_mfma_bf16(const uint16_t* operands, float* sink, int n_workgroups, int trips, double* flop, void* stream);
/* dst f32 [rows, cols] = src bf16 [rows, cols] (lds). */
int mg_cast_bf16_f32(const uint16_t* src, int lds, float* dst, int ldd, int64_t rows, int cols, void* stream);
/* elementwise sigmoid forward / backward for a stand-alone nn.Sigmoid. */
int mg_sigmoid_f32(const float* x, float* y, int64_t n, void* stream);
int mg_sigmoid_grad_f32(const float* dy, const float* y, float* dx, int64_t n, void* stream);
/* y = act(x) and dx = dy f'(y) for act = MG_ACT_SIGMOID / MG_ACT_TANH / MG_ACT_RELU: a stand-alone torch.nn.Tanh / ReLU / Sigmoid
 * of the container (morgana/utils.py:401-418, e.g. behind a recurrent wrapper) and the gradient of a Linear run's trailing
 * activation.  ReLU as torch.relu / threshold_backward: NaN passes through, relu(-0.0) = -0.0, dx = 0 where y <= 0. */
int mg_act_f32(const float* x, float* y, int64_t n, int act, void* stream);
int mg_act_grad_f32(const float* dy, const float* y, float* dx, int64_t n, int act, void* stream);

/* Fused tail of a Linear/Sigmoid stack ending in ... -> 128 -> 32 -> 1 under the masked MSE (the README F0Model's layers 3-4,
 * README.rst:65-73, with morgana/losses.py:29-51), bf16 mode: forward of both layers, the loss, and the whole backward
 * through both, in one pass over H2.
 *   H2 bf16 [B*T, ldh] (the 128 sigmoid outputs of the previous layer); W3 f32 [32,128], b3 [32], W4 f32 [1,32], b4 [1];
 *   target f32 [B*T] (D = 1); seq_len int64 [B] or NULL; grad_scale multiplies dL/dpred.
 * Outputs: pred f32 [B*T]; loss f32 [1]; dZ2 bf16 [B*T, ldh] = dL/d(pre-activation of the 128-wide layer);
 *   grads f32 [32*128 + 32 + 32 + 1] = dW3 | db3 | dW4 | db4 (accumulate != 0 adds into it).  If `loss` points at the
 *   float right behind `grads` (and accumulate == 0) both are finished by a single reduce launch.
 * workspace: mg_f0_tail_workspace_bytes(B*T).  Deterministic. */
size_t mg_f0_tail_workspace_bytes(int64_t M);
int mg_f0_tail_bf16(const uint16_t* H2, int ldh, int K3, const float* W3, const float* b3, const float* W4, const float* b4,
                    const float* target, const int64_t* seq_len, int B, int T, float grad_scale, float* pred, float* loss,
                    uint16_t* dZ2, float* grads, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* The tail on M rows that each stand for a group of frames sharing one input row (phone-rate step): loss = sum_m row_weight[m]
 * (pred[m] - target[m])^2 and its whole backward; target / row_weight from mg_phone_target_stats. */
int mg_f0_tail_rows_bf16(const uint16_t* H2, int ldh, int K3, const float* W3, const float* b3, const float* W4, const float* b4,
                         const float* target, const float* row_weight, int64_t M, float grad_scale, float* pred, float* loss,
                         uint16_t* dZ2, float* grads, int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* The 512 -> 128 Linear + Sigmoid in front of that tail fused INTO it (README.rst:65-73 layers 2-4 + morgana/losses.py:29-51):
 * one pass over H1, the 128-wide activation H2 never reaches memory (the backward of layer 2 needs dZ2 and H1 only).
 *   H1 bf16 [B*T, ldh1] (the 512 sigmoid outputs of the first layer); W2 bf16 [128, ldw2] (the optimiser's bf16 copy of the
 *   weight, mg_cast_params_bf16 / mg_adam_step_plan_f32), b2 f32 [128]; everything else as mg_f0_tail_bf16.
 * Outputs as mg_f0_tail_bf16, with dZ2 bf16 [B*T, lddz].  Same arithmetic per frame as mg_linear_fwd_bf16 + mg_f0_tail_bf16
 * up to the summation order inside the 512-deep dot products.  workspace: mg_f0_l2tail_workspace_bytes(B*T).  Deterministic. */
size_t mg_f0_l2tail_workspace_bytes(int64_t M);
int mg_f0_l2tail_bf16(const uint16_t* H1, int ldh1, int K2, const uint16_t* W2, int ldw2, int N2, const float* b2, const float* W3,
                      const float* b3, const float* W4, const float* b4, const float* target, const int64_t* seq_len, int B, int T,
                      float grad_scale, float* pred, float* loss, uint16_t* dZ2, int lddz, float* grads, int accumulate, void* workspace,
                      size_t workspace_bytes, void* stream);
/* mg_f0_l2tail_bf16 without its reduce launch (as mg_f0_l2tail_rows_slabs_bf16 below): the slabs stay in `workspace` for the update
 * kernel's plan - gradients as a slab source, the loss through mg_adam_tail.  For a step captured whole into a HIP graph. */
int mg_f0_l2tail_slabs_bf16(const uint16_t* H1, int ldh1, int K2, const uint16_t* W2, int ldw2, int N2, const float* b2, const float* W3,
                            const float* b3, const float* W4, const float* b4, const float* target, const int64_t* seq_len, int B, int T,
                            float grad_scale, float* pred, uint16_t* dZ2, int lddz, void* workspace, size_t workspace_bytes, int* n_slabs,
                            void* stream);
/* ... on M rows that each stand for a group of frames (phone-rate step), as mg_f0_tail_rows_bf16. */
int mg_f0_l2tail_rows_bf16(const uint16_t* H1, int ldh1, int K2, const uint16_t* W2, int ldw2, int N2, const float* b2, const float* W3,
                           const float* b3, const float* W4, const float* b4, const float* target, const float* row_weight, int64_t M,
                           float grad_scale, float* pred, float* loss, uint16_t* dZ2, int lddz, float* grads, int accumulate,
                           void* workspace, size_t workspace_bytes, void* stream);
/* mg_f0_l2tail_rows_bf16 without its reduce launch: the workgroups' sums (32*128 + 32 + 32 + 2 floats each: dW3 | db3 | dW4 | db4 | loss)
 * stay at the start of `workspace`, *n_slabs of them, mg_f0_l2tail_slab_stride() floats apart, for mg_expand_column_reduce_f32 (or the
 * update kernel's plan) to sum. */
int64_t mg_f0_l2tail_slab_stride(void);
int mg_f0_l2tail_rows_slabs_bf16(const uint16_t* H1, int ldh1, int K2, const uint16_t* W2, int ldw2, int N2, const float* b2, const float* W3,
                                 const float* b3, const float* W4, const float* b4, const float* target, const float* row_weight, int64_t M,
                                 float grad_scale, float* pred, uint16_t* dZ2, int lddz, void* workspace, size_t workspace_bytes, int* n_slabs,
                                 void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K3  GRU through RecurrentCuDNNWrapper   reference: morgana/utils.py:345-393 + torch.nn.GRU (gates r, z, n)
 * The sort / pack / unpack of the reference only restricts item b to its first seq_len[b] steps; here that is a
 * per-item length mask, outputs beyond the length are exactly 0 and h_n is the state at the last valid step.
 * ---------------------------------------------------------------------------------------------------------------- */
/* Forward recurrence, one launch per step.
 *   xproj  [B,T,3H] = x W_ih^T + b_ih (computed with mg_linear_fwd_*); w_hh [3H,H]; b_hh [3H]; seq_len NULL or int64 [B]
 *   hstate [B,T+1,H]: slot 0 must hold h0 (or zeros) on entry; slot t+1 receives the state after step t (frozen once
 *                     t >= seq_len[b]), so h_n = hstate[:, T, :] and h_{t-1} = hstate[:, t, :] for the backward
 *   out    [B,T,H]   = h_t on valid steps, exactly 0 on padded steps (pad_packed_sequence, utils.py:383)
 *   saved  [B,T,4H]  = (r, z, n, W_hn h + b_hn) for the backward
 * CONTRACT for steps past an item's length (t >= seq_len[b]), all GRU / LSTM entry points of this header:
 *   - out is exactly 0 there and hstate repeats the last valid state (both specified, both tested);
 *   - saved[b,t,:] is UNSPECIFIED there.  The forward kernels differ in what they leave: the per-step kernels (mg_gru_fwd_f32,
 *     mg_gru_fwd_bf16, mg_lstm_fwd_f32) store the gate values the frozen state and whatever xproj holds at that position produce;
 *     the workgroup-local kernels (mg_gru_fwd_small_f32) do the same; the persistent kernels (mg_gru_fwd_persist_*,
 *     mg_lstm_fwd_persist_bf16, mg_lstm_pstack_fwd_bf16) do so up to the longest sequence of the item's group and write zeros or
 *     nothing at all beyond it.  Callers must not compare or consume these elements;
 *   - every backward entry point treats such a step as inactive: the loads of saved[b,t,:] and grad_out[b,t,:] may be issued, but
 *     their values are discarded by a select (never multiplied by a 0/1 mask), so NaN or garbage there cannot reach dxproj,
 *     dhproj, dgates, dh0 / dc0 or any shadow; the gate gradients written for such a step are exactly 0.
 *     tests/test_gpu_configs.py::test_gru_backward_never_reads_saved_past_seq_len poisons these elements with NaN in all five
 *     backward forms and requires bit-identical, finite gradients. */
int mg_gru_fwd_f32(const float* xproj, const float* w_hh, const float* b_hh, const int64_t* seq_len, int B, int T, int H,
                   float* hstate, float* out, float* saved, void* stream);
/* BPTT, one launch per step.  grad_out [B,T,H]; grad_hn NULL or [B,H] (gradient of h_n).
 * Produces dxproj [B,T,3H] (= dL/d xproj: feed to wgrad / dgrad of W_ih), dhproj [B,T,3H] (= dL/d(h W_hh^T + b_hh):
 * dW_hh = dhproj^T h_prev with h_prev rows = hstate[:, t, :], db_hh = column sums) and dh0 [B,H].
 * workspace: mg_gru_bwd_workspace_bytes(B,H). */
size_t mg_gru_bwd_workspace_bytes(int B, int H);
int mg_gru_bwd_f32(const float* grad_out, const float* grad_hn, const float* hstate, const float* saved, const float* w_hh,
                   const int64_t* seq_len, int B, int T, int H, float* dxproj, float* dhproj, float* dh0, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Small hidden sizes (H = 64 or 128, e.g. the GRU-64 layers of models/f0_test_model.py): the same recurrence, exact fp32, as ONE
 * launch per direction in which a workgroup owns 256 / H items outright (W_hh in its registers, the state in its LDS, no
 * hand-off between workgroups).  Same arguments and results as mg_gru_fwd_f32 / mg_gru_bwd_f32 (no workspace); sums over the
 * contraction in a different order (equal to fp32 rounding).  mg_gru_fwd_f32 / mg_gru_bwd_f32 route here themselves when
 * mg_gru_small_supported(H) != 0. */
int mg_gru_small_supported(int H);
int mg_gru_fwd_small_f32(const float* xproj, const float* w_hh, const float* b_hh, const int64_t* seq_len, int B, int T, int H,
                         float* hstate, float* out, float* saved, void* stream);
int mg_gru_bwd_small_f32(const float* grad_out, const float* grad_hn, const float* hstate, const float* saved, const float* w_hh,
                         const int64_t* seq_len, int B, int T, int H, float* dxproj, float* dhproj, float* dh0, void* stream);

/* fp32 parity mode as ONE launch per direction for 256 <= H <= 512, H % 64 == 0, B <= 128: the group / slot scheme of the bf16
 * persistent kernels below with fp32 hand-off tiles and the exact-fp32 MFMA in the per-step kernels' block order, the same cell
 * code - results bit-identical to mg_gru_fwd_f32 / mg_gru_bwd_f32 on the live steps (gate values of steps beyond an item
 * group's longest sequence are written as zeros).  Workspace, status word and residency: as for mg_gru_fwd_persist_bf16. */
int mg_gru_persist_f32_supported(int B, int T, int H);
int mg_gru_fwd_persist_f32(const float* xproj, const float* w_hh, const float* b_hh, const int64_t* seq_len, int B, int T, int H,
                           float* hstate, float* out, float* saved, void* workspace, size_t workspace_bytes, void* stream);
int mg_gru_bwd_persist_f32(const float* grad_out, const float* grad_hn, const float* hstate, const float* saved, const float* w_hh,
                           const int64_t* seq_len, int B, int T, int H, float* dxproj, float* dhproj, float* dh0, void* workspace,
                           size_t workspace_bytes, void* stream);

/* The same recurrence with bf16 matmul operands (throughput mode; cell arithmetic, states, gate values and all outputs stay
 * f32): w_hh_bf = bf16(W_hh) [3H, ldw]; hstate_bf [B,T+1,H] is a bf16 shadow of hstate that the caller initialises at slot 0 and
 * the kernel extends; backward takes w_hh_t_bf = bf16(W_hh^T) [H, ldt >= 3H] and fills dhproj_bf [B,T,3H], the shadow of dhproj.
 * Needs H % 128 == 0 (H <= 1024). */
int mg_gru_fwd_bf16(const float* xproj, const uint16_t* w_hh_bf, int ldw, const float* b_hh, const int64_t* seq_len, int B, int T,
                    int H, float* hstate, uint16_t* hstate_bf, float* out, float* saved, void* stream);
int mg_gru_bwd_bf16(const float* grad_out, const float* grad_hn, const float* hstate, const float* saved,
                    const uint16_t* w_hh_t_bf, int ldt, const int64_t* seq_len, int B, int T, int H, float* dxproj, float* dhproj,
                    uint16_t* dhproj_bf, float* dh0, void* workspace, size_t workspace_bytes, void* stream);

/* The bf16-operand recurrence as ONE launch per direction (persistent kernel: W_hh in registers for all T steps, the state
 * handed between workgroups through write-through stores and per-slot flags; the batch is cut into 8 independent groups).
 * Same arguments and results as mg_gru_fwd_bf16 / mg_gru_bwd_bf16 plus a workspace of mg_gru_persist_workspace_bytes(B, H) holding the
 * hand-off ring, the flags and a status word.  mg_gru_persist_supported(B, T, H) != 0 says the shape is covered (H % 128 == 0, H <= 512,
 * B <= 256, buffers < 2 GiB); other shapes return MG_EINVAL - use the per-step entry points.  All workgroups of the launch
 * must be resident together (at most 256 of 256 threads): the calling stream must own the device.  The workspace (16-byte
 * aligned, zeroed ONCE by the caller after allocating it) may be reused by later launches on the same stream: each launch resets
 * the flags itself, the status word behind them is sticky.  Every wait in the kernel is bounded;
 * mg_gru_persist_status(workspace, stream) synchronises the stream, returns MG_ELAUNCH if any launch since the last call timed
 * out (its results are invalid) and clears the word. */
size_t mg_gru_persist_workspace_bytes(int B, int H);
int mg_gru_persist_supported(int B, int T, int H);
int mg_gru_persist_status(void* workspace, void* stream);
int mg_gru_fwd_persist_bf16(const float* xproj, const uint16_t* w_hh_bf, int ldw, const float* b_hh, const int64_t* seq_len, int B,
                            int T, int H, float* hstate, uint16_t* hstate_bf, float* out, float* saved, void* workspace,
                            size_t workspace_bytes, void* stream);
/* mg_gru_fwd_persist_bf16 with the input projections read through a row map: frame (b, t) takes row xrows[b * T + t] of the table xproj
 * [n_rows, 3H] (int32, every entry in [0, n_rows)) - the repetition of upsample_to_repetitions (morgana/utils.py:175-228) applied
 * inside the recurrence instead of to a [B, T, 3H] copy of the projected rows.  xrows NULL: xproj is [B, T, 3H] (the entry above). */
int mg_gru_fwd_persist_rows_bf16(const float* xproj, const int32_t* xrows, int64_t n_rows, const uint16_t* w_hh_bf, int ldw, const float* b_hh,
                                 const int64_t* seq_len, int B, int T, int H, float* hstate, uint16_t* hstate_bf, float* out, float* saved,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* mg_gru_fwd_persist_rows_bf16 that also writes out_bf (optional, may be NULL): the bf16 copy of `out` [B, T, H] (zero past each item's
 * length) - the operand of the nn.Linear that follows the wrapper in models/RNN_SPSS.py:38, without a cast pass over [B, T, H]. */
int mg_gru_fwd_persist_out_bf16(const float* xproj, const int32_t* xrows, int64_t n_rows, const uint16_t* w_hh_bf, int ldw, const float* b_hh,
                                const int64_t* seq_len, int B, int T, int H, float* hstate, uint16_t* hstate_bf, float* out, uint16_t* out_bf,
                                float* saved, void* workspace, size_t workspace_bytes, void* stream);
/* backward: dxproj_bf (optional) = bf16 shadow of dxproj [B,T,3H]; dxproj and dhproj (both or neither) may be NULL when the caller
 * only needs the bf16 shadows (the weight- and input-gradient GEMMs of bf16 mode) - the fp32 arrays are then not written */
int mg_gru_bwd_persist_bf16(const float* grad_out, const float* grad_hn, const float* hstate, const float* saved,
                            const uint16_t* w_hh_t_bf, int ldt, const int64_t* seq_len, int B, int T, int H, float* dxproj,
                            float* dhproj, uint16_t* dhproj_bf, uint16_t* dxproj_bf, float* dh0, void* workspace,
                            size_t workspace_bytes, void* stream);

/* fp32 parity mode of the LSTM recurrence as ONE launch per direction for 256 <= H <= 512, H % 64 == 0, B <= 128 (csrc/lstm_persist_f32.hip):
 * W_hh resident in registers, fp32 hand-off tiles, the exact-fp32 MFMA in the per-step kernels' block order and the same cell code -
 * results bit-identical to mg_lstm_fwd_f32 / mg_lstm_bwd_f32 on the live steps (gate values of steps beyond an item group's longest
 * sequence are written as zeros).  Arguments as mg_lstm_fwd_f32 / mg_lstm_bwd_f32 (grad_out may be NULL = zero); workspace
 * (mg_gru_persist_workspace_bytes(B, H)), status word and residency requirement as for mg_gru_fwd_persist_bf16. */
int mg_lstm_persist_f32_supported(int B, int T, int H);
int mg_lstm_fwd_persist_f32(const float* xproj, const float* w_hh, const float* b_hh, const int64_t* seq_len, int B, int T, int H,
                            float* hstate, float* cstate, float* out, float* saved, void* workspace, size_t workspace_bytes,
                            void* stream);
int mg_lstm_bwd_persist_f32(const float* grad_out, const float* grad_hn, const float* grad_cn, const float* cstate, const float* saved,
                            const float* w_hh, const int64_t* seq_len, int B, int T, int H, float* dgates, float* dh0, float* dc0,
                            void* workspace, size_t workspace_bytes, void* stream);

/* The LSTM recurrence (gates i, f, g, o) in the same persistent form: bf16 matmul operands, fp32 cell, one launch per
 * direction.  w_hh_bf = bf16(W_hh) [4H, ldw]; hstate_bf [B,T+1,H] = bf16 shadow of hstate (slot 0 set by the caller, the rest
 * written here); backward takes w_hh_t_bf = bf16(W_hh^T) [H, ldt >= 4H] and fills dgates [B,T,4H] (optional: NULL = not written)
 * and its bf16 shadow dgates_bf.
 * Other arguments as mg_lstm_fwd_f32 / mg_lstm_bwd_f32.  Workspace, status word and residency requirement: as for the GRU entry
 * points (mg_gru_persist_workspace_bytes(B, H) covers both; mg_gru_persist_status reads the shared status word). */
int mg_lstm_persist_supported(int B, int T, int H);
int mg_lstm_fwd_persist_bf16(const float* xproj, const uint16_t* w_hh_bf, int ldw, const float* b_hh, const int64_t* seq_len, int B,
                             int T, int H, float* hstate, float* cstate, uint16_t* hstate_bf, float* out, float* saved,
                             void* workspace, size_t workspace_bytes, void* stream);
int mg_lstm_bwd_persist_bf16(const float* grad_out, const float* grad_hn, const float* grad_cn, const float* cstate,
                             const float* saved, const uint16_t* w_hh_t_bf, int ldt, const int64_t* seq_len, int B, int T, int H,
                             float* dgates, uint16_t* dgates_bf, float* dh0, float* dc0, void* workspace, size_t workspace_bytes,
                             void* stream);

/* A whole stack of L LSTM layers (2 <= L <= MG_LSTM_MAX_LAYERS, the 8 x nn.LSTM(512, 512) of models/RNN_SPSS.py:36-37) forward
 * in ONE launch: a wavefront over (layer, time) - T + L - 1 dependent steps instead of L T.  Layer 0 takes xproj = x W_ih^T +
 * b_ih [B,T,4H] from memory; the layers above compute their input projection inside the step from the hand-off tiles of the
 * layer below (w_ih_bf = bf16(W_ih) [4H, ldwi], input size == H).  Per layer: cstate, saved and hstate_bf complete; of hstate
 * only slot T (h_n); out only for the top layer (the other layers' out buffers are not written).
 * mg_lstm_pstack_supported(B, T, H, L): H % 128 == 0, H <= 512 and L G H / 16 <= 512 workgroups for a group count G in
 * {8, 4, 2, 1} with ceil(B / G) <= 32 (L = 8, H = 512: B <= 64).  All workgroups must be resident together, two per CU.
 * The workspace (mg_lstm_pstack_workspace_bytes, zeroed once by the caller) carries the sticky status word at the same offset
 * as the other persistent entry points (mg_gru_persist_status). */
typedef struct {
    const float* xproj;           /* layer 0 only */
    const uint16_t* w_ih_bf;      /* layers >= 1 */
    const float* b_ih;            /* layers >= 1 */
    const uint16_t* w_hh_bf;
    const float* b_hh;
    float* hstate;                /* [B,T+1,H], slot 0 = h0 set by the caller; only slot T (h_n) is written */
    float* cstate;                /* [B,T+1,H], slot 0 = c0 set by the caller */
    uint16_t* hstate_bf;          /* [B,T+1,H] bf16 shadow, slot 0 set by the caller */
    float* out;                   /* [B,T,H]; written for the top layer only */
    float* saved;                 /* [B,T,4H] gate values i, f, g, o */
    int ldwi, ldwh;
} mg_lstm_pstack_layer;
int mg_lstm_pstack_supported(int B, int T, int H, int L);
size_t mg_lstm_pstack_workspace_bytes(int B, int H, int L);
int mg_lstm_pstack_fwd_bf16(const mg_lstm_pstack_layer* layers, int L, const int64_t* seq_len, int B, int T, int H, void* workspace,
                            size_t workspace_bytes, void* stream);

/* The backward of the same stack in ONE launch (reference: autograd through the 8 chained nn.LSTM of models/RNN_SPSS.py:36-37): the
 * forward's wavefront run down in time and down through the layers.  Layer l's step t takes the gate gradients of the layer above
 * at step t through that layer's W_ih inside the step (d out^l_t = dgates^{l+1}_t W_ih^{l+1}) instead of a grad_out row from memory,
 * so the L - 1 input-gradient GEMMs between per-layer launches go as well.  Per layer: dgates_bf [B,T,4H] (bf16 gate gradients
 * i, f, g, o: the operand of the weight-gradient GEMMs and, for layer 0, of the input-gradient GEMM; exactly 0 on padded steps),
 * optionally the fp32 copy dgates, dh0 / dc0 [B,H].  Same arithmetic as L chained mg_lstm_bwd_persist_bf16 calls with
 * mg_linear_dgrad_bf16 between them, up to the summation order of the in-step product.
 * mg_lstm_pstack_bwd_supported(B, T, H, L): H % 128 == 0, H <= 512, B T 4H < 2^31 and L G H / 32 <= 256 workgroups (one per CU, a
 * slot of 32 hidden units) or L G H / 16 <= 512 (two per CU) for a group count G in {8, 4, 2, 1} with ceil(B / G) <= 32.
 * Workspace: mg_lstm_pstack_bwd_workspace_bytes, zeroed once by the caller, status word as for the other persistent launches. */
typedef struct {
    const float* grad_out;          /* top layer only: [B,T,H] or NULL (zero); ignored below the top */
    const float* grad_hn;           /* NULL or [B,H] */
    const float* grad_cn;           /* NULL or [B,H] */
    const float* cstate;            /* [B,T+1,H] of the forward */
    const float* saved;             /* [B,T,4H] gate values of the forward */
    const uint16_t* w_hh_t_bf;      /* bf16(W_hh^T) [H, ldt] */
    const uint16_t* w_ih_up_t_bf;   /* layers below the top: bf16(W_ih^T) of the layer ABOVE, [H, ldt_up] */
    float* dgates;                  /* NULL or [B,T,4H] */
    uint16_t* dgates_bf;            /* [B,T,4H] */
    float* dh0;                     /* [B,H] */
    float* dc0;                     /* [B,H] */
    int ldt, ldt_up;
} mg_lstm_pstack_bwd_layer;
int mg_lstm_pstack_bwd_supported(int B, int T, int H, int L);
size_t mg_lstm_pstack_bwd_workspace_bytes(int B, int H, int L);
int mg_lstm_pstack_bwd_bf16(const mg_lstm_pstack_bwd_layer* layers, int L, const int64_t* seq_len, int B, int T, int H, void* workspace,
                            size_t workspace_bytes, void* stream);

/* A STACK of small GRU layers (reference: the three RecurrentCuDNNWrapper(nn.GRU(., 64)) of the shipped F0 model,
 * models/f0_test_model.py:31-37, one after the other through SequentialWithRecurrent, utils.py:396-418) as ONE launch per direction:
 * the workgroup-local kernels above run as a wavefront over (layer, time), one workgroup per (layer, block of 4 items).  Layers above
 * the first compute their input projection inside the step (w_ih [3H, H], b_ih: their input IS the lower layer's output, input size
 * == H) and, backward, the gradient they hand to the layer below (dxproj_t W_ih), so the projection and input-gradient GEMMs between
 * the layers go.  Exact fp32; per layer the same results as mg_gru_fwd_small_f32 / mg_gru_bwd_small_f32 fed with the neighbouring
 * layer's rows, up to the summation order of those in-step products.
 * Hand-off buffers: `out` of every layer below the top (forward) and `dxin` of every layer below the top (backward) are filled with a
 * sentinel by the entry point and written exactly once per element by the producing layer; after the launch they hold ordinary
 * values (`out`: the layer's outputs, zero on padded steps, as from mg_gru_fwd_f32).
 * mg_gru_stack_small_supported: H == 64, 2 <= L <= MG_GRU_STACK_MAX_LAYERS, all L ceil(B / 4) workgroups resident.
 * Workspace (mg_gru_stack_small_workspace_bytes, zeroed once by the caller): the sticky status word of mg_gru_persist_status. */
#define MG_GRU_STACK_MAX_LAYERS 4
typedef struct {
    /* forward */
    const float* xproj;     /* layer 0: [B,T,3H] = x W_ih^T + b_ih */
    const float* w_ih;      /* layers >= 1: [3H,H] (both directions) */
    const float* b_ih;      /* layers >= 1: [3H] */
    const float* w_hh;      /* [3H,H] (both directions) */
    const float* b_hh;      /* [3H] */
    float* hstate;          /* [B,T+1,H], slot 0 = h0 on entry (read by the backward) */
    float* out;             /* [B,T,H] */
    float* saved;           /* [B,T,4H] (read by the backward) */
    /* backward */
    const float* grad_out;  /* top layer: [B,T,H] */
    const float* grad_hn;   /* NULL or [B,H] */
    float* dxin;            /* layers below the top: [B,T,H], the gradient of the layer's outputs as the layer above hands it down */
    float* dxproj;          /* [B,T,3H] */
    float* dhproj;          /* [B,T,3H] */
    float* dh0;             /* [B,H] */
} mg_gru_stack_layer;
int mg_gru_stack_small_supported(int B, int T, int H, int L);
size_t mg_gru_stack_small_workspace_bytes(void);
int mg_gru_stack_fwd_small_f32(const mg_gru_stack_layer* layers, int L, const int64_t* seq_len, int B, int T, int H, void* workspace,
                               size_t workspace_bytes, void* stream);
/* The throughput-mode ("bf16" precision) forms, same arguments: the cell's sigmoid / tanh on v_exp_f32 / v_rcp_f32 and the step's
 * products on v_mfma_f32_16x16x32_bf16 (W_hh / W_ih, the state and what the layers hand each other rounded to bf16 as operands, fp32
 * accumulation - as the bf16-mode GRU-512 recurrence); state, cell and everything stored stay fp32.  The _f32 entries are exact fp32. */
int mg_gru_stack_fwd_small_fast_f32(const mg_gru_stack_layer* layers, int L, const int64_t* seq_len, int B, int T, int H, void* workspace,
                                    size_t workspace_bytes, void* stream);
int mg_gru_stack_bwd_small_f32(const mg_gru_stack_layer* layers, int L, const int64_t* seq_len, int B, int T, int H, void* workspace,
                               size_t workspace_bytes, void* stream);
int mg_gru_stack_bwd_small_fast_f32(const mg_gru_stack_layer* layers, int L, const int64_t* seq_len, int B, int T, int H, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* LSTM through RecurrentCuDNNWrapper   reference: morgana/utils.py:345-393 + torch.nn.LSTM (gates i, f, g, o), the cell of
 * the reference's shipped acoustic model (models/RNN_SPSS.py:36-37).  Same conventions as the GRU entry points:
 *   xproj [B,T,4H] = x W_ih^T + b_ih; w_hh [4H,H]; b_hh [4H]; hstate / cstate [B,T+1,H] with slot 0 = (h0, c0) on entry;
 *   out [B,T,H] zero on padded steps; saved [B,T,4H] = activated gates (i, f, g, o).
 * Backward: dgates [B,T,4H] = dL/d(gate pre-activations) (feeds dW_ih, dW_hh, both biases and dx); dh0, dc0 [B,H];
 *   grad_hn / grad_cn NULL or [B,H]; workspace mg_lstm_bwd_workspace_bytes(B,H). */
int mg_lstm_fwd_f32(const float* xproj, const float* w_hh, const float* b_hh, const int64_t* seq_len, int B, int T, int H,
                    float* hstate, float* cstate, float* out, float* saved, void* stream);
size_t mg_lstm_bwd_workspace_bytes(int B, int H);
int mg_lstm_bwd_f32(const float* grad_out, const float* grad_hn, const float* grad_cn, const float* cstate, const float* saved,
                    const float* w_hh, const int64_t* seq_len, int B, int T, int H, float* dgates, float* dh0, float* dc0,
                    void* workspace, size_t workspace_bytes, void* stream);

/* A stack of LSTM layers run skewed in time (reference: the 8 x RecurrentCuDNNWrapper(nn.LSTM) of models/RNN_SPSS.py:36-37,
 * or one multi-layer nn.LSTM): layer l runs `lag` steps behind layer l-1 and ONE launch per step serves every layer, so the
 * stack costs T + (L-1) lag dependent launches instead of L T.  The caller interleaves, every `lag` steps, the GEMMs that turn
 * the outputs a layer has just finished into the next chunk of its upper neighbour's input projections (forward) or the
 * gate gradients of a layer into the next chunk of its lower neighbour's output gradients (backward).
 *   forward  step s: layer l processes time t = s - l*lag (0 <= t < T), reading xproj rows of times x_t0 .. x_t0+x_T-1
 *   backward step u: layer l processes time t = T_pad-1 - (u - (L-1-l)*lag), T_pad = ceil(T/lag)*lag; t = -1 finishes
 *                    dh0 / dc0; grad_out (NULL = zero) holds times g_t0 .. g_t0+g_T-1; carry_h / carry_c [B,H] must hold
 *                    grad_hn / grad_cn (or zeros) before the first step.
 * Buffers per layer as in mg_lstm_fwd_f32 / mg_lstm_bwd_f32.  `layers` is a HOST array, n_layers <= MG_LSTM_MAX_LAYERS. */
#define MG_LSTM_MAX_LAYERS 8
typedef struct {
    const float* xproj;
    int x_T, x_t0;
    const float* w_hh;
    const float* b_hh;
    float* hstate;
    float* cstate;
    float* out;
    float* saved;
} mg_lstm_fwd_layer;
typedef struct {
    const float* grad_out;
    int g_T, g_t0;
    const float* cstate;
    const float* saved;
    const float* w_hh;
    float* dgates;
    float* carry_h;
    float* carry_c;
    float* dh0;
    float* dc0;
} mg_lstm_bwd_layer;
int mg_lstm_stack_fwd_f32(const mg_lstm_fwd_layer* layers, int n_layers, const int64_t* seq_len, int B, int T, int H, int lag,
                          int s_begin, int s_end, void* stream);
int mg_lstm_stack_bwd_f32(const mg_lstm_bwd_layer* layers, int n_layers, const int64_t* seq_len, int B, int T, int H, int lag,
                          int u_begin, int u_end, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Optimiser / EMA                         reference: torch.optim.Adam at experiment_builder.py:516, :468-474;
 *                                         ExponentialMovingAverage.update_params, morgana/utils.py:443-456
 * ---------------------------------------------------------------------------------------------------------------- */
/* One Adam step over a flat fp32 parameter buffer (torch defaults: L2 weight decay added to the gradient).
 * grad is read as grad * grad_scale (1/world_size after a sum all-reduce).  step is 1-based. */
int mg_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                     void* stream);
/* The same step with its two step-dependent scalars read from DEVICE memory (scalars[0] = lr / (1 - beta1^step),
 * scalars[1] = sqrt(1 - beta2^step); mg_adam_scalars forms them on the host exactly as mg_adam_step_f32 does): the launch can be
 * captured in a hipGraph and replayed for every step with only those 8 bytes rewritten. */
void mg_adam_scalars(float lr, float beta1, float beta2, int64_t step, float* out2);
/* dst[0..1] = (a, b) in stream order, the values carried as kernel arguments (safe however far the host runs ahead). */
int mg_store_pair_f32(float* dst, float a, float b, void* stream);
/* dst[0 .. 2 n_pairs) = the pairs of the HOST array `values` (n_pairs <= MG_STORE_PAIRS_MAX), the same way: one launch stages the
 * scalars of every step a multi-step graph replay performs (slot j = dst + 2 j, handed to the j-th update launch). */
#define MG_STORE_PAIRS_MAX 32
int mg_store_pairs_f32(float* dst, const float* values, int n_pairs, void* stream);
int mg_adam_step_dev_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                         float beta2, float eps, float weight_decay, const float* scalars, float grad_scale, void* stream);
/* The update as the LAST node of a training step that hands it more than a finished gradient (scalars from device memory as in
 * mg_adam_step_dev_f32).  `plan` is a HOST struct, copied into the launch:
 *   slabs[i]   : elements [begin, begin+count) of the flat gradient additionally receive sum_s slab[s*stride + (j - begin)],
 *                s < n_slabs, summed in the fixed order of the library's slab reduce (16 interleaved partitions, ascending) - the
 *                split-M partial results of a weight-gradient GEMM (mg_linear_wgrad_slabs_bf16), consumed here instead of by a
 *                reduce launch of their own; n_slabs == 1 adds a plain buffer (the fused tail's gradients)
 *   shadows[i] : the fp32 matrix [rows, cols] at flat offset `offset` is re-cast after its update into dst bf16 [rows, ldd] and / or
 *                its transpose dst_t bf16 [cols, ldt] (padding columns are never written: zero them once) - the operands of the next
 *                step's GEMMs, so no cast launch is needed
 *   clear_grad : != 0 zeroes the flat gradient behind the read (the next step needs no memset)
 * Results equal mg_adam_step_dev_f32 on the reduced gradient bit for bit. */
#define MG_ADAM_MAX_SLABS 4
#define MG_ADAM_MAX_SHADOWS 8
typedef struct {
    int64_t begin, count;
    const float* slab;
    int n_slabs;
    int64_t stride;
} mg_adam_slab_src;
typedef struct {
    int64_t offset;
    int rows, cols;
    uint16_t* dst;
    int ldd;
    uint16_t* dst_t;
    int ldt;
    int pair;       /* != 0: dst / dst_t are [hi | lo] PAIR PLANES (precision 'bf16x3', the mg_*_x3 entry points): ldd / ldt = the row stride
                     * of both planes, hi = bf16(w) at column c, lo = bf16(w - hi) at column ldd / 2 + c (ldt / 2 + r for the transpose) */
} mg_adam_shadow;
/* What a step captured whole into a HIP graph leaves of its FORWARD for the update's launch (nothing can observe the step half done
 * inside a replay): the per-phone prediction repeated to frames (out[f] = table[rows[f]], `frames` of them; 0 = none) and the loss =
 * ordered sum over n_slabs slabs of their element n - 1 (+ the constant term: n_partial partial sums, or none), stored at dst[n - 1]
 * (the 16-element chunk that holds it is formed: dst[16 ((n - 1) / 16) .. n)); n == 0: none.  Done by the launch's first blocks
 * before their share of the update; the arithmetic of mg_expand_column_reduce_f32. */
typedef struct {
    const float* table;
    const int32_t* rows;
    int64_t frames;
    float* out;
    const float* partial;
    int n_partial;
    const float* slab;
    int64_t n, stride;
    int n_slabs;
    float* dst;
} mg_adam_tail;
typedef struct {
    int n_slab_srcs;
    mg_adam_slab_src slabs[MG_ADAM_MAX_SLABS];
    int n_shadows;
    mg_adam_shadow shadows[MG_ADAM_MAX_SHADOWS];
    int clear_grad;
    mg_adam_tail tail;
} mg_adam_plan;
int mg_adam_step_plan_f32(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1, float beta2, float eps,
                          float weight_decay, const float* scalars, float grad_scale, const mg_adam_plan* plan, void* stream);
/* shadow -= (1 - decay) * (shadow - param). */
int mg_ema_update_f32(float* shadow, const float* param, int64_t n, float decay, void* stream);

/* ----------------------------------------------------------------------------------------------------------------
 * K21 (csrc/clip.hip)  global gradient-norm clipping over flat fp32 gradient buffers:
 *                      torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2, error_if_nonfinite=False)
 * Two launches per buffer and step, the norm never read by the host.  A buffer of n floats is cut into mg_grad_clip_blocks(n)
 * contiguous chunks of mg_grad_clip_chunk(n) floats (from n alone: at most MG_CLIP_MAX_BLOCKS chunks, a multiple of 1024 floats
 * each, at least 4096), one workgroup per chunk in both launches.
 * ---------------------------------------------------------------------------------------------------------------- */
#define MG_CLIP_MAX_BLOCKS 1024
#define MG_CLIP_MAX_PARTIALS 16384
int64_t mg_grad_clip_chunk(int64_t n);
int mg_grad_clip_blocks(int64_t n);
/* partials[offset + c] = sum of squares of chunk c of grad, accumulated in float64 in a fixed order (no atomics: the same bits on
 * every call).  partials holds n_partials doubles - one array for all buffers that share a norm, each with its own offset.  grad
 * need only be 4-byte aligned (a view into a larger allocation): each chunk reaches 16-byte loads behind a scalar head. */
int mg_grad_sumsq_f32(const float* grad, int64_t n, double* partials, int offset, int n_partials, void* stream);
/* norm = sqrt(sum of all n_partials partials) * inv_world, coef = min(1, max_norm / (norm + 1e-6)), both formed in float64 by every
 * workgroup in the same order and rounded to fp32; grad *= coef in place (not written at all when coef == 1; a NaN norm gives a NaN
 * coef and NaN gradients, an infinite one coef 0, as torch).  out (may be NULL): out[0] = norm, out[1] = coef.  inv_world in
 * (0, 1]: grad holds the SUM over the ranks whose mean the threshold applies to; max_norm > 0. */
int mg_grad_clip_scale_f32(float* grad, int64_t n, const double* partials, int n_partials, double inv_world, double max_norm, float* out,
                           void* stream);

/* ----------------------------------------------------------------------------------------------------------------
 * K22 (csrc/colstats.hip)  per-column corpus statistics for the normaliser parameter files ({name}_mvn.json, {name}_minmax.json,
 *                          their _deltas and per-speaker twins; the reference takes them from the un-vendored tts_data_tools)
 * state (S, MG_COLSTATS_FIELDS, D) float64: count, mean, M2 = sum (x - mean)^2, min, max of every column of every group, updated in
 * place batch after batch; all zeros is the empty state (count == 0: the other fields are ignored).  Shifted float64 chunk sums
 * merged by Chan's update in a fixed order, no float atomics: the same input and state give the same bits.  A NaN or an infinity
 * makes its column's mean and M2 non-finite and is counted; min / max skip NaNs.
 * ---------------------------------------------------------------------------------------------------------------- */
#define MG_COLSTATS_FIELDS 5
#define MG_COLSTATS_MAX_D 2048
/* Bytes of the job records of one call on B items of at most max_rows rows (0 for B <= 0, D outside 1..MG_COLSTATS_MAX_D). */
size_t mg_column_stats_workspace_bytes(int B, int64_t max_rows, int D);
/* x: float32 rows of D columns, row stride ld >= D floats (16-byte loads when ld == D).  Exactly one of
 *   offsets (B + 1, int64): packed - the rows of item b are [offsets[b], offsets[b + 1]); T is unused and the items are cut into
 *                           as many chunks as the workspace holds records for: size it for the longest item
 *                           (any size from mg_column_stats_workspace_bytes(B, 1, D) up is valid),
 *   seq_len (B, int64):     padded (B, T, D) - item b is rows [b T, b T + min(max(seq_len[b], 0), T))
 * is non-NULL.  item_row (B, int32, may be NULL when S == 1): the group of item b; an index outside [0, S) is never used as one -
 * that item contributes to nothing.  Two launches: job records into `workspace`, then the records and the state in job order.
 * B == 0: MG_OK, nothing launched.  MG_EWORKSPACE when the workspace is too small. */
int mg_column_stats_f32(const float* x, int64_t ld, int D, int B, int T, const int64_t* offsets, const int64_t* seq_len,
                        const int32_t* item_row, int S, double* state, void* workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------------------------
 * K23 (csrc/deltas.hip)  delta features: the forward of MLPG's window operator    reference: morgana/viz/synthesis.py:8-36
 *                        (_build_win_mats: output column w*D + d at frame t is row t of W_w applied to column d) - applied nowhere in
 *                        the reference, whose {name}_deltas files come from the un-vendored tts_data_tools (data.py:135-150 loads
 *                        and normalises them); here computed on the device inside the loader's pad-and-normalise pass.
 * Windows as in mg_mlpg_f32: win_l / win_u [W] ints, win_coeff [W][MG_MLPG_MAX_COEFF] doubles, l + u + 1 <= MG_MLPG_MAX_COEFF,
 * 1 <= W <= MG_MLPG_MAX_WINDOWS (host arrays).  out[t, w*D + d] = sum_k coeff[w][k] x[t - l_w + k, d], accumulated in float64,
 * taps in ascending k, rounded once to float32.  A tap outside [0, len) reads the item's first / last frame
 * (MG_DELTAS_EDGE_REPLICATE) or contributes nothing (MG_DELTAS_EDGE_ZERO: exactly W_w of MLPG).
 * Input x, exactly one of
 *   offsets (B + 1, int64): packed [N, D] - the rows of item b are [offsets[b], offsets[b + 1]); T_in is unused,
 *   seq_len (B, int64):     padded [B, T_in, D] - item b is rows [b T_in, b T_in + min(max(seq_len[b], 0), T_in)); later frames are
 *                           never read.
 * Output, raw_out and / or norm_out (either may be NULL), both of the form out_form:
 *   MG_DELTAS_OUT_PADDED  [B, out_rows, W*D]: an item longer than out_rows frames is cut to out_rows frames first (as
 *                         mg_pad_normalise_f32 cuts it); frames past the length are written as zeros by the same launch,
 *   MG_DELTAS_OUT_PACKED  [out_rows, W*D]: packed input - row r of the output belongs to row r of the input; padded input - the valid
 *                         frames of the items back to back (B <= MG_DELTAS_MAX_SCAN_ITEMS).  Rows that belong to no item, and rows
 *                         from out_rows on, are not written.
 * norm_out = kind (MG_NORM_MVN or MG_NORM_MINMAX) with p0 / p1 [W*D] applied to the rounded float32 value, the arithmetic of
 * mg_normalise_f32; with item_row (B, int32) non-NULL p0 / p1 are tables [S, W*D] and item b takes row item_row[b], as in
 * mg_pad_normalise_items_f32: an index outside [0, S) is never used as one and gives NaN in that item's valid frames.
 * Lengths 0, 1 and 2 are legal.  B == 0: MG_OK, nothing launched.  One launch, no workspace, no atomics; 16-byte accesses when
 * D % 4 == 0 and x, the outputs and the parameters are 16-byte aligned.
 * ---------------------------------------------------------------------------------------------------------------- */
#define MG_DELTAS_EDGE_REPLICATE 0
#define MG_DELTAS_EDGE_ZERO 1
#define MG_DELTAS_OUT_PADDED 0
#define MG_DELTAS_OUT_PACKED 1
#define MG_DELTAS_MAX_SCAN_ITEMS 4096
/* Destination rows of one chunk of the launch for features of D columns (0 for D <= 0): what a test needs to cross a chunk. */
int mg_deltas_chunk_rows(int D);
int mg_deltas_f32(const float* x, int D, int B, const int64_t* offsets, const int64_t* seq_len, int T_in, int n_windows, const int* win_l,
                  const int* win_u, const double* win_coeff, int edge, const float* p0, const float* p1, const int32_t* item_row, int S,
                  int kind, int out_form, int64_t out_rows, float* raw_out, float* norm_out, void* stream);

/* ----------------------------------------------------------------------------------------------------------------
 * K24 (csrc/seqmean.hip)  masked sequence mean of a feature loss: the reduction of losses.sequence_loss
 *                         reference: morgana/losses.py:29-46 (mask from morgana/utils.py:115-144)
 * loss[0] = (1 / (B D)) sum_b ( sum_{t < T, d} x[b,t,d] m[b,t] ) / n_b,  m[b,t] = (t < n_b),  n_b = min(max(seq_len[b], 0), T), or
 * T when seq_len is NULL (the rules of mg_masked_mse_f32).  x is float32, element (b, t, d) at x[b stride_b + t stride_t +
 * d stride_d] (element strides, not negative; 0 = an expanded operand): a column slice, a misaligned base and a stride-0 operand are
 * read in place.  Every frame is read and multiplied by its mask value: a NaN or Inf in a pad frame makes the loss NaN, and n_b == 0
 * gives NaN.  Accumulated in float64: one partial per (utterance, chunk of the (t, d) index space) in the workspace, summed in a
 * fixed order by a one-workgroup finish, divided by n_b in float64, rounded to float32 once.  The order depends on the logical index
 * alone: the same bits on every call, for every stride pattern and alignment of the same values.  No atomics, no host read.  Rows with
 * stride_d == 1 and stride_t == D take 16-byte loads at aligned addresses behind a scalar head and tail; anything else takes one
 * element per load.  workspace: mg_seq_mean_workspace_bytes(B, T, D) bytes (0 for a shape that is not positive), 8-byte aligned;
 * MG_EWORKSPACE when it is NULL or too small.
 *
 * Backward, one launch: grad [B, T, D] float32, contiguous; grad[b,t,d] = (float)((double)grad_loss[0] / ((double)n_b B D)) for
 * t < n_b, 0 for the pad frames of an utterance with n_b > 0, NaN on every frame of an utterance with n_b == 0 (the reference's
 * 0 * inf).  grad_loss is the upstream gradient, one float32 ON THE DEVICE.  16-byte stores behind a scalar head and tail.
 * mg_seq_mean_chunk(): elements of one utterance per workgroup, what a test needs to cross a chunk.
 * ---------------------------------------------------------------------------------------------------------------- */
int mg_seq_mean_chunk(void);
size_t mg_seq_mean_workspace_bytes(int B, int T, int D);
int mg_seq_mean_f32(const float* x, int64_t stride_b, int64_t stride_t, int64_t stride_d, const int64_t* seq_len, int B, int T, int D,
                    float* loss, void* workspace, size_t workspace_bytes, void* stream);
int mg_seq_mean_bwd_f32(const float* grad_loss, const int64_t* seq_len, int B, int T, int D, float* grad, void* stream);

/* ----------------------------------------------------------------------------------------------------------------
 * K26 (csrc/gv.hip)  global-variance loss: the per-utterance variance of a trajectory against that of the natural one
 *                    (Toda & Tokuda 2007); the reference has no such loss.
 * With n_b = min(max(seq_len[b], 0), T) (T when seq_len is NULL), over the valid frames t < n_b of utterance b and column d:
 *     m[b,d] = mean_t x[b,t,d],   v[b,d] = mean_t (x[b,t,d] - m[b,d])^2   (biased),
 *     f(v) = log(v + eps) if log_variance else v,
 *     loss[0] = (1 / (B D)) sum_{b,d} ( f(v_pred[b,d]) - f(v_tgt[b,d]) )^2.
 * pred / tgt are float32, element (b, t, d) at p[b stride_b + t stride_t + d stride_d] (element strides, not negative; 0 = an
 * expanded operand), read in place.  PAD FRAMES ARE NEVER READ: a NaN there changes nothing.  n_b == 1 gives v == 0; n_b == 0 gives
 * a NaN loss.
 *
 * Forward, two launches.  (1) grid (ceil(T / mg_gv_chunk_frames()), B, 2 operands): one workgroup streams the valid frames of its
 * chunk of pred or of tgt once, as a flat array in steps of W = R D elements (R whole frames, W near 1024 whatever D, so narrow features
 * fill the lanes), and leaves per column (mean - anchor, M2) in float64 in the workspace: shifted chunks of at most 32 values (sum
 * of x - k and of (x - k)^2, k the chunk's first value) folded by Chan's update, the anchor being x[b,0,d].  No sum of raw squares,
 * no atomics.  Rows with stride_d == 1 and stride_t == D whose step is a multiple of 4 take 16-byte loads at aligned addresses
 * whatever the base alignment; anything else takes one element per load.  The order of every sum is a function of (b, t, d) alone:
 * the same bits on every call and for every stride pattern and alignment of the same values.  (2) the finish, one thread per
 * (b, d): merges the chunks in ascending order for both operands, evaluates f in float64, writes state [B, D, 2] float64 =
 * (m_pred, c) with
 *     c[b,d] = (2 / (B D)) (f(v_pred) - f(v_tgt)) f'(v_pred) (2 / n_b)          (NaN for n_b == 0),
 * and sums the loss over (b, d) in a fixed tree: per workgroup of 256 items, then - by the workgroup that arrives last, found by one
 * integer ticket per workgroup, nobody waiting - over the workgroups in index order; rounded to float32 once.  v_pred / v_tgt [B, D] float32 (either may be NULL)
 * receive the variances.  tgt == NULL: only v_pred is computed (it must be given); loss and state are not touched.
 * D <= MG_GV_MAX_D.  workspace: mg_gv_workspace_bytes(B, T, D) bytes (0 for a shape that is not positive), 8-byte aligned;
 * MG_EWORKSPACE when it is NULL or too small.  No host read; capturable.
 *
 * Backward, one launch: grad [B, T, D] float32, contiguous; grad[b,t,d] = (float)(g c[b,d] (x[b,t,d] - m_pred[b,d])) in float64
 * with one rounding for t < n_b, 0 on the pad frames of an utterance with n_b > 0 (they are not read), NaN on every frame of an
 * utterance with n_b == 0.  g = grad_loss[0], one float32 ON THE DEVICE; pred is read in place through its strides.  16-byte
 * stores behind a scalar head and tail.
 * mg_gv_chunk_frames(): frames of one utterance per workgroup of launch (1), what a test needs to cross a chunk.
 * ---------------------------------------------------------------------------------------------------------------- */
#define MG_GV_MAX_D 2048
int mg_gv_chunk_frames(void);
size_t mg_gv_workspace_bytes(int B, int T, int D);
int mg_gv_f32(const float* pred, int64_t pred_stride_b, int64_t pred_stride_t, int64_t pred_stride_d, const float* tgt,
              int64_t tgt_stride_b, int64_t tgt_stride_t, int64_t tgt_stride_d, const int64_t* seq_len, int B, int T, int D,
              int log_variance, double eps, float* loss, double* state, float* v_pred, float* v_tgt, void* workspace,
              size_t workspace_bytes, void* stream);
int mg_gv_bwd_f32(const float* grad_loss, const double* state, const float* pred, int64_t pred_stride_b, int64_t pred_stride_t,
                  int64_t pred_stride_d, const int64_t* seq_len, int B, int T, int D, float* grad, void* stream);

/* ----------------------------------------------------------------------------------------------------------------
 * K28 (csrc/vq.hip)  vector quantisation for VQ-VAE latents, functional.VQFn (van den Oord et al. 2017); the reference has no discrete
 *                    latent.
 * z: N rows of D float32, row n at z + n ldz (ldz >= D, in elements): a column slice of a wider tensor and a base that is only
 * 4-byte aligned are read in place.  codebook [K, D] float32, contiguous.  seq_len NULL: every row counts.  seq_len [B] int64 with
 * N = B S: row b S + s counts when s < min(max(seq_len[b], 0), S); the other rows are NEVER READ, get index -1 and a zero
 * quantised row and stay out of every mean and count.  With
 *     d[n,k] = sum_d ( (double)z[n,d] - (double)E[k,d] )^2       (ascending d, float64, the direct difference, no contraction),
 * index[n] [N] int64 is the smallest k that attains min_k d[n,k] (a NaN distance never wins; a row whose distances are all NaN
 * gets code 0 and makes vq NaN), quantised [N, D] float32 is codebook[index[n]] bit for bit, vq[0] = sum_n d[n,index[n]] /
 * (N_valid D) summed in float64 in an order fixed by n alone and rounded once, counts [K] int32 the number of rows per code,
 * perplexity[0] = exp(-sum_k p_k ln p_k) with p_k = counts[k] / N_valid in float64, n_valid[0] (int64) = N_valid, which
 * mg_vq_bwd_f32 reads.  N_valid == 0: vq and perplexity are NaN.  Three launches (one wave per row over codebook tiles of
 * mg_vq_tile_codes(D) codes in LDS; a counting pass, one thread per code; a one-workgroup finish), no atomics, no host read:
 * the same bits on every call, capturable.  K <= MG_VQ_MAX_CODES, D <= MG_VQ_MAX_DIM, N <= MG_VQ_MAX_ROWS (MG_EINVAL otherwise,
 * nothing launched).  workspace: mg_vq_workspace_bytes(N, K) bytes (0 for a shape that is refused), 8-byte aligned; MG_EWORKSPACE
 * when it is NULL or too small.
 *
 * mg_vq_bwd_f32, with g = g_loss[0] (one float32 ON THE DEVICE) and z, quantised, index, n_valid as the assignment left them:
 *     dz[n,d] = (float)( g_lat[n,d] + g commitment_weight 2 (z[n,d] - q[n,d]) / (N_valid D) )      0 on rows with index -1,
 *     dE[k,d] = (float)( g codebook_weight 2 sum_{n: index[n] = k} (q[n,d] - z[n,d]) / (N_valid D) )
 * (q[n] is the code as the assignment read it: the codebook itself is not an argument and may have changed since), the members
 * summed in ascending n in float64 and rounded once; a code without members gets exactly 0.  g_lat [N, D] may be NULL (zeros);
 * dz [N, D] or dE [K, D] may be NULL: that part is skipped (not both).  One launch each, no atomics.
 *
 * mg_vq_ema_f32, the EMA codebook of the paper's appendix, in place (counts as the assignment left them):
 *     cluster_size[k] <- (float)( decay n_k + (1 - decay) counts[k] ),     total = sum_k of the new sizes (float64, fixed order),
 *     ema_sum[k,d]    <- (float)( m = decay m_kd + (1 - decay) sum_{n: index[n] = k} z[n,d] )      (ascending n, float64),
 *     codebook[k,d]   <- (float)( m / ( (cluster_size[k] + eps) / (total + K eps) total ) )        (left as it is when total == 0).
 * cluster_size [K], ema_sum [K, D], codebook [K, D] float32.  Two launches; workspace: 8 bytes (one float64), 8-byte aligned.
 * ---------------------------------------------------------------------------------------------------------------- */
#define MG_VQ_MAX_CODES 65536
#define MG_VQ_MAX_DIM 256
#define MG_VQ_MAX_ROWS 16777216
int mg_vq_tile_codes(int D);
size_t mg_vq_workspace_bytes(int64_t N, int K);
int mg_vq_assign_f32(const float* z, int64_t ldz, int64_t N, int D, const int64_t* seq_len, int S, const float* codebook, int K,
                     int64_t* index, float* quantised, float* vq, int32_t* counts, float* perplexity, int64_t* n_valid, void* workspace,
                     size_t workspace_bytes, void* stream);
int mg_vq_bwd_f32(const float* g_lat, const float* g_loss, const float* z, int64_t ldz, const float* quantised, const int64_t* index,
                  const int64_t* n_valid, int64_t N, int D, int K, double codebook_weight, double commitment_weight, float* dz, float* dE,
                  void* stream);
int mg_vq_ema_f32(const float* z, int64_t ldz, const int64_t* index, const int32_t* counts, int64_t N, int D, int K, double decay, double eps,
                  float* cluster_size, float* ema_sum, float* codebook, void* workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------------------------
 * K29 (csrc/f0.hip)  continuous log-F0 and voicing from a raw F0 track: the `lf0` and `vuv` features every F0 model of the reference
 *                    reads (models/f0_test_model.py, models/RNN_SPSS.py), which it gets as files from the un-vendored tts_data_tools;
 *                    here computed on the device inside the loader, in front of mg_deltas_f32 and mg_column_stats_f32.
 * Per item of n frames and per column d (columns are independent):
 *     voiced[t] = x[t,d] > voiced_above                     (a NaN is unvoiced)
 *     l[t]      = log((double)x[t,d]), or (double)x[t,d] when log_input != 0 (the track is a log-F0 track already)
 *     lf0[t,d]  = (float)l[t] on a voiced frame; on an unvoiced frame between the nearest voiced frames a < t < b
 *                 (float)( l[a] + (l[b] - l[a]) * w ), w = (double)(t - a) / (double)(b - a), in float64 in this order without
 *                 contraction, rounded once; (float)l[b] with no voiced frame before t, (float)l[a] with none after (np.interp's
 *                 convention); `fill` on every frame of an item without a voiced frame
 *     vuv[t,d]  = 1.0f on a voiced frame, else 0.0f.
 * A voiced value that is not finite, or whose logarithm is not, propagates by the formula.
 * Input x, exactly one of
 *   offsets (B + 1, int64): packed [N, D] - the rows of item b are [offsets[b], offsets[b + 1]); T_in is unused,
 *   seq_len (B, int64):     padded [B, T_in, D] - item b is rows [b T_in, b T_in + min(max(seq_len[b], 0), T_in)); later frames are
 *                           never read.
 * Outputs, each may be NULL (not all):
 *   packed_out [packed_rows, D]: lf0, row offsets[b] + t (packed input) or (the clamped lengths of the items before b) + t (padded
 *                                input); rows that belong to no item, and rows from packed_rows on, are not written - what
 *                                mg_deltas_f32 and mg_column_stats_f32 read next,
 *   padded_out [B, out_rows, D]: lf0; frames from out_rows on are not written (the interpolation still sees the whole item), frames
 *                                past the length are written as exact zeros by the same launch,
 *   norm_out   [B, out_rows, D]: kind (MG_NORM_MVN or MG_NORM_MINMAX) with p0 / p1 [D] applied to the rounded float32 lf0, the
 *                                arithmetic of mg_normalise_f32, zeros past the length; with item_row (B, int32) non-NULL p0 / p1 are
 *                                tables [S, D] and item b takes row item_row[b]: an index outside [0, S) is never used as one and
 *                                gives NaN in that item's valid frames,
 *   vuv_out: vuv_form MG_F0_VUV_PADDED - [B, out_rows, D] as padded_out; MG_F0_VUV_PACKED - [packed_rows, D] as packed_out.
 * Lengths 0, 1 and 2 are legal.  B == 0: MG_OK, nothing launched.  One launch (one workgroup per item, a wave per 64-frame segment,
 * neighbours by ballot), no workspace, no atomics, no host read: the same bits on every call, capturable.
 * mg_continuous_lf0_chunk_rows(): frames of one column a workgroup takes per trip, what a test needs to cross a chunk.
 * ---------------------------------------------------------------------------------------------------------------- */
#define MG_F0_VUV_PADDED 0
#define MG_F0_VUV_PACKED 1
int mg_continuous_lf0_chunk_rows(void);
int mg_continuous_lf0_f32(const float* x, int D, int B, const int64_t* offsets, const int64_t* seq_len, int T_in, int log_input,
                          float voiced_above, float fill, const float* p0, const float* p1, const int32_t* item_row, int S, int kind,
                          int64_t out_rows, int64_t packed_rows, float* packed_out, float* padded_out, float* norm_out, float* vuv_out,
                          int vuv_form, void* stream);

/* ----------------------------------------------------------------------------------------------------------------
 * K27  ragged segment pooling (csrc/segpool.hip): utils.pool_segments, frames -> phone / syllable / word / utterance rate.
 *
 *   out[b, s, f] = pool over t in [start_s, min(start_s + max(len_s, 0), n_b)) of x[b, t, f],   start_s = sum_{j < s} max(len_j, 0),
 *   n_b = min(max(seq_len[b], 0), T) (seq_len NULL: T).  x f32 [B, T, F] read in place through its strides (elements; none negative):
 *   16-byte loads when stride_f == 1, F % 4 == 0, x is 16-byte aligned and stride_t, stride_b are multiples of 4, else 4-byte loads,
 *   the same bits either way.  seg_lens int64 [B, S] (a negative length counts as 0), out f32 [B, S, F] contiguous.
 *   mode: MG_POOL_SUM / MG_POOL_MEAN - a float64 sum (MEAN: divided by the frame count m in float64) rounded to float32 once;
 *         MG_POOL_MAX / MG_POOL_MIN - the value x[b, t*, f] bit for bit, t* the lowest frame that holds the extremum, or the lowest
 *         NaN frame if there is one; arg int32 [B, S, F] (required for these two modes, unused otherwise) takes t*.
 *   An empty range (m == 0) gives +0 and arg -1.  A frame outside every range is never read.  Segments are reduced in chunks of
 *   mg_segment_pool_chunk() frames counted from the segment's own first frame, merged in ascending order: the order of operations
 *   depends on m and the position inside the segment alone.  One launch, no workspace, no atomics, no host read: the same bits on
 *   every call, capturable.
 * mg_segment_pool_bwd_f32: the dense gradient grad f32 [B, T, F] (contiguous) from grad_out f32 [B, S, F] (contiguous), every element
 *   written exactly once by one launch: SUM g, MEAN (float)((double)g / m), MAX / MIN g where arg[b, s, f] == t and +0 elsewhere,
 *   +0 on every frame outside all ranges.  arg: what the forward wrote (MAX / MIN only).
 * Refused (MG_EINVAL, nothing launched): an unknown mode, F < 1, a negative size or stride, B > 65535, S > 12288, a NULL or misaligned
 *   pointer where one is read or written.  Zero work (forward: B == 0 or S == 0; backward: B == 0 or T == 0): MG_OK, no launch.
 * ---------------------------------------------------------------------------------------------------------------- */
#define MG_POOL_SUM 0
#define MG_POOL_MEAN 1
#define MG_POOL_MAX 2
#define MG_POOL_MIN 3
int mg_segment_pool_chunk(void);
int mg_segment_pool_f32(const float* x, int64_t stride_b, int64_t stride_t, int64_t stride_f, const int64_t* seg_lens, const int64_t* seq_len,
                        int B, int S, int T, int F, int mode, float* out, int32_t* arg, void* stream);
int mg_segment_pool_bwd_f32(const float* grad_out, const int64_t* seg_lens, const int64_t* seq_len, const int32_t* arg, int B, int S, int T,
                            int F, int mode, float* grad, void* stream);

/* ----------------------------------------------------------------------------------------------------------------
 * K30 (csrc/counters.hip)  frame-level positional features from durations: the `counters` feature the acoustic models of the reference
 *                          read (models/RNN_SPSS.py:65), which it gets as files from the un-vendored tts_data_tools; here computed on
 *                          the device inside the loader from the durations it uploads anyway.
 * dur int64, logical [B, P, S], read in place through its element strides (none negative): P phones of S sub-phone states (S = 1: a
 * phone-level alignment).  A negative duration owns no frame.  n_phones (B, int64) or NULL: the phones from n_phones[b] on count as
 * absent (NULL: all P count).  With start[p,s] = the sum of the durations before (p, s) in (p, s) order, n_s = dur[p,s],
 * n_p = sum_s dur[p,s], and for frame t of the one segment with start <= t < start + n_s:  i = t - start[p,s],  j = t - start[p,0]:
 *   MG_COUNTERS_FULL   C = 9:  (i+1)/n_s, (n_s-i)/n_s, n_s, s+1, S-s, n_p, n_s/n_p, (n_p-j)/n_p, (j+1)/n_p      (Merlin's 'full')
 *   MG_COUNTERS_PHONE  C = 3:  (j+1)/n_p, (n_p-j)/n_p, n_p                                             (Merlin's 'minimal_phoneme')
 * every quotient one float64 division of the two integers rounded once to float32 (below 2^24 frames per phone: the correctly rounded
 * float32 of the exact rational), integer columns converted directly.  An item whose durations add up to 2^31 or more is outside the
 * contract: the scan saturates (nothing is read or written out of bounds).
 * Outputs, either may be NULL (not both):
 *   raw_out  [B, T, C]: frames t < min(T, total_b, seq_len[b] if seq_len != NULL) hold the counters (total_b: the sum of the item's
 *                       durations that count), every other frame exact zeros, written by the same launch,
 *   norm_out [B, T, C]: norm_kind (MG_NORM_MVN or MG_NORM_MINMAX) with p0 / p1 [C] applied to the rounded float32 value, the
 *                       arithmetic of mg_normalise_f32, zeros on the other frames; with item_row (B, int32) non-NULL p0 / p1 are tables
 *                       [n_rows, C] and item b takes row item_row[b]: an index outside [0, n_rows) is never used as one and gives NaN
 *                       in that item's valid frames.
 * blocks_per_item: workgroups that share the T * C output elements of an item, each repeating the item's scan; 0: the library's
 * choice (one per 768 elements).  The bits do not depend on it.
 * Refused (MG_EINVAL, nothing launched): an unknown kind, P < 1, S < 1, P * S > 12288 (the scan lives in LDS), a negative size or
 * stride, no output, a normalised output without parameters or kind.  B == 0 or T == 0: MG_OK, nothing launched.  One launch, no
 * workspace, no atomics, no host read: the same bits on every call, capturable.
 * ---------------------------------------------------------------------------------------------------------------- */
#define MG_COUNTERS_FULL 0
#define MG_COUNTERS_PHONE 1
#define MG_COUNTERS_FULL_COLS 9
#define MG_COUNTERS_PHONE_COLS 3
int mg_frame_counters_f32(const int64_t* dur, int B, int P, int S, int64_t stride_b, int64_t stride_p, int64_t stride_s, const int64_t* n_phones,
                          const int64_t* seq_len, int T, int counters_kind, const float* p0, const float* p1, const int32_t* item_row, int n_rows,
                          int norm_kind, float* raw_out, float* norm_out, int blocks_per_item, void* stream);

/* ----------------------------------------------------------------------------------------------------------------
 * K31 (csrc/durations.hip)  integer durations from a duration model's real-valued prediction: the quantiser between
 *                           models.DurationModel and everything that takes `dur` (K30, the upsampling kernels, the acoustic models).
 * pred f32, logical [B, P, S], read in place through its element strides (none negative): P phones of S sub-phone states, in the
 * normalised space.  n_phones (B, int64) or NULL: the phones from n_phones[b] on are never read and their outputs are 0 (NULL: all P
 * count).  p0 / p1 [S] (mean, std_dev of the `dur` normaliser) or NULL (pred is in frames already); with item_row (B, int32) non-NULL
 * they are tables [n_rows, S] and item b takes row item_row[b]: an index outside [0, n_rows) is never used as one, the item's outputs
 * are all 0 and its flags MG_DUR_FLAG_NO_ROW alone.  Segments i = 0 .. n-1 in (p, s) order over the item's valid phones:
 *   x_i = (double)pred * (double)p1[s] + (double)p0[s]  (one rounding);  exp(x_i) if log_input;  x_i * scale;
 *         a NaN, infinite or negative x_i becomes 0 and sets MG_DUR_FLAG_INVALID;  min(x_i, hi)
 *   q_i = floor(x_i * 65536 + 0.5) as int64: 16 fractional bits, everything below is integer arithmetic
 *   total (B, int64) non-NULL, the length to fit item b to:  Q = sum_i q_i;  if Q > 0 and total[b] > 0
 *         q_i = min(floor((double)q_i * ((double)(total[b] << 16) / (double)Q) + 0.5), hi << 16),  else MG_DUR_FLAG_NO_FIT and no fit
 *   MG_DUR_NEAREST  d_i = max(lo, (q_i + 32768) >> 16): every segment rounded on its own (Merlin's rule)
 *   MG_DUR_CARRY    C_i = q_0 + .. + q_i,  R_i = (C_i + 32768) >> 16,  E_i = (i+1) lo + max(0, max_{j<=i}(R_j - (j+1) lo)),
 *                   d_i = E_i - E_{i-1}, E_{-1} = 0: the closed form of "emit max(lo, R_i - the frames emitted so far)".
 *                   lo <= d_i <= max(lo, hi).  Where every clamped x_i >= lo the total is (C_{n-1} + 32768) >> 16 and every boundary
 *                   lies within half a frame of C_i / 65536; MG_DUR_FLAG_PUSHED: E_{n-1} differs from that total (the minimum
 *                   pushed the length out).
 * Outputs: dur int64 [B, P, S] contiguous, phone_dur int64 [B, P] = sum_s dur, n_frames int64 [B] = sum dur, flags int32 [B].
 * One workgroup per item walks its segments in chunks of 256 with a carried int64 sum and maximum: integer scans, so the bits depend
 * on the values alone.  One launch, no workspace, no atomics, no host read: the same bits on every call, capturable.
 * Refused (MG_EINVAL, nothing launched): an unknown rounding, P < 1, S < 1, B > 65535, P * S >= 2^24, a negative size or stride,
 * not 0 <= lo <= hi <= 2^20, a scale that is not positive and finite, one of p0 / p1 without the other, item_row without tables, a
 * NULL or misaligned pointer where one is read or written.  B == 0: MG_OK, nothing launched.
 * ---------------------------------------------------------------------------------------------------------------- */
#define MG_DUR_CARRY 0
#define MG_DUR_NEAREST 1
#define MG_DUR_FLAG_INVALID 1
#define MG_DUR_FLAG_NO_FIT 2
#define MG_DUR_FLAG_PUSHED 4
#define MG_DUR_FLAG_NO_ROW 8
#define MG_DUR_MAX_FRAMES 1048576
int mg_quantise_durations_f32(const float* pred, int B, int P, int S, int64_t stride_b, int64_t stride_p, int64_t stride_s,
                              const int64_t* n_phones, const float* p0, const float* p1, const int32_t* item_row, int n_rows, int log_input,
                              double scale, int64_t lo, int64_t hi, int rounding, const int64_t* total, int64_t* dur, int64_t* phone_dur,
                              int64_t* n_frames, int32_t* flags, void* stream);

/* ----------------------------------------------------------------------------------------------------------------
 * K32 (csrc/vocoder.hip)  vocoder features: the three arrays a WORLD-style synthesiser takes (f0, spectral envelope, aperiodicity)
 *                         from what the acoustic models generate (lf0, vuv, mcep, bap) - models/RNN_SPSS.py:141-161 up to the
 *                         call of the synthesiser, which stays the user's.
 * All inputs are float32.  Input x of `width` floats per frame, exactly one of
 *   offsets (B + 1, int64): packed [N, width] - the rows of item b are [offsets[b], offsets[b + 1]); T_in is unused,
 *   seq_len (B, int64):     padded [B, T_in, width] - item b is rows [b T_in, b T_in + min(max(seq_len[b], 0), T_in)); later frames
 *                           are never read; at most MG_VOC_MAX_ITEMS items (their first packed rows are scanned in LDS).
 * Output out, PACKED [packed_rows, cols]: frame t of item b is row offsets[b] + t (packed input) or (the clamped lengths of the items
 * before b) + t (padded input); rows that belong to no item, and rows from packed_rows on, are not written.  out_f64 == 0: float;
 * else double, holding (double)value of the same float32 result (a vocoder's float64 arrays without a host conversion pass).
 * B == 0 or packed_rows == 0: MG_OK, nothing launched.  One launch each, no workspace, no atomics, no host read: the same bits on
 * every call, capturable.
 *
 * mg_mcep_spectrum_f32: mel-cepstrum (M = 1 .. MG_VOC_MAX_ORDER coefficients per frame) -> power spectrum, cols = K = F / 2 + 1,
 *   F a power of two in [8, 8192]:
 *     L[t,k]  = sum_{m < M} c[t,m] basis[m,k]          float32, fmaf in ascending m from 0 (one rounding per term)
 *     sp[t,k] = expf(2 L[t,k]),  or 2 L[t,k] itself with log_out != 0
 *   basis f32 [M, ldb], ldb >= K: the caller's table basis[m,k] = cos(m w~_k), w_k = 2 pi k / F,
 *   w~ = w + 2 atan(alpha sin w / (1 - alpha cos w)) (the all-pass warp; alpha = 0: a plain cosine sum), built in float64 and rounded
 *   once; the kernel computes no cosine.  This closed form agrees with SPTK's freqt(-alpha) followed by a cosine sum at order F / 2 to
 *   1.5e-14 (checked on the host at (60, 0.77, 2048)); whether the un-vendored tts_data_tools called exactly that could not be verified.
 *   Non-finite cepstra propagate by the formula.  |L^ - L| <= (M + 1) 2^-24 sum_m |c[t,m]|.
 *   Lanes run along bins (a wave stores 64 consecutive bins), a thread holds its basis column in registers, a frame's cepstra are
 *   wave-uniform scalar operands.  mg_vocoder_tile_frames() / mg_vocoder_tile_bins(): packed rows / bins of one tile.
 *
 * mg_bap_aperiodicity_f32: coded band aperiodicity in dB (Nb columns, band i centred at 3000 i Hz) -> full-band aperiodicity,
 *   cols = K = F / 2 + 1; Nb >= 1 and 3000 Nb < fs / 2 (fs in Hz), anything else is refused.  Each coded value is clamped to [-60, 0]
 *   (a NaN stays a NaN): above 0 dB the aperiodicity would exceed 1 and WORLD takes sqrt(1 - ap^2).  Anchors (0 Hz, -60 dB),
 *   (3000 i Hz, bap[t,i-1]) for i = 1 .. Nb, (fs / 2, 0 dB); at f_k = k fs / F between anchors (f_lo, a) and (f_hi, b), the segment
 *   min(floor(f_k / 3000), Nb):
 *     w = (float)((f_k - f_lo) / (f_hi - f_lo))  in float64, rounded once
 *     dB = fmaf(b - a, w, a);   ap[t,k] = expf(dB * (float)(ln 10 / 20))
 *   Bin 0 is 10^-3, bin F / 2 is 1, a bin on an anchor returns that anchor's value.  This is WORLD's decode_aperiodicity (linear
 *   interpolation of the coded dB values over frequency, floor -60 dB) as its source is remembered; it could not be checked against
 *   pyworld, which is not installed where this was written.
 *
 * mg_smooth_f0_f32: log-F0 and voicing [.., D] -> a gated, smoothed F0, cols = D.  Per item of n frames and per column, in float64:
 *     y[t] = exp((double)lf0[t]);   window = w odd in [1, MG_VOC_MAX_WINDOW], h = (w - 1) / 2
 *     w >= 3 and n >= w:  h <= t < n - h:  s[t] = (y[t-h] + .. + y[t+h]) / w, summed in ascending order
 *                         the first / last h frames, i = t - base with base = 0 / n - w and y_j = y[base + j]:
 *                           s[t] = (sum_j y_j) / w + (i - h) * ((sum_j (j - h) y_j) / (sum_j (j - h)^2))
 *                         which is scipy.signal.savgol_filter(y, w, 1) in its default 'interp' mode (checked to 2e-15)
 *     w == 1 or n < w:    s[t] = y[t] (scipy raises there)
 *     f0[t] = vuv[t] > threshold ? (float)s[t] : 0            (a NaN vuv is unvoiced; a NaN threshold is refused)
 *   The window never reaches a neighbouring item.  One workgroup per item, chunks of mg_smooth_f0_chunk_rows() frames with a halo
 *   of h frames in LDS.
 * Refused (MG_EINVAL, nothing launched): both or neither of offsets and seq_len, F not a power of two in range, M outside
 *   [1, MG_VOC_MAX_ORDER], ldb < K, 3000 Nb >= fs / 2, an even or out-of-range window, D < 1, a negative size, a NULL out, a NULL or
 *   misaligned pointer where one is read or written.
 * ---------------------------------------------------------------------------------------------------------------- */
#define MG_VOC_MAX_ORDER 128
#define MG_VOC_MAX_WINDOW 65
#define MG_VOC_MAX_ITEMS 4096
int mg_vocoder_tile_frames(void);
int mg_vocoder_tile_bins(void);
int mg_smooth_f0_chunk_rows(void);
int mg_mcep_spectrum_f32(const float* mcep, int M, int B, const int64_t* offsets, const int64_t* seq_len, int T_in, const float* basis,
                         int64_t ldb, int F, int log_out, int out_f64, int64_t packed_rows, void* out, void* stream);
int mg_bap_aperiodicity_f32(const float* bap, int Nb, int B, const int64_t* offsets, const int64_t* seq_len, int T_in, int fs, int F,
                            int out_f64, int64_t packed_rows, void* out, void* stream);
int mg_smooth_f0_f32(const float* lf0, const float* vuv, int D, int B, const int64_t* offsets, const int64_t* seq_len, int T_in, int window,
                     float threshold, int out_f64, int64_t packed_rows, void* out, void* stream);

/* ----------------------------------------------------------------------------------------------------------------
 * K33 (csrc/analysis.hip)  vocoder analysis, the opposite direction of K32: what an analyser such as WORLD gives per frame - a power
 *                          spectrum and a full-band aperiodicity, K = F / 2 + 1 bins each - coded into the mel-cepstrum and the
 *                          band aperiodicity the models are trained on.  The waveform analysis itself stays the user's.
 * The input conventions are K32's: input x of K elements per frame, exactly one of offsets (B + 1, int64; packed [N, K]) and seq_len
 * (B, int64; padded [B, T_in, K], at most MG_VOC_MAX_ITEMS items, frames past the clamped length are never read); output PACKED
 * [packed_rows, cols], rows of no item and rows from packed_rows on are not written; B == 0 or packed_rows == 0: MG_OK, nothing
 * launched.  One launch each, no workspace, no atomics, no host read: the same bits on every call, capturable.
 * New in this family: the INPUT is float (in_f64 == 0) or double (in_f64 != 0) - analysers write float64; out_f64 chooses the output.
 *
 * mg_spectrum_mcep: power spectrum -> M = 1 .. MG_VOC_MAX_ORDER mel-cepstral coefficients, cols = M, F a power of two in [8, 8192]:
 *     l[t,k] = 0.5 * log((double)sp[t,k])       (log_in != 0: 0.5 * (double)x[t,k]; x is what mg_mcep_spectrum_f32 writes with log_out)
 *     c[t,m] = sum_{k < K} table[m,k] * l[t,k]   in float64; every product and every addition rounded at most once, in one fixed
 *                                                order (the float64 matrix instruction, K taken in ascending groups of four)
 *     out    = out_f64 ? c : (float)c            one rounding: the float32 output is bit for bit the float64 output rounded
 *   |c^ - c| <= (2K + 8) 2^-53 sum_k |table[m,k]| |l[t,k]| (the dot product in any order, one rounding per table entry, 2 ulp of log).
 *   table f64 [M, ldt], ldt >= K, is the caller's; the kernel computes no cosine and runs no recursion.  It is the composition of two
 *   linear maps, built on the host in float64:
 *     cepstrum   g_n = (kappa_n / F) [l_0 + (-1)^n l_{F/2} + 2 sum_{k=1}^{F/2-1} l_k cos(2 pi n k / F)],  n = 0 .. F/2,
 *                kappa_n = 1 for n in {0, F/2}, else 2: the one-sided cepstrum, l_k = sum_n g_n cos(n w_k) exactly on the grid;
 *     freqt      SPTK's frequency transform from order F/2 to order M - 1 with alpha: c~ = 0; for i = F/2 down to 0: d = c~;
 *                c~_0 = g_i + alpha d_0;  c~_1 = (1 - alpha^2) d_0 + alpha d_1;  c~_j = d_{j-1} + alpha (d_j - c~_{j-1}) for j >= 2.
 *   The composition is the left inverse of K32's basis, table . basis(M, alpha, F)^T = I_M, to 2e-15 at (60, .77, 2048), (25, .58,
 *   1024), (60, .58, 1024), (40, .42, 512), and agrees with the two-step route (irfft, then the recursion per frame) to 4e-15;
 *   max_m sum_k |table[m,k]| is about 1.3.  The identity does NOT hold where the warped series aliases - (128, .77, 2048): 6e-4,
 *   (5, .58, 16): 0.65 - which is a property of the truncated transform, not an error: such settings are held to the two-step route.
 *   This is pysptk.sp2mc as its source is remembered (irfft of the log power spectrum, c[0] halved, freqt); it could not be checked
 *   against pysptk, which is not installed where this was written.
 *   Non-finite and non-positive bins propagate by the formula (log(0) = -inf, log of a negative number is NaN): that frame's
 *   coefficients come out non-finite and no other frame changes.  Nothing at or past sp[t, K) of a row is read as an operand: the
 *   dead slots of the last group of four enter as exact zeros on both operands.
 *   mg_analysis_tile_frames(): packed rows of one workgroup's tile (a wave owns 16 of them).
 *
 * mg_aperiodicity_bap: full-band aperiodicity -> Nb >= 1 coded bands in dB, cols = Nb, 3000 Nb < fs / 2 (fs in Hz): the constraints of
 *   mg_bap_aperiodicity_f32.  Band b (0-based) is anchored at 3000 (b + 1) Hz, bin position 3000 (b + 1) F / fs: in integer arithmetic
 *   k0 the quotient and r the remainder of that division, w = (double)r / (double)fs;
 *     dB(k)    = min(max(20 * log10((double)ap[t,k]), -60), 0)      (a NaN stays a NaN; ap = 0 gives -60)
 *     bap[t,b] = fma(dB(k0 + 1) - dB(k0), w, dB(k0))                in float64, rounded to float once (out_f64: the double itself)
 *   This is WORLD's CodeAperiodicity as remembered (linear interpolation of the dB values at the coarse frequency axis); it could
 *   not be checked against pyworld.  Where every anchor falls on a bin (16 kHz / 1024, 48 kHz / 2048) it inverts
 *   mg_bap_aperiodicity_f32 exactly (1.4e-14 dB in float64); where none does (44.1 kHz / 2048, 22.05 kHz / 1024) the bin pair
 *   straddles the decoder's kink and the round trip is off by up to 0.17 dB.
 * Refused (MG_EINVAL, nothing launched): both or neither of offsets and seq_len, F not a power of two in range, M outside
 *   [1, MG_VOC_MAX_ORDER], ldt < K, 3000 Nb >= fs / 2, a negative size, a NULL out or table, a NULL input where one is read, a
 *   pointer misaligned for its element type.
 * ---------------------------------------------------------------------------------------------------------------- */
int mg_analysis_tile_frames(void);
int mg_spectrum_mcep(const void* sp, int in_f64, int log_in, int F, int B, const int64_t* offsets, const int64_t* seq_len, int T_in,
                     const double* table, int64_t ldt, int M, int out_f64, int64_t packed_rows, void* out, void* stream);
int mg_aperiodicity_bap(const void* ap, int in_f64, int F, int fs, int Nb, int B, const int64_t* offsets, const int64_t* seq_len,
                        int T_in, int out_f64, int64_t packed_rows, void* out, void* stream);

/* ----------------------------------------------------------------------------------------------------------------
 * K34 (csrc/synth.hip)  WORLD-style waveform synthesis: f0 [n], power spectrum sp [n, K] and aperiodicity ap [n, K] in [0, 1],
 *                       K = F / 2 + 1, F a power of two in [MG_SYNTH_MIN_FFT, MG_SYNTH_MAX_FFT], to N samples per utterance.
 * This is WORLD's synthesis.cpp as remembered - pulse positions from the F0 track, a minimum-phase response per pitch pulse, a
 * shaped-noise response per pulse interval, overlap-add; it could not be checked against pyworld, which is not installed where this
 * was written.  Unlike WORLD's newer versions the noise segment's mean is not removed.  All arithmetic is float64, contraction off.
 * tests/synth_ref64.py restates the definition in NumPy.
 *
 * The caller (ops.world_synthesise) owns the plan and describes the batch by int64 device arrays it builds from host-known lengths:
 *   frame_start [B]      first row of utterance b in f0 / sp / ap (packed rows: its offset; padded (B, T, .): b T)
 *   n_frames [B]         n_b
 *   sample_offsets [B+1] prefix sums of N_b = floor((n_b - 1) S) + 1 (n_b >= 1; 0 for n_b = 0), S = fs * frame_period / 1000
 *   region_offsets [B+1] prefix sums of the pulse capacities N_b / 2 + 1: where utterance b's pulse records start
 *   pulse_offsets [B+1]  prefix sums of the pulse counts the pulse kernel reported (read back once): the global pulse numbering g
 *
 * mg_synth_pulses, one workgroup per utterance (n_b < 2: nothing is written - the caller zero-fills counts).  For sample i:
 *     u = i / S, j = min(floor(u), n - 1), j1 = min(j + 1, n - 1), w = u - j;   v_j = f0_j > 0, g_j = v_j ? f0_j : 500
 *     v(i) = v_j (w < .5), v_j1 (w > .5), v_j && v_j1 (w == .5);   f(i) = v(i) ? min(max(g_j + (g_j1 - g_j) w, fs / F), fs / 2) : 500
 *     inc(i) = llrint(f(i) * inc_scale), inc_scale = 2^32 / fs from the host;  Phi(i) = sum_{j <= i} inc(j) in int64
 *   sample i carries a pulse iff (Phi(i) >> 32) > (Phi(i-1) >> 32); delta = (Phi(i) mod 2^32) / inc(i) in [0, 1) is how far before i
 *   the crossing lies; T_m = i_{m+1} - i_m (N - i_m for the last pulse; <= F by the floor fs / F, and by fs <= 500 F, which is
 *   required, where unvoiced); voiced_m = v(i_m).  Records
 *   pulse_idx / pulse_delta / pulse_T / pulse_voiced [region_offsets[b] + m] in ascending m, counts[b] pulses (<= N_b / 2).
 *   Integer scan: the same pulses on every call and in any chunking.
 *
 * mg_synth_responses, one workgroup per pulse g of [g_lo, g_hi), 32 F bytes of LDS (mg_synth_lds_bytes).  At pulse m of utterance b:
 *     u = min(max((i_m - delta_m) / S, 0), n - 1) with j, j1, w as above;  s[k] = max(sp_j[k] + (sp_j1[k] - sp_j[k]) w, 0),
 *     a[k] the same interpolation of ap, r[k] = min(max(a[k]^2, 0), 1)                      (a NaN stays a NaN in all of them)
 *     minphase(P): L = .5 ln P, c = irfft(L, F), c^ = c folded (c[0], 2 c[q] for 0 < q < F/2, c[F/2], 0 above), exp(rfft(c^))
 *     voiced:   h = irfft(minphase(s (1 - r) + 1e-12) e^{+2 pi i k delta / F});  x[p] = h[(p - F/2 + 1) mod F];
 *               x -= d sum(x), d[p] = .5 - .5 cos(2 pi (p + 1) / (F + 1)) normalised to sum 1;  x *= sqrt(T_m)
 *     always:   e[t] = z[sample_offsets[b] + i_m + t] for t < T_m, 0 up to F;  G = minphase(s r + 1e-12) where voiced,
 *               minphase(s + 1e-12 + 0 r) where not (0 r: a NaN aperiodicity reaches the response);  irfft(rfft(e) G), placed as x
 *   irfft as numpy.fft: 1 / F, the imaginary parts of bins 0 and F / 2 dropped.  workspace[(g - g_lo) F + p] = periodic + aperiodic
 *   response at time p - F/2 + 1 relative to i_m.  sp, ap: float (x_f64 == 0) or double, read in place.  table f64 [2 F]: (cos, sin)
 *   of 2 pi q / F for q < F / 2, then d[p] (ops.synth_table); z f64: the noise track of the packed samples (mg_synth_noise or the
 *   caller's).  Each real transform is half of an in-place radix-2 complex transform of size F; per transform the l2 error is at most
 *   8 log2(F) 2^-53 of the l2 norm of its input (tests/synth_ref64.py derives the bound of a sample from that).
 *
 * mg_synth_overlap_add, one thread per packed sample: y[i_m + t] += x_m[t + F/2 - 1], t in [-F/2 + 1, F/2], over the pulses of
 *   [g_lo, g_hi) that cover the sample, one addition at a time in ascending m on the value y holds (the caller zero-fills y and walks
 *   the ranges in ascending order: the bits do not depend on how the pulses are cut into ranges).  last != 0: out[s] = y[s] rounded
 *   once to float (out_f64 == 0) or copied (out may be y itself).  An empty range with last is valid (no pulse at all).  No atomics.
 *
 * mg_synth_noise: z[i] = (double) of the float32 N(0, 1) value of flat element i, i < n (the packed sample index), of the noise mapping
 *   of mg_vae_sample_f32 with counter used[0] (int64 on the device, one draw of the step counter per call).
 * Refused (MG_EINVAL, nothing launched): F outside the range or no power of two, B outside [0, MG_SYNTH_MAX_ITEMS], S outside
 *   [1, 2^20], fs outside (0, min(2^20, 500 F)], inc_scale not 2^32 / fs, a bad range, a NULL or misaligned pointer.  B == 0, an empty range (responses)
 *   or no samples: MG_OK, nothing launched.
 * ---------------------------------------------------------------------------------------------------------------- */
#define MG_SYNTH_MIN_FFT 32
#define MG_SYNTH_MAX_FFT 4096
#define MG_SYNTH_MAX_ITEMS 65535
size_t mg_synth_lds_bytes(int F);
int mg_synth_noise(double* z, int64_t n, uint64_t seed, uint32_t site, const int64_t* used, void* stream);
int mg_synth_pulses(const double* f0, int B, const int64_t* frame_start, const int64_t* n_frames, const int64_t* sample_offsets,
                    const int64_t* region_offsets, double S, double fs, double inc_scale, int F, int32_t* pulse_idx, double* pulse_delta,
                    int32_t* pulse_T, int32_t* pulse_voiced, int64_t* counts, void* stream);
int mg_synth_responses(const void* sp, int sp_f64, const void* ap, int ap_f64, int B, const int64_t* frame_start, const int64_t* n_frames,
                       const int64_t* sample_offsets, const int64_t* region_offsets, const int64_t* pulse_offsets, const int32_t* pulse_idx,
                       const double* pulse_delta, const int32_t* pulse_T, const int32_t* pulse_voiced, const double* z, const double* table,
                       double S, int F, int64_t g_lo, int64_t g_hi, double* workspace, void* stream);
int mg_synth_overlap_add(const double* workspace, int B, const int64_t* sample_offsets, const int64_t* region_offsets,
                         const int64_t* pulse_offsets, const int32_t* pulse_idx, int F, int64_t g_lo, int64_t g_hi, int64_t total_samples,
                         double* y, int last, int out_f64, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MORGANA_HIP_H */
