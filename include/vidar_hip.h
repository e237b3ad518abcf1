/* vidar_hip.h — C ABI of libvidar_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for ViDAR's BEV-encode -> latent-render -> chamfer hot path.
 * Every entry point takes raw DEVICE pointers + plain sizes + a hipStream_t
 * (passed as void*; NULL = the legacy default stream) and returns 0 on success,
 * a positive hipError_t code if a HIP call failed, or VIDAR_ERR_BAD_ARG.
 * No torch types cross this boundary.  All calls are asynchronous on `stream`;
 * unlike the reference (kernels on the legacy default stream followed by
 * cudaDeviceSynchronize(), e.g. third_lib/dvxlr/dvxlr.cu:510) nothing here
 * synchronises the device.  Outputs are written completely by the call
 * (including the -1 / 0 padding the reference obtains from torch::ones/zeros),
 * so callers may pass uninitialised buffers.
 *
 * Citations are file:line under the reference tree (OpenDriveLab/ViDAR @ v2).
 */
#ifndef VIDAR_HIP_H_
#define VIDAR_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIDAR_ERR_BAD_ARG (-22)

/* ABI revision of this header; bumped whenever a signature changes. */
int vidar_abi_version(void);
/* profiling aid: launches the empty kernel `vidar_marker_kernel` on `stream` (see tools/trace_stats.py) */
int vidar_marker(int id, void* stream);

/* Deterministic mode (process-wide, off at load; returns the previous value).  While it is on, the scatter backwards
 * that implement it accumulate in 64-bit fixed point instead of with fp32 atomics (csrc/det_acc.h): their result is a
 * function of the multiset of contributions only -- not of arrival order, launch geometry or kernel variant -- within
 * N_a * delta / 2 + one fp32 rounding of the exact sum per address.  Covered: vidar_msda_bwd_f32 and
 * vidar_msda_fused_bwd_f32 (grad_value; the plain scatter form for every size), vidar_ray_{ce,gumbel,dist}_bwd_f32,
 * vidar_latent_render_{prob,gather,gather_grouped}_bwd_f32, vidar_knn1_d3_bwd_ws (grad_p2), vidar_dcn_col2im_f32
 * (grad_x); vidar_drop_add_ln_bwd_f32 sums dgamma / dbeta in a fixed order instead.  In the mode
 *   - their workspace queries return the bytes of the deterministic form (8 B per output element + the max words) and
 *     the call returns VIDAR_ERR_BAD_ARG without such a workspace: it never falls back to float atomics;
 *   - a non-finite contribution makes the WHOLE gradient NaN (the default mode poisons the touched addresses only).
 * Every other entry point ignores the switch; the default mode is unchanged in every bit. */
int vidar_set_deterministic(int on);
int vidar_get_deterministic(void);

/* ---------------------------------------------------------------------------
 * third_lib/dvr  (pybind surface: third_lib/dvr/dvr.cpp:36-69)
 *   sigma   [N,T,Z,Y,X] f32     origin [N,TO,3] f32 (voxel units)
 *   points  [N,M,3]     f32     tindex [N,M]    f32 (frame id, <0 = padded ray)
 * ------------------------------------------------------------------------- */
int vidar_dvr_max_d(void);   /* 1446, third_lib/dvr/dvr.cu:9 */

/* dvr.render_forward(sigma, origin, points, tindex, grid, phase_name) -> [pred_dist, gt_dist]
 * third_lib/dvr/dvr.cu:65-383.  train_phase: 0 = "test", 1 = "train" (dvr.cu:361-366). */
int vidar_dvr_render_forward_f32(const float* sigma, const float* origin, const float* points,
                                 const float* tindex, float* pred_dist /*[N,M]*/,
                                 float* gt_dist /*[N,M]*/, int N, int M, int T, int TO, int Z, int Y,
                                 int X, int train_phase, void* stream);

/* dvr.render(sigma, origin, points, tindex, loss_name) -> [pred_dist, gt_dist, grad_sigma]
 * third_lib/dvr/dvr.cu:385-694.  loss_type: 0 = "l1" (and "bce"), 1 = "l2", 2 = "absrel"
 * (dvr.cu:658-672).  grad_sigma [N,T,Z,Y,X] is zeroed by the call, then accumulated with
 * fp32 hardware atomics (the reference's "+=" at dvr.cu:622 is racy). */
int vidar_dvr_render_f32(const float* sigma, const float* origin, const float* points,
                         const float* tindex, float* pred_dist, float* gt_dist, float* grad_sigma,
                         int N, int M, int T, int TO, int Z, int Y, int X, int loss_type,
                         void* stream);

/* dvr.init / dvxlr.init(points, tindex, grid) -> occupancy [N,T,Z,Y,X]
 * third_lib/dvr/dvr.cu:14-63,:705-738 == third_lib/dvxlr/dvxlr.cu:12-61,:528-561. */
int vidar_dvr_init_f32(const float* points, const float* tindex, float* occupancy, int N, int M,
                       int T, int Z, int Y, int X, void* stream);

/* ---------------------------------------------------------------------------
 * third_lib/dvxlr  (pybind surface: dvxlr.cpp:34-65, dvxlr_v2.cpp:34-70)
 * ------------------------------------------------------------------------- */
int vidar_dvxlr_max_d(void); /* 1026, third_lib/dvxlr/dvxlr.cu:10 */

/* Precision contract of the dvr / dvxlr family: the voxel traversal (tMax / tDelta, axis choice, voxel
 * indices, gt_dist) is IEEE fp64 in the reference's operation order, no FMA contraction -> index lists
 * and gt_dist are bit-exact.  The transmittance of the online ray integral is evaluated as
 * expf((float)(-cumulative_sigma_dt)) -- fp32, where the reference calls the fp64 exp -- because every
 * output it feeds (pred_dist, dd_dsigma, grad_sigma) is stored as fp32 anyway (the reference allocates
 * float outputs, dvxlr.cu:490-493); those values agree with the reference to 2e-5 relative
 * (tests/test_dvr_gpu.py), not bit for bit.  Only _f32 entry points exist for the same reason: fp64
 * tensor arguments make the reference itself fail in packed_accessor32. */

/* tuning/A-B switch of the dvr / dvxlr march launches: a launch with more than `min_waves` waves of
 * 64 rays (default 1024 = one per SIMD) ranks the rays of each 256-ray workgroup by estimated
 * length before walking them; 0 = always, INT_MAX = never.  Results do not depend on it.
 * Returns the previous value. */
int vidar_dvr_set_sort_min_waves(int min_waves);
/* which traversal the dvr / dvxlr march launches use: -1 (default) = step-parallel kernels (independent per-axis
 * tMax chains -- dvr.cu:232-251, dvxlr.cu:334-353 advance tMaxX only on X steps -- merged by exact comparisons,
 * lane-per-step integration; csrc/dvr_par.h) where they are the faster form (dvr.render at every size, the one-launch
 * dvxlr.render / render_v2 up to 98 304 rays, dvr.render_forward up to 24 576 rays), lane-per-ray kernels otherwise;
 * 0 = always lane-per-ray, 1 = always step-parallel.  Results do not depend on it: index lists and gt_dist are
 * bit-identical (tests/test_dvr_gpu.py runs every case under both).  Returns the previous value. */
int vidar_dvr_set_traversal(int mode);
/* tuning/A-B switch of dvxlr.render / render_v2: 0 = the finish pass pads the [1026] rows itself,
 * 1 (default) = one device fill ahead of the march, the finish pass only touches the live prefixes.
 * Results do not depend on it (tests/test_dvr_gpu.py runs every case under both).  Both switches are plain
 * process-wide ints read at launch time: set them before concurrent use, not during.
 * Returns the previous value. */
int vidar_dvxlr_set_pad_mode(int mode);

/* dvxlr.render(sigma, origin, points, tindex) -> [pred_dist, gt_dist, dd_dsigma, indices]
 * third_lib/dvxlr/dvxlr.cu:160-517.
 *   dd_dsigma [N,M,1026] f32 (0-padded), indices [N,M,1026,3] f32 as (z,y,x) (0-padded).
 *   The call writes every byte of the outputs (padding included); the padded row buffers must be
 *   8-byte aligned (VIDAR_ERR_BAD_ARG otherwise). */
int vidar_dvxlr_render_f32(const float* sigma, const float* origin, const float* points,
                           const float* tindex, float* pred_dist, float* gt_dist, float* dd_dsigma,
                           float* indices, int N, int M, int T, int TO, int Z, int Y, int X,
                           void* stream);

/* dvxlr.get_grad_sigma(elementwise_mult, indices, tindex, sigma_like) -> [grad_sigma]
 * third_lib/dvxlr/dvxlr.cu:63-156.  L = elementwise_mult.size(2). grad_sigma zeroed by the call.
 * `workspace` (vidar_dvxlr_get_grad_sigma_workspace_bytes(.., volumes): 1 for this call, 2 for get_grad_sigma_v2): caller-owned device
 * scratch for 8 private copies of the gradient volume -- the rays of a frame share their first voxels, whose
 * atomics otherwise serialise (one frame of 30 000 rays took as long as five); NULL = add straight into grad_sigma. */
size_t vidar_dvxlr_get_grad_sigma_workspace_bytes(int N, int T, int Z, int Y, int X, int volumes /* 1: get_grad_sigma, 2: _v2 */);
int vidar_dvxlr_get_grad_sigma_f32(const float* elementwise_mult /*[N,M,L]*/,
                                   const float* indices /*[N,M,L,3]*/, const float* tindex,
                                   float* grad_sigma /*[N,T,Z,Y,X]*/, int N, int M, int L, int T,
                                   int Z, int Y, int X, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* dvxlr_v2.render_v2(sigma, origin, points, tindex, sigma_regul)
 *   -> [pred_dist, gt_dist, dd_dsigma, indices, ray_pred, indicator]
 * third_lib/dvxlr/dvxlr_v2.cu:119-493. indicator is -1-padded, 1 at the first sample whose
 * exit distance reaches the un-clamped ray length (dvxlr_v2.cu:408-424). */
int vidar_dvxlr2_render_f32(const float* sigma, const float* origin, const float* points,
                            const float* tindex, const float* sigma_regul, float* pred_dist,
                            float* gt_dist, float* dd_dsigma, float* indices, float* ray_pred,
                            float* indicator, int N, int M, int T, int TO, int Z, int Y, int X,
                            void* stream);

/* dvxlr_v2.get_grad_sigma_v2(em, indices, tindex, sigma_like, indicator, grad_ray_pred)
 *   -> [grad_sigma, grad_sigma_regul]       third_lib/dvxlr/dvxlr_v2.cu:12-115 */
int vidar_dvxlr2_get_grad_sigma_f32(const float* elementwise_mult, const float* indices,
                                    const float* tindex, const float* indicator,
                                    const float* grad_ray_pred, float* grad_sigma,
                                    float* grad_sigma_regul, int N, int M, int L, int T, int Z, int Y,
                                    int X, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * third_lib/chamfer_dist/chamferdist  (pybind surface: chamferdist/ext.cpp:5-11)
 * K = 1, D = 3 specialisation of knn_points_idx / knn_points_backward
 * (knn.h:50-66, knn_cpu.cpp:7-58 & :64-106, knn.cu:297-435 & :482-544).
 *   p1 [N,P1,3] f32, p2 [N,P2,3] f32, lengths1/2 [N] i64 (device), idx [N,P1] i64,
 *   dist2 [N,P1] f32 = squared L2, evaluated as ((dx*dx+dy*dy)+dz*dz) without FMA; ties -> lowest
 *   index.  workspace: vidar_knn1_d3_workspace_bytes(N,P1) bytes of device scratch.
 * ------------------------------------------------------------------------- */
size_t vidar_knn1_d3_workspace_bytes(int N, int P1);
int vidar_knn1_d3_fwd(const float* p1, const float* p2, const int64_t* lengths1,
                      const int64_t* lengths2, int64_t* idx, float* dist2, void* workspace, int N,
                      int P1, int P2, void* stream);
/* grad_p1 [N,P1,3] written, grad_p2 [N,P2,3] zeroed then accumulated (fp32 atomics). */
int vidar_knn1_d3_bwd(const float* p1, const float* p2, const int64_t* lengths1,
                      const int64_t* lengths2, const int64_t* idx, const float* grad_dist2,
                      float* grad_p1, float* grad_p2, int N, int P1, int P2, void* stream);
/* The same with a caller-owned workspace, which the deterministic mode needs for grad_p2 (the entry above has nowhere
 * to put the accumulators: VIDAR_ERR_BAD_ARG in the mode).  *bytes: 0 with the mode off (workspace may be NULL),
 * 8 * (N*P2*3 + 1) with it on. */
int vidar_knn1_d3_bwd_workspace_bytes(int N, int P2, int64_t* bytes);
int vidar_knn1_d3_bwd_ws(const float* p1, const float* p2, const int64_t* lengths1,
                         const int64_t* lengths2, const int64_t* idx, const float* grad_dist2,
                         float* grad_p1, float* grad_p2, int N, int P1, int P2, void* workspace,
                         size_t workspace_bytes, void* stream);

/* knn_points_idx / knn_points_backward for 1 <= D <= 8, 1 <= K <= 32 (the reference's V2 range, knn.cu:261-264;
 * csrc/knn_generic.hip).  p1 [N,P1,D], p2 [N,P2,D] f32; idx [N,P1,K] i64, dist2 [N,P1,K] f32: for every row below
 * lengths1 the min(K, lengths2) points of p2[n, :lengths2[n]] that are smallest in (dist2, index), ascending; rows past
 * lengths1 and slots past lengths2 are zero.  dist2 = sum over d of (p1[d] - p2[d])^2 in the order d = 0, 1, .., every
 * product and sum rounded on its own (knn_cpu.cpp:36-40): the same bytes as the reference's CPU build.
 *   chunks: p2 is cut into that many ranges across workgroups; 0 = the library chooses from N, P1, P2, K and the CU
 *     count.  The result does not depend on it (the (dist2, index) order is total).
 *   workspace: *bytes of vidar_knn_workspace_bytes = 8 * N * P1 * chunks_used * K (the partial lists; never P1 * P2),
 *     chunks_used = min(chunks, max(P2, 1)).  The query returns VIDAR_ERR_BAD_ARG and *bytes = -1 for a (D, K) outside
 *     the range or extents the kernels' 32-bit indices cannot hold (P1 * D or P2 * D above INT32_MAX; N or chunks
 *     above 65535); it makes no call that needs a GPU.
 *   An extent of 0 (N, P1, P2 or K) returns 0 before any HIP call and writes nothing: with nothing to search every
 *     output is zero, and the caller provides that (chamferdist._C allocates zeros).  For every other call idx / dist2
 *     and grad_p1 / grad_p2 are written completely.
 * vidar_knn_bwd_f32: grad_p1[n,i,d] = sum over k < min(K, lengths2) of c = (2 g[n,i,k]) (p1[n,i,d] - p2[n,idx[n,i,k],d])
 * in the order k = 0, 1, .. (a plain store: the reference's bytes); grad_p2[n,idx,d] -= c with fp32 atomics on a zeroed
 * grad_p2 (knn_cpu.cpp:88-103).  An idx outside [0, P2) contributes nothing.  The deterministic mode does not change it. */
int vidar_knn_workspace_bytes(int N, int P1, int P2, int D, int K, int chunks, int64_t* bytes, int64_t* chunks_used);
int vidar_knn_fwd_f32(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2,
                      int64_t* idx, float* dist2, void* workspace, size_t workspace_bytes,
                      int N, int P1, int P2, int D, int K, int chunks, void* stream);
int vidar_knn_bwd_f32(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2,
                      const int64_t* idx, const float* grad_dist2, float* grad_p1, float* grad_p2,
                      int N, int P1, int P2, int D, int K, void* stream);

/* ---------------------------------------------------------------------------
 * Multi-scale deformable attention.  Replaces mmcv._ext.ms_deform_attn_{forward,backward}
 * (mmcv-full 1.4.0, third party) as called from
 * projects/mmdet3d_plugin/bevformer/modules/multi_scale_deformable_attn_function.py:118-124, :150-160.
 *   value [B,Nv,H,C] f32 (C must be 32), spatial_shapes [L,2] i64 (h,w), level_start_index [L] i64,
 *   sampling_loc [B,Nq,H,L,P,2] f32 in [0,1] (x,y), attn_weight [B,Nq,H,L,P] f32, out [B,Nq,H*C].
 * im2col_step of the reference API has no meaning here and is dropped at the Python layer.
 * Limits (VIDAR_ERR_BAD_ARG otherwise): C == 32, L <= 16, L*P <= 64, and ONE batch element of `value` smaller than
 * 4 GiB (Nv*H*C*4 < 2^32: corner lines are addressed with 32-bit byte offsets; a larger `value` tensor is processed
 * in several launches over batch elements, each with its own base pointers -- same results).
 * A sample outside its level, or with a NaN location, contributes nothing (zero output / gradients).
 * bwd: grad_value is zeroed by the call then accumulated with fp32 atomics; grad_sampling_loc and
 * grad_attn_weight are fully written (the reference expects pre-zeroed buffers, function.py:146-148).
 * ------------------------------------------------------------------------- */
int vidar_msda_fwd_f32(const float* value, const int64_t* spatial_shapes,
                       const int64_t* level_start_index, const float* sampling_loc,
                       const float* attn_weight, float* out, int B, int Nv, int H, int C, int Nq,
                       int L, int P, void* stream);
/* bwd has two scatter strategies for grad_value, chosen by the caller through `workspace`:
 *   workspace == NULL : one fp32 atomic per (sample, corner) 128-byte line (fine for small launches);
 *   workspace != NULL : samples are counting-sorted by destination tile (batch, level, 8x8 pixels, head)
 *                       into the workspace, accumulated per tile in LDS and flushed with one atomic per
 *                       non-zero window line (see csrc/msda.hip).  The workspace needs
 *                       vidar_msda_bwd_workspace_bytes(...) bytes (0 = shape not supported by this
 *                       strategy: >= 2^31 samples or grad_out of 2 GiB and more), is scratch (no state survives the
 *                       call) and must stay alive until the stream has run the call.
 * Both give the same result up to fp32 summation order. */
size_t vidar_msda_bwd_workspace_bytes(int B, int Nv, int H, int Nq, int L, int P);
/* tuning/A-B switch of the gather kernels (forward, grad_loc / grad_w): which 32 (batch, query, head) items a workgroup
 * owns.  1 (default) = head-major: 32 consecutive queries of ONE head, head = workgroup % H, so that with ViDAR's 8 heads
 * each of the 8 XCDs only reads its own head's plane of `value` (it fits the XCD's 4 MiB L2); 0 = 4 queries x 8 heads in
 * contiguous query bands per XCD (rounds 1-3).  Results do not depend on it.  Returns the previous value. */
int vidar_msda_set_item_order(int head_major);
int vidar_msda_bwd_f32(const float* value, const int64_t* spatial_shapes,
                       const int64_t* level_start_index, const float* sampling_loc,
                       const float* attn_weight, const float* grad_out, float* grad_value,
                       float* grad_sampling_loc, float* grad_attn_weight, int B, int Nv, int H, int C,
                       int Nq, int L, int P, void* workspace, size_t workspace_bytes, void* stream);

/* Fused operand preparation (csrc/msda.hip): the op consumes the raw outputs of the sampling_offsets and
 * attention_weights Linear layers instead of prepared locations / weights, replacing the softmax, the
 * division by the level size, the reference-point add and the (TSA) permute copies of
 * temporal_self_attention.py:218-245, spatial_cross_attention.py:359-383, vidar_decoder.py:463-490.
 *   off_raw [bs,Nq,H,Qn,L,P,2] f32, logit_raw [bs,Nq,H,Qn,L*P] f32, ref [bs*Qn,Nq,R,2] f32,
 *   value [bs*Qn,Nv,H,C]; loc = ref[.., r, :] + off / (W_l, H_l) with r = level (mode 0, R == L) or
 *   point % R (mode 1, P % R == 0); w = softmax over L*P.
 * fwd writes out [bs*Qn,Nq,H*C] and the prepared operands loc_out [bs*Qn,Nq,H,L,P,2] / w_out [bs*Qn,Nq,H,L,P]
 * (what the backward needs); bwd takes those and writes grad_value (zeroed + accumulated),
 * grad_off_raw, grad_logit_raw (fully written, raw layouts).  workspace as for vidar_msda_bwd_f32 with
 * B = bs*Qn.
 * merge_queue = 1: the op also takes the MEAN over the Qn queue entries that TemporalSelfAttention applies to its output
 * (`output.view(bs, Qn, Nq, C).mean(1)`, temporal_self_attention.py:256-264): out / grad_out are [bs,Nq,H*C], the Qn
 * entries of a (batch, query, head) are gathered by one item and summed in registers (Qn*L*P <= 64); loc_out / w_out and
 * the gradients keep the layouts above.  merge_queue = 0: out / grad_out [bs*Qn,Nq,H*C]. */
int vidar_msda_fused_fwd_f32(const float* value, const int64_t* spatial_shapes,
                             const int64_t* level_start_index, const float* off_raw, const float* logit_raw,
                             const float* ref, float* loc_out, float* w_out, float* out, int bs, int Qn, int Nv,
                             int H, int C, int Nq, int L, int P, int R, int mode, int merge_queue, void* stream);
int vidar_msda_fused_bwd_f32(const float* value, const int64_t* spatial_shapes,
                             const int64_t* level_start_index, const float* sampling_loc,
                             const float* attn_weight, const float* grad_out, float* grad_value,
                             float* grad_off_raw, float* grad_logit_raw, int bs, int Qn, int Nv, int H, int C,
                             int Nq, int L, int P, int merge_queue, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * y = LayerNorm(dropout(x) + residual) and its backward in one pass each (csrc/norm_fuse.hip): the tail of every
 * attention / FFN block of the encoder and the future decoder (temporal_self_attention.py:270-271,
 * spatial_cross_attention.py:172-174, vidar_decoder.py:515-516, mmcv FFN) followed by the layer's norm.
 *   x, residual, y, sum_out [rows, C] f32 with C == 256; gamma, beta [C]; mean_out, rstd_out [rows].
 *   dropout keeps element i iff hash(seed, i) >= p (recomputed in the backward from the same seed; p = 0: exact).
 *   bwd: grad_x, grad_residual, grad_gamma, grad_beta fully written (the affine gradients from per-workgroup
 *   partial rows kept in `workspace` (vidar_drop_add_ln_bwd_workspace_bytes, scratch).  `workspace` must hold
 *   vidar_drop_add_ln_bwd_workspace_bytes(rows) bytes: the call takes no size and cannot see a shorter one.
 *   Pointers (these two entries, vidar_relu_drop_{fwd,bwd}_f32 and vidar_colsum_f32): the [rows, C] and [n] tensors,
 *   gamma, beta, `workspace` and colsum's `x` are read and written as float4 and must sit on a 16-byte boundary; every
 *   operand the call dereferences must be non-NULL (an empty problem, rows == 0 / n == 0, dereferences only what it
 *   zeroes: grad_gamma, grad_beta, colsum's `out`).  Either fault, a NaN p, or p outside [0, 1) is VIDAR_ERR_BAD_ARG
 *   before anything is launched or written.
 *   Domain: the variance squares (sum - mean) in fp32, so a row with |dropout(x) + residual| beyond about 1e19
 *   overflows to var = inf, rstd = 0.
 *   grad_gamma / grad_beta are sums over rows: in the default mode their last bits depend on the order in which the
 *   row slices meet (fp32 atomics) and can differ from run to run; under vidar_set_deterministic(1) the order is fixed.
 * ------------------------------------------------------------------------- */
int vidar_drop_add_ln_fwd_f32(const float* x, const float* residual, const float* gamma, const float* beta, float* y,
                              float* sum_out, float* mean_out, float* rstd_out, int64_t rows, int C, float p, float eps,
                              uint32_t seed, void* stream);
int vidar_drop_add_ln_bwd_f32(const float* grad_y, const float* sum_in, const float* gamma, const float* mean_in,
                              const float* rstd_in, float* grad_x, float* grad_residual, float* grad_gamma,
                              float* grad_beta, void* workspace, int64_t rows, int C, float p, uint32_t seed,
                              void* stream);
size_t vidar_drop_add_ln_bwd_workspace_bytes(int64_t rows); /* scratch for the per-workgroup affine-gradient partials */

/* y = dropout(relu(x)) and its backward, one pass each (csrc/norm_fuse.hip): the hidden activation of the FFN blocks
 * (mmcv FFN [3P]: Linear -> ReLU -> Dropout -> Linear; custom_base_transformer_layer.py builds them from the configs'
 * ffn_cfgs).  n elements (a multiple of 4), 0 <= p < 1; keeps element i iff hash(seed, i) >= p and scales it by
 * 1 / (1 - p) (same hash as the fused LayerNorm tail; not torch's Philox stream: dropout noise has no parity contract,
 * p = 0 is exact).  bwd: grad_x = y > 0 ? grad_y / (1 - p) : 0 -- y is the forward's OUTPUT, no mask is stored.
 * x / y and grad_y / grad_x may alias.  The ReLU is fmaxf(x, 0), the rule of vidar_affine_act_fwd_f32: a NaN comes out
 * as 0 where torch.relu gives NaN.  A dropped element is relu(x) * 0, so a dropped +inf comes out as NaN (a kept one as
 * +inf), and the backward, which asks y > 0, gives such an element the gradient 0. */
int vidar_relu_drop_fwd_f32(const float* x, float* y, int64_t n, float p, uint32_t seed, void* stream);
int vidar_relu_drop_bwd_f32(const float* grad_y, const float* y, float* grad_x, int64_t n, float p, void* stream);

/* Column sums of a row-major [rows, cols] fp32 matrix: out[c] = sum_r x[r, c] -- the bias gradient of the Linear
 * layers on the path (what autograd computes with a generic `sum(0)` for every nn.Linear the reference's modules
 * own, e.g. temporal_self_attention.py:98-103, spatial_cross_attention.py:66, :244-248, vidar_decoder.py:358-363; mmcv FFN [3P]).  `out` [cols] is
 * zeroed and fully written by the call.  cols must be a multiple of 4 whose quarter is a power of two (<= 4096). */
int vidar_colsum_f32(const float* x, float* out, int64_t rows, int cols, void* stream);

/* ---------------------------------------------------------------------------
 * BEV-encoder bookkeeping for F frames at once.  Replaces BEVFormerEncoder.point_sampling
 * (projects/mmdet3d_plugin/bevformer/modules/encoder.py:96-156) and the visible-query rebatch index of
 * SpatialCrossAttention.forward (spatial_cross_attention.py:136-152, :164-171).
 *   ref_3d [D,Q,3] f32 pillar anchors in [0,1] (encoder.py:54-80), lidar2img [F,B,N,4,4] f32 row-major,
 *   pc_range: HOST pointer to 6 floats, img_h/img_w: padded image shape of camera 0 (encoder.py:137-138).
 * Outputs (caller-allocated, fully written): ref_cam [F,N,B,Q,D,2] f32, bev_mask [F,N,B,Q,D] u8 (0/1),
 *   count [F,B,Q] f32 = max(1, #cameras seeing the query), idx [F,N,Q] i64 = visible queries of batch item 0
 *   in ascending order, then distinct in-range filler (slot number), valid [F,N,Q] u8 = slot < lens, lens [F,N] i32.
 *   slot_of [F,N,Q] i32 = inverse of idx (slot of a query in its camera's list, -1 = not visible).
 * vidar_sca_rows_f32 / vidar_sca_combine_f32: the rebatch / scatter-back of SpatialCrossAttention
 * (spatial_cross_attention.py:141-152, :164-171) and their backwards, as row gathers (csrc/bev_prep.hip):
 *   rows   : dst [B,N,S,C] = valid[n,s] ? src[b, idx[n,s], :] (/ count[b,idx] if count) : 0;  idx/valid rows have
 *            `stride` elements (S <= stride: a [N,S] slice of the [N,Q] tables);
 *   combine: dst [B,Q,C]   = sum over cameras n with slot_of[n,q] in [0,S) of src[b,n,slot_of[n,q],:] (/ count[b,q]).
 * C must be a multiple of 4. */
int vidar_sca_plan_f32(const float* ref_3d, const float* lidar2img, float* ref_cam, uint8_t* bev_mask,
                       float* count, int64_t* idx, uint8_t* valid, int32_t* lens, int32_t* slot_of,
                       const float* pc_range, float img_h, float img_w, int F, int B, int N, int Q, int D,
                       void* stream);
int vidar_sca_rows_f32(const float* src, const int64_t* idx, const uint8_t* valid, const float* count, float* dst,
                       int B, int N, int S, int stride, int Q, int C, void* stream);
int vidar_sca_combine_f32(const float* src, const int32_t* slot_of, const float* count, float* dst, int B, int N,
                          int S, int Q, int C, void* stream);

/* ---------------------------------------------------------------------------
 * LatentRendering ray-march (fused).  Replaces the torch op chain of
 * projects/mmdet3d_plugin/bevformer/modules/ray_operations/latent_rendering.py:96-150.
 * All maps are channel-last f32: [bs, H*W, Z] for the Z = pred_height height bins, 1 <= Z <= 64, and [bs, H*W, A] for
 * the A = embed_dims/reduction LoRA channels, A = Z*J <= 256; LoRA channel ch belongs to bin ch / J (:148-150).
 * step = grid_step / (min(H,W)//2) rounded to f32 (:102-104); act: 0 = 'sigmoid', 1 = 'exp' (:117-123).
 *   prob   : occ logits -> path_prob = prod_{k<G,valid}(1 - act(occ(n_k))) * act(occ(n_cell))   (:96-129)
 *   gather : feat = sum_k a(n_k) m_k / (sum_k m_k + eps), m_k = path_prob(n_k)*valid2_k          (:131-150)
 *            lora_a, feat and their gradients have A channels, path_prob, msum and grad_path_prob Z; the entries
 *            without `grouped` are the case A == Z.  Any other Z or A: VIDAR_ERR_BAD_ARG, nothing is launched.
 * Backward entry points zero their gradient outputs and accumulate with fp32 atomics; `workspace`
 * (vidar_latent_render_bwd_workspace_bytes, caller-owned scratch, 16-byte aligned) holds 8 private copies of the
 * gradient maps as for the ray ops below, NULL = add straight into the outputs.  The grouped backward's two maps differ
 * in size: its workspace is vidar_latent_render_bwd_workspace_bytes(bs, H, W, max(Z, A), 2).
 * ------------------------------------------------------------------------- */
size_t vidar_latent_render_bwd_workspace_bytes(int bs, int H, int W, int Z, int maps /* 1: prob_bwd, 2: gather_bwd */);
int vidar_latent_render_prob_fwd_f32(const float* occ, float* path_prob, int bs, int H, int W, int Z,
                                     int grid_num, float step, int act, void* stream);
int vidar_latent_render_prob_bwd_f32(const float* occ, const float* grad_path_prob, float* grad_occ,
                                     int bs, int H, int W, int Z, int grid_num, float step, int act,
                                     void* workspace, size_t workspace_bytes, void* stream);
int vidar_latent_render_gather_fwd_f32(const float* path_prob, const float* lora_a, float* feat,
                                       float* msum, int bs, int H, int W, int Z, int grid_num,
                                       float step, float eps, void* stream);
int vidar_latent_render_gather_bwd_f32(const float* path_prob, const float* lora_a, const float* feat,
                                       const float* msum, const float* grad_feat,
                                       float* grad_path_prob, float* grad_lora_a, int bs, int H,
                                       int W, int Z, int grid_num, float step, float eps,
                                       void* workspace, size_t workspace_bytes, void* stream);
int vidar_latent_render_gather_grouped_fwd_f32(const float* path_prob, const float* lora_a, float* feat, float* msum,
                                               int bs, int H, int W, int Z, int A, int grid_num, float step,
                                               float eps, void* stream);
int vidar_latent_render_gather_grouped_bwd_f32(const float* path_prob, const float* lora_a, const float* feat,
                                               const float* msum, const float* grad_feat, float* grad_path_prob,
                                               float* grad_lora_a, int bs, int H, int W, int Z, int A, int grid_num,
                                               float step, float eps, void* workspace, size_t workspace_bytes,
                                               void* stream);

/* ---------------------------------------------------------------------------
 * ViDAR head ray-march over the predicted occupancy volume (fused).  Replaces the torch op chains
 * of projects/mmdet3d_plugin/bevformer/dense_heads/vidar_head_base.py:
 *   ray_ce     _get_grid_features :420-509 + cross_entropy(label 0) :586-592
 *   ray_gumbel dense rays :594-630 + _custom_gumbel_softmax_distance :754-773
 *   ray_argmax get_point_cloud_prediction :697-731 (test-time decode)
 *   ray_dist   the use_dist_loss branch :575-585 (_custom_gumbel_softmax_distance on the GT rays)
 * sigma [F,Z,Y,X] f32 logits; origin [F,3]; pts [R,3] ray end points; tindex [R] f32 frame slot
 * (<0 / NaN / >=F: ray skipped); all in voxel units.  K = ray_grid_num, 1 <= K <= vidar_ray_max_k()
 * (65536; anything else is VIDAR_ERR_BAD_ARG): K == 512 (the released configs) runs the register-resident kernels,
 * every other K the streamed ones, which never touch waypoints k >= K.  step = ray_grid_step.  Outputs are per ray;
 * reductions stay in the host framework.
 *   ce[r]   = logsumexp_k(logit_k) - logit_0 over {end point, K waypoints}; valid[r] = 1 iff the
 *             end point lies strictly inside the volume (others are dropped, :464-467); lse saved.
 *   dist[r] = ((1-pn)+pn) * pd, pd = length of argmax_k(logit_k + noise[r,k]),
 *             pn = softmax mass of waypoints farther than pd;  aux[r] = {pd, pn, lse}.
 *   ray_dist: the same rendered distance over the K + 1 logits of a GT ray -- entry 0 the sample AT the end point
 *             with length |p - o|, entries 1..K the waypoints; noise [R, K+1] in that order, row r for ray r.  Rays are
 *             dropped as in ray_ce (dist = gt_len = 0, valid = 0).  gt_len[r] = |p - o|, the L1 target.  aux [R,3] as
 *             above is what the backward needs; it scatters onto the end point's corners too.
 * Backward entry points zero grad_sigma and accumulate with fp32 atomics.  All rays of a frame start at the sensor
 * origin, so the first waypoints' atomics serialise on a few hundred addresses: given a `workspace` of
 * vidar_ray_bwd_workspace_bytes(F,Z,Y,X) bytes (caller-owned device scratch on the call's device / stream, nothing
 * survives the call) the kernels add into 8 private copies of the volume that a second kernel sums; with
 * workspace == NULL they add straight into grad_sigma.  Results agree to fp32 summation order.
 * Deterministic mode (vidar_set_deterministic): the workspace query returns 8 * (F*Z*Y*X + 1) and the backwards
 * accumulate in fixed point (the plain scatter, no private copies); the same bits for every K form and ray order.
 * ------------------------------------------------------------------------- */
size_t vidar_ray_bwd_workspace_bytes(int F, int Z, int Y, int X);
int vidar_ray_ce_fwd_f32(const float* sigma, const float* origin, const float* gt_pts,
                         const float* tindex, float* ce, float* lse, float* valid, int F, int R,
                         int Z, int Y, int X, int K, float step, void* stream);
int vidar_ray_ce_bwd_f32(const float* sigma, const float* origin, const float* gt_pts,
                         const float* tindex, const float* lse, const float* grad_ce,
                         float* grad_sigma, int F, int R, int Z, int Y, int X, int K, float step,
                         void* workspace, size_t workspace_bytes, void* stream);
int vidar_ray_gumbel_fwd_f32(const float* sigma, const float* origin, const float* pts,
                             const float* tindex, const float* noise /*[R,K]*/, float* dist,
                             float* aux /*[R,3]*/, int F, int R, int Z, int Y, int X, int K,
                             float step, void* stream);
int vidar_ray_gumbel_bwd_f32(const float* sigma, const float* origin, const float* pts,
                             const float* tindex, const float* aux, const float* grad_dist,
                             float* grad_sigma, int F, int R, int Z, int Y, int X, int K, float step,
                             void* workspace, size_t workspace_bytes, void* stream);
int vidar_ray_argmax_f32(const float* sigma, const float* origin, const float* pts,
                         const float* tindex, float* pred_dist, float* gt_dist, int F, int R, int Z,
                         int Y, int X, int K, float step, void* stream);
int vidar_ray_dist_fwd_f32(const float* sigma, const float* origin, const float* gt_pts,
                           const float* tindex, const float* noise /*[R,K+1]*/, float* dist,
                           float* gt_len, float* aux /*[R,3]*/, float* valid, int F, int R, int Z,
                           int Y, int X, int K, float step, void* stream);
int vidar_ray_dist_bwd_f32(const float* sigma, const float* origin, const float* gt_pts,
                           const float* tindex, const float* aux, const float* grad_dist,
                           float* grad_sigma, int F, int R, int Z, int Y, int X, int K, float step,
                           void* workspace, size_t workspace_bytes, void* stream);
/* largest accepted K */
int vidar_ray_max_k(void);
/* Test / benchmark hook, process-wide: nonzero sends K == 512 through the streamed kernels as well (same bits: every
 * lane adds its waypoints in the register form's order).  Returns the previous setting.  One atomic flag for the whole
 * process, not a per-call or per-thread option: a thread that flips it changes which kernel the K == 512 calls of every
 * other thread launch from then on (same results, different time), so production code leaves it alone. */
int vidar_ray_force_streamed(int on);

/* Camera-view arg-max march (csrc/ray_march.hip, pixel -> ray in csrc/cam_ray.h): the decode of vidar_ray_argmax_f32
 * with one ray per pixel of C cameras, generated in the kernel instead of read from a list.
 *   pix2vox [F,C,4,4] row-major f32 maps the homogeneous pixel (u*d, v*d, d, 1) to voxel coordinates of frame f's
 *           volume.  It is affine (the inverse of a camera matrix with last row 0 0 0 1): only rows 0..2 are read.
 *   pixel (x, y) of the [Hs, Ws] grid has u = u0 + x*du, v = v0 + y*dv (fp32, each operation rounded on its own).
 *   The camera centre is the image of (0,0,0,1), the ray's end point the image of (u,v,1,1); from the end point on
 *   the march is vidar_ray_argmax_f32's own body (K == 512 register-resident, every other K streamed).
 *   dist [F,C,Hs,Ws] f32, voxel units: the length of the arg-max waypoint; 0 for a ray without a live waypoint (all
 *           outside the volume, or on exact zeros of it).  The only store of the kernel, no atomics.
 * vidar_cam_rays_f32 writes out what the fused kernel marches -- origin [F,C,3], pts [F,C,Hs,Ws,3] -- from the same
 * device function, so vidar_ray_argmax_f32 per camera on (origin[:,c], pts[:,c], tindex = f) gives the fused kernel's
 * bits on every ray with a live waypoint (a ray without one gets waypoint 0's length there, the reference's answer).
 * F, C <= 0, negative Hs / Ws, a NaN or zero pixel pitch, F*C*Hs*Ws beyond the 32-bit ray index, or bad volume / K
 * (as above) return VIDAR_ERR_BAD_ARG; an empty grid returns 0 without a launch. */
int vidar_ray_argmax_cam_f32(const float* sigma, const float* pix2vox, float* dist, int F, int C, int Hs, int Ws,
                             float u0, float v0, float du, float dv, int Z, int Y, int X, int K, float step,
                             void* stream);
int vidar_cam_rays_f32(const float* pix2vox, float* origin, float* pts, int F, int C, int Hs, int Ws, float u0,
                       float v0, float du, float dv, void* stream);

/* The decode with its confidence (csrc/ray_march.hip, ray_stats_body): vidar_ray_argmax_f32 / vidar_ray_argmax_cam_f32
 * plus four statistics of the softmax over the ray's waypoints.  Same waypoints and sampler as the decode: zero padding,
 * an exact 0 sample counts as -inf, a NaN coordinate samples as 0.  z_k = logit, l_k = length of waypoint k; a waypoint
 * is live iff z_k is not -inf.  With m = max z_k, e_k = exp(z_k - m) (0 for a dead waypoint), S = sum e_k and d = the
 * arg-max length (first index wins), stats[r] = {p_max, mean, rms, entropy}, voxel units:
 *   p_max   = exp(z_argmax - m) / S, in (0, 1]
 *   mean    = d + sum e_k (l_k - d) / S          expected length, accumulated as a deviation from d
 *   rms     = sqrt(sum e_k (l_k - d)^2 / S)      spread about the decoded depth
 *   entropy = log S - sum_live e_k (z_k - m) / S  nats, >= 0; dead waypoints are skipped (no 0 * -inf)
 * A skipped ray (tindex < 0, NaN or >= F) and a ray without a live waypoint give four zeros.  pred_dist / gt_dist and dist
 * are what the two arg-max entries write for the ray, bit for bit (waypoint 0's length for a dead listed ray, 0 for a
 * dead camera ray).  +inf or NaN logits may give non-finite statistics.  fp32 sums in a fixed order, no atomics, no
 * workspace: equal inputs give equal bits, and K == 512 gives the same bits through the streamed kernels.
 * stats [R,4] / [F,C,Hs,Ws,4] is written as one 16-byte store per ray and must be 16-byte aligned; otherwise arguments
 * and VIDAR_ERR_BAD_ARG cases are those of the arg-max entries, and an empty problem returns 0 without a launch. */
int vidar_ray_stats_f32(const float* sigma, const float* origin, const float* pts, const float* tindex,
                        float* pred_dist, float* gt_dist, float* stats /*[R,4]*/,
                        int F, int R, int Z, int Y, int X, int K, float step, void* stream);
int vidar_ray_stats_cam_f32(const float* sigma, const float* pix2vox, float* dist /*[F,C,Hs,Ws]*/,
                            float* stats /*[F,C,Hs,Ws,4]*/, int F, int C, int Hs, int Ws,
                            float u0, float v0, float du, float dv, int Z, int Y, int X, int K, float step,
                            void* stream);

/* Occupancy evidence (csrc/ray_march.hip, ray_occupancy_body): the softmax of the decode scattered back onto the voxels
 * it was read from -- an inverse sensor model of the forecast.  Same rays, waypoints and sampler as vidar_ray_argmax_f32 /
 * vidar_ray_argmax_cam_f32; a waypoint is dead iff its sample is exactly 0 or its coordinate is NaN.  Over the live
 * waypoints of a ray, with m = max z_k, e_k = exp(z_k - m), S = sum e_k:
 *   p_k = e_k / S                  the return lies at k
 *   b_k = sum_{j > k, live} p_j    the return lies beyond k: the ray passed k
 * and with w_kc the eight trilinear weights of waypoint k (corners outside the volume dropped, as the zero padding
 * dropped them from the sample):
 *   hit [f, corner c of k] += p_k * w_kc          free[f, corner c of k] += b_k * w_kc
 * hit, free [F,Z,Y,X] f32 are zeroed by the call.  A dead waypoint, a skipped ray and a ray without a live waypoint add
 * nothing; R == 0 (an empty camera grid) leaves zeros.  b_k is a sum of non-negative terms taken from the far end, so
 * b_k >= 0 and the last live waypoint has b == 0 exactly.  +inf or NaN logits may give non-finite output.
 * The adds are those of the ray backwards: fp32 atomics, into 8 private copies of both volumes given a `workspace` of
 * *bytes of vidar_ray_occupancy_workspace_bytes(F,Z,Y,X,&bytes) (NULL: straight into the outputs; results agree to fp32
 * summation order).  Deterministic mode: the query gives 8 * (2*F*Z*Y*X + 2) and both volumes are accumulated in fixed
 * point -- the same bits for every K form and ray order; a missing or small workspace is VIDAR_ERR_BAD_ARG.
 * Other VIDAR_ERR_BAD_ARG cases are those of the arg-max entries; the query's: a NULL `bytes`, non-positive dimensions. */
int vidar_ray_occupancy_workspace_bytes(int F, int Z, int Y, int X, int64_t* bytes);
int vidar_ray_occupancy_f32(const float* sigma, const float* origin, const float* pts, const float* tindex,
                            float* hit, float* free_, int F, int R, int Z, int Y, int X, int K, float step,
                            void* workspace, size_t workspace_bytes, void* stream);
int vidar_ray_occupancy_cam_f32(const float* sigma, const float* pix2vox, float* hit, float* free_,
                                int F, int C, int Hs, int Ws, float u0, float v0, float du, float dv,
                                int Z, int Y, int X, int K, float step,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Measured evidence of a sweep (csrc/ray_march.hip, sweep_evidence_body; per-ray weight in csrc/occ_score_math.h): the
 * measured side of the inverse sensor model above, for rays whose end point is a measured return.  The rays are those of
 * vidar_ray_occupancy_f32 -- origin [F,3], pts [R,3], tindex [R], voxel units, the same skip rule, the same waypoints
 * s_k = o + rhat (k + 0.5) step, k < K, the same trilinear weights w_kc with corners outside the volume dropped -- and no
 * volume is read.  With L = |p - o| in fp32, a ray that is not skipped and has a finite L > 0 adds
 *   free[f, corner c of s_k] += a_k * w_kc     a_k = clamp((L - (k + 0.5) step) / step, 0, 1)
 *   hit [f, corner c of p  ] += w_pc           the trilinear weights of the END POINT itself
 * a_k is 1 well before the return, 0 from the return on and a ramp in between, so both grids are continuous in L and in
 * the waypoints; waypoints with a_k == 0 are not marched.  The return is splatted where it was measured, for every
 * marched ray, also when it lies beyond the marched range K * step.  Units are the predicted evidence's: free in
 * waypoints, hit in returns.  hit, free [F,Z,Y,X] f32 are zeroed by the call; all rays skipped, or R == 0, leaves exact
 * zeros; a ray with L == 0 or a non-finite L adds nothing.
 * The adds, the workspace (vidar_ray_occupancy_workspace_bytes) and the VIDAR_ERR_BAD_ARG cases are those of
 * vidar_ray_occupancy_f32; the deterministic mode's fixed point is sized for R * (K + 1) * 8 contributions. */
int vidar_sweep_evidence_f32(const float* origin, const float* pts, const float* tindex, float* hit, float* free_,
                             int F, int R, int Z, int Y, int X, int K, float step,
                             void* workspace, size_t workspace_bytes, void* stream);

/* The occupancy query (csrc/ray_march.hip, point_occupancy_body; the weights in csrc/occ_at_math.h): the decode's softmax
 * asked about ONE place on a ray instead of being scattered over all of them.  Rays, waypoints, sampler and the live rule
 * are those of vidar_ray_stats_f32; the ray runs from origin[f] through its end point q, L = |q - o| in fp32.  Waypoint k
 * owns the stretch [k step, (k + 1) step) of the ray, the query [L - extent/2, L + extent/2] (extent in voxel units).  With
 * p_k = e_k / S over the live waypoints,
 *   c_near(k) = clamp((L - extent/2 - k step) / step, 0, 1)      c_far(k) = clamp((L + extent/2 - k step) / step, 0, 1)
 *   hit  = sum p_k (c_far(k) - c_near(k))      the return lies in the query's stretch
 *   free = sum p_k (1 - c_far(k))              the return lies beyond it: the ray passed the query
 * Both are sums of non-negative terms; hit + free = sum p_k (1 - c_near(k)) in [0, 1] is the mass the ray has not spent
 * before the query; both are continuous and piecewise linear in L.  A skipped ray, a ray without a live waypoint and
 * q == o (a NaN direction: every waypoint dead) give two zeros; a query with L - extent/2 >= K step gives exact zeros.
 * +inf or NaN logits may give non-finite output.
 *   vidar_point_occupancy_f32: listed end points, origin [F,3], pts [R,3], tindex [R] -> out [R,2] = (hit, free);
 *   vidar_voxel_occupancy_f32: one ray per voxel (f, z, y, x) through its centre (x + 0.5, y + 0.5, z + 0.5), never
 *     stored -> hit, free [F,Z,Y,X]; the listed form's bits on the same end points.  The grids read like
 *     vidar_ray_occupancy_f32's, with the evidence hit + free a probability instead of a count of waypoints.
 * fp32 sums in a fixed order, no atomics, no workspace: equal inputs give equal bits in every mode, and K == 512 gives
 * the same bits through the streamed kernels.  VIDAR_ERR_BAD_ARG before any HIP call: K outside 1..vidar_ray_max_k(),
 * non-positive Z, Y, X, F <= 0 (the per-voxel form: F < 0, or F*Z*Y*X beyond the 32-bit ray index), R < 0, an extent that
 * is not finite and > 0, a NULL pointer with work to do.  R == 0 (the per-voxel form: F == 0) returns 0 and writes nothing. */
int vidar_point_occupancy_f32(const float* sigma, const float* origin, const float* pts, const float* tindex,
                              float* out /*[R,2] hit, free*/, int F, int R, int Z, int Y, int X, int K, float step,
                              float extent, void* stream);
int vidar_voxel_occupancy_f32(const float* sigma, const float* origin, float* hit /*[F,Z,Y,X]*/, float* free_,
                              int F, int Z, int Y, int X, int K, float step, float extent, void* stream);

/* ---------------------------------------------------------------------------
 * Occupancy score (csrc/occ_score.hip, per-voxel decisions in csrc/occ_score_math.h): a predicted evidence grid held
 * against a measured one, for S segments -- (sample, frame) pairs -- at once.
 *   pred, meas [S,2,V] f32 on the device: the hit plane, then the free plane, of every segment ([bs,F,2,Z,H,W] as it is);
 *   thresholds: T floats on the HOST, 1 <= T <= 8 (duplicates allowed); bins B, 0 <= B <= 16.
 * Per voxel, in fp32, every operation rounded on its own:
 *   ev_p = hit_p + free_p     ev_m = hit_m + free_m     o_p = hit_p / ev_p
 *   both = ev_p >= min_pred_evidence && ev_m >= min_meas_evidence
 *   y    = hit_m >= min_hits      a return was measured in this cell, whatever the free evidence says
 * A voxel with a non-finite value in any of its four planes takes part in no column.
 *   table [S, 5 + 3T + 2B] f64 (passed as void*, 8-byte aligned), written completely:
 *     [0] n_pred (ev_p reaches its floor)   [1] n_meas   [2] n_both   [3] n_occ (both and y)
 *     [4] brier = sum over both of (o_p - y)^2, the terms and the sum in fp64
 *     [5 + 3j ..] tp_j, fp_j, fn_j over both, with yhat = o_p >= thresholds[j]
 *     [5 + 3T + 2b ..] cnt_b, pos_b (those with y) over both, with b = min(int(o_p * B), B - 1)
 * Every column but brier is a count and exact; brier is summed in a fixed order; no atomics: equal inputs, equal bits.
 * (With min_pred_evidence <= 0 a voxel without predicted evidence has o_p = 0 / 0: it fails every threshold, falls
 * into bin 0 and makes brier NaN.)
 * workspace: vidar_occ_score_workspace_bytes(S,V,T,B,&bytes) bytes of device scratch, 8-byte aligned: the per-tile rows
 * a second launch sums in a fixed order.  S == 0 or V == 0 return 0 without a launch.  VIDAR_ERR_BAD_ARG before any HIP
 * call: negative sizes, S > 65535, T or B out of range, a NaN threshold or floor, a missing pointer, a short or
 * misaligned workspace.
 * ------------------------------------------------------------------------- */
int vidar_occ_score_workspace_bytes(int S, int V, int T, int B, int64_t* bytes);
int vidar_occ_score_f32(const float* pred, const float* meas, const float* thresholds, void* table,
                        int S, int V, int T, int B, float min_pred_evidence, float min_meas_evidence, float min_hits,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Modulated deformable convolution v2 (backbone, "next" row SURVEY 8f-1).  Replaces the sampling
 * kernels of mmcv.ops.ModulatedDeformConv2dPack (mmcv-full 1.4.0, third party); the convolution
 * itself is a GEMM of weight [Cout, C*kh*kw] with the column matrix built here.
 *   x [N,C,H,W], offset [N,2*kh*kw,Ho,Wo] ((dy,dx) per tap), mask [N,kh*kw,Ho,Wo],
 *   cols / grad_cols [N, C*kh*kw, Ho*Wo].  deform_groups == 1.
 *   kh*kw <= 9 (VIDAR_ERR_BAD_ARG beyond).  Any W >= 1: the kernels read a cell's two corner columns with one 8-byte
 *   load per row; a one-column image runs the same kernel bodies with single 4-byte loads.
 * col2im: grad_offset / grad_mask written; grad_x by one of two strategies chosen through `workspace`:
 *   NULL  : zeroed by the call, then one fp32 atomic per (channel, tap, pixel, corner);
 *   else  : the sampling positions are shared by all channels (deform_groups == 1), so the call sorts the
 *           4*K*P corner entries of every image by destination pixel into the workspace
 *           (vidar_dcn_col2im_workspace_bytes, scratch) and every destination pixel gathers its
 *           contributions -- no atomics on grad_x, fully written.  Same result up to fp32 summation order.
 * ------------------------------------------------------------------------- */
/* ---------------------------------------------------------------------------
 * Matrix products of the hot path on the gfx950 matrix cores (csrc/gemm_mfma.hip), fp32 in HBM on both sides:
 *     C[z] = act( (A[z] (M x K) * B[z] (K x N)) * scale + shift + residual[z] )      z = 0 .. batch-1
 * Replaces the library GEMMs behind the reference's nn.Linear layers -- first of all the attention value projection
 * (spatial_cross_attention.py:333-340 `value = self.value_proj(value)`, temporal_self_attention.py:197-208,
 * vidar_decoder.py:452-460), then sampling_offsets / attention_weights / output_proj of the same modules, the mmcv
 * FFN and the head MLPs -- and behind the 1x1 / deformable convolutions of the image backbone with the frozen
 * BatchNorm (+ residual + ReLU) that follows them folded into the epilogue (config vidar_1_8_nusc_1future.py:88-106).
 *   a_layout / b_layout: 0 = K-major (the contraction index is contiguous: element (m,k) at A[m*lda + k], element
 *     (k,n) at B[n*ldb + k], i.e. an nn.Linear weight [N,K] as B), 1 = MN-major (element (m,k) at A[k*lda + m],
 *     element (k,n) at B[k*ldb + n], i.e. an NCHW activation [C, H*W] as B).  C is row-major, C[m*ldc + n].
 *     Any alignment of the row starts is accepted (4-byte), any M, N, K >= 1.
 *   strideA/B/C/R: element offsets between batch items (0 = shared operand).
 *   scale, shift: optional vectors indexed by n (vec_axis 0: the bias of F.linear) or by m (vec_axis 1: per output
 *     channel of a convolution); residual: optional [M, N] tensor with leading dimension ldr; relu: 0/1.
 *   precision: 0 = VIDAR_GEMM_F32 (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate -- the arithmetic
 *     of the library kernels it replaces); 1 = VIDAR_GEMM_BF16X3: every operand element is split x = hi + lo into
 *     two bf16 while it is staged (hi = rne(x), lo = rne(x - hi): 16 significand bits, relative error <= 2^-16) and
 *     a product is lo*hi + hi*lo + hi*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  The reference runs
 *     these products in TF32 (11 significand bits; torch 1.10.1+cu111 defaults, README.md:96; tools/train.py:141-144
 *     only disables it under `close_tf32`, which no ViDAR config sets; encoder.py:98-100 is the one opt-out and
 *     stays fp32 here too).
 *   reduce = 1: ONE output C = act(sum_z A[z]*B[z] ...) -- the batch items are summed and K is additionally split
 *     (vidar_gemm_splits) so that a weight gradient fills the chip; partial products go to `workspace`
 *     (vidar_gemm_workspace_bytes) as fp32 slabs and are summed in a fixed order: deterministic, no atomics.
 *   a_rowsum (reduce = 1 and an MN-major A only; else NULL): a_rowsum[m] = sum_z sum_k A[z][m, k] written next to C --
 *     with A = grad_out^T this is the bias gradient of the nn.Linear whose weight gradient the call computes
 *     (autograd's grad_out.sum(0)): the tile-column-0 workgroups add up the A values they stage anyway, partial rows
 *     go behind the slabs and are reduced in the same fixed order.  Deterministic, and no second pass over grad_out.
 * ------------------------------------------------------------------------- */
#define VIDAR_GEMM_F32 0
#define VIDAR_GEMM_BF16X3 1
#define VIDAR_GEMM_K_MAJOR 0
#define VIDAR_GEMM_MN_MAJOR 1
int vidar_gemm_f32(const float* A, int64_t lda, int a_layout, const float* B, int64_t ldb, int b_layout, float* C,
                   int64_t ldc, int M, int N, int K, int batch, int64_t strideA, int64_t strideB, int64_t strideC,
                   const float* scale, const float* shift, int vec_axis, const float* residual, int64_t ldr,
                   int64_t strideR, int relu, int precision, int reduce, float* a_rowsum, void* workspace,
                   size_t workspace_bytes, void* stream);
int vidar_gemm_splits(int M, int N, int K, int batch, int precision, int reduce);
/* scratch of a reduced product: reduce = 1 the product alone (0 bytes when it is a single slab), reduce = 2 the product
 * with the row sums of A (`a_rowsum`): slabs + one partial row per slab */
size_t vidar_gemm_workspace_bytes(int M, int N, int K, int batch, int precision, int reduce);
/* A/B switch of the kernel's structure: 0 (default) = every wave does every job; 1 / 2 = wave-specialised workgroups
 * (4 staging waves + 4 matrix / epilogue waves, LDS double buffer, one LDS-only barrier per k-step), one / two per CU
 * (csrc/gemm_mfma.hip; measured equal or slower: profiles/r05_kbench_gemm_variants.log).  Same arithmetic, same tile
 * order: results are bit-identical.  Returns the previous value. */
int vidar_gemm_set_variant(int variant);

/* A/B switch of the DCNv2 sampling kernels.  bit 0 (default on): the grad_x gather of vidar_dcn_col2im_f32 (workspace form)
 * on 3x3 / stride 1 / dilation 1 layers copies, per tap, the window of grad_cols that can reach an 8 x 32 tile of
 * destination pixels (+ 4 pixels of learned offset) into LDS and gathers from there (sources beyond the window: global
 * loads); 0 = 4-byte global gathers everywhere (rounds 2-5).  Same sums up to fp32 order.  Values outside 0..1 are ignored.
 * Returns the previous value. */
int vidar_dcn_set_variant(int variant);
int vidar_dcn_im2col_f32(const float* x, const float* offset, const float* mask, float* cols, int N,
                         int C, int H, int W, int Ho, int Wo, int kh, int kw, int stride, int pad,
                         int dil, void* stream);
/* Deterministic mode (vidar_set_deterministic): grad_x is the fixed-point plain scatter for every shape and variant;
 * its workspace depends on C, which vidar_dcn_col2im_workspace_bytes does not take: *bytes = 8 * (N*C*H*W + 1).  In the mode
 * vidar_dcn_col2im_f32 returns VIDAR_ERR_BAD_ARG with a smaller workspace. */
int vidar_dcn_col2im_det_workspace_bytes(int N, int C, int H, int W, int64_t* bytes);
int vidar_dcn_col2im_f32(const float* grad_cols, const float* x, const float* offset,
                         const float* mask, float* grad_x, float* grad_offset, float* grad_mask,
                         int N, int C, int H, int W, int Ho, int Wo, int kh, int kw, int stride,
                         int pad, int dil, void* workspace, size_t workspace_bytes, void* stream);
/* (the gather's scratch; NOT the answer in the deterministic mode, where vidar_dcn_col2im_det_workspace_bytes sizes it) */
size_t vidar_dcn_col2im_workspace_bytes(int N, int H, int W, int Ho, int Wo, int kh, int kw);

/* 3x3 convolution (stride 1, pad 1, dilation 1, groups 1) with FEW output channels as an implicit GEMM on the fp32
 * matrix cores:  out[N,Cout,H,W] = conv2d(x[N,C,H,W], weight[Cout,C,3,3]) + bias  (bias may be NULL).
 * Replaces the library convolution behind `conv_offset` of mmcv's ModulatedDeformConv2dPack -- the 3x3 that predicts the
 * 18 offsets + 9 masks of every DCNv2 bottleneck (vidar_1_8_nusc_1future.py:93-95: DCNv2 on ResNet101 stages 3 and 4 =
 * 26 of the backbone's 37 3x3 convolutions); its backward stays the library's.  fp32 products are exact, the sum runs
 * channel-major with the 9 taps inside (within 1e-5 of an fp64 convolution, tests/test_conv3x3_gpu.py).
 * workspace: vidar_conv3x3_few_workspace_bytes(C) bytes (the packed weights; written by the call).
 * Limits (VIDAR_ERR_BAD_ARG otherwise): Cout <= 32, C % 8 == 0, W <= 191, H*W < 2^30. */
size_t vidar_conv3x3_few_workspace_bytes(int C);
int vidar_conv3x3_few_f32(const float* x, const float* weight, const float* bias, float* out, int N, int C, int H, int W,
                          int Cout, void* workspace, size_t workspace_bytes, void* stream);

/* Fused frozen-BatchNorm epilogue of the backbone: y = act(x*scale[c] + shift[c] (+ residual)),
 * NCHW, scale = gamma/sqrt(var+eps), shift = beta - mean*scale (BN is frozen / eval in every ViDAR
 * config: vidar_1_8_nusc_1future.py:93-95).  relu: 0/1.  residual / grad_residual may be NULL.
 * bwd needs y (the forward output) for the ReLU mask; scale/shift receive no gradient (frozen): grad_residual =
 * (y > 0 ? grad_y : 0), grad_x = grad_residual * scale[c]; with relu = 0, y is never read.
 * NaN: the ReLU is fmaxf(v, 0), so with relu = 1 a NaN (NaN input, inf - inf) comes out as 0 -- as from the GEMM
 * epilogue (csrc/gemm_mfma.hip) -- and the stem does the same; with relu = 0 it propagates.  +-inf follow IEEE.
 * N = 0 is an empty problem (returns 0, writes nothing); N < 0, C <= 0 or HW <= 0 is VIDAR_ERR_BAD_ARG.
 * N*C: fwd and bwd launch one grid row (gridDim.y) per channel plane and set no limit of their own; the HIP runtime
 * takes a y extent past 65535 on gfx950 (measured: 65537 and 33 x 2048 planes give the same bits as few planes,
 * tests/test_affine_act_gpu.py; stage 4 of the backbone on a two-sample batch has 48 x 2048).  The stem keeps its own,
 * narrower limit (below).  Pointers need no alignment: the float4 kernels run when HW % 4 == 0 and every operand is
 * 16-byte aligned, the scalar ones otherwise, with the same results. */
int vidar_affine_act_fwd_f32(const float* x, const float* scale, const float* shift,
                             const float* residual, float* y, int N, int C, int HW, int relu,
                             void* stream);
/* Stem of the backbone in one pass: y[N,C,Ho,Wo] = max_pool2d(relu(x*scale[c] + shift[c]), 3, stride 2, pad 1) with
 * Ho = (H-1)/2 + 1, Wo = W/2 -- mmdet ResNet.forward's conv1 -> norm1 -> relu -> maxpool with the frozen BN of the
 * ViDAR configs (vidar_1_8_nusc_1future.py:86-95, frozen_stages=1: forward only).  Bit-identical to
 * vidar_affine_act_fwd_f32(relu=1) followed by the pooling.  VIDAR_ERR_BAD_ARG unless W % 4 == 0, x 16-byte and
 * y 8-byte aligned, N*C <= 65535 (the caller then takes the two-kernel path). */
int vidar_stem_bn_relu_pool_f32(const float* x, const float* scale, const float* shift, float* y, int N, int C,
                                int H, int W, void* stream);
int vidar_affine_act_bwd_f32(const float* grad_y, const float* y, const float* scale, float* grad_x,
                             float* grad_residual, int N, int C, int HW, int relu, void* stream);

/* ---------------------------------------------------------------------------
 * Deformable convolution v3, the core op of the InternImage backbone (csrc/dcnv3.hip).  Replaces the reference's
 * `DCNv3` extension (projects/mmdet3d_plugin/bevformer/backbones/ops_dcnv3: dcnv3_forward / dcnv3_backward,
 * src/cuda/dcnv3_im2col_cuda.cuh:217-276, :149-213, :776-839).  Channel-last:
 *   input [N,H,W,G*gc], offset [N,Ho,Wo,G*P*2] as (w, h) pairs, mask [N,Ho,Wo,G*P], out / grad_out [N,Ho,Wo,G*gc],
 *   P = kh*kw with point p = i_w*kh + j_h, Ho = (H + 2*pad_h - (dil_h*(kh-1)+1)) / stride_h + 1 (same for Wo),
 *   out = sum_p mask_p * bilinear(input[:, g, :], loc_p), loc as in :249-260; a point counts iff
 *   loc_h > -1 && loc_w > -1 && loc_h < H && loc_w < W (zero outside, NaN locations contribute nothing).
 * group_channels: any positive value (16-byte loads when it is a multiple of 4 and the buffers are 16-byte aligned).
 * VIDAR_ERR_BAD_ARG: non-positive sizes, kh*kw > 1024, a kernel extent larger than the padded input, or any of the
 * tensors holding 2^31 - 512 elements or more.  The reference's im2col_step only batches its launches and has no
 * counterpart here.
 * backward: grad_offset (already multiplied by offset_scale, :212-213) and grad_mask are fully written with plain stores
 * in a fixed summation order (bit-reproducible); grad_input is zeroed by the call, then accumulated with fp32 atomics.
 * `workspace` / vidar_dcnv3_backward_workspace_bytes are RESERVED: every form of the backward accumulates on chip or
 * straight into grad_input, the function returns 0 and the call ignores both arguments (NULL / 0 is what callers pass).
 * ------------------------------------------------------------------------- */
/* A/B switch of the grad_input accumulation of vidar_dcnv3_backward_f32 (bit 0: lane layout, bit 1: LDS window).
 *   0: one fp32 atomic per (channel, point, corner), an item's lanes owning 4 channels each (16-byte loads);
 *   1 (default, measured fastest: profiles/kbench_dcnv3.md): the same with ONE channel per lane, so that an atomic
 *      instruction of an item covers one contiguous gc*4-byte segment;
 *   2 / 3: a workgroup owns a tile of output pixels of one (image, group), sums the tile's contributions in an LDS window
 *      of the input (tile + kernel extent + 3 pixels of learned offset on every side) and flushes the window once,
 *      channel-contiguous; samples beyond the window add straight to memory; lanes as in 0 / 1.  Shapes whose window
 *      exceeds 64 KiB of LDS take form 0 / 1.
 * Same sums up to fp32 order; grad_offset / grad_mask are plain stores in every form.  Values outside 0..3 are ignored.
 * Returns the previous value. */
int vidar_dcnv3_set_variant(int variant);
int vidar_dcnv3_forward_f32(const float* input, const float* offset, const float* mask, float* out, int N, int H, int W,
                            int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                            int group, int group_channels, float offset_scale, void* stream);
size_t vidar_dcnv3_backward_workspace_bytes(int N, int H, int W, int kh, int kw, int stride_h, int stride_w, int pad_h,
                                            int pad_w, int dil_h, int dil_w, int group, int group_channels);
int vidar_dcnv3_backward_f32(const float* input, const float* offset, const float* mask, const float* grad_out,
                             float* grad_input, float* grad_offset, float* grad_mask, int N, int H, int W, int kh, int kw,
                             int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int group,
                             int group_channels, float offset_scale, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Detection loss tail of the BEVFormer fine-tune step (csrc/det_loss.hip): Hungarian cost matrices and the focal / L1
 * losses of ALL decoder layers and samples in one launch each (bevformer/dense_heads/bevformer_head.py:215-393,
 * core/bbox/assigners/hungarian_assigner_3d.py:106-123).  fp32, latency-bound; its point is one host read per step.
 *   cls [NL,B,Q,C] logits (C <= 64), box [NL,B,Q,10] predictions in normalised code (cx, cy, log w, log l, cz, log h,
 *   sin, cos, vx, vy); ground truth packed over the batch: gt_box_norm [total_g,10] (normalize_bbox applied),
 *   gt_label [total_g] i32 in [0, C), gt_start [B+1] i32 (device; sample b owns rows gt_start[b] .. gt_start[b+1]).
 * match_cost: cost [NL, Q*total_g]; sample b's block of a layer's row starts at Q*gt_start[b] and is [Q, G_b] row-major:
 *   p = sigmoid(cls[l,b,q,gt_label[g]])
 *   cost = cls_weight * (-alpha (1-p)^gamma log(p + 1e-12) + (1-alpha) p^gamma log(1 - p + 1e-12))
 *        + reg_weight * sum_{k<8} |box[l,b,q,k] - gt_box_norm[g,k]|
 *   total_g == 0 (or any empty extent) returns 0 without a launch; samples with G_b == 0 write nothing.
 * loss_fwd: labels [NL,B,Q] i32 (C = background), matched_gt [NL,B,Q] i32 (index inside the sample's rows, -1 = none)
 *   sums[l,0] = sum over (b,q,c) of the sigmoid focal loss, mmcv semantics: target class
 *               -alpha (1-p)^gamma log(max(p, FLT_MIN)), other classes -(1-alpha) p^gamma log(max(1-p, FLT_MIN))
 *   sums[l,1] = sum over matched (b,q) whose target row is finite in all 10 entries of
 *               sum_k code_weights[k] |box[l,b,q,k] - gt_box_norm[matched,k]|
 *   Deterministic: per-workgroup partials (fp64 sums of the fp32 terms) in `workspace`
 *   (vidar_det_loss_workspace_bytes, caller-owned scratch, 8-byte aligned), then a fixed-order pass per layer; no
 *   floating-point atomics.
 * loss_bwd: grad_sums [NL,2] -> grad_cls, grad_box written in full (zeros where nothing flows); sign(0) = 0.
 * VIDAR_ERR_BAD_ARG: negative sizes, C outside 1..64, NL > 65535, B*Q or total_g*10 beyond the 32-bit index range used,
 * a missing pointer, a workspace that is too small.
 * ------------------------------------------------------------------------- */
int vidar_det_match_cost_f32(const float* cls, const float* box, const float* gt_box_norm, const int32_t* gt_label,
                             const int32_t* gt_start, float* cost, float alpha, float gamma, float cls_weight,
                             float reg_weight, int NL, int B, int Q, int C, int total_g, void* stream);
size_t vidar_det_loss_workspace_bytes(int NL, int B, int Q);
int vidar_det_loss_fwd_f32(const float* cls, const float* box, const int32_t* labels, const int32_t* matched_gt,
                           const float* gt_box_norm, const int32_t* gt_start, const float* code_weights, float* sums,
                           float alpha, float gamma, int NL, int B, int Q, int C, int total_g, void* workspace,
                           size_t workspace_bytes, void* stream);
int vidar_det_loss_bwd_f32(const float* cls, const float* box, const int32_t* labels, const int32_t* matched_gt,
                           const float* gt_box_norm, const int32_t* gt_start, const float* code_weights,
                           const float* grad_sums, float* grad_cls, float* grad_box, float alpha, float gamma, int NL,
                           int B, int Q, int C, int total_g, void* stream);

/* ---------------------------------------------------------------------------
 * Hungarian assignment of the detection loss tail on the device (csrc/det_assign.hip, per-problem body in
 * csrc/det_assign_math.h): scipy.optimize.linear_sum_assignment for ALL NL * B (layer, sample) cost blocks of a step in
 * one launch, one workgroup per problem, no host read.  Shortest augmenting paths with dual variables; rows are the
 * shorter side min(Q, G_b); duals and path costs are fp64 on the fp32 costs widened (fp32 duals lose the optimum at
 * 900 x 512).
 *   cost [NL, Q*total_g] f32 as vidar_det_match_cost_f32 writes it (sample b's [Q, G_b] row-major block of a layer's row
 *   at Q*gt_start[b]); gt_start [B+1] i32 on the DEVICE -- the kernel reads G_b there, the host passes total_g only.
 *   matched [NL,B,Q] i32: index inside the sample's ground truth, -1 = background; written completely (G_b == 0, Q > G_b
 *   and Q < G_b alike).  status [NL*B] i32, written completely:
 *     0 solved;
 *     1 the block holds NaN or -inf (SciPy: "matrix contains invalid numeric entries"), found by a pre-pass;
 *     2 every perfect matching of the short side needs a +inf entry (SciPy: "cost matrix is infeasible"; +inf entries that
 *       can be avoided are legal);
 *     3 the sample's gt_start range is not inside 0 .. total_g.
 *   A problem with a non-zero status has -1 in all of its matched row; the other problems of the launch are unaffected.
 * Ties: equal minima of a search step resolve to the LOWEST COLUMN INDEX, so the result does not depend on lane count,
 * wave count or arrival order.  Where the optimum is unique the assignment equals SciPy's; on exact ties only the total is.
 * Extent: the solver state stays in LDS, which holds a long side max(Q, G_b) <= 2048 and a short side min(Q, G_b) <= 1024.
 * The host knows total_g >= G_b only, so the rule is stated on it: max(Q, total_g) <= 2048 and min(Q, total_g) <= 1024.
 * vidar_det_assign_workspace_bytes reports *bytes = -1 (and returns 0) for an unsupported extent -- the caller keeps its
 * host path -- and otherwise the scratch the launch needs (a transposed copy of the cost; 4-byte aligned, caller-owned).
 * Deterministic: no atomics, nothing shared between workgroups; same inputs, same bytes, whatever slot a problem has.
 * Every loop of the kernel is bounded by the problem's size: no input makes it spin.
 * NL == 0 or B == 0 returns 0 without a launch.  total_g == 0 (cost and workspace may be NULL) and Q == 0 (matched may be
 * NULL) still launch: THE LAUNCH fills matched with -1 and status with 0, the caller does not.
 * VIDAR_ERR_BAD_ARG before any HIP call: negative sizes, NL*B beyond 2^31-1, a missing pointer, a workspace that is too
 * small or misaligned, an unsupported extent.
 * ------------------------------------------------------------------------- */
int vidar_det_assign_workspace_bytes(int NL, int B, int Q, int total_g, int64_t* bytes);
int vidar_det_assign_f32(const float* cost, const int32_t* gt_start, int32_t* matched, int32_t* status, int NL, int B,
                         int Q, int total_g, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Matching step of the nuScenes detection metric, mAP / NDS (csrc/det_eval.hip, pair errors in csrc/det_eval_math.h).  The
 * reference delegates the metric to the nuScenes devkit (datasets/nuscnes_eval.py:628-676 -> accumulate / calc_ap /
 * calc_tp); the semantics here are recalled from the devkit, which is not part of the reference tree.
 * Greedy, confidence-ordered nearest-centre matching for NT distance thresholds at once; one wave owns one (segment,
 * threshold), segment = (sample, class) = sample * num_classes + class, so nothing is shared, nothing is atomic and the
 * result is deterministic.
 *   pred_box [P,9] f32 (x, y, z, three sizes, yaw, vx, vy), grouped by segment and, inside a segment, in PROCESSING ORDER
 *   (score descending, equal scores with the later input index first); pred_attr [P] i32 attribute ids (NULL: none);
 *   gt_box [G,9] / gt_attr [G] (id < 0: no attribute) grouped by segment; pred_start / gt_start [NS+1] i32 (device):
 *   segment s owns rows start[s] .. start[s+1], start[0] = 0 and start[NS] = P resp. G.  dist_ths: NT <= 8 floats on the
 *   HOST, in metres.
 * A prediction takes the nearest row of its segment that is not taken yet -- squared centre distance on x, y in fp32,
 * dx*dx + dy*dy without contraction, the lowest row on ties -- and matches iff that distance is < th*th, strictly; a
 * prediction whose nearest untaken row is too far is a false positive even if a taken row is nearer.
 *   match    [NT,P] i32: the matched row of gt_box, or -1        gt_match [NT,G] i32: the matched row of pred_box, or -1
 *   err      [P,5]  f32, for threshold tp_index (-1: none, err may be NULL): trans_err, vel_err, scale_err, orient_err,
 *            attr_err of the matched pair (period pi for segments of class barrier_class, 2 pi otherwise; NaN velocity
 *            -> NaN vel_err; no ground-truth attribute -> NaN attr_err), NaN in all five for an unmatched row.
 * All three are written completely.  Any segment size (up to 256 annotations of a segment stay in registers, more are
 * streamed).  Empty extents (NS, NT, or P and G all zero) return 0 without a launch; negative sizes, NT > 8, a tp_index
 * outside -1 .. NT-1, num_classes < 1 or a missing pointer return VIDAR_ERR_BAD_ARG before any HIP call.
 * ------------------------------------------------------------------------- */
int vidar_det_eval_match_f32(const float* pred_box, const int32_t* pred_attr, const int32_t* pred_start,
                             const float* gt_box, const int32_t* gt_attr, const int32_t* gt_start, const float* dist_ths,
                             int32_t* match, int32_t* gt_match, float* err, int P, int G, int NS, int NT, int tp_index,
                             int num_classes, int barrier_class, void* stream);

/* ---------------------------------------------------------------------------
 * Ray errors of the forecasting metric, L1 / AbsRel along the ground-truth rays (csrc/ray_eval.hip, per-ray arithmetic
 * in csrc/ray_eval_math.h): projects/mmdet3d_plugin/bevformer/utils/eval_utils.py:185-225 for S segments at once, a
 * segment being one (sample, frame) pair.  All arithmetic is fp64 on the fp32 inputs widened first, as the reference's
 * numpy is, and the nearest neighbour is searched in fp64, as chamferdist does for the reference's fp64 input.
 *   pred [P,3] f32 / gt [G,3] f32, grouped by segment; pred_start / gt_start [S+1] i32 on the DEVICE: segment s owns rows
 *   start[s] .. start[s+1], start[0] = 0 and start[S] = P resp. G (values outside are clamped); origin [S,3] f32.
 *   max_gt: a HOST bound on the longest ground-truth segment; it sizes the grid, tiles = ceil(max_gt / 256), and rays
 *   of a segment beyond it are not scored.
 * With (theta, phi, d) = (atan2(x, y), atan2(z, y), sqrt(x*x + y*y + z*z)) of a point minus its segment's origin: a
 * prediction is kept iff d_hat > 1e-2, a ground-truth ray is counted iff d > 1e-2; every counted ray takes the kept
 * prediction of its segment with the smallest dtheta*dtheta + dphi*dphi (strict <: the lowest row wins ties; no
 * wrap-around), moves it onto its own ray, interp = origin + d_hat * unit(gt - origin), and is charged
 * |clamp(gt) - clamp(interp)| (L1) and that over the clamped ray length (AbsRel), unless clamp(gt) misses the volume or
 * is <= 0.01 long.  clamp cuts a ray to PC_RANGE = [-70, -70, -4.5, 70, 70, 4.5] (the metric's own range).
 *   partial [S,tiles,3] f64: (sum of L1, sum of AbsRel, counted rays) of each tile of 256 rays, summed in a fixed order;
 *            tiles beyond a segment hold zeros.  Their sum over tiles is the segment's (sum L1, sum AbsRel, count):
 *            l1_error = sum L1 / count.  A segment with counted rays and no kept prediction gives NaN sums (the
 *            reference raises there).  No atomics: equal inputs give equal bits.
 *   nn_idx  [G]   i32, may be NULL: the chosen row RELATIVE to the segment's start, -1 for an uncounted ray or a segment
 *            without a kept prediction
 *   ray_err [G,2] f64, may be NULL: the ray's two terms, 0 where it contributes nothing
 *   interp  [G,3] f64, may be NULL: the interpolated point, NaN where nn_idx is -1
 * The f64 buffers are passed as void*.  workspace: vidar_ray_eval_workspace_bytes(P) bytes of device scratch, 8-byte
 * aligned.  S == 0 or G == 0 return 0 without a launch; negative sizes, max_gt == 0 with rays to score, a missing
 * required pointer or a short workspace return VIDAR_ERR_BAD_ARG before any HIP call.
 * ------------------------------------------------------------------------- */
int vidar_ray_eval_workspace_bytes(int P, int64_t* bytes);
int vidar_ray_eval_f64(const float* pred, const int32_t* pred_start, const float* gt, const int32_t* gt_start,
                       const float* origin, void* partial, int32_t* nn_idx, void* ray_err, void* interp, int P, int G,
                       int S, int max_gt, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Device-side image pipeline (csrc/img_prep.hip, math in csrc/img_prep_math.h): raw uint8 HWC BGR frames -> the fp32
 * [n, 3, Hp, Wp] network input, with the bits of the host pipeline (PhotoMetricDistortionMultiViewImage, CropResizeFlipImage
 * = PIL crop / bicubic resize / flip, NormalizeMultiviewImage, RandomScaleImageMultiViewImage, PadMultiViewImage:
 * projects/mmdet3d_plugin/datasets/pipelines/transform_3d.py:8-190,:295-327, augmentation.py:10-203).  n = all images of a
 * sample (T * cams); every call is one launch, vidar_img_resample_u8 one per pass (at most two).
 *
 * photo [n, 12] f32 (device), per image: [0] shift, [1] gain before the HSV stage, [2] saturation factor, [3] hue turn in
 *   degrees, [4] gain after the HSV stage, [5] flags (1 shift, 2 gain-before, 4 saturation, 8 turn, 16 gain-after; a step
 *   whose bit is clear is not evaluated), [6..8] channel permutation, out[c] = in[perm[c]] (0 1 2 = none), [9..11] reserved.
 *   Every step is one correctly rounded fp32 operation in numpy's order; bit-identical to the host path.
 * photometric_u8: src [n,H,W,3] u8 -> dst [n,H,W,3] u8, the float -> uint8 rule being: truncate toward zero to int32, keep
 *   the low 8 bits.  photometric_f32: the same values before the cast, dst [n,H,W,3] f32.
 * resample_u8: PIL's two-pass 8-bit bicubic resampler of the window (crop_x, crop_y, crop_w, crop_h) of every image
 *   -> dst [n,out_h,out_w,3] u8, mirrored left-right when `flip`.  tab_x / tab_y (device, int32): [out, 2] pairs (first
 *   source index inside the window, tap count) followed by [out, ksize] fixed-point coefficients (22 fractional bits),
 *   ksize = 2 * ceil(2 * max(in / out, 1)) + 1; an output value is clip((sum pixel * k + 2^21) >> 22, 0, 255), horizontal
 *   pass first, uint8 in between.  A NULL table (with ksize 0) skips that pass and needs in == out; `flip` needs the
 *   horizontal pass (the in == out table is the identity).  With both passes the intermediate [n,crop_h,out_w,3] plane lives
 *   in `workspace` (vidar_img_resample_workspace_bytes, caller-owned).  Table CONTENTS cannot send an access outside the
 *   window (bounds are clamped on the device); the caller guarantees the table's SIZE.
 * normalise_f32: src [n,H,W,3] u8 -> dst [n,3,Hp,Wp] f32 (16-byte aligned, Wp a multiple of 4): out channel c =
 *   (in channel (to_rgb ? 2 - c : c) - mean[c]) / stdv[c]; when (out_h, out_w) != (H, W) the normalised values are resized
 *   bilinearly with torch's align_corners=False rule (scale = float(in) / out, src = scale * (dst + 0.5) - 0.5 clamped at
 *   0); rows >= out_h and columns >= out_w are written as 0 by the call.  photo != NULL applies the photometric stage to the
 *   source pixels first, in fp32 without the uint8 cast (the OpenScene order).  mean / stdv: 3 floats each on the HOST.
 * VIDAR_ERR_BAD_ARG (nothing is launched): a missing pointer, a non-positive size, a window that is not inside the image,
 *   a ksize that does not belong to (in, out), a skipped pass with in != out, both passes skipped, a workspace that is too
 *   small, Hp < out_h, Wp < out_w, Wp % 4 != 0, a misaligned dst.
 * ------------------------------------------------------------------------- */
#define VIDAR_IMG_PHOTO_FLOATS 12
int vidar_img_photometric_u8(const uint8_t* src, const float* photo, uint8_t* dst, int n, int H, int W, void* stream);
int vidar_img_photometric_f32(const uint8_t* src, const float* photo, float* dst, int n, int H, int W, void* stream);
size_t vidar_img_resample_workspace_bytes(int n, int crop_h, int out_w);
int vidar_img_resample_u8(const uint8_t* src, uint8_t* dst, int n, int H, int W, int crop_x, int crop_y, int crop_w,
                          int crop_h, int out_w, int out_h, const int32_t* tab_x, int ksize_x, const int32_t* tab_y,
                          int ksize_y, int flip, void* workspace, size_t workspace_bytes, void* stream);
int vidar_img_normalise_f32(const uint8_t* src, const float* photo, float* dst, int n, int H, int W, int out_h, int out_w,
                            int Hp, int Wp, const float* mean, const float* stdv, int to_rgb, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIDAR_HIP_H_ */
