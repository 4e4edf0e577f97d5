/*
 * egohmr_hip.h - C ABI of libegohmr_hip.so: the MI355X (gfx950) kernels of the EgoHMR stage-2
 * diffusion-sampling hot path.
 *
 * The reference (sanweiliti/EgoHMR) is single-process eager PyTorch and has NO FFI boundary of
 * its own.  Each entry point below therefore names the reference Python
 * interface (file:line under /root/reference) whose arithmetic it replaces; the Python host side
 * (egohmr_amd/) keeps those interfaces' names and calls in here through ctypes.
 *
 * Conventions
 *   - every `const float*` / `float*` is a DEVICE pointer, float32, contiguous row-major, owned by
 *     the caller, unless the parameter comment says "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call is
 *     stream-ordered, never synchronises and never allocates after *_create, so a sequence of
 *     calls may be captured into a hipGraph;
 *   - return value: 0 on success, negative on error (-22 bad argument, -12 out of memory,
 *     -5 HIP runtime error).  ehm_last_error() returns a thread-local description;
 *   - handles are opaque; create/destroy are host-synchronous.
 */
#ifndef EGOHMR_HIP_H
#define EGOHMR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EHM_NUM_JOINTS 24
#define EHM_NUM_BETAS 10
#define EHM_POSE_DIM 144 /* 24 joints x 6-D rotation */

const char* ehm_last_error(void);
/* compile-time facts, for the loader's sanity check: returns "gfx950" */
const char* ehm_target_arch(void);
/* optional parts this library was built with, space separated ("" for the default build): "stamps" (-DEHM_STAMPS: in-kernel time stamps for
 * tools/stamp_*.py).  (The experiment engines of rounds 4 - 5 - the one-launch sampling loop, the 96 x 64 wave tile - are gone from the tree: their
 * records are docs/EXPERIMENTS.md 3.2 / 3.7, their code is in the history.) */
const char* ehm_build_features(void);

/* ------------------------------------------------------------------ geometry ------------------ */
/* utils/geometry.py:47-66 rot6d_to_rotmat(x, rot6d_mode).  x6d [n,6] -> R [n,3,3].
 * mode 0 = 'prohmr' (a1 = x[0:3], a2 = x[3:6]); 1 = 'diffusion' (a1 = x[0::2], a2 = x[1::2]). */
int ehm_rot6d_to_rotmat(const float* x6d, float* R, int64_t n, int mode, void* stream);
/* vector-Jacobian product of the above (autograd of geometry.py:47-66 as used under
 * torch.enable_grad() in models/egohmr/egohmr.py:518-529): gR [n,3,3] -> gx [n,6]. */
int ehm_rot6d_to_rotmat_bwd(const float* x6d, const float* gR, float* gx, int64_t n, int mode, void* stream);
/* utils/konia_transform.py:316-340 rotation_matrix_to_angle_axis (-> rotation_matrix_to_quaternion :349-443 in WXYZ order, quaternion_to_angle_axis
 * :560-630; eps = 1e-6 in the clamps, safe_zero_division :343-346, torch_safe_atan2 :44-47): R [n,3,3] -> aa [n,3].  The `full_pose` feed of the
 * COAP / VolSMPL collision models (models/egohmr/egohmr.py:495, :540; egohmr_volsmpl.py:555, :596). */
int ehm_rotmat_to_angle_axis(const float* R, float* aa, int64_t n, void* stream);
/* vector-Jacobian product of the above through the branch the forward took (autograd through torch.where / clamp_min, as under
 * torch.enable_grad() in egohmr.py:518-545): gaa [n,3] -> gR [n,3,3]. */
int ehm_rotmat_to_angle_axis_bwd(const float* R, const float* gaa, float* gR, int64_t n, void* stream);

/* ------------------------------------------------------------------ SMPL body model ----------- */
typedef struct ehm_smpl ehm_smpl;

/* smplx.create('data/smpl', model_type='smpl', ...) (models/egohmr/egohmr.py:105-107): uploads /
 * re-packs the model constants.  v_template [V,3], shapedirs [V,3,10], posedirs [207,V*3],
 * J_regressor [24,V], lbs_weights [V,24] are device pointers (smplx buffer layouts);
 * parents [24] and extra_joint_vertex_ids [n_extra] are HOST int32 arrays. */
int ehm_smpl_create(ehm_smpl** out, const float* v_template, const float* shapedirs, const float* posedirs,
                    const float* J_regressor, const float* lbs_weights, const int32_t* parents,
                    const int32_t* extra_joint_vertex_ids, int num_verts, int n_extra, void* stream);
void ehm_smpl_destroy(ehm_smpl* h);

/* smplx SMPL.forward(betas, body_pose, global_orient, pose2rot=False) as called at
 * models/egohmr/egohmr.py:276,492,537 and test_egohmr.py:291.
 * betas [B,10]; rotmats [B,24,3,3] (global_orient then body_pose); verts [B,V,3];
 * joints [B,24+n_extra,3]; A_out (may be NULL) [B,24,3,4] = the skinning transforms. */
int ehm_smpl_forward(ehm_smpl* h, const float* betas, const float* rotmats, float* verts, float* joints,
                     float* A_out, int B, void* stream);

/* egohmr.py:258-260 + :276 fused: x [B,144] (normalised 6-D pose), pose6d = x*std+mean,
 * R = rot6d_to_rotmat(pose6d,'diffusion'), then SMPL.forward.  mean/std [144]; R_out (may be NULL)
 * [B,24,3,3]; pose6d_out (may be NULL) [B,144]. */
int ehm_smpl_forward_rot6d(ehm_smpl* h, const float* betas, const float* x, const float* mean, const float* std,
                           float* verts, float* joints, float* R_out, float* pose6d_out, float* A_out, int B,
                           void* stream);

/* ------------------------------------------------------------------ Modulated-GCN denoiser ---- */
/* One ModulatedGraphConv (+ optional BatchNorm1d) in the reference's parameter layout
 * (models/egohmr/modulated_gcn/modulated_gcn_conv.py:16-37, modulated_gcn.py:12-13). */
typedef struct {
  const float* W;         /* [2, in_dim, out_dim] */
  const float* M;         /* [24, out_dim]        */
  const float* adj2;      /* [24, 24]             */
  const float* bias;      /* [out_dim]            */
  const float* bn_weight; /* [out_dim] or NULL (no BatchNorm/ReLU after this conv) */
  const float* bn_bias;
  const float* bn_mean;
  const float* bn_var;
  int in_dim;
  int out_dim;
} ehm_gconv_params;

typedef struct ehm_gcn ehm_gcn;

/* ModulatedGCN(adj, in_dim, hid_dim, out_dim=6, num_layers) (modulated_gcn.py:60-97) with the
 * step-invariant part of the input conv hoisted (SURVEY.md section 0 finding 5):
 *   adj        [24,24]  fixed adjacency (egohmr.py:86-93)
 *   input_conv          epilogue parameters of gconv_input (its W is consumed by the caller's
 *                       one-off projections, so .W may be NULL; in_dim is ignored)
 *   hidden              2*num_blocks convs hid->hid, order gconv_layers.{b}.gconv1, gconv2
 *   output_conv         hid->6, no batch norm
 * HOST array of structs holding DEVICE pointers. */
int ehm_gcn_create(ehm_gcn** out, const float* adj, const ehm_gconv_params* input_conv,
                   const ehm_gconv_params* hidden, int num_hidden, const ehm_gconv_params* output_conv,
                   int hid_dim, void* stream);
void ehm_gcn_destroy(ehm_gcn* h);

/* Arithmetic of the hidden convs (docs/EXPERIMENTS.md 3.2).  0 = f32-input MFMA (exact f32 products; what a fresh handle is in);
 * 1 = "f16x3": f16 MFMA on hi/lo-split operands, three products per term, f32 accumulate (22-bit operands,
 * f32-grade results); 2 = plain f16 operands and f16 activation storage (NOT parity-grade on its own - BASELINE config 5's
 * fp16 denoiser, and the early steps of ehm_sample_desc.lowprec_steps);
 * 3 = "f16x2": mode 1's operands, buffers and activation formats bit for bit, but TWO products per term: a_hi * (w_hi + w_lo) - the
 * activations enter as their f16 hi halves, the weights in full (the al * wh MFMAs are not issued: 2/3 of mode 1's matrix work).  The stores
 * still write hi + lo, so a mode-1 conv behind it reads full operands.  Not parity-grade on its own either: the middle tier of the
 * calibrated precision schedule (ehm_sample_desc.twoterm_steps).
 * Activation matrices exchanged between ehm_gcn_input_layer -> ehm_gcn_hidden_layer / _stack: mode 0 float32 [rows_pad,hid];
 * mode 1 the opaque "X2" split format (same byte size), except that the LAST hidden conv writes float32 (with no hidden conv: the input conv); mode 2 f16
 * [rows_pad,hid] throughout.  ehm_gcn_output_layer reads what the handle's mode produces.  ehm_gcn_pack/unpack_activations convert float32 <-> the mode's format (tests, interop). */
enum { EHM_PREC_F32 = 0, EHM_PREC_F16X3 = 1, EHM_PREC_F16 = 2, EHM_PREC_F16X2 = 3 };
int ehm_gcn_set_precision(ehm_gcn* h, int mode);
int ehm_gcn_get_precision(const ehm_gcn* h);
/* group = ehm_gcn_activation_group(h): 32 = X2 split format (modes 1 and 3), 0 = plain f16 (mode 2); pass it to pack / unpack */
int ehm_gcn_activation_group(const ehm_gcn* h);
/* Size the handle's internal scratch (chained-launch counters, output-conv responses) for batches of up to max_bodies bodies x
 * passes.  ehm_gcn_create reserves 256 x 2; a larger batch grows the scratch on first use (a hipMalloc - so call this first when
 * the launches are going to be captured into a hipGraph). */
int ehm_gcn_reserve(ehm_gcn* h, int max_bodies, int passes);
int ehm_gcn_pack_activations(const float* X, void* X2, int64_t rows, int K, int group, void* stream);
int ehm_gcn_unpack_activations(const void* X2, float* X, int64_t rows, int K, int group, void* stream);
/* ehm_gcn_pack_activations into the handle's own activation format (modes 1 / 2; K = hid_dim) WITH the range guard of the conv kernels: a value with
 * |x| >= 65504 (clamped: see ehm_gcn_stack_status) raises bit 2 of the handle's status word. */
int ehm_gcn_pack_activations_checked(ehm_gcn* h, const float* X, void* X2, int64_t rows, void* stream);

/* rows of the activation matrices must be padded to a multiple of this many rows (zero-filled) */
int ehm_gcn_row_tile(void);

/* gconv_input (modulated_gcn.py:21-28 applied to egohmr.py:236/:245's concatenated feature) with
 * the conditioning/timestep part pre-projected.  For virtual body vb = p*B + b (p = 0 conditional
 * pass, p = 1 image-masked pass, egohmr.py:239-246), joint j, branch k (W[0] / W[1]):
 *   pre_k = (p==0 ? vis[b,j] * h_img[b,k,:] : 0) + h_oth[b,k,:] + tvec[k,:] + x[b,j,0:6] @ Wx[k]
 * then the modulated adjacency mix, bias, BatchNorm(eval), ReLU.
 *   h_img, h_oth [B,2,hid]; vis [B,24] uint8; x [B,144]; Wx [2,6,hid]; tvec [2,hid];
 *   out [rows_pad,hid], rows = passes*B*24 ((B + num_masked)*24 under ehm_gcn_set_pass_map). */
/* What the second pass of diffuse_fuse masks (EgoHMR.mask_cond(force_mask=True), egohmr.py:150-158): 0 (default) = the image features only
 * (only_mask_img_cond=True, the shipped test configuration) -> pre_k of p = 1 drops h_img; 1 = the whole condition (only_mask_img_cond=False)
 * -> it drops h_img and h_oth. */
int ehm_gcn_set_uncond_mode(ehm_gcn* h, int masks_whole_condition);
/* Exact pass pruning (from egohmr.py:239-254): an item whose 24 joints are ALL visible takes every output entry from the
 * conditional pass, so its second pass is dead work.  mask_items [num_masked] int32 = the items that still need it (ascending),
 * mask_slot [B] int32 = each item's index in that list or -1; DEVICE arrays that must stay alive while the map is set.  From then
 * on, with passes == 2, the activation matrices hold (B + num_masked) * 24 rows: rows [0, B*24) the conditional pass, then the second
 * pass of mask_items[0], mask_items[1], ...  num_masked < 0 clears the map (every item has a second pass: B * 2 * 24 rows). */
int ehm_gcn_set_pass_map(ehm_gcn* h, const int32_t* mask_items, const int32_t* mask_slot, int num_masked);
/* The optional non-local block behind the last hidden conv (ModulatedGCN(nonlocal_layer=True), modulated_gcn.py:104-110;
 * nets/non_local_embedded_gaussian.py:60-85) for the ONE-CALL sampling loop (ehm_sample_loop): two 1x1-conv GEMMs in the operand format
 * of ehm_conv_nhwc_split - Wqkv = [theta | phi | g] as [3*Ci (padded to 128), hid], Wo = W.0 with BatchNorm(eval) folded as [hid, Ci] -
 * with their biases and power-of-two scales, and ehm_nonlocal_attention between them.  The arrays must stay alive while set;
 * NULL removes the block.  ehm_sample_desc.nonlocal_ci must carry Ci (it sizes the workspace). */
typedef struct {
  const void* Wqkv; const float* bqkv; float qkv_scale;
  const void* Wo; const float* bo; float o_scale;
  int Ci;
} ehm_nonlocal_params;
int ehm_gcn_set_nonlocal(ehm_gcn* h, const ehm_nonlocal_params* p);
int ehm_gcn_input_layer(ehm_gcn* h, const float* h_img, const float* h_oth, const uint8_t* vis, const float* x,
                        const float* Wx, const float* tvec, float* out, int B, int passes, void* stream);
/* The same conv in its general form (modulated_gcn_conv.py:39-50 + the BatchNorm / ReLU of modulated_gcn.py:21-28) for an ARBITRARY input feature -
 * ModulatedGCN.forward called on its own (modulated_gcn.py:99-116), where nothing is hoisted: the caller hands over the two GEMM results
 *   pre [bodies*24][2][hid] float32,  pre[r][k][:] = x[r, :] @ W[k]      (one ehm_conv_nhwc_split call with H = W = 1 on the weights [W[0] | W[1]])
 * and this call applies the modulation M, the adjacency mix, bias, BatchNorm(eval), ReLU and writes out [rows_pad, hid] in the handle's activation format. */
int ehm_gcn_input_layer_rows(ehm_gcn* h, const float* pre, float* out, int bodies, void* stream);

/* _GraphConv hid->hid (modulated_gcn.py:21-28): out = ReLU(BN(mix(X W0, X W1))) [+ residual,
 * modulated_gcn.py:42].  X, out, residual [rows_pad,hid]; residual may be NULL. */
int ehm_gcn_hidden_layer(ehm_gcn* h, int layer, const float* X, const float* residual, float* out,
                         int64_t rows_pad, void* stream);

/* All hidden convs of one ModulatedGCN.forward (the `for i in range(self.num_layers): out = self.gconv_layers[i](out)` loop,
 * modulated_gcn.py:108-109; each _ResGraphConv = two _GraphConv + residual, :31-43).  bufs[0] holds the input conv's output,
 * bufs[1] and bufs[2] are scratch of the same size; *result_index says which buffer holds the result (0 or 2).  With the
 * f16 operands (modes 1, 2) this is ONE chained launch (per-row-tile counters instead of kernel boundaries); otherwise it
 * loops over ehm_gcn_hidden_layer with the same buffer rotation.  Env EHM_F16_CHAIN=0 forces the loop. */
int ehm_gcn_hidden_stack(ehm_gcn* h, float* const bufs[3], int64_t rows_pad, int* result_index, void* stream);
/* Synchronises the stream and reports (and clears) the handle's status word: whether ANY chained launch since the previous status call flagged a
 * timed-out producer wait or an unproduced tile (never expected; the kernel gives up instead of hanging the device, and audits its own completion):
 * -5 (EIO), the results computed since the previous call are invalid; or whether an activation of the input / hidden convs reached the f16 range
 * (|x| >= 65504) in an X2 / f16 store and was clamped: -34 (ERANGE) - finite results that are not parity grade; that checkpoint needs
 * ehm_gcn_set_precision(h, 0).  0 = fine.  (The reference's float32 activations have no such limit: modulated_gcn.py:99-116.)  The guard covers the
 * rows the handle's last ehm_gcn_input_layer / _rows / ehm_gcn_pack_activations_checked call produced; the tile padding behind them is don't-care. */
int ehm_gcn_stack_status(ehm_gcn* h, void* stream);
/* The same word copied to *host_flag (pinned host memory owned by the caller) in stream order WITHOUT synchronising: a pipeline that
 * keeps batches in flight looks at *host_flag once the stream has passed this point (an event), and calls ehm_gcn_stack_status to
 * report and clear when it is non-zero (bit 0: chain failure, bit 2: saturation).  The flag is sticky on the device, so nothing is lost by looking late. */
int ehm_gcn_stack_status_async(ehm_gcn* h, uint32_t* host_flag, void* stream);

/* gconv_output (modulated_gcn.py:113) + the visibility fuse of egohmr.py:247-256:
 *   x0[b, j*6+c] = vis[b,j] ? out_cond[b,j,c] : out_uncond[b,j,c]      (passes == 2)
 *   x0 = out_cond                                                      (passes == 1)
 * X [rows_pad,hid] -> x0 [B,144]. */
int ehm_gcn_output_layer(ehm_gcn* h, const float* X, const uint8_t* vis, float* x0, int B, int passes,
                         void* stream);
/* The same with classifier-free guidance scales on the two passes (egohmr.py:248-249 with its `guidance_param` a knob, per joint class):
 *   x0[b, j*6+c] = u + s (c - u),  c = out_cond[b,j,c], u = out_uncond[b,j,c],  s = vis[b,j] ? scale_visible : scale_invisible      (passes == 2)
 *   x0 = out_cond                                                                                                                   (passes == 1)
 * as float32 sub, mul, add with one rounding each; s == 1 takes c and s == 0 takes u unchanged, so (1, 0) gives ehm_gcn_output_layer's bits.
 * An item the pass map prunes (ehm_gcn_set_pass_map: slot < 0) takes c on every joint: the caller's map must keep every item that has a joint
 * with s != 1 (ehm_item_prep_desc.need_all when scale_visible != 1).  Non-finite scales are refused. */
int ehm_gcn_output_layer_cfg(ehm_gcn* h, const float* X, const uint8_t* vis, float* x0, int B, int passes, float scale_visible,
                             float scale_invisible, void* stream);
/* The visibility fuse of ehm_sample_loop's steps (both launch routes), a setting of the handle like the pass map it goes with: the loop reads it at
 * entry with the rest of the handle's settings.  cfg = 0 (the handle's default) = the select x0 = vis ? c : u, the scales are not read; cfg = 1 =
 * x0 = u + s (c - u) as ehm_gcn_output_layer_cfg computes it ((1, 0) gives cfg = 0's bits; a loop of passes == 1 takes c).  ehm_sample_desc
 * carries no such fields: its layout is pinned.  ehm_gcn_output_layer / _cfg do not look at this setting. */
int ehm_gcn_set_fuse_scales(ehm_gcn* h, int cfg, float scale_visible, float scale_invisible);

/* ------------------------------------------------------------------ Modulated-GCN denoiser: backward ---- */
/* First derivatives of one graph conv in eval mode (frozen BatchNorm statistics) - modulated_gcn_conv.py:39-50, modulated_gcn.py:21-28, :38-42 -
 * for ModulatedGCN.forward's autograd route (modulated_gcn.py:99-116).  A conv is addressed as the handle holds it: EHM_GCN_CONV_INPUT, the index of
 * a hidden conv (0 .. num_hidden-1) or EHM_GCN_CONV_OUTPUT; N = its out_dim (hid_dim, 6 for the output conv), rows = bodies*24.
 * With h_k = X W_k, u_k = M (.) h_k, A = sym(adj + adj2), c = bn_weight / sqrt(bn_var + eps), z[j] = A_jj u0[j] + sum_{i != j} A_ji u1[i] + bias,
 * v = c (z - bn_mean) + bn_bias, y = relu(v) (output conv: y = z), out = y (+ residual) and g = dL/dout [rows, N]:
 *   vbar = g (.) [y > 0]  (output conv: zbar = g),  zbar = c vbar,  h0bar[j] = M_j A_jj zbar[j],  h1bar[i] = M_i sum_{j != i} A_ji zbar[j].
 * The gradient of the residual is g itself.  The GEMMs of the conv's backward are ehm_conv_nhwc_split calls (H = W = 1) of the caller:
 *   Xbar = G [W0; W1]^T,   [W0bar | W1bar] = X^T G  (G^T packed with ehm_split_pack as the weight operand),   pre = X [W0 | W1] for ehm_gcn_bwd_params.
 * The backward entries read the parameter arrays ehm_gcn_create was given (M, adj2, bias, bn_*) and adj: they must be alive and unchanged since then.
 * No allocation, no host synchronisation, no atomics. */
#define EHM_GCN_CONV_INPUT (-1)
#define EHM_GCN_CONV_OUTPUT (-2)
/* Backward of the ReLU, BatchNorm1d(eval), bias, adjacency mix and modulation (modulated_gcn.py:21-28, :42; modulated_gcn_conv.py:43-50) down to the two
 * branch responses.  G [rows, ldg] (ldg >= 2N): columns [0, N) = h0bar, [N, 2N) = h1bar; columns past 2N are left alone.
 * gate [rows, N] = the conv's activation y BEFORE the residual add as the forward produced it (only its sign is read); NULL for the output conv, and
 * only for it (-22 otherwise). */
int ehm_gcn_bwd_epilogue(const ehm_gcn* h, int conv, const float* gout, const float* gate, float* G, int ldg, int bodies, void* stream);
/* The gradients of M, adj2, bias (modulated_gcn_conv.py:16-37, used at :43-50) and of the BatchNorm affine (modulated_gcn.py:23): the parameter
 * gradients that are not GEMMs, summed over bodies and joints in a fixed order (two calls on the same inputs give the same bits):
 *   gM [24,N] = sum_b (u0bar h0 + u1bar h1),  gadj2 [24,24] = (Abar + Abar^T)/2 with Abar_jj = sum zbar[j] u0[j], Abar_ji = sum zbar[j] u1[i],
 *   gbias [N] = sum zbar,  gbn_bias [N] = sum vbar,  gbn_weight [N] = sum vbar (z - bn_mean) / sqrt(bn_var + eps)   (both NULL for the output conv).
 * pre [rows][ld_pre] float32 (ld_pre >= 2N): columns [0, N) = X W0, [N, 2N) = X W1, the layout ehm_gcn_input_layer_rows reads.
 * workspace: at least *bytes of ehm_gcn_bwd_params_workspace_bytes(h, conv, bodies, &bytes), 4-byte aligned. */
int ehm_gcn_bwd_params_workspace_bytes(const ehm_gcn* h, int conv, int bodies, int64_t* bytes);
int ehm_gcn_bwd_params(const ehm_gcn* h, int conv, const float* gout, const float* gate, const float* pre, int ld_pre, int bodies,
                       float* gM, float* gadj2, float* gbias, float* gbn_weight, float* gbn_bias, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------ Modulated-GCN denoiser: train-mode BatchNorm ---- */
/* One BatchNorm'd graph conv (EHM_GCN_CONV_INPUT or a hidden conv's index; EHM_GCN_CONV_OUTPUT has no BatchNorm: -22) with nn.BatchNorm1d in training
 * mode (modulated_gcn.py:21-28 under self.training), for ModulatedGCN.train_batchnorm.  R = rows = bodies*24, N = hid_dim, everything float32 [rows, N]:
 *   z[j] = A_jj M_j h0[j] + sum_{i != j} A_ji M_i h1[i] + bias,  mean = sum z / R,  var = sum (z - mean)^2 / R,  invstd = 1 / sqrt(var + eps),
 *   xhat = (z - mean) invstd,  y = relu(bn_weight xhat + bn_bias),  out = y (+ residual),
 * and with g = dL/dout:  vbar = g (.) [y > 0],  betabar = sum vbar,  gammabar = sum vbar xhat,
 *   zbar = bn_weight invstd (vbar - betabar / R - xhat gammabar / R),
 * after which the conv's backward is that of a conv without BatchNorm and ReLU on the cotangent zbar (ehm_gcn_train_bwd_*), with the same three caller-side
 * GEMMs as above.  bias has a zero gradient (the batch mean removes it).  The entries read the raw parameter arrays ehm_gcn_create was given (M, adj2, bias,
 * bn_weight, bn_bias) and adj, never the handle's BatchNorm-folded tables, and neither bn_mean nor bn_var.  All sums run in float64 in a fixed order: two calls
 * on the same inputs give the same bits.  No allocation, no host synchronisation, no atomics.  NULL handle or a bad conv: -22 before any device call.
 * workspace of ehm_gcn_train_preact / _stats / _bn_backward: at least *bytes of ehm_gcn_train_workspace_bytes, 16-byte aligned.
 * A [24 x 24]: the conv's symmetrised adjacency (adj + adj2 on the diagonal), written by ehm_gcn_train_adjacency once per conv and call and read by
 * ehm_gcn_train_preact and the two ehm_gcn_train_bwd_* entries. */
int ehm_gcn_train_workspace_bytes(const ehm_gcn* h, int conv, int bodies, int64_t* bytes);
int ehm_gcn_train_adjacency(const ehm_gcn* h, int conv, float* A, void* stream);
/* pre [rows][ld_pre] = X [W0 | W1] (the layout ehm_gcn_input_layer_rows reads) -> z, and the partial column sums of z in the workspace (for a following
 * ehm_gcn_train_stats with have_sums = 1 on the same workspace). */
int ehm_gcn_train_preact(const ehm_gcn* h, int conv, const float* pre, int ld_pre, int bodies, const float* A, float* z, void* workspace,
                         int64_t workspace_bytes, void* stream);
/* Batch statistics of z, two-pass in float64: mean [N], invstd [N] = 1 / sqrt(biased var + eps), and - unless both are NULL - the in-place updates
 * running_mean <- (1 - momentum) running_mean + momentum mean,  running_var <- (1 - momentum) running_var + momentum var R / (R - 1).
 * have_sums: 1 = the workspace holds ehm_gcn_train_preact's column sums of this z; 0 = they are computed here (one more pass over z). */
int ehm_gcn_train_stats(const ehm_gcn* h, int conv, const float* z, int bodies, int have_sums, double eps, double momentum, float* mean, float* invstd,
                        float* running_mean, float* running_var, void* workspace, int64_t workspace_bytes, void* stream);
/* y = relu(bn_weight xhat + bn_bias) (the gate of the backward; may be NULL) and out = y + residual (out may be NULL without a residual).  16-byte
 * aligned arrays. */
int ehm_gcn_train_normalize(const ehm_gcn* h, int conv, const float* z, const float* mean, const float* invstd, const float* residual, float* y,
                            float* out, int bodies, void* stream);
/* gbn_bias [N] = betabar, gbn_weight [N] = gammabar (either may be NULL) and zbar [rows, N].  gate: y of the forward (only its sign is read).  16-byte
 * aligned arrays. */
int ehm_gcn_train_bn_backward(const ehm_gcn* h, int conv, const float* gout, const float* gate, const float* z, const float* mean, const float* invstd,
                              int bodies, float* zbar, float* gbn_weight, float* gbn_bias, void* workspace, int64_t workspace_bytes, void* stream);
/* ehm_gcn_bwd_epilogue / ehm_gcn_bwd_params for a train-mode conv: zbar -> G [rows, ldg] = [h0bar | h1bar], and gM [24,N], gadj2 [24,24].
 * workspace: *bytes of ehm_gcn_train_bwd_params_workspace_bytes, 4-byte aligned. */
int ehm_gcn_train_bwd_epilogue(const ehm_gcn* h, int conv, const float* zbar, const float* A, float* G, int ldg, int bodies, void* stream);
int ehm_gcn_train_bwd_params_workspace_bytes(const ehm_gcn* h, int conv, int bodies, int64_t* bytes);
int ehm_gcn_train_bwd_params(const ehm_gcn* h, int conv, const float* zbar, const float* A, const float* pre, int ld_pre, int bodies, float* gM,
                             float* gadj2, void* workspace, int64_t workspace_bytes, void* stream);
/* Data parallel: the batch's rows are spread over `world` ranks (at most 64), rank r holds R_r = 24 bodies_r of them.  Each rank runs the passes above on
 * its own rows and stops at local [2][N] float64 ON THE DEVICE; the caller all-gathers them into gathered [world][2][N] (ONE collective per BatchNorm each
 * way) and every rank merges that buffer in rank order: all ranks get the same bits.  rows [world] int64 ON THE HOST: every R_r (>= 24, a multiple of 24;
 * together >= 2 rows).  A local + merge pair and the one-call entry share one body (the same passes, one write-out kernel, one reduce kernel), cut at the
 * collective: with world == 1 the pair writes the bits of ehm_gcn_train_stats / ehm_gcn_train_bn_backward by construction.
 *   stats_local: local = (mu_r, M2_r = sum (z - mu_r)^2), two-pass; have_sums as above; no running-statistic update.
 *   stats_merge: R = sum R_r,  mu = mu_0 + sum R_r (mu_r - mu_0) / R,  M2 = sum M2_r + sum R_r (mu_r - mu)^2  (Chan et al.; nothing cancels when the
 *                ranks' means lie many sigma apart),  var = M2 / R -> mean, invstd and the running update with the GLOBAL R (unbiased by R / (R - 1)).
 *   bwd_local:   local = (sum vbar, sum vbar xhat) with the MERGED mean / invstd.
 *   bwd_merge:   the ranks' sums added in rank order -> zbar with the global R.  gbn_bias / gbn_weight (either may be NULL) receive rank `rank`'s OWN sums
 *                (float32 of gathered[rank]): summed over the ranks by the caller's gradient all-reduce they are betabar / gammabar.  rows[rank] must be
 *                24 bodies. */
int ehm_gcn_train_stats_local(const ehm_gcn* h, int conv, const float* z, int bodies, int have_sums, double* local, void* workspace,
                              int64_t workspace_bytes, void* stream);
int ehm_gcn_train_stats_merge(const ehm_gcn* h, int conv, const double* gathered, const int64_t* rows, int world, double eps, double momentum, float* mean,
                              float* invstd, float* running_mean, float* running_var, void* stream);
int ehm_gcn_train_bwd_local(const ehm_gcn* h, int conv, const float* gout, const float* gate, const float* z, const float* mean, const float* invstd,
                            int bodies, double* local, void* workspace, int64_t workspace_bytes, void* stream);
int ehm_gcn_train_bwd_merge(const ehm_gcn* h, int conv, const double* gathered, const int64_t* rows, int world, int rank, const float* gout,
                            const float* gate, const float* z, const float* mean, const float* invstd, int bodies, float* zbar, float* gbn_weight,
                            float* gbn_bias, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ scene PointNet (conditioning) ----------- */
/* Building blocks of ResnetPointnet.forward (models/respointnet.py:33-59, ResnetBlockFC :89-97) on the split-f16
 * matrix-core path (f32-grade, see ehm_gcn_set_precision mode 1).  All activation / weight operands are in the "X2"
 * split format (ehm_split_pack); the host side (egohmr_amd/encoders.py) chains them, see csrc/linear.hip. */
typedef struct {
  const void* A0;          /* X2 [M, K0]                                                           */
  const void* A1;          /* X2 [M, K1] or NULL: second K segment (dual-source A operand)          */
  const void* W;           /* X2 [N, K0+K1], values pre-multiplied by w_scale (ehm_split_pack)      */
  const float* bias;       /* [N] or NULL                                                           */
  const float* group_bias; /* [M/rows_per_group, N] or NULL: per-body bias (pooled half of a block) */
  void* Y;                 /* X2 [M, N] or NULL                                                     */
  float* colmax;           /* [M/rows_per_group, N] or NULL: running max over the group's valid rows
                              (caller initialises to -inf); fused torch.max(dim=1), respointnet.py:38 */
  int64_t M;               /* rows, multiple of 192 (the row tile)                                  */
  int N, K0, K1;           /* N multiple of 128; K0, K1 multiples of 32, K0 + K1 >= 64              */
  int rows_per_group;      /* padded points per body, multiple of 192                               */
  int valid_rows_per_group;/* real points per body, <= rows_per_group (a larger value is refused); 0 = all */
  int relu_in0;            /* apply ReLU to A0 on load (ResnetBlockFC's actvn before fc_0); needs K1 == 0 (else refused) */
  int relu_out;            /* apply ReLU before storing                                             */
  float w_scale;           /* the power-of-two scale baked into W                                   */
  const float* lift_points;/* NULL, or [M/rows_per_group, valid_rows_per_group, 3] float32: A0 is not read but generated on
                              the fly as relu(points . Wpos^T + bpos), K0 wide - fc_pos + the first block's actvn
                              (respointnet.py:35,:90) folded into the loader; then A0 == NULL, K1 == 0, relu_in0 == 0 */
  const float* lift_W4;    /* [K0][4] float32 rows (w_x, w_y, w_z, bias) of fc_pos                   */
  int hi_only;             /* 1 = the plain-f16 tier (NOT parity grade): hi halves of A0 / A1 / W only, hi halves of Y only; 0 = split-f16 (f32 grade) */
  int group_bias_stride;   /* floats between the rows of group_bias; 0 = N (dense).  Lets two blocks' per-body vectors come out of one small GEMM */
} ehm_linear_desc;
int ehm_linear_split(const ehm_linear_desc* d, void* stream);
/* float32 [rows,K] -> X2 [rows,K_padded] (zero padded), values multiplied by `scale` (1 for activations). */
int ehm_split_pack(const float* X, void* X2, int64_t rows, int K, int K_padded, float scale, void* stream);
/* The raw points zero-padded to 32 columns, P32 X2 [B*N_padded, 32] (input of the folded block_0 shortcut), and - when R0 is not
 * NULL - fc_pos + ReLU (respointnet.py:35,:90): pts [B,N,3] -> R0 = relu(pts W^T + b) as X2 [B*N_padded, C].  (The PointNet
 * generates R0 inside its first GEMM instead: ehm_linear_desc.lift_points; R0 here serves tests and other callers.) */
int ehm_pointnet_lift(const float* pts, const float* Wpos, const float* bpos, void* R0, void* P32, int B, int N, int N_padded,
                      int C, void* stream);

/* ------------------------------------------------------------------ scene PointNet: backward ---- */
/* First derivatives of ResnetPointnet (models/respointnet.py:33-97) around the GEMMs, which are ehm_conv_nhwc_split calls (H = W = 1) of the caller
 * (egohmr_amd/pointnet_grad.py), and the weight gradients, which are ehm_pointnet_bwd_wgrad.  Per block, x = cat[net, pooled] (block 0: x = net0 = fc_pos(p)), h = fc_0(relu(x)), net' = fc_1(relu(h)) + shortcut(x),
 * pooled' = max over a body's N points; with G = gnet' + one-hot(arg) gpool':  dh = (G W1) (.) [relu(h) > 0],  dx = (dh W0) (.) [x > 0] + G S.
 * Every matrix is [B * N_padded, C] row-major, N_padded a multiple of 192 (the row tile of ehm_linear_split), C a multiple of 128, 16-byte aligned;
 * rows >= N of a body are padding: never a candidate or a summand, written as exact zeros.  "X2" is the split format ehm_linear_split writes.
 * No allocation, no host synchronisation, no atomics: column sums are fixed-order reductions (two calls on the same inputs give the same bits) through
 * `workspace`, at least *bytes of ehm_pointnet_bwd_workspace_bytes(B, N_padded, C, &bytes), 16-byte aligned. */
int ehm_pointnet_bwd_workspace_bytes(int B, int N_padded, int C, int64_t* bytes);
/* arg [B,C] int32: the lowest row i < N of body b that maximises net[b * N_padded + i, c]; a NaN counts as the maximum (torch.max propagates it).
 * x2: 1 = net is X2, 0 = float32.  One pass over net. */
int ehm_pointnet_pool_argmax(const void* net, int x2, int32_t* arg, int B, int N, int N_padded, int C, void* workspace, int64_t workspace_bytes,
                             void* stream);
/* G[b * N_padded + i, c] = gnet[.] (0 when gnet is NULL) + (arg[b,c] == i ? gpool[b,c] : 0), and - each may be NULL - gsum [C] = the column sums of G,
 * gsum_group [B,C] = those of each body.  workspace may be NULL when both are. */
int ehm_pointnet_bwd_scatter(const float* gnet, const float* gpool, const int32_t* arg, float* G, float* gsum, float* gsum_group, int B, int N,
                             int N_padded, int C, void* workspace, int64_t workspace_bytes, void* stream);
/* out = (*t_scale) T (.) [act > 0] + (*add_scale) add, with `add` optional, the two factors device scalars (NULL = 1) and act X2 (act_x2 = 1) or
 * float32 (0); out may be T.  sum [C], sum_group [B,C]: the column sums of out, as above. */
int ehm_pointnet_bwd_gate(const float* T, const void* act, int act_x2, const float* add, const float* t_scale, const float* add_scale, float* out,
                          float* sum, float* sum_group, int B, int N, int N_padded, int C, void* workspace, int64_t workspace_bytes, void* stream);
/* net0 = pts Wpos^T + bpos (respointnet.py:35) and relu(net0) as float32 [B * N_padded, C] (either may be NULL), with the arithmetic of
 * ehm_linear_desc.lift_points, so that relu_net0 > 0 is the forward's own gate.  pts [B,N,3], Wpos [C,3], bpos [C]. */
int ehm_pointnet_bwd_net0(const float* pts, const float* Wpos, const float* bpos, float* net0, float* relu_net0, int B, int N, int N_padded, int C,
                          void* stream);
/* gW [C,3] = X^T pts, gb [C] = the column sums of X, gp [B,N,3] = X Wpos (each may be NULL, not all; gp needs Wpos [C,3]).  With X = net0bar these are
 * the gradients of fc_pos_0.weight, fc_pos_0.bias and the points; with X = G, gW is the K = 3 factor of block_0.shortcut's weight gradient. */
int ehm_pointnet_bwd_lift(const float* X, const float* pts, const float* Wpos, float* gW, float* gb, float* gp, int B, int N, int N_padded, int C,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* A weight gradient: out[g * ld_out + a] = sum over the valid rows m of P[m, g] act(Q[m, a]) - P float32 [B * N_padded, Cg] (a cotangent: G or dh),
 * Q [B * N_padded, Ca] X2 (q_x2 = 1) or float32 (0), act = ReLU when q_relu = 1; ld_out >= Ca, so a half of a wider matrix can be written in place
 * (the other columns are left alone).  Exact float32 products on the matrix cores straight from the row-major operands (the contraction runs over the
 * rows: no transpose, no packing), split over at most 256 runs of rows whose partial tiles are added in index order: fixed-order, no atomics.
 * workspace: *bytes of ehm_pointnet_bwd_wgrad_workspace_bytes(B, N_padded, Cg, Ca, &bytes), 16-byte aligned. */
int ehm_pointnet_bwd_wgrad_workspace_bytes(int B, int N_padded, int Cg, int Ca, int64_t* bytes);
int ehm_pointnet_bwd_wgrad(const float* P, const void* Q, int q_x2, int q_relu, float* out, int ld_out, int B, int N, int N_padded, int Cg, int Ca,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* Y[M,N] = act(X[M,K] . W[K,N] + bias[N]) in exact float32 on the matrix cores, for short M (batches of feature vectors): the
 * step-invariant slices of the input graph conv (models/egohmr/modulated_gcn/modulated_gcn_conv.py:39-50 on the image / scene
 * features) and the beta head's first layer (models/egohmr/egohmr.py:263-265, fc_head_beta).  K % 32 == 0, N % 32 == 0, any M;
 * X 16-byte aligned; bias may be NULL.  relu: bit 0 applies max(., 0) to the output; relu >> 1 = number of leading output columns (a multiple of 32:
 * other counts are refused) whose INPUT row is rectified first - [relu(x) . Wa | x . Wb] in one launch (the pooled halves of a ResnetBlockFC's fc_0 and shortcut,
 * models/respointnet.py:41-51).  Deterministic (no atomics). */
int ehm_skinny_gemm_f32(const float* X, const float* W, const float* bias, float* Y, int M, int K, int N, int relu, void* stream);


/* ResNet-50 stem in one pass (torchvision ResNet.forward conv1 / bn1 / relu / maxpool, models/resnet.py:139-150 as used at
 * models/egohmr/egohmr.py:183): conv 7x7 stride 2 pad 3 (3 -> 64) + bias + ReLU + max-pool 3x3 stride 2 pad 1.
 *   img [N,3,H,W] float32 (NCHW), H % 32 == 0, W % 32 == 0;   y [N,H/4,W/4,64] float32 (NHWC)
 *   Wt [147][64]: the BatchNorm-folded weights transposed, row k = (ci*7 + kh)*7 + kw;   bias [64]
 *   scratch: ehm_resnet_stem_scratch_bytes(N,H,W) bytes of device memory (zero-padded copy of the image)
 *   out_x2 != 0: y is written in the X2 split format instead (same byte size; the input format of ehm_conv_x2) */
size_t ehm_resnet_stem_scratch_bytes(int N, int H, int W);
int ehm_resnet_stem(const float* img, const float* Wt, const float* bias, float* scratch, float* y, int N, int H, int W,
                    int out_x2, void* stream);

/* ------------------------------------------------------------------ ResNet-50 trunk: backward (eval-mode BatchNorm, folded) ---- */
/* First derivatives of the folded trunk around its data-gradient convolutions, which are ehm_conv_nhwc_split calls of the caller
 * (egohmr_amd/trunk_grad.py).  Per conv y = relu(conv(x, w') + b' (+ res)), g = dL/dy:  G = g (.) [y > 0],  b'bar = sum_p G,
 * w'bar[co,kh,kw,ci] = sum_p G[p,co] x[tap(p),ci].  "X2" is the split format ehm_conv_x2 / ehm_resnet_stem write (rows of ehm_conv_x2_rows).
 * No allocation, no host synchronisation, no atomics: every sum over pixels is a fixed-order reduction (two calls on the same inputs give the same bits).
 *
 * out[n,h,w,c] = *scale * g * [y > 0] as float32 NHWC.  y_x2: the conv's saved X2 output [N*Ho*Wo rows, C] (only its sign is used; a NaN in g behind
 * a closed gate does not pass).  g: [N,Ho,Wo,C] float32, or with g_per_image [N,C] read as g[n,c] / (Ho*Wo) (the average pool).  (H, W) == (Ho, Wo):
 * dense.  Otherwise (H-1)/2+1 == Ho and (W-1)/2+1 == Wo: zero-dilated - the value of (ho, wo) at (2 ho, 2 wo), zeros elsewhere - so that the data
 * gradient of a stride-2 conv is a stride-1 conv.  scale: a float on the DEVICE, or NULL for 1.  C % 32 == 0, 16-byte aligned pointers. */
int ehm_conv_bwd_gate(const float* g, int g_per_image, const void* y_x2, const float* scale, float* out, int N, int Ho, int Wo, int C, int H, int W,
                      void* stream);
/* gw [Co][K*K*Ci] (tap-major, like the forward's packed weights) = sum over the output pixels of G[p,co] x[tap(p),ci] and gbias [Co] = sum_p G[p,co]
 * (either may be NULL, not both).  G float32 [N,Ho,Wo,Co] (dense), x_x2 the conv's saved X2 input [x_rows >= N*H*W, Ci]; K in {1, 3}, stride in {1, 2},
 * any pad (a tap outside the image counts as zero and is never loaded); Ci % 64 == 0, Co % 64 == 0.  Exact float32 products on the matrix cores
 * (v_mfma_f32_32x32x2_f32 with k = the pixel), split over at most 256 runs of pixels whose partial tiles are added in index order.
 * workspace: *bytes of ehm_conv_bwd_wgrad_workspace_bytes, 16-byte aligned. */
int ehm_conv_bwd_wgrad_workspace_bytes(int N, int H, int W, int Ci, int Co, int K, int stride, int pad, int64_t* bytes);
int ehm_conv_bwd_wgrad(const float* G, const void* x_x2, int64_t x_rows, float* gw, float* gbias, int N, int H, int W, int Ci, int Co, int K, int stride,
                       int pad, void* workspace, int64_t workspace_bytes, void* stream);
/* Weight and bias gradient of the stem (ehm_resnet_stem): gW [64][147] (k = (ci*7 + kh)*7 + kw), gb [64] (either may be NULL, not both) from
 * gpool [N,H/4,W/4,64] float32, the cotangent of the pooled output ALREADY gated by [pooled > 0].  The 7x7 / 2 pre-pool activation is recomputed in
 * float32 per chunk of images into the workspace and the pooled cotangent routed by gather: a pre-pool pixel takes the cotangent of each of the (at
 * most four) 3x3 / 2 windows whose arg-max it is (lowest row-major index among equals, NaN = maximum).  z_out / gz_out: optional [N,H/2,W/2,64]
 * float32 copies of the pre-pool activation and of its cotangent (tests).  img [N,3,H,W], Wt [147][64], bias [64] as for ehm_resnet_stem. */
int ehm_resnet_stem_backward_workspace_bytes(int N, int H, int W, int64_t* bytes);
int ehm_resnet_stem_backward(const float* img, const float* Wt, const float* bias, const float* gpool, float* gW, float* gb, float* z_out, float* gz_out,
                             int N, int H, int W, void* workspace, int64_t workspace_bytes, void* stream);
/* The three steps of ehm_resnet_stem_backward on their own, on whole-batch tensors (the train-mode BatchNorm route needs sums over all pre-pool pixels
 * between them): z [N,H/2,W/2,64] = conv 7x7 / 2 / pad 3 of img + bias in float32;  gz = gpool routed to each window's arg-max of z (z != gz);
 * gW [64][147], gb [64] (either may be NULL, not both) = sum over the pre-pool pixels of gz (x) the image taps, workspace: 256 * 148 * 64 floats. */
int ehm_resnet_stem_preact(const float* img, const float* Wt, const float* bias, float* z, int N, int H, int W, void* stream);
int ehm_resnet_stem_route(const float* z, const float* gpool, float* gz, int N, int H, int W, void* stream);
int ehm_resnet_stem_wgrad(const float* img, const float* gz, float* gW, float* gb, int N, int H, int W, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* ------------------------------------------------------------------ ResNet-50 trunk: train-mode BatchNorm2d (csrc/bn2d_train.hip) ---- */
/* z [pixels, C]: a conv's RAW output, as the X2 buffer ehm_conv_x2 wrote (z_is_x2 = 1; z_rows >= pixels rows, only the first `pixels` are read) or as
 * float32 rows (z_is_x2 = 0).  C % 32 == 0, pixels >= 2, 16-byte aligned pointers.  No allocation, no host synchronisation, no atomics: float64 partial
 * sums over runs of pixels that depend on the shape alone, added in index order.  workspace: *bytes of ehm_bn2d_train_workspace_bytes.
 *
 * stats: mean[c], var[c] (biased) and invstd[c] = 1 / sqrt(var + eps) as float32, from two passes in float64 (the mean, then the centred squares).
 * running_mean / running_var (may be NULL: left alone) <- (1 - momentum) old + momentum (mean | var pixels / (pixels - 1)); *num_batches_tracked
 * (int64 on the device, may be NULL) += 1 - nn.BatchNorm2d's update.
 * bwd_sums: gbeta[c] = sum_p G[p,c], ggamma[c] = sum_p G[p,c] (z[p,c] - mean[c]) invstd[c];  G float32 [pixels, C].
 * bwd_zbar: out[n,h,w,c] = *scale gamma invstd (G - gbeta / R - xhat ggamma / R), R = N Ho Wo, as float32 NHWC; dense ((H, W) == (Ho, Wo)) or
 * zero-dilated like ehm_conv_bwd_gate.  scale: a float on the DEVICE, or NULL for 1. */
int ehm_bn2d_train_workspace_bytes(int64_t pixels, int C, int64_t* bytes);
int ehm_bn2d_train_stats(const void* z, int z_is_x2, int64_t z_rows, int64_t pixels, int C, double eps, double momentum, float* mean, float* var,
                         float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, void* workspace, int64_t workspace_bytes,
                         void* stream);
int ehm_bn2d_train_bwd_sums(const float* G, const void* z, int z_is_x2, int64_t z_rows, int64_t pixels, int C, const float* mean, const float* invstd,
                            float* gbeta, float* ggamma, void* workspace, int64_t workspace_bytes, void* stream);
int ehm_bn2d_train_bwd_zbar(const float* G, const void* z, int z_is_x2, int64_t z_rows, const float* mean, const float* invstd, const float* gamma,
                            const float* gbeta, const float* ggamma, const float* scale, float* out, int N, int Ho, int Wo, int C, int H, int W,
                            void* stream);
/* Data parallel, as the ehm_gcn_train_*_local / _merge entries: local [2][C] float64 on the device, gathered [world][2][C], rows [world] int64 on the host
 * (each rank's pixel count R_r >= 1; together >= 2), world <= 64.  A rank's `pixels` may be 1 here; float32 rows need C % 8 == 0 only (X2: C % 32 == 0).
 * The workspace is that of ehm_bn2d_train_workspace_bytes(max(pixels, 2), C rounded up to 32).  A local + merge pair and the one-call entry share one body, cut at
 * the collective, and both zbar entries one checked launch: with world == 1, local + merge write the bits of ehm_bn2d_train_stats /
 * ehm_bn2d_train_bwd_sums, and zbar_rows with total_rows = N Ho Wo those of ehm_bn2d_train_bwd_zbar, by construction.
 *   stats_local: local = (mu_r, M2_r), two-pass, no running update.     stats_merge: Chan et al.'s merge in rank order -> mean, var, invstd; the running
 *   update and *num_batches_tracked += 1 with the GLOBAL R.             bwd_local: local = (sum G, sum G xhat) with the merged mean / invstd.
 *   bwd_merge: gbeta / ggamma = the ranks' sums added in rank order (for zbar_rows); gbeta_own / ggamma_own (either may be NULL) = float32 of rank `rank`'s
 *   own sums, the parameter gradients that the caller's gradient all-reduce completes.
 *   bwd_zbar_rows: ehm_bn2d_train_bwd_zbar with R = total_rows (all ranks' rows; >= 2 and >= N Ho Wo) instead of N Ho Wo. */
int ehm_bn2d_train_stats_local(const void* z, int z_is_x2, int64_t z_rows, int64_t pixels, int C, double* local, void* workspace, int64_t workspace_bytes,
                               void* stream);
int ehm_bn2d_train_stats_merge(const double* gathered, const int64_t* rows, int world, int C, double eps, double momentum, float* mean, float* var,
                               float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, void* stream);
int ehm_bn2d_train_bwd_local(const float* G, const void* z, int z_is_x2, int64_t z_rows, int64_t pixels, int C, const float* mean, const float* invstd,
                             double* local, void* workspace, int64_t workspace_bytes, void* stream);
int ehm_bn2d_train_bwd_merge(const double* gathered, int world, int rank, int C, float* gbeta, float* ggamma, float* gbeta_own, float* ggamma_own,
                             void* stream);
int ehm_bn2d_train_bwd_zbar_rows(const float* G, const void* z, int z_is_x2, int64_t z_rows, const float* mean, const float* invstd, const float* gamma,
                                 const float* gbeta, const float* ggamma, const float* scale, float* out, int N, int Ho, int Wo, int C, int H, int W,
                                 int64_t total_rows, void* stream);

/* NHWC convolution + bias (+ identity) + ReLU as an implicit GEMM on the f16 matrix cores with f32-grade accuracy (hi/lo split
 * operands, f32 accumulate): y[n,ho,wo,co] = act(sum x[n, ho*s-p+kh, wo*s-p+kw, ci] w[co,kh,kw,ci] + bias[co] (+ residual)).
 * Stands in for torchvision's Bottleneck conv1/conv2/conv3/downsample + BatchNorm(eval, folded by the caller) + ReLU of the
 * ResNet-50 backbone (models/egohmr/egohmr.py:183).
 *   x [N,H,W,Ci] float32, Ci % 32 == 0;   y [N,Ho,Wo,Co] float32, Co % 8 == 0;   residual NULL or like y;   bias NULL or [Co]
 *   W: the weights as [Co_pad][KH*KW*Ci] (tap-major: k = (kh*KW + kw)*Ci + ci), Co_pad = Co rounded up to 128 with zero rows,
 *      multiplied by w_scale (a power of two) and packed with ehm_split_pack(..., K, K, w_scale, ...);  KH*KW <= 32
 * Lengths: the kernel stages 128 weight rows per column tile whatever Co is, so W must hold all Co_pad rows; bias is read at [0, Co) - a caller
 *   whose true column count is no multiple of 8 passes Co rounded up to 8, zero weight rows behind the true ones and a bias of THAT length
 *   (split_gemm.pack_weight pads it): a padding column comes out as act(residual), or 0.  stride is 1 or 2, pad >= 0, and the kernel must fit the
 *   padded image (H + 2 pad >= KH, W + 2 pad >= KW); anything else is EHM_EINVAL before any device call.
 * Range: an activation is split in the kernel into hi = f16(clamp(x, +-65504)) and lo = f16(x - hi): |x| <= 65504 is represented to 2^-22 |x| + 2^-25
 *   (tests/conv_split_ref.py has the error bound the tests hold every output to).  A larger magnitude is outside the contract: lo carries the excess
 *   over 65504 at f16 precision only, and past the format's 131008 it is inf - such an activation acts like an inf one (below); there is no range
 *   flag.  Magnitudes below about 2^-14 lose their lo half to the f16 subnormal range: callers scale small operands up by a power of two first
 *   (split_gemm.pow2_scale).
 * Non-finite: a NaN or +-inf activation lands in its lo half and makes every output whose receptive field holds that pixel non-finite, in every
 *   channel (0 . inf of a zero weight included), and no other output; with relu = 1 the epilogue's max(v, 0) then returns 0 for a NaN or -inf, so
 *   a caller that must see the poison carries a flag beside the data.  An all-zero W on finite activations gives exactly act(bias + residual). */
typedef struct ehm_conv_desc {
  const float* x; const void* W; const float* bias; const float* residual; float* y;
  int N, H, Wd, Ci, Co;
  int KH, KW, stride, pad, relu;
  float w_scale;
} ehm_conv_desc;
int ehm_conv_nhwc_split(const ehm_conv_desc* d, void* stream);

/* The same convolution with the activations kept in the X2 split format between the layers (the ResNet-50 trunk of
 * models/resnet.py:139-150 / models/egohmr/egohmr.py:183 end to end): x, residual, y are X2 [rows, C] matrices (ehm_split_pack layout,
 * pixel-major NHWC) whose row count is ehm_conv_x2_rows(N*H*W) = pixels rounded up to the 192-row tile + ONE extra row; the LAST
 * row of x must be all zero (out-of-image taps read it).  Ci % 32 == 0, Co % 32 == 0, KH*KW*Ci >= 64; W, bias, relu, w_scale as
 * in ehm_conv_desc.  y's padding rows receive don't-care values; its last row is cleared by the call.
 * Pinned by tests/test_gpu_conv_x2.py (every valid output against float64 of the decoded operands, under the per-output bound derived in
 * tests/conv_x2_ref.py):
 *   rows: x may have MORE than ehm_conv_x2_rows(N*H*W) rows - the zero row is always row x_rows - 1.  The rows between the last pixel and the zero
 *   row (of x, x2 and residual) never reach a valid output: a row past the last output pixel gathers the zero row, and only y's own padding rows
 *   see the residual's.  No byte of y past column Co of a row, and none behind its last row, is written; hi_only leaves every lo half of y alone.
 *   range: activations and outputs up to +-65504 stay within the bound.  A FINITE output v past 65504 saturates (the epilogue converts with
 *   MODE.FP16_OVFL = 1): hi = +-65504, lo = f16(v -+ 65504) clamped to +-65504 - v itself to about 2^-11 of the part past 65504 up to +-131008,
 *   +-131008 beyond, never inf (hi_only: +-65504) - the halves ehm_split_pack writes for such a value.  An activation stored in that saturated form
 *   IS 131008 to the engine: there is no range flag in the data.
 *   non-finite: a NaN or +-inf half of an activation (hi, or lo in the split tier) makes every output whose receptive field holds that pixel
 *   non-finite, in every channel, and no other output: all others keep the bits of the clean launch.  With relu = 1 the epilogue's max(v, 0)
 *   returns 0 for a NaN or -inf, as in the float32-activation engine above.  The hi_only tier does not read lo halves at all.  (The K loop runs
 *   with MODE.FP16_OVFL clear: with the bit set the matrix cores do not propagate a non-finite half.)
 *   An all-zero W gives exactly the X2 split of act(bias + residual). */
typedef struct ehm_conv_x2_desc {
  const void* x; int64_t x_rows; const void* W; const float* bias; const void* residual; void* y;
  int N, H, Wd, Ci, Co;
  int KH, KW, stride, pad, relu;
  float w_scale;
  void* workspace;           /* ehm_conv_x2_workspace_bytes(d) bytes of device scratch, or NULL (then whole tiles only) */
  int64_t workspace_bytes;
  /* Optional second K segment (x2 != NULL): y = act( conv(x) + conv1x1_stride2(x2) + bias (+ residual) ) - a bottleneck's projection
   * shortcut accumulated inside its last convolution (torchvision Bottleneck.forward: out = bn3(conv3(.)) + downsample(x)), so that the
   * shortcut tensor never exists.  x2 is X2 [x2_rows, Ci2] over [N, H2, W2] pixels with its own zero row, (H2 - 1) / stride2 + 1 == Ho
   * (same for W); W then holds [Co_pad][KH*KW*Ci + Ci2] with the shortcut's weights behind the main ones (one common w_scale), bias
   * the SUM of the two folded biases; Co % 128 == 0. */
  const void* x2; int64_t x2_rows;
  int H2, W2, Ci2, stride2;
  int hi_only;               /* 0 = split-f16 arithmetic (f32 grade, the parity path).  1 = the plain-f16 tier (NOT parity grade): only the hi halves of x, W,
                                residual are read and only hi halves written - one MFMA per product, half the bytes; the lo halves of y are don't-care  */
  int workspace_clean;       /* 1 = the caller zeroed the first 4096 bytes of `workspace` once and nothing but ehm_conv_x2 has written to it since: the call
                                skips its memset node (every call leaves the arrival counters zeroed - or poisoned, after a hand-off time-out: then every later
                                stream-K conv on that workspace comes out as NaN until the caller zeroes it again).  0 = the call clears them itself */
} ehm_conv_x2_desc;
int64_t ehm_conv_x2_rows(int64_t pixels);
/* Scratch of the stream-K schedule: when a conv's tile count would leave a large share of the GPU's block slots idle in its last round
 * (ResNet-50 layers 3 / 4 at B = 256: 524 or 264 tiles on 512 slots), the tiles' K loops are dealt out to the blocks in equal runs and a tile
 * cut by a run boundary is finished by the block that started it (fixed summation order: deterministic).  0 = the conv runs whole tiles. */
int64_t ehm_conv_x2_workspace_bytes(const ehm_conv_x2_desc* d);
int ehm_conv_x2(const ehm_conv_x2_desc* d, void* stream);
/* Did a stream-K tile hand-off on `workspace` time out since the last call (a partner block did not deliver its partial sums within ~1 s: GPU shared,
 * preempted, under a profiler)?  Such a tile is written as NaN (through the ReLU as well), its arrival counter stays poisoned so that every later
 * stream-K conv on the workspace is NaN too, and the LAST word of the workspace's first 4096 bytes counts the time-outs (sticky on the device).
 *   host_flag != NULL : enqueue a stream-ordered copy of that count to *host_flag (pinned host memory) and return 0 - the asynchronous form;
 *   host_flag == NULL : wait for the stream, and when the count is non-zero zero the 4096 counter bytes again (the workspace is clean) and return -5 (EIO).
 * The torchvision convolution this replaces cannot fail (models/resnet.py:139-150); this is the hand-off protocol's own failure mode made loud. */
int ehm_conv_x2_workspace_status(void* workspace, uint32_t* host_flag, void* stream);
/* Y[g, c] = mean over the rows_per_group consecutive rows of group g of the X2 matrix X [groups*rows_per_group (+ padding), C]:
 * the global average pool behind the last bottleneck (models/resnet.py:148-149). */
int ehm_x2_group_mean(const void* X, float* Y, int groups, int rows_per_group, int C, int hi_only /* 1: X was written by a hi_only call */, void* stream);

/* Attention core of the optional non-local block of ModulatedGCN (nonlocal_layer=True, modulated_gcn.py:93-110;
 * nets/non_local_embedded_gaussian.py:68-79): per body, y = softmax(theta phi^T, dim=-1) g over the 24 joints.
 *   qkv [bodies*24, 3*Ci] float32 rows = [theta | phi | g] (one 1x1-conv GEMM, e.g. ehm_conv_nhwc_split with H = W = 1);
 *   y [bodies*24, Ci].  The W conv + BatchNorm + residual that follow are another ehm_conv_nhwc_split call. */
int ehm_nonlocal_attention(const float* qkv, float* y, int64_t bodies, int Ci, void* stream);
/* Its vector-Jacobian product (csrc/nonlocal_bwd.hip; nets/non_local_embedded_gaussian.py:68-79 - f = matmul(theta_x, phi_x), f_div_C = softmax(f, -1),
 * y = matmul(f_div_C, g_x) - on the joint axis, modulated_gcn.py:104-110):  qkv as above, gy [bodies*24, Ci] the cotangent of y ->
 * gqkv [bodies*24, 3*Ci] = [thetabar | phibar | gbar].  Per body P = softmax(theta phi^T) is recomputed with the max-subtraction (no saved probabilities),
 * Pbar = gy g^T, D_a = sum_b P_ab Pbar_ab, Fbar = P (.) (Pbar - D), thetabar = Fbar phi, phibar = Fbar^T theta, gbar = P^T gy.  One block per body, no
 * atomics, every sum in index order: two calls on the same inputs give the same bits.  Any Ci > 0; bodies in [1, 2^31). */
int ehm_nonlocal_attention_backward(const float* qkv, const float* gy, float* gqkv, int64_t bodies, int Ci, void* stream);
/* The block's tail for the autograd route (non_local_embedded_gaussian.py:81-82: W_y = self.W(y), z = W_y + x), BatchNorm2d unfolded:
 * out[r,c] = (u[r,c] - mean[c]) invstd[c] gamma[c] + beta[c] + res[r,c] on float32 rows [rows, C]; mean / invstd: the batch's (ehm_bn2d_train_stats) or the
 * running ones.  out may be res. */
int ehm_nonlocal_bn_residual(const float* u, const float* mean, const float* invstd, const float* gamma, const float* beta, const float* res,
                             float* out, int64_t rows, int C, void* stream);

/* ------------------------------------------------------------------ sampler steps ------------- */
/* diffusion/gaussian_diffusion.py:217-220 + :333-336 (p_sample) and :378-385 (p_sample_with_grad):
 *   mean = coef1*x0 + coef2*x  [+ grad_scale * grad]
 *   x_next = mean + nonzero * exp(0.5*log_variance) * noise
 * grad may be NULL.  All [B,144]; x_next may alias x. */
int ehm_ddpm_step(const float* x, const float* x0, const float* noise, const float* grad, float* x_next,
                  float coef1, float coef2, float log_variance, float nonzero, float grad_scale, int64_t n,
                  void* stream);
/* gaussian_diffusion.py:286-290 + :539-555 (ddim_sample):
 *   eps = (sqrt_recip_ac*x - x0) / sqrt_recipm1_ac
 *   x_next = x0*sqrt_ac_prev + dir_coef*eps + nonzero*sigma*noise,  dir_coef = sqrt(1-ac_prev-sigma^2) */
int ehm_ddim_step(const float* x, const float* x0, const float* noise, float* x_next, float sqrt_recip_ac,
                  float sqrt_recipm1_ac, float sqrt_ac_prev, float dir_coef, float sigma, float nonzero,
                  int64_t n, void* stream);

/* ------------------------------------------------------------------ collision guidance -------- */
/* Build-defined proxy for smpl.coap.collision_loss (egohmr.py:555; COAP is unavailable offline,
 * see DESIGN.md): with the bbox selection of egohmr.py:550-552,
 *   loss[b] = sum over scene points p inside bbox(verts[b]) of relu(tau - min_v |p - v|)^2
 * and gverts[b,v,:] = d(loss[b])/d(verts[b,v,:]).  scene [B,N,3] (already canonicalised,
 * egohmr.py:211); loss [B]; gverts [B,V,3] (overwritten).  V <= 13632 (the vertices live in
 * LDS): a larger V is refused with EINVAL before anything is allocated, launched or written. */
int ehm_collision_proxy(const float* verts, const float* scene, float* loss, float* gverts, int B, int V, int N,
                        float tau, void* stream);

/* The same proxy with the knobs of the reference's other call sites:
 *   all_points != 0   no bbox selection - the batched `volume.collision_loss(scene, smpl_output)` of the VolSMPL twin
 *                     (models/egohmr/egohmr_volsmpl.py:609-612); 0 = egohmr.py:550-552 as above
 *   hits [B] int32    (may be NULL) number of selected scene points closer than tau to the body: the count behind
 *                     EgoHMR.eval_coll (egohmr.py:487-514, `occupancy > 0.5`) / eval_coll_volsmpl (egohmr_volsmpl.py:548-579, `sdf < 0`)
 *   gverts            may be NULL (metric only) */
int ehm_collision_query(const float* verts, const float* scene, float* loss, float* gverts, int32_t* hits, int B, int V, int N,
                        float tau, int all_points, void* stream);

/* ---- mesh collision term (opt-in; EgoHMR.collision_proxy = 'mesh') ----
 * What COAP approximates is the occupancy of the posed SMPL mesh; a closed mesh gives it exactly.  Numbers from this term are the mesh's own
 * occupancy and depth, NOT outputs of COAP / VolumetricSMPL.  Per body b: verts[b] [V,3] float32, ONE faces [F,3] int32 for all bodies, wound so
 * that (v1 - v0) x (v2 - v0) points outwards (as SMPL's are), scene[b] [N,3].
 *   selection   all_points == 0: the points inside the vertex bounding box, both ends inclusive (egohmr.py:550-552); else every point
 *               (egohmr_volsmpl.py:609-612).  No tau, no margin.
 *   occupancy   with a = v0 - p, b = v1 - p, c = v2 - p:
 *                 Omega_f = 2 atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|),   w(p) = sum_f Omega_f / (4 pi),
 *               inside <=> w(p) > 0.5.  On a closed mesh w is 0 or 1 up to rounding; on a mesh that is not closed (the synthetic asset's
 *               random faces) w is fractional: the term is then defined, but not meaningful.
 *   depth       d(p) = min_f dist(p, triangle f), at the closest point c = sum_k beta_k v_{f,k} (closest point on a triangle: vertex, edge
 *               and face regions); among equally near faces the lowest index.
 *   degenerate  a face that repeats a vertex index has no area and no side: it adds 0 to w (never a NaN) and is left out of the minimum.
 *   outputs     loss[b] = sum over selected, inside points of d(p)^2;  hits[b] (may be NULL) = their number;
 *               gverts[b, f_k] (may be NULL; [B,V,3], overwritten) += 2 beta_k (c - p): the derivative of d^2 at fixed beta, exact in the face,
 *               edge and vertex regions alike (envelope argument); the indicator carries no gradient.  A body without a selected inside point has
 *               exact zeros in all three.
 * Any V, any F >= 1 (B <= 65535).  loss and hits are the same bits from call to call; gverts is accumulated with float atomics (last-bit spread).
 * faces is on the DEVICE; an index outside [0, V) is the caller's to avoid (nothing checks it here).
 * The kernel walks the faces through LDS in chunks of EHM_MESH_COLLISION_FACE_CHUNK, for blocks of EHM_MESH_COLLISION_POINT_BLOCK points. */
#define EHM_MESH_COLLISION_FACE_CHUNK 512
#define EHM_MESH_COLLISION_POINT_BLOCK 256
int ehm_mesh_collision_query(const float* verts, const int32_t* faces, const float* scene, float* loss, float* gverts, int32_t* hits, int B,
                             int V, int F, int N, int all_points, void* stream);

/* The collision term of the guided steps of ehm_sample_loop, as a setting of the SMPL handle (read at the loop's entry, like the GCN handle's
 * pass map and fuse scales): faces_host [F,3] int32 on the HOST, every index in [0, V) (else EINVAL, nothing changed); the handle takes its own
 * device copy.  F = 0 clears it.  With a mesh set the guided steps use the mesh collision term above (ehm_sample_desc.tau is ignored;
 * guide_all_points selects every point); with none they use the vertex proxy of ehm_collision_proxy, as before.  Waits for the device. */
int ehm_smpl_set_collision_mesh(ehm_smpl* h, const int32_t* faces_host, int F);

/* VJP of ehm_smpl_forward_rot6d w.r.t. the DE-NORMALISED 6-D pose (the quirk of egohmr.py:523-528:
 * autograd.grad is taken w.r.t. x_t*std+mean): gverts [B,V,3] -> gpose6d [B,144].
 * Needs the forward's x/mean/std/betas again (recomputes the chain). */
int ehm_smpl_backward_rot6d(ehm_smpl* h, const float* betas, const float* x, const float* mean, const float* std,
                            const float* gverts, float* gpose6d, int B, void* stream);

/* General VJP of ehm_smpl_forward (smplx lbs.py `lbs` / SMPL.forward: blend shapes, joint regression, rigid chain, skinning, vertex-picked
 * extra joints) - what autograd does behind `self.smpl(...)` at egohmr.py:537 when `torch.autograd.grad` is taken at :562:
 *   gverts  [B,V,3]          cotangent of the vertices, or NULL
 *   gjoints [B,24+n_extra,3] cotangent of the joints (posed joints, then the vertex picks), or NULL    (at least one of the two)
 *   gbetas  [B,10]           d / d betas, or NULL
 *   grotmats [B,24,3,3]      d / d the local rotation matrices, entry by entry (no orthogonality constraint), or NULL   (at least one of the two)
 * betas / rotmats: the forward's inputs (the chain is recomputed).  Reproducibility: the pose-blend and shape contractions, the extra-joint
 * scatter and the chain pass sum in a fixed order, but the skinning VJP they share with ehm_smpl_backward_rot6d accumulates the per-joint
 * transform gradients with float atomics, and both outputs are derived from those: with more than two contributing vertices per joint,
 * grotmats and gbetas are reproducible from call to call only up to the last bits (order of float32 additions) - ehm_smpl_backward_ordered
 * below is the variant that repeats its bits.  Launches on `stream`
 * out of `workspace` (16-byte aligned, at least *bytes of ehm_smpl_backward_workspace_bytes(h, B, &bytes)): no allocation, no host
 * synchronisation.  Bad arguments are refused with EINVAL before anything is launched. */
int ehm_smpl_backward(ehm_smpl* h, const float* betas, const float* rotmats, const float* gverts, const float* gjoints, float* gbetas,
                      float* grotmats, int B, void* workspace, int64_t workspace_bytes, void* stream);
/* ehm_smpl_backward with EVERY sum in a fixed order (the training route of EgoHMR.forward: a step's gradients repeat their bits).  The same
 * launches plus two: before the skinning VJP a kernel of its own sums the per-joint transform gradients without atomics (a wave adds its 64
 * vertices by lane, a block its four waves one after the other, per vertex tile), behind it a finish kernel adds the tiles in index order and
 * replaces the atomically accumulated values.  Same arguments; workspace: *bytes of ehm_smpl_backward_ordered_workspace_bytes (larger by the
 * tiles' partial sums).  ehm_smpl_backward and its callers are unchanged. */
int ehm_smpl_backward_ordered_workspace_bytes(const ehm_smpl* h, int B, int64_t* bytes);
int ehm_smpl_backward_ordered(ehm_smpl* h, const float* betas, const float* rotmats, const float* gverts, const float* gjoints, float* gbetas,
                              float* grotmats, int B, void* workspace, int64_t workspace_bytes, void* stream);
int ehm_smpl_backward_workspace_bytes(const ehm_smpl* h, int B, int64_t* bytes);

/* egohmr.py:561-570: g = -(1/denom) * gpose6d (denom = B for loss.mean(), 1 for loss.sum()),
 * joints 3..23 scaled by 2, joints {0,3,6,9,12..23} zeroed; all-zero loss -> zeros. */
int ehm_guidance_grad_finish(const float* gpose6d, const float* loss, float* grad, int B, float denom, void* stream);

/* ------------------------------------------------------------------ post-loop metric ---------- */
/* pytorch3d.ops.knn_points(x, y, K=1) as used by utils/pytorch3d_chamfer_distance.py:152-156 (contact score,
 * test_egohmr.py:496-505): for every x[b,i] the SQUARED distance to its nearest y[b,:] and (optionally) its index.
 * x [B,P1,3], y [B,P2,3] -> dist2 [B,P1], idx [B,P1] int32 or NULL. */
int ehm_nn_dist2(const float* x, const float* y, float* dist2, int32_t* idx, int B, int P1, int P2, void* stream);

/* ------------------------------------------------------------------ evaluation block ---------- */
/* test_egohmr.py:399-449: Euclidean error per point of S samples per item against ONE ground truth per item, its mean over the points and its sums over
 * the visible / invisible points (G-MPJPE :399-407: joints in the camera frame; MPJPE :409-417 and V2V :441-449: pelvis-aligned).
 *   pred [B,S,pred_points,3] and gt [B,gt_points,3]: the first P points of each are compared (SMPL hands over 45 joints, the metrics use 24);
 *   pred_origin [B,S,3] / gt_origin [B,3]: subtracted first (NULL = nothing: the caller aligned already, or G-MPJPE); or origin_point >= 0: each cloud's own
 *     point of that index is its origin (joint 0 = the pelvis, :409) and both pointers are NULL; origin_point < 0: pointers only;
 *   mask [B,P] (NULL: everything visible);  per_point [B,S,P] (may be NULL);  mean [B,S];  vis_sum, invis_sum [B,S] (may be NULL). */
typedef struct ehm_eval_points_desc {
  const float* pred; const float* gt; const float* pred_origin; const float* gt_origin; const uint8_t* mask;
  float* per_point; float* mean; float* vis_sum; float* invis_sum;
  int B, S, P, pred_points, gt_points, origin_point;
} ehm_eval_points_desc;
int ehm_eval_point_errors(const ehm_eval_points_desc* d, void* stream);
/* utils/pose_utils.py:10-66 (compute_similarity_transform) + :109-126 (reconstruction_error) as called at test_egohmr.py:419-437: the similarity transform
 * (scale, rotation, translation) of each pred[b,s] [J,3] closest to gt[b] [J,3] - float64 in registers like the reference's per-sample numpy loop, the
 * 3 x 3 SVD by one-sided Jacobi - then the per-joint error.  aligned [B,S,J,3], per_joint [B,S,J], mean [B,S], vis_sum / invis_sum [B,S] with mask [B,J]:
 * each may be NULL (one of aligned / per_joint / mean must not be).  Any J >= 3 (no per-joint arrays).  A rank-deficient correlation matrix (a collinear or
 * planar cloud) gets an orthonormal completion that keeps every known singular vector (csrc/procrustes_solve.h); a one-point pred is NaN, as the reference. */
int ehm_eval_procrustes(const float* pred, const float* gt, const uint8_t* mask, float* aligned, float* per_joint, float* mean, float* vis_sum,
                        float* invis_sum, int B, int S, int J, void* stream);
/* utils/pose_utils.py:75-107 (compute_similarity_transform_with_vis_mask) + :119-126 as test_egohmr.py:427-437 runs it with --eval_with_vis_mask_pa:
 * the joints of BOTH clouds that align_mask [B,J] marks invisible are multiplied by 0, not dropped - they stay in the means over all J as points at the
 * origin, and the centred masked copies give K and var1; the similarity is then applied to the UNMASKED pred[b,s] and the error is taken over all J
 * against the unmasked gt[b].  align_mask also splits vis_sum / invis_sum (sum of error * mask, error * (1 - mask): a NaN error reaches both, as in the
 * reference).  No visible joint: var1 = 0 and every output of that item is NaN.  Outputs as ehm_eval_procrustes; any J >= 1 (no per-joint arrays). */
int ehm_eval_procrustes_vis(const float* pred, const float* gt, const uint8_t* align_mask, float* aligned, float* per_joint, float* mean, float* vis_sum,
                            float* invis_sum, int B, int S, int J, void* stream);
/* test_egohmr.py:453-494: sample diversity of joints [B,S,J,3] over the joints selected by mask [B,J] (NULL: all; invert != 0: the unselected ones) -
 * std_out [B] = mean over the selected joints and the 3 coordinates of the unbiased std over the samples; apd_out [B] = sum over ordered sample pairs and
 * selected joints of the joint distance / n_selected / S / (S - 1) / 2 (the reference's normalisation).  No selected joint -> NaN, as the reference. */
int ehm_eval_diversity(const float* joints, const uint8_t* mask, int invert, float* std_out, float* apd_out, int B, int S, int J, void* stream);

/* ------------------------------------------------------------------ stage 1 (ProHMR-scene) translation ---------- */
/* The deterministic half of the stage-1 model (models/prohmr/prohmr_scene.py:111-130, fc_head.py:46-50) and the camera conversion of
 * test_prohmr_scene.py:175-213 (utils/geometry.py:119-131), per item, in one launch:
 *   ctx = [cam_cx/ofx, cam_cy/ofx | box_center_x/ofx, box_center_y/ofx, box_size/ofx | fx | img_feats | scene_feats],  ofx = fx * fx_norm,
 *         each of the three leading groups present only with its flag; read in place (no concatenated copy), K = its length
 *   h = relu(W1 ctx + b1) (hidden = 1024),  off = W2 h + b2 (13),  pred_betas = off[0:10] + init_betas,  pred_cam = off[10:13] + init_cam
 *   pred_cam_full = convert_pare_to_full_img_cam(pred_cam, box_size, box_center, 2 cam_cx, 2 cam_cy, fx * fx_norm, crop_res)   (s is not clamped)
 * W1t is nn.Linear's weight TRANSPOSED, [K, hidden] row-major; W2 is [13, hidden] as nn.Linear keeps it.  f32 FMA throughout.
 * pred_betas may be NULL. */
typedef struct ehm_stage1_desc {
  const float* img_feats;    /* [B, img_dim]   */
  const float* scene_feats;  /* [B, scene_dim] */
  const float* fx; const float* cam_cx; const float* cam_cy; const float* box_center /* [B,2] */; const float* box_size;   /* [B] each */
  const float* W1t; const float* b1; const float* W2; const float* b2; const float* init_cam; const float* init_betas;
  float* pred_cam;           /* [B,3]  */
  float* pred_cam_full;      /* [B,3]  */
  float* pred_betas;         /* [B,10] */
  float fx_norm, crop_res;
  int with_cam_center, with_bbox_info, with_focal_length;
  int img_dim, scene_dim, hidden, B;
} ehm_stage1_desc;
int ehm_stage1_head(const ehm_stage1_desc* d, void* stream);

/* ------------------------------------------------------------------ stage 1: the conditional Glow flow (csrc/flow.hip) ---------- */
/* The pose flow of models/prohmr/smpl_flow.py, nflows' ConditionalGlow(144, 1024, 4, 2, context_features = ctx), both directions and their first
 * derivatives (the entries from ehm_flow_wgrad on; eval-mode BatchNorm inside the ResidualNet is forward only): per block an
 * ActNorm and an LULinear (folded on the host into one affine map) and an additive coupling whose net is a ResidualNet conditioned on the context
 * by GLU gates.  The definition the kernels follow is restated in float64 in tests/flow_ref.py.  A direction is a chain of ehm_flow_gemm launches
 * (one per product) between ehm_flow_context and ehm_flow_finish; nothing in it synchronises or reads back, nothing uses atomics. */

/* The conditioning row of prohmr_scene.py:111-130, the columns of ehm_stage1_head's ctx, written out: out [B, ctx_pad], ctx_pad >= K (the live
 * width), columns K .. ctx_pad - 1 zero. */
typedef struct ehm_flow_context_desc {
  const float* img_feats;    /* [B, img_dim]   */
  const float* scene_feats;  /* [B, scene_dim] */
  const float* fx; const float* cam_cx; const float* cam_cy; const float* box_center /* [B,2] */; const float* box_size;   /* [B] each */
  float* out;                /* [B, ctx_pad]   */
  float fx_norm;
  int with_cam_center, with_bbox_info, with_focal_length;
  int img_dim, scene_dim, ctx_pad, B;
} ehm_flow_context_desc;
int ehm_flow_context(const ehm_flow_context_desc* d, void* stream);

/* Y = epi(pro(X)[R, K] . W[K, N]) in exact float32 (v_mfma_f32_32x32x2_f32), the numerics of ehm_skinny_gemm_f32: a 32 x 32 output tile per block,
 * its waves (16 for K >= 1024, else 4) split K in 8-k groups, each wave one k-ordered chain, the waves' sums added in wave order.  The order along k
 * depends on K alone.  Rows >= R of a tile are neither read nor written, columns >= N are not written.
 *   X        [R, ldx]; with `gather` (K ints) column k is X[r][gather[k]] (an index outside [0, ldx) reads as 0), else column k itself
 *            (ldx >= K, ldx % 4 == 0, X 16-byte aligned)
 *   W        [K, ldw] row-major (nn.Linear's weight transposed; in a backward product dY W^T the weight itself, [out, in] = [K, N]), ldw % 32 == 0,
 *            ldw >= N, K % 8 == 0; bias [N] or NULL.  w_window != 0 lifts ldw % 32 == 0: columns >= N of W are never read, so any row-major
 *            matrix with ldw >= N - a weight in torch layout, a column window of a wider one - is an operand as it lies, at no copy
 *   prologue EHM_FLOW_PRO_NONE x | _RELU max(x, 0) | _BN_RELU max(pro_scale[k] x + pro_shift[k], 0) (an eval-mode BatchNorm1d) |
 *            _SHIFT x - pro_shift[k] | _GATE x sigmoid(item[i][k]) (the cotangent of a GLU's value half; item as below with ld_item >= K, and the
 *            epilogue is then none of the two per-item ones)
 *   epilogue with v = acc + bias[n], i = r / S (the item of row r; S >= 1):
 *            EHM_FLOW_EPI_BIAS      Y[r][n] = v                                      (also the affine maps: state A^T + c, (state - c) Ainv^T by _SHIFT)
 *            EHM_FLOW_EPI_ITEM_ADD  Y[r][n] = v + item[i][n]                         (a first layer plus its context term)
 *            EHM_FLOW_EPI_GLU_RES   Y[r][n] = Y[r][n] + v sigmoid(item[i][n])        (F.glu of cat[v, context] plus the residual, in place)
 *            EHM_FLOW_EPI_SCATTER_ADD / _SUB   Y[r][scatter[n]] +/-= v               (the coupling update, in place on the state; scatter: N ints,
 *                                                                                     distinct; one outside [0, ldy) is skipped; with
 *                                                                                     gather = transform_features / scatter = identity_features the
 *                                                                                     two ends of a coupling's backward, the sign being the coupling's)
 *            EHM_FLOW_EPI_MASK      Y[r][n] = mask[r][n] > 0 ? v : 0                 (the backward of a ReLU on the saved pre-activation `mask`)
 *            EHM_FLOW_EPI_MASK_ADD  Y[r][n] = add[r][n] + (mask[r][n] > 0 ? v : 0)   (the same plus the residual's cotangent; add may be Y)
 *            EHM_FLOW_EPI_ADD       Y[r][n] = add[r][n] + v                          (a sum of products over several launches; add may be Y)
 *            With _GLU_RES, a non-NULL `add` [R, ld_add] is read in place of Y (Y = add + v sigmoid(.): the input of the block survives, same bits)
 *            and a non-NULL `aux` [R, ldy] receives v (the GLU's value half u2, kept for the backward).  Elsewhere add and aux are NULL.
 *   Y        [R, ldy], never X itself; item [ceil(R / S), ld_item]; mask [R, ld_mask], never Y. */
enum { EHM_FLOW_PRO_NONE = 0, EHM_FLOW_PRO_RELU = 1, EHM_FLOW_PRO_BN_RELU = 2, EHM_FLOW_PRO_SHIFT = 3, EHM_FLOW_PRO_GATE = 4 };
enum { EHM_FLOW_EPI_BIAS = 0, EHM_FLOW_EPI_ITEM_ADD = 1, EHM_FLOW_EPI_GLU_RES = 2, EHM_FLOW_EPI_SCATTER_ADD = 3, EHM_FLOW_EPI_SCATTER_SUB = 4,
       EHM_FLOW_EPI_MASK = 5, EHM_FLOW_EPI_MASK_ADD = 6, EHM_FLOW_EPI_ADD = 7 };
typedef struct ehm_flow_gemm_desc {
  const float* X; const int32_t* gather; const float* W; const float* bias;
  const float* pro_scale; const float* pro_shift;
  const float* item; const int32_t* scatter;
  float* Y;
  int R, K, N, S;
  int ldx, ldw, ldy, ld_item;
  int prologue, epilogue;
  const float* mask; const float* add; float* aux;    /* the backward's operands (above); NULL in a forward chain without saved activations */
  int ld_mask, ld_add;
  int w_window;
} ehm_flow_gemm_desc;
int ehm_flow_gemm(const ehm_flow_gemm_desc* d, void* stream);

/* The end of a direction, per row: log_prob[r] = -1/2 ||z_r||^2 + log_prob_const, the 144 squares added in index order by float32 fmaf and
 * log_prob_const = -72 log 2 pi -/+ the chain's log|det| (data independent, summed on the host in float64) added in float64.  With `pose`
 * (the sampling side: the chain's output x [R,144]) also pred_pose_6d = x and the 24 rotation matrices of utils/geometry.py:56-57 ('prohmr':
 * mode 0 of ehm_rot6d_to_rotmat, the same device function): global_orient [R,1,3,3], body_pose [R,23,3,3].  pose, pose6d_out, global_orient,
 * body_pose: all four or none. */
int ehm_flow_finish(const float* z, double log_prob_const, float* log_prob, const float* pose, float* pose6d_out, float* global_orient,
                    float* body_pose, int R, void* stream);

/* A weight gradient of the flow: out[n * ld_out + k] = alpha sum_r G'[r][n] X'[r][k] + beta out[n * ld_out + k], n < Cg, k < Ca, in nn.Linear's
 * [out, in] layout, so it lands in a gradient buffer or in a column window of a wider one (ld_out >= Ca; other columns are left alone; beta == 0
 * does not read out).  The contraction runs over the R rows straight from the row-major operands (no transpose, no packing), in exact float32
 * (v_mfma_f32_32x32x2_f32): one wave per 32 x 32 tile of out and ONE chain in row order per tile, so the order of the sum depends on R alone; no
 * atomics, no workspace, two calls give the same bits.  (ehm_pointnet_bwd_wgrad has the same numerics but a contract - rows in bodies of N_padded
 * % 192, widths % 128 - that none of the flow's operands meets.)
 *   G' [r][n] = G[r][gather_g ? gather_g[n] : n], times sigmoid(item[r / S][n]) when item is not NULL (a GLU's value-half cotangent)
 *   X' [r][k] = act(X[r][gather_x ? gather_x[k] : k] - (x_shift ? x_shift[k] : 0)), act = EHM_FLOW_ACT_NONE | _RELU
 * A gather index outside its row reads as 0.  G [R, ldg], X [R, ldx], item [ceil(R / S), ld_item >= Cg]; out is neither G nor X. */
enum { EHM_FLOW_ACT_NONE = 0, EHM_FLOW_ACT_RELU = 1 };
typedef struct ehm_flow_wgrad_desc {
  const float* G; const int32_t* gather_g; const float* item;
  const float* X; const int32_t* gather_x; const float* x_shift;
  float* out;
  int R, Cg, Ca, S;
  int ldg, ldx, ld_item, ld_out;
  int act;
  float alpha, beta;
} ehm_flow_wgrad_desc;
int ehm_flow_wgrad(const ehm_flow_wgrad_desc* d, void* stream);

/* The backward's sums, each in a fixed order (two calls give the same bits), i = r / S the item of row r:
 *   EHM_FLOW_RED_COLS   out[n] = scale sum_r G'[r][n], n < N, G' as in ehm_flow_wgrad (gather, item gate): a bias gradient.  Sixteen runs of
 *                       consecutive rows are summed in row order and the sixteen sums added in run order.
 *   EHM_FLOW_RED_ITEM   out[i * ld_out + n] = scale sum_{r in item i} G[r][n]: the gradient of a first layer's per-item term
 *   EHM_FLOW_RED_GATE   out[i * ld_out + n] = scale sum_{r in item i} G[r][n] U2[r][n] s (1 - s), s = sigmoid(item[i][n]): that of a GLU gate's
 * G [R, ldg], U2 [R, ldu], item [ceil(R / S), ld_item >= N]; the two per-item modes take no gather list. */
enum { EHM_FLOW_RED_COLS = 0, EHM_FLOW_RED_ITEM = 1, EHM_FLOW_RED_GATE = 2 };
typedef struct ehm_flow_reduce_desc {
  const float* G; const int32_t* gather; const float* U2; const float* item;
  float* out;
  int R, N, S;
  int ldg, ldu, ld_item, ld_out;
  int mode;
  float scale;
} ehm_flow_reduce_desc;
int ehm_flow_reduce(const ehm_flow_reduce_desc* d, void* stream);

/* The VJP of ehm_flow_finish.  Every group is optional (NULL outputs are not computed), at least one is asked for:
 *   dz [R,144] = (dz_add ? dz_add : 0) - g_log_prob[r] z[r][.]   (one fmaf: exact to one rounding; g_log_prob == NULL: a copy of dz_add)
 *   sum_g_log_prob [1] = sum_r g_log_prob[r], the cotangent of the chain's log|det| (lane l of one wave adds rows l, l + 64, ..., then the 64 sums
 *                        are added in lane order)
 *   dpose [R,144] = the 'prohmr' rot6d VJP (mode 0 of ehm_rot6d_to_rotmat_bwd, the same device function) of g_global_orient [R,1,3,3] and
 *                   g_body_pose [R,23,3,3] at pose [R,144], plus g_pose6d [R,144]; each of the three cotangents may be NULL (zero). */
int ehm_flow_finish_backward(const float* g_log_prob, const float* z, const float* dz_add, float* dz, float* sum_g_log_prob, const float* pose,
                             const float* g_pose6d, const float* g_global_orient, const float* g_body_pose, float* dpose, int R, void* stream);

/* ------------------------------------------------------------------ scene clouds -------------- */
/* The scene point cloud each stage reads, per item, from scene meshes resident on the device (csrc/scene.hip).  It replaces the offline
 * preprocessing plus the loader's transform:
 *   EHM_SCENE_WHOLE  stage 1: preprocess_scene_s1.py:94-118 (the chain of mesh.transform, z > 0, uniform_down_sample, first `target`) and
 *                    dataloaders/egobody_dataset.py:205-212 (points_coord_trans into the PV camera)
 *   EHM_SCENE_CUBE   stage 2: preprocess_scene_s2_for_test.py:176-208 (rotation about y through the centre, inclusive xz bounds,
 *                    y <= min(y) + cube_size, uniform_down_sample, first `target`) and egobody_dataset.py:213-225
 * then [::stride] and the float32 cast of egobody_dataset.py:272-273.  select(pred, target): the n vertices where pred holds, in mesh order;
 * k = n / target; rows r / k of the ranks r with r % k == 0 and r / k < target.  The predicates are float64 with every operation rounded in the
 * reference's order; the output row is T_out v of the ORIGINAL mesh vertex, ((T0 x + T1 y) + T2 z) + T3 in float64, rounded once to float32.
 *
 * Meshes: one float64 SoA buffer verts = [x[total_verts] | y[total_verts] | z[total_verts]], mesh m is [mesh_offsets[m], mesh_offsets[m+1]).
 * Items go in groups of up to EHM_SCENE_GROUP items of the same mesh (groups [num_groups, 1 + EHM_SCENE_GROUP] int32: the mesh, then the items,
 * -1 after the last): a vertex load serves the whole group.  params [B, EHM_SCENE_PARAMS] float64 per item, at the EHM_SCENE_P_* slots: the
 * chain (chain_len 3x4 matrices, rows of 4) or the cube's cos a, sin a, centre x, z, bounds and cube_size; T_out (3x4) in both modes.
 * Per item, written: status (EHM_SCENE_OK, _TOO_FEW: n < target, _EMPTY_CROP: no vertex passes the xz test) and n_selected; points
 * [B, ceil(target/stride), 3] f32 and index [B, ceil(target/stride)] int64 (the source vertex within its mesh; may be NULL) of the OK items
 * only.  At most five launches; the workspace (ehm_scene_workspace_bytes) needs no initialisation. */
#define EHM_SCENE_GROUP 8
#define EHM_SCENE_PARAMS 64
#define EHM_SCENE_MAX_CHAIN 4
#define EHM_SCENE_P_CHAIN 0   /* whole scene: chain_len x 12 */
#define EHM_SCENE_P_COS 0     /* cube: cos a, sin a, cx, cz, x_min, x_max, z_min, z_max, cube_size */
#define EHM_SCENE_P_SIN 1
#define EHM_SCENE_P_CX 2
#define EHM_SCENE_P_CZ 3
#define EHM_SCENE_P_XMIN 4
#define EHM_SCENE_P_XMAX 5
#define EHM_SCENE_P_ZMIN 6
#define EHM_SCENE_P_ZMAX 7
#define EHM_SCENE_P_CUBE 8
#define EHM_SCENE_P_OUT 48    /* both: T_out, 12 */
enum { EHM_SCENE_WHOLE = 0, EHM_SCENE_CUBE = 1 };
enum { EHM_SCENE_OK = 0, EHM_SCENE_TOO_FEW = 1, EHM_SCENE_EMPTY_CROP = 2 };
typedef struct ehm_scene_desc {
  const double* verts;          /* [3, total_verts] */
  int64_t total_verts;
  const int64_t* mesh_offsets;  /* [num_meshes + 1] */
  int num_meshes;
  int64_t max_mesh_verts;       /* the largest mesh's vertex count (sizes the grid and the workspace) */
  const int32_t* groups;        /* [num_groups, 1 + EHM_SCENE_GROUP] */
  int num_groups;
  const double* params;         /* [B, EHM_SCENE_PARAMS] */
  int mode, chain_len, B, target, stride;
  float* points;                /* [B, ceil(target/stride), 3] */
  int64_t* index;               /* [B, ceil(target/stride)] or NULL */
  int64_t* n_selected;          /* [B] */
  int32_t* status;              /* [B] */
  void* workspace;
  int64_t workspace_bytes;
} ehm_scene_desc;
/* *bytes = the workspace ehm_scene_select needs for this descriptor (its workspace fields are not read); a status, like every entry point whose
 * result is not a value of its own */
int ehm_scene_workspace_bytes(const ehm_scene_desc* d, int64_t* bytes);
int ehm_scene_select(const ehm_scene_desc* d, void* stream);

/* ------------------------------------------------------------------ batch building ------------ */
/* The two per-pixel / per-point stages of the reference loader's item (dataloaders/augmentation.py:get_example), per batch, on the device
 * (csrc/batch.hip).  Everything else of the item is 25 rows of arithmetic and stays on the host (egohmr_amd/batch.py).
 *
 * Image patch: generate_image_patch's warp + BGR -> RGB + convert_cvimg_to_tensor + the colour / normalise loop (augmentation.py:121-150,
 * :373-383) in one launch.  frames uint8 [F,H,W,3], BGR as decoded; item b reads frame frame_index[b] (any order, frames may be shared).
 * params [B, EHM_PATCH_PARAMS] float64 per item: Minv (2x3, patch pixel -> source pixel: the closed-form inverse of the loader's `trans`), the
 * flip flag (!= 0: the source is the mirrored frame, column W-1-x) and the three colour scales (RGB).  Output pixel (x, y), channel c (RGB;
 * BGR channel 2-c), every float64 operation rounded on its own:
 *   sx = (Minv00 x + Minv01 y) + Minv02, sy alike; x0 = floor(sx), fx = sx - x0; y0, fy alike
 *   a, b, c, d = source (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1); a neighbour outside the frame is 0 and is never loaded
 *   v = (a (1-fx) + b fx) (1-fy) + (c (1-fx) + d fx) fy;  quantize != 0: v = floor(v + 0.5) (the uint8 patch of the loader)
 *   p = float32(v); p = clip(p * float32(color[c]), 0, 255); img = (p - float32(mean[c])) / float32(std[c])     (float32 operations)
 * This is the real-valued bilinear rule, not cv2.warpAffine's 1/32-pixel grid with 15-bit weights.  An item whose frame index is outside
 * [0, F) gets NaN pixels.  P % 4 == 0 (one thread writes four consecutive x of each plane), img 16-byte aligned, B <= 65535.  No atomics:
 * two calls give the same bits. */
#define EHM_PATCH_PARAMS 16
#define EHM_PATCH_P_MINV 0    /* 6: the rows of Minv */
#define EHM_PATCH_P_FLIP 6
#define EHM_PATCH_P_COLOR 7   /* 3: RGB */
typedef struct ehm_image_patch_desc {
  const uint8_t* frames;        /* [F, H, W, 3] BGR */
  int F, H, W;
  const int32_t* frame_index;   /* [B] */
  const double* params;         /* [B, EHM_PATCH_PARAMS] */
  int B, P, quantize;
  double mean[3], std[3];       /* RGB, 0..255 units */
  float* img;                   /* [B, 3, P, P] */
} ehm_image_patch_desc;
int ehm_image_patch(const ehm_image_patch_desc* d, void* stream);

/* Scene-cloud augmentation: augmentation.py:429-438 + scene_verts_3d_processing + egobody_dataset.py:272-273 in one pass.  scene [B,N,3]
 * float32 (scene_is_f64 == 0) or float64; params [B, EHM_AUG_PARAMS] float64 per item: cam_t_full, cam_t_crop, the flip flag, cos and sin of
 * -rot.  Rows 0, stride, 2 stride, ... only; out float32 [B, ceil(N/stride), 3].  Per point p, every float64 operation rounded on its own:
 *   q = (p - t_full) + t_crop;  flip: q.x = -q.x;  r = ((cos q.x + (-sin) q.y) + 0 q.z, (sin q.x + cos q.y) + 0 q.z, (0 q.x + 0 q.y) + q.z)
 *   r = float32(r) (augmentation.py:287);  out = float32((r - t_crop') + t_full'), t' = t with x negated under flip (:434-436)
 * B <= 65535. */
#define EHM_AUG_PARAMS 16
#define EHM_AUG_P_TFULL 0     /* 3 */
#define EHM_AUG_P_TCROP 3     /* 3 */
#define EHM_AUG_P_FLIP 6
#define EHM_AUG_P_COS 7
#define EHM_AUG_P_SIN 8
int ehm_scene_augment(const void* scene, int scene_is_f64, const double* params, float* out, int B, int N, int stride, void* stream);

/* ------------------------------------------------------------------ JPEG decoding ------------- */
/* Baseline JPEG -> uint8 [F,H,W,3] BGR frames on the device, split where the format is serial: the bit-serial Huffman stage runs on the
 * host (csrc/jpeg_entropy.h, plain C++, one frame per caller thread), every arithmetic stage in two kernels (csrc/jpeg.hip).  The pixels
 * are libjpeg's defaults - the ISLOW integer IDCT, "fancy" upsampling, its fixed-point colour tables - which is what the reference's
 * cv2.imread(path, IMREAD_COLOR | IMREAD_IGNORE_ORIENTATION) (dataloaders/augmentation.py:346) and PIL both produce.  The rule was checked
 * bit for bit against PIL's decode (tests/golden/jpeg), NOT against cv2.  EXIF orientation is ignored, as the reference's flag asks.
 *
 * Entropy stage (host).  Markers SOI, DQT (8-bit tables), DHT, SOF0 / SOF1 with 8-bit precision, DRI, SOS, RSTn, EOI; APPn and COM are
 * skipped.  One interleaved scan of 1 or 3 components; luma sampling (1,1), (2,1) or (2,2) with chroma (1,1); a one-component frame counts
 * as (1,1).  Per block: the DC difference on a per-component predictor that resets at each restart interval, the AC run/size pairs (EOB,
 * ZRL), un-zigzag.  The output is the QUANTISED int16 coefficients (a dequantised value does not fit in int16): component planes one after
 * the other, each plane blocks in row-major order over the MCU-padded grid [blocks_y][blocks_x], each block 64 values in natural order.
 * Status -22 with a text for: progressive, arithmetic, lossless, 12-bit, 16-bit tables, 4 components, any other sampling, several scans, data
 * that ends early (a missing EOI included), a Huffman code with no entry, a coefficient index above 63, restart markers out of order, an
 * undefined table, a capacity too small.  Both host entries run without a GPU and make no device call.
 *
 * IDCT (jidctint; all int32, arithmetic right shifts).  x = coef * q, natural order.  One 1-D pass over x0..x7 with rounding r and shift s:
 *   z1 = (x2 + x6) 4433; t2 = z1 - x6 15137; t3 = z1 + x2 6270; t0 = ((x0 + x4) << 13) + r; t1 = ((x0 - x4) << 13) + r
 *   t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2
 *   a0 = x7, a1 = x5, a2 = x3, a3 = x1; z1 = a0 + a3, z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3; z5 = (z3 + z4) 9633
 *   a0 *= 2446, a1 *= 16819, a2 *= 25172, a3 *= 12299; z1 *= -7373, z2 *= -20995; z3 = z3 (-16069) + z5, z4 = z4 (-3196) + z5
 *   a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4
 *   outputs 0..7 = (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3) >> s
 * Columns first (s = 11, r = 1 << 10), then rows on their results (s = 18, r = 1 << 17); sample = clamp(result + 128, 0, 255).
 * The rule is exact where every intermediate of both passes - each value named above and the eight sums before the shift - fits in int32,
 * which holds for any block a DCT of 8-bit samples can produce (all 64 dequantised values at 1024 stay inside, all at 2048 leave it, and a
 * baseline stream may carry up to 1023 x 255).  Beyond that domain the pixels are unspecified, but every write stays inside frames and the workspace.
 * Upsampling, on each chroma plane cropped to its real size ceil(H v / vmax) x ceil(W h / hmax); edges replicate the last real row or
 * column, the samples of the MCU padding are never read:
 *   h2v1: out[2i] = (3 s[i] + s[i-1] + 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2
 *   h2v2: u = 3 cur + above for the upper output row, 3 cur + below for the lower one (at the plane's top and bottom the neighbour is cur);
 *         out[2i] = (3 u[i] + u[i-1] + 8) >> 4, out[2i+1] = (3 u[i] + u[i+1] + 7) >> 4
 *   a chroma plane of one or two columns is replicated instead (out[y][x] = s[y / v][x / h]): libjpeg takes the filter only above two.
 * Colour.  cb, cr = sample - 128; FIX(x) = int(x 65536 + 0.5); R = Y + ((FIX(1.40200) cr + 32768) >> 16);
 * B = Y + ((FIX(1.77200) cb + 32768) >> 16); G = Y + ((-FIX(0.34414) cb + (-FIX(0.71414) cr + 32768)) >> 16); clamped to 0..255, stored
 * B, G, R.  A one-component frame replicates Y.
 *
 * Device stage.  One call decodes F frames of ONE geometry (H, W, components, hmax, vmax - the block grids follow from them); quant holds a
 * row of 64 per frame and component (natural order), so qualities may differ within a call; rows 1 and 2 are independent: Cb is dequantised
 * with row 1 and Cr with row 2, whether or not the file gave them one table.  Two launches, no atomics, every byte written
 * once by one thread: two calls give the same bits.  The workspace holds the uint8 component planes on the MCU grid (coef_count bytes per
 * frame).  F <= 65535; coef 16-byte aligned. */
#define EHM_JPEG_MAX_COMPONENTS 3
typedef struct ehm_jpeg_header {
  int32_t H, W, components, hmax, vmax;
  int32_t mcus_x, mcus_y;                 /* the MCU grid */
  int32_t restart_interval;               /* MCUs, 0: none */
  int32_t h[EHM_JPEG_MAX_COMPONENTS], v[EHM_JPEG_MAX_COMPONENTS];                 /* sampling factors */
  int32_t blocks_x[EHM_JPEG_MAX_COMPONENTS], blocks_y[EHM_JPEG_MAX_COMPONENTS];   /* per-component block grid (MCU padded) */
  int32_t quant_id[EHM_JPEG_MAX_COMPONENTS];
  uint16_t quant[4][64];                  /* natural order; an undefined table is zero */
  int64_t coef_count;                     /* int16 values of one frame's coefficients */
} ehm_jpeg_header;
int ehm_jpeg_read_header(const uint8_t* data, int64_t n, ehm_jpeg_header* hdr);
/* hdr (may be NULL) is written as by the call above; nothing is written at or past coef + capacity (capacity in int16 values) */
int ehm_jpeg_entropy_decode(const uint8_t* data, int64_t n, ehm_jpeg_header* hdr, int16_t* coef, int64_t capacity);

typedef struct ehm_jpeg_decode_desc {
  const int16_t* coef;          /* device [F, coef_count] */
  const uint16_t* quant;        /* device [F, 3, 64]: frame f, component c (a one-component frame uses row 0) */
  int H, W, components, hmax, vmax;
  int F;
  uint8_t* frames;              /* device [F, H, W, 3] BGR */
  void* workspace;
  int64_t workspace_bytes;
} ehm_jpeg_decode_desc;
int ehm_jpeg_workspace_bytes(const ehm_jpeg_decode_desc* d, int64_t* bytes);
int ehm_jpeg_decode(const ehm_jpeg_decode_desc* d, void* stream);

/* ------------------------------------------------------------------ JPEG encoding ------------- */
/* uint8 [F,H,W,3] frames on the device -> baseline JPEG, every stage on the device (csrc/jpeg_enc.hip); only the compressed stream crosses
 * to the host, which writes 623 bytes of markers around it (csrc/jpeg_enc.h).  The rule is libjpeg's default encoder, the one behind
 * cv2.imwrite and PIL; it was checked bit for bit against PIL (libjpeg-turbo), NOT against cv2.  Fixed Huffman tables (no `optimize`), no
 * restart markers, no progressive mode.  Grey and 4-component files are out of scope.
 *
 * Input.  uint8 [F,H,W,3], B G R order (what the renderer and the decoder produce) or R G B with `rgb` set.
 * Colour (jccolor.c).  FIX(x) = int(x 65536 + 0.5), all integer:
 *   Y  = (FIX(.29900) R + FIX(.58700) G + FIX(.11400) B + 32768) >> 16
 *   Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.50000) B + (128 << 16) + 32767) >> 16
 *   Cr = (FIX(.50000) R - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16
 * Sampling.  Luma (hmax, vmax) is (1,1), (2,1) or (2,2), chroma (1,1): the decoder's three cases.
 * Padding and downsampling (jcsample.c, jcprepct.c).  The REAL block grid of a component is rw = ceil(W h / (8 hmax)) by
 * rh = ceil(H v / (8 vmax)).  Horizontally the full-resolution plane is extended to rw 8 (hmax / h) columns by repeating the last column,
 * then downsampled.  Vertically it is extended only to a multiple of vmax / v rows by repeating the last row, then downsampled; AFTER that
 * the plane is extended to rh 8 rows by repeating its last row (repeating full-resolution rows up to the block grid gives other numbers).
 *   h2v1: (a + b + bias) >> 1 with bias 0, 1, 0, 1, ... along the output row;  h2v2: (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ...
 * FDCT (jfdctint; int32; on the sample minus 128).  Rows first, then columns.  D(x, n) = (x + (1 << (n - 1))) >> n.  One pass over d0..d7:
 *   t0..t3 = d0 + d7, d1 + d6, d2 + d5, d3 + d4;  t7..t4 = d0 - d7, d1 - d6, d2 - d5, d3 - d4
 *   t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2
 *   out0, out4 = (t10 +- t11) << 2 in pass 1, D(t10 +- t11, 2) in pass 2
 *   z1 = (t12 + t13) 4433; out2 = D(z1 + t13 6270, n); out6 = D(z1 - t12 15137, n)
 *   z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7; z5 = (z3 + z4) 9633
 *   t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299; z1 *= -7373, z2 *= -20995; z3 = -16069 z3 + z5, z4 = -3196 z4 + z5
 *   out7 = D(t4 + z1 + z3, n), out5 = D(t5 + z2 + z4, n), out3 = D(t6 + z2 + z3, n), out1 = D(t7 + z1 + z4, n)
 * with n = 11 in pass 1 and n = 15 in pass 2; the result is 8 x the DCT.
 * Quantisation (jcdctmgr.c).  d = 8 q; a = |x| + (d >> 1); r = a / d if a >= d, else 0; the sign is restored.
 * Dummy blocks (jccoefct.c).  The coefficients use the decoder's layout: each plane [blocks_y = mcus_y v][blocks_x = mcus_x h][64] in natural
 * order, planes one after the other, int16 [F, coef_count].  Blocks beyond rw or rh are not transforms of padding: all their AC are zero; in a
 * real row a dummy block takes the DC of the block to its left; in a dummy row every block of an MCU takes the DC of the last block of the
 * previous block row of the same MCU (which may itself be a dummy column block).
 * Tables.  libjpeg's quality scaling of the Annex K.1 / K.2 tables: s = 5000 / q if q < 50, else 200 - 2 q; entry = clamp((base s + 50) / 100,
 * 1, 255).  Explicit uint16 [2][64] tables are accepted as well; luma uses table 0, both chroma planes table 1.  The four Annex K.3 - K.6
 * Huffman tables are fixed.
 * Entropy coding.  One interleaved scan, no restart markers.  MCUs in row-major order; within an MCU the luma blocks (rows, then columns),
 * then Cb, then Cr.  DC: the difference d to the previous block of the same component in scan order (predictor 0 at the start), size
 * s = bitlength(|d|): the Huffman code of s, then the low s bits of d if d >= 0, else of d - 1.  AC in zigzag order: a run of more than 15
 * zeros is one or more ZRL codes (0xF0), then the (run << 4) | size code and the value bits as for DC; a block that ends in zeros ends in
 * EOB (0x00).  The last byte is padded with 1 bits; then every byte FF is followed by 00.
 * File.  SOI, APP0 JFIF 1.01 (units 0, density 1 x 1, no thumbnail), DQT table 0, DQT table 1, SOF0, DHT DC0, AC0, DC1, AC1, SOS, the
 * stream, EOI (FF D9, the caller's two bytes): the order PIL writes.
 *
 * ehm_jpeg_forward: one launch; every value written once by one thread.  quant is [F,3,64] (natural order, the decoder's convention), so a call may mix
 * qualities; rows 1 and 2 are independent - Cb is quantised with row 1, Cr with row 2 - and a caller that writes a file with two tables
 * passes the chroma table twice; an entry of 0 is the caller's error (the device table is not inspected).
 * Its output is directly what ehm_jpeg_decode reads.  coef 16-byte aligned.
 * ehm_jpeg_entropy_encode: coefficients -> the stuffed streams uint8 [F, capacity] (SOS's end to EOI's start), lengths int64 [F] and needed
 * int64 [F].  needed[f] is the exact stream size whatever the capacity; lengths[f] = needed[f], or -1 when needed[f] > capacity (that
 * frame's stream is then not written; the others are), or -2 (needed 0) when a DC difference beyond +-2047 or an AC value beyond +-1023 has
 * no code.  Nothing is written at or past capacity.  Eight launches; the scans are one workgroup per frame walking
 * EHM_JPEG_ENC_SCAN_CHUNK elements at a time, the stuffing works on chunks of EHM_JPEG_ENC_STUFF_CHUNK bytes; no workgroup waits on
 * another.  The packing ORs atomically into the words two blocks share: OR commutes, so two calls give the same bits.  The workspace
 * (ehm_jpeg_entropy_encode_workspace_bytes; 16-byte aligned) holds EHM_JPEG_ENC_MAX_BLOCK_BYTES per block for the packed stream.
 * Both host entries run without a GPU.  Status -22 with a text, before any device call, for: a sampling other than the three, F > 65535,
 * misaligned buffers, a NULL pointer, a quantisation entry outside 1..255, a quality outside 1..100, a capacity below the header's size. */
#define EHM_JPEG_ENC_HEADER_BYTES 623
#define EHM_JPEG_ENC_SCAN_CHUNK 256
#define EHM_JPEG_ENC_STUFF_CHUNK 4096
#define EHM_JPEG_ENC_MAX_BLOCK_BYTES 208
int ehm_jpeg_quality_tables(int quality, uint16_t* quant /* [2][64] */);
/* SOI ... SOS into out[0 .. capacity): *n = EHM_JPEG_ENC_HEADER_BYTES, or 0 on a refusal (nothing is written then) */
int ehm_jpeg_write_header(int H, int W, int hmax, int vmax, const uint16_t* quant /* [2][64] */, uint8_t* out, int64_t capacity, int64_t* n);

typedef struct ehm_jpeg_forward_desc {
  const uint8_t* frames;        /* device [F, H, W, 3] */
  const uint16_t* quant;        /* device [F, 3, 64] */
  int H, W, hmax, vmax;
  int F;
  int rgb;                      /* 0: B G R, else R G B */
  int16_t* coef;                /* device [F, coef_count] */
} ehm_jpeg_forward_desc;
int ehm_jpeg_forward(const ehm_jpeg_forward_desc* d, void* stream);

typedef struct ehm_jpeg_entropy_encode_desc {
  const int16_t* coef;          /* device [F, coef_count] */
  int H, W, hmax, vmax;
  int F;
  uint8_t* streams;             /* device [F, capacity] */
  int64_t capacity;
  int64_t* lengths;             /* device [F] */
  int64_t* needed;              /* device [F] */
  void* workspace;
  int64_t workspace_bytes;
} ehm_jpeg_entropy_encode_desc;
int ehm_jpeg_entropy_encode_workspace_bytes(const ehm_jpeg_entropy_encode_desc* d, int64_t* bytes);
int ehm_jpeg_entropy_encode(const ehm_jpeg_entropy_encode_desc* d, void* stream);

/* ------------------------------------------------------------------ mesh rendering ------------ */
/* A software rasteriser for the overlays of test_egohmr.py --render True (utils/renderer.py:15-47 render_on_img / render_in_scene, called at
 * test_egohmr.py:576-619), which the reference draws with pyrender (csrc/render.hip).  The pixels are THIS RULE'S, not pyrender's: its PBR
 * shader, gamma and anti-aliasing are not reproduced.
 *
 * Inputs.  vertices float32 [B,V,3] in the camera frame, x right, y down, z forward (the reference's camera_pose = diag(1,-1,-1,1) is this
 * conversion); faces int32 [F,3], shared by the items; fx, fy, cx, cy float32 [B]; the output size H, W.
 * Projection and sampling.  u = fx x / z + cx, v = fy y / z + cy; pixel (row i, column j) is sampled at (u, v) = (j + 0.5, i + 0.5).
 * Coverage.  With p_k = (u_k, v_k) the projected vertices and s the sample, the edge functions are formed from differences to the triangle's own
 * vertices, never from products of absolute pixel coordinates:
 *   e0 = (u1-u0)(s.v-v0) - (v1-v0)(s.u-u0)    e1 = (u2-u1)(s.v-v1) - (v2-v1)(s.u-u1)    e2 = (u0-u2)(s.v-v2) - (v0-v2)(s.u-u2)
 *   area = (u1-u0)(v2-v0) - (v1-v0)(u2-u0)
 * The sample is covered when e0, e1, e2 all have the sign of area or are zero (edges inclusive, no top-left rule) and e0 + e1 + e2 != 0.
 * Dropped faces: area == 0; a vertex index outside [0, V); a non-finite vertex or projection; a vertex at z <= z_near (without clip_near, below,
 * a mesh that reaches behind the near plane loses those faces whole); cull_backface != 0 and area > 0 (v points down, so a face
 * that is counter-clockwise for an OpenGL viewer, i.e. front-facing, has area < 0).
 * Depth.  Perspective-correct: b = (e1, e2, e0) / (e0 + e1 + e2) are the weights of vertices 0, 1, 2; 1/z = b0/z0 + b1/z1 + b2/z2, evaluated as
 * z = (e0 + e1 + e2) / (e1/z0 + e2/z1 + e0/z2) with 1/z_k rounded to float32 once per face.  A pixel's
 * winner is the lexicographic minimum of (z, face index) over the covering faces, so the result does not depend on the order of the faces.
 * Normals.  Flat (smooth == 0): n = (p1 - p0) x (p2 - p0) of the camera-frame vertices.  smooth != 0: a vertex normal is the sum of that
 * un-normalised cross product over the incident faces in face-index order, gathered through the vertex -> face CSR (vf_offsets [V+1],
 * vf_faces [3F]; no atomics); a face whose cross product is not finite adds nothing.  The pixel's normal is sum_k (b_k / z_k) n_k.  It is
 * normalised per pixel; a zero or non-finite one gives n.l = 0.
 * Colour.  c = base * (ambient + diffuse * max(0, n.l)), two_sided != 0: |n.l|; base is base_color, or the per-vertex colours [V,3]
 * interpolated perspective-correctly (sum_k (b_k / z_k) c_k * z); clamped to [0, 1]; level = floor(255 c + 0.5).  light_dir is used as given
 * (the direction towards the light, unit length).
 * Composite (alphaMode OPAQUE).  A covered pixel takes the three levels, in the order of base_color's / vertex_colors' channels; every other
 * pixel keeps the background: frame frame_index[b] of frames uint8 [Fr,H,W,3] (items may share frames; an index outside [0, Fr) gives
 * bg_color), or bg_color when frames is NULL.
 * Outputs, each nullable and then not computed: color uint8 [B,H,W,3], depth float32 [B,H,W] (0 on background), face_index int32 [B,H,W] (-1).
 *
 * Faces are binned into 64 x 16 pixel tiles by their bounding boxes; an item's lists hold bin_capacity entries.  needed_capacity [B] receives
 * every item's need; an item that needs more is rendered as pure background (nothing is written past its lists) and the caller runs again with
 * max(needed_capacity).  ehm_render_workspace_bytes gives the workspace for a descriptor (its outputs' and workspace fields' VALUES are not
 * used, but at least one output must be requested).  No allocation, no host synchronisation, no float atomics: two calls give the same bits.
 * 16-byte stores of the colour tile need W % 16 == 0 and 16-byte aligned color / frames; any other case is written byte by byte.
 * B <= 65535, H, W <= 32768, V, F <= 2^24.
 *
 * Near-plane clipping (clip_near != 0; 0 is the rule above, bit for bit).  No geometry is cut: a face that straddles z = z_near is rasterised by a
 * homogeneous rule on its own three vertices, so its face index, normals and colours are the parent face's.
 * Which faces.  A face is CROSSING when its three vertex indices are valid, its three vertices are finite, at least one has z > z_near and at
 * least one has z <= z_near (a vertex exactly on the plane counts as behind).  A face wholly in front takes the rule above unchanged, with the same
 * bits; a face wholly behind, or with a non-finite vertex, is dropped as above.
 * The rule of a crossing face, in coordinates relative to the principal point (no product of absolute pixel coordinates appears):
 *   g_k = (fx x_k, fy y_k, z_k)        c_k = g_{k+1} x g_{k+2} (indices mod 3), a x b = (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x)
 *   D = (g_0x c_0x + g_0y c_0y) + g_0z c_0z                                    (= g_0 . (g_1 x g_2) = z_0 z_1 z_2 area)
 *   E_k = (c_kx (s.u - cx) + c_ky (s.v - cy)) + c_kz        S = (E_0 + E_1) + E_2
 * g_k, c_k and D are rounded once per face, not per pixel.  The face is dropped when D is 0 or not finite, or when cull_backface != 0 and D > 0
 * (the orientation test above).  The sample is covered when E_0, E_1, E_2 each have the sign of D or are zero, S != 0 and z = D / S > z_near:
 * the last condition is the clip.  Depth is that z.  The weights of vertices 0, 1, 2 are beta_k = E_k / S - the perspective-correct ones, what the
 * rule above calls (b_k / z_k) z - so the smooth normal is sum_k beta_k n_k (the flat one is unchanged) and the interpolated colour sum_k beta_k c_k.
 * The winner of a pixel is still the lexicographic minimum of (z, face index), over both kinds of face.
 * Binning box of a crossing face: the projections of its front vertices and of the two points where its edges meet the plane - on the edge a -> b
 * with exactly one end in front, t = (z_near - z_a) / (z_b - z_a), p = a + t (b - a), projected with z = z_near - padded and clamped like any
 * other box; the whole image when one of those coordinates is not finite.  A crossing face counts in needed_capacity like any other, its record
 * fits the same 64 bytes, and the workspace does not depend on clip_near.  clip_near must be 0 or 1. */
typedef struct ehm_render_desc {
  const float* vertices;        /* [B, V, 3] */
  const int32_t* faces;         /* [F, 3] */
  const int32_t* vf_offsets;    /* [V + 1], smooth != 0 only */
  const int32_t* vf_faces;      /* [3 F],   smooth != 0 only */
  const float* vertex_colors;   /* [V, 3] or NULL */
  const float *fx, *fy, *cx, *cy; /* [B] each */
  const uint8_t* frames;        /* [Fr, H, W, 3] or NULL */
  const int32_t* frame_index;   /* [B], with frames */
  int B, V, F, Fr, H, W;
  int smooth, two_sided, cull_backface;
  float z_near;
  float base_color[3], light_dir[3];
  float ambient, diffuse;
  uint8_t bg_color[4];          /* three used */
  int bin_capacity;             /* list entries per item */
  int32_t* needed_capacity;     /* [B] out */
  uint8_t* color;               /* [B, H, W, 3] or NULL */
  float* depth;                 /* [B, H, W] or NULL */
  int32_t* face_index;          /* [B, H, W] or NULL */
  void* workspace;
  int64_t workspace_bytes;
  int clip_near;                /* 0: a face with a vertex at z <= z_near is dropped whole; 1: it is drawn where z > z_near */
} ehm_render_desc;
int ehm_render_workspace_bytes(const ehm_render_desc* d, int64_t* bytes);
int ehm_render(const ehm_render_desc* d, void* stream);

/* ------------------------------------------------------------------ per-item scalars ---------- */
/* The per-item scalar work of EgoHMR.forward in front of the encoders, in two launches:
 *   vis [B,24] u8       models/egohmr/egohmr.py:186-188: confidence > 0, OpenPose joint `force_visible` (8) always on, gathered by joint_map
 *   mask_slot [B], mask_items [count], count [1] (int32)   which items need the image-masked second pass (:249-254: any invisible
 *                       joint), as ehm_gcn_set_pass_map wants them: slot of the item among those that do (ascending) or -1, and the
 *                       items in slot order.  pass_group > 1 rounds the need up to groups of pass_group consecutive items.
 *                       need_all = 1: EVERY item needs the second pass (guidance scales with scale_visible != 1: every joint combines the
 *                       two passes); 0 = the rule above.
 *   other[:, other_col0 ...] = TranslEnc(transl) (:217, Linear(3,t_hidden) -> ReLU -> Linear(t_hidden,t_out), torch [out,in] weights)
 *                       | camera features (:195-205: [cx, cy] / (fx*fx_norm), [box_center, box_size] / (fx*fx_norm), fx), zero-filled
 *                       up to other_ld (row stride of `other`; columns [0, other_col0) are the caller's: the scene features)
 *   finite [B] u8       0 when transl / fx / cx / cy / box / img_rowsum / scene_rowsum of the item hold a NaN or Inf (the float32
 *                       graph of the reference turns every output of such an item into NaN; see ehm_pack_outputs).  Every component
 *                       is tested on its own: finite components whose float32 sum would overflow are finite inputs
 * need_scratch: B bytes of device memory. */
typedef struct ehm_item_prep_desc {
  const float* keypoints_2d; /* [B, NK, 3] */
  const int32_t* joint_map;  /* [24] device */
  int NK, force_visible;
  const float *fx, *cx, *cy, *box_center, *box_size, *transl; /* [B], [B], [B], [B,2], [B], [B,3]; cx/cy/box may be NULL when unused */
  float fx_norm;
  int with_bbox, with_cam_center;
  const float *tW1, *tb1, *tW2, *tb2;
  int t_hidden, t_out;
  const float *img_rowsum, *scene_rowsum; /* [B] or NULL */
  float* other;
  int other_ld, other_col0;
  uint8_t* vis;
  int32_t *mask_slot, *mask_items, *count;
  uint8_t* finite;
  uint8_t* need_scratch;
  int pass_group;
  int B;
  int need_all;
} ehm_item_prep_desc;
int ehm_item_prep(const ehm_item_prep_desc* d, void* stream);

/* The output garnish of EgoHMR.forward (egohmr.py:283-301) in one launch, in place on the loop's outputs:
 *   bad item = !finite[b] or a non-finite value in chk[0..chk_rows)[b] (x_T and the draws that feed a denoiser evaluation, or the
 *   x_t of a single forward): x0, pose6d, R, verts, joints, betas of a bad item become NaN; x_final (may be NULL) additionally takes
 *   NaN where last_noise (the last step's draw, multiplied by nonzero_mask = 0: gaussian_diffusion.py:357-359) is not finite.
 *   global_orient [B,1,3,3] / body_pose [B,23,3,3] = the split of R; focal [B,2] = fx*fx_norm; center [B,2]; kp3d_full [B,J,3] =
 *   joints + transl; kp2d_full [B,J,2] = utils/geometry.py:78-116 perspective_projection, then x / 1920 - 0.5, y / 1080 - 0.5. */
typedef struct ehm_pack_desc {
  int B, J, V;
  const uint8_t* finite; /* [B] or NULL */
  const float* chk;      /* [chk_rows, B, 144] or NULL */
  int chk_rows;
  const float* last_noise; /* [B,144] or NULL */
  float* x_final;          /* [B,144] or NULL */
  float *x0, *pose6d, *R, *verts, *joints;
  const float* betas_in;
  float* betas_out;
  const float *transl, *fx, *cx, *cy;
  float fx_norm;
  float *global_orient, *body_pose, *kp3d_full, *kp2d_full, *focal, *center;
  uint8_t* finite_out; /* [B] or NULL */
} ehm_pack_desc;
int ehm_pack_outputs(const ehm_pack_desc* d, void* stream);

/* ------------------------------------------------------------------ validation losses -------- */
/* EgoHMR.compute_loss in its evaluation branch (models/egohmr/egohmr.py:307-449, self.training == False) on arrays that are already on the
 * device.  Terms, in the order of the reference's `losses` dict (:432-443) = the columns of `per_item` and the entries of `losses`:
 *   EHM_LOSS_TOTAL           :422-430  weights[0..8] . (V2V, KP3D, KP3D_FULL, KP2D_FULL, BETAS, BODY_POSE, GLOBAL_ORIENT, POSE_6D_ORTHO, PENETRATION)
 *   EHM_LOSS_V2V             :344-355  mean over B V 3 of |(pred_vertices - pred_keypoints_3d[:, 0]) - (gt_vertices - gt_joints[:, 0])|; the ground truth of
 *                                      item b is the FEMALE body where gender[b] == 1, else the male one (:350-351) - only the selected one is read
 *   EHM_LOSS_KP3D            :334-336, losses.py:44-50  joints 0..23 of pred_keypoints_3d / keypoints_3d, each minus its own joint 0, L1 summed per item
 *   EHM_LOSS_KP3D_FULL       :339-341  the same on pred_keypoints_3d_full / keypoints_3d_full without alignment
 *   EHM_LOSS_KP2D_FULL       :314-331, losses.py:20-25  pred_keypoints_2d_full[:, smpl_to_openpose] (:108-109) against keypoints_2d[:, :, :2], L1 times the
 *                                      confidence keypoints_2d[:, :, 2] with joints 1, 9, 12 set to 0, summed per item
 *   EHM_LOSS_BETAS / _BODY_POSE / _GLOBAL_ORIENT   :376-383  squared differences summed over the item ([10] / [23,3,3] / [1,3,3] rotation matrices)
 *   EHM_LOSS_POSE_6D_ORTHO   :386-388  per joint x = pose_6d.reshape(3, 2): sum of (x^T x - I_2)^2 over the 24 joints / 96
 *   EHM_LOSS_PENETRATION     :390-419  handed in: penetration [B] (NULL = 0)
 *   EHM_LOSS_KP3D_VIS_SUM    :358-372  selected ground-truth joints 0..23 projected with zero translation, focal [B,2], center [B,2]; visible = 0 <= u < 1920
 *                                      and 0 <= v < 1080; sum over the joints of (pelvis-aligned joint distance pred_keypoints_3d / keypoints_3d) * visible
 *                                      (a product: the NaN error of an invisible joint gives NaN, as in the reference)
 * per_item [B, EHM_LOSS_TERMS]: the contribution of each item; losses[k] = mean over B of per_item[:, k] (EHM_LOSS_KP3D_VIS_SUM: the sum), formed from the
 * float64 per-item sums and rounded once.  per_item_vis [B] int64 / joint_vis_num [1] int64: visible joints (:372); vis_mask [B,24] u8 (may be NULL).
 * Every input element is widened to float64 before the first subtraction, every sum runs in float64 in a fixed order (per-block partial sums in the
 * workspace, no atomics): results are bit-equal from run to run.  Vertex arrays must be 16-byte aligned.  gender [B] int64.
 * pred_joints >= 45: joints per item of the three pred_keypoints arrays; gt_joints / kp3d_points / kp3d_full_points >= 24, kp2d_points >= 25: points per
 * item of gt_joints_*, keypoints_3d, keypoints_3d_full, keypoints_2d.  workspace: *bytes of ehm_val_losses_workspace_bytes(B, V, &bytes), 8-byte aligned. */
enum {
  EHM_LOSS_TOTAL = 0, EHM_LOSS_V2V = 1, EHM_LOSS_KP3D = 2, EHM_LOSS_KP3D_FULL = 3, EHM_LOSS_KP2D_FULL = 4, EHM_LOSS_BETAS = 5, EHM_LOSS_BODY_POSE = 6,
  EHM_LOSS_GLOBAL_ORIENT = 7, EHM_LOSS_POSE_6D_ORTHO = 8, EHM_LOSS_PENETRATION = 9, EHM_LOSS_KP3D_VIS_SUM = 10, EHM_LOSS_TERMS = 11
};
typedef struct ehm_val_losses_desc {
  int B, V, pred_joints, gt_joints, kp3d_points, kp3d_full_points, kp2d_points;
  const float *pred_vertices, *pred_keypoints_3d, *pred_keypoints_3d_full, *pred_keypoints_2d_full; /* [B,V,3], [B,pred_joints,3] x 2, [B,pred_joints,2] */
  const float *pred_global_orient, *pred_body_pose, *pred_betas, *pred_pose_6d;                      /* [B,9], [B,207], [B,10], [B,144] */
  const float *keypoints_2d, *keypoints_3d, *keypoints_3d_full;                                     /* [B,kp2d_points,3], [B,kp3d_points,3], [B,kp3d_full_points,3] */
  const float *gt_vertices_male, *gt_vertices_female, *gt_joints_male, *gt_joints_female;           /* [B,V,3] x 2, [B,gt_joints,3] x 2 */
  const int64_t* gender;                                                                            /* [B] */
  const float *gt_global_orient, *gt_body_pose, *gt_betas;                                          /* [B,9], [B,207] rotation matrices, [B,10] */
  const float *focal, *center;                                                                      /* [B,2] each */
  const float* penetration;                                                                         /* [B] or NULL */
  double weights[9];
  void* workspace;
  int64_t workspace_bytes;
  float* losses;          /* [EHM_LOSS_TERMS] */
  int64_t* joint_vis_num; /* [1] */
  float* per_item;        /* [B, EHM_LOSS_TERMS] */
  int64_t* per_item_vis;  /* [B] */
  uint8_t* vis_mask;      /* [B,24] or NULL */
} ehm_val_losses_desc;
int ehm_val_losses_workspace_bytes(int B, int V, int64_t* bytes);
int ehm_val_losses(const ehm_val_losses_desc* d, void* stream);

/* The VJP of losses[EHM_LOSS_TOTAL] of ehm_val_losses with respect to the eight prediction arrays and the penetration term.  The input fields are those of
 * ehm_val_losses_desc (focal / center are kept for symmetry and never read; they may be NULL); gloss: device scalar, the cotangent of the total, NULL = 1 -
 * read on the device only.  Every g_* output may be NULL: it is then not computed (the vertex pass runs only for g_pred_vertices or g_pred_keypoints_3d).
 * A requested array is written in full - joints 24.. and the 2-D joints outside smpl_to_openpose get 0 - so the caller clears nothing.
 * With s_k = gloss weights[k] / B:
 *   V2V             d = (pv - pj0_c) - (gv - gj0_c) in float64 as the forward forms it; g_pv = s_0 / (3 V) sign(d); pelvis joint c: -s_0 / (3 V) sum_v sign(d)
 *   KP3D            joints 0..23, d as in the forward: +s_1 sign(d) to joint j, -s_1 sum_j sign(d) to joint 0
 *   KP3D_FULL       s_2 sign(pf - gf) on joints 0..23
 *   KP2D_FULL       at prediction joint smpl_to_openpose[j]: s_3 conf_j sign(p - g) per coordinate (conf of joints 1, 9, 12 is 0)
 *   BETAS / BODY_POSE / GLOBAL_ORIENT   2 s_k (pred - gt)
 *   POSE_6D_ORTHO   s_7 times the derivative of (m00^2 + m11^2 + 2 m01^2) / 96 per joint
 *   PENETRATION     g_penetration[b] = s_8;   KP3D_VIS_SUM is not part of the total: no gradient
 * sign(0) = 0 and sign(NaN) = NaN (torch.sign).  Everything that lands on one element - the pelvis joint's three sources included - is added in float64 in a
 * fixed order and rounded to float32 once; the vertex signs are summed as integers per block (workspace), no float atomics: two calls give the same bits.
 * pred_vertices, gt_vertices_* and g_pred_vertices must be 16-byte aligned.  workspace: *bytes of ehm_val_losses_backward_workspace_bytes, 4-byte aligned. */
typedef struct ehm_val_losses_bwd_desc {
  int B, V, pred_joints, gt_joints, kp3d_points, kp3d_full_points, kp2d_points;
  const float *pred_vertices, *pred_keypoints_3d, *pred_keypoints_3d_full, *pred_keypoints_2d_full;
  const float *pred_global_orient, *pred_body_pose, *pred_betas, *pred_pose_6d;
  const float *keypoints_2d, *keypoints_3d, *keypoints_3d_full;
  const float *gt_vertices_male, *gt_vertices_female, *gt_joints_male, *gt_joints_female;
  const int64_t* gender;
  const float *gt_global_orient, *gt_body_pose, *gt_betas;
  const float *focal, *center;
  const float* gloss;     /* [1] on the device, or NULL = 1 */
  double weights[9];
  void* workspace;
  int64_t workspace_bytes;
  float *g_pred_vertices, *g_pred_keypoints_3d, *g_pred_keypoints_3d_full, *g_pred_keypoints_2d_full; /* [B,V,3], [B,pred_joints,3] x 2, [B,pred_joints,2] */
  float *g_pred_global_orient, *g_pred_body_pose, *g_pred_betas, *g_pred_pose_6d;                      /* [B,9], [B,207], [B,10], [B,144] */
  float* g_penetration;                                                                               /* [B] */
} ehm_val_losses_bwd_desc;
int ehm_val_losses_backward_workspace_bytes(int B, int V, int64_t* bytes);
int ehm_val_losses_backward(const ehm_val_losses_bwd_desc* d, void* stream);

/* The point cap of the penetration term (egohmr.py:406-412): count [B] int32 = scene points of item b inside the bounding box of verts[b] (both ends
 * inclusive); scene_out [B,N,3] = scene, except that in an item with count > cap the points of index >= cap are moved out of every box (3e38) - the
 * reference's `inds[:, 4000:] = False`, not "the first 4000 selected".  ehm_collision_query on scene_out then gives the capped term. */
int ehm_scene_cap_points(const float* verts, const float* scene, float* scene_out, int32_t* count, int B, int V, int N, int cap, void* stream);

/* ------------------------------------------------------------------ whole sampling loop ------- */
/* One executed step of the loop (host-side table lookup already done, float32 like
 * _extract_into_tensor, gaussian_diffusion.py:794). */
typedef struct {
  float coef1, coef2, log_variance, variance; /* DDPM */
  float sqrt_recip_ac, sqrt_recipm1_ac, sqrt_ac_prev, dir_coef, sigma; /* DDIM */
  float nonzero;   /* 0 at respaced index 0 */
  float grad_scale; /* 0 = unguided step; p_sample_with_grad: cond_grad_weight*variance or cond_grad_weight*0.01 (gaussian_diffusion.py:378-385);
                       ddim_sample_with_grad (ddim = 1): float32 sqrt(1 - alpha_bar) on the last four respaced steps (:580-592, scale 1.0) */
} ehm_step_coefs;

typedef struct {
  int B;              /* bodies                                                     */
  int passes;         /* 2 = diffuse_fuse (conditional + image-masked pass), 1      */
  int num_steps;      /* executed steps T                                           */
  int ddim;           /* 0 = p_sample loop, 1 = ddim_sample loop (eta = 0)          */
  int lbs_every_step; /* 1 = decode the body every step like EgoHMR.forward does    */
  int num_scene_points; /* N (guidance only)                                        */
  float guide_denom;  /* B for COAP-style loss.mean(), 1 for VolSMPL-style sum()    */
  float tau;          /* collision proxy contact distance                          */
  int num_masked;     /* second passes after pruning = what ehm_gcn_set_pass_map was given; -1 = no map (B)   */
  int guide_all_points; /* 1 = VolSMPL-style guidance over ALL scene points (egohmr_volsmpl.py:609-612), 0 = bbox-selected (egohmr.py:550-552) */
  int lowprec_steps;  /* precision schedule: the FIRST lowprec_steps executed steps run the hidden convs on plain f16 operands
                         (ehm_gcn_set_precision mode 2), the remaining ones in the handle's mode; 0 = off.  docs/EXPERIMENTS.md 3.6  */
  int nonlocal_ci;    /* inter_channels of the non-local block set with ehm_gcn_set_nonlocal, 0 = none (needs float32 features:
                         handle mode 0 or 1 and lowprec_steps == 0)                                                              */
  int per_step_launches; /* 0 (default) = two launches per step: chained hidden convs, then step_fused_kernel (output responses + per-body
                         update + the next step's input conv); 1 = the separate launches of rounds 2-3 (input conv, chain, responses, per-body
                         step) - same bits, kept for A/B runs and the bit-equality tests                                                      */
  int twoterm_steps;  /* precision schedule, middle tier: executed steps [lowprec_steps, lowprec_steps + twoterm_steps) of a mode-1 loop run
                         the hidden convs as two-term products (ehm_gcn_set_precision mode 3: same X2 buffers, no format transition); 0 = off.
                         Needs handle mode 1 and no non-local block; lowprec_steps + twoterm_steps <= num_steps                               */
} ehm_sample_desc;

/* GaussianDiffusion.p_sample_loop / ddim_sample_loop (gaussian_diffusion.py:391-508, :618-718)
 * around EgoHMR.forward's per-step part (egohmr.py:232-278), everything step-invariant hoisted:
 *   steps [num_steps] HOST; tvecs [num_steps,2,hid] (timestep-embedding projection per step);
 *   noise [num_steps+1,B,144] (row 0 = x_T); scene [B,N,3] or NULL; betas [B,10];
 *   outputs: x_final [B,144], x0_final [B,144] (pred_x_start), verts [B,V,3], joints [B,45,3],
 *   R [B,24,3,3], pose6d [B,144] of the LAST step; trace (may be NULL) [num_steps,B,144] = x_t fed
 *   to each step.  workspace from ehm_sample_workspace_bytes(). */
int64_t ehm_sample_workspace_bytes(const ehm_sample_desc* d, int hid_dim, int num_verts);
int ehm_sample_loop(ehm_gcn* gcn, ehm_smpl* smpl, const ehm_sample_desc* d, const ehm_step_coefs* steps,
                    const float* h_img, const float* h_oth, const uint8_t* vis, const float* Wx, const float* tvecs,
                    const float* noise, const float* scene, const float* betas, const float* mean, const float* std,
                    float* x_final, float* x0_final, float* verts, float* joints, float* R, float* pose6d,
                    float* trace, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the denoiser's input feature on the training route of EgoHMR.forward and its VJP (csrc/train.hip; egohmr.py:190-191, :220-236, mask_cond :150-169).
 *   X [B,24,D], D = img_dim + n_other + 2 embed_dim, 16-byte aligned:
 *     X[b,j,:] = [ vis[b,j] keep_img[b] img_feats[b] | keep_oth[b] other[b] | x_feat[24 b + j] | temb[b] ]
 *   img_feats [B,img_dim]; vis [B,24] uint8; drop [B] uint8 or NULL (1 = the item's conditioning is dropped: keep_img = 1 - drop, keep_oth = 1 - drop or,
 *   with only_mask_img = 1, always 1); other [B,other_ld] of which the first n_other columns are read (the padded [scene | transl | cam] operand of the
 *   projections can be read in place); x_feat [24 B,embed_dim]; temb [B,embed_dim].  img_dim and embed_dim are multiples of 4, n_other is anything >= 1.
 *   The masks are products with 0.0f / 1.0f.
 * ehm_cond_assemble_backward: gX [B,24,D] -> g_img [B,img_dim] = keep_img sum_j vis gX, g_other [B,n_other] (contiguous) = keep_oth sum_j gX,
 *   g_x_feat [24 B,embed_dim] (16-byte aligned) = its columns of gX, g_temb [B,embed_dim] = sum_j gX.  An output that is NULL is not computed and its
 *   columns of gX are not read.  The sums over the joints run in index order in one thread (float32, no atomics): a call repeats bit for bit. */
int ehm_cond_assemble(const float* img_feats, const uint8_t* vis, const uint8_t* drop, const float* other, int other_ld, int n_other,
                      const float* x_feat, const float* temb, int only_mask_img, float* X, int B, int img_dim, int embed_dim, void* stream);
int ehm_cond_assemble_backward(const float* gX, const uint8_t* vis, const uint8_t* drop, int n_other, int only_mask_img, float* g_img, float* g_other,
                               float* g_x_feat, float* g_temb, int B, int img_dim, int embed_dim, void* stream);

/* ---- measurement aid (bench.py's roofline objects; SURVEY.md 8d asks for per-kernel figures).  No reference counterpart.
 * Between ehm_profile_begin() and ehm_profile_end() every launch of ehm_sample_loop is bracketed by a pair of HIP events ON THE
 * LAUNCH STREAM, tagged with its class; ehm_profile_end waits for them and adds the elapsed times up per class
 * (ms[c] = sum of (stop - start), launches[c] = pairs), c < n <= EHM_PROF_N.  The event pairs serialise nothing that is not
 * already serial (the loop is one dependency chain), but they cost a few microseconds each: never inside a timed region.
 * Not thread-safe, one profile at a time. */
enum {
  EHM_PROF_INPUT = 0,        /* gcn_input_kernel (only the first step when the skinning launch carries it)              */
  EHM_PROF_CHAIN_F16X3 = 1,  /* gcn_hidden_chain_kernel<3, 4>: the 8 hidden convs of a step, split-f16                   */
  EHM_PROF_CHAIN_F16 = 2,    /* gcn_hidden_chain_kernel<1, 8>: the same on plain f16 operands                            */
  EHM_PROF_HIDDEN_F32 = 3,   /* gcn_hidden_kernel x 8 (f32-input MFMA) or per-conv tile launches                         */
  EHM_PROF_OUT_DOT = 4,      /* gcn_out_dot_kernel                                                                       */
  EHM_PROF_STEP_BODY = 5,    /* step_body_kernel; with the fused step launches: pose_steps_kernel (the pending steps' poses, per flush) */
  EHM_PROF_SKIN_INPUT = 6,   /* skin_input_kernel (skinning of step t + input conv of step t+1) / skin_mfma_kernel       */
  EHM_PROF_GUIDANCE = 7,     /* the collision-guidance kernel sequence of a guided step                                  */
  EHM_PROF_RESERVED_8 = 8,   /* (was the one-launch loop experiment's class; kept so that the indices behind it do not move)           */
  EHM_PROF_RESERVED_9 = 9,
  EHM_PROF_G_NEAREST = 10,   /* inside EHM_PROF_GUIDANCE: bbox + select + nearest_grid_kernel (the collision proxy's search) */
  EHM_PROF_G_SKIN_BWD = 11,  /* inside EHM_PROF_GUIDANCE: skin_bwd_kernel (VJP of the skinning)                          */
  EHM_PROF_G_POSEFEAT_BWD = 12, /* inside EHM_PROF_GUIDANCE: posefeat_bwd_kernel ([B, 20670] x [20670, 207] contraction) */
  EHM_PROF_STEP_FUSED = 13,  /* step_fused_kernel: a step's output responses + per-body update + the NEXT step's input conv, one block per body */
  EHM_PROF_G_NEAREST_EVALS = 14, /* not a launch class: launches[14] = point-to-vertex distance evaluations of nearest_grid_kernel while the profile was open (ms[14] = 0) */
  EHM_PROF_CHAIN_F16X2 = 15, /* gcn_hidden_chain_kernel<2, 4>: the 8 hidden convs of a two-term step (ehm_sample_desc.twoterm_steps)                */
  EHM_PROF_N = 16
};
int ehm_profile_begin(void);
int ehm_profile_end(double* ms, int64_t* launches, int n);

#ifdef __cplusplus
}
#endif
#endif /* EGOHMR_HIP_H */
