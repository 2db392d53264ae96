/*
 * waldo_hip.h -- C ABI of the MI355X (gfx950) WIF warp/composite hot path.
 *
 * Drop-in boundary for the operator layer of 16lemoing/waldo that the hot path lives in
 * (reference files cited per entry point; paths relative to the reference root).  Every entry
 * point is a stream-ordered launcher:
 *   - plain pointers and sizes only (no torch types); all tensors are fp32, contiguous, in the
 *     layout stated below; index tensors are int32/int64 as stated;
 *   - the CALLER owns and allocates every buffer (inputs, outputs, workspaces); the library never
 *     allocates or frees device memory and never synchronises;
 *   - kernels are launched on `stream` (a hipStream_t passed as void*) of the CURRENT device;
 *   - returns 0 on success, a negative WALDO_E* code otherwise; no C++ exception crosses the ABI;
 *     waldo_last_error_string() gives the message of the last failure on the calling thread;
 *   - re-entrant: no global mutable state except the thread-local error string and ONE piece of
 *     process-global state, the debug options of waldo_set_debug_option below (three test-only
 *     switches between kernel variants that compute the same thing; all off unless a test
 *     switches one on; a caller that never calls it has a stateless library).
 *
 * Build: hipcc --offload-arch=gfx950 -shared -fPIC (see waldo_amd/build.py).
 */
#ifndef WALDO_HIP_H
#define WALDO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WALDO_OK 0
#define WALDO_EINVAL (-1)  /* bad shape / null pointer / unsupported size */
#define WALDO_ELAUNCH (-2) /* hipLaunch / runtime error */

typedef void* waldo_stream_t; /* hipStream_t */

/* Element type of a retyped buffer of the *_dt entry points (the 16-bit WIF path).  The arithmetic stays fp32; a
 * 16-bit result is the fp32 result rounded to nearest-even (the bits of torch's `.to(dtype)`), a 16-bit input is
 * widened to fp32 on load.  Any other code: WALDO_EINVAL with a message, before any launch. */
enum waldo_dtype { WALDO_DTYPE_F32 = 0, WALDO_DTYPE_F16 = 1, WALDO_DTYPE_BF16 = 2 };

/* Packed clip (waldo_amd.functional.PackedClip).  The clip that A9 / A10 read, (B,T,3+Nl,Hd,Wd) fp32 = three RGB planes
 * and Nl layout-logit planes, stored as (B,T,Hd,Wd) pixels of 4 bytes [R, G, B, class id] (uint8, 16-byte aligned
 * base for the staged frame warp).  Its UNPACKED form -- what every *_packed entry point computes with, bit for bit:
 *   channel c < 3:  rgb_table[byte c], rgb_table = 256 fp32 values owned by the caller (read_rgb's (u8/255 - 0.5)/0.5);
 *   channel 3 + n:  +5.0f where class id == n, -5.0f elsewhere (a class id >= Nl: -5 in every layout channel).
 * Nl <= 32, the fused path's class limit.  The packed entry points produce what their fp32 twins produce on the
 * unpacked clip (waldo_unpack_clip_fwd), bit for bit; the clip carries no gradient (no packed backward). */
int waldo_unpack_clip_fwd(const uint8_t* clip, const float* rgb_table, float* out, int B, int T, int Nl, int Hd, int Wd,
                          waldo_stream_t stream); /* out (B,T,3+Nl,Hd,Wd); 0 <= Nl <= 32 */

/* ABI version: major*1000 + minor. */
int waldo_version(void);
const char* waldo_last_error_string(void);
/* Largest layer count L the fused composite kernels accept. */
int waldo_max_layers(void);

/* Test-only switches between kernel variants that compute the same thing (A/B parity tests of the
 * fast paths against the plain ones).  THE ONE PIECE OF PROCESS-GLOBAL STATE of the library: process-wide,
 * off by default, relaxed atomics; nothing reads the environment.  Kernel variants that were measured and
 * rejected are NOT in the library, nor in its sources: DESIGN.md records them and where git history keeps them. */
#define WALDO_DEBUG_FWD_PLAIN 0   /* fused forward: gather kernel instead of the LDS-staged one */
#define WALDO_DEBUG_IW_PASSES 1   /* grid inversion: one kernel per fill / erosion pass */
#define WALDO_DEBUG_BWD_GENERIC 2 /* fused backward: the generic per-tap-atomics kernel for every shape
                                     (waldo_warp_composite_bwd_workspace_bytes answers 0) */
#define WALDO_DEBUG_COUNT 3
int waldo_set_debug_option(int option, int value);

/* Frame-index status.  The reference's gather_time (models/nets/lvd.py:462-467: `tensor.gather(1, ts)`) RAISES for
 * a frame index outside the time axis.  The forward entry points that index frames with ctx_ts / pred_ts from
 * device memory (waldo_time_gather_fwd, waldo_flow_ctx_warp_fwd / _raw_fwd, waldo_frame_warp_fuse_fwd / _raw_fwd)
 * take `status`: WALDO_INDEX_STATUS_WORDS int32 words owned by the caller (zero them once), device-accessible --
 * device memory, or pinned host memory through waldo_host_device_pointer, which the caller can read WITHOUT
 * synchronising the device.  A kernel that meets an index outside its range clamps it (memory safety) and reports:
 *   status[0] = the limit a ctx_ts entry violated (valid: 0 .. limit-1; never 0), status[1] = an offending value,
 *   status[2], status[3] likewise for pred_ts.
 * The words are STICKY (kernels only ever write non-zero limits); the caller checks and clears them when it
 * chooses -- after a synchronisation for the reference's raise-at-once behaviour, or lazily (a captured HIP graph:
 * after a replay).  status == NULL: out-of-range indices are clamped silently.  The backward entry points read the
 * indices the forward saw and clamp only. */
#define WALDO_INDEX_STATUS_WORDS 4
/* Device pointer of a pinned (page-locked, mapped) host allocation, hipHostGetDevicePointer: WALDO_EINVAL when
 * `host` is not such memory -- so that a status word in host memory fails at set-up, not as a fault in a kernel. */
int waldo_host_device_pointer(void* host, void** device);

/* ---------------------------------------------------------------------------------------
 * A2. Thin-plate-spline grid synthesis -- replaces TPSWarp.forward
 *     (models/modules/warp.py:49-55).  K3 = N + 3.
 *   mapping[b] = inverse_kernel (K3,K3) @ [src_pts[b] (N,2); 0 (3,2)]          (warp.py:52-53)
 *   grid[b,p]  = sum_k basis_t[k,p] * mapping[b,k]                              (warp.py:54)
 * basis_t is the reference buffer `tgt_grid_repr` (HW,K3) stored TRANSPOSED as (K3,HW) so that
 * a wavefront reads 64 consecutive pixels of one basis function in one coalesced request.
 * ------------------------------------------------------------------------------------- */
int waldo_tps_mapping_fwd(const float* inverse_kernel, const float* src_pts, float* mapping,
                          int64_t B, int N, waldo_stream_t stream);
/* grad_src_pts[b,n] = sum_r inverse_kernel[r,n] * grad_mapping[b,r]  (rows n < N only) */
int waldo_tps_mapping_bwd(const float* inverse_kernel, const float* grad_mapping,
                          float* grad_src_pts, int64_t B, int N, waldo_stream_t stream);
/* grid (B,HW,2) */
int waldo_tps_grid_fwd(const float* basis_t, const float* mapping, float* grid, int64_t B,
                       int64_t HW, int K3, waldo_stream_t stream);
/* grad_mapping (B,K3,2) is OVERWRITTEN (the launcher zero-fills it on `stream` first). */
int waldo_tps_grid_bwd(const float* basis_t, const float* grad_grid, float* grad_mapping,
                       int64_t B, int64_t HW, int K3, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A3. Grid inversion by forward splat + hole filling -- replaces InverseWarp.forward
 *     (models/modules/warp.py:71-174; pad == True) and its autograd.
 *   src_grid (B,Hs,Ws,2) layer->image grid;  src_id (Hs,Ws,2), tgt_id (H,W,2) the identity grids
 *   (reference buffers `src_grid`, `tgt_grid`);  gauss (ksize*ksize) the reference buffer `kernel`, ksize = the
 *   module's `kernel_size`: odd, 1 ... 15 (3 in every script: one launch; other sizes run the fill passes one by one);
 *   out (B,H,W,2) image->layer grid.  Hp = H + 2*(niter+1), Wp likewise.
 * Among several samples landing on one cell the lowest sample index wins (the reference's answer
 * under a stable sort; its own tie-break is implementation-defined).
 * Work / saved buffers, all caller-allocated, contents irrelevant on entry:
 *   dxy (B,2,H*W) f32, cell (B,H*W) i32, winner (B,H*W) i32, field_a / field_b (B,2,Hp*Wp) f32,
 *   fill_iter (B,Hp*Wp) u8, denom (B,Hp*Wp) f32, mask_a / mask_b (B,Hp*Wp) u8.
 * The backward needs cell, winner, fill_iter, denom and mask_a (final mask) as the forward left
 * them, plus gfield (B,2,Hp*Wp) f32 scratch; grad_src_grid (B,Hs,Ws,2) is overwritten.
 * ------------------------------------------------------------------------------------- */
int waldo_inverse_warp_fwd(const float* src_grid, const float* src_id, const float* tgt_id,
                           const float* gauss, float* out, float* dxy, int* cell, int* winner,
                           float* field_a, float* field_b, unsigned char* fill_iter, float* denom,
                           unsigned char* mask_a, unsigned char* mask_b, int64_t B, int Hs, int Ws,
                           int H, int W, int niter, int erode, int ksize, waldo_stream_t stream);
/* The same with the tie-break order given (InverseWarp with num_perm > 1, warp.py:91-111, one
 * call per permutation; the results are averaged by the caller -- the fill, the erosion and the
 * final grid are linear in the elected field for a fixed set of occupied cells, and that set does
 * not depend on the order):  order (H*W) i32 a permutation of the samples (one row of the
 * reference buffer `perm`), rank (H*W) i32 its inverse.  Among the samples landing on one cell
 * the one standing first in `order` wins.  waldo_inverse_warp_bwd serves both. */
int waldo_inverse_warp_order_fwd(const float* src_grid, const float* src_id, const float* tgt_id,
                                 const float* gauss, const int* rank, const int* order,
                                 float* out, float* dxy, int* cell, int* winner, float* field_a,
                                 float* field_b, unsigned char* fill_iter, float* denom,
                                 unsigned char* mask_a, unsigned char* mask_b, int64_t B, int Hs,
                                 int Ws, int H, int W, int niter, int erode, int ksize, waldo_stream_t stream);
int waldo_inverse_warp_bwd(const float* grad_out, const float* gauss, const int* cell,
                           const int* winner, const unsigned char* fill_iter, const float* denom,
                           const unsigned char* mask, float* gfield, float* grad_src_grid,
                           int64_t B, int Hs, int Ws, int H, int W, int niter, int ksize,
                           waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A4/A5. Bilinear backward warp -- replaces F.grid_sample(x + delta, grid) - delta with the
 *     defaults (bilinear, zeros, align_corners=False) as used by Warper.obj_to_output /
 *     bg_to_output / obj_from_input / bg_from_input (models/nets/lvd.py:502-559).
 *   input (Nin,C,Hi,Wi), grid (N,Ho,Wo,2), output (N,C,Ho,Wo).
 *   Input batch broadcast (the reference's .expand over T, lvd.py:544,555):
 *       n_in = (n / outer_div) * inner + (n % inner);  pass outer_div = inner = N for identity.
 *   Forward only: the same map for the GRID, n_grid = (n / grid_outer_div) * grid_inner + n % grid_inner,
 *       grid (N_grid,Ho,Wo,2) -- the predicted frames' grids repeated over the Tc contexts
 *       (`[:, pred_ts].unsqueeze(1).expand(-1, Tc, ...)`, lvd.py:665-668) without the Tc copies;
 *       grid_outer_div = grid_inner = N for one grid per output.
 * ------------------------------------------------------------------------------------- */
int waldo_grid_sample2d_fwd(const float* input, const float* grid, float* output, int64_t N,
                            int C, int Hi, int Wi, int Ho, int Wo, float delta,
                            int64_t outer_div, int64_t inner, int64_t grid_outer_div,
                            int64_t grid_inner, waldo_stream_t stream);
/* The same with two extras for Warper.grid_to_flow_ctx (models/nets/lvd.py:785-796), where the reference warps an
 * all-ones canvas, then the object flows and the background flow with the same grids, and concatenates the results:
 *   mask_out (N,1,Ho,Wo) or NULL: the sample of an ALL-ONES image at the same grid -- what Warper.obj_to_output(ones,
 *     grid) returns and the ghost test thresholds at 0.9 (lvd.py:785-791) -- a by-product of the taps (one store
 *     instead of a launch of its own over B*Tc*Tp*No maps);
 *   out_group / out_stride / out_offset: output map n is written to slot (n / out_group) * out_stride + out_offset +
 *     n % out_group of an output tensor of (slots, C, Ho, Wo) maps ((N, N, 0): the plain output).  With (1, L, 0) for
 *     the background and (No, L, 1) for the objects the two calls of Warper.layer_to_output (lvd.py:533-537) write
 *     straight into the (frames, L, C, Ho, Wo) tensor its torch.cat would build;
 *   pre_scale / pre_bias: the image sampled is pre_scale * input + pre_bias -- Warper.grid_to_flow[_ctx] warps
 *     `(obj_alpha + 1) / 2` and `(bg_alpha + 1) / 2` (lvd.py:602-606, 716-720): (0.5, 0.5) warps them without the
 *     two images being written first.  (1, 0): the plain call. */
int waldo_grid_sample2d_ex_fwd(const float* input, const float* grid, float* output, float* mask_out,
                               int64_t N, int C, int Hi, int Wi, int Ho, int Wo, float delta,
                               int64_t outer_div, int64_t inner, int64_t grid_outer_div, int64_t grid_inner,
                               int64_t out_group, int64_t out_stride, int64_t out_offset, float pre_scale,
                               float pre_bias, waldo_stream_t stream);
/* grad_input (Nin,C,Hi,Wi) must be ZERO-FILLED by the caller (accumulated with atomics; may be
 * NULL to skip); grad_grid (N,Ho,Wo,2) is overwritten (may be NULL to skip).  The float atomics make the last bits of
 * grad_input depend on the order of arrival; waldo_grid_sample2d_bwd_det ("Reproducible gradients" below) OVERWRITES
 * it with a sum that does not. */
int waldo_grid_sample2d_bwd(const float* input, const float* grid, const float* grad_output,
                            float* grad_input, float* grad_grid, int64_t N, int C, int Hi, int Wi,
                            int Ho, int Wo, float delta, int64_t outer_div, int64_t inner,
                            waldo_stream_t stream);
/* The backward of a waldo_grid_sample2d_ex_fwd call (one grid per output map): grad_output is the gradient of the
 * WHOLE (slots, C, Ho, Wo) tensor the forward wrote into, and map n reads slot (n / gout_group) * gout_stride +
 * gout_offset + n % gout_group of it -- the backward of Warper.layer_to_output's torch.cat (lvd.py:533-537) without
 * the two slices of the gradient being copied out first; pre_scale / pre_bias as in the forward (grad_input is the
 * gradient of `input`, not of the scaled image). */
int waldo_grid_sample2d_ex_bwd(const float* input, const float* grid, const float* grad_output,
                               float* grad_input, float* grad_grid, int64_t N, int C, int Hi, int Wi,
                               int Ho, int Wo, float delta, int64_t outer_div, int64_t inner,
                               int64_t gout_group, int64_t gout_stride, int64_t gout_offset, float pre_scale,
                               float pre_bias, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A6. Occlusion product / soft-alpha composite -- replaces the
 *     (1 - alpha * occ).prod(dim) * alpha pattern of models/nets/lvd.py:651-652,686,764-765,809
 *     (spec form LVD.reduce_comp, lvd.py:100-114).
 *   alpha (M,L,HW) in [0,1], occ (Mo,L,L) with m_occ = m / occ_div (broadcast of occ over a
 *   trailing group, e.g. Tc), out (M,L,HW):  out[m,j,p] = alpha[m,j,p] * prod_i (1 - alpha[m,i,p]*occ[m_occ,i,j])
 * ------------------------------------------------------------------------------------- */
int waldo_occ_composite_fwd(const float* alpha, const float* occ, float* out, int64_t M, int L,
                            int64_t HW, int64_t occ_div, waldo_stream_t stream);
/* grad_alpha (M,L,HW) overwritten; grad_occ (Mo,L,L) must be ZERO-FILLED by the caller
 * (accumulated with atomics; may be NULL to skip).  Order-independent and OVERWRITTEN instead:
 * waldo_occ_composite_bwd_det ("Reproducible gradients" below). */
int waldo_occ_composite_bwd(const float* alpha, const float* occ, const float* grad_out,
                            float* grad_alpha, float* grad_occ, int64_t M, int L, int64_t HW,
                            int64_t occ_div, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * f2. Producers of the path's inputs: the steps between the networks and the warp kernels.
 *
 * waldo_compute_occ_*: LVD.compute_occ (models/nets/lvd.py:59-68).
 *   score (M,No) -> occ (M,No+1,No+1):  s = exp(-score^2) + eps;
 *   occ[i+1][j+1] = s_i / (s_i + s_j) - [i == j] / 2;  occ[i+1][0] = 1;  occ[0][*] = 0.
 *   Backward: grad_score (M,No) is OVERWRITTEN.
 * waldo_alpha_head_*: ImageDecoder.forward's tail (lvd.py:245-254) + the alpha arithmetic of
 *   LVD.forward(mode="estimate_alpha_grid_occ") (lvd.py:128-132) in one pass.
 *   x (N,C,h,w) the decoder's raw image;  y = x + bias;  on the LAST channel when has_alpha:
 *   y = tanh(y), then y = prior + (1 - prior) * y with prior (h,w) (the `circle` buffer; NULL:
 *   no prior);  out (N,C,h*scale,w*scale) = F.interpolate(y, scale_factor=scale, "bilinear",
 *   align_corners=False);  then mode 1 (remove_obj): out = -1, mode 2 (freeze_obj): out = +1;
 *   then with mask (h*scale,w*scale) (the `obj_alpha_mask` buffer; NULL: none):
 *   out = mask * out - (1 - mask).   mode != 0 and mask act on the ONE-channel object alpha of
 *   lvd.py:128-132: with C > 1 either of them is refused (WALDO_EINVAL).
 *   Backward: grad_x (N,C,h,w) is OVERWRITTEN (gathered: no atomics).
 * waldo_pose_affine_*: the pose heads' affine (models/nets/flp.py:259-273, lvd.py:440-449).
 *   pose (R,6+2P) (after tanh / + last);  T = (mul6 * pose[:6] + bias6) as (3,2);
 *   pts[p] = pts_mul * base_pts[p] + mul_delta * pose[6+2p : 8+2p];  out (R,P,2) = [pts, 1] @ T.
 *   Backward: grad_pose (R,6+2P) is OVERWRITTEN.
 * ------------------------------------------------------------------------------------- */
int waldo_compute_occ_fwd(const float* score, float* occ, int64_t M, int No, float eps,
                          waldo_stream_t stream);
int waldo_compute_occ_bwd(const float* score, const float* grad_occ, float* grad_score, int64_t M,
                          int No, float eps, waldo_stream_t stream);
int waldo_alpha_head_fwd(const float* x, const float* prior, const float* mask, float* out,
                         int64_t N, int C, int h, int w, int scale, float bias, int has_alpha,
                         int mode, waldo_stream_t stream);
int waldo_alpha_head_bwd(const float* x, const float* prior, const float* mask,
                         const float* grad_out, float* grad_x, int64_t N, int C, int h, int w,
                         int scale, float bias, int has_alpha, int mode, waldo_stream_t stream);
int waldo_pose_affine_fwd(const float* pose, const float* mul6, const float* bias6,
                          const float* base_pts, float* out, int64_t R, int P, float mul_delta,
                          float pts_mul, waldo_stream_t stream);
int waldo_pose_affine_bwd(const float* pose, const float* mul6, const float* bias6,
                          const float* base_pts, const float* grad_out, float* grad_pose, int64_t R,
                          int P, float mul_delta, float pts_mul, waldo_stream_t stream);
/* waldo_disocc_test_fwd: the disocclusion test of Synthesizer.predict (models/synthesizer.py:447-450, 475-478)
 *   on layer_max (B,Tc,Tp,HW) = alpha_ctx.max(dim=3)[0] (the `alpha_max` by-product of waldo_flow_ctx_warp_*):
 *   dmax = max over Tc, dmin = min over Tc (NaN-propagating, as torch's);  out (B,Tp,HW) = dmax, 0 where
 *   dmax - dmin > 1.  Inference only (the reference runs it under no_grad). */
int waldo_disocc_test_fwd(const float* layer_max, float* out, int64_t B, int Tc, int Tp, int64_t HW,
                          waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A9: the two full-resolution passes of Warper.grid_to_flow_ctx / grid_to_flow
 * (models/nets/lvd.py:707-828, 602-705); their backward entry points follow A10.  The low-resolution
 * inputs come from waldo_grid_sample2d_fwd (lvd.py:723-728, 784-796); Hd = H*scale, Wd = W*scale.
 *
 * waldo_flow_ctx_alpha_fwd (lvd.py:731-766): bilinear x`scale` upsampling (F.interpolate,
 * align_corners=False) of the rough alphas, layout filter, occlusion product.
 *   alpha_lr (B*Tw,L,H,W) in [0,1]   rough alpha of every layer in image space, frames 0..Tw-1
 *   input    (B,T,C,Hd,Wd)           layout logits in channels [chan_off, chan_off+Nl) (lvd.py:731)
 *   dist     (B,L-1,Nl) or NULL      class distribution of every object (NULL: no filter)
 *   occ      (B,T,L,L)               occlusion order (LVD.compute_occ)
 *   a01      (B*Tw,L,Hd,Wd)          out: a'_j = a_j prod_i (1 - a_i occ[i][j]) in [0,1]
 *   alpha_out same shape or NULL     out: 2a' - 1 (the method's `alpha` / `alpha_unflt`)
 * waldo_flow_ctx_warp_fwd (lvd.py:784-818), M = B*Tc*Tp:
 *   flow_lr  (M,L,2,H,W)             per-layer flow warped to image space (low resolution)
 *   isobj_lr (M,L-1,H,W) or NULL     warped ones of the objects (ghost mask, `allow_ghost` = NULL)
 *   a01      (B*Tw,L,Hd,Wd)          from waldo_flow_ctx_alpha_fwd
 *   ctx_ts   (B,Tc,Tp) int64, pred_ts (Tp) int64, occ (B,T,L,L)
 *   flow (M,2,Hd,Wd), alpha_ctx (M,L,Hd,Wd) in [-1,1], disocc (M,Hd,Wd)      outputs
 * ------------------------------------------------------------------------------------- */
/* layer_bits, optional (NULL to skip), (B*Tw, Hd, ceil(Wd / 64)) uint32: bit l of word (n, y, s) is set when a01 of
 * layer l is non-zero (or NaN) somewhere in columns [64 s, 64 s + 64) of row y of frame n -- the first pass's map of
 * where each layer IS, for the second pass on the path that has no ghost mask (Warper.grid_to_flow, lvd.py:602-705):
 * waldo_flow_ctx_warp_* skip, per tile, the layers that are absent from every segment the tile's samples can reach. */
int waldo_flow_ctx_alpha_fwd(const float* alpha_lr, const float* input, const float* dist,
                             const float* occ, float* a01, float* alpha_out, unsigned* layer_bits, int B, int T,
                             int Tw, int L, int Nl, int C, int chan_off, int H, int W, int scale,
                             waldo_stream_t stream);
/* The same on a packed clip (B,T,Hd,Wd) ("Packed clip" above) in place of `input`: the layout logits of a pixel are the
 * +-5 of its class byte, fed to the same softmax.  1 <= Nl <= 32; `clip` is required. */
int waldo_flow_ctx_alpha_packed_fwd(const float* alpha_lr, const uint8_t* clip, const float* dist, const float* occ,
                                    float* a01, float* alpha_out, unsigned* layer_bits, int B, int T, int Tw, int L,
                                    int Nl, int H, int W, int scale, waldo_stream_t stream);
/* alpha_max (M,Hd,Wd), optional (NULL to skip): max over the layers of alpha_ctx -- what
 * Synthesizer.predict's disocclusion test takes from it (models/synthesizer.py:447, `alpha_ctx.max(dim=3)[0]`:
 * a pass over the largest tensor but one of the pipeline, here a by-product of writing it). */
/* ctx_ts must lie in [0, Tw), pred_ts in [0, T): violations are reported in `status` ("Frame-index status" above).
 * layer_bits, optional: waldo_flow_ctx_alpha_fwd's by-product for the SAME a01 (NULL: every layer is sampled in every
 * pixel unless the ghost mask excludes it).  The values do not depend on it. */
int waldo_flow_ctx_warp_fwd(const float* flow_lr, const float* isobj_lr, const float* a01,
                            const int64_t* ctx_ts, const int64_t* pred_ts, const float* occ,
                            float* flow, float* alpha_ctx, float* disocc, float* alpha_max,
                            const unsigned* layer_bits, int* status, int B, int T, int Tw, int Tc, int Tp, int L,
                            int H, int W, int scale, waldo_stream_t stream);
/* The same pass for a caller that runs waldo_frame_warp_fuse_raw_fwd next (LVD.forward(mode="decode_output"),
 * lvd.py:141-153, without autograd): the composited context alphas are written straight into the slots they
 * occupy in A10's `raw` tensor, raw[b, tp, tc, C + l] (lvd.py:846: `raw_output = cat(output, alpha)`), instead of
 * into a tensor of their own that the frame warp would read and copy there (L planes read + L written per
 * (b, tc, tp) and full-resolution pixel: 29 % of that kernel's traffic at the Cityscapes recipe), and
 *   score (M,Hd,Wd) = sum_l (alpha_ctx_l + 1) / 2   (lvd.py:841), summed in layer order from the stored values,
 * comes out beside them.  raw (B,Tp,Tc',C+L,Hd,Wd) as A10 lays it out, Tc' = Tc or Tc + 1; only the alpha slots
 * of contexts 0 .. Tc-1 are written.  The reference's alpha_ctx (B,Tc,Tp,L,Hd,Wd) is a strided view of raw. */
int waldo_flow_ctx_warp_raw_fwd(const float* flow_lr, const float* isobj_lr, const float* a01,
                                const int64_t* ctx_ts, const int64_t* pred_ts, const float* occ, float* flow,
                                float* raw, float* score, float* disocc, float* alpha_max,
                                const unsigned* layer_bits, int* status, int B, int T, int Tw, int Tc, int Tp, int L,
                                int H, int W, int scale, int C, int Tcx, waldo_stream_t stream);
/* The same with `raw` of element type raw_dtype (enum waldo_dtype): a 16-bit raw gets the alpha slots rounded to
 * nearest-even; flow, score, disocc and alpha_max stay fp32 (score is summed from the fp32 values, so nothing reads
 * the rounded alphas back).  WALDO_DTYPE_F32 = waldo_flow_ctx_warp_raw_fwd. */
int waldo_flow_ctx_warp_raw_fwd_dt(const float* flow_lr, const float* isobj_lr, const float* a01,
                                   const int64_t* ctx_ts, const int64_t* pred_ts, const float* occ, float* flow,
                                   void* raw, float* score, float* disocc, float* alpha_max,
                                   const unsigned* layer_bits, int* status, int B, int T, int Tw, int Tc, int Tp,
                                   int L, int H, int W, int scale, int C, int Tcx, int raw_dtype,
                                   waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A10: Warper.input_to_output (models/nets/lvd.py:830-853): warp of the context frames
 * by the composited flow and temporal fusion, incl. the include_self branch (lvd.py:842-845).
 *   input (B,T,C,Hd,Wd); flow (B,Tc,Tp,2,Hd,Wd); alpha (B,Tc,Tp,L,Hd,Wd) in [-1,1];
 *   ctx_ts (B,Tc,Tp) int64; Tc' = Tc + (include_self ? 1 : 0) <= 8; include_self needs Tp == T
 *   out (B,Tp,C+1,Hd,Wd)  fused frames, last channel = fused (2 score - 1)
 *   raw (B,Tp,Tc',C+L,Hd,Wd)  per-context warped frames and alphas (the WIF input, wif.py:21), stored
 *                             with the PREDICTED frame ahead of the context: the reference's
 *                             (B,Tc',Tp,...) tensor is the view raw.permute(0,2,1,3,4,5) (strides, no
 *                             copy), and WIF.forward's own permute + contiguous (wif.py:39) -- a copy of
 *                             the largest tensor of the pipeline -- finds it already in place
 * ctx_ts must lie in [0, T): violations are reported in `status` ("Frame-index status" above).
 * Any Wd >= 2 and any alignment give the same bits; with Wd % 4 == 0, a 16-byte aligned `input` and Tc <= 4 the
 * contexts' footprints are staged in LDS (16-byte loads) instead of gathered tap by tap.
 * ------------------------------------------------------------------------------------- */
int waldo_frame_warp_fuse_fwd(const float* input, const float* flow, const float* alpha,
                              const int64_t* ctx_ts, float* out, float* raw, int* status, int B, int T, int Tc,
                              int Tp, int C, int L, int Hd, int Wd, int include_self, float eps,
                              waldo_stream_t stream);
/* A10 behind waldo_flow_ctx_warp_raw_fwd: the alpha slots of `raw` are filled already and `score` (B,Tc,Tp,Hd,Wd)
 * holds their per-context sums; this call reads one score plane per context instead of L alpha planes, writes the C
 * warped channels of every context (and, with include_self, the whole self slot) and `out`.  Same values, bit
 * for bit, as waldo_frame_warp_fuse_fwd on the contiguous alpha tensor. */
int waldo_frame_warp_fuse_raw_fwd(const float* input, const float* flow, const float* score,
                                  const int64_t* ctx_ts, float* out, float* raw, int* status, int B, int T, int Tc,
                                  int Tp, int C, int L, int Hd, int Wd, int include_self, float eps,
                                  waldo_stream_t stream);
/* The same with `raw` of element type raw_dtype (the type waldo_flow_ctx_warp_raw_fwd_dt filled it in): a 16-bit raw
 * gets the warped channels (and the self slot) rounded to nearest-even; `out` stays fp32 and has the fp32 call's bits. */
int waldo_frame_warp_fuse_raw_fwd_dt(const float* input, const float* flow, const float* score,
                                     const int64_t* ctx_ts, float* out, void* raw, int* status, int B, int T, int Tc,
                                     int Tp, int C, int L, int Hd, int Wd, int include_self, float eps, int raw_dtype,
                                     waldo_stream_t stream);
/* The same on a packed clip (B,T,Hd,Wd) ("Packed clip" above) in place of `input`, C = 3 + Nl channels, 0 <= Nl <= 32;
 * the self slot (include_self) is the unpacked frame.  Every form of the fp32 call (the staged boxes with Wd % 4 == 0,
 * a 16-byte aligned clip and Tc <= 4 -- each box staged ONCE for all channels --, the per-context gathers, the plain
 * kernel) with the bits of waldo_frame_warp_fuse_raw_fwd_dt on the unpacked clip. */
int waldo_frame_warp_fuse_raw_packed_fwd(const uint8_t* clip, const float* rgb_table, const float* flow,
                                         const float* score, const int64_t* ctx_ts, float* out, void* raw, int* status,
                                         int B, int T, int Tc, int Tp, int Nl, int L, int Hd, int Wd, int include_self,
                                         float eps, int raw_dtype, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Backward of A9 / A10 (csrc/flow_ctx_bwd.hip): the reference's live backward path in LVD training
 * (models/synthesizer.py:841 through models/nets/lvd.py:602-853).  Shapes as the forward entry points.
 *
 * waldo_flow_ctx_alpha_bwd:  grad_a01, grad_alpha_out (B*Tw,L,Hd,Wd) = d loss / d a01 and d loss / d alpha_out, the
 *   two outputs of the forward (alpha_out = 2 a01 - 1: the kernel reads grad_a01 + 2 grad_alpha_out; either may be
 *   NULL = zero, not both);  grad_alpha_lr (B*Tw,L,H,W) OVERWRITTEN;
 *   grad_dist (B,L-1,Nl) and grad_occ (B,T,L,L) must be ZERO-FILLED (one float atomic per workgroup
 *   and entry; either may be NULL);  workspace: B*Tw*L*Hd*Wd floats when scale > 1 (the gradient at
 *   the HD raster, transposed-upsampled by a gather pass), unused at scale 1.
 * waldo_flow_ctx_warp_bwd:  grad_flow (M,2,Hd,Wd), grad_alpha_ctx (M,L,Hd,Wd), grad_disocc (M,Hd,Wd),
 *   any may be NULL (zero);  grad_flow_lr (M,L,2,H,W) OVERWRITTEN;  grad_a01 (B*Tw,L,Hd,Wd) must be
 *   ZERO-FILLED (bilinear splat with float atomics, as F.grid_sample's backward; NULL to skip);
 *   grad_occ as above;  workspace: M*L*2*Hd*Wd floats when scale > 1.  The ghost mask (isobj_lr > 0.9)
 *   and the frame indices carry no gradient.
 * waldo_frame_warp_fuse_bwd:  grad_out (B,Tp,C+1,Hd,Wd), grad_raw (B,Tc',Tp,C+L,Hd,Wd), either may be
 *   NULL;  grad_flow (B,Tc,Tp,2,Hd,Wd) and grad_alpha (B,Tc,Tp,L,Hd,Wd) OVERWRITTEN.  The frames
 *   (`input`) are data: no gradient is produced for them.
 * ------------------------------------------------------------------------------------- */
int waldo_flow_ctx_alpha_bwd(const float* alpha_lr, const float* input, const float* dist,
                             const float* occ, const float* grad_a01, const float* grad_alpha_out,
                             float* grad_alpha_lr, float* grad_dist, float* grad_occ, float* workspace, int B,
                             int T, int Tw, int L, int Nl, int C, int chan_off, int H, int W, int scale,
                             waldo_stream_t stream);
int waldo_flow_ctx_warp_bwd(const float* flow_lr, const float* isobj_lr, const float* a01,
                            const int64_t* ctx_ts, const int64_t* pred_ts, const float* occ,
                            const float* grad_flow, const float* grad_alpha_ctx,
                            const float* grad_disocc, float* grad_flow_lr, float* grad_a01,
                            float* grad_occ, float* workspace, int B, int T, int Tw, int Tc, int Tp,
                            int L, int H, int W, int scale, waldo_stream_t stream);
int waldo_frame_warp_fuse_bwd(const float* input, const float* flow, const float* alpha,
                              const int64_t* ctx_ts, const float* grad_out, const float* grad_raw,
                              float* grad_flow, float* grad_alpha, int B, int T, int Tc, int Tp, int C,
                              int L, int Hd, int Wd, int include_self, float eps,
                              waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A9, low-resolution part: the class distribution of every object for the layout filter
 * (models/nets/lvd.py:624-634 and 731-746; csrc/lyt_dist.hip).  Per batch item, with x running over
 * the Tw frames and H x W pixels:
 *   win[o][x]  = (alpha[o][x] + 1e-6) * sum_n (cls[o][n] + min_cls) * softmax_n(lyt[.][x])[n]
 *                (the sum is 1 when cls is NULL: the reference's `cls is None` / no weight_cls case)
 *   mean[o][n] = sum_x win[o][x] lyt[n][x] / sum_x win[o][x];   dist[o][.] = softmax_n(mean[o][.])
 *   alpha  (B,Tw,layers,H,W)   projected alpha in [0,1]; the objects are layers first_obj ..
 *                              first_obj + No - 1 = layers - 1 (layer 0 is the background)
 *   lyt    layout logits at the alpha's raster: plane n of frame t of item b starts at
 *          lyt + b * lyt_batch_stride + t * lyt_frame_stride + n * H * W (elements), so a channel
 *          slice of the (B,T,3+Nl,H,W) input is passed without a copy
 *   cls    (B,No,Nl) or NULL;   dist, mean (B,No,Nl) and total (B,No) out (mean / total are what the
 *          backward needs);   workspace: waldo_lyt_dist_workspace_bytes(), shared by both directions
 * Backward: grad_dist (B,No,Nl) -> grad_alpha (B,Tw,layers,H,W) OVERWRITTEN (zero for the layers in
 * front of the objects) and grad_cls (B,No,Nl) OVERWRITTEN (NULL exactly when cls is).  The layout
 * logits are data (no gradient).  No atomics: per-workgroup partial sums added in workgroup order.
 * No, Nl <= 32.
 * ------------------------------------------------------------------------------------- */
int64_t waldo_lyt_dist_workspace_bytes(int64_t B, int Tw, int No, int Nl, int H, int W);
int waldo_lyt_dist_fwd(const float* alpha, const float* lyt, int64_t lyt_batch_stride,
                       int64_t lyt_frame_stride, const float* cls, float min_cls, float* dist,
                       float* mean, float* total, float* workspace, int64_t B, int Tw, int layers,
                       int first_obj, int No, int Nl, int H, int W, waldo_stream_t stream);
int waldo_lyt_dist_bwd(const float* grad_dist, const float* alpha, const float* lyt,
                       int64_t lyt_batch_stride, int64_t lyt_frame_stride, const float* cls,
                       float min_cls, const float* dist, const float* mean, const float* total,
                       float* grad_alpha, float* grad_cls, float* workspace, int64_t B, int Tw,
                       int layers, int first_obj, int No, int Nl, int H, int W,
                       waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Fused hot path (BASELINE.json metric): TPS grid (A2) -> bilinear warp of every 4-channel
 * layer (A4) -> LVD.reduce_comp (A6, lvd.py:100-114) in ONE launch.
 *   layers   (F,L,4,H,W) in [-1,1]   channel 3 = alpha; the alpha of layer 0 is taken as +1
 *   basis_t  (K3,H*W)                TPS basis of the output raster (shared by all frames)
 *   mapping  (F*L,K3,2)              from waldo_tps_mapping_fwd
 *   occ      (F,L,L)
 *   rgb      (F,3,H,W)  out, in [-1,1]
 *   alpha    (F,L,H,W)  out, composited alpha in [-1,1]; may be NULL (not written)
 * K3 <= 32, L <= waldo_max_layers().
 * Padding: every layer is sampled as grid_sample(x + delta, grid) - delta (A4; lvd.py:548,559).
 * delta = 0: taps outside a layer contribute 0 (zeros padding on the raw values: alpha 0.5 / grey
 * after the (x + 1) / 2 of reduce_comp) -- the BASELINE pipeline.  delta = 1 is the default of the
 * reference's layer_to_output: out-of-range taps read -1 (alpha 0 / black).  The shift only acts
 * where a footprint leaves the layer; with delta = 0 the results have the same bits as before the
 * parameter existed.
 * Coordinates: the grid is evaluated directly in pixel units (the mapping column scaled by W/2 or
 * H/2 inside the kernels), which moves a sample position by rounding only (~1e-5 px at 512 px).
 * ------------------------------------------------------------------------------------- */
int waldo_warp_composite_fwd(const float* layers, const float* basis_t, const float* mapping,
                             const float* occ, float* rgb, float* alpha, int64_t F, int L, int H,
                             int W, int K3, float delta, waldo_stream_t stream);
/* The same forward from the control points: mapping = inverse_kernel (N+3,N+3) @ [src_pts (F*L,N,2); 0]
 * (A2, warp.py:52-53) is computed inside the kernel (same fma order as waldo_tps_mapping_fwd: the
 * outputs have the same bits as waldo_tps_mapping_fwd + waldo_warp_composite_fwd), so a forward-only
 * call is ONE launch.  Served shapes: waldo_warp_composite_pts_supported() != 0 (N = 16, 4 | W);
 * otherwise EINVAL -- call the two-step path. */
int waldo_warp_composite_pts_supported(int L, int H, int W, int N);
int waldo_warp_composite_pts_fwd(const float* layers, const float* basis_t,
                                 const float* inverse_kernel, const float* src_pts,
                                 const float* occ, float* rgb, float* alpha, int64_t F, int L,
                                 int H, int W, int N, float delta, waldo_stream_t stream);
/* Backward of waldo_warp_composite_fwd.
 *   grad_rgb (F,3,H,W); grad_alpha (F,L,H,W) or NULL;
 *   workspace: scratch of at least waldo_warp_composite_bwd_workspace_bytes() bytes (256-byte
 *       aligned, contents irrelevant).  Non-NULL selects the two-kernel path (K3 == 19, L <= 17,
 *       4 | W: pixel kernel + per-source-tile gather, no global atomics, bitwise reproducible
 *       grad_layers / grad_mapping); NULL -- and every other shape, for which the size query
 *       returns 0 -- selects the generic per-tap-atomics kernel.
 *   Precision of grad_layers on the two-kernel path: a layer's gradient is summed in 32-bit FIXED
 *       POINT per 8x16-texel sub-block (of the 32x64-texel tile a workgroup owns), one power-of-two
 *       quantum for the sub-block's three colour planes and one for its alpha plane, chosen from an
 *       upper bound of the sub-block's sums so that nothing can overflow: quantum ~ 2^-17 of the
 *       largest possible sum of the group in that sub-block.  The error of a texel is therefore
 *       ABSOLUTE per sub-block and group (a few quanta), not relative to the texel: gradients several
 *       orders of magnitude below the largest ones of their 8x16 neighbourhood lose relative
 *       precision (the generic path keeps fp32 relative precision); a region of small gradients
 *       next to a region of large ones keeps its own.  An infinity or NaN among the contributions
 *       that can reach a tile turns that whole tile (all four planes) into NaN -- never into finite
 *       garbage.
 *   grad_layers (F,L,4,H,W): with a workspace it is OVERWRITTEN (every texel written once);
 *       without, it must be ZERO-FILLED by the caller (accumulated with float atomics);
 *   grad_mapping (F*L,K3,2): must be ZERO-FILLED by the caller (accumulated into); NULL to skip;
 *   grad_occ (F,L,L): must be ZERO-FILLED by the caller (float atomics); NULL to skip. */
int64_t waldo_warp_composite_bwd_workspace_bytes(int64_t F, int L, int H, int W, int K3);
int waldo_warp_composite_bwd(const float* layers, const float* basis_t, const float* mapping,
                             const float* occ, const float* grad_rgb, const float* grad_alpha,
                             float* grad_layers, float* grad_mapping, float* grad_occ,
                             void* workspace, int64_t workspace_bytes, int64_t F, int L, int H,
                             int W, int K3, float delta, waldo_stream_t stream);
/* The three calls above with `layers` (and, in the backward, `grad_layers`) of element type layers_dtype (enum
 * waldo_dtype): a 16-bit layer stack from a decoder under autocast.  Every other buffer -- basis_t, mapping,
 * inverse_kernel, src_pts, occ, rgb, alpha, grad_rgb, grad_alpha, grad_mapping, grad_occ, the workspace and its
 * records -- stays fp32, and so does the arithmetic: each 16-bit texel is widened exactly on load.
 *   forward:  rgb and alpha have the bits of the fp32 call on the widened stack (layers.float());
 *   backward: grad_layers has the bits of the fp32 call's grad_layers rounded to nearest-even (NaN stays a NaN, its
 *             payload is not kept); grad_mapping has the fp32 call's bits; grad_occ (float atomics) is the fp32
 *             call's up to summation order.
 * WALDO_DTYPE_F32: exactly the fp32 entry point.  An unknown code: WALDO_EINVAL ("unknown dtype") before any pointer
 * is read.  A 16-bit code is served by the staged forward and the two-kernel backward only: WALDO_EINVAL with the
 * reason, before any launch, where waldo_warp_composite_pts_supported(L, H, W, K3 - 3) == 0 (forward) or
 * waldo_warp_composite_bwd_workspace_bytes(max(F, 1), L, H, W, K3) == 0 (backward; its workspace is then required).
 * The workspace size query does not change. */
int waldo_warp_composite_fwd_dt(const void* layers, const float* basis_t, const float* mapping, const float* occ,
                                float* rgb, float* alpha, int64_t F, int L, int H, int W, int K3, float delta,
                                int layers_dtype, waldo_stream_t stream);
int waldo_warp_composite_pts_fwd_dt(const void* layers, const float* basis_t, const float* inverse_kernel,
                                    const float* src_pts, const float* occ, float* rgb, float* alpha, int64_t F,
                                    int L, int H, int W, int N, float delta, int layers_dtype, waldo_stream_t stream);
int waldo_warp_composite_bwd_dt(const void* layers, const float* basis_t, const float* mapping, const float* occ,
                                const float* grad_rgb, const float* grad_alpha, void* grad_layers,
                                float* grad_mapping, float* grad_occ, void* workspace, int64_t workspace_bytes,
                                int64_t F, int L, int H, int W, int K3, float delta, int layers_dtype,
                                waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A12. Fusion epilogue of WIF.forward with ii_score (models/nets/wif.py:49-54).
 *   vid (N,Tc,C,HW)  the UNet INPUT after the permute of wif.py:39 (N = B*T), C >= 5
 *   net (N,Tc,Co,HW) the UNet output, Co >= 4 (channels 0-2 residual, 3 score)
 *   out (N,3,HW) = sum_tc (sigmoid(vid_4 + 5) * vid_{0..2} + net_{0..2}) * softmax_tc(net_3)
 *   ab == 0 drops the sigmoid term (opt.ii_ab false, wif.py:53).
 * Backward: grad_vid (N,Tc,C,HW) / grad_net (N,Tc,Co,HW) are OVERWRITTEN (zero on the channels
 * the epilogue does not read); either may be NULL.
 * ------------------------------------------------------------------------------------- */
int waldo_wif_fuse_fwd(const float* vid, const float* net, float* out, int64_t N, int Tc, int C,
                       int Co, int64_t HW, int ab, waldo_stream_t stream);
int waldo_wif_fuse_bwd(const float* vid, const float* net, const float* out, const float* grad_out,
                       float* grad_vid, float* grad_net, int64_t N, int Tc, int C, int Co,
                       int64_t HW, int ab, waldo_stream_t stream);
/* The same with vid / net each of element type vid_dtype / net_dtype (enum waldo_dtype), widened to fp32 on load;
 * out and grad_out stay fp32; grad_vid is written in vid's type and grad_net in net's (rounded to nearest-even), with
 * the same overwrite / zero contract per channel. */
int waldo_wif_fuse_fwd_dt(const void* vid, const void* net, float* out, int64_t N, int Tc, int C, int Co,
                          int64_t HW, int ab, int vid_dtype, int net_dtype, waldo_stream_t stream);
int waldo_wif_fuse_bwd_dt(const void* vid, const void* net, const float* out, const float* grad_out,
                          void* grad_vid, void* grad_net, int64_t N, int Tc, int C, int Co, int64_t HW, int ab,
                          int vid_dtype, int net_dtype, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * f3. The mask dilation of WIF.inpaint: expand() (tools/utils.py:300-323; called at models/nets/wif.py:77,
 * 108-112, 204).  `num` rounds; a round is the steps named in `steps` (bit 0 south, 1 north, 2 east, 3 west -- 15 =
 * the reference's dir=None) taken IN THAT ORDER over the whole plane, each seeing the result of the one before:
 *     south: m[y,x] = max(m[y,x], alpha*m[y-1,x])   north: ... alpha*m[y+1,x]   east: ... alpha*m[y,x-1]   west: ... alpha*m[y,x+1]
 * with torch.maximum's NaN rule.  soft == 0: the same recurrence on (mask != 0) with alpha = 1 (the reference's
 * bool branch), written as 0.0 / 1.0.  The recurrence is executed literally inside a workgroup's LDS tile, so the
 * result has the framework's bits for every input.
 *   mask (planes,H,W) -> out (planes,H,W); mask is never written; out / scratch must not alias mask or each other;
 *   scratch (planes,H,W) is needed only when num > 30 (passes of 30 rounds ping-pong through it), else NULL.
 * The masks are data: no backward.
 * ------------------------------------------------------------------------------------- */
int waldo_mask_expand_fwd(const float* mask, float* out, float* scratch, int64_t planes, int H, int W, int num,
                          int steps, int soft, float alpha, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * f3. The point-in-polygon test of WIF.inpaint (models/nets/wif.py:228-235: matplotlib.path.Path(corners)
 * .contains_points(pts) -- radius 0, no transform -- for the region an object enters the frame from, wif.py:140-160).
 * matplotlib's own test (the crossings-multiply test over the path's vertices, closed back to the first, in double
 * precision) restated operation by operation, so that a point ON an edge gets matplotlib's answer.
 *   pts (N,2) f32 on the device (x, y);  corners_host (K,2) f64 in HOST memory, read before the call returns
 *   (3 <= K <= 16; fewer than three corners: nothing is inside, as in matplotlib);  out (N) f32: 1.0 inside, 0.0 outside
 *   (a point with a non-finite coordinate is outside).
 * ------------------------------------------------------------------------------------- */
int waldo_points_in_polygon_fwd(const float* pts, const double* corners_host, int K, float* out, int64_t N,
                                waldo_stream_t stream);
/* The same test, operation by operation, for P polygons whose corners are in DEVICE memory (what
 * waldo_border_objects_fwd leaves there: nothing is read on the host, nothing stops the stream):
 *   pts (N,2) f32, shared by the polygons;  corners f64: polygon p's K corners (x, y) at corners + p * corner_stride
 *   (corner_stride in doubles, >= 0; (P,K,2) contiguous: 2 K);  valid: polygon p is tested where
 *   valid[p * valid_stride] != 0 (int32; NULL: every polygon);  out (P,N) f32 -- an invalid polygon, or K < 3: zeros.
 *   0 <= K <= 16. */
int waldo_points_in_polygon_dev_fwd(const float* pts, const double* corners, int64_t corner_stride, const int* valid,
                                    int64_t valid_stride, int K, float* out, int64_t P, int64_t N,
                                    waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * f3. The border objects of WIF.inpaint (models/nets/wif.py:134-157) for a BATCH of clips, chosen on the device: per
 * clip b and side s (0 = left, 1 = right image border) the object that enters the last predicted frame through that
 * border and the four corners of the region it enters from.  With ident (H,W,2) the identity grid and
 * to_px(g) = ((g.x W + W - 1) / 2, (g.y H + H - 1) / 2), every operation in the framework's order:
 *   pred_px = to_px(pred_flow[b] + ident),  orig_px = to_px(ident)
 *   at      = pred_px.x < 3 (left),  pred_px.x >= W - 3 (right)
 *   obj[o]  = max over tc of (alpha_ctx[b, tc, Tp - 1, 1 + o] + 1) / 2  >  0.9        (a NaN wins the maximum)
 *   count[o] = number of pixels with at & obj[o];  valid = any count > 0;  obj_id = the first o of the largest count
 *   over the pixels with at & obj[obj_id]: by0, by1 = min, max of pred_px.y; ox0, ox1, oy0, oy1 of orig_px.x / .y
 *   (a NaN among them gives NaN, as torch.min / torch.max do)
 *   corners: left (0, by0) (0, by1) (ox1, oy1) (ox1, oy0);  right (ox0, oy0) (ox0, oy1) (W - 1, by1) (W - 1, by0)
 * Counts are integers and the extrema are min / max (integer atomics on order-preserving keys): the result does not
 * depend on the order of arrival.
 *   pred_flow: the (2,H,W) flow planes of the last context and last predicted frame of clip b at
 *   pred_flow + b * flow_stride_b + c * flow_stride_c (element strides; the planes contiguous);
 *   alpha_ctx (B,Tc,Tp,L,H,W) f32 by its element strides over (b, tc, tp, l), the (H,W) planes contiguous, as
 *   waldo_inpaint_holes_fwd takes it (the raw-slot view of decode_output is read in place);  2 <= L <= 32;
 *   out: valid (B,2) int32 (1 / 0), obj_id (B,2) int64 (0 where invalid), corners (B,2,4,2) f64 -- the exact widening
 *   of the fp32 extrema; zeros where invalid;
 *   workspace: waldo_border_objects_workspace_bytes(B) bytes, 4-byte aligned, any contents (a kernel initialises it).
 * How waldo_amd.nets.WIF uses it (two attributes of the module):
 *   border_on_device = None (default): a one-clip call takes the reference's branch, unchanged (host reads of the hit
 *     test, the object id and the corners; waldo_points_in_polygon_fwd); a batch takes this entry point, then
 *     waldo_points_in_polygon_dev_fwd per side and one object id per clip for the flow.  True: one clip too.  False: never.
 *   always_inpaint_borders = False (default): ONE device -> host read per call, of `valid`, to skip the external
 *     inpainter for a side nothing enters through; True: no read, both sides' inpainter calls always made -- the call
 *     is stream-ordered from start to end (HIP-graph capture).
 *   A clip with valid == 0 at a side gets a zero region and a zero appearance in that slot, whatever the inpainter
 *   returned for it.  The inpainter is called on the whole batch and must treat its clips independently; clips with an
 *   empty mask are passed along and their result is ignored.
 * ------------------------------------------------------------------------------------- */
int64_t waldo_border_objects_workspace_bytes(int64_t B);
int waldo_border_objects_fwd(const float* pred_flow, int64_t flow_stride_b, int64_t flow_stride_c, const float* ident,
                             const float* alpha_ctx, int64_t stride_b, int64_t stride_tc, int64_t stride_tp,
                             int64_t stride_l, int* valid, int64_t* obj_id, double* corners, void* workspace, int64_t B,
                             int Tc, int Tp, int L, int H, int W, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * f3. The per-frame propagation step of WIF.inpaint (models/nets/wif.py:179-214) as one launch: the inpainted reference
 * background warped along the background flow, up to two objects entering through the image border pasted over it, the
 * shadow mask, the fill of the frame's holes, and the inputs of the external inpainter (csrc/inpaint_ops.hip spells the
 * arithmetic; every operation in the framework's order: the bits of the composition it replaces).  All planes (B,.,H,W)
 * f32 contiguous:
 *   flow (B,H,W,2) grid-unit flow of this frame, ident (H,W,2) the identity grid (WIF.src_grid_hd);
 *   ref_img (B,3,H,W), ref_mask (B,1,H,W), shadow (B,1,H,W) or NULL (opt.use_shadows off);
 *   enter_region[k] (B,1,H,W), enter_look[k] (B,3,H,W), enter_flow[k] (B,H,W,2): HOST arrays of n_enter <= 2 device
 *   pointers (read before the call returns);  img (B,3,H,W), todo (B,1,H,W), obj (B,1,H,W) the frame, its hole mask and
 *   its object mask;
 *   out: img_out (B,3,H,W), todo_out (B,1,H,W), inp_mask (B,1,H,W) = 1 - (1 - todo)(1 - obj), and -- fix_mask == 0 --
 *   inp_img (B,3,H,W) = (1 - todo)(1 - obj) img  (fix_mask != 0: the inpainter takes img_out; inp_img may be NULL).
 * waldo_inpaint_blend_fwd: out (B,3,HW) = (1 - todo) img + todo fill  (wif.py:214).
 * ------------------------------------------------------------------------------------- */
int waldo_inpaint_propagate_fwd(const float* flow, const float* ident, const float* ref_img, const float* ref_mask,
                                const float* shadow, const float* const* enter_region, const float* const* enter_look,
                                const float* const* enter_flow, int n_enter, const float* img, const float* todo,
                                const float* obj, float* img_out, float* todo_out, float* inp_img, float* inp_mask,
                                int64_t B, int H, int W, int soft_shadow, int fix_mask, waldo_stream_t stream);
int waldo_inpaint_blend_fwd(const float* img, const float* todo, const float* fill, float* out, int64_t B, int64_t HW,
                            waldo_stream_t stream);
/* The hole and object masks of the predicted frames (wif.py:60-75) in one pass over alpha_ctx (B,Tc,Tp,L,H,W) f32 --
 * given by its element strides over (b, tc, tp, l); the (H,W) planes contiguous, HW = H*W:
 *   cover = sum_l (alpha_ctx + 1) / 2,  obj = the same over l >= 1  (summed as the framework's reduction sums a short
 *   strided dimension: four accumulators j % 4, combined in order); last_only != 0: the last context's, else the maximum
 *   over the contexts (a NaN wins);  mask (B,Tp,HW) = (1 - cover) > thresh,  obj_mask (B,Tp,HW) = obj > 0.9, as 0 / 1.
 *   thresh: 0.1 with opt.fix_thresh, 0.9 without (wif.py:70-73). */
int waldo_inpaint_holes_fwd(const float* alpha_ctx, int64_t stride_b, int64_t stride_tc, int64_t stride_tp,
                            int64_t stride_l, float* mask, float* obj_mask, int64_t B, int Tc, int Tp, int L,
                            int64_t HW, int last_only, float thresh, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A8. gather_time (models/nets/lvd.py:462-467) with the frame arithmetic of the flow synthesis
 * (lvd.py:660-668, 780-787) on a clip's grids x (B,T,P,2) -- P pairs per frame:
 *   subtract != 0:  out[b,tc,tp] = x[b, ctx_ts[b,tc,tp]] - x[b, pred_ts[tp]]   (layer-space flow)
 *   subtract == 0:  out[b,tc,tp] = x[b, ctx_ts[b,tc,tp]]  (gather_time), or, with ctx_ts == NULL,
 *                   x[b, pred_ts[tp]] repeated over the Tc contexts (the `[:, pred_ts].unsqueeze(1).expand`)
 *   HW > 0 (a divisor of P): out is written channel-first, (B,Tc,Tp,P/HW,2,HW) -- the
 *   permute(..., 6, 4, 5) + reshape of lvd.py:662-664; HW == 0: (B,Tc,Tp,P,2).
 * ctx_ts (B,Tc,Tp) / pred_ts (Tp) int64 on the device, valid in [0,T): clamped, and the forward reports a violation
 * in `status` ("Frame-index status" above).
 * Backward: grad_x (B,T,P,2) is OVERWRITTEN with the sum over the output frames that read each input
 * frame (a gather: deterministic, no atomics, no zero fill needed).
 * ------------------------------------------------------------------------------------- */
int waldo_time_gather_fwd(const float* x, const int64_t* ctx_ts, const int64_t* pred_ts, float* out,
                          int* status, int B, int T, int Tc, int Tp, int64_t P, int64_t HW, int subtract,
                          waldo_stream_t stream);
int waldo_time_gather_bwd(const float* grad_out, const int64_t* ctx_ts, const int64_t* pred_ts,
                          float* grad_x, int B, int T, int Tc, int Tp, int64_t P, int64_t HW,
                          int subtract, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A7. scale(input[:, :Tw, c0:], 1 / S) (models/nets/lvd.py:611 / 716 through scale(), lvd.py:175-179):
 * F.interpolate(bilinear, align_corners=False, scale_factor=1/S) of the channel slice, S a power of two >= 2
 * (1 / S exact).   input (B,T,C,H*S,W*S)  ->  out (B,Tw,C-c0,H,W); the same bits as F.interpolate's device kernel
 * (its CPU kernel associates the four terms differently: last-ulp differences).  The frames are data: no backward.
 * ------------------------------------------------------------------------------------- */
int waldo_downscale_frames_fwd(const float* input, float* out, int B, int T, int Tw, int C, int c0, int H,
                               int W, int S, waldo_stream_t stream);
/* The same for the layout channels of a packed clip (B,T,H*S,W*S) ("Packed clip" above): out (B,Tw,Nl,H,W), the bits of
 * waldo_downscale_frames_fwd on the unpacked clip with c0 = 3.  1 <= Nl <= 32. */
int waldo_downscale_frames_packed_fwd(const uint8_t* clip, float* out, int B, int T, int Tw, int Nl, int H, int W,
                                      int S, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Frame metrics: PSNR, SSIM and MS-SSIM per frame of a predicted clip against the real one -- what the reference's
 * scorer takes from TensorFlow (tools/eval/metrics.py:67-74: tf.image.psnr / ssim / ssim_multiscale, max_val = 1, on
 * frames of bytes / 255).  Definitions: waldo_amd/metrics.py and DESIGN.md 4g.  Each operand is one of:
 *   WALDO_METRICS_F32     (B,T,3,H,W) fp32 in [lo, hi]; element strides sb, st, sc, sh (W unit-stride); quantised
 *                         by `quant` (below);
 *   WALDO_METRICS_U8      (B,T,3,H,W) uint8 bytes taken as they are (byte / 255); byte strides, W unit-stride;
 *   WALDO_METRICS_PACKED  a packed clip ("Packed clip" above) (B,T,H,W) of 4-byte pixels, read in place: its RGB
 *                         bytes go through rgb_table and then through the quantisation of an fp32 operand (the bits
 *                         of its unpacked form); strides sb, st, sh in PIXELS (sc unused), 4-byte aligned base.
 * quant (fp32 and packed operands): u = clamp((x - lo) / range, 0, 1) in fp32, then
 *   WALDO_METRICS_TRUNC  trunc(u * 255) / 255   (the reference's dump_video bytes, tools/utils.py:246-264),
 *   WALDO_METRICS_ROUND  trunc(u * 255 + 0.5) / 255   (waldo_amd.tools.io.dump_video's bytes),
 *   WALDO_METRICS_NONE   u.
 * `range` is hi - lo, as the caller computes it (> 0).  mask: WALDO_METRIC_* bits; SSIM needs H, W >= 11, MS-SSIM
 * five scales of at least 11 x 11 (each scale halves a side, rounding up: H, W >= 161).  partials / scratch: caller-
 * owned workspaces of waldo_frame_metrics_partial_bytes / _scratch_bytes (scratch: 0 bytes without MS-SSIM, NULL
 * allowed then).  Outputs (B*T) fp32 each, NULL where the mask does not ask for the metric; psnr = +inf for equal
 * frames.  Deterministic: fixed-order sums, no atomics; metrics(a, b) and metrics(b, a) have the same bits. */
enum waldo_metrics_enc { WALDO_METRICS_F32 = 0, WALDO_METRICS_U8 = 1, WALDO_METRICS_PACKED = 2 };
enum waldo_metrics_quant { WALDO_METRICS_TRUNC = 0, WALDO_METRICS_ROUND = 1, WALDO_METRICS_NONE = 2 };
#define WALDO_METRIC_PSNR 1
#define WALDO_METRIC_SSIM 2
#define WALDO_METRIC_MSSSIM 4
int64_t waldo_frame_metrics_partial_bytes(int B, int T, int H, int W, int mask);
int64_t waldo_frame_metrics_scratch_bytes(int B, int T, int H, int W, int mask);
int waldo_frame_metrics_fwd(const void* a, int enc_a, int64_t sa_b, int64_t sa_t, int64_t sa_c, int64_t sa_h,
                            const void* b, int enc_b, int64_t sb_b, int64_t sb_t, int64_t sb_c, int64_t sb_h,
                            const float* rgb_table, int B, int T, int H, int W, float lo, float range, int quant,
                            int mask, double* partials, float* scratch, float* psnr, float* ssim, float* msssim,
                            waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Byte output: predicted frames as uint8, quantised on the device -- what the reference's save_vid -> dump_video makes
 * of every clip predict() returns (models/synthesizer.py:403-411, tools/utils.py:246-264) and its scorer reads.
 * THE quantisation of the library (csrc/quantize.hip.h; waldo_frame_metrics_fwd applies the same text before its / 255):
 * for a value x and a span (lo, hi), hi > lo, range = hi - lo as the caller computes it in fp32,
 *     u = clamp((x - lo) / range, 0, 1)
 *     WALDO_METRICS_TRUNC   byte = (uint8) truncf(u * 255)         (the reference's dump_video)
 *     WALDO_METRICS_ROUND   byte = (uint8) truncf(u * 255 + 0.5)   (waldo_amd.tools.io.dump_video / dump_image)
 * in fp32 with IEEE division; a 16-bit value is widened exactly first.  NaN RULE: the clamp is fminf(fmaxf(u, 0), 1), so a
 * NaN gives byte 0; -inf gives 0 and +inf 255.  WALDO_METRICS_NONE is not a byte quantisation: WALDO_EINVAL.
 *
 * waldo_frames_to_bytes_fwd: N frames of C planes of H x W values -> uint8.
 *   src       src_code WALDO_DTYPE_F32 / _F16 / _BF16: planar frames, element strides ss_n, ss_c, ss_h (W unit-stride:
 *             a channel or time slice of a larger tensor needs no copy), aligned to its elements;
 *             src_code WALDO_BYTES_SRC_PACKED: a packed clip ("Packed clip" above), N frames of H x W 4-byte pixels,
 *             strides ss_n, ss_h in PIXELS (ss_c unused), 4-byte aligned, C = 3: the bytes are
 *             quantise(rgb_table[byte]) -- NOT the clip's own bytes, which "trunc" does not give back for 63 of the 256
 *             values; rgb_table (256 fp32) is read for a packed source only (else NULL allowed);
 *   dst       WALDO_BYTES_NCHW: (N, C, H, W), or WALDO_BYTES_NHWC: (N, H, W, 3) with C = 3 (what a video writer takes);
 *             each frame dense, frame stride ds_n in bytes, ANY alignment of the base (a view into a larger buffer).
 * Caller-owned buffers, the caller's stream, no allocation, no synchronisation; N == 0: WALDO_OK without a launch.
 * WALDO_EINVAL with a message before any launch: an unknown source, layout or quantisation code; range <= 0 or a
 * non-finite span; a negative stride; C != 3 with WALDO_BYTES_NHWC or a packed source; H or W outside [1, 32768], C
 * outside [1, 4096]; a null pointer; a source that is not aligned to its elements; more than 2^31 - 1 workgroups.
 *
 * waldo_wif_fuse_bytes_fwd / _dt: waldo_wif_fuse_fwd / _dt (A12 above) with out as bytes, (N, 3, HW) or (N, HW, 3):
 * the bytes of waldo_frames_to_bytes_fwd on A12's fp32 result, bit for bit (the same arithmetic in the same order, then
 * the quantisation above), without the 12 bytes per pixel in between.  Forward only.
 * ------------------------------------------------------------------------------------- */
enum waldo_bytes_layout { WALDO_BYTES_NCHW = 0, WALDO_BYTES_NHWC = 1 };
#define WALDO_BYTES_SRC_PACKED 3 /* a source code next to enum waldo_dtype's */
int waldo_frames_to_bytes_fwd(const void* src, int src_code, int64_t ss_n, int64_t ss_c, int64_t ss_h,
                              const float* rgb_table, uint8_t* dst, int64_t ds_n, int layout, int64_t N, int C, int H,
                              int W, float lo, float range, int quant, waldo_stream_t stream);
int waldo_wif_fuse_bytes_fwd(const float* vid, const float* net, uint8_t* out, int64_t N, int Tc, int C, int Co,
                             int64_t HW, int ab, float lo, float range, int quant, int layout, waldo_stream_t stream);
int waldo_wif_fuse_bytes_fwd_dt(const void* vid, const void* net, uint8_t* out, int64_t N, int Tc, int C, int Co,
                                int64_t HW, int ab, float lo, float range, int quant, int layout, int vid_dtype,
                                int net_dtype, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Renders: the three views of the layered decomposition as bytes, made on the device -- which class or object layer
 * owns a pixel (the reference's Logger.get_lyt, tools/logger.py:169-202 -> color_transfer, tools/utils.py:202-214) and
 * the flow that moved it (Logger.get_flow_rgb, tools/logger.py:265-318), without the reference's trip through the host.
 *
 * waldo_render_argmax_fwd: N frames of C planes of H x W values -> the class id of every pixel and / or its colour.
 *   src       src_code WALDO_DTYPE_F32 / _F16 / _BF16: planar frames, element strides ss_n, ss_c, ss_h (W unit-stride:
 *             the channel slice output[:, :, 3:3+Nl] or a time slice is read in place), aligned to its elements.  A
 *             packed clip holds its ids already: WALDO_BYTES_SRC_PACKED is WALDO_EINVAL.
 *   id        the index torch.max(dim) returns on the CPU: scanning c upward, c replaces the best so far when
 *             v > best || (v != v && best == best) -- the lowest c among the maxima wins, NaN is greater than
 *             everything and the first NaN wins, -0.0 == +0.0; a 16-bit value is widened exactly first.
 *   palette   C rows of 3 bytes on the device, read only when rgb != NULL: rgb[pixel] = palette[id].
 *   ids       (N, H, W) bytes, or NULL;  rgb: WALDO_BYTES_NCHW (N, 3, H, W) or WALDO_BYTES_NHWC (N, H, W, 3), or NULL --
 *             not both NULL; both come from the one pass.  Each frame dense, frame strides di_n, dr_n in bytes, ANY
 *             alignment of either base.
 *   C in [1, 256] (an id fits a byte), H and W in [1, 32768].
 *
 * waldo_render_flow_fwd: N flows (2, H, W) (plane 0 = u, plane 1 = v; strides as above) -> RGB bytes.  Per pixel, in fp32
 * with IEEE division and no contraction of u u + v v into an fma:
 *     m = sqrtf(u u + v v);  r = min(m / sqrt(2) * mul, 1), a NaN kept (the reference's r[r > 1] = 1)
 *     theta = (1 + atan2f(v, u) / pi) / 2;  k = min((int)(theta K), K - 1)
 *     channel c = byte of r * wheel[3 k + c] under the quantisation of "Byte output" with the span (0, 1)
 * NaN in u or v gives bytes 0 (the NaN rule of "Byte output"; the reference's "bad" colour (0, 0, 0) times NaN); a zero
 * flow gives bytes 0.  wheel: K rows of 3 fp32 on the device (the reference: hsv with 128 entries), K in [1, 4096];
 * mul finite; quant WALDO_METRICS_TRUNC / _ROUND (WALDO_METRICS_NONE: WALDO_EINVAL).  rgb as above.
 *
 * Both: caller-owned buffers, the caller's stream, no workspace, no allocation, no synchronisation; N == 0: WALDO_OK
 * without a launch.  WALDO_EINVAL with a message before any launch: an unknown dtype, layout or quantisation code; a
 * non-finite mul; a bad shape (N < 0, C, K, H or W outside its range); a negative stride; a null src / flow / wheel, ids
 * and rgb both null, rgb without a palette; a source that is not aligned to its elements; more than 2^31 - 1 workgroups.
 * ------------------------------------------------------------------------------------- */
int waldo_render_argmax_fwd(const void* src, int src_code, int64_t ss_n, int64_t ss_c, int64_t ss_h,
                            const uint8_t* palette, uint8_t* ids, int64_t di_n, uint8_t* rgb, int64_t dr_n,
                            int layout, int64_t N, int C, int H, int W, waldo_stream_t stream);
int waldo_render_flow_fwd(const void* flow, int src_code, int64_t ss_n, int64_t ss_c, int64_t ss_h,
                          const float* wheel, int K, float mul, uint8_t* rgb, int64_t dr_n, int layout, int quant,
                          int64_t N, int H, int W, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Supervision targets: the data-side target of LVD training and its control-point distance terms -- what the
 * reference's Synthesizer.extract_object builds from the real flow and layout on every step (models/synthesizer.py:
 * 907-945, 965-979; models/modules/edge.py).  fp32 throughout; every tensor contiguous NCHW.
 *
 * waldo_flow_edges_fwd: EdgeExtractor.forward (edge.py:28-40).  flow (N, C, H, W), C = 1 or 2 -> flow_edge and
 *   dominant, (N, 1, H, W) each.  Reflection padding k/2; per channel the k x k mean (weight 1.0f / (k k)) and the two
 *   gradient filters, weights (float)x_i / (float)(x_i x_i + y_j y_j) and (float)y_j / (the same), the centre's divisor
 *   1 -- divided in fp32 as the reference divides;  e_c = sqrtf(gx gx + gy gy + eps) / (float)sqrt(32);
 *   flow_edge = 1 - prod_c (1 - e_c);  dominant = [sum_c flow_c^2 > sum_c mean_c^2] as 0.0f / 1.0f.
 *   One launch: a 16 x 64 tile with its halo per channel in LDS, the weights in the kernel's arguments.
 *   k odd in [3, 15]; H, W > k/2.
 *
 * waldo_gaussian_blur_fwd: the reference's blur (synthesizer.py:1114-1118: GaussianBlur(kernel_size, sigma) with a
 *   fixed sigma), depthwise over P planes of H x W.  1-D weights exp(-0.5 (t / sigma)^2) at t = -(k-1)/2 .. (k-1)/2,
 *   normalised to sum 1, in fp32; reflection padding k/2; rows, then columns (the reference multiplies by the outer
 *   product: the same number up to rounding).  One launch: the row pass into LDS, the column pass from LDS.
 *   k odd in [3, 31]; H, W > k/2; sigma > 0 and finite.  y must not overlap x.
 *
 * waldo_mov_props_fwd: the per-pixel sums over layout channels (synthesizer.py:912-916, 924).  lyt (N, Nl, H, W), flow
 *   (N, 2, H, W); the channel lists as bit masks (bit c = channel c; Nl <= 32, no bit at or above Nl).
 *   prop(list) = sum over the list's channels, ascending, of lyt_c / 10 + 0.5.
 *   fg_prop = prop(fg);  nobg_prop = 1 - prop(bg);  other_prop = prop(other);  all (N, 1, H, W);
 *   blur_in (N, 3, H, W) = (1 - fg_prop, (1 - fg_prop) flow_0, (1 - fg_prop) flow_1).
 *
 * waldo_mov_finish_fwd: synthesizer.py:909, 917-942 (blur_alpha off).  blurred (N, 3, H, W) = the blur of blur_in;
 *   edge_raw, dominant = waldo_flow_edges_fwd's outputs.  Per pixel:
 *     edge = [edge_raw > flow_thresh];  sum = blurred_0 + [blurred_0 == 0];  mean_bg_flow = blurred_{1,2} / sum
 *     delta = fg_prop (|flow_0 - mean_0| + |flow_1 - mean_1|);  mask = [delta > mov_obj_thresh]
 *     WALDO_MOV_DOMINANT_OTHER: mask = max(mask, other_prop dominant edge)
 *     WALDO_MOV_FLOW_NOBG:      mask = mask | (edge > 0.1 & nobg_prop > 0)    (not with _DOMINANT_OTHER: the
 *                               reference's `|` of a float tensor raises there)
 *     mov_obj = 2 mask - 1;  negative values times reg_bg_mul;  then, in this order, each only where mov_obj < 0:
 *     WALDO_MOV_USE_FG:    fg_prop > 0 -> 0;   WALDO_MOV_USE_NOBG: nobg_prop > 0 -> 0;
 *     WALDO_MOV_USE_NOBG_EDGE: nobg_prop > 0 & edge > 0.1 -> nobg_edge_mul
 *   Writes edge, mask, mov_obj (N, 1, H, W) and mean_bg_flow (N, 2, H, W).
 *
 * waldo_cell_distance_fwd / _bwd: synthesizer.py:965-979 without its (B, T, No, K, H, W) tensor.  Per frame f and object
 *   n the caller passes the moments of the object's K points c_nk, moments (F, No, 3) = (sum_k c_x, sum_k c_y,
 *   sum_k |c|^2), so that  dis_n(g) = sum_k |g - c_nk|^2 = K |g|^2 - 2 g . S1_n + S2_n  at the pixel's coordinate
 *   g = (gx[x], gy[y]) (gx (W), gy (H): the columns and rows of get_grid).
 *     w = (mov_mask + eps) (1 - fg_mask)   with fg_mask;   w = mov_mask   with fg_mask == NULL (the centre term)
 *     out[0] = mean over F H W of min_n w dis_n;   chosen (F, H, W) bytes: the n of the minimum -- scanning n upward,
 *     n replaces the best when v < best || (v != v && best == best): ties go to the lowest index, as torch.min(dim) on
 *     the CPU; No <= 31.
 *   Backward, grad_out a device scalar:  grad_moments (F, No, 3) = grad_out / (F H W) * sum over the pixels that chose n
 *   of (-2 w gx, -2 w gy, w);  grad_fg (F, 1, H, W) = -grad_out (mov_mask + eps) dis_chosen / (F H W), or NULL.
 *   Both are OVERWRITTEN.  NO FLOAT ATOMICS: every sum is a partial per workgroup, stored to the workspace, then one
 *   pass over the partials in a fixed order -- out and both gradients are the same bits from run to run, whatever
 *   the deterministic mode of the caller.  workspace: waldo_cell_distance_workspace_bytes(F, No, H W) for either call.
 *
 * All: caller-owned buffers and workspace, the caller's stream, no allocation, no synchronisation; N == 0 (F == 0):
 * WALDO_OK without a launch.  WALDO_EINVAL with a message before any launch: k even or outside its range; H or W
 * <= k/2; C outside [1, 2]; Nl outside [1, 32] or a mask bit at or above Nl; No outside [1, 31]; unknown flag bits or
 * both _DOMINANT_OTHER and _FLOW_NOBG; a bad sigma, eps or K; a null pointer; a workspace that is too small; more
 * than 2^31 - 1 workgroups.
 * ------------------------------------------------------------------------------------- */
#define WALDO_MOV_USE_FG 1
#define WALDO_MOV_USE_NOBG 2
#define WALDO_MOV_USE_NOBG_EDGE 4
#define WALDO_MOV_FLOW_NOBG 8
#define WALDO_MOV_DOMINANT_OTHER 16
int waldo_flow_edges_fwd(const float* flow, float* flow_edge, float* dominant, int64_t N, int C, int H, int W, int k,
                         float eps, waldo_stream_t stream);
int waldo_gaussian_blur_fwd(const float* x, float* y, int64_t P, int H, int W, int k, float sigma,
                            waldo_stream_t stream);
int waldo_mov_props_fwd(const float* lyt, const float* flow, uint32_t fg_bits, uint32_t bg_bits, uint32_t other_bits,
                        float* fg_prop, float* nobg_prop, float* other_prop, float* blur_in, int64_t N, int Nl,
                        int64_t HW, waldo_stream_t stream);
int waldo_mov_finish_fwd(const float* flow, const float* blurred, const float* fg_prop, const float* nobg_prop,
                         const float* other_prop, const float* edge_raw, const float* dominant, float flow_thresh,
                         float mov_obj_thresh, float reg_bg_mul, float nobg_edge_mul, int flags, float* edge,
                         float* mean_bg_flow, float* mask, float* mov_obj, int64_t N, int64_t HW,
                         waldo_stream_t stream);
int64_t waldo_cell_distance_workspace_bytes(int64_t F, int No, int64_t HW);
int waldo_cell_distance_fwd(const float* moments, const float* mov_mask, const float* fg_mask, const float* gx,
                            const float* gy, float* out, uint8_t* chosen, void* workspace, int64_t workspace_bytes,
                            int64_t F, int No, int H, int W, float K, float eps, waldo_stream_t stream);
int waldo_cell_distance_bwd(const float* moments, const float* mov_mask, const float* fg_mask, const float* gx,
                            const float* gy, const uint8_t* chosen, const float* grad_out, float* grad_moments,
                            float* grad_fg, void* workspace, int64_t workspace_bytes, int64_t F, int No, int H, int W,
                            float K, float eps, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Reproducible gradients (deterministic mode).  The backward entry points above that say "ZERO-FILLED ... atomics"
 * sum with float atomics: the result depends on the order of arrival and differs in its last bits from run to run.
 * Each has a twin, suffix _det, whose result is a function of its inputs alone -- the same bits from run to run,
 * launched eagerly or replayed from a HIP graph.  Every other backward entry point already is (no atomics).  The
 * library keeps no mode: the caller picks the entry point.
 *
 * Contract of every *_det entry point: the arguments of its twin, plus (where the twin has none) a workspace and
 * its size in bytes from the *_det_workspace_bytes query next to it -- ONE workspace, which also holds what the
 * twin keeps in its own (the HD gradients of scale > 1, the two-kernel backward's records).  The gradients are
 * OVERWRITTEN: the caller zero-fills nothing (fills inside are kernels, never memset calls).  Caller-owned memory,
 * the caller's stream, no allocation, no synchronisation, nothing returns to the host.  WALDO_EINVAL with a message
 * before any launch for a bad argument, a workspace that is too small, or a shape that has no deterministic kernel.
 * A query returns 0 for such a shape.
 *
 * Two forms (csrc/det_common.hip.h):
 *
 *   SLAB         small tables summed over all pixels: grad_occ, grad_dist, grad_mapping.  Every workgroup (every
 *                wavefront of the fused backward's pixel kernel) stores its partial table to a row of a slab in the
 *                workspace; a second kernel sums the rows of one destination in a fixed order.  The order depends on
 *                the shapes and on nothing else.  fp32 throughout; values differ from the twin's by summation order.
 *
 *   FIXED POINT  bilinear splats onto texels chosen by the data: grad_input of grid_sample2d, grad_a01 of
 *                flow_ctx_warp.  (1) the largest contribution magnitude of every destination PLANE (one (map,
 *                channel) image) is taken with an integer atomic maximum on the bit patterns; (2) every contribution c
 *                is added as the 64-bit integer rint(c * 2^k) with integer atomics; (3) the sums are converted to
 *                fp32 with one rounding and scaled by 2^-k.  With the plane's maximum < 2^ex (frexp) and at most
 *                2^clog contributions to one texel,
 *
 *                    k = 63 - ex - clog,     clog = ceil(log2(max contributions per texel)) <= 32
 *
 *                so that no sum can overflow for ANY input and one quantum 2^-k is at most 2^(clog - 62) <= 2^-30 of
 *                the plane's largest contribution.  The contribution bound follows from the shapes:
 *                    grid_sample2d:  min(N, ceil(outer_div / inner)) * Ho * Wo  (the output maps that read one input
 *                                    map, one contribution per output pixel); the weights are in [0, 1], so the
 *                                    maximum of |grad_output * pre_scale| over those maps bounds the contributions;
 *                    flow_ctx_warp:  Tc * Tp * Hd * Wd; the value a pixel distributes (the gradient of its sample,
 *                                    gs * ghost) comes out of the composite's backward and has no bound from the
 *                                    inputs: the pixel kernel STORES it per (unit, layer, pixel) in the workspace, a
 *                                    pass takes the maximum, and the splat kernel derives the taps again.
 *                A shape beyond 2^32 contributions per texel is rejected.  k follows the maximum in powers of two:
 *                doubling the incoming gradient doubles these gradients exactly.
 *                NON-FINITE: a plane whose maximum is infinite or NaN comes back ALL NaN (a NaN has no integer);
 *                other planes are unaffected.  Coarser than the twin, which poisons only the texels touched.
 *
 *   grad_input   of waldo_grid_sample2d_bwd_det / _ex_bwd_det: FIXED POINT; all Nin maps are written (the twin's
 *                arguments do not say how many there are: Nin is an argument here).  grad_grid: per pixel, as the twin.
 *                workspace: round256(Nin*C*Hi*Wi*8) + round256(Nin*C*4)   (round256: up to a multiple of 256)
 *   grad_occ     of waldo_occ_composite_bwd_det: SLAB; the ceil(M / occ_div) matrices that maps read are written.
 *                workspace: round256(M * groups * L*L*4); groups = workgroups per map = ceil(ceil(HW / 256) / 4)
 *   grad_mapping of waldo_tps_grid_bwd_det: SLAB; K3 <= 136.
 *                workspace: round256(B * gx * K3*2*4); gx = pixel groups per map = ceil(ceil(HW / 1024) / 4)
 *   grad_dist, grad_occ of waldo_flow_ctx_alpha_bwd_det: SLAB; all of (B,L-1,Nl) and (B,T,L,L) written.
 *                workspace: [scale > 1: round256(B*Tw*L*Hd*Wd*4)] + round256(B*Tw*groups*L*L*4)
 *                           + round256(B*Tw*groups*(L-1)*Nl*4)    (Nl: 0 without a filter);
 *                           groups = workgroups per (b, t) = ceil(ceil(Hd*Wd / 256) / 4)
 *   grad_a01     of waldo_flow_ctx_warp_bwd_det: FIXED POINT; grad_occ: SLAB, summed per predicted frame; all written.
 *                workspace: [scale > 1: round256(M*L*2*Hd*Wd*4)] + round256(M*L*Hd*Wd*4) + round256(B*Tw*L*Hd*Wd*8)
 *                           + round256(B*Tw*L*4) + round256(M*groups*L*L*4),  M = B*Tc*Tp (groups as above)
 *   grad_occ     of waldo_warp_composite_bwd_det (layers of any waldo_dtype): SLAB, one row per (frame, 16x16 tile,
 *                wavefront).  The two-kernel backward only (K3 == 19, L <= 17, W % 4 == 0, H, W >= 2), where
 *                grad_layers and grad_mapping already are order-independent; the generic backward (per-tap float
 *                atomics for everything) has no twin: such a shape is rejected.  grad_mapping is zero-filled inside.
 *                workspace: waldo_warp_composite_bwd_workspace_bytes + round256(F * tiles16 * 4 * L*L*4),
 *                           tiles16 = ceil(H / 16) * ceil(W / 16)
 * ------------------------------------------------------------------------------------- */
int64_t waldo_grid_sample2d_bwd_det_workspace_bytes(int64_t N, int64_t Nin, int C, int Hi, int Wi, int Ho, int Wo);
int waldo_grid_sample2d_bwd_det(const float* input, const float* grid, const float* grad_output, float* grad_input,
                                float* grad_grid, int64_t N, int64_t Nin, int C, int Hi, int Wi, int Ho, int Wo,
                                float delta, int64_t outer_div, int64_t inner, void* workspace,
                                int64_t workspace_bytes, waldo_stream_t stream);
int waldo_grid_sample2d_ex_bwd_det(const float* input, const float* grid, const float* grad_output, float* grad_input,
                                   float* grad_grid, int64_t N, int64_t Nin, int C, int Hi, int Wi, int Ho, int Wo,
                                   float delta, int64_t outer_div, int64_t inner, int64_t gout_group,
                                   int64_t gout_stride, int64_t gout_offset, float pre_scale, float pre_bias,
                                   void* workspace, int64_t workspace_bytes, waldo_stream_t stream);
int64_t waldo_occ_composite_bwd_det_workspace_bytes(int64_t M, int L, int64_t HW);
int waldo_occ_composite_bwd_det(const float* alpha, const float* occ, const float* grad_out, float* grad_alpha,
                                float* grad_occ, int64_t M, int L, int64_t HW, int64_t occ_div, void* workspace,
                                int64_t workspace_bytes, waldo_stream_t stream);
int64_t waldo_tps_grid_bwd_det_workspace_bytes(int64_t B, int64_t HW, int K3);
int waldo_tps_grid_bwd_det(const float* basis_t, const float* grad_grid, float* grad_mapping, int64_t B, int64_t HW,
                           int K3, void* workspace, int64_t workspace_bytes, waldo_stream_t stream);
int64_t waldo_flow_ctx_alpha_bwd_det_workspace_bytes(int B, int Tw, int L, int Nl, int H, int W, int scale);
int waldo_flow_ctx_alpha_bwd_det(const float* alpha_lr, const float* input, const float* dist, const float* occ,
                                 const float* grad_a01, const float* grad_alpha_out, float* grad_alpha_lr,
                                 float* grad_dist, float* grad_occ, void* workspace, int64_t workspace_bytes, int B,
                                 int T, int Tw, int L, int Nl, int C, int chan_off, int H, int W, int scale,
                                 waldo_stream_t stream);
int64_t waldo_flow_ctx_warp_bwd_det_workspace_bytes(int B, int Tw, int Tc, int Tp, int L, int H, int W, int scale);
int waldo_flow_ctx_warp_bwd_det(const float* flow_lr, const float* isobj_lr, const float* a01, const int64_t* ctx_ts,
                                const int64_t* pred_ts, const float* occ, const float* grad_flow,
                                const float* grad_alpha_ctx, const float* grad_disocc, float* grad_flow_lr,
                                float* grad_a01, float* grad_occ, void* workspace, int64_t workspace_bytes, int B,
                                int T, int Tw, int Tc, int Tp, int L, int H, int W, int scale, waldo_stream_t stream);
int64_t waldo_warp_composite_bwd_det_workspace_bytes(int64_t F, int L, int H, int W, int K3);
int waldo_warp_composite_bwd_det(const void* layers, const float* basis_t, const float* mapping, const float* occ,
                                 const float* grad_rgb, const float* grad_alpha, void* grad_layers,
                                 float* grad_mapping, float* grad_occ, void* workspace, int64_t workspace_bytes,
                                 int64_t F, int L, int H, int W, int K3, float delta, int layers_dtype,
                                 waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Plane norm: the work between the convolutions of one UNet level (the reference's models/modules/conv.py:19-25,
 * 59: conv -> CustomNorm("ln2d") = GroupNorm(C, C) -> GELU, then torch.cat([y, y_skip], dim=1)) in one call each way.
 *
 * waldo_plane_norm_gelu_fwd: x (N, C, H, W) fp32, every plane dense (H W consecutive values), planes xs_c and frames
 *   xs_n elements apart; gamma, beta (C); skip (N, Cs, H, W) with strides ss_n, ss_c, or NULL with Cs == 0;
 *   out (N, C + Cs, H, W), frames os_n >= (C + Cs) H W elements apart, channels dense.  Per plane (n, c):
 *     mean = sum x / (H W);  var = sum (x - mean)^2 / (H W)  (biased);  rstd = 1 / sqrt(var + eps)
 *     z = (x - mean) rstd gamma[c] + beta[c];  out[n, c] = 0.5 z (1 + erf(z / sqrt 2))   (the exact GELU)
 *   out[n, C + cs] = the bits of skip[n, cs].  mean, rstd (N C) are written for the backward.
 *   The variance is NEVER E[x^2] - E[x]^2: a thread holds its values in registers, subtracts the mean and sums the
 *   squares; a plane larger than one workgroup's registers is cut into chunks whose (mean, M2) are combined pairwise
 *   (Chan et al.).  A constant plane gives gelu(beta[c]); H W == 1 gives z = beta[c].
 *
 * waldo_plane_norm_gelu_bwd: grad_out is the gradient of the WHOLE out; its first C channels are read through gs_n,
 *   gs_c (the gradient of skip is the other channel slice: a view, no kernel).  With xhat = (x - mean) rstd,
 *   dz = grad_out gelu'(z),  gelu'(z) = Phi(z) + z phi(z):
 *     sums[n C + c] = (sum dz, sum dz xhat)                            (N C, 2): grad_beta, grad_gamma summed over n
 *     grad_x = rstd gamma (dz - sum dz / (H W) - xhat sum dz xhat / (H W))           (N, C, H, W) dense
 *
 * NO FLOAT ATOMICS: every sum is taken in an order fixed by the shapes -- all results are the same bits from run to
 * run.  Traffic: H W <= 8192: x (and grad_out) read once, one write; above: read twice, one write; nothing
 * tensor-sized in between.  workspace: waldo_plane_norm_workspace_bytes(N, C, H, W) for either call (0 for
 * H W <= 8192; -1 for a bad shape).  waldo_plane_norm_limits(out, n): writes the first n of the launcher's regime
 * boundaries, ascending (H W <= out[i] takes regime i; above the last: chunked), and returns how many there are.
 *
 * Caller-owned buffers and workspace, the caller's stream, no allocation, no synchronisation; N == 0: WALDO_OK
 * without a launch.  WALDO_EINVAL with a message before any launch: "bad shape" (N, Cs < 0; C, H, W < 1),
 * "too large" (H W > 2^30, or more than 2^31 - 1 workgroups), "negative stride", "bad stride" (os_n below
 * (C + Cs) H W), "bad eps", "null pointer", "not aligned" (a pointer off a 4-byte boundary; 16-byte loads and stores
 * are used when every pointer is 16-byte aligned and H W and the strides are multiples of 4, element accesses
 * otherwise), "workspace too small".
 * ------------------------------------------------------------------------------------- */
int waldo_plane_norm_limits(int* out, int n);
int64_t waldo_plane_norm_workspace_bytes(int64_t N, int C, int H, int W);
int waldo_plane_norm_gelu_fwd(const float* x, int64_t xs_n, int64_t xs_c, const float* gamma, const float* beta,
                              float eps, const float* skip, int64_t ss_n, int64_t ss_c, float* out, int64_t os_n,
                              float* mean, float* rstd, void* workspace, int64_t workspace_bytes, int64_t N, int C,
                              int Cs, int H, int W, waldo_stream_t stream);
int waldo_plane_norm_gelu_bwd(const float* x, int64_t xs_n, int64_t xs_c, const float* gamma, const float* beta,
                              const float* mean, const float* rstd, const float* grad_out, int64_t gs_n, int64_t gs_c,
                              float* grad_x, float* sums, void* workspace, int64_t workspace_bytes, int64_t N, int C,
                              int H, int W, waldo_stream_t stream);

/* The same with the tensor-sized buffers of element type `dtype` (enum waldo_dtype): a UNet under autocast.  Forward:
 * x, skip and out; backward: x, grad_out and grad_x -- as void*, their strides in ELEMENTS.  gamma, beta, mean, rstd,
 * sums and the workspace stay fp32, and so do every register and every sum: a 16-bit value is widened on load (exact),
 * the arithmetic is the fp32 entry point's, a result is rounded to nearest-even on the store (the bits of
 * `fp32_result.to(dtype)`; a NaN stays a NaN), and out[n, C + cs] is still the bits of skip[n, cs].  The regimes count
 * values: waldo_plane_norm_limits and waldo_plane_norm_workspace_bytes hold for every dtype.  16-byte loads and stores
 * -- 8 consecutive 16-bit values per lane -- when every typed pointer is 16-byte aligned and H W and the strides are
 * multiples of 8, element accesses otherwise; the in-lane sums then run over other elements than the fp32 layout's, in
 * an order that is just as fixed: the same bits from run to run, not the fp32 entry point's rounded.
 * WALDO_DTYPE_F32: exactly the fp32 entry point.  An unknown code: WALDO_EINVAL ("unknown dtype") before any pointer
 * is looked at.  "not aligned": a 16-bit buffer off a 2-byte boundary, any other off a 4-byte one (an odd-H W plane
 * reached through a channel slice is 2- but not 4-byte aligned, and is accepted).  Every other check as above. */
int waldo_plane_norm_gelu_fwd_dt(const void* x, int64_t xs_n, int64_t xs_c, const float* gamma, const float* beta,
                                 float eps, const void* skip, int64_t ss_n, int64_t ss_c, void* out, int64_t os_n,
                                 float* mean, float* rstd, void* workspace, int64_t workspace_bytes, int64_t N, int C,
                                 int Cs, int H, int W, int dtype, waldo_stream_t stream);
int waldo_plane_norm_gelu_bwd_dt(const void* x, int64_t xs_n, int64_t xs_c, const float* gamma, const float* beta,
                                 const float* mean, const float* rstd, const void* grad_out, int64_t gs_n,
                                 int64_t gs_c, void* grad_x, float* sums, void* workspace, int64_t workspace_bytes,
                                 int64_t N, int C, int H, int W, int dtype, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Token attention: the attention of the LVD transformer blocks (the reference's models/modules/transform.py:109-117
 * FullAttention and :175-185 ObjAttention: matmul -> scale -> softmax -> matmul, with the permutes of qkv / kv, the
 * cat of the two key sets and the transpose in front of proj) in one call, forward and backward.
 *
 * waldo_token_attention_fwd: for every b < B, h < H, i < Nq, over the keys j of segment 1 (Nk1 of them) FOLLOWED BY
 *   those of segment 2 (Nk2 of them; Nk2 == 0: k2, v2 and their strides are ignored and may be NULL / 0):
 *     out[b, i, h, :] = sum_j softmax_j(scale * q[b, i, h, :] . k[b, j, h, :]) v[b, j, h, :]
 *   Every operand is a VIEW, never copied: a pointer, a batch stride (x_b) and a token stride (x_n) in floats; heads
 *   are D floats apart and the D values of a (token, head) row are consecutive -- so q, k, v may be the three slices
 *   of one (B, N, 3 H D) qkv projection and k, v the two slices of a (B, N, 2 H D) kv projection.  out is
 *   (B, Nq, H D) contiguous, the layout the output projection takes.  D is 16, 32 or 64.
 *   fp32 throughout: both products on the exact-fp32 matrix instruction (k-ordered fma chains), the softmax online
 *   (a running maximum and sum per row; the keys past the end of a tile are masked with -inf, a row always has a
 *   live key).  NO SCORE MATRIX in memory, no workspace, no allocation, no synchronisation, NO ATOMICS: the same bits
 *   from run to run; the caller's stream; capturable in a graph.
 *   waldo_token_attention_limits(out, n): writes the first n of {query rows per workgroup, keys per tile, the head
 *   dimensions served (ascending)} and returns how many values there are.
 *
 * B == 0 or Nq == 0: WALDO_OK without a launch.  WALDO_EINVAL with a message before any launch: "bad shape" (B, Nq,
 * Nk2 < 0; H, Nk1 < 1), "bad head dimension", "bad scale" (not finite), "too large", "negative stride", "bad token
 * stride" (no multiple of 4 floats: rows are read in 16-byte pieces, and a view with a non-unit inner stride has no
 * description here), "bad batch stride" (no multiple of 4 floats), "null pointer", "not aligned" (a pointer off a
 * 16-byte boundary).
 *
 * waldo_token_attention_fwd_lse: the same call (one host body, one kernel template, the same bits in out) that also
 *   stores the row statistics the backward needs: lse (B, H, Nq) contiguous fp32,
 *     lse[b, h, i] = m + log(l) = log sum_j exp(scale * q[b, i, h, :] . k[b, j, h, :]).
 *   Its refusals are the forward's under its own name; "null pointer" covers lse.
 *
 * waldo_token_attention_bwd: the gradients of the forward in its five views, from out, grad_out (both (B, Nq, H D)
 *   contiguous) and lse.  Per (b, h), fp32 throughout, every product on the exact-fp32 matrix instruction:
 *     P = exp(scale S - lse)   dP = dO V^T   delta = rowsum(dO o O)   dS = P o (dP - delta)
 *     dQ = scale dS K          dK = scale dS^T Q                      dV = P^T dO
 *   grad_q (B, Nq, H, D), grad_k1 / grad_v1 (B, Nk1, H, D) and grad_k2 / grad_v2 (B, Nk2, H, D) are contiguous fp32 and
 *   are OVERWRITTEN; a NULL gradient pointer means that gradient is not wanted (all five NULL: WALDO_OK without a
 *   launch; Nk2 == 0: grad_k2 and grad_v2 are ignored).  The gradients are per batch element: a caller whose keys are
 *   broadcast over the batch (batch stride 0, legal for reading) sums them itself.  delta (B, H, Nq) is a workspace
 *   the caller allocates; nothing is allocated here.  Three launches at the most: the delta pass, a dQ kernel (skipped
 *   when grad_q is NULL) and a dK/dV kernel (skipped when the other four are NULL), each recomputing the scores from
 *   the views -- NO SCORE-SIZED MEMORY and NO ATOMICS: every gradient element is summed by one lane in one order, so
 *   the gradients are a function of the inputs alone, the same bits from run to run.  No synchronisation; the caller's
 *   stream; capturable in a graph.
 *   waldo_token_attention_bwd_limits(out, n): as waldo_token_attention_limits, for the backward's kernels: {query rows
 *   per workgroup of the dQ kernel (and per tile of the dK/dV kernel), keys per tile of the dQ kernel (and per
 *   workgroup of the dK/dV kernel), the head dimensions served}.
 *   Refusals: the forward's, under this function's name ("too large" also covers the key blocks of all (b, h) and the
 *   rows of out); "null pointer" also for out, grad_out, lse and delta; "not aligned" for every non-NULL pointer.
 * ------------------------------------------------------------------------------------- */
int waldo_token_attention_limits(int* out, int n);
int waldo_token_attention_fwd(const float* q, int64_t qs_b, int64_t qs_n, const float* k1, int64_t k1s_b, int64_t k1s_n,
                              const float* v1, int64_t v1s_b, int64_t v1s_n, const float* k2, int64_t k2s_b,
                              int64_t k2s_n, const float* v2, int64_t v2s_b, int64_t v2s_n, float* out, float scale,
                              int64_t B, int H, int D, int Nq, int Nk1, int Nk2, waldo_stream_t stream);
int waldo_token_attention_fwd_lse(const float* q, int64_t qs_b, int64_t qs_n, const float* k1, int64_t k1s_b,
                                  int64_t k1s_n, const float* v1, int64_t v1s_b, int64_t v1s_n, const float* k2,
                                  int64_t k2s_b, int64_t k2s_n, const float* v2, int64_t v2s_b, int64_t v2s_n, float* out,
                                  float* lse, float scale, int64_t B, int H, int D, int Nq, int Nk1, int Nk2,
                                  waldo_stream_t stream);
int waldo_token_attention_bwd_limits(int* out, int n);
int waldo_token_attention_bwd(const float* q, int64_t qs_b, int64_t qs_n, const float* k1, int64_t k1s_b, int64_t k1s_n,
                              const float* v1, int64_t v1s_b, int64_t v1s_n, const float* k2, int64_t k2s_b,
                              int64_t k2s_n, const float* v2, int64_t v2s_b, int64_t v2s_n, const float* out,
                              const float* grad_out, const float* lse, float* delta, float* grad_q, float* grad_k1,
                              float* grad_v1, float* grad_k2, float* grad_v2, float scale, int64_t B, int H, int D,
                              int Nq, int Nk1, int Nk2, waldo_stream_t stream);

/* Token attention on 16-bit operands: waldo_token_attention_fwd_dt is waldo_token_attention_fwd and
 * waldo_token_attention_clips_fwd_dt is waldo_token_attention_clips_fwd (next section) with q, k, v and out of ONE
 * 16-bit element type, dtype = WALDO_DTYPE_F16 or WALDO_DTYPE_BF16, passed as void*.  Strides are in ELEMENTS and are
 * multiples of 8 (rows are read in 16-byte pieces of 8 values); every pointer is on a 16-byte boundary; D is 16, 32 or
 * 64; the tiles are the fp32 kernel's (waldo_token_attention_dt_limits reports them as waldo_token_attention_limits
 * does).  Both products run on the 16-bit matrix instruction with fp32 accumulation:
 *   a score is an fp32 sum of exact 16-bit products; scale, mask, the running maximum and the running sum l are fp32,
 *   and l sums the unrounded p; p is rounded to the element type only as the operand of the second product; o is
 *   accumulated and rescaled in fp32; one rounding (nearest even; a NaN stays a NaN) at the store.
 * No score matrix, no workspace, no atomics: the same bits from run to run; the caller's stream; capturable in a graph.
 * A clip with queries and no keys gets NaN rows.
 *
 * The dense form has a backward.  waldo_token_attention_fwd_lse_dt is waldo_token_attention_fwd_dt with one more
 * output after out: lse (B, H, Nq) contiguous FP32, the row's m + log(l) of the scaled scores; out has the bits of
 * waldo_token_attention_fwd_dt's.  waldo_token_attention_bwd_dt is waldo_token_attention_bwd on such operands: the
 * views, out (the forward's STORED 16-bit out), grad_out (B, Nq, H D) contiguous and the five gradients -- contiguous
 * (B, N, H, D) tensors of the element type, OVERWRITTEN, NULL: not wanted -- are void*; lse and delta (B, H, Nq, the
 * call's only workspace) are float*.  One call makes three launches at the most (the delta pass, the dQ kernel unless
 * grad_q is NULL, the dK/dV kernel unless its four gradients are); no score-sized memory, no atomics -- every gradient
 * element is summed by one lane in one order.  Its arithmetic:
 *   delta[b, h, i] = sum_d dO[i, d] O[i, d], one fp32 fma chain over d; a recomputed score and dP = dO V^T are fp32
 *   sums of exact 16-bit products; P = exp(scale S - lse) and dS = P o (dP - delta) are fp32; dS and P are rounded to
 *   the element type ONLY as operands of dQ = dS K, dK = dS^T Q and of dV = P^T dO, which are accumulated in fp32;
 *   scale multiplies the fp32 accumulators of dQ and dK once, after the sum; one rounding (nearest even) at the store.
 * A batch stride of 0 is read as it is: gradients are per batch element.  All five gradients NULL, B == 0 or Nq == 0
 * return WALDO_OK without a launch.
 * The per-clip form has neither: there is no _lse form and no backward on 16-bit operands for
 * waldo_token_attention_clips_fwd_dt (its callers differentiate by recomputing in framework ops; the future layer
 * predictor's shapes are launch-bound and gain nothing from 16-bit kernels).
 * Refusals: WALDO_DTYPE_F32 ("is served by" the fp32 entry point, which the message names) and an unknown code
 * ("unknown dtype") before anything else; then the fp32 entry point's, in its order and words, with "a multiple of 8
 * values" for the strides ("null pointer" covers out, grad_out, lse and delta; "not aligned" every non-NULL pointer). */
int waldo_token_attention_dt_limits(int* out, int n);
int waldo_token_attention_fwd_dt(const void* q, int64_t qs_b, int64_t qs_n, const void* k1, int64_t k1s_b, int64_t k1s_n,
                                 const void* v1, int64_t v1s_b, int64_t v1s_n, const void* k2, int64_t k2s_b,
                                 int64_t k2s_n, const void* v2, int64_t v2s_b, int64_t v2s_n, void* out, float scale,
                                 int64_t B, int H, int D, int Nq, int Nk1, int Nk2, int dtype, waldo_stream_t stream);
int waldo_token_attention_fwd_lse_dt(const void* q, int64_t qs_b, int64_t qs_n, const void* k1, int64_t k1s_b,
                                     int64_t k1s_n, const void* v1, int64_t v1s_b, int64_t v1s_n, const void* k2,
                                     int64_t k2s_b, int64_t k2s_n, const void* v2, int64_t v2s_b, int64_t v2s_n, void* out,
                                     float* lse, float scale, int64_t B, int H, int D, int Nq, int Nk1, int Nk2, int dtype,
                                     waldo_stream_t stream);
int waldo_token_attention_bwd_dt(const void* q, int64_t qs_b, int64_t qs_n, const void* k1, int64_t k1s_b, int64_t k1s_n,
                                 const void* v1, int64_t v1s_b, int64_t v1s_n, const void* k2, int64_t k2s_b,
                                 int64_t k2s_n, const void* v2, int64_t v2s_b, int64_t v2s_n, const void* out,
                                 const void* grad_out, const float* lse, float* delta, void* grad_q, void* grad_k1,
                                 void* grad_v1, void* grad_k2, void* grad_v2, float scale, int64_t B, int H, int D,
                                 int Nq, int Nk1, int Nk2, int dtype, waldo_stream_t stream);
int waldo_token_attention_clips_fwd_dt(const void* q, int64_t qs_n, const void* k, int64_t ks_n, const void* v,
                                       int64_t vs_n, const int* q_off, const int* k_off, void* out, float scale,
                                       int64_t B, int H, int D, int64_t Rq, int64_t Rk, int max_q_len, int max_k_len,
                                       int dtype, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Token attention over clips: the attention of the future layer predictor's blocks (the reference's
 * models/modules/transform.py FullAttention / CrossAttention with ctx_mask: from_ctx -> attention over all T N keys
 * under a -inf mask -> to_ctx), as what those masks say: within a clip the selected query rows attend to the selected
 * key rows and nothing else survives.  The rows stay PACKED -- the selected frames' tokens of all clips one after the
 * other -- and a clip is a segment of them.  The kernels are the section above's (one template, the same tile
 * pipeline and arithmetic); only where a workgroup finds its rows differs.
 *
 * waldo_token_attention_clips_fwd: q is (Rq, H, D) and k, v are (Rk, H, D), VIEWS as above with a token stride in
 *   floats and no batch axis; q_off and k_off are int32 tables of B + 1 entries IN DEVICE MEMORY: clip b's queries are
 *   the rows [q_off[b], q_off[b + 1]) and its keys the rows [k_off[b], k_off[b + 1]).  For every clip b, h < H and
 *   query row i of the clip, over the clip's key rows j:
 *     out[i, h, :] = sum_j softmax_j(scale * q[i, h, :] . k[j, h, :]) v[j, h, :]
 *   out is (Rq, H D) contiguous.  max_q_len and max_k_len are the caller's upper bounds on a clip's rows; the grid is
 *   B x H x ceil(max_q_len / 64) and a workgroup whose block starts at or past its clip's last query returns at once;
 *   the key loop runs to the clip's own length.  A clip longer than its bound is served up to the bound only.
 *   The host never reads the tables: NO SYNCHRONISATION, no allocation, NO ATOMICS, the same bits from run to run, the
 *   caller's stream, capturable in a graph.  The kernels clamp every table entry into [0, Rq] / [0, Rk] and take a
 *   clip whose end lies before its start as empty, so that NO TABLE CONTENT makes them address a row outside the
 *   operands; rows that belong to no clip are not written.
 *   A clip without queries writes nothing.  A clip with queries and no keys gets NaN in exactly its rows of out (the
 *   softmax of a row whose keys are all masked) and -inf in lse.
 *   The tile sizes and head dimensions are waldo_token_attention_limits's.
 *
 * B == 0 or Rq == 0: WALDO_OK without a launch.  WALDO_EINVAL with a message before any launch: "bad shape" (B, Rq,
 * Rk < 0; H < 1), "bad clip bound" (max_q_len or max_k_len < 0), "bad head dimension", "bad scale", "too large",
 * "negative stride", "bad token stride", "null pointer" (a view, out, a table), "not aligned" (a view or out off a
 * 16-byte boundary).
 *
 * waldo_token_attention_clips_fwd_lse: the same call that also stores lse (H, Rq) contiguous fp32, the row's
 *   log sum_j exp(scale * q . k_j); "null pointer" covers lse.
 *
 * waldo_token_attention_clips_bwd: the gradients in the three views, from out, grad_out (both (Rq, H D) contiguous)
 *   and lse, by the section above's formulas and structure: a delta pass (delta (H, Rq): the caller's workspace), a dQ
 *   kernel and a dK/dV kernel whose workgroup owns a key block of ONE clip and walks that clip's query tiles (grid
 *   B x H x ceil(max_k_len / 64)).  grad_q (Rq, H, D) and grad_k / grad_v (Rk, H, D) are contiguous fp32 and are
 *   OVERWRITTEN in the rows that belong to a clip; a NULL gradient pointer means that gradient is not wanted (all
 *   three NULL: WALDO_OK without a launch).  The keys of a clip without queries get exact zeros; the queries of a clip
 *   without keys get zeros, and no other clip's gradients see that clip's NaN rows.  NO SCORE-SIZED MEMORY, no atomics,
 *   no synchronisation; the same bits from run to run; capturable in a graph.
 *   Refusals: the forward's, under this function's name ("too large" also covers the key blocks and the rows of out);
 *   "null pointer" also for out, grad_out, lse and delta; "not aligned" for every non-NULL pointer but the tables.
 * ------------------------------------------------------------------------------------- */
int waldo_token_attention_clips_fwd(const float* q, int64_t qs_n, const float* k, int64_t ks_n, const float* v,
                                    int64_t vs_n, const int* q_off, const int* k_off, float* out, float scale, int64_t B,
                                    int H, int D, int64_t Rq, int64_t Rk, int max_q_len, int max_k_len,
                                    waldo_stream_t stream);
int waldo_token_attention_clips_fwd_lse(const float* q, int64_t qs_n, const float* k, int64_t ks_n, const float* v,
                                        int64_t vs_n, const int* q_off, const int* k_off, float* out, float* lse,
                                        float scale, int64_t B, int H, int D, int64_t Rq, int64_t Rk, int max_q_len,
                                        int max_k_len, waldo_stream_t stream);
int waldo_token_attention_clips_bwd(const float* q, int64_t qs_n, const float* k, int64_t ks_n, const float* v,
                                    int64_t vs_n, const int* q_off, const int* k_off, const float* out,
                                    const float* grad_out, const float* lse, float* delta, float* grad_q, float* grad_k,
                                    float* grad_v, float scale, int64_t B, int H, int D, int64_t Rq, int64_t Rk,
                                    int max_q_len, int max_k_len, waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Pose objective: the three L1 terms of the future layer predictor's training step (models/synthesizer.py:752-754),
 *   (to_ctx(real, ~ctx_mask) - to_ctx(pred, ~ctx_mask)).abs().mean()   for obj_pose, bg_pose and occ_score,
 * as what the mask says: the mean of |real - pred| over the frames the mask does NOT select, without the gathers and
 * without their host reads.  Term k = 0, 1, 2 (obj, bg, occ) has a pair of dense fp32 tensors (F, E_k), F = B T frames
 * of E_k elements, addressed FLAT: no row alignment is assumed (E_occ = No can be 3, 5, 17) and only 4-byte alignment of
 * the pointers.  ctx_mask is F bytes in device memory; frame f is KEPT when ctx_mask[f] == 0.
 *
 * waldo_pose_l1_fwd: terms[k] = (sum over the kept frames f and e < E_k of |real_k[f, e] - pred_k[f, e]|)
 *                               / (kept * E_k),   kept = the number of kept frames, counted on the device;
 *   kept_out[0] = kept as a float (for the backward).  No kept frame: the three terms are NaN (0 / 0: the reference's
 *   mean of an empty selection).  The values of the other frames are never part of a sum (a NaN there changes nothing).
 *   Two launches: a partial per workgroup of 2048 elements into the workspace (the three terms in the same launch), then
 *   one workgroup that counts the mask and adds each term's partials in a fixed order.  NO ATOMICS: the same bits from
 *   run to run and in a graph replay.  workspace: waldo_pose_l1_workspace_bytes(F, E_obj, E_bg, E_occ) (0: bad sizes).
 *
 * waldo_pose_l1_bwd: ONE launch.  On a kept frame
 *     grad_pred_k[f, e] = sgn(pred_k - real_k) * (grad_terms[k] / (kept * E_k)),   sgn(0) = 0 (exact zero);
 *   on every other frame EXACT 0, whatever kept is (no kept frame: all-zero gradients, not NaN ones).  grad_terms[k] is
 *   grad_obj, grad_bg, grad_occ: one float each in device memory, NULL = that term carries no gradient (zeros are
 *   written).  grad_real_k = -grad_pred_k, written only where the pointer is not NULL (each of the three
 *   on its own: NULL = not wanted).  Every element of every gradient tensor passed is written; nothing needs a fill.
 *
 * Both: caller-owned buffers, the caller's stream, no allocation, no synchronisation, no memset node; capturable in a
 * graph.  WALDO_EINVAL with a message before any launch: "null pointer" (a pair, ctx_mask, terms, kept_out / kept,
 * a grad_pred, the workspace), "bad shape" (F <= 0 or an E_k <= 0), "too large" (F > 2^24 or F E_k > 2^31 - 1),
 * "workspace" (smaller than the query's answer).
 * ------------------------------------------------------------------------------------- */
int64_t waldo_pose_l1_workspace_bytes(int64_t F, int64_t E_obj, int64_t E_bg, int64_t E_occ);
int waldo_pose_l1_fwd(const float* real_obj, const float* pred_obj, const float* real_bg, const float* pred_bg,
                      const float* real_occ, const float* pred_occ, const uint8_t* ctx_mask, float* terms,
                      float* kept_out, void* workspace, int64_t workspace_bytes, int64_t F, int64_t E_obj, int64_t E_bg,
                      int64_t E_occ, waldo_stream_t stream);
int waldo_pose_l1_bwd(const float* real_obj, const float* pred_obj, const float* real_bg, const float* pred_bg,
                      const float* real_occ, const float* pred_occ, const uint8_t* ctx_mask, const float* kept,
                      const float* grad_obj, const float* grad_bg, const float* grad_occ, float* grad_pred_obj,
                      float* grad_pred_bg, float* grad_pred_occ, float* grad_real_obj, float* grad_real_bg,
                      float* grad_real_occ, int64_t F, int64_t E_obj, int64_t E_bg, int64_t E_occ,
                      waldo_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * LPIPS level distance: the tail of LPIPS at ONE feature level -- lpips.normalize_tensor of both maps, the squared
 * difference, the bias-free 1 x 1 "lin" convolution to one channel and spatial_average (eval mode: the dropout in front
 * of the lin layer is the identity).  f0, f1: dense fp32 (N, C, P), P = H W pixels of unit stride; w: (C,) fp32.
 * Per image n:
 *     n0[p] = sqrt(sum_c f0[c, p]^2),  m0 = n0 + eps  (eps is added AFTER the square root);   n1, m1 likewise from f1
 *     d[p]  = sum_c w[c] * (f0[c, p] / m0[p] - f1[c, p] / m1[p])^2
 *     out[n] = (1 / P) * sum_p d[p]
 * evaluated in this form (not as the expanded A / m0^2 - 2 B / (m0 m1) + Cc / m1^2, which cancels where the maps are
 * close): f1 == f0 gives out == 0 and an all-zero gradient exactly.  Only 4-byte alignment of the pointers and no
 * alignment of P are assumed (a lane reads a dword per channel).  The image base n C P is 64-bit, offsets inside an
 * image are 32-bit.
 * eps is taken as it is: eps == 0 is served (lanes past the end of a ragged tile take no part in any product), and
 * a pixel that is zero on every channel then gives NaN in out[n], as the chain's 0 / 0 does.
 *
 * waldo_lpips_level_fwd: two launches.  A workgroup owns a tile of 64 pixels of one image and stores one partial into the
 *   workspace; a finishing launch adds each image's partials in a fixed order and divides by P.  NO ATOMICS: the same
 *   bits from run to run and in a graph replay.  workspace: waldo_lpips_level_workspace_bytes(N, C, P) (0: a bad
 *   shape; a multiple of 256 otherwise).  saved: NULL, or (N, 3, P) fp32 of waldo_lpips_level_saved_bytes(N, C, P)
 *   bytes that receives, per pixel, what the backward needs to walk the maps once: 1 / m0 (0 where n0 == 0),
 *   1 / m1 and q = (sum_k w[k] e[k] f0[k, p]) / (n0 m0^2) (0 where n0 == 0),  e = f0 / m0 - f1 / m1.
 *
 * waldo_lpips_level_bwd: ONE launch; produces grad_f0 (N, C, P) only, from `saved` of the forward on the same operands.
 *   With g = grad_out[n] / P:
 *     grad_f0[c, p] = 2 g (w[c] e[c] / m0 - f0[c, p] / (n0 m0^2) * sum_k w[k] e[k] f0[k, p])
 *   and where n0[p] == 0 every channel of that pixel gets EXACT 0.  (The framework chain yields NaN there: the
 *   backward of sqrt at 0 is 0 / 0.  In LPIPS every tapped feature sits behind a ReLU whose backward turns either value
 *   into 0 -- an all-zero pixel is one the ReLU clipped on every channel -- so the deviation is invisible at the module.)
 *   Every element of grad_f0 is written; nothing needs a fill.  grad_f1 is the same call with f0 and f1 exchanged (and
 *   the `saved` of a forward with them exchanged): the distance is symmetric.
 *
 * Both: caller-owned buffers, the caller's stream, no allocation, no synchronisation; capturable in a graph.
 * WALDO_EINVAL with a message before any launch: "null pointer" (f0, f1, w, out, the workspace / saved, grad_out,
 * grad_f0), "bad shape" (N, C or P <= 0), "too large" (C P > 2^31 - 1, or N x ceil(P / 64) > 2^31 - 1 workgroups),
 * "workspace" (smaller than the query's answer).
 * ------------------------------------------------------------------------------------- */
int64_t waldo_lpips_level_workspace_bytes(int64_t N, int64_t C, int64_t P);
int64_t waldo_lpips_level_saved_bytes(int64_t N, int64_t C, int64_t P);
int waldo_lpips_level_fwd(const float* f0, const float* f1, const float* w, float* out, float* saved, void* workspace,
                          int64_t workspace_bytes, int64_t N, int64_t C, int64_t P, float eps, waldo_stream_t stream);
int waldo_lpips_level_bwd(const float* f0, const float* f1, const float* w, const float* saved, const float* grad_out,
                          float* grad_f0, int64_t N, int64_t C, int64_t P, waldo_stream_t stream);

/* -------------------------------------------------------------------------------------
 * LPIPS level distance in 16 bits: the two entry points above for maps stored in 16 bits, which is what a backbone
 * under autocast hands over.  f0, f1 and grad_f0 are `dtype` = WALDO_DTYPE_BF16 or WALDO_DTYPE_F16, dense (N, C, P);
 * w, out, saved (N, 3, P), the workspace's partials and grad_out stay fp32, and ALL arithmetic is fp32 on the exactly
 * widened elements.  The contract is the one above, word for word where it does not speak of the storage: the two-walk
 * form with e = f0 / m0 - f1 / m1, eps AFTER the square root, NO ATOMICS (the partials are added in a fixed order: the
 * same bits from run to run and in a graph replay), equal operands give exact zeros in the value and the gradient, a
 * pixel with n0[p] == 0 gets EXACT 0 on every channel (saved 1 / m0 = 0 marks it), eps == 0 is served on ragged
 * tiles, no limit on C beyond C P <= 2^31 - 1.
 *   Alignment: a lane reads ONE 2-byte element per channel.  Nothing assumes more than 2-byte alignment of f0, f1 or
 *   grad_f0, or an even P: odd planes (AlexNet's 127 x 255 taps) and views that start on an odd element are served by
 *   the same kernels as everything else.  There is one kernel form per dtype; nothing is chosen from the pointers.
 *   The tile is the fp32 kernels' 64 pixels: waldo_lpips_level_workspace_bytes and waldo_lpips_level_saved_bytes size
 *   the workspace and `saved` of these entry points too.
 *   Rounding: grad_f0[c, p] is the fp32 expression 2 g (w[c] e[c] / m0 - f0[c, p] q) rounded ONCE to nearest-even in
 *   `dtype`; for fp16 that includes the subnormals (no flush, no truncation).  The gradient of a mean over 2^19
 *   pixels is small: fp16 TRAINING NEEDS A SCALED LOSS (waldo_amd.optim's scaler), or most of grad_f0 rounds to
 *   subnormals and zeros.  bf16 has fp32's exponent range and needs none.
 * WALDO_EINVAL with a message before any launch: WALDO_DTYPE_F32 is refused with the name of the fp32 entry point
 * that serves it, any other code with "unknown dtype"; then "null pointer", "bad shape", "too large" and "workspace"
 * as above.
 * ------------------------------------------------------------------------------------- */
int waldo_lpips_level_fwd_dt(const void* f0, const void* f1, const float* w, float* out, float* saved, void* workspace,
                             int64_t workspace_bytes, int64_t N, int64_t C, int64_t P, float eps, int dtype,
                             waldo_stream_t stream);
int waldo_lpips_level_bwd_dt(const void* f0, const void* f1, const float* w, const float* saved, const float* grad_out,
                             void* grad_f0, int64_t N, int64_t C, int64_t P, int dtype, waldo_stream_t stream);

/* -------------------------------------------------------------------------------------
 * Clip augmentation (waldo_amd.augment; the reference's data/base_dataset.py:113-165 parameters, :330-370 transforms,
 * :173-208 layout and flow).  A training sample from a packed clip ("Packed clip" above) in ONE launch: crop, bilinear
 * resize, flips, colour jitter and normalisation of the frames, the resized layout logits, and the flow through its
 * two resizes.
 *   clip (B,T,Hd,Wd) 4-byte pixels; flow NULL or (B,T,2,Hf,Wf) fp32, normalised (read_flo's units), Hf <= Hd, Wf <= Wd;
 *   per-clip tables in DEVICE memory (they may change between the replays of a graph that holds the launch):
 *     box    (B,4) int32   [top, left, h_crop, w_crop] in clip pixels
 *     flip   (B)   uint8   bit 0: left-right (the reference's v_flip), bit 1: top-bottom (its h_flip)
 *     jitter (B,3) fp32    [brightness, saturation, hue]
 *     order  (B,T) uint8   0..5: the six orders of (brightness, saturation, hue), lexicographic
 *                          (0 BSH, 1 BHS, 2 SBH, 3 SHB, 4 HBS, 5 HSB); any other byte: no jitter for that frame
 *     zoom   (B)   fp32    the flow's multiplier
 *   out (B,T,3+Nl,Ho,Wo) fp32, the layout of the unpacked clip; flow_out NULL (with flow NULL) or (B,T,2,Ho,Wo) fp32.
 *
 * The kernel CLAMPS every box into the clip (the tables cannot be checked without a device read):
 *   top <- clamp(top, 0, Hd-1), h_crop <- clamp(h_crop, 1, Hd-top); left and w_crop likewise.
 * No value of any table moves a read outside the clip or the flow.
 *
 * Per output pixel (y, x) of a frame, all in fp32:
 *   xf = Wo-1-x under the left-right flip, else x;  sx = clamp((xf + 0.5) (w_crop / Wo) - 0.5, 0, w_crop-1);
 *   x0 = floor(sx), x1 = min(x0+1, w_crop-1), fx = sx - x0; rows likewise.  The four taps are pixels
 *   (top + y0|y1, left + x0|x1) with weights (1-fy|fy)(1-fx|fx): F.interpolate(bilinear, align_corners=False) on the
 *   CROPPED frame -- the taps clamp to the box, not to the image.
 *   RGB: u = (sum of weight x byte) / 255 per channel; then the frame's jitter operations in its order:
 *     brightness  u <- clamp(u f, 0, 1)
 *     saturation  u <- clamp(f u + (1-f) g, 0, 1),  g = 0.299 r + 0.587 g + 0.114 b
 *     hue         hexcone RGB -> HSV, h <- (h + hue) mod 1, HSV -> RGB (max == min: s = 0, the pixel is unchanged)
 *   then (u - 0.5) / 0.5.  (No contrast: it needs the frame's mean, a second pass.)
 *   Layout channel n: 5 (2 s_n - 1), s_n = the sum of the weights of the taps whose class byte is n -- the bilinear
 *   resize of the one-hot planes, which are never written.  A class byte >= Nl adds to no channel.
 *   Flow channel c: each of the four taps, at (Y, X) of the Hd x Wd grid, is the bilinear sample of the (Hf,Wf) flow at
 *   ((Y + 0.5) Hf / Hd - 0.5, (X + 0.5) Wf / Wd - 0.5) clamped to the flow's edges (the reference resizes the flow to
 *   the frame size first); the four are blended with the frame's weights, multiplied by zoom, and channel 0 is negated
 *   under the left-right flip, channel 1 under the top-bottom flip.  Two bilinear resizes composed, no intermediate.
 * With the full box, Ho x Wo = Hd x Wd, no flip and no jitter, `out` is waldo_unpack_clip_fwd's, bit for bit.
 *
 * Caller-owned buffers, the caller's stream, no allocation, no synchronisation; capturable in a graph.  B T == 0:
 * WALDO_OK without a launch.  WALDO_EINVAL with a message before any launch: "bad shape" (B or T < 0, Nl outside
 * [0, 32], a size outside [1, 32767]), "downsample" (Ho < Hd or Wo < Wd: with the boxes clamped into the clip the
 * resize then never shrinks, which would need an antialiasing filter), "flow larger than the clip" (Hf > Hd or
 * Wf > Wd), "null pointer" (anything but flow AND flow_out together), "too large" (more than 2^31 - 1 workgroups).
 * ------------------------------------------------------------------------------------- */
int waldo_augment_clip_fwd(const uint8_t* clip, const float* flow, const int32_t* box, const uint8_t* flip,
                           const float* jitter, const uint8_t* order, const float* zoom, float* out, float* flow_out,
                           int B, int T, int Nl, int Hd, int Wd, int Hf, int Wf, int Ho, int Wo, waldo_stream_t stream);

/* -------------------------------------------------------------------------------------
 * Optimizer step (waldo_amd.optim): what ends every training step of the reference (models/synthesizer.py:1057-1072,
 * :619-631, :765-778; the optimizer of create_optimizers, :114-143) -- the NaN test, GradScaler's unscale and update,
 * clip_grad_norm_ and torch.optim.Adam / AdamW -- on the device, with no host read.  Multi-tensor over n_tensors
 * (param, grad, exp_avg, exp_avg_sq) quadruples of fp32 of any sizes, in three phases on the caller's stream:
 *
 *   statistics  one pass over the gradients: per chunk of 4096 elements of a tensor the sum of squares and a non-finite
 *               flag (any NaN or +-inf element) into the workspace.  The chunk geometry depends on the sizes alone.
 *               16-byte loads where the tensor's base is 16-byte aligned, element loads for the numel % 4 tail and for a
 *               base that is only 4-byte aligned.  NO ATOMICS: the same bits from run to run and in a graph replay.
 *   finalize    ONE workgroup: adds the partials in index order in double, ORs the flags and isnan(*loss) (loss: NULL or
 *               a device pointer; the reference's test), and writes `state`; updates hyper[5], the scale.
 *   update      per element, only on a finite step (a skipped step writes NOTHING), torch.optim.Adam's single-tensor
 *               arithmetic in its order of operations:
 *                 adamw and wd[t] != 0:  p = p (1 - lr wd[t])                       (decoupled decay, per tensor)
 *                 g' = g mult                                                        (mult = clip_coef / scale)
 *                 m  = lerp(m, g', 1 - beta1)     = m + (1 - beta1)(g' - m), in torch.lerp's two forms
 *                 v  = beta2 v + ((1 - beta2) g') g'
 *                 p  = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
 *               amsgrad, maximize and L2-style decay are not offered.
 *
 * The tensors' pointers travel BY VALUE in the kernel arguments, at most K = 64 non-empty tensors per launch; a workgroup
 * finds its tensor from the pack's chunk prefix.  There is no pointer table in device memory: new gradient addresses at
 * every eager step need no refresh, and in a graph capture the addresses are baked into the nodes.  A step over n
 * non-empty tensors is 2 ceil(n / K) + 1 launches; *launches (a HOST int, or NULL) receives the count.  The host arrays
 * (params .. weight_decays; weight_decays NULL: no decay) are consumed during the call.
 *
 * state: WALDO_ADAM_STATE_WORDS fp32 in device memory, zeroed once by the caller, written by finalize:
 *   [0] step (finite steps so far; +1 on a finite step)   [1] grad norm = sqrt(sum) / scale, what clip_grad_norm_ sees
 *   [2] clip_coef = min(1, max_norm / (norm + 1e-6)) when max_norm > 0, else 1       after unscale_
 *   [3] mult = clip_coef / scale          [4] 1 on a finite step, 0 on a skipped one
 *   [5] bias_correction1 = 1 - beta1^step [6] sqrt(bias_correction2)   [7] lr / bias_correction1  (double, one lane)
 *   [8] skipped steps in a row (0 after a finite step)    [9] skipped steps in all
 *   [10] finite steps since the scale last changed (GradScaler's growth tracker)      [11..15] reserved
 * hyper: WALDO_ADAM_HYPER_WORDS fp32 in device memory, read at every step -- a scheduler changes them between the
 * replays of a graph without a recapture:
 *   [0] lr  [1] beta1  [2] beta2  [3] eps  [4] max_norm (<= 0: no clipping)
 *   [5] scale (the loss scale the gradients carry; 1 without a scaler; WRITTEN by finalize, GradScaler.update's rule:
 *       x backoff_factor on a non-finite step, x growth_factor after growth_interval finite steps in a row)
 *   [6] growth_factor  [7] backoff_factor  [8] growth_interval (0: the scale never grows)   [9..11] reserved
 *
 * waldo_adam_limits(out, n): writes the first n of {K, the chunk's elements, WALDO_ADAM_STATE_WORDS,
 * WALDO_ADAM_HYPER_WORDS} and returns how many there are.  waldo_adam_workspace_bytes(n_tensors, numels): 8 bytes per
 * chunk, a multiple of 256 and at least 256; 0 for bad sizes (a negative count or size, too many chunks).
 *
 * Caller-owned buffers, the caller's stream, no allocation, no synchronisation, no memset node; capturable in a graph.
 * WALDO_EINVAL with a message before any launch: "null pointer" (state, hyper, the workspace, an array, a buffer of a
 * non-empty tensor), "bad shape" (n_tensors or a size < 0; a tensor of 0 elements is allowed and skipped), "too large"
 * (more than 2^31 - 1 chunks), "not aligned" (a pointer off a 4-byte boundary, the workspace off 8), "workspace"
 * (smaller than the query's answer).
 * ------------------------------------------------------------------------------------- */
#define WALDO_ADAM_STATE_WORDS 16
#define WALDO_ADAM_HYPER_WORDS 12
int waldo_adam_limits(int* out, int n);
int64_t waldo_adam_workspace_bytes(int64_t n_tensors, const int64_t* numels);
int waldo_adam_step(float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                    const int64_t* numels, const float* weight_decays, int64_t n_tensors, float* state, float* hyper,
                    const float* loss, void* workspace, int64_t workspace_bytes, int adamw, int* launches,
                    waldo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* WALDO_HIP_H */
