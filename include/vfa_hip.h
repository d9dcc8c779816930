/*
 * vfa_hip.h -- C ABI of the MI355X (gfx950) multiview feature -> voxel projection + aggregation path.
 *
 * The reference (Jiahao-Ma/VFA) has no FFI on this path: its boundary is the Python call
 * VFA.forward (vfa/model/vfa_op.py:61-125) and the camera loop of VFANet.forward
 * (vfa/model/vfanet.py:64-82).  This header is the boundary the MI355X build introduces underneath
 * that call; vfa_amd/vfa_op.py binds it with ctypes (see INTEGRATION.md for the stub a maintainer of
 * the reference would add).  Each entry point names the reference lines it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch-ROCm allocations in practice);
 *     the library allocates nothing, keeps no global state (every tuning choice is a per-call flag) and is re-entrant;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is stream-ordered
 *     and asynchronous, nothing synchronises the device;
 *   - return value: 0 on success, otherwise a hipError_t (launch failure) or VFA_ERR_* (bad argument);
 *     nothing throws, nothing exits;
 *   - fp32 everywhere, with the rounding sequence of the reference's PyTorch CPU path (SURVEY.md
 *     Appendix A): the STAGE entry points (integral images, box parameters, vfa_gather_f32 / vfa_project_gather_f32 /
 *     vfa_pool_windows_f32: the voxel features) are bit-identical to the reference up to the sign of zero of masked
 *     voxels.  The FUSED frame entry points (vfa_pool_collapse_relu_sum_f32, vfa_pipe_collapse_relu_sum_f32) never
 *     write voxel features; inside them the tap chains and the box sum are the same exact sequence, but the quotient is
 *     v * RN(1 / area) where the reference divides: their on-chip voxel features are within ONE unit in the last place of
 *     the reference's (79-87 % of them identical: VFA_FLAG_DUMP_VOX, tests/test_fused_frame.py), and
 *     their output is compared with the reference within the post-GEMM tolerance (rtol 1e-4, atol 1e-5 max|ref|);
 *   - `n_views` batches cameras that share feature-map and grid shapes (one scale of one frame).
 * The consumers at the end of the header (BEV decode, the AP/AOS metric, the CLEAR-MOD metric) follow the same conventions; the
 * CLEAR-MOD entry point alone is float64, like the reference's numpy (vfa_clear_mod_frames_f64).
 *
 * Layouts
 *   feature   (n_views, C, Hf, Wf)          NCHW, as the reference's lateral maps
 *   integral  (n_views, Hf+2, Wf+2, C)      channels-last with a one-pixel ZERO border: one tap of one box is C
 *                                           contiguous floats and grid_sample's zeros padding is a plain load
 *   box       (n_views, nl, n_cells, 4)     left, top, right, bottom in normalised [-1,1] image coords
 *   area      (n_views, nl, n_cells)
 *   visible   (n_views, nl, n_cells)        0/1 bytes
 *   vox       (n_views, cell_count, nl*C)   column = layer*C + c (VFA_VOX_LAYER_MAJOR) or
 *                                           column = c*nl + layer (VFA_VOX_REFERENCE, vfa_op.py:120)
 */
#ifndef VFA_HIP_H
#define VFA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VFA_ABI_VERSION 9

/* world-unit conversion of the grid, reference vfa_op.py:23-44 (chosen by args.data) */
#define VFA_CONV_MULTIVIEWC 0 /* x / 1.0                                   */
#define VFA_CONV_MULTIVIEWX 1 /* x / 40.0 (true division)                  */
#define VFA_CONV_WILDTRACK 2  /* x*2.5-300, y*2.5-900, z*2.5               */

#define VFA_VOX_REFERENCE 0   /* vox[cell, c*nl + layer]   (vfa_op.py:120) */
#define VFA_VOX_LAYER_MAJOR 1 /* vox[cell, layer*C + c]    (coalesced; collapse.weight columns permuted by the host) */

/* optional kernel choice for vfa_project_gather_f32, OR-ed into vox_layout (same results bit for bit):
 * neither flag = library default (tap cache on single-layer grids with C = 256, direct kernel otherwise) */
#define VFA_VOX_KERNEL_DIRECT 0x100
#define VFA_VOX_KERNEL_TAP_CACHE 0x200

#define VFA_ERR_BAD_ARGUMENT 10001
#define VFA_ERR_UNSUPPORTED 10002 /* shape outside what a specialised kernel was built for; use the general entry points */

/* ABI version of the loaded library (VFA_ABI_VERSION at build time). */
int vfa_abi_version(void);

/* Per-call `flags` of the MFMA collapse entry points (there is no process-wide state):
 *   bits 0-3   arithmetic of the `collapse` product (reference: an fp32 nn.Linear, vfa_op.py:59, :123):
 *                0 / 2  (default) TWO FP16 PIECES per operand, three products hi.hi + hi.lo + lo.hi, fp32 accumulation -- with a
 *                       power-of-two scale per operand and feature scale the split is exact to 22 bits and the result has the error
 *                       of an sgemm (2e-7 normwise against float64 at K = 256): the reference's arithmetic width.  The fused frame
 *                       kernels only (vfa_pool_collapse_relu_sum_f32, vfa_pipe_collapse_relu_sum_f32 and their geometry calls);
 *                       the unfused product kernels (vfa_collapse_relu_sum_f32, vfa_collapse_gemm_*) read 0 as 3.
 *                3      two bf16 pieces, three products (16 bits: ~4e-6 normwise; inside the path's 1e-4 / 1e-5 tolerance)
 *                4      ... plus lo.lo
 *                6      three bf16 pieces, six products (sgemm class at twice the matrix work; vfa_pipe_* only)
 *   bits 8-15  VFA_FLAG_RESERVED_CUS(n): the persistent kernels (one workgroup per CU with all of its LDS) launch on at
 *              most n_cu - n CUs whenever that does not add a round of tiles.  Multi-GPU: leaves room for the RCCL
 *              kernels of the all-reduce that overlaps the next frame, which could otherwise only start at a kernel
 *              boundary.  Results are unchanged. */
#define VFA_FLAG_TERMS_MASK 0xf
#define VFA_FLAG_RESERVED_CUS(n) (((n) & 0xff) << 8)
/* vfa_pool_collapse_relu_sum_f32 only, DIAGNOSTIC: bits 16-27 select a profiling build of the kernel (phase ablations,
 * in-kernel cycle stamps written behind the records in the workspace); its results are meaningless.  tools/ use it. */
#define VFA_FLAG_DEBUG(mask) (((mask) & 0xfff) << 16)
/* Both fused entry points, for TESTS: with ONE view, ONE scale (and one layer) `out` receives the pooled fp32 voxel features (cell,
 * channel) exactly as the kernel's own pooling code forms them in front of the operand split, instead of the map (a diagnostic
 * build of the same source).  That is how the fused kernels' pre-GEMM arithmetic is compared with the reference's. */
#define VFA_FLAG_DUMP_VOX (1 << 30)
/* vfa_pool_collapse_relu_sum_f32 only: the entry point in two calls -- first ROWS_ONLY (the pre-pass over the direct items: needs
 * the box records of the frame, not its work cuts), later SKIP_ROWS (everything else).  Lets a caller that computes the geometry
 * on a second stream wait for vfa_frame_boxes_f32 before the first call and for vfa_frame_cuts_f32 only before the second. */
#define VFA_FLAG_ROWS_ONLY (1 << 28)
#define VFA_FLAG_SKIP_ROWS (1 << 29)
/* `flags` of vfa_project_gather_backward_f32: bit 0 = accumulate into grad_integral (otherwise it is zeroed first);
 * VFA_VOX_KERNEL_DIRECT selects the per-box atomic kernel instead of the LDS-privatised one (C = 256). */
#define VFA_BWD_ACCUMULATE 1

/* Integral image of every feature map: cumsum over W then over H, double accumulator rounded to
 * fp32 at every element (what ATen's CPU cumsum does), written channels-last inside a zero border.
 *                                                               replaces vfa_op.py:110, 172-173 */
int vfa_integral_image_f32(const float *feature, float *integral, int n_views, int C, int Hf, int Wf,
                           void *stream);

/* Producer fusion: the same integral image, of  relu(x * scale[v, c] + shift[v, c])  -- the GroupNorm
 * affine + ReLU of the lateral branch applied while the rows are scanned (two separately rounded fp32 operations), so the
 * lateral map is never materialised.  x (n_views, C, Hf, Wf) = the lateral 1x1-conv output; scale, shift (n_views, C) with
 * scale = gamma * rstd, shift = beta - mean * scale of the channel's group.   replaces vfanet.py:72-74 (norm + ReLU) + vfa_op.py:110 */
int vfa_affine_relu_integral_image_f32(const float *x, const float *scale, const float *shift, float *integral, int n_views, int C,
                                       int Hf, int Wf, void *stream);

/* The integral images of all the feature maps of a frame (one per stride) in ONE launch pair: features[s] (n_views, C, H_s, W_s),
 * integrals[s] (n_views, H_s + 2, W_s + 2, C), feat_hw = {H_0, W_0, H_1, W_1, ...} (host array), n_maps <= 4.  scales / shifts:
 * both NULL (plain maps, vfa_integral_image_f32 of each) or both arrays of n_maps device pointers (n_views, C) (producer fusion,
 * vfa_affine_relu_integral_image_f32 of each).  Results are bit-identical to the per-map entry points; the small maps share the
 * launch of the large one instead of paying a launch pair each.   replaces the three vfa_op.py:110 calls of vfanet.py:76-78 */
/* absmax (ABI v6): NULL, or a HOST array of n_maps device pointers (entries may be NULL), absmax[s] -> vfa_feature_stats_count(n_views,
 * C, H_s) uint32: the call leaves there partial maxima of |feature| (fp32 bit patterns, sign cleared; the maximum of all entries is
 * the map's largest |value| AFTER the affine + ReLU) -- the fused frame kernels scale their fp16 operand split by it.  No
 * initialisation needed, every entry is written. */
size_t vfa_feature_stats_count(int n_views, int C, int Hf);
int vfa_integral_images_f32(const float *const *features, const float *const *scales, const float *const *shifts,
                            float *const *integrals, unsigned *const *absmax, int n_views, int C, int n_maps, const int *feat_hw,
                            void *stream);
/* The same statistic from a finished integral image (n_views, Hf+2, Wf+2, C), for callers that kept no feature map: second
 * differences of the integral image, exact up to its rounding -- enough for a power-of-two scale.  absmax: as above. */
int vfa_integral_absmax_f32(const float *integral, unsigned *absmax, int n_views, int C, int Hf, int Wf, void *stream);

/* The same for CHANNELS-LAST inputs features_hwc[s] (n_views, H_s, W_s, C) -- what vfa_lateral_conv_f32 writes --: no NCHW copy of the
 * lateral convolution exists.  C a multiple of 64.  Bit-identical to vfa_integral_images_f32 of the permuted input. */
int vfa_integral_images_hwc_f32(const float *const *features_hwc, const float *const *scales, const float *const *shifts,
                                float *const *integrals, unsigned *const *absmax, int n_views, int C, int n_maps, const int *feat_hw,
                                void *stream);

/* The lateral branch of one feature scale, as far as the integral image needs it:
 *   y = conv1x1(feat) + bias            feat (n_views, K, Hf, Wf) NCHW (the trunk's output), weight (256, K) = lat.weight.view(256, K)
 *   out_hwc (n_views, Hf, Wf, 256) = y, channels-last;   scale, shift (n_views, 256): the nn.GroupNorm(16, 256) affine of y,
 *   scale = gamma * rstd(group), shift = beta - mean(group) * scale   (biased variance, eps inside the root)
 * so that relu(y * scale + shift) = relu(bn(lat(feat))) -- applied by vfa_integral_images_hwc_f32 while it scans the rows.
 * The product: six bf16 MFMA products of a three-piece split of both operands, fp32 accumulation (x = p0 + p1 + p2 to 2^-25 |x|; what
 * is dropped is <= 2^-23 of a product: the class of an sgemm); the statistics are gathered in the epilogue (double partial sums, added
 * in a fixed order: the same bits on every run).  K a multiple of 32, <= 1024.
 * workspace: vfa_lateral_conv_workspace_bytes(n_views, Hf, Wf).
 *   replaces vfa/model/vfanet.py:37-42, 72-74 (self.lat8/16/32 + self.bn8/16/32; the ReLU rides in the integral image) */
size_t vfa_lateral_conv_workspace_bytes(int n_views, int Hf, int Wf);
int vfa_lateral_conv_f32(const float *feat, const float *weight, const float *bias, const float *gamma, const float *beta, float eps,
                         float *out_hwc, float *scale, float *shift, void *workspace, size_t workspace_bytes, int n_views, int K,
                         int Hf, int Wf, void *stream);
/* The lateral branches of ALL the feature scales of a frame (n_maps <= 3) in three launches instead of three per scale: HOST arrays
 * of n_maps device pointers / values with the meaning of vfa_lateral_conv_f32's arguments, Ks[s], feat_hw = {H_0, W_0, H_1, W_1, ...},
 * workspaces[s] of vfa_lateral_conv_workspace_bytes(n_views, H_s, W_s) bytes each.  Bit-identical to the per-scale calls; the small
 * maps' workgroups fill the tail of the first (largest) map's instead of paying a launch of their own (ABI v7).
 *   replaces vfa/model/vfanet.py:72-74 for the three scales */
int vfa_lateral_convs_f32(int n_maps, const float *const *feats, const float *const *weights, const float *const *biases,
                          const float *const *gammas, const float *const *betas, const float *eps, float *const *outs_hwc,
                          float *const *scales, float *const *shifts, void *const *workspaces, const size_t *workspace_bytes, int n_views,
                          const int *Ks, const int *feat_hw, void *stream);

/* Training through the producer: the same three launches as vfa_lateral_convs_f32 -- y, scale and shift bit for
 * bit that call's --, plus the GroupNorm statistics the backward needs: means[s], rstds[s] (n_views, 16) DOUBLE, the mean and
 * 1 / sqrt(var + eps) of each (view, group) (biased variance) exactly as the scale and shift were formed from them.  Both arrays and
 * every entry required.  workspaces: vfa_lateral_conv_workspace_bytes, as above.
 *   replaces the forward of vfa/model/vfanet.py:37-42, 72-74 under autograd */
int vfa_lateral_convs_train_f32(int n_maps, const float *const *feats, const float *const *weights, const float *const *biases,
                                const float *const *gammas, const float *const *betas, const float *eps, float *const *outs_hwc,
                                float *const *scales, float *const *shifts, double *const *means, double *const *rstds,
                                void *const *workspaces, const size_t *workspace_bytes, int n_views, const int *Ks, const int *feat_hw,
                                void *stream);
/* The backward of the producer, from d integral straight to the gradients of the trunk map and of the branch's parameters, in two
 * calls per frame (HOST arrays of n_maps <= 3 entries, as vfa_lateral_convs_f32; C = 256, 16 groups, K a multiple of 32 and <= 1024):
 *
 * vfa_lateral_scan_backward_f32: grad_integrals[s] (n_views, H_s + 2, W_s + 2, 256) channels-last, 16-byte aligned (only the
 *   interior is read: the border carries no gradient) -> dzs_hwc[s] (n_views, H_s, W_s, 256) = the reverse cumsums along H, then W
 *   (vfa_integral_image_backward_f32's sequence, bit for bit, channels-last) times the ReLU mask [y * scale + shift > 0] recomputed
 *   in the forward row scan's two fp32 operations from ys_hwc, scales, shifts (vfa_lateral_convs_train_f32's outputs).  Per (view,
 *   channel) the sums S1 = sum dz and S2 = sum dz (y - mean) in double, added in a fixed order, give
 *     grad_betas[s] = sum_n S1,  grad_gammas[s] = sum_n rstd S2,  grad_biases[s] = d conv bias (the exact sum of d y below, in double)
 *   (each array NULL, or entries NULL, to skip), and the workspace keeps the coefficients of
 *     d y = (rstd gamma_c) dz - rstd^2 B_g (y - mean) - rstd A_g,  A_g = mean_g(gamma S1) / P,  B_g = rstd mean_g(gamma S2) / P
 *   for the second call.
 * vfa_lateral_conv_backward_f32: forms d y on the fly from dzs_hwc, ys_hwc, means and the workspace the scan call filled, then
 *     grad_feats[s]   (n_views, K_s, H_s, W_s) NCHW = W^T d y                 (the trunk map's gradient)
 *     grad_weights[s] (256, K_s)                    = sum over views and pixels of d y f^T
 *   six bf16 MFMA products of a three-piece split of both operands with fp32 accumulation (sgemm class); grad_weights from
 *   per-workgroup partials added in a fixed order.  Either array, or any entry, NULL: that product is not run (a frozen trunk pays no
 *   d f product).  feats[s] (n_views, K_s, H_s, W_s) and weights[s] (256, K_s) are the forward's inputs.
 * workspaces[s]: vfa_lateral_backward_workspace_bytes(n_views, K_s, H_s, W_s) bytes, 16-byte aligned, the SAME buffer for both calls of
 * a frame.  ys_hwc and dzs_hwc 16-byte aligned too (vfa_lateral_conv_backward_f32 reads them as float4).
 * No float atomics: both calls give the same bits on every run.  Errors: VFA_ERR_BAD_ARGUMENT (NULL required pointer, short workspace,
 * n_maps outside 1..3), VFA_ERR_UNSUPPORTED (K, alignment or size outside the limits above).
 *   replace the autograd of vfa/model/vfanet.py:37-42, 72-74 and vfa_op.py:172-173 under vfa/trainer.py:41 */
size_t vfa_lateral_backward_workspace_bytes(int n_views, int K, int Hf, int Wf);
int vfa_lateral_scan_backward_f32(int n_maps, const float *const *grad_integrals, const float *const *ys_hwc, const float *const *scales,
                                  const float *const *shifts, const double *const *means, const double *const *rstds,
                                  const float *const *gammas, float *const *dzs_hwc, float *const *grad_biases, float *const *grad_gammas,
                                  float *const *grad_betas, void *const *workspaces, const size_t *workspace_bytes, int n_views,
                                  const int *Ks, const int *feat_hw, void *stream);
int vfa_lateral_conv_backward_f32(int n_maps, const float *const *dzs_hwc, const float *const *ys_hwc, const double *const *means,
                                  const float *const *feats, const float *const *weights, float *const *grad_feats,
                                  float *const *grad_weights, void *const *workspaces, const size_t *workspace_bytes, int n_views,
                                  const int *Ks, const int *feat_hw, void *stream);

/* Cube corners -> world units -> 3x4 projection -> normalise/clamp -> 2-D bounding box, area and
 * visibility of every (view, layer, cell).                      replaces vfa_op.py:64-88, 104-106
 * and vfa/utils.py:50-59 (project).
 *   calibs (n_views, 3, 4); grid (n_cells, 3) cell origins in grid units; z_layers (nl);
 *   corner_off (8, 3) in generate_cube order (vfa_op.py:127-133); img_w/img_h = args.image_size[::-1]. */
int vfa_box_params_f32(const float *calibs, const float *grid, const float *z_layers, const float *corner_off,
                       int n_views, int n_cells, int nl, int conv_kind, float img_w, float img_h, int Hf, int Wf,
                       float cmin, float cmax, float *box, float *area, uint8_t *visible, void *stream);

/* Box pooling: four bilinear samples of the integral image at the box corners,
 * vox = (((lt + rb) - rt) - lb) / area * visible.               replaces vfa_op.py:112-120
 * Processes cells [cell_begin, cell_begin + cell_count) of every view so that the caller can bound
 * the size of `vox` on large grids. */
int vfa_gather_f32(const float *integral, const float *box, const float *area, const uint8_t *visible, float *vox,
                   int n_views, int C, int Hf, int Wf, int nl, int n_cells, int cell_begin, int cell_count,
                   int vox_layout, void *stream);

/* Fused form of the two entry points above: each workgroup computes the box parameters of its tile of
 * boxes itself (one thread per box) and stages them in LDS; box/area/visible never touch HBM.
 *                                                               replaces vfa_op.py:64-120 */
int vfa_project_gather_f32(const float *integral, const float *calibs, const float *grid, const float *z_layers,
                           const float *corner_off, float *vox, int n_views, int C, int Hf, int Wf, int nl,
                           int n_cells, int cell_begin, int cell_count, int conv_kind, float img_w, float img_h,
                           float cmin, float cmax, int vox_layout, void *stream);

/* Fused projection + box pooling + collapse product (fp32 MFMA) for C = c_out = 256:
 *   lin[view, cell, :] = sum_layer vox[view, cell, layer, :] . W_layer^T          (no bias, no ReLU)
 * without materialising vox.  weight_t is collapse.weight re-laid as (nl*C, c_out): row layer*C + c, i.e. the
 * transpose of the layer-major weight.  Voxel features are formed exactly as in vfa_project_gather_f32; the
 * product is a k-ordered fp32 fmaf chain (within the collapse tolerance, not bitwise -- no GEMM order is).
 * Returns VFA_ERR_UNSUPPORTED for other channel counts.               replaces vfa_op.py:64-123 */
int vfa_project_collapse_f32(const float *integral, const float *calibs, const float *grid, const float *z_layers,
                             const float *corner_off, const float *weight_t, float *lin, int n_views, int C, int Hf, int Wf,
                             int nl, int n_cells, int c_out, int conv_kind, float img_w, float img_h, float cmin, float cmax,
                             void *stream);

/* Two-kernel form of vfa_project_gather_f32: a records kernel writes one 128-byte record per box into `workspace`
 * (vfa_gather_workspace_bytes() bytes, caller-owned scratch) and the pooling waves fetch them with scalar loads.
 * Same results, bit for bit. */
size_t vfa_gather_workspace_bytes(int n_views, int nl, int cell_count);
int vfa_project_gather_ws_f32(const float *integral, const float *calibs, const float *grid, const float *z_layers,
                              const float *corner_off, float *vox, void *workspace, size_t workspace_bytes, int n_views,
                              int C, int Hf, int Wf, int nl, int n_cells, int cell_begin, int cell_count, int conv_kind,
                              float img_w, float img_h, float cmin, float cmax, int vox_layout, void *stream);

/* Backward of vfa_project_gather_f32 with respect to the integral images (training: the reference back-propagates
 * through the path with autograd, trainer.py:41; the gradient of calib and grid is vfa_project_gather_backward_geometry_f32's,
 * below).  grad_vox is layer-major
 * (n_views, cell_count, nl*C); grad_integral (n_views, Hf+2, Wf+2, C) is zeroed first unless VFA_BWD_ACCUMULATE is set in `flags`.
 * Scatter-add with float atomics: results are not bit-reproducible run to run (vfa_project_gather_backward_det_f32 below is). */
int vfa_project_gather_backward_f32(const float *grad_vox, const float *calibs, const float *grid, const float *z_layers,
                                    const float *corner_off, float *grad_integral, int n_views, int C, int Hf, int Wf,
                                    int nl, int n_cells, int cell_begin, int cell_count, int conv_kind, float img_w,
                                    float img_h, float cmin, float cmax, int flags, void *stream);
/* The same, told the width of the ground grid (ABI v9): grid_w = cells per row of the (rows, grid_w) grid the n_cells cells come from,
 * row-major (n_cells a multiple of it; 0 = unknown: as above).  The scatter then works on patches of 4 x 8 cells instead of cells in a
 * line: neighbouring boxes share taps in both directions, and the kernel runs at the rate of its atomic rows (bench frame: 1.7 / 0.9 /
 * 0.5 distinct taps per box on strides 8 / 16 / 32 against 4.5 / 2.7 / 1.7).  Same sums up to the order of the float atomics. */
int vfa_project_gather_backward_grid_f32(const float *grad_vox, const float *calibs, const float *grid, const float *z_layers,
                                    const float *corner_off, float *grad_integral, int n_views, int C, int Hf, int Wf,
                                    int nl, int n_cells, int cell_begin, int cell_count, int grid_w, int conv_kind, float img_w,
                                    float img_h, float cmin, float cmax, int flags, void *stream);

/* The same backward, bit-reproducible (what the Python layer runs under torch.use_deterministic_algorithms(True)): the arguments of
 * vfa_project_gather_backward_grid_f32 plus a caller-owned `workspace` of exactly
 * vfa_gather_backward_det_workspace_bytes(n_views, nl, cell_count, C, Hf, Wf) bytes (a function of the shapes alone: 16 sort
 * records of 20 bytes, 16 bytes of digit counts and 2 x 16 / 256 gradient rows per box; 0 = shapes beyond 2^31 records or 2^32 taps).
 * No float atomics: every box stores its 16 (tap, coefficient) records in fixed slots, a stable radix sort orders them by tap, and the
 * gradient rows of each tap's list are summed in list order (lists cut into fixed runs of 256 sorted positions, whose sums are added
 * in run order).  Contract:
 *   - the result is a function of the inputs and shapes only: not of timing, workgroup count, VFA_FLAG_RESERVED_CUS(n) (accepted,
 *     no effect: no kernel here is persistent), tensor addresses or the process;
 *   - VFA_BWD_ACCUMULATE: grad_integral = grad_integral + S with exactly one fp32 add per element a box touches, S = what the call
 *     writes without the flag (elements no box touches are left as they are); without it grad_integral is zeroed first;
 *   - masked boxes pass nothing: their grad_vox rows are never read and may hold anything;
 *   - any C, any cell range (grid_w is checked as above and otherwise unused); no stream sync, no device-to-host read;
 *   - a workspace of another size: VFA_ERR_BAD_ARGUMENT, nothing written.
 * Same sums as the atomic kernels up to rounding (not bitwise). `flags`: VFA_BWD_ACCUMULATE | VFA_FLAG_RESERVED_CUS(n). */
size_t vfa_gather_backward_det_workspace_bytes(int n_views, int nl, int cell_count, int C, int Hf, int Wf);
int vfa_project_gather_backward_det_f32(const float *grad_vox, const float *calibs, const float *grid, const float *z_layers,
                                        const float *corner_off, float *grad_integral, int n_views, int C, int Hf, int Wf, int nl,
                                        int n_cells, int cell_begin, int cell_count, int grid_w, int conv_kind, float img_w,
                                        float img_h, float cmin, float cmax, int flags, void *workspace, size_t workspace_bytes,
                                        void *stream);

/* Backward of vfa_project_gather_f32 with respect to the GEOMETRY: the camera matrices and the ground grid (the reference's
 * autograd differentiates vfa_op.py:64-119 with respect to calib and grid whenever they require grad).  Inputs: grad_vox layer-major
 * (n_views, cell_count, nl*C), the zero-bordered channels-last integral images the forward pooled from, and the geometry arguments and
 * cell range of the gather.  Outputs, either may be NULL:
 *   grad_calibs (n_views, 12) = d L / d calibs (row-major 3 x 4 per view), summed over the range's cells and layers;
 *   grad_grid   (cell_count, 3) = d L / d grid of the cells cell_begin .. cell_begin + cell_count - 1 (grid units: the world-unit
 *               gradient times the conversion's scale, 1 MultiviewC, 1/40 MultiviewX, 2.5 Wildtrack), summed over views and layers.
 * Per box: the corners are projected again with the forward's exact fp32 sequence (so the min / max, clamp and visibility decisions
 * are the forward's); the box edges get d vox . d vox / d edge from the 16 taps the forward pools (grid_sample's derivative with
 * respect to the sample point, and the area term); each edge's gradient goes to the corner torch.min / max selects (lowest index on
 * ties), through the clamp (passed where cmin <= value <= cmax), the normalisation and the perspective division.  z_layers and
 * corner_off get no gradient.  Contract:
 *   - bit-reproducible, no float atomics: the result is a function of the inputs and shapes only (a wave owns 8 cells and walks their
 *     views and layers in a fixed order; per-view partials go to fixed slots of `workspace` and are summed in slot order);
 *   - VFA_BWD_ACCUMULATE: out = out + S with exactly one fp32 add per element, S = what the call writes without the flag;
 *   - masked boxes pass nothing: their grad_vox rows are never read;
 *   - a box with a NaN corner (a camera plane through the cube) is masked in the forward and passes NOTHING here, where the
 *     reference's autograd would carry NaN into calib.grad and grid.grad: a deliberate difference (the gradient stays finite);
 *   - any C, any cell range; no stream sync, no device-to-host read;
 *   - `workspace`: at least vfa_gather_backward_geometry_workspace_bytes(n_views, cell_count) bytes when grad_calibs is non-NULL
 *     (48 bytes per view and 8 cells, rounded up to 256), otherwise unused (may be NULL).
 * `flags`: VFA_BWD_ACCUMULATE. */
size_t vfa_gather_backward_geometry_workspace_bytes(int n_views, int cell_count);
int vfa_project_gather_backward_geometry_f32(const float *grad_vox, const float *integral, const float *calibs, const float *grid,
                                             const float *z_layers, const float *corner_off, float *grad_calibs, float *grad_grid,
                                             int n_views, int C, int Hf, int Wf, int nl, int n_cells, int cell_begin, int cell_count,
                                             int conv_kind, float img_w, float img_h, float cmin, float cmax, int flags, void *workspace,
                                             size_t workspace_bytes, void *stream);

/* Column sums in a fixed order (the bias gradient of the deterministic backward):  out[n] = (accumulate ? out[n] : 0) + S[n],
 * S[n] = sum over r < rows of x[r, n], x (rows, N) row-major.  A workgroup owns 64 columns; its row slot k < K (K = 64 when 4 | N,
 * else 16) adds rows k, k + K, ... in row order, then the K slot sums are added pairwise in a fixed tree: bit-reproducible, the
 * same on every launch.  Accumulate: one add per column.  Parallel over columns only: a tall matrix with few columns is best
 * summed in two calls, over its (rows / B, B N) view and then over the (B, N) result (ops.column_sum does). */
int vfa_column_sum_f32(const float *x, float *out, long long rows, int N, int accumulate, void *stream);

/* Backward of vfa_integral_image_f32: reverse cumsum over H (in place on grad_integral, which is destroyed) then over
 * W, written as NCHW grad_feature (n_views, C, Hf, Wf). */
int vfa_integral_image_backward_f32(float *grad_integral, float *grad_feature, int n_views, int C, int Hf, int Wf,
                                    void *stream);

/* Backward of the two epilogues below with respect to `lin` and `bias` (per scale):
 *   grad_lin[v] = grad * (lin[v] + bias > 0);  grad_bias = column sums of grad_lin (zeroed first; NULL to skip).
 * grad (M, N); lin, grad_lin (n_views, M, N).  Needs 4 | N and N | 1024, otherwise VFA_ERR_UNSUPPORTED. */
int vfa_relu_mask_backward_f32(const float *grad, const float *lin, const float *bias, float *grad_lin, float *grad_bias,
                               int n_views, size_t M, int N, void *stream);

/* Epilogue of `collapse` for one VFA call batch:  out = (accumulate ? out : 0) + sum_v relu(lin[v] + bias)
 * with views added in index order.            replaces vfa_op.py:124 (ReLU) and vfanet.py:82 (view sum)
 *   lin (n_views, M, N) = vox . W^T without bias; bias (N) or NULL; out (M, N). */
int vfa_bias_relu_accumulate_f32(const float *lin, const float *bias, float *out, int n_views, size_t M, int N,
                                 int accumulate, void *stream);

/* Scale sum + view sum in the reference's order:
 *   ortho = sum_v ((relu(lin8[v]+b8) + relu(lin16[v]+b16)) + relu(lin32[v]+b32))
 *                                                               replaces vfanet.py:79 and :82 */
int vfa_scale_view_sum_f32(const float *lin8, const float *lin16, const float *lin32, const float *bias8,
                           const float *bias16, const float *bias32, float *ortho, int n_views, size_t M, int N,
                           int accumulate, void *stream);

/* Scale sum, then a MAXIMUM over views where the reference adds them (view_reduce="max"):
 *   t_v   = (relu(lin8[v]+b8) + relu(lin16[v]+b16)) + relu(lin32[v]+b32)     fp32, vfanet.py:79's order
 *   ortho = max over v of t_v, elementwise, views scanned in index order;  argmax[m, c] = the winning view (uint8)
 * The winner is torch.max(dim=0)'s index: the LOWEST view attaining the maximum (exact ties go to the first view), and a NaN in
 * any t_v makes the element NaN with the first NaN view as its winner.  n_views = 0 writes zeros (and winner 0), like the sum.
 *   lin* (n_views, M, N) = vox . W_s^T without bias; bias* (N) or NULL; ortho (M, N); argmax (M, N) bytes, or NULL to skip.
 * Limits: 0 <= n_views <= 256 (the winner is one byte), N > 0 (VFA_ERR_BAD_ARGUMENT otherwise, or for a NULL lin / ortho).
 * With 4 | N and 16-byte aligned lin / ortho (4-byte aligned argmax) one thread owns 4 channels; otherwise one channel.
 * The result is exact (a selection of the fp32 t_v): the same bits on every run.  Across processes that each hold some views
 * (a MAX all-reduce of the partial maps), ties resolve as here only through a global-index reduction of the winners
 * (vfa_amd.aggregate._AllReduceMax); a NaN's winner there is unspecified. */
int vfa_scale_view_max_f32(const float *lin8, const float *lin16, const float *lin32, const float *bias8, const float *bias16,
                           const float *bias32, float *ortho, uint8_t *argmax, int n_views, size_t M, int N, void *stream);

/* Backward of vfa_scale_view_max_f32 with respect to lin* and bias*:
 *   w = argmax[m, c];  grad_lin_s[w, m, c] = grad[m, c] * (lin_s[w, m, c] + b_s[c] > 0)  (strict: ReLU's gradient at 0 is 0);
 *   grad_lin_s[v, m, c] = 0 for every other view v.  Dense (n_views, M, N) rows, zeros included (the product backward reads them).
 * Only the winner's lin values are read.  A winner >= n_views (not one the forward writes) passes no gradient.
 * grad_bias* (N): the column sums of grad_lin_s over its n_views * M rows, in a fixed order (vfa_column_sum_f32; parallel over
 * columns only -- a caller with tall rows passes NULL and sums them itself, ops.scale_view_max_backward does); NULL to skip.
 * No float atomics anywhere: the results are bit-reproducible whatever the caller's determinism setting.
 * Limits and error codes as for the forward (VFA_ERR_BAD_ARGUMENT also for a NULL grad / lin / argmax / grad_lin). */
int vfa_scale_view_max_backward_f32(const float *grad, const float *lin8, const float *lin16, const float *lin32, const float *bias8,
                                    const float *bias16, const float *bias32, const uint8_t *argmax, float *grad_lin8,
                                    float *grad_lin16, float *grad_lin32, float *grad_bias8, float *grad_bias16, float *grad_bias32,
                                    int n_views, size_t M, int N, void *stream);

/* `collapse` + ReLU + view sum in one MFMA kernel, for K = N = 256 (single-layer grids, C = 256):
 *   out[m, :] = (accumulate ? out[m, :] : 0) + sum_v relu(vox[v, m, :] . weight^T + bias)
 *                                              replaces vfa_op.py:121-124 (Linear, ReLU) and vfanet.py:82 (view sum)
 *   vox (n_views, M, K) layer-major; weight (N, K) = collapse.weight (layer-major columns; identical to the reference's
 *   for one layer); bias (N) or NULL; out (M, N).
 * fp32 in, fp32 out, fp32 accumulation; each fp32 product is formed from `terms` bf16 MFMA products of an exact
 * hi/lo split of both operands (`flags` bits 0-3: 3 = default when 0 is passed, 4 adds lo*lo): error ~5e-6 of max|out| (the fp32 library
 * GEMM: 1e-6), inside the 1e-4 / 1e-5 max tolerance of the path; not bitwise -- no GEMM order is.  Inf inputs give
 * NaN (Inf - Inf in the split).  Returns VFA_ERR_UNSUPPORTED for other K, N: use a GEMM + the epilogues above. */
int vfa_collapse_relu_sum_f32(const float *vox, const float *weight, const float *bias, float *out, int n_views, size_t M,
                              int K, int N, int accumulate, int flags, void *stream);

/* The `collapse` product alone for any layer count:  lin[m, :] = vox[m, :] . weight^T,  m < M = n_views * cells,
 * K = nl * C a multiple of 128, N = 256 (other shapes: VFA_ERR_UNSUPPORTED, use a library GEMM).  No bias, no ReLU: the
 * two epilogue entry points above add them while summing views.         replaces vfa_op.py:121-123 (nn.Linear)
 * Same arithmetic as vfa_collapse_relu_sum_f32 (bf16-split MFMA, fp32 accumulation, same `flags`), as a K-looped
 * 128-row tile GEMM.  `workspace`: vfa_collapse_gemm_workspace_bytes(K, N) bytes of caller-owned scratch (the weight,
 * split into bf16 planes in MFMA fragment order, rewritten by every call). */
size_t vfa_collapse_gemm_workspace_bytes(int K, int N);
int vfa_collapse_gemm_f32(const float *vox, const float *weight, float *lin, void *workspace, size_t workspace_bytes, size_t M,
                          int K, int N, int flags, void *stream);

/* Training backward behind the fused forward (which kept no pre-activations): the same product, recomputed, with the ReLU mask as
 * its epilogue --  grad_lin (n_views, cells, 256) = (vox . weight^T + bias > 0) ? grad_out[cell] : 0,  grad_bias (256) += column
 * sums (atomics; may be NULL).  `lin` is never written.  vox (n_views * cells, K), weight (256, K), grad_out (cells, 256).
 *   replaces the autograd of vfa_op.py:123-124 (Linear + ReLU) for the gradient w.r.t. the pre-activation; trainer.py:41 */
int vfa_collapse_gemm_relu_backward_f32(const float *vox, const float *weight, const float *bias, const float *grad_out,
                                        float *grad_lin, float *grad_bias, void *workspace, size_t workspace_bytes, int n_views,
                                        size_t cells, int K, int N, int flags, void *stream);
/* The same with the product of the FUSED FRAME KERNELS -- two fp16 pieces per operand under the frame's power-of-two scales (ABI v8) --
 * so that the recomputed pre-activation, and with it the ReLU mask of the backward, is the forward's bit for bit: feat_absmax /
 * absmax_count = the feature statistics of this scale (vfa_integral_images_f32: what the frame kernel reduced to its 2^ea), row_shift
 * = the sliver shift of every row of the product (n_views * cells bytes: vfa_sliver_shifts_u8, its per-cell form repeated per view;
 * NULL: none), tile_any = one byte per 128 rows, non-zero where a row of that block has a shift (NULL: every row is looked up).  Operands,
 * scales, accumulator start (bias 2^(ea+ew-shift)) and the order of the three MFMA products are the forward's.  flags: reserved CUs. */
int vfa_collapse_gemm_relu_backward_f16_f32(const float *vox, const float *weight, const float *bias, const float *grad_out,
                                            float *grad_lin, float *grad_bias, void *workspace, size_t workspace_bytes, int n_views,
                                            size_t cells, int K, int N, const unsigned *feat_absmax, int absmax_count,
                                            const unsigned char *row_shift, const unsigned char *tile_any, int flags, void *stream);
/* The sliver shifts of a frame, per output row of that product (vfa_geom.h: sliver_shift): the binary places the
 * fp16 operand split of the frame kernels gave up for the noisiest visible box of the row's item.  per_item = 1: the serial kernel's
 * items (view, 8 x 4-cell tile) of ONE scale (feature map Hf x Wf), single-layer grids -> shift (n_views, L * W); per_item = 0: the
 * pipelined kernel's (tile, scale) over all views and layers -> shift (L * W), scratch = vfa_sliver_shifts_scratch_bytes(L, W) bytes.
 *   restates vfa_op.py:64-106 for the training backward; same device code as the geometry passes */
size_t vfa_sliver_shifts_scratch_bytes(int L, int W);
int vfa_sliver_shifts_u8(const float *calibs, const float *grid, const float *z_layers, int n_layers, const float *corner_off, int n_views,
                         int L, int W, int conv_kind, float img_w, float img_h, float cmin, float cmax, int Hf, int Wf, int per_item,
                         unsigned char *shift, void *scratch, size_t scratch_bytes, void *stream);

/* ---- single-layer grids (nl = 1), C = c_out = 256, inference: the whole frame in two launches ------------------------------
 *
 * vfa_frame_records_f32: geometry ONCE per frame.  Every (view, cell) cube is projected once (vfa_op.py:64-88,
 * utils.py:50-59) and turned, per feature scale, into a 96-byte box record (16 bilinear tap weights, 1 / area, visibility,
 * tap coordinates: vfa_op.py:104-106 and the set-up of the four F.grid_sample calls :112-115) plus, per (view, 8 x 4-cell
 * tile, scale), the window of the integral image holding the tile's taps; `weights[k]` (collapse.weight of scale k, (256,
 * 256) fp32, may be NULL as a whole to skip) is split into bf16 hi / lo planes in MFMA fragment order.  All of it goes to
 * `workspace` (vfa_frame_workspace_bytes() bytes of caller-owned device memory, valid until the next call that uses it).
 *   n_scales in 1..3; feat_hw = HOST array {Hf0, Wf0, Hf1, Wf1, ...}; weights = HOST array of n_scales device pointers.
 *   grid (L * W, 3) row-major; z_layers[0] is the single layer.  n_views <= 32 (else VFA_ERR_UNSUPPORTED).
 *
 * vfa_pool_collapse_relu_sum_f32: box pooling + Linear + bias + ReLU + view sum + scale sum in ONE persistent kernel,
 *   out[cell, :] = (accumulate ? out[cell, :] : 0) + sum_scale sum_view relu(vox_{scale,view}[cell, :] . W_scale^T + b_scale)
 *                                                replaces vfa_op.py:112-125 and vfanet.py:79, 82 for every scale and camera
 * The voxel features never reach HBM: per (tile, scale, view) the tap window is brought into LDS by LDS-DMA, the 32 boxes are
 * pooled with the reference's FMA chains into bf16 hi / lo planes and multiplied on the matrix cores (same bf16-split
 * arithmetic and `flags` as vfa_collapse_relu_sum_f32); the quotient is v * RN(1 / area) instead of a division (<= 1.5 ulp,
 * far below the split).  Results: within the path's post-GEMM tolerance, not bitwise.
 *   integrals / biases = HOST arrays of n_scales device pointers ((n_views, Hf+2, Wf+2, 256) each / (256) or NULL);
 *   workspace = what vfa_frame_records_f32 filled for the same (n_views, L, W, n_scales, feat_hw). */
size_t vfa_frame_workspace_bytes(int n_views, int L, int W, int n_scales);
/* (That is the recommended size.  The last region holds the pooled rows of the direct items -- tiles whose tap window exceeds LDS
 * -- 32 KiB per slot; any size from offsets[21] of vfa_frame_workspace_layout upwards is accepted by the three entry points
 * below, which derive the number of row slots from the size they are given: pass the SAME size to all of them.  Direct items
 * without a slot take a slower second launch.) */
/* Where things are inside that workspace (tests and tools/ read the records back): offsets[25]: offsets[5 k + {0..4}] = live-view
 * masks, direct-item masks, tile headers (32 B), box records (96 B), split weight of scale k; offsets[15] diagnostics, offsets[16]
 * total bytes; offsets[17 + k] = masks of the direct items without a row slot, offsets[20] the direct-item counter,
 * offsets[21] the pooled rows of the direct items (slot x 32 boxes x 256 fp32), offsets[22] = the number of row slots,
 * offsets[23] / [24] the work cuts (tile, rank of the first item inside it), tiles[3] + 1 of them;
 * tiles[4] = {tile rows, tile columns, tap-window capacity in slots, number of work pieces}.  Tiles are 4 x 8 cells. */
int vfa_frame_workspace_layout(int n_views, int L, int W, int n_scales, size_t *offsets, int *tiles);
int vfa_frame_records_f32(const float *calibs, const float *grid, const float *z_layers, const float *corner_off, int n_views, int L,
                          int W, int conv_kind, float img_w, float img_h, float cmin, float cmax, int n_scales,
                          const int *feat_hw, const float *const *weights, int flags, void *workspace, size_t workspace_bytes,
                          void *stream);
/* The same in two calls (vfa_frame_records_f32 = boxes, then cuts): vfa_frame_boxes_f32 projects the boxes and writes records,
 * headers, masks and the list of direct items; vfa_frame_cuts_f32 forms the work cuts of the persistent kernel from them and
 * splits the collapse weights (`weights` NULL: left as they are in the workspace).                 replaces vfa_op.py:64-106 */
int vfa_frame_boxes_f32(const float *calibs, const float *grid, const float *z_layers, const float *corner_off, int n_views, int L,
                        int W, int conv_kind, float img_w, float img_h, float cmin, float cmax, int n_scales,
                        const int *feat_hw, void *workspace, size_t workspace_bytes, void *stream);
int vfa_frame_cuts_f32(int n_views, int L, int W, int n_scales, const float *const *weights, int flags, void *workspace,
                       size_t workspace_bytes, void *stream);
/* (flags, ABI v6: VFA_FLAG_TERMS_MASK -- the arithmetic the weights are split for; pass what goes to vfa_pool_collapse_relu_sum_f32.
 * vfa_pool_collapse_relu_sum_f32 / vfa_pipe_collapse_relu_sum_f32 take `feat_absmax`: NULL, or a HOST array of n_scales device
 * pointers to the statistics vfa_integral_images_f32 left for the SAME integral images (entries may be NULL).  With the default
 * fp16 arithmetic a scale without statistics costs one extra pass over its integral image inside the call.) */
/* Box pooling alone from the same workspace: vox (n_views, L * W, 256) fp32, BIT-IDENTICAL to vfa_project_gather_f32 (layer-major,
 * nl = 1): four bilinear samples of the integral image of scale `scale`, (((lt + rb) - rt) - lb) / area * visible.
 *                                                                                            replaces vfa_op.py:112-120
 * One 64-channel quarter of one (view, tile) per workgroup; the tile's tap window comes in by LDS-DMA, so every distinct tap is
 * read from L2 / HBM once; bound by the HBM write of `vox`.  Hf, Wf must be the sizes the records of `scale` were built for. */
int vfa_pool_windows_f32(const float *integral, const void *workspace, size_t workspace_bytes, float *vox, int n_views, int L, int W,
                         int n_scales, int scale, int Hf, int Wf, void *stream);
int vfa_pool_collapse_relu_sum_f32(const float *const *integrals, const unsigned *const *feat_absmax, const float *const *biases,
                                   const void *workspace, size_t workspace_bytes, float *out, int n_views, int L, int W, int n_scales,
                                   const int *feat_hw, int accumulate, int flags, void *stream);

/* ---- the frame as a producer / consumer pipeline, any number of z-layers (vfa_pipe.hip) ----------------------------------------
 *
 * The inference hot path for C = 256 and ANY K = n_layers * 256 (the reference builds collapse = Linear(C * nl -> C),
 * vfa_op.py:50-59, and every shipped config has nl > 1: vfa/config.py:22-24, 49-52, 77-80):
 *
 *   vfa_pipe_boxes_f32     geometry once per frame: every (view, cell, LAYER) cube projected once, a 48-byte box record per scale
 *                          and a 32-byte tap-window header per (tile, layer, view, scale)        replaces vfa_op.py:64-106
 *   vfa_pipe_cuts_f32      cost-balanced work cuts + collapse.weight of every scale as 16-bit MFMA fragments (fp16 hi / lo under a
 *                          power-of-two scale by default, bf16 pieces for terms 3 / 4 / 6).
 *                          weights[k]: (256, 256 * n_layers) fp32 in the REFERENCE layout, column = c * n_layers + layer
 *                          (vfa_op.py:59, :120) -- no host-side permutation
 *   vfa_pipe_records_f32   both of the above
 *   vfa_pipe_collapse_relu_sum_f32
 *                          out (L * W, 256) (+)= sum_scale sum_view relu(vox . W^T + b): one persistent kernel, 16 waves per
 *                          CU -- eight pool boxes (the reference's exact fp32 FMA chains and its correctly rounded quotient)
 *                          while eight multiply the previous 64 rows x 64 channels on the matrix cores (default: two fp16 pieces
 *                          per operand under a power-of-two scale, three products, fp32 accumulation: the width of the reference's
 *                          fp32 nn.Linear; vfa_split.h).  The accumulators of a GROUP of four sub-tiles (a sub-tile = one live
 *                          view of one (tile, scale)) stay in registers across all layers: `relu` follows the whole
 *                          K = n_layers * 256.  Round 6: a group takes its sub-tiles from a RUN of 1, 2 or 4 consecutive tiles
 *                          (vfa_pipe_seq.h: run_tiles_of -- chosen per frame from n_views, the tile count and n_layers), so a frame
 *                          of one or two views (a rank's share of a camera-sharded rig) fills its groups from four tiles instead of
 *                          streaming the weight for one view's 32 rows; the voxel features never reach HBM
 *                                                                                replaces vfa_op.py:110-125, vfanet.py:79, 82
 *
 * workspace: caller-owned, vfa_pipe_workspace_bytes(); the geometry calls fill it, the kernel reads it and uses three areas of its
 * own: the CONTRIBUTIONS of a workgroup to the tiles of the run it is in (one 32-row x 256-column buffer per (tile of the run,
 * scale, group): plain stores at the end of a group, read back and added in (scale, group) order when the workgroup leaves the
 * run), the PARTS of a run cut between workgroups (every matrix wave stores its 32 columns, draws a ticket of its own, and the wave
 * that arrives last adds the parts in workgroup order and writes the tiles: nobody waits, no barrier), and the balance state.
 * integrals[k]: zero-bordered channels-last (n_views, Hf+2, Wf+2, 256).  n_views <= 32.  flags: VFA_FLAG_TERMS_MASK |
 * VFA_FLAG_RESERVED_CUS(n) | VFA_FLAG_DEBUG(mask) | VFA_FLAG_DUMP_VOX.  Terms: 0 / 2 = two fp16 pieces per operand, three products
 * (1e-7 ... 3e-7 normwise against float64: an fp32 sgemm's error); 3 = two bf16 pieces, three products (16-bit operands, ~3e-6 of
 * max|out|, inside the path's 1e-5 but narrower than the reference); 4 adds lo.lo; 6 = THREE bf16 pieces per operand (x = p0 + p1 +
 * p2 to 2^-25) and the six products down to 2^-16 of the largest, at twice the matrix work.  The geometry calls take the same terms
 * in `flags` (the weight fragments are split for one arithmetic, and the three-piece variant has smaller LDS tap windows; pass the
 * value that goes to vfa_pipe_collapse_relu_sum_f32: a launch that asks for the other arithmetic returns a map of NaNs).  Results are
 * deterministic for a given geometry, launch size and balance state; the association of the view / scale sum differs from
 * vfa_pool_collapse_relu_sum_f32's (inside the post-GEMM tolerance).
 *
 *   vfa_pipe_balance_f32   (ABI v5) mode 1: from the work cuts the geometry call has just left (estimated cost per group), the BOUNDS
 *                          of the workgroups' shares that minimise the heaviest share, for a launch of the size `reserved_cus`
 *                          gives; the frame kernel uses them for every later frame whose cuts have the same total cost and whose
 *                          launch has the same number of workgroups, and falls back to the uniform split otherwise (cameras and grid
 *                          of a frame stream stand still).  mode 0 clears the state: call it once on a fresh workspace (the geometry
 *                          calls never touch the state).  Deterministic.  Results stay inside the path's tolerance but are NOT
 *                          bitwise the unbalanced ones: a run cut between two workgroups is summed in another association when the
 *                          cut moves.  offsets[18] of vfa_pipe_workspace_layout: the state (8 KiB: int bounds[513], launch size,
 *                          cost signature; at byte 4096 a u64 cycle count per workgroup of the last launch: diagnostics), for
 *                          callers that keep one state per band of a banded frame.  offsets must hold 19 entries since ABI v5, 22
 *                          since ABI v8: offsets[19 + k] = the sliver shifts of scale k, one unsigned per tile (binary places the
 *                          fp16 operand split of the frame kernel gives up for the noisiest visible box of (tile, scale): 0
 *                          everywhere but next to boxes of ~1e-5 pixels).  VFA_AMD_PIPE_RT = 1 | 2 | 4 in the environment overrides
 *                          the run length (geometry call and frame kernel read it alike): measurements only. */
size_t vfa_pipe_workspace_bytes(int n_views, int L, int W, int n_layers, int n_scales);
int vfa_pipe_workspace_layout(int n_views, int L, int W, int n_layers, int n_scales, size_t *offsets, int *tiles);
int vfa_pipe_boxes_f32(const float *calibs, const float *grid, const float *z_layers, int n_layers, const float *corner_off, int n_views,
                       int L, int W, int conv_kind, float img_w, float img_h, float cmin, float cmax, int n_scales, const int *feat_hw,
                       int flags, void *workspace, size_t workspace_bytes, void *stream);
int vfa_pipe_cuts_f32(int n_views, int L, int W, int n_layers, int n_scales, const float *const *weights, int flags, void *workspace,
                      size_t workspace_bytes, void *stream);
int vfa_pipe_records_f32(const float *calibs, const float *grid, const float *z_layers, int n_layers, const float *corner_off,
                         int n_views, int L, int W, int conv_kind, float img_w, float img_h, float cmin, float cmax, int n_scales,
                         const int *feat_hw, const float *const *weights, int flags, void *workspace, size_t workspace_bytes, void *stream);
int vfa_pipe_collapse_relu_sum_f32(const float *const *integrals, const unsigned *const *feat_absmax, const float *const *biases,
                                   void *workspace, size_t workspace_bytes, float *out, int n_views, int L, int W, int n_layers,
                                   int n_scales, const int *feat_hw, int accumulate, int flags, void *stream);
int vfa_pipe_balance_f32(int n_views, int L, int W, int n_layers, int n_scales, int reserved_cus, int mode, void *workspace,
                         size_t workspace_bytes, void *stream);

/* ---- batched frames of a static rig: B frames in ONE pipelined launch (vfa_pipe.hip) ------------------------------------------------
 *
 * The geometry of a frame depends on the calibrations, the grid, the z-layers and the feature-map sizes only, so on a static rig it is
 * the same for every frame of a batch.  vfa_pipe_batch_records_f32 writes the box records and tap-window headers ONCE (the same bytes
 * vfa_pipe_boxes_f32 writes for one frame) and makes the work cuts over n_frames x n_tiles VIRTUAL tiles, frame-minor: t' = t * n_frames
 * + b, so consecutive tiles of a run share their records and tap-window geometry.  n_views <= 32 stays a per-frame limit (the view
 * masks are 32 bits); n_frames * n_views may exceed it.  It also leaves a batch record (frame count, run length, block count) that the
 * frame kernel takes its run length from.
 *
 * vfa_pipe_batch_collapse_relu_sum_f32: integrals[k] (n_frames * n_views, Hf+2, Wf+2, 256), frame-major (what vfa_integral_images_f32
 * makes of a stacked lateral batch); feat_absmax[k]: NULL or the statistics of that stacked batch; out (n_frames, L * W, 256).  Frame b
 * keeps its own arithmetic: the fp16 operand split of frame b uses the power of two a single-frame call on frame b would (its own
 * statistics; it rides on the sliver shift of its sub-tiles), so its products use the same pieces; only the association of the
 * cross-workgroup and view / scale sums may differ from vfa_pipe_collapse_relu_sum_f32 on that frame alone.  VFA_FLAG_DUMP_VOX: one
 * view, one scale, one layer; out receives every frame's voxel features.  A terms mismatch, like a workspace whose batch record is
 * not this batch's, gives a map of NaNs.
 *
 * The batched workspace is caller-owned and EXACTLY vfa_pipe_batch_workspace_bytes(n_frames, ...) bytes: every batched call refuses
 * another size (VFA_ERR_BAD_ARGUMENT), so a workspace made for one frame count cannot be launched with another.  Layout: offsets
 * [0, 22) as vfa_pipe_workspace_layout, offsets[22] the batch record, offsets[23] the per-frame split exponents (25 entries);
 * tiles[5] = the virtual tile count (6 entries).  vfa_pipe_batch_balance_f32: vfa_pipe_balance_f32 for a batched workspace. */
size_t vfa_pipe_batch_workspace_bytes(int n_frames, int n_views, int L, int W, int n_layers, int n_scales);
int vfa_pipe_batch_workspace_layout(int n_frames, int n_views, int L, int W, int n_layers, int n_scales, size_t *offsets, int *tiles);
int vfa_pipe_batch_records_f32(const float *calibs, const float *grid, const float *z_layers, int n_layers, const float *corner_off,
                               int n_views, int L, int W, int conv_kind, float img_w, float img_h, float cmin, float cmax, int n_scales,
                               const int *feat_hw, const float *const *weights, int n_frames, int flags, void *workspace,
                               size_t workspace_bytes, void *stream);
int vfa_pipe_batch_collapse_relu_sum_f32(const float *const *integrals, const unsigned *const *feat_absmax, const float *const *biases,
                                         void *workspace, size_t workspace_bytes, float *out, int n_frames, int n_views, int L, int W,
                                         int n_layers, int n_scales, const int *feat_hw, int accumulate, int flags, void *stream);
int vfa_pipe_batch_balance_f32(int n_frames, int n_views, int L, int W, int n_layers, int n_scales, int reserved_cus, int mode,
                               void *workspace, size_t workspace_bytes, void *stream);

/* The weight gradient of `collapse` (training):  g_w (256, K) (+)= g_lin^T . vox  with g_lin (rows, 256) the
 * masked output gradient (vfa_relu_mask_backward_f32 / vfa_collapse_gemm_relu_backward_f32) and vox (rows, K) the voxel features of
 * the same rows, K = n_layers * 256 in the column order of the weight passed to the forward.  Six bf16 MFMA products of a three-piece
 * split of both operands, fp32 accumulation (sgemm class); per-workgroup partial sums added in a fixed order (the same bits on every
 * run).  workspace: vfa_grad_weight_workspace_bytes(rows, K).  K a multiple of 256 (ABI v7).
 *   replaces the autograd of nn.Linear's weight, vfa/model/vfa_op.py:59, :123 under vfa/trainer.py:41 */
size_t vfa_grad_weight_workspace_bytes(long long rows, int K);
int vfa_grad_weight_f32(const float *g_lin, const float *vox, float *g_w, long long rows, int K, int accumulate, void *workspace,
                        size_t workspace_bytes, void *stream);
/* ... and of its input:  g_vox (rows, K) = g_lin (rows, 256) . w (256, K), w = the weight in the column order of the forward.  The same
 * six-product arithmetic; workspace: vfa_grad_input_workspace_bytes(K) (the weight as three bf16 planes in MFMA fragment order,
 * rebuilt by every call).  K a multiple of 256, g_lin 16-byte aligned (ABI v7).
 *   replaces the autograd of nn.Linear's input, vfa/model/vfa_op.py:123 under vfa/trainer.py:41 */
size_t vfa_grad_input_workspace_bytes(int K);
int vfa_grad_input_f32(const float *g_lin, const float *w, float *g_vox, long long rows, int K, void *workspace, size_t workspace_bytes,
                       void *stream);

/* ---- consumers of the path ---------------------------------------------------------------------------
 *
 * vfa_sort_vertices_f32: anticlockwise order of the valid vertices of n convex polygons per batch entry (rectangle x rectangle
 * intersections of the AP/AOS metric).                       replaces vfa/evaluation/pyeval/cuda_op/sort_vert_kernel.cu:42-140
 *   vertices (b, n, m, 2) fp32 normalised around the polygon centre; mask (b, n, m) bytes (1 = valid candidate, the first 8 are box
 *   corners, the rest edge intersections); num_valid (b, n) int32; idx (b, n, 9) int32 out: the sorted indices, the first one
 *   repeated, then padded with an invalid intersection index.  m > 8.  Same selection rule, comparison and corner cases as the
 *   reference kernel; one lane per polygon.
 *
 * vfa_bev_nms_f32: conf (L, W) = sigmoid(heatmap) where it equals its 5 x 5 max-pool (padding 2), else 0.
 *                                                            replaces vfa/data/encoder.py:230-232 + the sigmoid of :238 / :278 */
int vfa_sort_vertices_f32(const float *vertices, const uint8_t *mask, const int *num_valid, int *idx, int b, int n, int m, void *stream);
int vfa_bev_nms_f32(const float *heatmap, float *conf, int L, int W, void *stream);
/* vfa_bev_nms_batch_f32: the same for B maps (B, L, W) in one launch; the 5 x 5 window never crosses from one frame into the next. */
int vfa_bev_nms_batch_f32(const float *heatmap, float *conf, int B, int L, int W, void *stream);

/* ---- the AP/AOS metric: rotated-box 3D IoU and the best ground truth of every detection ---------------------------------------
 *
 * A box is 7 floats  x y z l w h alpha  (centre, footprint l x w rotated by alpha around z, height h).  ONE LANE computes the
 * whole IoU3D of one pair (corners, 16 edge intersections, corner-inside tests, 24 candidate vertices, their ordering by the device
 * code of vfa_sort_vertices_f32, shoelace, union, z overlap); the candidates stay in LDS, memory sees the boxes and the results.
 * fp32, one operation per reference operation in the reference's order, no contraction; cosf / sinf are the device's, so the
 * reference's numbers are met within a tolerance, not bit for bit.  No atomics: every call gives the same bits on every run.
 *
 * vfa_iou3d_f32: elementwise.  box1, box2 (count, 7); iou3d (count) out; iou_bev (count) out or NULL: the IoU of the footprints
 * (the first result of IoUs2D).                              replaces vfa/evaluation/pyeval/IoU.py:6-225 for one pair per lane
 *   - the z overlap  min(zmax) - max(zmin)  is NOT clamped, like the reference's: boxes apart in z whose footprints overlap give a
 *     NEGATIVE IoU (above -1), which no positive threshold accepts;
 *   - footprints that do not meet give exactly 0 (never NaN); a NaN in any field of either box gives NaN in iou3d (a NaN in z or h:
 *     in iou3d only); boxes of zero area give 0 / 0 = NaN like the reference;
 *   - count == 0 returns 0 and touches nothing; count < 0 or a NULL box1 / box2 / iou3d: VFA_ERR_BAD_ARGUMENT; more than
 *     2^31 - 1 blocks of 64 pairs: VFA_ERR_UNSUPPORTED.
 *
 * vfa_iou3d_frames_f32: a whole evaluation set in one call.  det (n_det, 7) and gt (n_gt, 7), both sorted by frame; det_begin,
 * gt_begin (n_frames + 1) int32 CSR offsets of the frames' rows; pair_begin (n_frames + 1) int64: offset of each frame's
 * (P_f, G_f) IoU matrix (detection-major) in the packed output iou (n_pairs), n_pairs = pair_begin[n_frames] = sum P_f * G_f.
 *                                                            replaces the loops of vfa/evaluation/pyeval/evaluateAPAOS.py:74-92
 *   - iou != NULL: one lane per pair fills the matrices;
 *   - best_idx (n_det) int32 and best_iou (n_det) != NULL: per detection the LOWEST-INDEX MAXIMUM of its row: best_idx =
 *     frame-local index of that ground truth, best_iou its IoU; a NaN never wins; best_idx = -1 and best_iou = -1 when the frame
 *     has no ground truth or every IoU of the row is NaN.  Detections outside [det_begin[0], det_begin[n_frames]) get -1 / -1.
 *     16 lanes share a row and combine by value, then by lowest index: what a scan in index order keeps, whatever the order of
 *     the combination;
 *   - iou == NULL: no matrix is written or read (pair_begin may be NULL, n_pairs is ignored): the detection's lanes compute its
 *     row themselves with the same device function on the same operands, so best_idx / best_iou have the bits of the matrix form;
 *   - best_idx == NULL and best_iou == NULL: only the matrices.  One of the two NULL: VFA_ERR_BAD_ARGUMENT.
 * Why one best match serves every threshold: the reference keeps pair j when  iou >= thresh and iou > max_iou  with max_iou
 * starting at -1 (evaluateAPAOS.py:80-87); for any thresh > 0 that is "the first j that attains the row's maximum, if that maximum
 * is >= thresh".  So the thresholds 0.75 / 0.5 / 0.25 share one argmax and differ in one comparison of best_iou (the host wrapper
 * refuses thresholds <= 0, for which the equivalence does not hold).
 * Limits and errors: negative counts, a NULL det / det_begin / gt_begin (or gt with n_gt > 0, or pair_begin with iou):
 * VFA_ERR_BAD_ARGUMENT; n_frames == 0 or n_det == 0 returns 0.  Offsets that leave [0, n_det] / [0, n_gt] / [0, n_pairs) are not
 * followed (such a frame's outputs are left unwritten, or -1): a wrong table cannot make the kernels read or write out of bounds. */
int vfa_iou3d_f32(const float *box1, const float *box2, float *iou3d, float *iou_bev, long long count, void *stream);
int vfa_iou3d_frames_f32(const float *det, const int *det_begin, const float *gt, const int *gt_begin, int n_frames, int n_det, int n_gt,
                         const long long *pair_begin, long long n_pairs, float *iou, int *best_idx, float *best_iou, void *stream);

/* ---- the CLEAR-MOD metric (MODA / MODP): distances and the Hungarian assignment of every frame --------------------------------
 *
 * vfa_clear_mod_frames_f64: the match tables of a whole 2D evaluation set in one launch, ONE WAVE PER FRAME (grid = n_frames; the
 * workgroups share nothing: no atomics, no workspace, the same bits on every run).
 *                                                            replaces the frame loop of vfa/evaluation/pyeval/CLEAR_MOD_HUN.py:44-93
 *   det_xy (n_det, 2), gt_xy (n_gt, 2) float64 ground positions, rows sorted by frame; det_begin, gt_begin (n_frames + 1) int32 CSR
 *   offsets of the frames' rows, as vfa_iou3d_frames_f32 takes them; td the distance threshold (the reference's 30).
 *   Per frame, in float64 like the reference's numpy:
 *   - d(o, e) = sqrt((gx - ex) * (gx - ex) + (gy - ey) * (gy - ey)), no contraction: the bits of numpy's sqrt (:6-7, :63);
 *   - cost = d > td ? 1e6 : d (:69); a non-finite distance costs 1e6 too (a deviation: the reference lets scipy raise);
 *   - the minimum-cost assignment of min(G_f, P_f) pairs, what scipy.optimize.linear_sum_assignment solves (:72): shortest
 *     augmenting paths with duals (Jonker-Volgenant), the smaller side as rows, the lanes spread over the columns, the lowest
 *     column index on a tie; duals, slacks, predecessors and both match arrays in LDS, the cost matrix too when rows * cols <=
 *     2048, otherwise costs are computed again from the frame's coordinates in LDS.  Every loop is bounded (at most rows
 *     augmentations of at most cols + 1 steps) whatever the costs are;
 *   - a pair is a match when its assigned cost is < td (:73).  Kept quirk: a pair at exactly td keeps the cost td, competes in
 *     the assignment and is NOT a match.  Among assignments of equal cost the choice is unspecified, here as in scipy.
 *   Out:
 *   - gt_match (n_gt) int32: frame-local index of the matched detection, or -1; gt_dist (n_gt) float64: its distance, +inf where
 *     unmatched (the reference's `distances`, :42, :91);
 *   - frame_counts (n_frames, 4) int64: G_f, P_f, c = number of matches, number of pairs assigned at 1e6 (fp = P_f - c and
 *     m = G_f - c are the reference's :92-93); frame_cost (n_frames) float64: sum of the assigned costs below 1e6, added in
 *     ground-truth order; frame_status (n_frames) int32, 0 or one of VFA_CLEAR_MOD_*;
 *   - dist (n_pairs) float64 or NULL: the frames' distance matrices before the threshold, ground-truth-major like the reference's
 *     dist[o, e]; pair_begin (n_frames + 1) int64 their offsets, n_pairs = sum G_f * P_f (a matrix that would leave [0, n_pairs) is
 *     not written).
 *   Limits: frames up to max(P_f, G_f) <= VFA_CLEAR_MOD_MAX_SIDE.  A larger frame gets status VFA_CLEAR_MOD_TOO_LARGE, -1 / +inf in
 *   its rows of gt_match / gt_dist, and nothing else of it is written.  Offsets that are not non-decreasing within [0, n_det] /
 *   [0, n_gt] are not followed: status VFA_CLEAR_MOD_BAD_OFFSETS and nothing else written.  VFA_CLEAR_MOD_SOLVER_FLAG: a loop of
 *   the solver met its bound (not reachable with finite td; the tables of that frame are not to be used).  Rows outside
 *   [gt_begin[0], gt_begin[n_frames]) are not touched.
 *   Errors: negative counts or a NULL required pointer (pair_begin with dist): VFA_ERR_BAD_ARGUMENT; n_frames == 0 returns 0. */
#define VFA_CLEAR_MOD_MAX_SIDE 512
#define VFA_CLEAR_MOD_TOO_LARGE 1
#define VFA_CLEAR_MOD_BAD_OFFSETS 2
#define VFA_CLEAR_MOD_SOLVER_FLAG 3
int vfa_clear_mod_frames_f64(const double *det_xy, const int *det_begin, const double *gt_xy, const int *gt_begin, int n_frames, int n_det,
                             int n_gt, double td, const long long *pair_begin, long long n_pairs, double *dist, int *gt_match,
                             double *gt_dist, long long *frame_counts, double *frame_cost, int *frame_status, void *stream);

/* ---- the BEV decode: heads of a batch of frames -> detections, outputs of a fixed shape ----------------------------------------
 *
 * vfa_bev_decode_f32: peaks, top-k, box arithmetic and the rotation arg-max of B frames in one stream-ordered call: two launches
 * (the kernel of vfa_bev_nms_batch_f32 into the workspace, then one workgroup per frame), no allocation, no host round trip, no
 * atomics on memory: the same bits on every run.  Nothing crosses from one frame into another.
 *                                                            replaces vfa/data/encoder.py:234-305 (decode3d / decode2d)
 *   heatmap (B, 1, L, W) logits, contiguous.  loc_offset (B, L, W, 2), dim_offset (B, L, W, 3), rotation (B, L, W, n_rot) logits,
 *   each read through four ELEMENT strides {frame, cell row, cell column, channel} given as a HOST array, so a permute(0, 2, 3, 1)
 *   view of NCHW storage and a contiguous NHWC tensor are taken alike and no head is ever copied.  dim_offset == rotation == NULL:
 *   2D (dim_stride, rot_stride, dimension_mean, dimension, rotation_out are then ignored).  dimension_mean: 3 floats on the HOST.
 *   Per frame, k = min(topk, L * W):
 *   - conf[l, w] is what vfa_bev_nms_batch_f32 writes, bit for bit; a CANDIDATE is a cell with conf > cls_thresh;
 *   - the k candidates that come first by confidence descending, equal confidences by ascending flat cell index l * W + w, in that
 *     order: exact for any number of candidates (a constant map gives cells 0 .. k - 1).  For cls_thresh >= 0 this is the
 *     reference's top-k followed by its threshold, with the order among equal confidences (which torch.topk leaves open) fixed;
 *   - per selected cell, fp32, one operation per reference operation, s(x) = 1.0f / (1.0f + expf(-x)):
 *       cy = (l + s(loc[0])) / grid0 * world0,  cx = (w + s(loc[1])) / grid1 * world1,
 *       location = (cx, cy, 0), or (cy, cx, 0) with yx_first != 0 (the reference's 2D Wildtrack);
 *       dimension[j] = expf(dim[j]) * dimension_mean[j];
 *       rotation = (float)argmax * (float)(pi / 180), the arg-max over s(rotation[0 .. n_rot)), the FIRST index that attains the
 *       maximum (saturated logits tie at 1.0f like the reference's); a NaN never wins, all NaN gives index 0.
 *   Out, all written by the call: count (B) int32 = number of detections of the frame; conf (B, k); location (B, k, 3); cell (B, k)
 *   int32 = l * W + w; in 3D dimension (B, k, 3) and rotation_out (B, k).  Rows from count[b] on are zeros, their cell -1.
 *   Every loop is bounded by a count known before it starts (digit passes, cells, k, n_rot); NaN or +-Inf logits give no candidate
 *   or an unspecified one, never a read or write outside the buffers.
 *   workspace: vfa_bev_decode_workspace_bytes(B, L, W, topk) bytes (the confidence maps), 4-byte aligned, the caller's.
 *   Limits and errors: a negative size, topk < 1, a NULL required pointer, a short workspace, cls_thresh < 0 or NaN:
 *   VFA_ERR_BAD_ARGUMENT; B == 0 or L * W == 0 returns 0 and writes nothing; B > 65535, topk > VFA_BEV_DECODE_MAX_TOPK or
 *   L * W >= 2^31: VFA_ERR_UNSUPPORTED. */
#define VFA_BEV_DECODE_MAX_TOPK 1024
size_t vfa_bev_decode_workspace_bytes(int B, int L, int W, int topk);
int vfa_bev_decode_f32(const float *heatmap, const float *loc_offset, const long long *loc_stride, const float *dim_offset,
                       const long long *dim_stride, const float *rotation, const long long *rot_stride, int B, int L, int W, int n_rot,
                       int topk, float cls_thresh, float grid0, float grid1, float world0, float world1, const float *dimension_mean,
                       int yx_first, void *workspace, size_t workspace_bytes, int *count, float *conf, float *location, int *cell,
                       float *dimension, float *rotation_out, void *stream);

/* ---- a 3x3 convolution at listed cells: the orientation head where it is read ------------------------------------------------
 *
 * vfa_conv3x3_at_cells_f32: the dense convolution weight (O, C, 3, 3) * feat, dilation d >= 1, zero padding d ("same"), no bias,
 * evaluated at k listed cells of each of B frames instead of at all L * W: the same function gathered at the cells, up to the
 * fp32 summation order.  Stream-ordered, no allocation, no host round trip, no atomics: the same bits on every run.
 *                                    replaces orient_pred of vfa/model/vfanet.py:53 where decode3d / the CSL loss read it
 *   feat (B, C, L, W) float32, read through four ELEMENT strides {frame, channel, row, column} >= 0 given as a HOST array: NCHW
 *   and channels-last storage are taken alike and never copied.  weight (O, C, 3, 3) contiguous, 16-byte aligned.
 *   cell (B, k) int32, the flat index l * W + w.  An entry outside [0, L * W) -- the decode writes -1 behind a frame's count -- is a
 *   SKIPPED row: its logits are zeros, its rotation is 0.0f, and no address is formed from it.
 *   Out, at least one of the two:
 *   - logits (B, k, O): logits[b, j, o] = sum over the 9 taps t = 3 ty + tx and the C channels of
 *     weight[o, c, ty, tx] * feat[b, c, l + (ty - 1) d, w + (tx - 1) d]; a tap outside the map contributes nothing.  Products and
 *     sums are fp32 (v_mfma_f32_16x16x4_f32: an fmaf chain); the two partial sums of an element are added in a fixed order, and
 *     the logits are the same bits whether or not the rotation is asked for;
 *   - rotation (B, k): (float)argmax * (float)(pi / 180) by exactly the rule of vfa_bev_decode_f32 (one device function serves
 *     both: csrc/vfa_rotation.h).  With logits == NULL the logits are staged in `workspace`, the caller's, 4-byte aligned, of
 *     vfa_conv3x3_at_cells_workspace_bytes(B, k, O) bytes; otherwise the workspace is not looked at.
 *   Limits and errors: a negative size, C < 1, O < 1, d < 1, a negative stride, a NULL required pointer, neither output, a short
 *   workspace: VFA_ERR_BAD_ARGUMENT; B * k == 0 returns 0 and writes nothing; C % 32 != 0, a weight that is not 16-byte aligned,
 *   L * W or B * k >= 2^31 - 16, O > 2^21: VFA_ERR_UNSUPPORTED.
 *
 * vfa_conv3x3_at_cells_backward_f32: from d_logits (B, k, O), either or both of
 *   - d_weight (O, C, 3, 3) = the sum over the rows that are not skipped of d_logits[b, j, o] * tap, one fmaf chain per element in
 *     ASCENDING row order b * k + j;
 *   - d_feat (B, C, L, W), contiguous and dense, EVERY element written (zeros where no tap lies).  A location receives the sum
 *     over the (row, tap) pairs of its frame that lie on it and over o of d_logits * weight.  Several pairs do lie on one
 *     location (cells exactly d apart in a row, a column or a diagonal; duplicate cells): the location is written once, by its
 *     lowest pair, which adds the pairs in ascending (row, tap) order and inside a pair o ascending (csrc/vfa_cellconv.h).
 *   No float atomics, no workspace: both are the same bits on every run.  Skipped rows contribute nothing, whatever their
 *   d_logits hold.  Errors as for the forward (a NULL d_logits or neither output: VFA_ERR_BAD_ARGUMENT); B * k == 0 writes zeros;
 *   d_feat with k > VFA_CELLCONV_MAX_ROWS: VFA_ERR_UNSUPPORTED. */
#define VFA_CELLCONV_MAX_ROWS 1024
size_t vfa_conv3x3_at_cells_workspace_bytes(int B, int k, int O);
int vfa_conv3x3_at_cells_f32(const float *feat, const long long *feat_stride, const float *weight, const int *cell, int B, int C, int L,
                             int W, int O, int k, int dilation, float *logits, float *rotation, void *workspace, size_t workspace_bytes,
                             void *stream);
int vfa_conv3x3_at_cells_backward_f32(const float *d_logits, const float *feat, const long long *feat_stride, const float *weight,
                                      const int *cell, int B, int C, int L, int W, int O, int k, int dilation, float *d_feat,
                                      float *d_weight, void *stream);

/* ---- the training targets and the detection loss in the sparse (positive-cell list) form, no host round trip -------------------
 *
 * vfa_det_targets_f32: the encode half of ObjectEncoder for B frames of up to K objects, one workgroup per frame.
 *                                                            replaces vfa/data/encoder.py:152-217 (the three per-object loops)
 *   location (B, K, loc_width) with loc_width 2 or 3 (x, y[, z]); count (B) int32, clamped to [0, K]; dimension (B, K, 3) and
 *   rotation (B, K) radians, both or neither (neither: 2D; dim_offset and angle_label are then not written); dimension_mean: 3
 *   floats on the HOST.  kind: 0 MultiviewC, 1 MultiviewX, 2 Wildtrack (row = coord_x).  The rules (cell, offsets, label,
 *   duplicates: the later object wins, ascending cell order) are csrc/vfa_loss.h, fp32, one operation per reference operation.
 *   Out, all written: cells (B, K) int32 = row * W + column, ascending, -1 behind the frame's positives; n_pos (B) int32;
 *   loc_offset (B, K, 2); dim_offset (B, K, 3) = logf(dimension / mean); angle_label (B, K) int32; zeros behind n_pos.
 *   DEVIATION: an object outside the map or with a non-finite coordinate is dropped (the reference raises or wraps).
 *
 * vfa_det_loss_f32: per frame the reference's terms {heat map focal, location, dimension, angle focal} -> terms (B, 4), their
 * weighted sum loss (B) (loss.py:66-67, loss_weight: 4 floats on the HOST in the order heat map, location, dimension, angle) and
 * counts (B, 4) int32 {heat-map positives, negatives, angle positives, negatives} for the backward.  replaces vfa/model/loss.py
 *   heatmap logits and gt_heatmap through three ELEMENT strides {frame, row, column}; loc_offset (2 channels) / dim_offset (3)
 *   through four {frame, row, column, channel}; rotation_at (B, k, R) through three {frame, row, channel}; all strides >= 0, HOST
 *   arrays, nothing copied.  dim_offset == rotation_at == NULL: 2D (two terms, the others 0).  cells / n_pos / loc_target /
 *   dim_target / angle_label: what vfa_det_targets_f32 writes, (B, k, ...); table (R): exp(-(i - R/2)^2 / (2 sigma^2)) as float32.
 *   Row r < n_pos[b] of the list is read at cells[b, r]; a cell outside [0, L * W) is skipped.  Heat-map positives are
 *   gt_heatmap == 1, counted on the dense target.  A frame without positives: 0 for the three sparse terms.
 *   Two launches; the float32 elements are summed in float64, in a fixed order that depends on (L, W, k, R) only: the same bits
 *   on every run and in any batch.
 *   workspace: vfa_det_loss_workspace_bytes(B, L, W) bytes, 8-byte aligned, the caller's.
 *
 * vfa_det_loss_backward_f32: coef (B, 4) = d objective / d terms on the device, counts as the forward left them ->
 *   d_heatmap (B, L, W), d_loc_offset (B, L, W, 2), d_dim_offset (B, L, W, 3) contiguous and dense (zeros off the positive cells),
 *   d_rotation_at (B, k, R) contiguous (zero rows behind n_pos).  Nothing accumulates: bit-reproducible.
 *
 * Limits and errors of the three, decided before anything is launched: a negative size or stride, a NULL required pointer, a
 * short workspace, loc_width outside {2, 3}, world <= 0: VFA_ERR_BAD_ARGUMENT; K or k > VFA_DET_MAX_OBJECTS, R > VFA_DET_MAX_ROT or
 * odd, B > 65535, L * W >= 2^31: VFA_ERR_UNSUPPORTED; B == 0 or L * W == 0 (the loss) returns 0 and launches nothing. */
#define VFA_DET_MAX_OBJECTS 1024
#define VFA_DET_MAX_ROT 1024
int vfa_det_targets_f32(const float *location, int loc_width, const int *count, const float *dimension, const float *rotation,
                        const float *dimension_mean, int B, int K, int L, int W, float world0, float world1, int kind, int *cells,
                        int *n_pos, float *loc_offset, float *dim_offset, int *angle_label, void *stream);
size_t vfa_det_loss_workspace_bytes(int B, int L, int W);
int vfa_det_loss_f32(const float *heatmap, const long long *heat_stride, const float *gt_heatmap, const long long *gt_stride,
                     const float *loc_offset, const long long *loc_stride, const float *dim_offset, const long long *dim_stride,
                     const float *rotation_at, const long long *rot_stride, const int *cells, const int *n_pos, const float *loc_target,
                     const float *dim_target, const int *angle_label, const float *table, const float *loss_weight, int B, int L, int W,
                     int k, int R, void *workspace, size_t workspace_bytes, float *terms, float *loss, int *counts, void *stream);
int vfa_det_loss_backward_f32(const float *coef, const float *heatmap, const long long *heat_stride, const float *gt_heatmap,
                              const long long *gt_stride, const float *loc_offset, const long long *loc_stride, const float *dim_offset,
                              const long long *dim_stride, const float *rotation_at, const long long *rot_stride, const int *cells,
                              const int *n_pos, const float *loc_target, const float *dim_target, const int *angle_label,
                              const float *table, const int *counts, int B, int L, int W, int k, int R, float *d_heatmap,
                              float *d_loc_offset, float *d_dim_offset, float *d_rotation_at, void *stream);

/* ---- the dense heat-map target of a training step rendered from the object tensors, no host round trip --------------------------
 *                                       replaces vfa/data/GK.py (RotationGaussianKernel, GaussianKernel) and the cached .npy maps
 * Both take what vfa_det_targets_f32 takes -- location (B, K, loc_width), count (B) int32 clamped to [0, K], world, kind -- and give
 * every object the cell that call gives it (csrc/vfa_loss.h; outside the map or non-finite: dropped), so the cells of heat equal
 * to 1 are the cells vfa_det_targets_f32 lists.  heat (B, L, W) contiguous, every element written.  Slots behind count are not read.
 * The rules: csrc/vfa_heat.h.
 *
 * vfa_heat_rgk_f32: per object a rotated Gaussian kernel of n = k + 1 <= VFA_HEAT_MAX_KERNEL taps per side, k = (int)(ceil(max(w, l)
 *   * alpha) * ratio), from dimension (B, K, 3) = (h, w, l) and angle_deg (B, K) FLOAT64 degrees (the annotation's number); taps in
 *   float32, rotation and blend in float64 with the reference's operation order, pasted with its arg-max on the object's cell by an
 *   integer max on the bit patterns, the centre 1: the map does not depend on the order of the objects, the same bits on every run
 *   and in any batch.  DEVIATIONS: an arg-max tie takes the first cell in row-major order (the reference raises); kernel cells
 *   outside the map are dropped (the reference raises); an object with k > 64 (or k < 2, a non-positive or non-finite dimension or
 *   angle) contributes its centre only and is counted in n_clipped (B) int32.  One workgroup per (object slot, frame).
 * vfa_heat_gk_f32: occupancy (a duplicate counts once) convolved with table ((2r+1)^2 float32 on the DEVICE, r <=
 *   VFA_HEAT_MAX_RADIUS), zero padding, float64 sum in raster order rounded once, occupied cells 1 (no clip above 1).
 *   workspace: vfa_heat_workspace_bytes(B, L, W) bytes (one occupancy byte per cell), the caller's.
 *
 * Errors, decided before anything is launched, with the codes and limits of the vfa_det_* family: a negative size, a NULL required
 * pointer, a short workspace, loc_width outside {2, 3}, world <= 0, kind outside 0..2, alpha <= 0, ratio outside 1..1024, r < 0:
 * VFA_ERR_BAD_ARGUMENT; K > VFA_DET_MAX_OBJECTS, r > VFA_HEAT_MAX_RADIUS, B > 65535, L * W >= 2^31 - 1024: VFA_ERR_UNSUPPORTED;
 * B == 0 or L * W == 0 returns 0 and launches nothing. */
#define VFA_HEAT_MAX_KERNEL 65
#define VFA_HEAT_MAX_RADIUS 16
size_t vfa_heat_workspace_bytes(int B, int L, int W);
int vfa_heat_rgk_f32(const float *location, int loc_width, const int *count, const float *dimension, const double *angle_deg, int B,
                     int K, int L, int W, float world0, float world1, int kind, double alpha, int ratio, float *heat, int *n_clipped,
                     void *stream);
int vfa_heat_gk_f32(const float *location, int loc_width, const int *count, const float *table, int r, int B, int K, int L, int W,
                    float world0, float world1, int kind, void *workspace, size_t workspace_bytes, float *heat, void *stream);

/* ---- the front of a frame: the cameras' 8-bit frames -> the normalised float32 tensor of the trunk, no host resize ---------------
 *                         replaces transforms.Resize + ToTensor (vfa/data/dataset.py:63, train.py:209-214) and vfanet.py:59
 * src: N images of Hin x Win pixels, three interleaved bytes per pixel (the layout of a decoded camera frame); pixel (y, x) of
 * image i starts at src + i * image_stride_bytes + y * row_stride_bytes + 3 * x (row_stride_bytes >= 3 * Win, any alignment).
 * dst (N, 3, Hout, Wout) float32 contiguous, every element written.  The arithmetic is Pillow's antialiased bilinear resize of 8-bit
 * images -- per axis integer coefficients of 22 fractional bits made in double, the horizontal pass rounded to bytes before the
 * vertical one -- then (float)byte / 255.0f and (t - mean[c]) / std[c] with IEEE float32 divisions: BIT FOR BIT what the reference's
 * chain computes on the host.  An axis that keeps its length is copied (its coefficients are the identity); mean 0, std 1 gives
 * plain ToTensor.  The rules: csrc/vfa_resize.h.
 *
 * vfa_image_plan writes both axes' taps and the 3 x 256 table of the three channels (mean, std: 3 floats each on the DEVICE) into
 *   workspace (vfa_image_workspace_bytes(Hin, Win, Hout, Wout) bytes, the caller's, 16-byte aligned): one small launch, once per
 *   (sizes, mean, std).  vfa_image_frames_u8_f32 reads it: one launch, one workgroup per tile of one image, the horizontal pass into
 *   LDS bytes, the vertical pass out of LDS; no intermediate image in memory.  Both are stream-ordered and capturable.
 *
 * Errors, decided before anything is launched: a non-positive length, N < 0, a NULL pointer, a short workspace, row_stride_bytes <
 * 3 * Win, image_stride_bytes < 0: VFA_ERR_BAD_ARGUMENT; a length above VFA_IMAGE_MAX_LENGTH, an axis that shrinks by more than 8
 * (more than VFA_IMAGE_MAX_TAPS taps), N > 65535: VFA_ERR_UNSUPPORTED (the workspace size of such lengths is 0); N == 0 returns 0. */
#define VFA_IMAGE_MAX_TAPS 17
#define VFA_IMAGE_MAX_LENGTH 16384
size_t vfa_image_workspace_bytes(int Hin, int Win, int Hout, int Wout);
int vfa_image_plan(int Hin, int Win, int Hout, int Wout, const float *mean, const float *std, void *workspace, size_t workspace_bytes,
                   void *stream);
int vfa_image_frames_u8_f32(const unsigned char *src, long long image_stride_bytes, long long row_stride_bytes, int N, int Hin, int Win,
                            const void *workspace, size_t workspace_bytes, float *dst, int Hout, int Wout, void *stream);

/* ---- the dense 3x3 convolutions of the BEV heads at inference (csrc/vfa_conv.hip, vfa_dense.h; the rules: csrc/vfa_conv.h) -------------
 *                         replaces the nn.Conv2d / BatchNorm2d / GroupNorm calls of vfanet.py:131-149 in eval mode
 * All of them: stride 1, zero padding = dilation, 1 <= dilation <= 4, float32; x (B, C, L, W) is read through its four ELEMENT
 * strides x_stride[4] (>= 0: NCHW, channels-last or a slice; never copied), out is contiguous (B, O, L, W) and every element is
 * written.  Fixed summation order and no float atomics: the same bits on every run, and a frame gives the same bits alone and in a
 * batch.  Stream-ordered, no host wait, capturable; workspaces are the caller's, the library keeps no state.
 *
 * vfa_conv3x3_pack_weights_f32: weight (O, C, 3, 3) contiguous -> `packed` (vfa_conv3x3_packed_bytes(O, C) bytes, 16-byte aligned):
 *   the weight's absmax and its two fp16 planes scaled by a power of two (csrc/vfa_split.h).  Once per weight; C % 32 == 0.
 * vfa_conv3x3_f32: out[b, o] = act(conv(x, weight)[b, o] * scale[o] + shift[o]); scale / shift: device vectors of O floats or NULL
 *   (1 / 0), relu: 0 identity, otherwise max(., 0) (a NaN stays a NaN).  The product is the three-MFMA fp16 split of
 *   csrc/vfa_split.h; the input's scale is a power of two from the absmax of the finite values of EACH frame (a pre-pass into
 *   workspace, vfa_conv3x3_workspace_bytes(B) bytes, 4-byte aligned).  Any O >= 1.
 * vfa_bn_fold_f32: scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) * scale (O floats each, computed in float64 on the
 *   device): eval-mode BatchNorm and the convolution's bias as the epilogue above.  gamma, beta, bias may be NULL (1, 0, 0).
 * vfa_conv3x3_few_f32: 1 <= O <= 4, weight (O, C, 3, 3) contiguous float32, no bias, plain fmaf: per cell four chains over a
 *   quarter of the channels each (channel-ascending, tap-ascending), merged as (p0 + p1) + (p2 + p3).  a, b: both NULL, or (B, C)
 *   floats: every tap inside the map is read as relu(a[b, c] * x + b[b, c]) -- a GroupNorm affine and the ReLU -- and a tap
 *   outside the map is a zero AFTER that.  C % 4 == 0.
 * vfa_group_norm_affine_f32: per (frame, group) the mean and the biased variance of x in float64 (fixed order) ->
 *   a[b, c] = gamma[c] * rstd, b[b, c] = beta[c] - mean * a[b, c] ((B, C) floats; gamma / beta may be NULL), the prologue of
 *   vfa_conv3x3_few_f32.  workspace: vfa_group_norm_workspace_bytes(B, groups) bytes, 8-byte aligned.
 *
 * Errors, decided before anything is launched: a negative size, O < 1, dilation < 1, groups that do not divide C, a NULL required
 * pointer, a negative stride, a short or misaligned workspace, a `packed` of another size: VFA_ERR_BAD_ARGUMENT; C % 32 != 0 (few:
 * C % 4), dilation > 4, O > 4 (few), B or L > 65535, L * W >= 2^30: VFA_ERR_UNSUPPORTED (vfa_conv3x3_packed_bytes is 0 for such a
 * C).  B == 0 or L * W == 0 returns 0 and writes nothing. */
size_t vfa_conv3x3_packed_bytes(int O, int C);
int vfa_conv3x3_pack_weights_f32(const float *weight, int O, int C, void *packed, size_t packed_bytes, void *stream);
size_t vfa_conv3x3_workspace_bytes(int B);
int vfa_conv3x3_f32(const float *x, const long long *x_stride, const void *packed, size_t packed_bytes, const float *scale,
                    const float *shift, int relu, int B, int C, int L, int W, int O, int dilation, float *out, void *workspace,
                    size_t workspace_bytes, void *stream);
int vfa_bn_fold_f32(const float *gamma, const float *beta, const float *mean, const float *var, const float *bias, float eps, int O,
                    float *scale, float *shift, void *stream);
int vfa_conv3x3_few_f32(const float *x, const long long *x_stride, const float *weight, const float *a, const float *b, int B, int C, int L,
                        int W, int O, int dilation, float *out, void *stream);
size_t vfa_group_norm_workspace_bytes(int B, int groups);
int vfa_group_norm_affine_f32(const float *x, const long long *x_stride, const float *gamma, const float *beta, float eps, int B, int C,
                              int L, int W, int groups, float *a, float *b, void *workspace, size_t workspace_bytes, void *stream);

/* ---- training the dense 3x3 convolution above: its two gradients (csrc/vfa_conv_grad.hip; the integer rules: csrc/vfa_conv_grad.h) --
 *                         replaces the backward of the nn.Conv2d(256, 256, 3) layers of vfanet.py:131-149
 * y = conv(x, weight) + bias with x (B, C, L, W), weight (O, C, 3, 3), g = dL/dy (B, O, L, W); stride 1, zero padding = dilation,
 * 1 <= dilation <= 4, float32, C % 32 == 0 and O % 32 == 0.  Fixed summation order and no float atomics: the same bits on every
 * run.  Stream-ordered, no host wait, capturable; workspaces are the caller's, the library keeps no state.
 *
 * vfa_conv3x3_pack_weights_transposed_f32: weight (O, C, 3, 3) contiguous -> the `packed` planes (vfa_conv3x3_packed_bytes(C, O)
 *   bytes, 16-byte aligned) of w'[c, o, t] = weight[o, c, 8 - t], a convolution with O inputs and C outputs, without a transposed
 *   copy of the weight: dL/dx = vfa_conv3x3_f32(g, packed', B, C' = O, L, W, O' = C, the same dilation), and a frame's dL/dx is the
 *   same bits alone and in a batch.
 * vfa_conv3x3_wgrad_f32: dw[o, c, ty, tx] = sum_b sum_(l, w) g[b, o, l, w] * x[b, c, l + (ty - 1) d, w + (tx - 1) d] ((O, C, 3, 3)
 *   contiguous, every element written) and, where db is not NULL, db[o] = sum_b sum_(l, w) g[b, o, l, w] (O floats).  g and x are
 *   read through their four ELEMENT strides (>= 0, never copied).  The product is the three-MFMA fp16 split of csrc/vfa_split.h with
 *   both operands split as they are staged; each has a power-of-two scale from the absmax of the finite values of EACH frame.  The
 *   cells are cut into slabs by a rule of (L, W) alone (csrc/vfa_conv_grad.h); one workgroup writes the float32 partial of one
 *   (frame, slab, tile of 128 outputs x 32 inputs), unscaled by its frame's 2^-(eg + ex); the partials of an element are added in
 *   ascending (frame, slab) order in float64 and rounded once.  db: per output, float64 sums in a fixed order, rounded once.
 *   workspace: vfa_conv3x3_wgrad_workspace_bytes(B, O, C, L, W) bytes, 16-byte aligned.
 *
 * Errors, decided before anything is launched: a negative size, O < 1, C < 1, dilation < 1, a NULL required pointer, a negative
 * stride, a short or misaligned workspace, a `packed` of another size: VFA_ERR_BAD_ARGUMENT; C % 32 != 0, O % 32 != 0, dilation >
 * 4, B or L > 65535, L * W >= 2^30, O * C * 9 >= 2^30: VFA_ERR_UNSUPPORTED (vfa_conv3x3_wgrad_workspace_bytes is 0 for such sizes
 * and for an empty problem).  B == 0 or L * W == 0: dw and db are zeros (the empty sum). */
int vfa_conv3x3_pack_weights_transposed_f32(const float *weight, int O, int C, void *packed, size_t packed_bytes, void *stream);
size_t vfa_conv3x3_wgrad_workspace_bytes(int B, int O, int C, int L, int W);
int vfa_conv3x3_wgrad_f32(const float *g, const long long *g_stride, const float *x, const long long *x_stride, int B, int C, int L, int W,
                          int O, int dilation, float *dw, float *db, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the residual stages of the ResNet trunk at inference (csrc/vfa_trunk.hip, vfa_dense.h; the rules: csrc/vfa_conv.h) ----------------
 *                         replaces the nn.Conv2d / GroupNorm / ReLU calls of a block, resnet.py:26-57, in eval mode
 * The dense kernel above with a stride, one or nine taps and a prologue; float32; x (B, C, L, W) is read through its four ELEMENT
 * strides x_stride[4] (>= 0, never copied).  Fixed summation order and no float atomics: the same bits on every run, and an image
 * gives the same bits alone and in a batch.  Stream-ordered, no host wait, capturable; workspaces are the caller's, the library
 * keeps no state.
 *
 * vfa_trunk_pack_weights_f32: weight (O, C, 3, 3) with taps 9 or (O, C, 1, 1) with taps 1, contiguous -> `packed`
 *   (vfa_trunk_packed_bytes(O, C, taps) bytes, 16-byte aligned): the weight's absmax and its two fp16 planes scaled by a power of
 *   two, in the slices of csrc/vfa_conv.h with `taps` slices per (output tile, chunk).  Once per weight; C % 32 == 0.
 * vfa_trunk_conv_f32: out (B, O, Lo, Wo) contiguous, Lo = (L - 1) / stride + 1, Wo = (W - 1) / stride + 1, every element written:
 *   the raw convolution, without bias.  taps 9: 3 x 3, zero padding 1; taps 1: 1 x 1, no padding; stride 1 or 2.  a, b: both NULL,
 *   or (B, C) floats: every tap inside the map reads max(fmaf(a[b, c], x, b[b, c]), 0) -- a GroupNorm affine and the ReLU, the
 *   normalised map is never written -- and a tap outside the map is a zero AFTER that.  The product is the three-MFMA fp16 split of
 *   csrc/vfa_split.h; the input's scale is a power of two from the absmax of the finite values the products see (after the
 *   prologue; with one tap at the strided positions) of EACH image, a pre-pass into workspace (vfa_trunk_workspace_bytes(B) bytes,
 *   4-byte aligned).  With C > 256 the two halves of the channels are summed in separate fp32 chains and added once.  Any O >= 1.
 * vfa_residual_join_f32: out = max(fmaf(a[b, c], y, b[b, c]) + shortcut, 0) with shortcut = r, or fmaf(ra[b, c], r, rb[b, c]) where
 *   ra, rb are given (both or neither); y, r, out contiguous (B, C, L, W), a, b, ra, rb (B, C) floats; out may be y.  One rounding
 *   per written operation; a NaN stays a NaN.
 *
 * Errors, decided before anything is launched: a negative size, O < 1, taps other than 1 or 9, a stride other than 1 or 2, one of
 * a / b (ra / rb) without the other, a NULL required pointer, a negative element stride, a short or misaligned workspace, a `packed`
 * of another size: VFA_ERR_BAD_ARGUMENT; C % 32 != 0, B or L > 65535, L * W >= 2^30: VFA_ERR_UNSUPPORTED (vfa_trunk_packed_bytes
 * is 0 for such a C or such taps).  An empty problem (B == 0 or L * W == 0; the join: C == 0 too) returns 0 and writes nothing. */
size_t vfa_trunk_packed_bytes(int O, int C, int taps);
int vfa_trunk_pack_weights_f32(const float *weight, int O, int C, int taps, void *packed, size_t packed_bytes, void *stream);
size_t vfa_trunk_workspace_bytes(int B);
int vfa_trunk_conv_f32(const float *x, const long long *x_stride, const void *packed, size_t packed_bytes, const float *a, const float *b, int B,
                       int C, int L, int W, int O, int taps, int stride, float *out, void *workspace, size_t workspace_bytes, void *stream);
int vfa_residual_join_f32(const float *y, const float *a, const float *b, const float *r, const float *ra, const float *rb, int B, int C, int L,
                          int W, float *out, void *stream);

/* ---- training the identity residual blocks of the trunk (csrc/vfa_trunk_grad.hip, vfa_conv_grad.hip, vfa_conv.hip) ---------------------
 *                         replaces the backward of a BasicBlock of resnet.py:26-57 with stride 1 and no projection
 * A block keeps three maps (the two raw convolutions y1, y2 and the join) besides its input; the normalised maps are recomputed in
 * prologues.  float32, fixed summation order, no float atomics: the same bits on every run, and an image gives the same dx bits
 * alone and in a batch.  Stream-ordered, no host wait, capturable; workspaces are the caller's, the library keeps no state.
 * The input gradient of a stride-1 layer needs no entry point of its own: vfa_conv3x3_pack_weights_transposed_f32 writes the planes
 * vfa_trunk_conv_f32 reads (taps 9, stride 1, no prologue, C' = O, O' = C), two accumulator chains past 256 channels included.
 *
 * vfa_group_norm_stats_f32: vfa_group_norm_affine_f32 -- the same kernels, a and b bit for bit -- that also writes stats
 *   (B, groups, 2) doubles (8-byte aligned): the mean and rstd = 1 / sqrt(var + eps) of each (image, group), the float64 values a and
 *   b were made from.
 * vfa_group_norm_backward_f32: the backward of z = GroupNorm(y) behind a ReLU with mask m, u being the gradient behind that ReLU;
 *   y, u, out, dy, dz contiguous (B, C, L, W), no two of them the same memory.  mask VFA_GN_MASK_PROLOGUE: m = fmaf(a[b, c], y,
 *   b[b, c]) > 0 with the forward's (B, C) affine -- the ReLU the next convolution applied as it read y; out, dz unused.
 *   VFA_GN_MASK_OUT: m = out > 0 for the given map -- the ReLU of the join -- and dz = m ? u : 0, the gradient of the shortcut, is
 *   written too; a, b unused.  Three launches: per (image, channel) S1 = sum m u and S2 = sum m u y in float64 (32 parts of the
 *   plane, a fixed tree in each, the parts in ascending order); per (image, channel) the float64 coefficients p = gamma rstd, q, r of
 *   dy = p (m u) + q y + r, each rounded to float32 once, and dgamma[c], dbeta[c] (C floats, either may be NULL) as float64 sums over
 *   the images in ascending order, rounded once; elementwise dy = fmaf(p, m ? u : 0, fmaf(q, y, r)) (a NaN stays a NaN).  gamma:
 *   C floats or NULL (1); stats: those of vfa_group_norm_stats_f32.  workspace: vfa_group_norm_backward_workspace_bytes(B, C) bytes,
 *   8-byte aligned.
 * vfa_trunk_conv_wgrad_f32: vfa_conv3x3_wgrad_f32 at dilation 1 without db, whose x operand is max(fmaf(a[b, c], x, b[b, c]), 0)
 *   where a, b ((B, C) floats, both or neither) are given -- applied as a value of the window arrives, a position outside the map
 *   being a zero AFTER that, and seen by the absmax pre-pass -- and x itself where they are NULL.  The cells are cut into
 *   slabs_for(L, W, O, C) slabs (csrc/vfa_conv_grad.h): the slabs of vfa_conv3x3_wgrad_f32 up to O * C = 256^2 (there, without a and
 *   b, its bits), fewer in proportion past it, so that a frame's partials never exceed those of a 256 x 256 layer on the same map;
 *   partial layout and merge are unchanged.  workspace: vfa_trunk_conv_wgrad_workspace_bytes(B, O, C, L, W) bytes, 16-byte aligned.
 *
 * Errors, decided before anything is launched: as for the entry points above; a mask other than the two, one of a / b without the
 * other, groups that do not divide C: VFA_ERR_BAD_ARGUMENT; the backward with B, C or L > 65535, L * W >= 2^30 or B * C >= 2^29:
 * VFA_ERR_UNSUPPORTED.  B == 0 or L * W == 0: dgamma, dbeta (and dw) are zeros, nothing else is written. */
#define VFA_GN_MASK_PROLOGUE 0
#define VFA_GN_MASK_OUT 1
int vfa_group_norm_stats_f32(const float *x, const long long *x_stride, const float *gamma, const float *beta, float eps, int B, int C,
                             int L, int W, int groups, float *a, float *b, double *stats, void *workspace, size_t workspace_bytes, void *stream);
size_t vfa_group_norm_backward_workspace_bytes(int B, int C);
int vfa_group_norm_backward_f32(const float *y, const float *u, const float *a, const float *b, const float *out, const float *gamma,
                                const double *stats, int mask, int B, int C, int L, int W, int groups, float *dy, float *dz, float *dgamma,
                                float *dbeta, void *workspace, size_t workspace_bytes, void *stream);
size_t vfa_trunk_conv_wgrad_workspace_bytes(int B, int O, int C, int L, int W);
int vfa_trunk_conv_wgrad_f32(const float *g, const long long *g_stride, const float *x, const long long *x_stride, const float *a, const float *b,
                             int B, int C, int L, int W, int O, float *dw, void *workspace, size_t workspace_bytes, void *stream);

/* ---- training the projection blocks of the trunk: the gradients of a stride-2 convolution (csrc/vfa_conv_grad.hip, vfa_trunk.hip) -------
 *                         replaces the backward of a BasicBlock of resnet.py:26-57 with stride 2 and a 1 x 1 projection
 * y = conv(x, w, stride 2) with w (O, C, 3, 3) and padding 1 (kernel 3) or w (O, C, 1, 1) without padding (kernel 1); x (B, C, L, W), y and
 * its gradient g (B, O, Lo, Wo), Lo = (L - 1) / 2 + 1, Wo = (W - 1) / 2 + 1.  O and C multiples of 32.  float32, fixed summation order,
 * no float atomics: the same bits on every run.  Stream-ordered, no host wait, capturable.  The integer rules: csrc/vfa_conv_grad.h.
 *
 * vfa_trunk_down_wgrad_f32: dw[o, c, ty, tx] = sum_b sum_(i, j) g[b, o, i, j] x[b, c, 2 i + ty - 1, 2 j + tx - 1] (kernel 1: x[b, c, 2 i, 2 j]),
 *   positions outside x being zeros; dw (O, C, kernel, kernel) contiguous; (L, W) is the size of x; g and x are read through their
 *   four element strides.  The kernel of vfa_conv3x3_wgrad_f32 (cells as K, the three-product fp16 split of both operands under
 *   per-image power-of-two scales) with K tiles of 2 x 32 cells and the 5 x 65 window of x stored by column parity; float32 partials
 *   per (image, slab) in [image][slab][tap][o][c] with slabs_for(Lo, Wo, O, C) slabs, merged in float64 in ascending order.
 *   workspace: vfa_trunk_down_wgrad_workspace_bytes(B, O, C, L, W, kernel) = pad256(8 B) + 4 B slabs_for(Lo, Wo, O, C) kernel^2 O C
 *   bytes, 16-byte aligned.
 * vfa_trunk_down_dgrad_f32: dx[b, c, y, x] = sum_o sum g[b, o, i, j] w[o, c, ty, tx] over the (i, j, ty, tx) with 2 i + ty - 1 = y and
 *   2 j + tx - 1 = x; dx (B, C, L, W) contiguous; g is read through its strides, weight (O, C, kernel, kernel) contiguous as it lies.
 *   kernel 3: dx falls into four parity classes (y & 1, x & 1) with 1, 2, 2 and 4 taps, one launch of the dense kernel of
 *   vfa_trunk_conv_f32 each over that class's taps alone (a class without positions is not launched), stored through doubled
 *   strides: no zero-stuffed copy of g exists, and EVERY element of dx is written exactly once.  Two accumulator chains where
 *   O > 256; one scale per image from the absmax of the whole of g; an image gives the same bits alone and in a batch.
 *   accumulate 1: the stored value is dx + the sum instead, in that order -- the second term of a sum of two input gradients.
 *   kernel 1 touches only the class (0, 0) and exists with accumulate 1 alone (accumulate 0: VFA_ERR_UNSUPPORTED).  A projection
 *   block's dx is the 3 x 3 term FIRST (accumulate 0), then the projection's term added to it (kernel 1, accumulate 1): one rounding
 *   of each term and one of the sum, the order fixed.
 *   workspace: vfa_trunk_down_dgrad_workspace_bytes(B, O, C, kernel) = pad256(4 B) + 64 + 4 kernel^2 ceil(C / 128) 128 O bytes,
 *   16-byte aligned: the scales and the packed planes, made by every call and kept nowhere.
 *
 * Measured on one MI355X (tools/bench_trunk_proj_train.py, resnet18, 720 x 1280, 7 | 28 images; DESIGN 4.6 has the table): against the
 * library's gradients of the same convolutions the 3 x 3 weight gradient takes 1.5 - 2.4 x and the 1 x 1 weight gradient 1.7 - 3.3 x
 * their time (the weak point: a workgroup stages 128 outputs of g for 32 inputs and one or nine taps), the 3 x 3 input gradient
 * 0.63 - 1.37 x, the projection's added term 0.68 - 1.56 x.  wgrad_down_kernel<9>: 256 VGPRs + 144 AGPRs, 86 816 bytes of LDS;
 * wgrad_down_kernel<1>: 176 + 16, 45 056; the class kernels: 82 - 200 VGPRs + 64 AGPRs, 53 248 - 59 168 bytes; scratch 0 in all.
 *
 * Errors, decided before anything is launched: a NULL pointer, a negative stride or size, a kernel other than 3 and 1, (Lo, Wo) that
 * is not the stride-2 size of (L, W), a short or misaligned workspace: VFA_ERR_BAD_ARGUMENT; O or C not a multiple of 32, B or
 * L > 65535, L * W >= 2^30: VFA_ERR_UNSUPPORTED.  B == 0 or L * W == 0: dw is zeros, dx is not written. */
size_t vfa_trunk_down_wgrad_workspace_bytes(int B, int O, int C, int L, int W, int kernel);
int vfa_trunk_down_wgrad_f32(const float *g, const long long *g_stride, const float *x, const long long *x_stride, int B, int C, int L, int W, int O,
                             int kernel, float *dw, void *workspace, size_t workspace_bytes, void *stream);
size_t vfa_trunk_down_dgrad_workspace_bytes(int B, int O, int C, int kernel);
int vfa_trunk_down_dgrad_f32(const float *g, const long long *g_stride, const float *weight, int B, int O, int Lo, int Wo, int C, int L, int W,
                             int kernel, int accumulate, float *dx, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the stem of the ResNet trunk at inference (csrc/vfa_stem.hip; the integer rules: csrc/vfa_stem.h) ------------------------------
 *                         replaces conv1 and the max pooling of resnet.py:100-102, 139-140 in eval mode
 * float32; fixed summation order and no atomics: the same bits on every run, and an image gives the same bits alone and in a
 * batch.  Stream-ordered, no host wait, capturable; the workspace is the caller's, the library keeps no state.
 *
 * vfa_stem_conv_f32: out (B, O, Lo, Wo) contiguous, Lo = (L - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, every element written: the raw
 *   convolution F.conv2d(x, weight, stride=2, padding=3) of x (B, 3, L, W), read through its four ELEMENT strides x_stride[4] (>= 0,
 *   never copied), with weight (O, 3, 7, 7) contiguous, 1 <= O <= 64, without bias.  The exact f32 MFMA: per output ONE fmaf chain
 *   over k = (c 7 + ky) 7 + kx ascending, a tap outside the image being a zero operand.  workspace: vfa_stem_workspace_bytes(O) bytes,
 *   16-byte aligned (the weight as the kernel reads it, written by every call).
 * vfa_stem_pool_f32: out (B, C, (L - 1) / 2 + 1, (W - 1) / 2 + 1) = max_pool2d(max(fmaf(a[b, c], y, b[b, c]), 0), 3, stride 2,
 *   padding 1) of y (B, C, L, W) contiguous; a, b (B, C) floats (vfa_group_norm_affine_f32 on the raw map: GroupNorm and the ReLU).
 *   A tap outside the map is skipped; a NaN tap makes its cells NaNs.  Any C >= 1.
 *
 * Errors, decided before anything is launched: a negative size, O < 1, C < 1 (the convolution), a NULL required pointer, a negative
 * element stride, a short or misaligned workspace: VFA_ERR_BAD_ARGUMENT; C != 3 or O > 64 (the convolution;
 * vfa_stem_workspace_bytes is 0 for such an O), B or L > 65535, L * W >= 2^30: VFA_ERR_UNSUPPORTED.  An empty problem (B == 0 or
 * L * W == 0; the pooling: C == 0 too) returns 0 and writes nothing. */
size_t vfa_stem_workspace_bytes(int O);
int vfa_stem_conv_f32(const float *x, const long long *x_stride, const float *weight, int B, int C, int L, int W, int O, float *out,
                      void *workspace, size_t workspace_bytes, void *stream);
int vfa_stem_pool_f32(const float *y, const float *a, const float *b, int B, int C, int L, int W, float *out, void *stream);

/* ---- the stem with gradients (csrc/vfa_stem.hip; the integer rules: csrc/vfa_stem.h) -----------------------------------------------
 * The two backward kernels the stem needs besides vfa_group_norm_backward_f32 (VFA_GN_MASK_PROLOGUE on the raw map).  float32; no
 * atomics, fixed summation orders: the same bits on every run and on devices of any size.  Stream-ordered, no host wait, capturable.
 *
 * vfa_stem_pool_backward_f32: the backward of vfa_stem_pool_f32 up to, but not through, the ReLU.  gout (B, C, Lo, Wo) is the
 *   gradient of the pooled map, y (B, C, L, W) the raw map, a, b (B, C) the forward's affine, all contiguous; u (B, C, L, W), every
 *   element written exactly once: u[b, c, p, q] = the sum of gout[b, c, i, j] over the windows (i, j) whose winning tap is (p, q),
 *   added in ascending (i, j) order from +0 (a position that wins nowhere: +0).  A window's taps max(fmaf(a, y, b), 0) are recomputed
 *   with the forward's bits (no winner is saved by the forward) and scanned as the forward scans them, rows then columns ascending,
 *   taps outside the map skipped, under the forward's rule (t > best || t != t): the first of equal maxima wins, and a NaN takes the
 *   window, the last one in scan order -- torch's rule.  The ReLU's mask is NOT applied: a window whose maximum is 0 credits its first
 *   tap, and vfa_group_norm_backward_f32 removes it.  A gather per element of u: an image gives the same bits alone and in a batch.
 *   Any C >= 1.
 * vfa_stem_conv_wgrad_f32: dw (O, 3, 7, 7) contiguous, dw[o, c, ky, kx] = sum over b, then (i, j), of
 *   g[b, o, i, j] x[b, c, 2 i + ky - 3, 2 j + kx - 3], positions outside the image being zeros; g (B, O, Lo, Wo) contiguous, x
 *   (B, 3, L, W) read through its four element strides x_stride[4] (>= 0, never copied), 1 <= O <= 64.  No bias, no input gradient.
 *   The exact f32 MFMA with the output cells as K: the cells are cut into vfa_stem::wgrad_slabs(Lo, Wo) <= 64 slabs of consecutive
 *   4 x 32 tiles, a rule of (Lo, Wo) alone; an (image, slab) is one workgroup whose four waves each sum one row of every tile in
 *   ascending cell order, merged as ((w0 + w1) + w2) + w3 into one float32 partial; the partials of an element are added in float64,
 *   images then slabs ascending, and rounded once.  Integer-valued operands whose partial sums stay below 2^24 give float64's result
 *   exactly.  workspace: vfa_stem_conv_wgrad_workspace_bytes(B, O, L, W) = B * slabs * O * 147 * 4 bytes, 16-byte aligned (0 for an
 *   empty or unsupported problem).
 *
 * Errors, decided before anything is launched: a negative size, O < 1, a NULL required pointer (dw always), a negative element
 * stride, a short or misaligned workspace: VFA_ERR_BAD_ARGUMENT; O > 64, B or L > 65535, L * W >= 2^30, an image whose offsets pass
 * 2^31 (the pooling: B * C >= 2^31): VFA_ERR_UNSUPPORTED.  An empty problem (B == 0 or L * W == 0; the pooling: C == 0 too) returns 0:
 * dw is zeros, u is not written. */
int vfa_stem_pool_backward_f32(const float *gout, const float *y, const float *a, const float *b, int B, int C, int L, int W, float *u,
                               void *stream);
size_t vfa_stem_conv_wgrad_workspace_bytes(int B, int O, int L, int W);
int vfa_stem_conv_wgrad_f32(const float *g, const float *x, const long long *x_stride, int B, int L, int W, int O, float *dw, void *workspace,
                            size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VFA_HIP_H */
