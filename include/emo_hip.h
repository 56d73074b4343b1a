/*
 * emo_hip.h -- C ABI of libemoportraits_hip.so: hand-written gfx950 (MI355X / CDNA4) HIP kernels for the
 * EMOPortraits volumetric-avatar *inference hot path* (SURVEY.md section 8).
 *
 * The reference (neeek2303/EMOPortraits) is pure Python/PyTorch and has NO plugin / FFI interface for this
 * path; every entry point below therefore replaces a stock torch op *call site* of the reference, cited as
 * file:line relative to the reference root.  INTEGRATION.md shows the ctypes stub a reference maintainer
 * would add at each call site.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types.  All tensor pointers are DEVICE pointers to contiguous fp32
 *     (unless stated), at least 16-byte aligned.  The caller owns every buffer.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call is asynchronous on it.
 *   - return value: 0 on success; EMO_ERR_* (negative) for argument errors; a positive hipError_t if a
 *     launch failed.  No global mutable state: calls are thread-safe.
 *   - fp32 throughout; index arithmetic of the sampler is bit-identical to ATen's CPU grid_sampler_3d.
 */
#ifndef EMO_HIP_H_
#define EMO_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMO_ABI_VERSION 29

#define EMO_OK 0
#define EMO_ERR_BAD_ARG (-1)       /* null pointer / non-positive size / unknown enum          */
#define EMO_ERR_UNSUPPORTED (-2)   /* valid request outside what the kernels implement         */
#define EMO_ERR_ALIGN (-3)         /* pointer not 16-byte aligned                              */

/* padding_mode of torch.nn.functional.grid_sample (args.grid_sample_padding_mode,
 * models/stage_1/volumetric_avatar/va_arguments.py:185; default 'zeros') */
#define EMO_PAD_ZEROS 0
#define EMO_PAD_BORDER 1
#define EMO_PAD_REFLECTION 2

/* memory layout of a 5-D volume */
#define EMO_LAYOUT_NCDHW 0         /* the reference's layout                                    */
#define EMO_LAYOUT_NDHWC 1         /* channels-last, internal fast path (gathers read C contiguous floats) */
/* 2: retired (channel-group-per-XCD layout of round 2: equal time) */
#define EMO_LAYOUT_P4 3            /* packed-4: [N][C/4][D][H][W][4] -- a voxel's channel quad is one 16-byte slot, x-rows are
                                      contiguous: the layout of the LDS-staged sampler (one LDS-DMA lane per box voxel, ds_read_b128
                                      gathers).  Needs C % 4 == 0.  */

/* activation applied in a kernel epilogue */
#define EMO_ACT_NONE 0
#define EMO_ACT_RELU 1
#define EMO_ACT_TANH 2
#define EMO_ACT_SIGMOID 3

int emo_abi_version(void);
/* human-readable build string: arch, compiler, kernel variants */
const char* emo_build_info(void);
/* ABI 9.  Compute units of the current device as the launchers count them (rounded down to a multiple of 8, at least 8): the
 * persistent grids of the split convolutions and the thresholds of their launch forms are sized by it, and so is the Python
 * planner (emoportraits_amd/pack.py) -- no reference counterpart (the reference leaves launch geometry to cuDNN). */
int emo_device_cu_count(void);
/* ABI 9.  Diagnostic (bench.py `roofline.sustained_peak`, not on the hot path): one launch of a bare v_mfma_f32_32x32x16_f16
 * stream -- one wave per SIMD on every CU, `iters` x 96 MFMAs per wave on pseudo-random operands; lds_reads != 0 adds the
 * fragment reads of the split kernels' K loop (8 ds_read_b128 per 12 MFMAs).  *mfma_per_launch = MFMA instructions the launch
 * issues (x 32768 flop each).  sink: >= 256 x CUs floats (never written in practice). */
int emo_mfma_stream_f16(float* sink, int iters, int lds_reads, int64_t* mfma_per_launch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a1 -- 3-D trilinear grid_sample, align_corners=False.
 * Replaces Model.grid_sample = lambda inputs, grid: F.grid_sample(inputs.float(), grid.float(),
 * padding_mode=args.grid_sample_padding_mode)  (models/stage_1/volumetric_avatar/va.py:264-265);
 * call sites notebooks/infer.py:499-500 (source) and :618-619 (driver).
 *
 *   vol   [Nv, C, D, H, W] (NCDHW) or [Nv, D, H, W, C] (NDHWC); Nv = N, or 1 with vol_batch_stride = 0
 *         (one canonical volume shared by N driver frames -- the reference loops batch-1 calls instead).
 *   grid  [N, Do, Ho, Wo, 3] (x, y, z) in [-1, 1] coordinates; or NULL when `theta` is given.
 *   theta [N, 3, 4] row-major affine (rows 0..2 of the 4x4 head-pose matrix).  When non-NULL the grid is
 *         generated in-kernel:  g_j = fma-chain( lin_x[x]*t_j0, lin_y[y]*t_j1, lin_z[z]*t_j2, t_j3 )
 *         which is what identity_grid_3d.bmm(theta[:, :3].transpose(1, 2)) computes
 *         (va.py:101-105 + notebooks/infer.py:441-444,583-588) without materialising the 0.79 MB grid.
 *   lin_x [Wo], lin_y [Ho], lin_z [Do]  the identity lattice (torch.linspace(-1, 1, n) values); required
 *         with theta or grid_kind 1, ignored otherwise.
 *   grid_kind  0: `grid` holds coordinates [N,Do,Ho,Wo,3].  1: `grid` holds planar deltas [N,3,Do,Ho,Wo] and the
 *         coordinate is lattice + delta -- the WarpGenerator output  warp = (identity_grid + deltas).permute(0,2,3,4,1)
 *         (networks/volumetric_avatar/warp_generator_resnet.py:178) consumed without materialising `warp`.
 *   variant    0 = default kernels.  NCDHW -> NCDHW: channels per block of the direct gather (1..C).  NDHWC input, bits:
 *         1 = 4 x 4 x 4 output bricks per block instead of 64-voxel rows (NDHWC output); 2 = non-temporal stores of an
 *         NCDHW output (a result that is read much later: the driver pass's rotation call); 4 = fused multiply-add accumulation
 *         of the eight corners (opt-in: coordinates, floor, corner indices and weights stay bit-identical to ATen's CPU kernel,
 *         the sampled VALUES differ from it by the skipped product roundings, <= 8 * 2^-24 * max |v w| absolute).
 *         For the LDS-staged tile kernels (in_layout EMO_LAYOUT_P4, or NCDHW -> NCDHW with bit 30 set) it is a tuning word:
 *         bits 3..0 / 7..4 / 11..8 log2 of the output tile extents x / y / z (all 0: default), 16..12 channel units per
 *         block, 24..17 LDS per block in KiB, bit 25: 512-thread blocks.  tile voxels = threads or 2 * threads.
 *   out   [N, C, Do, Ho, Wo] or [N, Do, Ho, Wo, C] according to out_layout.
 *   vol_batch_stride  elements between consecutive volumes (0 = shared volume).
 * NDHWC paths require C % 4 == 0 and support out_layout NDHWC and NCDHW.
 * in_layout EMO_LAYOUT_P4 (C % 4 == 0) supports out_layout P4 and NCDHW: the LDS-staged kernels (csrc/gs3d_tile.h) --
 * the source box of an output tile is brought into LDS by LDS-DMA once and the 8-corner gather runs out of LDS.
 */
int emo_grid_sample3d_f32(const float* vol, const float* grid, const float* theta,
                          const float* lin_x, const float* lin_y, const float* lin_z,
                          float* out,
                          int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                          int64_t vol_batch_stride, int padding_mode,
                          int in_layout, int out_layout, int variant, int grid_kind, void* stream);

/* ABI 12.  emo_grid_sample3d_f32 over a BANK of volumes (several source identities in one driver batch): frame n samples volume
 * vol_index[n] of `vol_bank`, num_vols volumes of C*D*H*W floats each, back to back in in_layout:
 *   vol_bank   [num_vols, C, D, H, W] (NCDHW) or [num_vols, D, H, W, C] (NDHWC)
 *   vol_index  [N] int32, DEVICE memory (read by the kernels: a graph replay sees its current contents)
 * Everything else means what it means in emo_grid_sample3d_f32.  Served: NDHWC -> NDHWC and NDHWC -> NCDHW (every variant bit of
 * those kernels, the 4x4x4 bricks and fma accumulation included) and the planar direct gather NCDHW -> NCDHW.  in_layout
 * EMO_LAYOUT_P4 or the tile flag (bit 30): EMO_ERR_UNSUPPORTED.  vol_index NULL or num_vols <= 0: EMO_ERR_BAD_ARG.  An index
 * outside [0, num_vols) makes that frame all zeros; the bank is not read for it. */
int emo_grid_sample3d_indexed_f32(const float* vol_bank, const int32_t* vol_index, int num_vols,
                                  const float* grid, const float* theta,
                                  const float* lin_x, const float* lin_y, const float* lin_z,
                                  float* out,
                                  int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                                  int padding_mode, int in_layout, int out_layout, int variant, int grid_kind, void* stream);

/* a2 alone -- the rotation warp as a tensor: grid[n,z,y,x,:] = theta[n,:3,:4] . (lin_x[x], lin_y[y], lin_z[z], 1), the same
 * fma chain the theta variant of emo_grid_sample3d_f32 evaluates in-kernel.  Replaces
 * `identity_grid_3d.bmm(theta[:, :3].transpose(1, 2)).view(-1, d, s, s, 3)` (notebooks/infer.py:441-444, :583-588; cached there
 * as self.source_rotation_warp).  theta [N,3,4] row-major, grid [N,Do,Ho,Wo,3]. */
int emo_affine_grid3d_f32(const float* theta, const float* lin_x, const float* lin_y, const float* lin_z,
                          float* grid, int N, int Do, int Ho, int Wo, void* stream);

/* Layout repack of a 5-D volume (used once per identity on the cached canonical volume, notebooks/infer.py:507
 * `self.target_latent_volume`).  to_channels_last: 0 NDHWC -> NCDHW, 1 NCDHW -> NDHWC, 4 NCDHW -> P4, 5 P4 -> NCDHW. */
int emo_volume_repack_f32(const float* in, float* out, int N, int C, int DHW, int to_channels_last, void* stream);

/* ABI 14.  emo_volume_repack_f32(..., to_channels_last = 1) of N volumes into rows of a channels-last BANK (enrolment of several
 * source identities at once): bank[row[n]] = the NDHWC repack of in[n], the same 64x64 LDS-tile transpose, so every written row
 * is bit-identical to emo_volume_repack_f32(in + n * C * DHW, ..., 1).
 *   in    [N, C, D, H, W] (NCDHW; DHW = D * H * W)
 *   bank  [num_rows, D, H, W, C]
 *   row   [N] int32, DEVICE memory.  A row outside [0, num_rows) writes nothing.
 * in, bank or row NULL, N, C, DHW or num_rows <= 0: EMO_ERR_BAD_ARG.  N > 65535: EMO_ERR_UNSUPPORTED. */
int emo_volume_repack_indexed_f32(const float* in, float* bank, const int32_t* row, int N, int C, int DHW, int num_rows,
                                  void* stream);

/* ABI 29.  A question, not a launch: the kernel and the launch plan a 3-D sampler call with these arguments takes.  The
 * launchers' own host functions answer -- the ones they call themselves before they launch -- so a condition of a form is
 * written once; no HIP call is made and the call works on a machine without a device.  The arguments are those of
 * emo_grid_sample3d_indexed_f32 with the same meaning, except:
 *   vol, out   read for nullness and 16-byte alignment only.
 *   banked     != 0: the question is about emo_grid_sample3d_indexed_f32 (vol_batch_stride is then ignored: C D H W);
 *              0: about emo_grid_sample3d_f32 with this vol_batch_stride (0 = one volume shared by the N samples).
 *   grid_kind  an EMO_GS3D_KIND_*: 0 and 1 as in the entries, 2 = theta is given (the entries' non-NULL theta).
 * Returns what the entry would return before any launch (EMO_ERR_BAD_ARG, EMO_ERR_UNSUPPORTED, EMO_ERR_ALIGN; then plan is all
 * zero), otherwise EMO_OK with plan[EMO_GS3D_PLAN_COUNT] filled:
 *   FORM   the kernel --
 *     EMO_GS3D_FORM_PLANAR          NCDHW -> NCDHW direct gather, one lane per output voxel          (default for that pair)
 *     EMO_GS3D_FORM_ROWS            NDHWC -> NDHWC, 64 consecutive output voxels per block           (default for that pair)
 *     EMO_GS3D_FORM_ROWS_NCDHW      NDHWC -> NCDHW, the same blocks, transposed through LDS; refused (UNSUPPORTED) where
 *                                   64 tap records + C rows of 65 floats pass 64 KiB: C > 232
 *     EMO_GS3D_FORM_BRICK           NDHWC -> NDHWC, a 4 x 4 x 4 output brick per block: variant bit 1 AND Do, Ho, Wo multiples of
 *                                   4 (else the bit is ignored: ROWS).  The brick kernel accumulates without FMA: bit 1 wins
 *                                   over bit 4.
 *     EMO_GS3D_FORM_TILE_P4, _TILE_P4_NCDHW, _TILE_PLANAR   the LDS-staged kernels: P4 -> P4, P4 -> NCDHW, and NCDHW -> NCDHW
 *                                   with variant bit 30 where W % 4 == 0 and the extents fit (else PLANAR with variant 0)
 *   ORDER  block order of ROWS / ROWS_NCDHW / BRICK: 1 = XCD-contiguous; 3 = also row-group-major over an XCD's samples, taken by
 *          the two ROWS forms for one volume shared (stride 0, no bank) by N >= 8 samples where N % 8 == 0, Do Ho Wo % 64 == 0,
 *          BPS % Do == 0 and (BPS / Do) % 8 == 0 -- each condition failing alone gives ORDER 1.  0 for the other forms.
 *   FMA    variant bit 4 taken (ROWS forms).  NT: variant bit 2 taken (ROWS_NCDHW only; ignored for an NDHWC output).  BANK: the
 *          (index, num) instantiation.
 *   GRID_X, GRID_Y, GRID_Z  the launch grid.  BPS: blocks per sample (PLANAR: per sample and channel chunk).  LAST_VOX: output
 *          voxels of a sample's last block (PLANAR: of 256; ROWS forms and BRICK: of 64; tile forms: 0).
 *   CPB    channels per block: PLANAR min(variant > 0 ? variant : 8, C) with GRID_Y = ceil(C / CPB) chunks, the last one ragged
 *          where C % CPB; the channels-last forms C; tile forms the channels of UPB units.
 *   LDS    dynamic LDS bytes of the launch (ROWS_NCDHW: 5120 + 260 C; tile forms: the tuning word's KiB, default 40 / 80).
 *   THREADS, VPT, UPB, TXS, TYS, TZS, STAGE_SLOTS  tile forms only: block size, voxels per thread, channel units per block, log2
 *          of the tile extents x / y / z, 16-byte slots of the stage. */
enum { EMO_GS3D_KIND_GRID = 0, EMO_GS3D_KIND_DELTA = 1, EMO_GS3D_KIND_THETA = 2, EMO_GS3D_KIND_COUNT = 3 };
enum { EMO_GS3D_FORM_PLANAR = 0, EMO_GS3D_FORM_ROWS = 1, EMO_GS3D_FORM_ROWS_NCDHW = 2, EMO_GS3D_FORM_BRICK = 3,
       EMO_GS3D_FORM_TILE_P4 = 4, EMO_GS3D_FORM_TILE_P4_NCDHW = 5, EMO_GS3D_FORM_TILE_PLANAR = 6, EMO_GS3D_FORM_COUNT = 7 };
enum { EMO_GS3D_PLAN_FORM = 0, EMO_GS3D_PLAN_ORDER = 1, EMO_GS3D_PLAN_FMA = 2, EMO_GS3D_PLAN_NT = 3, EMO_GS3D_PLAN_BANK = 4,
       EMO_GS3D_PLAN_GRID_X = 5, EMO_GS3D_PLAN_GRID_Y = 6, EMO_GS3D_PLAN_GRID_Z = 7, EMO_GS3D_PLAN_BPS = 8,
       EMO_GS3D_PLAN_LAST_VOX = 9, EMO_GS3D_PLAN_CPB = 10, EMO_GS3D_PLAN_LDS = 11, EMO_GS3D_PLAN_THREADS = 12,
       EMO_GS3D_PLAN_VPT = 13, EMO_GS3D_PLAN_UPB = 14, EMO_GS3D_PLAN_TXS = 15, EMO_GS3D_PLAN_TYS = 16, EMO_GS3D_PLAN_TZS = 17,
       EMO_GS3D_PLAN_STAGE_SLOTS = 18, EMO_GS3D_PLAN_COUNT = 19 };
int emo_grid_sample3d_launch_form(const void* vol, const void* out, int banked, int N, int C, int D, int H, int W, int Do, int Ho, int Wo, int64_t vol_batch_stride, int padding_mode, int in_layout, int out_layout, int variant, int grid_kind, int64_t* plan);

/* ABI 29.  The same question about emo_volume_repack_f32 (indexed = 0) and emo_volume_repack_indexed_f32 (indexed != 0, which
 * has to_channels_last = 1; its row / num_rows arguments are no part of the question).  in, out: nullness only.  Returns what
 * the entry would return before any launch, plan all zero then -- among them EMO_ERR_UNSUPPORTED where the 64 x 64 tile grid
 * has more than 65535 rows of tiles (grid y: C for to_channels_last = 1, DHW for 0) -- otherwise EMO_OK and
 * plan[EMO_REPACK_PLAN_COUNT]: DIRECTION, an EMO_REPACK_*, and the grid: (ceil(columns / 64), ceil(rows / 64), N) tiles of the
 * [rows][columns] input matrices, or (ceil(C / 4 * DHW / 256), N, 1) for the packed-4 directions. */
enum { EMO_REPACK_FROM_CHANNELS_LAST = 0, EMO_REPACK_TO_CHANNELS_LAST = 1, EMO_REPACK_TO_CHANNELS_LAST_INDEXED = 2,
       EMO_REPACK_TO_P4 = 3, EMO_REPACK_FROM_P4 = 4, EMO_REPACK_COUNT = 5 };
enum { EMO_REPACK_PLAN_DIRECTION = 0, EMO_REPACK_PLAN_GRID_X = 1, EMO_REPACK_PLAN_GRID_Y = 2, EMO_REPACK_PLAN_GRID_Z = 3,
       EMO_REPACK_PLAN_COUNT = 4 };
int emo_volume_repack_launch_form(const void* in, const void* out, int N, int C, int DHW, int to_channels_last, int indexed, int64_t* plan);

/* ---------------------------------------------------------------------------------------------
 * a10 -- GroupNorm statistics folded to a per-(sample, channel) affine.
 * Replaces the nn.GroupNorm(32, C) / AdaptiveGroupNorm in front of every conv of the reference's ResBlock
 * (networks/volumetric_avatar/utils.py:711-731 block_feats; registries :953-957; AdaptiveGroupNorm :302-325):
 * the normalised tensor is never written, the consumer conv applies x*scale+shift (+ReLU) while staging.
 *   x [N, C, S] (S = product of spatial dims), G groups, eps as nn.GroupNorm (1e-5).
 *   gamma/beta [C] or NULL (=1/0).  ada_gamma/ada_beta [N rows, ada_stride apart] or NULL: the per-sample
 *   weights assigned by assign_adaptive_norm_params (utils.py:983-995); y = (xhat*gamma+beta)*ada_gamma+ada_beta.
 *   scale/shift [N, C] out.  mean_out/rstd_out [N, G] optional (both or neither).
 *   workspace: device buffer of at least emo_groupnorm_workspace_bytes(N, G) bytes.
 */
int64_t emo_groupnorm_workspace_bytes(int N, int G);
int emo_groupnorm_affine_f32(const float* x, int N, int C, int64_t S, int G, float eps,
                             const float* gamma, const float* beta,
                             const float* ada_gamma, const float* ada_beta, int64_t ada_stride,
                             float* scale, float* shift, float* mean_out, float* rstd_out,
                             void* workspace, int64_t workspace_bytes, void* stream);
/* The same affine from the per-tile statistics emo_conv_igemm_f32 leaves in `gn_stats` (no pass over the activation):
 *   stats [N][T][C][2] = (mean, centred sum of squares) of `cnt` values each, T tiles per sample and channel
 *   (emo_conv_igemm_f32: cnt = emo_conv_tile_positions(cfg), T = D*Hl*Wl / cnt).  Combined per (sample, group) in fp64: the tile M2 values add, and the
 *   between-tile term cnt * (sum(mean_i^2) - K * mean^2) is evaluated in fp64 on the fp32 tile means (an fp64 combine of
 *   fp32 tile statistics; within a tile the conv epilogue uses centred sums, so no fp32 E[x^2] - mean^2 is ever formed).  Other arguments as emo_groupnorm_affine_f32. */
int emo_groupnorm_affine_from_tiles_f32(const float* stats, int N, int C, int64_t T, int cnt, int G, float eps,
                                        const float* gamma, const float* beta,
                                        const float* ada_gamma, const float* ada_beta, int64_t ada_stride,
                                        float* scale, float* shift, float* mean_out, float* rstd_out, void* stream);

/* ABI 8.  The second half of emo_groupnorm_affine_f32 alone: `partial` = `split` (sum, sum of squares) fp64 slices per (sample,
 * group), workspace layout [N * G][64][2], left by a producer that had the tensor in registers (emo_upsample_trilinear_gn_sums_f32);
 * S = elements per (sample, channel) of the tensor the sums are of.  Other arguments as emo_groupnorm_affine_f32. */
int emo_groupnorm_affine_from_sums_f32(const void* partial, int split, int N, int C, int64_t S, int G, float eps,
                                       const float* gamma, const float* beta,
                                       const float* ada_gamma, const float* ada_beta, int64_t ada_stride,
                                       float* scale, float* shift, float* mean_out, float* rstd_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a5/a9/a10 -- implicit-GEMM convolution on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, exact fp32).
 * Replaces F.conv2d / F.conv3d inside ResBlock / ConvBlock (networks/volumetric_avatar/utils.py:661-788;
 * Conv2d_ws/Conv3d_ws :887-915; spectral-norm hook utils/spectral_norm.py:96-168 -- both folded into the packed
 * weights at load time), stride 1, "same" zero padding, kernel 1x1(x1) or 3x3 (2-D: KD=1) or 3x3x3 (KD=3).
 *   x     [N, Cin, D, H, W]            (D = 1 for 2-D convs)
 *   wpk   weights packed by the host for block config `cfg`: [co_tile][Cin chunk][kd][pair][tap][half][BM]
 *         (emoportraits_amd/pack.py; BM / KC from emo_conv_pack_info)
 *   bias  [Cout] or NULL.
 *   scale/shift [N, Cin] or NULL: input transform x*scale+shift (GroupNorm folded, see above);
 *         relu_in != 0 applies max(.,0) after it (ReLU of block_feats, utils.py:717,731).  Zero padding is applied
 *         to the transformed tensor, as F.conv does.
 *   ups   != 0: the conv input is the nearest-neighbour x2 upsampling of x in H and W (ResBlock
 *         resize_layer_type='nearest', utils.py:684-688,764-781); out is [N, Cout, D, 2H, 2W].  2-D only.
 *   res   residual added before `act` (ResBlock skip, utils.py:783); same shape as out, or the pre-upsample
 *         shape when res_ups != 0.  May alias `out`.
 *   act   EMO_ACT_* applied last (tanh head warp_generator_resnet.py:99-107; sigmoid head decoder.py:347-358).
 *   cfg   0: 128 output channels x 128 positions per block, 1: 64 x 128, 2: 32 x 128, 3: 64 x 256, 4: 64 x 512, 5: 32 x 256 (3-5: 3x3 layers, 3 and 5
 *         also 3x3x3; weights packed as for cfg 1 resp. 2).  emo_conv_tile_positions(cfg) = positions per block.
 *   ksplit / workspace   ksplit > 1 divides the K loop (input-channel chunks x depth taps) of every output tile over
 *         ksplit blocks -- small launches (64x64 maps at batch 1, the 8^3 / 16^3 WarpGenerator layers) otherwise leave most
 *         of the 256 CUs idle; partial sums go to workspace [ksplit][N*Cout*D*Hl*Wl] floats and a second kernel adds them
 *         in fixed order and applies bias / residual / activation (deterministic; `out` may alias `res`).  ksplit = 1,
 *         workspace = NULL: single pass.  emo_conv_igemm_ksplit returns the split count the launch heuristic wants.
 *   gn_stats   NULL, or [N][D*Hl*Wl/P][Cout][2] floats, P = emo_conv_tile_positions(cfg) (ksplit == 1 only): the epilogue
 *         also reduces, per sample, P-position tile and output channel, the mean and the centred sum of squares of the FINAL output values
 *         (after bias / residual / act) -- the statistics of the GroupNorm that follows in the next block
 *         (utils.py:711-731), consumed by emo_groupnorm_affine_from_tiles_f32 instead of a pass over `out`.
 * Supported output widths: multiples of 128, or 64 / 32 / 16 / 8 (with H resp. D divisible by the tile).
 */
int emo_conv_pack_info(int KH, int KW, int cfg, int* BM, int* KC);
int emo_conv_tile_positions(int cfg);
int emo_conv_igemm_f32(const float* x, const float* wpk, const float* bias,
                       const float* scale, const float* shift, const float* res, float* out,
                       int N, int Cin, int Cout, int D, int H, int W, int KD, int KH, int KW,
                       int ups, int relu_in, int act, int res_ups, int cfg, int ksplit, float* workspace,
                       float* gn_stats, void* stream);
int emo_conv_igemm_ksplit(int N, int Cin, int Cout, int D, int H, int W, int KD, int KH, int KW, int ups, int cfg);

/* Reduced-precision mode (BASELINE.json configs[4], "fp16 MFMA convs"; opt-in per layer, never the default): the same
 * convolution with fp16 MFMA operands (v_mfma_f32_32x32x16_f16) and fp32 accumulation.  Tensors in HBM stay fp32; the
 * producer's norm + ReLU is applied in fp32 and rounded to fp16 on the way into LDS.  3x3 (2-D / 3-D) and 1x1 kernels,
 * cfg 3 (64 x 256 tile) or, 3x3 only, cfg 6 (128 x 256 tile, one block per CU); output widths that are multiples of 128, or
 * 64 / 32; Cin % 8 == 0; x 16-byte aligned; Cin <= 1024 when scale / shift are given.  wpk16: fp16 weights packed
 * [co_tile][Cin chunk of KC][kd][q = KC/16][tap][half][BM][8] (channel in chunk = 16*q + 8*half + 0..7), BM / KC from
 * emo_conv_pack_info_f16.  Other arguments, incl. gn_stats, as emo_conv_igemm_f32. */
int emo_conv_pack_info_f16(int KH, int KW, int cfg, int* BM, int* KC);
int emo_conv_igemm_f16acc32(const float* x, const void* wpk16, const float* bias,
                            const float* scale, const float* shift, const float* res, float* out,
                            int N, int Cin, int Cout, int D, int H, int W, int KD, int KH, int KW,
                            int ups, int relu_in, int act, int res_ups, int cfg, int ksplit, float* workspace,
                            float* gn_stats, void* stream);

/* ABI 9.  The reduced-precision mode of BASELINE configs[4] ("fp16 MFMA convs") for the decoders' 3x3 / 3x3x3 layers on the
 * eight-wave two-tile kernel (csrc/conv_igemm_f16x2_w8.h, NPROD = 1): plain fp16 operands -- the LEADING product of the fp16
 * split alone --, fp32 accumulation, fp32 tensors; the operands saturate at +-65504 as in emo_conv_igemm_f16acc32 (no range
 * word, no guarded recomputation).  wpk1 = emoportraits_amd.pack.pack_weight_f16w8(w): the first plane of the split layout,
 * [channel tile][Cin chunk of 16][kd][kernel row][kernel column][half][64][8] fp16 of w * w_scale (a power of two; the result
 * is multiplied by 1 / w_scale).  One launch form only -- the straight-line epilogue's: cfg 3, ksplit 1, no activation, whole
 * 64-channel tiles, 4 x 64 position tiles (Wl % 64 == 0, Hl % 4 == 0), 16-byte aligned tensors, at least two pair items per CU --
 * EMO_ERR_UNSUPPORTED otherwise (run emo_conv_igemm_f16acc32).  Replaces the same reference code as emo_conv_igemm_f32
 * (networks/volumetric_avatar/utils.py:661-788) under notebooks/infer_s2.py:351-387's decoder. */
int emo_conv_igemm_f16w8(const float* x, const void* wpk1, const float* bias, const float* scale, const float* shift,
                         const float* res, float* out, int N, int Cin, int Cout, int D, int H, int W, int KD, int KH, int KW,
                         int ups, int relu_in, int act, int res_ups, int cfg, int ksplit, float* workspace, float* gn_stats,
                         void* stream, float w_scale);

/* ABI 10.  The same mode for a layer with an ODD number (>= 3) of 64-channel tiles (the decoder's 192- and 320-channel layers,
 * networks/volumetric_avatar/decoder.py:277): emo_conv_igemm_f16w8 would run the last tile in a half-empty pair that costs a
 * whole pair's staging; here the whole pairs run that kernel (wpk1, as above) and the last tile runs
 * emo_conv_igemm_f16acc32's kernel on the same arguments (wpk16: THAT entry's layout for cfg 3, the whole layer's weights) --
 * two launches on `stream`, every output element and every gn_stats entry written once.  The launch must be in the form of
 * BOTH kernels (emo_conv_igemm_f16w8's above; emo_conv_igemm_f16acc32's: Wl % 128 == 0 or Wl == 64); EMO_ERR_UNSUPPORTED
 * otherwise and for an even or single tile count. */
int emo_conv_igemm_f16w8_rest(const float* x, const void* wpk1, const void* wpk16, const float* bias, const float* scale,
                              const float* shift, const float* res, float* out, int N, int Cin, int Cout, int D, int H, int W,
                              int KD, int KH, int KW, int ups, int relu_in, int act, int res_ups, int cfg, int ksplit,
                              float* workspace, float* gn_stats, void* stream, float w_scale);

/* ABI 24.  A question, not a launch: the code the convolution entry `entry` would return for a launch with these arguments --
 * EMO_OK, or the EMO_ERR_* of the first condition of the entry or of its kernel's launcher that the launch misses; for
 * EMO_CONV_ENTRY_F16W8_REST both of that entry's launches.  The entry's own code answers, run in a mode in which it launches
 * nothing and makes no HIP call, so a condition of a launch form is written once, in the launcher that enforces it, and a
 * planner asks here (emoportraits_amd.pack).  N .. ksplit, in_scale, w_scale: the entry's arguments of those names (the scales
 * where the entry has them; cfg may be EMO_CONV_CFG_F16X2_UP2 for EMO_CONV_ENTRY_F16X2).  tensors[EMO_CONV_T_COUNT]: each
 * tensor argument as what the conditions read of it, -1 for a null pointer, otherwise its address modulo 16 (FLAG: the
 * overflow_flag of emo_conv_igemm_f16x2; RUN_IF: the run_if of the guarded entries).  ncu > 0: the compute units to assume for
 * the fill rules of the pair kernels (no device is asked, the call works on a machine without one); ncu <= 0: the current
 * device's.  The A/B switches of the launchers (EMO_CONV_CT2, EMO_CONV_CT2_MIN_ITEMS, EMO_F16_W8, ...) apply as they do to a
 * launch.  Thread safe; EMO_ERR_BAD_ARG for an unknown entry or null tensors. */
enum { EMO_CONV_ENTRY_F32 = 0, EMO_CONV_ENTRY_F32_GUARDED = 1, EMO_CONV_ENTRY_BF16X3 = 2, EMO_CONV_ENTRY_F16X2 = 3,
       EMO_CONV_ENTRY_F16ACC32 = 4, EMO_CONV_ENTRY_F16W8 = 5, EMO_CONV_ENTRY_F16W8_REST = 6, EMO_CONV_ENTRY_COUNT = 7 };
enum { EMO_CONV_T_X = 0, EMO_CONV_T_WPK = 1, EMO_CONV_T_WPK16 = 2, EMO_CONV_T_BIAS = 3, EMO_CONV_T_SCALE = 4, EMO_CONV_T_SHIFT = 5,
       EMO_CONV_T_RES = 6, EMO_CONV_T_OUT = 7, EMO_CONV_T_WORKSPACE = 8, EMO_CONV_T_GN_STATS = 9, EMO_CONV_T_FLAG = 10,
       EMO_CONV_T_RUN_IF = 11, EMO_CONV_T_COUNT = 12 };
int emo_conv_accepts(int entry, const int* tensors, int N, int Cin, int Cout, int D, int H, int W, int KD, int KH, int KW,
                     int ups, int relu_in, int act, int res_ups, int cfg, int ksplit, float in_scale, float w_scale, int ncu);

/* fp32 3x3 convolution on the bf16 matrix pipes (NOT a reduced-precision mode): every fp32 operand is the exact sum of three
 * bf16 terms (x = xh + xm + xl, 24 significand bits kept), the six partial products of order <= 2^-16 are accumulated in fp32
 * by v_mfma_f32_32x32x16_bf16; the dropped terms are <= 2^-23 |x w| per product, below the fp32 accumulation error of either
 * kernel.  Same arguments, epilogue, K split and gn_stats as emo_conv_igemm_f32 (reference: torch.nn.Conv2d / Conv3d forward
 * of the decoder and WarpGenerator blocks, networks/volumetric_avatar/utils.py:854-1005, fp32).  3x3 (KD 1 or 3) kernels,
 * cfg 3 (64 x 256 tile = 4 x 64 pixels, or 8 x 32 / 16 x 16 on 32- / 16-wide maps without upsample; one block per CU); output
 * width % 64 == 0 and height % 4 == 0, or width 32 and height % 8 == 0, or width 16 and height % 16 == 0; Cin % 8 == 0; x 16-byte
 * aligned; Cin <= 1024 when scale / shift are given.  wpk3: bf16 weights packed
 * [co_tile][Cin chunk of 16][kd][kernel row][plane h|m|l][kernel column][half][BM = 64][8] (channel in chunk = 8*half + 0..7).
 * Operand range (tests/test_conv_bf16x3_gpu.py::test_conv_bf16x3_operand_contract): the split is exact for every finite staged
 * value up to the largest finite bf16, 3.3895e38 (0x7f7f0000); staged values beyond it, +-inf included, SATURATE there (their
 * first bf16 term would round to infinity and the residual inf - inf to NaN) -- the exact-fp32 kernel passes +-inf on.  A NaN
 * input is staged as the lower clamp bound (0 with relu_in, else -3.39e38) by the v_med3 that also applies ReLU and zero padding,
 * exactly as in emo_conv_igemm_f32.  Signed zeros and fp32 subnormals are split like any other value (a subnormal's terms are
 * bf16 subnormals; the matrix pipe may flush them: absolute error <= 2^-126 per product).
 * run_if   NULL, or a device word: the launch (both halves of a K-split launch) does nothing unless *run_if != 0 when it starts
 *          executing -- the guarded fallback behind emo_conv_igemm_f16x2's overflow_flag (same stream, launched right after it). */
int emo_conv_pack_info_bf16x3(int KH, int KW, int cfg, int* BM, int* KC);
int emo_conv_igemm_bf16x3(const float* x, const void* wpk3, const float* bias,
                          const float* scale, const float* shift, const float* res, float* out,
                          int N, int Cin, int Cout, int D, int H, int W, int KD, int KH, int KW,
                          int ups, int relu_in, int act, int res_ups, int cfg, int ksplit, float* workspace,
                          float* gn_stats, void* stream, const int* run_if);

/* Companion of emo_conv_igemm_bf16x3 with half the matrix work: the SCALED operands (x * in_scale after the producer's
 * norm + ReLU, w * w_scale; powers of two) as the sum of two fp16 terms -- 22+ significand bits, exact to 2^-24 relative for
 * |value| >= 2^-2, to 2^-25 absolute below -- and the three partial products x1 w1 + x1 w2 + x2 w1 (dropped: x2 w2 <= 2^-24),
 * fp32 accumulation, result * 1 / (in_scale * w_scale).  Error against an fp64 convolution: that of a plain fp32 convolution
 * (tools/split_accuracy.py; tests/test_conv_bf16x3_gpu.py).  wpk2: fp16 weights packed like wpk3 with two planes
 * [.. kernel row][plane 1|2][kernel column][half][BM = 64][8].  Otherwise as emo_conv_igemm_bf16x3.
 * CONTRACT, checked on the device: |x * in_scale| saturates at 65504 (in_scale 32: staged inputs beyond +-2047 are clipped).
 *   overflow_flag  NULL (unchecked), or a device word the caller has zeroed: every thread tracks the largest |x * in_scale| it
 *          stages BEFORE the clamp (one v_max3 per two values) and the launch stores 1 there if any exceeded 65504 (+-inf
 *          included; a NaN is staged as the lower clamp bound like everywhere else and does not raise it).  Halo pixels are
 *          checked by every block that stages them; a value that is only ever clamped away by relu_in (below -65504) still
 *          raises the flag -- conservative.
 *   The caller then launches emo_conv_igemm_bf16x3 on the same arguments with run_if = overflow_flag on the same stream: it
 *   recomputes `out` (and gn_stats) only when the flag was raised -- no host synchronisation, hipGraph-capturable; the pair
 *   is what emoportraits_amd.ops.conv_igemm issues for a precision="f16x2" layer
 *   (tests/test_conv_bf16x3_gpu.py::test_conv_f16x2_overflow_is_detected_and_recomputed). */
int emo_conv_igemm_f16x2(const float* x, const void* wpk2, const float* bias,
                         const float* scale, const float* shift, const float* res, float* out,
                         int N, int Cin, int Cout, int D, int H, int W, int KD, int KH, int KW,
                         int ups, int relu_in, int act, int res_ups, int cfg, int ksplit, float* workspace,
                         float* gn_stats, void* stream, float in_scale, float w_scale, int* overflow_flag);

/* ABI 7.  POINTWISE layers on the fp16 split: emo_conv_igemm_f16x2 also takes KH = KW = 1 (KD = 1; 2-D, or 3-D with D as a
 * batch of planes) -- nn.Conv2d(Cin, Cout, 1) of decoder.py:66-70 (1536 -> 512) and the 1x1 skips of utils.py:764-781 -- on a
 * kernel of its own (csrc/conv_igemm_f16x2_p1.h: two 64-channel output tiles per work item on one converted patch).  wpk2 then is
 * [channel tile, padded to an even count][Cin chunk of 32][plane 1|2][k-step of 16][half][BM = 64][8] fp16 of w * w_scale
 * (emoportraits_amd.pack.pack_weight_f16x2_1x1).  Launch form: ksplit 1, ups 0, act EMO_ACT_NONE, Cout % 64 == 0, W % 64 == 0,
 * H % 4 == 0, 16-byte aligned x / out / res; EMO_ERR_UNSUPPORTED otherwise (such a launch runs emo_conv_igemm_f32).  Contract
 * and overflow_flag as above; the guarded exact recomputation behind it is
 * emo_conv_igemm_f32_guarded: emo_conv_igemm_f32 with run_if (NULL, or a device word: the launch does nothing unless
 * *run_if != 0 when it starts executing), same stream, launched right after the fp16-split launch. */
/* ABI 7, also: emo_conv_igemm_f16x2 takes cfg 5 (block config F: 32 channels x 256 positions) for 3x3 / 3x3x3 layers -- a 32-row
 * channel tile for layers with at most 32 output channels (the WarpGenerator's last 3-D block and its 3-channel head,
 * warp_generator_resnet.py:95-123; stage 2's 32-channel ResBlocks), which ran the 64-row tile half empty.  wpk2 is then packed
 * with BM = 32 (emoportraits_amd.pack.pack_weight_f16x2(w, bm=32)); 4 x 64 position tiles (W % 64 == 0, H % 4 == 0), no fused
 * upsample.  The guarded recomputation of such a layer is emo_conv_igemm_bf16x3 with cfg 3 and the BM = 64 weights, as for
 * every 3x3 layer.  A 3x3x3 launch that runs of at least six output slices spread over the whole device is computed by the
 * depth-shared form of the tile (csrc/conv_igemm_f16x2_zs.h: every staged input slice feeds all three depth taps): same
 * arguments, weights, statistics layout and overflow word; results differ from the one-slice kernel's only by the order in
 * which an output's (channel chunk, depth tap) contributions are accumulated. */
/* ABI 11.  emo_conv_igemm_f16x2 with cfg = EMO_CONV_CFG_F16X2_UP2: a 3x3 layer with the fused nearest x2 upsample (ups = 1) as
 * four 2x2 PHASE convolutions on the low-res input (csrc/conv_inst_f16x2_up2.hip): output pixel (2i + p, 2j + q) = sum over
 * a, b in {0, 1} of w_pq[a][b] . x[i - 1 + p + a][j - 1 + q + b], w_pq[a][b] = sum of the 3x3 taps w[r][s], r in R_p[a],
 * s in R_q[b], R_0 = ({0}, {1, 2}), R_1 = ({0, 1}, {2}) -- 4 instead of 9 Cin MACs per output.  Same arithmetic (two fp16 terms
 * of the scaled operands, three products, fp32 accumulation), operand-range contract and overflow_flag as above; the guarded
 * recomputation behind it is the same emo_conv_igemm_bf16x3 launch (cfg 3, the DIRECT 3x3 weights).
 *   wpk2 then is [co_tile][Cin chunk of 16][p][q][a][b][plane 1|2][half][BM = 64][8] fp16 of w_pq * w_scale, the sums taken in
 *          fp64 from the fp32 weights, w_scale = the power of two that puts max|w_pq| into [512, 1024), both planes split from
 *          fp64 (channel in chunk = 8 * half + 0..7; emoportraits_amd.pack.pack_weight_f16x2_up2).
 * Launch form (a planner asks emo_conv_accepts for it, ABI 24): ups 1, D 1, KD 1, KH = KW = 3, ksplit 1, no residual,
 * act EMO_ACT_NONE, Cout % 64 == 0, Cin % 8 == 0 (Cin <= 1024 with scale / shift), W % 64 == 0, H % 2 == 0, 16-byte aligned
 * x and out, Cin * H * W * 4 < 2^32; EMO_ERR_UNSUPPORTED (EMO_ERR_ALIGN) otherwise.  gn_stats: the TileStats layout of block
 * config D, [N][4 x 64 output tiles][Cout][2]. */
#define EMO_CONV_CFG_F16X2_UP2 7

int emo_conv_igemm_f32_guarded(const float* x, const float* wpk, const float* bias,
                               const float* scale, const float* shift, const float* res, float* out,
                               int N, int Cin, int Cout, int D, int H, int W, int KD, int KH, int KW,
                               int ups, int relu_in, int act, int res_ups, int cfg, int ksplit, float* workspace,
                               float* gn_stats, void* stream, const int* run_if);

/* ABI 8.  Pointwise convolution with at most 4 output channels as a stream (the decoder's image head: GroupNorm -> ReLU ->
 * 1x1 conv 128 -> 3 -> sigmoid, decoder.py:381-392): one 16-byte load per (channel, four positions), fp32 FMAs, no LDS.
 *   out[n][o][p] = act(bias[o] + sum_c w[o][c] * in(x[n][c][p])),  in(v) = v * scale[n][c] + shift[n][c], then max(., 0) if relu_in
 *   x [N, Cin, S] (S positions per channel: any spatial rank), w [Cout, Cin] plain row-major fp32 (NOT a packed layout),
 *   bias [Cout] or NULL, scale / shift [N, Cin] both or neither, act EMO_ACT_*.
 * Cout <= 4, S % 4 == 0 (EMO_ERR_UNSUPPORTED otherwise), 16-byte aligned x / out (EMO_ERR_ALIGN): such launches run
 * emo_conv_igemm_f32.  The sum over the channels is sequential in fp32 (the MFMA kernel's is blocked): same bounds against the
 * oracle, not the same bits. */
int emo_conv_head_f32(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
                      float* out, int N, int Cin, int Cout, int64_t S, int relu_in, int act, void* stream);

/* ABI 16.  The tail of stage 2 as one stream launch: the image head norm -> ReLU -> 1x1 conv Cin -> 3 -> tanh at the full
 * resolution (decoder_s2_old.py:444-456), the residual added under the matte x face mask and clamped (notebooks/infer_s2.py:
 * 365-375), written as fp32 planes and / or as HWC bytes.  emo_conv_head_f32's channel walk with another epilogue:
 *   out = clamp(img + tanh(bias[o] + sum_c w[o][c] * in(x[n][c][p])) * (mask * face_mask), 0, 1),  in(.) as emo_conv_head_f32
 *   x [N, Cin, S], w [3][Cin] plain row-major, bias [3] or NULL, scale / shift [N, Cin] both or neither, img [N,3,S],
 *   mask [N,1,S], face_mask [N,1,S] or NULL (= 1), out_f32 [N,3,S] or NULL, out_u8 [N,S,3] (the bytes emo_pack_rgb8 writes) or
 *   NULL; at least one of the two outputs (EMO_ERR_BAD_ARG otherwise).
 * The operations and their order are those of emo_conv_head_f32(act = EMO_ACT_TANH) -> emo_stage2_compose_f32 -> emo_pack_rgb8
 * (sequential fp32 FMA sum, tanhf, gate = mask * face_mask, img + add * gate as two rounded operations, clamp, (uint8)(v * 255)):
 * both outputs are bit-identical to that chain on the same operands.
 * S % 4 == 0 and N <= 65535 (EMO_ERR_UNSUPPORTED otherwise); x, img, mask, face_mask, out_f32 16-byte and out_u8 4-byte aligned
 * (EMO_ERR_ALIGN): such launches run the chain. */
int emo_stage2_head_f32(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
                        const float* img, const float* mask, const float* face_mask, float* out_f32, uint8_t* out_u8,
                        int N, int Cin, int64_t S, int relu_in, void* stream);

/* ---------------------------------------------------------------------------------------------
 * resampling / pointwise helpers (HBM-bound, one pass)
 *   emo_upsample_trilinear_f32: F.interpolate(x, scale_factor=(fd,fh,fw), mode='trilinear'), factors in {1,2}
 *       (warp_generator_resnet.py:163-166; unet_3d.py:223,269-272).  x [NC, D, H, W] -> [NC, D*fd, H*fh, W*fw]
 *   emo_avgpool_f32: nn.AvgPool2d/3d with kernel == stride in 1..16 per axis (utils.py:962-967; integer-window
 *       AdaptiveAvgPool2d of the embedders)
 *   emo_add_f32: out[i] = (a[i] + b[i % period]) * alpha   (unet_3d.py:281; va.py:857)
 */
int emo_upsample_trilinear_f32(const float* x, float* out, int64_t NC, int D, int H, int W,
                               int fd, int fh, int fw, void* stream);
/* ABI 8.  emo_upsample_trilinear_f32 with the GroupNorm statistics of its OUTPUT reduced on the way (WarpGenerator:
 * F.interpolate -> ResBlock3d, whose first norm would otherwise read the upsampled tensor once more;
 * warp_generator_resnet.py:163-166, utils.py:711-731).  x [N, C, D, H, W]; `partial` (>= emo_groupnorm_workspace_bytes(N, G)
 * bytes) receives *split_out slices per (sample, group) for emo_groupnorm_affine_from_sums_f32.  fw = 2, W even and a 16-byte
 * aligned `out` only: EMO_ERR_UNSUPPORTED otherwise (run the two operations one after the other). */
int emo_upsample_trilinear_gn_sums_f32(const float* x, float* out, int N, int C, int G, int D, int H, int W,
                                       int fd, int fh, int fw, void* partial, int64_t partial_bytes, int* split_out,
                                       void* stream);
int emo_avgpool_f32(const float* x, float* out, int64_t NC, int D, int H, int W, int kd, int kh, int kw, void* stream);
int emo_add_f32(const float* a, const float* b, float* out, int64_t n, int64_t period, float alpha, void* stream);
/* ABI 12.  emo_add_f32 with one table row per batch row: out[b][i] = (a[b][i] + table[index[b]][i]) * alpha, the same roundings
 * (add, then multiply), so rows whose indices are all equal are bit for bit the `period` form with b = that table row.
 *   a, out [B, row]; table [num_rows, row]; index [B] int32, DEVICE memory.  An index outside [0, num_rows) writes a zero row. */
int emo_add_rows_indexed_f32(const float* a, const float* table, const int32_t* index, float* out, int B, int num_rows,
                             int64_t row, float alpha, void* stream);

/* ABI 28.  A question, not a launch: the kernel and the launch plan that the launcher of `op` takes for these arguments.  The
 * launcher's own host function answers -- the one it calls itself before it launches -- so a condition of a form is written
 * once; no HIP call is made and the call works on a machine without a device.  Returns what the launcher would return before
 * any launch (EMO_ERR_BAD_ARG, EMO_ERR_UNSUPPORTED; then plan is all zero), otherwise EMO_OK with plan[EMO_OP_PLAN_COUNT] filled.
 *   x, out: the launcher's first input and its output, read for nullness and 16-byte alignment only (out is not read for
 *           EMO_OP_GROUPNORM_AFFINE).  dims: the launcher's integer shape arguments in its own order --
 *     EMO_OP_UPSAMPLE_TRILINEAR          (NC, D, H, W, fd, fh, fw)        emo_upsample_trilinear_f32
 *     EMO_OP_UPSAMPLE_TRILINEAR_GN_SUMS  (N, C, G, D, H, W, fd, fh, fw)   emo_upsample_trilinear_gn_sums_f32
 *     EMO_OP_AVGPOOL                     (NC, D, H, W, kd, kh, kw)        emo_avgpool_f32
 *     EMO_OP_GROUPNORM_AFFINE            (N, C, S, G)                     emo_groupnorm_affine_f32, its own pass
 *   plan[EMO_OP_PLAN_FORM]: the kernel, an EMO_*_FORM_* of the op.  GRID: thread blocks of the launch.  ITEMS: work items of the
 *   launch (outputs; quads of outputs for the x4 pooling kernels; blocks of up to 4 x 2 x 2 outputs for the block upsampling
 *   kernel; elements read for GroupNorm) -- a grid-stride kernel takes a second trip where ITEMS > 256 GRID.
 *   Block upsampling kernel and GroupNorm only (0 otherwise): RUNS x SPLIT = GRID, a run being CR consecutive (sample, channel)
 *   volumes (GN_SUMS: the channels of a group; GroupNorm: one (sample, group), CR = 0) of RUN_ITEMS items, cut into SPLIT slices;
 *   PER: items per slice of the upsampling kernel, the last slice holding the rest (RUN_ITEMS - (SPLIT - 1) PER, never empty). */
enum { EMO_OP_UPSAMPLE_TRILINEAR = 0, EMO_OP_UPSAMPLE_TRILINEAR_GN_SUMS = 1, EMO_OP_AVGPOOL = 2, EMO_OP_GROUPNORM_AFFINE = 3,
       EMO_OP_COUNT = 4 };
enum { EMO_UPSAMPLE_FORM_GENERIC = 0, EMO_UPSAMPLE_FORM_BLOCK = 1, EMO_UPSAMPLE_FORM_COUNT = 2 };
enum { EMO_AVGPOOL_FORM_GENERIC = 0, EMO_AVGPOOL_FORM_X4_W1 = 1, EMO_AVGPOOL_FORM_X4_W2 = 2, EMO_AVGPOOL_FORM_COUNT = 3 };
enum { EMO_GROUPNORM_FORM_PASS = 0, EMO_GROUPNORM_FORM_COUNT = 1 };
enum { EMO_OP_PLAN_FORM = 0, EMO_OP_PLAN_GRID = 1, EMO_OP_PLAN_ITEMS = 2, EMO_OP_PLAN_CR = 3, EMO_OP_PLAN_RUNS = 4,
       EMO_OP_PLAN_SPLIT = 5, EMO_OP_PLAN_PER = 6, EMO_OP_PLAN_RUN_ITEMS = 7, EMO_OP_PLAN_COUNT = 8 };
int emo_op_launch_form(int op, const void* x, const void* out, const int64_t* dims, int64_t* plan);

/* f4 -- F.interpolate(x, size=(Ho, Wo), mode='bilinear' (bicubic = 0) | 'bicubic' (1), align_corners=False) on NC
 * planes of H x W: the wrappers' crop resize (notebooks/infer.py:346,399-401,548-552; notebooks/infer_s2.py:360-362).
 * The input is strided (plane_stride / row_stride in floats; H*W / W when contiguous) so that a crop window of a larger
 * frame is read in place; clamp01 clips the result to [0,1] (crop_image, infer.py:350). */
int emo_resize2d_f32(const float* x, int64_t plane_stride, int64_t row_stride, float* out, int64_t NC, int H, int W,
                     int Ho, int Wo, int bicubic, int clamp01, void* stream);
/* ABI 9.  The same with one crop window PER SAMPLE in one launch (the reference crops every frame around its own face box,
 * notebooks/infer.py:301-352, one frame per call): x = N frames of C planes (plane_stride / row_stride in floats), windows =
 * N x (x0, y0, w, h) int32 in DEVICE memory, out [N, C, Ho, Wo].  Bit-identical to N single-window calls. */
int emo_resize2d_windows_f32(const float* x, int64_t plane_stride, int64_t row_stride, const int* windows, float* out, int N,
                             int C, int Ho, int Wo, int bicubic, int clamp01, void* stream);

/* ---------------------------------------------------------------------------------------------
 * f1 -- embedder ResNets (networks/volumetric_avatar/identity_embedder.py:59-69, expression_embedder.py:424-459,
 * head_pose_regressor.py:21-32; bodies = torchvision.models.resnet*).
 *
 * emo_conv2d_generic_f32: F.conv2d(x', w, bias, stride, padding) with x' = relu?(x * scale[n,c] + shift[n,c]) when
 *   scale/shift are given (the producer's norm + ReLU, applied before zero padding), any KH x KW / stride / pad.
 *   wt is the folded weight transposed to [Cin*KH*KW][CoutP] (k = (ci*KH + ky)*KW + kx, CoutP = Cout rounded up to 64,
 *   zero padded).  x [N,Cin,H,W], out [N,Cout,Ho,Wo].  splits > 1 divides K over gridDim.z through
 *   workspace [splits][N*Cout*Ho*Wo] floats, summed in fixed order (deterministic); emo_conv2d_generic_splits returns
 *   the split count the launch heuristic wants for a shape (>= 1; the kernel accepts any value >= 1).
 * emo_maxpool2d_f32:   nn.MaxPool2d(k, stride, pad) of relu?(x * scale + shift) (scale/shift [NC] or NULL).
 * emo_affine_add_relu_f32: out = relu?((a*sa+ta) + (b*sb+tb)), per-(n,c) affines optional, b optional: the tail of
 *   BasicBlock / Bottleneck.forward.
 * emo_grid_sample2d_f32: F.grid_sample(img, grid) 4-D bilinear / zeros / align_corners=False; either an explicit
 *   grid [N,Ho,Wo,2] or theta [N,2,3] + lin [Ho] (grid = theta @ (lin[xo], lin[yo], 1): expression_embedder.py:221-231);
 *   grid_out (optional) receives the grid that was used.  A grid value that is NaN, infinite or beyond the int range in pixels
 *   has no corner in range and reads nothing: the output is ATen's there (NaN from the weights of a NaN or infinite value, else 0). */
int emo_conv2d_generic_f32(const float* x, const float* wt, const float* bias, const float* scale, const float* shift,
                           float* out, int N, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad,
                           int relu_in, int splits, float* workspace, void* stream);
int emo_conv2d_generic_splits(int N, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad);
int emo_maxpool2d_f32(const float* x, const float* scale, const float* shift, float* out, int64_t NC, int H, int W,
                      int k, int stride, int pad, int relu, void* stream);
int emo_affine_add_relu_f32(const float* a, const float* sa, const float* ta, const float* b, const float* sb,
                            const float* tb, float* out, int64_t NC, int64_t S, int relu, void* stream);
int emo_grid_sample2d_f32(const float* img, const float* grid, const float* theta, const float* lin, float* out,
                          float* grid_out, int N, int C, int H, int W, int Ho, int Wo, void* stream);

/* stage-2 glue (notebooks/infer_s2.py:365-375):
 *   emo_mul_mask_f32:        out[n,c,p] = img[n,c,p] * mask[n,0,p]            (local_encoder input, :370)
 *   emo_stage2_compose_f32:  out = clamp(img + add * (mask * face_mask), 0, 1)   (:365,373-375); masks are [N,1,H,W] */
int emo_mul_mask_f32(const float* img, const float* mask, float* out, int N, int C, int64_t HW, void* stream);
int emo_stage2_compose_f32(const float* img, const float* add, const float* mask, const float* face_mask, float* out,
                           int N, int C, int64_t HW, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a3/a4/a5 -- small wave-reduced kernels
 *   emo_small_gemm_f32: C[b][m][0..NN) = sum_k A[m][k] * B[b][k][0..NN), NN in {1,2,4,16}: pose_unsqueeze_nw Linear
 *       (va.py:172-173,820-823), warp_embed_head_orig_nw 1x1 conv on 4x4 (va.py:177-181,857), WarpGenerator.first_conv
 *       (warp_generator_resnet.py:70,141), ProjectorNorm u @ embed (utils.py:1137-1151).
 *   emo_projector_finalize_f32: (u@embed) @ v -> (d_gamma, d_beta), then ada_gamma = gamma + d_gamma, ada_beta = beta +
 *       d_beta (utils.py:1146-1149 + assign_adaptive_norm_params :983-995) for all adaptive norms of a net at once:
 *       T [B, R, E], V [n_norms, E, 2], norm_of_row [R] int32, gamma/beta [R] -> ada_gamma/ada_beta [B, R].
 *   emo_pose_theta_f32: utils/point_transforms.py:188-242 get_transform_matrix -> theta [B,4,4]; scale [B,scale_cols].
 *   emo_pack_rgb8: notebooks/infer.py:641-644 clamp(0,1) + ToPILImage: [N,3,H,W] fp32 -> [N,H,W,3] uint8.
 *   emo_unpack_rgb8: notebooks/infer.py:211-223 convert_to_tensor (ToTensor) of decoded video frames:
 *       [N,H,W,3] uint8 -> [N,3,H,W] fp32 = byte / 255, on the device (frames are uploaded as bytes: 4x less PCIe).
 */
int emo_small_gemm_f32(const float* A, const float* B, float* C, int M, int K, int NN, int batch,
                       int64_t b_stride, int64_t c_stride, void* stream);
int emo_projector_finalize_f32(const float* T, const float* V, const int* norm_of_row, const float* gamma,
                               const float* beta, float* ada_gamma, float* ada_beta, int B, int R, int E, void* stream);
int emo_pose_theta_f32(const float* scale, int scale_cols, const float* rotation, const float* translation,
                       float* theta, int B, void* stream);
/* inverse of B row-major 4x4 matrices (`theta.float().inverse()`: notebooks/infer.py:443, expression_embedder.py:185-188) */
int emo_mat4_inverse_f32(const float* in, float* out, int B, void* stream);
/* ABI 13.  notebooks/infer.py:686-736 get_mixing_theta on the device, one frame per thread: frame n keeps the stretch of source
 * theta source[index[n]] and takes rotation and translation from target[n] (hostglue.mixing_theta for one source and one target).
 *   target [B,4,4], source [K,4,4] (a bank of source thetas), index [B] int32 DEVICE memory or NULL (every frame: source 0),
 *   out [B,4,4]: rows 0..2 the mixed theta, row 3 (0,0,0,1).
 * fp64 from the fp32 inputs, each output rounded to fp32 once; polar decomposition by a one-sided Jacobi SVD (det < 0 included).
 * mix_old != 0: [U_t P_s | t_t]; 0: P_s4 * mean(P_t4) / mean(P_s4) @ U_t4 @ T4 on the 4x4 homogeneous matrices.  A non-finite
 * source linear part, or an index outside [0, K) (the source is then not read), gives the target unchanged; a non-finite
 * target linear part gives [P_s | 0]. */
int emo_mixing_theta_f32(const float* target, const float* source, const int32_t* index, int B, int K, int mix_old, float* out,
                         void* stream);
/* ABI 13.  notebooks/infer.py:571-581 smooth_pose with one EMA stream per source identity: frame i (values [n,16], frame order)
 * belongs to stream stream_of[i] ([n] int32 DEVICE memory, or NULL: stream 0).  state [K,16] and has_state [K] int32 are read and
 * written: a stream without state starts at its first frame's value, then cur = v * m + cur * om (two rounded fp32 products,
 * one rounded sum), out[i] = cur -- per stream bit for bit hostglue.ema_scan with om = fp32(1 - momentum) formed by the caller.
 * A stream index outside [0, K) leaves its frames unwritten. */
int emo_theta_ema_scan_f32(const float* values, const int32_t* stream_of, float* state, int32_t* has_state, int n, int K, float m,
                           float om, float* out, void* stream);
/* ABI 20.  The expression controls of the batched entry points: relative transfer and gain about each identity's source
 * expression, an additive offset and an EMA, per stream and in row order.  Row i (values [n,E], frame order) belongs to stream
 * k = stream_of[i] ([n] int32 DEVICE memory, or NULL: stream 0).  neutral [K,E] or NULL, gain [n] or NULL, offset [n,E] or NULL;
 * anchor and ema [K,E] with their flags has_anchor and has_ema [K] int32 are read and written; out [n,E] may be `values`.
 * For every element j, within a stream in row order, every operation fp32 and rounded on its own:
 *   e = values[i,j]
 *   if neutral:  r = neutral[k,j], or with `relative` anchor[k,j] -- which a stream without anchor takes from its first row
 *                (anchor[k,j] = e, has_anchor[k] = 1 afterwards);  t = e - r;  if gain: t = t * gain[i];  e = neutral[k,j] + t
 *   if offset:   e = e + offset[i,j]
 *   if smooth:   a stream without EMA starts at cur = e; then a = e * m, b = cur * om, cur = a + b, e = cur as
 *                emo_theta_ema_scan_f32 (ema[k,j] = cur, has_ema[k] = 1 afterwards), om = fp32(1 - momentum) formed by the caller
 *   out[i,j] = e
 * -- bit for bit hostglue.expression_controls.  A stream index outside [0, K) leaves its row unwritten and touches no state.
 * EMO_ERR_BAD_ARG before any launch: values or out NULL; n, K or E <= 0; relative or gain without neutral; relative without
 * anchor and has_anchor; smooth without ema and has_ema.  One block per stream, no atomics. */
int emo_expr_controls_f32(const float* values, const int32_t* stream_of, const float* neutral, const float* gain,
                          const float* offset, float* anchor, int32_t* has_anchor, float* ema, int32_t* has_ema, int n, int K,
                          int E, int relative, int smooth, float m, float om, float* out, void* stream);
/* ABI 21.  The head-pose controls of the batched entry points: the (scale, rotation, translation) of every row edited before
 * theta is formed -- the reference's `normalize`, `delta_yaw` and `delta_pitch` (expression_embedder.py:302-316), relative
 * transfer and gain about each identity's source pose, offsets and a zoom.  Row i (scale [n,scale_cols], scale_cols 1 or 3, a
 * single column broadcast to three; rotation [n,3] = yaw, pitch, roll; translation [n,3]) belongs to stream k = stream_of[i]
 * ([n] int32 DEVICE memory, or NULL: stream 0).  source [K,9] or NULL, gain [n] or NULL, rotation_offset and translation_offset
 * [n,3] or NULL, zoom [n] or NULL; anchor [K,9] with its flags has_anchor [K] int32 is read and written.  A row is nine floats
 * p = [sx sy sz | yaw pitch roll | tx ty tz]; every operation fp32 and rounded on its own, clamp(v) = v limited to
 * [-pi/2, pi] with emo_pose_theta_f32's fp32 constants:
 *   0. p.rot = clamp(p.rot)
 *   1. if frontal:  yaw = pitch = 0, p.trans = 0   (roll and scale stay)
 *   2. if source:   q = source[k] with q.rot = clamp(q.rot);  ref = q, or with `relative` anchor[k] -- which a stream without
 *                   anchor takes from its first row after step 0 (has_anchor[k] = 1 afterwards);
 *                   d = p.rot - ref.rot;  if gain: d = d * gain[i];  p.rot = q.rot + d;  the same for p.trans;
 *                   with `relative` only:  p.scale = q.scale * (p.scale / ref.scale)
 *   3. if rotation_offset: p.rot += rotation_offset[i];  if translation_offset: p.trans += translation_offset[i];
 *      if zoom: p.scale *= zoom[i]
 *   4. out_srt[i] = p ([n,9]);  out_theta[i] = S R T of p ([n,16]), bit for bit emo_pose_theta_f32 of p (which clamps once more)
 * -- bit for bit hostglue.head_pose_controls.  A stream index outside [0, K) leaves its row unwritten and touches no state; a
 * stream without a row keeps its flag.  out_srt and out_theta must not overlap any input.
 * EMO_ERR_BAD_ARG before any launch: scale, rotation, translation, out_srt or out_theta NULL; n or K <= 0; scale_cols not 1 or
 * 3; relative or gain without source; relative without anchor and has_anchor; relative together with frontal.
 * One block per stream, its threads take the stream's rows in parallel; no atomics. */
int emo_head_pose_controls_f32(const float* scale, int scale_cols, const float* rotation, const float* translation,
                               const int32_t* stream_of, const float* source, const float* gain, const float* rotation_offset,
                               const float* translation_offset, const float* zoom, float* anchor, int32_t* has_anchor, int n,
                               int K, int relative, int frontal, float* out_srt, float* out_theta, void* stream);
/* ABI 23.  Face boxes in, crop windows out: the window arithmetic of crop_image (notebooks/infer.py:301-352: box -> centre and
 * size, `scale`, the use_smoothed_crop EMA, fixed_bounding_box, remove_overflow at :243-261) for the M rows of a batch, with the
 * tracker's state carried along the row order.  Row i (boxes [M,4] DOUBLE, frame order) belongs to tracker stream k = stream_of[i]
 * ([M] int32 DEVICE memory, or NULL: stream 0) and to a frame of W x H pixels = sizes[i] ([M,2] int32 DEVICE memory = (W, H) per
 * row, or NULL: Wf x Hf for every row).  state [K,3] double = (cx, cy, size) with its flags has_state [K] int32, and last [K,4]
 * int32, the stream's last present window (side 0: none), are read and written; state and has_state may be NULL without
 * `smooth`, last may be NULL without `hold` (it is then not kept).  crop and paste [M,4] int32 = (x0, y0, w, h); face_scale [M]
 * double or NULL.  Every operation is a double operation rounded on its own (no contraction); a value becomes an integer only
 * after its range test:
 *   box:      box_format 0: (x0, y0, x1, y1) = boxes[i].  box_format 1: boxes[i] = (xmin, ymin, width, height) relative to the
 *             frame, x0 = W * xmin, y0 = (H * ymin) * 0.9, x1 = W * (xmin + width), t = H * (ymin + height * 1.2),
 *             y1 = H - 1 if H - 1 < t else t   (notebooks/infer.py:385-391)
 *   missing:  a component of the box is not finite or has magnitude >= 2^30, or k is outside [0, K).  A missing row does not
 *             touch the tracker; a k outside [0, K) touches no state at all.
 *   centre:   cx = floor((x1 + x0) / 2), cy = floor((y1 + y0) / 2), size = (((x1 - x0) + y1) - y0) * scale
 *   smooth:   a stream without state takes (cx, cy, size) as its state (has_state[k] = 1 afterwards); otherwise, unless `fixed`,
 *             state = v * m + state * om for each of the three, om = 1 - momentum formed by the caller in double; the row goes
 *             on with the state
 *   window:   cx, cy, size = rint of each (half to even); absent unless size is finite and >= 2; size -= fmod(size, 2);
 *             half = size / 2, b = (cx - half, cy - half, cx + half, cy + half), over = max(0 | -b0, 0 | -b1, 0 | b2 - W,
 *             0 | b3 - H) (each term where the box leaves the frame), b0 += over, b1 += over, b2 -= over, b3 -= over;
 *             side = trunc((b2 - b0 + b3 - b1) / 2), side -= fmod(side, 2); absent unless side >= 2; absent unless |cx|, |cy| and
 *             side are below 2^30; then, as integers, x_lo = cx - side / 2, y_lo = cy - side / 2
 *   present:  side > 0, x_lo >= 0, y_lo >= 0, x_lo <= W - side, y_lo <= H - side (the test the crop and paste entry points make
 *             of a host window) and side >= min_side.  Then crop[i] = paste[i] = (x_lo, y_lo, side, side), last[k] is that window
 *             and face_scale[i] = side / size (the even size).
 *   missing or absent:  face_scale[i] = 0.  With `hold`, if last[k] has a side and passes the test of `present` for this row's
 *             frame: crop[i] = paste[i] = last[k].  Otherwise crop[i] = the centred square of side s = min(W, H) at
 *             ((W - s) / 2, (H - s) / 2), which can always be read, and paste[i] = (0, 0, 0, 0), which every paste entry point
 *             skips.
 * -- bit for bit hostglue.crop_track.  EMO_ERR_BAD_ARG before any launch: boxes, crop or paste NULL; M or K <= 0; sizes NULL and
 * Wf or Hf < 1; smooth without state and has_state; hold without last; m outside (0, 1] or om outside [0, 1); a scale that is
 * not finite; box_format not 0 or 1; min_side < 1.  Streams across threads, each walking its rows in order; no atomics. */
int emo_crop_track_f64(const double* boxes, const int32_t* stream_of, const int32_t* sizes, int Wf, int Hf, double* state,
                       int32_t* has_state, int32_t* last, int M, int K, double m, double om, int smooth, int fixed, double scale,
                       int box_format, int hold, int min_side, int32_t* crop, int32_t* paste, double* face_scale, void* stream);
/* ABI 25.  Unordered face detections in, ordered track rows out: greedy IoU association of the detections of every frame to the
 * P track slots of its video stream, the frames walked in order, so that a detector's output (a varying number of boxes per frame,
 * in no stable order) becomes the boxes [F,P,4] that emo_crop_track_restarts_f64 takes, column p the same face from frame to frame.
 *   dets [F,D,4] DOUBLE, frame order, D <= 32 detections per frame, rows that are not detections padded with NaN; stream_of [F]
 *   int32 DEVICE memory (or NULL: stream 0): the video stream of frame f; ref [K,P,4] double = (x0, y0, x1, y1) of each track's
 *   last matched box and age [K,P] int32 are the streams' state, read and written (P <= 16): age[k,p] = -1 means slot p is free,
 *   >= 0 that the track is live and has gone that many consecutive frames without a match (ref of a free slot means nothing).
 *   boxes_out [F,P,4] double, restart [F,P] int32, track_of [F,D] int32.
 * Every operation is a double operation rounded on its own (no contraction).
 *   box:      of detection d of frame f.  box_format 0: (x0, y0, x1, y1) = dets[f,d].  box_format 1: dets[f,d] = (xmin, ymin, width,
 *             height): (x0, y0, x1, y1) = (d0, d1, d0 + d2, d1 + d3) -- IoU does not change under a scaling of an axis, so the
 *             association needs neither the frame size nor emo_crop_track_f64's 0.9 and 1.2, which stay there: boxes_out holds
 *             the four numbers as they came.
 *   usable:   all four values of the box are finite and below 2^30 in magnitude, x1 > x0 and y1 > y0.
 *   IoU:      of a track's ref a and a box b: iw = min(ax1, bx1) - max(ax0, bx0), ih = min(ay1, by1) - max(ay0, by0); 0 if iw <= 0
 *             or ih <= 0, otherwise inter = iw * ih and IoU = inter / (((ax1 - ax0) * (ay1 - ay0) + (bx1 - bx0) * (by1 - by0)) - inter).
 * A frame f of stream k = stream_of[f], in this order:
 *   1. match: repeat: among the live tracks without a match in this frame and the usable detections without a track, take the
 *             pair of the largest IoU, ties to the smaller p, then to the smaller d; stop when there is no pair or its IoU <
 *             min_iou (a pair at exactly min_iou matches).  For the pair: ref[k,p] = the box, age[k,p] = 0, boxes_out[f,p] = the
 *             four values of dets[f,d] bit for bit, restart[f,p] = 0, track_of[f,d] = p.
 *   2. age:   every live track without a match: age += 1; if age > max_missed it dies: age = -1 and restart[f,p] = 1, otherwise
 *             restart[f,p] = 0.  Either way boxes_out[f,p] = the quiet NaN 0x7ff8000000000000 four times.
 *   3. birth: the usable detections without a track, in ascending d, each take the lowest free slot p, those that step 2 freed
 *             in this frame included: ref[k,p] = the box, age[k,p] = 0, boxes_out[f,p] = dets[f,d] bit for bit, restart[f,p] = 1,
 *             track_of[f,d] = p.  With no free slot left track_of[f,d] = -1.
 *   4. rest:  a slot that was free when the frame began and had no birth: boxes_out[f,p] = the quiet NaN row, restart[f,p] = 0.
 *             A detection that is not usable: track_of[f,d] = -1.
 * A frame whose stream lies outside [0, K): quiet NaN rows, restart = 0, track_of = -1, and no state is touched.
 * -- bit for bit hostglue.track_assign.  EMO_ERR_BAD_ARG before any launch: dets, ref, age or an output NULL; F, D, P or K <= 0;
 * P > 16 or D > 32; min_iou outside (0, 1]; max_missed < 0; box_format not 0 or 1.  One block of one wave per stream: the P x D
 * IoUs of a frame lie across the lanes, the pair of a round is a wave reduction over the total order (IoU, smaller p, smaller
 * d), whose result does not depend on the reduction's shape; frames are sequential; no atomics. */
int emo_track_assign_f64(const double* dets, const int32_t* stream_of, int F, int D, int P, int K, double* ref, int32_t* age,
                         double min_iou, int max_missed, int box_format, double* boxes_out, int32_t* restart, int32_t* track_of,
                         void* stream);
/* ABI 25.  emo_crop_track_f64 with restart [M] int32 DEVICE memory (or NULL: none) -- emo_track_assign_f64's, flattened to the rows:
 * a row i of a stream k in [0, K) with restart[i] != 0 first clears its stream (has_state[k] = 0 under `smooth`, last[k] = (0, 0,
 * 0, 0) where last is given) and is then processed as above: a birth starts the EMA at its own box, and a track that has died is
 * no longer held by `hold`.  emo_crop_track_f64 is this entry point with restart = NULL.  Bit for bit
 * hostglue.crop_track(restart=); the same refusals. */
int emo_crop_track_restarts_f64(const double* boxes, const int32_t* stream_of, const int32_t* sizes, int Wf, int Hf, double* state,
                                int32_t* has_state, int32_t* last, int M, int K, double m, double om, int smooth, int fixed,
                                double scale, int box_format, int hold, int min_side, const int32_t* restart, int32_t* crop,
                                int32_t* paste, double* face_scale, void* stream);
/* ABI 26.  The three per-identity control streams follow the face tracks: emo_theta_ema_scan_f32, emo_expr_controls_f32 and
 * emo_head_pose_controls_f32 with two row masks in front of their outputs, both [n] int32 DEVICE memory:
 *   restart  emo_track_assign_f64's flag, flattened to the rows, or NULL: no restarts;
 *   present  != 0 where the row has a face (emo_crop_track_f64 gave it a paste window with a side), or NULL: every row present.
 * For a row i of a stream k in [0, K), within the stream in row order:
 *   1. restart:  if restart[i] != 0 the stream begins again before the row is looked at -- the scan: has_state[k] = 0; the
 *                expression controls: has_anchor[k] = 0 under `relative`, has_ema[k] = 0 under `smooth`; the head-pose controls:
 *                has_anchor[k] = 0 under `relative` -- whether or not the row is present: a track that died does not leave its
 *                state to the next birth.
 *   2. present:  if present is NULL or present[i] != 0 the row is processed exactly as the entry point without masks processes
 *                it, and the stream's state advances.
 *   3. absent:   otherwise out[i] is what the entry point without masks would write for this row from a private copy of the
 *                stream's state at this point -- the row is its own anchor where the stream has none, and an EMA starts at the
 *                row where the stream has none -- and nothing of the stream is written, neither a state value nor a flag.  The row
 *                is still rendered: its outputs are finite whenever its inputs are.
 * When the launch returns a flag is 1 only if a present row set it after the stream's last restart: a flag that came in as 1 can
 * leave as 0.  The state values of a stream whose flag is 0 mean nothing.  A stream index outside [0, K) leaves its row
 * unwritten, touches no state, and its masks are not looked at.  For the head-pose controls this makes the anchor one per
 * segment: a row's reference is the stored anchor if no restart precedes it in the call, otherwise the first present row at or
 * after the last restart at or before it; an absent row ahead of that first present row is its own reference.  Without
 * `relative` (and for the expression controls without `smooth`) there is no state and the masks change nothing.
 * Each entry point without masks is this one with restart = present = NULL.  Bit for bit hostglue.ema_scan_tracks,
 * hostglue.expression_controls(restart=, present=) and hostglue.head_pose_controls(restart=, present=); the refusals, the launch
 * shapes and "no atomics" are those of the entry points without masks. */
int emo_theta_ema_scan_tracks_f32(const float* values, const int32_t* stream_of, float* state, int32_t* has_state, int n, int K,
                                  float m, float om, const int32_t* restart, const int32_t* present, float* out, void* stream);
int emo_expr_controls_tracks_f32(const float* values, const int32_t* stream_of, const float* neutral, const float* gain,
                                 const float* offset, float* anchor, int32_t* has_anchor, float* ema, int32_t* has_ema, int n, int K,
                                 int E, int relative, int smooth, float m, float om, const int32_t* restart, const int32_t* present,
                                 float* out, void* stream);
int emo_head_pose_controls_tracks_f32(const float* scale, int scale_cols, const float* rotation, const float* translation,
                                      const int32_t* stream_of, const float* source, const float* gain, const float* rotation_offset,
                                      const float* translation_offset, const float* zoom, float* anchor, int32_t* has_anchor, int n,
                                      int K, int relative, int frontal, const int32_t* restart, const int32_t* present,
                                      float* out_srt, float* out_theta, void* stream);
/* ABI 27.  The present rows of the crop tracker's windows, first and in order: a stable stream compaction of the M = F * P
 * frame-major rows (frame f holds the rows f * P ... f * P + P - 1) that emo_crop_track(_restarts)_f64 wrote, so that a caller
 * renders the faces that are there and no slot that is empty.
 *   crop, paste [M,4] int32 DEVICE memory: the tracker's windows.  Row i is present iff paste[i][2] > 0 (a side of 0, whatever
 *   its x and y, and a negative side are absent).  count [F], first [F + 1], row_of [M], crop_out [M,4], paste_out [M,4] int32.
 *   first[f], f = 0 ... F: the number of present rows with an index < f * P; first[F] = T, their total.
 *   count[f] = first[f + 1] - first[f], the present rows of frame f.
 *   j < T:   row_of[j] = the index of the j-th present row, ascending; crop_out[j] = crop[row_of[j]], paste_out[j] =
 *            paste[row_of[j]], the four values as they are.
 *   T <= j < M:  row_of[j] = -1, crop_out[j] = paste_out[j] = (0, 0, 0, 0).
 * Every element of every output is written -- bit for bit hostglue.present_rows.  EMO_ERR_BAD_ARG before any launch: a NULL
 * pointer; F <= 0; P outside 1 ... 16; F * P > 2^24; an output that overlaps crop or paste.  EMO_ERR_ALIGN: a window array that is
 * not 16-byte aligned (a row moves as one 16-byte load and one 16-byte store).  One block of 256 threads, each owning a contiguous
 * run of rows: the runs are counted, the run totals meet in LDS behind one barrier, every thread sums those in front of it and
 * writes its run.  Integer sums only: the result does not depend on the block's shape; no atomics. */
int emo_present_rows_i32(const int32_t* crop, const int32_t* paste, int F, int P, int32_t* count, int32_t* first, int32_t* row_of,
                         int32_t* crop_out, int32_t* paste_out, void* stream);
int emo_pack_rgb8(const float* img, uint8_t* out, int N, int H, int W, void* stream);
int emo_unpack_rgb8(const uint8_t* in, float* out, int N, int H, int W, void* stream);

/* ABI 15.  The inverse of the crop of emo_resize2d_windows_f32: the rendered S x S image of every frame goes back into that
 * frame's bytes, where its crop window was.  One launch per batch, frames updated IN PLACE inside the windows only: a byte
 * outside its frame's window is neither read nor written.
 *   img [N,3,S,S] fp32 (any range); matte [N,1,S,S] fp32 in [0,1] or NULL; windows N x (x0, y0, w, h) int32, DEVICE memory;
 *   windows_host the same N x 4 values in HOST memory, or NULL; frames [N,Hf,Wf,3] uint8; 0 <= feather <= 0.5.
 * Frame n, window (x0, y0, s, s), every pixel (y, x) with 0 <= y, x < s, every channel c:
 *   r   = clamp(R(img[n])[c, y, x], 0, 1) * 255, R = F.interpolate(size=(s, s), mode='bicubic', align_corners=False,
 *         antialias=(s < S)): for s >= S the arithmetic of emo_resize2d_f32 (A = -0.75); for s < S ATen's separable antialiased
 *         bicubic (A = -0.5, scale = S / s, taps within 2 * scale of scale * (i + 0.5), weights normalised by their sum)
 *   a   = clamp(min(d(y), d(x)) / (feather * s), 0, 1), d(i) = min(i + 0.5, s - (i + 0.5)); 1 where feather == 0; times the
 *         matte resized to (s, s) (bilinear, align_corners=False, no antialias: emo_resize2d_f32's) where one is given
 *   out = (uint8)((1 - a) * f + a * r), f the frame's byte: truncation, as emo_pack_rgb8.  In this form a == 1 gives
 *         emo_pack_rgb8's byte and a == 0 the frame's byte, exactly.
 * With windows_host, every window is checked before anything is launched: w or h <= 0 or a window that leaves the frame is
 * EMO_ERR_BAD_ARG, w != h or 4 * s < S (downscaling by more than 4) EMO_ERR_UNSUPPORTED, and the grid covers the largest side.
 * Without it (windows that only exist on the device) the grid covers min(Hf, Wf), and a frame whose device-side window fails
 * one of those checks is left untouched by the kernel: nothing is ever written outside a frame or outside a valid window. */
int emo_paste_windows_rgb8(const float* img, const float* matte, const int32_t* windows, const int32_t* windows_host,
                           uint8_t* frames, int N, int S, int Hf, int Wf, float feather, void* stream);

/* ABI 17.  NV12 video frames in and out, converted on the device.  A frame of height H and width W, both even, is H rows of Y
 * bytes and H / 2 rows of W / 2 interleaved (U, V) byte pairs.  Every entry point takes the pointer of the first frame's Y plane
 * and of its UV plane, the row pitch in bytes (>= W, shared by both planes) and the stride from one frame to the next in bytes
 * (shared too), which describes any placement of the planes a decoder uses; contiguous frames are uv = y + H * W, pitch = W,
 * frame_stride = 3 * H * W / 2.
 *   matrix 0 = bt709 (Kr, Kb) = (0.2126, 0.0722), 1 = bt601 (0.299, 0.114); Kg = 1 - Kr - Kb.
 *   full_range 0: oy = 16, sy = 219, sc = 224 (limited range); otherwise oy = 0, sy = 255, sc = 255.
 * Every coefficient derived from these is formed once in fp64 and rounded to fp32; the kernels' arithmetic is fp32, each
 * operation rounded on its own, summed in the order written.
 * D (bytes -> RGB in [0,1]); the chroma sample of luma pixel (y, x) is (y >> 1, x >> 1), plain replication:
 *   y' = (Y - oy) / sy, cb = (U - 128) / sc, cr = (V - 128) / sc
 *   R = y' + [2 (1 - Kr)] cr,  B = y' + [2 (1 - Kb)] cb,  G = (y' - [2 Kr (1 - Kr) / Kg] cr) - [2 Kb (1 - Kb) / Kg] cb,
 *   each clamped to [0,1].
 * E (fp32 image [3,H,W] -> bytes), on x = clamp(img, 0, 1):
 *   y' = (Kr R + Kg G) + Kb B,  Yc = oy + sy y',  Cbc = 128 + [sc / (2 (1 - Kb))] (B - y'),  Crc = 128 + [sc / (2 (1 - Kr))] (R - y')
 *   Y byte = floor(Yc + 0.5);  U byte (j, i) = floor((((Cbc[2j,2i] + Cbc[2j,2i+1]) + Cbc[2j+1,2i]) + Cbc[2j+1,2i+1]) * 0.25 + 0.5),
 *   V the same from Crc; every byte held to 0 ... 255.
 * All three refuse, before anything is launched, with EMO_ERR_BAD_ARG: a null pointer, an odd or non-positive H or W, pitch < W,
 * a negative frame stride, a matrix other than 0 or 1.
 *
 * emo_nv12_windows_f32 (C): out [N,3,Ho,Wo] fp32, frame n's window (x0, y0, w, h) of D(frame n) resized as
 *   clamp(F.interpolate(size=(Ho, Wo), mode='bicubic', align_corners=False), 0, 1) -- bit for bit what emo_resize2d_windows_f32
 *   (bicubic, clamp01) gives on the whole-frame D, without that fp32 frame: only the bytes under the window's taps are read.
 *   windows N x 4 int32 DEVICE memory, or NULL: every frame whole (with Ho x Wo = Hf x Wf that is D itself); windows_host the
 *   same values in HOST memory or NULL: a window that leaves the frame is then EMO_ERR_BAD_ARG before the launch.  A frame whose
 *   device-side window leaves the frame gets zeros.
 * emo_pack_nv12 (E): img [N,3,H,W] fp32 -> N frames.
 * emo_paste_windows_nv12 (P): emo_paste_windows_rgb8 on NV12 frames, in place; img, matte, windows, windows_host, S, feather and
 *   the window checks (square, inside the frame, 4 s >= S; nothing written on refusal) as there.  With r = the resized, clamped
 *   image in [0,1] (emo_paste_windows_rgb8's r before its * 255) and a its blend weight at a window pixel:
 *   Y <- floor(((1 - a) Y + a Yc(r)) + 0.5) at every luma pixel of the window;
 *   a chroma sample is touched if one of its four luma pixels lies in the window: a_i = a at those inside, 0 outside,
 *   am = (((a_00 + a_01) + a_10) + a_11) * 0.25,
 *   U <- floor(((1 - am) U + (((a_00 Cbc_00 + a_01 Cbc_01) + a_10 Cbc_10) + a_11 Cbc_11) * 0.25) + 0.5), V the same from Crc.
 *   a == 0 everywhere returns the frame's bytes and a == 1 (s == S, even x0 and y0) emo_pack_nv12's, exactly.  No byte outside
 *   the window's luma rectangle and its covering chroma rectangle is read or written, and every byte has one writer. */
int emo_nv12_windows_f32(const uint8_t* y, const uint8_t* uv, int64_t pitch, int64_t frame_stride, int Hf, int Wf,
                         const int32_t* windows, const int32_t* windows_host, float* out, int N, int Ho, int Wo, int matrix,
                         int full_range, void* stream);
int emo_pack_nv12(const float* img, uint8_t* y, uint8_t* uv, int64_t pitch, int64_t frame_stride, int N, int H, int W, int matrix,
                  int full_range, void* stream);
int emo_paste_windows_nv12(const float* img, const float* matte, const int32_t* windows, const int32_t* windows_host, uint8_t* y,
                           uint8_t* uv, int64_t pitch, int64_t frame_stride, int N, int S, int Hf, int Wf, float feather, int matrix,
                           int full_range, void* stream);

/* ABI 18.  Several faces per frame: M faces in F frames, face m lives in frame frame_of[m].  The crop and the paste entry points
 * above with the frame of a row looked up instead of being the row's own number.
 *   frame_of int32 [M], DEVICE memory, non-decreasing, every entry in [0, F) -- the faces of a frame are then the run of
 *   consecutive entries with its number, and their order in the list is the order they are pasted in; frame_of_host the same
 *   values in HOST memory; windows M x (x0, y0, w, h) int32 DEVICE memory and windows_host the same in HOST memory or NULL, as
 *   above.  x / y, uv / frames hold F frames; img, matte and out hold M rows.
 * Crops (emo_resize2d_faces_f32, emo_nv12_faces_f32): out[m] is bit for bit what emo_resize2d_windows_f32 / emo_nv12_windows_f32
 *   gives for a batch whose frame m is frame frame_of[m].  A face whose frame_of lies outside [0, F) gets zeros; for NV12 a face
 *   whose device-side window leaves the frame gets zeros too.
 * Paste (emo_paste_faces_rgb8, emo_paste_faces_nv12), in place and in ONE launch: the result is bit for bit that of pasting
 *   the M faces one after another, in list order, each with emo_paste_windows_rgb8 / emo_paste_windows_nv12 (N = 1) on its own
 *   frame -- the frame's bytes are rounded to bytes between two faces.  Overlapping windows of one frame are therefore well
 *   defined: the later face lies on top, blended by its own a.  No byte outside the union of the valid windows (NV12: and of
 *   their covering chroma rectangles) is read or written; every byte has exactly one writer, and no work item reads a byte
 *   another one writes: a pixel (NV12: a chroma sample with its four luma pixels) belongs to the last valid face of its frame
 *   that covers (touches) it, whose work item starts from the frame's bytes and applies every covering face of the run in list
 *   order, the value carried as a byte.  windows, frame_of, img and matte are only read.
 * Refusals, before anything is launched and with nothing written.  EMO_ERR_BAD_ARG: a null pointer (matte, windows_host and the
 *   crop's frame_of_host may be NULL), M < 0, F <= 0, a frame_of_host that decreases or leaves [0, F), a NULL frame_of_host for
 *   the paste entry points (the order of the paste rests on the list being sorted), a host-side window that leaves the frame
 *   (or has w or h <= 0), and what the single-window entry points refuse (feather, planes, matrix).  EMO_ERR_UNSUPPORTED: a
 *   host-side paste window with w != h or 4 * s < S.  M == 0 is EMO_OK and launches nothing.  A face whose window exists only on
 *   the device and is not a square inside the frame with 4 * s >= S, or whose device-side frame_of leaves [0, F), is treated as
 *   absent by the paste: it neither owns nor changes a byte. */
int emo_resize2d_faces_f32(const float* x, int64_t plane_stride, int64_t row_stride, const int32_t* windows, const int32_t* frame_of,
                           float* out, int M, int F, int C, int Ho, int Wo, int bicubic, int clamp01, void* stream);
int emo_nv12_faces_f32(const uint8_t* y, const uint8_t* uv, int64_t pitch, int64_t frame_stride, int Hf, int Wf,
                       const int32_t* windows, const int32_t* windows_host, const int32_t* frame_of, const int32_t* frame_of_host,
                       float* out, int M, int F, int Ho, int Wo, int matrix, int full_range, void* stream);
int emo_paste_faces_rgb8(const float* img, const float* matte, const int32_t* windows, const int32_t* windows_host,
                         const int32_t* frame_of, const int32_t* frame_of_host, uint8_t* frames, int M, int F, int S, int Hf, int Wf,
                         float feather, void* stream);
int emo_paste_faces_nv12(const float* img, const float* matte, const int32_t* windows, const int32_t* windows_host,
                         const int32_t* frame_of, const int32_t* frame_of_host, uint8_t* y, uint8_t* uv, int64_t pitch,
                         int64_t frame_stride, int M, int F, int S, int Hf, int Wf, float feather, int matrix, int full_range,
                         void* stream);

/* ABI 19.  The frames of a batch in DIFFERENT sizes (several video streams served by one batch): the four ABI 18 entry points
 * with the frames addressed through a frame table instead of (base, frame stride, Hf, Wf).
 *   table int64 [F,4], DEVICE memory, one row per frame: (byte address of the frame's first row, row pitch in bytes, H, W).
 *   rgb8: rows of W pixels of 3 bytes, pitch >= 3 W.  NV12: the address is the Y plane's, H and W are even, pitch >= W, and the
 *   UV plane starts at address + H * pitch (both planes share the pitch).  table_host: the same values in HOST memory.  Any
 *   address and any pitch are taken: nothing is assumed about their alignment.
 *   windows, windows_host, frame_of, frame_of_host, img, matte, out, S, feather, matrix, full_range: as for ABI 18.
 * The kernels only read the table.  A window is checked against ITS OWN frame's H and W, on the host (windows_host) and in the
 * kernel (always), with the predicates of ABI 18.
 * emo_rgb8_faces_ragged_f32: out[m] [3,Ho,Wo] is bit for bit emo_unpack_rgb8 (byte / 255) of frame frame_of[m] followed by
 *   emo_resize2d_faces_f32(bicubic = 1, clamp01 = 1) of window m -- every byte under a tap is converted where it is read, with
 *   the same arithmetic, and no full-frame fp32 picture is written.  A face whose frame_of lies outside [0, F), or whose
 *   device-side window is not inside its frame (w, h > 0), gets zeros.
 * emo_nv12_faces_ragged_f32: emo_nv12_faces_f32 with frame frame_of[m]'s own (address, pitch, H, W), the same arithmetic per
 *   output and the same zeros.
 * emo_paste_faces_ragged_rgb8, emo_paste_faces_ragged_nv12: emo_paste_faces_rgb8 / emo_paste_faces_nv12 with per-frame geometry,
 *   in place and in ONE launch: the faces of a frame in list order, the later one on top, every byte with one writer -- the
 *   bytes of pasting the faces one after another.  A face whose device-side window is not a square inside ITS frame with
 *   4 * s >= S, or whose frame_of leaves [0, F), is absent: it neither owns nor changes a byte.
 * Each result is therefore that of the ABI 18 entry point on a batch of uniform frames that holds every frame in its top-left
 *   corner (NV12: the Y rows at the top of the Y plane, the UV rows at the top of the UV plane), whatever the rest holds.
 * Refusals, before anything is launched and with nothing written.  EMO_ERR_BAD_ARG: a null pointer (matte and windows_host
 *   may be NULL; table_host and frame_of_host may not), M < 0, F <= 0, a table row with a null address, H or W <= 0 (NV12: or
 *   odd) or a pitch shorter than a row, a frame_of_host that decreases or leaves [0, F), a host-side window that leaves its
 *   frame (or has w or h <= 0), feather, matrix.  EMO_ERR_UNSUPPORTED: a host-side paste window with w != h or 4 * s < S;
 *   M > 65535 (one face per grid row).  M == 0 is EMO_OK and launches nothing. */
int emo_rgb8_faces_ragged_f32(const int64_t* table, const int64_t* table_host, const int32_t* windows, const int32_t* windows_host,
                              const int32_t* frame_of, const int32_t* frame_of_host, float* out, int M, int F, int Ho, int Wo,
                              void* stream);
int emo_nv12_faces_ragged_f32(const int64_t* table, const int64_t* table_host, const int32_t* windows, const int32_t* windows_host,
                              const int32_t* frame_of, const int32_t* frame_of_host, float* out, int M, int F, int Ho, int Wo,
                              int matrix, int full_range, void* stream);
int emo_paste_faces_ragged_rgb8(const float* img, const float* matte, const int64_t* table, const int64_t* table_host,
                                const int32_t* windows, const int32_t* windows_host, const int32_t* frame_of,
                                const int32_t* frame_of_host, int M, int F, int S, float feather, void* stream);
int emo_paste_faces_ragged_nv12(const float* img, const float* matte, const int64_t* table, const int64_t* table_host,
                                const int32_t* windows, const int32_t* windows_host, const int32_t* frame_of,
                                const int32_t* frame_of_host, int M, int F, int S, float feather, int matrix, int full_range,
                                void* stream);

/* ABI 22.  Planar and 10-bit YUV 4:2:0 frames: the NV12 operations of ABI 17 / 18 / 19 on four sample layouts of a frame of even
 * height H and even width W.
 *   layout 0  nv12       1-byte samples, chroma interleaved: H / 2 rows of W / 2 (U, V) pairs.            code = the byte
 *   layout 1  yuv420p    1-byte samples, a U plane and a V plane of H / 2 x W / 2 samples each.           code = the byte
 *   layout 2  p010       16-bit little-endian words, chroma interleaved (U, V) words.  code = word >> 6: the low 6 bits are
 *                        ignored on read and written as 0
 *   layout 3  yuv420p10  16-bit little-endian words, a U plane and a V plane.  code = word & 0x3FF: the high 6 bits are ignored
 *                        on read and written as 0
 * Every entry point takes the layout, the pointers of the first frame's Y, U and V planes (interleaved layouts: u is the chroma
 * plane and v is ignored), the row pitch of the luma plane and the one both chroma planes share, and the stride from one frame
 * to the next, which all planes share; pitches and the stride are in BYTES.
 * The definitions D, E, C and P are ABI 17's, word for word, with "code" for "byte":
 *   the chroma mid-point is 128 for 8-bit codes and 512 for 10-bit codes (where ABI 17 writes 128);
 *   8-bit codes: oy, sy, sc as in ABI 17.  10-bit codes: limited range oy = 64, sy = 876, sc = 896; full range oy = 0,
 *   sy = 1023, sc = 1023; every code is held to 0 ... 1023 (where ABI 17 writes 0 ... 255).
 * Unchanged: the matrices; coefficients formed once in fp64 and rounded to fp32; fp32 arithmetic, each operation rounded on its
 * own, in the order written; the chroma sample of luma pixel (y, x) is (y >> 1, x >> 1); the (1 - a) f + a r blends of P; every
 * sample has one writer; no sample outside a window's luma rectangle and its covering chroma rectangle is read or written.  A
 * sample that is written holds its code and zeros in the ignored bits; a sample that is not written keeps all its bits.
 * The limited-range 10-bit constants are 4 x the 8-bit ones, so a 10-bit frame of codes 4 * byte decodes (D, C) bit for bit to
 * what the 8-bit frame of those bytes does.
 *
 * emo_yuv420_crop_f32 (C): frame_of == NULL: row m is frame m, M >= 1 rows, F is not read, frame_of_host must be NULL and
 *   windows == NULL is every frame whole -- emo_nv12_windows_f32's form.  Otherwise face m lies in frame frame_of[m] of F --
 *   emo_nv12_faces_f32's form, with its windows, frame_of_host and M == 0 rules.
 * emo_pack_yuv420 (E): img [N,3,H,W] fp32 -> N frames.  Pairs of adjacent samples of an interleaved plane or a luma row go out
 *   as one store where the addresses, pitches and the stride are multiples of two samples.
 * emo_paste_yuv420 (P), in place: frame_of == NULL is emo_paste_windows_nv12's form (frame_of_host must be NULL), otherwise
 *   emo_paste_faces_nv12's, with its order and ownership rules.
 * emo_yuv420_crop_ragged_f32, emo_paste_ragged_yuv420: ABI 19's frame table [F,4] = (address, pitch, H, W).  Interleaved
 *   layouts: as NV12 there, the chroma plane at address + H * pitch with the same pitch.  Planar layouts: U at address +
 *   H * pitch with the chroma pitch pitch / 2, V at U + (H / 2) * (pitch / 2) -- a frame [3H/2, W] of dense rows.
 * Refusals, before anything is launched and with nothing written: everything ABI 17 / 18 / 19 refuses, with the same return
 *   codes and precedence; EMO_ERR_BAD_ARG also for an unknown layout, a NULL v of a planar layout, a pitch shorter than a row IN
 *   BYTES (luma: W samples; chroma: W samples interleaved, W / 2 planar), for 16-bit layouts an odd address, pitch or stride,
 *   and for planar rows of a frame table a pitch that is not a multiple of two samples.
 * The ten NV12 entry points of ABI 17 / 18 / 19 are layout 0 of these with pitch_y = pitch_c = pitch: the same floats and bytes. */
int emo_yuv420_crop_f32(int layout, const void* y, const void* u, const void* v, int64_t pitch_y, int64_t pitch_c, int64_t frame_stride,
                        int Hf, int Wf, const int32_t* windows, const int32_t* windows_host, const int32_t* frame_of,
                        const int32_t* frame_of_host, float* out, int M, int F, int Ho, int Wo, int matrix, int full_range, void* stream);
int emo_pack_yuv420(int layout, const float* img, void* y, void* u, void* v, int64_t pitch_y, int64_t pitch_c, int64_t frame_stride, int N,
                    int H, int W, int matrix, int full_range, void* stream);
int emo_paste_yuv420(int layout, const float* img, const float* matte, const int32_t* windows, const int32_t* windows_host,
                     const int32_t* frame_of, const int32_t* frame_of_host, void* y, void* u, void* v, int64_t pitch_y, int64_t pitch_c,
                     int64_t frame_stride, int M, int F, int S, int Hf, int Wf, float feather, int matrix, int full_range, void* stream);
int emo_yuv420_crop_ragged_f32(int layout, const int64_t* table, const int64_t* table_host, const int32_t* windows,
                               const int32_t* windows_host, const int32_t* frame_of, const int32_t* frame_of_host, float* out, int M,
                               int F, int Ho, int Wo, int matrix, int full_range, void* stream);
int emo_paste_ragged_yuv420(int layout, const float* img, const float* matte, const int64_t* table, const int64_t* table_host,
                            const int32_t* windows, const int32_t* windows_host, const int32_t* frame_of, const int32_t* frame_of_host,
                            int M, int F, int S, float feather, int matrix, int full_range, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMO_HIP_H_ */
