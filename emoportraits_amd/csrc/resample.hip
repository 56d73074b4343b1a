// Resampling + pointwise helpers of the hot path for gfx950 (all HBM-bound, one pass each).
//
//   emo_upsample_trilinear_f32  F.interpolate(x, scale_factor=(sd,sh,sw), mode='trilinear') with align_corners=False,
//                               scale factors 1 or 2 per axis: WarpGenerator.forward
//                               (networks/volumetric_avatar/warp_generator_resnet.py:163-166) and Unet3D.forward
//                               (unet_3d.py:223,269-272).
//   emo_avgpool_f32             nn.AvgPool3d / AvgPool2d with kernel == stride in 1..16 per axis (also the integer-window
//                               AdaptiveAvgPool2d of the embedders: identity_embedder.py:33, expression_embedder.py:394,408)
//                               (downsampling_layers['avgpool'(_3d)], utils.py:962-967; warp_generator_resnet.py:118,
//                               unet_3d.py:84-86,192-193, local_encoder.py via ResBlock stride 2).
//   emo_add_f32                 out = (a + b[i % period]) * alpha  (Unet3D skip sum unet_3d.py:281; embed mix va.py:857).
//   emo_add_rows_indexed_f32    out[b] = (a[b] + table[index[b]]) * alpha  (the same mix, one identity per row).
#include "common.h"

namespace {

// ATen area_pixel_compute_source_index(scale = 1/scale_factor, dst, align_corners=False, cubic=False):
//   src = scale * (dst + 0.5) - 0.5, clamped below at 0
__device__ __forceinline__ void lin_coeff(int o, int in_size, int factor, int& i0, int& i1, float& l0, float& l1) {
  if (factor == 1) { i0 = o; i1 = o; l0 = 1.0f; l1 = 0.0f; return; }
  float src = 0.5f * ((float)o + 0.5f) - 0.5f;
  src = src < 0.0f ? 0.0f : src;
  i0 = (int)src;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.0f - l1;
}

__global__ __launch_bounds__(256) void upsample_trilinear_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                  long NC, int D, int H, int W, int fd, int fh, int fw) {
  const int Do = D * fd, Ho = H * fh, Wo = W * fw;
  const long total = NC * Do * Ho * Wo;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int xo = (int)(i % Wo);
    long r = i / Wo;
    const int yo = (int)(r % Ho); r /= Ho;
    const int zo = (int)(r % Do);
    const long nc = r / Do;
    int z0, z1, y0, y1, x0, x1;
    float lz0, lz1, ly0, ly1, lx0, lx1;
    lin_coeff(zo, D, fd, z0, z1, lz0, lz1);
    lin_coeff(yo, H, fh, y0, y1, ly0, ly1);
    lin_coeff(xo, W, fw, x0, x1, lx0, lx1);
    const float* p = x + nc * (long)D * H * W;
    const long HW = (long)H * W;
    const float v000 = p[z0 * HW + y0 * W + x0], v001 = p[z0 * HW + y0 * W + x1];
    const float v010 = p[z0 * HW + y1 * W + x0], v011 = p[z0 * HW + y1 * W + x1];
    const float v100 = p[z1 * HW + y0 * W + x0], v101 = p[z1 * HW + y0 * W + x1];
    const float v110 = p[z1 * HW + y1 * W + x0], v111 = p[z1 * HW + y1 * W + x1];
    // ATen upsample_trilinear3d: t0 * (h0 * (w0 * v000 + w1 * v001) + h1 * (w0 * v010 + w1 * v011)) + t1 * (...)
    const float a = lz0 * (ly0 * (lx0 * v000 + lx1 * v001) + ly1 * (lx0 * v010 + lx1 * v011));
    const float b = lz1 * (ly0 * (lx0 * v100 + lx1 * v101) + ly1 * (lx0 * v110 + lx1 * v111));
    out[i] = a + b;
  }
}

// The same for a width factor of 2 and an even input width (every call of the driver pass).  The generic kernel spends three
// 64-bit divisions, eight 4-byte loads and a 4-byte store on every output and is bound by the CU's vector-memory instruction
// rate at a fifth of the HBM rate of its bytes.  Here one thread produces a BLOCK of outputs that share their inputs: four
// consecutive columns 4m .. 4m + 3 (input columns 2m - 1 .. 2m + 2) x the output rows 2k - 1, 2k (both interpolate the input
// rows k - 1, k; a factor-1 axis: one row) x the same pairing in depth -- up to 16 outputs from 16 loads (8 where the depth or
// the height factor is 1: both taps of that axis are the same row), written with four 16-byte stores.  Same coefficients and
// order of operations per output as the generic kernel (ATen's).
//   * First / last quad of a row: the input columns are clamped into the row, which IS the tap of the generic kernel there
//     (last column: x0 = x1 = W - 1); the first output of a row (source index clamped to 0: taps 0 and 1, weights 1 and 0) takes
//     its two values one register further right.  Round 4 sent those two quads of every row through the one-output-at-a-time
//     code -- 2 lanes in 16, so EVERY wave ran both paths, the second one with 128 scalar loads: 1.7 TB/s of the kernel's bytes.
//   * The first / last pair of an axis has one valid output (2k - 1 = -1, or 2k = 2 * in): its taps are used; two valid outputs
//     of a pair always share theirs (src = k - 0.75 and k - 0.25: both between the rows k - 1 and k).
//   * Work is laid out as runs of `cr` consecutive (sample, channel) volumes x `split` slices of a run's thread blocks
//     (grid = runs x split).  STATS: a run is a GroupNorm group (cr = C / G channels: one contiguous reduction domain of the
//     OUTPUT), and every block leaves the fp64 (sum, sum of squares) of the outputs it produced in partial[run][slice] -- the
//     layout gn_partial_kernel (groupnorm.hip) writes, so the norm in front of the next convolution needs no pass of its own
//     over the upsampled tensor (WarpGenerator: warp_generator_resnet.py:163-166 -> ResBlock3d's first norm).
constexpr int UPS_MAX_SPLIT = 64;         // == GN_MAX_SPLIT (groupnorm.hip): the partial-sum layout [run][64][2]

template <bool STATS>
__global__ __launch_bounds__(256) void upsample_trilinear_w2_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                     unsigned qrun, unsigned per, unsigned cr, int D, int H,
                                                                     int W, int fd, int fh, double* __restrict__ partial) {
  const int Do = D * fd, Ho = H * fh;
  const unsigned Wq = (unsigned)W >> 1;                      // quads per output row: 2 W / 4
  const unsigned Ky = fh == 2 ? H + 1 : H, Kz = fd == 2 ? D + 1 : D;   // pairs (2k - 1, 2k), k = 0 .. in; or single rows
  const long HW = (long)H * W;
  const unsigned run = blockIdx.x, sp = blockIdx.y;
  const unsigned lo = sp * per, hi = lo + per < qrun ? lo + per : qrun;
  double s_sum = 0.0, s_sq = 0.0;
  for (unsigned q = lo + threadIdx.x; q < hi; q += 256u) {
    const unsigned xq = q % Wq;
    unsigned r = q / Wq;
    const unsigned ky = r % Ky; r /= Ky;
    const unsigned kz = r % Kz;
    const long nc = (long)run * cr + r / Kz;
    // the (up to two) outputs of the pair along y and z: first = 2k - 1 (factor 2) or k (factor 1)
    const int ya = fh == 2 ? 2 * (int)ky - 1 : (int)ky, za = fd == 2 ? 2 * (int)kz - 1 : (int)kz;
    const int ny = fh == 2 ? 2 : 1, nz = fd == 2 ? 2 : 1;
    const float* p = x + nc * D * HW;
    float* const o = out + nc * Do * Ho * (2l * W) + 4 * xq;
    int yi0[2], yi1[2], zi0[2], zi1[2];
    float yl0[2], yl1[2], zl0[2], zl1[2];
    bool yv[2], zv[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int yo = ya + e, zo = za + e;
      yv[e] = e < ny && yo >= 0 && yo < Ho;
      zv[e] = e < nz && zo >= 0 && zo < Do;
      lin_coeff(yv[e] ? yo : 0, H, fh, yi0[e], yi1[e], yl0[e], yl1[e]);
      lin_coeff(zv[e] ? zo : 0, D, fd, zi0[e], zi1[e], zl0[e], zl1[e]);
    }
    const int xb = 2 * (int)xq - 1;
    const int ey = yv[0] ? 0 : 1, ez = zv[0] ? 0 : 1;         // (a pair has at least one valid output)
    int col[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int c = xb + k; col[k] = c < 0 ? 0 : (c > W - 1 ? W - 1 : c); }
    const float* r00 = p + zi0[ez] * HW + (long)yi0[ey] * W;
    float a00[4], a01[4], a10[4], a11[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a00[k] = r00[col[k]];
    if (fh == 2) {
      const float* r01 = p + zi0[ez] * HW + (long)yi1[ey] * W;
#pragma unroll
      for (int k = 0; k < 4; ++k) a01[k] = r01[col[k]];
    } else {
#pragma unroll
      // (factor 1 along y: the generic kernel / ATen form 1 * v[i0] + 0 * v[i1] with i1 = i0 + 1; here the second tap is a copy of
      // the first, i.e. v[i1] is never loaded.  Same bits for FINITE data; an Inf / NaN in v[i1] would propagate there (0 * Inf =
      // NaN) and does not here -- the "same bits as ATen" statement of this kernel holds for finite inputs, which is what a
      // GroupNorm'ed activation tensor is)
      for (int k = 0; k < 4; ++k) a01[k] = a00[k];
    }
    if (fd == 2) {
      const float* r10 = p + zi1[ez] * HW + (long)yi0[ey] * W;
#pragma unroll
      for (int k = 0; k < 4; ++k) a10[k] = r10[col[k]];
      if (fh == 2) {
        const float* r11 = p + zi1[ez] * HW + (long)yi1[ey] * W;
#pragma unroll
        for (int k = 0; k < 4; ++k) a11[k] = r11[col[k]];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) a11[k] = a10[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) { a10[k] = a00[k]; a11[k] = a01[k]; }
    }
    float lx0[4], lx1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int x0, x1;
      lin_coeff(4 * (int)xq + j, W, 2, x0, x1, lx0[j], lx1[j]);
    }
    // the first output of a row: taps (0, 1) = registers 1, 2 (register 0 holds the clamped column -1)
    const bool le = xq == 0;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (!(zv[c] && yv[e])) continue;
        float res[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int u = (j + 1) >> 1;
          float p00 = a00[u], q00 = a00[u + 1], p01 = a01[u], q01 = a01[u + 1];
          float p10 = a10[u], q10 = a10[u + 1], p11 = a11[u], q11 = a11[u + 1];
          if (j == 0) {
            p00 = le ? a00[1] : p00; q00 = le ? a00[2] : q00; p01 = le ? a01[1] : p01; q01 = le ? a01[2] : q01;
            p10 = le ? a10[1] : p10; q10 = le ? a10[2] : q10; p11 = le ? a11[1] : p11; q11 = le ? a11[2] : q11;
          }
          const float a = zl0[c] * (yl0[e] * (lx0[j] * p00 + lx1[j] * q00) + yl1[e] * (lx0[j] * p01 + lx1[j] * q01));
          const float b = zl1[c] * (yl0[e] * (lx0[j] * p10 + lx1[j] * q10) + yl1[e] * (lx0[j] * p11 + lx1[j] * q11));
          res[j] = a + b;
        }
        *reinterpret_cast<float4*>(o + ((long)(za + c) * Ho + (ya + e)) * (2l * W)) = make_float4(res[0], res[1], res[2], res[3]);
        if constexpr (STATS) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double v = (double)res[j];
            s_sum += v;
            s_sq += v * v;
          }
        }
      }
  }
  if constexpr (STATS) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s_sum += __shfl_down(s_sum, o, 64); s_sq += __shfl_down(s_sq, o, 64); }
    __shared__ double red[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = s_sum; red[1][wave] = s_sq; }
    __syncthreads();
    if (threadIdx.x == 0) {
      double* pp = partial + ((long)run * UPS_MAX_SPLIT + sp) * 2;
      pp[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
      pp[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
  }
}

// launch plan of the block kernel: runs x slices, a slice >= 2048 thread blocks of outputs where the run is that long
inline bool ups_w2_plan(long runs, long qrun, unsigned& split, unsigned& per) {
  if (runs < 1 || runs > 0x7fffffffL || qrun < 1 || qrun >= (1l << 31)) return false;
  long sp = (qrun + 2047) / 2048;
  sp = sp < 1 ? 1 : (sp > UPS_MAX_SPLIT ? UPS_MAX_SPLIT : sp);
  split = (unsigned)sp;
  per = (unsigned)((qrun + sp - 1) / sp);
  return true;
}

__global__ __launch_bounds__(256) void avgpool_kernel(const float* __restrict__ x, float* __restrict__ out, long NC,
                                                      int D, int H, int W, int kd, int kh, int kw) {
  const int Do = D / kd, Ho = H / kh, Wo = W / kw;
  const long total = NC * Do * Ho * Wo;
  const float inv = 1.0f / (float)(kd * kh * kw);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int xo = (int)(i % Wo);
    long r = i / Wo;
    const int yo = (int)(r % Ho); r /= Ho;
    const int zo = (int)(r % Do);
    const long nc = r / Do;
    const float* p = x + nc * (long)D * H * W;
    float s = 0.0f;
    for (int a = 0; a < kd; ++a)
      for (int b = 0; b < kh; ++b)
        for (int c = 0; c < kw; ++c) s += p[((long)(zo * kd + a) * H + (yo * kh + b)) * W + (xo * kw + c)];
    out[i] = s * inv;
  }
}

// The same for a window width of 1 or 2 on rows of whole quads (every call of the driver pass: the depth pooling (2, 1, 1) of the
// WarpGenerator's last block, 268 MB in, and the (1, 2, 2) / (2, 2, 2) poolings of the source pass): one thread produces four
// consecutive outputs from 16-byte loads and stores them with one 16-byte store, 32-bit index arithmetic.  The sum of an output
// runs over (depth, row, column) of its window in that order, as in the one-output-per-thread kernel: the same bits.
template <int KW>
__global__ __launch_bounds__(256) void avgpool_x4_kernel(const float* __restrict__ x, float* __restrict__ out, unsigned quads,
                                                         int D, int H, int W, int kd, int kh) {
  const unsigned Do = D / kd, Ho = H / kh, Wq = (unsigned)(W / KW) >> 2;
  const float inv = 1.0f / (float)(kd * kh * KW);
  const long vol = (long)D * H * W;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < quads; i += gridDim.x * 256u) {
    const unsigned xq = i % Wq;
    unsigned r = i / Wq;
    const unsigned yo = r % Ho; r /= Ho;
    const unsigned zo = r % Do;
    const unsigned nc = r / Do;
    const float* p = x + nc * vol + 4 * KW * xq;
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int a = 0; a < kd; ++a)
      for (int b = 0; b < kh; ++b) {
        const float4* row = reinterpret_cast<const float4*>(p + ((long)(zo * kd + a) * H + (yo * kh + b)) * W);
        const float4 v0 = row[0];
        if (KW == 1) {
          s[0] += v0.x; s[1] += v0.y; s[2] += v0.z; s[3] += v0.w;
        } else {
          const float4 v1 = row[1];
          s[0] += v0.x; s[0] += v0.y; s[1] += v0.z; s[1] += v0.w;
          s[2] += v1.x; s[2] += v1.y; s[3] += v1.z; s[3] += v1.w;
        }
      }
    reinterpret_cast<float4*>(out)[i] = make_float4(s[0] * inv, s[1] * inv, s[2] * inv, s[3] * inv);
  }
}


__global__ __launch_bounds__(256) void add_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                  float* __restrict__ out, long n, long period, float alpha) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    out[i] = (a[i] + b[i % period]) * alpha;
}

// out[b][i] = (a[b][i] + table[index[b]][i]) * alpha with add_kernel's roundings (separate add and multiply); grid (x, B).  The row
// index is uniform across a block: one load, kept in a scalar register.  An index outside [0, num_rows) writes a zero row.
__global__ __launch_bounds__(256) void add_rows_indexed_kernel(const float* __restrict__ a, const float* __restrict__ table,
                                                               const int* __restrict__ index, float* __restrict__ out,
                                                               long row, int num_rows, float alpha) {
  const int b = blockIdx.y;
  const int k = __builtin_amdgcn_readfirstlane(index[b]);
  const float* ap = a + (long)b * row;
  float* op = out + (long)b * row;
  if ((unsigned)k >= (unsigned)num_rows) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < row; i += (long)gridDim.x * 256) op[i] = 0.0f;
    return;
  }
  const float* tp = table + (long)k * row;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < row; i += (long)gridDim.x * 256)
    op[i] = (ap[i] + tp[i]) * alpha;
}

// F.interpolate(x, size=(Ho, Wo), mode='bilinear' | 'bicubic', align_corners=False) on 4-D tensors (ATen
// UpSampleBilinear2d / UpSampleBicubic2d: area_pixel_compute_source_index + cubic convolution, A = -0.75).
// Wrapper glue of the reference: bicubic resize of source / driver crops to image_size (notebooks/infer.py:399-401,
// :548-552), bilinear resize to output_size_s2 (notebooks/infer_s2.py:360-362).
// The two cubic-convolution polynomials in Horner form, every step one FMA.  The coefficients reach 8 |A| = 6 while the weights sum
// to 1, so each rounding of a step shows in the weight at up to 3e-07; with a product and a sum rounded apart the four weights of
// an axis came to 1 + 4.8e-07 (t = 2/3), on a one-pixel plane 1.8 x the error of ATen's CPU kernel
// (tests/test_op_launch_forms_gpu.py, `bicubic (1, 1) to (5, 3)`).  At t = 0 every step is exact: the weights are (0, 1, 0, 0).
__device__ __forceinline__ float cubic1(float x, float A) { return __fmaf_rn(__fmaf_rn(A + 2.0f, x, -(A + 3.0f)) * x, x, 1.0f); }
__device__ __forceinline__ float cubic2(float x, float A) {
  return __fmaf_rn(__fmaf_rn(__fmaf_rn(A, x, -5.0f * A), x, 8.0f * A), x, -4.0f * A);
}

// The bicubic sample at source index (sy, sx) of an H x W window, C channels at once: fraction, A = -0.75 weights and 4 x 4 taps
// clamped into the WINDOW, rows first.  tap(yy, xx, w, row) adds the C values of window pixel (yy, xx) times w to row -- a float
// load, an NV12 decode, a byte / 255 -- so every crop shares these sums and their order: row += tap * wx[b] over b, then
// acc += row * wy[a] over a.  acc is not clamped.
template <int C, class Tap>
__device__ __forceinline__ void bicubic_window(int H, int W, float sy, float sx, Tap tap, float acc[C]) {
  const float fy = floorf(sy), fx = floorf(sx);
  const int iy = (int)fy, ix = (int)fx;
  const float ty = sy - fy, tx = sx - fx;
  const float A = -0.75f;
  const float wy[4] = {cubic2(ty + 1.0f, A), cubic1(ty, A), cubic1(1.0f - ty, A), cubic2(2.0f - ty, A)};
  const float wx[4] = {cubic2(tx + 1.0f, A), cubic1(tx, A), cubic1(1.0f - tx, A), cubic2(2.0f - tx, A)};
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    int yy = iy - 1 + a;
    yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
    float row[C];
#pragma unroll
    for (int c = 0; c < C; ++c) row[c] = 0.0f;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      int xx = ix - 1 + b;
      xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
      tap(yy, xx, wx[b], row);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += row[c] * wy[a];
  }
}

// one output element of F.interpolate(size=(Ho, Wo), align_corners=False) from the H x W window at p (row stride in floats)
__device__ __forceinline__ float resize2d_at(const float* __restrict__ p, long row_stride, int H, int W, float sh, float sw,
                                             int yo, int xo, int bicubic, int clamp01) {
  float sy = sh * ((float)yo + 0.5f) - 0.5f, sx = sw * ((float)xo + 0.5f) - 0.5f;
  if (!bicubic) {
    sy = sy < 0.0f ? 0.0f : sy;
    sx = sx < 0.0f ? 0.0f : sx;
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float ly1 = sy - (float)y0, lx1 = sx - (float)x0, ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
    const float v = ly0 * (lx0 * p[y0 * row_stride + x0] + lx1 * p[y0 * row_stride + x1]) +
                    ly1 * (lx0 * p[y1 * row_stride + x0] + lx1 * p[y1 * row_stride + x1]);
    return clamp01 ? fminf(fmaxf(v, 0.0f), 1.0f) : v;
  }
  float acc[1];
  bicubic_window<1>(H, W, sy, sx, [&](int yy, int xx, float w, float row[1]) { row[0] += p[yy * row_stride + xx] * w; }, acc);
  return clamp01 ? fminf(fmaxf(acc[0], 0.0f), 1.0f) : acc[0];   // bicubic overshoots: crop_image clips (infer.py:350)
}

__global__ __launch_bounds__(256) void resize2d_kernel(const float* __restrict__ x, long plane_stride, long row_stride,
                                                       float* __restrict__ out, long NC,
                                                       int H, int W, int Ho, int Wo, int bicubic, int clamp01) {
  const long total = NC * Ho * Wo;
  const float sh = (float)H / (float)Ho, sw = (float)W / (float)Wo;   // scale = in/out when only `size` is given
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int xo = (int)(i % Wo);
    const long r = i / Wo;
    const int yo = (int)(r % Ho);
    const long nc = r / Ho;
    out[i] = resize2d_at(x + nc * plane_stride, row_stride, H, W, sh, sw, yo, xo, bicubic, clamp01);
  }
}

// ---- emo_paste_windows_rgb8 (ABI 15): the inverse of the window crop -- the rendered S x S image of every frame, resized to its
// window's side, feathered and blended into the frame's bytes in place (definition: include/emo_hip.h; kernel: paste_faces_kernel).

// what a window must satisfy to be pasted (the entry point refuses a host-side list that fails it; the kernel leaves the frame of
// a device-side window that fails it untouched): a square of side s inside the frame, downscaling by at most 4
__host__ __device__ inline bool paste_window_ok(int x0, int y0, int w, int h, int S, int Hf, int Wf) {
  return w > 0 && w == h && x0 >= 0 && y0 >= 0 && x0 <= Wf - w && y0 <= Hf - h && 4l * w >= S;
}

// ATen's antialiased bicubic filter (UpSampleKernel.cpp, _upsample_bicubic2d_aa: A = -0.5, support 2)
__device__ __forceinline__ float cubic_aa(float x) {
  x = fabsf(x);
  return x < 1.0f ? cubic1(x, -0.5f) : (x < 2.0f ? cubic2(x, -0.5f) : 0.0f);
}

// One output index of an antialiased axis S -> s (ATen _compute_indices_min_size_weights_aa, align_corners=False, scale = S / s
// >= 1): taps [lo, hi) around center = scale * (i + 0.5), tap j weighs cubic_aa((j - center + 0.5) / scale) / (their sum)
struct AaTaps { int lo, hi; float center, inv_total; };
__device__ __forceinline__ AaTaps aa_taps(int i, float scale, float inv_scale, int S) {
  AaTaps t;
  const float support = 2.0f * scale;
  t.center = scale * ((float)i + 0.5f);
  t.lo = (int)(t.center - support + 0.5f);
  t.lo = t.lo < 0 ? 0 : t.lo;
  t.hi = (int)(t.center + support + 0.5f);
  t.hi = t.hi > S ? S : t.hi;
  float total = 0.0f;
  for (int j = t.lo; j < t.hi; ++j) total += cubic_aa(((float)j - t.center + 0.5f) * inv_scale);
  t.inv_total = __fdiv_rn(1.0f, total);
  return t;
}

// r[c] = clamp(R(img)[c, y, x], 0, 1) of one window pixel; im = the frame's [3,S,S] image.  s >= S: resize2d_at's bicubic;
// s < S: the antialiased one, rows first (ATen resamples the width, then the height), ty = the taps of row y.  The weights are
// evaluated where they are used (up to 17 x 17 taps at scale 4: no register arrays with run-time indices, i.e. no scratch).
__device__ __forceinline__ void paste_render01(const float* __restrict__ im, int S, int s, float scale, float inv_scale,
                                               const AaTaps& ty, int y, int x, float r[3]) {
  const long SS = (long)S * S;
  if (s >= S) {
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = resize2d_at(im + c * SS, S, S, S, scale, scale, y, x, 1, 1);
    return;
  }
  const AaTaps tx = aa_taps(x, scale, inv_scale, S);
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (int yy = ty.lo; yy < ty.hi; ++yy) {
    const float wy = cubic_aa(((float)yy - ty.center + 0.5f) * inv_scale) * ty.inv_total;
    const float* p = im + (long)yy * S;
    float row[3] = {0.0f, 0.0f, 0.0f};
    for (int xx = tx.lo; xx < tx.hi; ++xx) {
      const float wx = cubic_aa(((float)xx - tx.center + 0.5f) * inv_scale) * tx.inv_total;
#pragma unroll
      for (int c = 0; c < 3; ++c) row[c] += wx * p[c * SS + xx];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += wy * row[c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) r[c] = fminf(fmaxf(acc[c], 0.0f), 1.0f);
}

// the same times 255: what the rgb8 paste blends with the frame's bytes
__device__ __forceinline__ void paste_render(const float* __restrict__ im, int S, int s, float scale, float inv_scale,
                                             const AaTaps& ty, int y, int x, float r[3]) {
  paste_render01(im, S, s, scale, inv_scale, ty, y, x, r);
#pragma unroll
  for (int c = 0; c < 3; ++c) r[c] *= 255.0f;
}

// the blend weight of window pixel (y, x): the feather ramp from the window's edge (fs = feather * s; 1 where feather == 0) times
// the matte resized to the window (bilinear, no antialias)
__device__ __forceinline__ float paste_alpha(const float* __restrict__ mt, int S, int s, float scale, float feather, float fs,
                                             int y, int x) {
  float a = 1.0f;
  if (feather > 0.0f) {
    const float cy = (float)y + 0.5f, cx = (float)x + 0.5f;
    const float d = fminf(fminf(cy, (float)s - cy), fminf(cx, (float)s - cx));
    a = fminf(fmaxf(__fdiv_rn(d, fs), 0.0f), 1.0f);
  }
  if (mt) a = fminf(fmaxf(a * resize2d_at(mt, S, S, S, scale, scale, y, x, 0, 0), 0.0f), 1.0f);   // (a matte outside [0,1]: clipped)
  return a;
}

// (1 - a) f + a r, truncated like pack_rgb8_kernel: a == 1 gives pack_rgb8's byte, a == 0 the frame's, both exactly
__device__ __forceinline__ unsigned paste_blend(float a, unsigned f, float r) { return (unsigned)(uint8_t)((1.0f - a) * (float)f + a * r); }

// ---- YUV 4:2:0 frames (ABI 17 and 22; the definitions D, E, C and P: include/emo_hip.h).  A frame is Hf rows of Y samples and
// Hf / 2 rows of chroma: Wf / 2 interleaved (U, V) pairs, or a U plane and a V plane of Wf / 2 samples a row.  Pitches and the
// frame stride are in bytes; the chroma planes share their pitch and every plane the frame stride.

// A sample layout: the sample's type, where the chroma lies, and where the code sits in the sample.  Together with yuv_decode_at,
// yuv_encode, yuv_code and yuv_store / yuv_store2 below it is all that knows where a sample lies and how wide it is.
template <class T, bool PLANAR, int BITS, int SHIFT>
struct YuvLayout {
  using sample = T;
  static constexpr bool planar = PLANAR;
  static constexpr int bits = BITS, shift = SHIFT;
  static constexpr unsigned max_code = (1u << BITS) - 1u;
  static constexpr float mid = (float)(1u << (BITS - 1)), top = (float)max_code;
  // the code of a sample: the bits outside it are ignored
  static __host__ __device__ __forceinline__ unsigned code(T w) {
    if constexpr (sizeof(T) == 1) return w;
    else return ((unsigned)w >> SHIFT) & max_code;
  }
  // the sample of a code: the bits outside it are zero
  static __host__ __device__ __forceinline__ T word(unsigned c) { return (T)(c << SHIFT); }
};
using Nv12 = YuvLayout<uint8_t, false, 8, 0>;          // layout 0
using Yuv420p = YuvLayout<uint8_t, true, 8, 0>;        // layout 1
using P010 = YuvLayout<uint16_t, false, 10, 6>;        // layout 2: the code in the high ten bits
using Yuv420p10 = YuvLayout<uint16_t, true, 10, 0>;    // layout 3: the code in the low ten bits

// fn(layout trait) of layout id 0 ... 3, or EMO_ERR_BAD_ARG
template <class Fn>
inline int with_layout(int layout, Fn fn) {
  switch (layout) {
    case 0: return fn(Nv12{});
    case 1: return fn(Yuv420p{});
    case 2: return fn(P010{});
    case 3: return fn(Yuv420p10{});
    default: return EMO_ERR_BAD_ARG;
  }
}

// Everything derived from the matrix (Kr, Kb), the range and the code width is formed once on the host in fp64 and rounded to fp32
struct Nv12Coef {
  float oy, sy, sc;          // luma offset; luma and chroma code ranges
  float kr, kg, kb;          // y' = kr R + kg G + kb B
  float rv, bu, gv, gu;      // decode: R = y' + rv cr, B = y' + bu cb, G = y' - gv cr - gu cb
  float cbs, crs;            // encode: Cbc = mid + cbs (B - y'), Crc = mid + crs (R - y')
};

inline bool nv12_coef(int matrix, int full_range, int bits, Nv12Coef& k) {
  double Kr, Kb;
  if (matrix == 0) { Kr = 0.2126; Kb = 0.0722; }            // bt709
  else if (matrix == 1) { Kr = 0.299; Kb = 0.114; }         // bt601
  else return false;
  const double Kg = 1.0 - Kr - Kb;
  const double ten = bits == 10 ? 4.0 : 1.0;                // limited range: the 10-bit constants are 4 x the 8-bit ones
  const double top = bits == 10 ? 1023.0 : 255.0;
  const double oy = full_range ? 0.0 : 16.0 * ten, sy = full_range ? top : 219.0 * ten, sc = full_range ? top : 224.0 * ten;
  k.oy = (float)oy; k.sy = (float)sy; k.sc = (float)sc;
  k.kr = (float)Kr; k.kg = (float)Kg; k.kb = (float)Kb;
  k.rv = (float)(2.0 * (1.0 - Kr)); k.bu = (float)(2.0 * (1.0 - Kb));
  k.gv = (float)(2.0 * Kr * (1.0 - Kr) / Kg); k.gu = (float)(2.0 * Kb * (1.0 - Kb) / Kg);
  k.cbs = (float)(sc / (2.0 * (1.0 - Kb))); k.crs = (float)(sc / (2.0 * (1.0 - Kr)));
  return true;
}

// what every entry point refuses before a launch: null planes (planar: v too), an odd frame, a pitch shorter than a row in
// bytes, and for 16-bit samples an odd address, pitch or stride
template <class L>
inline bool yuv_planes_ok(const void* y, const void* u, const void* v, int64_t pitch_y, int64_t pitch_c, int64_t frame_stride, int H,
                          int W) {
  constexpr int64_t B = sizeof(typename L::sample);
  if (!y || !u || (L::planar && !v) || H <= 0 || W <= 0 || (H & 1) || (W & 1) || frame_stride < 0) return false;
  if (pitch_y < W * B || pitch_c < (L::planar ? W / 2 : W) * B) return false;
  if (B == 2 && ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(u) | (L::planar ? reinterpret_cast<uintptr_t>(v) : 0) |
                  (uintptr_t)pitch_y | (uintptr_t)pitch_c | (uintptr_t)frame_stride) & 1)) return false;
  return true;
}

// may two adjacent samples go out as one store of twice the width: the luma planes' (and, interleaved, the chroma plane's)
// addresses, pitches and the frame stride are multiples of two samples
template <class L>
inline bool yuv_pairs(const void* y, const void* u, int64_t pitch_y, int64_t pitch_c, int64_t frame_stride) {
  uintptr_t all = reinterpret_cast<uintptr_t>(y) | (uintptr_t)pitch_y | (uintptr_t)frame_stride;
  if (!L::planar) all |= reinterpret_cast<uintptr_t>(u) | (uintptr_t)pitch_c;
  return (all & (2 * sizeof(typename L::sample) - 1)) == 0;
}

__host__ __device__ inline bool nv12_window_ok(int x0, int y0, int w, int h, int Hf, int Wf) {
  return w > 0 && h > 0 && x0 >= 0 && y0 >= 0 && x0 <= Wf - w && y0 <= Hf - h;
}

// the planes of one frame and their pitches in bytes (interleaved: v is not used)
struct YuvFrame { uint8_t* y; uint8_t* u; uint8_t* v; long pitch_y, pitch_c; };

template <class L>
__device__ __forceinline__ typename L::sample* yuv_row(uint8_t* plane, long row, long pitch) {
  return reinterpret_cast<typename L::sample*>(plane + row * pitch);
}

// D of frame pixel (y, x): its Y code and the chroma codes at (y >> 1, x >> 1) -> clamped R, G, B; converted once for all three
template <class L>
__device__ __forceinline__ void yuv_decode_at(const YuvFrame& f, const Nv12Coef& k, int y, int x, float rgb[3]) {
  unsigned cu, cv;
  if constexpr (L::planar) {
    cu = L::code(yuv_row<L>(f.u, y >> 1, f.pitch_c)[x >> 1]);
    cv = L::code(yuv_row<L>(f.v, y >> 1, f.pitch_c)[x >> 1]);
  } else {
    const typename L::sample* const c = yuv_row<L>(f.u, y >> 1, f.pitch_c) + (x & ~1);
    cu = L::code(c[0]);
    cv = L::code(c[1]);
  }
  const float yp = __fdiv_rn((float)L::code(yuv_row<L>(f.y, y, f.pitch_y)[x]) - k.oy, k.sy);
  const float cb = __fdiv_rn((float)cu - L::mid, k.sc), cr = __fdiv_rn((float)cv - L::mid, k.sc);
  const float r = yp + k.rv * cr, b = yp + k.bu * cb, g = (yp - k.gv * cr) - k.gu * cb;
  rgb[0] = fminf(fmaxf(r, 0.0f), 1.0f);
  rgb[1] = fminf(fmaxf(g, 0.0f), 1.0f);
  rgb[2] = fminf(fmaxf(b, 0.0f), 1.0f);
}

// E of one pixel before the rounding: the luma code and the two chroma codes of clamp(rgb, 0, 1)
template <class L>
__device__ __forceinline__ void yuv_encode(const Nv12Coef& k, const float rgb[3], float& yc, float& cbc, float& crc) {
  const float r = fminf(fmaxf(rgb[0], 0.0f), 1.0f), g = fminf(fmaxf(rgb[1], 0.0f), 1.0f), b = fminf(fmaxf(rgb[2], 0.0f), 1.0f);
  const float yp = (k.kr * r + k.kg * g) + k.kb * b;
  yc = k.oy + k.sy * yp;
  cbc = L::mid + k.cbs * (b - yp);
  crc = L::mid + k.crs * (r - yp);
}

// floor(v) held to 0 ... 255 (10 bits: 1023); the callers add the 0.5
template <class L>
__device__ __forceinline__ unsigned yuv_code(float v) { return (unsigned)fminf(fmaxf(floorf(v), 0.0f), L::top); }

// two adjacent samples: one store of twice the width where the planes allow it (`pairs`: yuv_pairs)
template <class L>
__device__ __forceinline__ void yuv_store2(typename L::sample* p, unsigned lo, unsigned hi, bool pairs) {
  if constexpr (sizeof(typename L::sample) == 1) {
    if (pairs) *reinterpret_cast<uint16_t*>(p) = (uint16_t)(lo | (hi << 8));
    else { p[0] = (uint8_t)lo; p[1] = (uint8_t)hi; }
  } else {
    if (pairs) *reinterpret_cast<uint32_t*>(p) = (uint32_t)L::word(lo) | ((uint32_t)L::word(hi) << 16);
    else { p[0] = L::word(lo); p[1] = L::word(hi); }
  }
}

// the chroma codes of sample (cy, cx): a pair of the interleaved plane, or one sample of each plane (neighbouring lanes hold
// neighbouring samples)
template <class L>
__device__ __forceinline__ void yuv_store_chroma(const YuvFrame& f, int cy, int cx, unsigned u, unsigned v, bool pairs) {
  if constexpr (L::planar) {
    yuv_row<L>(f.u, cy, f.pitch_c)[cx] = L::word(u);
    yuv_row<L>(f.v, cy, f.pitch_c)[cx] = L::word(v);
  } else {
    yuv_store2<L>(yuv_row<L>(f.u, cy, f.pitch_c) + 2 * cx, u, v, pairs);
  }
}

// emo_pack_nv12 / emo_pack_yuv420: one work item per 2 x 2 luma block -- its four Y samples and its (U, V) have no other writer
template <class L>
__global__ __launch_bounds__(256) void pack_yuv420_kernel(const float* __restrict__ img, YuvFrame f0, long fstride, long N, int H,
                                                          int W, bool pairs, Nv12Coef k) {
  const int Hc = H >> 1, Wc = W >> 1;
  const long HW = (long)H * W, total = N * Hc * Wc;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int cx = (int)(i % Wc);
    const long r = i / Wc;
    const int cy = (int)(r % Hc);
    const long n = r / Hc;
    const YuvFrame f = {f0.y + n * fstride, f0.u + n * fstride, L::planar ? f0.v + n * fstride : nullptr, f0.pitch_y, f0.pitch_c};
    const float* const src = img + n * 3 * HW + (long)(2 * cy) * W + 2 * cx;
    float cb = 0.0f, cr = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      unsigned yb[2];
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const float rgb[3] = {src[dy * W + dx], src[HW + dy * W + dx], src[2 * HW + dy * W + dx]};
        float yc, cbc, crc;
        yuv_encode<L>(k, rgb, yc, cbc, crc);
        yb[dx] = yuv_code<L>(yc + 0.5f);
        cb += cbc;                               // ((c00 + c01) + c10) + c11 (0 + c00 is c00)
        cr += crc;
      }
      yuv_store2<L>(yuv_row<L>(f.y, 2 * cy + dy, f.pitch_y) + 2 * cx, yb[0], yb[1], pairs);
    }
    yuv_store_chroma<L>(f, cy, cx, yuv_code<L>(cb * 0.25f + 0.5f), yuv_code<L>(cr * 0.25f + 0.5f), pairs);
  }
}

// stage-2 glue (notebooks/infer_s2.py:365-375)
__global__ __launch_bounds__(256) void mul_mask_kernel(const float* __restrict__ img, const float* __restrict__ mask,
                                                       float* __restrict__ out, long N, int C, long HW) {
  const long total = N * C * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long p = i % HW;
    const long n = i / (HW * C);
    out[i] = img[i] * mask[n * HW + p];
  }
}

__global__ __launch_bounds__(256) void stage2_compose_kernel(const float* __restrict__ img, const float* __restrict__ add,
                                                             const float* __restrict__ mask,
                                                             const float* __restrict__ face_mask,
                                                             float* __restrict__ out, long N, int C, long HW) {
  const long total = N * C * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long p = i % HW;
    const long n = i / (HW * C);
    const float m = mask[n * HW + p] * face_mask[n * HW + p];
    float v = img[i] + add[i] * m;
    v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    out[i] = v;
  }
}

inline int grid_for(long total) {
  long g = (total + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// ---- The launch forms of the two launchers that have more than one (ABI 28): each decided by ONE host function, which its
// launcher calls and emo_op_launch_form reports.  rc: what the launcher returns before any launch (EMO_OK: it launches `form`).

// emo_upsample_trilinear_f32 (stats = false) and emo_upsample_trilinear_gn_sums_f32 (stats = true: the run is the GroupNorm group,
// cr = the channels of a group, and there is no generic form to fall back to).  grid = runs x split blocks; items = the thread
// blocks of outputs (block kernel) or the outputs (generic kernel) of the launch
struct UpsForm { int rc, form; long cr, runs, qrun, items; unsigned split, per; long grid; };

inline UpsForm ups_form(const void* x, const void* out, long NC, int D, int H, int W, int fd, int fh, int fw) {
  UpsForm f = {EMO_OK, EMO_UPSAMPLE_FORM_GENERIC, 1, 0, 0, 0, 1, 0, 0};
  if (!x || !out || NC <= 0 || D <= 0 || H <= 0 || W <= 0) { f.rc = EMO_ERR_BAD_ARG; return f; }
  if ((fd != 1 && fd != 2) || (fh != 1 && fh != 2) || (fw != 1 && fw != 2)) { f.rc = EMO_ERR_UNSUPPORTED; return f; }
  const long qvol = (long)(fd == 2 ? D + 1 : D) * (fh == 2 ? H + 1 : H) * (W / 2);      // thread blocks of outputs per volume
  long cr = 1;                                                                         // volumes per run: small ones in groups
  while (qvol * cr < 2048 && NC % (2 * cr) == 0) cr *= 2;
  unsigned split, per;
  if (fw == 2 && (W & 1) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && ups_w2_plan(NC / cr, qvol * cr, split, per)) {
    f.form = EMO_UPSAMPLE_FORM_BLOCK;
    f.cr = cr; f.runs = NC / cr; f.qrun = qvol * cr; f.split = split; f.per = per;
    f.items = f.qrun * f.runs; f.grid = f.runs * split;
    return f;
  }
  f.items = NC * D * fd * H * fh * W * fw;
  f.grid = grid_for(f.items);
  return f;
}

inline UpsForm ups_gn_form(const void* x, const void* out, const void* partial, int64_t partial_bytes, const void* split_out, int N,
                           int C, int G, int D, int H, int W, int fd, int fh, int fw) {
  UpsForm f = {EMO_OK, EMO_UPSAMPLE_FORM_BLOCK, 1, 0, 0, 0, 1, 0, 0};
  if (!x || !out || !partial || !split_out || N <= 0 || C <= 0 || G <= 0 || C % G || D <= 0 || H <= 0 || W <= 0) { f.rc = EMO_ERR_BAD_ARG; return f; }
  if ((fd != 1 && fd != 2) || (fh != 1 && fh != 2) || fw != 2 || (W & 1)) { f.rc = EMO_ERR_UNSUPPORTED; return f; }
  if ((reinterpret_cast<uintptr_t>(out) & 15) != 0) { f.rc = EMO_ERR_UNSUPPORTED; return f; }
  if (partial_bytes < (int64_t)N * G * UPS_MAX_SPLIT * 2 * (int64_t)sizeof(double)) { f.rc = EMO_ERR_BAD_ARG; return f; }
  f.cr = C / G;
  f.runs = (long)N * G;
  f.qrun = f.cr * (fd == 2 ? D + 1 : D) * (fh == 2 ? H + 1 : H) * (W / 2);
  if (!ups_w2_plan(f.runs, f.qrun, f.split, f.per)) { f.rc = EMO_ERR_UNSUPPORTED; return f; }
  f.items = f.qrun * f.runs; f.grid = f.runs * f.split;
  return f;
}

// emo_avgpool_f32: items = the quads of outputs (x4 kernels) or the outputs (generic kernel); grid blocks of 256 threads
struct PoolForm { int rc, form; long items, grid; };

inline PoolForm pool_form(const void* x, const void* out, long NC, int D, int H, int W, int kd, int kh, int kw) {
  PoolForm f = {EMO_OK, EMO_AVGPOOL_FORM_GENERIC, 0, 0};
  if (!x || !out || NC <= 0 || D <= 0 || H <= 0 || W <= 0) { f.rc = EMO_ERR_BAD_ARG; return f; }
  if (kd < 1 || kh < 1 || kw < 1 || kd > 16 || kh > 16 || kw > 16) { f.rc = EMO_ERR_UNSUPPORTED; return f; }
  if (D % kd || H % kh || W % kw) { f.rc = EMO_ERR_UNSUPPORTED; return f; }
  const long total = NC * (D / kd) * (H / kh) * (W / kw);
  if ((kw == 1 || kw == 2) && W % (4 * kw) == 0 && total / 4 < (1l << 32) &&
      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) {
    f.form = kw == 1 ? EMO_AVGPOOL_FORM_X4_W1 : EMO_AVGPOOL_FORM_X4_W2;
    f.items = total / 4;
  } else {
    f.items = total;
  }
  f.grid = grid_for(f.items);
  return f;
}

}  // namespace

extern "C" int emo_upsample_trilinear_f32(const float* x, float* out, int64_t NC, int D, int H, int W, int fd, int fh,
                                          int fw, void* stream) {
  const UpsForm f = ups_form(x, out, NC, D, H, W, fd, fh, fw);
  if (f.rc != EMO_OK) return f.rc;
  if (f.form == EMO_UPSAMPLE_FORM_BLOCK) {
    hipLaunchKernelGGL(upsample_trilinear_w2_kernel<false>, dim3((unsigned)f.runs, f.split), dim3(256), 0, (hipStream_t)stream,
                       x, out, (unsigned)f.qrun, f.per, (unsigned)f.cr, D, H, W, fd, fh, (double*)nullptr);
    return emo_launch_status();
  }
  hipLaunchKernelGGL(upsample_trilinear_kernel, dim3((unsigned)f.grid), dim3(256), 0, (hipStream_t)stream, x, out,
                     (long)NC, D, H, W, fd, fh, fw);
  return emo_launch_status();
}

// The upsampling with the GroupNorm statistics of its OUTPUT reduced on the way: out as emo_upsample_trilinear_f32, and in
// `partial` ([N * G][64][2] doubles: emo_groupnorm_workspace_bytes(N, G)) the (sum, sum of squares) slices of every (sample,
// group) in the layout emo_groupnorm_affine_from_sums_f32 (groupnorm.hip) finishes; *split_out = the slices written per group.
// Width factor 2, an even input width and a 16-byte aligned output only (EMO_ERR_UNSUPPORTED otherwise: the caller runs the
// two operations one after the other).
extern "C" int emo_upsample_trilinear_gn_sums_f32(const float* x, float* out, int N, int C, int G, int D, int H, int W, int fd,
                                                  int fh, int fw, void* partial, int64_t partial_bytes, int* split_out,
                                                  void* stream) {
  const UpsForm f = ups_gn_form(x, out, partial, partial_bytes, split_out, N, C, G, D, H, W, fd, fh, fw);
  if (f.rc != EMO_OK) return f.rc;
  hipLaunchKernelGGL(upsample_trilinear_w2_kernel<true>, dim3((unsigned)f.runs, f.split), dim3(256), 0, (hipStream_t)stream, x, out,
                     (unsigned)f.qrun, f.per, (unsigned)f.cr, D, H, W, fd, fh, reinterpret_cast<double*>(partial));
  *split_out = (int)f.split;
  return emo_launch_status();
}

extern "C" int emo_avgpool_f32(const float* x, float* out, int64_t NC, int D, int H, int W, int kd, int kh, int kw,
                               void* stream) {
  const PoolForm f = pool_form(x, out, NC, D, H, W, kd, kh, kw);
  if (f.rc != EMO_OK) return f.rc;
  const dim3 grid((unsigned)f.grid);
  if (f.form == EMO_AVGPOOL_FORM_X4_W1)
    hipLaunchKernelGGL(avgpool_x4_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, out, (unsigned)f.items, D, H, W, kd, kh);
  else if (f.form == EMO_AVGPOOL_FORM_X4_W2)
    hipLaunchKernelGGL(avgpool_x4_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, x, out, (unsigned)f.items, D, H, W, kd, kh);
  else
    hipLaunchKernelGGL(avgpool_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, out, (long)NC, D, H, W, kd, kh, kw);
  return emo_launch_status();
}

// ABI 28 (definition: include/emo_hip.h): the form and plan the launcher of `op` takes for these arguments; nothing is launched
extern "C" int emo_op_launch_form(int op, const void* x, const void* out, const int64_t* dims, int64_t* plan) {
  if (!dims || !plan) return EMO_ERR_BAD_ARG;
  for (int i = 0; i < EMO_OP_PLAN_COUNT; ++i) plan[i] = 0;
  const auto i32 = [&](int i) { return (int)dims[i]; };
  // an int argument of the launcher that does not fit one: dims[first .. last]
  const auto ints = [&](int first, int last) {
    for (int i = first; i <= last; ++i)
      if (dims[i] != (int64_t)(int)dims[i]) return false;
    return true;
  };
  if (op == EMO_OP_UPSAMPLE_TRILINEAR || op == EMO_OP_UPSAMPLE_TRILINEAR_GN_SUMS) {
    UpsForm f;
    if (op == EMO_OP_UPSAMPLE_TRILINEAR) {
      if (!ints(1, 6)) return EMO_ERR_BAD_ARG;
      f = ups_form(x, out, (long)dims[0], i32(1), i32(2), i32(3), i32(4), i32(5), i32(6));
    } else {
      if (!ints(0, 8)) return EMO_ERR_BAD_ARG;
      // (the workspace and split_out of the launcher: any non-null address, a size that is enough)
      f = ups_gn_form(x, out, plan, INT64_MAX, plan, i32(0), i32(1), i32(2), i32(3), i32(4), i32(5), i32(6), i32(7), i32(8));
    }
    if (f.rc != EMO_OK) return f.rc;
    plan[EMO_OP_PLAN_FORM] = f.form; plan[EMO_OP_PLAN_GRID] = f.grid; plan[EMO_OP_PLAN_ITEMS] = f.items;
    if (f.form == EMO_UPSAMPLE_FORM_BLOCK) {
      plan[EMO_OP_PLAN_CR] = f.cr; plan[EMO_OP_PLAN_RUNS] = f.runs; plan[EMO_OP_PLAN_SPLIT] = f.split;
      plan[EMO_OP_PLAN_PER] = f.per; plan[EMO_OP_PLAN_RUN_ITEMS] = f.qrun;
    }
    return EMO_OK;
  }
  if (op == EMO_OP_AVGPOOL) {
    if (!ints(1, 6)) return EMO_ERR_BAD_ARG;
    const PoolForm f = pool_form(x, out, (long)dims[0], i32(1), i32(2), i32(3), i32(4), i32(5), i32(6));
    if (f.rc != EMO_OK) return f.rc;
    plan[EMO_OP_PLAN_FORM] = f.form; plan[EMO_OP_PLAN_GRID] = f.grid; plan[EMO_OP_PLAN_ITEMS] = f.items;
    return EMO_OK;
  }
  if (op == EMO_OP_GROUPNORM_AFFINE) return emo_groupnorm_launch_plan(x, dims, plan);
  return EMO_ERR_BAD_ARG;
}

extern "C" int emo_add_f32(const float* a, const float* b, float* out, int64_t n, int64_t period, float alpha,
                           void* stream) {
  if (!a || !b || !out || n <= 0 || period <= 0) return EMO_ERR_BAD_ARG;
  hipLaunchKernelGGL(add_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, a, b, out, (long)n,
                     (long)period, alpha);
  return emo_launch_status();
}

extern "C" int emo_add_rows_indexed_f32(const float* a, const float* table, const int32_t* index, float* out, int B, int num_rows,
                                        int64_t row, float alpha, void* stream) {
  if (!a || !table || !index || !out || B <= 0 || num_rows <= 0 || row <= 0) return EMO_ERR_BAD_ARG;
  if (B > 65535) return EMO_ERR_UNSUPPORTED;
  const unsigned gx = (unsigned)(row < 256L * 64 ? emo_cdiv(row, 256) : 64);
  hipLaunchKernelGGL(add_rows_indexed_kernel, dim3(gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, a, table, index, out,
                     (long)row, num_rows, alpha);
  return emo_launch_status();
}

extern "C" int emo_mul_mask_f32(const float* img, const float* mask, float* out, int N, int C, int64_t HW, void* stream) {
  if (!img || !mask || !out || N <= 0 || C <= 0 || HW <= 0) return EMO_ERR_BAD_ARG;
  hipLaunchKernelGGL(mul_mask_kernel, dim3(grid_for((long)N * C * HW)), dim3(256), 0, (hipStream_t)stream, img, mask, out,
                     (long)N, C, (long)HW);
  return emo_launch_status();
}

extern "C" int emo_stage2_compose_f32(const float* img, const float* add, const float* mask, const float* face_mask,
                                      float* out, int N, int C, int64_t HW, void* stream) {
  if (!img || !add || !mask || !face_mask || !out || N <= 0 || C <= 0 || HW <= 0) return EMO_ERR_BAD_ARG;
  hipLaunchKernelGGL(stage2_compose_kernel, dim3(grid_for((long)N * C * HW)), dim3(256), 0, (hipStream_t)stream, img,
                     add, mask, face_mask, out, (long)N, C, (long)HW);
  return emo_launch_status();
}

extern "C" int emo_resize2d_f32(const float* x, int64_t plane_stride, int64_t row_stride, float* out, int64_t NC, int H,
                                int W, int Ho, int Wo, int bicubic, int clamp01, void* stream) {
  if (!x || !out || NC <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || row_stride < W || plane_stride < 0) return EMO_ERR_BAD_ARG;
  hipLaunchKernelGGL(resize2d_kernel, dim3(grid_for(NC * Ho * Wo)), dim3(256), 0, (hipStream_t)stream, x,
                     (long)plane_stride, (long)row_stride, out, (long)NC, H, W, Ho, Wo, bicubic, clamp01);
  return emo_launch_status();
}

// ---- ABI 17 / 22: YUV 4:2:0 frames out (definitions: include/emo_hip.h; the crop and the paste: below)
namespace {
template <class L>
int pack_yuv420(const float* img, void* y, void* u, void* v, int64_t pitch_y, int64_t pitch_c, int64_t frame_stride, int N, int H, int W,
                int matrix, int full_range, void* stream) {
  Nv12Coef k;
  if (!img || !yuv_planes_ok<L>(y, u, v, pitch_y, pitch_c, frame_stride, H, W) || N <= 0 || !nv12_coef(matrix, full_range, L::bits, k))
    return EMO_ERR_BAD_ARG;
  const YuvFrame f = {static_cast<uint8_t*>(y), static_cast<uint8_t*>(u), static_cast<uint8_t*>(v), (long)pitch_y, (long)pitch_c};
  hipLaunchKernelGGL((pack_yuv420_kernel<L>), dim3(grid_for((long)N * (H / 2) * (W / 2))), dim3(256), 0, (hipStream_t)stream, img, f,
                     (long)frame_stride, (long)N, H, W, yuv_pairs<L>(y, u, pitch_y, pitch_c, frame_stride), k);
  return emo_launch_status();
}
}  // namespace

extern "C" int emo_pack_nv12(const float* img, uint8_t* y, uint8_t* uv, int64_t pitch, int64_t frame_stride, int N, int H, int W,
                             int matrix, int full_range, void* stream) {
  return pack_yuv420<Nv12>(img, y, uv, nullptr, pitch, pitch, frame_stride, N, H, W, matrix, full_range, stream);
}

extern "C" int emo_pack_yuv420(int layout, const float* img, void* y, void* u, void* v, int64_t pitch_y, int64_t pitch_c,
                               int64_t frame_stride, int N, int H, int W, int matrix, int full_range, void* stream) {
  return with_layout(layout, [&](auto l) {
    return pack_yuv420<decltype(l)>(img, y, u, v, pitch_y, pitch_c, frame_stride, N, H, W, matrix, full_range, stream);
  });
}

// ---- Frame crops and pastes (ABI 9, 15, 17, 18, 19; definitions: include/emo_hip.h): M rows (faces) cut out of or pasted into F
// frames.  One kernel per operation; what differs between the entry points is how a launch finds the frame of row m.
namespace {

enum class Frames {
  OnePerRow,   // the emo_*_windows_* entry points: row m is frame m and alone in it; frame_of is not read
  Shared,      // ABI 18: frame frame_of[m] of F frames of one size.  frame_of is sorted, so the faces of a frame are the run of
               // consecutive entries with its value
  Table,       // ABI 19: frames of different sizes behind a frame table, one face per blockIdx.y (below)
};

// [lo, hi): the run of face m, i.e. every face of its frame
template <Frames FR>
__device__ __forceinline__ void face_run(const int* __restrict__ frame_of, int M, int m, int& lo, int& hi) {
  lo = m;
  hi = m + 1;
  if constexpr (FR != Frames::OnePerRow) {
    const int f = frame_of[m];
    while (lo > 0 && frame_of[lo - 1] == f) --lo;
    while (hi < M && frame_of[hi] == f) ++hi;
  }
}

// ABI 19: frames of different sizes.  A row of the frame table is (byte address of the frame's first row, row pitch in bytes,
// H, W); a Table launch has one face per blockIdx.y, so the face's frame and its table row are uniform across the block and
// are loaded once, in front of the item loop.  A frame_of outside [0, F) gives an empty frame (H = W = 0): no window fits it.
struct FrameRow { uint8_t* base; long pitch; int H, W; };
__device__ __forceinline__ FrameRow frame_row(const long long* __restrict__ ftab, const int* __restrict__ frame_of, int F) {
  const int f = frame_of[blockIdx.y];
  FrameRow r = {nullptr, 0, 0, 0};
  if ((unsigned)f < (unsigned)F) {
    const long long* const t = ftab + 4l * f;
    r.base = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(t[0]));
    r.pitch = (long)t[1];
    r.H = (int)t[2];
    r.W = (int)t[3];
  }
  return r;
}

// The planes of a YUV 4:2:0 row of the frame table: the chroma straight after the H luma rows -- interleaved with the luma
// pitch; planar U with half of it, then V after U's H / 2 rows
template <class L>
__device__ __forceinline__ YuvFrame table_frame(const FrameRow& fr) {
  uint8_t* const u = fr.base + fr.H * fr.pitch;
  if constexpr (L::planar) return YuvFrame{fr.base, u, u + (fr.H >> 1) * (fr.pitch >> 1), fr.pitch, fr.pitch >> 1};
  else return YuvFrame{fr.base, u, nullptr, fr.pitch, fr.pitch};
}

// resize2d_kernel with one crop window PER ROW (ABI 9; animate_frames' `windows`: the reference crops every frame around its own
// face box, notebooks/infer.py:301-352): win[m] = (x0, y0, w, h) of row m inside the planes of its frame, read from device
// memory, so that a batch is ONE launch instead of one per frame (round 5: a Python loop of single-frame launches).  Per element
// the arithmetic is resize2d_kernel's on the window's first pixel: the two are bit-identical.
template <Frames FR>
__global__ __launch_bounds__(256) void resize2d_faces_kernel(const float* __restrict__ x, long plane_stride, long row_stride,
                                                             const int* __restrict__ win, const int* __restrict__ frame_of,
                                                             float* __restrict__ out, long M, int F, int C, int Ho, int Wo,
                                                             int bicubic, int clamp01) {
  const long total = M * C * Ho * Wo;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int xo = (int)(i % Wo);
    const long r = i / Wo;
    const int yo = (int)(r % Ho);
    const long mc = r / Ho, m = mc / C;
    const int f = FR == Frames::OnePerRow ? (int)m : frame_of[m];
    if (FR != Frames::OnePerRow && (unsigned)f >= (unsigned)F) { out[i] = 0.0f; continue; }
    const int* const w4 = win + 4 * m;
    const int wx0 = w4[0], wy0 = w4[1], ww = w4[2], wh = w4[3];
    const float sh = (float)wh / (float)Ho, sw = (float)ww / (float)Wo;
    const long plane = FR == Frames::OnePerRow ? mc : (long)f * C + mc % C;
    out[i] = resize2d_at(x + plane * plane_stride + (long)wy0 * row_stride + wx0, row_stride, wh, ww, sh, sw, yo, xo, bicubic, clamp01);
  }
}

// The NV12 crop (C of include/emo_hip.h): one thread per output pixel, all three channels.  The arithmetic per channel is
// resize2d_at's bicubic on the window (bicubic_window, clamp01) with every tap decoded from its bytes where it is used: the 16
// taps of neighbouring outputs overlap and the bytes under them (1.5 per pixel) stay in L1 / L2, so nothing is staged in LDS --
// the footprint of a block grows with the window's scale (up to 8.4 source pixels per output at 1080 -> 128) and has no bound a
// static tile could be sized for.  A window as large as the output is scale 1, where the bicubic weights are exactly (0, 1, 0,
// 0): the pixel's own conversion, taken directly.  A window outside its frame, or a frame_of outside [0, F), writes zeros.
// OnePerRow: win == nullptr is the whole frame.  Table (emo_nv12_faces_ragged_f32): grid (x, M), the items of a block are the
// outputs of face blockIdx.y, and the planes, the pitch and the size are those of the face's row of the frame table (frame
// stride 0: yp IS the frame).
template <Frames FR, class L>
__global__ __launch_bounds__(256) void yuv420_faces_kernel(YuvFrame f0, long fstride, int Hf, int Wf, const int* __restrict__ win,
                                                           const int* __restrict__ frame_of, float* __restrict__ out, long M, int F,
                                                           int Ho, int Wo, Nv12Coef k, const long long* __restrict__ ftab) {
  constexpr bool RAGGED = FR == Frames::Table;
  const long HWo = (long)Ho * Wo, total = (RAGGED ? 1 : M) * HWo;
  if constexpr (RAGGED) {
    const FrameRow fr = frame_row(ftab, frame_of, F);
    f0 = table_frame<L>(fr); fstride = 0; Hf = fr.H; Wf = fr.W;
  }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int xo = (int)(i % Wo);
    const long r = i / Wo;
    const int yo = (int)(r % Ho);
    const long m = RAGGED ? (long)blockIdx.y : r / Ho;
    const int f = FR == Frames::OnePerRow ? (int)m : frame_of[m];
    int wx0 = 0, wy0 = 0, ww = Wf, wh = Hf;
    if (FR != Frames::OnePerRow || win) { wx0 = win[4 * m]; wy0 = win[4 * m + 1]; ww = win[4 * m + 2]; wh = win[4 * m + 3]; }
    float* const o = out + m * 3 * HWo + (long)yo * Wo + xo;
    if ((FR != Frames::OnePerRow && (unsigned)f >= (unsigned)F) || !nv12_window_ok(wx0, wy0, ww, wh, Hf, Wf)) {
      o[0] = 0.0f; o[HWo] = 0.0f; o[2 * HWo] = 0.0f;
      continue;
    }
    const YuvFrame fr = {f0.y + f * fstride, f0.u + f * fstride, L::planar ? f0.v + f * fstride : nullptr, f0.pitch_y, f0.pitch_c};
    float acc[3];
    if (ww == Wo && wh == Ho) {
      yuv_decode_at<L>(fr, k, wy0 + yo, wx0 + xo, acc);
    } else {
      const float sh = (float)wh / (float)Ho, sw = (float)ww / (float)Wo;
      bicubic_window<3>(wh, ww, sh * ((float)yo + 0.5f) - 0.5f, sw * ((float)xo + 0.5f) - 0.5f,
                        [&](int yy, int xx, float w, float row[3]) {
                          float rgb[3];
                          yuv_decode_at<L>(fr, k, wy0 + yy, wx0 + xx, rgb);
#pragma unroll
                          for (int c = 0; c < 3; ++c) row[c] += rgb[c] * w;
                        }, acc);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = fminf(fmaxf(acc[c], 0.0f), 1.0f);
    }
    o[0] = acc[0]; o[HWo] = acc[1]; o[2 * HWo] = acc[2];
  }
}

// emo_rgb8_faces_ragged_f32: the NV12 crop's shape (and its reasoning about L1 / L2) on packed bytes -- one thread per output
// pixel of face blockIdx.y, all three channels, every tap unpack_rgb8_kernel's byte / 255, converted where it is read: bit for
// bit emo_unpack_rgb8 + emo_resize2d_faces_f32(bicubic, clamp01) without the fp32 frame.
__global__ __launch_bounds__(256) void rgb8_faces_ragged_kernel(const long long* __restrict__ ftab, const int* __restrict__ win,
                                                                const int* __restrict__ frame_of, float* __restrict__ out, int F,
                                                                int Ho, int Wo) {
  const long HWo = (long)Ho * Wo;
  const FrameRow fr = frame_row(ftab, frame_of, F);
  const long m = blockIdx.y;
  const int wx0 = win[4 * m], wy0 = win[4 * m + 1], ww = win[4 * m + 2], wh = win[4 * m + 3];
  const bool ok = nv12_window_ok(wx0, wy0, ww, wh, fr.H, fr.W);
  const uint8_t* const p = ok ? fr.base + (long)wy0 * fr.pitch + 3l * wx0 : nullptr;      // the window's first byte
  const float sh = (float)wh / (float)Ho, sw = (float)ww / (float)Wo;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < HWo; i += (long)gridDim.x * 256) {
    const int xo = (int)(i % Wo), yo = (int)(i / Wo);
    float* const o = out + m * 3 * HWo + i;
    if (!ok) { o[0] = 0.0f; o[HWo] = 0.0f; o[2 * HWo] = 0.0f; continue; }
    float acc[3];
    bicubic_window<3>(wh, ww, sh * ((float)yo + 0.5f) - 0.5f, sw * ((float)xo + 0.5f) - 0.5f, [&](int yy, int xx, float w, float row[3]) {
      const uint8_t* const px = p + (long)yy * fr.pitch + 3 * xx;
#pragma unroll
      for (int c = 0; c < 3; ++c) row[c] += __fdiv_rn((float)px[c], 255.0f) * w;
    }, acc);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * HWo] = fminf(fmaxf(acc[c], 0.0f), 1.0f);
  }
}

// The rgb8 paste.  Work items: (face, window row, run of 4 pixels), grid-stride over M * smax rows * Q runs with smax a
// host-known bound of the window sides -- the windows themselves are only read on the device.  A pixel is 3 bytes and a window's
// x0 is arbitrary, so the runs of a row start at its first pixel whose byte address is a multiple of 4 (`head` = address & 3
// pixels in: 3 * head = -head mod 4): a run inside the row is 12 bytes = three aligned dwords, read and written as such; run 0
// is the head in front of that pixel and the last run the tail, byte by byte.  No byte outside a window is read or written.
// A pixel belongs to the LAST valid face of its frame that covers it: the item of face m drops the pixels a later face of the
// run covers, starts from the frame's bytes at the others and applies every covering face lo .. m in list order, the value
// rounded to a byte after each -- the bytes of pasting the faces one after another (OnePerRow: the run is the face itself).  A
// run of 4 pixels that is wholly the item's own keeps the three aligned dwords; a mixed run, the head and the tail go byte by
// byte.  Every byte has one writer and is read by that writer only; `win`, `frame_of` and `img` are read by the items of every
// face of the frame.  A window that fails paste_window_ok, or a frame_of outside [0, F), is absent.
// Table (emo_paste_faces_ragged_rgb8): grid (x, M), `total` the items of ONE face, the face blockIdx.y; `frames`, the row pitch
// and the size are those of the face's row of the frame table.  The head of a row is taken from its address, whatever the
// frame's address and pitch are.
template <Frames FR>
__global__ __launch_bounds__(256) void paste_faces_kernel(const float* __restrict__ img, const float* __restrict__ matte,
                                                          const int* __restrict__ win, const int* __restrict__ frame_of,
                                                          uint8_t* __restrict__ frames, unsigned total, int M, int F, int S, int Hf,
                                                          int Wf, unsigned smax, float feather, const long long* __restrict__ ftab) {
  constexpr bool RAGGED = FR == Frames::Table;
  const unsigned Q = (smax + 3u) / 4u + 1u;
  const long SS = (long)S * S;
  long pitch = 0;
  if constexpr (RAGGED) {
    const FrameRow fr = frame_row(ftab, frame_of, F);
    frames = fr.base; pitch = fr.pitch; Hf = fr.H; Wf = fr.W;
  }
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned q = i % Q, rr = i / Q;
    const int y = (int)(rr % smax);
    const int m = RAGGED ? (int)blockIdx.y : (int)(rr / smax);
    const int wx0 = win[4 * m], wy0 = win[4 * m + 1], s = win[4 * m + 2];
    const int f = FR == Frames::OnePerRow ? m : frame_of[m];
    if ((FR != Frames::OnePerRow && (unsigned)f >= (unsigned)F) || !paste_window_ok(wx0, wy0, s, win[4 * m + 3], S, Hf, Wf) || y >= s) continue;
    const int py = wy0 + y;
    uint8_t* const row = RAGGED ? frames + (long)py * pitch + 3l * wx0 : frames + (((long)f * Hf + py) * Wf + wx0) * 3;
    const int head = (int)(reinterpret_cast<uintptr_t>(row) & 3);
    const int xa = head + 4 * ((int)q - 1);
    if (xa >= s) continue;
    int lo, hi;
    face_run<FR>(frame_of, M, m, lo, hi);
    // bit p: pixel xa + p is inside the window and no later face of the frame covers it
    unsigned own = 0u;
#pragma unroll
    for (int p = 0; p < 4; ++p) own |= (xa + p >= 0 && xa + p < s) ? 1u << p : 0u;
    for (int j = m + 1; j < hi; ++j) {
      const int jx = win[4 * j], jy = win[4 * j + 1], js = win[4 * j + 2];
      if (!paste_window_ok(jx, jy, js, win[4 * j + 3], S, Hf, Wf) || py < jy || py >= jy + js) continue;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int px = wx0 + xa + p;
        if (px >= jx && px < jx + js) own &= ~(1u << p);
      }
    }
    if (!own) continue;
    const bool whole = own == 15u;                       // (then xa >= 0 and xa + 4 <= s)
    uint32_t* const dw = reinterpret_cast<uint32_t*>(row + 3 * xa);
    unsigned v[12];
    if (whole) {
      const uint32_t d[3] = {dw[0], dw[1], dw[2]};
#pragma unroll
      for (int k = 0; k < 12; ++k) v[k] = (d[k >> 2] >> (8 * (k & 3))) & 255u;
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) v[k] = (own >> (k / 3)) & 1u ? row[3 * xa + k] : 0u;
    }
    for (int j = lo; j <= m; ++j) {
      const int jx = win[4 * j], jy = win[4 * j + 1], js = win[4 * j + 2];
      if (!paste_window_ok(jx, jy, js, win[4 * j + 3], S, Hf, Wf) || py < jy || py >= jy + js) continue;
      const int yj = py - jy;
      const float scale = (float)S / (float)js, inv_scale = __fdiv_rn(1.0f, scale), fs = feather * (float)js;
      const float* const im = img + j * 3 * SS;
      const float* const mt = matte ? matte + j * SS : nullptr;
      AaTaps ty = {0, 0, 0.0f, 0.0f};
      if (js < S) ty = aa_taps(yj, scale, inv_scale, S);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int xj = wx0 + xa + p - jx;
        if (!((own >> p) & 1u) || xj < 0 || xj >= js) continue;
        float r[3];
        paste_render(im, S, js, scale, inv_scale, ty, yj, xj, r);
        const float a = paste_alpha(mt, S, js, scale, feather, fs, yj, xj);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * p + c] = paste_blend(a, v[3 * p + c], r[c]);
      }
    }
    if (whole) {
      uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 12; ++k) o[k >> 2] |= v[k] << (8 * (k & 3));
      dw[0] = o[0]; dw[1] = o[1]; dw[2] = o[2];
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
        if ((own >> (k / 3)) & 1u) row[3 * xa + k] = (uint8_t)v[k];
    }
  }
}

// does the valid window (x0, y0, s) touch chroma sample (cy, cx), i.e. hold one of its four luma pixels
__device__ __forceinline__ bool chroma_touched(int x0, int y0, int s, int cy, int cx) {
  return cx >= (x0 >> 1) && 2 * cx < x0 + s && cy >= (y0 >> 1) && 2 * cy < y0 + s;
}

// The NV12 paste (P of include/emo_hip.h).  Work items: (face, chroma sample of the window's covering chroma rectangle, with
// those of the sample's four luma pixels that lie inside a window; the image and the blend weight of each from the rgb8
// paste's paste_render01 / paste_alpha), grid-stride over M * cmax * cmax with cmax a host-known bound of the samples along a
// window side.  A sample belongs to the LAST valid face of its frame that touches it; its item starts from the frame's bytes
// and applies every touching face lo .. m in list order, every value rounded to a byte after each face (OnePerRow: the run is
// the face itself).  A luma byte no window holds is neither read nor written; a chroma pair is touched only if one of its luma
// pixels is inside a window.
// Table (emo_paste_faces_ragged_nv12): as in paste_faces_kernel -- one face per blockIdx.y, its frame from the frame table
template <Frames FR, class L>
__global__ __launch_bounds__(256) void paste_faces_yuv420_kernel(const float* __restrict__ img, const float* __restrict__ matte,
                                                                 const int* __restrict__ win, const int* __restrict__ frame_of,
                                                                 YuvFrame f0, long fstride, unsigned total, int M, int F, int S,
                                                                 int Hf, int Wf, unsigned cmax, float feather, Nv12Coef k,
                                                                 const long long* __restrict__ ftab) {
  using T = typename L::sample;
  constexpr bool RAGGED = FR == Frames::Table;
  const long SS = (long)S * S;
  if constexpr (RAGGED) {
    const FrameRow fr = frame_row(ftab, frame_of, F);
    f0 = table_frame<L>(fr); fstride = 0; Hf = fr.H; Wf = fr.W;
  }
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned rr = i / cmax;
    const int m = RAGGED ? (int)blockIdx.y : (int)(rr / cmax);
    const int wx0 = win[4 * m], wy0 = win[4 * m + 1], s = win[4 * m + 2];
    const int f = FR == Frames::OnePerRow ? m : frame_of[m];
    if ((FR != Frames::OnePerRow && (unsigned)f >= (unsigned)F) || !paste_window_ok(wx0, wy0, s, win[4 * m + 3], S, Hf, Wf)) continue;
    const int cx = (wx0 >> 1) + (int)(i % cmax), cy = (wy0 >> 1) + (int)(rr % cmax);
    if (2 * cx >= wx0 + s || 2 * cy >= wy0 + s) continue;
    int lo, hi;
    face_run<FR>(frame_of, M, m, lo, hi);
    bool owned = true;
    for (int j = m + 1; j < hi; ++j) {
      const int jx = win[4 * j], jy = win[4 * j + 1], js = win[4 * j + 2];
      if (paste_window_ok(jx, jy, js, win[4 * j + 3], S, Hf, Wf) && chroma_touched(jx, jy, js, cy, cx)) owned = false;
    }
    if (!owned) continue;
    T* const fy0 = yuv_row<L>(f0.y + f * fstride, 2 * cy, f0.pitch_y) + 2 * cx;        // the sample's 2 x 2 luma block
    T* const fy[2] = {fy0, reinterpret_cast<T*>(reinterpret_cast<uint8_t*>(fy0) + f0.pitch_y)};
    T* const pu = L::planar ? yuv_row<L>(f0.u + f * fstride, cy, f0.pitch_c) + cx : yuv_row<L>(f0.u + f * fstride, cy, f0.pitch_c) + 2 * cx;
    T* const pv = L::planar ? yuv_row<L>(f0.v + f * fstride, cy, f0.pitch_c) + cx : pu + 1;
    // which of the block's luma pixels some face lo .. m holds: only those are read, carried and written
    unsigned held = 0u;
    for (int j = lo; j <= m; ++j) {
      const int jx = win[4 * j], jy = win[4 * j + 1], js = win[4 * j + 2];
      if (!paste_window_ok(jx, jy, js, win[4 * j + 3], S, Hf, Wf)) continue;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int yj = 2 * cy + (d >> 1) - jy, xj = 2 * cx + (d & 1) - jx;
        if (yj >= 0 && yj < js && xj >= 0 && xj < js) held |= 1u << d;
      }
    }
    unsigned yb[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) yb[d] = (held >> d) & 1u ? L::code(fy[d >> 1][d & 1]) : 0u;
    unsigned u = L::code(*pu), v = L::code(*pv);
    for (int j = lo; j <= m; ++j) {
      const int jx = win[4 * j], jy = win[4 * j + 1], js = win[4 * j + 2];
      if (!paste_window_ok(jx, jy, js, win[4 * j + 3], S, Hf, Wf) || !chroma_touched(jx, jy, js, cy, cx)) continue;
      const float scale = (float)S / (float)js, inv_scale = __fdiv_rn(1.0f, scale), fs = feather * (float)js;
      const float* const im = img + j * 3 * SS;
      const float* const mt = matte ? matte + j * SS : nullptr;
      float a4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, cb4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, cr4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        const int yj = 2 * cy + dy - jy;
        if (yj < 0 || yj >= js) continue;
        AaTaps ty = {0, 0, 0.0f, 0.0f};
        if (js < S) ty = aa_taps(yj, scale, inv_scale, S);
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int xj = 2 * cx + dx - jx;
          if (xj < 0 || xj >= js) continue;
          float r[3], yc, cbc, crc;
          paste_render01(im, S, js, scale, inv_scale, ty, yj, xj, r);
          const float a = paste_alpha(mt, S, js, scale, feather, fs, yj, xj);
          yuv_encode<L>(k, r, yc, cbc, crc);
          yb[2 * dy + dx] = yuv_code<L>(((1.0f - a) * (float)yb[2 * dy + dx] + a * yc) + 0.5f);
          a4[2 * dy + dx] = a;
          cb4[2 * dy + dx] = a * cbc;
          cr4[2 * dy + dx] = a * crc;
        }
      }
      const float na = 1.0f - (((a4[0] + a4[1]) + a4[2]) + a4[3]) * 0.25f;
      u = yuv_code<L>((na * (float)u + (((cb4[0] + cb4[1]) + cb4[2]) + cb4[3]) * 0.25f) + 0.5f);
      v = yuv_code<L>((na * (float)v + (((cr4[0] + cr4[1]) + cr4[2]) + cr4[3]) * 0.25f) + 0.5f);
    }
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if ((held >> d) & 1u) fy[d >> 1][d & 1] = L::word(yb[d]);
    *pu = L::word(u);
    *pv = L::word(v);
  }
}

// ---- the host side of the twelve entry points: what they check before a launch, and the launches

// frame_of_host: non-decreasing, every entry in [0, F)
inline bool frame_of_ok(const int32_t* frame_of_host, int M, int F) {
  for (int m = 0; m < M; ++m)
    if (frame_of_host[m] < 0 || frame_of_host[m] >= F || (m > 0 && frame_of_host[m] < frame_of_host[m - 1])) return false;
  return true;
}

// A host-side window list: every window inside its frame -- Hf x Wf, or with table_host the frame of ITS OWN face -- or
// EMO_ERR_BAD_ARG; for a paste also a square with 4 s >= S, or EMO_ERR_UNSUPPORTED.  -> EMO_OK and in smax the largest side;
// windows that only the device knows: any valid side (with a table the caller's bound stays).
inline int host_windows(const int32_t* windows_host, int M, int S, bool paste, int Hf, int Wf, const int64_t* table_host,
                        const int32_t* frame_of_host, int& smax) {
  if (!table_host) smax = Hf < Wf ? Hf : Wf;
  if (!windows_host) return EMO_OK;
  smax = 0;
  for (int m = 0; m < M; ++m) {
    const int32_t* w = windows_host + 4 * m;
    if (table_host) { Hf = (int)table_host[4l * frame_of_host[m] + 2]; Wf = (int)table_host[4l * frame_of_host[m] + 3]; }
    if (!nv12_window_ok(w[0], w[1], w[2], w[3], Hf, Wf)) return EMO_ERR_BAD_ARG;
    if (paste && !paste_window_ok(w[0], w[1], w[2], w[3], S, Hf, Wf)) return EMO_ERR_UNSUPPORTED;   // not square, or 4 s < S
    smax = w[2] > smax ? w[2] : smax;
  }
  return EMO_OK;
}

// ABI 19 / 22.  What the ragged entry points check on the host copy of the frame table and the lists, before a launch: every
// row an address, a size that fits an int (YUV: even) and a pitch of at least a row's bytes (16-bit samples: an even address
// and pitch; planar: a pitch that halves into whole samples); frame_of and the windows as above.  -> EMO_OK and, for the paste, the largest side to cover.
enum class Rows { Rgb8, Interleaved, Planar };   // what a row of the frame table holds: packed pixels, or YUV 4:2:0 planes
inline int ragged_args(const int64_t* table_host, int F, int px_bytes, Rows rows, const int32_t* windows_host,
                       const int32_t* frame_of_host, int M, int S, bool paste, int& smax) {
  smax = 0;
  for (int f = 0; f < F; ++f) {
    const int64_t* t = table_host + 4l * f;
    if (t[0] == 0 || t[2] <= 0 || t[3] <= 0 || t[2] > 0x7fffffffl || t[3] > 0x7fffffffl / px_bytes || t[1] < t[3] * px_bytes) return EMO_ERR_BAD_ARG;
    if (rows != Rows::Rgb8 && ((t[2] | t[3]) & 1)) return EMO_ERR_BAD_ARG;
    if (rows != Rows::Rgb8 && px_bytes == 2 && ((t[0] | t[1]) & 1)) return EMO_ERR_BAD_ARG;          // 16-bit samples: even address, pitch
    if (rows == Rows::Planar && t[1] % (2 * px_bytes)) return EMO_ERR_BAD_ARG;                       // the chroma pitch is pitch / 2
    const int side = (int)(t[2] < t[3] ? t[2] : t[3]);
    smax = side > smax ? side : smax;                // windows that only the device knows: any valid side of any frame
  }
  if (!frame_of_ok(frame_of_host, M, F)) return EMO_ERR_BAD_ARG;
  return host_windows(windows_host, M, S, paste, 0, 0, table_host, frame_of_host, smax);
}

// grid (x, M): one face per blockIdx.y, x covering `per` items of a face, about 8192 blocks in all as grid_for
inline dim3 ragged_grid(long per, int M) {
  const long cap = 8192 / M < 1 ? 1 : 8192 / M;
  long g = (per + 255) / 256;
  g = g < 1 ? 1 : (g > cap ? cap : g);
  return dim3((unsigned)g, (unsigned)M);
}

// The items of a paste launch over M >= 1 faces from the largest side to cover -> false where they exceed the kernels' 32-bit
// index.  rgb8: smax rows x ((smax + 3) / 4 + 1) runs per face, bound = smax; NV12: cmax x cmax chroma samples, bound = cmax.
// `total` is what the kernel strides over: the items of all faces, or with a table those of one (grid (x, M)).
inline bool paste_items(int smax, bool nv12, bool table, int M, unsigned& bound, unsigned& total, dim3& grid) {
  const long cmax = smax / 2 + 1;                  // chroma samples under s luma pixels: at most s / 2 + 1 (an odd origin)
  const long per = nv12 ? cmax * cmax : smax * (((long)smax + 3) / 4 + 1);
  if (table ? M > 65535 || per > 0x7fffffffl : per > 0x7fffffffl / M) return false;
  bound = (unsigned)(nv12 ? cmax : smax);
  total = (unsigned)(table ? per : per * M);
  grid = table ? ragged_grid(per, M) : dim3(grid_for(per * M));
  return true;
}

template <Frames FR, class L>
int launch_yuv420_crop(const YuvFrame& f, int64_t frame_stride, int Hf, int Wf, const int32_t* windows, const int32_t* frame_of, float* out,
                       int M, int F, int Ho, int Wo, const Nv12Coef& k, const int64_t* table, void* stream) {
  const dim3 grid = FR == Frames::Table ? ragged_grid((long)Ho * Wo, M) : dim3(grid_for((long)M * Ho * Wo));
  hipLaunchKernelGGL((yuv420_faces_kernel<FR, L>), grid, dim3(256), 0, (hipStream_t)stream, f, (long)frame_stride, Hf, Wf, windows,
                     frame_of, out, (long)M, F, Ho, Wo, k, reinterpret_cast<const long long*>(table));
  return emo_launch_status();
}

template <Frames FR>
int launch_paste_rgb8(const float* img, const float* matte, const int32_t* windows, const int32_t* frame_of, uint8_t* frames, int M,
                      int F, int S, int Hf, int Wf, int smax, float feather, const int64_t* table, void* stream) {
  unsigned bound, total;
  dim3 grid;
  if (!paste_items(smax, false, FR == Frames::Table, M, bound, total, grid)) return EMO_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(paste_faces_kernel<FR>, grid, dim3(256), 0, (hipStream_t)stream, img, matte, windows, frame_of, frames, total, M, F,
                     S, Hf, Wf, bound, feather, reinterpret_cast<const long long*>(table));
  return emo_launch_status();
}

template <Frames FR, class L>
int launch_paste_yuv420(const float* img, const float* matte, const int32_t* windows, const int32_t* frame_of, const YuvFrame& f,
                        int64_t frame_stride, int M, int F, int S, int Hf, int Wf, int smax, float feather, const Nv12Coef& k,
                        const int64_t* table, void* stream) {
  unsigned bound, total;
  dim3 grid;
  if (!paste_items(smax, true, FR == Frames::Table, M, bound, total, grid)) return EMO_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((paste_faces_yuv420_kernel<FR, L>), grid, dim3(256), 0, (hipStream_t)stream, img, matte, windows, frame_of, f,
                     (long)frame_stride, total, M, F, S, Hf, Wf, bound, feather, k, reinterpret_cast<const long long*>(table));
  return emo_launch_status();
}

inline bool feather_ok(float feather) { return feather >= 0.0f && feather <= 0.5f; }

inline YuvFrame yuv_frame(const void* y, const void* u, const void* v, int64_t pitch_y, int64_t pitch_c) {
  return YuvFrame{static_cast<uint8_t*>(const_cast<void*>(y)), static_cast<uint8_t*>(const_cast<void*>(u)),
                  static_cast<uint8_t*>(const_cast<void*>(v)), (long)pitch_y, (long)pitch_c};
}

// C on frames of one size.  frame_of == nullptr: row m is frame m (ABI 17's form; windows == nullptr: every frame whole);
// otherwise face m lies in frame frame_of[m] of F (ABI 18's form)
template <class L>
int yuv420_crop(const void* y, const void* u, const void* v, int64_t pitch_y, int64_t pitch_c, int64_t frame_stride, int Hf, int Wf,
                const int32_t* windows, const int32_t* windows_host, const int32_t* frame_of, const int32_t* frame_of_host, float* out,
                int M, int F, int Ho, int Wo, int matrix, int full_range, void* stream) {
  Nv12Coef k;
  int smax;
  if (!yuv_planes_ok<L>(y, u, v, pitch_y, pitch_c, frame_stride, Hf, Wf) || !out || Ho <= 0 || Wo <= 0) return EMO_ERR_BAD_ARG;
  if (!nv12_coef(matrix, full_range, L::bits, k)) return EMO_ERR_BAD_ARG;
  if (frame_of ? !windows || M < 0 || F <= 0 || (frame_of_host && !frame_of_ok(frame_of_host, M, F))
               : M <= 0 || frame_of_host || (windows_host && !windows)) return EMO_ERR_BAD_ARG;
  if (host_windows(windows_host, M, 0, false, Hf, Wf, nullptr, nullptr, smax) != EMO_OK) return EMO_ERR_BAD_ARG;
  if (M == 0) return EMO_OK;
  const YuvFrame f = yuv_frame(y, u, v, pitch_y, pitch_c);
  if (frame_of) return launch_yuv420_crop<Frames::Shared, L>(f, frame_stride, Hf, Wf, windows, frame_of, out, M, F, Ho, Wo, k, nullptr, stream);
  return launch_yuv420_crop<Frames::OnePerRow, L>(f, frame_stride, Hf, Wf, windows, nullptr, out, M, M, Ho, Wo, k, nullptr, stream);
}

// P on frames of one size, in place; frame_of as in yuv420_crop (the faces form needs frame_of_host: the order of the paste)
template <class L>
int yuv420_paste(const float* img, const float* matte, const int32_t* windows, const int32_t* windows_host, const int32_t* frame_of,
                 const int32_t* frame_of_host, void* y, void* u, void* v, int64_t pitch_y, int64_t pitch_c, int64_t frame_stride, int M,
                 int F, int S, int Hf, int Wf, float feather, int matrix, int full_range, void* stream) {
  Nv12Coef k;
  if (!img || !windows || !yuv_planes_ok<L>(y, u, v, pitch_y, pitch_c, frame_stride, Hf, Wf) || S <= 0) return EMO_ERR_BAD_ARG;
  if (!feather_ok(feather) || !nv12_coef(matrix, full_range, L::bits, k)) return EMO_ERR_BAD_ARG;
  if (frame_of ? !frame_of_host || M < 0 || F <= 0 || !frame_of_ok(frame_of_host, M, F) : M <= 0 || frame_of_host != nullptr)
    return EMO_ERR_BAD_ARG;
  int smax;
  const int rc = host_windows(windows_host, M, S, true, Hf, Wf, nullptr, nullptr, smax);
  if (rc != EMO_OK || M == 0) return rc;
  const YuvFrame f = yuv_frame(y, u, v, pitch_y, pitch_c);
  if (frame_of)
    return launch_paste_yuv420<Frames::Shared, L>(img, matte, windows, frame_of, f, frame_stride, M, F, S, Hf, Wf, smax, feather, k, nullptr, stream);
  return launch_paste_yuv420<Frames::OnePerRow, L>(img, matte, windows, nullptr, f, frame_stride, M, M, S, Hf, Wf, smax, feather, k, nullptr, stream);
}

// C and P on the frames of a frame table (ABI 19's form)
template <class L>
int yuv420_crop_ragged(const int64_t* table, const int64_t* table_host, const int32_t* windows, const int32_t* windows_host,
                       const int32_t* frame_of, const int32_t* frame_of_host, float* out, int M, int F, int Ho, int Wo, int matrix,
                       int full_range, void* stream) {
  Nv12Coef k;
  if (!table || !table_host || !windows || !frame_of || !frame_of_host || !out || M < 0 || F <= 0 || Ho <= 0 || Wo <= 0) return EMO_ERR_BAD_ARG;
  if (!nv12_coef(matrix, full_range, L::bits, k)) return EMO_ERR_BAD_ARG;
  int smax;
  const int rc = ragged_args(table_host, F, (int)sizeof(typename L::sample), L::planar ? Rows::Planar : Rows::Interleaved, windows_host,
                             frame_of_host, M, 0, false, smax);
  if (rc != EMO_OK || M == 0) return rc;
  if (M > 65535) return EMO_ERR_UNSUPPORTED;
  return launch_yuv420_crop<Frames::Table, L>(YuvFrame{nullptr, nullptr, nullptr, 0, 0}, 0, 0, 0, windows, frame_of, out, M, F, Ho, Wo, k, table, stream);
}

template <class L>
int yuv420_paste_ragged(const float* img, const float* matte, const int64_t* table, const int64_t* table_host, const int32_t* windows,
                        const int32_t* windows_host, const int32_t* frame_of, const int32_t* frame_of_host, int M, int F, int S,
                        float feather, int matrix, int full_range, void* stream) {
  Nv12Coef k;
  if (!img || !table || !table_host || !windows || !frame_of || !frame_of_host || M < 0 || F <= 0 || S <= 0) return EMO_ERR_BAD_ARG;
  if (!feather_ok(feather) || !nv12_coef(matrix, full_range, L::bits, k)) return EMO_ERR_BAD_ARG;
  int smax;
  const int rc = ragged_args(table_host, F, (int)sizeof(typename L::sample), L::planar ? Rows::Planar : Rows::Interleaved, windows_host,
                             frame_of_host, M, S, true, smax);
  if (rc != EMO_OK || M == 0) return rc;
  return launch_paste_yuv420<Frames::Table, L>(img, matte, windows, frame_of, YuvFrame{nullptr, nullptr, nullptr, 0, 0}, 0, M, F, S, 0, 0, smax,
                                               feather, k, table, stream);
}

}  // namespace

// ---- one crop window per frame (ABI 9, 15, 17): the faces kernels with one row per frame
extern "C" int emo_resize2d_windows_f32(const float* x, int64_t plane_stride, int64_t row_stride, const int* windows, float* out,
                                        int N, int C, int Ho, int Wo, int bicubic, int clamp01, void* stream) {
  if (!x || !out || !windows || N <= 0 || C <= 0 || Ho <= 0 || Wo <= 0 || row_stride <= 0 || plane_stride < 0) return EMO_ERR_BAD_ARG;
  hipLaunchKernelGGL(resize2d_faces_kernel<Frames::OnePerRow>, dim3(grid_for((long)N * C * Ho * Wo)), dim3(256), 0, (hipStream_t)stream,
                     x, (long)plane_stride, (long)row_stride, windows, (const int*)nullptr, out, (long)N, N, C, Ho, Wo, bicubic, clamp01);
  return emo_launch_status();
}

extern "C" int emo_nv12_windows_f32(const uint8_t* y, const uint8_t* uv, int64_t pitch, int64_t frame_stride, int Hf, int Wf,
                                    const int32_t* windows, const int32_t* windows_host, float* out, int N, int Ho, int Wo,
                                    int matrix, int full_range, void* stream) {
  return yuv420_crop<Nv12>(y, uv, nullptr, pitch, pitch, frame_stride, Hf, Wf, windows, windows_host, nullptr, nullptr, out, N, N, Ho, Wo,
                           matrix, full_range, stream);
}

extern "C" int emo_paste_windows_rgb8(const float* img, const float* matte, const int32_t* windows, const int32_t* windows_host,
                                      uint8_t* frames, int N, int S, int Hf, int Wf, float feather, void* stream) {
  if (!img || !windows || !frames || N <= 0 || S <= 0 || Hf <= 0 || Wf <= 0) return EMO_ERR_BAD_ARG;
  if (!feather_ok(feather)) return EMO_ERR_BAD_ARG;
  int smax;
  const int rc = host_windows(windows_host, N, S, true, Hf, Wf, nullptr, nullptr, smax);
  if (rc != EMO_OK) return rc;
  return launch_paste_rgb8<Frames::OnePerRow>(img, matte, windows, nullptr, frames, N, N, S, Hf, Wf, smax, feather, nullptr, stream);
}

extern "C" int emo_paste_windows_nv12(const float* img, const float* matte, const int32_t* windows, const int32_t* windows_host,
                                      uint8_t* y, uint8_t* uv, int64_t pitch, int64_t frame_stride, int N, int S, int Hf, int Wf,
                                      float feather, int matrix, int full_range, void* stream) {
  return yuv420_paste<Nv12>(img, matte, windows, windows_host, nullptr, nullptr, y, uv, nullptr, pitch, pitch, frame_stride, N, N, S, Hf, Wf,
                            feather, matrix, full_range, stream);
}

// ---- ABI 18: several faces per frame, face m in frame frame_of[m]
extern "C" int emo_resize2d_faces_f32(const float* x, int64_t plane_stride, int64_t row_stride, const int32_t* windows,
                                      const int32_t* frame_of, float* out, int M, int F, int C, int Ho, int Wo, int bicubic,
                                      int clamp01, void* stream) {
  if (!x || !out || !windows || !frame_of || M < 0 || F <= 0 || C <= 0 || Ho <= 0 || Wo <= 0 || row_stride <= 0 || plane_stride < 0)
    return EMO_ERR_BAD_ARG;
  if (M == 0) return EMO_OK;
  hipLaunchKernelGGL(resize2d_faces_kernel<Frames::Shared>, dim3(grid_for((long)M * C * Ho * Wo)), dim3(256), 0, (hipStream_t)stream, x,
                     (long)plane_stride, (long)row_stride, windows, frame_of, out, (long)M, F, C, Ho, Wo, bicubic, clamp01);
  return emo_launch_status();
}

extern "C" int emo_nv12_faces_f32(const uint8_t* y, const uint8_t* uv, int64_t pitch, int64_t frame_stride, int Hf, int Wf,
                                  const int32_t* windows, const int32_t* windows_host, const int32_t* frame_of,
                                  const int32_t* frame_of_host, float* out, int M, int F, int Ho, int Wo, int matrix, int full_range,
                                  void* stream) {
  if (!frame_of) return EMO_ERR_BAD_ARG;
  return yuv420_crop<Nv12>(y, uv, nullptr, pitch, pitch, frame_stride, Hf, Wf, windows, windows_host, frame_of, frame_of_host, out, M, F, Ho,
                           Wo, matrix, full_range, stream);
}

extern "C" int emo_paste_faces_rgb8(const float* img, const float* matte, const int32_t* windows, const int32_t* windows_host,
                                    const int32_t* frame_of, const int32_t* frame_of_host, uint8_t* frames, int M, int F, int S,
                                    int Hf, int Wf, float feather, void* stream) {
  if (!img || !windows || !frame_of || !frame_of_host || !frames || M < 0 || F <= 0 || S <= 0 || Hf <= 0 || Wf <= 0) return EMO_ERR_BAD_ARG;
  if (!feather_ok(feather) || !frame_of_ok(frame_of_host, M, F)) return EMO_ERR_BAD_ARG;
  int smax;
  const int rc = host_windows(windows_host, M, S, true, Hf, Wf, nullptr, nullptr, smax);
  if (rc != EMO_OK || M == 0) return rc;
  return launch_paste_rgb8<Frames::Shared>(img, matte, windows, frame_of, frames, M, F, S, Hf, Wf, smax, feather, nullptr, stream);
}

extern "C" int emo_paste_faces_nv12(const float* img, const float* matte, const int32_t* windows, const int32_t* windows_host,
                                    const int32_t* frame_of, const int32_t* frame_of_host, uint8_t* y, uint8_t* uv, int64_t pitch,
                                    int64_t frame_stride, int M, int F, int S, int Hf, int Wf, float feather, int matrix,
                                    int full_range, void* stream) {
  if (!frame_of) return EMO_ERR_BAD_ARG;
  return yuv420_paste<Nv12>(img, matte, windows, windows_host, frame_of, frame_of_host, y, uv, nullptr, pitch, pitch, frame_stride, M, F, S,
                            Hf, Wf, feather, matrix, full_range, stream);
}

// ---- ABI 19: the frames of a batch in different sizes, addressed through a frame table
extern "C" int emo_rgb8_faces_ragged_f32(const int64_t* table, const int64_t* table_host, const int32_t* windows,
                                         const int32_t* windows_host, const int32_t* frame_of, const int32_t* frame_of_host,
                                         float* out, int M, int F, int Ho, int Wo, void* stream) {
  if (!table || !table_host || !windows || !frame_of || !frame_of_host || !out || M < 0 || F <= 0 || Ho <= 0 || Wo <= 0) return EMO_ERR_BAD_ARG;
  int smax;
  const int rc = ragged_args(table_host, F, 3, Rows::Rgb8, windows_host, frame_of_host, M, 0, false, smax);
  if (rc != EMO_OK || M == 0) return rc;
  if (M > 65535) return EMO_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(rgb8_faces_ragged_kernel, ragged_grid((long)Ho * Wo, M), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(table), windows, frame_of, out, F, Ho, Wo);
  return emo_launch_status();
}

extern "C" int emo_nv12_faces_ragged_f32(const int64_t* table, const int64_t* table_host, const int32_t* windows,
                                         const int32_t* windows_host, const int32_t* frame_of, const int32_t* frame_of_host,
                                         float* out, int M, int F, int Ho, int Wo, int matrix, int full_range, void* stream) {
  return yuv420_crop_ragged<Nv12>(table, table_host, windows, windows_host, frame_of, frame_of_host, out, M, F, Ho, Wo, matrix, full_range,
                                  stream);
}

extern "C" int emo_paste_faces_ragged_rgb8(const float* img, const float* matte, const int64_t* table, const int64_t* table_host,
                                           const int32_t* windows, const int32_t* windows_host, const int32_t* frame_of,
                                           const int32_t* frame_of_host, int M, int F, int S, float feather, void* stream) {
  if (!img || !table || !table_host || !windows || !frame_of || !frame_of_host || M < 0 || F <= 0 || S <= 0) return EMO_ERR_BAD_ARG;
  if (!feather_ok(feather)) return EMO_ERR_BAD_ARG;
  int smax;
  const int rc = ragged_args(table_host, F, 3, Rows::Rgb8, windows_host, frame_of_host, M, S, true, smax);
  if (rc != EMO_OK || M == 0) return rc;
  return launch_paste_rgb8<Frames::Table>(img, matte, windows, frame_of, nullptr, M, F, S, 0, 0, smax, feather, table, stream);
}

extern "C" int emo_paste_faces_ragged_nv12(const float* img, const float* matte, const int64_t* table, const int64_t* table_host,
                                           const int32_t* windows, const int32_t* windows_host, const int32_t* frame_of,
                                           const int32_t* frame_of_host, int M, int F, int S, float feather, int matrix,
                                           int full_range, void* stream) {
  return yuv420_paste_ragged<Nv12>(img, matte, table, table_host, windows, windows_host, frame_of, frame_of_host, M, F, S, feather, matrix,
                                   full_range, stream);
}

// ---- ABI 22: the same five operations on any of the four sample layouts (0 nv12, 1 yuv420p, 2 p010, 3 yuv420p10)
extern "C" int emo_yuv420_crop_f32(int layout, const void* y, const void* u, const void* v, int64_t pitch_y, int64_t pitch_c,
                                   int64_t frame_stride, int Hf, int Wf, const int32_t* windows, const int32_t* windows_host,
                                   const int32_t* frame_of, const int32_t* frame_of_host, float* out, int M, int F, int Ho, int Wo,
                                   int matrix, int full_range, void* stream) {
  return with_layout(layout, [&](auto l) {
    return yuv420_crop<decltype(l)>(y, u, v, pitch_y, pitch_c, frame_stride, Hf, Wf, windows, windows_host, frame_of, frame_of_host, out, M,
                                    F, Ho, Wo, matrix, full_range, stream);
  });
}

extern "C" int emo_paste_yuv420(int layout, const float* img, const float* matte, const int32_t* windows, const int32_t* windows_host,
                                const int32_t* frame_of, const int32_t* frame_of_host, void* y, void* u, void* v, int64_t pitch_y,
                                int64_t pitch_c, int64_t frame_stride, int M, int F, int S, int Hf, int Wf, float feather, int matrix,
                                int full_range, void* stream) {
  return with_layout(layout, [&](auto l) {
    return yuv420_paste<decltype(l)>(img, matte, windows, windows_host, frame_of, frame_of_host, y, u, v, pitch_y, pitch_c, frame_stride, M,
                                     F, S, Hf, Wf, feather, matrix, full_range, stream);
  });
}

extern "C" int emo_yuv420_crop_ragged_f32(int layout, const int64_t* table, const int64_t* table_host, const int32_t* windows,
                                          const int32_t* windows_host, const int32_t* frame_of, const int32_t* frame_of_host,
                                          float* out, int M, int F, int Ho, int Wo, int matrix, int full_range, void* stream) {
  return with_layout(layout, [&](auto l) {
    return yuv420_crop_ragged<decltype(l)>(table, table_host, windows, windows_host, frame_of, frame_of_host, out, M, F, Ho, Wo, matrix,
                                           full_range, stream);
  });
}

extern "C" int emo_paste_ragged_yuv420(int layout, const float* img, const float* matte, const int64_t* table, const int64_t* table_host,
                                       const int32_t* windows, const int32_t* windows_host, const int32_t* frame_of,
                                       const int32_t* frame_of_host, int M, int F, int S, float feather, int matrix, int full_range,
                                       void* stream) {
  return with_layout(layout, [&](auto l) {
    return yuv420_paste_ragged<decltype(l)>(img, matte, table, table_host, windows, windows_host, frame_of, frame_of_host, M, F, S, feather,
                                            matrix, full_range, stream);
  });
}
