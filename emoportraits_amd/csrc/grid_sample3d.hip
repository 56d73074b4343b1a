// 3-D trilinear grid_sample (align_corners=False) for gfx950 -- SURVEY.md section 8 rows a1 + a2.
//
// Replaces  F.grid_sample(inputs.float(), grid.float(), padding_mode=...)  on 5-D tensors
// (reference: models/stage_1/volumetric_avatar/va.py:264-265; call sites notebooks/infer.py:499-500,
// :618-619).  The arithmetic restated here is ATen's CPU grid_sampler_3d (ATen/native/GridSampler.h:
// grid_sampler_unnormalize :27-36, clip_coordinates :58-60, reflect_coordinates :89-106) and is kept
// bit-identical to it: all coordinate/weight math is fp32 with explicit round-to-nearest intrinsics (no FMA
// contraction), corner weights are (wx*wy)*wz, corners accumulate in the order tnw,tne,tsw,tse,bnw,bne,
// bsw,bse with separate multiply and add, and out-of-range corners contribute nothing (zeros padding).
//
// Two data layouts:
//   NCDHW (reference layout): one lane per output voxel, loop over a chunk of channels.  Taps/weights are
//     computed once per voxel and reused for every channel; output stores are coalesced along x.
//   NDHWC (channels-last, internal): the C channels of a voxel are contiguous, so every corner is ONE
//     contiguous C*4-byte read (384 B for C=96) regardless of how the warp scatters neighbouring voxels --
//     each lane owns 4 channels (float4) of one voxel.  The canonical volume is repacked once per identity.
//
// The analytic variant (theta != NULL) fuses the head-pose affine of the identity lattice into the sampler
// (row a2: notebooks/infer.py:441-444, :583-588), removing the 0.79 MB grid tensor from HBM.
#include "gs3d_coord.h"
#include "gs3d_launch_form.h"

#define EMO_GS3D_TILE_FLAG (1 << 30)   /* variant bit: NCDHW -> NCDHW through the LDS-staged planar kernel (gs3d_tile.h) */

#ifndef EMO_GS3D_NT_STORES
#define EMO_GS3D_NT_STORES 0   /* A/B: non-temporal stores of the channels-last sampler output.  Measured (profiles/
                                  r3_sampler_nt_stores_ab.jsonl): the uv call itself does not change (12.8 vs 13.1 us per frame), the
                                  rotation call that reads the intermediate back in chunks of 4 frames goes from 13.1 to 17.3 us --
                                  the plain stores leave it in the Infinity Cache, the non-temporal ones do not.  Off. */
#endif
typedef float emo_f32x4 __attribute__((ext_vector_type(4)));
#ifndef EMO_GS3D_ABLATE
#define EMO_GS3D_ABLATE 0      /* timing experiments only (results are WRONG for any value != 0): 1 no corner gathers, 2 no output
                                  stores of the channels-last kernels, 4 no NCDHW stores of the rotation kernel (archive/profiles/r3_sampler_ablation.jsonl) */
#endif
#if EMO_GS3D_ABLATE & 2
#define EMO_GS3D_STORE(ptr, val)                                                                                       \
  do {                                                                                                                 \
    const float4 v_ = (val);                                                                                           \
    if (v_.x == 12345.678f) *(ptr) = v_;                                                                               \
  } while (0)
#elif EMO_GS3D_NT_STORES
#define EMO_GS3D_STORE(ptr, val)                                                                                       \
  do {                                                                                                                 \
    const float4 v_ = (val);                                                                                           \
    emo_f32x4 n_ = {v_.x, v_.y, v_.z, v_.w};                                                                          \
    __builtin_nontemporal_store(n_, reinterpret_cast<emo_f32x4*>(ptr));                                               \
  } while (0)
#else
#define EMO_GS3D_STORE(ptr, val) (*(ptr) = (val))
#endif

namespace {

struct Taps {
  int off[8];      // spatial offset (z*H + y)*W + x of each corner, 0 when the corner is out of range
  float w[8];      // corner weights, reference order tnw,tne,tsw,tse,bnw,bne,bsw,bse
  unsigned inb;    // bit k set <=> corner k is inside the volume
};

using gs3d::MODE_DELTA;
using gs3d::MODE_GRID;
using gs3d::MODE_THETA;
using gs3d::load_coord;
using gs3d::xcd_remap;

// floor corner + weights (gs3d_coord.h, bit-identical to ATen) -> per-corner offsets and the in-range mask
template <int PAD>
__device__ __forceinline__ void compute_taps(float gx, float gy, float gz, int D, int H, int W, Taps& t) {
  int x0, y0, z0;
  gs3d::corner_weights<PAD>(gx, gy, gz, D, H, W, x0, y0, z0, t.w);
  const int x1 = x0 + 1, y1 = y0 + 1, z1 = z0 + 1;
  const bool vx0 = (unsigned)x0 < (unsigned)W, vx1 = (unsigned)x1 < (unsigned)W;
  const bool vy0 = (unsigned)y0 < (unsigned)H, vy1 = (unsigned)y1 < (unsigned)H;
  const bool vz0 = (unsigned)z0 < (unsigned)D, vz1 = (unsigned)z1 < (unsigned)D;
  const bool v[8] = {vz0 && vy0 && vx0, vz0 && vy0 && vx1, vz0 && vy1 && vx0, vz0 && vy1 && vx1,
                     vz1 && vy0 && vx0, vz1 && vy0 && vx1, vz1 && vy1 && vx0, vz1 && vy1 && vx1};
  const int HW = H * W;
  const int o[8] = {z0 * HW + y0 * W + x0, z0 * HW + y0 * W + x1, z0 * HW + y1 * W + x0, z0 * HW + y1 * W + x1,
                    z1 * HW + y0 * W + x0, z1 * HW + y0 * W + x1, z1 * HW + y1 * W + x0, z1 * HW + y1 * W + x1};
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    t.off[k] = v[k] ? o[k] : 0;
    m |= v[k] ? (1u << k) : 0u;
  }
  t.inb = m;
}

// Volume of sample n in a bank (the indexed entry): one load per block -- n is uniform across it -- kept in a scalar register.
// False for an index outside [0, num_vols): the block then writes zeros and reads nothing of the bank.
__device__ __forceinline__ bool bank_volume(int n, int& vsel, const int* __restrict__ vol_index, int num_vols) {
  const int vi = __builtin_amdgcn_readfirstlane(vol_index[n]);
  vsel = vi;
  return (unsigned)vi < (unsigned)num_vols;
}

// ------------------------------------------------------------------------------------------------------
// NCDHW -> NCDHW.  grid = (ceil(nvox/256), channel chunks, N); one lane per output voxel.
// ------------------------------------------------------------------------------------------------------
// BankArgs (every sampler kernel of this file): empty, or (const int* vol_index, int num_vols) for the indexed entry
// (emo_grid_sample3d_indexed_f32) -- sample n then reads volume vol_index[n] of a bank whose volumes are vol_bstride floats apart.
// Empty, a kernel has the parameter list and code it has without a bank.
template <int PAD, int MODE, typename... BankArgs>
__global__ __launch_bounds__(256) void gs3d_ncdhw_kernel(
    const float* __restrict__ vol, const float* __restrict__ grid, const float* __restrict__ theta,
    const float* __restrict__ lin_x, const float* __restrict__ lin_y, const float* __restrict__ lin_z,
    float* __restrict__ out, int C, int D, int H, int W, int Do, int Ho, int Wo, long vol_bstride, int c_per_block, BankArgs... bank) {
  constexpr bool IDX = sizeof...(BankArgs) != 0;
  const int nvox = Do * Ho * Wo;
  const int vox = blockIdx.x * 256 + threadIdx.x;
  if (vox >= nvox) return;
  const int n = blockIdx.z;
  const int c0 = blockIdx.y * c_per_block;
  const int c1 = min(c0 + c_per_block, C);
  int vsel = n;
  if constexpr (IDX) {
    if (!bank_volume(n, vsel, bank...)) {
      float* op = out + ((long)n * C + c0) * nvox + vox;
      for (int c = c0; c < c1; ++c, op += nvox) *op = 0.0f;
      return;
    }
  }
  float gx, gy, gz;
  load_coord<MODE>(grid, theta, lin_x, lin_y, lin_z, n, vox, nvox, Ho, Wo, gx, gy, gz);
  Taps t;
  compute_taps<PAD>(gx, gy, gz, D, H, W, t);
  const long DHW = (long)D * H * W;
  const float* vp = vol + (long)vsel * vol_bstride + (long)c0 * DHW;
  float* op = out + ((long)n * C + c0) * nvox + vox;
  int c = c0;
  for (; c + 4 <= c1; c += 4) {
    float v[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k) v[j][k] = vp[j * DHW + t.off[k]];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float val = ((t.inb >> k) & 1u) ? v[j][k] : 0.0f;
        acc = __fadd_rn(acc, __fmul_rn(val, t.w[k]));
      }
      op[(long)j * nvox] = acc;
    }
    vp += 4 * DHW;
    op += 4L * nvox;
  }
  for (; c < c1; ++c) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float raw = vp[t.off[k]];
      const float val = ((t.inb >> k) & 1u) ? raw : 0.0f;
      acc = __fadd_rn(acc, __fmul_rn(val, t.w[k]));
    }
    op[0] = acc;
    vp += DHW;
    op += nvox;
  }
}

// ------------------------------------------------------------------------------------------------------
// v2 channels-last kernels: taps are computed ONCE per voxel (64 voxels per block, one lane each), parked in
// LDS, and every (voxel, channel-quad) item then only does: 5 broadcast LDS reads, 8 x 16-byte gathers,
// 64 mul/add.  v1 recomputed the ~150-instruction tap math in each of the C/4 lanes of a voxel and was
// VALU-bound (15 us/sample vs a 5 us L1-bandwidth bound).  Out-of-range corners are handled by a wave-uniform
// branch: the common all-in-range wave takes a path with no per-component selects.
// ------------------------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) TapRec {
  int off[8];
  float w[8];
  unsigned inb;
  unsigned pad[3];
};
// Block order of one launch.  ORDER 1: XCD-contiguous (gs3d::xcd_remap: block b runs on XCD b % 8, each XCD has a private
// 4 MiB L2; remapped, XCD k walks one contiguous eighth of the (sample, z, y, x) ordered work, so a corner row is fetched
// once and re-used out of that XCD's L2 by the following rows and the next z-slice).  ORDER 3: XCD-contiguous AND, inside an
// XCD's share, (z-slice, group of 8 blocks, sample, block in group) -- needs N % 8 == 0: when N driver frames sample ONE
// shared canonical volume with near-identity warps, a group's corner rows (a few hundred KB of the shared volume) stay in
// L2 while all of the XCD's samples pass over them.  (Other orders, 128 / 256 voxels per block, the first-generation
// kernels and the channel-group-per-XCD layout were measured in rounds 1-2 and retired: DESIGN.md section 3.2.)
template <int ORDER>
__device__ __forceinline__ void block_to_work(int b, int total, int bps, int nslices, int& n, int& blk) {
  constexpr int G = 8;                          // blocks (= output rows at Wo = 64) per row group
  if (ORDER == 1) { const int L = xcd_remap(b, total); n = L / bps; blk = L - n * bps; return; }
  const int xcd = b & 7, idx = b >> 3;
  const int spx = (total / bps) >> 3;          // samples per XCD
  const int per_group = spx * G;
  const int grp = idx / per_group;              // global group index = z * (bpz / G) + row group
  const int rem = idx - grp * per_group;
  const int j = rem / G;
  n = xcd * spx + j;
  blk = grp * G + (rem - j * G);
}

// voxel i (0..63) of 4x4x4 brick `blk` of a Do x Ho x Wo output lattice (all three multiples of 4): bricks x-fastest
__device__ __forceinline__ int brick_voxel(int blk, int i, int Ho, int Wo) {
  const int bw = Wo >> 2, bh = Ho >> 2;
  const int bx = blk % bw;
  const int t = blk / bw;
  const int by = t % bh, bz = t / bh;
  return (((bz << 2) + (i >> 4)) * Ho + (by << 2) + ((i >> 2) & 3)) * Wo + (bx << 2) + (i & 3);
}

// BRICK: the block's voxels are a 4x4x4 brick (vox0 = brick index) instead of VPB consecutive voxels
template <int PAD, int MODE, int VPB, bool BRICK = false>
__device__ __forceinline__ void stage_taps(TapRec* __restrict__ recs, const float* __restrict__ grid,
                                           const float* __restrict__ theta, const float* __restrict__ lin_x,
                                           const float* __restrict__ lin_y, const float* __restrict__ lin_z, int n,
                                           int vox0, int nvox, int D, int H, int W, int Ho, int Wo) {
  for (int i = threadIdx.x; i < VPB; i += 256) {
    const int vox = BRICK ? brick_voxel(vox0, i, Ho, Wo) : vox0 + i;
    Taps t;
    if (vox < nvox) {
      float gx, gy, gz;
      load_coord<MODE>(grid, theta, lin_x, lin_y, lin_z, n, vox, nvox, Ho, Wo, gx, gy, gz);
      compute_taps<PAD>(gx, gy, gz, D, H, W, t);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) { t.off[k] = 0; t.w[k] = 0.0f; }
      t.inb = 0;
    }
    TapRec r;
#pragma unroll
    for (int k = 0; k < 8; ++k) { r.off[k] = t.off[k]; r.w[k] = t.w[k]; }
    r.inb = t.inb; r.pad[0] = r.pad[1] = r.pad[2] = 0;
    recs[i] = r;
  }
}

// FMA (variant bit 4 of the channels-last kernels, opt-in): coordinates, floor, corner indices and the eight weights are the
// same bit-exact arithmetic; only the accumulation changes from ATen's separate multiply and add per corner (64 VALU
// instructions per item) to acc = fma(v, w, acc) in packed form (16 v_pk_fma_f32).  Values then differ from ATen's CPU kernel
// by the product roundings that are skipped: <= 8 * 2^-24 * max |v w| absolute (tests/test_grid_sample_gpu.py).
typedef float emo_f2 __attribute__((ext_vector_type(2)));
template <bool FMA = false>
__device__ __forceinline__ float4 gather_quad(const char* __restrict__ vbytes, const TapRec& r, unsigned row_bytes,
                                              unsigned qbyte) {
  float4 v[8];
#if EMO_GS3D_ABLATE & 1     /* timing experiment (wrong results): no corner gathers */
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = make_float4(r.w[k], r.w[(k + 1) & 7], (float)r.off[k], (float)qbyte);
#else
#pragma unroll
  for (int k = 0; k < 8; ++k)
    v[k] = *reinterpret_cast<const float4*>(vbytes + ((unsigned)r.off[k] * row_bytes + qbyte));
#endif
  if constexpr (FMA) {
    emo_f2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
    if (__all(r.inb == 0xffu)) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const emo_f2 w2 = {r.w[k], r.w[k]};
        a01 = __builtin_elementwise_fma(emo_f2{v[k].x, v[k].y}, w2, a01);
        a23 = __builtin_elementwise_fma(emo_f2{v[k].z, v[k].w}, w2, a23);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bool in = (r.inb >> k) & 1u;
        const emo_f2 w2 = {r.w[k], r.w[k]};
        a01 = __builtin_elementwise_fma(emo_f2{in ? v[k].x : 0.0f, in ? v[k].y : 0.0f}, w2, a01);
        a23 = __builtin_elementwise_fma(emo_f2{in ? v[k].z : 0.0f, in ? v[k].w : 0.0f}, w2, a23);
      }
    }
    return make_float4(a01[0], a01[1], a23[0], a23[1]);
  }
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  // wave-uniform: does every lane of this wave have all 8 corners in range?
  if (__all(r.inb == 0xffu)) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float w = r.w[k];
      acc.x = __fadd_rn(acc.x, __fmul_rn(v[k].x, w));
      acc.y = __fadd_rn(acc.y, __fmul_rn(v[k].y, w));
      acc.z = __fadd_rn(acc.z, __fmul_rn(v[k].z, w));
      acc.w = __fadd_rn(acc.w, __fmul_rn(v[k].w, w));
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool in = (r.inb >> k) & 1u;
      const float w = r.w[k];
      acc.x = __fadd_rn(acc.x, __fmul_rn(in ? v[k].x : 0.0f, w));
      acc.y = __fadd_rn(acc.y, __fmul_rn(in ? v[k].y : 0.0f, w));
      acc.z = __fadd_rn(acc.z, __fmul_rn(in ? v[k].z : 0.0f, w));
      acc.w = __fadd_rn(acc.w, __fmul_rn(in ? v[k].w : 0.0f, w));
    }
  }
  return acc;
}

// (voxel, quad) of item = threadIdx.x + 256 * k without a division per item: the runtime divisor LPV = C / 4 costs ~25 VALU
// instructions per division, a third of an item's instruction count (the kernels' arithmetic skeleton is 40 % of their time,
// archive/profiles/r3_sampler_ablation.jsonl); one division per thread, then (v, q) advance by (256 / LPV, 256 % LPV) with a carry
struct ItemWalk {
  int v, q, dv, dq, lpv;
  __device__ __forceinline__ ItemWalk(int tid, int LPV) : lpv(LPV) {
    v = tid / LPV; q = tid - v * LPV;
    dv = 256 / LPV; dq = 256 - dv * LPV;
  }
  __device__ __forceinline__ void next() {
    v += dv; q += dq;
    if (q >= lpv) { q -= lpv; ++v; }
  }
};

// NDHWC -> NDHWC, 1-D grid of N * ceil(nvox/VPB) blocks
template <int PAD, int MODE, int VPB, int ORDER, bool FMA, typename... BankArgs>
__global__ __launch_bounds__(256) void gs3d_cl_v2_kernel(
    const float* __restrict__ vol, const float* __restrict__ grid, const float* __restrict__ theta,
    const float* __restrict__ lin_x, const float* __restrict__ lin_y, const float* __restrict__ lin_z,
    float* __restrict__ out, int C, int D, int H, int W, int Do, int Ho, int Wo, long vol_bstride, int bps, BankArgs... bank) {
  constexpr bool IDX = sizeof...(BankArgs) != 0;
  __shared__ TapRec recs[VPB];
  const int LPV = C >> 2;
  const int nvox = Do * Ho * Wo;
  int n, blk;
  block_to_work<ORDER>(blockIdx.x, gridDim.x, bps, Do, n, blk);
  const int vox0 = blk * VPB;
  int vsel = n;
  if constexpr (IDX) {
    if (!bank_volume(n, vsel, bank...)) {
      const int nitems = min(VPB, nvox - vox0) * LPV;
      float4* obase = reinterpret_cast<float4*>(out) + ((long)n * nvox + vox0) * LPV;
      for (int item = threadIdx.x; item < nitems; item += 256) obase[item] = make_float4(0.f, 0.f, 0.f, 0.f);
      return;
    }
  }
  stage_taps<PAD, MODE, VPB>(recs, grid, theta, lin_x, lin_y, lin_z, n, vox0, nvox, D, H, W, Ho, Wo);
  __syncthreads();
  const char* vbytes = reinterpret_cast<const char*>(vol + (long)vsel * vol_bstride);
  const unsigned row_bytes = (unsigned)C * 4u;
  const int nitems = min(VPB, nvox - vox0) * LPV;
  float4* obase = reinterpret_cast<float4*>(out) + ((long)n * nvox + vox0) * LPV;
  ItemWalk w(threadIdx.x, LPV);
  for (int item = threadIdx.x; item < nitems; item += 256, w.next()) {
    const TapRec r = recs[w.v];
    EMO_GS3D_STORE(&obase[item], gather_quad<FMA>(vbytes, r, row_bytes, (unsigned)w.q * 16u));
  }
}

// NDHWC -> NDHWC with 4x4x4 output bricks per block: the 8 corners of a brick's 64 voxels fall into ~5x5x5 source voxels
// (48 KB at C = 96) instead of the 2x2x65 of an x-row (100 KB): half the L1 fills per output voxel.  The samplers are
// bound by the per-CU L1 path (64-byte granules per clock + outstanding-miss capacity), not by L2 or HBM
// (archive/profiles/r2_pmc_sampler_*.json), so fewer fills per voxel is the lever.  Needs Do, Ho, Wo multiples of 4.
template <int PAD, int MODE, int ORDER, typename... BankArgs>
__global__ __launch_bounds__(256) void gs3d_cl_brick_kernel(
    const float* __restrict__ vol, const float* __restrict__ grid, const float* __restrict__ theta,
    const float* __restrict__ lin_x, const float* __restrict__ lin_y, const float* __restrict__ lin_z,
    float* __restrict__ out, int C, int D, int H, int W, int Do, int Ho, int Wo, long vol_bstride, int bps, BankArgs... bank) {
  constexpr bool IDX = sizeof...(BankArgs) != 0;
  __shared__ TapRec recs[64];
  __shared__ int vox_of[64];
  const int LPV = C >> 2;
  const int nvox = Do * Ho * Wo;
  int n, blk;
  block_to_work<ORDER>(blockIdx.x, gridDim.x, bps, Do >> 2, n, blk);
  int vsel = n;
  if constexpr (IDX) {
    if (!bank_volume(n, vsel, bank...)) {
      float4* obase = reinterpret_cast<float4*>(out) + (long)n * nvox * LPV;
      ItemWalk w(threadIdx.x, LPV);
      for (int item = threadIdx.x; item < 64 * LPV; item += 256, w.next())
        obase[(long)brick_voxel(blk, w.v, Ho, Wo) * LPV + w.q] = make_float4(0.f, 0.f, 0.f, 0.f);
      return;
    }
  }
  stage_taps<PAD, MODE, 64, true>(recs, grid, theta, lin_x, lin_y, lin_z, n, blk, nvox, D, H, W, Ho, Wo);
  if (threadIdx.x < 64) vox_of[threadIdx.x] = brick_voxel(blk, threadIdx.x, Ho, Wo);
  __syncthreads();
  const char* vbytes = reinterpret_cast<const char*>(vol + (long)vsel * vol_bstride);
  const unsigned row_bytes = (unsigned)C * 4u;
  float4* obase = reinterpret_cast<float4*>(out) + (long)n * nvox * LPV;
  ItemWalk w(threadIdx.x, LPV);
  for (int item = threadIdx.x; item < 64 * LPV; item += 256, w.next()) {
    const TapRec r = recs[w.v];
    EMO_GS3D_STORE(&obase[(long)vox_of[w.v] * LPV + w.q], gather_quad(vbytes, r, row_bytes, (unsigned)w.q * 16u));
  }
}

// NDHWC -> NCDHW, 1-D grid; dynamic LDS = VPB tap records + C * (VPB + 1) floats (transpose tile)
template <int PAD, int MODE, int VPB, int ORDER, bool FMA, typename... BankArgs>
__global__ __launch_bounds__(256) void gs3d_cl2ncdhw_v2_kernel(
    const float* __restrict__ vol, const float* __restrict__ grid, const float* __restrict__ theta,
    const float* __restrict__ lin_x, const float* __restrict__ lin_y, const float* __restrict__ lin_z,
    float* __restrict__ out, int C, int D, int H, int W, int Do, int Ho, int Wo, long vol_bstride, int bps, int nt_out, BankArgs... bank) {
  constexpr bool IDX = sizeof...(BankArgs) != 0;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  TapRec* recs = reinterpret_cast<TapRec*>(smem);                 // VPB * 80 B
  float* tile = smem + VPB * (sizeof(TapRec) / 4);                 // [C][VPB + 1]
  constexpr int LD = VPB + 1;
  const int LPV = C >> 2;
  const int nvox = Do * Ho * Wo;
  int n, blk;
  block_to_work<ORDER>(blockIdx.x, gridDim.x, bps, Do, n, blk);
  const int vox0 = blk * VPB;
  int vsel = n;
  if constexpr (IDX) {
    if (!bank_volume(n, vsel, bank...)) {
      const int nv = min(VPB, nvox - vox0);
      float* obase = out + (long)n * C * nvox + vox0;
      for (int i = threadIdx.x; i < C * VPB; i += 256) {
        const int c = i / VPB;
        const int v = i - c * VPB;
        if (v < nv) obase[(long)c * nvox + v] = 0.0f;
      }
      return;
    }
  }
  stage_taps<PAD, MODE, VPB>(recs, grid, theta, lin_x, lin_y, lin_z, n, vox0, nvox, D, H, W, Ho, Wo);
  __syncthreads();
  const char* vbytes = reinterpret_cast<const char*>(vol + (long)vsel * vol_bstride);
  const unsigned row_bytes = (unsigned)C * 4u;
  const int nv = min(VPB, nvox - vox0);
  const int nitems = nv * LPV;
  ItemWalk w(threadIdx.x, LPV);
  for (int item = threadIdx.x; item < nitems; item += 256, w.next()) {
    const int v = w.v, q = w.q;
    const TapRec r = recs[v];
    const float4 acc = gather_quad<FMA>(vbytes, r, row_bytes, (unsigned)q * 16u);
    const int c = q * 4;
    tile[(c + 0) * LD + v] = acc.x;
    tile[(c + 1) * LD + v] = acc.y;
    tile[(c + 2) * LD + v] = acc.z;
    tile[(c + 3) * LD + v] = acc.w;
  }
  __syncthreads();
  float* obase = out + (long)n * C * nvox + vox0;
  for (int i = threadIdx.x; i < C * VPB; i += 256) {
    const int c = i / VPB;
    const int v = i - c * VPB;
    if (v < nv && (!(EMO_GS3D_ABLATE & 4) || tile[c * LD + v] == 12345.678f)) {
      // nt_out: the NCDHW result is streamed past the caches -- in the driver pass it is read much later (by the decoder),
      // while the Infinity Cache is what serves the intermediate of the sampler pair (measured: pair - 5 % at chunks of 4)
      if (nt_out) __builtin_nontemporal_store(tile[c * LD + v], &obase[(long)c * nvox + v]);
      else obase[(long)c * nvox + v] = tile[c * LD + v];
    }
  }
}

constexpr int CL_VPB = 64;      // output voxels per block of the row-shaped kernels

// The volume bank of the indexed entry: sample n reads volume index[n] of `num`.  index == nullptr: the plain entry (kernels with
// an empty BankArgs); with a bank their (const int*, int) instantiations run, in the same block order.
struct Bank {
  const int* index;
  int num;
};

// ------------------------------------------------------------------------------------------------------
// The launch decision of the direct kernels (ABI 29), made HERE and nowhere else: `launch` calls it and launches what it says,
// emo_grid_sample3d_launch_form reports it.  No HIP call.
//
// NCDHW -> NCDHW: the planar gather, variant = channels per block (0: 8), clipped to C.
// NDHWC -> NDHWC / NCDHW, variant word (bits): 1 = 4 x 4 x 4 output bricks per block instead of 64-voxel rows (NDHWC output,
// Do / Ho / Wo multiples of 4; otherwise the bit is ignored): half the L1 fills per voxel, the uv call alone 11.7 instead of
// 12.3 us per frame -- but the rotation call that reads its output back is then 0.6-0.8 us slower (its blocks walk the volume in
// row order), so the pair is 1.3 us per frame slower: opt-in.  The brick kernel has no FMA form: bit 1 wins over bit 4.
// 2 = non-temporal stores of an NCDHW output (the driver pass's rotation call); ignored for an NDHWC output.
// 4 = fused multiply-add accumulation (gather_quad<true>: taps bit-identical, values within 8 * 2^-24 * max|v w| of ATen).
// Default: 64-voxel rows, XCD-contiguous (ORDER 1), and for a volume shared by N >= 8 samples (no bank) row-group-major over the
// XCD's samples (ORDER 3) where the work divides into whole slices and groups: N % 8 == 0, nvox % 64 == 0, bps % Do == 0 and
// (bps / Do) % 8 == 0 -- otherwise ORDER 1.  (archive/profiles/r3_sampler_nt_stores_ab.jsonl, r3_sampler_nt_out_ab.jsonl)
// ------------------------------------------------------------------------------------------------------
gs3d::LaunchForm direct_form(int N, int C, int D, int H, int W, int Do, int Ho, int Wo, long vol_bstride, int in_layout,
                             int out_layout, int variant, bool banked) {
  gs3d::LaunchForm f = {};
  auto refuse = [&f](int rc) { f = gs3d::LaunchForm{}; f.rc = rc; return f; };
  const int nvox = Do * Ho * Wo;
  f.bank = banked;
  f.gy = f.gz = 1;
  if (in_layout == EMO_LAYOUT_NCDHW && out_layout == EMO_LAYOUT_NCDHW) {
    int cpb = variant > 0 ? variant : 8;
    if (cpb > C) cpb = C;
    f.form = EMO_GS3D_FORM_PLANAR;
    f.cpb = cpb;
    f.bps = emo_cdiv(nvox, 256);
    f.gx = f.bps; f.gy = emo_cdiv(C, cpb); f.gz = N;
    f.last_vox = nvox - (int)(f.bps - 1) * 256;
    return f;
  }
  if (in_layout != EMO_LAYOUT_NDHWC || (out_layout != EMO_LAYOUT_NDHWC && out_layout != EMO_LAYOUT_NCDHW))
    return refuse(EMO_ERR_UNSUPPORTED);
  if (C % 4) return refuse(EMO_ERR_UNSUPPORTED);
  if ((long)D * H * W * C * 4 >= (1L << 32)) return refuse(EMO_ERR_UNSUPPORTED);   // 32-bit byte offsets
  if (variant < 0 || variant > 7) return refuse(EMO_ERR_BAD_ARG);
  const bool out_cl = out_layout == EMO_LAYOUT_NDHWC;
  f.cpb = C;
  f.order = 1;
  if ((variant & 1) && out_cl && !(Do & 3) && !(Ho & 3) && !(Wo & 3)) {
    f.form = EMO_GS3D_FORM_BRICK;
    f.bps = nvox >> 6;
    f.last_vox = 64;
  } else {
    f.form = out_cl ? EMO_GS3D_FORM_ROWS : EMO_GS3D_FORM_ROWS_NCDHW;
    f.fma = (variant & 4) != 0;
    f.nt = (variant & 2) && !out_cl;
    f.bps = emo_cdiv(nvox, CL_VPB);
    f.last_vox = nvox - (int)(f.bps - 1) * CL_VPB;
    const bool shared = vol_bstride == 0 && !banked;
    if (shared && N >= 8 && !(N & 7) && !(nvox % CL_VPB) && !(f.bps % Do) && !((f.bps / Do) % 8)) f.order = 3;
    if (!out_cl) {
      f.lds = CL_VPB * sizeof(TapRec) + (size_t)C * (CL_VPB + 1) * sizeof(float);
      if (f.lds > 64 * 1024) return refuse(EMO_ERR_UNSUPPORTED);
    }
  }
  if (f.bps * N > 0x7fffffffL) return refuse(EMO_ERR_UNSUPPORTED);
  f.gx = f.bps * N;
  return f;
}

// the row-shaped channels-last kernels in the block order and accumulation `f` names (a bank never gets ORDER 3: direct_form)
template <int PAD, int MODE, int ORDER, bool FMA>
void run_rows(const gs3d::LaunchForm& f, const float* vol, const float* grid, const float* theta, const float* lin_x,
              const float* lin_y, const float* lin_z, float* out, int C, int D, int H, int W, int Do, int Ho, int Wo,
              long vol_bstride, hipStream_t s, Bank bank) {
  const bool out_cl = f.form == EMO_GS3D_FORM_ROWS;
  const dim3 g((unsigned)f.gx);
  const int bps = (int)f.bps;
  if constexpr (ORDER == 1) {
    if (bank.index) {
      if (out_cl)
        hipLaunchKernelGGL((gs3d_cl_v2_kernel<PAD, MODE, CL_VPB, ORDER, FMA, const int*, int>), g, dim3(256), 0, s, vol, grid,
                           theta, lin_x, lin_y, lin_z, out, C, D, H, W, Do, Ho, Wo, vol_bstride, bps, bank.index, bank.num);
      else
        hipLaunchKernelGGL((gs3d_cl2ncdhw_v2_kernel<PAD, MODE, CL_VPB, ORDER, FMA, const int*, int>), g, dim3(256), f.lds, s,
                           vol, grid, theta, lin_x, lin_y, lin_z, out, C, D, H, W, Do, Ho, Wo, vol_bstride, bps, f.nt, bank.index,
                           bank.num);
      return;
    }
  }
  if (out_cl)
    hipLaunchKernelGGL((gs3d_cl_v2_kernel<PAD, MODE, CL_VPB, ORDER, FMA>), g, dim3(256), 0, s, vol, grid, theta, lin_x, lin_y,
                       lin_z, out, C, D, H, W, Do, Ho, Wo, vol_bstride, bps);
  else
    hipLaunchKernelGGL((gs3d_cl2ncdhw_v2_kernel<PAD, MODE, CL_VPB, ORDER, FMA>), g, dim3(256), f.lds, s, vol, grid, theta, lin_x,
                       lin_y, lin_z, out, C, D, H, W, Do, Ho, Wo, vol_bstride, bps, f.nt);
}

// ------------------------------------------------------------------------------------------------------
// layout repack [N][C][S] <-> [N][S][C] through a 64x64 LDS tile
// ------------------------------------------------------------------------------------------------------
// RowArgs: empty, or (const int* row, int num_rows) for the indexed entry (emo_volume_repack_indexed_f32) -- matrix n is then
// written to matrix row[n] of the output bank, and a row outside [0, num_rows) writes nothing.  Empty, the kernel has the
// parameter list and code it has without rows.
template <typename... RowArgs>
__global__ __launch_bounds__(256) void repack_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                     int R, int Ccols, RowArgs... rows) {
  // in: [n][R][Ccols] -> out: [n][Ccols][R]
  __shared__ float tile[64][65];
  const int n = blockIdx.z;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const float* ip = in + (long)n * R * Ccols;
  float* op = out + (long)n * R * Ccols;
  if constexpr (sizeof...(RowArgs) != 0) {
    int rsel;
    if (!bank_volume(n, rsel, rows...)) return;        // uniform over the block: no barrier is skipped by part of it
    op = out + (long)rsel * R * Ccols;                  // 64-bit row base: a bank of R512 slots passes 2^31 floats
  }
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int r = r0 + i, c = c0 + tx;
    if (r < R && c < Ccols) tile[i][tx] = ip[(long)r * Ccols + c];
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int c = c0 + i, r = r0 + tx;
    if (r < R && c < Ccols) op[(long)c * R + r] = tile[tx][i];
  }
}

// executes a form direct_form decided (f.rc == EMO_OK)
template <int PAD, int MODE>
int launch(const gs3d::LaunchForm& f, const float* vol, const float* grid, const float* theta, const float* lin_x,
           const float* lin_y, const float* lin_z, float* out, int C, int D, int H, int W, int Do, int Ho, int Wo,
           long vol_bstride, hipStream_t s, Bank bank) {
#define EMO_GS3D_ROWS(ORDER, FMA) \
  run_rows<PAD, MODE, ORDER, FMA>(f, vol, grid, theta, lin_x, lin_y, lin_z, out, C, D, H, W, Do, Ho, Wo, vol_bstride, s, bank)
  if (f.form == EMO_GS3D_FORM_PLANAR) {
    const dim3 g((unsigned)f.gx, f.gy, f.gz);
    if (bank.index)
      hipLaunchKernelGGL((gs3d_ncdhw_kernel<PAD, MODE, const int*, int>), g, dim3(256), 0, s, vol, grid, theta, lin_x, lin_y, lin_z,
                         out, C, D, H, W, Do, Ho, Wo, vol_bstride, f.cpb, bank.index, bank.num);
    else
      hipLaunchKernelGGL((gs3d_ncdhw_kernel<PAD, MODE>), g, dim3(256), 0, s, vol, grid, theta, lin_x, lin_y, lin_z,
                         out, C, D, H, W, Do, Ho, Wo, vol_bstride, f.cpb);
  } else if (f.form == EMO_GS3D_FORM_BRICK) {
    if (bank.index)
      hipLaunchKernelGGL((gs3d_cl_brick_kernel<PAD, MODE, 1, const int*, int>), dim3((unsigned)f.gx), dim3(256), 0, s, vol, grid, theta,
                         lin_x, lin_y, lin_z, out, C, D, H, W, Do, Ho, Wo, vol_bstride, (int)f.bps, bank.index, bank.num);
    else
      hipLaunchKernelGGL((gs3d_cl_brick_kernel<PAD, MODE, 1>), dim3((unsigned)f.gx), dim3(256), 0, s, vol, grid, theta, lin_x,
                         lin_y, lin_z, out, C, D, H, W, Do, Ho, Wo, vol_bstride, (int)f.bps);
  } else if (f.order == 3) {
    if (f.fma) EMO_GS3D_ROWS(3, true); else EMO_GS3D_ROWS(3, false);
  } else {
    if (f.fma) EMO_GS3D_ROWS(1, true); else EMO_GS3D_ROWS(1, false);
  }
#undef EMO_GS3D_ROWS
  return emo_launch_status();
}

// ------------------------------------------------------------------------------------------------------
// The rotation warp itself (row a2): grid[n,z,y,x,:] = theta[n,:3,:4] . (u_x, v_y, w_z, 1) -- exactly the coordinates
// the MODE_THETA samplers generate on the fly, materialised for callers that want the reference's cached
// `source_rotation_warp` tensor (notebooks/infer.py:441-444) and for the parity tests that compare them with the
// reference's `identity_grid_3d.bmm(theta[:, :3].transpose(1, 2))`.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void affine_grid3d_kernel(const float* __restrict__ theta,
                                                            const float* __restrict__ lin_x,
                                                            const float* __restrict__ lin_y,
                                                            const float* __restrict__ lin_z, float* __restrict__ grid,
                                                            int Do, int Ho, int Wo) {
  const int nvox = Do * Ho * Wo;
  const int vox = blockIdx.x * 256 + threadIdx.x;
  if (vox >= nvox) return;
  const int n = blockIdx.y;
  float gx, gy, gz;
  load_coord<MODE_THETA>(nullptr, theta, lin_x, lin_y, lin_z, n, vox, nvox, Ho, Wo, gx, gy, gz);
  float* g = grid + ((long)n * nvox + vox) * 3;
  g[0] = gx; g[1] = gy; g[2] = gz;
}

template <int PAD>
int launch_pad(const gs3d::LaunchForm& f, const float* vol, const float* grid, const float* theta, const float* lin_x,
               const float* lin_y, const float* lin_z, float* out, int C, int D, int H, int W, int Do, int Ho, int Wo,
               long vol_bstride, int grid_kind, hipStream_t s, Bank bank) {
  if (theta)
    return launch<PAD, MODE_THETA>(f, vol, grid, theta, lin_x, lin_y, lin_z, out, C, D, H, W, Do, Ho, Wo, vol_bstride, s, bank);
  if (grid_kind == 1)
    return launch<PAD, MODE_DELTA>(f, vol, grid, theta, lin_x, lin_y, lin_z, out, C, D, H, W, Do, Ho, Wo, vol_bstride, s, bank);
  return launch<PAD, MODE_GRID>(f, vol, grid, theta, lin_x, lin_y, lin_z, out, C, D, H, W, Do, Ho, Wo, vol_bstride, s, bank);
}

}  // namespace

int emo_gs3d_tile_dispatch(const float* vol, const float* grid, const float* theta, const float* lin_x, const float* lin_y,
                           const float* lin_z, float* out, int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                           int64_t vol_batch_stride, int padding_mode, int in_layout, int out_layout, int variant,
                           int grid_kind, void* stream);
int emo_repack_p4_dispatch(const float* in, float* out, int N, int C, int DHW, int to_p4, void* stream);
// The decisions the launchers behind the two dispatchers make for these arguments (gs3d_tile_api.hip; tile_form of
// gs3d_tile_launch.h), nothing launched.  Weak references: a build of this file alone whose dispatchers are stubs that refuse
// (the host-compiled test library) need not define them -- absent, the answer is the stubs': EMO_ERR_UNSUPPORTED.
__attribute__((weak)) int emo_gs3d_tile_form(int N, int C, int D, int H, int W, int Do, int Ho, int Wo, int in_layout,
                                             int out_layout, int variant, gs3d::LaunchForm* form);
__attribute__((weak)) int emo_repack_p4_form(int N, int C, int DHW, long* blocks);

namespace {

// What a sampler call does before any launch, from the argument checks to the kernel and its plan: sample3d calls it and launches
// what it says, emo_grid_sample3d_launch_form reports it.  kind: EMO_GS3D_KIND_* (grid, delta, theta).  *tile: the LDS-staged
// kernels take the call (emo_gs3d_tile_dispatch), else the direct kernels of this file.
gs3d::LaunchForm sampler_form(const void* vol, const void* out, int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                              int64_t vol_batch_stride, int padding_mode, int in_layout, int out_layout, int variant, int kind,
                              bool banked, bool* tile) {
  gs3d::LaunchForm f = {};
  *tile = false;
  auto refuse = [&f](int rc) { f = gs3d::LaunchForm{}; f.rc = rc; return f; };
  if (!vol || !out) return refuse(EMO_ERR_BAD_ARG);
  if (kind != EMO_GS3D_KIND_GRID && kind != EMO_GS3D_KIND_DELTA && kind != EMO_GS3D_KIND_THETA) return refuse(EMO_ERR_BAD_ARG);
  if (N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0) return refuse(EMO_ERR_BAD_ARG);
  if (vol_batch_stride < 0) return refuse(EMO_ERR_BAD_ARG);
  if (N > 65535) return refuse(EMO_ERR_UNSUPPORTED);
  if ((long)D * H * W >= (1L << 31) / 4 || (long)Do * Ho * Wo >= (1L << 31) / 4) return refuse(EMO_ERR_UNSUPPORTED);
  if (!emo_aligned16(vol) || !emo_aligned16(out)) return refuse(EMO_ERR_ALIGN);
  if (banked && (in_layout == EMO_LAYOUT_P4 || (variant & EMO_GS3D_TILE_FLAG))) return refuse(EMO_ERR_UNSUPPORTED);
  if (padding_mode != EMO_PAD_ZEROS && padding_mode != EMO_PAD_BORDER && padding_mode != EMO_PAD_REFLECTION)
    return refuse(EMO_ERR_BAD_ARG);
  const bool planar = in_layout == EMO_LAYOUT_NCDHW && out_layout == EMO_LAYOUT_NCDHW;
  if (in_layout == EMO_LAYOUT_P4 || (planar && (variant & EMO_GS3D_TILE_FLAG))) {
    if (emo_gs3d_tile_form) emo_gs3d_tile_form(N, C, D, H, W, Do, Ho, Wo, in_layout, out_layout, variant & ~EMO_GS3D_TILE_FLAG, &f);
    else f.rc = EMO_ERR_UNSUPPORTED;
    // LDS-staged planar kernel; shapes it does not take (W % 4, huge extents) fall through to the direct-gather kernel
    if (in_layout == EMO_LAYOUT_P4 || f.rc != EMO_ERR_UNSUPPORTED) {
      *tile = f.rc == EMO_OK;
      return f.rc == EMO_OK ? f : refuse(f.rc);
    }
    variant = 0;
  }
  return direct_form(N, C, D, H, W, Do, Ho, Wo, (long)vol_batch_stride, in_layout, out_layout, variant, banked);
}

int sample3d(const float* vol, const float* grid, const float* theta, const float* lin_x, const float* lin_y, const float* lin_z,
             float* out, int N, int C, int D, int H, int W, int Do, int Ho, int Wo, int64_t vol_batch_stride, int padding_mode,
             int in_layout, int out_layout, int variant, int grid_kind, void* stream, Bank bank) {
  if (!vol || !out || (!grid && !theta)) return EMO_ERR_BAD_ARG;
  if (grid_kind != 0 && grid_kind != 1) return EMO_ERR_BAD_ARG;
  if ((theta || grid_kind == 1) && (!lin_x || !lin_y || !lin_z)) return EMO_ERR_BAD_ARG;
  if (theta && grid_kind == 1) return EMO_ERR_BAD_ARG;
  bool tile;
  const gs3d::LaunchForm f = sampler_form(vol, out, N, C, D, H, W, Do, Ho, Wo, vol_batch_stride, padding_mode, in_layout, out_layout,
                                          variant, theta ? EMO_GS3D_KIND_THETA : grid_kind, bank.index != nullptr, &tile);
  if (f.rc != EMO_OK) return f.rc;
  if (tile)
    return emo_gs3d_tile_dispatch(vol, grid, theta, lin_x, lin_y, lin_z, out, N, C, D, H, W, Do, Ho, Wo, vol_batch_stride,
                                  padding_mode, in_layout, out_layout, variant & ~EMO_GS3D_TILE_FLAG, grid_kind, stream);
  hipStream_t s = (hipStream_t)stream;
  switch (padding_mode) {
    case EMO_PAD_ZEROS:
      return launch_pad<EMO_PAD_ZEROS>(f, vol, grid, theta, lin_x, lin_y, lin_z, out, C, D, H, W, Do, Ho, Wo, vol_batch_stride,
                                       grid_kind, s, bank);
    case EMO_PAD_BORDER:
      return launch_pad<EMO_PAD_BORDER>(f, vol, grid, theta, lin_x, lin_y, lin_z, out, C, D, H, W, Do, Ho, Wo, vol_batch_stride,
                                        grid_kind, s, bank);
    default:
      return launch_pad<EMO_PAD_REFLECTION>(f, vol, grid, theta, lin_x, lin_y, lin_z, out, C, D, H, W, Do, Ho, Wo,
                                            vol_batch_stride, grid_kind, s, bank);
  }
}

// The launch decision of the two repack entries: `dir` is an EMO_REPACK_*; grid (g[0], g[1], g[2]).  No HIP call.
int repack_form(const void* in, const void* out, int N, int C, int DHW, int to_channels_last, bool indexed, int* dir, long* g) {
  *dir = 0; g[0] = g[1] = g[2] = 0;
  if (!in || !out || N <= 0 || C <= 0 || DHW <= 0) return EMO_ERR_BAD_ARG;
  if (N > 65535) return EMO_ERR_UNSUPPORTED;
  if (!indexed && (to_channels_last == 4 || to_channels_last == 5)) {     // NCDHW <-> packed-4
    const int rc = emo_repack_p4_form ? emo_repack_p4_form(N, C, DHW, &g[0]) : EMO_ERR_UNSUPPORTED;
    if (rc != EMO_OK) { g[0] = 0; return rc; }
    *dir = to_channels_last == 4 ? EMO_REPACK_TO_P4 : EMO_REPACK_FROM_P4;
    g[1] = N; g[2] = 1;
    return EMO_OK;
  }
  if (indexed ? to_channels_last != 1 : (to_channels_last != 0 && to_channels_last != 1)) return EMO_ERR_BAD_ARG;
  const int R = to_channels_last ? C : DHW;       // rows of the input matrix
  const int Ccols = to_channels_last ? DHW : C;   // columns of the input matrix
  if (emo_cdiv(R, 64) > 65535) return EMO_ERR_UNSUPPORTED;     // grid y
  *dir = indexed ? EMO_REPACK_TO_CHANNELS_LAST_INDEXED : to_channels_last ? EMO_REPACK_TO_CHANNELS_LAST : EMO_REPACK_FROM_CHANNELS_LAST;
  g[0] = emo_cdiv(Ccols, 64); g[1] = emo_cdiv(R, 64); g[2] = N;
  return EMO_OK;
}

}  // namespace

// ABI 29 (definition: include/emo_hip.h): the kernel and plan a sampler call with these arguments takes; nothing is launched
extern "C" int emo_grid_sample3d_launch_form(const void* vol, const void* out, int banked, int N, int C, int D, int H, int W,
                                             int Do, int Ho, int Wo, int64_t vol_batch_stride, int padding_mode, int in_layout,
                                             int out_layout, int variant, int grid_kind, int64_t* plan) {
  if (!plan) return EMO_ERR_BAD_ARG;
  for (int i = 0; i < EMO_GS3D_PLAN_COUNT; ++i) plan[i] = 0;
  bool tile;
  if (banked) vol_batch_stride = (int64_t)C * D * H * W;     // (as emo_grid_sample3d_indexed_f32 passes it)
  const gs3d::LaunchForm f = sampler_form(vol, out, N, C, D, H, W, Do, Ho, Wo, vol_batch_stride, padding_mode, in_layout, out_layout,
                                          variant, grid_kind, banked != 0, &tile);
  if (f.rc != EMO_OK) return f.rc;
  plan[EMO_GS3D_PLAN_FORM] = f.form; plan[EMO_GS3D_PLAN_ORDER] = f.order; plan[EMO_GS3D_PLAN_FMA] = f.fma;
  plan[EMO_GS3D_PLAN_NT] = f.nt; plan[EMO_GS3D_PLAN_BANK] = f.bank;
  plan[EMO_GS3D_PLAN_GRID_X] = f.gx; plan[EMO_GS3D_PLAN_GRID_Y] = f.gy; plan[EMO_GS3D_PLAN_GRID_Z] = f.gz;
  plan[EMO_GS3D_PLAN_BPS] = f.bps; plan[EMO_GS3D_PLAN_LAST_VOX] = f.last_vox; plan[EMO_GS3D_PLAN_CPB] = f.cpb;
  plan[EMO_GS3D_PLAN_LDS] = (int64_t)f.lds; plan[EMO_GS3D_PLAN_THREADS] = f.threads; plan[EMO_GS3D_PLAN_VPT] = f.vpt;
  plan[EMO_GS3D_PLAN_UPB] = f.upb; plan[EMO_GS3D_PLAN_TXS] = f.txs; plan[EMO_GS3D_PLAN_TYS] = f.tys;
  plan[EMO_GS3D_PLAN_TZS] = f.tzs; plan[EMO_GS3D_PLAN_STAGE_SLOTS] = f.cap_slots;
  return EMO_OK;
}

// ABI 29: the direction and grid of emo_volume_repack_f32 (indexed = 0) / emo_volume_repack_indexed_f32 (indexed != 0, with
// to_channels_last = 1); nothing is launched
extern "C" int emo_volume_repack_launch_form(const void* in, const void* out, int N, int C, int DHW, int to_channels_last,
                                             int indexed, int64_t* plan) {
  if (!plan) return EMO_ERR_BAD_ARG;
  int dir;
  long g[3];
  const int rc = repack_form(in, out, N, C, DHW, to_channels_last, indexed != 0, &dir, g);
  plan[EMO_REPACK_PLAN_DIRECTION] = rc == EMO_OK ? dir : 0;
  plan[EMO_REPACK_PLAN_GRID_X] = g[0]; plan[EMO_REPACK_PLAN_GRID_Y] = g[1]; plan[EMO_REPACK_PLAN_GRID_Z] = g[2];
  return rc;
}

extern "C" int emo_grid_sample3d_f32(const float* vol, const float* grid, const float* theta, const float* lin_x,
                                     const float* lin_y, const float* lin_z, float* out, int N, int C, int D, int H,
                                     int W, int Do, int Ho, int Wo, int64_t vol_batch_stride, int padding_mode,
                                     int in_layout, int out_layout, int variant, int grid_kind, void* stream) {
  return sample3d(vol, grid, theta, lin_x, lin_y, lin_z, out, N, C, D, H, W, Do, Ho, Wo, vol_batch_stride, padding_mode, in_layout,
                  out_layout, variant, grid_kind, stream, Bank{nullptr, 0});
}

// Frame n samples volume vol_index[n] of a bank of num_vols volumes, C * D * H * W floats apart (several source identities in one
// driver batch).  The channels-last kernels and the planar direct gather only; an index outside [0, num_vols) yields a zero frame.
extern "C" int emo_grid_sample3d_indexed_f32(const float* vol_bank, const int32_t* vol_index, int num_vols, const float* grid,
                                             const float* theta, const float* lin_x, const float* lin_y, const float* lin_z,
                                             float* out, int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                                             int padding_mode, int in_layout, int out_layout, int variant, int grid_kind,
                                             void* stream) {
  if (!vol_index || num_vols <= 0) return EMO_ERR_BAD_ARG;
  if (C <= 0 || D <= 0 || H <= 0 || W <= 0) return EMO_ERR_BAD_ARG;
  return sample3d(vol_bank, grid, theta, lin_x, lin_y, lin_z, out, N, C, D, H, W, Do, Ho, Wo, (int64_t)C * D * H * W,
                  padding_mode, in_layout, out_layout, variant, grid_kind, stream, Bank{vol_index, num_vols});
}

extern "C" int emo_affine_grid3d_f32(const float* theta, const float* lin_x, const float* lin_y, const float* lin_z,
                                     float* grid, int N, int Do, int Ho, int Wo, void* stream) {
  if (!theta || !lin_x || !lin_y || !lin_z || !grid) return EMO_ERR_BAD_ARG;
  if (N <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0) return EMO_ERR_BAD_ARG;
  if (N > 65535 || (long)Do * Ho * Wo >= (1L << 31) / 4) return EMO_ERR_UNSUPPORTED;
  dim3 g(emo_cdiv((long)Do * Ho * Wo, 256), N);
  hipLaunchKernelGGL(affine_grid3d_kernel, g, dim3(256), 0, (hipStream_t)stream, theta, lin_x, lin_y, lin_z, grid, Do, Ho, Wo);
  return emo_launch_status();
}

extern "C" int emo_volume_repack_f32(const float* in, float* out, int N, int C, int DHW, int to_channels_last,
                                     void* stream) {
  int dir;
  long g[3];
  const int rc = repack_form(in, out, N, C, DHW, to_channels_last, false, &dir, g);
  if (rc != EMO_OK) return rc;
  if (dir == EMO_REPACK_TO_P4 || dir == EMO_REPACK_FROM_P4)
    return emo_repack_p4_dispatch(in, out, N, C, DHW, dir == EMO_REPACK_TO_P4, stream);
  const int R = to_channels_last ? C : DHW;       // rows of the input matrix
  const int Ccols = to_channels_last ? DHW : C;   // columns of the input matrix
  hipLaunchKernelGGL(repack_kernel<>, dim3(g[0], g[1], g[2]), dim3(256), 0, (hipStream_t)stream, in, out, R, Ccols);
  return emo_launch_status();
}

// emo_volume_repack_f32(to_channels_last = 1) of N volumes into rows row[n] of a channels-last bank of num_rows volumes
extern "C" int emo_volume_repack_indexed_f32(const float* in, float* bank, const int32_t* row, int N, int C, int DHW,
                                             int num_rows, void* stream) {
  if (!row || num_rows <= 0) return EMO_ERR_BAD_ARG;
  int dir;
  long g[3];
  const int rc = repack_form(in, bank, N, C, DHW, 1, true, &dir, g);
  if (rc != EMO_OK) return rc;
  hipLaunchKernelGGL((repack_kernel<const int*, int>), dim3(g[0], g[1], g[2]), dim3(256), 0, (hipStream_t)stream, in, bank, C, DHW,
                     (const int*)row, num_rows);
  return emo_launch_status();
}
