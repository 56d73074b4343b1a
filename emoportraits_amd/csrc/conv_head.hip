// Pointwise convolution with a HANDFUL of output channels for gfx950 -- the decoder's image head: GroupNorm -> ReLU -> 1x1 conv
// 128 -> 3 -> sigmoid at the full output resolution (networks/volumetric_avatar/decoder.py:381-392, utils.py:661-788 toolkit).
//
// With 3 output channels the layer is a stream, not a GEMM: 2 x Cin x 3 FLOPs per position against 4 x Cin bytes read -- 1.5
// FLOP per byte, 2.1 GB per 16 frames at 512 x 512.  On the fp32 MFMA kernel a 32-row tile is 29/32 idle and the layer ran at
// 3.3 TB/s of its bytes behind LDS staging it does not need (0.65 ms: 1.5 % of the driver pass, a third of what was left on that
// kernel).  Here every thread owns four consecutive positions and walks the input channels: one 16-byte load per channel (a
// wave reads 1 KB contiguous of one channel plane), the per-(sample, channel) affine of the folded GroupNorm + ReLU applied in
// registers, COUT fused multiply-adds per value against weights the compiler keeps in scalar registers (uniform addresses:
// s_load), bias + activation, one 16-byte store per output channel.  No LDS, no barrier; 8 loads in flight per thread.
//
// Arithmetic per output: acc = fma(w[o][c], relu(fma(x, scale, shift)), acc) for c = 0 .. Cin-1 in order, + bias, activation --
// the operations of the implicit-GEMM kernel's staging and epilogue with a sequential fp32 sum over the channels in place of
// the MFMA's blocked one (held to the same bounds against the oracle: tests/test_kernels_gpu.py, test_bench_config_parity_gpu.py).
//
// The same channel walk with another epilogue is the tail of stage 2 (emo_stage2_head_f32, ABI 16): norm -> ReLU -> 1x1 conv
// 32 -> 3 -> tanh at the full resolution (decoder_s2_old.py:444-456), the residual added to the stage-1 image under the
// matte x face mask, clamped (notebooks/infer_s2.py:365-375) and written as fp32 planes and / or as the HWC bytes of
// pack_rgb8_kernel -- one launch where the chain emo_conv_head_f32(tanh) -> emo_stage2_compose_f32 -> emo_pack_rgb8 is three,
// with the same operations in the same order: bit-identical to that chain in both outputs.
#include "common.h"

namespace {

__device__ __forceinline__ float head_act(float v, int act) {
  if (act == EMO_ACT_RELU) return fmaxf(v, 0.0f);
  if (act == EMO_ACT_TANH) return tanhf(v);
  if (act == EMO_ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
  return v;
}

// what the stage-2 epilogue reads and writes beside the convolution's own operands (unused by the plain head)
struct Stage2Tail {
  const float* img;        // [N,3,S]
  const float* mask;       // [N,1,S]
  const float* face_mask;  // [N,1,S] or NULL (= 1)
  uint8_t* out_u8;         // [N,S,3] or NULL
};

// STAGE2 = false: out = act(acc + bias), COUT planes.  true (COUT == 3, act == tanh): out = clamp(img + tanh(acc + bias) *
// (mask * face_mask), 0, 1) into `out` (fp32 planes, may be NULL) and tail.out_u8 (bytes, may be NULL)
template <int COUT, bool STAGE2>
__global__ __launch_bounds__(256) void conv_head_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, float* __restrict__ out, int Cin,
                                                        long S, int relu_in, int act, Stage2Tail tail) {
  const int n = blockIdx.y;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;          // quad of positions
  if (4 * q >= S) return;
  const float4* xp = reinterpret_cast<const float4*>(x + (long)n * Cin * S) + q;
  const long S4 = S >> 2;
  const float* sc = scale ? scale + (long)n * Cin : nullptr;
  const float* sh = scale ? shift + (long)n * Cin : nullptr;
  const float floor_ = relu_in ? 0.0f : -__builtin_huge_valf();
  float acc[COUT][4];
#pragma unroll
  for (int o = 0; o < COUT; ++o)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[o][j] = 0.0f;
  constexpr int U = 8;
  int c = 0;
  for (; c + U <= Cin; c += U) {
    float4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = xp[(long)(c + u) * S4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
      if (sc) {
        const float a = sc[c + u], b = sh[c + u];
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = __fmaf_rn(e[j], a, b);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = fmaxf(e[j], floor_);
#pragma unroll
      for (int o = 0; o < COUT; ++o) {
        const float wv = w[o * Cin + c + u];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[o][j] = __fmaf_rn(wv, e[j], acc[o][j]);
      }
    }
  }
  for (; c < Cin; ++c) {
    const float4 v = xp[(long)c * S4];
    float e[4] = {v.x, v.y, v.z, v.w};
    if (sc) {
      const float a = sc[c], b = sh[c];
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = __fmaf_rn(e[j], a, b);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = fmaxf(e[j], floor_);
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
      const float wv = w[o * Cin + c];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[o][j] = __fmaf_rn(wv, e[j], acc[o][j]);
    }
  }
  if constexpr (!STAGE2) {
    float4* op = reinterpret_cast<float4*>(out + (long)n * COUT * S) + q;
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
      const float b = bias ? bias[o] : 0.0f;
      op[(long)o * S4] = make_float4(head_act(acc[o][0] + b, act), head_act(acc[o][1] + b, act), head_act(acc[o][2] + b, act),
                                     head_act(acc[o][3] + b, act));
    }
  } else {
    static_assert(!STAGE2 || COUT == 3, "the stage-2 tail writes an RGB image");
    // the operations of stage2_compose_kernel and pack_rgb8_kernel, each rounded on its own (the build's -ffp-contract=off)
    const float4 m4 = reinterpret_cast<const float4*>(tail.mask + (long)n * S)[q];
    float gate[4] = {m4.x, m4.y, m4.z, m4.w};
    if (tail.face_mask) {
      const float4 f4 = reinterpret_cast<const float4*>(tail.face_mask + (long)n * S)[q];
      gate[0] = gate[0] * f4.x; gate[1] = gate[1] * f4.y; gate[2] = gate[2] * f4.z; gate[3] = gate[3] * f4.w;
    }
    const float4* ip = reinterpret_cast<const float4*>(tail.img + (long)n * COUT * S) + q;
    float4 im[COUT];
#pragma unroll
    for (int o = 0; o < COUT; ++o) im[o] = ip[(long)o * S4];
    float v[COUT][4];
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
      const float b = bias ? bias[o] : 0.0f;
      const float i4[4] = {im[o].x, im[o].y, im[o].z, im[o].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float t = i4[j] + head_act(acc[o][j] + b, EMO_ACT_TANH) * gate[j];
        v[o][j] = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
      }
    }
    if (out) {
      float4* op = reinterpret_cast<float4*>(out + (long)n * COUT * S) + q;
#pragma unroll
      for (int o = 0; o < COUT; ++o) op[(long)o * S4] = make_float4(v[o][0], v[o][1], v[o][2], v[o][3]);
    }
    if (tail.out_u8) {
      // four pixels x RGB = 12 bytes at a 4-byte aligned address (S % 4 == 0): three dwords, byte k of the run in bits 8 (k % 4)
      uint32_t d[3] = {0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int o = 0; o < COUT; ++o) {
          const int k = j * 3 + o;
          d[k >> 2] |= (uint32_t)(uint8_t)(v[o][j] * 255.0f) << (8 * (k & 3));
        }
      uint32_t* bp = reinterpret_cast<uint32_t*>(tail.out_u8 + ((long)n * S + 4 * q) * 3);
      bp[0] = d[0];
      bp[1] = d[1];
      bp[2] = d[2];
    }
  }
}

}  // namespace

// out[n][o][p] = act(bias[o] + sum_c w[o][c] * in(x[n][c][p])),  in(v) = relu_in ? max(v * scale[n][c] + shift[n][c], 0) : affine
// x [N, Cin, S] (S positions per channel, any number of spatial dimensions), w [Cout, Cin] plain row-major fp32, Cout in 1..4,
// S a multiple of 4, x and out 16-byte aligned (EMO_ERR_UNSUPPORTED / EMO_ERR_ALIGN otherwise: the caller runs the
// implicit-GEMM kernel).  scale / shift [N, Cin] both or neither; bias [Cout] or NULL.
extern "C" int emo_conv_head_f32(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
                                 float* out, int N, int Cin, int Cout, int64_t S, int relu_in, int act, void* stream) {
  if (!x || !w || !out || N <= 0 || Cin <= 0 || Cout <= 0 || S <= 0) return EMO_ERR_BAD_ARG;
  if ((scale == nullptr) != (shift == nullptr)) return EMO_ERR_BAD_ARG;
  if (act < EMO_ACT_NONE || act > EMO_ACT_SIGMOID) return EMO_ERR_BAD_ARG;
  if (Cout > 4 || (S & 3) || N > 65535) return EMO_ERR_UNSUPPORTED;
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) != 0) return EMO_ERR_ALIGN;
  const long blocks = (S / 4 + 255) / 256;
  if (blocks > 0x7fffffffL) return EMO_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks, (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  const Stage2Tail none = {nullptr, nullptr, nullptr, nullptr};
  switch (Cout) {
    case 1: hipLaunchKernelGGL((conv_head_kernel<1, false>), grid, dim3(256), 0, s, x, w, bias, scale, shift, out, Cin, (long)S, relu_in, act, none); break;
    case 2: hipLaunchKernelGGL((conv_head_kernel<2, false>), grid, dim3(256), 0, s, x, w, bias, scale, shift, out, Cin, (long)S, relu_in, act, none); break;
    case 3: hipLaunchKernelGGL((conv_head_kernel<3, false>), grid, dim3(256), 0, s, x, w, bias, scale, shift, out, Cin, (long)S, relu_in, act, none); break;
    default: hipLaunchKernelGGL((conv_head_kernel<4, false>), grid, dim3(256), 0, s, x, w, bias, scale, shift, out, Cin, (long)S, relu_in, act, none); break;
  }
  return emo_launch_status();
}

// ABI 16.  The tail of stage 2 in one launch (include/emo_hip.h has the definition):
//   out = clamp(img + tanh(bias + sum_c w[o][c] * in(x[n][c][p])) * (mask * face_mask), 0, 1),  3 output channels
// x [N, Cin, S], w [3][Cin] plain row-major, img [N,3,S], mask [N,1,S], face_mask [N,1,S] or NULL (= 1), out_f32 [N,3,S] or NULL,
// out_u8 [N,S,3] or NULL (at least one of the two).  Refusals as emo_conv_head_f32; out_u8 4-byte aligned.
extern "C" int emo_stage2_head_f32(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
                                   const float* img, const float* mask, const float* face_mask, float* out_f32, uint8_t* out_u8,
                                   int N, int Cin, int64_t S, int relu_in, void* stream) {
  if (!x || !w || !img || !mask || N <= 0 || Cin <= 0 || S <= 0) return EMO_ERR_BAD_ARG;
  if (!out_f32 && !out_u8) return EMO_ERR_BAD_ARG;
  if ((scale == nullptr) != (shift == nullptr)) return EMO_ERR_BAD_ARG;
  if ((S & 3) || N > 65535) return EMO_ERR_UNSUPPORTED;
  const uintptr_t quads = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(mask) |
                          reinterpret_cast<uintptr_t>(face_mask) | reinterpret_cast<uintptr_t>(out_f32);
  if ((quads & 15) != 0 || (reinterpret_cast<uintptr_t>(out_u8) & 3) != 0) return EMO_ERR_ALIGN;
  const long blocks = (S / 4 + 255) / 256;
  if (blocks > 0x7fffffffL) return EMO_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks, (unsigned)N);
  const Stage2Tail tail = {img, mask, face_mask, out_u8};
  hipLaunchKernelGGL((conv_head_kernel<3, true>), grid, dim3(256), 0, (hipStream_t)stream, x, w, bias, scale, shift, out_f32, Cin,
                     (long)S, relu_in, EMO_ACT_TANH, tail);
  return emo_launch_status();
}
