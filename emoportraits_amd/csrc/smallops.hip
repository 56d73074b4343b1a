// Small wave-reduced kernels of the hot path for gfx950: the embedding arithmetic in front of the WarpGenerator
// (part of a5) and the output packing (a11).  None of these is MFMA-shaped:
// M is a few thousand rows, the per-frame "N" is 1..16, so each output row is one 64-lane dot product.
#include "common.h"

namespace {

// C[b][m][0..NN) = sum_k A[m][k] * B[b][k][0..NN)   (A shared by the batch: Linear / 1x1 conv on 4x4 / projector u)
// one wave per (m, b); lanes stride over k; NN <= 16 accumulators per lane; butterfly reduction.
template <int NN>
__global__ __launch_bounds__(256) void small_gemm_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                         float* __restrict__ C, int M, int K, long b_stride,
                                                         long c_stride) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + wave;
  const int b = blockIdx.y;
  if (m >= M) return;
  const float* a = A + (long)m * K;
  const float* bb = B + (long)b * b_stride;
  float acc[NN];
#pragma unroll
  for (int j = 0; j < NN; ++j) acc[j] = 0.0f;
  for (int k = lane; k < K; k += 64) {
    const float av = a[k];
    const float* br = bb + (long)k * NN;
#pragma unroll
    for (int j = 0; j < NN; ++j) acc[j] = __fmaf_rn(av, br[j], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    float v = acc[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    acc[j] = v;
  }
  if (lane == 0) {
    float* c = C + (long)b * c_stride + (long)m * NN;
#pragma unroll
    for (int j = 0; j < NN; ++j) c[j] = acc[j];
  }
}

// ProjectorNorm second half + assign_adaptive_norm_params (networks/volumetric_avatar/utils.py:1137-1151, :983-995):
//   T[b][c][0..E) (= u_i @ embed) times v_i [E][2] -> (d_gamma, d_beta); ada_gamma = gamma_c + d_gamma, ada_beta = beta_c + d_beta
// rows c of ALL adaptive norms of a net are concatenated; norm_of_row[c] selects v_i.
__global__ __launch_bounds__(256) void projector_finalize_kernel(const float* __restrict__ T, const float* __restrict__ V,
                                                                 const int* __restrict__ norm_of_row,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float* __restrict__ ag,
                                                                 float* __restrict__ ab, int B, int R, int E) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * R) return;
  const int c = i % R;
  const float* t = T + (long)i * E;
  const float* v = V + (long)norm_of_row[c] * E * 2;
  float dg = 0.0f, db = 0.0f;
  for (int k = 0; k < E; ++k) {
    dg = __fmaf_rn(t[k], v[2 * k], dg);
    db = __fmaf_rn(t[k], v[2 * k + 1], db);
  }
  ag[i] = gamma[c] + dg;
  ab[i] = beta[c] + db;
}

// the rotation clamp of get_transform_matrix (utils/point_transforms.py:188-242) and of ExpressionEmbed.forward_image
// (expression_embedder.py:302-316): [-pi/2, pi] in fp32
__device__ __forceinline__ float pose_clamp_angle(float v) {
  const float kPi = 3.14159265358979323846f;
  const float lo = -kPi / 2, hi = kPi;
  return v < lo ? lo : (v > hi ? hi : v);
}

// utils/point_transforms.py:188-242 get_transform_matrix: theta = S @ R @ T of one sample -> o[16]
__device__ __forceinline__ void pose_theta_row(float sx, float sy, float sz, float yaw_in, float pitch_in, float roll_in, float t0,
                                               float t1, float t2, float* __restrict__ o) {
  const float yaw = pose_clamp_angle(yaw_in), pitch = pose_clamp_angle(pitch_in), roll = pose_clamp_angle(roll_in);
  const float yc = cosf(yaw), ys = sinf(yaw), pc = cosf(pitch), ps = sinf(pitch), rc = cosf(roll), rs = sinf(roll);
  float R[3][3];
  R[0][0] = yc * pc;  R[0][1] = yc * ps * rs - ys * rc;  R[0][2] = yc * ps * rc + ys * rs;
  R[1][0] = ys * pc;  R[1][1] = ys * ps * rs + yc * rc;  R[1][2] = ys * ps * rc - yc * rs;
  R[2][0] = -ps;      R[2][1] = pc * rs;                 R[2][2] = pc * rc;
  const float S[3] = {sx, sy, sz};
  const float t[3] = {t0, t1, t2};
  for (int i = 0; i < 3; ++i) {
    float row[3];
    for (int j = 0; j < 3; ++j) { row[j] = S[i] * R[i][j]; o[i * 4 + j] = row[j]; }
    // (S R T)[i][3] = sum_j (S R)[i][j] * t[j]   (the 4th column of S R is zero, T's diagonal is one)
    o[i * 4 + 3] = row[0] * t[0] + row[1] * t[1] + row[2] * t[2];
  }
  o[12] = 0.0f; o[13] = 0.0f; o[14] = 0.0f; o[15] = 1.0f;
}

// one thread per sample
__global__ void pose_theta_kernel(const float* __restrict__ scale, int scale_cols, const float* __restrict__ rotation,
                                  const float* __restrict__ translation, float* __restrict__ theta, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float sx = scale[b * scale_cols], sy = scale_cols == 3 ? scale[b * 3 + 1] : sx,
              sz = scale_cols == 3 ? scale[b * 3 + 2] : sx;
  pose_theta_row(sx, sy, sz, rotation[b * 3 + 0], rotation[b * 3 + 1], rotation[b * 3 + 2], translation[b * 3],
                 translation[b * 3 + 1], translation[b * 3 + 2], theta + (long)b * 16);
}

// notebooks/infer.py:641-644: img.clamp(0,1) -> ToPILImage (mul(255).byte(), i.e. truncation) -> HWC uint8
__global__ __launch_bounds__(256) void pack_rgb8_kernel(const float* __restrict__ img, uint8_t* __restrict__ out,
                                                        long N, long HW) {
  const long total = N * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long n = i / HW, p = i - n * HW;
    const float* src = img + n * 3 * HW + p;
    uint8_t* dst = out + i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = src[c * HW];
      v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
      dst[c] = (uint8_t)(v * 255.0f);
    }
  }
}

// the inverse direction, notebooks/infer.py:211-223 convert_to_tensor (ToTensor): [N,H,W,3] uint8 -> [N,3,H,W] fp32 = byte / 255
// (an fp32 division like torch's, not a multiplication by the rounded reciprocal)
__global__ __launch_bounds__(256) void unpack_rgb8_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, long N,
                                                          long HW) {
  const long total = N * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long n = i / HW, p = i - n * HW;
    const uint8_t* src = in + i * 3;
    float* dst = out + n * 3 * HW + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c * HW] = __fdiv_rn((float)src[c], 255.0f);
  }
}

// inverse of B 4x4 matrices (head-pose affines: notebooks/infer.py:443, expression_embedder.py:185-188 call
// `theta.float().inverse()`): Gauss-Jordan with partial pivoting in double, one thread per matrix.
__global__ __launch_bounds__(64) void mat4_inverse_kernel(const float* __restrict__ in, float* __restrict__ out, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double m[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      m[i][j] = (double)in[b * 16 + i * 4 + j];
      m[i][4 + j] = i == j ? 1.0 : 0.0;
    }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    int piv = c;
    double best = fabs(m[c][c]);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r > c && fabs(m[r][c]) > best) {
        best = fabs(m[r][c]);
        piv = r;
      }
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r == piv && piv != c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const double t = m[c][j];
          m[c][j] = m[r][j];
          m[r][j] = t;
        }
      }
    const double inv = 1.0 / m[c][c];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[c][j] *= inv;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r != c) {
        const double f = m[r][c];
#pragma unroll
        for (int j = 0; j < 8; ++j) m[r][j] -= f * m[c][j];
      }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[b * 16 + i * 4 + j] = (float)m[i][4 + j];
}

// notebooks/infer.py:686-736 get_mixing_theta for ONE source and ONE target per frame (hostglue.mixing_theta with a single
// source: its roll along the source axis is then a no-op), one thread per frame, fp64 from the fp32 inputs.
// The polar decomposition L = U P of a 3x3 linear part comes from a one-sided Jacobi SVD run to convergence: columns of
// A = L V are made orthogonal by plane rotations (V accumulates them), then sigma_j = |a_j|, U = [a_j / sigma_j] V^T and
// P = V diag(sigma) V^T -- scipy.linalg.polar's own formula, for det L < 0 as well (U is then a reflection).
__device__ inline bool finite_f64(double x) { return (x - x) == 0.0; }   // false for +-inf and nan (no fast-math in either build)

__device__ inline void polar3(const double L[3][3], double U[3][3], double P[3][3]) {
  double a[3][3], v[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      a[i][j] = L[i][j];
      v[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool rotated = false;
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      double alpha = 0.0, beta = 0.0, gamma = 0.0;
      for (int i = 0; i < 3; ++i) {
        alpha += a[i][p] * a[i][p];
        beta += a[i][q] * a[i][q];
        gamma += a[i][p] * a[i][q];
      }
      if (!(fabs(gamma) > 4e-16 * sqrt(alpha * beta))) continue;
      rotated = true;
      const double zeta = (beta - alpha) / (2.0 * gamma);
      const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
      for (int i = 0; i < 3; ++i) {
        const double ap = a[i][p], aq = a[i][q];
        a[i][p] = c * ap - s * aq;
        a[i][q] = s * ap + c * aq;
        const double vp = v[i][p], vq = v[i][q];
        v[i][p] = c * vp - s * vq;
        v[i][q] = s * vp + c * vq;
      }
    }
    if (!rotated) break;
  }
  double sigma[3];
  for (int j = 0; j < 3; ++j) {
    sigma[j] = sqrt(a[0][j] * a[0][j] + a[1][j] * a[1][j] + a[2][j] * a[2][j]);
    if (sigma[j] > 0.0)
      for (int i = 0; i < 3; ++i) a[i][j] /= sigma[j];
  }
  // a rank-deficient L (outside the conditioning this serves): complete a zero column from the other two
  for (int j = 0; j < 3; ++j)
    if (!(sigma[j] > 0.0)) {
      const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      a[0][j] = a[1][j1] * a[2][j2] - a[2][j1] * a[1][j2];
      a[1][j] = a[2][j1] * a[0][j2] - a[0][j1] * a[2][j2];
      a[2][j] = a[0][j1] * a[1][j2] - a[1][j1] * a[0][j2];
    }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double u = 0.0, p = 0.0;
      for (int k = 0; k < 3; ++k) {
        u += a[i][k] * v[j][k];
        p += v[i][k] * sigma[k] * v[j][k];
      }
      U[i][j] = u;
      P[i][j] = p;
    }
}

__global__ __launch_bounds__(64) void mixing_theta_kernel(const float* __restrict__ target, const float* __restrict__ source,
                                                          const int* __restrict__ index, int B, int K, int mix_old,
                                                          float* __restrict__ out) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= B) return;
  const float* tg = target + (long)n * 16;
  float* o = out + (long)n * 16;
  double res[3][4];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) res[i][j] = (double)tg[i * 4 + j];     // the driver pose: every fallback but one
  const int k = index ? index[n] : 0;
  bool src_ok = k >= 0 && k < K;                    // (an unknown slot reads no source memory)
  double Ls[3][3], Lt[3][3];
  if (src_ok) {
    const float* sr = source + (long)k * 16;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        Ls[i][j] = (double)sr[i * 4 + j];
        src_ok = src_ok && finite_f64(Ls[i][j]);
      }
  }
  if (src_ok) {                                     // else: the source decomposition "failed" (:718-719), the driver pose
    bool tgt_ok = true;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        Lt[i][j] = res[i][j];
        tgt_ok = tgt_ok && finite_f64(Lt[i][j]);
      }
    double Us[3][3], Ps[3][3];
    polar3(Ls, Us, Ps);
    if (!tgt_ok) {                                  // :724-725: the source stretch, no translation
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) res[i][j] = Ps[i][j];
        res[i][3] = 0.0;
      }
    } else {
      double Ut[3][3], Pt[3][3];
      polar3(Lt, Ut, Pt);
      const double t[3] = {res[0][3], res[1][3], res[2][3]};
      if (mix_old) {                                // :727-728 translation @ tgt_rot @ src_stretch = [U_t P_s | t_t]
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
            for (int q = 0; q < 3; ++q) acc += Ut[i][q] * Ps[q][j];
            res[i][j] = acc;
          }
      } else {                                      // :729-730 src_stretch * mean(tgt_stretch) / mean(src_stretch) @ tgt_rot @ T
        double ms = 1.0, mt = 1.0;                  // (means of the 4x4 homogeneous stretches: the 1 at (3,3) counts)
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) {
            ms += Ps[i][j];
            mt += Pt[i][j];
          }
        ms /= 16.0;
        mt /= 16.0;
        double X[3][3], A[3][3];
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) X[i][j] = Ps[i][j] * mt / ms;
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
            for (int q = 0; q < 3; ++q) acc += X[i][q] * Ut[q][j];
            A[i][j] = acc;
          }
        for (int i = 0; i < 3; ++i) {
          for (int j = 0; j < 3; ++j) res[i][j] = A[i][j];
          res[i][3] = A[i][0] * t[0] + A[i][1] * t[1] + A[i][2] * t[2];
        }
      }
    }
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) o[i * 4 + j] = (float)res[i][j];
  o[12] = 0.0f; o[13] = 0.0f; o[14] = 0.0f; o[15] = 1.0f;
}

// notebooks/infer.py:571-581 smooth_pose, one EMA stream per source identity: frame i belongs to stream stream_of[i] (NULL:
// all to stream 0) and is smoothed within that stream's frames in frame order, fp32 exactly as hostglue.ema_scan (two
// rounded products, one rounded sum).  One thread per stream walks all 16 elements, so the stream's flag is read and
// written by one thread only.  ABI 26 (hostglue.ema_scan_tracks): a row with restart[i] != 0 first drops the stream's state; a
// row with present[i] == 0 is smoothed from a private copy of the state (started at the row where there is none) and leaves
// the stream as it was.  Both masks NULL: the scan as it always was.
__global__ __launch_bounds__(64) void theta_ema_scan_kernel(const float* __restrict__ values, const int* __restrict__ stream_of,
                                                            float* __restrict__ state, int* __restrict__ has_state, int n, int K,
                                                            float m, float om, const int* __restrict__ restart,
                                                            const int* __restrict__ present, float* __restrict__ out) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  bool has = has_state[k] != 0, cleared = false;
  float cur[16];
  for (int e = 0; e < 16; ++e) cur[e] = has ? state[(long)k * 16 + e] : 0.0f;
  for (int i = 0; i < n; ++i) {
    if ((stream_of ? stream_of[i] : 0) != k) continue;
    if (restart && restart[i] != 0) {
      has = false;
      cleared = true;
    }
    const bool here = !present || present[i] != 0;
    const float* v = values + (long)i * 16;
    float* o = out + (long)i * 16;
    for (int e = 0; e < 16; ++e) {
      const float prev = has ? cur[e] : v[e];
      const float a = v[e] * m, b = prev * om;
      const float next = a + b;
      if (here) cur[e] = next;
      o[e] = next;
    }
    if (here) has = true;
  }
  if (has) {
    for (int e = 0; e < 16; ++e) state[(long)k * 16 + e] = cur[e];
    has_state[k] = 1;
  } else if (cleared) {
    has_state[k] = 0;
  }
}

// The expression controls of the batched entry points (include/emo_hip.h, ABI 20; hostglue.expression_controls is the contract):
// relative transfer and gain about the identity's source expression, an additive offset, an EMA -- per stream and in row order.
// One block per stream; a thread owns the elements j = threadIdx.x, + blockDim.x, ... of every row and of the stream's anchor
// and EMA, and walks the n rows in order, so `out` may be `values`.  Every thread reads the stream's flags, then the barrier;
// the block's LAST thread alone writes them, at its end (a host build that runs thread after thread reaches it last as well).
// ABI 26: a row with restart[i] != 0 first drops the stream's anchor and EMA; a row with present[i] == 0 is its own anchor and
// the start of its own EMA where the stream has none, and leaves the stream as it was.  The flags the last thread writes are
// what the walk ends with: 1 only if a present row came after the stream's last restart.  Both masks NULL: as it always was.
__global__ __launch_bounds__(128) void expr_controls_kernel(const float* values, const int* __restrict__ stream_of,
                                                            const float* __restrict__ neutral, const float* __restrict__ gain,
                                                            const float* __restrict__ offset, float* __restrict__ anchor,
                                                            int* has_anchor, float* __restrict__ ema, int* has_ema, int n, int E,
                                                            int relative, int smooth, float m, float om,
                                                            const int* __restrict__ restart, const int* __restrict__ present,
                                                            float* out) {
  const int k = blockIdx.x;
  const bool had_anchor = relative && has_anchor[k] != 0;
  const bool had_ema = smooth && has_ema[k] != 0;
  __syncthreads();
  for (int j = threadIdx.x; j < E; j += blockDim.x) {
    const long kj = (long)k * E + j;
    bool ha = had_anchor, he = had_ema, taken = false;
    float anc = ha ? anchor[kj] : 0.0f;
    float cur = he ? ema[kj] : 0.0f;
    const float neu = neutral ? neutral[kj] : 0.0f;
    for (int i = 0; i < n; ++i) {
      if ((stream_of ? stream_of[i] : 0) != k) continue;
      if (restart && restart[i] != 0) { ha = false; he = false; }
      const bool here = !present || present[i] != 0;
      const long ij = (long)i * E + j;
      float e = values[ij];
      if (neutral) {
        float r = neu;
        if (relative) {
          if (!ha && here) { anc = e; ha = true; taken = true; }
          r = ha ? anc : e;
        }
        float t = e - r;
        if (gain) t = t * gain[i];
        e = neu + t;
      }
      if (offset) e = e + offset[ij];
      if (smooth) {
        const float prev = he ? cur : e;
        const float a = e * m, b = prev * om;
        e = a + b;
        if (here) { cur = e; he = true; }
      }
      out[ij] = e;
    }
    if (ha && taken) anchor[kj] = anc;
    if (he) ema[kj] = cur;
  }
  if (threadIdx.x == blockDim.x - 1 && (relative || smooth)) {
    bool seen = false, live_a = had_anchor, live_e = had_ema;
    for (int i = 0; i < n; ++i) {
      if ((stream_of ? stream_of[i] : 0) != k) continue;
      seen = true;
      if (restart && restart[i] != 0) { live_a = false; live_e = false; }
      if (!present || present[i] != 0) { live_a = true; live_e = true; }
    }
    if (seen && relative) has_anchor[k] = live_a ? 1 : 0;
    if (seen && smooth) has_ema[k] = live_e ? 1 : 0;
  }
}

// The head-pose controls of the batched entry points (include/emo_hip.h, ABI 21; hostglue.head_pose_controls is the contract):
// the regressed (scale, rotation, translation) of every row edited before theta is formed -- frontal, relative transfer and gain
// about the identity's source pose, offsets, zoom.  One block per stream.  Only the anchor depends on the row order: every
// thread reads the stream's flag and its stored anchor, then the barrier; every thread then walks the row indices once in
// order and carries the anchor of the segment it is in -- the stored one until a restart, else the segment's first present row,
// which it loads for itself into registers (ABI 26: a row with restart[i] != 0 begins a segment, a row with present[i] == 0
// cannot be an anchor and is its own reference while its segment has none; both masks NULL: one segment, its anchor the stored
// one or the stream's first row, as it always was) -- and edits the rows i = threadIdx.x, + blockDim.x, ... of the walk, a whole
// row each: nine floats in, nine floats and theta's sixteen out.  The block's LAST thread alone writes the anchor and the flag
// its walk ended with, at its end (a host build that runs thread after thread reaches it last as well, so no thread reads what
// it wrote).  The outputs alias no input.
__global__ __launch_bounds__(64) void head_pose_controls_kernel(
    const float* __restrict__ scale, int scale_cols, const float* __restrict__ rotation, const float* __restrict__ translation,
    const int* __restrict__ stream_of, const float* __restrict__ source, const float* __restrict__ gain,
    const float* __restrict__ rotation_offset, const float* __restrict__ translation_offset, const float* __restrict__ zoom,
    float* anchor, int* has_anchor, int n, int relative, int frontal, const int* __restrict__ restart,
    const int* __restrict__ present, float* __restrict__ out_srt, float* __restrict__ out_theta) {
  const int k = blockIdx.x;
  const bool had_anchor = relative && has_anchor[k] != 0;
  float q[9], ref[9];
  for (int j = 0; j < 9; ++j) { q[j] = 0.0f; ref[j] = 0.0f; }
  if (source) {
    for (int j = 0; j < 9; ++j) q[j] = source[(long)k * 9 + j];
    for (int j = 3; j < 6; ++j) q[j] = pose_clamp_angle(q[j]);
    for (int j = 0; j < 9; ++j) ref[j] = q[j];
  }
  if (had_anchor)
    for (int j = 0; j < 9; ++j) ref[j] = anchor[(long)k * 9 + j];
  __syncthreads();
  // step 0 of row i: the scale in three columns, the rotation clamped, the translation
  auto load = [&](int i, float* p) {
    p[0] = scale[(long)i * scale_cols];
    p[1] = scale_cols == 3 ? scale[(long)i * 3 + 1] : p[0];
    p[2] = scale_cols == 3 ? scale[(long)i * 3 + 2] : p[0];
    for (int j = 0; j < 3; ++j) {
      p[3 + j] = pose_clamp_angle(rotation[(long)i * 3 + j]);
      p[6 + j] = translation[(long)i * 3 + j];
    }
  };
  bool anchored = had_anchor;                                 // the segment at hand has an anchor, and `ref` holds it
  int taken = -1;                                             // the row it was taken from in this call (-1: the stored one)
  for (int i = 0; i < n; ++i) {
    if ((stream_of ? stream_of[i] : 0) != k) continue;
    if (relative) {
      if (restart && restart[i] != 0) anchored = false;
      if (!anchored && (!present || present[i] != 0)) {
        load(i, ref);
        anchored = true;
        taken = i;
      }
    }
    if (i % (int)blockDim.x != (int)threadIdx.x) continue;
    float p[9], r[9];
    load(i, p);
    for (int j = 0; j < 9; ++j) r[j] = relative && !anchored ? p[j] : ref[j];
    if (frontal) { p[3] = 0.0f; p[4] = 0.0f; p[6] = 0.0f; p[7] = 0.0f; p[8] = 0.0f; }
    if (source) {
      for (int j = 3; j < 9; ++j) {
        float d = p[j] - r[j];
        if (gain) d = d * gain[i];
        p[j] = q[j] + d;
      }
      if (relative)
        for (int j = 0; j < 3; ++j) p[j] = q[j] * __fdiv_rn(p[j], r[j]);
    }
    for (int j = 0; j < 3; ++j) {
      if (rotation_offset) p[3 + j] = p[3 + j] + rotation_offset[(long)i * 3 + j];
      if (translation_offset) p[6 + j] = p[6 + j] + translation_offset[(long)i * 3 + j];
      if (zoom) p[j] = p[j] * zoom[i];
    }
    for (int j = 0; j < 9; ++j) out_srt[(long)i * 9 + j] = p[j];
    pose_theta_row(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], out_theta + (long)i * 16);
  }
  if (threadIdx.x == blockDim.x - 1 && relative) {
    if (anchored && taken >= 0)
      for (int j = 0; j < 9; ++j) anchor[(long)k * 9 + j] = ref[j];
    if (anchored != had_anchor) has_anchor[k] = anchored ? 1 : 0;
  }
}

// Face boxes -> crop and paste windows with the crop tracker's state carried along the row order (include/emo_hip.h, ABI 23;
// hostglue.crop_track is the contract, which restates notebooks/infer.py:301-352 crop_image).  The launch pattern of
// theta_ema_scan_kernel: one thread per stream walks the M rows in order and owns its stream's state, flag and last window; a row
// whose stream lies outside [0, K) has no state and is written by thread 0.  Everything stays a double until it has passed its
// range test; -ffp-contract=off keeps the two products and the sum of the EMA apart.
__device__ inline bool crop_window_inside(int x, int y, int s, int W, int H, int min_side) {
  return s > 0 && x >= 0 && y >= 0 && x <= W - s && y <= H - s && s >= min_side;
}

__device__ inline bool crop_in_range(double v) { return finite_f64(v) && fabs(v) < 1073741824.0; }

__global__ __launch_bounds__(64) void crop_track_kernel(const double* __restrict__ boxes, const int* __restrict__ stream_of,
                                                        const int* __restrict__ sizes, int Wf, int Hf, double* __restrict__ state,
                                                        int* __restrict__ has, int* __restrict__ last, int M, int K, double m,
                                                        double om, int smooth, int fixed, double scale, int box_format, int hold,
                                                        int min_side, const int* __restrict__ restart, int* __restrict__ crop,
                                                        int* __restrict__ paste, double* __restrict__ face_scale) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  bool had = smooth && has[k] != 0;
  double st[3] = {0.0, 0.0, 0.0};
  if (had)
    for (int j = 0; j < 3; ++j) st[j] = state[(long)k * 3 + j];
  int lw[4] = {0, 0, 0, 0};
  if (last)
    for (int j = 0; j < 4; ++j) lw[j] = last[(long)k * 4 + j];
  bool touched = false, kept = false, cleared = false;
  for (int i = 0; i < M; ++i) {
    const int ki = stream_of ? stream_of[i] : 0;
    const bool in_range = ki >= 0 && ki < K;
    if (in_range ? ki != k : k != 0) continue;
    if (restart && in_range && restart[i] != 0) {             // (ABI 25: the stream begins again at this row)
      had = false;
      touched = false;
      kept = false;
      cleared = true;
      for (int j = 0; j < 4; ++j) lw[j] = 0;
    }
    const int W = sizes ? sizes[2 * i] : Wf, H = sizes ? sizes[2 * i + 1] : Hf;
    int* const c = crop + (long)i * 4;
    int* const p = paste + (long)i * 4;
    if (W < 1 || H < 1) {                                   // (no frame: nothing can be read)
      for (int j = 0; j < 4; ++j) { c[j] = 0; p[j] = 0; }
      if (face_scale) face_scale[i] = 0.0;
      continue;
    }
    const double* const b = boxes + (long)i * 4;
    double x0 = b[0], y0 = b[1], x1 = b[2], y1 = b[3];
    if (box_format == 1) {                                  // hostglue.detection_to_face, in its order of operations
      const double wd = (double)W, hd = (double)H, hm1 = (double)(H - 1);
      const double t = hd * (b[1] + b[3] * 1.2);
      x0 = wd * b[0];
      y0 = hd * b[1] * 0.9;
      x1 = wd * (b[0] + b[2]);
      y1 = hm1 < t ? hm1 : t;
    }
    bool present = false;
    int wx = 0, wy = 0, ws = 0;
    double fs = 0.0;
    if (in_range && crop_in_range(x0) && crop_in_range(y0) && crop_in_range(x1) && crop_in_range(y1)) {
      double v[3] = {floor((x1 + x0) / 2), floor((y1 + y0) / 2), (((x1 - x0) + y1) - y0) * scale};
      if (smooth) {
        for (int j = 0; j < 3; ++j) {
          if (!had) {
            st[j] = v[j];
          } else if (!fixed) {
            const double a = v[j] * m, bb = st[j] * om;
            st[j] = a + bb;
          }
          v[j] = st[j];
        }
        had = true;
        touched = true;
      }
      const double cx = rint(v[0]), cy = rint(v[1]);
      double sz = rint(v[2]);
      if (finite_f64(sz) && sz >= 2.0) {
        sz = sz - fmod(sz, 2.0);
        const double half = sz / 2;
        double b0 = cx - half, b1 = cy - half, b2 = cx + half, b3 = cy + half;
        double over = b0 >= 0 ? 0.0 : -b0;
        const double o1 = b1 >= 0 ? 0.0 : -b1, o2 = b2 <= (double)W ? 0.0 : b2 - (double)W, o3 = b3 <= (double)H ? 0.0 : b3 - (double)H;
        if (o1 > over) over = o1;
        if (o2 > over) over = o2;
        if (o3 > over) over = o3;
        b0 = b0 + over; b1 = b1 + over; b2 = b2 - over; b3 = b3 - over;
        double side = trunc((b2 - b0 + b3 - b1) / 2);
        side = side - fmod(side, 2.0);
        if (side >= 2.0 && side < 1073741824.0 && fabs(cx) < 1073741824.0 && fabs(cy) < 1073741824.0) {
          ws = (int)side;
          wx = (int)cx - ws / 2;
          wy = (int)cy - ws / 2;
          present = crop_window_inside(wx, wy, ws, W, H, min_side);
          if (present) fs = side / sz;
        }
      }
    }
    if (present) {
      lw[0] = wx; lw[1] = wy; lw[2] = ws; lw[3] = ws;
      kept = true;
      for (int j = 0; j < 4; ++j) { c[j] = lw[j]; p[j] = lw[j]; }
    } else if (hold && in_range && crop_window_inside(lw[0], lw[1], lw[2], W, H, min_side)) {
      for (int j = 0; j < 4; ++j) { c[j] = lw[j]; p[j] = lw[j]; }
    } else {
      const int s = W < H ? W : H;
      c[0] = (W - s) / 2; c[1] = (H - s) / 2; c[2] = s; c[3] = s;
      for (int j = 0; j < 4; ++j) p[j] = 0;
    }
    if (face_scale) face_scale[i] = fs;
  }
  if (touched) {
    for (int j = 0; j < 3; ++j) state[(long)k * 3 + j] = st[j];
    has[k] = 1;
  } else if (cleared && smooth) {
    has[k] = 0;
  }
  if ((kept || cleared) && last)
    for (int j = 0; j < 4; ++j) last[(long)k * 4 + j] = lw[j];
}

// Unordered detections -> ordered track rows (include/emo_hip.h, ABI 25; hostglue.track_assign is the contract): greedy IoU
// association, one block of one wave per video stream, the frames of the stream walked in order.  The stream's tracks (ref, age)
// live in LDS for the whole walk; per frame the lanes d < D take a detection each, the P x D IoU matrix lies across the lanes (pair
// p * D + d on lane (p * D + d) % 64, at most eight a lane, in registers), and every round of the matching is an xor butterfly over
// the total order (IoU, then the smaller pair index = the smaller p, then the smaller d): every lane ends with the same winner, so
// the loop's trip count is uniform and its result does not depend on the butterfly's shape.  Lane 0 books the winner; births are a
// serial walk of lane 0 over at most 32 detections; the rows of the frame are written by the lanes p < P and d < D at its end.
// The block is one wave, so its barriers cost nothing on the device; they are what orders the lanes' LDS traffic.
constexpr int kTrackMaxP = 16, kTrackMaxD = 32, kTrackPairs = kTrackMaxP * kTrackMaxD / 64;
constexpr unsigned long long kQuietNaN = 0x7ff8000000000000ull;

__global__ __launch_bounds__(64) void track_assign_kernel(const double* __restrict__ dets, const int* __restrict__ stream_of, int F,
                                                          int D, int P, int K, double* __restrict__ ref, int* __restrict__ age,
                                                          double min_iou, int max_missed, int box_format,
                                                          double* __restrict__ boxes_out, int* __restrict__ restart,
                                                          int* __restrict__ track_of) {
  __shared__ double s_ref[kTrackMaxP][4];
  __shared__ double s_box[kTrackMaxD][4];
  __shared__ int s_age[kTrackMaxP], s_row[kTrackMaxP], s_restart[kTrackMaxP], s_done[kTrackMaxP];
  __shared__ int s_usable[kTrackMaxD], s_track[kTrackMaxD];
  const int k = blockIdx.x, lane = threadIdx.x;
  if (lane < P) {
    s_age[lane] = age[(long)k * P + lane];
    for (int j = 0; j < 4; ++j) s_ref[lane][j] = ref[((long)k * P + lane) * 4 + j];
  }
  __syncthreads();
  const unsigned long long* const dets_bits = reinterpret_cast<const unsigned long long*>(dets);
  unsigned long long* const out_bits = reinterpret_cast<unsigned long long*>(boxes_out);
  for (int f = 0; f < F; ++f) {
    const int kf = stream_of ? stream_of[f] : 0;
    const bool in_range = kf >= 0 && kf < K;
    if (in_range ? kf != k : k != 0) continue;                // (uniform over the block: f and k are)
    if (!in_range) {                                          // no stream: block 0 says so, no state is touched
      if (lane < P) {
        for (int j = 0; j < 4; ++j) out_bits[((long)f * P + lane) * 4 + j] = kQuietNaN;
        restart[(long)f * P + lane] = 0;
      }
      if (lane < D) track_of[(long)f * D + lane] = -1;
      continue;
    }
    // the frame's detections, one a lane: the box and whether it can be used; s_done[p]: the row of track p is decided
    if (lane < D) {
      const double* const b = dets + ((long)f * D + lane) * 4;
      double x0 = b[0], y0 = b[1], x1 = b[2], y1 = b[3];
      if (box_format == 1) { x1 = b[0] + b[2]; y1 = b[1] + b[3]; }
      s_box[lane][0] = x0; s_box[lane][1] = y0; s_box[lane][2] = x1; s_box[lane][3] = y1;
      s_usable[lane] = crop_in_range(x0) && crop_in_range(y0) && crop_in_range(x1) && crop_in_range(y1) && x1 > x0 && y1 > y0;
      s_track[lane] = -1;
    }
    if (lane < P) { s_done[lane] = 0; s_row[lane] = -1; s_restart[lane] = 0; }
    __syncthreads();
    // the IoU of the lane's pairs; -1 where the track is free or the detection unusable
    double iou[kTrackPairs];
    for (int j = 0; j < kTrackPairs; ++j) {
      const int idx = lane + 64 * j;
      iou[j] = -1.0;
      if (idx >= P * D) continue;
      const int p = idx / D, d = idx % D;
      if (s_age[p] < 0 || !s_usable[d]) continue;
      const double ax0 = s_ref[p][0], ay0 = s_ref[p][1], ax1 = s_ref[p][2], ay1 = s_ref[p][3];
      const double bx0 = s_box[d][0], by0 = s_box[d][1], bx1 = s_box[d][2], by1 = s_box[d][3];
      const double iw = (ax1 < bx1 ? ax1 : bx1) - (ax0 > bx0 ? ax0 : bx0), ih = (ay1 < by1 ? ay1 : by1) - (ay0 > by0 ? ay0 : by0);
      double v = 0.0;
      if (iw > 0.0 && ih > 0.0) {
        const double inter = iw * ih;
        const double area_a = (ax1 - ax0) * (ay1 - ay0), area_b = (bx1 - bx0) * (by1 - by0);
        v = inter / ((area_a + area_b) - inter);
      }
      iou[j] = v;
    }
    // 1. match: the best remaining pair, until none reaches min_iou
    for (int round = 0; round < kTrackMaxP; ++round) {
      double best = -1.0;
      int best_idx = 0x7fffffff;
      for (int j = 0; j < kTrackPairs; ++j) {
        const int idx = lane + 64 * j;
        if (idx >= P * D || !(iou[j] >= 0.0)) continue;
        if (s_done[idx / D] || s_track[idx % D] >= 0) continue;
        if (iou[j] > best || (iou[j] == best && idx < best_idx)) { best = iou[j]; best_idx = idx; }
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(best, off);
        const int oi = __shfl_xor(best_idx, off);
        if (o > best || (o == best && oi < best_idx)) { best = o; best_idx = oi; }
      }
      if (best_idx == 0x7fffffff || !(best >= min_iou)) break;   // (the same on every lane)
      if (lane == 0) {
        const int p = best_idx / D, d = best_idx % D;
        for (int j = 0; j < 4; ++j) s_ref[p][j] = s_box[d][j];
        s_age[p] = 0;
        s_done[p] = 1;
        s_row[p] = d;
        s_track[d] = p;
      }
      __syncthreads();
    }
    __syncthreads();
    // 2. age: a live track without a match waits, or dies past max_missed
    if (lane < P && s_age[lane] >= 0 && !s_done[lane]) {
      s_age[lane] = s_age[lane] + 1;
      if (s_age[lane] > max_missed) { s_age[lane] = -1; s_restart[lane] = 1; }
      s_done[lane] = 1;
    }
    __syncthreads();
    // 3. births: the detections left over, in ascending d, each into the lowest free slot
    if (lane == 0) {
      int p = 0;
      for (int d = 0; d < D; ++d) {
        if (!s_usable[d] || s_track[d] >= 0) continue;
        while (p < P && s_age[p] >= 0) ++p;
        if (p >= P) break;
        for (int j = 0; j < 4; ++j) s_ref[p][j] = s_box[d][j];
        s_age[p] = 0;
        s_done[p] = 1;
        s_row[p] = d;
        s_restart[p] = 1;
        s_track[d] = p;
      }
    }
    __syncthreads();
    // 4. the frame's rows: a track's detection bit for bit, or the quiet NaN
    if (lane < P) {
      const int d = s_row[lane];
      for (int j = 0; j < 4; ++j)
        out_bits[((long)f * P + lane) * 4 + j] = d < 0 ? kQuietNaN : dets_bits[((long)f * D + d) * 4 + j];
      restart[(long)f * P + lane] = s_restart[lane];
    }
    if (lane < D) track_of[(long)f * D + lane] = s_track[lane];
    __syncthreads();
  }
  if (lane < P) {
    age[(long)k * P + lane] = s_age[lane];
    for (int j = 0; j < 4; ++j) ref[((long)k * P + lane) * 4 + j] = s_ref[lane][j];
  }
}

// The present rows of the tracker's windows, first and in order (include/emo_hip.h, ABI 27; hostglue.present_rows is the contract):
// a stable stream compaction in one block.  Thread t owns the contiguous run of rows [t * run, (t + 1) * run), run = ceil(M /
// threads): it counts the present rows of its run, the run totals meet in LDS behind the one barrier, every thread sums the totals
// in front of it and walks its run again, writing each present row at its place; the thread that meets the first row of a frame
// books the frame (first, count).  The rows behind the T present ones are filled by all threads, strided.  A window row is one
// 16-byte load and one 16-byte store.  Only sums of integers: the result does not depend on the number of threads.
constexpr int kPresentThreads = 256;
struct alignas(16) WindowRow { int x, y, w, h; };

__global__ __launch_bounds__(kPresentThreads) void present_rows_kernel(const WindowRow* __restrict__ crop,
                                                                       const WindowRow* __restrict__ paste, int F, int P,
                                                                       int* __restrict__ count, int* __restrict__ first,
                                                                       int* __restrict__ row_of, WindowRow* __restrict__ crop_out,
                                                                       WindowRow* __restrict__ paste_out) {
  __shared__ int s_total[kPresentThreads];
  const int M = F * P, t = threadIdx.x, nt = blockDim.x;       // (nt <= kPresentThreads: the launch below)
  const int run = (M + nt - 1) / nt;                           // (M <= 2^24: t * run stays below 2^25)
  const int lo = t * run < M ? t * run : M, hi = M - lo < run ? M : lo + run;
  int mine = 0;
  for (int i = lo; i < hi; ++i) mine += paste[i].w > 0;
  s_total[t] = mine;
  __syncthreads();
  int before = 0, total = 0;
  for (int u = 0; u < nt; ++u) {
    if (u == t) before = total;
    total += s_total[u];
  }
  int j = before;
  for (int i = lo; i < hi; ++i) {
    if (i % P == 0) {                                          // the first row of frame i / P: the frame is this thread's to book
      int c = 0;
      for (int p = 0; p < P; ++p) c += paste[i + p].w > 0;
      first[i / P] = j;
      count[i / P] = c;
    }
    const WindowRow w = paste[i];
    if (w.w > 0) {
      row_of[j] = i;
      crop_out[j] = crop[i];
      paste_out[j] = w;
      ++j;
    }
  }
  if (t == 0) first[F] = total;
  const WindowRow none = {0, 0, 0, 0};
  for (int k = total + t; k < M; k += nt) {
    row_of[k] = -1;
    crop_out[k] = none;
    paste_out[k] = none;
  }
}

}  // namespace

extern "C" int emo_present_rows_i32(const int32_t* crop, const int32_t* paste, int F, int P, int32_t* count, int32_t* first,
                                    int32_t* row_of, int32_t* crop_out, int32_t* paste_out, void* stream) {
  if (!crop || !paste || !count || !first || !row_of || !crop_out || !paste_out) return EMO_ERR_BAD_ARG;
  if (F <= 0 || P < 1 || P > kTrackMaxP || (long)F * P > (1l << 24)) return EMO_ERR_BAD_ARG;
  const long M = (long)F * P;
  const struct { const void* p; long bytes; } in[2] = {{crop, M * 16}, {paste, M * 16}},
      out[5] = {{count, F * 4l}, {first, (F + 1) * 4l}, {row_of, M * 4}, {crop_out, M * 16}, {paste_out, M * 16}};
  for (const auto& o : out)
    for (const auto& i : in) {
      const uintptr_t a = (uintptr_t)o.p, b = (uintptr_t)i.p;
      if (a < b + (uintptr_t)i.bytes && b < a + (uintptr_t)o.bytes) return EMO_ERR_BAD_ARG;
    }
  if ((((uintptr_t)crop | (uintptr_t)paste | (uintptr_t)crop_out | (uintptr_t)paste_out) & 15) != 0) return EMO_ERR_ALIGN;
  hipLaunchKernelGGL(present_rows_kernel, dim3(1), dim3(kPresentThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const WindowRow*>(crop), reinterpret_cast<const WindowRow*>(paste), F, P, count, first, row_of,
                     reinterpret_cast<WindowRow*>(crop_out), reinterpret_cast<WindowRow*>(paste_out));
  return emo_launch_status();
}

extern "C" int emo_track_assign_f64(const double* dets, const int32_t* stream_of, int F, int D, int P, int K, double* ref,
                                    int32_t* age, double min_iou, int max_missed, int box_format, double* boxes_out,
                                    int32_t* restart, int32_t* track_of, void* stream) {
  if (!dets || !ref || !age || !boxes_out || !restart || !track_of) return EMO_ERR_BAD_ARG;
  if (F <= 0 || D <= 0 || P <= 0 || K <= 0 || P > kTrackMaxP || D > kTrackMaxD) return EMO_ERR_BAD_ARG;
  if (!(min_iou > 0.0 && min_iou <= 1.0) || max_missed < 0 || (box_format != 0 && box_format != 1)) return EMO_ERR_BAD_ARG;
  hipLaunchKernelGGL(track_assign_kernel, dim3(K), dim3(64), 0, (hipStream_t)stream, dets, stream_of, F, D, P, K, ref, age, min_iou,
                     max_missed, box_format, boxes_out, restart, track_of);
  return emo_launch_status();
}

extern "C" int emo_crop_track_restarts_f64(const double* boxes, const int32_t* stream_of, const int32_t* sizes, int Wf, int Hf,
                                           double* state, int32_t* has_state, int32_t* last, int M, int K, double m, double om,
                                           int smooth, int fixed, double scale, int box_format, int hold, int min_side,
                                           const int32_t* restart, int32_t* crop, int32_t* paste, double* face_scale, void* stream) {
  if (!boxes || !crop || !paste || M <= 0 || K <= 0) return EMO_ERR_BAD_ARG;
  if (!sizes && (Wf < 1 || Hf < 1)) return EMO_ERR_BAD_ARG;
  if (smooth && (!state || !has_state)) return EMO_ERR_BAD_ARG;
  if (hold && !last) return EMO_ERR_BAD_ARG;
  if (!(m > 0.0 && m <= 1.0) || !(om >= 0.0 && om < 1.0)) return EMO_ERR_BAD_ARG;
  if (!((scale - scale) == 0.0) || (box_format != 0 && box_format != 1) || min_side < 1) return EMO_ERR_BAD_ARG;
  hipLaunchKernelGGL(crop_track_kernel, dim3(emo_cdiv(K, 64)), dim3(64), 0, (hipStream_t)stream, boxes, stream_of, sizes, Wf, Hf,
                     state, has_state, last, M, K, m, om, smooth ? 1 : 0, fixed ? 1 : 0, scale, box_format, hold ? 1 : 0, min_side,
                     restart, crop, paste, face_scale);
  return emo_launch_status();
}

extern "C" int emo_crop_track_f64(const double* boxes, const int32_t* stream_of, const int32_t* sizes, int Wf, int Hf, double* state,
                                  int32_t* has_state, int32_t* last, int M, int K, double m, double om, int smooth, int fixed,
                                  double scale, int box_format, int hold, int min_side, int32_t* crop, int32_t* paste,
                                  double* face_scale, void* stream) {
  return emo_crop_track_restarts_f64(boxes, stream_of, sizes, Wf, Hf, state, has_state, last, M, K, m, om, smooth, fixed, scale,
                                     box_format, hold, min_side, nullptr, crop, paste, face_scale, stream);
}

extern "C" int emo_small_gemm_f32(const float* A, const float* B, float* C, int M, int K, int NN, int batch,
                                  int64_t b_stride, int64_t c_stride, void* stream) {
  if (!A || !B || !C || M <= 0 || K <= 0 || batch <= 0) return EMO_ERR_BAD_ARG;
  if (batch > 65535) return EMO_ERR_UNSUPPORTED;
  dim3 g(emo_cdiv(M, 4), batch);
  hipStream_t s = (hipStream_t)stream;
  switch (NN) {
    case 1: hipLaunchKernelGGL(small_gemm_kernel<1>, g, dim3(256), 0, s, A, B, C, M, K, (long)b_stride, (long)c_stride); break;
    case 2: hipLaunchKernelGGL(small_gemm_kernel<2>, g, dim3(256), 0, s, A, B, C, M, K, (long)b_stride, (long)c_stride); break;
    case 4: hipLaunchKernelGGL(small_gemm_kernel<4>, g, dim3(256), 0, s, A, B, C, M, K, (long)b_stride, (long)c_stride); break;
    case 16: hipLaunchKernelGGL(small_gemm_kernel<16>, g, dim3(256), 0, s, A, B, C, M, K, (long)b_stride, (long)c_stride); break;
    default: return EMO_ERR_UNSUPPORTED;
  }
  return emo_launch_status();
}

extern "C" int emo_projector_finalize_f32(const float* T, const float* V, const int* norm_of_row, const float* gamma,
                                          const float* beta, float* ada_gamma, float* ada_beta, int B, int R, int E,
                                          void* stream) {
  if (!T || !V || !norm_of_row || !gamma || !beta || !ada_gamma || !ada_beta || B <= 0 || R <= 0 || E <= 0)
    return EMO_ERR_BAD_ARG;
  hipLaunchKernelGGL(projector_finalize_kernel, dim3(emo_cdiv((long)B * R, 256)), dim3(256), 0, (hipStream_t)stream, T,
                     V, norm_of_row, gamma, beta, ada_gamma, ada_beta, B, R, E);
  return emo_launch_status();
}

extern "C" int emo_pose_theta_f32(const float* scale, int scale_cols, const float* rotation, const float* translation,
                                  float* theta, int B, void* stream) {
  if (!scale || !rotation || !translation || !theta || B <= 0) return EMO_ERR_BAD_ARG;
  if (scale_cols != 1 && scale_cols != 3) return EMO_ERR_BAD_ARG;
  hipLaunchKernelGGL(pose_theta_kernel, dim3(emo_cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, scale, scale_cols,
                     rotation, translation, theta, B);
  return emo_launch_status();
}

extern "C" int emo_pack_rgb8(const float* img, uint8_t* out, int N, int H, int W, void* stream) {
  if (!img || !out || N <= 0 || H <= 0 || W <= 0) return EMO_ERR_BAD_ARG;
  const long total = (long)N * H * W;
  long g = (total + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(pack_rgb8_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, img, out, (long)N,
                     (long)H * W);
  return emo_launch_status();
}

extern "C" int emo_unpack_rgb8(const uint8_t* in, float* out, int N, int H, int W, void* stream) {
  if (!in || !out || N <= 0 || H <= 0 || W <= 0) return EMO_ERR_BAD_ARG;
  const long total = (long)N * H * W;
  long g = (total + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(unpack_rgb8_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, in, out, (long)N,
                     (long)H * W);
  return emo_launch_status();
}

extern "C" int emo_mat4_inverse_f32(const float* in, float* out, int B, void* stream) {
  if (!in || !out || B <= 0) return EMO_ERR_BAD_ARG;
  hipLaunchKernelGGL(mat4_inverse_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, in, out, B);
  return emo_launch_status();
}

extern "C" int emo_mixing_theta_f32(const float* target, const float* source, const int32_t* index, int B, int K, int mix_old,
                                    float* out, void* stream) {
  if (!target || !source || !out || B <= 0 || K <= 0) return EMO_ERR_BAD_ARG;
  hipLaunchKernelGGL(mixing_theta_kernel, dim3(emo_cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, target, source, index, B, K,
                     mix_old ? 1 : 0, out);
  return emo_launch_status();
}

extern "C" int emo_theta_ema_scan_tracks_f32(const float* values, const int32_t* stream_of, float* state, int32_t* has_state, int n,
                                             int K, float m, float om, const int32_t* restart, const int32_t* present, float* out,
                                             void* stream) {
  if (!values || !state || !has_state || !out || n <= 0 || K <= 0) return EMO_ERR_BAD_ARG;
  hipLaunchKernelGGL(theta_ema_scan_kernel, dim3(emo_cdiv(K, 64)), dim3(64), 0, (hipStream_t)stream, values, stream_of, state,
                     has_state, n, K, m, om, restart, present, out);
  return emo_launch_status();
}

extern "C" int emo_theta_ema_scan_f32(const float* values, const int32_t* stream_of, float* state, int32_t* has_state, int n, int K,
                                      float m, float om, float* out, void* stream) {
  return emo_theta_ema_scan_tracks_f32(values, stream_of, state, has_state, n, K, m, om, nullptr, nullptr, out, stream);
}

extern "C" int emo_expr_controls_tracks_f32(const float* values, const int32_t* stream_of, const float* neutral, const float* gain,
                                            const float* offset, float* anchor, int32_t* has_anchor, float* ema, int32_t* has_ema,
                                            int n, int K, int E, int relative, int smooth, float m, float om,
                                            const int32_t* restart, const int32_t* present, float* out, void* stream) {
  if (!values || !out || n <= 0 || K <= 0 || E <= 0) return EMO_ERR_BAD_ARG;
  if ((relative || gain) && !neutral) return EMO_ERR_BAD_ARG;
  if (relative && (!anchor || !has_anchor)) return EMO_ERR_BAD_ARG;
  if (smooth && (!ema || !has_ema)) return EMO_ERR_BAD_ARG;
  const int threads = E >= 128 ? 128 : emo_cdiv(E, 64) * 64;
  hipLaunchKernelGGL(expr_controls_kernel, dim3(K), dim3(threads), 0, (hipStream_t)stream, values, stream_of, neutral, gain, offset,
                     anchor, has_anchor, ema, has_ema, n, E, relative ? 1 : 0, smooth ? 1 : 0, m, om, restart, present, out);
  return emo_launch_status();
}

extern "C" int emo_expr_controls_f32(const float* values, const int32_t* stream_of, const float* neutral, const float* gain,
                                     const float* offset, float* anchor, int32_t* has_anchor, float* ema, int32_t* has_ema, int n,
                                     int K, int E, int relative, int smooth, float m, float om, float* out, void* stream) {
  return emo_expr_controls_tracks_f32(values, stream_of, neutral, gain, offset, anchor, has_anchor, ema, has_ema, n, K, E, relative,
                                      smooth, m, om, nullptr, nullptr, out, stream);
}

extern "C" int emo_head_pose_controls_tracks_f32(const float* scale, int scale_cols, const float* rotation, const float* translation,
                                                 const int32_t* stream_of, const float* source, const float* gain,
                                                 const float* rotation_offset, const float* translation_offset, const float* zoom,
                                                 float* anchor, int32_t* has_anchor, int n, int K, int relative, int frontal,
                                                 const int32_t* restart, const int32_t* present, float* out_srt, float* out_theta,
                                                 void* stream) {
  if (!scale || !rotation || !translation || !out_srt || !out_theta || n <= 0 || K <= 0) return EMO_ERR_BAD_ARG;
  if (scale_cols != 1 && scale_cols != 3) return EMO_ERR_BAD_ARG;
  if ((relative || gain) && !source) return EMO_ERR_BAD_ARG;
  if (relative && (!anchor || !has_anchor)) return EMO_ERR_BAD_ARG;
  if (relative && frontal) return EMO_ERR_BAD_ARG;
  hipLaunchKernelGGL(head_pose_controls_kernel, dim3(K), dim3(64), 0, (hipStream_t)stream, scale, scale_cols, rotation, translation,
                     stream_of, source, gain, rotation_offset, translation_offset, zoom, anchor, has_anchor, n, relative ? 1 : 0,
                     frontal ? 1 : 0, restart, present, out_srt, out_theta);
  return emo_launch_status();
}

extern "C" int emo_head_pose_controls_f32(const float* scale, int scale_cols, const float* rotation, const float* translation,
                                          const int32_t* stream_of, const float* source, const float* gain,
                                          const float* rotation_offset, const float* translation_offset, const float* zoom,
                                          float* anchor, int32_t* has_anchor, int n, int K, int relative, int frontal,
                                          float* out_srt, float* out_theta, void* stream) {
  return emo_head_pose_controls_tracks_f32(scale, scale_cols, rotation, translation, stream_of, source, gain, rotation_offset,
                                           translation_offset, zoom, anchor, has_anchor, n, K, relative, frontal, nullptr, nullptr,
                                           out_srt, out_theta, stream);
}
