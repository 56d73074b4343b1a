// 3x3x3 layers on 32-row channel tiles (fp16 two-term split, block config F): the depth-shared form of conv_igemm_bf16x3.h.
//
// conv_igemm_bf16x3_kernel<4, 64, false, 2, 32> runs the depth taps of a 3-D layer as K stages of a one-slice position tile:
// stage = (16-channel chunk, kd).  The (4 + 2) x (64 + 2) patch of input slice z is therefore loaded, sent through affine + ReLU
// + range check, split into two fp16 planes and stored to LDS THREE times -- once for each output slice z - 1, z, z + 1 that
// reads it -- and with 32 output channels a stage feeds only 54 MFMAs per wave (1.7 k matrix cycles) against about 1.5 k cycles
// of staging, barrier and waits per stage.
//
// Here a work item is (sample, y-x tile, channel tile, RUN of output slices) and marches in z.  Input slice zi of chunk cc is
// staged ONCE and feeds the MFMAs of every depth tap that reads it: with the kd = 0, 1, 2 kernels of cc it is accumulated into
// the live accumulator sets of output slices zi + 1, zi, zi - 1.  Slices run outermost, chunks inside, so output slice z is
// complete -- and goes through the epilogue -- when input slice z + 1 has been consumed; three accumulator sets (leading product
// + small products each: 3 x 2 x 32 = 192 registers) hold the outputs of taps 0, 1, 2 and move up one role per slice.
//   staged patch elements per MFMA     before  16 x 6 x 66 / 54        = 117
//                                      after   16 x 6 x 66 / (54 x 3)  =  39  in the interior of a run; a run of R output slices
//                                              stages R + 2 input slices (one fewer at each end of the volume): x (R + 2) / R
//                                              -- 41 for R = 32, 52 for R = 6 (the shortest run the launcher takes)
// Arithmetic per output value as before: leading product -> its own accumulator, the two cross products -> the second set, fp32;
// the sets are combined and scaled in the shared epilogue (conv_epilogue_fast_* / conv_epilogue_rows).  Only the order in which
// an output's (chunk, kd) contributions arrive changes: kd outermost instead of chunk outermost.
//
// LDS (143.5 KB, one block of four waves per CU, one wave per SIMD):
//   P      one patch buffer of ConvCfgS<4, 64, false, 2, 32> (29.0 KB, both planes) -- SINGLE-buffered: the next stage's patch is
//          loaded into registers in front of the stage's MFMAs, converted (registers to registers) beside the MFMAs of its last
//          four steps and stored between the two barriers that end the stage
//   W[2]   two weight stages of 54 KB: the three depth taps of a chunk ([co tile][chunk][kd][row] ...: contiguous in the packed
//          tensor), the next stage's by LDS-DMA during the MFMAs.  The idle one is the epilogue's transposition scratch
//   tables scale / shift of <= 256 input channels, bias, the (mean, M2) exchange of the tile statistics
// Everything the launch promises is the sibling kernel's: zero padding after affine + ReLU in all three axes (an input slice
// outside the volume is not staged at all), range check with the overflow word, residual, bias, activation, tile statistics in
// the TileStats layout (one entry per 4 x 64 tile of one output slice), ragged channel tile, Cin % 8 == 0.
//
// Included behind conv_igemm_bf16x3.h (whose helpers, configuration and epilogues it uses) by conv_inst_f16x2_zs.hip; the
// __global__ wrapper with the LDS declaration lives there.
#pragma once

#ifndef EMO_Z_CONV_EARLY
#define EMO_Z_CONV_EARLY 1   /* 0: A/B builds -- the next patch is converted between the two barriers that end a stage */
#endif

struct ConvCfgZ {
  using S = ConvCfgS<4, 64, false, 2, 32>;
  static constexpr int TR = 4, TW = 64, BM = 32, TP = 2, WGP = 4, KC = 16, NPL = 2;
  static constexpr int WST = 3 * S::WROW;               // one (chunk, kd) stage of weights, 16-byte slots
  static constexpr int WCH = 3 * WST;                   // the three depth taps of a chunk
  static constexpr int NPIECE = WCH * 16 / 1024;        // 1 KiB DMA pieces of a chunk
  static constexpr int NDMA = (NPIECE + 3) / 4;         // pieces EVERY wave issues (the last round re-copies: uniform counts)
  static constexpr int OFF_P = 0;
  static constexpr int OFF_W = S::PBUF;
  static constexpr int OFF_SCT = OFF_W + 2 * WCH;
  static constexpr int SCT = 256;                       // input channels of the scale / shift tables
  static constexpr int OFF_BIAS_F = OFF_SCT * 4 + 2 * SCT;
  static constexpr int OFF_STAT_F = OFF_BIAS_F + BM;
  static constexpr int LDS_BYTES = (OFF_STAT_F + 2 * WGP * BM) * 4;
  static constexpr int EPI_ROWF = S::EPI_ROWF, EPI_WAVE = S::EPI_WAVE;
  static_assert(NPIECE * 1024 == WCH * 16 && NPIECE >= 4 * (NDMA - 1) + 2, "whole pieces; the last round holds >= 2");
  static_assert(WGP * EPI_WAVE * 4 <= WCH * 16, "the epilogue transposes through the idle weight stage");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

// the MFMAs of depth taps KD0 .. KD1 of one staged (slice, chunk): 9 steps (kernel row r, tap column s); a step reads the patch
// fragments once for all its taps -- 4 + 2 (KD1 - KD0 + 1) ds_read_b128 for 6 (KD1 - KD0 + 1) MFMAs --, one step ahead.
// w_off: byte offset of the lane's weight fragment in the stage buffer; lo0 / hi0 .. lo2 / hi2: the accumulator sets of taps 0 .. 2
// convert(i), i = 0 .. 3: the conversion of pixel i of the NEXT stage's patch (registers to registers), placed in steps 5 .. 8 --
// 45 vector instructions beside 18 MFMAs: inside the five an MFMA gap hides
template <int KD0, int KD1, typename F>
__device__ __forceinline__ void conv_zs_mma(const char* lds_c, int w_off, const int (&b_off)[2][1][3],
                                            floatx16 (&lo0)[1][2], floatx16 (&hi0)[1][2], floatx16 (&lo1)[1][2],
                                            floatx16 (&hi1)[1][2], floatx16 (&lo2)[1][2], floatx16 (&hi2)[1][2], F&& convert) {
  using Cfg = ConvCfgZ;
  using S = Cfg::S;
  constexpr int NK = KD1 - KD0 + 1;
  constexpr int PA3[3] = {1, 0, 0}, PB3[3] = {0, 1, 0};   // (weight plane, patch plane), smallest product first
  halfx8 fa[2][NK][2], fb[2][2][2];
#define EMO_Z_FRAGS(set_, r_, s_)                                                                                     \
  {                                                                                                                   \
    _Pragma("unroll") for (int pl = 0; pl < 2; ++pl)                                                                  \
      _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                   \
        fb[set_][pl][j] = *reinterpret_cast<const halfx8*>(lds_c + b_off[j][0][s_] + ((r_) * S::NQ1 + Cfg::OFF_P + pl * S::PPL) * 16); \
    _Pragma("unroll") for (int k = 0; k < NK; ++k)                                                                    \
      _Pragma("unroll") for (int pl = 0; pl < 2; ++pl)                                                                \
        fa[set_][k][pl] = *reinterpret_cast<const halfx8*>(lds_c + w_off + ((KD0 + k) * Cfg::WST + (r_) * S::WROW + pl * S::WPLANE + (s_) * 2 * Cfg::BM) * 16); \
  }
  EMO_Z_FRAGS(0, 0, 0)
#pragma unroll
  for (int gs = 0; gs < 9; ++gs) {
    const int cur = gs & 1, nxt = cur ^ 1;
    __builtin_amdgcn_sched_barrier(0);
    if (gs < 8) EMO_Z_FRAGS(nxt, (gs + 1) / 3, (gs + 1) % 3)
    if (EMO_Z_CONV_EARLY && gs >= 5) convert(gs - 5);
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int kd = KD0 + k;
          const bool lead = PA3[p] == 0 && PB3[p] == 0;
          floatx16& acc_ = kd == 0 ? (lead ? lo0[0][j] : hi0[0][j]) : kd == 1 ? (lead ? lo1[0][j] : hi1[0][j]) : (lead ? lo2[0][j] : hi2[0][j]);
          acc_ = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[cur][PB3[p]][j], fa[cur][k][PA3[p]], acc_, 0, 0, 0);
        }
    if (EMO_Z_CONV_EARLY && gs >= 5) {
      // { MFMA, fragment read, <= 3 conversion instructions } ..., { MFMA, <= 3 conversion instructions } ...
#pragma unroll
      for (int k = 0; k < 6 * NK; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (gs < 8 && k < 4 + 2 * NK) __builtin_amdgcn_sched_group_barrier(0x100, (4 + 2 * NK + 6 * NK - 1) / (6 * NK), 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
      }
    } else if (gs < 8) {
      // { MFMA, fragment read } for the reads of the next step, the remaining MFMAs behind them
#pragma unroll
      for (int k = 0; k < 4 + 2 * NK && k < 6 * NK; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, (4 + 2 * NK + 6 * NK - 1) / (6 * NK), 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#undef EMO_Z_FRAGS
}

__device__ __forceinline__ void conv_f16x2_zs_body(const ConvArgs& a, float* smem, const unsigned smem_lds) {
  using Cfg = ConvCfgZ;
  using S = Cfg::S;
  constexpr int BM = Cfg::BM, TP = Cfg::TP, WGP = Cfg::WGP, KC = Cfg::KC, TW = Cfg::TW, TR = Cfg::TR;
  constexpr int PR = S::PR, NQ = S::NQ, NQ1 = S::NQ1, SUB = S::SUB, CHS = S::CHS, QPG = S::QPG, NHQ = S::NHQ, PPL = S::PPL;
  // (names of the shared macros, conv_split_common.h: no upsampling gather; one 32-channel tile of the fp16 split)
  constexpr bool UPS = false;
  constexpr int TWS = TW, TM = 1, SPLIT = 2;

  EMO_SPLIT_THREAD_IDS()
  const int wp = wave;
  const int p0 = wp * TP * 32;
  float sat_m = 0.0f;                                    // largest |scaled staged value| this thread has seen

  const int HW = a.H * a.W;
  const long DHW = (long)a.D * HW;
  const bool has_affine = a.scale != nullptr;
  const int epi_mode = __builtin_amdgcn_readfirstlane(     // as in conv_igemm_bf16x3_kernel: 0 / 1 the straight-line epilogue
      (a.act != EMO_ACT_NONE || a.Cout % BM != 0 || (long)a.Dl * a.Hl * a.Wl > (1l << 23) ||
       (reinterpret_cast<unsigned long long>(a.out) & 15ull) != 0) ? -1
      : a.res == nullptr ? 0
      : (!a.res_ups && (reinterpret_cast<unsigned long long>(a.res) & 15ull) == 0) ? 1 : -1);
  constexpr float CLAMP_HI = 65504.0f;
  const float clamp_lo = a.relu_in ? 0.0f : -CLAMP_HI;
  const int ncc = a.n_cchunks;
  const int nruns = (a.D + a.zrun - 1) / a.zrun;

  // ---- staging map, fragment offsets (bytes): weight fragment of the lane, and for every tap column the patch slot of its two
  //      output pixels (conv_split_common.h) ----
  EMO_SPLIT_STAGING_MAP(tid / QPG, 0)
  const int a_off = (half * BM + l32) * 16;
  EMO_SPLIT_DECLARE_B_OFF()
  EMO_SPLIT_LDS_VIEWS()
  float* const sct = smem + Cfg::OFF_SCT * 4;         // (EMO_SPLIT_LDS_TABLES_ADDR without smem_lds, a parameter here)
  const unsigned lane16 = (unsigned)lane * 16u;
  EMO_SPLIT_USOFF(8, 0, DHW, 1u)

  floatx4 qv[8];                 // the raw patch of the next stage: 8 channels x one quad
  halfx8 cv_h[4], cv_m[4];       // ... converted: the two planes of its four pixels
  floatx4 q_sc[2], q_sh[2];
  float q_lo = 0.0f, q_hi = 0.0f;
  int q_tix = 0;
  floatx16 acc_lo[3][1][2], acc_hi[3][1][2];

  for (int L = blockIdx.x; L < a.n_work; L += gridDim.x) {
    // item -> (sample, y tile, x tile, run, channel tile), channel tile fastest
    int rest = L;
    const int cot_ = rest % a.n_cotiles; rest /= a.n_cotiles;
    const int run_ = rest % nruns; rest /= nruns;
    const int tx_ = rest % a.tiles_x; rest /= a.tiles_x;
    const int ty_ = rest % a.tiles_y; rest /= a.tiles_y;
    const int it_cotile = __builtin_amdgcn_readfirstlane(cot_);
    const int it_n = __builtin_amdgcn_readfirstlane(rest);
    const int it_x0 = __builtin_amdgcn_readfirstlane(tx_ * TW), it_y0 = __builtin_amdgcn_readfirstlane(ty_ * TR);
    const int ptile_yx = __builtin_amdgcn_readfirstlane(ty_ * a.tiles_x + tx_);
    const int zb = __builtin_amdgcn_readfirstlane(run_ * a.zrun);
    const int nout = min(a.zrun, a.D - zb);                 // output slices zb .. zb + nout - 1
    const int zi_last = min(zb + nout, a.D - 1);            // input slices max(zb - 1, 0) .. zi_last
    const int zi_first = zb > 0 ? zb - 1 : 0;

    bool lq_ok;
    unsigned lq_off;
    EMO_SPLIT_CURSOR_OF(it_, lq_ok, lq_off)
    const emo_intx4 xrs = emo_raw_buffer(a.x + (long)it_n * a.Cin * DHW);
    const char* const wsrc = reinterpret_cast<const char*>(a.wpk) + (long)it_cotile * ncc * (Cfg::WCH * 16);

// weights of chunk cc_ (its three depth taps) into W[wb_] by LDS-DMA; patch loads of (slice zi_, chunk cc_) into qv
#define EMO_Z_ISSUE(zi_, cc_, wb_)                                                                                    \
  {                                                                                                                   \
    const char* const wp_ = wsrc + (long)(cc_) * (Cfg::WCH * 16);                                                     \
    _Pragma("unroll") for (int k = 0; k < Cfg::NDMA; ++k) {                                                           \
      const int j = k < Cfg::NDMA - 1 ? wave + 4 * k : 4 * (Cfg::NDMA - 1) + (wave & 1);                              \
      emo_dma16_pinned_s(wp_ + j * 1024, lane16, smem_lds + (unsigned)((Cfg::OFF_W + (wb_) * Cfg::WCH) * 16 + j * 1024)); \
    }                                                                                                                 \
    const int c0_ = (cc_) * KC + q_g * 8;                                                                             \
    const bool cv_ = c0_ < a.Cin;                                                                                     \
    const int cs_ = cv_ ? c0_ : 0;                                                                                    \
    const bool keep_ = lq_ok && cv_;                                                                                  \
    q_lo = keep_ ? clamp_lo : 0.0f;                                                                                   \
    q_hi = keep_ ? CLAMP_HI : 0.0f;                                                                                   \
    q_tix = cs_ >> 2;                                                                                                 \
    const unsigned q_vo = lq_off + ((unsigned)cs_ * (unsigned)DHW + (unsigned)((zi_) * HW)) * 4u;                     \
    EMO_SPLIT_ISSUE_LOADS(qv, q_vo, 0, 8)                                                                             \
  }
// qv -> registers: pixel i_ of the lane's four through the conversion core (conv_split_common.h)
#define EMO_Z_CONVERT_PX(i_)                                                                                          \
  {                                                                                                                   \
    if ((i_) == 0) EMO_SPLIT_TABLE2(q_tix, q_sc, q_sh)    /* scale / shift of the lane's eight channels: read once per stage */ \
    _Pragma("unroll") for (int hf = 0; hf < 2; ++hf) {                                                                \
      EMO_SPLIT_AFFINE4(t_, qv, 4 * hf, i_, q_sc[hf], q_sh[hf])                                                       \
      EMO_SPLIT_RANGE4(t_)                                                                                            \
      EMO_SPLIT_F16X2_4(t_, q_lo, q_hi, cv_h[i_], cv_m[i_], 4 * hf)                                                   \
    }                                                                                                                 \
  }
// the converted pixels -> P (every lane stores all four pixels of its loads: its own, or into dump slots)
#define EMO_Z_STORE_PATCH()                                                                                           \
  {                                                                                                                   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                   \
      char* d_ = lds_w + q_slb[i] + Cfg::OFF_P * 16;                                                                  \
      EMO_SPLIT_STORE_PLANES(halfx8, d_, cv_h[i], cv_m[i])                                                            \
    }                                                                                                                 \
  }
#define EMO_Z_LANDED() { emo_wait_vmem0(); EMO_SPLIT_TOUCH(qv, 8) }

    // ---- prologue: tables and bias of the item, the first stage ----
    {
      float te_sc = 1.0f, te_sh = 0.0f, te_b = 0.0f;
      if (has_affine && tid < a.Cin) {
        te_sc = a.scale[(long)it_n * a.Cin + tid];
        te_sh = a.shift[(long)it_n * a.Cin + tid];
      }
      if (tid < BM && a.bias != nullptr) {
        const int co_ = it_cotile * BM + tid;
        te_b = a.bias[co_ < a.Cout ? co_ : a.Cout - 1];
      }
      if (tid < Cfg::SCT) {               // (in_scale: the split's power of two; channels past Cin: identity, never kept)
        sct[tid] = te_sc * a.in_scale;
        sct[Cfg::SCT + tid] = te_sh * a.in_scale;
      }
      // bias of the block's channels in the order the epilogue's row layout reads it (conv_epilogue_rows)
      if (tid < BM) smem[Cfg::OFF_BIAS_F + (tid >> 5) * 32 + (tid & 3) * 8 + ((tid & 31) >> 2)] = te_b;
    }
    __syncthreads();                      // tables visible (and the compiler's own loads above consumed: none is in flight
                                          // when the first pinned load goes out)
    EMO_Z_ISSUE(zi_first, 0, 0)
#pragma unroll
    for (int st = 0; st < 3; ++st)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc_lo[st][0][j][r] = 0.0f; acc_hi[st][0][j][r] = 0.0f; }
    EMO_Z_LANDED()
#pragma unroll
    for (int i = 0; i < 4; ++i) EMO_Z_CONVERT_PX(i)
    EMO_Z_STORE_PATCH()
    __syncthreads();                      // P and W[0] hold the first stage

    int wb = 0;                           // the weight stage buffer of the current stage
    // ---- the march.  Step t: input slice zb - 1 + t feeds output slices t - kd of the run; the accumulator sets have fixed
    //      roles -- set kd holds output t - kd -- and move up one role behind the step (128 register moves per slice against
    //      >= 324 MFMAs: with the sets rotated by index instead, the three copies of the loop body it takes cost more in
    //      accumulator traffic between the register files than the moves).  Outputs outside the run (t - kd < 0 or >= nout) are
    //      accumulated like the others and dropped: one code path, 2 (nout + 2) / nout - 2 extra MFMAs per seam ----
    for (int t = 0; t < nout + 2; ++t) {
      const int zi_ = zb - 1 + t;
      if ((unsigned)zi_ < (unsigned)a.D) {
        for (int cc = 0; cc < ncc; ++cc) {
          const bool last_cc_ = cc + 1 == ncc;
          const int nzi_ = last_cc_ ? zi_ + 1 : zi_, ncc_ = last_cc_ ? 0 : cc + 1;
          const bool has_next_ = nzi_ <= zi_last;
          // (past the item's last stage: a harmless re-stage of this one.  Issued under a branch, the loads' destination registers
          // would meet the previous stage's in a phi, and the compiler copies them right behind the loads, while they are in
          // flight -- the ISA audit's finding on an earlier form of this loop)
          EMO_Z_ISSUE(has_next_ ? nzi_ : zi_, has_next_ ? ncc_ : cc, wb ^ 1)
          auto convert_ = [&](int i) __attribute__((always_inline)) {
            if (i == 0) EMO_Z_LANDED()
            EMO_Z_CONVERT_PX(i)
          };
          conv_zs_mma<0, 2>(lds_c, a_off + (Cfg::OFF_W + wb * Cfg::WCH) * 16, b_off, acc_lo[0], acc_hi[0], acc_lo[1], acc_hi[1],
                            acc_lo[2], acc_hi[2], convert_);
          if (!EMO_Z_CONV_EARLY) {
#pragma unroll
            for (int i = 0; i < 4; ++i) convert_(i);
          }
          __syncthreads();                // every wave is past its last read of P and W[wb]
          EMO_Z_STORE_PATCH()
          __syncthreads();                // P and W[wb ^ 1] hold the next stage
          wb ^= 1;
        }
      }
      if (t >= 2) {
        // output slice zb + t - 2 is complete; scratch: the weight stage buffer the next stage does not use
        const int ep_n = it_n, ep_cotile = it_cotile, ep_x0 = it_x0, ep_y0 = it_y0, ep_z0 = zb + t - 2;
        const int ep_ptile = ep_z0 * (a.tiles_x * a.tiles_y) + ptile_yx;
        float* const scratch = smem + (Cfg::OFF_W + (wb ^ 1) * Cfg::WCH) * 4 + wave * Cfg::EPI_WAVE;
        if (epi_mode == 1) EMO_SPLIT_EPI_FAST(1, acc_lo[2], acc_hi[2], EMO_SPLIT_NO_STAMPS)
        else if (epi_mode == 0) EMO_SPLIT_EPI_FAST(0, acc_lo[2], acc_hi[2], EMO_SPLIT_NO_STAMPS)
        else {
          conv_epilogue_rows<TR, TW, 1, TP, WGP, BM, 2, Cfg::EPI_ROWF>(a, acc_lo[2], acc_hi[2], scratch, smem + Cfg::OFF_BIAS_F,
                                                                       smem + Cfg::OFF_STAT_F, ep_n, ep_cotile, ep_ptile, 0, ep_x0,
                                                                       ep_y0, ep_z0, wp, half, l32, lane, tid);
#if defined(__HIP_DEVICE_COMPILE__)
          // (the general epilogue has paths on which the compiler's wait-count model keeps a residual load pending for ever -- a
          // K-split launch, which never comes here, does not read what it loaded -- and with that state arriving over the loop's
          // back edge it drains vmcnt in front of the first fragment read of every stage, the stage's own prefetch included
          // (seen in the ISA).  A wait it can see clears the model; only launches of the general form pay for it)
          __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0)
#endif
        }
        __syncthreads();                  // scratch and the statistics exchange are free again
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        acc_lo[2][0][j] = acc_lo[1][0][j]; acc_hi[2][0][j] = acc_hi[1][0][j];
        acc_lo[1][0][j] = acc_lo[0][0][j]; acc_hi[1][0][j] = acc_hi[0][0][j];
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc_lo[0][0][j][r] = 0.0f; acc_hi[0][0][j][r] = 0.0f; }
      }
    }
#undef EMO_Z_LANDED
#undef EMO_Z_STORE_PATCH
#undef EMO_Z_CONVERT_PX
#undef EMO_Z_ISSUE
    // (the closing barrier of the last epilogue stands between this item's LDS reads and the next item's prologue)
  }
  if (a.sat_flag != nullptr && sat_m > 65504.0f) *a.sat_flag = 1;   // (every writer stores the same value)
}

// The run length of a launch: 0 = the one-slice kernel of conv_igemm_bf16x3.h.  The items are (sample, y-x tile, channel tile,
// run); an item of run R stages R + 2 slices, so with `waves` items per persistent block the launch costs about
// waves * (R + 2) slice stagings -- and as many MFMA blocks: the outputs on either side of a run are computed and dropped --:
// the R that minimises it (the longest on a tie).  Below R = 6 the seams cost what the shared staging saves ((R + 2) / R stages
// of about 6.5 k cycles per output slice against three of 3.2 k in the one-slice kernel, whose pipeline hides its staging
// better), and a launch that no such run spreads over the chip stays there too.
static inline int conv_f16x2_zs_run_length(int N, int Cout, int D, int H, int W, int ncu) {
  constexpr int RMIN = 6;
  if (D < RMIN || H % ConvCfgZ::TR || W % ConvCfgZ::TW || ncu < 1) return 0;
  const long base = (long)N * (H / ConvCfgZ::TR) * (W / ConvCfgZ::TW) * ((Cout + ConvCfgZ::BM - 1) / ConvCfgZ::BM);
  if (base * ((D + RMIN - 1) / RMIN) < ncu) return 0;     // even the shortest runs leave CUs idle
  int best = 0;
  long best_cost = 0;
  for (int r = RMIN; r <= D; ++r) {
    const long items = base * ((D + r - 1) / r);
    const long cost = ((items + ncu - 1) / ncu) * (r + 2);
    if (best == 0 || cost <= best_cost) { best = r; best_cost = cost; }
  }
  return best;
}
