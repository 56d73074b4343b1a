// The stage machinery that the hand-scheduled split-operand kernels share, stated once: conv_igemm_bf16x3.h (one channel tile,
// bf16x3 / f16x2), conv_igemm_f16x2_ct2.h and conv_igemm_f16x2_w8.h (two tiles; four resp. eight waves, the latter also the
// plain-fp16 mode), conv_igemm_f16x2_p1.h (pointwise), conv_inst_f16x2_up2.hip (phase up-convolution), conv_igemm_f16x2_zs.h
// (depth-shared 3x3x3); conv_igemm_f16.h takes the patch slot formula and the wait / barrier (round 5's verdict on the first
// three: hand-scheduled copies of one schedule mean every fix lands once per copy).  These are MACROS over the kernels' local names
// (a, Cfg, smem, nptiles, TW, TR, UPS, TWS, TP, PR, NQ, NQ1, NHQ, QPG, SUB, CHS, PPL, BM, WGP, p0, half, l32, lq_off, sat_m, ...):
// textual sharing, so every kernel compiles to exactly the code it had (tools/device_code_digest.py holds a change here to that).
// What differs between kernels is a macro parameter -- a register buffer index or none, the channel-half terms of the eight-wave
// kernel, the first channel tile, the depth terms of a load offset.  What is a kernel's own -- its fragment loads, weight pieces /
// chunks, schedule, chaining and epilogue tiles -- stays in its file.  The macros stay defined for the includers.
// The four macros whose text only the GPU toolchain understands (EMO_SPLIT_WAIT, _BARRIER, _TIMED_BARRIER, _LDS_TABLES_ADDR) are
// defined in conv_split_pair_common.h, included here.
// Macros named ...() below that DECLARE (THREAD_IDS, LDS_VIEWS, USOFF, ITEM_WALK, STAGING_MAP, DECLARE_B_OFF, AFFINE4) are
// statement sequences for the scope they are written in, not single statements; the others are one statement or one block.
#pragma once
#include "conv_split_pair_common.h"

// measurement builds: 1 = every weight piece re-reads the FIRST KiB of the packed weights (resident in the CU's L1: WRONG
// results) -- what the weight stream out of the L2 costs a power-managed chip (both paired kernels;
// tools/session/r6_call16.sh, r6_call19.sh)
#ifndef EMO_CT2_W_CONST
#define EMO_CT2_W_CONST 0
#endif
// ... and 1 = every stage of an item re-reads the patch of input channel 0 (L1 / L2 hits after the first stage: WRONG results)
#ifndef EMO_CT2_X_CONST
#define EMO_CT2_X_CONST 0
#endif


// Host side: the gate of the two pair launchers (conv_f16x2_ct2_launch, conv_f16x2_w8_launch).  They differ in the switch they
// read, in how they count pairs and in the input channels per stage.
// conv_pair_form: the launch is in the pair kernels' form -- a final output (no K split, not a guarded launch) through the
// straight-line epilogue, TR x TW position tiles, the input by 16-byte quads (conv_igemm.h)
template <class Cfg, int TR, int TW>
static bool conv_pair_form(const ConvArgs& a) {
  static_assert(TW % 4 == 0, "rows of whole quads");
  return a.ksplit == 1 && a.run_if == nullptr && conv_straight_epilogue_fits(a, Cfg::BM) && a.Wl % TW == 0 && a.Hl % TR == 0 &&
         conv_input_quads_fit(a, Cfg::SCT);
}
// conv_pair_fill: the work items of `pairs` channel-tile pairs, `kc` input channels per stage, into the arguments and the
// persistent grid -- false when there are none, more than 32-bit counts hold, or fewer than two per CU: below that the
// single-tile kernels' twice as many, half as long items balance better (EMO_CONV_CT2_MIN_ITEMS: another threshold, for tests
// and A/B runs, which toggle it inside one process: read at every launch, a launch is microseconds)
template <int TR, int TW>
static bool conv_pair_fill(ConvArgs& a, int pairs, int kc, int* grid) {
  const long nt = (long)(a.Wl / TW) * (a.Hl / TR) * a.Dl;
  const int ncu = emo_cu_count();
  const char* const e_min = getenv("EMO_CONV_CT2_MIN_ITEMS");
  const long min_items = e_min ? atol(e_min) : 2l * ncu;
  if (pairs < 1 || nt > 0x7fffffffL || a.N > 65535 || nt * pairs * a.N > 0x7fffffffL || nt * pairs * a.N < min_items) return false;
  a.tiles_x = a.Wl / TW;
  a.tiles_y = a.Hl / TR;
  a.tiles_z = a.Dl;
  a.n_cchunks = (a.Cin + kc - 1) / kc;
  a.stages_per_split = a.n_cchunks * a.KD;
  a.partial = nullptr;
  a.cot0 = 0;
  a.n_cotiles = pairs;                         // (pairs: EMO_SPLIT_DECODE)
  a.n_work = (int)(nt * pairs * a.N);
  *grid = a.n_work > ncu ? ncu : a.n_work;
  return true;
}

// ---- per-thread preamble ----
#define EMO_SPLIT_THREAD_IDS()                                                                        \
  const int tid = threadIdx.x;                                                                        \
  const int lane = tid & 63;                                                                          \
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                          \
  const int half = lane >> 5, l32 = lane & 31;
// the block's LDS as bytes (EMO_SPLIT_LDS_TABLES_ADDR, conv_split_pair_common.h, declares the rest: two macros, used where the
// declarations stood, behind the fragment registers -- declared together, the eight-wave kernel's code changes)
#define EMO_SPLIT_LDS_VIEWS()                                                                         \
  const char* const lds_c = reinterpret_cast<const char*>(smem);                                      \
  char* const lds_w = reinterpret_cast<char*>(smem);
// scalar byte offsets of the n_ channel planes first_ .. of a thread's raw patch loads, plane_ elements apart (live_: 0u in the
// EMO_CT2_X_CONST measurement builds)
#define EMO_SPLIT_USOFF(n_, first_, plane_, live_)                                                    \
  unsigned usoff[n_];                                                                                 \
  _Pragma("unroll") for (int u = 0; u < (n_); ++u)                                                    \
    usoff[u] = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)((first_) + u) * (unsigned)(plane_) * 4u * (live_)));

// ---- work items of a persistent block: the launch's items in eight contiguous ranges, one per XCD; block b walks the range of
//      XCD b & 7 from b >> 3 with a stride (conv_igemm_bf16x3.h) ----
#define EMO_SPLIT_ITEM_WALK()                                                                         \
  const int q8 = a.n_work >> 3, r8 = a.n_work & 7;                                                    \
  const int xcd = blockIdx.x & 7;                                                                     \
  const int n_mine = q8 + (xcd < r8 ? 1 : 0);                                                         \
  const int l_base = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;                     \
  const int l_stride = (gridDim.x + 7) >> 3;

// work item l -> (sample, position tile, channel tile): XCD-contiguous order, channel tile fastest.  Every result through
// readfirstlane (conv_igemm_bf16x3.h).  cot_expr_: the item's first channel tile from the index cot_ -- the pair kernels count
// PAIRS in n_cotiles --; ksplit_: statements between the channel tile and the sample (the K split of conv_igemm_bf16x3.h) or none
#define EMO_SPLIT_DECODE(P_, L_, cot_expr_, ksplit_)                                                  \
  {                                                                                                   \
    const int l_ = (L_);                                                                              \
    const int cot_ = l_ % a.n_cotiles;                                                                \
    int rest_ = l_ / a.n_cotiles;                                                                     \
    ksplit_                                                                                           \
    const int n_ = rest_ / nptiles;                                                                   \
    int bx_ = rest_ - n_ * nptiles;                                                                   \
    P_##ptile = __builtin_amdgcn_readfirstlane(bx_);                                                  \
    const int tx_ = bx_ % a.tiles_x; bx_ /= a.tiles_x;                                                \
    const int ty_ = bx_ % a.tiles_y; bx_ /= a.tiles_y;                                                \
    P_##cotile = __builtin_amdgcn_readfirstlane(cot_expr_);                                           \
    P_##n = __builtin_amdgcn_readfirstlane(n_);                                                       \
    P_##x0 = __builtin_amdgcn_readfirstlane(tx_ * TW);                                                \
    P_##y0 = __builtin_amdgcn_readfirstlane(ty_ * TR);                                                \
    P_##z0 = __builtin_amdgcn_readfirstlane(bx_);                                                     \
  }

// ---- staging map: thread t belongs to channel group group_ (t / QPG, or what the kernel makes of it); within the group, lane
//      u < PR * NQ owns interior quad u (4 consecutive pixels of one patch row), lane PR * NQ + 2 * row + side owns one halo
//      pixel.  A halo lane issues the SAME 16-byte loads as everybody else -- the aligned quad that contains its pixel (left:
//      x0 - 4 .. x0 - 1, element 3; right: x0 + TWS .. + 3, element 0) -- and runs the same conversion; the three pixels it does
//      not own go to dump slots at the tail of their sub-row (why: conv_igemm_bf16x3.h).  q_slb: byte offsets of the lane's four
//      staging slots inside a patch buffer, + sub_ bytes into the slot ----
#define EMO_SPLIT_STAGING_MAP(group_, sub_)                                                           \
  const int q_u = tid % QPG;                                                                          \
  const int q_g = __builtin_amdgcn_readfirstlane(group_);                                             \
  const bool is_quad = q_u < PR * NQ;                                                                 \
  const int hq = q_u - PR * NQ;                                                                       \
  const bool is_halo = !is_quad && hq < NHQ;                                                          \
  const int h_side = hq & 1;                                                                          \
  const int q_r = is_quad ? q_u / NQ : (is_halo ? hq >> 1 : 0);                                       \
  const int q_c = is_quad ? q_u - q_r * NQ : 0;                                                       \
  int q_slb[4];                                                                                       \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                     \
    const int dump = q_g * CHS + i * SUB + PR * NQ1 + (q_u & 3);                                      \
    const int own = is_quad ? q_g * CHS + i * SUB + q_r * NQ1 + q_c : q_g * CHS + h_side * SUB + q_r * NQ1 + NQ; \
    q_slb[i] = ((is_quad || (is_halo && i == (h_side ? 0 : 3))) ? own : dump) * 16 + (sub_);          \
  }

// the lane's 16-byte patch load for the tile of item P_ (its quad, or the aligned quad that contains its halo pixel) and whether
// it lies inside the image
#define EMO_SPLIT_CURSOR_OF(P_, ok_, off_)                                                            \
  {                                                                                                   \
    const int x0s_ = UPS ? P_##x0 >> 1 : P_##x0, y0s_ = UPS ? P_##y0 >> 1 : P_##y0;   /* tile origin in source pixels */ \
    const int q_y_ = y0s_ - 1 + q_r;                                                                  \
    const int q_x_ = is_quad ? x0s_ + 4 * q_c : (h_side ? x0s_ + TWS : x0s_ - 4);   /* first pixel of the lane's 16-byte load */ \
    ok_ = (is_quad || is_halo) && (unsigned)q_y_ < (unsigned)a.H && q_x_ >= 0 && q_x_ < a.W;          \
    off_ = ok_ ? (unsigned)(q_y_ * a.W + q_x_) * 4u : 0u;                                             \
  }

// ---- LDS slot of patch pixel (row pr_, column pc_ relative to the tile: -1 / TWS = the halo columns) inside an 8-channel group
#define EMO_SPLIT_PATCH_SLOT(pr_, pc_)                                                                \
  ((pc_) < 0 ? (pr_) * NQ1 + NQ : ((pc_) >= TWS ? SUB + (pr_) * NQ1 + NQ : ((pc_) & 3) * SUB + (pr_) * NQ1 + ((pc_) >> 2)))
// LDS byte offsets of the lane's patch fragments: b_off[position tile][kernel-row class][tap column] (+ half * CHS: the lane's
// 8-channel group).  Kernel row r adds r patch rows = r * NQ1 slots (an immediate); with the fused upsample the source row of
// kernel row r is (row + r + 1) >> 1: kernel row 2 is kernel row 0 plus one patch row, kernel row 1 depends on the parity of
// the pixel row and keeps its own registers
#define EMO_SPLIT_DECLARE_B_OFF()                                                                     \
  constexpr int NBR = UPS ? 2 : 1;                                                                    \
  int b_off[TP][NBR][3];                                                                              \
  _Pragma("unroll") for (int j = 0; j < TP; ++j) {                                                    \
    const int p = p0 + j * 32 + l32;                                                                  \
    const int col = p % TW, row = p / TW;                                                             \
    _Pragma("unroll") for (int r = 0; r < NBR; ++r)                                                   \
    _Pragma("unroll") for (int s = 0; s < 3; ++s) {                                                   \
      const int pr = UPS ? ((row + r - 1 + 2) >> 1) - 1 + 1 : row + r;                                \
      const int pc = UPS ? ((col + s - 1 + 2) >> 1) - 1 : col + s - 1;                                \
      const int slot = EMO_SPLIT_PATCH_SLOT(pr, pc);                                                  \
      b_off[j][r][s] = (half * CHS + slot) * 16;                                                      \
    }                                                                                                 \
  }
#define EMO_SPLIT_B_OFF(j_, r_, s_) (UPS ? ((r_) == 2 ? b_off[j_][0][s_] + NQ1 * 16 : b_off[j_][(r_) < NBR ? (r_) : 0][s_]) \
                                         : b_off[j_][0][s_] + (r_) * NQ1 * 16)

// ---- issue of a stage's raw patch loads.  BEGIN: the 8-channel group at input channel c0_ -- clamp bounds into q_lo ix_ /
//      q_hi ix_ ([0, 0] where keep_, which may name cv_ = "the group lies inside Cin", is false: padding), table index into
//      q_tix ix_, load offset into vo_ = the cursor + voff_ bytes (an expression of cs_, the clamped channel).  ix_: the
//      register buffer's index, or nothing ----
#define EMO_SPLIT_ISSUE_BEGIN(ix_, vo_, c0_, keep_, voff_)                                            \
  {                                                                                                   \
    const int c0__ = (c0_);                                                                           \
    const bool cv_ = c0__ < a.Cin;                                                                    \
    const int cs_ = cv_ ? c0__ : 0;                                                                   \
    const bool keep__ = (keep_);                                                                      \
    q_lo ix_ = keep__ ? clamp_lo : 0.0f;                                                              \
    q_hi ix_ = keep__ ? CLAMP_HI : 0.0f;                                                              \
    vo_ = lq_off + (voff_);                                                                           \
    q_tix ix_ = (has_affine ? cs_ : (cs_ & (Cfg::SCT - 1))) >> 2;                                     \
  }
// the paired 16-byte loads of channel planes u0_ .. u1_ - 1 into the raw registers qv_
#define EMO_SPLIT_ISSUE_LOADS(qv_, vo_, u0_, u1_)                                                     \
  { _Pragma("unroll") for (int u = (u0_); u < (u1_); u += 2) emo_bload4x2_pinned(xrs, vo_, usoff[u], usoff[u + 1], qv_[u], qv_[u + 1]); }
// scale / shift of the four channels at table index tix_
#define EMO_SPLIT_TABLE(tix_, sc_, sh_)                                                               \
  {                                                                                                   \
    const floatx4* t4_ = reinterpret_cast<const floatx4*>(sct) + (tix_);                              \
    sc_ = t4_[0]; sh_ = t4_[Cfg::SCT / 4];                                                            \
  }
// ... of the eight channels at tix_, tix_ + 1
#define EMO_SPLIT_TABLE2(tix_, sc_, sh_)                                                              \
  {                                                                                                   \
    const floatx4* t4_ = reinterpret_cast<const floatx4*>(sct) + (tix_);                              \
    sc_[0] = t4_[0]; sc_[1] = t4_[1]; sh_[0] = t4_[Cfg::SCT / 4]; sh_[1] = t4_[Cfg::SCT / 4 + 1];     \
  }
#define EMO_SPLIT_TOUCH(qv_, n_) { _Pragma("unroll") for (int u = 0; u < (n_); ++u) emo_touch4(qv_[u]); }

// ---- conversion core, four channels of one pixel.  AFFINE4: t_[k] = the fp32 transform (GroupNorm affine of the producer) of
//      element i_ of the raw registers qv_[q0_ + k].  RANGE4: range check of the fp16 split, max |pre-clamp value| (v_max3 with
//      |.| modifiers).  F16X2_4: ReLU, saturation and zero padding in one v_med3 (bounds [0, 0] where the pixel is padding), then
//      the exact split v = h + m (round-to-nearest-even, the residual is exact) into elements k0_ .. k0_ + 3 of the plane
//      registers cvh_ / cvm_.  STORE_PLANES: the pixel's slot (T_: 8 or 4 channels wide) of both operand planes ----
#define EMO_SPLIT_AFFINE4(t_, qv_, q0_, i_, sc_, sh_)                                                 \
  float t_[4];                                                                                        \
  _Pragma("unroll") for (int k = 0; k < 4; ++k)                                                       \
    t_[k] = __fmaf_rn(qv_[(q0_) + k][i_], sc_[k], sh_[k]);
#define EMO_SPLIT_RANGE4(t_)                                                                          \
  {                                                                                                   \
    sat_m = __builtin_fmaxf(__builtin_fmaxf(sat_m, __builtin_fabsf(t_[0])), __builtin_fabsf(t_[1])); \
    sat_m = __builtin_fmaxf(__builtin_fmaxf(sat_m, __builtin_fabsf(t_[2])), __builtin_fabsf(t_[3])); \
  }
#define EMO_SPLIT_F16X2_4(t_, lo_, hi_, cvh_, cvm_, k0_)                                              \
  _Pragma("unroll") for (int k = 0; k < 4; k += 2)                                                    \
    emo_split_f16x2_pair(__builtin_amdgcn_fmed3f(t_[k], lo_, hi_), __builtin_amdgcn_fmed3f(t_[k + 1], lo_, hi_), cvh_, cvm_, (k0_) + k);
#define EMO_SPLIT_STORE_PLANES(T_, d_, cvh_, cvm_)                                                    \
  {                                                                                                   \
    *reinterpret_cast<T_*>(d_) = cvh_;                                                                \
    *reinterpret_cast<T_*>((d_) + PPL * 16) = cvm_;                                                   \
  }

// ---- straight-line epilogue of one channel tile (conv_epilogue_fast_issue / _finish, conv_igemm_bf16x3.h) of the item ep_n,
//      ep_ptile, ep_x0, ep_y0, ep_z0 through `scratch`: the residual loads of tile cot_ into rv_, and the tile's accumulators out.
//      pair_: the pair kernels' form (laundered offsets; the tile statistics left to EMO_SPLIT_COMBINE_STATS).  ts_:
//      EMO_SPLIT_STAMPS in a kernel that keeps the stamp array of the measurement builds (EMO_S_TIMING), EMO_SPLIT_NO_STAMPS in
//      one that has none -- the NAME of a macro, expanded where the call is written ----
#define EMO_SPLIT_STAMPS() EMO_S_TSTAMP_ARG
#define EMO_SPLIT_NO_STAMPS()
#define EMO_SPLIT_EPI_ISSUE(RES_, pair_, rv_, cot_)                                                   \
  conv_epilogue_fast_issue<TW, TP, BM, RES_, 0, pair_>(a, rv_, ep_n, cot_, ep_x0, ep_y0, ep_z0, wp, lane);
#define EMO_SPLIT_EPI_FINISH(RES_, pair_, lo_, hi_, rv_, bias_f_, stat_f_, cot_, ts_)                 \
  conv_epilogue_fast_finish<TW, TM, TP, WGP, BM, SPLIT, Cfg::EPI_ROWF, RES_, pair_, pair_>(                                         \
      a, lo_, hi_, rv_, scratch, smem + (bias_f_), smem + (stat_f_), ep_n, cot_, ep_ptile, ep_x0, ep_y0, ep_z0, wp, half, l32,     \
      lane, tid ts_());
// ... of a single-tile item
#define EMO_SPLIT_EPI_FAST(RES_, lo_, hi_, ts_)                                                       \
  {                                                                                                   \
    floatx4 rv_[8];                                                                                   \
    EMO_SPLIT_EPI_ISSUE(RES_, false, rv_, ep_cotile)                                                  \
    EMO_SPLIT_EPI_FINISH(RES_, false, lo_, hi_, rv_, Cfg::OFF_BIAS_F, Cfg::OFF_STAT_F, ep_cotile, ts_) \
  }

// tile statistics, second half (conv_epilogue_rows_stats, for both tiles of the pair at once, behind the barrier that ends the
// item): thread c of the first 2 BM combines the WGP position groups' (mean, M2) of channel c with the equal-count update.  The
// exchange areas are next written by the NEXT item's epilogue, a K loop away
// (real_: false for the unwritten second half of a half-empty last pair -- conv_igemm_f16x2_w8.h with plain fp16 operands only)
#define EMO_SPLIT_COMBINE_STATS(st1_f_, st2_f_, real_)                                                \
  if (a.gn_stats != nullptr && tid < 2 * BM && (real_)) {                                             \
    const int c_ = tid & (BM - 1);                                                                    \
    const float* const st_ = smem + (tid < BM ? (st1_f_) : (st2_f_));                                 \
    float mean = 0.0f, m2 = 0.0f;                                                                     \
    _Pragma("unroll") for (int w = 0; w < WGP; ++w) mean += st_[(w * BM + c_) * 2 + 0];               \
    mean *= 1.0f / (float)WGP;                                                                        \
    _Pragma("unroll") for (int w = 0; w < WGP; ++w) {                                                 \
      const float d = st_[(w * BM + c_) * 2 + 0] - mean;                                              \
      m2 += st_[(w * BM + c_) * 2 + 1] + (float)(TP * 32) * d * d;                                    \
    }                                                                                                 \
    float2* dst = reinterpret_cast<float2*>(a.gn_stats) + ((long)it_n * nptiles + it_ptile) * a.Cout + it_cotile * BM + tid; \
    *dst = make_float2(mean, m2);                                                                     \
  }
