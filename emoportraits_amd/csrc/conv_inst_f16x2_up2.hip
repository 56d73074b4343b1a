// The decoder's up-convolutions conv3x3(up2_nearest(relu(gn_affine(x)))) in the fp16 split (SPLIT = 2, as conv_igemm_bf16x3.h:
// two fp16 terms of the scaled operands, three products, fp32 accumulation, device-checked operand range) as FOUR 2x2 PHASE
// convolutions on the low-resolution input -- "UP2".
//
// Why.  Under nearest x2 upsampling the output pixel (2i + p, 2j + q) reads low-res rows i - 1 + p .. i + p and columns
// j - 1 + q .. j + q only: kernel row a of phase p is the sum of the 3x3 kernel rows R_p[a] (R_0 = {0}, {1, 2}; R_1 = {0, 1}, {2}),
// columns likewise.  So the layer is four 2x2 convolutions of x with pre-summed weights (emoportraits_amd.pack.pack_weight_f16x2_up2):
// 4 Cin MACs per output instead of 9 Cin -- 2.25x fewer MFMAs, and a shorter accumulation.  Zero padding stays exact (high-res
// row -1 reads low-res row -1, row 2H reads low-res row H).
//
// Item: one 64-channel output tile x a low-res region of 4 rows x 64 columns (a high-res 8 x 128 block, four 4 x 64 statistics
// tiles).  Stage: 16 input channels, one converted (4 + 2) x (64 + 2) low-res patch in LDS (the staging of conv_igemm_bf16x3.h
// and conv_igemm_f16x2_ct2.h on a low-res tile, no upsampling gather): 108 of the 128 threads of a staging group own a quad or a
// halo pixel.  Half-stage h = row phase p: its kernel W[h] holds the 8 taps (2 column phases x 2 x 2) of that phase, 32 KiB.
// Wave w = (q = w & 1, row pair g = w >> 1): it runs column phase q on the 128 positions of low-res rows 2 g, 2 g + 1, 4 tap steps
// per half-stage, 24 MFMAs per step, and keeps both row phases' accumulators in ONE set (2 x 128 registers): per tap step the two
// cross products, then the leading product, into the same accumulator.  A phase output sums 4 Cin products, not 9 Cin, so the
// single set stays inside the split's error bounds; the 9-tap kernels keep two sets.  A map whose height is no
// multiple of 4 ends in items whose rows 2, 3 lie outside: they are staged as zeros and neither stored nor counted.
// One barrier per half-stage, everything in flight drained there (vmcnt(0)):
//   (cg, h)  steps 0 .. 2  pieces 2 .. 7 of the next half-stage's kernel into W[h ^ 1]
//            step 3        barrier; pieces 0, 1 of the half-stage after it into W[h]; fragments of the next half-stage's step 0
//   (cg, 0)  steps 0 .. 3  the patch of stage cg + 1 converted from the raw registers into P[pp ^ 1], one pixel per step
//   (cg, 0)  step 3        behind the last pixel's conversion: the raw loads of stage cg + 2 -- four tap steps (96 MFMAs) ahead of
//                          the barrier of (cg, 1) that drains them (EMO_UP2_LOADS_EARLY = 0: steps 0 .. 2 of (cg, 1), one to
//                          three steps of flight)
// Epilogue: through LDS in eight passes of 32 channels x one 4 x 64 statistics tile (one row pair's two waves, 16-byte LDS writes
// into an image [channel][row][column phase][32 low-res columns]); the read-out interleaves the column phases into whole rows,
// + bias, 16-byte stores, the tile's (mean, M2) (the TileStats layout of block config D).  No residual, no activation.
// CHAINED items (EMO_UP2_CHAIN; the stage machinery is conv_split_common.h's, the chaining that of the pair kernels): when
// the block's next item belongs to the same sample (same
// scale / shift tables) and the item has >= 2 stages, the look-ahead of the last two stages -- dead re-stages otherwise -- fetches
// the next item's first stage instead: kernel (stage 0, p = 0) into W[0], the raw loads of its stages 0 and 1 with ITS cursor, its
// stage-0 patch converted into P[pp ^ 1].  The epilogue image lies in W[1] and the tail of LDS (dead at an item's end: the last
// half-stage read W[1]), so P, W[0] and the tables survive it, and the next item starts with a short prologue: its bias entries
// (fetched during the epilogue), pieces 0, 1 of (stage 0, p = 1) into W[1], one barrier that waits for no memory operation.
// The kernel lives in this instantiation file (not a header) so that the CPU emulation of tests/emul/convlib.py, which rewrites
// the instantiation files and a fixed list of headers, compiles it.
#include "conv_dispatch.h"
#include "conv_igemm_bf16x3.h"

#ifndef EMO_UP2_CHAIN
#define EMO_UP2_CHAIN 1         /* 0: A/B builds -- every item runs the full prologue */
#endif
#ifndef EMO_UP2_LOADS_EARLY
#define EMO_UP2_LOADS_EARLY 1   /* 0: A/B builds -- the raw loads of stage cg + 2 at steps 0 .. 2 of half-stage (cg, 1) */
#endif

struct ConvCfgUp2 {
  static constexpr int BM = 64, TM = 2, TP = 4, KC = 16, NPL = 2;
  static constexpr int TRL = 4, TWL = 64;                // low-res extent of an item
  static constexpr int PR = TRL + 2, NQ = TWL / 4, NQ1 = NQ + 1;
  static constexpr int SUB = ((PR * NQ1 + 4 + 11) / 16) * 16 + 4;
  static constexpr int CHS = 4 * SUB, NG = 2, QPG = 128, NHQ = 2 * PR;
  // (16-byte slots)
  static constexpr int WPLANE = 2 * BM;                  // one plane of a tap: [half][BM]
  static constexpr int WTAP = NPL * WPLANE;
  static constexpr int WST = 8 * WTAP;                   // a half-stage's kernel: [q][a][b][plane][half][BM] -- 32 KiB
  static constexpr int WST_BYTES = WST * 16;
  static constexpr int PPL = NG * CHS, PBUF = NPL * PPL;
  // LDS: P[0], P[1] | W[0] | scale / shift tables, bias | W[1] | tail.  The epilogue image starts at W[1] and runs into the tail
  static constexpr int SCT = 1024;
  static constexpr int OFF_P = 0, OFF_W = 2 * PBUF, OFF_SCT = OFF_W + WST;
  static constexpr int WSTRIDE = WST + (2 * SCT + BM) / 4;           // W[1] = W[0] + WSTRIDE: behind the tables and the bias
  static constexpr int OFF_BIAS_F = OFF_SCT * 4 + 2 * SCT;          // (float index) [BM]
  static constexpr int EPI_CS = 4 * 64 + 4;                          // floats per channel of the epilogue image: 4 rows of 2 x 32, + 4
  static constexpr int EPI_CH = 32;                                  // channels of one epilogue pass (4 rows x 128 columns do not fit behind W[0])
  static constexpr int OFF_IMG_F = (OFF_W + WSTRIDE) * 4;            // (float index) the image: over W[1] and the tail
  static constexpr int LDS_BYTES = (OFF_IMG_F + EPI_CH * EPI_CS) * 4;
  static_assert(OFF_IMG_F >= OFF_BIAS_F + BM, "the epilogue image spares the patch buffers, W[0], the tables and the bias: a chained successor's");
  static_assert(EPI_CH * EPI_CS * 4 >= WST_BYTES, "W[1] lies inside the image's allocation");
  static_assert(TRL == 4 && TP == 4, "a wave holds two low-res rows: one epilogue pass is one row pair's 4 high-res rows");
  static_assert(WST_BYTES == 32 * 1024, "eight 1 KiB pieces per wave and half-stage");
  static_assert(PR * NQ + NHQ <= QPG, "one interior quad or one halo pixel per thread and stage");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void conv_igemm_f16x2_up2_kernel(const ConvArgs a) {
  using Cfg = ConvCfgUp2;
  using opx8 = halfx8;
  constexpr int NPL = 2, NPROD = 3;
  constexpr int BM = Cfg::BM, TM = Cfg::TM, TP = Cfg::TP, KC = Cfg::KC;
  constexpr int PR = Cfg::PR, NQ = Cfg::NQ, NQ1 = Cfg::NQ1, SUB = Cfg::SUB, CHS = Cfg::CHS, QPG = Cfg::QPG;
  constexpr int NHQ = Cfg::NHQ, PPL = Cfg::PPL, PBUF = Cfg::PBUF;
  // (names of the shared staging macros: a low-res tile without the upsampling gather)
  constexpr bool UPS = false;
  constexpr int TW = Cfg::TWL, TWS = Cfg::TWL;

  extern __shared__ __attribute__((aligned(16))) float smem[];

  EMO_SPLIT_THREAD_IDS()
  const int wq = wave & 1;                               // column phase of the wave
  const int p0 = (wave >> 1) * TP * 32;                  // its 128 positions: low-res rows 2 (wave >> 1), + 1 of the item
  float sat_m = 0.0f;

  const int HW = a.H * a.W;
  const bool has_affine = a.scale != nullptr;
  const float in_scale = a.in_scale;
  constexpr float CLAMP_HI = 65504.0f;
  const float clamp_lo = a.relu_in ? 0.0f : -CLAMP_HI;
  const int nst = a.n_cchunks;
  const int nptiles = a.tiles_x * a.tiles_y;

  EMO_SPLIT_STAGING_MAP(tid / QPG, 0)

  floatx16 acc[2][TM][TP];                               // [row phase]: one set for the three products

  // ---- work items: (sample, low-res tile, channel tile), XCD-contiguous, channel tile fastest; persistent blocks ----
  EMO_SPLIT_ITEM_WALK()
// byte address of the packed kernel of (channel tile c_, stage k_, row phase p_)
#define EMO_U_WPTR(c_, k_, p_) (reinterpret_cast<const char*>(a.wpk) + ((long)((c_) * nst + (k_)) * 2 + (p_)) * Cfg::WST_BYTES)

  const int a_off = (half * BM + l32) * 16;
  EMO_SPLIT_DECLARE_B_OFF()

  EMO_SPLIT_LDS_VIEWS()
  opx8 fa_[2][NPL][TM], fb_[2][NPL][TP];
// fragments of tap (a_, b_) of half-stage buffer hb_ (patch buffer at byte pbyte_): the wave's column phase wq
#define EMO_U_LOAD_FRAGS_PLANE(set_, pl_, hb_, pbyte_, a_, b_)                                        \
  {                                                                                                   \
    _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                    \
      fa_[set_][pl_][i] = *reinterpret_cast<const opx8*>(lds_c + a_off + (Cfg::OFF_W + (hb_) * Cfg::WSTRIDE + \
          ((wq * 4 + (a_) * 2 + (b_)) * NPL + (pl_)) * Cfg::WPLANE + i * 32) * 16);                   \
    _Pragma("unroll") for (int j = 0; j < TP; ++j)                                                    \
      fb_[set_][pl_][j] = *reinterpret_cast<const opx8*>(lds_c + (EMO_SPLIT_B_OFF(j, (hb_) + (a_), wq + (b_)) + (pbyte_)) + ((pl_) * PPL) * 16); \
  }

  EMO_SPLIT_LDS_TABLES_ADDR()

  floatx4 qv[8];
  float q_lo, q_hi;
  int q_tix;
  floatx4 q_sc, q_sh;
  opx8 cv_h, cv_m;
  emo_intx4 xrs = emo_raw_buffer(a.x);
  EMO_SPLIT_USOFF(8, 0, HW, 1u)
  unsigned lq_off = 0;
  bool lq_ok = false;
  unsigned q_vo;
// the raw loads of stage st_ (16 input channels)
#define EMO_U_ISSUE_BEGIN(st_) EMO_SPLIT_ISSUE_BEGIN(, q_vo, (st_) * KC + q_g * 8, lq_ok && cv_, (unsigned)cs_ * (unsigned)HW * 4u)
#define EMO_U_ISSUE_LOADS(u0_, u1_) EMO_SPLIT_ISSUE_LOADS(qv, q_vo, u0_, u1_)
#define EMO_U_TOUCH_QUAD() EMO_SPLIT_TOUCH(qv, 8)
// conversion of pixel i_ of the raw registers (both halves of the lane's 8 channels) into the patch buffer at byte pbyte_
#define EMO_U_CONV_PIXEL(pbyte_, i_)                                                                  \
  {                                                                                                   \
    _Pragma("unroll") for (int hf_ = 0; hf_ < 2; ++hf_) {                                             \
      EMO_SPLIT_TABLE(q_tix + hf_, q_sc, q_sh)                                                        \
      EMO_SPLIT_AFFINE4(t_, qv, 4 * hf_, i_, q_sc, q_sh)                                              \
      EMO_SPLIT_RANGE4(t_)                                                                            \
      EMO_SPLIT_F16X2_4(t_, q_lo, q_hi, cv_h, cv_m, 4 * hf_)                                          \
    }                                                                                                 \
    char* d_ = lds_w + (q_slb[i_] + (pbyte_));                                                        \
    EMO_SPLIT_STORE_PLANES(opx8, d_, cv_h, cv_m)                                                      \
  }
// piece k_ = 0 .. 7 of a half-stage's kernel (wave w copies the 1 KiB pieces w + 4 k) into W[wb_]
#define EMO_U_DMA_PIECE(ptr_, wb_, k_)                                                                \
  {                                                                                                   \
    const int j_ = wave + 4 * (k_);                                                                   \
    emo_dma16_pinned_s((ptr_) + j_ * 1024, lane16, smem_lds + (unsigned)((Cfg::OFF_W + (wb_) * Cfg::WSTRIDE) * 16 + j_ * 1024)); \
  }

  constexpr int PA3[3] = {1, 0, 0}, PB3[3] = {0, 1, 0};
  constexpr int NTE = Cfg::SCT / 256;

// work item l -> (sample, low-res tile, channel tile); every result through readfirstlane (conv_igemm_bf16x3.h)
#define EMO_U_DECODE(P_, L_)                                                                          \
  {                                                                                                   \
    const int l_ = (L_);                                                                              \
    P_##cotile = __builtin_amdgcn_readfirstlane(l_ % a.n_cotiles);                                    \
    const int rest_ = l_ / a.n_cotiles;                                                               \
    P_##n = __builtin_amdgcn_readfirstlane(rest_ / nptiles);                                          \
    const int lt_ = rest_ - P_##n * nptiles;                                                          \
    P_##x0 = __builtin_amdgcn_readfirstlane((lt_ % a.tiles_x) * Cfg::TWL);     /* low-res origin */   \
    P_##y0 = __builtin_amdgcn_readfirstlane((lt_ / a.tiles_x) * Cfg::TRL);                            \
  }
// the raw loads of stage cg + 2, first part; past the item's end: the next item's stages 0 / 1 with its cursor (chained), a dead
// re-load of the last stage otherwise.  Indices are SELECTED: no branch
#define EMO_U_NEXT_STAGE_BEGIN()                                                                      \
  {                                                                                                   \
    const bool sw_ = chain_out && cg + 2 == nst;                                                      \
    const int tgt_ = (chain_out && cg + 2 >= nst) ? cg + 2 - nst : (cg + 2 < nst ? cg + 2 : nst - 1); \
    lq_ok = sw_ ? nxq_ok : lq_ok;                                                                     \
    lq_off = sw_ ? nxq_off : lq_off;                                                                  \
    EMO_U_ISSUE_BEGIN(tgt_)                                                                           \
  }

  constexpr bool CHAIN = EMO_UP2_CHAIN != 0, LOADS_EARLY = EMO_UP2_LOADS_EARLY != 0;
  float te_b = 0.0f;
  bool chained_in = false;                 // this item's first stage (and the loads of its second) were staged by the previous item
  int pp = 0;                              // patch buffer of the item's current stage
  for (int idx8 = blockIdx.x >> 3; idx8 < n_mine; idx8 += l_stride) {
#if EMO_S_TIMING
    unsigned long long tstamp[12];     // measurement builds (tools/conv_phase_timing.py): s_memtime at the phase boundaries
    for (int k = 0; k < 12; ++k) tstamp[k] = 0;
    unsigned long long tw_wait = 0, tw_bar = 0, tw_n = 0;
#endif
    EMO_S_STAMP(0)
    // ---- item, and the block's next one ----
    int cotile, it_n, x0, y0;
    {
      int it_cotile, it_x0, it_y0;
      EMO_U_DECODE(it_, l_base + idx8)
      cotile = it_cotile; x0 = it_x0; y0 = it_y0;
    }
    int nx_cotile = 0, nx_n = 0, nx_x0 = 0, nx_y0 = 0;
    bool chain_out = false, nxq_ok = false;
    unsigned nxq_off = 0;
    if (CHAIN && idx8 + l_stride < n_mine) {
      EMO_U_DECODE(nx_, l_base + idx8 + l_stride)
      chain_out = nx_n == it_n && nst >= 2;
      EMO_SPLIT_CURSOR_OF(nx_, nxq_ok, nxq_off)
    }
    xrs = emo_raw_buffer(a.x + (long)it_n * a.Cin * HW);
    asm volatile("" : "=v"(cv_h));
    asm volatile("" : "=v"(cv_m));
    if (CHAIN && chained_in) {
      // ---- chained prologue: P[pp] holds the converted patch of stage 0, W[0] the kernel of (stage 0, p = 0), qv the landed loads
      //      of stage 1, the tables are the sample's.  What is left: the bias entries and pieces 0, 1 of (0, 1), which had no live
      //      buffer to land in (W[1] was the epilogue image).  The barrier waits for NO memory operation: the pieces are drained
      //      by the barrier of (0, 0), the previous item's stores drain behind the first tap steps ----
      if (tid < BM) smem[Cfg::OFF_BIAS_F + tid] = te_b;
      const char* const w1_ = EMO_U_WPTR(cotile, 0, 1);
      EMO_U_DMA_PIECE(w1_, 1, 0)
      EMO_U_DMA_PIECE(w1_, 1, 1)
      EMO_SPLIT_BARRIER(63);                  // (the epilogue's stores and these two pieces stay outstanding)
    } else {
      // ---- full prologue: tables, bias, the whole kernel of (stage 0, p = 0), pieces 0, 1 of (0, 1), patch 0 converted, loads of stage 1 ----
      {
        int it_x0 = x0, it_y0 = y0;
        EMO_SPLIT_CURSOR_OF(it_, lq_ok, lq_off)
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) asm volatile("" : "=v"(qv[u]));
      {
        const char* const w0_ = EMO_U_WPTR(cotile, 0, 0);
#pragma unroll
        for (int k = 0; k < 8; ++k) EMO_U_DMA_PIECE(w0_, 0, k)
        const char* const w1_ = EMO_U_WPTR(cotile, 0, 1);
        EMO_U_DMA_PIECE(w1_, 1, 0)
        EMO_U_DMA_PIECE(w1_, 1, 1)
      }
      EMO_U_ISSUE_BEGIN(0)
      EMO_U_ISSUE_LOADS(0, 8)
#pragma unroll
      for (int k = 0; k < NTE; ++k) {       // (without an affine the index wraps at SCT: identity entries)
        const int c = tid + 256 * k;
        if (c < min(a.Cin, Cfg::SCT)) {
          const bool real = has_affine;
          sct[c] = (real ? a.scale[(long)it_n * a.Cin + c] : 1.0f) * in_scale;
          sct[Cfg::SCT + c] = (real ? a.shift[(long)it_n * a.Cin + c] : 0.0f) * in_scale;
        }
      }
      if (tid < BM) smem[Cfg::OFF_BIAS_F + tid] = a.bias != nullptr ? a.bias[cotile * BM + tid] : 0.0f;
      EMO_SPLIT_WAIT(0);
      EMO_U_TOUCH_QUAD()
      __syncthreads();   // scale / shift tables visible
#pragma unroll
      for (int i = 0; i < 4; ++i) EMO_U_CONV_PIXEL(Cfg::OFF_P * 16, i)
      EMO_U_ISSUE_BEGIN(nst > 1 ? 1 : 0)
      EMO_U_ISSUE_LOADS(0, 8)
      EMO_SPLIT_BARRIER(0);                    // (P[0] visible, W[0] and the loads of stage 1 landed)
      EMO_U_TOUCH_QUAD()
      pp = 0;
    }

    // ---- K loop ----
    EMO_S_STAMP(1)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TP; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[c][i][j][r] = 0.0f;
    {
      const int pb0_ = (Cfg::OFF_P + pp * PBUF) * 16;
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) EMO_U_LOAD_FRAGS_PLANE(0, pl, 0, pb0_, 0, 0)
    }
    for (int cg = 0; cg < nst; ++cg) {
      const int pcur_b = (Cfg::OFF_P + pp * PBUF) * 16, pnxt_b = (Cfg::OFF_P + (pp ^ 1) * PBUF) * 16;
      const bool last_ = cg + 1 >= nst;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // t = (cg, h); t + 1 = (cg, 1) resp. (cg + 1, 0); t + 2 = (cg + 1, h).  Past the item's end: the next item's (stage 0,
        // p = 0) into W[0] when chained -- its pieces 0, 1 as t + 2 of (last, 0), pieces 2 .. 7 as t + 1 of (last, 1) -- and the last
        // stage again otherwise (dead: whether to fetch must not depend on chain_out, a branch on it inside the loop costs 50
        // registers).  Pieces 0, 1 of the next item's (0, 1) would land in W[1], the epilogue image: the chained prologue fetches
        // them.  Pointers from SELECTED indices
        const bool past_ = last_ && chain_out;
        const bool have1_ = CHAIN || h == 0 || !last_, have2_ = !last_ || (CHAIN && h == 0);   // (EMO_UP2_CHAIN = 0: nothing is fetched past the end)
        const int ce_ = past_ ? nx_cotile : cotile, ke_ = last_ ? (chain_out ? 0 : nst - 1) : cg + 1;
        const char* const dma1 = h == 0 ? EMO_U_WPTR(cotile, cg, 1) : EMO_U_WPTR(ce_, ke_, 0);
        const char* const dma2 = EMO_U_WPTR(ce_, ke_, h);
        if (EMO_CONV_SETPRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int gs = 0; gs < 4; ++gs) {
          const int fcur = (h * 4 + gs) & 1, fnxt = fcur ^ 1;
          if (gs == 3) { EMO_SPLIT_TIMED_BARRIER(0); }
          if (gs == 3 && h == 1) EMO_U_TOUCH_QUAD()
          if (!LOADS_EARLY && gs == 0 && h == 1) EMO_U_NEXT_STAGE_BEGIN()
          __builtin_amdgcn_sched_barrier(0);
          {
            const int an = gs < 3 ? (gs + 1) >> 1 : 0, bn = gs < 3 ? (gs + 1) & 1 : 0;
            const int hbn = gs < 3 ? h : h ^ 1;
            const int pbn = (gs == 3 && h == 1) ? pnxt_b : pcur_b;
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl) {
              EMO_U_LOAD_FRAGS_PLANE(fnxt, pl, hbn, pbn, an, bn)
              if (gs < 3 && have1_) EMO_U_DMA_PIECE(dma1, h ^ 1, 2 + 2 * gs + pl)
              if (gs == 3 && have2_) EMO_U_DMA_PIECE(dma2, h, pl)
              if (!LOADS_EARLY && h == 1 && gs == 0) EMO_U_ISSUE_LOADS(2 * pl, 2 * pl + 2)
              if (!LOADS_EARLY && h == 1 && gs > 0 && gs < 3 && pl == 0) EMO_U_ISSUE_LOADS(2 + 2 * gs, 4 + 2 * gs)
            }
          }
          if (h == 0) EMO_U_CONV_PIXEL(pnxt_b, gs)
          if (LOADS_EARLY && h == 0 && gs == 3) {
            // the raw registers are free behind the last pixel's conversion; this step's two weight pieces went out above, so the
            // loads are the youngest operations in flight and nothing waits for them before the barrier of (cg, 1)
            EMO_U_NEXT_STAGE_BEGIN()
            EMO_U_ISSUE_LOADS(0, 8)
          }
#pragma unroll
          for (int p = 0; p < NPROD; ++p) {                // (the cross products first, the leading product last: 8 MFMAs
            const int pa = PA3[p], pb = PB3[p];              //  lie between two on one accumulator)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
              for (int j = 0; j < TP; ++j)
                acc[h][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb_[fcur][pb][j], fa_[fcur][pa][i], acc[h][i][j], 0, 0, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if (EMO_CONV_SETPRIO) __builtin_amdgcn_s_setprio(0);
      }
      pp ^= 1;
    }

    // ---- epilogue: eight passes (channel block i, row pair g, column half k = one 4 x 64 statistics tile) through an LDS image
    //      [32 channels][4 high-res rows][column phase][32 low-res columns] (+ 4) in W[1] + tail; a row pair beyond the map (ragged
    //      height) is skipped ----
    EMO_S_STAMP(2)
    EMO_SPLIT_WAIT(0);
    EMO_S_STAMP(5)
    __syncthreads();
    EMO_S_STAMP(6)
    EMO_S_STAMP(7)
    float* const img = smem + Cfg::OFF_IMG_F;
    if (CHAIN && chain_out && tid < BM) te_b = a.bias != nullptr ? a.bias[nx_cotile * BM + tid] : 0.0f;   // the next item's bias entries
    const bool want_stats = a.gn_stats != nullptr;
    const int Ho = a.Hl, Wo = a.Wl;
    const unsigned oplane = (unsigned)Ho * Wo;
    const int tiles_xo = Wo / 64;
    const int ec = tid >> 4, eu = tid & 15;                 // read-out: channels ec, ec + 16, high-res columns 4 eu .. 4 eu + 3 of the tile
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        if (y0 + 2 * g < a.H) {                             // (block-uniform: the barriers inside are taken by every thread or none)
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            if (i + g + k > 0) __syncthreads();             // (the image is rewritten: the previous pass has been read out)
            if ((wave >> 1) == g) {
#pragma unroll
              for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)              // low-res row 2 g + jj, columns 32 k + m: position tile j = 2 jj + k
#pragma unroll
                  for (int r4 = 0; r4 < 4; ++r4) {
                    floatx4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = emo_acc_read(acc[p][i][2 * jj + k][4 * r4 + e]) * a.out_scale;
                    const int m = r4 * 8 + half * 4;        // (the accumulator's rows 4 r4 .. 4 r4 + 3: four consecutive columns)
                    *reinterpret_cast<floatx4*>(img + l32 * Cfg::EPI_CS + (2 * jj + p) * 64 + wq * 32 + m) = v;
                  }
            }
            __syncthreads();
            const int ptile = ((y0 >> 1) + g) * tiles_xo + (x0 >> 5) + k;       // the 4 x 64 high-res tile
            float s_[2] = {0.0f, 0.0f};
            floatx4 v_[2][4];
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
              const int c = cc * 16 + ec;
              const float bs = smem[Cfg::OFF_BIAS_F + i * 32 + c];
              float* const obase = a.out + ((long)it_n * a.Cout + cotile * BM + i * 32 + c) * oplane;
#pragma unroll
              for (int hr = 0; hr < 4; ++hr) {
                const float2 e0 = *reinterpret_cast<const float2*>(img + c * Cfg::EPI_CS + hr * 64 + 2 * eu);
                const float2 e1 = *reinterpret_cast<const float2*>(img + c * Cfg::EPI_CS + hr * 64 + 32 + 2 * eu);
                const floatx4 v = floatx4{e0.x, e1.x, e0.y, e1.y} + floatx4{bs, bs, bs, bs};
                v_[cc][hr] = v;
                float* const op = obase + (unsigned)(2 * y0 + 4 * g + hr) * Wo + (2 * x0 + 64 * k + 4 * eu);
                if (EMO_CONV_NT_STORE) __builtin_nontemporal_store(v, reinterpret_cast<floatx4*>(op));
                else *reinterpret_cast<floatx4*>(op) = v;
                s_[cc] += (v[0] + v[1]) + (v[2] + v[3]);
              }
            }
            if (want_stats) {
              // (mean, M2) of the tile for two channels: 16 lanes of a DPP row per channel, 16 values per lane
              emo_row16_sum_n<2>(s_);
              float m2_[2] = {0.0f, 0.0f};
#pragma unroll
              for (int cc = 0; cc < 2; ++cc) {
                s_[cc] *= 1.0f / 256.0f;
#pragma unroll
                for (int hr = 0; hr < 4; ++hr)
#pragma unroll
                  for (int e = 0; e < 4; ++e) {
                    const float d = v_[cc][hr][e] - s_[cc];
                    m2_[cc] = __fmaf_rn(d, d, m2_[cc]);
                  }
              }
              emo_row16_sum_n<2>(m2_);
              if (eu == 0) {
#pragma unroll
                for (int cc = 0; cc < 2; ++cc)
                  reinterpret_cast<float2*>(a.gn_stats)[((long)it_n * (oplane / 256) + ptile) * a.Cout + cotile * BM + i * 32 + cc * 16 + ec] =
                      make_float2(s_[cc], m2_[cc]);
              }
            }
          }
        }
      }
      if (i == 0) { EMO_S_STAMP(8) }
    }
    EMO_S_STAMP(9)
#if EMO_S_TIMING
    EMO_S_STAMP(3)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    EMO_S_STAMP(4)
    {
      const int ep_L_ = l_base + idx8;
      if (tid == 0 && ep_L_ < EMO_S_TLOG_N) {
        unsigned long long* t_ = emo_s_tlog + (long)ep_L_ * EMO_S_TLOG_W;
#pragma unroll
        for (int k = 0; k < 12; ++k) t_[k] = tstamp[k];
        t_[12] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_ID
        t_[13] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20);    // XCC_ID
        t_[14] = (unsigned long long)blockIdx.x;
        t_[15] = (unsigned long long)(chained_in ? 1 : 0);
      }
      if (EMO_S_TIMING == 2 && lane == 0 && ep_L_ < EMO_S_TLOG_N / 8) {   // per-wave barrier accounting: rows N/4 + 4 item + wave
        unsigned long long* w_ = emo_s_tlog + ((long)EMO_S_TLOG_N / 4 + (long)ep_L_ * 4 + wave) * EMO_S_TLOG_W;
        w_[0] = tw_wait; w_[1] = tw_bar; w_[2] = tw_n; w_[3] = tstamp[2] - tstamp[1];
      }
    }
#endif
    // item end: the image and the bias are rewritten by the next item (its epilogue, its prologue), the tables, the patch buffers
    // and W by a full prologue -- every wave must be out of the epilogue first
    __syncthreads();
    chained_in = chain_out;
  }
  if (a.sat_flag != nullptr && sat_m > 65504.0f) *a.sat_flag = 1;   // (every writer stores the same value)
#undef EMO_U_WPTR
#undef EMO_U_DECODE
#undef EMO_U_NEXT_STAGE_BEGIN
#undef EMO_U_LOAD_FRAGS_PLANE
#undef EMO_U_ISSUE_BEGIN
#undef EMO_U_ISSUE_LOADS
#undef EMO_U_TOUCH_QUAD
#undef EMO_U_CONV_PIXEL
#undef EMO_U_DMA_PIECE
}

// The launch form (the Python planner asks emo_conv_accepts for it): 2-D, 3x3 with the fused nearest x2 upsample, no
// K split, no residual, no activation, not a guarded launch, whole 64-channel tiles, a multiple of 8 input channels (at most SCT
// with an affine), a low-res width that is a multiple of 64 and an even low-res height (items are 4 rows: the last ones of a
// height that is no multiple of 4 are half empty), 16-byte aligned input and output, input
// offsets inside 2^32 bytes per sample, output planes inside 2^31 elements.
int conv_f16x2_up2_launch(ConvArgs a, hipStream_t s) {
  using Cfg = ConvCfgUp2;
  if (a.KD != 1 || a.D != 1 || a.ksplit != 1 || a.res != nullptr || a.act != EMO_ACT_NONE || a.run_if != nullptr) return EMO_ERR_UNSUPPORTED;
  if (a.Cout % Cfg::BM || a.Cin % 8 || (a.scale && a.Cin > Cfg::SCT)) return EMO_ERR_UNSUPPORTED;
  if (a.W % Cfg::TWL || a.H % 2) return EMO_ERR_UNSUPPORTED;
  if (!emo_aligned16(a.x) || !emo_aligned16(a.out)) return EMO_ERR_ALIGN;
  if (!conv_offsets32(a) || (long)a.Hl * a.Wl >= (1l << 31)) return EMO_ERR_UNSUPPORTED;
  const long nt = (long)(a.W / Cfg::TWL) * ((a.H + Cfg::TRL - 1) / Cfg::TRL);
  const int cot = a.Cout / Cfg::BM;
  if (a.N > 65535 || nt * cot * a.N > 0x7fffffffL) return EMO_ERR_UNSUPPORTED;
  auto kern = conv_igemm_f16x2_up2_kernel;
  const int rc = emo_raise_dynamic_lds(kern);
  if (rc != EMO_OK) return rc;
  a.tiles_x = a.W / Cfg::TWL;
  a.tiles_y = (a.H + Cfg::TRL - 1) / Cfg::TRL;
  a.tiles_z = 1;
  a.n_cchunks = (a.Cin + Cfg::KC - 1) / Cfg::KC;
  a.stages_per_split = a.n_cchunks;
  a.partial = nullptr;
  a.cot0 = 0;
  a.n_cotiles = cot;
  a.n_work = (int)(nt * cot * a.N);
  const int ncu = emo_cu_count();
  const int grid = a.n_work > ncu ? ncu : a.n_work;
  return emo_launch(kern, dim3((unsigned)grid), dim3(256), (size_t)Cfg::LDS_BYTES, s, a);
}

#if EMO_S_TIMING
// measurement builds only: the per-work-item phase stamps of the last phase-kernel launch (EMO_S_TIMING, conv_igemm_bf16x3.h)
extern "C" int emo_debug_conv_timing_up2(unsigned long long* host_out, int n_items) {
  if (!host_out || n_items < 0 || n_items > EMO_S_TLOG_N) return EMO_ERR_BAD_ARG;
  if (hipDeviceSynchronize() != hipSuccess) return EMO_ERR_BAD_ARG;
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(emo_s_tlog), (size_t)n_items * EMO_S_TLOG_W * sizeof(unsigned long long)) == hipSuccess ? EMO_OK : EMO_ERR_BAD_ARG;
}
#endif
