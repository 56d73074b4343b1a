// The four macros of the split kernels' shared stage machinery (conv_split_common.h, which includes this file) whose text only
// the GPU toolchain understands: the inline-asm waits and barriers and the LDS address-space cast.  conv_split_common.h holds
// nothing else of that kind.
// Why a file of its own, under the name the pair kernels' common header had: the host emulation of the kernels
// (tests/emul/convlib.py) compiles rewritten COPIES of the headers it lists and takes any other header from this directory as it
// stands.  Its list is derived from this directory now; before, it was fixed and named this file.  With these statements here,
// the emulation tests of an earlier commit still build against these sources -- the first thing to try when a kernel change is
// to be bisected.  For that, conv_igemm_f16.h includes this file itself, in front of conv_split_common.h: the include there is
// then resolved beside the rewritten copies, and the include guard below skips the copy beside the header that was not rewritten.
// The rewrites match the text literally: the statements and the parameter name n_ stay as they are.
#ifndef EMO_CONV_SPLIT_PAIR_COMMON_H
#define EMO_CONV_SPLIT_PAIR_COMMON_H

// (documented in conv_igemm_bf16x3.h; the default stands here as well, in front of the #if below)
#ifndef EMO_S_TIMING
#define EMO_S_TIMING 0
#endif

// ---- the block's scale / shift tables, its LDS byte address (DMA destinations), the lane's byte offset in a 1 KiB DMA piece
//      (beside EMO_SPLIT_LDS_VIEWS, conv_split_common.h) ----
#define EMO_SPLIT_LDS_TABLES_ADDR()                                                                   \
  float* const sct = smem + Cfg::OFF_SCT * 4;                                                         \
  const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)reinterpret_cast<char*>(smem); \
  const unsigned lane16 = (unsigned)lane * 16u;

// ---- waits and barriers of the block.  TIMED_BARRIER: in EMO_S_TIMING == 2 measurement builds, how long the wave sits in the
//      waitcnt of a K-loop barrier (memory / LDS latency it did not hide) and in the s_barrier itself (skew between the block's
//      waves), summed per work item and wave into the kernel's tw_wait / tw_bar / tw_n ----
#define EMO_SPLIT_WAIT(n_) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n_) : "memory")
#define EMO_SPLIT_BARRIER(n_) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(n_) : "memory")
#if EMO_S_TIMING == 2
#define EMO_SPLIT_TIMED_BARRIER(n_)                                                                   \
  {                                                                                                   \
    const unsigned long long b0_ = __builtin_amdgcn_s_memtime();                                      \
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(n_) : "memory");                              \
    const unsigned long long b1_ = __builtin_amdgcn_s_memtime();                                      \
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                                  \
    const unsigned long long b2_ = __builtin_amdgcn_s_memtime();                                      \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                \
    tw_wait += b1_ - b0_; tw_bar += b2_ - b1_; ++tw_n;                                                \
  }
#else
#define EMO_SPLIT_TIMED_BARRIER(n_) EMO_SPLIT_BARRIER(n_)
#endif

#endif  // EMO_CONV_SPLIT_PAIR_COMMON_H
