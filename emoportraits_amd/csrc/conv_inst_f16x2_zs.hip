// the depth-shared 32-row kernel of conv_igemm_f16x2_zs.h (fp16 two-term split, 3x3x3, 4 x 64 tiles, block config F) and the
// rule that sends a config-F launch to it
#include "conv_dispatch.h"
#include "conv_igemm_bf16x3.h"
#include "conv_igemm_f16x2_zs.h"

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void conv_igemm_f16x2_zs_kernel(const ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)reinterpret_cast<char*>(smem);
  conv_f16x2_zs_body(a, smem, smem_lds);
}

// EMO_CONV_ZS_RUN (measurements and tests; read at every launch): 0 = never, k > 0 = runs of k output slices whatever the
// launch's size (the tests' small volumes would otherwise stay on the one-slice kernel), unset = the rule
static int conv_f16x2_zs_choose(int N, int Cout, int D, int H, int W, int ncu) {
  const char* e = getenv("EMO_CONV_ZS_RUN");
  if (e && *e) {
    const int k = atoi(e);
    if (k <= 0 || H % ConvCfgZ::TR || W % ConvCfgZ::TW) return 0;
    return k < D ? k : D;
  }
  return conv_f16x2_zs_run_length(N, Cout, D, H, W, ncu);
}

static int zs_last_run = 0;

// The config-F launcher of 4 x 64 tiles: 3x3x3 layers the rule takes run the depth-shared kernel, everything else (2-D layers,
// launches too small to fill the chip with any run, more input channels than its tables hold) the one-slice kernel
int conv_f16x2_bm32_4x64(ConvArgs a, hipStream_t s) {
  int unused = 0;
  int& last_run = emo_dry_run.on ? unused : zs_last_run;      // (a question to emo_conv_accepts is no launch)
  last_run = 0;
  const bool fits = a.KD == 3 && a.ksplit == 1 && a.run_if == nullptr && a.cot0 == 0 && !a.res_ups && a.Cin % 8 == 0 &&
                    a.Cin <= ConvCfgZ::SCT && a.D == a.Dl && a.H == a.Hl && a.W == a.Wl && a.N <= 65535 &&
                    conv_offsets32(a) && emo_aligned16(a.x);
  const int ncu = emo_cu_count();
  const int run = fits ? conv_f16x2_zs_choose(a.N, a.Cout, a.D, a.H, a.W, ncu) : 0;
  if (run <= 0) return conv_igemm_bf16x3_launch<4, 64, false, 2, 32>(a, s);
  a.tiles_x = a.Wl / ConvCfgZ::TW;
  a.tiles_y = a.Hl / ConvCfgZ::TR;
  a.tiles_z = a.Dl;
  a.n_cchunks = (a.Cin + ConvCfgZ::KC - 1) / ConvCfgZ::KC;
  a.n_cotiles = (a.Cout + ConvCfgZ::BM - 1) / ConvCfgZ::BM;
  a.stages_per_split = a.n_cchunks * a.KD;
  a.partial = nullptr;
  a.zrun = run;
  const long items = (long)a.N * a.tiles_y * a.tiles_x * ((a.D + run - 1) / run) * a.n_cotiles;
  if (items > 0x7fffffffL || (long)a.tiles_x * a.tiles_y * a.tiles_z > 0x7fffffffL) return EMO_ERR_UNSUPPORTED;
  a.n_work = (int)items;
  auto kern = conv_igemm_f16x2_zs_kernel;
  const int rc = emo_raise_dynamic_lds(kern);
  if (rc != EMO_OK) return rc;
  const int grid = a.n_work > ncu ? ncu : a.n_work;       // persistent blocks: block b walks items b, b + grid, ...
  last_run = run;
  return emo_launch(kern, dim3((unsigned)grid), dim3(256), (size_t)ConvCfgZ::LDS_BYTES, s, a);
}

// the run length the rule gives a config-F 3x3x3 launch of these sizes on `ncu` compute units (0: the one-slice kernel;
// ncu <= 0: this device's, and the EMO_CONV_ZS_RUN switch applies as it does to a launch)
extern "C" int emo_debug_conv_zs_run(int N, int Cout, int D, int H, int W, int ncu) {
  if (ncu <= 0) return conv_f16x2_zs_choose(N, Cout, D, H, W, emo_cu_count());
  return conv_f16x2_zs_run_length(N, Cout, D, H, W, ncu);
}
// the run length of the most recent config-F launch on 4 x 64 tiles (0: it ran the one-slice kernel)
extern "C" int emo_debug_conv_zs_last_run(void) { return zs_last_run; }
