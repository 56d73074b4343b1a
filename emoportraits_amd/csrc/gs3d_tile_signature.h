// the signature of the three per-padding entries of the LDS-staged 3-D grid_sample: defined in gs3d_tile_pad_*.hip (through
// gs3d_tile_launch.h), declared and dispatched in gs3d_tile_api.hip, which does not compile the kernels
#pragma once
#define EMO_GS3D_TILE_PAD_SIGNATURE(name)                                                                              \
  int name(const float* vol, const float* grid, const float* theta, const float* lin_x, const float* lin_y,            \
           const float* lin_z, float* out, int N, int C, int D, int H, int W, int Do, int Ho, int Wo, long vol_bstride, \
           int in_layout, int out_layout, int variant, int grid_kind, hipStream_t s)
