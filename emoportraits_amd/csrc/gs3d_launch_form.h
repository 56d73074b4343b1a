// The launch decision of the 3-D sampler (ABI 29): which kernel a call takes and with what plan.  Each launcher has ONE host
// function that fills this record -- direct_form (grid_sample3d.hip) for the direct kernels, tile_form (gs3d_tile_launch.h) for
// the LDS-staged ones -- calls it before it launches, and launches what it says; emo_grid_sample3d_launch_form reports the same
// record without launching.  The functions make no HIP call.  Plain C++: also read by the host-compiled test libraries.
#pragma once
#include <stddef.h>

namespace gs3d {

struct LaunchForm {
  int rc;            // what the launcher returns before any launch; EMO_OK: it launches `form`
  int form;          // EMO_GS3D_FORM_*
  int order;         // block order of the channels-last kernels (block_to_work): 1 or 3; 0 for the others
  int fma, nt, bank; // fused multiply-add accumulation; non-temporal NCDHW stores; the (const int*, int) instantiation
  long gx;           // grid (gx, gy, gz)
  int gy, gz;
  long bps;          // blocks per sample (per channel chunk for the planar gather)
  int last_vox;      // output voxels of a sample's last block (0: tile kernels)
  int cpb;           // channels per block (planar gather: a chunk; channels-last: all C; tile: 4 x units or units)
  size_t lds;        // dynamic LDS bytes of the launch
  int threads, vpt, upb, txs, tys, tzs, cap_slots;   // tile kernels: block size, voxels per thread, channel units per block,
                                                     // log2 tile extents, stage slots of 16 bytes
};

}  // namespace gs3d
