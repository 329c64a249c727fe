// spt_denoise.h — host launchers of the first-hit feature kernel (spt_kernels.hip, beside the intersectors
// it calls) and of the a-trous filter kernels (spt_denoise.hip). Internal.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spt_atrous.h"
#include "spt_kernels.h"

namespace spt {

// One camera ray per shard pixel (the reference pinhole, the posed camera through the pixel's corner, or
// through its centre with SPT_CAMERA_JITTER; no RNG draw) and its closest hit, as three float4 images:
//   feat_a = (P, caller's material bits)  feat_b = (n, t)  albedo = (albedo, primitive bits)
// mat_map[m]: the caller's material index behind device material m.
void launch_features(const PassParams& p, const uint32_t* mat_map, float4* feat_a, float4* feat_b, float4* albedo,
                     hipStream_t s);

// The two forms of one filter level: kAtrousStraight reads its 25 taps from global
// memory; kAtrousTiled stages one residue class's 20 x 20 records in LDS. Same bits.
constexpr int kAtrousStraight = 0;
constexpr int kAtrousTiled = 1;
// the form the library runs at `step` (measured, profiles/denoise_rates.txt)
int atrous_form_of_step(int step);
// out = level lv of (color / divisor) over a w x h image; divisor 0: the colour is already the mean
void launch_atrous(int form, const float4* color, float divisor, const float4* feat_a, const float4* feat_b,
                   float4* out, uint32_t w, uint32_t h, const AtrousLevel& lv, hipStream_t s);

}  // namespace spt
