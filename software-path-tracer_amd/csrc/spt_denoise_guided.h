// spt_denoise_guided.h — host launchers of the variance-guided a-trous filter's kernels
// (spt_denoise_guided.hip). Internal.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spt_atrous_guided.h"

namespace spt {

// The two forms of one guided level, as spt_denoise.h's: kGuidedStraight reads its 25 taps
// from global memory; kGuidedTiled stages one residue class's 20 x 20 records in LDS. Same bits.
constexpr int kGuidedStraight = 0;
constexpr int kGuidedTiled = 1;
// the form the library runs at `step` (measured, profiles/guided_rates.txt)
int guided_form_of_step(int step);

// var[i] = the variance of the mean luminance of pixel i of a w x h image of noise moments (mean, m2, prevL, 0):
// fmaxf(m2 * inv, 0), through the 3 x 3 prefilter if `prefilter`
void launch_guided_variance(const float4* moments, float* var, uint32_t w, uint32_t h, float inv, bool prefilter,
                            hipStream_t s);
// (out, out_var) = level lv of (color / divisor, var) over a w x h image; divisor 0: the colour is already the mean
void launch_guided_level(int form, const float4* color, float divisor, const float* var, const float4* feat_a,
                         const float4* feat_b, float4* out, float* out_var, uint32_t w, uint32_t h,
                         const GuidedLevel& lv, hipStream_t s);

}  // namespace spt
