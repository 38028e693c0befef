// Internal interface of the 2D SSN head's low-resolution combination (accumulate.hip), for the validation reduction
// (valstep.hip) that runs it as its first launch.  No argument checks: the callers have made them.
#pragma once
#include "common.h"

// comb [S][B * pix][C] = mean + sum_r factor_r * eps_w[s][b][r], expm [B * pix][C] = exp(mean) (nullable); generated eps_w of
// image b come from the streams of the global item item0 + b
int vx_ssn2d_lowres_launch(const float* mean, int mean_pitch, const float* factor, int factor_pitch, const float* eps_w, uint32_t seed,
                           uint32_t item0, int B, int64_t pix_per_image, int S, int C, int R, float* comb, float* expm, hipStream_t s,
                           const char* who);
