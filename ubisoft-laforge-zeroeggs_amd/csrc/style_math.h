// The mix of a live row's style from the style bank (live_styles.hip; include/zeggs_hip_styles.h; the definition is DESIGN.md
// 3.7), stated once: what a bank slot holds of an encoder row, one column of the mixed row, and what the call makes of the
// row's old / new pair.  Plain C++ behind a qualifier macro (no HIP include), so the same text runs in the kernels and in
// tests/host/style_math_check.cpp.  The sum is float64 arithmetic over the float32 operands; it becomes float32 once, where
// it is stored.  Every multiply-add of the sum is a written-out fma(): the host compile and the device compile then mean the
// same operations whatever either compiler's contraction default is.  The fade's weight and the lerp are gaze_math.h's.
#pragma once
#include <math.h>

#include "gaze_math.h"

#define STYLE_MAX_TERMS 8

// what a slot holds of column c of an encoder row: the mean, and the deviation exp(logvar / 2) -- vae_fwd_k's float32 expression
ZG_HD float style_slot_mean(const float* enc, int c) { return enc[c]; }
ZG_HD float style_slot_dev(const float* enc, int ST, int E, int c) { return E == 2 * ST ? expf(0.5f * enc[ST + c]) : 0.0f; }

// column c of the mixed row: sum_i w_i (mean_i[c] + (dev_i[c] / temperature) eps_i[c]), i = 0 .. terms - 1 in this order, float64;
// bank [.][2][ST]; eps [STYLE_MAX_TERMS][ST], the record's noise, or NULL (the means alone, as with temperature 0).  The loop
// runs over all STYLE_MAX_TERMS with the count as a guard, so that unrolled nothing is indexed by a variable.
ZG_HD double style_mix_sum(const int* slot, const float* weight, int terms, const float* bank, int ST, int c, const float* eps,
                           float temperature) {
  const bool noise = eps != nullptr && temperature > 0.0f;
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < STYLE_MAX_TERMS; ++i) {
    if (i < terms) {
      const float* s = bank + (long)slot[i] * 2 * ST;
      double v = (double)s[c];
      if (noise) v = fma((double)s[ST + c] / (double)temperature, (double)eps[(long)i * ST + c], v);
      acc = fma((double)weight[i], v, acc);
    }
  }
  return acc;
}

// the row's new old column: where the fade (k_style, fade_style) stands at frame k - 1, live_condition_k's statement
ZG_HD float style_collapse(float old_c, float new_c, long k, long k_style, long fade_style) {
  return gaze_style_lerp(old_c, new_c, gaze_style_weight(k - 1, k_style, fade_style));
}

// one column of a mix call: old_c / new_c in, the new pair out
ZG_HD void style_mix_column(const int* slot, const float* weight, int terms, const float* bank, int ST, int c, const float* eps,
                            float temperature, long k, long k_style, long fade_style, int reset, float* old_c, float* new_c) {
  const float mixed = (float)style_mix_sum(slot, weight, terms, bank, ST, c, eps, temperature);
  *old_c = reset ? mixed : style_collapse(*old_c, *new_c, k, k_style, fade_style);
  *new_c = mixed;
}
