// float4 helpers of the row kernels (layernorm.hip, the LayerNorm tail of skinny.hip, the casts of misc.hip).
// Only what those kernels repeat: this is not a vector algebra.
#pragma once
#include "common.h"

namespace pgca {

// acc += v
__device__ __forceinline__ void add4(float4& acc, const float4& v) {
  acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
}
// acc += w * t
__device__ __forceinline__ void fma4(float4& acc, float w, const float4& t) {
  acc.x += w * t.x; acc.y += w * t.y; acc.z += w * t.z; acc.w += w * t.w;
}

__device__ __forceinline__ void store_bf16x4(bf16_t* p, float4 v) {
  bf16x4 t;
  t[0] = (bf16_t)v.x;
  t[1] = (bf16_t)v.y;
  t[2] = (bf16_t)v.z;
  t[3] = (bf16_t)v.w;
  *reinterpret_cast<bf16x4*>(p) = t;
}

// LayerNorm's affine of four columns: (v - mean) * rstd * g + b
__device__ __forceinline__ float4 ln_affine(float4 v, float mean, float rstd, float4 g, float4 b) {
  float4 y;
  y.x = (v.x - mean) * rstd * g.x + b.x;
  y.y = (v.y - mean) * rstd * g.y + b.y;
  y.z = (v.z - mean) * rstd * g.z + b.z;
  y.w = (v.w - mean) * rstd * g.w + b.w;
  return y;
}

}  // namespace pgca
