// The fused epilogue every GEMM kernel of the library takes (gemm.hip,
// gemm256.hip, mxgemm.hip):  out = res + alpha * act(acc + bias), rows with
// a nonzero rowmask giving 0 before the residual.  Not part of the C ABI.
#pragma once
#include <stdint.h>

// activation ids of the C ABI (sbk_gemm's `act`, sbk_mx_gemm's `act`)
enum Act { ACT_NONE = 0, ACT_SWISH = 1, ACT_GLU = 2, ACT_LRELU = 3, ACT_GELU = 4 };

// Passed to kernels by value, alone or inside a larger argument struct: the
// field order and sizes are the kernels' argument layout.
struct GemmEpi {
  const float* bias;        // [N] (GLU: permuted like W) or null
  int act;                  // Act; GLU only in gemm.hip, Swish not in the MXFP8 kernels
  float slope;              // LeakyReLU negative slope
  const float* res;         // residual [M, ldr] fp32 or null
  int ldr;
  float alpha;              // value scale before the residual add
  const uint8_t* rowmask;   // [M]: nonzero -> value 0 before the residual
  void* out;
  int ldc;
  int out_bf16;
};
