// The three launches of cg_offset_prior_add (offset_prior.hip), as engine.cpp hands them over:
// the model's weights resolved to pointers, everything else as the caller gave it.
#pragma once
#include <stdint.h>

struct cg_offprior_args {
  int dtype;            // CG_F32 / CG_BF16: hist, the weights w1 / w2 / head and u1 / u2
  int n, B, d, V, Tmax;
  int offset[8];        // cfg.offsets[head[i]]
  float weight[8];
  const void* w1[8];    // [d][d], K-contiguous
  const void* w2[8];
  const float* b1[8];   // fp32 in either mode
  const float* b2[8];
  const void* head;     // [V][d]
  const void* hist;     // [B][Tmax][d]
  const int32_t* pos;
  void* u1;             // [n][B][d]
  void* u2;
  float* logits;
  long long ldl;
};

extern "C" int cg_offset_prior_stages(const cg_offprior_args* a, void* stream);
