// Per-element arithmetic of the parameter side, shared by quant.hip and fwht.hip (the launches fused with the Hadamard
// transform): the UAQ and AdaRound fake-quant (reference quantization/quantizer.py:117-119, 288-303), their backwards with the
// rounding regulariser's gradient (calib_model.py:39-47), Adam's update, and the per-step scalars.  ONE op sequence per
// operation (the files are built with -ffp-contract=off), so every caller produces the same bits.
#pragma once
#include "nq_common.h"

__device__ __forceinline__ float soft_target_lin(float a) { return nq_sigmoid(a) * (NQ_ZETA - NQ_GAMMA) + NQ_GAMMA; }

__device__ __forceinline__ float uaq_fwd_elem(float xv, float d, float z, float qmax) {
  float xi = rintf(xv / d) + z;
  float xq = fminf(fmaxf(xi, 0.f), qmax);
  return (xq - z) * d;
}
// this element's term of d(delta); inside = 1{0 <= rint(x/delta)+zp <= L-1}, the mask of the gradient w.r.t. x
__device__ __forceinline__ float uaq_bwd_term(float xv, float gyv, float d, float z, float qmax, float& inside) {
  float u = xv / d;
  float xi = rintf(u) + z;
  float xq = fminf(fmaxf(xi, 0.f), qmax);
  inside = (xi >= 0.f && xi <= qmax) ? 1.f : 0.f;
  return gyv * ((xq - z) - inside * u);
}

__device__ __forceinline__ float ada_fwd_elem(float xv, float a, float d, float z, float qmax, int soft, float& xq) {
  float h = soft ? fminf(fmaxf(soft_target_lin(a), 0.f), 1.f) : (a >= 0.f ? 1.f : 0.f);
  float xi = (floorf(xv / d) + h) + z;
  xq = fminf(fmaxf(xi, 0.f), qmax);
  return (xq - z) * d;
}
__device__ __forceinline__ float ada_bwd_elem(float xv, float gyv, float a, float d, float z, float qmax, float reg_weight,
                                              float reg_b) {
  float s = nq_sigmoid(a);
  float lin = s * (NQ_ZETA - NQ_GAMMA) + NQ_GAMMA;
  float h = fminf(fmaxf(lin, 0.f), 1.f);
  float hp = (lin >= 0.f && lin <= 1.f) ? (NQ_ZETA - NQ_GAMMA) * (s * (1.f - s)) : 0.f;
  float xi = (floorf(xv / d) + h) + z;
  float inside = (xi >= 0.f && xi <= qmax) ? 1.f : 0.f;
  float g = gyv * d * inside * hp;
  if (reg_weight != 0.f) {
    // R = w * sum(1 - (2|h-.5|)^b);  dR/dh = -w * b * (2|h-.5|)^(b-1) * 2 * sign(h-.5)
    float c = h - 0.5f;
    float t = fabsf(c) * 2.f;
    float sg = (c > 0.f) ? 1.f : ((c < 0.f) ? -1.f : 0.f);
    // t^(b-1), t in [0,1], b-1 >= 1, as exp2((b-1) * log2 t) on the two hardware transcendentals (relative error ~2e-6 at
    // b = 20; t = 0 -> 2^-inf = 0 like powf): the library powf was half of this kernel's time
    const float tp = __builtin_amdgcn_exp2f((reg_b - 1.f) * __builtin_amdgcn_logf(t));
    float dRdh = -reg_weight * (reg_b * tp) * 2.f * sg;
    g += dRdh * hp;
  }
  return g;
}

// Adam (torch/optim/adam.py _single_tensor_adam, no weight decay, no amsgrad)
__device__ __forceinline__ void adam_elem(float g, float& m, float& v, float& p, float step_size, float beta1, float beta2,
                                          float eps, float bc2_sqrt) {
  m = m + (1.f - beta1) * (g - m);             // exp_avg.lerp_(grad, 1-beta1)
  v = v * beta2 + (1.f - beta2) * (g * g);     // mul_(beta2).addcmul_(g, g, value=1-beta2)
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p = p - step_size * (m / denom);             // addcdiv_(exp_avg, denom, value=-step_size)
}

// The scalars that change from one calibration step to the next: from the host arguments, or (dyn != NULL; graph replays)
// from the device array nq_step_prologue fills: {reg_b, regulariser gate, lr/(1-beta1^t), sqrt(1-beta2^t)}.
struct StepScalars {
  float reg_b, gate, step_size, bc2_sqrt;
  bool dyn;
  __device__ __forceinline__ StepScalars(const float* __restrict__ d, float reg_b_, float step_size_, float bc2_sqrt_)
      : reg_b(reg_b_), gate(1.f), step_size(step_size_), bc2_sqrt(bc2_sqrt_), dyn(d != nullptr) {
    if (d) {
      reg_b = d[0];
      gate = d[1];
      step_size = d[2];
      bc2_sqrt = d[3];
    }
  }
  // a segment's regulariser weight under the warm-up gate (exactly 0 or 1)
  __device__ __forceinline__ float reg_weight(float w) const { return dyn ? w * gate : w; }
};
