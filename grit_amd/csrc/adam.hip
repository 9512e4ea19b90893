// Adam over one flat parameter range of the bf16-compute / fp32-master layout (grit_amd/amp.py): ONE pass that reads the
// bf16 gradient bucket (as all-reduced by RCCL), updates the fp32 master and both fp32 moments, and writes the bf16
// compute copy the next forward reads.  torch's multi-tensor fused Adam needs the gradients widened to fp32 first and a
// separate fp32 -> bf16 copy afterwards: 40 B of HBM traffic per parameter against 28 B here, and ~40 launches against ~7.
//
// Arithmetic = torch.optim.Adam (amsgrad = False, weight_decay = 0, maximize = False; reference build_optimizers,
// engine/caption_engine.py:18-73 -- the `weight_decay_rate` key of its groups is ignored by torch):
//   m <- m + (g - m) (1 - beta1);  v <- beta2 v + (1 - beta2) g^2;  p <- p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
#include "adam_flat.h"

extern "C" int grit_adam_flat(float* param, const void* grad, int grad_is_bf16, float* exp_avg, float* exp_avg_sq,
                              void* compute_bf16, long n, float lr, float beta1, float beta2, float eps, float bias_correction1,
                              float bias_correction2_sqrt, float grad_scale, void* stream) {
    if (bias_correction1 <= 0.f || bias_correction2_sqrt <= 0.f) return GRIT_ERR_BAD_ARG;
    return adam_launch<false>(param, grad, grad_is_bf16, exp_avg, exp_avg_sq, compute_bf16, n, lr, beta1, beta2, eps, bias_correction1,
                              bias_correction2_sqrt, grad_scale, nullptr, nullptr, stream);
}

extern "C" int grit_adam_flat_dev(float* param, const void* grad, int grad_is_bf16, float* exp_avg, float* exp_avg_sq,
                                  void* compute_bf16, long n, float beta1, float beta2, float eps, float grad_scale,
                                  const float* hyper, void* stream) {
    if (!hyper || ((uintptr_t)hyper % 8)) return GRIT_ERR_BAD_ARG;
    return adam_launch<false>(param, grad, grad_is_bf16, exp_avg, exp_avg_sq, compute_bf16, n, 0.f, beta1, beta2, eps, 1.f, 1.f,
                              grad_scale, hyper, nullptr, stream);
}
