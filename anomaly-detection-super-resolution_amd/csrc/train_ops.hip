// train_ops.hip - the C ABI of the training step's model-independent launches: the L1 gradient seed, the fused Adam steps (plain,
// with the weight EMA, guarded) and the gradient guard.  The DRCT and the DRN trainer call the same functions.
#include "srad_common.h"

extern "C" {

/* sign(a - b) * scale: the gradient seed of nn.L1Loss(reduction='mean') when scale = 1 / numel (src/loss.py:84) */
int srad_l1_grad(const float* a, const float* b, float* out, int64_t n, float scale, void* stream) {
  SRAD_REQUIRE(a && b && out && n > 0, "l1_grad: bad argument");
  return srad_launch_l1_grad(a, b, out, (size_t)n, scale, reinterpret_cast<hipStream_t>(stream));
}

/* torch.optim.Adam step on flat buffers (src/trainer.py:49-59: lr 1e-4, betas (0.9, 0.999), eps 1e-8, L2 weight decay) */
int srad_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream) {
  SRAD_REQUIRE(params && grads && exp_avg && exp_avg_sq && n > 0, "adam_step: bad argument");
  return srad_launch_adam(params, grads, exp_avg, exp_avg_sq, (size_t)n, lr, beta1, beta2, eps, weight_decay, step,
                          grad_scale, reinterpret_cast<hipStream_t>(stream));
}

/* the same step with [lr, 1 - beta1^t, sqrt(1 - beta2^t), grad_scale] in device memory (hipGraph replay of a training step) */
int srad_adam_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                       float beta2, float eps, float weight_decay, const float* dev_hyper, void* stream) {
  SRAD_REQUIRE(params && grads && exp_avg && exp_avg_sq && dev_hyper && n > 0, "adam_step_dev: bad argument");
  return srad_launch_adam_dev(params, grads, exp_avg, exp_avg_sq, (size_t)n, beta1, beta2, eps, weight_decay, dev_hyper,
                              reinterpret_cast<hipStream_t>(stream));
}

/* srad_adam_step / srad_adam_step_dev that also keep the weights' exponential moving average (BasicSR's model_ema) in the same
   launch: after the step ema = fl(fl(ema_decay * ema) + fl((1 - ema_decay) * params)); params, exp_avg, exp_avg_sq get the bits of
   the plain step */
int srad_adam_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, float ema_decay,
                       void* stream) {
  SRAD_REQUIRE(params && grads && exp_avg && exp_avg_sq && n > 0, "adam_ema_step: bad argument");
  return srad_launch_adam_ema(params, grads, exp_avg, exp_avg_sq, ema, (size_t)n, lr, beta1, beta2, eps, weight_decay, step,
                              grad_scale, ema_decay, reinterpret_cast<hipStream_t>(stream));
}

int srad_adam_ema_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                           float beta1, float beta2, float eps, float weight_decay, float ema_decay, const float* dev_hyper,
                           void* stream) {
  SRAD_REQUIRE(params && grads && exp_avg && exp_avg_sq && dev_hyper && n > 0, "adam_ema_step_dev: bad argument");
  return srad_launch_adam_ema_dev(params, grads, exp_avg, exp_avg_sq, ema, (size_t)n, beta1, beta2, eps, weight_decay, ema_decay,
                                  dev_hyper, reinterpret_cast<hipStream_t>(stream));
}

/* Guarded step (include/srad.h): the workspace size, the two guard launches and the two Adam steps that obey the record */
int srad_grad_guard_workspace(int64_t n, int* slots, size_t* bytes) {
  SRAD_REQUIRE(n > 0 && (slots || bytes), "grad_guard_workspace: bad argument");
  const int s = srad_guard_slots_for((size_t)n);
  if (slots) *slots = s;
  if (bytes) *bytes = SRAD_GUARD_HEADER_BYTES + (size_t)s * sizeof(double);
  return SRAD_OK;
}

int srad_grad_guard_partials(const float* grads, int64_t n, void* workspace, size_t workspace_bytes, int first_slot,
                             void* stream) {
  SRAD_REQUIRE(grads && workspace && n > 0, "grad_guard_partials: bad argument");
  return srad_launch_grad_guard_partials(grads, (size_t)n, workspace, workspace_bytes, first_slot,
                                         reinterpret_cast<hipStream_t>(stream));
}

int srad_grad_guard_finalize(void* workspace, size_t workspace_bytes, int n_slots, const float* dev_hyper, float beta1,
                             float beta2, double max_norm, void* stream) {
  SRAD_REQUIRE(workspace && dev_hyper, "grad_guard_finalize: bad argument");
  return srad_launch_grad_guard_finalize(workspace, workspace_bytes, n_slots, dev_hyper, beta1, beta2, max_norm,
                                         reinterpret_cast<hipStream_t>(stream));
}

int srad_adam_guarded_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                           float beta2, float eps, float weight_decay, const void* workspace, void* stream) {
  SRAD_REQUIRE(params && grads && exp_avg && exp_avg_sq && workspace && n > 0, "adam_guarded_step: bad argument");
  return srad_launch_adam_guarded(params, grads, exp_avg, exp_avg_sq, (size_t)n, beta1, beta2, eps, weight_decay, workspace,
                                  reinterpret_cast<hipStream_t>(stream));
}

int srad_adam_ema_guarded_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                               float beta1, float beta2, float eps, float weight_decay, float ema_decay, const void* workspace,
                               void* stream) {
  SRAD_REQUIRE(params && grads && exp_avg && exp_avg_sq && workspace && n > 0, "adam_ema_guarded_step: bad argument");
  return srad_launch_adam_ema_guarded(params, grads, exp_avg, exp_avg_sq, ema, (size_t)n, beta1, beta2, eps, weight_decay,
                                      ema_decay, workspace, reinterpret_cast<hipStream_t>(stream));
}

/* dst[0..3] = (a, b, c, d) by value through a kernel: how the host hands Adam's per-step scalars to a replayed graph */
int srad_set4(float* dst, float a, float b, float c, float d, void* stream) {
  SRAD_REQUIRE(dst, "set4: null argument");
  return srad_launch_set4(dst, a, b, c, d, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
