// gms_loss.h - the GMS / MSGMS loss kinds (csrc/kernels_gms.hip) as srad_loss_* of kernels_loss.hip calls them.
#pragma once
#include <stddef.h>

// levels of a loss kind: SRAD_LOSS_GMS 1, SRAD_LOSS_MSGMS 4
int srad_gms_loss_levels(int kind);
// the checks (C, level geometry) and the workspace size; `what` starts each message
int srad_gms_loss_workspace_bytes(const char* what, int kind, int B, int C, int H, int W, size_t* bytes);
int srad_gms_loss_forward(int kind, const float* sr, const float* hr, int B, int C, int H, int W, float rgb_range, double* out2,
                          void* workspace, void* stream);
int srad_gms_loss_backward(int kind, const float* sr, int B, int C, int H, int W, float rgb_range, const float* gscale_dev,
                           float weight, float* dsr, int accumulate, void* workspace, void* stream);
