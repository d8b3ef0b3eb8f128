// Helpers shared by the loss sources (losses.hip, dice_loss.hip).
#pragma once
#include "common.h"

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// grid of a grid-stride pointwise kernel: one 256-thread block per 256 elements, at most 4096 blocks
static inline int grid_for(long long n) { long long b = (n + 255) / 256; return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)); }
