// The launch loop of pcuda_stylize (stylize.hip), shared with pcuda_stylize_connect (spx_connect.hip): host code only, the
// kernels stay where they are.
#pragma once
#include "common.h"

// called behind the three launches of slot `slot`: `slot_in` is the slot's input image [b][h][w][c], `slot_out` the image the
// slot wrote, `labels` the uint8 label plane [b][h][w] the superpixel kernel left for the samples whose slot is SUPERPIXELS
typedef int (*StyleSlotHook)(void* ctx, int slot, const uint8_t* slot_in, uint8_t* slot_out, const uint8_t* labels);

// validates like pcuda_stylize (the first pcuda_stylize_workspace_size bytes of the workspace are its own; `workspace_need`
// is what the caller's hook needs in all, 0 for none) and launches every slot; a hook that is not null runs behind each slot
// and a status other than PCUDA_OK from it ends the loop
int stylize_run(const uint8_t* in, uint8_t* out, int b, int h, int w, int c, int slots, const int* opcode, const int* iarg,
                const double* farg, const double* table, const unsigned long long* seed, void* workspace, size_t workspace_bytes,
                size_t workspace_need, pcuda_stream_t s, StyleSlotHook hook, void* ctx);
