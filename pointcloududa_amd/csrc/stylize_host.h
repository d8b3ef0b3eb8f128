// The launch loop of pcuda_stylize (stylize.hip), shared with pcuda_stylize_connect (spx_connect.hip): host code only, the
// kernels stay where they are.
#pragma once
#include "common.h"

// called behind the three launches of slot `slot`: `slot_in` is the slot's input image [b][h][w][c], `slot_out` the image the
// slot wrote, `labels` the uint8 label plane [b][h][w] the superpixel kernel left for the samples whose slot is SUPERPIXELS
typedef int (*StyleSlotHook)(void* ctx, int slot, const uint8_t* slot_in, uint8_t* slot_out, const uint8_t* labels);

// validates like pcuda_stylize (the first pcuda_stylize_workspace_size bytes of the workspace are its own; `workspace_need`
// is what the caller's hook needs in all, 0 for none) and launches every slot; a hook that is not null runs behind each slot
// and a status other than PCUDA_OK from it ends the loop.  `scale`: 0 from pcuda_stylize and pcuda_stylize_connect (iarg[6] is
// never read); 1 from pcuda_stylize_scaled (spx_scale.hip, f9c): the superpixel kernel leaves the samples whose slot is
// scaled (imgdev::spx_working_size) to the hook, which has to write their part of `slot_out`
int stylize_run(const uint8_t* in, uint8_t* out, int b, int h, int w, int c, int slots, const int* opcode, const int* iarg,
                const double* farg, const double* table, const unsigned long long* seed, void* workspace, size_t workspace_bytes,
                size_t workspace_need, pcuda_stream_t s, StyleSlotHook hook, void* ctx, int scale);

// f9c, for pcuda_stylize_scaled's hook.  Both work on images and planes [b][h][w]([c]) whose samples stay h w pixels apart
// while a scaled sample's rows are w' pixels long (its h' w' pixels are the first of its plane), and both leave flag[n] = 1
// iff a final segment of scaled sample n is replaced:
//   stylize_superpixels_scaled  the superpixel kernel (stylize.hip) on the scaled samples of slot `slot` alone: `small` ->
//                               `painted`, the label plane to `labels`; flag[n] must be 0 before
//   spx_connect_scaled          the eight launches of the connectivity pass (spx_connect.hip): scale = 1 for the samples whose
//                               slot is not scaled (pcuda_stylize_connect's pass, `flag` unused), scale = 2 for the scaled ones
//                               (which resets flag[n] first); `conn_workspace` = the connect workspace behind pcuda_stylize's part
int stylize_superpixels_scaled(const uint8_t* small, uint8_t* painted, uint8_t* labels, int* flag, int b, int h, int w, int c,
                               int slots, int slot, const int* opcode, const int* iarg, const unsigned long long* seed,
                               pcuda_stream_t s);
int spx_connect_scaled(const uint8_t* slot_in, uint8_t* slot_out, const uint8_t* labels, void* conn_workspace, int* flag, int scale,
                       int b, int h, int w, int c, int slots, int slot, const int* opcode, const int* iarg,
                       const unsigned long long* seed, pcuda_stream_t s);
