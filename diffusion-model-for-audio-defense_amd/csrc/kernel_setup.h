// Per-device set-up of the kernels: the dynamic-LDS attribute (hipFuncSetAttribute acts on the current device only) and the CU count.
// Both are asked for through these two functions and nowhere else; see DESIGN.md "Per device, per engine".
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <utility>

namespace dmad {

// kernel families: one configure function each (in the family's own .hip file, listed in kernel_setup.hip)
enum : unsigned {
    KF_GEMM_F32 = 1u << 0,       // gemm_f32.hip: the 8-slot narrow tile
    KF_GEMM_X3 = 1u << 1,        // gemm_f32.hip: the split-f16 kernels
    KF_GEMM_H16 = 1u << 2,       // gemm_h16.hip
    KF_WN_LAYER = 1u << 3,       // wn_layer.hip
    KF_WN_FINAL = 1u << 4,       // wn_final.hip
    KF_M5 = 1u << 5,             // m5.hip
    KF_KWS = 1u << 6,            // kws.hip
    KF_UNET_ATT_BWD = 1u << 7,   // unet_vjp.hip: attention backward, T = 256
    KF_UNET_ATT = 1u << 8,       // unet_ops.hip: fp32 and f16 attention, T = 256
    KF_WAVE_IIR = 1u << 9,       // wave_defense.hip: wave_iir_kernel<1..8>
    KF_WAVE_FFT = 1u << 10,      // wave_fft.hip: the whole-clip real FFT pair
    KF_COUNT = 11
};
const char* kernel_family_name(unsigned family);        // of one family bit, for messages

// Makes the families of `mask` ready on the current device: the first call for a (device, family) pair runs the family's configure
// function, every later one is a hipGetDevice and a table read.  0 or the hipError_t; a failed family is tried again by the next call.
int kernels_ready(unsigned family_mask);

// multiProcessorCount of the current device (queried once per device; 256 when the query fails): the persistent kernels' grids
int device_cus();

// for the configure functions: max dynamic LDS bytes per kernel; the first error, or 0
int set_max_lds(std::initializer_list<std::pair<const void*, int>> kernels);

}  // namespace dmad
