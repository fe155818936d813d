// Per-device kernel set-up (kernel_setup.h): the table of the families' configure functions, the device id for SetupTable, the CU counts.
#include "kernel_setup.h"

#include <atomic>

#include "kernel_setup_table.h"

namespace dmad {

// each next to the kernels it names; called from here only
int gemm_f32_configure();
int gemm_x3_configure();
int gemm_h16_configure();
int wn_layer_p_configure();
int wn_final_p_configure();
int m5_configure();
int kws_configure();
int unvjp_configure();
int unet_att_configure();
int wave_iir_configure();
int wave_fft_configure();

namespace {
// both in the order of the KF_ bits
const SetupTable::ConfigureFn kConfigure[KF_COUNT] = {gemm_f32_configure,   gemm_x3_configure, gemm_h16_configure, wn_layer_p_configure,
                                                      wn_final_p_configure, m5_configure,      kws_configure,      unvjp_configure,
                                                      unet_att_configure,   wave_iir_configure, wave_fft_configure};
const char* const kNames[KF_COUNT] = {"fp32 narrow tile", "split-f16 tier", "f16 conv GEMM",      "WaveNet layer", "WaveNet tail",
                                      "M5",               "KWS",            "attention backward", "attention",     "IIR filter",
                                      "wave FFT"};

SetupTable& table() {
    static SetupTable t(kConfigure, KF_COUNT);
    return t;
}
}  // namespace

const char* kernel_family_name(unsigned family) {
    for (int f = 0; f < (int)KF_COUNT; ++f)
        if (family == 1u << f) return kNames[f];
    return "?";
}

int kernels_ready(unsigned family_mask) {
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return (int)e;
    if (!table().holds(dev)) return (int)hipErrorInvalidDevice;
    return table().ready(dev, family_mask);
}

int device_cus() {
    static std::atomic<int> cus[SetupTable::kMaxDevices] = {};       // 0: not asked yet
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= SetupTable::kMaxDevices) return 256;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (!n) {
        hipDeviceProp_t prop;
        n = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

int set_max_lds(std::initializer_list<std::pair<const void*, int>> kernels) {
    for (const auto& k : kernels)
        if (hipError_t e = hipFuncSetAttribute(k.first, hipFuncAttributeMaxDynamicSharedMemorySize, k.second)) return (int)e;
    return 0;
}

}  // namespace dmad
