// probes.cpp -- TEST INFRASTRUCTURE ONLY: device helpers of the kernel sources made callable from the tests through the CPU build.
#define HY_HELPERS_ONLY
#define FLT_DECLARE_ONLY
#include "../../hyena_dna_amd/csrc/filter_kernels.h"

extern "C" void hipemu_probe_sincos(const float* x, float* sn, float* cs, long n) {
    for (long i = 0; i < n; ++i) hyena::hy_sincos(x[i], sn + i, cs + i);
}
