// Stand-alone host program for tests/test_kenansville_cpu.py: the plan and the twiddle builder of csrc/wave_fft.h, which is free of HIP
// below its plan section.
//   wave_fft_plan_main plan L...      one line per length: "L ok M lds_bytes r0 r1 ..." or "L refused <rule>"
//   wave_fft_plan_main twiddles L     2 L fp32 values (cos, sin of -2 pi j / L) as raw bytes on stdout
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "wave_fft.h"

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "plan")) {
        for (int i = 2; i < argc; ++i) {
            const int L = atoi(argv[i]);
            dmad::FftPlan p;
            if (const char* why = dmad::wave_fft_plan(L, &p)) {
                printf("%d refused %s\n", L, why);
                continue;
            }
            printf("%d ok %d %d", L, p.M, p.lds_bytes);
            for (int s = 0; s < p.nstages; ++s) printf(" %d", p.radix[s]);
            printf("\n");
        }
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "twiddles")) {
        const int L = atoi(argv[2]);
        if (L < 1) return 2;
        std::vector<float> tw(2 * (size_t)L);
        dmad::wave_fft_twiddles(L, tw.data());
        return fwrite(tw.data(), sizeof(float), tw.size(), stdout) == tw.size() ? 0 : 3;
    }
    fprintf(stderr, "usage: %s plan L... | twiddles L\n", argv[0]);
    return 2;
}
