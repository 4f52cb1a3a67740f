// Prints what the wavefront sweeps' launch helper (launch.hpp: sweep_waves, sweep_grid) decides from sizes alone, at the real LDS
// sizes of a few instantiations (tests/test_sweep_launch_rules.py).  Host only.
//   lds <name> <bytes per wavefront>
//   waves <name> <12-wavefront tier> <DPILQR_MFMA_WAVES> <grid_items> <wavefronts per workgroup>
//   grid <grid_items> <CUs> <wavefronts per workgroup> <workgroups>
#include <cstdio>
#include "launch.hpp"
#include "riccati_mfma.hpp"
using namespace dpilqr;
int main() {
    struct Site { const char* name; size_t lds; } sites[] = {
        {"record_20_10", sizeof(double) * MfmaCfg<20, 10>::total},
        {"record_24_12", sizeof(double) * MfmaCfg<24, 12>::total},
        {"fused_20_10", sizeof(double) * MfmaCfg<20, 10, true>::total},
        {"general_20_10", sizeof(double) * MfmaCfg<20, 10, 2>::total},
        {"inprod6_20_10", sizeof(double) * (MfmaCfg<20, 10>::total + InprodCfg<20, 10, 6>::total)},
        {"inprod6_24_12", sizeof(double) * (MfmaCfg<24, 12>::total + InprodCfg<24, 12, 6>::total)},
        {"bike_16_8", sizeof(double) * (MfmaCfg<16, 8>::total + InprodCfg<16, 8, 5>::total)},
        {"bike_20_10", sizeof(double) * (MfmaCfg<20, 10>::total + InprodCfg<20, 10, 5>::total)},
    };
    const int items[] = {1, 256, 257, 1024, 1025, 2048, 2049, 6144};
    for (auto& s : sites) {
        std::printf("lds %s %zu\n", s.name, s.lds);
        for (int tier12 = 0; tier12 < 2; ++tier12)
            for (int max_wv : {4, 8, 12})
                for (int g : items) std::printf("waves %s %d %d %d %d\n", s.name, tier12, max_wv, g, sweep_waves(g, max_wv, s.lds, tier12 != 0));
    }
    for (int wv : {4, 8, 12})
        for (int g : items) std::printf("grid %d 256 %d %d\n", g, wv, sweep_grid(g, 256, wv));
    return 0;
}
