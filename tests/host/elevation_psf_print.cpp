// Slice thickness through the C++ shim, host side only (tests/test_elevation_contract.py builds and runs it; no GPU is touched):
// prints the bit patterns of psf<7,13,7,145>::elevation_kernel and of elevation_rows(n_rows, row_mm), one hex word per weight.
//     elevation_psf_print <var_z> <pitch_um or 0: leave the default> <normalize 0|1> <n_rows> <row_mm> <focal_range_mm> [focus_mm ...]
#include "mcrt_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace mcrt_host;
using psf_ = psf<7, 13, 7, 145>;

static void print_bits(const float *v, size_t n)
{
    for (size_t i = 0; i < n; i++) { uint32_t u; std::memcpy(&u, &v[i], 4); std::printf("%08x\n", (unsigned)u); }
}

int main(int argc, char **argv)
{
    if (argc < 7) { std::fprintf(stderr, "usage: elevation_psf_print var_z pitch_um normalize n_rows row_mm focal_range_mm [focus_mm ...]\n"); return 2; }
    try {
        psf_ p{ 4.5f, 0.05f, 0.2f, (float)std::atof(argv[1]) };
        const uint32_t pitch = (uint32_t)std::atol(argv[2]);
        std::vector<float> foci;
        for (int i = 7; i < argc; i++) foci.push_back((float)std::atof(argv[i]));
        if (pitch) p.set_elevation(pitch, std::atoi(argv[3]) != 0, foci.data(), (uint32_t)foci.size(), (float)std::atof(argv[6]));
        print_bits(p.elevation_kernel.data(), p.elevation_kernel.size());
        const std::vector<float> &rows = p.elevation_rows((uint32_t)std::atol(argv[4]), std::atof(argv[5]));
        print_bits(rows.data(), rows.size());
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
