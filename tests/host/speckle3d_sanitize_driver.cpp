// mcrt_default_speckle3d_opts, mcrt_speckle3d_weights and mcrt_speckle3d_tables -- host code of csrc/mcrt_host.cpp -- as a stand-alone program
// under AddressSanitizer + UBSan (tests/test_speckle3d_contract.py compiles this file with csrc/mcrt_host.cpp and compares the printed bits with
// the shipped library's).  Exact-size heap buffers, so that a write past a table shows.  Reads "n_iter q0 rho lambda wu wv ww" per line from
// the file given (the floats as hexadecimal words) and prints the return code, then on success q0sq[n_iter], kq[n_iter] and k[4] as words;
// then a few grids' weights and every refusal.
#include "mcrt.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static float word(uint32_t w) { float f; std::memcpy(&f, &w, 4); return f; }
static uint32_t bits(float f) { uint32_t w; std::memcpy(&w, &f, 4); return w; }

static mcrt_volume_grid grid(double hu, double hv, double hw, uint32_t nu, uint32_t nv, uint32_t nw)
{
    mcrt_volume_grid g{};
    g.du_mm[0] = hu; g.dv_mm[1] = hv; g.dw_mm[2] = hw; g.nu = nu; g.nv = nv; g.nw = nw;
    return g;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    mcrt_speckle3d_opts d;
    std::memset(&d, 0xA5, sizeof d);
    if (sizeof d != 28 || mcrt_default_speckle3d_opts(&d) != MCRT_OK || d.n_iter != 20u || d.q0 != 0.5227232f || d.lambda != 0.5f || d.weight[0] != 1.0f || d.weight[1] != 1.0f || d.weight[2] != 1.0f) return 3;
    if (mcrt_default_speckle3d_opts(nullptr) != MCRT_ERR_INVALID || !std::strstr(mcrt_last_error(), "null options")) return 3;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 4;
    unsigned n, w[6];
    while (std::fscanf(f, "%u %x %x %x %x %x %x", &n, &w[0], &w[1], &w[2], &w[3], &w[4], &w[5]) == 7) {
        mcrt_speckle3d_opts o;
        o.n_iter = n; o.q0 = word(w[0]); o.rho = word(w[1]); o.lambda = word(w[2]);
        for (int i = 0; i < 3; i++) o.weight[i] = word(w[3 + i]);
        const size_t len = n <= 256u ? n : 0u;
        std::vector<float> q0sq(len, 7.0f), kq(len, 7.0f), k(4, 7.0f);
        const int rc = mcrt_speckle3d_tables(&o, len ? q0sq.data() : nullptr, len ? kq.data() : nullptr, k.data());
        std::printf("%d", rc);
        if (rc == MCRT_OK) {
            for (float v : q0sq) std::printf(" %08x", bits(v));
            for (float v : kq) std::printf(" %08x", bits(v));
        } else if (n > 256u) {
            if (rc != MCRT_ERR_LIMIT) return 5;
        } else {
            for (float v : q0sq) if (v != 7.0f) return 5;               // an error writes nothing
            for (float v : kq) if (v != 7.0f) return 5;
        }
        for (float v : k) std::printf(" %08x", bits(v));
        std::printf("\n");
    }
    std::fclose(f);
    if (mcrt_speckle3d_tables(nullptr, nullptr, nullptr, nullptr) != MCRT_ERR_INVALID || mcrt_speckle3d_tables(&d, nullptr, nullptr, nullptr) != MCRT_ERR_INVALID) return 6;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const mcrt_volume_grid grids[] = { grid(0.5, 0.5, 1.0, 4, 5, 6), grid(0.5, 0.5, 1.0, 4, 5, 1), grid(0.125, 2.0, 1.0, 1, 5, 6), grid(1.0, 1.0, 7.0, 1, 1, 6),
                                       grid(0.3, 0.7, 1.1, 2, 2, 2), grid(0.0, 0.5, 1.0, 4, 5, 6), grid(0.5, 0.5, 1.0, 1, 1, 1), grid(0.5, nan, 1.0, 4, 5, 6),
                                       grid(0.5, 0.5, 1.0, 0, 5, 6), grid(1e-200, 1.0, 1e200, 2, 2, 2) };
    for (const mcrt_volume_grid &g : grids) {
        std::vector<float> w3(3, 7.0f);
        const int rc = mcrt_speckle3d_weights(&g, w3.data());
        std::printf("W %d %08x %08x %08x\n", rc, bits(w3[0]), bits(w3[1]), bits(w3[2]));
    }
    float w3[3];
    if (mcrt_speckle3d_weights(nullptr, w3) != MCRT_ERR_INVALID || mcrt_speckle3d_weights(&grids[0], nullptr) != MCRT_ERR_INVALID) return 7;
    std::puts("DONE");
    return 0;
}
