// mcrt_transmit_boundary and mcrt_default_transmit_opts -- host code of csrc/mcrt_host.cpp -- as a stand-alone program under AddressSanitizer +
// UBSan (tests/test_transmit_contract.py compiles this file with csrc/mcrt_host.cpp and compares the printed bits with the numpy mirror's).
// Reads "z_before z_after inc intensity" as four hexadecimal float words per line from the file given, prints "i_refl i_refr" the same way.
#include "mcrt.h"
#include <cstdint>
#include <cstdio>
#include <cstring>

static float word(uint32_t w) { float f; std::memcpy(&f, &w, 4); return f; }
static uint32_t bits(float f) { uint32_t w; std::memcpy(&w, &f, 4); return w; }

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    mcrt_transmit_opts o;
    if (mcrt_default_transmit_opts(&o) != MCRT_OK || o.mode != MCRT_TRANSMIT_TOTAL || o.rule != MCRT_LABEL_TRACED || o.start_offset != -1.0f) return 3;
    if (mcrt_default_transmit_opts(nullptr) != MCRT_ERR_INVALID || !std::strstr(mcrt_last_error(), "null options")) return 3;
    float a = 0.0f, b = 0.0f;
    if (mcrt_transmit_boundary(1.0f, 2.0f, 1.0f, 1.0f, nullptr, &b) != MCRT_ERR_INVALID || mcrt_transmit_boundary(1.0f, 2.0f, 1.0f, 1.0f, &a, nullptr) != MCRT_ERR_INVALID) return 3;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 4;
    unsigned z1, z2, inc, ia;
    while (std::fscanf(f, "%x %x %x %x", &z1, &z2, &inc, &ia) == 4) {
        if (mcrt_transmit_boundary(word(z1), word(z2), word(inc), word(ia), &a, &b) != MCRT_OK) return 5;
        std::printf("%08x %08x\n", bits(a), bits(b));
    }
    std::fclose(f);
    std::puts("DONE");
    return 0;
}
