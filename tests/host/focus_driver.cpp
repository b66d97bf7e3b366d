// Focal zones through the C++ shim (tests/test_gpu_focus.py builds and runs it): psf::set_focus + rf_image::convolve on an image
// deposited on the host with rf_image::add_echo.  Writes the image before and after the convolution, each row-major [465][64] float32.
//     focus_driver <out.bin> <focal_range_mm> [focus_mm ...]        (no foci: the reference's constant kernel)
#include "mcrt_host.hpp"
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iostream>

using namespace mcrt_host;

constexpr unsigned int E = 64;
using image = rf_image<E, 100, 322>;       // 465 rows, 0.322 mm apart
using psf_ = psf<7, 13, 7, 145>;

int main(int argc, char **argv)
{
    if (argc < 3) { std::cerr << "usage: focus_driver out.bin focal_range_mm [focus_mm ...]" << std::endl; return 2; }
    try {
        psf_ p{ 4.5f, 0.05f, 0.2f, 0.1f };
        std::vector<float> foci;
        for (int i = 3; i < argc; i++) foci.push_back((float)std::atof(argv[i]));
        if (!foci.empty()) p.set_focus(foci.data(), (uint32_t)foci.size(), (float)std::atof(argv[2]));
        image img(30.0, 1.0471975511965976);
        img.clear();
        for (unsigned int c = 0; c < E; c++)
            for (unsigned int j = 0; j < 40; j++)
                img.add_echo(c, std::sin(0.37f * (float)c + 1.1f * (float)j), 0.5 + (double)((c * 7u + j * 13u) % 99u));
        const std::vector<float> before = img.intensities();
        img.convolve(p);
        const std::vector<float> after = img.intensities();
        std::ofstream f(argv[1], std::ios::binary);
        f.write((const char *)before.data(), (std::streamsize)(before.size() * sizeof(float)));
        f.write((const char *)after.data(), (std::streamsize)(after.size() * sizeof(float)));
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
