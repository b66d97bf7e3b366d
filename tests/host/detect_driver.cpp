// Quadrature detection through the C++ shim (tests/test_gpu_detect.py builds and runs it): rf_image::iq and rf_image::detect on an image
// deposited on the host with rf_image::add_echo.  Writes, as float32: the image before [465][64]; after convolve its analytic pair
// [64][465][2] (rf_image::iq); after convolve + detect [465][64]; and, with bands, after convolve(p with bands) + detect [465][64].
//     detect_driver <out.bin> <n_taps> [band_mhz ...]
#include "mcrt_host.hpp"
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iostream>

using namespace mcrt_host;

constexpr unsigned int E = 64;
using image = rf_image<E, 100, 322>;       // 465 rows, 0.322 mm apart
using psf_ = psf<7, 13, 7, 145>;

static void deposit(image &img)
{
    img.clear();
    for (unsigned int c = 0; c < E; c++)
        for (unsigned int j = 0; j < 40; j++)
            img.add_echo(c, std::sin(0.37f * (float)c + 1.1f * (float)j), 0.5 + (double)((c * 7u + j * 13u) % 99u));
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::cerr << "usage: detect_driver out.bin n_taps [band_mhz ...]" << std::endl; return 2; }
    try {
        mcrt_detect_opts o; mcrt_default_detect_opts(&o);
        o.n_taps = (uint32_t)std::atoi(argv[2]);
        const psf_ plain{ 4.5f, 0.05f, 0.2f, 0.1f };
        image img(30.0, 1.0471975511965976);
        std::ofstream f(argv[1], std::ios::binary);
        auto put = [&](const std::vector<float> &v) { f.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(float))); };
        deposit(img);
        put(img.intensities());
        img.convolve(plain);
        std::vector<float> pair;
        img.iq(o, pair);
        put(pair);
        img.detect(o);
        put(img.intensities());
        if (argc > 3) {
            psf_ p{ 4.5f, 0.05f, 0.2f, 0.1f };
            mcrt_bands b; mcrt_default_bands(&b, 4.5f, 0.05f);
            b.n_bands = (uint32_t)(argc - 3);
            for (int i = 3; i < argc && i < 11; i++) { b.band_mhz[i - 3] = (float)std::atof(argv[i]); b.band_weight[i - 3] = (float)(i - 2); }
            p.set_bands(b);
            deposit(img);
            img.convolve(p); img.detect(o);
            put(img.intensities());
        }
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
