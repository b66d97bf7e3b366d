// Frequency compounding through the C++ shim (tests/test_gpu_bands.py builds and runs it): psf::set_bands + rf_image::convolve / add_noise /
// envelope / fold_bands on an image deposited on the host with rf_image::add_echo.  Writes four images, each row-major [465][64] float32: the
// image before, after convolve + envelope (the compounded frame), after convolve + fold_bands (the coherent sum), and after convolve +
// add_noise (30 dB, seed 77) + envelope.
//     bands_driver <out.bin> <downshift_mhz_per_mm> <min_mhz> <var_x> [band_mhz ...]        (no bands: the reference's constant kernel)
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
    if (argc < 5) { std::cerr << "usage: bands_driver out.bin downshift_mhz_per_mm min_mhz var_x [band_mhz ...]" << std::endl; return 2; }
    try {
        psf_ p{ 4.5f, 0.05f, 0.2f, 0.1f };
        if (argc > 5) {
            mcrt_bands b; mcrt_default_bands(&b, 4.5f, (float)std::atof(argv[4]));
            b.n_bands = (uint32_t)(argc - 5);
            for (int i = 5; i < argc && i < 13; i++) { b.band_mhz[i - 5] = (float)std::atof(argv[i]); b.band_weight[i - 5] = (float)(i - 4); }
            b.downshift_mhz_per_mm = (float)std::atof(argv[2]); b.min_mhz = (float)std::atof(argv[3]);
            p.set_bands(b);
        }
        mcrt_noise_opts noise; mcrt_default_noise_opts(&noise);
        noise.mode = MCRT_NOISE_SNR_DB; noise.snr_db = 30.0f; noise.seed = 77u;
        image img(30.0, 1.0471975511965976);
        std::ofstream f(argv[1], std::ios::binary);
        auto put = [&](const std::vector<float> &v) { f.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(float))); };
        deposit(img);
        put(img.intensities());
        img.convolve(p); img.envelope();
        put(img.intensities());
        deposit(img);
        img.convolve(p); img.fold_bands();
        put(img.intensities());
        deposit(img);
        img.convolve(p); img.add_noise(noise); img.envelope();
        put(img.intensities());
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
