// Automatic gain through the C++ shim (tests/test_gpu_autogain_host.py builds and runs it): rf_image::autogain over one traced frame with a
// noise floor of a given sigma, and over the three views of a compounded frame.  Writes float32 blocks: the plain frame before the gain
// [465][64] and after it, its row gains [465] and its penetration depth [1] (rows, as a float); then the compounded frame's three views
// before the gain, its middle view after it, the row gains and the penetration depth (the three views share one curve).
//     autogain_driver <scene.json> <out.bin> <frame> <samples> <sigma> <band_rows>
#include "mcrt_host.hpp"
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 64;
using image = rf_image<E, 100, 322>;       // 465 rows, 0.322 mm apart
using psf_ = psf<7, 13, 7, 145>;

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b)      // (a NaN equals itself)
{
    return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(float));
}

int main(int argc, char **argv)
{
    if (argc < 7) { std::cerr << "usage" << std::endl; return 2; }
    try {
        const json cfg = load_json(argv[1]);
        const uint32_t frame = (uint32_t)std::atol(argv[3]);
        mcrt_noise_opts noise;
        check(mcrt_default_noise_opts(&noise), "mcrt_default_noise_opts");
        noise.mode = MCRT_NOISE_ABS; noise.sigma = (float)std::atof(argv[5]);
        mcrt_autogain_opts gain;
        check(mcrt_default_autogain_opts(&gain), "mcrt_default_autogain_opts");
        if (gain.band_rows != 16u || gain.min_permille != 250u || gain.floor_scale != 3.0f || gain.max_gain != 1000.0f || gain.apply != 1u)
            throw std::runtime_error("the defaults are not the header's");
        gain.band_rows = (uint32_t)std::atoi(argv[6]);
        const psf_ p{ 4.5f, 0.05f, 0.2f, 0.1f };
        const auto &t_pos = cfg.at("transducerPosition");
        const auto &t_dir = cfg.at("transducerAngles");
        const double amplitude = 60.0 * 3.14159265358979323846264338327950288419716939937510 / 180.0;
        const double separation_mm = (((double)(float)amplitude * 3.0) / (double)E) * 10.0;
        transducer<E> tr(4.5f, 3.0, separation_mm, vec3((float)t_pos[0], (float)t_pos[1], (float)t_pos[2]),
                         std::array<float, 3>{ (float)t_dir[0], (float)t_dir[1], (float)t_dir[2] });
        auto dev = std::make_shared<device>(std::vector<int>{ 0 });
        scene sc{ cfg, tr, dev, (unsigned)std::atoi(argv[4]) };
        image img{ dev, 30.0, amplitude };
        std::ofstream f(argv[2], std::ios::binary);
        auto put = [&](const std::vector<float> &v) { f.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(float))); };

        img.trace(frame);
        img.convolve(p);
        bool threw = false;
        try { img.autogain(gain, true); } catch (const std::logic_error &) { threw = true; }      // no add_noise() on this pass yet
        if (!threw) throw std::runtime_error("autogain(noise_floor) without add_noise() did not throw");
        img.add_noise(noise);
        img.envelope();
        put(img.intensities());
        img.autogain(gain, true);
        put(img.intensities());
        if (img.gain_curve().size() != image::max_rows || img.penetration_rows().size() != 1u) throw std::runtime_error("the by-products' sizes");
        if (img.penetration_mm() != (double)img.penetration_rows()[0] * 0.322) throw std::runtime_error("penetration_mm is not rows x 0.322");
        put(img.gain_curve());
        put({ (float)img.penetration_rows()[0] });
        std::cout << "penetration " << img.penetration_mm() << " mm" << std::endl;

        const std::vector<float> steers{ -0.1f, 0.0f, 0.1f };
        img.trace(frame, tr, steers);
        img.convolve(p);
        img.add_noise(noise);
        img.envelope();
        const std::vector<float> v0 = img.view_intensities(0), before = img.view_intensities(1), v2 = img.view_intensities(2);
        gain.apply = 0;                                            // estimate only: the views keep their bits
        img.autogain(gain, true);
        if (!same_bits(img.view_intensities(1), before)) throw std::runtime_error("apply == 0 changed the views");
        const std::vector<float> k0 = img.gain_curve();
        gain.apply = 1;
        img.autogain(gain, true);
        if (!same_bits(img.gain_curve(), k0)) throw std::runtime_error("apply changed the curve");
        put(v0); put(before); put(v2);
        put(img.view_intensities(1));
        put(img.gain_curve());
        put({ (float)img.penetration_rows()[0] });
        check(dev->synchronize(), "mcrt_synchronize");
        if (!f) throw std::runtime_error("cannot write the output");
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
