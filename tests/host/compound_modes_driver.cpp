// The compounding modes through the C++ shim (tests/test_gpu_compound_modes.py builds and runs it): rf_image::postprocess(steer_rad, opts)
// and postprocess(bmode_params, steer_rad, tgc, opts) with an mcrt_compound_opts on a scene file.  Writes the float picture [400][500]
// float32 and the 8-bit picture [400][500].
//     compound_modes_driver <scene.json> <out.bin> <frame> <samples> <steer,steer,...> <mean|max|median> <feather_lines> <w,w,...>
#include "mcrt_host.hpp"
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 64;
using image = rf_image<E, 100, 322>;       // 465 rows, 0.322 mm apart
using psf_ = psf<7, 13, 7, 145>;

static std::vector<float> list_of(const char *q)
{
    std::vector<float> v;
    while (*q) { v.push_back((float)std::atof(q)); while (*q && *q != ',') q++; if (*q == ',') q++; }
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 9) { std::cerr << "usage: compound_modes_driver scene.json out.bin frame samples steer,... mode feather weight,..." << std::endl; return 2; }
    try {
        const std::vector<float> steers = list_of(argv[5]), weights = list_of(argv[8]);
        mcrt_compound_opts o; check(mcrt_default_compound_opts(&o), "mcrt_default_compound_opts");
        o.mode = !std::strcmp(argv[6], "max") ? MCRT_COMPOUND_MAX : !std::strcmp(argv[6], "median") ? MCRT_COMPOUND_MEDIAN : MCRT_COMPOUND_MEAN;
        o.feather_lines = (float)std::atof(argv[7]);
        for (size_t n = 0; n < weights.size() && n < 16; n++) o.view_weight[n] = weights[n];
        const json cfg = load_json(argv[1]);
        const uint32_t frame = (uint32_t)std::atol(argv[3]);
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
        mcrt_bmode_params bp; check(mcrt_default_bmode(&bp), "mcrt_default_bmode");
        img.trace(frame, tr, steers);
        img.convolve(p);
        img.envelope();
        img.postprocess(steers, &o);
        img.postprocess(bp, steers, nullptr, &o);
        check(dev->synchronize(), "mcrt_synchronize");
        const std::vector<float> picture = img.scan_converted();
        const std::vector<unsigned char> bytes = img.bmode();
        std::ofstream f(argv[2], std::ios::binary);
        f.write((const char *)picture.data(), (std::streamsize)(picture.size() * sizeof(float)));
        f.write((const char *)bytes.data(), (std::streamsize)bytes.size());
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
