// Slice thickness through the C++ shim (tests/test_gpu_elevation.py builds and runs it): rf_image::trace(frame) -- the thin sheet -- and
// rf_image::trace(frame, transducer, psf) -- K elevation planes as one pose pass, folded -- on a scene file.  Writes both images, each
// row-major [465][64] float32, before any convolution.
//     elevation_driver <scene.json> <out.bin> <frame> <samples> <var_z> <pitch_um> <n_planes or 0: the psf's 7> [--devices 0,0]
#include "mcrt_host.hpp"
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 64;
using image = rf_image<E, 100, 322>;       // 465 rows, 0.322 mm apart
using psf_ = psf<7, 13, 7, 145>;

int main(int argc, char **argv)
{
    if (argc < 8) { std::cerr << "usage: elevation_driver scene.json out.bin frame samples var_z pitch_um n_planes [--devices a,b]" << std::endl; return 2; }
    try {
        std::vector<int> devices{ 0 };
        if (argc > 9 && !std::strcmp(argv[8], "--devices")) {
            devices.clear();
            for (const char *q = argv[9]; *q;) { devices.push_back(std::atoi(q)); while (*q && *q != ',') q++; if (*q == ',') q++; }
        }
        const json cfg = load_json(argv[1]);
        const uint32_t frame = (uint32_t)std::atol(argv[3]);
        psf_ p{ 4.5f, 0.05f, 0.2f, (float)std::atof(argv[5]) };
        p.set_elevation((uint32_t)std::atol(argv[6]));
        const auto &t_pos = cfg.at("transducerPosition");
        const auto &t_dir = cfg.at("transducerAngles");
        const double amplitude = 60.0 * 3.14159265358979323846264338327950288419716939937510 / 180.0;
        const double separation_mm = (((double)(float)amplitude * 3.0) / (double)E) * 10.0;
        transducer<E> tr(4.5f, 3.0, separation_mm, vec3((float)t_pos[0], (float)t_pos[1], (float)t_pos[2]),
                         std::array<float, 3>{ (float)t_dir[0], (float)t_dir[1], (float)t_dir[2] });
        auto dev = std::make_shared<device>(devices);
        scene sc{ cfg, tr, dev, (unsigned)std::atoi(argv[4]) };
        image img{ dev, 30.0, amplitude };
        img.trace(frame);
        const std::vector<float> before = img.intensities();
        img.trace(frame, tr, p, (uint32_t)std::atol(argv[7]));
        const std::vector<float> after = img.intensities();
        check(dev->synchronize(), "mcrt_synchronize");
        std::ofstream f(argv[2], std::ios::binary);
        f.write((const char *)before.data(), (std::streamsize)(before.size() * sizeof(float)));
        f.write((const char *)after.data(), (std::streamsize)(after.size() * sizeof(float)));
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
