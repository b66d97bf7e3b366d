// Spatial compounding through the C++ shim (tests/test_gpu_compound.py builds and runs it): transducer<N>::steered, rf_image::trace(frame,
// transducer, steer_rad) -- the views as one pose pass --, convolve and envelope over the views, postprocess(steer_rad) and
// postprocess(bmode_params, steer_rad) on a scene file.  Writes the steered tables (pos, dir: [views][64][3] float32 each), the float
// picture [400][500] float32 and the 8-bit picture [400][500].
//     compound_driver <scene.json> <out.bin> <frame> <samples> <steer_rad,steer_rad,...> [--devices 0,0]
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
    if (argc < 6) { std::cerr << "usage: compound_driver scene.json out.bin frame samples steer,steer,... [--devices a,b]" << std::endl; return 2; }
    try {
        std::vector<int> devices{ 0 };
        if (argc > 7 && !std::strcmp(argv[6], "--devices")) {
            devices.clear();
            for (const char *q = argv[7]; *q;) { devices.push_back(std::atoi(q)); while (*q && *q != ',') q++; if (*q == ',') q++; }
        }
        std::vector<float> steers;
        for (const char *q = argv[5]; *q;) { steers.push_back((float)std::atof(q)); while (*q && *q != ',') q++; if (*q == ',') q++; }
        const json cfg = load_json(argv[1]);
        const uint32_t frame = (uint32_t)std::atol(argv[3]);
        const psf_ p{ 4.5f, 0.05f, 0.2f, 0.1f };
        const auto &t_pos = cfg.at("transducerPosition");
        const auto &t_dir = cfg.at("transducerAngles");
        const double amplitude = 60.0 * 3.14159265358979323846264338327950288419716939937510 / 180.0;
        const double separation_mm = (((double)(float)amplitude * 3.0) / (double)E) * 10.0;
        transducer<E> tr(4.5f, 3.0, separation_mm, vec3((float)t_pos[0], (float)t_pos[1], (float)t_pos[2]),
                         std::array<float, 3>{ (float)t_dir[0], (float)t_dir[1], (float)t_dir[2] });
        const auto tables = tr.steered(steers);
        auto dev = std::make_shared<device>(devices);
        scene sc{ cfg, tr, dev, (unsigned)std::atoi(argv[4]) };
        image img{ dev, 30.0, amplitude };
        mcrt_bmode_params bp; check(mcrt_default_bmode(&bp), "mcrt_default_bmode");
        img.trace(frame, tr, steers);
        img.convolve(p);
        img.envelope();
        img.postprocess(steers);
        img.postprocess(bp, steers);
        check(dev->synchronize(), "mcrt_synchronize");
        const std::vector<float> picture = img.scan_converted();
        const std::vector<unsigned char> bytes = img.bmode();
        std::ofstream f(argv[2], std::ios::binary);
        f.write((const char *)tables.pos.data(), (std::streamsize)(tables.pos.size() * sizeof(float)));
        f.write((const char *)tables.dir.data(), (std::streamsize)(tables.dir.size() * sizeof(float)));
        f.write((const char *)picture.data(), (std::streamsize)(picture.size() * sizeof(float)));
        f.write((const char *)bytes.data(), (std::streamsize)bytes.size());
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
