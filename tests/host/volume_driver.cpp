// Volume imaging through the C++ shim (tests/test_gpu_volume.py builds and runs it): transducer<N>::swept, rf_image::trace(frame, transducer,
// sweep), convolve / envelope over the planes and rf_image::volume in both forms on a scene file.  Writes the swept tables pos and dir
// [K][E][3] float32, the float cut [nv][nu] float32 and the 8-bit cut [nv][nu].
//     volume_driver <scene.json> <out.bin> <frame> <samples> <planes> <step_rad> <pivot_mm> <cplane depth_mm> <nu> <nv> <pitch_mm>
#include "mcrt_host.hpp"
#include <cstdlib>
#include <fstream>
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 64;
using image = rf_image<E, 100, 322>;       // 465 rows, 0.322 mm apart
using psf_ = psf<7, 13, 7, 145>;

int main(int argc, char **argv)
{
    if (argc < 12) { std::cerr << "usage: volume_driver scene.json out.bin frame samples planes step_rad pivot_mm depth_mm nu nv pitch_mm" << std::endl; return 2; }
    try {
        const json cfg = load_json(argv[1]);
        const uint32_t frame = (uint32_t)std::atol(argv[3]);
        const mcrt_sweep sw{ (uint32_t)std::atoi(argv[5]), (float)std::atof(argv[6]), (float)std::atof(argv[7]) };
        const uint32_t nu = (uint32_t)std::atoi(argv[9]), nv = (uint32_t)std::atoi(argv[10]);
        const double depth = std::atof(argv[8]), pitch = std::atof(argv[11]);
        mcrt_volume_grid g{};               // the C-plane at y = depth: u along x, v along z, centred on the arc's axis
        g.origin_mm[0] = -(double)(nu - 1) * pitch / 2.0; g.origin_mm[1] = depth; g.origin_mm[2] = -(double)(nv - 1) * pitch / 2.0;
        g.du_mm[0] = pitch; g.dv_mm[2] = pitch; g.nu = nu; g.nv = nv; g.nw = 1;
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
        const auto tables = tr.swept(sw);
        img.trace(frame, tr, sw);
        img.convolve(p);
        img.envelope();
        const std::vector<float> cut = img.volume(g);
        const std::vector<unsigned char> bytes = img.volume(bp, g);
        check(dev->synchronize(), "mcrt_synchronize");
        std::ofstream f(argv[2], std::ios::binary);
        f.write((const char *)tables.pos.data(), (std::streamsize)(tables.pos.size() * sizeof(float)));
        f.write((const char *)tables.dir.data(), (std::streamsize)(tables.dir.size() * sizeof(float)));
        f.write((const char *)cut.data(), (std::streamsize)(cut.size() * sizeof(float)));
        f.write((const char *)bytes.data(), (std::streamsize)bytes.size());
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
