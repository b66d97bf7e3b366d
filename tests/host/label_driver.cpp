// Ground-truth label maps through the C++ shim (tests/test_gpu_label.py builds and runs it): rf_image::labels, label_picture and, after a
// swept trace, label_volume on a scene file -- on one context, or on a group whose ranks share the GPU.  Writes the tissue map
// [planes][E][R] uint8, the interface map [planes][E][R] int32, the crossings [planes][E] uint32 and the picture: [400][500] uint8, or with
// a sweep the C-plane [nv][nu] uint8.
//     label_driver <scene.json> <out.bin> <devices 0 | 0,0> <rule 0|1> <offset> [<planes> <step_rad> <pivot_mm> <cplane depth_mm> <nu> <nv> <pitch_mm>]
#include "mcrt_host.hpp"
#include <cstdlib>
#include <fstream>
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 64;
using image = rf_image<E, 100, 322>;       // 465 rows, 0.322 mm apart

int main(int argc, char **argv)
{
    if (argc != 6 && argc != 13) { std::cerr << "usage: label_driver scene.json out.bin devices rule offset [planes step_rad pivot_mm depth_mm nu nv pitch_mm]" << std::endl; return 2; }
    try {
        const json cfg = load_json(argv[1]);
        std::vector<int> devices;
        for (const char *q = argv[3]; *q;) { devices.push_back(std::atoi(q)); while (*q && *q != ',') q++; if (*q == ',') q++; }
        mcrt_label_opts lo; check(mcrt_default_label_opts(&lo), "mcrt_default_label_opts");
        lo.rule = (uint32_t)std::atoi(argv[4]); lo.start_offset = (float)std::atof(argv[5]);
        const auto &t_pos = cfg.at("transducerPosition");
        const auto &t_dir = cfg.at("transducerAngles");
        const double amplitude = 60.0 * 3.14159265358979323846264338327950288419716939937510 / 180.0;
        const double separation_mm = (((double)(float)amplitude * 3.0) / (double)E) * 10.0;
        transducer<E> tr(4.5f, 3.0, separation_mm, vec3((float)t_pos[0], (float)t_pos[1], (float)t_pos[2]),
                         std::array<float, 3>{ (float)t_dir[0], (float)t_dir[1], (float)t_dir[2] });
        auto dev = std::make_shared<device>(devices);
        scene sc{ cfg, tr, dev, 4u };
        image img{ dev, 30.0, amplitude };
        std::vector<unsigned char> picture;
        image::label_maps m;
        if (argc == 13) {
            const mcrt_sweep sw{ (uint32_t)std::atoi(argv[6]), (float)std::atof(argv[7]), (float)std::atof(argv[8]) };
            const uint32_t nu = (uint32_t)std::atoi(argv[10]), nv = (uint32_t)std::atoi(argv[11]);
            const double depth = std::atof(argv[9]), pitch = std::atof(argv[12]);
            mcrt_volume_grid g{};               // the C-plane at y = depth: u along x, v along z, centred on the arc's axis
            g.origin_mm[0] = -(double)(nu - 1) * pitch / 2.0; g.origin_mm[1] = depth; g.origin_mm[2] = -(double)(nv - 1) * pitch / 2.0;
            g.du_mm[0] = pitch; g.dv_mm[2] = pitch; g.nu = nu; g.nv = nv; g.nw = 1;
            img.trace(0, tr, sw);
            m = img.labels(tr, &lo);
            picture = img.label_volume(g);
        } else {
            img.trace(0);
            m = img.labels(tr, &lo);
            picture = img.label_picture();
        }
        check(dev->synchronize(), "mcrt_synchronize");
        std::ofstream f(argv[2], std::ios::binary);
        f.write((const char *)m.tissue.data(), (std::streamsize)m.tissue.size());
        f.write((const char *)m.interface.data(), (std::streamsize)(m.interface.size() * 4));
        f.write((const char *)m.crossings.data(), (std::streamsize)(m.crossings.size() * 4));
        f.write((const char *)picture.data(), (std::streamsize)picture.size());
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
