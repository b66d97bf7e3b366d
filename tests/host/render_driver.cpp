// Volume rendering through the C++ shim (tests/test_gpu_render.py builds and runs it): rf_image::trace(frame, transducer, sweep), convolve /
// envelope over the planes, then rf_image::render of a box of voxels seen from a direction, once per mode.  Writes the three pictures
// [ny][nx] as bytes: MIP, mean, surface.
//     render_driver <scene.json> <out.bin> <frame> <samples> <planes> <step_rad> <pivot_mm> <x0> <y0> <z0> <voxel_mm> <nu> <nv> <nw>
//                   <dx> <dy> <dz> <pixel_mm> <step_mm> <nx> <ny>
#include "mcrt_host.hpp"
#include <cstdlib>
#include <fstream>
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 16;
using image = rf_image<E, 100, 322>;       // 465 rows, 0.322 mm apart
using psf_ = psf<7, 13, 7, 145>;

int main(int argc, char **argv)
{
    if (argc < 22) { std::cerr << "usage: render_driver scene.json out.bin frame samples planes step_rad pivot_mm x0 y0 z0 voxel_mm nu nv nw dx dy dz pixel_mm step_mm nx ny" << std::endl; return 2; }
    try {
        const json cfg = load_json(argv[1]);
        const uint32_t frame = (uint32_t)std::atol(argv[3]);
        const mcrt_sweep sw{ (uint32_t)std::atoi(argv[5]), (float)std::atof(argv[6]), (float)std::atof(argv[7]) };
        const double voxel = std::atof(argv[11]);
        mcrt_volume_grid g{};
        for (int k = 0; k < 3; k++) g.origin_mm[k] = std::atof(argv[8 + k]);
        g.du_mm[0] = g.dv_mm[1] = g.dw_mm[2] = voxel;
        g.nu = (uint32_t)std::atoi(argv[12]); g.nv = (uint32_t)std::atoi(argv[13]); g.nw = (uint32_t)std::atoi(argv[14]);
        const double dir[3] = { std::atof(argv[15]), std::atof(argv[16]), std::atof(argv[17]) }, up[3] = { 0.0, 0.0, 1.0 };
        mcrt_render_view view;
        check(mcrt_render_view_for_grid(&g, dir, up, std::atof(argv[18]), std::atof(argv[19]), (uint32_t)std::atoi(argv[20]), (uint32_t)std::atoi(argv[21]), &view),
              "mcrt_render_view_for_grid");
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
        img.trace(frame, tr, sw);
        img.convolve(p);
        img.envelope();
        std::ofstream f(argv[2], std::ios::binary);
        for (uint32_t mode : { (uint32_t)MCRT_RENDER_MIP, (uint32_t)MCRT_RENDER_MEAN, (uint32_t)MCRT_RENDER_SURFACE }) {
            mcrt_render_opts o;
            check(mcrt_default_render_opts(&o, 1), "mcrt_default_render_opts");
            o.mode = mode;
            const std::vector<unsigned char> pic = img.render(g, view, &o);          // (the display: mcrt_default_bmode)
            f.write((const char *)pic.data(), (std::streamsize)pic.size());
        }
        check(dev->synchronize(), "mcrt_synchronize");
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
