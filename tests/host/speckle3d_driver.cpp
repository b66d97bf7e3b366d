// 3-D speckle reduction through the C++ shim (tests/test_gpu_speckle3d.py builds and runs it): rf_image::volume(grid, filter) over a sweep and
// rf_image::reconstruct(grid, opts, counts, filter) over a freehand acquisition, each beside the same call without the filter.  Writes four
// float32 blocks: the sweep's plain and filtered [nw][nv][nu], the freehand's plain and filtered.
//     speckle3d_driver <scene.json> <out.bin> <frame> <samples> <planes> <step_rad> <pivot_mm> <depth_mm> <nu> <nv> <nw> <pitch_mm> <n_iter>
//                      <N> <step_mm> <fan_deg> <x0,y0,z0,x1,y1,z1> <voxel_mm>
// The sweep's grid is centred on (0, depth_mm, 0): u along x and v along y pitch_mm apart, w along z 2 * pitch_mm apart -- weights (1, 1, 0.25).
#include "mcrt_host.hpp"
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 64;
using image = rf_image<E, 100, 322>;       // 465 rows, 0.322 mm apart
using psf_ = psf<7, 13, 7, 145>;

int main(int argc, char **argv)
{
    if (argc < 19) { std::cerr << "usage" << std::endl; return 2; }
    try {
        const json cfg = load_json(argv[1]);
        const uint32_t frame = (uint32_t)std::atol(argv[3]);
        const mcrt_sweep sw{ (uint32_t)std::atoi(argv[5]), (float)std::atof(argv[6]), (float)std::atof(argv[7]) };
        const double depth = std::atof(argv[8]), pitch = std::atof(argv[12]);
        const uint32_t nu = (uint32_t)std::atoi(argv[9]), nv = (uint32_t)std::atoi(argv[10]), nw = (uint32_t)std::atoi(argv[11]);
        mcrt_volume_grid g{};
        g.origin_mm[0] = -(double)(nu - 1) * pitch / 2.0; g.origin_mm[1] = depth - (double)(nv - 1) * pitch / 2.0; g.origin_mm[2] = -(double)(nw - 1) * pitch;
        g.du_mm[0] = pitch; g.dv_mm[1] = pitch; g.dw_mm[2] = 2.0 * pitch; g.nu = nu; g.nv = nv; g.nw = nw;
        mcrt_speckle3d_opts filter;
        check(mcrt_default_speckle3d_opts(&filter), "mcrt_default_speckle3d_opts");
        filter.n_iter = (uint32_t)std::atoi(argv[13]);
        check(mcrt_speckle3d_weights(&g, filter.weight), "mcrt_speckle3d_weights");
        if (filter.weight[0] != 1.0f || filter.weight[1] != 1.0f || filter.weight[2] != 0.25f) throw std::runtime_error("the sweep grid's weights are not (1, 1, 0.25)");
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
        const std::vector<float> plain = img.volume(g);
        const std::vector<float> smooth = img.volume(g, &filter);
        const std::vector<float> again = img.volume(g, nullptr);                   // the filter leaves the planes alone
        if (again != plain) throw std::runtime_error("volume(grid) after volume(grid, filter) changed");
        // the freehand acquisition
        const uint32_t N = (uint32_t)std::atoi(argv[14]);
        const double step_mm = std::atof(argv[15]), fan_deg = std::atof(argv[16]), voxel = std::atof(argv[18]);
        double box[6]; int nb = 0;
        for (const char *q = argv[17]; *q && nb < 6;) { box[nb++] = std::atof(q); while (*q && *q != ',') q++; if (*q == ',') q++; }
        if (nb != 6) throw std::invalid_argument("six numbers");
        mcrt_volume_grid fg{};
        for (int k = 0; k < 3; k++) fg.origin_mm[k] = box[k];
        fg.du_mm[0] = fg.dv_mm[1] = fg.dw_mm[2] = voxel;
        fg.nu = (uint32_t)std::floor((box[3] - box[0]) / voxel) + 1u; fg.nv = (uint32_t)std::floor((box[4] - box[1]) / voxel) + 1u; fg.nw = (uint32_t)std::floor((box[5] - box[2]) / voxel) + 1u;
        check(mcrt_speckle3d_weights(&fg, filter.weight), "mcrt_speckle3d_weights");
        const auto poses = tr.freehand(N, step_mm, fan_deg);
        img.trace(frame, poses.pos, poses.dir);
        img.convolve(p);
        img.envelope();
        std::vector<uint32_t> c0, c1;
        const std::vector<float> fplain = img.reconstruct(fg, nullptr, &c0);
        const std::vector<float> fsmooth = img.reconstruct(fg, nullptr, &c1, &filter);
        if (c0 != c1) throw std::runtime_error("the counts changed under the filter");
        check(dev->synchronize(), "mcrt_synchronize");
        std::ofstream f(argv[2], std::ios::binary);
        for (const std::vector<float> *v : { &plain, &smooth, &fplain, &fsmooth }) f.write((const char *)v->data(), (std::streamsize)(v->size() * sizeof(float)));
        std::cout << fg.nu << " x " << fg.nv << " x " << fg.nw << std::endl;
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
