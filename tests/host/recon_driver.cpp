// recon_driver <scene.json> <frame> <samples> <N> <step_mm> <fan_deg> <x0,y0,z0,x1,y1,z1> <voxel_mm> <out.raw>: the freehand path of the C++ shim by
// hand -- transducer::freehand's poses handed to rf_image::trace as a vector of transducers' tables, convolve, envelope,
// rf_image::reconstruct (MAX, fill radius 2) -- and the state rules around it (tests/test_gpu_recon.py compares the bytes with
// Simulator.freehand and mattausch_hip --freehand-out)
#include "mcrt_host.hpp"
#include <cstring>
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 512;
using psf_ = psf<7, 13, 7, 145>;
using rf_image_ = rf_image<E, 100, 322>;
using transducer_ = transducer<E>;

int main(int argc, char **argv)
{
    if (argc < 10) { std::cout << "usage" << std::endl; return 2; }
    try {
        const json cfg = load_json(argv[1]);
        const uint32_t frame = (uint32_t)std::atoi(argv[2]), samples = (uint32_t)std::atoi(argv[3]), N = (uint32_t)std::atoi(argv[4]);
        const double step_mm = std::atof(argv[5]), fan_deg = std::atof(argv[6]), voxel = std::atof(argv[8]);
        double box[6]; int nb = 0;
        for (const char *q = argv[7]; *q && nb < 6;) { box[nb++] = std::atof(q); while (*q && *q != ',') q++; if (*q == ',') q++; }
        if (nb != 6) throw std::invalid_argument("six numbers");
        const double amplitude = 60.0 * 3.14159265358979323846264338327950288419716939937510 / 180.0;
        const double separation_mm = (((double)(float)amplitude * 3.0) / (double)E) * 10.0;
        const auto &tp = cfg.at("transducerPosition"); const auto &ta = cfg.at("transducerAngles");
        transducer_ t(4.5f, 3.0, separation_mm, vec3((float)tp[0], (float)tp[1], (float)tp[2]), std::array<float, 3>{ (float)ta[0], (float)ta[1], (float)ta[2] });
        auto dev = std::make_shared<device>(std::vector<int>{ 0 });
        scene sc{ cfg, t, dev, samples };
        rf_image_ img{ dev, 30.0, amplitude };
        mcrt_volume_grid g{};
        for (int k = 0; k < 3; k++) g.origin_mm[k] = box[k];
        g.du_mm[0] = g.dv_mm[1] = g.dw_mm[2] = voxel;
        g.nu = (uint32_t)std::floor((box[3] - box[0]) / voxel) + 1u; g.nv = (uint32_t)std::floor((box[4] - box[1]) / voxel) + 1u; g.nw = (uint32_t)std::floor((box[5] - box[2]) / voxel) + 1u;
        mcrt_recon_opts o; mcrt_default_recon_opts(&o);
        o.mode = MCRT_RECON_MAX; o.fill_radius = 2;
        bool threw = false;
        try { img.reconstruct(g, &o); } catch (const std::invalid_argument &) { threw = true; }     // nothing tracked yet
        if (!threw) throw std::runtime_error("reconstruct() before trace(frame, poses) did not throw");
        const auto poses = t.freehand(N, step_mm, fan_deg);
        img.trace(frame, poses.pos, poses.dir);
        const psf_ p{ 4.5f, 0.05f, 0.2f, 0.1f };
        img.convolve(p);
        img.envelope();
        std::vector<uint32_t> counts;
        const std::vector<float> vox = img.reconstruct(g, &o, &counts);
        size_t sampled = 0;
        for (uint32_t c : counts) sampled += c != 0;
        if (counts.size() != vox.size() || sampled == 0) throw std::runtime_error("no voxel was sampled");
        threw = false;
        try { img.volume(g); } catch (const std::invalid_argument &) { threw = true; }              // tracked frames are no sweep
        if (!threw) throw std::runtime_error("volume() over tracked frames did not throw");
        img.trace(frame);                                                                           // another kind of trace ends the tracked state
        threw = false;
        try { img.reconstruct(g, &o); } catch (const std::invalid_argument &) { threw = true; }
        if (!threw) throw std::runtime_error("reconstruct() after trace(frame) did not throw");
        std::ofstream f(argv[9], std::ios::binary);
        f.write((const char *)vox.data(), (std::streamsize)(vox.size() * sizeof(float)));
        std::cout << g.nu << " x " << g.nv << " x " << g.nw << ", " << sampled << " sampled" << std::endl;
    } catch (const std::exception &ex) {
        std::cout << "error: " << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
