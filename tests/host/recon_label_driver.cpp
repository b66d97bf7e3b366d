// recon_label_driver <scene.json> <samples> <N> <step_mm> <x0,y0,z0,x1,y1,z1> <voxel_mm> <traced|geometric> <offset> <fill> <out.raw>: the freehand
// label path of the C++ shim by hand -- transducer::freehand's poses (no fan) handed to rf_image::trace, rf_image::reconstruct_labels with
// the scene's material count -- and the state rules around it (tests/test_gpu_recon_label.py compares the bytes with
// Simulator.freehand_labels and mattausch_hip --freehand-labels)
#include "mcrt_host.hpp"
#include <cstring>
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 512;
using rf_image_ = rf_image<E, 100, 322>;
using transducer_ = transducer<E>;

int main(int argc, char **argv)
{
    if (argc < 11) { std::cout << "usage" << std::endl; return 2; }
    try {
        const json cfg = load_json(argv[1]);
        const uint32_t samples = (uint32_t)std::atoi(argv[2]), N = (uint32_t)std::atoi(argv[3]);
        const double step_mm = std::atof(argv[4]), voxel = std::atof(argv[6]);
        double box[6]; int nb = 0;
        for (const char *q = argv[5]; *q && nb < 6;) { box[nb++] = std::atof(q); while (*q && *q != ',') q++; if (*q == ',') q++; }
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
        mcrt_label_opts lo; mcrt_default_label_opts(&lo);
        lo.rule = !std::strcmp(argv[7], "geometric") ? MCRT_LABEL_GEOMETRIC : MCRT_LABEL_TRACED; lo.start_offset = (float)std::atof(argv[8]);
        mcrt_recon_label_opts ro; mcrt_default_recon_label_opts(&ro, (uint32_t)sc.materials.size());
        ro.fill_radius = (uint32_t)std::atoi(argv[9]);
        bool threw = false;
        try { img.reconstruct_labels(g, ro, &lo); } catch (const std::invalid_argument &) { threw = true; }     // nothing tracked yet
        if (!threw) throw std::runtime_error("reconstruct_labels() before trace(frame, poses) did not throw");
        const auto poses = t.freehand(N, step_mm, 0.0);
        img.trace(0, poses.pos, poses.dir);
        std::vector<uint32_t> counts, votes;
        const std::vector<unsigned char> lab = img.reconstruct_labels(g, ro, &lo, &counts, &votes);
        size_t sampled = 0;
        for (size_t i = 0; i < lab.size(); i++) {
            sampled += counts[i] != 0;
            if (votes[i] > counts[i] || (counts[i] != 0) != (votes[i] != 0)) throw std::runtime_error("a winner's votes are not a share of its voxel's");
            if (ro.fill_radius == 0 && (counts[i] != 0) != (lab[i] != MCRT_LABEL_NONE)) throw std::runtime_error("without filling a voxel has a label exactly where it was sampled");
        }
        if (counts.size() != lab.size() || votes.size() != lab.size() || sampled == 0) throw std::runtime_error("no voxel was sampled");
        if (img.reconstruct_labels(g, ro, &lo) != lab) throw std::runtime_error("the same call twice, without counts and votes, gave other labels");
        img.trace(0);                                                                               // another kind of trace ends the tracked state
        threw = false;
        try { img.reconstruct_labels(g, ro, &lo); } catch (const std::invalid_argument &) { threw = true; }
        if (!threw) throw std::runtime_error("reconstruct_labels() after trace(frame) did not throw");
        std::ofstream f(argv[10], std::ios::binary);
        f.write((const char *)lab.data(), (std::streamsize)lab.size());
        std::cout << g.nu << " x " << g.nv << " x " << g.nw << ", " << sampled << " sampled" << std::endl;
    } catch (const std::exception &ex) {
        std::cout << "error: " << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
