// Colour Doppler through the C++ shim (tests/test_gpu_flow_chain.py builds and runs it): one frame of a scene file under 64 scan-lines --
// trace, rf_image::flow_split, the B-mode chain, rf_image::colour_flow.  Writes: the rgb bytes [200][250][3], the grey bytes [200][250],
// then as float32 the velocity picture [200][250] and the beam-space vel, var and truth [64][465] each.
//     flow_driver <scene> <out.bin> <frame> <material> <vx> <vy> <vz> <sigma> [noise_db]
#include "mcrt_host.hpp"
#include <cstdlib>
#include <fstream>
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 64;
using image = rf_image<E, 100, 322>;       // 465 rows
using psf_ = psf<7, 13, 7, 145>;

int main(int argc, char **argv)
{
    if (argc < 9) { std::cerr << "usage: flow_driver scene out.bin frame material vx vy vz sigma [noise_db]" << std::endl; return 2; }
    try {
        const json cfg = load_json(argv[1]);
        const auto &t_pos = cfg.at("transducerPosition");
        const auto &t_dir = cfg.at("transducerAngles");
        const double amplitude = 60.0 * 3.14159265358979323846264338327950288419716939937510 / 180.0;
        const double separation_mm = (((double)(float)amplitude * 3.0) / (double)E) * 10.0;
        transducer<E> t(4.5f, 3.0, separation_mm, vec3((float)t_pos[0], (float)t_pos[1], (float)t_pos[2]),
                        std::array<float, 3>{ (float)t_dir[0], (float)t_dir[1], (float)t_dir[2] });
        auto dev = std::make_shared<device>(std::vector<int>{ 0 });
        scene sc{ cfg, t, dev, 8 };
        sc.step(1000.0f);
        image img{ dev, 30.0, amplitude };
        const psf_ p{ 4.5f, 0.05f, 0.2f, 0.1f };
        std::vector<float> vel(3 * sc.material_names.size(), 0.0f);
        const uint32_t m = sc.material_index(argv[4]);
        for (int k = 0; k < 3; k++) vel[3 * m + k] = (float)std::atof(argv[5 + k]);
        mcrt_flow_opts fo; mcrt_default_flow_opts(&fo);
        fo.sigma = (float)std::atof(argv[8]);
        mcrt_colour_opts co; mcrt_default_colour_opts(&co);
        mcrt_bmode_params bp; mcrt_default_bmode(&bp);
        bp.out_rows = 200; bp.out_cols = 250;
        const bool noise = argc > 9;
        mcrt_noise_opts no; mcrt_default_noise_opts(&no);
        if (noise) no.snr_db = (float)std::atof(argv[9]);

        img.trace((uint32_t)std::atoi(argv[3]));
        img.flow_split(t, vel);
        img.convolve(p);
        if (noise) img.add_noise(no);
        img.envelope();
        img.postprocess(bp);
        std::vector<unsigned char> rgb;
        std::vector<float> velocity;
        const auto maps = img.colour_flow(p, fo, co, rgb, noise, 4.0, nullptr, &velocity);

        std::ofstream f(argv[2], std::ios::binary);
        const std::vector<unsigned char> grey = img.bmode();
        f.write((const char *)rgb.data(), (std::streamsize)rgb.size());
        f.write((const char *)grey.data(), (std::streamsize)grey.size());
        auto put = [&](const std::vector<float> &v) { f.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(float))); };
        put(velocity); put(maps.vel); put(maps.var); put(maps.truth);
        if (!f) throw std::runtime_error("cannot write the output");
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
