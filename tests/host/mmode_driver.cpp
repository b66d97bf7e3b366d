// M-mode through the C++ shim (tests/test_gpu_mmode_chain.py builds and runs it): one frame of a scene file under 64 scan-lines -- trace,
// the PSF, rf_image::m_lines, rf_image::m_mode.  Writes: the grey bytes [H][W], the label bytes [H][W], then as float32 the true
// displacement [H][W] and the envelopes of every pulse [n_pulses][465], with W = n_pulses / hop.
//     mmode_driver <scene> <out.bin> <frame> <line> <material> <dilation> <n_pulses> <prf_hz> <beats_per_min> <bulk_rows> <bulk_per_min> <hop> <height> <sigma>
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
    if (argc < 15) { std::cerr << "usage: mmode_driver scene out.bin frame line material dilation n_pulses prf_hz beats_per_min bulk_rows bulk_per_min hop height sigma" << std::endl; return 2; }
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
        std::vector<double> dilation(sc.material_names.size(), 0.0);
        dilation[sc.material_index(argv[5])] = std::atof(argv[6]);
        mcrt_mmode_opts mo; mcrt_default_mmode_opts(&mo);
        mo.n_pulses = (uint32_t)std::atoi(argv[7]); mo.sigma = (float)std::atof(argv[14]);
        mcrt_mmode_display_opts dopts; mcrt_default_mmode_display_opts(&dopts);
        dopts.hop = (uint32_t)std::atoi(argv[12]); dopts.height = (uint32_t)std::atoi(argv[13]);
        std::vector<int32_t> w(mo.n_pulses), bulk(mo.n_pulses);
        if (mcrt_mmode_waveform(std::atof(argv[8]), std::atof(argv[9]), mo.n_pulses, w.data()) != MCRT_OK) throw std::runtime_error(mcrt_last_error());
        if (mcrt_mmode_bulk(std::atof(argv[8]), std::atof(argv[11]), std::atof(argv[10]), mo.n_pulses, bulk.data()) != MCRT_OK) throw std::runtime_error(mcrt_last_error());
        double cycles = 0.0;
        if (mcrt_psf_carrier(4.5f, 145, &cycles) != MCRT_OK) throw std::runtime_error(mcrt_last_error());

        img.trace((uint32_t)std::atoi(argv[3]));
        img.convolve(p);
        const auto lines = img.m_lines(t, (uint32_t)std::atoi(argv[4]), dilation, w, bulk, mo, cycles);
        const auto pic = img.m_mode(dopts);

        std::ofstream f(argv[2], std::ios::binary);
        f.write((const char *)pic.picture.data(), (std::streamsize)pic.picture.size());
        f.write((const char *)pic.labels.data(), (std::streamsize)pic.labels.size());
        f.write((const char *)pic.truth_disp.data(), (std::streamsize)(pic.truth_disp.size() * sizeof(float)));
        f.write((const char *)lines.env.data(), (std::streamsize)(lines.env.size() * sizeof(float)));
        if (!f) throw std::runtime_error("cannot write the output");
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
