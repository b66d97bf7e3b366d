// Shear-wave elastography through the C++ shim (tests/test_gpu_shear_chain.py builds and runs it): one frame of a scene file under 64
// scan-lines -- trace, the PSF, rf_image::shear_wave, the B-mode chain, rf_image::shear_speed, rf_image::shear_elastogram.  Writes: the rgb
// bytes [200][250][3], the grey bytes [200][250], then as float32 the beam-space speed, modulus, quality, peak_time, peak_disp,
// truth_arrival and truth_speed [64][465] each.
//     shear_driver <scene> <out.bin> <frame> <material> <speed_m_s> <push_line> <push_row0> <push_rows> <n_pulses> <prf_hz> <sigma>
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
    if (argc < 12) { std::cerr << "usage: shear_driver scene out.bin frame material speed_m_s push_line push_row0 push_rows n_pulses prf_hz sigma" << std::endl; return 2; }
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
        std::vector<double> speed(sc.material_names.size(), 2.0);
        speed[sc.material_index(argv[4])] = std::atof(argv[5]);
        mcrt_shear_opts so; mcrt_default_shear_opts(&so);
        so.push_line = (uint32_t)std::atoi(argv[6]); so.push_row0 = (uint32_t)std::atoi(argv[7]); so.push_rows = (uint32_t)std::atoi(argv[8]);
        so.n_pulses = (uint32_t)std::atoi(argv[9]); so.prf_hz = (float)std::atof(argv[10]); so.sigma = (float)std::atof(argv[11]);
        mcrt_elastogram_opts eo; mcrt_default_elastogram_opts(&eo);
        eo.ref_strain = 12.0f;                      // kPa: 3 rho c^2 at 2 m/s
        mcrt_bmode_params bp; mcrt_default_bmode(&bp);
        bp.out_rows = 200; bp.out_cols = 250;
        double cycles = 0.0;
        if (mcrt_psf_carrier(4.5f, 145, &cycles) != MCRT_OK) throw std::runtime_error(mcrt_last_error());

        img.trace((uint32_t)std::atoi(argv[3]));
        img.convolve(p);
        const auto wave = img.shear_wave(t, speed, so, cycles);
        img.envelope();
        img.postprocess(bp);
        const auto maps = img.shear_speed(so);
        std::vector<unsigned char> rgb;
        img.shear_elastogram(eo, rgb);

        std::ofstream f(argv[2], std::ios::binary);
        const std::vector<unsigned char> grey = img.bmode();
        f.write((const char *)rgb.data(), (std::streamsize)rgb.size());
        f.write((const char *)grey.data(), (std::streamsize)grey.size());
        auto put = [&](const std::vector<float> &v) { f.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(float))); };
        put(maps.speed); put(maps.modulus); put(maps.quality); put(wave.peak_time); put(wave.peak_disp); put(wave.truth_arrival); put(wave.truth_speed);
        if (!f) throw std::runtime_error("cannot write the output");
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
