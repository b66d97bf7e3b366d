// Spectral Doppler through the C++ shim (tests/test_gpu_spectral_chain.py builds and runs it): one frame of a scene file under 64
// scan-lines -- trace, rf_image::flow_split, rf_image::flow, then rf_image::tissue_line, spectral_series, spectrum and sonogram of one
// gate under mcrt_pulse_waveform.  Writes as float32 the series [T][2], the power [n_cols][N] and the mean [n_cols], then the bytes [N][n_cols].
//     spectral_driver <scene> <out.bin> <frame> <material> <vx> <vy> <vz> <line> <row0> <gate_rows> <n_pulses> <sigma>
#include "mcrt_host.hpp"
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 64;
using image = rf_image<E, 100, 322>;       // 465 rows
using psf_ = psf<7, 13, 7, 145>;

static void ok(int rc, const char *what) { if (rc != MCRT_OK) throw std::runtime_error(std::string(what) + ": " + mcrt_last_error()); }

int main(int argc, char **argv)
{
    if (argc < 13) { std::cerr << "usage: spectral_driver scene out.bin frame material vx vy vz line row0 gate_rows n_pulses sigma" << std::endl; return 2; }
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
        const uint32_t L = (uint32_t)sc.material_names.size(), m = sc.material_index(argv[4]);
        std::vector<float> vel(3 * L, 0.0f);
        for (int k = 0; k < 3; k++) vel[3 * m + k] = (float)std::atof(argv[5 + k]);
        const uint32_t line = (uint32_t)std::atoi(argv[8]), row0 = (uint32_t)std::atoi(argv[9]);
        mcrt_flow_opts fo; mcrt_default_flow_opts(&fo);
        mcrt_spectral_opts so; mcrt_default_spectral_opts(&so);
        so.gate_rows = (uint32_t)std::atoi(argv[10]); so.n_pulses = (uint32_t)std::atoi(argv[11]); so.sigma = (float)std::atof(argv[12]);
        mcrt_sonogram_opts go; mcrt_default_sonogram_opts(&go);

        img.trace((uint32_t)std::atoi(argv[3]));
        img.flow_split(t, vel);
        const auto maps = img.flow(p, fo);

        // the material's speed is the waveform's peak, its direction against the gate line's the cosine
        const double vx = vel[3 * m], vy = vel[3 * m + 1], vz = vel[3 * m + 2], norm = std::sqrt((vx * vx + vy * vy) + vz * vz);
        const double ux = (float)(vx / norm), uy = (float)(vy / norm), uz = (float)(vz / norm);
        const double dx = t.dir[3 * line], dy = t.dir[3 * line + 1], dz = t.dir[3 * line + 2];
        double axial = 0.0 - ((ux * dx + uy * dy) + uz * dz);
        axial = axial < -1.0 ? -1.0 : axial > 1.0 ? 1.0 : axial;
        std::vector<uint8_t> moving(L, 0); moving[m] = 1;
        const std::vector<uint8_t> labels = img.tissue_line(line);
        std::vector<float> frac(so.gate_rows), speed(so.n_pulses);
        std::vector<int32_t> rate(so.gate_rows);
        std::vector<int64_t> phase(so.n_pulses);
        ok(mcrt_spectral_profile(labels.data(), (uint32_t)labels.size(), row0, so.gate_rows, moving.data(), L, 2.0, frac.data()), "mcrt_spectral_profile");
        ok(mcrt_spectral_rates(frac.data(), so.gate_rows, axial, rate.data()), "mcrt_spectral_rates");
        ok(mcrt_pulse_waveform((double)fo.prf_hz, 72.0, norm, 0.0, so.n_pulses, speed.data()), "mcrt_pulse_waveform");
        ok(mcrt_spectral_phase(maps.v_nyq_mm_s, speed.data(), so.n_pulses, phase.data()), "mcrt_spectral_phase");

        const std::vector<float> series = img.spectral_series(line, row0, so, rate, phase);
        const auto sp = img.spectrum(so, maps.v_nyq_mm_s);
        const std::vector<unsigned char> grey = img.sonogram(go);

        std::ofstream f(argv[2], std::ios::binary);
        auto put = [&](const std::vector<float> &v) { f.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(float))); };
        put(series); put(sp.power); put(sp.mean);
        f.write((const char *)grey.data(), (std::streamsize)grey.size());
        if (!f) throw std::runtime_error("cannot write the output");
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
