// The image stages of the C++ shim over every kind of traced pass (tests/test_gpu_stages.py builds and runs it): for each of trace(frame), two
// steered views, a two-plane sweep and two tracked poses, without bands and with two, the chain
//     trace -> convolve -> add_noise (40 dB, seed 77) -> detect (31 taps) -> despeckle (2 iterations) -> autogain (the noise floor),
// and with the two bands the same chain with envelope() in the place of detect(), and trace -> convolve -> add_noise -> fold_bands alone.
// Every pass writes its images (row-major [465][64] float32 each), then -- unless it ended in fold_bands -- the gain curves [frames][465]
// float32 and the penetration rows [frames] uint32, then for the tracked poses reconstruct(grid)'s voxels [nw][nv][nu] float32.
//     stages_driver <scene.json> <out.bin> <frame> <samples> <x0,y0,z0,pitch_mm,nu,nv,nw>
#include "mcrt_host.hpp"
#include <cstdlib>
#include <fstream>
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 64;
using image = rf_image<E, 100, 322>;       // 465 rows, 0.322 mm apart
using psf_ = psf<7, 13, 7, 145>;
enum class detector { quadrature, envelope, none };

int main(int argc, char **argv)
{
    if (argc < 6) { std::cerr << "usage: stages_driver scene.json out.bin frame samples x0,y0,z0,pitch_mm,nu,nv,nw" << std::endl; return 2; }
    try {
        const json cfg = load_json(argv[1]);
        const uint32_t frame = (uint32_t)std::atol(argv[3]);
        double box[7]; int nb = 0;
        for (const char *q = argv[5]; *q && nb < 7;) { box[nb++] = std::atof(q); while (*q && *q != ',') q++; if (*q == ',') q++; }
        if (nb != 7) throw std::invalid_argument("seven numbers");
        mcrt_volume_grid grid{};
        for (int k = 0; k < 3; k++) grid.origin_mm[k] = (float)box[k];
        grid.du_mm[0] = grid.dv_mm[1] = grid.dw_mm[2] = (float)box[3];
        grid.nu = (uint32_t)box[4]; grid.nv = (uint32_t)box[5]; grid.nw = (uint32_t)box[6];
        const auto &t_pos = cfg.at("transducerPosition");
        const auto &t_dir = cfg.at("transducerAngles");
        const double amplitude = 60.0 * 3.14159265358979323846264338327950288419716939937510 / 180.0;
        const double separation_mm = (((double)(float)amplitude * 3.0) / (double)E) * 10.0;
        const std::array<float, 3> angles{ (float)t_dir[0], (float)t_dir[1], (float)t_dir[2] };
        transducer<E> tr(4.5f, 3.0, separation_mm, vec3((float)t_pos[0], (float)t_pos[1], (float)t_pos[2]), angles);
        const std::vector<transducer<E>> poses{ tr, transducer<E>(4.5f, 3.0, separation_mm, vec3((float)t_pos[0], (float)t_pos[1], (float)t_pos[2] + 0.125f), angles) };
        const std::vector<float> steers{ -0.1f, 0.1f };
        const mcrt_sweep sweep{ 2, 0.02f, 0.0f };
        auto dev = std::make_shared<device>(std::vector<int>{ 0 });
        scene sc{ cfg, tr, dev, (unsigned)std::atoi(argv[4]) };
        image img{ dev, 30.0, amplitude };
        mcrt_noise_opts noise; check(mcrt_default_noise_opts(&noise), "mcrt_default_noise_opts");
        noise.mode = MCRT_NOISE_SNR_DB; noise.snr_db = 40.0f; noise.seed = 77u;
        mcrt_detect_opts taps; check(mcrt_default_detect_opts(&taps), "mcrt_default_detect_opts");
        taps.n_taps = 31;
        mcrt_speckle_opts speckle; check(mcrt_default_speckle_opts(&speckle), "mcrt_default_speckle_opts");
        speckle.n_iter = 2;
        mcrt_autogain_opts gain; check(mcrt_default_autogain_opts(&gain), "mcrt_default_autogain_opts");
        std::ofstream f(argv[2], std::ios::binary);
        auto put = [&](const auto &v) { f.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(v[0]))); };

        auto pass = [&](int mode, bool bands, detector how) {
            psf_ p{ 4.5f, 0.05f, 0.2f, 0.1f };
            if (bands) {
                mcrt_bands b; check(mcrt_default_bands(&b, 4.5f, 0.05f), "mcrt_default_bands");
                b.n_bands = 2; b.band_mhz[0] = 4.0f; b.band_mhz[1] = 5.0f; b.band_weight[0] = 1.0f; b.band_weight[1] = 2.0f;
                p.set_bands(b);
            }
            switch (mode) {
            case 0: img.trace(frame); break;
            case 1: img.trace(frame, tr, steers); break;
            case 2: img.trace(frame, tr, sweep); break;
            default: img.trace(frame, poses); break;
            }
            img.convolve(p);
            img.add_noise(noise);
            if (how == detector::none) img.fold_bands();
            else {
                if (how == detector::quadrature) img.detect(taps); else img.envelope();
                img.despeckle(speckle);
                img.autogain(gain, true);
            }
            if (mode == 0) put(img.intensities());
            else for (uint32_t n = 0; n < 2; n++) put(img.view_intensities(n));
            if (how != detector::none) { put(img.gain_curve()); put(img.penetration_rows()); }
            if (mode == 3) put(img.reconstruct(grid));
        };
        for (int mode = 0; mode < 4; mode++) {
            pass(mode, false, detector::quadrature);
            pass(mode, true, detector::quadrature);
            pass(mode, true, detector::envelope);
            pass(mode, true, detector::none);
        }
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
