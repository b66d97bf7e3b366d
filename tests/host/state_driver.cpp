// Which call sequences rf_image accepts and which it refuses (tests/test_gpu_shim_state.py builds and runs it, and holds the table): what the
// stack holds after each kind of trace, what the label tables hold after labels(), and the limits of the steer list and the sweep.  Prints
// one line per step, "> <step>: ok[ <detail>]" or "> <step>: <exception type>".
//     state_driver <scene.json>
#include "mcrt_host.hpp"
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 16;
using image = rf_image<E, 100, 322>;       // 465 rows
using psf_ = psf<7, 13, 7, 145>;

template <typename F> static void step(const char *name, F &&f)
{
    std::string r;
    try { r = "ok" + f(); }
    catch (const std::out_of_range &) { r = "out_of_range"; }
    catch (const std::invalid_argument &) { r = "invalid_argument"; }
    catch (const std::exception &ex) { r = std::string("exception ") + ex.what(); }
    std::cout << "> " << name << ": " << r << std::endl;
}
#define DO(name, call) step(name, [&] { call; return std::string(); })
#define PLANES(name) step(name, [&] { return " planes=" + std::to_string(img.labels(tr).planes); })

int main(int argc, char **argv)
{
    if (argc != 2) { std::cerr << "usage: state_driver scene.json" << std::endl; return 2; }
    try {
        const json cfg = load_json(argv[1]);
        const psf_ p{ 4.5f, 0.05f, 0.2f, 0.1f };
        const auto &t_pos = cfg.at("transducerPosition");
        const auto &t_dir = cfg.at("transducerAngles");
        const double amplitude = 60.0 * 3.14159265358979323846264338327950288419716939937510 / 180.0;
        const double separation_mm = (((double)(float)amplitude * 3.0) / (double)E) * 10.0;
        transducer<E> tr(4.5f, 3.0, separation_mm, vec3((float)t_pos[0], (float)t_pos[1], (float)t_pos[2]),
                         std::array<float, 3>{ (float)t_dir[0], (float)t_dir[1], (float)t_dir[2] });
        auto dev = std::make_shared<device>(std::vector<int>{ 0 });
        scene sc{ cfg, tr, dev, 1u };
        image img{ dev, 30.0, amplitude };
        const std::vector<float> steers3{ -0.1f, 0.0f, 0.1f }, steers2{ -0.1f, 0.1f };
        const mcrt_sweep sweep3{ 3, 0.02f, 0.0f }, sweep5{ 5, 0.02f, 0.0f };
        mcrt_volume_grid g{};               // 4 x 4 points of the C-plane at y = 60 mm, 0.5 mm apart: inside the sector and both sweeps
        g.origin_mm[0] = -0.75; g.origin_mm[1] = 60.0; g.origin_mm[2] = -0.75; g.du_mm[0] = 0.5; g.dv_mm[2] = 0.5; g.nu = 4; g.nv = 4; g.nw = 1;
        const uint32_t f = 1;

        // a fresh image
        DO("fresh volume", img.volume(g));
        DO("fresh postprocess(steers3)", img.postprocess(steers3));
        DO("fresh label_picture", img.label_picture());
        DO("fresh label_volume", img.label_volume(g));
        DO("fresh view_intensities(0)", img.view_intensities(0));
        DO("fresh convolve", img.convolve(p));
        DO("fresh envelope", img.envelope());
        DO("fresh postprocess()", img.postprocess());
        step("fresh intensities", [&] { for (float v : img.intensities()) if (v != 0.0f) return std::string(" nonzero"); return std::string(" zero"); });

        // trace(f)
        std::vector<float> plain;
        DO("plain trace", img.trace(f));
        DO("plain postprocess()", img.postprocess());
        DO("plain postprocess(steers3)", img.postprocess(steers3));
        DO("plain volume", img.volume(g));
        PLANES("plain labels");
        DO("plain label_picture", img.label_picture());
        DO("plain label_volume", img.label_volume(g));
        plain = img.intensities();

        // then trace(f, t, steers3)
        DO("steered trace", img.trace(f, tr, steers3));
        DO("steered postprocess(steers3)", img.postprocess(steers3));
        DO("steered postprocess(steers2)", img.postprocess(steers2));
        DO("steered volume", img.volume(g));
        DO("steered view_intensities(2)", img.view_intensities(2));
        DO("steered view_intensities(3)", img.view_intensities(3));
        step("steered intensities", [&] { return std::string(img.intensities() == plain ? " same" : " changed"); });   // (bit for bit: no NaN, no -0 in a traced image)
        PLANES("steered labels");
        DO("steered label_picture", img.label_picture());

        // then trace(f, t, sweep3)
        DO("swept trace", img.trace(f, tr, sweep3));
        DO("swept volume", img.volume(g));
        DO("swept postprocess(steers3)", img.postprocess(steers3));
        PLANES("swept labels");
        DO("swept label_volume", img.label_volume(g));
        DO("swept label_picture", img.label_picture());

        // then trace(f)
        DO("plain again trace", img.trace(f));
        DO("plain again volume", img.volume(g));
        PLANES("plain again labels");
        DO("plain again label_picture", img.label_picture());
        DO("plain again label_volume", img.label_volume(g));

        // labels of a 3-plane sweep under a 5-plane sweep
        DO("resweep trace(sweep3)", img.trace(f, tr, sweep3));
        PLANES("resweep labels");
        DO("resweep trace(sweep5)", img.trace(f, tr, sweep5));
        DO("resweep label_volume, stale", img.label_volume(g));
        PLANES("resweep labels again");
        DO("resweep label_volume", img.label_volume(g));

        // a sweep, then steered views
        DO("sweep-steer trace(sweep3)", img.trace(f, tr, sweep3));
        DO("sweep-steer trace(steers3)", img.trace(f, tr, steers3));
        DO("sweep-steer postprocess(steers3)", img.postprocess(steers3));
        DO("sweep-steer volume", img.volume(g));

        // a sweep, then elevation planes
        DO("sweep-elevation trace(sweep3)", img.trace(f, tr, sweep3));
        DO("sweep-elevation trace(psf, 3)", img.trace(f, tr, p, 3));
        DO("sweep-elevation volume", img.volume(g));
        DO("sweep-elevation convolve", img.convolve(p));
        DO("sweep-elevation postprocess()", img.postprocess());

        // argument limits
        DO("limits 0 steers", img.trace(f, tr, std::vector<float>{}));
        DO("limits 17 steers", img.trace(f, tr, std::vector<float>(17, 0.0f)));
        DO("limits sweep of 0", img.trace(f, tr, mcrt_sweep{ 0, 0.02f, 0.0f }));
        DO("limits sweep of 257", img.trace(f, tr, mcrt_sweep{ 257, 0.001f, 0.0f }));
        check(dev->synchronize(), "mcrt_synchronize");
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
