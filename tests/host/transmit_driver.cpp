// Acoustic ground truth through the C++ shim (tests/test_gpu_transmit.py builds and runs it): rf_image::transmission and transmission_picture on a
// scene file -- on one context, or on a group whose ranks share the GPU --, each checked here against the C ABI called beside it
// (mcrt_transmit_frames on the tracing context, mcrt_scan_convert_frames on the root) bit for bit.  Writes transmit [E][R] float, reflect
// [E][R] float, crossings [E] uint32 and the picture [400][500] float.  Exit code 3: the shim and the C ABI disagree.
//     transmit_driver <scene.json> <out.bin> <devices 0 | 0,0> <mode 0|1> <rule 0|1> <offset>
#include "mcrt_host.hpp"
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

using namespace mcrt_host;

constexpr size_t E = 64;
using image = rf_image<E, 100, 322>;       // 465 rows, 0.322 mm apart

int main(int argc, char **argv)
{
    if (argc != 7) { std::cerr << "usage: transmit_driver scene.json out.bin devices mode rule offset" << std::endl; return 2; }
    try {
        const json cfg = load_json(argv[1]);
        std::vector<int> devices;
        for (const char *q = argv[3]; *q;) { devices.push_back(std::atoi(q)); while (*q && *q != ',') q++; if (*q == ',') q++; }
        mcrt_transmit_opts to; check(mcrt_default_transmit_opts(&to), "mcrt_default_transmit_opts");
        to.mode = (uint32_t)std::atoi(argv[4]); to.rule = (uint32_t)std::atoi(argv[5]); to.start_offset = (float)std::atof(argv[6]);
        const auto &t_pos = cfg.at("transducerPosition");
        const auto &t_dir = cfg.at("transducerAngles");
        const double amplitude = 60.0 * 3.14159265358979323846264338327950288419716939937510 / 180.0;
        const double separation_mm = (((double)(float)amplitude * 3.0) / (double)E) * 10.0;
        transducer<E> tr(4.5f, 3.0, separation_mm, vec3((float)t_pos[0], (float)t_pos[1], (float)t_pos[2]),
                         std::array<float, 3>{ (float)t_dir[0], (float)t_dir[1], (float)t_dir[2] });
        auto dev = std::make_shared<device>(devices);
        scene sc{ cfg, tr, dev, 4u };
        image img{ dev, 30.0, amplitude };
        img.trace(0);
        const image::transmission_maps m = img.transmission(tr, &to);
        const std::vector<float> picture = img.transmission_picture();
        check(dev->synchronize(), "mcrt_synchronize");
        // the same through the C ABI, into buffers of this program
        const size_t n = E * image::max_rows, npix = 400 * 500;
        void *buf = nullptr, *pic = nullptr;
        check(mcrt_alloc(dev->ctx, 4 * (2 * n + E), &buf), "mcrt_alloc");
        check(mcrt_alloc(dev->ctx, 4 * npix, &pic), "mcrt_alloc");
        float *t_dev = (float *)buf, *r_dev = t_dev + n; uint32_t *c_dev = (uint32_t *)(r_dev + n);
        check(mcrt_transmit_frames(dev->tracer(), 1, 0, E, tr.pos.data(), tr.dir.data(), &to, t_dev, r_dev, c_dev), "mcrt_transmit_frames");
        check(mcrt_synchronize(dev->tracer()), "mcrt_synchronize");
        check(mcrt_scan_convert_frames(dev->ctx, t_dev, 1, E, image::max_rows, 30.0, amplitude, (float *)pic, 400, 500), "mcrt_scan_convert_frames");
        std::vector<float> t(n), r(n), p(npix); std::vector<uint32_t> c(E);
        check(mcrt_memcpy_d2h(dev->ctx, t.data(), t_dev, 4 * n), "mcrt_memcpy_d2h");
        check(mcrt_memcpy_d2h(dev->ctx, r.data(), r_dev, 4 * n), "mcrt_memcpy_d2h");
        check(mcrt_memcpy_d2h(dev->ctx, c.data(), c_dev, 4 * E), "mcrt_memcpy_d2h");
        check(mcrt_memcpy_d2h(dev->ctx, p.data(), pic, 4 * npix), "mcrt_memcpy_d2h");
        mcrt_free(dev->ctx, buf); mcrt_free(dev->ctx, pic);
        if (m.planes != 1 || m.transmit.size() != n || m.reflect.size() != n || m.crossings.size() != E || picture.size() != npix
            || std::memcmp(m.transmit.data(), t.data(), 4 * n) || std::memcmp(m.reflect.data(), r.data(), 4 * n) || std::memcmp(m.crossings.data(), c.data(), 4 * E)
            || std::memcmp(picture.data(), p.data(), 4 * npix)) {
            std::cerr << "rf_image::transmission / transmission_picture differ from the C ABI's result" << std::endl;
            return 3;
        }
        std::ofstream f(argv[2], std::ios::binary);
        f.write((const char *)m.transmit.data(), (std::streamsize)(4 * n));
        f.write((const char *)m.reflect.data(), (std::streamsize)(4 * n));
        f.write((const char *)m.crossings.data(), (std::streamsize)(4 * E));
        f.write((const char *)picture.data(), (std::streamsize)(4 * npix));
    } catch (const std::exception &ex) {
        std::cerr << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
