// The host functions of volume imaging (mcrt_transducer_swept, mcrt_volume_maps; csrc/mcrt_host.cpp) over their error cases and a few grids.
// tests/test_volume_contract.py compiles this file with mcrt_host.cpp under AddressSanitizer + UBSan and runs it; every buffer is exactly as
// large as the contract says, so a write past a map's end is an error.  Prints one line per case and DONE.
#include "mcrt.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static uint64_t fnv(const void *p, size_t n, uint64_t h = 1469598103934665603ull)
{
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

static mcrt_volume_grid grid(double ox, double oy, double oz, double du, double dv, double dw, uint32_t nu, uint32_t nv, uint32_t nw)
{
    mcrt_volume_grid g;
    memset(&g, 0, sizeof g);
    g.origin_mm[0] = ox; g.origin_mm[1] = oy; g.origin_mm[2] = oz;
    g.du_mm[0] = du; g.dv_mm[1] = dv; g.dw_mm[2] = dw;
    g.nu = nu; g.nv = nv; g.nw = nw;
    return g;
}

static void maps_case(const char *name, uint32_t E, uint32_t R, const mcrt_sweep *sw, const mcrt_volume_grid *g, size_t n, bool null_map = false)
{
    std::vector<float> mz(n, -7.25f), mr(n, -7.25f), mc(n, -7.25f);
    const int rc = mcrt_volume_maps(E, R, 30.0, 1.0471975511965976, 100, 1500, sw, g, null_map ? nullptr : mz.data(), mr.data(), mc.data());
    if (rc != MCRT_OK) {
        bool untouched = true;
        for (size_t i = 0; i < n; i++) untouched = untouched && mz[i] == -7.25f && mr[i] == -7.25f && mc[i] == -7.25f;
        printf("%s: error %d %s\n", name, rc, untouched ? "untouched" : "WRITTEN");
        return;
    }
    printf("%s: ok fnv %llu\n", name, (unsigned long long)fnv(mc.data(), 4 * n, fnv(mr.data(), 4 * n, fnv(mz.data(), 4 * n))));
}

static void swept_case(const char *name, uint32_t n, float tilt, float pivot, bool null_dir = false)
{
    const float position[3] = { 1.0f, -2.0f, 3.0f }, angles[3] = { 10.0f, 20.0f, 30.0f };
    std::vector<float> pos(3 * (size_t)(n ? n : 1), -7.25f), dir(pos);
    const int rc = mcrt_transducer_swept(n, 3.0, 0.2454369, position, angles, tilt, pivot, pos.data(), null_dir ? nullptr : dir.data());
    bool untouched = true, finite = true;
    for (size_t i = 0; i < pos.size(); i++) { untouched = untouched && pos[i] == -7.25f && dir[i] == -7.25f; finite = finite && std::isfinite(pos[i]) && std::isfinite(dir[i]); }
    if (rc != MCRT_OK) printf("%s: error %d %s\n", name, rc, untouched ? "untouched" : "WRITTEN");
    else printf("%s: ok %s\n", name, finite ? "finite" : "NOT FINITE");
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const mcrt_sweep sw{ 8, 0.05f, 10.0f };
    mcrt_volume_grid g = grid(-20.0, 60.0, -8.0, 2.5, 2.0, 1.75, 17, 19, 7);
    maps_case("maps.volume", 128, 465, &sw, &g, (size_t)17 * 19 * 7);
    g = grid(-40.0, 90.0, -30.0, 0.5, 0.0, 0.25, 161, 1, 1);
    maps_case("maps.line", 3, 2048, &sw, &g, 161);
    g = grid(0.0, 10.0, 0.0, 0.0, 0.0, 0.0, 1, 1, 1);                 // the pivot itself: h = 0, atan2(0, 0)
    maps_case("maps.at_the_pivot", 1, 2, &sw, &g, 1);
    const mcrt_sweep one{ 1, 0.001f, -20.0f };
    g = grid(-300.0, -300.0, -300.0, 100.0, 100.0, 100.0, 7, 7, 7);   // around and behind the probe
    maps_case("maps.far_and_behind", 512, 2, &one, &g, 343);
    g = grid(-20.0, 60.0, -8.0, 2.5, 2.0, 1.75, 5, 4, 3);
    maps_case("maps.null_map", 128, 465, &sw, &g, 60, true);
    maps_case("maps.null_sweep", 128, 465, nullptr, &g, 60);
    maps_case("maps.null_grid", 128, 465, &sw, nullptr, 60);
    maps_case("maps.zero_elements", 0, 465, &sw, &g, 60);
    maps_case("maps.zero_rows", 128, 0, &sw, &g, 60);
    { mcrt_sweep s = sw; s.n_planes = 0; maps_case("maps.no_planes", 128, 465, &s, &g, 60); }
    { mcrt_sweep s = sw; s.n_planes = 257; maps_case("maps.257_planes", 128, 465, &s, &g, 60); }
    { mcrt_sweep s = sw; s.step_rad = 0.0f; maps_case("maps.step_zero", 128, 465, &s, &g, 60); }
    { mcrt_sweep s = sw; s.step_rad = nan; maps_case("maps.step_nan", 128, 465, &s, &g, 60); }
    { mcrt_sweep s = sw; s.step_rad = 0.45f; maps_case("maps.sweep_past_90_degrees", 128, 465, &s, &g, 60); }
    { mcrt_sweep s = sw; s.pivot_mm = inf; maps_case("maps.pivot_inf", 128, 465, &s, &g, 60); }
    { mcrt_volume_grid h = g; h.nv = 0; maps_case("maps.zero_nv", 128, 465, &sw, &h, 60); }
    { mcrt_volume_grid h = g; h.dw_mm[1] = (double)nan; maps_case("maps.grid_nan", 128, 465, &sw, &h, 60); }
    { mcrt_volume_grid h = g; h.origin_mm[2] = (double)inf; maps_case("maps.grid_inf", 128, 465, &sw, &h, 60); }
    { mcrt_volume_grid h = g; h.nu = 65536; h.nv = 32768; h.nw = 1; maps_case("maps.2^31_points", 128, 465, &sw, &h, 60); }
    swept_case("swept.tilt_0", 512, 0.0f, 10.0f);
    swept_case("swept.tilt_0.3", 512, 0.3f, -20.0f);
    swept_case("swept.tilt_-1.2", 1, -1.2f, 25.0f);
    swept_case("swept.zero_elements", 0, 0.3f, 0.0f);
    swept_case("swept.null_dir", 16, 0.3f, 0.0f, true);
    swept_case("swept.tilt_nan", 16, nan, 0.0f);
    swept_case("swept.tilt_90_degrees", 16, 1.5707964f, 0.0f);
    swept_case("swept.pivot_nan", 16, 0.3f, nan);
    printf("DONE\n");
    return 0;
}
