// The host helper of volume rendering (mcrt_render_view_for_grid; csrc/mcrt_host.cpp) over its error cases and a few views.
// tests/test_render_contract.py compiles this file with mcrt_host.cpp under AddressSanitizer + UBSan and runs it; the view is a struct of
// exactly the contract's size between two guard words.  Prints one line per case and DONE.
#include "mcrt.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

static mcrt_volume_grid grid(double du, double dv, double dw, uint32_t nu, uint32_t nv, uint32_t nw)
{
    mcrt_volume_grid g;
    memset(&g, 0, sizeof g);
    g.origin_mm[0] = -3.0; g.origin_mm[1] = 41.0; g.origin_mm[2] = -2.5;
    g.du_mm[0] = du; g.dv_mm[1] = dv; g.dw_mm[2] = dw;
    g.nu = nu; g.nv = nv; g.nw = nw;
    return g;
}

static void view_case(const char *name, const mcrt_volume_grid *g, const double *dir, const double *up, double pixel, double step, uint32_t nx, uint32_t ny,
                      bool null_out = false)
{
    struct { uint32_t before; mcrt_render_view v; uint32_t after; } box;
    memset(&box, 0xA5, sizeof box);
    const int rc = mcrt_render_view_for_grid(g, dir, up, pixel, step, nx, ny, null_out ? nullptr : &box.v);
    bool untouched = true;
    for (size_t i = 0; i < sizeof box; i++) untouched = untouched && ((const unsigned char *)&box)[i] == 0xA5;
    if (rc != MCRT_OK) { printf("%s: error %d %s\n", name, rc, untouched ? "untouched" : "WRITTEN"); return; }
    bool finite = box.before == 0xA5A5A5A5u && box.after == 0xA5A5A5A5u;
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(box.v.origin[k]) && std::isfinite(box.v.di[k]) && std::isfinite(box.v.dj[k]) && std::isfinite(box.v.ds[k]);
    printf("%s: ok %u x %u, %u steps, %s\n", name, box.v.nx, box.v.ny, box.v.n_steps, finite ? "finite" : "NOT FINITE");
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double z[3] = { 0, 0, 1 }, y[3] = { 0, 1, 0 }, obl[3] = { 0.5, 0.3, 0.8 }, zero[3] = { 0, 0, 0 }, bad[3] = { 0, nan, 1 }, far[3] = { inf, 0, 0 }, mz[3] = { 0, 0, -2 };
    mcrt_volume_grid g = grid(0.5, 0.375, 0.75, 17, 13, 11);
    view_case("view.along_w", &g, z, y, 0.25, 0.25, 33, 35);
    view_case("view.oblique", &g, obl, y, 0.1, 0.05, 64, 3);
    view_case("view.one_pixel", &g, obl, z, 1.0, 1.0, 1, 1);
    { mcrt_volume_grid h = grid(0.5, 0.375, 0.75, 1, 1, 1); view_case("view.one_voxel", &h, z, y, 0.25, 0.25, 5, 4); }
    { mcrt_volume_grid h = g; h.du_mm[1] = 0.2; h.dv_mm[2] = -0.1; h.dw_mm[0] = 0.3; view_case("view.sheared_grid", &h, obl, y, 0.25, 0.25, 9, 7); }
    view_case("view.many_steps", &g, z, y, 0.25, 12.5 / 4095.5, 2, 2);
    view_case("view.null_grid", nullptr, z, y, 0.25, 0.25, 4, 4);
    view_case("view.null_dir", &g, nullptr, y, 0.25, 0.25, 4, 4);
    view_case("view.null_up", &g, z, nullptr, 0.25, 0.25, 4, 4);
    view_case("view.null_out", &g, z, y, 0.25, 0.25, 4, 4, true);
    view_case("view.zero_nx", &g, z, y, 0.25, 0.25, 0, 4);
    view_case("view.zero_ny", &g, z, y, 0.25, 0.25, 4, 0);
    view_case("view.dir_zero", &g, zero, y, 0.25, 0.25, 4, 4);
    view_case("view.dir_nan", &g, bad, y, 0.25, 0.25, 4, 4);
    view_case("view.dir_inf", &g, far, y, 0.25, 0.25, 4, 4);
    view_case("view.up_parallel", &g, z, mz, 0.25, 0.25, 4, 4);
    view_case("view.up_zero", &g, z, zero, 0.25, 0.25, 4, 4);
    view_case("view.up_nan", &g, z, bad, 0.25, 0.25, 4, 4);
    view_case("view.pixel_zero", &g, z, y, 0.0, 0.25, 4, 4);
    view_case("view.pixel_negative", &g, z, y, -0.25, 0.25, 4, 4);
    view_case("view.pixel_nan", &g, z, y, nan, 0.25, 4, 4);
    view_case("view.step_zero", &g, z, y, 0.25, 0.0, 4, 4);
    view_case("view.step_inf", &g, z, y, 0.25, inf, 4, 4);
    { mcrt_volume_grid h = g; h.dw_mm[2] = 0.0; view_case("view.a_cut", &h, z, y, 0.25, 0.25, 4, 4); }
    { mcrt_volume_grid h = g; h.dw_mm[0] = 0.5; h.dw_mm[2] = 0.0; view_case("view.coplanar_axes", &h, z, y, 0.25, 0.25, 4, 4); }
    { mcrt_volume_grid h = g; h.nv = 0; view_case("view.zero_nv", &h, z, y, 0.25, 0.25, 4, 4); }
    { mcrt_volume_grid h = g; h.origin_mm[1] = nan; view_case("view.grid_nan", &h, z, y, 0.25, 0.25, 4, 4); }
    { mcrt_volume_grid h = g; h.dv_mm[0] = inf; view_case("view.grid_inf", &h, z, y, 0.25, 0.25, 4, 4); }
    view_case("view.too_many_steps", &g, z, y, 0.25, 1e-4, 4, 4);
    view_case("view.steps_overflow", &g, z, y, 0.25, 1e-300, 4, 4);
    {
        mcrt_render_opts o;
        memset(&o, 0xA5, sizeof o);
        const int a = mcrt_default_render_opts(&o, 0), b = mcrt_default_render_opts(nullptr, 1);
        printf("opts.defaults: %d %d mode %u window %g %g\n", a, b, o.mode, (double)o.lo, (double)o.hi);
    }
    printf("DONE\n");
    return 0;
}
