// mcrt_host.hpp -- C++ host side above the C-ABI (include/mcrt.h), mirroring the reference's interface for the hot
// path: same class names, argument meaning and error behaviour, so a program written against the reference's
// `scene` / `transducer<N>` / `psf<...>` / `rf_image<...>` reads the same (namespace mcrt_host).
//
//   transducer<N>            transducer.h:24-137   (frequency MHz, radius cm, element separation mm, position, angles deg)
//   psf<ax,lat,elev,res>     psf.h:34-77
//   scene                    scene.h:19-76, scene.cpp:16-48,185-247 (JSON keys, "Error while loading scene: ..." wrapping)
//   rf_image<cols,us,um>     rfimage.h:20-219      (clear / convolve / envelope / postprocess; data lives on the GPU); + detect / iq; + flow_split / flow / colour_flow; + spectral_series / spectrum / sonogram; + compress / track / elastogram; + shear_wave / shear_speed / shear_elastogram; + m_lines / m_mode
//   ray_physics::segment     ray.h:28-36           (vec3 stands in for btVector3; `media` is held BY VALUE: the reference's
//                                                   `const material &` dangles by the time main.cpp:126 reads it)
//   volume<size,res>         volume.h:19-61        (host copy of the texture the GPU samples)
//
// Units are plain doubles (the reference's units.h types are compile-time only); names say the unit.
#pragma once
#include <mcrt.h>

#include <array>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace mcrt_host {

inline void check(int rc, const char *what)
{
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + mcrt_last_error());
}

// ---------------------------------------------------------------- minimal JSON (objects, arrays, strings, numbers, bools)
struct json {
    enum kind_t { null_k, bool_k, num_k, str_k, arr_k, obj_k } kind = null_k;
    bool b = false; double num = 0; std::string str; std::vector<json> arr; std::vector<std::pair<std::string, json>> obj;

    const json &at(const std::string &key) const   // nlohmann::json::at semantics: throws when absent
    {
        for (auto &kv : obj) if (kv.first == key) return kv.second;
        throw std::out_of_range("key '" + key + "' not found");
    }
    bool contains(const std::string &key) const { for (auto &kv : obj) if (kv.first == key) return true; return false; }
    const json &operator[](size_t i) const { return arr.at(i); }
    bool is_array() const { return kind == arr_k; }
    operator double() const { if (kind != num_k) throw std::domain_error("type must be number"); return num; }
    operator float() const { return (float)(double)*this; }
    operator bool() const { if (kind != bool_k) throw std::domain_error("type must be boolean"); return b; }
    operator std::string() const { if (kind != str_k) throw std::domain_error("type must be string"); return str; }

    static json parse(const std::string &s) { size_t i = 0; json j = value(s, i, 0); ws(s, i); if (i != s.size()) fail("trailing characters", i); return j; }

    static constexpr int max_depth = 256;      // nesting the recursive descent accepts (a scene file nests 3 deep); deeper input is a parse error, not a stack overflow

private:
    static void fail(const char *m, size_t i) { throw std::invalid_argument("parse error at " + std::to_string(i) + ": " + m); }
    static void ws(const std::string &s, size_t &i) { while (i < s.size() && (s[i] == ' ' || s[i] == '\t' || s[i] == '\n' || s[i] == '\r')) i++; }
    static unsigned hex4(const std::string &s, size_t &i)      // the four hex digits after \u; i is left on the last one
    {
        if (i + 4 >= s.size()) fail("truncated \\u escape", i);
        unsigned v = 0;
        for (int k = 1; k <= 4; k++) {
            const char h = s[i + (size_t)k];
            v = v * 16u + (h >= '0' && h <= '9' ? (unsigned)(h - '0') : h >= 'a' && h <= 'f' ? (unsigned)(h - 'a' + 10) : h >= 'A' && h <= 'F' ? (unsigned)(h - 'A' + 10) : (fail("bad hex digit in \\u escape", i + (size_t)k), 0u));
        }
        i += 4;
        return v;
    }
    static void utf8(std::string &o, unsigned cp)
    {
        if (cp < 0x80) o += (char)cp;
        else if (cp < 0x800) { o += (char)(0xC0 | (cp >> 6)); o += (char)(0x80 | (cp & 0x3F)); }
        else if (cp < 0x10000) { o += (char)(0xE0 | (cp >> 12)); o += (char)(0x80 | ((cp >> 6) & 0x3F)); o += (char)(0x80 | (cp & 0x3F)); }
        else { o += (char)(0xF0 | (cp >> 18)); o += (char)(0x80 | ((cp >> 12) & 0x3F)); o += (char)(0x80 | ((cp >> 6) & 0x3F)); o += (char)(0x80 | (cp & 0x3F)); }
    }
    static json value(const std::string &s, size_t &i, int depth)
    {
        if (depth > max_depth) fail("nested too deeply", i);
        ws(s, i);
        if (i >= s.size()) fail("unexpected end", i);
        json j;
        const char c = s[i];
        if (c == '{') {
            j.kind = obj_k; i++; ws(s, i);
            if (i < s.size() && s[i] == '}') { i++; return j; }
            for (;;) {
                ws(s, i);
                json k = value(s, i, depth + 1);
                if (k.kind != str_k) fail("object key must be a string", i);
                ws(s, i);
                if (i >= s.size() || s[i] != ':') fail("expected ':'", i);
                i++;
                j.obj.emplace_back(k.str, value(s, i, depth + 1));
                ws(s, i);
                if (i < s.size() && s[i] == ',') { i++; continue; }
                if (i < s.size() && s[i] == '}') { i++; return j; }
                fail("expected ',' or '}'", i);
            }
        }
        if (c == '[') {
            j.kind = arr_k; i++; ws(s, i);
            if (i < s.size() && s[i] == ']') { i++; return j; }
            for (;;) {
                j.arr.push_back(value(s, i, depth + 1));
                ws(s, i);
                if (i < s.size() && s[i] == ',') { i++; continue; }
                if (i < s.size() && s[i] == ']') { i++; return j; }
                fail("expected ',' or ']'", i);
            }
        }
        if (c == '"') {
            j.kind = str_k; i++;
            while (i < s.size() && s[i] != '"') {
                if ((unsigned char)s[i] < 0x20) fail("control character in string", i);
                if (s[i] == '\\') {
                    if (i + 1 >= s.size()) fail("unterminated string", i);
                    const char e = s[++i];
                    switch (e) {
                    case '"': case '\\': case '/': j.str += e; break;
                    case 'b': j.str += '\b'; break; case 'f': j.str += '\f'; break; case 'n': j.str += '\n'; break;
                    case 'r': j.str += '\r'; break; case 't': j.str += '\t'; break;
                    case 'u': {
                        unsigned cp = hex4(s, i);
                        if (cp >= 0xD800 && cp <= 0xDBFF) {                      // a surrogate pair: the low half must follow
                            if (i + 2 >= s.size() || s[i + 1] != '\\' || s[i + 2] != 'u') fail("lone surrogate in \\u escape", i);
                            i += 2;
                            const unsigned lo = hex4(s, i);
                            if (lo < 0xDC00 || lo > 0xDFFF) fail("bad low surrogate in \\u escape", i);
                            cp = 0x10000u + ((cp - 0xD800u) << 10) + (lo - 0xDC00u);
                        } else if (cp >= 0xDC00 && cp <= 0xDFFF) fail("lone surrogate in \\u escape", i);
                        utf8(j.str, cp);
                        break;
                    }
                    default: fail("bad escape", i);
                    }
                } else j.str += s[i];
                i++;
            }
            if (i >= s.size()) fail("unterminated string", i);
            i++;
            return j;
        }
        if (!s.compare(i, 4, "true")) { j.kind = bool_k; j.b = true; i += 4; return j; }
        if (!s.compare(i, 5, "false")) { j.kind = bool_k; j.b = false; i += 5; return j; }
        if (!s.compare(i, 4, "null")) { i += 4; return j; }
        {   // a JSON number: -? digits ...  (strtod alone would take "nan", "inf", hex floats and a leading '+')
            const size_t d = i + (c == '-' ? 1u : 0u);
            if (d >= s.size() || !(s[d] >= '0' && s[d] <= '9')) fail("unexpected character", i);
            if (s[d] == '0' && d + 1 < s.size() && ((s[d + 1] >= '0' && s[d + 1] <= '9') || s[d + 1] == 'x' || s[d + 1] == 'X')) fail("bad number", i);
        }
        char *end = nullptr;
        j.num = std::strtod(s.c_str() + i, &end);
        if (end == s.c_str() + i) fail("unexpected character", i);
        j.kind = num_k; i = (size_t)(end - s.c_str());
        return j;
    }
};

inline json load_json(const std::string &path)
{
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::stringstream ss; ss << f.rdbuf();
    return json::parse(ss.str());
}

// ---------------------------------------------------------------- meshes (mesh.h:7-20) and OBJ triangles (objloader.h:28-139: positions, face order, fans)
struct material { float impedance, attenuation, mu0, mu1, sigma, specularity, shininess, thickness; };
struct mesh { std::string filename; bool is_rigid, is_vascular; std::array<float, 3> deltas; bool outside_normals; uint32_t material_inside, material_outside; };

// positions and faces the way the reference's loader reads them (tiny_obj_loader.cpp:97-187,504-717): a coordinate is (float)atof of its token
// (so "nan" and "inf" are values, a missing coordinate is 0), a face corner is atoi of the token up to its first '/', index > 0 counts from one,
// < 0 from the end, and 0 is the first vertex (fixIndex); polygons become fans.  The reference then indexes its arrays unchecked: a corner
// outside the vertices read so far is an error here, never a wild read.
inline void load_obj_triangles(std::istream &f, const std::string &name, std::vector<float> &tri9)
{
    std::vector<std::array<float, 3>> v;
    std::string line;
    while (std::getline(f, line)) {
        const char *t = line.c_str();
        t += std::strspn(t, " \t");
        if (t[0] == 'v' && (t[1] == ' ' || t[1] == '\t')) {
            t += 2;
            std::array<float, 3> p{};
            for (int k = 0; k < 3; k++) { t += std::strspn(t, " \t"); p[(size_t)k] = (float)std::atof(t); t += std::strcspn(t, " \t\r"); }
            v.push_back(p);
        } else if (t[0] == 'f' && (t[1] == ' ' || t[1] == '\t')) {
            t += 2;
            std::vector<long> idx;
            for (;;) {
                t += std::strspn(t, " \t");
                if (t[0] == '\0' || t[0] == '\r' || t[0] == '\n') break;
                const long i = std::strtol(t, nullptr, 10);            // stops at '/': the position index of v, v/vt, v//vn, v/vt/vn
                idx.push_back(i > 0 ? i - 1 : i == 0 ? 0 : (long)v.size() + i);
                t += std::strcspn(t, " \t\r");
            }
            for (size_t k = 1; k + 1 < idx.size(); k++)
                for (long i : { idx[0], idx[k], idx[k + 1] }) {
                    if (i < 0 || (size_t)i >= v.size()) throw std::runtime_error("face index out of range in '" + name + "'");
                    tri9.insert(tri9.end(), v[(size_t)i].begin(), v[(size_t)i].end());
                }
        }
    }
}
inline void load_obj_triangles(const std::string &path, std::vector<float> &tri9)
{
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot read mesh '" + path + "'");
    load_obj_triangles(f, path, tri9);
}

// the subset of btVector3 the reference's host code uses (main.cpp:72,117,120,131; scene.cpp:342-346)
struct vec3 {
    float v[3] = { 0, 0, 0 };
    vec3() = default;
    vec3(float x, float y, float z) : v{ x, y, z } {}
    float x() const { return v[0]; } float y() const { return v[1]; } float z() const { return v[2]; }
    vec3 operator+(const vec3 &o) const { return { v[0] + o.v[0], v[1] + o.v[1], v[2] + o.v[2] }; }
    vec3 operator-(const vec3 &o) const { return { v[0] - o.v[0], v[1] - o.v[1], v[2] - o.v[2] }; }
    vec3 &operator+=(const vec3 &o) { v[0] += o.v[0]; v[1] += o.v[1]; v[2] += o.v[2]; return *this; }
    float dot(const vec3 &o) const { return v[0] * o.v[0] + v[1] * o.v[1] + v[2] * o.v[2]; }
    float length() const { return std::sqrt(dot(*this)); }
    float distance(const vec3 &o) const { return (o - *this).length(); }
};
inline vec3 operator*(float s, const vec3 &a) { return { s * a.v[0], s * a.v[1], s * a.v[2] }; }
inline vec3 operator*(const vec3 &a, float s) { return s * a; }

namespace ray_physics {
struct segment {   // ray.h:28-36
    vec3 from, to, direction;
    float reflected_intensity;   // reflected back to the transducer, at the end of the segment
    float initial_intensity, attenuation;
    double distance_traveled;    // [mm] traveled from the transducer to the beginning of the segment
    material media;              // by value (see the header comment)
    int32_t tri;                 // triangle hit at the end of the segment (-1 none): not in the reference, free with the GPU walk
};
}  // namespace ray_physics

// ---------------------------------------------------------------- transducer<N> (transducer.h)
template <size_t transducer_elements>
class transducer {
public:
    struct transducer_element { vec3 position, direction; };

    // transducer.h:24-62 (frequency MHz, radius cm, element separation mm, position in scene units, angles in degrees)
    transducer(float frequency_mhz, double radius_cm, double element_separation_mm, const vec3 &position, const std::array<float, 3> &angles_deg)
        : frequency(frequency_mhz), position(position), angles(angles_deg), radius_cm(radius_cm), separation_mm(element_separation_mm)
    {
        if (!(element_separation_mm * transducer_elements < 3.14159 * radius_cm * 10.0))      // the assert of transducer.h:35
            throw std::invalid_argument("transducer: elements do not fit on the arc");
        update();
    }
    void update()   // transducer.h:82-118: the elements from the current position and angles
    {
        pos.resize(3 * transducer_elements); dir.resize(3 * transducer_elements);
        check(mcrt_transducer_elements((uint32_t)transducer_elements, radius_cm, separation_mm, position.v, angles.data(), pos.data(), dir.data()), "transducer");
    }
    transducer_element element(size_t i) const   // transducer.h:64-67 (std::array::at: throws when out of range)
    {
        if (i >= transducer_elements) throw std::out_of_range("transducer::element");
        return { vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), vec3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]) };
    }
    void print(bool direction) const   // transducer.h:69-80: "x,z" per element
    {
        for (size_t i = 0; i < transducer_elements; i++) {
            const auto e = element(i);
            const vec3 &v = direction ? e.direction : e.position;
            std::cout << v.x() << "," << v.z() << std::endl;
        }
    }
    // slice thickness: the element tables of n_planes parallel elevation planes pitch_um apart, centred on the probe's own plane
    // (mcrt_elevation_planes along mcrt_transducer_elevation_axis): pos / dir [K][N][3], z_mm [K]
    struct plane_tables { std::vector<float> pos, dir, z_mm; };
    plane_tables planes(uint32_t n_planes, uint32_t pitch_um) const
    {
        float axis[3];
        check(mcrt_transducer_elevation_axis(angles.data(), axis), "transducer elevation axis");
        plane_tables t;
        const size_t K = n_planes >= 1 && n_planes <= 32 ? n_planes : 1;      // (the library refuses other counts before it writes)
        t.pos.resize(K * 3 * transducer_elements); t.dir.resize(K * 3 * transducer_elements); t.z_mm.resize(K);
        check(mcrt_elevation_planes(pos.data(), dir.data(), (uint32_t)transducer_elements, axis, n_planes, pitch_um, t.pos.data(), t.dir.data(), t.z_mm.data()), "transducer planes");
        return t;
    }
    // spatial compounding: the element tables of the views of a compounded frame, one per in-plane steering angle [rad]
    // (mcrt_transducer_steered: the beams pivot on their elements): pos / dir [views][N][3]; z_mm stays empty
    plane_tables steered(const std::vector<float> &steer_rad) const
    {
        plane_tables t;
        const size_t one = 3 * transducer_elements;
        t.pos.resize(steer_rad.size() * one); t.dir.resize(steer_rad.size() * one);
        for (size_t n = 0; n < steer_rad.size(); n++)
            check(mcrt_transducer_steered((uint32_t)transducer_elements, radius_cm, separation_mm, position.v, angles.data(), steer_rad[n], t.pos.data() + n * one,
                                          t.dir.data() + n * one), "transducer steered");
        return t;
    }
    // volume imaging: the element tables of the planes of a sweep (mcrt_transducer_swept at theta_k = (k - (K-1)/2.0) * step_rad, the array
    // tilted about the line parallel to x through (0, pivot_mm, 0) of the probe-local frame): pos / dir [K][N][3]; z_mm stays empty
    plane_tables swept(const mcrt_sweep &sw) const
    {
        plane_tables t;
        const size_t one = 3 * transducer_elements;
        t.pos.resize(sw.n_planes * one); t.dir.resize(sw.n_planes * one);
        for (uint32_t k = 0; k < sw.n_planes; k++) {
            const float tilt = (float)(((double)k - (double)(sw.n_planes - 1u) / 2.0) * (double)sw.step_rad);
            check(mcrt_transducer_swept((uint32_t)transducer_elements, radius_cm, separation_mm, position.v, angles.data(), tilt, sw.pivot_mm, t.pos.data() + k * one,
                                        t.dir.data() + k * one), "transducer swept");
        }
        return t;
    }
    // freehand 3-D: the element tables of a hand-held sweep of n_frames frames -- the probe translated along its elevation axis
    // (mcrt_transducer_elevation_axis) in steps of step_mm centred on its own pose, step k tilted by (k - (n-1)/2) * fan_deg about the line
    // through the arc's apex (mcrt_transducer_swept with the pivot at the radius): pos / dir [n_frames][N][3]; z_mm the offsets [mm]
    plane_tables freehand(uint32_t n_frames, double step_mm, double fan_deg = 0.0) const
    {
        float axis[3];
        check(mcrt_transducer_elevation_axis(angles.data(), axis), "transducer elevation axis");
        plane_tables t;
        const size_t one = 3 * transducer_elements;
        t.pos.resize(n_frames * one); t.dir.resize(n_frames * one); t.z_mm.resize(n_frames);
        for (uint32_t k = 0; k < n_frames; k++) {
            const double kk = (double)k - (double)(n_frames - 1u) / 2.0;
            const float s = (float)(kk * step_mm / 10.0), tilt = (float)(kk * fan_deg * 3.14159265358979323846 / 180.0);
            float p[3];
            for (int i = 0; i < 3; i++) { const float d = axis[i] * s; p[i] = position.v[i] + d; }
            t.z_mm[k] = (float)(kk * step_mm);
            check(mcrt_transducer_swept((uint32_t)transducer_elements, radius_cm, separation_mm, p, angles.data(), tilt, (float)(radius_cm * 10.0), t.pos.data() + k * one,
                                        t.dir.data() + k * one), "transducer freehand");
        }
        return t;
    }
    void setPosition(const vec3 &p) { position = p; }
    void setAngles(const std::array<float, 3> &a) { angles = a; }
    vec3 getPosition() const { return position; }
    static constexpr size_t size() { return transducer_elements; }

    const float frequency;
    vec3 position, direction;
    std::array<float, 3> angles;
    std::vector<float> pos, dir;          // [N][3] each, what mcrt_set_transducer takes
private:
    const double radius_cm, separation_mm;
};

// ---------------------------------------------------------------- psf (psf.h)
template <size_t axial_size, size_t lateral_size, size_t elevation_size, unsigned int resolution_micrometers>
class psf {
    static_assert(axial_size % 2 && lateral_size % 2 && elevation_size % 2, "kernel sizes must be odd");
public:
    psf(float freq, float var_x, float var_y, float var_z) : var_y(var_y), var_z(var_z)
    {
        check(mcrt_psf_kernels(freq, var_x, var_y, resolution_micrometers, axial_kernel.data(), axial_size, lateral_kernel.data(), lateral_size), "psf");
        // psf.h:42,77: the constant elevation kernel exp(-z_k^2 / (2 var_z)) at the plane positions of mcrt_elevation_planes, unnormalised as the
        // lateral taps are (a var_z the model refuses leaves it zero, as the reference leaves it: only elevation_rows() then fails)
        if (var_z > 0.0f && std::isfinite(var_z) && elevation_size <= 32)
            check(mcrt_psf_elevation_kernels(var_z, resolution_micrometers, nullptr, 1, 1.0, 0, elevation_kernel.data(), (uint32_t)elevation_size), "psf elevation");
    }
    // slice thickness (psf.h:16-18,42,77; the model in mcrt.h): the pitch of the elevation planes [um] (default: resolution_micrometers), whether
    // every row of weights is divided by its sum, and an optional elevation focus (a lens has one) away from which the slice thickens.
    // elevation_kernel is refilled for the new pitch.
    void set_elevation(uint32_t pitch_um, bool normalize = true, const float *focus_mm = nullptr, uint32_t n = 0, float focal_range_mm = 20.0f)
    {
        elev_pitch_um = pitch_um; elev_normalize = normalize;
        elev_focus = mcrt_focus{};
        elev_focus.n_focus = focus_mm ? n : 0u;
        for (uint32_t i = 0; i < elev_focus.n_focus && i < 8; i++) elev_focus.focus_mm[i] = focus_mm[i];
        elev_focus.focal_range_mm = focal_range_mm;
        elev_table.clear(); elev_rows = 0;
        check(mcrt_psf_elevation_kernels(var_z, pitch_um, nullptr, 1, 1.0, 0, elevation_kernel.data(), (uint32_t)elevation_size), "psf elevation");
    }
    uint32_t elevation_pitch_um() const { return elev_pitch_um; }
    // the elevation weights of every RF row [n_rows][n_planes] for rows row_mm apart (n_planes = 0: elevation_size); made once per shape
    const std::vector<float> &elevation_rows(uint32_t n_rows, double row_mm, uint32_t n_planes = 0) const
    {
        const uint32_t K = n_planes ? n_planes : (uint32_t)elevation_size;
        if (elev_table.empty() || elev_rows != n_rows || elev_row_mm != row_mm || elev_planes != K) {
            std::vector<float> t((size_t)n_rows * K);
            check(mcrt_psf_elevation_kernels(var_z, elev_pitch_um, &elev_focus, n_rows, row_mm, elev_normalize ? 1 : 0, t.data(), K), "psf elevation");
            elev_table = std::move(t); elev_rows = n_rows; elev_row_mm = row_mm; elev_planes = K;
        }
        return elev_table;
    }
    // focal zones (psf.h:17-24 plans them): up to 8 ascending focal depths [mm]; rf_image::convolve then gives every RF row its own lateral
    // taps (mcrt_psf_focus_kernels, the model in mcrt.h).  n = 0 goes back to the reference's one constant kernel.  focal_range_mm = 20 is
    // a display choice that no measurement backs.  The foci are checked when the table is made (by the first convolve).
    void set_focus(const float *focus_mm, uint32_t n, float focal_range_mm = 20.0f)
    {
        focus = mcrt_focus{};
        focus.n_focus = n;
        for (uint32_t i = 0; i < n && i < 8; i++) focus.focus_mm[i] = focus_mm[i];
        focus.focal_range_mm = focal_range_mm;
        table.clear(); table_rows = 0;
    }
    bool has_focus() const { return focus.n_focus > 0; }
    // the lateral taps of every RF row [n_rows][lateral_size] for rows row_mm apart; made once per (n_rows, row_mm)
    const std::vector<float> &lateral_rows(uint32_t n_rows, double row_mm) const
    {
        if (table.empty() || table_rows != n_rows || table_row_mm != row_mm) {
            std::vector<float> t((size_t)n_rows * lateral_size);
            check(mcrt_psf_focus_kernels(var_y, resolution_micrometers, &focus, n_rows, row_mm, t.data(), (uint32_t)lateral_size), "psf focus");
            table = std::move(t); table_rows = n_rows; table_row_mm = row_mm;
        }
        return table;
    }
    // frequency compounding and the depth downshift (the model in mcrt.h): the received band split into b.n_bands sub-bands, each with an axial
    // kernel of its own per RF row (mcrt_psf_band_kernels; b.var_x is the bands' own axial variance).  rf_image::convolve then writes a band
    // stack, add_noise acts on it and envelope() detects every band image and folds them back.  A downshift has no default that the reference
    // backs: a value is the caller's choice.  The struct is checked when the tables are made (by the first convolve).
    void set_bands(const mcrt_bands &b) { band = b; with_bands = true; band_table.clear(); band_rows = 0; }
    bool has_bands() const { return with_bands; }
    uint32_t n_bands() const { return with_bands ? band.n_bands : 0u; }
    // the axial taps of every band and RF row [B][n_rows][axial_size] for rows row_mm apart, and the bands' weights [n_rows][B]; made once per
    // (n_rows, row_mm)
    const std::vector<float> &axial_rows(uint32_t n_rows, double row_mm) const { band_tables(n_rows, row_mm); return band_table; }
    const std::vector<float> &band_weights(uint32_t n_rows, double row_mm) const { band_tables(n_rows, row_mm); return band_wtable; }
    constexpr size_t get_axial_size() const { return axial_size; }
    constexpr size_t get_lateral_size() const { return lateral_size; }
    constexpr size_t get_elevation_size() const { return elevation_size; }
    std::array<float, axial_size> axial_kernel;
    std::array<float, lateral_size> lateral_kernel;
    std::array<float, elevation_size> elevation_kernel{};   // declared and never filled in the reference (psf.h:77); here the constant elevation kernel
    float var_y, var_z;
private:
    mcrt_focus focus{};
    mutable std::vector<float> table; mutable uint32_t table_rows = 0; mutable double table_row_mm = 0.0;
    mcrt_focus elev_focus{}; uint32_t elev_pitch_um = resolution_micrometers; bool elev_normalize = true;
    mutable std::vector<float> elev_table; mutable uint32_t elev_rows = 0, elev_planes = 0; mutable double elev_row_mm = 0.0;
    mcrt_bands band{}; bool with_bands = false;
    mutable std::vector<float> band_table, band_wtable; mutable uint32_t band_rows = 0; mutable double band_row_mm = 0.0;
    void band_tables(uint32_t n_rows, double row_mm) const
    {
        if (!band_table.empty() && band_rows == n_rows && band_row_mm == row_mm) return;
        const uint32_t B = band.n_bands >= 1 && band.n_bands <= 8 ? band.n_bands : 1u;     // (any other count is refused below: the size only has to exist)
        std::vector<float> t((size_t)B * n_rows * axial_size), w((size_t)n_rows * B);
        check(mcrt_psf_band_kernels(&band, resolution_micrometers, n_rows, row_mm, t.data(), (uint32_t)axial_size, w.data()), "psf bands");
        band_table = std::move(t); band_wtable = std::move(w); band_rows = n_rows; band_row_mm = row_mm;
    }
};

// ---------------------------------------------------------------- GPU context shared by scene and rf_image
// One GPU (mcrt_ctx), or several behind the same objects (mcrt_group: scan-line shards, blocks gathered on the first device; a
// device may be listed more than once).  `ctx` is the context the images live on -- the group's root -- in either case.
struct device {
    explicit device(int id = 0) { check(mcrt_create(id, &ctx), "mcrt_create"); }
    explicit device(const std::vector<int> &ids)
    {
        if (ids.size() == 1) { check(mcrt_create(ids[0], &ctx), "mcrt_create"); return; }
        check(mcrt_group_create(ids.data(), (uint32_t)ids.size(), &group), "mcrt_group_create");
        ctx = mcrt_group_root(group);
    }
    ~device() { if (group) mcrt_group_destroy(group); else mcrt_destroy(ctx); }
    device(const device &) = delete; device &operator=(const device &) = delete;
    mcrt_ctx *tracer() const { return group ? mcrt_group_member(group, 0) : ctx; }      // for calls on one shard (scene::cast_rays)
    // the set-up and trace calls, on the one context or on every rank of the group
    int set_params(const mcrt_params *p) { return group ? mcrt_group_set_params(group, p) : mcrt_set_params(ctx, p); }
    int upload_scene(const float *tri, const uint32_t *tri_mesh, uint32_t n_tri, const mcrt_mesh *meshes, uint32_t n_mesh, const float *mats, uint32_t n_mat, uint32_t start_mat, const float *spacing)
    {
        return group ? mcrt_group_upload_scene(group, tri, tri_mesh, n_tri, meshes, n_mesh, mats, n_mat, start_mat, spacing)
                     : mcrt_upload_scene(ctx, tri, tri_mesh, n_tri, meshes, n_mesh, mats, n_mat, start_mat, spacing);
    }
    int upload_texture(const float *vox, uint32_t n) { return group ? mcrt_group_upload_texture(group, vox, n) : mcrt_upload_texture(ctx, vox, n); }
    int set_transducer(const float *pos, const float *dir, uint32_t n) { return group ? mcrt_group_set_transducer(group, pos, dir, n) : mcrt_set_transducer(ctx, pos, dir, n); }
    int trace_frames(uint32_t frame, uint32_t n_frames, uint32_t columns, float *rf_dev)
    {
        return group ? mcrt_group_trace_frames(group, frame, n_frames, rf_dev) : mcrt_trace_frames(ctx, frame, n_frames, 0, columns, rf_dev);
    }
    int trace_frames_poses(uint32_t frame, uint32_t n_frames, uint32_t columns, const float *pos, const float *dir, float *rf_dev)   // host tables [n_frames][columns][3]
    {
        return group ? mcrt_group_trace_frames_poses(group, frame, n_frames, pos, dir, rf_dev) : mcrt_trace_frames_poses(ctx, frame, n_frames, 0, columns, pos, dir, rf_dev);
    }
    int synchronize() { return group ? mcrt_group_synchronize(group) : mcrt_synchronize(ctx); }
    mcrt_ctx *ctx = nullptr;
    mcrt_group *group = nullptr;
};
// the reference's objects take no device argument: they share this process-wide one (GPU 0), created on first use
inline std::shared_ptr<device> default_device()
{
    static std::weak_ptr<device> weak;
    auto d = weak.lock();
    if (!d) { d = std::make_shared<device>(0); weak = d; }
    return d;
}

// ---------------------------------------------------------------- volume (volume.h): host copy of the tissue texture
template <unsigned int size, unsigned int resolution_micrometers>
class volume {
public:
    volume() : matrix((size_t)size * size * size * 2) { check(mcrt_generate_texture(matrix.data(), size), "mcrt_generate_texture"); }   // volume.h:19-35
    constexpr float get_resolution_in_millis() const { return static_cast<float>(resolution_micrometers) / 1000.0f; }
    // volume.h:46-61 (float -> unsigned of a negative coordinate wraps like x86-64: DESIGN.md, quirk 4)
    float get_scattering(const float scattering_density, const float scattering_mu, const float scattering_sigma,
                         const float x_millis, const float y_millis, const float z_millis) const
    {
        constexpr float resolution = resolution_micrometers / 1000.0f;
        const unsigned int x = index(x_millis / resolution), y = index(y_millis / resolution), z = index(z_millis / resolution);
        const float *voxel = &matrix[2 * (((size_t)x * size + y) * size + z)];     // { texture_noise, scattering_probability }
        return voxel[1] >= scattering_density ? voxel[0] * scattering_sigma + scattering_mu : 0.0f;
    }
    const float *data() const { return matrix.data(); }
private:
    static unsigned int index(float q)
    {
        long long i = std::fabs(q) < 9.2233720368547758e18f ? (long long)q : (long long)0x8000000000000000ull;
        return (unsigned int)i % size;
    }
    std::vector<float> matrix;
};

// ---------------------------------------------------------------- scene (scene.h / scene.cpp)
// what scene::parse_config (scene.cpp:185-247) reads of a scene file -- host data only, no GPU: every key but workingDirectory is mandatory
// (nlohmann::json::at throws), and load() wraps any failure the way the reference's constructor does (scene.cpp:19-26)
struct scene_config {
    std::vector<std::string> material_names;
    std::vector<material> materials;
    std::vector<mesh> meshes;
    std::string working_dir, starting_material;
    std::array<float, 3> spacing{}, origin{};
    float scaling = 1.f;

    static scene_config load(const json &config)
    {
        scene_config c;
        try { c.parse_config(config); }
        catch (const std::exception &ex) { throw std::runtime_error{ "Error while loading scene: " + std::string{ ex.what() } }; }
        return c;
    }
    uint32_t material_index(const std::string &name) const
    {
        for (size_t i = 0; i < material_names.size(); i++) if (material_names[i] == name) return (uint32_t)i;
        throw std::out_of_range("key '" + name + "' not found");
    }
    // scene.cpp:38-48 + 300-334: each mesh's OBJ, placed; the triangle soup mcrt_upload_scene takes
    void triangles(std::vector<float> &tri, std::vector<uint32_t> &tri_mesh, std::vector<mcrt_mesh> &recs) const
    {
        for (size_t mi = 0; mi < meshes.size(); mi++) {
            const mesh &m = meshes[mi];
            std::vector<float> t9;
            load_obj_triangles(working_dir + m.filename, t9);
            float pos[3];
            for (int i = 0; i < 3; i++) pos[i] = m.deltas[(size_t)i] * scaling * scaling + origin[(size_t)i];   // scene.cpp:322-324
            for (size_t k = 0; k < t9.size(); k++) t9[k] = t9[k] * scaling + pos[k % 3];
            tri.insert(tri.end(), t9.begin(), t9.end());
            tri_mesh.insert(tri_mesh.end(), t9.size() / 9, (uint32_t)mi);
            recs.push_back(mcrt_mesh{ m.material_inside, m.material_outside, m.is_vascular ? 1u : 0u, 0u });
        }
    }
private:
    static std::array<float, 3> float3(const json &a)
    {
        if (!a.is_array()) throw std::domain_error("type must be array");
        return { (float)a[0], (float)a[1], (float)a[2] };
    }
    void parse_config(const json &config)   // scene.cpp:185-247
    {
        working_dir = config.contains("workingDirectory") ? (std::string)config.at("workingDirectory") : "";
        (void)config.at("transducerPosition");
        origin = float3(config.at("origin"));
        spacing = float3(config.at("spacing"));
        starting_material = (std::string)config.at("startingMaterial");
        scaling = (float)config.at("scaling");
        const auto &mats = config.at("materials");
        if (!mats.is_array()) throw std::runtime_error("materials must be an array");
        for (const auto &m : mats.arr) {
            const std::string name = m.at("name");
            material v{ m.at("impedance"), m.at("attenuation"), m.at("mu0"), m.at("mu1"), m.at("sigma"), m.at("specularity"), m.at("shininess"), m.at("thickness") };
            bool found = false;
            for (size_t i = 0; i < material_names.size(); i++) if (material_names[i] == name) { materials[i] = v; found = true; }
            if (!found) { material_names.push_back(name); materials.push_back(v); }
        }
        const auto &ms = config.at("meshes");
        if (!ms.is_array()) throw std::runtime_error("meshes must be an array");
        for (const auto &m : ms.arr) {
            // (every field into a local first: an initializer that throws half way through a braced aggregate leaks the fields already built
            //  under GCC < 12 -- found by the sanitizer run, tests/test_host_sanitize.py)
            const std::string file = m.at("file");
            const bool rigid = m.at("rigid"), vascular = m.at("vascular"), outside_normals = m.at("outsideNormals");
            const std::array<float, 3> deltas = float3(m.at("deltas"));
            const uint32_t inside = material_index(m.at("material")), outside = material_index(m.at("outsideMaterial"));
            meshes.push_back(mesh{ file, rigid, vascular, deltas, outside_normals, inside, outside });
        }
        (void)material_index(starting_material);
    }
};

class scene : public scene_config {
public:
    // scene(json, transducer&): parse_config + upload (replaces create_empty_world/init/add_rigidbody_from_obj)
    template <size_t N>
    scene(const json &config, transducer<N> &t, std::shared_ptr<device> dev_ = nullptr, unsigned samples = 5, unsigned seed = 0x5EED)
        : scene_config(scene_config::load(config)), dev(dev_ ? std::move(dev_) : default_device())
    {
        mcrt_params p; mcrt_default_params(&p);
        p.n_elements = (uint32_t)N; p.n_samples = samples; p.frequency = t.frequency; p.seed = seed;
        check(this->dev->set_params(&p), "mcrt_set_params");
        params = p;
        init();
        check(this->dev->upload_texture(nullptr, p.tex_n), "mcrt_upload_texture");     // static volume_ texture_volume (main.cpp:52)
        set_transducer(t);
    }

    template <size_t N> void set_transducer(const transducer<N> &t) { check(dev->set_transducer(t.pos.data(), t.dir.data(), (uint32_t)N), "mcrt_set_transducer"); }

    // scene::cast_rays<sample_count, ray_count>(transducer) (scene.h:29-30, scene.cpp:50-183): the segments of every
    // (element, sample) path, traced on the GPU.  The reference draws fresh random numbers on every call (random_device);
    // here every call advances the frame id of the counter-based generator.
    template <unsigned int sample_count, unsigned int ray_count, size_t N>
    std::array<std::array<std::vector<ray_physics::segment>, sample_count>, ray_count> cast_rays(transducer<N> &t)
    {
        static_assert(ray_count == N, "one ray bundle per transducer element");
        if (params.n_samples != sample_count || params.n_elements != ray_count) {
            check(mcrt_get_params(dev->ctx, &params), "mcrt_get_params");
            params.n_samples = sample_count; params.n_elements = ray_count;
            check(dev->set_params(&params), "mcrt_set_params");
        }
        set_transducer(t);
        const size_t B = params.max_depth;
        std::vector<mcrt_segment> flat((size_t)ray_count * sample_count * B); std::vector<uint32_t> cnt((size_t)ray_count * sample_count);
        check(mcrt_cast_rays(dev->tracer(), frame_id++, 0, ray_count, flat.data(), cnt.data(), nullptr), "mcrt_cast_rays");
        std::array<std::array<std::vector<ray_physics::segment>, sample_count>, ray_count> out;
        for (size_t e = 0; e < ray_count; e++)
            for (size_t s = 0; s < sample_count; s++) {
                const size_t p = e * sample_count + s;
                auto &dst = out[e][s];
                dst.reserve(cnt[p]);
                for (uint32_t b = 0; b < cnt[p]; b++) {
                    const mcrt_segment &g = flat[p * B + b];
                    dst.push_back(ray_physics::segment{ vec3(g.from[0], g.from[1], g.from[2]), vec3(g.to[0], g.to[1], g.to[2]), vec3(g.dir[0], g.dir[1], g.dir[2]),
                                                        g.reflected_intensity, g.initial_intensity, g.attenuation, g.distance_traveled, materials[(size_t)g.media], g.tri });
                }
            }
        return out;
    }
    // the flat form of the same call, for a given frame id
    std::vector<std::vector<std::vector<mcrt_segment>>> cast_rays(uint32_t frame)
    {
        const size_t E = params.n_elements, S = params.n_samples, B = params.max_depth;
        std::vector<mcrt_segment> flat(E * S * B); std::vector<uint32_t> cnt(E * S);
        check(mcrt_cast_rays(dev->tracer(), frame, 0, (uint32_t)E, flat.data(), cnt.data(), nullptr), "mcrt_cast_rays");
        std::vector<std::vector<std::vector<mcrt_segment>>> out(E, std::vector<std::vector<mcrt_segment>>(S));
        for (size_t e = 0; e < E; e++)
            for (size_t s = 0; s < S; s++) {
                const size_t p = e * S + s;
                out[e][s].assign(flat.begin() + (long)(p * B), flat.begin() + (long)(p * B + cnt[p]));
            }
        return out;
    }
    void step(float) {}   // scene.cpp:336-339: all bodies are static, nothing to integrate
    double distance(const vec3 &from, const vec3 &to) const { return (double)(from.distance(to) * 10.0f); }   // [mm], scene.cpp:342-346

    std::shared_ptr<device> dev;
    mcrt_params params{};
    uint32_t frame_id = 0;

private:
    void init()   // scene.cpp:38-48 + 300-334: load each OBJ, place it, hand the triangle soup to the GPU
    {
        std::vector<float> tri; std::vector<uint32_t> tri_mesh; std::vector<mcrt_mesh> recs;
        triangles(tri, tri_mesh, recs);
        if (materials.empty()) throw std::runtime_error("Error while loading scene: no materials");
        check(dev->upload_scene(tri.data(), tri_mesh.data(), (uint32_t)(tri.size() / 9), recs.data(), (uint32_t)recs.size(),
                                &materials[0].impedance, (uint32_t)materials.size(), material_index(starting_material), spacing.data()), "mcrt_upload_scene");
    }
};

// ---------------------------------------------------------------- what rf_image is made of
// A device allocation of a context, freed with it.  Move-only; it keeps the context alive.
class device_buffer {
public:
    explicit device_buffer(std::shared_ptr<device> dev_) : dev(std::move(dev_)) {}
    device_buffer(device_buffer &&o) noexcept : dev(std::move(o.dev)), p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    ~device_buffer() { release(); }
    void reserve(size_t bytes)   // room for `bytes`: grown, never shrunk
    {
        if (p && bytes <= cap) return;
        release();
        check(mcrt_alloc(dev->ctx, bytes, &p), "mcrt_alloc");
        cap = bytes;
    }
    void release() { if (p) mcrt_free(dev->ctx, p); p = nullptr; cap = 0; }
    template <typename T> T *as() const { return static_cast<T *>(p); }
private:
    std::shared_ptr<device> dev;
    void *p = nullptr;
    size_t cap = 0;
};

// a float picture as the 8-bit image of rfimage.h:142-148: times 255, clamped, NaN black
inline std::vector<unsigned char> to_bytes(const std::vector<float> &img)
{
    std::vector<unsigned char> b;
    b.reserve(img.size());
    for (float v : img) { const float x = v * 255.0f; b.push_back((unsigned char)(x != x || x < 0 ? 0 : x > 255 ? 255 : x)); }
    return b;
}
inline void write_pgm(const std::string &path, uint32_t cols, uint32_t rows, const std::vector<unsigned char> &bytes)   // binary PGM, the bytes as they are
{
    std::ofstream f(path, std::ios::binary);
    f << "P5\n" << cols << " " << rows << "\n255\n";
    f.write((const char *)bytes.data(), (std::streamsize)bytes.size());
}

inline void write_ppm(const std::string &path, uint32_t cols, uint32_t rows, const std::vector<unsigned char> &rgb)   // binary PPM, the bytes as they are
{
    std::ofstream f(path, std::ios::binary);
    f << "P6\n" << cols << " " << rows << "\n255\n";
    f.write((const char *)rgb.data(), (std::streamsize)rgb.size());
}

// ---------------------------------------------------------------- rf_image (rfimage.h)
// Two ways to fill it, both the reference's semantics:
//   trace(frame)            clear + cast_rays + the accumulation loop of main.cpp:102-144 fused on the GPU (the fast path)
//   clear() / add_echo()    the reference's own host-side accumulation (rfimage.h:33-40,161-164) into a host image [max_rows][columns]
// convolve / envelope / postprocess always run on the GPU: a host-accumulated image is uploaded first.
template <unsigned int columns, unsigned int max_travel_time_us, unsigned int axial_resolution_um, unsigned int speed_of_sound = 1500>
class rf_image {
public:
    static constexpr unsigned int max_rows = (speed_of_sound * max_travel_time_us) / axial_resolution_um;   // rfimage.h:180

    rf_image(double radius_mm, double angle_rad, std::shared_ptr<device> dev_ = nullptr)
        : dev(dev_ ? std::move(dev_) : default_device()), radius_mm(radius_mm), angle(angle_rad), host((size_t)columns * max_rows, 0.0f),
          rf(dev), scan(dev), bmode_buf(dev), state(dev), planes(dev), stack(dev), points(dev), rendered(dev), label(dev), sound(dev), sigma(dev), curve(dev), band_stack(dev), flow_in(dev), flow_out(dev), spectral_buf(dev), strain_buf(dev), strain_pic(dev), shear_buf(dev), shear_pic(dev), mmode_buf(dev), mmode_pic(dev)
    {
        std::cout << "rf_image: " << max_rows << ", " << columns << std::endl;          // rfimage.h:30
        rf.reserve(sizeof(float) * columns * max_rows);
        scan.reserve(sizeof(float) * 400 * 500);
    }
    rf_image(std::shared_ptr<device> dev_, double radius_mm, double angle_rad) : rf_image(radius_mm, angle_rad, std::move(dev_)) {}
    rf_image(const rf_image &) = delete; rf_image &operator=(const rf_image &) = delete;

    // rfimage.h:33-40: row = micros / (axial_resolution / speed_of_sound), integer micrometres over um/us
    void add_echo(const unsigned int column, const float echo, const double micros_from_source)
    {
        to_host();
        const double row = micros_from_source / ((double)axial_resolution_um / (double)speed_of_sound);
        if (row < (double)max_rows) host[(size_t)(int)row * columns + column] += echo;
    }
    constexpr double get_dt() const { return (double)axial_resolution_um / (double)speed_of_sound; }                      // [us] rfimage.h:43-46
    constexpr double micros_traveled(double microm_from_source) const { return microm_from_source / (double)speed_of_sound; }   // rfimage.h:48-51
    void clear() { std::fill(host.begin(), host.end(), 0.0f); where = on_host; banded = 0; }                                     // rfimage.h:161-164
    void print(size_t column) const                                                                                       // rfimage.h:166-173
    {
        const auto img = intensities();
        for (size_t i = 0; i < max_rows; i++) std::cout << img[i * columns + column] << ", ";
        std::cout << std::endl;
    }

    // clear() + cast_rays + the accumulation loop of main.cpp:102-144 in one call, on the GPU
    void trace(uint32_t frame_id)
    {
        shape_params();
        check(dev->trace_frames(frame_id, 1, columns, rf.as<float>()), "mcrt_trace_frame");       // (every GPU of a group traces its scan-line shard)
        where = on_device; traced_as(stack_of::nothing, 0, frame_id);
    }
    // the same with slice thickness (psf.h:16-18,42,77; mcrt.h): the frame's n_planes elevation planes (0: the psf's elevation_size), spread
    // p.elevation_pitch_um() apart around the transducer's own plane, traced as ONE pose pass -- plane k with frame id frame_id * K + k, the
    // frame-id rule of mcrt.h -- and folded into this image with p.elevation_rows() (mcrt_elevation_frames).  trace(frame_id) keeps its meaning.
    template <size_t N, typename psf_> void trace(uint32_t frame_id, const transducer<N> &t, const psf_ &p, uint32_t n_planes = 0)
    {
        static_assert(N == columns, "one scan-line per transducer element");
        const uint32_t K = n_planes ? n_planes : (uint32_t)p.get_elevation_size();
        const auto tables = t.planes(K, p.elevation_pitch_um());
        const std::vector<float> &w = p.elevation_rows(max_rows, row_mm(), K);
        pose_pass(frame_id, K, tables, planes, "rf_image::trace: frame_id * n_planes does not fit a frame id");
        check(mcrt_elevation_frames(dev->ctx, planes.as<float>(), 1, K, columns, max_rows, w.data(), rf.as<float>()), "mcrt_elevation_frames");
        where = on_device; traced_as(stack_of::nothing, 0, frame_id);
    }
    // spatial compounding (mcrt.h): the frame's views, one per steering angle [rad] of steer_rad (1..16), traced as ONE pose pass -- view n with
    // frame id frame_id * N + n, the frame-id rule of mcrt.h -- into a stack [N][columns][max_rows] this image owns.  convolve() and envelope()
    // then run over the N views, and the views meet in postprocess(steer_rad) / postprocess(bmode_params, steer_rad).  The RF image of
    // trace(frame_id) is left as it is; the next trace(frame_id ...) without a steer list ends the compounded state.
    template <size_t N> void trace(uint32_t frame_id, const transducer<N> &t, const std::vector<float> &steer_rad)
    {
        static_assert(N == columns, "one scan-line per transducer element");
        const uint32_t V = (uint32_t)steer_rad.size();
        if (V == 0 || V > 16) throw std::invalid_argument("rf_image::trace: 1..16 steering angles");
        pose_pass(frame_id, V, t.steered(steer_rad), stack, "rf_image::trace: frame_id * views does not fit a frame id");
        traced_as(stack_of::views, V, frame_id * V);
    }
    // volume imaging (mcrt.h): the K planes of a probe swept in elevation, traced as ONE pose pass -- plane k with frame id frame_id * K + k, the
    // frame-id rule of mcrt.h -- into the stack [K][columns][max_rows] the views of a compounded frame use.  convolve() and envelope() then run
    // over the K planes, and volume(grid) / volume(bmode_params, grid) gather them at a grid's points.  The next trace of another kind ends
    // the swept state.
    template <size_t N> void trace(uint32_t frame_id, const transducer<N> &t, const mcrt_sweep &sw)
    {
        static_assert(N == columns, "one scan-line per transducer element");
        if (sw.n_planes == 0 || sw.n_planes > 256) throw std::invalid_argument("rf_image::trace: a sweep has 1..256 planes");
        pose_pass(frame_id, sw.n_planes, t.swept(sw), stack, "rf_image::trace: frame_id * planes does not fit a frame id");
        sweep = sw; traced_as(stack_of::sweep_planes, sw.n_planes, frame_id * sw.n_planes);
    }
    // freehand 3-D (mcrt.h: mcrt_recon_frames): the frames of a tracked probe moved by hand, one pose per frame -- a vector of transducers, or the
    // two tables [F][columns][3] (transducer::freehand makes a regular one) --, traced as ONE pose pass -- pose f with frame id frame_id * F + f
    // -- into the stack the views of a compounded frame use.  convolve(), envelope() and despeckle() then run over the F frames, and
    // reconstruct(grid) bins them into voxels.  The tables are kept for it.  The next trace of another kind ends the tracked state.
    void trace(uint32_t frame_id, const std::vector<float> &pos, const std::vector<float> &dir)
    {
        const size_t one = 3 * (size_t)columns, F = pos.size() / one;
        if (F == 0 || F > 65535 || pos.size() != F * one || dir.size() != pos.size()) throw std::invalid_argument("rf_image::trace: pose tables [F][columns][3], F = 1..65535");
        tracked.pos = pos; tracked.dir = dir;
        pose_pass(frame_id, (uint32_t)F, tracked, stack, "rf_image::trace: frame_id * poses does not fit a frame id");
        traced_as(stack_of::tracked_frames, (uint32_t)F, frame_id * (uint32_t)F);
    }
    template <size_t N> void trace(uint32_t frame_id, const std::vector<transducer<N>> &poses)
    {
        static_assert(N == columns, "one scan-line per transducer element");
        std::vector<float> pos, dir;
        for (const auto &t : poses) { pos.insert(pos.end(), t.pos.begin(), t.pos.end()); dir.insert(dir.end(), t.dir.begin(), t.dir.end()); }
        trace(frame_id, pos, dir);
    }
    // the frames of trace(frame, poses) binned into grid's voxels (a grid in the WORLD frame, mm; scene units are cm) with hole filling: floats
    // [nw][nv][nu].  opts: null = mcrt_default_recon_opts; counts: the samples per voxel, when asked for.  A row of a scan-line is
    // depth_mm_f / max_rows long, the row pitch of volume(grid)'s maps.  filter: 3-D speckle reduction over the block on the device, in place,
    // before it is copied (mcrt.h: mcrt_speckle_volume_frames; a hole's `empty` value is a value like any other, counts tell which voxels were empty)
    std::vector<float> reconstruct(const mcrt_volume_grid &grid, const mcrt_recon_opts *opts = nullptr, std::vector<uint32_t> *counts = nullptr,
                                   const mcrt_speckle3d_opts *filter = nullptr)
    {
        if (holds != stack_of::tracked_frames) throw std::invalid_argument("rf_image::reconstruct: trace(frame, poses) first");
        const size_t n = grid_points(grid, "reconstruct");
        points.reserve(8 * n);
        check(mcrt_recon_frames(dev->ctx, stack.as<float>(), n_views, columns, max_rows, tracked.pos.data(), tracked.dir.data(), row_pitch_mm(), 10.0,
                                &grid, opts, points.as<float>(), counts ? points.as<uint32_t>() + n : nullptr, nullptr), "mcrt_recon_frames");
        if (counts) *counts = download<uint32_t>(points.as<uint32_t>() + n, n);
        if (filter) check(mcrt_speckle_volume_frames(dev->ctx, points.as<float>(), 1, grid.nu, grid.nv, grid.nw, filter, points.as<float>()), "mcrt_speckle_volume_frames");
        return download<float>(points, n);
    }
    // the ground truth of reconstruct(grid) (mcrt.h: mcrt_recon_label_frames): the central beams of the poses of trace(frame, poses) walked through
    // the scene (mcrt_label_frames, at most 1024 poses; lopts: null = the tracer's rule at the tracer's start offset) and voted into grid's voxels:
    // bytes [nw][nv][nu], the material most of a voxel's samples carry, holes filled as ropts says, MCRT_LABEL_NONE where nothing is near.
    // ropts.n_labels is the scene's material count (mcrt_default_recon_label_opts(&o, scene.materials.size())).  counts, votes: the samples per
    // voxel and the winner's share of them, when asked for.  It needs the tracked state as reconstruct() does; the tables of labels() are
    // overwritten, so label_picture() / label_volume() want a new labels() after it.
    std::vector<unsigned char> reconstruct_labels(const mcrt_volume_grid &grid, const mcrt_recon_label_opts &ropts, const mcrt_label_opts *lopts = nullptr,
                                                  std::vector<uint32_t> *counts = nullptr, std::vector<uint32_t> *votes = nullptr)
    {
        if (holds != stack_of::tracked_frames) throw std::invalid_argument("rf_image::reconstruct_labels: trace(frame, poses) first");
        const size_t n = grid_points(grid, "reconstruct_labels"), taps = (size_t)n_views * columns * max_rows;
        shape_params();
        label.reserve(taps);
        labelled = labels_of::nothing; label_planes = 0; label_tissue = nullptr;
        mcrt_ctx *tracer = dev->tracer();
        check(mcrt_label_frames(tracer, n_views, 0, columns, tracked.pos.data(), tracked.dir.data(), lopts, label.as<uint8_t>(), nullptr, nullptr), "mcrt_label_frames");
        check(mcrt_synchronize(tracer), "mcrt_synchronize");
        points.reserve(9 * n);                                     // counts, votes, then the labels' bytes (the 32-bit tables first: aligned)
        uint32_t *count_dev = points.as<uint32_t>(), *votes_dev = count_dev + n;
        uint8_t *out_dev = points.as<uint8_t>() + 8 * n;
        check(mcrt_recon_label_frames(dev->ctx, label.as<uint8_t>(), n_views, columns, max_rows, tracked.pos.data(), tracked.dir.data(), row_pitch_mm(), 10.0, &grid, &ropts,
                                      out_dev, counts ? count_dev : nullptr, votes ? votes_dev : nullptr, nullptr), "mcrt_recon_label_frames");
        if (counts) *counts = download<uint32_t>(count_dev, n);
        if (votes) *votes = download<uint32_t>(votes_dev, n);
        return download<unsigned char>(out_dev, n);
    }
    template <typename psf_> void convolve(const psf_ &p)
    {
        const image_set s = traced();     // (the views of a compounded frame, the planes of a sweep, as so many frames)
        const uint32_t n_ax = (uint32_t)p.get_axial_size(), n_lat = (uint32_t)p.get_lateral_size();
        if (p.has_bands()) {   // frequency compounding: the images go to the band stack, where add_noise() finds them and envelope() / fold_bands() brings them back
            const std::vector<float> &ax = p.axial_rows(max_rows, row_mm());
            const uint32_t B = p.n_bands();
            band_w = p.band_weights(max_rows, row_mm());
            band_stack.reserve(sizeof(float) * s.images * B * columns * max_rows);
            check(mcrt_convolve_bands_frames(dev->ctx, s.dev, s.images, columns, max_rows, B, ax.data(), n_ax, p.has_focus() ? nullptr : p.lateral_kernel.data(),
                                             p.has_focus() ? p.lateral_rows(max_rows, row_mm()).data() : nullptr, n_lat, band_stack.as<float>()), "mcrt_convolve_bands_frames");
            banded = B;
        } else if (p.has_focus())   // focal zones: a lateral kernel per row, rows axial_resolution_um / 1000 mm apart
            check(mcrt_convolve_frames_depth(dev->ctx, s.dev, s.images, columns, max_rows, p.axial_kernel.data(), n_ax, p.lateral_rows(max_rows, row_mm()).data(), n_lat), "mcrt_convolve_frames_depth");
        else
            check(mcrt_convolve_frames(dev->ctx, s.dev, s.images, columns, max_rows, p.axial_kernel.data(), n_ax, p.lateral_kernel.data(), n_lat), "mcrt_convolve_frames");
    }
    // the band images that convolve(p) left (p.has_bands()) folded back into the images with the bands' weights (mcrt_band_fold_frames); nothing
    // to do when there are none.  envelope() ends in it: detected band images averaged, frequency compounding.  Called on its own, before any
    // envelope, it is a coherent sum: the same as one pulse that is the weighted sum of the bands', and it reduces no speckle
    void fold_bands()
    {
        if (!banded) return;
        const image_set s = traced();
        check(mcrt_band_fold_frames(dev->ctx, band_stack.as<float>(), s.images, banded, columns, max_rows, band_w.data(), s.dev), "mcrt_band_fold_frames");
        banded = 0;
    }
    void envelope()
    {
        const image_set s = pending();
        check(mcrt_envelope_frames(dev->ctx, s.dev, s.images, columns, max_rows), "mcrt_envelope_frames");
        fold_bands();
    }
    // quadrature detection (mcrt.h: mcrt_detect_frames) in the place of envelope(): the FIR Hilbert envelope of whatever envelope() would have
    // detected, in place -- the band images of a convolve(p) with bands, which it then folds; the views, planes or tracked frames of the last
    // trace(); or this image.  Everything after it sees what it saw after envelope()
    void detect(const mcrt_detect_opts &o)
    {
        const image_set s = pending();
        check(mcrt_detect_frames(dev->ctx, s.dev, s.images, columns, max_rows, &o, s.dev, nullptr), "mcrt_detect_frames");
        fold_bands();
    }
    // the analytic pair of this image's RF at the RF rate: interleaved [columns][max_rows][2] = (the RF's own bits, its FIR Hilbert transform
    // along the scan-line).  The image is left as it is (call it before envelope() / detect()).  A stack of views, planes or tracked
    // frames is not one image and band images have no one carrier: it throws
    void iq(const mcrt_detect_opts &o, std::vector<float> &interleaved)
    {
        if (n_views || banded) throw std::logic_error("rf_image::iq: the analytic pair is of one RF image, not of a stack or of band images");
        const image_set s = traced();
        const size_t n = (size_t)columns * max_rows;
        points.reserve(2 * sizeof(float) * n);
        check(mcrt_detect_frames(dev->ctx, s.dev, s.images, columns, max_rows, &o, nullptr, points.as<float>()), "mcrt_detect_frames");
        interleaved = download<float>(points.as<float>(), 2 * n);
    }
    // colour Doppler (mcrt.h: mcrt_flow_split_frames, mcrt_flow_frames, mcrt_colour_frames), three steps around the B-mode chain of ONE trace:
    //   trace(f);  flow_split(t, vel);  convolve(p); [add_noise();] envelope() / detect();  postprocess(bmode_params);  colour_flow(p, fo, co, rgb);
    // flow_split() goes right after trace(frame_id), while this image holds the raw RF: the label pass of t's central beams (lopts: null =
    // the tracer's rule) and the split into what stands still and what moves, a device copy this image keeps.  vel_mm_s: a velocity
    // vector per material of the scene [n_materials][3] (scene::material_index names them).  A stack of views, planes or tracked frames,
    // or a host-deposited image, has no labels of its own: it throws
    template <size_t N> void flow_split(const transducer<N> &t, const std::vector<float> &vel_mm_s, const mcrt_label_opts *lopts = nullptr)
    {
        static_assert(N == columns, "one scan-line per transducer element");
        if (n_views || where != on_device) throw std::logic_error("rf_image::flow_split: right after trace(frame_id), on one traced image");
        const uint32_t L = (uint32_t)(vel_mm_s.size() / 3u);
        if (L == 0 || L > 254 || vel_mm_s.size() != 3u * L) throw std::invalid_argument("rf_image::flow_split: a velocity [3] per material, 1..254 materials");
        const size_t n = (size_t)columns * max_rows;
        flow_in.reserve(4 * 6 * n + n);                              // floats: the parts [2][n], their pairs [2][n][2]; then the tissue bytes
        mcrt_ctx *tracer = dev->tracer();
        check(mcrt_label_frames(tracer, 1, 0, columns, t.pos.data(), t.dir.data(), lopts, flow_tissue(), nullptr, nullptr), "mcrt_label_frames");
        check(mcrt_synchronize(tracer), "mcrt_synchronize");
        std::vector<uint8_t> moving(L);
        for (uint32_t l = 0; l < L; l++) moving[l] = vel_mm_s[3 * l] != 0.0f || vel_mm_s[3 * l + 1] != 0.0f || vel_mm_s[3 * l + 2] != 0.0f;
        check(mcrt_flow_split_frames(dev->ctx, rf.as<float>(), flow_tissue(), 1, columns, max_rows, moving.data(), L, flow_in.as<float>()), "mcrt_flow_split_frames");
        flow_vel = vel_mm_s; flow_dir = t.dir; flow_frequency = (double)t.frequency; flow_detected = false; spectral_T = spectral_cols = 0;
    }
    // the colour processor in beam space: the two parts through p's PSF and the detector's I/Q (dopts: null = 31 taps), then mcrt_flow_frames.
    // noise_sigma: the ensemble's sigma is the one add_noise() left on the device for this pass (it throws when it has not run), else
    // fo.sigma.  The maps are [columns][max_rows]; the autocorrelation stays on the device for colour_flow()
    struct flow_maps { std::vector<float> vel, var, truth; double v_nyq_mm_s = 0.0, sigma = 0.0; };
    template <typename psf_> flow_maps flow(const psf_ &p, const mcrt_flow_opts &fo, bool noise_sigma = false, const mcrt_detect_opts *dopts = nullptr)
    {
        if (flow_vel.empty()) throw std::logic_error("rf_image::flow: flow_split(transducer, velocities) first");
        if (p.has_bands()) throw std::invalid_argument("rf_image::flow: colour flow is one pulse: a psf without bands");
        if (noise_sigma && sigma_frames != 1) throw std::logic_error("rf_image::flow: noise_sigma needs add_noise() on the same pass");
        const size_t n = (size_t)columns * max_rows;
        const uint32_t L = (uint32_t)(flow_vel.size() / 3u), n_ax = (uint32_t)p.get_axial_size(), n_lat = (uint32_t)p.get_lateral_size();
        flow_maps m;
        check(mcrt_flow_nyquist(&fo, flow_frequency, (double)speed_of_sound, &m.v_nyq_mm_s), "mcrt_flow_nyquist");
        std::vector<float> phasor(2 * (size_t)L * columns), truth((size_t)L * columns);
        check(mcrt_flow_phasors(m.v_nyq_mm_s, flow_vel.data(), flow_dir.data(), L, columns, phasor.data(), truth.data()), "mcrt_flow_phasors");
        float *parts = flow_in.as<float>(), *pairs = parts + 2 * n;
        if (p.has_focus())
            check(mcrt_convolve_frames_depth(dev->ctx, parts, 2, columns, max_rows, p.axial_kernel.data(), n_ax, p.lateral_rows(max_rows, row_mm()).data(), n_lat), "mcrt_convolve_frames_depth");
        else
            check(mcrt_convolve_frames(dev->ctx, parts, 2, columns, max_rows, p.axial_kernel.data(), n_ax, p.lateral_kernel.data(), n_lat), "mcrt_convolve_frames");
        mcrt_detect_opts d; mcrt_default_detect_opts(&d);
        check(mcrt_detect_frames(dev->ctx, parts, 2, columns, max_rows, dopts ? dopts : &d, nullptr, pairs), "mcrt_detect_frames");
        flow_out.reserve(4 * 6 * n);                                 // corr [3][n], vel, var, truth
        float *corr = flow_out.as<float>(), *vel = corr + 3 * n, *var = vel + n, *tr = var + n;
        check(mcrt_flow_frames(dev->ctx, pairs, pairs + 2 * n, flow_tissue(), 1, columns, max_rows, &fo, m.v_nyq_mm_s, phasor.data(), truth.data(), L, first_id,
                               noise_sigma ? sigma.as<float>() : nullptr, corr, vel, var, tr), "mcrt_flow_frames");
        m.vel = download<float>(vel, n); m.var = download<float>(var, n); m.truth = download<float>(tr, n);
        flow_detected = true;
        m.sigma = noise_sigma ? (double)download<float>(sigma.as<float>(), 1)[0] : (double)fo.sigma;
        return m;
    }
    // the colour-flow picture over the last postprocess(bmode_params) frame: flow(), the autocorrelation gathered through
    // mcrt_scan_convert_frames at that frame's size, and mcrt_colour_frames with co -- whose power_thr is REPLACED by power_scale * 2 * N *
    // sigma^2 when power_scale >= 0 (4 by default: a modelling choice nothing measures).  rgb: [out_rows][out_cols][3]; returns flow()'s maps
    template <typename psf_> flow_maps colour_flow(const psf_ &p, const mcrt_flow_opts &fo, const mcrt_colour_opts &co, std::vector<unsigned char> &rgb,
                                                   bool noise_sigma = false, double power_scale = 4.0, const mcrt_detect_opts *dopts = nullptr, std::vector<float> *velocity = nullptr)
    {
        if (!bmode_n) throw std::logic_error("rf_image::colour_flow: postprocess(bmode_params) first: the picture under the colour");
        const size_t n = (size_t)columns * max_rows, np = bmode_n;
        flow_out.reserve(4 * 6 * n + 4 * 4 * np + 3 * np);          // flow()'s six planes, then corr_img [3][np], vel_img [np] and the rgb bytes (before flow(): growing forgets)
        flow_maps m = flow(p, fo, noise_sigma, dopts);
        float *corr = flow_out.as<float>(), *img = corr + 6 * n, *vimg = img + 3 * np;
        uint8_t *out = reinterpret_cast<uint8_t *>(vimg + np);
        check(mcrt_scan_convert_frames(dev->ctx, corr, 3, columns, max_rows, radius_mm, angle, img, bmode_rows, bmode_cols), "mcrt_scan_convert_frames");
        mcrt_colour_opts c = co;
        if (power_scale >= 0.0) c.power_thr = (float)(power_scale * 2.0 * (double)fo.n_packets * m.sigma * m.sigma);
        uint8_t lut[256 * 3];
        check(mcrt_colour_map(0, lut), "mcrt_colour_map");
        check(mcrt_colour_frames(dev->ctx, img, bmode_buf.as<uint8_t>(), 1, bmode_rows, bmode_cols, lut, &c, m.v_nyq_mm_s, out, vimg), "mcrt_colour_frames");
        rgb = download<unsigned char>(out, 3 * np);
        if (velocity) *velocity = download<float>(vimg, np);
        return m;
    }
    // spectral Doppler (mcrt.h: mcrt_spectral_series_frames, mcrt_spectral_frames, mcrt_sonogram_frames), three steps after flow() or
    // colour_flow(), which leave the detected pairs of what stands still and what moves on the device:
    //   ...;  flow(p, fo);  tissue_line(line);  spectral_series(line, row0, so, rate, phase);  spectrum(so, v_nyq);  sonogram(go);
    // the tissue labels [max_rows] of one scan-line of the last flow_split(), for mcrt_spectral_profile
    std::vector<uint8_t> tissue_line(uint32_t line)
    {
        if (flow_vel.empty() || line >= columns) throw std::logic_error("rf_image::tissue_line: flow_split() first, and a scan-line of this image");
        return download<uint8_t>(flow_tissue() + (size_t)line * max_rows, max_rows);
    }
    // the slow-time series [T][2] of ONE gate -- rows row0 .. row0 + so.gate_rows - 1 of scan-line `line`, every row's weight 1 -- from rate
    // [gate_rows] (mcrt_spectral_rates) and phase [T] (mcrt_spectral_phase).  noise_sigma as in flow().  It stays on the device for spectrum()
    std::vector<float> spectral_series(uint32_t line, uint32_t row0, const mcrt_spectral_opts &so, const std::vector<int32_t> &rate, const std::vector<int64_t> &phase,
                                       bool noise_sigma = false)
    {
        if (!flow_detected) throw std::logic_error("rf_image::spectral_series: flow() or colour_flow() first: they detect the two parts");
        if (noise_sigma && sigma_frames != 1) throw std::logic_error("rf_image::spectral_series: noise_sigma needs add_noise() on the same pass");
        if (rate.size() != so.gate_rows || phase.size() != so.n_pulses) throw std::invalid_argument("rf_image::spectral_series: rate [gate_rows] and phase [n_pulses]");
        const size_t n = (size_t)columns * max_rows, T = so.n_pulses;
        spectral_buf.reserve(8 * T);
        const float *pairs = flow_in.as<float>() + 2 * n;
        const mcrt_gate gate{ 0u, line, row0 };
        const std::vector<float> weight(so.gate_rows, 1.0f);
        spectral_cols = 0;
        check(mcrt_spectral_series_frames(dev->ctx, pairs, pairs + 2 * n, 1, columns, max_rows, &gate, 1, weight.data(), rate.data(), phase.data(), &so, first_id,
                                          noise_sigma ? sigma.as<float>() : nullptr, spectral_buf.as<float>()), "mcrt_spectral_series_frames");
        spectral_T = (uint32_t)T;
        return download<float>(spectral_buf.as<float>(), 2 * T);
    }
    // the spectra of the last spectral_series(): power [n_cols][n_fft] in velocity order and the mean velocity [n_cols]; window_kind:
    // mcrt_spectral_window's (1: Hann).  The power stays on the device for sonogram()
    struct spectra { std::vector<float> power, mean; uint32_t n_cols = 0, n_fft = 0; };
    spectra spectrum(const mcrt_spectral_opts &so, double v_nyq_mm_s, uint32_t window_kind = 1)
    {
        if (!spectral_T || spectral_T != so.n_pulses) throw std::logic_error("rf_image::spectrum: spectral_series() with the same options first");
        std::vector<float> h(so.n_fft >= 32 && so.n_fft <= 512 ? so.n_fft : 512);
        check(mcrt_spectral_window(window_kind, so.n_fft, h.data()), "mcrt_spectral_window");
        if (so.hop == 0 || so.n_pulses < so.n_fft) throw std::invalid_argument("rf_image::spectrum: hop >= 1 and n_pulses >= n_fft");
        spectra out;
        out.n_fft = so.n_fft; out.n_cols = (so.n_pulses - so.n_fft) / so.hop + 1u;
        const size_t T = so.n_pulses, np = (size_t)out.n_cols * so.n_fft;
        {   // the series moves into a buffer with room for the spectra, their means and the picture behind it (growing forgets)
            const std::vector<float> z = download<float>(spectral_buf.as<float>(), 2 * T);
            spectral_buf.reserve(8 * T + 4 * np + 4 * out.n_cols + np);
            check(mcrt_memcpy_h2d(dev->ctx, spectral_buf.as<float>(), z.data(), 8 * T), "mcrt_memcpy_h2d");
        }
        float *power = spectral_buf.as<float>() + 2 * T, *mean = power + np;
        check(mcrt_spectral_frames(dev->ctx, spectral_buf.as<float>(), 1, h.data(), &so, v_nyq_mm_s, power, mean), "mcrt_spectral_frames");
        out.power = download<float>(power, np); out.mean = download<float>(mean, out.n_cols);
        spectral_cols = out.n_cols; spectral_N = so.n_fft;
        return out;
    }
    // the picture of the last spectrum(), bytes [n_fft][n_cols], row 0 the highest velocity towards the probe
    std::vector<unsigned char> sonogram(const mcrt_sonogram_opts &go)
    {
        if (!spectral_cols) throw std::logic_error("rf_image::sonogram: spectrum() first");
        const size_t T = spectral_T, np = (size_t)spectral_cols * spectral_N;
        float *power = spectral_buf.as<float>() + 2 * T;
        uint8_t *grey = reinterpret_cast<uint8_t *>(power + np + spectral_cols);
        check(mcrt_sonogram_frames(dev->ctx, power, 1, spectral_cols, spectral_N, &go, nullptr, grey), "mcrt_sonogram_frames");
        return download<unsigned char>(grey, np);
    }
    // strain elastography (mcrt.h: mcrt_strain_compress_frames, mcrt_strain_frames, mcrt_elastogram_frames), three steps around the B-mode
    // chain of ONE trace:
    //   trace(f);  convolve(p); [add_noise();]  compress(t, modulus, applied, ref, so, cycles);  envelope() / detect();  postprocess(bmode_params);
    //   track(so);  elastogram(eo, rgb);
    // compress() goes while this image holds the RF before the envelope: the label pass of t's central beams (lopts: null = the tracer's
    // rule), the detector's I/Q (dopts: null = 31 taps) and the post-compression pairs, device copies this image keeps.  modulus: a
    // Young's modulus per material of the scene [n_materials] (scene::material_index names them; 0: rigid); applied: the strain of a
    // material of ref_modulus; cycles_per_row: mcrt_psf_carrier's.  A stack of views, planes or tracked frames, band images or a
    // host-deposited image has no one analytic line: it throws.  The maps are [columns][max_rows]
    struct strain_truth { std::vector<float> disp, strain; };
    template <size_t N> strain_truth compress(const transducer<N> &t, const std::vector<double> &modulus, double applied, double ref_modulus, const mcrt_strain_opts &so,
                                              double cycles_per_row, const mcrt_label_opts *lopts = nullptr, const mcrt_detect_opts *dopts = nullptr)
    {
        static_assert(N == columns, "one scan-line per transducer element");
        if (n_views || banded || where != on_device) throw std::logic_error("rf_image::compress: after trace(frame_id) and convolve(psf), on one traced image");
        const uint32_t L = (uint32_t)modulus.size();
        if (L == 0 || L > 254) throw std::invalid_argument("rf_image::compress: a modulus per material, 1..254 materials");
        std::vector<int32_t> eps(L);
        check(mcrt_strain_table(modulus.data(), L, applied, ref_modulus, eps.data()), "mcrt_strain_table");
        const size_t n = (size_t)columns * max_rows;
        strain_buf.reserve(4 * 9 * n + n);                           // floats: the pairs [n][2], post [n][2], truth_disp, truth_strain, disp, rho, strain; then the tissue bytes
        uint8_t *tissue = strain_buf.as<uint8_t>() + 4 * 9 * n;
        mcrt_ctx *tracer = dev->tracer();
        check(mcrt_label_frames(tracer, 1, 0, columns, t.pos.data(), t.dir.data(), lopts, tissue, nullptr, nullptr), "mcrt_label_frames");
        check(mcrt_synchronize(tracer), "mcrt_synchronize");
        float *pairs = strain_buf.as<float>(), *post = pairs + 2 * n, *td = post + 2 * n, *ts = td + n;
        mcrt_detect_opts d; mcrt_default_detect_opts(&d);
        check(mcrt_detect_frames(dev->ctx, rf.as<float>(), 1, columns, max_rows, dopts ? dopts : &d, nullptr, pairs), "mcrt_detect_frames");
        check(mcrt_strain_compress_frames(dev->ctx, pairs, tissue, 1, columns, max_rows, eps.data(), L, cycles_per_row, &so, first_id, nullptr, post, td, ts),
              "mcrt_strain_compress_frames");
        strain_cycles = cycles_per_row; strain_tracked = false;
        return { download<float>(td, n), download<float>(ts, n) };
    }
    // the tracker between the pairs compress() left: the displacement [rows], the correlation coefficient and the strain in beam space;
    // they stay on the device for elastogram()
    struct strain_maps { std::vector<float> disp, rho, strain; };
    strain_maps track(const mcrt_strain_opts &so)
    {
        if (strain_cycles == 0.0) throw std::logic_error("rf_image::track: compress() first");
        const size_t n = (size_t)columns * max_rows;
        float *pairs = strain_buf.as<float>(), *post = pairs + 2 * n, *disp = post + 4 * n, *rho = disp + n, *st = rho + n;
        check(mcrt_strain_frames(dev->ctx, pairs, post, 1, columns, max_rows, &so, strain_cycles, disp, rho, st), "mcrt_strain_frames");
        strain_tracked = true;
        return { download<float>(disp, n), download<float>(rho, n), download<float>(st, n) };
    }
    // the elastogram over the last postprocess(bmode_params) frame: track()'s strain and correlation coefficient gathered through
    // mcrt_scan_convert_frames at that frame's size, and mcrt_elastogram_frames with eo and mcrt_strain_map's table.  rgb: [out_rows][out_cols][3]
    void elastogram(const mcrt_elastogram_opts &eo, std::vector<unsigned char> &rgb)
    {
        if (!strain_tracked) throw std::logic_error("rf_image::elastogram: track() first");
        if (!bmode_n) throw std::logic_error("rf_image::elastogram: postprocess(bmode_params) first: the picture under the colour");
        const size_t n = (size_t)columns * max_rows, np = bmode_n;
        strain_pic.reserve(4 * 2 * np + 3 * np);                     // strain_img, rho_img, then the rgb bytes
        float *st = strain_buf.as<float>() + 8 * n, *rho = st - n, *img = strain_pic.as<float>();
        uint8_t *out = reinterpret_cast<uint8_t *>(img + 2 * np);
        check(mcrt_scan_convert_frames(dev->ctx, st, 1, columns, max_rows, radius_mm, angle, img, bmode_rows, bmode_cols), "mcrt_scan_convert_frames");
        check(mcrt_scan_convert_frames(dev->ctx, rho, 1, columns, max_rows, radius_mm, angle, img + np, bmode_rows, bmode_cols), "mcrt_scan_convert_frames");
        uint8_t lut[256 * 3];
        check(mcrt_strain_map(0, lut), "mcrt_strain_map");
        check(mcrt_elastogram_frames(dev->ctx, img, img + np, bmode_buf.as<uint8_t>(), 1, bmode_rows, bmode_cols, lut, &eo, out), "mcrt_elastogram_frames");
        rgb = download<unsigned char>(out, 3 * np);
    }
    // shear-wave elastography (mcrt.h: mcrt_shear_wave_frames, mcrt_shear_speed_frames, mcrt_elastogram_frames), three steps around the B-mode
    // chain of ONE trace:
    //   trace(f);  convolve(p); [add_noise();]  shear_wave(t, speed_m_s, so, cycles);  envelope() / detect();  postprocess(bmode_params);
    //   shear_speed(so);  shear_elastogram(eo, rgb);
    // shear_wave() goes while this image holds the RF before the envelope: the label pass of t's central beams (lopts: null = the tracer's
    // rule), the detector's I/Q (dopts: null = 31 taps), then the push of so and its tracked wave.  speed_m_s: a shear speed per material
    // of the scene [n_materials] (scene::material_index names them; 0: a fluid, the wave does not pass); the tables are the helpers' own:
    // mcrt_shear_table at so.prf_hz, mcrt_shear_pitch of this image's sector, a raised cosine of width_pulses, a decay of decay_lines;
    // cycles_per_row: mcrt_psf_carrier's.  A stack of views, planes or tracked frames, band images or a host-deposited image has no one
    // analytic line: it throws.  The maps are [columns][max_rows]
    struct shear_wave_maps { std::vector<float> peak_time, peak_disp, truth_arrival, truth_speed; };
    template <size_t N> shear_wave_maps shear_wave(const transducer<N> &t, const std::vector<double> &speed_m_s, const mcrt_shear_opts &so, double cycles_per_row,
                                                   uint32_t width_pulses = 12, double decay_lines = 8.0, const mcrt_label_opts *lopts = nullptr,
                                                   const mcrt_detect_opts *dopts = nullptr)
    {
        static_assert(N == columns, "one scan-line per transducer element");
        if (n_views || banded || where != on_device) throw std::logic_error("rf_image::shear_wave: after trace(frame_id) and convolve(psf), on one traced image");
        const uint32_t L = (uint32_t)speed_m_s.size();
        if (L == 0 || L > 254) throw std::invalid_argument("rf_image::shear_wave: a shear speed per material, 1..254 materials");
        if (width_pulses == 0 || width_pulses > 256) throw std::invalid_argument("rf_image::shear_wave: width_pulses takes 1..256");
        std::vector<int64_t> slow(L);
        std::vector<float> speed_f(L);
        check(mcrt_shear_table(speed_m_s.data(), L, (double)so.prf_hz, slow.data(), speed_f.data()), "mcrt_shear_table");
        std::vector<uint32_t> pitch(max_rows), shape(64u * width_pulses), amp(columns);
        shear_pitch_mm.assign(max_rows, 0.0f);
        check(mcrt_shear_pitch(columns, max_rows, radius_mm, angle, max_travel_time_us, speed_of_sound, pitch.data(), shear_pitch_mm.data()), "mcrt_shear_pitch");
        check(mcrt_shear_shape(width_pulses, shape.data()), "mcrt_shear_shape");
        check(mcrt_shear_decay(columns, decay_lines, amp.data()), "mcrt_shear_decay");
        const size_t n = (size_t)columns * max_rows;
        shear_buf.reserve(4 * 9 * n + n);                            // floats: the pairs [n][2], peak_time, peak_disp, truth_arrival, truth_speed, speed, modulus, quality; then the tissue bytes
        uint8_t *tissue = shear_buf.as<uint8_t>() + 4 * 9 * n;
        mcrt_ctx *tracer = dev->tracer();
        check(mcrt_label_frames(tracer, 1, 0, columns, t.pos.data(), t.dir.data(), lopts, tissue, nullptr, nullptr), "mcrt_label_frames");
        check(mcrt_synchronize(tracer), "mcrt_synchronize");
        float *pairs = shear_buf.as<float>(), *pt = pairs + 2 * n, *pd = pt + n, *ta = pd + n, *ts = ta + n;
        mcrt_detect_opts d; mcrt_default_detect_opts(&d);
        check(mcrt_detect_frames(dev->ctx, rf.as<float>(), 1, columns, max_rows, dopts ? dopts : &d, nullptr, pairs), "mcrt_detect_frames");
        shear_stage = 0;
        check(mcrt_shear_wave_frames(dev->ctx, pairs, tissue, 1, columns, max_rows, slow.data(), speed_f.data(), L, pitch.data(), shape.data(), (uint32_t)shape.size(),
                                     amp.data(), columns, cycles_per_row, &so, first_id, nullptr, pt, pd, nullptr, ta, ts), "mcrt_shear_wave_frames");
        shear_stage = 1;
        return { download<float>(pt, n), download<float>(pd, n), download<float>(ta, n), download<float>(ts, n) };
    }
    // the fit across scan-lines over the peak times shear_wave() left: the speed [m/s], the modulus [kPa] and the quality in beam space;
    // they stay on the device for shear_elastogram()
    struct shear_maps { std::vector<float> speed, modulus, quality; };
    shear_maps shear_speed(const mcrt_shear_opts &so)
    {
        if (shear_stage < 1) throw std::logic_error("rf_image::shear_speed: shear_wave() first");
        const size_t n = (size_t)columns * max_rows;
        float *pt = shear_buf.as<float>() + 2 * n, *sp = pt + 4 * n, *mo = sp + n, *qu = mo + n;
        check(mcrt_shear_speed_frames(dev->ctx, pt, 1, columns, max_rows, shear_pitch_mm.data(), &so, sp, mo, qu), "mcrt_shear_speed_frames");
        shear_stage = 2;
        return { download<float>(sp, n), download<float>(mo, n), download<float>(qu, n) };
    }
    // the shear-wave elastogram over the last postprocess(bmode_params) frame: shear_speed()'s modulus and quality gathered through
    // mcrt_scan_convert_frames at that frame's size, and mcrt_elastogram_frames as it is with eo (ref_strain: the reference kPa, rho_min: the
    // smallest quality shown) and mcrt_shear_map's table.  rgb: [out_rows][out_cols][3]
    void shear_elastogram(const mcrt_elastogram_opts &eo, std::vector<unsigned char> &rgb)
    {
        if (shear_stage < 2) throw std::logic_error("rf_image::shear_elastogram: shear_speed() first");
        if (!bmode_n) throw std::logic_error("rf_image::shear_elastogram: postprocess(bmode_params) first: the picture under the colour");
        const size_t n = (size_t)columns * max_rows, np = bmode_n;
        shear_pic.reserve(4 * 2 * np + 3 * np);                      // modulus_img, quality_img, then the rgb bytes
        float *mo = shear_buf.as<float>() + 7 * n, *qu = mo + n, *img = shear_pic.as<float>();
        uint8_t *out = reinterpret_cast<uint8_t *>(img + 2 * np);
        check(mcrt_scan_convert_frames(dev->ctx, mo, 1, columns, max_rows, radius_mm, angle, img, bmode_rows, bmode_cols), "mcrt_scan_convert_frames");
        check(mcrt_scan_convert_frames(dev->ctx, qu, 1, columns, max_rows, radius_mm, angle, img + np, bmode_rows, bmode_cols), "mcrt_scan_convert_frames");
        uint8_t lut[256 * 3];
        check(mcrt_shear_map(0, lut), "mcrt_shear_map");
        check(mcrt_elastogram_frames(dev->ctx, img, img + np, bmode_buf.as<uint8_t>(), 1, bmode_rows, bmode_cols, lut, &eo, out), "mcrt_elastogram_frames");
        rgb = download<unsigned char>(out, 3 * np);
    }
    // M-mode (mcrt.h: mcrt_mmode_lines_frames, mcrt_mmode_picture_frames), two steps after ONE trace:
    //   trace(f);  convolve(p); [add_noise();]  m_lines(t, line, dilation, w_q16, bulk_q24, mo, cycles);  m_mode(display);
    // m_lines() goes while this image holds the RF before the envelope: the label pass of t's central beams (lopts: null = the tracer's
    // rule), the detector's I/Q (dopts: null = 31 taps), then mo.n_pulses pulses of scan-line `line`.  dilation: the peak axial strain per
    // material of the scene [n_materials] (scene::material_index names them; positive: compression); w_q16 and bulk_q24: one entry per
    // pulse (mcrt_mmode_waveform's, mcrt_mmode_bulk's or the caller's own); cycles_per_row: mcrt_psf_carrier's.  A stack of views, planes
    // or tracked frames, band images or a host-deposited image has no one analytic line: it throws.  The maps are [n_pulses][max_rows]
    struct m_line_maps { std::vector<float> env, truth_disp; std::vector<unsigned char> truth_label; };
    template <size_t N> m_line_maps m_lines(const transducer<N> &t, uint32_t line, const std::vector<double> &dilation, const std::vector<int32_t> &w_q16,
                                            const std::vector<int32_t> &bulk_q24, const mcrt_mmode_opts &mo, double cycles_per_row,
                                            const mcrt_label_opts *lopts = nullptr, const mcrt_detect_opts *dopts = nullptr)
    {
        static_assert(N == columns, "one scan-line per transducer element");
        if (n_views || banded || where != on_device) throw std::logic_error("rf_image::m_lines: after trace(frame_id) and convolve(psf), on one traced image");
        const uint32_t L = (uint32_t)dilation.size(), T = mo.n_pulses;
        if (L == 0 || L > 254) throw std::invalid_argument("rf_image::m_lines: a dilation per material, 1..254 materials");
        if (w_q16.size() != T || bulk_q24.size() != T) throw std::invalid_argument("rf_image::m_lines: w_q16 and bulk_q24 take one entry per pulse");
        std::vector<int32_t> dil(L);
        check(mcrt_mmode_table(dilation.data(), L, dil.data()), "mcrt_mmode_table");
        const size_t n = (size_t)columns * max_rows, m = (size_t)T * max_rows;
        mmode_buf.reserve(4 * 2 * n + 4 * 2 * m + m + n);            // floats: the pairs [n][2], env [m], truth_disp [m]; then the label bytes [m] and the tissue bytes [n]
        float *pairs = mmode_buf.as<float>(), *env = pairs + 2 * n, *td = env + m;
        uint8_t *tl = reinterpret_cast<uint8_t *>(td + m), *tissue = tl + m;
        mcrt_ctx *tracer = dev->tracer();
        check(mcrt_label_frames(tracer, 1, 0, columns, t.pos.data(), t.dir.data(), lopts, tissue, nullptr, nullptr), "mcrt_label_frames");
        check(mcrt_synchronize(tracer), "mcrt_synchronize");
        mcrt_detect_opts d; mcrt_default_detect_opts(&d);
        check(mcrt_detect_frames(dev->ctx, rf.as<float>(), 1, columns, max_rows, dopts ? dopts : &d, nullptr, pairs), "mcrt_detect_frames");
        mmode_pulses = 0;
        const mcrt_mline which{ 0u, line };
        check(mcrt_mmode_lines_frames(dev->ctx, pairs, tissue, 1, columns, max_rows, &which, 1, dil.data(), L, w_q16.data(), bulk_q24.data(), cycles_per_row, &mo, first_id,
                                      nullptr, env, nullptr, td, tl), "mcrt_mmode_lines_frames");
        mmode_pulses = T;
        return { download<float>(env, m), download<float>(td, m), download<unsigned char>(tl, m) };
    }
    // the sweep display of the pulses m_lines() left: the grey bytes and, registered with them pixel for pixel, the material and the true
    // displacement [rows], each [height][n_pulses / hop]
    struct m_mode_picture { std::vector<unsigned char> picture, labels; std::vector<float> truth_disp; uint32_t height = 0, width = 0; };
    m_mode_picture m_mode(const mcrt_mmode_display_opts &o)
    {
        if (!mmode_pulses) throw std::logic_error("rf_image::m_mode: m_lines() first");
        if (o.hop == 0 || o.hop > mmode_pulses) throw std::invalid_argument("rf_image::m_mode: hop takes 1..n_pulses");
        const size_t n = (size_t)columns * max_rows, m = (size_t)mmode_pulses * max_rows, np = (size_t)o.height * (mmode_pulses / o.hop);
        mmode_pic.reserve(4 * np + 2 * np);                          // truth_disp's picture, then the grey and the label bytes
        float *env = mmode_buf.as<float>() + 2 * n, *td = env + m, *dp = mmode_pic.as<float>();
        uint8_t *tl = reinterpret_cast<uint8_t *>(td + m), *grey = reinterpret_cast<uint8_t *>(dp + np), *lp = grey + np;
        check(mcrt_mmode_picture_frames(dev->ctx, env, tl, td, 1, mmode_pulses, max_rows, &o, nullptr, nullptr, grey, lp, dp), "mcrt_mmode_picture_frames");
        return { download<unsigned char>(grey, np), download<unsigned char>(lp, np), download<float>(dp, np), o.height, mmode_pulses / o.hop };
    }
    // receiver noise (mcrt.h: mcrt_noise_frames): a noise floor and a gain per scan-line (element_gain: [columns] or null) over whatever the
    // last trace() filled, in place -- this image, or the views of a compounded frame or the planes of a sweep as ONE frame (one receiver,
    // one peak), or the tracked frames of a freehand pass as so many frames -- with the ids that trace used.  It goes after convolve() and
    // before envelope(): receive noise is uncorrelated between scan-lines.  Every frame's sigma stays on the device for autogain().  After a
    // convolve(p) with bands it acts on the band images, B per image of the same frame, image i's band b with the id (first id + i) * B + b
    void add_noise(const mcrt_noise_opts &o, const float *element_gain = nullptr)
    {
        const image_set s = pending();
        sigma.reserve(4 * (size_t)s.frames);
        check(mcrt_noise_frames(dev->ctx, s.dev, s.frames, s.per_frame, columns, max_rows, s.first_id, &o, element_gain, sigma.as<float>()), "mcrt_noise_frames");
        sigma_frames = s.frames;
    }
    // automatic gain (mcrt.h: mcrt_autogain_frames): a depth gain curve estimated from each frame itself over whatever the last trace()
    // filled, in place -- this image, or the views of a compounded frame or the planes of a sweep as ONE frame (one receiver, one curve), or
    // the tracked frames of a freehand pass as so many frames.  It goes after envelope() (and despeckle()) and before whatever makes the
    // picture.  noise_floor: every frame's floor is the sigma that add_noise() left on the device (it throws when add_noise() has not run
    // on this pass); otherwise o.floor.  gain_curve(), penetration_rows() and penetration_mm() return its by-products
    void autogain(const mcrt_autogain_opts &o, bool noise_floor = false)
    {
        const image_set s = traced();                                      // (band images that wait are not looked at: envelope() comes first)
        const size_t F = s.frames;
        if (noise_floor && sigma_frames != F) throw std::logic_error("rf_image::autogain: noise_floor needs add_noise() on the same pass");
        curve.reserve(4 * F * (max_rows + 1u));                            // the gains [F][max_rows], then the penetration depths [F]
        float *k = curve.as<float>();
        uint32_t *pen = reinterpret_cast<uint32_t *>(k + F * max_rows);
        check(mcrt_autogain_frames(dev->ctx, s.dev, s.frames, s.per_frame, columns, max_rows, &o, noise_floor ? sigma.as<float>() : nullptr, k, nullptr, pen), "mcrt_autogain_frames");
        gains = download<float>(k, F * max_rows);
        pens = download<uint32_t>(pen, F);
    }
    const std::vector<float> &gain_curve() const { return gains; }                 // the last autogain()'s row gains, [frames][max_rows]
    const std::vector<uint32_t> &penetration_rows() const { return pens; }         // ... and penetration depths [frames], in rows
    static constexpr double row_mm() { return (double)axial_resolution_um / 1000.0; }   // the RF row pitch [mm]
    double penetration_mm(size_t frame = 0) const { return (double)pens.at(frame) * row_mm(); }   // ... in mm: rows times the row pitch
    // speckle reduction (mcrt.h: mcrt_speckle_frames): speckle-reducing anisotropic diffusion over the enveloped image -- the views of a
    // compounded frame, the planes of a sweep --, in place; it goes after envelope() and before whatever makes the picture
    void despeckle(const mcrt_speckle_opts &o)
    {
        const image_set s = traced();
        check(mcrt_speckle_frames(dev->ctx, s.dev, s.images, columns, max_rows, &o, s.dev), "mcrt_speckle_frames");
    }
    // the views of trace(frame, transducer, steer_rad) compounded into the float picture scan_converted() / save() read (mcrt_compound_frames):
    // every pixel the mean of the views that cover it; with opts (mcrt_compound_opts: weights per view, a lateral edge ramp, max or median)
    // through mcrt_compound_frames_opts
    void postprocess(const std::vector<float> &steer_rad, const mcrt_compound_opts *opts = nullptr)
    {
        const mcrt_compound cp = compound_of(steer_rad);
        if (opts) check(mcrt_compound_frames_opts(dev->ctx, stack.as<float>(), 1, columns, max_rows, radius_mm, angle, &cp, scan.as<float>(), 400, 500, opts), "mcrt_compound_frames_opts");
        else check(mcrt_compound_frames(dev->ctx, stack.as<float>(), 1, columns, max_rows, radius_mm, angle, &cp, scan.as<float>(), 400, 500), "mcrt_compound_frames");
    }
    void postprocess() { to_device(); check(mcrt_scan_convert(dev->ctx, rf.as<float>(), columns, max_rows, radius_mm, angle, scan.as<float>(), 400, 500), "mcrt_scan_convert"); }
    // the displayed picture instead of the float scan conversion: log compression (dynamic range, gain, TGC) and 8-bit grey on the GPU
    // (mcrt_bmode_frames; rfimage.h:131-136 planned it).  tgc_db: max_rows dB values or nullptr.  The persistence state lives here and is
    // carried from one call to the next: it starts afresh on the first call and whenever bp.reset_state is set (mcrt_default_bmode sets it;
    // pass 0 to smooth across frames).  The size is bp.out_rows x bp.out_cols; the sector is this image's own (the constructor's radius and
    // angle, as postprocess() uses: bp.radius_mm / total_angle_rad are not read).  save_bmode() writes the last frame.
    void postprocess(const mcrt_bmode_params &bp, const float *tgc_db = nullptr)
    {
        to_device();
        const mcrt_bmode_params p = bmode_prepare(bp);
        check(mcrt_bmode_frames(dev->ctx, rf.as<float>(), 1, columns, max_rows, &p, tgc_db, state.as<float>(), nullptr, bmode_buf.as<uint8_t>()), "mcrt_bmode_frames");
        state_valid = true; bmode_rows = bp.out_rows; bmode_cols = bp.out_cols;
    }
    // the same over the views of trace(frame, transducer, steer_rad) (mcrt_bmode_compound_frames): one reference per frame, the peak of all views
    // (opts: as above, through mcrt_bmode_compound_frames_opts)
    void postprocess(const mcrt_bmode_params &bp, const std::vector<float> &steer_rad, const float *tgc_db = nullptr, const mcrt_compound_opts *opts = nullptr)
    {
        const mcrt_compound cp = compound_of(steer_rad);
        const mcrt_bmode_params p = bmode_prepare(bp);
        float *views = stack.as<float>(), *st = state.as<float>(); uint8_t *out = bmode_buf.as<uint8_t>();
        if (opts) check(mcrt_bmode_compound_frames_opts(dev->ctx, views, 1, columns, max_rows, &p, &cp, tgc_db, st, nullptr, out, opts), "mcrt_bmode_compound_frames_opts");
        else check(mcrt_bmode_compound_frames(dev->ctx, views, 1, columns, max_rows, &p, &cp, tgc_db, st, nullptr, out), "mcrt_bmode_compound_frames");
        state_valid = true; bmode_rows = bp.out_rows; bmode_cols = bp.out_cols;
    }
    // the planes of trace(frame, transducer, sweep) gathered at grid's points (mcrt_volume_frames): floats [nw][nv][nu], a volume or any cut.
    // filter: 3-D speckle reduction over the block on the device, in place, before it is copied (mcrt.h: mcrt_speckle_volume_frames;
    // mcrt_speckle3d_weights gives the weights of grid's pitches)
    std::vector<float> volume(const mcrt_volume_grid &grid, const mcrt_speckle3d_opts *filter = nullptr)
    {
        const size_t n = volume_prepare(grid, sizeof(float));
        check(mcrt_volume_frames(dev->ctx, stack.as<float>(), 1, columns, max_rows, radius_mm, angle, &sweep, &grid, points.as<float>()), "mcrt_volume_frames");
        if (filter) check(mcrt_speckle_volume_frames(dev->ctx, points.as<float>(), 1, grid.nu, grid.nv, grid.nw, filter, points.as<float>()), "mcrt_speckle_volume_frames");
        return download<float>(points, n);
    }
    // the same as the displayed 8-bit voxels (mcrt_bmode_volume_frames): one reference per volume, the peak of the whole sweep.  The sector is
    // this image's own; bp.out_rows / out_cols are not read (the picture is the grid's) and bp.persistence must be 0
    std::vector<unsigned char> volume(const mcrt_bmode_params &bp, const mcrt_volume_grid &grid, const float *tgc_db = nullptr)
    {
        const size_t n = volume_prepare(grid, 1);
        mcrt_bmode_params p = bp;
        p.radius_mm = radius_mm; p.total_angle_rad = angle;
        check(mcrt_bmode_volume_frames(dev->ctx, stack.as<float>(), 1, columns, max_rows, &p, &sweep, &grid, tgc_db, nullptr, points.as<uint8_t>()), "mcrt_bmode_volume_frames");
        return download<unsigned char>(points, n);
    }
    // volume rendering (mcrt.h: mcrt_render_frames): the displayed voxels of volume(bp, grid) seen through `view` -- mcrt_render_view_for_grid's, or
    // twelve floats filled by hand -- as the bytes of the picture [view.ny][view.nx].  The voxels stay on the device.  opts: null = the defaults
    // for a byte block (the surface view); bp: null = mcrt_default_bmode; the sector is this image's own, as in volume(bp, grid)
    std::vector<unsigned char> render(const mcrt_volume_grid &grid, const mcrt_render_view &view, const mcrt_render_opts *opts = nullptr,
                                      const mcrt_bmode_params *bp = nullptr, const float *tgc_db = nullptr)
    {
        return download<unsigned char>(rendered, render_pass(grid, view, opts, bp, tgc_db, false));
    }
    // the ground truth of render(...) (mcrt.h: mcrt_render_label_frames): the same rendering with its depth buffer kept, the label block of
    // label_volume(grid), and the label of the voxel every pixel shows -- bytes [view.ny][view.nx], MCRT_LABEL_NONE where the ray saw nothing
    // (every pixel of the mean view) or saw it outside the sweep.  It needs labels(transducer) after trace(frame, transducer, sweep), as
    // label_volume() does, with its known stale cases.  picture: the rendering itself, when asked for (the bytes render() returns)
    std::vector<unsigned char> render_labels(const mcrt_volume_grid &grid, const mcrt_render_view &view, const mcrt_render_opts *opts = nullptr,
                                             const mcrt_bmode_params *bp = nullptr, const float *tgc_db = nullptr, std::vector<unsigned char> *picture = nullptr)
    {
        volume_prepare(grid, 1);
        if (label_planes != sweep.n_planes) throw std::invalid_argument("rf_image::render_labels: labels(transducer) after trace(frame, transducer, sweep) first");
        const size_t npix = render_pass(grid, view, opts, bp, tgc_db, true);
        if (picture) *picture = download<unsigned char>(rendered, npix);
        float *depth_dev = rendered.as<float>() + (npix + 3) / 4;
        check(mcrt_label_volume_frames(dev->ctx, label_tissue, 1, columns, max_rows, radius_mm, angle, &sweep, &grid, points.as<uint8_t>()), "mcrt_label_volume_frames");   // (the voxels are rendered: the block is free)
        check(mcrt_render_label_frames(dev->ctx, points.as<uint8_t>(), 1, grid.nu, grid.nv, grid.nw, &view, depth_dev, rendered.as<uint8_t>()), "mcrt_render_label_frames");
        return download<unsigned char>(rendered, npix);
    }
    // ground-truth label maps (mcrt.h: mcrt_label_frames): the central beam of every scan-line of t walked through the scene -- of the K planes of
    // the sweep when the last trace was trace(frame, transducer, sweep), else of t's own plane, whatever was traced before (the unsteered probe
    // of a compounded frame, the probe's own plane of an elevation pass).  opts: null = the tracer's rule at the tracer's start offset.  The
    // maps stay on the device for label_picture() / label_volume(grid).  With several GPUs the pass runs on rank 0's context, which shares the
    // root's GPU, and is waited for here.
    struct label_maps {
        uint32_t planes = 1;                     // the leading axis of the three tables: 1, or the sweep's K
        std::vector<unsigned char> tissue;       // [planes][columns][max_rows]  material index per scan-line sample
        std::vector<int32_t> interface;          // [planes][columns][max_rows]  mesh id of the boundary in a sample, -1: none
        std::vector<uint32_t> crossings;         // [planes][columns]            boundaries per scan-line; bit 31: stopped at the cap
    };
    template <size_t N> label_maps labels(const transducer<N> &t, const mcrt_label_opts *opts = nullptr)
    {
        const beam_poses b = central_beams(t);
        const uint32_t K = b.planes;
        const size_t lines = (size_t)K * columns, taps = lines * max_rows;
        label.reserve(taps + 4 * taps + 4 * lines);      // bytes: tissue, interface, crossings
        unsigned char *tissue_dev = label.as<unsigned char>() + 4 * taps + 4 * lines;      // (the 32-bit tables first: aligned)
        int32_t *interface_dev = label.as<int32_t>(); uint32_t *crossings_dev = label.as<uint32_t>() + taps;
        mcrt_ctx *tracer = dev->tracer();
        check(mcrt_label_frames(tracer, K, 0, columns, b.pos.data(), b.dir.data(), opts, tissue_dev, interface_dev, crossings_dev), "mcrt_label_frames");
        check(mcrt_synchronize(tracer), "mcrt_synchronize");
        label_maps m;
        m.planes = K;
        m.tissue = download<unsigned char>(tissue_dev, taps); m.interface = download<int32_t>(interface_dev, taps); m.crossings = download<uint32_t>(crossings_dev, lines);
        labelled = K == 1 ? labels_of::one_plane : labels_of::sweep_planes; label_planes = K; label_tissue = tissue_dev;
        return m;
    }
    // the tissue map of labels() scan-converted like the picture, nearest neighbour (mcrt_label_scan_convert_frames): bytes [400][500],
    // MCRT_LABEL_NONE outside the sector.  The interface map has no picture: a one-row arc does not survive a nearest gather
    std::vector<unsigned char> label_picture()
    {
        if (labelled != labels_of::one_plane || holds == stack_of::sweep_planes) throw std::invalid_argument("rf_image::label_picture: labels(transducer) of an unswept probe first");
        points.reserve(400 * 500);
        check(mcrt_label_scan_convert_frames(dev->ctx, label_tissue, 1, columns, max_rows, radius_mm, angle, points.as<uint8_t>(), 400, 500), "mcrt_label_scan_convert_frames");
        return download<unsigned char>(points, 400 * 500);
    }
    // the tissue maps of labels() over a sweep gathered at grid's points (mcrt_label_volume_frames): bytes [nw][nv][nu], the labels of volume(grid).
    // Only the plane count is compared, so two stale tables pass (known, kept): the labels of a K-plane sweep after a re-trace with the same K
    // and another step, and the labels of the unswept probe under a 1-plane sweep.
    std::vector<unsigned char> label_volume(const mcrt_volume_grid &grid)
    {
        const size_t n = volume_prepare(grid, 1);
        if (label_planes != sweep.n_planes) throw std::invalid_argument("rf_image::label_volume: labels(transducer) after trace(frame, transducer, sweep) first");
        check(mcrt_label_volume_frames(dev->ctx, label_tissue, 1, columns, max_rows, radius_mm, angle, &sweep, &grid, points.as<uint8_t>()), "mcrt_label_volume_frames");
        return download<unsigned char>(points, n);
    }
    // acoustic ground truth (mcrt.h: mcrt_transmit_frames): the tracer's intensity carried along the central beam of every scan-line of t -- the
    // probe and the planes are labels()' own --: the fraction of the emitted intensity that arrives at every sample, the fraction the boundary in
    // a sample turns back, the boundaries per scan-line.  opts: null = everything (attenuation and boundaries) under the tracer's rule at the
    // tracer's start offset.  The stack stays on the device for transmission_picture(); with several GPUs the pass runs on rank 0's context.
    struct transmission_maps {
        uint32_t planes = 1;                     // the leading axis of the three tables: 1, or the sweep's K
        std::vector<float> transmit;             // [planes][columns][max_rows]  what arrives, 1 at the probe
        std::vector<float> reflect;              // [planes][columns][max_rows]  what the boundary in a sample turns back, 0: none
        std::vector<uint32_t> crossings;         // [planes][columns]            boundaries per scan-line; bit 31: stopped at the cap
    };
    template <size_t N> transmission_maps transmission(const transducer<N> &t, const mcrt_transmit_opts *opts = nullptr)
    {
        const beam_poses b = central_beams(t);
        const uint32_t K = b.planes;
        const size_t lines = (size_t)K * columns, taps = lines * max_rows;
        sound.reserve(4 * (2 * taps + lines));      // transmit, reflect, crossings
        float *transmit_dev = sound.as<float>(), *reflect_dev = transmit_dev + taps; uint32_t *crossings_dev = sound.as<uint32_t>() + 2 * taps;
        mcrt_ctx *tracer = dev->tracer();
        check(mcrt_transmit_frames(tracer, K, 0, columns, b.pos.data(), b.dir.data(), opts, transmit_dev, reflect_dev, crossings_dev), "mcrt_transmit_frames");
        check(mcrt_synchronize(tracer), "mcrt_synchronize");
        transmission_maps m;
        m.planes = K;
        m.transmit = download<float>(transmit_dev, taps); m.reflect = download<float>(reflect_dev, taps); m.crossings = download<uint32_t>(crossings_dev, lines);
        sound_planes = K;
        return m;
    }
    // the transmit map of transmission() scan-converted like the float picture (mcrt_scan_convert_frames): floats [400][500], 0 outside the
    // sector (label_picture() == MCRT_LABEL_NONE is the mask).  The reflect map has no picture: a one-row arc does not survive scan conversion
    std::vector<float> transmission_picture()
    {
        if (sound_planes != 1 || holds == stack_of::sweep_planes) throw std::invalid_argument("rf_image::transmission_picture: transmission(transducer) of an unswept probe first");
        points.reserve(sizeof(float) * 400 * 500);
        check(mcrt_scan_convert_frames(dev->ctx, sound.as<float>(), 1, columns, max_rows, radius_mm, angle, points.as<float>(), 400, 500), "mcrt_scan_convert_frames");
        return download<float>(points, 400 * 500);
    }
    std::vector<unsigned char> bmode() const { return download<unsigned char>(bmode_buf, bmode_n); }   // the last postprocess(bmode_params) frame, row-major [out_rows][out_cols]
    void save_bmode(const std::string &filename) const { write_pgm(filename, bmode_cols, bmode_rows, bmode()); }   // that frame as a binary PGM, the bytes as they are
    void show() const {}   // rfimage.h:150-158 opens an OpenCV window and blocks on a key: out of scope
    std::vector<float> intensities() const   // row-major [max_rows][columns], the cv::Mat of rfimage.h:217
    {
        return where == on_host ? host : export_rf(rf.as<float>());
    }
    std::vector<float> view_intensities(uint32_t n) const   // view n of the last compounded trace, row-major [max_rows][columns]
    {
        if (n >= n_views) throw std::out_of_range("rf_image::view_intensities");
        return export_rf(stack.as<float>() + (size_t)n * columns * max_rows);
    }
    std::vector<float> scan_converted() const { return download<float>(scan, 400 * 500); }
    void save(const std::string &filename) const { write_pgm(filename, 500, 400, to_bytes(scan_converted())); }   // rfimage.h:142-148 writes an 8-bit image; here: binary PGM
    std::shared_ptr<device> dev;
private:
    enum class stack_of { nothing, views, sweep_planes, tracked_frames };
    // the device images a stage acts on: `images` of them from dev on, as `frames` frames of `per_frame` each, the first with the id first_id.
    // traced() and pending() are the only place that reads n_views, holds, banded, first_id and where together
    struct image_set { float *dev; uint32_t images, frames, per_frame, first_id; };
    // what the last trace() left: the RF image (uploaded if it is on the host) as one image of one frame; or the stack's n_views images -- one
    // frame of n_views (one receiver), or with tracked frames n_views frames of one
    image_set traced()
    {
        if (!n_views) { to_device(); return { rf.as<float>(), 1u, 1u, 1u, first_id }; }
        const bool own = holds == stack_of::tracked_frames;
        return { stack.as<float>(), n_views, own ? n_views : 1u, own ? 1u : n_views, first_id };
    }
    // traced(); while band images wait for envelope() / fold_bands() the band stack instead: B per image of the same frame, image i's band b with the
    // id (first id + i) * B + b
    image_set pending()
    {
        const image_set s = traced();
        return banded ? image_set{ band_stack.as<float>(), s.images * banded, s.frames, s.per_frame * banded, s.first_id * banded } : s;
    }
    // the tail of every trace(): what the stack holds now, how many images, the first one's id; no sigma, no band images
    void traced_as(stack_of what, uint32_t n, uint32_t id) { holds = what; n_views = n; first_id = id; sigma_frames = 0; banded = 0; }
    uint8_t *flow_tissue() { return flow_in.as<uint8_t>() + 4 * 6 * (size_t)columns * max_rows; }      // flow_in's tissue bytes, behind its floats
    double flow_frequency = 0.0;
    // labels() / transmission(): the poses whose central beams they walk -- the K planes of the sweep when the last trace was a sweep, else t's own plane
    struct beam_poses { uint32_t planes; std::vector<float> pos, dir; };
    template <size_t N> beam_poses central_beams(const transducer<N> &t)
    {
        static_assert(N == columns, "one scan-line per transducer element");
        shape_params();
        if (holds != stack_of::sweep_planes) return { 1u, t.pos, t.dir };
        auto tab = t.swept(sweep);
        return { sweep.n_planes, std::move(tab.pos), std::move(tab.dir) };
    }
    static size_t grid_points(const mcrt_volume_grid &grid, const char *who)   // the points of a grid; 0 or 2^31 and more: it throws
    {
        const size_t n = (size_t)grid.nu * grid.nv * grid.nw;
        if (n == 0 || n >= ((size_t)1 << 31)) throw std::invalid_argument(std::string("rf_image::") + who + ": the grid needs 1 .. 2^31 - 1 points");
        return n;
    }
    // the length of a row of a scan-line [mm] as reconstruct() bins it: depth_mm_f / max_rows, the row pitch of volume(grid)'s maps
    static double row_pitch_mm() { return (double)((float)(uint32_t)(max_travel_time_us * speed_of_sound) * 0.001f) / (double)max_rows; }
    void to_device()
    {
        if (where == on_host) { check(mcrt_import_rf(dev->ctx, host.data(), columns, max_rows, rf.as<float>()), "mcrt_import_rf"); where = on_device; }
    }
    void to_host()
    {
        if (where == on_device) { host = export_rf(rf.as<float>()); where = on_host; }
    }
    std::vector<float> export_rf(const float *img) const   // one device image [columns][max_rows] as the host's [max_rows][columns]
    {
        std::vector<float> h((size_t)columns * max_rows);
        check(mcrt_export_rf(dev->ctx, img, columns, max_rows, h.data()), "mcrt_export_rf");
        return h;
    }
    template <typename T> std::vector<T> download(const void *src, size_t n) const   // n elements of T from device memory
    {
        std::vector<T> h(n);
        if (n) check(mcrt_memcpy_d2h(dev->ctx, h.data(), src, n * sizeof(T)), "mcrt_memcpy_d2h");
        return h;
    }
    template <typename T> std::vector<T> download(const device_buffer &b, size_t n) const { return download<T>(b.as<const void>(), n); }
    // this image's shape in the context's parameters: the image's shape is the kernel's, rows from THIS image's template arguments
    void shape_params()
    {
        mcrt_params p; check(mcrt_get_params(dev->ctx, &p), "mcrt_get_params");
        if (p.n_rows != max_rows || p.n_elements != columns) {
            p.n_rows = max_rows; p.n_elements = columns; p.speed_of_sound = speed_of_sound;
            check(dev->set_params(&p), "mcrt_set_params");
        }
    }
    // one pose pass of n images into buf [n][columns][max_rows] (grown, never shrunk), image k with frame id frame_id * n + k
    template <typename tables_> void pose_pass(uint32_t frame_id, uint32_t n, const tables_ &t, device_buffer &buf, const char *overflow)
    {
        if ((uint64_t)frame_id * n + n > 0xffffffffull) throw std::out_of_range(overflow);
        shape_params();
        buf.reserve(sizeof(float) * n * columns * max_rows);
        check(dev->trace_frames_poses(frame_id * n, n, columns, t.pos.data(), t.dir.data(), buf.as<float>()), "mcrt_trace_frames_poses");
    }
    // the buffers of postprocess(bmode_params ...) for bp's size -- exactly that size: another size reallocates both and forgets the state --,
    // and bp with this image's sector and the reset rule applied
    mcrt_bmode_params bmode_prepare(const mcrt_bmode_params &bp)
    {
        const size_t n = (size_t)bp.out_rows * bp.out_cols;
        if (n != bmode_n) {
            bmode_buf.release(); state.release();
            bmode_buf.reserve(n); state.reserve(sizeof(float) * n);
            bmode_n = n; state_valid = false;
        }
        mcrt_bmode_params p = bp;
        p.radius_mm = radius_mm; p.total_angle_rad = angle;
        p.reset_state = (bp.reset_state || !state_valid) ? 1u : 0u;
        return p;
    }
    // before volume() / label_volume(): the stack holds a sweep's planes, and `points` has room for grid's points of `size` bytes each; returns their number
    size_t volume_prepare(const mcrt_volume_grid &grid, size_t size)
    {
        if (holds != stack_of::sweep_planes) throw std::invalid_argument("rf_image::volume: trace(frame, transducer, sweep) first");
        const size_t n = grid_points(grid, "volume");
        points.reserve(n * size);
        return n;
    }
    // render() / render_labels(): grid's displayed voxels into `points`, their picture into `rendered` -- npix bytes, then with want_depth the
    // depth buffer, npix floats from the next word on; returns npix
    size_t render_pass(const mcrt_volume_grid &grid, const mcrt_render_view &view, const mcrt_render_opts *opts, const mcrt_bmode_params *bp, const float *tgc_db, bool want_depth)
    {
        volume_prepare(grid, 1);
        const size_t npix = (size_t)view.nx * view.ny;
        if (npix == 0) throw std::invalid_argument("rf_image::render: the view has no pixels");
        mcrt_bmode_params p;
        if (bp) p = *bp; else mcrt_default_bmode(&p);
        p.radius_mm = radius_mm; p.total_angle_rad = angle;
        check(mcrt_bmode_volume_frames(dev->ctx, stack.as<float>(), 1, columns, max_rows, &p, &sweep, &grid, tgc_db, nullptr, points.as<uint8_t>()), "mcrt_bmode_volume_frames");
        rendered.reserve(want_depth ? 4 * ((npix + 3) / 4) + 4 * npix : npix);
        check(mcrt_render_frames(dev->ctx, points.as<uint8_t>(), 1, 1, grid.nu, grid.nv, grid.nw, &view, opts, nullptr, rendered.as<uint8_t>(),
                                 want_depth ? rendered.as<float>() + (npix + 3) / 4 : nullptr), "mcrt_render_frames");
        return npix;
    }
    mcrt_compound compound_of(const std::vector<float> &steer_rad) const
    {
        if (holds != stack_of::views || steer_rad.size() != n_views) throw std::invalid_argument("rf_image::postprocess: the steer list is not the one the views were traced with");
        mcrt_compound cp{};
        cp.n_views = n_views;
        for (uint32_t n = 0; n < n_views; n++) cp.steer_rad[n] = steer_rad[n];
        return cp;
    }
    double radius_mm, angle;
    std::vector<float> host;                     // [max_rows][columns]
    enum { on_host, on_device } where = on_host;
    device_buffer rf, scan;                      // the RF image [columns][max_rows] and the float picture [400][500]
    device_buffer bmode_buf, state;              // postprocess(bmode_params): the 8-bit frame and the persistence state
    size_t bmode_n = 0; uint32_t bmode_rows = 0, bmode_cols = 0; bool state_valid = false;
    device_buffer planes;                        // trace(frame, transducer, psf): the plane stack [K][columns][max_rows]
    device_buffer stack;                         // trace(frame, transducer, steer_rad | sweep): the images [n_views][columns][max_rows]
    stack_of holds = stack_of::nothing;          // ... what the last trace left in it
    uint32_t n_views = 0;                        // ... and how many (nothing: 0)
    uint32_t first_id = 0;                       // the frame id the last trace() gave its first image (add_noise: the noise streams' ids)
    uint32_t sigma_frames = 0;                   // ... the frames sigma holds since the last trace() (0: add_noise() has not run)
    std::vector<float> gains; std::vector<uint32_t> pens;   // autogain()'s by-products on the host
    mcrt_sweep sweep{ 0, 0.0f, 0.0f };           // ... the sweep of sweep_planes
    struct pose_tables { std::vector<float> pos, dir; } tracked;   // ... the poses of tracked_frames, [n_views][columns][3] each
    device_buffer points;                        // volume(), label_picture(), label_volume(): the gathered points, floats or bytes
    device_buffer rendered;                      // render(), render_labels(): the picture's bytes (then the depth buffer)
    device_buffer label;                         // labels(): interface, crossings and tissue tables in one allocation; reconstruct_labels(): the tissue stack
    enum class labels_of { nothing, one_plane, sweep_planes } labelled = labels_of::nothing;   // ... what they hold (one_plane: a 1-plane sweep's too)
    uint32_t label_planes = 0; const unsigned char *label_tissue = nullptr;   // ... their leading axis (nothing: 0) and the tissue table
    device_buffer sound;                         // transmission(): the transmit, reflect and crossings tables in one allocation
    device_buffer sigma, curve;                  // add_noise(): every frame's sigma; autogain(): the row gains and the penetration depths
    device_buffer band_stack;                    // convolve(p) with p.has_bands(): the band images [images][B][columns][max_rows] (grown, never shrunk)
    device_buffer flow_in, flow_out;             // flow_split() / flow(): tissue, the two parts and their I/Q pairs; the correlation, vel, var, truth and the gathered pictures
    std::vector<float> flow_vel, flow_dir;       // flow_split()'s velocities and scan-line directions, for flow()'s phasors
    bool flow_detected = false;                  // flow() has left the two parts' I/Q pairs in flow_in since the last flow_split()
    device_buffer spectral_buf;                  // spectral_series() / spectrum() / sonogram(): the series [T][2], then power [n_cols][N], mean [n_cols] and the bytes
    uint32_t spectral_T = 0, spectral_cols = 0, spectral_N = 0;   // ... the shapes of what it holds (0: nothing yet)
    device_buffer strain_buf, strain_pic;        // compress() / track(): the pairs, the post-compression pairs, five maps and the tissue bytes; elastogram(): the gathered pictures and the rgb bytes
    device_buffer shear_buf, shear_pic;          // shear_wave() / shear_speed(): the pairs, seven maps and the tissue bytes; shear_elastogram(): the gathered pictures and the rgb bytes
    std::vector<float> shear_pitch_mm; int shear_stage = 0;   // shear_wave()'s pitch table [max_rows]; 0: nothing yet, 1: shear_wave() has run, 2: shear_speed() since
    device_buffer mmode_buf, mmode_pic;          // m_lines(): the pairs, the pulses' envelopes, displacements and labels and the tissue bytes; m_mode(): the three pictures
    uint32_t mmode_pulses = 0;                   // the pulses m_lines() left on the device; 0: nothing yet
    double strain_cycles = 0.0; bool strain_tracked = false;   // compress()'s carrier (0: it has not run); track() has run since
    uint32_t banded = 0;                         // ... B while they wait there for envelope() / fold_bands() (0: the images are where trace() left them)
    std::vector<float> band_w;                   // ... and the bands' weights [max_rows][B] they are folded with
    uint32_t sound_planes = 0;                   // ... their leading axis (nothing yet: 0)
};

}  // namespace mcrt_host
