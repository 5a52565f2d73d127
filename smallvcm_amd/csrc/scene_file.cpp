// scene_file.cpp -- scene files for the version-2 scene description (include/smallvcm_amd.h: vcm_scene_load).
//
// The reference has no loader: "Scenes are hard-coded" (README:210), Scene::LoadCornellBox (src/scene.hxx:132-398) is
// the only way a scene comes into being.  This one reads the common denominator of what people have -- Wavefront OBJ
// geometry with an MTL material library -- plus a small text file for what OBJ cannot say (camera, analytic spheres,
// non-area lights), and produces a vcm_scene_desc2 with the library's own constructors (vcm_make_triangle /
// vcm_make_area_light / vcm_make_camera / ...: the reference's constructors restated, scene_cornell.cpp), so a loaded
// scene holds exactly what the reference's Scene would hold for the same numbers.
//
//   .vcmscene   one directive per line, processed IN ORDER (primitive order = list order = tie-break order of
//               Scene::Intersect, geometry.hxx:65-78); '#' starts a comment; paths are relative to the file
//       obj <file.obj>                                   triangles of a Wavefront OBJ (with its mtllib)
//       mtllib <file.mtl>                                materials for the directives below (spheres)
//       sphere cx cy cz radius <material>                Sphere (geometry.hxx:184-192)
//       camera px py pz  fx fy fz  ux uy uz  hfovDeg     Camera::Setup (camera.hxx:37-76)
//       light point px py pz  r g b                      PointLight (lights.hxx:324-328)
//       light directional dx dy dz  r g b                DirectionalLight (lights.hxx:239-243)
//       light spot px py pz  dx dy dz  r g b  outerDeg innerDeg
//                                                        a point light with a cone around (dx, dy, dz): r g b on the axis,
//                                                        full inside the half-angle innerDeg, smoothly to zero at outerDeg
//                                                        (0 < outerDeg <= 180, 0 <= innerDeg <= outerDeg; equal: a hard edge)
//       light sphere cx cy cz radius  r g b              a sphere that emits the radiance r g b outwards: the sphere
//                                                        primitive, a black material of its own and its light
//       light background scale                           BackgroundLight (lights.hxx:404-408)
//       light envmap <file.hdr|file.pfm> scale           an environment map as the background (vcm_scene_desc3,
//                                                        vcm_scene_file_desc3; the image: vcm_envmap_load below)
//       lens apertureRadius focusDistance                a thin lens instead of the pinhole, at most one: radius >= 0
//                                                        and focus distance > 0 in world units, both finite, nothing
//                                                        after them (vcm_scene_desc4, vcm_scene_file_desc4)
//       lightpick uniform|power [uniformMix]             how a light is chosen where a path samples one, at most once:
//                                                        with equal probability (the default) or by emitted power,
//                                                        mixed with the share uniformMix in [0, 1] of the uniform
//                                                        choice (vcm_light_pick, vcm_scene_desc5, vcm_scene_file_desc5)
//       filter tent|bspline radius                       the pixel reconstruction filter, at most once: the support of
//                                                        the offset density in pixels, finite, > 0 and <= 16, nothing
//                                                        after it (vcm_pixel_filter, vcm_scene_desc6,
//                                                        vcm_scene_file_desc6)
//       sampler sobol|philox                             where the paths' random floats come from, at most once: the
//                                                        Owen-scrambled Sobol sequence or the default white noise,
//                                                        nothing after it (vcm_sampler, vcm_scene_desc7,
//                                                        vcm_scene_file_desc7)
//       projection fisheye fovDeg | projection panorama  the camera's projection, at most once: an equidistant fisheye
//                                                        with its field of view across the image width, finite and
//                                                        in (0, 360) degrees, or a 360 x 180 degree equirectangular
//                                                        panorama; nothing after it.  The camera line keeps giving the
//                                                        position and the axes; its fov is not used (vcm_camera_model,
//                                                        vcm_scene_desc9, vcm_scene_file_desc9)
//   .obj        v, f (triangles; polygons are fanned around their first vertex; v, v/vt, v/vt/vn, v//vn; negative
//               = relative indices), usemtl, mtllib; everything else is skipped
//   .mtl        newmtl, Kd -> mDiffuseReflectance, Ks + Ns -> mPhongReflectance / mPhongExponent (materials.hxx:54-65),
//               Pr <r> (roughness, 0 .. 1) -> Ks becomes the F0 of a GGX lobe of alpha = max(r^2, 0.01) instead of a Phong
//               lobe with Ns (vcm_material_ext, vcm_scene_file_desc8); illum mirror and glass keep their meaning;
//               illum 3 | 5 -> mirror: mMirrorReflectance = Ks;  illum 4 | 6 | 7 | 9 -> glass: mIOR = Ni and
//               mMirrorReflectance = Ks;  Ke != 0 -> every triangle of the material is an AreaLight of that intensity:
//               a primitive with a material of its own whose mat2light entry names the light, and no reflectance,
//               as the reference's light box (scene.hxx:333-361)
// A bare .obj loads too (default camera: in front of the bounding sphere, looking along +y, z up, 45 degrees).
//
// Environment maps (vcm_envmap_load): Radiance RGBE -- header "#?RADIANCE" or "#?RGBE", FORMAT=32-bit_rle_rgbe (other
// formats refused), a blank line, the resolution line "-Y H +X W" (the only orientation accepted: rows top-down), then
// H scanlines, each flat (4 bytes per texel) or new-style run-length encoded (2, 2, W >> 8, W & 255, then the four
// channels one after the other in runs); a texel is channel * 2^(E - 136), 0 for E = 0 -- or PFM: "PF", width, height
// and a scale whose sign gives the byte order (< 0 little-endian), then 3 floats per texel, rows BOTTOM-up (flipped
// here).  Sizes 1..8192 x 1..4096; a truncated file, a bad header or a texel that is not finite or negative is refused.
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "smallvcm_amd.h"

struct vcm_scene_file {
    std::vector<vcm_prim> prims;
    std::vector<vcm_material> materials;
    std::vector<int> mat2light;
    std::vector<vcm_light> lights;
    vcm_scene_desc2 desc;
    vcm_envmap *envmap = NULL;        /* `light envmap` */
    vcm_scene_desc3 desc3;
    bool haveLens = false;            /* `lens` */
    vcm_thin_lens lens;
    vcm_scene_desc4 desc4;
    bool havePick = false;            /* `lightpick` */
    vcm_light_pick pick;
    vcm_scene_desc5 desc5;
    bool haveFilter = false;          /* `filter` */
    vcm_pixel_filter filter;
    vcm_scene_desc6 desc6;
    bool haveSampler = false;         /* `sampler` */
    vcm_sampler sampler;
    vcm_scene_desc7 desc7;
    std::vector<vcm_material_ext> materialExt;   /* one per material once a `Pr` material is in use, else empty */
    bool haveGgx = false;
    vcm_scene_desc8 desc8;
    bool haveModel = false;           /* `projection` */
    vcm_camera_model model;
    vcm_scene_desc9 desc9;
    ~vcm_scene_file() { vcm_envmap_free(envmap); }
};

namespace {

thread_local std::string g_sceneError;

/* ---- environment maps ---- */
bool env_fail(const std::string &what) { g_sceneError = what; return false; }
bool env_size_ok(long w, long h) { return w >= 1 && w <= 8192 && h >= 1 && h <= 4096; }
bool read_file(const std::string &path, std::vector<unsigned char> &buf)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return env_fail("cannot open " + path);
    unsigned char tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) {
        buf.insert(buf.end(), tmp, tmp + n);
        if (buf.size() > ((size_t)8192 * 4096 * 12 + 4096)) { fclose(f); return env_fail(path + ": larger than any accepted map"); }
    }
    fclose(f);
    return true;
}
/* the next '\n'-terminated line from pos (without the '\n'); false at the end of the data */
bool next_line(const std::vector<unsigned char> &b, size_t &pos, std::string &line)
{
    if (pos >= b.size()) return false;
    size_t e = pos;
    while (e < b.size() && b[e] != '\n') e++;
    if (e >= b.size()) return false;   /* a header line without its end: truncated */
    line.assign((const char *)&b[pos], e - pos);
    pos = e + 1;
    return true;
}
bool load_rgbe(const std::string &path, const std::vector<unsigned char> &b, std::vector<float> &rgb, int &W, int &H)
{
    size_t pos = 0;
    std::string line;
    if (!next_line(b, pos, line) || (line.compare(0, 10, "#?RADIANCE") != 0 && line.compare(0, 6, "#?RGBE") != 0))
        return env_fail(path + ": not a Radiance file (#?RADIANCE / #?RGBE)");
    for (;;) {
        if (!next_line(b, pos, line)) return env_fail(path + ": truncated header");
        if (line.empty()) break;
        if (line.compare(0, 7, "FORMAT=") == 0 && line != "FORMAT=32-bit_rle_rgbe") return env_fail(path + ": unsupported " + line);
    }
    if (!next_line(b, pos, line)) return env_fail(path + ": no resolution line");
    long h = 0, w = 0;
    char tail = 0;
    if (sscanf(line.c_str(), "-Y %ld +X %ld %c", &h, &w, &tail) != 2) return env_fail(path + ": resolution line '" + line + "' is not -Y H +X W");
    if (!env_size_ok(w, h)) return env_fail(path + ": size outside 1..8192 x 1..4096");
    W = (int)w; H = (int)h;
    rgb.assign((size_t)W * H * 3, 0.f);
    std::vector<unsigned char> scan((size_t)W * 4);
    for (int y = 0; y < H; y++) {
        const bool rle = W >= 8 && W < 32768 && pos + 4 <= b.size() && b[pos] == 2 && b[pos + 1] == 2 && (b[pos + 2] & 0x80) == 0 &&
                         ((int)b[pos + 2] << 8 | b[pos + 3]) == W;
        if (rle) {
            pos += 4;
            for (int c = 0; c < 4; c++) {
                for (int x = 0; x < W;) {
                    if (pos >= b.size()) return env_fail(path + ": truncated scanline " + std::to_string(y));
                    int n = b[pos++];
                    if (n > 128) {
                        n -= 128;
                        if (x + n > W) return env_fail(path + ": run overflows scanline " + std::to_string(y));
                        if (pos >= b.size()) return env_fail(path + ": truncated scanline " + std::to_string(y));
                        const unsigned char v = b[pos++];
                        for (int k = 0; k < n; k++) scan[(size_t)(x++) * 4 + c] = v;
                    } else {
                        if (n == 0 || x + n > W) return env_fail(path + ": bad run in scanline " + std::to_string(y));
                        if (pos + n > b.size()) return env_fail(path + ": truncated scanline " + std::to_string(y));
                        for (int k = 0; k < n; k++) scan[(size_t)(x++) * 4 + c] = b[pos++];
                    }
                }
            }
        } else {
            if (pos + (size_t)W * 4 > b.size()) return env_fail(path + ": truncated scanline " + std::to_string(y));
            memcpy(scan.data(), &b[pos], (size_t)W * 4);
            pos += (size_t)W * 4;
        }
        for (int x = 0; x < W; x++) {
            const unsigned char *t = &scan[(size_t)x * 4];
            const float f = t[3] ? ldexpf(1.f, (int)t[3] - 136) : 0.f;
            for (int c = 0; c < 3; c++) rgb[((size_t)y * W + x) * 3 + c] = t[3] ? (float)t[c] * f : 0.f;
        }
    }
    return true;
}
bool load_pfm(const std::string &path, const std::vector<unsigned char> &b, std::vector<float> &rgb, int &W, int &H)
{
    /* "PF" whitespace width whitespace height whitespace scale, ONE whitespace character, then the data */
    size_t pos = 2;
    std::string tok[3];
    for (int t = 0; t < 3; t++) {
        while (pos < b.size() && isspace(b[pos])) pos++;
        while (pos < b.size() && !isspace(b[pos]) && tok[t].size() < 32) tok[t] += (char)b[pos++];
        if (tok[t].empty() || pos >= b.size()) return env_fail(path + ": truncated PFM header");
    }
    pos++;   /* the single whitespace character after the scale */
    char *end = NULL;
    const long w = strtol(tok[0].c_str(), &end, 10);
    if (*end) return env_fail(path + ": bad PFM width");
    const long h = strtol(tok[1].c_str(), &end, 10);
    if (*end) return env_fail(path + ": bad PFM height");
    const double scale = strtod(tok[2].c_str(), &end);
    if (*end || scale == 0.0 || !std::isfinite(scale)) return env_fail(path + ": bad PFM scale");
    if (!env_size_ok(w, h)) return env_fail(path + ": size outside 1..8192 x 1..4096");
    W = (int)w; H = (int)h;
    const size_t n = (size_t)W * H * 3;
    if (b.size() < pos + n * 4) return env_fail(path + ": truncated PFM data");
    const bool little = scale < 0.0;
    rgb.assign(n, 0.f);
    for (int y = 0; y < H; y++)
        for (size_t k = 0; k < (size_t)W * 3; k++) {
            const unsigned char *q = &b[pos + ((size_t)y * W * 3 + k) * 4];
            const uint32_t u = little ? (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24
                                      : (uint32_t)q[3] | (uint32_t)q[2] << 8 | (uint32_t)q[1] << 16 | (uint32_t)q[0] << 24;
            float f;
            memcpy(&f, &u, 4);
            rgb[(size_t)(H - 1 - y) * W * 3 + k] = f;   /* PFM rows run bottom-up */
        }
    return true;
}
vcm_envmap *envmap_load(const std::string &path)
{
    std::vector<unsigned char> b;
    if (!read_file(path, b)) return NULL;
    std::vector<float> rgb;
    int W = 0, H = 0;
    bool ok;
    if (b.size() >= 3 && b[0] == 'P' && b[1] == 'F' && isspace(b[2])) ok = load_pfm(path, b, rgb, W, H);
    else if (b.size() >= 2 && b[0] == '#' && b[1] == '?') ok = load_rgbe(path, b, rgb, W, H);
    else ok = env_fail(path + ": neither a Radiance .hdr nor a .pfm file");
    if (!ok) return NULL;
    for (size_t i = 0; i < rgb.size(); i++)
        if (!std::isfinite(rgb[i]) || rgb[i] < 0.f) { env_fail(path + ": texel " + std::to_string(i / 3) + " is not finite or negative"); return NULL; }
    float *px = new float[rgb.size()];
    memcpy(px, rgb.data(), rgb.size() * sizeof(float));
    vcm_envmap *m = new vcm_envmap;
    m->width = W; m->height = H; m->rgb = px;
    return m;
}

struct MtlEntry { vcm_material m; float ke[3]; bool emissive; int index; /* in materials, -1: not added yet */ vcm_material_ext x; /* `Pr`: its GGX lobe, else zero */ };

struct Loader {
    vcm_scene_file *out;
    std::map<std::string, MtlEntry> mtl;
    int background;
    bool haveCamera;
    float camPos[3], camFwd[3], camUp[3], camFov;
    Loader() : out(NULL), background(-1), haveCamera(false), camFov(45.f) {}

    bool fail(const std::string &what) { g_sceneError = what; return false; }

    static std::string dir_of(const std::string &path)
    {
        const size_t k = path.find_last_of("/\\");
        return k == std::string::npos ? std::string() : path.substr(0, k + 1);
    }
    static bool ends_with(const std::string &s, const char *suffix)
    {
        const size_t n = strlen(suffix);
        return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
    }
    static bool floats(const char *&p, float *v, int n)
    {
        for (int i = 0; i < n; i++) {
            char *e = NULL;
            v[i] = strtof(p, &e);
            if (e == p) return false;
            p = e;
        }
        return true;
    }
    static std::string word(const char *&p)
    {
        while (*p == ' ' || *p == '\t') p++;
        const char *b = p;
        while (*p && *p != ' ' && *p != '\t' && *p != '\r' && *p != '\n') p++;
        return std::string(b, p);
    }

    int material_index(const std::string &name)
    {   // materials enter the scene when first used: unused library entries cost nothing
        std::map<std::string, MtlEntry>::iterator it = mtl.find(name);
        if (it == mtl.end()) return -1;
        if (it->second.index < 0) {
            it->second.index = (int)out->materials.size();
            out->materials.push_back(it->second.m);
            out->mat2light.push_back(-1);
            const vcm_material_ext &x = it->second.x;
            if (x.ggx[0] != 0.f || x.ggx[1] != 0.f || x.ggx[2] != 0.f) {
                const vcm_material_ext none = { { 0.f, 0.f, 0.f }, 0.f };
                out->materialExt.resize(out->materials.size(), none);
                out->materialExt.back() = x;
                out->haveGgx = true;
            }
        }
        return it->second.index;
    }

    /* one whole line of any length (a polygon with a thousand vertices is one `f` line: a fixed buffer would cut it in
       the middle of an index and read the tail as an unknown key) */
    static bool read_line(FILE *f, std::string &line)
    {
        /* character by character (getc is buffered): a NUL byte inside a line is data like any other -- fgets + strlen lost
           everything between it and the end of the chunk and then glued the next physical line onto this one */
        line.clear();
        bool any = false;
        for (int ch; (ch = getc(f)) != EOF;) {
            any = true;
            line += (char)ch;
            if (ch == '\n') break;
        }
        return any;
    }

    bool load_mtl(const std::string &path)
    {
        FILE *f = fopen(path.c_str(), "r");
        if (!f) return fail("cannot open " + path);
        std::string lineBuf;
        MtlEntry *cur = NULL;
        int illum = 2;
        float ks[3] = { 0, 0, 0 }, ni = 1.f, pr = 0.f;
        bool haveKs = false, havePr = false;
        auto finish = [&]() {
            if (!cur) return;
            const bool mirror = illum == 3 || illum == 5, glass = illum == 4 || illum == 6 || illum == 7 || illum == 9;
            if (mirror || glass) {
                for (int k = 0; k < 3; k++) { cur->m.mirror[k] = haveKs ? ks[k] : 1.f; cur->m.phong[k] = 0.f; }
                if (glass) cur->m.ior = ni;
            } else if (haveKs && havePr) {   /* a GGX lobe: Ks is its F0, Ns is not looked at */
                for (int k = 0; k < 3; k++) cur->x.ggx[k] = ks[k];
                cur->x.alpha = pr * pr < 0.01f ? 0.01f : pr * pr;
            } else if (haveKs) {
                for (int k = 0; k < 3; k++) cur->m.phong[k] = ks[k];
            }
        };
        while (read_line(f, lineBuf)) {
            const char *p = lineBuf.c_str();
            const std::string key = word(p);
            if (key.empty() || key[0] == '#') continue;
            if (key == "newmtl") {
                finish();
                const std::string name = word(p);
                if (mtl.count(name)) { fclose(f); return fail(path + ": material '" + name + "' is defined twice"); }
                MtlEntry e;
                vcm_make_material(&e.m);
                e.ke[0] = e.ke[1] = e.ke[2] = 0.f; e.emissive = false; e.index = -1;
                e.x.ggx[0] = e.x.ggx[1] = e.x.ggx[2] = 0.f; e.x.alpha = 0.f;
                cur = &(mtl[name] = e);
                illum = 2; haveKs = false; ni = 1.f; havePr = false;
            } else if (!cur) {
                continue;
            } else if (key == "Kd") { if (!floats(p, cur->m.diffuse, 3)) { fclose(f); return fail(path + ": bad Kd"); } }
            else if (key == "Ks") { if (!floats(p, ks, 3)) { fclose(f); return fail(path + ": bad Ks"); } haveKs = true; }
            else if (key == "Ns") { if (!floats(p, &cur->m.phongExp, 1)) { fclose(f); return fail(path + ": bad Ns"); } }
            else if (key == "Pr") {
                if (!floats(p, &pr, 1) || !(pr >= 0.f && pr <= 1.f)) { fclose(f); return fail(path + ": bad Pr (a roughness in [0, 1])"); }
                havePr = true;
            }
            else if (key == "Ni") { if (!floats(p, &ni, 1)) { fclose(f); return fail(path + ": bad Ni"); } }
            else if (key == "illum") { illum = atoi(p); }
            else if (key == "Ke") {
                if (!floats(p, cur->ke, 3)) { fclose(f); return fail(path + ": bad Ke"); }
                cur->emissive = cur->ke[0] != 0.f || cur->ke[1] != 0.f || cur->ke[2] != 0.f;
            }
        }
        finish();
        fclose(f);
        return true;
    }

    void add_triangle(const float *a, const float *b, const float *c, const std::string &mtlName, const MtlEntry *e)
    {
        int mat;
        if (e && e->emissive) {   // scene.hxx:333-361: its own material, mat2light -> the AreaLight over the same points
            vcm_material m;
            vcm_make_material(&m);
            mat = (int)out->materials.size();
            out->materials.push_back(m);
            vcm_light l;
            vcm_make_area_light(a, b, c, e->ke, &l);
            out->mat2light.push_back((int)out->lights.size());
            out->lights.push_back(l);
        } else {
            mat = material_index(mtlName);
        }
        vcm_prim p;
        vcm_make_triangle(a, b, c, mat, &p);
        out->prims.push_back(p);
    }

    bool load_obj(const std::string &path)
    {
        FILE *f = fopen(path.c_str(), "r");
        if (!f) return fail("cannot open " + path);
        std::vector<float> v;
        std::string current;
        const MtlEntry *cur = NULL;
        std::string lineBuf;
        long lineNo = 0;
        while (read_line(f, lineBuf)) {
            lineNo++;
            const char *p = lineBuf.c_str();
            const std::string key = word(p);
            if (key == "v") {
                float x[3];
                if (!floats(p, x, 3)) { fclose(f); return fail(path + ": bad vertex at line " + std::to_string(lineNo)); }
                v.insert(v.end(), x, x + 3);
            } else if (key == "mtllib") {
                if (!load_mtl(dir_of(path) + word(p))) { fclose(f); return false; }
            } else if (key == "usemtl") {
                current = word(p);
                std::map<std::string, MtlEntry>::const_iterator it = mtl.find(current);
                if (it == mtl.end()) { fclose(f); return fail(path + ": unknown material " + current); }
                cur = &it->second;
            } else if (key == "f") {
                std::vector<long> idx;
                for (;;) {
                    const std::string w = word(p);
                    if (w.empty()) break;
                    long i = strtol(w.c_str(), NULL, 10);   // the vertex index is what precedes the first '/'
                    const long n = (long)(v.size() / 3);
                    if (i < 0) i = n + i + 1;
                    if (i < 1 || i > n) { fclose(f); return fail(path + ": face index out of range at line " + std::to_string(lineNo)); }
                    idx.push_back(i - 1);
                }
                if (idx.size() < 3) { fclose(f); return fail(path + ": face with fewer than 3 vertices at line " + std::to_string(lineNo)); }
                if (!cur) { fclose(f); return fail(path + ": face before any usemtl at line " + std::to_string(lineNo)); }
                for (size_t k = 1; k + 1 < idx.size(); k++)
                    add_triangle(&v[3 * idx[0]], &v[3 * idx[k]], &v[3 * idx[k + 1]], current, cur);
            }
        }
        fclose(f);
        return true;
    }

    bool load_scene(const std::string &path)
    {
        FILE *f = fopen(path.c_str(), "r");
        if (!f) return fail("cannot open " + path);
        const std::string base = dir_of(path);
        std::string lineBuf;
        long lineNo = 0;
        bool ok = true;
        while (ok && read_line(f, lineBuf)) {
            lineNo++;
            const char *p = lineBuf.c_str();
            const std::string key = word(p);
            const std::string at = path + " line " + std::to_string(lineNo);
            if (key.empty() || key[0] == '#') continue;
            if (key == "obj") ok = load_obj(base + word(p));
            else if (key == "mtllib") ok = load_mtl(base + word(p));
            else if (key == "sphere") {
                float x[4];
                if (!floats(p, x, 4)) { ok = fail(at + ": sphere cx cy cz radius material"); break; }
                const int mat = material_index(word(p));
                if (mat < 0) { ok = fail(at + ": unknown material"); break; }
                vcm_prim s;
                vcm_make_sphere(x, x[3], mat, &s);
                out->prims.push_back(s);
            } else if (key == "camera") {
                float x[10];
                if (!floats(p, x, 10)) { ok = fail(at + ": camera px py pz fx fy fz ux uy uz fov"); break; }
                memcpy(camPos, x, 12); memcpy(camFwd, x + 3, 12); memcpy(camUp, x + 6, 12); camFov = x[9];
                haveCamera = true;
            } else if (key == "lens") {
                float x[2];
                const bool got = floats(p, x, 2);
                const std::string rest = got ? word(p) : std::string();
                if (!got || (!rest.empty() && rest[0] != '#')) { ok = fail(at + ": lens apertureRadius focusDistance"); break; }
                if (out->haveLens) { ok = fail(at + ": a second lens"); break; }
                if (!std::isfinite(x[0]) || x[0] < 0.f) { ok = fail(at + ": lens apertureRadius must be finite and >= 0"); break; }
                if (!std::isfinite(x[1]) || !(x[1] > 0.f)) { ok = fail(at + ": lens focusDistance must be finite and > 0"); break; }
                out->lens.apertureRadius = x[0]; out->lens.focusDistance = x[1];
                out->haveLens = true;
            } else if (key == "lightpick") {
                const std::string mode = word(p);
                if (mode != "uniform" && mode != "power") { ok = fail(at + ": lightpick uniform|power [uniformMix]"); break; }
                if (out->havePick) { ok = fail(at + ": a second lightpick"); break; }
                float mix = 0.f;
                std::string rest = word(p);
                if (!rest.empty() && rest[0] != '#') {
                    char *e = NULL;
                    mix = strtof(rest.c_str(), &e);
                    if (e == rest.c_str() || *e) { ok = fail(at + ": lightpick uniform|power [uniformMix]"); break; }
                    rest = word(p);
                    if (!rest.empty() && rest[0] != '#') { ok = fail(at + ": lightpick uniform|power [uniformMix]"); break; }
                }
                if (!std::isfinite(mix) || mix < 0.f || mix > 1.f) { ok = fail(at + ": lightpick uniformMix must be finite and in [0, 1]"); break; }
                out->pick.mode = mode == "power" ? VCM_LIGHT_PICK_POWER : VCM_LIGHT_PICK_UNIFORM;
                out->pick.uniformMix = mix; out->pick.weights = NULL;
                out->havePick = true;
            } else if (key == "filter") {
                const std::string kind = word(p);
                float x[1];
                const bool got = (kind == "tent" || kind == "bspline") && floats(p, x, 1);
                const std::string rest = got ? word(p) : std::string();
                if (!got || (!rest.empty() && rest[0] != '#')) { ok = fail(at + ": filter tent|bspline radius"); break; }
                if (out->haveFilter) { ok = fail(at + ": a second filter"); break; }
                if (!std::isfinite(x[0]) || !(x[0] > 0.f) || x[0] > 16.f) { ok = fail(at + ": filter radius must be finite, > 0 and <= 16"); break; }
                out->filter.kind = kind == "tent" ? VCM_FILTER_TENT : VCM_FILTER_BSPLINE;
                out->filter.radius = x[0];
                out->haveFilter = true;
            } else if (key == "sampler") {
                const std::string kind = word(p);
                const std::string rest = word(p);
                if ((kind != "sobol" && kind != "philox") || (!rest.empty() && rest[0] != '#')) { ok = fail(at + ": sampler sobol|philox"); break; }
                if (out->haveSampler) { ok = fail(at + ": a second sampler"); break; }
                out->sampler.kind = kind == "sobol" ? VCM_SAMPLER_SOBOL : VCM_SAMPLER_PHILOX;
                out->haveSampler = true;
            } else if (key == "projection") {
                const std::string kind = word(p);
                float x[1] = { 0.f };
                const bool got = kind == "panorama" || (kind == "fisheye" && floats(p, x, 1));
                const std::string rest = got ? word(p) : std::string();
                if (!got || (!rest.empty() && rest[0] != '#')) { ok = fail(at + ": projection fisheye fovDeg | projection panorama"); break; }
                if (out->haveModel) { ok = fail(at + ": a second projection"); break; }
                if (kind == "fisheye" && (!std::isfinite(x[0]) || !(x[0] > 0.f) || !(x[0] < 360.f))) { ok = fail(at + ": projection fisheye fovDeg must be finite and in (0, 360)"); break; }
                out->model.kind = kind == "fisheye" ? VCM_PROJ_FISHEYE : VCM_PROJ_PANORAMA;
                out->model.fovDegrees = x[0];
                out->haveModel = true;
            } else if (key == "light") {
                const std::string kind = word(p);
                vcm_light l;
                float x[11];
                if (kind == "spot") {
                    if (!floats(p, x, 11)) { ok = fail(at + ": light spot px py pz dx dy dz r g b outerDeg innerDeg"); break; }
                    if (!std::isfinite(x[9]) || !(x[9] > 0.f) || x[9] > 180.f) { ok = fail(at + ": light spot outerDeg must be finite, > 0 and <= 180"); break; }
                    if (!std::isfinite(x[10]) || x[10] < 0.f || x[10] > x[9]) { ok = fail(at + ": light spot innerDeg must be finite, >= 0 and <= outerDeg"); break; }
                    vcm_make_spot_light(x, x + 3, x + 6, x[9], x[10], &l);
                } else if (kind == "sphere") {
                    if (!floats(p, x, 7)) { ok = fail(at + ": light sphere cx cy cz radius r g b"); break; }
                    if (!std::isfinite(x[3]) || !(x[3] > 0.f)) { ok = fail(at + ": light sphere radius must be finite and > 0"); break; }
                    vcm_material m;   // its own black material, mat2light -> the light, as an emissive triangle's
                    vcm_make_material(&m);
                    vcm_make_sphere_light(x, x[3], x + 4, &l);
                    vcm_prim s;
                    vcm_make_sphere(x, x[3], (int)out->materials.size(), &s);
                    out->materials.push_back(m);
                    out->mat2light.push_back((int)out->lights.size());
                    out->prims.push_back(s);
                }
                else if (kind == "point" && floats(p, x, 6)) vcm_make_point_light(x, x + 3, &l);
                else if (kind == "directional" && floats(p, x, 6)) vcm_make_directional_light(x, x + 3, &l);
                else if (kind == "background" && floats(p, x, 1)) { vcm_make_background_light(x[0], &l); background = (int)out->lights.size(); }
                else if (kind == "envmap") {
                    const std::string file = word(p);
                    if (file.empty() || !floats(p, x, 1)) { ok = fail(at + ": light envmap <file> scale"); break; }
                    if (out->envmap) { ok = fail(at + ": a second env map"); break; }
                    out->envmap = envmap_load(base + file);
                    if (!out->envmap) { ok = fail(at + ": " + g_sceneError); break; }
                    vcm_make_envmap_light(x[0], &l);
                    background = (int)out->lights.size();
                }
                else { ok = fail(at + ": light point|directional x y z r g b, light spot px py pz dx dy dz r g b outerDeg innerDeg, light sphere cx cy cz radius r g b, light background scale, or light envmap file scale"); break; }
                out->lights.push_back(l);
            } else ok = fail(at + ": unknown directive " + key);
        }
        fclose(f);
        return ok;
    }

    bool finish(int resX, int resY)
    {
        if (out->prims.empty()) return fail("the scene has no primitives");
        if (out->lights.empty()) return fail("the scene has no light (an MTL material with Ke, or a light directive)");
        vcm_scene_desc2 &d = out->desc;
        memset(&d, 0, sizeof(d));
        d.nPrims = (int)out->prims.size(); d.prims = out->prims.data();
        d.nMaterials = (int)out->materials.size(); d.materials = out->materials.data(); d.mat2light = out->mat2light.data();
        d.nLights = (int)out->lights.size(); d.lights = out->lights.data();
        d.backgroundLight = background;
        vcm_make_scene_sphere(d.prims, d.nPrims, d.sceneCenter, &d.sceneRadius, &d.invSceneRadiusSqr);
        if (!haveCamera) {
            camPos[0] = d.sceneCenter[0]; camPos[1] = d.sceneCenter[1] - 2.6f * d.sceneRadius; camPos[2] = d.sceneCenter[2];
            camFwd[0] = 0.f; camFwd[1] = 1.f; camFwd[2] = 0.f;
            camUp[0] = 0.f; camUp[1] = 0.f; camUp[2] = 1.f;
            camFov = 45.f;
        }
        if (vcm_make_camera(camPos, camFwd, camUp, camFov, resX, resY, &d.camera) != 0) return fail("bad camera");
        out->desc3.base = d;
        out->desc3.envmap = out->envmap;
        out->desc4.base = out->desc3;
        out->desc4.lens = out->haveLens ? &out->lens : NULL;
        out->desc5.base = out->desc4;
        out->desc5.pick = out->havePick ? &out->pick : NULL;
        out->desc6.base = out->desc5;
        out->desc6.filter = out->haveFilter ? &out->filter : NULL;
        out->desc7.base = out->desc6;
        out->desc7.sampler = out->haveSampler ? &out->sampler : NULL;
        if (out->haveGgx) { const vcm_material_ext none = { { 0.f, 0.f, 0.f }, 0.f }; out->materialExt.resize(out->materials.size(), none); }
        out->desc8.base = out->desc7;
        out->desc8.materialExt = out->haveGgx ? out->materialExt.data() : NULL;
        out->desc9.base = out->desc8;
        out->desc9.model = out->haveModel ? &out->model : NULL;
        return true;
    }
};

} // namespace

extern "C" {

const char *vcm_scene_load_error(void) { return g_sceneError.c_str(); }

vcm_scene_file *vcm_scene_load(const char *path, int resX, int resY)
{
    g_sceneError.clear();
    if (!path || resX < 1 || resY < 1) { g_sceneError = "vcm_scene_load: bad argument"; return NULL; }
    vcm_scene_file *s = new (std::nothrow) vcm_scene_file();
    if (!s) { g_sceneError = "out of memory"; return NULL; }
    bool ok = false;
    try {   /* nothing may be thrown through the C-ABI (std::string / std::vector / std::map allocate) */
        Loader ld;
        ld.out = s;
        const std::string p(path);
        ok = (Loader::ends_with(p, ".obj") ? ld.load_obj(p) : ld.load_scene(p)) && ld.finish(resX, resY);
    } catch (const std::exception &e) {
        try { g_sceneError = std::string("vcm_scene_load: ") + e.what(); } catch (...) { try { g_sceneError.assign("vcm_scene_load: exception"); } catch (...) {} }
        ok = false;
    } catch (...) {
        try { g_sceneError = "vcm_scene_load: exception"; } catch (...) {}   /* never a stale message from an earlier call */
        ok = false;
    }
    if (!ok) { delete s; return NULL; }
    return s;
}

const vcm_scene_desc2 *vcm_scene_file_desc(const vcm_scene_file *s) { return s ? &s->desc : NULL; }

void vcm_scene_file_free(vcm_scene_file *s) { delete s; }

const vcm_scene_desc3 *vcm_scene_file_desc3(const vcm_scene_file *s) { return s ? &s->desc3 : NULL; }
const vcm_scene_desc4 *vcm_scene_file_desc4(const vcm_scene_file *s) { return s ? &s->desc4 : NULL; }
const vcm_scene_desc5 *vcm_scene_file_desc5(const vcm_scene_file *s) { return s ? &s->desc5 : NULL; }
const vcm_scene_desc6 *vcm_scene_file_desc6(const vcm_scene_file *s) { return s ? &s->desc6 : NULL; }
const vcm_scene_desc7 *vcm_scene_file_desc7(const vcm_scene_file *s) { return s ? &s->desc7 : NULL; }
const vcm_scene_desc8 *vcm_scene_file_desc8(const vcm_scene_file *s) { return s ? &s->desc8 : NULL; }
const vcm_scene_desc9 *vcm_scene_file_desc9(const vcm_scene_file *s) { return s ? &s->desc9 : NULL; }

vcm_envmap *vcm_envmap_load(const char *path)
{
    g_sceneError.clear();
    if (!path) { g_sceneError = "vcm_envmap_load: path is NULL"; return NULL; }
    try {   /* nothing may be thrown through the C-ABI */
        return envmap_load(path);
    } catch (...) {
        try { g_sceneError = "vcm_envmap_load: out of memory"; } catch (...) {}
        return NULL;
    }
}

void vcm_envmap_free(vcm_envmap *m)
{
    if (!m) return;
    delete[] m->rgb;
    delete m;
}

} // extern "C"
