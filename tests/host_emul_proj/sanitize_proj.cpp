// TEST INFRASTRUCTURE.  A stand-alone program for the host sanitizers (`make sanitize_proj` builds it with
// -fsanitize=address,undefined; it runs on the CPU and touches no device): the scene host's checks of a version-9
// description (smallvcm_amd/csrc/scene_host.h scene_host_set_projection) on ordinary and on hostile camera models, the
// frame it derives, and the `projection` directive of the scene-file loader (smallvcm_amd/csrc/scene_file.cpp) on good
// and malformed files.  Prints "ok" and returns 0; a wrong answer returns 1, a sanitizer report aborts.
//
//   sanitize_proj <directory to write scene files into>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "../../smallvcm_amd/csrc/scene_host.h"

using namespace vcm;

static int g_failed;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "sanitize_proj: line %d: %s\n", __LINE__, #cond); g_failed = 1; } } while (0)

static void write_file(const std::string &path, const std::string &text)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) { fprintf(stderr, "sanitize_proj: cannot write %s\n", path.c_str()); g_failed = 1; return; }
    fwrite(text.data(), 1, text.size(), f);
    fclose(f);
}

/* the description through the scene host: "" or the refusal */
static std::string host_verdict(const vcm_scene_desc9 *d, SceneHost *keep)
{
    SceneHost h;
    std::string err;
    if (!scene_host_from_desc9(*d, h, err)) return err.empty() ? "refused" : err;
    if (keep) *keep = h;
    return "";
}

static void directive(const std::string &dir)
{
    write_file(dir + "/q.obj", "mtllib q.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nusemtl white\nf 1 2 3 4\n");
    write_file(dir + "/q.mtl", "newmtl white\nKd 0.8 0.8 0.8\n");
    const std::string head = "obj q.obj\ncamera 0 -4 2  0 1 -0.4  0 0 1  50\nlight background 1\n";
    struct Good { const char *line; int kind; float fov; } good[] = {
        { "projection fisheye 180\n", VCM_PROJ_FISHEYE, 180.f }, { "projection fisheye 0.5   # narrow\n", VCM_PROJ_FISHEYE, 0.5f },
        { "projection panorama\n", VCM_PROJ_PANORAMA, 0.f }, { "projection panorama # all around", VCM_PROJ_PANORAMA, 0.f } };
    for (const Good &g : good) {
        write_file(dir + "/s.vcmscene", head + g.line);
        vcm_scene_file *s = vcm_scene_load((dir + "/s.vcmscene").c_str(), 12, 8);
        EXPECT(s != NULL);
        if (!s) continue;
        const vcm_scene_desc9 *d = vcm_scene_file_desc9(s);
        EXPECT(d && d->model && d->model->kind == g.kind && d->model->fovDegrees == g.fov);
        SceneHost h;
        EXPECT(host_verdict(d, &h) == "" && h.projKind == g.kind);
        vcm_scene_file_free(s);
    }
    write_file(dir + "/s.vcmscene", head);
    vcm_scene_file *s = vcm_scene_load((dir + "/s.vcmscene").c_str(), 12, 8);
    EXPECT(s != NULL);
    if (s) { EXPECT(vcm_scene_file_desc9(s)->model == NULL); EXPECT(host_verdict(vcm_scene_file_desc9(s), NULL) == ""); vcm_scene_file_free(s); }
    /* a lens and a projection in one file: the file loads, the scene host refuses */
    write_file(dir + "/s.vcmscene", head + "lens 0.1 3\nprojection panorama\n");
    s = vcm_scene_load((dir + "/s.vcmscene").c_str(), 12, 8);
    EXPECT(s != NULL);
    if (s) { EXPECT(host_verdict(vcm_scene_file_desc9(s), NULL).find("thin lens") != std::string::npos); vcm_scene_file_free(s); }
    /* malformed lines are refused and name their line (the fourth) */
    const char *bad[] = { "projection\n", "projection fisheye\n", "projection fisheye x\n", "projection fisheye 0\n", "projection fisheye 360\n",
                          "projection fisheye -10\n", "projection fisheye nan\n", "projection fisheye inf\n", "projection fisheye 1e999\n",
                          "projection fisheye 90 3\n", "projection panorama 90\n", "projection ortho\n", "projection perspective\n", "projection" };
    for (const char *b : bad) {
        write_file(dir + "/s.vcmscene", head + b);
        s = vcm_scene_load((dir + "/s.vcmscene").c_str(), 12, 8);
        EXPECT(s == NULL);
        if (s) vcm_scene_file_free(s);
        else {
            const std::string e = vcm_scene_load_error();
            EXPECT(e.find("projection") != std::string::npos && e.find(" line 4") != std::string::npos);
        }
    }
    write_file(dir + "/s.vcmscene", head + "projection panorama\nprojection fisheye 90\n");
    s = vcm_scene_load((dir + "/s.vcmscene").c_str(), 12, 8);
    EXPECT(s == NULL);
    if (s) vcm_scene_file_free(s);
    else EXPECT(std::string(vcm_scene_load_error()).find("a second projection") != std::string::npos);
}

static void model_checks()
{
    vcm_material m;
    vcm_make_material(&m);
    m.diffuse[0] = m.diffuse[1] = m.diffuse[2] = 0.5f;
    const float a[3] = { 0, 0, 0 }, b[3] = { 1, 0, 0 }, c[3] = { 1, 1, 0 }, p[3] = { 0, 0, 3 }, i3[3] = { 1, 1, 1 };
    vcm_prim tri;
    vcm_make_triangle(a, b, c, 0, &tri);
    vcm_light l;
    vcm_make_point_light(p, i3, &l);
    int m2l = -1;
    vcm_scene_desc9 d;
    memset(&d, 0, sizeof(d));
    vcm_scene_desc2 &d2 = d.base.base.base.base.base.base.base;
    d2.nPrims = 1; d2.prims = &tri; d2.nMaterials = 1; d2.materials = &m; d2.mat2light = &m2l; d2.nLights = 1; d2.lights = &l;
    d2.backgroundLight = -1;
    vcm_make_scene_sphere(d2.prims, d2.nPrims, d2.sceneCenter, &d2.sceneRadius, &d2.invSceneRadiusSqr);
    const float pos[3] = { 0, -3, 1 }, fwd[3] = { 0.2f, 1, -0.3f }, up[3] = { 0, 0, 1 };
    EXPECT(vcm_make_camera(pos, fwd, up, 45.f, 12, 8, &d2.camera) == 0);
    SceneHost h;
    EXPECT(host_verdict(&d, &h) == "" && h.projKind == VCM_PROJ_PERSPECTIVE);   /* model NULL */
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    struct Case { vcm_camera_model x; const char *text; } cases[] = {
        { { VCM_PROJ_PERSPECTIVE, nan }, "" }, { { VCM_PROJ_FISHEYE, 180.f }, "" }, { { VCM_PROJ_FISHEYE, 359.9f }, "" }, { { VCM_PROJ_FISHEYE, 1e-3f }, "" },
        { { VCM_PROJ_PANORAMA, 0.f }, "" }, { { VCM_PROJ_PANORAMA, nan }, "" },
        { { 3, 90.f }, "unknown" }, { { -1, 90.f }, "unknown" }, { { VCM_PROJ_FISHEYE, 0.f }, "fovDegrees" }, { { VCM_PROJ_FISHEYE, 360.f }, "fovDegrees" },
        { { VCM_PROJ_FISHEYE, -90.f }, "fovDegrees" }, { { VCM_PROJ_FISHEYE, nan }, "fovDegrees" }, { { VCM_PROJ_FISHEYE, inf }, "fovDegrees" } };
    for (const Case &k : cases) {
        d.model = &k.x;
        const std::string v = host_verdict(&d, &h);
        if (!k.text[0]) EXPECT(v == "" && h.projKind == k.x.kind);
        else EXPECT(v.find(k.text) != std::string::npos && v.find("camera model") != std::string::npos);
    }
    /* the frame: orthonormal, f along forward, ex and ey along the raster axes */
    const vcm_camera_model fish = { VCM_PROJ_FISHEYE, 120.f };
    d.model = &fish;
    EXPECT(host_verdict(&d, &h) == "");
    const float *f = h.projF, *x = h.projEx, *y = h.projEy;
    auto dot3 = [](const float *u, const float *v) { return (double)u[0] * v[0] + (double)u[1] * v[1] + (double)u[2] * v[2]; };
    EXPECT(std::fabs(dot3(f, f) - 1) < 1e-6 && std::fabs(dot3(x, x) - 1) < 1e-6 && std::fabs(dot3(y, y) - 1) < 1e-6);
    EXPECT(std::fabs(dot3(f, x)) < 1e-6 && std::fabs(dot3(f, y)) < 1e-6 && std::fabs(dot3(x, y)) < 1e-6);
    EXPECT(y[2] < 0.f);   /* raster +y points down for an upright camera */
    EXPECT(std::fabs(h.projK - 12.0 / (120.0 * 3.14159265358979323846 / 180.0)) < 1e-5 && std::fabs(h.projThetaMax - 1.0471975512) < 1e-6);
    /* a thin lens with either projection */
    const vcm_thin_lens lens = { 0.1f, 3.f }, closed = { 0.f, 3.f };
    d.base.base.base.base.base.lens = &lens;
    EXPECT(host_verdict(&d, NULL).find("thin lens") != std::string::npos);
    const vcm_camera_model persp = { VCM_PROJ_PERSPECTIVE, 0.f };
    d.model = &persp;
    EXPECT(host_verdict(&d, NULL) == "");
    d.model = &fish;
    d.base.base.base.base.base.lens = &closed;   /* a closed lens is the pinhole */
    EXPECT(host_verdict(&d, NULL) == "");
    /* a camera without a forward direction */
    d.base.base.base.base.base.lens = NULL;
    d2.camera.forward[0] = d2.camera.forward[1] = d2.camera.forward[2] = 0.f;
    EXPECT(host_verdict(&d, NULL).find("forward") != std::string::npos);
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: sanitize_proj <directory>\n"); return 2; }
    model_checks();
    directive(argv[1]);
    if (!g_failed) printf("ok\n");
    return g_failed;
}
