// TEST INFRASTRUCTURE.  A stand-alone program for the host sanitizers (`make sanitize_ggx` builds it with
// -fsanitize=address,undefined; it runs on the CPU and touches no device): the scene host's checks of a version-8
// description (smallvcm_amd/csrc/scene_host.h scene_host_set_material_ext) on ordinary and on hostile tables, and the
// `Pr` key of the .mtl loader (smallvcm_amd/csrc/scene_file.cpp) on good and malformed files.  Prints "ok" and returns
// 0; a wrong answer returns 1, a sanitizer report aborts.
//
//   sanitize_ggx <directory to write scene files into>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "../../smallvcm_amd/csrc/scene_host.h"

using namespace vcm;

static int g_failed;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "sanitize_ggx: line %d: %s\n", __LINE__, #cond); g_failed = 1; } } while (0)

static void write_file(const std::string &path, const std::string &text)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) { fprintf(stderr, "sanitize_ggx: cannot write %s\n", path.c_str()); g_failed = 1; return; }
    fwrite(text.data(), 1, text.size(), f);
    fclose(f);
}

static const char *OBJ = "mtllib m.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nusemtl floor\nf 1 2 3 4\n"
                         "v -1 1 0\nv 1 1 0\nv 1 1 2\nusemtl wall\nf 5 6 7\nv 0 0 2\nv 1 0 2\nv 0 1 2\nusemtl lamp\nf -3 -1 -2\n";

/* the loaded file as a version-8 description through the scene host: "" or the refusal */
static std::string host_verdict(const vcm_scene_desc8 *d, size_t *nExt)
{
    SceneHost h;
    std::string err;
    if (!scene_host_from_desc8(*d, h, err)) return err.empty() ? "refused" : err;
    if (nExt) *nExt = h.materialExt.size();
    return "";
}

static void mtl(const std::string &dir)
{
    write_file(dir + "/m.obj", OBJ);
    write_file(dir + "/s.vcmscene", "obj m.obj\ncamera 0 -4 1 0 1 0 0 0 1 45\n");
    /* a Pr material, a Phong one, the emitter */
    write_file(dir + "/m.mtl", "newmtl floor\nKd 0.1 0.2 0.3\nKs 0.9 0.75 0.5\nNs 40\nPr 0.5\nnewmtl wall\nKd 0.5 0.5 0.5\nKs 0.2 0.2 0.2\nNs 30\n"
                               "newmtl lamp\nKe 5 5 5\n");
    vcm_scene_file *s = vcm_scene_load((dir + "/s.vcmscene").c_str(), 8, 8);
    EXPECT(s != NULL);
    if (s) {
        const vcm_scene_desc8 *d = vcm_scene_file_desc8(s);
        const vcm_scene_desc2 *d2 = vcm_scene_file_desc(s);
        EXPECT(d && d->materialExt && d2->nMaterials == 3);
        if (d && d->materialExt) {
            int lobes = 0;
            for (int m = 0; m < d2->nMaterials; m++) {
                const vcm_material_ext &x = d->materialExt[m];
                if (x.ggx[0] == 0.f && x.ggx[1] == 0.f && x.ggx[2] == 0.f) continue;
                lobes++;
                EXPECT(x.ggx[0] == 0.9f && x.ggx[1] == 0.75f && x.ggx[2] == 0.5f && x.alpha == 0.25f);
                EXPECT(d2->materials[m].phong[0] == 0.f && d2->materials[m].diffuse[1] == 0.2f);   /* Ks went to F0, not to Phong */
            }
            EXPECT(lobes == 1);
            size_t nExt = 0;
            EXPECT(host_verdict(d, &nExt) == "" && nExt == 3);
        }
        vcm_scene_file_free(s);
    }
    /* Pr 0: alpha is clamped to 0.01; Pr with illum 3 stays a mirror; Pr without Ks is no lobe */
    write_file(dir + "/m.mtl", "newmtl floor\nKs 1 1 1\nPr 0\nnewmtl wall\nKs 1 1 1\nPr 0.3\nillum 3\nnewmtl lamp\nKe 5 5 5\n");
    s = vcm_scene_load((dir + "/s.vcmscene").c_str(), 8, 8);
    EXPECT(s != NULL);
    if (s) {
        const vcm_scene_desc8 *d = vcm_scene_file_desc8(s);
        const vcm_scene_desc2 *d2 = vcm_scene_file_desc(s);
        EXPECT(d->materialExt != NULL);
        if (d->materialExt) {
            EXPECT(d->materialExt[0].alpha == 0.01f && d->materialExt[0].ggx[0] == 1.f);
            EXPECT(d->materialExt[1].ggx[0] == 0.f && d2->materials[1].mirror[0] == 1.f);
            EXPECT(host_verdict(d, NULL) == "");
        }
        vcm_scene_file_free(s);
    }
    write_file(dir + "/m.mtl", "newmtl floor\nKd 0.5 0.5 0.5\nPr 0.4\nnewmtl wall\nKd 0.5 0.5 0.5\nnewmtl lamp\nKe 5 5 5\n");
    s = vcm_scene_load((dir + "/s.vcmscene").c_str(), 8, 8);
    EXPECT(s != NULL);
    if (s) { EXPECT(vcm_scene_file_desc8(s)->materialExt == NULL); vcm_scene_file_free(s); }
    /* malformed lines are refused and named */
    const char *bad[] = { "Pr\n", "Pr x\n", "Pr -0.1\n", "Pr 1.5\n", "Pr nan\n", "Pr inf\n", "Pr 1e999\n", "Pr" };
    for (const char *b : bad) {
        write_file(dir + "/m.mtl", std::string("newmtl floor\nKs 1 1 1\n") + b);
        s = vcm_scene_load((dir + "/s.vcmscene").c_str(), 8, 8);
        EXPECT(s == NULL);
        if (s) vcm_scene_file_free(s);
        else EXPECT(std::string(vcm_scene_load_error()).find("bad Pr") != std::string::npos);
    }
}

static void ext_checks()
{
    /* one triangle, one material, one point light; then an emissive material */
    vcm_material m;
    vcm_make_material(&m);
    m.diffuse[0] = m.diffuse[1] = m.diffuse[2] = 0.5f;
    const float a[3] = { 0, 0, 0 }, b[3] = { 1, 0, 0 }, c[3] = { 1, 1, 0 }, p[3] = { 0, 0, 3 }, i3[3] = { 1, 1, 1 };
    vcm_prim tri;
    vcm_make_triangle(a, b, c, 0, &tri);
    vcm_light l;
    vcm_make_point_light(p, i3, &l);
    int m2l = -1;
    vcm_scene_desc8 d;
    memset(&d, 0, sizeof(d));
    vcm_scene_desc2 &d2 = d.base.base.base.base.base.base;
    d2.nPrims = 1; d2.prims = &tri; d2.nMaterials = 1; d2.materials = &m; d2.mat2light = &m2l; d2.nLights = 1; d2.lights = &l;
    d2.backgroundLight = -1;
    vcm_make_scene_sphere(d2.prims, d2.nPrims, d2.sceneCenter, &d2.sceneRadius, &d2.invSceneRadiusSqr);
    const float pos[3] = { 0, -3, 1 }, fwd[3] = { 0, 1, 0 }, up[3] = { 0, 0, 1 };
    EXPECT(vcm_make_camera(pos, fwd, up, 45.f, 8, 8, &d2.camera) == 0);
    size_t n = 99;
    EXPECT(host_verdict(&d, &n) == "" && n == 0);   /* materialExt NULL */
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    struct Case { vcm_material_ext x; const char *text; } cases[] = {
        { { { 0.5f, 0.5f, 0.5f }, 0.3f }, "" }, { { { 0.f, 0.f, 0.f }, 0.f }, "" }, { { { 0.f, 0.f, 0.f }, 9.f }, "" },
        { { { 1.f, 1.f, 1.f }, 0.01f }, "" }, { { { 1.f, 0.f, 0.f }, 1.f }, "" },
        { { { nan, 0.5f, 0.5f }, 0.3f }, "not finite" }, { { { 0.5f, 0.5f, 0.5f }, inf }, "not finite" }, { { { 0.f, 0.f, 0.f }, nan }, "not finite" },
        { { { 1.5f, 0.5f, 0.5f }, 0.3f }, "[0, 1]" }, { { { 0.5f, -0.1f, 0.5f }, 0.3f }, "[0, 1]" },
        { { { 0.5f, 0.5f, 0.5f }, 0.005f }, "alpha" }, { { { 0.5f, 0.5f, 0.5f }, 1.5f }, "alpha" }, { { { 0.f, 0.f, 0.1f }, 0.f }, "alpha" } };
    for (const Case &k : cases) {
        d.materialExt = &k.x;
        const std::string v = host_verdict(&d, &n);
        if (!k.text[0]) EXPECT(v == "");
        else EXPECT(v.find(k.text) != std::string::npos && v.find("materialExt[0]") != std::string::npos);
    }
    /* a lobe on a light's material */
    m2l = 0;
    vcm_make_area_light(a, b, c, i3, &l);
    const vcm_material_ext lobe = { { 0.5f, 0.5f, 0.5f }, 0.3f }, none = { { 0.f, 0.f, 0.f }, 0.f };
    d.materialExt = &lobe;
    EXPECT(host_verdict(&d, NULL).find("light") != std::string::npos);
    d.materialExt = &none;
    EXPECT(host_verdict(&d, &n) == "" && n == 0);
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: sanitize_ggx <directory>\n"); return 2; }
    ext_checks();
    mtl(argv[1]);
    if (!g_failed) printf("ok\n");
    return g_failed;
}
