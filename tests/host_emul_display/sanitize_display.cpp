// TEST INFRASTRUCTURE.  A stand-alone program for the host sanitizers (`make sanitize_display` builds it with
// -fsanitize=address,undefined; it runs on the CPU and touches no device): the display flags of vcm_render and the BMP
// file they write (smallvcm_amd/host/vcm_render_display.hpp), and the host-side functions of
// smallvcm_amd/csrc/vcm_display.h -- the exposure from the histogram, the parameter check, the bin of a luminance, the
// dither and the bytes -- on ordinary and on hostile inputs.  Prints "ok" and returns 0; a wrong answer returns 1, a
// sanitizer report aborts.
//
//   sanitize_display <directory to write a BMP into>
#include <limits>
#include <string>
#include <vector>

#include "../../smallvcm_amd/host/vcm_render_display.hpp"
#include "../../smallvcm_amd/csrc/vcm_display.h"

using namespace vcm;

static int g_failed;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "sanitize_display: line %d: %s\n", __LINE__, #cond); g_failed = 1; } } while (0)

// parse a command line of display flags; -1: refused, else the number of flags taken
static int parse(std::vector<std::string> words, DisplayFlags &d)
{
    std::vector<char *> argv;
    words.insert(words.begin(), "vcm_render");
    for (auto &w : words) argv.push_back(&w[0]);
    d = DisplayFlags();
    disp_defaults(&d.p);
    int taken = 0;
    for (int i = 1; i < (int)argv.size(); i++) {
        const int t = display_parse_flag((int)argv.size(), argv.data(), i, d);
        if (t < 0) return -1;
        taken += t;
    }
    return taken;
}

static void flags()
{
    DisplayFlags d;
    EXPECT(parse({}, d) == 0 && !d.any);
    EXPECT(parse({ "-o", "x.bmp", "--json" }, d) == 0 && !d.any);
    EXPECT(parse({ "--tonemap", "aces", "--exposure", "-1.5", "--auto-exposure", "--bloom", "0.25", "--srgb", "--dither" }, d) == 6 && d.any);
    EXPECT(d.p.curve == VCM_CURVE_ACES && d.p.exposureEV == -1.5f && d.p.autoExposure == 1 && d.p.key == 0.18f && d.p.bloomStrength == 0.25f);
    EXPECT(d.p.bloomLevels == 5 && d.p.transfer == VCM_TRANSFER_SRGB && d.p.dither == 1 && disp_check_params(&d.p) == NULL);
    EXPECT(parse({ "--auto-exposure", "0.25", "--bloom", "1", "8", "--tonemap", "hable" }, d) == 3 && d.p.key == 0.25f && d.p.bloomLevels == 8 && d.p.curve == VCM_CURVE_HABLE);
    EXPECT(parse({ "--auto-exposure", "-o", "x.bmp" }, d) == 1 && d.p.key == 0.18f);   // the key is optional: the next option stays
    EXPECT(parse({ "--bloom", ".5", "-i", "4" }, d) == 1 && d.p.bloomStrength == 0.5f && d.p.bloomLevels == 5);
    EXPECT(parse({ "--tonemap", "reinhard" }, d) == 1 && d.p.curve == VCM_CURVE_REINHARD);
    EXPECT(parse({ "--tonemap", "clamp" }, d) == 1 && d.any && d.p.curve == VCM_CURVE_CLAMP);
    const std::string longWord(100000, '9');
    const std::vector<std::vector<std::string>> bad = {
        { "--tonemap" }, { "--tonemap", "filmic" }, { "--tonemap", "" }, { "--exposure" }, { "--exposure", "bright" }, { "--exposure", "1e" },
        { "--exposure", "nan" }, { "--exposure", "inf" }, { "--exposure", "40" }, { "--exposure", "1.5x" }, { "--exposure", longWord },
        { "--auto-exposure", "0" }, { "--auto-exposure", "0.18abc" }, { "--auto-exposure", "1e99" },
        { "--bloom" }, { "--bloom", "-0.1" }, { "--bloom", "1.5" }, { "--bloom", "x" }, { "--bloom", "0.5", "0" }, { "--bloom", "0.5", "9" },
        { "--bloom", "0.5", "3.5" }, { "--bloom", "0.5", longWord }, { "--bloom", longWord },
    };
    for (const auto &b : bad) {
        if (parse(b, d) != -1) { fprintf(stderr, "sanitize_display: accepted:"); for (const auto &w : b) fprintf(stderr, " %.20s", w.c_str()); fprintf(stderr, "\n"); g_failed = 1; }
    }
}

static void bmp(const std::string &dir)
{
    const int W = 5, H = 3;   // a row of 15 bytes: the reference pads nothing, and neither does this
    std::vector<unsigned char> px((size_t)W * H * 3);
    for (size_t i = 0; i < px.size(); i++) px[i] = (unsigned char)(i * 7 + 1);
    const std::string path = dir + "/sanitize_display.bmp";
    EXPECT(display_write_bmp(path.c_str(), W, H, px.data()) == 0);
    FILE *f = fopen(path.c_str(), "rb");
    EXPECT(f != NULL);
    if (f) {
        std::vector<unsigned char> file(54 + px.size() + 8);
        const size_t got = fread(file.data(), 1, file.size(), f);
        fclose(f);
        EXPECT(got == 54 + px.size() && file[0] == 'B' && file[1] == 'M');
        uint32_t h[13];
        memcpy(h, &file[2], sizeof(h));
        EXPECT(h[0] == 54 + px.size() && h[2] == 54 && h[3] == 40 && h[4] == (uint32_t)W && h[5] == (uint32_t)H && h[6] == (1u | (24u << 16)) && h[8] == px.size());
        EXPECT(memcmp(&file[54], px.data(), px.size()) == 0);
        remove(path.c_str());
    }
    EXPECT(display_write_bmp((dir + "/no/such/directory/x.bmp").c_str(), W, H, px.data()) == -1);
    EXPECT(display_write_bmp(path.c_str(), 0, H, px.data()) == -1 && display_write_bmp(path.c_str(), W, -1, px.data()) == -1);
    EXPECT(display_write_bmp(path.c_str(), 65536, 65536, px.data()) == -1 && display_write_bmp(NULL, W, H, px.data()) == -1 && display_write_bmp(path.c_str(), W, H, NULL) == -1);
    vcm_display_stats s = {};
    s.autoEV = -std::numeric_limits<double>::max(); s.multiplier = std::numeric_limits<double>::max(); s.logAvgLuminance = std::numeric_limits<double>::quiet_NaN();
    s.counted = s.zero = s.nonFinite = s.clampedLow = s.clampedHigh = s.clipped = std::numeric_limits<long long>::min();
    char json[480];
    display_stats_json(s, json, sizeof(json));
    EXPECT(strlen(json) < sizeof(json) - 1 && json[strlen(json) - 1] == '}');
    char tiny[16];
    display_stats_json(s, tiny, sizeof(tiny));
    EXPECT(strlen(tiny) == sizeof(tiny) - 1);
}

static void exposure()
{
    vcm_display_params p;
    disp_defaults(&p);
    p.autoExposure = 1;
    EXPECT(disp_check_params(&p) == NULL && disp_check_params(NULL) != NULL);
    vcm_display_stats st;
    std::vector<unsigned long long> c(VCM_DISP_COUNTERS, 0ull);
    disp_auto_exposure(c.data(), p, &st);
    EXPECT(st.autoEV == 0.0 && st.multiplier == 1.0 && st.counted == 0);
    c[8 * 20] = 1000;   // everything in [1, 1.125)
    disp_auto_exposure(c.data(), p, &st);
    EXPECT(st.counted == 1000 && fabs(st.logAvgLuminance - 0.5 * log2(1.125)) < 1e-12 && fabs(st.autoEV - (log2(0.18) - 0.5 * log2(1.125))) < 1e-6);
    for (int b = 0; b < VCM_DISP_BINS; b++) c[b] = 0x7fffffffull;   // every bin as full as an image can make it
    c[VCM_DISP_ZERO] = c[VCM_DISP_NONFINITE] = 0x7fffffffull;
    disp_auto_exposure(c.data(), p, &st);
    EXPECT(st.counted == 256ll * 0x7fffffffll && st.autoEV > -16.0 && st.autoEV < 16.0);
    for (int b = 0; b < VCM_DISP_COUNTERS; b++) c[b] = ~0ull;         // counters no image can produce: no overflow in the conversions
    disp_auto_exposure(c.data(), p, &st);
    EXPECT(st.counted > 0 && st.autoEV == st.autoEV);
    p.lowPercentile = 0.f; p.highPercentile = 1.f; p.minEV = -32.f; p.maxEV = 32.f; p.exposureEV = 32.f;
    std::fill(c.begin(), c.end(), 0ull);
    c[0] = 1;
    disp_auto_exposure(c.data(), p, &st);
    EXPECT(st.autoEV > 17.0 && st.multiplier > 1e14 && st.multiplier < 3.5e38);   // 2^(17.4 + 32) fits fp32
    c[0] = 0; c[255] = 1; p.exposureEV = -32.f;
    disp_auto_exposure(c.data(), p, &st);
    EXPECT(st.autoEV < -14.0 && st.multiplier > 0.0);
    const float specials[] = { 0.f, -0.f, 1e-45f, 1e-38f, 9.5e-7f, 1.f, 4095.9f, 4096.f, 3.4e38f, -1.f, std::numeric_limits<float>::infinity(),
                               -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN() };
    for (float y : specials) {
        int second;
        const int slot = disp_counter(y, second);
        EXPECT(slot >= 0 && slot <= VCM_DISP_NONFINITE && (second == -1 || second == VCM_DISP_CLAMPED_LOW || second == VCM_DISP_CLAMPED_HIGH));
        const unsigned char b = disp_byte(y, 1, 0x7fffffffll, 2, 0xffffffffu);
        EXPECT(b == 0 || b == 255 || y == 1e-45f || y == 1e-38f || y == 9.5e-7f);
        int clipped;
        const F4 v = disp_finish(mk3(y, y, y), VCM_CURVE_HABLE, 4.f, VCM_TRANSFER_SRGB, 1.f / 2.2f, clipped);
        EXPECT(v.x >= 0.f && v.x <= 1.f && v.w == 1.f);
    }
    EXPECT(disp_dither(0x7fffffffll, 2, 0xffffffffu) < 1.f && disp_dither(0, 0, 0) >= 0.f);
    EXPECT(disp_bloom_scratch_f4(1, 1, 8) == 10 && disp_bloom_scratch_f4(46340, 46340, 8) > 0);
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: sanitize_display <directory>\n"); return 2; }
    flags();
    bmp(argv[1]);
    exposure();
    if (!g_failed) printf("ok\n");
    return g_failed;
}
