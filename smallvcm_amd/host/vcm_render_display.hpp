// vcm_render_display.hpp -- the display-transform flags of vcm_render and the BMP file they write.  A header of its own, free
// of any device call, so that a stand-alone program can run the parsing and the file writing under the host sanitizers
// (tests/host_emul_display/sanitize_display.cpp).
//
//   --tonemap clamp|reinhard|aces|hable   the tone curve (vcm_display_params.curve)
//   --exposure EV                         manual exposure compensation in stops
//   --auto-exposure [key]                 exposure from the log-luminance histogram; key: the luminance the trimmed mean goes to
//   --bloom S [levels]                    bloom of strength S in [0, 1] over `levels` (1 .. 8) pyramid levels
//   --srgb                                the sRGB transfer curve instead of gamma 2.2
//   --dither                              stochastic rounding to 8 bits instead of truncation
#ifndef SMALLVCM_AMD_VCM_RENDER_DISPLAY_HPP
#define SMALLVCM_AMD_VCM_RENDER_DISPLAY_HPP

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "smallvcm_amd.h"

struct DisplayFlags {
    bool any;                  // one of the flags was given: .bmp output goes through vcm_display
    vcm_display_params p;      // the caller fills the defaults (vcm_display_defaults) before parsing
};

// a whole number / a finite float, nothing behind it
static inline bool display_parse_float(const char *s, float *out)
{
    if (!s || !*s) return false;
    char *e = NULL;
    const float v = strtof(s, &e);
    if (e == s || *e || !(v - v == 0.f)) return false;
    *out = v;
    return true;
}
static inline bool display_parse_int(const char *s, int *out)
{
    if (!s || !*s) return false;
    char *e = NULL;
    const long v = strtol(s, &e, 10);
    if (e == s || *e || v < -1000000 || v > 1000000) return false;
    *out = (int)v;
    return true;
}
static inline bool display_starts_a_number(const char *s)
{
    return s && ((s[0] >= '0' && s[0] <= '9') || (s[0] == '.' && s[1] >= '0' && s[1] <= '9'));
}

// argv[i] as a display flag: 1 = taken (i stands on its last argument), 0 = not one of them, -1 = refused (said on stderr)
static inline int display_parse_flag(int argc, char **argv, int &i, DisplayFlags &d)
{
    const char *a = argv[i];
    if (!strcmp(a, "--tonemap")) {
        if (i + 1 >= argc) { fprintf(stderr, "vcm_render: --tonemap clamp|reinhard|aces|hable\n"); return -1; }
        const char *v = argv[++i];
        if (!strcmp(v, "clamp")) d.p.curve = VCM_CURVE_CLAMP;
        else if (!strcmp(v, "reinhard")) d.p.curve = VCM_CURVE_REINHARD;
        else if (!strcmp(v, "aces")) d.p.curve = VCM_CURVE_ACES;
        else if (!strcmp(v, "hable")) d.p.curve = VCM_CURVE_HABLE;
        else { fprintf(stderr, "vcm_render: --tonemap clamp|reinhard|aces|hable\n"); return -1; }
    } else if (!strcmp(a, "--exposure")) {
        if (i + 1 >= argc || !display_parse_float(argv[i + 1], &d.p.exposureEV) || d.p.exposureEV < -32.f || d.p.exposureEV > 32.f) {
            fprintf(stderr, "vcm_render: --exposure needs a number of stops in [-32, 32]\n");
            return -1;
        }
        i++;
    } else if (!strcmp(a, "--auto-exposure")) {
        d.p.autoExposure = 1;
        if (i + 1 < argc && display_starts_a_number(argv[i + 1])) {
            if (!display_parse_float(argv[i + 1], &d.p.key) || !(d.p.key > 0.f)) { fprintf(stderr, "vcm_render: --auto-exposure [key] needs a positive key\n"); return -1; }
            i++;
        }
    } else if (!strcmp(a, "--bloom")) {
        if (i + 1 >= argc || !display_parse_float(argv[i + 1], &d.p.bloomStrength) || d.p.bloomStrength < 0.f || d.p.bloomStrength > 1.f) {
            fprintf(stderr, "vcm_render: --bloom S [levels] needs a strength in [0, 1]\n");
            return -1;
        }
        i++;
        if (i + 1 < argc && display_starts_a_number(argv[i + 1])) {
            if (!display_parse_int(argv[i + 1], &d.p.bloomLevels) || d.p.bloomLevels < 1 || d.p.bloomLevels > 8) { fprintf(stderr, "vcm_render: --bloom S [levels] takes 1 .. 8 levels\n"); return -1; }
            i++;
        }
    } else if (!strcmp(a, "--srgb")) d.p.transfer = VCM_TRANSFER_SRGB;
    else if (!strcmp(a, "--dither")) d.p.dither = 1;
    else return 0;
    d.any = true;
    return 1;
}

// Framebuffer::SaveBMP's file (BmpHeader, framebuffer.hxx:150-168, :175-191) around pixel data in vcm_read_image's BGR8
// layout: 0, or -1 where the file cannot be written
static inline int display_write_bmp(const char *path, int resX, int resY, const unsigned char *bgr)
{
    if (!path || !bgr || resX < 1 || resY < 1 || (uint64_t)resX * (uint64_t)resY * 3u > 0xffffff00ull) return -1;
    FILE *f = fopen(path, "wb");
    if (!f) return -1;
    const uint32_t bytes = (uint32_t)resX * (uint32_t)resY * 3u;
    const uint32_t h[13] = { 54u + bytes, 0u, 54u, 40u, (uint32_t)resX, (uint32_t)resY, 1u | (24u << 16), 0u, bytes, 2953u, 2953u, 0u, 0u };
    bool ok = fwrite("BM", 1, 2, f) == 2 && fwrite(h, 4, 13, f) == 13 && fwrite(bgr, 1, bytes, f) == bytes;
    ok = (fclose(f) == 0) && ok;
    return ok ? 0 : -1;
}

// the "display" member of the --json line (with its leading comma) into buf
static inline void display_stats_json(const vcm_display_stats &s, char *buf, size_t size)
{
    snprintf(buf, size, ", \"display\": {\"autoEV\": %.17g, \"multiplier\": %.17g, \"logAvgLuminance\": %.17g, \"counted\": %lld, \"zero\": %lld, "
             "\"nonFinite\": %lld, \"clampedLow\": %lld, \"clampedHigh\": %lld, \"clipped\": %lld}", s.autoEV, s.multiplier, s.logAvgLuminance,
             s.counted, s.zero, s.nonFinite, s.clampedLow, s.clampedHigh, s.clipped);
}

#endif
