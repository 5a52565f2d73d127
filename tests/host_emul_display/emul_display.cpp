// TEST INFRASTRUCTURE.  The host emulation of the display transform: the functions of smallvcm_amd/csrc/vcm_display.h that
// the kernels of vcm_display.hip run, compiled for the host and driven serially over whole images -- the lanes of a grid
// and the levels of the pyramid in loops -- for tests/test_display.py and tests/test_gpu_display.py.  Never built into
// libsmallvcm_amd.so.
#include <string.h>
#include <string>
#include <vector>
#include "../../smallvcm_amd/csrc/vcm_display.h"

using namespace vcm;

static thread_local std::string g_err;
static int refuse(const char *why) { g_err = why; return -1; }

/* k_disp_histogram: the counters of the n pixels of src * scale.  The counts are integers: the order in which the grid's
   lanes, waves and workgroups add does not show, so the loop runs over the pixels. */
static void histogram(long long n, const float *src, int channels, float scale, unsigned long long *counters)
{
    memset(counters, 0, VCM_DISP_COUNTERS * sizeof(unsigned long long));
    for (long long p = 0; p < n; p++) {
        int second;
        const int slot = disp_counter(disp_luminance(disp_load(src, channels, p, scale)), second);
        counters[slot]++;
        if (second >= 0) counters[second]++;
    }
}

/* disp_launch_transform's bloom: U_1 (w1 x h1) of the image */
static std::vector<F4> bloom_u1(int W, int H, const float *src, int channels, float scale, float mult, int L, int &w1, int &h1)
{
    std::vector<int> w((size_t)L + 1), h((size_t)L + 1);
    std::vector<std::vector<F4>> g((size_t)L + 1);
    w[0] = W; h[0] = H;
    for (int l = 1; l <= L; l++) {
        w[l] = disp_level_dim(w[l - 1]); h[l] = disp_level_dim(h[l - 1]);
        const size_t n = (size_t)w[l] * h[l];
        std::vector<F4> d(n), t(n);
        g[l].resize(n);
        for (int y = 0; y < h[l]; y++)
            for (int x = 0; x < w[l]; x++)
                d[(size_t)y * w[l] + x] = (l == 1)
                    ? disp_down(x, y, w[0], h[0], [&](int xs, int ys) { return disp_bloom_input(disp_load(src, channels, (long long)ys * W + xs, scale), mult); })
                    : disp_down(x, y, w[l - 1], h[l - 1], [&](int xs, int ys) { return g[l - 1][(size_t)ys * w[l - 1] + xs]; });
        for (int y = 0; y < h[l]; y++)
            for (int x = 0; x < w[l]; x++) t[(size_t)y * w[l] + x] = disp_blur5(x, w[l], [&](int j) { return d[(size_t)y * w[l] + j]; });
        for (int y = 0; y < h[l]; y++)
            for (int x = 0; x < w[l]; x++) g[l][(size_t)y * w[l] + x] = disp_blur5(y, h[l], [&](int j) { return t[(size_t)j * w[l] + x]; });
    }
    for (int l = L - 1; l >= 1; l--)
        for (int y = 0; y < h[l]; y++)
            for (int x = 0; x < w[l]; x++) {
                F4 &v = g[l][(size_t)y * w[l] + x];
                v = disp_add4(v, disp_up(x, y, w[l + 1], h[l + 1], [&](int xs, int ys) { return g[l + 1][(size_t)ys * w[l + 1] + xs]; }));
            }
    w1 = w[1]; h1 = h[1];
    return g[1];
}

/* steps 1 and 2 of pixel p = (x, y): the linear pixel the curve takes */
static V3 linear_pixel(int x, int y, int W, const float *src, int channels, float scale, float mult, const vcm_display_params &p,
                       const std::vector<F4> &u1, int w1, int h1)
{
    const V3 c = disp_load(src, channels, (long long)y * W + x, scale);
    if (!(p.bloomStrength > 0.f)) return mk3(c.x * mult, c.y * mult, c.z * mult);
    const F4 up1 = disp_up(x, y, w1, h1, [&](int xs, int ys) { return u1[(size_t)ys * w1 + xs]; });
    return disp_bloom_combine(c, mult, up1, 1.f / (float)p.bloomLevels, p.bloomStrength);
}

extern "C" {

const char *emul_display_error() { return g_err.c_str(); }

void emul_display_defaults(vcm_display_params *out) { disp_defaults(out); }

int emul_display_check(const vcm_display_params *p)
{
    if (const char *why = disp_check_params(p)) return refuse(why);
    return 0;
}

/* the 264 counters of src * scale */
void emul_display_histogram(long long n, const float *src, int channels, float scale, unsigned long long *counters264)
{
    histogram(n, src, channels, scale, counters264);
}

/* disp_auto_exposure on given counters */
void emul_display_exposure(const unsigned long long *counters264, const vcm_display_params *p, vcm_display_stats *out)
{
    disp_auto_exposure(counters264, *p, out);
}

/* vcm_display_buffers: out = W * H float4; histogram256 (may be NULL) = the bins where autoExposure is on; -1 (and
   emul_display_error) where the library refuses */
int emul_display(int W, int H, const float *src, int channels, float scale, const vcm_display_params *p, float *out, vcm_display_stats *stats,
                 unsigned long long *histogram256)
{
    if (!src || !out) return refuse("NULL image");
    if (W <= 0 || H <= 0 || (long long)W * H > 0x7fffffffll) return refuse("bad size");
    if (channels != 3 && channels != 4) return refuse("channels must be 3 or 4");
    if (out == src) return refuse("outDev is the input");
    if (const char *why = disp_check_params(p)) return refuse(why);
    if (!disp_finite(scale)) return refuse("scale is not finite");
    unsigned long long counters[VCM_DISP_COUNTERS];
    memset(counters, 0, sizeof(counters));
    if (p->autoExposure) histogram((long long)W * H, src, channels, scale, counters);
    if (histogram256) memcpy(histogram256, counters, VCM_DISP_BINS * sizeof(unsigned long long));
    vcm_display_stats st;
    disp_auto_exposure(counters, *p, &st);
    const float mult = (float)st.multiplier;
    std::vector<F4> u1;
    int w1 = 0, h1 = 0;
    if (p->bloomStrength > 0.f) u1 = bloom_u1(W, H, src, channels, scale, mult, p->bloomLevels, w1, h1);
    long long clipped = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            int cl;
            ((F4 *)out)[(size_t)y * W + x] = disp_finish(linear_pixel(x, y, W, src, channels, scale, mult, *p, u1, w1, h1), p->curve, p->whitePoint,
                                                         p->transfer, 1.f / p->gamma, cl);
            clipped += cl;
        }
    st.clipped = clipped;
    if (stats) *stats = st;
    return 0;
}

/* steps 1 and 2 alone: out = W * H * 3 floats, the linear image the curve would take (multiplier mult) */
int emul_display_bloom(int W, int H, const float *src, int channels, float mult, float strength, int levels, float *out3)
{
    vcm_display_params p;
    disp_defaults(&p);
    p.bloomStrength = strength; p.bloomLevels = levels;
    if (const char *why = disp_check_params(&p)) return refuse(why);
    std::vector<F4> u1;
    int w1 = 0, h1 = 0;
    if (strength > 0.f) u1 = bloom_u1(W, H, src, channels, 1.f, mult, levels, w1, h1);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const V3 v = linear_pixel(x, y, W, src, channels, 1.f, mult, p, u1, w1, h1);
            float *o = out3 + ((size_t)y * W + x) * 3;
            o[0] = v.x; o[1] = v.y; o[2] = v.z;
        }
    return 0;
}

/* steps 3 and 4 of n linear pixels (3 floats each) -> n * 3 floats */
void emul_display_curve(long long n, const float *lin3, int curve, float whitePoint, int transfer, float gamma, int applyTransfer, float *out3)
{
    for (long long i = 0; i < n; i++) {
        int cl;
        V3 c = disp_curve(mk3(lin3[i * 3], lin3[i * 3 + 1], lin3[i * 3 + 2]), curve, whitePoint, cl);
        if (applyTransfer) c = mk3(disp_transfer(c.x, transfer, 1.f / gamma), disp_transfer(c.y, transfer, 1.f / gamma), disp_transfer(c.z, transfer, 1.f / gamma));
        out3[i * 3] = c.x; out3[i * 3 + 1] = c.y; out3[i * 3 + 2] = c.z;
    }
}

/* step 4 of n channels in [0, 1] */
void emul_display_transfer(long long n, const float *c, int transfer, float gamma, float *out)
{
    for (long long i = 0; i < n; i++) out[i] = disp_transfer(c[i], transfer, 1.f / gamma);
}

/* vcm_read_display_image: the bytes of a W * H float4 display image */
int emul_display_encode(int W, int H, const float *img4, int format, int dither, unsigned seed, unsigned char *out)
{
    if (format == VCM_IMAGE_RGBE) return refuse("RGBE is a linear format: vcm_read_image writes it");
    if (format != VCM_IMAGE_BGR8 && format != VCM_IMAGE_RGBA8) return refuse("unknown format");
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) disp_encode_pixel(((const F4 *)img4)[(size_t)y * W + x], x, y, W, H, format, dither, seed, out);
    return 0;
}

} // extern "C"
