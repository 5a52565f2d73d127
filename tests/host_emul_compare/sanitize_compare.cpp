// TEST INFRASTRUCTURE.  A stand-alone program (its own main) that runs the host emulation of the comparison -- every
// function of vcm_compare.h, over the shapes at which the indexing changes: no window, one, a partial tile on both axes,
// more lanes than pixels, a capped grid -- under AddressSanitizer and UndefinedBehaviorSanitizer (make sanitize_compare).
// tests/test_compare.py builds and runs it; it prints "ok" and exits 0.
#include <stdio.h>
#include "emul_compare.cpp"

static unsigned lcg(unsigned &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

int main()
{
    const int shapes[][2] = { { 1, 1 }, { 3, 2 }, { 10, 64 }, { 11, 11 }, { 12, 11 }, { 33, 9 }, { 67, 45 }, { 75, 27 } };
    unsigned seed = 7u;
    for (const auto &sh : shapes)
        for (int imgCh = 3; imgCh <= 4; imgCh++)
            for (int refCh = 3; refCh <= 4; refCh++)
                for (int cap = 0; cap <= 2; cap += 2) {
                    const int W = sh[0], H = sh[1];
                    const size_t n = (size_t)W * H;
                    std::vector<float> img(n * imgCh), ref(n * refCh);
                    std::vector<F4> map(n);
                    for (float &v : img) v = (float)lcg(seed) / 16777216.f;
                    for (float &v : ref) v = (float)lcg(seed) / 16777216.f;
                    if (n > 5) { img[4] = u2f(0x7fc00000u); ref[(n - 1) * refCh] = u2f(0x7f800000u); }
                    vcm_compare_params p;
                    emul_compare_defaults(&p);
                    p.writeMap = 1; p.threshold = 0.5f;
                    vcm_compare_stats st;
                    if (emul_compare(W, H, img.data(), imgCh, 0.5f, ref.data(), refCh, &p, cap, (float *)map.data(), &st)) { fprintf(stderr, "%s\n", emul_compare_error()); return 1; }
                    if (st.pixels != (long long)n || st.nonFinite != (n > 5 ? 2 : 0)) { fprintf(stderr, "%d x %d: counts\n", W, H); return 1; }
                    const long long want = (W < 11 || H < 11) ? 0 : (long long)(W - 10) * (H - 10);
                    if (st.ssimWindows > want || (st.ssimWindows == 0) != (st.ssim != st.ssim)) { fprintf(stderr, "%d x %d: windows\n", W, H); return 1; }
                }
    if (emul_compare(3, 2, NULL, 3, 1.f, NULL, 3, NULL, 0, NULL, NULL) != -1) return 1;
    printf("ok\n");
    return 0;
}
