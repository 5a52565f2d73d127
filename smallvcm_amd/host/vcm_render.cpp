// vcm_render.cpp -- a C++ host over the C-ABI alone (include/smallvcm_amd.h; no
// reference headers, no Python): the driver options the reference's CLI does not
// expose.  smallvcm.cxx hard-wires 512x512, seed 1234,
// path lengths 0..10, one renderer per host core and CPU-seconds timing
// (src/config.hxx:233-240, src/smallvcm.cxx:66, :150); the benchmark and parity
// configurations need other resolutions, a fixed renderer count, raw fp32
// output and wall-clock time.
//
//   vcm_render -s <scene 0..3> -a <el|pt|lt|ppm|bpm|bpt|vcm> -i <iterations>
//              [--res W H] [--seed S] [--minlen A] [--maxlen B]
//              [--renderers R] [--radius-factor F] [--radius-alpha A]
//              [--device D] [--strict] [--warmup W] [-o out.pfm] [--json] [--scene-file f.vcmscene|f.obj]
//              [--envmap f.hdr|f.pfm [--envmap-scale S]] [--aperture R --focus D]
//              [--light-pick uniform|power [--light-pick-mix A] [--light-pick-report]]
//              [--filter tent|bspline R]
//              [--projection fisheye DEG|panorama]
//              [--denoise [passes]] [--denoise-sigma c,n,z] [--no-demodulate] [--features-out prefix]
//              [--noise-target E [--check-every N] [--max-iterations M]] [--track-variance] [--robust [M]]
//              [--reference FILE [--compare-every N] [--compare-log FILE.csv] [--error-target relMSE [--max-iterations M]] [--error-map FILE.pfm]]
//              [--tonemap clamp|reinhard|aces|hable] [--exposure EV] [--auto-exposure [key]] [--bloom S [levels]]
//              [--srgb] [--dither]
//              [--parts prefix]
//              [--gpus N [--shards S] [--inflight K] [--devices 0,1,..] [--collectives rccl|threads] [--same-window]]
//
// --gpus N: the multi-GPU host (vcm_farm.hpp): N ranks = N host threads, one per GPU, cut into N / S groups; a
// renderer lives on a group (S path-index shards, RCCL all-gather of the light vertices every iteration), K
// renderers take turns on a group, one RCCL all-reduce of the framebuffers at read-out.  --shards 1 = one renderer per
// GPU (the reference's own iteration-parallel scheme).  --collectives threads replaces RCCL by an in-process
// stand-in so that several ranks can share one GPU (tests; RCCL refuses two ranks on one device).
//
// --envmap: the built-in scene's BackgroundLight (scene 3) replaced by an environment map (vcm_envmap_load,
// radiance = texel * S, S = 1 by default) over the same geometry; a scene file names its map itself (`light envmap`).
//
// --aperture R --focus D: a thin lens of radius R focused at distance D along the camera's forward axis (world units;
// vcm_scene_desc4), for a built-in scene or a scene file; they override a scene file's `lens` directive.
//
// --light-pick uniform|power: how a light is chosen where a path samples one (vcm_light_pick, vcm_scene_desc5): with
// equal probability (the default) or by emitted power, --light-pick-mix A in [0, 1] of the uniform choice mixed in; they
// override a scene file's `lightpick` directive.  The mode in effect is printed when it is not the default, and with
// --light-pick-report the five most probable lights and their probabilities.
//
// --filter tent|bspline R: the pixel reconstruction filter (vcm_pixel_filter, vcm_scene_desc6) in place of the reference's
// box: filter importance sampling with an offset density of support R pixels (finite, 0 < R <= 16) on the camera side
// and on the light splats; it overrides a scene file's `filter` directive, and with --gpus every renderer of the farm
// takes it.  The guide images of --features-out stay unfiltered.
//
// --sampler sobol|philox: where the paths' random floats come from (vcm_sampler, vcm_scene_desc7): the Owen-scrambled
// Sobol sequence or the default white noise; it overrides a scene file's `sampler` directive, and with --gpus every
// renderer of the farm takes it.
//
// --projection fisheye DEG|panorama: the camera's projection (vcm_camera_model, vcm_scene_desc9) in place of the pinhole:
// an equidistant fisheye of DEG degrees (finite, in (0, 360)) across the image width, or a 360 x 180 degree
// equirectangular panorama (written as .pfm or .hdr it loads back as an environment map; DESIGN.md "Camera projections"
// has the recipe); it overrides a scene file's `projection` directive.  Not with --gpus, and not with a lens.
//
// --denoise [passes]: the image goes through the edge-avoiding a-trous filter (vcm_denoise: vcm_denoise_defaults with
// `passes`, --denoise-sigma's sigmaColor,sigmaNormal,sigmaDepth and --no-demodulate applied) before it is written to
// -o; the unfiltered image is written beside it as <name>.noisy.<ext>.  --features-out P writes the first-hit guide
// images P.albedo.pfm, P.normal.pfm ("PF") and P.depth.pfm ("Pf", one channel).  Both want one renderer on one GPU.
//
// --noise-target E: render to a noise level instead of an iteration count.  The per-pixel variance is tracked
// (vcm_track_variance) and the mean of the noise statistic (vcm_get_noise_stats: the expected relative squared error
// V / (mean^2 + 0.01)) is looked at after every N iterations (--check-every, default 4) and after the last one, never
// before the second; rendering stops at the first look at or below E or after M iterations (--max-iterations, default
// 1024; -i is not used).  Every look and the iterations used are printed.  --track-variance alone tracks the variance
// over the -i iterations and prints the statistic at the end.  Both want one renderer on one GPU.
//
// --robust [M]: the image written to -o (and summed into image_mean) is the firefly-robust estimate instead of the mean:
// the iterations go round-robin into M buckets (vcm_track_robust; odd, 3 .. 15, default VCM_ROBUST_DEFAULT_BUCKETS) and
// every pixel averages the central bucket means, trimmed by their Gini coefficient (vcm_read_robust).  Wants -i >= M and
// one renderer on one GPU.  What the rule decided (vcm_get_robust_stats) is printed, and is "robust" in --json.  With
// --denoise it is refused: filtering the robust image is a host's own vcm_robust_device + vcm_denoise_buffers for now.
//
// --parts P: the technique breakdown (vcm_track_parts): which part of the estimator carries a pixel.  Writes
// P_emission.pfm, P_direct.pfm, P_connect.pfm, P_merge.pfm and P_lighttrace.pfm -- each plane divided by the iteration
// count, so that the five add up to the image -- prints each part's share of the total luminance (vcm_get_parts_stats) and
// adds "parts" to --json.  Wants one renderer on one GPU, a VertexCM algorithm (lt, ppm, bpm, bpt, vcm), no --strict and
// --maxlen <= 31; anything else is refused with exit status 2 before any device call.
//
// --tonemap / --exposure / --auto-exposure / --bloom / --srgb / --dither (vcm_render_display.hpp): with any of them a .bmp
// goes through the display transform on the device (vcm_display, then vcm_read_display_image) instead of the reference's
// clamp-and-gamma encoding: the denoised image with --denoise (the .noisy.bmp beside it: the framebuffer, the same way),
// the robust image with --robust, else the framebuffer / iterations.  What the transform saw (vcm_get_display_stats: the
// exposure picked, the channels clipped) is printed, and is "display" in --json; .hdr and .pfm stay linear, and without
// these flags every file is what it was.  They want one renderer on one GPU.
//
// --reference FILE [--compare-every N] [--compare-log FILE.csv] [--error-target relMSE [--max-iterations M]]
// [--error-map FILE.pfm]: the image is compared with a reference image on the device (vcm_set_reference, vcm_compare).  FILE is
// a .pfm or .hdr of the frame's resolution (vcm_envmap_load reads it; a .pfm is taken with its rows top to bottom, as -o and
// the reference's SavePFM write them, not bottom-up as the format has them; another resolution is refused).  Every
// N iterations (--compare-every) and after the last, a line "compare after K iteration(s): relMSE .. MSE .. PSNR .. SSIM ..
// maxAbs .. nonFinite .." is printed, and written to --compare-log as a CSV row (iteration, relMSE, MSE, PSNR, SSIM, maxAbs,
// nonFinite, under a header row).  With --error-target rendering runs iterations 0, 1, ... and stops at the first check at
// or below the target, or at --max-iterations (default 1024; without --compare-every every 4 iterations are checked).  The
// compared image is the one written to -o: the denoised image with --denoise (filtered for every check), the robust estimate
// with --robust (checked once it has as many iterations as buckets; fewer iterations than buckets in all are refused), else
// framebuffer / iterations.  With --noise-target the run stops by the noise statistic as before and the error is looked at
// every --compare-every iterations (default: --check-every) and at the iteration the run stops, so that the last line is
// the true error of the image written.  --error-map writes the
// last check's relative squared error of r, g, b as a PFM.  The last check is "compare" in --json.  One renderer on one GPU;
// without --reference every file is what it was.
//
// -s / -a / -i keep the meaning they have in the reference's CLI
// (src/config.hxx:246-395; scenes = g_SceneConfigs[0..3], :146-151).
// --renderers R reproduces render() (src/smallvcm.cxx:52-151) with R "threads":
// renderer g has seed S+g and runs the iterations OpenMP's static schedule gives
// thread g; the image is the mean of the used renderers' means.  -o picks the
// format by extension like the reference (src/smallvcm.cxx:300-309): .bmp
// (gamma 2.2, Framebuffer::SaveBMP src/framebuffer.hxx:170-214), .hdr (SaveHDR
// :219-251), anything else raw fp32 PFM (SavePFM :137-146: "PF", "W H", "-1",
// rows top to bottom).  With one renderer the 8-bit formats are encoded on the
// device (vcm_read_image); with several, from the averaged framebuffer here.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "smallvcm_amd.h"
#include "smallvcm_amd_debug.h"
#include "vcm_farm.hpp"
#include "vcm_render_display.hpp"

static int die(const char *what)
{
    fprintf(stderr, "vcm_render: %s: %s\n", what, vcm_last_error());
    return 2;   // the reference's convention for fatal errors (src/config.hxx:140-141)
}

static int algorithm_by_acronym(const std::string &a)
{   // Config::GetAcronym, src/config.hxx:86-91
    if (a == "el") return VCM_ALGO_EYE_LIGHT;
    if (a == "pt") return VCM_ALGO_PATH_TRACE;
    if (a == "lt") return VCM_ALGO_LIGHT_TRACE;
    if (a == "ppm") return VCM_ALGO_PPM;
    if (a == "bpm") return VCM_ALGO_BPM;
    if (a == "bpt") return VCM_ALGO_BPT;
    if (a == "vcm") return VCM_ALGO_VCM;
    return -1;
}

int main(int argc, char **argv)
{
    int sceneID = 0, algorithm = VCM_ALGO_VCM, iterations = 1, resX = 512, resY = 512, seed = 1234;   // config.hxx:233-240
    unsigned minLen = 0, maxLen = 10;
    int renderers = 1, device = 0, warmup = 0, strict = 0, json = 0;
    int gpus = 0, shards = 0, inflight = 0, rccl = 1, sameWindow = 0, rcclRanks = 0;
    std::vector<float> rankMs;
    std::vector<int> devices;
    float radiusFactor = 0.003f, radiusAlpha = 0.75f;
    std::string out, algoName = "vcm", sceneFile, envFile;
    float envScale = 1.f;
    float aperture = 0.f, focus = 0.f;
    bool haveAperture = false, haveFocus = false;
    std::string pickName;
    float pickMix = 0.f;
    bool havePickMix = false, pickReport = false;
    std::string filterName;
    std::string samplerName;
    std::string projName;
    float projFov = 0.f;
    float filterRadius = 0.f;
    bool denoise = false;
    vcm_denoise_params dn;
    vcm_denoise_defaults(&dn);
    std::string featuresOut;
    bool trackVariance = false, haveTarget = false, haveTargetOption = false;
    float noiseTarget = 0.f;
    int checkEvery = 4, maxIterations = 1024;
    int robust = 0;
    vcm_robust_stats rs = {};
    std::string partsOut;
    vcm_parts_stats ps = {};
    DisplayFlags disp = {};
    vcm_display_defaults(&disp.p);
    vcm_display_stats ds = {};
    bool displayed = false;
    std::string refFile, compareLog, errorMap;
    int compareEvery = 0;
    bool haveErrorTarget = false, haveCompareOption = false, haveMaxIterations = false;
    float errorTarget = 0.f;
    vcm_compare_stats cs = {};
    int compareChecks = 0;
    for (int i = 1; i < argc; i++) {
        const std::string a(argv[i]);
        if (const int taken = display_parse_flag(argc, argv, i, disp)) { if (taken < 0) return 2; continue; }
        auto need = [&](int n) { if (i + n >= argc) { fprintf(stderr, "vcm_render: %s needs %d argument(s)\n", a.c_str(), n); exit(2); } };
        if (a == "-s") { need(1); sceneID = atoi(argv[++i]); }
        else if (a == "-a") { need(1); algoName = argv[++i]; algorithm = algorithm_by_acronym(algoName); }
        else if (a == "-i") { need(1); iterations = atoi(argv[++i]); }
        else if (a == "-o") { need(1); out = argv[++i]; }
        else if (a == "--res") { need(2); resX = atoi(argv[++i]); resY = atoi(argv[++i]); }
        else if (a == "--seed") { need(1); seed = atoi(argv[++i]); }
        else if (a == "--minlen") { need(1); minLen = (unsigned)atoi(argv[++i]); }
        else if (a == "--maxlen") { need(1); maxLen = (unsigned)atoi(argv[++i]); }
        else if (a == "--renderers") { need(1); renderers = atoi(argv[++i]); }
        else if (a == "--radius-factor") { need(1); radiusFactor = (float)atof(argv[++i]); }
        else if (a == "--radius-alpha") { need(1); radiusAlpha = (float)atof(argv[++i]); }
        else if (a == "--device") { need(1); device = atoi(argv[++i]); }
        else if (a == "--warmup") { need(1); warmup = atoi(argv[++i]); }
        else if (a == "--gpus") { need(1); gpus = atoi(argv[++i]); }
        else if (a == "--shards") { need(1); shards = atoi(argv[++i]); }
        else if (a == "--inflight") { need(1); inflight = atoi(argv[++i]); }
        else if (a == "--collectives") { need(1); rccl = std::string(argv[++i]) == "threads" ? 0 : 1; }
        else if (a == "--devices") { need(1); for (const char *p = argv[++i]; *p;) { char *e; devices.push_back((int)strtol(p, &e, 10)); p = (*e == ',') ? e + 1 : e; if (e == p && *p) break; } }
        else if (a == "--same-window") sameWindow = 1;   // benchmark schedule: every renderer runs the iteration indices warmup ..
        else if (a == "--scene-file") { need(1); sceneFile = argv[++i]; }   // instead of -s: OBJ + MTL / .vcmscene (vcm_scene_load)
        else if (a == "--envmap") { need(1); envFile = argv[++i]; }
        else if (a == "--envmap-scale") { need(1); envScale = (float)atof(argv[++i]); }
        else if (a == "--aperture" || a == "--focus") {
            need(1);
            char *e = NULL;
            const float v = strtof(argv[++i], &e);
            if (e == argv[i] || *e) { fprintf(stderr, "vcm_render: %s needs a number\n", a.c_str()); return 2; }
            if (a == "--aperture") { aperture = v; haveAperture = true; } else { focus = v; haveFocus = true; }
        }
        else if (a == "--light-pick") { need(1); pickName = argv[++i]; }
        else if (a == "--light-pick-mix") {
            need(1);
            char *e = NULL;
            pickMix = strtof(argv[++i], &e);
            if (e == argv[i] || *e) { fprintf(stderr, "vcm_render: %s needs a number\n", a.c_str()); return 2; }
            havePickMix = true;
        }
        else if (a == "--light-pick-report") pickReport = true;
        else if (a == "--filter") {
            need(2);
            filterName = argv[++i];
            char *e = NULL;
            filterRadius = strtof(argv[++i], &e);
            if ((filterName != "tent" && filterName != "bspline") || e == argv[i] || *e) { fprintf(stderr, "vcm_render: --filter tent|bspline R\n"); return 2; }
        }
        else if (a == "--sampler") {
            need(1);
            samplerName = argv[++i];
            if (samplerName != "sobol" && samplerName != "philox") { fprintf(stderr, "vcm_render: --sampler sobol|philox\n"); return 2; }
        }
        else if (a == "--projection") {
            need(1);
            projName = argv[++i];
            if (projName != "fisheye" && projName != "panorama") { fprintf(stderr, "vcm_render: --projection fisheye DEG|panorama\n"); return 2; }
            if (projName == "fisheye") {
                need(1);
                char *e = NULL;
                projFov = strtof(argv[++i], &e);
                if (e == argv[i] || *e) { fprintf(stderr, "vcm_render: --projection fisheye DEG|panorama\n"); return 2; }
            }
        }
        else if (a == "--denoise") {
            denoise = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') dn.passes = atoi(argv[++i]);
        }
        else if (a == "--denoise-sigma") {
            need(1);
            if (sscanf(argv[++i], "%f,%f,%f", &dn.sigmaColor, &dn.sigmaNormal, &dn.sigmaDepth) != 3) { fprintf(stderr, "vcm_render: --denoise-sigma c,n,z\n"); return 2; }
        }
        else if (a == "--no-demodulate") dn.demodulate = 0;
        else if (a == "--features-out") { need(1); featuresOut = argv[++i]; }
        else if (a == "--noise-target") {
            need(1);
            char *e = NULL;
            noiseTarget = strtof(argv[++i], &e);
            if (e == argv[i] || *e || !(noiseTarget >= 0.f)) { fprintf(stderr, "vcm_render: --noise-target needs a number >= 0\n"); return 2; }
            haveTarget = trackVariance = true;
        }
        else if (a == "--check-every") { need(1); checkEvery = atoi(argv[++i]); haveTargetOption = true; }
        else if (a == "--max-iterations") { need(1); maxIterations = atoi(argv[++i]); haveMaxIterations = true; }
        else if (a == "--reference") { need(1); refFile = argv[++i]; }
        else if (a == "--compare-every") { need(1); compareEvery = atoi(argv[++i]); haveCompareOption = true; if (compareEvery < 1) { fprintf(stderr, "vcm_render: --compare-every >= 1\n"); return 2; } }
        else if (a == "--compare-log") { need(1); compareLog = argv[++i]; haveCompareOption = true; }
        else if (a == "--error-map") { need(1); errorMap = argv[++i]; haveCompareOption = true; }
        else if (a == "--error-target") {
            need(1);
            char *e = NULL;
            errorTarget = strtof(argv[++i], &e);
            if (e == argv[i] || *e || !(errorTarget >= 0.f)) { fprintf(stderr, "vcm_render: --error-target needs a number >= 0\n"); return 2; }
            haveErrorTarget = haveCompareOption = true;
        }
        else if (a == "--track-variance") trackVariance = true;
        else if (a == "--robust") {
            robust = VCM_ROBUST_DEFAULT_BUCKETS;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') robust = atoi(argv[++i]);
            if (robust < 3 || robust > 15 || robust % 2 == 0) { fprintf(stderr, "vcm_render: --robust takes an odd number of buckets, 3 .. 15\n"); return 2; }
        }
        else if (a == "--parts") { need(1); partsOut = argv[++i]; }
        else if (a == "--strict") strict = 1;
        else if (a == "--json") json = 1;
        else { fprintf(stderr, "vcm_render: unknown option %s (see the header of vcm_render.cpp)\n", a.c_str()); return 2; }
    }
    if (algorithm < 0 || sceneID < 0 || sceneID > 3 || iterations < 1 || resX < 1 || resY < 1 || renderers < 1) {
        fprintf(stderr, "vcm_render: invalid argument\n");
        return 2;
    }
    if ((denoise || !featuresOut.empty()) && (renderers != 1 || gpus > 0)) {
        fprintf(stderr, "vcm_render: --denoise and --features-out want one renderer on one GPU (a farm host denoises the reduced frame with vcm_denoise_buffers)\n");
        return 2;
    }
    if (trackVariance && (renderers != 1 || gpus > 0)) {
        fprintf(stderr, "vcm_render: --noise-target and --track-variance want one renderer on one GPU (a farm host reduces the frames and calls vcm_variance_update_buffers)\n");
        return 2;
    }
    if (robust && denoise) {
        fprintf(stderr, "vcm_render: --robust and --denoise do not combine yet: the filter takes the mean (a host may feed vcm_robust_device to vcm_denoise_buffers)\n");
        return 2;
    }
    if (robust && (renderers != 1 || gpus > 0)) {
        fprintf(stderr, "vcm_render: --robust wants one renderer on one GPU (a farm host reduces the frames and calls vcm_robust_update_buffers)\n");
        return 2;
    }
    if (disp.any && (renderers != 1 || gpus > 0)) {
        fprintf(stderr, "vcm_render: --tonemap, --exposure, --auto-exposure, --bloom, --srgb and --dither want one renderer on one GPU (a farm host reduces the frames and calls vcm_display_buffers)\n");
        return 2;
    }
    if (!partsOut.empty() && (renderers != 1 || gpus > 0)) {
        fprintf(stderr, "vcm_render: --parts wants one renderer on one GPU (the technique breakdown is kept beside one context's framebuffer)\n");
        return 2;
    }
    if (!partsOut.empty() && (algorithm == VCM_ALGO_PATH_TRACE || algorithm == VCM_ALGO_EYE_LIGHT)) {
        fprintf(stderr, "vcm_render: --parts wants a VertexCM algorithm (lt, ppm, bpm, bpt, vcm): %s has no technique split\n", algoName.c_str());
        return 2;
    }
    if (!partsOut.empty() && (strict || maxLen > 31)) {
        fprintf(stderr, "vcm_render: --parts reads what wavefront mode keeps apart: no --strict, --maxlen <= 31\n");
        return 2;
    }
    if (haveCompareOption && refFile.empty()) { fprintf(stderr, "vcm_render: --compare-every, --compare-log, --error-target and --error-map go with --reference\n"); return 2; }
    if (!refFile.empty() && (renderers != 1 || gpus > 0)) {
        fprintf(stderr, "vcm_render: --reference wants one renderer on one GPU (a farm host reduces the frames and calls vcm_compare_buffers)\n");
        return 2;
    }
    if (!refFile.empty() && robust && ((haveTarget || haveErrorTarget) ? maxIterations : iterations) < robust) {
        fprintf(stderr, "vcm_render: --reference with --robust %d wants at least %d iterations: the estimate cannot be resolved, and so not compared, before\n", robust, robust);
        return 2;
    }
    if (haveErrorTarget && haveTarget) { fprintf(stderr, "vcm_render: --error-target and --noise-target do not combine\n"); return 2; }
    if (haveErrorTarget && maxIterations < 1) { fprintf(stderr, "vcm_render: --max-iterations >= 1\n"); return 2; }
    if ((haveTargetOption || (haveMaxIterations && !haveErrorTarget)) && !haveTarget) { fprintf(stderr, "vcm_render: --check-every and --max-iterations go with --noise-target\n"); return 2; }
    if (haveTarget && (checkEvery < 1 || maxIterations < 2)) { fprintf(stderr, "vcm_render: --check-every >= 1, --max-iterations >= 2\n"); return 2; }
    if (haveAperture != haveFocus) { fprintf(stderr, "vcm_render: --aperture and --focus go together\n"); return 2; }
    if (!pickName.empty() && pickName != "uniform" && pickName != "power") { fprintf(stderr, "vcm_render: --light-pick uniform|power\n"); return 2; }
    if (havePickMix && pickName.empty()) { fprintf(stderr, "vcm_render: --light-pick-mix goes with --light-pick\n"); return 2; }

    vcm_scene_desc scene;
    if (vcm_scene_cornell(resX, resY, vcm_scene_config_mask(sceneID), &scene)) return die("vcm_scene_cornell");
    vcm_scene_file *loaded = NULL;   // --scene-file: a version-2 description (any number of primitives, BVH)
    const vcm_scene_desc3 *envScene = NULL;   // a scene with an environment map (--envmap, or a scene file's `light envmap`)
    if (!sceneFile.empty()) {
        loaded = vcm_scene_load(sceneFile.c_str(), resX, resY);
        if (!loaded) { fprintf(stderr, "vcm_render: %s\n", vcm_scene_load_error()); return 2; }
        if (gpus > 0) { fprintf(stderr, "vcm_render: --scene-file with --gpus is not supported (the farm takes the built-in scenes)\n"); return 2; }
        if (vcm_scene_file_desc3(loaded)->envmap) envScene = vcm_scene_file_desc3(loaded);
    }
    // --envmap: the built-in scene as a version-3 description whose background light is the map
    vcm_envmap *envmap = NULL;
    std::vector<vcm_light> envLights;
    vcm_scene_desc3 envDesc;
    if (!envFile.empty()) {
        if (gpus > 0) { fprintf(stderr, "vcm_render: --envmap with --gpus is not supported (the farm takes the built-in scenes)\n"); return 2; }
        if (loaded) { fprintf(stderr, "vcm_render: --envmap with --scene-file: name the map in the scene file (light envmap)\n"); return 2; }
        if (scene.backgroundLight < 0) { fprintf(stderr, "vcm_render: --envmap replaces the scene's background light; scene %d has none (scene 3 has)\n", sceneID); return 2; }
        envmap = vcm_envmap_load(envFile.c_str());
        if (!envmap) { fprintf(stderr, "vcm_render: %s\n", vcm_scene_load_error()); return 2; }
        envLights.assign(scene.lights, scene.lights + scene.nLights);
        vcm_make_envmap_light(envScale, &envLights[(size_t)scene.backgroundLight]);
        memset(&envDesc, 0, sizeof(envDesc));
        vcm_scene_desc2 &b = envDesc.base;
        scene_as_desc2(scene, b);
        b.lights = envLights.data();
        envDesc.envmap = envmap;
        envScene = &envDesc;
    }
    // a thin lens (--aperture / --focus, else a scene file's `lens`): the scene as a version-4 description
    vcm_thin_lens flagLens;
    flagLens.apertureRadius = aperture; flagLens.focusDistance = focus;
    const vcm_thin_lens *lens = haveAperture ? &flagLens : loaded ? vcm_scene_file_desc4(loaded)->lens : NULL;
    vcm_scene_desc4 lensDesc;
    const vcm_scene_desc4 *lensScene = NULL;
    if (lens) {
        if (gpus > 0) { fprintf(stderr, "vcm_render: a lens with --gpus is not supported (the farm takes version-1 scenes)\n"); return 2; }
        memset(&lensDesc, 0, sizeof(lensDesc));
        if (envScene) lensDesc.base = *envScene;
        else if (loaded) lensDesc.base = *vcm_scene_file_desc3(loaded);
        else scene_as_desc2(scene, lensDesc.base.base);   // the built-in scene (the arrays stay in `scene`)
        lensDesc.lens = lens;
        lensScene = &lensDesc;
    }
    // light selection (--light-pick, else a scene file's `lightpick`): the scene as a version-5 description
    vcm_light_pick flagPick;
    flagPick.mode = pickName == "power" ? VCM_LIGHT_PICK_POWER : VCM_LIGHT_PICK_UNIFORM;
    flagPick.uniformMix = pickMix; flagPick.weights = NULL;
    const vcm_light_pick *pick = !pickName.empty() ? &flagPick : loaded ? vcm_scene_file_desc5(loaded)->pick : NULL;
    if (pick && pick->mode == VCM_LIGHT_PICK_UNIFORM && gpus > 0) pick = NULL;   // the uniform choice is what the farm does
    vcm_scene_desc5 pickDesc;
    const vcm_scene_desc5 *pickScene = NULL;
    if (pick) {
        if (gpus > 0) { fprintf(stderr, "vcm_render: --light-pick with --gpus is not supported (the farm takes version-1 scenes)\n"); return 2; }
        memset(&pickDesc, 0, sizeof(pickDesc));
        if (lensScene) pickDesc.base = *lensScene;
        else {
            if (envScene) pickDesc.base.base = *envScene;
            else if (loaded) pickDesc.base.base = *vcm_scene_file_desc3(loaded);
            else scene_as_desc2(scene, pickDesc.base.base.base);   // the built-in scene (the arrays stay in `scene`)
            pickDesc.base.lens = NULL;
        }
        pickDesc.pick = pick;
        pickScene = &pickDesc;
    }
    // the pixel filter (--filter, else a scene file's `filter`): the scene as a version-6 description
    vcm_pixel_filter flagFilter;
    flagFilter.kind = filterName == "tent" ? VCM_FILTER_TENT : VCM_FILTER_BSPLINE;
    flagFilter.radius = filterRadius;
    const vcm_pixel_filter *filter = !filterName.empty() ? &flagFilter : loaded ? vcm_scene_file_desc6(loaded)->filter : NULL;
    vcm_scene_desc6 filterDesc;
    const vcm_scene_desc6 *filterScene = NULL;
    if (filter && gpus <= 0) {
        memset(&filterDesc, 0, sizeof(filterDesc));
        if (pickScene) filterDesc.base = *pickScene;
        else if (lensScene) filterDesc.base.base = *lensScene;
        else if (envScene) filterDesc.base.base.base = *envScene;
        else if (loaded) filterDesc.base.base.base = *vcm_scene_file_desc3(loaded);
        else scene_as_desc2(scene, filterDesc.base.base.base.base);   // the built-in scene (the arrays stay in `scene`)
        filterDesc.filter = filter;
        filterScene = &filterDesc;
    }
    // the sampler (--sampler, else a scene file's `sampler`): the scene as a version-7 description
    vcm_sampler flagSampler;
    flagSampler.kind = samplerName == "sobol" ? VCM_SAMPLER_SOBOL : VCM_SAMPLER_PHILOX;
    const vcm_sampler *sampler = !samplerName.empty() ? &flagSampler : loaded ? vcm_scene_file_desc7(loaded)->sampler : NULL;
    vcm_scene_desc7 samplerDesc;
    const vcm_scene_desc7 *samplerScene = NULL;
    if (sampler && sampler->kind != VCM_SAMPLER_PHILOX && gpus <= 0) {
        memset(&samplerDesc, 0, sizeof(samplerDesc));
        if (filterScene) samplerDesc.base = *filterScene;
        else if (pickScene) samplerDesc.base.base = *pickScene;
        else if (lensScene) samplerDesc.base.base.base = *lensScene;
        else if (envScene) samplerDesc.base.base.base.base = *envScene;
        else if (loaded) samplerDesc.base.base.base.base = *vcm_scene_file_desc3(loaded);
        else scene_as_desc2(scene, samplerDesc.base.base.base.base.base);   // the built-in scene (the arrays stay in `scene`)
        samplerDesc.sampler = sampler;
        samplerScene = &samplerDesc;
    }
    // the GGX lobes of a scene file's `Pr` materials: the scene as a version-8 description over whatever the flags made of it
    const vcm_material_ext *materialExt = loaded ? vcm_scene_file_desc8(loaded)->materialExt : NULL;
    vcm_scene_desc8 ggxDesc;
    const vcm_scene_desc8 *ggxScene = NULL;
    if (materialExt && gpus <= 0) {
        memset(&ggxDesc, 0, sizeof(ggxDesc));
        if (samplerScene) ggxDesc.base = *samplerScene;
        else if (filterScene) ggxDesc.base.base = *filterScene;
        else if (pickScene) ggxDesc.base.base.base = *pickScene;
        else if (lensScene) ggxDesc.base.base.base.base = *lensScene;
        else if (envScene) ggxDesc.base.base.base.base.base = *envScene;
        else ggxDesc.base.base.base.base.base = *vcm_scene_file_desc3(loaded);
        ggxDesc.materialExt = materialExt;
        ggxScene = &ggxDesc;
    }
    if (materialExt && gpus > 0) { fprintf(stderr, "vcm_render: a scene file with Pr materials cannot be rendered with --gpus yet\n"); return 1; }
    // the projection (--projection, else a scene file's `projection`): the scene as a version-9 description over whatever the flags made of it
    vcm_camera_model flagModel;
    flagModel.kind = projName == "fisheye" ? VCM_PROJ_FISHEYE : VCM_PROJ_PANORAMA;
    flagModel.fovDegrees = projFov;
    const vcm_camera_model *model = !projName.empty() ? &flagModel : loaded ? vcm_scene_file_desc9(loaded)->model : NULL;
    vcm_scene_desc9 projDesc;
    const vcm_scene_desc9 *projScene = NULL;
    if (model && model->kind != VCM_PROJ_PERSPECTIVE) {
        if (gpus > 0) { fprintf(stderr, "vcm_render: a projection with --gpus is not supported (the farm takes version-1 scenes)\n"); return 2; }
        memset(&projDesc, 0, sizeof(projDesc));
        if (ggxScene) projDesc.base = *ggxScene;
        else if (samplerScene) projDesc.base.base = *samplerScene;
        else if (filterScene) projDesc.base.base.base = *filterScene;
        else if (pickScene) projDesc.base.base.base.base = *pickScene;
        else if (lensScene) projDesc.base.base.base.base.base = *lensScene;
        else if (envScene) projDesc.base.base.base.base.base.base = *envScene;
        else if (loaded) projDesc.base.base.base.base.base.base = *vcm_scene_file_desc3(loaded);
        else scene_as_desc2(scene, projDesc.base.base.base.base.base.base.base);   // the built-in scene (the arrays stay in `scene`)
        projDesc.model = model;
        projScene = &projDesc;
    }
    auto create = [&](int s) {
        return projScene ? vcm_create_sharded9(projScene, algorithm, radiusFactor, radiusAlpha, s, device, 0, 1)
             : ggxScene ? vcm_create_sharded8(ggxScene, algorithm, radiusFactor, radiusAlpha, s, device, 0, 1)
             : samplerScene ? vcm_create_sharded7(samplerScene, algorithm, radiusFactor, radiusAlpha, s, device, 0, 1)
             : filterScene ? vcm_create_sharded6(filterScene, algorithm, radiusFactor, radiusAlpha, s, device, 0, 1)
             : pickScene ? vcm_create_sharded5(pickScene, algorithm, radiusFactor, radiusAlpha, s, device, 0, 1)
             : lensScene ? vcm_create_sharded4(lensScene, algorithm, radiusFactor, radiusAlpha, s, device, 0, 1)
             : envScene ? vcm_create_sharded3(envScene, algorithm, radiusFactor, radiusAlpha, s, device, 0, 1)
             : loaded ? vcm_create_sharded2(vcm_scene_file_desc(loaded), algorithm, radiusFactor, radiusAlpha, s, device, 0, 1)
                      : vcm_create_sharded(&scene, algorithm, radiusFactor, radiusAlpha, s, device, 0, 1);
    };

    const size_t n3 = (size_t)resX * resY * 3;
    std::vector<float> fb(n3, 0.f), tmp(n3);
    double wall = 0;
    vcm_stats st;
    memset(&st, 0, sizeof(st));
    std::vector<vcm_ctx *> r;
    if (gpus > 0) {   // multi-GPU host: ranks x shards x in-flight renderers (vcm_farm.hpp)
        FarmConfig fc;
        fc.scene = scene; fc.algorithm = algorithm; fc.radiusFactor = radiusFactor; fc.radiusAlpha = radiusAlpha;
        fc.baseSeed = seed; fc.minLen = minLen; fc.maxLen = maxLen; fc.iterations = iterations; fc.ranks = gpus;
        fc.shards = shards > 0 ? shards : gpus;        // default: north_star's decomposition, one renderer across all GPUs
        fc.inflight = inflight > 0 ? inflight : 1;
        fc.rccl = rccl != 0; fc.warmup = warmup;
        fc.firstRank = 0; fc.localRanks = gpus;   // every rank is a thread of this process
        fc.sameWindow = sameWindow != 0;
        if (filter) fc.filter = *filter;
        if (sampler) fc.sampler = *sampler;
        const int visible = vcm_device_count();
        if (visible <= 0) { fprintf(stderr, "vcm_render: no HIP device available (this program has no CPU path)\n"); return 2; }
        for (int k = 0; k < gpus; k++) fc.devices.push_back(k < (int)devices.size() ? devices[(size_t)k] : (fc.rccl ? k : k % visible));
        for (int d : fc.devices) if (d < 0 || d >= visible) { fprintf(stderr, "vcm_render: device %d not visible (%d device(s))\n", d, visible); return 2; }
        const FarmResult fr = farm_render(fc);
        if (!fr.error.empty()) { fprintf(stderr, "vcm_render: %s\n", fr.error.c_str()); return 2; }
        fb = fr.image;
        wall = fr.wallSeconds;
        renderers = fr.renderers;
        rcclRanks = fr.rcclRanks;
        rankMs = fr.rankIterationMs;
        st = fr.meanStats;
    } else {
    // render(): one renderer per "thread", seed base + i (smallvcm.cxx:61-72)
    r.assign((size_t)renderers, (vcm_ctx *)NULL);
    for (int g = 0; g < renderers; g++) {
        r[g] = create(seed + g);
        if (!r[g]) return die("vcm_create");
        if (strict && vcm_set_strict_order(r[g], 1)) return die("vcm_set_strict_order");
        if (trackVariance && vcm_track_variance(r[g], 1)) return die("vcm_track_variance");
        if (robust && vcm_track_robust(r[g], robust)) return die("vcm_track_robust");
        if (!partsOut.empty() && vcm_track_parts(r[g], 1)) return die("vcm_track_parts");
    }
    if (!refFile.empty()) {   // the reference image: a .pfm or .hdr of the frame's resolution
        vcm_envmap *ref = vcm_envmap_load(refFile.c_str());
        if (!ref) { fprintf(stderr, "vcm_render: --reference: %s\n", vcm_scene_load_error()); return 2; }
        if (ref->width != resX || ref->height != resY) {
            fprintf(stderr, "vcm_render: --reference %s is %d x %d, the frame %d x %d\n", refFile.c_str(), ref->width, ref->height, resX, resY);
            vcm_envmap_free(ref);
            return 2;
        }
        // a .pfm is read as this program (and the reference's SavePFM) writes it, rows top to bottom; vcm_envmap_load takes a
        // PFM's rows bottom-up, as the format has them, so its rows are turned back
        std::vector<float> rows(ref->rgb, ref->rgb + (size_t)resX * resY * 3);
        const std::string ext = refFile.size() >= 4 ? refFile.substr(refFile.size() - 4) : "";
        if (ext == ".pfm" || ext == ".PFM")
            for (int y = 0; y < resY; y++) memcpy(&rows[(size_t)y * resX * 3], ref->rgb + (size_t)(resY - 1 - y) * resX * 3, (size_t)resX * 3 * sizeof(float));
        const int rc = vcm_set_reference(r[0], rows.data());
        vcm_envmap_free(ref);
        if (rc) return die("vcm_set_reference");
    }
    if (pick && (pick->mode != VCM_LIGHT_PICK_UNIFORM || pickReport) && !json) {
        const int nLights = pickScene->base.base.base.nLights;
        printf("light pick: %s, uniform mix %g, %d light(s)\n", pick->mode == VCM_LIGHT_PICK_POWER ? "power" : "uniform", pick->uniformMix, nLights);
        if (pickReport) {   // every light's probability through the known-answer op, the five largest printed
            std::vector<float> in((size_t)nLights * VCM_KAT_FLOATS, 0.f), res(in.size());
            for (int l = 0; l < nLights; l++) { in[(size_t)l * VCM_KAT_FLOATS] = 0.5f; in[(size_t)l * VCM_KAT_FLOATS + 1] = (float)l; }
            if (vcm_debug_kat(r[0], VCM_KAT_LIGHT_PICK, nLights, in.data(), res.data())) return die("vcm_debug_kat");
            std::vector<std::pair<float, int>> top;
            for (int l = 0; l < nLights; l++) top.push_back(std::make_pair(-res[(size_t)l * VCM_KAT_FLOATS + 2], l));
            std::sort(top.begin(), top.end());
            static const char *const typeNames[] = { "area", "directional", "point", "background", "envmap", "spot", "sphere" };
            const vcm_light *lights = pickScene->base.base.base.lights;
            for (size_t k = 0; k < top.size() && k < 5; k++) {
                const int t = lights[top[k].second].type;
                printf("  light %d (%s): pmf %.7g\n", top[k].second, t >= 0 && t <= VCM_LIGHT_SPHERE ? typeNames[t] : "?", -top[k].first);
            }
        }
    }
    // untimed warm-up on a throw-away renderer: allocations, first-launch costs
    if (warmup > 0) {
        vcm_ctx *w = create(seed);
        if (!w) return die("vcm_create");
        for (int it = 0; it < warmup; it++) if (vcm_run_iteration(w, it, minLen, maxLen)) return die("vcm_run_iteration");
        vcm_synchronize(w);
        vcm_destroy(w);
    }

    const auto t0 = std::chrono::steady_clock::now();
    // static schedule of `#pragma omp parallel for` (smallvcm.cxx:98-108): contiguous blocks, the first
    // iterations % renderers threads get one more
    if (haveTarget || !refFile.empty()) {   // one renderer, iterations 0, 1, ...: looks at the noise statistic, at the error against the reference, or both
        FILE *log = NULL;
        if (!compareLog.empty()) {
            log = fopen(compareLog.c_str(), "w");
            if (!log) { fprintf(stderr, "vcm_render: cannot write %s\n", compareLog.c_str()); return 2; }
            fprintf(log, "iteration,relMSE,MSE,PSNR,SSIM,maxAbs,nonFinite\n");
        }
        // with a stop rule (--noise-target, --error-target) up to --max-iterations; the error is looked at every --compare-every
        // iterations (default: 4 with --error-target, --check-every with --noise-target, else never), after the last iteration and
        // where the noise target stops the run
        const int last = (haveTarget || haveErrorTarget) ? maxIterations : iterations;
        const int every = compareEvery > 0 ? compareEvery : (haveErrorTarget ? 4 : (haveTarget ? checkEvery : 0));
        vcm_compare_params cp;
        vcm_compare_defaults(&cp);
        if (haveErrorTarget) cp.threshold = errorTarget;
        vcm_noise_stats ns;
        for (iterations = 0; iterations < last;) {
            if (vcm_run_iteration(r[0], iterations, minLen, maxLen)) return die("vcm_run_iteration");
            iterations++;
            bool stop = iterations == last;
            if (haveTarget && iterations >= 2 && (iterations % checkEvery == 0 || iterations == last)) {
                if (vcm_get_noise_stats(r[0], noiseTarget, &ns)) return die("vcm_get_noise_stats");
                if (!json) printf("noise after %d iteration(s): mean %.9g, max %.9g, %lld of %lld above the target, %lld non-finite\n",
                                  ns.iterations, ns.mean, ns.max, ns.above, ns.elements, ns.nonFinite);
                if (ns.mean <= (double)noiseTarget) stop = true;
            }
            if (!refFile.empty() && (stop || (every > 0 && iterations % every == 0)) && !(robust && iterations < robust)) {   // (a robust estimate
                // of fewer iterations than buckets is not resolvable: refused before rendering for the last iteration, skipped before it)
                if (denoise && vcm_denoise(r[0], 1.f / iterations, &dn)) return die("vcm_denoise");
                const int source = denoise ? VCM_DISPLAY_DENOISED : (robust ? VCM_DISPLAY_ROBUST : VCM_DISPLAY_FRAMEBUFFER);
                cp.writeMap = (!errorMap.empty() && (stop || haveErrorTarget)) ? 1 : 0;
                if (vcm_compare(r[0], source, source == VCM_DISPLAY_FRAMEBUFFER ? 1.f / iterations : 1.f, &cp, &cs)) return die("vcm_compare");
                compareChecks++;
                if (!json) printf("compare after %d iteration(s): relMSE %.9g MSE %.9g PSNR %.6g SSIM %.9g maxAbs %.9g nonFinite %lld\n", iterations,
                                  cs.relMse, cs.mse, cs.psnr, cs.ssim, cs.maxAbs, cs.nonFinite);
                if (log) fprintf(log, "%d,%.17g,%.17g,%.17g,%.17g,%.17g,%lld\n", iterations, cs.relMse, cs.mse, cs.psnr, cs.ssim, cs.maxAbs, cs.nonFinite);
                if (haveErrorTarget && cs.relMse <= (double)errorTarget) stop = true;
            }
            if (stop) break;
        }
        if (haveTarget && !json) printf("noise target %g: %d iteration(s) used\n", noiseTarget, iterations);
        if (log) fclose(log);
        if (haveErrorTarget && !json) printf("error target %g: %d iteration(s) used\n", errorTarget, iterations);
        if (!refFile.empty() && compareChecks == 0) {   // the noise target stopped a --robust run before it had an iteration per bucket
            fprintf(stderr, "vcm_render: --reference: no check was possible, the robust estimate needs %d iterations and the run ended after %d\n", robust, iterations);
            return 2;
        }
        if (!errorMap.empty()) {   // the last check's relative squared error, rows top to bottom like SavePFM
            std::vector<float> m4((size_t)resX * resY * 4), m3((size_t)resX * resY * 3);
            if (vcm_read_compare_map(r[0], m4.data())) return die("vcm_read_compare_map");
            for (size_t p = 0; p < (size_t)resX * resY; p++) for (int k = 0; k < 3; k++) m3[p * 3 + k] = m4[p * 4 + k];
            FILE *f = fopen(errorMap.c_str(), "wb");
            if (!f) { fprintf(stderr, "vcm_render: cannot write %s\n", errorMap.c_str()); return 2; }
            fprintf(f, "PF\n%d %d\n-1\n", resX, resY);
            fwrite(m3.data(), sizeof(float), m3.size(), f);
            fclose(f);
        }
    }
    const int q = iterations / renderers, rem = iterations % renderers;
    for (int g = 0; g < renderers && !haveTarget && refFile.empty(); g++) {
        const int lo = g * q + (g < rem ? g : rem), n = q + (g < rem ? 1 : 0);
        for (int it = lo; it < lo + n; it++)
            if (vcm_run_iteration(r[g], it, minLen, maxLen)) return die("vcm_run_iteration");
    }
    for (int g = 0; g < renderers; g++) if (vcm_synchronize(r[g])) return die("vcm_synchronize");
    wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    // accumulate the used renderers: mean of (running sum / own iterations), smallvcm.cxx:116-142
    int used = 0;
    for (int g = 0; g < renderers; g++) {
        const int its = vcm_iterations(r[g]);
        if (its == 0) continue;                       // WasUsed(), renderer.hxx:58
        if (vcm_read_framebuffer(r[g], tmp.data())) return die("vcm_read_framebuffer");
        const float s = 1.f / its;                    // renderer.hxx:53-54
        if (used == 0) for (size_t i = 0; i < n3; i++) fb[i] = tmp[i] * s;
        else for (size_t i = 0; i < n3; i++) fb[i] = fb[i] + tmp[i] * s;   // Framebuffer::Add, framebuffer.hxx:75-79
        used++;
    }
    const float su = 1.f / used;                      // Framebuffer::Scale, smallvcm.cxx:142
    for (size_t i = 0; i < n3; i++) fb[i] = fb[i] * su;
    vcm_get_stats(r[0], &st);
    if (trackVariance && !haveTarget && !json && iterations >= 2) {
        vcm_noise_stats ns;
        if (vcm_get_noise_stats(r[0], 0.f, &ns)) return die("vcm_get_noise_stats");
        printf("noise after %d iteration(s): mean %.9g, max %.9g, %lld non-finite\n", ns.iterations, ns.mean, ns.max, ns.nonFinite);
    }
    if (robust) {   // the estimate takes the mean's place in everything below
        if (vcm_read_robust(r[0], fb.data())) return die("vcm_read_robust");
        if (vcm_get_robust_stats(r[0], &rs)) return die("vcm_get_robust_stats");
        if (!json) printf("robust estimate after %d iteration(s) in %d buckets: %lld of %lld pixels trimmed, %lld with a non-finite bucket, Gini mean %.9g, max %.9g\n",
                          rs.iterations, rs.buckets, rs.trimmed, rs.pixels, rs.nonFinite, rs.meanGini, rs.maxGini);
    }
    if (!partsOut.empty()) {   // the five planes / iterations, rows top to bottom like SavePFM, and their shares
        const char *name[VCM_PART_COUNT] = { "emission", "direct", "connect", "merge", "lighttrace" };
        if (vcm_get_parts_stats(r[0], &ps)) return die("vcm_get_parts_stats");
        for (int k = 0; k < VCM_PART_COUNT; k++) {
            if (vcm_read_part(r[0], k, 1.f / ps.iterations, tmp.data())) return die("vcm_read_part");
            const std::string path = partsOut + "_" + name[k] + ".pfm";
            FILE *f = fopen(path.c_str(), "wb");
            if (!f) { fprintf(stderr, "vcm_render: cannot write %s\n", path.c_str()); return 2; }
            fprintf(f, "PF\n%d %d\n-1\n", resX, resY);
            fwrite(tmp.data(), sizeof(float), n3, f);
            fclose(f);
        }
        double total = 0;
        for (int k = 0; k < VCM_PART_COUNT; k++) total += ps.luminance[k];
        if (!json) {
            printf("technique breakdown after %d iteration(s), %lld pixel(s) with a non-finite value left out:\n", ps.iterations, ps.nonFinite);
            for (int k = 0; k < VCM_PART_COUNT; k++)
                printf("  %-10s %6.2f %% of the luminance\n", name[k], total > 0 ? 100.0 * ps.luminance[k] / total : 0.0);
        }
    }
    }

    if (!featuresOut.empty()) {   // the guide images, rows top to bottom like SavePFM
        const int which[3] = { VCM_FEATURE_ALBEDO, VCM_FEATURE_NORMAL, VCM_FEATURE_DEPTH };
        const char *name[3] = { ".albedo.pfm", ".normal.pfm", ".depth.pfm" };
        for (int k = 0; k < 3; k++) {
            const size_t nf = (size_t)resX * resY * (k == 2 ? 1 : 3);
            if (vcm_read_feature(r[0], which[k], tmp.data())) return die("vcm_read_feature");
            FILE *f = fopen((featuresOut + name[k]).c_str(), "wb");
            if (!f) { fprintf(stderr, "vcm_render: cannot write %s%s\n", featuresOut.c_str(), name[k]); return 2; }
            fprintf(f, "%s\n%d %d\n-1\n", k == 2 ? "Pf" : "PF", resX, resY);
            fwrite(tmp.data(), sizeof(float), nf, f);
            fclose(f);
        }
    }
    std::vector<float> clean;
    if (denoise) {
        if (vcm_denoise(r[0], 1.f / vcm_iterations(r[0]), &dn)) return die("vcm_denoise");
        clean.resize(n3);
        if (vcm_read_denoised(r[0], clean.data())) return die("vcm_read_denoised");
    }
    // img: the fp32 image; denoised: the 8-bit encodings come from the context's denoised image, else from its framebuffer
    auto save = [&](const std::string &path, const std::vector<float> &img, bool denoised) -> int {
        const std::string ext = path.size() >= 4 ? path.substr(path.size() - 4) : "";
        const bool bmp = ext == ".bmp", hdr = ext == ".hdr";
        std::vector<unsigned char> px;
        if (disp.any) {   // the display transform: its statistics in any case, its bytes for a .bmp
            const int source = denoised ? VCM_DISPLAY_DENOISED : (robust ? VCM_DISPLAY_ROBUST : VCM_DISPLAY_FRAMEBUFFER);
            if (vcm_display(r[0], source, source == VCM_DISPLAY_FRAMEBUFFER ? 1.f / vcm_iterations(r[0]) : 1.f, &disp.p)) return die("vcm_display");
            if (vcm_get_display_stats(r[0], &ds)) return die("vcm_get_display_stats");
            displayed = true;
            if (bmp) {
                px.resize((size_t)resX * resY * 3);
                if (vcm_read_display_image(r[0], VCM_IMAGE_BGR8, px.data())) return die("vcm_read_display_image");
                if (display_write_bmp(path.c_str(), resX, resY, px.data())) { fprintf(stderr, "vcm_render: cannot write %s\n", path.c_str()); return 2; }
                return 0;
            }
        }
        if (bmp || hdr) {
            px.resize((size_t)resX * resY * (bmp ? 3 : 4));
            if (denoised) {
                if (vcm_read_denoised_image(r[0], bmp ? VCM_IMAGE_BGR8 : VCM_IMAGE_RGBE, 2.2f, px.data())) return die("vcm_read_denoised_image");
            } else if (renderers == 1 && !r.empty() && !robust) {   // encoded on the device
                if (vcm_read_image(r[0], bmp ? VCM_IMAGE_BGR8 : VCM_IMAGE_RGBE, 1.f / vcm_iterations(r[0]), 2.2f, px.data()))
                    return die("vcm_read_image");
            } else if (bmp) {       // Framebuffer::SaveBMP, framebuffer.hxx:194-214
                const float invGamma = 1.f / 2.2f;
                for (int y = 0; y < resY; y++) for (int x = 0; x < resX; x++) {
                    const float *c = &img[((size_t)x + (size_t)(resY - y - 1) * resX) * 3];
                    unsigned char *o = &px[((size_t)y * resX + x) * 3];
                    for (int k = 0; k < 3; k++)
                        o[k] = (unsigned char)std::min(255.f, std::max(0.f, std::pow(c[2 - k], invGamma) * 255.f));
                }
            } else {                // Framebuffer::SaveHDR, framebuffer.hxx:229-247
                for (size_t p = 0; p < (size_t)resX * resY; p++) {
                    const float *c = &img[p * 3];
                    unsigned char *o = &px[p * 4];
                    o[0] = o[1] = o[2] = o[3] = 0;
                    float v = std::max(c[0], std::max(c[1], c[2]));
                    if (v >= 1e-32f) {
                        int e;
                        v = float(frexp(v, &e) * 256.f / v);
                        o[0] = (unsigned char)(c[0] * v); o[1] = (unsigned char)(c[1] * v); o[2] = (unsigned char)(c[2] * v);
                        o[3] = (unsigned char)(e + 128);
                    }
                }
            }
        }
        FILE *f = fopen(path.c_str(), "wb");
        if (!f) { fprintf(stderr, "vcm_render: cannot write %s\n", path.c_str()); return 2; }
        if (bmp) {   // BmpHeader, framebuffer.hxx:150-168, :175-191
            const uint32_t bytes = (uint32_t)resX * resY * 3;
            uint32_t h[13] = { 54u + bytes, 0u, 54u, 40u, (uint32_t)resX, (uint32_t)resY, 1u | (24u << 16), 0u, bytes, 2953u, 2953u, 0u, 0u };
            fwrite("BM", 1, 2, f);
            fwrite(h, 4, 13, f);
            fwrite(px.data(), 1, px.size(), f);
        } else if (hdr) {
            fprintf(f, "#?RADIANCE\n# SmallVCM\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n", resY, resX);
            fwrite(px.data(), 1, px.size(), f);
        } else {     // Framebuffer::SavePFM, framebuffer.hxx:137-146
            fprintf(f, "PF\n%d %d\n-1\n", resX, resY);
            fwrite(img.data(), sizeof(float), n3, f);
        }
        fclose(f);
        return 0;
    };
    if (!out.empty()) {
        if (!denoise) { if (int rc = save(out, fb, false)) return rc; }
        else {   // the denoised image under the name asked for, the noisy one beside it
            const size_t dot = out.rfind('.');
            const bool hasExt = dot != std::string::npos && out.find('/', dot) == std::string::npos;
            const std::string noisy = hasExt ? out.substr(0, dot) + ".noisy" + out.substr(dot) : out + ".noisy";
            if (int rc = save(noisy, fb, false)) return rc;
            if (int rc = save(out, clean, true)) return rc;
        }
    }
    if (disp.any && !displayed) {   // no -o: the statistics alone
        const int source = denoise ? VCM_DISPLAY_DENOISED : (robust ? VCM_DISPLAY_ROBUST : VCM_DISPLAY_FRAMEBUFFER);
        if (vcm_display(r[0], source, source == VCM_DISPLAY_FRAMEBUFFER ? 1.f / vcm_iterations(r[0]) : 1.f, &disp.p)) return die("vcm_display");
        if (vcm_get_display_stats(r[0], &ds)) return die("vcm_get_display_stats");
    }
    if (disp.any && !json)
        printf("display transform: exposure x %.9g (auto %+.4f EV over %lld pixel(s); %lld black, %lld non-finite left out), %lld channel(s) clipped\n",
               ds.multiplier, ds.autoEV, ds.counted, ds.zero, ds.nonFinite, ds.clipped);
    for (size_t g = 0; g < r.size(); g++) vcm_destroy(r[g]);
    vcm_scene_file_free(loaded);
    vcm_envmap_free(envmap);
    double mean[3] = { 0, 0, 0 };
    for (size_t i = 0; i < n3; i++) mean[i % 3] += fb[i];
    const double paths = (algorithm == VCM_ALGO_PATH_TRACE || algorithm == VCM_ALGO_EYE_LIGHT ? 1.0 : 2.0) * resX * resY * iterations;
    if (json) {
        char robustJson[320] = "";
        if (robust) snprintf(robustJson, sizeof(robustJson), ", \"robust\": {\"iterations\": %d, \"buckets\": %d, \"pixels\": %lld, \"trimmed\": %lld, "
                             "\"nonFinite\": %lld, \"meanGini\": %.17g, \"maxGini\": %.17g}", rs.iterations, rs.buckets, rs.pixels, rs.trimmed, rs.nonFinite,
                             rs.meanGini, rs.maxGini);
        char partsJson[480] = "";
        if (!partsOut.empty()) snprintf(partsJson, sizeof(partsJson), ", \"parts\": {\"iterations\": %d, \"pixels\": %lld, \"nonFinite\": %lld, \"luminance\": "
                                        "{\"emission\": %.17g, \"direct\": %.17g, \"connect\": %.17g, \"merge\": %.17g, \"lighttrace\": %.17g}}",
                                        ps.iterations, ps.pixels, ps.nonFinite, ps.luminance[0], ps.luminance[1], ps.luminance[2], ps.luminance[3], ps.luminance[4]);
        char displayJson[880] = "";
        if (disp.any) display_stats_json(ds, displayJson, 480);
        if (!refFile.empty()) {   // (a NaN or an infinity is no JSON number: null)
            auto num = [](double v) { char b[40]; if (std::isfinite(v)) snprintf(b, sizeof(b), "%.17g", v); else snprintf(b, sizeof(b), "null"); return std::string(b); };
            const size_t at = strlen(displayJson);
            snprintf(displayJson + at, sizeof(displayJson) - at, ", \"compare\": {\"iterations\": %d, \"pixels\": %lld, \"nonFinite\": %lld, \"above\": %lld, "
                     "\"ssimWindows\": %lld, \"maxPixel\": %lld, \"mse\": %s, \"relMse\": %s, \"mae\": %s, \"maxAbs\": %s, \"psnr\": %s, \"ssim\": %s}",
                     cs.iterations, cs.pixels, cs.nonFinite, cs.above, cs.ssimWindows, cs.maxPixel, num(cs.mse).c_str(), num(cs.relMse).c_str(),
                     num(cs.mae).c_str(), num(cs.maxAbs).c_str(), num(cs.psnr).c_str(), num(cs.ssim).c_str());
        }
        std::string ms = "[";
        for (size_t i = 0; i < rankMs.size(); i++) { char b[32]; snprintf(b, sizeof(b), "%s%.3f", i ? ", " : "", rankMs[i]); ms += b; }
        ms += "]";
        printf("{\"scene\": %d, \"algorithm\": \"%s\", \"res\": [%d, %d], \"iterations\": %d, \"renderers\": %d, \"seed\": %d, "
               "\"gpus\": %d, \"rccl_ranks\": %d, \"wall_s\": %.6f, \"Mpaths_s\": %.3f, \"image_mean\": [%.6f, %.6f, %.6f], "
               "\"last_iteration_ms\": %.3f, \"rank_iteration_ms\": %s, \"library\": \"%s\", "
               "\"last_iteration_kernel_ms\": {\"light\": %.3f, \"camera\": %.3f, \"connect_di\": %.3f, \"merge\": %.3f, \"grid_side\": %.3f, \"light_phase\": %.3f, \"camera_phase\": %.3f}, "
               "\"last_iteration_counters\": {\"lightVertices\": %lld, \"lightRays\": %lld, \"cameraRays\": %lld, \"shadowRays\": %lld, "
               "\"mergeQueries\": %lld, \"mergeCandidates\": %lld, \"mergeAccepted\": %lld, \"connections\": %lld, \"lightSplats\": %lld}%s%s%s}\n",
               sceneID, algoName.c_str(), resX, resY, iterations, renderers, seed, gpus > 0 ? gpus : 1, rcclRanks, wall, paths / wall / 1e6,
               mean[0] / (n3 / 3), mean[1] / (n3 / 3), mean[2] / (n3 / 3), st.msTotal, ms.c_str(), vcm_build_tag(),
               st.msLightKernel, st.msCameraKernel, st.msConnectKernels, st.msMergeKernel, st.msGrid, st.msLight, st.msCamera,
               st.lightVertices, st.lightRays, st.cameraRays, st.shadowRays, st.mergeQueries, st.mergeCandidates, st.mergeAccepted,
               st.connections, st.lightSplats, robustJson, partsJson, displayJson);
    }
    else
        printf("scene %d, %s, %dx%d, %d iteration(s) on %d renderer(s): %.3f s wall clock, %.2f Mpaths/s\n", sceneID,
               algoName.c_str(), resX, resY, iterations, renderers, wall, paths / wall / 1e6);
    return 0;
}
