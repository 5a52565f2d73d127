/*
 * smallvcm_amd_debug.h -- parity / test entry points of libsmallvcm_amd.so.
 *
 * NOT part of the drop-in boundary (that is include/smallvcm_amd.h): nothing a renderer host needs is here.
 * These symbols let tests/ read the intermediate state the reference keeps in VertexCM::mLightVertices and
 * HashGrid (src/vertexcm.hxx:1021-1028, src/hashgrid.hxx:205-214), evaluate the numeric specification
 * (detmath, Philox) on the device and on the host, and check the POD sizes the ctypes
 * mirror assumes.  tests/test_abi.py requires every exported vcm_* symbol to be declared in one of the two
 * headers, and every declared symbol to be exported.
 */
#ifndef SMALLVCM_AMD_DEBUG_H
#define SMALLVCM_AMD_DEBUG_H

#include "smallvcm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Hash grid of the last iteration (HashGrid::mCellEnds / mIndices, hashgrid.hxx:205-214):
 * cellStart (nCells+1 ints, cellStart[c+1] == mCellEnds[c]), sortedIndex (grid position -> record index =
 * mIndices, nRecords ints), bbox (mBBoxMin, mBBoxMax: 6 floats).  Any pointer may be NULL. */
int vcm_debug_read_grid(vcm_ctx *ctx, int *cellStart, int *sortedIndex, float *bbox6, long long *nRecords);

/* The local merge records of the last iteration (VCM_MERGE_RECORD_FLOATS floats each, reference vertex order),
 * host copy; `count` from vcm_light_records. */
int vcm_debug_read_records(vcm_ctx *ctx, float *out, long long count);

/* Element-wise evaluation ON THE DEVICE of the numeric specification: op 0 sinf(a), 1 cosf(a), 2 powf(a,b)
 * (detmath.h), 3 a/b, 4 sqrtf(a) (correctly rounded), 5 a*b+a as separate mul and add (no contraction). */
int vcm_debug_numeric_spec(int op, int n, const float *a, const float *b, float *out);
/* nFloats consecutive floats of nPaths paths of the counter-based stream (philox.h), on the device */
int vcm_debug_philox_spec(unsigned seed, unsigned iter, unsigned kind, int nPaths, int nFloats, float *out);

/* The same definitions evaluated on the host (the radius schedule uses powf on the host, vertexcm.hxx:296) */
float vcm_host_sinf(float x);
float vcm_host_cosf(float x);
float vcm_host_powf(float x, float y);
float vcm_host_path_float(unsigned seed, unsigned iter, unsigned path, unsigned kind, unsigned k);

/* Function-level known answers (T0): record i = VCM_KAT_FLOATS input floats -> VCM_KAT_FLOATS output floats of ONE
 * call of a device function, evaluated on the device with the context's scene (smallvcm_amd/csrc/vcm_kat.h has the
 * field layout per op; unused fields are 0).  oracle/ref_driver.cpp answers the same records with the reference's
 * classes (ref_kat), tests/host_emul with the device functions compiled for the host. */
#define VCM_KAT_FLOATS 16
enum {
    VCM_KAT_INTERSECT = 0,        /* in: org, dir, tmin -> hit, dist, matID, lightID, normal                 scene.hxx:53-70 */
    VCM_KAT_OCCLUDED = 1,         /* in: point, dir, tmax -> occluded                                        scene.hxx:72-85 */
    VCM_KAT_BSDF_EVAL = 2,        /* in: rayDir, normal, matID, dirGen -> valid, isDelta, contProb, f, cosGen, dirPdf,
                                     revPdf, Pdf(dir), Pdf(rev), WorldDirFix, CosThetaFix                    bsdf.hxx:95-180 */
    VCM_KAT_BSDF_SAMPLE = 3,      /* in: rayDir, normal, matID, rnd3, fixIsLight -> valid, f, dirGen, pdfW, cosGen, event
                                                                                                             bsdf.hxx:191-257 */
    VCM_KAT_LIGHT_EMIT = 4,       /* in: light, dirRnd2, posRnd2 -> energy, position, direction, emissionPdfW, directPdfA,
                                     cosLight, IsFinite, IsDelta                                             lights.hxx */
    VCM_KAT_LIGHT_ILLUMINATE = 5, /* in: light, receiver, rnd2 -> radiance, dirToLight, distance, directPdfW, emissionPdfW,
                                     cosAtLight */
    VCM_KAT_LIGHT_RADIANCE = 6,   /* in: light, rayDir, hitPoint -> radiance, directPdfA, emissionPdfW */
    VCM_KAT_CAMERA = 7,           /* in: raster x, y, world point -> ray dir, raster of the point, CheckRaster
                                                                                                             camera.hxx:95-117 */
    VCM_KAT_LENS = 8,             /* in: raster x, y, lens sample u1, u2, world point -> ray origin, ray dir, cameraPdfW, raster
                                     of the world point through that lens point, valid (1: in front of the lens); needs a
                                     context with a thin lens (vcm_create4)                       DESIGN.md "Thin lens" */
    VCM_KAT_LIGHT_PICK = 9,       /* in: the pick's random float -> light index, its pmf; in[1] = a light index -> out[2] = the
                                     pmf the emitter-hit sites use for it (pick_light / light_pick_prob)
                                                                                                  DESIGN.md "Light selection" */
    VCM_KAT_FILTER = 10,          /* in: raster x, y of a projection, then the 8 floats of a filter draw -> offset x, y, the pixel the
                                     splat goes to (-1: outside the image), and the moved point (x, y) + offset, added in the
                                     record itself, for reading the pixel; needs a context with a pixel filter (vcm_create6)
                                                                                                  DESIGN.md "Pixel filter" */
    VCM_KAT_LIGHT_RADIANCE_AT = 11, /* in: light, rayDir, the normal at the hit -> radiance, directPdfA, emissionPdfW: the emitter
                                     hit as the render path asks it (a sphere light needs the normal; every other type
                                     answers as VCM_KAT_LIGHT_RADIANCE does); needs a context with a spot or a sphere light
                                                                                     DESIGN.md "Spot and sphere lights" */
    VCM_KAT_SAMPLER = 12,         /* in: the BIT PATTERNS of the integers seed, sample index i, path, kind, position k in floats 0..4
                                     (memcpy, not values: i and seed need 32 bits) -> out[0] = float k of the Sobol sampler for that
                                     stream and index, out[1] = the bit pattern of its 32-bit word.  The op names the
                                     sampler's function (csrc/sobol.h sobol_word), not the context's mode: any context answers
                                                                                                  DESIGN.md "Sampler" */
    VCM_KAT_PROJECTION = 13,      /* in: raster x, y, world point -> ray dir, cameraPdfW, valid (0: outside the fisheye's image circle
                                     or the panorama's rows), then the raster x, y of the world point, valid (1: inside the
                                     field of view and the image) and the cameraPdfW of that direction; needs a context with a
                                     fisheye or panorama projection (vcm_create9)              DESIGN.md "Camera projections" */
    VCM_KAT_OPS = 14
};
int vcm_debug_kat(vcm_ctx *ctx, int op, int n, const float *in, float *out);

/* Which code path a context takes, for tests that must assert it rather than infer it: out = VCM_INFO_COUNT ints.
 * The kind flags are read off the one kind the context's launches use (csrc/scene_kind.h) -- rects / quads: the SceneRects(E) / SceneQuads kernels (both 0 on a
 * list: SceneList(E)); nodes: a BVH (SceneBvh / SceneBvhG / SceneBvhE); intPhong 0: the general-pow kinds; envMap, lens,
 * pick: the E kinds, WithLens, WithPick -- then the table sizes the LDS-or-global branches compare, and the merge kernel
 * the LAST iteration launched (VCM_MERGE_WALK or VCM_MERGE_PAIRS after the fall-back above VCM_PAIR_MATERIALS; 0: it
 * launched neither -- an algorithm without merging, or strict order, whose camera kernel merges in place). */
enum {
    VCM_INFO_RECTS = 0, VCM_INFO_QUADS = 1, VCM_INFO_NODES = 2, VCM_INFO_INT_PHONG = 3, VCM_INFO_ENVMAP = 4, VCM_INFO_LENS = 5,
    VCM_INFO_PICK = 6, VCM_INFO_MATERIALS = 7, VCM_INFO_PRIMS = 8, VCM_INFO_LIGHTS = 9, VCM_INFO_MERGE_KERNEL = 10,
    VCM_INFO_COUNT = 11
};
int vcm_debug_context_info(vcm_ctx *ctx, int *out);

/* 1: the context launches the WithLights kinds (its scene holds a spot or a sphere light; VCM_INFO_PICK is then 1 too,
 * whatever the caller asked for); 0: it launches exactly the kernels it launched before there were such lights. */
int vcm_debug_lights_kind(vcm_ctx *ctx);

/* The pixel filter of a context as its kernels see it (vcm_pixel_filter; kind VCM_FILTER_BOX: none, the context launches
 * exactly the kernels of vcm_create5).  A filter without a lens launches the WithLens kinds, so VCM_INFO_LENS -- which
 * stays "the scene has a thin lens" -- does not tell; this does.  Either pointer may be NULL. */
int vcm_debug_pixel_filter(vcm_ctx *ctx, int *kind, float *radius);

/* The sampler of a context as its kernels see it (vcm_sampler; VCM_SAMPLER_PHILOX: the context launches exactly the
 * kernels of vcm_create6, VCM_SAMPLER_SOBOL: the WithSobol kinds). */
int vcm_debug_sampler(vcm_ctx *ctx, int *kind);

/* Whether a context launches the WithGgx kinds (1: some material has a GGX lobe; 0: it launches exactly the kernels of
 * vcm_create7), and in *nLobes, if not NULL, how many materials have one. */
int vcm_debug_ggx(vcm_ctx *ctx, int *nLobes);

/* The projection of a context as its kernels see it (vcm_camera_model): *kind = VCM_PROJ_*, *fovDegrees = the fisheye's
 * field of view (0 otherwise); either pointer may be NULL.  Returns 1 when the context launches the WithLens kinds
 * because of its projection, 0 for PERSPECTIVE: it then launches exactly the kernels of vcm_create8.  (This is the
 * VCM_INFO_PROJECTION read-back; it is a function of its own because callers size vcm_debug_context_info's array by the
 * VCM_INFO_COUNT they were built with.) */
#define VCM_INFO_PROJECTION(ctx, kind, fov) vcm_debug_projection((ctx), (kind), (fov))
int vcm_debug_projection(vcm_ctx *ctx, int *kind, float *fovDegrees);

/* The rule that picks a context's kind from the five facts about its scene (csrc/scene_kind.h, scene_kind_of), for a
 * test of the rule itself: 0 SceneList, 1 SceneQuads, 2 SceneRects, 3 SceneBvh, 4 SceneBvhG, 5 SceneRectsE, 6 SceneListE,
 * 7 SceneBvhE.  A pure host function: it touches no device. */
int vcm_debug_scene_kind(int envMap, int bvh, int intPhong, int rects, int quads);

/* The two images of a context with vcm_track_variance on, as they stand after the last iteration: W*H float4 each,
 * prev = { S_{k-1}.rgb, 0 } and mom = { M2.rgb, 0 } (either may be NULL).  Synchronises. */
int vcm_debug_read_variance_images(vcm_ctx *ctx, float *prevHost4, float *momHost4);

/* The cap of the grid of k_var_update and k_var_stats (0 restores the default, 2048 workgroups of 256 lanes), so that a
 * test reaches the grid-stride path and the second reduction level with a few hundred pixels.  Process-wide; the
 * combination tree, and so the last bits of vcm_noise_stats.mean, depend on it: not for production hosts. */
void vcm_debug_variance_max_blocks(int blocks);

/* The images of a context with vcm_track_robust on, as they stand after the last iteration: prev = { S_{k-1}.rgb, 0 }, W*H
 * float4, and the M bucket planes, M*W*H float4 (either may be NULL).  Synchronises.  The grid of the robust kernels is
 * that of the variance kernels: vcm_debug_variance_max_blocks caps both. */
int vcm_debug_read_robust_images(vcm_ctx *ctx, float *prevHost4, float *bucketsHost4);

/* The cap of the grids of k_resolve_parts, k_parts_stats and the part reads of a context with vcm_track_parts on (0
 * restores the default, 2048 workgroups of 256 lanes), so that a test reaches the grid-stride paths and the second
 * reduction level with a few hundred pixels.  Process-wide; the combination tree, and so the last bits of
 * vcm_parts_stats.luminance, depend on it: not for production hosts. */
void vcm_debug_parts_max_blocks(int blocks);

/* The cap of the grid of the display transform's histogram kernel (0 restores the default, 2048 workgroups of 256 lanes),
 * so that a test reaches the grid-stride path with a few hundred pixels.  Process-wide; the counts do not depend on it. */
void vcm_debug_display_max_blocks(int blocks);

/* The 256 bins of the last histogram this thread's vcm_display / vcm_display_buffers read back (autoExposure == 1); -1
 * where there has been none. */
int vcm_debug_read_display_histogram(unsigned long long *out256);

/* The cap of the grid of the comparison's pixel kernel (0 restores the default, 2048 workgroups of 256 lanes), so that a
 * test reaches the grid-stride path with a few hundred pixels.  Process-wide; the combination tree, and so the last bits
 * of the sums of vcm_compare_stats, depend on it: not for production hosts. */
void vcm_debug_compare_max_blocks(int blocks);

/* sizeof the PODs of smallvcm_amd.h as the library was compiled */
unsigned vcm_sizeof_scene_desc(void);
unsigned vcm_sizeof_stats(void);

#ifdef __cplusplus
}
#endif
#endif /* SMALLVCM_AMD_DEBUG_H */
