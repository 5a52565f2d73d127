/*
 * smallvcm_amd.h -- C-ABI of the MI355X-native VCM integrator.
 *
 * This is the drop-in boundary for SmallVCM's `VertexCM::RunIteration`
 * (reference: src/vertexcm.hxx:284-548) behind `AbstractRenderer`
 * (src/renderer.hxx:33-70).  Everything crossing it is plain C: POD structs,
 * pointers and sizes.  The C++ shim `smallvcm_amd/dropin/vertexcm.hxx` binds
 * these entry points under the reference's own class name/ctor so that
 * `smallvcm.cxx` and `config.hxx` compile unchanged.
 *
 * Conventions
 *   - all entry points returning int return 0 on success, non-zero on error;
 *     `vcm_last_error()` then holds a message (thread-local).
 *   - "paths" are indexed 0..N-1, N = resX*resY, light path p and camera
 *     path (pixel) p share the index (vertexcm.hxx:321, :415, :504-506).
 *   - random numbers: counter-based Philox4x32-10 keyed by
 *     (seed, renderer-local iteration count), counter (path, kind, block);
 *     replaces src/rng.hxx (see DESIGN.md "RNG").
 */
#ifndef SMALLVCM_AMD_H
#define SMALLVCM_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define VCM_MAX_PRIMS      32
#define VCM_MAX_MATERIALS  16
#define VCM_MAX_LIGHTS      8

/* ---- scene description: POD flattening of the public members of `Scene`
 *      (src/scene.hxx:476-485) ------------------------------------------- */

enum { VCM_PRIM_TRIANGLE = 0, VCM_PRIM_SPHERE = 1 };

/* Triangle {p[3], matID, mNormal} (src/geometry.hxx:174-176) or
 * Sphere {center, radius, matID} (src/geometry.hxx:263-265: p0 = center,
 * p1[0] = radius).  Primitives keep the order of GeometryList::mGeometry
 * (src/geometry.hxx:104); closest-hit ties resolve to the first one. */
typedef struct vcm_prim {
    int   type;
    int   matID;
    float p0[3];
    float p1[3];
    float p2[3];
    float n[3];
} vcm_prim;

/* Material (src/materials.hxx:54-65) */
typedef struct vcm_material {
    float diffuse[3];
    float phong[3];
    float phongExp;
    float mirror[3];
    float ior;
} vcm_material;

enum {
    VCM_LIGHT_AREA = 0,        /* src/lights.hxx:112 */
    VCM_LIGHT_DIRECTIONAL = 1, /* src/lights.hxx:236 */
    VCM_LIGHT_POINT = 2,       /* src/lights.hxx:320 */
    VCM_LIGHT_BACKGROUND = 3,  /* src/lights.hxx:401 */
    VCM_LIGHT_ENVMAP = 4,      /* an image around the scene (vcm_scene_desc3; DESIGN.md "Environment map") */
    VCM_LIGHT_SPOT = 5,        /* a point light with a cone (DESIGN.md "Spot and sphere lights") */
    VCM_LIGHT_SPHERE = 6       /* an emissive sphere primitive (same section) */
};

/* Tagged union of the public light fields (src/lights.hxx:229-232, 314-315,
 * 395-396, 512-513).
 *   area:        p0,e1,e2, frame (mX,mY,mZ), intensity, invArea
 *   directional: frame, intensity
 *   point:       p0 = mPosition, intensity
 *   background:  intensity = mBackgroundColor, scale = mScale
 *   envmap:      scale (the radiance is texel * scale; the image comes with vcm_scene_desc3)
 *   spot:        p0 = position, frame (mZ = the axis, built as the directional light's), intensity = radiant intensity on
 *                the axis, e1 = { cos(outer half-angle), cos(inner half-angle), 1 / (cosInner - cosOuter) or 0 for a hard
 *                edge }, scale = the cone's pdf 1 / (2 pi (1 - cosOuter)).  Falloff for c = dot(axis, direction from the
 *                light): 0 for c < cosOuter, else t^2 (3 - 2 t) with t = clamp((c - cosOuter) e1[2], 0, 1); 1 inside a
 *                hard-edged cone
 *   sphere:      p0 = centre, e1[0] = radius, intensity = emitted radiance (outward only), invArea = 1 / (4 pi r^2).  It
 *                belongs to ONE sphere primitive of the same centre and radius, whose material maps to it (mat2light) */
typedef struct vcm_light {
    int   type;
    float p0[3];
    float e1[3];
    float e2[3];
    float frameX[3];
    float frameY[3];
    float frameZ[3];
    float intensity[3];
    float invArea;
    float scale;
} vcm_light;

/* Camera (src/camera.hxx:121-126).  Matrices are the 16 floats of Mat4f in
 * its memory order (column-major, src/math.hxx:255-259). */
typedef struct vcm_camera {
    float position[3];
    float forward[3];
    float resolution[2];
    float rasterToWorld[16];
    float worldToRaster[16];
    float imagePlaneDist;
} vcm_camera;

typedef struct vcm_scene_desc {
    int          nPrims;
    vcm_prim     prims[VCM_MAX_PRIMS];
    int          nMaterials;
    vcm_material materials[VCM_MAX_MATERIALS];
    int          mat2light[VCM_MAX_MATERIALS]; /* Scene::mMaterial2Light, -1 = none */
    int          nLights;
    vcm_light    lights[VCM_MAX_LIGHTS];
    int          backgroundLight;              /* index into lights or -1 (Scene::mBackground) */
    float        sceneCenter[3];               /* SceneSphere (src/lights.hxx:32-40) */
    float        sceneRadius;
    float        invSceneRadiusSqr;
    vcm_camera   camera;
} vcm_scene_desc;

/* Scene description, version 2: the same members with POINTER + count for primitives, materials and lights, for
 * scenes beyond the reference's built-in Cornell boxes (which is all its CLI can load: config.hxx:146-151; "no
 * acceleration structure", README:208-209; Scene::Intersect is a loop over every primitive, scene.hxx:53-70).  A
 * scene with more than VCM_MAX_PRIMS primitives is traced through a BVH built at vcm_create2; the results are those of
 * the reference's list walk (closest hit, ties to the lower list index: geometry.hxx:65-78).  The arrays are copied:
 * they may be freed after the call.  mat2light has nMaterials entries (Scene::mMaterial2Light: an emissive triangle
 * needs a material of its own, as in scene.hxx:333-361); at most 2^24 materials. */
typedef struct vcm_scene_desc2 {
    int                 nPrims;
    const vcm_prim     *prims;
    int                 nMaterials;
    const vcm_material *materials;
    const int          *mat2light;
    int                 nLights;
    const vcm_light    *lights;
    int                 backgroundLight;
    float               sceneCenter[3];
    float               sceneRadius;
    float               invSceneRadiusSqr;
    vcm_camera          camera;
} vcm_scene_desc2;

/* An environment map: width x height linear RGB texels (3 floats each), row 0 = the TOP of the sky.  Equirectangular
 * with +z up (the reference scenes' up axis): theta = acos z from +z, phi = atan2(y, x) in [0, 2 pi), u = phi / 2 pi
 * (column), v = theta / pi (row); nearest texel, radiance = texel * the light's scale.  1 <= width <= 8192,
 * 1 <= height <= 4096; every texel finite and >= 0, not all black. */
typedef struct vcm_envmap {
    int          width, height;
    const float *rgb;             /* width * height * 3 floats */
} vcm_envmap;

/* Scene description, version 3: a version-2 scene whose background may be an image.  With `envmap` set, the scene
 * holds exactly one light of type VCM_LIGHT_ENVMAP (vcm_make_envmap_light) and it is the backgroundLight (no other
 * background light); with `envmap` NULL and no such light it is the version-2 scene.  The map is copied. */
typedef struct vcm_scene_desc3 {
    vcm_scene_desc2   base;
    const vcm_envmap *envmap;
} vcm_scene_desc3;

/* A thin lens in place of the pinhole (DESIGN.md "Thin lens"): a disc of radius apertureRadius (world units, >= 0)
 * centred at the camera position and perpendicular to its forward axis, focused on the plane at focusDistance (world
 * units, > 0) along forward.  Every raster sample keeps its pixel; its ray starts at a uniformly drawn lens point and
 * passes through the sample's point on the focus plane.  apertureRadius == 0 is the pinhole. */
typedef struct vcm_thin_lens {
    float apertureRadius;
    float focusDistance;
} vcm_thin_lens;

/* Scene description, version 4: a version-3 scene (environment map or not) seen through an optional thin lens.
 * `lens` NULL, or an apertureRadius of 0, renders exactly what vcm_create3 renders.  The lens is copied. */
typedef struct vcm_scene_desc4 {
    vcm_scene_desc3      base;
    const vcm_thin_lens *lens;
} vcm_scene_desc4;

/* How a light is chosen where a path samples one (DESIGN.md "Light selection").  UNIFORM: every light with probability
 * 1 / nLights, as the reference does.  POWER: in proportion to the flux the light emits (area: pi lum(intensity) area;
 * point: 4 pi lum; directional: pi R^2 lum; background: 4 pi^2 R^2 lum scale; environment map: pi R^2 x the integral of
 * lum(texel scale) over the sphere; spot: 2 pi lum ((1 - cosInner) + (cosInner - cosOuter) / 2); sphere: pi lum x 4 pi r^2;
 * lum = the reference's Luminance, R = the scene sphere's radius).  A scene with a spot or a sphere light always chooses
 * through a table: UNIFORM, or no vcm_light_pick at all, then means equal weights (DESIGN.md "Spot and sphere lights").  CUSTOM: in proportion
 * to `weights` (nLights floats, finite, >= 0, not all zero; a zero weight is accepted only for a light that emits
 * nothing).  uniformMix a in [0, 1] blends the normalised weights with the uniform choice over the lights of non-zero
 * weight: w_i <- (1 - a) w_i / sum w + a / n'.  The probabilities are whole multiples of 2^-23 that sum to 1, at least one
 * multiple for every light of non-zero weight, so a path's random float picks light i with exactly pmf[i]. */
enum {
    VCM_LIGHT_PICK_UNIFORM = 0,
    VCM_LIGHT_PICK_POWER = 1,
    VCM_LIGHT_PICK_CUSTOM = 2
};
typedef struct vcm_light_pick {
    int          mode;
    float        uniformMix;
    const float *weights;      /* nLights floats, CUSTOM only */
} vcm_light_pick;

/* Scene description, version 5: a version-4 scene and how its lights are chosen.  `pick` NULL, or mode UNIFORM, renders
 * exactly what vcm_create4 renders.  The weights are copied. */
typedef struct vcm_scene_desc5 {
    vcm_scene_desc4       base;
    const vcm_light_pick *pick;
} vcm_scene_desc5;

/* The pixel reconstruction filter (DESIGN.md "Pixel filter").  BOX: the reference's -- a camera path jitters inside its
 * pixel, a light vertex adds to the pixel its projection falls in.  TENT and BSPLINE: filter importance sampling on
 * both sides with a separable offset density g whose support is `radius` pixels (finite, 0 < radius <= 16) per axis:
 * a camera path keeps its pixel and sends its ray through its sample moved by o ~ g, a light vertex is splatted to the
 * pixel that holds its projection moved by o ~ g (dropped when that point is outside the image).  Every pixel is then
 * measured with h = box * g on both sides; no splat carries a weight.  TENT: o = radius (u1 - u2) per axis, the tent of
 * half-width radius (variance radius^2 / 6).  BSPLINE: o = radius (u1 + u2 + u3 + u4 - 2) / 2, the cubic B-spline on
 * (-radius, radius) (variance radius^2 / 12: close to a Gaussian of sigma = radius / sqrt(12), 0.577 pixels at radius
 * 2).  The first-hit guide images (vcm_render_features) stay unfiltered. */
enum {
    VCM_FILTER_BOX = 0,
    VCM_FILTER_TENT = 1,
    VCM_FILTER_BSPLINE = 2
};
typedef struct vcm_pixel_filter {
    int   kind;
    float radius;              /* pixels; ignored for BOX */
} vcm_pixel_filter;

/* Scene description, version 6: a version-5 scene and its pixel filter.  `filter` NULL, or kind BOX, renders exactly
 * what vcm_create5 renders.  The filter is copied. */
typedef struct vcm_scene_desc6 {
    vcm_scene_desc5         base;
    const vcm_pixel_filter *filter;
} vcm_scene_desc6;

/* The sampler: where a path's random floats come from.  PHILOX (the default): independent white noise, float k of the
 * counter-based stream (seed, local iteration, path, kind) -- the reference's Rng made random-access.  SOBOL: float k is
 * component k & 1 of pair k >> 1 of a padded two-dimensional Sobol sequence with hash-based Owen scrambling (Burley
 * 2020), indexed by the local iteration: the scrambles depend on (seed, path, kind, pair) only, so for every pair the
 * points of iterations a 2^m .. (a + 1) 2^m - 1 are a (0, m, 2)-net, and the draw groups of a path start on pair
 * boundaries (one position is skipped where needed; skipped positions count in vcm_get_rng_counts).  Lower error at
 * equal cost where the integrand is smooth in a few dimensions (anti-aliasing, area and sky lights, the first bounce,
 * depth of field); largest gain at power-of-two iteration counts.  DESIGN.md "Sampler". */
enum {
    VCM_SAMPLER_PHILOX = 0,
    VCM_SAMPLER_SOBOL = 1
};
typedef struct vcm_sampler {
    int kind;
} vcm_sampler;

/* Scene description, version 7: a version-6 scene and its sampler.  `sampler` NULL, or kind PHILOX, renders exactly
 * what vcm_create6 renders.  The sampler is copied. */
typedef struct vcm_scene_desc7 {
    vcm_scene_desc6    base;
    const vcm_sampler *sampler;
} vcm_scene_desc7;

/* The optional fifth BSDF component of a material: a GGX microfacet lobe (reflection only, non-delta, one-sided like the
 * Phong lobe; Schlick's Fresnel term over F0, the height-correlated Smith masking term, visible-normal sampling by the
 * spherical cap, Dupuy & Benyoub 2023).  `ggx` is F0, the reflectance at normal incidence, each channel in [0, 1];
 * `alpha` the GGX width in [0.01, 1] (alpha = roughness^2 of the usual artists' parameter).  ggx = {0, 0, 0}: the material
 * has no such lobe, and alpha is not looked at.  DESIGN.md "Microfacet materials". */
typedef struct vcm_material_ext {
    float ggx[3];
    float alpha;
} vcm_material_ext;

/* Scene description, version 8: a version-7 scene and one vcm_material_ext per material (nMaterials entries, copied).
 * `materialExt` NULL, or every ggx zero, renders exactly what vcm_create7 renders, with the kernels it launches.  A lobe
 * on a material that mat2light maps to a light is refused. */
typedef struct vcm_scene_desc8 {
    vcm_scene_desc7         base;
    const vcm_material_ext *materialExt;
} vcm_scene_desc8;

/* The camera's projection.  PERSPECTIVE (the default): the reference's pinhole behind a planar image, as described by
 * vcm_camera's matrices.  The two angular projections read only camera.position, camera.forward, camera.resolution
 * (W, H) and the raster axes the matrices imply: with f = forward, ex = the raster +x direction made orthogonal to f
 * and ey = +-(f x ex), the sign that points along raster +y (all three derived in binary64), a raster point (x, y) in
 * pixels looks along
 *   FISHEYE (equidistant; fovDegrees in (0, 360), measured across the image WIDTH): k = W / fov[rad] pixels per radian,
 *     q = (x - W/2, y - H/2), rho = |q|, theta = rho / k, dir = sin(theta) (q / rho . (ex, ey)) + cos(theta) f.  A
 *     sample with theta > fov / 2 lies outside the image circle and contributes exactly 0.
 *   PANORAMA (equirectangular, 360 x 180 degrees, no parameter, any W and H): lambda = 2 pi (x / W - 1/2), the azimuth
 *     from f towards ex, theta = pi y / H, the polar angle from -ey (row 0 is up):
 *     dir = sin(theta) (cos(lambda) f + sin(lambda) ex) - cos(theta) ey.
 * Densities are per raster area, so non-square images are correct.  A thin lens combines with PERSPECTIVE only; a
 * pixel filter combines with all three.  DESIGN.md "Camera projections". */
enum {
    VCM_PROJ_PERSPECTIVE = 0,
    VCM_PROJ_FISHEYE = 1,
    VCM_PROJ_PANORAMA = 2
};
typedef struct vcm_camera_model {
    int   kind;
    float fovDegrees;   /* FISHEYE only */
} vcm_camera_model;

/* Scene description, version 9: a version-8 scene and its camera model (copied).  `model` NULL, or kind PERSPECTIVE,
 * renders exactly what vcm_create8 renders, with the kernels it launches. */
typedef struct vcm_scene_desc9 {
    vcm_scene_desc8         base;
    const vcm_camera_model *model;
} vcm_scene_desc9;

/* VertexCM::AlgorithmType (src/vertexcm.hxx:182-204) -- same values */
enum {
    VCM_ALGO_LIGHT_TRACE = 0,
    VCM_ALGO_PPM = 1,
    VCM_ALGO_BPM = 2,
    VCM_ALGO_BPT = 3,
    VCM_ALGO_VCM = 4,
    /* the reference's two other renderers behind the same interface (AbstractRenderer, renderer.hxx:33-70;
       created at config.hxx:118-121).  radiusFactor / radiusAlpha are ignored. */
    VCM_ALGO_PATH_TRACE = 5,                   /* PathTracer  src/pathtracer.hxx:45-215 */
    VCM_ALGO_EYE_LIGHT = 6                     /* EyeLight    src/eyelight.hxx:46-77 */
};

/* Per-iteration workload counters (what SURVEY.md section 8(d) calls N_LV, C, A, K, S)
 * of the most recent iteration on this rank, plus kernel times in ms measured
 * with HIP events on the context's stream. */
typedef struct vcm_stats {
    long long lightVertices;   /* N_LV stored on this rank                    */
    long long gridVertices;    /* vertices in the hash grid (all ranks)       */
    long long lightRays;       /* Scene::Intersect calls, light pass          */
    long long cameraRays;      /* Scene::Intersect calls, camera pass         */
    long long shadowRays;      /* Scene::Occluded calls                       */
    long long mergeQueries;    /* HashGrid::Process calls                     */
    long long mergeCandidates; /* C: distance tests (hashgrid.hxx:162-165)    */
    long long mergeAccepted;   /* A: RangeQuery::Process calls                */
    long long connections;     /* K: ConnectVertices calls                    */
    long long lightSplats;     /* S: Framebuffer::AddColor from light paths   */
    float msLight, msGrid, msCamera, msTotal; /* phases: light(+compaction; the light splats run on a stream of their own
                                                 and end inside msCamera), grid build, camera(+resolve) */
    float msLightKernel, msCameraKernel;      /* k_light_trace / k_camera_trace alone        */
    float msMergeKernel;                      /* k_merge_lane (0 in strict-order mode)       */
    float msQuerySort;                        /* camera-vertex counting sort (0 in strict mode) */
    float msConnectKernels;                   /* k_connect_di (0 in strict mode); k_connect_vc runs on another stream and is
                                                 not in this span */
    float radius;              /* merge radius of the iteration               */
} vcm_stats;

typedef struct vcm_ctx vcm_ctx;

/* Record layout used to exchange light vertices between ranks (13 floats =
 * 52 bytes: the part of LightVertex that RangeQuery::Process reads,
 * src/vertexcm.hxx:130-169). */
#define VCM_MERGE_RECORD_FLOATS 13

int         vcm_device_count(void);
const char *vcm_last_error(void);
/* "default", or name and flags of a measurement build of the library (profiles/quick_ab.sh prints it per run) */
const char *vcm_build_tag(void);

/* Replaces `new VertexCM(scene, algo, radiusFactor, radiusAlpha, seed)`
 * (src/vertexcm.hxx:208-282, called from src/config.hxx:124-138).
 * Includes the PPM->BPM downgrade of :246-278.  Device resources are
 * allocated lazily at the first iteration (unused renderers exist:
 * src/renderer.hxx:58, src/smallvcm.cxx:66). */
vcm_ctx *vcm_create(const vcm_scene_desc *scene, int algorithm,
                    float radiusFactor, float radiusAlpha, int seed);
/* vcm_create puts the renderer on the calling thread's CURRENT HIP device (a host that hands over its own stream or
 * device buffers allocated them there).  A renderer-per-host-core host on a multi-GPU node -- the reference's render()
 * builds one renderer per host core, smallvcm.cxx:61-72 -- asks vcm_next_device() for the device of its next renderer
 * and passes it to vcm_create_sharded(..., device, 0, 1): round-robin over the visible devices, so that every GPU
 * renders whole iterations of its share of the renderers and the driver's own framebuffer average is the only reduce
 * (this is what the drop-in does, smallvcm_amd/dropin/gpu_renderer.hxx).  Environment SMALLVCM_AMD_DEVICES: "all"
 * (what vcm_next_device deals over by default), "current" or a list such as "0,2,5"; when it is set, vcm_create
 * follows it too. */
int vcm_next_device(void);

/* Same, for one rank of a sharded renderer: rank r of worldSize traces light
 * paths and pixels [r*N/W, (r+1)*N/W) on HIP device `device`. */
vcm_ctx *vcm_create_sharded(const vcm_scene_desc *scene, int algorithm,
                            float radiusFactor, float radiusAlpha, int seed,
                            int device, int rank, int worldSize);

/* The same for a version-2 scene description. */
vcm_ctx *vcm_create2(const vcm_scene_desc2 *scene, int algorithm,
                     float radiusFactor, float radiusAlpha, int seed);
vcm_ctx *vcm_create_sharded2(const vcm_scene_desc2 *scene, int algorithm,
                             float radiusFactor, float radiusAlpha, int seed,
                             int device, int rank, int worldSize);

/* The same for a version-3 scene description (environment map).  NULL with vcm_last_error() for a bad map (size,
 * non-finite or negative texels, zero total luminance) or a map without its light / a light without its map. */
vcm_ctx *vcm_create3(const vcm_scene_desc3 *scene, int algorithm,
                     float radiusFactor, float radiusAlpha, int seed);
vcm_ctx *vcm_create_sharded3(const vcm_scene_desc3 *scene, int algorithm,
                             float radiusFactor, float radiusAlpha, int seed,
                             int device, int rank, int worldSize);

/* The same for a version-4 scene description (thin lens).  NULL with vcm_last_error() for a bad lens (apertureRadius
 * negative or not finite; focusDistance <= 0 or not finite) or a bad version-3 scene. */
vcm_ctx *vcm_create4(const vcm_scene_desc4 *scene, int algorithm,
                     float radiusFactor, float radiusAlpha, int seed);
vcm_ctx *vcm_create_sharded4(const vcm_scene_desc4 *scene, int algorithm,
                             float radiusFactor, float radiusAlpha, int seed,
                             int device, int rank, int worldSize);

/* The same for a version-5 scene description (light selection).  NULL with vcm_last_error() for a bad mode, a
 * uniformMix outside [0, 1] or not finite, bad CUSTOM weights, more than 2^23 lights of non-zero weight, or a bad
 * version-4 scene. */
vcm_ctx *vcm_create5(const vcm_scene_desc5 *scene, int algorithm,
                     float radiusFactor, float radiusAlpha, int seed);
vcm_ctx *vcm_create_sharded5(const vcm_scene_desc5 *scene, int algorithm,
                             float radiusFactor, float radiusAlpha, int seed,
                             int device, int rank, int worldSize);

/* The same for a version-6 scene description (pixel filter).  NULL with vcm_last_error() for an unknown kind, a radius
 * that is not finite, <= 0 or > 16 (TENT, BSPLINE), or a bad version-5 scene; checked before a device is looked for. */
vcm_ctx *vcm_create6(const vcm_scene_desc6 *scene, int algorithm,
                     float radiusFactor, float radiusAlpha, int seed);
vcm_ctx *vcm_create_sharded6(const vcm_scene_desc6 *scene, int algorithm,
                             float radiusFactor, float radiusAlpha, int seed,
                             int device, int rank, int worldSize);

/* The same for a version-7 scene description (sampler).  NULL with vcm_last_error() for an unknown kind or a bad
 * version-6 scene; checked before a device is looked for. */
vcm_ctx *vcm_create7(const vcm_scene_desc7 *scene, int algorithm,
                     float radiusFactor, float radiusAlpha, int seed);
vcm_ctx *vcm_create_sharded7(const vcm_scene_desc7 *scene, int algorithm,
                             float radiusFactor, float radiusAlpha, int seed,
                             int device, int rank, int worldSize);

/* The same for a version-8 scene description (GGX lobes).  NULL with vcm_last_error() for a non-finite field, an F0
 * channel outside [0, 1], an alpha outside [0.01, 1] on a material with a lobe, a lobe on an emitting material, or a bad
 * version-7 scene; checked before a device is looked for. */
vcm_ctx *vcm_create8(const vcm_scene_desc8 *scene, int algorithm,
                     float radiusFactor, float radiusAlpha, int seed);
vcm_ctx *vcm_create_sharded8(const vcm_scene_desc8 *scene, int algorithm,
                             float radiusFactor, float radiusAlpha, int seed,
                             int device, int rank, int worldSize);

/* The same for a version-9 scene description (camera projection).  NULL with vcm_last_error() for an unknown kind, a
 * FISHEYE fovDegrees that is not finite or not in (0, 360), a thin lens together with a projection other than
 * PERSPECTIVE, or a bad version-8 scene; checked before a device is looked for. */
vcm_ctx *vcm_create9(const vcm_scene_desc9 *scene, int algorithm,
                     float radiusFactor, float radiusAlpha, int seed);
vcm_ctx *vcm_create_sharded9(const vcm_scene_desc9 *scene, int algorithm,
                             float radiusFactor, float radiusAlpha, int seed,
                             int device, int rank, int worldSize);

void vcm_destroy(vcm_ctx *ctx);

/* Execution mode.  0 (default, "wavefront"): the camera pass only traces and
 * scatters; direct illumination, vertex connections and merges are evaluated
 * by dense task kernels and every path's additions are replayed in the
 * reference's order, light splats included: bit-identical to the reference for
 * every algorithm.  1 ("strict"): everything is evaluated inside the paths as
 * the reference does (about 2x slower; light splats are fp32 atomics there).
 * The environment variable SMALLVCM_AMD_STRICT_ORDER=1 sets the default. */
int vcm_set_strict_order(vcm_ctx *ctx, int on);
/* 1 if an iteration with this maxPathLength will run in wavefront mode, 0 if it falls back to / was set to the
 * strict order (vcm_set_strict_order, or maxPathLength > 31: the per-path vertex masks are 32 bits).  A sharded
 * host asks this to know whether vcm_trace_camera may run before vcm_build_grid. */
int vcm_is_wavefront(vcm_ctx *ctx, unsigned maxPathLength);

/* The merge sharded by SPACE (round 6 prototype).  With the calls above every rank merges ITS pixels' camera
 * vertices against ALL ranks' light vertices (vertexcm.hxx:532-533): the grid and the merge do not shrink with the shard.  Here rank s
 * owns a SLAB of un-hashed grid cells along one axis -- cells [X[s], X[s+1]) -- and one cell of halo: it receives the light vertices of
 * cells [X[s] - 1, X[s+1]] only, builds HashGrid::Build's grid over those (vcm_import_light_records + vcm_build_grid: records arrive grouped by
 * source rank = in global index order, so the in-cell order is the reference's), receives the camera vertices whose base cell lies in its slab
 * from every rank, evaluates RangeQuery::Process for them and sends the 16-byte terms back to the pixels' owner.  A query's accepted photons
 * all lie in its own 2 x 2 x 2 block of cells (hashgrid.hxx:124-155), so its accepted sequence -- and the frame -- are the unsharded
 * renderer's; the candidate COUNT is not (a hash bucket no longer holds the far-away cells that collide into it).
 *   vcm_space_histogram          after vcm_trace_light: 256 bins of the local light vertices' coordinate along `axis` over the scene's
 *                                bounding sphere ([*lo, *lo + 256 * *binWidth)); the ranks sum them and pick S - 1 split coordinates
 *   vcm_space_set_slabs          after vcm_set_grid_bbox: splits[1 .. S-1] = the world coordinates where slab s begins (every rank
 *                                passes the same values)
 *   vcm_space_partition_light    the local light records (13 floats each) grouped by destination slab, index order inside a destination,
 *                                halo vertices once per destination: destination d at dstDev + d * strideRecords records; counts[d] to
 *                                the host (one stream synchronisation).  The host exchanges the groups all-to-all and hands what it received
 *                                to vcm_import_light_records (segment s = what rank s sent), then vcm_build_grid
 *   vcm_space_partition_queries  after vcm_trace_camera: the camera vertices (64-byte records) grouped by the slab of their base cell
 *   vcm_space_merge              after vcm_build_grid: queriesDev = nSeg segments (rank order) of counts[s] queries at a stride of
 *                                `stride` queries; sorts and merges them against this rank's grid; resultsDev gets the terms (16 bytes
 *                                each) in the same layout
 *   vcm_space_import_results     resultsDev = for every destination d the terms of the queries this rank sent to d (the layout
 *                                vcm_space_partition_queries wrote); vcm_merge then skips its own merge and resolves */
int vcm_space_histogram(vcm_ctx *ctx, int axis, float *lo, float *binWidth, int *hist256);
int vcm_space_set_slabs(vcm_ctx *ctx, int axis, const float *splits, int nSlabs);
int vcm_space_partition_light(vcm_ctx *ctx, void *dstDev, long long strideRecords, long long *counts);
int vcm_space_partition_queries(vcm_ctx *ctx, void *dstDev, long long strideQueries, long long *counts);
int vcm_space_merge(vcm_ctx *ctx, const void *queriesDev, const long long *counts, int nSeg, long long stride, void *resultsDev);
int vcm_space_import_results(vcm_ctx *ctx, const void *resultsDev, long long stride);

/* Which kernel evaluates the range merges (HashGrid::Process, hashgrid.hxx:110-169) in wavefront mode: both produce the
 * same bits, they differ in who evaluates an accepted photon (vcm_kernels.h; measured in DESIGN.md 5).
 * The environment variable SMALLVCM_AMD_MERGE=walk|pairs sets the default (pairs). */
#define VCM_MERGE_LANE   0   /* retired in round 6 (the 8 cells in lockstep): vcm_set_merge_kernel refuses it */
#define VCM_MERGE_STAGED 1   /* retired in round 6 (cell lists staged through LDS by a workgroup): refused */
#define VCM_MERGE_WALK   2   /* every lane walks its own non-empty runs back to back and evaluates its own accepted photons */
#define VCM_MERGE_PAIRS  3   /* the scan per lane as in WALK; the accepted (query, photon) pairs of a wave evaluated 64 at a time
                                by whichever lane gets them (scenes with more than 32 materials: WALK) */
int vcm_set_merge_kernel(vcm_ctx *ctx, int kind);

/* Use an externally owned HIP stream (e.g. torch's current stream) for all
 * work of this context; NULL = the context's own stream. */
int vcm_set_stream(vcm_ctx *ctx, void *hipStream);

/* Iteration scratch (light-vertex store, hash grid, camera-vertex queues: 1.5 GB at 512^2, 24 GB at 2048^2) is not
 * owned by a renderer: single-rank renderers of a device borrow it per iteration from a pool of arenas, so the
 * reference's one-renderer-per-host-core driver (smallvcm.cxx:66) fits in HBM and iterations of different renderers
 * overlap on the GPU.  maxArenas 1..8, 0 = as many as fit a quarter of the device memory (default; environment
 * SMALLVCM_AMD_ARENAS). */
int vcm_set_arena_limit(int device, int maxArenas);

/* Optional: allocate up front everything the first iteration with this maxPathLength would allocate lazily
 * (the context's buffers and the device's scratch arena), e.g. before a timed region. */
int vcm_reserve(vcm_ctx *ctx, unsigned maxPathLength);
/* Replaces VertexCM::RunIteration(aIteration) (src/vertexcm.hxx:284-548) for a
 * single-GPU renderer.  minLen/maxLen are AbstractRenderer::mMinPathLength /
 * mMaxPathLength, which the driver assigns after construction
 * (src/smallvcm.cxx:70-71).  Asynchronous on the context's stream. */
int vcm_run_iteration(vcm_ctx *ctx, int iteration, unsigned minLen, unsigned maxLen);

/* Phase-level entry points: vcm_run_iteration == begin, trace_light,
 * build_grid, trace_camera, merge, end.  A multi-GPU host puts the all-gather
 * of the light-vertex records between trace_light and build_grid; in the
 * default (wavefront) mode vcm_trace_camera does not need the grid, so it may
 * run BEFORE vcm_build_grid, overlapping the all-gather. */
/* A phase call that fails ENDS the iteration (HIP error or wrong call order alike): the iteration scratch goes
 * back to the device's arena and the next call must be vcm_begin_iteration. */
int vcm_begin_iteration(vcm_ctx *ctx, int iteration, unsigned minLen, unsigned maxLen); /* :288-316 */
int vcm_trace_light(vcm_ctx *ctx);   /* :321-396, then compaction into merge records */
int vcm_build_grid(vcm_ctx *ctx);    /* :403-408 -> hashgrid.hxx:41-107 */
int vcm_trace_camera(vcm_ctx *ctx);  /* :415-545 (wavefront mode: all but the merge :530-538) */
int vcm_merge(vcm_ctx *ctx);         /* :530-538 for every camera vertex, then AddColor :544 */
int vcm_end_iteration(vcm_ctx *ctx); /* :547 */

/* Local merge records of this rank after vcm_trace_light: device pointer to
 * count x VCM_MERGE_RECORD_FLOATS floats, in the reference's vertex order.
 * `count` is read back from the device (synchronises the stream). */
int vcm_light_records(vcm_ctx *ctx, void **devPtr, long long *count);

/* Sharded hosts: the bounding box (and number) of this rank's light vertices after vcm_trace_light -- empty:
 * min = +1e36, max = -1e36 (hashgrid.hxx:47-48) -- and, the other way, the box of ALL ranks' vertices (min / max of
 * the per-rank boxes), to be set before vcm_trace_camera / vcm_build_grid.  Exchanging 7 numbers per rank instead
 * of the count alone lets the camera pass prepare the query sort while the vertices are still in flight. */
int vcm_local_light_bbox(vcm_ctx *ctx, float *min3, float *max3, long long *count);
int vcm_set_grid_bbox(vcm_ctx *ctx, const float *min3, const float *max3);
/* Copy the local merge records (count from vcm_light_records) / the
 * framebuffer into caller-owned DEVICE memory (e.g. a torch tensor that is
 * then handed to an RCCL collective).  Asynchronous on the context's stream. */
int vcm_export_light_records(vcm_ctx *ctx, void *dstDev, long long count);
int vcm_export_framebuffer(vcm_ctx *ctx, void *dstDev);
/* the same multiplied by `scale` (1 / iterations gives GetFramebuffer, renderer.hxx:49-55): what a multi-GPU host
 * hands to the framebuffer all-reduce */
int vcm_export_framebuffer_scaled(vcm_ctx *ctx, void *dstDev, float scale);

/* Install the all-gathered records: nSeg segments (one per rank, rank order),
 * segment s holds counts[s] records starting at devPtr + s*strideRecords
 * records.  Repacks them contiguously; build_grid then uses them. */
int vcm_import_light_records(vcm_ctx *ctx, const void *devPtr,
                             const long long *counts, int nSeg,
                             long long strideRecords);

/* The SORTED exchange of a sharded renderer (round 5; replaces the three calls above on the hot path -- they stay for hosts
 * that want the records in the reference's order).  Path-index blocks are contiguous per rank, so a cell's vertices in
 * HashGrid::Build's stable order (hashgrid.hxx:83-88) are rank 0's in their local order, then rank 1's, ...: every rank
 * counting-sorts ONLY ITS OWN vertices by hash cell (1 / worldSize of the grid build), the ranks all-gather the sorted
 * slabs, and vcm_build_grid merges them cell block by cell block in one streaming pass -- no rank ever counts, scans or
 * ranks the other ranks' vertices (rounds 2-4: the whole build replicated on every rank).
 *   vcm_sorted_slab_words    4-byte words one rank's slab takes for `strideRecords` records: the records (13 words each,
 *                            cell order) + one block-start word per block of cells (+ padding to 16 bytes); -1 with
 *                            vcm_last_error() when the context cannot use the sorted exchange (not sharded, no merging
 *                            algorithm, more than 64 shards, 2^24 or more records in a shard): use the calls above.
 *   vcm_sort_light_records   after vcm_set_grid_bbox (the cell of a vertex depends on the box of ALL vertices): sorts the
 *                            local vertices and writes the slab to dstDev (device memory of the caller, e.g. the send
 *                            buffer of ncclAllGather).  Asynchronous on the context's stream.
 *   vcm_import_sorted_light_records   `gathered` = worldSize slabs of vcm_sorted_slab_words(strideRecords) words, rank
 *                            order, counts[s] = records of rank s; vcm_build_grid then merges them.  The memory must stay
 *                            valid until vcm_merge has been enqueued. */
long long vcm_sorted_slab_words(vcm_ctx *ctx, long long strideRecords);
int vcm_sort_light_records(vcm_ctx *ctx, void *dstDev, long long strideRecords);
int vcm_import_sorted_light_records(vcm_ctx *ctx, const void *gathered, const long long *counts, int nSeg,
                                    long long strideRecords);

/* The image in the reference's two 8-bit output encodings, converted on the device (a quarter / a third of
 * the bytes of the fp32 framebuffer cross PCIe).  The framebuffer (running sum) is scaled by `scale` first --
 * 1 / iterations gives what GetFramebuffer returns (renderer.hxx:49-55).
 *   VCM_IMAGE_BGR8  Framebuffer::SaveBMP's pixel data (framebuffer.hxx:194-214): rows bottom-up, B,G,R bytes,
 *                   byte(min(255, max(0, pow(c, 1/gamma) * 255))); resX*resY*3 bytes.  pow is the deterministic
 *                   powf of this library, so a byte can differ by one level from a glibc build of the reference.
 *   VCM_IMAGE_RGBE  Framebuffer::SaveHDR's pixel data (:229-247): rows top-down, R,G,B,E bytes; resX*resY*4
 *                   bytes, bit-identical to the reference's (frexp and IEEE double arithmetic only). */
enum { VCM_IMAGE_BGR8 = 0, VCM_IMAGE_RGBE = 1, VCM_IMAGE_RGBA8 = 2 /* vcm_read_display_image only */ };
int vcm_read_image(vcm_ctx *ctx, int format, float scale, float gamma, unsigned char *outHost);
/* Framebuffer = running SUM over iterations of this context (the reference's
 * mFramebuffer, src/renderer.hxx:68); W*H*3 floats, row-major, RGB. */
int vcm_read_framebuffer(vcm_ctx *ctx, float *rgbHost);
/* Page-lock / release caller-owned HOST memory (hipHostRegister / hipHostUnregister), so that vcm_read_framebuffer into it is
 * one DMA at link speed instead of a staged copy through the runtime's bounce buffers.  The drop-in registers the reference
 * Framebuffer's own pixel storage once (dropin/gpu_renderer.hxx) and refreshes it after every RunIteration
 * (src/renderer.hxx:49-55).  Both return 0 or -1 with vcm_last_error(); a host that cannot pin simply reads slower. */
int vcm_pin_host_memory(void *hostPtr, unsigned long long bytes);
int vcm_unpin_host_memory(void *hostPtr);
int vcm_framebuffer_device(vcm_ctx *ctx, void **devPtr);
int vcm_clear_framebuffer(vcm_ctx *ctx);

int vcm_iterations(vcm_ctx *ctx); /* AbstractRenderer::mIterations */
int vcm_synchronize(vcm_ctx *ctx);
int vcm_get_stats(vcm_ctx *ctx, vcm_stats *out);
/* The same for an earlier iteration: `ago` = 0 is the last completed one; the counters and the phase times
 * (stamped on the context's stream by every iteration) of the last 64 iterations are kept on the device, so a
 * host can run a batch of iterations without reading anything back in between and still get per-iteration
 * figures afterwards. */
int vcm_get_stats_at(vcm_ctx *ctx, int ago, vcm_stats *out);

/* Number of random floats each path consumed in the last iteration (local
 * paths of this rank): the "tape" that lets the unmodified reference replay
 * the same random numbers (oracle/ref_driver.cpp).  Host buffers of
 * localPathCount bytes each. */
int vcm_get_rng_counts(vcm_ctx *ctx, unsigned char *lightCounts, unsigned char *cameraCounts);
int vcm_local_path_range(vcm_ctx *ctx, int *first, int *count);

/* Host-side restatement of Scene::LoadCornellBox + BuildSceneSphere
 * (src/scene.hxx:132-398) and Camera::Setup (src/camera.hxx:37-76) for hosts
 * that do not link the reference's scene code (Python, bench). boxMask uses
 * Scene::BoxMask bits (src/scene.hxx:112-126). */
int vcm_scene_cornell(int resX, int resY, unsigned boxMask, vcm_scene_desc *out);
/* g_SceneConfigs[sceneID] (src/config.hxx:146-151) */
unsigned vcm_scene_config_mask(int sceneID);

/* Building a version-2 scene: one call per object, each computing the derived members the way the reference's
 * constructor does (same operations, same bits), so that a scene assembled here equals what the reference would hold
 * for the same input:
 *   vcm_make_triangle          Triangle::Triangle        geometry.hxx:111-123  (mNormal)
 *   vcm_make_sphere            Sphere::Sphere            geometry.hxx:184-192
 *   vcm_make_area_light        AreaLight::AreaLight      lights.hxx:116-127    (edges, frame, 1 / area)
 *   vcm_make_directional_light DirectionalLight          lights.hxx:239-243    (frame)
 *   vcm_make_point_light       PointLight                lights.hxx:324-328
 *   vcm_make_background_light  BackgroundLight           lights.hxx:404-408    (the reference's sky colour)
 *   vcm_make_spot_light        (no counterpart)          direction need not be normalised; half-angles in degrees,
 *                                                        0 < outerDeg <= 180, 0 <= innerDeg <= outerDeg
 *   vcm_make_sphere_light      (no counterpart)          goes with a vcm_make_sphere primitive of the same centre and radius
 *   vcm_make_material          Material::Reset           materials.hxx:44-51   (black, exponent 1, no refraction)
 *   vcm_make_camera            Camera::Setup             camera.hxx:37-76
 *   vcm_make_scene_sphere      Scene::BuildSceneSphere   scene.hxx:387-398
 * An emissive triangle is a primitive with a material of its own whose mat2light entry names the area light over the
 * same three points (scene.hxx:333-361). */
void vcm_make_triangle(const float *p0, const float *p1, const float *p2, int matID, vcm_prim *out);
void vcm_make_sphere(const float *center, float radius, int matID, vcm_prim *out);
void vcm_make_area_light(const float *p0, const float *p1, const float *p2, const float *intensity, vcm_light *out);
void vcm_make_directional_light(const float *direction, const float *intensity, vcm_light *out);
void vcm_make_point_light(const float *position, const float *intensity, vcm_light *out);
void vcm_make_background_light(float scale, vcm_light *out);
/* the light of a vcm_scene_desc3's environment map (radiance = texel * scale); it must be the scene's backgroundLight */
void vcm_make_envmap_light(float scale, vcm_light *out);
void vcm_make_spot_light(const float *position, const float *direction, const float *intensity, float outerDeg, float innerDeg,
                         vcm_light *out);
void vcm_make_sphere_light(const float *center, float radius, const float *intensity, vcm_light *out);
void vcm_make_material(vcm_material *out);
int  vcm_make_camera(const float *position, const float *forward, const float *up, float horizontalFovDeg, int resX, int resY,
                     vcm_camera *out);
void vcm_make_scene_sphere(const vcm_prim *prims, int nPrims, float *center3, float *radius, float *invRadiusSqr);

/* Scene files.  The reference has no loader ("Scenes are hard-coded", README:210; Scene::LoadCornellBox,
 * scene.hxx:132-398, is the only way a scene comes into being).  vcm_scene_load reads a `.vcmscene` text file --
 * directives processed in order: `obj <file>` (Wavefront OBJ triangles with their MTL library: Kd / Ks+Ns / illum /
 * Ni -> Material, Ke -> one AreaLight per triangle as in scene.hxx:333-361), `sphere`, `camera`, `light
 * point|directional|background|envmap`, `lens`, `lightpick`, `mtllib` -- or a bare `.obj` (default camera), and builds the version-2 description
 * with the vcm_make_* constructors above; smallvcm_amd/csrc/scene_file.cpp documents the format.  The description
 * points into the handle: keep it until the renderers are created (vcm_create2 copies).  NULL on failure, with the
 * reason in vcm_scene_load_error(). */
typedef struct vcm_scene_file vcm_scene_file;
vcm_scene_file *vcm_scene_load(const char *path, int resX, int resY);
const vcm_scene_desc2 *vcm_scene_file_desc(const vcm_scene_file *scene);
void vcm_scene_file_free(vcm_scene_file *scene);
const char *vcm_scene_load_error(void);
/* The scene as a version-3 description: envmap set when the file has a `light envmap <file> <scale>` directive, NULL
 * otherwise.  Points into the handle, like vcm_scene_file_desc. */
const vcm_scene_desc3 *vcm_scene_file_desc3(const vcm_scene_file *scene);
/* The scene as a version-4 description: lens set when the file has a `lens <apertureRadius> <focusDistance>`
 * directive, NULL otherwise; its base is vcm_scene_file_desc3's.  Points into the handle, like vcm_scene_file_desc. */
const vcm_scene_desc4 *vcm_scene_file_desc4(const vcm_scene_file *scene);
/* The scene as a version-5 description: pick set when the file has a `lightpick uniform|power [uniformMix]` directive,
 * NULL otherwise; its base is vcm_scene_file_desc4's.  Points into the handle, like vcm_scene_file_desc. */
const vcm_scene_desc5 *vcm_scene_file_desc5(const vcm_scene_file *scene);
/* The same scene as a version-6 description: `filter` set when the file has a `filter tent|bspline radius` directive,
 * NULL otherwise; its base is vcm_scene_file_desc5's.  Points into the handle, like vcm_scene_file_desc. */
const vcm_scene_desc6 *vcm_scene_file_desc6(const vcm_scene_file *scene);
/* The same scene as a version-7 description: its base is vcm_scene_file_desc6's, its sampler that of the file's
 * `sampler sobol|philox` directive, NULL without one.  Points into the handle, like vcm_scene_file_desc. */
const vcm_scene_desc7 *vcm_scene_file_desc7(const vcm_scene_file *scene);
/* The same scene as a version-8 description: its base is vcm_scene_file_desc7's, materialExt is set when a material in
 * use has a `Pr` line in its .mtl (Ks is then the F0 of a GGX lobe of alpha = max(Pr^2, 0.01)), NULL otherwise.  Points
 * into the handle, like vcm_scene_file_desc. */
const vcm_scene_desc8 *vcm_scene_file_desc8(const vcm_scene_file *scene);
/* The same scene as a version-9 description: its base is vcm_scene_file_desc8's, its model that of the file's
 * `projection fisheye <fovDeg>|panorama` directive, NULL without one.  Points into the handle, like vcm_scene_file_desc. */
const vcm_scene_desc9 *vcm_scene_file_desc9(const vcm_scene_file *scene);

/* Environment maps from files: Radiance RGBE (.hdr: "#?RADIANCE" / "#?RGBE", FORMAT=32-bit_rle_rgbe, "-Y H +X W", flat
 * or new-style run-length scanlines) or PFM (.pfm: "PF", either byte order; its bottom-up rows are flipped), picked by
 * the file's magic.  Rows come out top first, as vcm_envmap wants them.  NULL on failure, with the reason in
 * vcm_scene_load_error(); vcm_envmap_free releases the map and its texels. */
vcm_envmap *vcm_envmap_load(const char *path);
void vcm_envmap_free(vcm_envmap *map);

/* ---- first-hit feature buffers and the edge-avoiding denoiser ----
 * vcm_render_features casts one ray through the CENTRE of every pixel of the context's local path range -- from the
 * pinhole, also where the scene has a thin lens -- and keeps, per pixel,
 *   VCM_FEATURE_NORMAL  the hit's geometric normal as the closest-hit routine returns it; (0, 0, 0) on a miss
 *   VCM_FEATURE_DEPTH   the distance along the ray; 0 on a miss (no hit has distance 0)
 *   VCM_FEATURE_ALBEDO  clamp(diffuse + phong + mirror, 0, 1) of the hit's material; (1, 1, 1) where it refracts, on an
 *                       emitter and on a miss; a component that comes out 0 becomes 1
 * (mirror and glass chains are NOT followed to the first rough surface: what is seen in them is smoothed).  A sharded
 * context fills its own pixel range and leaves the rest of the frame 0.
 * vcm_denoise filters framebuffer * scale with the edge-avoiding a-trous wavelet of Dammertz et al. 2010: pass i of
 * `passes` applies the 5 x 5 B3-spline kernel with taps 2^i pixels apart, a tap's weight multiplied by
 *   max(0, n_p . n_q)^sigmaNormal,  f((|z_p - z_q| / (sigmaDepth max(z_p, z_q)))^2)  and  f(|c_p - c_q|^2 / sigmaColor_i^2),
 * f(x) = 1 / (1 + x / 4)^4, sigmaColor_i = sigmaColor / 2^i; misses match only misses; a non-finite tap counts 0, a
 * non-finite centre passes through.  demodulate: the input is divided by the albedo before the first pass and
 * multiplied back after the last.  passes = 0 copies the input; passes outside [0, 12] and sigmas that are not finite
 * and positive are refused.  It renders the features first if they are not there, and it leaves the framebuffer alone.
 * Memory: a context keeps, from its first vcm_render_features / vcm_denoise to vcm_destroy, two float4 feature images
 * and three float4 colour images (the two the passes ping-pong between and the result): 5 x 16 bytes per pixel, of
 * which the ping-pong pair is 128 MB at 2048^2.
 * vcm_denoise, vcm_read_denoised, vcm_denoised_device and vcm_read_denoised_image refuse a sharded context (its
 * framebuffer is a shard of the image): such a host gathers the features, reduces the frame and calls
 * vcm_denoise_buffers, which needs no context: float4 images on `device` (colour rgb?, albedo rgb1, guide
 * normal.xyz|depth), asynchronous on `hipStream`; outDev must not be one of the inputs.  Its two scratch images come
 * from hipMallocAsync / hipFreeAsync on that stream. */
typedef struct vcm_denoise_params { int passes; float sigmaColor, sigmaNormal, sigmaDepth; int demodulate; } vcm_denoise_params;
void vcm_denoise_defaults(vcm_denoise_params *out);               /* passes 5, demodulate 1, the sigmas DESIGN.md "Denoising" chose */
enum { VCM_FEATURE_ALBEDO = 0, VCM_FEATURE_NORMAL = 1, VCM_FEATURE_DEPTH = 2 };
int vcm_render_features(vcm_ctx *ctx);                            /* asynchronous on the context's stream; needs no iteration */
int vcm_read_feature(vcm_ctx *ctx, int which, float *host);       /* W*H*3 floats (albedo, normal) or W*H (depth) */
int vcm_features_device(vcm_ctx *ctx, void **albedoDev, void **guideDev);   /* the two W*H float4 images */
int vcm_denoise(vcm_ctx *ctx, float scale, const vcm_denoise_params *p);
int vcm_read_denoised(vcm_ctx *ctx, float *rgbHost);              /* W*H*3 floats */
int vcm_denoised_device(vcm_ctx *ctx, void **devPtr);             /* W*H float4 */
int vcm_read_denoised_image(vcm_ctx *ctx, int format, float gamma, unsigned char *outHost);  /* BGR8 / RGBE as vcm_read_image */
int vcm_denoise_buffers(int device, int width, int height, const void *colorDev, const void *albedoDev,
                        const void *guideDev, void *outDev, const vcm_denoise_params *p, void *hipStream);

/* ---- per-pixel variance of the running mean, and the noise statistic ----
 * The framebuffer is a running sum S_k over iterations and the iterations are independent samples of the image, so the
 * variance of the mean is accumulated BESIDE the framebuffer, without touching a rendering kernel: after iteration k's
 * resolve one kernel recovers the iteration's own frame x = S_k - S_{k-1} and applies Welford's update
 *   M2 += (x - S_{k-1} / (k - 1)) (x - S_k / k)      (M2 = 0 for k = 1)
 * per pixel and channel; the variance of the mean is V = M2 / (k (k - 1)), defined for k >= 2.  A non-finite sample leaves
 * M2 non-finite for that pixel and channel and nowhere else.
 * vcm_track_variance(ctx, 1) switches this on for a context whose framebuffer holds no iteration: a new context, or one
 * right after vcm_clear_framebuffer (which also resets the two images; k counts the iterations since then).  Off -- the
 * default -- costs nothing: no launch, no allocation, no byte.  Memory when on: two float4 images, 32 bytes per pixel
 * (134 MB at 2048^2), until vcm_destroy.  A sharded context is refused (its framebuffer is a shard of the image): such a
 * host reduces the frames itself and calls vcm_variance_update_buffers -- the same kernel on caller-owned images, no
 * context: sumDev3 = W*H*3 floats (the running sum after iteration k, k = 1, 2, ...), prevDev and momDev = n float4 each,
 * zeroed before k = 1; asynchronous on `hipStream`.
 * vcm_variance_device: the moments image { M2.rgb, 0 } (float4 per pixel); whoever reads it orders against the context's
 * stream.  vcm_read_variance: W*H*3 floats of V; fails with k < 2.
 * vcm_get_noise_stats reduces  noise = V / (mean^2 + 0.01),  mean = S_k / k,  over all pixels and channels: the
 * expectation of the relative squared error (img - ref)^2 / (ref^2 + 0.01) against a converged reference, with no
 * reference.  `above` counts the elements with noise > threshold; non-finite elements are counted in nonFinite and left
 * out of mean, max and above.  The reduction has no floating-point atomics, a fixed grid and a fixed combination tree
 * (binary64 sums): the same bits on every run.  It synchronises; it fails with k < 2.
 * CAVEAT: the statistic normalises by the noisy mean where the error metric normalises by the reference.  The two agree
 * where the mean is itself near converged (within 10 % on the sky-lit scene 3 after 16 iterations) and NOT where the
 * error is carried by fireflies: one bright sample F in k gives its pixel V = mean^2, so its noise saturates just below 1
 * whatever F is -- on scene 1 under path tracing the mean of the statistic is thirty times below the measured error
 * (DESIGN.md "Variance").  A host that renders such scenes to a target should watch `max` and `above` as well.
 *
 * The variance-guided filter.  vcm_denoise_params2 = vcm_denoise_params + { varianceGuided, sigmaVariance };
 * vcm_denoise2 / vcm_denoise_buffers2 with varianceGuided == 0 ARE vcm_denoise / vcm_denoise_buffers, bit for bit.  With
 * varianceGuided == 1 the colour stop of a tap is  |c_p - c_q|^2 / (sigmaVariance^2 v~_p + 1e-10)  instead of
 * |c_p - c_q|^2 / sigmaColor_i^2 (SVGF, Schied et al. 2017): v~_p is the 3 x 3 Gaussian of the centre's variance, which
 * rides in the colour image's .w -- sum over channels of V (/ albedo^2 when demodulating) before the first pass,
 * sum w_q^2 v_q / (sum w_q)^2 after every pass; sigmaColor then only serves pixels whose variance is not finite.
 * vcm_denoise2 takes the variance from the context (vcm_track_variance on, at least two iterations, else refused);
 * vcm_denoise_buffers2 takes a moments image { M2.rgb, 0 } and k, the colour being the mean S_k / k.
 * vcm_denoise_defaults2: vcm_denoise_defaults, varianceGuided 1, sigmaVariance 4 -- in the sweep of DESIGN.md "Variance"
 * the guided stop at 4 has a lower error than the fixed stop on all twelve cases, so the new call guides by default (and
 * so wants a tracked context); vcm_denoise and vcm_denoise_defaults stay what they were. */
typedef struct vcm_noise_stats { int iterations; long long elements, above, nonFinite; double mean, max; } vcm_noise_stats;
int vcm_track_variance(vcm_ctx *ctx, int on);
int vcm_variance_device(vcm_ctx *ctx, void **momDev);
int vcm_read_variance(vcm_ctx *ctx, float *rgbHost);
int vcm_get_noise_stats(vcm_ctx *ctx, float threshold, vcm_noise_stats *out);
int vcm_variance_update_buffers(int device, long long n, const void *sumDev3, int k, void *prevDev, void *momDev, void *hipStream);
int vcm_noise_stats_buffers(int device, long long n, const void *prevDev, const void *momDev, int k, float threshold,
                            vcm_noise_stats *out, void *hipStream);
typedef struct vcm_denoise_params2 {
    int passes; float sigmaColor, sigmaNormal, sigmaDepth; int demodulate;   /* as vcm_denoise_params */
    int varianceGuided; float sigmaVariance;
} vcm_denoise_params2;
void vcm_denoise_defaults2(vcm_denoise_params2 *out);
int vcm_denoise2(vcm_ctx *ctx, float scale, const vcm_denoise_params2 *p);   /* the result: vcm_read_denoised and its kin */
int vcm_denoise_buffers2(int device, int width, int height, const void *colorDev, const void *albedoDev, const void *guideDev,
                         const void *momDev, int k, void *outDev, const vcm_denoise_params2 *p, void *hipStream);

/* ---- the firefly-robust estimate: median of means over buckets of iterations, trimmed by their Gini coefficient ----
 * The plain mean S_k / k pays for one firefly -- a path that finds a small bright light -- for a long time.  Because the
 * iterations are independent samples x_k = S_k - S_{k-1} of the image, a robust estimate is accumulated BESIDE the
 * framebuffer, without touching a rendering kernel: iteration k (1, 2, ...: the iterations since the last clear, as the
 * variance counts them) adds x_k to bucket (k - 1) mod M of M partial framebuffers, M odd, 3 .. 15, and a resolve ranks the
 * M bucket means of every pixel and averages the central ones (Jung et al. 2015; Buisine et al. 2021, "G-MoN").  Per pixel,
 * with n_j = ceil((k - j) / M) the iterations in bucket j:
 *   m_j = B_j / n_j,  y_j = 0.212671 m_j.r + 0.715160 m_j.g + 0.072169 m_j.b;  buckets with a non-finite y_j are dropped,
 *   M' stay;  r_j = the number of kept buckets with a smaller key, or an equal key and a lower index;
 *   G = clamp(sum_j (2 (r_j + 1) - M' - 1) y_j / (M' sum_j y_j), 0, 1), 0 where sum_j y_j <= 0;
 *   t = min((M' - 1) / 2, floor(G M' / 2)) buckets are trimmed from each end of the ranking;
 *   rgb = sum of the kept B_j / sum of their n_j -- whole RGB triples, never channels separately.
 * Equal bucket means (G = 0) give the mean of all k iterations; where one bucket carries everything G nears 1 and the median
 * bucket alone remains.  A pixel with no finite bucket passes S_k / k through.  Needs k >= M.
 * vcm_track_robust(ctx, M) switches this on for a context whose framebuffer holds no iteration: a new context, or one right
 * after vcm_clear_framebuffer (which also zeroes the images); 0 switches it off.  Off -- the default -- costs nothing: no
 * launch, no allocation, no byte.  Memory when on: (M + 2) x 16 bytes per pixel -- the sum the last update saw, M bucket
 * planes and the result (9 x 16 = 144 B per pixel, 604 MB at 2048^2, for the default M = 7) -- until vcm_destroy.  Robust
 * tracking and vcm_track_variance are independent; either, both or neither may be on.  A sharded context is refused (its
 * framebuffer is a shard of the image): such a host reduces the frames itself and calls the _buffers twins, the same
 * kernels on caller-owned images, no context: sumDev3 = n * 3 floats (the running sum after iteration k), prevDev = n
 * float4, bucketsDev = M planes of n float4 each ([M][n]), all zeroed before k = 1, outDev = n float4 that is none of the
 * inputs; asynchronous on `hipStream`.
 * vcm_robust_resolve computes the estimate on the context's stream, asynchronously; vcm_read_robust resolves and copies
 * W*H*3 floats; vcm_robust_device resolves and gives the W*H float4 image { rgb, 1 }, fit for vcm_denoise_buffers'
 * colour input (whoever reads it orders against the context's stream).  Resolving changes no state: iterations may go on.
 * vcm_get_robust_stats reduces what the rule decided: `trimmed` counts the pixels with t > 0, `nonFinite` those with
 * M' < M, meanGini and maxGini are over all pixels.  No floating-point atomics, a fixed grid and the combination tree of
 * vcm_get_noise_stats: the same bits on every run.  It synchronises.
 * What it buys (DESIGN.md "Robust estimate", 64 x 64, the default M = 7): on scene 1 under path tracing, whose error is
 * carried by fireflies, an error 13 - 22 times below the mean's after 16 iterations and 4.5 - 5.5 times after 64; on scene
 * 3, which has none, an error 1.32 - 1.45 times the mean's after 16 iterations and 1.05 - 1.09 times after 64 (M = 5: 1.2
 * and 1.02, for a smaller gain at 64 iterations).  The estimate is biased where a pixel's distribution is skewed: it
 * converges to the mean only as the bucket means become equal.  M = 3 trims only where two buckets are at or below zero
 * (G >= 2 / 3): it is the mean almost everywhere. */
#define VCM_ROBUST_DEFAULT_BUCKETS 7
typedef struct vcm_robust_stats { int iterations, buckets; long long pixels, trimmed, nonFinite; double meanGini, maxGini; } vcm_robust_stats;
int vcm_track_robust(vcm_ctx *ctx, int buckets);      /* 0 = off (default: no launch, no allocation); odd 3..15 */
int vcm_robust_resolve(vcm_ctx *ctx);                 /* asynchronous on the context's stream; fails with k < buckets */
int vcm_read_robust(vcm_ctx *ctx, float *rgbHost);    /* W*H*3; resolves first */
int vcm_robust_device(vcm_ctx *ctx, void **devPtr);   /* W*H float4 {rgb, 1}: fit for vcm_denoise_buffers' colour input */
int vcm_get_robust_stats(vcm_ctx *ctx, vcm_robust_stats *out);   /* synchronises */
int vcm_robust_update_buffers(int device, long long n, const void *sumDev3, int k, int buckets, void *prevDev, void *bucketsDev, void *hipStream);
int vcm_robust_resolve_buffers(int device, long long n, const void *prevDev, const void *bucketsDev, int k, int buckets, void *outDev, void *hipStream);
int vcm_robust_stats_buffers(int device, long long n, const void *prevDev, const void *bucketsDev, int k, int buckets, vcm_robust_stats *out, void *hipStream);

/* ---- the technique breakdown: which part of the estimator carries a pixel ----
 * The framebuffer is the sum of five kinds of addends, and a tracked context keeps each kind in a plane of its own BESIDE
 * the framebuffer, without touching a rendering kernel: running sums over iterations with the framebuffer's meaning
 * (divide by the iteration count to get the image), which add up to the framebuffer up to the rounding of another order.
 *   VCM_PART_EMISSION     the camera path ends on an emitter or on the background (vertexcm.hxx:434-447, :468-479)
 *   VCM_PART_DIRECT       direct illumination of every camera vertex, MIS-weighted (:487-494)
 *   VCM_PART_CONNECT      the connections of camera vertices to light vertices (:498-526)
 *   VCM_PART_MERGE        the range merges (:530-538)
 *   VCM_PART_LIGHT_TRACE  the light vertices connected to the camera: the light splats (:380-384, :862-933)
 * The order of the additions is fixed (smallvcm_amd/csrc/vcm_parts.h "THE ORDER"): the planes are the same bits on every
 * run.  A plane an algorithm cannot fill stays exactly zero: light tracing fills LIGHT_TRACE alone, and it then equals the
 * framebuffer bit for bit; PPM and BPM fill EMISSION and MERGE; BPT leaves MERGE empty.
 * vcm_track_parts(ctx, 1) switches this on for a context whose framebuffer holds no iteration: a new context, or one right
 * after vcm_clear_framebuffer (which also zeroes the planes); 0 switches it off.  Off -- the default -- costs nothing: no
 * launch, no allocation, no byte.  Memory when on: 5 planes x 12 = 60 bytes per pixel (252 MB at 2048^2) until vcm_destroy,
 * and 16 more from the first vcm_part_device on.  Independent of vcm_track_variance and vcm_track_robust.  The split is
 * read from what wavefront mode keeps apart, so it is refused for a sharded context (its framebuffer is a shard of the
 * image), for VCM_ALGO_PATH_TRACE / VCM_ALGO_EYE_LIGHT (no technique split here) and for a context in strict order;
 * vcm_set_strict_order(ctx, 1) is refused while tracking is on, and vcm_begin_iteration fails with maxPathLength > 31 (the
 * iteration would not be wavefront).  The reads are refused before the first iteration, for a part outside 0..4 and for
 * a scale that is not finite.
 * vcm_get_parts_stats: luminance[i] = the sum over pixels of 0.212671 r + 0.715160 g + 0.072169 b of plane i, divided by
 * the iteration count; a pixel with a non-finite value in any plane is counted in nonFinite and left out of every sum.
 * Binary64, no floating-point atomics, a fixed grid and a fixed combination tree (that of vcm_get_noise_stats): the same
 * bits on every run.  It synchronises. */
#define VCM_PART_EMISSION 0
#define VCM_PART_DIRECT 1
#define VCM_PART_CONNECT 2
#define VCM_PART_MERGE 3
#define VCM_PART_LIGHT_TRACE 4
#define VCM_PART_COUNT 5
typedef struct vcm_parts_stats { int iterations; long long pixels, nonFinite; double luminance[VCM_PART_COUNT]; } vcm_parts_stats;
int vcm_track_parts(vcm_ctx *ctx, int on);
int vcm_read_part(vcm_ctx *ctx, int part, float scale, float *rgbHost);   /* W*H*3 floats = plane * scale; scale 1 gives the raw sums */
int vcm_part_device(vcm_ctx *ctx, int part, float scale, void **devPtr);  /* W*H float4 {rgb*scale, 1}, fit for vcm_denoise_buffers; valid until the next call */
int vcm_get_parts_stats(vcm_ctx *ctx, vcm_parts_stats *out);              /* synchronises */

/* ---- the display transform: auto-exposure, tone curves, bloom, sRGB ----
 * What turns a linear HDR image into one a screen can show, on the device.  The pipeline on the linear pixel c * scale:
 *   1 exposure    times m = (float)exp2(autoEV + exposureEV)
 *   2 bloom       (1 - s) E + s B, s = bloomStrength; B = an energy-preserving pyramid blur of bloomLevels levels (2 x 2
 *                 means down, the binomial [1 4 6 4 1] / 16 at every level, bilinear x 2 up, the levels' mean); no threshold.
 *                 bloomStrength 0 launches nothing.  A pixel with a non-finite channel enters the blur as 0 and stays
 *                 what it was.
 *   3 tone curve  VCM_CURVE_CLAMP identity | VCM_CURVE_REINHARD extended Reinhard on the luminance, white point
 *                 whitePoint | VCM_CURVE_ACES Narkowicz's fit | VCM_CURVE_HABLE Hable's filmic curve h(2x) / h(11.2); NaN
 *                 and negative channels enter a curve as 0, +Inf as 2^40; the result is clamped to [0, 1]
 *   4 transfer    VCM_TRANSFER_GAMMA c^(1 / gamma), as vcm_read_image | VCM_TRANSFER_SRGB the piecewise sRGB curve
 *   5 bytes       vcm_read_display_image only: truncation (byte)min(255, v * 255) as vcm_read_image, or with dither == 1
 *                 floor(v * 255 + d), d in [0, 1) an integer hash of (pixel index, channel, ditherSeed): unbiased
 *                 stochastic rounding, no state, the same bytes on every run
 * vcm_display_defaults reproduces vcm_read_image(BGR8, scale, 2.2) byte for byte: CLAMP, GAMMA 2.2, everything else off
 * (whitePoint 4, key 0.18, percentiles 0.10 / 0.95, minEV -16, maxEV 16, bloomLevels 5 are what switching a stage on uses).
 * autoExposure == 1 picks autoEV from a histogram of the log luminance Y = 0.2126 r + 0.7152 g + 0.0722 b of c * scale
 * (eight bins per octave over 2^-20 .. 2^12, 64-bit counts: the same on every run): the mean log2 luminance of the pixels
 * between the two percentiles goes to `key`, clamped to [minEV, maxEV].  Pixels with Y <= 0 or a non-finite Y are left
 * out and counted apart.  This reads 2 KB back and waits for the stream; everything else of vcm_display is asynchronous on
 * the context's stream.  Parameters out of range or not finite are refused with -1 (vcm_last_error says which).
 * vcm_display(ctx, source, scale, p): source VCM_DISPLAY_FRAMEBUFFER = the running sum * scale, VCM_DISPLAY_DENOISED /
 * VCM_DISPLAY_ROBUST = that image * scale (refused where vcm_denoise has not run / the robust estimate cannot be
 * resolved).  Refused for a sharded context: reduce the frame and call vcm_display_buffers.  The result stays with the
 * context until the next vcm_display: vcm_display_device gives the W*H float4 image { rgb in [0, 1], 1 }, vcm_read_display
 * W*H*3 floats, vcm_read_display_image the bytes -- VCM_IMAGE_BGR8 bottom-up as vcm_read_image, VCM_IMAGE_RGBA8 top-down
 * with alpha 255 (VCM_IMAGE_RGBE is refused: it is a linear format) -- and vcm_get_display_stats what the histogram saw
 * (all zero but multiplier and clipped without autoExposure) and `clipped`, the channels that reached 1.0 after the curve;
 * it synchronises.  Memory: 16 bytes per pixel, and about 16 more with bloom, from the first vcm_display to vcm_destroy.
 * vcm_display_buffers needs no context: colorDev holds width * height pixels of `channels` (3 or 4) floats on `device`,
 * outDev width * height float4 (16-byte aligned, not colorDev); scratch comes from hipMallocAsync / hipFreeAsync on the
 * stream.  With statsOut != NULL it fills *statsOut and synchronises the stream; with NULL and autoExposure 0 the host
 * does not wait. */
enum { VCM_CURVE_CLAMP = 0, VCM_CURVE_REINHARD = 1, VCM_CURVE_ACES = 2, VCM_CURVE_HABLE = 3 };
enum { VCM_TRANSFER_GAMMA = 0, VCM_TRANSFER_SRGB = 1 };
enum { VCM_DISPLAY_FRAMEBUFFER = 0, VCM_DISPLAY_DENOISED = 1, VCM_DISPLAY_ROBUST = 2 };
typedef struct vcm_display_params {
    int curve; float whitePoint;
    float exposureEV;
    int autoExposure; float key, lowPercentile, highPercentile, minEV, maxEV;
    int transfer; float gamma;
    float bloomStrength; int bloomLevels;
    int dither; unsigned int ditherSeed;
} vcm_display_params;
typedef struct vcm_display_stats {
    double autoEV, multiplier, logAvgLuminance;   /* logAvgLuminance: log2 of the trimmed geometric mean luminance */
    long long counted, zero, nonFinite, clampedLow, clampedHigh, clipped;
} vcm_display_stats;
void vcm_display_defaults(vcm_display_params *out);
int vcm_display(vcm_ctx *ctx, int source, float scale, const vcm_display_params *p);
int vcm_display_device(vcm_ctx *ctx, void **devPtr);              /* W*H float4 {rgb in [0, 1], 1} */
int vcm_read_display(vcm_ctx *ctx, float *rgbHost);               /* W*H*3 floats */
int vcm_read_display_image(vcm_ctx *ctx, int format, unsigned char *outHost);   /* BGR8: W*H*3 bytes, RGBA8: W*H*4 */
int vcm_get_display_stats(vcm_ctx *ctx, vcm_display_stats *out);  /* synchronises */
int vcm_display_buffers(int device, int width, int height, const void *colorDev, int channels, float scale,
                        const vcm_display_params *p, void *outDev, vcm_display_stats *statsOut, void *hipStream);

/* ---- image comparison: relMSE, PSNR, SSIM against a reference image ----
 * "How far is this image from that one", on the device: nothing is read back but 72 bytes of sums.  img = source * scale and
 * ref are linear RGB; d_c = img_c - ref_c in binary32, per pixel and channel:
 *   mse      the mean of d^2
 *   relMse   the mean of d^2 / (ref^2 + relEpsilon): the relative squared error the noise statistic estimates
 *   mae      the mean of |d|
 *   maxAbs   the largest |d|; maxPixel the index y * W + x of the pixel that holds it, the lowest on ties (-1 without one)
 *   psnr     10 log10(peak^2 / mse), computed on the host in binary64; +Inf for mse == 0
 *   above    the pixels whose largest per-channel d^2 / (ref^2 + relEpsilon) exceeds `threshold` (+Inf counts none)
 *   ssim     the mean SSIM (Wang et al. 2004) of the luminance Y = 0.212671 r + 0.715160 g + 0.072169 b of both images,
 *            clamped to [0, peak] and divided by peak: the 11 x 11 Gaussian window of sigma 1.5, C1 = 0.01^2, C2 = 0.03^2,
 *            moments in binary32.  Only the windows that lie wholly inside the image count, (W - 10) x (H - 10) at most:
 *            ssimWindows says how many, and ssim is NaN with none (every image narrower or lower than 11 pixels).  Identical
 *            images give exactly 1.  ssim == 0 in the parameters launches no window kernel: ssim NaN, ssimWindows 0.
 * A pixel with a non-finite channel in either image is counted in nonFinite and left out of every sum, of the maximum and
 * of every window that holds it (121 windows for a pixel well inside); without a counted pixel the means are NaN.  `pixels`
 * is W * H, `iterations` what the framebuffer held (0 from vcm_compare_buffers).  The sums are binary64 sums of binary32
 * terms over a fixed grid and a fixed combination tree, without floating-point atomics: the same bits on every run.
 * With writeMap == 1 the same kernels write the error map, W * H float4 { d^2 / (ref^2 + relEpsilon) of r, g, b; the SSIM
 * of the window centred on the pixel, or 0 where it has none or ssim is off }; a non-finite pixel's entry is all zero.
 * vcm_set_reference copies W*H*3 floats, row 0 = top, into the context (a non-finite texel is refused);
 * vcm_set_reference_device copies a W*H float4 device image on the context's stream (non-finite texels are allowed and
 * counted); NULL drops the reference.  vcm_envmap_load reads .pfm and .hdr files with rows top first: it is the loader for
 * reference images too (its limits: at most 8192 x 4096, finite, >= 0, not all black).  CAUTION: it takes a PFM's rows
 * bottom-up, as the format has them, while vcm_render -o x.pfm (like the reference's SavePFM) writes them top to bottom: such
 * a file comes out of vcm_envmap_load upside down, without an error, and a host turns its rows round before it hands them
 * to vcm_set_reference (vcm_render --reference does, for a name that ends in .pfm or .PFM).  With ssim == 1 a frame of more
 * than 524290 rows is refused (the SSIM kernel's grid): compare it with ssim 0.  vcm_compare(ctx, source, scale, p,
 * out): source as vcm_display's, with its refusals; it synchronises, because it returns numbers, and leaves the framebuffer
 * and every tracked image alone.  Refused with -1 (vcm_last_error says which): a NULL argument, no reference, a scale or a
 * parameter that is not finite (threshold may be +Inf), relEpsilon <= 0, peak <= 0, ssim or writeMap other than 0 / 1, and a
 * sharded context: reduce the frame and call vcm_compare_buffers.  Memory: nothing before the first vcm_set_reference, which
 * allocates 16 bytes per pixel; the first vcm_compare adds the partial sums (about 0.1 MB + 16 bytes per 256 windows), the
 * first with writeMap 16 bytes per pixel; until vcm_destroy.  vcm_compare_map_device / vcm_read_compare_map give the map of
 * the last vcm_compare with writeMap.  vcm_compare_buffers needs no context: images of 3 or 4 floats per pixel on `device`
 * (a float4 image 16-byte aligned), mapOutDev W*H float4 or NULL (it must be given with writeMap == 1, and be neither
 * input); scratch comes from hipMallocAsync / hipFreeAsync on the stream, which it synchronises. */
typedef struct vcm_compare_params { float relEpsilon, peak, threshold; int ssim; int writeMap; } vcm_compare_params;
typedef struct vcm_compare_stats  { int iterations; long long pixels, nonFinite, above, ssimWindows, maxPixel;
                                    double mse, relMse, mae, maxAbs, psnr, ssim; } vcm_compare_stats;
void vcm_compare_defaults(vcm_compare_params *out);              /* 0.01, 1, +Inf, ssim 1, writeMap 0 */
int  vcm_set_reference(vcm_ctx *ctx, const float *rgbHost);      /* W*H*3, row 0 = top, copied; NULL drops it */
int  vcm_set_reference_device(vcm_ctx *ctx, const void *float4Dev);
int  vcm_compare(vcm_ctx *ctx, int source, float scale, const vcm_compare_params *p, vcm_compare_stats *out);
int  vcm_compare_map_device(vcm_ctx *ctx, void **devPtr);        /* W*H float4, after a compare with writeMap */
int  vcm_read_compare_map(vcm_ctx *ctx, float *host4);           /* W*H*4 floats */
int  vcm_compare_buffers(int device, int width, int height, const void *imgDev, int imgChannels, float scale,
                         const void *refDev, int refChannels, const vcm_compare_params *p, void *mapOutDev /* or NULL */,
                         vcm_compare_stats *out, void *hipStream);

#ifdef __cplusplus
}
#endif
#endif /* SMALLVCM_AMD_H */
