// scene_kind.h -- which instantiation of a ray-casting kernel a context launches, stated once.
//
// Kernels that cast rays exist once per kind of scene (vcm_core.h: SceneList ... SceneBvhE).  The kind follows from five
// facts about the scene (scene_kind_of); a context computes it once, when its scene is uploaded, and every launch, the
// feature kernel of the denoiser and vcm_debug_context_info read that value.  with_scene_kind turns it back into a type
// and adds the wrappers a kernel has instantiations for: WithLens (the kernels that hold the camera vertex, for a scene
// with a thin lens) and WithPick (the kernels that choose a light or weigh an emitter hit, for a scene with a light-pick
// table), WithPick over WithLens where a kernel has both, and WithLights over WithPick for a scene with a spot or a sphere
// light (such a scene always has a table, so WithLights exists over the WithPick kinds alone).  A scene with the Sobol
// sampler takes, in every kernel that draws (kWrapSobol), ONE kind per kind of scene: WithSobol over the widest chain
// of the other wrappers the kernel has, whatever else the scene holds; there lens, filter and table are run-time
// branches (vcm_core.h WithSobol).  Kernels that draw nothing are launched as without it.  A scene with a GGX lobe
// takes, in every kernel that handles a BSDF (kWrapGgx), WithGgx over that same widest chain, or over its WithSobol kind
// when the scene also asks for the Sobol sampler and the kernel draws: at most two kinds per kernel and kind of scene,
//     WithGgx<C>  and  WithGgx<WithSobol<C>>,   C = WidestChain<the kernel's lens / pick wrappers, S>::type.
#ifndef SMALLVCM_AMD_SCENE_KIND_H
#define SMALLVCM_AMD_SCENE_KIND_H

#include <type_traits>
#include "vcm_core.h"

namespace vcm {

enum class SceneKind : int { List = 0, Quads, Rects, Bvh, BvhG, RectsE, ListE, BvhE };

struct SceneFacts {
    bool envMap;     /* the background is an environment map */
    bool bvh;        /* the scene has BVH nodes */
    bool intPhong;   /* every Phong exponent in use is an integer detmath.h's binary exponentiation takes */
    bool rects;      /* the primitive list is one-plane triangle pairs, some of them axis-aligned rectangles */
    bool quads;      /* the primitive list is one-plane triangle pairs */
};

/* The rule.  An environment map comes first (its kinds carry the general pow, except the rectangles'), then a BVH, then
   the general pow, then rectangles before quads. */
constexpr SceneKind scene_kind_of(SceneFacts f)
{
    if (f.envMap) return f.bvh ? SceneKind::BvhE : (f.intPhong && f.rects) ? SceneKind::RectsE : SceneKind::ListE;
    if (f.bvh) return f.intPhong ? SceneKind::Bvh : SceneKind::BvhG;
    if (!f.intPhong) return SceneKind::List;
    if (f.rects) return SceneKind::Rects;
    if (f.quads) return SceneKind::Quads;
    return SceneKind::List;
}

/* { envMap, bvh, intPhong, rects, quads }: the rows of KIND_FLAGS in tests/capacity_lib.py ... */
static_assert(scene_kind_of({ true, false, true, true, false }) == SceneKind::RectsE, "rects (with its environment map)");
static_assert(scene_kind_of({ false, false, true, false, true }) == SceneKind::Quads, "quads");
static_assert(scene_kind_of({ false, false, true, false, false }) == SceneKind::List, "list");
static_assert(scene_kind_of({ false, true, true, false, false }) == SceneKind::Bvh, "bvh");
static_assert(scene_kind_of({ false, true, false, false, false }) == SceneKind::BvhG, "bvhG");
static_assert(scene_kind_of({ true, false, false, false, false }) == SceneKind::ListE, "listE");
static_assert(scene_kind_of({ true, true, false, false, false }) == SceneKind::BvhE, "bvhE");
/* ... and the two precedence cases: quads without rectangles have no E kind of their own, a BVH under an environment
   map has one kind whatever the exponents */
static_assert(scene_kind_of({ true, false, true, false, true }) == SceneKind::ListE, "env map + quads");
static_assert(scene_kind_of({ true, true, true, false, false }) == SceneKind::BvhE, "env map + BVH + integer exponents");

constexpr bool scene_kind_is_bvh(SceneKind k) { return k == SceneKind::Bvh || k == SceneKind::BvhG || k == SceneKind::BvhE; }
constexpr bool scene_kind_is_rects(SceneKind k) { return k == SceneKind::Rects || k == SceneKind::RectsE; }

/* what with_scene_kind hands its callable: `typename decltype(tag)::type` is the kernel's scene argument */
template <class S> struct SceneTag { using type = S; };

/* the wrappers a kernel is instantiated for */
enum : unsigned { kWrapNone = 0, kWrapLens = 1, kWrapPick = 2, kWrapSobol = 4, kWrapGgx = 8 };

/* the wrappers a context launches with; lights implies pick (wrappers_valid) */
struct SceneWrappers { bool lens, pick, lights; bool sobol = false; bool ggx = false; };
constexpr bool wrappers_valid(SceneWrappers w) { return !w.lights || w.pick; }
static_assert(wrappers_valid({ false, false, false }) && wrappers_valid({ true, true, false }) && wrappers_valid({ false, true, true }),
              "what a scene without / with the spot and sphere lights launches");
static_assert(!wrappers_valid({ false, false, true }), "no WithLights kernel exists without the table");

/* the widest chain of wrappers a kernel of `Wrap` has over S: what WithSobol sits on */
template <unsigned Wrap, class S> struct WidestChain {
    using L = std::conditional_t<(Wrap & kWrapLens) != 0, WithLens<S>, S>;
    using type = std::conditional_t<(Wrap & kWrapPick) != 0, WithLights<WithPick<L>>, L>;
};
static_assert(std::is_same_v<WidestChain<kWrapLens | kWrapPick, SceneRects>::type, WithLights<WithPick<WithLens<SceneRects>>>>, "K3, the path tracer, strict K1");
static_assert(std::is_same_v<WidestChain<kWrapPick, SceneBvh>::type, WithLights<WithPick<SceneBvh>>>, "K1, k_connect_di");
static_assert(std::is_same_v<WidestChain<kWrapLens, SceneList>::type, WithLens<SceneList>>, "k_connect_camera, eye light");
static_assert(WithSobol<WidestChain<kWrapLens | kWrapPick, SceneListE>::type>::kSobol && WithSobol<WidestChain<kWrapLens | kWrapPick, SceneListE>::type>::kLens &&
              WithSobol<WidestChain<kWrapLens | kWrapPick, SceneListE>::type>::kPick && WithSobol<WidestChain<kWrapLens | kWrapPick, SceneListE>::type>::kLights &&
              WithSobol<WidestChain<kWrapLens | kWrapPick, SceneListE>::type>::kEnvMap, "the Sobol kind carries every branch");
static_assert(!WithLights<WithPick<WithLens<SceneRects>>>::kSobol && !SceneRects::kSobol, "no other kind draws from it");

/* the kinds of a scene with GGX lobes */
template <unsigned Wrap, class S> struct GgxChain {
    using C = typename WidestChain<Wrap & (kWrapLens | kWrapPick), S>::type;
    using philox = WithGgx<C>;
    using sobol = WithGgx<WithSobol<C>>;
};
static_assert(std::is_same_v<GgxChain<kWrapLens | kWrapPick | kWrapSobol | kWrapGgx, SceneRects>::philox, WithGgx<WithLights<WithPick<WithLens<SceneRects>>>>>, "K3, the path tracer, strict K1, k_kat");
static_assert(std::is_same_v<GgxChain<kWrapPick | kWrapSobol | kWrapGgx, SceneBvh>::sobol, WithGgx<WithSobol<WithLights<WithPick<SceneBvh>>>>>, "K1, k_connect_di under Sobol");
static_assert(std::is_same_v<GgxChain<kWrapGgx, SceneList>::philox, WithGgx<SceneList>>, "k_connect_vc");
static_assert(GgxChain<kWrapLens | kWrapPick, SceneListE>::sobol::kGgx && GgxChain<kWrapLens | kWrapPick, SceneListE>::sobol::kSobol &&
              GgxChain<kWrapLens | kWrapPick, SceneListE>::sobol::kLens && GgxChain<kWrapLens | kWrapPick, SceneListE>::sobol::kPick &&
              GgxChain<kWrapLens | kWrapPick, SceneListE>::sobol::kLights && GgxChain<kWrapLens | kWrapPick, SceneListE>::sobol::kEnvMap, "the GGX kind carries every branch");
static_assert(GgxChain<kWrapLens, SceneBvh>::philox::kGgx && !GgxChain<kWrapLens, SceneBvh>::philox::kSobol, "under Philox it holds no Sobol draw");
static_assert(!WithSobol<WithLights<WithPick<WithLens<SceneRects>>>>::kGgx && !SceneRects::kGgx && !DScene::kGgx, "no other kind holds the lobe");

template <unsigned Wrap, class S, class F> void with_wrappers(SceneWrappers w, F &f)
{
    if constexpr (Wrap & kWrapGgx) {
        if (w.ggx) {
            if constexpr (Wrap & kWrapSobol) { if (w.sobol) { f(SceneTag<typename GgxChain<Wrap, S>::sobol>{}); return; } }
            f(SceneTag<typename GgxChain<Wrap, S>::philox>{});
        } else with_wrappers<Wrap & ~kWrapGgx, S>(w, f);
    } else if constexpr (Wrap & kWrapSobol) {
        if (w.sobol) f(SceneTag<WithSobol<typename WidestChain<Wrap & ~kWrapSobol, S>::type>>{});
        else with_wrappers<Wrap & ~kWrapSobol, S>(w, f);
    } else if constexpr (Wrap & kWrapLens) {
        if (w.lens) with_wrappers<Wrap & ~kWrapLens, WithLens<S>>(w, f);
        else with_wrappers<Wrap & ~kWrapLens, S>(w, f);
    } else if constexpr (Wrap & kWrapPick) {
        if (w.pick && w.lights) f(SceneTag<WithLights<WithPick<S>>>{});
        else if (w.pick) f(SceneTag<WithPick<S>>{});
        else f(SceneTag<S>{});
    } else f(SceneTag<S>{});
}

/* Calls f once, with the tag of the instantiation a scene of `kind` takes.  Only the wrappers named in Wrap are ever
   applied, so f is instantiated for exactly the types the kernel exists for. */
template <unsigned Wrap, class F> void with_scene_kind(SceneKind kind, SceneWrappers w, F &&f)
{
    switch (kind) {
    case SceneKind::List:   return with_wrappers<Wrap, SceneList>(w, f);
    case SceneKind::Quads:  return with_wrappers<Wrap, SceneQuads>(w, f);
    case SceneKind::Rects:  return with_wrappers<Wrap, SceneRects>(w, f);
    case SceneKind::Bvh:    return with_wrappers<Wrap, SceneBvh>(w, f);
    case SceneKind::BvhG:   return with_wrappers<Wrap, SceneBvhG>(w, f);
    case SceneKind::RectsE: return with_wrappers<Wrap, SceneRectsE>(w, f);
    case SceneKind::ListE:  return with_wrappers<Wrap, SceneListE>(w, f);
    case SceneKind::BvhE:   return with_wrappers<Wrap, SceneBvhE>(w, f);
    }
}

} // namespace vcm

#endif
