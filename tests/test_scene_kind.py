"""The rule that picks a context's scene kind (smallvcm_amd/csrc/scene_kind.h, scene_kind_of) against the if-chain the
launch macros carried before the rule was stated once: all 32 combinations of the five facts, through the pure host entry
point vcm_debug_scene_kind.  No device."""
import ctypes as C
import itertools

import capacity_lib
from smallvcm_amd.renderer import load_library

KINDS = ("List", "Quads", "Rects", "Bvh", "BvhG", "RectsE", "ListE", "BvhE")   # enum class SceneKind, in order


def former_launch_chain(envMap, bvh, intPhong, rects, quads):
    """the nine-branch chain of the launch macro vcm_api.hip had before scene_kind.h, branch for branch: the source of truth"""
    if envMap:
        if bvh:
            return "BvhE"
        elif intPhong and rects:
            return "RectsE"
        else:
            return "ListE"
    elif bvh:
        if intPhong:
            return "Bvh"
        else:
            return "BvhG"
    elif not intPhong:
        return "List"
    elif rects:
        return "Rects"
    elif quads:
        return "Quads"
    else:
        return "List"


def former_context_info(envMap, bvh, intPhong, rects, quads):
    """(RECTS, QUADS, NODES) as vcm_debug_context_info computed them from the flags, before it read the stored kind"""
    return (int(not bvh and intPhong and rects), int(not bvh and not envMap and intPhong and not rects and quads), int(bvh))


def _kind(L, *facts):
    k = L.vcm_debug_scene_kind(*[C.c_int(int(f)) for f in facts])
    assert 0 <= k < len(KINDS), k
    return KINDS[k]


def _lib():
    L = load_library(require_gpu=False)
    L.vcm_debug_scene_kind.restype = C.c_int
    L.vcm_debug_scene_kind.argtypes = [C.c_int] * 5
    return L


def test_all_32_combinations_take_the_kind_the_launch_macro_took():
    L = _lib()
    reached = set()
    for facts in itertools.product((0, 1), repeat=5):
        got = _kind(L, *facts)
        assert got == former_launch_chain(*facts), (facts, got)
        reached.add(got)
    assert reached == set(KINDS), reached
    # any non-zero int is a true fact
    assert _kind(L, 7, 0, -1, 2, 0) == "RectsE"


def test_the_flags_read_off_the_kind_are_the_flags_the_accessor_computed():
    """vcm_debug_context_info reports RECTS / QUADS / NODES from the stored kind: for every combination (those a context
    cannot reach -- rectangles behind a BVH -- included) the values its former formula gave"""
    L = _lib()
    for facts in itertools.product((0, 1), repeat=5):
        k = _kind(L, *facts)
        from_kind = (int(k in ("Rects", "RectsE")), int(k == "Quads"), int(k in ("Bvh", "BvhG", "BvhE")))
        assert from_kind == former_context_info(*facts), (facts, k)


def test_the_rows_of_kind_flags_map_to_the_kinds_their_names_say():
    """capacity_lib.KIND_FLAGS = (rects, quads, nodes, intPhong, envMap) as the device tests assert them; the row of
    "rects" carries its environment map (SceneRectsE), and without it the scene takes SceneRects"""
    L = _lib()
    named = {"rects": "RectsE", "quads": "Quads", "list": "List", "bvh": "Bvh", "bvhG": "BvhG", "listE": "ListE", "bvhE": "BvhE"}
    assert set(named) == set(capacity_lib.KIND_FLAGS) == set(capacity_lib.KINDS) and len(named) == 7
    for name, (rects, quads, nodes, intPhong, envMap) in capacity_lib.KIND_FLAGS.items():
        assert _kind(L, envMap, nodes, intPhong, rects, quads) == named[name], name
    rects, quads, nodes, intPhong, _ = capacity_lib.KIND_FLAGS["rects"]
    assert _kind(L, 0, nodes, intPhong, rects, quads) == "Rects"


def test_the_two_precedence_cases():
    L = _lib()
    assert _kind(L, 1, 0, 1, 0, 1) == "ListE"    # env map + quads, no rectangles: no E kind of its own
    assert _kind(L, 1, 1, 1, 0, 0) == "BvhE"     # env map + BVH: one kind whatever the exponents
    assert _kind(L, 1, 1, 0, 0, 0) == "BvhE"
