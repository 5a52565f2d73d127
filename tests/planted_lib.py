"""Planted light vertices for K2 (HashGrid::Build, src/hashgrid.hxx:41-107) and K4 (RangeQuery::Process,
src/vertexcm.hxx:130-169): record sets whose CELLS are chosen, not met, so that a test can put the grid build's radix sort,
k_cell_starts, the range merge and the sorted exchange in front of key distributions a render never makes -- and say,
from the oracle's grid alone, that the case it aimed at was reached.  Test infrastructure; needs no GPU.

A set is made of the genuine merge records of an oracle light pass (Oracle.trace_light / .records): repeated, reordered
and re-positioned.  Only floats 0..2 (the position) are ever changed; every other field stays a value a light path
produced, so the merge arithmetic sees nothing non-finite.  A record's cell is never computed here: the set is imported
into the oracle, the oracle builds its grid, and the cell is read back (cells_of) -- the oracle is the reference for the
hash and the radius.

Also here, because both sides of the sorted exchange need it: the slab layout of vcm_sort_light_records /
vcm_import_sorted_light_records in numpy (build_slab / place_slabs), given the cells."""
import numpy as np

from oracle_lib import Oracle
from smallvcm_amd._abi import VCM_MERGE_RECORD_FLOATS

R = VCM_MERGE_RECORD_FLOATS
SCENE_ID = 1
MAX_LEN = 10                 # capacity: (MAX_LEN - 1) records per path of the FRAME (every rank's vertices are imported)
RADIUS_FACTOR = 0.01         # radius 0.022: a camera vertex of a 64 x 64 frame finds a planted position now and then
ALGO_PPM, ALGO_BPM, ALGO_VCM = 1, 2, 4
SORTED_WORDS = 13


# ---- the oracle side -------------------------------------------------------------------------------------------------
def oracle_for(scene, algo, world, radius_factor=RADIUS_FACTOR, rank=0):
    return Oracle(scene, algo, radius_factor=radius_factor, rank=rank, world=world)


_genuine_cache = {}


def genuine_records(scene, world, radius_factor=RADIUS_FACTOR, algo=ALGO_BPM, iteration=0):
    """the merge records rank 0's light pass really produces"""
    key = (int(scene.camera.resolution[0]), int(scene.camera.resolution[1]), world, radius_factor, algo, iteration)
    if key not in _genuine_cache:
        o = oracle_for(scene, algo, world, radius_factor)
        o.begin(iteration, 0, MAX_LEN)
        o.trace_light()
        _genuine_cache[key] = o.records()
    return _genuine_cache[key]


def cells_from_grid(cell_ends, indices):
    """record -> cell, read off HashGrid's two arrays (after Build, mCellEnds[c] is the END of cell c)"""
    counts = np.diff(np.concatenate(([0], cell_ends.astype(np.int64))))
    cells = np.full(len(indices), -1, np.int64)
    cells[indices] = np.repeat(np.arange(len(cell_ends), dtype=np.int64), counts)
    return cells


def oracle_flow(scene, algo, world, recs, radius_factor=RADIUS_FACTOR, iteration=0, camera=True, o=None):
    """begin, trace_light, import, build_grid, (trace_camera -- the oracle merges inline --, end) on Oracle(rank 0, world).
    The random numbers of an iteration follow the number of iterations the renderer has RUN (vertexcm.hxx:547), `iteration`
    only sets the radius: a fresh oracle (o = None) stands for a fresh context; pass `o` to go on with the same renderer.
    recs = None: the rank's own records of this light pass.  -> {cell_ends, indices, bbox, cells, stats, fb, radius, recs, o}"""
    if o is None:
        o = oracle_for(scene, algo, world, radius_factor)
    o.begin(iteration, 0, MAX_LEN)
    o.trace_light()
    if recs is None:
        recs = o.records()
    o.import_records(recs)
    o.build_grid()
    ce, idx, bbox = o.grid()
    out = {"cell_ends": ce, "indices": idx, "bbox": bbox, "cells": cells_from_grid(ce, idx), "radius": o.stats()["radius"], "recs": recs, "o": o}
    if camera:
        o.trace_camera()
        o.end()
        out["stats"] = o.stats()
        out["fb"] = o.framebuffer()
    return out


def cells_of(scene, world, recs, radius_factor=RADIUS_FACTOR):
    g = oracle_flow(scene, ALGO_BPM, world, recs, radius_factor, camera=False)
    return g["cells"], g


# ---- building sets ---------------------------------------------------------------------------------------------------
def take(genuine, n):
    """n records: the genuine ones, repeated as often as it takes"""
    assert len(genuine) > 0
    return genuine[np.arange(n) % len(genuine)].copy()


def box_of(recs):
    """the box HashGrid::Build takes over the records (hashgrid.hxx:47-61); the empty set keeps the start values"""
    if len(recs) == 0:
        return np.full(3, 1e36, np.float32), np.full(3, -1e36, np.float32)
    return recs[:, :3].min(axis=0).astype(np.float32), recs[:, :3].max(axis=0).astype(np.float32)


# The back wall of the Cornell box (scene.hxx:166-173: y = 1.30455, x in [-1.27, 1.29], z in [-1.28, 1.28]) faces the camera.
WALL_Y = np.float32(1.30455)
WALL_X = (-1.2, 1.2)
WALL_Z = (-1.2, 1.2)
WALL_EPS = np.float32(1e-3)
_anchor_cache = {}


def radius_of(scene, world, radius_factor):
    """the merge radius of iteration 0, as the oracle reports it"""
    return oracle_flow(scene, ALGO_BPM, world, take(genuine_records(scene, world, radius_factor), 1), radius_factor, camera=False)["radius"]


def cluster(genuine, n, centre, half):
    """n records inside ONE cell: all at `centre`, but the first at centre - half and the last at centre + half.
    HashGrid::Process drops a query that lies outside the box of the records (hashgrid.hxx:117-121), so records at one
    single point would never be merged with anything; with half < half a cell the box is smaller than a cell and the
    oracle puts every record into the same one."""
    recs = take(genuine, n)
    recs[:, :3] = centre
    if n >= 2:
        recs[0, :3], recs[-1, :3] = centre - half, centre + half
    return recs


def anchor(scene, world, radius_factor=RADIUS_FACTOR):
    """a position on the back wall that rank 0's camera vertices find: of a 9 x 9 lattice, the point where a cluster of 32
    planted photons is accepted most often by the oracle (which pixels a rank owns is the oracle's business, not restated)"""
    key = (int(scene.camera.resolution[0]), int(scene.camera.resolution[1]), world, radius_factor)
    if key not in _anchor_cache:
        g = genuine_records(scene, world, radius_factor)
        half = np.float32(0.9 * radius_of(scene, world, radius_factor))
        best, best_acc = None, -1
        for x in np.linspace(WALL_X[0], WALL_X[1], 9):
            for z in np.linspace(WALL_Z[0], WALL_Z[1], 9):
                at = np.array([x, WALL_Y, z], np.float32)
                acc = oracle_flow(scene, ALGO_BPM, world, cluster(g, 32, at, half), radius_factor)["stats"]["mergeAccepted"]
                if acc > best_acc:
                    best, best_acc = at, acc
        assert best_acc > 0, "no lattice point of the back wall is seen by rank 0"
        _anchor_cache[key] = best
    return _anchor_cache[key].copy()


def one_cell(scene, world, n, radius_factor=RADIUS_FACTOR):
    """all n records in one cell: n - 2 at one position on the back wall, the first and the last 0.45 cells to either side"""
    half = np.float32(0.9 * radius_of(scene, world, radius_factor))
    return cluster(genuine_records(scene, world, radius_factor), n, anchor(scene, world, radius_factor), half)


def two_cells(scene, world, n, radius_factor=RADIUS_FACTOR):
    """records alternate between two positions either side of the anchor that the oracle puts into different cells (with
    different low digits); the two positions span the box the queries have to lie in"""
    g = genuine_records(scene, world, radius_factor)
    at = anchor(scene, world, radius_factor)
    radius = radius_of(scene, world, radius_factor)
    for mult in (3.0, 5.0, 7.0, 9.0):
        h = np.array([0.5 * mult * radius, WALL_EPS, 0.5 * mult * radius], np.float32)
        recs = take(g, max(n, 2))
        recs[0::2, :3], recs[1::2, :3] = at - h, at + h
        cells, _ = cells_of(scene, world, recs, radius_factor)
        if cells[0] != cells[1] and (cells[0] & 255) != (cells[1] & 255):
            return recs[:n]
    raise AssertionError("no pair of positions in different cells")


def spread(scene, world, n, radius_factor=RADIUS_FACTOR):
    """consecutive records in different cells: a lattice of more than one cell size stepped across the back wall, row by
    row, a millimetre in front of and behind it in turn; the step is searched until the oracle's cells satisfy reached_spread"""
    g = genuine_records(scene, world, radius_factor)
    cell = 2.0 * radius_of(scene, world, radius_factor)
    for mult in (1.37, 1.61, 1.83, 2.09, 2.41):
        step = mult * cell
        per_row = int((WALL_X[1] - WALL_X[0]) / step)
        rows = int((WALL_Z[1] - WALL_Z[0]) / step)
        if per_row * rows < 64:
            continue
        k = np.arange(n) % (per_row * rows)
        recs = take(g, n)
        recs[:, 0] = (WALL_X[0] + (k % per_row) * step).astype(np.float32)
        recs[:, 1] = WALL_Y + WALL_EPS * (2 * (np.arange(n) & 1) - 1).astype(np.float32)   # (a box of no depth holds no query)
        recs[:, 2] = (WALL_Z[0] + (k // per_row) * step).astype(np.float32)
        cells, _ = cells_of(scene, world, recs, radius_factor)
        if reached_spread(cells):
            return recs
    raise AssertionError("no lattice step spreads the records")


def _by_cell(scene, world, n, radius_factor, descending):
    recs = take(genuine_records(scene, world, radius_factor), n)
    cells, _ = cells_of(scene, world, recs, radius_factor)       # a reordering keeps the box, so it keeps the cells
    order = np.argsort(cells, kind="stable")
    return recs[order[::-1] if descending else order].copy()


def descending(scene, world, n, radius_factor=RADIUS_FACTOR):
    """a genuine set from the highest cell to the lowest, and inside a cell from the last record to the first"""
    return _by_cell(scene, world, n, radius_factor, True)


def ascending(scene, world, n, radius_factor=RADIUS_FACTOR):
    return _by_cell(scene, world, n, radius_factor, False)


def hot_range(n):
    """the middle 70 % of the index range"""
    lo = (n * 15) // 100
    return lo, max(lo + 1, min(n, lo + (n * 70 + 99) // 100))


def hot_middle(scene, world, n, radius_factor=RADIUS_FACTOR, position=None):
    recs = take(genuine_records(scene, world, radius_factor), n)
    lo, hi = hot_range(n)
    recs[lo:hi, :3] = anchor(scene, world, radius_factor) if position is None else position
    return recs


def edge_min_gap(n_cells):
    """the empty stretch edge_cells asks for: 600 cells (ten wave-wide strides of k_cell_starts' fill), or a quarter of a
    table too small to have 600 empty cells at all (a 16 x 16 frame has 256)"""
    return min(600, n_cells // 4)


def edge_cells(scene, world, radius_factor=0.003, n_extra=60, seed=7):
    """at least one record in cell 0, one in cell nCells - 1, and a long stretch of empty cells: found by search.  Two
    corner records fix the box, so a candidate's cell does not depend on which other candidates are kept; the oracle
    gives every candidate's cell in one build; kept are one candidate of cell 0, one of the last cell and a few of the
    lowest eighth of the table."""
    g = genuine_records(scene, world, radius_factor)
    n_cells = int(scene.camera.resolution[0]) * int(scene.camera.resolution[1])      # vertexcm.hxx:406
    lo, hi = np.array([-1.25, -1.25, -1.25], np.float32), np.array([1.25, 1.3, 1.25], np.float32)
    rng = np.random.default_rng(seed)
    m = max(4096, 6 * n_cells)
    cand = take(g, m + 2)
    cand[2:, :3] = (lo + rng.random((m, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    cand[0, :3], cand[1, :3] = lo, hi
    cells, _ = cells_of(scene, world, cand, radius_factor)
    first, last = np.flatnonzero(cells[2:] == 0), np.flatnonzero(cells[2:] == n_cells - 1)
    low = np.flatnonzero((cells[2:] > 0) & (cells[2:] < n_cells // 8))
    assert len(first) and len(last), "no candidate in cell 0 / in the last cell"
    keep = np.concatenate(([0, 1], 2 + first[:2], 2 + last[:2], 2 + low[:n_extra]))
    keep = keep[rng.permutation(len(keep))]
    return cand[keep].copy()


PATTERNS = {"one_cell": one_cell, "two_cells": two_cells, "spread": spread, "descending": descending,
            "ascending": ascending, "hot_middle": hot_middle}


def make(pattern, scene, world, n=None, radius_factor=RADIUS_FACTOR):
    if pattern == "edge_cells":
        return edge_cells(scene, world)
    return PATTERNS[pattern](scene, world, n, radius_factor)


# ---- reach predicates: functions of the oracle's grid alone ----------------------------------------------------------
def reached_one_cell(cells):
    return len(cells) > 0 and int(np.bincount(cells).max()) == len(cells)


def reached_two_cells(cells):
    if len(cells) < 2:
        return len(cells) == 1
    a, b = cells[0::2], cells[1::2]
    return bool(np.all(a == a[0]) and np.all(b == b[0]) and a[0] != b[0] and (a[0] & 255) != (b[0] & 255))


def reached_spread(cells):
    """every aligned group of 64 consecutive records (one round of a wave of k_radix_scatter) holds at least 48 distinct
    low digits; a shorter tail: three quarters of its length"""
    n = len(cells)
    if n > 1 and np.any(cells[1:] == cells[:-1]):
        return False
    for g0 in range(0, n, 64):
        grp = cells[g0:g0 + 64] & 255
        if len(np.unique(grp)) < (48 * len(grp) + 63) // 64:
            return False
    return n > 0


def reached_descending(cells):
    return len(np.unique(cells)) > 1 and bool(np.all(np.diff(cells) <= 0))


def reached_ascending(cells):
    return len(np.unique(cells)) > 1 and bool(np.all(np.diff(cells) >= 0))


def reached_hot_middle(cells):
    lo, hi = hot_range(len(cells))
    hot = cells[lo:hi]
    rest = np.concatenate((cells[:lo], cells[hi:]))
    return bool(np.all(hot == hot[0])) and int(np.bincount(cells).argmax()) == int(hot[0]) and bool(np.any(rest != hot[0]))


def reached_edge_cells(cells, n_cells):
    used = np.unique(cells)
    return bool(used[0] == 0 and used[-1] == n_cells - 1 and int(np.diff(used).max()) - 1 >= edge_min_gap(n_cells))


def reached(pattern, cells, n_cells):
    if pattern == "edge_cells":
        return reached_edge_cells(cells, n_cells)
    return {"one_cell": reached_one_cell, "two_cells": reached_two_cells, "spread": reached_spread,
            "descending": reached_descending, "ascending": reached_ascending, "hot_middle": reached_hot_middle}[pattern](cells)


# ---- the slab layout of the sorted exchange (include/smallvcm_amd.h), given the cells ----------------------------------
def sorted_block_cells(S):
    """cells per block of the sorted exchange (smallvcm_amd/csrc/vcm_kernels.h sorted_block_cells)"""
    k, p = 4096 // max(S, 1), 16
    while p * 2 <= k and p < 1024:
        p *= 2
    return p


def slab_words(stride, n_cells, K):
    return (stride * SORTED_WORDS + (n_cells + K - 1) // K + 1 + 3) & ~3


def block_edges(n_cells, K):
    return np.minimum(np.arange((n_cells + K - 1) // K + 1, dtype=np.int64) * K, n_cells)


def build_slab(recs, cells, stride, n_cells, K):
    """one rank's slab: its records in cell order (stable: local vertex order inside a cell), word 12 = path length |
    local index << 8, behind them (at record `stride`) the start of every block of K cells; uint32 words"""
    n = len(recs)
    assert n <= stride and len(cells) == n
    slab = np.zeros(slab_words(stride, n_cells, K), np.uint32)
    cells = np.asarray(cells, np.int64)
    order = np.argsort(cells, kind="stable")
    w = np.ascontiguousarray(recs, np.float32)[order].view(np.uint32).copy().reshape(n, SORTED_WORDS)
    if n:
        w[:, 12] = (w[:, 12] & 0xff) | (order.astype(np.uint32) << 8)
    slab[:n * SORTED_WORDS] = w.ravel()
    edges = block_edges(n_cells, K)
    slab[stride * SORTED_WORDS:stride * SORTED_WORDS + len(edges)] = np.searchsorted(cells[order], edges, side="left").astype(np.uint32)
    return slab


def place_slabs(slabs, counts, stride, cells, n_cells, K):
    """the receiver: every record at cellStart[c] + (records of lower ranks in c) + (its place in its rank's run).
    slabs: [S, words] uint32; cells[r]: the cells of rank r's slab records, in slab order.
    -> (records in grid order [total, 13] uint32, index: grid position -> vertex index in rank-major order, cellStart)"""
    S = len(counts)
    base = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    total = int(base[-1])
    cnt = np.zeros((S, n_cells), np.int64)
    recs = []
    edges = block_edges(n_cells, K)
    for r in range(S):
        c = np.asarray(cells[r], np.int64)
        assert len(c) == counts[r] and np.all(np.diff(c) >= 0), "a slab is in cell order"
        assert np.array_equal(slabs[r, stride * SORTED_WORDS:stride * SORTED_WORDS + len(edges)].astype(np.int64),
                              np.searchsorted(c, edges, side="left")), "block starts"
        cnt[r] = np.bincount(c, minlength=n_cells) if counts[r] else 0
        recs.append(slabs[r, :counts[r] * SORTED_WORDS].reshape(counts[r], SORTED_WORDS))
    cell_start = np.concatenate(([0], np.cumsum(cnt.sum(axis=0))))                 # hashgrid.hxx:75-81
    before = np.cumsum(cnt, axis=0) - cnt                                             # records of lower ranks in the cell
    placed = np.zeros((total, SORTED_WORDS), np.uint32)
    index = np.zeros(total, np.int64)
    for r in range(S):
        c = np.asarray(cells[r], np.int64)
        local_start = np.concatenate(([0], np.cumsum(cnt[r])))
        i = np.arange(counts[r], dtype=np.int64)
        dst = cell_start[c] + before[r][c] + (i - local_start[c])
        placed[dst] = recs[r]
        index[dst] = base[r] + (recs[r][:, 12] >> 8)
    assert len(np.unique(index)) == total
    return placed, index, cell_start


def reference_order(placed, index):
    """the placed records back in the reference's order (rank-major vertex order), word 12 = the path length again"""
    ref = np.zeros_like(placed)
    ref[index] = placed
    ref[:, 12] &= 0xff
    return ref


# ---- one rank of a sharded HipBackend ----------------------------------------------------------------------------------
def device_flow(b, recs=None, iteration=0, slabs=None, box=None):
    """begin, trace_light, set_grid_bbox, import_records (recs) or import_sorted_records (slabs), build_grid, trace_camera,
    merge, end -- with the camera pass where ShardedVertexCM._start puts it when camera_before_grid allows.
    recs: the flat record array, imported as ONE segment of rank 0 and empty segments for the others.
    slabs: (make_rest(dev_slab_words) -> [S - 1, words] uint32, counts, stride): rank 0's slab is sorted on the device from
    its own light pass (vcm_sort_light_records), the others' are given; `box` is then the box of all of them.
    -> {cell_start, sorted_index, bbox, stats, fb[, slab0]}"""
    import torch
    with b.stream_context():
        b.begin(iteration, 0, MAX_LEN)
        b.trace_light()
        _, _, n_local = b.local_bbox()                      # (ShardedVertexCM._start: counts and boxes travel first)
        out = {}
        if slabs is None:
            mn, mx = box_of(recs)
            b.set_grid_bbox([float(x) for x in mn], [float(x) for x in mx])
            dev = torch.from_numpy(np.ascontiguousarray(recs, np.float32).ravel()).cuda() if len(recs) else b.new_tensor(R)
            stride = max(len(recs), 1)
            counts = [len(recs)] + [0] * (b.world - 1)
        else:
            make_rest, counts, stride = slabs
            assert n_local == counts[0] <= stride, (n_local, counts[0], stride)
            b.set_grid_bbox([float(x) for x in box[0]], [float(x) for x in box[1]])
            words = b.sorted_slab_words(stride)
            assert words > 0, b.L.vcm_last_error()
            dev = torch.zeros(words * b.world, dtype=torch.float32, device="cuda")
            b.sort_records(dev[:words], stride)
            rest = make_rest(words)
            if b.world > 1:
                dev[words:] = torch.from_numpy(np.ascontiguousarray(rest).view(np.float32).ravel()).cuda()
            out["slab0"] = dev[:words].cpu().numpy().view(np.uint32)
        early = b.camera_before_grid
        if early:
            b.trace_camera()
        if slabs is None:
            b.import_records(dev, counts, stride)
        else:
            b.import_sorted_records(dev, counts, stride)
        b.build_grid()
        if not early:
            b.trace_camera()
        b.merge()
        b.end()
        b.synchronize()
    cs, idx, bbox = b.grid()
    out.update(cell_start=cs, sorted_index=idx, bbox=bbox, stats=b.stats(), fb=b.framebuffer_sum())
    del dev
    return out


# ---- the cases (tests/test_planted_records.py reaches them on the oracle, tests/test_gpu_planted_records.py runs them) ---------
SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 8191)   # a wave's round, a quarter tile, a tile, two, four, +- 1
BIG = (2049, 4097, 8191)
ONE_BLOCK = "SMALLVCM_AMD_SHAPE=grid_sort_blocks=1"
RES, WORLD = (64, 64), 2


def _case(env, pattern, n, algo=ALGO_BPM, strict=False, res=RES, world=WORLD, radius_factor=RADIUS_FACTOR, kernel=None):
    return {"env": env, "pattern": pattern, "n": n, "algo": algo, "strict": strict, "res": tuple(res), "world": world,
            "radius_factor": radius_factor, "kernel": kernel}


def case_id(c):
    return "%s-%s-n%s-%dx%d-w%d-a%d%s%s" % (c["env"].replace("SMALLVCM_AMD_", "").replace("=", "_") or "default", c["pattern"], c["n"],
                                              c["res"][0], c["res"][1], c["world"], c["algo"], "-strict" if c["strict"] else "",
                                              "-" + c["kernel"] if c["kernel"] else "")


TILE_CASES = ([_case(ONE_BLOCK, p, n) for p in ("one_cell", "two_cells", "spread") for n in SIZES] +
              [_case(ONE_BLOCK, p, n) for p in ("descending", "hot_middle") for n in BIG] +
              [_case(ONE_BLOCK, "ascending", n) for n in (2049, 8191)])
ALGO_CASES = ([_case(ONE_BLOCK, p, 2049, algo=a) for p in ("one_cell", "two_cells", "spread", "descending", "hot_middle")
               for a in (ALGO_PPM, ALGO_VCM)] +
              [_case(ONE_BLOCK, p, 2049, strict=True) for p in ("one_cell", "two_cells", "spread", "descending", "hot_middle")] +
              [_case("", "edge_cells", None, algo=a, radius_factor=0.003) for a in (ALGO_PPM, ALGO_VCM)] +
              [_case("", "edge_cells", None, strict=True, radius_factor=0.003)])
CHUNK_CASES = [_case(env, p, n) for env, n in (("SMALLVCM_AMD_SHAPE=grid_sort_blocks=3", 5000), ("SMALLVCM_AMD_SHAPE=grid_sort_blocks=7", 5),
                                               ("SMALLVCM_AMD_SHAPE=grid_sort_blocks=7", 9000), ("", 17000))
               for p in ("spread", "hot_middle")]
COUNT_CASES = [_case("SMALLVCM_AMD_GRID_SORT=count", p, n) for p in ("one_cell", "two_cells", "spread", "descending", "hot_middle")
               for n in (2049, 8191)]
EDGE_CASES = [_case("", "edge_cells", None, radius_factor=0.003),                              # 4096 cells: two passes
              _case("", "edge_cells", None, res=(16, 16), radius_factor=0.003),                # 256 cells: one pass
              _case("", "edge_cells", None, res=(272, 256), world=16, radius_factor=0.003)]    # 69632 cells: three passes
DENSE_RADIUS_FACTOR = 0.12        # queries accepting the whole cluster on the oracle: 21 at 0.05, 51 at 0.08, 91 at 0.12
DENSE_CASES = [_case("", p, 8191, radius_factor=DENSE_RADIUS_FACTOR, kernel=k) for p in ("one_cell", "hot_middle") for k in ("walk", "pairs")]
FLOW_CASES = TILE_CASES + ALGO_CASES + CHUNK_CASES + COUNT_CASES + EDGE_CASES + DENSE_CASES

_scene_cache, _set_cache = {}, {}


def scene_of(res):
    from smallvcm_amd.renderer import cornell_scene
    if tuple(res) not in _scene_cache:
        _scene_cache[tuple(res)] = cornell_scene(SCENE_ID, res[0], res[1])
    return _scene_cache[tuple(res)]


def case_records(c):
    """the record set of a case (built once per pattern, size, frame and radius)"""
    key = (c["pattern"], c["n"], c["res"], c["world"], c["radius_factor"])
    if key not in _set_cache:
        sc = scene_of(c["res"])
        _set_cache[key] = (edge_cells(sc, c["world"], c["radius_factor"]) if c["pattern"] == "edge_cells"
                           else PATTERNS[c["pattern"]](sc, c["world"], c["n"], c["radius_factor"]))
    return _set_cache[key]


def case_oracle(c):
    return oracle_flow(scene_of(c["res"]), c["algo"], c["world"], case_records(c), c["radius_factor"])


def dense_queries(c):
    """(queries that accept the whole planted cluster, size of the fullest cell), from the oracle's counters and grid: all
    records of the cluster lie at ONE position, so a query accepts all of them or none, and taking all but one of them away
    lowers mergeAccepted by (cluster - 1) per such query"""
    recs = case_records(c)
    lo, hi = (1, len(recs) - 1) if c["pattern"] == "one_cell" else hot_range(len(recs))
    assert len(np.unique(recs[lo:hi, :3], axis=0)) == 1
    a = oracle_flow(scene_of(c["res"]), ALGO_BPM, c["world"], recs, c["radius_factor"])
    b = oracle_flow(scene_of(c["res"]), ALGO_BPM, c["world"], np.concatenate((recs[:lo + 1], recs[hi:])), c["radius_factor"])
    diff = a["stats"]["mergeAccepted"] - b["stats"]["mergeAccepted"]
    assert diff % (hi - lo - 1) == 0
    return diff // (hi - lo - 1), int(np.bincount(a["cells"]).max())
