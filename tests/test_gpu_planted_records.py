"""K2 (the grid build: k_cell_keys / k_radix_hist / k_radix_scatter / k_cell_starts, the counting sort kept beside them, and
k_grid_merge_blocks of the sorted exchange) and K4 (k_merge_walk / k_merge_pairs) on PLANTED light vertices
(tests/planted_lib.py): one rank of a sharded HipBackend is fed a record set whose cells were chosen, Oracle(rank 0, world)
is fed the identical array, and box, cellStart, sortedIndex, the merge counters and the rank's framebuffer have to be the
oracle's bit for bit (HashGrid::Build, src/hashgrid.hxx:41-107; RangeQuery::Process, src/vertexcm.hxx:130-169).  Every case
first asserts, from the oracle's grid, that the pattern reached what it aimed at.

The launch-shape and sort switches are read once per process, so the device side of every case runs in a child process
(this file, run as a script): one child per environment, all of that environment's cases inside it, results back through
an .npz.  A child that ends by a signal or at its time limit fails every case of its environment; nothing is retried.
GPU only.  (The launch arithmetic alone, on the same cells: tests/test_planted_records.py.)"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import planted_lib as pl  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTERS = ("gridVertices", "mergeQueries", "mergeCandidates", "mergeAccepted")
MERGE_KERNEL_ID = {"walk": 2, "pairs": 3}     # VCM_MERGE_WALK / VCM_MERGE_PAIRS
INFO_MERGE_KERNEL, INFO_COUNT = 10, 11         # include/smallvcm_amd_debug.h
CAP_RES, CAP_WORLD = (16, 16), 2


# ---- the child: everything that touches the GPU ----------------------------------------------------------------------------
def _child(inp, outp):
    from smallvcm_amd.renderer import HipBackend
    d = np.load(inp)
    jobs = json.loads(str(d["jobs"]))
    out, ctxs = {}, []

    def backend(j):
        """a fresh context per job: the random numbers of an iteration follow the number of iterations the context has run"""
        b = HipBackend(pl.scene_of(j["res"]), j["algo"], j["radius_factor"], 0.75, 1234, device=0, rank=0, world=j["world"])
        if j["strict"]:
            b.set_strict_order(True)
        if j["kernel"]:
            b.set_merge_kernel(j["kernel"])
        b.L.vcm_debug_context_info.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        ctxs.append(b)
        return b

    def keep(i, r, b):
        info = (C.c_int * INFO_COUNT)()
        assert b.L.vcm_debug_context_info(b.ctx, info) == 0
        out["bbox_%d" % i], out["cs_%d" % i], out["idx_%d" % i], out["fb_%d" % i] = r["bbox"], r["cell_start"], r["sorted_index"], r["fb"]
        out["st_%d" % i] = np.array([r["stats"][k] for k in COUNTERS] + [info[INFO_MERGE_KERNEL]], np.int64)
        if "slab0" in r:
            out["slab0_%d" % i] = r["slab0"]

    for i, j in enumerate(jobs):
        while ctxs:
            ctxs.pop().close()
        if j["kind"] == "flow":
            b = backend(j)
            keep(i, pl.device_flow(b, d["recs_%d" % i]), b)
        elif j["kind"] == "capacity":
            import torch
            b = backend(j)
            full = d["recs_%d" % i]
            keep(i, pl.device_flow(b, full[:-1]), b)                      # exactly the capacity
            b.begin(0, 0, pl.MAX_LEN)
            b.trace_light()
            b.local_bbox()
            mn, mx = pl.box_of(full)
            b.set_grid_bbox([float(x) for x in mn], [float(x) for x in mx])
            dev = torch.from_numpy(full.ravel()).cuda()
            try:
                b.import_records(dev, [len(full), 0], len(full))           # one more
                out["refused_%d" % i] = np.array("accepted")
            except RuntimeError as e:
                out["refused_%d" % i] = np.array(str(e))
            r = pl.device_flow(b, d["after_%d" % i], iteration=1)          # the refusal ended the iteration: the next one opens
            for k in ("bbox", "cell_start", "sorted_index", "fb"):
                out["after_%s_%d" % (k, i)] = r[k]
            out["after_st_%d" % i] = np.array([r["stats"][k] for k in COUNTERS], np.int64)
        elif j["kind"] == "sorted":
            b = backend(j)
            W, n_cells = j["world"], j["res"][0] * j["res"][1]
            K = pl.sorted_block_cells(W)

            def rest(words, i=i, j=j, W=W, n_cells=n_cells, K=K):
                assert words == pl.slab_words(j["stride"], n_cells, K)
                return np.stack([pl.build_slab(d["recs_%d_%d" % (i, r)], d["cells_%d_%d" % (i, r)], j["stride"], n_cells, K)
                                 for r in range(1, W)])
            keep(i, pl.device_flow(b, slabs=(rest, j["counts"], j["stride"]), box=(d["box_%d" % i][:3], d["box_%d" % i][3:])), b)
        elif j["kind"] == "refuse65":
            b = HipBackend(pl.scene_of(j["res"]), j["algo"], j["radius_factor"], 0.75, 1234, device=0, rank=0, world=65)
            words = b.L.vcm_sorted_slab_words(b.ctx, 100)
            out["refuse65_%d" % i] = np.array("%d|%s" % (words, (b.L.vcm_last_error() or b"").decode()))
            b.close()
    while ctxs:
        ctxs.pop().close()
    np.savez(outp, **out)


# ---- the parent: sets, oracle, comparison ---------------------------------------------------------------------------------
def _sorted_scenarios():
    """rank 0: its own genuine records, sorted on the device.  The other ranks: records of rank 0 again (so every position
    lies in rank 0's box, which stays the box of the whole set), chosen by the cell the oracle gave them."""
    out = []
    for name, W in (("rank1_empty", 2), ("one_block_and_last_block", 3), ("count_equals_stride", 3), ("64_shards", 64)):
        sc = pl.scene_of(pl.RES)
        G = pl.genuine_records(sc, W)
        cells, _ = pl.cells_of(sc, W, G)
        n_cells, K = pl.RES[0] * pl.RES[1], pl.sorted_block_cells(W)
        last = (n_cells - 1) // K
        if name == "rank1_empty":
            rest = [G[:0]]
        elif name == "one_block_and_last_block":
            blk = int(np.bincount(cells[cells // K != last] // K).argmax())
            rest = [G[cells // K == blk], G[cells // K == last]]
        elif name == "count_equals_stride":
            rest = [pl.take(G, 2 * len(G)), G[::7].copy()]
        else:
            hot = pl.take(G, 3 * len(G))
            lo, hi = pl.hot_range(len(hot))
            hot[lo:hi, :3] = G[len(G) // 2, :3]
            rest = [G[:0]] * 62 + [hot]
        out.append({"name": name, "world": W, "ranks": [G] + rest, "K": K, "last": last})
    return out


def _jobs_of(env):
    """(jobs, arrays, expectations) of one environment"""
    jobs, arrays, expect = [], {}, []
    for c in pl.FLOW_CASES:
        if c["env"] != env:
            continue
        i = len(jobs)
        jobs.append(dict(c, kind="flow"))
        arrays["recs_%d" % i] = pl.case_records(c)
        expect.append(("flow", pl.case_id(c), c))
    if env == "":
        sc = pl.scene_of(CAP_RES)
        cap = (pl.MAX_LEN - 1) * CAP_RES[0] * CAP_RES[1]
        i = len(jobs)
        jobs.append(dict(pl._case("", "hot_middle", cap + 1, res=CAP_RES, world=CAP_WORLD), kind="capacity"))
        arrays["recs_%d" % i] = pl.hot_middle(sc, CAP_WORLD, cap + 1)
        arrays["after_%d" % i] = _capacity_oracle()[1]["recs"]
        expect.append(("capacity", "capacity", None))
        for s in _sorted_scenarios():
            i = len(jobs)
            counts = [len(r) for r in s["ranks"]]
            allrecs = np.concatenate(s["ranks"])
            o = pl.oracle_flow(pl.scene_of(pl.RES), pl.ALGO_BPM, s["world"], allrecs)
            base = np.concatenate(([0], np.cumsum(counts)))
            j = dict(pl._case("", "sorted:" + s["name"], len(allrecs), world=s["world"]), kind="sorted", counts=counts, stride=max(max(counts), 1))
            for r in range(1, s["world"]):
                arrays["recs_%d_%d" % (i, r)] = s["ranks"][r]
                arrays["cells_%d_%d" % (i, r)] = o["cells"][base[r]:base[r + 1]]
            arrays["box_%d" % i] = np.concatenate(pl.box_of(allrecs))
            jobs.append(j)
            expect.append(("sorted", s["name"], (s, o, counts, base)))
        jobs.append(dict(pl._case("", "refuse65", 0, world=65), kind="refuse65"))
        expect.append(("refuse65", "refuse65", None))
    return jobs, arrays, expect


_runs = {}


def _run(env):
    """the child of one environment, once; a failure is remembered, not retried"""
    if env not in _runs:
        jobs, arrays, expect = _jobs_of(env)
        tmp = tempfile.mkdtemp(prefix="planted_")
        inp, outp = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")
        np.savez(inp, jobs=np.array(json.dumps(jobs)), **arrays)
        e = dict(os.environ)
        for kv in env.split():
            k, v = kv.split("=", 1)
            e[k] = v
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), inp, outp], capture_output=True, text=True, timeout=600, env=e)
            if r.returncode != 0:
                raise AssertionError("child of %r ended with %d (negative: a signal)\n%s" % (env, r.returncode, r.stdout[-1000:] + r.stderr[-3000:]))
            got = dict(np.load(outp))
            _runs[env] = ({name: (i, kind, x) for i, (kind, name, x) in enumerate(expect)}, got, None)
        except (AssertionError, subprocess.TimeoutExpired) as err:
            _runs[env] = (None, None, repr(err) if isinstance(err, subprocess.TimeoutExpired) else str(err))
    index, got, failure = _runs[env]
    assert failure is None, failure
    return index, got


def _compare(got, i, o, what):
    assert np.array_equal(got["bbox_%d" % i].view(np.uint32), o["bbox"].view(np.uint32)), (what, "box")
    cs = got["cs_%d" % i]
    assert cs[0] == 0 and np.array_equal(cs[1:], o["cell_ends"]), (what, "cellStart")
    assert np.array_equal(got["idx_%d" % i], o["indices"]), (what, "sortedIndex")
    for k, v in zip(COUNTERS, got["st_%d" % i]):
        assert int(v) == o["stats"][k], (what, k, int(v), o["stats"][k])
    assert np.array_equal(got["fb_%d" % i].view(np.uint32), o["fb"].view(np.uint32)), (what, "framebuffer")


def _flow(case):
    o = pl.case_oracle(case)
    n_cells = case["res"][0] * case["res"][1]
    assert pl.reached(case["pattern"], o["cells"], n_cells), pl.case_id(case)          # reached, before anything is compared
    index, got = _run(case["env"])
    i, _, _ = index[pl.case_id(case)]
    _compare(got, i, o, pl.case_id(case))
    return got, i, o


@pytest.mark.parametrize("case", pl.TILE_CASES, ids=pl.case_id)
def test_one_workgroup_sorts_tiles_and_rounds(case):
    """grid_sort_blocks=1: the whole set is ONE workgroup's chunk of k_radix_scatter -- the tile loop and the carry of
    sGlobal from tile to tile (n > 2048), rounds 1 to 8 of a wave's running count, a last tile whose last waves are short or
    empty; wave shapes: 64 equal digits (one_cell), two interleaved groups of 32 (two_cells), ~64 different digits (spread)"""
    _flow(case)


@pytest.mark.parametrize("case", pl.ALGO_CASES, ids=pl.case_id)
def test_every_merging_algorithm_and_strict_order_see_the_planted_grid(case):
    """PPM, VCM and BPM in strict order (the camera kernel merges in place), one case per pattern"""
    _flow(case)


@pytest.mark.parametrize("case", pl.CHUNK_CASES, ids=pl.case_id)
def test_chunks_that_are_no_tile_multiple_and_empty_chunks(case):
    """3 and 7 workgroups (chunks of 1792 and 1536 entries: no tile multiple; with 5 records six of seven workgroups own
    nothing), and the default 64 workgroups over 17000 records (chunks of 512)"""
    _flow(case)


@pytest.mark.parametrize("case", pl.COUNT_CASES, ids=pl.case_id)
def test_counting_sort_builds_the_same_grid(case):
    """SMALLVCM_AMD_GRID_SORT=count: k_cell_count / scan / k_cell_scatter and the in-cell ranking of k_cell_rank_gather"""
    _flow(case)


@pytest.mark.parametrize("case", pl.EDGE_CASES, ids=pl.case_id)
def test_cell_starts_at_the_tables_edges(case):
    """k_cell_starts: a key equal to 0, a key equal to nCells - 1 (position n then starts one cell only), and empty stretches
    far longer than the 8 cells a lane fills alone -- with one, two and three radix passes (256, 4096 and 69632 cells)"""
    _flow(case)


@pytest.mark.parametrize("case", pl.DENSE_CASES, ids=pl.case_id)
def test_both_merge_kernels_equal_the_oracle_on_a_dense_cluster(case):
    """at least 64 queries that each accept at least 256 planted photons (the condition under which a step of k_merge_pairs
    accepts more pairs than its ring has room for), walk and pairs, each against the oracle"""
    q, m = pl.dense_queries(case)
    assert q >= 64 and m >= 256, (q, m)
    got, i, _ = _flow(case)
    assert int(got["st_%d" % i][-1]) == MERGE_KERNEL_ID[case["kernel"]]


_cap = []


def _capacity_oracle():
    """the same renderer twice: the full grid, then (the refused iteration never ended, so it does not count) a normal
    iteration on the rank's own records; the second frame is the sum of both, as on the device"""
    if not _cap:
        sc = pl.scene_of(CAP_RES)
        full = pl.hot_middle(sc, CAP_WORLD, (pl.MAX_LEN - 1) * CAP_RES[0] * CAP_RES[1] + 1)
        a = pl.oracle_flow(sc, pl.ALGO_BPM, CAP_WORLD, full[:-1])
        _cap.extend([a, pl.oracle_flow(sc, pl.ALGO_BPM, CAP_WORLD, None, iteration=1, o=a["o"])])
    return _cap


def test_capacity_is_exact_and_a_refusal_ends_the_iteration():
    """vcm_import_light_records takes the records of EVERY rank, so its capacity is (maxPathLength - 1) records per path of
    the frame: exactly that many are accepted and build the oracle's grid, one more is refused with "too many records", the
    refusal ends the iteration, and the next vcm_begin_iteration opens a normal one"""
    sc = pl.scene_of(CAP_RES)
    cap = (pl.MAX_LEN - 1) * CAP_RES[0] * CAP_RES[1]
    full = pl.hot_middle(sc, CAP_WORLD, cap + 1)
    o, after = _capacity_oracle()
    assert o["stats"]["gridVertices"] == cap and pl.reached_hot_middle(pl.cells_of(sc, CAP_WORLD, full[:-1])[0])
    index, got = _run("")
    i, _, _ = index["capacity"]
    _compare(got, i, o, "capacity")
    assert "too many records" in str(got["refused_%d" % i]), str(got["refused_%d" % i])
    assert after["stats"]["gridVertices"] > 0
    assert np.array_equal(got["after_bbox_%d" % i].view(np.uint32), after["bbox"].view(np.uint32))
    assert np.array_equal(got["after_cell_start_%d" % i][1:], after["cell_ends"]) and np.array_equal(got["after_sorted_index_%d" % i], after["indices"])
    for k, v in zip(COUNTERS, got["after_st_%d" % i]):
        assert int(v) == after["stats"][k], k
    assert np.array_equal(got["after_fb_%d" % i].view(np.uint32), after["fb"].view(np.uint32))


@pytest.mark.parametrize("name", ["rank1_empty", "one_block_and_last_block", "count_equals_stride", "64_shards"])
def test_sorted_exchange_places_planted_slabs(name):
    """k_grid_merge_blocks: rank 0's slab from vcm_sort_light_records, the others' from the numpy builder -- an empty rank, a
    rank whose records all lie in one block of cells, one whose records lie only in the last block, counts[1] ==
    strideRecords, 64 shards of which 62 are empty; grid and frame against the oracle fed the same records in rank order"""
    sc = [s for s in _sorted_scenarios() if s["name"] == name][0]
    counts = [len(r) for r in sc["ranks"]]
    base = np.concatenate(([0], np.cumsum(counts)))
    o = pl.oracle_flow(pl.scene_of(pl.RES), pl.ALGO_BPM, sc["world"], np.concatenate(sc["ranks"]))
    blocks = [np.unique(o["cells"][base[r]:base[r + 1]] // sc["K"]) for r in range(sc["world"])]
    if name == "rank1_empty":
        assert counts[1] == 0 and counts[0] > 0
    elif name == "one_block_and_last_block":
        assert counts[1] > 0 and len(blocks[1]) == 1 and counts[2] > 0 and list(blocks[2]) == [sc["last"]]
    elif name == "count_equals_stride":
        assert counts[1] == max(counts) > counts[0]
    else:
        assert sc["world"] == 64 and not any(counts[1:63]) and pl.reached_hot_middle(o["cells"][base[63]:])
    index, got = _run("")
    i, _, _ = index[name]
    _compare(got, i, o, name)
    n_cells = pl.RES[0] * pl.RES[1]
    want = pl.build_slab(sc["ranks"][0], o["cells"][:counts[0]], max(counts), n_cells, sc["K"])
    edges = max(counts) * pl.SORTED_WORDS + (n_cells + sc["K"] - 1) // sc["K"] + 1
    assert np.array_equal(got["slab0_%d" % i][:counts[0] * pl.SORTED_WORDS], want[:counts[0] * pl.SORTED_WORDS]), "rank 0's records, cell order"
    assert np.array_equal(got["slab0_%d" % i][max(counts) * pl.SORTED_WORDS:edges], want[max(counts) * pl.SORTED_WORDS:edges]), "block starts"


def test_65_shards_are_refused_by_the_sorted_exchange():
    index, got = _run("")
    i, _, _ = index["refuse65"]
    words, msg = str(got["refuse65_%d" % i]).split("|", 1)
    assert int(words) == -1 and "more than 64 shards" in msg, (words, msg)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
