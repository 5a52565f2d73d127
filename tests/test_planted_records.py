"""The planted record sets of tests/planted_lib.py on the CPU: every pattern reaches its case on the oracle at every size the
device test uses; the radix plan of tests/test_radix_plan.py, given the SAME cells the device gets, produces the oracle's
grid (HashGrid::Build, src/hashgrid.hxx:41-107); the numpy slab builder and the receiver's placement reproduce the
oracle's grid order for 2, 3 and 64 ranks, empty ranks included.  The device side: tests/test_gpu_planted_records.py."""
import time

import numpy as np
import pytest

import planted_lib as pl
from test_radix_plan import sort_cells


def _unique_sets(cases):
    seen, out = set(), []
    for c in cases:
        key = (c["pattern"], c["n"], c["res"], c["world"], c["radius_factor"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


SETS = _unique_sets(pl.FLOW_CASES)


@pytest.mark.parametrize("case", SETS, ids=pl.case_id)
def test_pattern_reaches_its_case_and_the_radix_plan_builds_the_oracles_grid(case):
    t0 = time.time()
    recs = pl.case_records(case)
    o = pl.case_oracle(case)
    wall = time.time() - t0
    n_cells = case["res"][0] * case["res"][1]
    cells = o["cells"]
    print("%s: %d records, %d accepted pairs, %d candidates, oracle + search %.2f s"
          % (pl.case_id(case), len(recs), o["stats"]["mergeAccepted"], o["stats"]["mergeCandidates"], wall))
    assert case["n"] is None or len(recs) == case["n"]
    assert len(o["cell_ends"]) == n_cells and cells.min() >= 0
    assert pl.reached(case["pattern"], cells, n_cells), pl.case_id(case)
    assert o["stats"]["mergeAccepted"] < 5_000_000                    # the oracle stays cheap
    assert np.array_equal(o["bbox"], np.concatenate(pl.box_of(recs)))   # the box the device is given is the oracle's, bit for bit
    order = np.argsort(cells, kind="stable")
    assert np.array_equal(o["indices"], order)                          # hashgrid.hxx:83-88
    for V in (1, 3, 7, 64):
        key, pay, cs = sort_cells(cells, n_cells, V)
        assert np.array_equal(pay, order), V
        assert np.array_equal(key, cells[order]), V
        assert cs[0] == 0 and np.array_equal(cs[1:], o["cell_ends"]), V


def test_dense_cases_aim_at_the_pair_rings_overflow():
    """the condition of the dense cluster cases, on the oracle: at least 64 queries that each accept at least 256 planted
    photons (tests/test_gpu_planted_records.py asserts the same before it compares)"""
    for case in pl.DENSE_CASES[::2]:
        q, m = pl.dense_queries(case)
        print("%s: %d queries accept the cluster of %d" % (pl.case_id(case), q, m))
        assert q >= 64 and m >= 256


@pytest.mark.parametrize("S,empty", [(2, (1,)), (3, ()), (3, (0, 2)), (64, tuple(range(1, 63))), (64, ())])
def test_slab_builder_round_trip_is_the_oracles_grid_order(S, empty):
    """a set split over S ranks (contiguous pieces, rank-major: the reference's vertex order), every rank's slab built by
    build_slab, placed as sharded_worker.SortedOracleBackend.import_sorted_records places them: the oracle's grid order"""
    case = pl._case("", "hot_middle", 4097)
    recs, o = pl.case_records(case), pl.case_oracle(case)
    n_cells, K = 64 * 64, pl.sorted_block_cells(S)
    full = [r for r in range(S) if r not in empty]
    cuts = np.linspace(0, len(recs), len(full) + 1).astype(int)
    pieces = {r: (cuts[i], cuts[i + 1]) for i, r in enumerate(full)}
    counts = [pieces[r][1] - pieces[r][0] if r in pieces else 0 for r in range(S)]
    stride = max(counts)
    ordered = np.concatenate([recs[pieces[r][0]:pieces[r][1]] for r in full])
    assert np.array_equal(ordered, recs)
    slabs, cells = [], []
    for r in range(S):
        lo, hi = pieces.get(r, (0, 0))
        slabs.append(pl.build_slab(recs[lo:hi], o["cells"][lo:hi], stride, n_cells, K))
        cells.append(np.sort(o["cells"][lo:hi], kind="stable"))
    assert counts.count(stride) >= 1 and all(len(s) == pl.slab_words(stride, n_cells, K) for s in slabs)
    placed, index, cell_start = pl.place_slabs(np.stack(slabs), counts, stride, cells, n_cells, K)
    assert np.array_equal(index, o["indices"])
    assert cell_start[0] == 0 and np.array_equal(cell_start[1:], o["cell_ends"])
    assert np.array_equal(pl.reference_order(placed, index), recs.view(np.uint32))
    assert np.array_equal(placed[:, :12], recs[o["indices"]].view(np.uint32)[:, :12])
