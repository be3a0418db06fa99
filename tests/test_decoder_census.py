"""The committed decoder path inputs (tests/decoder_inputs.py) reach every lane path of the device decoders
that tests/decoder_census.py names: each event in at least 3 different rows (the EG decoder's per-plane
events: at least once), the events argued unreachable never. No GPU: the census reads the oracle's streams
and row indices and restates the kernels' branch conditions; it also decodes every row and asserts that it
ends exactly at the row's last stream bit with the residual's 1s placed."""
import pytest

import decoder_census as dc
import decoder_inputs as di


@pytest.fixture(scope="module")
def counts(oracle):
    total = {}
    for name in di.PATH_INPUTS:
        P, cols = di.get(oracle, name)
        for pred in (0, 1):
            dc.census(oracle, P, cols, pred, total)
    print({e: total.get(e, 0) for e in dc.ALL_EVENTS})
    return total


def test_event_names(counts):
    assert set(counts) <= set(dc.ALL_EVENTS), set(counts) - set(dc.ALL_EVENTS)
    assert set(dc.UNREACHABLE) <= set(dc.ALL_EVENTS)
    assert len(set(dc.ALL_EVENTS)) == len(dc.ALL_EVENTS)


@pytest.mark.parametrize("event", [e for e in dc.ALL_EVENTS if e not in dc.UNREACHABLE])
def test_event_reached(counts, event):
    need = 1 if event in dc.PER_PLANE_EVENTS else 3
    assert counts.get(event, 0) >= need, (event, counts.get(event, 0))


@pytest.mark.parametrize("event", sorted(dc.UNREACHABLE))
def test_event_unreachable(counts, event):
    assert counts.get(event, 0) == 0, (event, dc.UNREACHABLE[event])


def test_input_limits(oracle):
    """path inputs stay small: rows <= 192, cols <= 4096, n <= 4, but for one 16384-column input"""
    wide = 0
    for name in di.PATH_INPUTS:
        P, cols = di.get(oracle, name)
        assert P.shape[0] <= 4 and P.shape[1] <= 192, name
        if cols > 4096:
            assert cols == 16384, name
            wide += 1
    assert wide == 1
    assert {di.get(oracle, n)[1] for n in di.PATH_INPUTS if di.family(n) == "widths"} == set(di.WIDTHS)


def test_census_sees_the_known_defect_rows(oracle):
    """the three rows of test_gpu_pbm.py::test_round_trip_first_row_run_across_word enter a stepped table
    step with (j >> 6) > ow (bic_decode.hip:530): what the defect of DESIGN.md §3 needed"""
    for seed in di.FIRST_ROW_SEEDS:
        c = {}
        dc.census_golomb(oracle, oracle.gen_plane(seed, 0.5, 1, 256)[None], 256, 0, c)
        assert c.get("g_stale_step_first_row") == 1, seed
