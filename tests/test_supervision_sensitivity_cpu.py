"""Do the GPU cases of the supervision kernels discriminate?  On the CPU: tests/supervision_tiled.py restates
``cell_distance`` chunk by chunk and the blur tile by tile, and takes one named fault at a time.  The restatement goes
through the check helpers of tests/test_gpu_supervision.py -- the same operands, the same ``close`` / ``decisions`` calls
against tests/supervision_ref.py in fp32 and fp64 -- in place of the kernels.  Unfaulted it must pass every case, the
OLD ones (one chunk, one tile row: the cases the file had before supervision_regimes.py) and the NEW ones; each fault must
be rejected by at least one new case, and the faults that need a second chunk or a second tile row by no old case:

    fault                                    what gives it away
    last_chunk_dropped                       a ragged second chunk: value and gradients lose its pixels
    partials_indexed_chunk_major             two chunks, F > 1: the moments' gradient mixes frames
    mean_stops_at_256_partials               F = 130, two chunks: 4 of 260 partials missing from the value
    chosen_read_from_chunk_0                 two chunks: the second one's gradient goes to the first one's objects
    tail_lanes_live                          any ragged last chunk -- the OLD cases have one each and all reject it too:
                                             for this fault there was no gap
    bound_on_chunk_local_index               its variant that needs a second chunk (of 262 pixels: 1786 lanes counted
                                             at the last pixel); no old case can see it
    object_30_unreachable                    No = 31 (old cases stop at 16: they cannot see it either way)
    tile_row_halo_reflected_at_tile          H > 32: rows beside a tile seam
    column_pass_shifted_in_second_tile_row   H > 32: every row below the seam
    taps_beyond_23_dropped                   k = 31 (old cases stop at 23)

Each fault's test prints how many old and how many new cases reject it."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import supervision_regimes as SR  # noqa: E402
import supervision_tiled as T  # noqa: E402
import test_gpu_supervision as G  # noqa: E402

NEEDS_A_SECOND_WORKGROUP = {"last_chunk_dropped", "partials_indexed_chunk_major", "mean_stops_at_256_partials",
                            "chosen_read_from_chunk_0", "bound_on_chunk_local_index", "tile_row_halo_reflected_at_tile",
                            "column_pass_shifted_in_second_tile_row"}
# ``tail_lanes_live`` was thought to be among them and is not: the old 24 x 40 and 17 x 33 cases end in a ragged chunk
# too, and every one of them rejects it
CAUGHT_BY_EVERY_OLD_CASE = {"tail_lanes_live"}


# ---------------------------------------------------------------------------------------------------------------------
# the cases, as closures over the candidate
# ---------------------------------------------------------------------------------------------------------------------
def cell_cases():
    refs = SR.target_refs()[4]
    old, new = [], []
    for no, obj_shape, h, w in G.OLD_CELL_CASES:
        ops = G.old_cell_operands(refs, no, obj_shape, h, w)
        old.append(lambda fn, ops=ops, c=(no, obj_shape, h, w): G.check_cell(fn, *ops, c[1], f"old {c}"))
    tie = G.tie_operands(refs)
    old.append(lambda fn: G.check_cell_ties(fn, *tie))
    for case in SR.CELL_CASES:
        ops = SR.cell_inputs(*case, seed=SR.cell_seed(case))
        new.append(lambda fn, ops=ops, case=case: G.check_cell(fn, *ops, case[3], f"new {case}"))
    return old, new


def blur_cases():
    old = [lambda fn, c=c: G.check_blur(fn, G.old_blur_input(*c), 2.0, c[0], f"old blur {c}") for c in G.OLD_BLUR_CASES]
    new = [lambda fn, c=c: G.check_blur(fn, SR.blur_input(*c[:2]), c[3], c[2], f"new blur {c}", SR.blur_refs(*c))
           for c in SR.BLUR_CASES]
    return old, new


def target_cases():
    """The targets take a candidate BLUR: ``fn`` here is supervision_tiled.moving_object_target around it."""
    flow, lyt, lists, thresh, refs = SR.target_refs()
    old = [lambda fn, o=o: G.check_target(fn, flow, lyt, lists, thresh, refs, o, "old") for o in G.OPTION_SETS]
    new = []
    for h, w, e in SR.TARGET_CASES:
        args = SR.target_refs(h, w, e)
        for o in (SR.RECIPE_OPTS, SR.ALL_OPTS):
            new.append(lambda fn, a=args, o=o: G.check_target(fn, *a[:5], o, f"new {a[0].shape[-2:]} e={a[3]['edge_size']}"))
    return old, new


def rejections(cases, candidate):
    n = 0
    for case in cases:
        try:
            case(candidate)
        except AssertionError:
            n += 1
    return n


@pytest.fixture(scope="module")
def cell():
    return cell_cases()


@pytest.fixture(scope="module")
def blur():
    return blur_cases()


@pytest.fixture(scope="module")
def target():
    return target_cases()


# ---------------------------------------------------------------------------------------------------------------------
# without a fault
# ---------------------------------------------------------------------------------------------------------------------
def test_the_cell_restatement_passes_every_case(cell):
    for case in cell[0] + cell[1]:
        case(T.cell_distance(None))


def test_the_blur_restatement_passes_every_case(blur, target):
    for case in blur[0] + blur[1]:
        case(T.gaussian_blur(None))
    for case in target[0] + target[1]:
        case(T.moving_object_target(None))


def test_the_faults_are_the_named_ones_and_no_other_name_runs():
    assert set(T.CELL_FAULTS) == {"last_chunk_dropped", "partials_indexed_chunk_major", "mean_stops_at_256_partials",
                                  "chosen_read_from_chunk_0", "tail_lanes_live", "object_30_unreachable",
                                  "bound_on_chunk_local_index"}
    assert set(T.BLUR_FAULTS) == {"tile_row_halo_reflected_at_tile", "column_pass_shifted_in_second_tile_row",
                                  "taps_beyond_23_dropped"}
    assert NEEDS_A_SECOND_WORKGROUP | CAUGHT_BY_EVERY_OLD_CASE <= set(T.CELL_FAULTS) | set(T.BLUR_FAULTS)
    for make in (T.cell_distance, T.gaussian_blur, T.moving_object_target):
        with pytest.raises(AssertionError):
            make("tail_lanes_alive")


# ---------------------------------------------------------------------------------------------------------------------
# one fault at a time
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", list(T.CELL_FAULTS))
def test_the_new_cell_cases_reject_the_fault(cell, fault):
    old, new = (rejections(cases, T.cell_distance(fault)) for cases in cell)
    print(f"[sensitivity] {fault}: rejected by {old} of {len(cell[0])} old cases and {new} of {len(cell[1])} new cases")
    assert new >= 1
    if fault in NEEDS_A_SECOND_WORKGROUP:
        assert old == 0
    if fault in CAUGHT_BY_EVERY_OLD_CASE:
        assert old == len(cell[0])


@pytest.mark.parametrize("fault", list(T.BLUR_FAULTS))
def test_the_new_blur_cases_reject_the_fault(blur, target, fault):
    old, new = (rejections(cases, T.gaussian_blur(fault)) for cases in blur)
    told, tnew = (rejections(cases, T.moving_object_target(fault)) for cases in target)
    print(f"[sensitivity] {fault}: rejected by {old} of {len(blur[0])} old blur cases and {new} of {len(blur[1])} new "
          f"ones; inside the target by {told} of {len(target[0])} old cases and {tnew} of {len(target[1])} new ones")
    assert new >= 1
    if fault in NEEDS_A_SECOND_WORKGROUP:
        assert old == 0 and told == 0
